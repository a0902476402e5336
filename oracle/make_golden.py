"""Generate tests/golden/*.npz by RUNNING THE REFERENCE'S OWN CLASSES.

Runs only in the build container (needs /root/reference, read-only; nothing is
copied from it).  The reference's hot-path classes are imported under
oracle/pyg_shim (see oracle/ref_import.py); every expected output below is
produced by the reference's `define_G(...)`, `GraphResnetBlock`,
`FastInstanceNorm`, `SingleBatchGraphNorm`, `HierarchicalData.__inc__`,
`ImageGraphTextureDataSet`, `Inpainting3DTrainer._graph_forward/compute_loss`
and `utils.metrics.graph_metrics`.  Fixtures hold DATA only: inputs, seeded
weights, expected outputs / gradients.

    python oracle/make_golden.py            # rewrites tests/golden/
"""
import copy
import json
import os
import sys
import types
import warnings

import numpy as np
import torch

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _REPO)
warnings.filterwarnings('ignore')

from oracle import ref_import  # noqa: E402
from surface_texture_inpainting_net_amd.data import HierarchicalBatch  # noqa: E402
from surface_texture_inpainting_net_amd.synthetic import make_synthetic_mesh  # noqa: E402

OUT = os.path.join(_REPO, 'tests', 'golden')


def _np(t):
    return t.detach().cpu().numpy().copy()


def _randomize_biases(net, gen, scale=0.1):
    # the reference zero-inits every Linear bias; fixtures use non-zero biases so that
    # bias handling (incl. the b2 * [indeg > 0] mask) is actually pinned.
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=gen) * scale)


def _pack_sample(d, sample):
    for k in sample.keys():
        v = sample[k]
        if torch.is_tensor(v):
            d['s.' + k] = _np(v)


MAX_FILE_BYTES = 1 << 20      # no committed file above 1 MiB: a larger fixture is split into name.npz + name.part2.npz ...


def _save_npz(name, d):
    """np.savez_compressed(tests/golden/<name>.npz), split by key into parts of at most MAX_FILE_BYTES each when one file would be
    larger (tests/_golden.load_npz merges the parts)."""
    keys = list(d)
    for parts in range(1, len(keys) + 1):
        total = sum(d[k].nbytes for k in keys)
        groups, cur, acc = [], [], 0
        for k in keys:                                  # contiguous groups of about total / parts raw bytes
            if cur and acc + d[k].nbytes > total / parts * 1.05 and len(groups) < parts - 1:
                groups.append(cur)
                cur, acc = [], 0
            cur.append(k)
            acc += d[k].nbytes
        groups.append(cur)
        paths = [os.path.join(OUT, name + ('.npz' if i == 0 else '.part%d.npz' % (i + 1))) for i in range(len(groups))]
        for f in os.listdir(OUT):
            if f.startswith(name + '.part') and f.endswith('.npz'):
                os.remove(os.path.join(OUT, f))
        for path, g in zip(paths, groups):
            np.savez_compressed(path, **{k: d[k] for k in g})
        if all(os.path.getsize(path) <= MAX_FILE_BYTES for path in paths):
            return
    raise RuntimeError('%s: one array alone is larger than %d bytes compressed' % (name, MAX_FILE_BYTES))


def _fp64_run(net, T, sample):
    """The same forward + loss + backward with the network and the float inputs in float64 -> (out, d loss / d x)."""
    net = copy.deepcopy(net).double()
    net.zero_grad(set_to_none=True)
    s = HierarchicalBatch(**sample._store)
    s.x, s.color, s.mask = sample.x.detach().double().requires_grad_(True), sample.color.double(), sample.mask.double()
    fake = types.SimpleNamespace(models={'graph': net}, criterion=torch.nn.L1Loss(reduction='none'))
    out = net(s)
    T.compute_loss(fake, T._graph_forward(fake, s, s.color), s.color, weights=s.mask).backward()
    return out, s.x.grad


def _model_fixture(name, stin, trainer_mod, cfg, sample, seed, adam_step=False, fp64=False):
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed + 1)
    net = stin.define_G(**cfg)
    _randomize_biases(net, gen)
    d = {'cfg': np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8)}
    for k, v in net.state_dict().items():
        d['sd.' + k] = _np(v)
    _pack_sample(d, sample)
    fake = types.SimpleNamespace(models={'graph': net}, criterion=torch.nn.L1Loss(reduction='none'))
    T = trainer_mod.Inpainting3DTrainer
    if fp64:                                    # out64 / gx64: the reference's float64 run of the same weights and sample
        out64, gx64 = _fp64_run(net, T, sample)
        d['out64'], d['gx64'] = _np(out64), _np(gx64)
    x = sample.x.clone().requires_grad_(True)
    sample.x = x
    out = net(sample)
    pred = T._graph_forward(fake, sample, sample.color)
    loss = T.compute_loss(fake, pred, sample.color, weights=sample.mask)
    opt = torch.optim.Adam(net.parameters(), lr=7e-5, weight_decay=0, amsgrad=True) if adam_step else None
    loss.backward()
    d['out'] = _np(out)
    d['pred'] = _np(pred)
    d['loss'] = _np(loss)
    d['gx'] = _np(x.grad)
    for k, p in net.named_parameters():
        d['g.' + k] = _np(p.grad)
    if adam_step:
        opt.step()
        for k, v in net.state_dict().items():
            d['sd1.' + k] = _np(v)
    sample.x = x.detach()
    _save_npz(name, d)
    print(name, 'N0 =', sample.x.shape[0], 'loss =', float(loss), 'params =',
          sum(p.numel() for p in net.parameters()))


def g1_imagegraph(stin, trainer_mod):
    """Config 1: the reference's own 32x32 grid-graph index maps + small edgeconv net."""
    ig = ref_import.load_imagegraph_dataset_class()
    ds = ig.ImageGraphTextureDataSet([], end_level=2, is_train=False, benchmark=False, img_size=32,
                                     crop_half_width=8, circle_radius=4)
    gen = torch.Generator().manual_seed(11)
    img = torch.rand(1024, 3, generator=gen) * 2 - 1
    mask = (torch.rand(1024, 1, generator=gen) < 0.25)
    s = HierarchicalBatch()
    s['x'] = torch.cat([img * ~mask, mask.float()], dim=-1)
    s['color'] = img
    s['mask'] = mask.long() * torch.randint(1, 17, (1024, 1), generator=gen)
    s['edge_index'] = torch.from_numpy(ds.edge_indices_list[0]).t().contiguous()
    s['hierarchy_edge_index_1'] = torch.from_numpy(ds.edge_indices_list[1]).t().contiguous()
    s['hierarchy_trace_index_1'] = torch.from_numpy(ds.traces_list[0])
    s['num_vertices'] = torch.tensor([[1024, 256]], dtype=torch.int32)
    s['batch'] = torch.zeros(1024, dtype=torch.long)
    cfg = dict(input_nc=4, output_nc=3, ngf=8, filter_type='edgeconv', norm='instance', n_blocks=2,
               n_levels=1, pooling_type='max')
    _model_fixture('g1_imagegraph_edgeconv', stin, trainer_mod, cfg, s, seed=101)


def g2_three_level(stin, trainer_mod):
    for pooling in ('max', 'mean'):
        s = make_synthetic_mesh(700, 3, seed=2, dilations=(2, 4))
        cfg = dict(input_nc=10, output_nc=3, ngf=8, filter_type='edgeconvtransinv', norm='instance',
                   n_blocks=3, n_levels=2, pooling_type=pooling, dilations=[1, 2, 4],
                   checkpoint_bottleneck=True)
        _model_fixture('g2_3level_transinv_%s' % pooling, stin, trainer_mod, cfg, s, seed=202)


def g3_batch_unequal(stin, trainer_mod):
    """Two UNEQUAL graphs collated with the reference's HierarchicalData.__inc__ rules."""
    du = ref_import.load_module('utils.data_utils')
    from torch_geometric.data import Batch
    graphs = [make_synthetic_mesh(300, 3, seed=31, dilations=()),
              make_synthetic_mesh(520, 3, seed=32, dilations=())]
    items, d_extra = [], {}
    for gi, g in enumerate(graphs):
        h = du.HierarchicalData(x=g.x, color=g.color, mask=g.mask, edge_index=g.edge_index)
        h.num_vertices = g.num_vertices.reshape(-1)
        for k in g.keys():
            if k.startswith('hierarchy_'):
                setattr(h, k, g[k])
        items.append(h)
        for k in g.keys():
            if torch.is_tensor(g[k]):
                d_extra['g%d.%s' % (gi, k)] = _np(g[k])
    b = Batch.from_data_list(items)
    s = HierarchicalBatch()
    for k in b.keys:
        s[k] = b[k]
    s['batch'] = b['batch']
    assert s.num_vertices.shape == (2, 3)
    cfg = dict(input_nc=10, output_nc=3, ngf=8, filter_type='edgeconvtransinv', norm='instance',
               n_blocks=2, n_levels=2, pooling_type='max')
    _model_fixture('g3_batch2_unequal', stin, trainer_mod, cfg, s, seed=303)
    np.savez_compressed(os.path.join(OUT, 'g3_graphs.npz'), **d_extra)


def g4_per_op(stin):
    gen = torch.Generator().manual_seed(404)
    d = {}
    s = make_synthetic_mesh(200, 2, seed=4, dilations=())
    ei = s.edge_index
    n = s.x.shape[0]
    ecf = ref_import.load_module('models.modules.edge_conv_filter')
    fin = ref_import.load_module('models.modules.fastinstancenorm')
    sbg = ref_import.load_module('models.modules.singlebatchgroupnorm')
    d['ei'] = _np(ei)
    half = n // 3
    batch_uneq = torch.cat([torch.zeros(half, dtype=torch.long), torch.ones(n - half, dtype=torch.long)])
    d['batch_uneq'] = _np(batch_uneq)
    for tag, cin, cout, batch in (('neq', 6, 8, None), ('eq', 8, 8, None), ('eqb', 8, 8, batch_uneq)):
        torch.manual_seed(410 + cin + cout)
        blk = stin.GraphResnetBlock(cin, cout, ecf.get_gcn_filter, fin.FastInstanceNorm, False, True)
        _randomize_biases(blk, gen)
        x = torch.randn(n, cin, generator=gen).requires_grad_(True)
        w = torch.randn(n, cout, generator=gen)
        y = blk(x, ei, batch)
        (y * w).sum().backward()
        d['blk_%s.x' % tag], d['blk_%s.w' % tag], d['blk_%s.y' % tag] = _np(x), _np(w), _np(y)
        d['blk_%s.gx' % tag] = _np(x.grad)
        for k, p in blk.named_parameters():
            d['blk_%s.sd.%s' % (tag, k)] = _np(p)
            d['blk_%s.g.%s' % (tag, k)] = _np(p.grad)
    # norms
    x = torch.randn(60, 5, generator=gen) * 2 + 1
    d['norm.x'] = _np(x)
    b_eq = torch.arange(60) // 30
    b_un = (torch.arange(60) >= 17).long()
    d['norm.b_eq'], d['norm.b_un'] = _np(b_eq), _np(b_un)
    fi = fin.FastInstanceNorm(5)
    for tag, b in (('none', None), ('zeros', torch.zeros(60, dtype=torch.long)), ('eq', b_eq), ('un', b_un)):
        xx = x.clone().requires_grad_(True)
        y = fi(xx, b)
        wv = torch.linspace(-1, 1, y.numel()).view_as(y)
        (y * wv).sum().backward()
        d['fin.%s.y' % tag], d['fin.%s.gx' % tag] = _np(y), _np(xx.grad)
    gn = sbg.SingleBatchGraphNorm(5)
    with torch.no_grad():
        gn.weight.copy_(torch.randn(5, generator=gen))
        gn.bias.copy_(torch.randn(5, generator=gen))
        gn.mean_scale.copy_(torch.randn(5, generator=gen))
    d['gn.weight'], d['gn.bias'], d['gn.mean_scale'] = _np(gn.weight), _np(gn.bias), _np(gn.mean_scale)
    for tag, b in (('none', None), ('un', b_un)):
        xx = x.clone().requires_grad_(True)
        y = gn(xx, b)
        wv = torch.linspace(-1, 1, y.numel()).view_as(y)
        (y * wv).sum().backward()
        d['gn.%s.y' % tag], d['gn.%s.gx' % tag] = _np(y), _np(xx.grad)
        d['gn.%s.gweight' % tag] = _np(gn.weight.grad.clone())
        d['gn.%s.gmean_scale' % tag] = _np(gn.mean_scale.grad.clone())
        gn.zero_grad()
    # pooling through the reference's own _pooling/_unpooling methods (engineered ties, empty cluster)
    net_max = types.SimpleNamespace(_pooling_type='max')
    net_mean = types.SimpleNamespace(_pooling_type='mean')
    P = stin.SurfaceTextureInpaintingNet
    xv = torch.tensor([[1., 5., 2.], [3., 5., 2.], [3., 1., 2.], [0., 0., 7.], [-1., -2., -3.], [-1., -5., -3.],
                       [4., 4., 4.]])
    trace = torch.tensor([0, 0, 0, 2, 4, 4, 2])     # clusters 1 and 3 are empty; ties inside 0 and 4
    d['pool.x'], d['pool.trace'] = _np(xv), _np(trace)
    for tag, ns in (('max', net_max), ('mean', net_mean)):
        xx = xv.clone().requires_grad_(True)
        y = P._pooling(ns, xx, trace, 5)
        wv = torch.arange(1., 16.).view(5, 3)
        (y * wv).sum().backward()
        d['pool.%s.y' % tag], d['pool.%s.gx' % tag] = _np(y), _np(xx.grad)
    xx = torch.randn(5, 3, generator=gen).requires_grad_(True)
    y = P._unpooling(None, xx, trace)
    wv = torch.arange(1., 22.).view(7, 3)
    (y * wv).sum().backward()
    d['unpool.x'], d['unpool.y'], d['unpool.gx'] = _np(xx), _np(y), _np(xx.grad)
    # batch-vector propagation (models/surfacetextureinpaintingnet.py:421-422, :446-447)
    from torch_scatter import scatter_max
    bvec = torch.tensor([0, 0, 0, 1, 1, 1, 1])
    d['batch.pooled'] = _np(scatter_max(bvec, trace, dim=0, dim_size=5)[0])
    np.savez_compressed(os.path.join(OUT, 'g4_per_op.npz'), **d)
    print('g4_per_op', len(d), 'arrays')


def g5_sage(stin, trainer_mod):
    for ft in ('sageconv', 'sageconvtransinv'):
        s = make_synthetic_mesh(260, 2, seed=5, dilations=())
        cfg = dict(input_nc=10, output_nc=3, ngf=8, filter_type=ft, norm='instance', n_blocks=2, n_levels=1,
                   pooling_type='mean')
        _model_fixture('g5_%s' % ft, stin, trainer_mod, cfg, s, seed=505)


def g6_graphnorm(stin, trainer_mod):
    s = make_synthetic_mesh(260, 2, seed=6, dilations=())
    cfg = dict(input_nc=10, output_nc=3, ngf=8, filter_type='edgeconv', norm='graph', n_blocks=1, n_levels=1,
               pooling_type='max')
    _model_fixture('g6_graphnorm', stin, trainer_mod, cfg, s, seed=606)


def g7_train_step(stin, trainer_mod):
    s = make_synthetic_mesh(500, 3, seed=7, dilations=(2,))
    cfg = dict(input_nc=10, output_nc=3, ngf=8, filter_type='edgeconvtransinv', norm='instance', n_blocks=2,
               n_levels=2, pooling_type='max', dilations=[1, 2])
    _model_fixture('g7_train_step', stin, trainer_mod, cfg, s, seed=707, adam_step=True)


def g8_metrics():
    gm = ref_import.load_module('utils.metrics.graph_metrics')
    s = make_synthetic_mesh(300, 1, seed=8, dilations=())
    gen = torch.Generator().manual_seed(808)
    pred = torch.rand(s.x.shape[0], 3, generator=gen) * 2 - 1
    d = {'pred': _np(pred), 'ei': _np(s.edge_index),
         'lap_var': _np(gm.GraphLaplaceVariance()(pred, s.edge_index)),
         'tv': _np(gm.graph_total_variation(pred, s.edge_index)),
         'psnr': _np(gm.psnr(pred, s.color, data_range=2.0)), 'color': _np(s.color)}
    np.savez_compressed(os.path.join(OUT, 'g8_metrics.npz'), **d)


def _jittered_mesh(n_side, seed):
    """Small triangulated grid with jittered positions, noisy unit normals, permuted ids and shuffled edge order."""
    rng = np.random.default_rng(seed)
    idx = np.arange(n_side * n_side).reshape(n_side, n_side)
    e = list(zip(idx[:, :-1].ravel(), idx[:, 1:].ravel())) + list(zip(idx[:-1, :].ravel(), idx[1:, :].ravel())) + \
        list(zip(idx[:-1, :-1].ravel(), idx[1:, 1:].ravel()))
    e = np.array(e).T
    e = np.concatenate([e, e[::-1]], axis=1)
    perm = rng.permutation(n_side * n_side)
    e = perm[e]
    gx, gy = np.meshgrid(np.arange(n_side), np.arange(n_side), indexing='ij')
    pos = np.stack([gx.ravel(), gy.ravel(), np.zeros(n_side * n_side)], 1).astype(np.float64) + rng.normal(0, 0.2, (n_side * n_side, 3))
    p = np.empty_like(pos)
    p[perm] = pos
    nrm = rng.normal(0, 0.3, pos.shape)
    nrm[:, 2] += 1.0
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return e[:, rng.permutation(e.shape[1])].astype(np.int64), p, nrm


def g9_preprocessing():
    """Offline preprocessing either side of the path, outputs of the reference's OWN functions:
    graph_dilation.compute_all_node_dilated_edges on its dil_test toy graph (float32, the only known-answer candidate
    the reference holds) and on a jittered mesh (float64, as the pipeline calls it), and
    graph_level_generation.vertex_clustering on the same mesh."""
    gd, gl = ref_import.load_preprocessing()
    d = {}
    toy_e = np.array([[10, 9], [9, 10], [9, 6], [6, 9], [9, 7], [7, 9], [0, 7], [7, 0], [0, 8], [8, 0], [10, 0], [0, 10],
                      [10, 3], [3, 10], [3, 1], [1, 3], [10, 11], [11, 10], [11, 2], [2, 11], [11, 5], [5, 11], [5, 4], [4, 5],
                      [6, 4], [4, 6], [8, 12], [12, 8], [12, 13], [13, 12], [6, 14], [14, 6], [7, 14], [14, 7], [2, 15], [15, 2],
                      [5, 15], [15, 5], [2, 16], [16, 2], [1, 16], [16, 1], [2, 3], [3, 2], [3, 0], [0, 3], [4, 17], [17, 4],
                      [11, 17], [17, 11], [9, 17], [17, 9], [8, 13], [13, 8]], dtype=np.int64).T       # the toy graph of dil_test
    toy_x = np.array([[2, -1], [-2, -4], [-5, -1], [-2, -1.5], [0, 3], [-4, 3], [3, 3], [4, 3], [4, -3], [2, 2], [1, 1], [-3, 1],
                      [6, -2], [8, -3], [5, 4], [-7, 1], [-6, -4], [1, 2]], dtype=np.float32)
    toy_x = np.concatenate([toy_x, np.zeros((toy_x.shape[0], 1), np.float32)], 1)
    toy_n = np.zeros_like(toy_x)
    toy_n[:, 2] = 1.0
    d['toy_edge_index'], d['toy_pos'], d['toy_nrm'] = toy_e, toy_x, toy_n
    d['toy_dilations'] = np.array([2, 4, 6])
    for dil, out in zip((2, 4, 6), gd.compute_all_node_dilated_edges(toy_e, toy_x, toy_n, dilation=[2, 4, 6])):
        d['toy_d%d' % dil] = out.numpy()
    e, p, nrm = _jittered_mesh(16, 9)
    d['mesh_edge_index'], d['mesh_pos'], d['mesh_nrm'] = e, p, nrm
    d['mesh_dilations'] = np.array([2, 4, 8, 16])
    for dil, out in zip((2, 4, 8, 16), gd.compute_all_node_dilated_edges(e, p, nrm, dilation=[2, 4, 8, 16])):
        d['mesh_d%d' % dil] = out.numpy()
    adj = [[] for _ in range(p.shape[0])]
    for s, t in e.T:
        adj[s].append(int(t))
    nc, trace, _, edge_out = gl.vertex_clustering(p, adj, 2.5)
    d['vc_voxel'] = np.array(2.5)
    d['vc_coords'], d['vc_trace'] = nc, np.asarray(trace, dtype=np.int64)
    d['vc_edges'] = np.array(sorted(map(tuple, edge_out)), dtype=np.int64)       # the reference's order is a set order
    np.savez_compressed(os.path.join(OUT, 'g9_preprocessing.npz'), **d)
    print('g9_preprocessing', {k: v.shape for k, v in d.items() if k.startswith(('toy_d', 'mesh_d', 'vc_'))})


def g10_singleconvmeshnet():
    """the reference's own SingleConvMeshNet (BatchNorm1d inside the edge MLP, statistics over all
    edges) in training mode - output, loss, gradients, running statistics after the step - and in eval mode."""
    scmn = ref_import.load_singleconvmeshnet_module()
    for pooling in ('mean', 'max'):
        torch.manual_seed(1010)
        gen = torch.Generator().manual_seed(1011)
        net = scmn.SingleConvMeshNet(feature_number=10, num_propagation_steps=2, filter_sizes=[16, 32, 48], num_classes=3,
                                     pooling_method=pooling)
        with torch.no_grad():
            for m in net.modules():                       # non-trivial BN affine parameters and running statistics
                if isinstance(m, torch.nn.BatchNorm1d):
                    m.weight.copy_(1.0 + 0.2 * torch.randn(m.weight.shape, generator=gen))
                    m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=gen))
                    m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=gen))
                    m.running_var.copy_(1.0 + 0.2 * torch.rand(m.running_var.shape, generator=gen))
        s = make_synthetic_mesh(520, 3, seed=10, dilations=())
        d = {}
        _pack_sample(d, s)
        for k, v in net.state_dict().items():
            d['w/' + k] = _np(v)
        target = torch.randn(s.x.shape[0], 3, generator=gen)
        init_state = {k: v.clone() for k, v in net.state_dict().items()}
        net.train()
        with torch.no_grad():        # the reference's ResBlock adds IN PLACE into a ReLU output (singleconvmeshnet.py:104):
            out = net(s)             # legal for autograd in its torch era, rejected by torch 2.x -> forward only here
        loss = ((out - target) ** 2).mean()
        d['target'], d['out_train'], d['loss'] = _np(target), _np(out), _np(loss)
        for k, v in net.state_dict().items():
            if 'running' in k or 'num_batches' in k:
                d['after/' + k] = _np(v)
        net.eval()
        with torch.no_grad():
            d['out_eval'] = _np(net(s))
        # gradients: from the build's restatement (out-of-place residual add, otherwise op for op), after checking that
        # its training-mode forward reproduces the reference's output bit for bit
        from oracle import scmn_oracle
        rest = scmn_oracle.SingleConvMeshNet(feature_number=10, num_propagation_steps=2, filter_sizes=[16, 32, 48],
                                             num_classes=3, pooling_method=pooling)
        rest.load_state_dict(init_state)
        rest.train()
        out_r = rest(s)
        assert torch.equal(out_r.detach(), out), float((out_r.detach() - out).abs().max())
        ((out_r - target) ** 2).mean().backward()
        for k, p in rest.named_parameters():
            d['g_restatement/' + k] = _np(p.grad)
        np.savez_compressed(os.path.join(OUT, 'g10_singleconvmeshnet_%s.npz' % pooling), **d)
        print('g10_singleconvmeshnet', pooling, 'loss', float(loss), 'params', sum(p.numel() for p in net.parameters()))


def g11_scene_reader():
    """the reference's OWN reader.  A synthetic scene is written in the on-disk schema of
    preprocessing/graph_level_generation.py:492-536 (graphs/<scene>.pt, masks/<name>/<scene>/<id>.npz) and read back by
    ScanNetGraphColorDataSet.__getitem__ (datasets/scannetcolorgraph_dataloader.py:83-156, with the config's
    CoordsNormalization transform) - as a full validation scene and as a training crop (the two trace conventions,
    :124-128).  The fixture holds the file CONTENT (the saved tensors) and the sample the reference assembled from it."""
    import tempfile
    from surface_texture_inpainting_net_amd.scene_io import save_scene_like_reference
    mod = ref_import.load_scannet_color_dataset_module()
    import transform
    d = {}
    with tempfile.TemporaryDirectory() as root:
        for tag, is_train, dil in (('full', False, (2, 4, 8)), ('crop', True, (2,))):
            s = make_synthetic_mesh(350, 3, seed=11 + is_train, dilations=(2, 4) if not is_train else (2,))
            scene = 'scene0042_00' if not is_train else 'scene0042_00_3'
            os.makedirs(os.path.join(root, 'graphs'), exist_ok=True)
            os.makedirs(os.path.join(root, 'masks', 'rand', scene), exist_ok=True)
            gp = os.path.join(root, 'graphs', scene + '.pt')
            mp = os.path.join(root, 'masks', 'rand', scene, '7.npz')
            save_scene_like_reference(s, gp, mp, dilation_dists=dil)       # dist 8 empty -> the reader's fall-back (:143-145)
            saved = torch.load(gp, weights_only=False)
            if is_train:                                                    # crops carry no trace to the original mesh (:124-126)
                saved['traces'] = saved['traces'][1:]
                torch.save(saved, gp)
            ds = object.__new__(mod.ScanNetGraphColorDataSet)               # the index (glob over ScanNet split files) is not under test
            ds._root_dir, ds._mask_name, ds._end_level = root, 'rand', 3
            ds._is_train, ds._no_train_cropped = is_train, False
            ds._transform = [transform.CoordsNormalization([1.5, 1.5, 1.5])]
            ds._transform = (lambda ts: (lambda smp: [smp := t(smp) for t in ts][-1]))(ds._transform)
            ds.index2filenames = np.asarray([scene])
            ds.index2maskfilenames = [{7: '7.npz'}]
            smp = ds[0]
            assert smp.name == scene
            for k in smp.keys:
                v = smp[k]
                if torch.is_tensor(v):
                    d['%s.s.%s' % (tag, k)] = _np(v)
            for k in ('vertices', 'edges', 'traces'):
                for i, v in enumerate(saved[k]):
                    d['%s.f.%s.%d' % (tag, k, i)] = _np(v)
            for lvl, sets in enumerate(saved['dilated_edges']):
                if sets is not None:
                    for i, v in enumerate(sets):
                        d['%s.f.dil.%d.%d' % (tag, lvl, i)] = _np(v) if torch.is_tensor(v) else np.zeros((0, 2), dtype=np.int64)
            d['%s.f.dilation_dists' % tag] = np.asarray(saved['dilation_dists'])
            with open(mp, 'rb') as f:
                d['%s.f.vertex_mask' % tag] = np.load(f, allow_pickle=True)['vertex_mask']
    np.savez_compressed(os.path.join(OUT, 'g11_scene_reader.npz'), **d)
    print('g11_scene_reader', len(d), 'arrays')


def g12_batchnorm_step(stin, trainer_mod):
    """norm='batch' (models/surfacetextureinpaintingnet.py:236-241) through one REAL training step of the reference:
    forward + backward run the checkpointed encoder / bottleneck / decoder blocks twice (:429, :438, :451, :454), so their
    BatchNorm running statistics are updated twice and num_batches_tracked ends at 2 (bottleneck momentum sqrt(0.1),
    :496-499); the fixture's post-step state_dict (sd1.*) pins exactly that, plus output, loss, gradients, Adam update."""
    s = make_synthetic_mesh(420, 3, seed=12, dilations=(2,))
    cfg = dict(input_nc=10, output_nc=3, ngf=8, filter_type='edgeconvtransinv', norm='batch', n_blocks=2, n_levels=2,
               pooling_type='max', dilations=[1, 2], checkpoint_bottleneck=True)
    _model_fixture('g12_batchnorm_step', stin, trainer_mod, cfg, s, seed=1212, adam_step=True)


def g13_five_levels(stin, trainer_mod):
    """BASELINE config 5's DEPTH (n_levels=4: five graph levels, four pool / unpool pairs, encoder and decoder built per level -
    reference models/surfacetextureinpaintingnet.py:316-338) at fixture size: ngf 4 (widths 4 .. 64), two bottleneck blocks, the
    second on a dilated edge set of the coarsest level."""
    s = make_synthetic_mesh(3000, 5, seed=13, dilations=(2,))
    cfg = dict(input_nc=10, output_nc=3, ngf=4, filter_type='edgeconvtransinv', norm='instance', n_blocks=2, n_levels=4,
               pooling_type='max', dilations=[1, 2], checkpoint_bottleneck=True)
    _model_fixture('g13_5level', stin, trainer_mod, cfg, s, seed=1313, fp64=True)


def _sha256_state(sd):
    """[key, dtype, shape, sha256 of the bytes] per state_dict entry, in state_dict order."""
    import hashlib
    return [[k, str(v.dtype), list(v.shape), hashlib.sha256(v.detach().contiguous().cpu().numpy().tobytes()).hexdigest()]
            for k, v in sd.items()]


def g14_live_reference(stin):
    """What the two former side-by-side tests compared live: (a) the reference's forward of a fresh-seed random config on a
    synthetic mesh (seed 1234 weights, mesh seed 99), (b) the reference's seeded initialisation of the shipped 3-D config (seed
    49, 4 202 051 parameters) as one sha256 per state_dict entry."""
    from surface_texture_inpainting_net_amd.synthetic import make_synthetic_mesh as mesh
    cfg = dict(input_nc=10, output_nc=3, ngf=8, filter_type='edgeconvtransinv', norm='instance', n_blocks=3,
               n_levels=2, pooling_type='max', dilations=[1, 2, 4], checkpoint_bottleneck=True)
    torch.manual_seed(1234)
    ref = stin.define_G(**cfg)
    out = ref(mesh(900, 3, seed=99, dilations=(2, 4)))
    cfg3d = dict(input_nc=10, output_nc=3, ngf=64, filter_type='edgeconvtransinv', norm='instance', n_blocks=9,
                 n_levels=2, pooling_type='max', dilations=[1, 1, 1, 2, 4, 8, 16, 1, 1], checkpoint_bottleneck=True)
    torch.manual_seed(49)
    init = _sha256_state(stin.define_G(**cfg3d).state_dict())
    np.savez_compressed(os.path.join(OUT, 'g14_live_reference.npz'), out=_np(out),
                        cfg=np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8),
                        init_sha256=np.frombuffer(json.dumps(init).encode(), dtype=np.uint8))
    print('g14_live_reference', tuple(out.shape), len(init), 'state entries')


def param_counts(stin):
    """The structural constants SURVEY.md §8(c) records."""
    out = {}
    base = dict(output_nc=3, ngf=64, norm='instance', pooling_type='max')
    out['c1_edgeconv_nl1_nb9'] = sum(p.numel() for p in stin.define_G(
        input_nc=4, filter_type='edgeconv', n_blocks=9, n_levels=1, **base).parameters())
    for nl in (2, 3, 4):
        out['3d_transinv_nl%d_nb9' % nl] = sum(p.numel() for p in stin.define_G(
            input_nc=10, filter_type='edgeconvtransinv', n_blocks=9, n_levels=nl, **base).parameters())
    net = stin.define_G(input_nc=10, filter_type='edgeconvtransinv', n_blocks=9, n_levels=2, **base)
    out['3d_state_dict_keys'] = {k: list(v.shape) for k, v in net.state_dict().items()}
    with open(os.path.join(OUT, 'param_counts.json'), 'w') as f:
        json.dump(out, f, indent=1)
    print({k: v for k, v in out.items() if not isinstance(v, dict)})


def main():
    os.makedirs(OUT, exist_ok=True)
    stin = ref_import.load_model_module()
    trainer_mod = ref_import.load_trainer3d_module()
    if sys.argv[1:] == ['g13']:                 # (round 5: add the five-level fixture without rewriting the others)
        g13_five_levels(stin, trainer_mod)
        param_counts(stin)
        return
    g1_imagegraph(stin, trainer_mod)
    g2_three_level(stin, trainer_mod)
    g3_batch_unequal(stin, trainer_mod)
    g4_per_op(stin)
    g5_sage(stin, trainer_mod)
    g6_graphnorm(stin, trainer_mod)
    g7_train_step(stin, trainer_mod)
    g8_metrics()
    g9_preprocessing()
    g10_singleconvmeshnet()
    g11_scene_reader()
    g12_batchnorm_step(stin, trainer_mod)
    g13_five_levels(stin, trainer_mod)
    g14_live_reference(stin)
    param_counts(stin)


if __name__ == '__main__':
    main()
