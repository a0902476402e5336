"""The CPU oracle (oracle/stin_oracle.py) against the golden vectors produced by the
REFERENCE's own classes (oracle/make_golden.py) - runs on CPU, no GPU needed."""
import copy

import numpy as np
import pytest
import torch

from oracle import scatter_ops, stin_oracle
from _golden import MODEL_FIXTURES, ModelFixture, load_npz, rel_err


@pytest.mark.parametrize('name', MODEL_FIXTURES)
def test_oracle_model_matches_reference_fixture(name):
    fx = ModelFixture(name)
    net = stin_oracle.define_G(**fx.cfg)
    assert set(net.state_dict().keys()) == set(fx.state_dict.keys())
    net.load_state_dict(fx.state_dict)
    s = fx.sample()
    s.x = s.x.clone().requires_grad_(True)
    out = net(s)
    # same ops in the same order: bit-exact on the host that generated the fixture; another CPU's BLAS kernels may sum in a
    # different order (measured 1.2e-6 on the GPU boxes' EPYC hosts), hence a bound instead of torch.equal
    assert float((out - fx.out).abs().max()) <= 2e-5
    pred = stin_oracle.graph_forward(net, s)
    loss = stin_oracle.compute_loss(pred, s.color, weights=s.mask)
    assert float((pred - fx.pred).abs().max()) <= 2e-5
    assert abs(float(loss.detach()) - float(fx.loss)) <= 1e-6
    loss.backward()
    if fx.gx64 is None:
        assert rel_err(s.x.grad, fx.gx) < 1e-5
    else:
        # five graph levels: the reference's own fp32 input gradient lies 1.3e-5 (relative) from its fp64 run, so another CPU's
        # BLAS moves the fp32 comparison past 1e-5 (measured 5.4e-7 on the recording host, 1.8e-5 with MKL's AVX2 path, 2.3e-5
        # on an AMD EPYC host): the fp32 bar of this fixture is 5e-5.  Beside it, the oracle in fp64 against the reference's
        # fp64 run is independent of the host and far tighter (measured 0 / 9e-16).
        assert rel_err(s.x.grad, fx.gx) < 5e-5
        net64 = copy.deepcopy(net).double()
        s64 = fx.sample()
        s64.x, s64.color, s64.mask = s64.x.double().requires_grad_(True), s64.color.double(), s64.mask.double()
        out64 = net64(s64)
        stin_oracle.compute_loss(stin_oracle.graph_forward(net64, s64), s64.color, weights=s64.mask).backward()
        assert float((out64 - fx.out64).abs().max()) <= 1e-12
        assert rel_err(s64.x.grad, fx.gx64) < 1e-12
    # some grads are analytically zero (a bias in front of an instance norm): compare against the
    # fixture-wide gradient scale, not per tensor
    scale = max(float(g.abs().max()) for g in fx.grads.values())
    for k, p in net.named_parameters():
        assert float((p.grad - fx.grads[k]).abs().max()) < 2e-5 * scale, k


def test_oracle_train_step_adam_amsgrad():
    fx = ModelFixture('g7_train_step')
    net = stin_oracle.define_G(**fx.cfg)
    net.load_state_dict(fx.state_dict)
    opt = torch.optim.Adam(net.parameters(), lr=7e-5, weight_decay=0, amsgrad=True)
    s = fx.sample()
    loss = stin_oracle.compute_loss(stin_oracle.graph_forward(net, s), s.color, weights=s.mask)
    loss.backward()
    opt.step()
    # first Adam step = lr * g / (|g| + eps): ill-conditioned where g is rounding noise (e.g. the bias in
    # front of an instance norm has an analytically ZERO gradient), so compare only where |g| is resolved
    for k, v in net.state_dict().items():
        ok = fx.grads[k].abs() > 1e-6
        assert torch.allclose(v[ok], fx.state_dict_after[k][ok], rtol=0, atol=2e-7), k
        assert float((v - fx.state_dict_after[k]).abs().max()) <= 2 * 7e-5 + 1e-7, k


def test_oracle_per_op_fixtures():
    z = {k: torch.from_numpy(v) for k, v in load_npz('g4_per_op').items()}
    # norms
    x = z['norm.x']
    for tag, b in (('none', None), ('zeros', torch.zeros(60, dtype=torch.long)), ('eq', z['norm.b_eq']),
                   ('un', z['norm.b_un'])):
        xx = x.clone().requires_grad_(True)
        y = stin_oracle.fast_instance_norm(xx, b)
        assert torch.allclose(y, z['fin.%s.y' % tag], atol=1e-6), tag
        (y * torch.linspace(-1, 1, y.numel()).view_as(y)).sum().backward()
        assert torch.allclose(xx.grad, z['fin.%s.gx' % tag], atol=2e-5), tag
    for tag, b in (('none', None), ('un', z['norm.b_un'])):
        y = stin_oracle.single_batch_graph_norm(x, z['gn.weight'], z['gn.bias'], z['gn.mean_scale'], b)
        assert torch.allclose(y, z['gn.%s.y' % tag], atol=1e-6), tag
    # pooling: engineered ties + empty clusters (arg-first rule, zero fill)
    xv, trace = z['pool.x'], z['pool.trace']
    for kind in ('max', 'mean'):
        xx = xv.clone().requires_grad_(True)
        y = stin_oracle.pool(xx, trace, 5, kind)
        assert torch.equal(y, z['pool.%s.y' % kind])
        (y * torch.arange(1., 16.).view(5, 3)).sum().backward()
        assert torch.equal(xx.grad, z['pool.%s.gx' % kind])
    xx = z['unpool.x'].clone().requires_grad_(True)
    y = stin_oracle.unpool(xx, trace)
    assert torch.equal(y, z['unpool.y'])
    (y * torch.arange(1., 22.).view(7, 3)).sum().backward()
    assert torch.equal(xx.grad, z['unpool.gx'])
    assert torch.equal(stin_oracle.pool_batch(torch.tensor([0, 0, 0, 1, 1, 1, 1]), trace, 5), z['batch.pooled'])


def test_scatter_max_known_answers():
    """Hand-computed: first occurrence wins ties, empty -> value 0 / arg = len(src)."""
    src = torch.tensor([[1., 5.], [3., 5.], [3., 1.], [-2., -2.]], requires_grad=True)
    idx = torch.tensor([0, 0, 0, 2])
    out, arg = scatter_ops.scatter_max(src, idx, dim=0, dim_size=4)
    assert out.tolist() == [[3., 5.], [0., 0.], [-2., -2.], [0., 0.]]
    assert arg.tolist() == [[1, 0], [4, 4], [3, 3], [4, 4]]
    out.sum().backward()
    assert src.grad.tolist() == [[0., 1.], [1., 0.], [0., 0.], [1., 1.]]
    m = scatter_ops.scatter_mean(torch.tensor([[2.], [4.], [9.]]), torch.tensor([1, 1, 3]), dim=0, dim_size=5)
    assert m.view(-1).tolist() == [0., 3., 0., 9., 0.]
    mi = scatter_ops.scatter_mean(torch.tensor([3, 4, -7]), torch.tensor([0, 0, 1]), dim=0, dim_size=2)
    assert mi.tolist() == [3, -7]


def test_oracle_metrics_fixture():
    z = {k: torch.from_numpy(v) for k, v in load_npz('g8_metrics').items()}
    assert torch.allclose(stin_oracle.graph_laplace_variance(z['pred'], z['ei']), z['lap_var'], rtol=1e-6)
    assert torch.allclose(stin_oracle.graph_total_variation(z['pred'], z['ei']), z['tv'], rtol=1e-6)


def _g11_saved(z, tag):
    """The dict of a graphs/<scene>.pt file rebuilt from the fixture's file-content arrays."""
    def lst(prefix):
        out, i = [], 0
        while '%s.f.%s.%d' % (tag, prefix, i) in z:
            out.append(torch.from_numpy(z['%s.f.%s.%d' % (tag, prefix, i)]))
            i += 1
        return out
    vertices, edges, traces = lst('vertices'), lst('edges'), lst('traces')
    dil = []
    for lvl in range(len(edges)):
        sets, i = [], 0
        while '%s.f.dil.%d.%d' % (tag, lvl, i) in z:
            a = z['%s.f.dil.%d.%d' % (tag, lvl, i)]
            sets.append(torch.from_numpy(a) if a.shape[0] else [])
            i += 1
        dil.append(sets if sets else None)
    return {'vertices': vertices, 'edges': edges, 'traces': traces, 'dilated_edges': dil,
            'dilation_dists': [int(v) for v in z['%s.f.dilation_dists' % tag]]}


@pytest.mark.parametrize('tag,cropped', [('full', False), ('crop', True)])
def test_scene_reader_equals_the_reference_reader(tag, cropped, tmp_path):
    """scene_io against the reference's OWN ScanNetGraphColorDataSet.__getitem__ (fixture g11, generated by running it on
    these very file contents, CoordsNormalization included): full validation scene and training crop (the two trace
    conventions, datasets/scannetcolorgraph_dataloader.py:124-128), the empty-dilation fall-back (:143-145)."""
    from surface_texture_inpainting_net_amd.scene_io import load_scene, sample_from_tensors
    import numpy as np
    z = load_npz('g11_scene_reader')
    saved = _g11_saved(z, tag)
    got = sample_from_tensors(saved, z['%s.f.vertex_mask' % tag], end_level=3, cropped=cropped)
    # ... and through real files in the on-disk schema
    gp, mp = str(tmp_path / 'scene.pt'), str(tmp_path / '7.npz')
    torch.save(saved, gp)
    np.savez(mp, vertex_mask=z['%s.f.vertex_mask' % tag])
    from_disk = load_scene(gp, mp, end_level=3, cropped=cropped)
    want = {k[len(tag) + 3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith(tag + '.s.')}
    assert len(want) >= 10
    for smp in (got, from_disk):
        for k, v in want.items():
            if k == 'num_vertices':
                assert smp[k].reshape(-1).tolist() == v.reshape(-1).tolist() and smp[k].dtype == torch.int32
            elif v.is_floating_point():
                assert smp[k].dtype == v.dtype and torch.equal(smp[k], v), k       # same operations in the same order: exact
            else:
                assert torch.equal(smp[k], v.to(smp[k].dtype)), k
        extra = set(smp.keys()) - set(want) - {'batch', 'name'}
        assert not extra, extra
    if tag == 'full':                                          # dist 8 was empty on disk: the reference reuses dist 4
        assert torch.equal(want['hierarchy_dil_8_edge_index_2'], want['hierarchy_dil_4_edge_index_2'])


def test_oracle_batchnorm_step_fixture():
    """norm='batch' through a REAL training step of the reference (fixture g12): its checkpointed encoder / bottleneck /
    decoder blocks run their forward twice, so their BatchNorm running statistics take the batch twice per step.  Fixture
    protocol: one forward-only call in train mode, then forward + loss + backward + Adam."""
    fx = ModelFixture('g12_batchnorm_step')
    net = stin_oracle.define_G(**fx.cfg)
    net.load_state_dict(fx.state_dict)
    net.train()
    s = fx.sample()
    out = net(s)
    assert float((out - fx.out).abs().max()) <= 1e-6
    opt = torch.optim.Adam(net.parameters(), lr=7e-5, weight_decay=0, amsgrad=True)
    loss = stin_oracle.compute_loss(stin_oracle.graph_forward(net, s), s.color, s.mask)
    loss.backward()
    assert abs(float(loss) - float(fx.loss)) <= 1e-6
    for k, p in net.named_parameters():
        assert float((p.grad - fx.grads[k]).abs().max()) <= 2e-6 + 1e-4 * float(fx.grads[k].abs().max()), k
    opt.step()
    sd = net.state_dict()
    counts = {k: int(v) for k, v in fx.state_dict_after.items() if k.endswith('num_batches_tracked')}
    assert sorted(set(counts.values())) == [2, 3], 'recomputed blocks count one more batch'
    for k, v in fx.state_dict_after.items():
        if k.endswith('num_batches_tracked'):
            assert int(sd[k]) == int(v), k
        elif 'running_' in k:
            assert float((sd[k] - v).abs().max()) <= 1e-6, k


def test_oracle_against_live_reference_random_config():
    """A fresh-seed config the other fixtures do not cover, against the reference's own forward recorded by
    oracle/make_golden.py (fixture g14: the reference's seed-1234 weights, synthetic mesh seed 99)."""
    import json
    from surface_texture_inpainting_net_amd.synthetic import make_synthetic_mesh
    z = load_npz('g14_live_reference')
    cfg = json.loads(bytes(z['cfg']).decode())
    assert cfg == dict(input_nc=10, output_nc=3, ngf=8, filter_type='edgeconvtransinv', norm='instance', n_blocks=3,
                       n_levels=2, pooling_type='max', dilations=[1, 2, 4], checkpoint_bottleneck=True)
    torch.manual_seed(1234)                     # = the reference's seeded weights (test below)
    net = stin_oracle.define_G(**cfg)
    s = make_synthetic_mesh(900, 3, seed=99, dilations=(2, 4))
    with torch.no_grad():
        out = net(s)
    want = torch.from_numpy(z['out'])
    assert out.shape == want.shape
    # bit-exact on the host that recorded the fixture (also with 1 or 3 threads); another CPU's BLAS may sum in a different
    # order, hence the bound of the other model fixtures instead of torch.equal
    assert float((out - want).abs().max()) <= 2e-5


def test_seeded_init_equals_reference_for_product_and_oracle():
    """Same torch seed -> the reference's define_G, the oracle's and the product's produce identical
    parameters (same construction order), for the shipped 3-D config (4 202 051 parameters): every state_dict entry's
    key, dtype, shape and sha256 against the reference's, recorded by oracle/make_golden.py (fixture g14)."""
    import hashlib
    import json
    import warnings
    from surface_texture_inpainting_net_amd import surfacetextureinpaintingnet as S
    want = json.loads(bytes(load_npz('g14_live_reference')['init_sha256']).decode())
    assert sum(int(np.prod(shape)) for _, _, shape, _ in want) == 4_202_051
    cfg = dict(input_nc=10, output_nc=3, ngf=64, filter_type='edgeconvtransinv', norm='instance', n_blocks=9,
               n_levels=2, pooling_type='max', dilations=[1, 1, 1, 2, 4, 8, 16, 1, 1], checkpoint_bottleneck=True)
    for mod in (stin_oracle, S):
        torch.manual_seed(49)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            sd = mod.define_G(**cfg).state_dict()
        got = [[k, str(v.dtype), list(v.shape), hashlib.sha256(v.detach().contiguous().numpy().tobytes()).hexdigest()]
               for k, v in sd.items()]
        assert [g[0] for g in got] == [w[0] for w in want], mod.__name__
        assert got == want, mod.__name__
