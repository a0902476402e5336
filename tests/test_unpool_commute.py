"""A decoder block's first Linear on the COARSE rows in front of its unpool step (stin_net_op_t::y_from_src, functional.
USE_UNPOOL_COMMUTE): x_up[v] = x_c[trace[v]] makes every row of Y = x_up Wcat^T + bcat a copy of a row of Yc = x_c Wcat^T + bcat,
so the product runs on the coarse rows and the edge stage and the residual read Yc through the trace.  Nothing may change by a
bit: every comparison here is torch.equal, on the mapped kernels against their plain forms on gathered rows, on the products
at shapes where the coarse and the fine product take different GEMM kernels, and on the whole network with the switch on and off."""
import functools

import pytest
import torch

from surface_texture_inpainting_net_amd import _lib
from surface_texture_inpainting_net_amd import functional as SF
from surface_texture_inpainting_net_amd import surfacetextureinpaintingnet as S
from surface_texture_inpainting_net_amd.plan import EdgeSet, _ptr, _stream
from surface_texture_inpainting_net_amd.synthetic import make_synthetic_mesh

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N_FINE, N_COARSE = 777, 211


def _trace(n_fine, n_coarse, seed):
    """A fine -> coarse map with repeated coarse rows and with coarse rows nobody maps to (every 7th)."""
    g = torch.Generator().manual_seed(seed)
    used = torch.tensor([c for c in range(n_coarse) if c % 7 != 3])
    t = used[torch.randint(0, len(used), (n_fine,), generator=g)]
    t[:5] = t[5]                                                  # a run of equal entries as well
    assert len(torch.unique(t)) < n_coarse and len(torch.unique(t)) < n_fine
    return t.to(torch.int32).to(DEV)


def _graph_with_degrees(n, seed):
    """Edges whose in-degrees cycle through 0, 1, 5, 6, 7 and 13: no neighbour, one, either side of the 6 rows a 512-byte-row lane
    group requests per trip, and more than two trips."""
    g = torch.Generator().manual_seed(seed)
    degs = (0, 1, 5, 6, 7, 13)
    dst = torch.cat([torch.full((degs[v % 6],), v, dtype=torch.int64) for v in range(n)])
    dst = dst[torch.randperm(len(dst), generator=g)]
    src = torch.randint(0, n, (len(dst),), generator=g)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    es = EdgeSet(torch.stack([src, dst]).to(DEV), n, bad)
    deg = (es.by_dst.rowptr[1:] - es.by_dst.rowptr[:-1]).cpu()
    assert sorted(set(deg.tolist())) == sorted(degs) and int(bad.item()) == 0
    return es


@pytest.mark.parametrize('with_mask', [True, False])
@pytest.mark.parametrize('H', [128, 256, 512])
def test_mapped_edge_stage_equals_the_plain_stage_on_gathered_rows(H, with_mask):
    """stin_edge_relu_mean_fwd_map_f32 on [A | B | S] of the coarse rows against stin_edge_relu_mean_fwd_f32 on the gathered rows:
    hE with its indicator column and the ReLU mask words, all three lane layouts (32 lanes, 64 lanes, 64 lanes x 2 chunks)."""
    lib = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(H)
    ld = 2 * H + H // 2
    Yc = torch.randn(N_COARSE, ld, generator=g, device=DEV)
    trace = _trace(N_FINE, N_COARSE, H)
    Yf = Yc[trace.long()].contiguous()
    assert torch.equal(Yf[3], Yc[int(trace[3])])
    es = _graph_with_degrees(N_FINE, H + 1)
    csr = es.by_dst
    words = es.n_edges * (H // 32)

    def buffers():
        return (torch.zeros(N_FINE, H + 4, device=DEV), torch.zeros(words, dtype=torch.int32, device=DEV) if with_mask else None)
    h_ref, m_ref = buffers()
    SF.edge_relu_mean_fwd(Yf[:, :H], Yf[:, H:2 * H], csr, h_ref, indicator=True, mask=m_ref)
    h, m = buffers()
    rc = lib.stin_edge_relu_mean_fwd_map_f32(_ptr(Yc), ld, _ptr(Yc[:, H:]), ld, _ptr(csr.rowptr), _ptr(csr.col), _ptr(trace), N_FINE, H,
                                             _ptr(h), H + 4, 1, _ptr(m), _stream(Yc))
    assert rc == 0
    assert float(h_ref[:, :H].abs().max()) > 0 and set(h_ref[:, H].tolist()) == {0.0, 1.0}
    assert torch.equal(h, h_ref)
    if with_mask:
        assert int((m_ref != 0).sum()) > 0 and torch.equal(m, m_ref)


@pytest.mark.parametrize('C', [64, 128, 256])
def test_mapped_residual_norm_kernels_equal_the_plain_ones_on_a_gathered_residual(C):
    """stin_norm_act_res_fwd_map_f32 and stin_norm_act_res_fwd_fold_map_f32 read res[row_map[r]]: outputs (and the fold form's mean /
    rstd) equal the plain entry points on the gathered residual.  The residual is a column slice of wider rows, as in a block."""
    lib = _lib.load()
    N = N_FINE
    g = torch.Generator(device=DEV).manual_seed(C)
    x = torch.randn(N, C, generator=g, device=DEV) * 1.7 + 0.3
    wide = torch.randn(N_COARSE, C + 8, generator=g, device=DEV)
    res_c = wide[:, 4:4 + C]
    trace = _trace(N, N_COARSE, C)
    res_f = res_c[trace.long()].contiguous()
    inv = torch.full((1,), 1.0 / N, device=DEV)
    groups = 13
    cuts = torch.linspace(0, N, groups + 1).long().tolist()
    pm = torch.stack([torch.stack([x[a:b].double().sum(0), x[a:b].double().pow(2).sum(0)]) for a, b in zip(cuts, cuts[1:])]).contiguous()
    mean, rstd = SF.moments_final(pm, inv)
    # the elementwise launch: one graph, and rows of three graphs through gid
    gid = (torch.arange(N, device=DEV) * 3 // N).to(torch.int32)
    mean3 = torch.cat([mean, mean * 0.5, mean + 1.0]).contiguous()
    rstd3 = torch.cat([rstd, rstd * 2.0, rstd * 0.25]).contiguous()
    for mu, rs, gd in ((mean, rstd, None), (mean3, rstd3, gid)):
        y_ref, y = torch.zeros(N, C, device=DEV), torch.zeros(N, C, device=DEV)
        assert lib.stin_norm_act_res_fwd_f32(_ptr(x), C, _ptr(mu), _ptr(rs), _ptr(gd), _ptr(res_f), C, N, C, 1, _ptr(y_ref), C,
                                             _stream(x)) == 0
        assert lib.stin_norm_act_res_fwd_map_f32(_ptr(x), C, _ptr(mu), _ptr(rs), _ptr(gd), _ptr(res_c), C + 8, _ptr(trace), N, C, 1,
                                                 _ptr(y), C, _stream(x)) == 0
        assert float(y_ref.abs().max()) > 0 and torch.equal(y, y_ref)
    # the fold form
    assert lib.stin_norm_fold_rows(N, C, groups) > 0
    m1, r1, y1 = torch.zeros(1, C, device=DEV), torch.zeros(1, C, device=DEV), torch.zeros(N, C, device=DEV)
    m2, r2, y2 = torch.zeros(1, C, device=DEV), torch.zeros(1, C, device=DEV), torch.zeros(N, C, device=DEV)
    assert lib.stin_norm_act_res_fwd_fold_f32(_ptr(pm), groups, _ptr(x), C, _ptr(res_f), C, _ptr(inv), float(SF.EPS), N, C, _ptr(m1),
                                              _ptr(r1), _ptr(y1), C, _stream(x)) == 0
    assert lib.stin_norm_act_res_fwd_fold_map_f32(_ptr(pm), groups, _ptr(x), C, _ptr(res_c), C + 8, _ptr(trace), _ptr(inv), float(SF.EPS),
                                                  N, C, _ptr(m2), _ptr(r2), _ptr(y2), C, _stream(x)) == 0
    assert torch.equal(m1, mean) and torch.equal(r1, rstd)
    assert torch.equal(m2, m1) and torch.equal(r2, r1) and float(y1.abs().max()) > 0 and torch.equal(y2, y1)


@pytest.mark.parametrize('Mc,Mf,Nc,K', [(1806, 6000, 640, 256), (6021, 20070, 320, 128), (211, 777, 320, 128)])
def test_first_product_rows_do_not_depend_on_the_other_rows(Mc, Mf, Nc, K):
    """gather(gemm(x_c)) == gemm(gather(x_c)) with the operands block_fwd uses (pre-split fragment-order weights, fp16x3): the
    coarse and the fine product have different row counts, hence possibly different kernels of the NT family.  A pair that
    differed would mean the commutation has to be refused for that dispatch."""
    g = torch.Generator(device=DEV).manual_seed(Mc + Nc)
    xc = torch.randn(Mc, K, generator=g, device=DEV)
    W = torch.randn(Nc, K, generator=g, device=DEV) * K ** -0.5
    b = torch.randn(Nc, generator=g, device=DEV)
    trace = _trace(Mf, Mc, Mc).long()
    prec = SF.GEMM_F16X3 | SF.GEMM_W_FRAG
    Wf = SF.split_weights(W, prec)
    pf = prec | SF.GEMM_W_PRESPLIT
    coarse = SF.gemm_nt(xc, Wf, b, precision=pf)
    fine = SF.gemm_nt(xc[trace].contiguous(), Wf, b, precision=pf)
    assert float(fine.abs().max()) > 0
    assert torch.equal(coarse[trace], fine)


_CFG = dict(input_nc=10, output_nc=3, ngf=64, filter_type='edgeconvtransinv', norm='instance', n_blocks=3, n_levels=2,
            pooling_type='max', dilations=[1, 2, 4])


@functools.lru_cache(maxsize=None)
def _sample(batched):
    from surface_texture_inpainting_net_amd.data import collate
    if batched:
        return collate([make_synthetic_mesh(n, 3, seed=90 + i, dilations=(2, 4)) for i, n in enumerate((900, 1500, 700))]).to(DEV)
    return make_synthetic_mesh(6000, 3, seed=90, dilations=(2, 4)).to(DEV)


@functools.lru_cache(maxsize=None)
def _run(batched, dtype, commute):
    """-> (tensors of a training run, blocks commuted by the first forward, no-grad output, commuted / skipped of the no-grad forward)"""
    from surface_texture_inpainting_net_amd.train_step import TrainStep
    s = _sample(batched)
    old = SF.USE_UNPOOL_COMMUTE
    SF.USE_UNPOOL_COMMUTE = commute
    try:
        torch.manual_seed(11)
        net = S.define_G(**_CFG).to(DEV)
        if dtype == 'bf16':
            net.set_activation_dtype(torch.bfloat16)
        x = s.x.clone().requires_grad_(True)
        s2 = type(s)(**{k: (x if k == 'x' else s[k]) for k in s.keys()})
        s2._nv_host = s._nv_host
        c0 = SF.NetFn.commuted
        out = net(s2)
        took = SF.NetFn.commuted - c0
        out.float().square().mean().backward()
        res = [out.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in net.parameters()]
        net.zero_grad(set_to_none=True)
        c0, k0 = SF.NetFn.commuted, SF.NetFn.gathers_skipped
        with torch.no_grad():
            quiet = net(s).clone()
        quiet_counts = (SF.NetFn.commuted - c0, SF.NetFn.gathers_skipped - k0)
        step = TrainStep(net, lr=1e-3)
        losses = [float(step(s)) for _ in range(3)]
        step.finish()
        return res + [torch.tensor(losses)] + [p.detach().clone() for p in net.parameters()], took, quiet, quiet_counts
    finally:
        SF.USE_UNPOOL_COMMUTE = old


@pytest.mark.parametrize('batched', [False, True])
def test_network_with_the_first_product_on_coarse_rows_equals_the_switch_off_bitwise(batched):
    """Output, input gradient, every parameter gradient, three TrainStep losses and the parameters after them, with
    USE_UNPOOL_COMMUTE on and off; both decoder blocks take the path (and none with the switch off)."""
    got, took, _, _ = _run(batched, 'f32', True)
    want, took_off, _, _ = _run(batched, 'f32', False)
    assert took == 2 and took_off == 0
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), i


def test_bf16_storage_keeps_the_product_on_the_unpooled_rows():
    _, took, _, quiet_counts = _run(False, 'bf16', True)
    assert took == 0 and quiet_counts == (0, 0)


@pytest.mark.parametrize('batched', [False, True])
def test_no_grad_forward_equals_the_training_forward_and_runs_no_unpool_gather(batched):
    """A forward nobody differentiates keeps no x for backward: the unpool ops in front of the two commuted blocks get NO output
    buffer (stin_net_fwd has nothing to gather into), and the output still equals the training forward's bit for bit - which
    equals the switch-off forward (the test above)."""
    res, _, quiet, quiet_counts = _run(batched, 'f32', True)
    assert quiet_counts == (2, 2)
    assert torch.equal(quiet, res[0])
    _, _, quiet_off, counts_off = _run(batched, 'f32', False)
    assert counts_off == (0, 0) and torch.equal(quiet_off, quiet)
