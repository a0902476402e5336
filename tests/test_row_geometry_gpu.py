"""Bit equality of every row kernel of stin_graph.hip with the sequential fp32 contract (tests/_row_oracle.py), on every lane
geometry (G, VPL) and across every boundary of the rows-in-flight count U.

The tolerance tests of test_hip_parity.py pass a reordered sum or a dropped last trip of a U-loop; these do not.  Shapes are the
smallest at which a class can go wrong: N = 301 leaves a partial last block for every G (301 mod {256, 128, .., 4} != 0) and a
partial last TI_ITER group, N = 1 is the single row, N = 0 must write nothing; in-degree i mod 14 walks two full trips plus a
remainder of the largest U = 6 and U - 1, U, U + 1 of every U; each case also runs on the reversed graph so that the source CSR
sees the same sweep.  One exact and one ragged width per 4-channel class, 6 and 3 for the scalar route, the five saved-mask
widths in fp32 and in bf16 (8 channels per lane, 2048 included), and the 4-channel bf16 route on 8-byte aligned rows."""
import pytest
import torch

import _row_oracle as O
from oracle import scatter_ops
from surface_texture_inpainting_net_amd import _lib
from surface_texture_inpainting_net_amd import functional as SF
from surface_texture_inpainting_net_amd.plan import EdgeSet, PoolMap, _ptr, _stream

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_C = _lib.CONSTANTS
EXACT_W = [4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048]
RAGGED_W = [12, 20, 36, 68, 132, 260, 516, 1028]
WIDTHS = EXACT_W + RAGGED_W + [6, 3]
MASK_W = [128, 256, 512, 1024, 2048]
SENT = 7.0


class Graph:
    """An edge set on the GPU and its two CSRs on the CPU (built independently: stable order by key)."""

    def __init__(self, ei, n):
        self.n, self.ei, self.E = n, ei, ei.shape[1]
        self.es = EdgeSet(ei.to(DEV), n, torch.zeros(1, dtype=torch.int32, device=DEV))
        self.rp_d, self.col_d, _ = O.csr(ei[1], ei[0], n)
        self.rp_s, self.col_s, _ = O.csr(ei[0], ei[1], n)
        self.inv_deg = 1.0 / (self.rp_d[1:] - self.rp_d[:-1]).clamp(min=1).float()
        assert torch.equal(self.es.by_dst.col.cpu().long(), self.col_d) and torch.equal(self.es.by_src.col.cpu().long(), self.col_s)
        assert torch.equal(self.es.inv_deg.cpu(), self.inv_deg)


_GRAPHS = {}


def graph(n, rev):
    if (n, rev) not in _GRAPHS:
        ei = O.sweep_graph(n, seed=n, first=0 if n > 1 else 3)       # (the single row: three self loops)
        _GRAPHS[n, rev] = Graph(ei.flip(0) if rev else ei, n)
    return _GRAPHS[n, rev]


def _rows(n, C, seed, dtype=torch.float32, count=1, ints=False):
    g = torch.Generator().manual_seed(seed)
    mk = (lambda: torch.randint(-3, 4, (n, C), generator=g).float()) if ints else (lambda: torch.randn(n, C, generator=g))
    return [mk().to(dtype) for _ in range(count)]


def _in_slices(ts, lead=0):
    """the operands as column slices of one wider device matrix (`lead` unused columns first, 8 between and behind)"""
    n = ts[0].shape[0]
    wide = torch.full((n, lead + sum(t.shape[1] + 8 for t in ts)), SENT, dtype=ts[0].dtype, device=DEV)
    out, c = [], lead
    for t in ts:
        wide[:, c:c + t.shape[1]] = t.to(DEV)
        out.append(wide[:, c:c + t.shape[1]])
        c += t.shape[1] + 8
    return out


class Out:
    """an output as a column slice of a wider matrix pre-filled with a sentinel, which must stay untouched"""

    def __init__(self, n, C, dtype=torch.float32, lead=4, tail=8):
        self.wide = torch.full((n, lead + C + tail), SENT, dtype=dtype, device=DEV)
        self.v = self.wide[:, lead:lead + C]
        self.lead, self.C = lead, C

    def get(self, extra=0):
        w = self.wide.cpu()
        assert bool((w[:, :self.lead] == SENT).all()) and bool((w[:, self.lead + self.C + extra:] == SENT).all())
        return w[:, self.lead:self.lead + self.C]


# ------------------------------------------------------------------ every (G, VPL) class, fp32: recompute kernels and row ops
@pytest.mark.parametrize('rev', [0, 1])
@pytest.mark.parametrize('n', [301, 1])
@pytest.mark.parametrize('H', WIDTHS)
def test_edge_forward_and_recompute_backward(H, n, rev):
    gr = graph(n, rev)
    A, B, G = _rows(n, H, H, count=3)
    Ad, Bd, Gd = _in_slices([A, B, G])
    out = Out(n, H)
    SF.edge_relu_mean_fwd(Ad, Bd, gr.es.by_dst, out.v)
    assert torch.equal(out.get(), O.edge_fwd(A, B, gr.rp_d, gr.col_d))
    dA, dB = Out(n, H), Out(n, H)
    SF.edge_relu_mean_bwd_dst(Ad, Bd, Gd, gr.es.by_dst, dA.v)
    SF.edge_relu_mean_bwd_src(Ad, Bd, Gd, gr.es.inv_deg, gr.es.by_src, dB.v)
    assert torch.equal(dA.get(), O.edge_bwd_dst(A, B, G, gr.rp_d, gr.col_d))
    assert torch.equal(dB.get(), O.edge_bwd_src(A, B, G, gr.inv_deg, gr.rp_s, gr.col_s))
    if H >= 4:
        ind = Out(n, H, tail=12)
        SF.edge_relu_mean_fwd(Ad, Bd, gr.es.by_dst, ind.wide[:, 4:], indicator=True)
        assert torch.equal(ind.get(extra=4), out.get())
        has = (gr.rp_d[1:] > gr.rp_d[:-1]).float()
        assert torch.equal(ind.wide[:, 4 + H:8 + H].cpu(), torch.stack([has, 0 * has, 0 * has, 0 * has], 1))


@pytest.mark.parametrize('rev', [0, 1])
@pytest.mark.parametrize('n', [301, 1])
@pytest.mark.parametrize('C', WIDTHS)
def test_segment_sum_pool_and_gather(C, n, rev):
    gr = graph(n, rev)
    (src,) = _rows(max(gr.E, n), C, C + 1)
    (sd,) = _in_slices([src])
    for mean in (False, True):
        got = SF.segment_sum(sd, gr.es.by_dst.rowptr, gr.es.by_dst.col, n, mean=mean)
        assert torch.equal(got.cpu(), O.segment_sum(src, gr.rp_d, gr.col_d, mean)), mean
        got = SF.segment_sum(sd, gr.es.by_dst.rowptr, None, n, mean=mean)               # col = None: slot e reads row e
        assert torch.equal(got.cpu(), O.segment_sum(src, gr.rp_d, None, mean)), mean
    # max pool over the same degree sweep: coarse vertex i has the fine vertices of its slots as children (many exact ties)
    trace = gr.ei[1][torch.randperm(gr.E, generator=torch.Generator().manual_seed(C))]
    pm = PoolMap(trace.to(DEV), gr.E, n, torch.zeros(1, dtype=torch.int32, device=DEV))
    x, = _rows(gr.E, C, C + 2, ints=True)
    w, = _rows(n, C, C + 3)
    x.requires_grad_(True)
    want, _ = scatter_ops.scatter_max(x, trace, dim=0, dim_size=n)
    (want * w).sum().backward()
    xd = _in_slices([x.detach()])[0].requires_grad_(True)
    got = SF.PoolMaxFn.apply(xd, pm)
    (got * w.to(DEV)).sum().backward()
    assert torch.equal(got.cpu(), want.detach())
    assert torch.equal(xd.grad.cpu(), x.grad)
    idx = torch.randint(0, src.shape[0], (n,), generator=torch.Generator().manual_seed(C + 4))
    scale = torch.randn(src.shape[0], generator=torch.Generator().manual_seed(C + 5))
    assert torch.equal(SF.gather_rows(sd, idx.to(DEV).int()).cpu(), src[idx])
    assert torch.equal(SF.gather_rows(sd, idx.to(DEV).int(), scale.to(DEV)).cpu(), src[idx] * scale[idx][:, None])


# ------------------------------------------------------------------ saved-mask widths, fp32
def _ti_call(gr, G, mask, D, cp=(0, 0, 0, 0, 0)):
    lib = _lib.load()
    n, H = G.shape
    rows = int(lib.stin_edge_bwd_ti_colsum_rows(n, H))
    colsum = torch.full((rows + 1, H), SENT, device=DEV)
    es = gr.es
    _lib.check(lib.stin_edge_relu_mean_bwd_mask_ti_f32(
        _ptr(G), G.stride(0), _ptr(mask), _ptr(es.by_dst.rowptr), _ptr(es.w_src), _ptr(es.by_src.rowptr), _ptr(es.by_src.col),
        _ptr(es.xslot), n, H, _ptr(D), D.stride(0), *cp, _ptr(colsum), rows, _stream(G)), 'bwd_mask_ti')
    assert bool((colsum[rows] == SENT).all())
    return colsum[:rows].cpu()


@pytest.mark.parametrize('rev', [0, 1])
@pytest.mark.parametrize('n', [301, 1])
@pytest.mark.parametrize('H', MASK_W)
def test_saved_mask_kernels_fp32(H, n, rev):
    gr = graph(n, rev)
    es = gr.es
    A, B, G = _rows(n, H, H + 7, count=3)
    Ad, Bd, Gd = _in_slices([A, B, G])
    want = O.edge_fwd(A, B, gr.rp_d, gr.col_d)
    want_dA = O.edge_bwd_dst(A, B, G, gr.rp_d, gr.col_d)
    want_dB = O.edge_bwd_src(A, B, G, gr.inv_deg, gr.rp_s, gr.col_s)
    mask = torch.zeros(max(gr.E, 1) * (H // 32), dtype=torch.int32, device=DEV)
    out0, out1 = Out(n, H), Out(n, H)
    SF.edge_relu_mean_fwd(Ad, Bd, es.by_dst, out0.v)
    SF.edge_relu_mean_fwd(Ad, Bd, es.by_dst, out1.v, mask=mask)
    assert torch.equal(out0.get(), want) and torch.equal(out1.get(), want)
    # the two mask kernels == the recompute kernels == the contract
    r = {k: Out(n, H) for k in ('dA0', 'dB0', 'dA1', 'dB1', 'pA', 'pB', 'qA', 'qB', 'D', 'D2')}
    SF.edge_relu_mean_bwd_dst(Ad, Bd, Gd, es.by_dst, r['dA0'].v)
    SF.edge_relu_mean_bwd_src(Ad, Bd, Gd, es.inv_deg, es.by_src, r['dB0'].v)
    SF.edge_relu_mean_bwd_dst_mask(Gd, mask, es.by_dst, r['dA1'].v)
    SF.edge_relu_mean_bwd_src_mask(Gd, mask, es, r['dB1'].v)
    for k in ('dA0', 'dA1'):
        assert torch.equal(r[k].get(), want_dA), k
    for k in ('dB0', 'dB1'):
        assert torch.equal(r[k].get(), want_dB), k
    # both halves in one launch, without and with the row-copy rider (H / 2 channels from a strided source)
    cp_src, = _in_slices(_rows(n, H // 2, H + 8))
    cp = Out(n, H // 2)
    SF.edge_relu_mean_bwd_mask(Gd, mask, es, r['pA'].v, r['pB'].v)
    SF.edge_relu_mean_bwd_mask(Gd, mask, es, r['qA'].v, r['qB'].v, copy_src=cp_src, copy_dst=cp.v)
    for k in ('pA', 'qA'):
        assert torch.equal(r[k].get(), want_dA), k
    for k in ('pB', 'qB'):
        assert torch.equal(r[k].get(), want_dB), k
    assert torch.equal(cp.get(), cp_src.cpu())
    # translation-invariant compact form: D = dB - dA in fp32, and the per-block column sums of dA
    want_cs = O.ti_colsum(want_dA, H)
    cs = _ti_call(gr, Gd, mask, r['D'].v)
    assert torch.equal(r['D'].get(), want_dB - want_dA)
    assert torch.equal(cs, want_cs)
    assert torch.equal(O.fold_rows(cs), O.fold_rows(want_cs))
    cp2 = Out(n, H // 2)
    cs2 = _ti_call(gr, Gd, mask, r['D2'].v, (_ptr(cp_src), cp_src.stride(0), _ptr(cp2.v), cp2.v.stride(0), H // 2))
    assert torch.equal(r['D2'].get(), want_dB - want_dA) and torch.equal(cs2, want_cs) and torch.equal(cp2.get(), cp_src.cpu())
    # the forward forms that exist at these widths only: A_i = b1 - B_i formed per row, and rows read through a row map
    b1 = torch.randn(H, generator=torch.Generator().manual_seed(H))
    for bias in (b1, None):
        ti = Out(n, H)
        SF.edge_relu_mean_fwd_ti(None if bias is None else bias.to(DEV), Bd, es.by_dst, ti.v, mask=mask)
        assert torch.equal(ti.get(), O.edge_fwd((bias if bias is not None else 0) - B, B, gr.rp_d, gr.col_d))
    nc = n // 3 + 1
    row_map = torch.randint(0, nc, (n,), generator=torch.Generator().manual_seed(n))
    Ac, Bc = _rows(nc, H, H + 9, count=2)
    Acd, Bcd = _in_slices([Ac, Bc])
    mp = Out(n, H)
    _lib.check(_lib.load().stin_edge_relu_mean_fwd_map_f32(
        _ptr(Acd), Acd.stride(0), _ptr(Bcd), Bcd.stride(0), _ptr(es.by_dst.rowptr), _ptr(es.by_dst.col),
        _ptr(row_map.to(DEV).int()), n, H, _ptr(mp.v), mp.v.stride(0), 0, _ptr(mask), _stream(Acd)), 'fwd_map')
    assert torch.equal(mp.get(), O.edge_fwd(Ac[row_map], Bc[row_map], gr.rp_d, gr.col_d))


# ------------------------------------------------------------------ bf16 storage
@pytest.mark.parametrize('rev', [0, 1])
@pytest.mark.parametrize('n', [301, 1])
@pytest.mark.parametrize('H', MASK_W)
def test_eight_channel_bf16_kernels(H, n, rev):
    bf = torch.bfloat16
    gr = graph(n, rev)
    es = gr.es
    A, B, G = _rows(n, H, H + 11, dtype=bf, count=3)
    Ad, Bd, Gd = _in_slices([A, B, G], lead=8)                      # 16-byte aligned rows: the 8-channel geometry
    assert all(t.data_ptr() % 16 == 0 and t.stride(0) % 8 == 0 for t in (Ad, Bd, Gd))
    want = O.edge_fwd(A, B, gr.rp_d, gr.col_d).to(bf)
    want_dA = O.edge_bwd_dst(A, B, G, gr.rp_d, gr.col_d).to(bf)
    want_dB = O.edge_bwd_src(A, B, G, gr.inv_deg, gr.rp_s, gr.col_s).to(bf)
    mask = torch.zeros(max(gr.E, 1) * (H // 32), dtype=torch.int32, device=DEV)
    out0, out1 = Out(n, H, bf, lead=8), Out(n, H, bf, lead=8)
    SF.edge_relu_mean_fwd(Ad, Bd, es.by_dst, out0.v)
    SF.edge_relu_mean_fwd(Ad, Bd, es.by_dst, out1.v, mask=mask)
    assert torch.equal(out0.get(), want) and torch.equal(out1.get(), want)
    r = {k: Out(n, H, bf, lead=8) for k in ('dA', 'dB', 'pA', 'pB', 'qA', 'qB')}
    SF.edge_relu_mean_bwd_dst_mask(Gd, mask, es.by_dst, r['dA'].v)
    SF.edge_relu_mean_bwd_src_mask(Gd, mask, es, r['dB'].v)
    cp_src, = _in_slices(_rows(n, H // 2, H + 12, dtype=bf), lead=8)
    cp = Out(n, H // 2, bf, lead=8)
    SF.edge_relu_mean_bwd_mask(Gd, mask, es, r['pA'].v, r['pB'].v)
    SF.edge_relu_mean_bwd_mask(Gd, mask, es, r['qA'].v, r['qB'].v, copy_src=cp_src, copy_dst=cp.v)
    for k in ('dA', 'pA', 'qA'):
        assert torch.equal(r[k].get(), want_dA), k
    for k in ('dB', 'pB', 'qB'):
        assert torch.equal(r[k].get(), want_dB), k
    assert torch.equal(cp.get(), cp_src.cpu())


@pytest.mark.parametrize('rev', [0, 1])
@pytest.mark.parametrize('C', [8, 128, 132])
def test_four_channel_bf16_route_on_8_byte_rows(C, rev):
    """Rows offset by 4 elements: 8- but not 16-byte aligned, so bf16 rows take the 4-channel kernels - and a mask is refused."""
    bf = torch.bfloat16
    n = 301
    gr = graph(n, rev)
    es = gr.es
    A, B = _rows(n, C, C + 13, dtype=bf, count=2)
    Ad, Bd = _in_slices([A, B], lead=4)
    assert Ad.data_ptr() % 16 == 8 and Bd.data_ptr() % 8 == 0 and Ad.stride(0) % 4 == 0
    out = Out(n, C, bf, lead=4)
    SF.edge_relu_mean_fwd(Ad, Bd, es.by_dst, out.v)
    assert torch.equal(out.get(), O.edge_fwd(A, B, gr.rp_d, gr.col_d).to(bf))
    for mean in (False, True):
        got = SF.segment_sum(Ad, es.by_dst.rowptr, es.by_dst.col, n, mean=mean)
        assert torch.equal(got.cpu(), O.segment_sum(A, gr.rp_d, gr.col_d, mean).to(bf)), mean
    idx = torch.randint(0, n, (n,), generator=torch.Generator().manual_seed(C))
    assert torch.equal(SF.gather_rows(Ad, idx.to(DEV).int()).cpu(), A[idx])
    trace = torch.randint(0, 90, (n,), generator=torch.Generator().manual_seed(C + 1))
    pm = PoolMap(trace.to(DEV), n, 90, torch.zeros(1, dtype=torch.int32, device=DEV))
    x = torch.randint(-3, 4, (n, C), generator=torch.Generator().manual_seed(C + 2)).float().requires_grad_(True)
    w = torch.randint(-3, 4, (90, C), generator=torch.Generator().manual_seed(C + 3)).float()
    want, _ = scatter_ops.scatter_max(x, trace, dim=0, dim_size=90)
    (want * w).sum().backward()
    xd = _in_slices([x.detach().to(bf)], lead=4)[0].requires_grad_(True)
    got = SF.PoolMaxFn.apply(xd, pm)
    (got.float() * w.to(DEV)).sum().backward()
    assert torch.equal(got.float().cpu(), want.detach()) and torch.equal(xd.grad.float().cpu(), x.grad)
    if C == 128:
        mask = torch.zeros(gr.E * (C // 32), dtype=torch.int32, device=DEV)
        code = _lib.load().stin_edge_relu_mean_fwd_bf16(_ptr(Ad), Ad.stride(0), _ptr(Bd), Bd.stride(0), _ptr(es.by_dst.rowptr),
                                                        _ptr(es.by_dst.col), n, C, _ptr(out.v), out.v.stride(0), 0, _ptr(mask),
                                                        _stream(Ad))
        assert code == _C['STIN_E_ALIGN']
        assert int(mask.abs().max()) == 0


# ------------------------------------------------------------------ N = 0: STIN_OK, nothing written
@pytest.mark.parametrize('H', [32, 128])
def test_no_rows_is_ok_and_writes_nothing(H):
    lib = _lib.load()
    gr = graph(301, 0)
    es = gr.es
    X = torch.full((4, H), SENT, device=DEV)
    outs = [torch.full((4, H + 4), SENT, device=DEV) for _ in range(3)]
    iarg = torch.full((4, H), 77, dtype=torch.int32, device=DEV)
    mask = torch.full((64,), 77, dtype=torch.int32, device=DEV)
    o0, o1, cs = outs
    p, ld, st = _ptr(X), X.stride(0), _stream(X)
    rp, col, rps, cols, xs, ws = (_ptr(t) for t in (es.by_dst.rowptr, es.by_dst.col, es.by_src.rowptr, es.by_src.col, es.xslot, es.w_src))
    m = _ptr(mask) if H == 128 else 0
    codes = [
        lib.stin_edge_relu_mean_fwd_f32(p, ld, p, ld, rp, col, 0, H, _ptr(o0), H + 4, 1, m, st),
        lib.stin_edge_relu_mean_bwd_dst_f32(p, ld, p, ld, p, ld, rp, col, 0, H, _ptr(o0), H + 4, st),
        lib.stin_edge_relu_mean_bwd_src_f32(p, ld, p, ld, p, ld, _ptr(es.inv_deg), rps, cols, 0, H, _ptr(o0), H + 4, st),
        lib.stin_segment_sum_f32(p, ld, rp, col, 0, H, 1, _ptr(o0), H + 4, st),
        lib.stin_pool_max_fwd_f32(p, ld, rp, col, 0, H, _ptr(o0), H + 4, _ptr(iarg), st),
        lib.stin_pool_max_bwd_f32(p, ld, _ptr(iarg), col, 0, H, _ptr(o0), H + 4, st),
        lib.stin_gather_rows_f32(p, ld, col, 0, 0, H, _ptr(o0), H + 4, st),
    ]
    if H == 128:
        codes += [
            lib.stin_edge_relu_mean_bwd_dst_mask_f32(p, ld, m, rp, 0, H, _ptr(o0), H + 4, st),
            lib.stin_edge_relu_mean_bwd_src_mask_f32(p, ld, ws, m, rps, cols, xs, 0, H, _ptr(o0), H + 4, st),
            lib.stin_edge_relu_mean_bwd_mask_f32(p, ld, m, rp, ws, rps, cols, xs, 0, H, _ptr(o0), H + 4, _ptr(o1), H + 4, p, ld,
                                                 _ptr(cs), H + 4, H, st),
            lib.stin_edge_relu_mean_bwd_mask_ti_f32(p, ld, m, rp, ws, rps, cols, xs, 0, H, _ptr(o0), H + 4, p, ld, _ptr(o1), H + 4, H,
                                                    _ptr(cs), 4, st),
            lib.stin_edge_relu_mean_fwd_ti_f32(0, p, ld, rp, col, 0, H, _ptr(o0), H + 4, 0, m, st),
        ]
    torch.cuda.synchronize()
    assert codes == [_C['STIN_OK']] * len(codes)
    assert all(bool((t == SENT).all()) for t in outs) and bool((iarg == 77).all()) and bool((mask == 77).all())
