"""Every launchable point of tests/_nt_table.py through its public entry point, under the point's switches, on small INTEGER operands:
A and W in [-3, 3], integer bias, 0 / 1 row mask, integer residual.  Every partial sum is then exact in fp32 and every 16-bit piece
of a split operand is exact, so each route must give the integer product itself: torch.equal with the product computed on the CPU
(in float64, exact below 2^53, then int64), an identical second call, and untouched guard rows / columns around the strided output
view.  bf16 output rows hold the exact result rounded once to bf16.  Fused epilogues: the product bit for bit, the group count of the
table, exact integer statistics.  tests/test_nt_geometry.py (no GPU) checks that each point aims at the route its line names; this
file uses only entry points and switches that exist without the query, so it also runs against a library built before it."""
import pytest
import torch

import _nt_table as T
from surface_texture_inpainting_net_amd import _lib
from surface_texture_inpainting_net_amd import functional as SF

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _view(vals, ld, off, dtype=torch.float32):
    """vals [R, C] as a view of width C in rows of ld elements whose base is `off` elements behind a 256-byte boundary"""
    R, C = vals.shape
    flat = torch.zeros(R * ld + off + 8, dtype=dtype, device=DEV)
    v = flat[off:off + R * ld].view(R, ld)[:, :C]
    v.copy_(vals.to(dtype))
    return v


def _out(M, Nc, padc, dtype):
    """-> (wide, view): the output as rows 1 .. M, columns c0 .. c0 + Nc of a wider matrix filled with 3"""
    c0 = (8 if dtype == torch.bfloat16 else 4) if padc >= 8 else 0
    wide = torch.full((M + 2, Nc + padc), 3.0, dtype=dtype, device=DEV)
    return wide, wide[1:M + 1, c0:c0 + Nc]


def _guards_untouched(wide, view):
    view.fill_(3.0)
    return bool((wide == 3.0).all())


def _operands(p):
    g = torch.Generator().manual_seed(p.M + 7 * p.Nc + 13 * p.K)
    A, W = _ints(g, -3, 3, p.M, p.K), _ints(g, -3, 3, p.Nc, p.K)
    bias = _ints(g, -4, 4, p.Nc) if p.parts & T.BIAS else None
    mask = (torch.rand(p.M, generator=g) < 0.7).float() if p.parts & T.MASK else None
    res = _ints(g, -9, 9, p.M, p.Nc) if p.parts & T.RES else None
    a = torch.relu(A) if p.parts & T.BN_TF else A                     # (the operand transform below is relu(1 x + 0))
    want = (a.double() @ W.double().t())
    if bias is not None:
        want = want + bias.double() * (mask.double()[:, None] if mask is not None else 1.0)
    if res is not None:
        want = want + res.double()
    return A, W, bias, mask, res, want.long()


def _unit_bn(K):
    z, o = torch.zeros(K, device=DEV), torch.ones(K, device=DEV)
    return z, o, o.clone(), z.clone()                                 # mean, rstd, gamma, beta


def _run_f32(p, lib, A, W, bias, mask, res, out):
    """one call of the point's entry point into `out`; -> (groups, partial) of a fused epilogue or None"""
    M, Nc, K = p.M, p.Nc, p.K
    st = SF._stream(A)
    Wd = SF.split_weights(W.contiguous(), p.prec & ~T.PRE) if p.prec & T.PRE else W
    ldw = K if p.prec & T.PRE else W.stride(0)
    mk, ldm = (mask, mask.stride(0)) if mask is not None else (None, 0)
    rs, ldr = (res, res.stride(0)) if res is not None else (None, 0)
    if p.parts & (T.STREAM_ONLY | T.BN_TF):
        bn = _unit_bn(K) if p.parts & T.BN_TF else (None,) * 4
        name = 'stin_gemm_nt_stream_f32' if p.parts & T.STREAM_ONLY else 'stin_gemm_nt_bn_f32'
        SF._call(name, SF._ptr(A), A.stride(0), SF._ptr(Wd), ldw, *(SF._ptr(t) for t in bn), M, Nc, K, SF._ptr(out), out.stride(0), p.prec, st)
        return None
    if p.parts & T.COLSTATS:
        if p.parts & T.DOTELU:
            assert lib.stin_gemm_nt_dotelu_groups(M, Nc, K, p.prec) == p.groups
        else:
            assert lib.stin_gemm_nt_colstats_groups(M, Nc, K, p.prec) == p.groups
        partial = torch.full((p.groups + 1, 2, Nc), -7.0, dtype=torch.float64, device=DEV)         # (one guard group behind)
        nbytes = p.groups * 2 * Nc * 8
        if p.parts & T.DOTELU:
            g = torch.Generator().manual_seed(5)
            nx = torch.randn(M, Nc, generator=g).to(DEV)
            z, o = torch.zeros(1, Nc, device=DEV), torch.ones(1, Nc, device=DEV)
            SF._call('stin_gemm_nt_dotelu_f32', SF._ptr(A), A.stride(0), SF._ptr(Wd), ldw, SF._ptr(bias), SF._ptr(rs), ldr, M, Nc, K,
                     SF._ptr(out), out.stride(0), p.prec, SF._ptr(nx), Nc, SF._ptr(z), SF._ptr(o), SF._ptr(partial), nbytes, st)
        else:
            SF._call('stin_gemm_nt_colstats_f32', SF._ptr(A), A.stride(0), SF._ptr(Wd), ldw, SF._ptr(bias), SF._ptr(mk), ldm, SF._ptr(rs),
                     ldr, M, Nc, K, SF._ptr(out), out.stride(0), p.prec, SF._ptr(partial), nbytes, st)
        return partial
    SF.gemm_nt(A, Wd, bias, out=out, row_mask=mask, precision=p.prec, residual=res)
    return None


_LAUNCH = [p for p in T.POINTS if T.launchable(p)]
_BN_BWD = T.BWD_STATS | T.BWD_APPLY


@pytest.mark.parametrize('p', [p for p in _LAUNCH if p.storage == 0 and not p.parts & _BN_BWD], ids=lambda p: p.id)
def test_fp32_rows_point_gives_the_integer_product(p, monkeypatch):
    lib = _lib.load()
    T.set_env(monkeypatch, p.env)
    A, W, bias, mask, res, want = _operands(p)
    ld = p.K + p.padk
    A, W = _view(A, ld, p.off), _view(W, ld, p.off)
    bias = bias.to(DEV) if bias is not None else None
    mask = _view(mask[:, None], 3, 0)[:, 0] if mask is not None else None
    res = _view(res, p.Nc + p.padc, 0) if res is not None else None
    wide, out = _out(p.M, p.Nc, p.padc, torch.float32)
    partial = _run_f32(p, lib, A, W, bias, mask, res, out)
    got = out.cpu()
    assert torch.equal(got.long(), want) and torch.equal(got, want.float()), p.id
    if partial is not None:
        assert partial.shape[0] == p.groups + 1 and bool((partial[p.groups] == -7.0).all())
        if not p.parts & T.DOTELU:                                    # exact integer column sums of the stored values, group by group folded
            assert torch.equal(partial[:p.groups, 0].sum(0).cpu(), want.double().sum(0))
            assert torch.equal(partial[:p.groups, 1].sum(0).cpu(), (want.double() ** 2).sum(0))
        else:
            assert bool(torch.isfinite(partial[:p.groups]).all())
        # the plain product of the same operands, bit for bit
        Wd = SF.split_weights(W.contiguous(), p.prec & ~T.PRE)
        plain = SF.gemm_nt(A, Wd, bias, row_mask=mask, precision=p.prec, residual=res)
        assert torch.equal(plain, out)
    out.zero_()
    again = _run_f32(p, lib, A, W, bias, mask, res, out)
    assert torch.equal(out.cpu(), got)
    if partial is not None:
        assert torch.equal(again, partial)
    assert _guards_untouched(wide, out), p.id


@pytest.mark.parametrize('p', [p for p in _LAUNCH if p.parts & _BN_BWD], ids=lambda p: p.id)
def test_batchnorm_backward_point_gives_the_integer_sums_and_gradient(p, monkeypatch):
    """dh = A W^T as the output gradient of BatchNorm + ReLU over X with mean 0, rstd 1, gamma 1, beta 0: d = dh [X > 0], nhat = X.
    stats: P = sum d X, Q = sum d (integers below 2^24: exact as floats); apply with P = Q = 0: dx = d."""
    lib = _lib.load()
    T.set_env(monkeypatch, p.env)
    M, Nc, K = p.M, p.Nc, p.K
    A, W, _, _, _, dh = _operands(p)
    g = torch.Generator().manual_seed(11)
    X = _ints(g, -3, 3, M, Nc)
    d = dh * (X > 0).long()
    A, W, Xd = _view(A, K + p.padk, 0), _view(W, K + p.padk, 0), _view(X, Nc + 4, 0)
    bn = _unit_bn(Nc)
    args = (SF._ptr(A), A.stride(0), SF._ptr(W), W.stride(0), SF._ptr(Xd), Xd.stride(0)) + tuple(SF._ptr(t) for t in bn)
    if p.parts & T.BWD_STATS:
        assert lib.stin_gemm_nt_bn_bwd_groups(M, Nc, K, p.prec) == p.groups
        want = torch.stack([(d * X.long()).sum(0), d.sum(0)])
        assert int(want.abs().max()) < 2 ** 24
        outs = []
        for _ in range(2):
            partial = torch.full((p.groups + 1, 2, Nc), -7.0, dtype=torch.float64, device=DEV)
            sums = torch.full((2, Nc), 3.0, device=DEV)
            SF._call('stin_gemm_nt_bn_bwd_stats_f32', *args, M, Nc, K, p.prec, SF._ptr(partial), p.groups * 2 * Nc * 8, SF._ptr(sums),
                     SF._stream(A))
            assert torch.equal(sums.cpu().long(), want) and bool((partial[p.groups] == -7.0).all())
            assert torch.equal(partial[:p.groups].sum(0).cpu(), want.double())
            outs.append((partial, sums))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        return
    sums = torch.zeros(2, Nc, device=DEV)
    wide, out = _out(M, Nc, p.padc, torch.float32)
    got = None
    for _ in range(2):
        out.zero_()
        SF._call('stin_gemm_nt_bn_bwd_apply_f32', *args, SF._ptr(sums), 1.0 / M, M, Nc, K, SF._ptr(out), out.stride(0), p.prec, SF._stream(A))
        assert torch.equal(out.cpu().long(), d)
        assert got is None or torch.equal(out, got)
        got = out.clone()
    assert _guards_untouched(wide, out)


@pytest.mark.parametrize('p', [p for p in _LAUNCH if p.storage == 1], ids=lambda p: p.id)
def test_bf16_rows_point_gives_the_integer_product(p, monkeypatch):
    T.set_env(monkeypatch, p.env)
    A, W, bias, mask, res, want = _operands(p)
    bf = torch.bfloat16
    A = _view(A, p.K + p.padk, p.off, bf)
    W = _view(W, p.K + p.padk, p.off, bf if p.prec & T.WB16 else torch.float32)
    bias = bias.to(DEV) if bias is not None else None
    mask = _view(mask[:, None], 3, 0, bf)[:, 0] if mask is not None else None
    res = _view(res, p.Nc + p.padc, 0, bf) if res is not None else None
    odt = torch.float32 if p.parts & T.OUT_F32 else bf
    wide, out = _out(p.M, p.Nc, p.padc, odt)
    SF.gemm_nt(A, W, bias, out=out, row_mask=mask, residual=res)
    got = out.cpu()
    assert torch.equal(got, want.float().to(odt)), p.id               # (bf16 rows: the exact fp32 result rounded once, to nearest even)
    out.zero_()
    SF.gemm_nt(A, W, bias, out=out, row_mask=mask, residual=res)
    assert torch.equal(out.cpu(), got)
    assert _guards_untouched(wide, out), p.id
