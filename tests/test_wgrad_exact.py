"""The weight-gradient products dW = G^T [X | w] (stin_gemm_tn_*, stin_edgeconv_wgrad*) pinned to EXACT results on every route.

Integer-valued operands (entries in {-3 .. 3}, row weights in {0, 1, 2}, at most 32 897 rows) make every partial sum, in ANY
order, an integer below 2^24: exactly representable in fp32 at every step of every tiling, chunking and fold.  The result must
therefore EQUAL the fp64 product - no tolerance, no dependence on the summation order.  These tests are meant to stay green
across a retiling; the bit-identity tests between two HIP routes (test_hip_parity.py: ..._ws_kernel_equals_four_wave_kernel,
..._wgrad_equals_two_tn_gemms_plus_unpack, ..._transposed_read_kernel_equals_register_transpose_kernel; test_backward_without_copies.py:
test_mapped_weight_gradient_...) are expected to be replaced by one.

Every case takes its geometry from tests/_tn_table.py (whose expectations tests/test_tn_geometry.py checks without a GPU) and
asserts it again through stin_gemm_tn_route for the operands it really passes.  Operands are views with ld != width inside
buffers filled with 1e30, so a read outside an operand changes a sum instead of faulting; outputs lie inside buffers pre-filled
with 7.0 that must stay 7.0 around the result.
"""
import pytest
import torch

import _tn_table as T
from surface_texture_inpainting_net_amd import _lib
from surface_texture_inpainting_net_amd import functional as SF
from surface_texture_inpainting_net_amd import singleconvmeshnet as SCMN

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
POISON = 1.0e30
FILL = 7.0
DT = {0: torch.float32, 1: torch.bfloat16}


def ints(shape, seed, dtype=torch.float32, lo=-3, hi=3):
    """uniform in {lo .. hi}: exact in fp32 and in bf16"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g, device=DEV).to(dtype)


def strided(values, pad, off):
    """`values` [M, W] as a view with row pitch W + pad whose base is `off` elements behind a 16-byte boundary, inside a buffer
    of POISON (eight rows in front, one behind)"""
    M, W = values.shape
    if pad == 0 and off == 0:
        return values.contiguous()
    ld = W + pad
    buf = torch.full(((M + 9) * ld + 16,), POISON, dtype=values.dtype, device=DEV)
    v = buf.as_strided((M, W), (ld, 1), 8 * ld + off)
    v.copy_(values)
    assert (v.data_ptr() % 16 == 0) == (off == 0)
    return v


def column(values):
    """an [M] vector as column 1 of an [M, 3] matrix of POISON: a strided row-weight view"""
    buf = torch.full((values.shape[0], 3), POISON, dtype=values.dtype, device=DEV)
    buf[:, 1] = values
    return buf[:, 1]


def guarded(rows, cols):
    """-> (buffer, view [rows, cols]): one row and four columns larger, filled with FILL"""
    buf = torch.full((rows + 1, cols + 4), FILL, device=DEV)
    return buf, buf[:rows, :cols]


def guarded_flat(*shape):
    """a CONTIGUOUS output (the block entry points take no pitch) with four elements of FILL in front and behind"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 8,), FILL, device=DEV)
    return buf, buf[4:4 + n].view(*shape)


def untouched(buf, view):
    keep = view.clone()
    view.fill_(FILL)
    ok = bool((buf == FILL).all())
    view.copy_(keep)
    return ok


def tn_raw(G, X, ones, w, prec, wb=False):
    """The C entry point itself with guarded destinations -> (dW [Nc, K (+1)], db or None)"""
    lib = _lib.load()
    M, Nc = G.shape
    K = X.shape[1]
    b16 = G.dtype == torch.bfloat16
    Kp = K + (1 if ones and not wb else 0)
    buf, dW = guarded(Nc, Kp)
    dbuf, db = guarded_flat(Nc) if wb else (None, None)
    ws_bytes = lib.stin_gemm_tn_workspace_bytes(M, Nc, K, int(ones))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    head = (SF._ptr(G), G.stride(0), SF._ptr(X), X.stride(0), M, Nc, K)
    wargs = (SF._ptr(w), w.stride(0) if w is not None else 0)
    tail = (SF._ptr(ws), ws_bytes, SF._stream(G))
    p = () if b16 else (int(prec),)
    if wb:
        SF._call('stin_gemm_tn_wb_bf16' if b16 else 'stin_gemm_tn_wb_f32', *head, *wargs, SF._ptr(dW), dW.stride(0), SF._ptr(db), *p, *tail)
    else:
        SF._call('stin_gemm_tn_bf16' if b16 else 'stin_gemm_tn_f32', *head, int(ones), *wargs, SF._ptr(dW), dW.stride(0), *p, *tail)
    assert untouched(buf, dW) and (not wb or untouched(dbuf, db))
    return dW.clone(), (db.clone() if wb else None)


def check_geometry(p, G, X, ones=1):
    aligned = int(G.data_ptr() % 16 == 0 and X.data_ptr() % 16 == 0)
    g = T.geometry(_lib.load(), p.storage, p.M, p.Nc, p.K, G.stride(0), X.stride(0), aligned, ones, p.prec)
    assert (g['family'], g['tile'], g['chunks'], g['vec'], g['ws']) == (p.family, p.tile, p.chunks, p.vec, p.ws), (p.id, g)


def operands(p, seed=0):
    dt = DT[p.storage]
    G = strided(ints((p.M, p.Nc), 3 * p.M + p.Nc + seed, dt), p.padg, p.off)
    X = strided(ints((p.M, p.K), 5 * p.M + p.K + 1 + seed, dt), p.padx, p.off)
    w = column(ints((p.M,), 7 * p.M + 2 + seed, dt, 0, 2))
    return G, X, w


def exact_product(G, X, w=None):
    """fp64 on the device: [G^T X | sum_m w[m] G[m, :]]"""
    Gd = G.double()
    bias = (Gd * w.double()[:, None]).sum(0) if w is not None else Gd.sum(0)
    return Gd.t() @ X.double(), bias


def all_forms_equal(p, G, X, w, want, want_b1, want_bw):
    """every form of the stand-alone product: no bias column | ones column | weighted column | dW and db apart (with and without
    row weights) - the C entry point with guarded outputs, then the wrapper: the same tensor twice, equal to the fp64 product"""
    K = p.K
    for ones, rw, bias in ((False, None, None), (True, None, want_b1), (True, w, want_bw)):
        got, _ = tn_raw(G, X, ones, rw, p.prec)
        again = SF.gemm_tn(G, X, ones_column=ones, row_weight=rw, precision=p.prec)
        assert torch.equal(got, again), (p.id, ones, rw is not None)
        assert torch.equal(got[:, :K].double(), want), (p.id, ones, rw is not None)
        if ones:
            assert torch.equal(got[:, K].double(), bias), (p.id, rw is not None)
    dW, db = tn_raw(G, X, True, w, p.prec, wb=True)
    assert torch.equal(dW.double(), want) and torch.equal(db.double(), want_bw), p.id
    dW2, db2 = torch.full((p.Nc, K), FILL, device=DEV), torch.full((p.Nc,), FILL, device=DEV)
    SF.gemm_tn_wb(G, X, dW2, db2, precision=p.prec)
    assert torch.equal(dW2.double(), want) and torch.equal(db2.double(), want_b1), p.id


# ---------------------------------------------------------------------------------------------- stand-alone products
@pytest.mark.parametrize('p', T.POINTS, ids=lambda p: p.id)
def test_tn_product_of_integers_is_exact(p, monkeypatch):
    T.set_env(monkeypatch, p.env)
    G, X, w = operands(p)
    check_geometry(p, G, X)
    want, want_b1 = exact_product(G, X)
    _, want_bw = exact_product(G, X, w)
    if p.M == 0:
        assert float(want.abs().max()) == 0.0 and float(want_b1.abs().max()) == 0.0
    else:
        assert float(want.abs().max()) > 0 and float(want.abs().max()) < 2 ** 24
    all_forms_equal(p, G, X, w, want, want_b1, want_bw)


# ---------------------------------------------------------------------------------------------- two-piece operands
# v = a + sign(a) b / 256, |a| in {2, 3}, b in {0, 1, 2}: bf16 keeps 8 significant bits, one ulp in [2, 4) is 4 / 256, so v rounds
# to a under round-to-nearest-even (b = 2 is the tie: 2 and 3 have even bf16 mantissas) and under truncation alike, and the
# remainder sign(a) b / 256 is a bf16 number: the two-piece split of v is exactly (a, b') whatever the rounding.  (b = 3 would
# round AWAY from a under round-to-nearest: 3 / 256 is beyond the half ulp.)
TWO_PIECE_A, TWO_PIECE_B = (-3.0, -2.0, 2.0, 3.0), (0.0, 1.0, 2.0)
TWO_PIECE_POINTS = [p for p in T.POINTS if p.storage == 0 and p.prec == T.X3 and 0 < p.M <= 4096 and p.tile != T.SKINNY]


def two_piece(shape, seed):
    a = ints(shape, seed, lo=0, hi=3)
    a = torch.tensor(TWO_PIECE_A, device=DEV)[a.long()]
    b = torch.sign(a) * ints(shape, seed + 1, lo=0, hi=2) / 256.0
    return a + b, a, b


def test_two_piece_values_split_exactly():
    """on the CPU: every value of the set, under round-to-nearest (torch's conversion) and under truncation of the low 16 bits"""
    a = torch.tensor([x for x in TWO_PIECE_A for _ in TWO_PIECE_B])
    b = torch.sign(a) * torch.tensor(list(TWO_PIECE_B) * len(TWO_PIECE_A)) / 256.0
    v = a + b
    assert torch.equal((v.double() - a.double()), b.double())                                   # the sum itself is exact in fp32
    assert torch.equal(v.bfloat16().float(), a)
    assert torch.equal((v.view(torch.int32) & -65536).view(torch.float32), a)
    rem = v - v.bfloat16().float()
    assert torch.equal(rem, b) and torch.equal(rem.bfloat16().float(), rem)
    assert len(TWO_PIECE_POINTS) >= 30 and {p.ws for p in TWO_PIECE_POINTS} == {0, 1}


@pytest.mark.parametrize('p', TWO_PIECE_POINTS, ids=lambda p: p.id)
def test_bf16x3_keeps_three_of_the_four_piece_products(p, monkeypatch):
    """The contract of STIN_GEMM_BF16X3 (stin_hip.h: "2 bf16 pieces, 3 bf16 MFMAs"): with G = Ga + Gb', X = Xa + Xb' split as
    above the result is Ga^T Xa + (Ga^T Xb' + Gb'^T Xa) - the Gb'^T Xb' term is NOT there.  Every term is a multiple of 2^-8 and
    |sum| <= 9.1 x 4096 < 2^16, so 9.1 x 4096 x 2^8 < 2^24: exact in any order.  The bias column is summed in fp32 from the
    unsplit G: sum w (Ga + Gb'), exact too.  Both MFMA kernels of fp32 rows (k_gemm_tn_bf16s<.., 2, ..>, k_gemm_tn_ws) keep
    exactly these three products."""
    T.set_env(monkeypatch, p.env)
    Gv, Ga, Gb = two_piece((p.M, p.Nc), 11 * p.M + p.Nc)
    Xv, Xa, Xb = two_piece((p.M, p.K), 13 * p.M + p.K)
    assert torch.equal(Gv.bfloat16().float(), Ga) and torch.equal((Gv - Ga).bfloat16().float(), Gb)
    assert torch.equal(Xv.bfloat16().float(), Xa) and torch.equal((Xv - Xa).bfloat16().float(), Xb)
    G, X = strided(Gv, p.padg, p.off), strided(Xv, p.padx, p.off)
    w = column(ints((p.M,), 17 * p.M, lo=0, hi=2))
    check_geometry(p, G, X)
    Ga, Gb, Xa, Xb = Ga.double(), Gb.double(), Xa.double(), Xb.double()
    want = Ga.t() @ Xa + (Ga.t() @ Xb + Gb.t() @ Xa)
    dropped = Gb.t() @ Xb
    assert float(dropped.abs().max()) > 0                          # (so leaving the term out is visible)
    want_b1, want_bw = G.double().sum(0), (G.double() * w.double()[:, None]).sum(0)
    all_forms_equal(p, G, X, w, want, want_b1, want_bw)


# ---------------------------------------------------------------------------------------------- X read as relu(bn(X))
def bn_product_is_exact(p, tf_off=0):
    """stin_gemm_tn_bn_f32: dW = G^T relu(X s + t), s = gamma rstd, t = beta - mean s (the form stin_hip.h documents).  Integer
    mean, beta in {-2 .. 2}, gamma in {-2 .. 2}, rstd in {0.5, 1, 2}: s, t and relu(X s + t) <= 22 are exact half-integers of
    at most 6 significant bits (one bf16 piece); |G X'| <= 66 in steps of 0.5 and 32 896 x 66 x 2 < 2^24: exact in any order.
    tf_off: the four transform vectors lie that many elements behind a 16-byte boundary, in buffers of POISON."""
    lib = _lib.load()
    G, X = ints((p.M, p.Nc), 3 * p.M + p.Nc), ints((p.M, p.K), 5 * p.M + p.K)
    if tf_off == 0:
        check_geometry(p, G, X, ones=0)
    else:       # the query takes no transform: it answers for the aligned form, whose tile and chunks this route keeps
        g = T.geometry(lib, 0, p.M, p.Nc, p.K, p.Nc, p.K, 1, 0, p.prec)
        assert (g['tile'], g['chunks']) == (p.tile, p.chunks) and G.data_ptr() % 16 == 0 and X.data_ptr() % 16 == 0
    mean, beta, gamma = (ints((p.K,), 19 + i + p.K, lo=-2, hi=2) for i in range(3))
    rstd = torch.tensor([0.5, 1.0, 2.0], device=DEV)[ints((p.K,), 23 + p.K, lo=0, hi=2).long()]
    if tf_off:
        mean, beta, gamma, rstd = (strided(v[None, :], 4, tf_off)[0] for v in (mean, beta, gamma, rstd))
        assert all(v.data_ptr() % 16 == 4 * tf_off and v.is_contiguous() for v in (mean, beta, gamma, rstd))
    s = gamma.double() * rstd.double()
    t = beta.double() - mean.double() * s
    Xn = torch.relu(X.double() * s + t)
    assert float(Xn.max()) <= 22 and torch.equal(Xn.float().bfloat16().double(), Xn) and torch.equal(Xn * 2, (Xn * 2).round())
    want = G.double().t() @ Xn
    buf, dW = guarded(p.Nc, p.K)
    ws_bytes = lib.stin_gemm_tn_workspace_bytes(p.M, p.Nc, p.K, 0)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    SF._call('stin_gemm_tn_bn_f32', SF._ptr(G), p.Nc, SF._ptr(X), p.K, SF._ptr(mean), SF._ptr(rstd), SF._ptr(gamma), SF._ptr(beta), p.M,
             p.Nc, p.K, SF._ptr(dW), dW.stride(0), int(p.prec), SF._ptr(ws), ws_bytes, SF._stream(G))
    assert untouched(buf, dW)
    assert torch.equal(dW.double(), want), p.id
    assert torch.equal(SCMN._gemm_tn_bn(G, X, mean, rstd, gamma, beta, p.prec), dW), p.id


@pytest.mark.parametrize('p', T.BN_POINTS, ids=lambda p: p.id)
def test_tn_bn_product_of_integers_is_exact(p, monkeypatch):
    T.set_env(monkeypatch, p.env)
    bn_product_is_exact(p)


def test_tn_bn_product_with_unaligned_transform_vectors_is_exact(monkeypatch):
    """bf16x3 on aligned operands whose transform vectors are no 16-byte vectors.  tn_route (csrc/gemm_tn_route.inc) gives this
    the tile and chunks of the producer / consumer route on the four-wave kernel without 16-byte loads.  Asserted here: the exact
    product, intact guards, and the tile and chunks of the aligned form.  NOT asserted: which kernel ran - the query takes no
    transform; a kernel trace recorded it once (profiles/r24_tn_routes.md)."""
    T.set_env(monkeypatch, {})
    bn_product_is_exact(T.BN_UNALIGNED_TF_POINT, tf_off=1)


def test_tn_bn_refuses_the_skinny_shape():
    G, X = ints((300, 64), 1), ints((300, 12), 2)
    v = ints((12,), 3)
    with pytest.raises(_lib.StinError):
        SCMN._gemm_tn_bn(G, X, v, v, v, v, T.X3)


# ---------------------------------------------------------------------------------------------- the block entry points
def block_operands(shape, shortcut, ti, storage, N, rows_x=None, seed=0):
    Cin, Cp, H, Cout = shape
    dt = DT[storage]
    Yw = T.block_yw(H, Cout, shortcut, ti)
    dagg = ints((N, Cout), N + seed + 1, dt)
    hE = torch.full((N, H + 4), POISON, dtype=dt, device=DEV)          # columns behind the indicator are never read
    hE[:, :H] = ints((N, H), N + seed + 2, dt)
    hE[:, H] = ints((N,), N + seed + 3, dt, 0, 1)                       # the [deg > 0] column: weights of db2
    dY = ints((N, Yw), N + seed + 4, dt)
    nx = N if rows_x is None else rows_x
    x = torch.zeros(nx, Cp, dtype=dt, device=DEV)                       # zero-padded from Cin to Cp columns
    x[:, :Cin] = ints((nx, Cin), N + seed + 5, dt)
    return dagg, hE, dY, x


def block_reference(dagg, hE, dY, x, shape, shortcut, ti):
    """fp64 autograd through the packed forward as the pack comment of stin_hip.h defines it:
    Y = x wcat^T + bcat, wcat = [Wa - Wb ; Wb ; Ws] (trans_inv: [-W1 ; W1 ; Ws], compact: [W1 ; Ws]), bcat = [b1 ; 0 ; bs]
    (compact: [0 ; bs]), contracted with dY; the second Linear h W2^T + [deg > 0] b2 contracted with dagg.
    -> [dW1, db1 (None: compact), dW2, db2, dWs, dbs]"""
    Cin, Cp, H, Cout = shape
    kw = dict(dtype=torch.float64, device=DEV, requires_grad=True)
    W1, b1 = torch.zeros(H, Cin if ti else 2 * Cin, **kw), torch.zeros(H, **kw)
    W2, b2 = torch.zeros(Cout, H, **kw), torch.zeros(Cout, **kw)
    Ws, bs = torch.zeros(Cout, Cin, **kw), torch.zeros(Cout, **kw)
    zero = torch.zeros(H, dtype=torch.float64, device=DEV)
    if ti == 0:
        rows, bias = [W1[:, :Cin] - W1[:, Cin:], W1[:, Cin:]], [b1, zero]
    elif ti == 1:
        rows, bias = [-W1, W1], [b1, zero]
    else:
        rows, bias = [W1], [zero]
    if shortcut:
        rows, bias = rows + [Ws], bias + [bs]
    Y = x[:, :Cin].double() @ torch.cat(rows).t() + torch.cat(bias)
    out = hE[:, :H].double() @ W2.t() + hE[:, H:H + 1].double() * b2
    loss = (Y * dY.double()).sum() + (out * dagg.double()).sum()
    g = torch.autograd.grad(loss, [W1, b1, W2, b2, Ws, bs], allow_unused=True)
    return [None if (t is None or (i >= 4 and not shortcut)) else t for i, t in enumerate(g)]


def block_call(entry, storage, dagg, hE, dY, x, N, shape, shortcut, ti, prec, extra=()):
    lib = _lib.load()
    Cin, Cp, H, Cout = shape
    outs = [guarded_flat(H, Cin if ti else 2 * Cin), guarded_flat(H), guarded_flat(Cout, H), guarded_flat(Cout),
            guarded_flat(Cout, Cin), guarded_flat(Cout)]
    ws_bytes = lib.stin_edgeconv_wgrad_workspace_bytes(N, Cp, H, Cout, shortcut)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    ptrs = [SF._ptr(v) if (i < 4 or shortcut) else 0 for i, (_, v) in enumerate(outs)]
    SF._call(entry, storage, SF._ptr(dagg), dagg.stride(0), SF._ptr(hE), hE.stride(0), SF._ptr(dY), dY.stride(0), SF._ptr(x), x.stride(0),
             N, Cin, Cp, H, Cout, shortcut, ti, int(prec), *ptrs, *extra, SF._ptr(ws), ws_bytes, SF._stream(dagg))
    got = []
    for i, (buf, v) in enumerate(outs):
        if i < 4 or shortcut:
            assert untouched(buf, v), i
            got.append(v.clone())
        else:
            assert bool((buf == FILL).all()), i                          # no shortcut: dWs / dbs are not written
            got.append(None)
    return got


def same(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        if b is not None:
            assert a.shape == b.shape and torch.equal(a.double(), b), (what, 'dW1 db1 dW2 db2 dWs dbs'.split()[i])


def check_block_geometry(shape, shortcut, ti, storage, N, prec, dagg, hE, dY, x_ld):
    lib = _lib.load()
    args = T.block_products(shape, shortcut, ti, storage, N, prec)
    assert (args[0][4], args[0][5], args[1][4], args[1][5]) == (dagg.stride(0), hE.stride(0), dY.stride(0), x_ld)
    ga, gb = (T.geometry(lib, *a) for a in args)
    for g in (ga, gb):
        assert g['chunks'] * g['rows'] >= N > (g['chunks'] - 1) * g['rows']
        if g['tiles'] == (1, 1):
            assert g['chunks'] == (N + 127) // 128
    return ga, gb


@pytest.mark.parametrize('case', list(T.block_cases()), ids=lambda c: '%s-sc%d-ti%d-st%d-p%d-n%d' % ('x'.join(map(str, c[0])), *c[1:]))
def test_block_weight_gradients_of_integers_are_exact(case, monkeypatch):
    """All six gradients of stin_edgeconv_wgrad / stin_edgeconv_wgrad_ti against fp64 autograd through the packed forward; the
    geometry of both products from the query (tests/test_tn_geometry.py::test_block_products_geometry names what each shape
    reaches).  Compact layout: db1 = the column sum of the integer ti_colsum rows, from the finalize launch and from
    stin_edge_bwd_ti_colsum_fold_f32 alone."""
    T.set_env(monkeypatch, {})
    shape, shortcut, ti, storage, prec, N = case
    Cin, Cp, H, Cout = shape
    dagg, hE, dY, x = block_operands(shape, shortcut, ti, storage, N)
    check_block_geometry(shape, shortcut, ti, storage, N, prec, dagg, hE, dY, x.stride(0))
    want = block_reference(dagg, hE, dY, x, shape, shortcut, ti)
    assert float(want[2].abs().max()) < 2 ** 24 and float(want[0].abs().max()) < 2 ** 24
    if ti == 2:
        entry = 'stin_edgeconv_wgrad_ti'                                # (the only entry point of the compact layout)
        rows = T.COLSUM_ROWS[T.BLOCK_NS.index(N) % len(T.COLSUM_ROWS)]
        colsum = ints((rows, H), N + rows)
        want[1] = colsum.double().sum(0)
        extra = (SF._ptr(colsum), rows)
        fbuf, folded = guarded_flat(H)
        SF._call('stin_edge_bwd_ti_colsum_fold_f32', SF._ptr(colsum), rows, H, SF._ptr(folded), SF._stream(colsum))
        assert untouched(fbuf, folded) and torch.equal(folded.double(), want[1])
    else:
        entry, extra = 'stin_edgeconv_wgrad', ()
    got = block_call(entry, storage, dagg, hE, dY, x, N, shape, shortcut, ti, prec, extra)
    same(got, want, 'first call')
    same(block_call(entry, storage, dagg, hE, dY, x, N, shape, shortcut, ti, prec, extra), want, 'second call of the same entry point')
    if ti != 2:     # and stin_edgeconv_wgrad_ti in the plain modes, which ignore its two extra arguments (stin_hip.h): the same gradients
        same(block_call('stin_edgeconv_wgrad_ti', storage, dagg, hE, dY, x, N, shape, shortcut, ti, prec, (0, 0)), want, '_ti entry point')


MAP_CASES = [(shape, sc, ti, N) for shape in T.BLOCK_MAP_SHAPES for sc in (0, 1) for ti in (0, 1) for N in T.BLOCK_MAP_NS]


@pytest.mark.parametrize('case', MAP_CASES, ids=lambda c: '%s-sc%d-ti%d-n%d' % ('x'.join(map(str, c[0])), *c[1:]))
def test_mapped_block_weight_gradients_of_integers_are_exact(case, monkeypatch):
    """stin_edgeconv_wgrad_map where stin_edgeconv_wgrad_map_supported says 1 (the packed product on the producer / consumer kernel):
    x is [N // 3, Cp], read through an int32 map with repeats and with coarse rows that no fine row names; N is no multiple of 4, so
    the last slab's map entries are read one by one.  Rows of 1e30 follow x and entries naming them follow the map."""
    T.set_env(monkeypatch, {})
    shape, shortcut, ti, N = case
    lib = _lib.load()
    Cin, Cp, H, Cout = shape
    assert lib.stin_edgeconv_wgrad_map_supported(N, Cp, H, Cout, shortcut, T.X3) == 1
    assert N % 4 != 0
    n_in = N // 3
    dagg, hE, dY, xs = block_operands(shape, shortcut, ti, 0, N, rows_x=n_in)
    ga, gb = check_block_geometry(shape, shortcut, ti, 0, N, T.X3, dagg, hE, dY, Cp)
    assert gb['ws'] == 1
    x_big = torch.full((n_in + 64, Cp), POISON, device=DEV)
    x_big[:n_in] = xs
    g = torch.Generator(device=DEV).manual_seed(N)
    used = torch.arange(n_in, device=DEV)
    used = used[used % 7 != 3]                                          # coarse rows that no fine row names
    m = used[torch.randint(0, len(used), (N,), generator=g, device=DEV)]
    m[:5] = m[5]                                                        # repeats
    m[7], m[N - 1] = 0, n_in - 1
    assert len(torch.unique(m)) < n_in
    map_buf = torch.full((N + 64,), n_in + 63, dtype=torch.int32, device=DEV)
    map_buf[:N] = m.to(torch.int32)
    want = block_reference(dagg, hE, dY, x_big[m], shape, shortcut, ti)
    extra = (SF._ptr(map_buf), n_in)
    got = block_call('stin_edgeconv_wgrad_map', 0, dagg, hE, dY, x_big, N, shape, shortcut, ti, T.X3, extra)
    same(got, want, 'first call')
    again = block_call('stin_edgeconv_wgrad_map', 0, dagg, hE, dY, x_big, N, shape, shortcut, ti, T.X3, extra)
    same(again, [None if t is None else t.double() for t in got], 'second call')
