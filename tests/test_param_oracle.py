"""tests/_param_oracle.py held to first principles on the CPU - never to the kernels: the split pieces reconstruct the value,
every layout is a bijection onto its buffer and decodes to the logical matrix, the packed operands compute the reference block's
first Linear, unpack is the adjoint of pack, Adam follows torch.optim.Adam, the loss follows oracle/stin_oracle.py and the graph
metrics the formulas of the g8_metrics fixture; plus layouts typed out by hand.  tests/test_param_exact_gpu.py then holds the
device to the restatement with `==`."""
import os
import re

import numpy as np
import pytest
import torch

import _param_oracle as O
from _golden import load_npz
from oracle import stin_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16, WB16, FRAG = O.GEMM_F16X3, O.GEMM_BF16X3, O.GEMM_W_BF16, O.GEMM_W_FRAG
U = 2.0 ** -24                                            # unit roundoff of fp32


def test_constants_are_the_headers():
    text = open(os.path.join(ROOT, 'include', 'stin_hip.h')).read()
    for name, value in (('STIN_GEMM_BF16X3', BF16), ('STIN_GEMM_F16X3', F16), ('STIN_GEMM_W_BF16', WB16), ('STIN_GEMM_W_FRAG', FRAG),
                        ('STIN_TI_COMPACT', O.TI_COMPACT)):
        assert int(re.search(r'#define\s+%s\s+(\S+)' % name, text).group(1), 0) == value


# ------------------------------------------------------------------ pieces
def _domain_values(rng, n):
    """2^-9 <= |w| < 1023, log-uniform, both signs, mixed with values whose lo piece is zero in either format."""
    w = np.exp2(rng.uniform(-9, np.log2(1023), n)) * rng.choice([-1.0, 1.0], n)
    w = w.astype(np.float32)
    w[::7] = (w[::7].view(np.uint32) & 0xFFFF0000).view(np.float32)          # exactly bf16
    w[3::7] = (w[3::7].view(np.uint32) & 0xFFFFE000).view(np.float32)        # 11 significant bits: exactly fp16 after x 64
    return np.clip(w, -1022.0, 1022.0).astype(np.float32)


def test_split16_reconstructs_within_the_piece_accuracy():
    """bf16 pieces carry 8 significant bits each: |v - hi| <= 2^-8 |v| and the rounding of that residual adds at most 2^-8 of
    it: 2^-16 |v|.  fp16 pieces carry 11: 2^-22 |v| while lo is a normal fp16 number or s >= 2^-3 (|w| >= 2^-9: an fp16
    subnormal lo is within 2^-25 of the residual); below that domain only the absolute 2^-25 / 64 = 2^-31 holds."""
    rng = np.random.default_rng(1)
    w = _domain_values(rng, 20000)
    w64 = w.astype(np.float64)
    for prec, rel in ((BF16, 2.0 ** -16), (F16, 2.0 ** -22)):
        hi, lo = O.split16(w, prec)
        assert np.all(np.abs(O.join16(hi, lo, prec) - w64) <= rel * np.abs(w64))
    exact = (w.view(np.uint32) & 0xFFFF) == 0
    assert exact.sum() > 1000 and np.all(O.split16(w[exact], BF16)[1] == 0)
    exact = (w.view(np.uint32) & 0x1FFF) == 0
    assert np.all((O.split16(w[exact], F16)[1] & 0x7FFF) == 0)
    tiny = (np.exp2(rng.uniform(-30, -9, 5000)) * rng.choice([-1.0, 1.0], 5000)).astype(np.float32)
    hi, lo = O.split16(tiny, F16)
    assert np.all(np.abs(O.join16(hi, lo, F16) - tiny.astype(np.float64)) <= 2.0 ** -31)


def test_split16_typed_out():
    v = np.array([1.0, 2.0, 3.0, 1.0 + 2.0 ** -9, -1.0], np.float32)
    hi, lo = O.split16(v, BF16)
    assert hi.tolist() == [0x3F80, 0x4000, 0x4040, 0x3F80, 0xBF80] and lo.tolist() == [0, 0, 0, 0x3B00, 0]
    v = np.array([1.0, 0.5, -1.0, 1.0 + 2.0 ** -12], np.float32)             # x 64: 64, 32, -64, 64 + 2^-6
    hi, lo = O.split16(v, F16)
    assert hi.tolist() == [0x5400, 0x5000, 0xD400, 0x5400] and lo.tolist() == [0, 0, 0x0000, 0x2400]
    # round to nearest EVEN: 1 + 2^-8 lies halfway between the bf16 neighbours 1 and 1 + 2^-7
    assert O.bf16_bits(np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], np.float32)).tolist() == [0x3F80, 0x3F82]


# ------------------------------------------------------------------ layouts
def test_kgroup_layout_typed_out():
    W = np.array([[1.0, 2.0, 3.0, 1.0 + 2.0 ** -9]], np.float32)
    assert O.encode(W, BF16).tolist() == [0x3F80, 0x4000, 0x4040, 0x3F80, 0, 0, 0, 0x3B00]
    W = np.arange(1, 17, dtype=np.float32).reshape(2, 8)                     # small integers: hi = bf16(v), lo = 0
    hi = O.bf16_bits(W)
    want = []
    for r in range(2):
        for g in range(2):
            want += hi[r, 4 * g:4 * g + 4].tolist() + [0] * 4
    assert O.encode(W, BF16 | FRAG).tolist() == want                         # 2 x 8 is no fragment shape: the flag changes nothing
    # ld = 12 fp32 elements: row 1 starts at half 24, the 8 halves between the rows keep the fill
    got = O.encode(W, BF16, ld=12, fill=0xABCD)
    assert got.shape == (40,) and got[:16].tolist() == want[:16] and got[24:].tolist() == want[16:] and set(got[16:24].tolist()) == {0xABCD}


def test_plain_layouts_typed_out():
    W = np.array([[1.0, -2.0], [0.5, 3.0]], np.float32)
    assert O.encode(W, 0).view(np.uint32).tolist() == [0x3F800000, 0xC0000000, 0x3F000000, 0x40400000]
    assert O.encode(W, WB16).tolist() == [0x3F80, 0xC000, 0x3F00, 0x4040]


def test_fragment_tile_typed_out():
    """One 32 x 16 tile: lane L < 32 holds row L, columns 0 .. 7 as [hi x 8 | lo x 8]; lane 32 + L holds columns 8 .. 15."""
    rng = np.random.default_rng(2)
    W = rng.standard_normal((32, 16)).astype(np.float32)
    hi, lo = O.split16(W, F16)
    want = []
    for lane in range(64):
        r, c0 = lane % 32, 8 * (lane // 32)
        want += hi[r, c0:c0 + 8].tolist() + lo[r, c0:c0 + 8].tolist()
    idx = O.frag_index(32, 16)
    got = np.zeros(1024, np.uint16)
    got[idx.reshape(-1)] = hi.reshape(-1)
    got[idx.reshape(-1) + 8] = lo.reshape(-1)
    assert got.tolist() == want
    # beyond the first tile: tile t = r >> 5 and step s = c >> 4 own 2 KB = 1024 halves at (t * K / 16 + s)
    idx = O.frag_index(64, 32)
    assert idx[0, 0] == 0 and idx[0, 16] == 1024 and idx[32, 0] == 2048 and idx[32, 16] == 3072 and idx[33, 27] == 3603
    idx = O.frag_index(320, 128)
    assert idx[319, 127] + 8 == 2 * 320 * 128 - 1                            # the last lo piece is the last half of the buffer


def test_frag_shape_typed_out():
    yes = [(320, 128), (320, 256), (352, 192), (1024, 128), (256, 512), (256, 1024), (128, 256), (128, 512)]
    no = [(288, 128), (320, 64), (320, 320), (336, 128), (320, 512), (256, 256), (256, 448), (128, 128), (128, 192), (96, 128),
          (64, 512), (320, 130), (512, 512)]
    assert all(O.frag_shape(*s) for s in yes) and not any(O.frag_shape(*s) for s in no)


LAYOUT_CASES = [(1, 4, BF16, None), (5, 8, F16, 11), (5, 8, BF16 | FRAG, 12), (96, 128, F16 | FRAG, None), (320, 128, F16 | FRAG, None),
                (128, 256, BF16 | FRAG, None), (128, 256, BF16, 260), (256, 512, F16 | FRAG, None), (3, 8, WB16, 16), (3, 5, 0, 7)]


@pytest.mark.parametrize('nc,kk,mode,ld', LAYOUT_CASES)
def test_layouts_are_bijections_and_decode(nc, kk, mode, ld):
    rng = np.random.default_rng(nc + kk)
    W = _domain_values(rng, nc * kk).reshape(nc, kk)
    buf = O.encode(W, mode, ld, fill=0xABCD)
    prec = mode & ~FRAG
    if prec in (F16, BF16):
        hi, lo, n = O.split_layout(nc, kk, mode, ld)
        both = np.concatenate([hi.reshape(-1), lo.reshape(-1)])
        assert buf.shape == (n,) and np.unique(both).size == 2 * nc * kk and both.min() >= 0 and both.max() < n
        if ld in (None, kk) or ((mode & FRAG) and O.frag_shape(nc, kk)):
            assert n == 2 * nc * kk                                          # onto: every half of the buffer is written once
        else:
            owned = np.zeros(n, bool)
            owned[both] = True
            assert np.all(buf[~owned] == 0xABCD)
        assert ((mode & FRAG) and O.frag_shape(nc, kk)) == (not np.array_equal(hi, O.kgroup_index(nc, kk, ld)))
        rel = 2.0 ** -16 if prec == BF16 else 2.0 ** -22
    else:
        rel = 2.0 ** -8 if prec == WB16 else 0.0
    assert np.all(np.abs(O.decode(buf, nc, kk, mode, ld) - W.astype(np.float64)) <= rel * np.abs(W))


# ------------------------------------------------------------------ pack / unpack
def _params(rng, Cin, H, Cout, shortcut, ti, dtype, b1=True, bs=True):
    r = lambda *s: rng.standard_normal(s).astype(dtype)
    return dict(W1=r(H, Cin if ti else 2 * Cin), b1=r(H) if b1 else None, Ws=r(Cout, Cin) if shortcut else None,
                bs=r(Cout) if shortcut and bs else None, W2=r(Cout, H))


@pytest.mark.parametrize('ti', [0, 1, 2])
@pytest.mark.parametrize('Cin,Cp,shortcut,b1', [(3, 4, True, True), (10, 16, True, False), (6, 6, False, True)])
def test_packed_operands_compute_the_blocks_first_linear(ti, Cin, Cp, shortcut, b1):
    """oracle/stin_oracle.py: the EdgeConv message is nn([x_i ; x_j - x_i]) and the translation-invariant one nn(x_j - x_i) with
    nn.0 = Linear(W1, b1); the block's shortcut is Linear(Ws, bs)(x).  With Y = x_pad wcat^T + bcat: Lin1 = A_i + B_j, A = Y[:, :H],
    B = Y[:, H:2H]; compact: B = Y[:, :H] and A_i = b1 - B_i.  fp64 throughout."""
    rng = np.random.default_rng(10 * ti + Cin)
    H, Cout, N = 5, 4, 9
    p = _params(rng, Cin, H, Cout, shortcut, ti, np.float64, b1=b1, bs=b1)
    x = rng.standard_normal((N, Cin))
    x_pad = np.concatenate([x, rng.standard_normal((N, Cp - Cin))], 1)       # whatever sits in the padding must not matter ...
    wcat, bcat = O.edgeconv_pack_values(p['W1'], p['b1'], p['Ws'], p['bs'], Cin, Cp, H, Cout, shortcut, ti)
    assert wcat.shape == (O.yw_of(H, Cout, shortcut, ti), Cp) and np.all(wcat[:, Cin:] == 0)      # ... because these are zeros
    Y = x_pad @ wcat.T + bcat
    i, j = rng.integers(0, N, 40), rng.integers(0, N, 40)
    bias1 = p['b1'] if b1 else np.zeros(H)
    msg_in = x[j] - x[i] if ti else np.concatenate([x[i], x[j] - x[i]], 1)
    want = msg_in @ p['W1'].T + bias1
    if ti == O.TI_COMPACT:
        B = Y[:, :H]
        A = bias1 - B
        assert np.all(bcat[:H] == 0)
    else:
        A, B = Y[:, :H], Y[:, H:2 * H]
    assert np.abs(A[i] + B[j] - want).max() <= 1e-12
    if shortcut:
        assert np.abs(Y[:, -Cout:] - (x @ p['Ws'].T + (p['bs'] if b1 else 0.0))).max() <= 1e-12


@pytest.mark.parametrize('ti', [0, 1, 2])
@pytest.mark.parametrize('Cin,Cp,shortcut,second', [(3, 4, True, True), (10, 12, True, False), (5, 5, False, True)])
def test_unpack_is_the_adjoint_of_pack(ti, Cin, Cp, shortcut, second):
    """<unpack(dwb), params> = <dwb, [wcat | bcat]> for every dwb: unpack is the transpose of the linear map pack (fp64)."""
    rng = np.random.default_rng(20 * ti + Cp)
    H, Cout = 6, 7
    p = _params(rng, Cin, H, Cout, shortcut, ti, np.float64)
    Yw = O.yw_of(H, Cout, shortcut, ti)
    wcat, bcat = O.edgeconv_pack_values(p['W1'], p['b1'], p['Ws'], p['bs'], Cin, Cp, H, Cout, shortcut, ti)
    dwb = rng.standard_normal((Yw, Cp + 1))
    dw2b = rng.standard_normal((Cout, H + 1)) if second else None
    g = O.edgeconv_unpack(dwb, dw2b, Cin, Cp, H, Cout, shortcut, ti)
    assert g['dW1'].shape == p['W1'].shape and (g['db1'] is None) == (ti == O.TI_COMPACT)
    assert (g['dWs'] is None) == (not shortcut) and (g['dbs'] is None) == (not shortcut)
    lhs = sum(float((g[k] * p[n]).sum()) for k, n in (('dW1', 'W1'), ('db1', 'b1'), ('dWs', 'Ws'), ('dbs', 'bs')) if g[k] is not None)
    rhs = float((dwb[:, :Cp] * wcat).sum() + (dwb[:, Cp] * bcat).sum())
    assert abs(lhs - rhs) <= 1e-12 * (abs(rhs) + 1.0)
    if second:
        assert np.array_equal(g['dW2'], dw2b[:, :H]) and np.array_equal(g['db2'], dw2b[:, H])
    else:
        assert g['dW2'] is None and g['db2'] is None


def test_edgeconv_pack_encodes_each_operand_on_its_own_shape():
    rng = np.random.default_rng(5)
    Cin = Cp = 128
    H, Cout = 128, 64
    p = _params(rng, Cin, H, Cout, True, 0, np.float32)
    out = O.edgeconv_pack(p['W1'], p['b1'], p['Ws'], p['bs'], p['W2'], Cin, Cp, H, Cout, True, 0, F16 | FRAG, BF16 | FRAG)
    wcat, bcat = O.edgeconv_pack_values(p['W1'], p['b1'], p['Ws'], p['bs'], Cin, Cp, H, Cout, True, 0)
    assert wcat.dtype == np.float32 and np.array_equal(wcat[:H], p['W1'][:, :Cin] - p['W1'][:, Cin:])
    assert O.frag_shape(320, 128) and np.array_equal(out['wcat'], O.encode(wcat, F16 | FRAG))
    assert O.frag_shape(128, 320) and not np.array_equal(out['wcatT'], O.encode(wcat.T, BF16))     # Nc = 128 with K = 320: fragment order
    assert np.abs(O.decode(out['wcatT'], Cp, 320, BF16 | FRAG) - wcat.T).max() <= 2.0 ** -16 * np.abs(wcat).max()
    assert np.array_equal(out['w2s'], O.encode(p['W2'], F16)) and np.array_equal(out['w2T'], O.encode(p['W2'].T, BF16))    # 64 x 128, 128 x 64: k-group
    assert np.abs(O.decode(out['w2T'], H, Cout, BF16) - p['W2'].T).max() <= 2.0 ** -16 * np.abs(p['W2']).max()
    assert np.array_equal(out['bcat'].view(np.float32), bcat)


def test_scmn_pack_and_unpack_are_adjoint_and_compute_the_layers_first_linear():
    rng = np.random.default_rng(6)
    cin, h2, cout = 3, 4, 5
    for ti in (0, 1):
        W1, W2 = rng.standard_normal((h2, cin if ti else 2 * cin)), rng.standard_normal((cout, h2))
        g1, b1, g2, b2 = (rng.standard_normal(n) for n in (h2, h2, cout, cout))
        o = O.scmn_pack(W1, W2, g1, b1, g2, b2, cin, h2, cout, ti)
        x = rng.standard_normal((8, cin))
        i, j = rng.integers(0, 8, 20), rng.integers(0, 8, 20)
        Y = x @ o['wcat'].T
        msg_in = x[j] - x[i] if ti else np.concatenate([x[i], x[j] - x[i]], 1)
        assert np.abs(Y[i, :h2] + Y[j, h2:] - msg_in @ W1.T).max() <= 1e-12
        assert np.array_equal(o['wcatT'], o['wcat'].T) and np.array_equal(o['w2T'], W2.T)
        assert np.array_equal(o['gb1'], np.stack([g1, b1])) and np.array_equal(o['gb2'], np.stack([g2, b2]))
        d = rng.standard_normal((2 * h2, cin))
        assert abs(float((O.scmn_unpack(d, cin, h2, ti) * W1).sum()) - float((d * o['wcat']).sum())) <= 1e-12


# ------------------------------------------------------------------ elementwise passes
def test_elementwise_restatements_typed_out():
    nan = np.float32('nan')
    x = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, -6.0]], np.float32)
    mean, rstd = np.array([1.0, 1.0], np.float32), np.array([2.0, 0.5], np.float32)
    gamma, beta = np.array([1.0, -1.0], np.float32), np.array([0.5, 0.25], np.float32)
    rowptr = np.array([0, 1, 1, 3], np.int32)                                # row 1 has no in-edge
    res = np.array([[1.0, 1.0], [-7.0, 7.0], [0.0, 0.0]], np.float32)
    y = O.bn_affine_res(x, mean, rstd, gamma, beta, rowptr, res, relu=1)
    assert y.tolist() == [[1.5, 0.75], [0.0, 7.0], [8.5, 3.75]]
    y = O.bn_affine_res(x, mean, rstd, gamma, beta, None, None, relu=0)
    assert y.tolist() == [[0.5, -0.25], [4.5, -1.25], [8.5, 3.75]]
    g = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]], np.float32)
    yy = np.array([[0.0, -0.0], [nan, 1.0], [2.0, -1.0]], np.float32)
    ge, gi = O.relu_mask_bwd(g, yy, rowptr, relu=1)
    assert ge.tolist() == [[0.0, 0.0], [0.0, 4.0], [5.0, 0.0]] and gi.tolist() == [[0.0, 0.0], [0.0, 0.0], [5.0, 0.0]]
    ge, gi = O.relu_mask_bwd(g, yy, None, relu=0)
    assert np.array_equal(ge, g) and np.array_equal(gi, g)
    out = O.cols_axpy_rowmask(g, x, rowptr, 1, 2, -1.0)
    assert out.tolist() == [[1.0, 0.0], [3.0, 4.0], [5.0, 12.0]]
    b = O.cols_axpy_rowmask(O.bf16_bits(g), O.bf16_bits(x), rowptr, 0, 2, 0.5, bf16=True)
    assert O.bf16_value(b).tolist() == [[1.5, 3.0], [3.0, 4.0], [7.5, 3.0]]
    assert O.pad_rows(np.arange(6, dtype=np.float32).reshape(2, 3), 2, 4).tolist() == [[0.0, 1.0, 0.0, 0.0], [3.0, 4.0, 0.0, 0.0]]
    T1, S0 = np.array([[2.0, 3.0]], np.float32), np.array([[4.0, 5.0]], np.float32)
    r, ic = np.array([[2.0, 0.5]], np.float32), np.array([0.25], np.float32)
    k, m = O.norm_bwd_coef(T1, S0, r, ic)
    assert k.tolist() == [[-4.0, -0.09375]] and m.tolist() == [[-2.0, -0.625]]
    assert O.norm_bwd_coef_m_quirk(S0, T1, r, ic).tolist() == [[-2.5, -1.375]]


# ------------------------------------------------------------------ Adam
@pytest.mark.parametrize('amsgrad,wd', [(True, 0.0), (False, 0.0), (True, 0.01)])
def test_adam_restatement_follows_torch_adam(amsgrad, wd):
    g = torch.Generator().manual_seed(9)
    p0 = torch.randn(1027, generator=g)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref], lr=7e-5, weight_decay=wd, amsgrad=amsgrad)
    p = p0.numpy().copy()
    m, v, vm = (np.zeros_like(p) for _ in range(3))
    for step in range(1, 6):
        grad = torch.randn(1027, generator=g) * (0.1 if step != 3 else 10.0)
        ref.grad = grad.clone()
        opt.step()
        p, m, v, vm = O.adam(p, grad.numpy(), m, v, vm if amsgrad else None, 7e-5, 0.9, 0.999, 1e-8, wd, step, int(amsgrad))
        assert float(np.abs(p - ref.detach().numpy()).max()) <= 5e-7, step
    assert vm is None or np.all(vm >= v)


# ------------------------------------------------------------------ loss and graph metrics
def _loss_case(rng, N, C):
    out = rng.uniform(-1, 1, (N, C)).astype(np.float32)
    color = rng.uniform(-1, 1, (N, C)).astype(np.float32)
    mask = rng.choice(np.array([0, 0, 0, 1, 2, 16, 17, 64, 300]), N).astype(np.int64)
    out[::5] = color[::5]
    return out, color, mask


@pytest.mark.parametrize('N,C', [(2, 1), (85, 3), (700, 4)])       # (N = 1: the oracle's own squeeze() drops the vertex axis)
@pytest.mark.parametrize('use_weight', [0, 1])
def test_masked_l1_restatement_follows_the_oracles_loss(N, C, use_weight):
    """Against stin_oracle.compute_loss in fp64 on the same fp32 inputs.  Every term is non-negative and carries three roundings
    (the difference, the weight, their product), the sum is exact to fp64, then inv, the product with it and the cast: the loss is
    within 6 u, a gradient entry w * inv within 4 u, relative (u = 2^-24); plus what the two bases of the power differ by."""
    rng = np.random.default_rng(N)
    out, color, mask = _loss_case(rng, N, C)
    w = np.power(np.float64(np.float32(0.99)), mask.astype(np.float64)).astype(np.float32)
    grad, loss = O.masked_l1(out, color, mask, use_weight, w)
    o64 = torch.from_numpy(out).double().requires_grad_(True)
    c64, m = torch.from_numpy(color).double(), torch.from_numpy(mask)
    pred = torch.where((m > 0)[:, None].expand_as(c64), o64, c64)
    want = stin_oracle.compute_loss(pred, c64, m.double()[:, None] if use_weight else None)
    want.backward()
    want = want.detach()
    # compute_loss raises the double 0.99, the kernel's contract the float: (a (1 + d))^m = a^m (1 + m d + ..), m <= 300
    base = 300 * 1.001 * abs(float(np.float32(0.99)) - 0.99) / 0.99 if use_weight else 0.0
    assert loss.dtype == np.float32 and grad.dtype == np.float32
    assert abs(float(loss) - float(want)) <= (6 * U + base) * float(want)
    assert np.all(np.abs(grad - o64.grad.numpy()) <= (4 * U + base) * np.abs(o64.grad.numpy()))
    assert np.all(grad[mask <= 0] == 0) and np.all(grad[::5] == 0)


def test_fixed_order_sums_typed_out():
    """The order matters only in the last bits: terms chosen so that each order gives a different fp64 result."""
    t = np.zeros(512)
    t[0], t[128], t[1] = 1.0, 2.0 ** -53, 2.0 ** -53      # tree: (t0 + t128) rounds to 1, + (t1 + ..) -> 1 + 2^-53 rounds to 1
    assert O.block_sums(t).tolist() == [1.0, 0.0]
    t[128], t[129] = 0.0, 2.0 ** -53                      # now t1 + t129 = 2^-52 joins first: 1 + 2^-52
    assert O.block_sums(t).tolist() == [1.0 + 2.0 ** -52, 0.0]
    p = np.zeros(600)
    p[0], p[256], p[512] = 1.0, 2.0 ** -53, 2.0 ** -53    # thread 0: (1 + 2^-53) + 2^-53 = 1 (twice rounded down), not 1 + 2^-52
    p[1], p[257] = 2.0 ** -53, 2.0 ** -53                 # thread 1: 2^-52, joins thread 0 in the last tree step
    assert O.final_sum(p, np.float32(1.0)) == np.float32(1.0)
    assert float(_final64(p)) == 1.0 + 2.0 ** -52
    assert O.final_sum(np.array([3.0]), np.float32(0.5)) == np.float32(1.5)


def _final64(p):
    acc = np.zeros(256)
    for k in range(0, p.shape[0], 256):
        row = np.zeros(256)
        row[:min(256, p.shape[0] - k)] = p[k:k + 256]
        acc = acc + row
    return O._tree256(acc[None, :])[0]


def _csr(ei, N):
    src, dst = ei[0].astype(np.int64), ei[1].astype(np.int64)
    order = np.argsort(dst, kind='stable')
    rowptr = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(dst, minlength=N), out=rowptr[1:])
    return rowptr, src[order]


def test_graph_metric_restatements_follow_the_fixtures_formulas():
    """g8_metrics (recorded from the reference's utils/metrics/graph_metrics.py) and its formulas in fp64.  TV: every term
    |x_j - x_i| >= 0 carries one rounding, the C - 1 channel adds one each, then inv (2), the product and the cast: (C + 4) u
    relative.  Laplace: deg adds and one product, each within u of a partial result bounded by sum |x_j| + deg |x_i|."""
    z = load_npz('g8_metrics')
    pred, ei = z['pred'].astype(np.float32), z['ei']
    N, C = pred.shape
    rowptr, col = _csr(ei, N)
    tv = O.total_variation(pred, rowptr, col)
    p64 = torch.from_numpy(pred).double()
    want = float(stin_oracle.graph_total_variation(p64, torch.from_numpy(ei)))
    assert tv.dtype == np.float32 and abs(float(tv) - want) <= (C + 4) * U * want
    assert abs(float(tv) - float(z['tv'])) <= 1e-6 * want                    # the recorded fp32 value (torch's own summation order)
    lap = O.graph_laplace(pred, rowptr, col)
    x64 = pred.astype(np.float64)
    deg = np.diff(rowptr).astype(np.float64)[:, None]
    s64, a64 = np.zeros((N, C)), np.zeros((N, C))
    np.add.at(s64, ei[1], x64[ei[0]])
    np.add.at(a64, ei[1], np.abs(x64[ei[0]]))
    assert np.all(np.abs(lap - (s64 - deg * x64)) <= (deg + 2) * U * (a64 + deg * np.abs(x64)))
    gray = (0.299 * p64[:, 0:1] + 0.587 * p64[:, 1:2] + 0.114 * p64[:, 2:3]).numpy().astype(np.float32)
    lv = np.var(O.graph_laplace(gray, rowptr, col).astype(np.float64), axis=0)
    assert abs(float(lv[0]) - float(z['lap_var'].reshape(-1)[0])) <= 1e-5 * float(lv[0])
    assert abs(float(lv[0]) - float(stin_oracle.graph_laplace_variance(p64, torch.from_numpy(ei))[0])) <= 1e-5 * float(lv[0])


def test_graph_metric_restatements_typed_out():
    x = np.array([[1.0, 2.0], [4.0, 8.0], [-1.0, 0.5]], np.float32)
    rowptr, col = np.array([0, 3, 3, 4]), np.array([1, 1, 0, 2])              # row 0: a repeated edge and a self loop; row 1 empty
    # TV: row 0: 2 x (3 + 6) + 0, row 2: self loop 0 -> 18 / 6
    assert O.total_variation(x, rowptr, col) == np.float32(3.0)
    assert O.graph_laplace(x, rowptr, col).tolist() == [[9.0 - 3.0, 18.0 - 6.0], [0.0, 0.0], [0.0, 0.0]]
