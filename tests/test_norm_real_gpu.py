"""What the exact layer (tests/test_norm_exact_gpu.py) cannot see: rounding.  Gaussian operands through every reduction mode on
both routes against torch fp64 within derived bounds, and the two inexact functions of the ELU - the device's expm1f and its fast
exponential - measured in ulp against fp64 through the forward and backward elementwise kernels.  The reference is always fp64,
never a second run of a kernel.

Bounds of the sums (u = 2^-24; n_b rows in range b; t the fp64-exact terms on the fp32 operands), extending those of
test_colreduce_two_stage_route_at_four_channels_per_lane_against_fp64 (tests/test_hip_parity.py):
  |got - want| <= u |want|                     one fp32 rounding of the result
               +  n_b 2^-52 sum |t|            fp64 accumulation in any order
               +  sum_r k_r u |t_r| 1.0001     the k_r fp32 roundings inside term r before it is widened:
    SUM, MOMENTS   k = 0 (the terms are formed in fp64);
    CSQ            k = 3: d = x - mean, then d * d squares d's rounding (2) and rounds (1);
    COEF_XC        k = 2: x - mean, the product;
    DOT_BN[_RELU]  t0 = d n: k = 3 (x - mean, * rstd, the product); t1 = d: k = 0.  RELU: a row whose fp64 z = gamma n + beta lies
                   within 4 u (|gamma n| + |beta|) of 0 may take the other branch: its whole |t| is added to the bound;
    DOT_ELU        n = xc rstd carries 2 roundings, an ABSOLUTE error 2 u |n| that exp turns into a relative one; the exponential
                   itself is EXPF_ULP ulp off (measured below; an ulp is at most 2 u relative); dy = gout e rounds once:
                   n <= 0: t1 = dy: k = 2 |n| + 2 EXPF_ULP + 1, t0 = dy xc: that + 2 (xc's rounding, the product);
                   n > 0:  e = 1 and dy = gout exactly: t1: k = 0, t0: k = 2; rows with |n| <= 4 u: the n <= 0 figure.
  MOMENTS mean: the SUM bound times inv_cnt; rstd: 2^-23 relative (see the test named above)."""
import numpy as np
import pytest
import torch

import _norm_oracle as O
import _norm_table as T
from surface_texture_inpainting_net_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24
F = np.float32
# Measured on the MI355X over 2^16 points of [-20, 0]: the largest distance, in ulp of the correctly rounded
# fp32 value, of the device's expm1f from fp64 expm1 (0.787) and of its fast exponential from fp64 exp (15.322, at n = -19.41: the
# exponential is exp2 of the ROUNDED product n log2(e), whose rounding is an absolute error of the exponent that grows with |n|) -
# rounded up to whole ulp.  The same figures at four channels per lane and at one.
EXPM1_ULP = 1.0
EXPF_ULP = 16.0


@pytest.fixture(autouse=True)
def _end_the_run_after_a_device_fault():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit('device fault, run ended: %s' % e, returncode=3)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def ulp_of(ref):
    """The spacing of fp32 at |ref| (normal range)"""
    return np.spacing(np.abs(ref).astype(F)).astype(np.float64)


def measure_elu(C, pad):
    """-> (largest ulp distance of expm1f, of the fast exponential) over 2^16 points of [-20, 0], through stin_norm_act_res_fwd_f32
    and stin_norm_act_bwd_f32 with mean = 0, rstd = 1, gout = 1, a = 1, k = m = 0: y = expm1f(x) and dx = exp(x), no other rounding"""
    lib = _lib.load()
    n = np.linspace(-20.0, 0.0, 2 ** 16).astype(F)
    N, ld = n.size // C, C + pad
    x = torch.zeros(N, ld, device=DEV)
    x[:, :C] = dev(n.reshape(N, C))
    zero, one = torch.zeros(1, C, device=DEV), torch.ones(1, C, device=DEV)
    g = torch.ones(N, ld, device=DEV)
    y, dx = torch.zeros(N, ld, device=DEV), torch.zeros(N, ld, device=DEV)
    assert lib.stin_norm_lane_class(C, 4, 16, 1, 4 if ld % 4 == 0 else 1) == (4 if pad == 0 else 1)
    assert lib.stin_norm_act_res_fwd_f32(ptr(x), ld, ptr(zero), ptr(one), None, None, 0, N, C, 1, ptr(y), ld, stream()) == 0
    assert lib.stin_norm_act_bwd_f32(ptr(x), ld, ptr(g), ld, ptr(zero), ptr(one), ptr(one), ptr(zero), ptr(zero), None, None, N, C, 1, ptr(dx),
                                     ld, stream()) == 0
    n64 = n.astype(np.float64)
    got_m1, got_e = y[:, :C].cpu().numpy().reshape(-1).astype(np.float64), dx[:, :C].cpu().numpy().reshape(-1).astype(np.float64)
    ref_m1, ref_e = np.expm1(n64), np.exp(n64)
    d_m1 = np.abs(got_m1 - ref_m1) / np.where(ref_m1 == 0, 1.0, ulp_of(ref_m1))
    d_e = np.abs(got_e - ref_e) / ulp_of(ref_e)
    return float(d_m1.max()), float(d_e.max()), float(n[d_e.argmax()])


@pytest.mark.parametrize('C,pad', [(256, 0), (16, 1)])
def test_elu_functions_within_the_measured_ulp_distance(C, pad):
    """Four channels per lane and one.  With these operands the kernels add no rounding to the two functions, so the bound is the
    measured distance itself (rounded up to whole ulp), and the reference is fp64."""
    m1, e, at = measure_elu(C, pad)
    print('expm1f: max %.3f ulp; fast exp: max %.3f ulp (at n = %.4f)' % (m1, e, at))
    assert m1 <= EXPM1_ULP
    assert e <= EXPF_ULP


# ------------------------------------------------------------------------------------------------ Gaussian sums
def gaussian(seed, N, C, B):
    rng = np.random.default_rng(seed)
    d = dict(x=(rng.standard_normal((N, C)) * 1.7 + 0.3).astype(F), gout=rng.standard_normal((N, C)).astype(F),
             mean=(rng.standard_normal((B, C)) * 0.3 + 0.3).astype(F), rstd=(0.4 + rng.random((B, C))).astype(F),
             coef=rng.standard_normal((B, C)).astype(F))
    d['gid'] = np.sort(rng.integers(0, B, N)).astype(np.int32)
    d['sid'] = rng.integers(0, B, N).astype(np.int32)
    return d


def terms_and_roundings(mode, d, B):
    """-> [(t, k, extra)]: the fp64-exact terms on the fp32 operands, the roundings per term and what a term may be off by
    outright (see the module docstring)"""
    x, g = d['x'].astype(np.float64), d['gout'].astype(np.float64)
    if mode in (O.RED_SUM, O.RED_MOMENTS):
        return [(x, 0.0, 0.0)] + ([(x * x, 0.0, 0.0)] if mode == O.RED_MOMENTS else [])
    if mode in (O.RED_DOT_BN, O.RED_DOT_BN_RELU):
        mean, rstd = d['mean'][0].astype(np.float64), d['rstd'][0].astype(np.float64)
        gamma, beta = d['coef'][0].astype(np.float64), d['coef'][1 % B].astype(np.float64)
        n = (x - mean) * rstd
        near = np.zeros(n.shape, bool)
        if mode == O.RED_DOT_BN_RELU:
            z = gamma * n + beta
            near = np.abs(z) <= 4 * U * (np.abs(gamma * n) + np.abs(beta))
            g = np.where(z > 0, g, 0.0)
        g_all = d['gout'].astype(np.float64)
        return [(g * n, 3.0, np.where(near, np.abs(g_all * n), 0.0)), (g, 0.0, np.where(near, np.abs(g_all), 0.0))]
    xc = x - d['mean'].astype(np.float64)[d['gid']]
    if mode == O.RED_CSQ:
        return [(xc * xc, 3.0, 0.0)]
    if mode == O.RED_COEF_XC:
        return [(d['coef'].astype(np.float64)[d['sid']] * xc, 2.0, 0.0)]
    n = xc * d['rstd'].astype(np.float64)[d['gid']]
    assert n.min() >= -20.0                                  # the range EXPF_ULP was measured on
    neg = n <= 4 * U
    dy = g * np.where(n > 0, 1.0, np.exp(np.minimum(n, 0.0)))
    k1 = np.where(neg, 2 * np.abs(n) + 2 * EXPF_ULP + 1, 0.0)
    return [(dy * xc, k1 + 2.0, 0.0), (dy, k1, 0.0)]


ROUTES = (('one-launch', 32, 0, T.ONE), ('two-stage', 30, 1, T.TWO))


@pytest.mark.parametrize('route', ROUTES, ids=lambda r: r[0])
@pytest.mark.parametrize('mode', range(7))
def test_gaussian_sums_against_fp64(mode, route):
    """N = 20 000 rows in three ragged ranges (BatchNorm modes: one), C = 32 on the one-launch route and C = 30 at ldx = 31 on the
    two-stage route at one channel per lane; ids that differ from the range index"""
    _, C, pad, family = route
    lib = _lib.load()
    bn = mode in (O.RED_DOT_BN, O.RED_DOT_BN_RELU)
    lens = [20000] if bn else [7001, 12, 12987]
    B, N = len(lens), 20000
    d = gaussian(10 * mode + C, N, C, 2 if bn else B)
    if bn:
        d['gid'] = d['sid'] = None
    cuts = np.concatenate([[0], np.cumsum(lens)])
    inv = (1.0 / np.asarray(lens, np.float64)).astype(F)
    nout = 2 if mode in O.TWO_OUTPUTS else 1
    cu = torch.cuda.get_device_properties(torch.device(DEV)).multi_processor_count
    rc, rt = T.route(lib, N, C, B, nout, int(pad == 0), 1, cu)
    assert rc == 0 and rt['family'] == family
    ld = C + pad
    x, g = torch.zeros(N, ld, device=DEV), torch.zeros(N, ld, device=DEV)
    x[:, :C], g[:, :C] = dev(d['x']), dev(d['gout'])
    t = {k: (None if d[k] is None else dev(d[k])) for k in ('mean', 'rstd', 'coef', 'gid', 'sid')}
    tp, tinv = (None if bn else dev(cuts.astype(np.int32))), dev(inv)
    out = torch.full((2, B, C), float('nan'), device=DEV)
    nb = lib.stin_colreduce_workspace_bytes(C, B)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    eps = 1e-5
    assert lib.stin_colreduce_f32(mode, ptr(x), ld, ptr(g), ld, N, C, ptr(tp), B, ptr(t['gid']), ptr(t['sid']), ptr(t['mean']), ptr(t['rstd']),
                                  ptr(t['coef']), 0, ptr(tinv), eps, ptr(out[0]), ptr(out[1]), ptr(ws), nb, stream()) == 0
    got = out.cpu().numpy().astype(np.float64)
    seg = lambda a: np.stack([a[lo:hi].sum(0) for lo, hi in zip(cuts, cuts[1:])])
    worst = 0.0
    sums = []
    for o, (tm, k, extra) in enumerate(terms_and_roundings(mode, d, 2 if bn else B)):
        want, mag = seg(tm), seg(np.abs(tm))
        bound = U * np.abs(want) + np.asarray(lens, np.float64)[:, None] * 2.0 ** -52 * mag + 1.0001 * U * seg(k * np.abs(tm)) + seg(extra + 0.0 * tm)
        sums.append((want, bound))
        if mode != O.RED_MOMENTS:
            err = np.abs(got[o] - want)
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (o, float((err / np.maximum(bound, 1e-300)).max()))
    if mode == O.RED_MOMENTS:
        ic = inv.astype(np.float64)[:, None]
        mean = sums[0][0] * ic
        var = np.maximum(sums[1][0] * ic - mean * mean, 0.0)
        rstd = 1.0 / np.sqrt(var + float(F(eps)))
        err_m, rel_r = np.abs(got[0] - mean), np.abs((got[1] - rstd) / rstd)
        worst = float((err_m / (sums[0][1] * ic)).max())
        print('MOMENTS: rstd max rel err = %.3e, max mean^2 / var = %.3g' % (float(rel_r.max()), float((mean * mean / var).max())))
        assert (err_m <= sums[0][1] * ic).all()
        assert float(rel_r.max()) <= 2.0 ** -23
    print('mode %d %s: max |err| / bound = %.3f' % (mode, route[0], worst))
