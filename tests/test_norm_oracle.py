"""tests/_norm_oracle.py, the numpy restatement the norm kernels are held to (tests/test_norm_exact_gpu.py), held to first
principles on the CPU - never against the kernels: FastInstanceNorm of oracle/stin_oracle.py in fp64 with and without its
linspace-slice quirk, forward and autograd backward; torch's batch_norm, forward, backward and running statistics; and small cases
typed out by hand (an empty range, a range of one row, sid != gid, the variance clamp).

Bounds.  u = 2^-24 is the unit roundoff of fp32.  The restatement forms every sum in fp64 and rounds each documented fp32
operation once, so against an fp64 evaluation of the same formula a result that went through k fp32 roundings of quantities of
magnitude at most M is within k u M (first order).  Each test names its k and its M; the sums themselves add one rounding of the
sum (u |sum|) plus the roundings of their terms (u sum|terms| per fp32 operation inside a term)."""
import numpy as np
import pytest
import torch

import _norm_oracle as O
import _param_oracle as P
from oracle import stin_oracle

U = 2.0 ** -24
F = np.float32


def data(seed, N, C):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((N, C)) * 1.7 + 0.3).astype(F), rng.standard_normal((N, C)).astype(F), rng.standard_normal((N, C)).astype(F))


def reference(x, w, res, batch, eps):
    """y = res + ELU(FastInstanceNorm(x)) and d(sum w y)/dx in fp64 through autograd"""
    xt = torch.from_numpy(x).double().requires_grad_(True)
    n = stin_oracle.fast_instance_norm(xt, None if batch is None else torch.from_numpy(batch), eps)
    y = torch.nn.functional.elu(n) + torch.from_numpy(res).double()
    (y * torch.from_numpy(w).double()).sum().backward()
    return n.detach().numpy(), y.detach().numpy(), xt.grad.numpy()


@pytest.mark.parametrize('N,C', [(2, 3), (300, 5), (4097, 2)])
def test_single_graph_instance_norm_forward_and_backward(N, C):
    """batch = None: MOMENTS, the forward pass, DOT_ELU with POST_NORM_COEF, the backward pass with a = rstd.
    Forward: mean and rstd are fp32 roundings of fp64-accurate values (u each); n = (x - mean) rstd is 2 more roundings of a
    quantity of size (|x| + |mean|) rstd; ELU and the residual add one each: 6 u ((|x| + |mean|) rstd + |res|), taken as 8.
    Backward: dx = rstd dy + k xc + m.  k and m carry 5 and 3 roundings plus those of their sums' terms (4 per term of dy xc,
    relative to sum |dy xc| / n); dy 3; the three products and two additions 5 more, each relative to the sum of the magnitudes
    of the three addends A: 24 u A bounds all of them - but for one thing: an ABSOLUTE error of n, 3 u Mn with Mn = (|x| + |mean|)
    rstd, is a RELATIVE error of exp(n) and so of dy.  With the largest Mn of the case: (24 + 3 max Mn) u A."""
    x, w, res = data(N + C, N, C)
    eps = 1e-5
    n64, y64, dx64 = reference(x, w, res, None, eps)
    inv = [1.0 / N]
    mean, rstd = O.colreduce(O.RED_MOMENTS, x, inv_cnt=inv, eps=eps)
    y = O.norm_act_res_fwd(x, mean, rstd, None, res, 1)
    M = (np.abs(x) + np.abs(mean)) * rstd + np.abs(res)
    assert (np.abs(y - y64) <= 8 * U * M).all(), float((np.abs(y - y64) / M).max() / U)
    k, m = O.colreduce(O.RED_DOT_ELU, x, w, mean=mean, rstd=rstd, kind=O.POST_NORM_COEF, inv_cnt=inv)
    dx = O.norm_act_bwd(x, w, mean, rstd, rstd, k, m)
    xc = np.abs(x.astype(np.float64) - mean)
    dy = np.abs(w.astype(np.float64)) * np.where(n64 > 0, 1.0, np.exp(np.minimum(n64, 0)))
    A = rstd * dy + rstd.astype(np.float64) ** 3 * (dy * xc).sum(0) / N * xc + rstd * dy.sum(0) / N
    c = 24 + 3 * float(((np.abs(x) + np.abs(mean)) * rstd).max())
    assert (np.abs(dx - dx64) <= c * U * A).all(), float((np.abs(dx - dx64) / A).max() / U)


def groups_of(counts):
    """batch (sorted graph ids), the linspace slices the reference sums over, the true graph boundaries, and the slice of every row"""
    batch = np.repeat(np.arange(len(counts)), counts).astype(np.int64)
    N = len(batch)
    ptr_sum = torch.linspace(0, N, len(counts) + 1, dtype=torch.int).numpy()
    ptr_true = np.concatenate([[0], np.cumsum(counts)])
    sid = (np.searchsorted(ptr_sum[1:], np.arange(N), side='right')).astype(np.int32)
    return batch, ptr_sum, ptr_true, np.minimum(sid, len(counts) - 1)


@pytest.mark.parametrize('counts', [(8, 8, 8), (5, 11, 8), (40, 3, 100, 57)])
def test_batched_instance_norm_with_the_linspace_slice_quirk(counts):
    """batch given: sums over linspace slices, divisors the true counts, centring through the graph id - equal slices (no quirk:
    sid == gid) and unequal ones.  Forward: SUM with POST_SCALE, CSQ with POST_RSTD, the forward pass; backward: DOT_ELU over the
    true ranges, stin_norm_bwd_coef, COEF_XC through sid, the m of the quirk, the backward pass through gid and sid.
    The two-pass variance rounds every (x - mean)^2 in fp32 (3 u per term) and the post 4 more: rstd within 6 u, n within
    10 u (|x| + |mean|) rstd, taken as 12 with ELU and residual.  Backward as in the single-graph test with U = sum k xc of the quirk
    as a fourth addend of m, and the absolute error 10 u Mn of n as a relative error of dy: (32 + 10 max Mn) u A."""
    C = 4
    batch, ptr_sum, ptr_true, sid = groups_of(counts)
    N, B = len(batch), len(counts)
    x, w, res = data(N, N, C)
    eps = 1e-5
    n64, y64, dx64 = reference(x, w, res, batch, eps)
    inv = (1.0 / np.asarray(counts, np.float64)).astype(F)
    gid = batch.astype(np.int32)
    mean, _ = O.colreduce(O.RED_SUM, x, ptr=ptr_sum, B=B, kind=O.POST_SCALE, inv_cnt=inv)
    rstd, _ = O.colreduce(O.RED_CSQ, x, ptr=ptr_sum, B=B, gid=gid, mean=mean, kind=O.POST_RSTD, inv_cnt=inv, eps=eps)
    y = O.norm_act_res_fwd(x, mean, rstd, gid, res, 1)
    M = (np.abs(x) + np.abs(mean[gid])) * rstd[gid] + np.abs(res)
    assert (np.abs(y - y64) <= 12 * U * M).all(), float((np.abs(y - y64) / M).max() / U)
    T1, S0 = O.colreduce(O.RED_DOT_ELU, x, w, ptr=ptr_true, B=B, gid=gid, mean=mean, rstd=rstd)
    k, m0 = P.norm_bwd_coef(T1, S0, rstd, inv)
    if tuple(ptr_sum) == tuple(ptr_true):
        m = m0
    else:
        Uq, _ = O.colreduce(O.RED_COEF_XC, x, ptr=ptr_true, B=B, gid=gid, sid=sid, mean=mean, coef=k)
        m = P.norm_bwd_coef_m_quirk(S0, Uq, rstd, inv)
    dx = O.norm_act_bwd(x, w, mean, rstd, rstd, k, m, gid, sid)
    xc = np.abs(x.astype(np.float64) - mean[gid])
    dy = np.abs(w.astype(np.float64)) * np.where(n64 > 0, 1.0, np.exp(np.minimum(n64, 0)))
    r64 = rstd.astype(np.float64)
    seg = lambda t: np.stack([t[a:b].sum(0) for a, b in zip(ptr_true, ptr_true[1:])])
    kabs = r64 ** 3 * seg(dy * xc) * inv[:, None]
    mabs = (r64 * seg(dy) + seg(kabs[sid] * xc)) * inv[:, None]
    A = r64[gid] * dy + kabs[sid] * xc + mabs[sid]
    c = 32 + 10 * float(((np.abs(x) + np.abs(mean[gid])) * rstd[gid]).max())
    assert (np.abs(dx - dx64) <= c * U * A).all(), float((np.abs(dx - dx64) / A).max() / U)


@pytest.mark.parametrize('act', [0, 1])
def test_batchnorm_against_torch(act):
    """MOMENTS, stin_bn_act_fwd, DOT_BN[_RELU], stin_bn_act_bwd and the running statistics against torch.nn.functional.batch_norm
    (+ relu) in fp64.  Forward: 5 roundings of (|gamma| (|x| + |mean|) rstd + |beta|): 6 u.  Backward: dx = rstd gamma (d - Q / n
    - nhat P / n), 3 roundings in nhat, 4 in the sums' terms, 7 in the expression, relative to the sum of magnitudes A: 16 u A.
    Running statistics: var = 1 / rstd^2 - eps recovers the biased variance within 4 u (var + eps); 8 u (|running| + |new|)."""
    N, C, eps, mom = 301, 6, 1e-5, 0.1
    x, w, _ = data(7, N, C)
    rng = np.random.default_rng(1)
    gamma, beta = rng.standard_normal(C).astype(F), rng.standard_normal(C).astype(F)
    rm0, rv0 = rng.standard_normal(C).astype(F), rng.random(C).astype(F) + 0.5
    xt = torch.from_numpy(x).double().requires_grad_(True)
    rm, rv = torch.from_numpy(rm0).double(), torch.from_numpy(rv0).double()
    z = torch.nn.functional.batch_norm(xt, rm, rv, torch.from_numpy(gamma).double(), torch.from_numpy(beta).double(), True, mom, eps)
    yt = torch.relu(z) if act else z
    (yt * torch.from_numpy(w).double()).sum().backward()
    mean, rstd = O.colreduce(O.RED_MOMENTS, x, inv_cnt=[1.0 / N], eps=eps)
    mean, rstd = mean[0], rstd[0]
    y = O.bn_act_fwd(x, mean, rstd, gamma, beta, act)
    M = np.abs(gamma) * (np.abs(x) + np.abs(mean)) * rstd + np.abs(beta)
    assert (np.abs(y - yt.detach().numpy()) <= 6 * U * M).all()
    Pq, Qq = O.colreduce(O.RED_DOT_BN_RELU if act else O.RED_DOT_BN, x, w, mean=mean, rstd=rstd, coef=np.stack([gamma, beta]))
    dx = O.bn_act_bwd(x, w, mean, rstd, gamma, beta, Pq[0], Qq[0], 1.0 / N, act)
    nh = np.abs((x.astype(np.float64) - mean) * rstd)
    d = np.abs(w.astype(np.float64)) * ((z.detach().numpy() > 0) if act else 1.0)
    A = rstd * np.abs(gamma) * (d + d.sum(0) / N + nh * (d * nh).sum(0) / N)
    assert (np.abs(dx - xt.grad.numpy()) <= 16 * U * A).all(), float((np.abs(dx - xt.grad.numpy()) / A).max() / U)
    nm, nv = O.bn_running_stats(mean, rstd, eps, N / (N - 1.0), mom, rm0, rv0)
    assert (np.abs(nm - rm.numpy()) <= 8 * U * (np.abs(rm0) + np.abs(mean))).all()
    var = x.astype(np.float64).var(0, ddof=1)
    assert (np.abs(nv - rv.numpy()) <= 8 * U * (np.abs(rv0) + var + eps)).all()


def test_typed_out_reductions():
    """An empty range, a range of one row, ids that differ from the range index (sid != gid): every number below worked out by hand"""
    x = np.array([[1, 2], [3, 4], [5, 6], [7, 8]], F)
    ptr = [0, 0, 1, 4]
    s, none = O.colreduce(O.RED_SUM, x, ptr=ptr, B=3)
    assert none is None and s.dtype == F and np.array_equal(s, [[0, 0], [1, 2], [15, 18]])
    s, _ = O.colreduce(O.RED_SUM, x, ptr=ptr, B=3, kind=O.POST_SCALE, inv_cnt=[1, 1, 0.25])
    assert np.array_equal(s, [[0, 0], [1, 2], [3.75, 4.5]])
    mean, gid, sid = np.array([[1, 1], [2, 0]], F), [0, 1, 1, 0], [1, 0, 0, 1]
    # xc = [[0, 1], [1, 4], [3, 6], [6, 7]]
    s, _ = O.colreduce(O.RED_CSQ, x, ptr=ptr, B=3, gid=gid, mean=mean)
    assert np.array_equal(s, [[0, 0], [0, 1], [1 + 9 + 36, 16 + 36 + 49]])
    s, _ = O.colreduce(O.RED_CSQ, x, ptr=ptr, B=3, gid=gid, mean=mean, kind=O.POST_RSTD, inv_cnt=[1, 12, 0.5], eps=4.0)      # 0 + 4, 12 + 4; 23 + 4, 50.5 + 4
    assert np.array_equal(s, [[0.5, 0.5], [0.5, 0.25], [F(1) / np.sqrt(F(27)), F(1) / np.sqrt(F(54.5))]])
    coef = np.array([[2, 0.5], [-1, 1]], F)
    s, _ = O.colreduce(O.RED_COEF_XC, x, ptr=ptr, B=3, gid=gid, sid=sid, mean=mean, coef=coef)
    assert np.array_equal(s, [[0, 0], [0, 1], [2 + 6 - 6, 2 + 3 + 7]])
    s, _ = O.colreduce(O.RED_COEF_XC, x, ptr=ptr, B=3, gid=gid, sid=None, mean=mean, coef=coef)            # sid NULL: coef[0]
    assert np.array_equal(s, [[0, 0], [0, 0.5], [2 + 6 + 12, 2 + 3 + 3.5]])
    s, _ = O.colreduce(O.RED_CSQ, x, gid=None, mean=mean)                                                  # gid NULL: mean[0], one range
    assert np.array_equal(s, [[0 + 4 + 16 + 36, 1 + 9 + 25 + 49]])


def test_typed_out_moments_and_the_variance_clamp():
    m, r = O.colreduce(O.RED_MOMENTS, np.array([[3, 4]], F), inv_cnt=[1.0], eps=0.25)                      # one row: var = 0
    assert np.array_equal(m, [[3, 4]]) and np.array_equal(r, [[2, 2]])
    m, r = O.colreduce(O.RED_MOMENTS, np.array([[1], [3]], F), inv_cnt=[0.5], eps=0.0)                      # var = 5 - 4
    assert np.array_equal(m, [[2]]) and np.array_equal(r, [[1]])
    # a divisor that is not the row count (the linspace quirk can produce one): E[x^2] - mean^2 = 2 - 4 < 0 is raised to 0
    m, r = O.colreduce(O.RED_MOMENTS, np.array([[1], [1]], F), inv_cnt=[1.0], eps=0.25)
    assert np.array_equal(m, [[2]]) and np.array_equal(r, [[2]])
    m, r = O.colreduce(O.RED_MOMENTS, np.zeros((0, 2), F), inv_cnt=[1.0], eps=0.25)                        # no rows
    assert np.array_equal(m, [[0, 0]]) and np.array_equal(r, [[2, 2]])
    part = np.array([[[1], [5]], [[2], [6]], [[3], [9]]], np.float64)                                           # [3 groups][2][1]: sums 6, 20
    m, r = O.moments_final(part, [0.5], 0.0)                                                              # mu = 3, var = 10 - 9
    assert np.array_equal(m, [[3]]) and np.array_equal(r, [[1]])
    k, mm = O.norm_coef_from_partials(part, np.array([[2]], F), [0.5])
    assert np.array_equal(k, [[-8 * 6 * 0.5]]) and np.array_equal(mm, [[-2 * 20 * 0.5]])


def test_typed_out_elu_sums_and_passes():
    """rstd = 128 and xc = 1, 0, -1: ELU' = 1, 1, 0 and ELU = 128, 0, -1 after rounding"""
    x, g = np.array([[2], [1], [0]], F), np.array([[2], [3], [5]], F)
    mean, rstd = np.array([[1]], F), np.array([[128]], F)
    assert np.array_equal(O.elu_grad(F(-128) * np.ones(1, F)), [0]) and np.array_equal(O.elu(F(-128) * np.ones(1, F)), [-1])
    t1, s0 = O.colreduce(O.RED_DOT_ELU, x, g, mean=mean, rstd=rstd)
    assert np.array_equal(t1, [[2]]) and np.array_equal(s0, [[5]])
    k, m = O.colreduce(O.RED_DOT_ELU, x, g, mean=mean, rstd=rstd, kind=O.POST_NORM_COEF, inv_cnt=[0.5])
    assert np.array_equal(k, [[-(128.0 ** 3) * 2 * 0.5]]) and np.array_equal(m, [[-128.0 * 5 * 0.5]])
    y = O.norm_act_res_fwd(x, mean, rstd, None, np.array([[1], [1], [1]], F), 1)
    assert np.array_equal(y, [[129], [1], [0]])
    assert np.array_equal(O.norm_act_res_fwd(x, mean, rstd, None, None, 0), [[128], [0], [-128]])
    y = O.norm_act_res_fwd(x, mean, rstd, None, np.array([[10], [20]], F), 1, row_map=[1, 1, 0])
    assert np.array_equal(y, [[148], [20], [9]])
    dx = O.norm_act_bwd(x, g, mean, rstd, np.array([[0.5]], F), np.array([[2]], F), np.array([[-1]], F))
    assert np.array_equal(dx, [[0.5 * 2 + 2 * 1 - 1], [0.5 * 3 + 0 - 1], [0 - 2 - 1]])
    dx = O.norm_act_bwd(x, g, mean, rstd, np.array([[0.5]], F), np.array([[2], [4]], F), np.array([[-1], [1]], F), None, [0, 1, 1], 0)
    assert np.array_equal(dx, [[1 + 2 - 1], [1.5 + 0 + 1], [2.5 - 4 + 1]])


def test_typed_out_batchnorm_and_bf16_rounding():
    x, g = np.array([[4], [6], [2]], F), np.array([[1], [2], [3]], F)
    mean, rstd, gamma, beta = [2.0], [0.5], [0.5], [-0.5]                                                  # n = 1, 2, 0;  z = 0, 0.5, -0.5
    assert np.array_equal(O.bn_act_fwd(x, mean, rstd, gamma, beta, 0), [[0], [0.5], [-0.5]])
    assert np.array_equal(O.bn_act_fwd(x, mean, rstd, gamma, beta, 1), [[0], [0.5], [0]])
    p, q = O.colreduce(O.RED_DOT_BN, x, g, mean=mean, rstd=rstd, coef=[gamma, beta])
    assert np.array_equal(p, [[1 + 4 + 0]]) and np.array_equal(q, [[6]])
    p, q = O.colreduce(O.RED_DOT_BN_RELU, x, g, mean=mean, rstd=rstd, coef=[gamma, beta])                  # only the row with z > 0
    assert np.array_equal(p, [[4]]) and np.array_equal(q, [[2]])
    dx = O.bn_act_bwd(x, g, mean, rstd, gamma, beta, [4.0], [2.0], 0.5, 1)                                  # d = 0, 2, 0
    assert np.array_equal(dx, 0.25 * np.array([[0 - 1 - 1 * 2], [2 - 1 - 2 * 2], [0 - 1 - 0]], F))
    rm, rv = O.bn_running_stats([1.0, 1.0], [2.0, 128.0], 0.125, 2.0, 0.5, [3.0, 3.0], [1.0, 1.0])          # var = 1/4 - 1/8; < 0 -> 0
    assert np.array_equal(rm, [2, 2]) and np.array_equal(rv, [0.5 + 0.5 * 0.25, 0.5])
    bits = O.round_bf16(np.array([2051, 2056, 2044, 1.0, -3.5, 257, 259], F))                              # ties to even: 2056 -> 2048, 2044 -> 2048
    assert np.array_equal(O.bf16_to_f32(bits), [2048, 2048, 2048, 1, -3.5, 256, 260])
