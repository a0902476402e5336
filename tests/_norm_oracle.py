"""The norm statistics and epilogues of include/stin_hip.h ("norm statistics and epilogues", the BatchNorm passes, the fold
forms) restated in numpy: one np.float32 or np.float64 operation per operation the header documents, in the header's order.  It
does not import the package.  tests/test_norm_oracle.py holds it to first principles on the CPU; tests/test_norm_exact_gpu.py
holds the kernels to it, bit for bit, on operands whose every sum is exact.

Sums are numpy fp64 sums in numpy's order: equal to any other order exactly where every partial sum is exact (integers, small
dyadic numbers) - the cases the exact tests use.  `exp` and `expm1` are the correctly rounded fp32 values of the fp64 functions;
the device's are not, so the exact tests keep their arguments where both agree (0, or far enough below 0 that the result rounds
to 0 / -1) and tests/test_norm_exact_gpu.py measures the distance elsewhere."""
import numpy as np

F = np.float32
D = np.float64

RED_SUM, RED_CSQ, RED_DOT_ELU, RED_COEF_XC, RED_MOMENTS, RED_DOT_BN, RED_DOT_BN_RELU = range(7)
POST_NONE, POST_SCALE, POST_RSTD, POST_NORM_COEF = range(4)
TWO_OUTPUTS = (RED_DOT_ELU, RED_MOMENTS, RED_DOT_BN, RED_DOT_BN_RELU)


def f32(a):
    return np.asarray(a, dtype=F)


def elu_grad(n):
    """e = n > 0 ? 1 : exp(n)"""
    n = f32(n)
    with np.errstate(under='ignore'):
        return np.where(n > 0, F(1), np.exp(np.minimum(n, F(0)).astype(D)).astype(F))


def elu(n):
    """n > 0 ? n : expm1(n)"""
    n = f32(n)
    return np.where(n > 0, n, np.expm1(np.minimum(n, F(0)).astype(D)).astype(F))


def _rows(v, idx, n):
    """v[idx] with idx == None meaning group 0 for every row"""
    v = f32(v)
    if v.ndim == 1:
        v = v[None]
    return v[np.zeros(n, np.int64) if idx is None else np.asarray(idx, np.int64)]


def terms(mode, x, gout=None, gid=None, sid=None, mean=None, rstd=None, coef=None):
    """The fp64 terms t0 (, t1) [N, C] a reduction adds, per element."""
    x = f32(x)
    n_rows = x.shape[0]
    if mode == RED_SUM:
        return (x.astype(D),)
    if mode == RED_MOMENTS:
        d = x.astype(D)
        return d, d * d
    if mode in (RED_DOT_BN, RED_DOT_BN_RELU):
        gamma, beta = f32(coef).reshape(2, -1)
        n = (x - f32(mean).reshape(1, -1)) * f32(rstd).reshape(1, -1)
        d = f32(gout)
        if mode == RED_DOT_BN_RELU:
            d = np.where(gamma[None] * n + beta[None] > 0, d, F(0))
        return (d * n).astype(D), d.astype(D)
    xc = x - _rows(mean, gid, n_rows)
    if mode == RED_CSQ:
        return ((xc * xc).astype(D),)
    if mode == RED_COEF_XC:
        return ((_rows(coef, sid, n_rows) * xc).astype(D),)
    assert mode == RED_DOT_ELU
    dy = f32(gout) * elu_grad(xc * _rows(rstd, gid, n_rows))
    return (dy * xc).astype(D), dy.astype(D)


def range_sums(t, ptr, B):
    """fp64 sums [B, C] of the rows ptr[b] .. ptr[b + 1] (ptr None: one range); the accumulators start at +0"""
    cuts = [0, t.shape[0]] if ptr is None else [int(v) for v in ptr]
    assert len(cuts) == B + 1
    return np.stack([t[a:b].sum(axis=0, dtype=D) + 0.0 for a, b in zip(cuts, cuts[1:])])


def moments_post(s0, s1, inv_cnt, eps):
    """fp64 sums [B, C] -> mean, rstd fp32"""
    ic = f32(inv_cnt).astype(D).reshape(-1, 1)
    mu = s0 * ic
    var = s1 * ic - mu * mu
    var = np.where(var < 0.0, 0.0, var)
    return mu.astype(F), (1.0 / np.sqrt(var + D(F(eps)))).astype(F)


def post(kind, o, s, inv_cnt=None, eps=0.0, rstd=None):
    """Output o of the fp64 sums s [B, C] through post-operation `kind`"""
    r = s.astype(F)
    if kind == POST_NONE:
        return r
    ic = f32(inv_cnt).reshape(-1, 1)
    if kind == POST_SCALE:
        return r * ic
    if kind == POST_RSTD:
        return F(1) / np.sqrt(r * ic + F(eps))
    assert kind == POST_NORM_COEF
    rs = f32(rstd).reshape(r.shape)
    if o == 0:
        return ((-((rs * rs) * rs)) * r) * ic
    return (-(rs * r)) * ic


def colreduce(mode, x, gout=None, ptr=None, B=1, gid=None, sid=None, mean=None, rstd=None, coef=None, kind=POST_NONE,
              inv_cnt=None, eps=0.0):
    """stin_colreduce_*: -> (out0, out1 or None), fp32 [B, C]"""
    sums = [range_sums(t, ptr, B) for t in terms(mode, x, gout, gid, sid, mean, rstd, coef)]
    if mode == RED_MOMENTS:
        return moments_post(sums[0], sums[1], inv_cnt, eps)
    outs = [post(kind, o, s, inv_cnt, eps, rstd) for o, s in enumerate(sums)]
    return outs[0], (outs[1] if len(outs) == 2 else None)


def fold(partial):
    """partial [groups][2][C] fp64 -> the two sums [1, C]"""
    p = np.asarray(partial, D)
    return p[:, 0].sum(axis=0)[None] + 0.0, p[:, 1].sum(axis=0)[None] + 0.0


def moments_final(partial, inv_cnt, eps):
    """stin_moments_final_f32 -> mean, rstd [1, C]"""
    s0, s1 = fold(partial)
    return moments_post(s0, s1, inv_cnt, eps)


def norm_coef_from_partials(partial, rstd, inv_cnt):
    """stin_norm_coef_from_partials_f32 -> k, m [1, C]"""
    s0, s1 = fold(partial)
    return post(POST_NORM_COEF, 0, s0, inv_cnt, 0.0, rstd), post(POST_NORM_COEF, 1, s1, inv_cnt, 0.0, rstd)


def round_bf16(a):
    """fp32 -> the nearest bf16 (ties to even) as uint16 bits; finite inputs"""
    u = f32(a).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def bf16_to_f32(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(F)


def norm_act_res_fwd(x, mean, rstd, gid=None, res=None, act=1, row_map=None):
    """stin_norm_act_res_fwd_* (row_map: the _map form) -> y fp32 [N, C] (bf16 rows: round_bf16 of it)"""
    x = f32(x)
    n = (x - _rows(mean, gid, x.shape[0])) * _rows(rstd, gid, x.shape[0])
    if act:
        n = elu(n)
    if res is not None:
        r = f32(res)
        n = n + (r if row_map is None else r[np.asarray(row_map, np.int64)])
    return n


def norm_act_bwd(x, gout, mean, rstd, a, k, m, gid=None, sid=None, act=1):
    """stin_norm_act_bwd_* -> dx fp32 [N, C]"""
    x = f32(x)
    n_rows = x.shape[0]
    xc = x - _rows(mean, gid, n_rows)
    dy = f32(gout)
    if act:
        dy = dy * elu_grad(xc * _rows(rstd, gid, n_rows))
    return (_rows(a, gid, n_rows) * dy + _rows(k, sid, n_rows) * xc) + _rows(m, sid, n_rows)


def norm_fwd_fold(partial, x, res, inv_cnt, eps, row_map=None):
    """stin_norm_act_res_fwd_fold_f32 / _fold_map_f32 -> mean, rstd [1, C], y"""
    mean, rstd = moments_final(partial, inv_cnt, eps)
    return mean, rstd, norm_act_res_fwd(x, mean, rstd, None, res, 1, row_map)


def norm_bwd_fold(partial, x, gout, mean, rstd, inv_cnt):
    """stin_norm_act_bwd_fold_f32 -> dx (a = rstd)"""
    k, m = norm_coef_from_partials(partial, rstd, inv_cnt)
    return norm_act_bwd(x, gout, mean, rstd, rstd, k, m)


def bn_act_fwd(x, mean, rstd, gamma, beta, act):
    n = (f32(x) - f32(mean)[None]) * f32(rstd)[None]
    z = f32(gamma)[None] * n + f32(beta)[None]
    return np.where(z > 0, z, F(0)) if act else z


def bn_act_bwd(x, gout, mean, rstd, gamma, beta, P, Q, inv_n, act):
    rs, ga, inv_n = f32(rstd)[None], f32(gamma)[None], F(inv_n)
    n = (f32(x) - f32(mean)[None]) * rs
    d = f32(gout)
    if act:
        d = np.where(ga * n + f32(beta)[None] > 0, d, F(0))
    return (rs * ga) * ((d - f32(Q)[None] * inv_n) - n * (f32(P)[None] * inv_n))


def bn_running_stats(mean, rstd, eps, unbias, momentum, running_mean, running_var):
    r, mo = f32(rstd), F(momentum)
    with np.errstate(over='ignore', divide='ignore'):
        var = np.maximum(F(1) / (r * r) - F(eps), F(0))
    return ((F(1) - mo) * f32(running_mean) + mo * f32(mean), (F(1) - mo) * f32(running_var) + mo * (var * F(unbias)))
