"""numpy restatement of the parameter-side and train-step contracts of include/stin_hip.h: the weight operand layouts the GEMMs
decode (plain fp32, plain bf16 rows, the k-group pre-split form, the MFMA fragment order), the EdgeConv pack / unpack, the small
elementwise passes of the SingleConvMeshNet layer and of the SAGE message, the instance-norm backward coefficients, Adam, and the
loss / graph metrics in the summation order the header documents.  Written from the header; nothing here imports the package.

Every float operation is one IEEE single operation on np.float32 arrays (the library is built without contraction, with IEEE
division and square root), so a result is defined to the bit and the device is compared with `==` on integer views
(tests/test_param_exact_gpu.py).  tests/test_param_oracle.py checks this file from first principles on the CPU."""
import math

import numpy as np

# the #defines of include/stin_hip.h (tests/test_param_oracle.py checks them against the header text)
GEMM_BF16X3, GEMM_F16X3, GEMM_W_BF16, GEMM_W_FRAG, TI_COMPACT = 2, 4, 0x200, 0x400, 2
F32 = np.float32


# ------------------------------------------------------------------ number formats
def bf16_bits(v):
    """float32 -> the uint16 bit pattern of bf16(v), round to nearest even (finite values)."""
    b = np.ascontiguousarray(v, dtype=F32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


def split16(v, prec):
    """-> (hi, lo) uint16 bit patterns of the two 16-bit pieces of a pre-split weight.
    BF16X3: hi = bf16(v), lo = bf16(v - f32(hi)).  F16X3: s = v * 64 (exact), hi = f16(s), lo = f16(s - f32(hi))."""
    v = np.ascontiguousarray(v, dtype=F32)
    if prec == GEMM_F16X3:
        s = v * F32(64.0)
        hi = s.astype(np.float16)
        lo = (s - hi.astype(F32)).astype(np.float16)
        return hi.view(np.uint16), lo.view(np.uint16)
    assert prec == GEMM_BF16X3
    hi = bf16_bits(v)
    lo = bf16_bits(v - bf16_value(hi))
    return hi, lo


def join16(hi, lo, prec):
    """fp64 value the two pieces stand for: f32(hi) + f32(lo), divided by 64 for fp16 pieces."""
    if prec == GEMM_F16X3:
        return (hi.view(np.float16).astype(np.float64) + lo.view(np.float16).astype(np.float64)) / 64.0
    return bf16_value(hi).astype(np.float64) + bf16_value(lo).astype(np.float64)


# ------------------------------------------------------------------ operand layouts
def frag_shape(nc, kk):
    """STIN_GEMM_W_FRAG: the shapes stored in fragment order - K % 64 == 0 and (Nc % 32 == 0, 128 <= K <= 256, Nc >= 320; or
    Nc = 256 with K >= 512; or Nc = 128 with K >= 256)."""
    if kk % 64 != 0:
        return False
    return (nc % 32 == 0 and 128 <= kk <= 256 and nc >= 320) or (nc == 256 and kk >= 512) or (nc == 128 and kk >= 256)


def kgroup_index(nc, kk, ld=None):
    """Half (uint16) index of the hi piece of element (r, c) in the k-group form: the 16 bytes of the fp32 values 4g .. 4g + 3 of
    a row hold [hi x 4 | lo x 4]; the lo piece lies 4 halves further.  ld = row pitch in fp32 elements."""
    ld = kk if ld is None else ld
    r, c = np.meshgrid(np.arange(nc, dtype=np.int64), np.arange(kk, dtype=np.int64), indexing='ij')
    return (r * ld + (c & ~3)) * 2 + (c & 3)


def frag_index(nc, kk):
    """Half index of the hi piece of element (r, c) in fragment order: tile t = r >> 5, step s = c >> 4, lane = ((c >> 3) & 1)
    * 32 + (r & 31), 32 bytes = 16 halves per lane at lane slot (t * kk / 16 + s) * 64 + lane, hi at c & 7; lo 8 halves further."""
    r, c = np.meshgrid(np.arange(nc, dtype=np.int64), np.arange(kk, dtype=np.int64), indexing='ij')
    slot = ((r >> 5) * (kk >> 4) + (c >> 4)) * 64 + ((c >> 3) & 1) * 32 + (r & 31)
    return slot * 16 + (c & 7)


def split_layout(nc, kk, mode, ld=None):
    """-> (hi index, lo index, halves in the buffer) of a pre-split [nc, kk] operand written with `mode` (precision, optionally
    | GEMM_W_FRAG: fragment order where frag_shape holds - ld is then ignored -, the k-group form otherwise)."""
    if (mode & GEMM_W_FRAG) and frag_shape(nc, kk):
        hi = frag_index(nc, kk)
        return hi, hi + 8, 2 * nc * kk
    ld = kk if ld is None else ld
    hi = kgroup_index(nc, kk, ld)
    return hi, hi + 4, 2 * ((nc - 1) * ld + kk)


def encode(M, mode, ld=None, fill=0):
    """The halves (uint16) a weight operand M [nc, kk] occupies in its buffer for storage `mode`: 0 = fp32 rows, GEMM_W_BF16 =
    bf16 rows (ld then counts bf16 elements), a split precision = k-group form, | GEMM_W_FRAG = fragment order where the shape
    takes it.  Halves no element owns (between rows when ld > kk) hold `fill`."""
    M = np.ascontiguousarray(M, dtype=F32)
    nc, kk = M.shape
    ld = kk if ld is None else ld
    if (mode & ~GEMM_W_FRAG) == 0:
        out = np.full(((nc - 1) * ld + kk, 2), fill, dtype=np.uint16)
        rows = (np.arange(nc)[:, None] * ld + np.arange(kk)[None, :]).reshape(-1)
        out[rows] = M.reshape(-1).view(np.uint16).reshape(-1, 2)
        return out.reshape(-1)
    if (mode & ~GEMM_W_FRAG) == GEMM_W_BF16:
        out = np.full((nc - 1) * ld + kk, fill, dtype=np.uint16)
        out[(np.arange(nc)[:, None] * ld + np.arange(kk)[None, :]).reshape(-1)] = bf16_bits(M).reshape(-1)
        return out
    hi_i, lo_i, n = split_layout(nc, kk, mode, ld)
    hi, lo = split16(M, mode & ~GEMM_W_FRAG)
    out = np.full(n, fill, dtype=np.uint16)
    out[hi_i.reshape(-1)] = hi.reshape(-1)
    out[lo_i.reshape(-1)] = lo.reshape(-1)
    return out


def decode(buf, nc, kk, mode, ld=None):
    """The fp64 matrix [nc, kk] the halves `buf` stand for (the inverse of encode up to the rounding of the storage form)."""
    buf = np.asarray(buf, dtype=np.uint16)
    ld = kk if ld is None else ld
    rows = np.arange(nc)[:, None] * ld + np.arange(kk)[None, :]
    if (mode & ~GEMM_W_FRAG) == 0:
        return buf.reshape(-1, 2)[rows.reshape(-1)].reshape(-1).view(F32).reshape(nc, kk).astype(np.float64)
    if (mode & ~GEMM_W_FRAG) == GEMM_W_BF16:
        return bf16_value(buf[rows]).astype(np.float64)
    hi_i, lo_i, _ = split_layout(nc, kk, mode, ld)
    return join16(buf[hi_i], buf[lo_i], mode & ~GEMM_W_FRAG)


# ------------------------------------------------------------------ EdgeConv pack / unpack
def yw_of(H, Cout, shortcut, trans_inv):
    return (H if trans_inv == TI_COMPACT else 2 * H) + (Cout if shortcut else 0)


def edgeconv_pack_values(W1, b1, Ws, bs, Cin, Cp, H, Cout, shortcut, trans_inv):
    """-> wcat [Yw, Cp], bcat [Yw] in the dtype of W1: wcat = [Wa - Wb ; Wb ; Ws] (trans_inv 1: [-W1 ; W1 ; Ws], COMPACT: [W1 ;
    Ws]), bcat = [b1 ; 0 ; bs] (COMPACT: [0 ; bs] - b1 is not in bcat), columns Cin .. Cp - 1 zero, NULL biases = zeros."""
    W1 = np.asarray(W1)
    dt = W1.dtype
    W1 = W1.reshape(H, Cin if trans_inv else 2 * Cin)
    b1 = np.zeros(H, dt) if b1 is None else np.asarray(b1, dtype=dt)
    if trans_inv == TI_COMPACT:
        rows, bias = [W1], [np.zeros(H, dt)]
    elif trans_inv:
        rows, bias = [-W1, W1], [b1, np.zeros(H, dt)]
    else:
        rows, bias = [W1[:, :Cin] - W1[:, Cin:], W1[:, Cin:]], [b1, np.zeros(H, dt)]
    if shortcut:
        rows.append(np.asarray(Ws, dtype=dt).reshape(Cout, Cin))
        bias.append(np.zeros(Cout, dt) if bs is None else np.asarray(bs, dtype=dt))
    wcat = np.zeros((yw_of(H, Cout, shortcut, trans_inv), Cp), dt)
    wcat[:, :Cin] = np.concatenate(rows, 0)
    return wcat, np.concatenate(bias)


def edgeconv_pack(W1, b1, Ws, bs, W2, Cin, Cp, H, Cout, shortcut, trans_inv, fwd_mode, bwd_mode):
    """-> dict of the halves (uint16) of wcat [Yw, Cp] and w2s [Cout, H] = W2 (storage fwd_mode), wcatT [Cp, Yw] and w2T [H, Cout]
    (storage bwd_mode), and bcat as the halves of its fp32 values.  Each operand takes fragment order on its own shape."""
    wcat, bcat = edgeconv_pack_values(np.asarray(W1, dtype=F32), b1, Ws, bs, Cin, Cp, H, Cout, shortcut, trans_inv)
    W2 = np.asarray(W2, dtype=F32).reshape(Cout, H)
    return {'wcat': encode(wcat, fwd_mode), 'bcat': encode(bcat[None, :], 0), 'wcatT': encode(wcat.T, bwd_mode),
            'w2T': encode(W2.T, bwd_mode), 'w2s': encode(W2, fwd_mode)}


def edgeconv_unpack(dwb, dw2b, Cin, Cp, H, Cout, shortcut, trans_inv):
    """dwb [Yw, Cp + 1] (Cin columns used | bias gradient in column Cp), dw2b [Cout, H + 1] or None -> dict dW1, db1, dWs, dbs,
    dW2, db2 in the dtype of dwb; None = the contract leaves that output alone (db1 in COMPACT mode, the shortcut / second-Linear
    outputs without a shortcut / dw2b).  dWa = top, dWb = bottom - top (trans_inv 1: dW1 = bottom - top; COMPACT: dW1 = top)."""
    dwb = np.asarray(dwb).reshape(yw_of(H, Cout, shortcut, trans_inv), Cp + 1)
    top, out = dwb[:H], dict.fromkeys(('dW1', 'db1', 'dWs', 'dbs', 'dW2', 'db2'))
    if trans_inv == TI_COMPACT:
        out['dW1'], s0 = top[:, :Cin].copy(), H
    else:
        bot, s0 = dwb[H:2 * H], 2 * H
        diff = bot[:, :Cin] - top[:, :Cin]
        out['dW1'] = diff if trans_inv else np.concatenate([top[:, :Cin], diff], 1)
        out['db1'] = top[:, Cp].copy()
    if shortcut:
        out['dWs'], out['dbs'] = dwb[s0:s0 + Cout, :Cin].copy(), dwb[s0:s0 + Cout, Cp].copy()
    if dw2b is not None:
        dw2b = np.asarray(dw2b).reshape(Cout, H + 1)
        out['dW2'], out['db2'] = dw2b[:, :H].copy(), dw2b[:, H].copy()
    return out


# ------------------------------------------------------------------ SingleConvMeshNet layer passes, SAGE message, padding
def scmn_pack(W1, W2, g1, b1, g2, b2, cin, h2, cout, trans_inv):
    """-> wcat [2 h2, cin] = [Wa - Wb ; Wb] (trans_inv: [-W1 ; W1]), wcatT [cin, 2 h2], w2T [h2, cout], gb1 [2, h2], gb2 [2, cout]."""
    W1 = np.asarray(W1).reshape(h2, cin if trans_inv else 2 * cin)
    wcat = np.concatenate([-W1, W1] if trans_inv else [W1[:, :cin] - W1[:, cin:], W1[:, cin:]], 0)
    return {'wcat': wcat, 'wcatT': np.ascontiguousarray(wcat.T), 'w2T': np.ascontiguousarray(np.asarray(W2).reshape(cout, h2).T),
            'gb1': np.stack([g1, b1]), 'gb2': np.stack([g2, b2])}


def scmn_unpack(dwcat, cin, h2, trans_inv):
    """dwcat [2 h2, cin] -> dW1 [h2, 2 cin] = [top | bottom - top] (trans_inv: [h2, cin] = bottom - top)."""
    dwcat = np.asarray(dwcat).reshape(2 * h2, cin)
    diff = dwcat[h2:] - dwcat[:h2]
    return diff if trans_inv else np.concatenate([dwcat[:h2], diff], 1)


def pad_rows(x, Cin, Cp):
    """[x[:, :Cin] | zeros] as [N, Cp] (any dtype: bf16 rows travel as uint16, whose zero is bf16's +0)."""
    out = np.zeros((x.shape[0], Cp), x.dtype)
    out[:, :Cin] = x[:, :Cin]
    return out


def has_in_edge(rowptr, N):
    return np.ones(N, bool) if rowptr is None else np.diff(np.asarray(rowptr, dtype=np.int64)) > 0


def cols_axpy_rowmask(dst, src, rowptr, c0, c1, alpha, bf16=False):
    """dst[n, c] = fl(dst[n, c] + fl(alpha * src[n, c])) for c in [c0, c1) on the rows with an in-edge; every other element keeps
    its bits.  bf16: dst / src are uint16 bit patterns, the two operations run in fp32 and the result is rounded once to bf16."""
    out = dst.copy()
    rows = has_in_edge(rowptr, dst.shape[0])
    d, s = dst[rows, c0:c1], src[rows, c0:c1]
    if bf16:
        out[rows, c0:c1] = bf16_bits(bf16_value(d) + F32(alpha) * bf16_value(s))
    else:
        out[rows, c0:c1] = d + F32(alpha) * s
    return out


def bn_affine_res(x, mean, rstd, gamma, beta, rowptr, res, relu):
    """y = [relu](res + [row has an in-edge] * (gamma * ((x - mean) * rstd) + beta)), every operation rounded on its own in this
    order: the affine, `* has_in` (a multiplication by 1.0 or 0.0), `res + .`, relu = (z > 0 ? z : +0): NaN and -0 become +0."""
    with np.errstate(all='ignore'):                                          # (inf * 0 = NaN is part of the contract)
        z = gamma[None, :] * ((x - mean[None, :]) * rstd[None, :]) + beta[None, :]
        z = z * has_in_edge(rowptr, x.shape[0]).astype(F32)[:, None]
        if res is not None:
            z = res + z
    if relu:
        z = np.where(z > 0, z, F32(0.0))
    return z.astype(F32)


def relu_mask_bwd(g, y, rowptr, relu):
    """-> g_eff = g where y > 0 else +0 (relu == 0: g), g_in = g_eff on rows with an in-edge else +0; !(y > 0) covers NaN, -0."""
    g_eff = np.where(y > 0, g, F32(0.0)).astype(F32) if relu else g.copy()
    return g_eff, np.where(has_in_edge(rowptr, g.shape[0])[:, None], g_eff, F32(0.0)).astype(F32)


def norm_bwd_coef(T1, S0, rstd, inv_cnt):
    """k = ((-((rstd * rstd) * rstd)) * T1) * inv_cnt[b], m = (-(rstd * S0)) * inv_cnt[b]; operands [B, C], inv_cnt [B]."""
    ic = inv_cnt[:, None]
    return (-((rstd * rstd) * rstd)) * T1 * ic, (-(rstd * S0)) * ic


def norm_bwd_coef_m_quirk(S0, U, rstd, inv_cnt):
    """m = (-((rstd * S0) + U)) * inv_cnt[b]."""
    return (-((rstd * S0) + U)) * inv_cnt[:, None]


# ------------------------------------------------------------------ Adam
def adam(p, g, m, v, vmax, lr, b1, b2, eps, wd, step, amsgrad):
    """One step on float32 arrays -> (p, m, v, vmax) (vmax returned as given when amsgrad == 0).  The host scalars are formed in
    double and cast once: -(lr / (1 - b1^t)), 1 - b1, b2, 1 - b2, eps, wd, sqrt(1 - b2^t).  Per element, each operation rounded:
    g' = g + wd * p (wd != 0); m' = m + (1 - b1) * (g' - m); v' = b2 * v + ((1 - b2) * g') * g'; vh = max(vmax, v');
    p' = p + (nss * m') / (sqrt(vh) / bc2s + eps)."""
    nss = F32(-(lr / (1.0 - math.pow(b1, step))))
    omb1, b2f, omb2, epsf, wdf = F32(1.0 - b1), F32(b2), F32(1.0 - b2), F32(eps), F32(wd)
    bc2s = F32(math.sqrt(1.0 - math.pow(b2, step)))
    gi = g + wdf * p if wdf != 0 else g
    mi = m + omb1 * (gi - m)
    vi = b2f * v + (omb2 * gi) * gi
    vh = np.maximum(vmax, vi) if amsgrad else vi
    denom = np.sqrt(vh) / bc2s + epsf
    pn = p + (nss * mi) / denom
    assert all(a.dtype == F32 for a in (pn, mi, vi, vh))
    return pn, mi, vi, (vh if amsgrad else vmax)


# ------------------------------------------------------------------ fixed-order fp64 sums of the loss and the metrics
def _tree256(a):
    """a [blocks, 256] fp64 -> [blocks]: the pairwise tree s = 128 .. 1 (element t += element t + s)."""
    a = a.copy()
    s = 128
    while s > 0:
        a[:, :s] += a[:, s:2 * s]
        s >>= 1
    return a[:, 0].copy()


def block_sums(terms):
    """fp64 terms, one per thread in launch order -> one partial per 256-thread block (threads past the end add 0.0)."""
    n = terms.shape[0]
    blocks = (n + 255) // 256
    a = np.zeros(blocks * 256, np.float64)
    a[:n] = terms
    return _tree256(a.reshape(blocks, 256))


def final_sum(partial, inv):
    """k_loss_final: thread t adds partial[t], partial[t + 256], ... in that order, the 256 sums go through the same tree, the
    result is multiplied by (double)inv and cast once to fp32."""
    n = partial.shape[0]
    rounds = (n + 255) // 256
    a = np.zeros(rounds * 256, np.float64)
    a[:n] = partial
    acc = np.zeros(256, np.float64)
    for row in a.reshape(rounds, 256):
        acc = acc + row
    return F32(_tree256(acc[None, :])[0] * float(F32(inv)))


def masked_l1(out, color, mask, use_weight, w=None):
    """-> (grad [N, C] float32, loss float32).  w [N] float32 = the per-vertex weight 0.99^mask as the caller evaluates it (the
    accuracy of the device's powf is not part of this restatement); ignored without use_weight.  inv = fl(1 / (float)(N C));
    rows with mask > 0: d = out - color, grad = (sign(d) * w) * inv, term = (double)(|d| * w); other rows: grad = +0, term = 0."""
    N, C = out.shape
    inv = F32(1.0) / F32(N * C)
    w = np.asarray(w, dtype=F32) if use_weight else np.ones(N, F32)
    on = (np.asarray(mask) > 0)[:, None]
    d = np.where(on, out - color, F32(0.0)).astype(F32)
    grad = np.where(on, (np.sign(d) * w[:, None]) * inv, F32(0.0)).astype(F32)
    terms = (np.abs(d) * w[:, None]).astype(F32).astype(np.float64).reshape(-1)
    return grad, final_sum(block_sums(terms), inv)


def _csr_fold(values, rowptr, acc):
    """acc[i] += values[e] for e = rowptr[i] .. rowptr[i + 1] - 1, in that order, in the dtype of acc."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    deg = np.diff(rowptr)
    for k in range(int(deg.max()) if deg.size else 0):
        rows = np.nonzero(deg > k)[0]
        acc[rows] = acc[rows] + values[rowptr[rows] + k]
    return acc


def total_variation(x, rowptr, col):
    """out = (float)(sum * (double)inv), inv = fl(1 / fl((float)N * (float)C)); per destination row i (one thread each, 256 per
    block) an fp64 sum over its CSR entries e, in order, of (double)s_e with s_e = the fp32 sum over c, in order, of
    |x[col[e], c] - x[i, c]| starting from 0; block partials and their fold as in the loss."""
    N, C = x.shape
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    dst = np.repeat(np.arange(N, dtype=np.int64), np.diff(rowptr))
    s = np.zeros(col.shape[0], F32)
    for c in range(C):
        s = s + np.abs(x[col, c] - x[dst, c])
    acc = _csr_fold(s.astype(np.float64), rowptr, np.zeros(N, np.float64))
    return final_sum(block_sums(acc), F32(1.0) / (F32(N) * F32(C)))


def graph_laplace(x, rowptr, col):
    """out[i, c] = s - fl((float)deg_i * x[i, c]), s = the fp32 sum of x[col[e], c] over the CSR entries of row i, in order, from 0."""
    N, C = x.shape
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    s = _csr_fold(x[col], rowptr, np.zeros((N, C), F32))
    return (s - np.diff(rowptr).astype(F32)[:, None] * x).astype(F32)
