"""torch.autograd bindings of the HIP kernels (libstin_hip.so) - the operator layer
the nn.Modules in surfacetextureinpaintingnet.py are written on.

Every function here runs on GPU tensors only and calls through the C ABI
(include/stin_hip.h); there is no eager/CPU fallback.  The dense per-vertex GEMMs are
the hand-written MFMA kernels too (gemm_nt / gemm_tn); the library-GEMM A/B aid of round 1 lives in
profiles/gemm_bench.py, outside the package.
"""
import collections
import ctypes
import dataclasses
import os

import torch

from . import _lib
from .plan import _ptr, _stream

EPS = 1e-5
# save the edge-stage ReLU decisions as a bit-mask in forward (STIN_EDGE_MASK=0: recompute them in backward)
USE_EDGE_MASK = os.environ.get('STIN_EDGE_MASK', '1') != '0'
_C = _lib.CONSTANTS                 # the integer #defines of include/stin_hip.h
RED_SUM, RED_CSQ, RED_DOT_ELU, RED_COEF_XC, RED_MOMENTS, RED_DOT_BN, RED_DOT_BN_RELU = (_C[n] for n in (
    'STIN_RED_SUM', 'STIN_RED_CSQ', 'STIN_RED_DOT_ELU', 'STIN_RED_COEF_XC', 'STIN_RED_MOMENTS', 'STIN_RED_DOT_BN',
    'STIN_RED_DOT_BN_RELU'))
POST_NONE, POST_SCALE, POST_RSTD, POST_NORM_COEF = (_C[n] for n in (
    'STIN_POST_NONE', 'STIN_POST_SCALE', 'STIN_POST_RSTD', 'STIN_POST_NORM_COEF'))
SEG_NONTEMPORAL = _C['STIN_SEG_NONTEMPORAL']


def _mat(t):
    """2-D fp32 (or bf16-storage) GPU tensor with unit inner stride -> (tensor, ld)."""
    if not (t.dim() == 2 and t.dtype in (torch.float32, torch.bfloat16) and t.is_cuda):
        raise TypeError('the STINet HIP path takes 2-D float32 (or bfloat16-storage) CUDA tensors (no CPU / eager '
                        'fallback exists); got shape %s dtype %s device %s' % (tuple(t.shape), t.dtype, t.device))
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0)))


def _sfx(t):
    """C-ABI suffix of the kernel family for a tensor's storage type."""
    return '_bf16' if t.dtype == torch.bfloat16 else '_f32'


def _same(ref, *ts):
    """The optional operands of a kernel must share the storage type of its main operand."""
    for t in ts:
        if t is not None and t.dtype != ref.dtype:
            raise TypeError('mixed storage types in one kernel call: %s vs %s' % (ref.dtype, t.dtype))


class KernelTimer:
    """Optional HIP-event bracket around chosen C-ABI launches (bench.py's live roofline numbers).
    Events are recorded on the stream the kernel is enqueued on (torch's current stream)."""
    enabled = False
    names = ()
    records = []          # (name, tag, start_event, end_event)
    max_records = 400     # thousands of outstanding timing events slow the HIP runtime down: sample, do not flood
    in_net = False        # round 3: edge-stage brackets INSIDE the whole-network call (stin_net_op_t::ev_edge0 / 1) - the step stays
                          # on the fast path (one C call per direction); other names still need the per-kernel path

    @classmethod
    def start(cls, names, max_records=400, in_net=False):
        cls.enabled, cls.names, cls.records, cls.max_records = True, tuple(names), [], max_records
        cls.in_net = bool(in_net)

    @classmethod
    def per_kernel_path(cls):
        """True while brackets are on that only the per-kernel host path can place."""
        return cls.enabled and not cls.in_net

    @classmethod
    def edge_events(cls, name, tag):
        """-> (ev0, ev1) raw hipEvent_t handles bracketing one edge-stage launch inside stin_net_fwd / _bwd, or (0, 0)."""
        if not (cls.enabled and cls.in_net and name in cls.names) or len(cls.records) >= cls.max_records:
            return 0, 0
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()                                  # (creates the handles; the call re-records them around the kernel)
        b.record()
        cls.records.append((name, tag, a, b))
        return a.cuda_event, b.cuda_event

    @classmethod
    def stop(cls):
        cls.enabled = False
        cls.in_net = False
        torch.cuda.synchronize()
        out = {}
        for name, tag, a, b in cls.records:
            out.setdefault((name, tag), []).append(a.elapsed_time(b) * 1e-3)
        cls.records = []
        return out


def _call(name, *args, tag=None):
    if KernelTimer.enabled and name in KernelTimer.names:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.check(getattr(_lib.load(), name)(*args), name)
        b.record()
        KernelTimer.records.append((name, tag, a, b))
        if len(KernelTimer.records) >= KernelTimer.max_records:
            KernelTimer.enabled = False          # the rest of the timed region runs un-instrumented
        return
    _lib.check(getattr(_lib.load(), name)(*args), name)


# ------------------------------------------------------------------ raw kernel wrappers
def edge_relu_mean_fwd(A, B, csr, out, indicator=False, mask=None):
    A, lda = _mat(A)
    B, ldb = _mat(B)
    _same(A, B, out)
    H = A.shape[1]
    _call('stin_edge_relu_mean_fwd' + _sfx(A), _ptr(A), lda, _ptr(B), ldb, _ptr(csr.rowptr), _ptr(csr.col), A.shape[0], H,
          _ptr(out), out.stride(0), int(indicator), _ptr(mask), _stream(A), tag=(A.shape[0], csr.n_entries, H))
    return out


def edge_mask_supported(H):
    """The saved-ReLU-mask path stores wave-ballot words of full rows: H = 128, 256, 512, 1024 or 2048."""
    return H in (128, 256, 512, 1024, 2048)


def edge_relu_mean_bwd_dst_mask(G, mask, csr, dA):
    G, ldg = _mat(G)
    _same(G, dA)
    _call('stin_edge_relu_mean_bwd_dst_mask' + _sfx(G), _ptr(G), ldg, _ptr(mask), _ptr(csr.rowptr), G.shape[0], G.shape[1],
          _ptr(dA), dA.stride(0), _stream(G), tag=(G.shape[0], csr.n_entries, G.shape[1]))
    return dA


def edge_relu_mean_bwd_src_mask(G, mask, edges, dB):
    G, ldg = _mat(G)
    cs = edges.by_src
    _same(G, dB)
    _call('stin_edge_relu_mean_bwd_src_mask' + _sfx(G), _ptr(G), ldg, _ptr(edges.w_src), _ptr(mask), _ptr(cs.rowptr),
          _ptr(cs.col), _ptr(edges.xslot), G.shape[0], G.shape[1], _ptr(dB), dB.stride(0), _stream(G),
          tag=(G.shape[0], cs.n_entries, G.shape[1]))
    return dB


def edge_relu_mean_bwd_mask(G, mask, edges, dA, dB, copy_src=None, copy_dst=None):
    """dA and dB of the mask backward in one launch (bit-identical to the two separate kernels); optionally
    copy_dst[:, :] = copy_src (row views of the same height) in the same launch."""
    G, ldg = _mat(G)
    cs = edges.by_src
    _same(G, dA)
    _same(G, dB)
    cp = (None, 0, None, 0, 0)
    if copy_src is not None:
        _same(G, copy_src, copy_dst)
        cp = (_ptr(copy_src), copy_src.stride(0), _ptr(copy_dst), copy_dst.stride(0), copy_src.shape[1])
    _call('stin_edge_relu_mean_bwd_mask' + _sfx(G), _ptr(G), ldg, _ptr(mask), _ptr(edges.by_dst.rowptr), _ptr(edges.w_src),
          _ptr(cs.rowptr), _ptr(cs.col), _ptr(edges.xslot), G.shape[0], G.shape[1], _ptr(dA), dA.stride(0), _ptr(dB),
          dB.stride(0), *cp, _stream(G), tag=(G.shape[0], cs.n_entries, G.shape[1]))
    return dA, dB


def edge_relu_mean_fwd_ti(b1, B, csr, out, indicator=False, mask=None):
    """h = mean_j ReLU(A_i + B_j) with A_i = fl(b1 - B_i) formed per row (translation-invariant filter, compact layout): the same
    bits as edge_relu_mean_fwd given that A.  b1 [H] or None.  fp32 rows, saved-mask widths."""
    B, ldb = _mat(B)
    _same(B, out)
    H = B.shape[1]
    _call('stin_edge_relu_mean_fwd_ti_f32', _ptr(b1), _ptr(B), ldb, _ptr(csr.rowptr), _ptr(csr.col), B.shape[0], H,
          _ptr(out), out.stride(0), int(indicator), _ptr(mask), _stream(B), tag=(B.shape[0], csr.n_entries, H))
    return out


def edge_relu_mean_bwd_mask_ti(G, mask, edges, D, copy_src=None, copy_dst=None):
    """D = dB - dA of the mask backward in one row of H columns (compact trans-inv layout) -> db1 = sum_i dA_i [H] (the kernel's
    per-workgroup column partials, folded in a fixed order)."""
    G, ldg = _mat(G)
    cs = edges.by_src
    _same(G, D)
    N, H = G.shape
    rows = int(_lib.load().stin_edge_bwd_ti_colsum_rows(N, H))
    colsum = torch.empty(max(rows, 1), H, dtype=torch.float32, device=G.device)
    cp = (None, 0, None, 0, 0)
    if copy_src is not None:
        _same(G, copy_src, copy_dst)
        cp = (_ptr(copy_src), copy_src.stride(0), _ptr(copy_dst), copy_dst.stride(0), copy_src.shape[1])
    _call('stin_edge_relu_mean_bwd_mask_ti_f32', _ptr(G), ldg, _ptr(mask), _ptr(edges.by_dst.rowptr), _ptr(edges.w_src),
          _ptr(cs.rowptr), _ptr(cs.col), _ptr(edges.xslot), N, H, _ptr(D), D.stride(0), *cp, _ptr(colsum), rows, _stream(G),
          tag=(N, cs.n_entries, H))
    db1 = torch.empty(H, dtype=torch.float32, device=G.device)
    _call('stin_edge_bwd_ti_colsum_fold_f32', _ptr(colsum), rows if N > 0 else 0, H, _ptr(db1), _stream(G))
    return db1


def edge_relu_mean_bwd_dst(A, B, G, csr, dA):
    A, lda = _mat(A)
    B, ldb = _mat(B)
    G, ldg = _mat(G)
    _call('stin_edge_relu_mean_bwd_dst_f32', _ptr(A), lda, _ptr(B), ldb, _ptr(G), ldg, _ptr(csr.rowptr), _ptr(csr.col),
          A.shape[0], A.shape[1], _ptr(dA), dA.stride(0), _stream(A), tag=(A.shape[0], csr.n_entries, A.shape[1]))
    return dA


def edge_relu_mean_bwd_src(A, B, G, inv_deg, csr_src, dB):
    A, lda = _mat(A)
    B, ldb = _mat(B)
    G, ldg = _mat(G)
    _call('stin_edge_relu_mean_bwd_src_f32', _ptr(A), lda, _ptr(B), ldb, _ptr(G), ldg, _ptr(inv_deg),
          _ptr(csr_src.rowptr), _ptr(csr_src.col), A.shape[0], A.shape[1], _ptr(dB), dB.stride(0), _stream(A),
          tag=(A.shape[0], csr_src.n_entries, A.shape[1]))
    return dB


def segment_sum(src, rowptr, col, n_rows, mean=False):
    src, ld = _mat(src)
    out = torch.empty(n_rows, src.shape[1], dtype=src.dtype, device=src.device)
    # (a source that cannot be Infinity-Cache resident is read with non-temporal loads)
    flags = int(mean) | (SEG_NONTEMPORAL if (src.dtype == torch.float32 and src.shape[0] * ld * 4 > (256 << 20)) else 0)
    _call('stin_segment_sum' + _sfx(src), _ptr(src), ld, _ptr(rowptr), _ptr(col), n_rows, src.shape[1], flags, _ptr(out),
          out.stride(0) if n_rows > 1 else src.shape[1], _stream(src), tag=(int(src.shape[0]), int(n_rows), int(src.shape[1])))
    return out


def gather_rows(src, idx, row_scale=None):
    src, ld = _mat(src)
    n = idx.numel()
    out = torch.empty(n, src.shape[1], dtype=src.dtype, device=src.device)
    _call('stin_gather_rows' + _sfx(src), _ptr(src), ld, _ptr(idx), _ptr(row_scale), n, src.shape[1], _ptr(out), src.shape[1],
          _stream(src))
    return out


def batch_pool(batch, pool):
    out = torch.empty(pool.n_coarse, dtype=torch.int64, device=batch.device)
    _call('stin_batch_pool_i64', _ptr(batch), _ptr(pool.children.rowptr), _ptr(pool.children.col), pool.n_coarse, _ptr(out),
          _stream(batch))
    return out


def batch_unpool(batch, pool):
    out = torch.empty(pool.n_fine, dtype=torch.int64, device=batch.device)
    _call('stin_gather_i64', _ptr(batch), _ptr(pool.trace), pool.n_fine, _ptr(out), _stream(batch))
    return out


def colreduce(mode, x, groups, ptr, *, gout=None, mean=None, rstd=None, coef=None, post=POST_NONE, eps=EPS,
              use_sid=False):
    """Column sums of `x` rows over the ranges `ptr` (None: all rows) -> [B, C] (two for DOT_ELU)."""
    lib = _lib.load()
    x, ldx = _mat(x)
    N, C = x.shape
    B = groups.B
    out0 = torch.empty(B, C, dtype=torch.float32, device=x.device)
    out1 = torch.empty(B, C, dtype=torch.float32, device=x.device) if mode in (RED_DOT_ELU, RED_MOMENTS, RED_DOT_BN, RED_DOT_BN_RELU) else None
    ldg = 0
    if gout is not None:
        gout, ldg = _mat(gout)
        _same(x, gout)
    ws_bytes = lib.stin_colreduce_workspace_bytes(C, B)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    _call('stin_colreduce' + _sfx(x), mode, _ptr(x), ldx, _ptr(gout), ldg, N, C, _ptr(ptr), B, _ptr(groups.gid),
          _ptr(groups.sid if use_sid else None), _ptr(mean), _ptr(rstd), _ptr(coef), post, _ptr(groups.inv_cnt),
          float(eps), _ptr(out0), _ptr(out1), _ptr(ws), ws_bytes, _stream(x))
    return (out0, out1) if out1 is not None else out0


def colsum(x):
    """[N, C] -> [C] column sums (bias gradients), fixed summation order."""
    class _One:
        B, gid, sid, inv_cnt = 1, None, None, None
    return colreduce(RED_SUM, x, _One, None).view(-1)


def instance_stats(x, groups, eps=EPS):
    """-> (mean, rstd) [B, C]: biased variance, eps inside the sqrt (F.instance_norm /
    FastInstanceNorm semantics, reference models/modules/fastinstancenorm.py:44-98)."""
    if groups.gid is None and x.shape[0] == 1:   # F.instance_norm's own check on the batch=None branch
        raise ValueError('Expected more than 1 spatial element when training, got input size {}'.format(
            torch.Size([1, x.shape[1], 1])))
    if not groups.quirk:
        # one pass: fp64 sum x and sum x^2 over each graph's rows (slices == graphs here)
        return colreduce(RED_MOMENTS, x, groups, groups.ptr_sum, eps=eps)
    # linspace-slice quirk: sums over slices, centring through the graph id -> two passes as the reference does
    mean = colreduce(RED_SUM, x, groups, groups.ptr_sum, post=POST_SCALE)
    rstd = colreduce(RED_CSQ, x, groups, groups.ptr_sum, mean=mean, post=POST_RSTD, eps=eps)
    return mean, rstd


def norm_act_res_fwd(x, mean, rstd, groups, res=None, act=True):
    x, ldx = _mat(x)
    N, C = x.shape
    ldres = 0
    if res is not None:
        res, ldres = _mat(res)
        _same(x, res)
    y = torch.empty(N, C, dtype=x.dtype, device=x.device)
    _call('stin_norm_act_res_fwd' + _sfx(x), _ptr(x), ldx, _ptr(mean), _ptr(rstd), _ptr(groups.gid), _ptr(res), ldres, N, C,
          int(act), _ptr(y), C, _stream(x))
    return y


def instance_norm_act_bwd(x, gout, mean, rstd, groups, act=True, out=None):
    """d/dx of y = act((x - mean[g]) * rstd[g]) with the statistics taken over `groups`
    (incl. the linspace-slice quirk: sums over slices sigma, centring through g)."""
    x, ldx = _mat(x)
    gout, ldg = _mat(gout)
    _same(x, gout, out)
    N, C = x.shape
    if act:
        T1, S0 = colreduce(RED_DOT_ELU, x, groups, groups.ptr_true, gout=gout, mean=mean, rstd=rstd)
    else:
        # without activation dY = gout: sum dY*xc and sum dY via the same kernel with rstd = 0 -> ELU'(0)=1
        T1, S0 = colreduce(RED_DOT_ELU, x, groups, groups.ptr_true, gout=gout, mean=mean, rstd=torch.zeros_like(rstd))
    if not groups.quirk:                                            # sum_g xc = 0 when slices == graphs
        k = torch.empty_like(rstd)
        m = torch.empty_like(rstd)
        _call('stin_norm_bwd_coef_f32', _ptr(T1), _ptr(S0), _ptr(rstd), _ptr(groups.inv_cnt), rstd.shape[0], C, _ptr(k),
              _ptr(m), _stream(x))
    else:
        # k = -(rstd^3) T1 / n, indexed by the SUM slice (sid): the coefficient kernel's k (its m is overwritten below) - the same
        # float operations as the four framework launches this replaces, as the slice-quirk path of stin_net_bwd's block op does
        k = torch.empty_like(rstd)
        m = torch.empty_like(rstd)
        _call('stin_norm_bwd_coef_f32', _ptr(T1), _ptr(S0), _ptr(rstd), _ptr(groups.inv_cnt), rstd.shape[0], C, _ptr(k),
              _ptr(m), _stream(x))
        U = colreduce(RED_COEF_XC, x, groups, groups.ptr_true, mean=mean, coef=k, use_sid=True)
        _call('stin_norm_bwd_coef_m_quirk_f32', _ptr(S0), _ptr(U), _ptr(rstd), _ptr(groups.inv_cnt), rstd.shape[0], C, _ptr(m),
              _stream(x))
    dx = out if out is not None else torch.empty(N, C, dtype=x.dtype, device=x.device)
    _call('stin_norm_act_bwd' + _sfx(x), _ptr(x), ldx, _ptr(gout), ldg, _ptr(mean), _ptr(rstd), _ptr(rstd), _ptr(k.contiguous()),
          _ptr(m.contiguous()), _ptr(groups.gid), _ptr(groups.sid), N, C, int(act), _ptr(dx), dx.stride(0), _stream(x))
    return dx


GEMM_F32, GEMM_BF16X3, GEMM_BF16X6, GEMM_F16X3 = (_C[n] for n in (
    'STIN_GEMM_F32', 'STIN_GEMM_BF16X3', 'STIN_GEMM_BF16X6', 'STIN_GEMM_F16X3'))
PREC_NAMES = {GEMM_F32: 'fp32', GEMM_BF16X3: 'bf16x3', GEMM_BF16X6: 'bf16x6', GEMM_F16X3: 'fp16x3'}
# matrix-core path per GEMM role (env override for A/B experiments: STIN_GEMM_FWD / STIN_GEMM_BWD = 0 | 2 | 3 | 4)
# Defaults: forward GEMMs on the 2-piece fp16 split (3 MFMAs; rms 1-5e-7 against fp64 = the fp32 MFMA chain's
# accuracy on unit-scale activations, 1.7x faster than it; whole-net forward error 5-6e-6 like fp32 and bf16x6,
# where bf16x3 gives 1.2e-4); backward GEMMs on the 2-piece bf16 split (gradients need bf16's exponent range;
# rms 4e-6, far inside the 1e-3 gradient tolerance).
PREC_FWD = int(os.environ.get('STIN_GEMM_FWD', GEMM_F16X3))
PREC_BWD = int(os.environ.get('STIN_GEMM_BWD', GEMM_BF16X3))
GEMM_W_PRESPLIT = _C['STIN_GEMM_W_PRESPLIT']   # nt: the weight operand already holds its two 16-bit pieces (stin_hip.h)
GEMM_W_BF16 = _C['STIN_GEMM_W_BF16']           # stin_gemm_nt_bf16: the weight operand holds bf16 [Nc][K] (stin_hip.h)
# pre-split operands in MFMA fragment order where the shape allows (stin_hip.h STIN_GEMM_W_FRAG): what the resident-strip NT
# kernel reads.  Without the flag the operand keeps the k-group layout and with it the tiled kernel (tests flip GEMM_W_FRAG for that A/B).
GEMM_W_FRAG = _C['STIN_GEMM_W_FRAG']           # (a module constant since round 6; tests flip the attribute)
WEIGHT_PRESPLIT = True
# one C call per direction for a GraphResnetBlock or a run of them (NetFn: stin_net_fwd / _bwd enqueue the same kernels in the
# same order as the per-kernel path of EdgeConvBlockFn): removes ~25 Python-level foreign calls per block.  STIN_BLOCK_CALL=0 =
# per-kernel path.
USE_BLOCK_CALL = os.environ.get('STIN_BLOCK_CALL', '1') != '0'


def gemm_nt_colstats(A, W, bias, row_mask, precision, n_cols):
    """hE W2^T + masked bias AND the first stage of the column statistics of the result in one launch, or None when this
    shape / precision has no all-columns kernel.  -> (C, partial [groups, 2, n_cols] float64)."""
    A, lda = _mat(A)
    M, K = A.shape
    lib = _lib.load()
    groups = int(lib.stin_gemm_nt_colstats_groups(M, n_cols, K, int(precision))) if A.dtype == torch.float32 else 0
    if groups <= 0 or groups > 1024:
        return None
    C = torch.empty(M, n_cols, dtype=torch.float32, device=A.device)
    partial = torch.empty(groups, 2, n_cols, dtype=torch.float64, device=A.device)
    mk, ldm = (row_mask, row_mask.stride(0)) if row_mask is not None else (None, 0)
    _call('stin_gemm_nt_colstats_f32', _ptr(A), lda, _ptr(W), K, _ptr(bias), _ptr(mk), ldm, None, 0, M, n_cols, K, _ptr(C), n_cols,
          int(precision), _ptr(partial), partial.numel() * 8, _stream(A), tag=(M, n_cols, K))
    return C, partial


def gemm_nt_dotelu(A, W, residual, precision, n_cols, nx, nmean, nrstd):
    """A W^T (+ residual) AND the first stage of the instance-norm + ELU backward statistics of the layer whose output gradient
    the product is (nx / nmean / nrstd: that layer's pre-norm rows and statistics), or None when the shape is not served by the
    panel kernel.  -> (C, partial [groups, 2, n_cols] float64).  (stin_gemm_nt_dotelu_f32; test / probe helper - the block
    backward calls it inside stin_net_bwd.)"""
    A, lda = _mat(A)
    M, K = A.shape
    lib = _lib.load()
    groups = int(lib.stin_gemm_nt_dotelu_groups(M, n_cols, K, int(precision))) if A.dtype == torch.float32 else 0
    if groups <= 0:
        return None
    C = torch.empty(M, n_cols, dtype=torch.float32, device=A.device)
    partial = torch.empty(groups, 2, n_cols, dtype=torch.float64, device=A.device)
    res, ldr = (residual, residual.stride(0)) if residual is not None else (None, 0)
    _call('stin_gemm_nt_dotelu_f32', _ptr(A), lda, _ptr(W), K, None, _ptr(res), ldr, M, n_cols, K, _ptr(C), n_cols, int(precision),
          _ptr(nx), nx.stride(0), _ptr(nmean), _ptr(nrstd), _ptr(partial), partial.numel() * 8, _stream(A), tag=(M, n_cols, K))
    return C, partial


def norm_coef_from_partials(partial, rstd, inv_cnt):
    """Second stage: the instance-norm backward coefficients k, m [1, C] of one graph from gemm_nt_dotelu's partials."""
    groups, _, C = partial.shape
    out = torch.empty(2, 1, C, dtype=torch.float32, device=partial.device)
    _call('stin_norm_coef_from_partials_f32', _ptr(partial), groups, C, _ptr(rstd), _ptr(inv_cnt), _ptr(out[0]), _ptr(out[1]),
          _stream(partial))
    return out[0], out[1]


def moments_final(partial, inv_cnt, eps=EPS):
    """Second stage: mean, rstd [1, C] of one instance (inv_cnt [1] = 1 / rows)."""
    groups, _, C = partial.shape
    out = torch.empty(2, 1, C, dtype=torch.float32, device=partial.device)
    _call('stin_moments_final_f32', _ptr(partial), groups, C, _ptr(inv_cnt), float(eps), _ptr(out[0]), _ptr(out[1]), _stream(partial))
    return out[0], out[1]


def gemm_nt(A, W, bias=None, out=None, row_mask=None, precision=GEMM_F32, residual=None, out_dtype=None):
    """A[M, K] . W[Nc, K]^T + bias * row_mask -> [M, Nc]  (hand-written MFMA kernels).
    row_mask: optional [M] column view (stride = its row pitch) multiplying the bias per row.
    A in bf16 storage: W and bias stay fp32, one bf16 MFMA per k-step (`precision` is ignored), the result is bf16
    unless out_dtype=torch.float32."""
    if A.dtype == torch.bfloat16:
        return _gemm_nt_bf16(A, W, bias, out, row_mask, residual, out_dtype)
    A, lda = _mat(A)
    W, ldw = _mat(W)
    M, K = A.shape
    Nc = W.shape[0]
    assert W.shape[1] == K
    if out is None:
        out = torch.empty(M, Nc, dtype=torch.float32, device=A.device)
    ld_res = 0
    if residual is not None:
        residual, ld_res = _mat(residual)
    _call('stin_gemm_nt_f32', _ptr(A), lda, _ptr(W), ldw, _ptr(bias), _ptr(row_mask),
          row_mask.stride(0) if row_mask is not None else 0, _ptr(residual), ld_res, M, Nc, K, _ptr(out),
          out.stride(0) if M > 1 else max(Nc, out.stride(0)), int(precision), _stream(A), tag=(M, Nc, K))
    return out


def _gemm_nt_bf16(A, W, bias, out, row_mask, residual, out_dtype):
    A, lda = _mat(A)
    W, ldw = _mat(W)
    if W.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError('gemm_nt on bf16 activations takes the fp32 master weights or their bf16 rounding')
    _same(A, row_mask, residual)
    M, K = A.shape
    Nc = W.shape[0]
    assert W.shape[1] == K
    if out is None:
        out = torch.empty(M, Nc, dtype=out_dtype or torch.bfloat16, device=A.device)
    ld_res = 0
    if residual is not None:
        residual, ld_res = _mat(residual)
    _call('stin_gemm_nt_bf16', _ptr(A), lda, _ptr(W), ldw, _ptr(bias), _ptr(row_mask),
          row_mask.stride(0) if row_mask is not None else 0, _ptr(residual), ld_res, M, Nc, K, _ptr(out),
          out.stride(0) if M > 1 else max(Nc, out.stride(0)),
          int(out.dtype == torch.float32) | (GEMM_W_BF16 if W.dtype == torch.bfloat16 else 0), _stream(A), tag=(M, Nc, K))
    return out


def split_weights(W, precision):
    """fp32 W [Nc, K] -> the STIN_GEMM_W_PRESPLIT form for `precision` (GEMM_BF16X3 or GEMM_F16X3, optionally
    | GEMM_W_FRAG: fragment order where the shape allows - pass the same flag to gemm_nt), same shape."""
    W, ldw = _mat(W)
    out = torch.empty_like(W, memory_format=torch.contiguous_format)
    _call('stin_gemm_split_weights_f32', _ptr(W), ldw, W.shape[0], W.shape[1], int(precision), _ptr(out), W.shape[1],
          _stream(W))
    return out


def gemm_tn(G, X, ones_column=False, row_weight=None, precision=GEMM_F32):
    """G[M, Nc]^T . [X[M, K] | w] -> [Nc, K (+1)]  (weight gradient; last column = bias gradient
    sum_m w[m] G[m, :], w = row_weight (an [M] column view) or 1).  bf16-storage operands -> fp32 result."""
    if G.dtype == torch.bfloat16:
        lib = _lib.load()
        G, ldg = _mat(G)
        X, ldx = _mat(X)
        _same(G, X, row_weight)
        M, Nc = G.shape
        K = X.shape[1]
        assert X.shape[0] == M
        Kp = K + int(ones_column)
        out = torch.empty(Nc, Kp, dtype=torch.float32, device=G.device)
        ws_bytes = lib.stin_gemm_tn_workspace_bytes(M, Nc, K, int(ones_column))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=G.device)
        _call('stin_gemm_tn_bf16', _ptr(G), ldg, _ptr(X), ldx, M, Nc, K, int(ones_column), _ptr(row_weight),
              row_weight.stride(0) if row_weight is not None else 0, _ptr(out), Kp, _ptr(ws), ws_bytes, _stream(G),
              tag=(M, Nc, K))
        return out
    lib = _lib.load()
    G, ldg = _mat(G)
    X, ldx = _mat(X)
    M, Nc = G.shape
    K = X.shape[1]
    assert X.shape[0] == M
    Kp = K + int(ones_column)
    out = torch.empty(Nc, Kp, dtype=torch.float32, device=G.device)
    ws_bytes = lib.stin_gemm_tn_workspace_bytes(M, Nc, K, int(ones_column))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=G.device)
    _call('stin_gemm_tn_f32', _ptr(G), ldg, _ptr(X), ldx, M, Nc, K, int(ones_column), _ptr(row_weight),
          row_weight.stride(0) if row_weight is not None else 0, _ptr(out), Kp, int(precision), _ptr(ws), ws_bytes,
          _stream(G),
          tag=(M, Nc, K))
    return out


def gemm_tn_wb(G, X, dW, db, precision=GEMM_F32):
    """dW[Nc, K] = G^T X and db[Nc] = column sums of G, written into the two given fp32 tensors (contiguous; e.g. the views of
    an nn.Linear's gradients in a TrainStep bucket) - no [Nc, K + 1] intermediate and no slicing copies (stin_gemm_tn_wb_*)."""
    lib = _lib.load()
    G, ldg = _mat(G)
    X, ldx = _mat(X)
    _same(G, X)
    M, Nc = G.shape
    K = X.shape[1]
    assert X.shape[0] == M and tuple(dW.shape) == (Nc, K) and db.numel() == Nc and dW.is_contiguous() and db.is_contiguous()
    ws_bytes = lib.stin_gemm_tn_workspace_bytes(M, Nc, K, 1)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=G.device)
    if G.dtype == torch.bfloat16:
        _call('stin_gemm_tn_wb_bf16', _ptr(G), ldg, _ptr(X), ldx, M, Nc, K, None, 0, _ptr(dW), K, _ptr(db), _ptr(ws), ws_bytes,
              _stream(G), tag=(M, Nc, K))
    else:
        _call('stin_gemm_tn_wb_f32', _ptr(G), ldg, _ptr(X), ldx, M, Nc, K, None, 0, _ptr(dW), K, _ptr(db), int(precision), _ptr(ws),
              ws_bytes, _stream(G), tag=(M, Nc, K))


class LinearFn(torch.autograd.Function):
    """y = x W^T + b on the MFMA kernels (the tail Linears and the generic filter paths).  wT: the weight already
    transposed ([K, Nc] fp32, written by the network's PackSet beside the block operands) - without it the backward
    transposes the weight itself.  wT points into a buffer that every PackSet.run() rewrites and is NOT under autograd's version
    tracking, so wT_guard = (pack set, its run count at this forward) is compared again in backward: after another pack run
    (a second forward following an in-place weight change) the backward transposes the SAVED, version-checked weight instead.
    Gradients of weight / bias go straight into an accepting TrainStep bucket."""

    @staticmethod
    def forward(ctx, x, weight, bias, out_fp32=False, precision=None, wT=None, wT_guard=None):
        x, _ = _mat(x)
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        ctx.params = (weight, bias)
        ctx.wT = wT
        ctx.wT_guard = wT_guard
        return gemm_nt(x, weight, bias, precision=PREC_FWD if precision is None else precision,
                       out_dtype=torch.float32 if out_fp32 else None)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        if g.dtype != x.dtype:                     # fp32 network output on bf16-storage activations
            g = g.to(x.dtype)
        g, _ = _mat(g)
        fresh = ctx.wT is not None and (ctx.wT_guard is None or getattr(ctx.wT_guard[0], 'runs', None) == ctx.wT_guard[1])
        wT = ctx.wT if fresh else weight.t().contiguous()
        dx = gemm_nt(g, wT, precision=PREC_BWD) if ctx.needs_input_grad[0] else None
        if not ctx.has_bias:
            return dx, gemm_tn(g, x, ones_column=False, precision=PREC_BWD), None, None, None, None, None
        direct = _direct_grad_views(ctx.params) if g.is_cuda else None
        if direct is not None:                     # written where the optimizer reads them: nothing for autograd to copy
            gemm_tn_wb(g, x, direct[0], direct[1], precision=PREC_BWD)
            return dx, None, None, None, None, None, None
        if g.is_cuda:
            dW = torch.empty(weight.shape, dtype=torch.float32, device=g.device)
            db = torch.empty(weight.shape[0], dtype=torch.float32, device=g.device)
            gemm_tn_wb(g, x, dW, db, precision=PREC_BWD)
            return dx, dW, db, None, None, None, None
        dwb = gemm_tn(g, x, ones_column=True, precision=PREC_BWD)
        return dx, dwb[:, :-1].contiguous(), dwb[:, -1].contiguous(), None, None, None, None


def linear_tanh_eligible(x, weight, bias):
    """The one-launch last layer (stin_linear_tanh_*): at most 4 output channels from K <= 256 channels, 16-byte rows."""
    Nc, K = weight.shape
    return (USE_TAIL_KERNEL and x.is_cuda and x.dim() == 2 and x.dtype in (torch.float32, torch.bfloat16) and x.stride(1) == 1 and
            x.stride(0) % 4 == 0 and K % 4 == 0 and K <= 256 and 1 <= Nc <= 4 and Nc * K + Nc <= 1024 and
            weight.dtype == torch.float32 and weight.is_contiguous() and (bias is None or bias.is_contiguous()) and
            x.data_ptr() % (16 if x.dtype == torch.float32 else 8) == 0)


USE_TAIL_KERNEL = True


class LinearTanhFn(torch.autograd.Function):
    """tanh(x W^T + b) -> fp32 [N, Nc], the network's last layer (reference models/surfacetextureinpaintingnet.py:470-471), one
    launch per direction (csrc/stin_tail.hip).  Gradients of W / b go straight into an accepting TrainStep bucket."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        N, K = x.shape
        Nc = weight.shape[0]
        y = torch.empty(N, Nc, dtype=torch.float32, device=x.device)
        sfx = '_bf16' if x.dtype == torch.bfloat16 else '_f32'
        _call('stin_linear_tanh_fwd' + sfx, _ptr(x), x.stride(0), _ptr(weight), _ptr(bias), N, K, Nc, _ptr(y), _stream(x), tag=(N, Nc, K))
        ctx.save_for_backward(x, weight, y)
        ctx.params = (weight, bias)
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, y = ctx.saved_tensors
        lib = _lib.load()
        N, K = x.shape
        Nc = weight.shape[0]
        g = g.contiguous()
        if g.dtype != torch.float32:
            g = g.float()
        dev = x.device
        dx = torch.empty(N, K, dtype=x.dtype, device=dev) if ctx.needs_input_grad[0] else None
        direct = _direct_grad_views(ctx.params)
        if direct is not None:
            dW, db = direct
        else:
            dW = torch.empty(Nc, K, dtype=torch.float32, device=dev)
            db = torch.empty(Nc, dtype=torch.float32, device=dev) if ctx.params[1] is not None else None
        ws_bytes = lib.stin_linear_tanh_bwd_workspace_bytes(N, K, Nc)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        sfx = '_bf16' if x.dtype == torch.bfloat16 else '_f32'
        _call('stin_linear_tanh_bwd' + sfx, _ptr(g), _ptr(y), _ptr(x), x.stride(0), _ptr(weight), N, K, Nc, _ptr(dx), K, _ptr(dW),
              _ptr(db), _ptr(ws), ws_bytes, _stream(x), tag=(N, Nc, K))
        if direct is not None:
            return dx, None, None
        return dx, dW, db


def linear_tanh(x, weight, bias=None, precision=None):
    """tanh(x W^T + b) as fp32: the one-launch kernel where the shape allows it (exact fp32 products), else the GEMM
    (`precision` as in linear()) + torch.tanh."""
    if linear_tanh_eligible(x, weight, bias):
        return LinearTanhFn.apply(x, weight, bias)
    return torch.tanh(linear(x, weight, bias, out_fp32=True, precision=precision))


def linear(x, weight, bias=None, out_fp32=False, precision=None, wT=None, wT_guard=None):
    """x W^T + b.  out_fp32: fp32 result from bf16-storage activations (the network's final output).
    precision: forward matrix-core path (None = PREC_FWD); see forward_precision().  wT / wT_guard: see LinearFn."""
    return LinearFn.apply(x, weight, bias, out_fp32, precision, wT, wT_guard)


def forward_precision(unbounded_input):
    """Forward GEMM path for a layer.  fp16x3 (the default PREC_FWD) carries fp32-grade products for operands inside
    fp16's range (|activation| < 8188, |weight| < 1023; out-of-range operands give inf/NaN, never a silently wrong
    value) - true for everything downstream of an instance / batch / graph norm.  A layer fed by RAW data (the first
    block: un-normalised vertex features) or living in a network built without norms gets bf16x6 instead: bf16 pieces
    have fp32's exponent range, the 3-piece split is exact, and the first block's GEMMs are tiny (K = 12)."""
    if unbounded_input and PREC_FWD == GEMM_F16X3:
        return GEMM_BF16X6
    return PREC_FWD


# ----------------------------------------------------------------------- autograd ops
# ---- weight-gradient side stream of the whole-block backward ----------------------------------------------------------
USE_WGRAD_STREAM = os.environ.get('STIN_WGRAD_STREAM', '1') == '1'
WGRAD_DEFER_JOIN = True
# the overlap pays where kernels are too short to fill the GPU; a weight-gradient GEMM of N * Yw * Cp above this keeps the
# whole chip busy for hundreds of microseconds and only slows the critical-path kernels it runs beside (measured: 500 k
# vertices / 4 levels +4.7 %, every block <= 1.5e10; 1 M vertices / 3 levels -13 %, every block >= 2e10)
WGRAD_MAX_WORK = float(os.environ.get('STIN_WGRAD_MAX_WORK', 1.6e10))
# ... and below this a step is launch-bound on the host, where the second stream only adds host work (3 event records / waits
# per block): 40 k vertices 4.2-4.8 ms per step without vs 5.4-5.5 with (every block <= 1.6e9), 60 k equal, 100 k 6.09 without
# vs 5.60 with (bottleneck blocks 2.4e9), batch of 8 crops / 4 levels 9.8 vs 9.3
WGRAD_MIN_WORK = float(os.environ.get('STIN_WGRAD_MIN_WORK', 2.0e9))
_WGRAD_SIDE = {}


class _WgradSide:
    """Per device: the HIP stream the weight-gradient GEMMs of a block's backward (stin_net_bwd, use_side) run on and a ring
    of event triples that order it against the compute stream (a fresh triple per block, so no event is re-recorded while
    a wait on its previous record may still be queued)."""
    RING = 64

    def __init__(self, dev):
        self.stream = torch.cuda.Stream(device=dev)
        self.ring = [[torch.cuda.Event() for _ in range(3)] for _ in range(self.RING)]
        for tri in self.ring:
            for e in tri:
                e.record(self.stream)               # forces creation of the hipEvent_t handles
        self.at = 0
        self.last_done = self.ring[0][2]
        self.hold = []                              # tensors the side stream may still be reading (dropped at the join)

    def next_events(self, track=True):
        """track=False: an event triple for a block that stays on the compute stream (its ev_done is recorded there): it must not
        become `last_done`, the event the deferred join of the SIDE stream waits for."""
        self.at = (self.at + 1) % self.RING
        tri = self.ring[self.at]
        if track:
            self.last_done = tri[2]
        return tri


def _wgrad_side(dev):
    side = _WGRAD_SIDE.get(dev.index)
    if side is None:
        side = _WGRAD_SIDE[dev.index] = _WgradSide(dev)
    return side


USE_DIRECT_GRADS = True


def _direct_grad_views(params, dry_run=False):
    """(dW1, db1, dW2, db2, dWs, dbs) as the parameters' views in an accepting train_step.FlatGradBucket, or None.
    The backward then OVERWRITES those views (one backward per step, every weight used by one block) and returns no
    gradient to autograd for them: no per-parameter accumulate node, no copy into the bucket afterwards, and nothing of
    autograd can read a gradient before the end-of-backward join of the weight-gradient stream."""
    if not USE_DIRECT_GRADS:
        return None
    bucket, out = None, []
    for p in params:
        if p is None:
            out.append(None)
            continue
        slot = getattr(p, '_stin_slot', None)
        if slot is None or not slot[0].accepting or (bucket is not None and slot[0] is not bucket) or slot[0].written[slot[1]]:
            return None
        bucket = slot[0]
        out.append(bucket.views[slot[1]])
    if bucket is None:
        return None
    if dry_run:                  # eligibility probe only (a node that covers several blocks decides for ALL of them first)
        return out
    for p in params:
        if p is not None:
            bucket.written[p._stin_slot[1]] = True
    return out


def _plain_autograd_may_defer():
    """The deferred join is safe under plain autograd only while nothing outside this module can read a gradient before
    the end of the backward pass.  DistributedDataParallel registers its reducer as C++ post-hooks on the AccumulateGrad
    nodes - invisible to `p._backward_hooks` / `_post_accumulate_grad_hooks` - and copies each gradient into its bucket on
    the compute stream as soon as autograd produces it.  DDP cannot exist without an initialised multi-rank process
    group, so in that situation only the TrainStep bucket route (which bypasses autograd for these gradients) uses the
    side stream; every other caller keeps the block on one stream."""
    import torch.distributed as dist
    return not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)


def _join_deferrable(params, direct):
    """The join of the weight-gradient stream may wait until the end of the backward pass when nothing can read these
    parameters' gradients earlier: the TrainStep bucket route (`direct`), or plain single-process autograd with every
    parameter a leaf whose .grad is None (autograd then adopts the returned tensor without a kernel) and without hooks."""
    return WGRAD_DEFER_JOIN and (bool(direct) or (_plain_autograd_may_defer() and all(
        p is None or (p.is_leaf and p.grad is None and not p._backward_hooks and
                      not getattr(p, '_post_accumulate_grad_hooks', None)) for p in params)))


def wgrad_side_settle(dev):
    """Defensive join for callers that own the step (TrainStep.forward_backward's finally): when a backward pass raised
    after a block had put work on the weight-gradient stream, the autograd engine dropped the end-of-backward callbacks
    and the join never ran - wait for the side stream now and release what it was reading / writing.  A no-op after a
    normal pass (the join emptied `hold`)."""
    side = _WGRAD_SIDE.get(dev.index if dev.index is not None else torch.cuda.current_device())
    if side is not None and side.hold:
        torch.cuda.current_stream(dev).wait_event(side.last_done)
        side.hold.clear()


def _wgrad_deferred_join(dev, params, grads):
    """Queue the end-of-backward join for one block whose weight gradients were left on the side stream: the compute
    stream waits for ev_done (recorded after every side-stream kernel enqueued so far), and the gradient tensors must
    have been adopted by autograd as they are - a copy would have read them before this join.  One callback per block
    call and no state between passes, so an aborted backward cannot leave a join behind."""
    side = _wgrad_side(dev)
    adopted = [(p, t.data_ptr()) for p, t in zip(params, grads) if p is not None and t is not None]

    def join():
        torch.cuda.current_stream(dev).wait_event(side.last_done)    # the newest ev_done: after all side work so far
        side.hold.clear()                                             # freed from here on = ordered after the join
        for p, ptr in adopted:
            if p.grad is not None and p.grad.data_ptr() != ptr:
                raise RuntimeError('weight-gradient stream: autograd copied a gradient before the end-of-backward join; '
                                   'set STIN_WGRAD_STREAM=0 for this autograd configuration')

    torch.autograd.Variable._execution_engine.queue_callback(join)


def block_split_modes(prec_fwd, b16, Cout):
    """(fwd_split, bwd_split) of one fused block: the storage form of its forward / backward weight operands."""
    fsp = (prec_fwd | GEMM_W_FRAG) if (not b16 and prec_fwd in (GEMM_BF16X3, GEMM_F16X3) and WEIGHT_PRESPLIT) else 0
    bsp = (PREC_BWD | GEMM_W_FRAG) if (not b16 and PREC_BWD in (GEMM_BF16X3, GEMM_F16X3) and WEIGHT_PRESPLIT and Cout % 4 == 0) else 0
    return fsp, bsp


# Translation-invariant blocks in the COMPACT layout (round 6; include/stin_hip.h STIN_TI_COMPACT): the reference's message is
# nn(x_j - x_i) (models/modules/edge_conv_translation_invariance.py:20-22), so W1 (x_j - x_i) + b1 = A_i + B_j with B = x W1^T and
# A_i = b1 - B_i: only B is a GEMM output (Yw = H (+ Cout) instead of 2 H (+ Cout)), the edge stage forms A_i per row - what the
# [-W1 ; W1] product wrote up to one ulp of its accumulator - and the backward pass carries D = dB - dA in H columns.  Half the first Linear's GEMM work in
# every direction.  fp32 storage with a saved-mask hidden width; STIN_TI_COMPACT=0 keeps both halves materialised (A/B switch).
TI_COMPACT = os.environ.get('STIN_TI_COMPACT', '1') != '0'
TI_MODE_COMPACT = _C['STIN_TI_COMPACT']


def trans_inv_mode(trans_inv, b16, H):
    """The `trans_inv` value the C entry points take: 0 = EdgeConv, 1 = translation-invariant (A and B materialised), 2 = compact."""
    if not trans_inv:
        return 0
    return TI_MODE_COMPACT if (TI_COMPACT and not b16 and USE_EDGE_MASK and edge_mask_supported(H)) else 1


def block_yw(H, Cout, has_shortcut, ti_mode):
    """Width of Y / dY / the packed first-Linear operand (csrc/stin_common.h: stin_yw)."""
    return (H if ti_mode == TI_MODE_COMPACT else 2 * H) + (Cout if has_shortcut else 0)


def _pad_rows(x, pad):
    """x [N, Cin] with its rows padded to a multiple of `pad` channels (the inner dimension of the 16-byte GEMM paths: the
    10-channel network input -> 12; bf16: 16) in one launch (F.pad: fill + copy), or x itself."""
    N, Cin = x.shape
    Cp = (Cin + pad - 1) // pad * pad
    if Cp == Cin:
        return x
    xp = torch.empty(N, Cp, dtype=x.dtype, device=x.device)
    _call('stin_pad_rows' + _sfx(x), _ptr(x), x.stride(0), N, Cin, Cp, _ptr(xp), _stream(x))
    return xp


def _fresh_grads(params, dev):
    """Fresh fp32 gradient tensors [dW1, db1, dW2, db2, dWs, dbs] of one block's params (W1, b1, W2, b2, Ws, bs; None stays None)."""
    return [None if p is None else torch.empty(p.shape, dtype=torch.float32, device=dev) for p in params]


# Everything one fused block's parameter shapes, filter kind, input range and storage type decide, derived in block_shape() and
# nowhere else: PackSet, EdgeConvBlockFn, net_eligible, usable_prepack and the NetFn planner read it.  Cp: Cin padded to the inner
# dimension of the 16-byte GEMM paths (_pad_rows); ti: trans_inv_mode(); Yw: block_yw(); prec_fwd: forward_precision(); fwd_split,
# bwd_split: block_split_modes().
BlockShape = collections.namedtuple('BlockShape', 'Cin Cp H Cout has_shortcut ti Yw prec_fwd fwd_split bwd_split')


def block_shape(w1_shape, w2_shape, has_shortcut, trans_inv, unbounded_input, b16, width=None):
    """The BlockShape of a block with first / second Linear weights of these shapes.  Cin comes from W1; `width`, the width of
    the rows the caller is about to feed the block, must agree with it."""
    H, Cout = w1_shape[0], w2_shape[0]
    Cin = w1_shape[1] if trans_inv else w1_shape[1] // 2
    assert width is None or width == Cin, 'block input has %s channels, its first Linear takes %d' % (width, Cin)
    pad = 8 if b16 else 4
    ti = trans_inv_mode(trans_inv, b16, H)
    prec = forward_precision(unbounded_input)
    return BlockShape(Cin, (Cin + pad - 1) // pad * pad, H, Cout, bool(has_shortcut), ti, block_yw(H, Cout, has_shortcut, ti), prec,
                      *block_split_modes(prec, b16, Cout))


# One block's entry of PackSet.buffers: the block call's forward workspace `ws`, the backward operands (wcatT | w2T in `wts`, and as
# ready-made views) and what they were packed for.
Prepack = collections.namedtuple('Prepack', 'ws wts fwd_split bwd_split wcatT w2T b16')


BLOCK_PACKED = _C['STIN_BLOCK_PACKED']
_PACK_JOB = _lib.STRUCTS['stin_pack_job_t']
USE_PACK_MANY = True


class PackSet:
    """The weight packs of ALL fused blocks of a network in one launch per step (stin_edgeconv_pack_many_f32) instead of
    one tiny launch at the head of every block: persistent per-block operand buffers (the block call's forward workspace
    and wcatT | w2T), a job table in device memory written once.  specs: [(W1, b1, W2, b2, Ws, bs, trans_inv, unbounded_input,
    B)] in block order (GraphResnetBlock.pack_spec), fp32 storage.  Valid while the parameters stay where they are (`matches`)."""

    def __init__(self, specs, dev, b16=False, transposes=()):
        lib = _lib.load()
        self.key = self.key_of(specs) + (bool(b16),) + tuple((_ptr(W), tuple(W.shape)) for W in transposes)
        self.b16 = bool(b16)
        self.buffers = []                      # per block: a Prepack
        blob, self.max_elems = b'', 0
        for (W1, b1, W2, b2, Ws, bs, trans_inv, unbounded_input, B) in specs:
            # (fsp, bsp: what the block call is handed - bf16 rows: 0, 0)
            Cin, Cp, H, Cout, has_sc, ti, Yw, _, fsp, bsp = block_shape(W1.shape, W2.shape, Ws is not None, trans_inv, unbounded_input, b16)
            # what the pack writes: bf16 rows -> plain bf16 operands where every reduction length is a multiple of 8
            # (the rule of stin_net_fwd's block op), else the fp32 / split form of the fp32-storage path
            jf, jb = ((GEMM_W_BF16, GEMM_W_BF16) if (Cp % 8 == 0 and Cout % 8 == 0) else (0, 0)) if b16 else (fsp, bsp)
            ws = torch.empty(lib.stin_edgeconv_block_fwd_workspace_bytes(Cin, Cp, H, Cout, int(has_sc), B), dtype=torch.uint8, device=dev)
            wts = torch.empty(Yw * Cp + H * Cout, dtype=torch.float32, device=dev)
            off = [ctypes.c_size_t(0) for _ in range(3)]
            _lib.check(lib.stin_edgeconv_block_fwd_pack_offsets(Cp, H, Cout, int(has_sc), *[ctypes.byref(o) for o in off]),
                       'stin_edgeconv_block_fwd_pack_offsets')
            base = (ws.data_ptr() + 255) & ~255
            wcat, w2s, bcat = (base + o.value for o in off)
            W1c, W2c = W1.contiguous(), W2.contiguous()
            assert W1c.data_ptr() == W1.data_ptr() and W2c.data_ptr() == W2.data_ptr(), 'pack_many needs contiguous weights'
            blob += _PACK_JOB.pack(W1=_ptr(W1), b1=_ptr(b1), Ws=_ptr(Ws), bs=_ptr(bs), W2=_ptr(W2), wcat=wcat, bcat=bcat,
                                   wcatT=_ptr(wts), w2T=_ptr(wts) + 4 * Yw * Cp, w2s=w2s if jf else 0, Cin=Cin, Cp=Cp, H=H,
                                   Cout=Cout, has_shortcut=int(has_sc), trans_inv=ti, fwd_split=jf, bwd_split=jb)
            self.max_elems = max(self.max_elems, Yw * Cp + H * Cout)
            # (the two backward operands as ready-made views: no tensor views are created inside autograd.Function.forward)
            self.buffers.append(Prepack(ws, wts, fsp, bsp, wts[:Yw * Cp].view(Cp, Yw), wts[Yw * Cp:].view(H, Cout), bool(b16)))
        # plain transposes riding on the same launch (the tail Linear's backward operand W^T): a job whose first operand is
        # empty (Cin = Cp = 0) and whose "second Linear" is the weight - the pack writes w2T [K, Nc] = W^T in plain fp32
        self.transposed = []
        for W in transposes:
            Nc, K = W.shape
            assert W.is_contiguous() and W.dtype == torch.float32
            wT = torch.empty(K, Nc, dtype=torch.float32, device=dev)
            blob += _PACK_JOB.pack(W2=_ptr(W), w2T=_ptr(wT), H=K, Cout=Nc)
            self.max_elems = max(self.max_elems, K * Nc)
            self.transposed.append(wT)
        self.jobs = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
        self.n = len(specs) + len(transposes)

    @staticmethod
    def key_of(specs):
        return tuple((_ptr(W1), _ptr(b1), _ptr(W2), _ptr(Ws), _ptr(bs), tuple(W1.shape), tuple(W2.shape), bool(t), forward_precision(u),
                      int(B), PREC_BWD, WEIGHT_PRESPLIT, GEMM_W_FRAG, TI_COMPACT, USE_EDGE_MASK) for (W1, b1, W2, b2, Ws, bs, t, u, B) in specs)

    def matches(self, specs, b16=False, transposes=()):
        return self.key == self.key_of(specs) + (bool(b16),) + tuple((_ptr(W), tuple(W.shape)) for W in transposes)

    def run(self):
        self.runs = getattr(self, 'runs', 0) + 1       # what a consumer of `transposed` compares (LinearFn's wT guard)
        _call('stin_edgeconv_pack_many_f32', _ptr(self.jobs), self.n, self.max_elems, _stream(self.jobs))


class EdgeConvBlockFn(torch.autograd.Function):
    """One GraphResnetBlock with an EdgeConv(mean) filter and instance norm, fused at the
    autograd level (reference models/surfacetextureinpaintingnet.py:507-521), taking the
    reference-layout parameters directly:

        Y   = x Wcat^T + bcat          Wcat = [Wa-Wb ; Wb ; Ws]   (per-VERTEX MFMA GEMM)
        h   = mean_j ReLU(A_i + B_j)   A = Y[:, :H], B = Y[:, H:2H]   (HIP edge stage)
        agg = h W2^T + b2 [deg > 0]                                (per-VERTEX MFMA GEMM, masked bias)
        out = (Y[:, 2H:] or x) + ELU(InstanceNorm(agg))            (HIP epilogue)

    Saved for backward: per-vertex tensors plus the E*H-bit ReLU mask (recompute kernels when the hidden width does not
    support the mask).  This is the per-kernel path: one foreign call per launch.  GraphResnetBlock.forward takes it where
    net_eligible declines (STIN_BLOCK_CALL=0, STIN_EDGE_MASK=0, a hidden width without a saved mask, N <= 1, the bench's
    per-kernel brackets); everywhere else the block is a one-op NetFn, which enqueues the same kernels in the same order."""

    @staticmethod
    def forward(ctx, x, W1, b1, W2, b2, Ws, bs, edges, groups, trans_inv, eps=EPS, unbounded_input=False):
        x, _ = _mat(x)
        N = x.shape[0]
        dev = x.device
        b16 = x.dtype == torch.bfloat16
        # ti: 2 = compact: Y = [B | S], A_i = b1 - B_i formed by the edge stage.  fsp / bsp: the forward / backward weight operands,
        # pre-split once here into the two 16-bit pieces the split GEMMs use (instead of once per GEMM block); plain fp32 for the
        # other precisions and for bf16-storage activations
        Cin, Cp, H, Cout, has_shortcut, ti, Yw, prec_fwd, fsp, bsp = block_shape(W1.shape, W2.shape, Ws is not None, trans_inv,
                                                                                 unbounded_input, b16, x.shape[1])
        oS = Yw - (Cout if has_shortcut else 0)                   # column of the shortcut in Y / dY
        pad = 8 if b16 else 4
        xp = _pad_rows(x, pad)
        pack = torch.empty(Yw * Cp * 2 + 2 * H * Cout + Yw, dtype=torch.float32, device=dev)
        wcat = pack[:Yw * Cp].view(Yw, Cp)
        wcatT = pack[Yw * Cp:2 * Yw * Cp].view(Cp, Yw)
        w2T = pack[2 * Yw * Cp:2 * Yw * Cp + H * Cout].view(H, Cout)
        w2s = pack[2 * Yw * Cp + H * Cout:2 * Yw * Cp + 2 * H * Cout].view(Cout, H)
        bcat = pack[2 * Yw * Cp + 2 * H * Cout:]
        W1c, W2c = W1.contiguous(), W2.contiguous()
        _call('stin_edgeconv_pack_f32', _ptr(W1c), _ptr(b1), _ptr(Ws), _ptr(bs), _ptr(W2c), Cin, Cp, H, Cout,
              int(has_shortcut), ti, _ptr(wcat), _ptr(bcat), _ptr(wcatT), _ptr(w2T), _ptr(w2s) if fsp else None,
              fsp, bsp, _stream(x))
        pf = (prec_fwd | GEMM_W_PRESPLIT | GEMM_W_FRAG) if fsp else prec_fwd
        Y = gemm_nt(xp, wcat, bcat, precision=pf)
        hE = torch.empty(N, H + pad, dtype=x.dtype, device=dev)     # [h | (deg > 0) | pad]: rows stay 16-byte multiples
        # ReLU decisions as bits (E*H/8 bytes): backward then needs no recompute gathers
        use_mask = USE_EDGE_MASK and edge_mask_supported(H) and Y.stride(0) % 4 == 0
        if b16 and not use_mask:
            raise NotImplementedError('bf16 storage needs the saved ReLU mask: hidden width %d not in '
                                      '{128, 256, 512, 1024, 2048} (or STIN_EDGE_MASK=0)' % H)
        mask = torch.empty(max(edges.n_edges, 1) * (H // 32), dtype=torch.int32, device=dev) if use_mask else None
        if ti == TI_MODE_COMPACT:
            if not use_mask:
                raise RuntimeError('compact trans-inv layout needs the saved ReLU mask (16-byte aligned rows)')
            edge_relu_mean_fwd_ti(b1, Y[:, :H], edges.by_dst, hE, indicator=True, mask=mask)
        else:
            edge_relu_mean_fwd(Y[:, :H], Y[:, H:2 * H], edges.by_dst, hE, indicator=True, mask=mask)
        fused = None
        if fsp and groups.B == 1 and groups.gid is None and not groups.quirk and N > 1:
            fused = gemm_nt_colstats(hE[:, :H], w2s, b2, hE[:, H], pf, Cout)       # GEMM2 + column sums in one launch
        if fused is not None:
            agg = fused[0]
            mean, rstd = moments_final(fused[1], groups.inv_cnt, eps)
        else:
            agg = gemm_nt(hE[:, :H], w2s if fsp else W2c, b2, row_mask=hE[:, H], precision=pf)
            mean, rstd = instance_stats(agg, groups, eps)
        res = Y[:, oS:] if has_shortcut else x
        out = norm_act_res_fwd(agg, mean, rstd, groups, res=res, act=True)
        ctx.save_for_backward(xp, Y, hE, agg, mean, rstd, wcatT, w2T)
        ctx.mask = mask
        ctx.cin = Cin
        ctx.edges, ctx.groups, ctx.H, ctx.has_shortcut, ctx.trans_inv = edges, groups, H, has_shortcut, ti
        ctx.params = (W1, b1, W2, b2, Ws, bs)
        ctx.prec_bwd_nt = (PREC_BWD | GEMM_W_PRESPLIT | GEMM_W_FRAG) if bsp else PREC_BWD
        return out

    @staticmethod
    def backward(ctx, g):
        x, Y, hE, agg, mean, rstd, wcatT, w2T = ctx.saved_tensors          # x: the (possibly channel-padded) block input
        edges, groups, H = ctx.edges, ctx.groups, ctx.H
        Cin, Cp, Cout = ctx.cin, x.shape[1], agg.shape[1]
        g, ldg = _mat(g)
        dagg = instance_norm_act_bwd(agg, g, mean, rstd, groups, act=True)
        dw2b = gemm_tn(dagg, hE[:, :H], ones_column=True, row_weight=hE[:, H], precision=PREC_BWD)   # [Cout, H + 1] = dW2 | db2
        dhE = gemm_nt(dagg, w2T, precision=ctx.prec_bwd_nt)                                             # [N, H] = dagg W2
        dY = torch.empty_like(Y)
        compact = ctx.trans_inv == TI_MODE_COMPACT
        oS = Y.shape[1] - (Cout if ctx.has_shortcut else 0)
        db1_ti = None
        if compact:                                     # D = dB - dA in one row of H columns (+ the column sums of dA = db1)
            db1_ti = edge_relu_mean_bwd_mask_ti(dhE, ctx.mask, edges, dY[:, :H])
            ctx.mask = None
        elif ctx.mask is not None:
            edge_relu_mean_bwd_mask(dhE, ctx.mask, edges, dY[:, :H], dY[:, H:2 * H])
            ctx.mask = None
        else:
            A, B = Y[:, :H], Y[:, H:2 * H]
            edge_relu_mean_bwd_dst(A, B, dhE, edges.by_dst, dY[:, :H])
            edge_relu_mean_bwd_src(A, B, dhE, edges.inv_deg, edges.by_src, dY[:, H:2 * H])
        if ctx.has_shortcut:
            dY[:, oS:].copy_(g)                     # (the whole-block C call lets this ride on the edge launch)
        dwb = gemm_tn(dY, x, ones_column=True, precision=PREC_BWD)           # [Yw, Cp + 1]: packed weight grad (Cin columns used) | bias grad in column Cp
        # dx = dY Wcat (+ g: the identity-residual path, added in the GEMM epilogue); skipped when the block input
        # needs no gradient (the network input of the first block)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = gemm_nt(dY, wcatT, precision=ctx.prec_bwd_nt, residual=None if ctx.has_shortcut else g)
            if Cp != Cin:
                dx = dx[:, :Cin]
        dW1, db1, dW2, db2, dWs, dbs = _fresh_grads(ctx.params, x.device)
        _call('stin_edgeconv_unpack_grads_f32', _ptr(dwb), _ptr(dw2b), Cin, Cp, H, Cout, int(ctx.has_shortcut),
              int(ctx.trans_inv), _ptr(dW1), _ptr(db1), _ptr(dWs), _ptr(dbs), _ptr(dW2), _ptr(db2), _stream(x))
        if compact and db1 is not None:
            db1 = db1_ti                            # (the packed product's ones column holds sum_i D_i ~ 0, not db1)
        return dx, dW1, db1, dW2, db2, dWs, dbs, None, None, None, None, None


# ---- the graph part of the network in ONE autograd node ----------------------------------------------------------------------
USE_NET_CALL = os.environ.get('STIN_NET_CALL', '1') != '0'     # the WHOLE graph part as one node (the model's forward() asks)
USE_CHAIN = True        # ... else the bottleneck blocks as one node (tests flip the attribute to get the per-block nodes)
# A decoder block's first product on the COARSE rows in front of its unpool step (stin_net_op_t::y_from_src): x_up[v] = x_c[trace[v]]
# makes every row of Y = x_up Wcat^T + bcat a copy of a row of Yc = x_c Wcat^T + bcat, so the product, Y and the reads of x_up shrink
# by the unpooling ratio (~3.3) and the edge stage / the residual read Yc through the trace - same bits (a row of an NT product
# depends on no other row).  STIN_UNPOOL_COMMUTE=0: the product over the unpooled rows, as before (A/B switch).
USE_UNPOOL_COMMUTE = os.environ.get('STIN_UNPOOL_COMMUTE', '1') != '0'
# ... and its backward without the unpooled rows (stin_net_op_t::x_from_src): their one reader, the packed weight-gradient product,
# reads x_c through the trace (stin_edgeconv_wgrad_map), so a TRAINING forward launches no gather either and the arena does not hold
# x_up.  Only where stin_edgeconv_wgrad_map_supported says so; other shapes keep the gather.  Off with STIN_UNPOOL_COMMUTE=0.
USE_WGRAD_MAP = True
# The op behind a shortcut block writes its input gradient - that block's g - straight into the shortcut columns of the block's
# dY = [dA | dB | g] (stin_net_op_t::g_in_dy): no copy of g.  fp32 rows.
USE_G_IN_DY = True
_NET_OP = _lib.STRUCTS['stin_net_op_t']
OP_BLOCK, OP_POOL_MAX, OP_UNPOOL = _C['STIN_OP_BLOCK'], _C['STIN_OP_POOL_MAX'], _C['STIN_OP_UNPOOL']


def _align256(n):
    return (n + 255) & ~255


def _block_shape_of(blk, params, b16, width=None):
    """BlockShape of a fused GraphResnetBlock with the parameters `params` (blk.fused_params()), fed rows of `width` channels."""
    return block_shape(params[0].shape, params[2].shape, params[4] is not None, blk.first_filter.trans_inv, blk.unbounded_input,
                       b16, width)


def usable_prepack(blk, b16, shape):
    """blk._prepacked - the block's operand buffers in the network's PackSet - when it was packed for this storage type and
    the split modes the block runs with now (`shape`), else None: the node then packs for itself."""
    pp = blk._prepacked
    return pp if (pp is not None and pp.b16 == b16 and pp.fwd_split == shape.fwd_split and pp.bwd_split == shape.bwd_split) else None


def net_eligible(steps, x):
    """steps = [('block', GraphResnetBlock, EdgeSet, NormGroups) | ('pool', PoolMap) | ('unpool', PoolMap)] can run as one
    NetFn: fused EdgeConv + instance-norm blocks on the whole-block path (saved ReLU mask available), max pooling, fp32 or
    bf16 storage; operands of every block packed by the network's PackSet or of none.  One block alone is a valid list."""
    if not (USE_BLOCK_CALL and USE_EDGE_MASK and not KernelTimer.per_kernel_path() and x.is_cuda and x.dim() == 2):
        return False
    if x.dtype not in (torch.float32, torch.bfloat16) or x.shape[0] <= 1:
        return False
    b16 = x.dtype == torch.bfloat16
    packed = []
    for st in steps:
        if st[0] != 'block':
            continue
        shape = _block_shape_of(st[1], st[1].fused_params(), b16)
        if not edge_mask_supported(shape.H) or st[2].n <= 1:
            return False
        packed.append(usable_prepack(st[1], b16, shape) is not None)
    return bool(packed) and any(packed) == all(packed)


# ---- the plan of a NetFn (plan_net): what the op table and the arena look like, from shapes and integer attributes alone - no data
# pointer is read, so it runs without a GPU (tests/test_net_plan.py).
class Slot:
    """`nbytes` of the arena; `offset` is set when the layout is closed (Arena.close)."""
    __slots__ = ('kind', 'nbytes', 'at', 'offset')

    def __init__(self, kind, nbytes, at):
        self.kind, self.nbytes, self.at, self.offset = kind, nbytes, at, None


# A training forward keeps everything for backward: all three kinds bump one offset.  (round 6) A forward nobody differentiates
# (shared) keeps nothing, so every op's temporaries (Y, hE, agg, statistics, unpacked weights) restart in ONE region and the op
# outputs ping-pong between two regions of the largest output - [kept | out 0 | out 1 | temporaries]: the arena of an evaluation
# pass is the largest block's working set instead of the sum over blocks (200 704 vertices: 0.5 GB instead of 3 GB), and it
# stays cache-warm.
class Arena:
    """Byte layout of a NetFn's one allocation in 256-byte aligned slots: KEPT until backward, an op's temporaries, an op's output."""
    KEPT, TMP, OUT = range(3)

    def __init__(self, shared):
        self.shared, self.slots, self.nbytes = shared, [], None
        self.top = [0, 0]                       # where the next KEPT / TMP slot starts inside its region
        self.tmp_max = self.out_max = self.n_out = 0

    def next_op(self):
        self.top[Arena.TMP] = 0

    def take(self, nbytes, kind=KEPT):
        kind = kind if self.shared else Arena.KEPT
        if kind == Arena.OUT:
            slot = Slot(kind, nbytes, self.n_out & 1)           # which of the two output regions
            self.n_out += 1
            self.out_max = max(self.out_max, _align256(nbytes))
        else:
            slot = Slot(kind, nbytes, self.top[kind])
            self.top[kind] = _align256(self.top[kind] + nbytes)
            self.tmp_max = max(self.tmp_max, self.top[Arena.TMP])
        self.slots.append(slot)
        return slot

    def close(self):
        """Resolve every slot's offset; `nbytes` is the arena's size."""
        kept = self.top[Arena.KEPT]
        for s in self.slots:
            s.offset = {Arena.KEPT: s.at, Arena.OUT: kept + s.at * self.out_max, Arena.TMP: kept + 2 * self.out_max + s.at}[s.kind]
        self.nbytes = kept + 2 * self.out_max + self.tmp_max


# The descriptors of a plan's ops.  `rel`: the fields of stin_net_op_t that point into the arena, name -> (Slot, byte offset inside
# it); a Slot of None is a buffer the op does not have (no mask in a plan without backward, no x behind an unpool step that wrote
# no rows).  `out`: the Slot of the output rows; None for the last op, which writes the node's output tensor.
@dataclasses.dataclass(eq=False)
class BlockOp:
    """One fused block of a plan."""
    params: tuple           # (W1, b1, W2, b2, Ws, bs)
    edges: object
    groups: object
    shape: BlockShape
    N: int
    B: int
    eps: float
    pp: object              # usable_prepack()
    fwd_ws_bytes: int
    bwd_ws_bytes: int       # (0 in a plan without backward)
    kind: int = OP_BLOCK
    src: object = None      # the unpool op in front when the first product runs on ITS input rows (y_from_src): Y holds those rows only
    x_from_src: bool = False        # ... and that op wrote no rows: backward reads x through its trace
    rel: dict = None
    out: Slot = None


@dataclasses.dataclass(eq=False)
class PoolOp:
    """One max-pool (OP_POOL_MAX) or unpool (OP_UNPOOL) step of a plan, C channels wide."""
    kind: int
    pool: object
    n_in: int
    n_out: int
    C: int
    writes_no_rows: bool = False    # an unpool step whose block reads the coarse rows through the trace: no gather, no output
    rel: dict = None
    out: Slot = None


NetPlan = collections.namedtuple('NetPlan', 'ops arena n_rows width')        # (n_rows, width: shape of the node's output)


def _commutes(shape, b16):
    """A block behind an unpool step takes its first product from that step's input rows (USE_UNPOOL_COMMUTE): fp32 storage, a shortcut
    (the residual comes out of Y), A materialised in Y, no channel padding in between.  Every level takes it; a level whose mapped edge and
    norm launches lose more than its product saves is to be excluded HERE (profiles/r14_unpool_commute.md: the per-level figures are open)."""
    return (USE_UNPOOL_COMMUTE and not b16 and shape.has_shortcut and shape.ti != TI_MODE_COMPACT and shape.Cin % 4 == 0
            and shape.Cout % 4 == 0)


def plan_net(steps, params, n_rows, width, b16, need_grad):
    """The NetPlan of `steps` (see net_eligible) with the flat parameters `params` (see run_net) over [n_rows, width] input rows, in
    three passes: shapes, decisions, arena layout."""
    lib = _lib.load()
    es, pad = (2, 8) if b16 else (4, 4)
    # ---- pass 1, shapes: (rows, width) through the steps -> one BlockOp / PoolOp each
    ops = []
    for stp in steps:
        if stp[0] == 'block':
            _, blk, edges, groups = stp
            p, params = tuple(params[:6]), params[6:]
            sh = _block_shape_of(blk, p, b16, width)
            ops.append(BlockOp(p, edges, groups, sh, n_rows, groups.B, float(blk.first_norm.eps), usable_prepack(blk, b16, sh),
                               lib.stin_edgeconv_block_fwd_workspace_bytes(sh.Cin, sh.Cp, sh.H, sh.Cout, int(sh.has_shortcut), groups.B),
                               lib.stin_edgeconv_block_bwd_workspace_bytes(n_rows, sh.Cp, sh.H, sh.Cout, int(sh.has_shortcut), groups.B,
                                                                           int(b16)) if need_grad else 0))
            width = sh.Cout
        else:
            pool = stp[1]
            n_in, n_rows = (pool.n_fine, pool.n_coarse) if stp[0] == 'pool' else (pool.n_coarse, pool.n_fine)
            ops.append(PoolOp(OP_POOL_MAX if stp[0] == 'pool' else OP_UNPOOL, pool, n_in, n_rows, width))
    # ---- pass 2, decisions: for every block behind an unpool step, once: does its first product run on the coarse rows (src), and
    # does the unpool step then write rows at all
    for prev, op in zip(ops, ops[1:]):
        if op.kind == OP_BLOCK and prev.kind == OP_UNPOOL and _commutes(op.shape, b16):
            sh = op.shape
            op.src = prev
            # a no-grad forward keeps no x for backward: the unpool step writes no rows at all - nor does it in a training forward
            # when the block's backward reads x through the trace (USE_WGRAD_MAP): the shapes whose packed weight-gradient product
            # runs on the producer / consumer kernel
            prev.writes_no_rows = not need_grad or bool(USE_WGRAD_MAP and lib.stin_edgeconv_wgrad_map_supported(
                int(op.N), int(sh.Cin), int(sh.H), int(sh.Cout), 1, int(PREC_BWD)))
            op.x_from_src = need_grad and prev.writes_no_rows
    # ---- pass 3, layout: the arena slots, in the order  block: Y, hE, mask, agg, stats, [unpacked weights, forward workspace], out;
    # pool: arg, out;  unpool: out
    arena = Arena(shared=not need_grad)
    x, tmp = None, Arena.TMP
    for op in ops:
        arena.next_op()
        last = op is ops[-1]
        if op.kind == OP_BLOCK:
            sh, N = op.shape, op.N
            Y = arena.take((op.src.n_in if op.src else N) * sh.Yw * es, tmp)
            hE = arena.take(N * (sh.H + pad) * es, tmp)
            # (round 6) a forward nobody differentiates - torch.no_grad(), the reference's validation loop - keeps no ReLU mask
            mask = arena.take(max(op.edges.n_edges, 1) * (sh.H // 32) * 4) if need_grad else None
            agg = arena.take(N * sh.Cout * es, tmp)
            stats = arena.take(2 * op.B * sh.Cout * 4, tmp)
            op.rel = dict(x=(x, 0), Y=(Y, 0), hE=(hE, 0), mask=(mask, 0), agg=(agg, 0), mean=(stats, 0), rstd=(stats, op.B * sh.Cout * 4))
            if op.pp is None:
                W = arena.take((sh.Yw * sh.Cp + sh.H * sh.Cout) * 4, tmp)
                op.rel.update(wcatT=(W, 0), w2T=(W, sh.Yw * sh.Cp * 4), fwd_ws=(arena.take(op.fwd_ws_bytes, tmp), 0))
            elif op.pp.ws.numel() < op.fwd_ws_bytes:
                raise RuntimeError('NetFn: prepacked workspace too small for this batch (PackSet built for another batch size)')
            if not last:
                op.out = arena.take(N * sh.Cout * es, Arena.OUT)
        else:
            op.rel = dict(x=(x, 0), arg=(arena.take(op.n_out * op.C * 4, tmp) if op.kind == OP_POOL_MAX else None, 0))
            if not (last or op.writes_no_rows):
                op.out = arena.take(op.n_out * op.C * es, Arena.OUT)
        x = op.out
    arena.close()
    return NetPlan(ops, arena, n_rows, width)


def _static_fields(plan, ldx, pad):
    """Per op, the stin_net_op_t fields both directions share and that do not point into the arena; ldx: the input's row pitch."""
    out = []
    for op in plan.ops:
        if op.kind == OP_BLOCK:
            sh, g, cd, pp = op.shape, op.groups, op.edges.by_dst, op.pp
            W1, b1, W2, b2, Ws, bs = op.params
            packed = {} if pp is None else dict(wcatT=_ptr(pp.wcatT), w2T=_ptr(pp.w2T), fwd_ws=_ptr(pp.ws))
            out.append(dict(kind=OP_BLOCK, Cin=sh.Cin, Cp=sh.Cp, H=sh.H, Cout=sh.Cout, has_shortcut=int(sh.has_shortcut),
                            trans_inv=int(sh.ti), prec_fwd=int(sh.prec_fwd), bwd_split=sh.bwd_split, B=op.B, slice_quirk=int(g.quirk),
                            eps=op.eps, y_from_src=int(op.src is not None), x_from_src=int(op.x_from_src),
                            n_out=op.N, n_in=op.N, ldx=ldx, ldo=sh.Cout, ldy=sh.Yw, ldh=sh.H + pad, fwd_ws_bytes=op.fwd_ws_bytes,
                            fwd_split=sh.fwd_split | (BLOCK_PACKED if pp is not None else 0),
                            W1=_ptr(W1.contiguous()), b1=_ptr(b1), W2=_ptr(W2.contiguous()), b2=_ptr(b2), Ws=_ptr(Ws),
                            bs=_ptr(bs), rowptr_dst=_ptr(cd.rowptr), col_dst=_ptr(cd.col),
                            ptr_sum=_ptr(g.ptr_sum), gid=_ptr(g.gid), inv_cnt=_ptr(g.inv_cnt), **packed))
            ldx = sh.Cout
        else:
            ch, C = op.pool.children, op.C
            out.append(dict(kind=op.kind, Cin=C, Cp=C, Cout=C, n_out=op.n_out, n_in=op.n_in, ldx=ldx, ldo=C,
                            rowptr_dst=_ptr(ch.rowptr), col_dst=_ptr(ch.col), trace=_ptr(op.pool.trace)))
            ldx = C
    return out


# The arena fields are resolved on the arena of the saved tensors the DIRECTION is handed: under torch.utils.checkpoint(
# use_reentrant=False) backward gets the recomputed ones, not the forward call's.  (stin_net_bwd and the block backward read no
# forward-only field, so backward packs the forward's static fields again with its own on top.)
def _pack_table(plan, static, base, xp, own):
    """The op table of one direction: per op its static fields, its arena fields as addresses above `base` (the first op reads
    the padded input xp instead) and the direction's own fields, own(i, op)."""
    blob = []
    for i, (op, fields) in enumerate(zip(plan.ops, static)):
        ptrs = {k: 0 if s is None else base + s.offset + o for k, (s, o) in op.rel.items()}
        if i == 0:
            ptrs['x'] = _ptr(xp)
        blob.append(_NET_OP.pack(**fields, **ptrs, **own(i, op)))
    return ctypes.create_string_buffer(b''.join(blob), len(blob) * _NET_OP.size)


def _grad_targets(plan, blocks, xp, arena, g, need_dx):
    """Gradient tensors, scratch memory, the weight-gradient stream and the events of one backward pass over `plan`."""
    dev, dt, es = xp.device, xp.dtype, xp.element_size()
    # gradients: straight into an accepting TrainStep bucket (all blocks or none), else fresh tensors handed to autograd
    # (probe every block BEFORE any bucket bookkeeping changes: with a frozen or unslotted parameter in one block - a frozen
    # decoder, say - the whole node hands fresh tensors to autograd instead of leaving `written` half set and raising)
    direct = []
    if all(_direct_grad_views(d.params, dry_run=True) is not None for d in blocks):
        direct = [_direct_grad_views(d.params) for d in blocks]
    grads = None
    if len(direct) != len(blocks):
        direct = []
        grads = [t for d in blocks for t in _fresh_grads(d.params, dev)]
    # scratch: input gradients ping-pong between two buffers of the largest size; every block its own backward workspace
    # (the side stream reads it after this call has returned)
    dx_bytes, ws_off, off = 0, [], 0
    for i, d in enumerate(plan.ops):
        if d.kind == OP_BLOCK:
            if i > 0 or need_dx:
                dx_bytes = max(dx_bytes, d.N * d.shape.Cp * es)
            ws_off.append(off)
            off = _align256(off + d.bwd_ws_bytes)
        else:
            dx_bytes = max(dx_bytes, d.n_in * d.C * es)
    dx_bytes = _align256(dx_bytes)
    scratch = torch.empty(2 * dx_bytes + off, dtype=torch.uint8, device=dev)
    dx0 = None
    d0 = plan.ops[0]
    if need_dx:
        dx0 = torch.empty(d0.N if d0.kind == OP_BLOCK else d0.n_in, d0.shape.Cp if d0.kind == OP_BLOCK else d0.C,
                          dtype=dt, device=dev)
    all_params = [p for d in blocks for p in d.params]
    side_ok = USE_WGRAD_STREAM and _join_deferrable(all_params, direct)
    use = [side_ok and WGRAD_MIN_WORK <= float(d.N) * d.shape.Yw * d.shape.Cp <= WGRAD_MAX_WORK for d in blocks]
    side_stream, any_side = 0, any(use)
    evs = [(0, 0)] * len(blocks)
    # Overlapped gradient all-reduce (train_step.FlatGradBucket.enable_overlap, round 4): every block records its ev_done when
    # its parameter gradients are written - on the weight-gradient stream, or on the compute stream for a block that does
    # not use it - INSIDE the C call's kernel sequence, and the bucket hands each completed segment to RCCL behind exactly
    # those events: the reduction of the decoder's gradients runs while the encoder's backward kernels are still queued.
    bucket = None
    if direct:
        for p in all_params:
            if p is not None:
                bucket = p._stin_slot[0]
                break
    seg_events = bucket is not None and bucket.wants_block_events()
    done_ev = [None] * len(blocks)
    if any_side or seg_events:
        side = _wgrad_side(dev)
    if any_side:
        side.hold.append((scratch, xp, arena, g))
        side_stream = side.stream.cuda_stream
    if any_side or seg_events:
        for bi in reversed(range(len(blocks))):      # in BACKWARD order: side.last_done = the event recorded last
            if use[bi]:
                tri = side.next_events()
                evs[bi] = (tri[1].cuda_event, tri[2].cuda_event)
                done_ev[bi] = tri[2]
            elif seg_events:
                tri = side.next_events(track=False)
                evs[bi] = (0, tri[2].cuda_event)
                done_ev[bi] = tri[2]
        if grads is not None:
            for t in grads:
                if t is not None:
                    t.record_stream(side.stream)
    return direct, grads, scratch, dx_bytes, ws_off, dx0, all_params, use, side_stream, any_side, evs, bucket, done_ev


class NetFn(torch.autograd.Function):
    """A run of fused blocks and pool / unpool steps - the network's whole graph part, its bottleneck chain, or one block - as
    ONE autograd node and one C call per direction (stin_net_fwd / _bwd: loops over the per-op launch sequences, same kernels
    in the same order -> bit-identical to the per-kernel path).  All tensors backward needs live in one arena allocation, laid
    out by plan_net; the op table is packed on the host (480 bytes per op, _pack_table).
    args: x, meta = (steps, need_grad), then the flat parameters (W1, b1, W2, b2, Ws, bs) of every block in step order."""

    calls = 0                           # nodes created ...
    sizes = collections.Counter()       # ... and how many of them per number of ops (1 = a block on its own)
    commuted = 0                        # blocks whose first product ran on the coarse rows in front of their unpool step
    gathers_skipped = 0                 # ... and unpool ops that were given no output (no gather launch): those of no-grad forwards and,
                                        # in training, those whose block reads x through the trace in backward (USE_WGRAD_MAP)

    @staticmethod
    def forward(ctx, x, meta, *params):
        steps, need_grad = meta
        NetFn.calls += 1
        NetFn.sizes[len(steps)] += 1
        x, _ = _mat(x)
        b16 = x.dtype == torch.bfloat16
        sfx = '_bf16' if b16 else '_f32'
        pad = 8 if b16 else 4
        xp = _pad_rows(x, pad)
        plan = plan_net(steps, params, x.shape[0], x.shape[1], b16, need_grad)
        arena = torch.empty(plan.arena.nbytes, dtype=torch.uint8, device=x.device)
        out = torch.empty(plan.n_rows, plan.width, dtype=x.dtype, device=x.device)
        base, p_out = _ptr(arena), _ptr(out)
        assert base % 256 == 0
        static = _static_fields(plan, xp.stride(0), pad)

        def own(i, op):
            if op.kind != OP_BLOCK:
                NetFn.gathers_skipped += int(op.writes_no_rows)
                return dict(out=0 if op.writes_no_rows else p_out if op.out is None else base + op.out.offset)
            NetFn.commuted += int(op.src is not None)
            # (the mapped launch of a commuted block is bracketed under the plain kernel's name and tag: same rows, edges, width)
            ev0, ev1 = KernelTimer.edge_events('stin_edge_relu_mean_fwd' + sfx, (op.N, op.edges.n_edges, op.shape.H))
            return dict(ev_edge0=ev0, ev_edge1=ev1, out=p_out if op.out is None else base + op.out.offset)
        buf = _pack_table(plan, static, base, xp, own)
        _call('stin_net_fwd', int(b16), buf, len(plan.ops), _stream(x))
        if need_grad:
            ctx.save_for_backward(xp, arena)
            ctx.plan, ctx.static = plan, static
            ctx.cin0 = x.shape[1]
            ctx.params = params
        return out

    @staticmethod
    def backward(ctx, g):
        xp, arena = ctx.saved_tensors                    # (the ops' pointers go into the arena)
        plan, params = ctx.plan, ctx.params
        dev = xp.device
        b16 = xp.dtype == torch.bfloat16
        sfx = '_bf16' if b16 else '_f32'
        g, ldg = _mat(g)
        _same(xp, g)
        blocks = [d for d in plan.ops if d.kind == OP_BLOCK]
        direct, grads, scratch, dx_bytes, ws_off, dx0, all_params, use, side_stream, any_side, evs, bucket, done_ev = _grad_targets(
            plan, blocks, xp, arena, g, ctx.needs_input_grad[0])
        p_scr = _ptr(scratch)
        p_ws = p_scr + 2 * dx_bytes

        def own(i, d):
            p_dx = _ptr(dx0) if i == 0 else p_scr + (i & 1) * dx_bytes            # (dx0 is None, p_dx 0, when x needs no gradient)
            if d.kind != OP_BLOCK:
                return dict(lddx=d.C, dx=p_dx)
            bi, sh = blocks.index(d), d.shape
            e, gr, cs = d.edges, d.groups, d.edges.by_src
            gs = direct[bi] if direct else grads[6 * bi:6 * bi + 6]
            ev0, ev1 = KernelTimer.edge_events('stin_edge_relu_mean_bwd_mask' + ('_ti' if sh.ti == TI_MODE_COMPACT else '') + sfx,
                                               (d.N, e.n_edges, sh.H))
            return dict(use_side=int(use[bi]), lddx=sh.Cp, g_in_dy=int(USE_G_IN_DY and not b16 and sh.has_shortcut),
                        bwd_ws_bytes=d.bwd_ws_bytes, dx=p_dx,
                        rowptr_src=_ptr(cs.rowptr), col_src=_ptr(cs.col), xslot=_ptr(e.xslot), w_src=_ptr(e.w_src),
                        ptr_true=_ptr(gr.ptr_true), sid=_ptr(gr.sid if gr.quirk else None),
                        dW1=_ptr(gs[0]), db1=_ptr(gs[1]), dW2=_ptr(gs[2]), db2=_ptr(gs[3]), dWs=_ptr(gs[4]), dbs=_ptr(gs[5]),
                        bwd_ws=p_ws + ws_off[bi], ev_dy=evs[bi][0], ev_done=evs[bi][1], ev_edge0=ev0, ev_edge1=ev1)
        buf = _pack_table(plan, ctx.static, _ptr(arena), xp, own)
        _call('stin_net_bwd', int(b16), buf, len(plan.ops), _ptr(g), ldg, int(PREC_BWD), _stream(xp), side_stream)
        if any_side:
            _wgrad_deferred_join(dev, all_params if not direct else (), () if direct else grads)
        if dx0 is not None and dx0.shape[1] != ctx.cin0:
            dx0 = dx0[:, :ctx.cin0]
        if direct:
            # completed segments go to RCCL now, each behind its own blocks' events; one that also holds gradients of another node
            # waits behind the side stream's NEWEST event whenever any block of THIS backward pass has put weight-gradient work
            # there (`hold` is emptied by the end-of-backward join), not only when a block of this node did
            sd = _WGRAD_SIDE.get(dev.index if dev.index is not None else torch.cuda.current_device())
            bucket.blocks_done([([p._stin_slot[1] for p in d.params if p is not None], done_ev[bi]) for bi, d in enumerate(blocks)],
                                 sd.last_done if (sd is not None and sd.hold) else None)
            return (dx0, None) + (None,) * len(params)
        return (dx0, None) + tuple(grads)


def run_net(x, steps):
    """x through `steps` (see net_eligible) as one NetFn node."""
    params = [p for st in steps if st[0] == 'block' for p in st[1].fused_params()]
    # need_grad is decided HERE: inside an autograd.Function's forward the grad mode is always off
    need_grad = torch.is_grad_enabled() and (x.requires_grad or any(p is not None and p.requires_grad for p in params))
    return NetFn.apply(x, (steps, need_grad), *params)


class EdgeReluMeanFn(torch.autograd.Function):
    """h = mean_j ReLU(A_i + B_j) as a standalone differentiable op."""

    @staticmethod
    def forward(ctx, A, B, edges):
        A, _ = _mat(A)
        B, _ = _mat(B)
        out = torch.empty(A.shape[0], A.shape[1], dtype=torch.float32, device=A.device)
        edge_relu_mean_fwd(A, B, edges.by_dst, out)
        ctx.save_for_backward(A, B)
        ctx.edges = edges
        return out

    @staticmethod
    def backward(ctx, g):
        A, B = ctx.saved_tensors
        g, _ = _mat(g)
        dA = torch.empty_like(A)
        dB = torch.empty_like(B)
        edge_relu_mean_bwd_dst(A, B, g, ctx.edges.by_dst, dA)
        edge_relu_mean_bwd_src(A, B, g, ctx.edges.inv_deg, ctx.edges.by_src, dB)
        return dA, dB, None


def _cols_axpy_rowmask(dst, src, rowptr, c0, c1, alpha):
    """dst[:, c0:c1] += alpha * src[:, c0:c1] on the rows that have an in-edge, in place (stin_cols_axpy_rowmask_*)."""
    _same(dst, src)
    _call('stin_cols_axpy_rowmask' + _sfx(dst), _ptr(dst), dst.stride(0), _ptr(src), src.stride(0), _ptr(rowptr), dst.shape[0], int(c0),
          int(c1), float(alpha), _stream(dst))


class NeighborMeanFn(torch.autograd.Function):
    """agg_i = mean_{j in N(i)} x_j (SAGEConv aggregation; sum for mean=False).  sub_cols = (c0, c1): the translation-invariant
    message x_j[:, c0:c1] - x_i[:, c0:c1] on those columns (models/modules/sage_conv_filter.py:87-90), i.e.
    agg[:, c0:c1] -= x_i[:, c0:c1] on rows with an in-edge - one in-place HIP pass per direction."""

    @staticmethod
    def forward(ctx, x, edges, mean, sub_cols=None):
        ctx.edges, ctx.mean, ctx.sub_cols = edges, mean, sub_cols
        agg = segment_sum(x, edges.by_dst.rowptr, edges.by_dst.col, edges.n, mean=mean)
        if sub_cols is not None:
            xm = x if (x.dim() == 2 and x.stride(1) == 1) else x.contiguous()
            _cols_axpy_rowmask(agg, xm, edges.by_dst.rowptr, sub_cols[0], sub_cols[1], -1.0)
        return agg

    @staticmethod
    def backward(ctx, g):
        e = ctx.edges
        gs = g * e.inv_deg.view(-1, 1) if ctx.mean else g
        dx = segment_sum(gs, e.by_src.rowptr, e.by_src.col, e.n, mean=False)
        if ctx.sub_cols is not None:
            gm = g if (g.dim() == 2 and g.stride(1) == 1) else g.contiguous()
            _cols_axpy_rowmask(dx, gm, e.by_dst.rowptr, ctx.sub_cols[0], ctx.sub_cols[1], -1.0)
        return dx, None, None, None


class ScatterAddFn(torch.autograd.Function):
    """out[n] = sum_{e: index[e]=n} src[e]  (torch_scatter.scatter_sum with a prebuilt CSR)."""

    @staticmethod
    def forward(ctx, src, csr):
        ctx.csr = csr
        return segment_sum(src, csr.rowptr, csr.perm, csr.n_rows, mean=False)

    @staticmethod
    def backward(ctx, g):
        raise NotImplementedError('ScatterAddFn is forward-only (benchmark / metrics op)')


class PoolMaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pool):
        x, ldx = _mat(x)
        C = x.shape[1]
        out = torch.empty(pool.n_coarse, C, dtype=x.dtype, device=x.device)
        arg = torch.empty(pool.n_coarse, C, dtype=torch.int32, device=x.device)
        _call('stin_pool_max_fwd' + _sfx(x), _ptr(x), ldx, _ptr(pool.children.rowptr), _ptr(pool.children.col), pool.n_coarse, C,
              _ptr(out), C, _ptr(arg), _stream(x))
        ctx.save_for_backward(arg)
        ctx.pool = pool
        return out

    @staticmethod
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        pool = ctx.pool
        g, ldg = _mat(g)
        C = g.shape[1]
        gx = torch.empty(pool.n_fine, C, dtype=g.dtype, device=g.device)
        _call('stin_pool_max_bwd' + _sfx(g), _ptr(g), ldg, _ptr(arg), _ptr(pool.trace), pool.n_fine, C, _ptr(gx), C, _stream(g))
        return gx, None


class PoolMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pool):
        ctx.pool = pool
        return segment_sum(x, pool.children.rowptr, pool.children.col, pool.n_coarse, mean=True)

    @staticmethod
    def backward(ctx, g):
        return gather_rows(g, ctx.pool.trace, ctx.pool.inv_count), None


class UnpoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pool):
        ctx.pool = pool
        return gather_rows(x, pool.trace)

    @staticmethod
    def backward(ctx, g):
        p = ctx.pool
        return segment_sum(g, p.children.rowptr, p.children.col, p.n_coarse, mean=False), None


class PermuteRowsFn(torch.autograd.Function):
    """y = x[idx] for a PERMUTATION idx (inv = its inverse): the two gathers at the model's boundary when the plan has
    renumbered the vertices (plan.GraphPlan._ensure_order); backward = the gather with the inverse."""

    @staticmethod
    def forward(ctx, x, idx, inv):
        ctx.inv = inv
        return gather_rows(x, idx)

    @staticmethod
    def backward(ctx, g):
        return gather_rows(g.contiguous(), ctx.inv), None, None


class InstanceNormActResFn(torch.autograd.Function):
    """y = res + act(InstanceNorm(x)) (res optional, act = ELU or identity)."""

    @staticmethod
    def forward(ctx, x, res, groups, act, eps=EPS):
        x, _ = _mat(x)
        mean, rstd = instance_stats(x, groups, eps)
        y = norm_act_res_fwd(x, mean, rstd, groups, res=res, act=act)
        ctx.save_for_backward(x, mean, rstd)
        ctx.groups, ctx.act, ctx.has_res = groups, act, res is not None
        return y

    @staticmethod
    def backward(ctx, g):
        x, mean, rstd = ctx.saved_tensors
        dx = instance_norm_act_bwd(x, g, mean, rstd, ctx.groups, act=ctx.act)
        return dx, (g if ctx.has_res else None), None, None, None


class MaskedL1LossFn(torch.autograd.Function):
    """The inpainting trainer's loss in one kernel: pred = where(mask > 0, out, color);
    loss = mean(|pred - color| * 0.99^mask) (reference trainers/inpainting3d_trainer.py:127-137).  The gradient
    w.r.t. `out` is produced by the same pass and only scaled in backward."""

    @staticmethod
    def forward(ctx, out, color, mask, use_weight):
        lib = _lib.load()
        out, _ = _mat(out)
        color, _ = _mat(color)
        out, color = out.contiguous(), color.contiguous()
        N, C = out.shape
        m = mask.reshape(-1).contiguous()
        if m.dtype != torch.int64:
            m = m.long()
        loss = torch.empty((), dtype=torch.float32, device=out.device)
        grad = torch.empty_like(out)
        ws_bytes = lib.stin_masked_l1_workspace_bytes(N, C)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=out.device)
        _call('stin_masked_l1_loss_f32', _ptr(out), _ptr(color), _ptr(m), N, C, int(use_weight), _ptr(loss), _ptr(grad),
              _ptr(ws), ws_bytes, _stream(out))
        ctx.save_for_backward(grad)
        return loss

    # a caller that differentiates the loss itself with weight 1 can pass THIS tensor as the seed (`loss.backward(unit_seed(dev))`):
    # backward then returns the stored gradient as it is - no ones-fill for the seed and no [N, C] multiply (two launches)
    _UNIT = {}

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        u = MaskedL1LossFn._UNIT.get(g.device.index)
        if u is not None and g.data_ptr() == u.data_ptr():
            return grad, None, None, None
        return grad * g, None, None, None


def unit_seed(device):
    """The cached scalar 1.0 of `device` that MaskedL1LossFn.backward recognises (see there)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    u = MaskedL1LossFn._UNIT.get(idx)
    if u is None:
        u = MaskedL1LossFn._UNIT[idx] = torch.ones((), dtype=torch.float32, device=device)
    return u


def masked_l1_loss(out, color, mask, use_weight=True):
    return MaskedL1LossFn.apply(out, color, mask, use_weight)


def adam_step(p, g, m, v, vmax, lr, beta1, beta2, eps, weight_decay, step, amsgrad=True):
    """torch.optim.Adam(amsgrad) on flat fp32 buffers, one launch."""
    _call('stin_adam_f32', _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(vmax), p.numel(), float(lr), float(beta1), float(beta2),
          float(eps), float(weight_decay), int(step), int(amsgrad), _stream(p))


class SliceSumFn(torch.autograd.Function):
    """[N, C] -> [B, C] sums over contiguous row ranges (SingleBatchGraphNorm statistics)."""

    @staticmethod
    def forward(ctx, x, groups):
        ctx.groups = groups
        return colreduce(RED_SUM, x, groups, groups.ptr_sum)

    @staticmethod
    def backward(ctx, g):
        gr = ctx.groups
        if gr.sid is None:
            return g.expand(gr.n_rows, -1).contiguous(), None
        return g.index_select(0, gr.sid.long()), None
