// One GraphResnetBlock (EdgeConv(mean) -> instance norm -> ELU -> + residual) as a launch SEQUENCE, forward and backward, and
// the loops of stin_net_fwd / stin_net_bwd over a host op table of such blocks and the pool / unpool steps between them:
// enqueued from native code instead of ~9 / ~16 Python-level ctypes calls per block.  The arithmetic is exactly that of the
// individual entry points (this file only calls them, in the order of functional.EdgeConvBlockFn's per-kernel path); what it
// removes is host time - at 200k vertices the training step was launch-bound on the Python side in its backward half, at
// 20k vertices entirely.  A block's operands are the named fields of its op record (include/stin_hip.h: stin_net_op_t).
// Reference composition: models/surfacetextureinpaintingnet.py:507-521 (GraphResnetBlock.forward).
#include "stin_common.h"

namespace {

inline char* align256(void* p) { return reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(p) + 255) & ~(uintptr_t)255); }
inline char* carve(char*& p, size_t bytes) {
    char* r = p;
    p += stin_up256(bytes);
    return r;
}
#define STIN_TRY(expr)            \
    do {                          \
        const int rc_ = (expr);   \
        if (rc_ != STIN_OK) return rc_; \
    } while (0)

// element-size aware column offset
inline const void* col_off(const void* base, int64_t cols, int storage) {
    return static_cast<const char*>(base) + cols * (storage ? 2 : 4);
}

// Width of Y / dY / the packed first-Linear operand in the WIDE layout [A | B | shortcut].  Every workspace is sized and carved for it;
// the compact trans-inv layout (stin_common.h: stin_yw) uses H columns less of the same regions.
inline size_t yw_wide(int H, int Cout, int has_shortcut) { return 2 * (size_t)H + (has_shortcut ? Cout : 0); }

// The backward workspace of one block, as byte offsets from its 256-byte aligned base: what block_bwd carves, what
// stin_edgeconv_block_bwd_workspace_bytes adds up, and where stin_net_bwd finds the column-reduction scratch of the block that
// consumes a BwdLink's partials.
struct BwdLayout {
    size_t dagg, dhE, dY;      // [N, Cout], [N, H], [N, yw_wide] rows of the storage type
    size_t coef[5];            // k, m (+ T1, S0, U with the linspace-slice quirk): [B, Cout] floats each
    size_t red, red_bytes;     // column-reduction scratch
    size_t tn;                 // the slabs of both weight-gradient products: from here to the end of the workspace
};
inline BwdLayout bwd_layout(int64_t N, int H, int Cout, int has_shortcut, int B, int storage) {
    const size_t es = storage ? 2 : 4;
    BwdLayout L;
    size_t o = 0;
    auto take = [&o](size_t bytes) {
        const size_t r = o;
        o += stin_up256(bytes);
        return r;
    };
    L.dagg = take((size_t)N * Cout * es);
    L.dhE = take((size_t)N * H * es);
    L.dY = take((size_t)N * yw_wide(H, Cout, has_shortcut) * es);
    for (size_t& c : L.coef) c = take((size_t)B * Cout * 4);
    L.red_bytes = stin_colreduce_workspace_bytes(Cout, B);
    L.red = take(L.red_bytes);
    L.tn = o;
    return L;
}

// stin_colreduce_{f32,bf16} by storage type (identical parameter lists up to the row type)
inline int colreduce(int storage, int mode, const void* x, int64_t ldx, const void* gout, int64_t ldg, int64_t N, int C, const int32_t* ptr,
                     int B, const int32_t* gid, const int32_t* sid, const float* mean, const float* rstd, const float* coef, int post,
                     const float* inv_cnt, float eps, float* out0, float* out1, void* ws, size_t ws_bytes, stin_stream_t stream) {
    if (storage)
        return stin_colreduce_bf16(mode, static_cast<const stin_bf16_t*>(x), ldx, static_cast<const stin_bf16_t*>(gout), ldg, N, C, ptr, B,
                                   gid, sid, mean, rstd, coef, post, inv_cnt, eps, out0, out1, ws, ws_bytes, stream);
    return stin_colreduce_f32(mode, static_cast<const float*>(x), ldx, static_cast<const float*>(gout), ldg, N, C, ptr, B, gid, sid, mean,
                              rstd, coef, post, inv_cnt, eps, out0, out1, ws, ws_bytes, stream);
}

// Forward instance statistics of agg [N, Cout] -> J.mean, J.rstd: one moments pass, or with the linspace-slice quirk the sums over
// the slices and the centring through the graph id in two passes, as the reference computes them.
int fwd_stats(int storage, const stin_net_op_t& J, void* red_ws, size_t red_bytes, stin_stream_t stream) {
    if (!J.slice_quirk)
        return colreduce(storage, STIN_RED_MOMENTS, J.agg, J.Cout, nullptr, 0, J.n_out, J.Cout, J.ptr_sum, J.B, J.gid, nullptr, nullptr,
                         nullptr, nullptr, STIN_POST_NONE, J.inv_cnt, J.eps, J.mean, J.rstd, red_ws, red_bytes, stream);
    STIN_TRY(colreduce(storage, STIN_RED_SUM, J.agg, J.Cout, nullptr, 0, J.n_out, J.Cout, J.ptr_sum, J.B, J.gid, nullptr, nullptr, nullptr,
                       nullptr, STIN_POST_SCALE, J.inv_cnt, J.eps, J.mean, nullptr, red_ws, red_bytes, stream));
    return colreduce(storage, STIN_RED_CSQ, J.agg, J.Cout, nullptr, 0, J.n_out, J.Cout, J.ptr_sum, J.B, J.gid, nullptr, J.mean, nullptr,
                     nullptr, STIN_POST_RSTD, J.inv_cnt, J.eps, J.rstd, nullptr, red_ws, red_bytes, stream);
}

// Backward coefficients k, m of instance norm + ELU from the two column sums over (agg, g): one reduction finalised straight into
// them, or with the linspace-slice quirk k from the per-graph sums, then U = the sum over the slice of k xc, then m.
// coef = {k, m, T1, S0, U} (BwdLayout::coef).
int bwd_norm_coef(int storage, const stin_net_op_t& J, const void* g, int64_t ldg, float* const coef[5], void* red_ws, size_t red_bytes,
                  stin_stream_t stream) {
    float *kk = coef[0], *mm = coef[1], *t1 = coef[2], *s0 = coef[3], *uu = coef[4];
    if (!J.sid)
        return colreduce(storage, STIN_RED_DOT_ELU, J.agg, J.Cout, g, ldg, J.n_out, J.Cout, J.ptr_true, J.B, J.gid, nullptr, J.mean, J.rstd,
                         nullptr, STIN_POST_NORM_COEF, J.inv_cnt, 0.f, kk, mm, red_ws, red_bytes, stream);
    STIN_TRY(colreduce(storage, STIN_RED_DOT_ELU, J.agg, J.Cout, g, ldg, J.n_out, J.Cout, J.ptr_true, J.B, J.gid, nullptr, J.mean, J.rstd,
                       nullptr, STIN_POST_NONE, J.inv_cnt, 0.f, t1, s0, red_ws, red_bytes, stream));
    STIN_TRY(stin_norm_bwd_coef_f32(t1, s0, J.rstd, J.inv_cnt, J.B, J.Cout, kk, mm, stream));
    STIN_TRY(colreduce(storage, STIN_RED_COEF_XC, J.agg, J.Cout, nullptr, 0, J.n_out, J.Cout, J.ptr_true, J.B, J.gid, J.sid, J.mean, nullptr,
                       kk, STIN_POST_NONE, J.inv_cnt, 0.f, uu, nullptr, red_ws, red_bytes, stream));
    return stin_norm_bwd_coef_m_quirk_f32(s0, uu, J.rstd, J.inv_cnt, J.B, J.Cout, mm, stream);
}

// the optional HIP-event bracket of a block op around its edge-stage launch (stin_net_op_t::ev_edge0 / ev_edge1)
#define STIN_EDGE_BRACKET(CALL)                                                               \
    do {                                                                                      \
        if (J.ev_edge0) (void)hipEventRecord((hipEvent_t)J.ev_edge0, (hipStream_t)stream);    \
        STIN_TRY(CALL);                                                                       \
        if (J.ev_edge1) (void)hipEventRecord((hipEvent_t)J.ev_edge1, (hipStream_t)stream);    \
    } while (0)

}  // namespace

extern "C" size_t stin_edgeconv_block_fwd_workspace_bytes(int Cin, int Cp, int H, int Cout, int has_shortcut, int B) {
    if (Cp <= 0 || H <= 0 || Cout <= 0 || B <= 0) return 0;
    const size_t Yw = yw_wide(H, Cout, has_shortcut);
    (void)Cin;
    // wcat [Yw, Cp] + w2s [Cout, H] + bcat [Yw] (forward-only weight operands) + column-reduction workspace
    return stin_up256(Yw * Cp * 4) + stin_up256((size_t)Cout * H * 4) + stin_up256(Yw * 4) + stin_up256(stin_colreduce_workspace_bytes(Cout, B)) + 256;
}

extern "C" int stin_edgeconv_block_fwd_pack_offsets(int Cp, int H, int Cout, int has_shortcut, size_t* off_wcat, size_t* off_w2s,
                                                    size_t* off_bcat) {
    if (Cp <= 0 || H <= 0 || Cout <= 0 || !off_wcat || !off_w2s || !off_bcat) return STIN_E_SIZE;
    *off_wcat = 0;                                                  // the carve order of block_fwd
    *off_w2s = stin_up256(yw_wide(H, Cout, has_shortcut) * Cp * 4);
    *off_bcat = *off_w2s + stin_up256((size_t)Cout * H * 4);
    return STIN_OK;
}

extern "C" size_t stin_edgeconv_block_bwd_workspace_bytes(int64_t N, int Cp, int H, int Cout, int has_shortcut, int B,
                                                          int storage) {
    if (N < 0 || Cp <= 0 || H <= 0 || Cout <= 0 || B <= 0) return 0;
    // (sized for the wide layout; the compact trans-inv layout uses H of dY's 2 H columns and the slack pays for its dA column partials)
    return bwd_layout(N, H, Cout, has_shortcut, B, storage).tn + stin_up256(stin_edgeconv_wgrad_workspace_bytes(N, Cp, H, Cout, has_shortcut)) + 256;
}

// The unpool op `Un` in front of block `J` commutes with the block's first product (stin_net_op_t::y_from_src): the block reads
// exactly that op's output, fp32 rows, a shortcut (the residual comes out of Y, not out of x) and A materialised in Y.
static bool commutes(int storage, const stin_net_op_t& Un, const stin_net_op_t& J) {
    return storage == 0 && Un.kind == STIN_OP_UNPOOL && J.kind == STIN_OP_BLOCK && J.y_from_src != 0 && J.x == Un.out &&
           J.n_out == Un.n_out && J.Cin == Un.Cout && J.Cp == J.Cin && J.ldx == Un.ldo && J.has_shortcut != 0 &&
           J.trans_inv != STIN_TI_COMPACT && Un.trace != nullptr && Un.x != nullptr && Un.n_in > 0;
}

// Forward of one STIN_OP_BLOCK op (include/stin_hip.h: stin_net_op_t).  storage: 0 = fp32 rows, 1 = bf16 rows (x, Y, hE, agg, out).
// Un != NULL (y_from_src, checked by `commutes`): the unpool op in front - the first product runs on ITS input rows and the edge
// stage and the residual read Y through its trace.
static int block_fwd(int storage, const stin_net_op_t& J, stin_stream_t stream, const stin_net_op_t* Un = nullptr) {
    const int64_t N = J.n_out;
    const int Cp = J.Cp, H = J.H, Cout = J.Cout;
    STIN_REQUIRE(N >= 0 && J.Cin > 0 && Cp >= J.Cin && H > 0 && Cout > 0 && J.B > 0, STIN_E_SIZE);
    // mask == NULL (round 6): a forward nobody differentiates (torch.no_grad() / evaluation) - the ReLU mask is not stored
    STIN_REQUIRE((J.x || Un) && J.W1 && J.W2 && J.rowptr_dst && J.wcatT && J.w2T && J.Y && J.hE && J.agg && J.mean && J.rstd && J.out &&
                     J.fwd_ws,
                 STIN_E_NULL);
    STIN_REQUIRE(J.fwd_ws_bytes >= stin_edgeconv_block_fwd_workspace_bytes(J.Cin, Cp, H, Cout, J.has_shortcut, J.B), STIN_E_WORKSPACE);
    // trans_inv == STIN_TI_COMPACT (round 6, fp32 rows): Y = [B | S], the edge stage forms A_i = b1 - B_i (stin_common.h: stin_yw)
    const bool compact = J.trans_inv == STIN_TI_COMPACT;
    STIN_REQUIRE(!compact || storage == 0, STIN_E_UNSUPPORTED);
    const int Yw = stin_yw(H, Cout, J.has_shortcut, J.trans_inv);
    const size_t Yw_max = yw_wide(H, Cout, J.has_shortcut);        // the carve keeps the offsets of stin_edgeconv_block_fwd_pack_offsets
    STIN_REQUIRE(J.ldy >= Yw, STIN_E_SIZE);
    char* p = align256(J.fwd_ws);
    float* wcat = reinterpret_cast<float*>(carve(p, Yw_max * Cp * 4));
    float* w2s = reinterpret_cast<float*>(carve(p, (size_t)Cout * H * 4));
    float* bcat = reinterpret_cast<float*>(carve(p, Yw_max * 4));
    void* red_ws = p;
    const size_t red_bytes = stin_colreduce_workspace_bytes(Cout, J.B);

    // bf16 rows: the GEMM weight operands are written as bf16 once here (half the bytes every tile load, no conversion)
    // when every reduction length is a multiple of 8; fwd_split / bwd_split then carry STIN_GEMM_W_BF16
    const bool packed = (J.fwd_split & STIN_BLOCK_PACKED) != 0;    // the caller ran the pack (pack_many; bf16 rows: with the modes below)
    int fwd_split = J.fwd_split & ~STIN_BLOCK_PACKED, bwd_split = J.bwd_split;
    if (storage == 1) fwd_split = bwd_split = (Cp % 8 == 0 && Cout % 8 == 0) ? STIN_GEMM_W_BF16 : 0;
    if (!packed)
        STIN_TRY(stin_edgeconv_pack_f32(J.W1, J.b1, J.Ws, J.bs, J.W2, J.Cin, Cp, H, Cout, J.has_shortcut, J.trans_inv, wcat, bcat, J.wcatT,
                                        J.w2T, fwd_split ? w2s : nullptr, fwd_split, bwd_split, stream));
    const float* w2_op = fwd_split ? w2s : J.W2;
    const int wbf = (storage == 1 && fwd_split) ? STIN_GEMM_W_BF16 : 0;
    const int pf = fwd_split ? (J.prec_fwd | STIN_GEMM_W_PRESPLIT | (fwd_split & STIN_GEMM_W_FRAG)) : J.prec_fwd;
    const void* res = J.has_shortcut ? col_off(static_cast<const void*>(J.Y), (int64_t)(Yw - Cout), storage) : J.x;
    const int64_t ld_res = J.has_shortcut ? J.ldy : J.ldx;
    if (storage == 0) {
        float* Yf = static_cast<float*>(J.Y);
        float* hf = static_cast<float*>(J.hE);
        float* aggf = static_cast<float*>(J.agg);
        const int32_t* row_map = Un ? Un->trace : nullptr;
        if (Un)     // Yc = x_c Wcat^T + bcat over the coarse rows: Y[v] of the unpooled input is Yc[trace[v]], bit for bit
            STIN_TRY(stin_gemm_nt_f32(static_cast<const float*>(Un->x), Un->ldx, wcat, Cp, bcat, nullptr, 0, nullptr, 0, Un->n_in, Yw, Cp,
                                      Yf, J.ldy, pf, stream));
        else
            STIN_TRY(stin_gemm_nt_f32(static_cast<const float*>(J.x), J.ldx, wcat, Cp, bcat, nullptr, 0, nullptr, 0, N, Yw, Cp, Yf, J.ldy,
                                      pf, stream));
        if (Un)
            STIN_EDGE_BRACKET(stin_edge_relu_mean_fwd_map_f32(Yf, J.ldy, Yf + H, J.ldy, J.rowptr_dst, J.col_dst, row_map, N, H, hf, J.ldh,
                                                              1, J.mask, stream));
        else if (compact)
            STIN_EDGE_BRACKET(stin_edge_relu_mean_fwd_ti_f32(J.b1, Yf, J.ldy, J.rowptr_dst, J.col_dst, N, H, hf, J.ldh, 1, J.mask, stream));
        else
            STIN_EDGE_BRACKET(stin_edge_relu_mean_fwd_f32(Yf, J.ldy, Yf + H, J.ldy, J.rowptr_dst, J.col_dst, N, H, hf, J.ldh, 1, J.mask,
                                                          stream));
        // one graph, all-columns GEMM shape: the column sums of agg come out of GEMM2's epilogue (no pass over agg for them)
        const int64_t stat_groups = (J.B == 1 && J.gid == nullptr && !J.slice_quirk) ? stin_gemm_nt_colstats_groups(N, Cout, H, pf) : 0;
        const bool fused_stats = stat_groups > 0 && (size_t)stat_groups * 2 * Cout * sizeof(double) + 256 <= red_bytes;
        bool normed = false;
        if (fused_stats) {
            double* partial = reinterpret_cast<double*>(align256(red_ws));
            STIN_TRY(stin_gemm_nt_colstats_f32(hf, J.ldh, w2_op, H, J.b2, hf + H, J.ldh, nullptr, 0, N, Cout, H, aggf, Cout, pf, partial,
                                               (size_t)stat_groups * 2 * Cout * sizeof(double), stream));
            // (round 5) few row groups (the bottleneck level): every workgroup of the normalisation launch folds its own columns'
            // partials - no separate fold launch on the critical path; same sums, same order: bit-identical (k_norm_fold)
            int rc_fold = STIN_E_UNSUPPORTED;
            if (N > 0 && stin_norm_fold_rows(N, Cout, stat_groups) > 0)
                rc_fold = row_map
                              ? stin_norm_act_res_fwd_fold_map_f32(partial, stat_groups, aggf, Cout, static_cast<const float*>(res), ld_res,
                                                                   row_map, J.inv_cnt, J.eps, N, Cout, J.mean, J.rstd,
                                                                   static_cast<float*>(J.out), J.ldo, stream)
                              : stin_norm_act_res_fwd_fold_f32(partial, stat_groups, aggf, Cout, static_cast<const float*>(res), ld_res,
                                                               J.inv_cnt, J.eps, N, Cout, J.mean, J.rstd, static_cast<float*>(J.out),
                                                               J.ldo, stream);
            if (rc_fold == STIN_OK) normed = true;
            else if (rc_fold != STIN_E_UNSUPPORTED) return rc_fold;
            else STIN_TRY(stin_moments_final_f32(partial, stat_groups, Cout, J.inv_cnt, J.eps, J.mean, J.rstd, stream));
        } else {
            STIN_TRY(stin_gemm_nt_f32(hf, J.ldh, w2_op, H, J.b2, hf + H, J.ldh, nullptr, 0, N, Cout, H, aggf, Cout, pf, stream));
            STIN_TRY(fwd_stats(0, J, red_ws, red_bytes, stream));
        }
        if (!normed && row_map)
            STIN_TRY(stin_norm_act_res_fwd_map_f32(aggf, Cout, J.mean, J.rstd, J.gid, static_cast<const float*>(res), ld_res, row_map, N,
                                                   Cout, 1, static_cast<float*>(J.out), J.ldo, stream));
        else if (!normed)
            STIN_TRY(stin_norm_act_res_fwd_f32(aggf, Cout, J.mean, J.rstd, J.gid, static_cast<const float*>(res), ld_res, N, Cout, 1,
                                               static_cast<float*>(J.out), J.ldo, stream));
    } else {
        stin_bf16_t* Yh = static_cast<stin_bf16_t*>(J.Y);
        stin_bf16_t* hh = static_cast<stin_bf16_t*>(J.hE);
        STIN_TRY(stin_gemm_nt_bf16(static_cast<const stin_bf16_t*>(J.x), J.ldx, wcat, Cp, bcat, nullptr, 0, nullptr, 0, N, Yw, Cp, Yh, J.ldy,
                                   wbf, stream));
        STIN_EDGE_BRACKET(stin_edge_relu_mean_fwd_bf16(Yh, J.ldy, Yh + H, J.ldy, J.rowptr_dst, J.col_dst, N, H, hh, J.ldh, 1, J.mask, stream));
        STIN_TRY(stin_gemm_nt_bf16(hh, J.ldh, w2_op, H, J.b2, hh + H, J.ldh, nullptr, 0, N, Cout, H, J.agg, Cout, wbf, stream));
        STIN_TRY(fwd_stats(1, J, red_ws, red_bytes, stream));
        STIN_TRY(stin_norm_act_res_fwd_bf16(static_cast<const stin_bf16_t*>(J.agg), Cout, J.mean, J.rstd, J.gid,
                                            static_cast<const stin_bf16_t*>(res), ld_res, N, Cout, 1, static_cast<stin_bf16_t*>(J.out),
                                            J.ldo, stream));
    }
    return STIN_OK;
}

// Hand-off between consecutive blocks of stin_net_bwd (round 4).  The input gradient dx of block k is the output gradient of
// block k - 1, whose instance-norm backward starts with two column sums over (agg_{k-1}, dx): when block k's dx product runs on
// the panel kernel those sums ride on its epilogue (stin_gemm_nt_dotelu_f32) and block k - 1 only folds the partials
// (stin_norm_coef_from_partials_f32) - one short, contention-sensitive launch less on the critical path per hand-off.
struct BwdLink {
    // producer side (this block's dx product computes the NEXT block-in-backward-order's statistics)
    const float* next_agg = nullptr;
    int64_t next_ld = 0;
    const float* next_mean = nullptr;
    const float* next_rstd = nullptr;
    double* next_partial = nullptr;
    size_t next_partial_bytes = 0;
    int64_t produced_groups = 0;         // out: > 0 when the partials were written
    // consumer side (this block's statistics were computed by the block before it in backward order)
    const double* pre_partial = nullptr;
    int64_t pre_groups = 0;
};

// Backward of one STIN_OP_BLOCK op.  g = dL/dout [N, Cout]; J.dx may be NULL (block input needs no gradient).  Gradients of the
// reference-layout parameters are written to dW1 [H, Cin or 2 Cin], db1 [H], dW2 [Cout, H], db2 [Cout], dWs [Cout, Cin],
// dbs [Cout] (bias / shortcut outputs may be NULL when the parameter does not exist).
// Un != NULL (x_from_src, checked by `commutes`): the unpool op in front, whose output was never written - the one reader of x, the
// packed weight-gradient product, reads Un's input rows through its trace.
// g may already BE the shortcut columns of this block's dY (g_in_dy: the op behind wrote its dx there) - then nothing copies it.
static int block_bwd(int storage, const stin_net_op_t& J, const void* g, int64_t ldg, int prec_bwd, stin_stream_t stream,
                     stin_stream_t wgrad_stream, BwdLink* link, const stin_net_op_t* Un = nullptr) {
    const int64_t N = J.n_out;
    const int Cp = J.Cp, H = J.H, Cout = J.Cout, has_shortcut = J.has_shortcut;
    STIN_REQUIRE(N >= 0 && J.Cin > 0 && Cp >= J.Cin && H > 0 && Cout > 0 && J.B > 0, STIN_E_SIZE);
    STIN_REQUIRE(g && (J.x || Un) && J.hE && J.mask && J.agg && J.mean && J.rstd && J.wcatT && J.w2T && J.rowptr_dst && J.rowptr_src && J.col_src &&
                     J.xslot && J.w_src && J.inv_cnt && J.dW1 && J.dW2 && J.bwd_ws && (!has_shortcut || J.dWs),
                 STIN_E_NULL);
    STIN_REQUIRE(J.bwd_ws_bytes >= stin_edgeconv_block_bwd_workspace_bytes(N, Cp, H, Cout, has_shortcut, J.B, storage), STIN_E_WORKSPACE);
    const bool compact = J.trans_inv == STIN_TI_COMPACT;
    STIN_REQUIRE(!compact || storage == 0, STIN_E_UNSUPPORTED);
    const int Yw = stin_yw(H, Cout, has_shortcut, J.trans_inv);
    const BwdLayout L = bwd_layout(N, H, Cout, has_shortcut, J.B, storage);
    char* base = align256(J.bwd_ws);
    void* dagg = base + L.dagg;
    void* dhE = base + L.dhE;
    void* dY = base + L.dY;
    // compact layout: dY is [N, Yw] inside that region; the column partials of dA ([rows][H] floats, rows ~ N / 16..32) live behind it
    // in the H unused columns' worth of space (N * H * 4 bytes >= rows * H * 4)
    float* ti_colsum = nullptr;
    int64_t ti_rows = 0;
    if (compact) {
        ti_rows = stin_edge_bwd_ti_colsum_rows(N, H);
        ti_colsum = reinterpret_cast<float*>(static_cast<char*>(dY) + stin_up256((size_t)N * Yw * 4));
        STIN_REQUIRE(stin_up256((size_t)N * Yw * 4) + (size_t)ti_rows * H * 4 <= stin_up256((size_t)N * yw_wide(H, Cout, has_shortcut) * 4),
                     STIN_E_WORKSPACE);
    }
    float* coef[5];
    for (int i = 0; i < 5; ++i) coef[i] = reinterpret_cast<float*>(base + L.coef[i]);
    float *kk = coef[0], *mm = coef[1];
    const int32_t* sid_n = J.sid ? J.sid : J.gid;     // slice id of the norm backward (== graph id without the quirk)
    void* red_ws = base + L.red;
    void* tn_ws = base + L.tn;
    const size_t tn_bytes = (size_t)J.bwd_ws_bytes - (size_t)(static_cast<char*>(tn_ws) - static_cast<char*>(J.bwd_ws));
    const int pb = J.bwd_split ? (prec_bwd | STIN_GEMM_W_PRESPLIT | (J.bwd_split & STIN_GEMM_W_FRAG)) : prec_bwd;
    hipStream_t hs = (hipStream_t)stream;
    // weight-gradient GEMMs are off the critical path dx <- g: with use_side they run on wgrad_stream beside the edge-stage /
    // dx kernels of this block (and the head of the next one), ordered by the caller's events
    const bool side = J.use_side && wgrad_stream != nullptr && wgrad_stream != stream;
    if (side) STIN_REQUIRE(J.ev_dy && J.ev_done, STIN_E_NULL);
    stin_stream_t ws_ = side ? wgrad_stream : stream;
    // the fork event is bound to the edge-stage kernel's own completion signal where that launch is the last one before the fork
    // (STIN_LAUNCH_STOP, stin_common.h) - never under an active edge-stage bracket, whose stop event is recorded behind that launch
    bool bind_on = false;
    if (side && N > 0 && J.ev_edge1 == nullptr) {   // (a stream being captured into a hipGraph keeps the event-record node)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        bind_on = hipStreamIsCapturing(hs, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone;
    }
    struct StopEventGuard { ~StopEventGuard() { stin_tl_stop_event = nullptr; } } stop_event_guard;   // never left set on an error return
    bool bound = false;
    auto fork = [&]() -> int {     // the side stream continues behind ev_dy
        if (!side) return STIN_OK;
        hipError_t e = bound ? hipSuccess : hipEventRecord((hipEvent_t)J.ev_dy, hs);
        if (e == hipSuccess) e = hipStreamWaitEvent((hipStream_t)wgrad_stream, (hipEvent_t)J.ev_dy, 0);
        return (int)e;
    };

    if (storage == 0) {
        const float* gf = static_cast<const float*>(g);
        const float* hf = static_cast<const float*>(J.hE);
        const float* aggf = static_cast<const float*>(J.agg);
        float* dYf = static_cast<float*>(dY);
        // instance norm + ELU backward: two column sums finalised straight into the k / m coefficients, one elementwise pass
        if (link != nullptr && link->pre_partial != nullptr && link->pre_groups > 0 && !J.sid && J.B == 1 && J.gid == nullptr) {
            // the two column sums came out of the previous block's dx product (BwdLink): fold its partials - (round 5) inside the
            // normalisation launch itself where the row groups are few (k_norm_fold: every workgroup folds its own columns)
            // Measured (round 5): the forward form is 16 us where norm + fold were 19; the backward twin (stin_norm_act_bwd_fold_f32:
            // two fp64 folds per workgroup in front of the rows) 44 us where they were 39 - the backward keeps the separate fold.
            STIN_TRY(stin_norm_coef_from_partials_f32(link->pre_partial, link->pre_groups, Cout, J.rstd, J.inv_cnt, kk, mm, stream));
        } else {
            STIN_TRY(bwd_norm_coef(0, J, g, ldg, coef, red_ws, L.red_bytes, stream));
        }
        STIN_TRY(stin_norm_act_bwd_f32(aggf, Cout, gf, ldg, J.mean, J.rstd, J.rstd, kk, mm, J.gid, sid_n, N, Cout, 1,
                                       static_cast<float*>(dagg), Cout, stream));
        // second Linear: weight gradient (+ masked bias gradient) and input gradient
        STIN_TRY(stin_gemm_nt_f32(static_cast<const float*>(dagg), Cout, J.w2T, Cout, nullptr, nullptr, 0, nullptr, 0, N, H, Cout,
                                  static_cast<float*>(dhE), H, pb, stream));
        // edge stage backward from the saved ReLU mask -> dY = [dA | dB | g]
        // (a shortcut block's dY[:, 2H:] = g rides on the same launch when the rows allow 16-byte copies, else one 2-D memcpy)
        float* dYs = dYf + (Yw - Cout);                             // the shortcut columns of dY (has_shortcut)
        const bool placed = has_shortcut && gf == dYs && ldg == Yw;  // g_in_dy: the producer of g wrote it here
        const bool ride = has_shortcut && !placed && N > 0 && Cout % 4 == 0 && ldg % 4 == 0 && Yw % 4 == 0 && stin_aligned16(gf) &&
                          stin_aligned16(dYs) && Cout <= H;
        const bool bind = bind_on && (!has_shortcut || ride || placed);     // (no copy follows the edge launch)
        if (bind) stin_tl_stop_event = (hipEvent_t)J.ev_dy;
        if (compact)     // D = dB - dA in ONE row of H columns, + the column partials of dA for db1 (stin_graph.hip: k_edge_bwd_mask_ti)
            STIN_EDGE_BRACKET(stin_edge_relu_mean_bwd_mask_ti_f32(static_cast<const float*>(dhE), H, J.mask, J.rowptr_dst, J.w_src,
                                                                 J.rowptr_src, J.col_src, J.xslot, N, H, dYf, Yw, ride ? gf : nullptr, ldg,
                                                                 ride ? dYs : nullptr, Yw, ride ? Cout : 0, ti_colsum, ti_rows, stream));
        else
            STIN_EDGE_BRACKET(stin_edge_relu_mean_bwd_mask_f32(static_cast<const float*>(dhE), H, J.mask, J.rowptr_dst, J.w_src, J.rowptr_src,
                                                              J.col_src, J.xslot, N, H, dYf, Yw, dYf + H, Yw, ride ? gf : nullptr, ldg,
                                                              ride ? dYs : nullptr, Yw, ride ? Cout : 0, stream));
        if (has_shortcut && N > 0 && !ride && !placed) {
            hipError_t e = hipMemcpy2DAsync(dYs, (size_t)Yw * 4, gf, (size_t)ldg * 4, (size_t)Cout * 4, (size_t)N,
                                            hipMemcpyDeviceToDevice, hs);
            if (e != hipSuccess) return (int)e;
        }
        // first Linear (+ shortcut): packed weight gradient and the block-input gradient (+ identity residual)
        // all weight gradients: both transposed products in one grid + one finalize launch (stin_wgrad.hip), off the
        // critical path dx <- g on the caller's weight-gradient stream
        bound = bind && stin_tl_stop_event == nullptr;              // (the launch that took the event cleared it)
        stin_tl_stop_event = nullptr;
        STIN_TRY(fork());
        if (Un)     // x_up[v] = x_c[trace[v]] read where it is (the same slabs bit for bit; never the compact layout: `commutes`)
            STIN_TRY(stin_edgeconv_wgrad_map(0, dagg, Cout, hf, J.ldh, dYf, Yw, Un->x, Un->ldx, N, J.Cin, Cp, H, Cout, has_shortcut,
                                             J.trans_inv, prec_bwd, J.dW1, J.db1, J.dW2, J.db2, J.dWs, J.dbs, Un->trace, Un->n_in, tn_ws,
                                             tn_bytes, ws_));
        else
            STIN_TRY(stin_edgeconv_wgrad_ti(0, dagg, Cout, hf, J.ldh, dYf, Yw, J.x, J.ldx, N, J.Cin, Cp, H, Cout, has_shortcut, J.trans_inv,
                                            prec_bwd, J.dW1, J.db1, J.dW2, J.db2, J.dWs, J.dbs, ti_colsum, ti_rows, tn_ws, tn_bytes, ws_));
        if (J.dx != nullptr) {
            const bool link_ok = link != nullptr && link->next_agg != nullptr && link->next_ld % 4 == 0 && stin_aligned16(link->next_agg) &&
                                 stin_aligned16(link->next_mean) && stin_aligned16(link->next_rstd) && link->next_partial != nullptr;
            const int64_t lg = link_ok ? stin_gemm_nt_dotelu_groups(N, Cp, Yw, pb) : 0;
            if (lg > 0 && (size_t)lg * 2 * Cp * sizeof(double) <= link->next_partial_bytes) {
                STIN_TRY(stin_gemm_nt_dotelu_f32(dYf, Yw, J.wcatT, Yw, nullptr, has_shortcut ? nullptr : gf, ldg, N, Cp, Yw,
                                                 static_cast<float*>(J.dx), J.lddx, pb, link->next_agg, link->next_ld, link->next_mean,
                                                 link->next_rstd, link->next_partial, link->next_partial_bytes, stream));
                link->produced_groups = lg;
            } else {
                STIN_TRY(stin_gemm_nt_f32(dYf, Yw, J.wcatT, Yw, nullptr, nullptr, 0, has_shortcut ? nullptr : gf, ldg, N, Cp, Yw,
                                          static_cast<float*>(J.dx), J.lddx, pb, stream));
            }
        }
    } else {
        STIN_REQUIRE(Un == nullptr, STIN_E_UNSUPPORTED);
        const stin_bf16_t* gh = static_cast<const stin_bf16_t*>(g);
        const stin_bf16_t* hh = static_cast<const stin_bf16_t*>(J.hE);
        stin_bf16_t* dYh = static_cast<stin_bf16_t*>(dY);
        STIN_TRY(bwd_norm_coef(1, J, g, ldg, coef, red_ws, L.red_bytes, stream));
        STIN_TRY(stin_norm_act_bwd_bf16(static_cast<const stin_bf16_t*>(J.agg), Cout, gh, ldg, J.mean, J.rstd, J.rstd, kk, mm, J.gid, sid_n,
                                        N, Cout, 1, static_cast<stin_bf16_t*>(dagg), Cout, stream));
        const int wbb = (Cp % 8 == 0 && Cout % 8 == 0) ? STIN_GEMM_W_BF16 : 0;   // as written by the forward call's pack
        STIN_TRY(stin_gemm_nt_bf16(static_cast<const stin_bf16_t*>(dagg), Cout, J.w2T, Cout, nullptr, nullptr, 0, nullptr, 0, N, H, Cout,
                                   dhE, H, wbb, stream));
        const bool ride = has_shortcut && N > 0 && Cout % 8 == 0 && ldg % 8 == 0 && Yw % 8 == 0 && stin_aligned16(gh) &&
                          stin_aligned16(dYh + 2 * H);
        const bool bind = bind_on && (!has_shortcut || ride);
        if (bind) stin_tl_stop_event = (hipEvent_t)J.ev_dy;
        STIN_EDGE_BRACKET(stin_edge_relu_mean_bwd_mask_bf16(static_cast<const stin_bf16_t*>(dhE), H, J.mask, J.rowptr_dst, J.w_src,
                                                           J.rowptr_src, J.col_src, J.xslot, N, H, dYh, Yw, dYh + H, Yw, ride ? gh : nullptr,
                                                           ldg, ride ? dYh + 2 * H : nullptr, Yw, ride ? Cout : 0, stream));
        if (has_shortcut && N > 0 && !ride) {
            hipError_t e = hipMemcpy2DAsync(dYh + 2 * H, (size_t)Yw * 2, gh, (size_t)ldg * 2, (size_t)Cout * 2, (size_t)N,
                                            hipMemcpyDeviceToDevice, hs);
            if (e != hipSuccess) return (int)e;
        }
        bound = bind && stin_tl_stop_event == nullptr;
        stin_tl_stop_event = nullptr;
        STIN_TRY(fork());
        STIN_TRY(stin_edgeconv_wgrad(1, dagg, Cout, hh, J.ldh, dYh, Yw, J.x, J.ldx, N, J.Cin, Cp, H, Cout, has_shortcut, J.trans_inv, prec_bwd,
                                     J.dW1, J.db1, J.dW2, J.db2, J.dWs, J.dbs, tn_ws, tn_bytes, ws_));
        if (J.dx != nullptr)
            STIN_TRY(stin_gemm_nt_bf16(dYh, Yw, J.wcatT, Yw, nullptr, nullptr, 0, has_shortcut ? nullptr : gh, ldg, N, Cp, Yw, J.dx, J.lddx,
                                       wbb, stream));
    }
    // ev_done marks "this block's parameter gradients are written": on the weight-gradient stream, or (round 4) on the compute
    // stream for a block that does not use it - what the overlapped gradient all-reduce of a data-parallel step waits for
    // segment by segment while the rest of stin_net_bwd's kernels are still queued (train_step.FlatGradBucket.blocks_done)
    if (side || J.ev_done != nullptr) {
        hipError_t e = hipEventRecord((hipEvent_t)J.ev_done, side ? (hipStream_t)wgrad_stream : hs);
        if (e != hipSuccess) return (int)e;
    }
    return STIN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The graph part of the network - or one block of it - as one op list per direction (include/stin_hip.h: stin_net_op_t).  Only
// loops: a block op is the launch sequence above, every other op one of the existing entry points with the pointers of the host array.
extern "C" int stin_net_fwd(int storage, const stin_net_op_t* ops, int n_ops, stin_stream_t stream) {
    STIN_REQUIRE(n_ops >= 0 && (n_ops == 0 || ops != nullptr), STIN_E_NULL);
    STIN_REQUIRE(storage == 0 || storage == 1, STIN_E_UNSUPPORTED);
    for (int i = 0; i < n_ops; ++i) {
        const stin_net_op_t& J = ops[i];
        if (J.kind == STIN_OP_BLOCK) {
            const stin_net_op_t* un = (i > 0 && commutes(storage, ops[i - 1], J)) ? &ops[i - 1] : nullptr;
            STIN_REQUIRE(un != nullptr || (J.y_from_src == 0 && J.x_from_src == 0), STIN_E_UNSUPPORTED);   // (its Y holds the coarse rows only)
            STIN_TRY(block_fwd(storage, J, stream, un));
        } else if (J.kind == STIN_OP_POOL_MAX) {
            if (storage)
                STIN_TRY(stin_pool_max_fwd_bf16(static_cast<const stin_bf16_t*>(J.x), J.ldx, J.rowptr_dst, J.col_dst, J.n_out, J.Cout,
                                                static_cast<stin_bf16_t*>(J.out), J.ldo, J.arg, stream));
            else
                STIN_TRY(stin_pool_max_fwd_f32(static_cast<const float*>(J.x), J.ldx, J.rowptr_dst, J.col_dst, J.n_out, J.Cout,
                                               static_cast<float*>(J.out), J.ldo, J.arg, stream));
        } else if (J.kind == STIN_OP_UNPOOL) {
            // no output: a forward nobody differentiates, whose next block takes its first product from this op's input rows
            if (J.out == nullptr && i + 1 < n_ops && commutes(storage, J, ops[i + 1])) continue;
            if (storage)
                STIN_TRY(stin_gather_rows_bf16(static_cast<const stin_bf16_t*>(J.x), J.ldx, J.trace, nullptr, J.n_out, J.Cout,
                                               static_cast<stin_bf16_t*>(J.out), J.ldo, stream));
            else
                STIN_TRY(stin_gather_rows_f32(static_cast<const float*>(J.x), J.ldx, J.trace, nullptr, J.n_out, J.Cout,
                                              static_cast<float*>(J.out), J.ldo, stream));
        } else {
            return STIN_E_UNSUPPORTED;
        }
    }
    return STIN_OK;
}

// g_in_dy: op i's input gradient IS the output gradient g of the shortcut block ops[i - 1], which needs it as the last Cout columns of
// its dY = [dA | dB | g] - so op i writes it there (every producer takes a leading dimension) and the block copies nothing.
// True where that block permits it and the two agree in rows and width without channel padding; *dx / *lddx = the target.
static bool g_in_dy(int storage, const stin_net_op_t* ops, int n_ops, int i, void** dx, int64_t* lddx) {
    if (storage != 0 || ops == nullptr || i < 1 || i >= n_ops) return false;
    const stin_net_op_t &J = ops[i], &Pn = ops[i - 1];
    if (Pn.kind != STIN_OP_BLOCK || Pn.g_in_dy == 0 || Pn.has_shortcut == 0 || Pn.bwd_ws == nullptr || J.dx == nullptr) return false;
    if (Pn.n_out <= 0 || Pn.Cp <= 0 || Pn.H <= 0 || Pn.Cout <= 0 || Pn.B <= 0) return false;
    int64_t rows, width;
    if (J.kind == STIN_OP_BLOCK) {
        if (J.Cin != J.Cp) return false;
        rows = J.n_out, width = J.Cp;
    } else if (J.kind == STIN_OP_POOL_MAX || J.kind == STIN_OP_UNPOOL) {
        rows = J.n_in, width = J.Cout;
    } else {
        return false;
    }
    const int Yw = stin_yw(Pn.H, Pn.Cout, Pn.has_shortcut, Pn.trans_inv);
    if (rows != Pn.n_out || width != Pn.Cout || Pn.Cout % 4 != 0 || Yw % 4 != 0) return false;
    if (Pn.bwd_ws_bytes < stin_edgeconv_block_bwd_workspace_bytes(Pn.n_out, Pn.Cp, Pn.H, Pn.Cout, Pn.has_shortcut, Pn.B, storage)) return false;
    char* t = align256(Pn.bwd_ws) + bwd_layout(Pn.n_out, Pn.H, Pn.Cout, Pn.has_shortcut, Pn.B, storage).dY + (size_t)(Yw - Pn.Cout) * 4;
    if (!stin_aligned16(t)) return false;
    if (dx) *dx = t;
    if (lddx) *lddx = Yw;
    return true;
}

extern "C" int stin_net_bwd_g_in_dy(int storage, const stin_net_op_t* ops, int n_ops, int i) {
    return g_in_dy(storage, ops, n_ops, i, nullptr, nullptr) ? 1 : 0;
}

extern "C" int stin_net_bwd(int storage, const stin_net_op_t* ops, int n_ops, const void* g, int64_t ldg, int prec_bwd,
                            stin_stream_t stream, stin_stream_t wgrad_stream) {
    STIN_REQUIRE(n_ops >= 0 && (n_ops == 0 || ops != nullptr), STIN_E_NULL);
    STIN_REQUIRE(storage == 0 || storage == 1, STIN_E_UNSUPPORTED);
    const void* gi = g;
    int64_t ldgi = ldg;
    const double* pre_partial = nullptr;       // statistics of op i computed by op i + 1's dx product (BwdLink)
    int64_t pre_groups = 0;
    for (int i = n_ops - 1; i >= 0; --i) {
        stin_net_op_t Jr;                       // op i on a copy of its record when its dx goes into the dY of the block in front
        void* dx_in_dy = nullptr;
        int64_t ld_in_dy = 0;
        const bool redirect = g_in_dy(storage, ops, n_ops, i, &dx_in_dy, &ld_in_dy);
        if (redirect) {
            Jr = ops[i];
            Jr.dx = dx_in_dy;
            Jr.lddx = ld_in_dy;
        }
        const stin_net_op_t& J = redirect ? Jr : ops[i];
        STIN_REQUIRE(J.dx != nullptr || i == 0, STIN_E_NULL);
        if (J.kind == STIN_OP_BLOCK) {
            // x_from_src: the unpool op in front never wrote this block's x (found the way stin_net_fwd finds it)
            const stin_net_op_t* un = (J.x_from_src != 0 && i > 0 && commutes(storage, ops[i - 1], J)) ? &ops[i - 1] : nullptr;
            STIN_REQUIRE(un != nullptr || J.x_from_src == 0, STIN_E_UNSUPPORTED);
            BwdLink link;
            link.pre_partial = pre_partial;
            link.pre_groups = pre_groups;
            pre_partial = nullptr;
            pre_groups = 0;
            if (storage == 0 && i > 0 && J.dx != nullptr && ops[i - 1].kind == STIN_OP_BLOCK) {
                // op i - 1 is a block whose output is this block's input: single graph, no slice quirk, same rows, and this
                // block's input width is that block's output width (no channel padding in between)
                const stin_net_op_t& Pn = ops[i - 1];
                if (Pn.B == 1 && Pn.gid == nullptr && Pn.sid == nullptr && Pn.n_out == J.n_out && Pn.Cout == J.Cp && J.Cin == J.Cp &&
                    Pn.bwd_ws != nullptr) {
                    const BwdLayout Ln = bwd_layout(Pn.n_out, Pn.H, Pn.Cout, Pn.has_shortcut, Pn.B, storage);
                    link.next_agg = static_cast<const float*>(Pn.agg);
                    link.next_ld = Pn.Cout;
                    link.next_mean = Pn.mean;
                    link.next_rstd = Pn.rstd;
                    link.next_partial = reinterpret_cast<double*>(align256(Pn.bwd_ws) + Ln.red);
                    link.next_partial_bytes = Ln.red_bytes > 256 ? Ln.red_bytes - 256 : 0;
                }
            }
            STIN_TRY(block_bwd(storage, J, gi, ldgi, prec_bwd, stream, wgrad_stream, &link, un));
            if (link.produced_groups > 0) {
                pre_partial = link.next_partial;
                pre_groups = link.produced_groups;
            }
        } else if (J.kind == STIN_OP_POOL_MAX) {
            if (J.dx != nullptr) {
                if (storage)
                    STIN_TRY(stin_pool_max_bwd_bf16(static_cast<const stin_bf16_t*>(gi), ldgi, J.arg, J.trace, J.n_in, J.Cout,
                                                    static_cast<stin_bf16_t*>(J.dx), J.lddx, stream));
                else
                    STIN_TRY(stin_pool_max_bwd_f32(static_cast<const float*>(gi), ldgi, J.arg, J.trace, J.n_in, J.Cout,
                                                   static_cast<float*>(J.dx), J.lddx, stream));
            }
        } else if (J.kind == STIN_OP_UNPOOL) {
            if (J.dx != nullptr) {
                if (storage)
                    STIN_TRY(stin_segment_sum_bf16(static_cast<const stin_bf16_t*>(gi), ldgi, J.rowptr_dst, J.col_dst, J.n_in, J.Cout, 0,
                                                   static_cast<stin_bf16_t*>(J.dx), J.lddx, stream));
                else   // (non-temporal loads on a once-read source beyond the Infinity Cache, as functional.segment_sum asks for)
                    STIN_TRY(stin_segment_sum_f32(static_cast<const float*>(gi), ldgi, J.rowptr_dst, J.col_dst, J.n_in, J.Cout,
                                                  (J.n_out * (int64_t)J.Cout * 4 > ((int64_t)256 << 20)) ? STIN_SEG_NONTEMPORAL : 0,
                                                  static_cast<float*>(J.dx), J.lddx, stream));
            }
        } else {
            return STIN_E_UNSUPPORTED;
        }
        gi = J.dx;
        ldgi = J.lddx;
    }
    return STIN_OK;
}
