// Per-vertex dense GEMMs of the STINet hot path on the gfx950 matrix cores.  Kernel families in this file:
//   k_gemm_nt / k_gemm_tn              exact fp32 (v_mfma_f32_32x32x2_f32: bit-for-bit an fp32 fmaf chain, 157 TFLOP/s peak)
//   k_gemm_nt_bf16s / k_gemm_tn_bf16s  fp32 storage, operands split on the fly into 16-bit pieces (bf16 x3 / x6, fp16 x3),
//                                      v_mfma_f32_32x32x16_{bf16,f16} with fp32 accumulation - what the network runs on
//   k_gemm_nt_b16 / k_gemm_tn_b16      bf16 storage (the *_bf16 entry points), one MFMA per k-step
//
//   stin_gemm_nt_f32 : C[M, Nc] = A[M, K] . W[Nc, K]^T (+ bias)      forward GEMMs and dgrad (with W^T)
//   stin_gemm_tn_f32 : dW[Nc, K(+1)] = G[M, Nc]^T . [X[M, K] | 1]    weight (+bias) gradients, split over M
//
// M is the vertex count (1e4..1e6), Nc and K are channel counts (3..2052): tall-skinny shapes where
// library GEMMs pick poor tiles.  Fragment maps (cdna_hip_programming.md §3): A operand lane l holds
// A[i = l&31][k = l>>5], B operand B[k = l>>5][j = l&31]; C/D reg r of lane l is
// row (r&3) + 8*(r>>2) + 4*(l>>5), col l&31.
#include <cstdlib>
#include <tuple>
#include <type_traits>
#include "stin_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BLOCK = 256;
constexpr int BK = 32;

// NT block -> output tile, XCD-aware: workgroups are dealt round-robin to the 8 XCDs (blockIdx % 8), each with its own
// 4 MB L2.  Row tile r lives on XCD r % 8 and its column blocks get CONSECUTIVE slots of that XCD, so the A rows of a tile
// are fetched across the fabric once and then re-read from that L2 by the other column blocks (a 2-D grid dispatches
// x-fastest: the column blocks of one row tile would start thousands of workgroups apart, on different XCDs).
__device__ __forceinline__ bool nt_block_tile(int64_t M, int Nc, int BM, int BN, int64_t& m0, int& n0) {
    const int64_t L = blockIdx.x;
    const int ncol = (Nc + BN - 1) / BN;
    if ((M + BM - 1) / BM < 16) {        // too few row tiles to give every XCD its own (coarsest levels): plain order
        m0 = (L / ncol) * BM;
        n0 = (int)(L % ncol) * BN;
        return true;
    }
    const int64_t j = L >> 3;
    const int64_t rt = (j / ncol) * 8 + (L & 7);
    if (rt * BM >= M) return false;
    m0 = rt * BM;
    n0 = (int)(j % ncol) * BN;
    return true;
}

#include "gemm_nt_tiled.inc"   // NT products: the exact-fp32 tiling and the split-16-bit tiling (k_gemm_nt, k_gemm_nt_bf16s)
#include "gemm_nt_stream.inc"   // NT products, streaming rows through wave-private LDS (k_gemm_nt_stream and its epilogue modes)
#include "gemm_nt_resident.inc"   // NT products on fragment-order weights: resident strip, all-columns and balanced column-panel kernels (k_gemm_nt_strip / _wide / _panel)
#include "gemm_tn.inc"   // TN (weight-gradient) products of fp32 rows: exact-fp32 and split-bf16 tilings (k_gemm_tn, k_gemm_tn_bf16s)
#include "gemm_b16.inc"   // GEMMs of bf16-STORAGE rows: NT tiled / LDS-DMA, TN register-transpose / hardware-transposed reads
#include "gemm_tn_skinny.inc"   // TN products with K <= 16 (k_gemm_tn_skinny) and the slab reduction (k_reduce_slabs)
inline int stin_cu_count() { return stin_cu_count_dev(); }          // (per device: stin_common.h)
#include "gemm_nt_route.inc"   // host only: which kernel runs an NT product - the switches, the rules, nt_route
#include "gemm_tn_route.inc"   // host only: which kernel runs a TN product - the switches, the rules, tn_route
}  // namespace

// ------------------------------------------------------------------ NT products: route (gemm_nt_route.inc), then launch
namespace {
struct NtOperands {                    // one NT product of fp32 rows as the kernels take it; what an entry point does not have stays zero
    const float* A; int64_t lda; const float* W; int64_t ldw;                             // (in the order of the entry points' arguments)
    const float *bias, *row_mask; int64_t ld_mask; const float* residual; int64_t ld_res;
    float* C; int64_t ldc;
    double* stats;                     // [groups][2][Nc] partial sums of a fused epilogue (column statistics, dot-ELU, BatchNorm backward)
    NtDotElu de;
    stin_bn_tf tf;
    const float *X, *P, *Q;            // BatchNorm backward (the streaming kernel's modes 1 / 2): pre-norm rows, the two column sums
    int64_t ldx;
    float inv_n;
};
inline int nt_parts(const float* bias, const float* row_mask, const float* residual) {
    return (bias ? STIN_NT_PART_BIAS : 0) | (row_mask ? STIN_NT_PART_ROW_MASK : 0) | (residual ? STIN_NT_PART_RESIDUAL : 0);
}

// THE launch of every NT and TN kernel of this file: raise the kernel's dynamic-LDS limit on this device where it needs more than
// 64 KB (max_lds > 0), then launch.  One flag per kernel instantiation.
struct KernelLaunch { dim3 grid; int threads; int64_t lds; int max_lds; hipStream_t stream; };
template <auto KERNEL, typename... Args>
void launch_kernel(const KernelLaunch& l, const std::tuple<Args...>& args) {
    if (l.max_lds > 0) {
        static stin_once_per_device raised;
        stin_raise_dynamic_lds(raised, (const void*)KERNEL, l.max_lds);
    }
    std::apply([&](auto... a) { hipLaunchKernelGGL(KERNEL, l.grid, dim3(l.threads), (size_t)l.lds, l.stream, a...); }, args);
}

// ---- one launch table per family: the route's tile / parameter -> the template arguments
template <int BM, int BN, int WM, int WN, typename Args>
void nt_launch_tile(const NtRoute& r, int precision, bool wpre, const KernelLaunch& l, const Args& a) {
    if (wpre) {                                                     // (pre-split W: 16-byte rows, 64 x 64 and 128 x 128 only)
        if constexpr (BN != 32) {
            if (precision == STIN_GEMM_BF16X3) launch_kernel<k_gemm_nt_bf16s<BM, BN, WM, WN, 2, __bf16, true, true>>(l, a);
            else launch_kernel<k_gemm_nt_bf16s<BM, BN, WM, WN, 2, _Float16, true, true>>(l, a);
        }
    } else if (precision == STIN_GEMM_F32)
        r.vec ? launch_kernel<k_gemm_nt<BM, BN, WM, WN, true>>(l, a) : launch_kernel<k_gemm_nt<BM, BN, WM, WN, false>>(l, a);
    else if (precision == STIN_GEMM_BF16X3)
        r.vec ? launch_kernel<k_gemm_nt_bf16s<BM, BN, WM, WN, 2, __bf16, true>>(l, a) : launch_kernel<k_gemm_nt_bf16s<BM, BN, WM, WN, 2, __bf16, false>>(l, a);
    else if (precision == STIN_GEMM_BF16X6)
        r.vec ? launch_kernel<k_gemm_nt_bf16s<BM, BN, WM, WN, 3, __bf16, true>>(l, a) : launch_kernel<k_gemm_nt_bf16s<BM, BN, WM, WN, 3, __bf16, false>>(l, a);
    else
        r.vec ? launch_kernel<k_gemm_nt_bf16s<BM, BN, WM, WN, 2, _Float16, true>>(l, a) : launch_kernel<k_gemm_nt_bf16s<BM, BN, WM, WN, 2, _Float16, false>>(l, a);
}
void nt_launch_tiled(const NtRoute& r, const NtProblem& p, int precision, const NtOperands& o, hipStream_t stream) {
    const KernelLaunch l = {dim3((unsigned)r.grid), BLOCK, 0, 0, stream};
    const auto a = std::make_tuple(o.A, o.lda, o.W, o.ldw, o.bias, o.row_mask, o.ld_mask, o.residual, o.ld_res, p.M, p.Nc, p.K, o.C, o.ldc, o.tf);
    const bool wpre = (p.precision & STIN_GEMM_W_PRESPLIT) != 0;
    if (r.bn == 32) nt_launch_tile<128, 32, 4, 1>(r, precision, wpre, l, a);
    else if (r.bm == 128) nt_launch_tile<128, 128, 2, 2>(r, precision, wpre, l, a);
    else nt_launch_tile<64, 64, 2, 2>(r, precision, wpre, l, a);
}

template <int NT, int MODE, bool TF, typename Args>
void nt_launch_stream_tiles(int precision, const KernelLaunch& l, const Args& a) {
    if (precision == STIN_GEMM_BF16X3) launch_kernel<k_gemm_nt_stream<64, NT, 2, __bf16, MODE, TF>>(l, a);
    else if (precision == STIN_GEMM_BF16X6) launch_kernel<k_gemm_nt_stream<64, NT, 3, __bf16, MODE, TF>>(l, a);
    else launch_kernel<k_gemm_nt_stream<64, NT, 2, _Float16, MODE, TF>>(l, a);
}
template <int MODE, bool TF>
void nt_launch_stream_mode(const NtRoute& r, const NtProblem& p, int precision, const NtOperands& o, hipStream_t stream) {
    const KernelLaunch l = {dim3((unsigned)r.grid, (unsigned)r.grid_y), BLOCK, r.lds, 160 * 1024, stream};
    const auto a = std::make_tuple(o.A, o.lda, o.W, o.ldw, p.M, p.Nc, p.K, o.X, o.ldx, o.tf, o.P, o.Q, o.inv_n, o.stats, o.C, o.ldc, o.bias,
                                   o.row_mask, o.ld_mask, o.residual, o.ld_res, (p.precision & STIN_GEMM_W_PRESPLIT) ? 1 : 0);
    if (r.param == 2) nt_launch_stream_tiles<2, MODE, TF>(precision, l, a);
    else nt_launch_stream_tiles<4, MODE, TF>(precision, l, a);
}
void nt_launch_stream(const NtRoute& r, const NtProblem& p, int precision, const NtOperands& o, hipStream_t stream) {
    if (p.has(STIN_NT_PART_BN_BWD_STATS)) nt_launch_stream_mode<1, false>(r, p, precision, o, stream);
    else if (p.has(STIN_NT_PART_BN_BWD_APPLY)) nt_launch_stream_mode<2, false>(r, p, precision, o, stream);
    else if (p.has(STIN_NT_PART_BN_TF)) nt_launch_stream_mode<0, true>(r, p, precision, o, stream);
    else nt_launch_stream_mode<0, false>(r, p, precision, o, stream);
}

template <typename PT>
void nt_launch_strip(const NtRoute& r, const NtProblem& p, const NtOperands& o, hipStream_t stream) {
    const int KC = p.K < 256 ? p.K : 256, P = (p.Nc + ST_PANEL - 1) / ST_PANEL;
    const int64_t units = ((p.M + r.bm - 1) / r.bm) * P;
    const KernelLaunch l = {dim3((unsigned)r.grid), r.param == 22 ? 512 : 256, r.lds, 160 * 1024, stream};
    const auto a = std::make_tuple(o.A, o.lda, o.W, o.bias, o.row_mask, o.ld_mask, o.residual, o.ld_res, p.M, p.Nc, p.K, o.C, o.ldc, KC, units,
                                   P, r.vec_out);
    switch (r.param) {
        case 22: launch_kernel<k_gemm_nt_strip<PT, 2, 2>>(l, a); break;
        case 41: launch_kernel<k_gemm_nt_strip<PT, 4, 1>>(l, a); break;
        default: launch_kernel<k_gemm_nt_strip<PT, 2, 1>>(l, a); break;
    }
}
template <typename PT>
void nt_launch_wide(const NtRoute& r, const NtProblem& p, const NtOperands& o, hipStream_t stream) {
    const KernelLaunch l = {dim3((unsigned)r.grid), p.Nc * r.param, 0, 0, stream};       // Nc / 64 column waves x param row waves x 64 lanes
    const auto a = std::make_tuple(o.A, o.lda, o.W, o.bias, o.row_mask, o.ld_mask, o.residual, o.ld_res, p.M, p.K, o.C, o.ldc, o.stats, r.vec_out);
    if (p.Nc == 128) launch_kernel<k_gemm_nt_wide<PT, 2, 2>>(l, a);
    else if (r.param == 2) launch_kernel<k_gemm_nt_wide<PT, 4, 2>>(l, a);
    else launch_kernel<k_gemm_nt_wide<PT, 4, 1>>(l, a);
}
template <typename PT>
void nt_launch_panel(const NtRoute& r, const NtProblem& p, const NtOperands& o, hipStream_t stream) {
    const int P = p.Nc / 128, nrb = (int)((p.M + r.bm - 1) / r.bm);
    const KernelLaunch l = {dim3((unsigned)r.grid), 512, r.lds, 160 * 1024, stream};
    const auto a = std::make_tuple(o.A, o.lda, o.W, o.bias, o.row_mask, o.ld_mask, o.residual, o.ld_res, p.M, p.Nc, p.K, o.C, o.ldc, o.stats, nrb,
                                   P, nrb >= 16 ? 1 : 0, o.de);
    switch (r.param) {                                              // 32-row tiles per block = MT0 + MT1
        case 2: launch_kernel<k_gemm_nt_panel<PT, 1, 1>>(l, a); break;
        case 3: launch_kernel<k_gemm_nt_panel<PT, 2, 1>>(l, a); break;
        case 4: launch_kernel<k_gemm_nt_panel<PT, 2, 2>>(l, a); break;
        case 5: launch_kernel<k_gemm_nt_panel<PT, 3, 2>>(l, a); break;
        case 6: launch_kernel<k_gemm_nt_panel<PT, 3, 3>>(l, a); break;
        case 7: launch_kernel<k_gemm_nt_panel<PT, 4, 3>>(l, a); break;
        case 8: launch_kernel<k_gemm_nt_panel<PT, 4, 4>>(l, a); break;
        default: launch_kernel<k_gemm_nt_panel<PT, 5, 4>>(l, a); break;
    }
}

// sizes and alignment facts of an fp32-row call -> its route (p: storage, M, Nc, K, precision, parts, null_operand set by the caller)
int nt_f32_route(NtProblem& p, const NtOperands& o, const NtSwitches& sw, NtRoute* r) {
    stin_clear_stale_error();
    const bool bn_bwd = p.has(STIN_NT_PART_BN_BWD_STATS | STIN_NT_PART_BN_BWD_APPLY);
    // (the streaming kernel asked for by name answers STIN_E_UNSUPPORTED for a shape it does not serve, an empty one included)
    STIN_REQUIRE(bn_bwd || p.has(STIN_NT_PART_STREAM_ONLY) || (p.M >= 0 && p.Nc > 0 && p.K > 0), STIN_E_SIZE);
    STIN_REQUIRE(o.lda >= p.K && o.ldw >= p.K && (p.has(STIN_NT_PART_BN_BWD_STATS) || o.ldc >= p.Nc), STIN_E_SIZE);
    STIN_REQUIRE((o.residual == nullptr || o.ld_res >= p.Nc) && (!bn_bwd || o.ldx >= p.Nc), STIN_E_SIZE);
    const bool in16 = o.lda % 4 == 0 && o.ldw % 4 == 0 && o.ldx % 4 == 0 && stin_aligned16(o.A) && stin_aligned16(o.W) && stin_aligned16(o.X);
    const bool out16 = o.ldc % 4 == 0 && stin_aligned16(o.C) && (o.residual == nullptr || (o.ld_res % 4 == 0 && stin_aligned16(o.residual)));
    const bool tf16 = stin_aligned16(o.tf.mean) && stin_aligned16(o.tf.rstd) && stin_aligned16(o.tf.gamma) && stin_aligned16(o.tf.beta);
    p.align = (in16 ? STIN_NT_ALIGN_IN : 0) | (out16 ? STIN_NT_ALIGN_OUT : 0) | (tf16 ? STIN_NT_ALIGN_TF : 0) |
              (stin_aligned16(o.bias) ? STIN_NT_ALIGN_BIAS : 0);
    *r = nt_route(p, sw, stin_cu_count());
    return r->status;
}
int nt_f32_launch(const NtRoute& r, const NtProblem& p, const NtOperands& o, stin_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int precision = p.precision & ~(STIN_GEMM_W_PRESPLIT | STIN_GEMM_W_FRAG);
    const bool bf = precision == STIN_GEMM_BF16X3;                  // (the fragment-order kernels: bf16 or fp16 pieces)
    switch (r.family) {
        case STIN_NT_NONE: return STIN_OK;
        case STIN_NT_TILED: nt_launch_tiled(r, p, precision, o, stream); break;
        case STIN_NT_STREAM: nt_launch_stream(r, p, precision, o, stream); break;
        case STIN_NT_STRIP: bf ? nt_launch_strip<__bf16>(r, p, o, stream) : nt_launch_strip<_Float16>(r, p, o, stream); break;
        case STIN_NT_WIDE: bf ? nt_launch_wide<__bf16>(r, p, o, stream) : nt_launch_wide<_Float16>(r, p, o, stream); break;
        case STIN_NT_PANEL: bf ? nt_launch_panel<__bf16>(r, p, o, stream) : nt_launch_panel<_Float16>(r, p, o, stream); break;
        default: return STIN_E_UNSUPPORTED;
    }
    return stin_launch_status();
}
int nt_f32(int parts, int precision, int64_t M, int Nc, int K, const NtOperands& o, bool null_operand, const NtSwitches& sw,
           stin_stream_t stream) {
    NtProblem p = {0, M, Nc, K, precision, parts, 0, null_operand};
    NtRoute r;
    const int rc = nt_f32_route(p, o, sw, &r);
    return rc != STIN_OK ? rc : nt_f32_launch(r, p, o, stream);
}
// the statistics groups a fused epilogue will write: the route of the ALIGNED form of the problem (what the launches carry);
// 0: not served
int64_t nt_groups(int parts, int precision, int64_t M, int Nc, int K, const NtSwitches& sw) {
    if (M <= 0 || Nc <= 0 || K <= 0) return 0;
    const NtProblem p = {0, M, Nc, K, precision, parts, STIN_NT_ALIGN_IN | STIN_NT_ALIGN_OUT | STIN_NT_ALIGN_TF | STIN_NT_ALIGN_BIAS, false};
    const NtRoute r = nt_route(p, sw, stin_cu_count());
    return r.status == STIN_OK ? r.groups : 0;
}
}  // namespace

extern "C" int stin_gemm_nt_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias,
                                const float* row_mask, int64_t ld_mask, const float* residual, int64_t ld_res, int64_t M,
                                int Nc, int K, float* C, int64_t ldc, int precision, stin_stream_t stream) {
    return nt_f32(nt_parts(bias, row_mask, residual), precision, M, Nc, K,
                  {A, lda, W, ldw, bias, row_mask, ld_mask, residual, ld_res, C, ldc}, !(A && W && C), nt_switches(), stream);
}

// C = relu(gamma ((A - mean) rstd) + beta) W^T: BatchNorm1d + ReLU over the columns of A applied while the rows are staged
// (SingleConvMeshNet's per-EDGE product: the normalised [E, 2 cout] matrix never exists in memory).  W plain fp32 [Nc, K].
extern "C" int stin_gemm_nt_bn_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* mean, const float* rstd,
                                   const float* gamma, const float* beta, int64_t M, int Nc, int K, float* C, int64_t ldc,
                                   int precision, stin_stream_t stream) {
    STIN_REQUIRE((precision & (STIN_GEMM_W_PRESPLIT | STIN_GEMM_W_FRAG)) == 0, STIN_E_UNSUPPORTED);
    NtOperands o = {A, lda, W, ldw, nullptr, nullptr, 0, nullptr, 0, C, ldc};
    o.tf = {mean, rstd, gamma, beta};
    return nt_f32(STIN_NT_PART_BN_TF, precision, M, Nc, K, o, !(A && W && C && mean && rstd && gamma && beta), nt_switches(), stream);
}
// The plain product C = A W^T (mean == NULL) or C = relu(gamma ((A - mean) rstd) + beta) W^T on the streaming kernel BY NAME, whatever
// the row count; STIN_E_UNSUPPORTED for the shapes it does not serve (K not a multiple of 64 in 64 .. 512, rows not 16-byte aligned,
// a pre-split precision flag).  stin_gemm_nt_f32 / stin_gemm_nt_bn_f32 route M >= 65 536 rows to it (STIN_NT_STREAM=0: never).
extern "C" int stin_gemm_nt_stream_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* mean, const float* rstd,
                                       const float* gamma, const float* beta, int64_t M, int Nc, int K, float* C, int64_t ldc,
                                       int precision, stin_stream_t stream) {
    NtOperands o = {A, lda, W, ldw, nullptr, nullptr, 0, nullptr, 0, C, ldc};
    o.tf = {mean, rstd, gamma, beta};
    return nt_f32(STIN_NT_PART_STREAM_ONLY | (mean ? STIN_NT_PART_BN_TF : 0), precision, M, Nc, K, o,
                  !(A && W && C && (mean == nullptr || (rstd && gamma && beta))), nt_switches(), stream);
}

// dh = A W^T used ONLY as the output gradient of BatchNorm1d + ReLU over the rows X (k_gemm_nt_stream MODE 1 / 2; SingleConvMeshNet's
// per-edge backward, edge_conv_filter.py:34-44): `stats` = the product with the two column sums on its epilogue (nothing stored:
// partial [groups][2][Nc] doubles, then sums [2][Nc] floats = P | Q, the gradients of gamma | beta); `apply` = the product again,
// stored as dx = rstd gamma (d - Q / n - nhat P / n).  groups = stin_gemm_nt_bn_bwd_groups (0: shape / precision not served -
// the caller keeps stin_gemm_nt_f32 + stin_colreduce_f32(DOT_BN_RELU) + stin_bn_act_bwd_f32).  W plain fp32 [Nc, K].
extern "C" int64_t stin_gemm_nt_bn_bwd_groups(int64_t M, int Nc, int K, int precision) {
    const NtSwitches sw = nt_switches();
    return sw.bnbwd ? nt_groups(STIN_NT_PART_BN_BWD_STATS, precision, M, Nc, K, sw) : 0;
}
extern "C" int stin_gemm_nt_bn_bwd_stats_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* X, int64_t ldx,
                                             const float* mean, const float* rstd, const float* gamma, const float* beta, int64_t M,
                                             int Nc, int K, int precision, double* partial, size_t partial_bytes, float* sums,
                                             stin_stream_t stream) {
    NtOperands o = {A, lda, W, ldw, nullptr, nullptr, 0, nullptr, 0, nullptr, 0};
    o.X = X, o.ldx = ldx, o.tf = {mean, rstd, gamma, beta}, o.stats = partial;
    NtProblem p = {0, M, Nc, K, precision, STIN_NT_PART_BN_BWD_STATS, 0, !(A && W && X && mean && rstd && gamma && beta && partial && sums)};
    NtRoute r;
    int rc = nt_f32_route(p, o, nt_switches(), &r);
    if (rc != STIN_OK) return rc;
    STIN_REQUIRE(partial_bytes >= (size_t)r.groups * 2 * (size_t)Nc * sizeof(double), STIN_E_WORKSPACE);
    rc = nt_f32_launch(r, p, o, stream);
    if (rc != STIN_OK) return rc;
    hipLaunchKernelGGL(k_partial_sums_final, dim3((unsigned)((2 * Nc + 63) / 64)), dim3(1024), 0, (hipStream_t)stream, partial, r.groups,
                       2 * Nc, sums);
    return stin_launch_status();
}
extern "C" int stin_gemm_nt_bn_bwd_apply_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* X, int64_t ldx,
                                             const float* mean, const float* rstd, const float* gamma, const float* beta,
                                             const float* sums, float inv_n, int64_t M, int Nc, int K, float* dx, int64_t lddx,
                                             int precision, stin_stream_t stream) {
    NtOperands o = {A, lda, W, ldw, nullptr, nullptr, 0, nullptr, 0, dx, lddx};
    o.X = X, o.ldx = ldx, o.tf = {mean, rstd, gamma, beta}, o.P = sums, o.Q = sums + Nc, o.inv_n = inv_n;
    return nt_f32(STIN_NT_PART_BN_BWD_APPLY, precision, M, Nc, K, o, !(A && W && X && mean && rstd && gamma && beta && sums && dx),
                  nt_switches(), stream);
}

// The GEMM plus the FIRST stage of the instance-norm statistics of its output: colstats [groups][2][Nc] doubles (groups =
// stin_gemm_nt_colstats_groups; 0 = this shape / precision does not support it: only the all-columns kernel's blocks own whole
// rows - one group per 64 rows - and the panel kernel folds two groups per row block).  Second stage: stin_moments_final_f32.
extern "C" int64_t stin_gemm_nt_colstats_groups(int64_t M, int Nc, int K, int precision) {
    return nt_groups(STIN_NT_PART_COLSTATS, precision, M, Nc, K, nt_switches());
}
extern "C" int stin_gemm_nt_colstats_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias,
                                         const float* row_mask, int64_t ld_mask, const float* residual, int64_t ld_res,
                                         int64_t M, int Nc, int K, float* C, int64_t ldc, int precision, double* colstats,
                                         size_t colstats_bytes, stin_stream_t stream) {
    const NtSwitches sw = nt_switches();
    const int64_t groups = nt_groups(STIN_NT_PART_COLSTATS, precision, M, Nc, K, sw);
    STIN_REQUIRE(groups > 0, STIN_E_UNSUPPORTED);
    STIN_REQUIRE(colstats != nullptr, STIN_E_NULL);
    STIN_REQUIRE(colstats_bytes >= (size_t)groups * 2 * (size_t)Nc * sizeof(double), STIN_E_WORKSPACE);
    NtOperands o = {A, lda, W, ldw, bias, row_mask, ld_mask, residual, ld_res, C, ldc};
    o.stats = colstats;
    return nt_f32(nt_parts(bias, row_mask, residual) | STIN_NT_PART_COLSTATS, precision, M, Nc, K, o, !(A && W && C), sw, stream);
}

// The GEMM plus the first stage of the instance-norm + ELU BACKWARD statistics of the layer whose output gradient it produces
// (NtDotElu): partial [groups][2][Nc] doubles, groups = stin_gemm_nt_dotelu_groups (0: this shape / precision is not served
// by the panel kernel - the caller keeps its separate reduction).  Second stage: stin_norm_coef_from_partials_f32.
extern "C" int64_t stin_gemm_nt_dotelu_groups(int64_t M, int Nc, int K, int precision) {
    return nt_groups(STIN_NT_PART_COLSTATS | STIN_NT_PART_DOTELU, precision, M, Nc, K, nt_switches());
}
extern "C" int stin_gemm_nt_dotelu_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias,
                                       const float* residual, int64_t ld_res, int64_t M, int Nc, int K, float* C, int64_t ldc,
                                       int precision, const float* nx, int64_t ld_nx, const float* nmean, const float* nrstd,
                                       double* partial, size_t partial_bytes, stin_stream_t stream) {
    const NtSwitches sw = nt_switches();
    const int64_t groups = nt_groups(STIN_NT_PART_COLSTATS | STIN_NT_PART_DOTELU, precision, M, Nc, K, sw);
    STIN_REQUIRE(groups > 0, STIN_E_UNSUPPORTED);
    STIN_REQUIRE(nx && nmean && nrstd && partial, STIN_E_NULL);
    STIN_REQUIRE(ld_nx >= Nc, STIN_E_SIZE);
    STIN_REQUIRE(ld_nx % 4 == 0 && stin_aligned16(nx) && stin_aligned16(nmean) && stin_aligned16(nrstd), STIN_E_ALIGN);
    STIN_REQUIRE(partial_bytes >= (size_t)groups * 2 * (size_t)Nc * sizeof(double), STIN_E_WORKSPACE);
    NtOperands o = {A, lda, W, ldw, bias, nullptr, 0, residual, ld_res, C, ldc};
    o.stats = partial;
    o.de.x = nx, o.de.ldx = ld_nx, o.de.mean = nmean, o.de.rstd = nrstd;
    return nt_f32(nt_parts(bias, nullptr, residual) | STIN_NT_PART_COLSTATS | STIN_NT_PART_DOTELU, precision, M, Nc, K, o, !(A && W && C), sw,
                  stream);
}

// The route an NT product of this description takes - host only: nothing is launched, no device is touched (stin_hip.h).
extern "C" int stin_gemm_nt_geometry(int storage, int64_t M, int Nc, int K, int precision, int parts, int align, int cu, int32_t* out10) {
    STIN_REQUIRE(out10 != nullptr, STIN_E_NULL);
    STIN_REQUIRE(storage == 0 || storage == 1, STIN_E_UNSUPPORTED);
    STIN_REQUIRE(M >= 0 && Nc > 0 && K > 0 && cu > 0, STIN_E_SIZE);
    const NtProblem p = {storage, M, Nc, K, precision, parts, align, false};
    const NtRoute r = nt_route(p, nt_switches(), cu);
    if (r.status != STIN_OK) return r.status;
    const int64_t v[10] = {r.family, r.bm, r.bn, r.param, r.vec, r.vec_out, r.lds, r.grid, r.grid_y, r.groups};
    for (int i = 0; i < 10; ++i) out10[i] = (int32_t)v[i];
    return STIN_OK;
}

// ------------------------------------------------------------------ TN products: route (gemm_tn_route.inc), then launch
TnSwitches stin_tn_switches() { return tn_switches(); }
TnRoute stin_tn_route(const TnProblem& p, const TnSwitches& sw) { return tn_route(p, sw); }

// The slab workspace of a product of these four arguments: the largest chunks x tn_chunk_stride x 4 + 256 over the routes a caller can
// reach with them - both storages, every precision, operands that are 16-byte vectors or not (row pitches beyond Nc / K add no
// case: they only decide between these two), and the settings of the switches that move the geometry (STIN_TN_WS on fp32 rows,
// STIN_TN_BIG on bf16 rows).  Asked of tn_route itself; at least one slab.
extern "C" size_t stin_gemm_tn_workspace_bytes(int64_t M, int Nc, int K, int ones_column) {
    if (M < 0 || Nc <= 0 || K <= 0) return 0;
    int64_t chunks = 1;
    auto ask = [&](int storage, int precision, bool aligned16, const TnSwitches& sw) {
        const TnProblem p = {storage, M, Nc, K, Nc, K, precision, ones_column != 0, aligned16, false, false, false};
        const TnRoute r = tn_route(p, sw);
        if (r.status == STIN_OK && r.chunks > chunks) chunks = r.chunks;
    };
    for (int aligned16 = 0; aligned16 < 2; ++aligned16) {
        for (int precision : {STIN_GEMM_F32, STIN_GEMM_BF16X3, STIN_GEMM_BF16X6})
            for (int pc = 0; pc < 2; ++pc) ask(0, precision, aligned16 != 0, TnSwitches{pc != 0, -1, -1});
        for (int big = -1; big <= 1; ++big) ask(1, STIN_GEMM_BF16X3, aligned16 != 0, TnSwitches{true, big, -1});
    }
    return (size_t)chunks * (size_t)tn_chunk_stride(Nc, (K + 3) & ~3) * sizeof(float) + 256;
}

// One TN product: its argument checks, its route and its kernel argument (shared with stin_wgrad.hip)
int stin_tn_setup(stin_tn_problem* p, TnRoute* r, const TnSwitches& sw, int storage, const void* G, int64_t ldg, const void* X,
                  int64_t ldx, int64_t M, int Nc, int K, int ones_column, const void* row_w, int64_t ld_w, int precision, float* slab,
                  const stin_bn_tf* xtf, const int32_t* x_row_map) {
    const bool tf16 = xtf != nullptr && stin_aligned16(xtf->mean) && stin_aligned16(xtf->rstd) && stin_aligned16(xtf->gamma) && stin_aligned16(xtf->beta);
    const TnProblem q = {storage, M, Nc, K, ldg, ldx, precision, ones_column != 0, stin_aligned16(G) && stin_aligned16(X),
                         xtf != nullptr, tf16, x_row_map != nullptr};
    *r = tn_route(q, sw);
    if (r->status == STIN_E_SIZE) return STIN_E_SIZE;
    STIN_REQUIRE(slab && (M == 0 || (G && X)), STIN_E_NULL);
    STIN_REQUIRE(xtf == nullptr || (xtf->mean && xtf->rstd && xtf->gamma && xtf->beta), STIN_E_NULL);
    if (r->status != STIN_OK) return r->status;
    p->xtf.mean = p->xtf.rstd = p->xtf.gamma = p->xtf.beta = nullptr;
    if (xtf != nullptr) p->xtf = *xtf;
    p->G = static_cast<const float*>(G);
    p->X = static_cast<const float*>(X);
    p->row_w = static_cast<const float*>(row_w);
    p->slab = slab;
    p->ldg = ldg, p->ldx = ldx, p->ld_w = ld_w, p->M = M, p->chunks = r->chunks;
    p->Nc = Nc, p->K = K, p->Kq = r->Kq, p->has_bias = ones_column ? 1 : 0, p->rows_per_chunk = r->rows_per_chunk;
    p->tiles_i = r->tiles_i, p->tiles_j = r->tiles_j, p->vec = r->vec;
    p->TI = (short)r->TI, p->TJ = (short)r->TJ;
    p->block0 = 0;
    p->x_row_map = x_row_map;
    return STIN_OK;
}

// The route a TN product of this shape takes, for tests and tools (stin_hip.h).  Host only: nothing is launched, no device is touched.
// stin_gemm_tn_geometry keeps the eight values its callers have room for; stin_gemm_tn_route adds the kernel family and the grid.
static int tn_query(int storage, int64_t M, int Nc, int K, int64_t ldg, int64_t ldx, int aligned16, int ones_column, int precision,
                    int n, int32_t* out) {
    STIN_REQUIRE(out != nullptr, STIN_E_NULL);
    STIN_REQUIRE(storage == 0 || storage == 1, STIN_E_UNSUPPORTED);
    const TnProblem p = {storage, M, Nc, K, ldg, ldx, precision, ones_column != 0, aligned16 != 0, false, false, false};
    const TnRoute r = tn_route(p, tn_switches());
    if (r.status != STIN_OK) return r.status;
    const int64_t v[10] = {r.TI, r.TJ, r.tiles_i, r.tiles_j, r.rows_per_chunk, r.chunks, r.vec, r.family == STIN_TN_FAMILY_PC, r.family, r.grid};
    for (int i = 0; i < n; ++i) out[i] = (int32_t)v[i];
    return STIN_OK;
}
extern "C" int stin_gemm_tn_geometry(int storage, int64_t M, int Nc, int K, int64_t ldg, int64_t ldx, int aligned16, int ones_column,
                                     int precision, int32_t* out8) {
    return tn_query(storage, M, Nc, K, ldg, ldx, aligned16, ones_column, precision, 8, out8);
}
extern "C" int stin_gemm_tn_route(int storage, int64_t M, int Nc, int K, int64_t ldg, int64_t ldx, int aligned16, int ones_column,
                                  int precision, int32_t* out10) {
    return tn_query(storage, M, Nc, K, ldg, ldx, aligned16, ones_column, precision, 10, out10);
}

namespace {
// ---- the launch table: the route's family and tile -> the template arguments
template <typename F>
void tn_with_tile(const TnRoute& r, F&& f) {                        // the four tiles of the four-wave kernels
    typedef std::integral_constant<int, 64> c64;
    typedef std::integral_constant<int, 128> c128;
    if (r.TI == 128 && r.TJ == 128) f(c128(), c128());
    else if (r.TI == 128) f(c128(), c64());
    else if (r.TJ == 128) f(c64(), c128());
    else f(c64(), c64());
}
template <typename T>
auto tn_args(const stin_tn_problem& p) {                            // the arguments the tiled kernels share, operands as rows of T
    return std::make_tuple(reinterpret_cast<const T*>(p.G), p.ldg, reinterpret_cast<const T*>(p.X), p.ldx, p.M, p.Nc, p.K, p.Kq, p.has_bias,
                           reinterpret_cast<const T*>(p.row_w), p.ld_w, p.rows_per_chunk, p.tiles_i, p.tiles_j, p.chunks, p.slab);
}
int tn_launch(const stin_tn_problem& p, const TnRoute& r, int precision, hipStream_t stream) {
    const KernelLaunch l = {dim3((unsigned)r.grid), r.threads, r.lds, r.family == STIN_TN_FAMILY_B16_TR ? (int)r.lds : 0, stream};
    switch (r.family) {
        case STIN_TN_FAMILY_NONE: return STIN_OK;
        case STIN_TN_FAMILY_PC: return stin_tn_ws_launch(&p, &r, nullptr, nullptr, (stin_stream_t)stream);
        case STIN_TN_FAMILY_SKINNY: {                               // KP = K: the shape rule admits 4, 8, 12, 16
            const auto a = std::make_tuple(p.G, p.ldg, p.X, p.ldx, p.M, p.Nc, p.K, p.Kq, p.has_bias, p.row_w, p.ld_w, p.rows_per_chunk, p.slab);
            switch (p.Kq) {
                case 4: launch_kernel<k_gemm_tn_skinny<4>>(l, a); break;
                case 8: launch_kernel<k_gemm_tn_skinny<8>>(l, a); break;
                case 12: launch_kernel<k_gemm_tn_skinny<12>>(l, a); break;
                default: launch_kernel<k_gemm_tn_skinny<16>>(l, a); break;
            }
            break;
        }
        case STIN_TN_FAMILY_F32:
            tn_with_tile(r, [&](auto ti, auto tj) {
                const auto a = std::tuple_cat(tn_args<float>(p), std::make_tuple(p.xtf));
                r.vec ? launch_kernel<k_gemm_tn<ti(), tj(), true>>(l, a) : launch_kernel<k_gemm_tn<ti(), tj(), false>>(l, a);
            });
            break;
        case STIN_TN_FAMILY_BF16S:
            tn_with_tile(r, [&](auto ti, auto tj) {
                const auto a = std::tuple_cat(tn_args<float>(p), std::make_tuple(p.xtf));
                if (precision == STIN_GEMM_BF16X6)
                    r.vec ? launch_kernel<k_gemm_tn_bf16s<ti(), tj(), 3, true>>(l, a) : launch_kernel<k_gemm_tn_bf16s<ti(), tj(), 3, false>>(l, a);
                else
                    r.vec ? launch_kernel<k_gemm_tn_bf16s<ti(), tj(), 2, true>>(l, a) : launch_kernel<k_gemm_tn_bf16s<ti(), tj(), 2, false>>(l, a);
            });
            break;
        case STIN_TN_FAMILY_B16_REG:
            tn_with_tile(r, [&](auto ti, auto tj) {
                const auto a = tn_args<stin_bf16>(p);
                r.vec ? launch_kernel<k_gemm_tn_b16<ti(), tj(), true>>(l, a) : launch_kernel<k_gemm_tn_b16<ti(), tj(), false>>(l, a);
            });
            break;
        case STIN_TN_FAMILY_B16_TR:
            if (r.TI == 256) launch_kernel<k_gemm_tn_b16_tr<2, 4, 4, 2>>(l, tn_args<stin_bf16>(p));
            else launch_kernel<k_gemm_tn_b16_tr<2, 2, 2, 2>>(l, tn_args<stin_bf16>(p));
            break;
    }
    return stin_launch_status();
}
}  // namespace

// The TN kernels of one product or of two (pb != NULL): partial slabs only (k_reduce_slabs / k_wgrad_finalize add them).  Both
// products on the producer / consumer kernel: ONE grid; else one launch each.
int stin_tn_slabs(const stin_tn_problem* pa, const TnRoute* ra, const stin_tn_problem* pb, const TnRoute* rb, int precision,
                  stin_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (pb != nullptr && ra->family == STIN_TN_FAMILY_PC && rb->family == STIN_TN_FAMILY_PC) return stin_tn_ws_launch(pa, ra, pb, rb, stream_);
    int rc = tn_launch(*pa, *ra, precision, stream);
    if (rc == STIN_OK && pb != nullptr) rc = tn_launch(*pb, *rb, precision, stream);
    return rc;
}

// THE driver of the six stand-alone TN entry points: checks, slab alignment, route, launch, fold
static int gemm_tn_impl(int storage, const void* G, int64_t ldg, const void* X, int64_t ldx, int64_t M, int Nc, int K, int ones_column,
                        const void* row_weight, int64_t ld_weight, float* dW, int64_t lddw, float* db, int precision, void* workspace,
                        size_t workspace_bytes, stin_stream_t stream_, const stin_bn_tf* xtf = nullptr) {
    stin_clear_stale_error();
    hipStream_t stream = (hipStream_t)stream_;
    const int Kp = K + ((ones_column && db == nullptr) ? 1 : 0);
    STIN_REQUIRE(M >= 0 && Nc > 0 && K > 0 && ldg >= Nc && ldx >= K && lddw >= Kp, STIN_E_SIZE);
    STIN_REQUIRE(dW && workspace && (M == 0 || (G && X)), STIN_E_NULL);
    STIN_REQUIRE(workspace_bytes >= stin_gemm_tn_workspace_bytes(M, Nc, K, ones_column), STIN_E_WORKSPACE);
    STIN_REQUIRE(precision == STIN_GEMM_F32 || precision == STIN_GEMM_BF16X3 || precision == STIN_GEMM_BF16X6, STIN_E_UNSUPPORTED);
    float* slab = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    stin_tn_problem p;
    TnRoute r;
    int rc = stin_tn_setup(&p, &r, tn_switches(), storage, G, ldg, X, ldx, M, Nc, K, ones_column, row_weight, ld_weight, precision, slab, xtf, nullptr);
    if (rc != STIN_OK) return rc;
    // the slab the kernels will write must fit what the caller was told to allocate
    STIN_REQUIRE((size_t)r.chunks * (size_t)tn_chunk_stride(Nc, r.Kq) * sizeof(float) + 256 <= workspace_bytes, STIN_E_WORKSPACE);
    rc = stin_tn_slabs(&p, &r, nullptr, nullptr, precision, stream_);
    if (rc != STIN_OK) return rc;
    const int64_t n4 = (int64_t)Nc * r.Kq / 4 + (p.has_bias ? (Nc + 3) / 4 : 0);
    hipLaunchKernelGGL(k_reduce_slabs, dim3((unsigned)((n4 + FN_COLS - 1) / FN_COLS)), dim3(BLOCK), 0, stream, slab, r.chunks, Nc, K, r.Kq,
                       p.has_bias, dW, lddw, db);
    return stin_launch_status();
}
extern "C" int stin_gemm_tn_f32(const float* G, int64_t ldg, const float* X, int64_t ldx, int64_t M, int Nc, int K,
                                int ones_column, const float* row_weight, int64_t ld_weight, float* dW, int64_t lddw,
                                int precision, void* workspace, size_t workspace_bytes, stin_stream_t stream_) {
    return gemm_tn_impl(0, G, ldg, X, ldx, M, Nc, K, ones_column, row_weight, ld_weight, dW, lddw, nullptr, precision, workspace,
                            workspace_bytes, stream_);
}
// dW [Nc, K] = G^T relu(gamma ((X - mean) rstd) + beta): the weight gradient of SingleConvMeshNet's per-edge Linear from the
// PRE-normalisation rows (the BatchNorm1d + ReLU of stin_gemm_nt_bn_f32 applied to the X operand while it is staged)
extern "C" int stin_gemm_tn_bn_f32(const float* G, int64_t ldg, const float* X, int64_t ldx, const float* mean, const float* rstd,
                                   const float* gamma, const float* beta, int64_t M, int Nc, int K, float* dW, int64_t lddw,
                                   int precision, void* workspace, size_t workspace_bytes, stin_stream_t stream_) {
    stin_bn_tf tf;
    tf.mean = mean;
    tf.rstd = rstd;
    tf.gamma = gamma;
    tf.beta = beta;
    return gemm_tn_impl(0, G, ldg, X, ldx, M, Nc, K, 0, nullptr, 0, dW, lddw, nullptr, precision, workspace, workspace_bytes, stream_, &tf);
}
// weight gradient dW [Nc, K] (row pitch lddw >= K) and bias gradient db [Nc] as SEPARATE destinations - e.g. the views of an
// nn.Linear's weight.grad / bias.grad in a flat gradient bucket: no [Nc, K + 1] intermediate and no slicing copies afterwards
extern "C" int stin_gemm_tn_wb_f32(const float* G, int64_t ldg, const float* X, int64_t ldx, int64_t M, int Nc, int K,
                                   const float* row_weight, int64_t ld_weight, float* dW, int64_t lddw, float* db, int precision,
                                   void* workspace, size_t workspace_bytes, stin_stream_t stream_) {
    STIN_REQUIRE(db != nullptr, STIN_E_NULL);
    return gemm_tn_impl(0, G, ldg, X, ldx, M, Nc, K, 1, row_weight, ld_weight, dW, lddw, db, precision, workspace, workspace_bytes,
                            stream_);
}

// ------------------------------------------------------------------ bf16-storage entry points
namespace {
template <int BM, int BN, int WM, int WN, typename OUT, typename Args>
void nt_launch_b16_tile(const NtRoute& r, bool wb, const KernelLaunch& l, const Args& a) {
    if (wb) launch_kernel<k_gemm_nt_b16<BM, BN, WM, WN, OUT, true, true>>(l, a);
    else if (r.vec) launch_kernel<k_gemm_nt_b16<BM, BN, WM, WN, OUT, true>>(l, a);
    else launch_kernel<k_gemm_nt_b16<BM, BN, WM, WN, OUT, false>>(l, a);
}
}  // namespace
extern "C" int stin_gemm_nt_bf16(const stin_bf16_t* A_, int64_t lda, const float* W, int64_t ldw, const float* bias,
                                 const stin_bf16_t* row_mask_, int64_t ld_mask, const stin_bf16_t* residual_,
                                 int64_t ld_res, int64_t M, int Nc, int K, void* C, int64_t ldc, int c_is_f32,
                                 stin_stream_t stream_) {
    stin_clear_stale_error();
    hipStream_t stream = (hipStream_t)stream_;
    const stin_bf16* A = reinterpret_cast<const stin_bf16*>(A_);
    const stin_bf16* row_mask = reinterpret_cast<const stin_bf16*>(row_mask_);
    const stin_bf16* residual = reinterpret_cast<const stin_bf16*>(residual_);
    STIN_REQUIRE(M >= 0 && Nc > 0 && K > 0 && lda >= K && ldw >= K && ldc >= Nc, STIN_E_SIZE);
    STIN_REQUIRE(residual == nullptr || ld_res >= Nc, STIN_E_SIZE);
    const bool wb = (c_is_f32 & STIN_GEMM_W_BF16) != 0;          // flags: bit 0 = fp32 output, STIN_GEMM_W_BF16 = bf16 weight operand
    const bool in16 = lda % 8 == 0 && ldw % (wb ? 8 : 4) == 0 && stin_aligned16(A) && stin_aligned16(W);
    const NtProblem p = {1, M, Nc, K, wb ? STIN_GEMM_W_BF16 : 0, (c_is_f32 & 1) ? STIN_NT_PART_OUT_F32 : 0,
                         (in16 ? STIN_NT_ALIGN_IN : 0) | ((ldc % 8 == 0 && stin_aligned16(C)) ? STIN_NT_ALIGN_OUT : 0), !(A && W && C)};
    const NtRoute r = nt_route(p, nt_switches(), stin_cu_count());
    if (r.status != STIN_OK || r.family == STIN_NT_NONE) return r.status;
    auto launch = [&](auto* c) {                                    // c: the output rows in their type, float or bf16
        typedef typename std::remove_pointer<decltype(c)>::type OUT;
        const auto head = std::make_tuple(A, lda);
        const auto tail = std::make_tuple(ldw, bias, row_mask, ld_mask, residual, ld_res, M, Nc, K, c, ldc, r.vec_out);
        if (r.family == STIN_NT_B16_GLDS) {
            const auto a = std::tuple_cat(head, std::make_tuple(reinterpret_cast<const stin_bf16*>(W)), tail);
            const KernelLaunch l = {dim3((unsigned)r.grid), r.bm == 256 ? 512 : 256, r.lds, (int)r.lds, stream};
            if (r.bm == 256) launch_kernel<k_gemm_nt_b16_glds<OUT, 2, 4, 4, 2>>(l, a);
            else launch_kernel<k_gemm_nt_b16_glds<OUT, 2, 2, 2, 2>>(l, a);
            return;
        }
        const auto a = std::tuple_cat(head, std::make_tuple(W), tail);
        const KernelLaunch l = {dim3((unsigned)r.grid), BLOCK, 0, 0, stream};
        if (r.bn == 32) nt_launch_b16_tile<128, 32, 4, 1, OUT>(r, wb, l, a);
        else if (r.bm == 128) nt_launch_b16_tile<128, 64, 2, 2, OUT>(r, wb, l, a);
        else nt_launch_b16_tile<64, 64, 2, 2, OUT>(r, wb, l, a);
    };
    if (c_is_f32 & 1) launch(static_cast<float*>(C));
    else launch(static_cast<stin_bf16*>(C));
    return stin_launch_status();
}

extern "C" int stin_gemm_tn_bf16(const stin_bf16_t* G_, int64_t ldg, const stin_bf16_t* X_, int64_t ldx, int64_t M, int Nc,
                                 int K, int ones_column, const stin_bf16_t* row_weight_, int64_t ld_weight, float* dW,
                                 int64_t lddw, void* workspace, size_t workspace_bytes, stin_stream_t stream_) {
    return gemm_tn_impl(1, G_, ldg, X_, ldx, M, Nc, K, ones_column, row_weight_, ld_weight, dW, lddw, nullptr, STIN_GEMM_BF16X3, workspace,
                        workspace_bytes, stream_);
}
extern "C" int stin_gemm_tn_wb_bf16(const stin_bf16_t* G_, int64_t ldg, const stin_bf16_t* X_, int64_t ldx, int64_t M, int Nc,
                                    int K, const stin_bf16_t* row_weight_, int64_t ld_weight, float* dW, int64_t lddw, float* db,
                                    void* workspace, size_t workspace_bytes, stin_stream_t stream_) {
    STIN_REQUIRE(db != nullptr, STIN_E_NULL);
    return gemm_tn_impl(1, G_, ldg, X_, ldx, M, Nc, K, 1, row_weight_, ld_weight, dW, lddw, db, STIN_GEMM_BF16X3, workspace, workspace_bytes,
                        stream_);
}
