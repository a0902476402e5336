// Shared helpers for the libstin_hip.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include "../../include/stin_hip.h"

// The Python side packs these records field by field from the header's declarations (no padding anywhere); the sizes anchor
// the layouts on the C side.
static_assert(sizeof(stin_plan_job_t) == 120, "stin_plan_job_t layout");
static_assert(sizeof(stin_order_level_t) == 32, "stin_order_level_t layout");
static_assert(sizeof(stin_relabel_job_t) == 64, "stin_relabel_job_t layout");
static_assert(sizeof(stin_pack_job_t) == 112, "stin_pack_job_t layout");
static_assert(sizeof(stin_net_op_t) == 480, "stin_net_op_t layout");
static_assert(sizeof(stin_crop_seg_t) == 128, "stin_crop_seg_t layout");

#define STIN_WAVE 64

#define STIN_REQUIRE(cond, code) \
    do {                         \
        if (!(cond)) return (code); \
    } while (0)

// hipGetLastError() is per-thread sticky state shared with every other HIP user in the process
// (PyTorch included): drop whatever an earlier, unrelated call left behind before we launch.
static inline void stin_clear_stale_error() { (void)hipGetLastError(); }

// Fork without a marker packet (round 4).  hipEventRecord on the compute stream puts a barrier packet behind the kernel and the
// next kernel waits for the command processor to retire it: ~4 us of idle compute stream per fork (profiles/probes/fork_bind_probe.hip:
// record + wait + side kernel 16.1 us per link of an 11.0 us chain, event bound to the kernel's own completion signal 12.0).  A
// caller that wants "this launch is done" as an event sets stin_tl_stop_event; a launch site that supports it passes the event as
// hipExtLaunchKernelGGL's stopEvent and clears the variable (= "bound"); the caller records the event the ordinary way if the
// variable is still set afterwards.
extern thread_local hipEvent_t stin_tl_stop_event;
#define STIN_LAUNCH_STOP(KERNEL, GRID, BLOCK_, STREAM, ...)                                                          \
    do {                                                                                                             \
        if (stin_tl_stop_event != nullptr) {                                                                         \
            hipExtLaunchKernelGGL(KERNEL, GRID, BLOCK_, 0, STREAM, nullptr, stin_tl_stop_event, 0, __VA_ARGS__);     \
            stin_tl_stop_event = nullptr;                                                                            \
        } else {                                                                                                     \
            hipLaunchKernelGGL(KERNEL, GRID, BLOCK_, 0, STREAM, __VA_ARGS__);                                        \
        }                                                                                                            \
    } while (0)

static inline int stin_launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? STIN_OK : (int)e;
}

// Shapes whose pre-split NT weight operand is stored in MFMA fragment order under STIN_GEMM_W_FRAG (stin_hip.h), i.e. the
// shapes the resident-strip kernel takes.  Layout constraints: K % 64 == 0, Nc % 32 == 0.  Selection (measured per shape on
// MI355X, profiles/r02_gemm_shapes.md): one resident K chunk (K <= 256) with enough work per staged strip (K >= 128) and
// at least 2.5 column panels (Nc >= 320) - 5-15 % faster there; narrower outputs leave waves of the 128-column panel idle,
// longer K would add its chunks through memory, and both stay on the tiled kernel.
// Narrow outputs with a long reduction (Nc = 256 and K >= 512, Nc = 128 and K >= 256; K a multiple of 64) go to the
// all-columns kernel (k_gemm_nt_wide), which reads the same layout; shorter K measured slower there than on the 64x64 tiling.
__host__ __device__ static inline bool stin_w_frag_shape(int Nc, int K) {
    if (K % 64 != 0) return false;
    if ((Nc == 256 && K >= 512) || (Nc == 128 && K >= 256)) return true;
    return Nc % 32 == 0 && K >= 128 && K <= 256 && Nc >= 320;
}

// Width of the packed first-Linear operand / of Y and dY of a fused block.  trans_inv: 0 = EdgeConv ([Wa - Wb ; Wb ; Ws], A and B
// materialised), 1 = translation-invariant, both halves materialised ([-W1 ; W1 ; Ws]), 2 = translation-invariant COMPACT (round 6):
// the operand is [W1 ; Ws], only B = x W1^T exists - A_i = b1 - B_i is formed by the edge stage (the value the GEMM wrote for mode 1
// up to one ulp of the accumulator) - and the backward pass carries D = dB - dA (stin_hip.h, STIN_TI_COMPACT).
__host__ __device__ static inline int stin_yw(int H, int Cout, int has_shortcut, int trans_inv) {
    return (trans_inv == STIN_TI_COMPACT ? H : 2 * H) + (has_shortcut ? Cout : 0);
}

// Ticket words of the one-launch reductions (stin_norm.hip k_colreduce_t, stin_tail.hip k_linear_tanh_bwd) live in a global
// array of `slots` rows and every launch takes the next row, so launches in flight never share a word.  A launch that is being
// CAPTURED into a hipGraph bakes its row into the graph and will run at every replay - possibly beside eager launches whose
// rotating counter has come round to the same row.  Captured launches therefore rotate through the upper half of the rows and
// eager launches through the lower half: the two populations never meet.
#include <atomic>
static inline int stin_ticket_slot(std::atomic<unsigned>& seq_eager, std::atomic<unsigned>& seq_captured, int slots, hipStream_t stream) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
    const unsigned half = (unsigned)slots / 2;
    if (capturing) return (int)(half + seq_captured.fetch_add(1, std::memory_order_relaxed) % half);
    return (int)(seq_eager.fetch_add(1, std::memory_order_relaxed) % half);
}

// Per-DEVICE caches (round 6; a process may drive more than one GPU): the CU count, and "this function's dynamic-LDS attribute has
// been raised on this device" (hipFuncSetAttribute is per device: a process-wide once-flag left the second GPU's launches of the
// > 64 KB kernels failing).
static inline int stin_device_slot() {
    int d = 0;
    return (hipGetDevice(&d) == hipSuccess && d >= 0 && d < 64) ? d : 0;
}
static inline int stin_cu_count_dev() {
    static std::atomic<int> n[64];
    const int d = stin_device_slot();
    int v = n[d].load(std::memory_order_relaxed);
    if (v == 0) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || v <= 0) v = 256;
        n[d].store(v, std::memory_order_relaxed);
    }
    return v;
}
struct stin_once_per_device {
    std::atomic<unsigned long long> mask{0};
    bool done() const { return (mask.load(std::memory_order_acquire) >> stin_device_slot() & 1ull) != 0; }
    void publish() { mask.fetch_or(1ull << stin_device_slot(), std::memory_order_release); }
};
// Raise a kernel's dynamic-LDS limit on the current device.  "Raised" is published only AFTER hipFuncSetAttribute has returned: a
// second host thread that arrives earlier sets the attribute again (idempotent) instead of launching without it.
static inline void stin_raise_dynamic_lds(stin_once_per_device& raised, const void* kernel, int bytes) {
    if (raised.done()) return;
    (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    raised.publish();
}

// splitmix64's finaliser: the counter-based hash of the circle masks' centres (stin_mask.hip) and of the surface samples
// (stin_surface.hip).  The constants are part of both contracts (include/stin_hip.h).
__device__ inline uint64_t stin_mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static inline bool stin_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// workspace regions start on 256 bytes
static inline size_t stin_up256(size_t v) { return (v + 255) & ~(size_t)255; }

// Lanes that cooperate on one feature row: smallest power of two >= ceil(C/4), capped at a wave.
static inline int stin_group_lanes(int c4) {
    int g = 1;
    while (g < c4 && g < STIN_WAVE) g <<= 1;
    return g;
}

// fp64 sum over the 64 lanes of a wave (lane 0 holds it): shuffle-down by 32, 16, ... 1
__device__ __forceinline__ double stin_wave_sum(double v) {
#pragma unroll
    for (int o = STIN_WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o, STIN_WAVE);
    return v;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// bf16 STORAGE (the *_bf16 entry points): rows of __bf16 in HBM, every kernel widens to fp32 on load, computes and
// accumulates in fp32 and rounds to nearest-even on store.  A 4-channel chunk is 8 bytes.
typedef __bf16 stin_bf16;
typedef __bf16 stin_bf16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4(const stin_bf16* p) {
    const uint2 r = *reinterpret_cast<const uint2*>(p);
    return make_float4(__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u), __uint_as_float(r.y << 16),
                       __uint_as_float(r.y & 0xffff0000u));
}
__device__ __forceinline__ void st4(stin_bf16* p, float4 v) {
    stin_bf16x4 h = {(stin_bf16)v.x, (stin_bf16)v.y, (stin_bf16)v.z, (stin_bf16)v.w};
    *reinterpret_cast<stin_bf16x4*>(p) = h;
}
__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const stin_bf16* p) { return (float)*p; }
__device__ __forceinline__ void st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void st1(stin_bf16* p, float v) { *p = (stin_bf16)v; }

// 4-channel vector access needs 16-byte (fp32) / 8-byte (bf16) aligned rows
template <typename T> static inline bool stin_aligned_vec4(const void* p) {
    return (reinterpret_cast<uintptr_t>(p) & (4 * sizeof(T) - 1)) == 0;
}

// ---- weight-gradient (TN) products shared between stin_gemm.hip and stin_wgrad.hip ------------------------------------
// One dW[Nc, K (+1)] = G[M, Nc]^T [X[M, K] | w] product split over row chunks: its geometry and operands as the TN kernels
// take them.  Pointers are typed float* also for bf16 storage (only the fp32 kernels read them through this struct).
// Operand transform of the SingleConvMeshNet products (round 5): the operand rows are read as relu(bn(v)) per column - BatchNorm1d
// + ReLU of the E x 2 cout edge rows applied while the GEMM stages them, so that the normalised matrix never exists in memory
// (stin_gemm_nt_bn_f32: the A operand; stin_gemm_tn_bn_f32: the X operand).  mean == NULL: off.
// The staging threads of these kernels are bound by vector-ALU work (the 16-bit split), so the transform is the affine form
//   relu(v s + t),  s = gamma rstd,  t = beta - mean s        (mul, add, max: 3 operations per element)
// with (s, t) formed once per thread for its fixed columns - not stin_bn_act_fwd_f32's gamma ((v - mean) rstd) + beta (6
// operations; measured +80 % on the four-wave TN kernel, +50 % on the producer / consumer kernel).  The two agree to fp32 rounding
// (~1e-7 relative); forward product and weight gradient use the SAME form, so they stay consistent with each other.
struct stin_bn_tf {
    const float *mean, *rstd, *gamma, *beta;
};
__device__ __forceinline__ void stin_bn_st(const stin_bn_tf& tf, int c, float& s, float& t) {
    s = tf.gamma[c] * tf.rstd[c];
    t = tf.beta[c] - tf.mean[c] * s;
}
__device__ __forceinline__ float stin_bn_relu(float v, float s, float t) { return fmaxf(v * s + t, 0.f); }
// (s, t) of columns [c, c + 4) in registers (a staging thread's columns are fixed: formed once)
struct stin_bn_coef4 {
    float4 s, t;
};
__device__ __forceinline__ stin_bn_coef4 stin_bn_coef4_load(const stin_bn_tf& tf, int c) {
    stin_bn_coef4 q;
    stin_bn_st(tf, c, q.s.x, q.t.x);
    stin_bn_st(tf, c + 1, q.s.y, q.t.y);
    stin_bn_st(tf, c + 2, q.s.z, q.t.z);
    stin_bn_st(tf, c + 3, q.s.w, q.t.w);
    return q;
}
__device__ __forceinline__ float4 stin_bn_relu4(float4 v, const stin_bn_coef4& q) {
    return make_float4(stin_bn_relu(v.x, q.s.x, q.t.x), stin_bn_relu(v.y, q.s.y, q.t.y), stin_bn_relu(v.z, q.s.z, q.t.z),
                       stin_bn_relu(v.w, q.s.w, q.t.w));
}
// ragged / unaligned form: element e of the float4 is column c + e, valid while c + e < lim
__device__ __forceinline__ float4 stin_bn_relu4_ragged(float4 v, const stin_bn_tf& tf, int c, int lim) {
    float s, t;
    if (c + 0 < lim) { stin_bn_st(tf, c, s, t); v.x = stin_bn_relu(v.x, s, t); }
    if (c + 1 < lim) { stin_bn_st(tf, c + 1, s, t); v.y = stin_bn_relu(v.y, s, t); }
    if (c + 2 < lim) { stin_bn_st(tf, c + 2, s, t); v.z = stin_bn_relu(v.z, s, t); }
    if (c + 3 < lim) { stin_bn_st(tf, c + 3, s, t); v.w = stin_bn_relu(v.w, s, t); }
    return v;
}

struct stin_tn_problem {
    stin_bn_tf xtf;                    // transform of the X operand (mean == NULL: none)
    const float *G, *X, *row_w;
    float* slab;                       // [chunks][Nc * Kq + roundup4(Nc)] partial results
    int64_t ldg, ldx, ld_w, M, chunks;
    int Nc, K, Kq, has_bias, rows_per_chunk, tiles_i, tiles_j, vec;
    short TI, TJ;                      // tile (0, 64, 128, 256; host side only) - 16 bits each so that the record keeps its 152 bytes
    unsigned block0;                   // first block of the problem in a merged grid (set by stin_tn_ws_launch)
    const int32_t* x_row_map;          // optional, k_gemm_tn_ws<true> only: row m of the X operand is X[x_row_map[m]] (NULL: X[m])
};
static_assert(sizeof(stin_tn_problem) == 152, "stin_tn_problem is a kernel argument: k_gemm_tn_ws indexes batch.p[] by this stride");
struct stin_tn_batch {
    stin_tn_problem p[2];
    int n;
};
// Block -> (row chunk, output tile) of every tiled TN kernel.  chunks >= 8: XCD x (blocks b = x mod 8; blockIdx % 8 is the observed
// XCD round-robin) owns the row chunks x, x + 8, ... - its tiles re-read the same rows from its own L2; the grid is rounded up to
// whole rounds of 8 chunks, false = a block past the last chunk (block-uniform).  Fewer chunks than XCDs (the wide layers: >= 64
// output tiles): plain order, so that every XCD gets tiles of every chunk.
__device__ __forceinline__ bool tn_block_map(int64_t b, int64_t chunks, int tiles, int64_t& chunk, int& tile) {
    const int64_t xcd = b % 8, q = b / 8;
    chunk = chunks >= 8 ? (q / tiles) * 8 + xcd : b / tiles;
    tile = (int)(chunks >= 8 ? q % tiles : b % tiles);
    return chunk < chunks;
}

// One chunk-lane's share of a fixed-order fold over `chunks` rows of stride `cs` floats: 16 chunk-lanes x 16 float4 groups per block,
// lane ty of FN_KL walks rows ty, ty + FN_KL, ...; four running sums, merged (s0 + s1) + (s2 + s3); the caller adds the lanes in
// order through LDS.  THE fold of k_reduce_slabs, k_wgrad_finalize and k_colsum_fold: one body, so all three give the same bits.
constexpr int FN_COLS = 16, FN_KL = 16;
__device__ __forceinline__ void add4(float4& a, const float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
__device__ __forceinline__ float4 fn_partial(const float* __restrict__ p, int64_t cs, int64_t chunks, int ty) {
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0, s2 = s0, s3 = s0;
    if (p != nullptr) {
        int64_t c = ty;
        // (round 4) sixteen slab loads in flight per thread where the chunk list is long (the first block's skinny product
        // writes ~900 chunks: with four in flight this fold is 14-28 dependent trips to the fabric - 200 us at the very end of
        // the backward pass under rocprofv3, 11 us now; stand-alone and in the un-profiled step the difference is small); the
        // additions keep the order of the four-at-a-time loop below: bit-identical sums
        for (; c + 15 * FN_KL < chunks; c += 16 * FN_KL) {
            float4 v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = ld4(p + (c + u * FN_KL) * cs);
#pragma unroll
            for (int u = 0; u < 16; u += 4) {
                add4(s0, v[u]);
                add4(s1, v[u + 1]);
                add4(s2, v[u + 2]);
                add4(s3, v[u + 3]);
            }
        }
        for (; c + 3 * FN_KL < chunks; c += 4 * FN_KL) {
            add4(s0, ld4(p + c * cs));
            add4(s1, ld4(p + (c + FN_KL) * cs));
            add4(s2, ld4(p + (c + 2 * FN_KL) * cs));
            add4(s3, ld4(p + (c + 3 * FN_KL) * cs));
        }
        for (; c < chunks; c += FN_KL) add4(s0, ld4(p + c * cs));
    }
    add4(s0, s1);
    add4(s2, s3);
    add4(s0, s2);
    return s0;
}

// ---- which kernel runs a TN product.  The records live here because two translation units use them; the rules are compiled once,
// in stin_gemm.hip (csrc/gemm_tn_route.inc), and stin_wgrad.hip asks them through the functions below.
struct TnSwitches {
    bool pc;                   // STIN_TN_WS=0: never the producer / consumer kernel (the four-wave kernel on the tiles of the width rule)
    int big, tr;               // STIN_TN_BIG / STIN_TN_TR = 0 | 1 force the 256 x 256 tile / the transposed-read kernel of bf16 rows, -1 (unset) = the rule
};
struct TnProblem {
    int storage;               // 0 = fp32 rows, 1 = bf16 rows
    int64_t M;
    int Nc, K;
    int64_t ldg, ldx;          // row pitches of G and X, in elements
    int precision;             // STIN_GEMM_F32 / _BF16X3 / _BF16X6 (bf16 rows: _BF16X3)
    bool ones_column;          // a bias-gradient column [X | w]
    bool aligned16;            // the bases of G and X are 16-byte aligned
    bool bn_tf;                // X is read as relu(bn(X)) (stin_gemm_tn_bn_f32) ...
    bool bn_tf_aligned16;      // ... and its four vectors are 16-byte aligned
    bool x_row_map;            // row m of X is X[x_row_map[m]] (stin_edgeconv_wgrad_map)
};
struct TnRoute {
    int status;                // STIN_OK, or why this call cannot be served
    int family;                // STIN_TN_FAMILY_* (stin_hip.h); _NONE: no rows, only the fold is launched
    int TI, TJ;                // output tile of a block (0, 0: the skinny kernel, whose block owns all columns)
    int tiles_i, tiles_j, rows_per_chunk;
    int64_t chunks;            // row chunks = partial slabs
    int Kq, vec;               // K rounded up to 4 (the slab's row pitch); 16-byte operand loads
    int threads;
    int64_t lds, grid;         // dynamic LDS bytes; blocks
};
// stin_gemm.hip.  stin_tn_setup: the argument checks of one product, its route and its kernel argument (xtf / x_row_map: the
// optional transform of X and row map, NULL = none; they are part of what the route decides on).  stin_tn_slabs launches the TN
// kernels of one product or of two (pb != NULL) - partial slabs, no reduction: both on the producer / consumer kernel -> ONE grid,
// else one launch each.
TnSwitches stin_tn_switches();
TnRoute stin_tn_route(const TnProblem& p, const TnSwitches& sw);
int stin_tn_setup(stin_tn_problem* p, TnRoute* r, const TnSwitches& sw, int storage, const void* G, int64_t ldg, const void* X,
                  int64_t ldx, int64_t M, int Nc, int K, int ones_column, const void* row_w, int64_t ld_w, int precision, float* slab,
                  const stin_bn_tf* xtf, const int32_t* x_row_map);
int stin_tn_slabs(const stin_tn_problem* pa, const TnRoute* ra, const stin_tn_problem* pb, const TnRoute* rb, int precision,
                  stin_stream_t stream);
// stin_wgrad.hip: one or two (pb != NULL) products on the producer / consumer kernel, in one grid
int stin_tn_ws_launch(const stin_tn_problem* pa, const TnRoute* ra, const stin_tn_problem* pb, const TnRoute* rb, stin_stream_t stream);
