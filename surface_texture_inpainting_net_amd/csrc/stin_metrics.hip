// The seven per-step metrics of the inpainting trainer (trainers/inpainting3d_trainer.py:254-271) in one call: loss, l1, mse,
// graph_tv, graph_lap_var, psnr, psnr_mask_only - and the masked-row count - written as one row of 8 floats into a caller-owned
// device table.  No host synchronisation, no allocation, no float atomics: every sum is an fp64 block partial written to the
// workspace and folded in a fixed order by the finaliser, so two runs on the same inputs give the same bits.
//
//   P = composite ? where(mask > 0, out, color) : out         G = color         d = P - G
//
// Two layouts of the same arithmetic (the same per-row values, the same block partition -> the same bits):
//   STIN_METRICS_ONE_PASS  one kernel: every neighbour visit gathers out / color / mask of the neighbour and rebuilds its P row
//                          (12 + 12 + 8 = 32 bytes per edge), then the finaliser: 2 launches;
//   STIN_METRICS_STAGED    a row pass writes (P_r, P_g, P_b, gray) of every vertex as one float4 into the workspace - in CSR row
//                          order, so a locality-ordered plan's rows lie next to each other whatever the caller's vertex order - and
//                          the edge pass gathers 16 aligned bytes per edge, then the finaliser: 3 launches.
#include "stin_common.h"

#include <math.h>

namespace {
constexpr int MB = 256;                   // threads per block = rows per block
enum { Q_ABS, Q_WABS, Q_SQ, Q_SQ_IN, Q_CNT_IN, Q_TV, Q_LAP, Q_LAP2, NQ };

// partial[(q0 + k) * blocks + blockIdx.x] = sum over the block of acc[k]: lanes by shuffle, the four waves in a fixed order
template <int K>
__device__ __forceinline__ void block_partials(const double (&acc)[K], int q0, double* __restrict__ partial, int64_t blocks) {
    __shared__ double sm[K][MB / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = stin_wave_sum(acc[k]);
        if (lane == 0) sm[k][wave] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < K) {
        const int k = threadIdx.x;
        partial[(int64_t)(q0 + k) * blocks + blockIdx.x] = (sm[k][0] + sm[k][1]) + (sm[k][2] + sm[k][3]);
    }
}

// (P_0, P_1, P_2, gray) of vertex v; channels beyond C are zero, gray is 0.299 R + 0.587 G + 0.114 B as torch evaluates it
template <int C>
__device__ __forceinline__ float4 pred_row(const float* __restrict__ out, int64_t ldo, const float* __restrict__ color,
                                           const int64_t* __restrict__ mask, int64_t v, int composite) {
    float p[3] = {0.f, 0.f, 0.f};
    const bool keep = composite && !(mask[v] > 0);
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = keep ? color[v * C + c] : out[v * ldo + c];
    const float gray = C == 3 ? (0.299f * p[0] + 0.587f * p[1]) + 0.114f * p[2] : 0.f;
    return make_float4(p[0], p[1], p[2], gray);
}

// one in-edge j -> i: the edge's total-variation term (fp32 over the channels, as k_total_variation forms it) and the neighbour's
// gray value added to the row's running fp32 sum in edge order (as k_graph_laplace forms it)
__device__ __forceinline__ void edge_terms(const float4 pi, const float4 pj, double& tv, float& lap) {
    float s = 0.f;
    s += fabsf(pj.x - pi.x);
    s += fabsf(pj.y - pi.y);
    s += fabsf(pj.z - pi.z);
    tv += (double)s;
    lap += pj.w;
}

// Row terms of vertex r (CSR order; the caller's row perm[r]).  ONE_PASS: also the edge terms, every neighbour rebuilt from
// out / color / mask; otherwise the row is staged for k_metrics_edges.
template <int C, bool ONE_PASS>
__global__ __launch_bounds__(MB) void k_metrics_rows(const float* __restrict__ out, int64_t ldo, const float* __restrict__ color,
                                                     const int64_t* __restrict__ mask, const int32_t* __restrict__ rowptr,
                                                     const int32_t* __restrict__ col, const int32_t* __restrict__ perm, int64_t N,
                                                     int composite, int use_weight, float4* __restrict__ stage,
                                                     double* __restrict__ partial, int64_t blocks) {
    constexpr int K = ONE_PASS ? (int)NQ : (int)Q_TV;
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    const int64_t r = (int64_t)blockIdx.x * MB + threadIdx.x;
    if (r < N) {
        const int64_t v = perm ? (int64_t)perm[r] : r;
        const int64_t m = mask[v];
        const bool inside = m > 0;
        const float w = use_weight ? powf(0.99f, (float)m) : 1.f;
        const float4 pi = pred_row<C>(out, ldo, color, mask, v, composite);
        const float p[3] = {pi.x, pi.y, pi.z};
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float d = p[c] - color[v * C + c];
            const float a = fabsf(d), q = d * d;
            acc[Q_ABS] += (double)a;
            acc[Q_WABS] += (double)(a * w);
            acc[Q_SQ] += (double)q;
            if (inside) acc[Q_SQ_IN] += (double)q;
        }
        if (inside) acc[Q_CNT_IN] = 1.0;
        if constexpr (ONE_PASS) {
            const int beg = rowptr[r], end = rowptr[r + 1];
            double tv = 0.0;
            float lap = 0.f;
            for (int e = beg; e < end; ++e) {
                const int64_t j = col[e];
                if ((uint64_t)j >= (uint64_t)N) continue;                // (a valid CSR never has one)
                const int64_t u = perm ? (int64_t)perm[j] : j;
                edge_terms(pi, pred_row<C>(out, ldo, color, mask, u, composite), tv, lap);
            }
            const float L = lap - (float)(end - beg) * pi.w;
            acc[Q_TV] = tv;
            acc[Q_LAP] = (double)L;
            acc[Q_LAP2] = (double)L * (double)L;
        } else {
            stage[r] = pi;
        }
    }
    block_partials<K>(acc, 0, partial, blocks);
}

__global__ __launch_bounds__(MB) void k_metrics_edges(const float4* __restrict__ stage, const int32_t* __restrict__ rowptr,
                                                      const int32_t* __restrict__ col, int64_t N, double* __restrict__ partial,
                                                      int64_t blocks) {
    double acc[3] = {0.0, 0.0, 0.0};
    const int64_t r = (int64_t)blockIdx.x * MB + threadIdx.x;
    if (r < N) {
        const float4 pi = stage[r];
        const int beg = rowptr[r], end = rowptr[r + 1];
        double tv = 0.0;
        float lap = 0.f;
        for (int e = beg; e < end; ++e) {
            const int64_t j = col[e];
            if ((uint64_t)j >= (uint64_t)N) continue;
            edge_terms(pi, stage[j], tv, lap);
        }
        const float L = lap - (float)(end - beg) * pi.w;
        acc[0] = tv;
        acc[1] = (double)L;
        acc[2] = (double)L * (double)L;
    }
    block_partials<3>(acc, Q_TV, partial, blocks);
}

// wave q folds quantity q's block partials (lane-strided, then the shuffle tree: a fixed order); the divisions, the log10 and the
// variance in double; eight lanes store the row
__global__ __launch_bounds__(64 * NQ) void k_metrics_final(const double* __restrict__ partial, int64_t blocks, int64_t N, int C,
                                                           float data_range, const float* __restrict__ loss_in,
                                                           float* __restrict__ row_out) {
    __shared__ double sums[NQ];
    __shared__ float vals[8];
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    double s = 0.0;
    for (int64_t i = lane; i < blocks; i += 64) s += partial[(int64_t)q * blocks + i];
    s = stin_wave_sum(s);
    if (lane == 0) sums[q] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double n = (double)N * (double)C, r2 = (double)data_range * (double)data_range;
        const double mse = sums[Q_SQ] / n;
        const double mse_in = sums[Q_SQ_IN] / (sums[Q_CNT_IN] * (double)C);          // no masked row: 0 / 0 = NaN, as the reference
        const double mean_l = sums[Q_LAP] / (double)N;
        double var = sums[Q_LAP2] / (double)N - mean_l * mean_l;
        if (var < 0.0) var = 0.0;                                                    // (a NaN stays a NaN)
        vals[0] = loss_in ? loss_in[0] : (float)(sums[Q_WABS] / n);
        vals[1] = (float)(sums[Q_ABS] / n);
        vals[2] = (float)mse;
        vals[3] = (float)(sums[Q_TV] / n);
        vals[4] = C == 3 ? (float)var : __builtin_nanf("");
        vals[5] = (float)(-10.0 * log10(mse / r2 + 1e-8));
        vals[6] = (float)(-10.0 * log10(mse_in / r2 + 1e-8));
        vals[7] = (float)sums[Q_CNT_IN];
    }
    __syncthreads();
    if (threadIdx.x < 8) row_out[threadIdx.x] = vals[threadIdx.x];
}

inline int64_t n_blocks(int64_t N) { return (N + MB - 1) / MB; }
}  // namespace

extern "C" size_t stin_inpaint_metrics_workspace_bytes(int64_t N) {
    if (N <= 0) return 0;
    return 256 + stin_up256((size_t)NQ * (size_t)n_blocks(N) * sizeof(double)) + (size_t)N * sizeof(float4);
}

extern "C" int stin_inpaint_metrics_f32(const float* out, int64_t ldo, const float* color, const int64_t* mask,
                                        const int32_t* rowptr_dst, const int32_t* col_dst, const int32_t* perm, int64_t N, int C,
                                        int composite, int use_weight, float data_range, const float* loss, int layout,
                                        float* row_out, void* workspace, size_t workspace_bytes, stin_stream_t stream_) {
    stin_clear_stale_error();
    STIN_REQUIRE(N > 0 && N <= ((int64_t)1 << 24) && (C == 1 || C == 3) && ldo >= C && data_range > 0.f, STIN_E_SIZE);
    STIN_REQUIRE(layout == STIN_METRICS_ONE_PASS || layout == STIN_METRICS_STAGED, STIN_E_UNSUPPORTED);
    STIN_REQUIRE(out && color && mask && rowptr_dst && col_dst && row_out && workspace, STIN_E_NULL);
    STIN_REQUIRE(workspace_bytes >= stin_inpaint_metrics_workspace_bytes(N), STIN_E_WORKSPACE);
    const int64_t blocks = n_blocks(N);
    char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    double* partial = reinterpret_cast<double*>(base);
    float4* stage = reinterpret_cast<float4*>(base + stin_up256((size_t)NQ * (size_t)blocks * sizeof(double)));
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((unsigned)blocks), block(MB);
#define STIN_METRICS_ROWS(C_, ONE_)                                                                                              \
    hipLaunchKernelGGL((k_metrics_rows<C_, ONE_>), grid, block, 0, stream, out, ldo, color, mask, rowptr_dst, col_dst, perm, N, \
                       composite, use_weight, stage, partial, blocks)
    if (layout == STIN_METRICS_ONE_PASS) {
        if (C == 3) STIN_METRICS_ROWS(3, true);
        else STIN_METRICS_ROWS(1, true);
    } else {
        if (C == 3) STIN_METRICS_ROWS(3, false);
        else STIN_METRICS_ROWS(1, false);
        hipLaunchKernelGGL(k_metrics_edges, grid, block, 0, stream, stage, rowptr_dst, col_dst, N, partial, blocks);
    }
#undef STIN_METRICS_ROWS
    hipLaunchKernelGGL(k_metrics_final, dim3(1), dim3(64 * NQ), 0, stream, partial, blocks, N, C, data_range, loss, row_out);
    return stin_launch_status();
}
