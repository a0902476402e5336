// Colour-map optimisation on the device: the photometric normal equations of every camera pose, for the rigid optimiser of
// preprocessing.optimize_poses_rigid (Zhou & Koltun 2014: the step Open3D's colour-map pipeline runs with maximum_iteration > 0).
// Contract: include/stin_hip.h ("Colour-map optimisation"); tests/_colormap_oracle.py restates it in numpy, pose-major, and agrees
// byte for byte.
//
//   gradients:  one workgroup per 64 x 16 tile of one frame: the tile's intensities G = 299 R + 587 G + 114 B and a halo of one
//               pixel (indices clamped to the image) through LDS, then the two Sobel responses; one 16-byte pixel (G, gx, gy, 0)
//               per thread and store, so that every bilinear tap of the sampling kernel is one 16-byte load.
//   proxy:      one thread per vertex, from the integer sums of stin_frames_accumulate_f64.
//   normal:     two kernels.  k_colormap_partial: one workgroup per (tile of 256 U vertices, chunk of poses).  Lanes run along the
//               vertices; a thread keeps its U vertices' coordinates, proxies and bit rows in registers over the chunk's poses, adds
//               the 28 terms of its pairs in registers (i ascending), and the 256 lane sums are folded once per (tile, pose) by the
//               contract's halving tree: the steps 128 and 64 through LDS, the steps 32 .. 1 inside wave 0 with shuffles - the same
//               pairs in the same order, and a + b is b + a.  A tile without a contributing pair for a pose writes its row of +0.0
//               without folding (a workgroup-uniform test).  k_colormap_fold: one thread per (pose, value), tiles ascending.
//               The pair test, the sampler and the Jacobian are stin_view.h's, shared with the frame colours and the non-rigid kernels.
// No float atomics; the order of every sum is a function of N alone.
#include "stin_view.h"

namespace {

constexpr int CB = 256;                                   // threads per workgroup = lanes of a tile
constexpr int U = STIN_COLORMAP_U;                        // vertices per lane and tile
constexpr int ROW = STIN_COLORMAP_ROW_DOUBLES;            // 21 + 6 + 1
constexpr int TW = 64, TH = 16;                           // gradient tile
constexpr int MIN_POSES = 8;                              // poses per chunk, at least

__global__ __launch_bounds__(CB) void k_colormap_gradients(const uint8_t* __restrict__ color, int H, int W, int4* __restrict__ images) {
    __shared__ int g[(TH + 2) * (TW + 2)];
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const uint8_t* src = color + (int64_t)blockIdx.z * H * W * 3;
    for (int t = threadIdx.x; t < (TH + 2) * (TW + 2); t += CB) {
        const int ty = t / (TW + 2), tx = t - ty * (TW + 2);
        int gy = y0 - 1 + ty, gx = x0 - 1 + tx;
        gy = gy < 0 ? 0 : (gy > H - 1 ? H - 1 : gy);
        gx = gx < 0 ? 0 : (gx > W - 1 ? W - 1 : gx);
        const uint8_t* p = src + ((int64_t)gy * W + gx) * 3;
        g[t] = 299 * (int)p[0] + 587 * (int)p[1] + 114 * (int)p[2];
    }
    __syncthreads();
    int4* dst = images + (int64_t)blockIdx.z * H * W;
    for (int t = threadIdx.x; t < TH * TW; t += CB) {
        const int ty = t / TW, tx = t - ty * TW;
        const int py = y0 + ty, px = x0 + tx;
        if (py >= H || px >= W) continue;
        const int* c = g + (ty + 1) * (TW + 2) + (tx + 1);
        const int ul = c[-(TW + 2) - 1], uc = c[-(TW + 2)], ur = c[-(TW + 2) + 1];
        const int cl = c[-1], cr = c[1];
        const int dl = c[(TW + 2) - 1], dc = c[TW + 2], dr = c[(TW + 2) + 1];
        const int sx = (ur + 2 * cr + dr) - (ul + 2 * cl + dl);
        const int sy = (dl + 2 * dc + dr) - (ul + 2 * uc + ur);
        dst[(int64_t)py * W + px] = make_int4(c[0], sx, sy, 0);
    }
}

__global__ __launch_bounds__(CB) void k_colormap_proxy(const int64_t* __restrict__ sum, const int32_t* __restrict__ count, int64_t N,
                                                       double* __restrict__ proxy) {
    const int64_t v = (int64_t)blockIdx.x * CB + threadIdx.x;
    if (v >= N) return;
    const int32_t n = count[v];
    double out = 0.0;
    if (n > 0) {
        const int64_t num = 299 * sum[3 * v] + 587 * sum[3 * v + 1] + 114 * sum[3 * v + 2];
        out = (double)num / ((double)n * 16711680000.0);
    }
    proxy[v] = out;
}

struct NormalArgs {
    const double* vertices;
    const double* RT;
    const uint8_t* valid;
    const int4* images;
    const uint32_t* bits;
    const double* proxy;
    double* part;                                         // [tiles][B][ROW]
    int32_t* part_n;                                      // [tiles][B]
    int64_t N, first_pose, words;
    View C;
    int B, H, W, per_chunk;
};

__global__ __launch_bounds__(CB) void k_colormap_partial(const NormalArgs A) {
    __shared__ double sh[ROW][128];
    __shared__ int shn[128];
    const int l = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * (CB * U);
    const int b0 = (int)blockIdx.y * A.per_chunk;
    const int b1 = b0 + A.per_chunk < A.B ? b0 + A.per_chunk : A.B;
    double x[U], y[U], z[U], px[U];
    const uint32_t* brow[U];
    bool live[U];
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int64_t v = base + l + (int64_t)CB * i;
        live[i] = v < A.N;
        const int64_t w = live[i] ? v : 0;                // a lane beyond N reads vertex 0 and contributes nothing
        x[i] = A.vertices[3 * w];
        y[i] = A.vertices[3 * w + 1];
        z[i] = A.vertices[3 * w + 2];
        px[i] = A.proxy[w];
        brow[i] = A.bits + w * A.words;
    }
    for (int b = b0; b < b1; ++b) {
        double acc[ROW];
#pragma unroll
        for (int k = 0; k < ROW; ++k) acc[k] = 0.0;
        int n = 0;
        if (A.valid[b]) {
            const int64_t p = A.first_pose + b;
            const double* m = A.RT + (int64_t)b * 12;
            const int4* img = A.images + (int64_t)b * A.H * A.W;
#pragma unroll
            for (int i = 0; i < U; ++i) {
                if (!live[i]) continue;
                if (!((brow[i][p >> 5] >> (p & 31)) & 1u)) continue;
                double xv, yv, zv, u, w, I, dIdx, dIdy, J[6];
                if (!view_transform(A.C, m, x[i], y[i], z[i], xv, yv, zv)) continue;
                if (!view_project(A.C.fx, A.C.fy, A.C.cx, A.C.cy, xv, yv, zv, u, w)) continue;
                if (!view_inside(A.C, u, w)) continue;
                sample_gradients(img, A.W, taps_of(u, w, A.H, A.W), I, dIdx, dIdy);   // margin >= 1: the taps are in [1, W - 2], [1, H - 2]
                const double r = I - px[i];
                pose_jacobian(xv, yv, zv, A.C.fx, A.C.fy, dIdx, dIdy, J);
                int k = 0;
#pragma unroll
                for (int i0 = 0; i0 < 6; ++i0)
#pragma unroll
                    for (int j0 = i0; j0 < 6; ++j0) acc[k++] += J[i0] * J[j0];
#pragma unroll
                for (int i0 = 0; i0 < 6; ++i0) acc[21 + i0] += J[i0] * r;
                acc[27] += r * r;
                n += 1;
            }
        }
        double* out = A.part + ((int64_t)blockIdx.x * A.B + b) * ROW;
        int32_t* out_n = A.part_n + (int64_t)blockIdx.x * A.B + b;
        if (!__syncthreads_or(n)) {                       // nobody in the tile contributes: the row of +0.0, unfolded
            if (l < ROW) out[l] = 0.0;
            if (l == ROW) *out_n = 0;
            continue;
        }
        if (l >= 128) {
#pragma unroll
            for (int k = 0; k < ROW; ++k) sh[k][l - 128] = acc[k];
            shn[l - 128] = n;
        }
        __syncthreads();
        if (l < 128) {
#pragma unroll
            for (int k = 0; k < ROW; ++k) acc[k] += sh[k][l];
            n += shn[l];
        }
        __syncthreads();
        if (l >= 64 && l < 128) {
#pragma unroll
            for (int k = 0; k < ROW; ++k) sh[k][l - 64] = acc[k];
            shn[l - 64] = n;
        }
        __syncthreads();
        if (l < 64) {
#pragma unroll
            for (int k = 0; k < ROW; ++k) acc[k] += sh[k][l];
            n += shn[l];
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
                for (int k = 0; k < ROW; ++k) acc[k] += __shfl_down(acc[k], s, 64);
                n += __shfl_down(n, s, 64);
            }
            if (l == 0) {
#pragma unroll
                for (int k = 0; k < ROW; ++k) out[k] = acc[k];
                *out_n = n;
            }
        }
    }
}

__global__ __launch_bounds__(CB) void k_colormap_fold(const double* __restrict__ part, const int32_t* __restrict__ part_n, int64_t tiles,
                                                      int B, double* __restrict__ rows, int32_t* __restrict__ counts) {
    const int64_t t = (int64_t)blockIdx.x * CB + threadIdx.x;
    if (t >= (int64_t)B * (ROW + 1)) return;
    const int b = (int)(t / (ROW + 1)), k = (int)(t - (int64_t)b * (ROW + 1));
    if (k < ROW) {
        double s = 0.0;
        for (int64_t tile = 0; tile < tiles; ++tile) s += part[(tile * B + b) * ROW + k];
        rows[(int64_t)b * ROW + k] = s;
    } else {
        int32_t s = 0;
        for (int64_t tile = 0; tile < tiles; ++tile) s += part_n[tile * B + b];
        counts[b] = s;
    }
}

inline int64_t tiles_of(int64_t N) { return (N + (int64_t)CB * U - 1) / ((int64_t)CB * U); }

}  // namespace

extern "C" int stin_colormap_gradients_u8(const uint8_t* color, int B, int H, int W, int32_t* images, stin_stream_t stream_) {
    STIN_REQUIRE(B >= 0 && B <= STIN_FRAMES_MAX_BATCH && frame_size_ok(H, W, 1), STIN_E_SIZE);
    if (B == 0) return STIN_OK;
    STIN_REQUIRE(color != nullptr && images != nullptr, STIN_E_NULL);
    STIN_REQUIRE(((uintptr_t)images & 15u) == 0, STIN_E_SIZE);
    stin_clear_stale_error();
    hipLaunchKernelGGL(k_colormap_gradients, dim3((unsigned)((W + TW - 1) / TW), (unsigned)((H + TH - 1) / TH), (unsigned)B), dim3(CB), 0,
                       (hipStream_t)stream_, color, H, W, (int4*)images);
    return stin_launch_status();
}

extern "C" int stin_colormap_proxy_f64(const int64_t* sum, const int32_t* count, int64_t N, double* proxy, stin_stream_t stream_) {
    STIN_REQUIRE(N >= 0 && N < (int64_t)INT32_MAX, STIN_E_SIZE);
    if (N == 0) return STIN_OK;
    STIN_REQUIRE(sum != nullptr && count != nullptr && proxy != nullptr, STIN_E_NULL);
    stin_clear_stale_error();
    hipLaunchKernelGGL(k_colormap_proxy, dim3((unsigned)((N + CB - 1) / CB)), dim3(CB), 0, (hipStream_t)stream_, sum, count, N, proxy);
    return stin_launch_status();
}

extern "C" size_t stin_colormap_workspace_bytes(int64_t N, int B) {
    if (N < 0 || N >= (int64_t)INT32_MAX || B < 0 || B > STIN_FRAMES_MAX_BATCH) return 0;
    const size_t cells = (size_t)(N > 0 ? tiles_of(N) : 1) * (size_t)(B > 0 ? B : 1);
    return stin_up256(cells * ROW * sizeof(double)) + stin_up256(cells * sizeof(int32_t));
}

extern "C" int stin_colormap_normal_f64(const double* vertices, int64_t N, const double* RT, const uint8_t* valid, int B,
                                        int64_t first_pose, const int32_t* images, int H, int W, const double* camera, double z_near,
                                        const uint32_t* bits, int64_t words, int margin, const double* proxy, double* rows,
                                        int32_t* counts, void* workspace, size_t workspace_bytes, stin_stream_t stream_) {
    STIN_REQUIRE(camera != nullptr, STIN_E_NULL);
    STIN_REQUIRE(N >= 0 && N < (int64_t)INT32_MAX && B >= 0 && B <= STIN_FRAMES_MAX_BATCH, STIN_E_SIZE);
    STIN_REQUIRE(first_pose >= 0 && first_pose + B < (int64_t)INT32_MAX, STIN_E_SIZE);
    STIN_REQUIRE(frame_size_ok(H, W, 1) && margin >= 1 && z_near > 0.0, STIN_E_SIZE);
    STIN_REQUIRE(words >= (first_pose + B + 31) / 32 || N == 0 || B == 0, STIN_E_SIZE);
    if (B == 0) return STIN_OK;
    STIN_REQUIRE(rows != nullptr && counts != nullptr, STIN_E_NULL);
    hipStream_t stream = (hipStream_t)stream_;
    stin_clear_stale_error();
    const int64_t tiles = N > 0 ? tiles_of(N) : 0;
    double* part = (double*)workspace;
    int32_t* part_n = nullptr;
    if (N > 0) {
        STIN_REQUIRE(vertices && RT && valid && images && bits && proxy, STIN_E_NULL);
        STIN_REQUIRE(((uintptr_t)images & 15u) == 0, STIN_E_SIZE);
        STIN_REQUIRE(workspace != nullptr && workspace_bytes >= stin_colormap_workspace_bytes(N, B), STIN_E_WORKSPACE);
        part_n = (int32_t*)((char*)workspace + stin_up256((size_t)tiles * B * ROW * sizeof(double)));
        NormalArgs A;
        A.vertices = vertices; A.RT = RT; A.valid = valid; A.images = (const int4*)images; A.bits = bits; A.proxy = proxy;
        A.part = part; A.part_n = part_n;
        A.N = N; A.first_pose = first_pose; A.words = words;
        A.C = view_of(camera, z_near, margin, H, W);
        A.B = B; A.H = H; A.W = W;
        const PoseChunks ch = pose_chunks(tiles, B, MIN_POSES, STIN_FRAMES_ROUTE_AUTO);   // every (tile, pose) has its own row: no split to handle
        A.per_chunk = ch.per_chunk;
        hipLaunchKernelGGL(k_colormap_partial, dim3((unsigned)tiles, ch.count), dim3(CB), 0, stream, A);
    }
    hipLaunchKernelGGL(k_colormap_fold, dim3((unsigned)(((int64_t)B * (ROW + 1) + CB - 1) / CB)), dim3(CB), 0, stream, part, part_n, tiles, B,
                       rows, counts);
    return stin_launch_status();
}
