// Frame colours on the device: per-vertex colours of a mesh from a scan's RGB-D frames and camera trajectory (reference
// preprocessing/texture_map_optimization.py, which hands the job to Open3D's colour-map pipeline with maximum_iteration = 0).
// Contract: include/stin_hip.h ("Frame colours"); tests/_frames_oracle.py restates it in numpy, pose-major, and agrees bit for bit.
//
//   edges:      per batch of depth frames, two passes.  k_frames_edge0: one thread per pixel, the 3 x 3 Sobel pair on the truncated
//               raw values in integers, the test against T T, one byte into the workspace.  k_frames_dilate: one workgroup per
//               64 x 16 tile, the tile and its halo of k through LDS, OR along the rows, then along the columns.
//   accumulate: one thread per vertex (lanes along the vertices: the vertex reads coalesce, a pose's twelve numbers are
//               wave-uniform), a loop over a chunk of the batch's poses, three int64 sums and a count in registers.
//               Owner route: the chunk is the whole batch, the thread adds to its vertex's row with plain loads and stores.
//               Split route (few vertices, many poses): blockIdx.y picks the chunk, every value is added with one integer atomicAdd.
//               One kernel template, three visibility modes: the depth test, observer bits, and bits with the colour frame sampled
//               at the position a warp lattice moves the projection to (stin_nonrigid_accumulate_f64, the colour pass of the
//               non-rigid optimiser, defined here beside the kernel it launches).  The pair test and the sampler are stin_view.h's.
//   finish:     one thread per vertex.
// "raw / depth_scale > depth_trunc" is monotone in raw for depth_scale > 0: the host finds the largest raw value that stays (a
// binary search with the contract's own expression) and the kernels compare integers.
// Integer sums and integer atomics only: the result does not depend on the schedule, the route or the batching.
#include "stin_view.h"

namespace {

constexpr int FB = 256;                                   // threads per workgroup
constexpr int TW = 64, TH = 16;                           // dilation tile
constexpr int KMAX = STIN_FRAMES_MAX_HALF_KERNEL;
constexpr int SPLIT_MIN_POSES = 8;                        // poses per chunk of the split route, at least

// The largest raw value r with !((double)r / depth_scale > depth_trunc); -1: none stays, 65535: all stay (also for a NaN limit).
int keep_max_raw(double depth_scale, double depth_trunc) {
    int lo = -1, hi = 65535;                              // predicate "stays" holds on [0, lo], fails above hi
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if ((double)mid / depth_scale > depth_trunc) hi = mid - 1; else lo = mid;
    }
    return lo;
}

__device__ inline int trunc_raw(const uint16_t* __restrict__ d, int i, int j, int W, int keep_max) {
    const int r = d[(int64_t)i * W + j];
    return r > keep_max ? 0 : r;
}

__global__ __launch_bounds__(FB) void k_frames_edge0(const uint16_t* __restrict__ depth, int H, int W, int keep_max, double TT,
                                                      uint8_t* __restrict__ edge0) {
    const int64_t pix = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (pix >= (int64_t)H * W) return;
    const int i = (int)(pix / W), j = (int)(pix % W);
    const uint16_t* d = depth + (int64_t)blockIdx.y * H * W;
    const int iu = i > 0 ? i - 1 : 0, id = i < H - 1 ? i + 1 : H - 1;
    const int jl = j > 0 ? j - 1 : 0, jr = j < W - 1 ? j + 1 : W - 1;
    const int ul = trunc_raw(d, iu, jl, W, keep_max), uc = trunc_raw(d, iu, j, W, keep_max), ur = trunc_raw(d, iu, jr, W, keep_max);
    const int cl = trunc_raw(d, i, jl, W, keep_max), cr = trunc_raw(d, i, jr, W, keep_max);
    const int dl = trunc_raw(d, id, jl, W, keep_max), dc = trunc_raw(d, id, j, W, keep_max), dr = trunc_raw(d, id, jr, W, keep_max);
    const int64_t gx = (int64_t)(ur + 2 * cr + dr) - (int64_t)(ul + 2 * cl + dl);
    const int64_t gy = (int64_t)(dl + 2 * dc + dr) - (int64_t)(ul + 2 * uc + ur);
    edge0[(int64_t)blockIdx.y * H * W + pix] = (double)(gx * gx + gy * gy) > TT ? 1 : 0;
}

__global__ __launch_bounds__(FB) void k_frames_dilate(const uint8_t* __restrict__ edge0, int H, int W, int k, uint8_t* __restrict__ edge) {
    __shared__ uint8_t tile[(TH + 2 * KMAX) * (TW + 2 * KMAX)];
    __shared__ uint8_t rows[(TH + 2 * KMAX) * TW];
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int tw = TW + 2 * k, th = TH + 2 * k;
    const uint8_t* src = edge0 + (int64_t)blockIdx.z * H * W;
    for (int t = threadIdx.x; t < th * tw; t += FB) {
        const int ty = t / tw, tx = t - ty * tw;
        const int gy = y0 - k + ty, gx = x0 - k + tx;
        tile[t] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? src[(int64_t)gy * W + gx] : 0;   // outside the image: not in the window
    }
    __syncthreads();
    for (int t = threadIdx.x; t < th * TW; t += FB) {
        const int ty = t / TW, tx = t - ty * TW;
        const uint8_t* r = tile + ty * tw + tx;
        uint8_t any = 0;
        for (int o = 0; o <= 2 * k; ++o) any |= r[o];
        rows[t] = any;
    }
    __syncthreads();
    uint8_t* dst = edge + (int64_t)blockIdx.z * H * W;
    for (int t = threadIdx.x; t < TH * TW; t += FB) {
        const int ty = t / TW, tx = t - ty * TW;
        const int gy = y0 + ty, gx = x0 + tx;
        if (gy >= H || gx >= W) continue;
        uint8_t any = 0;
        for (int o = 0; o <= 2 * k; ++o) any |= rows[(ty + o) * TW + tx];
        dst[(int64_t)gy * W + gx] = any ? 1 : 0;
    }
}

enum AccMode { ACC_DEPTH, ACC_BITS, ACC_WARP };           // visibility from the depth frames; from bits; from bits, sampled at the warped position

struct FrameArgs {
    const double* vertices;
    const double* RT;
    const uint8_t* valid;
    const uint8_t* color;
    const uint16_t* depth;
    const uint8_t* edge;
    const uint32_t* bits;
    const double* flow;                                   // ACC_WARP: [B][Ah][Aw][2]
    int64_t* sum;
    int32_t* count;
    uint32_t* seen;
    int64_t N, first_pose, words, seen_words;
    View C;                                               // the colour camera and frame
    double dfx, dfy, dcx, dcy;
    double depth_scale, max_depth, depth_threshold;
    int B, Hc, Wc, Hd, Wd, keep_max, per_chunk;
};

template <AccMode MODE, bool ATOMIC> __global__ __launch_bounds__(FB) void k_frames_accumulate(const FrameArgs A) {
    const int64_t v = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (v >= A.N) return;
    const int b0 = (int)blockIdx.y * A.per_chunk;
    const int b1 = b0 + A.per_chunk < A.B ? b0 + A.per_chunk : A.B;
    const double x = A.vertices[3 * v], y = A.vertices[3 * v + 1], z = A.vertices[3 * v + 2];
    const uint32_t* brow = MODE == ACC_DEPTH ? nullptr : A.bits + v * A.words;
    const int64_t per_flow = (int64_t)A.C.Ah * A.C.Aw * 2;
    int64_t s0 = 0, s1 = 0, s2 = 0;
    int32_t cnt = 0;
    uint32_t sacc = 0u;
    int64_t sword = 0;
    for (int b = b0; b < b1; ++b) {
        if (!A.valid[b]) continue;
        const int64_t p = A.first_pose + b;
        if (MODE != ACC_DEPTH && !((brow[p >> 5] >> (p & 31)) & 1u)) continue;
        double xv, yv, zv, u, w;
        if (!view_transform(A.C, A.RT + (int64_t)b * 12, x, y, z, xv, yv, zv)) continue;
        if (!view_project(A.C.fx, A.C.fy, A.C.cx, A.C.cy, xv, yv, zv, u, w)) continue;
        if (MODE == ACC_DEPTH) {
            double ud, vd;
            if (!view_project(A.dfx, A.dfy, A.dcx, A.dcy, xv, yv, zv, ud, vd)) continue;
            const double ui = rint(ud), vi = rint(vd);
            if (!(ui >= 0.0 && ui < (double)A.Wd && vi >= 0.0 && vi < (double)A.Hd)) continue;
            const int64_t at = ((int64_t)b * A.Hd + (int64_t)vi) * A.Wd + (int64_t)ui;
            const int rr = A.depth[at];
            if (rr == 0 || rr > A.keep_max) continue;
            const double d = (double)rr / A.depth_scale;
            if (d > A.max_depth) continue;
            if (A.edge[at]) continue;
            if (!(fabs(zv - d) < A.depth_threshold)) continue;
        }
        if (!view_inside(A.C, u, w)) continue;
        if (MODE == ACC_WARP) {
            double wts[4], uw, vw;
            int cell;
            if (!view_warp(A.C, A.flow + (int64_t)b * per_flow, u, w, wts, uw, vw, cell)) continue;
            u = uw;
            w = vw;
        }
        int64_t q[3];
        sample_rgb(A.color + (int64_t)b * A.Hc * A.Wc * 3, A.Wc, taps_of(u, w, A.Hc, A.Wc), q);
        s0 += q[0];
        s1 += q[1];
        s2 += q[2];
        cnt += 1;
        if (A.seen != nullptr) seen_mark<ATOMIC>(A.seen + v * A.seen_words, p, sword, sacc);
    }
    if (cnt == 0) return;
    if (A.seen != nullptr) seen_flush<ATOMIC>(A.seen + v * A.seen_words, sword, sacc);
    sums_commit<ATOMIC>(A.sum + 3 * v, A.count + v, s0, s1, s2, cnt);
}

__global__ void k_frames_finish(const int64_t* __restrict__ sum, const int32_t* __restrict__ count, int64_t N, float f0, float f1,
                                float f2, float* __restrict__ colors, uint8_t* __restrict__ observed) {
    const int64_t v = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (v >= N) return;
    const int32_t n = count[v];
    if (observed != nullptr) observed[v] = n > 0 ? 1 : 0;
    if (colors == nullptr) return;
    if (n > 0) {
        const double den = (double)n * 16711680.0;
        colors[3 * v] = (float)((double)sum[3 * v] / den);
        colors[3 * v + 1] = (float)((double)sum[3 * v + 1] / den);
        colors[3 * v + 2] = (float)((double)sum[3 * v + 2] / den);
    } else {
        colors[3 * v] = f0;
        colors[3 * v + 1] = f1;
        colors[3 * v + 2] = f2;
    }
}

// The route, from N and B alone (pose_chunks), and the instantiation of (mode, split); fills A.per_chunk.
int launch_accumulate(FrameArgs& A, AccMode mode, int route, hipStream_t stream) {
    const int64_t groups = (A.N + FB - 1) / FB;
    const PoseChunks ch = pose_chunks(groups, A.B, SPLIT_MIN_POSES, route);
    A.per_chunk = ch.per_chunk;
    const dim3 grid((unsigned)groups, ch.count);
    void (*kernel)(const FrameArgs) =
        mode == ACC_DEPTH  ? (ch.split ? k_frames_accumulate<ACC_DEPTH, true> : k_frames_accumulate<ACC_DEPTH, false>)
        : mode == ACC_BITS ? (ch.split ? k_frames_accumulate<ACC_BITS, true> : k_frames_accumulate<ACC_BITS, false>)
                           : (ch.split ? k_frames_accumulate<ACC_WARP, true> : k_frames_accumulate<ACC_WARP, false>);
    stin_clear_stale_error();
    hipLaunchKernelGGL(kernel, grid, dim3(FB), 0, stream, A);
    return stin_launch_status();
}

}  // namespace

extern "C" size_t stin_frames_edges_workspace_bytes(int B, int Hd, int Wd) {
    if (B < 0 || B > STIN_FRAMES_MAX_BATCH || !frame_size_ok(Hd, Wd, 1)) return 0;
    return stin_up256((size_t)(B > 0 ? B : 1) * (size_t)Hd * (size_t)Wd);
}

extern "C" int stin_frames_depth_edges_u16(const uint16_t* depth, int B, int Hd, int Wd, double depth_scale, double depth_trunc,
                                           double discontinuity_threshold, int half_kernel, uint8_t* edge, void* workspace,
                                           size_t workspace_bytes, stin_stream_t stream_) {
    STIN_REQUIRE(B >= 0 && B <= STIN_FRAMES_MAX_BATCH && frame_size_ok(Hd, Wd, 1), STIN_E_SIZE);
    STIN_REQUIRE(half_kernel >= 0 && half_kernel <= STIN_FRAMES_MAX_HALF_KERNEL && depth_scale > 0.0, STIN_E_SIZE);
    if (B == 0) return STIN_OK;
    STIN_REQUIRE(depth != nullptr && edge != nullptr, STIN_E_NULL);
    STIN_REQUIRE(workspace != nullptr && workspace_bytes >= stin_frames_edges_workspace_bytes(B, Hd, Wd), STIN_E_WORKSPACE);
    hipStream_t stream = (hipStream_t)stream_;
    stin_clear_stale_error();
    const double T = discontinuity_threshold * depth_scale;
    const int64_t HW = (int64_t)Hd * Wd;
    uint8_t* edge0 = (uint8_t*)workspace;
    hipLaunchKernelGGL(k_frames_edge0, dim3((unsigned)((HW + FB - 1) / FB), (unsigned)B), dim3(FB), 0, stream, depth, Hd, Wd,
                       keep_max_raw(depth_scale, depth_trunc), T * T, edge0);
    hipLaunchKernelGGL(k_frames_dilate, dim3((unsigned)((Wd + TW - 1) / TW), (unsigned)((Hd + TH - 1) / TH), (unsigned)B), dim3(FB), 0,
                       stream, edge0, Hd, Wd, half_kernel, edge);
    return stin_launch_status();
}

extern "C" int stin_frames_accumulate_f64(const double* vertices, int64_t N, const double* RT, const uint8_t* valid, int B,
                                          int64_t first_pose, const uint8_t* color, int Hc, int Wc, const uint16_t* depth,
                                          const uint8_t* edge, int Hd, int Wd, const double* cameras, const double* params,
                                          const uint32_t* bits, int64_t words, int margin, int route, int64_t* sum, int32_t* count,
                                          uint32_t* seen, int64_t seen_words, stin_stream_t stream_) {
    STIN_REQUIRE(cameras != nullptr && params != nullptr, STIN_E_NULL);
    const double depth_scale = params[0], depth_trunc = params[1], max_depth = params[2], depth_threshold = params[3], z_near = params[4];
    STIN_REQUIRE(N >= 0 && N < (int64_t)INT32_MAX && B >= 0 && B <= STIN_FRAMES_MAX_BATCH, STIN_E_SIZE);
    STIN_REQUIRE(first_pose >= 0 && first_pose + B < (int64_t)INT32_MAX, STIN_E_SIZE);
    STIN_REQUIRE(frame_size_ok(Hc, Wc, 1) && margin >= 0 && z_near > 0.0, STIN_E_SIZE);
    STIN_REQUIRE(route == STIN_FRAMES_ROUTE_AUTO || route == STIN_FRAMES_ROUTE_OWNER || route == STIN_FRAMES_ROUTE_SPLIT, STIN_E_SIZE);
    STIN_REQUIRE((depth != nullptr) != (bits != nullptr) || N == 0 || B == 0, STIN_E_UNSUPPORTED);   // exactly one visibility source
    const int64_t need_words = (first_pose + B + 31) / 32;
    if (depth != nullptr) STIN_REQUIRE(frame_size_ok(Hd, Wd, 1) && depth_scale > 0.0, STIN_E_SIZE);
    if (depth == nullptr && bits != nullptr) STIN_REQUIRE(words >= need_words, STIN_E_SIZE);
    if (seen != nullptr) STIN_REQUIRE(seen_words >= need_words, STIN_E_SIZE);
    if (N == 0 || B == 0) return STIN_OK;
    STIN_REQUIRE(vertices && RT && valid && color && sum && count, STIN_E_NULL);
    STIN_REQUIRE(depth == nullptr || edge != nullptr, STIN_E_NULL);
    FrameArgs A = {};
    A.vertices = vertices; A.RT = RT; A.valid = valid; A.color = color; A.depth = depth; A.edge = edge; A.bits = bits;
    A.sum = sum; A.count = count; A.seen = seen;
    A.N = N; A.first_pose = first_pose; A.words = words; A.seen_words = seen_words;
    A.C = view_of(cameras, z_near, margin, Hc, Wc);
    A.dfx = cameras[4]; A.dfy = cameras[5]; A.dcx = cameras[6]; A.dcy = cameras[7];
    A.depth_scale = depth_scale; A.max_depth = max_depth; A.depth_threshold = depth_threshold;
    A.B = B; A.Hc = Hc; A.Wc = Wc; A.Hd = Hd; A.Wd = Wd;
    A.keep_max = depth != nullptr ? keep_max_raw(depth_scale, depth_trunc) : 0;
    return launch_accumulate(A, depth != nullptr ? ACC_DEPTH : ACC_BITS, route, (hipStream_t)stream_);
}

extern "C" int stin_nonrigid_accumulate_f64(const double* vertices, int64_t N, const double* RT, const uint8_t* valid, int B,
                                            int64_t first_pose, const uint8_t* color, int H, int W, const double* flow, int lattice_step,
                                            const double* camera, double z_near, const uint32_t* bits, int64_t words, int margin,
                                            int route, int64_t* sum, int32_t* count, uint32_t* seen, int64_t seen_words,
                                            stin_stream_t stream_) {
    STIN_REQUIRE(camera != nullptr, STIN_E_NULL);
    STIN_REQUIRE(N >= 0 && N < (int64_t)INT32_MAX && B >= 0 && B <= STIN_FRAMES_MAX_BATCH, STIN_E_SIZE);
    STIN_REQUIRE(first_pose >= 0 && first_pose + B < (int64_t)INT32_MAX, STIN_E_SIZE);
    STIN_REQUIRE(frame_size_ok(H, W, 2) && lattice_step >= 1 && margin >= 0 && z_near > 0.0, STIN_E_SIZE);
    STIN_REQUIRE(route == STIN_FRAMES_ROUTE_AUTO || route == STIN_FRAMES_ROUTE_OWNER || route == STIN_FRAMES_ROUTE_SPLIT, STIN_E_SIZE);
    const int64_t need_words = (first_pose + B + 31) / 32;
    STIN_REQUIRE(words >= need_words || N == 0 || B == 0, STIN_E_SIZE);
    if (seen != nullptr) STIN_REQUIRE(seen_words >= need_words, STIN_E_SIZE);
    if (N == 0 || B == 0) return STIN_OK;
    STIN_REQUIRE(vertices && RT && valid && color && flow && bits && sum && count, STIN_E_NULL);
    FrameArgs A = {};
    A.vertices = vertices; A.RT = RT; A.valid = valid; A.color = color; A.bits = bits; A.flow = flow;
    A.sum = sum; A.count = count; A.seen = seen;
    A.N = N; A.first_pose = first_pose; A.words = words; A.seen_words = seen_words;
    A.C = view_of(camera, z_near, margin, H, W, lattice_step);
    A.B = B; A.Hc = H; A.Wc = W;
    return launch_accumulate(A, ACC_WARP, route, (hipStream_t)stream_);
}

extern "C" int stin_frames_finish_f32(const int64_t* sum, const int32_t* count, int64_t N, float fill_r, float fill_g, float fill_b,
                                      float* colors, uint8_t* observed, stin_stream_t stream_) {
    STIN_REQUIRE(N >= 0 && N < (int64_t)INT32_MAX, STIN_E_SIZE);
    if (N == 0) return STIN_OK;
    STIN_REQUIRE(sum != nullptr && count != nullptr && (colors != nullptr || observed != nullptr), STIN_E_NULL);
    stin_clear_stale_error();
    hipLaunchKernelGGL(k_frames_finish, dim3((unsigned)((N + FB - 1) / FB)), dim3(FB), 0, (hipStream_t)stream_, sum, count, N, fill_r,
                       fill_g, fill_b, colors, observed);
    return stin_launch_status();
}
