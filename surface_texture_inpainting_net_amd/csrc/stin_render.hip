// Result views on the device: a vertex-coloured mesh through a pinhole camera from every pose -> colour, depth and face-id images
// (what the reference's utils/ColorCompletionVisualizer.py shows in an Open3D window, unlit, and what its `P` key saves).
// Contract: include/stin_hip.h ("Render"); tests/_render_oracle.py restates it in numpy, pixel-major, and agrees bit for bit.
//
//   faces, and per batch of poses clear, transform, raster, large: the shared rasteriser (stin_raster.hip) with the pinhole screen;
//              keys and screen coordinates of a batch live in the workspace.  At 480 x 640 and above the large-face kernel is
//              where most of the covered pixels come from (profiles/r26_render.md).
//   resolve:   a workgroup owns 512 consecutive pixels of the [P][H][W] arrays (two per thread: one 16-byte key load), recomputes
//              the winner's barycentrics, interpolates the colour perspective-correctly and stages colour / depth / face id in LDS;
//              the workgroup then streams each array out with 16-byte stores.  The pixel index is GLOBAL over the poses, so the 3-
//              and 12-byte pixels need no alignment beyond the array's own: 512 pixels are a multiple of 16 bytes in every format.
// Integer min only: the images do not depend on the schedule, the batch size or `large_box`.
#include "stin_raster.h"

#include <cmath>

namespace {

constexpr int RB = 256;                                   // threads per workgroup
constexpr int RES_PIX = 512;                              // pixels of a resolve workgroup
constexpr unsigned long long NO_FACE = STIN_RASTER_NO_FACE;
constexpr int LARGE_GRID = 2048;                          // workgroups of the large-face kernel (r26_render.md)
constexpr int ALL_STAGES = STIN_RASTER_ALL_STAGES | STIN_RENDER_STAGE_RESOLVE;

// the keys of a batch start at its first pixel's GLOBAL index modulo RES_PIX, so that a resolve workgroup's keys are aligned
RasterLayout render_layout(int64_t N, int64_t F, int H, int W, int batch) {
    return stin_raster_layout(N, F, batch, (size_t)batch * (size_t)H * (size_t)W + RES_PIX);
}

struct Background {
    float f[4];
    uint8_t u[4];
};

struct Outputs {
    float* color_f32;
    uint8_t* color_u8;
    uint16_t* depth;
    int32_t* face;
    int vec;                                               // bit 0..3: the array's base is 16-byte aligned
};

__host__ __device__ inline uint8_t quantise(float c) {
    double t = (double)c;
    if (!(t > 0.0)) t = 0.0;                               // also NaN
    if (t > 1.0) t = 1.0;
    return (uint8_t)rint(t * 255.0);
}

// The workgroup's `bytes` bytes of one output array, staged in LDS, to global memory: 16 bytes per lane when the array's base is
// aligned and the whole region belongs to the batch; the first and last workgroup of a batch (and an unaligned array) go by element.
__device__ inline void stream_out(char* __restrict__ dst, const char* src, int bytes, int lo, int hi, bool vec) {
    if (vec && lo == 0 && hi == bytes) {
        for (int i = threadIdx.x * 16; i < bytes; i += RB * 16) *reinterpret_cast<uint4*>(dst + i) = *reinterpret_cast<const uint4*>(src + i);
    } else {
        for (int i = lo + threadIdx.x; i < hi; i += RB) dst[i] = src[i];
    }
}

// g_base: the global pixel index ([P][H][W] flattened) of the first workgroup's first pixel, a multiple of RES_PIX; the batch owns
// [g_lo, g_hi); keys[0] is pixel g_base's key.
__global__ __launch_bounds__(RB) void k_render_resolve(const unsigned long long* __restrict__ keys, const int32_t* __restrict__ f32,
                                                       const double* __restrict__ coords, int64_t N, const float* __restrict__ colors,
                                                       int K, int64_t g_base, int64_t g_lo, int64_t g_hi, int64_t p0, int H, int W,
                                                       double depth_scale, Background bg, Outputs out) {
    __shared__ uint4 s_f32[RES_PIX * 4 * 4 / 16];
    __shared__ uint4 s_u8[RES_PIX * 4 / 16];
    __shared__ uint4 s_depth[RES_PIX * 2 / 16];
    __shared__ uint4 s_face[RES_PIX * 4 / 16];
    float* cf = reinterpret_cast<float*>(s_f32);
    uint8_t* cu = reinterpret_cast<uint8_t*>(s_u8);
    uint16_t* dp = reinterpret_cast<uint16_t*>(s_depth);
    int32_t* fc = reinterpret_cast<int32_t*>(s_face);
    const int64_t g0 = g_base + (int64_t)blockIdx.x * RES_PIX;           // the workgroup's first pixel
    const int l0 = 2 * threadIdx.x;                                       // the thread's two pixels: l0, l0 + 1
    const int64_t HW = (int64_t)H * W;
    const int64_t pose0 = g0 / HW, rest0 = g0 - pose0 * HW;               // workgroup-uniform: the one 64-bit division
    const bool in0 = g0 + l0 >= g_lo && g0 + l0 < g_hi, in1 = g0 + l0 + 1 >= g_lo && g0 + l0 + 1 < g_hi;
    unsigned long long key0 = NO_FACE, key1 = NO_FACE;
    const unsigned long long* kp = keys + (int64_t)blockIdx.x * RES_PIX + l0;
    if (in0 && in1) {
        const ulonglong2 k2 = *reinterpret_cast<const ulonglong2*>(kp);
        key0 = k2.x;
        key1 = k2.y;
    } else {
        if (in0) key0 = kp[0];
        if (in1) key1 = kp[1];
    }
#pragma unroll 1
    for (int j = 0; j < 2; ++j) {
        if (!(j == 0 ? in0 : in1)) continue;
        const unsigned long long key = j == 0 ? key0 : key1;
        const int l = l0 + j;
        int32_t face = -1;
        uint16_t mm16 = 0;
        if (key == NO_FACE) {
#pragma unroll
            for (int k = 0; k < 4; ++k)                    // (static indices: the background stays in scalar registers)
                if (k < K) {
                    cf[l * K + k] = bg.f[k];
                    cu[l * K + k] = bg.u[k];
                }
        } else {
            int64_t p = pose0, rest = rest0 + l;                          // pose and pixel of g0 + l
            if (HW >= RES_PIX) {
                if (rest >= HW) {
                    rest -= HW;
                    ++p;
                }
            } else {                                                      // an image smaller than the tile: several poses in it
                p += rest / HW;
                rest %= HW;
            }
            const int r = (int)rest, py = r / W, px = r - py * W;
            const int64_t f = (int64_t)(key & 0xffffffffull);
            face = (int32_t)f;
            const int32_t ia = f32[3 * f], ib = f32[3 * f + 1], ic = f32[3 * f + 2];
            const double* c = coords + (p - p0) * N * 3;
            const double ax = c[3 * (int64_t)ia], ay = c[3 * (int64_t)ia + 1], az = c[3 * (int64_t)ia + 2];
            const double bx = c[3 * (int64_t)ib], by = c[3 * (int64_t)ib + 1], bz = c[3 * (int64_t)ib + 2];
            const double cx = c[3 * (int64_t)ic], cy = c[3 * (int64_t)ic + 1], cz = c[3 * (int64_t)ic + 2];
            const double X = (double)px, Y = (double)py;
            const double area2 = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
            const double wa = (cx - bx) * (Y - by) - (cy - by) * (X - bx);
            const double wb = (ax - cx) * (Y - cy) - (ay - cy) * (X - cx);
            const double wc = (bx - ax) * (Y - ay) - (by - ay) * (X - ax);
            const double la = wa / area2, lb = wb / area2, lc = wc / area2;
            const double zp = 1.0 / ((la / az + lb / bz) + lc / cz);
            const double qa = (la / az) * zp, qb = (lb / bz) * zp, qc = (lc / cz) * zp;
            const float *ca = colors + (int64_t)ia * K, *cb = colors + (int64_t)ib * K, *cc = colors + (int64_t)ic * K;
            for (int k = 0; k < K; ++k) {
                const double val = (qa * (double)ca[k] + qb * (double)cb[k]) + qc * (double)cc[k];
                const float v32 = (float)val;
                cf[l * K + k] = v32;
                cu[l * K + k] = quantise(v32);
            }
            const double mm = rint(zp * depth_scale);
            if (isfinite(mm) && mm > 0.0 && mm < 65535.0) mm16 = (uint16_t)mm;
        }
        dp[l] = mm16;
        fc[l] = face;
    }
    __syncthreads();
    const int64_t first = g_lo > g0 ? g_lo - g0 : 0, last = g_hi - g0 < RES_PIX ? g_hi - g0 : RES_PIX;   // the batch's share, in pixels
    const int lo = (int)first, hi = (int)last;
    if (out.color_f32 != nullptr)
        stream_out(reinterpret_cast<char*>(out.color_f32 + g0 * K), reinterpret_cast<const char*>(cf), RES_PIX * K * 4, lo * K * 4, hi * K * 4,
                   out.vec & 1);
    if (out.color_u8 != nullptr)
        stream_out(reinterpret_cast<char*>(out.color_u8 + g0 * K), reinterpret_cast<const char*>(cu), RES_PIX * K, lo * K, hi * K, out.vec & 2);
    if (out.depth != nullptr)
        stream_out(reinterpret_cast<char*>(out.depth + g0), reinterpret_cast<const char*>(dp), RES_PIX * 2, lo * 2, hi * 2, out.vec & 4);
    if (out.face != nullptr)
        stream_out(reinterpret_cast<char*>(out.face + g0), reinterpret_cast<const char*>(fc), RES_PIX * 4, lo * 4, hi * 4, out.vec & 8);
}

bool render_sizes_ok(int64_t N, int64_t F, int H, int W, int batch) {
    return N >= 0 && F >= 0 && N < (int64_t)INT32_MAX && F < (int64_t)INT32_MAX && H >= 1 && H <= STIN_RENDER_MAX_SIZE && W >= 1 &&
           W <= STIN_RENDER_MAX_SIZE && batch >= 1 && batch <= STIN_RENDER_MAX_BATCH;
}

}  // namespace

extern "C" size_t stin_render_workspace_bytes(int64_t N, int64_t F, int H, int W, int batch) {
    if (!render_sizes_ok(N, F, H, W, batch)) return 0;
    return render_layout(N, F, H, W, batch).total;
}

extern "C" int stin_render_poses_f64(const double* vertices, int64_t N, const int64_t* faces, int64_t F, const float* colors, int K,
                                     const double* RT, const uint8_t* valid, int64_t P, const double* camera, int H, int W,
                                     double z_near, double depth_scale, const float* background, int batch, int64_t large_box,
                                     int stages, float* color_f32, uint8_t* color_u8, uint16_t* depth, int32_t* face_ids,
                                     int32_t* status, void* workspace, size_t workspace_bytes, stin_stream_t stream_) {
    STIN_REQUIRE(render_sizes_ok(N, F, H, W, batch) && P >= 0 && P < (int64_t)INT32_MAX, STIN_E_SIZE);
    STIN_REQUIRE(K >= 1 && K <= 4 && z_near > 0.0 && depth_scale > 0.0 && stages <= ALL_STAGES, STIN_E_SIZE);
    STIN_REQUIRE(status != nullptr && camera != nullptr && background != nullptr, STIN_E_NULL);
    STIN_REQUIRE((N == 0 || (vertices && colors)) && (F == 0 || faces) && (P == 0 || (RT && valid)), STIN_E_NULL);
    STIN_REQUIRE(workspace != nullptr && workspace_bytes >= stin_render_workspace_bytes(N, F, H, W, batch), STIN_E_WORKSPACE);
    hipStream_t stream = (hipStream_t)stream_;
    stin_clear_stale_error();
    RasterCall c = {vertices, N, F, RT, valid, {STIN_RASTER_PINHOLE, {camera[0], camera[1], camera[2], camera[3]}}, H, W, z_near,
                    large_box > 0 ? large_box : STIN_RENDER_LARGE_BOX, LARGE_GRID, status};
    stin_raster_bind(c, render_layout(N, F, H, W, batch), workspace);
    if (stages <= 0) stages = ALL_STAGES;
    Background bg = {};
    for (int k = 0; k < K; ++k) {
        bg.f[k] = background[k];
        bg.u[k] = quantise(background[k]);
    }
    Outputs out = {color_f32, color_u8, depth, face_ids, 0};
    out.vec = (stin_aligned16(color_f32) ? 1 : 0) | (stin_aligned16(color_u8) ? 2 : 0) | (stin_aligned16(depth) ? 4 : 0) |
              (stin_aligned16(face_ids) ? 8 : 0);
    (void)hipMemsetAsync(status, 0, 4, stream);
    if (P == 0) return stin_launch_status();
    const int64_t HW = (int64_t)H * W;
    stin_raster_faces(c, faces, stream);
    for (int64_t p0 = 0; p0 < P; p0 += batch) {
        const unsigned nb = (unsigned)(P - p0 < batch ? P - p0 : batch);
        const int64_t g_lo = p0 * HW, g_hi = g_lo + (int64_t)nb * HW, g_base = g_lo & ~(int64_t)(RES_PIX - 1);
        stin_raster_batch(c, p0, nb, g_hi - g_base, g_lo - g_base, stages, stream);      // (no geometry: every pixel is background)
        if (stages & STIN_RENDER_STAGE_RESOLVE)
            hipLaunchKernelGGL(k_render_resolve, dim3((unsigned)((g_hi - g_base + RES_PIX - 1) / RES_PIX)), dim3(RB), 0, stream, c.keys, c.f32,
                               c.coords, N, colors, K, g_base, g_lo, g_hi, p0, H, W, depth_scale, bg, out);
    }
    return stin_launch_status();
}
