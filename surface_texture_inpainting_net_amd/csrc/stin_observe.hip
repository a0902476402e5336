// Observer masks on the device: which vertices does every camera pose of a scan see (reference
// preprocessing/observed_texture_map_generation.py :159-267, `generate_masks.sh observers`; the reference renders the mesh with
// PyTorch3D's MeshRasterizer and keeps pix_to_face).  Contract: include/stin_hip.h ("observer masks"); tests/_observers_oracle.py
// restates it in numpy, pixel-major, and agrees bit for bit.
//
//   faces:     int64 -> int32 once, a face with an index outside [0, N) becomes (-1, -1, -1) and sets STIN_OBSERVE_BAD_INDEX
//              (stin_narrow_i64_to_i32 truncates before anyone can look: 2^40 would come out as vertex 0).
//   per batch of poses (the z-buffers of a batch live in the workspace):
//   clear:     every key of the batch = all ones ("no face"), the large-face queue emptied.
//   transform: one thread per (vertex, pose): view space, then the screen position in pixel units -> (X, Y, zv), 24 bytes that the
//              faces around the vertex (six on a manifold mesh) read from L2 instead of transforming it again.
//   raster:    one thread per (face, pose): cull, bounding box clamped to the image, loop over its centres, 64-bit atomicMin of
//              (fp32 depth bits << 32 | face id).  A box of more than `large_box` centres is not looped by its lane (a wave64 would
//              wait for it with 63 lanes idle): the (face, pose) goes to a queue.
//   large:     one wavefront per queue entry, lane k takes the centres k, k + 64, ... of the box.  Same setup, same per-centre
//              expressions, same atomicMin: which kernel rasterises a face cannot change a key.
//   resolve:   one thread per (pixel, pose): the winning face's three vertices get bit p of their row (atomicOr on uint32, after a
//              plain look that skips the bits already there).
// Integer min / or only: the result does not depend on the schedule, the batch size or `large_box`.
#include "stin_common.h"

namespace {

constexpr int OB = 256;                                   // threads per workgroup
constexpr unsigned long long NO_FACE = ~0ull;
constexpr unsigned QUEUE_CAP = 1u << 20;                  // large-face queue entries per batch; beyond it a lane loops its own face
constexpr int LARGE_GRID = 1024;                          // workgroups of the large-face kernel (4 waves each, entries strided)

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct ObserveLayout {
    size_t faces, coords, keys, queue, ctl, total;
};
ObserveLayout observe_layout(int64_t N, int64_t F, int S, int batch) {
    ObserveLayout L;
    size_t off = 0;
    L.faces = off; off += up256((size_t)(F > 0 ? F : 1) * 3 * 4);
    L.coords = off; off += up256((size_t)batch * (size_t)(N > 0 ? N : 1) * 3 * 8);
    L.keys = off; off += up256((size_t)batch * (size_t)S * (size_t)S * 8);
    L.queue = off; off += up256((size_t)QUEUE_CAP * 8);
    L.ctl = off; off += 256;
    L.total = off;
    return L;
}

__global__ void k_observe_faces(const int64_t* __restrict__ faces, int64_t F, int64_t N, int32_t* __restrict__ f32,
                                int32_t* __restrict__ status) {
    const int64_t f = (int64_t)blockIdx.x * OB + threadIdx.x;
    if (f >= F) return;
    int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (a < 0 || a >= N || b < 0 || b >= N || c < 0 || c >= N) {
        atomicOr(status, STIN_OBSERVE_BAD_INDEX);
        a = b = c = -1;
    }
    f32[3 * f] = (int32_t)a;
    f32[3 * f + 1] = (int32_t)b;
    f32[3 * f + 2] = (int32_t)c;
}

__global__ void k_observe_clear(unsigned long long* __restrict__ keys, int64_t n, unsigned* __restrict__ qcount) {
    const int64_t i = (int64_t)blockIdx.x * OB + threadIdx.x;
    if (i < n) keys[i] = NO_FACE;
    if (i == 0) *qcount = 0u;
}

// coords[b][v] = (X, Y, zv) of vertex v seen from pose p0 + b
__global__ void k_observe_transform(const double* __restrict__ vertices, int64_t N, const double* __restrict__ RT,
                                    const uint8_t* __restrict__ valid, int64_t p0, double sx, double sy, double half,
                                    double* __restrict__ coords) {
    const int64_t v = (int64_t)blockIdx.x * OB + threadIdx.x;
    const int64_t p = p0 + blockIdx.y;
    if (v >= N || !valid[p]) return;
    const double* m = RT + p * 12;
    const double x = vertices[3 * v], y = vertices[3 * v + 1], z = vertices[3 * v + 2];
    const double xv = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    const double yv = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    const double zv = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
    double* o = coords + ((int64_t)blockIdx.y * N + v) * 3;
    o[0] = (sx * xv / zv + 1.0) * half - 0.5;
    o[1] = (sy * yv / zv + 1.0) * half - 0.5;
    o[2] = zv;
}

struct Tri {
    double ax, ay, az, bx, by, bz, cx, cy, cz, area2;
    int x0, x1, y0, y1;
};

__device__ inline bool finite3(double a, double b, double c) { return isfinite(a) && isfinite(b) && isfinite(c); }

// The cull tests of the contract and the box of centres that can be covered; false: the face is skipped for this pose.
__device__ inline bool tri_setup(const int32_t* __restrict__ f32, int64_t f, const double* __restrict__ c, double z_near, int S, Tri& t) {
    const int32_t ia = f32[3 * f], ib = f32[3 * f + 1], ic = f32[3 * f + 2];
    if (ia < 0) return false;                              // an index outside [0, N)
    t.az = c[3 * (int64_t)ia + 2];
    t.bz = c[3 * (int64_t)ib + 2];
    t.cz = c[3 * (int64_t)ic + 2];
    if (t.az < z_near || t.bz < z_near || t.cz < z_near) return false;
    t.ax = c[3 * (int64_t)ia];
    t.ay = c[3 * (int64_t)ia + 1];
    t.bx = c[3 * (int64_t)ib];
    t.by = c[3 * (int64_t)ib + 1];
    t.cx = c[3 * (int64_t)ic];
    t.cy = c[3 * (int64_t)ic + 1];
    if (!finite3(t.ax, t.bx, t.cx) || !finite3(t.ay, t.by, t.cy)) return false;
    t.area2 = (t.bx - t.ax) * (t.cy - t.ay) - (t.by - t.ay) * (t.cx - t.ax);
    if (!(t.area2 > 0.0) && !(t.area2 < 0.0)) return false;   // zero (or not a number: no centre could pass the sign tests)
    // centres inside [min, max] of the corners, inside the image; compared as doubles before anything becomes an int
    const double xlo = fmax(ceil(fmin(t.ax, fmin(t.bx, t.cx))), 0.0), xhi = fmin(floor(fmax(t.ax, fmax(t.bx, t.cx))), (double)(S - 1));
    const double ylo = fmax(ceil(fmin(t.ay, fmin(t.by, t.cy))), 0.0), yhi = fmin(floor(fmax(t.ay, fmax(t.by, t.cy))), (double)(S - 1));
    if (xlo > xhi || ylo > yhi) return false;
    t.x0 = (int)xlo;
    t.x1 = (int)xhi;
    t.y0 = (int)ylo;
    t.y1 = (int)yhi;
    return true;
}

// One centre: coverage (inclusive edges), perspective-correct depth, the key, atomicMin.
__device__ inline void tri_centre(const Tri& t, int px, int py, unsigned long long* __restrict__ keys, int S, uint32_t face) {
    const double X = (double)px, Y = (double)py;
    const double wa = (t.cx - t.bx) * (Y - t.by) - (t.cy - t.by) * (X - t.bx);
    const double wb = (t.ax - t.cx) * (Y - t.cy) - (t.ay - t.cy) * (X - t.cx);
    const double wc = (t.bx - t.ax) * (Y - t.ay) - (t.by - t.ay) * (X - t.ax);
    const bool in = t.area2 > 0.0 ? (wa >= 0.0 && wb >= 0.0 && wc >= 0.0) : (wa <= 0.0 && wb <= 0.0 && wc <= 0.0);
    if (!in) return;
    const double la = wa / t.area2, lb = wb / t.area2, lc = wc / t.area2;
    const double zp = 1.0 / ((la / t.az + lb / t.bz) + lc / t.cz);
    const unsigned long long key = ((unsigned long long)__float_as_uint((float)zp) << 32) | face;
    unsigned long long* k = keys + (int64_t)py * S + px;
    if (*k > key) atomicMin(k, key);                       // keys only fall: a stale look can cost an atomic, never lose one
}

__global__ __launch_bounds__(OB) void k_observe_raster(const int32_t* __restrict__ f32, int64_t F, const double* __restrict__ coords,
                                                       int64_t N, const uint8_t* __restrict__ valid, int64_t p0, double z_near, int S,
                                                       int64_t large_box, unsigned long long* __restrict__ keys,
                                                       unsigned long long* __restrict__ queue, unsigned* __restrict__ qcount) {
    const int64_t f = (int64_t)blockIdx.x * OB + threadIdx.x;
    const int b = blockIdx.y;
    if (f >= F || !valid[p0 + b]) return;
    Tri t;
    if (!tri_setup(f32, f, coords + (int64_t)b * N * 3, z_near, S, t)) return;
    if ((int64_t)(t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1) > large_box) {
        const unsigned slot = atomicAdd(qcount, 1u);
        if (slot < QUEUE_CAP) {
            queue[slot] = ((unsigned long long)b << 32) | (unsigned long long)f;
            return;
        }                                                  // queue full: rasterise it here, the keys come out the same
    }
    unsigned long long* kp = keys + (int64_t)b * S * S;
    for (int py = t.y0; py <= t.y1; ++py)
        for (int px = t.x0; px <= t.x1; ++px) tri_centre(t, px, py, kp, S, (uint32_t)f);
}

__global__ __launch_bounds__(OB) void k_observe_raster_large(const int32_t* __restrict__ f32, const double* __restrict__ coords, int64_t N,
                                                             double z_near, int S, unsigned long long* __restrict__ keys,
                                                             const unsigned long long* __restrict__ queue,
                                                             const unsigned* __restrict__ qcount, int32_t* __restrict__ status) {
    const unsigned n = *qcount < QUEUE_CAP ? *qcount : QUEUE_CAP;
    const int lane = threadIdx.x & (STIN_WAVE - 1);
    const unsigned waves = gridDim.x * (OB / STIN_WAVE);
    for (unsigned e = blockIdx.x * (OB / STIN_WAVE) + threadIdx.x / STIN_WAVE; e < n; e += waves) {
        const unsigned long long entry = queue[e];
        const int b = (int)(entry >> 32);
        const int64_t f = (int64_t)(entry & 0xffffffffull);
        Tri t;
        if (!tri_setup(f32, f, coords + (int64_t)b * N * 3, z_near, S, t)) continue;   // (it passed in k_observe_raster)
        unsigned long long* kp = keys + (int64_t)b * S * S;
        const int w = t.x1 - t.x0 + 1, total = w * (t.y1 - t.y0 + 1);
        for (int k = lane; k < total; k += STIN_WAVE) tri_centre(t, t.x0 + k % w, t.y0 + k / w, kp, S, (uint32_t)f);
        if (lane == 0 && !(*status & STIN_OBSERVE_LARGE_FACE)) atomicOr(status, STIN_OBSERVE_LARGE_FACE);
    }
}

__global__ void k_observe_resolve(const unsigned long long* __restrict__ keys, const int32_t* __restrict__ f32, int64_t S2, int64_t p0,
                                  uint32_t* __restrict__ bits, int64_t words) {
    const int64_t i = (int64_t)blockIdx.x * OB + threadIdx.x;
    if (i >= S2) return;
    const unsigned long long key = keys[(int64_t)blockIdx.y * S2 + i];
    if (key == NO_FACE) return;
    const int64_t f = (int64_t)(key & 0xffffffffull);
    const int64_t p = p0 + blockIdx.y;
    const uint32_t bit = 1u << (p & 31);
    for (int k = 0; k < 3; ++k) {
        uint32_t* w = bits + (int64_t)f32[3 * f + k] * words + (p >> 5);
        if (!(*w & bit)) atomicOr(w, bit);
    }
}

__global__ void k_observe_mask(const uint32_t* __restrict__ bits, int64_t N, int64_t words, const uint32_t* __restrict__ visible,
                               int min_num_poses, int invert, int64_t* __restrict__ mask, int32_t* __restrict__ count) {
    const int64_t v = (int64_t)blockIdx.x * OB + threadIdx.x;
    if (v >= N) return;
    const uint32_t* row = bits + v * words;
    const uint32_t* vis = visible + (int64_t)blockIdx.y * words;
    int c = 0;
    for (int64_t w = 0; w < words; ++w) c += __popc(row[w] & vis[w]);
    const int64_t o = (int64_t)blockIdx.y * N + v;
    if (mask != nullptr) mask[o] = (int64_t)((c >= min_num_poses ? 1 : 0) ^ (invert ? 1 : 0));
    if (count != nullptr) count[o] = c;
}

}  // namespace

extern "C" size_t stin_observe_workspace_bytes(int64_t N, int64_t F, int S, int batch) {
    if (N < 0 || F < 0 || S < 1 || S > STIN_OBSERVE_MAX_SIZE || batch < 1 || batch > STIN_OBSERVE_MAX_BATCH) return 0;
    return observe_layout(N, F, S, batch).total;
}

extern "C" int stin_observe_poses_f64(const double* vertices, int64_t N, const int64_t* faces, int64_t F, const double* RT,
                                      const uint8_t* valid, int64_t P, double sx, double sy, int S, double z_near, int batch,
                                      int64_t large_box, uint32_t* bits, int64_t words, int32_t* status, void* workspace,
                                      size_t workspace_bytes, stin_stream_t stream_) {
    STIN_REQUIRE(N >= 0 && F >= 0 && P >= 0 && N < (int64_t)INT32_MAX && F < (int64_t)INT32_MAX, STIN_E_SIZE);
    STIN_REQUIRE(S >= 1 && S <= STIN_OBSERVE_MAX_SIZE && batch >= 1 && batch <= STIN_OBSERVE_MAX_BATCH, STIN_E_SIZE);
    STIN_REQUIRE(words >= (P + 31) / 32 && z_near > 0.0, STIN_E_SIZE);
    STIN_REQUIRE(status != nullptr && (N == 0 || vertices) && (N == 0 || words == 0 || bits), STIN_E_NULL);
    STIN_REQUIRE((F == 0 || faces) && (P == 0 || (RT && valid)), STIN_E_NULL);
    STIN_REQUIRE(workspace != nullptr && workspace_bytes >= stin_observe_workspace_bytes(N, F, S, batch), STIN_E_WORKSPACE);
    hipStream_t stream = (hipStream_t)stream_;
    stin_clear_stale_error();
    const ObserveLayout L = observe_layout(N, F, S, batch);
    char* w = (char*)workspace;
    int32_t* f32 = (int32_t*)(w + L.faces);
    double* coords = (double*)(w + L.coords);
    unsigned long long* keys = (unsigned long long*)(w + L.keys);
    unsigned long long* queue = (unsigned long long*)(w + L.queue);
    unsigned* qcount = (unsigned*)(w + L.ctl);
    if (large_box <= 0) large_box = STIN_OBSERVE_LARGE_BOX;
    (void)hipMemsetAsync(status, 0, 4, stream);
    if (N > 0 && words > 0) (void)hipMemsetAsync(bits, 0, (size_t)N * (size_t)words * 4, stream);
    if (N == 0 || F == 0 || P == 0) return stin_launch_status();
    const unsigned gf = (unsigned)((F + OB - 1) / OB), gv = (unsigned)((N + OB - 1) / OB);
    const int64_t S2 = (int64_t)S * S;
    hipLaunchKernelGGL(k_observe_faces, dim3(gf), dim3(OB), 0, stream, faces, F, N, f32, status);
    for (int64_t p0 = 0; p0 < P; p0 += batch) {
        const unsigned nb = (unsigned)(P - p0 < batch ? P - p0 : batch);
        const int64_t nk = (int64_t)nb * S2;
        hipLaunchKernelGGL(k_observe_clear, dim3((unsigned)((nk + OB - 1) / OB)), dim3(OB), 0, stream, keys, nk, qcount);
        hipLaunchKernelGGL(k_observe_transform, dim3(gv, nb), dim3(OB), 0, stream, vertices, N, RT, valid, p0, sx, sy, 0.5 * (double)S,
                           coords);
        hipLaunchKernelGGL(k_observe_raster, dim3(gf, nb), dim3(OB), 0, stream, f32, F, coords, N, valid, p0, z_near, S, large_box, keys,
                           queue, qcount);
        hipLaunchKernelGGL(k_observe_raster_large, dim3(LARGE_GRID), dim3(OB), 0, stream, f32, coords, N, z_near, S, keys, queue, qcount,
                           status);
        hipLaunchKernelGGL(k_observe_resolve, dim3((unsigned)((S2 + OB - 1) / OB), nb), dim3(OB), 0, stream, keys, f32, S2, p0, bits,
                           words);
    }
    return stin_launch_status();
}

extern "C" int stin_observe_mask_u32(const uint32_t* bits, int64_t N, int64_t words, const uint32_t* visible_words, int M,
                                     int min_num_poses, int invert, int64_t* mask, int32_t* count, stin_stream_t stream_) {
    STIN_REQUIRE(N >= 0 && words >= 0 && M >= 0 && M <= 65535, STIN_E_SIZE);
    STIN_REQUIRE(mask != nullptr || count != nullptr, STIN_E_NULL);
    if (N == 0 || M == 0) return STIN_OK;
    STIN_REQUIRE(words == 0 || (bits && visible_words), STIN_E_NULL);
    stin_clear_stale_error();
    hipLaunchKernelGGL(k_observe_mask, dim3((unsigned)((N + OB - 1) / OB), (unsigned)M), dim3(OB), 0, (hipStream_t)stream_, bits, N, words,
                       visible_words, min_num_poses, invert, mask, count);
    return stin_launch_status();
}
