// The test of a (vertex, pose) pair and what is sampled at its projection: one copy under the frame colours (stin_frames.hip), the
// rigid normal equations (stin_colormap.hip) and the non-rigid ones (stin_nonrigid.hip); stin_raster.hip takes the view transform.
// The three contracts in include/stin_hip.h state every expression below with its bracketing, and the numpy restatements under
// tests/ compare bytes: an operand, a bracket or an order changed here changes all of them at once.  Built with -ffp-contract=off.
#pragma once
#include "stin_common.h"

inline bool frame_size_ok(int H, int W, int least) {
    return H >= least && W >= least && H <= STIN_FRAMES_MAX_SIZE && W <= STIN_FRAMES_MAX_SIZE;
}
inline int anchors_of(int n, int S) { return (n - 1 + S - 1) / S + 1; }      // ceil((n - 1) / S) + 1

struct View {                                             // what the pair test and the warp need besides the pose and the vertex
    double fx, fy, cx, cy, z_near;
    double u_lo, u_hi, v_lo, v_hi;                        // margin, W - 1 - margin, margin, H - 1 - margin
    double S;                                             // the warp lattice: its step and anchors (0: the caller has none)
    int Ah, Aw;
};

inline View view_of(const double* camera, double z_near, int margin, int H, int W, int S = 0) {
    View C;
    C.fx = camera[0]; C.fy = camera[1]; C.cx = camera[2]; C.cy = camera[3]; C.z_near = z_near;
    C.u_lo = (double)margin; C.u_hi = (double)(W - 1 - margin); C.v_lo = (double)margin; C.v_hi = (double)(H - 1 - margin);
    C.S = (double)S;
    C.Ah = S > 0 ? anchors_of(H, S) : 0;
    C.Aw = S > 0 ? anchors_of(W, S) : 0;
    return C;
}

// Chunks of poses over grid.y until the chip is full: as many chunks of at least min_poses poses as it takes to reach FILL_GROUPS
// workgroups, from the workgroups of one chunk and B (> 0) alone.  route: STIN_FRAMES_ROUTE_*; OWNER is one chunk, SPLIT at least
// two where B allows.  split: more than one chunk may add to the same output, so the kernel has to add atomically.  A launch
// decision: no sum sees it.
struct PoseChunks {
    int per_chunk;
    unsigned count;
    bool split;
};
inline PoseChunks pose_chunks(int64_t groups, int B, int min_poses, int route) {
    constexpr int64_t FILL_GROUPS = 1024;                 // workgroups that fill the chip (256 CUs x 4)
    int64_t chunks = (FILL_GROUPS + groups - 1) / groups;
    const int64_t most = (B + min_poses - 1) / min_poses;
    if (chunks > most) chunks = most;
    if (route == STIN_FRAMES_ROUTE_OWNER) chunks = 1;
    if (route == STIN_FRAMES_ROUTE_SPLIT && chunks < 2) chunks = B < 2 ? 1 : 2;
    PoseChunks r;
    r.per_chunk = (int)((B + chunks - 1) / chunks);
    r.count = (unsigned)((B + r.per_chunk - 1) / r.per_chunk);
    r.split = route == STIN_FRAMES_ROUTE_SPLIT || chunks > 1;
    return r;
}

// view = m [x y z 1], m the 3 x 4 extrinsic, row-major
__device__ inline double view_x(const double* m, double x, double y, double z) { return ((m[0] * x + m[1] * y) + m[2] * z) + m[3]; }
__device__ inline double view_y(const double* m, double x, double y, double z) { return ((m[4] * x + m[5] * y) + m[6] * z) + m[7]; }
__device__ inline double view_z(const double* m, double x, double y, double z) { return ((m[8] * x + m[9] * y) + m[10] * z) + m[11]; }

// false: zv < z_near, the pair is rejected whatever xv and yv are.  zv is formed and tested first; xv and yv have no branch of their own here, so
// that the caller's is the only one: the compiler sinks them behind it, and a kernel's loop is instruction for instruction what it
// was with the test written out.
__device__ inline bool view_transform(const View& C, const double* m, double x, double y, double z, double& xv, double& yv,
                                      double& zv) {
    zv = view_z(m, x, y, z);
    const bool front = !(zv < C.z_near);
    xv = view_x(m, x, y, z);
    yv = view_y(m, x, y, z);
    return front;
}

// false: a projection that is not finite
__device__ inline bool view_project(double fx, double fy, double cx, double cy, double xv, double yv, double zv, double& u, double& v) {
    u = fx * xv / zv + cx;
    v = fy * yv / zv + cy;
    return isfinite(u) && isfinite(v);
}

__device__ inline bool view_inside(const View& C, double u, double v) { return u >= C.u_lo && u <= C.u_hi && v >= C.v_lo && v <= C.v_hi; }

// The warp of a position inside the box by the pose's lattice f [Ah][Aw][2]: the cell, the four anchor weights w00, w01, w10, w11,
// the warped position.  false: the warped position is not finite or outside the box.
__device__ inline bool view_warp(const View& C, const double* __restrict__ f, double u, double v, double* w, double& uw, double& vw,
                                 int& cell) {
    const double gu = u / C.S, gv = v / C.S;
    int cj = (int)floor(gu), ci = (int)floor(gv);         // u, v >= 0 here: margin >= 0
    cj = cj < C.Aw - 2 ? cj : C.Aw - 2;
    ci = ci < C.Ah - 2 ? ci : C.Ah - 2;
    const double a = gu - (double)cj, b = gv - (double)ci;
    w[0] = (1.0 - a) * (1.0 - b);
    w[1] = a * (1.0 - b);
    w[2] = (1.0 - a) * b;
    w[3] = a * b;
    const double* f0 = f + ((int64_t)ci * C.Aw + cj) * 2;
    const double* f1 = f0 + (int64_t)C.Aw * 2;
    uw = u + ((w[0] * f0[0] + w[1] * f0[2]) + (w[2] * f1[0] + w[3] * f1[2]));
    vw = v + ((w[0] * f0[1] + w[1] * f0[3]) + (w[2] * f1[1] + w[3] * f1[3]));
    if (!isfinite(uw) || !isfinite(vw)) return false;
    cell = ci * (C.Aw - 1) + cj;
    return view_inside(C, uw, vw);
}

// The four bilinear taps of a position inside an H x W image (u, v >= 0: margin >= 0), the far neighbours clamped to the image.
struct Taps {
    int ix0, iy0, ix1, iy1;
    double w00, w01, w10, w11;
};
__device__ inline Taps taps_of(double u, double v, int H, int W) {
    const double fx0 = floor(u), fy0 = floor(v);
    const double a = u - fx0, c = v - fy0;
    Taps t;
    t.ix0 = (int)fx0;
    t.iy0 = (int)fy0;
    t.ix1 = t.ix0 + 1 < W ? t.ix0 + 1 : W - 1;
    t.iy1 = t.iy0 + 1 < H ? t.iy0 + 1 : H - 1;
    t.w00 = (1.0 - a) * (1.0 - c);
    t.w01 = a * (1.0 - c);
    t.w10 = (1.0 - a) * c;
    t.w11 = a * c;
    return t;
}
__device__ inline double taps_mix(const Taps& t, double v00, double v01, double v10, double v11) {
    return (t.w00 * v00 + t.w01 * v01) + (t.w10 * v10 + t.w11 * v11);
}

// uint8 RGB frame -> the three channels in 1/65536 of a grey level
__device__ inline void sample_rgb(const uint8_t* __restrict__ img, int W, const Taps& t, int64_t* q) {
    const uint8_t* p00 = img + ((int64_t)t.iy0 * W + t.ix0) * 3;
    const uint8_t* p01 = img + ((int64_t)t.iy0 * W + t.ix1) * 3;
    const uint8_t* p10 = img + ((int64_t)t.iy1 * W + t.ix0) * 3;
    const uint8_t* p11 = img + ((int64_t)t.iy1 * W + t.ix1) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        q[ch] = (int64_t)rint(taps_mix(t, (double)p00[ch], (double)p01[ch], (double)p10[ch], (double)p11[ch]) * 65536.0);
}

// (G, gx, gy, 0) image of stin_colormap_gradients_u8 -> intensity in [0, 1] and its derivatives per pixel
__device__ inline void sample_gradients(const int4* __restrict__ img, int W, const Taps& t, double& I, double& dIdx, double& dIdy) {
    const int4 t00 = img[(int64_t)t.iy0 * W + t.ix0], t01 = img[(int64_t)t.iy0 * W + t.ix1];
    const int4 t10 = img[(int64_t)t.iy1 * W + t.ix0], t11 = img[(int64_t)t.iy1 * W + t.ix1];
    const double sI = taps_mix(t, (double)t00.x, (double)t01.x, (double)t10.x, (double)t11.x);
    const double sX = taps_mix(t, (double)t00.y, (double)t01.y, (double)t10.y, (double)t11.y);
    const double sY = taps_mix(t, (double)t00.z, (double)t01.z, (double)t10.z, (double)t11.z);
    I = sI / 255000.0;
    dIdx = sX / 2040000.0, dIdy = sY / 2040000.0;
}

// d intensity / d (rotation x, y, z, translation x, y, z) of a rigid increment of the extrinsic
__device__ inline void pose_jacobian(double xv, double yv, double zv, double fx, double fy, double dIdx, double dIdy, double* J) {
    const double iz = 1.0 / zv;
    const double v0 = (dIdx * fx) * iz;
    const double v1 = (dIdy * fy) * iz;
    const double v2 = -((v0 * xv + v1 * yv) * iz);
    J[0] = (-zv * v1) + yv * v2;
    J[1] = zv * v0 - xv * v2;
    J[2] = (-yv * v0) + xv * v1;
    J[3] = v0;
    J[4] = v1;
    J[5] = v2;
}

// The tail of the accumulate kernel.  A thread's poses ascend, so the `seen` bits of one word are gathered in a register and
// written when the word changes and once more at the end; ATOMIC: other chunks of poses add to the same vertex (split route).
template <bool ATOMIC> __device__ inline void seen_flush(uint32_t* row, int64_t word, uint32_t acc) {
    if (acc == 0u) return;
    if (ATOMIC) atomicOr(row + word, acc); else row[word] |= acc;
}
template <bool ATOMIC> __device__ inline void seen_mark(uint32_t* row, int64_t p, int64_t& word, uint32_t& acc) {
    if ((p >> 5) != word) {
        seen_flush<ATOMIC>(row, word, acc);
        word = p >> 5;
        acc = 0u;
    }
    acc |= 1u << (p & 31);
}
template <bool ATOMIC> __device__ inline void sums_commit(int64_t* sum, int32_t* count, int64_t s0, int64_t s1, int64_t s2, int32_t cnt) {
    if (ATOMIC) {
        unsigned long long* s = (unsigned long long*)sum;   // two's complement: the unsigned add is the signed add
        atomicAdd(s, (unsigned long long)s0);
        atomicAdd(s + 1, (unsigned long long)s1);
        atomicAdd(s + 2, (unsigned long long)s2);
        atomicAdd(count, cnt);
    } else {
        sum[0] += s0;
        sum[1] += s1;
        sum[2] += s2;
        *count += cnt;
    }
}
