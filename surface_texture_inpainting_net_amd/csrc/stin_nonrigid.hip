// Non-rigid colour-map optimisation on the device: a low-resolution warp lattice per frame on top of the rigid optimiser (Zhou &
// Koltun 2014, section 5; what Open3D's colour-map pipeline calls run_non_rigid_optimizer), for preprocessing.optimize_poses_nonrigid.
// Contract: include/stin_hip.h ("Non-rigid colour-map optimisation"); tests/_nonrigid_oracle.py restates it in numpy, pose-major,
// and agrees byte for byte.
//
//   accumulate: stin_frames.hip's bits-mode kernel with the colour frame sampled at the warped position: one thread per vertex, a
//               loop over a chunk of the batch's poses, three int64 sums and a count in registers; owner route (plain stores) or
//               split route (integer atomics), identical bits.
//   keys:       one thread per (vertex, pose): the pair test, the cell of the projection, one int64 key
//               (pose-in-batch cells + cell) << 31 | vertex, or the sentinel for a pair that does not contribute.  The caller sorts
//               the keys (rocPRIM through torch.sort): every (pose, cell) becomes one run of keys in ascending vertex id.
//   blocks:     one workgroup of 128 threads per (pose, cell).  It finds its run by two binary searches, then, 128 pairs at a time:
//               thread t computes pair t's (J[14], r) - projection, weights, warp, the three bilinear samples - into LDS, pair-major
//               with a row of 15 doubles (the readers of one pair hit 15 different banks); then thread i < 120 adds its product
//               z[a_i] z[b_i] over the staged pairs IN ORDER.  The sum of every entry is therefore the contract's: ascending
//               vertex id from +0.0, whatever the batching.  15 KB of LDS and two waves per workgroup: ten workgroups per CU.
// No float atomics.  Nothing is contracted (the file is built with -ffp-contract=off like every other).
#include "stin_common.h"

namespace {

constexpr int FB = 256;                                   // threads per workgroup: accumulate, keys
constexpr int NB = 128;                                   // threads per workgroup = pairs per staging round: blocks
constexpr int LOCAL = 14;                                 // local unknowns: 6 of the pose, 2 x 4 of the cell's anchors
constexpr int ZW = LOCAL + 1;                             // a staged pair: J[14], r
constexpr int BLOCK = STIN_NONRIGID_BLOCK_DOUBLES;        // 105 + 14 + 1
constexpr int SPLIT_MIN_POSES = 8;                        // poses per chunk of the split route, at least
constexpr int64_t FILL_GROUPS = 1024;                     // workgroups that fill the chip (256 CUs x 4)
constexpr int64_t SENTINEL = INT64_MAX;                   // the key of a pair that does not contribute
static_assert(BLOCK == LOCAL * (LOCAL + 1) / 2 + LOCAL + 1 && BLOCK <= NB, "one thread per entry of a block");

inline bool size_ok(int H, int W) { return H >= 2 && W >= 2 && H <= STIN_FRAMES_MAX_SIZE && W <= STIN_FRAMES_MAX_SIZE; }
inline int anchors_of(int n, int S) { return (n - 1 + S - 1) / S + 1; }      // ceil((n - 1) / S) + 1

struct View {                                             // what the pair test and the warp need besides the pose and the vertex
    double fx, fy, cx, cy, z_near;
    double u_lo, u_hi, v_lo, v_hi;                        // margin, W - 1 - margin, margin, H - 1 - margin
    double S;
    int Ah, Aw;
};

struct Pair {
    double xv, yv, zv, uw, vw;                            // the view, unwarped; the warped position
    double w[4];                                          // w00, w01, w10, w11
    int cell;
};

// The contract's pair test, minus the pose's validity and the visibility bit; f: the pose's flow [Ah][Aw][2].
__device__ inline bool pair_of(const View& C, const double* __restrict__ m, const double* __restrict__ f, double x, double y, double z,
                               Pair& o) {
    o.zv = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
    if (o.zv < C.z_near) return false;
    o.xv = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    o.yv = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    const double u = C.fx * o.xv / o.zv + C.cx, v = C.fy * o.yv / o.zv + C.cy;
    if (!isfinite(u) || !isfinite(v)) return false;
    if (!(u >= C.u_lo && u <= C.u_hi && v >= C.v_lo && v <= C.v_hi)) return false;
    const double gu = u / C.S, gv = v / C.S;
    int cj = (int)floor(gu), ci = (int)floor(gv);         // u, v >= 0 here: margin >= 0
    cj = cj < C.Aw - 2 ? cj : C.Aw - 2;
    ci = ci < C.Ah - 2 ? ci : C.Ah - 2;
    const double a = gu - (double)cj, b = gv - (double)ci;
    o.w[0] = (1.0 - a) * (1.0 - b);
    o.w[1] = a * (1.0 - b);
    o.w[2] = (1.0 - a) * b;
    o.w[3] = a * b;
    const double* f0 = f + ((int64_t)ci * C.Aw + cj) * 2;
    const double* f1 = f0 + (int64_t)C.Aw * 2;
    o.uw = u + ((o.w[0] * f0[0] + o.w[1] * f0[2]) + (o.w[2] * f1[0] + o.w[3] * f1[2]));
    o.vw = v + ((o.w[0] * f0[1] + o.w[1] * f0[3]) + (o.w[2] * f1[1] + o.w[3] * f1[3]));
    if (!isfinite(o.uw) || !isfinite(o.vw)) return false;
    if (!(o.uw >= C.u_lo && o.uw <= C.u_hi && o.vw >= C.v_lo && o.vw <= C.v_hi)) return false;
    o.cell = ci * (C.Aw - 1) + cj;
    return true;
}

// ------------------------------------------------------------------------------------------------------------------ accumulate
struct AccArgs {
    const double* vertices;
    const double* RT;
    const uint8_t* valid;
    const uint8_t* color;
    const double* flow;
    const uint32_t* bits;
    int64_t* sum;
    int32_t* count;
    uint32_t* seen;
    int64_t N, first_pose, words, seen_words;
    View C;
    int B, H, W, per_chunk;
};

template <bool ATOMIC> __device__ inline void seen_flush(const AccArgs& A, int64_t v, int64_t word, uint32_t acc) {
    if (acc == 0u) return;
    uint32_t* w = A.seen + v * A.seen_words + word;
    if (ATOMIC) atomicOr(w, acc); else *w |= acc;
}

template <bool ATOMIC> __global__ __launch_bounds__(FB) void k_nonrigid_accumulate(const AccArgs A) {
    const int64_t v = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (v >= A.N) return;
    const int b0 = (int)blockIdx.y * A.per_chunk;
    const int b1 = b0 + A.per_chunk < A.B ? b0 + A.per_chunk : A.B;
    const double x = A.vertices[3 * v], y = A.vertices[3 * v + 1], z = A.vertices[3 * v + 2];
    const uint32_t* brow = A.bits + v * A.words;
    const int64_t per_flow = (int64_t)A.C.Ah * A.C.Aw * 2;
    int64_t s0 = 0, s1 = 0, s2 = 0;
    int32_t cnt = 0;
    uint32_t sacc = 0u;
    int64_t sword = 0;
    for (int b = b0; b < b1; ++b) {
        if (!A.valid[b]) continue;
        const int64_t p = A.first_pose + b;
        if (!((brow[p >> 5] >> (p & 31)) & 1u)) continue;
        Pair q;
        if (!pair_of(A.C, A.RT + (int64_t)b * 12, A.flow + (int64_t)b * per_flow, x, y, z, q)) continue;
        const double fx0 = floor(q.uw), fy0 = floor(q.vw);
        const double a = q.uw - fx0, c = q.vw - fy0;
        const int ix0 = (int)fx0, iy0 = (int)fy0;         // in [0, W - 1], [0, H - 1]: margin >= 0
        const int ix1 = ix0 + 1 < A.W ? ix0 + 1 : A.W - 1, iy1 = iy0 + 1 < A.H ? iy0 + 1 : A.H - 1;
        const uint8_t* img = A.color + (int64_t)b * A.H * A.W * 3;
        const uint8_t* p00 = img + ((int64_t)iy0 * A.W + ix0) * 3;
        const uint8_t* p01 = img + ((int64_t)iy0 * A.W + ix1) * 3;
        const uint8_t* p10 = img + ((int64_t)iy1 * A.W + ix0) * 3;
        const uint8_t* p11 = img + ((int64_t)iy1 * A.W + ix1) * 3;
        const double w00 = (1.0 - a) * (1.0 - c), w01 = a * (1.0 - c), w10 = (1.0 - a) * c, w11 = a * c;
        int64_t qs[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const double val = (w00 * (double)p00[ch] + w01 * (double)p01[ch]) + (w10 * (double)p10[ch] + w11 * (double)p11[ch]);
            qs[ch] = (int64_t)rint(val * 65536.0);
        }
        s0 += qs[0];
        s1 += qs[1];
        s2 += qs[2];
        cnt += 1;
        if (A.seen != nullptr) {
            if ((p >> 5) != sword) {
                seen_flush<ATOMIC>(A, v, sword, sacc);
                sword = p >> 5;
                sacc = 0u;
            }
            sacc |= 1u << (p & 31);
        }
    }
    if (cnt == 0) return;
    if (A.seen != nullptr) seen_flush<ATOMIC>(A, v, sword, sacc);
    if (ATOMIC) {
        unsigned long long* s = (unsigned long long*)(A.sum + 3 * v);   // two's complement: the unsigned add is the signed add
        atomicAdd(s, (unsigned long long)s0);
        atomicAdd(s + 1, (unsigned long long)s1);
        atomicAdd(s + 2, (unsigned long long)s2);
        atomicAdd(A.count + v, cnt);
    } else {
        A.sum[3 * v] += s0;
        A.sum[3 * v + 1] += s1;
        A.sum[3 * v + 2] += s2;
        A.count[v] += cnt;
    }
}

// ------------------------------------------------------------------------------------------------------------ keys and blocks
struct NormalArgs {
    const double* vertices;
    const double* RT;
    const uint8_t* valid;
    const int4* images;
    const double* flow;
    const uint32_t* bits;
    const double* proxy;
    int64_t* keys;                                        // [B][N]: written by the key kernel, read SORTED by the block kernel
    double* blocks;                                       // [B][cells][BLOCK]
    int32_t* counts;                                      // [B][cells]
    int64_t N, first_pose, words, cells;
    View C;
    int B, H, W;
};

__global__ __launch_bounds__(FB) void k_nonrigid_keys(const NormalArgs A) {
    const int64_t v = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (v >= A.N) return;
    const int b = (int)blockIdx.y;
    const int64_t p = A.first_pose + b;
    int64_t key = SENTINEL;
    if (A.valid[b] && ((A.bits[v * A.words + (p >> 5)] >> (p & 31)) & 1u)) {
        Pair q;
        if (pair_of(A.C, A.RT + (int64_t)b * 12, A.flow + (int64_t)b * A.C.Ah * A.C.Aw * 2, A.vertices[3 * v], A.vertices[3 * v + 1],
                    A.vertices[3 * v + 2], q))
            key = (((int64_t)b * A.cells + q.cell) << 31) | v;
    }
    A.keys[(int64_t)b * A.N + v] = key;
}

// The first index in sorted keys[0, n) whose key is >= want.
__device__ inline int64_t lower_bound(const int64_t* __restrict__ keys, int64_t n, int64_t want) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < want) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(NB) void k_nonrigid_blocks(const NormalArgs A) {
    __shared__ double st[NB][ZW];
    const int t = threadIdx.x;
    const int64_t seg = blockIdx.x;                       // pose-in-batch cells + cell
    const int b = (int)(seg / A.cells);
    const int64_t total = (int64_t)A.B * A.N;
    const int64_t lo = lower_bound(A.keys, total, seg << 31), hi = lower_bound(A.keys, total, (seg + 1) << 31);
    // entry t of the block is z[ia] z[ib] with z = (J[0 .. 13], r): the triangle (105), J r (14), r r (1)
    int ia = 0, ib = 0;
    if (t < BLOCK - LOCAL - 1) {
        int rem = t;
        while (rem >= LOCAL - ia) {
            rem -= LOCAL - ia;
            ++ia;
        }
        ib = ia + rem;
    } else if (t < BLOCK - 1) {
        ia = t - (BLOCK - LOCAL - 1);
        ib = LOCAL;
    } else {
        ia = ib = LOCAL;
    }
    const double* m = A.RT + (int64_t)b * 12;
    const double* f = A.flow + (int64_t)b * A.C.Ah * A.C.Aw * 2;
    const int4* img = A.images + (int64_t)b * A.H * A.W;
    double acc = 0.0;
    for (int64_t base = lo; base < hi; base += NB) {
        const int n = hi - base < NB ? (int)(hi - base) : NB;
        if (t < n) {
            const int64_t v = A.keys[base + t] & (int64_t)0x7fffffff;
            Pair q;
            double* z = st[t];
            if (v < A.N && pair_of(A.C, m, f, A.vertices[3 * v], A.vertices[3 * v + 1], A.vertices[3 * v + 2], q)) {
                const double fx0 = floor(q.uw), fy0 = floor(q.vw);
                const double a = q.uw - fx0, c = q.vw - fy0;
                const int ix0 = (int)fx0, iy0 = (int)fy0; // in [1, W - 2], [1, H - 2]: margin >= 1
                const int ix1 = ix0 + 1 < A.W ? ix0 + 1 : A.W - 1, iy1 = iy0 + 1 < A.H ? iy0 + 1 : A.H - 1;
                const int4 t00 = img[(int64_t)iy0 * A.W + ix0], t01 = img[(int64_t)iy0 * A.W + ix1];
                const int4 t10 = img[(int64_t)iy1 * A.W + ix0], t11 = img[(int64_t)iy1 * A.W + ix1];
                const double w00 = (1.0 - a) * (1.0 - c), w01 = a * (1.0 - c), w10 = (1.0 - a) * c, w11 = a * c;
                const double sI = (w00 * (double)t00.x + w01 * (double)t01.x) + (w10 * (double)t10.x + w11 * (double)t11.x);
                const double sX = (w00 * (double)t00.y + w01 * (double)t01.y) + (w10 * (double)t10.y + w11 * (double)t11.y);
                const double sY = (w00 * (double)t00.z + w01 * (double)t01.z) + (w10 * (double)t10.z + w11 * (double)t11.z);
                const double I = sI / 255000.0, dIdx = sX / 2040000.0, dIdy = sY / 2040000.0;
                const double iz = 1.0 / q.zv;
                const double v0 = (dIdx * A.C.fx) * iz;
                const double v1 = (dIdy * A.C.fy) * iz;
                const double v2 = -((v0 * q.xv + v1 * q.yv) * iz);
                z[0] = (-q.zv * v1) + q.yv * v2;
                z[1] = q.zv * v0 - q.xv * v2;
                z[2] = (-q.yv * v0) + q.xv * v1;
                z[3] = v0;
                z[4] = v1;
                z[5] = v2;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    z[6 + 2 * k] = dIdx * q.w[k];
                    z[7 + 2 * k] = dIdy * q.w[k];
                }
                z[LOCAL] = I - A.proxy[v];
            } else {                                      // keys that were not made from these inputs: the pair adds +0.0
#pragma unroll
                for (int k = 0; k < ZW; ++k) z[k] = 0.0;
            }
        }
        __syncthreads();
        if (t < BLOCK)
            for (int p = 0; p < n; ++p) acc += st[p][ia] * st[p][ib];
        __syncthreads();
    }
    if (t < BLOCK) A.blocks[seg * BLOCK + t] = acc;
    if (t == BLOCK) A.counts[seg] = (int32_t)(hi - lo);
}

inline View view_of(const double* camera, double z_near, int margin, int H, int W, int S) {
    View C;
    C.fx = camera[0]; C.fy = camera[1]; C.cx = camera[2]; C.cy = camera[3]; C.z_near = z_near;
    C.u_lo = (double)margin; C.u_hi = (double)(W - 1 - margin); C.v_lo = (double)margin; C.v_hi = (double)(H - 1 - margin);
    C.S = (double)S;
    C.Ah = anchors_of(H, S);
    C.Aw = anchors_of(W, S);
    return C;
}

inline int64_t cells_of(int H, int W, int S) { return (int64_t)(anchors_of(H, S) - 1) * (anchors_of(W, S) - 1); }

}  // namespace

extern "C" int stin_nonrigid_accumulate_f64(const double* vertices, int64_t N, const double* RT, const uint8_t* valid, int B,
                                            int64_t first_pose, const uint8_t* color, int H, int W, const double* flow, int lattice_step,
                                            const double* camera, double z_near, const uint32_t* bits, int64_t words, int margin,
                                            int route, int64_t* sum, int32_t* count, uint32_t* seen, int64_t seen_words,
                                            stin_stream_t stream_) {
    STIN_REQUIRE(camera != nullptr, STIN_E_NULL);
    STIN_REQUIRE(N >= 0 && N < (int64_t)INT32_MAX && B >= 0 && B <= STIN_FRAMES_MAX_BATCH, STIN_E_SIZE);
    STIN_REQUIRE(first_pose >= 0 && first_pose + B < (int64_t)INT32_MAX, STIN_E_SIZE);
    STIN_REQUIRE(size_ok(H, W) && lattice_step >= 1 && margin >= 0 && z_near > 0.0, STIN_E_SIZE);
    STIN_REQUIRE(route == STIN_FRAMES_ROUTE_AUTO || route == STIN_FRAMES_ROUTE_OWNER || route == STIN_FRAMES_ROUTE_SPLIT, STIN_E_SIZE);
    const int64_t need_words = (first_pose + B + 31) / 32;
    STIN_REQUIRE(words >= need_words || N == 0 || B == 0, STIN_E_SIZE);
    if (seen != nullptr) STIN_REQUIRE(seen_words >= need_words, STIN_E_SIZE);
    if (N == 0 || B == 0) return STIN_OK;
    STIN_REQUIRE(vertices && RT && valid && color && flow && bits && sum && count, STIN_E_NULL);
    stin_clear_stale_error();
    AccArgs A;
    A.vertices = vertices; A.RT = RT; A.valid = valid; A.color = color; A.flow = flow; A.bits = bits;
    A.sum = sum; A.count = count; A.seen = seen;
    A.N = N; A.first_pose = first_pose; A.words = words; A.seen_words = seen_words;
    A.C = view_of(camera, z_near, margin, H, W, lattice_step);
    A.B = B; A.H = H; A.W = W;
    // The route, from N and B alone, as stin_frames_accumulate_f64 decides it.
    const int64_t groups = (N + FB - 1) / FB;
    int64_t chunks = (FILL_GROUPS + groups - 1) / groups;
    const int64_t most = (B + SPLIT_MIN_POSES - 1) / SPLIT_MIN_POSES;
    if (chunks > most) chunks = most;
    if (route == STIN_FRAMES_ROUTE_OWNER) chunks = 1;
    if (route == STIN_FRAMES_ROUTE_SPLIT && chunks < 2) chunks = B < 2 ? 1 : 2;
    const bool atomic = route == STIN_FRAMES_ROUTE_SPLIT || chunks > 1;
    A.per_chunk = (int)((B + chunks - 1) / chunks);
    const dim3 grid((unsigned)groups, (unsigned)((B + A.per_chunk - 1) / A.per_chunk));
    if (atomic) hipLaunchKernelGGL((k_nonrigid_accumulate<true>), grid, dim3(FB), 0, (hipStream_t)stream_, A);
    else hipLaunchKernelGGL((k_nonrigid_accumulate<false>), grid, dim3(FB), 0, (hipStream_t)stream_, A);
    return stin_launch_status();
}

extern "C" size_t stin_nonrigid_workspace_bytes(int64_t N, int B, int H, int W, int lattice_step) {
    if (N < 0 || N >= (int64_t)INT32_MAX || B < 0 || B > STIN_FRAMES_MAX_BATCH || !size_ok(H, W) || lattice_step < 1) return 0;
    if ((int64_t)(B > 0 ? B : 1) * cells_of(H, W, lattice_step) >= (int64_t)INT32_MAX) return 0;
    return (size_t)(N > 0 ? N : 1) * (size_t)(B > 0 ? B : 1) * sizeof(int64_t);      // not rounded: a sorted copy is exactly this long
}

namespace {

// The checks and the argument record that the two halves of the normal equations share.
int normal_args(NormalArgs& A, const double* vertices, int64_t N, const double* RT, const uint8_t* valid, int B, int64_t first_pose,
                int H, int W, const double* flow, int lattice_step, const double* camera, double z_near, int margin, void* keys,
                size_t keys_bytes) {
    STIN_REQUIRE(camera != nullptr, STIN_E_NULL);
    STIN_REQUIRE(N >= 0 && N < (int64_t)INT32_MAX && B >= 0 && B <= STIN_FRAMES_MAX_BATCH, STIN_E_SIZE);
    STIN_REQUIRE(first_pose >= 0 && first_pose + B < (int64_t)INT32_MAX, STIN_E_SIZE);
    STIN_REQUIRE(size_ok(H, W) && lattice_step >= 1 && margin >= 1 && z_near > 0.0, STIN_E_SIZE);
    STIN_REQUIRE(stin_nonrigid_workspace_bytes(N, B, H, W, lattice_step) != 0, STIN_E_SIZE);
    if (B == 0) return STIN_OK;
    if (N > 0) {
        STIN_REQUIRE(vertices && RT && valid && flow, STIN_E_NULL);
        STIN_REQUIRE(keys != nullptr && keys_bytes >= stin_nonrigid_workspace_bytes(N, B, H, W, lattice_step), STIN_E_WORKSPACE);
        STIN_REQUIRE(((uintptr_t)keys & 7u) == 0, STIN_E_SIZE);
    }
    A.vertices = vertices; A.RT = RT; A.valid = valid; A.flow = flow; A.keys = (int64_t*)keys;
    A.images = nullptr; A.bits = nullptr; A.proxy = nullptr; A.blocks = nullptr; A.counts = nullptr;
    A.N = N; A.first_pose = first_pose; A.words = 0; A.cells = cells_of(H, W, lattice_step);
    A.C = view_of(camera, z_near, margin, H, W, lattice_step);
    A.B = B; A.H = H; A.W = W;
    return STIN_OK;
}

}  // namespace

extern "C" int stin_nonrigid_keys_f64(const double* vertices, int64_t N, const double* RT, const uint8_t* valid, int B,
                                      int64_t first_pose, int H, int W, const double* flow, int lattice_step, const double* camera,
                                      double z_near, const uint32_t* bits, int64_t words, int margin, void* keys, size_t keys_bytes,
                                      stin_stream_t stream_) {
    NormalArgs A;
    const int rc = normal_args(A, vertices, N, RT, valid, B, first_pose, H, W, flow, lattice_step, camera, z_near, margin, keys, keys_bytes);
    if (rc != STIN_OK || B == 0 || N == 0) return rc;
    STIN_REQUIRE(bits != nullptr, STIN_E_NULL);
    STIN_REQUIRE(words >= (first_pose + B + 31) / 32, STIN_E_SIZE);
    A.bits = bits;
    A.words = words;
    stin_clear_stale_error();
    hipLaunchKernelGGL(k_nonrigid_keys, dim3((unsigned)((N + FB - 1) / FB), (unsigned)B), dim3(FB), 0, (hipStream_t)stream_, A);
    return stin_launch_status();
}

extern "C" int stin_nonrigid_normal_f64(const double* vertices, int64_t N, const double* RT, const uint8_t* valid, int B,
                                        int64_t first_pose, const int32_t* images, int H, int W, const double* flow, int lattice_step,
                                        const double* camera, double z_near, int margin, const double* proxy, const void* sorted_keys,
                                        size_t keys_bytes, double* blocks, int32_t* counts, stin_stream_t stream_) {
    NormalArgs A;
    const int rc = normal_args(A, vertices, N, RT, valid, B, first_pose, H, W, flow, lattice_step, camera, z_near, margin,
                               (void*)sorted_keys, keys_bytes);
    if (rc != STIN_OK || B == 0) return rc;
    STIN_REQUIRE(blocks != nullptr && counts != nullptr, STIN_E_NULL);
    if (N > 0) {
        STIN_REQUIRE(images != nullptr && proxy != nullptr, STIN_E_NULL);
        STIN_REQUIRE(((uintptr_t)images & 15u) == 0, STIN_E_SIZE);
    }
    A.images = (const int4*)images;
    A.proxy = proxy;
    A.blocks = blocks;
    A.counts = counts;
    stin_clear_stale_error();
    hipLaunchKernelGGL(k_nonrigid_blocks, dim3((unsigned)((int64_t)B * A.cells)), dim3(NB), 0, (hipStream_t)stream_, A);
    return stin_launch_status();
}
