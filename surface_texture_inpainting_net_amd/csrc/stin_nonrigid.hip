// Non-rigid colour-map optimisation on the device: a low-resolution warp lattice per frame on top of the rigid optimiser (Zhou &
// Koltun 2014, section 5; what Open3D's colour-map pipeline calls run_non_rigid_optimizer), for preprocessing.optimize_poses_nonrigid.
// Contract: include/stin_hip.h ("Non-rigid colour-map optimisation"); tests/_nonrigid_oracle.py restates it in numpy, pose-major,
// and agrees byte for byte.
//
//   accumulate: stin_nonrigid_accumulate_f64 is the warp mode of the frame colours' accumulate kernel and lives beside it in
//               stin_frames.hip; the pair test here (pair_of) and there are built from the same pieces of stin_view.h.
//   keys:       one thread per (vertex, pose): the pair test, the cell of the projection, one int64 key
//               (pose-in-batch cells + cell) << 31 | vertex, or the sentinel for a pair that does not contribute.  The caller sorts
//               the keys (rocPRIM through torch.sort): every (pose, cell) becomes one run of keys in ascending vertex id.
//   blocks:     one workgroup of 128 threads per (pose, cell).  It finds its run by two binary searches, then, 128 pairs at a time:
//               thread t computes pair t's (J[14], r) - projection, weights, warp, the three bilinear samples - into LDS, pair-major
//               with a row of 15 doubles (the readers of one pair hit 15 different banks); then thread i < 120 adds its product
//               z[a_i] z[b_i] over the staged pairs IN ORDER.  The sum of every entry is therefore the contract's: ascending
//               vertex id from +0.0, whatever the batching.  15 KB of LDS and two waves per workgroup: ten workgroups per CU.
// No float atomics.  Nothing is contracted (the file is built with -ffp-contract=off like every other).
#include "stin_view.h"

namespace {

constexpr int FB = 256;                                   // threads per workgroup: keys
constexpr int NB = 128;                                   // threads per workgroup = pairs per staging round: blocks
constexpr int LOCAL = 14;                                 // local unknowns: 6 of the pose, 2 x 4 of the cell's anchors
constexpr int ZW = LOCAL + 1;                             // a staged pair: J[14], r
constexpr int BLOCK = STIN_NONRIGID_BLOCK_DOUBLES;        // 105 + 14 + 1
constexpr int64_t SENTINEL = INT64_MAX;                   // the key of a pair that does not contribute
static_assert(BLOCK == LOCAL * (LOCAL + 1) / 2 + LOCAL + 1 && BLOCK <= NB, "one thread per entry of a block");

struct Pair {
    double xv, yv, zv, uw, vw;                            // the view, unwarped; the warped position
    double w[4];                                          // w00, w01, w10, w11
    int cell;
};

// The contract's pair test, minus the pose's validity and the visibility bit; f: the pose's flow [Ah][Aw][2].
__device__ inline bool pair_of(const View& C, const double* __restrict__ m, const double* __restrict__ f, double x, double y, double z,
                               Pair& o) {
    double u, v;
    if (!view_transform(C, m, x, y, z, o.xv, o.yv, o.zv)) return false;
    if (!view_project(C.fx, C.fy, C.cx, C.cy, o.xv, o.yv, o.zv, u, v)) return false;
    if (!view_inside(C, u, v)) return false;
    return view_warp(C, f, u, v, o.w, o.uw, o.vw, o.cell);
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
                double I, dIdx, dIdy;
                sample_gradients(img, A.W, taps_of(q.uw, q.vw, A.H, A.W), I, dIdx, dIdy);   // margin >= 1: the taps are in [1, W - 2], [1, H - 2]
                pose_jacobian(q.xv, q.yv, q.zv, A.C.fx, A.C.fy, dIdx, dIdy, z);
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

inline int64_t cells_of(int H, int W, int S) { return (int64_t)(anchors_of(H, S) - 1) * (anchors_of(W, S) - 1); }

}  // namespace

extern "C" size_t stin_nonrigid_workspace_bytes(int64_t N, int B, int H, int W, int lattice_step) {
    if (N < 0 || N >= (int64_t)INT32_MAX || B < 0 || B > STIN_FRAMES_MAX_BATCH || !frame_size_ok(H, W, 2) || lattice_step < 1) return 0;
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
    STIN_REQUIRE(frame_size_ok(H, W, 2) && lattice_step >= 1 && margin >= 1 && z_near > 0.0, STIN_E_SIZE);
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
