// Surface samples: area-uniform points on a triangle mesh, Poisson-disk thinning in index order, first occurrences of a stream
// of vertex ids - the sampler the reference's process_frame_circles left as a TODO (preprocessing/
// observed_texture_map_generation.py:545-562).  Contract: include/stin_hip.h ("Surface samples").
//
//   weights:  A2_f = |e1 x e2| in fp64 (two rounded products and one subtraction per component, IEEE sqrt), Amax = max A2 through
//             an integer atomicMax of the bit pattern (order-free), W_f = floor(ldexp(A2_f, 40 - e)) with (_, e) = frexp(Amax):
//             integers below 2^40 whose rocPRIM inclusive scan is the same bytes on any schedule.
//   samples:  one thread per sample: three counter hashes, u = mulhi(r0, T), the first face with cum[f] > u by binary search,
//             the square-root barycentric map.  Sample i depends on (seed, first + i) only.
//   poisson:  candidate i is accepted iff no accepted j < i lies closer than r.  A uniform grid of edge r (1 + 2^-20) (one 63-bit
//             key per candidate, a stable radix sort) gives every candidate the nine runs of the sorted order that hold its 27
//             cells; decision rounds (ordinary launches, one state byte per candidate) settle every candidate whose earlier
//             conflicts are settled.  States only move from undecided to their final value, so what a thread reads of the same
//             round changes the number of rounds and nothing else.  No kernel waits for another workgroup.
//   first:    keep[i] = (i is the lowest stream position of ids[i]): an integer atomicMin per vertex, then one compare.
#include <cstring>
#include <rocprim/rocprim.hpp>
#include "stin_common.h"

namespace {

constexpr int T = 256;
typedef unsigned long long u64;
constexpr u64 GOLDEN = 0x9E3779B97F4A7C15ull;
constexpr int64_t MAX_CELLS = (int64_t)1 << 21;        // per axis: three coordinates share one 63-bit key

constexpr long long SURF_BAD_INDEX = 1;       // a face index outside [0, N): the face has weight 0
constexpr long long SURF_NOT_FINITE = 2;      // a non-finite vertex (or area) of a referenced face: weight 0
constexpr long long SURF_NO_WEIGHT = 4;       // the weights sum to 0: nothing was drawn
constexpr long long PD_NOT_FINITE = 1;        // a non-finite candidate
constexpr long long PD_TOO_MANY_CELLS = 2;    // more than 2^21 cells along an axis

enum : uint8_t { UNDECIDED = 0, ACCEPTED = 1, REJECTED = 2 };

inline unsigned grid_for(int64_t n) { return (unsigned)((n + T - 1) / T); }

__device__ inline uint8_t ld_agent(const uint8_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void st_agent(uint8_t* p, uint8_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// -------------------------------------------------------------------------------------------------------------------- weights
// state: [0] bit pattern of Amax, [1] flags, [2] T (total weight), [3] reserved
__global__ __launch_bounds__(T) void k_face_area(const double* __restrict__ V, int64_t N, const int64_t* __restrict__ faces, int64_t F,
                                                 double* __restrict__ a2, long long* __restrict__ state) {
    const int64_t f = (int64_t)blockIdx.x * T + threadIdx.x;
    if (f >= F) return;
    const int64_t ia = faces[f * 3 + 0], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
    double area = 0.0;
    if (ia < 0 || ia >= N || ib < 0 || ib >= N || ic < 0 || ic >= N) {
        atomicOr(reinterpret_cast<u64*>(state + 1), (u64)SURF_BAD_INDEX);
    } else {
        double e1[3], e2[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double a = V[ia * 3 + d];
            e1[d] = V[ib * 3 + d] - a;
            e2[d] = V[ic * 3 + d] - a;
        }
        const double nx = e1[1] * e2[2] - e1[2] * e2[1];
        const double ny = e1[2] * e2[0] - e1[0] * e2[2];
        const double nz = e1[0] * e2[1] - e1[1] * e2[0];
        area = sqrt((nx * nx + ny * ny) + nz * nz);
        if (!(area < 1.0e308)) {                           // inf or nan: a non-finite vertex, or an overflow of the products
            atomicOr(reinterpret_cast<u64*>(state + 1), (u64)SURF_NOT_FINITE);
            area = 0.0;
        }
    }
    a2[f] = area;
    // non-negative doubles order like their bit patterns
    if (area > 0.0) atomicMax(reinterpret_cast<u64*>(state), (u64)__double_as_longlong(area));
}

__global__ __launch_bounds__(T) void k_face_weight(const double* __restrict__ a2, int64_t F, const long long* __restrict__ state,
                                                   int64_t* __restrict__ w) {
    const int64_t f = (int64_t)blockIdx.x * T + threadIdx.x;
    if (f >= F) return;
    const double amax = __longlong_as_double(state[0]);
    int e = 0;
    (void)frexp(amax, &e);                                 // amax = m 2^e, m in [0.5, 1): a2 2^(40 - e) < 2^40
    w[f] = amax > 0.0 ? (int64_t)floor(ldexp(a2[f], 40 - e)) : 0;
}

__global__ void k_total(const int64_t* __restrict__ cum, int64_t F, long long* __restrict__ state) {
    if (threadIdx.x == 0 && blockIdx.x == 0) state[2] = F > 0 ? cum[F - 1] : 0;
}

// -------------------------------------------------------------------------------------------------------------------- samples
__global__ __launch_bounds__(T) void k_sample(const double* __restrict__ V, int64_t N, const int64_t* __restrict__ faces, int64_t F,
                                              const int64_t* __restrict__ cum, int64_t n, u64 seed, u64 first,
                                              double* __restrict__ points, int64_t* __restrict__ face_out, double* __restrict__ bary,
                                              long long* __restrict__ state) {
    const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
    if (i >= n) return;
    const int64_t total = F > 0 ? cum[F - 1] : 0;
    if (total <= 0) {
        if (i == 0) atomicOr(reinterpret_cast<u64*>(state + 1), (u64)SURF_NO_WEIGHT);
        return;
    }
    const u64 base = stin_mix64(seed + GOLDEN);
    const u64 c = 3ull * (first + (u64)i);
    const u64 r0 = stin_mix64(base + c * GOLDEN), r1 = stin_mix64(base + (c + 1ull) * GOLDEN), r2 = stin_mix64(base + (c + 2ull) * GOLDEN);
    const int64_t u = (int64_t)__umul64hi(r0, (u64)total);             // in [0, total)
    int64_t lo = 0, hi = F - 1;                            // first f with cum[f] > u (cum[F - 1] = total > u)
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (cum[mid] > u) hi = mid;
        else lo = mid + 1;
    }
    const int64_t f = lo;
    const int64_t ia = faces[f * 3 + 0], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
    if (ia < 0 || ia >= N || ib < 0 || ib >= N || ic < 0 || ic >= N) return;      // (such a face has weight 0: never drawn)
    const double x1 = (double)(r1 >> 11) * 0x1.0p-53, x2 = (double)(r2 >> 11) * 0x1.0p-53;
    const double s = sqrt(x1);
    const double b0 = 1.0 - s, b1 = s * (1.0 - x2), b2 = s * x2;
#pragma unroll
    for (int d = 0; d < 3; ++d) points[i * 3 + d] = (b0 * V[ia * 3 + d] + b1 * V[ib * 3 + d]) + b2 * V[ic * 3 + d];
    face_out[i] = f;
    bary[i * 3 + 0] = b0;
    bary[i * 3 + 1] = b1;
    bary[i * 3 + 2] = b2;
}

// -------------------------------------------------------------------------------------------------------------------- poisson
// doubles -> uint64 keys of the same order (atomicMin / atomicMax on integers: order-free)
__device__ inline u64 ordered_bits(double v) {
    const u64 b = (u64)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ inline double from_ordered_bits(u64 k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}

// state: [0..2] ordered bits of the minimum, [3..5] of the maximum, [6] flags, [7] reserved
__global__ void k_pd_init(u64* __restrict__ state) {
    if (threadIdx.x < 8) state[threadIdx.x] = threadIdx.x < 3 ? ~0ull : 0ull;
}

__global__ __launch_bounds__(T) void k_pd_bounds(const double* __restrict__ P, int64_t C, u64* __restrict__ state) {
    const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
    const bool live = i < C;
    u64 lo[3], hi[3];
    bool bad = false;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double v = live ? P[i * 3 + d] : 0.0;
        const bool fin = fabs(v) < 1.0e308 * 10.0;         // false for inf and nan
        bad |= live && !fin;
        lo[d] = (live && fin) ? ordered_bits(v) : ~0ull;
        hi[d] = (live && fin) ? ordered_bits(v) : 0ull;
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        for (int o = STIN_WAVE / 2; o > 0; o >>= 1) {
            const u64 a = __shfl_xor(lo[d], o, STIN_WAVE), b = __shfl_xor(hi[d], o, STIN_WAVE);
            lo[d] = a < lo[d] ? a : lo[d];
            hi[d] = b > hi[d] ? b : hi[d];
        }
    }
    if ((threadIdx.x & (STIN_WAVE - 1)) == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            if (lo[d] != ~0ull) atomicMin(state + d, lo[d]);
            if (hi[d] != 0ull) atomicMax(state + 3 + d, hi[d]);
        }
    }
    if (bad) atomicOr(state + 6, (u64)PD_NOT_FINITE);
}

// cell coordinate of v along an axis with origin o: floor((v - o) / h); -1 when it cannot be used
__device__ inline int64_t cell_of(double v, double o, double h) {
    const double q = floor((v - o) / h);
    return (q >= 0.0 && q < (double)MAX_CELLS) ? (int64_t)q : -1;
}

__global__ __launch_bounds__(T) void k_pd_keys(const double* __restrict__ P, int64_t C, double h, u64* __restrict__ state,
                                               u64* __restrict__ keys, int32_t* __restrict__ ids) {
    const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
    if (i >= C) return;
    ids[i] = (int32_t)i;
    u64 key = 0;
    bool bad = false;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double v = P[i * 3 + d];
        int64_t c = -1;
        if (fabs(v) < 1.0e308 * 10.0) c = cell_of(v, from_ordered_bits(state[d]), h);
        bad |= c < 0;
        key = (key << 21) | (u64)(c < 0 ? 0 : c);
    }
    if (bad && !(state[6] & (u64)PD_NOT_FINITE)) atomicOr(state + 6, (u64)PD_TOO_MANY_CELLS);
    keys[i] = key;
}

__device__ inline int64_t lower_bound(const u64* __restrict__ keys, int64_t n, u64 key) {      // first position with keys[.] >= key
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// candidate i: the nine runs [beg, end) of the sorted order that hold the cells (cx + dx, cy + dy, cz - 1 .. cz + 1) - the three
// cells of a run are consecutive keys.  runs: int32 [C][18].
__global__ __launch_bounds__(T) void k_pd_runs(const double* __restrict__ P, int64_t C, double h, const u64* __restrict__ state,
                                               const u64* __restrict__ sorted, int32_t* __restrict__ runs) {
    const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
    if (i >= C) return;
    int64_t c[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) c[d] = cell_of(P[i * 3 + d], from_ordered_bits(state[d]), h);
    const bool usable = state[6] == 0 && c[0] >= 0 && c[1] >= 0 && c[2] >= 0;
    int q = 0;
    for (int dx = -1; dx <= 1; ++dx) {
        for (int dy = -1; dy <= 1; ++dy, ++q) {
            int32_t beg = 0, end = 0;
            const int64_t x = c[0] + dx, y = c[1] + dy;
            if (usable && x >= 0 && x < MAX_CELLS && y >= 0 && y < MAX_CELLS) {
                const int64_t z0 = c[2] > 0 ? c[2] - 1 : 0, z1 = c[2] + 1 < MAX_CELLS ? c[2] + 1 : MAX_CELLS - 1;
                const u64 head = ((u64)x << 42) | ((u64)y << 21);
                beg = (int32_t)lower_bound(sorted, C, head | (u64)z0);
                end = (int32_t)lower_bound(sorted, C, (head | (u64)z1) + 1ull);
            }
            runs[i * 18 + 2 * q] = beg;
            runs[i * 18 + 2 * q + 1] = end;
        }
    }
}

// One decision round.  remaining[0] += the candidates still undecided after it.
__global__ __launch_bounds__(T) void k_pd_round(const double* __restrict__ P, int64_t C, double r2, const int32_t* __restrict__ ids,
                                                const int32_t* __restrict__ runs, uint8_t* __restrict__ st,
                                                u64* __restrict__ remaining) {
    const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
    bool waits = false;
    if (i < C && ld_agent(st + i) == UNDECIDED) {
        const double px = P[i * 3 + 0], py = P[i * 3 + 1], pz = P[i * 3 + 2];
        bool rejected = false;
        for (int q = 0; q < 9 && !rejected; ++q) {
            int64_t beg = runs[i * 18 + 2 * q], end = runs[i * 18 + 2 * q + 1];
            beg = beg < 0 ? 0 : beg;
            end = end > C ? C : end;
            for (int64_t p = beg; p < end; ++p) {
                const int64_t j = ids[p];
                if (j >= i || j < 0) continue;
                const uint8_t sj = ld_agent(st + j);
                if (sj == REJECTED) continue;
                const double dx = px - P[j * 3 + 0], dy = py - P[j * 3 + 1], dz = pz - P[j * 3 + 2];
                if ((dx * dx + dy * dy) + dz * dz < r2) {
                    if (sj == ACCEPTED) {
                        rejected = true;
                        break;
                    }
                    waits = true;
                }
            }
        }
        if (rejected) {
            st_agent(st + i, REJECTED);
            waits = false;
        } else if (!waits) {
            st_agent(st + i, ACCEPTED);
        }
    }
    const u64 ballot = __ballot(waits);
    if ((threadIdx.x & (STIN_WAVE - 1)) == 0 && ballot) atomicAdd(remaining, (u64)__popcll(ballot));
}

// --------------------------------------------------------------------------------------------------------------------- first
__global__ __launch_bounds__(T) void k_first_min(const int64_t* __restrict__ ids, int64_t n, int64_t N, long long* __restrict__ pos,
                                                 int32_t* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
    if (i >= n) return;
    const int64_t v = ids[i];
    if (v < 0 || v >= N) {
        *bad = 1;
        return;
    }
    atomicMin(pos + v, (long long)i);
}

__global__ __launch_bounds__(T) void k_first_keep(const int64_t* __restrict__ ids, int64_t n, int64_t N, const long long* __restrict__ pos,
                                                  uint8_t* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
    if (i >= n) return;
    const int64_t v = ids[i];
    keep[i] = (v >= 0 && v < N && pos[v] == (long long)i) ? 1 : 0;
}

size_t scan_i64_bytes(int64_t n) {
    size_t bytes = 0;
    (void)rocprim::inclusive_scan(nullptr, bytes, (int64_t*)nullptr, (int64_t*)nullptr, (size_t)(n > 0 ? n : 1), rocprim::plus<int64_t>(),
                                  (hipStream_t)0);
    return bytes;
}
size_t sort_bytes(int64_t n) {
    size_t bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, bytes, (u64*)nullptr, (u64*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr,
                                    (size_t)(n > 0 ? n : 1), 0, 64, (hipStream_t)0);
    return bytes;
}

struct WeightLayout {
    size_t a2, w, temp, total;
};
WeightLayout weight_layout(int64_t F) {
    WeightLayout L;
    const size_t m = (size_t)(F > 0 ? F : 1);
    size_t off = 0;
    L.a2 = off; off += stin_up256(m * 8);
    L.w = off; off += stin_up256(m * 8);
    L.temp = off; off += stin_up256(scan_i64_bytes(F));
    L.total = off + 256;
    return L;
}

struct GridLayout {
    size_t keys0, keys1, ids0, temp, total;
};
GridLayout grid_layout(int64_t C) {
    GridLayout L;
    const size_t m = (size_t)(C > 0 ? C : 1);
    size_t off = 0;
    L.keys0 = off; off += stin_up256(m * 8);
    L.keys1 = off; off += stin_up256(m * 8);
    L.ids0 = off; off += stin_up256(m * 4);
    L.temp = off; off += stin_up256(sort_bytes(C));
    L.total = off + 256;
    return L;
}

inline char* aligned256(void* p) { return reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(p) + 255) & ~(uintptr_t)255); }

}  // namespace

extern "C" size_t stin_surface_weights_workspace_bytes(int64_t F) { return (F < 0 || F > STIN_SURFACE_MAX_FACES) ? 0 : weight_layout(F).total; }

extern "C" int stin_surface_weights_f64(const double* vertices, int64_t N, const int64_t* faces, int64_t F, int64_t* cum, int64_t* state,
                                        void* workspace, size_t workspace_bytes, stin_stream_t stream_) {
    stin_clear_stale_error();
    hipStream_t stream = (hipStream_t)stream_;
    STIN_REQUIRE(N >= 0 && F >= 0, STIN_E_SIZE);
    STIN_REQUIRE(F <= STIN_SURFACE_MAX_FACES, STIN_E_UNSUPPORTED);        // T < 2^62
    STIN_REQUIRE(state != nullptr, STIN_E_NULL);
    long long* st = reinterpret_cast<long long*>(state);
    hipError_t e = hipMemsetAsync(st, 0, 4 * sizeof(long long), stream);
    if (e != hipSuccess) return (int)e;
    if (F == 0) return STIN_OK;
    STIN_REQUIRE(faces && cum && workspace && (vertices || N == 0), STIN_E_NULL);
    STIN_REQUIRE(workspace_bytes >= stin_surface_weights_workspace_bytes(F), STIN_E_WORKSPACE);
    const WeightLayout L = weight_layout(F);
    char* w = aligned256(workspace);
    double* a2 = reinterpret_cast<double*>(w + L.a2);
    int64_t* wt = reinterpret_cast<int64_t*>(w + L.w);
    hipLaunchKernelGGL(k_face_area, dim3(grid_for(F)), dim3(T), 0, stream, vertices, N, faces, F, a2, st);
    hipLaunchKernelGGL(k_face_weight, dim3(grid_for(F)), dim3(T), 0, stream, a2, F, st, wt);
    size_t tb = scan_i64_bytes(F);
    e = rocprim::inclusive_scan(w + L.temp, tb, wt, cum, (size_t)F, rocprim::plus<int64_t>(), stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_total, dim3(1), dim3(64), 0, stream, cum, F, st);
    return stin_launch_status();
}

extern "C" int stin_surface_sample_f64(const double* vertices, int64_t N, const int64_t* faces, int64_t F, const int64_t* cum, int64_t n,
                                       uint64_t seed, uint64_t first, double* points, int64_t* face, double* bary, int64_t* state,
                                       stin_stream_t stream_) {
    stin_clear_stale_error();
    hipStream_t stream = (hipStream_t)stream_;
    STIN_REQUIRE(N >= 0 && F >= 0 && n >= 0 && F <= STIN_SURFACE_MAX_FACES, STIN_E_SIZE);
    STIN_REQUIRE(state != nullptr, STIN_E_NULL);
    if (n == 0) return STIN_OK;
    STIN_REQUIRE(points && face && bary && (F == 0 || (faces && cum && vertices)), STIN_E_NULL);
    hipLaunchKernelGGL(k_sample, dim3(grid_for(n)), dim3(T), 0, stream, vertices, N, faces, F, cum, n, (u64)seed, (u64)first, points,
                       face, bary, reinterpret_cast<long long*>(state));
    return stin_launch_status();
}

extern "C" size_t stin_poisson_grid_workspace_bytes(int64_t C) { return C < 0 ? 0 : grid_layout(C).total; }

extern "C" int stin_poisson_grid_f64(const double* points, int64_t C, double radius, int32_t* order, int32_t* runs, uint8_t* decided,
                                     int64_t* state, void* workspace, size_t workspace_bytes, stin_stream_t stream_) {
    stin_clear_stale_error();
    hipStream_t stream = (hipStream_t)stream_;
    STIN_REQUIRE(C >= 0 && C < ((int64_t)1 << 31) - 1, STIN_E_SIZE);
    STIN_REQUIRE(radius > 0.0 && radius < 1.0e300, STIN_E_SIZE);
    STIN_REQUIRE(state != nullptr, STIN_E_NULL);
    u64* st = reinterpret_cast<u64*>(state);
    hipLaunchKernelGGL(k_pd_init, dim3(1), dim3(64), 0, stream, st);
    if (C == 0) return stin_launch_status();
    STIN_REQUIRE(points && order && runs && decided && workspace, STIN_E_NULL);
    STIN_REQUIRE(workspace_bytes >= stin_poisson_grid_workspace_bytes(C), STIN_E_WORKSPACE);
    const GridLayout L = grid_layout(C);
    char* w = aligned256(workspace);
    u64 *k0 = reinterpret_cast<u64*>(w + L.keys0), *k1 = reinterpret_cast<u64*>(w + L.keys1);
    int32_t* i0 = reinterpret_cast<int32_t*>(w + L.ids0);
    const double h = radius * (1.0 + 0x1.0p-20);
    hipError_t e = hipMemsetAsync(decided, 0, (size_t)C, stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_pd_bounds, dim3(grid_for(C)), dim3(T), 0, stream, points, C, st);
    hipLaunchKernelGGL(k_pd_keys, dim3(grid_for(C)), dim3(T), 0, stream, points, C, h, st, k0, i0);
    size_t tb = sort_bytes(C);
    e = rocprim::radix_sort_pairs(w + L.temp, tb, k0, k1, i0, order, (size_t)C, 0, 63, stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_pd_runs, dim3(grid_for(C)), dim3(T), 0, stream, points, C, h, st, k1, runs);
    return stin_launch_status();
}

extern "C" int stin_poisson_rounds_f64(const double* points, int64_t C, double radius, const int32_t* order, const int32_t* runs,
                                       uint8_t* decided, int rounds, int64_t* remaining, stin_stream_t stream_) {
    stin_clear_stale_error();
    hipStream_t stream = (hipStream_t)stream_;
    STIN_REQUIRE(C >= 0 && C < ((int64_t)1 << 31) - 1 && rounds >= 1 && rounds <= 64, STIN_E_SIZE);
    STIN_REQUIRE(radius > 0.0 && radius < 1.0e300, STIN_E_SIZE);
    STIN_REQUIRE(remaining != nullptr, STIN_E_NULL);
    hipError_t e = hipMemsetAsync(remaining, 0, (size_t)rounds * 8, stream);
    if (e != hipSuccess) return (int)e;
    if (C == 0) return STIN_OK;
    STIN_REQUIRE(points && order && runs && decided, STIN_E_NULL);
    const double r2 = radius * radius;
    for (int k = 0; k < rounds; ++k)
        hipLaunchKernelGGL(k_pd_round, dim3(grid_for(C)), dim3(T), 0, stream, points, C, r2, order, runs, decided,
                           reinterpret_cast<u64*>(remaining) + k);
    return stin_launch_status();
}

extern "C" int stin_first_occurrence_i64(const int64_t* ids, int64_t n, int64_t N, int64_t* first_pos, uint8_t* keep, int32_t* bad,
                                         stin_stream_t stream_) {
    stin_clear_stale_error();
    hipStream_t stream = (hipStream_t)stream_;
    STIN_REQUIRE(n >= 0 && N >= 0, STIN_E_SIZE);
    STIN_REQUIRE(bad != nullptr, STIN_E_NULL);
    hipError_t e = hipMemsetAsync(bad, 0, 4, stream);
    if (e != hipSuccess) return (int)e;
    if (n == 0) return STIN_OK;
    STIN_REQUIRE(ids && keep && (first_pos || N == 0), STIN_E_NULL);
    if (N > 0) {
        e = hipMemsetAsync(first_pos, 0x7f, (size_t)N * 8, stream);           // 0x7f7f...: above every stream position
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k_first_min, dim3(grid_for(n)), dim3(T), 0, stream, ids, n, N, reinterpret_cast<long long*>(first_pos), bad);
    hipLaunchKernelGGL(k_first_keep, dim3(grid_for(n)), dim3(T), 0, stream, ids, n, N, reinterpret_cast<const long long*>(first_pos), keep);
    return stin_launch_status();
}
