// Exact k nearest neighbours in fp64 between two large point sets, brute force, and the mean of the neighbours' rows.
// Contract: include/stin_hip.h ("k nearest neighbours").
//
//   knn:   the structure of k_nearest_f64 (stin_levels.hip).  A workgroup of T = 256 threads owns T * QPT queries (in registers:
//          query q0 + j T + t, so the loads coalesce) and streams its chunk of the points through LDS as separate x / y / z arrays
//          of doubles, TILE = 512 points per stage.  In the inner loop every lane reads the SAME LDS address (a broadcast: no bank
//          conflicts) and compares that point with its own queries: three subtractions, three multiplications, two additions and
//          one compare per pair - 9 fp64 vector ALU operations - shared LDS reads for the thread's QPT queries.
//          d = (dx dx + dy dy) + dz dz without contraction (-ffp-contract=off).
//          New against nearest is a sorted list of (d, index) per query, KC entries (the capacity: 1, 2, 4, 8 or 16, the smallest
//          >= k), held in REGISTERS: every element is named by a compile-time index in fully unrolled loops, nothing is indexed by a
//          run-time value (that would send the list to scratch memory).  Queries per thread fall as the capacity rises (4, 4, 4, 2,
//          2) to keep the list in registers at an occupancy that still hides the LDS reads.
//   ties:  the answer is the k smallest under the total order (d, index).  Points arrive in ASCENDING INDEX, so two choices give it:
//            (a) a point is accepted only on strict d < worst (worst = the list's last d): a point that ties with the worst
//                stored entry has a higher index than it and must lose;
//            (b) an accepted point is inserted AFTER every stored entry with d' <= d: everything stored arrived earlier, i.e. has a
//                lower index, so an equal distance sorts before the newcomer.
//          The list is therefore sorted by (d, index) at all times, and so are its first k entries when KC > k (the top k of the
//          top KC).  The insertion is one unrolled compare-and-shift chain behind the single `d < worst` test: it runs only for the
//          rare accepted point.  Empty slots hold (+inf, INT32_MAX); +inf is never < worst, so they are never displaced by a
//          point at d = +inf and come out as (-1, +inf).
//   valid: an invalid point is staged into LDS as NaN coordinates: its d is NaN, `d < worst` is false, and it is skipped in place at
//          no cost in the inner loop; its own coordinates are never inspected (they may be non-finite without raising a flag).
//   chunks: few queries (less than two workgroups per CU): the points are cut into gridDim.y chunks of whole tiles, every chunk
//          writes the first k entries of its list per query into [chunks][Q][k] partials, padded with (+inf, INT32_MAX), and
//          k_knn_fold inserts them chunk after chunk, entry after entry, into a list of the same kind.  Equal distances still arrive
//          in ascending index (chunks ascend, a chunk's list is sorted by (d, index)), so (a) and (b) hold there too.  A chunk may
//          hold fewer than k candidates, or none.  No float atomics anywhere.
//   mean:  one thread per (listed row, column): the fp64 sum of the neighbours' float32 values left to right, divided by their number.
#include "stin_common.h"

namespace {

constexpr int T = 256;
constexpr int TILE = 512;                  // points per LDS stage: 3 x 4 KB
constexpr int MAX_CHUNKS = 64;

constexpr int capacity_of(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16; }
constexpr int qpt_of(int kc) { return kc <= 4 ? 4 : 2; }      // queries per thread
inline int64_t block_queries(int k) { return (int64_t)T * qpt_of(capacity_of(k)); }

__device__ __forceinline__ bool finite3(double x, double y, double z) {
    return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
}
__device__ __forceinline__ void raise_flag(int64_t* flags, unsigned long long bit) {
    atomicOr(reinterpret_cast<unsigned long long*>(flags), bit);
}
__device__ __forceinline__ int64_t listed(const int64_t* q_count, int64_t Q) {
    if (q_count == nullptr) return Q;
    const int64_t c = *q_count;
    return c < 0 ? 0 : (c < Q ? c : Q);
}

// The sorted list of one query.  Every index below is a compile-time constant once the loops are unrolled.
template <int KC> struct KList {
    double d[KC];
    int32_t i[KC];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int s = 0; s < KC; ++s) {
            d[s] = __builtin_huge_val();
            i[s] = INT32_MAX;
        }
    }
    __device__ __forceinline__ double worst() const { return d[KC - 1]; }
    // nd < worst().  Slot s takes its left neighbour where that one is > nd (it moves up), else the newcomer where the slot itself is
    // > nd (the first such slot: everything left of it is <= nd), else it stays.  Downwards, so d[s - 1] is still the old value.
    __device__ __forceinline__ void insert(double nd, int32_t ni) {
#pragma unroll
        for (int s = KC - 1; s >= 1; --s) {
            const bool up = d[s - 1] > nd, here = d[s] > nd;
            i[s] = up ? i[s - 1] : (here ? ni : i[s]);
            d[s] = up ? d[s - 1] : (here ? nd : d[s]);
        }
        if (d[0] > nd) {
            d[0] = nd;
            i[0] = ni;
        }
    }
};

// grid: x = query block, y = chunk of the points.  part_d == NULL: answers go to out / out_d2 [n_query_rows][k]; else the first k
// entries of every list go to part_d / part_i [chunks][Q][k].
template <int KC, int QPT>
__global__ void __launch_bounds__(T) k_knn_f64(const double* __restrict__ queries, int64_t Q, int64_t n_query_rows,
                                                 const double* __restrict__ points, const uint8_t* __restrict__ p_valid, int64_t P,
                                                 const int64_t* __restrict__ q_index, const int64_t* __restrict__ q_count, int k,
                                                 int64_t tiles_per_chunk, int64_t* __restrict__ out, double* __restrict__ out_d2,
                                                 double* __restrict__ part_d, int32_t* __restrict__ part_i,
                                                 int64_t* __restrict__ flags) {
    constexpr int QB = T * QPT;
    __shared__ double sx[TILE], sy[TILE], sz[TILE];
    const int64_t nq = listed(q_count, Q);
    const int64_t q0 = (int64_t)blockIdx.x * QB;
    if (q0 >= nq) return;                                          // uniform over the workgroup
    const int t = threadIdx.x;
    double px[QPT], py[QPT], pz[QPT];
    KList<KC> best[QPT];
    int64_t row[QPT];
#pragma unroll
    for (int j = 0; j < QPT; ++j) {
        const int64_t q = q0 + (int64_t)j * T + t;
        px[j] = py[j] = pz[j] = 0.0;
        best[j].clear();
        row[j] = -1;
        if (q < nq) {
            int64_t r = q_index != nullptr ? q_index[q] : q;
            if (r < 0 || r >= n_query_rows) {
                raise_flag(flags, 4ull);
                r = -1;
            } else {
                px[j] = queries[3 * r];
                py[j] = queries[3 * r + 1];
                pz[j] = queries[3 * r + 2];
                if (blockIdx.y == 0 && !finite3(px[j], py[j], pz[j])) raise_flag(flags, 1ull);
            }
            row[j] = r;
        }
    }
    const int64_t p_lo = (int64_t)blockIdx.y * tiles_per_chunk * TILE;
    int64_t p_hi = p_lo + tiles_per_chunk * TILE;
    if (p_hi > P) p_hi = P;
    for (int64_t t0 = p_lo; t0 < p_hi; t0 += TILE) {
        __syncthreads();
        for (int s = t; s < TILE; s += T) {
            const int64_t p = t0 + s;
            if (p < p_hi) {
                double x = __builtin_nan(""), y = x, z = x;        // an invalid point: d is NaN and never < worst
                if (p_valid == nullptr || p_valid[p] != 0) {
                    x = points[3 * p];
                    y = points[3 * p + 1];
                    z = points[3 * p + 2];
                    if (blockIdx.x == 0 && !finite3(x, y, z)) raise_flag(flags, 2ull);
                }
                sx[s] = x;
                sy[s] = y;
                sz[s] = z;
            }
        }
        __syncthreads();
        const int m = (int)(p_hi - t0 < TILE ? p_hi - t0 : TILE);
        const int32_t base = (int32_t)t0;
#pragma unroll 4
        for (int s = 0; s < m; ++s) {                              // (unrolled: the LDS reads of four points are issued together)
            const double x = sx[s], y = sy[s], z = sz[s];          // one address for the whole wave: a broadcast
#pragma unroll
            for (int j = 0; j < QPT; ++j) {
                const double dx = px[j] - x, dy = py[j] - y, dz = pz[j] - z;
                const double d = (dx * dx + dy * dy) + dz * dz;    // -ffp-contract=off: no fused multiply-add
                if (d < best[j].worst()) best[j].insert(d, base + s);      // (a) strict; (b) after its equals
            }
        }
    }
#pragma unroll
    for (int j = 0; j < QPT; ++j) {
        const int64_t q = q0 + (int64_t)j * T + t;
        if (q >= nq) continue;
        if (part_d != nullptr) {
            const int64_t at = ((int64_t)blockIdx.y * Q + q) * k;
#pragma unroll
            for (int s = 0; s < KC; ++s)
                if (s < k) {
                    part_d[at + s] = best[j].d[s];
                    part_i[at + s] = best[j].i[s];
                }
        } else if (row[j] >= 0) {
            const int64_t at = row[j] * k;
#pragma unroll
            for (int s = 0; s < KC; ++s)
                if (s < k) {
                    const bool none = best[j].i[s] == INT32_MAX;
                    out[at + s] = none ? -1 : (int64_t)best[j].i[s];
                    if (out_d2 != nullptr) out_d2[at + s] = none ? __builtin_huge_val() : best[j].d[s];
                }
        }
    }
}

// One thread per query: the chunk lists, in ascending chunk order, through the same list.  An entry that is not accepted ends its
// chunk (the rest of that list is no smaller); so does padding.
template <int KC>
__global__ void __launch_bounds__(T) k_knn_fold(const double* __restrict__ part_d, const int32_t* __restrict__ part_i, int chunks,
                                                  int64_t Q, int k, int64_t n_query_rows, const int64_t* __restrict__ q_index,
                                                  const int64_t* __restrict__ q_count, int64_t* __restrict__ out,
                                                  double* __restrict__ out_d2) {
    const int64_t nq = listed(q_count, Q);
    for (int64_t q = (int64_t)blockIdx.x * T + threadIdx.x; q < nq; q += (int64_t)gridDim.x * T) {
        KList<KC> best;
        best.clear();
        for (int c = 0; c < chunks; ++c) {
            const int64_t at = ((int64_t)c * Q + q) * k;
            for (int s = 0; s < k; ++s) {
                const double d = part_d[at + s];
                if (!(d < best.worst())) break;
                best.insert(d, part_i[at + s]);
            }
        }
        const int64_t r = q_index != nullptr ? q_index[q] : q;
        if (r < 0 || r >= n_query_rows) continue;                  // (flagged by k_knn_f64)
#pragma unroll
        for (int s = 0; s < KC; ++s)
            if (s < k) {
                const bool none = best.i[s] == INT32_MAX;
                out[r * k + s] = none ? -1 : (int64_t)best.i[s];
                if (out_d2 != nullptr) out_d2[r * k + s] = none ? __builtin_huge_val() : best.d[s];
            }
    }
}

__global__ void __launch_bounds__(T) k_knn_mean(const float* values, int64_t ld_values, int64_t P, int C,
                                                  const int64_t* __restrict__ idx, int k, const int64_t* __restrict__ q_index,
                                                  const int64_t* __restrict__ q_count, int64_t Q, int64_t n_rows, float* out,
                                                  int64_t ld_out, uint8_t* __restrict__ filled) {
    // (values and out carry no __restrict__: they may be the same array, see the contract)
    const int64_t total = listed(q_count, Q) * C;
    for (int64_t e = (int64_t)blockIdx.x * T + threadIdx.x; e < total; e += (int64_t)gridDim.x * T) {
        const int64_t q = e / C;
        const int c = (int)(e - q * C);
        const int64_t r = q_index != nullptr ? q_index[q] : q;
        if (r < 0 || r >= n_rows) continue;
        double sum = 0.0;
        int m = 0;
        for (; m < k; ++m) {
            const int64_t p = idx[r * k + m];
            if (p < 0 || p >= P) break;
            const double v = (double)values[p * ld_values + c];
            sum = m == 0 ? v : sum + v;
        }
        if (m > 0) out[r * ld_out + c] = (float)(sum / (double)m);
        if (c == 0 && filled != nullptr) filled[r] = m > 0 ? 1 : 0;
    }
}

inline size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }
inline unsigned grid_1d(int64_t n) {
    int64_t g = (n + T - 1) / T;
    if (g < 1) g = 1;
    if (g > 4096) g = 4096;
    return (unsigned)g;
}

template <int KC>
void launch_knn(const double* queries, int64_t n_query_rows, const double* points, const uint8_t* p_valid, int64_t P,
                const int64_t* q_index, const int64_t* q_count, int64_t Q, int k, int chunks, int64_t tpc, int64_t* out, double* out_d2,
                double* part_d, int32_t* part_i, int64_t* flags, hipStream_t s) {
    constexpr int QPT = qpt_of(KC);
    const dim3 grid((unsigned)((Q + T * QPT - 1) / (T * QPT)), (unsigned)chunks);
    hipLaunchKernelGGL((k_knn_f64<KC, QPT>), grid, dim3(T), 0, s, queries, Q, n_query_rows, points, p_valid, P, q_index, q_count, k, tpc,
                       out, out_d2, part_d, part_i, flags);
    if (chunks > 1)
        hipLaunchKernelGGL((k_knn_fold<KC>), dim3(grid_1d(Q)), dim3(T), 0, s, (const double*)part_d, (const int32_t*)part_i, chunks, Q, k,
                           n_query_rows, q_index, q_count, out, out_d2);
}

}  // namespace

extern "C" int stin_knn_chunks(int64_t Q, int64_t P, int k) {
    if (Q <= 0 || P <= 0 || k < 1 || k > STIN_KNN_MAX_K) return 1;
    const int64_t qb = block_queries(k);
    const int64_t blocks = (Q + qb - 1) / qb, tiles = (P + TILE - 1) / TILE;
    const int64_t want = 2 * (int64_t)stin_cu_count_dev();
    int64_t c = (want + blocks - 1) / blocks;
    if (c > tiles) c = tiles;
    if (c > MAX_CHUNKS) c = MAX_CHUNKS;
    return c < 1 ? 1 : (int)c;
}

extern "C" size_t stin_knn_workspace_bytes(int64_t Q, int chunks, int k) {
    if (Q <= 0 || chunks <= 1 || k < 1 || k > STIN_KNN_MAX_K) return 0;
    const size_t n = (size_t)chunks * (size_t)Q * (size_t)k;
    return round16(n * 8) + round16(n * 4);
}

extern "C" int stin_knn_f64(const double* queries, int64_t n_query_rows, const double* points, const uint8_t* p_valid, int64_t P,
                            const int64_t* q_index, const int64_t* q_count, int64_t Q, int k, int chunks, int64_t* out_index,
                            double* out_d2, int64_t* flags, void* workspace, size_t workspace_bytes, stin_stream_t stream) {
    STIN_REQUIRE(Q >= 0 && n_query_rows >= 0 && P >= 0, STIN_E_SIZE);
    STIN_REQUIRE(k >= 1 && k <= STIN_KNN_MAX_K, STIN_E_SIZE);
    STIN_REQUIRE(chunks >= 1 && chunks <= MAX_CHUNKS, STIN_E_SIZE);
    if (Q == 0) return STIN_OK;
    STIN_REQUIRE(P < INT32_MAX && Q < ((int64_t)INT32_MAX - 1) * T, STIN_E_UNSUPPORTED);
    STIN_REQUIRE(q_index != nullptr || Q <= n_query_rows, STIN_E_SIZE);
    STIN_REQUIRE(queries != nullptr && out_index != nullptr && flags != nullptr, STIN_E_NULL);
    STIN_REQUIRE(P == 0 || points != nullptr, STIN_E_NULL);
    const int64_t tiles = (P + TILE - 1) / TILE;
    if (chunks > tiles) chunks = tiles < 1 ? 1 : (int)tiles;
    const int64_t tpc = (tiles + chunks - 1) / chunks;
    double* part_d = nullptr;
    int32_t* part_i = nullptr;
    if (chunks > 1) {
        STIN_REQUIRE(workspace != nullptr, STIN_E_NULL);
        STIN_REQUIRE(workspace_bytes >= stin_knn_workspace_bytes(Q, chunks, k), STIN_E_WORKSPACE);
        part_d = (double*)workspace;
        part_i = (int32_t*)((char*)workspace + round16((size_t)chunks * (size_t)Q * (size_t)k * 8));
    }
    stin_clear_stale_error();
    hipStream_t s = (hipStream_t)stream;
#define STIN_KNN_GO(KC) \
    launch_knn<KC>(queries, n_query_rows, points, p_valid, P, q_index, q_count, Q, k, chunks, tpc, out_index, out_d2, part_d, part_i, flags, s)
    switch (capacity_of(k)) {
        case 1: STIN_KNN_GO(1); break;
        case 2: STIN_KNN_GO(2); break;
        case 4: STIN_KNN_GO(4); break;
        case 8: STIN_KNN_GO(8); break;
        default: STIN_KNN_GO(16); break;
    }
#undef STIN_KNN_GO
    return stin_launch_status();
}

extern "C" int stin_knn_mean_f32(const float* values, int64_t ld_values, int64_t P, int C, const int64_t* idx, int k,
                                 const int64_t* q_index, const int64_t* q_count, int64_t Q, int64_t n_rows, float* out, int64_t ld_out,
                                 uint8_t* filled, stin_stream_t stream) {
    STIN_REQUIRE(Q >= 0 && n_rows >= 0 && P >= 0, STIN_E_SIZE);
    STIN_REQUIRE(C >= 1 && C <= STIN_KNN_MAX_C && k >= 1 && k <= STIN_KNN_MAX_K, STIN_E_SIZE);
    STIN_REQUIRE(ld_values >= C && ld_out >= C, STIN_E_SIZE);
    STIN_REQUIRE(q_index != nullptr || Q <= n_rows, STIN_E_SIZE);
    if (Q == 0) return STIN_OK;
    STIN_REQUIRE(idx != nullptr && out != nullptr, STIN_E_NULL);
    STIN_REQUIRE(P == 0 || values != nullptr, STIN_E_NULL);
    stin_clear_stale_error();
    hipLaunchKernelGGL(k_knn_mean, dim3(grid_1d(Q * C)), dim3(T), 0, (hipStream_t)stream, values, ld_values, P, C, idx, k, q_index,
                       q_count, Q, n_rows, out, ld_out, filled);
    return stin_launch_status();
}
