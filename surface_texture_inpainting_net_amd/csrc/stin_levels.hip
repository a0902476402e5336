// Graph level generation on the device (reference preprocessing/graph_level_generation.py: csv2npy :135-191, get_color_and_labels
// :98-116, nearest_neighbor_interpolation_for_unassigned_traces :284-295).  Contract: include/stin_hip.h ("graph levels").
//
//   nearest:  exact nearest neighbour in fp64 between two large point sets, brute force.  A workgroup of T = 256 threads owns
//             T * QPT = 1024 queries (QPT = 4 per thread, in registers: query q0 + j T + t, so the loads coalesce) and streams its
//             chunk of the points through LDS as separate x / y / z arrays of doubles, TILE = 512 points per stage.  In the inner
//             loop every lane reads the SAME LDS address (a broadcast: no bank conflicts) and compares that point with its own
//             queries: three subtractions, three multiplications, two additions, one compare and two selects per pair, all fp64
//             vector ALU work; the three LDS reads are shared by the thread's QPT queries.
//             d = (dx dx + dy dy) + dz dz without contraction (-ffp-contract=off), strict < in ascending index order: exactly
//             k_nearest of stin_crop.hip and numpy's argmin of the same expression, ties included.
//             Few queries (less than two workgroups per CU): the points are cut into gridDim.y chunks of whole tiles, every chunk
//             writes its (d, index) per query into [chunks][Q] partials and k_nearest_fold takes the smaller d, then the lower
//             index, walking the chunks in ascending order.  No float atomics anywhere.
//             Optional: an index list (query i is row q_index[i] of the query array and its answer goes to out[q_index[i]]) whose
//             length is a DEVICE word - the unassigned vertices of a trace are looked up without the host ever learning how many.
//   traces:   k_trace_rows (rows, rows with traces and the last row per new vertex: integer atomics), k_trace_scatter
//             (trace[old_id[t]] = new_id[row_of[t]] and a hit count per old vertex), k_trace_unassigned (compaction of trace == -1
//             through an integer cursor: the ORDER of the list varies between runs, what is written for each entry does not),
//             k_trace_check (old vertices named twice, rows that resolve to a taken new vertex, new vertices left uncovered).
//             Every condition ends in ONE int64 state vector that the host reads once.
#include "stin_common.h"

namespace {

constexpr int T = 256;
constexpr int QPT = 4;                     // queries per thread
constexpr int QB = T * QPT;                // queries per workgroup
constexpr int TILE = 512;                  // points per LDS stage: 3 x 4 KB
constexpr int MAX_CHUNKS = 64;

__device__ __forceinline__ bool finite3(double x, double y, double z) {
    return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
}
__device__ __forceinline__ void raise_flag(int64_t* flags, unsigned long long bit) {
    atomicOr(reinterpret_cast<unsigned long long*>(flags), bit);
}

// grid: x = query block, y = chunk of the points.  chunks == 1: answers go to out / out_d2; else to part_d / part_i [chunks][Q].
__global__ void __launch_bounds__(T) k_nearest_f64(const double* __restrict__ queries, int64_t Q, int64_t n_query_rows,
                                                     const double* __restrict__ points, int64_t P, const int64_t* __restrict__ q_index,
                                                     const int64_t* __restrict__ q_count, int64_t tiles_per_chunk,
                                                     int64_t* __restrict__ out, double* __restrict__ out_d2,
                                                     double* __restrict__ part_d, int32_t* __restrict__ part_i,
                                                     int64_t* __restrict__ flags) {
    __shared__ double sx[TILE], sy[TILE], sz[TILE];
    int64_t nq = Q;
    if (q_count != nullptr) {
        const int64_t c = *q_count;
        nq = c < 0 ? 0 : (c < Q ? c : Q);
    }
    const int64_t q0 = (int64_t)blockIdx.x * QB;
    if (q0 >= nq) return;                                          // uniform over the workgroup
    const int t = threadIdx.x;
    double px[QPT], py[QPT], pz[QPT], best[QPT];
    int32_t bi[QPT];
    int64_t row[QPT];
#pragma unroll
    for (int j = 0; j < QPT; ++j) {
        const int64_t q = q0 + (int64_t)j * T + t;
        px[j] = py[j] = pz[j] = 0.0;
        best[j] = __builtin_huge_val();
        bi[j] = INT32_MAX;
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
        for (int k = t; k < TILE; k += T) {
            const int64_t p = t0 + k;
            if (p < p_hi) {
                const double x = points[3 * p], y = points[3 * p + 1], z = points[3 * p + 2];
                sx[k] = x;
                sy[k] = y;
                sz[k] = z;
                if (blockIdx.x == 0 && !finite3(x, y, z)) raise_flag(flags, 2ull);
            }
        }
        __syncthreads();
        const int m = (int)(p_hi - t0 < TILE ? p_hi - t0 : TILE);
        const int32_t base = (int32_t)t0;
#pragma unroll 4
        for (int k = 0; k < m; ++k) {                              // (unrolled: the LDS reads of four points are issued together)
            const double x = sx[k], y = sy[k], z = sz[k];          // one address for the whole wave: a broadcast
#pragma unroll
            for (int j = 0; j < QPT; ++j) {
                const double dx = px[j] - x, dy = py[j] - y, dz = pz[j] - z;
                const double d = (dx * dx + dy * dy) + dz * dz;    // -ffp-contract=off: no fused multiply-add
                if (d < best[j]) {                                 // ascending index, strict: the lowest index wins a tie
                    best[j] = d;
                    bi[j] = base + k;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < QPT; ++j) {
        const int64_t q = q0 + (int64_t)j * T + t;
        if (q >= nq) continue;
        if (part_d != nullptr) {
            part_d[(int64_t)blockIdx.y * Q + q] = best[j];
            part_i[(int64_t)blockIdx.y * Q + q] = bi[j];
        } else if (row[j] >= 0) {
            out[row[j]] = bi[j] == INT32_MAX ? 0 : (int64_t)bi[j];
            if (out_d2 != nullptr) out_d2[row[j]] = best[j];
        }
    }
}

__global__ void __launch_bounds__(T) k_nearest_fold(const double* __restrict__ part_d, const int32_t* __restrict__ part_i, int chunks,
                                                      int64_t Q, int64_t n_query_rows, const int64_t* __restrict__ q_index,
                                                      const int64_t* __restrict__ q_count, int64_t* __restrict__ out,
                                                      double* __restrict__ out_d2) {
    int64_t nq = Q;
    if (q_count != nullptr) {
        const int64_t c = *q_count;
        nq = c < 0 ? 0 : (c < Q ? c : Q);
    }
    for (int64_t q = (int64_t)blockIdx.x * T + threadIdx.x; q < nq; q += (int64_t)gridDim.x * T) {
        double best = __builtin_huge_val();
        int32_t bi = INT32_MAX;
        for (int c = 0; c < chunks; ++c) {
            const double d = part_d[(int64_t)c * Q + q];
            const int32_t i = part_i[(int64_t)c * Q + q];
            if (d < best || (d == best && i < bi)) {               // smaller distance, then lower index
                best = d;
                bi = i;
            }
        }
        const int64_t r = q_index != nullptr ? q_index[q] : q;
        if (r < 0 || r >= n_query_rows) continue;                  // (flagged by k_nearest_f64)
        out[r] = bi == INT32_MAX ? 0 : (int64_t)bi;
        if (out_d2 != nullptr) out_d2[r] = best;
    }
}

// ---------------------------------------------------------------------------------------------------------------- traces
struct TraceWs {
    int32_t *hits, *rows, *nzrows, *last_row, *cover;
};
inline size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }
inline size_t trace_ws_bytes(int64_t n_old, int64_t n_new) {
    return round16((size_t)(n_old > 0 ? n_old : 1) * 4) + 4 * round16((size_t)(n_new > 0 ? n_new : 1) * 4);
}
inline TraceWs trace_ws(void* ws, int64_t n_old, int64_t n_new) {
    char* p = (char*)ws;
    const size_t so = round16((size_t)(n_old > 0 ? n_old : 1) * 4), sn = round16((size_t)(n_new > 0 ? n_new : 1) * 4);
    TraceWs w;
    w.hits = (int32_t*)p;
    w.rows = (int32_t*)(p + so);
    w.nzrows = (int32_t*)(p + so + sn);
    w.last_row = (int32_t*)(p + so + 2 * sn);
    w.cover = (int32_t*)(p + so + 3 * sn);
    return w;
}
inline unsigned grid_1d(int64_t n) {
    int64_t g = (n + T - 1) / T;
    if (g < 1) g = 1;
    if (g > 4096) g = 4096;
    return (unsigned)g;
}

__global__ void k_trace_init(int64_t* __restrict__ trace, int64_t n_old, int32_t* __restrict__ last_row, int64_t n_new) {
    const int64_t n = n_old > n_new ? n_old : n_new;
    for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < n; i += (int64_t)gridDim.x * T) {
        if (i < n_old) trace[i] = -1;
        if (i < n_new) last_row[i] = -1;
    }
}

__global__ void k_trace_rows(const int64_t* __restrict__ new_id, const int64_t* __restrict__ row_ptr, int64_t R, int64_t n_new,
                             TraceWs w, int64_t* __restrict__ state) {
    for (int64_t r = (int64_t)blockIdx.x * T + threadIdx.x; r < R; r += (int64_t)gridDim.x * T) {
        const int64_t v = new_id[r];
        if (v < 0 || v >= n_new) {
            raise_flag(state + 3, 8ull);
            continue;
        }
        atomicAdd(w.rows + v, 1);
        if (row_ptr[r + 1] > row_ptr[r]) atomicAdd(w.nzrows + v, 1);
        atomicMax(w.last_row + v, (int32_t)r);
    }
}

__global__ void k_trace_scatter(const int64_t* __restrict__ new_id, int64_t R, const int64_t* __restrict__ old_id,
                                const int64_t* __restrict__ row_of, int64_t n_entries, int64_t n_old, int64_t n_new, TraceWs w,
                                int64_t* __restrict__ trace, int64_t* __restrict__ state) {
    for (int64_t e = (int64_t)blockIdx.x * T + threadIdx.x; e < n_entries; e += (int64_t)gridDim.x * T) {
        const int64_t o = old_id[e], r = row_of[e];
        if (o < 0 || o >= n_old || r < 0 || r >= R) {
            raise_flag(state + 3, 8ull);
            continue;
        }
        const int64_t v = new_id[r];
        if (v < 0 || v >= n_new) continue;                         // (flagged by k_trace_rows)
        atomicAdd(w.hits + o, 1);
        trace[o] = v;                                              // named twice: an error of the call, whichever store lands
    }
}

__global__ void k_trace_unassigned(const int64_t* __restrict__ trace, int64_t n_old, int64_t* __restrict__ list,
                                   int64_t* __restrict__ state) {
    for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < n_old; i += (int64_t)gridDim.x * T) {
        if (trace[i] == -1) {
            const unsigned long long s = atomicAdd(reinterpret_cast<unsigned long long*>(state + 4), 1ull);
            if ((int64_t)s < n_old) list[s] = i;
        }
    }
}

__global__ void k_trace_cover(const int64_t* __restrict__ trace, int64_t n_old, int64_t n_new, TraceWs w, int64_t* __restrict__ state) {
    for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < n_old; i += (int64_t)gridDim.x * T) {
        const int64_t v = trace[i];
        if (v >= 0 && v < n_new) atomicAdd(w.cover + v, 1);
        else raise_flag(state + 3, 16ull);                         // still unassigned, or out of range
        if (w.hits[i] > 1) atomicAdd(reinterpret_cast<unsigned long long*>(state + 0), 1ull);
    }
}

__global__ void k_trace_check_new(const int64_t* __restrict__ row_ptr, int64_t n_new, TraceWs w, int64_t* __restrict__ state) {
    for (int64_t v = (int64_t)blockIdx.x * T + threadIdx.x; v < n_new; v += (int64_t)gridDim.x * T) {
        const int32_t lr = w.last_row[v];
        if (lr >= 0) {
            // a row is refused when an EARLIER row of the same new vertex carried old vertices: every row with traces but the last
            const int last_has = row_ptr[lr + 1] > row_ptr[lr] ? 1 : 0;
            if (w.nzrows[v] - last_has > 0) atomicAdd(reinterpret_cast<unsigned long long*>(state + 1), 1ull);
        }
        if (w.rows[v] == 0 && w.cover[v] == 0) atomicAdd(reinterpret_cast<unsigned long long*>(state + 2), 1ull);
    }
}

// float32 centre of gravity of every cluster as numpy forms it for float32 rows (`coords[members].mean(axis=0)`): the members in
// ascending vertex order added one by one into a float32 sum, then divided by the float32 count.  One thread per cluster.
__global__ void k_cluster_mean_f32(const float* __restrict__ coords, int64_t n, const int64_t* __restrict__ order,
                                   const int64_t* __restrict__ seg_ptr, int64_t n_seg, float* __restrict__ out) {
    for (int64_t c = (int64_t)blockIdx.x * T + threadIdx.x; c < n_seg; c += (int64_t)gridDim.x * T) {
        int64_t lo = seg_ptr[c], hi = seg_ptr[c + 1];
        if (lo < 0) lo = 0;
        if (hi > n) hi = n;
        float sx = 0.f, sy = 0.f, sz = 0.f;
        for (int64_t k = lo; k < hi; ++k) {
            const int64_t v = order[k];
            if (v < 0 || v >= n) continue;
            sx += coords[3 * v];
            sy += coords[3 * v + 1];
            sz += coords[3 * v + 2];
        }
        const float cnt = (float)(hi > lo ? hi - lo : 0);
        out[3 * c] = sx / cnt;
        out[3 * c + 1] = sy / cnt;
        out[3 * c + 2] = sz / cnt;
    }
}

}  // namespace

extern "C" int stin_nearest_chunks(int64_t Q, int64_t P) {
    if (Q <= 0 || P <= 0) return 1;
    const int64_t blocks = (Q + QB - 1) / QB, tiles = (P + TILE - 1) / TILE;
    const int64_t want = 2 * (int64_t)stin_cu_count_dev();
    int64_t c = (want + blocks - 1) / blocks;
    if (c > tiles) c = tiles;
    if (c > MAX_CHUNKS) c = MAX_CHUNKS;
    return c < 1 ? 1 : (int)c;
}

extern "C" size_t stin_nearest_workspace_bytes(int64_t Q, int chunks) {
    if (Q <= 0 || chunks <= 1) return 0;
    return round16((size_t)chunks * (size_t)Q * 8) + round16((size_t)chunks * (size_t)Q * 4);
}

extern "C" int stin_nearest_f64(const double* queries, int64_t n_query_rows, const double* points, int64_t P, const int64_t* q_index,
                                const int64_t* q_count, int64_t Q, int chunks, int64_t* out_index, double* out_d2, int64_t* flags,
                                void* workspace, size_t workspace_bytes, stin_stream_t stream) {
    STIN_REQUIRE(Q >= 0 && n_query_rows >= 0 && P >= 0, STIN_E_SIZE);
    if (Q == 0) return STIN_OK;
    STIN_REQUIRE(P > 0, STIN_E_SIZE);
    STIN_REQUIRE(P < INT32_MAX && Q < ((int64_t)INT32_MAX - 1) * QB, STIN_E_UNSUPPORTED);
    STIN_REQUIRE(q_index != nullptr || Q <= n_query_rows, STIN_E_SIZE);
    STIN_REQUIRE(queries != nullptr && points != nullptr && out_index != nullptr && flags != nullptr, STIN_E_NULL);
    STIN_REQUIRE(chunks >= 1 && chunks <= MAX_CHUNKS, STIN_E_SIZE);
    const int64_t tiles = (P + TILE - 1) / TILE;
    if (chunks > tiles) chunks = (int)tiles;
    const int64_t tpc = (tiles + chunks - 1) / chunks;
    double* part_d = nullptr;
    int32_t* part_i = nullptr;
    if (chunks > 1) {
        STIN_REQUIRE(workspace != nullptr, STIN_E_NULL);
        STIN_REQUIRE(workspace_bytes >= stin_nearest_workspace_bytes(Q, chunks), STIN_E_WORKSPACE);
        part_d = (double*)workspace;
        part_i = (int32_t*)((char*)workspace + round16((size_t)chunks * (size_t)Q * 8));
    }
    stin_clear_stale_error();
    const dim3 grid((unsigned)((Q + QB - 1) / QB), (unsigned)chunks);
    hipLaunchKernelGGL(k_nearest_f64, grid, dim3(T), 0, (hipStream_t)stream, queries, Q, n_query_rows, points, P, q_index, q_count, tpc,
                       out_index, out_d2, part_d, part_i, flags);
    if (chunks > 1)
        hipLaunchKernelGGL(k_nearest_fold, dim3(grid_1d(Q)), dim3(T), 0, (hipStream_t)stream, (const double*)part_d,
                           (const int32_t*)part_i, chunks, Q, n_query_rows, q_index, q_count, out_index, out_d2);
    return stin_launch_status();
}

extern "C" size_t stin_trace_workspace_bytes(int64_t n_old, int64_t n_new) { return trace_ws_bytes(n_old, n_new); }

extern "C" int stin_trace_scatter_i64(const int64_t* new_id, const int64_t* row_ptr, int64_t R, const int64_t* old_id,
                                      const int64_t* row_of, int64_t n_entries, int64_t n_old, int64_t n_new, int64_t* trace,
                                      int64_t* state, void* workspace, size_t workspace_bytes, stin_stream_t stream) {
    STIN_REQUIRE(R >= 0 && n_entries >= 0 && n_old >= 0 && n_new >= 0, STIN_E_SIZE);
    STIN_REQUIRE(R < INT32_MAX && n_old < INT32_MAX && n_new < INT32_MAX, STIN_E_UNSUPPORTED);
    STIN_REQUIRE(state != nullptr && workspace != nullptr && row_ptr != nullptr, STIN_E_NULL);
    STIN_REQUIRE(n_old == 0 || trace != nullptr, STIN_E_NULL);
    STIN_REQUIRE(R == 0 || new_id != nullptr, STIN_E_NULL);
    STIN_REQUIRE(n_entries == 0 || (old_id != nullptr && row_of != nullptr), STIN_E_NULL);
    STIN_REQUIRE(workspace_bytes >= trace_ws_bytes(n_old, n_new), STIN_E_WORKSPACE);
    hipStream_t s = (hipStream_t)stream;
    stin_clear_stale_error();
    const TraceWs w = trace_ws(workspace, n_old, n_new);
    hipError_t e = hipMemsetAsync(workspace, 0, trace_ws_bytes(n_old, n_new), s);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(state, 0, 5 * sizeof(int64_t), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_trace_init, dim3(grid_1d(n_old > n_new ? n_old : n_new)), dim3(T), 0, s, trace, n_old, w.last_row, n_new);
    if (R > 0) hipLaunchKernelGGL(k_trace_rows, dim3(grid_1d(R)), dim3(T), 0, s, new_id, row_ptr, R, n_new, w, state);
    if (n_entries > 0)
        hipLaunchKernelGGL(k_trace_scatter, dim3(grid_1d(n_entries)), dim3(T), 0, s, new_id, R, old_id, row_of, n_entries, n_old, n_new,
                           w, trace, state);
    return stin_launch_status();
}

extern "C" int stin_trace_unassigned_i64(const int64_t* trace, int64_t n_old, int64_t* list, int64_t* state, stin_stream_t stream) {
    STIN_REQUIRE(n_old >= 0, STIN_E_SIZE);
    STIN_REQUIRE(state != nullptr, STIN_E_NULL);
    STIN_REQUIRE(n_old == 0 || (trace != nullptr && list != nullptr), STIN_E_NULL);
    hipStream_t s = (hipStream_t)stream;
    stin_clear_stale_error();
    hipError_t e = hipMemsetAsync(state + 4, 0, sizeof(int64_t), s);
    if (e != hipSuccess) return (int)e;
    if (n_old > 0) hipLaunchKernelGGL(k_trace_unassigned, dim3(grid_1d(n_old)), dim3(T), 0, s, trace, n_old, list, state);
    return stin_launch_status();
}

extern "C" int stin_trace_check_i64(const int64_t* trace, int64_t n_old, const int64_t* row_ptr, int64_t R, int64_t n_new,
                                    int64_t* state, void* workspace, size_t workspace_bytes, stin_stream_t stream) {
    STIN_REQUIRE(n_old >= 0 && n_new >= 0 && R >= 0, STIN_E_SIZE);
    STIN_REQUIRE(state != nullptr && workspace != nullptr && row_ptr != nullptr, STIN_E_NULL);
    STIN_REQUIRE(n_old == 0 || trace != nullptr, STIN_E_NULL);
    STIN_REQUIRE(workspace_bytes >= trace_ws_bytes(n_old, n_new), STIN_E_WORKSPACE);
    hipStream_t s = (hipStream_t)stream;
    stin_clear_stale_error();
    const TraceWs w = trace_ws(workspace, n_old, n_new);
    if (n_old > 0) hipLaunchKernelGGL(k_trace_cover, dim3(grid_1d(n_old)), dim3(T), 0, s, trace, n_old, n_new, w, state);
    if (n_new > 0) hipLaunchKernelGGL(k_trace_check_new, dim3(grid_1d(n_new)), dim3(T), 0, s, row_ptr, n_new, w, state);
    return stin_launch_status();
}

extern "C" int stin_cluster_mean_f32(const float* coords, int64_t n, const int64_t* order, const int64_t* seg_ptr, int64_t n_seg,
                                     float* out, stin_stream_t stream) {
    STIN_REQUIRE(n >= 0 && n_seg >= 0, STIN_E_SIZE);
    if (n_seg == 0) return STIN_OK;
    STIN_REQUIRE(coords != nullptr && order != nullptr && seg_ptr != nullptr && out != nullptr, STIN_E_NULL);
    stin_clear_stale_error();
    hipLaunchKernelGGL(k_cluster_mean_f32, dim3(grid_1d(n_seg)), dim3(T), 0, (hipStream_t)stream, coords, n, order, seg_ptr, n_seg, out);
    return stin_launch_status();
}
