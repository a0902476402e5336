// Geodesic circle masks: bounded multi-source shortest paths over the mesh edges weighted by their Euclidean length (the Dijkstra
// metric of the edge graph, NOT the exact polyhedral geodesic, which crosses faces).  Contract: include/stin_hip.h ("Geodesic
// distances"); tests/_geodesic_oracle.py restates it (heap Dijkstra and Bellman-Ford sweeps) and the device agrees bit for bit.
//
//   lengths:   one thread per slot of stin_mask_adjacency_i64's CSR: the row by a binary search in rowptr, then
//              sqrt((dx dx + dy dy) + dz dz) in fp64 (the file is built with -ffp-contract=off; sqrt is IEEE).
//   distance:  dist[m][v] is a non-negative double, so its bit pattern orders as a uint64 and is lowered with the 64-bit integer
//              atomicMin (no float atomics).  A plain frontier label-correcting pass; every round is ONE launch and launch
//              boundaries are the only grid-wide seams.  A round shares the global worklist out in slices of up to 256 entries; a
//              workgroup stages its slice as an LDS frontier of (vertex, value) entries, shares the edges of a chunk out evenly
//              over its threads (a hub is not one lane's loop) and keeps the vertices it lowered as the next LDS frontier for up
//              to `levels` levels; entries beyond the LDS capacity, and what is left after the last level, go to the global list of
//              the NEXT round.
//              Why the schedule cannot change a bit: D is the unique fixed point of D[s] = 0, D[v] = min_u fl(D[u] + len(u, v))
//              (fp64 addition of non-negative numbers is monotone), every value ever stored is the folded length of a real path
//              (so never below D), and every successful lowering of w to a value x leaves an entry that is expanded later with
//              the value then current unless somebody lowered w below x in between - who then left an entry of their own.  An
//              LDS entry carries x and is skipped when dist[w] != x at its turn (Dijkstra's stale-entry rule); a global entry is
//              read back in the next launch, after the boundary.  Hence whoever writes a vertex's final value gets it expanded,
//              and an empty worklist means the fixed point.
//              One flag word per (m, v) dedups the global list: it holds the stamp of the last round the vertex was listed FOR
//              (atomicMax), so a list never holds a vertex twice and never exceeds M N entries.  Dedup against the list of the
//              next launch is safe (it is consumed after the boundary); dedup against an LDS frontier of another workgroup would
//              not be, and is not done.
//              No kernel waits for another workgroup.  The last workgroup to arrive (a ticket, as in stin_mask.hip) publishes the
//              next round's count and resets the ticket; a round that finds its list empty returns at once and takes no ticket.
//              Every loop is bounded by the list count read at the start, `levels`, the LDS capacity or a row's degree.
//   mask:      one thread per (m, v): 0 where D >= radius, else min(rings, (int64) ceil((radius - D) / ring)).
#include "stin_common.h"

namespace {

typedef unsigned long long u64;

constexpr int GB = 256;          // threads per workgroup = the most worklist entries per slice
constexpr int FCAP = 2048;       // LDS frontier entries per level buffer (12 bytes each, two buffers: 48 KB)
constexpr int CTL_WORDS = 4;     // ticket, entries of list 0, entries of list 1, reserved
constexpr int MAX_LEVELS = 64;
constexpr int MAX_ROUNDS_PER_CALL = 4096;
constexpr u64 INF_BITS = 0x7FF0000000000000ull;
constexpr u64 ST_LENGTH = 1, ST_INDEX = 2, ST_OPEN = 4;

__device__ inline u64 ld_agent(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline int32_t ld_agent(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void st_agent(u64* p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void st_agent(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

inline unsigned grid_for(int64_t n) { return (unsigned)((n + GB - 1) / GB); }

// ------------------------------------------------------------------------------------------------------------------ lengths
__global__ __launch_bounds__(GB) void k_geo_lengths(const double* __restrict__ pos, int64_t N, const int32_t* __restrict__ rowptr,
                                                    const int32_t* __restrict__ col, int64_t E2, double* __restrict__ len,
                                                    long long* __restrict__ flags) {
    const int64_t e = (int64_t)blockIdx.x * GB + threadIdx.x;
    if (e >= E2) return;
    int64_t lo = 0, hi = N;                                // the row: largest u with rowptr[u] <= e
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (rowptr[mid] <= e) lo = mid;
        else hi = mid;
    }
    const int64_t u = lo, v = col[e];
    if (v < 0 || v >= N) {                                 // nothing is read through it; an infinite length is never relaxed
        atomicOr((u64*)flags, ST_INDEX);
        len[e] = __longlong_as_double((long long)INF_BITS);
        return;
    }
    const double dx = pos[u * 3 + 0] - pos[v * 3 + 0], dy = pos[u * 3 + 1] - pos[v * 3 + 1], dz = pos[u * 3 + 2] - pos[v * 3 + 2];
    const double l = sqrt((dx * dx + dy * dy) + dz * dz);
    if (!(l < __longlong_as_double((long long)INF_BITS))) atomicOr((u64*)flags, ST_LENGTH);        // inf or NaN
    len[e] = l;
}

// ---------------------------------------------------------------------------------------------------------------- distances
struct GeoArgs {
    const int32_t* rowptr;
    const int32_t* col;
    const double* len;
    u64* dist;                   // [M][N] bit patterns of non-negative doubles
    int32_t* flag;               // [M][N] stamp of the last round the vertex was listed for
    int32_t* list[2];            // [M][N] each: the worklists of even and odd rounds (global ids m N + v)
    u64* ctl;                    // CTL_WORDS
    long long* state;            // status, entries waiting, rounds run, edges relaxed
    int64_t N, E2;
    double cap;
    int levels;
};

__global__ __launch_bounds__(GB) void k_geo_init(u64* __restrict__ dist, int32_t* __restrict__ flag, int64_t MN) {
    for (int64_t i = (int64_t)blockIdx.x * GB + threadIdx.x; i < MN; i += (int64_t)gridDim.x * GB) {
        dist[i] = INF_BITS;
        flag[i] = 0;
    }
}

// sources: distance 0, listed for round 0 (stamp 1); a repeated source lowers nothing and is not listed again
__global__ __launch_bounds__(GB) void k_geo_seed(GeoArgs a, const int64_t* __restrict__ sources, const int32_t* __restrict__ inst,
                                                 int64_t S, int M) {
    const int64_t i = (int64_t)blockIdx.x * GB + threadIdx.x;
    if (i < S) {
        const int64_t s = sources[i];
        const int m = inst != nullptr ? inst[i] : 0;
        if (s < 0 || s >= a.N || m < 0 || m >= M) {
            atomicOr((u64*)a.state, ST_INDEX);
        } else {
            const int64_t gid = (int64_t)m * a.N + s;
            if (atomicMin(a.dist + gid, 0ull) > 0ull && atomicMax(a.flag + gid, 1) < 1) {
                const u64 q = atomicAdd(a.ctl + 1, 1ull);
                st_agent(a.list[0] + q, (int32_t)gid);
                atomicAdd((u64*)(a.state + 1), 1ull);
                atomicOr((u64*)a.state, ST_OPEN);          // cleared by the round that leaves the list empty
            }
        }
    }
}

// Expand `n` LDS frontier entries (global id, value) in chunks of GB entries whose edges are shared out evenly over the workgroup.
// An entry whose vertex no longer holds its value is skipped: whoever lowered it left an entry of their own.
// push(gid, bits) is called once for every vertex this workgroup lowered.
template <class Push>
__device__ void geo_expand(const GeoArgs& a, const int32_t* f_gid, const u64* f_val, int n, Push push, u64& relaxed) {
    __shared__ int s_pre[GB + 1];
    __shared__ int s_beg[GB];
    __shared__ int s_off[GB];
    __shared__ double s_d[GB];
    const int t = threadIdx.x;
    const double cap = a.cap;
    for (int base = 0; base < n; base += GB) {
        int deg = 0, beg = 0, off = 0;
        double d = 0.0;
        if (base + t < n) {
            const int32_t gid = f_gid[base + t];
            const u64 val = f_val[base + t];
            if (ld_agent(a.dist + gid) == val) {
                const int64_t v = gid % a.N;
                beg = a.rowptr[v];
                deg = a.rowptr[v + 1] - beg;
                if (beg < 0 || deg < 0 || (int64_t)beg + deg > a.E2) deg = 0;        // a malformed row is not walked
                off = gid - (int32_t)v;
                d = __longlong_as_double((long long)val);
            }
        }
        s_beg[t] = beg;
        s_off[t] = off;
        s_d[t] = d;
        s_pre[t + 1] = deg;
        if (t == 0) s_pre[0] = 0;
        __syncthreads();
        for (int o = 1; o < GB; o <<= 1) {                 // inclusive scan of s_pre[1..GB]
            const int add = (t >= o) ? s_pre[t + 1 - o] : 0;
            __syncthreads();
            s_pre[t + 1] += add;
            __syncthreads();
        }
        const int total = s_pre[GB];
        for (int e = t; e < total; e += GB) {
            int lo = 0, hi = GB;                           // owner: largest q with s_pre[q] <= e
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_pre[mid] <= e) lo = mid;
                else hi = mid;
            }
            const int idx = s_beg[lo] + (e - s_pre[lo]);
            const double nd = s_d[lo] + a.len[idx];        // the path's length folded from the source outward
            ++relaxed;
            if (!(nd < cap)) continue;                     // at or beyond the cut-off, an infinite or NaN length: never stored
            const int32_t wg = s_off[lo] + a.col[idx];
            const u64 bits = (u64)__double_as_longlong(nd);
            if (ld_agent(a.dist + wg) <= bits) continue;   // values only fall: a stale look can cost an atomic, never lose one
            if (atomicMin(a.dist + wg, bits) > bits) push(wg, bits);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(GB) void k_geo_round(GeoArgs a, int round) {
    __shared__ int32_t s_gid[2][FCAP];
    __shared__ u64 s_val[2][FCAP];
    __shared__ int s_cnt[2];
    __shared__ int s_last;
    __shared__ u64 s_relaxed;
    const int t = threadIdx.x;
    const int par = round & 1, stamp = round + 2;          // this round's pushes are listed for round + 1, whose stamp is round + 2
    const int64_t n = (int64_t)ld_agent(a.ctl + 1 + par);
    if (n <= 0) return;                                    // nothing listed: nothing to do, nobody takes a ticket
    const int32_t* list = a.list[par];
    int32_t* nlist = a.list[par ^ 1];
    u64* ncount = a.ctl + 1 + (par ^ 1);
    auto list_next = [&](int32_t gid) {                    // the next round's list, once per vertex
        if (atomicMax(a.flag + gid, stamp) < stamp) {
            const u64 q = atomicAdd(ncount, 1ull);
            st_agent(nlist + q, gid);
        }
    };
    u64 relaxed = 0;
    if (t == 0) s_relaxed = 0;
    // slices of at most GB entries, sized so that a short list still goes round every workgroup: a round is a chain of dependent
    // memory trips per edge a thread owns, and a frontier of a few thousand vertices in slices of GB would leave most CUs idle
    int64_t per = (n + gridDim.x - 1) / gridDim.x;
    per = per > GB ? GB : per;
    for (int64_t base = (int64_t)blockIdx.x * per; base < n; base += (int64_t)gridDim.x * per) {
        const int mine = (int)(n - base < per ? n - base : per);
        __syncthreads();
        if (t == 0) {
            s_cnt[0] = mine;
            s_cnt[1] = 0;
        }
        if (t < mine) {
            const int32_t gid = ld_agent(list + base + t);
            s_gid[0][t] = gid;
            s_val[0][t] = ld_agent(a.dist + gid);
        }
        __syncthreads();
        int cur = 0;
        for (int lvl = 0; lvl < a.levels; ++lvl) {
            const int nfr = s_cnt[cur];
            if (nfr == 0) break;
            int32_t* ngid = s_gid[cur ^ 1];
            u64* nval = s_val[cur ^ 1];
            int* ncnt = &s_cnt[cur ^ 1];
            auto push = [&](int32_t gid, u64 bits) {
                const int p = atomicAdd(ncnt, 1);
                if (p < FCAP) {
                    ngid[p] = gid;
                    nval[p] = bits;
                } else {
                    list_next(gid);                        // overflow: the global list
                }
            };
            geo_expand(a, s_gid[cur], s_val[cur], nfr < FCAP ? nfr : FCAP, push, relaxed);
            if (t == 0) s_cnt[cur] = 0;
            __syncthreads();
            cur ^= 1;
        }
        const int left = s_cnt[cur] < FCAP ? s_cnt[cur] : FCAP;
        for (int i = t; i < left; i += GB) {               // what the levels left over waits for the next round
            const int32_t gid = s_gid[cur][i];
            if (ld_agent(a.dist + gid) == s_val[cur][i]) list_next(gid);
        }
    }
    if (relaxed) atomicAdd(&s_relaxed, relaxed);
    // ---- ticket: the last workgroup publishes the next round's count
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) {
        if (s_relaxed) atomicAdd((u64*)(a.state + 3), s_relaxed);
        const u64 tk = __hip_atomic_fetch_add(a.ctl, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (tk == (u64)gridDim.x - 1) ? 1 : 0;
    }
    __syncthreads();
    if (!s_last || t != 0) return;
    const long long waiting = (long long)ld_agent(ncount);
    st_agent(a.ctl + 1 + par, 0ull);                       // this round's list is consumed: empty for the round after next
    st_agent(a.ctl, 0ull);                                 // ticket ready for the next launch
    a.state[1] = waiting;
    a.state[2] = (long long)round + 1;
    a.state[0] = (long long)(((u64)a.state[0] & ~ST_OPEN) | (waiting > 0 ? ST_OPEN : 0ull));
}

__global__ __launch_bounds__(GB) void k_geo_mask(const double* __restrict__ dist, int64_t MN, double radius, double ring, int rings,
                                                 int64_t* __restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * GB + threadIdx.x;
    if (i >= MN) return;
    const double d = dist[i];
    int64_t m = 0;
    if (d < radius) {
        m = (int64_t)ceil((radius - d) / ring);
        m = m < rings ? m : rings;
    }
    mask[i] = m;
}

struct GeoLayout {
    size_t ctl, flag, list0, list1, total;
};
GeoLayout geo_layout(int64_t N, int M) {
    GeoLayout L;
    const size_t mn = (size_t)(N > 0 ? N : 1) * (size_t)(M > 0 ? M : 1);
    size_t off = 0;
    L.ctl = off; off += stin_up256(CTL_WORDS * 8);
    L.flag = off; off += stin_up256(mn * 4);
    L.list0 = off; off += stin_up256(mn * 4);
    L.list1 = off; off += stin_up256(mn * 4);
    L.total = off + 256;
    return L;
}

inline char* aligned256(void* p) { return reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(p) + 255) & ~(uintptr_t)255); }

inline bool geo_sizes_ok(int64_t N, int M) { return N >= 0 && M >= 1 && (int64_t)M * (N > 0 ? N : 1) < (int64_t)INT32_MAX; }

GeoArgs geo_args(const int32_t* rowptr, const int32_t* col, const double* length, int64_t N, int64_t E2, int M, double cap,
                 double* dist, int levels, int64_t* state, void* workspace) {
    const GeoLayout L = geo_layout(N, M);
    char* w = aligned256(workspace);
    GeoArgs a;
    a.rowptr = rowptr;
    a.col = col;
    a.len = length;
    a.dist = reinterpret_cast<u64*>(dist);
    a.flag = reinterpret_cast<int32_t*>(w + L.flag);
    a.list[0] = reinterpret_cast<int32_t*>(w + L.list0);
    a.list[1] = reinterpret_cast<int32_t*>(w + L.list1);
    a.ctl = reinterpret_cast<u64*>(w + L.ctl);
    a.state = reinterpret_cast<long long*>(state);
    a.N = N;
    a.E2 = E2;
    a.cap = cap;
    a.levels = levels;
    return a;
}

}  // namespace

extern "C" int stin_geodesic_lengths_f64(const double* vertices, int64_t N, const int32_t* rowptr, const int32_t* col, int64_t E2,
                                         double* length, int64_t* flags, stin_stream_t stream_) {
    stin_clear_stale_error();
    hipStream_t stream = (hipStream_t)stream_;
    STIN_REQUIRE(N >= 0 && N < (int64_t)INT32_MAX && E2 >= 0 && E2 < (int64_t)INT32_MAX, STIN_E_SIZE);
    STIN_REQUIRE(flags != nullptr, STIN_E_NULL);
    hipError_t e = hipMemsetAsync(flags, 0, 8, stream);
    if (e != hipSuccess) return (int)e;
    if (E2 == 0) return STIN_OK;
    STIN_REQUIRE(N >= 1, STIN_E_SIZE);
    STIN_REQUIRE(vertices && rowptr && col && length, STIN_E_NULL);
    hipLaunchKernelGGL(k_geo_lengths, dim3(grid_for(E2)), dim3(GB), 0, stream, vertices, N, rowptr, col, E2, length,
                       reinterpret_cast<long long*>(flags));
    return stin_launch_status();
}

extern "C" size_t stin_geodesic_workspace_bytes(int64_t N, int num_instances) {
    return geo_sizes_ok(N, num_instances) ? geo_layout(N, num_instances).total : 0;
}

extern "C" int stin_geodesic_begin_f64(const int64_t* sources, const int32_t* source_instance, int64_t S, int64_t N, int num_instances,
                                       double* dist, int64_t* state, void* workspace, size_t workspace_bytes, stin_stream_t stream_) {
    stin_clear_stale_error();
    hipStream_t stream = (hipStream_t)stream_;
    STIN_REQUIRE(S >= 0 && N >= 0 && num_instances >= 1, STIN_E_SIZE);
    STIN_REQUIRE(geo_sizes_ok(N, num_instances), STIN_E_UNSUPPORTED);
    STIN_REQUIRE(state != nullptr && workspace != nullptr && (dist != nullptr || N == 0) && (sources != nullptr || S == 0), STIN_E_NULL);
    STIN_REQUIRE(workspace_bytes >= stin_geodesic_workspace_bytes(N, num_instances), STIN_E_WORKSPACE);
    GeoArgs a = geo_args(nullptr, nullptr, nullptr, N, 0, num_instances, 0.0, dist, 1, state, workspace);
    hipError_t e = hipMemsetAsync(state, 0, 4 * 8, stream);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(a.ctl, 0, CTL_WORDS * 8, stream);
    if (e != hipSuccess) return (int)e;
    const int64_t MN = (int64_t)num_instances * N;
    if (MN == 0) return STIN_OK;
    unsigned gi = grid_for(MN);
    gi = gi > 2048 ? 2048 : gi;
    hipLaunchKernelGGL(k_geo_init, dim3(gi), dim3(GB), 0, stream, a.dist, a.flag, MN);
    if (S > 0) hipLaunchKernelGGL(k_geo_seed, dim3(grid_for(S)), dim3(GB), 0, stream, a, sources, source_instance, S, num_instances);
    return stin_launch_status();
}

extern "C" int stin_geodesic_rounds_f64(const int32_t* rowptr, const int32_t* col, const double* length, int64_t N, int64_t E2,
                                        int num_instances, double cap, double* dist, int first_round, int rounds, int levels,
                                        int64_t* state, void* workspace, size_t workspace_bytes, stin_stream_t stream_) {
    stin_clear_stale_error();
    hipStream_t stream = (hipStream_t)stream_;
    STIN_REQUIRE(N >= 0 && E2 >= 0 && E2 < (int64_t)INT32_MAX && num_instances >= 1, STIN_E_SIZE);
    STIN_REQUIRE(rounds >= 1 && rounds <= MAX_ROUNDS_PER_CALL && first_round >= 0 && first_round <= INT32_MAX - 2 - MAX_ROUNDS_PER_CALL,
                 STIN_E_SIZE);
    STIN_REQUIRE(levels >= 1 && levels <= MAX_LEVELS && cap > 0.0, STIN_E_SIZE);                 // (a NaN cap fails here)
    STIN_REQUIRE(geo_sizes_ok(N, num_instances), STIN_E_UNSUPPORTED);
    STIN_REQUIRE(state != nullptr && workspace != nullptr, STIN_E_NULL);
    STIN_REQUIRE(workspace_bytes >= stin_geodesic_workspace_bytes(N, num_instances), STIN_E_WORKSPACE);
    const int64_t MN = (int64_t)num_instances * N;
    if (MN == 0) return STIN_OK;
    STIN_REQUIRE(rowptr && dist && (E2 == 0 || (col && length)), STIN_E_NULL);
    const GeoArgs a = geo_args(rowptr, col, length, N, E2, num_instances, cap, dist, levels, state, workspace);
    // at most one workgroup per CU; a round's list is shared out over them in slices (grid stride)
    int64_t gb = (MN + GB - 1) / GB;
    const int64_t cus = stin_cu_count_dev();
    gb = gb > cus ? cus : gb;
    for (int k = 0; k < rounds; ++k) hipLaunchKernelGGL(k_geo_round, dim3((unsigned)gb), dim3(GB), 0, stream, a, first_round + k);
    return stin_launch_status();
}

extern "C" int stin_geodesic_mask_f64(const double* dist, int64_t count, double radius, int rings, int64_t* mask, stin_stream_t stream_) {
    stin_clear_stale_error();
    hipStream_t stream = (hipStream_t)stream_;
    STIN_REQUIRE(count >= 0 && rings >= 1, STIN_E_SIZE);
    STIN_REQUIRE(radius > 0.0 && radius < __builtin_inf(), STIN_E_SIZE);
    if (count == 0) return STIN_OK;
    STIN_REQUIRE(dist && mask, STIN_E_NULL);
    hipLaunchKernelGGL(k_geo_mask, dim3(grid_for(count)), dim3(GB), 0, stream, dist, count, radius, radius / (double)rings, rings, mask);
    return stin_launch_status();
}
