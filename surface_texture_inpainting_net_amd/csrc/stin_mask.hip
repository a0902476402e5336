// Circle inpainting masks and the training transforms on the device (reference preprocessing/observed_texture_map_generation.py
// :530-603 `process_frame_circles`, transform/random_linear_transformation.py, transform/random_rotation.py).  Contract:
// include/stin_hip.h ("circle masks").
//
//   adjacency: both directions of every edge_index column -> int32 CSR (degree count with integer atomics, rocprim scan, fill with
//              an atomic cursor).  The order inside a row is not fixed, and nothing below depends on it.
//   distance:  dist[m][v] = min(R, hop distance to the nearest centre of mask m), int32.  One launch per batch of centres: a workgroup
//              runs a level-ordered BFS from each of its centres, lowering dist with atomicMin and expanding a vertex only where its
//              own atomicMin lowered it (whoever writes a vertex's final value expands it, so the result is the exact multi-source
//              distance whatever the schedule).  A level's frontier lives in LDS; entries beyond its capacity go to a global list
//              (one entry per vertex: a flag word dedups), which the last-arriving workgroup of the launch drains alone
//              (label-correcting rounds over the global list, bounded by R + 2).  That workgroup then applies the reference's
//              batch-size rule per (mask, graph) and writes the next batch's sizes: launch boundaries are the only grid-wide seams.
//              A vertex is counted as masked when its distance first drops below R, so no reduction per batch is needed.
//   rewrite:   one thread per vertex: x[:, 0:3] = colour * known, x[:, 9] = known, mask = R - dist; normal @ Rz; (pos @ M) @ Rz.
#include <cstring>
#include <rocprim/rocprim.hpp>
#include "stin_common.h"

namespace {

constexpr int MB = 256;          // threads per workgroup
constexpr int FCAP = 2048;       // LDS frontier entries per level buffer
constexpr int CTL_WORDS = 8;     // ticket, global-list count, ktot, status, batch, reserved
constexpr int INFO_HEAD = 5;
constexpr int MAX_SEEDED_GRAPHS = 64;     // per instance: batches, done, capped, masked, total; then sizes[max_iters], counts[max_iters]

// centre i of batch b of mask m, drawn from [0, n) (with replacement): a counter-based hash, no state
__device__ inline int64_t draw_centre(uint64_t seed, int m, int b, int64_t i, int64_t n) {
    uint64_t h = stin_mix64(seed + 0x9E3779B97F4A7C15ull);
    h = stin_mix64(h ^ ((uint64_t)(uint32_t)m << 32 | (uint32_t)b));
    h = stin_mix64(h + (uint64_t)i * 0x9E3779B97F4A7C15ull);
    return (int64_t)(((h >> 32) * (uint64_t)n) >> 32);
}

__device__ inline int graph_of(const int64_t* ptr, int B, int64_t v) {
    int lo = 0, hi = B;                                    // largest g with ptr[g] <= v
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ptr[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ inline int64_t ld_agent(const int64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline int ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void st_agent(int64_t* p, int64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void st_agent(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---------------------------------------------------------------------------------------------------------------- adjacency
__global__ void k_adj_count(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t E, int64_t N,
                            int32_t* __restrict__ deg, int32_t* __restrict__ bad) {
    const int64_t e = (int64_t)blockIdx.x * MB + threadIdx.x;
    if (e >= E) return;
    const int64_t a = src[e], b = dst[e];
    if (a < 0 || a >= N || b < 0 || b >= N) {
        *bad = 1;
        return;
    }
    atomicAdd(deg + a, 1);
    atomicAdd(deg + b, 1);
}

__global__ void k_adj_fill(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t E, int64_t N,
                           int32_t* __restrict__ cursor, int32_t* __restrict__ col) {
    const int64_t e = (int64_t)blockIdx.x * MB + threadIdx.x;
    if (e >= E) return;
    const int64_t a = src[e], b = dst[e];
    if (a < 0 || a >= N || b < 0 || b >= N) return;
    col[atomicAdd(cursor + a, 1)] = (int32_t)b;
    col[atomicAdd(cursor + b, 1)] = (int32_t)a;
}

// ---------------------------------------------------------------------------------------------------------------- distances
struct MaskArgs {
    const int32_t* rowptr;
    const int32_t* col;
    const int64_t* ptr;          // [B + 1] vertex ranges of the graphs
    const int64_t* centres;      // given centres (instance 0) or NULL: hashed draws
    int32_t* dist;               // [M][N]
    int32_t* flag;               // [M][N] "on the global list"
    int32_t* list0;              // [M][N] global overflow list (filled by all workgroups)
    int32_t* list1;              // [M][N] second buffer of the drain
    int64_t* ctl;                // CTL_WORDS
    int64_t* k;                  // [I] centres of the current batch
    int64_t* kofs;               // [I + 1] exclusive prefix of k
    int64_t* info;               // [I][INFO_HEAD + 2 * max_iters]
    int64_t* centre_log;         // [I][log_cap] or NULL
    int64_t N, log_cap;
    uint64_t seed;
    uint64_t graph_seed[MAX_SEEDED_GRAPHS];   // per-graph seeds (has_graph_seeds) instead of `seed`
    int has_graph_seeds;
    double frac;
    int B, M, R, max_iters;
};

__device__ inline int64_t* inst_info(const MaskArgs& a, int j) { return a.info + (int64_t)j * (INFO_HEAD + 2 * a.max_iters); }

// Expand `n` frontier entries (global ids m * N + v) with level value `lvl` (lvl < 0: read each entry's current distance), in
// chunks of MB entries whose edges are shared out evenly over the workgroup (a hub's neighbours are not one lane's loop).
// push(gid) is called once for every vertex whose distance this workgroup lowered; `newly` counts those that were at R.
template <bool FROM_LDS, class Push>
__device__ void expand(const MaskArgs& a, const int32_t* items, int n, int lvl, Push push, int64_t* newly_per_inst, int64_t& newly) {
    __shared__ int s_pre[MB + 1];
    __shared__ int s_beg[MB];
    __shared__ int s_val[MB];
    __shared__ int s_gid[MB];
    const int t = threadIdx.x;
    for (int base = 0; base < n; base += MB) {
        int deg = 0, beg = 0, val = 0, gid = 0;
        if (base + t < n) {
            gid = FROM_LDS ? items[base + t] : ld_agent(items + base + t);
            if (!FROM_LDS) __hip_atomic_store(a.flag + gid, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // may be listed again
            val = lvl >= 0 ? lvl : ld_agent(a.dist + gid);
            if (val < a.R - 1) {
                const int64_t v = gid % a.N;
                beg = a.rowptr[v];
                deg = a.rowptr[v + 1] - beg;
            }
        }
        s_beg[t] = beg;
        s_val[t] = val;
        s_gid[t] = gid;
        s_pre[t + 1] = deg;
        if (t == 0) s_pre[0] = 0;
        __syncthreads();
        for (int o = 1; o < MB; o <<= 1) {                 // inclusive scan of s_pre[1..MB]
            const int add = (t >= o) ? s_pre[t + 1 - o] : 0;
            __syncthreads();
            s_pre[t + 1] += add;
            __syncthreads();
        }
        const int total = s_pre[MB];
        for (int e = t; e < total; e += MB) {
            int lo = 0, hi = MB;                           // owner: largest q with s_pre[q] <= e
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_pre[mid] <= e) lo = mid;
                else hi = mid;
            }
            const int g = s_gid[lo];
            const int64_t moff = (int64_t)(g / a.N) * a.N;
            const int w = a.col[s_beg[lo] + (e - s_pre[lo])];
            const int nv = s_val[lo] + 1;
            const int64_t wg = moff + w;
            const int old = atomicMin(a.dist + wg, nv);
            if (old > nv) {
                if (old >= a.R) {
                    if (newly_per_inst != nullptr) {       // drain: vertices of any (mask, graph)
                        const int j = (int)(wg / a.N) * a.B + graph_of(a.ptr, a.B, w);
                        atomicAdd((unsigned long long*)(newly_per_inst + j), 1ull);
                    } else {
                        ++newly;
                    }
                }
                push((int32_t)wg);
            }
        }
        __syncthreads();
    }
}

// every instance: k = min(10, n), dist = R, no flags, empty lists
__global__ void k_mask_init(MaskArgs a, int64_t given) {
    const int64_t MN = (int64_t)a.M * a.N;
    for (int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x; i < MN; i += (int64_t)gridDim.x * MB) {
        a.dist[i] = a.R;
        a.flag[i] = 0;
    }
    if (blockIdx.x != 0) return;
    const int I = a.M * a.B;
    for (int j = threadIdx.x; j < I; j += MB) {
        const int g = j % a.B;
        const int64_t n = a.ptr[g + 1] - a.ptr[g];
        int64_t k0 = given >= 0 ? given : (n < 10 ? n : 10);
        if (n <= 0) k0 = 0;
        a.k[j] = k0;
        int64_t* inf = inst_info(a, j);
        for (int q = 0; q < INFO_HEAD + 2 * a.max_iters; ++q) inf[q] = 0;
        inf[1] = k0 == 0 ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t s = 0;
        for (int j = 0; j < I; ++j) {
            a.kofs[j] = s;
            s += a.k[j];
        }
        a.kofs[I] = s;
        for (int q = 0; q < CTL_WORDS; ++q) a.ctl[q] = 0;
        a.ctl[2] = s;
    }
}

__global__ __launch_bounds__(MB) void k_mask_batch(MaskArgs a, int b) {
    __shared__ int32_t s_fr[2][FCAP];
    __shared__ int s_cnt[2];
    __shared__ int s_last;
    __shared__ unsigned long long s_new;
    const int t = threadIdx.x;
    const int64_t ktot = a.ctl[2];
    if (ktot <= 0) return;                                 // every instance finished: nothing to do, nobody takes a ticket
    const int I = a.M * a.B;
    if (t == 0) s_new = 0;
    for (int64_t c = blockIdx.x; c < ktot; c += gridDim.x) {
        int lo = 0, hi = I;                                // instance: largest j with kofs[j] <= c
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a.kofs[mid] <= c) lo = mid;
            else hi = mid;
        }
        const int j = lo, m = j / a.B, g = j % a.B;
        const int64_t i = c - a.kofs[j];
        const int64_t v0 = a.ptr[g], n = a.ptr[g + 1] - v0;
        int64_t s = a.centres != nullptr ? a.centres[i] : v0 + draw_centre(a.has_graph_seeds ? a.graph_seed[g] : a.seed, m, b, i, n);
        const int64_t pos = inst_info(a, j)[4] + i;        // position in this instance's log (total before this batch)
        if (t == 0 && a.centre_log != nullptr) {
            if (pos < a.log_cap) a.centre_log[(int64_t)j * a.log_cap + pos] = s;
            else atomicOr((unsigned long long*)(a.ctl + 3), 2ull);          // the log is too short for this draw
        }
        if (s < 0 || s >= a.N) s = -1;
        int64_t newly = 0;
        __syncthreads();
        if (t == 0) {
            s_cnt[0] = 0;
            s_cnt[1] = 0;
            if (s >= 0) {
                const int64_t sg = (int64_t)m * a.N + s;
                const int old = atomicMin(a.dist + sg, 0);
                if (old > 0) {
                    if (old >= a.R) ++newly;
                    s_fr[0][0] = (int32_t)sg;
                    s_cnt[0] = 1;
                }
            }
        }
        __syncthreads();
        int cur = 0;
        for (int lvl = 0; lvl < a.R - 1; ++lvl) {
            const int nfr = s_cnt[cur];
            if (nfr == 0) break;
            int32_t* nxt = s_fr[cur ^ 1];
            int* ncnt = &s_cnt[cur ^ 1];
            auto push = [&](int32_t gid) {
                const int p = atomicAdd(ncnt, 1);
                if (p < FCAP) {
                    nxt[p] = gid;
                } else if (atomicExch(a.flag + gid, 1) == 0) {      // overflow: the global list, once per vertex
                    const int64_t q = atomicAdd((unsigned long long*)(a.ctl + 1), 1ull);
                    st_agent(a.list0 + q, gid);
                }
            };
            expand<true>(a, s_fr[cur], nfr < FCAP ? nfr : FCAP, lvl, push, nullptr, newly);
            if (t == 0) s_cnt[cur] = 0;
            __syncthreads();
            cur ^= 1;
        }
        if (newly) atomicAdd(&s_new, (unsigned long long)newly);
        __syncthreads();
        if (t == 0 && s_new) {
            atomicAdd((unsigned long long*)(inst_info(a, j) + 3), s_new);
            s_new = 0;
        }
        __syncthreads();
    }
    // ---- ticket: the last workgroup drains the global list and applies the batch-size rule
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) {
        const int64_t tk = (int64_t)__hip_atomic_fetch_add((unsigned long long*)a.ctl, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (tk == (int64_t)gridDim.x - 1) ? 1 : 0;
    }
    __syncthreads();
    if (!s_last) return;
    __shared__ int s_n;
    if (t == 0) s_n = (int)ld_agent(a.ctl + 1);
    __syncthreads();
    int32_t* curl = a.list0;
    int32_t* nxtl = a.list1;
    int64_t unused = 0;
    auto push = [&](int32_t gid) {
        if (atomicExch(a.flag + gid, 1) == 0) {
            const int64_t q = atomicAdd((unsigned long long*)(a.ctl + 1), 1ull);
            nxtl[q] = gid;
        }
    };
    for (int round = 0; round < a.R + 2 && s_n > 0; ++round) {
        const int n = s_n;
        __syncthreads();
        if (t == 0) st_agent(a.ctl + 1, (int64_t)0);
        __syncthreads();
        // the masked counts of the drain go to ctl[CTL_WORDS + instance]
        expand<false>(a, curl, n, -1, push, a.ctl + CTL_WORDS, unused);
        __threadfence_block();
        __syncthreads();
        if (t == 0) s_n = (int)ld_agent(a.ctl + 1);
        int32_t* tmp = curl;
        curl = nxtl;
        nxtl = tmp;
        __syncthreads();
    }
    if (t == 0) {
        if (s_n > 0) atomicOr((unsigned long long*)(a.ctl + 3), 1ull);   // drain unfinished (cannot happen within R + 2 rounds)
        st_agent(a.ctl + 1, (int64_t)0);
        st_agent(a.ctl, (int64_t)0);                      // ticket ready for the next launch
    }
    __syncthreads();
    // drain counts (ctl[CTL_WORDS + j]) into the instances, then the rule
    for (int j = t; j < I; j += MB) {
        int64_t* inf = inst_info(a, j);
        const int64_t extra = ld_agent(a.ctl + CTL_WORDS + j);
        st_agent(a.ctl + CTL_WORDS + j, (int64_t)0);
        const int64_t masked = ld_agent(inf + 3) + extra;
        st_agent(inf + 3, masked);
        int64_t knext = 0;
        if (!inf[1]) {
            const int g = j % a.B;
            const int64_t n = a.ptr[g + 1] - a.ptr[g];
            const int64_t kb = a.k[j];
            const int64_t total = inf[4] + kb;
            inf[4] = total;
            if (b < a.max_iters) {
                inf[INFO_HEAD + b] = kb;
                inf[INFO_HEAD + a.max_iters + b] = masked;
            }
            inf[0] = b + 1;
            const double cur = (double)masked / (double)n;
            if (cur >= a.frac || masked == 0) {
                inf[1] = 1;
            } else {
                const double x = (double)total * (a.frac / cur - 1.0);
                if (x >= (double)n) knext = n;
                else knext = (int64_t)x;                   // truncation toward zero, as int() of the reference
                if (knext <= 0) {
                    knext = 0;
                    inf[1] = 1;
                }
            }
            if (!inf[1] && b + 1 >= a.max_iters) {
                inf[2] = 1;                                // iteration cap reached before the rule stopped
                knext = 0;
            }
        }
        a.k[j] = knext;
    }
    __syncthreads();
    if (t == 0) {
        int64_t s = 0;
        for (int j = 0; j < I; ++j) {
            a.kofs[j] = s;
            s += a.k[j];
        }
        a.kofs[I] = s;
        a.ctl[2] = s;
        a.ctl[4] = b + 1;
    }
}

__global__ void k_mask_values(const int32_t* __restrict__ dist, int64_t MN, int R, int64_t* __restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x;
    if (i < MN) mask[i] = (int64_t)(R - dist[i]);
}

// ---------------------------------------------------------------------------------------------------------------- rewrite
struct Mat3 {
    float m[9];
};

template <bool HAS_MASK, bool HAS_LIN, bool HAS_ROT>
__global__ void k_augment_rewrite(float* __restrict__ x, int64_t ldx, const float* __restrict__ color, int64_t ldc,
                                  const int32_t* __restrict__ dist, int R, int64_t* __restrict__ mask, int64_t N, Mat3 lin, Mat3 rot) {
    const int64_t v = (int64_t)blockIdx.x * MB + threadIdx.x;
    if (v >= N) return;
    float* xr = x + v * ldx;
    if (HAS_MASK) {
        const int d = dist[v];
        const float known = d >= R ? 1.f : 0.f;
        const float* cr = color + v * ldc;
        xr[0] = cr[0] * known;
        xr[1] = cr[1] * known;
        xr[2] = cr[2] * known;
        xr[9] = known;
        mask[v] = (int64_t)(R - d);
    }
    if (HAS_ROT) {                                         // normal @ Rz
        const float n0 = xr[3], n1 = xr[4], n2 = xr[5];
        for (int c = 0; c < 3; ++c) xr[3 + c] = (n0 * rot.m[c] + n1 * rot.m[3 + c]) + n2 * rot.m[6 + c];
    }
    if (HAS_LIN || HAS_ROT) {                              // (pos @ M) @ Rz, the product rounded to fp32 in between
        float p0 = xr[6], p1 = xr[7], p2 = xr[8];
        if (HAS_LIN) {
            const float q0 = (p0 * lin.m[0] + p1 * lin.m[3]) + p2 * lin.m[6];
            const float q1 = (p0 * lin.m[1] + p1 * lin.m[4]) + p2 * lin.m[7];
            const float q2 = (p0 * lin.m[2] + p1 * lin.m[5]) + p2 * lin.m[8];
            p0 = q0;
            p1 = q1;
            p2 = q2;
        }
        if (HAS_ROT) {
            const float q0 = (p0 * rot.m[0] + p1 * rot.m[3]) + p2 * rot.m[6];
            const float q1 = (p0 * rot.m[1] + p1 * rot.m[4]) + p2 * rot.m[7];
            const float q2 = (p0 * rot.m[2] + p1 * rot.m[5]) + p2 * rot.m[8];
            p0 = q0;
            p1 = q1;
            p2 = q2;
        }
        xr[6] = p0;
        xr[7] = p1;
        xr[8] = p2;
    }
}

struct MaskLayout {
    size_t flag, list0, list1, ctl, k, kofs, total;
};
MaskLayout mask_layout(int64_t N, int M, int B) {
    MaskLayout L;
    const size_t mn = (size_t)(N > 0 ? N : 1) * (size_t)M;
    const size_t I = (size_t)M * (size_t)B;
    size_t off = 0;
    L.flag = off; off += stin_up256(mn * 4);
    L.list0 = off; off += stin_up256(mn * 4);
    L.list1 = off; off += stin_up256(mn * 4);
    L.ctl = off; off += stin_up256((CTL_WORDS + I) * 8);
    L.k = off; off += stin_up256(I * 8);
    L.kofs = off; off += stin_up256((I + 1) * 8);
    L.total = off;
    return L;
}

size_t adj_scan_bytes(int64_t n) {
    size_t bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, bytes, (int32_t*)nullptr, (int32_t*)nullptr, 0, (size_t)(n > 0 ? n : 1),
                                  rocprim::plus<int32_t>(), (hipStream_t)0);
    return bytes;
}

}  // namespace

extern "C" size_t stin_mask_adjacency_workspace_bytes(int64_t N) {
    return stin_up256((size_t)(N + 1) * 4) * 2 + stin_up256(adj_scan_bytes(N + 1));
}

extern "C" int stin_mask_adjacency_i64(const int64_t* src, const int64_t* dst, int64_t E, int64_t N, int32_t* rowptr, int32_t* col,
                                       int32_t* bad, void* workspace, size_t workspace_bytes, stin_stream_t stream_) {
    STIN_REQUIRE(N >= 0 && E >= 0 && 2 * E < (int64_t)INT32_MAX && N < (int64_t)INT32_MAX, STIN_E_SIZE);
    STIN_REQUIRE(rowptr != nullptr && bad != nullptr && (E == 0 || (src && dst && col)), STIN_E_NULL);
    STIN_REQUIRE(workspace != nullptr && workspace_bytes >= stin_mask_adjacency_workspace_bytes(N), STIN_E_WORKSPACE);
    hipStream_t stream = (hipStream_t)stream_;
    stin_clear_stale_error();
    char* w = (char*)workspace;
    int32_t* deg = (int32_t*)w;
    int32_t* cursor = (int32_t*)(w + stin_up256((size_t)(N + 1) * 4));
    void* temp = w + 2 * stin_up256((size_t)(N + 1) * 4);
    size_t temp_bytes = stin_up256(adj_scan_bytes(N + 1));
    (void)hipMemsetAsync(deg, 0, (size_t)(N + 1) * 4, stream);
    (void)hipMemsetAsync(bad, 0, 4, stream);
    const unsigned ge = (unsigned)((E + MB - 1) / MB);
    if (E > 0) hipLaunchKernelGGL(k_adj_count, dim3(ge), dim3(MB), 0, stream, src, dst, E, N, deg, bad);
    hipError_t e = rocprim::exclusive_scan(temp, temp_bytes, deg, rowptr, 0, (size_t)(N + 1), rocprim::plus<int32_t>(), stream);
    if (e != hipSuccess) return (int)e;
    (void)hipMemcpyAsync(cursor, rowptr, (size_t)(N + 1) * 4, hipMemcpyDeviceToDevice, stream);
    if (E > 0) hipLaunchKernelGGL(k_adj_fill, dim3(ge), dim3(MB), 0, stream, src, dst, E, N, cursor, col);
    return stin_launch_status();
}

extern "C" size_t stin_circle_mask_workspace_bytes(int64_t N, int num_masks, int num_graphs) {
    return mask_layout(N, num_masks, num_graphs).total;
}

extern "C" int stin_circle_mask_run(const int32_t* rowptr, const int32_t* col, int64_t N, const int64_t* ptr, int num_graphs,
                                    int num_masks, int radius, double frac, uint64_t seed, const int64_t* graph_seeds, int max_iters,
                                    const int64_t* centres,
                                    int64_t num_centres, int32_t* dist, int64_t* mask, int64_t* info, int64_t* centre_log,
                                    int64_t log_cap, void* workspace, size_t workspace_bytes, stin_stream_t stream_) {
    STIN_REQUIRE(rowptr && ptr && dist && info, STIN_E_NULL);
    STIN_REQUIRE(N >= 0 && num_graphs >= 1 && num_masks >= 1 && max_iters >= 1 && max_iters <= 1024, STIN_E_SIZE);
    STIN_REQUIRE(radius >= 1 && radius <= (1 << 20), STIN_E_SIZE);
    STIN_REQUIRE((int64_t)num_masks * (N > 0 ? N : 1) < (int64_t)INT32_MAX, STIN_E_UNSUPPORTED);
    STIN_REQUIRE(graph_seeds == nullptr || num_graphs <= MAX_SEEDED_GRAPHS, STIN_E_UNSUPPORTED);
    STIN_REQUIRE(centres == nullptr || (num_masks == 1 && num_graphs == 1 && num_centres >= 0), STIN_E_SIZE);
    STIN_REQUIRE(workspace != nullptr && workspace_bytes >= stin_circle_mask_workspace_bytes(N, num_masks, num_graphs), STIN_E_WORKSPACE);
    hipStream_t stream = (hipStream_t)stream_;
    stin_clear_stale_error();
    const MaskLayout L = mask_layout(N, num_masks, num_graphs);
    char* w = (char*)workspace;
    MaskArgs a;
    a.rowptr = rowptr;
    a.col = col;
    a.ptr = ptr;
    a.centres = centres;
    a.dist = dist;
    a.flag = (int32_t*)(w + L.flag);
    a.list0 = (int32_t*)(w + L.list0);
    a.list1 = (int32_t*)(w + L.list1);
    a.ctl = (int64_t*)(w + L.ctl);
    a.k = (int64_t*)(w + L.k);
    a.kofs = (int64_t*)(w + L.kofs);
    a.info = info;
    a.centre_log = log_cap > 0 ? centre_log : nullptr;
    a.N = N;
    a.log_cap = log_cap;
    a.seed = seed;
    a.has_graph_seeds = graph_seeds != nullptr;
    for (int g = 0; g < MAX_SEEDED_GRAPHS; ++g) a.graph_seed[g] = (graph_seeds != nullptr && g < num_graphs) ? (uint64_t)graph_seeds[g] : 0;
    a.frac = frac;
    a.B = num_graphs;
    a.M = num_masks;
    a.R = radius;
    a.max_iters = centres != nullptr ? 1 : max_iters;
    const int64_t MN = (int64_t)num_masks * N;
    const int64_t I = (int64_t)num_masks * num_graphs;
    (void)hipMemsetAsync(a.ctl, 0, (CTL_WORDS + I) * 8, stream);
    unsigned gi = (unsigned)((MN + MB - 1) / MB);
    gi = gi < 1 ? 1 : (gi > 2048 ? 2048 : gi);
    hipLaunchKernelGGL(k_mask_init, dim3(gi), dim3(MB), 0, stream, a, centres != nullptr ? num_centres : (int64_t)-1);
    // one workgroup per CU; a batch's centres are shared out over them (grid stride)
    int64_t gb = N > 0 ? N : 1;
    gb = gb > 256 ? 256 : gb;
    for (int b = 0; b < a.max_iters; ++b) hipLaunchKernelGGL(k_mask_batch, dim3((unsigned)gb), dim3(MB), 0, stream, a, b);
    if (mask != nullptr && MN > 0)
        hipLaunchKernelGGL(k_mask_values, dim3((unsigned)((MN + MB - 1) / MB)), dim3(MB), 0, stream, dist, MN, radius, mask);
    // status word after the instances' rows: bit 0 drain unfinished, bit 1 centres beyond the log
    (void)hipMemcpyAsync(info + I * (INFO_HEAD + 2 * a.max_iters), a.ctl + 3, 8, hipMemcpyDeviceToDevice, stream);
    return stin_launch_status();
}

extern "C" int stin_augment_rewrite_f32(float* x, int64_t ldx, const float* color, int64_t ldc, const int32_t* dist, int radius,
                                        int64_t* mask, int64_t N, const float* lin, const float* rot, stin_stream_t stream_) {
    STIN_REQUIRE(N >= 0 && ldx >= 10 && (dist == nullptr || ldc >= 3), STIN_E_SIZE);
    STIN_REQUIRE(x != nullptr || N == 0, STIN_E_NULL);
    STIN_REQUIRE(dist == nullptr || (color != nullptr && mask != nullptr), STIN_E_NULL);
    if (N == 0 || (dist == nullptr && lin == nullptr && rot == nullptr)) return STIN_OK;
    hipStream_t stream = (hipStream_t)stream_;
    stin_clear_stale_error();
    Mat3 L{}, Rm{};
    for (int i = 0; i < 9; ++i) {
        L.m[i] = lin ? lin[i] : 0.f;
        Rm.m[i] = rot ? rot[i] : 0.f;
    }
    const dim3 grid((unsigned)((N + MB - 1) / MB));
    const int sel = (dist ? 4 : 0) | (lin ? 2 : 0) | (rot ? 1 : 0);
#define STIN_AUG(A, B_, C)                                                                                                   \
    case (A ? 4 : 0) | (B_ ? 2 : 0) | (C ? 1 : 0):                                                                          \
        hipLaunchKernelGGL((k_augment_rewrite<A, B_, C>), grid, dim3(MB), 0, stream, x, ldx, color, ldc, dist, radius, mask, N, L, Rm); \
        break;
    switch (sel) {
        STIN_AUG(true, true, true)
        STIN_AUG(true, true, false)
        STIN_AUG(true, false, true)
        STIN_AUG(true, false, false)
        STIN_AUG(false, true, true)
        STIN_AUG(false, true, false)
        STIN_AUG(false, false, true)
        default: break;
    }
#undef STIN_AUG
    return stin_launch_status();
}
