// Harmonic fill: every masked vertex becomes the weighted mean of its neighbours, the known vertices being boundary values - the
// zero of the graph Laplacian on the hole - by Jacobi-preconditioned CG in a fixed order of operations.  Contract:
// include/stin_hip.h ("Harmonic fill"); tests/_harmonic_oracle.py restates it in numpy and the device agrees bit for bit.
//
//   reach:    one byte per vertex (0 known, 1 masked, 2 reached); a round is one launch, one thread per vertex, a masked vertex
//             that finds a known or reached neighbour becomes reached.  Bytes only go 1 -> 2, so a flag set in the same launch
//             may be seen or not: the least fixed point is the same.  One count per round (a ballot, one atomic per wave).
//   setup:    the unknowns = the reached vertices in ascending id (block counts, one scan workgroup, a ranked scatter), then one
//             thread per unknown: d, b, r = b, z = b / d, x = 0, the unknown index of every slot of its row (ucol: -1 for a self
//             slot or a known neighbour) and its checked slot range (urow), so that the product never looks a vertex up again,
//             and the <r, z>, <b, b> tile sums.
//   iterate:  two launches per iteration, one workgroup per tile of 256 unknowns, one thread per unknown for all C channels.
//             product k: every workgroup folds the <r, r> and <r, z> tile sums of update k - 1 itself (staged in LDS with one trip
//             to memory, then lanes 0 .. 15 and 16 .. 31 add them in ascending tile order), decides per channel (done? else beta), forms p = z + beta p_old for its own row and, on the
//             fly, for the neighbours it gathers (p_old is the other of two ping-pong buffers, so nobody reads what this launch
//             writes), q = d p - acc and the <p, q> tile sum.  update k: folds <p, q>, alpha = rz / pq, x, r, z and the
//             <r, r>, <r, z> tile sums.  The per-channel scalars live in two tables: the product reads SB and its workgroup 0
//             writes SA, the update reads SA and its workgroup 0 writes SB - no launch reads a word it writes, so launch
//             boundaries are the only seams: no atomics, no cooperative launch, no grid-wide wait, no in-kernel loop that is not
//             bounded by a row's degree or the tile count.
//             A channel that is done or stopped is skipped by both kernels: its bytes freeze.
//   tile sum: products in LDS, s[j] += s[j + h] for h = 128, 64 through LDS and 32 .. 1 by shuffle-down in wave 0 (lane j < h adds
//             lane j + h, whose value is the tree's as long as j + h < 2 h: the same tree).
#include "stin_common.h"

namespace {

constexpr int HB = 256;                      // threads per workgroup = unknowns per tile (part of the contract)
constexpr int MAXC = STIN_HARMONIC_MAX_C;
constexpr int PSTRIDE = MAXC;                // doubles per tile in a tile-sum array
constexpr int MAX_REACH_ROUNDS = 64;
constexpr int MAX_ITER_PER_CALL = 4096;
constexpr int SMALL_PT = 8;                 // the one-workgroup kernels stage 8 tile sums per thread: 2048 doubles
// doubles of LDS per thread of an iteration kernel: its tile_sums need CT, and 8 lets one chunk hold 341 tiles of 3 channels twice
constexpr int iter_pt(int CT) { return CT > 8 ? CT : 8; }
constexpr long long ST_WEIGHT = 1, ST_VALUE = 2, ST_INDEX = 4;
constexpr long long F_DONE = 1, F_BREAK = 2, F_NOTCONV = 4, F_PENDING = 8;      // F_PENDING: internal (an update awaits its decision)

struct ChanState {
    double rz, bb, rr;
    long long it, flags;
};

inline unsigned grid_for(int64_t n) { return (unsigned)((n + HB - 1) / HB); }

__device__ inline uint8_t ld_flag(const uint8_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void st_flag(uint8_t* p, uint8_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the slots of row i, or an empty range (and false) when rowptr does not describe one inside [0, E2]
__device__ inline bool row_range(const int32_t* __restrict__ rowptr, int64_t i, int64_t E2, int& beg, int& end) {
    beg = rowptr[i];
    end = rowptr[i + 1];
    if (beg < 0 || end < beg || (int64_t)end > E2) {
        beg = end = 0;
        return false;
    }
    return true;
}

// ------------------------------------------------------------------------------------------------------------------- reach
__global__ __launch_bounds__(HB) void k_harm_flag_init(const uint8_t* __restrict__ masked, int64_t N, uint8_t* __restrict__ flag,
                                                       long long* __restrict__ state) {
    const int64_t i = (int64_t)blockIdx.x * HB + threadIdx.x;
    const bool m = i < N && masked[i] != 0;
    if (i < N) flag[i] = m ? 1 : 0;
    const unsigned long long b = __ballot(m);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd((unsigned long long*)(state + 4), (unsigned long long)__popcll(b));
}

__global__ __launch_bounds__(HB) void k_harm_reach(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t N,
                                                   int64_t E2, uint8_t* flag, long long* __restrict__ state) {
    const int64_t i = (int64_t)blockIdx.x * HB + threadIdx.x;
    bool hit = false, bad = false;
    if (i < N && ld_flag(flag + i) == 1) {
        int beg, end;
        bad = !row_range(rowptr, i, E2, beg, end);
        for (int s = beg; s < end; ++s) {
            const int64_t j = col[s];
            if (j == i) continue;
            if (j < 0 || j >= N) {
                bad = true;
                continue;
            }
            if (ld_flag(flag + j) != 1) {
                hit = true;
                break;
            }
        }
        if (hit) st_flag(flag + i, 2);
    }
    const unsigned long long b = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && b) {
        const unsigned long long c = (unsigned long long)__popcll(b);
        atomicAdd((unsigned long long*)(state + 3), c);
        atomicAdd((unsigned long long*)(state + 1), c);
    }
    if (bad) atomicOr((unsigned long long*)state, (unsigned long long)ST_INDEX);
}

// ------------------------------------------------------------------------------------------------------- the unknown list
__global__ __launch_bounds__(HB) void k_harm_count(const uint8_t* __restrict__ flag, int64_t N, int32_t* __restrict__ bc) {
    __shared__ int s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * HB + threadIdx.x;
    const unsigned long long b = __ballot(i < N && flag[i] == 2);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&s_n, (int)__popcll(b));       // (integer: the order does not matter)
    __syncthreads();
    if (threadIdx.x == 0) bc[blockIdx.x] = s_n;
}

// one workgroup: bc[0 .. nb) -> its exclusive prefix sums in place; a total that is not n_U marks the state (nothing depends on it:
// every later write is guarded by n_U)
__global__ __launch_bounds__(HB) void k_harm_scan(int32_t* __restrict__ bc, int64_t nb, int64_t n_U, long long* __restrict__ state) {
    __shared__ long long s[HB];
    __shared__ long long s_carry;
    const int t = threadIdx.x;
    if (t == 0) s_carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < nb; base += HB) {
        const long long v = base + t < nb ? bc[base + t] : 0;
        s[t] = v;
        __syncthreads();
        for (int o = 1; o < HB; o <<= 1) {
            const long long add = t >= o ? s[t - o] : 0;
            __syncthreads();
            s[t] += add;
            __syncthreads();
        }
        const long long carry = s_carry;
        if (base + t < nb) {
            const long long ex = carry + s[t] - v;
            bc[base + t] = (int32_t)(ex < (long long)INT32_MAX ? ex : INT32_MAX);
        }
        __syncthreads();
        if (t == HB - 1) s_carry = carry + s[t];
        __syncthreads();
    }
    if (t == 0 && s_carry != (long long)n_U) atomicOr((unsigned long long*)state, (unsigned long long)ST_INDEX);
}

__global__ __launch_bounds__(HB) void k_harm_scatter(const uint8_t* __restrict__ flag, int64_t N, const int32_t* __restrict__ bo,
                                                     int64_t n_U, int32_t* __restrict__ unk, int32_t* __restrict__ inv) {
    __shared__ int s_w[HB / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t i = (int64_t)blockIdx.x * HB + t;
    const bool is = i < N && flag[i] == 2;
    const unsigned long long b = __ballot(is);
    if (lane == 0) s_w[w] = (int)__popcll(b);
    __syncthreads();
    int before = 0;
    for (int q = 0; q < w; ++q) before += s_w[q];
    const int64_t u = (int64_t)bo[blockIdx.x] + before + (int)__popcll(b & ((1ull << lane) - 1ull));
    if (i < N) {
        const bool ok = is && u < n_U;
        inv[i] = ok ? (int32_t)u : -1;
        if (ok) unk[u] = (int32_t)i;
    }
}

// ------------------------------------------------------------------------------------------------------------- tile sums
// v[c] of this thread -> the tile's tree sum of channel c in out[c] (c < C); all threads of the workgroup call it.  buf: CT * HB
// doubles of LDS.
template <int CT>
__device__ inline void tile_sums(const double (&v)[CT], int C, double* __restrict__ out, double* buf) {
    const int t = threadIdx.x;
    __syncthreads();                                       // (the previous use of buf is over)
#pragma unroll
    for (int c = 0; c < CT; ++c) buf[c * HB + t] = v[c];
    __syncthreads();
    if (t < 128) {
#pragma unroll
        for (int c = 0; c < CT; ++c) buf[c * HB + t] += buf[c * HB + t + 128];
    }
    __syncthreads();
    if (t < 64) {
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            double a = buf[c * HB + t] + buf[c * HB + t + 64];
#pragma unroll
            for (int h = 32; h > 0; h >>= 1) a += __shfl_down(a, h, 64);
            if (t == 0 && c < C) out[c] = a;
        }
    }
}

// The tile sums of one or two arrays (P1 may be NULL) folded in ascending tile order from +0.0, for the channels of `want` (uniform
// over the workgroup): the workgroup stages as many tiles as buf holds with one trip to memory, then lane c (array 0) and lane
// MAXC + c (array 1) add them up in order from LDS - a serial chain of additions, not of memory trips.  buf: PER_THREAD doubles of
// LDS per thread of the workgroup; out: LDS [2][MAXC].  Ends with a barrier.
template <int PER_THREAD>
__device__ inline void fold_tiles(const double* __restrict__ P0, const double* __restrict__ P1, int64_t T, int C, unsigned want,
                                  double* buf, double* out) {
    const int t = threadIdx.x, nt = blockDim.x;
    const int buf_doubles = PER_THREAD * nt;
    const int narr = P1 != nullptr ? 2 : 1;
    const int cap = buf_doubles / (narr * C);              // tiles per chunk
    const int arr = t / MAXC, c = t % MAXC;
    const bool mine = arr < narr && c < C && (want >> c & 1u);
    double acc = 0.0;
    for (int64_t base = 0; base < T; base += cap) {
        const int m = (int)(T - base < cap ? T - base : cap);
        __syncthreads();                                   // (the previous chunk, or the previous use of buf, is over)
        double v[PER_THREAD];                              // all loads of a chunk in flight, then the LDS stores
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) {
            const int i = t + q * nt;
            if (i < narr * m * C) {
                const int a = i / (m * C), rem = i - a * (m * C), tt = rem / C, cc = rem - tt * C;
                v[q] = (a ? P1 : P0)[(base + tt) * PSTRIDE + cc];
            }
        }
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) {
            const int i = t + q * nt;
            if (i < narr * m * C) buf[i] = v[q];
        }
        __syncthreads();
        if (mine) {                                        // sixteen LDS reads in flight, the additions in order
            const double* b = buf + arr * (m * C) + c;
            int tt = 0;
            for (; tt + 16 <= m; tt += 16) {
                double v[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) v[q] = b[(tt + q) * C];
#pragma unroll
                for (int q = 0; q < 16; ++q) acc += v[q];
            }
            for (; tt < m; ++tt) acc += b[tt * C];
        }
    }
    if (mine) out[arr * MAXC + c] = acc;
    __syncthreads();
}

struct HarmArgs {
    const int32_t* rowptr;
    const double* weight;        // NULL: all 1.0
    const int32_t* unk;          // [n_U] vertex of an unknown
    const int32_t* ucol;         // [E2] unknown index of a slot, -1 = skipped (rows of unknowns only)
    int2* urow;                  // [n_U] the checked slot range [x, y) of an unknown's row
    const double* d;             // [n_U]
    double *x, *r, *z, *q;       // [n_U][C]
    double* p[2];                // [n_U][C] ping-pong
    double *Ppq, *Prr, *Prz;     // [T][PSTRIDE] tile sums
    ChanState *SA, *SB;          // [MAXC] each
    int64_t N, n_U, T, E2;
    double tol2;
    int C;
};

// What the product and the report decide from SB and the tile sums of the last update: <r, r> and <r, z> are folded where an update
// is pending, then lane c < C decides channel c.  Results in LDS: s_st (the channel's new state), s_beta, s_mode (0 frozen, 1 first
// iteration: p = z, 2: p = z + beta p).  Ends with a barrier.
template <int PER_THREAD>
__device__ inline void harm_decide(const HarmArgs& a, ChanState* s_st, double* s_beta, int* s_mode, double* buf) {
    __shared__ double s_f[2 * MAXC];
    const int t = threadIdx.x;
    if (t < a.C) s_st[t] = a.SB[t];
    __syncthreads();
    unsigned want = 0;
    for (int c = 0; c < a.C; ++c)
        if (s_st[c].flags & F_PENDING) want |= 1u << c;
    if (want) fold_tiles<PER_THREAD>(a.Prr, a.Prz, a.T, a.C, want, buf, s_f);
    else __syncthreads();                                  // (s_st is rewritten below)
    if (t < a.C) {
        ChanState s = s_st[t];
        int mode = 0;
        double beta = 0.0;
        if (!(s.flags & (F_DONE | F_BREAK))) {
            if (s.flags & F_PENDING) {
                s.flags &= ~F_PENDING;
                s.rr = s_f[t];
                if (s.rr <= a.tol2 * s.bb) {
                    s.flags |= F_DONE;
                } else {
                    const double rzn = s_f[MAXC + t];
                    beta = rzn / s.rz;
                    s.rz = rzn;
                    mode = 2;
                }
            } else {
                mode = 1;
            }
        }
        s_st[t] = s;
        s_beta[t] = beta;
        s_mode[t] = mode;
    }
    __syncthreads();
}

// --------------------------------------------------------------------------------------------------------------- setup rows
template <int CT>
__global__ __launch_bounds__(HB) void k_harm_rows(HarmArgs a, const int32_t* __restrict__ col, const float* __restrict__ values,
                                                  const uint8_t* __restrict__ flag, const int32_t* __restrict__ inv, int64_t N,
                                                  int32_t* __restrict__ ucol, double* __restrict__ d_out,
                                                  long long* __restrict__ state) {
    __shared__ double s_buf[CT * HB];
    const int C = a.C;
    const int64_t u = (int64_t)blockIdx.x * HB + threadIdx.x;
    double prz[CT], pbb[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) prz[c] = pbb[c] = 0.0;
    if (u < a.n_U) {
        const int64_t i = a.unk[u];
        int beg = 0, end = 0;
        long long bad = (i >= 0 && i < N && row_range(a.rowptr, i, a.E2, beg, end)) ? 0 : ST_INDEX;
        double d = 0.0, b[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) b[c] = 0.0;
        for (int s = beg; s < end; ++s) {
            const int64_t j = col[s];
            int32_t uc = -1;
            if (j < 0 || j >= N) {
                bad |= ST_INDEX;
            } else if (j != i) {
                const double w = a.weight != nullptr ? a.weight[s] : 1.0;
                if (!(w > 0.0 && w < __builtin_inf())) bad |= ST_WEIGHT;
                d += w;
                const uint8_t f = flag[j];
                if (f == 0) {
#pragma unroll
                    for (int c = 0; c < CT; ++c) {
                        if (c < C) {
                            const double v = (double)values[j * C + c];
                            if (!(fabs(v) < __builtin_inf())) bad |= ST_VALUE;
                            b[c] += w * v;
                        }
                    }
                } else if (f == 2) {
                    uc = inv[j];
                }
            }
            ucol[s] = uc;
        }
        d_out[u] = d;
        a.urow[u] = make_int2(beg, end);
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            if (c < C) {
                const double z = b[c] / d;
                a.x[u * C + c] = 0.0;
                a.r[u * C + c] = b[c];
                a.z[u * C + c] = z;
                prz[c] = b[c] * z;
                pbb[c] = b[c] * b[c];
            }
        }
        if (bad) atomicOr((unsigned long long*)state, (unsigned long long)bad);
    }
    tile_sums<CT>(prz, C, a.Prz + (int64_t)blockIdx.x * PSTRIDE, s_buf);
    tile_sums<CT>(pbb, C, a.Prr + (int64_t)blockIdx.x * PSTRIDE, s_buf);
}

// one workgroup: rz = <r, z>, bb = <b, b>, rr = bb; bb == 0: done with no iteration
__global__ __launch_bounds__(HB) void k_harm_start(HarmArgs a) {
    __shared__ double s_buf[SMALL_PT * HB];
    __shared__ double s_f[2 * MAXC];
    const int t = threadIdx.x;
    fold_tiles<SMALL_PT>(a.Prr, a.Prz, a.T, a.C, (1u << a.C) - 1u, s_buf, s_f);
    if (t < MAXC) {
        ChanState s;
        s.rz = t < a.C ? s_f[MAXC + t] : 0.0;
        s.bb = t < a.C ? s_f[t] : 0.0;
        s.rr = s.bb;
        s.it = 0;
        s.flags = (t < a.C && s.bb == 0.0) ? F_DONE : 0;
        a.SB[t] = s;
        a.SA[t] = s;
    }
}

// ------------------------------------------------------------------------------------------------------------- iteration k
template <int CT>
__global__ __launch_bounds__(HB) void k_harm_product(HarmArgs a, int k) {
    __shared__ ChanState s_st[MAXC];
    __shared__ double s_beta[MAXC];
    __shared__ int s_mode[MAXC];
    __shared__ double s_buf[iter_pt(CT) * HB];
    const int C = a.C, t = threadIdx.x;
    harm_decide<iter_pt(CT)>(a, s_st, s_beta, s_mode, s_buf);
    if (blockIdx.x == 0 && t < C) a.SA[t] = s_st[t];
    int mode[CT];
    double beta[CT];
    bool any = false;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        mode[c] = c < C ? s_mode[c] : 0;
        beta[c] = c < C ? s_beta[c] : 0.0;
        any = any || mode[c] != 0;
    }
    if (!any) return;                                      // every channel is frozen (uniform over the grid)
    const double* __restrict__ po = a.p[(k & 1) ^ 1];
    double* __restrict__ pn = a.p[k & 1];
    const double* __restrict__ z = a.z;
    const int64_t u = (int64_t)blockIdx.x * HB + t;
    double prod[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) prod[c] = 0.0;
    if (u < a.n_U) {
        double own[CT], acc[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            acc[c] = 0.0;
            own[c] = 0.0;
            if (mode[c] == 1) own[c] = z[u * C + c];
            else if (mode[c] == 2) own[c] = z[u * C + c] + beta[c] * po[u * C + c];
            if (mode[c] != 0) pn[u * C + c] = own[c];
        }
        const int2 row = a.urow[u];
        for (int s = row.x; s < row.y; ++s) {
            const int64_t v = a.ucol[s];
            if (v < 0 || v >= a.n_U) continue;                 // a self slot or a known neighbour
            const bool weighted = a.weight != nullptr;
            const double w = weighted ? a.weight[s] : 1.0;
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                if (mode[c] != 0) {
                    double pj = z[v * C + c];
                    if (mode[c] == 2) pj = pj + beta[c] * po[v * C + c];
                    acc[c] += weighted ? w * pj : pj;      // (1.0 * pj is pj exactly)
                }
            }
        }
        const double d = a.d[u];
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            if (mode[c] != 0) {
                const double q = d * own[c] - acc[c];
                a.q[u * C + c] = q;
                prod[c] = own[c] * q;
            }
        }
    }
    tile_sums<CT>(prod, C, a.Ppq + (int64_t)blockIdx.x * PSTRIDE, s_buf);
}

template <int CT>
__global__ __launch_bounds__(HB) void k_harm_update(HarmArgs a, int k) {
    __shared__ double s_alpha[MAXC];
    __shared__ int s_act[MAXC];
    __shared__ double s_f[2 * MAXC];
    __shared__ ChanState s_st[MAXC];
    __shared__ double s_buf[iter_pt(CT) * HB];
    const int C = a.C, t = threadIdx.x;
    if (t < C) s_st[t] = a.SA[t];
    __syncthreads();
    unsigned want = 0;
    for (int c = 0; c < C; ++c)
        if (!(s_st[c].flags & (F_DONE | F_BREAK))) want |= 1u << c;
    if (want == 0) {                                       // every channel is frozen (uniform over the grid)
        if (blockIdx.x == 0 && t < C) a.SB[t] = s_st[t];
        return;
    }
    fold_tiles<iter_pt(CT)>(a.Ppq, nullptr, a.T, C, want, s_buf, s_f);
    if (t < C) {
        ChanState s = s_st[t];
        int act = 0;
        double alpha = 0.0;
        if (want >> t & 1u) {
            const double pq = s_f[t];
            if (!(pq > 0.0)) {
                s.flags |= F_BREAK;
            } else {
                alpha = s.rz / pq;
                s.it += 1;
                s.flags |= F_PENDING;
                act = 1;
            }
        }
        s_alpha[t] = alpha;
        s_act[t] = act;
        if (blockIdx.x == 0) a.SB[t] = s;
    }
    __syncthreads();
    unsigned act = 0;                                      // bit c: channel c takes this update
    double alpha[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        if (c < C && s_act[c] != 0) act |= 1u << c;
        alpha[c] = c < C ? s_alpha[c] : 0.0;
    }
    if (act == 0) return;                                  // every channel is frozen (uniform over the grid)
    const double* __restrict__ p = a.p[k & 1];
    const int64_t u = (int64_t)blockIdx.x * HB + t;
    double prr[CT], prz[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) prr[c] = prz[c] = 0.0;
    if (u < a.n_U) {
        const double d = a.d[u];
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            if (act >> c & 1u) {
                const int64_t o = u * C + c;
                a.x[o] = a.x[o] + alpha[c] * p[o];
                const double r = a.r[o] - alpha[c] * a.q[o];
                const double z = r / d;
                a.r[o] = r;
                a.z[o] = z;
                prr[c] = r * r;
                prz[c] = r * z;
            }
        }
    }
    tile_sums<CT>(prr, C, a.Prr + (int64_t)blockIdx.x * PSTRIDE, s_buf);
    tile_sums<CT>(prz, C, a.Prz + (int64_t)blockIdx.x * PSTRIDE, s_buf);
}

// one workgroup: the state table as the next product would decide it (SB is left alone); final: the not-converged bit and the
// number of masked vertices never reached
__global__ __launch_bounds__(HB) void k_harm_report(HarmArgs a, long long* __restrict__ state, int final_) {
    __shared__ ChanState s_st[MAXC];
    __shared__ double s_beta[MAXC];
    __shared__ int s_mode[MAXC];
    __shared__ double s_buf[SMALL_PT * HB];
    harm_decide<SMALL_PT>(a, s_st, s_beta, s_mode, s_buf);
    const int t = threadIdx.x;
    if (t < MAXC) {
        long long w[4] = {0, 0, 0, 0};
        if (t < a.C) {
            const ChanState s = s_st[t];
            w[0] = s.it;
            w[1] = __double_as_longlong(s.rr);
            w[2] = __double_as_longlong(s.bb);
            w[3] = (s.flags & (F_DONE | F_BREAK)) | ((final_ && !(s.flags & F_DONE)) ? F_NOTCONV : 0);
        }
        for (int q = 0; q < 4; ++q) state[8 + 4 * t + q] = w[q];
    }
    if (t == 0 && final_) state[2] = state[4] - state[1];
}

__global__ __launch_bounds__(HB) void k_harm_out(const float* __restrict__ values, const uint8_t* __restrict__ flag,
                                                 const int32_t* __restrict__ inv, const double* __restrict__ x, int64_t NC, int C,
                                                 int64_t n_U, float fill, float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * HB + threadIdx.x;
    if (e >= NC) return;
    const int64_t v = e / C;
    const int c = (int)(e - v * C);
    const uint8_t f = flag[v];
    float o = fill;
    if (f == 0) {
        o = values[e];
    } else if (f == 2) {
        const int64_t u = inv[v];
        if (u >= 0 && u < n_U) o = (float)x[u * C + c];
    }
    out[e] = o;
}

// ------------------------------------------------------------------------------------------------------------------ host side
struct HarmLayout {
    size_t SA, SB, bc, unk, inv, ucol, urow, d, x, r, z, q, p0, p1, Ppq, Prr, Prz, total;
};

inline bool harm_sizes_ok(int64_t N, int64_t E2, int64_t n_U, int C) {
    return N >= 0 && N < (int64_t)INT32_MAX && E2 >= 0 && E2 < (int64_t)INT32_MAX && n_U >= 0 && n_U <= N && C >= 1 && C <= MAXC;
}

HarmLayout harm_layout(int64_t N, int64_t E2, int64_t n_U, int C) {
    HarmLayout L;
    const size_t n = (size_t)(N > 0 ? N : 1), e = (size_t)(E2 > 0 ? E2 : 1), nu = (size_t)(n_U > 0 ? n_U : 1);
    const size_t T = (nu + HB - 1) / HB, vec = nu * (size_t)C * 8;
    size_t off = 0;
    L.SA = off; off += stin_up256(MAXC * sizeof(ChanState));
    L.SB = off; off += stin_up256(MAXC * sizeof(ChanState));
    L.bc = off; off += stin_up256(((n + HB - 1) / HB) * 4);
    L.unk = off; off += stin_up256(nu * 4);
    L.inv = off; off += stin_up256(n * 4);
    L.ucol = off; off += stin_up256(e * 4);
    L.urow = off; off += stin_up256(nu * 8);
    L.d = off; off += stin_up256(nu * 8);
    L.x = off; off += stin_up256(vec);
    L.r = off; off += stin_up256(vec);
    L.z = off; off += stin_up256(vec);
    L.q = off; off += stin_up256(vec);
    L.p0 = off; off += stin_up256(vec);
    L.p1 = off; off += stin_up256(vec);
    L.Ppq = off; off += stin_up256(T * PSTRIDE * 8);
    L.Prr = off; off += stin_up256(T * PSTRIDE * 8);
    L.Prz = off; off += stin_up256(T * PSTRIDE * 8);
    L.total = off + 256;
    return L;
}

struct HarmWs {
    HarmArgs a;
    int32_t *bc, *unk, *inv, *ucol;
    double* d;
};

HarmWs harm_ws(const int32_t* rowptr, const double* weight, int64_t N, int64_t E2, int64_t n_U, int C, double tol, void* workspace) {
    const HarmLayout L = harm_layout(N, E2, n_U, C);
    char* w = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    HarmWs h;
    h.bc = reinterpret_cast<int32_t*>(w + L.bc);
    h.unk = reinterpret_cast<int32_t*>(w + L.unk);
    h.inv = reinterpret_cast<int32_t*>(w + L.inv);
    h.ucol = reinterpret_cast<int32_t*>(w + L.ucol);
    h.d = reinterpret_cast<double*>(w + L.d);
    HarmArgs& a = h.a;
    a.rowptr = rowptr;
    a.weight = weight;
    a.unk = h.unk;
    a.ucol = h.ucol;
    a.d = h.d;
    a.urow = reinterpret_cast<int2*>(w + L.urow);
    a.x = reinterpret_cast<double*>(w + L.x);
    a.r = reinterpret_cast<double*>(w + L.r);
    a.z = reinterpret_cast<double*>(w + L.z);
    a.q = reinterpret_cast<double*>(w + L.q);
    a.p[0] = reinterpret_cast<double*>(w + L.p0);
    a.p[1] = reinterpret_cast<double*>(w + L.p1);
    a.Ppq = reinterpret_cast<double*>(w + L.Ppq);
    a.Prr = reinterpret_cast<double*>(w + L.Prr);
    a.Prz = reinterpret_cast<double*>(w + L.Prz);
    a.SA = reinterpret_cast<ChanState*>(w + L.SA);
    a.SB = reinterpret_cast<ChanState*>(w + L.SB);
    a.N = N;
    a.n_U = n_U;
    a.T = (n_U + HB - 1) / HB;
    a.E2 = E2;
    a.tol2 = tol * tol;
    a.C = C;
    return h;
}

// the kernel instance for C channels: the smallest of 1, 2, 3, 4, 8, 16 that holds them
#define HARM_DISPATCH(C_, CALL)          \
    do {                                 \
        if ((C_) <= 1) { CALL(1); }      \
        else if ((C_) == 2) { CALL(2); } \
        else if ((C_) == 3) { CALL(3); } \
        else if ((C_) == 4) { CALL(4); } \
        else if ((C_) <= 8) { CALL(8); } \
        else { CALL(16); }               \
    } while (0)

}  // namespace

extern "C" size_t stin_harmonic_workspace_bytes(int64_t N, int64_t E2, int64_t n_unknown, int C) {
    return harm_sizes_ok(N, E2, n_unknown, C) ? harm_layout(N, E2, n_unknown, C).total : 0;
}

extern "C" int stin_harmonic_reach_u8(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t E2, const uint8_t* masked,
                                      int first_round, int rounds, uint8_t* flag, int64_t* state, stin_stream_t stream_) {
    stin_clear_stale_error();
    hipStream_t stream = (hipStream_t)stream_;
    STIN_REQUIRE(harm_sizes_ok(N, E2, 0, 1), STIN_E_SIZE);
    STIN_REQUIRE(first_round >= 0 && rounds >= 1 && rounds <= MAX_REACH_ROUNDS, STIN_E_SIZE);
    STIN_REQUIRE(state != nullptr, STIN_E_NULL);
    long long* st = reinterpret_cast<long long*>(state);
    hipError_t e;
    if (first_round == 0) {
        e = hipMemsetAsync(state, 0, STIN_HARMONIC_STATE * 8, stream);
        if (e != hipSuccess) return (int)e;
    }
    if (N == 0) return STIN_OK;
    STIN_REQUIRE(rowptr && masked && flag && (E2 == 0 || col), STIN_E_NULL);
    if (first_round == 0) hipLaunchKernelGGL(k_harm_flag_init, dim3(grid_for(N)), dim3(HB), 0, stream, masked, N, flag, st);
    for (int k = 0; k < rounds; ++k) {
        e = hipMemsetAsync(state + 3, 0, 8, stream);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(k_harm_reach, dim3(grid_for(N)), dim3(HB), 0, stream, rowptr, col, N, E2, flag, st);
    }
    return stin_launch_status();
}

extern "C" int stin_harmonic_setup_f64(const int32_t* rowptr, const int32_t* col, const double* weight, int64_t N, int64_t E2,
                                       const float* values, int C, const uint8_t* flag, int64_t n_unknown, int64_t* state,
                                       void* workspace, size_t workspace_bytes, stin_stream_t stream_) {
    stin_clear_stale_error();
    hipStream_t stream = (hipStream_t)stream_;
    STIN_REQUIRE(C >= 1 && C <= MAXC, STIN_E_UNSUPPORTED);
    STIN_REQUIRE(harm_sizes_ok(N, E2, n_unknown, C), STIN_E_SIZE);
    STIN_REQUIRE(state != nullptr && workspace != nullptr, STIN_E_NULL);
    STIN_REQUIRE(workspace_bytes >= stin_harmonic_workspace_bytes(N, E2, n_unknown, C), STIN_E_WORKSPACE);
    STIN_REQUIRE(N == 0 || (rowptr && flag && values && (E2 == 0 || col)), STIN_E_NULL);
    HarmWs h = harm_ws(rowptr, weight, N, E2, n_unknown, C, 0.0, workspace);
    long long* st = reinterpret_cast<long long*>(state);
    if (N > 0) {
        const int64_t nb = (N + HB - 1) / HB;
        hipLaunchKernelGGL(k_harm_count, dim3((unsigned)nb), dim3(HB), 0, stream, flag, N, h.bc);
        hipLaunchKernelGGL(k_harm_scan, dim3(1), dim3(HB), 0, stream, h.bc, nb, n_unknown, st);
        hipLaunchKernelGGL(k_harm_scatter, dim3((unsigned)nb), dim3(HB), 0, stream, flag, N, h.bc, n_unknown, h.unk, h.inv);
    }
    if (h.a.T > 0) {
#define HARM_ROWS(CT) \
    hipLaunchKernelGGL(k_harm_rows<CT>, dim3((unsigned)h.a.T), dim3(HB), 0, stream, h.a, col, values, flag, h.inv, N, h.ucol, h.d, st)
        HARM_DISPATCH(C, HARM_ROWS);
#undef HARM_ROWS
    }
    hipLaunchKernelGGL(k_harm_start, dim3(1), dim3(HB), 0, stream, h.a);
    return stin_launch_status();
}

extern "C" int stin_harmonic_iterate_f64(const double* weight, int64_t N, int64_t E2, int C, int64_t n_unknown, double tol,
                                         int first_iteration, int count, int64_t* state, void* workspace, size_t workspace_bytes,
                                         stin_stream_t stream_) {
    stin_clear_stale_error();
    hipStream_t stream = (hipStream_t)stream_;
    STIN_REQUIRE(C >= 1 && C <= MAXC, STIN_E_UNSUPPORTED);
    STIN_REQUIRE(harm_sizes_ok(N, E2, n_unknown, C), STIN_E_SIZE);
    STIN_REQUIRE(count >= 1 && count <= MAX_ITER_PER_CALL && first_iteration >= 0 && first_iteration <= INT32_MAX - MAX_ITER_PER_CALL,
                 STIN_E_SIZE);
    STIN_REQUIRE(tol >= 0.0, STIN_E_SIZE);                                        // (a NaN fails here)
    STIN_REQUIRE(state != nullptr && workspace != nullptr, STIN_E_NULL);
    STIN_REQUIRE(workspace_bytes >= stin_harmonic_workspace_bytes(N, E2, n_unknown, C), STIN_E_WORKSPACE);
    const HarmWs h = harm_ws(nullptr, weight, N, E2, n_unknown, C, tol, workspace);
    if (h.a.T > 0) {
        const dim3 grid((unsigned)h.a.T), block(HB);
        for (int j = 0; j < count; ++j) {
            const int k = first_iteration + j;
#define HARM_ITER(CT)                                                              \
    hipLaunchKernelGGL(k_harm_product<CT>, grid, block, 0, stream, h.a, k);        \
    hipLaunchKernelGGL(k_harm_update<CT>, grid, block, 0, stream, h.a, k)
            HARM_DISPATCH(C, HARM_ITER);
#undef HARM_ITER
        }
    }
    hipLaunchKernelGGL(k_harm_report, dim3(1), dim3(HB), 0, stream, h.a, reinterpret_cast<long long*>(state), 0);
    return stin_launch_status();
}

extern "C" int stin_harmonic_finish_f32(const float* values, const uint8_t* flag, int64_t N, int64_t E2, int C, int64_t n_unknown,
                                        double tol, float fill, float* out, int64_t* state, void* workspace, size_t workspace_bytes,
                                        stin_stream_t stream_) {
    stin_clear_stale_error();
    hipStream_t stream = (hipStream_t)stream_;
    STIN_REQUIRE(C >= 1 && C <= MAXC, STIN_E_UNSUPPORTED);
    STIN_REQUIRE(harm_sizes_ok(N, E2, n_unknown, C), STIN_E_SIZE);
    STIN_REQUIRE(tol >= 0.0, STIN_E_SIZE);
    STIN_REQUIRE(state != nullptr && workspace != nullptr, STIN_E_NULL);
    STIN_REQUIRE(workspace_bytes >= stin_harmonic_workspace_bytes(N, E2, n_unknown, C), STIN_E_WORKSPACE);
    STIN_REQUIRE(N == 0 || (values && flag && out), STIN_E_NULL);
    const HarmWs h = harm_ws(nullptr, nullptr, N, E2, n_unknown, C, tol, workspace);
    hipLaunchKernelGGL(k_harm_report, dim3(1), dim3(HB), 0, stream, h.a, reinterpret_cast<long long*>(state), 1);
    const int64_t NC = N * C;
    if (NC > 0)
        hipLaunchKernelGGL(k_harm_out, dim3(grid_for(NC)), dim3(HB), 0, stream, values, flag, h.inv, h.a.x, NC, C, n_unknown, fill, out);
    return stin_launch_status();
}
