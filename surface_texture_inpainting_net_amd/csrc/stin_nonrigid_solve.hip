// The linear solve of the non-rigid colour-map optimisation on the device: one banded-arrow Cholesky per pose, for
// preprocessing.nonrigid_solve / optimize_poses_nonrigid(solver='banded').  Contract: include/stin_hip.h ("Non-rigid solve");
// tests/_nonrigid_solve_oracle.py restates it in numpy, dense and left-looking, and agrees byte for byte.
//
// The system of a pose has n = m + 6 unknowns, m = 2 Ah Aw anchor offsets in which only neighbouring anchors couple (half bandwidth
// w = 2 Aw + 3) and a border of the pose's six.  With the pose LAST the Cholesky factor keeps the band: m (w + 1) + 7 n stored
// numbers instead of n^2, about m w^2 multiply-adds instead of n^3 / 3.
//
//   stats:     one workgroup per pose: pairs (integer sum of the counts), residual (cells ascending from +0.0, by one thread over
//              values the workgroup stages 256 at a time), FEW_PAIRS, whether the pose is solved, wgt^2; an unsolved pose's x row.
//   assemble:  a GATHER - one thread per stored entry of the band [B][m][w + 1] (row i, column c holds M[i][i - w + c]) and of the
//              border [B][7][n] (rows 0 .. 5: the pose's rows of M over all columns; row 6: r = -b).  An anchor entry adds the at
//              most four cells that hold both its anchors, ascending; a pose entry adds all cells.  No atomics: the sums are the
//              host assembly's, bit for bit.
//   factor:    one workgroup of 256 threads per pose, RIGHT-looking, in place.  LDS holds a window of the w + 1 band rows k .. k + w
//              (circular in the row), the 7 border rows over the same columns (circular in the column), the 7 x 6 border-border
//              block and the scaled pivot column: ((w + 1)(w + 8) + 42 + w + 7) doubles - 19.8 KB at Aw = 21, 63.5 KB at Aw = 41,
//              the widest lattice (64 KB of LDS per workgroup without raising any limit).  Per pivot: every thread takes sqrt of the
//              pivot itself (no broadcast), w + 7 threads scale the column into LDS and write it through to memory, a barrier, the
//              threads share the w (w + 1) / 2 + 7 w + 27 entries of the rank-1 update (each thread's entries are fixed RELATIVE to
//              the window, decoded once), the next band row and border column slide in, a barrier.  The right-hand side is border
//              row 6, so forward substitution is part of the factorisation.  The 6 x 6 border is then factored and solved by every
//              thread in registers (42 doubles; no broadcast, and every thread knows whether a pivot failed).  Back substitution is
//              a column sweep: the border's six first, one thread per anchor unknown; then the band, descending, through a ring of
//              w + 2 partial sums in LDS, one barrier per unknown, the factor's rows read one step ahead.
// An entry receives its subtractions in ascending pivot order, as in the left-looking statement of the contract.  No loop bound
// and no barrier depends on a data value: a pivot that is not > 0 only sets a flag, the arithmetic runs on, and the flag (or a
// non-finite x) turns the pose's x row into +0.0 at the end.  Nothing is contracted (-ffp-contract=off), division and sqrt are
// the IEEE operations, there is no reciprocal.
#include "stin_common.h"

namespace {

constexpr int TB = 256;                                   // threads per workgroup, all three kernels
constexpr int LOCAL = STIN_NONRIGID_LOCAL;
constexpr int BLOCK = STIN_NONRIGID_BLOCK_DOUBLES;
constexpr int MAX_AW = STIN_NONRIGID_SOLVE_MAX_AW;
constexpr int MAX_W = 2 * MAX_AW + 3;
constexpr int BORDER = 7;                                 // the pose's six rows and the right-hand side
constexpr int BB = 27;                                    // border-border entries: the 6 x 6 triangle and 6 of the right-hand side
// entries of one rank-1 update, as enumerated below, over the threads of a workgroup, at the widest band
constexpr int SLOTS = (((MAX_W + 1) / 2) * (MAX_W + 1) + BORDER * MAX_W + BB + TB - 1) / TB;
constexpr unsigned NO_ENTRY = 0xffffu;
static_assert(((MAX_W + 1) * (MAX_W + 8) + 6 * BORDER + MAX_W + BORDER) * 8 <= 65536, "the window fits 64 KB of LDS");
static_assert(MAX_W + BORDER + 1 <= TB && MAX_W + BORDER < 256, "one thread per entry of a pivot column; an entry code is two bytes");

struct SolveArgs {
    const double* blocks;                                 // [B][cells][120]
    const int32_t* counts;                                // [B][cells]
    const double* flow;                                   // [B][Ah][Aw][2]
    const uint8_t* valid;
    const uint8_t* free_;
    double* x;                                            // [B][n]
    double* residual;
    int64_t* pairs;
    int32_t* status;
    double* w2;                                           // workspace: [B] wgt^2
    int32_t* go;                                          // workspace: [B] 1 = this pose is solved
    double* band;                                         // workspace: [B][m][w + 1]
    double* border;                                       // workspace: [B][7][n]
    int64_t cells, n_vertices, min_pairs;
    double anchor_weight;
    int B, Ah, Aw, m, n, w;
};

// --------------------------------------------------------------------------------------------------------------------- stats
__global__ __launch_bounds__(TB) void k_solve_stats(const SolveArgs A) {
    __shared__ double sr[TB];
    __shared__ long long sc[TB];
    const int p = blockIdx.x, t = threadIdx.x;
    const double* blk = A.blocks + (int64_t)p * A.cells * BLOCK;
    const int32_t* cnt = A.counts + (int64_t)p * A.cells;
    long long c = 0;
    for (int64_t i = t; i < A.cells; i += TB) c += cnt[i];
    sc[t] = c;
    double e = 0.0;                                       // thread 0's: r r over the cells ascending
    for (int64_t base = 0; base < A.cells; base += TB) {
        if (base + t < A.cells) sr[t] = blk[(base + t) * BLOCK + (BLOCK - 1)];
        __syncthreads();
        if (t == 0) {
            const int k1 = A.cells - base < TB ? (int)(A.cells - base) : TB;
            for (int k = 0; k < k1; ++k) e = e + sr[k];
        }
        __syncthreads();
    }
    for (int s = TB / 2; s > 0; s >>= 1) {
        if (t < s) sc[t] += sc[t + s];
        __syncthreads();
    }
    const long long n_p = sc[0];
    const bool open = A.free_[p] != 0 && A.valid[p] != 0;
    const bool go = open && n_p >= A.min_pairs;
    if (!go)
        for (int j = t; j < A.n; j += TB) A.x[(int64_t)p * A.n + j] = 0.0;
    if (t == 0) {
        const double wgt = (A.anchor_weight * (double)n_p) / (double)A.n_vertices;
        A.pairs[p] = n_p;
        A.residual[p] = e;
        A.status[p] = open && !go ? STIN_NONRIGID_FEW_PAIRS : 0;
        A.go[p] = go ? 1 : 0;
        A.w2[p] = wgt * wgt;
    }
}

// ------------------------------------------------------------------------------------------------------------------ assemble
// Index of (a, b), a <= b, in the row-major upper triangle of the 14 x 14.
__device__ inline int tri(int a, int b) { return a * LOCAL - a * (a - 1) / 2 + (b - a); }

// The local unknown of anchor unknown u (0 .. m - 1) in cell (cr, cc), which holds its anchor.
__device__ inline int local_of(int u, int ar, int ac, int cr, int cc) { return 6 + 2 * ((ar - cr) * 2 + (ac - cc)) + (u & 1); }

// Sum over the cells that hold the anchors of BOTH anchor unknowns ua <= ub, ascending, from +0.0: A[6 + ua][6 + ub].
__device__ inline double gather_pair(const double* __restrict__ blk, int Ah, int Aw, int ua, int ub) {
    const int a = ua >> 1, b = ub >> 1;
    const int ar = a / Aw, ac = a % Aw, br = b / Aw, bc = b % Aw;
    int r0 = (ar > br ? ar : br) - 1, r1 = ar < br ? ar : br, c0 = (ac > bc ? ac : bc) - 1, c1 = ac < bc ? ac : bc;
    r0 = r0 < 0 ? 0 : r0;
    c0 = c0 < 0 ? 0 : c0;
    r1 = r1 > Ah - 2 ? Ah - 2 : r1;
    c1 = c1 > Aw - 2 ? Aw - 2 : c1;
    double acc = 0.0;
    for (int cr = r0; cr <= r1; ++cr)
        for (int cc = c0; cc <= c1; ++cc)
            acc = acc + blk[((int64_t)cr * (Aw - 1) + cc) * BLOCK + tri(local_of(ua, ar, ac, cr, cc), local_of(ub, br, bc, cr, cc))];
    return acc;
}

// Sum over the cells that hold the anchor of unknown u, ascending: row >= 0: A[row][6 + u], row < 0: b[6 + u].
__device__ inline double gather_one(const double* __restrict__ blk, int Ah, int Aw, int row, int u) {
    const int a = u >> 1, ar = a / Aw, ac = a % Aw;
    const int r0 = ar - 1 < 0 ? 0 : ar - 1, r1 = ar > Ah - 2 ? Ah - 2 : ar, c0 = ac - 1 < 0 ? 0 : ac - 1, c1 = ac > Aw - 2 ? Aw - 2 : ac;
    double acc = 0.0;
    for (int cr = r0; cr <= r1; ++cr)
        for (int cc = c0; cc <= c1; ++cc) {
            const int l = local_of(u, ar, ac, cr, cc);
            acc = acc + blk[((int64_t)cr * (Aw - 1) + cc) * BLOCK + (row >= 0 ? tri(row, l) : BLOCK - LOCAL - 1 + l)];
        }
    return acc;
}

// Entry `entry` of every cell, ascending.
__device__ inline double gather_all(const double* __restrict__ blk, int64_t cells, int entry) {
    double acc = 0.0;
#pragma unroll 8
    for (int64_t c = 0; c < cells; ++c) acc = acc + blk[c * BLOCK + entry];
    return acc;
}

__global__ __launch_bounds__(TB) void k_solve_assemble(const SolveArgs A) {
    const int p = blockIdx.y;
    if (!A.go[p]) return;
    const int W1 = A.w + 1;
    const int64_t e = (int64_t)blockIdx.x * TB + threadIdx.x, in_band = (int64_t)A.m * W1;
    if (e >= in_band + (int64_t)BORDER * A.n) return;
    const double* blk = A.blocks + (int64_t)p * A.cells * BLOCK;
    const double w2 = A.w2[p];
    if (e < in_band) {                                    // M[i][j], j = i - w + c <= i, both anchor unknowns
        const int i = (int)(e / W1), c = (int)(e % W1), j = i - A.w + c;
        double v = 0.0;
        if (j >= 0) {
            v = gather_pair(blk, A.Ah, A.Aw, j, i);
            if (j == i) v = v + w2;
        }
        A.band[(int64_t)p * in_band + e] = v;
        return;
    }
    const int r = (int)((e - in_band) / A.n), j = (int)((e - in_band) % A.n);
    double v = 0.0;
    if (r < 6) {                                          // the pose's row r of M: M[m + r][j], j <= m + r
        if (j < A.m) v = gather_one(blk, A.Ah, A.Aw, r, j);
        else if (j - A.m <= r) v = gather_all(blk, A.cells, tri(j - A.m, r));
    } else {                                              // r = -b
        if (j < A.m) {
            v = gather_one(blk, A.Ah, A.Aw, -1, j);
            v = v + w2 * A.flow[(int64_t)p * A.m + j];
        } else {
            v = gather_all(blk, A.cells, BLOCK - LOCAL - 1 + (j - A.m));
        }
        v = -v;
    }
    A.border[(int64_t)p * BORDER * A.n + (e - in_band)] = v;
}

// -------------------------------------------------------------------------------------------------------------------- factor
// Entry e of a rank-1 update -> (row c << 8 | column dj) RELATIVE to the pivot k, or NO_ENTRY.  Rows: c < w: band row k + 1 + c;
// c = w + r: border row r.  Columns: dj < w: column k + 1 + dj; dj = w + s: border column s.  The band's triangle dj <= c is
// enumerated as (w + 1) / 2 rows of w + 1: row pr holds triangle row pr (pr + 1 entries) and triangle row w - 1 - pr (w - pr).
__device__ inline unsigned entry_of(int e, int w) {
    const int W1 = w + 1, half = W1 / 2;                  // w is odd
    if (e < half * W1) {
        const int pr = e / W1, q = e % W1;
        if (q <= pr) return (unsigned)(pr << 8 | q);
        if (w - 1 - pr == pr) return NO_ENTRY;
        return (unsigned)((w - 1 - pr) << 8 | (q - pr - 1));
    }
    e -= half * W1;
    if (e < BORDER * w) return (unsigned)((w + e / w) << 8 | (e % w));
    e -= BORDER * w;
    if (e >= BB) return NO_ENTRY;
    if (e >= 21) return (unsigned)((w + 6) << 8 | (w + e - 21));
    int r = 0;
    while (e > r) {
        e -= r + 1;
        ++r;
    }
    return (unsigned)((w + r) << 8 | (w + e));
}

__global__ __launch_bounds__(TB) void k_solve_factor(const SolveArgs A) {
    extern __shared__ double lds[];
    const int p = blockIdx.x, t = threadIdx.x;
    if (!A.go[p]) return;                                 // the whole workgroup, before any barrier
    const int w = A.w, W1 = w + 1, m = A.m, n = A.n;
    double* Wn = lds;                                     // [W1][W1]: band row i in slot i mod W1, column j at j - i + w
    double* Bw = Wn + W1 * W1;                            // [7][W1]: border row r, column j in slot j mod W1
    double* Bb = Bw + BORDER * W1;                        // [7][6]: border row r, border column s
    double* colk = Bb + BORDER * 6;                       // [w + 7]: column k of L: band rows k + 1 .. k + w, then the border's
    double* Lb = A.band + (int64_t)p * m * W1;
    double* Br = A.border + (int64_t)p * BORDER * n;
    double* xp = A.x + (int64_t)p * n;

    unsigned tab[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) tab[s] = entry_of(t + s * TB, w);
    for (int e = t; e < W1 * W1; e += TB)
        if (e / W1 < m) Wn[e] = Lb[e];
    for (int e = t; e < BORDER * W1; e += TB)
        if (e % W1 < m) Bw[e] = Br[(int64_t)(e / W1) * n + e % W1];
    if (t < BORDER * 6) Bb[t] = Br[(int64_t)(t / 6) * n + m + t % 6];
    __syncthreads();

    bool bad = false;
    int ks = 0, kn = 1;                                   // k mod W1, (k + 1) mod W1
    for (int k = 0; k < m; ++k) {
        const int lim = m - 1 - k;                        // band rows below the pivot
        const int in = k + W1;                            // the band row and border column that slide in
        const bool has = in < m && t < W1 + BORDER;
        double pre = 0.0;
        if (has) pre = t < W1 ? Lb[(int64_t)in * W1 + t] : Br[(int64_t)(t - W1) * n + in];
        const double piv = Wn[ks * W1 + w];
        bad = bad || !(piv > 0.0);
        const double d = sqrt(piv);
        if (t < w) {
            if (t < lim) {
                const int slot = kn + t < W1 ? kn + t : kn + t - W1;
                const double l = Wn[slot * W1 + (w - 1 - t)] / d;
                colk[t] = l;
                Lb[(int64_t)(k + 1 + t) * W1 + (w - 1 - t)] = l;
            }
        } else if (t < w + BORDER) {
            const double l = Bw[(t - w) * W1 + ks] / d;
            colk[t] = l;
            Br[(int64_t)(t - w) * n + k] = l;
        } else if (t == w + BORDER) {
            Lb[(int64_t)k * W1 + w] = d;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const unsigned code = tab[s];
            if (code == NO_ENTRY) continue;
            const int c = (int)(code >> 8), dj = (int)(code & 255u);
            double* target;
            if (c < w) {
                if (c >= lim) continue;
                const int slot = kn + c < W1 ? kn + c : kn + c - W1;
                target = Wn + slot * W1 + (dj - c + w);
            } else if (dj < w) {
                if (dj >= lim) continue;
                target = Bw + (c - w) * W1 + (kn + dj < W1 ? kn + dj : kn + dj - W1);
            } else {
                target = Bb + (c - w) * 6 + (dj - w);
            }
            *target = *target - colk[c] * colk[dj];
        }
        if (has) {
            if (t < W1) Wn[ks * W1 + t] = pre;
            else Bw[(t - W1) * W1 + ks] = pre;
        }
        __syncthreads();
        ks = kn;
        kn = kn + 1 < W1 ? kn + 1 : 0;
    }

    // the border: its 6 x 6 and the right-hand side's six, by every thread for itself
    double g[BORDER][6];
#pragma unroll
    for (int r = 0; r < BORDER; ++r)
#pragma unroll
        for (int s = 0; s < 6; ++s) g[r][s] = Bb[r * 6 + s];
#pragma unroll
    for (int r = 0; r < BORDER; ++r)
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            if (s > r) continue;
            double v = g[r][s];
#pragma unroll
            for (int q = 0; q < s; ++q) v = v - g[r][q] * g[s][q];
            if (s < r) {
                g[r][s] = v / g[s][s];
            } else {
                bad = bad || !(v > 0.0);
                g[r][s] = sqrt(v);
            }
            if (t == 0) Br[(int64_t)r * n + m + s] = g[r][s];
        }
    double xb[6];
    bool fin = true;
#pragma unroll
    for (int k = 5; k >= 0; --k) {
        double v = g[6][k];
#pragma unroll
        for (int q = 5; q > k; --q) v = v - g[q][k] * xb[q];
        xb[k] = v / g[k][k];
        fin = fin && isfinite(xb[k]);
        if (t == 0) xp[k] = xb[k];
    }
    // back substitution, the border's six columns first: y_i - L[n - 1][i] x_(n - 1) - .. - L[m][i] x_m, kept in border row 6
    for (int i = t; i < m; i += TB) {
        double v = Br[(int64_t)6 * n + i];
#pragma unroll
        for (int r = 5; r >= 0; --r) v = v - Br[(int64_t)r * n + i] * xb[r];
        Br[(int64_t)6 * n + i] = v;
    }
    __syncthreads();
    // the band, descending: a ring of w + 2 partial sums; slot of unknown i: i mod (w + 2)
    const int R2 = w + 2;
    double* T = lds;
    for (int i = m - W1 + t; i < m; i += TB)
        if (i >= 0) T[i % R2] = Br[(int64_t)6 * n + i];
    __syncthreads();
    ks = (m - 1) % R2;
    double lrow = 0.0, diag = Lb[(int64_t)(m - 1) * W1 + w], tin = 0.0;
    if (t < w) lrow = Lb[(int64_t)(m - 1) * W1 + t];
    if (t == w + 1 && m - 1 - W1 >= 0) tin = Br[(int64_t)6 * n + (m - 1 - W1)];
    for (int k = m - 1; k >= 0; --k) {
        const double lrow_k = lrow, diag_k = diag, tin_k = tin;
        if (k > 0) {                                      // the next step's operands, one step ahead
            diag = Lb[(int64_t)(k - 1) * W1 + w];
            if (t < w) lrow = Lb[(int64_t)(k - 1) * W1 + t];
            if (t == w + 1 && k - 1 - W1 >= 0) tin = Br[(int64_t)6 * n + (k - 1 - W1)];
        }
        const double xk = T[ks] / diag_k;
        fin = fin && isfinite(xk);
        if (t < w) {
            if (k - w + t >= 0) {                         // unknown i = k - w + t
                const int si = ks - (w - t) < 0 ? ks - (w - t) + R2 : ks - (w - t);
                T[si] = T[si] - lrow_k * xk;
            }
        } else if (t == w) {
            xp[6 + k] = xk;
        } else if (t == w + 1) {
            if (k - W1 >= 0) T[ks + 1 < R2 ? ks + 1 : 0] = tin_k;      // unknown k - w - 1 enters where k + 1 was
        }
        __syncthreads();
        ks = ks > 0 ? ks - 1 : R2 - 1;
    }
    if (bad || !fin) {
        for (int j = t; j < n; j += TB) xp[j] = 0.0;
        if (t == 0) A.status[p] = STIN_NONRIGID_SINGULAR;
    }
}

inline bool lattice_ok(int B, int Ah, int Aw) {
    return B >= 0 && B <= STIN_NONRIGID_SOLVE_MAX_BATCH && Ah >= 2 && Aw >= 2 && Aw <= MAX_AW && (int64_t)Ah * Aw < (int64_t)(1 << 22);
}

struct Layout {
    size_t w2, go, band, border, total;
};

inline Layout layout_of(int B, int Ah, int Aw) {
    const size_t b = (size_t)(B > 0 ? B : 1), m = (size_t)2 * Ah * Aw, n = m + 6, W1 = (size_t)2 * Aw + 4;
    Layout L;
    L.w2 = 0;
    L.go = L.w2 + stin_up256(b * sizeof(double));
    L.band = L.go + stin_up256(b * sizeof(int32_t));
    L.border = L.band + stin_up256(b * m * W1 * sizeof(double));
    L.total = L.border + stin_up256(b * BORDER * n * sizeof(double));
    return L;
}

}  // namespace

extern "C" size_t stin_nonrigid_solve_workspace_bytes(int B, int Ah, int Aw) {
    if (!lattice_ok(B, Ah, Aw)) return 0;
    return layout_of(B, Ah, Aw).total;
}

extern "C" int stin_nonrigid_solve_stages_f64(const double* blocks, const int32_t* counts, const double* flow, const uint8_t* valid,
                                              const uint8_t* free_, int B, int Ah, int Aw, int64_t n_vertices, double anchor_weight,
                                              int64_t min_pairs, double* x, double* residual, int64_t* pairs, int32_t* status,
                                              void* workspace, size_t workspace_bytes, int stages, stin_stream_t stream_) {
    STIN_REQUIRE(lattice_ok(B, Ah, Aw), STIN_E_SIZE);
    STIN_REQUIRE(stages >= 0 && stages <= (STIN_NONRIGID_SOLVE_STAGE_STATS | STIN_NONRIGID_SOLVE_STAGE_ASSEMBLE | STIN_NONRIGID_SOLVE_STAGE_FACTOR),
                 STIN_E_SIZE);
    if (B == 0) return STIN_OK;
    STIN_REQUIRE(blocks && counts && flow && valid && free_ && x && residual && pairs && status, STIN_E_NULL);
    const Layout L = layout_of(B, Ah, Aw);
    STIN_REQUIRE(workspace != nullptr && workspace_bytes >= L.total, STIN_E_WORKSPACE);
    STIN_REQUIRE(((uintptr_t)workspace & 7u) == 0, STIN_E_SIZE);
    SolveArgs A;
    A.blocks = blocks; A.counts = counts; A.flow = flow; A.valid = valid; A.free_ = free_;
    A.x = x; A.residual = residual; A.pairs = pairs; A.status = status;
    char* ws = (char*)workspace;
    A.w2 = (double*)(ws + L.w2); A.go = (int32_t*)(ws + L.go); A.band = (double*)(ws + L.band); A.border = (double*)(ws + L.border);
    A.cells = (int64_t)(Ah - 1) * (Aw - 1); A.n_vertices = n_vertices; A.min_pairs = min_pairs; A.anchor_weight = anchor_weight;
    A.B = B; A.Ah = Ah; A.Aw = Aw; A.m = 2 * Ah * Aw; A.n = A.m + 6; A.w = 2 * Aw + 3;
    const int W1 = A.w + 1;
    const int64_t entries = (int64_t)A.m * W1 + (int64_t)BORDER * A.n;
    const size_t lds = (size_t)(W1 * (W1 + BORDER) + BORDER * 6 + A.w + BORDER) * sizeof(double);
    hipStream_t stream = (hipStream_t)stream_;
    stin_clear_stale_error();
    if (stages == 0 || (stages & STIN_NONRIGID_SOLVE_STAGE_STATS)) hipLaunchKernelGGL(k_solve_stats, dim3((unsigned)B), dim3(TB), 0, stream, A);
    if (stages == 0 || (stages & STIN_NONRIGID_SOLVE_STAGE_ASSEMBLE))
        hipLaunchKernelGGL(k_solve_assemble, dim3((unsigned)((entries + TB - 1) / TB), (unsigned)B), dim3(TB), 0, stream, A);
    if (stages == 0 || (stages & STIN_NONRIGID_SOLVE_STAGE_FACTOR)) hipLaunchKernelGGL(k_solve_factor, dim3((unsigned)B), dim3(TB), lds, stream, A);
    return stin_launch_status();
}

extern "C" int stin_nonrigid_solve_f64(const double* blocks, const int32_t* counts, const double* flow, const uint8_t* valid,
                                       const uint8_t* free_, int B, int Ah, int Aw, int64_t n_vertices, double anchor_weight,
                                       int64_t min_pairs, double* x, double* residual, int64_t* pairs, int32_t* status, void* workspace,
                                       size_t workspace_bytes, stin_stream_t stream_) {
    return stin_nonrigid_solve_stages_f64(blocks, counts, flow, valid, free_, B, Ah, Aw, n_vertices, anchor_weight, min_pairs, x, residual,
                                          pairs, status, workspace, workspace_bytes, 0, stream_);
}
