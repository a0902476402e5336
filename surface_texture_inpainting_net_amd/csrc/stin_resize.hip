// Image resize on uint8 [H, W, C] images (include/stin_hip.h, "Image resize"): what the reference asks cv2.resize for - colour frames
// to the depth size (preprocessing/texture_map_optimization.py:93) and Rescale of the 2-D experiment
// (datasets/imagegraph_dataloader.py:215) - as ONE launch over a table of jobs:
//
//   stin_resize_u8   STIN_RESIZE_LINEAR (11-bit bilinear, half-pixel centres) or STIN_RESIZE_AREA (exact area average) of J images
//                    that lie at any byte offsets of one source buffer, into any byte offsets of one destination buffer.
//
// Both modes are a weighted sum of source rows, each a weighted sum of source columns, with one rounding at the end:
//   LINEAR  rows (sy, 2048 - by), (sy', by);  columns (sx, 2048 - bx), (sx', bx);        32-bit sums
//   AREA    rows [y0, y0 + ny) with the overlaps oy; columns [x0, x0 + nx) with ox;      32-bit row sums, 64-bit totals
// A block owns a tile of TH output rows x TB output columns, one thread per column with the TH x C sums of its column in registers.
// The thread forms its column's taps / overlaps once per tile (registers), threads 0 .. TH-1 form the rows' (LDS).  The tile's source
// rows [first row of its first output row, last row of its last) are staged through LDS as many at a time as fit into STAGE bytes -
// the whole tile at the frame shape, 17 rows of 1.6 KB - with aligned 16-byte loads, up to eight per thread in flight before the
// first is written to LDS: it is the bytes in flight per CU that hide the memory latency of a streaming kernel.  A row of 3 W bytes
// starts anywhere: its segment is staged from the 16-byte boundary below it; the bytes of a piece that straddles an end of the source
// buffer are read one by one.  A row segment longer than STAGE is staged in chunks of STAGE bytes, a pixel may straddle two chunks,
// and nothing assumes that a footprint fits: 2000 rows to 3 is a longer loop.  Where all rows of the tile are staged at once (the
// two users' shapes), every output row walks its own source rows; else every staged row adds wy * (its column sum) to the output
// rows it overlaps (block-uniform weights) - the same integer sums in another order.  The TH result rows go to LDS, each at its
// destination's own phase (mod 16), and leave as aligned 16-byte stores, ragged ends byte by byte.
// LINEAR reads every row and column between the taps of a tile: reducing by more than two reads what it then skips.
//
// The job table lives on the device and the host never reads it, so the grid is fixed and the blocks share the tiles of all jobs
// round-robin: block b takes tiles b, b + G, ... of the concatenated tile list and walks the table forward as it goes.  A job that
// fails the checks of the header has no tiles.
//
// Plain C++ loads and stores only; no float, no atomics.
#include "stin_common.h"

#include <type_traits>

namespace {
constexpr int TB = 256;                    // threads per block = output columns of a tile
constexpr int TH = 8;                      // output rows of a tile
constexpr int STAGE = 32768;               // bytes of staged source rows
constexpr int LOADS = STAGE / 16 / TB;     // 16-byte loads per thread and step (8)
constexpr int OUT_PITCH = 16 + TB * 4 + 16;  // bytes of a result row in LDS: phase + the widest row + the last piece's tail
constexpr int OUT_PIECES = OUT_PITCH / 16;
constexpr int GRID = 256 * 3;              // 41 KB of LDS: three blocks per CU
constexpr int JW = STIN_RESIZE_JOB_WORDS;
constexpr int MAX_SIDE = STIN_RESIZE_MAX_SIDE;

struct Job {
    int64_t src_off, dst_off;
    int H, W, h, w;
    int64_t tiles;                         // 0: the job is not served
};

// One axis entry.  LINEAR: taps s and q, the second with weight p (the first 2048 - p), n = 2.  AREA: source indices [s, s + n), each
// with weight n_out, less p at the first and q at the last (the parts of those pixels outside the cell).
struct Axis {
    int s, n, p, q;
};

template <int MODE> __device__ __forceinline__ Axis axis(int d, int n_in, int n_out) {
    Axis a;
    if (MODE == STIN_RESIZE_LINEAR) {
        const int num = (2 * d + 1) * n_in - n_out, den = 2 * n_out;        // |num| < 2^30: sides <= 2^14
        int s = num >= 0 ? num / den : -((den - 1 - num) / den);
        const int r = num - s * den;
        int b = (4096 * r + den) / (2 * den);                               // r < den <= 2^15
        if (s < 0) { s = 0; b = 0; }
        if (s >= n_in - 1) { s = n_in - 1; b = 0; }
        a.s = s;
        a.n = 2;
        a.p = b;
        a.q = min(s + 1, n_in - 1);
    } else {
        const int lo = d * n_in, hi = lo + n_in;                            // the cell, in units of 1 / n_out of a source pixel
        a.s = lo / n_out;
        const int end = (hi + n_out - 1) / n_out;
        a.n = end - a.s;
        a.p = lo - a.s * n_out;
        a.q = end * n_out - hi;
    }
    return a;
}

// weight of tap t of an entry (columns: the thread walks its own taps)
template <int MODE> __device__ __forceinline__ unsigned tap_weight(const Axis& a, int t, int n_out) {
    if (MODE == STIN_RESIZE_LINEAR) return t == 0 ? 2048u - (unsigned)a.p : (unsigned)a.p;
    return (unsigned)(n_out - (t == 0 ? a.p : 0) - (t == a.n - 1 ? a.q : 0));
}
template <int MODE> __device__ __forceinline__ int tap_index(const Axis& a, int t) {
    if (MODE == STIN_RESIZE_LINEAR) return t == 0 ? a.s : a.q;
    return a.s + t;
}
// weight of source index r in an entry, 0 when the entry does not touch it (rows: the block walks the source rows)
template <int MODE> __device__ __forceinline__ unsigned index_weight(const Axis& a, int r, int n_out) {
    if (MODE == STIN_RESIZE_LINEAR) return (r == a.s ? 2048u - (unsigned)a.p : 0u) + (r == a.q ? (unsigned)a.p : 0u);   // (s == q: p = 0)
    const int t = r - a.s;
    return t >= 0 && t < a.n ? (unsigned)(n_out - (t == 0 ? a.p : 0) - (t == a.n - 1 ? a.q : 0)) : 0u;
}

template <int MODE>
__device__ __forceinline__ Job load_job(const int64_t* __restrict__ jobs, int j, int64_t src_bytes, int64_t dst_bytes, int C) {
    const int64_t* __restrict__ q = jobs + (int64_t)j * JW;
    const int64_t so = q[0], H = q[1], W = q[2], dof = q[3], h = q[4], w = q[5];
    bool ok = H >= 1 && H <= MAX_SIDE && W >= 1 && W <= MAX_SIDE && h >= 1 && h <= MAX_SIDE && w >= 1 && w <= MAX_SIDE;
    ok = ok && so >= 0 && dof >= 0;
    if (ok) ok = H * W * C <= src_bytes - so && h * w * C <= dst_bytes - dof;           // (sides checked: no overflow)
    if (ok && MODE == STIN_RESIZE_AREA) ok = h <= H && w <= W;
    Job jb;
    jb.src_off = so;
    jb.dst_off = dof;
    jb.H = (int)H;
    jb.W = (int)W;
    jb.h = (int)h;
    jb.w = (int)w;
    jb.tiles = ok ? ((h + TH - 1) / TH) * ((w + TB - 1) / TB) : 0;
    return jb;
}

// 16 bytes at byte g of src, g a multiple of 16 away from an aligned address; bytes outside [0, src_bytes) are not read (0)
__device__ __forceinline__ uint4 load_piece(const uint8_t* __restrict__ src, int64_t src_bytes, int64_t g) {
    if (g >= 0 && g + 16 <= src_bytes) return *reinterpret_cast<const uint4*>(src + g);
    unsigned wds[4] = {0u, 0u, 0u, 0u};                                     // the buffer's own ragged ends
    for (int e = 0; e < 16; ++e) {
        const int64_t gg = g + e;
        if (gg >= 0 && gg < src_bytes) wds[e >> 2] |= (unsigned)src[gg] << (8 * (e & 3));
    }
    return make_uint4(wds[0], wds[1], wds[2], wds[3]);
}

template <int MODE, int C>
__global__ __launch_bounds__(TB, 3) void k_resize(const uint8_t* __restrict__ src, int64_t src_bytes, uint8_t* __restrict__ dst,
                                               int64_t dst_bytes, const int64_t* __restrict__ jobs, int J) {
    typedef typename std::conditional<MODE == STIN_RESIZE_LINEAR, unsigned, unsigned long long>::type acc_t;
    __shared__ __attribute__((aligned(16))) uint8_t stage[STAGE];
    __shared__ __attribute__((aligned(16))) uint8_t outbuf[TH * OUT_PITCH];
    __shared__ Axis rowtab[TH];
    const int tid = threadIdx.x;
    const uintptr_t src_addr = reinterpret_cast<uintptr_t>(src), dst_addr = reinterpret_cast<uintptr_t>(dst);
    int j = 0;
    int64_t first_tile = 0;                                                 // of job j in the concatenated list
    bool loaded = false;
    Job jb;
    for (int64_t t = blockIdx.x;; t += gridDim.x) {
        while (j < J) {
            if (!loaded) {
                jb = load_job<MODE>(jobs, j, src_bytes, dst_bytes, C);
                loaded = true;
            }
            if (t < first_tile + jb.tiles) break;
            first_tile += jb.tiles;
            ++j;
            loaded = false;
        }
        if (j >= J) break;
        const int tiles_x = (jb.w + TB - 1) / TB;
        const int tile = (int)(t - first_tile);                             // < 2^17: sides <= 2^14
        const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const int x_first = tx * TB, ncol = min(TB, jb.w - x_first), nrow = min(TH, jb.h - ty * TH);
        const bool active = tid < ncol;
        const Axis cx = axis<MODE>(x_first + (active ? tid : 0), jb.W, jb.w);
        // the tile's span of source columns [clo, chi): taps and cells move right with the output column
        const Axis c_first = axis<MODE>(x_first, jb.W, jb.w), c_last = axis<MODE>(x_first + ncol - 1, jb.W, jb.w);
        const int clo = c_first.s, chi = MODE == STIN_RESIZE_LINEAR ? c_last.q + 1 : c_last.s + c_last.n;
        const int span_bytes = (chi - clo) * C;
        if (tid < TH) {
            Axis none;                                                      // touches no row
            none.s = -1, none.n = 0, none.p = 0, none.q = -1;
            rowtab[tid] = tid < nrow ? axis<MODE>(ty * TH + tid, jb.H, jb.h) : none;
        }
        __syncthreads();
        // source rows [rlo, rhi) of the tile, and how they are staged: `rows` at a time at `pitch` bytes each, in chunks of `pitch`
        // bytes (one chunk, unless a row segment is longer than STAGE)
        Axis rt[TH];                                                        // the same in every lane: scalar registers
#pragma unroll
        for (int yy = 0; yy < TH; ++yy) {
            rt[yy].s = __builtin_amdgcn_readfirstlane(rowtab[yy].s);
            rt[yy].n = __builtin_amdgcn_readfirstlane(rowtab[yy].n);
            rt[yy].p = __builtin_amdgcn_readfirstlane(rowtab[yy].p);
            rt[yy].q = __builtin_amdgcn_readfirstlane(rowtab[yy].q);
        }
        const Axis r_first = rt[0], r_last = rowtab[nrow - 1];
        const int rlo = r_first.s, rhi = MODE == STIN_RESIZE_LINEAR ? r_last.q + 1 : r_last.s + r_last.n;
        const int whole = (15 + span_bytes + 15) & ~15;                     // a segment behind any head, in 16-byte pieces
        const int pitch = min(whole, STAGE), chunks = (whole + STAGE - 1) / STAGE, pieces = pitch / 16;
        const int rows_per_step = STAGE / pitch;
        const bool whole_tile = chunks == 1 && rhi - rlo <= rows_per_step;  // every source row of the tile is staged at once
        const unsigned to_rows = 0xffffffffu / (unsigned)pieces + 1u;       // pieces >= 2: i / pieces = umulhi(i, to_rows), i < 2^11
        // first byte of row r's segment relative to src_off (< 2^31: sides <= 2^14, C <= 4) and its phase mod 16
        const unsigned phase0 = (unsigned)src_addr + (unsigned)jb.src_off;
#define ROW_BYTE(r) (((r) * jb.W + clo) * C)
#define ROW_HEAD(r) ((int)((phase0 + (unsigned)ROW_BYTE(r)) & 15u))
        acc_t acc[TH][C];
#pragma unroll
        for (int yy = 0; yy < TH; ++yy)
#pragma unroll
            for (int ch = 0; ch < C; ++ch) acc[yy][ch] = 0;
        // rows [r0, r0 + R) into the stage, chunk k of their segments: every load of a thread is issued before its first LDS write
        auto stage_rows = [&](int r0, int R, int k) {
            __syncthreads();                                                // the stage's readers are done
            uint4 v[LOADS];
#pragma unroll
            for (int u = 0; u < LOADS; ++u) {
                const int i = tid + u * TB;
                if (i < R * pieces) {
                    const int rr = pieces == 1 ? i : (int)__umulhi((unsigned)i, to_rows), pc = i - rr * pieces;
                    const int row_byte = ROW_BYTE(r0 + rr), head = ROW_HEAD(r0 + rr);
                    const int rel = k * pitch + 16 * pc;
                    v[u] = rel < head + span_bytes ? load_piece(src, src_bytes, jb.src_off + (row_byte - head + rel))
                                                   : make_uint4(0u, 0u, 0u, 0u);
                }
            }
#pragma unroll
            for (int u = 0; u < LOADS; ++u) {
                const int i = tid + u * TB;
                if (i < R * pieces) *reinterpret_cast<uint4*>(stage + 16 * i) = v[u];                // row rr at rr * pitch
            }
            __syncthreads();
        };
        if (whole_tile) {
            // every output row walks its own source rows: no chunk ends, no search for the output rows a source row touches
            stage_rows(rlo, rhi - rlo, 0);
            if (active) {
                const int colpos = (cx.s - clo) * C;
#pragma unroll
                for (int yy = 0; yy < TH; ++yy) {
                    for (int i = 0; i < rt[yy].n; ++i) {
                        const unsigned wy = tap_weight<MODE>(rt[yy], i, jb.h);
                        if (wy == 0) continue;                              // (block-uniform)
                        const int r = tap_index<MODE>(rt[yy], i);
                        const uint8_t* __restrict__ px = stage + (r - rlo) * pitch + ROW_HEAD(r) + colpos;
                        unsigned hsum[C];
                        if (MODE == STIN_RESIZE_LINEAR) {
                            const unsigned wx0 = 2048u - (unsigned)cx.p, wx1 = (unsigned)cx.p;
                            const int second = (cx.q - cx.s) * C;
#pragma unroll
                            for (int ch = 0; ch < C; ++ch) hsum[ch] = wx0 * px[ch] + wx1 * px[second + ch];
                        } else {
#pragma unroll
                            for (int ch = 0; ch < C; ++ch) hsum[ch] = 0;
                            for (int tt = 0; tt < cx.n; ++tt) {
                                const unsigned wx = tap_weight<MODE>(cx, tt, jb.w);
#pragma unroll
                                for (int ch = 0; ch < C; ++ch) hsum[ch] += wx * px[tt * C + ch];
                            }
                        }
#pragma unroll
                        for (int ch = 0; ch < C; ++ch) acc[yy][ch] += (acc_t)wy * hsum[ch];
                    }
                }
            }
        } else {
            for (int r0 = rlo; r0 < rhi; r0 += rows_per_step) {
                const int R = min(rows_per_step, rhi - r0);
                for (int k = 0; k < chunks; ++k) {
                    stage_rows(r0, R, k);
                    if (active) {
                        for (int rr = 0; rr < R; ++rr) {
                            const int r = r0 + rr;
                            const int head = ROW_HEAD(r);
                            const uint8_t* __restrict__ buf = stage + rr * pitch;
                            // byte position of the thread's first tap in this chunk (any sign); a tap's bytes may lie in two chunks
                            const int base = head + (cx.s - clo) * C - k * pitch;
                            unsigned hsum[C];
#pragma unroll
                            for (int ch = 0; ch < C; ++ch) hsum[ch] = 0;
                            if (MODE == STIN_RESIZE_LINEAR) {
#pragma unroll
                                for (int tt = 0; tt < 2; ++tt) {
                                    const unsigned wx = tap_weight<MODE>(cx, tt, jb.w);
                                    const int pos = base + (tap_index<MODE>(cx, tt) - cx.s) * C;
                                    if (wx != 0) {
#pragma unroll
                                        for (int ch = 0; ch < C; ++ch)
                                            if ((unsigned)(pos + ch) < (unsigned)pitch) hsum[ch] += wx * buf[pos + ch];
                                    }
                                }
                            } else {
                                // taps with a byte in [0, pitch): base + t C > -C and base + t C < pitch
                                const int t_lo = base >= 0 ? 0 : (-base) / C;
                                const int t_hi = base >= pitch ? 0 : min(cx.n, (pitch - base + C - 1) / C);
                                for (int tt = t_lo; tt < t_hi; ++tt) {
                                    const unsigned wx = tap_weight<MODE>(cx, tt, jb.w);
                                    const int pos = base + tt * C;
#pragma unroll
                                    for (int ch = 0; ch < C; ++ch)
                                        if ((unsigned)(pos + ch) < (unsigned)pitch) hsum[ch] += wx * buf[pos + ch];
                                }
                            }
#pragma unroll
                            for (int yy = 0; yy < TH; ++yy) {
                                const unsigned wy = index_weight<MODE>(rt[yy], r, jb.h);                 // (block-uniform)
                                if (wy != 0) {
#pragma unroll
                                    for (int ch = 0; ch < C; ++ch) acc[yy][ch] += (acc_t)wy * hsum[ch];
                                }
                            }
                        }
                    }
                }
            }
        }
        // one rounding, then every result row at its destination's phase so that 16-byte pieces are aligned on both sides
        const int64_t d_tile = jb.dst_off + ((int64_t)(ty * TH) * jb.w + x_first) * C;
        if (active) {
#pragma unroll
            for (int yy = 0; yy < TH; ++yy) {
                if (yy < nrow) {
                    const int shift = (int)((dst_addr + (uintptr_t)(d_tile + (int64_t)yy * jb.w * C)) & 15u);
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) {
                        unsigned o;
                        if (MODE == STIN_RESIZE_LINEAR) {
                            o = (unsigned)((acc[yy][ch] + (1u << 21)) >> 22);
                        } else {
                            const unsigned long long wh = (unsigned long long)jb.W * (unsigned long long)jb.H;
                            const unsigned long long num = 2ull * acc[yy][ch] + wh;
                            // (the narrow division gives the same quotient: it is taken only when both operands fit)
                            o = wh < (1ull << 22) ? (unsigned)num / (unsigned)(2ull * wh) : (unsigned)(num / (2ull * wh));
                        }
                        outbuf[yy * OUT_PITCH + shift + tid * C + ch] = (uint8_t)o;
                    }
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < nrow * OUT_PIECES; i += TB) {
            const int yy = i / OUT_PIECES, lo = 16 * (i - yy * OUT_PIECES);
            const int64_t d0 = d_tile + (int64_t)yy * jb.w * C;
            const int shift = (int)((dst_addr + (uintptr_t)d0) & 15u), total_out = shift + ncol * C;
            if (lo < total_out) {
                uint8_t* __restrict__ line = dst + (d0 - shift);            // 16-byte aligned; bytes before `shift` are not ours
                const uint8_t* __restrict__ from = outbuf + yy * OUT_PITCH;
                if (lo >= shift && lo + 16 <= total_out) {
                    *reinterpret_cast<uint4*>(line + lo) = *reinterpret_cast<const uint4*>(from + lo);
                } else {
                    for (int e = 0; e < 16; ++e)
                        if (lo + e >= shift && lo + e < total_out) line[lo + e] = from[lo + e];
                }
            }
        }
        // (the next tile writes rowtab and outbuf only behind barriers that every thread reaches after this loop)
#undef ROW_BYTE
#undef ROW_HEAD
    }
}

template <int MODE>
int launch(const uint8_t* src, int64_t src_bytes, uint8_t* dst, int64_t dst_bytes, const int64_t* jobs, int J, int channels,
           hipStream_t stream) {
    switch (channels) {
        case 1: hipLaunchKernelGGL((k_resize<MODE, 1>), dim3(GRID), dim3(TB), 0, stream, src, src_bytes, dst, dst_bytes, jobs, J); break;
        case 3: hipLaunchKernelGGL((k_resize<MODE, 3>), dim3(GRID), dim3(TB), 0, stream, src, src_bytes, dst, dst_bytes, jobs, J); break;
        default: hipLaunchKernelGGL((k_resize<MODE, 4>), dim3(GRID), dim3(TB), 0, stream, src, src_bytes, dst, dst_bytes, jobs, J); break;
    }
    return stin_launch_status();
}
}  // namespace

extern "C" int stin_resize_u8(const uint8_t* src, int64_t src_bytes, uint8_t* dst, int64_t dst_bytes, const int64_t* jobs, int J,
                              int channels, int mode, stin_stream_t stream_) {
    stin_clear_stale_error();
    STIN_REQUIRE(J > 0 && src_bytes > 0 && dst_bytes > 0, STIN_E_SIZE);
    STIN_REQUIRE(channels == 1 || channels == 3 || channels == 4, STIN_E_SIZE);
    STIN_REQUIRE(mode == STIN_RESIZE_LINEAR || mode == STIN_RESIZE_AREA, STIN_E_SIZE);
    STIN_REQUIRE(src && dst && jobs, STIN_E_NULL);
    STIN_REQUIRE((reinterpret_cast<uintptr_t>(jobs) & 7u) == 0, STIN_E_ALIGN);
    hipStream_t stream = (hipStream_t)stream_;
    return mode == STIN_RESIZE_LINEAR ? launch<STIN_RESIZE_LINEAR>(src, src_bytes, dst, dst_bytes, jobs, J, channels, stream)
                                      : launch<STIN_RESIZE_AREA>(src, src_bytes, dst, dst_bytes, jobs, J, channels, stream);
}
