// View metrics on the device: PSNR's sums and SSIM of two sets of rendered views, per pose, in one pass over the images.
// Contract: include/stin_hip.h ("View metrics"); tests/_viewmetrics_oracle.py restates it in numpy, one 121-tap sum per window, and
// agrees byte for byte.  NOT pinned against skimage or piq: integer taps, no padding, no luma conversion, no multi-scale SSIM.
//
//   tile     a workgroup owns the TH x TW windows whose top-left corners are the pixels [y0, y0 + TH) x [x0, x0 + TW) of one pose, and
//            the same pixels for the pixel sums: every pixel and every window belongs to exactly one workgroup.
//   stage    the (TH + 10) x (TW + 10) pixels under those windows, of a, b and the two masks, as whole 16-byte lines (stage_rows).
//   box      horizontal counts of covered pixels, then 11 of them down a column: a window counts when they sum to 121.  A pixel
//            outside the image is not covered, so 'valid' mode needs no test of its own.  A tile without a counted window (off the
//            mesh, outside the region) skips the channel passes.
//   channel  one at a time: horizontal pass into five uint32 planes (the largest row sum is 65536 * 65025 < 2^32), vertical pass
//            in uint64 registers (v_mad_u64_u32), v and q in fp64.
//   reduce   wave shuffles, four partial rows in LDS, one 64-bit integer atomic per figure into the pose's row.
// Integers are all that is summed: the table does not depend on the tiling or on the order in which workgroups arrive.
#include "stin_common.h"

#include <cmath>

namespace {

constexpr int NT = 256;                                    // threads per workgroup
constexpr int WIN = STIN_VIEW_METRICS_WINDOW, HALO = WIN - 1;
constexpr int TH = 16, TW = 32;                            // window corners (and owned pixels) of a workgroup
constexpr int SH = TH + HALO, SW = TW + HALO;              // staged pixels: 26 x 42
constexpr int AP = (SW * 4 + 15 + 15) / 16 * 16;           // row pitch of a staged image: 4 channels and up to 15 bytes in front
constexpr int MP = (SW + 15 + 15) / 16 * 16;               // row pitch of a staged mask
constexpr int COLS = STIN_VIEW_METRICS_COLS;
constexpr int PER_THREAD = TH * TW / NT;                   // windows of a thread: rows ry * PER_THREAD + i of column cx
static_assert(TH * TW % NT == 0 && NT % TW == 0 && NT / STIN_WAVE * COLS <= NT, "thread maps of the tile");
// LDS: 2 * 26 * 192 + 2 * 26 * 64 + 26 * 32 + 5 * 26 * 32 * 4 + 4 * 5 * 8 = 30 944 bytes, 31 200 with the workgroup vote's

__host__ __device__ constexpr unsigned tap(int j) {
    constexpr unsigned w[WIN] = {67, 498, 2359, 7167, 13960, 17434, 13960, 7167, 2359, 498, 67};
    return w[j];
}
static_assert(tap(0) + tap(1) + tap(2) + tap(3) + tap(4) + tap(5) + tap(6) + tap(7) + tap(8) + tap(9) + tap(10) == 65536, "taps");

struct Image {
    const uint8_t* base;                                   // nullptr: no array
    int64_t bytes, stride;                                 // of the whole array, of an image row
};

// Rows [0, nrows) of a byte array into `dst` (row pitch `pitch`, a multiple of 16): row r is the `seg` bytes at offset row0 + r * stride.
// What is copied are the 16-byte lines of memory those bytes lie in, so byte i of row r lands at dst[r * pitch + row_shift(r) + i]:
// one 16-byte load per line that lies inside the array, a line that crosses one of its ends byte by byte.
__device__ inline void stage_rows(uint8_t* dst, int pitch, const Image& im, int64_t row0, int seg, int nrows) {
    const int lines = pitch / 16;
    for (int i = threadIdx.x; i < nrows * lines; i += NT) {
        const int r = i / lines, l = i - r * lines;
        const int64_t first = row0 + r * im.stride;
        const int64_t p = first - (int64_t)(reinterpret_cast<uintptr_t>(im.base + first) & 15u) + 16 * l;     // may be < 0: in front of the array
        if (p >= first + seg) continue;
        uint4 v;
        if (p >= 0 && p + 16 <= im.bytes) {
            v = *reinterpret_cast<const uint4*>(im.base + p);
        } else {
            unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (p + e >= 0 && p + e < im.bytes) w[e >> 2] |= (unsigned)im.base[p + e] << (8 * (e & 3));
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4*>(dst + r * pitch + 16 * l) = v;
    }
}

// where row r of the staged region starts inside its LDS row (the address of its first byte modulo 16)
__device__ __forceinline__ int row_shift(const Image& im, int64_t row0, int r) {
    return (int)((unsigned)reinterpret_cast<uintptr_t>(im.base + row0 + r * im.stride) & 15u);
}

__device__ inline long long ssim_q(unsigned long long Sa, unsigned long long Sb, unsigned long long Saa, unsigned long long Sbb,
                                   unsigned long long Sab) {
    const double s = 1.0 / 4294967296.0, C1 = 6.5025, C2 = 58.5225;
    const double ma = (double)Sa * s, mb = (double)Sb * s;
    const double va = (double)Saa * s - ma * ma, vb = (double)Sbb * s - mb * mb, c = (double)Sab * s - ma * mb;
    const double v = ((2.0 * ma * mb + C1) * (2.0 * c + C2)) / ((ma * ma + mb * mb + C1) * (va + vb + C2));
    return (long long)rint(v * 4294967296.0);
}

__global__ __launch_bounds__(NT) void k_view_metrics(Image ima, Image imb, Image imc, Image imr, int64_t p0, int H, int W, int K,
                                                     int tiles_x, unsigned long long* __restrict__ table) {
    __shared__ uint4 s_a4[SH * AP / 16], s_b4[SH * AP / 16], s_c4[SH * MP / 16], s_r4[SH * MP / 16];
    __shared__ uint8_t s_hc[SH * TW];                                     // covered pixels among the 11 to the right, per staged row
    __shared__ unsigned s_plane[5][SH * TW];                              // Sa, Sb, Saa, Sbb, Sab of the horizontal pass
    __shared__ unsigned long long s_red[NT / STIN_WAVE][COLS];
    const uint8_t* s_a = reinterpret_cast<const uint8_t*>(s_a4);
    const uint8_t* s_b = reinterpret_cast<const uint8_t*>(s_b4);
    const uint8_t* s_c = reinterpret_cast<const uint8_t*>(s_c4);
    const uint8_t* s_r = reinterpret_cast<const uint8_t*>(s_r4);
    const int t = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * TH, x0 = tx * TW;
    const int64_t pose = p0 + blockIdx.y;
    const int nrows = H - y0 < SH ? H - y0 : SH, ncols = W - x0 < SW ? W - x0 : SW;        // the staged pixels inside the image
    const int64_t pix0 = (pose * H + y0) * W + x0;
    const int64_t ab0 = pix0 * K;                                         // byte offsets of the first staged pixel
    const bool has_c = imc.base != nullptr, has_r = imr.base != nullptr;
    stage_rows(reinterpret_cast<uint8_t*>(s_a4), AP, ima, ab0, ncols * K, nrows);
    stage_rows(reinterpret_cast<uint8_t*>(s_b4), AP, imb, ab0, ncols * K, nrows);
    if (has_c) stage_rows(reinterpret_cast<uint8_t*>(s_c4), MP, imc, pix0, ncols, nrows);
    if (has_r) stage_rows(reinterpret_cast<uint8_t*>(s_r4), MP, imr, pix0, ncols, nrows);
    __syncthreads();
    // staged pixel (r, c): inside the image and covered / in the region
    auto covered = [&](int r, int c) { return r < nrows && c < ncols && (!has_c || s_c[r * MP + row_shift(imc, pix0, r) + c] != 0); };
    auto in_region = [&](int r, int c) { return r < nrows && c < ncols && (!has_r || s_r[r * MP + row_shift(imr, pix0, r) + c] != 0); };

    unsigned long long n_pix = 0, sum_abs = 0, sum_sq = 0, n_win = 0;
    long long sum_q = 0;
    for (int i = t; i < TH * TW; i += NT) {                               // the tile's own pixels
        const int r = i / TW, c = i - r * TW;
        if (!(covered(r, c) && in_region(r, c))) continue;
        const uint8_t* pa = s_a + r * AP + row_shift(ima, ab0, r) + c * K;
        const uint8_t* pb = s_b + r * AP + row_shift(imb, ab0, r) + c * K;
        ++n_pix;
        for (int k = 0; k < K; ++k) {
            const int d = (int)pa[k] - (int)pb[k];
            sum_abs += (unsigned)(d < 0 ? -d : d);
            sum_sq += (unsigned)(d * d);
        }
    }
    for (int i = t; i < SH * TW; i += NT) {
        const int r = i / TW, c = i - r * TW;
        int n = 0;
#pragma unroll
        for (int j = 0; j < WIN; ++j) n += covered(r, c + j) ? 1 : 0;
        s_hc[i] = (uint8_t)n;
    }
    __syncthreads();
    const int cx = t % TW, wr0 = t / TW * PER_THREAD;                     // the thread's windows: corners (wr0 + i, cx)
    bool counted[PER_THREAD];
    bool any = false;
#pragma unroll
    for (int i = 0; i < PER_THREAD; ++i) {
        int box = 0;
#pragma unroll
        for (int j = 0; j < WIN; ++j) box += s_hc[(wr0 + i + j) * TW + cx];
        counted[i] = box == WIN * WIN && in_region(wr0 + i + HALO / 2, cx + HALO / 2);
        n_win += counted[i] ? 1 : 0;
        any |= counted[i];
    }
    const int channels = __syncthreads_or(any) ? K : 0;                   // a tile without a counted window (off the mesh, outside the region) is done
    for (int k = 0; k < channels; ++k) {
        for (int i = t; i < nrows * TW; i += NT) {                      // horizontal pass of channel k (rows below the image: never read)
            const int r = i / TW, c = i - r * TW;
            const uint8_t* pa = s_a + r * AP + row_shift(ima, ab0, r) + c * K + k;
            const uint8_t* pb = s_b + r * AP + row_shift(imb, ab0, r) + c * K + k;
            unsigned Sa = 0, Sb = 0, Saa = 0, Sbb = 0, Sab = 0;
#pragma unroll
            for (int j = 0; j < WIN; ++j) {
                const unsigned av = pa[j * K], bv = pb[j * K], wa = tap(j) * av, wb = tap(j) * bv;
                Sa += wa;
                Sb += wb;
                Saa += wa * av;
                Sbb += wb * bv;
                Sab += wa * bv;
            }
            s_plane[0][i] = Sa;
            s_plane[1][i] = Sb;
            s_plane[2][i] = Saa;
            s_plane[3][i] = Sbb;
            s_plane[4][i] = Sab;
        }
        __syncthreads();
        if (any) {                                                        // vertical pass: PER_THREAD + 10 rows feed PER_THREAD windows
            unsigned long long acc[PER_THREAD][5] = {};
#pragma unroll
            for (int r = 0; r < PER_THREAD + HALO; ++r) {
                unsigned h[5];
#pragma unroll
                for (int m = 0; m < 5; ++m) h[m] = s_plane[m][(wr0 + r) * TW + cx];
#pragma unroll
                for (int i = 0; i < PER_THREAD; ++i)
                    if (r - i >= 0 && r - i < WIN) {
#pragma unroll
                        for (int m = 0; m < 5; ++m) acc[i][m] += (unsigned long long)tap(r - i) * h[m];
                    }
            }
#pragma unroll
            for (int i = 0; i < PER_THREAD; ++i)
                if (counted[i]) sum_q += ssim_q(acc[i][0], acc[i][1], acc[i][2], acc[i][3], acc[i][4]);
        }
        __syncthreads();                                                  // the planes are free for the next channel
    }
    unsigned long long part[COLS] = {n_pix, sum_abs, sum_sq, n_win, (unsigned long long)sum_q};
#pragma unroll
    for (int m = 0; m < COLS; ++m) {
#pragma unroll
        for (int o = STIN_WAVE / 2; o > 0; o >>= 1) part[m] += __shfl_down(part[m], o, STIN_WAVE);
        if (t % STIN_WAVE == 0) s_red[t / STIN_WAVE][m] = part[m];
    }
    __syncthreads();
    if (t < COLS) {
        unsigned long long sum = 0;
#pragma unroll
        for (int w = 0; w < NT / STIN_WAVE; ++w) sum += s_red[w][t];
        atomicAdd(table + pose * COLS + t, sum);                          // (two's complement: ssim_q adds as a signed figure)
    }
}

bool view_metrics_sizes_ok(int64_t P, int H, int W, int K) {
    return P >= 0 && P < (int64_t)INT32_MAX && H >= 1 && H <= STIN_RENDER_MAX_SIZE && W >= 1 && W <= STIN_RENDER_MAX_SIZE && K >= 1 && K <= 4;
}

}  // namespace

extern "C" size_t stin_view_metrics_workspace_bytes(int64_t P, int H, int W, int K) {
    return 0;                                              // (the query is part of the ABI so that a later form may need one)
}

extern "C" int stin_view_metrics_u8(const uint8_t* a, const uint8_t* b, const uint8_t* covered, const uint8_t* region, int64_t P, int H,
                                    int W, int K, int64_t* table, void* workspace, size_t workspace_bytes, stin_stream_t stream_) {
    STIN_REQUIRE(view_metrics_sizes_ok(P, H, W, K), STIN_E_SIZE);
    STIN_REQUIRE(P == 0 || (a != nullptr && b != nullptr && table != nullptr), STIN_E_NULL);
    (void)workspace;
    (void)workspace_bytes;
    hipStream_t stream = (hipStream_t)stream_;
    stin_clear_stale_error();
    if (P == 0) return STIN_OK;
    (void)hipMemsetAsync(table, 0, (size_t)P * COLS * sizeof(int64_t), stream);
    const int64_t pixels = P * H * W;
    const Image ima = {a, pixels * K, (int64_t)W * K}, imb = {b, pixels * K, (int64_t)W * K};
    const Image imc = {covered, pixels, W}, imr = {region, pixels, W};
    const int tiles_x = (W + TW - 1) / TW, tiles = tiles_x * ((H + TH - 1) / TH);          // <= 128 * 256
    const int64_t per_launch = tiles > (1 << 22) / 65535 ? (1 << 22) / tiles : 65535;      // grid.y <= 65535, under 2^32 threads a launch
    for (int64_t p0 = 0; p0 < P; p0 += per_launch) {
        const unsigned np = (unsigned)(P - p0 < per_launch ? P - p0 : per_launch);
        hipLaunchKernelGGL(k_view_metrics, dim3((unsigned)tiles, np), dim3(NT), 0, stream, ima, imb, imc, imr, p0, H, W, K, tiles_x,
                           reinterpret_cast<unsigned long long*>(table));
    }
    return stin_launch_status();
}
