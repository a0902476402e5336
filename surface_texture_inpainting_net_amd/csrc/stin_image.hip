// The 2-D image-graph inpainting experiment around the network (experiments/2d_inpainting, config 1): what the reference's
// ImageGraphTextureDataSet builds on CPU workers per item (datasets/imagegraph_dataloader.py:46-160) and what its trainer reads
// back with four .item() calls per step (trainers/inpainting2d_trainer.py:382-398), as three enqueue-only calls:
//
//   stin_grid_levels_i64     the 4-connected grid graph of every level, the 2x-repeat traces, num_vertices and the batch vector of
//                            B images in ONE launch (closed-form edge positions: no sort, no set);
//   stin_image_samples_u8    normalise + centre crop + rot90 + flip + circle masks of B resident uint8 images in ONE launch;
//   stin_image_metrics_f32   loss / l1 / mse / per-image-mean psnr / masked count as one row of a device table: fp64 block
//                            partials per image, folded in a fixed order by the finaliser - no float atomics, same bits every run.
//
// Plain vector loads and stores only.  Compiled with -ffp-contract=off: v * 2 - 1 is a multiply and an add, as numpy forms it.
#include "stin_common.h"

#include <math.h>

namespace {
constexpr int TB = 256;                    // threads per block
constexpr int MAX_LEVELS = STIN_GRID_MAX_LEVELS;

// ---------------------------------------------------------------------------------------------------------------- grid levels
// Flat work list of one launch: level l's edge part is one item per (image, vertex), its trace part one item per fine vertex
// (levels >= 1), then the batch vector (one item per level-0 vertex) and num_vertices (B * L items).
struct grid_args {
    int64_t edge_begin[MAX_LEVELS], trace_begin[MAX_LEVELS];       // first work item of the part (trace_begin[0] unused)
    int64_t edge_out[MAX_LEVELS], trace_out[MAX_LEVELS];           // first element of the part in `out`
    int64_t batch_begin, batch_out, nv_begin, total;
    int32_t side[MAX_LEVELS];
    int32_t B, L;
};

__global__ __launch_bounds__(TB) void k_grid_levels(grid_args a, int64_t* __restrict__ out, int32_t* __restrict__ num_vertices) {
    const int64_t t = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (t >= a.total) return;
    if (t >= a.nv_begin) {                                          // num_vertices [B, L]
        const int64_t i = t - a.nv_begin;
        const int s = a.side[i % a.L];
        num_vertices[i] = s * s;
        return;
    }
    if (t >= a.batch_begin) {                                       // batch [B * S * S]
        const int64_t i = t - a.batch_begin;
        out[a.batch_out + i] = i / ((int64_t)a.side[0] * a.side[0]);
        return;
    }
    int l = a.L - 1;
    while (l > 0 && t < a.edge_begin[l]) --l;                       // parts are laid out level by level: edges, then trace
    if (l > 0 && t >= a.trace_begin[l]) {                           // trace of level l: fine = level l - 1, coarse = level l
        const int64_t i = t - a.trace_begin[l];
        const int64_t sc = a.side[l], sf = a.side[l - 1];
        const int64_t b = i / (sf * sf), p = i % (sf * sf);
        const int64_t r = p / sf, c = p % sf;
        out[a.trace_out[l] + i] = b * sc * sc + (r / 2) * sc + (c / 2);
        return;
    }
    // edges of level l: vertex (r, c) of image b owns the slots behind those of every earlier vertex, neighbours up / left / right / down
    const int64_t i = t - a.edge_begin[l];
    const int64_t s = a.side[l], n = s * s;
    const int64_t b = i / n, p = i % n;
    const int64_t r = p / s, c = p % s;
    const bool up = r > 0, left = c > 0, right = c < s - 1, down = r < s - 1;
    const int64_t row_deg = 2 + (up ? 1 : 0) + (down ? 1 : 0);      // of an inner column of this row
    const int64_t before_rows = r > 0 ? r * (4 * s - 2) - s : 0;    // row 0 has no `up`; rows < r never include the last row
    const int64_t before_cols = c * row_deg - (c > 0 ? 1 : 0);      // column 0 has no `left`
    const int64_t per_image = 4 * s * (s - 1), total_e = a.B * per_image;
    int64_t e = a.edge_out[l] + b * per_image + before_rows + before_cols;
    const int64_t v = b * n + p;
    int64_t* __restrict__ src = out;
    int64_t* __restrict__ dst = out + total_e;
    if (up) { src[e] = v; dst[e] = v - s; ++e; }
    if (left) { src[e] = v; dst[e] = v - 1; ++e; }
    if (right) { src[e] = v; dst[e] = v + 1; ++e; }
    if (down) { src[e] = v; dst[e] = v + s; ++e; }
}

// the layout both the size query and the launch use; -> false when the shape is not supported
bool grid_layout(int B, int S, int L, grid_args* a) {
    if (B <= 0 || S <= 0 || L <= 0 || L > MAX_LEVELS) return false;
    if (S % (1 << (L - 1)) != 0) return false;
    if ((int64_t)B * S * S >= ((int64_t)1 << 31)) return false;
    a->B = B;
    a->L = L;
    int64_t work = 0, elems = 0;
    for (int l = 0; l < L; ++l) {
        const int64_t s = S >> l;
        a->side[l] = (int32_t)s;
        a->edge_begin[l] = work;
        a->edge_out[l] = elems;
        work += (int64_t)B * s * s;
        elems += 2 * (int64_t)B * 4 * s * (s - 1);
        a->trace_begin[l] = work;
        a->trace_out[l] = elems;
        if (l > 0) {
            const int64_t sf = S >> (l - 1);
            work += (int64_t)B * sf * sf;
            elems += (int64_t)B * sf * sf;
        }
    }
    for (int l = L; l < MAX_LEVELS; ++l) {
        a->side[l] = 0;
        a->edge_begin[l] = a->trace_begin[l] = work;
        a->edge_out[l] = a->trace_out[l] = elems;
    }
    a->batch_begin = work;
    a->batch_out = elems;
    work += (int64_t)B * S * S;
    elems += (int64_t)B * S * S;
    a->nv_begin = work;
    work += (int64_t)B * L;
    a->total = work;
    return true;
}

int64_t grid_elems(const grid_args& a) { return a.batch_out + (int64_t)a.B * a.side[0] * a.side[0]; }

// ------------------------------------------------------------------------------------------------------------ sample builder
// One thread per output pixel (b, r, c).  rec = int64 [B][HEAD + 2 * num_circles]: pool offset, h, w, k, flip, (row_start, col_start)...
constexpr int HEAD = STIN_IMAGE_RECORD_HEAD;

__global__ __launch_bounds__(TB) void k_image_samples(const uint8_t* __restrict__ pool, int64_t pool_bytes,
                                                      const int64_t* __restrict__ rec, int B, int S, int R, int num_circles,
                                                      float* __restrict__ x, float* __restrict__ color,
                                                      uint8_t* __restrict__ mask) {
    const int64_t n = (int64_t)S * S;
    const int64_t t = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (t >= (int64_t)B * n) return;
    const int64_t b = t / n, p = t % n;
    const int r = (int)(p / S), c = (int)(p % S);
    const int64_t* __restrict__ q = rec + b * (HEAD + 2 * (int64_t)num_circles);
    const int64_t off = q[0], h = q[1], w = q[2];
    const int k = (int)q[3] & 3;
    // undo the flip along axis 1, then np.rot90(m, k): k = 1: out[i, j] = m[j, S-1-i]; 2: m[S-1-i, S-1-j]; 3: m[S-1-j, i]
    const int j = q[4] ? S - 1 - c : c, i = r;
    int si, sj;
    switch (k) {
        case 0: si = i; sj = j; break;
        case 1: si = j; sj = S - 1 - i; break;
        case 2: si = S - 1 - i; sj = S - 1 - j; break;
        default: si = S - 1 - j; sj = i; break;
    }
    const int64_t h0 = (h - S) / 2, w0 = (w - S) / 2;               // CenterCrop: int((h - S) / 2), h >= S
    const int64_t at = off + ((h0 + si) * w + (w0 + sj)) * 3;
    float col[3] = {0.f, 0.f, 0.f};
    if (at >= 0 && at + 3 <= pool_bytes) {                          // (the host has checked the records: never false for them)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float v = (float)pool[at + ch] * (1.0f / 255.0f);
            col[ch] = v * 2.0f - 1.0f;
        }
    }
    bool m = false;
    for (int ci = 0; ci < num_circles; ++ci) {
        const int64_t rr = r - q[HEAD + 2 * ci], cc = c - q[HEAD + 2 * ci + 1];
        if (rr >= 0 && rr < 2 * R && cc >= 0 && cc < 2 * R) m = m || ((rr - R) * (rr - R) + (cc - R) * (cc - R) <= (int64_t)R * R);
    }
    const float keep = m ? 0.f : 1.f;
    color[t * 3 + 0] = col[0];
    color[t * 3 + 1] = col[1];
    color[t * 3 + 2] = col[2];
    st4(x + t * 4, make_float4(col[0] * keep, col[1] * keep, col[2] * keep, m ? 1.f : 0.f));
    mask[t] = m ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------------- metrics
enum { Q_ABS, Q_SQ, Q_CNT, NQ };

// block (x, b) covers rows [x * TB, (x + 1) * TB) of image b; partial[(q * B + b) * bpi + x]
__global__ __launch_bounds__(TB) void k_image_metrics_rows(const float* __restrict__ out, int64_t ldo, const float* __restrict__ color,
                                                           const uint8_t* __restrict__ mask, int64_t n_img, int C, int composite,
                                                           double* __restrict__ partial, int64_t bpi) {
    __shared__ double sm[NQ][TB / 64];
    double acc[NQ] = {0.0, 0.0, 0.0};
    const int64_t b = blockIdx.y, B = gridDim.y;
    const int64_t r = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (r < n_img) {
        const int64_t v = b * n_img + r;
        const bool inside = mask[v] != 0;
        if (inside) acc[Q_CNT] = 1.0;
        if (inside || !composite) {                                  // P = color elsewhere: d = color - color = 0 exactly
            for (int c = 0; c < C; ++c) {
                const float d = out[v * ldo + c] - color[v * C + c];
                acc[Q_ABS] += (double)fabsf(d);
                acc[Q_SQ] += (double)(d * d);
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const double s = stin_wave_sum(acc[q]);
        if (lane == 0) sm[q][wave] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < NQ) {
        const int q = threadIdx.x;
        partial[((int64_t)q * B + b) * bpi + blockIdx.x] = (sm[q][0] + sm[q][1]) + (sm[q][2] + sm[q][3]);
    }
}

// wave q folds quantity q: image after image, each image's block partials lane-strided and then the shuffle tree (a fixed order);
// the wave of the squares also forms the per-image psnr terms.  Divisions and log10 in double.
__global__ __launch_bounds__(64 * NQ) void k_image_metrics_final(const double* __restrict__ partial, int64_t bpi, int B, int64_t n_img,
                                                                 int C, float data_range, const float* __restrict__ loss_in,
                                                                 float* __restrict__ row_out) {
    __shared__ double sums[NQ];
    __shared__ double psnr_sum;
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const double per_image = (double)n_img * (double)C, r2 = (double)data_range * (double)data_range;
    double total = 0.0, psnr = 0.0;
    for (int b = 0; b < B; ++b) {
        double s = 0.0;
        for (int64_t i = lane; i < bpi; i += 64) s += partial[((int64_t)q * B + b) * bpi + i];
        s = stin_wave_sum(s);
        total += s;                                                  // (lane 0 holds the sum)
        if (q == Q_SQ) psnr += -10.0 * log10(s / per_image / r2 + 1e-8);
    }
    if (lane == 0) {
        sums[q] = total;
        if (q == Q_SQ) psnr_sum = psnr;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        const double n = per_image * (double)B;
        const float l1 = (float)(sums[Q_ABS] / n);
        float v = 0.f;
        switch (threadIdx.x) {
            case 0: v = loss_in ? loss_in[0] : l1; break;
            case 1: v = l1; break;
            case 2: v = (float)(sums[Q_SQ] / n); break;
            case 3: v = (float)(psnr_sum / (double)B); break;
            case 4: v = (float)sums[Q_CNT]; break;
            default: break;
        }
        row_out[threadIdx.x] = v;
    }
}

inline int64_t blocks_per_image(int64_t n_img) { return (n_img + TB - 1) / TB; }
}  // namespace

extern "C" int64_t stin_grid_levels_elems(int B, int S, int L) {
    grid_args a;
    return grid_layout(B, S, L, &a) ? grid_elems(a) : 0;
}

extern "C" int stin_grid_levels_i64(int B, int S, int L, int64_t* out, int64_t out_elems, int32_t* num_vertices,
                                    stin_stream_t stream_) {
    stin_clear_stale_error();
    STIN_REQUIRE(B > 0 && S > 0 && L > 0, STIN_E_SIZE);
    STIN_REQUIRE(L <= MAX_LEVELS, STIN_E_UNSUPPORTED);
    STIN_REQUIRE(S % (1 << (L - 1)) == 0, STIN_E_SIZE);
    grid_args a;
    STIN_REQUIRE(grid_layout(B, S, L, &a), STIN_E_UNSUPPORTED);
    STIN_REQUIRE(out && num_vertices, STIN_E_NULL);
    STIN_REQUIRE(out_elems >= grid_elems(a), STIN_E_WORKSPACE);
    const int64_t blocks = (a.total + TB - 1) / TB;
    STIN_REQUIRE(blocks < ((int64_t)1 << 31), STIN_E_UNSUPPORTED);
    hipLaunchKernelGGL(k_grid_levels, dim3((unsigned)blocks), dim3(TB), 0, (hipStream_t)stream_, a, out, num_vertices);
    return stin_launch_status();
}

extern "C" int stin_image_samples_u8(const uint8_t* pool, int64_t pool_bytes, const int64_t* records, int B, int S, int R,
                                     int num_circles, float* x, float* color, uint8_t* mask, stin_stream_t stream_) {
    stin_clear_stale_error();
    STIN_REQUIRE(B > 0 && S > 0 && R >= 0 && num_circles >= 0 && pool_bytes > 0, STIN_E_SIZE);
    STIN_REQUIRE((int64_t)B * S * S < ((int64_t)1 << 31), STIN_E_UNSUPPORTED);
    STIN_REQUIRE(pool && records && x && color && mask, STIN_E_NULL);
    STIN_REQUIRE(stin_aligned16(x) && (reinterpret_cast<uintptr_t>(records) & 7u) == 0, STIN_E_ALIGN);
    const int64_t blocks = ((int64_t)B * S * S + TB - 1) / TB;
    hipLaunchKernelGGL(k_image_samples, dim3((unsigned)blocks), dim3(TB), 0, (hipStream_t)stream_, pool, pool_bytes, records, B, S, R,
                       num_circles, x, color, mask);
    return stin_launch_status();
}

extern "C" size_t stin_image_metrics_workspace_bytes(int64_t N, int num_images) {
    if (N <= 0 || num_images <= 0 || N % num_images != 0) return 0;
    return 256 + (size_t)NQ * (size_t)num_images * (size_t)blocks_per_image(N / num_images) * sizeof(double);
}

extern "C" int stin_image_metrics_f32(const float* out, int64_t ldo, const float* color, const uint8_t* mask, int64_t N,
                                      int num_images, int C, int composite, float data_range, const float* loss, float* row_out,
                                      void* workspace, size_t workspace_bytes, stin_stream_t stream_) {
    stin_clear_stale_error();
    STIN_REQUIRE(N > 0 && N <= ((int64_t)1 << 24) && num_images > 0 && num_images <= 65535 && N % num_images == 0, STIN_E_SIZE);
    STIN_REQUIRE(C >= 1 && C <= 4 && ldo >= C && data_range > 0.f, STIN_E_SIZE);
    STIN_REQUIRE(out && color && mask && row_out && workspace, STIN_E_NULL);
    STIN_REQUIRE(workspace_bytes >= stin_image_metrics_workspace_bytes(N, num_images), STIN_E_WORKSPACE);
    const int64_t n_img = N / num_images, bpi = blocks_per_image(n_img);
    double* partial = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(k_image_metrics_rows, dim3((unsigned)bpi, (unsigned)num_images), dim3(TB), 0, stream, out, ldo, color, mask,
                       n_img, C, composite, partial, bpi);
    hipLaunchKernelGGL(k_image_metrics_final, dim3(1), dim3(64 * NQ), 0, stream, partial, bpi, num_images, n_img, C, data_range,
                       loss, row_out);
    return stin_launch_status();
}
