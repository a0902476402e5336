// The segmentation experiment's objective and metric (reference trainers/segmentation_trainer.py:54, :125-166, :206-235) for
// gfx950.  Contract: include/stin_hip.h ("segmentation").
//
//   fwd: weighted cross entropy with ignore_index (torch.nn.CrossEntropyLoss(weight, ignore_index), reduction 'mean') AND the
//        confusion matrix of the arg-max prediction (ConfusionMatrixDCM.add) in ONE pass over the [N, C] logits, optionally
//        through a row gather (rows = original_index_traces: the full-resolution evaluation without the [N_orig, C] copy).
//        One lane per row: max + first arg-max (NaN maximal, as torch.max), lse = max + log sum exp(z - max) in fp32,
//        nll = (max - z_y) + log sum.  sum w_y nll and sum w_y go into fp64 per-block partials; k_seg_ce_final adds them in a
//        fixed order.  Blocks own 256 consecutive targets: the grid depends on N only, so the loss has the same bits on every run
//        and device.  Without a gather, a block's rows are staged into LDS with coalesced loads first (an 84-byte row at C = 21
//        is not 16-byte aligned: per-lane row loads would not coalesce); the LDS row stride is odd (no bank conflicts).
//        Confusion counts go into a C x C int32 LDS histogram per block (integer LDS atomics) whose non-zero bins are flushed
//        with integer atomics into the int64 matrix: exact and order-independent.
//   bwd: dlogits = g w_y (softmax(z) - onehot(y)) / den, g and den read from device memory (no host round trip); softmax
//        recomputed from the logits (the forward stores no gradient).  Ignored / invalid rows get zeros.
// A target outside [0, C) that is not ignore_index (or a gather index outside [0, M)) contributes nothing and sets *bad.
#include "stin_common.h"

namespace {

constexpr int SEG_BLOCK = 256;                 // targets per block (one per lane)
constexpr int SEG_STAGE_FLOATS = 8192;         // 32 KB LDS staging tile of logits rows

__host__ __device__ inline int seg_stride(int C) { return C | 1; }                  // odd LDS row stride
__host__ __device__ inline int seg_rows_per_pass(int C) {
    const int p = SEG_STAGE_FLOATS / seg_stride(C);
    return p < SEG_BLOCK ? p : SEG_BLOCK;
}

// Stage rows [r0, r0 + nr) of the logits (row stride ld) into LDS rows of stride S: consecutive lanes read consecutive floats.
__device__ inline void seg_stage(const float* __restrict__ logits, int64_t ld, int64_t r0, int nr, int C, int S,
                                 float* __restrict__ tile) {
    const int n = nr * C;
    const int dr = SEG_BLOCK / C, dc = SEG_BLOCK % C;
    int r = threadIdx.x / C, c = threadIdx.x % C;
    for (int e = threadIdx.x; e < n; e += SEG_BLOCK) {
        tile[r * S + c] = logits[(r0 + r) * ld + c];
        r += dr;
        c += dc;
        if (c >= C) {
            c -= C;
            ++r;
        }
    }
}

// max and first arg-max of a row; a NaN is maximal and the first NaN wins (torch.max over a dim)
__device__ inline void seg_argmax(const float* __restrict__ z, int C, float& m, int& am) {
    m = z[0];
    am = 0;
    if (m != m) return;
    for (int c = 1; c < C; ++c) {
        const float v = z[c];
        if (v != v) {
            m = v;
            am = c;
            return;
        }
        if (v > m) {
            m = v;
            am = c;
        }
    }
}

template <bool WANT_LOSS, bool WANT_CONF, bool HAS_ROWS>
__global__ __launch_bounds__(SEG_BLOCK) void k_seg_ce_fwd(const float* __restrict__ logits, int64_t ld, int64_t M,
                                                          const int64_t* __restrict__ rows, const int64_t* __restrict__ target,
                                                          int64_t N, int C, const float* __restrict__ weight, int64_t ignore_index,
                                                          double* __restrict__ partial, unsigned long long* __restrict__ conf,
                                                          int32_t* __restrict__ bad) {
    extern __shared__ float seg_lds[];
    int* hist = reinterpret_cast<int*>(seg_lds);                        // [C][C] when WANT_CONF
    float* tile = seg_lds + (WANT_CONF ? C * C : 0);                    // [P][S] when !HAS_ROWS
    __shared__ double red[2][SEG_BLOCK / STIN_WAVE];
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * SEG_BLOCK;
    const int nrows = (int)((N - row0) < SEG_BLOCK ? (N - row0) : SEG_BLOCK);
    if (WANT_CONF) {
        for (int k = t; k < C * C; k += SEG_BLOCK) hist[k] = 0;
    }
    double num = 0.0, den = 0.0;
    bool flag = false;

    // one target: -> loss / histogram contributions of this lane
    auto visit = [&](const float* z, int64_t y) {
        const bool ignored = WANT_LOSS && (y == ignore_index);          // (a matrix-only launch flags every invalid target)
        const bool valid = (y >= 0 && y < C);
        if (!ignored && !valid) {
            flag = true;
            return;
        }
        if (!WANT_CONF && ignored) return;
        float m;
        int am;
        seg_argmax(z, C, m, am);
        if (WANT_CONF && valid) atomicAdd(&hist[(int)y * C + am], 1);
        if (WANT_LOSS && !ignored) {
            float s = 0.f;
            for (int c = 0; c < C; ++c) s += expf(z[c] - m);
            const float nll = (m - z[y]) + logf(s);
            const double w = weight != nullptr ? (double)weight[y] : 1.0;
            num += w * (double)nll;
            den += w;
        }
    };

    if (HAS_ROWS) {
        if (WANT_CONF) __syncthreads();
        if (t < nrows) {
            const int64_t i = row0 + t;
            const int64_t r = rows[i];
            if (r < 0 || r >= M) flag = true;
            else visit(logits + r * ld, target[i]);
        }
    } else {
        const int S = seg_stride(C), P = seg_rows_per_pass(C);
        for (int p0 = 0; p0 < nrows; p0 += P) {
            const int nr = (nrows - p0) < P ? (nrows - p0) : P;
            __syncthreads();                                            // previous pass done with the tile (and hist zeroed)
            seg_stage(logits, ld, row0 + p0, nr, C, S, tile);
            __syncthreads();
            if (t < nr) visit(tile + t * S, target[row0 + p0 + t]);
        }
    }
    if (flag && bad != nullptr) *bad = 1;
    if (WANT_CONF) {
        __syncthreads();
        for (int k = t; k < C * C; k += SEG_BLOCK) {
            const int v = hist[k];
            if (v != 0) atomicAdd(conf + k, (unsigned long long)v);
        }
    }
    if (WANT_LOSS) {
        num = stin_wave_sum(num);
        den = stin_wave_sum(den);
        const int w = t / STIN_WAVE;
        if (t % STIN_WAVE == 0) {
            red[0][w] = num;
            red[1][w] = den;
        }
        __syncthreads();
        if (t == 0) {
            double a = 0.0, b = 0.0;
            for (int k = 0; k < SEG_BLOCK / STIN_WAVE; ++k) {
                a += red[0][k];
                b += red[1][k];
            }
            partial[2 * (int64_t)blockIdx.x] = a;
            partial[2 * (int64_t)blockIdx.x + 1] = b;
        }
    }
}

// fixed-order sum of the block partials: loss = sum w nll / sum w (fp32), den = sum w (fp64, read by the backward)
__global__ __launch_bounds__(SEG_BLOCK) void k_seg_ce_final(const double* __restrict__ partial, int64_t blocks,
                                                            float* __restrict__ loss, double* __restrict__ den_out) {
    __shared__ double red[2][SEG_BLOCK / STIN_WAVE];
    double a = 0.0, b = 0.0;
    for (int64_t k = threadIdx.x; k < blocks; k += SEG_BLOCK) {
        a += partial[2 * k];
        b += partial[2 * k + 1];
    }
    a = stin_wave_sum(a);
    b = stin_wave_sum(b);
    const int w = threadIdx.x / STIN_WAVE;
    if (threadIdx.x % STIN_WAVE == 0) {
        red[0][w] = a;
        red[1][w] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sa = 0.0, sb = 0.0;
        for (int k = 0; k < SEG_BLOCK / STIN_WAVE; ++k) {
            sa += red[0][k];
            sb += red[1][k];
        }
        loss[0] = (float)(sa / sb);                                     // 0 / 0 = NaN for an all-ignored batch (as torch)
        den_out[0] = sb;
    }
}

__global__ __launch_bounds__(SEG_BLOCK) void k_seg_ce_bwd(const float* __restrict__ logits, int64_t ld,
                                                          const int64_t* __restrict__ target, int64_t N, int C,
                                                          const float* __restrict__ weight, int64_t ignore_index,
                                                          const float* __restrict__ grad_loss, const double* __restrict__ den,
                                                          float* __restrict__ dlogits, int64_t ldd) {
    extern __shared__ float seg_lds[];
    __shared__ float rscale[SEG_BLOCK], rinv[SEG_BLOCK];
    __shared__ int ry[SEG_BLOCK];
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * SEG_BLOCK;
    const int nrows = (int)((N - row0) < SEG_BLOCK ? (N - row0) : SEG_BLOCK);
    const int S = seg_stride(C), P = seg_rows_per_pass(C);
    const double gd = (double)grad_loss[0] / den[0];
    for (int p0 = 0; p0 < nrows; p0 += P) {
        const int nr = (nrows - p0) < P ? (nrows - p0) : P;
        __syncthreads();
        seg_stage(logits, ld, row0 + p0, nr, C, S, seg_lds);
        __syncthreads();
        if (t < nr) {                                                   // the lane's row: softmax numerators in place, 1 / sum
            float* z = seg_lds + t * S;
            const int64_t y = target[row0 + p0 + t];
            const bool live = (y != ignore_index && y >= 0 && y < C);
            float m;
            int am;
            seg_argmax(z, C, m, am);
            float s = 0.f;
            for (int c = 0; c < C; ++c) {
                const float e = expf(z[c] - m);
                z[c] = e;
                s += e;
            }
            rinv[t] = 1.f / s;
            rscale[t] = live ? (float)(gd * (weight != nullptr ? (double)weight[y] : 1.0)) : 0.f;
            ry[t] = live ? (int)y : -1;
        }
        __syncthreads();
        const int n = nr * C;                                           // coalesced stores of the tile's gradient rows
        const int dr = SEG_BLOCK / C, dc = SEG_BLOCK % C;
        int r = t / C, c = t % C;
        for (int e = t; e < n; e += SEG_BLOCK) {
            const float sc = rscale[r];
            const float v = sc == 0.f ? 0.f : sc * (seg_lds[r * S + c] * rinv[r] - (c == ry[r] ? 1.f : 0.f));
            dlogits[(row0 + p0 + r) * ldd + c] = v;
            r += dr;
            c += dc;
            if (c >= C) {
                c -= C;
                ++r;
            }
        }
    }
}

template <bool L, bool F, bool R>
void seg_launch_fwd(int blocks, size_t lds, hipStream_t stream, const float* logits, int64_t ld, int64_t M, const int64_t* rows,
                    const int64_t* target, int64_t N, int C, const float* weight, int64_t ignore_index, double* partial,
                    unsigned long long* conf, int32_t* bad) {
    if (lds > 64 * 1024) {
        static stin_once_per_device raised;
        stin_raise_dynamic_lds(raised, (const void*)k_seg_ce_fwd<L, F, R>, 160 * 1024);
    }
    hipLaunchKernelGGL((k_seg_ce_fwd<L, F, R>), dim3((unsigned)blocks), dim3(SEG_BLOCK), lds, stream, logits, ld, M, rows, target, N,
                       C, weight, ignore_index, partial, conf, bad);
}

}  // namespace

extern "C" size_t stin_seg_ce_workspace_bytes(int64_t N) {
    if (N <= 0) return 0;
    return (size_t)((N + SEG_BLOCK - 1) / SEG_BLOCK) * 2 * sizeof(double) + 256;
}

extern "C" int stin_seg_ce_fwd_f32(const float* logits, int64_t ld, int64_t M, const int64_t* rows, const int64_t* target, int64_t N,
                                   int C, const float* weight, int64_t ignore_index, float* loss, double* den,
                                   int64_t* confusion, int32_t* bad, void* workspace, size_t workspace_bytes,
                                   stin_stream_t stream_) {
    stin_clear_stale_error();
    STIN_REQUIRE(N > 0 && M > 0 && C >= STIN_SEG_MIN_CLASSES && C <= STIN_SEG_MAX_CLASSES && ld >= C, STIN_E_SIZE);
    STIN_REQUIRE(rows != nullptr || M >= N, STIN_E_SIZE);
    STIN_REQUIRE(logits && target, STIN_E_NULL);
    STIN_REQUIRE(loss != nullptr || confusion != nullptr, STIN_E_NULL);
    const bool want_loss = loss != nullptr, want_conf = confusion != nullptr, has_rows = rows != nullptr;
    double* partial = nullptr;
    if (want_loss) {
        STIN_REQUIRE(den && workspace, STIN_E_NULL);
        STIN_REQUIRE(workspace_bytes >= stin_seg_ce_workspace_bytes(N), STIN_E_WORKSPACE);
        partial = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    }
    const int64_t blocks = (N + SEG_BLOCK - 1) / SEG_BLOCK;
    STIN_REQUIRE(blocks <= 0x7fffffff, STIN_E_SIZE);
    const size_t lds = (want_conf ? (size_t)C * C * sizeof(int) : 0) +
                       (has_rows ? 0 : (size_t)seg_rows_per_pass(C) * seg_stride(C) * sizeof(float));
    hipStream_t s = (hipStream_t)stream_;
    unsigned long long* conf = reinterpret_cast<unsigned long long*>(confusion);
    const int b = (int)blocks;
#define SEG_FWD(L_, F_, R_) seg_launch_fwd<L_, F_, R_>(b, lds, s, logits, ld, M, rows, target, N, C, weight, ignore_index, partial, conf, bad)
    if (want_loss && want_conf) {
        if (has_rows) SEG_FWD(true, true, true); else SEG_FWD(true, true, false);
    } else if (want_loss) {
        if (has_rows) SEG_FWD(true, false, true); else SEG_FWD(true, false, false);
    } else {
        if (has_rows) SEG_FWD(false, true, true); else SEG_FWD(false, true, false);
    }
#undef SEG_FWD
    if (want_loss) hipLaunchKernelGGL(k_seg_ce_final, dim3(1), dim3(SEG_BLOCK), 0, s, partial, blocks, loss, den);
    return stin_launch_status();
}

extern "C" int stin_seg_ce_bwd_f32(const float* logits, int64_t ld, const int64_t* target, int64_t N, int C, const float* weight,
                                   int64_t ignore_index, const float* grad_loss, const double* den, float* dlogits, int64_t ldd,
                                   stin_stream_t stream_) {
    stin_clear_stale_error();
    STIN_REQUIRE(N > 0 && C >= STIN_SEG_MIN_CLASSES && C <= STIN_SEG_MAX_CLASSES && ld >= C && ldd >= C, STIN_E_SIZE);
    STIN_REQUIRE(logits && target && grad_loss && den && dlogits, STIN_E_NULL);
    const int64_t blocks = (N + SEG_BLOCK - 1) / SEG_BLOCK;
    STIN_REQUIRE(blocks <= 0x7fffffff, STIN_E_SIZE);
    const size_t lds = (size_t)seg_rows_per_pass(C) * seg_stride(C) * sizeof(float);
    hipLaunchKernelGGL(k_seg_ce_bwd, dim3((unsigned)blocks), dim3(SEG_BLOCK), lds, (hipStream_t)stream_, logits, ld, target, N, C, weight,
                       ignore_index, grad_loss, den, dlogits, ldd);
    return stin_launch_status();
}
