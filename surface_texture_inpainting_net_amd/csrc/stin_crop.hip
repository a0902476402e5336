// Training crops of a scene on the device (reference preprocessing/crop_training_samples.py `process_frame` :51-237): every crop of
// the sampling grid, every level, in one batched pass.  Contract: include/stin_hip.h ("training crops").
//
// A scene is described by a DEVICE table of segments; the crop index is a grid dimension (blockIdx.y), the segment another
// (blockIdx.z), the element of the segment the grid-strided x.  All flags of all (segment, crop, element) live in ONE flat byte
// array and ONE rocprim exclusive scan over it gives every new id, every per-crop count and every output offset at once: the
// output of a segment is the concatenation of its crops in crop order, element k of crop c at pos[base + c n + k] - pos[base].
//
//   mark:    k_inbox (vertex in the crop's closed fp64 box) -> k_mark_edges (edge flag = both endpoints in the box; keep flags of
//            its endpoints: plain stores of 1) -> k_mark_dilated (both endpoints kept; optional "occurs in this set" flags for the
//            reference's own relabelling).  The sweep is dense, (crop, edge): the flags it reads are one byte per vertex of ONE crop
//            (200 KB at 200 k vertices, cache resident), so the crops a vertex is not in cost one byte load each.
//   scan:    rocprim::exclusive_scan over the bytes (widened to int32 by an iterator), then k_bounds: the [segment][crop] table the
//            host reads once to size the outputs.
//   gather:  k_gather writes vertex rows, kept ids, relabelled edges and dilated sets in original order.
//   traces:  k_trace_direct relabels a kept fine vertex whose coarse target is kept, or appends it to the crop's query list (an
//            integer-atomic cursor: the ORDER of the list varies between runs, what is written for each query does not);
//            k_nearest: 16 queries of one crop per workgroup, 16 lanes per query, the crop's kept coarse positions streamed
//            through LDS as fp64 triples, running (best d^2, lowest index) in registers and a shuffle reduction over the lanes;
//            k_trace_hit / k_trace_miss count the coarse vertices left without a predecessor
//            (the host repairs those: rare and sequential).
//   labels:  integer histogram [N0, n_labels] of the original mesh's labels under traces[0] + row arg-max (lowest label on a tie).
#include <cstring>
#include <rocprim/rocprim.hpp>
#include "stin_common.h"

namespace {

constexpr int T = 256;
constexpr unsigned GX_CAP = 256;           // grid-x cap (grid-strided beyond it): y * z multiply it by crops * segments

struct widen_u8 {
    __device__ __host__ int32_t operator()(uint8_t f) const { return (int32_t)f; }
};
using flag_iter = rocprim::transform_iterator<const uint8_t*, widen_u8, int32_t>;

size_t scan_temp_bytes(int64_t n) {
    size_t bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, bytes, flag_iter((const uint8_t*)nullptr, widen_u8()), (int32_t*)nullptr, (int32_t)0,
                                  (size_t)(n > 0 ? n : 1), rocprim::plus<int32_t>(), (hipStream_t)0);
    return bytes;
}

inline dim3 grid_for(int64_t max_n, int n_crops, int n_segs) {
    int64_t gx = (max_n + T - 1) / T;
    if (gx < 1) gx = 1;
    if (gx > GX_CAP) gx = GX_CAP;
    return dim3((unsigned)gx, (unsigned)n_crops, (unsigned)n_segs);
}

// ---------------------------------------------------------------------------------------------------------------- mark
__global__ void k_inbox(const stin_crop_seg_t* __restrict__ segs, const double* __restrict__ boxes, uint8_t* __restrict__ inbox) {
    const stin_crop_seg_t s = segs[blockIdx.z];
    if (s.kind != STIN_CROP_VERTICES) return;
    const int64_t c = blockIdx.y;
    const double lox = boxes[4 * c], hix = boxes[4 * c + 1], loy = boxes[4 * c + 2], hiy = boxes[4 * c + 3];
    const float* v = (const float*)s.src;
    uint8_t* o = inbox + s.ibase + c * s.n;
    for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < s.n; i += (int64_t)gridDim.x * T) {
        const double x = (double)v[i * s.width], y = (double)v[i * s.width + 1], z = (double)v[i * s.width + 2];
        o[i] = (x >= lox && x <= hix && y >= loy && y <= hiy && z == z) ? 1 : 0;      // z is unbounded; a NaN fails every comparison
    }
}

__global__ void k_mark_edges(const stin_crop_seg_t* __restrict__ segs, const uint8_t* __restrict__ inbox, uint8_t* __restrict__ flags,
                             int32_t* __restrict__ status) {
    const stin_crop_seg_t s = segs[blockIdx.z];
    if (s.kind != STIN_CROP_EDGES) return;
    const stin_crop_seg_t vs = segs[s.vseg];
    const int64_t c = blockIdx.y, N = vs.n;
    const int64_t* e = (const int64_t*)s.src;
    const uint8_t* in = inbox + vs.ibase + c * N;
    uint8_t* keep = flags + vs.base + c * N;
    uint8_t* ef = flags + s.base + c * s.n;
    for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < s.n; i += (int64_t)gridDim.x * T) {
        const int64_t a = e[2 * i], b = e[2 * i + 1];
        if (a < 0 || a >= N || b < 0 || b >= N) {
            status[0] = 1;
            continue;                                              // (flags were zeroed: the edge is left out)
        }
        if (in[a] & in[b]) {
            ef[i] = 1;
            keep[a] = 1;
            keep[b] = 1;
        }
    }
}

__global__ void k_mark_dilated(const stin_crop_seg_t* __restrict__ segs, uint8_t* __restrict__ flags, int32_t* __restrict__ status) {
    const stin_crop_seg_t s = segs[blockIdx.z];
    if (s.kind != STIN_CROP_DILATED) return;
    const stin_crop_seg_t vs = segs[s.vseg];
    const int64_t c = blockIdx.y, N = vs.n;
    const int64_t* e = (const int64_t*)s.src;
    const uint8_t* keep = flags + vs.base + c * N;
    uint8_t* occ = s.aux >= 0 ? flags + segs[s.aux].base + c * N : nullptr;
    uint8_t* ef = flags + s.base + c * s.n;
    for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < s.n; i += (int64_t)gridDim.x * T) {
        const int64_t a = e[2 * i], b = e[2 * i + 1];
        if (a < 0 || a >= N || b < 0 || b >= N) {
            status[0] = 1;
            continue;
        }
        if (keep[a] & keep[b]) {
            ef[i] = 1;
            if (occ) {
                occ[a] = 1;
                occ[b] = 1;
            }
        }
    }
}

__global__ void k_bounds(const stin_crop_seg_t* __restrict__ segs, int n_segs, int n_crops, const int32_t* __restrict__ pos,
                         int64_t* __restrict__ bounds) {
    const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
    const int64_t per = n_crops + 1;
    if (i >= per * n_segs) return;
    const stin_crop_seg_t s = segs[i / per];
    bounds[i] = s.kind == STIN_CROP_TRACE ? 0 : (int64_t)pos[s.base + (i % per) * s.n];
}

// ---------------------------------------------------------------------------------------------------------------- gather
__global__ void k_gather(const stin_crop_seg_t* __restrict__ segs, const uint8_t* __restrict__ flags, const int32_t* __restrict__ pos) {
    const stin_crop_seg_t s = segs[blockIdx.z];
    if (s.kind == STIN_CROP_OCCURS || s.kind == STIN_CROP_TRACE || s.out == nullptr) return;
    const int64_t c = blockIdx.y;
    const int64_t sb = s.base + c * s.n;
    const int32_t p0 = pos[s.base];
    if (s.kind == STIN_CROP_VERTICES) {
        const float* src = (const float*)s.src;
        float* out = (float*)s.out;
        const int W = (int)s.width;
        const bool vec2 = (W % 2 == 0) && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(out)) & 7u) == 0;
        for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < s.n; i += (int64_t)gridDim.x * T) {
            if (!flags[sb + i]) continue;
            const int64_t o = pos[sb + i] - p0;
            if (vec2) {
                const float2* a = reinterpret_cast<const float2*>(src + i * W);
                float2* b = reinterpret_cast<float2*>(out + o * W);
                for (int k = 0; k < W / 2; ++k) b[k] = a[k];
            } else {
                for (int k = 0; k < W; ++k) out[o * W + k] = src[i * W + k];
            }
            if (s.ids_out) s.ids_out[o] = i;
        }
        return;
    }
    // edges / dilated sets: both endpoints through the new ids of the level (or of the set's own occurrence flags)
    const stin_crop_seg_t r = (s.kind == STIN_CROP_DILATED && s.aux >= 0) ? segs[s.aux] : segs[s.vseg];
    const int64_t rb = r.base + c * r.n;
    const int32_t r0 = pos[rb];
    const int64_t* e = (const int64_t*)s.src;
    longlong2* out = (longlong2*)s.out;
    for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < s.n; i += (int64_t)gridDim.x * T) {
        if (!flags[sb + i]) continue;
        const int64_t a = e[2 * i], b = e[2 * i + 1];              // in range: a flagged row passed the check of the mark pass
        out[pos[sb + i] - p0] = make_longlong2((long long)(pos[rb + a] - r0), (long long)(pos[rb + b] - r0));
    }
}

// ---------------------------------------------------------------------------------------------------------------- traces
struct TraceView {
    int64_t fb, gb;            // flag / pos index of the crop's first fine / coarse vertex
    int64_t foff, goff;        // first row of the crop in the fine / coarse flat outputs
    int64_t nf, nc;            // kept fine / coarse vertices of the crop
    int32_t* info;             // qcount, direct, miss, reserved
};
__device__ inline TraceView trace_view(const stin_crop_seg_t& s, const stin_crop_seg_t& f, const stin_crop_seg_t& g, int64_t c,
                                       int n_crops, const int32_t* pos, int32_t* info) {
    TraceView v;
    v.fb = f.base + c * f.n;
    v.gb = g.base + c * g.n;
    v.foff = pos[v.fb] - pos[f.base];
    v.goff = pos[v.gb] - pos[g.base];
    v.nf = pos[v.fb + f.n] - pos[v.fb];
    v.nc = pos[v.gb + g.n] - pos[v.gb];
    v.info = info + (s.ibase * n_crops + c) * 4;
    return v;
}

__global__ void k_trace_direct(const stin_crop_seg_t* __restrict__ segs, int n_crops, const uint8_t* __restrict__ flags,
                               const int32_t* __restrict__ pos, int32_t* __restrict__ info, int32_t* __restrict__ status) {
    const stin_crop_seg_t s = segs[blockIdx.z];
    if (s.kind != STIN_CROP_TRACE) return;
    const stin_crop_seg_t f = segs[s.vseg], g = segs[s.aux];
    const TraceView v = trace_view(s, f, g, blockIdx.y, n_crops, pos, info);
    const int64_t* trace = (const int64_t*)s.src;
    int64_t* out = (int64_t*)s.out;
    int32_t* qlist = (int32_t*)s.p0;
    const int32_t pf = pos[v.fb], pg = pos[v.gb];
    for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < f.n; i += (int64_t)gridDim.x * T) {
        if (!flags[v.fb + i]) continue;
        const int64_t lid = pos[v.fb + i] - pf;                   // new id of the fine vertex inside its crop
        const int64_t t = trace[i];
        if (t < 0 || t >= g.n) {
            status[0] = 1;
            out[v.foff + lid] = 0;
            continue;
        }
        if (flags[v.gb + t]) {
            out[v.foff + lid] = pos[v.gb + t] - pg;
            v.info[1] = 1;
        } else {
            const int q = atomicAdd(v.info, 1);                    // q < nf: the list has the crop's nf slots
            qlist[v.foff + q] = (int32_t)lid;
        }
    }
}

// Brute force on purpose: the queries are a crop's boundary vertices (a few hundred), the candidates its kept coarse vertices (a
// few thousand).  A workgroup takes QT = 16 queries of ONE crop; each query is served by NL = 16 lanes that share the candidates of
// every LDS tile between them (lane j takes candidates j, j + 16, ... in ascending order), so a tile read is 16 distinct fp64
// addresses per wave, broadcast to its four queries.  One thread per query walking all candidates was measured first: 0.8 ms for a
// single crop, three busy workgroups on the whole device.
constexpr int NL = 16, QT = T / NL;
__global__ void __launch_bounds__(T) k_nearest(const stin_crop_seg_t* __restrict__ segs, int n_crops, const int32_t* __restrict__ pos,
                                                 int32_t* __restrict__ info) {
    __shared__ double sx[T], sy[T], sz[T];
    const stin_crop_seg_t s = segs[blockIdx.z];
    if (s.kind != STIN_CROP_TRACE) return;
    const stin_crop_seg_t f = segs[s.vseg], g = segs[s.aux];
    const TraceView v = trace_view(s, f, g, blockIdx.y, n_crops, pos, info);
    const int64_t nq = v.info[0];
    const float* fv = (const float*)f.out + v.foff * f.width;
    const float* cv = (const float*)g.out + v.goff * g.width;
    const int32_t* qlist = (const int32_t*)s.p0 + v.foff;
    int64_t* out = (int64_t*)s.out + v.foff;
    const int t = threadIdx.x, j = t % NL, qi = t / NL;
    for (int64_t q0 = (int64_t)blockIdx.x * QT; q0 < nq; q0 += (int64_t)gridDim.x * QT) {     // uniform over the workgroup
        const bool active = q0 + qi < nq;
        const int64_t lid = active ? qlist[q0 + qi] : 0;
        double px = 0, py = 0, pz = 0;
        if (active) {
            px = (double)fv[lid * f.width];
            py = (double)fv[lid * f.width + 1];
            pz = (double)fv[lid * f.width + 2];
        }
        double best = __builtin_huge_val();
        int bi = INT32_MAX;
        for (int64_t t0 = 0; t0 < v.nc; t0 += T) {
            __syncthreads();
            if (t0 + t < v.nc) {
                const float* p = cv + (t0 + t) * g.width;
                sx[t] = (double)p[0];
                sy[t] = (double)p[1];
                sz[t] = (double)p[2];
            }
            __syncthreads();
            const int m = (int)(v.nc - t0 < T ? v.nc - t0 : T);
            for (int k = j; k < m; k += NL) {
                const double dx = px - sx[k], dy = py - sy[k], dz = pz - sz[k];
                const double d = (dx * dx + dy * dy) + dz * dz;    // -ffp-contract=off: no fused multiply-add
                if (d < best) {                                    // ascending index, strict: this lane's lowest index wins a tie
                    best = d;
                    bi = (int)(t0 + k);
                }
            }
        }
        for (int o = NL / 2; o > 0; o >>= 1) {                     // across the query's lanes: smaller distance, then lower index
            const double od = __shfl_xor(best, o, NL);
            const int oi = __shfl_xor(bi, o, NL);
            if (od < best || (od == best && oi < bi)) {
                best = od;
                bi = oi;
            }
        }
        if (active && j == 0) out[lid] = bi == INT32_MAX ? 0 : bi;
    }
}

__global__ void k_trace_hit(const stin_crop_seg_t* __restrict__ segs, int n_crops, const int32_t* __restrict__ pos,
                            int32_t* __restrict__ info) {
    const stin_crop_seg_t s = segs[blockIdx.z];
    if (s.kind != STIN_CROP_TRACE) return;
    const stin_crop_seg_t f = segs[s.vseg], g = segs[s.aux];
    const TraceView v = trace_view(s, f, g, blockIdx.y, n_crops, pos, info);
    const int64_t* out = (const int64_t*)s.out + v.foff;
    uint8_t* hit = (uint8_t*)s.p1 + v.goff;
    for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < v.nf; i += (int64_t)gridDim.x * T) {
        const int64_t t = out[i];
        if (t >= 0 && t < v.nc) hit[t] = 1;
    }
}

__global__ void k_trace_miss(const stin_crop_seg_t* __restrict__ segs, int n_crops, const int32_t* __restrict__ pos,
                             int32_t* __restrict__ info) {
    const stin_crop_seg_t s = segs[blockIdx.z];
    if (s.kind != STIN_CROP_TRACE) return;
    const stin_crop_seg_t f = segs[s.vseg], g = segs[s.aux];
    const TraceView v = trace_view(s, f, g, blockIdx.y, n_crops, pos, info);
    const uint8_t* hit = (const uint8_t*)s.p1 + v.goff;
    for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < v.nc; i += (int64_t)gridDim.x * T)
        if (!hit[i]) atomicAdd(v.info + 2, 1);
}

// ---------------------------------------------------------------------------------------------------------------- labels
__global__ void k_label_hist(const int64_t* __restrict__ trace0, const int64_t* __restrict__ labels, int64_t n_orig, int64_t n0,
                             int n_labels, int32_t* __restrict__ hist, int32_t* __restrict__ status) {
    for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < n_orig; i += (int64_t)gridDim.x * T) {
        const int64_t v = trace0[i], l = labels[i];
        if (v < 0 || v >= n0 || l < 0 || l >= n_labels) {
            status[0] = 1;
            continue;
        }
        atomicAdd(hist + v * n_labels + l, 1);
    }
}

__global__ void k_label_argmax(const int32_t* __restrict__ hist, int64_t n0, int n_labels, int64_t* __restrict__ out) {
    for (int64_t v = (int64_t)blockIdx.x * T + threadIdx.x; v < n0; v += (int64_t)gridDim.x * T) {
        const int32_t* h = hist + v * n_labels;
        int32_t best = h[0];
        int bl = 0;
        for (int l = 1; l < n_labels; ++l)
            if (h[l] > best) {                                     // strict: np.argmax's first (= lowest) label on a tie, 0 for an empty row
                best = h[l];
                bl = l;
            }
        out[v] = bl;
    }
}

inline unsigned flat_grid(int64_t n) {
    int64_t g = (n + T - 1) / T;
    if (g < 1) g = 1;
    if (g > 65536) g = 65536;
    return (unsigned)g;
}

bool table_ok(const void* segs, int n_segs, int64_t max_n, int n_crops) {
    return segs != nullptr && n_segs >= 1 && n_segs <= STIN_CROP_MAX_SEGS && n_crops >= 1 && n_crops <= STIN_CROP_MAX_CROPS && max_n >= 0;
}

}  // namespace

extern "C" size_t stin_crop_workspace_bytes(int64_t total) { return scan_temp_bytes(total + 1) + 256; }

extern "C" int stin_crop_mark(const stin_crop_seg_t* segs, int n_segs, int64_t max_n, const double* boxes, int n_crops, int64_t total,
                              int64_t inbox_total, uint8_t* inbox, uint8_t* flags, int32_t* pos, int64_t* bounds, int32_t* status,
                              void* workspace, size_t workspace_bytes, stin_stream_t stream_) {
    STIN_REQUIRE(boxes && inbox && flags && pos && bounds && status && workspace, STIN_E_NULL);
    STIN_REQUIRE(table_ok(segs, n_segs, max_n, n_crops) && total >= 0 && inbox_total >= 0, STIN_E_SIZE);
    STIN_REQUIRE(total + 1 < (int64_t)INT32_MAX, STIN_E_UNSUPPORTED);
    STIN_REQUIRE(workspace_bytes >= stin_crop_workspace_bytes(total), STIN_E_WORKSPACE);
    hipStream_t stream = (hipStream_t)stream_;
    stin_clear_stale_error();
    (void)hipMemsetAsync(flags, 0, (size_t)total + 1, stream);
    (void)hipMemsetAsync(status, 0, 2 * sizeof(int32_t), stream);
    const dim3 grid = grid_for(max_n, n_crops, n_segs);
    hipLaunchKernelGGL(k_inbox, grid, dim3(T), 0, stream, segs, boxes, inbox);
    hipLaunchKernelGGL(k_mark_edges, grid, dim3(T), 0, stream, segs, inbox, flags, status);
    hipLaunchKernelGGL(k_mark_dilated, grid, dim3(T), 0, stream, segs, flags, status);
    size_t tb = scan_temp_bytes(total + 1);
    const hipError_t e = rocprim::exclusive_scan(workspace, tb, flag_iter(flags, widen_u8()), pos, (int32_t)0, (size_t)(total + 1),
                                                 rocprim::plus<int32_t>(), stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_bounds, dim3(flat_grid((int64_t)n_segs * (n_crops + 1))), dim3(T), 0, stream, segs, n_segs, n_crops, pos, bounds);
    return stin_launch_status();
}

extern "C" int stin_crop_gather(const stin_crop_seg_t* segs, int n_segs, int64_t max_n, int n_crops, const uint8_t* flags,
                                const int32_t* pos, stin_stream_t stream_) {
    STIN_REQUIRE(flags && pos, STIN_E_NULL);
    STIN_REQUIRE(table_ok(segs, n_segs, max_n, n_crops), STIN_E_SIZE);
    stin_clear_stale_error();
    hipLaunchKernelGGL(k_gather, grid_for(max_n, n_crops, n_segs), dim3(T), 0, (hipStream_t)stream_, segs, flags, pos);
    return stin_launch_status();
}

extern "C" int stin_crop_traces(const stin_crop_seg_t* segs, int n_segs, int64_t max_n, int n_crops, const uint8_t* flags,
                                const int32_t* pos, int32_t* info, int32_t* status, stin_stream_t stream_) {
    STIN_REQUIRE(flags && pos && info && status, STIN_E_NULL);
    STIN_REQUIRE(table_ok(segs, n_segs, max_n, n_crops), STIN_E_SIZE);
    hipStream_t stream = (hipStream_t)stream_;
    stin_clear_stale_error();
    const dim3 grid = grid_for(max_n, n_crops, n_segs);
    dim3 near = grid;
    near.x = (unsigned)((max_n + QT - 1) / QT < 64 ? (max_n + QT - 1) / QT : 64);     // 16 queries per workgroup; hundreds per crop and level
    if (near.x < 1) near.x = 1;
    hipLaunchKernelGGL(k_trace_direct, grid, dim3(T), 0, stream, segs, n_crops, flags, pos, info, status + 1);
    hipLaunchKernelGGL(k_nearest, near, dim3(T), 0, stream, segs, n_crops, pos, info);
    hipLaunchKernelGGL(k_trace_hit, grid, dim3(T), 0, stream, segs, n_crops, pos, info);
    hipLaunchKernelGGL(k_trace_miss, grid, dim3(T), 0, stream, segs, n_crops, pos, info);
    return stin_launch_status();
}

extern "C" size_t stin_label_pool_workspace_bytes(int64_t n0, int n_labels) {
    return (size_t)(n0 > 0 ? n0 : 1) * (size_t)(n_labels > 0 ? n_labels : 1) * sizeof(int32_t);
}

extern "C" int stin_label_pool_i64(const int64_t* trace0, const int64_t* labels, int64_t n_orig, int64_t n0, int n_labels, int64_t* out,
                                   int32_t* status, void* workspace, size_t workspace_bytes, stin_stream_t stream_) {
    STIN_REQUIRE(out && status && workspace && (n_orig == 0 || (trace0 && labels)), STIN_E_NULL);
    STIN_REQUIRE(n_orig >= 0 && n0 >= 1 && n_labels >= 1, STIN_E_SIZE);
    STIN_REQUIRE(workspace_bytes >= stin_label_pool_workspace_bytes(n0, n_labels), STIN_E_WORKSPACE);
    hipStream_t stream = (hipStream_t)stream_;
    stin_clear_stale_error();
    int32_t* hist = (int32_t*)workspace;
    (void)hipMemsetAsync(hist, 0, (size_t)n0 * n_labels * sizeof(int32_t), stream);
    (void)hipMemsetAsync(status, 0, sizeof(int32_t), stream);
    if (n_orig > 0) hipLaunchKernelGGL(k_label_hist, dim3(flat_grid(n_orig)), dim3(T), 0, stream, trace0, labels, n_orig, n0, n_labels, hist, status);
    hipLaunchKernelGGL(k_label_argmax, dim3(flat_grid(n0)), dim3(T), 0, stream, hist, n0, n_labels, out);
    return stin_launch_status();
}
