// Mesh files: the body of a binary PLY file decoded on the device, and the per-face label vote of the Matterport scans.
// Contract: include/stin_hip.h ("Mesh files").
//
//   decode:  a workgroup owns RUN consecutive records = one contiguous byte range of the file.  It copies the 16-byte chunks
//            that cover the range into LDS (aligned uint4 loads; the last chunk of the buffer byte by byte when the buffer ends
//            inside it), then walks the items (record, column) of every output group with consecutive lanes on consecutive
//            destination elements: a dense group ([N, 3] positions, colours, normals; any single column) leaves in full lines.
//            A field is assembled from its LDS bytes one at a time, so no alignment of `first`, `stride` or an offset matters.
//   faces:   the same staging; one pass over the records checks the count field against K and every index against [0, N)
//            (an integer atomicOr of the flag, an integer atomicMin of the record id - only on an offending record), one pass
//            over the items (record, triangle, corner) writes the int64 triangles, quads as (0, 1, 2), (0, 2, 3).
//   vote:    int32 histogram [N, C] by integer atomicAdd (order-free), then one wave per vertex: lane c holds class c, the key
//            count * 64 + (63 - c) is maximised by butterfly shuffles - the highest count, ties to the lowest class.
#include <cstring>
#include "stin_common.h"

namespace {

constexpr int T = 256;
constexpr int RUN = 256;                       // records of a workgroup
typedef unsigned long long u64;

struct Field {
    unsigned char* dst;
    long long row_stride;                      // destination elements per record
    int col, offset;                           // destination column; byte offset of the source scalar in the record
    short src, to;                             // STIN_PLY_* source scalar, STIN_PLY_TO_* destination
    short group_size, pad;                     // on the first field of a group: its fields (a dense group: columns 0 .. size - 1
};                                             // of one destination in field order), 0 on the others
struct FieldTable {
    Field f[STIN_PLY_MAX_FIELDS];
    int n;
};

__host__ __device__ inline int src_width(int t) { return t < 2 ? 1 : t < 4 ? 2 : t < 7 ? 4 : 8; }
__host__ __device__ inline bool src_is_int(int t) { return t <= STIN_PLY_UINT32; }
inline int to_width(int t) { return t == STIN_PLY_TO_U8 ? 1 : (t == STIN_PLY_TO_F32 || t == STIN_PLY_TO_I32) ? 4 : 8; }

inline bool conversion_ok(int src, int to) {
    switch (to) {
        case STIN_PLY_TO_F64: return true;
        case STIN_PLY_TO_F32: return src == STIN_PLY_FLOAT32;
        case STIN_PLY_TO_I64: return src_is_int(src);
        case STIN_PLY_TO_I32: return src_is_int(src) && src != STIN_PLY_UINT32;
        case STIN_PLY_TO_U8:
        case STIN_PLY_TO_UNORM_F64: return src == STIN_PLY_UINT8;
    }
    return false;
}

// The bytes [begin, begin + bytes) of `body` -> LDS, chunk c of the run at lds[c]; the run starts `begin & 15` bytes into lds.
// Every address read lies inside [0, body_bytes): a chunk that would cross the end of the buffer is read byte by byte.
__device__ inline int stage_run(const uint8_t* __restrict__ body, int64_t body_bytes, int64_t begin, int64_t bytes, uint4* lds) {
    const int64_t a0 = begin & ~(int64_t)15;
    const int chunks = (int)((begin + bytes - a0 + 15) >> 4);
    for (int c = threadIdx.x; c < chunks; c += T) {
        const int64_t a = a0 + ((int64_t)c << 4);
        uint4 v;
        if (a + 16 <= body_bytes) {
            v = *reinterpret_cast<const uint4*>(body + a);
        } else {
            unsigned w[4] = {0u, 0u, 0u, 0u};
            for (int k = 0; k < 16 && a + k < body_bytes; ++k) w[k >> 2] |= (unsigned)body[a + k] << (8 * (k & 3));
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        lds[c] = v;
    }
    __syncthreads();
    return (int)(begin - a0);
}

// `width` bytes at p as an unsigned integer: the first byte is the lowest (little endian) or the highest (big endian)
__device__ inline u64 raw_bytes(const uint8_t* p, int width, int big_endian) {
    u64 r = 0;
    for (int b = 0; b < width; ++b) r |= (u64)p[big_endian ? width - 1 - b : b] << (8 * b);
    return r;
}

__device__ inline long long as_integer(u64 raw, int src) {
    switch (src) {
        case STIN_PLY_INT8: return (long long)(signed char)raw;
        case STIN_PLY_INT16: return (long long)(short)raw;
        case STIN_PLY_INT32: return (long long)(int)raw;
        default: return (long long)raw;                    // the unsigned types
    }
}

__device__ inline double as_double(u64 raw, int src) {
    if (src == STIN_PLY_FLOAT64) return __longlong_as_double((long long)raw);
    if (src == STIN_PLY_FLOAT32) return (double)__uint_as_float((unsigned)raw);
    return (double)as_integer(raw, src);                   // |value| < 2^32: exact
}

// ---------------------------------------------------------------------------------------------------------------------- decode
__global__ __launch_bounds__(T) void k_ply_decode(const uint8_t* __restrict__ body, int64_t body_bytes, int64_t first, int stride,
                                                  int64_t count, int big_endian, const FieldTable tab) {
    extern __shared__ uint4 lds[];
    const int64_t r0 = (int64_t)blockIdx.x * RUN;
    const int nrec = (int)(count - r0 < RUN ? count - r0 : RUN);
    const int lead = stage_run(body, body_bytes, first + r0 * stride, (int64_t)nrec * stride, lds);
    const uint8_t* rec0 = reinterpret_cast<const uint8_t*>(lds) + lead;
    for (int g = 0; g < tab.n; ++g) {
        const int S = tab.f[g].group_size;
        if (S == 0) continue;
        for (int j = threadIdx.x; j < nrec * S; j += T) {
            const int rec = j / S, c = j - rec * S;
            const Field& f = tab.f[g + c];
            const u64 raw = raw_bytes(rec0 + rec * stride + f.offset, src_width(f.src), big_endian);
            const int64_t at = (r0 + rec) * f.row_stride + f.col;
            switch (f.to) {
                case STIN_PLY_TO_F64: reinterpret_cast<double*>(f.dst)[at] = as_double(raw, f.src); break;
                case STIN_PLY_TO_F32: reinterpret_cast<unsigned*>(f.dst)[at] = (unsigned)raw; break;
                case STIN_PLY_TO_I64: reinterpret_cast<long long*>(f.dst)[at] = as_integer(raw, f.src); break;
                case STIN_PLY_TO_I32: reinterpret_cast<int*>(f.dst)[at] = (int)as_integer(raw, f.src); break;
                case STIN_PLY_TO_U8: f.dst[at] = (unsigned char)raw; break;
                default: reinterpret_cast<double*>(f.dst)[at] = (double)(unsigned char)raw / 255.0; break;      // _TO_UNORM_F64
            }
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------------- faces
__global__ void k_status_init(long long* __restrict__ status) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        status[0] = 0;
        status[1] = status[2] = 0x7fffffffffffffffll;
        status[3] = 0;
    }
}

template <int K>
__global__ __launch_bounds__(T) void k_ply_faces(const uint8_t* __restrict__ body, int64_t body_bytes, int64_t first, int stride,
                                                 int64_t count, int big_endian, int list_offset, int count_type, int index_type,
                                                 int64_t n_vertices, long long* __restrict__ faces, long long* __restrict__ status) {
    extern __shared__ uint4 lds[];
    const int64_t r0 = (int64_t)blockIdx.x * RUN;
    const int nrec = (int)(count - r0 < RUN ? count - r0 : RUN);
    const int lead = stage_run(body, body_bytes, first + r0 * stride, (int64_t)nrec * stride, lds);
    const uint8_t* rec0 = reinterpret_cast<const uint8_t*>(lds) + lead + list_offset;
    const int cw = src_width(count_type), iw = src_width(index_type);
    for (int rec = threadIdx.x; rec < nrec; rec += T) {
        const uint8_t* p = rec0 + rec * stride;
        if (as_integer(raw_bytes(p, cw, big_endian), count_type) != K) {
            atomicOr(reinterpret_cast<u64*>(status), (u64)STIN_PLY_COUNT_DIFFERS);
            atomicMin(reinterpret_cast<u64*>(status + 1), (u64)(r0 + rec));
            continue;
        }
        bool bad = false;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const long long v = as_integer(raw_bytes(p + cw + k * iw, iw, big_endian), index_type);
            bad = bad || v < 0 || v >= n_vertices;
        }
        if (bad) {
            atomicOr(reinterpret_cast<u64*>(status), (u64)STIN_PLY_BAD_INDEX);
            atomicMin(reinterpret_cast<u64*>(status + 2), (u64)(r0 + rec));
        }
    }
    constexpr int PER = 3 * (K - 2);                       // int64 words of a record's triangles
    for (int j = threadIdx.x; j < nrec * PER; j += T) {
        const int rec = j / PER, e = j - rec * PER;
        const int tri = e / 3, corner = e - tri * 3;
        const uint8_t* p = rec0 + rec * stride;
        long long v = -1;
        if (as_integer(raw_bytes(p, cw, big_endian), count_type) == K)
            v = as_integer(raw_bytes(p + cw + (corner == 0 ? 0 : tri + corner) * iw, iw, big_endian), index_type);
        faces[r0 * PER + j] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------------ vote
__global__ __launch_bounds__(T) void k_vote_count(const long long* __restrict__ faces, const long long* __restrict__ labels, int64_t F,
                                                  int64_t N, int C, int* __restrict__ hist, long long* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;         // (face, corner)
    if (i >= F * 3) return;
    const int64_t f = i / 3;
    const long long v = faces[i], l = labels[f];
    if (l < 0 || l >= C) {
        atomicOr(reinterpret_cast<u64*>(status), (u64)STIN_VOTE_BAD_LABEL);
        atomicMin(reinterpret_cast<u64*>(status + 1), (u64)f);
    } else if (v < 0 || v >= N) {
        atomicOr(reinterpret_cast<u64*>(status), (u64)STIN_VOTE_BAD_INDEX);
        atomicMin(reinterpret_cast<u64*>(status + 2), (u64)f);
    } else {
        atomicAdd(hist + v * C + l, 1);
    }
}

__global__ __launch_bounds__(T) void k_vote_argmax(const int* __restrict__ hist, int64_t N, int C, long long* __restrict__ out) {
    const int lane = threadIdx.x & (STIN_WAVE - 1);
    const int64_t v = (int64_t)blockIdx.x * (T / STIN_WAVE) + (threadIdx.x / STIN_WAVE);       // wave-uniform
    if (v >= N) return;
    long long key = lane < C ? (long long)hist[v * C + lane] * 64 + (63 - lane) : -1;
#pragma unroll
    for (int o = STIN_WAVE / 2; o > 0; o >>= 1) {
        const long long other = __shfl_xor(key, o, STIN_WAVE);
        key = other > key ? other : key;
    }
    if (lane == 0) out[v] = 63 - (key & 63);
}

inline size_t run_lds_bytes(int64_t stride) { return (size_t)RUN * (size_t)stride + 32; }

// first + count * stride <= body_bytes without overflow
inline bool range_ok(int64_t body_bytes, int64_t first, int64_t stride, int64_t count) {
    return body_bytes >= 0 && first >= 0 && first <= body_bytes && stride >= 1 && count >= 0 && count <= (body_bytes - first) / stride;
}

}  // namespace

extern "C" int stin_ply_decode(const uint8_t* body, int64_t body_bytes, int64_t first, int64_t stride, int64_t count, int big_endian,
                               const int64_t* fields, int n_fields, stin_stream_t stream_) {
    stin_clear_stale_error();
    hipStream_t stream = (hipStream_t)stream_;
    STIN_REQUIRE(stride >= 1 && stride <= STIN_PLY_MAX_STRIDE && count <= STIN_PLY_MAX_RECORDS, STIN_E_SIZE);
    STIN_REQUIRE(range_ok(body_bytes, first, stride, count), STIN_E_SIZE);
    STIN_REQUIRE(n_fields >= 0 && n_fields <= STIN_PLY_MAX_FIELDS && (big_endian == 0 || big_endian == 1), STIN_E_SIZE);
    STIN_REQUIRE(fields || n_fields == 0, STIN_E_NULL);
    FieldTable tab;
    memset(&tab, 0, sizeof(tab));
    tab.n = n_fields;
    for (int i = 0; i < n_fields; ++i) {
        const int64_t* w = fields + (int64_t)i * STIN_PLY_FIELD_WORDS;
        const int64_t offset = w[0], src = w[1], to = w[3], row_stride = w[4], col = w[5];
        STIN_REQUIRE(src >= STIN_PLY_INT8 && src <= STIN_PLY_FLOAT64 && to >= STIN_PLY_TO_F64 && to <= STIN_PLY_TO_UNORM_F64,
                     STIN_E_UNSUPPORTED);
        STIN_REQUIRE(conversion_ok((int)src, (int)to), STIN_E_UNSUPPORTED);
        STIN_REQUIRE(offset >= 0 && offset <= stride - src_width((int)src), STIN_E_SIZE);
        STIN_REQUIRE(row_stride >= 1 && row_stride <= STIN_PLY_MAX_FIELDS && col >= 0 && col < row_stride, STIN_E_SIZE);
        STIN_REQUIRE(w[2] != 0, STIN_E_NULL);
        STIN_REQUIRE((uint64_t)w[2] % (uint64_t)to_width((int)to) == 0, STIN_E_ALIGN);
        Field& f = tab.f[i];
        f.dst = reinterpret_cast<unsigned char*>((uintptr_t)w[2]);
        f.row_stride = row_stride;
        f.col = (int)col;
        f.offset = (int)offset;
        f.src = (short)src;
        f.to = (short)to;
    }
    // groups: `row_stride` consecutive fields that fill the columns 0 .. row_stride - 1 of one destination in order are written as
    // one dense matrix; any other field is a group of its own (and is written with its row stride)
    for (int i = 0; i < n_fields;) {
        const Field& a = tab.f[i];
        int S = 1;
        if (a.col == 0 && a.row_stride > 1 && i + a.row_stride <= n_fields) {
            bool dense = true;
            for (int c = 1; c < a.row_stride && dense; ++c) {
                const Field& b = tab.f[i + c];
                dense = b.dst == a.dst && b.to == a.to && b.row_stride == a.row_stride && b.col == c;
            }
            if (dense) S = (int)a.row_stride;
        }
        tab.f[i].group_size = (short)S;
        i += S;
    }
    if (count == 0 || n_fields == 0) return STIN_OK;
    STIN_REQUIRE(body, STIN_E_NULL);
    STIN_REQUIRE(stin_aligned16(body), STIN_E_ALIGN);
    hipLaunchKernelGGL(k_ply_decode, dim3((unsigned)((count + RUN - 1) / RUN)), dim3(T), run_lds_bytes(stride), stream, body, body_bytes,
                       first, (int)stride, count, big_endian, tab);
    return stin_launch_status();
}

extern "C" int stin_ply_faces(const uint8_t* body, int64_t body_bytes, int64_t first, int64_t stride, int64_t count, int big_endian,
                              int list_offset, int count_type, int index_type, int K, int64_t n_vertices, int64_t* faces,
                              int64_t* status, stin_stream_t stream_) {
    stin_clear_stale_error();
    hipStream_t stream = (hipStream_t)stream_;
    STIN_REQUIRE(stride >= 1 && stride <= STIN_PLY_MAX_STRIDE && count <= STIN_PLY_MAX_RECORDS, STIN_E_SIZE);
    STIN_REQUIRE(range_ok(body_bytes, first, stride, count), STIN_E_SIZE);
    STIN_REQUIRE((big_endian == 0 || big_endian == 1) && n_vertices >= 0, STIN_E_SIZE);
    STIN_REQUIRE(K == 3 || K == 4, STIN_E_UNSUPPORTED);
    STIN_REQUIRE(count_type >= STIN_PLY_INT8 && count_type <= STIN_PLY_UINT32 && index_type >= STIN_PLY_INT8 &&
                     index_type <= STIN_PLY_UINT32, STIN_E_UNSUPPORTED);
    STIN_REQUIRE(list_offset >= 0 && (int64_t)list_offset + src_width(count_type) + (int64_t)K * src_width(index_type) <= stride,
                 STIN_E_SIZE);
    STIN_REQUIRE(status, STIN_E_NULL);
    hipLaunchKernelGGL(k_status_init, dim3(1), dim3(64), 0, stream, reinterpret_cast<long long*>(status));
    if (count == 0) return stin_launch_status();
    STIN_REQUIRE(body && faces, STIN_E_NULL);
    STIN_REQUIRE(stin_aligned16(body), STIN_E_ALIGN);
    const dim3 grid((unsigned)((count + RUN - 1) / RUN));
    if (K == 3)
        hipLaunchKernelGGL(k_ply_faces<3>, grid, dim3(T), run_lds_bytes(stride), stream, body, body_bytes, first, (int)stride, count,
                           big_endian, list_offset, count_type, index_type, n_vertices, reinterpret_cast<long long*>(faces),
                           reinterpret_cast<long long*>(status));
    else
        hipLaunchKernelGGL(k_ply_faces<4>, grid, dim3(T), run_lds_bytes(stride), stream, body, body_bytes, first, (int)stride, count,
                           big_endian, list_offset, count_type, index_type, n_vertices, reinterpret_cast<long long*>(faces),
                           reinterpret_cast<long long*>(status));
    return stin_launch_status();
}

extern "C" size_t stin_face_label_vote_workspace_bytes(int64_t N, int C) {
    if (N < 0 || N > STIN_VOTE_MAX_VERTICES || C < 1 || C > STIN_VOTE_MAX_CLASSES) return 0;
    return stin_up256((size_t)(N > 0 ? N : 1) * (size_t)C * sizeof(int));
}

extern "C" int stin_face_label_vote(const int64_t* faces, const int64_t* face_labels, int64_t F, int64_t N, int C,
                                    int64_t* vertex_labels, int64_t* status, void* workspace, size_t workspace_bytes,
                                    stin_stream_t stream_) {
    stin_clear_stale_error();
    hipStream_t stream = (hipStream_t)stream_;
    STIN_REQUIRE(F >= 0 && F <= STIN_VOTE_MAX_FACES && N >= 0 && N <= STIN_VOTE_MAX_VERTICES, STIN_E_SIZE);
    STIN_REQUIRE(C >= 1 && C <= STIN_VOTE_MAX_CLASSES, STIN_E_UNSUPPORTED);
    STIN_REQUIRE(status, STIN_E_NULL);
    hipLaunchKernelGGL(k_status_init, dim3(1), dim3(64), 0, stream, reinterpret_cast<long long*>(status));
    if (N == 0 && F == 0) return stin_launch_status();
    STIN_REQUIRE(workspace && (vertex_labels || N == 0) && ((faces && face_labels) || F == 0), STIN_E_NULL);
    STIN_REQUIRE(workspace_bytes >= stin_face_label_vote_workspace_bytes(N, C), STIN_E_WORKSPACE);
    int* hist = reinterpret_cast<int*>(workspace);
    if (N > 0) {
        hipError_t e = hipMemsetAsync(hist, 0, (size_t)N * (size_t)C * sizeof(int), stream);
        if (e != hipSuccess) return (int)e;
    }
    if (F > 0)
        hipLaunchKernelGGL(k_vote_count, dim3((unsigned)((F * 3 + T - 1) / T)), dim3(T), 0, stream,
                           reinterpret_cast<const long long*>(faces), reinterpret_cast<const long long*>(face_labels), F, N, C, hist,
                           reinterpret_cast<long long*>(status));
    if (N > 0) {
        constexpr int PER = T / STIN_WAVE;
        hipLaunchKernelGGL(k_vote_argmax, dim3((unsigned)((N + PER - 1) / PER)), dim3(T), 0, stream, hist, N, C,
                           reinterpret_cast<long long*>(vertex_labels));
    }
    return stin_launch_status();
}
