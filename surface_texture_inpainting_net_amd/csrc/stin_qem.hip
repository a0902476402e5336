// Quadric-error-metric (QEM) edge-collapse decimation and vertex normals on the device.  Contract: include/stin_hip.h ("QEM").
//
// One decimation is a host loop of rounds (preprocessing.decimate_qem).  Per round the host builds, by sorting, the unique
// undirected edges (i < j) of the current faces ordered by (i, j), the sorted neighbour list of every vertex with the edge id of
// every slot, and the ascending face list of every vertex; the kernels of this file do everything else:
//   k_edges     one thread per edge: Q = Q_i + Q_j, placement by Cramer's rule or the cheapest of v_i, v_j, mid, the cost, the link
//               condition (two sorted neighbour lists walked with two cursors) and the flip condition (the faces of both
//               endpoints through the vertex -> face CSR).  Mesh degree is about 6: the loops are short and stay in registers.
//   k_min_edge / k_min_ring / k_select
//               the order of the valid edges is (cost, edge id) - the edge id IS the rank of (i, j).  Per vertex the minimum
//               over its own edges, then over its closed one-ring of those minima; an edge is selected when both endpoints name
//               it.  Two segmented minima over a CSR: no atomics, the same result on every run.
//   k_collapse  one thread per selected edge (no two share or neighbour an endpoint): v_i = x, Q_i += Q_j, parent[j] = i.
//   k_remap     one thread per face: range check, vertices through parent, keep flag = no repeated vertex (the host compacts).
//   k_trace     one thread per original vertex: follow parent to the survivor, trace = its rank.
// Quadrics: k_face_quadrics / k_boundary_quadrics fill one 10-entry row per face / boundary edge and k_vertex_sum adds the rows of
// every vertex in CSR order - a fixed-order segmented sum in fp64, no float atomics.  The same k_vertex_sum, three wide and with
// the normalising tail, gives the vertex normals.
// Arithmetic: fp64, every expression with its association written out and -ffp-contract=off, so that tests/_qem_oracle.py (numpy,
// the same expressions) agrees bit for bit.  A symmetric 4 x 4 quadric is the row q[10] = a00 a01 a02 a03 a11 a12 a13 a22 a23 a33.
// No kernel reads through an index it has not compared with the array's size.
#include "stin_common.h"

namespace {

constexpr int T = 256;

inline unsigned grid_1d(int64_t n) {
    int64_t g = (n + T - 1) / T;
    if (g < 1) g = 1;
    if (g > 8192) g = 8192;
    return (unsigned)g;
}

__device__ __forceinline__ bool inr(int64_t x, int64_t n) { return x >= 0 && x < n; }

struct d3 {
    double x, y, z;
};
__device__ __forceinline__ d3 ld3(const double* __restrict__ p, int64_t r) { return {p[3 * r], p[3 * r + 1], p[3 * r + 2]}; }
__device__ __forceinline__ d3 sub3(d3 a, d3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot3(d3 a, d3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ d3 cross3(d3 a, d3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// w p p^T as a 10-row, p = (u, d)
__device__ __forceinline__ void plane_quadric(double w, d3 u, double d, double* __restrict__ k) {
    k[0] = w * (u.x * u.x);
    k[1] = w * (u.x * u.y);
    k[2] = w * (u.x * u.z);
    k[3] = w * (u.x * d);
    k[4] = w * (u.y * u.y);
    k[5] = w * (u.y * u.z);
    k[6] = w * (u.y * d);
    k[7] = w * (u.z * u.z);
    k[8] = w * (u.z * d);
    k[9] = w * (d * d);
}

// h^T Q h, h = (p, 1)
__device__ __forceinline__ double quadric_cost(const double* q, d3 p) {
    const double r0 = ((q[0] * p.x + q[1] * p.y) + q[2] * p.z) + q[3];
    const double r1 = ((q[1] * p.x + q[4] * p.y) + q[5] * p.z) + q[6];
    const double r2 = ((q[2] * p.x + q[5] * p.y) + q[7] * p.z) + q[8];
    const double r3 = ((q[3] * p.x + q[6] * p.y) + q[8] * p.z) + q[9];
    return ((p.x * r0 + p.y * r1) + p.z * r2) + r3;
}

// ---------------------------------------------------------------------------------------------------------------- quadrics
// Kf[f] = area n n^T-quadric of face f (zero for a zero-area or out-of-range face), fn[f] = its unit normal (zero likewise).
__global__ void __launch_bounds__(T) k_face_quadrics(const double* __restrict__ V, int64_t N, const int64_t* __restrict__ faces,
                                                       int64_t F, double* __restrict__ Kf, double* __restrict__ fn) {
    for (int64_t f = (int64_t)blockIdx.x * T + threadIdx.x; f < F; f += (int64_t)gridDim.x * T) {
        const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        d3 u = {0.0, 0.0, 0.0};
        double k[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (inr(a, N) && inr(b, N) && inr(c, N)) {
            const d3 v0 = ld3(V, a);
            const d3 n = cross3(sub3(ld3(V, b), v0), sub3(ld3(V, c), v0));
            const double len = sqrt(dot3(n, n));
            if (len > 0.0) {
                u = {n.x / len, n.y / len, n.z / len};
                plane_quadric(0.5 * len, u, -dot3(u, v0), k);
            }
        }
        if (Kf != nullptr) {
#pragma unroll
            for (int t = 0; t < 10; ++t) Kf[10 * f + t] = k[t];
        }
        if (fn != nullptr) {
            fn[3 * f] = u.x;
            fn[3 * f + 1] = u.y;
            fn[3 * f + 2] = u.z;
        }
    }
}

// Kb[b] = |e|^2 q q^T of boundary edge (bi[b] < bj[b]) of face bface[b]: q the unit plane through the edge, perpendicular to the face.
__global__ void __launch_bounds__(T) k_boundary_quadrics(const double* __restrict__ V, int64_t N, const int64_t* __restrict__ bi,
                                                           const int64_t* __restrict__ bj, const int64_t* __restrict__ bface, int64_t B,
                                                           const double* __restrict__ fn, int64_t F, double* __restrict__ Kb) {
    for (int64_t b = (int64_t)blockIdx.x * T + threadIdx.x; b < B; b += (int64_t)gridDim.x * T) {
        const int64_t i = bi[b], j = bj[b], f = bface[b];
        double k[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (inr(i, N) && inr(j, N) && inr(f, F)) {
            const d3 a = ld3(V, i);
            const d3 e = sub3(ld3(V, j), a);
            const d3 m = cross3(e, ld3(fn, f));
            const double len = sqrt(dot3(m, m));
            if (len > 0.0) {
                const d3 u = {m.x / len, m.y / len, m.z / len};
                plane_quadric(dot3(e, e), u, -dot3(u, a), k);
            }
        }
#pragma unroll
        for (int t = 0; t < 10; ++t) Kb[10 * b + t] = k[t];
    }
}

// out[v] (+)= table[col[s]] for s = rowptr[v] .. rowptr[v + 1), in that order.  W <= 10 columns.  normalize (W == 3): the sum is
// divided by its length, a zero (or non-finite) length gives (0, 0, 1).
__global__ void __launch_bounds__(T) k_vertex_sum(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t nnz,
                                                    const double* __restrict__ table, int64_t n_items, int W, int64_t N,
                                                    double* __restrict__ out, int accumulate, int normalize) {
    for (int64_t v = (int64_t)blockIdx.x * T + threadIdx.x; v < N; v += (int64_t)gridDim.x * T) {
        double acc[10];
#pragma unroll
        for (int t = 0; t < 10; ++t) acc[t] = (accumulate && t < W) ? out[(int64_t)W * v + t] : 0.0;
        int64_t lo = rowptr[v], hi = rowptr[v + 1];
        if (lo < 0) lo = 0;
        if (hi > nnz) hi = nnz;
        for (int64_t s = lo; s < hi; ++s) {
            const int64_t it = col[s];
            if (!inr(it, n_items)) continue;
#pragma unroll
            for (int t = 0; t < 10; ++t)
                if (t < W) acc[t] += table[(int64_t)W * it + t];
        }
        if (normalize) {
            const double len = sqrt((acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2]);
            if (len > 0.0 && __builtin_isfinite(len)) {
                acc[0] = acc[0] / len;
                acc[1] = acc[1] / len;
                acc[2] = acc[2] / len;
            } else {
                acc[0] = 0.0;
                acc[1] = 0.0;
                acc[2] = 1.0;
            }
        }
#pragma unroll
        for (int t = 0; t < 10; ++t)
            if (t < W) out[(int64_t)W * v + t] = acc[t];
    }
}

// ------------------------------------------------------------------------------------------------------------ candidate edges
struct EdgeArgs {
    const double *V, *Q;
    int64_t N;
    const int64_t *ei, *ej, *nf;
    int64_t E;
    const int64_t *nrp, *ncol;      // neighbour CSR: rowptr [N + 1], sorted neighbour ids [nn]
    int64_t nn;
    const int64_t *frp, *fface;     // vertex -> face CSR: rowptr [N + 1], ascending face ids [nfs]
    int64_t nfs;
    const int64_t* faces;
    int64_t F;
    double *x, *cost;
    uint8_t* valid;
};

// Does moving vertex `moved` (one of i, j) of every face around it to x keep each face's normal within the bound?  Faces that hold
// both i and j vanish with the collapse and are skipped.
__device__ bool flips_ok(const EdgeArgs& A, int64_t moved, int64_t i, int64_t j, d3 x) {
    int64_t lo = A.frp[moved], hi = A.frp[moved + 1];
    if (lo < 0) lo = 0;
    if (hi > A.nfs) hi = A.nfs;
    for (int64_t s = lo; s < hi; ++s) {
        const int64_t f = A.fface[s];
        if (!inr(f, A.F)) return false;
        const int64_t a = A.faces[3 * f], b = A.faces[3 * f + 1], c = A.faces[3 * f + 2];
        if (!inr(a, A.N) || !inr(b, A.N) || !inr(c, A.N)) return false;
        const bool has_i = a == i || b == i || c == i, has_j = a == j || b == j || c == j;
        if (has_i && has_j) continue;
        const d3 pa = ld3(A.V, a), pb = ld3(A.V, b), pc = ld3(A.V, c);
        const d3 qa = (a == moved) ? x : pa, qb = (b == moved) ? x : pb, qc = (c == moved) ? x : pc;
        const d3 n0 = cross3(sub3(pb, pa), sub3(pc, pa));
        const d3 n1 = cross3(sub3(qb, qa), sub3(qc, qa));
        const double l0 = sqrt(dot3(n0, n0)), l1 = sqrt(dot3(n1, n1));
        if (!(dot3(n0, n1) > 0.2 * (l0 * l1))) return false;
    }
    return true;
}

__global__ void __launch_bounds__(T) k_edges(EdgeArgs A) {
    for (int64_t e = (int64_t)blockIdx.x * T + threadIdx.x; e < A.E; e += (int64_t)gridDim.x * T) {
        const int64_t i = A.ei[e], j = A.ej[e], faces_on_edge = A.nf[e];
        d3 h = {0.0, 0.0, 0.0};
        double cost = 0.0;
        bool ok = inr(i, A.N) && inr(j, A.N) && i != j;
        if (ok) {
            double q[10];
#pragma unroll
            for (int t = 0; t < 10; ++t) q[t] = A.Q[10 * i + t] + A.Q[10 * j + t];
            const d3 vi = ld3(A.V, i), vj = ld3(A.V, j);
            const d3 mid = {0.5 * (vi.x + vj.x), 0.5 * (vi.y + vj.y), 0.5 * (vi.z + vj.z)};
            // A x = b by cofactors: A = [[q0 q1 q2] [q1 q4 q5] [q2 q5 q7]], b = -(q3, q6, q8)
            const double c00 = q[4] * q[7] - q[5] * q[5], c01 = q[2] * q[5] - q[1] * q[7], c02 = q[1] * q[5] - q[4] * q[2];
            const double c11 = q[0] * q[7] - q[2] * q[2], c12 = q[1] * q[2] - q[0] * q[5], c22 = q[0] * q[4] - q[1] * q[1];
            const double det = (q[0] * c00 + q[1] * c01) + q[2] * c02;
            double m = fabs(q[0]);
            m = fmax(m, fabs(q[1]));
            m = fmax(m, fabs(q[2]));
            m = fmax(m, fabs(q[4]));
            m = fmax(m, fabs(q[5]));
            m = fmax(m, fabs(q[7]));
            bool placed = false;
            double c = 0.0;
            if (fabs(det) > 1e-10 * ((m * m) * m)) {
                const double b0 = -q[3], b1 = -q[6], b2 = -q[8];
                const d3 x = {((c00 * b0 + c01 * b1) + c02 * b2) / det, ((c01 * b0 + c11 * b1) + c12 * b2) / det,
                              ((c02 * b0 + c12 * b1) + c22 * b2) / det};
                const d3 dm = sub3(x, mid), dv = sub3(vi, vj);
                if (sqrt(dot3(dm, dm)) <= sqrt(dot3(dv, dv))) {
                    placed = true;
                    h = x;
                    c = quadric_cost(q, x);
                }
            }
            if (!placed) {                                        // the cheapest of v_i, v_j, mid; a tie goes to the earlier one
                h = vi;
                c = quadric_cost(q, vi);
                const double cj = quadric_cost(q, vj), cm = quadric_cost(q, mid);
                if (cj < c) {
                    h = vj;
                    c = cj;
                }
                if (cm < c) {
                    h = mid;
                    c = cm;
                }
            }
            ok = __builtin_isfinite(c) && faces_on_edge >= 1 && faces_on_edge <= 2;
            cost = c > 0.0 ? c : 0.0;
            if (ok) {                                             // link condition: common neighbours == faces on the edge
                int64_t p = A.nrp[i], pe = A.nrp[i + 1], r = A.nrp[j], re = A.nrp[j + 1];
                if (p < 0) p = 0;
                if (r < 0) r = 0;
                if (pe > A.nn) pe = A.nn;
                if (re > A.nn) re = A.nn;
                int64_t common = 0;
                while (p < pe && r < re) {
                    const int64_t a = A.ncol[p], b = A.ncol[r];
                    if (a == b) {
                        ++common;
                        ++p;
                        ++r;
                    } else if (a < b) {
                        ++p;
                    } else {
                        ++r;
                    }
                }
                ok = common == faces_on_edge;
            }
            if (ok) ok = flips_ok(A, i, i, j, h);
            if (ok) ok = flips_ok(A, j, i, j, h);
        }
        A.x[3 * e] = h.x;
        A.x[3 * e + 1] = h.y;
        A.x[3 * e + 2] = h.z;
        A.cost[e] = cost;
        A.valid[e] = ok ? 1 : 0;
    }
}

// --------------------------------------------------------------------------------------------------------------- selection
// a before b in the order (cost, edge id); b < 0: nothing yet
__device__ __forceinline__ bool before(const double* __restrict__ cost, int64_t a, int64_t b) {
    if (b < 0) return true;
    const double ca = cost[a], cb = cost[b];
    return ca < cb || (ca == cb && a < b);
}

// m1[v] = the first valid edge of vertex v in the order, -1: none.  neid[s] = the edge of neighbour slot s.
__global__ void __launch_bounds__(T) k_min_edge(const int64_t* __restrict__ nrp, const int64_t* __restrict__ neid, int64_t nn,
                                                  const double* __restrict__ cost, const uint8_t* __restrict__ valid, int64_t E,
                                                  int64_t N, int64_t* __restrict__ m1) {
    for (int64_t v = (int64_t)blockIdx.x * T + threadIdx.x; v < N; v += (int64_t)gridDim.x * T) {
        int64_t lo = nrp[v], hi = nrp[v + 1], best = -1;
        if (lo < 0) lo = 0;
        if (hi > nn) hi = nn;
        for (int64_t s = lo; s < hi; ++s) {
            const int64_t e = neid[s];
            if (inr(e, E) && valid[e] && before(cost, e, best)) best = e;
        }
        m1[v] = best;
    }
}

// m2[v] = the first of m1 over the closed one-ring of v
__global__ void __launch_bounds__(T) k_min_ring(const int64_t* __restrict__ nrp, const int64_t* __restrict__ ncol, int64_t nn,
                                                  const double* __restrict__ cost, const int64_t* __restrict__ m1, int64_t E, int64_t N,
                                                  int64_t* __restrict__ m2) {
    for (int64_t v = (int64_t)blockIdx.x * T + threadIdx.x; v < N; v += (int64_t)gridDim.x * T) {
        int64_t lo = nrp[v], hi = nrp[v + 1], best = m1[v];
        if (lo < 0) lo = 0;
        if (hi > nn) hi = nn;
        if (!inr(best, E)) best = -1;
        for (int64_t s = lo; s < hi; ++s) {
            const int64_t u = ncol[s];
            if (!inr(u, N)) continue;
            const int64_t e = m1[u];
            if (inr(e, E) && e != best && before(cost, e, best)) best = e;
        }
        m2[v] = best;
    }
}

__global__ void __launch_bounds__(T) k_select(const int64_t* __restrict__ ei, const int64_t* __restrict__ ej,
                                                const uint8_t* __restrict__ valid, const int64_t* __restrict__ m2, int64_t E, int64_t N,
                                                uint8_t* __restrict__ sel) {
    for (int64_t e = (int64_t)blockIdx.x * T + threadIdx.x; e < E; e += (int64_t)gridDim.x * T) {
        const int64_t i = ei[e], j = ej[e];
        sel[e] = (valid[e] && inr(i, N) && inr(j, N) && m2[i] == e && m2[j] == e) ? 1 : 0;
    }
}

// ----------------------------------------------------------------------------------------------------- collapse, remap, trace
__global__ void __launch_bounds__(T) k_collapse(const int64_t* __restrict__ ids, int64_t S, const int64_t* __restrict__ ei,
                                                  const int64_t* __restrict__ ej, int64_t E, const double* __restrict__ x,
                                                  double* __restrict__ V, double* __restrict__ Q, int64_t* __restrict__ parent,
                                                  int64_t N) {
    for (int64_t s = (int64_t)blockIdx.x * T + threadIdx.x; s < S; s += (int64_t)gridDim.x * T) {
        const int64_t e = ids[s];
        if (!inr(e, E)) continue;
        const int64_t i = ei[e], j = ej[e];
        if (!inr(i, N) || !inr(j, N) || i == j) continue;
        V[3 * i] = x[3 * e];
        V[3 * i + 1] = x[3 * e + 1];
        V[3 * i + 2] = x[3 * e + 2];
#pragma unroll
        for (int t = 0; t < 10; ++t) Q[10 * i + t] = Q[10 * i + t] + Q[10 * j + t];
        parent[j] = i;
    }
}

// faces (in place) through parent (NULL: as they are); keep[f] = in range and no repeated vertex; *status |= 1: out of range.
__global__ void __launch_bounds__(T) k_remap(int64_t* __restrict__ faces, int64_t F, const int64_t* __restrict__ parent, int64_t N,
                                               uint8_t* __restrict__ keep, int32_t* __restrict__ status) {
    for (int64_t f = (int64_t)blockIdx.x * T + threadIdx.x; f < F; f += (int64_t)gridDim.x * T) {
        int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        bool ok = inr(a, N) && inr(b, N) && inr(c, N);
        if (ok && parent != nullptr) {
            a = parent[a];
            b = parent[b];
            c = parent[c];
            ok = inr(a, N) && inr(b, N) && inr(c, N);
            if (ok) {
                faces[3 * f] = a;
                faces[3 * f + 1] = b;
                faces[3 * f + 2] = c;
            }
        }
        if (!ok) atomicOr(status, 1);
        keep[f] = (ok && a != b && b != c && a != c) ? 1 : 0;
    }
}

// trace[v] = rank[survivor of v]: parent followed until it points at itself.  *status |= 2: a chain that does not end.
__global__ void __launch_bounds__(T) k_trace(const int64_t* __restrict__ parent, const int64_t* __restrict__ rank, int64_t N,
                                               int64_t* __restrict__ trace, int32_t* __restrict__ status) {
    for (int64_t v = (int64_t)blockIdx.x * T + threadIdx.x; v < N; v += (int64_t)gridDim.x * T) {
        int64_t r = v, steps = 0;
        bool ok = true;
        for (;;) {
            const int64_t p = parent[r];
            if (!inr(p, N) || ++steps > N) {
                ok = false;
                break;
            }
            if (p == r) break;
            r = p;
        }
        if (!ok) atomicOr(status, 2);
        trace[v] = ok ? rank[r] : -1;
    }
}

}  // namespace

extern "C" int stin_qem_face_quadrics_f64(const double* vertices, int64_t N, const int64_t* faces, int64_t F, double* face_quadrics,
                                          double* face_normals, stin_stream_t stream) {
    STIN_REQUIRE(N >= 0 && F >= 0, STIN_E_SIZE);
    if (F == 0) return STIN_OK;
    STIN_REQUIRE(faces != nullptr && (N == 0 || vertices != nullptr), STIN_E_NULL);
    STIN_REQUIRE(face_quadrics != nullptr || face_normals != nullptr, STIN_E_NULL);
    stin_clear_stale_error();
    hipLaunchKernelGGL(k_face_quadrics, dim3(grid_1d(F)), dim3(T), 0, (hipStream_t)stream, vertices, N, faces, F, face_quadrics,
                       face_normals);
    return stin_launch_status();
}

extern "C" int stin_qem_boundary_quadrics_f64(const double* vertices, int64_t N, const int64_t* bi, const int64_t* bj,
                                              const int64_t* bface, int64_t B, const double* face_normals, int64_t F,
                                              double* boundary_quadrics, stin_stream_t stream) {
    STIN_REQUIRE(N >= 0 && F >= 0 && B >= 0, STIN_E_SIZE);
    if (B == 0) return STIN_OK;
    STIN_REQUIRE(vertices != nullptr && bi != nullptr && bj != nullptr && bface != nullptr && face_normals != nullptr &&
                     boundary_quadrics != nullptr, STIN_E_NULL);
    stin_clear_stale_error();
    hipLaunchKernelGGL(k_boundary_quadrics, dim3(grid_1d(B)), dim3(T), 0, (hipStream_t)stream, vertices, N, bi, bj, bface, B,
                       face_normals, F, boundary_quadrics);
    return stin_launch_status();
}

extern "C" int stin_qem_vertex_sum_f64(const int64_t* rowptr, const int64_t* col, int64_t nnz, const double* table, int64_t n_items,
                                       int width, int64_t N, double* out, int accumulate, int normalize, stin_stream_t stream) {
    STIN_REQUIRE(N >= 0 && nnz >= 0 && n_items >= 0, STIN_E_SIZE);
    STIN_REQUIRE(width >= 1 && width <= 10 && (!normalize || width == 3), STIN_E_SIZE);
    if (N == 0) return STIN_OK;
    STIN_REQUIRE(rowptr != nullptr && out != nullptr, STIN_E_NULL);
    STIN_REQUIRE(nnz == 0 || (col != nullptr && (n_items == 0 || table != nullptr)), STIN_E_NULL);
    stin_clear_stale_error();
    hipLaunchKernelGGL(k_vertex_sum, dim3(grid_1d(N)), dim3(T), 0, (hipStream_t)stream, rowptr, col, nnz, table, n_items, width, N, out,
                       accumulate, normalize);
    return stin_launch_status();
}

extern "C" int stin_qem_edges_f64(const double* vertices, const double* quadrics, int64_t N, const int64_t* ei, const int64_t* ej,
                                  const int64_t* faces_on_edge, int64_t E, const int64_t* nbr_rowptr, const int64_t* nbr_col,
                                  int64_t nbr_nnz, const int64_t* vf_rowptr, const int64_t* vf_face, int64_t vf_nnz,
                                  const int64_t* faces, int64_t F, double* x, double* cost, uint8_t* valid, stin_stream_t stream) {
    STIN_REQUIRE(N >= 0 && E >= 0 && F >= 0 && nbr_nnz >= 0 && vf_nnz >= 0, STIN_E_SIZE);
    if (E == 0) return STIN_OK;
    STIN_REQUIRE(vertices != nullptr && quadrics != nullptr && ei != nullptr && ej != nullptr && faces_on_edge != nullptr &&
                     nbr_rowptr != nullptr && vf_rowptr != nullptr && x != nullptr && cost != nullptr && valid != nullptr, STIN_E_NULL);
    STIN_REQUIRE(nbr_nnz == 0 || nbr_col != nullptr, STIN_E_NULL);
    STIN_REQUIRE(vf_nnz == 0 || (vf_face != nullptr && faces != nullptr), STIN_E_NULL);
    EdgeArgs A;
    A.V = vertices;
    A.Q = quadrics;
    A.N = N;
    A.ei = ei;
    A.ej = ej;
    A.nf = faces_on_edge;
    A.E = E;
    A.nrp = nbr_rowptr;
    A.ncol = nbr_col;
    A.nn = nbr_nnz;
    A.frp = vf_rowptr;
    A.fface = vf_face;
    A.nfs = vf_nnz;
    A.faces = faces;
    A.F = F;
    A.x = x;
    A.cost = cost;
    A.valid = valid;
    stin_clear_stale_error();
    hipLaunchKernelGGL(k_edges, dim3(grid_1d(E)), dim3(T), 0, (hipStream_t)stream, A);
    return stin_launch_status();
}

extern "C" int stin_qem_select_i64(const int64_t* ei, const int64_t* ej, int64_t E, const int64_t* nbr_rowptr, const int64_t* nbr_col,
                                   const int64_t* nbr_edge, int64_t nbr_nnz, const double* cost, const uint8_t* valid, int64_t N,
                                   int64_t* vertex_min, int64_t* ring_min, uint8_t* selected, stin_stream_t stream) {
    STIN_REQUIRE(N >= 0 && E >= 0 && nbr_nnz >= 0, STIN_E_SIZE);
    if (E == 0 || N == 0) return STIN_OK;
    STIN_REQUIRE(ei != nullptr && ej != nullptr && nbr_rowptr != nullptr && cost != nullptr && valid != nullptr &&
                     vertex_min != nullptr && ring_min != nullptr && selected != nullptr, STIN_E_NULL);
    STIN_REQUIRE(nbr_nnz == 0 || (nbr_col != nullptr && nbr_edge != nullptr), STIN_E_NULL);
    hipStream_t s = (hipStream_t)stream;
    stin_clear_stale_error();
    hipLaunchKernelGGL(k_min_edge, dim3(grid_1d(N)), dim3(T), 0, s, nbr_rowptr, nbr_edge, nbr_nnz, cost, valid, E, N, vertex_min);
    hipLaunchKernelGGL(k_min_ring, dim3(grid_1d(N)), dim3(T), 0, s, nbr_rowptr, nbr_col, nbr_nnz, cost, (const int64_t*)vertex_min, E, N,
                       ring_min);
    hipLaunchKernelGGL(k_select, dim3(grid_1d(E)), dim3(T), 0, s, ei, ej, valid, (const int64_t*)ring_min, E, N, selected);
    return stin_launch_status();
}

extern "C" int stin_qem_collapse_f64(const int64_t* edge_ids, int64_t S, const int64_t* ei, const int64_t* ej, int64_t E, const double* x,
                                     double* vertices, double* quadrics, int64_t* parent, int64_t N, stin_stream_t stream) {
    STIN_REQUIRE(N >= 0 && E >= 0 && S >= 0, STIN_E_SIZE);
    if (S == 0) return STIN_OK;
    STIN_REQUIRE(edge_ids != nullptr && ei != nullptr && ej != nullptr && x != nullptr && vertices != nullptr && quadrics != nullptr &&
                     parent != nullptr, STIN_E_NULL);
    stin_clear_stale_error();
    hipLaunchKernelGGL(k_collapse, dim3(grid_1d(S)), dim3(T), 0, (hipStream_t)stream, edge_ids, S, ei, ej, E, x, vertices, quadrics,
                       parent, N);
    return stin_launch_status();
}

extern "C" int stin_qem_remap_faces_i64(int64_t* faces, int64_t F, const int64_t* parent, int64_t N, uint8_t* keep, int32_t* status,
                                        stin_stream_t stream) {
    STIN_REQUIRE(N >= 0 && F >= 0, STIN_E_SIZE);
    if (F == 0) return STIN_OK;
    STIN_REQUIRE(faces != nullptr && keep != nullptr && status != nullptr, STIN_E_NULL);
    stin_clear_stale_error();
    hipLaunchKernelGGL(k_remap, dim3(grid_1d(F)), dim3(T), 0, (hipStream_t)stream, faces, F, parent, N, keep, status);
    return stin_launch_status();
}

extern "C" int stin_qem_trace_i64(const int64_t* parent, const int64_t* rank, int64_t N, int64_t* trace, int32_t* status,
                                  stin_stream_t stream) {
    STIN_REQUIRE(N >= 0, STIN_E_SIZE);
    if (N == 0) return STIN_OK;
    STIN_REQUIRE(parent != nullptr && rank != nullptr && trace != nullptr && status != nullptr, STIN_E_NULL);
    stin_clear_stale_error();
    hipLaunchKernelGGL(k_trace, dim3(grid_1d(N)), dim3(T), 0, (hipStream_t)stream, parent, rank, N, trace, status);
    return stin_launch_status();
}
