"""numpy restatement of the QEM decimation contract (include/stin_hip.h, "QEM"; preprocessing.decimate_qem): the yardstick of
tests/test_qem.py and tests/test_qem_gpu.py.  Nothing exists to pin the decimator against bit for bit (the reference shells out to
vcglib's tridecimator), so the contract is restated here with the kernels' own expressions - explicit cofactors, every sum with its
association written out, fp64 - and the HIP path has to reproduce it exactly.

* `parallel`        the contract: rounds of independent collapses picked by two per-vertex minimum passes.
* `greedy`          the sequential decimator with the same quadrics, placement and validity rules: the single cheapest valid edge,
                    then everything again.  The quality yardstick.
* `error`           sum over the original vertices of h^T Q_v h at their image, Q_v from the original face quadrics only.
* `vertex_normals`  unit face normals summed per vertex in ascending face id, normalised, (0, 0, 1) for a zero sum.
* `icosphere`       a jittered closed test mesh.
"""
import numpy as np


class LevelError(ValueError):
    pass


# ------------------------------------------------------------------------------------------------------------------- arithmetic
def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def plane_quadric(w, u, d):
    """w p p^T, p = (u, d), as rows a00 a01 a02 a03 a11 a12 a13 a22 a23 a33."""
    x, y, z = u[..., 0], u[..., 1], u[..., 2]
    return np.stack([w * (x * x), w * (x * y), w * (x * z), w * (x * d), w * (y * y), w * (y * z), w * (y * d), w * (z * z), w * (z * d),
                     w * (d * d)], -1)


def quadric_cost(q, p):
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    r0 = ((q[..., 0] * x + q[..., 1] * y) + q[..., 2] * z) + q[..., 3]
    r1 = ((q[..., 1] * x + q[..., 4] * y) + q[..., 5] * z) + q[..., 6]
    r2 = ((q[..., 2] * x + q[..., 5] * y) + q[..., 7] * z) + q[..., 8]
    r3 = ((q[..., 3] * x + q[..., 6] * y) + q[..., 8] * z) + q[..., 9]
    return ((x * r0 + y * r1) + z * r2) + r3


def csr(keys, n):
    """rowptr [n + 1] of sorted keys in [0, n)."""
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(np.bincount(keys, minlength=n))
    return rp


def ordered_sum(rowptr, col, table, out):
    """out[v] += table[col[s]] for s in rowptr[v] .. rowptr[v + 1), one slot after the other."""
    deg = np.diff(rowptr)
    for k in range(int(deg.max(initial=0))):
        rows = np.flatnonzero(deg > k)
        out[rows] = out[rows] + table[col[rowptr[rows] + k]]
    return out


def face_normals_and_quadrics(V, F):
    v0 = V[F[:, 0]]
    n = cross3(V[F[:, 1]] - v0, V[F[:, 2]] - v0)
    length = np.sqrt(dot3(n, n))
    ok = length > 0.0
    with np.errstate(all='ignore'):
        u = np.where(ok[:, None], n / length[:, None], 0.0)
    K = np.where(ok[:, None], plane_quadric(0.5 * length, u, -dot3(u, v0)), 0.0)
    return u, K


def half_edges(F, n):
    """-> (unique keys i n + j of the undirected edges (i < j) in ascending order, faces per edge, the first face of each)."""
    a = np.concatenate([F[:, 0], F[:, 1], F[:, 2]])
    b = np.concatenate([F[:, 1], F[:, 2], F[:, 0]])
    keys = np.minimum(a, b) * n + np.maximum(a, b)
    order = np.argsort(keys, kind='stable')
    uniq, start, counts = np.unique(keys[order], return_index=True, return_counts=True)
    return uniq, counts.astype(np.int64), order[start] % max(F.shape[0], 1)


def drop_degenerate(F):
    keep = (F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 0] != F[:, 2])
    return F[keep]


def vertex_quadrics(V, F, boundary=True):
    n = V.shape[0]
    fn, Kf = face_normals_and_quadrics(V, F)
    flat = F.reshape(-1)
    order = np.argsort(flat, kind='stable')
    Q = ordered_sum(csr(flat[order], n), order // 3, Kf, np.zeros((n, 10)))
    if not boundary or F.shape[0] == 0:
        return Q
    keys, counts, first = half_edges(F, n)
    b = counts == 1
    bi, bj, bf = keys[b] // n, keys[b] % n, first[b]
    nb = bi.shape[0]
    if nb == 0:
        return Q
    a = V[bi]
    e = V[bj] - a
    m = cross3(e, fn[bf])
    length = np.sqrt(dot3(m, m))
    ok = length > 0.0
    with np.errstate(all='ignore'):
        u = np.where(ok[:, None], m / length[:, None], 0.0)
    Kb = np.where(ok[:, None], plane_quadric(dot3(e, e), u, -dot3(u, a)), 0.0)
    vkeys = np.concatenate([bi, bj]) * nb + np.concatenate([np.arange(nb), np.arange(nb)])
    vkeys.sort()
    return ordered_sum(csr(vkeys // nb, n), vkeys % nb, Kb, Q)


# -------------------------------------------------------------------------------------------------------------------- one round
def analyse(V, Q, F):
    """The candidate edges of the current mesh -> dict(ei, ej, x, cost, valid, nrp, ncol, neid)."""
    n = V.shape[0]
    keys, nf, _ = half_edges(F, n)
    ei, ej = keys // n, keys % n
    E = ei.shape[0]
    k2 = np.concatenate([ei * n + ej, ej * n + ei])
    order = np.argsort(k2, kind='stable')
    k2 = k2[order]
    nrp, ncol, neid = csr(k2 // n, n), k2 % n, order % max(E, 1)
    flat = F.reshape(-1)
    forder = np.argsort(flat, kind='stable')
    frp, fface = csr(flat[forder], n), forder // 3
    with np.errstate(all='ignore'):
        q = Q[ei] + Q[ej]
        vi, vj = V[ei], V[ej]
        mid = 0.5 * (vi + vj)
        c00, c01, c02 = q[:, 4] * q[:, 7] - q[:, 5] * q[:, 5], q[:, 2] * q[:, 5] - q[:, 1] * q[:, 7], q[:, 1] * q[:, 5] - q[:, 4] * q[:, 2]
        c11, c12, c22 = q[:, 0] * q[:, 7] - q[:, 2] * q[:, 2], q[:, 1] * q[:, 2] - q[:, 0] * q[:, 5], q[:, 0] * q[:, 4] - q[:, 1] * q[:, 1]
        det = (q[:, 0] * c00 + q[:, 1] * c01) + q[:, 2] * c02
        m = np.abs(q[:, 0])
        for k in (1, 2, 4, 5, 7):
            m = np.fmax(m, np.abs(q[:, k]))
        b0, b1, b2 = -q[:, 3], -q[:, 6], -q[:, 8]
        x = np.stack([((c00 * b0 + c01 * b1) + c02 * b2) / det, ((c01 * b0 + c11 * b1) + c12 * b2) / det,
                      ((c02 * b0 + c12 * b1) + c22 * b2) / det], -1)
        dm, dv = x - mid, vi - vj
        placed = (np.abs(det) > 1e-10 * ((m * m) * m)) & (np.sqrt(dot3(dm, dm)) <= np.sqrt(dot3(dv, dv)))
        h, c = vi.copy(), quadric_cost(q, vi)
        cj, cm = quadric_cost(q, vj), quadric_cost(q, mid)
        t = cj < c
        h[t], c[t] = vj[t], cj[t]
        t = cm < c
        h[t], c[t] = mid[t], cm[t]
        cx = quadric_cost(q, x)
        h[placed], c[placed] = x[placed], cx[placed]
    valid = np.isfinite(c) & (nf >= 1) & (nf <= 2)
    cost = np.where(c > 0.0, c, 0.0)
    # link condition: for every neighbour k of i, is (k, j) an edge?
    deg = np.diff(nrp)
    rep = np.repeat(np.arange(E), deg[ei])
    slot = np.arange(rep.shape[0]) - np.repeat(np.cumsum(deg[ei]) - deg[ei], deg[ei]) + nrp[ei][rep]
    k = ncol[slot]
    j = ej[rep]
    common = np.bincount(rep, weights=np.isin(np.minimum(k, j) * n + np.maximum(k, j), keys) & (k != j), minlength=E).astype(np.int64)
    valid &= common == nf
    # flip condition over the faces of both endpoints
    fdeg = np.diff(frp)
    for moved in (ei, ej):
        rep = np.repeat(np.arange(E), fdeg[moved])
        slot = np.arange(rep.shape[0]) - np.repeat(np.cumsum(fdeg[moved]) - fdeg[moved], fdeg[moved]) + frp[moved][rep]
        tri = F[fface[slot]]
        both = (tri == ei[rep, None]).any(1) & (tri == ej[rep, None]).any(1)
        P = V[tri]                                                             # [rows, 3 corners, 3]
        Pn = np.where((tri == moved[rep, None])[:, :, None], h[rep][:, None, :], P)
        with np.errstate(all='ignore'):
            n0 = cross3(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
            n1 = cross3(Pn[:, 1] - Pn[:, 0], Pn[:, 2] - Pn[:, 0])
            good = dot3(n0, n1) > 0.2 * (np.sqrt(dot3(n0, n0)) * np.sqrt(dot3(n1, n1)))
        bad = np.bincount(rep, weights=~good & ~both, minlength=E)
        valid &= bad == 0
    return dict(ei=ei, ej=ej, x=h, cost=cost, valid=valid, nrp=nrp, ncol=ncol, neid=neid)


def first_of(cost, a, b):
    """Elementwise the earlier of edge ids a, b (-1: none) in the order (cost, id)."""
    ca, cb = cost[np.maximum(a, 0)], cost[np.maximum(b, 0)]
    take_b = (b >= 0) & ((a < 0) | (cb < ca) | ((cb == ca) & (b < a)))
    return np.where(take_b, b, a)


def select(A, n):
    """The contract's selection: per-vertex minimum over the own valid edges, then over the closed one-ring."""
    cost, valid, nrp = A['cost'], A['valid'], A['nrp']
    deg = np.diff(nrp)
    m1 = np.full(n, -1, dtype=np.int64)
    for k in range(int(deg.max(initial=0))):
        rows = np.flatnonzero(deg > k)
        e = A['neid'][nrp[rows] + k]
        m1[rows] = first_of(cost, m1[rows], np.where(valid[e], e, -1))
    m2 = m1.copy()
    for k in range(int(deg.max(initial=0))):
        rows = np.flatnonzero(deg > k)
        m2[rows] = first_of(cost, m2[rows], m1[A['ncol'][nrp[rows] + k]])
    e = np.arange(cost.shape[0])
    return np.flatnonzero(valid & (m2[A['ei']] == e) & (m2[A['ej']] == e))


def target(n, percent=None, n_vertices=None):
    return int(n_vertices) if n_vertices is not None else max(3, n * int(percent) // 100)


def _decimate(vertices, faces, percent, n_vertices, strict, pick):
    V = np.array(vertices, dtype=np.float64)[:, :3].copy()
    F = np.array(faces, dtype=np.int64).reshape(-1, 3)
    n = V.shape[0]
    if F.size and (F.min() < 0 or F.max() >= n):
        raise IndexError('a face refers to a vertex outside [0, %d)' % n)
    F = drop_degenerate(F)
    n_target = target(n, percent, n_vertices)
    Q = vertex_quadrics(V, F)
    parent = np.arange(n)
    n_cur, rounds = n, 0
    while n_cur > n_target and F.shape[0]:
        A = analyse(V, Q, F)
        ids = pick(A, n)
        if ids.shape[0] == 0:
            break
        if ids.shape[0] > n_cur - n_target:
            ids = ids[np.argsort(A['cost'][ids], kind='stable')[:n_cur - n_target]]
        i, j = A['ei'][ids], A['ej'][ids]
        V[i] = A['x'][ids]
        Q[i] = Q[i] + Q[j]
        parent[j] = i
        F = drop_degenerate(parent[F])
        n_cur -= ids.shape[0]
        rounds += 1
    root = parent.copy()
    while not np.array_equal(root, root[root]):
        root = root[root]
    alive = parent == np.arange(n)
    rank = np.cumsum(alive) - 1
    if strict and n_cur > n_target:
        raise LevelError('%d vertices left, %d asked for' % (n_cur, n_target))
    return V[alive], rank[F], rank[root], int(n_cur), rounds


def parallel(vertices, faces, percent=None, n_vertices=None, strict=False):
    """-> (vertices' f64 [N', 3], faces' int64, trace int64 [N], N', rounds)."""
    return _decimate(vertices, faces, percent, n_vertices, strict, select)


def _cheapest(A, n):
    ids = np.flatnonzero(A['valid'])
    return ids[np.argsort(A['cost'][ids], kind='stable')[:1]]


def greedy(vertices, faces, percent=None, n_vertices=None, strict=False):
    """One collapse per step: the first valid edge in the order (cost, i, j)."""
    return _decimate(vertices, faces, percent, n_vertices, strict, _cheapest)


def error(V0, F0, V1, trace):
    V0 = np.asarray(V0, dtype=np.float64)
    Q = vertex_quadrics(V0, drop_degenerate(np.asarray(F0, dtype=np.int64)), boundary=False)
    return float(quadric_cost(Q, np.asarray(V1)[np.asarray(trace)]).sum())


def vertex_normals(vertices, faces):
    V = np.asarray(vertices, dtype=np.float64)[:, :3]
    F = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    fn, _ = face_normals_and_quadrics(V, F)
    flat = F.reshape(-1)
    order = np.argsort(flat, kind='stable')
    s = ordered_sum(csr(flat[order], V.shape[0]), order // 3, fn, np.zeros((V.shape[0], 3)))
    length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    ok = (length > 0.0) & np.isfinite(length)
    with np.errstate(all='ignore'):
        out = np.where(ok[:, None], s / length[:, None], np.array([0.0, 0.0, 1.0]))
    return out


# ----------------------------------------------------------------------------------------------------------------- test meshes
def icosphere(subdivisions=2, seed=0, jitter=0.03):
    """A closed, jittered icosphere: 12, 42, 162, 642 vertices for 0, 1, 2, 3 subdivisions."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    V = [np.asarray(v, dtype=np.float64) for v in V]
    for _ in range(subdivisions):
        mid, out = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                mid[k] = len(V)
                V.append((V[a] + V[b]) / 2)
            return mid[k]
        for a, b, c in F:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = out
    V = np.stack(V)
    V = V / np.linalg.norm(V, axis=1, keepdims=True)
    V = V + np.random.default_rng(seed).normal(0, jitter, V.shape)
    return V, np.asarray(F, dtype=np.int64)
