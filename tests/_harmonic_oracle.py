"""CPU oracle of the harmonic fill (test helper): include/stin_hip.h, "Harmonic fill", restated in numpy from the header alone - the
reach fixed point, the row folds as a loop over the slot position (vectorised across rows), the 256-wide tile tree as a
reshape(-1, 256) with halving adds, Jacobi-preconditioned CG per channel with frozen channels, and the state table.  numpy rounds
every elementwise product and sum once (no contraction), which is the header's arithmetic.  Plus small graph builders."""
import struct

import numpy as np

MAX_C = 16
STATE_WORDS = 72
TILE = 256
ST_WEIGHT, ST_VALUE, ST_INDEX = 1, 2, 4
F_DONE, F_BREAK, F_NOTCONV = 1, 2, 4


def bits(x):
    return struct.unpack('<q', struct.pack('<d', float(x)))[0]


# ---------------------------------------------------------------------------------------------------------------------- graphs
def csr(edge_index, n):
    """Both directions of every column, every row in ascending neighbour id (preprocessing.harmonic_adjacency's order) ->
    (rowptr int32 [n + 1], col int32 [2E], src int64 [2E]: the column of edge_index a slot came from)."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    E = ei.shape[1]
    rows = np.concatenate([ei[0], ei[1]])
    cols = np.concatenate([ei[1], ei[0]])
    src = np.concatenate([np.arange(E), np.arange(E)])
    order = np.lexsort((cols, rows))
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rowptr, rows + 1, 1)
    return np.cumsum(rowptr).astype(np.int32), cols[order].astype(np.int32), src[order]


def slot_rows(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def inverse_length_weights(vertices, rowptr, col):
    """1.0 / sqrt((dx dx + dy dy) + dz dz) per slot, float32 vertices promoted first (the geodesic contract's edge length)."""
    V = np.asarray(vertices)[:, :3].astype(np.float64)
    d = V[slot_rows(rowptr)] - V[np.asarray(col, dtype=np.int64)]
    with np.errstate(all='ignore'):
        return 1.0 / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def path(n):
    return np.stack([np.arange(n - 1), np.arange(1, n)])


def grid4(nx, ny):
    """The 4-neighbour grid; vertex id = ix * ny + iy -> (xy float64 [nx ny, 2], edge_index)."""
    idx = np.arange(nx * ny).reshape(nx, ny)
    ei = np.concatenate([np.stack([idx[:-1].ravel(), idx[1:].ravel()]), np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()])], axis=1)
    gx, gy = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing='ij')
    return np.stack([gx.ravel(), gy.ravel()], axis=1), ei


def tri_grid(nx, ny, sx=1.0, sy=1.0, jitter=0.0, seed=0):
    """A triangulated grid (axis edges and one diagonal per cell), spacing (sx, sy), vertices moved by up to jitter * min spacing
    in x, y and z -> (V float64 [nx ny, 3], edge_index)."""
    rng = np.random.default_rng(seed)
    xy, ei = grid4(nx, ny)
    V = np.stack([xy[:, 0] * sx, xy[:, 1] * sy, np.zeros(nx * ny)], axis=1)
    V += rng.uniform(-jitter, jitter, V.shape) * min(sx, sy)
    idx = np.arange(nx * ny).reshape(nx, ny)
    diag = np.stack([idx[1:, :-1].ravel(), idx[:-1, 1:].ravel()])
    return V, np.concatenate([ei, diag], axis=1)


def icosphere(subdivisions=3):
    """-> (V float64 [10 4^s + 2, 3] on the unit sphere, edge_index [2, E] with every edge once)."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    V = [np.asarray(v, dtype=np.float64) for v in V]
    for _ in range(subdivisions):
        mid, F2 = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                mid[key] = len(V)
                V.append((V[a] + V[b]) / 2.0)
            return mid[key]

        for a, b, c in F:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            F2 += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = F2
    V = np.stack(V)
    V /= np.linalg.norm(V, axis=1, keepdims=True)
    e = set()
    for a, b, c in F:
        e |= {(min(a, b), max(a, b)), (min(b, c), max(b, c)), (min(c, a), max(c, a))}
    return V, np.asarray(sorted(e), dtype=np.int64).T


def hop_ball(rowptr, col, centre, radius):
    """Vertices within `radius` hops of `centre` -> bool [n]."""
    n = len(rowptr) - 1
    dist = np.full(n, -1)
    dist[centre] = 0
    frontier = [centre]
    for r in range(radius):
        nxt = []
        for v in frontier:
            for j in col[rowptr[v]:rowptr[v + 1]]:
                if dist[j] < 0:
                    dist[j] = r + 1
                    nxt.append(int(j))
        frontier = nxt
    return dist >= 0


# ----------------------------------------------------------------------------------------------------------------------- reach
def reach(rowptr, col, masked):
    """-> uint8 [n]: 0 known, 1 masked and never reached, 2 reached (the least fixed point, by whole sweeps)."""
    n = len(rowptr) - 1
    col = np.asarray(col, dtype=np.int64)
    flag = (np.asarray(masked).reshape(-1) != 0).astype(np.uint8)
    rows = slot_rows(rowptr)
    keep = rows != col                                                  # a slot with col == row is skipped everywhere
    rows, cols = rows[keep], col[keep]
    while True:
        hit = np.zeros(n, dtype=bool)
        ok = flag[cols] != 1
        hit[rows[ok]] = True
        new = hit & (flag == 1)
        if not new.any():
            return flag
        flag[new] = 2


# ---------------------------------------------------------------------------------------------------------------------- system
class System:
    """The unknowns (reached vertices, ascending id), d, b and the slots of the product, each fold laid out by slot position."""

    def __init__(self, rowptr, col, weight, values, flag):
        rowptr = np.asarray(rowptr, dtype=np.int64)
        col = np.asarray(col, dtype=np.int64)
        n = len(rowptr) - 1
        V = np.asarray(values, dtype=np.float32).astype(np.float64)
        self.C = V.shape[1]
        self.unk = np.nonzero(flag == 2)[0]
        self.nU = len(self.unk)
        inv = np.full(n, -1, dtype=np.int64)
        inv[self.unk] = np.arange(self.nU)
        w_all = np.ones(len(col)) if weight is None else np.asarray(weight, dtype=np.float64)
        beg, deg = rowptr[self.unk], rowptr[self.unk + 1] - rowptr[self.unk]
        self.d = np.zeros(self.nU)
        self.b = np.zeros((self.nU, self.C))
        self.steps = []                                                 # per slot position: (rows, weights, unknown neighbours)
        for pos in range(int(deg.max()) if self.nU else 0):
            rows = np.nonzero(deg > pos)[0]
            s = beg[rows] + pos
            j = col[s]
            live = j != self.unk[rows]
            rows, s, j = rows[live], s[live], j[live]
            w = w_all[s]
            if not np.all((w > 0) & (w < np.inf)):
                raise ValueError('a used weight is not finite or not positive')
            self.d[rows] = self.d[rows] + w
            known = flag[j] == 0
            if not np.all(np.isfinite(V[j[known]])):
                raise ValueError('a known value next to an unknown is not finite')
            self.b[rows[known]] = self.b[rows[known]] + w[known, None] * V[j[known]]
            unknown = flag[j] == 2
            self.steps.append((rows[unknown], w[unknown, None], inv[j[unknown]]))

    def acc(self, p):
        a = np.zeros_like(p)
        for rows, w, uj in self.steps:
            a[rows] = a[rows] + w * p[uj]
        return a

    def matvec(self, p):
        return self.d[:, None] * p - self.acc(p)


def tile_dot(a, b):
    """<a, b> per channel: [nU, C] x [nU, C] -> [C] by the header's tree."""
    nU, C = a.shape
    T = (nU + TILE - 1) // TILE
    s = np.zeros((T * TILE, C))
    s[:nU] = a * b
    s = s.reshape(T, TILE, C)
    h = TILE // 2
    while h >= 1:
        s[:, :h] = s[:, :h] + s[:, h:2 * h]
        h //= 2
    out = np.zeros(C)
    for t in range(T):
        out = out + s[t, 0]
    return out


def solve(rowptr, col, weight, values, masked, tol=1e-6, max_iterations=None, fill=0.0, trace=None):
    """-> (out float32 [N, C], state int64 [STATE_WORDS]).  trace: a list that receives (k, x.copy()) after every iteration."""
    values = np.asarray(values, dtype=np.float32)
    n, C = values.shape
    assert 1 <= C <= MAX_C
    flag = reach(rowptr, col, masked)
    S = System(rowptr, col, weight, values, flag)
    nU = S.nU
    tol2 = float(tol) * float(tol)
    budget = nU if max_iterations is None else int(max_iterations)
    d = S.d[:, None]
    x = np.zeros((nU, C))
    r = S.b.copy()
    with np.errstate(all='ignore'):
        z = r / d
        p = z.copy()
        rz = tile_dot(r, z)
        bb = tile_dot(S.b, S.b)
        rr = bb.copy()
        it = np.zeros(C, dtype=np.int64)
        done = bb == 0
        stopped = np.zeros(C, dtype=bool)
        for k in range(budget):
            a = ~(done | stopped)
            if not a.any():
                break
            q = S.matvec(p)
            pq = tile_dot(p, q)
            stopped |= a & ~(pq > 0)
            a &= ~stopped
            alpha = np.where(a, rz / np.where(a, pq, 1.0), 0.0)
            x[:, a] = x[:, a] + alpha[a] * p[:, a]
            r[:, a] = r[:, a] - alpha[a] * q[:, a]
            rr = np.where(a, tile_dot(r, r), rr)
            it[a] += 1
            done |= a & (rr <= tol2 * bb)
            a &= ~done
            z[:, a] = r[:, a] / d
            rzn = tile_dot(r, z)
            beta = np.where(a, rzn / np.where(a, rz, 1.0), 0.0)
            p[:, a] = z[:, a] + beta[a] * p[:, a]
            rz = np.where(a, rzn, rz)
            if trace is not None:
                trace.append((k, x.copy()))
        out = values.copy()
        out[flag == 1] = np.float32(fill)
        out[S.unk] = x.astype(np.float32)
    state = np.zeros(STATE_WORDS, dtype=np.int64)
    n_masked = int(np.count_nonzero(flag))
    state[1], state[2], state[4] = nU, n_masked - nU, n_masked
    for c in range(C):
        fl = (F_DONE if done[c] else 0) | (F_BREAK if stopped[c] else 0) | (0 if done[c] else F_NOTCONV)
        state[8 + 4 * c:12 + 4 * c] = [it[c], bits(rr[c]), bits(bb[c]), fl]
    return out, state


def dense_system(rowptr, col, weight, values, masked):
    """The same system written entry by entry -> (A [nU, nU], b [nU, C], unknown vertex ids), for np.linalg."""
    flag = reach(rowptr, col, masked)
    unk = np.nonzero(flag == 2)[0]
    inv = {int(v): u for u, v in enumerate(unk)}
    V = np.asarray(values, dtype=np.float64)
    A = np.zeros((len(unk), len(unk)))
    b = np.zeros((len(unk), V.shape[1]))
    for u, i in enumerate(unk):
        for s in range(rowptr[i], rowptr[i + 1]):
            j = int(col[s])
            if j == i:
                continue
            w = 1.0 if weight is None else float(weight[s])
            A[u, u] += w
            if flag[j] == 0:
                b[u] += w * V[j]
            else:
                A[u, inv[j]] -= w
    return A, b, unk
