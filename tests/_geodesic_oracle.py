"""CPU oracle of the geodesic circle masks (test helper): include/stin_hip.h, "Geodesic distances", restated in numpy and pure
Python - explicit dx*dx + dy*dy + dz*dz edge lengths, heap Dijkstra on Python floats (fp64, one rounding per addition), the cap rule,
the mask rule and the circle_masks_geodesic loop on top of _surface_oracle.  A second, independent form of the distance -
Bellman-Ford sweeps to the fixed point - takes no heap and no order from the first.  The metric is Dijkstra's on the edge graph,
not the exact polyhedral geodesic."""
import heapq
import math

import numpy as np

import _mask_oracle as MO
import _surface_oracle as SO

INF = math.inf


def edge_lengths(vertices, edge_index):
    """-> float64 [E]: sqrt((dx dx + dy dy) + dz dz) of every column, float32 vertices promoted first."""
    V = np.asarray(vertices)[:, :3].astype(np.float64)
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    if ei.size and (ei.min() < 0 or ei.max() >= len(V)):
        raise IndexError('an edge refers to a vertex outside [0, %d)' % len(V))
    with np.errstate(all='ignore'):
        d = V[ei[0]] - V[ei[1]]
        sq = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        ln = np.sqrt(sq)
    if not np.all(np.isfinite(ln)):
        raise ValueError('the length of an edge is not finite')
    return ln


def weighted_adjacency(vertices, edge_index):
    """Per vertex the list of (neighbour, length) over both directions of every column; duplicates, self loops and zero lengths
    are kept."""
    n = len(vertices)
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    ln = edge_lengths(vertices, ei)
    adj = [[] for _ in range(n)]
    for (a, b), l in zip(ei.T.tolist(), ln.tolist()):
        adj[a].append((b, l))
        adj[b].append((a, l))
    return adj


def _checked_sources(sources, n):
    s = [int(x) for x in np.asarray(sources, dtype=np.int64).reshape(-1)]
    if any(x < 0 or x >= n for x in s):
        raise IndexError('a source lies outside [0, %d)' % n)
    return s


def _cut(D, cap):
    out = np.asarray(D, dtype=np.float64)
    out[~(out < cap)] = INF
    return out


def dijkstra(adj, sources, cap=INF):
    """Heap Dijkstra on Python floats: the path's length folded from the source outward; D where D < cap (strict), +inf elsewhere."""
    if not cap > 0.0:
        raise ValueError('cap must be > 0')
    n = len(adj)
    D = [INF] * n
    heap = []
    for s in _checked_sources(sources, n):
        if D[s] != 0.0:
            D[s] = 0.0
            heapq.heappush(heap, (0.0, s))
    while heap:
        d, u = heapq.heappop(heap)
        if d != D[u] or not d < cap:
            continue
        for w, l in adj[u]:
            nd = d + l
            if nd < D[w]:
                D[w] = nd
                heapq.heappush(heap, (nd, w))
    return _cut(D, cap)


def bellman_ford(adj, sources, cap=INF):
    """The fixed point D[s] = 0, D[v] = min_u fl(D[u] + len(u, v)) by whole sweeps in descending vertex id (in place) until a sweep
    changes nothing - no heap, no frontier; then the cap rule."""
    if not cap > 0.0:
        raise ValueError('cap must be > 0')
    n = len(adj)
    D = [INF] * n
    for s in _checked_sources(sources, n):
        D[s] = 0.0
    for _ in range(n + 1):
        changed = False
        for v in range(n - 1, -1, -1):
            best = D[v]
            for u, l in adj[v]:                                         # (the adjacency is symmetric: u -> v has the same length)
                nd = D[u] + l
                if nd < best:
                    best = nd
            if best < D[v]:
                D[v] = best
                changed = True
        if not changed:
            break
    else:
        raise AssertionError('no fixed point after n + 1 sweeps')
    return _cut(D, cap)


def mask_values(D, radius, rings):
    """mask = 0 where D >= radius, else min(rings, (int64) ceil((radius - D) / (radius / rings)))."""
    radius, rings = float(radius), int(rings)
    if not (radius > 0.0 and math.isfinite(radius)):
        raise ValueError('radius must be positive and finite')
    if rings < 1:
        raise ValueError('rings must be >= 1')
    ring = radius / rings
    D = np.asarray(D, dtype=np.float64)
    out = np.zeros(D.shape, dtype=np.int64)
    inside = D < radius
    out[inside] = np.minimum(rings, np.ceil((radius - D[inside]) / ring).astype(np.int64))
    return out


def circle_mask_from_centres(vertices, edge_index, centres, radius, rings=16, adj=None):
    adj = weighted_adjacency(vertices, edge_index) if adj is None else adj
    mask_values(0.0, radius, rings)                                     # the argument checks
    return mask_values(dijkstra(adj, centres, float(radius)), radius, rings)


def circle_masks_geodesic(vertices, faces, radius, frac, num_masks, seed, spacing, candidates, rings=16, max_iters=32, edge_index=None):
    """-> per mask a dict: mask, batches (list of centre arrays), sizes, counts, exhausted, capped - _surface_oracle's loop with the
    metric mask value."""
    V = np.asarray(vertices)[:, :3].astype(np.float64)
    n = len(V)
    adj = weighted_adjacency(V, SO.mesh_edges(faces) if edge_index is None else edge_index)
    out = []
    for m in range(num_masks):
        stream = SO.surface_centres(V, faces, candidates, SO.stream_seed(seed, m), spacing)
        mask = np.zeros(n, dtype=np.int64)
        pos, total, k, done, exhausted = 0, 0, 10, False, False
        batches, sizes, counts = [], [], []
        for _ in range(max_iters):
            take = stream[pos:pos + k]
            if len(take):
                np.maximum(mask, circle_mask_from_centres(V, None, take, radius, rings, adj=adj), out=mask)
            pos, total = pos + len(take), total + len(take)
            batches.append(take)
            sizes.append(len(take))
            counts.append(int(np.count_nonzero(mask)))
            if len(take) < k:
                exhausted = done = True
                break
            done, k = MO.next_batch_size(total, counts[-1], n, frac)
            if done:
                break
            k = min(k, n)
        out.append(dict(mask=mask, batches=batches, sizes=sizes, counts=counts, exhausted=exhausted, capped=not done))
    return out


# ------------------------------------------------------------------------------------------------------------------- the cases
def grid_mesh(nx, ny, sx=1.0, sy=1.0, jitter=0.0, seed=0):
    """A triangulated nx x ny grid (spacing sx, sy; vertices moved by up to jitter * min spacing, z included) -> (V, F)."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(nx) * sx, np.arange(ny) * sy, indexing='ij')
    V = np.stack([gx.ravel(), gy.ravel(), np.zeros(nx * ny)], axis=1)
    V += rng.uniform(-jitter, jitter, V.shape) * min(sx, sy)
    idx = np.arange(nx * ny).reshape(nx, ny)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    F = np.concatenate([np.stack([a, b, c], axis=1), np.stack([b, d, c], axis=1)])
    return V, F.astype(np.int64)


def unit_grid_edges(nx, ny):
    """The axis edges (no diagonals) of an nx x ny unit grid -> (V, edge_index)."""
    gx, gy = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing='ij')
    V = np.stack([gx.ravel(), gy.ravel(), np.zeros(nx * ny)], axis=1)
    idx = np.arange(nx * ny).reshape(nx, ny)
    ei = np.concatenate([np.stack([idx[:-1].ravel(), idx[1:].ravel()]), np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()])], axis=1)
    return V, ei


def kite():
    """The 4-cycle 0 - 1 - 2 - 3 - 0: the one-hop edge 0 - 3 (length 3) is longer than the two-hop path 0 - 1 - 2 (1 + 1), so from
    vertex 0 the hop metric puts 3 before 2 and the edge metric 2 before 3.  (Between the SAME two vertices a straight edge can never
    be longer than a path - the triangle inequality - so the two paths end at different vertices.)"""
    V = np.array([[0.0, 0, 0], [1.0, 0, 0], [1.0, 1.0, 0], [-3.0, 0, 0]])
    return V, np.array([[0, 1, 2, 3], [1, 2, 3, 0]])


def ladder_with_shortcut(n=300):
    """Two straight rails of h = (n - 20) / 2 closely spaced vertices with rungs, and a shortcut in HOPS that joins their ends: an
    arc of 20 vertices with long edges (21 hops, length ~ 1.5 x the rails').  From vertex 0 the far end is first reached over the
    arc, the wave runs back down the rails, and every vertex it touched is lowered again when the wave along the rails arrives,
    up to h rounds after its first value.  (A single straight edge between the ends could not be longer than the rails.)"""
    h, k = (n - 20) // 2, n - 2 * ((n - 20) // 2)
    x = np.linspace(0.0, 10.0, h)
    rails = np.concatenate([np.stack([x, np.zeros(h), np.zeros(h)], axis=1), np.stack([x, np.full(h, 0.05), np.zeros(h)], axis=1)])
    t = np.linspace(np.pi, 0.0, k + 2)[1:-1]
    arc = np.stack([5.0 + 5.0 * np.cos(t), np.zeros(k), 5.0 * np.sin(t)], axis=1)
    V = np.concatenate([rails, arc])
    a, c = np.arange(h - 1), 2 * h + np.arange(k - 1)
    ei = np.concatenate([np.stack([a, a + 1]), np.stack([a + h, a + h + 1]), np.stack([np.arange(h), np.arange(h) + h]),
                         np.stack([c, c + 1]), np.array([[0, 2 * h + k - 1], [2 * h, h - 1]])], axis=1)
    return V, ei


def chain(n=1025):
    rng = np.random.default_rng(5)
    V = np.zeros((n, 3))
    V[:, 0] = np.cumsum(rng.uniform(0.5, 1.5, n))
    return V, np.stack([np.arange(n - 1), np.arange(1, n)])


def double_star(leaves=5000):
    """Hub 0 with `leaves` leaves at distinct lengths, hub 1 with 600 leaves, the hubs joined: rows far above any LDS frontier."""
    rng = np.random.default_rng(9)
    n2 = 600
    V = np.zeros((2 + leaves + n2, 3))
    V[1] = [40.0, 0, 0]
    ang = rng.uniform(0, 2 * np.pi, leaves)
    rad = 1.0 + np.arange(leaves) * 1e-3
    V[2:2 + leaves] = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-1, 1, leaves)], axis=1)
    ang2 = rng.uniform(0, 2 * np.pi, n2)
    V[2 + leaves:] = V[1] + np.stack([2.0 * np.cos(ang2), 2.0 * np.sin(ang2), np.arange(n2) * 1e-2], axis=1)
    ei = np.concatenate([np.stack([np.zeros(leaves, dtype=np.int64), np.arange(2, 2 + leaves)]),
                         np.stack([np.ones(n2, dtype=np.int64), np.arange(2 + leaves, 2 + leaves + n2)]), np.array([[0], [1]])], axis=1)
    return V, ei


def degenerate():
    """Duplicate edges, self loops, two coincident vertices (a zero-length edge), an isolated vertex and an unreachable component."""
    V = np.array([[0.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0], [2.0, 1.0, 0], [5.0, 5.0, 5.0], [9.0, 0, 0], [9.0, 1.0, 0], [0.5, 2.0, 1.0]])
    ei = np.array([[0, 0, 1, 1, 2, 3, 3, 5, 7, 1, 0], [1, 1, 2, 1, 3, 3, 7, 6, 0, 0, 7]])
    return V, ei                                                        # vertex 4 is isolated, {5, 6} is unreachable from 0
