"""CPU oracle of the surface samples (test helper): include/stin_hip.h, "Surface samples", restated in numpy - integer face
weights, the counter hash, the square-root barycentric map, the sequential-greedy Poisson-disk set by brute force (no grid), the
first occurrences of a stream and the circle-mask loop over it.  Every float expression is written with the roundings of the
contract (one per product and per sum), so the device agrees bit for bit."""
import numpy as np

import _mask_oracle as MO

G = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
U = np.uint64


def mix64(z):
    """splitmix64's finaliser on uint64 arrays (wrap arithmetic)."""
    with np.errstate(over='ignore'):
        z = np.asarray(z, dtype=U)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def mix64_int(z):
    """The same on one Python integer."""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def stream_seed(seed, m):
    return mix64_int(mix64_int(int(seed) + G) + (int(m) + 1) * G)


def mulhi64(a, b):
    """High 64 bits of the 128-bit product of uint64 arrays (32-bit limbs)."""
    with np.errstate(over='ignore'):
        a, b = np.asarray(a, dtype=U), np.asarray(b, dtype=U)
        m32 = U(0xFFFFFFFF)
        a0, a1, b0, b1 = a & m32, a >> U(32), b & m32, b >> U(32)
        t = a0 * b0
        w1 = a1 * b0 + (t >> U(32))
        w2 = a0 * b1 + (w1 & m32)
        return a1 * b1 + (w1 >> U(32)) + (w2 >> U(32))


def face_weights(vertices, faces):
    """-> (W int64 [F], A2 float64 [F]).  IndexError / ValueError as the device reports them."""
    V, F = np.asarray(vertices, dtype=np.float64)[:, :3], np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if F.size and (F.min() < 0 or F.max() >= len(V)):
        raise IndexError('a face refers to a vertex outside [0, %d)' % len(V))
    with np.errstate(all='ignore'):
        a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
        e1, e2 = b - a, c - a
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        A2 = np.sqrt((nx * nx + ny * ny) + nz * nz)
    if not np.all(np.isfinite(A2)):
        raise ValueError('a vertex of a face is not finite')
    amax = A2.max() if len(A2) else 0.0
    if not amax > 0.0:
        raise ValueError('the mesh has no face of positive area')
    _, e = np.frexp(amax)
    W = np.floor(np.ldexp(A2, 40 - int(e))).astype(np.int64)
    return W, A2


def randoms(seed, first, n):
    """r_k [3, n] uint64 of samples first .. first + n."""
    with np.errstate(over='ignore'):
        base = mix64(U((int(seed) + G) & M64))
        i = (np.arange(n, dtype=U) + U(int(first) & M64)) * U(3)
        return np.stack([mix64(base + (i + U(k)) * U(G)) for k in range(3)])


def sample_surface(vertices, faces, n, seed=0, first=0):
    V, F = np.asarray(vertices, dtype=np.float64)[:, :3], np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    W, _ = face_weights(V, F)
    cum = np.cumsum(W)
    r = randoms(seed, first, n)
    u = mulhi64(r[0], U(int(cum[-1]))).astype(np.int64)
    f = np.searchsorted(cum, u, side='right')                      # the first f with cum[f] > u
    x1 = (r[1] >> U(11)).astype(np.float64) * 2.0 ** -53
    x2 = (r[2] >> U(11)).astype(np.float64) * 2.0 ** -53
    s = np.sqrt(x1)
    b0, b1, b2 = 1.0 - s, s * (1.0 - x2), s * x2
    a, b, c = V[F[f, 0]], V[F[f, 1]], V[F[f, 2]]
    p = (b0[:, None] * a + b1[:, None] * b) + b2[:, None] * c
    return p, f.astype(np.int64), np.stack([b0, b1, b2], axis=1)


def d2_to(points, i, js):
    d = points[js] - points[i]
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def poisson_disk(points, radius):
    """Sequential greedy, brute force: i is kept iff no kept j < i has d2 < r2 (strict)."""
    P = np.asarray(points, dtype=np.float64)[:, :3]
    r = float(radius)
    if not (r > 0.0 and np.isfinite(r)):
        raise ValueError('radius must be positive and finite')
    if not np.all(np.isfinite(P)):
        raise ValueError('a point is not finite')
    r2 = r * r
    kept = np.empty(len(P), dtype=np.int64)
    k = 0
    for i in range(len(P)):
        if k == 0 or not np.any(d2_to(P, i, kept[:k]) < r2):
            kept[k] = i
            k += 1
    return kept[:k].copy()


def nearest(queries, points):
    out = np.empty(len(queries), dtype=np.int64)
    for i, q in enumerate(queries):
        d = points - q
        out[i] = np.argmin((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return out


def first_occurrences(ids):
    _, first = np.unique(ids, return_index=True)
    return np.asarray(ids)[np.sort(first)]


def surface_centres(vertices, faces, candidates, seed=0, spacing=None):
    V = np.asarray(vertices, dtype=np.float64)[:, :3]
    p, _, _ = sample_surface(V, faces, candidates, seed)
    if spacing is not None:
        p = p[poisson_disk(p, spacing)]
    return first_occurrences(nearest(p, V)) if len(p) else np.empty(0, dtype=np.int64)


def mesh_edges(faces):
    F = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]).T


def circle_masks_on_surface(vertices, faces, radius, frac, num_masks, seed, spacing, candidates, max_iters=32, edge_index=None):
    """-> per mask a dict: mask, batches (list of centre arrays), sizes, counts, exhausted, capped."""
    V = np.asarray(vertices, dtype=np.float64)[:, :3]
    n = len(V)
    adj = MO.adjacency(mesh_edges(faces) if edge_index is None else edge_index, n)
    out = []
    for m in range(num_masks):
        stream = surface_centres(V, faces, candidates, stream_seed(seed, m), spacing)
        mask = np.zeros(n, dtype=np.int64)
        pos, total, k, done, exhausted = 0, 0, 10, False, False
        batches, sizes, counts = [], [], []
        for _ in range(max_iters):
            take = stream[pos:pos + k]
            MO.heap_bfs_mask(adj, radius, take, mask)
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
