"""Mesh clustering restated in numpy, independent of the HIP code: the contract of include/stin_hip.h ("Mesh clustering") that
preprocessing.cluster_mesh has to reproduce bit for bit.  `//` for the bins, np.unique(axis=0) for the cluster ids, one sequential
fp64 sum per cluster in ascending vertex id, and the first occurrence of every sorted cluster triple for the faces."""
import numpy as np


def distinct(F):
    return (F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 0] != F[:, 2])


def cluster_mesh(vertices, faces, cell_size, return_info=False):
    """-> (vertices' float64 [N', 3], faces' int64 [F', 3], trace int64 [N], N'); return_info: also a dict with what the case
    contains ('faces_in' after the input's own degenerate faces have gone, 'degenerate', 'merged', 'merged_opposite')."""
    V = np.asarray(vertices, dtype=np.float64)[:, :3]
    F = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    n = V.shape[0]
    cell = float(cell_size)
    if not (np.isfinite(cell) and cell > 0):
        raise ValueError('cell_size must be finite and > 0')
    if not np.isfinite(V).all():
        raise ValueError('a coordinate is not finite')
    if F.size and (F.min() < 0 or F.max() >= n):
        raise IndexError('a face refers to a vertex outside [0, %d)' % n)
    F = F[distinct(F)]                                                   # faces that repeat a vertex are dropped at once
    # ---- cells: every vertex, whether a face references it or not
    if n:
        _, trace = np.unique(V // cell, axis=0, return_inverse=True)
        trace = np.asarray(trace, dtype=np.int64).reshape(-1)
        nc = int(trace.max()) + 1
    else:
        trace, nc = np.zeros(0, dtype=np.int64), 0
    # ---- positions: one sum per cluster, member after member in ascending vertex id, from 0.0; one division
    sums, counts = np.zeros((nc, 3), dtype=np.float64), np.zeros(nc, dtype=np.int64)
    for v in range(n):
        c = trace[v]
        sums[c, 0] = sums[c, 0] + V[v, 0]
        sums[c, 1] = sums[c, 1] + V[v, 1]
        sums[c, 2] = sums[c, 2] + V[v, 2]
        counts[c] += 1
    pos = sums / counts.astype(np.float64)[:, None]
    # ---- faces: image, degenerate images out, the lowest face id of every vertex set, input order
    img = trace[F]
    ok = distinct(img)
    seen, kept, merged, opposite = {}, [], 0, 0
    for k in np.flatnonzero(ok):                                         # ascending face id: the first of a vertex set stays
        a = tuple(int(x) for x in img[k])
        first = seen.setdefault(tuple(sorted(a)), a)
        if first is a:
            kept.append(k)
            continue
        merged += 1
        r = first.index(a[0])
        opposite += int(first[r:] + first[:r] != a)                      # the same set in the other cyclic order
    out = img[np.asarray(kept, dtype=np.int64)]
    if not return_info:
        return pos, out, trace, nc
    info = dict(faces_in=int(F.shape[0]), degenerate=int((~ok).sum()), merged=merged, merged_opposite=opposite)
    return pos, out, trace, nc, info


def faces_per_edge(F):
    a = np.concatenate([F[:, 0], F[:, 1], F[:, 2]])
    b = np.concatenate([F[:, 1], F[:, 2], F[:, 0]])
    _, counts = np.unique(np.stack([np.minimum(a, b), np.maximum(a, b)], 1), axis=0, return_counts=True)
    return counts


def unreferenced(F, nc):
    return int(nc - np.unique(F).size)


def is_subsequence(sub, seq):
    """Rows of `sub` appear in `seq` in this order."""
    j = 0
    for row in seq:
        if j < sub.shape[0] and np.array_equal(row, sub[j]):
            j += 1
    return j == sub.shape[0]
