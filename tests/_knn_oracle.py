"""The k-nearest-neighbour contract of include/stin_hip.h ("k nearest neighbours") restated in numpy, one query at a time: the
distance expression in the order written, a stable argsort over the valid points, padding with (-1, +inf), and the mean with the
fp64 sum taken left to right.  The GPU tests compare with this bit for bit; tests/test_knn.py compares it with scipy's cKDTree."""
import numpy as np


def sq_dist(q, points):
    """d(q, p) = (dx dx + dy dy) + dz dz for one query against every point, fp64 in that order."""
    dx, dy, dz = q[0] - points[:, 0], q[1] - points[:, 1], q[2] - points[:, 2]
    with np.errstate(all='ignore'):
        return (dx * dx + dy * dy) + dz * dz


def knn(queries, points, k, point_valid=None, query_index=None):
    """-> (index int64 [Q, k], d2 float64 [Q, k]): per query the k smallest candidates under (d, index), ascending; -1 / +inf where
    fewer exist.  point_valid: skipped in place, indices stay those of `points`.  query_index: only these rows, the others -1 / inf.
    A candidate whose d is not < +inf is never reported."""
    queries = np.asarray(queries)[:, :3].astype(np.float64)
    points = np.asarray(points)[:, :3].astype(np.float64).reshape(-1, 3)
    valid = np.ones(len(points), dtype=bool) if point_valid is None else np.asarray(point_valid) != 0
    ids = np.flatnonzero(valid)
    cand = points[ids]
    index = np.full((len(queries), k), -1, dtype=np.int64)
    d2 = np.full((len(queries), k), np.inf, dtype=np.float64)
    for i in (range(len(queries)) if query_index is None else np.asarray(query_index).reshape(-1)):
        d = sq_dist(queries[i], cand)
        order = np.argsort(d, kind='stable')[:k]                # ties: the earlier candidate = the lower index
        order = order[d[order] < np.inf]
        index[i, :len(order)] = ids[order]
        d2[i, :len(order)] = d[order]
    return index, d2


def knn_mean(values, index, rows=None, out=None):
    """out[row][c] = (float32)((((double)v1 + (double)v2) + ...) / (double)m) over the m leading non-negative entries of index[row];
    a row with m == 0 keeps out's value.  -> (out float32, filled bool)."""
    values = np.asarray(values, dtype=np.float32)
    out = np.zeros((len(index), values.shape[1]), dtype=np.float32) if out is None else np.array(out, dtype=np.float32)
    filled = np.zeros(len(index), dtype=bool)
    for r in (range(len(index)) if rows is None else rows):
        m = 0
        while m < index.shape[1] and index[r, m] >= 0:
            m += 1
        if m == 0:
            continue
        total = values[index[r, 0]].astype(np.float64)
        for j in range(1, m):
            total = total + values[index[r, j]].astype(np.float64)
        out[r] = (total / np.float64(m)).astype(np.float32)
        filled[r] = True
    return out, filled


def fill_unseen(vertices, colors, count, k=3, min_count=1):
    """-> (colours float32, filled bool): every vertex with count < min_count takes the mean of its k nearest vertices with
    count >= min_count; nobody seen: unchanged."""
    seen = np.asarray(count) >= min_count
    todo = np.flatnonzero(~seen)
    if not seen.any() or not len(todo):
        return np.array(colors, dtype=np.float32), np.zeros(len(seen), dtype=bool)
    index, _ = knn(vertices, vertices, k, point_valid=seen, query_index=todo)
    return knn_mean(colors, index, rows=todo, out=colors)


# ---- the baseline's scene, shared with the GPU test: a 32 x 32 grid, a colour field linear in x and y, one hole of hop radius 5
SIDE, HOLE_CENTRE, HOLE_RADIUS = 32, 6 * 32 + 25, 5


def baseline_scene():
    """-> (positions float64 [1024, 3], colour float32 [1024, 3] in [-1, 1], edge_index int64 [2, E] of the 4-connected grid)."""
    i, j = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing='ij')
    pos = np.stack([j.ravel() * 0.05, i.ravel() * 0.05, np.zeros(SIDE * SIDE)], axis=1)
    color = np.stack([pos[:, 0] / 0.8 - 1.0, pos[:, 1] / 0.8 - 1.0, 0.5 * pos[:, 0] - 0.25 * pos[:, 1]], axis=1).astype(np.float32)
    vid = np.arange(SIDE * SIDE).reshape(SIDE, SIDE)
    a = np.concatenate([vid[:, :-1].ravel(), vid[:-1, :].ravel()])
    b = np.concatenate([vid[:, 1:].ravel(), vid[1:, :].ravel()])
    return pos, color, np.stack([np.concatenate([a, b]), np.concatenate([b, a])]).astype(np.int64)


def hole_mask():
    """The circle mask of hop radius HOLE_RADIUS around HOLE_CENTRE on the 4-connected grid: R - hops inside, 0 outside."""
    ci, cj = divmod(HOLE_CENTRE, SIDE)
    i, j = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing='ij')
    return np.maximum(HOLE_RADIUS - (np.abs(i - ci) + np.abs(j - cj)), 0).ravel().astype(np.int64)
