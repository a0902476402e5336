"""numpy restatement of the reference's graph level generation (preprocessing/graph_level_generation.py), written from what the
functions compute, not from their code: the yardstick of tests/test_levels.py (against fixture g19, i.e. the reference's own
outputs) and of tests/test_levels_gpu.py (the HIP path against it on other inputs).

* `nearest`            chunked brute force: argmin over d = (dx dx + dy dy) + dz dz in float64, the lowest index on a tie.
* `trace_from_rows`    csv2npy: rows (new coordinate, old coordinates) -> fine -> coarse trace, LevelError where the reference refuses.
* `fill_unassigned`    nearest_neighbor_interpolation_for_unassigned_traces.
* `colors_and_labels`  get_color_and_labels.
* `graph_levels`       the dict process_frame saves; edges sorted by (row 0, row 1) (the reference's order inside a vertex group is a
                       CPython set order), dilated sets and vertex clustering through oracle/dilation_oracle.py.
"""
import io

import numpy as np

from oracle import dilation_oracle as D


class LevelError(ValueError):
    pass


def sq_dist(q, p):
    """[Q, 3] x [P, 3] float64 -> [Q, P], the expression every implementation shares."""
    dx = q[:, None, 0] - p[None, :, 0]
    dy = q[:, None, 1] - p[None, :, 1]
    dz = q[:, None, 2] - p[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def nearest(queries, points, return_sq_dist=False, return_gap=False, block=None):
    q = np.asarray(queries, dtype=np.float64)[:, :3]
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float64)[:, :3])
    if p.shape[0] == 0 and q.shape[0]:
        raise ValueError('no points')
    out = np.empty(q.shape[0], dtype=np.int64)
    d2 = np.empty(q.shape[0], dtype=np.float64)
    gap = np.inf
    step = block or max(1, (1 << 22) // max(p.shape[0], 1))
    for i in range(0, q.shape[0], step):
        d = sq_dist(q[i:i + step], p)
        out[i:i + step] = np.argmin(d, axis=1)               # the first minimum: the lowest index on a tie
        d2[i:i + step] = d[np.arange(d.shape[0]), out[i:i + step]]
        if return_gap and p.shape[0] > 1:
            part = np.partition(d, 1, axis=1)
            gap = min(gap, float((part[:, 1] - part[:, 0]).min()))
    res = (out,)
    if return_sq_dist:
        res += (d2,)
    if return_gap:
        res += (gap,)
    return res[0] if len(res) == 1 else res


def read_trace_csv(text):
    """CSV text (str or bytes) -> (new_xyz [R, 3], old_xyz [T, 3], row_ptr [R + 1])."""
    if isinstance(text, (bytes, bytearray, np.ndarray)):
        text = bytes(text).decode()
    new, old, ptr = [], [], [0]
    for line in io.StringIO(text):
        line = line.strip('\r\n')
        if not line:
            continue
        f = line.split(';')
        new.append([float(x) for x in f[:3]])
        k = len(f) // 3 - 1
        for i in range(k):
            old.append([float(x) for x in f[3 * i + 3:3 * i + 6]])
        ptr.append(len(old))
    return (np.asarray(new, np.float64).reshape(-1, 3), np.asarray(old, np.float64).reshape(-1, 3), np.asarray(ptr, np.int64))


def fill_unassigned(new_coords, old_coords, trace):
    trace = np.asarray(trace).astype(np.int64).copy()
    todo = np.flatnonzero(trace == -1)
    if todo.size:
        trace[todo] = nearest(np.asarray(old_coords)[todo], new_coords)
    return trace


def trace_from_rows(rows, old_vertices, new_vertices):
    """rows = (new_xyz, old_xyz, row_ptr).  -> int64 [n_old]; LevelError in the three cases the reference refuses."""
    new_xyz, old_xyz, ptr = rows
    n_old, n_new = old_vertices.shape[0], new_vertices.shape[0]
    new_id = nearest(new_xyz, new_vertices) if new_xyz.shape[0] else np.zeros(0, np.int64)
    old_id = nearest(old_xyz, old_vertices) if old_xyz.shape[0] else np.zeros(0, np.int64)
    counts = np.diff(ptr)
    # a row is refused when an earlier row of the same new vertex carried old vertices
    taken = np.zeros(n_new, dtype=bool)
    for r in range(new_id.shape[0]):
        if taken[new_id[r]]:
            raise LevelError('new vertex %d taken twice' % new_id[r])
        if counts[r] > 0:
            taken[new_id[r]] = True
    row_of = np.repeat(np.arange(new_id.shape[0]), counts)
    hits = np.bincount(old_id, minlength=n_old)
    trace = np.full(n_old, -1, dtype=np.int64)
    trace[old_id] = new_id[row_of]
    trace = fill_unassigned(new_vertices, old_vertices, trace)
    covered = np.zeros(n_new, dtype=bool)
    covered[new_id] = True
    covered[trace] = True
    if not covered.all():
        raise LevelError('%d new vertices uncovered' % int((~covered).sum()))
    if hits.max(initial=0) > 1:
        raise LevelError('an old vertex named twice')
    return trace


def colors_and_labels(original_vertices, level_coords):
    return [original_vertices[nearest(c, original_vertices)][:, 3:] for c in level_coords]


SCANNET_KEPT = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39]   # nyu40 ids of the 20 benchmark classes


def remap_scannet_labels(labels):
    ids = np.asarray(labels).astype(np.int64).copy()
    ids[ids > 40] = 0
    table = np.zeros(41, dtype=np.int64)
    table[SCANNET_KEPT] = np.arange(1, 21)
    return table[ids]


def mesh_edges(faces, n):
    """Triangles -> [E, 2] rows (vertex, neighbour), sorted, without duplicates."""
    f = np.asarray(faces, dtype=np.int64)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2], f[:, 1], f[:, 2], f[:, 0]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0], f[:, 0], f[:, 1], f[:, 2]])
    keep = a != b
    return D.coalesce(np.stack([a[keep], b[keep]]), n).T.copy()


def sorted_rows(e):
    e = np.asarray(e, dtype=np.int64).reshape(-1, 2)
    return e[np.lexsort((e[:, 1], e[:, 0]))]


def graph_levels(mesh, levels, dilated_levels, dilation_dists, labels=None, reference_vc_normals=False):
    """numpy arrays in, numpy arrays out: {'vertices', 'labels'?, 'edges', 'traces', 'dilated_edges', 'dilation_dists'}.
    levels as preprocessing.graph_levels takes them ('csv' of a decimator level: the (new_xyz, old_xyz, row_ptr) tuple or text)."""
    v = np.asarray(mesh['vertices'], dtype=np.float64)
    n = v.shape[0]
    nrm0 = np.asarray(mesh['normals'], dtype=np.float64)
    cols = [v, np.asarray(mesh['colors'], dtype=np.float64), nrm0, np.arange(n, dtype=np.float64)[:, None]]
    if labels is not None:
        cols.append(np.asarray(labels, dtype=np.float64).reshape(n, 1))
    original = np.concatenate(cols, axis=1)
    vc_mode = all(isinstance(x, (int, float)) for x in levels)
    coords, edges, traces, normals = [v], [], [], []
    cur = dict(vertices=v, faces=np.asarray(mesh['faces']), normals=nrm0)
    cur_edges = mesh_edges(cur['faces'], n)
    for spec in levels:
        if vc_mode:
            c, t, e = D.vertex_clustering(coords[-1], cur_edges.T, float(spec))     # numpy's own dtype rules, as in the reference
            cur_edges = e
            nr = None
        elif isinstance(spec, dict):
            c = np.asarray(spec['vertices'], dtype=np.float64)
            e = mesh_edges(spec['faces'], c.shape[0])
            if 'csv' in spec:
                rows = spec['csv'] if isinstance(spec['csv'], tuple) else read_trace_csv(spec['csv'])
                t = trace_from_rows(rows, coords[-1], c)
            else:
                t = nearest(coords[0], c)
            cur = dict(vertices=c, faces=np.asarray(spec['faces']), normals=np.asarray(spec['normals'], dtype=np.float64))
            nr = cur['normals']
        else:
            c = cur['vertices']
            e = mesh_edges(cur['faces'], c.shape[0])
            t = np.arange(c.shape[0], dtype=np.int64)
            nr = cur['normals']
        coords.append(c)
        edges.append(e)
        traces.append(np.asarray(t, dtype=np.int64))
        normals.append(nr)
    near = [nearest(c, original) for c in coords]
    ccl = [np.column_stack((coords[i], original[near[i]][:, 3:])) for i in range(len(coords))]
    dilated = []
    for l in range(len(levels)):
        if int(dilated_levels[l]) != 1:
            dilated.append(None)
            continue
        c = coords[l + 1].astype(np.float64)
        nr = normals[l]
        if nr is None:
            nr = nrm0[:c.shape[0]] if reference_vc_normals else nrm0[near[l + 1]]
        dilated.append(D.dilated_edges(edges[l].T, c, nr.astype(np.float64), [int(d) for d in dilation_dists]))
    out = {}
    if labels is not None:
        out['vertices'] = [ccl[1][:, :-1].astype(np.float32)] + [ccl[i][:, :3].astype(np.float32) for i in range(2, len(ccl))]
        out['labels'] = ccl[0][:, -1].astype(np.int64)
    else:
        out['vertices'] = [ccl[1].astype(np.float32)] + [ccl[i][:, :3].astype(np.float32) for i in range(2, len(ccl))]
    out['edges'] = edges
    out['traces'] = traces
    out['dilated_edges'] = dilated
    out['dilation_dists'] = dilation_dists
    return out


def grid_mesh(side, seed, spacing=0.25):
    """A jittered, triangulated height field with vertex ids in random order: {'vertices' f64, 'faces' int64, 'colors', 'normals'}
    (area-weighted vertex normals) - the synthetic stand-in for a scanned mesh in the tests and profiles."""
    rng = np.random.default_rng(seed)
    gi, gj = np.meshgrid(np.arange(side), np.arange(side), indexing='ij')
    ij = np.stack([gi.ravel(), gj.ravel()], 1)
    ij = ij[rng.permutation(ij.shape[0])]
    xy = ij * spacing + rng.uniform(-0.3, 0.3, ij.shape) * spacing
    z = 0.4 * np.sin(xy[:, 0] * 1.3) * np.cos(xy[:, 1] * 0.9) + rng.normal(0, 0.08 * spacing, ij.shape[0])
    v = np.column_stack([xy, z])
    ids = np.empty((side, side), dtype=np.int64)
    ids[ij[:, 0], ij[:, 1]] = np.arange(ij.shape[0])
    a, b, c, d = ids[:-1, :-1].ravel(), ids[1:, :-1].ravel(), ids[:-1, 1:].ravel(), ids[1:, 1:].ravel()
    f = np.concatenate([np.stack([a, b, d], 1), np.stack([a, d, c], 1)])
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    nrm = np.zeros_like(v)
    for k in range(3):
        np.add.at(nrm, f[:, k], fn)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return dict(vertices=v, faces=f, colors=rng.uniform(0, 1, v.shape), normals=nrm)
