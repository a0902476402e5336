"""Numpy restatement of the reference's training-crop generation (preprocessing/crop_training_samples.py `process_frame`
:51-237).  TEST INFRASTRUCTURE, like _mask_oracle.py: tests/tools/make_golden_crops.py checks it array by array against the
reference's own code, tests/golden/g17_crops*.npz pins that, and the GPU tests compare `preprocessing.crop_scene` with it on scenes
no fixture holds.

Semantics (per grid position, x outer loop, y inner loop; lo / hi = position -/+ block / 2 in float64, z unbounded):
  per level: inbox = x, y inside the closed box; kept edges = both endpoints inbox, original order; keep = endpoint of a kept
  edge; new id = rank among the kept; dilated rows with both endpoints kept, relabelled by the level's new ids (default) or by
  the rank among the vertices occurring in that filtered set (`reference_dilated_labels`, the reference's np.unique);
  rejection (counter + 2): a level without kept vertices or fewer than `min_coarsest` on the last one;
  traces: the kept target's new id, else the kept coarse vertex nearest to the fine vertex's OWN position (float64
  ((dx dx + dy dy) + dz dz), lowest index on a tie); coarse vertices left without a predecessor, ascending: the nearest kept fine
  vertex (stable order) whose target has more than one predecessor is re-pointed; a crop that cannot be repaired, or in which no
  fine vertex keeps its target at some level, is skipped (counter + 1);
  labels: per level-0 vertex the most frequent label of its originals (lowest on a tie, 0 without originals).
"""
import numpy as np
import torch

MIN_COARSEST = 50


def crop_positions(vertices0, stride):
    """get_sampling_positions (:27-48): float64 centres along x and y from the float32 extent of level 0."""
    v = np.asarray(vertices0)
    mins, maxs = v[:, :3].min(axis=0), v[:, :3].max(axis=0)
    out = []
    for a in (0, 1):
        p = np.arange(mins[a], maxs[a], stride)
        out.append(np.asarray(p + (maxs[a] - p[-1]) / 2, dtype=np.float64))
    return out[0], out[1]


def crop_boxes(centres, block_size):
    """[(x, y)] -> float64 [C, 4] = lo_x, hi_x, lo_y, hi_y."""
    c = np.asarray(centres, dtype=np.float64).reshape(-1, 2)
    h = block_size / 2
    return np.stack([c[:, 0] - h, c[:, 0] + h, c[:, 1] - h, c[:, 1] + h], 1)


def pooled_labels(trace0, labels, n0):
    hist = np.zeros((n0, int(labels.max()) + 1), dtype=np.int64)
    np.add.at(hist, (trace0, labels), 1)
    return hist.argmax(axis=1)


def _d2(q, c):
    """float64 squared distances [Q, C] from float32 rows, summed as ((dx dx + dy dy) + dz dz)."""
    q, c = q[:, :3].astype(np.float64), c[:, :3].astype(np.float64)
    dx, dy, dz = (q[:, None, k] - c[None, :, k] for k in range(3))
    return (dx * dx + dy * dy) + dz * dz


def nearest(q, c, chunk=512):
    out = np.zeros(q.shape[0], dtype=np.int64)
    for i in range(0, q.shape[0], chunk):
        out[i:i + chunk] = _d2(q[i:i + chunk], c).argmin(axis=1)      # first minimum = lowest index
    return out


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def scene_to_numpy(saved):
    d = {'vertices': [_np(v) for v in saved['vertices']], 'edges': [_np(e).reshape(-1, 2) for e in saved['edges']],
         'traces': [_np(t) for t in saved['traces']], 'dilation_dists': saved.get('dilation_dists'),
         'dilated_edges': [None if x is None else [_np(y).reshape(-1, 2) if len(y) else [] for y in x]
                           for x in saved.get('dilated_edges', [None] * len(saved['vertices']))]}
    if 'labels' in saved:
        d['labels'] = _np(saved['labels'])
    return d


def crop_one(sc, box, pooled, min_coarsest=MIN_COARSEST, reference_dilated_labels=False, stats=None):
    """-> ('ok', crop, kept ids per level) | ('size', None, None) | ('skip', None, None)."""
    lox, hix, loy, hiy = (float(b) for b in box)
    L = len(sc['vertices'])
    keeps, newids, coords, c_edges, c_dil = [], [], [], [], []
    for l in range(L):
        v = sc['vertices'][l]
        p = v[:, :3].astype(np.float64)
        inbox = (p[:, 0] >= lox) & (p[:, 0] <= hix) & (p[:, 1] >= loy) & (p[:, 1] <= hiy) & ~np.isnan(p[:, 2])
        e = sc['edges'][l]
        ke = e[inbox[e[:, 0]] & inbox[e[:, 1]]]
        keep = np.zeros(v.shape[0], dtype=bool)
        keep[ke.ravel()] = True
        newid = np.cumsum(keep) - 1
        keeps.append(keep)
        newids.append(newid)
        coords.append(v[keep])
        c_edges.append(newid[ke].reshape(-1, 2))
        dl = sc['dilated_edges'][l]
        if dl is None:
            c_dil.append(None)
        else:
            sets = []
            for s in dl:
                if len(s) == 0:
                    sets.append([])
                    continue
                ks = s[keep[s[:, 0]] & keep[s[:, 1]]]
                if reference_dilated_labels:
                    sets.append(np.unique(ks, return_inverse=True)[1].reshape(-1, 2).astype(np.int64))
                else:
                    sets.append(newid[ks].reshape(-1, 2))
            c_dil.append(sets)
    if min(c.shape[0] for c in coords) == 0 or coords[-1].shape[0] < min_coarsest:
        return 'size', None, None
    c_traces = []
    for l in range(L - 1):
        t = sc['traces'][l + 1][keeps[l]]
        direct = keeps[l + 1][t]
        if not direct.any():
            return 'skip', None, None
        tr = np.where(direct, newids[l + 1][t], 0).astype(np.int64)
        q = np.flatnonzero(~direct)
        if q.size:
            tr[q] = nearest(coords[l][q], coords[l + 1])
        if stats is not None:
            stats['redirected'] = stats.get('redirected', 0) + int(q.size)
        nc = coords[l + 1].shape[0]
        counts = np.bincount(tr, minlength=nc)
        missing = np.flatnonzero(counts == 0)
        for m in missing:                                              # ascending
            order = np.argsort(_d2(coords[l + 1][m:m + 1], coords[l])[0], kind='stable')
            for nb in order:
                if counts[tr[nb]] > 1:
                    counts[tr[nb]] -= 1
                    counts[m] += 1
                    tr[nb] = m
                    break
            else:
                return 'skip', None, None
            if stats is not None:
                stats['repairs'] = stats.get('repairs', 0) + 1
        c_traces.append(tr)
    crop = {'vertices': [c.astype(np.float32) for c in coords], 'edges': c_edges, 'dilated_edges': c_dil,
            'dilation_dists': sc['dilation_dists'], 'traces': c_traces}
    if pooled is not None:
        crop['labels'] = pooled[keeps[0]].astype(np.int64)
    return 'ok', crop, [np.flatnonzero(k) for k in keeps]


def crop_scene(saved, block_size=3.0, stride=1.5, positions=None, min_coarsest=MIN_COARSEST, reference_dilated_labels=False,
               stats=None, return_kept=False):
    """The restatement of process_frame for one scene dict -> [(counter, crop of numpy arrays)] (+ kept ids with return_kept).
    Counter: + 1 per grid position, + 2 for a size-rejected one (the reference's `block_counter += 1; continue` runs the
    `finally` increment too); with `positions` the list index."""
    sc = scene_to_numpy(saved)
    pooled = pooled_labels(sc['traces'][0], sc['labels'], sc['vertices'][0].shape[0]) if 'labels' in sc else None
    if positions is None:
        xs, ys = crop_positions(sc['vertices'][0], stride)
        centres = [(x, y) for x in xs for y in ys]
    else:
        centres = list(positions)
    out, counter = [], 0
    for i, box in enumerate(crop_boxes(centres, block_size)):
        what, crop, kept = crop_one(sc, box, pooled, min_coarsest, reference_dilated_labels, stats)
        cnt = counter if positions is None else i
        if what == 'ok':
            out.append((cnt, crop, kept) if return_kept else (cnt, crop))
        elif stats is not None:
            stats[what] = stats.get(what, 0) + 1
        counter += 2 if what == 'size' else 1
    return out


def synthetic_scene(n0, levels, seed, irregular=False, extent=4.0, n_labels=0, original_factor=2, dilations=(2, 4)):
    """make_synthetic_mesh as the dict of a graphs/<scene>.pt file (CPU tensors): positions scaled to `extent` metres, coarse
    positions = float32 mean of the children (float64 sum in vertex order), dilated sets on the last level.  n_labels > 0: a
    label scene - traces[0] maps original_factor * N0 originals to level 0 at random (some level-0 vertices get none) and
    `labels` are random labels of the originals; otherwise traces[0] is the identity."""
    from surface_texture_inpainting_net_amd.synthetic import make_synthetic_mesh
    s = make_synthetic_mesh(n0, levels, seed=seed, dilations=tuple(dilations), irregular=irregular)
    x = s.x
    n = x.shape[0]
    v0 = torch.zeros(n, 10)
    v0[:, 0:3] = x[:, 6:9] * 1.5 * float(extent)
    v0[:, 3:6] = (s.color + 1.0) / 2.0
    v0[:, 6:9] = x[:, 3:6]
    v0[:, 9] = torch.arange(n)
    vertices, edges, traces, dilated = [v0], [s.edge_index.t().contiguous()], [torch.arange(n)], [None]
    pos = v0[:, :3].double().numpy()
    for lvl in range(1, levels):
        tr = s['hierarchy_trace_index_%d' % lvl].numpy()
        nc = int(s.num_vertices.reshape(-1)[lvl])
        acc = np.zeros((nc, 3))
        np.add.at(acc, tr, pos)
        pos = acc / np.maximum(np.bincount(tr, minlength=nc), 1)[:, None]
        vertices.append(torch.from_numpy(pos.astype(np.float32)))
        pos = vertices[-1].double().numpy()
        edges.append(s['hierarchy_edge_index_%d' % lvl].t().contiguous())
        traces.append(torch.from_numpy(tr))
        sets = []
        for d in dilations:
            k = 'hierarchy_dil_%s_edge_index_%d' % (d, lvl)
            sets.append(s[k].t().contiguous() if k in s and s[k].numel() else [])
        dilated.append(sets if any(len(z) > 0 for z in sets) else None)
    saved = {'vertices': vertices, 'edges': edges, 'traces': traces, 'dilated_edges': dilated, 'dilation_dists': list(dilations)}
    if n_labels:
        rng = np.random.default_rng(seed + 1000)
        saved['traces'][0] = torch.from_numpy(rng.integers(0, n, size=original_factor * n))
        saved['labels'] = torch.from_numpy(rng.integers(0, n_labels, size=original_factor * n))
    return saved


def scene_to(saved, device):
    """The scene dict with every tensor on `device`."""
    out = {}
    for k, v in saved.items():
        if k == 'dilated_edges':
            out[k] = [None if x is None else [y.to(device) if torch.is_tensor(y) else y for y in x] for x in v]
        elif isinstance(v, list) and v and torch.is_tensor(v[0]):
            out[k] = [t.to(device) for t in v]
        elif torch.is_tensor(v):
            out[k] = v.to(device)
        else:
            out[k] = v
    return out


# ---- tests/golden/g17_crops*.npz (written by tests/tools/make_golden_crops.py from the reference's own process_frame)
def fixture_scene_count(z):
    return sum(1 for k in z if k.endswith('.block'))


def fixture_scene(z, i):
    """-> (scene dict of CPU tensors, block, stride) of fixture scene i."""
    p = 's%d.' % i
    L = sum(1 for k in z if k.startswith(p + 'v.'))
    dists = [int(d) for d in z[p + 'dists']]
    saved = {'vertices': [torch.from_numpy(z[p + 'v.%d' % l]) for l in range(L)],
             'edges': [torch.from_numpy(z[p + 'e.%d' % l].astype(np.int64)) for l in range(L)],
             'traces': [torch.from_numpy(z[p + 't.%d' % l].astype(np.int64)) for l in range(L)],
             'dilated_edges': [None if int(z[p + 'dl.%d' % l]) == 0 else
                               [torch.from_numpy(z[p + 'd.%d.%d' % (l, j)].astype(np.int64)) if p + 'd.%d.%d' % (l, j) in z else []
                                for j in range(len(dists))] for l in range(L)],
             'dilation_dists': dists}
    if p + 'labels' in z:
        saved['labels'] = torch.from_numpy(z[p + 'labels'].astype(np.int64))
    return saved, float(z[p + 'block']), float(z[p + 'stride'])


def fixture_crops(z, i):
    """-> [(counter, crop of numpy arrays as the reference stored it, kept ids per level)] of fixture scene i."""
    p = 's%d.' % i
    saved, _, _ = fixture_scene(z, i)
    L = len(saved['vertices'])
    out = []
    for k, cnt in enumerate(z[p + 'counters']):
        q = p + 'c%d.' % k
        kept = [z[q + 'kept.%d' % l].astype(np.int64) for l in range(L)]
        crop = {'vertices': [saved['vertices'][l].numpy()[kept[l]] for l in range(L)],
                'edges': [z[q + 'e.%d' % l].astype(np.int64) for l in range(L)],
                'traces': [z[q + 't.%d' % l].astype(np.int64) for l in range(L - 1)],
                'dilated_edges': [None if saved['dilated_edges'][l] is None else
                                  [z[q + 'd.%d.%d' % (l, j)].astype(np.int64) if len(saved['dilated_edges'][l][j]) else []
                                   for j in range(len(saved['dilation_dists']))] for l in range(L)],
                'dilation_dists': saved['dilation_dists']}
        if q + 'labels' in z:
            crop['labels'] = z[q + 'labels'].astype(np.int64)
        out.append((int(cnt), crop, kept))
    return out


def same_crop(got, want):
    """Bit-exact comparison of two crop dicts (tensors or arrays) -> the first difference as a string, or None."""
    if sorted(got) != sorted(want):
        return 'keys %s != %s' % (sorted(got), sorted(want))
    for k in ('vertices', 'edges', 'traces'):
        if len(got[k]) != len(want[k]):
            return '%s: %d levels != %d' % (k, len(got[k]), len(want[k]))
        for l, (a, b) in enumerate(zip(got[k], want[k])):
            a, b = _np(a), _np(b)
            if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(a, b):
                return '%s[%d] differs (%s %s vs %s %s)' % (k, l, a.dtype, a.shape, b.dtype, b.shape)
    for l, (a, b) in enumerate(zip(got['dilated_edges'], want['dilated_edges'])):
        if (a is None) != (b is None):
            return 'dilated_edges[%d]: None on one side' % l
        for j, (x, y) in enumerate(zip(a or [], b or [])):
            if len(x) == 0 or len(y) == 0:
                if len(x) != len(y) or torch.is_tensor(x) != torch.is_tensor(y) and not isinstance(y, np.ndarray):
                    return 'dilated_edges[%d][%d]: empty on one side' % (l, j)
                continue
            x, y = _np(x), _np(y)
            if x.dtype != y.dtype or x.shape != y.shape or not np.array_equal(x, y):
                return 'dilated_edges[%d][%d] differs' % (l, j)
    if 'labels' in want:
        a, b = _np(got['labels']), _np(want['labels'])
        if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(a, b):
            return 'labels differ'
    if list(got['dilation_dists'] or []) != list(want['dilation_dists'] or []):
        return 'dilation_dists differ'
    return None
