"""Graph preprocessing on the GPU for the data either side of the hot path.

* ``dilated_edges``     - the reference's ``preprocessing/graph_dilation.compute_all_node_dilated_edges`` (:50-75), which
  produces the ``hierarchy_dil_{d}_edge_index_{L}`` sets the bottleneck blocks run on.  The per-vertex python loops of
  the reference (~30 min per ScanNet scene, README.md:89) become ONE launch of ``stin_dilated_walk_*`` (one thread per
  directed edge) plus a sort/unique per dilation.
* ``vertex_clustering`` - ``preprocessing/graph_level_generation.vertex_clustering`` (:193-244), the Rossignac voxel
  clustering alternative to QEM for building the hierarchy (trace + coarse edges + coarse coordinates): one 63-bit voxel key
  per vertex, a stable radix sort and a scan (``stin_voxel_cluster_f64``), the coarse edges through ``stin_coalesce_pairs_i64``.
* ``circle_masks``      - ``preprocessing/observed_texture_map_generation.process_frame_circles`` (:530-603, ``generate_masks.sh
  circles``): circles of hop radius R around random centres until a fraction of the vertices is masked, the value being
  R - (hop distance to the nearest centre).  The python heap BFS per circle becomes one launch per batch of centres
  (``stin_circle_mask_run``), every mask of a scene and every graph of a collated batch in the same launches, with no host
  synchronisation; ``circle_mask_from_centres`` is the distance pass alone for given centres.

All take and return tensors in the reference's own formats.  QEM decimation itself stays out of scope (it shells out
to vcglib's ``tridecimator``).
"""
import ctypes

import torch

from . import _lib
from .plan import _ptr, _stream


def coalesce(edge_index, num_nodes, vertex_map=None, drop_loops=False):
    """pyg.utils.coalesce: sort by (row 0, row 1) and drop duplicates.  [2, E] int64 CUDA -> [2, E'] int64.
    vertex_map: both endpoints go through this int64 map first (a trace: the coarse edges of a clustering);
    drop_loops: pairs with equal endpoints are left out.  One radix sort + scan on the GPU (stin_coalesce_pairs_i64)."""
    if edge_index.numel() == 0:
        return edge_index.reshape(2, 0)
    if not edge_index.is_cuda:
        raise TypeError('coalesce runs on the GPU only')
    lib = _lib.load()
    ei = edge_index.long().contiguous()
    E, dev = ei.shape[1], ei.device
    out = torch.empty(2, E, dtype=torch.int64, device=dev)
    state = torch.empty(5, dtype=torch.int64, device=dev)
    ws_bytes = lib.stin_coalesce_workspace_bytes(E)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    vm = vertex_map.contiguous() if vertex_map is not None else None
    _lib.check(lib.stin_coalesce_pairs_i64(_ptr(ei[0]), _ptr(ei[1]), _ptr(vm), (int(vm.numel()) if vm is not None else 0), E, int(num_nodes), int(bool(drop_loops)), _ptr(out[0]),
                                           _ptr(out[1]), _ptr(state), _ptr(ws), ws_bytes, _stream(ei)), 'stin_coalesce_pairs_i64')
    st = state.cpu()
    if int(st[3]) != 0:
        raise IndexError('coalesce: an endpoint lies outside [0, %d)%s' % (
            num_nodes, '' if vm is None else ' or a raw endpoint outside the vertex map [0, %d)' % vm.numel()))
    return out[:, :int(st[4])]


def dilated_edges(edge_index, pos, normals, dilations):
    """edge_index: [2, E] int64 CUDA tensor (row 0 -> row 1; any order, duplicates allowed);
    pos, normals: [N, 3] float32 or float64 (the arithmetic type of the walk; the reference pipeline uses float64);
    dilations: ascending ints in [2, 63].
    -> one entry per dilation: an [E_d, 2] int64 tensor of rows [far vertex, centre] sorted by (far, centre) without
    duplicates - exactly what the reference stores in ``dilated_edges[level][i]`` - or ``[]`` when no walker got that far
    (the reference leaves an empty python list there)."""
    lib = _lib.load()
    if not (edge_index.is_cuda and pos.is_cuda and normals.is_cuda):
        raise TypeError('dilated_edges runs on the GPU only (no CPU fallback exists)')
    if pos.dtype not in (torch.float32, torch.float64) or normals.dtype != pos.dtype:
        raise TypeError('pos and normals must both be float32 or both float64')
    dil = [int(d) for d in dilations]
    if any(d < 2 or d > 63 for d in dil) or any(b <= a for a, b in zip(dil, dil[1:])):
        raise ValueError('dilations must be ascending ints in [2, 63]')
    n = pos.shape[0]
    if edge_index.numel() and (int(edge_index.min()) < 0 or int(edge_index.max()) >= n):
        raise IndexError('edge_index refers to a vertex outside [0, %d)' % n)
    ei = coalesce(edge_index.long(), n)
    e = ei.shape[1]
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=pos.device)
    if e:
        rowptr[1:] = torch.cumsum(torch.bincount(ei[0], minlength=n), 0)
    rowptr, row_of, col = rowptr.int(), ei[0].int().contiguous(), ei[1].int().contiguous()
    pos, normals = pos.contiguous(), normals.contiguous()
    out = torch.empty(len(dil), max(e, 1), dtype=torch.int32, device=pos.device)[:, :e]
    harr = (ctypes.c_int32 * len(dil))(*dil)
    fn = lib.stin_dilated_walk_f64 if pos.dtype == torch.float64 else lib.stin_dilated_walk_f32
    _lib.check(fn(_ptr(rowptr), _ptr(col), _ptr(row_of), _ptr(pos), _ptr(normals), n, e, harr, len(dil),
                  _ptr(out) if e else None, _stream(pos)), 'stin_dilated_walk')
    res = []
    for i in range(len(dil)):
        far = out[i] if e else out.new_zeros(0)
        ok = far >= 0
        if e == 0 or not bool(ok.any()):
            res.append([])
            continue
        pairs = coalesce(torch.stack([far[ok].long(), row_of[ok].long()]), n)
        res.append(pairs.t().contiguous())
    return res


def vertex_clustering(coords, edge_index, voxel_size):
    """coords [N, 3] float (CUDA), edge_index [2, E] int64, voxel_size float ->
    (new_coords float32 [Nc, 3], trace int64 [N], coarse_edges int64 [Ec, 2] sorted by (row 0, row 1)).
    Coarse ids follow the lexicographic order of the voxel bins (``np.unique(bins, axis=0)``)."""
    if not coords.is_cuda:
        raise TypeError('vertex_clustering runs on the GPU only')
    lib = _lib.load()
    c64 = coords.double().contiguous()
    n, dev = c64.shape[0], c64.device
    trace = torch.empty(n, dtype=torch.int64, device=dev)
    new_coords = torch.empty(max(n, 1), 3, dtype=torch.float32, device=dev)
    state = torch.empty(5, dtype=torch.int64, device=dev)
    ws_bytes = lib.stin_voxel_cluster_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.stin_voxel_cluster_f64(_ptr(c64), n, float(voxel_size), _ptr(trace), _ptr(new_coords), _ptr(state), _ptr(ws),
                                          ws_bytes, _stream(c64)), 'stin_voxel_cluster_f64')
    st = state.cpu()
    if int(st[3]) != 0:
        raise ValueError('vertex_clustering: non-finite coordinates or more than 2^21 voxels along an axis')
    nc = int(st[4])
    if edge_index.numel():
        ce = coalesce(edge_index, max(nc, 1), vertex_map=trace, drop_loops=True)
    else:
        ce = edge_index.reshape(2, 0)
    return new_coords[:nc], trace, ce.t().contiguous()


def edges_from_faces(faces, num_nodes):
    """Triangles [F, 3] (int, CUDA) -> the symmetric, coalesced edge_index [2, E] of their sides (what open3d's
    compute_adjacency_list gives the reference's mask generation), through ``coalesce``."""
    f = faces.long()
    if f.numel() == 0:
        return f.new_zeros(2, 0)
    a = torch.cat([f[:, 0], f[:, 1], f[:, 2], f[:, 1], f[:, 2], f[:, 0]])
    b = torch.cat([f[:, 1], f[:, 2], f[:, 0], f[:, 0], f[:, 1], f[:, 2]])
    return coalesce(torch.stack([a, b]), num_nodes, drop_loops=True)


def mask_adjacency(edge_index, num_nodes, check=True):
    """The undirected int32 CSR of the mask pass: both directions of every edge_index column (duplicates and self loops are
    harmless to a hop distance) -> (rowptr [N + 1], col [2E]).  No host synchronisation unless `check` (which raises IndexError
    for an endpoint outside [0, num_nodes))."""
    if not edge_index.is_cuda:
        raise TypeError('mask_adjacency runs on the GPU only')
    lib = _lib.load()
    ei = edge_index.long().contiguous()
    n, e, dev = int(num_nodes), int(ei.shape[1]), ei.device
    rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
    col = torch.empty(max(2 * e, 1), dtype=torch.int32, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    ws_bytes = lib.stin_mask_adjacency_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.stin_mask_adjacency_i64(_ptr(ei[0]) if e else None, _ptr(ei[1]) if e else None, e, n, _ptr(rowptr), _ptr(col),
                                           _ptr(bad), _ptr(ws), ws_bytes, _stream(ei)), 'stin_mask_adjacency_i64')
    if check and int(bad.item()) != 0:
        raise IndexError('edge_index refers to a vertex outside [0, %d)' % n)
    return rowptr, col


INFO_HEAD = 5          # per (mask, graph) row of stin_circle_mask_run's info: batches, done, capped, masked, total


def _circle_dist(adjacency, num_nodes, radius, frac, num_masks, seed, ptr, max_iters, centres=None, log_cap=0, want_mask=False,
                 graph_seeds=None):
    """-> (dist int32 [M, N], mask int64 [M, N] or None, info int64, centre_log or None); everything stays on the device and
    nothing synchronises the host.  graph_seeds: one int per graph (host) instead of `seed`."""
    lib = _lib.load()
    rowptr, col = adjacency
    n, dev = int(num_nodes), rowptr.device
    if ptr is None:
        ptr = torch.arange(2, dtype=torch.int64, device=dev) * n         # [0, n] without a host-to-device copy
    ptr = ptr.to(device=dev, dtype=torch.int64).contiguous()
    B, M = int(ptr.numel()) - 1, int(num_masks)
    if int(radius) < 1:
        raise ValueError('radius must be >= 1')
    iters = 1 if centres is not None else int(max_iters)
    dist = torch.empty(M, max(n, 1), dtype=torch.int32, device=dev)[:, :n]
    mask = torch.empty(M, n, dtype=torch.int64, device=dev) if want_mask else None
    info = torch.empty(M * B * (INFO_HEAD + 2 * iters) + 1, dtype=torch.int64, device=dev)
    clog = torch.full((M * B, max(int(log_cap), 1)), -1, dtype=torch.int64, device=dev) if log_cap else None
    ws_bytes = lib.stin_circle_mask_workspace_bytes(n, M, B)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    c = centres.to(device=dev, dtype=torch.int64).contiguous() if centres is not None else None
    gs = None
    if graph_seeds is not None:
        if len(graph_seeds) != B:
            raise ValueError('graph_seeds needs one seed per graph')
        gs = (ctypes.c_int64 * B)(*[int(v) & ((1 << 63) - 1) for v in graph_seeds])
    _lib.check(lib.stin_circle_mask_run(_ptr(rowptr), _ptr(col), n, _ptr(ptr), B, M, int(radius), float(frac), int(seed) & ((1 << 64) - 1),
                                        gs, iters, _ptr(c) if c is not None and c.numel() else None,
                                        int(c.numel()) if c is not None else 0, _ptr(dist), _ptr(mask), _ptr(info), _ptr(clog),
                                        int(log_cap), _ptr(ws), ws_bytes, _stream(rowptr)), 'stin_circle_mask_run')
    return dist, mask, info, clog


def circle_mask_from_centres(edge_index, num_nodes, radius, centres):
    """The distance pass alone: mask[v] = max(0, R - hop distance from v to the nearest of `centres`) (int64 [N], CUDA) over
    edge_index taken as undirected - the value process_frame_circles writes for these centres (:570-584)."""
    n = int(num_nodes)
    c = torch.as_tensor(centres, dtype=torch.int64).reshape(-1).to(edge_index.device)
    if c.numel() and (int(c.min()) < 0 or int(c.max()) >= n):
        raise IndexError('a centre lies outside [0, %d)' % n)
    adj = mask_adjacency(edge_index, n)
    if c.numel() == 0:
        return torch.zeros(n, dtype=torch.int64, device=edge_index.device)
    _, mask, info, _ = _circle_dist(adj, n, radius, 0.0, 1, 0, None, 1, centres=c, want_mask=True)
    if int(info[-1]) != 0:
        raise RuntimeError('circle_mask_from_centres: the overflow drain did not finish (status %d)' % int(info[-1]))
    return mask[0]


def circle_masks(edge_index, num_nodes, radius=16, frac_masked_vertices=0.25, num_masks=1, seed=0, ptr=None,
                 return_centres=False, max_iters=32, adjacency=None):
    """Circle masks as ``generate_masks.sh circles --radius R --frac_masked_vertices F --masks_per_scene num_masks`` makes
    them, on the GPU: int64 [num_masks, N], mask[v] = max(0, R - hop distance to the nearest centre).  edge_index is taken as
    undirected.  ptr (optional, [B + 1]): the vertex ranges of the graphs of a collated batch - every graph gets its own
    masks (own count, own batch sizes, centres from its own range).  Per (mask, graph) the reference's loop: 10 centres, then
    k = int(total * (frac / cur - 1)) more until cur = masked / n >= frac or k <= 0; centres are drawn with replacement by a
    counter-based hash of (seed, mask, batch, i) (the reference samples without replacement from Python's random), k is
    clamped to n (the reference would raise), and at most max_iters batches are run.
    return_centres=True: also a dict with, per mask m and graph g, 'centres'[m][g] (one int64 tensor of global vertex ids per
    batch), 'sizes' / 'counts' (int64 [M, B, max_iters]: batch sizes and the masked count after each batch; zero after the last
    batch), 'batches' and 'capped' ([M, B])."""
    n = int(num_nodes)
    dev = edge_index.device
    adj = adjacency if adjacency is not None else mask_adjacency(edge_index, n)
    log_cap = 0
    if return_centres:
        log_cap = min(max(int(max_iters) * max(n, 1), 16), 1 << 16)
    dist, mask, info, clog = _circle_dist(adj, n, radius, frac_masked_vertices, num_masks, seed, ptr, max_iters, log_cap=log_cap,
                                          want_mask=True)
    if not return_centres:
        return mask
    M, B = int(num_masks), (1 if ptr is None else int(torch.as_tensor(ptr).numel()) - 1)
    it = int(max_iters)
    inf = info.cpu()
    status = int(inf[-1])
    if status & 2:
        raise RuntimeError('circle_masks: more centres than the log holds (%d per mask and graph)' % log_cap)
    if status & 1:
        raise RuntimeError('circle_masks: the overflow drain did not finish')
    rows = inf[:-1].reshape(M, B, INFO_HEAD + 2 * it)
    clog = clog.cpu().reshape(M, B, -1)
    centres = []
    for m in range(M):
        per_g = []
        for g in range(B):
            sizes = rows[m, g, INFO_HEAD:INFO_HEAD + it]
            nb = int(rows[m, g, 0])
            out, pos = [], 0
            for b in range(nb):
                k = int(sizes[b])
                out.append(clog[m, g, pos:pos + k].to(dev))
                pos += k
            per_g.append(out)
        centres.append(per_g)
    return mask, dict(centres=centres, sizes=rows[:, :, INFO_HEAD:INFO_HEAD + it].clone(),
                      counts=rows[:, :, INFO_HEAD + it:].clone(), batches=rows[:, :, 0].clone(), capped=rows[:, :, 2].bool(),
                      masked=rows[:, :, 3].clone())
