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

* ``graph_levels``      - the body of ``preprocessing/graph_level_generation.process_frame`` (:298-539): mesh -> level hierarchy
  -> the dict of ``graphs/<scene>.pt``, fully on the GPU in vertex-clustering mode and in decimator mode with percentage levels
  (``['100', '30', '30', '30']``: ``decimate_qem``), or from an external decimator's outputs.  Its parts: ``nearest`` (exact fp64 nearest neighbour between two large point sets, tiled brute force:
  ``stin_nearest_f64``), ``read_trace_csv`` / ``trace_from_csv`` (``csv2npy`` :135-191: two batched searches, an integer scatter and
  one state vector instead of one BallTree query per CSV coordinate), ``fill_unassigned_trace``
  (``nearest_neighbor_interpolation_for_unassigned_traces`` :284-295), ``colors_and_labels`` (``get_color_and_labels`` :98-116) and
  ``remap_scannet_labels``; ``LevelError`` where the reference raises ``QEMError`` or trips an assert.

* ``decimate_qem``      - the QEM decimator the reference shells out to (vcglib's ``tridecimator``): a deterministic, parallel
  edge-collapse decimator in HIP (``stin_qem_*``): rounds of independent collapses chosen by two per-vertex minimum passes, fixed-order
  fp64 quadric sums, and the fine -> coarse trace as a direct result instead of a CSV and one BallTree query per row.  Its contract is
  stated in include/stin_hip.h and restated in numpy by the test suite (bit-exact parity); it is NOT pinned against vcglib.
  ``vertex_normals`` - open3d's documented ``compute_vertex_normals`` rule (unit face normals summed, normalised), for the levels it makes.

* ``cluster_mesh``      - the mesh clustering the reference shells out to vcglib's ``trimesh_clustering`` for (a ``--qem`` level such
  as ``0.04``): ``vertex_clustering``'s cells and trace with fp64 means (``stin_voxel_cluster_mean_f64``) and the faces carried along -
  degenerate images dropped, one face per vertex set (``stin_face_cluster_i64``: a stable radix sort of the sorted cluster triples) - so
  that QEM levels can follow (``['0.04', '30', '30', '30']`` from a mesh alone).  A contract of this project's own, NOT pinned against
  vcglib (grid origin 0, unweighted means).

* ``observe_vertices``  - ``preprocessing/observed_texture_map_generation.compute_observed_vertex_map`` (:159-251, ``generate_masks.sh
  observers``), which renders the mesh from every camera pose with PyTorch3D and keeps the face seen at each pixel: a depth-tested
  triangle rasteriser in HIP (``stin_observe_poses_f64``) that answers "which poses see vertex v" as one bit per (vertex, pose).
  ``pose_extrinsics`` is ``load_camera_poses``' inverse (:58-63) plus the validity rule; ``observer_visible`` is
  ``select_pose_random_subset`` (:254-256) with a stated seed; ``observer_masks`` is ``generate_mask_from_vertex_observing_poses``
  (:259-267, ``stin_observe_mask_u32``) for every mask of a scene at once - ``process_frame_observers`` (:486-527) with the
  ``masks_per_scene`` its TODO (:731) asks for; ``observer_counts`` are the two statistics of ``plot_statistics`` (:454-483);
  ``observers_to_lists`` gives the reference's ``observed_poses_per_vert`` cache format.  The projection convention is derived from
  reading the reference and PyTorch3D's documented conventions, NOT pinned against a PyTorch3D run (its imports are commented out
  in the reference and it is not installed here); faces that cross the near plane are dropped, not clipped.

* ``FrameColors`` / ``vertex_colors_from_frames`` - ``preprocessing/texture_map_optimization.py``, which hands a mesh, the scan's colour
  and depth frames and the camera trajectory to Open3D's colour-map pipeline with ``maximum_iteration=0``: per vertex and frame a
  visibility test (against the sensor's depth away from depth discontinuities, or ``observe_vertices``' bits), a projection and a
  bilinear colour sample, averaged in integers (``stin_frames_*``).  ``frame_intrinsics`` is its rescaled camera (:104-107).  A
  contract of this project's own, NOT pinned against an Open3D run.

* ``optimize_poses_rigid`` - the rigid optimisation the same pipeline runs with ``maximum_iteration > 0`` (Zhou & Koltun 2014): per
  iteration the proxy intensities from ``FrameColors``' sums, the photometric residual and 6-DoF Jacobian of every visible (vertex,
  pose) pair, the normal equations of every pose summed in a fixed order (``stin_colormap_*``), and one Gauss-Newton step per free pose
  on the host (``rigid_update``, ``rigid_increment``).  A contract of this project's own, NOT pinned against Open3D.

* ``optimize_poses_nonrigid`` - the non-rigid optimisation, the call the reference actually makes (``run_non_rigid_optimizer``;
  Zhou & Koltun 2014, section 5): a low-resolution warp lattice per frame beside its pose.  The normal equations are summed per
  (pose, lattice cell) in ascending vertex id (``stin_nonrigid_*``: keys, a sort, one workgroup per cell), the colours are sampled at
  the warped positions, and the host solves one (6 + 2 anchors) system per free pose (``nonrigid_update``) - or, with
  ``solver='banded'``, the device does: ``nonrigid_solve``, a banded-arrow Cholesky per pose (``stin_nonrigid_solve_f64``).  NOT
  pinned against Open3D.

* ``knn`` / ``fill_unseen_colors`` / ``knn_inpaint`` - exact fp64 k nearest neighbours with a validity mask on the points
  (``stin_knn_f64``: ``nearest``'s tiled brute force with a k-list per query in registers) and the mean of the neighbours' rows
  (``stin_knn_mean_f32``): the fill of unseen vertices that Open3D's pipeline ends with (``FrameColors.result(knn=3)``), and the
  nearest-known-vertex baseline to put beside the network's l1 / psnr.

* ``resize_u8`` / ``resize_pool_u8`` / ``scan_vertex_colors`` - the two ``cv2.resize`` calls of the reference: colour frames to the
  depth size (``texture_map_optimization.py:93``, bilinear) and ``Rescale`` of the 2-D experiment (``INTER_AREA``), in integers, one
  launch for a batch or a ragged pool of images (``stin_resize_u8``); ``scan_vertex_colors`` is ``load_dataset`` plus the averaging,
  from a scan directory.  A contract of this project's own (include/stin_hip.h, "Image resize"), NOT pinned against cv2.

* ``sample_surface`` / ``poisson_disk`` / ``surface_centres`` / ``circle_masks_on_surface`` - the sampler ``process_frame_circles``
  planned and left as a TODO (:545-562, "Sample using poisson disk"; it draws centres over vertex ids instead, which ``circle_masks``
  reproduces): area-uniform points on the mesh with exact integer face weights, a Poisson-disk subset in index order (uniform grid,
  decision rounds), the nearest vertices without repeats, and the reference's batch loop over that stream (``stin_surface_*``,
  ``stin_poisson_*``, ``stin_first_occurrence_i64``).  A contract of this project's own (include/stin_hip.h, "Surface samples"),
  NOT pinned against Open3D's ``sample_points_poisson_disk``; Euclidean spacing, hop-count radii.

* ``geodesic_adjacency`` / ``geodesic_distance`` / ``circle_mask_from_centres_geodesic`` / ``circle_masks_geodesic`` - the same
  masks with a radius that is a LENGTH in the units of the vertices: bounded multi-source shortest paths over the mesh edges
  weighted by their Euclidean length (``stin_geodesic_*``: frontier rounds, 64-bit integer atomicMin on fp64 bit patterns), the
  same bytes on every schedule and equal to heap Dijkstra's.  The Dijkstra metric of the edge graph, NOT the exact polyhedral
  geodesic.  A contract of this project's own (include/stin_hip.h, "Geodesic distances").

* ``harmonic_fill`` / ``harmonic_inpaint`` / ``harmonic_adjacency`` - the classic non-learned inpainting baseline: harmonic
  (diffusion, Laplace) fill, every masked vertex the weighted mean of its neighbours with the known vertices as boundary values,
  by Jacobi-preconditioned CG in fp64 with every sum in a fixed order (``stin_harmonic_*``: two ordinary launches per iteration,
  channels frozen when done), the same bytes on every run.  Uniform or inverse-length weights, NOT cotangent weights.  A contract
  of this project's own (include/stin_hip.h, "Harmonic fill").

All take and return tensors in the reference's own formats.  Mesh files are read by scene_io.read_ply (PLY, decoded on the GPU:
its dict is the `mesh` argument of the functions here; read_scannet_mesh adds the labels of a ScanNet scan, vertex_labels_from_faces
the per-face vote of the Matterport path).  Out of scope: the Matterport category tables and the S3DIS label path.
"""
import ctypes
import re

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


# ------------------------------------------------------------------------------------------------------------- training crops
MIN_NUM_MAXIMALLY_DECIMATED_VERTS = 50      # preprocessing/crop_training_samples.py:24
_SEG = _lib.STRUCTS['stin_crop_seg_t']
_SEG_WORDS = _SEG.size // 8                                      # int64 words of a stin_crop_seg_t
_SEG_VERTICES, _SEG_EDGES, _SEG_DILATED, _SEG_OCCURS, _SEG_TRACE = (_lib.CONSTANTS[n] for n in (
    'STIN_CROP_VERTICES', 'STIN_CROP_EDGES', 'STIN_CROP_DILATED', 'STIN_CROP_OCCURS', 'STIN_CROP_TRACE'))


def crop_positions(vertices0, stride):
    """The reference's get_sampling_positions (crop_training_samples.py:27-48): centres of the crop grid along x and y -
    np.arange(min, max, stride) on the float32 extent of level 0, centred by (max - last) / 2.  -> (xs, ys) float64 numpy arrays.
    vertices0: [N0, >= 3] tensor (any device) or array."""
    import numpy as np
    v = vertices0[:, :3] if torch.is_tensor(vertices0) else torch.as_tensor(np.asarray(vertices0)[:, :3])
    mins, maxs = v.min(dim=0).values.cpu().numpy(), v.max(dim=0).values.cpu().numpy()
    out = []
    for a in (0, 1):
        p = np.arange(mins[a], maxs[a], stride)
        out.append(np.asarray(p + (maxs[a] - p[-1]) / 2, dtype=np.float64))
    return out[0], out[1]


def pooled_labels(trace0, labels, n0):
    """Label of every level-0 vertex from the labels of the ORIGINAL mesh's vertices (crop_training_samples.py:119-125): the most
    frequent label among trace0 == v, the lowest on a tie, 0 for a vertex without originals.  int64 [n0], on the device; an integer
    histogram (stin_label_pool_i64), so the result does not depend on the schedule."""
    if not (trace0.is_cuda and labels.is_cuda):
        raise TypeError('pooled_labels runs on the GPU only')
    lib = _lib.load()
    t, lab = trace0.long().contiguous(), labels.long().contiguous()
    if t.numel() != lab.numel():
        raise ValueError('labels and traces[0] must have one entry per vertex of the original mesh')
    n_labels = int(lab.max()) + 1 if lab.numel() else 1
    if n_labels < 1:
        raise IndexError('negative label')
    out = torch.empty(int(n0), dtype=torch.int64, device=t.device)
    status = torch.empty(1, dtype=torch.int32, device=t.device)
    ws_bytes = lib.stin_label_pool_workspace_bytes(int(n0), n_labels)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=t.device)
    _lib.check(lib.stin_label_pool_i64(_ptr(t), _ptr(lab), int(t.numel()), int(n0), n_labels, _ptr(out), _ptr(status), _ptr(ws),
                                       ws_bytes, _stream(t)), 'stin_label_pool_i64')
    if int(status.item()) != 0:
        raise IndexError('traces[0] refers to a vertex outside [0, %d) or a label is negative' % int(n0))
    return out


def _repair_trace(trace, fine, coarse):
    """The reference's fix for coarse vertices without a predecessor (crop_training_samples.py:168-189), on the host: the missing
    ones in ascending order; for each, the kept fine vertices by ascending distance (stable), the first whose target has more than
    one predecessor is re-pointed.  trace int64 [nf] (modified), fine / coarse float32 [., >= 3] numpy.  -> False: no candidate."""
    import numpy as np
    counts = np.bincount(trace, minlength=coarse.shape[0])
    f = fine[:, :3].astype(np.float64)
    for m in np.flatnonzero(counts == 0):
        c = coarse[m, :3].astype(np.float64)
        dx, dy, dz = c[0] - f[:, 0], c[1] - f[:, 1], c[2] - f[:, 2]
        for nb in np.argsort((dx * dx + dy * dy) + dz * dz, kind='stable'):
            if counts[trace[nb]] > 1:
                counts[trace[nb]] -= 1
                counts[m] += 1
                trace[nb] = m
                break
        else:
            return False
    return True


def _crop_chunk(saved, boxes, pooled, reference_dilated_labels, min_coarsest):
    """All crops of `boxes` (float64 [C, 4] numpy) in one batched pass -> per crop None (rejected by size), False (skipped) or
    (crop dict, kept ids per level)."""
    import numpy as np
    lib = _lib.load()
    verts = [v.float().contiguous() for v in saved['vertices']]
    dev = verts[0].device
    L, C = len(verts), int(boxes.shape[0])
    edges = [e.long().reshape(-1, 2).contiguous() for e in saved['edges']]
    traces = [t.long().contiguous() for t in saved['traces']]
    dil_in = saved.get('dilated_edges') or [None] * L
    if len(edges) != L or len(traces) != L or len(dil_in) != L:
        raise ValueError('vertices, edges, traces and dilated_edges need one entry per level')
    for l in range(1, L):
        if traces[l].numel() != verts[l - 1].shape[0]:
            raise ValueError('traces[%d] needs one entry per vertex of level %d' % (l, l - 1))
    # ---- segment table: one row per vertex set, edge list, dilated set (and its occurrence flags) and trace
    rows = []
    base = ibase = 0

    def add(kind, level, n, src=None, vseg=-1, aux=-1, width=0, flagged=True, ib=0):
        nonlocal base
        rows.append(dict(kind=kind, level=level, vseg=vseg, aux=aux, n=int(n), base=base if flagged else 0, width=width, ibase=ib,
                         src=src, out=None, ids=None, p0=None, p1=None))
        if flagged:
            base += C * int(n)
        return len(rows) - 1

    vseg = []
    for l in range(L):
        if verts[l].dim() != 2 or verts[l].shape[1] < 3:
            raise ValueError('vertices[%d] must be [N, >= 3]' % l)
        vseg.append(add(_SEG_VERTICES, l, verts[l].shape[0], verts[l], width=int(verts[l].shape[1]), ib=ibase))
        ibase += C * int(verts[l].shape[0])
    eseg = [add(_SEG_EDGES, l, edges[l].shape[0], edges[l], vseg=vseg[l]) for l in range(L)]
    dseg = []
    for l in range(L):
        if dil_in[l] is None:
            dseg.append(None)
            continue
        cur = []
        for s in dil_in[l]:
            if not torch.is_tensor(s) or s.numel() == 0:
                cur.append(None)                                   # an empty list stays an empty list
                continue
            s = s.long().reshape(-1, 2).contiguous()
            occ = add(_SEG_OCCURS, l, verts[l].shape[0], vseg=vseg[l]) if reference_dilated_labels else -1
            cur.append(add(_SEG_DILATED, l, s.shape[0], s, vseg=vseg[l], aux=occ))
        dseg.append(cur)
    tseg = [add(_SEG_TRACE, l, verts[l].shape[0], traces[l + 1], vseg=vseg[l], aux=vseg[l + 1], flagged=False, ib=l)
            for l in range(L - 1)]
    total, inbox_total, n_segs = base, ibase, len(rows)
    max_n = max(r['n'] for r in rows)
    if total + 1 >= 2 ** 31 - 1:
        raise ValueError('too many crops for one pass')           # (crop_scene splits the crop list before this can happen)

    def table():
        ptr = lambda t: 0 if t is None else t.data_ptr()
        blob = b''.join(_SEG.pack(kind=r['kind'], level=r['level'], vseg=r['vseg'], aux=r['aux'], n=r['n'], base=r['base'],
                                  width=r['width'], ibase=r['ibase'], src=ptr(r['src']), out=ptr(r['out']), ids_out=ptr(r['ids']),
                                  p0=ptr(r['p0']), p1=ptr(r['p1'])) for r in rows)
        return torch.from_numpy(np.frombuffer(blob, dtype=np.int64).reshape(n_segs, _SEG_WORDS).copy()).to(dev)

    stream = _stream(verts[0])
    boxes_d = torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.float64)).to(dev)
    inbox = torch.empty(max(inbox_total, 1), dtype=torch.uint8, device=dev)
    flags = torch.empty(total + 1, dtype=torch.uint8, device=dev)
    pos = torch.empty(total + 1, dtype=torch.int32, device=dev)
    bounds = torch.empty(n_segs, C + 1, dtype=torch.int64, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    ws_bytes = lib.stin_crop_workspace_bytes(total)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    segs = table()
    _lib.check(lib.stin_crop_mark(_ptr(segs), n_segs, max_n, _ptr(boxes_d), C, total, inbox_total, _ptr(inbox), _ptr(flags), _ptr(pos),
                                  _ptr(bounds), _ptr(status), _ptr(ws), ws_bytes, stream), 'stin_crop_mark')
    bnd = bounds.cpu().numpy()                                     # the one read that sizes the outputs
    bnd = bnd - bnd[:, :1]
    # ---- outputs: every segment's crops back to back
    for i, r in enumerate(rows):
        n_out = int(bnd[i, C])
        if r['kind'] == _SEG_VERTICES:
            r['out'] = torch.empty(max(n_out, 1), r['width'], dtype=torch.float32, device=dev)
            r['ids'] = torch.empty(max(n_out, 1), dtype=torch.int64, device=dev)
        elif r['kind'] in (_SEG_EDGES, _SEG_DILATED):
            r['out'] = torch.empty(max(n_out, 1), 2, dtype=torch.int64, device=dev)
    for l, i in enumerate(tseg):
        nf, nc = int(bnd[vseg[l], C]), int(bnd[vseg[l + 1], C])
        rows[i]['out'] = torch.empty(max(nf, 1), dtype=torch.int64, device=dev)
        rows[i]['p0'] = torch.empty(max(nf, 1), dtype=torch.int32, device=dev)
        rows[i]['p1'] = torch.zeros(max(nc, 1), dtype=torch.uint8, device=dev)
    segs = table()
    _lib.check(lib.stin_crop_gather(_ptr(segs), n_segs, max_n, C, _ptr(flags), _ptr(pos), stream), 'stin_crop_gather')
    info = torch.zeros(max(L - 1, 1), C, 4, dtype=torch.int32, device=dev)
    if L > 1:
        _lib.check(lib.stin_crop_traces(_ptr(segs), n_segs, max_n, C, _ptr(flags), _ptr(pos), _ptr(info), _ptr(status), stream),
                   'stin_crop_traces')
    word = torch.cat([status, info.reshape(-1)]).cpu().numpy()     # the status word of the scene: read once
    if word[0] != 0:
        raise IndexError('an edge or dilated edge refers to a vertex outside its level')
    if word[1] != 0:
        raise IndexError('a trace refers to a vertex outside the next level')
    info_h = word[2:].reshape(max(L - 1, 1), C, 4)
    labels_flat = pooled[rows[vseg[0]]['ids'][:int(bnd[vseg[0], C])]] if pooled is not None else None
    out = []
    for c in range(C):
        def part(i, _c=c):
            return rows[i]['out'][int(bnd[i, _c]):int(bnd[i, _c + 1])]
        counts = [int(bnd[vseg[l], c + 1] - bnd[vseg[l], c]) for l in range(L)]
        if min(counts) == 0 or counts[-1] < min_coarsest:         # rejected by size: before the traces are looked at (:136)
            out.append((None, counts))
            continue
        ok = True
        tr = []
        for l in range(L - 1):
            if info_h[l, c, 1] == 0:                               # no fine vertex kept its target (the reference: IndexError)
                ok = False
                break
            t = rows[tseg[l]]['out'][int(bnd[vseg[l], c]):int(bnd[vseg[l], c + 1])]   # one entry per kept fine vertex
            if info_h[l, c, 2] != 0:                               # rare: a coarse vertex without predecessor -> host repair
                th = t.cpu().numpy().copy()
                if not _repair_trace(th, part(vseg[l]).cpu().numpy(), part(vseg[l + 1]).cpu().numpy()):
                    ok = False
                    break
                t = torch.from_numpy(th).to(dev)
            tr.append(t)
        if not ok:
            out.append((False, counts))
            continue
        crop = {'vertices': [part(vseg[l]) for l in range(L)], 'edges': [part(eseg[l]) for l in range(L)],
                'dilated_edges': [None if dseg[l] is None else [[] if i is None else part(i) for i in dseg[l]] for l in range(L)],
                'dilation_dists': saved.get('dilation_dists'), 'traces': tr}
        if labels_flat is not None:
            crop['labels'] = labels_flat[int(bnd[vseg[0], c]):int(bnd[vseg[0], c + 1])]
        kept = [rows[vseg[l]]['ids'][int(bnd[vseg[l], c]):int(bnd[vseg[l], c + 1])] for l in range(L)]
        out.append(((crop, kept), counts))
    return out


def crop_scene(saved, block_size=3.0, stride=1.5, positions=None, min_coarsest=MIN_NUM_MAXIMALLY_DECIMATED_VERTS,
               reference_dilated_labels=False, return_kept=False):
    """Training crops of one scene, the reference's preprocessing/crop_training_samples.py `process_frame` (:51-237), with every
    crop of the sampling grid cut in ONE batched pass on the GPU (the crop index is a grid dimension of the kernels).

    saved: the dict of a graphs/<scene>.pt file - vertices[L] (level 0: [N0, 10]), edges[L] [E, 2] int64, traces[L] (traces[0]
    maps the original mesh to level 0, traces[l + 1] level l to level l + 1), dilated_edges[L] (None or a list of [E_d, 2] tensors /
    empty lists), dilation_dists, optional labels (of the ORIGINAL mesh's vertices) - with its tensors on a CUDA device.
    -> [(counter, crop)]: crop has the keys and dtypes the reference writes (vertices float32; edges, traces, dilated_edges, labels
    int64; dilation_dists passed through), tensors on the device (views of one buffer per level and kind);
    scene_io.sample_from_tensors(crop, mask, end_level, cropped=True) takes it as it is.  return_kept=True: (counter, crop, kept)
    with kept[l] = the scene rows of the crop's level-l vertices (int64).

    Per grid position of crop_positions (x outer loop, y inner loop) the box is position -/+ block_size / 2 in float64, closed,
    z unbounded.  Per level: edges with both endpoints in the box, in their order; vertices = the endpoints of those edges,
    renumbered in their order; dilated rows between kept vertices; traces of kept targets relabelled, the others redirected to
    the kept coarse vertex nearest to the vertex's own position (float64, lowest index on a tie); coarse vertices left without a
    predecessor repaired as the reference does (ascending).  A crop with an empty level or fewer than min_coarsest vertices on the
    last one is left out, as is one that cannot be repaired or in which no vertex of a level keeps its target.
    counter: the number the reference puts into the file name - its block_counter advances by 1 per grid position and by 2 for a
    position rejected by the size rule (`block_counter += 1; continue` runs the `finally` increment as well); a crop skipped
    otherwise advances it by 1.  positions: explicit [(x, y)] centres instead of the grid; the counter is then the list index.
    reference_dilated_labels: relabel each dilated set by the rank among the vertices that occur in THAT filtered set - the
    reference's np.unique(..., return_inverse=True), which mislabels the set whenever a crop vertex has no dilated edge.  Off by
    default (the level's new ids, like data.collate(fix_dilated_offsets=True)); on for file parity."""
    import numpy as np
    v0 = saved['vertices'][0]
    if not all(torch.is_tensor(v) and v.is_cuda for v in saved['vertices']):
        raise TypeError('crop_scene runs on the GPU only (no CPU fallback exists)')
    if positions is None:
        xs, ys = crop_positions(v0, stride)
        centres = np.asarray([(x, y) for x in xs for y in ys], dtype=np.float64).reshape(-1, 2)
    else:
        centres = np.asarray([(float(x), float(y)) for x, y in positions], dtype=np.float64).reshape(-1, 2)
    if centres.shape[0] == 0:
        return []
    h = block_size / 2
    boxes = np.stack([centres[:, 0] - h, centres[:, 0] + h, centres[:, 1] - h, centres[:, 1] + h], 1)
    pooled = pooled_labels(saved['traces'][0], saved['labels'], v0.shape[0]) if 'labels' in saved else None   # once per scene
    per_crop = sum(2 * int(v.shape[0]) for v in saved['vertices']) + sum(int(e.numel()) // 2 for e in saved['edges'])
    for x in saved.get('dilated_edges') or []:
        per_crop += sum(int(s.numel()) // 2 + int(s.numel() > 0) * max(int(v.shape[0]) for v in saved['vertices'])
                        for s in (x or []) if torch.is_tensor(s))
    step = int(max(1, min(65535, (2 ** 31 - 16) // max(per_crop, 1))))     # flags of a pass are indexed with int32
    res = []
    for i in range(0, boxes.shape[0], step):
        res.extend(_crop_chunk(saved, boxes[i:i + step], pooled, bool(reference_dilated_labels), int(min_coarsest)))
    out, counter = [], 0
    for i, (what, counts) in enumerate(res):
        size_rejected = min(counts) == 0 or counts[-1] < int(min_coarsest)
        if not size_rejected and what:
            cnt = counter if positions is None else i
            out.append((cnt, what[0], what[1]) if return_kept else (cnt, what[0]))
        counter += 2 if size_rejected else 1
    return out


# ------------------------------------------------------------------------------------------------------------- graph levels
SCANNET_CLASS_REMAP = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 0, 13, 0, 14, 0, 0, 0, 0, 0, 0, 0, 15, 0, 0, 0, 16, 0, 0, 0, 0, 17, 18,
                       0, 19, 0, 0, 20, 0)      # nyu40 id -> ScanNet benchmark class (graph_level_generation.py:26-47)
_NEAREST_FLAGS = ((1, 'a query coordinate is not finite'), (2, 'a point coordinate is not finite'),
                  (4, 'a query index lies outside the query array'), (8, 'an id lies outside its vertex set'),
                  (16, 'a trace entry is unassigned or outside the coarse level'))


class LevelError(ValueError):
    """A decimator trace that the reference refuses (its QEMError / failed asserts in csv2npy)."""


def remap_scannet_labels(labels):
    """The ScanNet label fix of process_frame (:345-349): ids above 40 become 0, then SCANNET_CLASS_REMAP.  Tensor (any device) or
    array of ints -> int64 of the same kind."""
    if torch.is_tensor(labels):
        ids = labels.long()
        ids = torch.where(ids > 40, torch.zeros_like(ids), ids)
        return torch.tensor(SCANNET_CLASS_REMAP, dtype=torch.int64, device=ids.device)[ids]
    import numpy as np
    ids = np.asarray(labels).astype(np.int64)
    ids = np.where(ids > 40, 0, ids)
    return np.asarray(SCANNET_CLASS_REMAP, dtype=np.int64)[ids]


def _flag_text(word):
    return '; '.join(t for b, t in _NEAREST_FLAGS if word & b)


def _xyz64(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise TypeError('%s must be a CUDA tensor (no CPU fallback exists)' % what)
    if t.dtype not in (torch.float32, torch.float64):
        raise TypeError('%s must be float32 or float64' % what)
    if t.dim() != 2 or t.shape[1] < 3:
        raise ValueError('%s must be [N, >= 3]' % what)
    return t[:, :3].double().contiguous()


def _nearest_launch(q64, p64, out, flags, q_index=None, q_count=None, n_queries=None, chunks=None, d2=None):
    """stin_nearest_f64 on fp64 [., 3] tensors; nothing synchronises.  flags: an int64 device word (OR-ed)."""
    lib = _lib.load()
    nq = int(q64.shape[0]) if n_queries is None else int(n_queries)
    P = int(p64.shape[0])
    if nq == 0:
        return
    if P == 0:
        raise ValueError('nearest: no points to search')
    c = int(chunks) if chunks is not None else int(lib.stin_nearest_chunks(nq, P))
    ws_bytes = lib.stin_nearest_workspace_bytes(nq, c)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=q64.device)
    _lib.check(lib.stin_nearest_f64(_ptr(q64), int(q64.shape[0]), _ptr(p64), P, _ptr(q_index), _ptr(q_count), nq, c, _ptr(out), _ptr(d2),
                                    _ptr(flags), _ptr(ws), ws_bytes, _stream(q64)), 'stin_nearest_f64')


def nearest(queries, points, return_sq_dist=False, chunks=None):
    """Exact nearest neighbour: for every row of queries [Q, >= 3] the index (int64 [Q], CUDA) of the nearest row of points
    [P, >= 3], by d = (dx dx + dy dy) + dz dz in fp64 (float32 input is promoted), the lowest index on a tie - numpy's argmin of
    the same expression, which is what sklearn's BallTree.query(k=1) answers in the reference whenever the nearest point is unique.
    Tiled brute force (stin_nearest_f64).  return_sq_dist: also the squared distances (float64 [Q]).  chunks: parts the points
    are cut into (default: chosen from Q and the device's CU count).  ValueError for P == 0 or non-finite coordinates."""
    q64, p64 = _xyz64(queries, 'queries'), _xyz64(points, 'points')
    nq = int(q64.shape[0])
    out = torch.empty(nq, dtype=torch.int64, device=q64.device)
    d2 = torch.empty(nq, dtype=torch.float64, device=q64.device) if return_sq_dist else None
    if nq:
        flags = torch.zeros(1, dtype=torch.int64, device=q64.device)
        _nearest_launch(q64, p64, out, flags, chunks=chunks, d2=d2)
        word = int(flags.item())
        if word:
            raise ValueError('nearest: ' + _flag_text(word))
    return (out, d2) if return_sq_dist else out


def _check_k(k, what):
    kmax = _lib.CONSTANTS['STIN_KNN_MAX_K']
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= kmax:
        raise ValueError('%s: k must be an integer in [1, %d]' % (what, kmax))
    return int(k)


def _knn_launch(q64, p64, k, idx, d2, flags, p_valid=None, q_index=None, chunks=None):
    """stin_knn_f64 on fp64 [., 3] tensors into idx int64 [rows, k] / d2 float64 [rows, k] (or None); nothing synchronises."""
    lib = _lib.load()
    nq = int(q64.shape[0]) if q_index is None else int(q_index.numel())
    P = int(p64.shape[0])
    if nq == 0:
        return
    c = int(chunks) if chunks is not None else int(lib.stin_knn_chunks(nq, P, k))
    ws_bytes = lib.stin_knn_workspace_bytes(nq, c, k)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=q64.device)
    _lib.check(lib.stin_knn_f64(_ptr(q64), int(q64.shape[0]), _ptr(p64) if P else None, _ptr(p_valid), P, _ptr(q_index), None, nq, k, c,
                                _ptr(idx), _ptr(d2), _ptr(flags), _ptr(ws), ws_bytes, _stream(q64)), 'stin_knn_f64')


def _knn_mean_launch(values, idx, out, filled=None, q_index=None):
    """stin_knn_mean_f32: values float32 [P, C] (rows may be strided), idx int64 [rows, k], out float32 [rows, C]."""
    lib = _lib.load()
    nq = int(idx.shape[0]) if q_index is None else int(q_index.numel())
    _lib.check(lib.stin_knn_mean_f32(_ptr(values), int(values.stride(0)), int(values.shape[0]), int(values.shape[1]), _ptr(idx),
                                     int(idx.shape[1]), _ptr(q_index), None, nq, int(idx.shape[0]), _ptr(out), int(out.stride(0)),
                                     _ptr(filled), _stream(values)), 'stin_knn_mean_f32')


def _point_valid(point_valid, n, device, what):
    if point_valid is None:
        return None
    if not torch.is_tensor(point_valid) or not point_valid.is_cuda:
        raise TypeError('%s must be a CUDA tensor (no CPU fallback exists)' % what)
    if point_valid.dim() != 1 or int(point_valid.numel()) != n:
        raise ValueError('%s needs one entry per point' % what)
    return (point_valid != 0).to(device=device, dtype=torch.uint8).contiguous()


def knn(queries, points, k, point_valid=None, query_index=None, return_sq_dist=False, chunks=None):
    """Exact k nearest neighbours: for every row of queries [Q, >= 3] the indices (int64 [Q, k], CUDA) of its k nearest rows of
    points [P, >= 3] by d = (dx dx + dy dy) + dz dz in fp64 (float32 input is promoted), ascending under (d, index): the lowest
    index first among equal distances - np.argsort(d, kind='stable')[:k].  point_valid ([P], bool or integer, non-zero = a candidate):
    the other points are skipped IN PLACE - their indices are never reported, their coordinates never read, and the indices stay
    those of the full array.  Fewer than k candidates (P == 0 and no valid point included): the remaining slots hold -1 (and inf).
    query_index (int64 [M]): only these rows are searched, the rows not listed hold -1 / inf.  return_sq_dist: also the squared
    distances (float64 [Q, k]).  chunks: parts the points are cut into (default: from Q, k and the device's CU count; the result
    does not depend on it).  Tiled brute force with the k-list in registers (stin_knn_f64; include/stin_hip.h, "k nearest
    neighbours").  ValueError for k outside [1, STIN_KNN_MAX_K], non-finite queries or valid points, or a row id out of range."""
    k = _check_k(k, 'knn')
    q64, p64 = _xyz64(queries, 'queries'), _xyz64(points, 'points')
    nq, dev = int(q64.shape[0]), q64.device
    valid = _point_valid(point_valid, int(p64.shape[0]), dev, 'point_valid')
    qi = None
    if query_index is not None:
        if not torch.is_tensor(query_index) or not query_index.is_cuda:
            raise TypeError('query_index must be a CUDA tensor (no CPU fallback exists)')
        qi = query_index.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    idx = torch.full((nq, k), -1, dtype=torch.int64, device=dev)        # (what a row that is not listed keeps)
    d2 = torch.full((nq, k), float('inf'), dtype=torch.float64, device=dev) if return_sq_dist else None
    if nq == 0 and qi is not None and qi.numel():
        raise ValueError('knn: ' + _flag_text(4))
    if nq:
        flags = torch.zeros(1, dtype=torch.int64, device=dev)
        _knn_launch(q64, p64, k, idx, d2, flags, p_valid=valid, q_index=qi, chunks=chunks)
        word = int(flags.item())
        if word:
            raise ValueError('knn: ' + _flag_text(word))
    return (idx, d2) if return_sq_dist else idx


def fill_unseen_colors(vertices, colors, count, k=3, min_count=1, return_filled=False):
    """The fill of unseen vertices that Open3D's colour-map pipeline ends with, as a step of its own: a vertex with count <
    min_count gets the mean colour of its k nearest SEEN vertices (count >= min_count) - knn with point_valid = seen, then per
    channel (float)((((double)c1 + (double)c2) + ...) / m) over the m <= k neighbours found, nearest first (stin_knn_mean_f32).
    vertices [N, >= 3] float CUDA; colors float32 [N, C], C <= 16 (any value range); count [N] integer (FrameColors' count).
    -> a new colours tensor whose seen rows are bit-identical to the input; return_filled: also bool [N], true for the rows that
    were written.  No seen vertex: the input comes back unchanged (nothing is filled).  k = 3 is Open3D's default
    (invisible_vertex_color_knn) to our knowledge; this is the project's own contract, not pinned against an Open3D run."""
    k = _check_k(k, 'fill_unseen_colors')
    v64 = _xyz64(vertices, 'vertices')
    n, dev = int(v64.shape[0]), v64.device
    if not torch.is_tensor(colors) or not colors.is_cuda or not torch.is_tensor(count) or not count.is_cuda:
        raise TypeError('colors and count must be CUDA tensors (no CPU fallback exists)')
    if colors.dtype != torch.float32:
        raise TypeError('colors must be float32')
    cmax = _lib.CONSTANTS['STIN_KNN_MAX_C']
    if colors.dim() != 2 or int(colors.shape[0]) != n or not 1 <= int(colors.shape[1]) <= cmax:
        raise ValueError('colors must be [N, C] with 1 <= C <= %d' % cmax)
    if count.dim() != 1 or int(count.numel()) != n or count.dtype.is_floating_point:
        raise ValueError('count must be an integer tensor with one entry per vertex')
    out = colors.to(dev).clone(memory_format=torch.contiguous_format)
    seen = count.to(dev) >= int(min_count)
    filled = torch.zeros(n, dtype=torch.uint8, device=dev)
    todo = torch.nonzero(~seen).reshape(-1)
    if int(todo.numel()) and int(todo.numel()) < n:
        idx = torch.empty(n, k, dtype=torch.int64, device=dev)
        flags = torch.zeros(1, dtype=torch.int64, device=dev)
        _knn_launch(v64, v64, k, idx, None, flags, p_valid=seen.to(torch.uint8), q_index=todo)
        # in place: the listed rows (unseen) and the rows that are read (seen) are disjoint
        _knn_mean_launch(out, idx, out, filled=filled, q_index=todo)
        word = int(flags.item())
        if word:
            raise ValueError('fill_unseen_colors: ' + _flag_text(word))
    return (out, filled.bool()) if return_filled else out


def knn_inpaint(sample, k=3):
    """The non-learned inpainting baseline: every masked vertex (mask > 0) of a training sample gets the mean colour of its k
    nearest known vertices (mask == 0).  sample: the tuple (positions [N, >= 3], color [N, C], mask [N] or [N, 1]) of level 0, or a
    training sample with `color`, `mask` and its positions in `pos` or, failing that, in x[:, 6:9] (the reference's feature
    layout: rgb, normal, position, known; a uniform scale of the positions does not change who is nearest beyond rounding).
    -> the composite float32 [N, C]: `color` itself outside the mask, bit for bit - what StepMetrics.update accepts as `out`
    (composite=True and False alike), so the baseline's l1 / psnr stand beside the network's.  A few lines on fill_unseen_colors."""
    if isinstance(sample, (tuple, list)):
        pos, color, mask = sample
    else:
        pos = getattr(sample, 'pos', None)
        pos, color, mask = (sample.x[:, 6:9] if pos is None else pos), sample.color, sample.mask
    known = (mask.reshape(-1) == 0).to(torch.int32)
    return fill_unseen_colors(pos, color.float(), known, k=k)


def read_trace_csv(path):
    """The decimator's trace file (host): `;`-separated ragged rows `new xyz; old xyz; old xyz; ...`, a row with zero old
    coordinates allowed, empty lines skipped.  -> (new_xyz float64 [R, 3], old_xyz float64 [T, 3], row_ptr int64 [R + 1]) numpy
    arrays; row r names old_xyz[row_ptr[r]:row_ptr[r + 1]].  As csv2npy (:147-161): the first three fields are the new vertex,
    len(row) // 3 - 1 triples follow (trailing fields short of a triple - a `;` at the end of the line - are ignored)."""
    import numpy as np
    new, old, ptr = [], [], [0]
    with open(path, 'r') as f:
        for line in f:
            line = line.rstrip('\r\n')
            if not line:
                continue
            row = line.split(';')
            new.append([float(r) for r in row[:3]])
            for i in range(len(row) // 3 - 1):
                old.append([float(r) for r in row[3 + 3 * i:6 + 3 * i]])
            ptr.append(len(old))
    return (np.asarray(new, dtype=np.float64).reshape(-1, 3), np.asarray(old, dtype=np.float64).reshape(-1, 3),
            np.asarray(ptr, dtype=np.int64))


def _fill_unassigned(new64, old64, trace, state):
    """trace (int64 [n_old], -1 = unassigned, modified in place): every unassigned old vertex goes to its nearest new vertex.
    state: int64 [5] device vector ([3] flag word, [4] receives the unassigned count).  Nothing synchronises."""
    lib = _lib.load()
    n_old = int(trace.numel())
    if n_old == 0:
        return
    todo = torch.empty(n_old, dtype=torch.int64, device=trace.device)
    _lib.check(lib.stin_trace_unassigned_i64(_ptr(trace), n_old, _ptr(todo), _ptr(state), _stream(trace)), 'stin_trace_unassigned_i64')
    _nearest_launch(old64, new64, trace, state[3:4], q_index=todo, q_count=state[4:5], n_queries=n_old)


def fill_unassigned_trace(new_coords, old_coords, trace):
    """The reference's nearest_neighbor_interpolation_for_unassigned_traces (:284-295): entries of trace (int [n_old]) equal to
    -1 become the index of the new vertex nearest to that old vertex; the others are kept.  -> int64 [n_old] (a new tensor)."""
    new64, old64 = _xyz64(new_coords, 'new_coords'), _xyz64(old_coords, 'old_coords')
    out = trace.to(device=old64.device, dtype=torch.int64).clone().contiguous()
    if out.numel() != old64.shape[0]:
        raise ValueError('trace needs one entry per old vertex')
    state = torch.zeros(5, dtype=torch.int64, device=old64.device)
    if new64.shape[0] == 0:
        if bool((out == -1).any()):
            raise LevelError('unassigned old vertices and no new vertex to send them to')
        return out
    _fill_unassigned(new64, old64, out, state)
    word = int(state[3].item())
    if word:
        raise LevelError('fill_unassigned_trace: ' + _flag_text(word))
    return out


def trace_from_csv(csv, old_vertices, new_vertices):
    """The reference's csv2npy (:135-191) on the GPU: the fine -> coarse trace (int64 [n_old], CUDA) of one decimation from the
    decimator's trace file.  csv: a path or the (new_xyz, old_xyz, row_ptr) of read_trace_csv.
    1. every row's new coordinate -> its nearest vertex of new_vertices; 2. every old coordinate -> its nearest vertex of
    old_vertices (two `nearest` calls instead of one BallTree query per coordinate); 3. trace[old] = new, scattered; 4. every
    old vertex that no row names goes to its nearest new vertex.  LevelError where the reference raises QEMError or trips an
    assert: an old vertex named by two entries; a row that resolves to a new vertex which an earlier row WITH old vertices
    already took (an earlier row without any is tolerated); a new vertex that no row and no old vertex reaches.  All
    conditions are gathered in one device vector that is read once, after the last launch."""
    import numpy as np
    lib = _lib.load()
    old64, new64 = _xyz64(old_vertices, 'old_vertices'), _xyz64(new_vertices, 'new_vertices')
    dev = old64.device
    new_xyz, old_xyz, row_ptr = read_trace_csv(csv) if isinstance(csv, (str, bytes)) or hasattr(csv, '__fspath__') else csv
    new_xyz = np.ascontiguousarray(new_xyz, dtype=np.float64).reshape(-1, 3)
    old_xyz = np.ascontiguousarray(old_xyz, dtype=np.float64).reshape(-1, 3)
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64)
    R, n_ent, n_old, n_new = int(new_xyz.shape[0]), int(old_xyz.shape[0]), int(old64.shape[0]), int(new64.shape[0])
    if row_ptr.shape[0] != R + 1 or int(row_ptr[-1]) != n_ent or row_ptr[0] != 0 or np.any(np.diff(row_ptr) < 0):
        raise ValueError('row_ptr does not describe the rows')
    if n_new == 0 or n_old == 0:
        raise LevelError('a level without vertices')
    row_of = np.repeat(np.arange(R, dtype=np.int64), np.diff(row_ptr))
    rp_d, ro_d = torch.from_numpy(row_ptr).to(dev), torch.from_numpy(row_of).to(dev)
    state = torch.empty(5, dtype=torch.int64, device=dev)
    trace = torch.empty(n_old, dtype=torch.int64, device=dev)
    new_id = torch.empty(R, dtype=torch.int64, device=dev)
    old_id = torch.empty(n_ent, dtype=torch.int64, device=dev)
    ws_bytes = lib.stin_trace_workspace_bytes(n_old, n_new)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    first = torch.zeros(1, dtype=torch.int64, device=dev)              # flag word of the two matching passes
    _nearest_launch(torch.from_numpy(new_xyz).to(dev), new64, new_id, first)
    _nearest_launch(torch.from_numpy(old_xyz).to(dev), old64, old_id, first)
    _lib.check(lib.stin_trace_scatter_i64(_ptr(new_id), _ptr(rp_d), R, _ptr(old_id), _ptr(ro_d), n_ent, n_old, n_new, _ptr(trace),
                                          _ptr(state), _ptr(ws), ws_bytes, _stream(trace)), 'stin_trace_scatter_i64')
    _fill_unassigned(new64, old64, trace, state)
    _lib.check(lib.stin_trace_check_i64(_ptr(trace), n_old, _ptr(rp_d), R, n_new, _ptr(state), _ptr(ws), ws_bytes, _stream(trace)),
               'stin_trace_check_i64')
    st = torch.cat([state, first]).cpu().tolist()                      # the one read
    word = int(st[3]) | int(st[5])
    if word & ~16:
        raise LevelError('trace_from_csv: ' + _flag_text(word & ~16))
    if st[1]:
        raise LevelError('trace_from_csv: %d new vertices are matched by a row after an earlier row with old vertices' % st[1])
    if st[2]:
        raise LevelError('trace_from_csv: %d new vertices are reached by no row and no old vertex' % st[2])
    if st[0]:
        raise LevelError('trace_from_csv: %d old vertices are named by more than one entry' % st[0])
    if word:
        raise LevelError('trace_from_csv: ' + _flag_text(word))
    return trace


def colors_and_labels(original_vertices, level_coords):
    """The reference's get_color_and_labels (:98-116): for each entry of level_coords ([N_l, >= 3] positions) the columns 3: of the
    nearest row of original_vertices ([N, 3 + C]: position first) - one `nearest` per level and a gather.
    -> list of [N_l, C] tensors in original_vertices' dtype."""
    return [c for c, _ in _colors_and_labels(original_vertices, level_coords)]


def _colors_and_labels(original_vertices, level_coords):
    out = []
    for c in level_coords:
        idx = nearest(c, original_vertices)
        out.append((original_vertices[idx][:, 3:], idx))
    return out


def _cluster_level_f32(coords32, edge_index, voxel_size):
    """vertex_clustering for a level whose positions are float32 (every level after the first in the reference's vertex-clustering
    mode): numpy evaluates `coords // voxel_size` and the centres of gravity in float32 there, so the voxel size is rounded to
    float32 and the means are accumulated in float32, member after member (stin_cluster_mean_f32)."""
    import numpy as np
    lib = _lib.load()
    _, trace, ce = vertex_clustering(coords32, edge_index, float(np.float32(voxel_size)))
    n = int(trace.numel())
    order = torch.sort(trace, stable=True).indices.contiguous()
    nc = int(trace.max()) + 1 if n else 0
    seg = torch.zeros(nc + 1, dtype=torch.int64, device=trace.device)
    if n:
        seg[1:] = torch.cumsum(torch.bincount(trace, minlength=nc), 0)
    c32 = coords32.float().contiguous()
    out = torch.empty(max(nc, 1), 3, dtype=torch.float32, device=trace.device)
    _lib.check(lib.stin_cluster_mean_f32(_ptr(c32), n, _ptr(order), _ptr(seg), nc, _ptr(out), _stream(c32)), 'stin_cluster_mean_f32')
    return out[:nc], trace, ce


def _mesh_edges(faces, n):
    """[E, 2] int64 rows (vertex, neighbour) of a triangle mesh, sorted by (row 0, row 1): the reference's edges_from_faces +
    flattening, whose order inside a vertex group is a CPython set order."""
    return edges_from_faces(faces, n).t().contiguous()


# ------------------------------------------------------------------------------------------------------------- QEM decimation
def _rowptr(sorted_keys, n):
    rp = torch.zeros(n + 1, dtype=torch.int64, device=sorted_keys.device)
    if sorted_keys.numel():
        rp[1:] = torch.cumsum(torch.bincount(sorted_keys, minlength=n), 0)
    return rp


def _half_edges(faces, n):
    """Faces [F, 3] int64 (checked) -> (keys i n + j of the unique undirected edges (i < j), ascending; faces per edge; a face of
    each edge - THE face of a boundary edge)."""
    a = torch.cat([faces[:, 0], faces[:, 1], faces[:, 2]])
    b = torch.cat([faces[:, 1], faces[:, 2], faces[:, 0]])
    keys, order = torch.sort(torch.minimum(a, b) * n + torch.maximum(a, b), stable=True)
    uniq, counts = torch.unique_consecutive(keys, return_counts=True)
    start = torch.cumsum(counts, 0) - counts
    return uniq, counts, order[start] % max(int(faces.shape[0]), 1)


def _vertex_faces(faces, n):
    """-> (rowptr [n + 1], face ids): the faces of every vertex in ascending face id."""
    flat, order = torch.sort(faces.reshape(-1), stable=True)
    return _rowptr(flat, n), (order // 3).contiguous()


def _checked_faces(faces, n, what):
    """int64 [F, 3] copy of `faces` without the faces that repeat a vertex; IndexError (from a device status word: nothing reads
    through the indices before) when one lies outside [0, n)."""
    lib = _lib.load()
    f = faces.long().reshape(-1, 3).contiguous().clone()
    keep = torch.empty(max(f.shape[0], 1), dtype=torch.uint8, device=f.device)
    status = torch.zeros(1, dtype=torch.int32, device=f.device)
    _lib.check(lib.stin_qem_remap_faces_i64(_ptr(f), int(f.shape[0]), None, int(n), _ptr(keep), _ptr(status), _stream(f)),
               'stin_qem_remap_faces_i64')
    if int(status.item()) != 0:
        raise IndexError('%s: a face refers to a vertex outside [0, %d)' % (what, n))
    return f[keep[:f.shape[0]].bool()]


def vertex_normals(vertices, faces):
    """Vertex normals [N, 3] float64 of a triangle mesh (vertices [N, >= 3] float, faces [F, 3] int; CUDA) by the rule open3d
    documents for compute_vertex_normals: the UNIT normals of a vertex's faces are summed (here in ascending face id, a fixed-order
    segmented sum: stin_qem_vertex_sum_f64) and the sum is normalised; a zero sum - no face, or only zero-area ones - gives
    (0, 0, 1).  This is the documented rule only: open3d is not available to pin it against the library itself."""
    v = _xyz64(vertices, 'vertices')
    if not (torch.is_tensor(faces) and faces.is_cuda):
        raise TypeError('faces must be a CUDA tensor (no CPU fallback exists)')
    lib = _lib.load()
    n = int(v.shape[0])
    f = _checked_faces(faces, n, 'vertex_normals')
    nf = int(f.shape[0])
    out = torch.empty(max(n, 1), 3, dtype=torch.float64, device=v.device)[:n]
    fn = torch.empty(max(nf, 1), 3, dtype=torch.float64, device=v.device)
    _lib.check(lib.stin_qem_face_quadrics_f64(_ptr(v), n, _ptr(f), nf, None, _ptr(fn), _stream(v)), 'stin_qem_face_quadrics_f64')
    rp, col = _vertex_faces(f, n)
    _lib.check(lib.stin_qem_vertex_sum_f64(_ptr(rp), _ptr(col), int(col.numel()), _ptr(fn), nf, 3, n, _ptr(out), 0, 1, _stream(v)),
               'stin_qem_vertex_sum_f64')
    return out


class _Stages:
    """Wall time per stage of decimate_qem when a `profile` dict is given (each stage is bracketed by a device synchronisation)."""

    def __init__(self, profile):
        self.profile, self.name, self.t0 = profile, None, 0.0

    def __call__(self, name):
        if self.profile is None:
            return
        import time
        torch.cuda.synchronize()
        now = time.perf_counter()
        if self.name is not None:
            self.profile[self.name] = self.profile.get(self.name, 0.0) + (now - self.t0)
        self.name, self.t0 = name, now


def decimate_qem(vertices, faces, percent=None, n_vertices=None, strict=False, profile=None):
    """Quadric-error-metric edge-collapse decimation on the GPU (csrc/stin_qem.hip) - the step the reference shells out to vcglib's
    tridecimator for - deterministic, parallel, and with the fine -> coarse trace as a result (no CSV, no nearest-neighbour search).
    vertices [N, >= 3] float, faces [F, 3] int (CUDA); percent (of the vertices to keep) or n_vertices.
    -> (vertices' float64 [N', 3], faces' int64 [F', 3], trace int64 [N] onto [0, N'), N').

    Target: n_vertices, else max(3, N * percent // 100) (the rounding of the reference's decimator fork is unknown).  The contract
    (include/stin_hip.h, "QEM"; restated in numpy by the test suite, which this reproduces bit for bit), fp64 throughout:
    * quadrics: per face area p p^T (p = unit plane), per boundary edge |e|^2 q q^T (q = the plane through the edge, perpendicular to
      its face) on both endpoints; Q_v = the faces of v in ascending id, then its boundary edges in ascending (min, max) order.
    * a round, on the unmodified mesh: candidates = the unique edges (i < j) ordered by (i, j); Q = Q_i + Q_j; placement by Cramer's
      rule when |det A| > 1e-10 max|A|^3 and |x - mid| <= |v_i - v_j|, else the cheapest of v_i, v_j, mid; cost = max(h^T Q h, 0).
      Valid: finite cost, link condition (common neighbours == faces on the edge, at most two) and flip condition (every other face
      of i or j keeps n_old . n_new > 0.2 |n_old| |n_new|; a zero-area face blocks).  Selected: the minimum in the order (cost, i, j)
      among all valid edges with an endpoint in N[i] | N[j] - so no two selected edges touch or neighbour each other - and, when
      more are selected than vertices are left to remove, the first of them in that order.
    * collapse: j merges into i, v_i = x, Q_i += Q_j; faces are remapped, those with a repeated vertex dropped, the others keep
      their relative order and orientation.  Stop at the target or when a round selects nothing.
    * new ids are the ranks of the surviving original ids; vertices that no face references never collapse and count.
    Faces of the input that repeat a vertex are dropped at once.  strict: LevelError when N' > target.  IndexError for a face index
    outside [0, N) (a device status word, read before anything indexes with it).  One host read per round (the selected count); the
    sorts of a round (unique edges, neighbour and face lists) are torch's.  profile: a dict that receives 'rounds', 'n_target' and
    the wall seconds per stage ('structures', 'edges', 'select', 'collapse', 'remap')."""
    v = _xyz64(vertices, 'vertices').clone()
    if not (torch.is_tensor(faces) and faces.is_cuda):
        raise TypeError('faces must be a CUDA tensor (no CPU fallback exists)')
    if (percent is None) == (n_vertices is None):
        raise ValueError('give percent or n_vertices')
    lib = _lib.load()
    n, dev, stream = int(v.shape[0]), v.device, _stream(v)
    if n >= 2 ** 31:
        raise ValueError('too many vertices')
    n_target = int(n_vertices) if n_vertices is not None else max(3, n * int(percent) // 100)
    stage = _Stages(profile)
    stage('setup')
    f = _checked_faces(faces, n, 'decimate_qem')
    # ---- vertex quadrics: faces in ascending id, then boundary edges in ascending (min, max)
    Q = torch.zeros(max(n, 1), 10, dtype=torch.float64, device=dev)
    nf = int(f.shape[0])
    if nf:
        Kf = torch.empty(nf, 10, dtype=torch.float64, device=dev)
        fn = torch.empty(nf, 3, dtype=torch.float64, device=dev)
        _lib.check(lib.stin_qem_face_quadrics_f64(_ptr(v), n, _ptr(f), nf, _ptr(Kf), _ptr(fn), stream), 'stin_qem_face_quadrics_f64')
        rp, col = _vertex_faces(f, n)
        _lib.check(lib.stin_qem_vertex_sum_f64(_ptr(rp), _ptr(col), int(col.numel()), _ptr(Kf), nf, 10, n, _ptr(Q), 0, 0, stream),
                   'stin_qem_vertex_sum_f64')
        keys, counts, first = _half_edges(f, n)
        b = counts == 1
        bi, bj, bf = (keys[b] // n).contiguous(), (keys[b] % n).contiguous(), first[b].contiguous()
        nb = int(bi.numel())
        if nb:
            Kb = torch.empty(nb, 10, dtype=torch.float64, device=dev)
            _lib.check(lib.stin_qem_boundary_quadrics_f64(_ptr(v), n, _ptr(bi), _ptr(bj), _ptr(bf), nb, _ptr(fn), nf, _ptr(Kb), stream),
                       'stin_qem_boundary_quadrics_f64')
            ids = torch.arange(nb, dtype=torch.int64, device=dev)
            vk = torch.sort(torch.cat([bi, bj]) * nb + torch.cat([ids, ids])).values
            rp, col = _rowptr(vk // nb, n), (vk % nb).contiguous()
            _lib.check(lib.stin_qem_vertex_sum_f64(_ptr(rp), _ptr(col), int(col.numel()), _ptr(Kb), nb, 10, n, _ptr(Q), 1, 0, stream),
                       'stin_qem_vertex_sum_f64')
    parent = torch.arange(n, dtype=torch.int64, device=dev)
    m1 = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    m2 = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    n_cur, rounds = n, 0
    while n_cur > n_target and f.shape[0]:
        stage('structures')
        keys, counts, _ = _half_edges(f, n)
        ei, ej = (keys // n).contiguous(), (keys % n).contiguous()
        E, nf = int(ei.numel()), int(f.shape[0])
        k2, order = torch.sort(torch.cat([keys, ej * n + ei]), stable=True)
        nrp, ncol, neid = _rowptr(k2 // n, n), (k2 % n).contiguous(), (order % E).contiguous()
        frp, fface = _vertex_faces(f, n)
        x = torch.empty(E, 3, dtype=torch.float64, device=dev)
        cost = torch.empty(E, dtype=torch.float64, device=dev)
        valid = torch.empty(E, dtype=torch.uint8, device=dev)
        sel = torch.empty(E, dtype=torch.uint8, device=dev)
        stage('edges')
        _lib.check(lib.stin_qem_edges_f64(_ptr(v), _ptr(Q), n, _ptr(ei), _ptr(ej), _ptr(counts), E, _ptr(nrp), _ptr(ncol), int(ncol.numel()),
                                          _ptr(frp), _ptr(fface), int(fface.numel()), _ptr(f), nf, _ptr(x), _ptr(cost), _ptr(valid),
                                          stream), 'stin_qem_edges_f64')
        stage('select')
        _lib.check(lib.stin_qem_select_i64(_ptr(ei), _ptr(ej), E, _ptr(nrp), _ptr(ncol), _ptr(neid), int(ncol.numel()), _ptr(cost),
                                           _ptr(valid), n, _ptr(m1), _ptr(m2), _ptr(sel), stream), 'stin_qem_select_i64')
        ids = torch.nonzero(sel).reshape(-1)                              # (the round's host read: how many were selected)
        if ids.numel() == 0:
            break
        if ids.numel() > n_cur - n_target:                                # the first of them in the order (cost, edge id)
            ids = ids[torch.sort(cost[ids], stable=True).indices[:n_cur - n_target]].contiguous()
        stage('collapse')
        _lib.check(lib.stin_qem_collapse_f64(_ptr(ids), int(ids.numel()), _ptr(ei), _ptr(ej), E, _ptr(x), _ptr(v), _ptr(Q), _ptr(parent),
                                             n, stream), 'stin_qem_collapse_f64')
        stage('remap')
        keep = torch.empty(nf, dtype=torch.uint8, device=dev)
        _lib.check(lib.stin_qem_remap_faces_i64(_ptr(f), nf, _ptr(parent), n, _ptr(keep), _ptr(status), stream),
                   'stin_qem_remap_faces_i64')
        f = f[keep.bool()]
        n_cur -= int(ids.numel())
        rounds += 1
    stage('finish')
    alive = parent == torch.arange(n, dtype=torch.int64, device=dev)
    rank = (torch.cumsum(alive.long(), 0) - 1).contiguous()
    trace = torch.empty(n, dtype=torch.int64, device=dev)
    _lib.check(lib.stin_qem_trace_i64(_ptr(parent), _ptr(rank), n, _ptr(trace), _ptr(status), stream), 'stin_qem_trace_i64')
    if int(status.item()) != 0:
        raise RuntimeError('decimate_qem: inconsistent merge state (status %d)' % int(status.item()))
    stage(None)
    if profile is not None:
        profile['rounds'], profile['n_target'] = rounds, n_target
    if strict and n_cur > n_target:
        raise LevelError('decimate_qem: %d vertices left, %d asked for (no valid collapse remains)' % (n_cur, n_target))
    return v[alive], rank[f], trace, n_cur


def _cluster_faces_torch(f, trace):
    """cluster_mesh's faces without stin_face_cluster_i64 (more than 2^21 clusters: three ids do not fit its key) - the same rule
    with torch's sorts, the same result."""
    img = trace[f]
    ids = torch.nonzero((img[:, 0] != img[:, 1]) & (img[:, 1] != img[:, 2]) & (img[:, 0] != img[:, 2])).reshape(-1)
    if ids.numel() == 0:
        return img[:0]
    _, inverse = torch.unique(torch.sort(img[ids], dim=1).values, dim=0, return_inverse=True)
    order = torch.sort(inverse, stable=True).indices                       # runs of one vertex set, ascending face id inside
    run = inverse[order]
    head = torch.ones_like(run, dtype=torch.bool)
    head[1:] = run[1:] != run[:-1]
    return img[torch.sort(ids[order[head]]).values]


def cluster_mesh(vertices, faces, cell_size, profile=None, _torch_faces=False):
    """Voxel clustering of a triangle mesh that keeps it a triangle mesh (csrc/stin_cluster.hip) - the step the reference shells out
    to vcglib's trimesh_clustering for (a --qem level that is no digit string, `--level_params 0.04 30 30 30`) - so that QEM levels
    can follow it.  vertices [N, >= 3] float, faces [F, 3] int (CUDA); cell_size finite and > 0.
    -> (vertices' float64 [N', 3], faces' int64 [F', 3], trace int64 [N] onto [0, N'), N').

    The contract (include/stin_hip.h, "Mesh clustering"; restated in numpy by the test suite, which this reproduces bit for bit) is
    this project's own.  It is NOT pinned against vcglib, which is not available, and differs from it on purpose in two places: the
    grid origin is 0, as in the reference's own python vertex_clustering (vcglib anchors the grid on an inflated bounding box), and
    a cell's position is the unweighted mean of its members (vcglib averages with face-corner weights).  fp64 throughout:
    * faces of the input are range-checked; those that repeat a vertex are dropped at once (as decimate_qem does).
    * cells: the bin of a vertex is numpy's `coords // cell_size` per axis; cluster ids are the ranks of the bin triples in
      lexicographic order (np.unique(bins, axis=0)).  ALL N vertices are clustered, referenced by a face or not, so trace and N' are
      bitwise those of vertex_clustering(vertices, edges, cell_size).
    * positions: per cluster the members' coordinates summed in ascending vertex id from 0.0 and divided by the count with one IEEE
      division; vertices'.float() is bitwise vertex_clustering's new_coords.
    * faces: the image of a face is trace[face], corner order kept; images with two equal corners are dropped; among images with
      the same vertex SET only the one of the lowest input face id survives, with that face's orientation; survivors keep their
      relative input order.
    Clusters that no surviving face references stay: they count in N' and have no edges.  The result may be non-manifold (an edge
    with more than two faces); decimate_qem's link condition leaves such edges alone.
    TypeError for CPU input, IndexError for a face index outside [0, N) (a device status word, read before anything indexes with
    it), ValueError for a non-finite coordinate, a cell_size that is not finite and > 0, or more than 2^21 cells along an axis.
    With more than 2^21 clusters the faces go through torch's sorts instead of stin_face_cluster_i64 (the same result).
    profile: a dict that receives the wall seconds per stage ('faces_in', 'cells', 'faces')."""
    import math
    v = _xyz64(vertices, 'vertices')
    if not (torch.is_tensor(faces) and faces.is_cuda):
        raise TypeError('faces must be a CUDA tensor (no CPU fallback exists)')
    cell = float(cell_size)
    if not (math.isfinite(cell) and cell > 0.0):
        raise ValueError('cluster_mesh: cell_size must be finite and > 0')
    lib = _lib.load()
    n, dev, stream = int(v.shape[0]), v.device, _stream(v)
    if n >= 2 ** 31:
        raise ValueError('too many vertices')
    stage = _Stages(profile)
    stage('faces_in')
    f = _checked_faces(faces, n, 'cluster_mesh')
    stage('cells')
    trace = torch.empty(n, dtype=torch.int64, device=dev)
    means = torch.empty(max(n, 1), 3, dtype=torch.float64, device=dev)
    state = torch.empty(5, dtype=torch.int64, device=dev)
    ws_bytes = lib.stin_voxel_cluster_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.stin_voxel_cluster_mean_f64(_ptr(v), n, cell, _ptr(trace), _ptr(means), _ptr(state), _ptr(ws), ws_bytes, stream),
               'stin_voxel_cluster_mean_f64')
    st = state.cpu()
    if int(st[3]) != 0:
        raise ValueError('cluster_mesh: non-finite coordinates or more than 2^21 cells along an axis')
    nc = int(st[4])
    stage('faces')
    nf = int(f.shape[0])
    if nf == 0:
        out = f
    elif _torch_faces:
        out = _cluster_faces_torch(f, trace)
    else:
        out = torch.empty(nf, 3, dtype=torch.int64, device=dev)
        ws_bytes = lib.stin_face_cluster_workspace_bytes(nf)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.stin_face_cluster_i64(_ptr(f), nf, _ptr(trace), n, nc, _ptr(out), _ptr(state), _ptr(ws), ws_bytes, stream),
                   'stin_face_cluster_i64')
        st = state.cpu()
        if int(st[3]) & 1:
            raise RuntimeError('cluster_mesh: a checked face or the trace is out of range')
        out = _cluster_faces_torch(f, trace) if int(st[3]) & 2 else out[:int(st[4])]
    stage(None)
    return means[:nc], out, trace, nc


def _qem_percent(x):
    """The percentage of a decimator-mode level given as a digit string '1' .. '99', else None."""
    if isinstance(x, str) and x.isdigit() and 1 <= int(x) <= 99:
        return int(x)
    return None


_DECIMAL = re.compile(r'(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?')


def _cell_size(x):
    """The cell size of a decimator-mode clustering level - a python float, or a decimal string that is not all digits ('0.04': the
    reference's `not isdigit()` branch) - finite and > 0, else None."""
    import math
    if isinstance(x, str):
        if x.isdigit() or not _DECIMAL.fullmatch(x):
            return None
        x = float(x)
    if isinstance(x, float) and math.isfinite(x) and x > 0.0:
        return x
    return None


def graph_levels(mesh, levels, dilated_levels, dilation_dists, labels=None, reference_vc_normals=False):
    """The body of the reference's process_frame (preprocessing/graph_level_generation.py:298-539) on the GPU: from a mesh and, per
    level, either a voxel size or a decimator's output to the dict the reference passes to torch.save for graphs/<scene>.pt
    (scene_io.write_graph_levels writes it; crop_scene, circle_masks / write_circle_masks, load_scene and load_label_scene read it).

    mesh: dict of CUDA tensors - vertices [N, 3] float64, faces [F, 3] int, colors [N, 3], normals [N, 3] (optional:
    vertex_normals(vertices, faces) when absent).
    levels: one entry per --level_params item, all of one mode:
      * vertex-clustering mode (--vertex_clustering): every entry a voxel size (float / int).  Level l clusters level l - 1 (the
        first one the mesh itself) with `vertex_clustering`; runs fully on the GPU.
      * decimator mode (--qem): each entry is '100' (the plain current mesh with an identity trace: extract_plain_mesh), a digit
        string '1' .. '99' (decimate_qem of the current mesh to that percentage of its vertices, on the GPU: the trace is the
        decimator's own, the level's normals are vertex_normals of the result - `['100', '30', '30', '30']` from a mesh alone), a
        cell size - a decimal string that is not all digits ('0.04', the reference's `not isdigit()` branch) or a python float, finite
        and > 0 - (cluster_mesh of the current mesh: the trace is the clustering's own membership trace onto the previous level, the
        normals are vertex_normals of the result, the edges those of its faces - `['0.04', '30', '30', '30']` from a mesh alone), a dict
        (vertices [n, 3] float64, faces, csv = path or read_trace_csv tuple, normals) with a decimator's result for the current
        mesh (extract_qem_mesh: trace_from_csv against the previous level), or a dict without 'csv' - an externally clustered
        mesh (the trimesh_clustering branch) whose trace is nearest(ORIGINAL mesh vertices, its vertices), as the reference has
        it, whatever the previous level was.
    dilated_levels: one 0 / 1 per level - 1: dilated_edges(level edges, positions, normals, dilation_dists) is stored for it.
    labels: int [N] labels of the original mesh (train mode: already remapped, see remap_scannet_labels); None: the --test mode.
    -> {'vertices': [level 0: float32 [N_0, 10] pos, colour, normal, original index (train) or every column (test); others
        float32 [N_l, 3]], 'labels': int64 [N] (train), 'edges': int64 [E_l, 2], 'traces': int64, one per level (traces[0] from the
        original mesh), 'dilated_edges': None or the list of dilated_edges, 'dilation_dists': as given}, tensors on the device.

    Differences from the reference: each level's edges come sorted by (row 0, row 1) instead of in CPython
    set order; and in vertex-clustering mode the normals of a dilated level are those of each coarse vertex's nearest original
    vertex - the reference walks with rows 0 .. N_l - 1 of the INPUT mesh's normals there because it never updates its current
    mesh (reference_vc_normals=True reproduces that for file parity); and a cell-size level's trace is the membership trace of the
    clustering of the previous level, where the reference takes nearest(ORIGINAL mesh vertices, clustered vertices) whatever the
    previous level was (the dict-without-'csv' branch keeps the reference's rule).
    `mesh` is what scene_io.read_ply returns for a PLY file (scene_io.write_scene_from_ply chains the two); out of scope: the Matterport
    category tables (scene_io.vertex_labels_from_faces is its vote) and the S3DIS label path.  A dict level still takes the output of an external
    decimator (vcglib's tridecimator or trimesh_clustering in the reference) as it is."""
    if len(levels) != len(dilated_levels):
        raise ValueError('levels and dilated_levels need one entry per level')
    if len(levels) == 0:
        raise ValueError('at least one level is needed')
    verts = mesh['vertices']
    if not (torch.is_tensor(verts) and verts.is_cuda):
        raise TypeError('graph_levels runs on the GPU only (no CPU fallback exists)')
    dev = verts.device
    v64 = verts.double().contiguous()
    n = int(v64.shape[0])
    dists = [int(d) for d in dilation_dists] if dilation_dists is not None else []
    faces0 = mesh['faces'].to(dev)
    normals0 = mesh['normals'].to(dev).double() if mesh.get('normals') is not None else vertex_normals(v64, faces0)
    cols = [v64, mesh['colors'].to(dev).double(), normals0, torch.arange(n, device=dev, dtype=torch.float64).unsqueeze(1)]
    if labels is not None:
        cols.append(torch.as_tensor(labels).to(dev).double().reshape(n, 1))
    original = torch.cat(cols, dim=1)
    vc_mode = all(isinstance(x, (int, float)) and not isinstance(x, bool) for x in levels)
    if not vc_mode and any(not (isinstance(x, dict) or str(x) == '100' or _qem_percent(x) is not None or _cell_size(x) is not None)
                           for x in levels):
        raise ValueError("levels: all voxel sizes (vertex-clustering mode), or each '100', a percentage '1' .. '99', a cell size "
                         "('0.04' or a float, finite and > 0) or a dict (decimator mode)")
    coords = [v64]
    edges, traces, level_normals = [], [], []
    cur = dict(vertices=v64, faces=faces0, normals=normals0)                          # the reference's curr_mesh
    cur_edges = _mesh_edges(cur['faces'], n)
    for l, spec in enumerate(levels):
        if vc_mode:
            prev = coords[-1]
            ei = cur_edges.t().contiguous()
            if prev.dtype == torch.float64:
                c_l, tr, e_l = vertex_clustering(prev, ei, float(spec))
            else:
                c_l, tr, e_l = _cluster_level_f32(prev, ei, float(spec))
            cur_edges = e_l
            nrm = None                                                            # filled in after the colour lookup
        elif isinstance(spec, dict) and 'csv' not in spec:
            c_l = spec['vertices'].to(dev).double().contiguous()
            e_l = _mesh_edges(spec['faces'].to(dev), c_l.shape[0])
            tr = nearest(coords[0], c_l)
            cur = dict(vertices=c_l, faces=spec['faces'].to(dev), normals=spec['normals'].to(dev).double())
            nrm = cur['normals']
        elif isinstance(spec, dict):
            c_l = spec['vertices'].to(dev).double().contiguous()
            e_l = _mesh_edges(spec['faces'].to(dev), c_l.shape[0])
            tr = trace_from_csv(spec['csv'], coords[-1], c_l)
            cur = dict(vertices=c_l, faces=spec['faces'].to(dev), normals=spec['normals'].to(dev).double())
            nrm = cur['normals']
        elif _qem_percent(spec) is not None:                                      # the decimator itself: the trace comes with it
            c_l, f_l, tr, _ = decimate_qem(cur['vertices'], cur['faces'], percent=_qem_percent(spec))
            e_l = _mesh_edges(f_l, c_l.shape[0])
            cur = dict(vertices=c_l, faces=f_l, normals=vertex_normals(c_l, f_l))
            nrm = cur['normals']
        elif _cell_size(spec) is not None:                                        # mesh clustering: its own membership trace
            c_l, f_l, tr, _ = cluster_mesh(cur['vertices'], cur['faces'], _cell_size(spec))
            e_l = _mesh_edges(f_l, c_l.shape[0])
            cur = dict(vertices=c_l, faces=f_l, normals=vertex_normals(c_l, f_l))
            nrm = cur['normals']
        else:
            c_l = cur['vertices']
            e_l = _mesh_edges(cur['faces'], c_l.shape[0])
            tr = torch.arange(c_l.shape[0], dtype=torch.int64, device=dev)
            nrm = cur['normals']
        coords.append(c_l)
        edges.append(e_l)
        traces.append(tr.long())
        level_normals.append(nrm)
    looked = _colors_and_labels(original, coords)
    dilated = []
    for l in range(len(levels)):
        if int(dilated_levels[l]) != 1:
            dilated.append(None)
            continue
        c_l = coords[l + 1]
        nrm = level_normals[l]
        if nrm is None:
            nrm = normals0[:c_l.shape[0]] if reference_vc_normals else normals0[looked[l + 1][1]]
        dilated.append(dilated_edges(edges[l].t().contiguous(), c_l.double().contiguous(), nrm.double().contiguous(), dists))
    ccl = [torch.cat([coords[i].double(), looked[i][0]], dim=1) for i in range(len(coords))]
    out = {}
    if labels is not None:
        out['vertices'] = [ccl[1][:, :-1].float()] + [ccl[i][:, :3].float() for i in range(2, len(ccl))]
        out['labels'] = ccl[0][:, -1].long()
    else:
        out['vertices'] = [ccl[1].float()] + [ccl[i][:, :3].float() for i in range(2, len(ccl))]
    out['edges'] = [e.long() for e in edges]
    out['traces'] = traces
    out['dilated_edges'] = dilated
    out['dilation_dists'] = dilation_dists
    return out


# ------------------------------------------------------------------------------------------------------------- observer masks
def pose_extrinsics(poses):
    """Camera-to-world poses [P, 4, 4] (the content of ScanNet's *.pose.txt; array or tensor) -> (RT float64 [P, 12], valid uint8 [P])
    numpy arrays on the host: RT[p] = the rows of E[:3, :4], E = np.linalg.inv(pose) - the reference's read_camera_pose (:58-63)
    without its transpose for PyTorch3D's row-vector convention.  A pose with a non-finite entry (ScanNet writes -inf where tracking
    was lost; the reference would crash on it) is invalid: valid[p] = 0, RT[p] = 0, it observes nothing."""
    import numpy as np
    p = poses.detach().cpu().numpy() if torch.is_tensor(poses) else np.asarray(poses)
    p = np.asarray(p, dtype=np.float64).reshape(-1, 4, 4)
    valid = np.isfinite(p).reshape(p.shape[0], 16).all(axis=1)
    RT = np.zeros((p.shape[0], 12), dtype=np.float64)
    for i in np.flatnonzero(valid):
        RT[i] = np.linalg.inv(p[i])[:3, :4].reshape(12)
    return RT, valid.astype(np.uint8)


def observe_vertices(vertices, faces, poses, fx, fy, width, height, image_size=256, z_near=0.01, batch=64, large_box=None,
                     return_status=False):
    """Which camera poses see which vertices: the reference's compute_observed_vertex_map (:159-251) as a depth-tested triangle
    rasteriser on the GPU (csrc/stin_observe.hip).  vertices [N, >= 3] float, faces [F, 3] int (CUDA); poses [P, 4, 4] camera-to-world
    (array or tensor, any device: they are inverted on the host); fx, fy = entries [0, 0] and [1, 1] of the colour intrinsic; width,
    height of the colour image.
    -> (bits uint32 [N, ceil(P / 32)] on the device: bit (p & 31) of word (p >> 5) = pose p observes the vertex, i.e. it is a corner of
        the face seen at one pixel centre at least; valid_pose_ids int64 numpy: the poses without a non-finite entry).
    return_status=True: also the status word (int): bit STIN_OBSERVE_BAD_INDEX - a face had an index outside [0, N) and was skipped;
    bit STIN_OBSERVE_LARGE_FACE - a face went through the large-face rasteriser (informational).

    The contract (include/stin_hip.h, "Observer masks"; restated per pixel in numpy by the test suite, which this reproduces bit
    for bit), fp64 throughout: view = E [x y z 1], E the inverse pose; screen X = (sx xv / zv + 1) (S / 2) - 1 / 2 with sx = 2 fx /
    width (Y likewise), pixel (row i, column j) centred at (X, Y) = (j, i) - a pinhole with the principal point at the image centre and
    the full field of view stretched onto the S x S image, which is what the reference's compute_projection_matrix composed with
    PyTorch3D's NDC convention amounts to.  This was derived from reading that code and PyTorch3D's documented conventions; it is NOT
    pinned against a PyTorch3D run.  A face with a corner nearer than z_near is DROPPED, not clipped; so is one with no area on
    screen.  Coverage is inclusive on every edge and takes both orientations; the nearest face wins a pixel after its depth is rounded
    to fp32, the lowest face id on a tie.  The result does not depend on `batch` (poses per pass: batch * S * S * 8 bytes of depth
    keys and batch * N * 24 bytes of screen coordinates) nor on `large_box` (faces whose clamped box holds more centres go to a
    wavefront each; default STIN_OBSERVE_LARGE_BOX)."""
    import numpy as np
    if not (torch.is_tensor(faces) and faces.is_cuda):
        raise TypeError('faces must be a CUDA tensor (no CPU fallback exists)')
    v = _xyz64(vertices, 'vertices')
    lib = _lib.load()
    S, B = int(image_size), int(batch)
    if not 1 <= S <= _lib.CONSTANTS['STIN_OBSERVE_MAX_SIZE'] or not 1 <= B <= _lib.CONSTANTS['STIN_OBSERVE_MAX_BATCH']:
        raise ValueError('image_size must be in [1, %d] and batch in [1, %d]' % (_lib.CONSTANTS['STIN_OBSERVE_MAX_SIZE'],
                                                                                _lib.CONSTANTS['STIN_OBSERVE_MAX_BATCH']))
    if not float(z_near) > 0.0:
        raise ValueError('z_near must be positive')
    RT, valid = pose_extrinsics(poses)
    n, dev, P = int(v.shape[0]), v.device, int(RT.shape[0])
    f = faces.long().reshape(-1, 3).contiguous()
    F, words = int(f.shape[0]), (P + 31) // 32
    B = max(1, min(B, P))
    bits = torch.empty(n, words, dtype=torch.uint32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    rt_d, valid_d = torch.from_numpy(RT).to(dev), torch.from_numpy(valid).to(dev)
    ws_bytes = lib.stin_observe_workspace_bytes(n, F, S, B)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    sx, sy = 2.0 * float(fx) / float(width), 2.0 * float(fy) / float(height)
    _lib.check(lib.stin_observe_poses_f64(_ptr(v), n, _ptr(f) if F else None, F, _ptr(rt_d) if P else None, _ptr(valid_d) if P else None,
                                          P, sx, sy, S, float(z_near), B, int(large_box) if large_box is not None else 0,
                                          _ptr(bits) if bits.numel() else None, words, _ptr(status), _ptr(ws), ws_bytes, _stream(v)),
               'stin_observe_poses_f64')
    ids = np.flatnonzero(valid).astype(np.int64)
    return (bits, ids, int(status.item())) if return_status else (bits, ids)


def observer_visible(valid_pose_ids, num_poses, keep_probability=0.5, num_masks=1, seed=0):
    """The pose subsets of num_masks masks -> bool [num_masks, num_poses] numpy: row m keeps the valid poses where
    np.random.RandomState(seed + m).rand(len(valid_pose_ids)) <= keep_probability - the reference's select_pose_random_subset
    (:254-256), with a stated seed instead of the global generator."""
    import numpy as np
    ids = np.asarray(valid_pose_ids, dtype=np.int64).reshape(-1)
    if ids.size and (ids.min() < 0 or ids.max() >= int(num_poses)):
        raise IndexError('a valid pose id lies outside [0, %d)' % int(num_poses))
    out = np.zeros((int(num_masks), int(num_poses)), dtype=bool)
    for m in range(int(num_masks)):
        out[m, ids] = np.random.RandomState(int(seed) + m).rand(ids.size) <= keep_probability
    return out


def _pack_pose_bits(visible, words):
    """bool [M, P] -> uint32 [M, words] with bit (p & 31) of word (p >> 5) (numpy, little-endian words)."""
    import numpy as np
    vis = np.asarray(visible, dtype=bool)
    padded = np.zeros((vis.shape[0], words * 32), dtype=np.uint8)
    padded[:, :vis.shape[1]] = vis
    w = padded.reshape(vis.shape[0], words, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)
    return w.sum(axis=2).astype(np.uint32)


def _observer_counts(bits, visible_words, min_num_poses, invert, want_mask, want_count):
    lib = _lib.load()
    if not (torch.is_tensor(bits) and bits.is_cuda):
        raise TypeError('bits must be a CUDA tensor (no CPU fallback exists)')
    if bits.dtype != torch.uint32 or bits.dim() != 2:
        raise TypeError('bits must be uint32 [N, words], as observe_vertices returns it')
    b = bits.contiguous()
    n, words, M = int(b.shape[0]), int(b.shape[1]), int(visible_words.shape[0])
    vw = torch.from_numpy(visible_words).to(b.device)
    mask = torch.empty(M, n, dtype=torch.int64, device=b.device) if want_mask else None
    count = torch.empty(M, n, dtype=torch.int32, device=b.device) if want_count else None
    _lib.check(lib.stin_observe_mask_u32(_ptr(b) if b.numel() else None, n, words, _ptr(vw) if vw.numel() else None, M, int(min_num_poses),
                                         int(bool(invert)), _ptr(mask), _ptr(count), _stream(b)), 'stin_observe_mask_u32')
    return mask, count


def observer_masks(bits, valid_pose_ids, num_poses, keep_probability=0.5, min_num_poses=40, num_masks=1, seed=0, visible=None,
                   invert=False, return_counts=False):
    """Observer masks of one scene: int64 [num_masks, N] on the device, the reference's generate_mask_from_vertex_observing_poses
    (:259-267) for every mask at once (stin_observe_mask_u32).  bits: observe_vertices' result.  Mask m takes the pose subset
    visible[m] (bool [M, num_poses]; default observer_visible(valid_pose_ids, num_poses, keep_probability, num_masks, seed)), counts
    per vertex the poses of the subset that observe it, and writes
        invert=False (default, the reference's values): 1 where at least min_num_poses poses of the subset see the vertex, else 0;
        invert=True:                                    1 where FEWER than min_num_poses see it, else 0.
    The reference's loader inpaints where mask > 0 (scene_io.load_scene): with the default the network is asked to repaint what the
    subset observed and is shown what it did not; invert=True asks it to fill in what the partial capture missed.  The default keeps
    the reference's values as they are.  return_counts=True: also the counts (int32 [M, N]).
    scene_io.write_circle_masks writes either kind to the mask files."""
    import numpy as np
    if visible is None:
        visible = observer_visible(valid_pose_ids, num_poses, keep_probability, num_masks, seed)
    vis = visible.detach().cpu().numpy() if torch.is_tensor(visible) else np.asarray(visible)
    vis = np.atleast_2d(vis.astype(bool))
    if vis.ndim != 2 or vis.shape[1] != int(num_poses):
        raise ValueError('visible must be [num_masks, %d]' % int(num_poses))
    words = (int(num_poses) + 31) // 32
    if torch.is_tensor(bits) and bits.dim() == 2 and int(bits.shape[1]) != words:
        raise ValueError('bits has %d words per vertex, %d poses need %d' % (int(bits.shape[1]), int(num_poses), words))
    mask, count = _observer_counts(bits, _pack_pose_bits(vis, words), min_num_poses, invert, True, return_counts)
    return (mask, count) if return_counts else mask


def observer_counts(bits, num_poses=None):
    """The two statistics the reference plots (plot_statistics :454-483) -> (per_vertex int64 [N]: poses that observe each vertex;
    per_pose int64 [P]: vertices each pose observes; P = num_poses, default 32 * words), on the device.  per_vertex is
    stin_observe_mask_u32's count with every pose visible; per_pose sums each bit position over the vertices (32 integer
    reductions in torch: a statistic beside the path, not on it)."""
    import numpy as np
    words = int(bits.shape[1]) if torch.is_tensor(bits) and bits.dim() == 2 else 0
    _, count = _observer_counts(bits, np.full((1, words), 0xFFFFFFFF, dtype=np.uint32), 0, False, False, True)
    P = 32 * words if num_poses is None else int(num_poses)
    b = bits.contiguous().view(torch.int32)
    per_bit = torch.stack([((b >> k) & 1).sum(dim=0) for k in range(32)], dim=1)        # [words, 32]
    return count[0].long(), per_bit.reshape(-1)[:P].contiguous()


def observers_to_lists(bits, num_poses=None):
    """bits (uint32 [N, words]; tensor on any device or array) -> the reference's observed_poses_per_vert: a list with, per vertex, the
    ascending list of the pose ids that observe it (the content of its observers_per_vert/<scene>.npz cache), on the host."""
    import numpy as np
    b = bits.detach().cpu().numpy() if torch.is_tensor(bits) else np.asarray(bits)
    b = np.ascontiguousarray(b, dtype=np.uint32)
    n, words = b.shape
    flags = ((b[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(n, words * 32)
    if num_poses is not None:
        flags = flags[:, :int(num_poses)]
    return [np.flatnonzero(row).tolist() for row in flags]


# ------------------------------------------------------------------------------------------------------------- frame colours
def frame_intrinsics(colorintrinsic, orig_width, orig_height, width, height):
    """The reference's camera for colour frames resized from orig_width x orig_height to width x height
    (texture_map_optimization.py:104-107) -> (fx, fy, cx, cy) floats: fx * width / orig_width, fy * height / orig_height,
    width / 2 - 0.5, height / 2 - 0.5; fx, fy = entries [0, 0] and [1, 1] of colorintrinsic (scene_io.load_scan_config's
    'colorintrinsic', with its 'colorwidth' / 'colorheight' as the original size).  The principal point of the file is NOT used: the
    reference puts it at the image centre."""
    import numpy as np
    ic = colorintrinsic.detach().cpu().numpy() if torch.is_tensor(colorintrinsic) else np.asarray(colorintrinsic)
    ic = np.asarray(ic, dtype=np.float64)
    return (float(ic[0, 0]) * width / orig_width, float(ic[1, 1]) * height / orig_height, width / 2.0 - 0.5, height / 2.0 - 0.5)


def _camera4(cam, what):
    c = tuple(float(v) for v in cam)
    if len(c) != 4:
        raise ValueError('%s must be (fx, fy, cx, cy)' % what)
    return c


def _frames_u(t, dtype, tail, what):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise TypeError('%s must be a CUDA tensor (no CPU fallback exists)' % what)
    if t.dtype != dtype:
        raise TypeError('%s must be %s' % (what, dtype))
    if t.dim() != 3 + len(tail) or tuple(t.shape[3:]) != tail:
        raise ValueError('%s must be [B, H, W%s]' % (what, ''.join(', %d' % d for d in tail)))
    return t.contiguous()


def _camera_doubles(camera, constant='STIN_COLORMAP_CAMERA_DOUBLES'):
    """(fx, fy, cx, cy), or the colour camera followed by the depth camera, as the C ABI takes it."""
    return (ctypes.c_double * _lib.CONSTANTS[constant])(*camera)


def _depth_frames(depth, P):
    """depth as FrameColors.add takes it, one frame per pose -> contiguous."""
    d = _frames_u(depth, torch.uint16, (), 'depth')
    if int(d.shape[0]) != P:
        raise ValueError('%d poses but %d depth frames' % (P, int(d.shape[0])))
    return d


def _pose_bits(bits, n, poses, counted):
    """bits as observe_vertices returns it for n vertices, with a bit for every pose below `poses` (`counted`: how the message
    words that number) -> contiguous."""
    if not (torch.is_tensor(bits) and bits.is_cuda):
        raise TypeError('bits must be a CUDA tensor (no CPU fallback exists)')
    if bits.dtype != torch.uint32 or bits.dim() != 2 or int(bits.shape[0]) != n:
        raise TypeError('bits must be uint32 [N, words], as observe_vertices returns it')
    words, need = int(bits.shape[1]), (poses + 31) // 32
    if words < need:
        raise ValueError('bits has %d words per vertex, %s need %d' % (words, counted % poses, need))
    return bits.contiguous()


class FrameColors:
    """Per-vertex colours of a mesh from a scan's colour and depth frames and its camera trajectory, on the GPU
    (csrc/stin_frames.hip) - the step the reference's preprocessing/texture_map_optimization.py hands to Open3D's colour-map
    pipeline with maximum_iteration = 0: nothing is optimised; per vertex and frame a visibility test, a projection, a bilinear
    sample of the colour image, and the average over the frames that see the vertex.  The result is what becomes
    vertices[0][:, 3:6] of graphs/<scene>.pt (pass it to graph_levels as mesh['colors']); the count is the honest mask of what the
    scan never observed.

    vertices [N, >= 3] float CUDA tensor; color_camera, depth_camera = (fx, fy, cx, cy) in pixels of the colour / depth frames
    (frame_intrinsics; depth_camera None: the colour camera, for colour frames resized to the depth size as the reference does).
    The object owns sum int64 [N, 3], count int32 [N] and, when num_poses is given, seen uint32 [N, ceil(num_poses / 32)] (bit
    (p & 31) of word (p >> 5): pose p coloured the vertex) on the vertices' device.

    The contract (include/stin_hip.h, "Frame colours"; restated in numpy by the test suite, which this reproduces bit for bit), fp64:
    view = E [x y z 1], E the inverse pose; u = fx xv / zv + cx, v = fy yv / zv + cy, pixel (row i, column j) centred at (j, i); a pair
    with zv < z_near or a non-finite u, v is skipped.  Depth: raw uint16, 0 = no measurement, also where raw / depth_scale >
    depth_trunc.  A vertex is visible in a frame when the depth pixel nearest to its projection (rint, ties to even) lies in the
    image, holds a measurement d = raw / depth_scale <= max_depth with |zv - d| < depth_threshold, and is not within half_kernel
    pixels of a depth discontinuity: a pixel whose 3 x 3 Sobel response on the raw depth exceeds discontinuity_threshold *
    depth_scale (the threshold is in metres of SOBEL response: a step of s metres gives 4 s to 8 s).  Or, without depth frames, when
    observe_vertices' bit says so.  The sample: bilinear in the uint8 colour frame, required to lie `margin` pixels inside it,
    rounded to 1 / 65536 of a grey level and summed as integers - the result does not depend on the order or the batching.

    Not Open3D's result bit for bit and not pinned against a run of it.  Frames arrive here decoded and at their final size: resize_u8
    brings colour frames to the depth size on the device, scene_io.read_frames reads a scan's files, and scan_vertex_colors does
    both from a scan directory.  Open3D's optimisers are optimize_poses_rigid (iterations > 0) and optimize_poses_nonrigid (warp
    lattices per frame): run one first and average with what it returns.  Out of scope: clipping at the near plane, and a CPU fallback.  Unseen vertices get `fill` and count 0, or, with result(knn=k), the mean colour of their k nearest coloured
    vertices (fill_unseen_colors: exact fp64 k-NN with a stated tie rule; k = 3 is Open3D's default to our knowledge, which - like
    its tie handling - could not be checked against a run of it)."""

    def __init__(self, vertices, color_camera, depth_camera=None, *, depth_scale=1000.0, depth_trunc=3.0, max_depth=2.5,
                 depth_threshold=0.03, discontinuity_threshold=0.1, half_kernel=3, margin=10, z_near=0.01, num_poses=None):
        self.vertices = _xyz64(vertices, 'vertices')
        self.color_camera = _camera4(color_camera, 'color_camera')
        self.depth_camera = self.color_camera if depth_camera is None else _camera4(depth_camera, 'depth_camera')
        self.depth_scale, self.depth_trunc, self.max_depth = float(depth_scale), float(depth_trunc), float(max_depth)
        self.depth_threshold, self.discontinuity_threshold = float(depth_threshold), float(discontinuity_threshold)
        self.half_kernel, self.margin, self.z_near = int(half_kernel), int(margin), float(z_near)
        if not self.z_near > 0.0:
            raise ValueError('z_near must be positive')
        if not self.depth_scale > 0.0:
            raise ValueError('depth_scale must be positive')
        if self.margin < 0 or not 0 <= self.half_kernel <= _lib.CONSTANTS['STIN_FRAMES_MAX_HALF_KERNEL']:
            raise ValueError('margin must be >= 0 and half_kernel in [0, %d]' % _lib.CONSTANTS['STIN_FRAMES_MAX_HALF_KERNEL'])
        n, dev = int(self.vertices.shape[0]), self.vertices.device
        self.num_poses = None if num_poses is None else int(num_poses)
        self.sum = torch.zeros(n, 3, dtype=torch.int64, device=dev)
        self.count = torch.zeros(n, dtype=torch.int32, device=dev)
        self.seen = None if num_poses is None else torch.zeros(n, (self.num_poses + 31) // 32, dtype=torch.int32,
                                                               device=dev).view(torch.uint32)

    def depth_edges(self, depth):
        """depth uint16 [B, Hd, Wd] (CUDA) -> the depth-discontinuity mask uint8 [B, Hd, Wd] of the contract."""
        d = _frames_u(depth, torch.uint16, (), 'depth')
        lib = _lib.load()
        B, H, W = (int(s) for s in d.shape)
        edge = torch.empty(B, H, W, dtype=torch.uint8, device=d.device)
        if B == 0 or H == 0 or W == 0:
            return edge
        ws_bytes = lib.stin_frames_edges_workspace_bytes(B, H, W)
        if ws_bytes == 0:
            raise ValueError('depth frames of %d x %d x %d are outside what the edge kernel supports' % (B, H, W))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=d.device)
        _lib.check(lib.stin_frames_depth_edges_u16(_ptr(d), B, H, W, self.depth_scale, self.depth_trunc, self.discontinuity_threshold,
                                                   self.half_kernel, _ptr(edge), _ptr(ws), ws_bytes, _stream(d)),
                   'stin_frames_depth_edges_u16')
        return edge

    def add(self, poses, color, depth=None, bits=None, first_pose=0, _route=None, flow=None, lattice_step=None):
        """One batch: poses [B, 4, 4] camera-to-world (array or tensor; inverted on the host), color uint8 [B, Hc, Wc, 3] RGB and
        either depth uint16 [B, Hd, Wd] or bits (observe_vertices' uint32 [N, words], indexed by first_pose + b) - CUDA tensors.
        first_pose: the scan-wide id of the batch's first pose (for bits and seen).  Batches arrive in any order and any size.
        _route (tests): STIN_FRAMES_ROUTE_OWNER / _SPLIT instead of the host's choice from N and B.
        flow, lattice_step: the warp lattices of optimize_poses_nonrigid for these poses, float64 [B, Ah, Aw, 2] (array or tensor),
        and their step - the colour frame is then sampled at the warped position (stin_nonrigid_accumulate_f64).  Bits mode only:
        the depth test knows no warp."""
        if (depth is None) == (bits is None):
            raise ValueError('exactly one of depth and bits must be given')
        if flow is not None and depth is not None:
            raise ValueError('flow needs bits mode: the depth test knows no warp (vertex_colors_from_frames makes the two passes)')
        c = _frames_u(color, torch.uint8, (3,), 'color')
        RT, valid = pose_extrinsics(poses)
        B, n, dev, first = int(RT.shape[0]), int(self.vertices.shape[0]), self.vertices.device, int(first_pose)
        if int(c.shape[0]) != B:
            raise ValueError('%d poses but %d colour frames' % (B, int(c.shape[0])))
        if first < 0 or (self.num_poses is not None and first + B > self.num_poses):
            raise ValueError('poses %d .. %d lie outside [0, num_poses)' % (first, first + B))
        if B > _lib.CONSTANTS['STIN_FRAMES_MAX_BATCH']:
            raise ValueError('at most %d poses per batch' % _lib.CONSTANTS['STIN_FRAMES_MAX_BATCH'])
        _lib.load()
        d = edge = b = None
        if depth is not None:
            d = _depth_frames(depth, B)
        else:
            b = _pose_bits(bits, n, first + B, 'poses up to %d')
        if flow is not None:
            flow, lattice_step = _nonrigid_flow(flow, lattice_step, B, int(c.shape[1]), int(c.shape[2]))
        if B == 0 or n == 0:
            return self
        if 0 in c.shape or (d is not None and 0 in d.shape):
            raise ValueError('empty frames')
        if d is not None:
            edge = self.depth_edges(d)
        rt_d, valid_d = torch.from_numpy(RT).to(dev), torch.from_numpy(valid).to(dev)
        if flow is not None:
            flow = flow.to(dev)
        return self._add_extrinsics(rt_d, valid_d, c, first, depth=d, edge=edge, bits=b, seen=self.seen, route=_route, flow=flow,
                                    lattice_step=lattice_step)

    def _add_extrinsics(self, rt_d, valid_d, color, first_pose, depth=None, edge=None, bits=None, seen=None, route=None, flow=None,
                        lattice_step=None):
        """The launch under add(), for extrinsics that are already on the device (rt_d fp64 [B, 12], valid_d uint8 [B],
        pose_extrinsics' rows) and arguments as add() has checked them; optimize_poses_rigid repeats it in bits mode at the poses of
        every iteration; flow (fp64 [B, Ah, Aw, 2] on the device, bits mode): optimize_poses_nonrigid's warped pass."""
        n, B = int(self.vertices.shape[0]), int(rt_d.shape[0])
        if B == 0 or n == 0:
            return self
        route = _lib.CONSTANTS['STIN_FRAMES_ROUTE_AUTO'] if route is None else int(route)
        if flow is not None:
            cam = _camera_doubles(self.color_camera)
            _lib.check(_lib.load().stin_nonrigid_accumulate_f64(_ptr(self.vertices), n, _ptr(rt_d), _ptr(valid_d), B, int(first_pose),
                                                                _ptr(color), int(color.shape[1]), int(color.shape[2]), _ptr(flow),
                                                                int(lattice_step), cam, self.z_near, _ptr(bits), int(bits.shape[1]),
                                                                self.margin, route, _ptr(self.sum), _ptr(self.count), _ptr(seen),
                                                                0 if seen is None else int(seen.shape[1]), _stream(self.vertices)),
                       'stin_nonrigid_accumulate_f64')
            return self
        cameras = _camera_doubles(self.color_camera + self.depth_camera, 'STIN_FRAMES_CAMERA_DOUBLES')
        params = (ctypes.c_double * _lib.CONSTANTS['STIN_FRAMES_PARAM_DOUBLES'])(self.depth_scale, self.depth_trunc, self.max_depth,
                                                                                 self.depth_threshold, self.z_near)
        Hd, Wd = (int(depth.shape[1]), int(depth.shape[2])) if depth is not None else (0, 0)
        _lib.check(_lib.load().stin_frames_accumulate_f64(_ptr(self.vertices), n, _ptr(rt_d), _ptr(valid_d), B, int(first_pose),
                                                          _ptr(color), int(color.shape[1]), int(color.shape[2]), _ptr(depth), _ptr(edge),
                                                          Hd, Wd, cameras, params, _ptr(bits), 0 if bits is None else int(bits.shape[1]),
                                                          self.margin, route,
                                                          _ptr(self.sum), _ptr(self.count), _ptr(seen),
                                                          0 if seen is None else int(seen.shape[1]), _stream(self.vertices)),
                   'stin_frames_accumulate_f64')
        return self

    def result(self, fill=(0, 0, 0), knn=0):
        """-> (colors float32 [N, 3] in [0, 1], count int32 [N]): the mean of the samples; `fill` where count is 0.  knn = k > 0:
        a vertex with count 0 gets the mean colour of its k nearest coloured vertices instead (fill_unseen_colors; `fill` remains
        only when no vertex was coloured at all); count is returned as it is - the honest mask of what was never observed."""
        lib = _lib.load()
        n = int(self.vertices.shape[0])
        f = tuple(float(v) for v in fill)
        if len(f) != 3:
            raise ValueError('fill must have three entries')
        if int(knn) != 0:
            _check_k(knn, 'FrameColors.result')
        colors = torch.empty(n, 3, dtype=torch.float32, device=self.vertices.device)
        _lib.check(lib.stin_frames_finish_f32(_ptr(self.sum), _ptr(self.count), n, f[0], f[1], f[2], _ptr(colors), None,
                                              _stream(self.vertices)), 'stin_frames_finish_f32')
        if int(knn) != 0 and n:
            colors = fill_unseen_colors(self.vertices, colors, self.count, k=int(knn))
        return colors, self.count


def vertex_colors_from_frames(vertices, poses, color, depth=None, bits=None, batch=64, color_camera=None, depth_camera=None,
                              fill=(0, 0, 0), return_seen=False, _route=None, knn=0, flow=None, lattice_step=None, **params):
    """FrameColors for frames that are all resident: poses [P, 4, 4], color uint8 [P, Hc, Wc, 3], depth uint16 [P, Hd, Wd] or bits
    (observe_vertices), added in batches of `batch` poses (the result does not depend on it) -> (colors float32 [N, 3], count int32
    [N]), with return_seen=True also seen uint32 [N, ceil(P / 32)].  color_camera is required; knn = k > 0 fills the vertices no
    frame coloured from their k nearest coloured ones (FrameColors.result); the other keywords are FrameColors'.
    Frames of another size go through resize_u8 first; scan_vertex_colors reads, resizes and adds a scan directory batch by batch.
    flow float64 [P, Ah, Aw, 2] and lattice_step: the warp lattices that optimize_poses_nonrigid returns with its poses - the colour
    frames are sampled at the warped positions.  In bits mode that is one warped pass; in depth mode one UNWARPED pass establishes
    which frames see which vertex (the depth test knows no warp, as in the optimiser) and a second, warped pass in bits mode fills
    fresh sums under that visibility.  Without flow every path is what it was, to the byte.
    Out of scope, as there: near-plane clipping, a CPU fallback (the optimisers are optimize_poses_rigid and
    optimize_poses_nonrigid, whose poses go in here)."""
    if color_camera is None:
        raise ValueError('color_camera = (fx, fy, cx, cy) is required')
    _frames_u(color, torch.uint8, (3,), 'color')
    P, step = int(color.shape[0]), int(batch)
    if step < 1:
        raise ValueError('batch must be positive')
    if len(poses) != P:
        raise ValueError('%d poses but %d colour frames' % (len(poses), P))
    two_passes = flow is not None and depth is not None
    fc = FrameColors(vertices, color_camera, depth_camera, num_poses=P if return_seen or two_passes else None, **params)
    if (depth is None) == (bits is None):
        raise ValueError('exactly one of depth and bits must be given')
    if flow is not None:
        flow, lattice_step = _nonrigid_flow(flow, lattice_step, P, int(color.shape[1]), int(color.shape[2]))

    def add_all(fc, depth, bits, flow):
        for p0 in range(0, P, step):
            p1 = min(p0 + step, P)
            fc.add(poses[p0:p1], color[p0:p1], None if depth is None else depth[p0:p1], bits, first_pose=p0, _route=_route,
                   flow=None if flow is None else flow[p0:p1], lattice_step=lattice_step)
        return fc

    add_all(fc, depth, bits, None if two_passes else flow)
    if two_passes:                                                     # the visibility of the unwarped pass, the colours of a warped one
        fc = add_all(FrameColors(vertices, color_camera, depth_camera, num_poses=P if return_seen else None, **params), None, fc.seen, flow)
    colors, count = fc.result(fill, knn=knn)
    return (colors, count, fc.seen) if return_seen else (colors, count)


# -------------------------------------------------------------------------------------------------------------- image resize
RESIZE_MODES = {'linear': 'STIN_RESIZE_LINEAR', 'area': 'STIN_RESIZE_AREA'}


def _resize_job(job, pool_bytes, out_bytes, channels, mode):
    """One (src_off, H, W, dst_off, h, w) row, checked the way the kernel checks it (which then writes nothing): raised here."""
    if len(job) != _lib.CONSTANTS['STIN_RESIZE_JOB_WORDS']:
        raise ValueError('a resize job is (src_off, H, W, dst_off, h, w)')
    so, H, W, do, h, w = (int(v) for v in job)
    top = _lib.CONSTANTS['STIN_RESIZE_MAX_SIDE']
    if min(H, W, h, w) < 1:
        raise ValueError('resize %d x %d -> %d x %d: every side must be at least 1' % (H, W, h, w))
    if max(H, W, h, w) > top:
        raise ValueError('resize %d x %d -> %d x %d: a side above %d' % (H, W, h, w, top))
    if mode == 'area' and (h > H or w > W):
        raise ValueError('resize %d x %d -> %d x %d: the area mode does not enlarge (use mode="linear")' % (H, W, h, w))
    if so < 0 or so + H * W * channels > pool_bytes:
        raise ValueError('image at offset %d (%d x %d x %d bytes) lies outside the pool of %d bytes' % (so, H, W, channels, pool_bytes))
    if do < 0 or do + h * w * channels > out_bytes:
        raise ValueError('result at offset %d (%d x %d x %d bytes) lies outside the %d output bytes' % (do, h, w, channels, out_bytes))
    return so, H, W, do, h, w


def _linear_axis_np(n_in, n_out):
    import numpy as np
    d = np.arange(n_out, dtype=np.int64)
    num, den = (2 * d + 1) * n_in - n_out, 2 * n_out
    s = num // den
    b = (4096 * (num - s * den) + den) // (2 * den)
    edge = (s < 0) | (s >= n_in - 1)
    s = np.clip(s, 0, n_in - 1)
    b = np.where(edge, 0, b).astype(np.int32)
    return s, np.minimum(s + 1, n_in - 1), b


def _area_axis_np(v, n_out):
    """v float64 [n_in, M] (integers) -> [n_out, M]: the overlap-weighted sums along axis 0, exact while they stay below 2^53; the
    overlap matrix is formed for 256 outputs at a time, over the inputs they touch."""
    import numpy as np
    n_in = v.shape[0]
    out = np.empty((n_out, v.shape[1]), dtype=np.float64)
    for j0 in range(0, n_out, 256):
        j1 = min(j0 + 256, n_out)
        x0, x1 = j0 * n_in // n_out, -(-(j1 * n_in) // n_out)
        j, x = np.arange(j0, j1, dtype=np.int64)[:, None], np.arange(x0, x1, dtype=np.int64)[None, :]
        o = np.maximum(0, np.minimum((x + 1) * n_out, (j + 1) * n_in) - np.maximum(x * n_out, j * n_in))
        out[j0:j1] = o.astype(np.float64) @ v[x0:x1]
    return out


def _resize_np(img, h, w, mode):
    """The CPU path: uint8 numpy [H, W, C] -> [h, w, C], the bytes of the contract (include/stin_hip.h, "Image resize")."""
    import numpy as np
    H, W, C = img.shape
    if mode == 'linear':
        sx, tx, bx = _linear_axis_np(W, w)
        sy, ty, by = _linear_axis_np(H, h)
        v = img.astype(np.int32)
        bx = bx[None, :, None]
        rows = (2048 - bx) * v[:, sx] + bx * v[:, tx]                                   # [H, w, C], < 2^19
        by = by[:, None, None]
        return (((2048 - by) * rows[sy] + by * rows[ty] + (1 << 21)) >> 22).astype(np.uint8)
    part = _area_axis_np(img.reshape(H, W * C).astype(np.float64), h).reshape(h, W, C)
    S = _area_axis_np(np.ascontiguousarray(part.transpose(1, 0, 2)).reshape(W, h * C), w).reshape(w, h, C).transpose(1, 0, 2)
    S = np.rint(S).astype(np.int64)
    return ((2 * S + W * H) // (2 * W * H)).astype(np.uint8)


def resize_pool_u8(pool, jobs, out_bytes, channels=3, mode='linear', out=None):
    """The ragged form under resize_u8: `pool` is a contiguous 1-D uint8 tensor that holds row-major H x W x channels images at any
    byte offsets, jobs = [(src_off, H, W, dst_off, h, w), ...]: image at byte src_off becomes h x w at byte dst_off of the result, a
    uint8 tensor of out_bytes bytes on the pool's device (`out`: write into this tensor instead of a new one; bytes that no job
    covers keep their value, in a new tensor they are 0).  The contract is include/stin_hip.h, "Image resize".  A CUDA pool: the
    table travels in one non-blocking copy from pinned memory and ONE launch serves every job (stin_resize_u8); a CPU pool takes a
    numpy path with the same bytes.  Results must not overlap each other.  TypeError / ValueError as resize_u8, and for an image or
    a result outside its buffer."""
    if mode not in RESIZE_MODES:
        raise ValueError('mode must be one of %s' % ', '.join(sorted(RESIZE_MODES)))
    channels, out_bytes = int(channels), int(out_bytes)
    if channels not in (1, 3, 4):
        raise ValueError('channels must be 1, 3 or 4')
    if not torch.is_tensor(pool) or pool.dtype != torch.uint8 or pool.dim() != 1 or not pool.is_contiguous():
        raise TypeError('pool must be a contiguous 1-D uint8 tensor')
    if out is None:
        out = torch.zeros(max(out_bytes, 0), dtype=torch.uint8, device=pool.device)
    elif (not torch.is_tensor(out) or out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous()
          or out.device != pool.device or out.numel() != out_bytes):
        raise TypeError('out must be a contiguous 1-D uint8 tensor of out_bytes bytes on the pool\'s device')
    rows = [_resize_job(job, pool.numel(), out_bytes, channels, mode) for job in jobs]
    if not rows:
        return out
    if not pool.is_cuda:
        src, dst = pool.numpy(), out.numpy()
        for so, H, W, do, h, w in rows:
            img = src[so:so + H * W * channels].reshape(H, W, channels)
            dst[do:do + h * w * channels] = _resize_np(img, h, w, mode).reshape(-1)
        return out
    words = _lib.CONSTANTS['STIN_RESIZE_JOB_WORDS']
    host = torch.empty(len(rows), words, dtype=torch.int64, pin_memory=True)
    host.copy_(torch.tensor(rows, dtype=torch.int64))
    table = host.to(pool.device, non_blocking=True)
    with torch.cuda.device(pool.device):
        _lib.check(_lib.load().stin_resize_u8(_ptr(pool), pool.numel(), _ptr(out), out_bytes, _ptr(table), len(rows), channels,
                                              _lib.CONSTANTS[RESIZE_MODES[mode]], _stream(pool)), 'stin_resize_u8')
    return out


def resize_u8(images, size, mode='linear'):
    """uint8 images [B, H, W, C] or [H, W, C] (C = 1, 3 or 4) -> the same rank at size = (h, w).  mode 'linear': bilinear with
    half-pixel centres and 11-bit coefficients, enlarging or reducing, no antialiasing - what cv2.resize does by default on 8-bit
    images to our knowledge, within one grey level of any correctly rounded bilinear resize (|out - exact| < 0.625).  mode 'area':
    the exact area average (cv2.INTER_AREA's meaning when reducing); it does not enlarge.  Integer arithmetic with one rounding:
    the contract is include/stin_hip.h, "Image resize", restated in numpy by the test suite; equal sizes return the bytes
    unchanged; NEITHER mode is pinned against a run of cv2.  The reference's Rescale runs after Normalize, on float32; this runs
    on the bytes, which differs by at most half a grey level.  CUDA tensors: one launch for the batch (stin_resize_u8, no
    synchronisation); CPU tensors: a numpy path with the same bytes.  TypeError: not a uint8 tensor; ValueError: another rank or
    C, an empty side, a side above STIN_RESIZE_MAX_SIDE, 'area' asked to enlarge."""
    if not torch.is_tensor(images) or images.dtype != torch.uint8:
        raise TypeError('images must be a uint8 tensor')
    if images.dim() not in (3, 4) or int(images.shape[-1]) not in (1, 3, 4):
        raise ValueError('images must be [B, H, W, C] or [H, W, C] with C = 1, 3 or 4')
    if mode not in RESIZE_MODES:
        raise ValueError('mode must be one of %s' % ', '.join(sorted(RESIZE_MODES)))
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError('size must be (h, w)') from None
    batch = images if images.dim() == 4 else images[None]
    B, H, W, C = (int(s) for s in batch.shape)
    rows = [(b * H * W * C, H, W, b * h * w * C, h, w) for b in range(B)]
    if not rows:
        _resize_job((0, H, W, 0, h, w), H * W * C, h * w * C, C, mode)                 # the checks, for an empty batch too
    out = resize_pool_u8(batch.contiguous().view(-1), rows, B * max(h, 0) * max(w, 0) * C, C, mode)
    out = out.view(B, h, w, C)
    return out if images.dim() == 4 else out[0]


def scan_vertex_colors(vertices, scan_dir, width=640, height=480, trajectory_slice=slice(None, None, 10), batch=32, knn=0,
                       nonrigid_iterations=0, nonrigid_solver='dense', **frame_colors_options):
    """Per-vertex colours of a mesh straight from a scan directory: the reference's load_dataset (texture_map_optimization.py:48-123)
    plus FrameColors' averaging -> (colors float32 [N, 3], count int32 [N]).  scan_dir holds color/*.jpg, depth/*.png, pose/*.txt
    (scene_io.scan_frame_files: natural order for all three) and intrinsic/intrinsic_color.txt; every trajectory_slice-th frame is
    used.  Per batch of `batch` frames: the files are read (scene_io.read_frames) and uploaded, the colour frames are resized to
    (height, width) on the device (resize_u8, 'linear': the reference's cv2.resize), the depth frames must already have that size
    (the reference asserts it), and FrameColors.add takes them with the camera of frame_intrinsics (original size: the first colour
    frame's).  knn: FrameColors.result's fill of unseen vertices; further keywords are FrameColors'.  vertices: a CUDA tensor - the
    mesh is the caller's business, as everywhere here.
    nonrigid_iterations = k > 0: what the reference asks of Open3D (run_non_rigid_optimizer) - the frames are then all kept on the
    device (0.9 MB per 480 x 640 colour frame, 0.6 MB per depth frame, 4.9 MB of gradient images), optimize_poses_nonrigid runs k
    iterations on them in depth mode at its defaults, and the colours are averaged with its poses and warp lattices
    (vertex_colors_from_frames).  0, the default: no optimisation, batch by batch, as before.  nonrigid_solver: the optimiser's
    `solver`, 'dense' (the host's, the default) or 'banded' (on the device)."""
    import os
    import numpy as np
    from . import scene_io
    width, height, step = int(width), int(height), int(batch)
    if step < 1:
        raise ValueError('batch must be positive')
    if nonrigid_solver not in NONRIGID_SOLVERS:
        raise ValueError("nonrigid_solver must be 'dense' or 'banded', not %r" % (nonrigid_solver,))
    files = scene_io.scan_frame_files(scan_dir)
    color_files, depth_files, pose_files = (files[k][trajectory_slice] for k in ('color', 'depth', 'pose'))
    if not (len(color_files) == len(depth_files) == len(pose_files)):
        raise ValueError('%d colour frames, %d depth frames and %d poses' % (len(color_files), len(depth_files), len(pose_files)))
    if not color_files:
        raise ValueError('no frames in %s' % scan_dir)
    intrinsic = np.loadtxt(os.path.join(scan_dir, 'intrinsic', 'intrinsic_color.txt'), dtype=np.float64)
    fc, dev = None, vertices.device
    resident = int(nonrigid_iterations) > 0
    kept = ([], [], [])
    for p0 in range(0, len(color_files), step):
        p1 = min(p0 + step, len(color_files))
        color, depth = scene_io.read_frames(color_files[p0:p1], depth_files[p0:p1])
        if tuple(depth.shape[1:]) != (height, width):
            raise ValueError('depth frames are %d x %d, not height x width = %d x %d' % (depth.shape[1], depth.shape[2], height, width))
        if fc is None:
            camera = frame_intrinsics(intrinsic, int(color.shape[2]), int(color.shape[1]), width, height)
            fc = FrameColors(vertices, camera, **frame_colors_options)
        poses = np.stack([np.loadtxt(name, dtype=np.float64).reshape(4, 4) for name in pose_files[p0:p1]])
        small = resize_u8(torch.from_numpy(color).to(dev), (height, width), 'linear')
        if resident:
            for k, x in zip(kept, (poses, small, torch.from_numpy(depth).to(dev))):
                k.append(x)
            continue
        fc.add(poses, small, torch.from_numpy(depth).to(dev), first_pose=p0)
    if resident:
        poses, small, depth = np.concatenate(kept[0]), torch.cat(kept[1]), torch.cat(kept[2])
        poses, flow, info = optimize_poses_nonrigid(vertices, poses, small, depth=depth, color_camera=camera,
                                                    iterations=int(nonrigid_iterations), batch=step, solver=nonrigid_solver,
                                                    **frame_colors_options)
        return vertex_colors_from_frames(vertices, poses, small, depth=depth, batch=step, color_camera=camera, knn=knn, flow=flow,
                                         lattice_step=info['lattice_step'], **frame_colors_options)
    return fc.result(knn=knn)


# ------------------------------------------------------------------------------------------------- colour-map optimisation
COLORMAP_NOT_FREE, COLORMAP_INVALID, COLORMAP_FEW_PAIRS, COLORMAP_SINGULAR = 1, 2, 4, 8      # bits of info['status']


def rigid_increment(x):
    """x = (rotation x, y, z in radians, translation x, y, z) -> D(x) float64 [4, 4] = [[Rz(x2) Ry(x1) Rx(x0), x[3:6]], [0 0 0 1]],
    the increment the rigid optimiser multiplies onto an extrinsic from the left (include/stin_hip.h, "Colour-map optimisation")."""
    import numpy as np
    x = np.asarray(x, dtype=np.float64).reshape(6)
    c, s = np.cos(x[:3]), np.sin(x[:3])
    D = np.zeros((4, 4), dtype=np.float64)
    D[0, 0], D[0, 1], D[0, 2] = c[2] * c[1], (c[2] * s[1]) * s[0] - s[2] * c[0], (c[2] * s[1]) * c[0] + s[2] * s[0]
    D[1, 0], D[1, 1], D[1, 2] = s[2] * c[1], (s[2] * s[1]) * s[0] + c[2] * c[0], (s[2] * s[1]) * c[0] - c[2] * s[0]
    D[2, 0], D[2, 1], D[2, 2] = -s[1], c[1] * s[0], c[1] * c[0]
    D[:3, 3] = x[3:6]
    D[3, 3] = 1.0
    return D


def rigid_update(E, valid, free, rows, counts, min_pairs, status):
    """One Gauss-Newton update on the host: E float64 [P, 4, 4] extrinsics (changed in place), rows [P, 28] and counts [P] as
    stin_colormap_normal_f64 writes them, status int32 [P] (bits COLORMAP_FEW_PAIRS / COLORMAP_SINGULAR are OR-ed in).  A pose moves
    when it is free, valid, has counts >= min_pairs and np.linalg.solve on its symmetrised 6 x 6 gives a finite x: E' = D(x) E.
    -> bool [P]: which poses moved."""
    import numpy as np
    iu = np.triu_indices(6)
    moved = np.zeros(E.shape[0], dtype=bool)
    for p in range(E.shape[0]):
        if not (free[p] and valid[p]):
            continue
        if int(counts[p]) < min_pairs:
            status[p] |= COLORMAP_FEW_PAIRS
            continue
        A = np.zeros((6, 6), dtype=np.float64)
        A[iu] = rows[p, :21]
        A.T[iu] = rows[p, :21]
        try:
            x = np.linalg.solve(A, -rows[p, 21:27])
        except np.linalg.LinAlgError:
            x = None
        if x is None or not np.isfinite(x).all():
            status[p] |= COLORMAP_SINGULAR
            continue
        E[p] = rigid_increment(x) @ np.ascontiguousarray(E[p])
        moved[p] = True
    return moved


def _colormap_gradients(color, images=None):
    """color uint8 [B, H, W, 3] (CUDA, contiguous) -> the intensity and gradient images int32 [B, H, W, 4] = (G, gx, gy, 0)."""
    B, H, W = (int(s) for s in color.shape[:3])
    if images is None:
        images = torch.empty(B, H, W, 4, dtype=torch.int32, device=color.device)
    _lib.check(_lib.load().stin_colormap_gradients_u8(_ptr(color), B, H, W, _ptr(images), _stream(color)), 'stin_colormap_gradients_u8')
    return images


def _colormap_proxy(total, count, proxy=None):
    """sum int64 [N, 3], count int32 [N] of FrameColors -> the proxy intensity fp64 [N]."""
    n = int(count.shape[0])
    if proxy is None:
        proxy = torch.empty(n, dtype=torch.float64, device=count.device)
    _lib.check(_lib.load().stin_colormap_proxy_f64(_ptr(total), _ptr(count), n, _ptr(proxy), _stream(count)), 'stin_colormap_proxy_f64')
    return proxy


def _colormap_workspace(n, batch, device):
    ws_bytes = _lib.load().stin_colormap_workspace_bytes(n, batch)
    if ws_bytes == 0:
        raise ValueError('%d vertices in batches of %d poses are outside what the normal-equation kernel supports' % (n, batch))
    return torch.empty(ws_bytes, dtype=torch.uint8, device=device)


def _colormap_normal(v64, rt_d, valid_d, first_pose, images, camera, z_near, bits, margin, proxy, rows, counts, ws):
    """One batch of poses -> rows fp64 [B, 28], counts int32 [B] (written in place): stin_colormap_normal_f64 on device arrays."""
    n, B = int(v64.shape[0]), int(rt_d.shape[0])
    cam = _camera_doubles(camera)
    _lib.check(_lib.load().stin_colormap_normal_f64(_ptr(v64), n, _ptr(rt_d), _ptr(valid_d), B, int(first_pose), _ptr(images),
                                                    int(images.shape[1]), int(images.shape[2]), cam, float(z_near),
                                                    _ptr(bits) if n else None, int(bits.shape[1]), int(margin), _ptr(proxy), _ptr(rows),
                                                    _ptr(counts), _ptr(ws), int(ws.numel()), _stream(v64)), 'stin_colormap_normal_f64')


def _colormap_inputs(vertices, poses, color, depth, bits, color_camera, depth_camera, iterations, free, batch, params):
    """The argument checks that the colour-map optimisers share, and the visibility both keep fixed: in depth mode one FrameColors
    pass at the given poses whose `seen` becomes the bits, in bits mode the caller's bits.
    -> (fc, color, bits, free bool [P], RT, valid, poses float64 [P, 4, 4], status int32 [P], batch, margin)"""
    import numpy as np
    if color_camera is None:
        raise ValueError('color_camera = (fx, fy, cx, cy) is required')
    if (depth is None) == (bits is None):
        raise ValueError('exactly one of depth and bits must be given')
    margin, iters, step = int(params.get('margin', 10)), int(iterations), int(batch)
    if margin < 1:
        raise ValueError('margin must be >= 1: the gradient is sampled like the colour')
    if iters < 0 or step < 1:
        raise ValueError('iterations must be >= 0 and batch positive')
    P = len(poses)
    free = np.ones(P, dtype=bool) if free is None else np.asarray(free.detach().cpu().numpy() if torch.is_tensor(free) else free)
    if free.dtype != np.bool_ or free.shape != (P,):
        raise ValueError('free must be bool [%d], one entry per pose' % P)
    c = _frames_u(color, torch.uint8, (3,), 'color')
    if int(c.shape[0]) != P:
        raise ValueError('%d poses but %d colour frames' % (P, int(c.shape[0])))
    fc = FrameColors(vertices, color_camera, depth_camera, num_poses=P if depth is not None else None, **params)
    v, n, dev = fc.vertices, int(fc.vertices.shape[0]), fc.vertices.device
    step = max(1, min(step, P, _lib.CONSTANTS['STIN_FRAMES_MAX_BATCH']))
    if depth is not None:
        d = _depth_frames(depth, P)
    else:
        vis = _pose_bits(bits, n, P, '%d poses')
    if P and 0 in c.shape:
        raise ValueError('empty frames')
    RT, valid = pose_extrinsics(poses)
    given = np.array(poses.detach().cpu().numpy() if torch.is_tensor(poses) else poses, dtype=np.float64).reshape(P, 4, 4)
    status = np.where(free, 0, COLORMAP_NOT_FREE).astype(np.int32) | np.where(valid != 0, 0, COLORMAP_INVALID).astype(np.int32)
    if depth is not None:                                              # visibility, once, at the given poses
        for p0 in range(0, P, step):
            fc.add(given[p0:p0 + step], c[p0:p0 + step], depth=d[p0:p0 + step], first_pose=p0)
        vis = fc.seen
    return fc, c, vis, free, RT, valid, given, status, step, margin


def _optimize_poses(fc, color, vis, RT, valid, given, step, info, normal, solve, flow=None, lattice_step=None):
    """The iteration of both colour-map optimisers, on the output of _colormap_inputs: the gradient images of all P > 0 frames once;
    then iterations + 1 times (the rows of info['residual']): the extrinsics (and the lattices `flow`, float64 [P, Ah, Aw, 2], changed
    in place) to the device, the colour sums at them in batches of `step` poses, the proxy, the normal equations in batches, and
    one read-back.  The optimiser brings its buffers and two functions:
    normal(batch, rt_d, valid_d, images, flow_d, proxy) launches the normal equations of the poses in the slice `batch`;
    solve(E, flow_d, valid_d, update) reads back -> (residual [P], pairs [P], moved bool [P] or None) and, where `update` (every
    iteration but the last), moves E float64 [P, 4, 4] (and flow) in place.
    Fills info['residual'], info['pairs'] (and info['flow_norm']) -> poses float64 [P, 4, 4]: the inverse of every extrinsic that
    ever moved, the given pose otherwise."""
    import numpy as np
    P, n, dev = len(given), int(fc.vertices.shape[0]), fc.vertices.device
    iters = info['residual'].shape[0] - 1
    images = torch.empty(P, int(color.shape[1]), int(color.shape[2]), 4, dtype=torch.int32, device=dev)
    for p0 in range(0, P, step):
        _colormap_gradients(color[p0:p0 + step], images[p0:p0 + step])
    proxy = torch.empty(n, dtype=torch.float64, device=dev)
    valid_d = torch.from_numpy(valid).to(dev)
    E = np.zeros((P, 4, 4), dtype=np.float64)
    E[:, :3, :] = RT.reshape(P, 3, 4)
    E[:, 3, 3] = 1.0
    ever = np.zeros(P, dtype=bool)
    for it in range(iters + 1):
        rt_d = torch.from_numpy(np.ascontiguousarray(E[:, :3, :]).reshape(P, 12)).to(dev)
        flow_d = None if flow is None else torch.from_numpy(flow).to(dev)
        fc.sum.zero_()
        fc.count.zero_()
        for p0 in range(0, P, step):
            fc._add_extrinsics(rt_d[p0:p0 + step], valid_d[p0:p0 + step], color[p0:p0 + step], p0, bits=vis,
                               flow=None if flow is None else flow_d[p0:p0 + step], lattice_step=lattice_step)
        _colormap_proxy(fc.sum, fc.count, proxy)
        for p0 in range(0, P, step):
            normal(slice(p0, p0 + step), rt_d, valid_d, images, flow_d, proxy)
        if flow is not None:
            info['flow_norm'][it] = np.abs(flow).reshape(P, -1).max(axis=1)
        info['residual'][it], info['pairs'][it], moved = solve(E, flow_d, valid_d, it < iters)
        if moved is not None:
            ever |= moved
    out = given.copy()
    for p in np.flatnonzero(ever):
        out[p] = np.linalg.inv(E[p])
    return out


def optimize_poses_rigid(vertices, poses, color, depth=None, bits=None, *, color_camera=None, depth_camera=None, iterations=30,
                         free=None, min_pairs=16, batch=64, **params):
    """The rigid colour-map optimisation (Zhou & Koltun 2014; what Open3D's colour-map pipeline does with maximum_iteration > 0
    before it averages colours): refine the camera poses photometrically, so that the frames agree on the mesh's intensities, on the
    GPU (csrc/stin_colormap.hip).  vertices [N, >= 3] float, color uint8 [P, H, W, 3] and either depth uint16 [P, Hd, Wd] or bits
    (observe_vertices' uint32 [N, words]) - CUDA tensors, checked as FrameColors.add checks them; poses [P, 4, 4] camera-to-world
    (array or tensor); color_camera (required), depth_camera and **params are FrameColors'; margin must be >= 1.
    -> (poses float64 [P, 4, 4] camera-to-world numpy, info): info['residual'] float64 and info['pairs'] int64, both
    [iterations + 1, P] - the sum of squared intensity residuals and the number of (vertex, pose) pairs of every pose before each
    update and after the last; info['status'] int32 [P], bits COLORMAP_NOT_FREE, COLORMAP_INVALID, COLORMAP_FEW_PAIRS (fewer than
    min_pairs pairs in some iteration: not moved in it), COLORMAP_SINGULAR (its 6 x 6 could not be solved in some iteration).

    Visibility is established ONCE, at the given poses: in depth mode by one FrameColors pass whose `seen` becomes the bits, in
    bits mode by the caller's bits; only the projection moves afterwards.  Per iteration (the count is fixed, there is no early
    stop: the result is a pure function of the inputs): the proxy intensity of every vertex from the integer colour sums at the
    current poses; per pair the residual between the frame's intensity and the proxy and its Jacobian for a rigid increment of the
    extrinsic; per pose the 6 x 6 normal equations, summed in a fixed order; the P x 29 numbers are read back (the only
    synchronisation) and every free, valid pose with at least min_pairs pairs takes one Gauss-Newton step on the host.  The contract
    is in include/stin_hip.h ("Colour-map optimisation"); the test suite restates it in numpy and this reproduces it byte for byte.
    free: bool [P], default all.  A held pose takes part in the proxy but never moves - anchor keyframes with it: with every pose
    free the cameras settle on a consensus, which need not be the truth.  A pose that never moved (held, invalid, too few pairs)
    comes back exactly as given.  Memory: the intensity and gradient images of ALL P frames are built once, 16 bytes per pixel
    (4.9 MB per 480 x 640 frame); the rows are computed in batches of `batch` poses (the result does not depend on it).

    The recipe: poses, info = optimize_poses_rigid(vertices, poses, color, depth, color_camera=cam); then
    vertex_colors_from_frames(vertices, poses, color, depth, color_camera=cam) with the returned poses.
    Not Open3D's result and not pinned against a run of it; the non-rigid optimisation (per-camera warp grids) is
    optimize_poses_nonrigid, which runs this loop first when asked to."""
    import numpy as np
    fc, c, vis, free, RT, valid, given, status, step, margin = _colormap_inputs(vertices, poses, color, depth, bits, color_camera,
                                                                                depth_camera, iterations, free, batch, params)
    P, iters, min_pairs = len(given), int(iterations), int(min_pairs)
    v, n, dev = fc.vertices, int(fc.vertices.shape[0]), fc.vertices.device
    info = dict(residual=np.zeros((iters + 1, P), dtype=np.float64), pairs=np.zeros((iters + 1, P), dtype=np.int64), status=status)
    if P == 0:
        return given, info
    rows = torch.empty(P, _lib.CONSTANTS['STIN_COLORMAP_ROW_DOUBLES'], dtype=torch.float64, device=dev)
    counts = torch.empty(P, dtype=torch.int32, device=dev)
    ws = _colormap_workspace(n, step, dev)

    def normal(batch, rt_d, valid_d, images, flow_d, proxy):
        _colormap_normal(v, rt_d[batch], valid_d[batch], batch.start, images[batch], fc.color_camera, fc.z_near, vis, margin, proxy,
                         rows[batch], counts[batch], ws)

    def solve(E, flow_d, valid_d, update):
        r, k = rows.cpu().numpy(), counts.cpu().numpy()
        return r[:, 27], k, rigid_update(E, valid, free, r, k, min_pairs, status) if update else None

    return _optimize_poses(fc, c, vis, RT, valid, given, step, info, normal, solve), info


# --------------------------------------------------------------------------------------- non-rigid colour-map optimisation
def nonrigid_lattice(height, width, lattice_step):
    """-> (Ah, Aw): the anchors of a warp lattice of step lattice_step over a height x width frame, at the pixels (j S, i S):
    ceil((height - 1) / S) + 1 rows and ceil((width - 1) / S) + 1 columns (include/stin_hip.h, "Non-rigid colour-map optimisation")."""
    S = int(lattice_step)
    if S < 1:
        raise ValueError('lattice_step must be >= 1')
    if int(height) < 2 or int(width) < 2:
        raise ValueError('a warp lattice needs frames of at least 2 x 2 pixels')
    return -(-(int(height) - 1) // S) + 1, -(-(int(width) - 1) // S) + 1


def _nonrigid_flow(flow, lattice_step, P, H, W):
    """flow as a caller gives it (array or tensor) -> (float64 tensor [P, Ah, Aw, 2], contiguous, where it was; lattice_step)"""
    import numpy as np
    if lattice_step is None:
        raise ValueError('flow needs its lattice_step')
    Ah, Aw = nonrigid_lattice(H, W, lattice_step)
    t = flow if torch.is_tensor(flow) else torch.from_numpy(np.ascontiguousarray(flow))
    if t.dtype != torch.float64 or tuple(t.shape) != (P, Ah, Aw, 2):
        raise ValueError('flow must be float64 [%d, %d, %d, 2] for %d frames of %d x %d and lattice_step %d'
                         % (P, Ah, Aw, P, H, W, int(lattice_step)))
    return t.contiguous(), int(lattice_step)


_NONRIGID_TRI = tuple((i, j) for i in range(14) for j in range(i, 14))


def _nonrigid_move(E, flow, p, x):
    """Pose p takes the step x of a solve: E[p] = D(x[:6]) E[p], flow[p] += x[6:], both in place."""
    import numpy as np
    E[p] = rigid_increment(x[:6]) @ np.ascontiguousarray(E[p])
    flow[p] += x[6:].reshape(flow.shape[1:])


def nonrigid_update(E, flow, valid, free, blocks, counts, n_vertices, anchor_weight, min_pairs, status):
    """One Gauss-Newton update of poses and warp lattices on the host: E float64 [P, 4, 4] extrinsics and flow float64
    [P, Ah, Aw, 2] (both changed in place), blocks [P, cells, 120] and counts [P, cells] as stin_nonrigid_normal_f64 writes them,
    status int32 [P] (COLORMAP_FEW_PAIRS / COLORMAP_SINGULAR are OR-ed in).  Per free, valid pose with n_p = counts.sum() >=
    min_pairs: the (6 + 2 Ah Aw)^2 system from the blocks, cells ascending; every anchor unknown regularised with wgt =
    anchor_weight n_p / n_vertices (A[k][k] += wgt^2, b[k] += wgt^2 f_k); x = np.linalg.solve(A, -b); E' = D(x[:6]) E, flow += x[6:].
    A pose whose system is singular or whose x is not finite does not move.  -> bool [P]: which poses moved."""
    import numpy as np
    P, Ah, Aw = (int(s) for s in flow.shape[:3])
    n = 6 + 2 * Ah * Aw
    # the unknowns of every cell's 14 local ones, ascending within a cell (so that the triangle of a block lands in the upper triangle),
    # and from them the targets of every block entry, cell-major: np.add.at adds in the order of its index array - cells ascending
    ti, tj = (np.array(k) for k in zip(*_NONRIGID_TRI))
    cell = np.arange((Ah - 1) * (Aw - 1))
    anchors = ((cell // (Aw - 1)) * Aw + cell % (Aw - 1))[:, None] + np.array([0, 1, Aw, Aw + 1])
    g = np.concatenate([np.broadcast_to(np.arange(6), (len(cell), 6)), 6 + (2 * anchors[:, :, None] + np.arange(2)).reshape(len(cell), 8)], axis=1)
    gi, gj, gb = g[:, ti].reshape(-1), g[:, tj].reshape(-1), g.reshape(-1)
    moved = np.zeros(P, dtype=bool)
    for p in range(P):
        if not (free[p] and valid[p]):
            continue
        n_p = int(counts[p].sum())
        if n_p < min_pairs:
            status[p] |= COLORMAP_FEW_PAIRS
            continue
        A, b = np.zeros((n, n), dtype=np.float64), np.zeros(n, dtype=np.float64)
        np.add.at(A, (gi, gj), np.ascontiguousarray(blocks[p, :, :105]).reshape(-1))
        np.add.at(b, gb, np.ascontiguousarray(blocks[p, :, 105:119]).reshape(-1))
        with np.errstate(all='ignore'):
            wgt = (np.float64(anchor_weight) * np.float64(n_p)) / np.float64(n_vertices)
        anchor = np.arange(6, n)
        A[anchor, anchor] += wgt * wgt
        b[6:] += (wgt * wgt) * flow[p].reshape(-1)
        lower = A.T.copy()                                              # A is upper triangular so far: mirror it
        np.fill_diagonal(lower, 0.0)
        A += lower
        try:
            x = np.linalg.solve(A, -b)
        except np.linalg.LinAlgError:
            x = None
        if x is None or not np.isfinite(x).all():
            status[p] |= COLORMAP_SINGULAR
            continue
        _nonrigid_move(E, flow, p, x)
        moved[p] = True
    return moved


def _nonrigid_workspace(n, batch, H, W, lattice_step, device):
    """The key buffer of one batch: int64 [batch * n] on the device (stin_nonrigid_workspace_bytes)."""
    ws_bytes = _lib.load().stin_nonrigid_workspace_bytes(n, batch, H, W, int(lattice_step))
    if ws_bytes == 0:
        raise ValueError('%d vertices, batches of %d poses and a lattice of step %d over %d x %d frames are outside what the '
                         'non-rigid kernels support' % (n, batch, int(lattice_step), H, W))
    return torch.empty(ws_bytes // 8, dtype=torch.int64, device=device)


def _nonrigid_keys(v64, rt_d, valid_d, first_pose, H, W, flow_d, lattice_step, camera, z_near, bits, margin, keys):
    """One batch of poses -> keys int64 [B * N] (the head of `keys`, written in place): stin_nonrigid_keys_f64 on device arrays."""
    n, B = int(v64.shape[0]), int(rt_d.shape[0])
    cam = _camera_doubles(camera)
    _lib.check(_lib.load().stin_nonrigid_keys_f64(_ptr(v64), n, _ptr(rt_d), _ptr(valid_d), B, int(first_pose), int(H), int(W),
                                                  _ptr(flow_d), int(lattice_step), cam, float(z_near), _ptr(bits) if n else None,
                                                  int(bits.shape[1]), int(margin), _ptr(keys), int(keys.numel()) * 8, _stream(v64)),
               'stin_nonrigid_keys_f64')
    return keys[:B * n]


def _nonrigid_blocks(v64, rt_d, valid_d, first_pose, images, flow_d, lattice_step, camera, z_near, margin, proxy, ordered, blocks, counts):
    """One batch of poses and its SORTED keys -> blocks fp64 [B, cells, 120], counts int32 [B, cells] (written in place)."""
    n, B = int(v64.shape[0]), int(rt_d.shape[0])
    cam = _camera_doubles(camera)
    _lib.check(_lib.load().stin_nonrigid_normal_f64(_ptr(v64), n, _ptr(rt_d), _ptr(valid_d), B, int(first_pose), _ptr(images),
                                                    int(images.shape[1]), int(images.shape[2]), _ptr(flow_d), int(lattice_step), cam,
                                                    float(z_near), int(margin), _ptr(proxy), _ptr(ordered), int(ordered.numel()) * 8,
                                                    _ptr(blocks), _ptr(counts), _stream(v64)), 'stin_nonrigid_normal_f64')


def _nonrigid_normal(v64, rt_d, valid_d, first_pose, images, flow_d, lattice_step, camera, z_near, bits, margin, proxy, blocks, counts, keys):
    """One batch of poses -> blocks fp64 [B, cells, 120], counts int32 [B, cells] (written in place): the key kernel, the sort of the
    B N keys (rocPRIM through torch.sort), and one workgroup per (pose, cell) over its run of sorted keys."""
    made = _nonrigid_keys(v64, rt_d, valid_d, first_pose, images.shape[1], images.shape[2], flow_d, lattice_step, camera, z_near, bits,
                          margin, keys)
    ordered = torch.sort(made)[0] if made.numel() else keys
    _nonrigid_blocks(v64, rt_d, valid_d, first_pose, images, flow_d, lattice_step, camera, z_near, margin, proxy, ordered, blocks, counts)


def _dev_array(t, dtype, shape, name):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise ValueError('%s must be a CUDA tensor' % name)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise ValueError('%s must be %s %s' % (name, str(dtype).replace('torch.', ''), list(shape)))
    return t.contiguous()


def nonrigid_solve(blocks, counts, flow, valid, free, n_vertices, anchor_weight, min_pairs):
    """The linear solve of one non-rigid update on the device (csrc/stin_nonrigid_solve.hip; include/stin_hip.h, "Non-rigid solve"):
    per pose the (6 + 2 Ah Aw) system is gathered from the blocks into band storage, pose last, and factored by a banded-arrow
    Cholesky in one workgroup - about (2 Ah Aw)(2 Aw + 3)^2 multiply-adds where the dense solve spends (6 + 2 Ah Aw)^3 / 3.
    blocks float64 [P, cells, 120] and counts int32 [P, cells] as stin_nonrigid_normal_f64 writes them, flow float64 [P, Ah, Aw, 2],
    valid and free uint8 or bool [P]: CUDA tensors.  -> (x float64 [P, 6 + 2 Ah Aw] in the order of the unknowns - the pose's six,
    then the anchors' offsets -, residual float64 [P], pairs int64 [P], status int32 [P]) on the device.  status holds
    COLORMAP_FEW_PAIRS / COLORMAP_SINGULAR of THIS call; a pose that is held, invalid, short of min_pairs or singular has an x row
    of +0.0.  residual and pairs are those of every pose.  A lattice of more than 41 columns is not supported (ValueError: use
    solver='dense').  The workspace (the band factors: 8 (2 Ah Aw (2 Aw + 4) + 7 (6 + 2 Ah Aw)) bytes per pose) is allocated here.
    The test suite restates the contract in numpy and this reproduces it byte for byte; it agrees with np.linalg.solve to rounding,
    and reports COLORMAP_SINGULAR where a pivot is not positive."""
    if not (torch.is_tensor(flow) and flow.dim() == 4 and int(flow.shape[3]) == 2):
        raise ValueError('flow must be a float64 CUDA tensor [P, Ah, Aw, 2]')
    P, Ah, Aw = (int(s) for s in flow.shape[:3])
    if Ah < 2 or Aw < 2:
        raise ValueError('a warp lattice has at least 2 x 2 anchors')
    cells = (Ah - 1) * (Aw - 1)
    flow = _dev_array(flow, torch.float64, (P, Ah, Aw, 2), 'flow')
    blocks = _dev_array(blocks, torch.float64, (P, cells, _lib.CONSTANTS['STIN_NONRIGID_BLOCK_DOUBLES']), 'blocks')
    counts = _dev_array(counts, torch.int32, (P, cells), 'counts')
    flags = []
    for name, t in (('valid', valid), ('free', free)):
        if torch.is_tensor(t) and t.dtype == torch.bool:
            t = t.to(torch.uint8)
        flags.append(_dev_array(t, torch.uint8, (P,), name))
    if int(n_vertices) < 0 or int(min_pairs) < 0:
        raise ValueError('n_vertices and min_pairs must be >= 0')
    if Aw > _lib.CONSTANTS['STIN_NONRIGID_SOLVE_MAX_AW']:
        raise ValueError("a lattice of %d columns is wider than the %d the banded solve supports: use solver='dense'"
                         % (Aw, _lib.CONSTANTS['STIN_NONRIGID_SOLVE_MAX_AW']))
    dev, n = flow.device, 6 + 2 * Ah * Aw
    x = torch.empty(P, n, dtype=torch.float64, device=dev)
    residual = torch.empty(P, dtype=torch.float64, device=dev)
    pairs = torch.empty(P, dtype=torch.int64, device=dev)
    status = torch.empty(P, dtype=torch.int32, device=dev)
    lib, step = _lib.load(), _lib.CONSTANTS['STIN_NONRIGID_SOLVE_MAX_BATCH']
    for p0 in range(0, P, step):
        B = min(step, P - p0)
        ws_bytes = lib.stin_nonrigid_solve_workspace_bytes(B, Ah, Aw)
        if ws_bytes == 0:
            raise ValueError("a lattice of %d x %d anchors is outside what the banded solve supports: use solver='dense'" % (Ah, Aw))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.stin_nonrigid_solve_f64(_ptr(blocks[p0:]), _ptr(counts[p0:]), _ptr(flow[p0:]), _ptr(flags[0][p0:]),
                                               _ptr(flags[1][p0:]), B, Ah, Aw, int(n_vertices), float(anchor_weight), int(min_pairs),
                                               _ptr(x[p0:]), _ptr(residual[p0:]), _ptr(pairs[p0:]), _ptr(status[p0:]), _ptr(ws),
                                               ws_bytes, _stream(flow)), 'stin_nonrigid_solve_f64')
    return x, residual, pairs, status


NONRIGID_SOLVERS = ('dense', 'banded')


def optimize_poses_nonrigid(vertices, poses, color, depth=None, bits=None, *, color_camera=None, depth_camera=None, iterations=30,
                            rigid_iterations=0, lattice_step=None, vertical_anchors=16, anchor_weight=0.316, free=None, min_pairs=16,
                            batch=64, solver='dense', **params):
    """The non-rigid colour-map optimisation (Zhou & Koltun 2014, section 5; Open3D's run_non_rigid_optimizer, the call the
    reference's texture_map_optimization.py makes): beside its pose every frame gets a low-resolution warp lattice - an (x, y) offset
    in pixels at anchors every lattice_step pixels, interpolated bilinearly - and both are refined photometrically on the GPU
    (csrc/stin_nonrigid.hip).  The lattice absorbs what no rigid pose can: rolling shutter, lens distortion, a depth/colour
    misregistration that differs across the frame.  Arguments as optimize_poses_rigid's; margin must be >= 1.
    -> (poses float64 [P, 4, 4] camera-to-world numpy, flow float64 [P, Ah, Aw, 2] numpy, info).  info['residual'], info['pairs'],
    info['status'] as the rigid optimiser's; info['flow_norm'] float64 [iterations + 1, P]: the largest |offset| of every pose's
    lattice, in pixels, beside each residual; info['lattice_step']; info['rigid']: the rigid loop's info when rigid_iterations > 0.

    The iteration is the rigid one's: visibility is established ONCE, at the given poses (depth mode: one unwarped FrameColors pass;
    the depth test knows no warp), the iteration count is fixed, there is one read-back per iteration (P x cells x 121 numbers), and
    the result is a pure function of the inputs, independent of `batch`.  Per iteration: the colour sums at the warped positions,
    the proxy, per (pose, lattice cell) the normal equations of the 14 unknowns a pair touches - the pose's six and its cell's four
    anchors - summed in ascending vertex id, and on the host one Gauss-Newton step per free, valid pose with at least min_pairs
    pairs (nonrigid_update).  Every anchor is pulled towards zero with weight anchor_weight n_p / N (n_p pairs of the pose, N
    vertices): the shape of Open3D's non_rigid_anchor_point_weight term as far as we know, 0.316 being its default; NOT checked
    against Open3D.  A held pose takes part in the proxy, never moves and keeps a zero flow.
    rigid_iterations = k > 0: optimize_poses_rigid runs k iterations first, under the same visibility, and this loop starts from its
    poses.  lattice_step: default ceil((H - 1) / (vertical_anchors - 1)) - 32 pixels at 480 rows, 16 x 21 anchors and 678 unknowns
    per frame, the size the paper uses.  A finer lattice is allowed; the host solve is dense, O((6 + 2 Ah Aw)^3) per free pose and
    iteration (678 unknowns: about 0.1 Gflop and 3.7 MB; step 8 at 480 x 640: 9 888 unknowns, 0.3 Tflop and 0.8 GB per pose).
    solver: 'dense' (the default) is that host solve, np.linalg.solve on the blocks read back.  'banded' solves on the device
    (nonrigid_solve: a banded-arrow Cholesky per pose, one call per iteration on all P poses) and reads back x, the residuals, pair
    counts and status instead of the blocks - P (6 + 2 Ah Aw) numbers for P cells 121; the poses and lattices are then updated on
    the host by the code the dense path uses, so the two solvers differ in x only: to rounding, not in bytes, which is why 'dense'
    stays the default and 'banded' has a contract and a restatement of its own ("Non-rigid solve").  Cholesky reports a pose whose
    system is not positive definite as COLORMAP_SINGULAR where LU may still move it.  'banded' supports lattices of up to 41 columns
    (step 16 at 640 pixels; ValueError beyond).  info['solver'] names the solver.

    The recipe: poses, flow, info = optimize_poses_nonrigid(vertices, poses, color, depth, color_camera=cam); then
    vertex_colors_from_frames(vertices, poses, color, depth, color_camera=cam, flow=flow, lattice_step=info['lattice_step']).
    The contract is in include/stin_hip.h ("Non-rigid colour-map optimisation"); the test suite restates it in numpy and this
    reproduces it byte for byte.  Not Open3D's result and not pinned against a run of it; warp-aware depth visibility is not built."""
    import numpy as np
    if solver not in NONRIGID_SOLVERS:
        raise ValueError("solver must be 'dense' or 'banded', not %r" % (solver,))
    if int(rigid_iterations) < 0 or int(vertical_anchors) < 2:
        raise ValueError('rigid_iterations must be >= 0 and vertical_anchors >= 2')
    if lattice_step is not None and int(lattice_step) < 1:
        raise ValueError('lattice_step must be >= 1')
    fc, c, vis, free, RT, valid, given, status, step, margin = _colormap_inputs(vertices, poses, color, depth, bits, color_camera,
                                                                                depth_camera, iterations, free, batch, params)
    P, iters, min_pairs = len(given), int(iterations), int(min_pairs)
    v, n, dev = fc.vertices, int(fc.vertices.shape[0]), fc.vertices.device
    H, W = int(c.shape[1]), int(c.shape[2])
    S = -(-(H - 1) // (int(vertical_anchors) - 1)) if lattice_step is None else int(lattice_step)
    Ah, Aw = nonrigid_lattice(H, W, max(S, 1))
    cells = (Ah - 1) * (Aw - 1)
    flow = np.zeros((P, Ah, Aw, 2), dtype=np.float64)
    info = dict(residual=np.zeros((iters + 1, P), dtype=np.float64), pairs=np.zeros((iters + 1, P), dtype=np.int64), status=status,
                flow_norm=np.zeros((iters + 1, P), dtype=np.float64), lattice_step=S, solver=solver)
    if solver == 'banded' and Aw > _lib.CONSTANTS['STIN_NONRIGID_SOLVE_MAX_AW']:
        raise ValueError("a lattice of %d columns is wider than the %d the banded solve supports: use solver='dense'"
                         % (Aw, _lib.CONSTANTS['STIN_NONRIGID_SOLVE_MAX_AW']))
    if P == 0:
        return given, flow, info
    if int(rigid_iterations) > 0:                                      # the rigid loop first, under the same visibility
        given, info['rigid'] = optimize_poses_rigid(v, given, c, bits=vis, color_camera=fc.color_camera, iterations=int(rigid_iterations),
                                                    free=free, min_pairs=min_pairs, batch=step, **params)
        status |= info['rigid']['status']
        RT, valid = pose_extrinsics(given)
    keys = _nonrigid_workspace(n, step, H, W, S, dev)
    blocks = torch.empty(P, cells, _lib.CONSTANTS['STIN_NONRIGID_BLOCK_DOUBLES'], dtype=torch.float64, device=dev)
    counts = torch.empty(P, cells, dtype=torch.int32, device=dev)
    free_d = torch.from_numpy(free.astype(np.uint8)).to(dev) if solver == 'banded' else None

    def normal(batch, rt_d, valid_d, images, flow_d, proxy):
        _nonrigid_normal(v, rt_d[batch], valid_d[batch], batch.start, images[batch], flow_d[batch], S, fc.color_camera, fc.z_near, vis,
                         margin, proxy, blocks[batch], counts[batch], keys)

    def solve_dense(E, flow_d, valid_d, update):
        blk, k = blocks.cpu().numpy(), counts.cpu().numpy()
        moved = nonrigid_update(E, flow, valid, free, blk, k, n, anchor_weight, min_pairs, status) if update else None
        return np.cumsum(blk[:, :, 119], axis=1)[:, -1], k.sum(axis=1), moved           # cells ascending

    def solve_banded(E, flow_d, valid_d, update):                      # the solve on the device: x comes back, not the blocks
        x, e, k, st = (t.cpu().numpy() for t in nonrigid_solve(blocks, counts, flow_d, valid_d, free_d, n, anchor_weight, min_pairs))
        if not update:
            return e, k, None
        status[:] |= st
        moved = (st == 0) & free & (valid != 0)
        for p in np.flatnonzero(moved):
            _nonrigid_move(E, flow, p, x[p])
        return e, k, moved

    out = _optimize_poses(fc, c, vis, RT, valid, given, step, info, normal, solve_banded if solver == 'banded' else solve_dense,
                          flow=flow, lattice_step=S)
    return out, flow, info


# ------------------------------------------------------------------------------------------------------------ surface samples
_GOLDEN, _M64 = 0x9E3779B97F4A7C15, (1 << 64) - 1
SURFACE_MAX_CANDIDATES = 1 << 20     # upper end of circle_masks_on_surface's default candidate count
_POISSON_GROUP = 4                   # decision rounds per host read of poisson_disk


def _mix64(z):
    """The hash finaliser of the circle masks and the surface samples (csrc: mix64) on Python integers."""
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def surface_stream_seed(seed, m):
    """Seed of mask m's centre stream in circle_masks_on_surface: mix64(mix64(seed + G) + (m + 1) G) (include/stin_hip.h)."""
    return _mix64(_mix64(int(seed) + _GOLDEN) + (int(m) + 1) * _GOLDEN)


def _surface_mesh(vertices, faces, what):
    """-> (fp64 vertices, int64 faces as given, cum int64 [F], state int64 [4] on the host): checked faces (IndexError), face
    weights and their scan (stin_surface_weights_f64); ValueError for a non-finite vertex of a face or no positive weight."""
    v = _xyz64(vertices, 'vertices')
    if not (torch.is_tensor(faces) and faces.is_cuda):
        raise TypeError('faces must be a CUDA tensor (no CPU fallback exists)')
    lib = _lib.load()
    n = int(v.shape[0])
    _checked_faces(faces, n, what)                                      # the range check; a face that repeats a vertex has weight 0
    f = faces.long().reshape(-1, 3).contiguous()
    nf = int(f.shape[0])
    if nf > _lib.CONSTANTS['STIN_SURFACE_MAX_FACES']:
        raise ValueError('%s: more than %d faces' % (what, _lib.CONSTANTS['STIN_SURFACE_MAX_FACES']))
    cum = torch.empty(max(nf, 1), dtype=torch.int64, device=v.device)[:nf]
    state = torch.empty(4, dtype=torch.int64, device=v.device)
    ws_bytes = lib.stin_surface_weights_workspace_bytes(nf)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=v.device)
    _lib.check(lib.stin_surface_weights_f64(_ptr(v), n, _ptr(f) if nf else None, nf, _ptr(cum) if nf else None, _ptr(state), _ptr(ws),
                                            ws_bytes, _stream(v)), 'stin_surface_weights_f64')
    st = state.cpu()
    if int(st[1]) & 1:
        raise IndexError('%s: a face refers to a vertex outside [0, %d)' % (what, n))
    if int(st[1]) & 2:
        raise ValueError('%s: a vertex of a face is not finite (or its area overflows)' % what)
    if int(st[2]) <= 0:
        raise ValueError('%s: the mesh has no face of positive area' % what)
    return v, f, cum, state, st


def _surface_area(st):
    """The area the integer weights stand for: T 2^(e - 40) / 2 with (_, e) = frexp(Amax) - the same on every run."""
    import math
    amax = float(st[0:1].numpy().view('float64')[0])
    return math.ldexp(float(int(st[2])), math.frexp(amax)[1] - 40) / 2.0


def _surface_draw(v, f, cum, state, n, seed, first):
    lib = _lib.load()
    n, dev = int(n), v.device
    points = torch.empty(max(n, 1), 3, dtype=torch.float64, device=dev)[:n]
    face = torch.empty(max(n, 1), dtype=torch.int64, device=dev)[:n]
    bary = torch.empty(max(n, 1), 3, dtype=torch.float64, device=dev)[:n]
    if n:
        _lib.check(lib.stin_surface_sample_f64(_ptr(v), int(v.shape[0]), _ptr(f), int(f.shape[0]), _ptr(cum), n, int(seed) & _M64,
                                               int(first) & _M64, _ptr(points), _ptr(face), _ptr(bary), _ptr(state), _stream(v)),
                   'stin_surface_sample_f64')
    return points, face, bary


def sample_surface(vertices, faces, n, seed=0, first=0):
    """Area-weighted uniform points on a triangle mesh (vertices [N, >= 3] float, faces [F, 3] int; CUDA) ->
    (points float64 [n, 3], face int64 [n] - ids into `faces` as given -, bary float64 [n, 3]).  Sample i depends on
    (seed, first + i) only, so ``sample_surface(v, f, n, seed, first=k)`` is the tail of a longer draw.  Integer face weights
    (exact in any summation order), a counter hash per sample, a binary search and the square-root map: include/stin_hip.h,
    "Surface samples" (csrc/stin_surface.hip).  A face of zero area - one that repeats a vertex included - is never drawn.
    IndexError for a face index out of range; ValueError for a non-finite vertex of a face or a mesh without positive area."""
    if int(n) < 0 or int(first) < 0:
        raise ValueError('sample_surface: n and first must be >= 0')
    v, f, cum, state, _ = _surface_mesh(vertices, faces, 'sample_surface')
    return _surface_draw(v, f, cum, state, n, seed, first)


def _ordered_bits_to_float(k):
    import numpy as np
    k &= _M64
    b = (k & ~(1 << 63)) if k >> 63 else (~k & _M64)
    return float(np.array([b], dtype=np.uint64).view(np.float64)[0])


def poisson_disk(points, radius, return_info=False):
    """The Poisson-disk subset of `points` ([C, >= 3] float, CUDA) in index order: candidate i is kept iff no kept j < i has
    (dx dx + dy dy) + dz dz < radius radius in fp64 (strict) -> the kept indices, int64 ascending.  The unique sequential-greedy
    set; every prefix of the result is the result for the same prefix of candidates.  On the device: a uniform grid of cell edge
    radius (1 + 2^-20) (stin_poisson_grid_f64), then decision rounds until nobody is undecided (stin_poisson_rounds_f64; the
    host reads one count per %d rounds).  The grid and the schedule do not change the result (include/stin_hip.h).
    ValueError for radius <= 0, a non-finite point or more than 2^21 cells along an axis.
    return_info=True: also a dict with 'rounds' (decision rounds until the last candidate was settled), 'launched' (rounds
    launched), 'grid' (cells per axis) and 'cell' (the cell edge).""" % _POISSON_GROUP
    import math
    p = _xyz64(points, 'points')
    r = float(radius)
    if not (r > 0.0 and math.isfinite(r)):
        raise ValueError('poisson_disk: radius must be positive and finite')
    lib = _lib.load()
    C, dev = int(p.shape[0]), p.device
    if C == 0:
        out = torch.empty(0, dtype=torch.int64, device=dev)
        return (out, dict(rounds=0, launched=0, grid=(0, 0, 0), cell=r * (1.0 + 2.0 ** -20))) if return_info else out
    order = torch.empty(C, dtype=torch.int32, device=dev)
    runs = torch.empty(C, 18, dtype=torch.int32, device=dev)
    decided = torch.empty(C, dtype=torch.uint8, device=dev)
    state = torch.empty(8, dtype=torch.int64, device=dev)
    ws_bytes = lib.stin_poisson_grid_workspace_bytes(C)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    _lib.check(lib.stin_poisson_grid_f64(_ptr(p), C, r, _ptr(order), _ptr(runs), _ptr(decided), _ptr(state), _ptr(ws), ws_bytes,
                                         _stream(p)), 'stin_poisson_grid_f64')
    st = [int(x) for x in state.cpu()]
    if st[6] & 1:
        raise ValueError('poisson_disk: a point is not finite')
    if st[6] & 2:
        raise ValueError('poisson_disk: more than 2^21 cells of edge %g along an axis' % r)
    del ws
    remaining = torch.empty(_POISSON_GROUP, dtype=torch.int64, device=dev)
    rounds = launched = 0
    while True:
        if launched >= C + _POISSON_GROUP:                              # (the lowest undecided index decides in every round)
            raise RuntimeError('poisson_disk: %d candidates still undecided after %d rounds' % (int(left[-1]), launched))
        _lib.check(lib.stin_poisson_rounds_f64(_ptr(p), C, r, _ptr(order), _ptr(runs), _ptr(decided), _POISSON_GROUP,
                                               _ptr(remaining), _stream(p)), 'stin_poisson_rounds_f64')
        left = remaining.cpu().tolist()
        launched += _POISSON_GROUP
        if 0 in left:
            rounds += left.index(0) + 1
            break
        rounds += _POISSON_GROUP
    out = torch.nonzero(decided == 1).reshape(-1)
    if not return_info:
        return out
    h = r * (1.0 + 2.0 ** -20)
    lo, hi = [_ordered_bits_to_float(k) for k in st[0:3]], [_ordered_bits_to_float(k) for k in st[3:6]]
    grid = tuple(int(math.floor((b - a) / h)) + 1 for a, b in zip(lo, hi))
    return out, dict(rounds=rounds, launched=launched, grid=grid, cell=h)


def first_occurrences(ids, num_values):
    """`ids` (int64, CUDA, values in [0, num_values)) without its repeats, every value at its first position, order kept: an integer
    atomicMin of the stream position per value, then one compare (stin_first_occurrence_i64)."""
    if not (torch.is_tensor(ids) and ids.is_cuda):
        raise TypeError('ids must be a CUDA tensor (no CPU fallback exists)')
    lib = _lib.load()
    s = ids.long().reshape(-1).contiguous()
    n, N, dev = int(s.numel()), int(num_values), s.device
    if n == 0:
        return s
    pos = torch.empty(max(N, 1), dtype=torch.int64, device=dev)
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(lib.stin_first_occurrence_i64(_ptr(s), n, N, _ptr(pos), _ptr(keep), _ptr(bad), _stream(s)), 'stin_first_occurrence_i64')
    if int(bad.item()) != 0:
        raise IndexError('first_occurrences: a value lies outside [0, %d)' % N)
    return s[keep.bool()]


def _surface_centres(v, f, cum, state, candidates, seed, spacing):
    pts, _, _ = _surface_draw(v, f, cum, state, candidates, seed, 0)
    if spacing is not None:
        pts = pts[poisson_disk(pts, spacing)]
    if pts.shape[0] == 0:
        return torch.empty(0, dtype=torch.int64, device=v.device)
    return first_occurrences(nearest(pts, v), int(v.shape[0]))


def surface_centres(vertices, faces, candidates, seed=0, spacing=None):
    """Vertex ids (int64, CUDA) spread over the SURFACE of a mesh, in stream order: ``sample_surface(candidates, seed)``, thinned by
    ``poisson_disk(spacing)`` when spacing is given (Euclidean, in the units of the vertices), snapped to the nearest vertex
    (``nearest``), repeats removed keeping the first occurrence.  Every prefix of the result is a well-spread set."""
    if int(candidates) < 0:
        raise ValueError('surface_centres: candidates must be >= 0')
    v, f, cum, state, _ = _surface_mesh(vertices, faces, 'surface_centres')
    return _surface_centres(v, f, cum, state, int(candidates), seed, spacing)


def default_surface_candidates(area, num_vertices, spacing=None):
    """The candidate count circle_masks_on_surface uses when none is given: with a spacing, ceil(4 area / spacing^2) - about five
    darts for every point a saturated Poisson-disk set of that spacing can hold (~0.7 area / spacing^2) -, else the number of
    vertices (no more centres than that exist); clamped to [1024, SURFACE_MAX_CANDIDATES]."""
    import math
    c = int(num_vertices) if spacing is None else int(math.ceil(4.0 * float(area) / (float(spacing) * float(spacing))))
    return min(max(c, 1024), SURFACE_MAX_CANDIDATES)


def circle_masks_on_surface(vertices, faces, radius=16, frac_masked_vertices=0.25, num_masks=1, seed=0, spacing=None, candidates=None,
                            edge_index=None, max_iters=32, return_centres=False):
    """Circle masks whose centres are spread over the surface instead of over the vertex ids: int64 [num_masks, N], mask[v] =
    max(0, R - hop distance to the nearest centre), ready for ``scene_io.write_circle_masks``.  The reference's loop
    (``circle_masks``; that function stays the way to reproduce the reference's files) with the sampler its TODO asks for: mask m
    draws ``surface_centres(candidates, surface_stream_seed(seed, m), spacing)`` once and every batch - 10 centres, then
    k = int(total * (frac / cur - 1)) more until cur >= frac or k <= 0 - takes the next k entries of that stream.  A stream with
    fewer than k entries left gives what it has; the mask is then reported `exhausted` and the loop stops.  Hop distances
    (``circle_mask_from_centres``' pass) run on the mesh's own edges, or on `edge_index` when given.  candidates=None:
    ``default_surface_candidates(area, N, spacing)``.  One host read per batch (an offline path).  Spacing is Euclidean, radii are
    hop counts; NOT pinned against Open3D's sample_points_poisson_disk.
    return_centres=True: also a dict in circle_masks' shape (one graph): 'centres'[m][0] (one int64 tensor per batch), 'sizes' /
    'counts' (int64 [M, 1, max_iters]), 'batches', 'masked' ([M, 1]), 'capped' and 'exhausted' (bool [M, 1]), 'candidates'."""
    v, f, cum, state, st = _surface_mesh(vertices, faces, 'circle_masks_on_surface')
    n, dev, M, it = int(v.shape[0]), v.device, int(num_masks), int(max_iters)
    frac = float(frac_masked_vertices)
    if int(radius) < 1 or M < 1 or it < 1:
        raise ValueError('circle_masks_on_surface: radius, num_masks and max_iters must be >= 1')
    cand = int(candidates) if candidates is not None else default_surface_candidates(_surface_area(st), n, spacing)
    ei = edge_index.to(dev) if edge_index is not None else edges_from_faces(f, n)
    adj = mask_adjacency(ei, n)
    masks = torch.zeros(M, n, dtype=torch.int64, device=dev)
    sizes, counts = torch.zeros(M, 1, it, dtype=torch.int64), torch.zeros(M, 1, it, dtype=torch.int64)
    batches, masked_out = torch.zeros(M, 1, dtype=torch.int64), torch.zeros(M, 1, dtype=torch.int64)
    capped, exhausted = torch.zeros(M, 1, dtype=torch.bool), torch.zeros(M, 1, dtype=torch.bool)
    centres = []
    for m in range(M):
        stream = _surface_centres(v, f, cum, state, cand, surface_stream_seed(seed, m), spacing)
        pos, total, k, masked, done, per_batch = 0, 0, 10, 0, False, []
        for b in range(it):
            take = stream[pos:pos + k]
            got = int(take.numel())
            if got:
                _, mk, info, _ = _circle_dist(adj, n, radius, 0.0, 1, 0, None, 1, centres=take, want_mask=True)
                torch.maximum(masks[m], mk[0], out=masks[m])
                masked = int((masks[m] > 0).sum())
                if int(info[-1]) != 0:
                    raise RuntimeError('circle_masks_on_surface: the overflow drain did not finish (status %d)' % int(info[-1]))
            pos, total = pos + got, total + got
            per_batch.append(take)
            sizes[m, 0, b], counts[m, 0, b], batches[m, 0] = got, masked, b + 1
            if got < k:
                exhausted[m, 0] = done = True
                break
            cur = masked / n
            if cur >= frac:
                done = True
                break
            k = min(int(total * (frac / cur - 1)), n)
            if k <= 0:
                done = True
                break
        capped[m, 0] = not done
        masked_out[m, 0] = masked
        centres.append([per_batch])
    if not return_centres:
        return masks
    return masks, dict(centres=centres, sizes=sizes, counts=counts, batches=batches, masked=masked_out, capped=capped,
                       exhausted=exhausted, candidates=cand)


# -------------------------------------------------------------------------------------------------------- geodesic circle masks
GEODESIC_LEVELS = 4                  # LDS levels a workgroup follows inside one round (changes rounds and work, never the result)
_GEODESIC_GROUP = 16                 # rounds per host read of geodesic_distance (max_rounds=None)
_GEODESIC_CALL = 4096                # rounds per stin_geodesic_rounds_f64 call (its upper bound)


def _geodesic_edges(n, dev, edge_index, faces, what):
    if edge_index is not None:
        return edge_index.to(dev)
    if faces is None:
        raise ValueError('%s: give edge_index, faces or adjacency' % what)
    if not (torch.is_tensor(faces) and faces.is_cuda):
        raise TypeError('faces must be a CUDA tensor (no CPU fallback exists)')
    return edges_from_faces(_checked_faces(faces, n, what), n)


def geodesic_adjacency(vertices, edge_index=None, faces=None, check=True):
    """The weighted CSR of the geodesic pass: ``mask_adjacency``'s (rowptr [N + 1], col [2E]) as it is, plus length float64 [2E],
    the Euclidean length of every slot's edge in fp64: sqrt((dx dx + dy dy) + dz dz), symmetric bit for bit
    (``stin_geodesic_lengths_f64``).  vertices [N, >= 3] float (float32 is promoted first); the edges are edge_index [2, E] taken as
    undirected, or the sides of `faces`.  check=True reads one status word: ValueError for a length that is not finite (a
    non-finite vertex of an edge), IndexError for an endpoint outside [0, N).  Unchecked, such an edge is simply never walked."""
    v = _xyz64(vertices, 'vertices')
    lib = _lib.load()
    n, dev = int(v.shape[0]), v.device
    ei = _geodesic_edges(n, dev, edge_index, faces, 'geodesic_adjacency')
    rowptr, col = mask_adjacency(ei, n, check=check)
    e2 = 2 * int(ei.shape[1])
    col = col[:e2]
    length = torch.empty(max(e2, 1), dtype=torch.float64, device=dev)[:e2]
    flags = torch.empty(1, dtype=torch.int64, device=dev)
    _lib.check(lib.stin_geodesic_lengths_f64(_ptr(v), n, _ptr(rowptr), _ptr(col), e2, _ptr(length), _ptr(flags), _stream(v)),
               'stin_geodesic_lengths_f64')
    if check:
        fl = int(flags.item())
        if fl & 2:
            raise IndexError('geodesic_adjacency: an edge refers to a vertex outside [0, %d)' % n)
        if fl & 1:
            raise ValueError('geodesic_adjacency: the length of an edge is not finite (a non-finite vertex)')
    return rowptr, col, length


def _geodesic_adjacency_arg(adjacency, n, what):
    rowptr, col, length = adjacency
    if not (rowptr.is_cuda and rowptr.dtype == torch.int32 and col.dtype == torch.int32 and length.dtype == torch.float64):
        raise TypeError('%s: adjacency must be what geodesic_adjacency returns (int32, int32, float64 on the GPU)' % what)
    if int(rowptr.numel()) != n + 1 or int(col.numel()) != int(length.numel()):
        raise ValueError('%s: adjacency does not belong to %d vertices' % (what, n))
    return rowptr.contiguous(), col.contiguous(), length.contiguous()


def _geodesic_run(adj, n, sources, inst, M, cap, max_rounds, levels, what):
    """-> (dist float64 [M, n], state int64 [4] on the device, rounds launched).  max_rounds=None: until the worklist is empty."""
    lib = _lib.load()
    rowptr, col, length = adj
    dev = rowptr.device
    e2 = int(col.numel())
    if M * max(n, 1) >= (1 << 31) - 1:
        raise ValueError('%s: num_instances * N must stay below 2^31' % what)
    dist = torch.empty(M, max(n, 1), dtype=torch.float64, device=dev)[:, :n]
    state = torch.zeros(4, dtype=torch.int64, device=dev)
    ws_bytes = lib.stin_geodesic_workspace_bytes(n, M)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    S = int(sources.numel())
    _lib.check(lib.stin_geodesic_begin_f64(_ptr(sources) if S else None, _ptr(inst) if inst is not None and S else None, S, n, M,
                                           _ptr(dist) if n else None, _ptr(state), _ptr(ws), ws_bytes, _stream(rowptr)),
               'stin_geodesic_begin_f64')
    launched = 0

    def rounds(k):
        nonlocal launched
        while k > 0:
            step = min(k, _GEODESIC_CALL)
            _lib.check(lib.stin_geodesic_rounds_f64(_ptr(rowptr), _ptr(col), _ptr(length), n, e2, M, cap, _ptr(dist) if n else None,
                                                    launched, step, int(levels), _ptr(state), _ptr(ws), ws_bytes, _stream(rowptr)),
                       'stin_geodesic_rounds_f64')
            launched, k = launched + step, k - step

    if max_rounds is not None:
        rounds(int(max_rounds))
        return dist, state, launched
    while True:
        st = state.tolist()
        if st[0] & 2:
            raise IndexError('%s: a source lies outside [0, %d) or its instance outside [0, %d)' % (what, n, M))
        if st[1] == 0:
            return dist, state, launched
        if launched >= n + _GEODESIC_GROUP:                                 # (a shortest path has fewer than N edges)
            raise RuntimeError('%s: %d vertices still listed after %d rounds' % (what, st[1], launched))
        rounds(_GEODESIC_GROUP)


def _geodesic_sources(sources, source_instance, num_instances, n, dev, what):
    s = torch.as_tensor(sources, dtype=torch.int64).reshape(-1).to(dev).contiguous()
    M = int(num_instances)
    if M < 1:
        raise ValueError('%s: num_instances must be >= 1' % what)
    inst = None
    if source_instance is not None:
        inst = torch.as_tensor(source_instance).reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
        if inst.numel() != s.numel():
            raise ValueError('%s: one instance per source' % what)
    return s, inst, M


def geodesic_distance(vertices, sources, edge_index=None, faces=None, max_distance=None, source_instance=None, num_instances=1,
                      adjacency=None, max_rounds=None, levels=None, return_info=False):
    """Distances along the mesh EDGES, weighted by their Euclidean length in the units of the vertices, to the nearest of `sources`:
    float64 [N] (CUDA), or [num_instances, N] when `source_instance` (one int per source) spreads the sources over several
    independent instances that run in the same launches.  The Dijkstra metric of the edge graph - NOT the exact polyhedral geodesic,
    which crosses faces - cut off at max_distance: D[v] where D[v] < max_distance (strict), +inf elsewhere and for unreachable
    vertices (None: no cut-off).  D is the minimum over all edge paths of the length folded from the source outward in fp64, the
    same bytes on every schedule and equal to heap Dijkstra's (include/stin_hip.h, "Geodesic distances"; csrc/stin_geodesic.hip:
    frontier rounds, 64-bit integer atomicMin on the bit patterns).  Edges: edge_index, the sides of `faces`, or a ready
    `adjacency` from ``geodesic_adjacency``.  Runs on the GPU only.  IndexError for a source outside [0, N); no sources: all +inf.
    max_rounds=None: rounds are launched %d at a time and one count is read per group until the worklist is empty (RuntimeError
    after N rounds, which no input needs).  max_rounds=k: exactly k round launches and NO host synchronisation; returns
    (dist, status) with status int64 [4] on the device: [0] flags (bit 1: a source out of range, bit 2: not converged), [1]
    vertices still listed, [2] rounds that found work, [3] directed edges relaxed.
    levels: LDS levels per round (default GEODESIC_LEVELS; changes rounds and work, never the result).  return_info=True (with
    max_rounds=None): also a dict with 'rounds', 'launched' and 'relaxed'.""" % _GEODESIC_GROUP
    import math
    what = 'geodesic_distance'
    v = _xyz64(vertices, 'vertices')
    n, dev = int(v.shape[0]), v.device
    cap = math.inf if max_distance is None else float(max_distance)
    if not cap > 0.0:
        raise ValueError('%s: max_distance must be > 0' % what)
    if max_rounds is not None and int(max_rounds) < 1:
        raise ValueError('%s: max_rounds must be >= 1' % what)
    s, inst, M = _geodesic_sources(sources, source_instance, num_instances, n, dev, what)
    adj = (_geodesic_adjacency_arg(adjacency, n, what) if adjacency is not None
           else geodesic_adjacency(v, edge_index=edge_index, faces=faces))
    dist, state, launched = _geodesic_run(adj, n, s, inst, M, cap, max_rounds, levels or GEODESIC_LEVELS, what)
    out = dist if source_instance is not None or M > 1 else dist[0]
    if max_rounds is not None:
        return out, state
    if return_info:
        st = state.tolist()
        return out, dict(rounds=st[2], launched=launched, relaxed=st[3])
    return out


def _geodesic_mask_values(dist, radius, rings):
    lib = _lib.load()
    d = dist.contiguous()
    mask = torch.empty(d.shape, dtype=torch.int64, device=d.device)
    _lib.check(lib.stin_geodesic_mask_f64(_ptr(d) if d.numel() else None, int(d.numel()), float(radius), int(rings),
                                          _ptr(mask) if d.numel() else None, _stream(d)), 'stin_geodesic_mask_f64')
    return mask


def _geodesic_radius(radius, rings, what):
    import math
    r = float(radius)
    if not (r > 0.0 and math.isfinite(r)):
        raise ValueError('%s: radius must be positive and finite' % what)
    if int(rings) < 1:
        raise ValueError('%s: rings must be >= 1' % what)
    return r, int(rings)


def circle_mask_from_centres_geodesic(vertices, centres, radius, rings=16, edge_index=None, faces=None, adjacency=None):
    """``circle_mask_from_centres`` with a metric radius: int64 [N] (CUDA), mask[v] = 0 where the edge-path distance D[v] from the
    nearest centre (``geodesic_distance``, cut off at `radius`) is >= radius, else min(rings, ceil((radius - D[v]) / (radius /
    rings))): a centre gets `rings`, the rim 1.  With rings = 16 the loss weight 0.99^mask spans the range of the hop masks.
    radius is a length in the units of the vertices; the metric is Dijkstra's on the edge graph, not the polyhedral geodesic."""
    what = 'circle_mask_from_centres_geodesic'
    r, rings = _geodesic_radius(radius, rings, what)
    dist = geodesic_distance(vertices, centres, edge_index=edge_index, faces=faces, max_distance=r, adjacency=adjacency)
    return _geodesic_mask_values(dist, r, rings)


def circle_masks_geodesic(vertices, faces, radius, frac_masked_vertices=0.25, num_masks=1, seed=0, rings=16, spacing=None,
                          candidates=None, edge_index=None, max_iters=32, return_centres=False):
    """``circle_masks_on_surface`` with a metric radius: int64 [num_masks, N], ready for ``scene_io.write_circle_masks``.  The same
    centre streams (``surface_centres(candidates, surface_stream_seed(seed, m), spacing)``), the same batch rule (10 centres, then
    k = int(total * (frac / cur - 1)) more until cur >= frac or k <= 0; a short stream ends the mask `exhausted`) and the same info
    dict; the value is ``circle_mask_from_centres_geodesic``'s, so a hole has the same physical size whatever the local
    tessellation and on every hierarchy of a scan.  Batch b of ALL masks still running is ONE distance call (one instance per
    mask); one host read per batch (an offline path).  Distances run on the mesh's own edges, or on `edge_index` when given.
    Dijkstra's metric on the edge graph, not the polyhedral geodesic; the Poisson-disk `spacing` stays Euclidean."""
    what = 'circle_masks_geodesic'
    r, rings = _geodesic_radius(radius, rings, what)
    v, f, cum, state, st = _surface_mesh(vertices, faces, what)
    n, dev, M, it = int(v.shape[0]), v.device, int(num_masks), int(max_iters)
    frac = float(frac_masked_vertices)
    if M < 1 or it < 1:
        raise ValueError('%s: num_masks and max_iters must be >= 1' % what)
    cand = int(candidates) if candidates is not None else default_surface_candidates(_surface_area(st), n, spacing)
    adj = geodesic_adjacency(v, edge_index=edge_index.to(dev) if edge_index is not None else edges_from_faces(f, n))
    masks = torch.zeros(M, n, dtype=torch.int64, device=dev)
    sizes, counts = torch.zeros(M, 1, it, dtype=torch.int64), torch.zeros(M, 1, it, dtype=torch.int64)
    batches, masked_out = torch.zeros(M, 1, dtype=torch.int64), torch.zeros(M, 1, dtype=torch.int64)
    capped, exhausted = torch.ones(M, 1, dtype=torch.bool), torch.zeros(M, 1, dtype=torch.bool)
    streams = [_surface_centres(v, f, cum, state, cand, surface_stream_seed(seed, m), spacing) for m in range(M)]
    centres = [[[]] for _ in range(M)]
    pos, total, k, masked = [0] * M, [0] * M, [10] * M, [0] * M
    running = list(range(M))
    for b in range(it):
        if not running:
            break
        takes = [streams[m][pos[m]:pos[m] + k[m]] for m in running]
        if sum(int(t.numel()) for t in takes):
            inst = torch.cat([torch.full((int(t.numel()),), j, dtype=torch.int32, device=dev) for j, t in enumerate(takes)])
            dist = geodesic_distance(v, torch.cat(takes), max_distance=r, source_instance=inst, num_instances=len(running),
                                     adjacency=adj)
            idx = torch.as_tensor(running, device=dev)
            masks[idx] = torch.maximum(masks[idx], _geodesic_mask_values(dist, r, rings))
            for m, c in zip(running, (masks[idx] > 0).sum(dim=1).tolist()):
                masked[m] = int(c)
        still = []
        for m, take in zip(running, takes):
            got = int(take.numel())
            pos[m], total[m] = pos[m] + got, total[m] + got
            centres[m][0].append(take)
            sizes[m, 0, b], counts[m, 0, b], batches[m, 0] = got, masked[m], b + 1
            if got < k[m]:
                exhausted[m, 0], capped[m, 0] = True, False
                continue
            cur = masked[m] / n
            if cur >= frac:
                capped[m, 0] = False
                continue
            k[m] = min(int(total[m] * (frac / cur - 1)), n)
            if k[m] <= 0:
                capped[m, 0] = False
                continue
            still.append(m)
        running = still
    masked_out[:, 0] = torch.as_tensor(masked)
    if not return_centres:
        return masks
    return masks, dict(centres=centres, sizes=sizes, counts=counts, batches=batches, masked=masked_out, capped=capped,
                       exhausted=exhausted, candidates=cand)


# ----------------------------------------------------------------------------------------------------------------- harmonic fill
_HARMONIC_REACH_GROUP = 16           # reach rounds per host read
_HARMONIC_CALL = 4096                # iterations per stin_harmonic_iterate_f64 call (its upper bound)
_HARMONIC_STATUS = ((1, 'a weight of an edge at a masked vertex is not finite or not positive'),
                    (2, 'a known value next to a masked vertex is not finite'),
                    (4, 'the adjacency refers to a vertex outside [0, N) or its rowptr is malformed'))


def _harmonic_info(state, C):
    """The device table (int64 [STIN_HARMONIC_STATE], on the host) -> a dict."""
    st = [int(v) for v in state]
    ch = [st[8 + 4 * c:12 + 4 * c] for c in range(C)]
    bits = lambda w: float(torch.tensor([w], dtype=torch.int64).view(torch.float64)[0])     # the word holds a double's bits
    return dict(status=st[0], n_unknown=st[1], n_unreached=st[2], n_masked=st[4], iterations=[w[0] for w in ch],
                rr=[bits(w[1]) for w in ch], bb=[bits(w[2]) for w in ch], flags=[w[3] for w in ch],
                converged=all(w[3] & 1 for w in ch), state=st)


def harmonic_adjacency(edge_index, num_nodes, vertices=None):
    """The CSR ``harmonic_fill`` builds when it is given edge_index: ``mask_adjacency``'s (or, with `vertices`,
    ``geodesic_adjacency``'s with its lengths) with the slots of every row put in ascending neighbour id.  ``mask_adjacency`` fills
    its rows with atomics, so its slot order changes from call to call, and the fixed-order sums of the harmonic fill follow the
    slot order: sorted rows make the bytes of the result a function of the graph alone.  (Equal slots - a duplicate edge - carry
    equal lengths, so their order among themselves does not matter.)"""
    n = int(num_nodes)
    if not edge_index.is_cuda:
        raise TypeError('edge_index must be a CUDA tensor (no CPU fallback exists)')
    if vertices is not None:
        rowptr, col, length = geodesic_adjacency(vertices, edge_index=edge_index)
    else:
        rowptr, col = mask_adjacency(edge_index, n)
        col, length = col[:2 * int(edge_index.shape[1])], None
    rows = torch.repeat_interleave(torch.arange(n, device=col.device), (rowptr[1:] - rowptr[:-1]).long())
    order = torch.argsort(rows * max(n, 1) + col.long(), stable=True)
    col = col[order].contiguous()
    return (rowptr, col) if length is None else (rowptr, col, length[order].contiguous())


def harmonic_fill(values, masked, edge_index=None, adjacency=None, vertices=None, weights='uniform', tol=1e-6, max_iterations=None,
                  fill=0.0, iterations_per_sync=16, return_info=False):
    """Harmonic (diffusion, Laplace) inpainting on a graph: every masked vertex becomes the weighted mean of its neighbours, with
    the known vertices as boundary values - the zero of the graph Laplacian on the hole, the minimiser of sum_edges w (x_i - x_j)^2
    - by Jacobi-preconditioned CG in fp64 with every sum in a fixed order: the same bytes on every run and every grouping of the
    launches, equal to the numpy restatement of include/stin_hip.h, "Harmonic fill" (csrc/stin_harmonic.hip).
    values float32 [N, C] (C <= 16, CUDA); masked [N] (non-zero / True = fill it); the graph is edge_index [2, E] taken as
    undirected (``harmonic_adjacency``: rows sorted, so the bytes depend on the graph alone), or a ready `adjacency` from
    ``mask_adjacency`` / ``geodesic_adjacency`` / ``harmonic_adjacency`` (the sums follow its slot order).  weights: 'uniform' (every edge 1.0),
    'inverse_length' (1.0 / length in torch fp64 from ``geodesic_adjacency``: needs `vertices` or an adjacency with lengths; a
    zero-length edge gives inf and is an error) or a float64 tensor [2E] aligned with the adjacency's `col`.
    -> float32 [N, C]: known rows bit for bit, masked rows the solution, masked vertices no path of masked vertices joins to a known
    one (an isolated vertex, an island without a rim) `fill`.  A channel stops when ||r|| <= tol ||b||; max_iterations=None allows
    n_U (the number of unknowns) iterations, launched `iterations_per_sync` at a time with one small host read per group.  An integer
    max_iterations with iterations_per_sync=None launches exactly that many iterations with no host read between them and returns
    (out, status) with the device table int64 [STIN_HARMONIC_STATE] (the reach pass before them still reads one count per group
    of rounds).  return_info=True: (out, dict) with 'iterations', 'rr', 'bb', 'flags' per channel (bit 0 done, bit 1 breakdown, bit 2
    not converged), 'n_unknown', 'n_unreached', 'converged' and 'state' (the whole table).  ValueError for a weight that is not finite or not positive and for a
    non-finite known value on the rim.  Runs on the GPU only.
    A graph Laplacian with uniform or inverse-length weights, not cotangent weights; one global solve, zero start."""
    what = 'harmonic_fill'
    if not (torch.is_tensor(values) and values.is_cuda and torch.is_tensor(masked) and masked.is_cuda):
        raise TypeError('values and masked must be CUDA tensors (no CPU fallback exists)')
    if values.dtype != torch.float32:
        raise TypeError('values must be float32')
    cmax = _lib.CONSTANTS['STIN_HARMONIC_MAX_C']
    if values.dim() != 2 or not 1 <= int(values.shape[1]) <= cmax:
        raise ValueError('values must be [N, C] with 1 <= C <= %d' % cmax)
    n, C, dev = int(values.shape[0]), int(values.shape[1]), values.device
    if int(masked.numel()) != n:
        raise ValueError('masked needs one entry per vertex')
    tol = float(tol)
    if not tol >= 0.0:
        raise ValueError('%s: tol must be >= 0' % what)
    if max_iterations is not None and int(max_iterations) < 0:
        raise ValueError('%s: max_iterations must be >= 0' % what)
    if iterations_per_sync is None and max_iterations is None:
        raise ValueError('%s: iterations_per_sync=None needs an integer max_iterations' % what)
    if iterations_per_sync is not None and int(iterations_per_sync) < 1:
        raise ValueError('%s: iterations_per_sync must be >= 1' % what)
    lib = _lib.load()
    # ---- the graph and its weights
    length = None
    if adjacency is not None:
        adj = tuple(adjacency)
        if not (len(adj) in (2, 3) and adj[0].is_cuda and adj[0].dtype == torch.int32 and adj[1].dtype == torch.int32):
            raise TypeError('%s: adjacency must be what mask_adjacency or geodesic_adjacency returns (int32 on the GPU)' % what)
        rowptr, col = adj[0].contiguous(), adj[1].contiguous()
        length = adj[2] if len(adj) == 3 else None
    else:
        if edge_index is None:
            raise ValueError('%s: give edge_index or adjacency' % what)
        inv_len = isinstance(weights, str) and weights == 'inverse_length'
        if inv_len and vertices is None:
            raise ValueError("%s: weights='inverse_length' needs vertices (or an adjacency from geodesic_adjacency)" % what)
        adj = harmonic_adjacency(edge_index.to(dev), n, vertices=vertices if inv_len else None)
        rowptr, col, length = adj[0], adj[1], (adj[2] if inv_len else None)
    if int(rowptr.numel()) != n + 1:
        raise ValueError('%s: adjacency does not belong to %d vertices' % (what, n))
    e2 = int(col.numel())
    if isinstance(weights, str):
        if weights == 'uniform':
            w = None
        elif weights == 'inverse_length':
            if length is None:
                raise ValueError("%s: weights='inverse_length' needs vertices or an adjacency from geodesic_adjacency" % what)
            w = (1.0 / length.to(device=dev, dtype=torch.float64)).contiguous()
        else:
            raise ValueError("%s: weights must be 'uniform', 'inverse_length' or a float64 tensor" % what)
    else:
        if not (torch.is_tensor(weights) and weights.is_cuda and weights.dtype == torch.float64):
            raise TypeError('%s: weights must be a float64 CUDA tensor' % what)
        w = weights.reshape(-1).contiguous()
    if w is not None and int(w.numel()) != e2:
        raise ValueError('%s: one weight per adjacency slot (%d), got %d' % (what, e2, int(w.numel())))
    vals = values.contiguous()
    m8 = (masked.reshape(-1) != 0).to(torch.uint8).contiguous()
    stream = _stream(vals)
    flag = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    nstate = _lib.CONSTANTS['STIN_HARMONIC_STATE']
    state = torch.zeros(nstate, dtype=torch.int64, device=dev)
    # ---- reached: rounds until one changes nothing (a path of masked vertices has fewer than N of them)
    launched = 0
    while True:
        _lib.check(lib.stin_harmonic_reach_u8(_ptr(rowptr), _ptr(col) if e2 else None, n, e2, _ptr(m8) if n else None, launched,
                                              _HARMONIC_REACH_GROUP, _ptr(flag), _ptr(state), stream), 'stin_harmonic_reach_u8')
        launched += _HARMONIC_REACH_GROUP
        head = state[:5].tolist()
        if head[3] == 0:
            break
        if launched >= n + _HARMONIC_REACH_GROUP:
            raise RuntimeError('%s: the reach pass still changes after %d rounds' % (what, launched))
    n_u = int(head[1])
    ws_bytes = lib.stin_harmonic_workspace_bytes(n, e2, n_u, C)
    if ws_bytes == 0:
        raise ValueError('%s: sizes beyond the int32 CSR' % what)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.stin_harmonic_setup_f64(_ptr(rowptr), _ptr(col) if e2 else None, _ptr(w), n, e2, _ptr(vals) if n else None, C,
                                           _ptr(flag), n_u, _ptr(state), _ptr(ws), ws_bytes, stream), 'stin_harmonic_setup_f64')
    budget = n_u if max_iterations is None else int(max_iterations)
    done = 0

    def iterate(k):
        nonlocal done
        while k > 0:
            step = min(k, _HARMONIC_CALL)
            _lib.check(lib.stin_harmonic_iterate_f64(_ptr(w), n, e2, C, n_u, tol, done, step, _ptr(state), _ptr(ws), ws_bytes,
                                                     stream), 'stin_harmonic_iterate_f64')
            done, k = done + step, k - step

    if iterations_per_sync is None:
        iterate(budget)
    else:
        while done < budget:
            iterate(min(int(iterations_per_sync), budget - done))
            st = state.tolist()
            if st[0] or all(st[8 + 4 * c + 3] & 3 for c in range(C)):
                break
    out = torch.empty(n, C, dtype=torch.float32, device=dev)
    _lib.check(lib.stin_harmonic_finish_f32(_ptr(vals) if n else None, _ptr(flag), n, e2, C, n_u, tol, float(fill),
                                            _ptr(out) if n else None, _ptr(state), _ptr(ws), ws_bytes, stream),
               'stin_harmonic_finish_f32')
    if iterations_per_sync is None:
        return out, state
    st = state.tolist()
    for bit, text in _HARMONIC_STATUS:
        if st[0] & bit:
            raise ValueError('%s: %s' % (what, text))
    return (out, _harmonic_info(st, C)) if return_info else out


def harmonic_inpaint(sample, weights='uniform', **kw):
    """The classic non-learned inpainting baseline: every masked vertex (mask > 0) of a sample gets the harmonic extension of the
    known colours over the sample's own graph (``harmonic_fill``).  sample: anything with `color` [N, C], `mask` [N] or [N, 1] and
    `edge_index` [2, E] - a 3-D training sample, a collated batch (a disjoint union needs nothing special) or an ``imagegraph``
    sample; positions (`pos`, or failing that x[:, 6:9]) are read only for weights='inverse_length'.
    -> the composite float32 [N, C]: `color` itself outside the mask, bit for bit - what StepMetrics.update and
    ImageStepMetrics.update accept as `out` (composite=True and False alike), beside ``knn_inpaint``.  Further keywords go to
    ``harmonic_fill`` (tol, max_iterations, fill, return_info, ...)."""
    color, mask, ei = sample.color, sample.mask, sample.edge_index
    pos = None
    if isinstance(weights, str) and weights == 'inverse_length':
        pos = getattr(sample, 'pos', None)
        pos = sample.x[:, 6:9] if pos is None else pos
    return harmonic_fill(color.float(), mask.reshape(-1) > 0, edge_index=ei, vertices=pos, weights=weights, **kw)
