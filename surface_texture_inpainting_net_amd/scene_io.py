"""Reader for the reference's on-disk scene format -> HierarchicalBatch.

The reference's offline preprocessing (preprocessing/graph_level_generation.py:492-536) writes per scene a
``graphs/<scene>.pt`` dict with
    vertices      list[L]  level 0: [N0, 10] = pos(0:3) rgb in [0,1](3:6) normal(6:9) original-id(9); others [N_l, 3]
    edges         list[L]  int64 [E_l, 2]   (row-wise pairs: source, target)
    traces        list[L]  int64; traces[0] maps to the ORIGINAL mesh, traces[l] (l >= 1): level l-1 -> level l
    dilated_edges list[L]  None or list over dilation_dists of int64 [E_d, 2]  (dilated node, centre)
    dilation_dists list[int]
and per mask a ``masks/<mask_name>/<scene>/<id>.npz`` with ``vertex_mask`` (0 = known, > 0 = inpaint, the value
being the distance to the nearest known vertex).  ``load_scene`` assembles exactly the sample that
datasets/scannetcolorgraph_dataloader.py:83-156 hands to the model (same feature layout, same key names, same
fall-back to the previous dilation distance when one is empty), plus the CoordsNormalization transform
(transform/coords_normalization.py:16: x[:, 6:9] /= max_sizes).  Everything stays on the CPU (worker side);
``sample.to(device)`` and the GPU plan build happen in the training process.

The semantic-segmentation experiment reads LABEL-graph files of the same schema plus ``labels`` (int64, one per vertex of
level 0 for a training crop, one per ORIGINAL mesh vertex for an evaluation scene) and without masks:
``load_label_scene`` / ``label_sample_from_tensors`` restate datasets/scannetlabelgraph_dataloader.py:62-101.
"""
import numpy as np
import torch

from .data import HierarchicalBatch


def sample_from_tensors(saved, vertex_mask, end_level, cropped=False, coords_max_sizes=(1.5, 1.5, 1.5), name=None):
    """saved: the dict of a graphs/<scene>.pt file (or a crop of preprocessing.crop_scene); vertex_mask: int array or tensor [N0].
    The tensors may live on any device (all on the same one): the sample comes out there."""
    coords = [v.clone() if torch.is_tensor(v) else torch.as_tensor(v) for v in saved['vertices'][:end_level]]
    coords[0][:, 3:6] = coords[0][:, 3:6] * 2.0 - 1.0                       # colour to [-1, 1] (:95)
    edges = saved['edges'][:end_level]
    dil = saved.get('dilated_edges')
    dists = saved.get('dilation_dists')
    if dil is not None and dists is not None:
        dil = dil[:end_level]
    else:
        dil, dists = None, None
    dev = coords[0].device
    if torch.is_tensor(vertex_mask):
        mask = vertex_mask.to(dev).unsqueeze(1)
    else:
        mask = torch.as_tensor(np.asarray(vertex_mask)).to(dev).unsqueeze(1)
    known = (mask == 0)
    x = torch.cat([coords[0][:, 3:6] * known, coords[0][:, 6:9], coords[0][:, :3], known], dim=-1).float()   # (:115)
    s = HierarchicalBatch(x=x, color=coords[0][:, 3:6].float(), mask=mask.long(),
                          edge_index=torch.as_tensor(edges[0]).t().contiguous().long())
    if name is not None:
        s['name'] = name
    # full scenes carry the trace back to the original mesh at position 0, crops do not (:124-128)
    traces = saved['traces'][:end_level - 1] if cropped else saved['traces'][1:end_level]
    nv = [int(coords[0].shape[0])]
    for lvl in range(1, len(edges)):
        s['hierarchy_edge_index_%d' % lvl] = torch.as_tensor(edges[lvl]).t().contiguous().long()
        if dil is not None and dil[lvl] is not None:
            for i, d in enumerate(dists):
                cur = dil[lvl][i]
                if len(cur) > 0:
                    s['hierarchy_dil_%s_edge_index_%d' % (d, lvl)] = torch.as_tensor(cur).t().contiguous().long()
                elif i > 0:                                                  # empty set: reuse the previous distance (:143-145)
                    s['hierarchy_dil_%s_edge_index_%d' % (d, lvl)] = torch.as_tensor(dil[lvl][i - 1]).t().contiguous().long()
        tr = torch.as_tensor(traces[lvl - 1]).long()
        s['hierarchy_trace_index_%d' % lvl] = tr
        nv.append(int(tr.max()) + 1)
    s['num_vertices'] = torch.tensor([nv], dtype=torch.int32, device=dev)
    s['batch'] = torch.zeros(nv[0], dtype=torch.long, device=dev)
    if coords_max_sizes is not None:                                         # CoordsNormalization on the position channels
        s['x'][:, 6:9] = s['x'][:, 6:9] / torch.tensor(coords_max_sizes, dtype=s['x'].dtype, device=dev)
    return s


def load_scene(graph_path, mask_path, end_level=3, cropped=False, coords_max_sizes=(1.5, 1.5, 1.5), locality_order=False):
    """graphs/<scene>.pt + masks/<name>/<scene>/<id>.npz -> HierarchicalBatch (CPU).
    locality_order=True (not in the reference): renumber the vertices of every level so that memory order follows space
    (synthetic.renumber_by_locality: Morton order of the positions at level 0, first-child order above; edge lists and traces
    keep their order, index values are relabelled) - the GPU kernels' neighbour gathers then hit L2 instead of crossing the
    fabric (3-4 % of a training step at 200 k vertices).  The sample carries `vertex_order` (new row -> row of the scene file)
    so per-vertex outputs can be mapped back: out_file_order[sample.vertex_order] = out."""
    saved = torch.load(graph_path, map_location='cpu', weights_only=False)
    with open(mask_path, 'rb') as f:
        vertex_mask = np.load(f, allow_pickle=True)['vertex_mask']
    name = str(graph_path).rsplit('/', 1)[-1].rsplit('.', 1)[0]
    sample = sample_from_tensors(saved, vertex_mask, end_level, cropped, coords_max_sizes, name)
    if locality_order:
        from .synthetic import renumber_by_locality
        sample, order = renumber_by_locality(sample)
        sample['vertex_order'] = order
    return sample


def label_sample_from_tensors(saved, end_level=4, is_train=True, name=None, with_labels=True):
    """The semantic-segmentation sample (datasets/scannetlabelgraph_dataloader.py:62-101, ScanNetLabelDataSet.__getitem__)
    from the dict of a label-graph file: x = [colour, normal, position] = [vertices[0][:, 3:9], vertices[0][:, :3]]
    (9 channels, no normalisation - the experiment's transform lists are empty), per-vertex `labels` (int64 [N0]; left out
    with with_labels=False, the reference's benchmark mode), and the two trace conventions: a training crop (is_train) takes
    traces[:end_level - 1] as the hierarchy; an evaluation scene keeps traces[0] (level-0 vertex of every ORIGINAL mesh
    vertex) as `original_index_traces` and takes traces[1:end_level]."""
    coords = [torch.as_tensor(v) for v in saved['vertices'][:end_level]]
    edges = saved['edges'][:end_level]
    x = torch.cat([coords[0][:, 3:9], coords[0][:, :3]], dim=-1).float()
    s = HierarchicalBatch(x=x, edge_index=torch.as_tensor(edges[0]).t().contiguous().long())
    if with_labels:
        s['labels'] = torch.as_tensor(saved['labels']).long()
    if name is not None:
        s['name'] = name
    if is_train:
        traces = saved['traces'][:end_level - 1]
    else:
        s['original_index_traces'] = torch.as_tensor(saved['traces'][0]).long()
        traces = saved['traces'][1:end_level]
    nv = [int(coords[0].shape[0])]
    for lvl in range(1, len(edges)):
        s['hierarchy_edge_index_%d' % lvl] = torch.as_tensor(edges[lvl]).t().contiguous().long()
        tr = torch.as_tensor(traces[lvl - 1]).long()
        s['hierarchy_trace_index_%d' % lvl] = tr
        nv.append(int(tr.max()) + 1)
    s['num_vertices'] = torch.tensor([nv], dtype=torch.int32)
    s['batch'] = torch.zeros(nv[0], dtype=torch.long)
    return s


def load_label_scene(graph_path, end_level=4, is_train=True, with_labels=True):
    """A label-graph file of the segmentation experiment (training crop: is_train=True; full evaluation scene with the
    trace to the original mesh: is_train=False) -> HierarchicalBatch (CPU).  Items of loader.SceneLoader as
    `functools.partial(load_label_scene, path, 4, False)`."""
    saved = torch.load(graph_path, map_location='cpu', weights_only=False)
    name = str(graph_path).rsplit('/', 1)[-1]                                 # the reference keeps the file name (:64-66)
    return label_sample_from_tensors(saved, end_level, is_train, name, with_labels)


def label_graph_tensors(sample, labels, original_index_traces=None):
    """A single-graph HierarchicalBatch (synthetic.make_synthetic_mesh layout) + per-vertex labels -> the dict of a label-graph
    file (test / synthetic-data helper): vertices[0] = [pos, rgb, normal, id] [N0, 10], coarser levels [N_l, 3], edges [E_l, 2],
    traces = [original_index_traces] + level traces for an evaluation scene (labels then belong to the ORIGINAL mesh's
    vertices), the level traces alone for a training crop."""
    L = int(sample.num_vertices.shape[-1])
    x = sample.x
    n0 = x.shape[0]
    v0 = torch.zeros(n0, 10)
    v0[:, 0:3] = x[:, 6:9] * 1.5
    v0[:, 3:6] = (sample.color + 1.0) / 2.0
    v0[:, 6:9] = x[:, 3:6]
    v0[:, 9] = torch.arange(n0)
    vertices, edges, traces = [v0], [sample.edge_index.t().contiguous()], []
    if original_index_traces is not None:
        traces.append(torch.as_tensor(original_index_traces).long())
    for lvl in range(1, L):
        vertices.append(torch.zeros(int(sample.num_vertices.reshape(-1)[lvl]), 3))
        edges.append(sample['hierarchy_edge_index_%d' % lvl].t().contiguous())
        traces.append(sample['hierarchy_trace_index_%d' % lvl])
    return {'vertices': vertices, 'edges': edges, 'traces': traces, 'labels': torch.as_tensor(labels).long()}


def save_scene_like_reference(sample, graph_path, mask_path, dilation_dists=(2, 4, 8, 16)):
    """Write a single-graph HierarchicalBatch in the reference's on-disk schema (test / synthetic-data helper;
    the inverse of load_scene up to the normalisations)."""
    L = int(sample.num_vertices.shape[-1])
    x = sample.x
    n0 = x.shape[0]
    v0 = torch.zeros(n0, 10)
    v0[:, 0:3] = x[:, 6:9] * 1.5
    v0[:, 3:6] = (sample.color + 1.0) / 2.0
    v0[:, 6:9] = x[:, 3:6]
    v0[:, 9] = torch.arange(n0)
    vertices, edges, traces, dilated = [v0], [sample.edge_index.t().contiguous()], [torch.arange(n0)], [None]
    for lvl in range(1, L):
        n = int(sample.num_vertices.reshape(-1)[lvl])
        vertices.append(torch.zeros(n, 3))
        edges.append(sample['hierarchy_edge_index_%d' % lvl].t().contiguous())
        traces.append(sample['hierarchy_trace_index_%d' % lvl])
        sets = []
        for d in dilation_dists:
            k = 'hierarchy_dil_%s_edge_index_%d' % (d, lvl)
            sets.append(sample[k].t().contiguous() if k in sample else [])
        dilated.append(sets if any(len(z) > 0 for z in sets) else None)
    torch.save({'vertices': vertices, 'edges': edges, 'traces': traces, 'dilated_edges': dilated,
                'dilation_dists': list(dilation_dists)}, graph_path)
    np.savez(mask_path, vertex_mask=sample.mask.reshape(-1).numpy())


MIN_FRAC_MASKED_VERTS = 0.02            # preprocessing/observed_texture_map_generation.py:54


def write_circle_masks(graph_path, masks_dir, masks):
    """approve_and_write_out_mask (preprocessing/observed_texture_map_generation.py:616-652) for one graph file: every full-mesh
    mask (masks: [num_masks, N_orig] int, e.g. preprocessing.circle_masks on the original mesh) is gathered to the file's level 0
    by round(vertices[0][:, -1]), rejected when less than MIN_FRAC_MASKED_VERTS of those vertices are masked, else written as
    masks_dir/'{:06d}.npz' (key vertex_mask) numbered by mask index - rejected masks leave gaps.  -> the paths written.
    load_scene(graph_path, path) reads each back unchanged.  It serves both mask types of generate_masks.sh: `circles`
    (preprocessing.circle_masks) and `observers` (preprocessing.observer_masks)."""
    import os
    saved = torch.load(graph_path, map_location='cpu', weights_only=False)
    v0 = saved['vertices'][0]
    v0 = v0.numpy() if torch.is_tensor(v0) else np.asarray(v0)
    vertex_indices = np.round(v0[:, -1]).astype(int)
    if torch.is_tensor(masks):
        masks = masks.detach().cpu().numpy()
    written = []
    for mask_num, vertex_mask in enumerate(masks):
        out = np.asarray(vertex_mask)[vertex_indices]
        counts = np.bincount((out == 0).astype(int))
        if counts.size == 0 or counts[0] / counts.sum() < MIN_FRAC_MASKED_VERTS:
            continue
        os.makedirs(masks_dir, exist_ok=True)
        path = os.path.join(masks_dir, '{:06d}.npz'.format(mask_num))
        with open(path, 'wb') as f:
            np.savez_compressed(f, vertex_mask=out)
        written.append(path)
    return written


def write_crops(graph_path, out_dir, block_size=3.0, stride=1.5, **kw):
    """preprocessing/crop_training_samples.py for one graph file, on the GPU (preprocessing.crop_scene: all crops of the sampling
    grid in one batched pass): writes out_dir/<scene>_<counter>.pt with CPU tensors, named by the reference's counters.  **kw goes
    to crop_scene (positions, min_coarsest, reference_dilated_labels) except device= (default 'cuda').  With
    reference_dilated_labels=True torch.load of each file equals what the reference's script writes for that scene (keys, dtypes,
    shapes, values); the default writes the dilated sets with the level's own ids (see crop_scene).  load_scene(path, mask,
    cropped=True), load_label_scene(path, is_train=True) and write_circle_masks(path, ...) read the files.  -> the paths written."""
    import os
    from .preprocessing import crop_scene

    def to(v, d):
        if torch.is_tensor(v):
            return v.to(d)
        if isinstance(v, (list, tuple)) and any(torch.is_tensor(y) or isinstance(y, (list, tuple)) for y in v):
            return [to(y, d) for y in v]
        return v

    saved = torch.load(graph_path, map_location='cpu', weights_only=False)
    name = os.path.basename(str(graph_path)).rsplit('.', 1)[0]
    device = kw.pop('device', 'cuda')
    crops = crop_scene({k: to(v, device) for k, v in saved.items()}, block_size, stride, **kw)
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for counter, crop in crops:
        path = os.path.join(out_dir, '%s_%d.pt' % (name, counter))
        torch.save({k: to(v, 'cpu') for k, v in crop.items()}, path)       # (.to('cpu') of a view copies only the view)
        written.append(path)
    return written


def write_graph_levels(out_dir, scene_name, mesh, levels, dilated_levels, dilation_dists, labels=None, device='cuda', **kw):
    """preprocessing/graph_level_generation.py for one scene, on the GPU (preprocessing.graph_levels: the arguments are its own;
    tensors or arrays of `mesh`, the level dicts and `labels` are moved to `device`): writes out_dir/<scene_name>.pt with CPU
    tensors in the reference's schema - the file load_scene, load_label_scene(is_train=False), write_crops and write_circle_masks
    read.  **kw goes to graph_levels (reference_vc_normals).  -> the path written."""
    import os
    from .preprocessing import graph_levels

    def to(v, d):
        if torch.is_tensor(v):
            return v.to(d)
        if isinstance(v, np.ndarray):
            return torch.from_numpy(v).to(d)
        if isinstance(v, (list, tuple)) and any(torch.is_tensor(y) or isinstance(y, (list, tuple)) for y in v):
            return [to(y, d) for y in v]
        return v

    def level(x):
        return {k: (v if k == 'csv' else to(v, device)) for k, v in x.items()} if isinstance(x, dict) else x

    saved = graph_levels({k: to(v, device) for k, v in mesh.items()}, [level(x) for x in levels], dilated_levels, dilation_dists,
                         labels=None if labels is None else to(labels, device), **kw)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, '%s.pt' % scene_name)
    torch.save({k: to(v, 'cpu') for k, v in saved.items()}, path)
    return path


# ------------------------------------------------------------------------------------------------------------- observer masks
def load_camera_poses(path, max_num_poses=None, cpp_sens_reader=True):
    """The camera-to-world matrices of a scan as the reference's load_camera_poses (observed_texture_map_generation.py:57-79) finds
    them: `*.pose.txt` (the C++ SensReader's export; `*.txt` for the python one) of directory `path`, sorted by name, the first
    max_num_poses of them -> float64 [P, 4, 4] numpy (pose id = position).  The files are returned as they are: the inverse and the
    validity rule (ScanNet writes -inf for lost tracking) are preprocessing.pose_extrinsics'."""
    import glob
    import os
    names = sorted(glob.glob(os.path.join(path, '*.pose.txt' if cpp_sens_reader else '*.txt')))
    if max_num_poses is not None:
        names = names[:int(max_num_poses)]
    poses = np.zeros((len(names), 4, 4), dtype=np.float64)
    for i, name in enumerate(names):
        poses[i] = np.loadtxt(name, dtype=np.float64).reshape(4, 4)
    return poses


def load_scan_config(path, scan_name, cpp_sens_reader=True):
    """The reference's load_scan_config (:82-114) -> {'colorheight': int, 'colorwidth': int, 'colorintrinsic': float64 [4, 4]}.
    cpp_sens_reader: path/_info.txt with m_colorWidth, m_colorHeight and the 16 numbers of m_calibrationColorIntrinsic; else
    path/<scan_name>.txt with colorWidth, colorHeight, and the matrix from path/intrinsic_color.txt.  `key = value` lines, keys
    compared without case (as configparser does for the reference); fx, fy of observe_vertices are entries [0, 0] and [1, 1]."""
    import os
    config = {}
    with open(os.path.join(path, '_info.txt' if cpp_sens_reader else '%s.txt' % scan_name), 'r') as f:
        for line in f:
            key, sep, value = line.partition('=')
            if sep:
                config[key.strip().lower()] = value.strip()
    prefix = 'm_' if cpp_sens_reader else ''
    if cpp_sens_reader:
        intrinsic = np.array([float(v) for v in config['m_calibrationcolorintrinsic'].split()], dtype=np.float64).reshape(4, 4)
    else:
        intrinsic = np.loadtxt(os.path.join(path, 'intrinsic_color.txt'), dtype=np.float64).reshape(4, 4)
    return {'colorheight': int(config[prefix + 'colorheight']), 'colorwidth': int(config[prefix + 'colorwidth']),
            'colorintrinsic': intrinsic}


# --------------------------------------------------------------------------------------------------------------- scan frames
def _natural_key(name):
    """Runs of digits compare as numbers, everything between them as text; the leading text run (possibly empty) keeps the two
    kinds at the same positions of every key."""
    import re
    parts = re.findall(r'\d+|\D+', name)
    if parts and parts[0][0].isdigit():
        parts.insert(0, '')
    return [int(p) if p[0:1].isdigit() else p for p in parts]


def scan_frame_files(scan_dir):
    """The frame files of an exported scan -> {'color': [...], 'depth': [...], 'pose': [...]}: color/*.jpg, depth/*.png and
    pose/*.txt of scan_dir as full paths, each list in natural (alphanumeric) order - 2.jpg before 10.jpg - which is what the
    reference's sorted_alphanum gives its colour and depth lists (texture_map_optimization.py:52-76).  The reference sorts its pose
    files lexicographically (:101-102), which pairs them with the wrong frames once the ids are not zero-padded; here all three lists
    are in natural order, so that entry i of each belongs to frame i."""
    import os
    out = {}
    for kind, ext in (('color', '.jpg'), ('depth', '.png'), ('pose', '.txt')):
        folder = os.path.join(str(scan_dir), kind)
        names = [f for f in os.listdir(folder) if os.path.isfile(os.path.join(folder, f)) and os.path.splitext(f)[1] == ext]
        out[kind] = [os.path.join(folder, f) for f in sorted(names, key=_natural_key)]
    return out


def read_frames(color_files, depth_files):
    """Decoded frames of a scan -> (color uint8 [B, Hc, Wc, 3] RGB, depth uint16 [B, Hd, Wd]) numpy arrays, with depth == 65535 set
    to 0 as the reference does (texture_map_optimization.py:86-92); every colour file must have one size and every depth file one
    size.  What preprocessing.resize_u8 and FrameColors.add take after torch.from_numpy(...).to(device).  Decoding is Pillow's,
    imported here and only here: the package does not depend on it, and a missing Pillow is an ImportError that says so."""
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError('read_frames decodes JPEG and PNG files with Pillow (PIL), which is not installed') from e
    colors, depths = [], []
    for name in color_files:
        with Image.open(name) as im:
            colors.append(np.asarray(im.convert('RGB'), dtype=np.uint8))
    for name in depth_files:
        with Image.open(name) as im:
            d = np.asarray(im)
        if d.ndim != 2 or d.min(initial=0) < 0 or d.max(initial=0) > 65535:
            raise ValueError('%s is not a 16-bit single-channel depth image' % name)
        d = d.astype(np.uint16)
        d[d == 65535] = 0
        depths.append(d)
    for what, frames in (('colour', colors), ('depth', depths)):
        if len({f.shape for f in frames}) > 1:
            raise ValueError('%s frames of different sizes' % what)
    color = np.stack(colors) if colors else np.zeros((0, 0, 0, 3), dtype=np.uint8)
    depth = np.stack(depths) if depths else np.zeros((0, 0, 0), dtype=np.uint16)
    return color, depth


def write_observers(path, bits, valid_pose_ids, num_poses):
    """The per-scene cache the reference keeps under observers_per_vert/<scene>.npz (:489-507), as plain arrays instead of a pickled
    dict of lists: bits (uint32 [N, words], preprocessing.observe_vertices), valid_pose_ids (int64), num_poses.  -> path."""
    import os
    b = bits.detach().cpu().numpy() if torch.is_tensor(bits) else np.asarray(bits)
    if os.path.dirname(str(path)):
        os.makedirs(os.path.dirname(str(path)), exist_ok=True)
    with open(path, 'wb') as f:
        np.savez_compressed(f, bits=np.ascontiguousarray(b, dtype=np.uint32), valid_pose_ids=np.asarray(valid_pose_ids, dtype=np.int64),
                            num_poses=np.asarray(int(num_poses), dtype=np.int64))
    return path


def read_observers(path, device=None):
    """-> (bits uint32 [N, words], valid_pose_ids int64 numpy, num_poses int) of a write_observers file, read without pickle.  bits is
    a numpy array, or a tensor on `device` when one is given (what preprocessing.observer_masks takes)."""
    with open(path, 'rb') as f:
        data = np.load(f, allow_pickle=False)
        bits, ids, num_poses = data['bits'], data['valid_pose_ids'], int(data['num_poses'])
    if device is not None:
        bits = torch.from_numpy(bits).to(device)
    return bits, ids, num_poses


# ---------------------------------------------------------------------------------------------------------------- mesh files
# PLY (the Stanford polygon format): a text header that names the elements, their counts and their properties in file order, then
# the body - ascii numbers, or fixed-stride binary records in either byte order.  read_ply returns the `mesh` dict every
# preprocessing entry point starts from (graph_levels, decimate_qem, cluster_mesh, observe_vertices, FrameColors, sample_surface,
# circle_masks_geodesic, views.render_mesh): what the reference gets from open3d.io.read_triangle_mesh and PlyData.read.  A
# contract of the project's own (include/stin_hip.h, "Mesh files"), restated with numpy structured dtypes by the test suite and
# NOT pinned against open3d or plyfile themselves: neither is installed here.
PLY_SCALARS = ('int8', 'uint8', 'int16', 'uint16', 'int32', 'uint32', 'float32', 'float64')      # position = STIN_PLY_* code
PLY_TYPE_NAMES = dict({t: t for t in PLY_SCALARS}, char='int8', uchar='uint8', short='int16', ushort='uint16', int='int32',
                      uint='uint32', float='float32', double='float64')
PLY_FORMATS = ('ascii', 'binary_little_endian', 'binary_big_endian')
PLY_MAX_HEADER_BYTES = 1 << 20
_PLY_WIDTH = dict(zip(PLY_SCALARS, (1, 1, 2, 2, 4, 4, 4, 8)))
_PLY_COUNT = dict(zip(PLY_SCALARS, 'i1 u1 i2 u2 i4 u4 f4 f8'.split()))


def read_ply_header(path_or_bytes):
    """The header of a PLY file (a path, or the bytes of the file or of its beginning) ->
        {'format': 'ascii' | 'binary_little_endian' | 'binary_big_endian', 'version': str, 'comments': [str], 'obj_info': [str],
         'elements': [{'name': str, 'count': int, 'properties': [{'name': str, 'type': str, 'count_type': str or None}]}],
         'body_offset': int}
    with elements and properties in file order.  Types are the eight canonical names of PLY_SCALARS - the aliases char, uchar,
    short, ushort, int, uint, float, double and int8 .. float64 are both read; a list property has the type of its entries as
    'type' and the type of its count as 'count_type'.  body_offset is the byte after the end_header line.  Standard library only.
    ValueError with the offending line for a malformed header, an unknown type name, or a missing end_header."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        data = bytes(path_or_bytes[:PLY_MAX_HEADER_BYTES])
    else:
        data = b''
        with open(path_or_bytes, 'rb') as f:
            while b'end_header' not in data and len(data) < PLY_MAX_HEADER_BYTES:
                chunk = f.read(1 << 16)
                if not chunk:
                    break
                data += chunk
            if b'end_header' in data:
                data += f.readline()                                    # the rest of the end_header line, if a chunk cut it

    def bad(number, text, why):
        return ValueError('PLY header line %d: %r: %s' % (number, text, why))

    header = {'format': None, 'version': None, 'comments': [], 'obj_info': [], 'elements': [], 'body_offset': None}
    pos, number = 0, 0
    while True:
        end = data.find(b'\n', pos)
        if end < 0:
            raise ValueError('PLY header: no end_header line in the first %d bytes' % len(data))
        text = data[pos:end].rstrip(b'\r').decode('latin-1')
        pos, number = end + 1, number + 1
        words = text.split()
        if number == 1:
            if text.strip() != 'ply':
                raise bad(number, text, "the first line must be 'ply'")
            continue
        if not words:
            continue
        key = words[0]
        if key == 'end_header':
            break
        if key == 'comment' or key == 'obj_info':
            header['comments' if key == 'comment' else 'obj_info'].append(text.strip()[len(key):].strip())
        elif key == 'format':
            if len(words) != 3 or words[1] not in PLY_FORMATS or header['format'] is not None:
                raise bad(number, text, 'expected one line `format <%s> <version>`' % ' | '.join(PLY_FORMATS))
            header['format'], header['version'] = words[1], words[2]
        elif key == 'element':
            if len(words) != 3 or not words[2].isdigit():
                raise bad(number, text, 'expected `element <name> <count>`')
            if any(e['name'] == words[1] for e in header['elements']):
                raise bad(number, text, 'second element of that name')
            header['elements'].append({'name': words[1], 'count': int(words[2]), 'properties': []})
        elif key == 'property':
            if not header['elements']:
                raise bad(number, text, 'a property before the first element')
            is_list = len(words) > 1 and words[1] == 'list'
            if len(words) != (5 if is_list else 3):
                raise bad(number, text, 'expected `property <type> <name>` or `property list <count type> <type> <name>`')
            for t in words[1 + is_list:-1]:
                if t not in PLY_TYPE_NAMES:
                    raise bad(number, text, 'unknown type %r' % t)
            count_type = PLY_TYPE_NAMES[words[2]] if is_list else None
            if is_list and count_type in ('float32', 'float64'):
                raise bad(number, text, 'the count of a list must be an integer type')
            props = header['elements'][-1]['properties']
            if any(p['name'] == words[-1] for p in props):
                raise bad(number, text, 'second property of that name')
            props.append({'name': words[-1], 'type': PLY_TYPE_NAMES[words[-2]], 'count_type': count_type})
        else:
            raise bad(number, text, 'unknown keyword %r' % key)
    if header['format'] is None:
        raise ValueError('PLY header: no format line before end_header (line %d)' % number)
    header['body_offset'] = pos
    return header


def _ply_record(props, list_len=None):
    """Byte layout of one binary record of an element: ({property name: offset}, list offset or None, record bytes); a list
    property counts as its count field plus list_len entries.  None when a list is present and list_len is not given."""
    offsets, at, list_at = {}, 0, None
    for p in props:
        offsets[p['name']] = at
        if p['count_type'] is None:
            at += _PLY_WIDTH[p['type']]
        elif list_len is None:
            return None
        else:
            list_at = at
            at += _PLY_WIDTH[p['count_type']] + list_len * _PLY_WIDTH[p['type']]
    return offsets, list_at, at


def _ply_plan(header):
    """The elements read_ply decodes and the rules every decode path shares -> (vertex element or None, face element or None)."""
    vertex = face = None
    for el in header['elements']:
        lists = [p for p in el['properties'] if p['count_type'] is not None]
        if el['name'] == 'vertex':
            if lists:
                raise ValueError('read_ply: the vertex element has a list property (%r)' % lists[0]['name'])
            vertex = el
        elif el['name'] == 'face':
            if len(lists) > 1:
                raise ValueError('read_ply: the face element has %d list properties; one is supported' % len(lists))
            if lists and lists[0]['type'] in ('float32', 'float64'):
                raise ValueError('read_ply: the face list %r holds floats' % lists[0]['name'])
            face = el
        elif lists:
            raise ValueError('read_ply: element %r has a list property, so its size is not fixed by the header and it cannot '
                             'be skipped' % el['name'])
    if vertex is not None and vertex['count'] > 0:
        names = [p['name'] for p in vertex['properties']]
        if not all(k in names for k in 'xyz'):
            raise ValueError('read_ply: the vertex element lacks x, y or z')
    return vertex, face


def _ply_roles(props):
    """Which scalar properties of the vertex element become which key: x y z -> vertices, uint8 red green blue -> colors and
    colors_u8, nx ny nz -> normals, every other one (colours of another type included) -> vertex_properties."""
    by_name = {p['name']: p for p in props}
    roles = {}
    if all(k in by_name for k in 'xyz'):
        roles['vertices'] = ('x', 'y', 'z')
    if all(k in by_name and by_name[k]['type'] == 'uint8' for k in ('red', 'green', 'blue')):
        roles['colors'] = ('red', 'green', 'blue')
    if all(k in by_name for k in ('nx', 'ny', 'nz')):
        roles['normals'] = ('nx', 'ny', 'nz')
    taken = {k for names in roles.values() for k in names}
    return roles, [p for p in props if p['count_type'] is None and p['name'] not in taken]


def _ply_is_float(t):
    return t in ('float32', 'float64')


def _ply_fans(counts, flat, triangulate):
    """Polygons (counts [R], their indices one after the other in `flat`, int64 numpy) -> (triangles int64 [F, 3] in record order,
    a polygon (v0, v1, ..., vk-1) as the fan (v0, v1, v2), (v0, v2, v3), ..., and the record of every triangle [F])."""
    if counts.size and int(counts.min()) < 3:
        r = int(np.argmax(counts < 3))
        raise ValueError('read_ply: face %d has %d vertices; a polygon needs at least 3' % (r, int(counts[r])))
    if not triangulate and counts.size and int(counts.max()) != 3:
        r = int(np.argmax(counts != 3))
        raise ValueError('read_ply: face %d has %d vertices and triangulate=False' % (r, int(counts[r])))
    per = counts - 2
    start = np.cumsum(counts) - counts                                   # first entry of every record in flat
    rec = np.repeat(np.arange(counts.size, dtype=np.int64), per)
    t = np.arange(int(per.sum()), dtype=np.int64) - np.repeat(np.cumsum(per) - per, per)
    base = start[rec]
    tri = np.stack([flat[base], flat[base + t + 1], flat[base + t + 2]], axis=1) if rec.size else np.zeros((0, 3), dtype=np.int64)
    return tri.astype(np.int64), rec


def _ply_ascii_column(tokens, t, what):
    """Ascii tokens (numpy 'S' array) -> the numpy array of PLY type t: a number is read as a python float (floats) or int
    (integers, which must fit the type) and then stored in the property's type."""
    try:
        if _ply_is_float(t):
            return tokens.astype(np.float64).astype(_PLY_COUNT[t])
        wide = tokens.astype(np.int64)
    except ValueError as e:
        raise ValueError('read_ply: %s: %s' % (what, e)) from None
    info = np.iinfo(_PLY_COUNT[t])
    if wide.size and (int(wide.min()) < info.min or int(wide.max()) > info.max):
        raise ValueError('read_ply: %s: a value does not fit %s' % (what, t))
    return wide.astype(_PLY_COUNT[t])


def _ply_parse_host(data, header):
    """The body on the host -> ({vertex property: numpy array in its own type}, {face scalar property: array}, counts, flat)."""
    order = '>' if header['format'] == 'binary_big_endian' else '<'
    ascii_body = header['format'] == 'ascii'
    at = header['body_offset']
    tokens = np.array(data[at:].tobytes().split(), dtype='S') if ascii_body else None
    at = 0 if ascii_body else at
    columns = {'vertex': {}, 'face': {}}
    counts, flat = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)

    def short(el):
        return ValueError('read_ply: the file ends inside element %r (%d records expected): truncated' % (el['name'], el['count']))

    for el in header['elements']:
        props, n = el['properties'], el['count']
        lists = [i for i, p in enumerate(props) if p['count_type'] is not None]
        keep = el['name'] in columns
        if not lists:
            if ascii_body:
                need = n * len(props)
                if at + need > tokens.size:
                    raise short(el)
                if keep:
                    block = tokens[at:at + need].reshape(n, len(props))
                    for i, p in enumerate(props):
                        columns[el['name']][p['name']] = _ply_ascii_column(block[:, i], p['type'], '%s.%s' % (el['name'], p['name']))
                at += need
            else:
                dt = np.dtype([(p['name'], order + _PLY_COUNT[p['type']]) for p in props]) if props else np.dtype([])
                need = n * dt.itemsize
                if at + need > data.size:
                    raise short(el)
                if keep and props:
                    block = np.frombuffer(data, dtype=dt, count=n, offset=at)
                    for p in props:
                        columns[el['name']][p['name']] = np.ascontiguousarray(block[p['name']]).astype(_PLY_COUNT[p['type']])
                at += need
            continue
        # the face element with its one list
        li = lists[0]
        lp = props[li]
        scalars = [p for p in props if p['count_type'] is None]
        if n == 0:
            for p in scalars:
                columns['face'][p['name']] = np.zeros(0, dtype=_PLY_COUNT[p['type']])
            continue
        if ascii_body:
            if at >= tokens.size:
                raise short(el)
            k0 = int(_ply_ascii_column(tokens[at + li:at + li + 1], lp['count_type'], 'face count')[0]) if at + li < tokens.size else -1
            w = len(props) + k0
            uniform = k0 >= 0 and at + n * w <= tokens.size
            if uniform:
                block = tokens[at:at + n * w].reshape(n, w)
                try:
                    c = _ply_ascii_column(block[:, li], lp['count_type'], 'face count').astype(np.int64)
                    uniform = bool((c == k0).all())
                except ValueError:                                          # not a column of counts: the lists differ in length
                    uniform = False
            if uniform:
                counts = c
                flat = _ply_ascii_column(block[:, li + 1:li + 1 + k0].reshape(-1), lp['type'], 'face indices').astype(np.int64)
                for i, p in enumerate(props):
                    if i != li:
                        columns['face'][p['name']] = _ply_ascii_column(block[:, i if i < li else i + k0], p['type'], 'face.' + p['name'])
                at += n * w
                continue
            rows, cs, ids = {p['name']: [] for p in scalars}, [], []
            for r in range(n):
                for i, p in enumerate(props):
                    if at >= tokens.size:
                        raise short(el)
                    if i != li:
                        rows[p['name']].append(tokens[at])
                        at += 1
                        continue
                    k = int(_ply_ascii_column(tokens[at:at + 1], lp['count_type'], 'face count')[0])
                    if k < 0 or at + 1 + k > tokens.size:
                        raise short(el)
                    cs.append(k)
                    ids.append(tokens[at + 1:at + 1 + k])
                    at += 1 + k
            counts = np.asarray(cs, dtype=np.int64)
            flat = _ply_ascii_column(np.concatenate(ids), lp['type'], 'face indices').astype(np.int64)
            for p in scalars:
                columns['face'][p['name']] = _ply_ascii_column(np.array(rows[p['name']], dtype='S'), p['type'], 'face.' + p['name'])
            continue
        ct, it = order + _PLY_COUNT[lp['count_type']], order + _PLY_COUNT[lp['type']]
        list_at = _ply_record(props, 0)[1]
        if at + list_at + _PLY_WIDTH[lp['count_type']] > data.size:
            raise short(el)
        k0 = int(np.frombuffer(data, dtype=ct, count=1, offset=at + list_at)[0])
        stride = _ply_record(props, max(k0, 0))[2]
        uniform = 0 <= k0 <= 255 and at + n * stride <= data.size
        if uniform:
            dt = np.dtype([(p['name'], order + _PLY_COUNT[p['type']]) if p['count_type'] is None else (p['name'], [('n', ct), ('ids', it, (k0,))])
                           for p in props])
            block = np.frombuffer(data, dtype=dt, count=n, offset=at)
            c = block[lp['name']]['n'].astype(np.int64)
            uniform = bool((c == k0).all())
        if uniform:
            counts = c
            flat = np.ascontiguousarray(block[lp['name']]['ids']).astype(np.int64).reshape(-1)
            for p in scalars:
                columns['face'][p['name']] = np.ascontiguousarray(block[p['name']]).astype(_PLY_COUNT[p['type']])
            at += n * stride
            continue
        before = np.dtype([(p['name'], order + _PLY_COUNT[p['type']]) for p in props[:li]])       # lists of different lengths:
        after = np.dtype([(p['name'], order + _PLY_COUNT[p['type']]) for p in props[li + 1:]])    # one record at a time
        rows, cs, ids = {p['name']: [] for p in scalars}, [], []
        cw, iw = _PLY_WIDTH[lp['count_type']], _PLY_WIDTH[lp['type']]
        for r in range(n):
            if at + before.itemsize + cw > data.size:
                raise short(el)
            head = np.frombuffer(data, dtype=before, count=1, offset=at) if li else None
            k = int(np.frombuffer(data, dtype=ct, count=1, offset=at + before.itemsize)[0])
            at += before.itemsize + cw
            if k < 0 or at + k * iw + after.itemsize > data.size:
                raise short(el)
            cs.append(k)
            ids.append(np.frombuffer(data, dtype=it, count=k, offset=at))
            at += k * iw
            tail = np.frombuffer(data, dtype=after, count=1, offset=at) if li + 1 < len(props) else None
            at += after.itemsize
            for p in props[:li]:
                rows[p['name']].append(head[p['name']][0])
            for p in props[li + 1:]:
                rows[p['name']].append(tail[p['name']][0])
        counts = np.asarray(cs, dtype=np.int64)
        flat = np.concatenate(ids).astype(np.int64)
        for p in scalars:
            columns['face'][p['name']] = np.asarray(rows[p['name']], dtype=_PLY_COUNT[p['type']])
    return columns['vertex'], columns['face'], counts, flat


def _ply_widen(a):
    return a.astype(np.float64) if a.dtype.kind == 'f' else a.astype(np.int64)


def _ply_bad_index(record, n):
    return IndexError('read_ply: face %d has a vertex index outside [0, %d)' % (record, n))


def _ply_host(data, header, vertex, face, triangulate, device):
    vcols, fcols, counts, flat = _ply_parse_host(data, header)
    n = vertex['count'] if vertex is not None else 0
    tri, rec = _ply_fans(counts, flat, triangulate)
    wrong = (tri < 0) | (tri >= n)
    if wrong.any():
        raise _ply_bad_index(int(rec[int(np.argmax(wrong.any(axis=1)))]), n)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    roles, others = _ply_roles(vertex['properties']) if vertex is not None else ({}, [])
    mesh = {}
    stack = lambda names, dtype: (np.stack([vcols[k].astype(dtype) for k in names], axis=1) if n else np.zeros((0, 3), dtype=dtype))
    mesh['vertices'] = up(stack(roles['vertices'], np.float64) if 'vertices' in roles else np.zeros((0, 3), dtype=np.float64))
    mesh['faces'] = up(tri)
    if 'colors' in roles:
        u8 = stack(roles['colors'], np.uint8)
        mesh['colors'], mesh['colors_u8'] = up(u8.astype(np.float64) / 255.0), up(u8)
    if 'normals' in roles:
        mesh['normals'] = up(stack(roles['normals'], np.float64))
    mesh['vertex_properties'] = {p['name']: up(_ply_widen(vcols[p['name']])) for p in others}
    mesh['face_properties'] = {k: up(_ply_widen(v)) for k, v in fcols.items()}
    mesh['header'] = header
    return mesh


def _ply_device_layout(data_bytes, header, vertex, face):
    """Where every element's records start when the file can be decoded on the device -> ({element name: (first, stride)},
    K or None); or a str: the reason why it cannot (ascii, lists of different lengths, a record the kernels do not take)."""
    from . import _lib
    if header['format'] == 'ascii':
        return 'an ascii file'
    fixed, face_el = 0, None
    for el in header['elements']:
        if el is face and any(p['count_type'] is not None for p in el['properties']):
            face_el = el
        else:
            fixed += el['count'] * _ply_record(el['properties'])[2]
    K = None
    if face_el is not None and face_el['count'] > 0:
        lp = [p for p in face_el['properties'] if p['count_type'] is not None][0]
        left = data_bytes - header['body_offset'] - fixed - face_el['count'] * _ply_record(face_el['properties'], 0)[2]
        per = face_el['count'] * _PLY_WIDTH[lp['type']]
        if left < 0 or left % per != 0 or left // per not in (3, 4):
            return 'the size of the file does not fit %d faces of 3 or of 4 vertices each' % face_el['count']
        K = left // per
    elif data_bytes - header['body_offset'] < fixed:
        return 'a truncated body'
    layout, at = {}, header['body_offset']
    for el in header['elements']:
        stride = _ply_record(el['properties'], (K or 0) if el is face_el else None)[2]
        layout[el['name']] = (at, stride)
        at += el['count'] * stride
        if el in (vertex, face) and el['count'] > 0:
            scalars = sum(p['count_type'] is None for p in el['properties'])
            if stride > _lib.CONSTANTS['STIN_PLY_MAX_STRIDE'] or scalars + 3 > _lib.CONSTANTS['STIN_PLY_MAX_FIELDS']:
                return 'a %s record of %d bytes and %d properties is more than the decode kernel takes' % (el['name'], stride, scalars)
            if el['count'] > _lib.CONSTANTS['STIN_PLY_MAX_RECORDS']:
                return 'too many %s records' % el['name']
    return layout, K


def _ply_decode_call(lib, buf, first, stride, count, big, rows):
    """rows: [(offset, PLY type, destination tensor, STIN_PLY_TO_* name, column)] -> one stin_ply_decode launch."""
    import ctypes
    from . import _lib
    from .plan import _ptr, _stream
    if count == 0 or not rows:
        return
    words = []
    for offset, t, dst, to, col in rows:
        words += [offset, PLY_SCALARS.index(t), _ptr(dst), _lib.CONSTANTS['STIN_PLY_TO_' + to], dst.shape[1] if dst.dim() == 2 else 1, col]
    table = (ctypes.c_int64 * len(words))(*words)
    _lib.check(lib.stin_ply_decode(_ptr(buf), int(buf.numel()), first, stride, count, big, table, len(rows), _stream(buf)),
               'stin_ply_decode')


def _ply_device(data, header, vertex, face, layout, K, triangulate, device):
    """-> the mesh dict, or None when the device status says that a face's count differs from K."""
    from . import _lib
    from .plan import _ptr, _stream
    lib = _lib.load()
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise TypeError("read_ply: decode='device' needs a CUDA device")
    buf = torch.from_numpy(data).to(dev)                                   # the file's bytes, once
    big = int(header['format'] == 'binary_big_endian')
    n = vertex['count'] if vertex is not None else 0
    mesh = {'vertices': torch.empty(n, 3, dtype=torch.float64, device=dev)}
    props, face_props = {}, {}
    if vertex is not None:
        roles, others = _ply_roles(vertex['properties'])
        types = {p['name']: p['type'] for p in vertex['properties']}
        offsets, _, stride = _ply_record(vertex['properties'])
        rows = []
        for key, to, dtype in (('vertices', 'F64', torch.float64), ('colors', 'UNORM_F64', torch.float64), ('normals', 'F64', torch.float64)):
            if key in roles:
                mesh[key] = mesh.get(key) if key == 'vertices' else torch.empty(n, 3, dtype=dtype, device=dev)
                rows += [(offsets[k], types[k], mesh[key], to, c) for c, k in enumerate(roles[key])]
        if 'colors' in roles:
            mesh['colors_u8'] = torch.empty(n, 3, dtype=torch.uint8, device=dev)
            rows += [(offsets[k], types[k], mesh['colors_u8'], 'U8', c) for c, k in enumerate(roles['colors'])]
        for p in others:
            wide = _ply_is_float(p['type'])
            props[p['name']] = torch.empty(n, dtype=torch.float64 if wide else torch.int64, device=dev)
            rows.append((offsets[p['name']], p['type'], props[p['name']], 'F64' if wide else 'I64', 0))
        _ply_decode_call(lib, buf, layout['vertex'][0], stride, n, big, rows)
    nf = face['count'] if face is not None else 0
    lists = [p for p in face['properties'] if p['count_type'] is not None] if face is not None else []
    faces = torch.empty(0, 3, dtype=torch.int64, device=dev)
    status = None
    if face is not None:
        offsets, list_at, stride = _ply_record(face['properties'], K if lists and nf else 0)
        rows = []
        for p in face['properties']:
            if p['count_type'] is None:
                wide = _ply_is_float(p['type'])
                face_props[p['name']] = torch.empty(nf, dtype=torch.float64 if wide else torch.int64, device=dev)
                rows.append((offsets[p['name']], p['type'], face_props[p['name']], 'F64' if wide else 'I64', 0))
        _ply_decode_call(lib, buf, layout['face'][0], stride, nf, big, rows)
        if lists and nf:
            if K != 3 and not triangulate:
                raise ValueError('read_ply: the faces have %d vertices and triangulate=False' % K)
            faces = torch.empty(nf * (K - 2), 3, dtype=torch.int64, device=dev)
            status = torch.empty(4, dtype=torch.int64, device=dev)
            _lib.check(lib.stin_ply_faces(_ptr(buf), int(buf.numel()), layout['face'][0], stride, nf, big, list_at,
                                          PLY_SCALARS.index(lists[0]['count_type']), PLY_SCALARS.index(lists[0]['type']), K, n,
                                          _ptr(faces), _ptr(status), _stream(buf)), 'stin_ply_faces')
    if status is not None:
        st = status.cpu().tolist()                                         # the one read-back of the file
        if st[0] & _lib.CONSTANTS['STIN_PLY_COUNT_DIFFERS']:
            return None
        if st[0] & _lib.CONSTANTS['STIN_PLY_BAD_INDEX']:
            raise _ply_bad_index(st[2], n)
    mesh['faces'] = faces
    mesh['vertex_properties'], mesh['face_properties'], mesh['header'] = props, face_props, header
    order = ('vertices', 'faces', 'colors', 'colors_u8', 'normals', 'vertex_properties', 'face_properties', 'header')
    return {k: mesh[k] for k in order if k in mesh}


def read_ply(path, device='cuda', decode='auto', triangulate=True):
    """A PLY mesh file -> the `mesh` dict of tensors on `device` that preprocessing.graph_levels (and write_graph_levels,
    decimate_qem, cluster_mesh, vertex_normals, observe_vertices, FrameColors, sample_surface, views.render_mesh) take as it is:
        vertices [N, 3] float64 (x y z);  faces [F, 3] int64;
        colors [N, 3] float64 = uint8 / 255 (one IEEE division: open3d's vertex_colors) and colors_u8 [N, 3] uint8, when red, green
            and blue are uchar properties;  normals [N, 3] float64, when nx, ny and nz are present;
        vertex_properties / face_properties: every other scalar property under its own name, [N] / [records], widened to int64
            or float64 (`label`, `alpha`, `category_id`, ...);  header: read_ply_header's dict.
    Polygons with more than three vertices are cut into fans (v0, v1, v2), (v0, v2, v3), ... in record order (triangulate=False:
    ValueError instead); face_properties stay one entry per RECORD of the file.  Elements other than vertex and face are skipped
    when the header fixes their size; one with a list property is a ValueError that names it.  In an ascii file a number is read
    as a python float or int and then stored in the property's type.
    decode='device': the file's bytes are uploaded once and two kernels unpack them (stin_ply_decode for the scalar columns,
        stin_ply_faces for the list; include/stin_hip.h, "Mesh files"); the host parses nothing but the header.  For binary files
        whose lists all have 3 or all have 4 entries - which the host knows from the header and the size of the file alone.
    decode='host': numpy structured dtypes, then one upload per tensor: the same bytes on the same device (device='cpu' works).
    decode='auto': the device path when it applies; the host path for ascii files, for lists of different lengths, for records
        beyond the kernel's limits, and when the device status reports a count that differs (a file whose size fits by accident).
    ValueError for a truncated body (found from the header and the file size, before any launch), a polygon of fewer than 3
    vertices; IndexError, naming the first such face, for a vertex index outside [0, N)."""
    if decode not in ('auto', 'device', 'host'):
        raise ValueError("read_ply: decode is 'auto', 'device' or 'host'")
    data = np.fromfile(path, dtype=np.uint8)
    header = read_ply_header(data[:PLY_MAX_HEADER_BYTES].tobytes())
    vertex, face = _ply_plan(header)
    if decode == 'device' or (decode == 'auto' and torch.device(device).type == 'cuda'):
        plan = _ply_device_layout(int(data.size), header, vertex, face)
        if isinstance(plan, str):
            if decode == 'device':
                raise ValueError('read_ply: %s cannot be decoded on the device: %s' % (path, plan))
        else:
            mesh = _ply_device(data, header, vertex, face, plan[0], plan[1], triangulate, device)
            if mesh is not None:
                return mesh
            if decode == 'device':
                raise ValueError('read_ply: %s: the faces do not all have %d vertices' % (path, plan[1]))
    return _ply_host(data, header, vertex, face, triangulate, device)


def read_scannet_mesh(scan_dir, scan_name, with_labels=True, device='cuda', decode='auto'):
    """A ScanNet scan directory -> (mesh, labels): read_ply of <scan_dir>/<scan_name>_vh_clean_2.ply and, with_labels, the `label`
    vertex property of <scan_name>_vh_clean_2.labels.ply through preprocessing.remap_scannet_labels (ids above 40 -> 0, then the
    class table) as int64 [N] on the device - what graph_levels takes as `labels` in train mode; labels is None otherwise.
    ValueError when the label file has another number of vertices than the mesh.  The segs.json / aggregation.json route to
    instance labels is out of scope."""
    import os
    from .preprocessing import remap_scannet_labels
    mesh = read_ply(os.path.join(str(scan_dir), '%s_vh_clean_2.ply' % scan_name), device=device, decode=decode)
    if not with_labels:
        return mesh, None
    path = os.path.join(str(scan_dir), '%s_vh_clean_2.labels.ply' % scan_name)
    labelled = read_ply(path, device=device, decode=decode)
    if 'label' not in labelled['vertex_properties']:
        raise ValueError('%s has no vertex property `label`' % path)
    labels = labelled['vertex_properties']['label']
    if int(labels.shape[0]) != int(mesh['vertices'].shape[0]):
        raise ValueError('%s has %d vertices, the mesh has %d' % (path, int(labels.shape[0]), int(mesh['vertices'].shape[0])))
    return mesh, remap_scannet_labels(labels)


def vertex_labels_from_faces(faces, face_labels, num_vertices, num_classes, strict=True):
    """Per-face labels -> per-vertex labels, the Matterport step of the reference (preprocessing/graph_level_generation.py:328-336):
    every face votes with its label at its three corners and a vertex takes the class with the most votes, the lowest one on a
    tie, 0 without faces (np.argmax over the rows of the histogram).  faces [F, 3] int, face_labels [F] int in [0, num_classes)
    (CUDA), num_classes <= STIN_VOTE_MAX_CLASSES -> int64 [num_vertices].  Integer counts: the same bytes on every run
    (stin_face_label_vote).  A label outside [0, num_classes) or a vertex outside [0, num_vertices) is not counted; strict:
    ValueError / IndexError that names the first such face; strict=False: -> (labels, flags) with the STIN_VOTE_BAD_* bits.
    Out of scope: the Matterport category tables that produce face_labels from `category_id` (premapping,
    MATTERPORT_CLASS_REMAP) and the ScanNet segs.json / aggregation.json route."""
    from . import _lib
    from .plan import _ptr, _stream
    if not (torch.is_tensor(faces) and faces.is_cuda and torch.is_tensor(face_labels) and face_labels.is_cuda):
        raise TypeError('faces and face_labels must be CUDA tensors (no CPU fallback exists)')
    lib = _lib.load()
    f = faces.long().reshape(-1, 3).contiguous()
    l = face_labels.long().reshape(-1).contiguous()
    nf, n, c, dev = int(f.shape[0]), int(num_vertices), int(num_classes), f.device
    if int(l.shape[0]) != nf:
        raise ValueError('vertex_labels_from_faces: %d faces and %d face labels' % (nf, int(l.shape[0])))
    if n < 0 or not 1 <= c <= _lib.CONSTANTS['STIN_VOTE_MAX_CLASSES']:
        raise ValueError('vertex_labels_from_faces: num_vertices >= 0 and 1 <= num_classes <= %d' % _lib.CONSTANTS['STIN_VOTE_MAX_CLASSES'])
    out = torch.empty(max(n, 1), dtype=torch.int64, device=dev)[:n]
    status = torch.empty(4, dtype=torch.int64, device=dev)
    ws_bytes = lib.stin_face_label_vote_workspace_bytes(n, c)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    _lib.check(lib.stin_face_label_vote(_ptr(f), _ptr(l), nf, n, c, _ptr(out), _ptr(status), _ptr(ws), ws_bytes, _stream(f)),
               'stin_face_label_vote')
    st = status.cpu().tolist()
    if not strict:
        return out, st[0]
    if st[0] & _lib.CONSTANTS['STIN_VOTE_BAD_LABEL']:
        raise ValueError('vertex_labels_from_faces: the label of face %d lies outside [0, %d)' % (st[1], c))
    if st[0] & _lib.CONSTANTS['STIN_VOTE_BAD_INDEX']:
        raise IndexError('vertex_labels_from_faces: face %d has a vertex outside [0, %d)' % (st[2], n))
    return out


def write_scene_from_ply(out_dir, ply_path, levels, dilated_levels, dilation_dists, labels_path=None, crops=None, masks=None):
    """One scene from its mesh file to the files training reads, a chain of existing calls and nothing else:
    read_ply(ply_path) -> write_graph_levels(<out_dir>/graphs, <scene>, ...) (scene = the file name without `.ply`; labels_path: a
    ScanNet `.labels.ply` whose `label` property goes through remap_scannet_labels - train mode); then, when `crops` is a dict,
    write_crops(graph file, crops.pop('out_dir', <out_dir>/crops), **crops); then, when `masks` is a dict,
    write_circle_masks(graph file, masks.pop('masks_dir', <out_dir>/masks/<scene>), circle_masks(edges of the mesh's faces, N,
    **masks)).  -> the list of the files written, the graph file first."""
    import os
    from .preprocessing import circle_masks, edges_from_faces, remap_scannet_labels
    mesh = read_ply(ply_path)
    labels = None
    if labels_path is not None:
        labels = remap_scannet_labels(read_ply(labels_path)['vertex_properties']['label'])
    scene = os.path.basename(str(ply_path)).rsplit('.', 1)[0]
    graph = write_graph_levels(os.path.join(str(out_dir), 'graphs'), scene, mesh, levels, dilated_levels, dilation_dists, labels=labels)
    written = [graph]
    if crops is not None:
        kw = dict(crops)
        written += write_crops(graph, kw.pop('out_dir', os.path.join(str(out_dir), 'crops')), **kw)
    if masks is not None:
        kw = dict(masks)
        masks_dir = kw.pop('masks_dir', os.path.join(str(out_dir), 'masks', scene))
        n = int(mesh['vertices'].shape[0])
        written += write_circle_masks(graph, masks_dir, circle_masks(edges_from_faces(mesh['faces'], n), n, **kw))
    return written
