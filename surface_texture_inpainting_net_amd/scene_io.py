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
