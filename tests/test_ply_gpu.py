"""PLY mesh files on the GPU (csrc/stin_ply.hip through scene_io.read_ply / read_scannet_mesh / vertex_labels_from_faces /
write_scene_from_ply): read_ply(decode='device') equals the restatement of the contract (tests/_ply_oracle.py) and the host path
(decode='host') byte for byte, and 'auto' equals both.

Sizes cross the kernels' edges, not the workload's: a workgroup stages 256 records, so N = 257 and F = 509 give full and partial
runs and N = 67, F = 131 a lone partial one; record strides 13, 15, 16, 17, 26 and 27 with body offsets of all 16 residues put the
staged range at every alignment against the 16-byte loads, with the end of the file inside the last chunk."""
import functools
import os

import numpy as np
import pytest
import torch

import _ply_oracle as PO
import _qem_oracle as QO
from surface_texture_inpainting_net_amd import _lib
from surface_texture_inpainting_net_amd import preprocessing as P
from surface_texture_inpainting_net_amd import scene_io as IO
from surface_texture_inpainting_net_amd import views as VW

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu
TRI = [('list', 'uchar', 'int', 'vertex_indices')]
RGBA = [('float', 'x'), ('float', 'y'), ('float', 'z'), ('uchar', 'red'), ('uchar', 'green'), ('uchar', 'blue'), ('uchar', 'alpha')]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_tensors(a, b, where=''):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), (where, list(a), list(b))
        for k in a:
            same_tensors(a[k], b[k], '%s.%s' % (where, k))
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same_tensors(x, y, '%s[%d]' % (where, i))
    elif torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.device == b.device and a.shape == b.shape, where
        assert torch.equal(a, b) or a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), where      # (bytes: NaN == NaN)
    else:
        assert a == b, where


def read_all_ways(tmp_path, blob, name='mesh.ply', **kw):
    """device == restatement, device == host, auto == device -> the device path's dict"""
    path = tmp_path / name
    path.write_bytes(blob)
    got = IO.read_ply(str(path), device=DEV, decode='device', **kw)
    assert all(t.is_cuda for t in (got['vertices'], got['faces']))
    PO.same_mesh(got, PO.decode(blob, **kw))
    same_tensors(got, IO.read_ply(str(path), device=DEV, decode='host', **kw))
    same_tensors(got, IO.read_ply(str(path), device=DEV, **kw))
    return got


def columns(n, f, seed, coord=np.float32, limit=None):
    rng = np.random.default_rng(seed)
    cols = {k: (rng.standard_normal(n) * 3.0).astype(coord).tolist() for k in 'xyz'}
    cols.update({k: rng.integers(0, 256, n).tolist() for k in ('red', 'green', 'blue', 'alpha')})
    return cols, rng.integers(0, limit or max(n, 1), (f, 3)).tolist()


# ------------------------------------------------------------------------------------------------------------------ round trip
def test_write_ply_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    v = dev(rng.standard_normal((257, 3)).astype(np.float32))
    f = dev(rng.integers(0, 257, (509, 3)))
    c = dev(rng.integers(0, 256, (257, 3)).astype(np.uint8))
    unit = dev(c.cpu().numpy().astype(np.float64) / 255.0)      # (numpy: torch divides by a scalar through its reciprocal on the GPU)
    path = str(tmp_path / 'views.ply')
    VW.write_ply(path, v, f, c)
    for decode in ('device', 'host', 'auto'):
        m = IO.read_ply(path, device=DEV, decode=decode)
        assert torch.equal(m['vertices'], v.double()) and torch.equal(m['faces'], f) and torch.equal(m['colors_u8'], c)
        assert torch.equal(m['colors'], unit) and m['colors'].dtype == torch.float64
        assert m['vertex_properties'] == {} and m['face_properties'] == {} and m['header']['elements'][0]['count'] == 257
    PO.same_mesh(m, PO.decode(open(path, 'rb').read()))
    VW.write_ply(path, v, f, unit)                               # float colours are written as the same bytes
    assert torch.equal(IO.read_ply(path, device=DEV, decode='device')['colors_u8'], c)


# ------------------------------------------------------------------------------------------------------------------- alignment
@pytest.mark.parametrize('fmt', ('binary_little_endian', 'binary_big_endian'))
@pytest.mark.parametrize('stride', (16, 15, 27))
def test_every_body_offset_and_odd_strides(tmp_path, stride, fmt):
    coord = 'double' if stride == 27 else 'float'
    cols, faces = columns(67, 131, stride, np.float64 if stride == 27 else np.float32)
    props = [(coord, k) for k in 'xyz'] + RGBA[3:7 if stride == 16 else 6]
    residues = set()
    for pad in range(16):
        blob = PO.make_ply(fmt, props, cols, TRI, {'vertex_indices': faces}, comment='x' * pad)
        m = read_all_ways(tmp_path, blob)
        residues.add(m['header']['body_offset'] % 16)
        layout, K = IO._ply_device_layout(len(blob), m['header'], *IO._ply_plan(m['header']))
        assert layout['vertex'][1] == stride and layout['face'][1] == 13 and K == 3
    assert residues == set(range(16))
    assert m['vertices'][:, 2].tolist() == cols['z'] and m['colors_u8'][:, 0].tolist() == cols['red'] and m['faces'].tolist() == faces


# ----------------------------------------------------------------------------------------------------------------------- types
@pytest.mark.parametrize('fmt', ('binary_little_endian', 'binary_big_endian'))
def test_every_scalar_type_as_a_vertex_property(tmp_path, fmt):
    rng = np.random.default_rng(3)
    n = 300
    edge = {'char': (-128, 127), 'uchar': (0, 255), 'short': (-32768, 32767), 'ushort': (0, 65535), 'int': (-2 ** 31, 2 ** 31 - 1),
            'uint': (0, 2 ** 32 - 1)}
    cols, props = {}, []
    for t, (lo, hi) in edge.items():
        cols['p_' + t] = [lo, hi, -1 if lo < 0 else hi // 2 + 7] + rng.integers(lo, hi + 1, n - 3).tolist()
        props.append((t, 'p_' + t))
    cols['p_float'] = [3.0e38, -1.0e-45, float('inf')] + rng.standard_normal(n - 3).astype(np.float32).tolist()
    cols['p_double'] = [1.0e-300, -1.7e308, 0.1] + rng.standard_normal(n - 3).tolist()
    props += [('float', 'p_float'), ('double', 'p_double')]
    cols.update({k: rng.standard_normal(n).tolist() for k in 'xyz'})
    props = props[:4] + [('double', 'x')] + props[4:] + [('double', 'y'), ('double', 'z')]        # 50-byte records, x at byte 6
    m = read_all_ways(tmp_path, PO.make_ply(fmt, props, cols))
    p = m['vertex_properties']
    assert p['p_uint'].dtype == torch.int64 and p['p_uint'][:3].tolist() == [0, 2 ** 32 - 1, 2 ** 31 + 6]
    assert p['p_char'][:3].tolist() == [-128, 127, -1] and p['p_short'][:3].tolist() == [-32768, 32767, -1]
    assert p['p_int'].tolist() == cols['p_int'] and p['p_double'].tolist() == cols['p_double'] and p['p_double'].dtype == torch.float64
    assert p['p_float'][:3].tolist() == [float(np.float32(3.0e38)), float(np.float32(-1.0e-45)), float('inf')]
    assert m['vertices'].tolist() == [list(r) for r in zip(cols['x'], cols['y'], cols['z'])]


@pytest.mark.parametrize('count_type', ('uchar', 'ushort', 'int'))
@pytest.mark.parametrize('index_type', ('short', 'ushort', 'int', 'uint'))
def test_index_and_count_types(tmp_path, index_type, count_type):
    cols, faces = columns(67, 131, 5)
    for fmt in ('binary_little_endian', 'binary_big_endian'):
        fprops = [('ushort', 'material'), ('list', count_type, index_type, 'vertex_index'), ('double', 'area'), ('char', 'flag')]
        fcols = {'material': list(range(60000, 60131)), 'vertex_index': faces, 'area': [0.1 * i for i in range(131)],
                 'flag': [i - 128 for i in range(131)]}
        m = read_all_ways(tmp_path, PO.make_ply(fmt, RGBA, cols, fprops, fcols))
        assert m['faces'].tolist() == faces and m['face_properties']['flag'].tolist() == fcols['flag']
        assert m['face_properties']['area'].tolist() == fcols['area'] and m['face_properties']['material'].tolist() == fcols['material']


def test_uint_indices_above_2_to_31_are_out_of_range_not_negative(tmp_path):
    cols, faces = columns(67, 131, 6)
    faces[40][2] = 2 ** 32 - 1
    blob = PO.make_ply('binary_little_endian', RGBA, cols, [('list', 'uchar', 'uint', 'vertex_indices')], {'vertex_indices': faces})
    (tmp_path / 'm.ply').write_bytes(blob)
    for decode in ('device', 'host', 'auto'):
        with pytest.raises(IndexError, match='face 40 has'):
            IO.read_ply(str(tmp_path / 'm.ply'), device=DEV, decode=decode)


# ----------------------------------------------------------------------------------------------------------------------- quads
def test_quads_become_two_triangles_in_record_order(tmp_path):
    cols, _ = columns(257, 0, 7)
    quads = np.random.default_rng(7).integers(0, 257, (509, 4)).tolist()
    fprops = [('list', 'uchar', 'int', 'vertex_indices'), ('int', 'category_id')]
    fcols = {'vertex_indices': quads, 'category_id': list(range(-254, 255))}
    m = read_all_ways(tmp_path, PO.make_ply('binary_little_endian', RGBA, cols, fprops, fcols))
    want = [[q[0], q[1], q[2]] if t == 0 else [q[0], q[2], q[3]] for q in quads for t in (0, 1)]
    assert m['faces'].tolist() == want and m['face_properties']['category_id'].tolist() == fcols['category_id']
    (tmp_path / 'q.ply').write_bytes(PO.make_ply('binary_little_endian', RGBA, cols, fprops, fcols))
    for decode in ('device', 'host'):
        with pytest.raises(ValueError, match='triangulate=False'):
            IO.read_ply(str(tmp_path / 'q.ply'), device=DEV, decode=decode, triangulate=False)


def test_lists_of_different_lengths_fall_back_to_the_host_path(tmp_path):
    cols, _ = columns(257, 0, 8)
    quads = np.random.default_rng(8).integers(0, 257, (509, 4)).tolist()
    fprops = [('uchar', 'flag'), ('list', 'uchar', 'int', 'vertex_indices')]
    flags = [i % 256 for i in range(509)]
    for name, polys in (('last', quads[:-1] + [quads[-1][:3]]),                       # the size of the file gives it away
                        ('swap', [quads[0][:3], quads[1] + [5]] + quads[2:]),          # 3 + 5: the size fits K = 4, the status tells
                        ('late', quads[:300] + [quads[300][:3], quads[301] + [9]] + quads[302:])):
        blob = PO.make_ply('binary_little_endian', RGBA, cols, fprops, {'flag': flags, 'vertex_indices': polys})
        path = tmp_path / (name + '.ply')
        path.write_bytes(blob)
        auto = IO.read_ply(str(path), device=DEV)
        PO.same_mesh(auto, PO.decode(blob))
        same_tensors(auto, IO.read_ply(str(path), device=DEV, decode='host'))
        assert auto['faces'].shape == (1017 if name == 'last' else 1018, 3) and auto['faces'].is_cuda
        with pytest.raises(ValueError):
            IO.read_ply(str(path), device=DEV, decode='device')
        layout = IO._ply_device_layout(len(blob), auto['header'], *IO._ply_plan(auto['header']))
        assert isinstance(layout, str) == (name == 'last')


# ---------------------------------------------------------------------------------------------------------------------- errors
@pytest.mark.parametrize('record', (0, 300, 508))
def test_an_index_equal_to_n_names_its_face(tmp_path, record):
    cols, faces = columns(257, 509, 9)
    faces[record][record % 3] = 257
    if record == 0:
        faces[400][1] = 300                                                            # a later one: the FIRST is named
    (tmp_path / 'm.ply').write_bytes(PO.make_ply('binary_little_endian', RGBA, cols, TRI, {'vertex_indices': faces}))
    for decode in ('device', 'host', 'auto'):
        with pytest.raises(IndexError, match=r'face %d has a vertex index outside \[0, 257\)' % record):
            IO.read_ply(str(tmp_path / 'm.ply'), device=DEV, decode=decode)


@pytest.mark.parametrize('index_type', ('char', 'short', 'int'))
def test_a_negative_index_is_rejected(tmp_path, index_type):
    cols, faces = columns(67, 131, 10)
    faces[77][0] = -1
    blob = PO.make_ply('binary_big_endian', RGBA, cols, [('list', 'uchar', index_type, 'vertex_indices')], {'vertex_indices': faces})
    (tmp_path / 'm.ply').write_bytes(blob)
    for decode in ('device', 'host', 'auto'):
        with pytest.raises(IndexError, match='face 77 has'):
            IO.read_ply(str(tmp_path / 'm.ply'), device=DEV, decode=decode)


def test_a_truncated_body_raises_before_any_launch(tmp_path, monkeypatch):
    cols, faces = columns(67, 131, 11)
    blob = PO.make_ply('binary_little_endian', RGBA, cols, TRI, {'vertex_indices': faces})
    start = blob.index(b'end_header\n') + 11

    def no_launch(*a, **k):
        raise AssertionError('the device path was entered')
    monkeypatch.setattr(IO, '_ply_device', no_launch)
    for cut in (start, start + 100, start + 67 * 16, start + 67 * 16 + 13 * 60 + 5, len(blob) - 13, len(blob) - 1):
        (tmp_path / 'cut.ply').write_bytes(blob[:cut])
        for decode in ('device', 'auto', 'host'):
            with pytest.raises(ValueError):
                IO.read_ply(str(tmp_path / 'cut.ply'), device=DEV, decode=decode)
    no_faces = PO.make_ply('binary_little_endian', RGBA, cols)
    (tmp_path / 'cut.ply').write_bytes(no_faces[:-1])
    for decode in ('device', 'auto'):
        with pytest.raises(ValueError, match='truncated'):
            IO.read_ply(str(tmp_path / 'cut.ply'), device=DEV, decode=decode)


# -------------------------------------------------------------------------------------------------------------- empty and tiny
@pytest.mark.parametrize('n,f', ((0, 0), (1, 0), (3, 1)))
def test_empty_and_tiny_files(tmp_path, n, f):
    cols, faces = columns(n, f, 12)
    for fmt in ('binary_little_endian', 'binary_big_endian'):
        m = read_all_ways(tmp_path, PO.make_ply(fmt, RGBA, cols, TRI, {'vertex_indices': faces}, n_faces=f))
        assert m['vertices'].shape == (n, 3) and m['faces'].shape == (f, 3) and m['colors_u8'].shape == (n, 3)
        assert m['vertex_properties']['alpha'].shape == (n,) and m['faces'].dtype == torch.int64


# ----------------------------------------------------------------------------------------------------------------- label files
def test_scannet_label_file_through_read_scannet_mesh(tmp_path):
    cols, faces = columns(257, 509, 13)
    mesh = PO.make_ply('binary_little_endian', RGBA, cols, TRI, {'vertex_indices': faces})
    raw = np.random.default_rng(13).integers(0, 48, 257)
    raw[[0, 100, 256]] = (65535, 41, 40)
    labelled = PO.make_ply('binary_little_endian', RGBA + [('ushort', 'label')], dict(cols, label=raw.tolist()), TRI, {'vertex_indices': faces})
    (tmp_path / 'scene0191_00_vh_clean_2.ply').write_bytes(mesh)
    (tmp_path / 'scene0191_00_vh_clean_2.labels.ply').write_bytes(labelled)
    for decode in ('device', 'host', 'auto'):
        got, labels = IO.read_scannet_mesh(str(tmp_path), 'scene0191_00', device=DEV, decode=decode)
        PO.same_mesh(got, PO.decode(mesh))
        assert labels.is_cuda and labels.dtype == torch.int64
        assert labels.tolist() == P.remap_scannet_labels(PO.decode(labelled)['vertex_properties']['label']).tolist()
    assert labels[0].item() == labels[100].item() == P.SCANNET_CLASS_REMAP[0]
    assert IO.read_scannet_mesh(str(tmp_path), 'scene0191_00', with_labels=False, device=DEV)[1] is None
    shorter = {k: v[:256] for k, v in dict(cols, label=raw.tolist()).items()}
    (tmp_path / 'scene0191_00_vh_clean_2.labels.ply').write_bytes(PO.make_ply('binary_little_endian', RGBA + [('ushort', 'label')], shorter))
    with pytest.raises(ValueError, match='256 vertices'):
        IO.read_scannet_mesh(str(tmp_path), 'scene0191_00', device=DEV)


# ------------------------------------------------------------------------------------------------------------------------ vote
@functools.lru_cache(maxsize=None)
def vote_case(C):
    rng = np.random.default_rng(100 + C)
    faces = rng.integers(10, 250, (509, 3))                        # vertices 0 .. 9 and 250 .. 256 start without faces
    labels = rng.integers(0, C, 509)
    faces[:200, 0] = 5                                             # a vertex of degree 200
    faces[200, 1], labels[200] = 7, 9                              # built ties: one vote each for 9 and 3 -> 3
    faces[201, 2], labels[201] = 7, 3
    faces[202], labels[202] = (8, 8, 9), C - 1                     # a face that names a vertex twice votes twice
    faces[203], labels[203] = (8, 9, 9), 0                         # 8: {C-1: 2, 0: 1}; 9: {C-1: 1, 0: 2}
    return faces, labels


@pytest.mark.parametrize('C', (22, 64))
def test_vote_equals_the_reference_loop(C):
    faces, labels = vote_case(C)
    want, flagged = PO.vote(faces, labels, 257, C)
    assert not flagged and want[7] == 3 and want[8] == C - 1 and want[9] == 0 and want[0] == 0 and want[256] == 0
    got = IO.vertex_labels_from_faces(dev(faces), dev(labels), 257, C)
    assert got.dtype == torch.int64 and got.shape == (257,) and np.array_equal(got.cpu().numpy(), want)
    got2, flags = IO.vertex_labels_from_faces(dev(faces), dev(labels), 257, C, strict=False)
    assert flags == 0 and torch.equal(got, got2)


@pytest.mark.parametrize('C', (22, 64))
def test_a_label_equal_to_c_is_flagged_and_not_counted(C):
    faces, labels = vote_case(C)
    labels = labels.copy()
    labels[201] = C                                                # vertex 7 keeps one vote: 9
    labels[300] = C
    want, flagged = PO.vote(faces, labels, 257, C)
    assert flagged and want[7] == 9
    got, flags = IO.vertex_labels_from_faces(dev(faces), dev(labels), 257, C, strict=False)
    assert flags == _lib.CONSTANTS['STIN_VOTE_BAD_LABEL'] and np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(ValueError, match='face 201 '):
        IO.vertex_labels_from_faces(dev(faces), dev(labels), 257, C)
    labels[201], labels[300] = 0, -1
    with pytest.raises(ValueError, match='face 300 '):
        IO.vertex_labels_from_faces(dev(faces), dev(labels), 257, C)


def test_vote_edges():
    faces, labels = vote_case(22)
    bad = faces.copy()
    bad[77, 1] = 257
    with pytest.raises(IndexError, match='face 77 '):
        IO.vertex_labels_from_faces(dev(bad), dev(labels), 257, 22)
    none = IO.vertex_labels_from_faces(dev(faces[:0]), dev(labels[:0]), 5, 22)
    assert none.tolist() == [0] * 5
    assert IO.vertex_labels_from_faces(dev(faces[:0]), dev(labels[:0]), 0, 22).shape == (0,)
    one = IO.vertex_labels_from_faces(dev(faces), dev(np.zeros(509, dtype=np.int64)), 257, 1)
    assert one.tolist() == [0] * 257
    with pytest.raises(ValueError):
        IO.vertex_labels_from_faces(dev(faces), dev(labels), 257, 65)
    with pytest.raises(TypeError):
        IO.vertex_labels_from_faces(torch.from_numpy(faces), torch.from_numpy(labels), 257, 22)


# ----------------------------------------------------------------------------------------------------------------------- chain
@functools.lru_cache(maxsize=None)
def sphere_file_parts():
    V, F = QO.icosphere(3)
    colors = np.random.default_rng(14).integers(0, 256, (V.shape[0], 3)).astype(np.uint8)
    return V.astype(np.float32), np.asarray(F, dtype=np.int64), colors


def test_scene_from_ply_to_graph_file_masks_and_sample(tmp_path):
    V, F, colors = sphere_file_parts()
    path = str(tmp_path / 'scene0000_00.ply')
    VW.write_ply(path, V, F, colors)
    levels, dilated, dists = ['100', '30'], [0, 1], [2]
    written = IO.write_scene_from_ply(str(tmp_path / 'out'), path, levels, dilated, dists,
                                      crops=dict(block_size=3.0, stride=1.5), masks=dict(radius=3, num_masks=2, seed=1))
    assert written[0] == str(tmp_path / 'out' / 'graphs' / 'scene0000_00.pt') and all(os.path.exists(p) for p in written)
    saved = torch.load(written[0], map_location='cpu', weights_only=False)
    mesh = IO.read_ply(path, device=DEV)
    want = P.graph_levels(mesh, levels, dilated, dists)
    to_cpu = lambda v: v.cpu() if torch.is_tensor(v) else [to_cpu(y) for y in v] if isinstance(v, (list, tuple)) else v
    same_tensors({k: to_cpu(v) for k, v in saved.items()}, {k: to_cpu(v) for k, v in want.items()})
    assert saved['vertices'][0].shape == (V.shape[0], 10) and torch.equal(saved['vertices'][0][:, :3], torch.from_numpy(V))
    assert torch.equal(saved['vertices'][0][:, 3:6], torch.from_numpy(colors).double().div(255.0).float())
    masks = [p for p in written if p.endswith('.npz')]
    assert masks and all(os.path.dirname(p) == str(tmp_path / 'out' / 'masks' / 'scene0000_00') for p in masks)
    sample = IO.load_scene(written[0], masks[0], end_level=2)
    assert sample.x.shape == (V.shape[0], 10) and int(sample.num_vertices[0, 0]) == V.shape[0] and sample['name'] == 'scene0000_00'
    assert torch.equal(sample.color, saved['vertices'][0][:, 3:6] * 2.0 - 1.0)
    for p in written:
        if p.endswith('.pt') and p != written[0]:
            assert os.path.dirname(p) == str(tmp_path / 'out' / 'crops')
            assert 'vertices' in torch.load(p, map_location='cpu', weights_only=False)
    only = IO.write_scene_from_ply(str(tmp_path / 'plain'), path, levels, dilated, dists)
    assert only == [str(tmp_path / 'plain' / 'graphs' / 'scene0000_00.pt')]


def test_the_mesh_dict_feeds_the_mesh_entry_points_as_it_is(tmp_path):
    V, F, colors = sphere_file_parts()
    path = str(tmp_path / 'sphere.ply')
    VW.write_ply(path, V, F, colors)
    m = IO.read_ply(path)                                                      # the defaults: cuda, auto
    v, f, c = dev(V).double(), dev(F), dev(colors.astype(np.float64) / 255.0)
    assert m['vertices'].is_cuda and torch.equal(m['vertices'], v) and torch.equal(m['faces'], f) and torch.equal(m['colors'], c)
    assert torch.equal(P.vertex_normals(m['vertices'], m['faces']), P.vertex_normals(v, f))
    same_tensors(list(P.decimate_qem(m['vertices'], m['faces'], percent=50)), list(P.decimate_qem(v, f, percent=50)))
    pose = np.eye(4)
    pose[2, 3] = -4.0
    args = (pose[None], (40.0, 40.0, 16.0, 16.0), 32, 32)
    image = VW.render_mesh(m['vertices'], m['faces'], m['colors'], *args)
    assert torch.equal(image, VW.render_mesh(v, f, c, *args)) and int(image.sum()) > 0
