"""Result views, the part that needs no GPU: the numpy restatement of the render contract (tests/_render_oracle.py) on 8 x 8 images
with an identity pose and dyadic values, where every expected pixel can be written down by hand; `result_colorings` against hand
values; the PNG and PLY writers decoded again with zlib and struct; the entry points' declarations, their argument checks (which
return before anything is launched) and their refusal of CPU tensors."""
import ctypes
import struct
import zlib

import numpy as np
import pytest
import torch

import _render_oracle as RO
from surface_texture_inpainting_net_amd import _lib, views

S = 8
CAM = (4.0, 4.0, 3.5, 3.5)                                               # X = 4 x / z + 3.5: exact for the dyadic values used here
EYE = np.eye(4)[None]                                                    # at the origin, +z forward, +x right, +y down the rows
RGB = np.array([[0.25, 0.5, 1.0], [0.5, 0.125, 0.0], [0.75, 1.0, 0.5]], dtype=np.float32)


def at(u, v, z=1.0):
    """The point that projects to (u, v) at depth z through CAM."""
    return [(u - 3.5) / 4.0 * z, (v - 3.5) / 4.0 * z, z]


def run(V, F, C=None, **kw):
    V = np.asarray(V, dtype=np.float64).reshape(-1, 3)
    C = np.tile(RGB, ((len(V) + 2) // 3, 1))[:len(V)] if C is None else np.asarray(C, dtype=np.float32)
    return RO.render(V, np.asarray(F, dtype=np.int64).reshape(-1, 3), C, EYE, CAM, S, S, **kw)


def test_a_triangle_covers_its_centres_with_inclusive_edges():
    corner = [at(1, 1), at(5, 1), at(1, 5)]                              # legs along row 1 and column 1, hypotenuse i + j = 6
    want = np.array([[1 <= i and 1 <= j and i + j <= 6 for j in range(S)] for i in range(S)])
    assert want.sum() == 15
    for faces in ([[0, 1, 2]], [[0, 2, 1]]):                             # both orientations are drawn
        r = run(corner, faces)
        assert r.face.dtype == np.int32 and r.face.shape == (1, S, S) and r.status == 0
        assert np.array_equal(r.face[0] == 0, want) and np.array_equal(r.face[0] == -1, ~want)
        assert np.array_equal(r.depth[0], np.where(want, 1000, 0).astype(np.uint16))
    # half a pixel further in: the hypotenuse i + j = 5.5 passes between the centres, the legs at 1.5 cover from 2 on
    r = run([at(1.5, 1.5), at(4, 1.5), at(1.5, 4)], [[0, 1, 2]])
    want = np.array([[2 <= i and 2 <= j and i + j <= 5 for j in range(S)] for i in range(S)])
    assert want.sum() == 3 and np.array_equal(r.face[0] == 0, want)
    # H != W: a column index beyond the height is reached, a row index beyond it is not
    wide = RO.render(np.asarray([at(0, 0), at(11, 0), at(0, 3)]), np.array([[0, 1, 2]]), RGB, EYE, CAM, 4, 12)
    assert wide.face.shape == (1, 4, 12) and wide.face[0, 0, 11] == 0 and wide.face[0, 3, 0] == 0 and wide.face[0, 3, 1] == -1


def test_a_vertex_on_a_pixel_centre_returns_its_own_colour():
    r = run([at(1, 1, 2.0), at(5, 1, 1.0), at(1, 5, 4.0)], [[0, 1, 2]])  # three depths: the weights are perspective-correct
    assert r.color_f32.dtype == np.float32 and r.color_f32.shape == (1, S, S, 3)
    for (i, j), k, mm in (((1, 1), 0, 2000), ((1, 5), 1, 1000), ((5, 1), 2, 4000)):
        assert np.array_equal(r.color_f32[0, i, j], RGB[k]) and r.depth[0, i, j] == mm
        assert np.array_equal(r.color_u8[0, i, j], np.rint(RGB[k].astype(np.float64) * 255.0).astype(np.uint8))
    # halfway along the edge from a (z = 2) to b (z = 1) ON SCREEN: 1 / z is linear there, z = 4 / 3, and the nearer end weighs 2 / 3
    la, lb = 0.5, 0.5
    zp = 1.0 / ((la / 2.0 + lb / 1.0) + 0.0 / 4.0)
    mid = ((la / 2.0) * zp) * RGB[0].astype(np.float64) + ((lb / 1.0) * zp) * RGB[1].astype(np.float64) + 0.0 * RGB[2].astype(np.float64)
    assert np.array_equal(r.color_f32[0, 1, 3], mid.astype(np.float32)) and r.depth[0, 1, 3] == 1333
    assert abs(float(r.color_f32[0, 1, 3, 0]) - (0.25 / 3 + 0.5 * 2 / 3)) < 1e-7


def test_the_nearer_face_wins_and_the_lowest_id_on_equal_depth():
    tri = lambda z: [at(1, 1, z), at(5, 1, z), at(1, 5, z)]
    r = run(tri(2.0) + tri(1.0), [[0, 1, 2], [3, 4, 5]])
    assert set(np.unique(r.face)) == {-1, 1} and set(np.unique(r.depth)) == {0, 1000}
    r = run(tri(1.0) + tri(2.0), [[0, 1, 2], [3, 4, 5]])
    assert set(np.unique(r.face)) == {-1, 0}
    r = run(tri(1.0) + tri(1.0), [[3, 4, 5], [0, 1, 2], [0, 1, 2]])      # the same depth thrice
    assert set(np.unique(r.face)) == {-1, 0}
    # two depths that round to one float32: the id decides, not the fp64 depth
    near = np.nextafter(1.0, 0.0)
    assert np.float32(near) == np.float32(1.0)
    r = run(tri(1.0) + tri(near), [[0, 1, 2], [3, 4, 5]])
    assert r.face[0, 2, 2] == 0 and run(tri(1.0) + tri(near), [[3, 4, 5], [3, 4, 5]]).face[0, 2, 2] == 0      # (both cover that centre)


def test_uint8_rounds_to_even_clamps_and_sends_nan_to_zero():
    got = RO.quantise(np.array([0.5, 0.25, 0.125, 1.0, 1.5, -0.25, np.nan, np.inf, -np.inf, 0.0, 0.5 + 2.0 ** -9], dtype=np.float32))
    assert got.tolist() == [128, 64, 32, 255, 255, 0, 0, 255, 0, 0, 128]  # 127.5 -> 128 (even), 63.75 -> 64, 31.875 -> 32
    C = np.array([[np.nan, 2.0, -1.0], [np.nan, 2.0, -1.0], [np.nan, 2.0, -1.0]], dtype=np.float32)
    r = run([at(1, 1), at(5, 1), at(1, 5)], [[0, 1, 2]], C=C)
    assert np.isnan(r.color_f32[0, 2, 2, 0]) and r.color_f32[0, 2, 2, 1:].tolist() == [2.0, -1.0]
    assert r.color_u8[0, 2, 2].tolist() == [0, 255, 0]
    assert r.color_u8[0, 7, 7].tolist() == [0, 0, 0]


def test_background_depth_zero_and_face_minus_one_where_nothing_is_covered():
    r = run([at(1, 1), at(5, 1), at(1, 5)], [[0, 1, 2]], background=(0.25, 0.5, 2.0))
    empty = r.face[0] == -1
    assert empty.sum() == S * S - 15 and (r.depth[0][empty] == 0).all()
    assert (r.color_f32[0][empty] == np.array([0.25, 0.5, 2.0], dtype=np.float32)).all()
    assert (r.color_u8[0][empty] == np.array([64, 128, 255], dtype=np.uint8)).all()
    # nothing at all: no faces, no vertices, a lost pose, a face across the near plane, a face with an index that does not exist
    for r in (run([at(1, 1), at(5, 1), at(1, 5)], np.zeros((0, 3))), run(np.zeros((0, 3)), np.zeros((0, 3)), C=np.zeros((0, 3))),
              run([at(1, 1), at(5, 1), [0.0, 0.0, 0.005]], [[0, 1, 2]]), run([at(1, 1), at(5, 1), at(1, 5)], [[0, 1, 3]])):
        assert (r.face == -1).all() and not r.depth.any() and not r.color_u8.any()
    assert run([at(1, 1), at(5, 1), at(1, 5)], [[0, 1, 3], [0, 1, 2]]).status == RO.BAD_INDEX
    lost = RO.render(np.asarray([at(1, 1), at(5, 1), at(1, 5)]), np.array([[0, 1, 2]]), RGB, np.full((1, 4, 4), -np.inf), CAM, S, S)
    assert (lost.face == -1).all()
    # depth outside the uint16 format is 0, the face is still there
    r = run([at(1, 1, 70.0), at(5, 1, 70.0), at(1, 5, 70.0)], [[0, 1, 2]])
    assert r.face[0, 2, 2] == 0 and r.depth[0, 2, 2] == 0
    assert run([at(1, 1, 65.534), at(5, 1, 65.534), at(1, 5, 65.534)], [[0, 1, 2]]).depth[0, 1, 1] == 65534


def test_result_colorings_match_hand_values():
    gt = torch.tensor([[0.0, 0.0, 0.0], [0.5, -0.5, 1.0], [-1.0, -1.0, -1.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    # d of the [0, 1] colours = half the mean difference of the [-1, 1] ones: 0.125, 0.25, 0.5, then 0.25 outside the mask, then 0
    pred = gt + torch.tensor([[0.25, 0.25, 0.25], [0.5, -0.5, -0.5], [1.0, 1.0, 1.0], [0.5, 0.5, 0.5], [0.0, 0.0, 0.0]])
    mask = torch.tensor([[1], [2], [1], [0], [1]])
    rgb = torch.rand(5, 3)
    out = views.result_colorings(pred, gt, mask, rgb=rgb)
    assert sorted(out) == ['diff', 'gt', 'mask', 'pred', 'rgb'] and all(v.dtype == torch.float32 and v.shape == (5, 3) for v in out.values())
    assert out['diff'].tolist() == [[0.0, 0.5, 0.5], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.25, 0.25, 0.25], [0.0, 0.0, 1.0]]
    assert out['gt'].tolist() == [[0.5, 0.5, 0.5], [0.75, 0.25, 1.0], [0.0, 0.0, 0.0], [0.5, 0.5, 0.5], [1.0, 1.0, 1.0]]
    assert out['pred'][0].tolist() == [0.625, 0.625, 0.625] and out['pred'][2].tolist() == [0.5, 0.5, 0.5]
    assert out['mask'].tolist() == [[0.0] * 3, [0.0] * 3, [0.0] * 3, [0.5, 0.5, 0.5], [0.0] * 3]
    assert torch.equal(out['rgb'], rgb) and 'rgb' not in views.result_colorings(pred, gt, mask)
    far = views.result_colorings(-torch.ones(1, 3), torch.ones(1, 3), torch.ones(1))['diff']          # d = 1: clamped, still red
    assert far.tolist() == [[1.0, 0.0, 0.0]]
    with pytest.raises(ValueError):
        views.result_colorings(pred, gt[:4], mask)


def chunks(blob):
    assert blob[:8] == b'\x89PNG\r\n\x1a\n'
    at_, out = 8, []
    while at_ < len(blob):
        n, = struct.unpack('>I', blob[at_:at_ + 4])
        tag, data = blob[at_ + 4:at_ + 8], blob[at_ + 8:at_ + 8 + n]
        crc, = struct.unpack('>I', blob[at_ + 8 + n:at_ + 12 + n])
        assert crc == zlib.crc32(tag + data) & 0xFFFFFFFF
        out.append((tag, data))
        at_ += 12 + n
    return out


def decode_png(path):
    """-> uint8 [H, W, channels] of a PNG of the kind write_png writes (8 bit, grey or RGB, filter 0, not interlaced)."""
    with open(path, 'rb') as f:
        parts = chunks(f.read())
    assert [t for t, _ in parts] == [b'IHDR', b'IDAT', b'IEND'] and parts[2][1] == b''
    w, h, bits, kind, compression, filt, interlace = struct.unpack('>IIBBBBB', parts[0][1])
    assert (bits, compression, filt, interlace) == (8, 0, 0, 0) and kind in (0, 2)
    ch = 1 if kind == 0 else 3
    rows = np.frombuffer(zlib.decompress(parts[1][1]), dtype=np.uint8).reshape(h, 1 + w * ch)
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(h, w, ch)


def test_write_png_decodes_to_the_same_pixels(tmp_path):
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    views.write_png(str(tmp_path / 'a.png'), rgb)
    assert np.array_equal(decode_png(str(tmp_path / 'a.png')), rgb)
    grey = rng.integers(0, 256, (6, 3), dtype=np.uint8)
    views.write_png(str(tmp_path / 'b.png'), torch.from_numpy(grey))
    assert np.array_equal(decode_png(str(tmp_path / 'b.png'))[:, :, 0], grey)
    views.write_png(str(tmp_path / 'c.png'), grey[:, :, None])
    assert np.array_equal(decode_png(str(tmp_path / 'c.png'))[:, :, 0], grey)
    with pytest.raises(TypeError):
        views.write_png(str(tmp_path / 'd.png'), rgb.astype(np.float32))
    with pytest.raises(ValueError):
        views.write_png(str(tmp_path / 'd.png'), np.zeros((4, 4, 2), dtype=np.uint8))


def test_write_ply_header_and_byte_count(tmp_path):
    V = np.array([at(1, 1), at(5, 1), at(1, 5), at(5, 5)], dtype=np.float64)
    F = np.array([[0, 1, 2], [1, 3, 2]])
    C = np.array([[0.5, 0.25, 1.0], [np.nan, 2.0, -1.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], dtype=np.float32)
    views.write_ply(str(tmp_path / 'm.ply'), torch.from_numpy(V), torch.from_numpy(F), torch.from_numpy(C))
    blob = (tmp_path / 'm.ply').read_bytes()
    header, body = blob[:blob.index(b'end_header\n') + 11], blob[blob.index(b'end_header\n') + 11:]
    assert header.decode('ascii').split('\n') == ['ply', 'format binary_little_endian 1.0', 'element vertex 4', 'property float x',
                                                   'property float y', 'property float z', 'property uchar red', 'property uchar green',
                                                   'property uchar blue', 'element face 2', 'property list uchar int vertex_indices',
                                                   'end_header', '']
    assert len(body) == 4 * (12 + 3) + 2 * (1 + 12)
    assert struct.unpack('<fffBBB', body[:15]) == (-0.625, -0.625, 1.0, 128, 64, 255)
    assert struct.unpack('<BBB', body[15 + 12:30]) == (0, 255, 0)
    assert struct.unpack('<Biii', body[60:73]) == (3, 0, 1, 2) and struct.unpack('<Biii', body[73:86]) == (3, 1, 3, 2)


NAMES = ('stin_render_workspace_bytes', 'stin_render_poses_f64')


def test_entry_points_are_declared_exported_and_check_their_arguments():
    lib = _lib.load()                                                    # no GPU needed for these calls: they return before a launch
    for name in NAMES:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    C = _lib.CONSTANTS
    assert (C['STIN_RENDER_BAD_INDEX'], C['STIN_RENDER_LARGE_FACE']) == (1, 2) and C['STIN_RENDER_LARGE_BOX'] >= 1
    assert C['STIN_RENDER_MAX_SIZE'] >= 1296 and C['STIN_RENDER_MAX_BATCH'] >= 64 and C['STIN_RENDER_CAMERA_DOUBLES'] == 4
    ws = lib.stin_render_workspace_bytes
    assert ws(200704, 399618, 480, 640, 16) >= 16 * 480 * 640 * 8 + 16 * 200704 * 24 + 399618 * 12
    assert ws(0, 0, 1, 1, 1) > 0
    assert ws(-1, 0, 8, 8, 1) == 0 and ws(0, -1, 8, 8, 1) == 0 and ws(0, 0, 0, 8, 1) == 0 and ws(0, 0, 8, 0, 1) == 0
    assert ws(0, 0, C['STIN_RENDER_MAX_SIZE'] + 1, 8, 1) == 0 and ws(0, 0, 8, C['STIN_RENDER_MAX_SIZE'] + 1, 1) == 0
    assert ws(0, 0, 8, 8, 0) == 0 and ws(0, 0, 8, 8, C['STIN_RENDER_MAX_BATCH'] + 1) == 0 and ws(2 ** 31 - 1, 0, 8, 8, 1) == 0
    E_NULL, E_SIZE, E_WS = C['STIN_E_NULL'], C['STIN_E_SIZE'], C['STIN_E_WORKSPACE']

    def render(N=0, F=0, K=3, P=0, H=8, W=8, z_near=0.01, scale=1000.0, batch=1, large_box=0, stages=0, camera=True, background=True,
               status=64, data=None, work=None, work_bytes=0):
        cam = (ctypes.c_double * 4)(*CAM) if camera else None
        bg = (ctypes.c_float * 4)(0.0, 0.0, 0.0, 0.0) if background else None
        return lib.stin_render_poses_f64(data, N, data, F, data, K, data, data, P, cam, H, W, z_near, scale, bg, batch, large_box, stages,
                                         None, None, None, None, status, work, work_bytes, None)
    assert render(H=0) == E_SIZE and render(W=C['STIN_RENDER_MAX_SIZE'] + 1) == E_SIZE and render(batch=0) == E_SIZE
    assert render(batch=C['STIN_RENDER_MAX_BATCH'] + 1) == E_SIZE and render(K=0) == E_SIZE and render(K=5) == E_SIZE
    assert render(z_near=0.0) == E_SIZE and render(scale=0.0) == E_SIZE and render(N=-1) == E_SIZE and render(P=-1) == E_SIZE
    assert render(N=2 ** 31 - 1) == E_SIZE and render(F=2 ** 31 - 1) == E_SIZE and render(stages=32) == E_SIZE
    assert render(status=None) == E_NULL and render(camera=False) == E_NULL and render(background=False) == E_NULL
    assert render(N=1) == E_NULL and render(F=1) == E_NULL and render(P=1) == E_NULL      # vertices, faces, poses are missing
    assert render() == E_WS and render(N=4, F=2, P=1, data=64) == E_WS                   # (the pointers are never followed)
    assert render(N=4, F=2, P=1, data=64, work=64, work_bytes=ws(4, 2, 8, 8, 1) - 1) == E_WS


def test_cpu_tensors_and_bad_arguments_are_refused():
    V = torch.zeros(4, 3, dtype=torch.float64)
    F = torch.zeros(2, 3, dtype=torch.int64)
    Cc = torch.zeros(4, 3)
    with pytest.raises(TypeError):
        views.render_mesh(V, F, Cc, EYE, CAM, S, S)
    with pytest.raises(TypeError):
        views.render_mesh(V.numpy(), F.numpy(), Cc.numpy(), EYE, CAM, S, S)
    with pytest.raises(ValueError):
        views.write_result_views('unused', 'scene', V, F, {}, poses=EYE)
