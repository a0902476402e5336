"""Result views on the GPU (csrc/stin_render.hip through views.render_mesh): equal to the numpy restatement of the contract
(tests/_render_oracle.py) byte for byte - `tobytes()` of the float32 and uint8 colour images, the depth images and the face ids - on
a sphere for every batch size and both rasteriser routes, at odd image sizes with 1 and 4 channels (also into output arrays without
16-byte alignment), with faces of a thousand pixels, and on degenerate inputs; against closed forms (an analytic wall's depth, its
shadow, a tilted quad's perspective-correct colours); chained into FrameColors and back to the vertex colours; and written out by
write_result_views."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import _render_oracle as RO
import _frames_oracle as FO
from surface_texture_inpainting_net_amd import _lib, preprocessing as P, views
from surface_texture_inpainting_net_amd.plan import _ptr, _stream
from test_render import decode_png

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

BAD, LARGE = _lib.CONSTANTS['STIN_RENDER_BAD_INDEX'], _lib.CONSTANTS['STIN_RENDER_LARGE_FACE']


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def run(V, F, C, poses, cam, H, W, **kw):
    """views.render_mesh twice (uint8 with depth and face ids, float32) -> (RO.Render of numpy arrays, status of the first call)."""
    v, f, c = dev(np.asarray(V, dtype=np.float64).reshape(-1, 3)), dev(np.asarray(F, dtype=np.int64).reshape(-1, 3)), dev(np.asarray(C, dtype=np.float32))
    K = 1 if c.dim() == 1 else int(c.shape[1])
    a = views.render_mesh(v, f, c, poses, cam, H, W, depth=True, face_ids=True, **kw)
    b = views.render_mesh(v, f, c, poses, cam, H, W, dtype=torch.float32, **kw)
    n = len(poses)
    assert a.color.is_cuda and a.color.dtype == torch.uint8 and a.color.shape == (n, H, W, K)
    assert b.dtype == torch.float32 and b.shape == (n, H, W, K)
    assert a.depth.dtype == torch.uint16 and a.depth.shape == (n, H, W) and a.face_ids.dtype == torch.int32 and a.face_ids.shape == (n, H, W)
    return RO.Render(host(b), host(a.color), host(a.depth), host(a.face_ids), a.status)


def same(got, want):
    assert got.face.tobytes() == want.face.tobytes()
    assert got.depth.tobytes() == want.depth.tobytes()
    assert got.color_f32.tobytes() == want.color_f32.tobytes()
    assert got.color_u8.tobytes() == want.color_u8.tobytes()
    assert got.status & BAD == want.status


# ------------------------------------------------------------------------------------------------------------------ 1: sphere
SPHERE_A = (120.0, 120.0, 128 / 2 - 0.5, 96 / 2 - 0.5)                   # 96 x 128
SPHERE_B = (60.0, 58.2, 64 / 2 - 0.5, 48 / 2 - 0.5)                      # 48 x 64: another size, fx != fy
SIZES = {'96x128': (SPHERE_A, 96, 128), '48x64': (SPHERE_B, 48, 64)}


@functools.lru_cache(maxsize=None)
def sphere():
    V, F = RO.icosphere(2, 3, jitter=0.0)
    V = V / np.linalg.norm(V, axis=1, keepdims=True)
    return V, F, (0.5 + 0.4 * V).astype(np.float32), RO.orbit(12, 3.0, 0.8)


@functools.lru_cache(maxsize=None)
def sphere_oracle(size):
    V, F, C, poses = sphere()
    cam, H, W = SIZES[size]
    return RO.render(V, F, C, poses, cam, H, W)


@pytest.mark.parametrize('size', sorted(SIZES))
@pytest.mark.parametrize('batch', [1, 5, 12])
@pytest.mark.parametrize('large_box', [1, None, 2 ** 40])
def test_sphere_equals_the_oracle_for_every_batch_and_route(size, batch, large_box):
    V, F, C, poses = sphere()
    assert V.shape == (162, 3) and F.shape == (320, 3)
    cam, H, W = SIZES[size]
    want = sphere_oracle(size)
    assert (want.face >= 0).any(axis=(1, 2)).all() and (want.face < 0).any()
    got = run(V, F, C, poses, cam, H, W, batch=batch, large_box=large_box)
    same(got, want)
    if large_box == 1:
        assert got.status & LARGE                                        # every face that reaches a centre went through the queue
    if large_box == 2 ** 40:
        assert not got.status & LARGE                                    # none did


# --------------------------------------------------------------------------------------------------------------- 2: odd sizes
def raw_render(V, F, C, poses, cam, H, W, shift, batch=2):
    """stin_render_poses_f64 with every output array `shift` ELEMENTS into its allocation: bases without 16-byte alignment."""
    lib = _lib.load()
    v, f, c = dev(np.asarray(V, dtype=np.float64)), dev(np.asarray(F, dtype=np.int64)), dev(np.asarray(C, dtype=np.float32).reshape(len(V), -1))
    K, n, N, nf = int(c.shape[1]), len(poses), len(V), len(F)
    RT, valid = P.pose_extrinsics(poses)
    rt_d, valid_d = dev(RT), dev(valid)
    bufs = [torch.full((n * H * W * k + shift,), fill, dtype=dt, device=DEV)
            for k, dt, fill in ((K, torch.float32, -7.0), (K, torch.uint8, 7), (1, torch.int16, 7), (1, torch.int32, 7))]
    ptrs = [b.data_ptr() + shift * b.element_size() for b in bufs]
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws_bytes = lib.stin_render_workspace_bytes(N, nf, H, W, batch)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    camera, bg = (ctypes.c_double * 4)(*cam), (ctypes.c_float * K)(*([0.25] * K))
    _lib.check(lib.stin_render_poses_f64(_ptr(v), N, _ptr(f), nf, _ptr(c), K, _ptr(rt_d), _ptr(valid_d), n, camera, H, W, 0.01, 1000.0, bg, batch,
                                         0, 0, ptrs[0], ptrs[1], ptrs[2], ptrs[3], _ptr(status), _ptr(ws), ws_bytes, _stream(v)),
               'stin_render_poses_f64')
    outs = [host(b) for b in bufs]
    assert (outs[0][:shift] == -7.0).all() and all((o[:shift] == 7).all() for o in outs[1:])          # nothing in front of the arrays moved
    return RO.Render(outs[0][shift:].reshape(n, H, W, K), outs[1][shift:].reshape(n, H, W, K), outs[2][shift:].view(np.uint16).reshape(n, H, W),
                     outs[3][shift:].reshape(n, H, W), int(status.item()))


@pytest.mark.parametrize('K', [1, 4])
def test_odd_image_sizes_and_channel_counts(K):
    V, F, C3, poses = sphere()
    poses = poses[:5]
    C = C3[:, 0].copy() if K == 1 else np.concatenate([C3, C3[:, :1] * 0.5], axis=1)
    cam, H, W = (90.0, 88.0, 46.0, 34.5), 70, 93                         # 6 510 pixels a pose: every batch starts inside a resolve tile
    bg = (0.25,) * K
    want = RO.render(V, F, C, poses, cam, H, W, background=bg)
    assert (want.face >= 0).any() and want.color_f32.shape == (5, H, W, K)
    same(run(V, F, C, poses, cam, H, W, batch=2, background=bg), want)
    same(run(V, F, C, poses, cam, H, W, batch=1, background=bg), want)
    same(raw_render(V, F, C, poses, cam, H, W, shift=1), want)           # no array is 16-byte aligned: the element-wise stores
    same(raw_render(V, F, C, poses, cam, H, W, shift=4), want)           # (only the float32 and int32 arrays are)


# ------------------------------------------------------------------------------------------------------------- 3: large faces
def through(pose, cam, u, v, z):
    """The world point that the camera-to-world `pose` sees at screen position (u, v) and depth z."""
    fx, fy, cx, cy = cam
    return pose[:3, :3] @ np.array([(u - cx) / fx * z, (v - cy) / fy * z, z]) + pose[:3, 3]


def test_faces_of_a_thousand_pixels_and_one_that_covers_none():
    ux, uy = (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
    V, F = RO.wall(6, 4.0, origin=(1.2, 0.0, 0.0), u=ux, v=uy)           # quads of 0.67 m at 1.2 m: 55 pixels a side
    cam, H, W = (100.0, 100.0, 159.5, 119.5), 240, 320
    poses = np.stack([RO.look_at((0, 0, 0), (1.2, 0, 0)), RO.look_at((0, 0.3, 0.2), (1.2, 0, 0)), RO.look_at((-0.2, -0.4, 0.1), (1.2, 0.2, 0))])
    tiny = np.stack([through(poses[0], cam, u, v, 1.0) for u, v in ((10.3, 10.3), (10.7, 10.3), (10.3, 10.7))])   # between four centres
    V, F = np.concatenate([V, tiny]), np.concatenate([F, [[len(V), len(V) + 1, len(V) + 2]]])
    C = (0.5 + 0.1 * V).astype(np.float32)
    want = RO.render(V, F, C, poses, cam, H, W)
    counts = np.bincount(want.face[0].ravel() + 1, minlength=len(F) + 1)[1:]
    assert (want.face[0] >= 0).all() and counts.max() > 1000 and counts[-1] == 0 and not (want.face == len(F) - 1).any()
    for large_box in (None, 1, 2 ** 40):
        same(run(V, F, C, poses, cam, H, W, large_box=large_box), want)


# ---------------------------------------------------------------------------------------------------- 4: against closed forms
UX, UY = (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
WALL_POSES = np.stack([RO.look_at((0, 0, 0), (2, 0, 0)), RO.look_at((0, 0.2, 0.1), (2, 0, 0)), RO.look_at((-0.3, -0.2, 0), (2, 0.1, 0))])
WALL_CAM = (60.0, 60.0, 31.5, 23.5)                                      # 48 x 64


def test_wall_depth_equals_the_analytic_depth_frames():
    """Checked on the CPU with the numpy oracle of this contract: 4 119 covered pixels with this camera, no mismatch."""
    V, F = RO.wall(4, 0.8, origin=(1.2, 0.0, 0.0), u=UX, v=UY)
    want = RO.render_walls(WALL_POSES, 48, 64, WALL_CAM, [((1.2, 0, 0), UX, UY, 0.8)])
    got = run(V, F, np.zeros((len(V), 3), dtype=np.float32), WALL_POSES, WALL_CAM, 48, 64)
    assert int((want > 0).sum()) == 4119 and np.array_equal(got.depth > 0, want > 0)
    assert int(np.abs(got.depth.astype(np.int64) - want.astype(np.int64)).max()) == 0
    assert np.array_equal(got.face >= 0, want > 0)


def test_the_near_wall_hides_the_far_one():
    near, Fn = RO.wall(4, 0.8, origin=(1.2, 0.0, 0.0), u=UX, v=UY)
    far, Ff = RO.wall(6, 3.0, origin=(2.0, 0.0, 0.0), u=UX, v=UY)
    V, F = np.concatenate([far, near]), np.concatenate([Ff, Fn + len(far)])          # the far wall's faces have the LOWER ids
    got = run(V, F, np.zeros((len(V), 3), dtype=np.float32), WALL_POSES, WALL_CAM, 48, 64)
    footprint = RO.render_walls(WALL_POSES, 48, 64, WALL_CAM, [((1.2, 0, 0), UX, UY, 0.8)]) > 0
    both = RO.render_walls(WALL_POSES, 48, 64, WALL_CAM, [((1.2, 0, 0), UX, UY, 0.8), ((2.0, 0, 0), UX, UY, 3.0)])
    assert footprint.sum() == 4119 and (got.face[footprint] >= len(Ff)).all()
    assert (got.face[~footprint & (both > 0)] < len(Ff)).all() and (got.face[~footprint & (both > 0)] >= 0).all()
    assert np.array_equal(got.depth, both)


def test_colours_are_interpolated_perspective_correctly():
    """A quad tilted 60 degrees to the view axis with the linear field c = 0.5 + 0.4 p on its corners: at every covered pixel the
    colour is the field at the ray's intersection with the quad's plane.  1e-6: the arithmetic is fp64 and the one rounding of size
    is the float32 cast of values in [0, 1] (6e-8), the corners' colours being rounded to float32 too (3e-8 each).  Interpolating in
    screen space instead misses by percent: the quad's far edge is 1.67 times as far as its near one."""
    t = np.radians(60.0)
    centre, e1, e2 = np.array([1.0, 0.0, 0.0]), np.array([np.cos(t), np.sin(t), 0.0]), np.array([0.0, 0.0, 1.0])
    V = np.stack([centre - 0.5 * e1 - 0.5 * e2, centre + 0.5 * e1 - 0.5 * e2, centre + 0.5 * e1 + 0.5 * e2, centre - 0.5 * e1 + 0.5 * e2])
    F = np.array([[0, 1, 2], [0, 2, 3]])
    C = (0.5 + 0.4 * V).astype(np.float32)
    pose, cam, H, W = RO.look_at((0, 0, 0), (1, 0, 0)), (60.0, 60.0, 31.5, 23.5), 48, 64
    got = run(V, F, C, pose[None], cam, H, W)
    covered = got.face[0] >= 0
    assert covered.sum() > 500
    rays = FO.rays(H, W, cam) @ pose[:3, :3].T                           # world directions through the centres, from the origin
    n = np.cross(e1, e2)
    s = (centre @ n) / (rays @ n)
    hit = s[:, :, None] * rays
    err = np.abs(got.color_f32[0].astype(np.float64) - (0.5 + 0.4 * hit))[covered]
    assert err.max() < 1e-6
    la = (hit - V[0]) @ e1                                               # and it is not the screen-space answer: depth varies over the quad
    assert (hit[covered][:, 0].max() / hit[covered][:, 0].min()) > 1.6 and la[covered].min() > -1e-9 and la[covered].max() < 1 + 1e-9


# --------------------------------------------------------------------------------------------------------------- 5: degenerate
def test_degenerate_inputs():
    V, F, C, poses = sphere()
    cam, H, W = SPHERE_B, 48, 64
    poses = poses[:3].copy()
    poses[1, 0, 3] = -np.inf                                             # tracking lost
    far = V * 0.5 + poses[0][:3, 3]                                      # a second sphere around the first camera: across its near plane
    V2 = np.concatenate([V, far])
    F2 = np.concatenate([F[:100], [[0, 1, len(V2)], [0, 1, -1]], F[100:], F + len(V)])
    C2 = np.concatenate([C, C])
    C2[F[sphere_oracle('48x64').face[2, H // 2, W // 2], 0]] = np.nan   # a corner of what the third camera sees at the image centre
    want = RO.render(V2, F2, C2, poses, cam, H, W, background=(0.5, 0.25, 1.0))
    got = run(V2, F2, C2, poses, cam, H, W, background=(0.5, 0.25, 1.0))
    same(got, want)
    assert got.status & BAD and (got.face[1] == -1).all() and (got.color_u8[1] == np.array([128, 64, 255], dtype=np.uint8)).all()
    assert (got.face[0] >= 0).any() and not np.isin(got.face, [100, 101]).any()
    touched = np.isnan(C2[:, 0])[F2[np.maximum(got.face, 0)]].any(axis=-1) & (got.face >= 0)
    assert touched.any() and np.isnan(got.color_f32[touched]).all() and not got.color_u8[touched].any()      # NaN colours -> 0
    # the first camera sits inside the second sphere: faces with a corner behind its near plane are dropped, not clipped
    Z = RO.screen(V2, P.pose_extrinsics(poses)[0][0], cam)[2]
    crossing = (Z[F2[102:]] < 0.01).any(axis=1) & (Z[F2[102:]] >= 0.01).any(axis=1)
    assert crossing.any() and not np.isin(got.face[0], 102 + np.flatnonzero(crossing)).any()
    # nothing to draw, nothing to draw on, nobody to look
    empty = run(V, np.zeros((0, 3)), C, poses, cam, H, W, background=(0.5, 0.25, 1.0))
    same(empty, RO.render(V, np.zeros((0, 3)), C, poses, cam, H, W, background=(0.5, 0.25, 1.0)))
    assert (empty.face == -1).all() and not empty.depth.any() and (empty.color_f32 == np.array([0.5, 0.25, 1.0], dtype=np.float32)).all()
    none = run(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), poses, cam, H, W)
    assert (none.face == -1).all() and not none.color_u8.any() and none.status == 0
    nobody = run(V, F, C, np.zeros((0, 4, 4)), cam, H, W)
    assert nobody.color_u8.shape == (0, H, W, 3) and nobody.face.shape == (0, H, W) and nobody.status == 0


# --------------------------------------------------------------------------------------------------------------- 6: round trip
ROUND_KW = dict(margin=2, discontinuity_threshold=0.5, half_kernel=3)


def test_rendered_frames_give_the_vertex_colours_back():
    """Render the sphere with C = 0.5 + 0.4 V, hand the uint8 colour and uint16 depth frames to FrameColors, compare with C.
    Measured on the CPU with the two numpy oracles chained (_render_oracle.render -> _frames_oracle.colors): 110 of the 162 vertices
    coloured, maximum error 0.003289 (0.84 grey levels); with 642 vertices 434 coloured and 0.002383.  The bound is twice the first
    figure; the margin covers nothing but a later change of scene constants."""
    V, F, C, poses = sphere()
    cam, H, W = SIZES['96x128']
    v, f, c = dev(V), dev(F), dev(C)
    frames = views.render_mesh(v, f, c, poses, cam, H, W, depth=True)
    colors, count = P.vertex_colors_from_frames(v, poses, frames.color, depth=frames.depth, color_camera=cam, depth_camera=cam, **ROUND_KW)
    fc = P.FrameColors(v, cam, cam, **ROUND_KW).add(poses, frames.color, depth=frames.depth)
    want = sphere_oracle('96x128')
    w_colors, w_count, _, w_sum = FO.colors(V, poses, want.color_u8, cam, depth=want.depth, depth_camera=cam, **ROUND_KW)
    assert host(fc.sum).tobytes() == w_sum.tobytes() and host(count).tobytes() == w_count.tobytes()          # (a)
    assert host(colors).tobytes() == w_colors.tobytes()
    lit = host(count) > 0                                                                                    # (b)
    assert int(lit.sum()) >= 100
    assert np.abs(host(colors)[lit].astype(np.float64) - C[lit].astype(np.float64)).max() <= 2 * 0.003289


# ------------------------------------------------------------------------------------------------------ 7: write_result_views
def test_write_result_views_writes_five_plys_and_sixty_pngs(tmp_path):
    V, F, C, poses = sphere()
    cam, H, W = SIZES['48x64']
    g = torch.Generator().manual_seed(3)
    gt = dev(C) * 2 - 1
    pred = (gt + 0.3 * torch.randn(gt.shape, generator=g).to(DEV)).clamp(-1, 1)
    mask = (torch.rand(len(V), 1, generator=g) < 0.5).to(DEV).long()
    colorings = views.result_colorings(pred, gt, mask, rgb=dev(C))
    assert sorted(colorings) == sorted(views.VIEWS) and all(t.is_cuda for t in colorings.values())
    written = views.write_result_views(str(tmp_path), 'scene0000_00', dev(V), dev(F), colorings, poses=poses, camera=cam, height=H, width=W)
    names = sorted(os.listdir(tmp_path))
    assert len(written) == len(names) == 65 and sorted(os.path.basename(w) for w in written) == names
    for view in views.VIEWS:
        ply = tmp_path / ('scene0000_00_%s.ply' % view)
        header = ply.read_bytes().split(b'end_header\n')[0]
        assert ply.stat().st_size == len(header) + 11 + 162 * 15 + 320 * 13
        for p in range(12):
            assert (tmp_path / ('scene0000_00_%s_%d.png' % (view, p))).stat().st_size > 60
    first = decode_png(str(tmp_path / 'scene0000_00_rgb_0.png'))
    assert first.shape == (H, W, 3)
    assert np.array_equal(first, host(views.render_mesh(dev(V), dev(F), dev(C), poses, cam, H, W))[0])
    assert np.array_equal(first, sphere_oracle('48x64').color_u8[0])
    only = views.write_result_views(str(tmp_path / 'plys'), 's', dev(V), dev(F), {'pred': colorings['pred']})
    assert [os.path.basename(p) for p in only] == ['s_pred.ply']
