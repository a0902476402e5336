"""Frame colours on the GPU (csrc/stin_frames.hip through preprocessing.FrameColors / vertex_colors_from_frames): equal to the numpy
restatement of the contract (tests/_frames_oracle.py) byte for byte - `tobytes()` of sum, count, seen, colours and edge bytes - on a
sphere and on two walls with analytic depth frames, for every batch size, order and both host routes of the accumulate kernel, in
observer-bits mode, for the depth-edge kernel alone, at ScanNet's frame sizes, on degenerate inputs, and chained into graph_levels."""
import functools

import numpy as np
import pytest
import torch

import _frames_oracle as FO
import _levels_oracle as LO
import _observers_oracle as OO
import _qem_oracle as QO
from surface_texture_inpainting_net_amd import _lib, preprocessing as P
from test_qem import SEED

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

OWNER, SPLIT = _lib.CONSTANTS['STIN_FRAMES_ROUTE_OWNER'], _lib.CONSTANTS['STIN_FRAMES_ROUTE_SPLIT']


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def run(V, poses, color, color_camera, depth=None, bits=None, fill=(0, 0, 0), **kw):
    """vertex_colors_from_frames -> (colours, count, seen, sum) as numpy arrays; the sums through a FrameColors of its own."""
    frames = dict(depth=None if depth is None else dev(depth), bits=None if bits is None else dev(bits))
    colors, count, seen = P.vertex_colors_from_frames(dev(V), poses, dev(color), color_camera=color_camera, fill=fill, return_seen=True,
                                                      **frames, **kw)
    assert colors.is_cuda and colors.dtype == torch.float32 and colors.shape == (len(V), 3)
    assert count.dtype == torch.int32 and count.shape == (len(V),)
    assert seen.dtype == torch.uint32 and seen.shape == (len(V), (len(poses) + 31) // 32)
    kw = {k: v for k, v in kw.items() if k not in ('batch', '_route')}
    fc = P.FrameColors(dev(V), color_camera, kw.pop('depth_camera', None), **kw)
    fc.add(poses, dev(color), **frames)
    return host(colors), host(count), host(seen), host(fc.sum)


def same(got, want):
    """got: run()'s tuple; want: FO.colors' tuple (colours, count, seen bool [N, P], sum)."""
    assert got[3].dtype == np.int64 and got[3].tobytes() == want[3].tobytes()
    assert got[1].tobytes() == want[1].tobytes()
    assert got[2].tobytes() == FO.pack_seen(want[2]).tobytes()
    assert got[0].tobytes() == want[0].tobytes()


# ------------------------------------------------------------------------------------------------------------------ 1: sphere
SPHERE_D = (120.0, 120.0, 128 / 2 - 0.5, 96 / 2 - 0.5)                   # depth frames 96 x 128
SPHERE_C = (60.0, 58.2, 64 / 2 - 0.5, 48 / 2 - 0.5)                      # colour frames 48 x 64: another size, fx != fy
SPHERE_KW = dict(margin=2, discontinuity_threshold=0.5, half_kernel=3)


@functools.lru_cache(maxsize=None)
def sphere():
    V, F = QO.icosphere(2, 3, jitter=0.0)
    V = V / np.linalg.norm(V, axis=1, keepdims=True)
    poses = OO.orbit(12, 3.0, 0.8)
    depth = FO.render_sphere(poses, 96, 128, SPHERE_D)
    color = np.random.default_rng(SEED).integers(0, 256, (12, 48, 64, 3), dtype=np.uint8)
    return V, F, poses, depth, color


def test_sphere_with_analytic_depth_parity_and_geometry():
    V, _, poses, depth, color = sphere()
    assert V.shape == (162, 3) and depth.dtype == np.uint16 and depth.any(axis=(1, 2)).all()
    want = FO.colors(V, poses, color, SPHERE_C, depth=depth, depth_camera=SPHERE_D, **SPHERE_KW)
    got = run(V, poses, color, SPHERE_C, depth=depth, depth_camera=SPHERE_D, **SPHERE_KW)
    same(got, want)
    to_eye = poses[None, :, :3, 3] - V[:, None, :]
    cos = (to_eye / np.linalg.norm(to_eye, axis=2, keepdims=True) * V[:, None, :]).sum(axis=2)      # the unit normal is the vertex
    seen = OO.unpack(got[2], 12)
    assert int((cos > 0.7).sum()) == 152 and seen[cos > 0.7].all()       # whoever faces the eye is seen
    assert not seen[cos < 0].any()                                       # nobody on the far side is
    assert int((got[1] > 0).sum()) == 112
    assert np.array_equal(seen.sum(axis=1), got[1])
    lit = got[1] > 0
    assert (got[0][lit] >= 0).all() and (got[0][lit] <= 1).all() and (got[0][~lit] == 0).all()


# --------------------------------------------------------------------------------------------------------------- 2: occlusion
def test_a_wall_hides_what_is_behind_it_and_not_what_is_beside_it():
    ux, uy = (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
    near, _ = OO.wall(4, 0.8, origin=(1.2, 0.0, 0.0), u=ux, v=uy)
    far, _ = OO.wall(6, 3.0, origin=(2.0, 0.0, 0.0), u=ux, v=uy)         # vertices every 0.5 m
    V = np.concatenate([near, far])
    poses = np.stack([OO.look_at((0, 0, 0), (2, 0, 0)), OO.look_at((0, 0.2, 0.1), (2, 0, 0)), OO.look_at((-0.3, -0.2, 0), (2, 0.1, 0))])
    d_cam, c_cam = (120.0, 120.0, 63.5, 47.5), (50.0, 50.0, 31.5, 23.5)
    depth = FO.render_walls(poses, 96, 128, d_cam, [((1.2, 0, 0), ux, uy, 0.8), ((2.0, 0, 0), ux, uy, 3.0)])
    assert set(np.unique(depth[0])) == {1200, 2000}
    color = np.random.default_rng(SEED + 1).integers(0, 256, (3, 48, 64, 3), dtype=np.uint8)
    kw = dict(depth=depth, depth_camera=d_cam, margin=2)
    got = run(V, poses, color, c_cam, **kw)
    same(got, FO.colors(V, poses, color, c_cam, **kw))
    seen0 = OO.unpack(got[2], 3)[:, 0]                                   # from the origin: the near wall's shadow on the far one is
    y, z = np.abs(far[:, 1]), np.abs(far[:, 2])                          # |y|, |z| < 0.8 / 2 * 2.0 / 1.2 = 0.667
    behind, beside = (y < 0.6) & (z < 0.6), (np.abs(y - 1.0) < 1e-9) & (z < 0.6)
    assert behind.sum() == 9 and beside.sum() == 6
    assert not seen0[len(near):][behind].any() and seen0[len(near):][beside].all()
    inner = (np.abs(near[:, 1]) < 0.3) & (np.abs(near[:, 2]) < 0.3)     # the near wall itself, away from its rim
    assert inner.sum() == 9 and seen0[:len(near)][inner].all()


# ------------------------------------------------------------------------------------------------------ 3: batching and order
MANY_D = MANY_C = (20.0, 20.0, 7.5, 7.5)
MANY_KW = dict(margin=1, discontinuity_threshold=1.0, half_kernel=1, max_depth=4.0, depth_threshold=0.05)   # 16 x 16: coarse


@functools.lru_cache(maxsize=None)
def many_poses():
    """42 vertices, 70 poses of which one is lost, 16 x 16 frames of both kinds; the restatement once, for all tests."""
    V, _ = QO.icosphere(1, 5)
    assert V.shape[0] == 42
    poses = np.concatenate([OO.orbit(35, 3.0, 0.8), OO.orbit(35, 2.5, -1.2, phase=0.4)])
    poses[5] = -np.inf
    depth = FO.render_sphere(poses, 16, 16, MANY_D)
    color = np.random.default_rng(SEED + 2).integers(0, 256, (70, 16, 16, 3), dtype=np.uint8)
    want = FO.colors(V, poses, color, MANY_C, depth=depth, depth_camera=MANY_D, **MANY_KW)
    assert want[2][:, :35].any() and want[2][:, 35:].any() and int(want[1].max()) >= 6      # poses of several chunks add to one vertex
    return V, poses, depth, color, want


@pytest.mark.parametrize('batch', [1, 32, 33, 64, 70])
def test_every_batch_size_gives_the_same_bytes(batch):
    V, poses, depth, color, want = many_poses()
    got = run(V, poses, color, MANY_C, depth=depth, depth_camera=MANY_D, batch=batch, **MANY_KW)
    same(got, want)
    assert got[2].shape[1] == 3 and not OO.unpack(got[2], 70)[:, 5].any()            # three words; the lost pose saw nothing


@pytest.mark.parametrize('route', [OWNER, SPLIT])
@pytest.mark.parametrize('batch', [7, 70])
def test_both_routes_of_the_accumulate_kernel_give_the_same_bytes(route, batch):
    V, poses, depth, color, want = many_poses()
    same(run(V, poses, color, MANY_C, depth=depth, depth_camera=MANY_D, batch=batch, _route=route, **MANY_KW), want)


def test_batches_in_reverse_order_and_uneven_sizes_give_the_same_bytes():
    V, poses, depth, color, want = many_poses()
    fc = P.FrameColors(dev(V), MANY_C, MANY_D, num_poses=70, **MANY_KW)
    d, c = dev(depth), dev(color)
    cuts = [0, 3, 4, 36, 64, 70]
    for p0, p1 in reversed(list(zip(cuts[:-1], cuts[1:]))):
        fc.add(poses[p0:p1], c[p0:p1], depth=d[p0:p1], first_pose=p0)
    colors, count = fc.result()
    same((host(colors), host(count), host(fc.seen), host(fc.sum)), want)
    again, _ = fc.result(fill=(1, 1, 1))                                  # result() reads the sums, it does not consume them
    assert torch.equal(again[count > 0], colors[count > 0]) and (again[count == 0] == 1).all()


# ------------------------------------------------------------------------------------------------------- 4: observer-bits mode
def test_observer_bits_take_the_place_of_depth_frames():
    V, F, poses, _, color = sphere()
    cam = dict(fx=1170.19, fy=1165.37, width=1296, height=968)
    want_bits, _, _ = OO.observe(V, F, poses, image_size=32, **cam)
    bits, _ = P.observe_vertices(dev(V), dev(F), poses, image_size=32, **cam)
    want = FO.colors(V, poses, color, SPHERE_C, bits=want_bits, margin=2)
    colors, count, seen = P.vertex_colors_from_frames(dev(V), poses, dev(color), bits=bits, color_camera=SPHERE_C, margin=2,
                                                      return_seen=True, batch=5)
    fc = P.FrameColors(dev(V), SPHERE_C, margin=2).add(poses, dev(color), bits=bits)
    same((host(colors), host(count), host(seen), host(fc.sum)), want)
    assert host(count).sum() > 0
    assert not (host(seen) & ~host(bits)).any()                           # seen is a subset of bits


# ---------------------------------------------------------------------------------------------------- 5: the depth-edge kernel
def random_depth(B, H, W, seed):
    rng = np.random.default_rng(seed)
    base = rng.integers(988, 1013, (B, H, W))                            # a wall with sensor noise: |g| stays below T = 100
    for value, share in ((0, 0.002), (65535, 0.001), (None, 0.003)):    # holes, the 65535 the reference zeroes, and jumps, some
        hit = rng.random((B, H, W)) < share                              # beyond depth_trunc: islands of edges that the windows grow
        base = np.where(hit, rng.integers(1100, 3400, (B, H, W)) if value is None else value, base)
    if H > 1:
        base[:, H // 2, W // 2], base[:, 0, W - 1] = 0, 65535            # one of each also in the smallest image
    return base.astype(np.uint16)


@pytest.mark.parametrize('half_kernel', [0, 1, 3, 15])
@pytest.mark.parametrize('shape', [(3, 1, 1), (3, 7, 5), (2, 33, 65), (1, 480, 640)])
def test_depth_edges_alone(shape, half_kernel):
    raw = random_depth(*shape, seed=SEED + shape[1])
    fc = P.FrameColors(torch.zeros(0, 3, dtype=torch.float64, device=DEV), (1.0, 1.0, 0.0, 0.0), half_kernel=half_kernel)
    edge = fc.depth_edges(dev(raw))
    assert edge.dtype == torch.uint8 and edge.shape == shape
    want = FO.depth_edges(raw, half_kernel=half_kernel)
    assert host(edge).tobytes() == want.tobytes()
    if shape[1] > 7 and half_kernel <= 3:
        assert 0 < want.mean() < 1                                       # both answers occur


def test_depth_edges_with_other_parameters():
    raw = random_depth(2, 33, 65, seed=SEED)
    for kw in (dict(depth_trunc=1.05, half_kernel=2), dict(discontinuity_threshold=0.04, half_kernel=0),     # T inside the noise
               dict(depth_scale=500.0, half_kernel=1), dict(depth_trunc=float('inf'), half_kernel=2)):
        fc = P.FrameColors(torch.zeros(0, 3, dtype=torch.float64, device=DEV), (1.0, 1.0, 0.0, 0.0), **kw)
        want = FO.depth_edges(raw, **kw)
        assert 0 < want.mean() < 1 and host(fc.depth_edges(dev(raw))).tobytes() == want.tobytes(), kw


# ------------------------------------------------------------------------------------------------- 6: ScanNet's frame sizes
SCAN_D = (577.87, 577.87, 640 / 2 - 0.5, 480 / 2 - 0.5)
SCAN_C = (1170.19, 1165.37, 1296 / 2 - 0.5, 968 / 2 - 0.5)


def render_height_field(poses, H, W, cam, lo, hi):
    """z-depth (uint16 mm) of the surface z = 0.4 sin(1.3 x) cos(0.9 y) - LO.grid_mesh without its noise - over [lo, hi]: Newton
    on the ray parameter (the camera-space direction has z = 1, so the parameter is the z-depth)."""
    D = FO.rays(H, W, cam).reshape(-1, 3)
    out = np.zeros((len(poses), H * W), dtype=np.uint16)
    for p, pose in enumerate(poses):
        d, e = D @ pose[:3, :3].T, pose[:3, 3]
        t = np.full(len(D), e[2] / max(-d[:, 2].mean(), 1e-3))
        for _ in range(4):
            x, y = e[0] + t * d[:, 0], e[1] + t * d[:, 1]
            sx, cx, sy, cy = np.sin(1.3 * x), np.cos(1.3 * x), np.sin(0.9 * y), np.cos(0.9 * y)
            g = e[2] + t * d[:, 2] - 0.4 * sx * cy
            dg = d[:, 2] - 0.4 * (1.3 * cx * cy * d[:, 0] - 0.9 * sx * sy * d[:, 1])
            t = t - g / dg
        x, y = e[0] + t * d[:, 0], e[1] + t * d[:, 1]
        ok = (x >= lo[0]) & (x <= hi[0]) & (y >= lo[1]) & (y <= hi[1]) & (np.abs(g) < 1e-6)
        out[p] = FO.millimetres(np.where(ok, t, np.inf))
    return out.reshape(len(poses), H, W)


@functools.lru_cache(maxsize=None)
def scan():
    """The 400-vertex height field under 8 cameras at ScanNet's sizes, the restatement and the GPU's answer once."""
    m = LO.grid_mesh(20, SEED)
    V = m['vertices']
    lo, hi = V.min(axis=0), V.max(axis=0)
    eyes = [(1.2, 1.2, 1.9), (3.6, 1.2, 2.0), (1.2, 3.6, 1.8), (3.6, 3.6, 2.1), (2.4, 2.4, 2.2), (2.0, 3.0, 1.7), (3.0, 2.0, 1.9), (2.4, 1.0, 2.0)]
    poses = np.stack([OO.look_at(e, (e[0] + 0.2 * np.cos(i), e[1] + 0.2 * np.sin(i), 0.0)) for i, e in enumerate(eyes)])
    depth = render_height_field(poses, 480, 640, SCAN_D, lo, hi)
    color = np.random.default_rng(SEED + 3).integers(0, 256, (8, 968, 1296, 3), dtype=np.uint8)
    want = FO.colors(V, poses, color, SCAN_C, depth=depth, depth_camera=SCAN_D)
    got = run(V, poses, color, SCAN_C, depth=depth, depth_camera=SCAN_D)
    return m, poses, depth, color, want, got


def test_frame_size_parity_with_default_parameters():
    m, poses, depth, color, want, got = scan()
    assert m['vertices'].shape == (400, 3) and depth.shape == (8, 480, 640) and color.shape == (8, 968, 1296, 3)
    same(got, want)
    # the vertices carry noise of sigma = 2 cm around the rendered surface and the test is at 3 cm: most of those in view pass
    assert int((want[1] > 0).sum()) >= 100 and int(want[1].max()) >= 2


def test_frame_size_identity_of_two_runs_and_of_both_routes():
    m, poses, depth, color, _, got = scan()
    for route in (None, OWNER, SPLIT):
        again = run(m['vertices'], poses, color, SCAN_C, depth=depth, depth_camera=SCAN_D, _route=route)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, got)), route


# --------------------------------------------------------------------------------------------------------- 7: degenerate inputs
def test_degenerate_inputs():
    V, _, poses, depth, color = sphere()
    fill = (0.25, 0.5, 0.75)
    kw = dict(depth=depth, depth_camera=SPHERE_D, fill=fill, **SPHERE_KW)
    base = run(V, poses, color, SPHERE_C, **kw)
    # no vertices
    got = run(V[:0], poses, color, SPHERE_C, **kw)
    assert got[0].shape == (0, 3) and got[1].shape == (0,) and got[3].shape == (0, 3)
    # no poses
    got = run(V, poses[:0], color[:0], SPHERE_C, **dict(kw, depth=depth[:0]))
    assert (got[0] == np.asarray(fill, dtype=np.float32)).all() and not got[1].any() and got[2].shape == (162, 0)
    # every pose lost
    got = run(V, np.full((12, 4, 4), -np.inf), color, SPHERE_C, **kw)
    assert (got[0] == np.asarray(fill, dtype=np.float32)).all() and not got[1].any() and not got[2].any() and not got[3].any()
    # vertices that are not finite get the fill colour; the others are unaffected
    W = V.copy()
    W[3, 0], W[50, 1], W[99, 2], W[120] = np.nan, np.inf, -np.inf, np.nan
    bad = [3, 50, 99, 120]
    got = run(W, poses, color, SPHERE_C, **kw)
    same(got, FO.colors(W, poses, color, SPHERE_C, **{k: v for k, v in kw.items()}))
    keep = np.setdiff1d(np.arange(162), bad)
    assert (got[0][bad] == np.asarray(fill, dtype=np.float32)).all() and not got[1][bad].any()
    assert all(g[keep].tobytes() == b[keep].tobytes() for g, b in zip(got, base))
    # wrong arguments are refused before anything runs
    fc = P.FrameColors(dev(V), SPHERE_C, SPHERE_D, num_poses=12)
    with pytest.raises(ValueError):
        fc.add(poses, dev(color))                                        # neither depth nor bits
    with pytest.raises(ValueError):
        fc.add(poses, dev(color), depth=dev(depth), bits=torch.zeros(162, 1, dtype=torch.int32, device=DEV).view(torch.uint32))
    with pytest.raises(ValueError):
        fc.add(poses, dev(color[:5]), depth=dev(depth))
    with pytest.raises(ValueError):
        fc.add(poses, dev(color), depth=dev(depth), first_pose=1)        # pose 12 of 12
    with pytest.raises(TypeError):
        fc.add(poses, dev(color).float(), depth=dev(depth))
    with pytest.raises(TypeError):
        fc.add(poses, dev(color), depth=dev(depth.astype(np.int32)))
    assert not fc.count.any()


# --------------------------------------------------------------------------------------------------------------------- 8: chain
def test_the_colours_go_into_graph_levels_as_the_mesh_colours():
    m, _, _, _, _, got = scan()
    colors = dev(got[0])
    mesh = dict(vertices=dev(m['vertices']), faces=dev(m['faces']), colors=colors, normals=dev(m['normals']))
    out = P.graph_levels(mesh, [0.5], [0], [])
    level0 = out['vertices'][0]                                          # position, colour, normal, index of the nearest original vertex
    assert level0.shape[1] == 10 and 0 < level0.shape[0] < 400
    index = level0[:, 9].long()
    assert torch.equal(level0[:, 3:6], colors[index])
    assert (level0[:, 3:6] != 0).any()
