"""Frame colours, the part that needs no GPU: the numpy restatement of the contract (tests/_frames_oracle.py) on 8 x 8 frames with an
identity pose, where every expected value can be written down by hand; `frame_intrinsics`; the entry points' declarations, their
argument checks (which return before anything is launched) and their refusal of CPU tensors."""
import ctypes

import numpy as np
import pytest
import torch

import _frames_oracle as FO
from surface_texture_inpainting_net_amd import _lib, preprocessing as P

S = 8
CAM = (4.0, 4.0, 3.5, 3.5)                                               # u = 4 x / z + 3.5: exact for the dyadic values used here
EYE = np.eye(4)[None]                                                    # at the origin, +z forward, +x right, +y down the rows
RNG = np.random.default_rng(11)
COLOR = RNG.integers(0, 256, (1, S, S, 3), dtype=np.uint8)
FLAT = np.full((1, S, S), 1000, dtype=np.uint16)                         # a wall at 1 m: no discontinuity anywhere
ALL = np.full((1, 1), 0xFFFFFFFF, dtype=np.uint32)                       # observer bits: every pose sees the (one) vertex


def at(u, v, z=1.0):
    """The point that projects to (u, v) at depth z through CAM."""
    return [(u - 3.5) / 4.0 * z, (v - 3.5) / 4.0 * z, z]


def run(V, color_camera=CAM, depth=FLAT, poses=EYE, color=COLOR, **kw):
    kw.setdefault('margin', 0)
    if depth is not None:
        kw.update(depth=depth, depth_camera=CAM)
    total, count, seen = FO.accumulate(np.asarray(V, dtype=np.float64).reshape(-1, 3), poses, color, color_camera, **kw)
    return total, count, seen


def test_a_vertex_on_a_pixel_centre_returns_that_pixel():
    total, count, seen = run([at(2, 5), at(7, 0), at(0, 7)])
    assert count.tolist() == [1, 1, 1] and seen.all()
    assert total[0].tolist() == (65536 * COLOR[0, 5, 2].astype(np.int64)).tolist()
    assert total[1].tolist() == (65536 * COLOR[0, 0, 7].astype(np.int64)).tolist()      # the last column: x1 is clamped, a = 0
    assert total[2].tolist() == (65536 * COLOR[0, 7, 0].astype(np.int64)).tolist()
    colours, observed = FO.finish(total, count)
    assert observed.all() and colours.dtype == np.float32
    assert np.array_equal(colours[0], (COLOR[0, 5, 2].astype(np.float64) / 255.0).astype(np.float32))


def test_a_vertex_between_four_pixels_returns_their_mean():
    total, count, _ = run([at(2.5, 4.5)])
    four = COLOR[0, 4:6, 2:4].astype(np.int64).reshape(4, 3).sum(axis=0)
    assert count.tolist() == [1] and total[0].tolist() == (16384 * four).tolist()
    total, _, _ = run([at(2.25, 4.0)])                                   # a quarter of the way along a row
    want = 49152 * COLOR[0, 4, 2].astype(np.int64) + 16384 * COLOR[0, 4, 3].astype(np.int64)
    assert total[0].tolist() == want.tolist()


def test_the_margin_is_inclusive_and_the_next_value_outside_is_not():
    V = [[0.0, 0.0, 1.0]]                                                # u = cx and v = cy of the colour camera, exactly
    for inside, outside in ((2.0, np.nextafter(2.0, 0.0)), (5.0, np.nextafter(5.0, 9.0))):
        for cam_in, cam_out in (((4.0, 4.0, inside, 3.5), (4.0, 4.0, outside, 3.5)), ((4.0, 4.0, 3.5, inside), (4.0, 4.0, 3.5, outside))):
            assert run(V, color_camera=cam_in, margin=2)[1].tolist() == [1]
            assert run(V, color_camera=cam_out, margin=2)[1].tolist() == [0]
            assert run(V, color_camera=cam_out, margin=1)[1].tolist() == [1]
    assert run(V, color_camera=(4.0, 4.0, 0.0, 7.0), margin=0)[1].tolist() == [1]         # margin 0: the outermost centres count
    assert run(V, color_camera=(4.0, 4.0, np.nextafter(7.0, 8.0), 7.0), margin=0)[1].tolist() == [0]
    assert run(V, color_camera=(4.0, 4.0, -np.nextafter(0.0, 1.0), 7.0), margin=0)[1].tolist() == [0]   # the smallest u below 0
    assert run(V, color_camera=CAM, margin=4)[1].tolist() == [0]          # margin > Wc - 1 - margin: nothing can pass


def test_a_vertex_nearer_than_z_near_is_skipped():
    below = np.nextafter(0.01, 0.0)
    _, count, _ = run([[0.0, 0.0, 0.01], [0.0, 0.0, below], [0.0, 0.0, -1.0], [0.0, 0.0, 0.0]], depth=None, bits=np.repeat(ALL, 4, axis=0))
    assert count.tolist() == [1, 0, 0, 0]


def test_the_depth_test_is_strict_at_three_centimetres():
    _, count, _ = run([at(3, 3, 1.031), at(3, 3, 1.029), at(4, 4, 0.971), at(4, 4, 0.969), at(2, 2, 1.0)])
    assert count.tolist() == [0, 1, 1, 0, 1]
    _, count, _ = run([at(3, 3, 1.031), at(3, 3, 1.06)], depth_threshold=0.05)
    assert count.tolist() == [1, 0]


def test_missing_far_and_truncated_depth_is_not_seen():
    def one(raw, z, **kw):
        return run([at(3, 3, z)], depth=np.full((1, S, S), raw, dtype=np.uint16), **kw)[1].tolist()
    assert one(0, 0.02) == [0] and one(0, 0.02, depth_threshold=1.0) == [0]           # 0 is "no measurement", not "0 metres"
    assert one(2500, 2.5) == [1] and one(2501, 2.501) == [0]                          # !(d > max_depth)
    assert one(2501, 2.501, max_depth=2.6) == [1]
    assert one(3000, 3.0, max_depth=10.0) == [1] and one(3001, 3.001, max_depth=10.0) == [0]     # raw / scale > depth_trunc -> 0
    assert one(3001, 3.001, max_depth=10.0, depth_trunc=4.0) == [1]
    assert one(65535, 65.535, max_depth=100.0) == [0]                                 # the 65535 the reference zeroes


def test_a_depth_step_is_flagged_where_the_sobel_support_and_the_dilation_reach():
    raw = np.full((1, S, S), 1000, dtype=np.uint16)
    raw[:, :, 4:] = 2000                                                 # 1 m step between columns 3 and 4: |gx| = 4000 > T = 100 there
    for k, columns in ((0, [3, 4]), (1, [2, 3, 4, 5]), (2, [1, 2, 3, 4, 5, 6]), (3, list(range(8)))):
        edge = FO.depth_edges(raw, half_kernel=k)
        want = np.zeros((1, S, S), dtype=np.uint8)
        want[:, :, columns] = 1
        assert edge.dtype == np.uint8 and np.array_equal(edge, want), k
    # a 2 cm step: |gx| = 80 <= T; in Sobel units the default threshold passes steps up to 2.5 cm
    raw[:, :, 4:] = 1020
    assert not FO.depth_edges(raw, half_kernel=3).any()
    raw[:, :, 4:] = 1026
    assert FO.depth_edges(raw, half_kernel=0)[0, :, 3:5].all()
    # one pixel alone: the 3 x 3 support, then the window, clipped at the image's corner
    raw = np.full((1, S, S), 1000, dtype=np.uint16)
    raw[0, 0, 0] = 2000
    e0 = FO.depth_edges(raw, half_kernel=0)[0]
    assert e0[:2, :2].all() and e0.sum() == 4                            # clamped indices: the corner pixel is its own neighbour
    e1 = FO.depth_edges(raw, half_kernel=1)[0]
    assert e1[:3, :3].all() and e1.sum() == 9
    # a measurement beyond depth_trunc is 0 BEFORE the gradient: the hole's rim is an edge
    raw = np.full((1, S, S), 1000, dtype=np.uint16)
    raw[0, 4, 4] = 3001
    assert FO.depth_edges(raw, half_kernel=0)[0, 3:6, 3:6].sum() == 8 and not FO.depth_edges(raw, half_kernel=0, depth_trunc=4.0)[0, 0, 0]


def test_a_vertex_next_to_a_depth_step_is_not_coloured():
    raw = np.full((1, S, S), 1000, dtype=np.uint16)
    raw[:, :, 4:] = 2000
    V = [at(0, 3, 1.0), at(2, 3, 1.0), at(5, 3, 2.0), at(7, 3, 2.0)]
    assert run(V, depth=raw, half_kernel=0)[1].tolist() == [1, 1, 1, 1]
    assert run(V, depth=raw, half_kernel=1)[1].tolist() == [1, 0, 0, 1]
    assert run(V, depth=raw, half_kernel=3)[1].tolist() == [0, 0, 0, 0]


def test_the_nearest_depth_pixel_is_taken_with_ties_to_even():
    raw = np.full((1, S, S), 1000, dtype=np.uint16)
    raw[0, 3, 2] = 0                                                     # (u, v) = (2.5, 3): rint -> column 2, a hole
    assert run([at(2.5, 3.0)], depth=raw, half_kernel=0, discontinuity_threshold=1e9)[1].tolist() == [0]
    raw = np.full((1, S, S), 1000, dtype=np.uint16)
    raw[0, 3, 3] = 0                                                     # column 3 is not the one looked at
    assert run([at(2.5, 3.0)], depth=raw, half_kernel=0, discontinuity_threshold=1e9)[1].tolist() == [1]
    assert run([at(3.5, 3.0)], depth=raw, half_kernel=0, discontinuity_threshold=1e9)[1].tolist() == [1]   # 3.5 -> 4
    wide = (2.0, 2.0, 3.5, 3.5)                                          # a colour camera that still holds both: only the depth test fails
    assert run([at(7.75, 3.0), at(-0.75, 3.0)], color_camera=wide)[1].tolist() == [0, 0]     # rint lands outside the depth image
    assert run([at(7.25, 3.0), at(-0.25, 3.0)], color_camera=wide)[1].tolist() == [1, 1]


def test_a_lost_pose_contributes_nothing_and_sums_add_over_poses():
    lost = np.full((1, 4, 4), -np.inf)
    poses = np.concatenate([EYE, lost, EYE])
    color = RNG.integers(0, 256, (3, S, S, 3), dtype=np.uint8)
    depth = np.repeat(FLAT, 3, axis=0)
    total, count, seen = run([at(2, 5)], poses=poses, color=color, depth=depth)
    assert count.tolist() == [2] and seen.tolist() == [[True, False, True]]
    assert total[0].tolist() == (65536 * (color[0, 5, 2].astype(np.int64) + color[2, 5, 2])).tolist()
    colours, _ = FO.finish(total, count)
    mean = (color[0, 5, 2].astype(np.float64) + color[2, 5, 2]) * 65536.0 / (2 * 16711680.0)
    assert np.array_equal(colours[0], mean.astype(np.float32))
    assert FO.pack_seen(seen).tolist() == [[5]]
    # in two batches, in the other order, into the same sums
    into = FO.accumulate(np.asarray([at(2, 5)]), poses[2:], color[2:], CAM, depth=depth[2:], depth_camera=CAM, margin=0, first_pose=2)
    again = FO.accumulate(np.asarray([at(2, 5)]), poses[:2], color[:2], CAM, depth=depth[:2], depth_camera=CAM, margin=0, into=into)
    assert np.array_equal(again[0], total) and np.array_equal(again[1], count) and np.array_equal(again[2], seen)


def test_unseen_vertices_get_the_fill_colour():
    total, count, _ = run([at(2, 5), at(3, 3, 5.0), [np.nan, 0.0, 1.0], [np.inf, 0.0, 1.0]])
    colours, observed = FO.finish(total, count, fill=(0.25, 0.5, 1.0))
    assert count.tolist() == [1, 0, 0, 0] and observed.tolist() == [True, False, False, False]
    assert colours[1:].tolist() == [[0.25, 0.5, 1.0]] * 3 and (colours[0] <= 1.0).all()


def test_observer_bits_select_the_poses():
    bits = np.array([[0b101], [0b010]], dtype=np.uint32)
    poses = np.repeat(EYE, 3, axis=0)
    color = RNG.integers(0, 256, (3, S, S, 3), dtype=np.uint8)
    _, count, seen = run([at(2, 5), at(2, 5)], poses=poses, color=color, depth=None, bits=bits)
    assert count.tolist() == [2, 1] and seen.tolist() == [[True, False, True], [False, True, False]]


def test_frame_intrinsics_are_the_four_formulas():
    ic = np.array([[1170.19, 0.0, 647.75, 0.0], [0.0, 1165.37, 483.75, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    fx, fy, cx, cy = P.frame_intrinsics(ic, 1296, 968, 640, 480)
    assert (fx, fy, cx, cy) == (1170.19 * 640 / 1296, 1165.37 * 480 / 968, 640 / 2 - 0.5, 480 / 2 - 0.5)
    assert P.frame_intrinsics(torch.from_numpy(ic), 1296, 968, 1296, 968) == (1170.19, 1165.37, 647.5, 483.5)
    assert all(isinstance(v, float) for v in (fx, fy, cx, cy))


NAMES = ('stin_frames_edges_workspace_bytes', 'stin_frames_depth_edges_u16', 'stin_frames_accumulate_f64', 'stin_frames_finish_f32')


def test_entry_points_are_declared_exported_and_check_their_arguments():
    lib = _lib.load()                                                    # no GPU needed for these calls: they return before a launch
    for name in NAMES:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    C = _lib.CONSTANTS
    assert (C['STIN_FRAMES_ROUTE_AUTO'], C['STIN_FRAMES_ROUTE_OWNER'], C['STIN_FRAMES_ROUTE_SPLIT']) == (0, 1, 2)
    assert C['STIN_FRAMES_MAX_HALF_KERNEL'] >= 3 and C['STIN_FRAMES_MAX_SIZE'] >= 1296 and C['STIN_FRAMES_MAX_BATCH'] >= 64
    assert lib.stin_frames_edges_workspace_bytes(64, 480, 640) >= 64 * 480 * 640
    assert lib.stin_frames_edges_workspace_bytes(1, 0, 640) == 0 and lib.stin_frames_edges_workspace_bytes(-1, 4, 4) == 0
    assert lib.stin_frames_edges_workspace_bytes(1, C['STIN_FRAMES_MAX_SIZE'] + 1, 4) == 0
    E_NULL, E_SIZE, E_WS, E_UNSUPPORTED = C['STIN_E_NULL'], C['STIN_E_SIZE'], C['STIN_E_WORKSPACE'], C['STIN_E_UNSUPPORTED']
    edges = lib.stin_frames_depth_edges_u16
    assert edges(None, 0, 8, 8, 1000.0, 3.0, 0.1, 3, None, None, 0, None) == 0          # B = 0: nothing to do, null pointers allowed
    assert edges(None, 1, 8, 8, 1000.0, 3.0, 0.1, 3, None, None, 0, None) == E_NULL
    assert edges(None, 1, 8, 8, 1000.0, 3.0, 0.1, -1, None, None, 0, None) == E_SIZE
    assert edges(None, 1, 8, 8, 1000.0, 3.0, 0.1, C['STIN_FRAMES_MAX_HALF_KERNEL'] + 1, None, None, 0, None) == E_SIZE
    assert edges(None, 1, 8, 8, 0.0, 3.0, 0.1, 3, None, None, 0, None) == E_SIZE
    assert edges(64, 1, 8, 8, 1000.0, 3.0, 0.1, 3, 64, 64, 8, None) == E_WS               # (the pointers are never followed)

    def acc(N=0, B=0, first=0, depth=None, bits=None, words=0, margin=10, route=0, z_near=0.01, scale=1000.0, seen=None, seen_words=0,
            other=None, size=8, cameras=True, params=True):
        cam = (ctypes.c_double * C['STIN_FRAMES_CAMERA_DOUBLES'])(4.0, 4.0, 3.5, 3.5, 4.0, 4.0, 3.5, 3.5) if cameras else None
        par = (ctypes.c_double * C['STIN_FRAMES_PARAM_DOUBLES'])(scale, 3.0, 2.5, 0.03, z_near) if params else None
        return lib.stin_frames_accumulate_f64(other, N, other, other, B, first, other, size, size, depth, depth, size, size, cam, par, bits,
                                              words, margin, route, other, other, seen, seen_words, None)
    assert acc(cameras=False) == E_NULL and acc(params=False) == E_NULL                  # host arrays: always read
    assert acc() == 0 and acc(N=5) == 0 and acc(B=3) == 0                                # a count of 0: nothing to do
    assert acc(margin=-1) == E_SIZE and acc(route=3) == E_SIZE and acc(z_near=0.0) == E_SIZE and acc(N=-1) == E_SIZE
    assert acc(size=0) == E_SIZE and acc(first=-1) == E_SIZE and acc(B=C['STIN_FRAMES_MAX_BATCH'] + 1) == E_SIZE
    assert acc(N=1, B=1) == E_UNSUPPORTED and acc(N=1, B=1, depth=64, bits=64, words=1) == E_UNSUPPORTED    # exactly one source
    assert acc(N=1, B=1, depth=64, scale=0.0) == E_SIZE
    assert acc(N=1, B=33, bits=64, words=1) == E_SIZE and acc(N=1, B=1, first=32, bits=64, words=1) == E_SIZE
    assert acc(N=1, B=33, bits=64, words=2, seen=64, seen_words=1) == E_SIZE
    assert acc(N=1, B=1, bits=64, words=1) == E_NULL                                      # vertices, poses, frames and sums are missing
    fin = lib.stin_frames_finish_f32
    assert fin(None, None, 0, 0.0, 0.0, 0.0, None, None, None) == 0 and fin(None, None, 1, 0.0, 0.0, 0.0, None, None, None) == E_NULL
    assert fin(None, None, -1, 0.0, 0.0, 0.0, None, None, None) == E_SIZE


def test_cpu_tensors_are_refused():
    V = torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(TypeError):
        P.FrameColors(V, CAM)
    with pytest.raises(TypeError):
        P.vertex_colors_from_frames(V, EYE, torch.from_numpy(COLOR), depth=torch.from_numpy(FLAT), color_camera=CAM)
    with pytest.raises(TypeError):
        P.vertex_colors_from_frames(V, EYE, COLOR, depth=FLAT, color_camera=CAM)
