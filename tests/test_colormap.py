"""The rigid colour-map optimisation on the host: the numpy restatement of the contract (tests/_colormap_oracle.py) does what an
optimiser has to do - it recovers a perturbed pose between anchored ones, lowers the photometric residual, and leaves exact poses
alone - and the host code of preprocessing.optimize_poses_rigid (the increment, the update, the argument checks) behaves as stated.
The kernels are compared against the same restatement in tests/test_colormap_gpu.py."""
import functools

import numpy as np
import pytest
import torch

import _colormap_oracle as CO
import _observers_oracle as OO
import _render_oracle as RO
from surface_texture_inpainting_net_amd import preprocessing as P

CAM = (60.0, 58.0, 31.5, 23.5)                                          # 48 x 64 frames, fx != fy
H, W, MARGIN = 48, 64, 2
FREED = 3


def bumpy_wall(k):
    """A textured wall in front of the cameras: (vertices, faces, colours float32 in [0, 1])."""
    V, F = OO.wall(k, 3.0, origin=(2, 0, 0), u=(0, 1, 0), v=(0, 0, 1))
    V = V.copy()
    y, z = V[:, 1], V[:, 2]
    V[:, 0] += 0.25 * np.sin(2.1 * y) * np.cos(1.7 * z)
    C = np.stack([0.5 + 0.49 * np.sin(1.86 * y + 0.3) * np.cos(1.38 * z), 0.5 + 0.49 * np.cos(1.62 * y) * np.sin(1.98 * z + 0.5),
                  0.5 + 0.49 * np.sin(1.14 * y + 1.74 * z)], axis=1).astype(np.float32)      # smooth: wavelengths of 3 m and more
    return V, F, C


EYES = [(0.0, 0.0, 0.0), (0.1, 0.2, 0.05), (-0.15, -0.1, 0.1), (0.05, -0.25, -0.1), (-0.1, 0.15, -0.15), (0.2, 0.05, 0.12)]
TARGETS = [(2.0, 0.0, 0.0), (2.0, 0.1, 0.05), (2.0, -0.1, 0.1), (2.0, -0.05, -0.1), (2.0, 0.15, -0.05), (2.0, 0.0, 0.1)]


@functools.lru_cache(maxsize=None)
def scene(k=24):
    """The wall rendered from six poses within 0.3 m of the origin: (V, F, C, poses, colour frames uint8, depth uint16, all-ones bits)."""
    V, F, C = bumpy_wall(k)
    poses = np.stack([OO.look_at(e, t) for e, t in zip(EYES, TARGETS)])
    r = RO.render(V, F, C, poses, CAM, H, W)
    bits = np.full((len(V), 1), 0xFFFFFFFF, dtype=np.uint32)
    return V, F, C, poses, r.color_u8, r.depth, bits


def perturbed(pose, degrees, metres):
    """The camera-to-world pose with its extrinsic turned by `degrees` about a fixed axis and shifted by `metres` along another."""
    axis = np.array([0.28, 0.94, 0.2]) / np.linalg.norm([0.28, 0.94, 0.2])      # mostly a pan; the shift moves the image the same way
    shift = np.array([0.96, -0.28, 0.0]) * metres
    w = axis * np.radians(degrees)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    t = np.linalg.norm(w)
    R = np.eye(3) + np.sin(t) / t * K + (1 - np.cos(t)) / (t * t) * K @ K
    D = np.eye(4)
    D[:3, :3], D[:3, 3] = R, shift
    return np.linalg.inv(D @ np.linalg.inv(pose))


def pose_error(got, want):
    """(rotation in degrees, translation in metres) between two camera-to-world poses"""
    R = got[:3, :3].T @ want[:3, :3]
    return np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))), np.linalg.norm(got[:3, 3] - want[:3, 3])


@functools.lru_cache(maxsize=None)
def one_free(degrees=0.52, metres=0.010, k=24, iterations=30):
    V, _, _, poses, color, _, bits = scene(k)
    start = poses.copy()
    start[FREED] = perturbed(poses[FREED], degrees, metres)
    free = np.zeros(6, dtype=bool)
    free[FREED] = True
    out, info = CO.optimize(V, start, color, CAM, bits, iterations=iterations, free=free, margin=MARGIN)
    return poses, start, out, info


def test_the_fixture_is_what_the_conditions_rest_on():
    V, _, _, poses, color, depth, _ = scene()
    assert V.shape == (625, 3) and color.shape == (6, H, W, 3) and color.dtype == np.uint8 and depth.shape == (6, H, W)
    assert all(np.linalg.norm(e) <= 0.3 for e in EYES)
    _, _, _, info = one_free()
    assert 900 <= int(info['pairs'][0].sum()) <= 1400                   # about 1 130 pairs
    r0, t0 = pose_error(perturbed(poses[FREED], 0.52, 0.010), poses[FREED])
    assert abs(r0 - 0.52) < 1e-6 and 0.009 < t0 < 0.012


@pytest.mark.parametrize('degrees,metres,k', [(0.52, 0.010, 24), (1.30, 0.030, 24)])
def test_one_free_pose_between_five_held_ones_is_recovered(degrees, metres, k):
    poses, start, out, info = one_free(degrees, metres, k)
    r0, t0 = pose_error(start[FREED], poses[FREED])
    r1, t1 = pose_error(out[FREED], poses[FREED])
    e = info['residual'].sum(axis=1)
    print('one free, %g deg / %g m, wall(%d): rotation %.4f -> %.4f deg, translation %.2f -> %.2f mm, e %.6f -> %.6f, pairs %d'
          % (degrees, metres, k, r0, r1, t0 * 1e3, t1 * 1e3, e[0], e[-1], info['pairs'][0].sum()))
    assert r1 < 0.5 * r0 and t1 < 0.5 * t0
    assert e[-1] < 0.25 * e[0]
    held = [p for p in range(6) if p != FREED]
    assert out[held].tobytes() == start[held].tobytes()                # bit-identical to their input
    assert info['status'].tolist() == [CO.NOT_FREE if p != FREED else 0 for p in range(6)]
    assert info['residual'].shape == (31, 6) and info['pairs'].shape == (31, 6)


def test_all_free_lowers_the_residual():
    V, _, _, poses, color, _, bits = scene()
    start = poses.copy()
    for p in range(1, 6):
        start[p] = perturbed(poses[p], 0.52 * (1 if p % 2 else -1), 0.010 + 0.001 * p)
    out, info = CO.optimize(V, start, color, CAM, bits, iterations=30, margin=MARGIN)
    e = info['residual'].sum(axis=1)
    print('all free: e %.6f -> %.6f' % (e[0], e[-1]))
    assert e[-1] < 0.25 * e[0]
    assert not info['status'].any()


EXACT_STEP = 5.25e-3                                                    # max |x| seen on this fixture (radians, metres); the floor is the uint8 quantisation


def test_exact_poses_hardly_move():
    V, _, _, poses, color, _, bits = scene()
    steps = []
    CO.optimize(V, poses, color, CAM, bits, iterations=1, margin=MARGIN, steps=steps)
    assert len(steps) == 6
    worst = max(float(np.abs(x).max()) for _, _, x in steps)
    print('exact poses, one iteration: max |x| = %.3e' % worst)
    assert worst < 10 * EXACT_STEP


def test_the_increment_is_a_rotation_and_matches_its_first_order_form():
    assert np.array_equal(P.rigid_increment(np.zeros(6)), np.eye(4))
    rng = np.random.default_rng(5)
    for scale in (1.0, 1e-4):
        x = rng.uniform(-1, 1, 6) * scale
        D = P.rigid_increment(x)
        assert D.tobytes() == CO.increment(x).tobytes()
        R = D[:3, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1) < 1e-15
        assert D[3].tolist() == [0, 0, 0, 1] and D[:3, 3].tobytes() == x[3:].tobytes()
    first = np.eye(3) + np.array([[0, -x[2], x[1]], [x[2], 0, -x[0]], [-x[1], x[0], 0]])
    assert np.abs(R - first).max() < 2 * scale * scale               # I + [x]_x up to second order
    # one pose about one axis at a time: the rotation the name says
    a = 0.3
    assert np.allclose(P.rigid_increment([a, 0, 0, 0, 0, 0])[:3, :3], [[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    assert np.allclose(P.rigid_increment([0, a, 0, 0, 0, 0])[:3, :3], [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    assert np.allclose(P.rigid_increment([0, 0, a, 0, 0, 0])[:3, :3], [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])


def rows_of_the_scene():
    V, _, _, poses, color, _, bits = scene()
    RT, valid = P.pose_extrinsics(poses)
    total, count = CO.accumulate(V, RT, valid, color, CAM, bits, margin=MARGIN)
    return CO.normal(V, RT, valid, CO.gradients(color), CAM, bits, CO.proxy(total, count), margin=MARGIN)


def test_the_host_update_moves_what_it_may_and_reports_the_rest():
    rows, counts = rows_of_the_scene()
    rows, counts = rows.copy(), counts.copy()
    rows[1] = 0.0                                                       # a constant image: J = 0, A = 0
    counts[2] = 15                                                      # one pair short of min_pairs
    rows[4, 21:27] = np.inf                                             # solvable, but x is not finite
    valid = np.array([1, 1, 1, 1, 1, 0], dtype=np.uint8)
    free = np.array([1, 1, 1, 0, 1, 1], dtype=bool)
    E = np.stack([np.linalg.inv(p) for p in scene()[3]])
    before = E.copy()
    status = np.zeros(6, dtype=np.int32)
    with np.errstate(all='ignore'):
        moved = P.rigid_update(E, valid, free, rows, counts, 16, status)
    assert moved.tolist() == [True, False, False, False, False, False]
    assert status.tolist() == [0, P.COLORMAP_SINGULAR, P.COLORMAP_FEW_PAIRS, 0, P.COLORMAP_SINGULAR, 0]
    assert E[1:].tobytes() == before[1:].tobytes() and E[0].tobytes() != before[0].tobytes()
    # the same update, restated
    F, st = before.copy(), np.zeros(6, dtype=np.int32)
    with np.errstate(all='ignore'):
        assert CO.update(F, valid, free, rows, counts, 16, st).tolist() == moved.tolist()
    assert F.tobytes() == E.tobytes() and st.tolist() == status.tolist()
    assert (P.COLORMAP_NOT_FREE, P.COLORMAP_INVALID, P.COLORMAP_FEW_PAIRS, P.COLORMAP_SINGULAR) == (CO.NOT_FREE, CO.INVALID, CO.FEW_PAIRS, CO.SINGULAR)


def test_a_constant_image_and_a_line_of_sight_keep_the_pose():
    V, _, _, poses, color, _, bits = scene()
    flat = color.copy()
    flat[2] = 77                                                        # pose 2 sees a constant image: no gradient, A = 0
    out, info = CO.optimize(V, poses, flat, CAM, bits, iterations=2, margin=MARGIN)
    assert info['status'][2] == CO.SINGULAR and out[2].tobytes() == poses[2].tobytes()
    assert not info['status'][[0, 1, 3, 4, 5]].any()
    # all vertices on one line of sight of pose 0 (and too few of them for min_pairs elsewhere)
    line = np.stack([np.linspace(1.0, 3.0, 40), np.zeros(40), np.zeros(40)], axis=1)
    out, info = CO.optimize(line, poses, color, CAM, np.full((40, 1), 1, dtype=np.uint32), iterations=1, margin=MARGIN, min_pairs=41)
    assert info['pairs'][0, 0] == 40 and info['status'][0] == CO.FEW_PAIRS and out.tobytes() == poses.tobytes()
    # with enough of them: xv = yv = 0 for every pair, so the columns of rotation z and translation z are zero - singular
    out, info = CO.optimize(line, poses, color, CAM, np.full((40, 1), 1, dtype=np.uint32), iterations=1, margin=MARGIN, min_pairs=16)
    assert info['status'][0] == CO.SINGULAR and out.tobytes() == poses.tobytes()


def test_invalid_poses_come_back_as_given():
    V, _, _, poses, color, _, bits = scene()
    lost = poses.copy()
    lost[4] = -np.inf
    lost[5, 1, 2] = np.nan
    out, info = CO.optimize(V, lost, color, CAM, bits, iterations=2, margin=MARGIN)
    assert out[4:].tobytes() == lost[4:].tobytes()
    assert info['status'][4] == CO.INVALID and info['status'][5] == CO.INVALID and not info['status'][:4].any()
    assert not info['pairs'][:, 4:].any() and not info['residual'][:, 4:].any()


def test_the_order_of_the_sums_is_the_contracts():
    rng = np.random.default_rng(9)
    for n in (1, 37, 1024, 1025, 2304):
        T = rng.standard_normal((n, 3)) * 10.0 ** rng.integers(-8, 8, (n, 3))
        want = np.zeros(3)
        tiles = -(-n // 1024)
        for tile in range(tiles):
            x = np.zeros((256, 3))
            for i in range(4):
                for lane in range(256):
                    v = tile * 1024 + lane + 256 * i
                    if v < n:
                        x[lane] = x[lane] + T[v]
            s = 128
            while s >= 1:
                for i in range(s):
                    x[i] = x[i] + x[i + s]
                s //= 2
            want = want + x[0]
        assert CO.ordered_sum(T).tobytes() == want.tobytes()
    assert np.signbit(CO.ordered_sum(np.full((5, 2), -0.0))).tolist() == [False, False]      # +0.0 + -0.0: no lane sum is -0.0


def test_argument_errors_are_raised_before_any_library_call():
    V, _, _, poses, color, depth, bits = scene()
    v, c, d = torch.from_numpy(V), torch.from_numpy(color), torch.from_numpy(depth)
    b = torch.from_numpy(bits.view(np.int32)).view(torch.uint32)
    kw = dict(color_camera=CAM, margin=MARGIN)
    with pytest.raises(ValueError, match='exactly one of depth and bits'):
        P.optimize_poses_rigid(v, poses, c, **kw)
    with pytest.raises(ValueError, match='exactly one of depth and bits'):
        P.optimize_poses_rigid(v, poses, c, depth=d, bits=b, **kw)
    with pytest.raises(ValueError, match='margin must be >= 1'):
        P.optimize_poses_rigid(v, poses, c, depth=d, color_camera=CAM, margin=0)
    with pytest.raises(ValueError, match='color_camera'):
        P.optimize_poses_rigid(v, poses, c, depth=d)
    with pytest.raises(ValueError, match='free must be bool'):
        P.optimize_poses_rigid(v, poses, c, depth=d, free=np.ones(5, dtype=bool), **kw)
    with pytest.raises(ValueError, match='free must be bool'):
        P.optimize_poses_rigid(v, poses, c, depth=d, free=np.ones(6), **kw)
    with pytest.raises(ValueError, match='iterations'):
        P.optimize_poses_rigid(v, poses, c, depth=d, iterations=-1, **kw)
    with pytest.raises(TypeError, match='color must be a CUDA tensor'):
        P.optimize_poses_rigid(v, poses, c, depth=d, **kw)             # CPU tensors: there is no CPU fallback
    with pytest.raises(TypeError, match='color must be a CUDA tensor'):
        P.optimize_poses_rigid(v, poses, color, bits=b, **kw)
