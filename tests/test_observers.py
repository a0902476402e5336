"""Observer masks, the part that needs no GPU: the numpy restatement of the contract (tests/_observers_oracle.py) on scenes small
enough to check by hand at S = 8, the scan readers on temporary files in both flavours of the reference, the observer cache, the
list format of the reference, the default pose subsets, and the entry points' refusal of CPU tensors."""
import os

import numpy as np
import pytest
import torch

import _observers_oracle as OO
from surface_texture_inpainting_net_amd import _lib, preprocessing as P, scene_io

S = 8
CAM = dict(fx=4.0, fy=4.0, width=8, height=8, image_size=S)             # sx = sy = 1: X = (x / z + 1) 4 - 1 / 2
EYE = np.eye(4)[None]                                                    # at the origin, +z forward, +x right, +y down the rows


def at(X, Y, z=1.0):
    """The point that lands on screen position (X, Y) (pixel units) at depth z; exact for the dyadic values used here."""
    return [((X + 0.5) / 4.0 - 1.0) * z, ((Y + 0.5) / 4.0 - 1.0) * z, z]


def render(V, F, **kw):
    bits, ids, faces = OO.observe(np.asarray(V, dtype=np.float64), np.asarray(F), EYE, **dict(CAM, **kw))
    assert ids.tolist() == [0] and bits.shape == (len(V), 1)
    return bits[:, 0], faces[0]


def test_one_triangle_covers_the_centres_listed_by_hand():
    V = [at(1, 1), at(6, 1), at(1, 6)]
    want = np.full((S, S), -1)
    for i in range(S):                                                   # legs on row 1 and column 1, hypotenuse i + j = 7, all inclusive
        for j in range(S):
            if i >= 1 and j >= 1 and i + j <= 7:
                want[i, j] = 0
    assert int((want == 0).sum()) == 21
    for F in ([[0, 1, 2]], [[0, 2, 1]]):                                 # either orientation
        bits, faces = render(V, F)
        assert np.array_equal(faces, want) and bits.tolist() == [1, 1, 1]
    # half a pixel further out the edges pass between the centres: rows / columns 1 and the diagonal are lost
    bits, faces = render([at(1.5, 1.5), at(5.5, 1.5), at(1.5, 5.5)], [[0, 1, 2]])
    want = np.full((S, S), -1)
    for i in range(S):
        for j in range(S):
            if i >= 2 and j >= 2 and i + j <= 7:
                want[i, j] = 0
    assert np.array_equal(faces, want)


def test_the_nearer_of_two_overlapping_triangles_wins():
    far = [at(0, 0, 2.0), at(7, 0, 2.0), at(0, 7, 2.0)]
    near = [at(1, 1), at(3, 1), at(1, 3)]
    for order in (0, 1):
        V = far + near if order == 0 else near + far
        F = [[0, 1, 2], [3, 4, 5]]
        f_far, f_near = (0, 1) if order == 0 else (1, 0)
        bits, faces = render(V, F)
        for i in range(S):
            for j in range(S):
                if i >= 1 and j >= 1 and i + j <= 4:
                    assert faces[i, j] == f_near
                elif i + j <= 7:
                    assert faces[i, j] == f_far
                else:
                    assert faces[i, j] == -1
        assert bits.tolist() == [1] * 6
    # the far one entirely behind the near one: its vertices are not observed
    bits, faces = render([at(0, 0), at(7, 0), at(0, 7), at(1, 1, 2.0), at(3, 1, 2.0), at(1, 3, 2.0)], [[0, 1, 2], [3, 4, 5]])
    assert bits.tolist() == [1, 1, 1, 0, 0, 0] and set(np.unique(faces)) == {-1, 0}


def test_of_two_coplanar_duplicates_the_lower_id_wins():
    tri = [at(1, 1), at(6, 1), at(1, 6)]
    bits, faces = render(tri + tri, [[0, 1, 2], [3, 4, 5]])
    assert set(np.unique(faces)) == {-1, 0} and bits.tolist() == [1, 1, 1, 0, 0, 0]
    bits, faces = render(tri + tri, [[3, 4, 5], [0, 1, 2]])
    assert set(np.unique(faces)) == {-1, 0} and bits.tolist() == [0, 0, 0, 1, 1, 1]


def test_a_centre_on_a_shared_edge_goes_to_the_lower_id():
    V = [at(1, 1), at(5, 1), at(5, 5), at(1, 5)]                         # a square split along the diagonal (1, 1) - (5, 5)
    upper, lower = [0, 1, 2], [0, 2, 3]                                  # above / below the diagonal in the image
    for F in ([upper, lower], [lower, upper]):
        bits, faces = render(V, F)
        for k in range(1, 6):
            assert faces[k, k] == 0                                      # both cover it at the same depth: face 0, whichever that is
        up, lo = (0, 1) if F[0] is upper else (1, 0)
        assert faces[1, 4] == up and faces[4, 1] == lo
        assert int((faces >= 0).sum()) == 25 and bits.tolist() == [1, 1, 1, 1]


def test_a_face_with_a_vertex_behind_z_near_is_dropped_not_clipped():
    V = [at(1, 1), at(6, 1), at(1, 6, 0.005), at(1, 6)]
    bits, faces = render(V, [[0, 1, 2]])
    assert (faces == -1).all() and bits.tolist() == [0, 0, 0, 0]
    bits, faces = render(V, [[0, 1, 2]], z_near=0.001)                   # the same face with the plane moved in front of it
    assert (faces == 0).any()
    bits, faces = render(V, [[0, 1, 2], [0, 1, 3]])
    assert set(np.unique(faces)) == {-1, 1} and bits.tolist() == [1, 1, 0, 1]
    V[2] = [0.0, 0.0, -1.0]                                              # behind the camera
    assert (render(V, [[0, 1, 2]])[1] == -1).all()


def test_a_face_without_area_is_dropped():
    bits, faces = render([at(1, 1), at(3, 3), at(6, 6)], [[0, 1, 2]])    # collinear on screen: its centres lie ON all three edges
    assert (faces == -1).all() and bits.tolist() == [0, 0, 0]
    bits, faces = render([at(2, 2), at(2, 2), at(5, 2)], [[0, 1, 2]])
    assert (faces == -1).all()


def test_invalid_poses_and_bad_indices_in_the_restatement():
    V = [at(1, 1), at(6, 1), at(1, 6)]
    poses = np.repeat(EYE, 4, axis=0)
    poses[1, 0, 3] = -np.inf
    poses[2, 2, 2] = np.nan
    bits, ids, faces = OO.observe(np.asarray(V), np.asarray([[0, 1, 2], [0, 1, 3], [0, -1, 2]]), poses, **CAM)
    assert ids.tolist() == [0, 3] and bits[:, 0].tolist() == [9, 9, 9]
    assert (faces[1] == -1).all() and (faces[2] == -1).all() and set(np.unique(faces[0])) == {-1, 0}


def test_look_at_and_orbit_put_the_target_in_the_centre():
    poses = OO.orbit(5, 3.0, height=1.0, target=(0.5, -0.25, 0.125))
    RT, valid = P.pose_extrinsics(poses)
    assert valid.tolist() == [1] * 5 and RT.shape == (5, 12)
    X, Y, Z = OO.screen(np.array([[0.5, -0.25, 0.125]]), RT[3], 1.0, 1.0, 256)
    assert abs(X[0] - 127.5) < 1e-9 and abs(Y[0] - 127.5) < 1e-9 and abs(Z[0] - np.sqrt(10.0)) < 1e-12
    up = OO.screen(np.array([[0.5, -0.25, 1.125]]), RT[3], 1.0, 1.0, 256)
    assert up[1][0] < 127.5                                              # world +z is up in the image (smaller row)


def write_pose(path, M):
    with open(path, 'w') as f:
        for row in M:
            f.write(' '.join('-inf' if v == -np.inf else repr(float(v)) for v in row) + '\n')


def test_scan_readers_in_both_flavours(tmp_path):
    poses = OO.orbit(4, 2.0, height=0.5)
    poses[2] = -np.inf
    K = np.array([[1170.19, 0, 647.75, 0], [0, 1170.19, 483.75, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    cpp, py = tmp_path / 'cpp', tmp_path / 'py'
    os.makedirs(cpp)
    os.makedirs(py)
    for i, M in enumerate(poses):
        write_pose(cpp / ('frame-%06d.pose.txt' % i), M)
        write_pose(py / ('%d.txt' % (i + 10)), M)                        # sorted by NAME, as the reference: 10, 11, 12, 13
    (cpp / 'frame-000000.color.jpg').write_bytes(b'')
    (cpp / '_info.txt').write_text('m_versionNumber = 4\nm_sensorName = StructureSensor\nm_colorWidth = 1296\nm_colorHeight = 968\n'
                                   'm_depthWidth = 640\nm_calibrationColorIntrinsic = %s\nm_frames.size = 4\n'
                                   % ' '.join(repr(float(v)) for v in K.ravel()))
    got = scene_io.load_camera_poses(str(cpp))
    assert got.dtype == np.float64 and got.shape == (4, 4, 4)
    assert np.array_equal(got[[0, 1, 3]], poses[[0, 1, 3]]) and np.all(got[2] == -np.inf)
    assert scene_io.load_camera_poses(str(cpp), max_num_poses=2).shape == (2, 4, 4)
    assert P.pose_extrinsics(got)[1].tolist() == [1, 1, 0, 1]
    cfg = scene_io.load_scan_config(str(cpp), 'scene0000_00')
    assert cfg['colorwidth'] == 1296 and cfg['colorheight'] == 968 and np.array_equal(cfg['colorintrinsic'], K)
    # the python SensReader's export: <scan>.txt + intrinsic_color.txt; its pose files are every other *.txt of the directory in
    # the reference too, so they live in a directory of their own here
    scan = tmp_path / 'scan'
    os.makedirs(scan)
    (scan / 'scene0000_00.txt').write_text('axisAlignment = 1 0 0 0 0 1 0 0 0 0 1 0 0 0 0 1\ncolorHeight = 968\ncolorWidth = 1296\n'
                                           'fx_color = 1170.19\nnumColorFrames = 4\n')
    np.savetxt(scan / 'intrinsic_color.txt', K)
    cfg = scene_io.load_scan_config(str(scan), 'scene0000_00', cpp_sens_reader=False)
    assert cfg['colorwidth'] == 1296 and cfg['colorheight'] == 968 and np.array_equal(cfg['colorintrinsic'], K)
    got = scene_io.load_camera_poses(str(py), cpp_sens_reader=False)
    assert got.shape == (4, 4, 4) and np.array_equal(got[3], poses[3])


def test_observer_cache_round_trip_without_pickle(tmp_path):
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 2 ** 32, (37, 3), dtype=np.uint64).astype(np.uint32)
    ids = np.array([0, 1, 3, 70], dtype=np.int64)
    path = scene_io.write_observers(str(tmp_path / 'observers_per_vert' / 'scene0000_00.npz'), torch.from_numpy(bits), ids, 71)
    b, i, n = scene_io.read_observers(path)
    assert b.dtype == np.uint32 and np.array_equal(b, bits) and i.dtype == np.int64 and np.array_equal(i, ids) and n == 71
    with np.load(path, allow_pickle=False) as data:
        assert sorted(data.files) == ['bits', 'num_poses', 'valid_pose_ids']
    b, _, _ = scene_io.read_observers(path, device='cpu')
    assert torch.is_tensor(b) and b.dtype == torch.uint32 and np.array_equal(b.numpy(), bits)


def test_observers_to_lists_and_the_masks_of_the_restatement():
    rng = np.random.default_rng(1)
    seen = rng.uniform(size=(23, 70)) < 0.3
    bits = P._pack_pose_bits(seen, 3)
    assert bits.shape == (23, 3) and np.array_equal(OO.unpack(bits, 70), seen)
    lists = P.observers_to_lists(torch.from_numpy(bits), 70)
    assert lists == [np.flatnonzero(r).tolist() for r in seen] and lists == P.observers_to_lists(bits)
    visible = rng.uniform(size=(2, 70)) < 0.5
    for least in (0, 1, 5, 71):
        mask, count = OO.masks(bits, visible, least)
        for m in range(2):                                               # generate_mask_from_vertex_observing_poses, as written
            keep = set(np.flatnonzero(visible[m]).tolist())
            want = [1 if len([p for p in lst if p in keep]) >= least else 0 for lst in lists]
            assert mask[m].tolist() == want
        assert np.array_equal(OO.masks(bits, visible, least, invert=True)[0], 1 - mask)


def test_the_default_subsets_restate_the_numpy_call():
    ids = np.array([0, 2, 3, 7, 8, 40, 41, 69])
    vis = P.observer_visible(ids, 70, keep_probability=0.5, num_masks=3, seed=11)
    assert vis.dtype == bool and vis.shape == (3, 70)
    for m in range(3):
        keep = np.random.RandomState(11 + m).rand(len(ids)) <= 0.5
        want = np.zeros(70, dtype=bool)
        want[ids[keep]] = True
        assert np.array_equal(vis[m], want)
    assert P.observer_visible(ids, 70, 1.0).all(axis=0).sum() == len(ids)
    assert not P.observer_visible(ids, 70, -1.0).any()
    with pytest.raises(IndexError):
        P.observer_visible(ids, 69)


def test_entry_points_exist_and_refuse_cpu_tensors():
    V, F = OO.wall(2, 1.0)
    v, f = torch.from_numpy(V), torch.from_numpy(F)
    with pytest.raises(TypeError):
        P.observe_vertices(v, f, OO.orbit(2, 2.0, 1.0), 1170.0, 1170.0, 1296, 968)
    with pytest.raises(TypeError):
        P.observer_masks(torch.zeros(5, 1, dtype=torch.uint32), np.arange(2), 2)
    with pytest.raises(TypeError):
        P.observer_counts(torch.zeros(5, 1, dtype=torch.uint32))
    for name in ('stin_observe_workspace_bytes', 'stin_observe_poses_f64', 'stin_observe_mask_u32'):
        assert name in _lib.SIGNATURES
    assert _lib.CONSTANTS['STIN_OBSERVE_BAD_INDEX'] == 1 and _lib.CONSTANTS['STIN_OBSERVE_LARGE_FACE'] == 2
    assert _lib.CONSTANTS['STIN_OBSERVE_LARGE_BOX'] > 0
