"""k nearest neighbours, the part that needs no GPU: the numpy restatement of the contract (tests/_knn_oracle.py) against scipy's
cKDTree on tie-free points and against hand-written ties; the entry points' declarations, their argument checks (which return
before anything is launched) and the refusal of CPU tensors; the baseline's ordering (a linear field, one hole) on the oracle."""
import ctypes

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import _knn_oracle as KO
from surface_texture_inpainting_net_amd import _lib, preprocessing as P

_I, _L, _Z, _P = ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_void_p


def test_oracle_agrees_with_a_kd_tree_on_tie_free_points():
    rng = np.random.default_rng(11)
    pts, qs = rng.uniform(-2, 2, (700, 3)), rng.uniform(-2, 2, (90, 3))
    for k in (1, 3, 16):
        dist, want = cKDTree(pts).query(qs, k=k)
        idx, d2 = KO.knn(qs, pts, k)
        assert idx.dtype == np.int64 and d2.dtype == np.float64 and idx.shape == d2.shape == (90, k)
        assert np.array_equal(idx, np.asarray(want).reshape(90, k))
        # scipy returns distances, not squares: squaring its rounded root costs an ulp or two
        assert np.all(np.abs(d2 - np.asarray(dist).reshape(90, k) ** 2) <= 4 * np.spacing(d2))
        assert np.all(np.diff(d2, axis=1) > 0)                            # tie free, ascending
    # a validity mask = the tree of the valid points, mapped back to indices of the full array
    valid = rng.uniform(size=700) < 0.4
    _, want = cKDTree(pts[valid]).query(qs, k=5)
    assert np.array_equal(KO.knn(qs, pts, 5, point_valid=valid)[0], np.flatnonzero(valid)[want])


def test_hand_written_ties_padding_and_subsets():
    q = np.zeros((1, 3))
    square = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]], dtype=np.float64)      # four points at d = 1
    idx, d2 = KO.knn(q, square, 2)
    assert idx.tolist() == [[0, 1]] and d2.tolist() == [[1.0, 1.0]]
    assert KO.knn(q, square[::-1], 3)[0].tolist() == [[0, 1, 2]]                              # the index decides, not the position
    # an invalid point in the middle of a tie is skipped in place; the indices stay those of the full array
    assert KO.knn(q, square, 2, point_valid=[1, 0, 1, 1])[0].tolist() == [[0, 2]]
    assert KO.knn(q, square, 4, point_valid=[0, 0, 1, 1])[0].tolist() == [[2, 3, -1, -1]]
    assert KO.knn(q, square, 4, point_valid=[0, 0, 1, 1])[1].tolist() == [[1.0, 1.0, np.inf, np.inf]]
    # a nearer point with a higher index comes first; equal ones behind it in index order
    pts = np.concatenate([square, [[0.5, 0, 0]], square[:1]])
    assert KO.knn(q, pts, 4)[0].tolist() == [[4, 0, 1, 2]]
    assert KO.knn(q, pts, 16)[0][0, :7].tolist() == [4, 0, 1, 2, 3, 5, -1]
    # a query that coincides with points: d = 0, twice
    idx, d2 = KO.knn(square[:1], pts, 3)
    assert idx.tolist() == [[0, 5, 4]] and d2.tolist() == [[0.0, 0.0, 0.25]]
    # nothing to find: no points, no valid point; a non-finite invalid point is never looked at
    assert KO.knn(q, np.zeros((0, 3)), 2)[0].tolist() == [[-1, -1]]
    assert KO.knn(q, square, 2, point_valid=np.zeros(4))[1].tolist() == [[np.inf, np.inf]]
    bad = square.copy()
    bad[1] = np.nan
    assert KO.knn(q, bad, 3, point_valid=[1, 0, 1, 1])[0].tolist() == [[0, 2, 3]]
    # a query subset: the other rows hold -1 / inf
    idx, d2 = KO.knn(np.concatenate([q, q + 0.1, q]), square, 1, query_index=[2, 0])
    assert idx.tolist() == [[0], [-1], [0]] and d2[1, 0] == np.inf
    # float32 input is promoted exactly
    assert np.array_equal(KO.knn(pts.astype(np.float32), pts.astype(np.float32), 3)[1], KO.knn(pts, pts, 3)[1])


def test_mean_is_the_left_to_right_fp64_sum():
    vals = np.array([[1e8], [1.0], [-1e8], [0.25]], dtype=np.float32)
    idx = np.array([[0, 1, 2], [0, 2, 1], [3, -1, -1], [-1, -1, -1], [1, 3, -1]])
    out, filled = KO.knn_mean(vals, idx, out=np.full((5, 1), 7.0, dtype=np.float32))
    assert out[:, 0].tolist() == [np.float32(1.0 / 3.0), np.float32(1.0 / 3.0), 0.25, 7.0, 0.625]   # fp64 holds 1e8 + 1 exactly
    assert filled.tolist() == [True, True, True, False, True]
    c, f = KO.fill_unseen(np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0], [9, 9, 9]], dtype=np.float64), vals, [1, 0, 2, 0], k=2)
    assert c[:, 0].tolist() == [1e8, 0.0, -1e8, 0.0] and f.tolist() == [False, True, False, True]
    c, f = KO.fill_unseen(np.zeros((4, 3)), vals, [1, 0, 2, 0], k=2, min_count=2)
    assert c[:, 0].tolist() == [-1e8, -1e8, -1e8, -1e8] and f.tolist() == [True, True, False, True]
    c, f = KO.fill_unseen(np.zeros((4, 3)), vals, [0, 0, 0, 0])
    assert np.array_equal(c, vals) and not f.any()


NAMES = {'stin_knn_chunks': (_I, [_L, _L, _I]),
         'stin_knn_workspace_bytes': (_Z, [_L, _I, _I]),
         'stin_knn_f64': (_I, [_P, _L, _P, _P, _L, _P, _P, _L, _I, _I, _P, _P, _P, _P, _Z, _P]),
         'stin_knn_mean_f32': (_I, [_P, _L, _L, _I, _P, _I, _P, _P, _L, _L, _P, _L, _P, _P])}


def test_entry_points_are_declared_exported_and_check_their_arguments():
    lib = _lib.load()                                                    # no GPU needed for these calls: they return before a launch
    for name, want in NAMES.items():
        assert _lib.SIGNATURES[name] == want and getattr(lib, name) is not None
    C = _lib.CONSTANTS
    assert C['STIN_KNN_MAX_K'] == 16 and C['STIN_KNN_MAX_C'] == 16
    E_NULL, E_SIZE, E_WS, E_UNSUP = C['STIN_E_NULL'], C['STIN_E_SIZE'], C['STIN_E_WORKSPACE'], C['STIN_E_UNSUPPORTED']
    ws = lib.stin_knn_workspace_bytes
    assert ws(1000, 1, 3) == 0 and ws(0, 4, 3) == 0 and ws(1000, 4, 0) == 0 and ws(1000, 4, 17) == 0
    assert ws(1000, 4, 3) >= 4 * 1000 * 3 * 12 and ws(1001, 3, 16) >= 3 * 1001 * 16 * 12
    assert lib.stin_knn_chunks(0, 100, 3) == 1 and lib.stin_knn_chunks(100, 0, 3) == 1 and lib.stin_knn_chunks(100, 100, 0) == 1

    def knn(n_rows=8, P=8, Q=8, k=3, chunks=1, data=64, q_index=None, out=64, flags=64, work=None, work_bytes=0):
        return lib.stin_knn_f64(data, n_rows, data, None, P, q_index, None, Q, k, chunks, out, None, flags, work, work_bytes, None)
    assert knn(k=0) == E_SIZE and knn(k=17) == E_SIZE and knn(k=-1) == E_SIZE
    assert knn(chunks=0) == E_SIZE and knn(chunks=65) == E_SIZE and knn(P=-1) == E_SIZE and knn(Q=-1) == E_SIZE and knn(n_rows=-1) == E_SIZE
    assert knn(Q=9) == E_SIZE                                            # more queries than rows and no q_index
    assert knn(P=2 ** 31 - 1) == E_UNSUP
    assert knn(data=None) == E_NULL and knn(out=None) == E_NULL and knn(flags=None) == E_NULL
    assert knn(Q=0, data=None, out=None, flags=None) == 0                # nothing to do
    assert knn(P=2000, chunks=2) == E_NULL                               # chunked and no workspace
    assert knn(P=2000, chunks=2, work=64, work_bytes=ws(8, 2, 3) - 1) == E_WS
    assert knn(P=2000, chunks=3, k=16, work=64, work_bytes=ws(8, 3, 3)) == E_WS

    def mean(P=8, C=3, k=3, Q=8, n_rows=8, ld_values=None, ld_out=None, data=64, q_index=None):
        return lib.stin_knn_mean_f32(data, C if ld_values is None else ld_values, P, C, data, k, q_index, None, Q, n_rows, data,
                                     C if ld_out is None else ld_out, None, None)
    assert mean(C=0) == E_SIZE and mean(C=17) == E_SIZE and mean(k=0) == E_SIZE and mean(k=17) == E_SIZE
    assert mean(ld_values=2) == E_SIZE and mean(ld_out=2) == E_SIZE and mean(Q=9) == E_SIZE and mean(P=-1) == E_SIZE
    assert mean(data=None) == E_NULL and mean(Q=0, data=None) == 0


def test_cpu_tensors_and_bad_arguments_are_refused():
    V = torch.zeros(5, 3, dtype=torch.float64)
    with pytest.raises(TypeError):
        P.knn(V, V, 3)
    with pytest.raises(TypeError):
        P.knn(V.numpy(), V.numpy(), 3)
    with pytest.raises(TypeError):
        P.fill_unseen_colors(V, torch.zeros(5, 3), torch.ones(5, dtype=torch.int32))
    with pytest.raises(TypeError):
        P.knn_inpaint((V, torch.zeros(5, 3), torch.zeros(5, 1)))
    for k in (0, 17, -1, 2.5, True):
        with pytest.raises(ValueError):
            P.knn(V, V, k)
        with pytest.raises(ValueError):
            P.fill_unseen_colors(V, torch.zeros(5, 3), torch.ones(5, dtype=torch.int32), k=k)


def test_baseline_beats_the_constant_fill_on_a_linear_field_with_the_oracle():
    pos, color, _ = KO.baseline_scene()
    mask = KO.hole_mask()
    hole = mask > 0
    assert hole.sum() == 41 and not hole.reshape(KO.SIDE, KO.SIDE)[[0, -1]].any()       # a hole well inside the grid
    got, filled = KO.fill_unseen(pos, color, (~hole).astype(np.int32), k=3)
    assert np.array_equal(filled, hole) and np.array_equal(got[~hole], color[~hole])
    err_knn = np.abs(got[hole].astype(np.float64) - color[hole]).mean()
    err_const = np.abs(0.0 - color[hole].astype(np.float64)).mean()
    print('mean |error| over the hole: knn %.4f, constant fill %.4f' % (err_knn, err_const))
    # the field changes by 0.0625 per grid step and every filled value is a mean of rim values at most 5 steps away
    assert err_knn <= 5 * 0.0625 and err_knn < err_const
