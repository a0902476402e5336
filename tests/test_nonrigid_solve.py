"""The banded solve of the non-rigid colour-map optimisation on the host: the numpy restatement of its contract
(tests/_nonrigid_solve_oracle.py; include/stin_hip.h, "Non-rigid solve") solves the systems the host update builds as well as
LAPACK does, treats the special poses as stated, and drives the recovery scene of tests/test_nonrigid.py to the same end - and
preprocessing refuses a wrong `solver` before it calls the library.  The kernels are compared against the same restatement, byte
for byte, in tests/test_nonrigid_solve_gpu.py."""
import functools

import numpy as np
import pytest
import torch

import _colormap_oracle as CO
import _nonrigid_oracle as NO
import _nonrigid_solve_oracle as SO
from surface_texture_inpainting_net_amd import preprocessing as P
from test_colormap import CAM, FREED, MARGIN, scene
from test_nonrigid import ANCHOR_WEIGHT, ITERATIONS, S, fixed_poses, recovery, some_flow

N_VERTICES, MIN_PAIRS = 20000, 16


@functools.lru_cache(maxsize=None)
def random_system(ah, aw, n=2, per_cell=20, seed=0):
    """test_the_host_update_at_the_papers_lattice_size's recipe -> (blocks [n, cells, 120], counts, flow): per cell the sum of
    per_cell random pairs' terms, one block of -0.0 (where there is more than one cell)."""
    rng = np.random.default_rng(seed)
    cells = (ah - 1) * (aw - 1)
    z = rng.standard_normal((n, cells, per_cell, 15))
    blocks = np.stack([[NO.block_terms(z[p, c]).sum(axis=0) for c in range(cells)] for p in range(n)])
    if cells > 1:
        blocks[0, min(7, cells - 1)] = -0.0
    counts = np.full((n, cells), per_cell, dtype=np.int32)
    return blocks, counts, rng.standard_normal((n, ah, aw, 2))


@functools.lru_cache(maxsize=None)
def random_solution(ah, aw, n=2, per_cell=20, seed=0):
    blocks, counts, flow = random_system(ah, aw, n, per_cell, seed)
    return SO.solve(blocks, counts, flow, np.ones(n, dtype=np.uint8), np.ones(n, dtype=bool), N_VERTICES, 0.316, min(MIN_PAIRS, per_cell))


@functools.lru_cache(maxsize=None)
def scene_system():
    """The systems of test_the_host_update_is_the_restatements_byte_for_byte: blocks of the scene's six poses at a random flow, pose
    2 one pair short of min_pairs, pose 3 held, pose 5 invalid."""
    V, RT, valid, color, bits = fixed_poses()
    images, flow = CO.gradients(color), some_flow(amplitude=0.5)
    flow[3] = 0.0
    prox = CO.proxy(*NO.accumulate(V, RT, valid, color, CAM, bits, flow, S, margin=MARGIN))
    blocks, counts = NO.normal(V, RT, valid, images, CAM, bits, prox, flow, S, margin=MARGIN)
    blocks, counts = blocks.copy(), counts.copy()
    counts[2] = 0
    counts[2, 0] = 15
    valid = np.array([1, 1, 1, 1, 1, 0], dtype=np.uint8)
    free = np.array([1, 1, 1, 0, 1, 1], dtype=bool)
    return blocks, counts, flow, valid, free, len(V)


def scaled_residual(A, b, x):
    """max |A x + b| / (2^-53 (|A|_inf max |x| + max |b|)), the product in extended precision"""
    r = A.astype(np.longdouble) @ x.astype(np.longdouble) + b.astype(np.longdouble)
    return float(np.abs(r).max() / (2.0 ** -53 * (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max())))


def lapack_agreement(blocks, counts, flow, x, n_vertices, anchor_weight, poses):
    out = []
    for p in poses:
        A, b = SO.system(blocks[p], flow[p], int(counts[p].sum()), n_vertices, anchor_weight)
        banded, lapack = scaled_residual(A, b, x[p]), scaled_residual(A, b, np.linalg.solve(A, -b))
        print('pose %d: %d unknowns, scaled residual %.3f banded, %.3f LAPACK' % (p, len(b), banded, lapack))
        assert banded <= 4 * max(lapack, 1.0), (p, banded, lapack)
        out.append((banded, lapack))
    return out


# ----------------------------------------------------------------------------------------------------------------- the envelope
@pytest.mark.parametrize('ah,aw', [(2, 2), (3, 6), (4, 5)])
def test_the_assembled_anchor_part_lies_inside_the_envelope(ah, aw):
    blocks, counts, flow = random_system(ah, aw)
    m, n, w, lo = SO.envelope(ah, aw)
    assert (m, n, w) == (2 * ah * aw, 2 * ah * aw + 6, 2 * aw + 3) and lo[:m] == [max(0, i - w) for i in range(m)] and lo[m:] == [0] * 6
    A, _ = SO.system(blocks[1], flow[1], int(counts[1].sum()), N_VERTICES, 0.316)
    q = np.concatenate([np.arange(6, n), np.arange(6)])
    M = A[np.ix_(q, q)]
    i, j = np.nonzero(M[:m, :m])
    assert np.abs(i - j).max() <= w and (M == M.T).all()
    if m > w + 1:
        assert np.abs(i - j).max() == w                                 # and the band is no wider than it has to be


# ------------------------------------------------------------------------------------------------------- agreement with LAPACK
@pytest.mark.parametrize('ah,aw,per_cell', [(4, 5, 20), (16, 21, 20), (4, 5, 3), (16, 21, 3)])
def test_the_banded_solve_is_as_good_as_lapack_on_random_systems(ah, aw, per_cell):
    """Both solvers are backward stable and differ in the order of their sums: the banded x's scaled residual is at most 4 x
    LAPACK's on the same system (floored at 1).  Measured on these systems: 0.01-0.45 banded against 0.01-0.32 LAPACK."""
    blocks, counts, flow = random_system(ah, aw, 2, per_cell)
    x, residual, pairs, status = random_solution(ah, aw, 2, per_cell)
    assert not status.any() and x.shape == (2, 6 + 2 * ah * aw) and x.dtype == np.float64 and status.dtype == np.int32
    assert pairs.dtype == np.int64 and pairs.tolist() == [per_cell * (ah - 1) * (aw - 1)] * 2
    assert residual.tobytes() == NO.residuals(blocks).tobytes()
    assert np.isfinite(x).all() and (x != 0).all()                      # the block of -0.0 of pose 0 is no obstacle
    lapack_agreement(blocks, counts, flow, x, N_VERTICES, 0.316, range(2))


def test_the_banded_solve_is_as_good_as_lapack_on_the_scenes_systems():
    blocks, counts, flow, valid, free, n = scene_system()
    x, residual, pairs, status = SO.solve(blocks, counts, flow, valid, free, n, 0.316, MIN_PAIRS)
    assert status.tolist() == [0, 0, P.COLORMAP_FEW_PAIRS, 0, 0, 0] and pairs[2] == 15
    lapack_agreement(blocks, counts, flow, x, n, 0.316, (0, 1, 4))
    for p in (2, 3, 5):                                                 # one pair short, held, invalid: rows of +0.0
        assert not x[p].any() and not np.signbit(x[p]).any()
    assert residual.tobytes() == NO.residuals(blocks).tobytes() and pairs.tolist() == counts.sum(axis=1).tolist()


# ------------------------------------------------------------------------------------------------------------- the special poses
def test_the_banded_update_moves_the_poses_the_dense_one_moves():
    blocks, counts, flow, valid, free, n = scene_system()
    E0 = np.stack([np.linalg.inv(p) for p in scene()[3]])

    def both(anchor_weight, blocks, same=range(6)):
        out = []
        for fn in (SO.update, NO.update):
            E, f, status = E0.copy(), flow.copy(), np.zeros(6, dtype=np.int32)
            moved = fn(E, f, valid, free, blocks, counts, n, anchor_weight, MIN_PAIRS, status)
            out.append((E, f, status, moved))
        (E, f, status, moved), (E2, f2, status2, moved2) = out
        for p in same:
            assert status[p] == status2[p] and moved[p] == moved2[p], p
        return E, f, status, moved
    E, f, status, moved = both(0.316, blocks)
    assert moved.tolist() == [True, True, False, False, True, False]
    assert status.tolist() == [0, 0, P.COLORMAP_FEW_PAIRS, 0, 0, 0]
    for p in (2, 3, 5):
        assert E[p].tobytes() == E0[p].tobytes() and f[p].tobytes() == flow[p].tobytes()
    # anchor_weight = 0 with an anchor that no pair touches: its pivot is exactly 0
    untouched = blocks.copy()
    untouched[4, 0] = 0.0
    # (without a regulariser a pose whose system is rank-deficient for OTHER reasons - an anchor with too few pairs round it - may
    # still move under LU, on a pivot that is rounding noise, and is SINGULAR under Cholesky: only pose 4 is compared)
    E, f, status, moved = both(0.0, untouched, same=(2, 3, 4, 5))
    assert status[4] == P.COLORMAP_SINGULAR and not moved[4]
    assert E[4].tobytes() == E0[4].tobytes() and f[4].tobytes() == flow[4].tobytes()
    x = SO.solve(untouched, counts, flow, valid, free, n, 0.0, MIN_PAIRS)[0]
    assert not x[4].any() and not np.signbit(x[4]).any()
    # the same anchor under the regulariser alone: pulled to zero by its own equation wgt^2 x = -wgt^2 f
    E, f, status, moved = both(0.316, untouched)
    assert moved[4] and status[4] == 0 and np.abs(f[4, 0, 0]).max() < 1e-12 and np.abs(flow[4, 0, 0]).min() > 0


def test_an_indefinite_or_nan_system_is_singular_and_leaves_the_others_alone():
    blocks, counts, flow = random_system(4, 5)
    ones = np.ones(2, dtype=np.uint8)
    want = random_solution(4, 5)[0]
    for spoil in (lambda b: -b, lambda b: np.where(np.arange(120) == 17, np.nan, b), lambda b: np.where(np.arange(120) == 3, np.inf, b)):
        bad = blocks.copy()
        bad[1] = spoil(bad[1])
        x, residual, pairs, status = SO.solve(bad, counts, flow, ones, ones.astype(bool), N_VERTICES, 0.316, MIN_PAIRS)
        assert status.tolist() == [0, P.COLORMAP_SINGULAR] and not x[1].any() and not np.signbit(x[1]).any()
        assert x[0].tobytes() == want[0].tobytes()


# ----------------------------------------------------------------------------------------------------------------------- recovery
@functools.lru_cache(maxsize=None)
def banded_recovery():
    V, C, poses, color, bits, free, _, _ = recovery()
    return SO.optimize(V, poses, color, CAM, bits, S, iterations=ITERATIONS, anchor_weight=ANCHOR_WEIGHT, free=free, margin=MARGIN)


def test_the_recovery_scene_under_the_banded_optimiser():
    """tests/test_nonrigid.py's own assertions on its recovery scene, with the banded update in the loop."""
    V, C, poses, color, bits, free, (dense_out, dense_flow, dense_info), (rigid_out, rigid_info) = recovery()
    out, flow, info = banded_recovery()
    e, e_rigid = info['residual'][:, FREED], rigid_info['residual'][:, FREED]
    print('free frame: e %.6f -> %.6f banded, %.6f dense, -> %.6f rigid only; |flow| %.3f px'
          % (e[0], e[-1], dense_info['residual'][-1, FREED], e_rigid[-1], info['flow_norm'][-1, FREED]))
    n = int(info['pairs'][0, FREED])
    assert abs(e[0] - e_rigid[0]) <= 2 * (n - 1) * 2.0 ** -53 * e[0]
    assert e[-1] < e[0]
    assert e[-1] < e_rigid[-1]
    held = [p for p in range(6) if p != FREED]
    assert out[held].tobytes() == poses[held].tobytes() and not flow[held].any()
    assert info['status'].tolist() == [NO.NOT_FREE if p != FREED else 0 for p in range(6)]
    assert info['residual'].shape == info['pairs'].shape == info['flow_norm'].shape == (ITERATIONS + 1, 6)
    assert not info['flow_norm'][0].any() and 0.5 < info['flow_norm'][-1, FREED] < 3.0 and not info['flow_norm'][:, held].any()
    assert info['solver'] == 'banded'
    assert info['residual'][0].tobytes() == dense_info['residual'][0].tobytes()          # the same start, whatever the solver


# ---------------------------------------------------------------------------------------------------------------------- arguments
def test_solver_argument_errors_are_raised_before_any_library_call(tmp_path):
    V, _, _, poses, color, depth, bits = scene()
    v, c, d = torch.from_numpy(V), torch.from_numpy(color), torch.from_numpy(depth)
    kw = dict(color_camera=CAM, margin=MARGIN)
    assert P.NONRIGID_SOLVERS == ('dense', 'banded')
    for wrong in ('sparse', None, 'Banded'):
        with pytest.raises(ValueError, match="solver must be 'dense' or 'banded'"):
            P.optimize_poses_nonrigid(v, poses, c, depth=d, solver=wrong, **kw)
    for right in P.NONRIGID_SOLVERS:                                   # accepted: the next check speaks (CPU tensors)
        with pytest.raises(TypeError, match='color must be a CUDA tensor'):
            P.optimize_poses_nonrigid(v, poses, c, depth=d, solver=right, **kw)
    with pytest.raises(ValueError, match="nonrigid_solver must be 'dense' or 'banded'"):
        P.scan_vertex_colors(v, str(tmp_path / 'nowhere'), nonrigid_iterations=2, nonrigid_solver='lu')
    blocks, counts, flow = (torch.from_numpy(a) for a in random_system(4, 5))
    ones = torch.ones(2, dtype=torch.uint8)
    with pytest.raises(ValueError, match='flow must be a CUDA tensor'):
        P.nonrigid_solve(blocks, counts, flow, ones, ones, N_VERTICES, 0.316, MIN_PAIRS)
    with pytest.raises(ValueError, match='flow must be a float64 CUDA tensor'):
        P.nonrigid_solve(blocks, counts, flow[0], ones, ones, N_VERTICES, 0.316, MIN_PAIRS)
