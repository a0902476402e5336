"""The banded solve of the non-rigid colour-map optimisation on the GPU (csrc/stin_nonrigid_solve.hip through
preprocessing.nonrigid_solve and optimize_poses_nonrigid(solver='banded')): equal to the numpy restatement of its contract
(tests/_nonrigid_solve_oracle.py) byte for byte - `tobytes()` of x, residual, pairs and status at every lattice shape the window
treats differently, for every state a pose can be in and every batching, and of the poses, flows and info of a whole
optimisation; the dense solver beside it still equals its own restatement."""
import functools

import numpy as np
import pytest
import torch

import _nonrigid_oracle as NO
import _nonrigid_solve_oracle as SO
from surface_texture_inpainting_net_amd import _lib, preprocessing as P
from test_colormap import CAM, MARGIN
from test_nonrigid import ANCHOR_WEIGHT, ITERATIONS, S, recovery
from test_nonrigid_solve import MIN_PAIRS, N_VERTICES, banded_recovery, random_solution, random_system

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_bits(b):
    return dev(np.ascontiguousarray(b).view(np.int32)).view(torch.uint32)


def gpu_solve(blocks, counts, flow, valid, free, n_vertices=N_VERTICES, anchor_weight=0.316, min_pairs=MIN_PAIRS):
    out = P.nonrigid_solve(dev(blocks), dev(counts), dev(flow), dev(np.asarray(valid, dtype=np.uint8)), dev(np.asarray(free, dtype=bool)),
                           n_vertices, anchor_weight, min_pairs)
    assert [t.dtype for t in out] == [torch.float64, torch.float64, torch.int64, torch.int32] and all(t.is_cuda for t in out)
    return tuple(t.cpu().numpy() for t in out)


def same(got, want):
    for g, w, name in zip(got, want, ('x', 'residual', 'pairs', 'status')):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert g.tobytes() == w.tobytes(), (name, np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))[:8])


# ------------------------------------------------------------------------------------------------------------------ lattices
@pytest.mark.parametrize('ah,aw', [(2, 2), (3, 6), (4, 5), (2, 41), (16, 21)])
def test_every_lattice_shape_is_the_restatement(ah, aw):
    """2 x 2: one cell, the band wider than the matrix; 3 x 6: ragged; 2 x 41: the widest band on the fewest rows; 16 x 21: the
    paper's size, two poses, the window slides over 600 times."""
    blocks, counts, flow = random_system(ah, aw)
    want = random_solution(ah, aw)
    assert not want[3].any() and want[0].all()
    same(gpu_solve(blocks, counts, flow, [1, 1], [True, True]), want)


# ----------------------------------------------------------------------------------------------------------------- pose states
@functools.lru_cache(maxsize=None)
def states(n, seed=1):
    """n poses at 4 x 5 in a cycle of six states: solved, held, invalid, few pairs, singular (its blocks negated: the first pivot is
    negative), a NaN in one block."""
    blocks, counts, flow = (a.copy() for a in random_system(4, 5, n, 20, seed))
    valid, free = np.ones(n, dtype=np.uint8), np.ones(n, dtype=bool)
    for p in range(n):
        k = p % 6
        if k == 1:
            free[p] = False
        elif k == 2:
            valid[p] = 0
        elif k == 3:
            counts[p] = 0
            counts[p, p % 12] = MIN_PAIRS - 1                              # one pair short
        elif k == 4:
            blocks[p] = -blocks[p]
        elif k == 5:
            blocks[p, (p // 6) % 12, (7 * p) % 119] = np.nan
    want = SO.solve(blocks, counts, flow, valid, free, N_VERTICES, 0.316, MIN_PAIRS)
    return blocks, counts, flow, valid, free, want


@pytest.mark.parametrize('n', [1, 6, 70])
def test_every_pose_state_and_batch_size(n):
    blocks, counts, flow, valid, free, want = states(n)
    x, residual, pairs, status = want
    cycle = [0, 0, 0, P.COLORMAP_FEW_PAIRS, P.COLORMAP_SINGULAR, P.COLORMAP_SINGULAR]
    assert status.tolist() == [cycle[p % 6] for p in range(n)]
    assert all(x[p].all() == (p % 6 == 0) and (p % 6 == 0 or not (x[p].any() or np.signbit(x[p]).any())) for p in range(n))
    got = gpu_solve(blocks, counts, flow, valid, free)
    same(got, want)
    if n >= 6:
        assert pairs[3] == MIN_PAIRS - 1 and np.isfinite(residual).all() and (residual[4::6] < 0).all()     # written for every pose


def test_poses_solved_separately_equal_those_solved_at_once():
    blocks, counts, flow, valid, free, want = states(6)
    parts = [gpu_solve(blocks[a:b], counts[a:b], flow[a:b], valid[a:b], free[a:b]) for a, b in ((0, 3), (3, 6))]
    same(tuple(np.concatenate(k) for k in zip(*parts)), want)
    neighbours = states(6)[0].copy()
    neighbours[5] = random_system(4, 5, 6, 20, 1)[0][5]                 # without the NaN: pose 0 .. 4 are unaffected by it
    clean = gpu_solve(neighbours, counts, flow, valid, free)
    assert clean[0][:5].tobytes() == want[0][:5].tobytes() and clean[3][5] == 0 and clean[0][5].all()


def test_the_untouched_anchor_under_both_weights():
    blocks, counts, flow = (a.copy() for a in random_system(4, 5))
    blocks[1, 0] = 0.0                                                  # no pair in the cell round anchor (0, 0) of pose 1
    for anchor_weight, status in ((0.0, [0, P.COLORMAP_SINGULAR]), (0.316, [0, 0])):
        want = SO.solve(blocks, counts, flow, [1, 1], [True, True], N_VERTICES, anchor_weight, MIN_PAIRS)
        assert want[3].tolist() == status
        same(gpu_solve(blocks, counts, flow, [1, 1], [True, True], anchor_weight=anchor_weight), want)
    assert np.abs(want[0][1, 6:8] + flow[1, 0, 0]).max() < 1e-12        # pulled to zero by wgt^2 x = -wgt^2 f alone


# -------------------------------------------------------------------------------------------------------------------- arguments
def test_an_unsupported_lattice_and_wrong_arrays_are_refused():
    cap = _lib.CONSTANTS['STIN_NONRIGID_SOLVE_MAX_AW']
    assert cap >= 41
    lib = _lib.load()
    assert lib.stin_nonrigid_solve_workspace_bytes(1, 2, cap) > 0 and lib.stin_nonrigid_solve_workspace_bytes(128, 16, 21) > 0
    assert lib.stin_nonrigid_solve_workspace_bytes(1, 2, cap + 1) == 0 and lib.stin_nonrigid_solve_workspace_bytes(1, 1, 5) == 0
    assert lib.stin_nonrigid_solve_workspace_bytes(1, 5, 1) == 0 and lib.stin_nonrigid_solve_workspace_bytes(-1, 4, 5) == 0
    cells = cap
    blocks, counts = torch.zeros(1, cells, 120, dtype=torch.float64, device=DEV), torch.zeros(1, cells, dtype=torch.int32, device=DEV)
    flow, ones = torch.zeros(1, 2, cap + 1, 2, dtype=torch.float64, device=DEV), torch.ones(1, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="solver='dense'"):
        P.nonrigid_solve(blocks, counts, flow, ones, ones, 100, 0.316, 1)
    with pytest.raises(ValueError, match='blocks must be float64'):
        P.nonrigid_solve(blocks[:, :-1], counts, flow, ones, ones, 100, 0.316, 1)
    with pytest.raises(ValueError, match='counts must be int32'):
        P.nonrigid_solve(blocks, counts.long(), flow, ones, ones, 100, 0.316, 1)
    with pytest.raises(ValueError, match='free must be uint8'):
        P.nonrigid_solve(blocks, counts, flow, ones, ones[:0], 100, 0.316, 1)
    empty = P.nonrigid_solve(blocks[:0, :4], counts[:0, :4], flow[:0, :, :5], ones[:0], ones[:0], 100, 0.316, 1)
    assert [tuple(t.shape) for t in empty] == [(0, 26), (0,), (0,), (0,)]
    # a frame whose default-size lattice is too wide for the banded solve: 2 x 43 anchors at step 1 over 2 x 43 pixels
    v = torch.zeros(4, 3, dtype=torch.float64, device=DEV)
    color, bits = torch.zeros(1, 2, 43, 3, dtype=torch.uint8, device=DEV), torch.ones(4, 1, dtype=torch.int32, device=DEV).view(torch.uint32)
    with pytest.raises(ValueError, match="solver='dense'"):
        P.optimize_poses_nonrigid(v, np.eye(4)[None], color, bits=bits, color_camera=CAM, margin=1, lattice_step=1, iterations=1,
                                  solver='banded')


# ------------------------------------------------------------------------------------------------------------------- end to end
def equal(got, want):
    (gp, gf, gi), (wp, wf, wi) = got, want
    assert gp.dtype == np.float64 and gf.dtype == np.float64 and gp.shape == wp.shape and gf.shape == wf.shape
    for k in ('pairs', 'residual', 'status', 'flow_norm'):
        assert gi[k].dtype == wi[k].dtype and gi[k].tobytes() == wi[k].tobytes(), k
    assert gi['solver'] == wi.get('solver', 'dense')
    assert gf.tobytes() == wf.tobytes() and gp.tobytes() == wp.tobytes()


def test_whole_optimisations_under_both_solvers_are_their_restatements():
    V, C, poses, color, bits, free, dense_want, _ = recovery()
    kw = dict(bits=dev_bits(bits), color_camera=CAM, margin=MARGIN, iterations=ITERATIONS, lattice_step=S, anchor_weight=ANCHOR_WEIGHT,
              free=free)
    want = banded_recovery()
    for batch in (2, 6):
        equal(P.optimize_poses_nonrigid(dev(V), poses, dev(color), solver='banded', batch=batch, **kw), want)
    equal(P.optimize_poses_nonrigid(dev(V), poses, dev(color), solver='dense', batch=6, **kw), dense_want)
    equal(P.optimize_poses_nonrigid(dev(V), poses, dev(color), batch=2, **kw), dense_want)                # the default
    assert want[1].tobytes() != dense_want[1].tobytes()                 # two solvers, two roundings
