"""The harmonic fill's numpy restatement (tests/_harmonic_oracle.py, written from include/stin_hip.h, "Harmonic fill") held to first
principles on the CPU: what a harmonic extension must be on graphs where it is known in closed form, the reach rule on a hand-made
graph, the per-channel stop and freeze rules, and agreement with a dense solve.

The error bound is derived in the test, never in advance: a channel stops at ||r|| <= tol ||b||, which bounds the relative error
||x - x*|| / ||x*|| by cond(A) tol (cond from np.linalg.cond on that very matrix); a factor of 2 on top covers the rounding of the
recurrence, and the float32 result adds half an ulp (2^-24) per entry."""
import numpy as np
import pytest

import _harmonic_oracle as H

TOL = 1e-10


def error_bound(A, x_star, tol):
    return 2.0 * np.linalg.cond(A) * tol * np.linalg.norm(x_star) + 2.0 ** -24 * np.linalg.norm(x_star)


def solved(ei, n, values, masked, weight=None, tol=TOL, **kw):
    rowptr, col, _ = H.csr(ei, n)
    out, state = H.solve(rowptr, col, weight, values, masked, tol=tol, **kw)
    return rowptr, col, out, state


def check_against(rowptr, col, weight, values, masked, out, x_star=None, tol=TOL):
    """Every channel of the unknown rows lies within the derived bound of x_star (default: the dense solve)."""
    A, b, unk = H.dense_system(rowptr, col, weight, values, masked)
    want = np.linalg.solve(A, b) if x_star is None else x_star[unk]
    for c in range(values.shape[1]):
        err = np.linalg.norm(out[unk, c].astype(np.float64) - want[:, c])
        assert err <= error_bound(A, want[:, c], tol), (c, err, error_bound(A, want[:, c], tol))
    return A, unk


def flags(state, c):
    return int(state[8 + 4 * c + 3])


def iterations(state, c):
    return int(state[8 + 4 * c])


# ------------------------------------------------------------------------------------------------------------- closed forms
def test_a_path_between_two_known_ends_is_the_linear_ramp():
    n = 14
    values = np.zeros((n, 2), dtype=np.float32)
    values[0], values[-1] = (1.0, -3.0), (14.0, 10.0)
    masked = np.ones(n, dtype=bool)
    masked[[0, -1]] = False
    ramp = np.stack([np.linspace(1.0, 14.0, n), np.linspace(-3.0, 10.0, n)], axis=1)
    rowptr, col, out, state = solved(H.path(n), n, values, masked)
    check_against(rowptr, col, None, values, masked, out, x_star=ramp)
    assert out[[0, -1]].tobytes() == values[[0, -1]].tobytes()
    assert all(flags(state, c) == H.F_DONE for c in range(2)) and state[1] == n - 2 and state[2] == 0


def test_an_affine_field_on_a_regular_grid_is_reproduced():
    xy, ei = H.grid4(13, 11)
    n = len(xy)
    field = np.stack([0.25 * xy[:, 0] - 0.5 * xy[:, 1] + 1.0, 0.125 * xy[:, 1] - 2.0, -0.75 * xy[:, 0]], axis=1)
    rowptr, col, _ = H.csr(ei, n)
    masked = H.hop_ball(rowptr, col, 6 * 11 + 5, 4)
    values = field.astype(np.float32)                                   # (exactly representable: multiples of 1 / 8)
    assert np.array_equal(values.astype(np.float64), field)
    values[masked] = 77.0                                               # what lies under the mask must not matter
    out, state = H.solve(rowptr, col, None, values, masked, tol=TOL)
    check_against(rowptr, col, None, values, masked, out, x_star=field)
    assert out[~masked].tobytes() == values[~masked].tobytes()


def test_a_constant_rim_gives_the_constant_and_values_stay_within_the_rim():
    V, ei = H.tri_grid(12, 12, jitter=0.2, seed=3)
    n = len(V)
    rowptr, col, _ = H.csr(ei, n)
    w = H.inverse_length_weights(V, rowptr, col)
    masked = H.hop_ball(rowptr, col, 5 * 12 + 6, 3)
    rng = np.random.default_rng(0)
    values = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    values[:, 0] = 0.625                                                # channel 0: a constant rim
    out, state = H.solve(rowptr, col, w, values, masked, tol=TOL)
    A, unk = check_against(rowptr, col, w, values, masked, out)
    const = np.full((n, 3), 0.625)
    assert np.linalg.norm(out[unk, 0] - 0.625) <= error_bound(A, const[unk, 0], TOL)
    flag = H.reach(rowptr, col, masked)
    rows = H.slot_rows(rowptr)
    rim = np.unique(col[(flag[rows] == 2) & (flag[col] == 0)])
    for c in range(3):                                                  # the maximum principle, up to the error bound
        x_star = np.linalg.solve(A, H.dense_system(rowptr, col, w, values, masked)[1][:, c])
        slack = error_bound(A, x_star, TOL)
        assert out[unk, c].min() >= values[rim, c].min() - slack and out[unk, c].max() <= values[rim, c].max() + slack


# -------------------------------------------------------------------------------------------------------------------- reach
def hand_made():
    """0 - 1 - 2 - 3 known/masked chain with a duplicate edge and a self loop; 4 isolated and masked; {5, 6, 7} a masked island with
    no known vertex; 8 known and isolated; 9 masked with nothing but a self loop."""
    ei = np.array([[0, 1, 1, 2, 2, 5, 6, 9], [1, 2, 2, 3, 2, 6, 7, 9]])
    masked = np.array([0, 1, 1, 1, 1, 1, 1, 1, 0, 1], dtype=bool)
    return ei, 10, masked


def test_reach_rule_on_a_hand_made_graph():
    ei, n, masked = hand_made()
    rowptr, col, _ = H.csr(ei, n)
    flag = H.reach(rowptr, col, masked)
    assert flag.tolist() == [0, 2, 2, 2, 1, 1, 1, 1, 0, 1]
    values = np.zeros((n, 1), dtype=np.float32)
    values[0] = 3.0
    out, state = H.solve(rowptr, col, None, values, masked, tol=TOL, fill=-9.0)
    # one known vertex on the rim: the whole reached chain takes its value; a self loop is skipped and a duplicate edge counts twice
    A, b, unk = H.dense_system(rowptr, col, None, values, masked)
    assert unk.tolist() == [1, 2, 3]
    assert A.tolist() == [[3.0, -2.0, 0.0], [-2.0, 3.0, -1.0], [0.0, -1.0, 1.0]] and b[:, 0].tolist() == [3.0, 0.0, 0.0]
    assert np.abs(out[[1, 2, 3], 0] - 3.0).max() <= error_bound(A, np.full(3, 3.0), TOL)
    assert out[[4, 5, 6, 7, 9], 0].tolist() == [-9.0] * 5 and out[[0, 8], 0].tolist() == [3.0, 0.0]
    assert state[1] == 3 and state[2] == 5 and state[4] == 8


def test_everything_or_nothing_masked():
    _, ei = H.grid4(5, 5)
    rowptr, col, _ = H.csr(ei, 25)
    values = np.random.default_rng(1).uniform(-1, 1, (25, 2)).astype(np.float32)
    out, state = H.solve(rowptr, col, None, values, np.ones(25, dtype=bool), fill=0.5)
    assert np.all(out == 0.5) and state[1] == 0 and state[2] == 25 and flags(state, 0) == H.F_DONE and iterations(state, 0) == 0
    out, state = H.solve(rowptr, col, None, values, np.zeros(25, dtype=bool))
    assert out.tobytes() == values.tobytes() and state[1] == 0 and state[2] == 0 and state[4] == 0


# ------------------------------------------------------------------------------------------------------------ stop and freeze
def three_speed_case():
    """Channel 0 has a zero right-hand side, channel 1 a constant rim (its first search direction is the solution), channel 2 a
    random rim: three different stopping iterations."""
    xy, ei = H.grid4(16, 16)
    n = len(xy)
    rowptr, col, _ = H.csr(ei, n)
    masked = H.hop_ball(rowptr, col, 8 * 16 + 8, 5)
    values = np.random.default_rng(5).uniform(-1, 1, (n, 3)).astype(np.float32)
    values[:, 0] = 0.0
    values[:, 1] = -0.25
    return rowptr, col, values, masked


def test_a_zero_right_hand_side_is_done_at_iteration_zero():
    rowptr, col, values, masked = three_speed_case()
    out, state = H.solve(rowptr, col, None, values, masked, tol=1e-8)
    assert iterations(state, 0) == 0 and flags(state, 0) == H.F_DONE and state[8 + 2] == H.bits(0.0)
    assert np.all(out[masked, 0] == 0.0)
    its = [iterations(state, c) for c in range(3)]
    assert its[0] < its[1] < its[2], its


def test_channels_that_finish_at_different_iterations_are_frozen():
    rowptr, col, values, masked = three_speed_case()
    full, state = H.solve(rowptr, col, None, values, masked, tol=1e-8)
    its = [iterations(state, c) for c in range(3)]
    for budget in sorted({its[1], its[1] + 1, its[2] - 1, its[2], its[2] + 7}):
        out, st = H.solve(rowptr, col, None, values, masked, tol=1e-8, max_iterations=budget)
        for c in range(3):
            if budget >= its[c]:                                        # done by then: the same bytes whatever follows
                assert out[:, c].tobytes() == full[:, c].tobytes() and np.array_equal(st[8 + 4 * c:12 + 4 * c], state[8 + 4 * c:12 + 4 * c])
            else:
                assert flags(st, c) == H.F_NOTCONV and iterations(st, c) == budget
    for c in range(3):                                                  # scalars of its own: a channel alone gives the same bytes
        alone, st = H.solve(rowptr, col, None, values[:, c:c + 1], masked, tol=1e-8)
        assert alone[:, 0].tobytes() == full[:, c].tobytes() and np.array_equal(st[8:12], state[8 + 4 * c:12 + 4 * c])


# -------------------------------------------------------------------------------------------------------------- dense solve
@pytest.mark.parametrize('tol', [1e-6, 1e-10])
@pytest.mark.parametrize('weights', ['uniform', 'inverse_length'])
def test_agrees_with_the_dense_solve(weights, tol):
    V, ei = H.tri_grid(20, 18, sx=3.0, sy=1.0, jitter=0.25, seed=11)
    n = len(V)
    rowptr, col, _ = H.csr(ei, n)
    w = H.inverse_length_weights(V, rowptr, col) if weights == 'inverse_length' else None
    masked = H.hop_ball(rowptr, col, 10 * 18 + 9, 6) | H.hop_ball(rowptr, col, 2 * 18 + 3, 2)
    values = np.random.default_rng(7).uniform(-1, 1, (n, 3)).astype(np.float32)
    out, state = H.solve(rowptr, col, w, values, masked, tol=tol)
    check_against(rowptr, col, w, values, masked, out, tol=tol)
    assert all(flags(state, c) == H.F_DONE for c in range(3))
    A, b, unk = H.dense_system(rowptr, col, w, values, masked)
    assert np.array_equal(A, A.T) and np.all(np.linalg.eigvalsh(A) > 0)


def test_bad_inputs_raise():
    _, ei = H.grid4(4, 4)
    rowptr, col, _ = H.csr(ei, 16)
    values = np.ones((16, 1), dtype=np.float32)
    masked = np.zeros(16, dtype=bool)
    masked[5] = True
    for bad in (0.0, -1.0, np.nan, np.inf):
        w = np.ones(len(col))
        w[rowptr[5]] = bad
        with pytest.raises(ValueError):
            H.solve(rowptr, col, w, values, masked)
    w = np.ones(len(col))
    w[rowptr[0]] = np.nan                                               # a weight no unknown's row uses is never looked at
    H.solve(rowptr, col, w, values, masked)
    values[col[rowptr[5]]] = np.inf
    with pytest.raises(ValueError):
        H.solve(rowptr, col, None, values, masked)


# ---------------------------------------------------------------------------------------------------------------- the tree
def test_the_tile_tree_is_the_header_s():
    rng = np.random.default_rng(2)
    for n in (0, 1, 255, 256, 257, 700):
        a, b = rng.standard_normal((n, 2)), rng.standard_normal((n, 2))
        want = np.zeros(2)
        for c in range(2):
            acc = 0.0
            for t in range((n + 255) // 256):
                s = [float(a[u, c] * b[u, c]) if u < n else 0.0 for u in range(256 * t, 256 * t + 256)]
                h = 128
                while h >= 1:
                    for j in range(h):
                        s[j] += s[j + h]
                    h //= 2
                acc += s[0]
            want[c] = acc
        assert H.tile_dot(a, b).tobytes() == want.tobytes()
