"""The harmonic fill on the GPU (csrc/stin_harmonic.hip through preprocessing.harmonic_fill / harmonic_inpaint): the output equals the
numpy restatement of the contract (tests/_harmonic_oracle.py) by tobytes() and the device's state table equals it by array_equal.

Sizes cross the kernel's edges, not the workload's: a tile is 256 unknowns (0, 1, 255, 256, 257 unknowns), the tile sums are folded
by every workgroup (more than 256 tiles: 66 564 unknowns, compared after 20 iterations in the not-converged state), the kernels are
instantiated for 1, 2, 3, 4, 8 and 16 channels (C = 1, 3, 5, 16), a reach round moves one hop (a 1025-chain), a row is one lane's
loop (degree 300)."""
import functools

import numpy as np
import pytest
import torch

import _harmonic_oracle as H
from surface_texture_inpainting_net_amd import metrics, preprocessing as P

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(ei, n, values, masked, weights='uniform', V=None, **kw):
    """harmonic_fill on the device and the oracle on the device's own CSR -> (out tensor, info, want out, want state)."""
    inv = isinstance(weights, str) and weights == 'inverse_length'
    adj = P.harmonic_adjacency(dev(ei), n, vertices=dev(V.astype(np.float32)) if inv else None)
    rowptr, col = adj[0].cpu().numpy(), adj[1].cpu().numpy()
    want_rowptr, want_col, _ = H.csr(ei, n)
    assert np.array_equal(rowptr, want_rowptr) and np.array_equal(col, want_col)
    if inv:
        w = H.inverse_length_weights(V.astype(np.float32), rowptr, col)
    else:
        w = None if isinstance(weights, str) else weights
    okw = {k: v for k, v in kw.items() if k in ('tol', 'max_iterations', 'fill')}
    want, state = H.solve(rowptr, col, w, values, masked, **okw)
    got, info = P.harmonic_fill(dev(values), dev(masked), adjacency=adj, weights=weights if w is None or inv else dev(w),
                                return_info=True, **kw)
    return got, info, want, state


def same(got, info, want, state):
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == want.shape
    assert np.array_equal(np.asarray(info['state'], dtype=np.int64), state), (info['state'][:16], state[:16].tolist())
    assert got.cpu().numpy().tobytes() == want.tobytes()


def rng_values(n, C, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (n, C)).astype(np.float32)


# --------------------------------------------------------------------------------------------------------- 1: tile boundaries
@pytest.mark.parametrize('n_unknown', [1, 255, 256, 257])
def test_unknown_counts_around_a_tile(n_unknown):
    """A ladder (two rails with rungs): the upper rail known, n_unknown vertices of the lower rail masked."""
    m = n_unknown + 3
    ei = np.concatenate([H.path(m), H.path(m) + m, np.stack([np.arange(m), np.arange(m) + m])], axis=1)
    masked = np.zeros(2 * m, dtype=bool)
    masked[m + 1:m + 1 + n_unknown] = True
    got, info, want, state = run(ei, 2 * m, rng_values(2 * m, 3, n_unknown), masked, tol=1e-8)
    assert info['n_unknown'] == n_unknown and info['converged']
    same(got, info, want, state)


def test_nothing_masked_and_everything_masked():
    _, ei = H.grid4(9, 7)
    values = rng_values(63, 3, 1)
    got, info, want, state = run(ei, 63, values, np.zeros(63, dtype=bool))
    same(got, info, want, state)
    assert got.cpu().numpy().tobytes() == values.tobytes() and info['n_unknown'] == 0 and info['iterations'] == [0, 0, 0]
    got, info, want, state = run(ei, 63, values, np.ones(63, dtype=bool), fill=0.25)
    same(got, info, want, state)
    assert bool((got == 0.25).all()) and info['n_unreached'] == 63 and info['n_unknown'] == 0


def test_more_than_256_tiles_compared_before_convergence():
    xy, ei = H.grid4(260, 260)
    n = len(xy)
    masked = ((xy[:, 0] > 0) & (xy[:, 0] < 259) & (xy[:, 1] > 0) & (xy[:, 1] < 259))
    got, info, want, state = run(ei, n, rng_values(n, 1, 2), masked, max_iterations=20)
    assert info['n_unknown'] == 258 * 258 > 256 * 256 and info['flags'] == [H.F_NOTCONV] and info['iterations'] == [20]
    same(got, info, want, state)


# ----------------------------------------------------------------------------------------------------------------- 2: channels
@functools.lru_cache(maxsize=None)
def hole_grid():
    xy, ei = H.grid4(24, 21)
    rowptr, col, _ = H.csr(ei, len(xy))
    return ei, len(xy), H.hop_ball(rowptr, col, 12 * 21 + 10, 7)


@pytest.mark.parametrize('C', [1, 3, 5, 16])
def test_channel_counts(C):
    ei, n, masked = hole_grid()
    values = rng_values(n, C, 10 + C)
    if C >= 3:
        values[:, 1] = 0.0                                              # a zero right-hand side: done at iteration 0
        values[:, 2] = 0.5                                              # a constant rim: done long before the others
    got, info, want, state = run(ei, n, values, masked)
    same(got, info, want, state)
    assert info['converged'] and (C < 3 or info['iterations'][1] == 0 < info['iterations'][2] < info['iterations'][0])


@pytest.mark.parametrize('ips', [1, 7])
def test_grouping_of_the_launches_does_not_change_a_byte(ips):
    ei, n, masked = hole_grid()
    values = rng_values(n, 3, 13)
    values[:, 1], values[:, 2] = 0.0, 0.5
    got, info, want, state = run(ei, n, values, masked, iterations_per_sync=ips)
    same(got, info, want, state)
    # no host read at all: more iterations than any channel needs, every channel frozen when it is done
    out, status = P.harmonic_fill(dev(values), dev(masked), edge_index=dev(ei), max_iterations=max(info['iterations']) + 9,
                                  iterations_per_sync=None)
    assert out.cpu().numpy().tobytes() == want.tobytes() and np.array_equal(status.cpu().numpy(), state)


# ------------------------------------------------------------------------------------------------------------------- 3: graphs
def test_a_1025_chain_needs_many_reach_rounds():
    n = 1025
    masked = np.ones(n, dtype=bool)
    masked[0] = False
    got, info, want, state = run(H.path(n), n, rng_values(n, 2, 3), masked, max_iterations=40)
    assert info['n_unknown'] == 1024 and info['n_unreached'] == 0
    same(got, info, want, state)


def test_a_row_of_degree_300():
    """Hub 0 (masked) with 300 leaves, every third leaf masked too; the leaves form a ring."""
    leaves = np.arange(1, 301)
    ei = np.concatenate([np.stack([np.zeros(300, dtype=np.int64), leaves]), np.stack([leaves, np.roll(leaves, 1)])], axis=1)
    masked = np.zeros(301, dtype=bool)
    masked[0] = True
    masked[1::3] = True
    got, info, want, state = run(ei, 301, rng_values(301, 3, 4), masked, tol=1e-9)
    same(got, info, want, state)
    assert info['converged']


def test_jittered_anisotropic_grid_with_inverse_length_weights():
    V, ei = H.tri_grid(40, 40, sx=10.0, sy=1.0, jitter=0.2, seed=6)
    n = len(V)
    rowptr, col, _ = H.csr(ei, n)
    masked = H.hop_ball(rowptr, col, 20 * 40 + 20, 8)
    values = rng_values(n, 3, 5)
    got, info, want, state = run(ei, n, values, masked, weights='inverse_length', V=V)
    same(got, info, want, state)
    assert info['converged']
    uni, _, _, _ = run(ei, n, values, masked)
    assert not torch.equal(uni, got)                                    # the weights do something
    # the same through edge_index + vertices, and explicit weights
    again = P.harmonic_fill(dev(values), dev(masked), edge_index=dev(ei), vertices=dev(V.astype(np.float32)), weights='inverse_length')
    assert torch.equal(again, got)
    w = H.inverse_length_weights(V.astype(np.float32), rowptr, col)
    got_w, info_w, want_w, state_w = run(ei, n, values, masked, weights=w)
    same(got_w, info_w, want_w, state_w)
    assert torch.equal(got_w, got)


@functools.lru_cache(maxsize=None)
def sphere_two_holes():
    V, ei = H.icosphere(3)
    rowptr, col, _ = H.csr(ei, len(V))
    masked = H.hop_ball(rowptr, col, int(np.argmax(V[:, 2])), 4) | H.hop_ball(rowptr, col, int(np.argmin(V[:, 2])), 3)
    return V, ei, masked


def test_icosphere_with_two_disjoint_holes():
    V, ei, masked = sphere_two_holes()
    values = (V * np.array([1.0, 0.5, -0.25])).astype(np.float32)
    got, info, want, state = run(ei, len(V), values, masked, weights='inverse_length', V=V, tol=1e-8)
    same(got, info, want, state)
    assert info['converged'] and 0 < info['n_unknown'] < len(V)


def test_a_batch_of_two_graphs_and_an_island_without_a_rim():
    """The disjoint union of the sphere (two holes) and a grid whose hole touches nothing known PLUS a wholly masked third
    component: the island and an isolated masked vertex get `fill`."""
    V, ei_a, masked_a = sphere_two_holes()
    ei_b, nb, masked_b = hole_grid()
    na = len(V)
    island = H.path(6) + na + nb
    n = na + nb + 6 + 1                                                 # ... and one isolated vertex at the end
    ei = np.concatenate([ei_a, ei_b + na, island], axis=1)
    masked = np.concatenate([masked_a, masked_b, np.ones(7, dtype=bool)])
    values = rng_values(n, 3, 8)
    got, info, want, state = run(ei, n, values, masked, fill=-2.0)
    same(got, info, want, state)
    assert info['n_unreached'] == 7 and bool((got[-7:] == -2.0).all())
    # each graph alone gives the rows it gives in the batch only up to the stop rule (one global solve: shared scalars);
    # the known rows are the input bit for bit
    assert torch.equal(got[~dev(masked)], dev(values)[~dev(masked)])


def test_self_loops_and_duplicate_edges():
    ei = np.array([[0, 1, 1, 2, 2, 5, 6, 9], [1, 2, 2, 3, 2, 6, 7, 9]])
    masked = np.array([0, 1, 1, 1, 1, 1, 1, 1, 0, 1], dtype=bool)
    values = rng_values(10, 2, 9)
    got, info, want, state = run(ei, 10, values, masked, fill=7.0)
    same(got, info, want, state)
    assert info['n_unknown'] == 3 and info['n_unreached'] == 5


# ------------------------------------------------------------------------------------------------------------------- 4: errors
def test_error_cases():
    ei, n, masked = hole_grid()
    values = rng_values(n, 2, 20)
    adj = P.harmonic_adjacency(dev(ei), n)
    rowptr, col = adj[0].cpu().numpy(), adj[1].cpu().numpy()
    v = int(np.nonzero(masked)[0][0])
    for bad in (0.0, float('nan')):
        w = np.ones(len(col))
        w[rowptr[v]] = bad
        with pytest.raises(ValueError, match='weight'):
            P.harmonic_fill(dev(values), dev(masked), adjacency=adj, weights=dev(w))
    flag = H.reach(rowptr, col, masked)
    rows = H.slot_rows(rowptr)
    rim = int(col[(flag[rows] == 2) & (flag[col] == 0)][0])
    poisoned = values.copy()
    poisoned[rim, 1] = np.inf
    with pytest.raises(ValueError, match='finite'):
        P.harmonic_fill(dev(poisoned), dev(masked), adjacency=adj)
    with pytest.raises(TypeError):
        P.harmonic_fill(torch.from_numpy(values), torch.from_numpy(masked), edge_index=torch.from_numpy(ei))
    with pytest.raises(ValueError):
        P.harmonic_fill(dev(rng_values(n, 17, 21)), dev(masked), adjacency=adj)
    with pytest.raises(ValueError):
        P.harmonic_fill(dev(values), dev(masked), adjacency=adj, weights='cotangent')


# ----------------------------------------------------------------------------------------------------------------- 5: baseline
class Sample:
    pass


def test_harmonic_inpaint_feeds_step_metrics():
    V, ei = H.tri_grid(30, 30, jitter=0.2, seed=12)
    n = len(V)
    rowptr, col, _ = H.csr(ei, n)
    hole = H.hop_ball(rowptr, col, 15 * 30 + 15, 6)
    color = np.stack([np.sin(V[:, 0] / 5.0), np.cos(V[:, 1] / 7.0), 0.02 * V[:, 0] - 0.3], axis=1).astype(np.float32)
    s = Sample()
    s.color, s.mask, s.edge_index = dev(color), dev(hole.astype(np.int64) * 3).reshape(-1, 1), dev(np.concatenate([ei, ei[::-1]], axis=1))
    s.x = torch.cat([torch.zeros(n, 6, device=DEV), dev(V.astype(np.float32)), torch.ones(n, 1, device=DEV)], dim=1)
    m = metrics.StepMetrics(DEV, capacity=4)
    keys = metrics.StepMetrics.KEYS
    row_const = m.update(torch.zeros_like(s.color), s, composite=True).cpu()
    for weights in ('uniform', 'inverse_length'):
        got = P.harmonic_inpaint(s, weights=weights)
        assert got.dtype == torch.float32 and torch.equal(got[~dev(hole)], s.color[~dev(hole)])
        for composite in (False, True):
            row = m.update(got, s, composite=composite).cpu()
            assert bool(torch.isfinite(row).all())
            assert float(row[keys.index('l1')]) < float(row_const[keys.index('l1')])
    s.pos = dev(V.astype(np.float32))
    assert torch.equal(P.harmonic_inpaint(s, weights='inverse_length'), got)
