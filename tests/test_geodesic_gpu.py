"""Geodesic circle masks on the GPU (csrc/stin_geodesic.hip through preprocessing.geodesic_adjacency / geodesic_distance /
circle_mask_from_centres_geodesic / circle_masks_geodesic): equal to the restatement of the contract (tests/_geodesic_oracle.py) as
bytes - distances by tobytes(), +inf included, masks by array_equal.

Sizes cross the kernel's edges, not the workload's: a workgroup takes up to 256 worklist entries and keeps 2048 in LDS, so a star of
5000 leaves overflows the LDS frontier and shares one row out over the whole workgroup; a checkerboard of 80 000 sources lists
more than 256 x 256 vertices for one round, the size at which a workgroup loops over several full slices; a chain needs as many
rounds as it has vertices (divided by the LDS levels per round); a ladder lowers vertices again long after their first value;
`levels` 1 and 3 run the same cases on other schedules."""
import functools
import math

import numpy as np
import pytest
import torch

import _geodesic_oracle as GO
import _qem_oracle as QO
import _surface_oracle as SO
from surface_texture_inpainting_net_amd import preprocessing as P

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bytes(got, want):
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == want.shape
    assert got.cpu().numpy().tobytes() == np.ascontiguousarray(want).tobytes()


@functools.lru_cache(maxsize=None)
def graph(name):
    """-> (vertices, edge_index, weighted adjacency of the oracle)"""
    if name == 'kite':
        V, ei = GO.kite()
    elif name == 'ladder':
        V, ei = GO.ladder_with_shortcut(300)
    elif name == 'chain':
        V, ei = GO.chain(1025)
    elif name in ('grid', 'grid-10:1'):
        V, F = GO.grid_mesh(40, 40, 1.0, 1.0 if name == 'grid' else 0.1, jitter=0.3, seed=2)
        ei = SO.mesh_edges(F)
    elif name == 'icosphere':
        V, F = QO.icosphere(3)
        ei = SO.mesh_edges(F)
    elif name == 'star':
        V, ei = GO.double_star()
    elif name == 'degenerate':
        V, ei = GO.degenerate()
    return V, ei, GO.weighted_adjacency(V, ei)


@functools.lru_cache(maxsize=None)
def want(name, sources, cap=math.inf):
    return GO.dijkstra(graph(name)[2], list(sources), cap)


def check(name, sources, cap=None, **kw):
    V, ei, _ = graph(name)
    got = P.geodesic_distance(dev(V), list(sources), edge_index=dev(ei), max_distance=cap, **kw)
    same_bytes(got, want(name, tuple(sources), math.inf if cap is None else cap))
    return got


# ------------------------------------------------------------------------------------------------------------------ distances
def test_lengths_are_the_oracles_and_symmetric():
    V, ei, _ = graph('grid-10:1')
    rowptr, col, length = P.geodesic_adjacency(dev(V), edge_index=dev(ei))
    assert rowptr.dtype == torch.int32 and col.dtype == torch.int32 and length.dtype == torch.float64
    assert int(rowptr[-1]) == col.numel() == length.numel() == 2 * ei.shape[1]
    rp, c, ln = rowptr.cpu().numpy(), col.cpu().numpy().astype(np.int64), length.cpu().numpy()
    row = np.repeat(np.arange(len(V)), np.diff(rp))
    assert ln.tobytes() == GO.edge_lengths(V, np.stack([row, c])).tobytes()
    assert ln.tobytes() == GO.edge_lengths(V, np.stack([c, row])).tobytes()
    by_pair = {}
    for u, w, l in zip(row.tolist(), c.tolist(), ln.tolist()):
        assert by_pair.setdefault((min(u, w), max(u, w)), l) == l


def test_kite_where_the_hop_metric_and_the_edge_metric_disagree():
    got = check('kite', (0,))
    assert got.tolist() == [0.0, 1.0, 2.0, 3.0]
    check('kite', (0,), cap=2.5)
    V, ei, _ = graph('kite')
    hops = 4 - P.circle_mask_from_centres(dev(ei), 4, 4, [0]).cpu().numpy()
    assert hops.tolist() == [0, 1, 2, 1]                                 # one hop to vertex 3, the farthest by length


@pytest.mark.parametrize('levels', (1, 3, None))
def test_ladder_whose_vertices_are_lowered_again_many_rounds_later(levels):
    V, ei, _ = graph('ladder')
    got, info = P.geodesic_distance(dev(V), [0], edge_index=dev(ei), levels=levels, return_info=True)
    same_bytes(got, want('ladder', (0,)))
    directed = 2 * ei.shape[1]
    assert info['relaxed'] > 1.1 * directed                             # > 30 of the 300 vertices were expanded twice
    assert 139 / (levels or P.GEODESIC_LEVELS) <= info['rounds'] <= 300


@pytest.mark.parametrize('levels', (1, None))
def test_chain_runs_as_many_rounds_as_it_is_long(levels):
    V, ei, _ = graph('chain')
    got, info = P.geodesic_distance(dev(V), [0], edge_index=dev(ei), levels=levels, return_info=True)
    same_bytes(got, want('chain', (0,)))
    lv = levels or P.GEODESIC_LEVELS
    assert 1024 // lv <= info['rounds'] <= 1025 and info['launched'] >= info['rounds']
    assert bool(torch.all(got[1:] > got[:-1]))


def test_chain_with_max_rounds_reports_not_converged_and_raises_nothing():
    V, ei, _ = graph('chain')
    got, status = P.geodesic_distance(dev(V), [0], edge_index=dev(ei), max_rounds=8)
    assert status.dtype == torch.int64 and status.is_cuda and status.numel() == 4
    st = status.tolist()
    assert st[0] & 4 and st[1] >= 1 and st[2] == 8                      # not converged, somebody waits, every round found work
    full = want('chain', (0,))
    g = got.cpu().numpy()
    reached = np.isfinite(g)
    assert 8 <= reached.sum() <= 8 * P.GEODESIC_LEVELS + 1 and reached[:reached.sum()].all()
    assert g[reached].tobytes() == full[reached].tobytes()               # what is there is final: a chain has one path
    got2, status2 = P.geodesic_distance(dev(V), [0], edge_index=dev(ei), max_rounds=1100)
    same_bytes(got2, full)
    st2 = status2.tolist()
    assert st2[0] == 0 and st2[1] == 0 and st2[2] <= 1025                # converged; the rounds after that returned at once


@pytest.mark.parametrize('name,cap', (('grid', None), ('grid', 9.0), ('grid-10:1', None), ('grid-10:1', 4.0)))
def test_jittered_grids(name, cap):
    got = check(name, (41, 1311), cap=cap)
    inside = torch.isfinite(got).sum().item()
    assert (inside == 1600) if cap is None else (100 < inside < 1500)
    check(name, (41, 1311), cap=cap, levels=1)


def test_icosphere_instances_equal_separate_calls_and_the_oracle():
    V, ei, _ = graph('icosphere')
    rng = np.random.default_rng(3)
    sources = rng.choice(len(V), 12, replace=False)
    inst = np.array([0, 1, 2, 0, 1, 2, 2, 2, 0, 1, 2, 2])
    adj = P.geodesic_adjacency(dev(V), edge_index=dev(ei))
    for cap in (None, 0.9):
        got = P.geodesic_distance(dev(V), sources, max_distance=cap, source_instance=inst, num_instances=3, adjacency=adj)
        assert tuple(got.shape) == (3, len(V))
        for m in range(3):
            mine = tuple(int(s) for s in sources[inst == m])
            same_bytes(got[m], want('icosphere', mine, math.inf if cap is None else cap))
            alone = P.geodesic_distance(dev(V), list(mine), max_distance=cap, adjacency=adj)
            assert alone.dim() == 1 and torch.equal(alone, got[m])
    again = P.geodesic_distance(dev(V), sources, max_distance=0.9, source_instance=inst, num_instances=3, adjacency=adj)
    assert torch.equal(again, got)                                       # two runs, equal bytes
    faces = P.geodesic_distance(dev(V), list(sources[inst == 0]), faces=dev(QO.icosphere(3)[1]), max_distance=0.9)
    assert torch.equal(faces, got[0])                                    # the sides of the faces are the same edges


@pytest.mark.parametrize('levels', (1, None))
def test_star_above_the_lds_frontier_capacity(levels):
    V, ei, _ = graph('star')
    for sources, cap in (((0,), None), ((0,), 3.0), ((4321,), None), ((4321, 1), None)):
        got = check('star', sources, cap=cap, levels=levels)
    assert torch.isfinite(got).all()
    hub = want('star', (0,))
    assert len(np.unique(hub[2:5002])) == 5000                          # distinct lengths: 5000 different values


def test_checkerboard_lists_more_than_256_slices_of_256():
    """Unit grid 400 x 400 without diagonals (Manhattan distances, exact): instance 0 starts from the 80 000 vertices of one colour,
    so round 0 and round 1 each hold more than 65 536 entries; instance 1 is one source cut off at 30."""
    V, ei = GO.unit_grid_edges(400, 400)
    even = np.flatnonzero((V[:, 0] + V[:, 1]) % 2 == 0)
    s = 200 * 400 + 200
    sources = np.concatenate([even, [s]])
    inst = np.concatenate([np.zeros(len(even), dtype=np.int64), [1]])
    got = P.geodesic_distance(dev(V), sources, edge_index=dev(ei), max_distance=30.0, source_instance=inst, num_instances=2)
    manhattan = np.abs(V[:, 0] - V[s, 0]) + np.abs(V[:, 1] - V[s, 1])
    same_bytes(got, np.stack([(V[:, 0] + V[:, 1]) % 2, np.where(manhattan < 30.0, manhattan, math.inf)]))


def test_degenerate_input():
    got = check('degenerate', (0, 0, 7))                                # a repeated source
    assert got[1].item() == got[2].item() == 1.0 and math.isinf(got[4].item()) and math.isinf(got[5].item())
    check('degenerate', (0, 0, 7), cap=1.5)
    check('degenerate', (2,))                                           # the coincident twin of vertex 1
    check('degenerate', (5, 5, 6, 5))
    V, ei, _ = graph('degenerate')
    none = P.geodesic_distance(dev(V), [], edge_index=dev(ei))
    assert none.shape == (8,) and torch.isinf(none).all()
    empty = P.geodesic_distance(dev(V), torch.empty(0, dtype=torch.int64), edge_index=dev(ei), source_instance=[], num_instances=2)
    assert empty.shape == (2, 8) and torch.isinf(empty).all()
    one = P.geodesic_distance(dev(np.array([[1.0, 2.0, 3.0]])), [0], edge_index=torch.zeros(2, 0, dtype=torch.int64, device=DEV))
    assert one.tolist() == [0.0]
    loop = P.geodesic_distance(dev(np.array([[1.0, 2.0, 3.0]])), [0, 0], edge_index=torch.zeros(2, 3, dtype=torch.int64, device=DEV))
    assert loop.tolist() == [0.0]


def test_float32_vertices_with_int32_faces():
    V, F = QO.icosphere(2)
    V32 = (V * np.array([1.0, 0.3, 2.0])).astype(np.float32)
    got = P.geodesic_distance(dev(V32), [5, 77], faces=dev(F.astype(np.int32)), max_distance=1.25)
    same_bytes(got, GO.dijkstra(GO.weighted_adjacency(V32, SO.mesh_edges(F)), [5, 77], 1.25))


def test_vertex_at_exactly_the_cap_is_outside():
    V = np.array([[0.0, 0, 0], [3.0, 0, 0], [3.0, 4.0, 0]])
    ei = np.array([[0, 0], [1, 2]])                                      # 0 - 2 has length exactly 5
    assert P.geodesic_distance(dev(V), [0], edge_index=dev(ei), max_distance=5.0).tolist() == [0.0, 3.0, math.inf]
    assert P.geodesic_distance(dev(V), [0], edge_index=dev(ei), max_distance=float(np.nextafter(5.0, 6.0))).tolist() == [0.0, 3.0, 5.0]
    mask = P.circle_mask_from_centres_geodesic(dev(V), [0], 5.0, edge_index=dev(ei))
    assert mask.dtype == torch.int64 and mask.tolist() == [16, 7, 0]


def test_union_of_sources_is_the_elementwise_minimum():
    s1, s2 = (41, 900), (1311, 5, 1599)
    for cap in (None, 9.0):
        a, b, u = check('grid', s1, cap=cap), check('grid', s2, cap=cap), check('grid', s1 + s2, cap=cap)
        assert torch.minimum(a, b).cpu().numpy().tobytes() == u.cpu().numpy().tobytes()


# ---------------------------------------------------------------------------------------------------------------------- masks
@pytest.mark.parametrize('rings', (1, 16, 7))
def test_masks_from_centres_on_the_jittered_grid(rings):
    V, ei, adj = graph('grid')
    centres = [41, 1311, 820]
    got = P.circle_mask_from_centres_geodesic(dev(V), centres, 6.5, rings=rings, edge_index=dev(ei))
    exp = GO.mask_values(want('grid', tuple(centres), 6.5), 6.5, rings)
    assert got.dtype == torch.int64 and got.is_cuda and np.array_equal(got.cpu().numpy(), exp)
    assert exp.max() == rings and exp.min() == 0 and np.array_equal(exp, GO.circle_mask_from_centres(V, ei, centres, 6.5, rings, adj=adj))
    assert got[41].item() == rings
    ready = P.geodesic_adjacency(dev(V), edge_index=dev(ei))
    assert torch.equal(got, P.circle_mask_from_centres_geodesic(dev(V), centres, 6.5, rings=rings, adjacency=ready))


RADIUS, FRAC, SEED = 0.3, 0.25, 6


@functools.lru_cache(maxsize=None)
def oracle_masks(spacing, cand):
    V, F = QO.icosphere(3)
    return GO.circle_masks_geodesic(V, F, RADIUS, FRAC, 2, SEED, spacing, cand)


@pytest.mark.parametrize('spacing,cand', ((None, 2048), (1.2, 2048)))
def test_circle_masks_end_to_end(spacing, cand):
    V, F = QO.icosphere(3)
    n = len(V)
    w2 = oracle_masks(spacing, cand)
    ei = P.edges_from_faces(dev(F), n)
    before = P.circle_masks_on_surface(dev(V), dev(F), radius=2, num_masks=2, seed=SEED, spacing=spacing, candidates=cand)
    masks, info = P.circle_masks_geodesic(dev(V), dev(F), RADIUS, frac_masked_vertices=FRAC, num_masks=2, seed=SEED, spacing=spacing,
                                          candidates=cand, return_centres=True)
    after = P.circle_masks_on_surface(dev(V), dev(F), radius=2, num_masks=2, seed=SEED, spacing=spacing, candidates=cand)
    assert torch.equal(before, after)                                    # the hop masks keep their bytes
    assert masks.dtype == torch.int64 and masks.shape == (2, n) and masks.is_cuda and info['candidates'] == cand
    for m in range(2):
        w = w2[m]
        nb = int(info['batches'][m, 0])
        assert nb == len(w['sizes'])
        assert info['sizes'][m, 0, :nb].tolist() == w['sizes'] and info['counts'][m, 0, :nb].tolist() == w['counts']
        assert not info['sizes'][m, 0, nb:].any() and not info['counts'][m, 0, nb:].any()
        assert bool(info['exhausted'][m, 0]) == w['exhausted'] == (spacing is not None) and not bool(info['capped'][m, 0])
        assert bool(info['capped'][m, 0]) == w['capped']
        assert len(info['centres'][m][0]) == nb
        for got, exp in zip(info['centres'][m][0], w['batches']):
            assert np.array_equal(got.cpu().numpy(), exp)
        mk = masks[m].cpu().numpy()
        assert np.array_equal(mk, w['mask']) and mk.max() == 16
        assert int(info['masked'][m, 0]) == w['counts'][-1] == np.count_nonzero(mk)
    assert not torch.equal(masks[0], masks[1])
    assert torch.equal(masks, P.circle_masks_geodesic(dev(V), dev(F), RADIUS, frac_masked_vertices=FRAC, num_masks=2, seed=SEED,
                                                      spacing=spacing, candidates=cand, edge_index=ei))


def test_iteration_cap():
    V, F = QO.icosphere(3)
    capped, ic = P.circle_masks_geodesic(dev(V), dev(F), RADIUS, candidates=2048, seed=1, max_iters=1, return_centres=True)
    assert bool(ic['capped'][0, 0]) and int(ic['batches'][0, 0]) == 1 and ic['sizes'][0, 0].tolist() == [10]
    w = GO.circle_masks_geodesic(V, F, RADIUS, 0.25, 1, 1, None, 2048, max_iters=1)[0]
    assert w['capped'] and np.array_equal(capped[0].cpu().numpy(), w['mask'])


# --------------------------------------------------------------------------------------------------------------------- errors
def test_errors():
    V, ei, _ = graph('grid')
    for bad in ([1600], [-1], [3, 1600, 5]):
        with pytest.raises(IndexError):
            P.geodesic_distance(dev(V), bad, edge_index=dev(ei))
    with pytest.raises(IndexError):
        P.geodesic_distance(dev(V), [3], edge_index=dev(ei), source_instance=[2], num_instances=2)
    with pytest.raises(IndexError):
        P.geodesic_adjacency(dev(V), edge_index=dev(np.array([[0, 5], [1, 1600]])))
    _, status = P.geodesic_distance(dev(V), [3, 1600], edge_index=dev(ei), max_rounds=2)
    assert status.tolist()[0] & 2                                        # without a host check the status word says so
    Vn = V.copy()
    Vn[ei[0, 7], 2] = np.nan
    with pytest.raises(ValueError):
        P.geodesic_distance(dev(Vn), [0], edge_index=dev(ei))
    with pytest.raises(ValueError):
        P.geodesic_adjacency(dev(Vn), edge_index=dev(ei))
    Vn[ei[0, 7], 2] = np.inf
    with pytest.raises(ValueError):
        P.circle_mask_from_centres_geodesic(dev(Vn), [0], 2.0, edge_index=dev(ei))
    assert len(P.geodesic_adjacency(dev(Vn), edge_index=dev(ei), check=False)) == 3
    for radius, rings in ((0.0, 16), (-2.0, 16), (float('nan'), 16), (2.0, 0), (2.0, -3)):
        with pytest.raises(ValueError):
            P.circle_mask_from_centres_geodesic(dev(V), [0], radius, rings=rings, edge_index=dev(ei))
    with pytest.raises(ValueError):
        P.geodesic_distance(dev(V), [0], edge_index=dev(ei), max_distance=0.0)
    with pytest.raises(ValueError):
        P.geodesic_distance(dev(V), [0])                                 # no edges given
    with pytest.raises(TypeError):
        P.geodesic_distance(torch.from_numpy(V), [0], edge_index=torch.from_numpy(ei))
