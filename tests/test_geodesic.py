"""The restatement of the geodesic circle masks (tests/_geodesic_oracle.py; include/stin_hip.h, "Geodesic distances") against first
principles, on the CPU: its two independent forms - heap Dijkstra and Bellman-Ford sweeps - agree byte for byte on every case the
device is held to in test_geodesic_gpu.py, a unit grid gives Manhattan distances exactly, and the mask rule holds at its edges.
The distance is Dijkstra's metric on the edge graph, not the exact polyhedral geodesic."""
import functools
import math

import numpy as np
import pytest

import _geodesic_oracle as GO
import _qem_oracle as QO
import _surface_oracle as SO
from surface_texture_inpainting_net_amd import _abi, _lib, preprocessing as P

ENTRY_POINTS = ('stin_geodesic_lengths_f64', 'stin_geodesic_workspace_bytes', 'stin_geodesic_begin_f64', 'stin_geodesic_rounds_f64',
                'stin_geodesic_mask_f64')
WRAPPERS = ('geodesic_adjacency', 'geodesic_distance', 'circle_mask_from_centres_geodesic', 'circle_masks_geodesic')


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (vertices, edge_index, sources, caps): the graphs of the GPU tests."""
    out = {}
    V, ei = GO.kite()
    out['kite'] = (V, ei, [0], (math.inf, 2.5))
    V, ei = GO.ladder_with_shortcut(300)
    out['ladder'] = (V, ei, [0], (math.inf,))
    V, ei = GO.chain(1025)
    out['chain'] = (V, ei, [0], (math.inf,))
    for name, sy in (('grid', 1.0), ('grid-10:1', 0.1)):
        V, F = GO.grid_mesh(40, 40, 1.0, sy, jitter=0.3, seed=2)
        out[name] = (V, SO.mesh_edges(F), [41, 1311], (math.inf, 9.0 if sy == 1.0 else 4.0))
    V, F = QO.icosphere(3)
    out['icosphere'] = (V, SO.mesh_edges(F), [0, 17, 300, 641], (math.inf, 0.9))
    V, ei = GO.double_star()
    out['star-hub'] = (V, ei, [0], (math.inf, 3.0))
    out['star-leaf'] = (V, ei, [4321], (math.inf,))
    V, ei = GO.degenerate()
    out['degenerate'] = (V, ei, [0, 0, 2], (math.inf, 1.5))
    return out


@pytest.mark.parametrize('name', ('kite', 'ladder', 'chain', 'grid', 'grid-10:1', 'icosphere', 'star-hub', 'star-leaf', 'degenerate'))
def test_dijkstra_and_bellman_ford_agree_byte_for_byte(name):
    V, ei, sources, caps = cases()[name]
    adj = GO.weighted_adjacency(V, ei)
    for cap in caps:
        a, b = GO.dijkstra(adj, sources, cap), GO.bellman_ford(adj, sources, cap)
        assert a.dtype == np.float64 and a.tobytes() == b.tobytes()
        assert a[sources[0]] == 0.0 and np.all((a < cap) | np.isinf(a))
        if cap < math.inf:
            full = GO.dijkstra(adj, sources)
            assert a.tobytes() == np.where(full < cap, full, math.inf).tobytes()       # the cap only hides, it never changes


def test_lengths_are_symmetric_and_the_explicit_sum():
    V, F = GO.grid_mesh(7, 5, 1.0, 0.1, jitter=0.3, seed=1)
    ei = SO.mesh_edges(F)
    ln = GO.edge_lengths(V, ei)
    assert ln.tobytes() == GO.edge_lengths(V, ei[::-1]).tobytes()
    d = V[ei[0, 3]] - V[ei[1, 3]]
    assert ln[3] == math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    V32 = V.astype(np.float32)
    assert GO.edge_lengths(V32, ei).tobytes() == GO.edge_lengths(V32.astype(np.float64), ei).tobytes()
    with pytest.raises(IndexError):
        GO.edge_lengths(V, np.array([[0], [len(V)]]))
    Vn = V.copy()
    Vn[ei[0, 0], 1] = np.nan
    with pytest.raises(ValueError):
        GO.edge_lengths(Vn, ei)


def test_unit_grid_without_diagonals_gives_manhattan_distances_exactly():
    V, ei = GO.unit_grid_edges(23, 17)
    adj = GO.weighted_adjacency(V, ei)
    s = 5 * 17 + 3
    want = np.abs(V[:, 0] - V[s, 0]) + np.abs(V[:, 1] - V[s, 1])
    for form in (GO.dijkstra, GO.bellman_ford):
        assert form(adj, [s]).tobytes() == want.tobytes()
        capped = form(adj, [s], 6.0)
        assert capped.tobytes() == np.where(want < 6.0, want, math.inf).tobytes()      # a vertex at exactly the cap is +inf
    two = GO.dijkstra(adj, [s, 0])
    assert two.tobytes() == np.minimum(want, V[:, 0] + V[:, 1]).tobytes()


def test_kite_the_hop_metric_and_the_edge_metric_disagree():
    V, ei = GO.kite()
    D = GO.dijkstra(GO.weighted_adjacency(V, ei), [0])
    assert D.tolist() == [0.0, 1.0, 2.0, 3.0]
    import _mask_oracle as MO
    hops = 4 - MO.heap_bfs_mask(MO.adjacency(ei, 4), 4, [0])
    assert hops.tolist() == [0, 1, 2, 1]                                 # vertex 3 is one hop away and the farthest
    assert GO.dijkstra(GO.weighted_adjacency(V, ei), [0], 2.5).tolist() == [0.0, 1.0, 2.0, math.inf]


def test_ladder_lowers_vertices_again_after_their_first_value():
    """What the case is for: in hop-level order the far end gets a first value over the arc that the rails lower later."""
    V, ei = GO.ladder_with_shortcut(300)
    adj = GO.weighted_adjacency(V, ei)
    D = GO.dijkstra(adj, [0])
    first, frontier, lowered_again = {0: 0.0}, [0], 0
    cur = {0: 0.0}
    while frontier:                                                      # level-synchronous label correcting
        nxt = {}
        for u in frontier:
            for w, l in adj[u]:
                nd = cur[u] + l
                if nd < cur.get(w, math.inf) and nd < nxt.get(w, math.inf):
                    nxt[w] = nd
        for w, nd in nxt.items():
            lowered_again += w in first
            first.setdefault(w, nd)
            cur[w] = nd
        frontier = list(nxt)
    assert lowered_again > 50 and first[139] > D[139] * 1.3
    assert np.array([cur[v] for v in range(300)]).tobytes() == D.tobytes()


def test_mask_rule_at_its_edges():
    r = 1.0                                                              # ring = 2^-4 exactly: the expected values are exact
    below = np.nextafter(r, 0.0)
    D = np.array([0.0, below, r, np.nextafter(r, 2.0), math.inf, 0.0625, 0.06, 0.5])
    assert GO.mask_values(D, r, 16).tolist() == [16, 1, 0, 0, 0, 15, 16, 8]
    assert GO.mask_values(D, r, 1).tolist() == [1, 1, 0, 0, 0, 1, 1, 1]
    assert GO.mask_values(D, r, 7).tolist() == [7, 1, 0, 0, 0, 7, 7, 4]
    m = GO.mask_values(np.linspace(0.0, 1.0, 1001), 1.0, 16)
    assert m[0] == 16 and m[-1] == 0 and m[-2] == 1 and np.all(np.diff(m) <= 0) and set(m.tolist()) == set(range(17))
    for bad in (dict(radius=0.0, rings=16), dict(radius=-1.0, rings=16), dict(radius=math.inf, rings=16), dict(radius=1.0, rings=0)):
        with pytest.raises(ValueError):
            GO.mask_values(D, **bad)


def test_three_four_five_triangle_at_exactly_the_cap():
    V = np.array([[0.0, 0, 0], [3.0, 0, 0], [3.0, 4.0, 0]])
    ei = np.array([[0, 0], [1, 2]])                                      # 0 - 2 has length exactly 5
    adj = GO.weighted_adjacency(V, ei)
    assert GO.dijkstra(adj, [0], 5.0).tolist() == [0.0, 3.0, math.inf]
    assert GO.circle_mask_from_centres(V, ei, [0], 5.0, 16).tolist() == [16, 7, 0]
    assert GO.dijkstra(adj, [0], np.nextafter(5.0, 6.0)).tolist() == [0.0, 3.0, 5.0]


def test_circle_mask_loop_finishes_by_the_rule_or_ends_exhausted():
    V, F = QO.icosphere(3)
    done = GO.circle_masks_geodesic(V, F, 0.3, 0.25, 1, 0, None, 2048)[0]
    assert not done['exhausted'] and not done['capped'] and done['sizes'][0] == 10 and len(done['sizes']) > 1
    assert 0.15 < done['counts'][-1] / len(V) < 0.45 and done['mask'].max() == 16
    short = GO.circle_masks_geodesic(V, F, 0.3, 0.25, 1, 0, 1.2, 2048)[0]
    assert short['exhausted'] and sum(short['sizes']) < 10
    surface = SO.circle_masks_on_surface(V, F, 2, 0.25, 1, 0, None, 2048)[0]
    assert np.array_equal(surface['batches'][0], done['batches'][0])     # the same centre stream as circle_masks_on_surface


def test_header_declares_the_entry_points_and_the_package_exposes_them():
    """Fails without the feature: the prototypes of include/stin_hip.h, the signatures _lib derives from them, the wrappers."""
    import ctypes
    header = open(_abi.HEADER_PATH).read()
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES and (name + '(') in header
    assert all(callable(getattr(P, name, None)) for name in WRAPPERS)
    sig = _lib.SIGNATURES
    assert sig['stin_geodesic_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int])
    ptr, i64, i32, f64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
    assert sig['stin_geodesic_lengths_f64'] == (i32, [ptr, i64, ptr, ptr, i64, ptr, ptr, ptr])
    assert sig['stin_geodesic_begin_f64'] == (i32, [ptr, ptr, i64, i64, i32, ptr, ptr, ptr, ctypes.c_size_t, ptr])
    assert sig['stin_geodesic_rounds_f64'] == (i32, [ptr, ptr, ptr, i64, i64, i32, f64, ptr, i32, i32, i32, ptr, ptr, ctypes.c_size_t, ptr])
    assert sig['stin_geodesic_mask_f64'] == (i32, [ptr, i64, f64, i32, ptr, ptr])
    lib = _lib.load()                                                    # the built library has every one of them
    assert lib.stin_geodesic_workspace_bytes(1000, 3) >= 3 * 1000 * 12
    assert lib.stin_geodesic_workspace_bytes(1 << 30, 4) == 0            # M N beyond 2^31: refused
    import os
    assert 'stin_geodesic.hip' in open(os.path.join(os.path.dirname(P.__file__), 'csrc', 'Makefile')).read()


def test_wrappers_refuse_cpu_tensors_and_bad_arguments_before_any_launch():
    import torch
    V = torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(TypeError):
        P.geodesic_distance(V, [0], edge_index=torch.zeros(2, 0, dtype=torch.int64))
    with pytest.raises(TypeError):
        P.geodesic_adjacency(V, edge_index=torch.zeros(2, 0, dtype=torch.int64))
    for r, rings in ((0.0, 16), (-1.0, 16), (math.inf, 16), (1.0, 0)):
        with pytest.raises(ValueError):
            P.circle_mask_from_centres_geodesic(V, [0], r, rings=rings)
        with pytest.raises(ValueError):
            P.circle_masks_geodesic(V, torch.zeros(1, 3, dtype=torch.int64), r, rings=rings)
