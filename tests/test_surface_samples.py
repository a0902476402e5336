"""The numpy restatement of the surface samples (tests/_surface_oracle.py; include/stin_hip.h, "Surface samples") against first
principles, on the CPU: the drawn face against Python integers, exact weight ratios, barycentric coordinates and points inside
their triangles, and the defining properties of the sequential-greedy Poisson-disk set.  The device is held to this oracle bit
for bit in test_surface_samples_gpu.py."""
import functools

import numpy as np
import pytest

import _qem_oracle as QO
import _surface_oracle as SO
from surface_texture_inpainting_net_amd import _lib, preprocessing as P

EPS = 2.0 ** -52
ENTRY_POINTS = ('stin_surface_weights_workspace_bytes', 'stin_surface_weights_f64', 'stin_surface_sample_f64',
                'stin_poisson_grid_workspace_bytes', 'stin_poisson_grid_f64', 'stin_poisson_rounds_f64', 'stin_first_occurrence_i64')


@pytest.fixture(autouse=True)
def the_package_has_the_feature():
    """The oracle restates a contract of the package: its header declares the entry points and its module has the wrappers."""
    assert all(name in _lib.SIGNATURES for name in ENTRY_POINTS)
    assert all(callable(getattr(P, name)) for name in ('sample_surface', 'poisson_disk', 'surface_centres', 'circle_masks_on_surface'))


@functools.lru_cache(maxsize=None)
def sphere(sub):
    return QO.icosphere(sub)


@functools.lru_cache(maxsize=None)
def drawn(sub, n, seed):
    V, F = sphere(sub)
    return SO.sample_surface(V, F, n, seed)


def test_hash_and_stream_seed_agree_with_the_package_and_python_integers():
    z = np.array([0, 1, 2 ** 63, 2 ** 64 - 1, 0x123456789ABCDEF], dtype=np.uint64)
    assert [int(x) for x in SO.mix64(z)] == [SO.mix64_int(int(x)) for x in z] == [P._mix64(int(x)) for x in z]
    assert SO.mix64_int(0) == 0 and SO.mix64_int(1) == 0x5692161D100B05E5          # splitmix64's finaliser
    seeds = [SO.stream_seed(7, m) for m in range(4)]
    assert seeds == [P.surface_stream_seed(7, m) for m in range(4)] and len(set(seeds)) == 4
    a, b = np.array([2 ** 64 - 1, 3, 2 ** 63 + 12345], dtype=np.uint64), np.array([2 ** 64 - 1, 2 ** 63, 987654321987], dtype=np.uint64)
    assert [int(x) for x in SO.mulhi64(a, b)] == [(int(x) * int(y)) >> 64 for x, y in zip(a, b)]
    assert P.default_surface_candidates(12.5, 642, 0.3) == P.default_surface_candidates(12.5, 642, 0.3) == 1024
    assert P.default_surface_candidates(100.0, 642, 0.1) == 40000 and P.default_surface_candidates(1.0, 5000) == 5000


def test_drawn_face_is_the_first_with_cum_above_u_in_python_integers():
    V, F = sphere(1)
    n, seed, first = 500, 5, 1000
    W, _ = SO.face_weights(V, F)
    assert W.max() < 2 ** 40 and W.max() >= 2 ** 39 and W.min() > 0
    cum, s = [], 0
    for w in W:
        s += int(w)
        cum.append(s)
    _, face, _ = SO.sample_surface(V, F, n, seed, first)
    base = SO.mix64_int(seed + SO.G)
    for i in range(n):
        r0 = SO.mix64_int(base + (3 * (first + i)) * SO.G)
        u = (r0 * cum[-1]) >> 64
        assert face[i] == next(f for f in range(len(cum)) if cum[f] > u)
    assert len(set(face.tolist())) > 40                                 # the draw spreads over the 80 faces


def test_first_is_the_tail_of_a_longer_draw():
    V, F = sphere(1)
    p, f, b = SO.sample_surface(V, F, 300, 3)
    q, g, c = SO.sample_surface(V, F, 100, 3, first=200)
    assert q.tobytes() == p[200:].tobytes() and np.array_equal(g, f[200:]) and c.tobytes() == b[200:].tobytes()


def test_weights_of_areas_1_and_3_are_in_the_exact_ratio():
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [3, 0, 0]], dtype=np.float64)
    F = np.array([[0, 1, 2], [0, 3, 2]])
    W, A2 = SO.face_weights(V, F)
    assert A2.tolist() == [2.0, 6.0] and W[1] == 3 * W[0] and W[1] == 6 * 2 ** 37
    _, face, _ = SO.sample_surface(V, F, 4000, 1)
    assert abs(np.mean(face == 1) - 0.75) < 0.03
    W, _ = SO.face_weights(V, np.array([[0, 1, 2], [0, 3, 2], [1, 1, 2], [0, 1, 3]]))      # a repeated vertex, a zero area
    assert W[2] == 0 and W[3] == 0
    _, face, _ = SO.sample_surface(V, np.array([[1, 1, 2], [0, 1, 2], [0, 1, 3]]), 500, 2)
    assert np.all(face == 1)                                            # zero-weight faces are never drawn
    with pytest.raises(ValueError):
        SO.face_weights(V, np.array([[1, 1, 2], [0, 1, 3]]))
    with pytest.raises(IndexError):
        SO.face_weights(V, np.array([[0, 1, 4]]))
    Vn = V.copy()
    Vn[3, 1] = np.nan
    with pytest.raises(ValueError):
        SO.face_weights(Vn, F)


def test_barycentric_coordinates_lie_in_the_unit_interval_and_sum_to_one():
    _, _, b = drawn(3, 4096, 0)
    assert b.min() >= 0.0 and b.max() <= 1.0
    assert np.abs(b.sum(axis=1) - 1.0).max() <= 2 * EPS
    assert np.abs((b[:, 0] + b[:, 1]) + b[:, 2] - 1.0).max() <= 2 * EPS


def test_points_lie_in_their_triangles_plane_and_inside_it():
    V, F = sphere(3)
    p, f, b = drawn(3, 4096, 0)
    a, bb, c = (V[F[f, k]].astype(np.longdouble) for k in range(3))
    bl = b.astype(np.longdouble)
    exact = bl[:, :1] * a + bl[:, 1:2] * bb + bl[:, 2:] * c
    scale = np.abs(V).max()
    assert np.abs(p - exact).max() <= 4 * EPS * scale                   # p is the convex combination its coordinates say
    nrm = np.cross(V[F[f, 1]] - V[F[f, 0]], V[F[f, 2]] - V[F[f, 0]])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    assert np.abs(np.einsum('ij,ij->i', nrm, p - V[F[f, 0]])).max() <= 16 * EPS * scale
    # inside: the coordinates solved back from the point are those of the draw, hence >= 0
    e1, e2, d = V[F[f, 1]] - V[F[f, 0]], V[F[f, 2]] - V[F[f, 0]], p - V[F[f, 0]]
    g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    r1, r2 = (d * e1).sum(1), (d * e2).sum(1)
    det = g11 * g22 - g12 * g12
    s1, s2 = (g22 * r1 - g12 * r2) / det, (g11 * r2 - g12 * r1) / det
    assert np.abs(s1 - b[:, 1]).max() < 1e-9 and np.abs(s2 - b[:, 2]).max() < 1e-9
    assert s1.min() > -1e-9 and s2.min() > -1e-9 and (s1 + s2).max() < 1 + 1e-9


@functools.lru_cache(maxsize=None)
def cloud():
    pts = np.random.default_rng(7).uniform(-1, 1, (600, 3))
    r = 0.3
    return pts, r, SO.poisson_disk(pts, r)


def test_greedy_set_keeps_every_pair_apart():
    pts, r, kept = cloud()
    assert 20 < len(kept) < 400 and np.all(np.diff(kept) > 0) and kept[0] == 0
    for a in range(1, len(kept)):
        assert np.all(SO.d2_to(pts, kept[a], kept[:a]) >= r * r)


def test_every_rejected_candidate_has_an_earlier_accepted_one_within_reach():
    pts, r, kept = cloud()
    is_kept = np.zeros(len(pts), dtype=bool)
    is_kept[kept] = True
    for i in np.flatnonzero(~is_kept):
        assert np.any(SO.d2_to(pts, i, kept[kept < i]) < r * r)


def test_every_prefix_of_the_result_is_the_result_of_the_same_prefix_of_candidates():
    pts, r, kept = cloud()
    for c in (1, 2, 57, 300, 599):
        assert np.array_equal(SO.poisson_disk(pts[:c], r), kept[kept < c])


def test_lattice_at_the_radius_keeps_all_and_just_below_keeps_half():
    g = np.arange(6, dtype=np.float64)
    lattice = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
    assert len(SO.poisson_disk(lattice, 1.0)) == 216                    # d2 = r2 is not a conflict: the inequality is strict
    half = SO.poisson_disk(lattice, 1.0 + 2.0 ** -30)
    assert len(half) == 108 and np.all(lattice[half].sum(axis=1) % 2 == 0)


def test_chain_and_repeats():
    line = np.zeros((300, 3))
    line[:, 0] = np.arange(300) * 0.6
    assert np.array_equal(SO.poisson_disk(line, 1.0), np.arange(0, 300, 2))
    rep = np.repeat(np.random.default_rng(0).uniform(0, 10, (20, 3)), 3, axis=0)
    assert np.array_equal(SO.poisson_disk(rep, 1e-3), np.arange(0, 60, 3))
    assert np.array_equal(SO.first_occurrences(np.array([5, 3, 5, 5, 1, 3, 9])), [5, 3, 1, 9])


def test_circle_mask_loop_finishes_by_the_rule_or_ends_exhausted():
    V, F = sphere(3)
    done = SO.circle_masks_on_surface(V, F, 2, 0.25, 1, 0, None, 2048)[0]
    assert not done['exhausted'] and not done['capped'] and done['sizes'][0] == 10 and len(done['sizes']) > 1
    assert 0.15 < done['counts'][-1] / len(V) < 0.4
    short = SO.circle_masks_on_surface(V, F, 2, 0.25, 1, 0, 1.2, 2048)[0]
    assert short['exhausted'] and sum(short['sizes']) < 10
    cs = np.concatenate(short['batches'])
    d = V[cs][:, None, :] - V[cs][None, :, :]
    assert np.sqrt((d * d).sum(-1))[np.triu_indices(len(cs), 1)].min() > 0.8      # spread out (samples >= 1.2 apart, then snapped)
