"""k nearest neighbours on the GPU (csrc/stin_knn.hip through preprocessing.knn / fill_unseen_colors / FrameColors.result(knn=) /
knn_inpaint): equal to the numpy restatement of the contract (tests/_knn_oracle.py) bit for bit - indices equal, squared distances
equal as bit patterns, filled colours torch.equal.

Sizes cross the kernel's edges, not the workload's: a query block is 1024 queries at capacities 1, 2 and 4 and 512 at capacities 8
and 16, so Q = 1025 gives every capacity a partial last block; a tile is 512 points, so P = 2 tiles + 37 with 1, 2 and 3 chunks leaves
a 37-point last chunk and P = 2 tiles + 5 one that holds fewer than k candidates for k = 8 and 16.  One oracle run per point set at
k = 16 serves every smaller k (the answer for k is its first k columns)."""
import functools

import numpy as np
import pytest
import torch

import _frames_oracle as FO
import _knn_oracle as KO
from surface_texture_inpainting_net_amd import metrics, preprocessing as P

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

TILE, Q = 512, 1025
KS = (1, 2, 3, 4, 5, 8, 16)
CHUNKS = (1, 2, 3, None)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(got, want, k=None):
    """got: (index, d2) tensors; want: the oracle's pair at k = 16 or at k itself."""
    idx, d2 = got
    k = idx.shape[1] if k is None else k
    assert idx.dtype == torch.int64 and d2.dtype == torch.float64 and idx.is_cuda and idx.shape == d2.shape == (len(want[0]), k)
    assert np.array_equal(idx.cpu().numpy(), want[0][:, :k])
    assert d2.cpu().numpy().tobytes() == np.ascontiguousarray(want[1][:, :k]).tobytes()


# ------------------------------------------------------------------------------------------------------------ 1: random points
@functools.lru_cache(maxsize=None)
def random_set(extra):
    rng = np.random.default_rng(100 + extra)
    qs, pts = rng.uniform(-1, 1, (Q, 3)), rng.uniform(-1, 1, (2 * TILE + extra, 3))
    return qs, pts, KO.knn(qs, pts, 16)


@pytest.mark.parametrize('k', KS)
def test_random_points_every_k_and_chunk_count(k):
    qs, pts, want = random_set(37)
    for chunks in CHUNKS:
        same(P.knn(dev(qs), dev(pts), k, return_sq_dist=True, chunks=chunks), want, k)
    only = P.knn(dev(qs), dev(pts), k)
    assert torch.is_tensor(only) and np.array_equal(only.cpu().numpy(), want[0][:, :k])


@pytest.mark.parametrize('k', (8, 16))
def test_a_last_chunk_with_fewer_than_k_candidates(k):
    qs, pts, want = random_set(5)
    for chunks in (3, None, 1):
        same(P.knn(dev(qs), dev(pts), k, return_sq_dist=True, chunks=chunks), want, k)


def test_k_1_is_nearest():
    qs, pts, want = random_set(37)
    for chunks in (1, 3):
        idx, d2 = P.knn(dev(qs), dev(pts), 1, return_sq_dist=True, chunks=chunks)
        ni, nd = P.nearest(dev(qs), dev(pts), return_sq_dist=True, chunks=chunks)
        assert torch.equal(idx[:, 0], ni) and d2[:, 0].cpu().numpy().tobytes() == nd.cpu().numpy().tobytes()


def test_float32_input_is_promoted():
    qs, pts, _ = random_set(37)
    q32, p32 = dev(qs.astype(np.float32)), dev(pts.astype(np.float32))
    a, b = P.knn(q32, p32, 5, return_sq_dist=True), P.knn(q32.double(), p32.double(), 5, return_sq_dist=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    same(a, KO.knn(qs.astype(np.float32), pts.astype(np.float32), 5))


# ------------------------------------------------------------------------------------------------------------------ 2: ties
@functools.lru_cache(maxsize=None)
def lattice_set():
    """Points and queries on the lattice {0 .. 3}^3 (queries also at half steps): every d is exact and heavily tied.  Lattice point
    l sits at every index p with 37 p = l (mod 64): 16 or 17 copies, 64 indices apart, so its copies lie in every tile and chunk
    and on both sides of every tile edge.  Even queries coincide with points (d = 0)."""
    g = np.stack(np.meshgrid(np.arange(4.0), np.arange(4.0), np.arange(4.0), indexing='ij'), axis=3).reshape(64, 3)
    pts = g[(np.arange(2 * TILE + 37) * 37) % 64]
    qs = g[(np.arange(Q) * 29) % 64] + 0.5 * (np.arange(Q) % 2)[:, None] * g[(np.arange(Q) // 2) % 64]
    valid = np.random.default_rng(7).uniform(size=len(pts)) < 0.5
    return qs, pts, valid, KO.knn(qs, pts, 16), KO.knn(qs, pts, 16, point_valid=valid)


@pytest.mark.parametrize('k', KS)
def test_lattice_ties(k):
    qs, pts, valid, want, want_valid = lattice_set()
    assert (want[1][::2, 0] == 0).all() and (want[1][:, 0] == want[1][:, 1]).all()         # coincident queries; every answer tied
    for chunks in CHUNKS:
        same(P.knn(dev(qs), dev(pts), k, return_sq_dist=True, chunks=chunks), want, k)
        same(P.knn(dev(qs), dev(pts), k, point_valid=dev(valid), return_sq_dist=True, chunks=chunks), want_valid, k)


# ------------------------------------------------------------------------------------------------------------- 3: validity
def test_few_or_no_valid_points_pad_with_minus_one_and_inf():
    qs, pts, _, _, _ = lattice_set()
    two = np.zeros(len(pts), dtype=np.uint8)
    two[[700, 3]] = 1
    want = KO.knn(qs, pts, 3, point_valid=two)
    assert (want[0][:, 2] == -1).all() and (want[0][:, :2] >= 0).all()
    for chunks in CHUNKS:
        same(P.knn(dev(qs), dev(pts), 3, point_valid=dev(two), return_sq_dist=True, chunks=chunks), want)
        idx, d2 = P.knn(dev(qs), dev(pts), 3, point_valid=dev(np.zeros(len(pts), dtype=bool)), return_sq_dist=True, chunks=chunks)
        assert (idx == -1).all() and torch.isinf(d2).all() and (d2 > 0).all()
    idx, d2 = P.knn(dev(qs), dev(np.zeros((0, 3))), 2, return_sq_dist=True)                 # no points at all: not an error
    assert idx.shape == (Q, 2) and (idx == -1).all() and torch.isinf(d2).all()
    assert P.knn(dev(np.zeros((0, 3))), dev(pts), 2).shape == (0, 2)


def test_non_finite_coordinates():
    qs, pts, valid, _, want_valid = lattice_set()
    bad = pts.copy()
    bad[np.flatnonzero(~valid)[[0, 5, -1]]] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]]
    for chunks in (1, 3):                                                # an invalid point is never looked at
        same(P.knn(dev(qs), dev(bad), 4, point_valid=dev(valid), return_sq_dist=True, chunks=chunks), want_valid, 4)
    for p in (np.flatnonzero(valid)[0], np.flatnonzero(valid)[-1]):     # a valid one raises, in the first and in the last chunk
        bad = pts.copy()
        bad[p, 1] = np.inf
        with pytest.raises(ValueError, match='not finite'):
            P.knn(dev(qs), dev(bad), 4, point_valid=dev(valid), chunks=3)
    badq = qs.copy()
    badq[Q - 1, 2] = np.nan
    with pytest.raises(ValueError, match='not finite'):
        P.knn(dev(badq), dev(pts), 2)


# --------------------------------------------------------------------------------------------------------- 4: query subset
def test_query_subset_scrambled_with_gaps():
    qs, pts, want = random_set(37)
    rows = np.random.default_rng(3).permutation(Q)[:600]                 # scrambled, with gaps
    ref_i, ref_d = np.full((Q, 5), -1, dtype=np.int64), np.full((Q, 5), np.inf)
    ref_i[rows], ref_d[rows] = want[0][rows, :5], want[1][rows, :5]
    for chunks in CHUNKS:
        same(P.knn(dev(qs), dev(pts), 5, query_index=dev(rows), return_sq_dist=True, chunks=chunks), (ref_i, ref_d))
    idx = P.knn(dev(qs), dev(pts), 2, query_index=dev(np.zeros(0, dtype=np.int64)))
    assert idx.shape == (Q, 2) and (idx == -1).all()
    for wrong in (Q, -1):
        with pytest.raises(ValueError, match='outside'):
            P.knn(dev(qs), dev(pts), 2, query_index=dev(np.array([4, wrong, 7])))


# ------------------------------------------------------------------------------------------------------------------ 5: fill
@functools.lru_cache(maxsize=None)
def fill_set():
    rng = np.random.default_rng(21)
    V = rng.uniform(-1, 1, (2 * TILE + 37, 3))
    count = rng.integers(1, 4, len(V)).astype(np.int32) * (rng.uniform(size=len(V)) > 0.3)
    return V, count.astype(np.int32), rng.uniform(-1, 1, (len(V), 16)).astype(np.float32)


@pytest.mark.parametrize('C', (1, 3, 16))
def test_fill_unseen_colors_against_the_oracle(C):
    V, count, colors = fill_set()
    colors = colors[:, :C]
    unseen = count == 0
    assert 0.25 < unseen.mean() < 0.35
    want, want_filled = KO.fill_unseen(V, colors, count, k=3)
    got, filled = P.fill_unseen_colors(dev(V), dev(colors), dev(count), return_filled=True)
    assert got.dtype == torch.float32 and filled.dtype == torch.bool
    assert torch.equal(got.cpu(), torch.from_numpy(want)) and np.array_equal(filled.cpu().numpy(), want_filled)
    assert np.array_equal(want_filled, unseen)
    assert torch.equal(got.cpu()[~unseen], torch.from_numpy(colors)[~unseen])               # seen rows are never modified
    assert torch.equal(P.fill_unseen_colors(dev(V), dev(colors), dev(count)), got)
    # a view with a row pitch (the colour columns of a wider array) and int64 counts
    wide = dev(np.concatenate([colors, colors], axis=1))[:, :C]
    assert torch.equal(P.fill_unseen_colors(dev(V), wide, dev(count.astype(np.int64))), got)


def test_fill_min_count_all_seen_and_none_seen():
    V, count, colors = fill_set()
    colors = colors[:, :3]
    want2, filled2 = KO.fill_unseen(V, colors, count, k=3, min_count=2)
    got2, f2 = P.fill_unseen_colors(dev(V), dev(colors), dev(count), min_count=2, return_filled=True)
    assert torch.equal(got2.cpu(), torch.from_numpy(want2)) and np.array_equal(f2.cpu().numpy(), filled2)
    assert filled2.sum() > (count == 0).sum() and not np.array_equal(want2, KO.fill_unseen(V, colors, count, k=3)[0])
    for k in (1, 8):
        assert torch.equal(P.fill_unseen_colors(dev(V), dev(colors), dev(count), k=k).cpu(),
                           torch.from_numpy(KO.fill_unseen(V, colors, count, k=k)[0]))
    src = dev(colors)
    got, filled = P.fill_unseen_colors(dev(V), src, dev(np.ones_like(count)), return_filled=True)             # all seen
    assert torch.equal(got, src) and got.data_ptr() != src.data_ptr() and not filled.any()
    got, filled = P.fill_unseen_colors(dev(V), src, dev(np.zeros_like(count)), return_filled=True)            # none seen
    assert torch.equal(got, src) and got.data_ptr() != src.data_ptr() and not filled.any()
    assert torch.equal(src.cpu(), torch.from_numpy(colors))                                                   # the input is left alone


# ---------------------------------------------------------------------------------------------------------- 6: FrameColors
SPHERE_D = (120.0, 120.0, 128 / 2 - 0.5, 96 / 2 - 0.5)                   # depth frames 96 x 128
SPHERE_C = (60.0, 58.2, 64 / 2 - 0.5, 48 / 2 - 0.5)                      # colour frames 48 x 64
SPHERE_KW = dict(margin=2, discontinuity_threshold=0.5, half_kernel=3)


def look_at(eye, target=(0.0, 0.0, 0.0)):
    """Camera-to-world [4, 4]: +z forward, +x right, +y down the rows."""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    M = np.eye(4)
    M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = right, np.cross(fwd, right), fwd, eye
    return M


@functools.lru_cache(maxsize=None)
def sphere():
    """162 points spread over the unit sphere, 12 poses on a circle above its equator (the underside is never seen), analytic depth."""
    i = np.arange(162) + 0.5
    z, phi = 1.0 - 2.0 * i / 162, i * np.pi * (3.0 - np.sqrt(5.0))
    V = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], axis=1)
    poses = np.stack([look_at([3.0 * np.cos(a), 3.0 * np.sin(a), 0.8]) for a in 0.1 + 2 * np.pi * np.arange(12) / 12])
    depth = FO.render_sphere(poses, 96, 128, SPHERE_D)
    color = np.random.default_rng(1).integers(0, 256, (12, 48, 64, 3), dtype=np.uint8)
    return V, poses, depth, color


def test_frame_colors_with_the_fill():
    V, poses, depth, color = sphere()
    base, count_o, _, _ = FO.colors(V, poses, color, SPHERE_C, depth=depth, depth_camera=SPHERE_D, **SPHERE_KW)
    assert 20 <= (count_o == 0).sum() <= 120 and (count_o > 0).sum() >= 40
    fc = P.FrameColors(dev(V), SPHERE_C, SPHERE_D, **SPHERE_KW)
    fc.add(poses, dev(color), depth=dev(depth))
    plain, count = fc.result()
    zero, count0 = fc.result(knn=0)
    assert torch.equal(zero, plain) and torch.equal(count0, count) and np.array_equal(count.cpu().numpy(), count_o)
    assert plain.cpu().numpy().tobytes() == base.tobytes()
    filled, count3 = fc.result(knn=3)
    assert torch.equal(count3, count)
    assert torch.equal(filled, P.fill_unseen_colors(dev(V), plain, count, k=3))
    want, _ = KO.fill_unseen(V, base, count_o, k=3)
    assert torch.equal(filled.cpu(), torch.from_numpy(want)) and not torch.equal(filled, plain)
    assert torch.equal(fc.result(fill=(0.5, 0.25, 1.0), knn=3)[0], filled)                  # `fill` is overwritten wherever someone is seen
    c2, n2 = P.vertex_colors_from_frames(dev(V), poses, dev(color), depth=dev(depth), color_camera=SPHERE_C, depth_camera=SPHERE_D,
                                         batch=5, knn=3, **SPHERE_KW)
    assert torch.equal(c2, filled) and torch.equal(n2, count)
    c0, _ = P.vertex_colors_from_frames(dev(V), poses, dev(color), depth=dev(depth), color_camera=SPHERE_C, depth_camera=SPHERE_D,
                                        **SPHERE_KW)
    assert torch.equal(c0, plain)
    with pytest.raises(ValueError):
        fc.result(knn=17)


# ------------------------------------------------------------------------------------------------------------- 7: baseline
class Sample:
    pass


def test_knn_inpaint_beats_the_constant_fill_and_feeds_step_metrics():
    pos, color, edge_index = KO.baseline_scene()
    mask = P.circle_mask_from_centres(dev(edge_index), KO.SIDE ** 2, KO.HOLE_RADIUS, [KO.HOLE_CENTRE])
    assert np.array_equal(mask.cpu().numpy(), KO.hole_mask())
    s = Sample()
    s.pos, s.color, s.mask, s.edge_index = dev(pos), dev(color), mask.reshape(-1, 1), dev(edge_index)
    got = P.knn_inpaint(s)
    hole = mask > 0
    want, _ = KO.fill_unseen(pos, color, (~hole).cpu().numpy().astype(np.int32), k=3)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert torch.equal(got[~hole], s.color[~hole])                       # exactly 0 outside the hole
    err_knn = float((got[hole].double() - s.color[hole].double()).abs().mean())
    err_const = float(s.color[hole].double().abs().mean())               # the constant fill: 0, the middle of [-1, 1]
    print('mean |error| over the hole: knn %.4f, constant fill %.4f' % (err_knn, err_const))
    assert err_knn < err_const
    assert torch.equal(P.knn_inpaint((s.pos, s.color, s.mask), k=3), got)
    del s.pos                                                            # a training sample: positions in x[:, 6:9]
    s.x = torch.cat([torch.zeros(len(pos), 6, device=DEV), dev(pos).float() / 1.5, torch.ones(len(pos), 1, device=DEV)], dim=1)
    assert torch.equal(P.knn_inpaint(s)[~hole], s.color[~hole])
    m = metrics.StepMetrics(DEV, capacity=2)
    row = m.update(got, s, composite=False).cpu()
    row_const = m.update(torch.zeros_like(got), s, composite=True).cpu()
    keys = metrics.StepMetrics.KEYS
    assert float(row[keys.index('l1')]) < float(row_const[keys.index('l1')])
    assert float(row[keys.index('psnr')]) > float(row_const[keys.index('psnr')])
