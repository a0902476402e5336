"""The non-rigid colour-map optimisation on the host: the numpy restatement of the contract (tests/_nonrigid_oracle.py) is the rigid
one at a zero flow, its weights and anchor Jacobian are what the warp says, it removes a smooth warp of a frame that no rigid pose
can remove - and the host code of preprocessing.optimize_poses_nonrigid (the update, the argument checks) behaves as stated.
The kernels are compared against the same restatement in tests/test_nonrigid_gpu.py."""
import functools

import numpy as np
import pytest
import torch

import _colormap_oracle as CO
import _nonrigid_oracle as NO
from surface_texture_inpainting_net_amd import preprocessing as P
from test_colormap import CAM, FREED, H, MARGIN, W, scene

S = 16                                                                  # 48 x 64 frames: 4 x 5 anchors, 3 x 4 cells, 46 unknowns
AH, AW = 4, 5
ITERATIONS = 8
DENSE = 48                                                              # wall(48): 2 401 vertices, some 730 pairs per frame
ANCHOR_WEIGHT = 0.03


def fixed_poses():
    V, _, _, poses, color, _, bits = scene()
    RT, valid = P.pose_extrinsics(poses)
    return V, RT, valid, color, bits


def some_flow(seed=2, amplitude=1.5, n=6):
    return np.random.default_rng(seed).uniform(-amplitude, amplitude, (n, AH, AW, 2))


def test_the_lattice_is_the_contracts():
    assert NO.lattice(48, 64, 16) == (4, 5) == P.nonrigid_lattice(48, 64, 16)
    assert NO.lattice(33, 70, 16) == (3, 6) == P.nonrigid_lattice(33, 70, 16)            # ragged last cells
    assert NO.lattice(480, 640, 32) == (16, 21) == P.nonrigid_lattice(480, 640, 32)      # 678 unknowns, the paper's size
    assert NO.lattice(2, 2, 5) == (2, 2) == P.nonrigid_lattice(2, 2, 5)
    assert NO.unknowns(1, 2, 5) == [0, 1, 2, 3, 4, 5, 20, 21, 22, 23, 30, 31, 32, 33]
    assert len(NO.TRI) == 105 and NO.TRI[0] == (0, 0) and NO.TRI[14] == (1, 1) and NO.TRI[-1] == (13, 13)


# -------------------------------------------------------------------------------------------------- the rigid contract at zero flow
def test_zero_flow_accumulate_is_the_unwarped_one():
    V, RT, valid, color, bits = fixed_poses()
    zero = np.zeros((6, AH, AW, 2))
    for margin in (0, MARGIN):
        want = CO.accumulate(V, RT, valid, color, CAM, bits, margin=margin)
        got = NO.accumulate(V, RT, valid, color, CAM, bits, zero, S, margin=margin)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and want[1].sum() > 900


@functools.lru_cache(maxsize=None)
def zero_flow_normal():
    V, RT, valid, color, bits = fixed_poses()
    images = CO.gradients(color)
    prox = CO.proxy(*CO.accumulate(V, RT, valid, color, CAM, bits, margin=MARGIN))
    zero = np.zeros((6, AH, AW, 2))
    return prox, CO.normal(V, RT, valid, images, CAM, bits, prox, margin=MARGIN), NO.normal(V, RT, valid, images, CAM, bits, prox, zero, S,
                                                                                           margin=MARGIN)


def test_zero_flow_counts_sum_to_the_rigid_counts():
    _, (_, counts), (_, cell_counts) = zero_flow_normal()
    assert cell_counts.shape == (6, 12) and cell_counts.dtype == np.int32
    assert cell_counts.sum(axis=1).tolist() == counts.tolist() and (cell_counts > 0).sum() > 12        # pairs in many cells


def test_zero_flow_pose_blocks_are_the_rigid_rows_up_to_reordering():
    """The 6 x 6, the right-hand side and e of a pose, summed over its cells, are the rigid row's sums in another order: they differ
    by at most 2 (n - 1) 2^-53 sum |term| (each of the two orders is within (n - 1) 2^-53 sum |term| of the exact sum)."""
    V, RT, valid, color, bits = fixed_poses()
    prox, (rows, counts), (blocks, _) = zero_flow_normal()
    images, zero = CO.gradients(color), np.zeros((AH, AW, 2))
    pose_entries = [k for k, (i, j) in enumerate(NO.TRI) if j < 6] + [105 + i for i in range(6)] + [119]
    assert len(pose_entries) == 28
    for p in range(6):
        ids, cell, z = NO.terms(V, RT[p], valid[p], p, images[p], CAM, bits, prox, zero, S, 0.01, MARGIN)
        T = NO.block_terms(z)[:, pose_entries]
        assert len(ids) == counts[p] > 100
        bound = 2 * (len(ids) - 1) * 2.0 ** -53 * np.abs(T).sum(axis=0)
        got = blocks[p][:, pose_entries].sum(axis=0)
        assert (np.abs(got - rows[p]) <= bound).all(), p
        assert np.abs(rows[p]).min() > 0


# ------------------------------------------------------------------------------------------------------------ weights and Jacobian
def test_weights_sum_to_one_and_lattice_lines_open_their_cell():
    V, RT, valid, color, bits = fixed_poses()
    for p in range(6):
        q = NO.pairs(V, RT[p], valid[p], p, CAM, bits, some_flow()[p], S, 0.01, MARGIN, H, W)
        assert len(q['ids']) > 100
        assert (np.abs(q['w'].sum(axis=1) - 1.0) <= 2 * 2.0 ** -52).all() and (q['w'] >= 0).all()
        assert q['ci'].min() >= 0 and q['ci'].max() <= AH - 2 and q['cj'].min() >= 0 and q['cj'].max() <= AW - 2
    # a point on a lattice line, and one on the last line: u = 32 -> cell column 2, a = 0; u = 64 does not exist at W = 64, so 33 x 70
    Vl = np.array([[0.0, 0.0, 2.0], [0.5, 0.25, 2.0]])
    eye = np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])
    q = NO.pairs(Vl, eye, 1, 0, (32.0, 32.0, 32.0, 16.0), np.ones((2, 1), dtype=np.uint32), np.zeros((3, 6, 2)), 16, 0.01, 1, 33, 70)
    assert q['u'].tolist() == [32.0, 40.0] and q['v'].tolist() == [16.0, 20.0]
    assert q['cj'].tolist() == [2, 2] and q['ci'].tolist() == [1, 1] and q['w'][0].tolist() == [1.0, 0.0, 0.0, 0.0]
    q = NO.pairs(Vl[:1], eye, 1, 0, (32.0, 32.0, 64.0, 31.0), np.ones((1, 1), dtype=np.uint32), np.zeros((3, 6, 2)), 16, 0.01, 1, 33, 70)
    assert q['u'].tolist() == [64.0] and q['cj'].tolist() == [4] and q['ci'].tolist() == [1]             # v = 31 < 32: the last row of cells
    assert q['w'][0].tolist() == [1.0 * (1 - 15 / 16), 0.0, 15 / 16, 0.0]


def test_the_anchor_jacobian_is_the_derivative_of_the_sampled_intensity():
    """J[6:] against a central difference of the sampled intensity in every anchor offset.  The sample is bilinear in (u', v'), hence
    exactly linear in f while the warped position stays inside one pixel: pairs closer than 2 h to a pixel boundary are left out
    (w <= 1, so a displacement h of one anchor moves no pair by more than h), and the difference then holds to rounding - but the
    Jacobian uses the SOBEL derivative, the difference the bilinear one, so the two are compared on an image where both agree: a
    plane in x and y."""
    V, RT, valid, _, bits = fixed_poses()
    yy, xx = np.mgrid[0:H, 0:W]
    plane = np.clip(20 + 2 * xx + 1 * yy, 0, 255).astype(np.uint8)
    color = np.repeat(np.repeat(plane[None, :, :, None], 6, axis=0), 3, axis=3)
    images = CO.gradients(color)
    assert (images[0, 1:-1, 1:-1, 1] == 2 * 8 * 1000).all() and (images[0, 1:-1, 1:-1, 2] == 1 * 8 * 1000).all()
    flow = some_flow(amplitude=1.0)
    prox = np.zeros(len(V))
    h, p = 0.01, 2
    ids, cell, z = NO.terms(V, RT[p], valid[p], p, images[p], CAM, bits, prox, flow[p], S, 0.01, MARGIN)
    q = NO.pairs(V, RT[p], valid[p], p, CAM, bits, flow[p], S, 0.01, MARGIN, H, W)
    inside = np.ones(len(ids), dtype=bool)
    for pos in (q['uw'], q['vw']):
        frac = pos - np.floor(pos)
        inside &= (frac > 2 * h) & (frac < 1 - 2 * h) & (pos > MARGIN + 2 * h) & (pos < (W if pos is q['uw'] else H) - 1 - MARGIN - 2 * h)
    assert inside.sum() > 100
    checked = 0
    for i in range(AH):
        for j in range(AW):
            for c in range(2):
                up, down = flow[p].copy(), flow[p].copy()
                up[i, j, c] += h
                down[i, j, c] -= h
                ids_u, _, z_u = NO.terms(V, RT[p], valid[p], p, images[p], CAM, bits, prox, up, S, 0.01, MARGIN)
                ids_d, _, z_d = NO.terms(V, RT[p], valid[p], p, images[p], CAM, bits, prox, down, S, 0.01, MARGIN)
                assert np.array_equal(ids_u, ids) and np.array_equal(ids_d, ids)
                numeric = (z_u[:, 14] - z_d[:, 14]) / (2 * h)                 # r = I - proxy: d r = d I
                analytic = np.zeros(len(ids))
                for k, (di, dj) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                    hit = (q['ci'] + di == i) & (q['cj'] + dj == j)
                    analytic[hit] = z[hit, 6 + 2 * k + c]
                assert np.abs(numeric - analytic)[inside].max() < 1e-12, (i, j, c)
                checked += int((analytic[inside] != 0).sum())
    assert checked > 8 * 100                                            # every pair is seen through its four anchors, twice


# --------------------------------------------------------------------------------------------------------------- the host update
def test_the_host_update_is_the_restatements_byte_for_byte():
    V, RT, valid, color, bits = fixed_poses()
    images, flow = CO.gradients(color), some_flow(amplitude=0.5)
    flow[3] = 0.0
    prox = CO.proxy(*NO.accumulate(V, RT, valid, color, CAM, bits, flow, S, margin=MARGIN))
    blocks, counts = NO.normal(V, RT, valid, images, CAM, bits, prox, flow, S, margin=MARGIN)
    blocks, counts = blocks.copy(), counts.copy()
    counts[2] = 0
    counts[2, 0] = 15                                                   # one pair short of min_pairs
    valid = np.array([1, 1, 1, 1, 1, 0], dtype=np.uint8)                # pose 5 invalid
    free = np.array([1, 1, 1, 0, 1, 1], dtype=bool)                     # pose 3 held
    E0 = np.stack([np.linalg.inv(p) for p in scene()[3]])

    def both(anchor_weight, blocks):
        out = []
        for fn in (P.nonrigid_update, NO.update):
            E, f, status = E0.copy(), flow.copy(), np.zeros(6, dtype=np.int32)
            moved = fn(E, f, valid, free, blocks, counts, len(V), anchor_weight, 16, status)
            out.append((E, f, status, moved))
        (E, f, status, moved), (E2, f2, status2, moved2) = out
        assert E.tobytes() == E2.tobytes() and f.tobytes() == f2.tobytes()
        assert status.tolist() == status2.tolist() and moved.tolist() == moved2.tolist()
        return E, f, status, moved
    E, f, status, moved = both(0.316, blocks)
    assert moved.tolist() == [True, True, False, False, True, False]
    assert status.tolist() == [0, 0, P.COLORMAP_FEW_PAIRS, 0, 0, 0]
    for p in (2, 3, 5):
        assert E[p].tobytes() == E0[p].tobytes() and f[p].tobytes() == flow[p].tobytes()
    assert not f[3].any()                                               # a held pose keeps its zero flow
    for p in (0, 1, 4):
        assert E[p].tobytes() != E0[p].tobytes() and (f[p] != flow[p]).all()
    # anchor_weight = 0 with an anchor that no pair touches: pose 4's pairs taken out of every cell round anchor (0, 0)
    untouched = blocks.copy()
    untouched[4, 0] = 0.0
    E, f, status, moved = both(0.0, untouched)
    assert status[4] == P.COLORMAP_SINGULAR and not moved[4]
    assert E[4].tobytes() == E0[4].tobytes() and f[4].tobytes() == flow[4].tobytes()
    # the same anchor under the regulariser alone: pulled to zero, exactly by its own equation wgt^2 x = -wgt^2 f
    E, f, status, moved = both(0.316, untouched)
    assert moved[4] and status[4] == 0 and np.abs(f[4, 0, 0]).max() < 1e-12 and np.abs(flow[4, 0, 0]).min() > 0


def test_the_host_update_at_the_papers_lattice_size():
    """16 x 21 anchors, 678 unknowns: the vectorised assembly of nonrigid_update against the restatement's loops, a block of -0.0
    included (symmetrising must not turn the signs of zeros differently on the two sides)."""
    rng = np.random.default_rng(0)
    n, ah, aw = 2, 16, 21
    z = rng.standard_normal((n, 15 * 20, 20, 15))
    blocks = np.stack([[NO.block_terms(z[p, c]).sum(axis=0) for c in range(15 * 20)] for p in range(n)])
    blocks[0, 7] = -0.0
    counts = np.full((n, 15 * 20), 20, dtype=np.int32)
    E0, flow = np.stack([np.eye(4)] * n), rng.standard_normal((n, ah, aw, 2))
    got = []
    for fn in (P.nonrigid_update, NO.update):
        E, f, status = E0.copy(), flow.copy(), np.zeros(n, dtype=np.int32)
        assert fn(E, f, np.ones(n, dtype=np.uint8), np.ones(n, dtype=bool), blocks, counts, 20000, 0.316, 16, status).all() and not status.any()
        got.append((E, f))
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes()
    assert (got[0][1] != flow).all()


# ----------------------------------------------------------------------------------------------------------------------- recovery
def warped_frame(frame, amplitude):
    """The frame as a camera with a smooth distortion of `amplitude` pixels would have recorded it: resampled bilinearly at
    (x + dx, y + dy), dx = amplitude sin(2 pi y / (H - 1)) (a shear that changes sign down the frame, as a rolling shutter gives),
    dy = amplitude / 2 sin(2 pi x / (W - 1)).  No rigid pose produces it."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    x = np.clip(xx + amplitude * np.sin(2 * np.pi * yy / (H - 1)), 0, W - 1)
    y = np.clip(yy + 0.5 * amplitude * np.sin(2 * np.pi * xx / (W - 1)), 0, H - 1)
    out = CO._sample(frame.astype(np.float64), x.reshape(-1), y.reshape(-1))
    return np.rint(out).astype(np.uint8).reshape(H, W, 3)


@functools.lru_cache(maxsize=None)
def recovery(amplitude=1.5):
    """The scene of tests/test_colormap.py (on the denser wall) with exact poses, frame FREED resampled through a smooth warp, all
    other frames held: -> (V, C, poses, colour frames, bits, free, the restatement's non-rigid (poses, flow, info), its rigid (poses,
    info)).  anchor_weight: every frame sees 30 % of this wall's vertices, where a frame of a scan sees a percent or so of a mesh,
    and the regulariser's weight is anchor_weight n_p / N: 0.03 here weighs the anchors as the default 0.316 does at n_p / N = 0.03."""
    V, _, C, poses, color, _, bits = scene(DENSE)
    color = color.copy()
    color[FREED] = warped_frame(color[FREED], amplitude)
    free = np.zeros(6, dtype=bool)
    free[FREED] = True
    nonrigid = NO.optimize(V, poses, color, CAM, bits, S, iterations=ITERATIONS, anchor_weight=ANCHOR_WEIGHT, free=free, margin=MARGIN)
    rigid = CO.optimize(V, poses, color, CAM, bits, iterations=ITERATIONS, free=free, margin=MARGIN)
    return V, C, poses, color, bits, free, nonrigid, rigid


def oracle_colour_error(V, C, poses, color, bits, flow):
    RT, valid = P.pose_extrinsics(poses)
    total, count = NO.accumulate(V, RT, valid, color, CAM, bits, flow, S, margin=MARGIN)
    lit = count > 0
    got = (total[lit] / (count[lit, None] * 16711680.0)).astype(np.float32)
    return float(np.abs(got.astype(np.float64) - C[lit]).mean()), int(lit.sum())


def test_a_smooth_warp_of_one_frame_is_removed_where_a_rigid_pose_cannot():
    V, C, poses, color, bits, free, (out, flow, info), (rigid_out, rigid_info) = recovery()
    e, e_rigid = info['residual'][:, FREED], rigid_info['residual'][:, FREED]
    print('free frame: e %.6f -> %.6f non-rigid, -> %.6f rigid only; |flow| %.3f px; pairs %d'
          % (e[0], e[-1], e_rigid[-1], info['flow_norm'][-1, FREED], info['pairs'][0, FREED]))
    n = int(info['pairs'][0, FREED])
    assert abs(e[0] - e_rigid[0]) <= 2 * (n - 1) * 2.0 ** -53 * e[0]    # the same start, summed in another order (the terms are r r >= 0)
    assert e[-1] < e[0]
    assert e[-1] < e_rigid[-1]
    held = [p for p in range(6) if p != FREED]
    assert out[held].tobytes() == poses[held].tobytes() and not flow[held].any()
    assert info['status'].tolist() == [NO.NOT_FREE if p != FREED else 0 for p in range(6)]
    assert info['residual'].shape == info['pairs'].shape == info['flow_norm'].shape == (ITERATIONS + 1, 6)
    assert not info['flow_norm'][0].any() and 0.5 < info['flow_norm'][-1, FREED] < 3.0 and not info['flow_norm'][:, held].any()
    # and the colours it is for (the GPU test repeats this through vertex_colors_from_frames)
    zero = np.zeros_like(flow)
    err_rigid, lit = oracle_colour_error(V, C, rigid_out, color, bits, zero)
    err_nonrigid, _ = oracle_colour_error(V, C, out, color, bits, flow)
    print('mean absolute colour error over %d vertices: rigid only %.6f, non-rigid %.6f' % (lit, err_rigid, err_nonrigid))
    assert err_nonrigid <= err_rigid


# ---------------------------------------------------------------------------------------------------------------------- arguments
def test_argument_errors_are_raised_before_any_library_call():
    V, _, _, poses, color, depth, bits = scene()
    v, c, d = torch.from_numpy(V), torch.from_numpy(color), torch.from_numpy(depth)
    b = torch.from_numpy(bits.view(np.int32)).view(torch.uint32)
    kw = dict(color_camera=CAM, margin=MARGIN)
    with pytest.raises(ValueError, match='exactly one of depth and bits'):
        P.optimize_poses_nonrigid(v, poses, c, **kw)
    with pytest.raises(ValueError, match='margin must be >= 1'):
        P.optimize_poses_nonrigid(v, poses, c, depth=d, color_camera=CAM, margin=0)
    with pytest.raises(ValueError, match='lattice_step must be >= 1'):
        P.optimize_poses_nonrigid(v, poses, c, depth=d, lattice_step=0, **kw)
    with pytest.raises(ValueError, match='rigid_iterations'):
        P.optimize_poses_nonrigid(v, poses, c, depth=d, rigid_iterations=-1, **kw)
    with pytest.raises(ValueError, match='free must be bool'):
        P.optimize_poses_nonrigid(v, poses, c, depth=d, free=np.ones(5, dtype=bool), **kw)
    with pytest.raises(TypeError, match='color must be a CUDA tensor'):
        P.optimize_poses_nonrigid(v, poses, c, depth=d, **kw)           # CPU tensors: there is no CPU fallback
    fc = P.FrameColors.__new__(P.FrameColors)                           # add() checks the flow before it touches the object
    with pytest.raises(ValueError, match='flow needs bits mode'):
        P.FrameColors.add(fc, poses, c, depth=d, flow=np.zeros((6, AH, AW, 2)), lattice_step=S)
    with pytest.raises(ValueError, match='flow must be float64'):
        P._nonrigid_flow(np.zeros((6, AH, AW + 1, 2)), S, 6, H, W)
    with pytest.raises(ValueError, match='flow must be float64'):
        P._nonrigid_flow(np.zeros((6, AH, AW, 2), dtype=np.float32), S, 6, H, W)
    with pytest.raises(ValueError, match='lattice_step'):
        P._nonrigid_flow(np.zeros((6, AH, AW, 2)), None, 6, H, W)
    assert P._nonrigid_flow(np.zeros((6, AH, AW, 2)), S, 6, H, W)[0].shape == (6, AH, AW, 2)
