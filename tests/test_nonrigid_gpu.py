"""The non-rigid colour-map optimisation on the GPU (csrc/stin_nonrigid.hip through preprocessing.optimize_poses_nonrigid and its
launch helpers): equal to the numpy restatement of the contract (tests/_nonrigid_oracle.py) byte for byte - `tobytes()` of the
warped colour sums on both routes, of the blocks and counts of every (pose, cell) for every batching, and of the poses, flows,
residuals and pair counts of whole optimisations in bits and in depth mode - and good for what it is for: on a frame that was
warped smoothly, the colours averaged with the returned poses and flow are no worse than with the rigid optimiser's poses."""
import functools

import numpy as np
import pytest
import torch

import _colormap_oracle as CO
import _frames_oracle as FO
import _nonrigid_oracle as NO
from surface_texture_inpainting_net_amd import _lib, preprocessing as P
from test_colormap import CAM, FREED, MARGIN, perturbed, scene
from test_nonrigid import ANCHOR_WEIGHT, ITERATIONS, S, recovery

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu
OWNER, SPLIT = _lib.CONSTANTS['STIN_FRAMES_ROUTE_OWNER'], _lib.CONSTANTS['STIN_FRAMES_ROUTE_SPLIT']


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_bits(b):
    return dev(np.ascontiguousarray(b).view(np.int32)).view(torch.uint32)


def host(t):
    return t.cpu().numpy()


# --------------------------------------------------------------------------------------------------------------- the dense scene
DENSE_CAM = (32.0, 32.0, 32.0, 16.0)
SHAPES = {'48x64': (48, 64), '33x70': (33, 70)}                         # 3 x 4 cells; 2 x 5 cells, the last column and row ragged


@functools.lru_cache(maxsize=None)
def dense_scene(n, shape):
    """(V, poses [5], colour frames, bits {ones, random}, flow): n vertices on the plane z = 2 over x, y in [0, 1).  Pose 0 is the
    identity: u = 32 + 16 x, v = 16 + 16 y EXACTLY, so all of them project into cell (1, 2) - 2 304 pairs, eighteen staging rounds,
    every other cell empty - and those with x = 0 or y = 0 sit on the lattice lines u = 32, v = 16.  Pose 1 and 4 are shifted, pose
    3 is turned (pairs in several cells; pose 4 has some left of the frame), pose 2 is lost.  The flow is random within 1.5 pixels, except
    that pose 0's anchor (2, 3) is pushed 20 pixels down: the pairs near it leave the frame although their unwarped positions are
    well inside."""
    H, W = SHAPES[shape]
    side = 48 if n == 2304 else 7
    g = np.arange(side, dtype=np.float64) / side
    V = np.stack([np.repeat(g, side), np.tile(g, side), np.full(side * side, 2.0)], axis=1)[:n]
    assert V.shape == (n, 3)
    poses = np.stack([np.eye(4)] * 5)
    poses[1, :3, 3] = [0.25, 0.125, 0.0]
    poses[2] = -np.inf
    c, s = np.cos(0.2), np.sin(0.2)
    poses[3, :3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    poses[3, :3, 3] = [-0.5, 0.0, 0.125]
    poses[4, :3, 3] = [2.5, -0.75, -0.5]
    rng = np.random.default_rng(n + H)
    color = rng.integers(0, 256, (5, H, W, 3), dtype=np.uint8)
    ones = np.full((n, 1), 0xFFFFFFFF, dtype=np.uint32)
    some = rng.integers(0, 32, (n, 1)).astype(np.uint32) | np.uint32(1 << 3)      # pose 3 sees everything, the others about half
    Ah, Aw = NO.lattice(H, W, S)
    flow = rng.uniform(-1.5, 1.5, (5, Ah, Aw, 2))
    flow[0, 2, 3, 1] = 20.0
    return V, poses, color, {'ones': ones, 'random': some}, flow


@functools.lru_cache(maxsize=None)
def dense_want(n, shape, which, margin=1):
    V, poses, color, bits, flow = dense_scene(n, shape)
    RT, valid = P.pose_extrinsics(poses)
    total, count = NO.accumulate(V, RT, valid, color, DENSE_CAM, bits[which], flow, S, margin=margin)
    prox = CO.proxy(total, count)
    blocks, counts = NO.normal(V, RT, valid, CO.gradients(color), DENSE_CAM, bits[which], prox, flow, S, margin=margin)
    return RT, valid, total, count, prox, blocks, counts


def test_the_dense_scene_is_what_its_docstring_says():
    V, poses, color, bits, flow = dense_scene(2304, '48x64')
    RT, valid, _, _, _, blocks, counts = dense_want(2304, '48x64', 'ones')
    q = NO.pairs(V, RT[0], valid[0], 0, DENSE_CAM, bits['ones'], flow[0], S, 0.01, 1, 48, 64)
    unwarped = CO._pairs(V, RT[0], valid[0], 0, DENSE_CAM, bits['ones'], 0.01, 1, 48, 64)
    assert len(unwarped[0]) == 2304 and unwarped[4].min() == 32.0 and unwarped[5].min() == 16.0
    assert (unwarped[4] == 32.0).sum() == 48 and (unwarped[5] == 16.0).sum() == 48              # on the lattice lines
    assert 0 < 2304 - len(q['ids']) < 600                               # pairs that the warp takes out of the frame
    assert counts[0, 1 * 4 + 2] == len(q['ids']) > 128 * 13 and counts[0].sum() == len(q['ids'])
    assert not blocks[0, [c for c in range(12) if c != 6]].any()
    assert not counts[2].any() and not blocks[2].any() and not np.signbit(blocks[2]).any()      # the lost pose
    assert (counts[[1, 3, 4]] > 0).sum(axis=1).min() >= 2               # several cells
    assert 0 < counts[4].sum() < 2304                                   # some outside the frame


# ---------------------------------------------------------------------------------------------------------- the warped accumulate
def gpu_accumulate(V, poses, color, bits, flow, margin, route, cuts, cam=DENSE_CAM):
    fc = P.FrameColors(dev(V), cam, margin=margin, num_poses=len(poses))
    for p0, p1 in zip(cuts[:-1], cuts[1:]):
        fc.add(poses[p0:p1], dev(color[p0:p1]), bits=dev_bits(bits), first_pose=p0, _route=route,
               flow=None if flow is None else flow[p0:p1], lattice_step=None if flow is None else S)
    return host(fc.sum), host(fc.count), host(fc.seen)


@pytest.mark.parametrize('route', [OWNER, SPLIT])
@pytest.mark.parametrize('n,shape', [(2304, '48x64'), (37, '33x70')])
def test_zero_flow_accumulate_is_the_frame_kernel(n, shape, route):
    V, poses, color, bits, flow = dense_scene(n, shape)
    for margin in (0, 2):
        want = gpu_accumulate(V, poses, color, bits['random'], None, margin, route, [0, 5])
        got = gpu_accumulate(V, poses, color, bits['random'], np.zeros_like(flow), margin, route, [0, 5])
        assert want[1].sum() > n // 4
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


@pytest.mark.parametrize('route', [OWNER, SPLIT])
@pytest.mark.parametrize('which', ['ones', 'random'])
@pytest.mark.parametrize('n,shape', [(2304, '48x64'), (37, '48x64'), (2304, '33x70'), (37, '33x70')])
def test_warped_accumulate_is_the_restatement(n, shape, which, route):
    V, poses, color, bits, flow = dense_scene(n, shape)
    _, _, total, count, _, _, _ = dense_want(n, shape, which)
    zero = gpu_accumulate(V, poses, color, bits[which], None, 1, route, [0, 5])
    assert zero[0].tobytes() != total.tobytes()                         # the flow matters
    for cuts in ([0, 5], [0, 2, 5], [0, 1, 2, 3, 4, 5]):
        got = gpu_accumulate(V, poses, color, bits[which], flow, 1, route, cuts)
        assert got[0].tobytes() == total.tobytes() and got[1].tobytes() == count.tobytes(), cuts
        assert int(FO.pack_seen(np.zeros((n, 5), dtype=bool)).size) == got[2].size and (np.bitwise_count(got[2]).sum() == count.sum())


# --------------------------------------------------------------------------------------------------------------- blocks and counts
def gpu_blocks(n, shape, which, cuts, margin=1):
    V, poses, color, bits, flow = dense_scene(n, shape)
    RT, valid, _, _, prox, _, _ = dense_want(n, shape, which, margin)
    H, W = SHAPES[shape]
    cells = (NO.lattice(H, W, S)[0] - 1) * (NO.lattice(H, W, S)[1] - 1)
    v, rt, ok, b, px, fl = dev(V), dev(RT), dev(valid), dev_bits(bits[which]), dev(prox), dev(flow)
    images = P._colormap_gradients(dev(color))
    blocks = torch.full((5, cells, 120), float('nan'), dtype=torch.float64, device=DEV)
    counts = torch.full((5, cells), -1, dtype=torch.int32, device=DEV)
    keys = P._nonrigid_workspace(n, max(p1 - p0 for p0, p1 in zip(cuts[:-1], cuts[1:])), H, W, S, DEV)
    for p0, p1 in zip(cuts[:-1], cuts[1:]):
        P._nonrigid_normal(v, rt[p0:p1], ok[p0:p1], p0, images[p0:p1], fl[p0:p1], S, DENSE_CAM, 0.01, b, margin, px, blocks[p0:p1],
                           counts[p0:p1], keys)
    return host(blocks), host(counts)


@pytest.mark.parametrize('which', ['ones', 'random'])
@pytest.mark.parametrize('n,shape', [(2304, '48x64'), (37, '48x64'), (2304, '33x70'), (37, '33x70')])
def test_blocks_and_counts_for_every_batching(n, shape, which):
    _, _, _, count, _, blocks, counts = dense_want(n, shape, which)
    assert int(counts.sum()) == int(count.sum()) > 0
    first = None
    for cuts in ([0, 5], [0, 1, 2, 3, 4, 5], [0, 2, 4, 5], [0, 3, 5], [0, 5]):      # batches of P, 1, 2; a first_pose split; again
        got_blocks, got_counts = gpu_blocks(n, shape, which, cuts)
        assert got_counts.tobytes() == counts.tobytes(), cuts
        assert got_blocks.tobytes() == blocks.tobytes(), cuts
        first = first if first is not None else got_blocks
        assert got_blocks.tobytes() == first.tobytes()


def test_no_vertices_and_no_poses():
    V, poses, color, bits, flow = dense_scene(37, '48x64')
    RT, valid, _, _, prox, _, _ = dense_want(37, '48x64', 'ones')
    images, fl = P._colormap_gradients(dev(color)), dev(flow)
    blocks = torch.full((5, 12, 120), -1.0, dtype=torch.float64, device=DEV)
    counts = torch.full((5, 12), 5, dtype=torch.int32, device=DEV)
    keys = P._nonrigid_workspace(0, 5, 48, 64, S, DEV)
    P._nonrigid_normal(dev(V[:0]), dev(RT), dev(valid), 0, images, fl, S, DENSE_CAM, 0.01, dev_bits(bits['ones'][:0]), 1, dev(prox[:0]),
                       blocks, counts, keys)
    assert not host(blocks).any() and not np.signbit(host(blocks)).any() and not host(counts).any()
    keys = P._nonrigid_workspace(37, 5, 48, 64, S, DEV)
    P._nonrigid_normal(dev(V), dev(RT[:0]), dev(valid[:0]), 0, images[:0], fl[:0], S, DENSE_CAM, 0.01, dev_bits(bits['ones']), 1, dev(prox),
                       blocks[:0], counts[:0], keys)
    out, f, info = P.optimize_poses_nonrigid(dev(V), poses[:0], dev(color[:0]), bits=dev_bits(bits['ones']), color_camera=DENSE_CAM,
                                             margin=1, iterations=2, lattice_step=S)
    assert out.shape == (0, 4, 4) and f.shape == (0, 4, 5, 2) and info['residual'].shape == (3, 0) and info['flow_norm'].shape == (3, 0)
    fc = P.FrameColors(dev(V[:0]), DENSE_CAM, margin=1)
    fc.add(poses, dev(color), bits=dev_bits(bits['ones'][:0]), flow=flow, lattice_step=S)
    assert fc.count.shape == (0,)


# ------------------------------------------------------------------------------------------------------------------- end to end
def same(got, want):
    (gp, gf, gi), (wp, wf, wi) = got, want
    assert gp.dtype == np.float64 and gf.dtype == np.float64 and gp.shape == wp.shape and gf.shape == wf.shape
    assert gi['pairs'].tobytes() == wi['pairs'].tobytes()
    assert gi['residual'].tobytes() == wi['residual'].tobytes()
    assert gi['status'].tobytes() == wi['status'].tobytes() and gi['flow_norm'].tobytes() == wi['flow_norm'].tobytes()
    assert gf.tobytes() == wf.tobytes() and gp.tobytes() == wp.tobytes()


def perturbed_start():
    poses = scene()[3]
    start = poses.copy()
    for p in range(1, 6):
        start[p] = perturbed(poses[p], 0.52 * (1 if p % 2 else -1), 0.010 + 0.001 * p)
    start[4] = np.nan                                                   # and one lost pose
    free = np.ones(6, dtype=bool)
    free[0] = False
    return start, free


@pytest.mark.parametrize('mode', ['bits', 'depth'])
def test_whole_optimisations_are_the_restatements(mode):
    V, _, _, _, color, depth, bits = scene()
    start, free = perturbed_start()
    if mode == 'depth':
        _, _, seen = FO.accumulate(V, start, color, CAM, depth=depth, margin=MARGIN)
        vis, how = FO.pack_seen(seen), dict(depth=dev(depth))
    else:
        vis, how = bits, dict(bits=dev_bits(bits))
    want = NO.optimize(V, start, color, CAM, vis, S, iterations=4, free=free, margin=MARGIN)
    first = None
    for batch in (4, 1, 64):
        got = P.optimize_poses_nonrigid(dev(V), start, dev(color), color_camera=CAM, margin=MARGIN, iterations=4, lattice_step=S,
                                        free=free, batch=batch, **how)
        same(got, want)
        assert got[2]['lattice_step'] == S
    poses, flow, info = got
    e = info['residual'].sum(axis=1)
    print('%s mode: e %.6f -> %.6f, pairs %d, |flow| %.3f px' % (mode, e[0], e[-1], info['pairs'][0].sum(), info['flow_norm'][-1].max()))
    assert e[-1] < e[0] and info['status'][0] == P.COLORMAP_NOT_FREE and info['status'][4] == P.COLORMAP_INVALID
    assert poses[0].tobytes() == start[0].tobytes() and np.isnan(poses[4]).all() and not flow[[0, 4]].any() and flow[1].any()
    assert info['flow_norm'].shape == (5, 6) and not info['flow_norm'][0].any()


def test_the_default_lattice_step_comes_from_the_vertical_anchors():
    V, _, _, poses, color, _, bits = scene()
    _, flow, info = P.optimize_poses_nonrigid(dev(V), poses, dev(color), bits=dev_bits(bits), color_camera=CAM, margin=MARGIN,
                                              iterations=0, vertical_anchors=4)
    assert info['lattice_step'] == 16 and flow.shape == (6, 4, 5, 2) and not flow.any()      # ceil(47 / 3)
    _, flow, info = P.optimize_poses_nonrigid(dev(V), poses, dev(color), bits=dev_bits(bits), color_camera=CAM, margin=MARGIN, iterations=0)
    assert info['lattice_step'] == 4 and flow.shape == (6, 13, 17, 2)   # ceil(47 / 15): 16 anchors would overshoot, 13 cover 48 rows


def test_rigid_iterations_run_the_rigid_optimiser_first():
    V, _, _, _, color, _, bits = scene()
    start, free = perturbed_start()
    kw = dict(bits=dev_bits(bits), color_camera=CAM, margin=MARGIN, free=free)
    rigid_poses, rigid_info = P.optimize_poses_rigid(dev(V), start, dev(color), iterations=3, **kw)
    want = P.optimize_poses_nonrigid(dev(V), rigid_poses, dev(color), iterations=2, lattice_step=S, **kw)
    got = P.optimize_poses_nonrigid(dev(V), start, dev(color), iterations=2, rigid_iterations=3, lattice_step=S, **kw)
    same(got, want)
    assert all(got[2]['rigid'][k].tobytes() == rigid_info[k].tobytes() for k in rigid_info)
    assert got[0][1].tobytes() != rigid_poses[1].tobytes() and 'rigid' not in want[2]


# ------------------------------------------------------------------------------------------------------------------ the colours
def test_the_returned_poses_and_flow_give_colours_no_worse_than_the_rigid_poses():
    V, C, poses, color, bits, free, want, (rigid_poses, rigid_info) = recovery()
    kw = dict(bits=dev_bits(bits), color_camera=CAM, margin=MARGIN)
    got = P.optimize_poses_nonrigid(dev(V), poses, dev(color), iterations=ITERATIONS, lattice_step=S, anchor_weight=ANCHOR_WEIGHT,
                                    free=free, **kw)
    same(got, want)
    out, flow, info = got
    r_poses, r_info = P.optimize_poses_rigid(dev(V), poses, dev(color), iterations=ITERATIONS, free=free, **kw)
    assert r_poses.tobytes() == rigid_poses.tobytes() and r_info['residual'].tobytes() == rigid_info['residual'].tobytes()
    assert info['residual'][-1, FREED] < info['residual'][0, FREED] and info['residual'][-1, FREED] < r_info['residual'][-1, FREED]
    err = []
    for p, f in ((r_poses, None), (out, flow)):
        colors, count = P.vertex_colors_from_frames(dev(V), p, dev(color), flow=f, lattice_step=None if f is None else S, **kw)
        lit = host(count) > 0
        assert lit.sum() > 900
        err.append(float(np.abs(host(colors)[lit].astype(np.float64) - C[lit]).mean()))
    print('mean absolute colour error: rigid only %.6f, non-rigid %.6f' % tuple(err))
    assert err[1] <= err[0]


def test_vertex_colours_with_a_flow_in_depth_mode_take_two_passes():
    V, _, _, poses, color, depth, _ = scene()
    flow = np.random.default_rng(4).uniform(-1.5, 1.5, (6, 4, 5, 2))
    kw = dict(color_camera=CAM, margin=MARGIN, batch=4)
    colors, count, seen = P.vertex_colors_from_frames(dev(V), poses, dev(color), depth=dev(depth), flow=flow, lattice_step=S,
                                                      return_seen=True, **kw)
    _, _, vis = FO.accumulate(V, poses, color, CAM, depth=depth, margin=MARGIN)          # the unwarped pass fixes the visibility
    RT, valid = P.pose_extrinsics(poses)
    total, n = NO.accumulate(V, RT, valid, color, CAM, FO.pack_seen(vis), flow, S, margin=MARGIN)
    assert host(count).tobytes() == n.tobytes() and host(colors).tobytes() == FO.finish(total, n)[0].tobytes() and n.sum() > 100
    assert np.bitwise_count(host(seen)).sum() == n.sum() <= vis.sum()


def test_without_a_flow_every_path_gives_the_bytes_it_gave():
    V, _, _, poses, color, depth, bits = scene()
    for how, kw in ((dict(depth=dev(depth)), dict(depth=depth)), (dict(bits=dev_bits(bits)), dict(bits=bits))):
        want, want_count, want_seen, _ = FO.colors(V, poses, color, CAM, margin=MARGIN, **kw)
        for batch in (64, 4):
            colors, count, seen = P.vertex_colors_from_frames(dev(V), poses, dev(color), color_camera=CAM, margin=MARGIN, batch=batch,
                                                              return_seen=True, **how)
            assert host(colors).tobytes() == want.tobytes() and host(count).tobytes() == want_count.tobytes()
            assert host(seen).tobytes() == FO.pack_seen(want_seen).tobytes()


def test_a_scan_directory_goes_through_the_optimiser_when_asked(tmp_path):
    pytest.importorskip('PIL')
    from surface_texture_inpainting_net_amd import scene_io
    from test_resize_gpu import SCAN_KW, write_scan
    root = str(tmp_path / 'scan')
    poses, cam = write_scan(root)
    g = np.linspace(-0.55, 0.55, 5)
    V = dev(np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=3).reshape(-1, 3))      # 125 points inside the rendered sphere's cube
    V = V / V.norm(dim=1, keepdim=True).clamp_min(0.1)                                 # on the unit sphere the depth frames show
    colors, count = P.scan_vertex_colors(V, root, width=16, height=12, trajectory_slice=slice(None), batch=2, nonrigid_iterations=2, **SCAN_KW)
    files = scene_io.scan_frame_files(root)
    color, depth = scene_io.read_frames(files['color'], files['depth'])
    small, d = P.resize_u8(dev(color), (12, 16)), dev(depth)
    out, flow, info = P.optimize_poses_nonrigid(V, poses, small, depth=d, color_camera=cam, iterations=2, batch=2, **SCAN_KW)
    assert info['lattice_step'] == 1 and flow.shape == (3, 12, 16, 2) and int(info['pairs'][0].sum()) > 48 and flow.any()
    want, want_count = P.vertex_colors_from_frames(V, out, small, depth=d, color_camera=cam, flow=flow, lattice_step=1, **SCAN_KW)
    # two undamped steps of 390 unknowns on some 36 pairs of JPEG frames per pose are no optimisation to judge: the test is the chain
    assert host(colors).tobytes() == host(want).tobytes() and torch.equal(count, want_count) and int(count.sum()) > 0
    plain, _ = P.scan_vertex_colors(V, root, width=16, height=12, trajectory_slice=slice(None), batch=2, **SCAN_KW)
    assert host(plain).tobytes() != host(colors).tobytes()


# -------------------------------------------------------------------------------------------------------------------- arguments
def test_wrong_arguments_are_refused():
    V, _, _, poses, color, depth, bits = scene()
    v, c, d, b = dev(V), dev(color), dev(depth), dev_bits(bits)
    kw = dict(color_camera=CAM, iterations=1)
    with pytest.raises(ValueError, match='margin must be >= 1'):
        P.optimize_poses_nonrigid(v, poses, c, bits=b, margin=0, **kw)
    with pytest.raises(ValueError, match='lattice_step must be >= 1'):
        P.optimize_poses_nonrigid(v, poses, c, bits=b, margin=MARGIN, lattice_step=0, **kw)
    with pytest.raises(TypeError):
        P.optimize_poses_nonrigid(v, poses, c.float(), depth=d, margin=MARGIN, **kw)
    with pytest.raises(ValueError):
        P.optimize_poses_nonrigid(v, poses, c[:5], depth=d, margin=MARGIN, **kw)
    fc = P.FrameColors(v, CAM, margin=MARGIN)
    zero = np.zeros((6, 4, 5, 2))
    with pytest.raises(ValueError, match='flow needs bits mode'):
        fc.add(poses, c, depth=d, flow=zero, lattice_step=S)
    with pytest.raises(ValueError, match='flow must be float64'):
        fc.add(poses, c, bits=b, flow=zero[:, :3], lattice_step=S)
    with pytest.raises(ValueError, match='flow must be float64'):
        fc.add(poses, c, bits=b, flow=zero.astype(np.float32), lattice_step=S)
    with pytest.raises(ValueError, match='flow must be float64'):
        fc.add(poses, c, bits=b, flow=zero, lattice_step=8)
    with pytest.raises(ValueError, match='lattice_step'):
        fc.add(poses, c, bits=b, flow=zero)
    with pytest.raises(ValueError, match='lattice_step must be >= 1'):
        P.vertex_colors_from_frames(v, poses, c, bits=b, color_camera=CAM, margin=MARGIN, flow=zero, lattice_step=0)
    with pytest.raises(ValueError, match='flow must be float64'):
        P.vertex_colors_from_frames(v, poses, c, depth=d, color_camera=CAM, margin=MARGIN, flow=zero[:5], lattice_step=S)
    assert not host(fc.count).any()                                     # nothing was launched
    lib = _lib.load()
    assert lib.stin_nonrigid_workspace_bytes(100, 4, 48, 64, 16) == 100 * 4 * 8
    assert lib.stin_nonrigid_workspace_bytes(100, 4, 1, 64, 16) == 0 and lib.stin_nonrigid_workspace_bytes(100, 4, 48, 64, 0) == 0
    assert lib.stin_nonrigid_workspace_bytes(100, 4096, 16384, 16384, 1) == 0          # B cells beyond 2^31
