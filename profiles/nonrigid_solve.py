"""Timing of the non-rigid optimisation's linear solve on the device (csrc/stin_nonrigid_solve.hip, preprocessing.nonrigid_solve,
optimize_poses_nonrigid(solver='banded')) on one GPU, with the host solve ('dense') on the same scene in the same run as the figure
to set it beside.

    python profiles/nonrigid_solve.py [--out FILE] [--side 448] [--poses 128] [--batch 64] [--lattice-step 32] [--reps 7]
                                      [--iterations 2] [--only kernels]

Scene and method: profiles/nonrigid.py's - the 200 704-vertex grid mesh with ids in random order, `poses` cameras, 480 x 640
frames, the visibility bits of one FrameColors pass in depth mode, a flow random within one pixel; HIP events around one call on
buffers allocated beforehand, no host read inside, two warm-up calls, the median of `reps`; the arms alternate inside every
repetition.

* the three kernels of stin_nonrigid_solve_f64 alone (stin_nonrigid_solve_stages_f64: stats, assemble, factor - in this order
  inside a repetition, so the factor kernel always finds a freshly assembled workspace) and the whole call;
* the read-back of x, residual, pairs and status, beside the read-back of the blocks and counts that 'dense' needs
  (time.perf_counter around synchronised copies);
* the host update of all poses under 'dense' (nonrigid_update, wall clock) and the scaled residual of the device's x against
  LAPACK's on the first poses' systems;
* one iteration end to end under 'banded' and under 'dense', alternating: wall clock of optimize_poses_nonrigid with `iterations`
  and with 0 iterations, the difference divided by `iterations`.
* --only kernels: one call, for a `rocprofv3 --kernel-trace --stats` run.
Prints one JSON line per measurement."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'profiles'))

import _levels_oracle as LO  # noqa: E402
from colormap import CAM, DEV, H, MARGIN, W, emit, timed, walk_poses  # noqa: E402
from nonrigid import wall  # noqa: E402
from surface_texture_inpainting_net_amd import _lib, preprocessing as P, views  # noqa: E402
from surface_texture_inpainting_net_amd.plan import _ptr, _stream  # noqa: E402

ANCHOR_WEIGHT, MIN_PAIRS = 0.316, 16


def scaled_residual(A, b, x):
    r = A.astype(np.longdouble) @ x.astype(np.longdouble) + b.astype(np.longdouble)
    return float(np.abs(r).max() / (2.0 ** -53 * (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--side', type=int, default=448)            # 448^2 = 200 704 vertices
    ap.add_argument('--poses', type=int, default=128)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--lattice-step', type=int, default=32)     # 16 x 21 anchors at 480 x 640: 678 unknowns per frame
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--iterations', type=int, default=2)
    ap.add_argument('--only', default=None, choices=[None, 'kernels'])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('profiles/nonrigid_solve.py measures on a GPU; none is visible (nothing is timed on the CPU)')
    f = open(args.out, 'a') if args.out else None
    props = torch.cuda.get_device_properties(0)
    emit(f, what='device', name=props.name, cus=int(props.multi_processor_count), lib=_lib.LIB_PATH)
    mesh = LO.grid_mesh(args.side, 1, spacing=0.02)
    Vn = mesh['vertices']
    n, B, step, S = int(Vn.shape[0]), args.poses, args.batch, args.lattice_step
    C = np.stack([0.5 + 0.45 * np.sin(3.1 * Vn[:, 0]) * np.cos(2.3 * Vn[:, 1]), 0.5 + 0.45 * np.cos(2.7 * Vn[:, 0] + 0.5),
                  0.5 + 0.45 * np.sin(1.9 * Vn[:, 0] + 2.9 * Vn[:, 1])], axis=1).astype(np.float32)
    poses = walk_poses(Vn, B)
    V, F = torch.from_numpy(Vn).to(DEV), torch.from_numpy(mesh['faces']).to(DEV)
    r = views.render_mesh(V, F, torch.from_numpy(C).to(DEV), poses, CAM, H, W, depth=True)
    color, depth = r.color.contiguous(), r.depth.contiguous()
    fc = P.FrameColors(V, CAM, margin=MARGIN, num_poses=B)
    for p0 in range(0, B, step):
        fc.add(poses[p0:p0 + step], color[p0:p0 + step], depth=depth[p0:p0 + step], first_pose=p0)
    bits = fc.seen
    Ah, Aw = P.nonrigid_lattice(H, W, S)
    cells, unknowns = (Ah - 1) * (Aw - 1), 6 + 2 * Ah * Aw
    flow = np.random.default_rng(0).uniform(-1.0, 1.0, (B, Ah, Aw, 2))
    flow_d = torch.from_numpy(flow).to(DEV)
    RT, valid = P.pose_extrinsics(poses)
    rt_d, valid_d = torch.from_numpy(RT).to(DEV), torch.from_numpy(valid).to(DEV)
    free = np.ones(B, dtype=bool)
    free_d = torch.from_numpy(free.astype(np.uint8)).to(DEV)
    images = torch.empty(B, H, W, 4, dtype=torch.int32, device=DEV)
    for p0 in range(0, B, step):
        P._colormap_gradients(color[p0:p0 + step], images[p0:p0 + step])
    # the blocks of one iteration, as optimize_poses_nonrigid forms them
    fc.sum.zero_()
    fc.count.zero_()
    for p0 in range(0, B, step):
        fc._add_extrinsics(rt_d[p0:p0 + step], valid_d[p0:p0 + step], color[p0:p0 + step], p0, bits=bits, flow=flow_d[p0:p0 + step], lattice_step=S)
    proxy = P._colormap_proxy(fc.sum, fc.count)
    blocks = torch.empty(B, cells, 120, dtype=torch.float64, device=DEV)
    counts = torch.empty(B, cells, dtype=torch.int32, device=DEV)
    keys = P._nonrigid_workspace(n, step, H, W, S, DEV)
    for p0 in range(0, B, step):
        P._nonrigid_normal(V, rt_d[p0:p0 + step], valid_d[p0:p0 + step], p0, images[p0:p0 + step], flow_d[p0:p0 + step], S, CAM, fc.z_near,
                           bits, MARGIN, proxy, blocks[p0:p0 + step], counts[p0:p0 + step], keys)
    lib = _lib.load()
    ws_bytes = lib.stin_nonrigid_solve_workspace_bytes(B, Ah, Aw)
    if ws_bytes == 0:
        raise SystemExit('a lattice of %d x %d anchors is outside what the banded solve supports' % (Ah, Aw))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    x = torch.empty(B, unknowns, dtype=torch.float64, device=DEV)
    residual = torch.empty(B, dtype=torch.float64, device=DEV)
    pairs = torch.empty(B, dtype=torch.int64, device=DEV)
    status = torch.empty(B, dtype=torch.int32, device=DEV)

    def stage(mask):
        _lib.check(lib.stin_nonrigid_solve_stages_f64(_ptr(blocks), _ptr(counts), _ptr(flow_d), _ptr(valid_d), _ptr(free_d), B, Ah, Aw, n,
                                                      ANCHOR_WEIGHT, MIN_PAIRS, _ptr(x), _ptr(residual), _ptr(pairs), _ptr(status), _ptr(ws),
                                                      ws_bytes, mask, _stream(blocks)), 'stin_nonrigid_solve_stages_f64')

    K = _lib.CONSTANTS
    arms = [('k_solve_stats', lambda: stage(K['STIN_NONRIGID_SOLVE_STAGE_STATS'])),
            ('k_solve_assemble', lambda: stage(K['STIN_NONRIGID_SOLVE_STAGE_ASSEMBLE'])),
            ('k_solve_factor', lambda: stage(K['STIN_NONRIGID_SOLVE_STAGE_FACTOR'])),
            ('stin_nonrigid_solve_f64 (all three)', lambda: stage(0))]
    if args.only == 'kernels':
        stage(0)
        torch.cuda.synchronize()
        return
    for _ in range(2):
        for _, fn in arms:
            fn()
    torch.cuda.synchronize()
    times = {w: [] for w, _ in arms}
    for _ in range(args.reps):
        for w, fn in arms:
            times[w].append(timed(fn))
    st = status.cpu().numpy()
    emit(f, what='scene', N=n, poses=B, H=H, W=W, batch=step, lattice_step=S, anchors=[Ah, Aw], cells=cells, unknowns=unknowns,
         half_bandwidth=2 * Aw + 3, pairs=int(pairs.sum().item()), solved=int((st == 0).sum()), singular=int((st == 8).sum()),
         few_pairs=int((st == 4).sum()), workspace_bytes=int(ws_bytes), lds_bytes=8 * ((2 * Aw + 4) * (2 * Aw + 11) + 42 + 2 * Aw + 10))
    for w, v in times.items():
        emit(f, what=w, ms_median=statistics.median(v), ms_min=min(v), ms_all=v)
    # ---- the read-backs
    back, back_all = wall(lambda: (x.cpu(), residual.cpu(), pairs.cpu(), status.cpu()))
    emit(f, what='read-back of x, residual, pairs, status', ms_median=back, ms_all=back_all, bytes=int(x.numel()) * 8 + B * 20)
    back, back_all = wall(lambda: (blocks.cpu(), counts.cpu()))
    emit(f, what='read-back of blocks and counts (dense)', ms_median=back, ms_all=back_all, bytes=int(blocks.numel()) * 8 + int(counts.numel()) * 4)
    # ---- the host solve on the same blocks, and the quality of the device's x against LAPACK's
    blk, k, xs = blocks.cpu().numpy(), counts.cpu().numpy(), x.cpu().numpy()
    E = np.zeros((B, 4, 4))
    E[:, :3, :], E[:, 3, 3] = RT.reshape(B, 3, 4), 1.0

    def host():
        s = np.zeros(B, dtype=np.int32)
        assert P.nonrigid_update(E.copy(), flow.copy(), valid, free, blk, k, n, ANCHOR_WEIGHT, MIN_PAIRS, s).any()
    upd, upd_all = wall(host)
    emit(f, what='nonrigid_update on the host, all poses (dense)', ms_median=upd, ms_all=upd_all, per_pose_ms=upd / B)
    import _nonrigid_solve_oracle as SO
    for p in [q for q in range(B) if st[q] == 0][:4]:
        A, b = SO.system(blk[p], flow[p], int(k[p].sum()), n, ANCHOR_WEIGHT)
        emit(f, what='scaled residual', pose=p, banded=scaled_residual(A, b, xs[p]), lapack=scaled_residual(A, b, np.linalg.solve(A, -b)),
             max_abs_difference=float(np.abs(xs[p] - np.linalg.solve(A, -b)).max()), max_abs_x=float(np.abs(xs[p]).max()))
    # ---- one iteration end to end, the two solvers alternating
    def run(solver, it):
        return P.optimize_poses_nonrigid(V, poses, color, bits=bits, color_camera=CAM, margin=MARGIN, iterations=it, lattice_step=S,
                                         batch=step, solver=solver)
    walls = {}
    for iters in (0, args.iterations):
        for solver in P.NONRIGID_SOLVERS:
            walls[solver, iters], ts = wall(lambda: run(solver, iters), reps=2)
            emit(f, what='optimize_poses_nonrigid, wall clock', solver=solver, iterations=iters, ms_median=walls[solver, iters], ms_all=ts)
    per = {s: (walls[s, args.iterations] - walls[s, 0]) / args.iterations for s in P.NONRIGID_SOLVERS}
    emit(f, what='one iteration, wall clock', dense_ms=per['dense'], banded_ms=per['banded'], dense_over_banded=per['dense'] / per['banded'])


if __name__ == '__main__':
    main()
