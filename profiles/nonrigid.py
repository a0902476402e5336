"""Timing of the non-rigid colour-map optimisation (csrc/stin_nonrigid.hip, preprocessing.optimize_poses_nonrigid) on one GPU, with
the rigid optimiser's normal-equation kernels (stin_colormap_normal_f64) on the same scene in the same run as the figure to set it
beside.

    python profiles/nonrigid.py [--out FILE] [--side 448] [--poses 128] [--batch 64] [--lattice-step 32] [--reps 7]
                                [--iterations 2] [--only kernels]

Scene: profiles/colormap.py's - tests/_levels_oracle.grid_mesh(side, 1, spacing=0.02), 200 704 vertices at side 448 with ids in
random order, smooth vertex colours, `poses` cameras walking over it at 1.6 m, 480 x 640 frames from views.render_mesh, the
visibility bits of one FrameColors pass in depth mode.  The flow is random within one pixel (a zero flow would warp nothing; the
time does not depend on its values).

* every stage of an iteration alone - the warped accumulate, the proxy, the keys, the sort (torch.sort: rocPRIM), the blocks - and,
  for comparison, the unwarped accumulate and the rigid normal equations: HIP events around one call on buffers allocated
  beforehand, no host read inside, two warm-up calls, the median of `reps` calls; the arms alternate inside every repetition.
* beside the block kernel's time its byte term: pairs x the bytes a pair reads (key 8, vertex 24, proxy 8, four anchors 64, four
  taps of 16) plus the blocks and counts written, over the HBM rate.
* the read-back of the blocks and counts (time.perf_counter around a synchronised copy) and the host update of all poses
  (nonrigid_update, wall clock).
* one iteration end to end: wall clock of optimize_poses_nonrigid with `iterations` and with 0 iterations, the difference divided by
  `iterations`; the same for optimize_poses_rigid.
* --only kernels: one call of each stage, for a `rocprofv3 --kernel-trace --stats` run.
Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'profiles'))

import _levels_oracle as LO  # noqa: E402
from colormap import CAM, DEV, H, MARGIN, W, emit, timed, walk_poses  # noqa: E402
from surface_texture_inpainting_net_amd import _lib, preprocessing as P, views  # noqa: E402

BYTES_PER_PAIR = 8 + 24 + 8 + 4 * 16 + 4 * 16
HBM_BYTES_PER_S = 8.0e12                                                 # MI355X: 8 TB/s


def wall(fn, reps=3):
    ts = []
    for i in range(1 + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= 1:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


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
        raise SystemExit('profiles/nonrigid.py measures on a GPU; none is visible (nothing is timed on the CPU)')
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
    cells = (Ah - 1) * (Aw - 1)
    flow = np.random.default_rng(0).uniform(-1.0, 1.0, (B, Ah, Aw, 2))
    flow_d = torch.from_numpy(flow).to(DEV)
    RT, valid = P.pose_extrinsics(poses)
    rt_d, valid_d = torch.from_numpy(RT).to(DEV), torch.from_numpy(valid).to(DEV)
    images = torch.empty(B, H, W, 4, dtype=torch.int32, device=DEV)
    for p0 in range(0, B, step):
        P._colormap_gradients(color[p0:p0 + step], images[p0:p0 + step])
    proxy = torch.empty(n, dtype=torch.float64, device=DEV)
    rows = torch.empty(B, 28, dtype=torch.float64, device=DEV)
    row_counts = torch.empty(B, dtype=torch.int32, device=DEV)
    ws = P._colormap_workspace(n, step, DEV)
    blocks = torch.empty(B, cells, 120, dtype=torch.float64, device=DEV)
    counts = torch.empty(B, cells, dtype=torch.int32, device=DEV)
    batches = list(range(0, B, step))
    keys = [P._nonrigid_workspace(n, step, H, W, S, DEV) for _ in batches]            # one buffer per batch: the stages are timed apart
    made, ordered = [None] * len(batches), [None] * len(batches)

    def accumulate(warped):
        fc.sum.zero_()
        fc.count.zero_()
        for p0 in batches:
            fc._add_extrinsics(rt_d[p0:p0 + step], valid_d[p0:p0 + step], color[p0:p0 + step], p0, bits=bits,
                               flow=flow_d[p0:p0 + step] if warped else None, lattice_step=S)

    def make_proxy():
        P._colormap_proxy(fc.sum, fc.count, proxy)

    def make_keys():
        for i, p0 in enumerate(batches):
            made[i] = P._nonrigid_keys(V, rt_d[p0:p0 + step], valid_d[p0:p0 + step], p0, H, W, flow_d[p0:p0 + step], S, CAM, fc.z_near, bits,
                                       MARGIN, keys[i])

    def sort():
        for i in range(len(batches)):
            ordered[i] = torch.sort(made[i])[0]

    def make_blocks():
        for i, p0 in enumerate(batches):
            P._nonrigid_blocks(V, rt_d[p0:p0 + step], valid_d[p0:p0 + step], p0, images[p0:p0 + step], flow_d[p0:p0 + step], S, CAM,
                               fc.z_near, MARGIN, proxy, ordered[i], blocks[p0:p0 + step], counts[p0:p0 + step])

    def rigid_normal():
        for p0 in batches:
            P._colormap_normal(V, rt_d[p0:p0 + step], valid_d[p0:p0 + step], p0, images[p0:p0 + step], CAM, fc.z_near, bits, MARGIN, proxy,
                               rows[p0:p0 + step], row_counts[p0:p0 + step], ws)

    arms = [('stin_frames_accumulate_f64 (bits mode, unwarped)', lambda: accumulate(False)),
            ('stin_nonrigid_accumulate_f64', lambda: accumulate(True)), ('stin_colormap_proxy_f64', make_proxy),
            ('stin_nonrigid_keys_f64', make_keys), ('torch.sort of the keys', sort), ('stin_nonrigid_normal_f64 (blocks)', make_blocks),
            ('stin_colormap_normal_f64 (rigid, same scene)', rigid_normal)]
    if args.only == 'kernels':
        for _, fn in arms:
            fn()
        torch.cuda.synchronize()
        return
    for _ in range(2):
        for _, fn in arms:
            fn()
    torch.cuda.synchronize()
    times = {w: [] for w, _ in arms}
    for _ in range(args.reps):                                           # alternate: drift hits every arm alike
        for w, fn in arms:
            times[w].append(timed(fn))
    pairs = int(counts.sum().item())
    emit(f, what='scene', N=n, poses=B, H=H, W=W, batch=step, lattice_step=S, anchors=[Ah, Aw], cells=cells, unknowns=6 + 2 * Ah * Aw,
         pairs=pairs, rigid_pairs=int(row_counts.sum().item()), pairs_per_cell=pairs / (B * cells), most_pairs_in_a_cell=int(counts.max().item()),
         empty_cells=int((counts == 0).sum().item()), key_bytes=n * step * 8, block_bytes=int(blocks.numel()) * 8)
    med = {w: statistics.median(v) for w, v in times.items()}
    for w, v in times.items():
        extra = {}
        if w.startswith('stin_nonrigid_normal_f64'):
            moved = pairs * BYTES_PER_PAIR + int(blocks.numel()) * 8 + int(counts.numel()) * 4
            extra = dict(pairs=pairs, bytes_per_pair=BYTES_PER_PAIR, bytes=moved, byte_term_ms=moved / HBM_BYTES_PER_S * 1e3,
                         times_the_byte_term=med[w] / (moved / HBM_BYTES_PER_S * 1e3),
                         ratio_to_rigid_normal=med[w] / med['stin_colormap_normal_f64 (rigid, same scene)'])
        if w.startswith('torch.sort'):
            extra = dict(keys=n * B, gkeys_per_s=n * B / med[w] / 1e6)
        emit(f, what=w, ms_median=med[w], ms_min=min(v), ms_all=v, **extra)
    kernels = sum(med[w] for w, _ in arms[1:6])
    emit(f, what='kernels of one iteration', ms=kernels, rigid_ms=med[arms[0][0]] + med[arms[2][0]] + med[arms[6][0]])
    # ---- the read-back and the host update
    back, back_all = wall(lambda: (blocks.cpu(), counts.cpu()))
    emit(f, what='read-back of blocks and counts', ms_median=back, ms_all=back_all, bytes=int(blocks.numel()) * 8 + int(counts.numel()) * 4)
    blk, k = blocks.cpu().numpy(), counts.cpu().numpy()
    E = np.zeros((B, 4, 4))
    E[:, :3, :], E[:, 3, 3] = RT.reshape(B, 3, 4), 1.0
    free = np.ones(B, dtype=bool)

    def host():
        status = np.zeros(B, dtype=np.int32)
        moved = P.nonrigid_update(E.copy(), flow.copy(), valid, free, blk, k, n, 0.316, 16, status)
        assert moved.any()
    upd, upd_all = wall(host)
    emit(f, what='nonrigid_update on the host, all poses', ms_median=upd, ms_all=upd_all, per_pose_ms=upd / B, unknowns=6 + 2 * Ah * Aw)
    # ---- one iteration end to end
    for name, fn in (('optimize_poses_nonrigid', lambda it: P.optimize_poses_nonrigid(V, poses, color, bits=bits, color_camera=CAM, margin=MARGIN,
                                                                                       iterations=it, lattice_step=S, batch=step)),
                     ('optimize_poses_rigid', lambda it: P.optimize_poses_rigid(V, poses, color, bits=bits, color_camera=CAM, margin=MARGIN,
                                                                                 iterations=it, batch=step))):
        walls = {}
        for iters in (0, args.iterations):
            walls[iters], ts = wall(lambda: fn(iters), reps=2)
            emit(f, what='%s, wall clock' % name, iterations=iters, ms_median=walls[iters], ms_all=ts)
        emit(f, what='%s: one iteration, wall clock' % name, ms=(walls[args.iterations] - walls[0]) / args.iterations)


if __name__ == '__main__':
    main()
