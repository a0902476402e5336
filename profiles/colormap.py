"""Timing of the rigid colour-map optimisation (csrc/stin_colormap.hip, preprocessing.optimize_poses_rigid) on one GPU, with the
parent's stin_frames_accumulate_f64 in bits mode on the same pairs in the same run as the yardstick.

    python profiles/colormap.py [--out FILE] [--side 448] [--poses 128] [--reps 7] [--iterations 3] [--only kernels]

Scene: tests/_levels_oracle.grid_mesh(side, 1, spacing=0.02) - 200 704 vertices at side 448, the benchmark's mesh size, vertex ids in
random order - with smooth vertex colours, under `poses` cameras walking over it at 1.6 m (profiles/frames.py's walk); the colour and
depth frames are views.render_mesh's, 480 x 640, so that they are consistent with the mesh.  The visibility bits are the `seen` of
one FrameColors pass in depth mode, as optimize_poses_rigid establishes them.

* every kernel alone - gradients (all frames), accumulate in bits mode (the yardstick), proxy, normal - HIP events around one call on
  buffers allocated beforehand, no host read inside, two warm-up calls, the median of `reps` calls; the arms alternate inside every
  repetition.
* beside the normal kernel's time: the pairs, the fp64 vector-ALU bound - pairs x OPS_PER_PAIR operations over CUs x 64 lanes x the
  clock the device reports (the count is of the contract's operations, see OPS_PER_PAIR) - and the bytes a pair gathers (four taps
  of 16 bytes).
* one iteration end to end (accumulate, proxy, normal, the read-back of P x 29 numbers and the host update): wall clock of
  optimize_poses_rigid with `iterations` and with 0 iterations, the difference divided by `iterations`.
* --only kernels: one call of each kernel, for a `rocprofv3 --kernel-trace --stats` run.
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

import _levels_oracle as LO  # noqa: E402
import _observers_oracle as OO  # noqa: E402
from surface_texture_inpainting_net_amd import _lib, preprocessing as P, views  # noqa: E402

DEV = 'cuda:0'
H, W = 480, 640
CAM = (577.87, 577.87, W / 2 - 0.5, H / 2 - 0.5)
MARGIN = 10
# fp64 operations of one contributing pair, as the contract writes them: view 18, projection 6, floor / weights 10, three samples
# 3 x 11, three divisions, r, iz, v0 v1 v2 9, J 9, the 28 products and 28 additions.  Divisions count as one.
OPS_PER_PAIR = 18 + 6 + 10 + 33 + 3 + 1 + 1 + 9 + 9 + 56
BYTES_PER_PAIR = 4 * 16


def emit(f, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if f is not None:
        f.write(line + '\n')
        f.flush()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def walk_poses(V, n):
    lo, hi, c = V.min(axis=0), V.max(axis=0), V.mean(axis=0)
    t = np.linspace(0.0, 1.0, n + 1)
    path = np.stack([lo[0] + (0.1 + 0.8 * t) * (hi[0] - lo[0]), c[1] + 0.3 * (hi[1] - lo[1]) * np.sin(2 * np.pi * t), np.full_like(t, 1.6)], 1)
    return np.stack([OO.look_at(path[i], path[i] + (path[i + 1] - path[i]) / np.linalg.norm(path[i + 1] - path[i]) + [0, 0, -1.5])
                     for i in range(n)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--side', type=int, default=448)            # 448^2 = 200 704 vertices
    ap.add_argument('--poses', type=int, default=128)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--iterations', type=int, default=3)
    ap.add_argument('--only', default=None, choices=[None, 'kernels'])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('profiles/colormap.py measures on a GPU; none is visible (nothing is timed on the CPU)')
    f = open(args.out, 'a') if args.out else None
    props = torch.cuda.get_device_properties(0)
    cus, ghz = int(props.multi_processor_count), float(getattr(props, 'clock_rate', 2400000)) / 1e6
    rate = cus * 64 * ghz * 1e9                                          # fp64 vector operations per second, non-FMA
    emit(f, what='device', name=props.name, cus=cus, clock_ghz=ghz, fp64_vector_ops_per_s=rate, lib=_lib.LIB_PATH,
         U=_lib.CONSTANTS['STIN_COLORMAP_U'])
    mesh = LO.grid_mesh(args.side, 1, spacing=0.02)
    Vn = mesh['vertices']
    n, B, step = int(Vn.shape[0]), args.poses, args.batch
    C = np.stack([0.5 + 0.45 * np.sin(3.1 * Vn[:, 0]) * np.cos(2.3 * Vn[:, 1]), 0.5 + 0.45 * np.cos(2.7 * Vn[:, 0] + 0.5),
                  0.5 + 0.45 * np.sin(1.9 * Vn[:, 0] + 2.9 * Vn[:, 1])], axis=1).astype(np.float32)
    poses = walk_poses(Vn, B)
    V, F = torch.from_numpy(Vn).to(DEV), torch.from_numpy(mesh['faces']).to(DEV)
    r = views.render_mesh(V, F, torch.from_numpy(C).to(DEV), poses, CAM, H, W, depth=True)
    color, depth = r.color.contiguous(), r.depth.contiguous()
    fc = P.FrameColors(V, CAM, margin=MARGIN, num_poses=B)
    for p0 in range(0, B, step):
        fc.add(poses[p0:p0 + step], color[p0:p0 + step], depth=depth[p0:p0 + step], first_pose=p0)
    bits, pairs = fc.seen, int(fc.count.sum().item())
    RT, valid = P.pose_extrinsics(poses)
    rt_d, valid_d = torch.from_numpy(RT).to(DEV), torch.from_numpy(valid).to(DEV)
    images = torch.empty(B, H, W, 4, dtype=torch.int32, device=DEV)
    proxy = torch.empty(n, dtype=torch.float64, device=DEV)
    rows = torch.empty(B, 28, dtype=torch.float64, device=DEV)
    counts = torch.empty(B, dtype=torch.int32, device=DEV)
    ws = P._colormap_workspace(n, step, DEV)
    emit(f, what='scene', N=n, poses=B, H=H, W=W, batch=step, pairs=pairs, pairs_per_pose=pairs / B,
         visible_fraction=pairs / (n * B), image_bytes=int(images.numel()) * 4, workspace_bytes=int(ws.numel()))

    def gradients():
        for p0 in range(0, B, step):
            P._colormap_gradients(color[p0:p0 + step], images[p0:p0 + step])

    def accumulate():
        fc.sum.zero_()
        fc.count.zero_()
        for p0 in range(0, B, step):
            fc._add_extrinsics(rt_d[p0:p0 + step], valid_d[p0:p0 + step], color[p0:p0 + step], p0, bits=bits)

    def make_proxy():
        P._colormap_proxy(fc.sum, fc.count, proxy)

    def normal():
        for p0 in range(0, B, step):
            P._colormap_normal(V, rt_d[p0:p0 + step], valid_d[p0:p0 + step], p0, images[p0:p0 + step], CAM, fc.z_near, bits, MARGIN, proxy,
                               rows[p0:p0 + step], counts[p0:p0 + step], ws)

    arms = [('stin_colormap_gradients_u8', gradients), ('stin_frames_accumulate_f64 (bits mode)', accumulate),
            ('stin_colormap_proxy_f64', make_proxy), ('stin_colormap_normal_f64', normal)]
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
    assert int(counts.sum().item()) == pairs, (int(counts.sum().item()), pairs)
    med = {w: statistics.median(v) for w, v in times.items()}
    bound_ms = pairs * OPS_PER_PAIR / rate * 1e3
    for w, v in times.items():
        extra = {}
        if w == 'stin_colormap_normal_f64':
            extra = dict(pairs=pairs, ops_per_pair=OPS_PER_PAIR, valu_bound_ms=bound_ms, achieved_fraction=bound_ms / med[w],
                         bytes_per_pair=BYTES_PER_PAIR, gathered_gb_per_s=pairs * BYTES_PER_PAIR / med[w] / 1e6,
                         ratio_to_accumulate=med[w] / med['stin_frames_accumulate_f64 (bits mode)'], residual=float(rows[:, 27].sum().item()))
        if w == 'stin_colormap_gradients_u8':
            extra = dict(bytes_moved=B * H * W * 19, gb_per_s=B * H * W * 19 / med[w] / 1e6)
        emit(f, what=w, ms_median=med[w], ms_min=min(v), ms_all=v, **extra)
    # ---- one iteration end to end: the read-back and the host update included
    walls = {}
    for iters in (0, args.iterations):
        ts = []
        for i in range(1 + 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            P.optimize_poses_rigid(V, poses, color, bits=bits, color_camera=CAM, margin=MARGIN, iterations=iters, batch=step)
            torch.cuda.synchronize()
            if i >= 1:
                ts.append((time.perf_counter() - t0) * 1e3)
        walls[iters] = statistics.median(ts)
        emit(f, what='optimize_poses_rigid, wall clock', iterations=iters, ms_median=walls[iters], ms_all=ts)
    emit(f, what='one iteration, wall clock', ms=(walls[args.iterations] - walls[0]) / args.iterations,
         kernels_ms=med['stin_frames_accumulate_f64 (bits mode)'] + med['stin_colormap_proxy_f64'] + med['stin_colormap_normal_f64'])


if __name__ == '__main__':
    main()
