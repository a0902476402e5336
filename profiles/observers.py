"""Timing of the observer-mask path (csrc/stin_observe.hip on csrc/stin_raster.hip, preprocessing.observe_vertices / observer_masks) on one GPU.

    python profiles/observers.py [--out FILE] [--side 390] [--poses 256] [--reps 5] [--trace-only]

Scene: tests/_levels_oracle.grid_mesh(side, 1, spacing=0.02) - 152 100 vertices and 302 642 faces at side 390, the size of a ScanNet
scan - seen at S = 256 through ScanNet's colour camera from `poses` poses: one half on an orbit above the scene looking at its
middle, the other half a walk-through 1.2 m above the surface looking ahead and slightly down.
* stages, each between two device events (median / min / max of `reps` after a warm-up call): pose_extrinsics + uploads (host),
  observe_vertices, observer_masks for 8 masks, observer_counts;
* observe_vertices by batch size, and ms per pose = its time / poses, x 2 000 poses as the scan-level estimate, beside the bound of
  DESIGN.md's count (bytes per pose over the measured HBM copy rate);
* the share of (face, pose) pairs that survive the cull tests and the share whose clamped box exceeds the threshold (computed
  with torch from the contract's formulas: a statistic, no kernel of the path);
* 16 close-up poses 0.3 m above the surface looking straight at it: observe_vertices with the large-face kernel at thresholds
  16 .. 4096 and with a threshold no box can exceed (the per-lane loop alone), alternating - the pair that justifies the
  threshold - and that the bits agree.
--trace-only: 3 calls of the 256-pose set and 3 of the close-up set and nothing else, for a `rocprofv3 --kernel-trace --stats` run
of its own (per-kernel times: k_raster_clear / k_raster_transform / k_raster / k_raster_large / k_observe_resolve).  Never reads the reference.
Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _levels_oracle as LO  # noqa: E402
import _observers_oracle as OO  # noqa: E402
from surface_texture_inpainting_net_amd import _lib, preprocessing as P  # noqa: E402

DEV = 'cuda:0'
CAM = dict(fx=1170.19, fy=1165.37, width=1296, height=968)
S = 256
THRESHOLDS = (16, 32, 64, 128, 256, 1024, 4096)
HBM_COPY_TBS = 6.29                                        # measured float4 copy rate of the MI355X (8.0 TB/s spec)


def emit(f, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if f is not None:
        f.write(line + '\n')
        f.flush()


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return dict(ms_median=statistics.median(ts), ms_min=min(ts), ms_max=max(ts))


def scene_poses(V, n):
    c, lo, hi = V.mean(axis=0), V.min(axis=0), V.max(axis=0)
    half = n // 2
    orbit = OO.orbit(half, 0.45 * (hi[0] - lo[0]), 2.0, target=c)
    t = np.linspace(0.0, 1.0, n - half + 1)
    path = np.stack([lo[0] + (0.1 + 0.8 * t) * (hi[0] - lo[0]), c[1] + 0.3 * (hi[1] - lo[1]) * np.sin(2 * np.pi * t), np.full_like(t, 1.2)], 1)
    walk = np.stack([OO.look_at(path[i], path[i] + (path[i + 1] - path[i]) / np.linalg.norm(path[i + 1] - path[i]) + [0, 0, -0.4])
                     for i in range(n - half)])
    return np.concatenate([orbit, walk])


def closeup_poses(V, n):
    rng = np.random.default_rng(3)
    lo, hi = V.min(axis=0), V.max(axis=0)
    xy = lo[:2] + (0.2 + 0.6 * rng.uniform(size=(n, 2))) * (hi[:2] - lo[:2])
    z = 0.4 * np.sin(xy[:, 0] * 1.3) * np.cos(xy[:, 1] * 0.9)              # the height field of grid_mesh
    return np.stack([OO.look_at((x, y, h + 0.3), (x, y, h)) for (x, y), h in zip(xy, z)])


def box_statistics(v, f, poses, threshold):
    """(pairs, pairs surviving the cull tests, pairs with a box above the threshold), from the contract's formulas in torch."""
    RT, valid = P.pose_extrinsics(poses)
    sx, sy = 2 * CAM['fx'] / CAM['width'], 2 * CAM['fy'] / CAM['height']
    kept = large = 0
    for p in np.flatnonzero(valid):
        m = torch.from_numpy(RT[p]).to(DEV)
        x, y, z = v[:, 0], v[:, 1], v[:, 2]
        xv, yv, zv = (((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3] for r in range(3))
        X, Y = (sx * xv / zv + 1.0) * (0.5 * S) - 0.5, (sy * yv / zv + 1.0) * (0.5 * S) - 0.5
        Xf, Yf, Zf = X[f], Y[f], zv[f]
        ok = (Zf >= 0.01).all(1) & torch.isfinite(Xf).all(1) & torch.isfinite(Yf).all(1)
        x0, x1 = Xf.min(1).values.ceil().clamp(min=0), Xf.max(1).values.floor().clamp(max=S - 1)
        y0, y1 = Yf.min(1).values.ceil().clamp(min=0), Yf.max(1).values.floor().clamp(max=S - 1)
        ok &= (x0 <= x1) & (y0 <= y1)
        box = (x1 - x0 + 1) * (y1 - y0 + 1)
        kept += int(ok.sum())
        large += int((ok & (box > threshold)).sum())
    return int(f.shape[0]) * int(valid.sum()), kept, large


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--side', type=int, default=390)
    ap.add_argument('--poses', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--trace-only', action='store_true')
    args = ap.parse_args()
    out = open(args.out, 'a') if args.out else None
    _lib.load()
    threshold = _lib.CONSTANTS['STIN_OBSERVE_LARGE_BOX']
    mesh = LO.grid_mesh(args.side, 1, spacing=0.02)
    V, F = mesh['vertices'], mesh['faces']
    N, nf, n = V.shape[0], F.shape[0], args.poses
    poses, close = scene_poses(V, n), closeup_poses(V, 16)
    v, f = torch.from_numpy(V).to(DEV), torch.from_numpy(F).to(DEV)
    observe = lambda ps, **kw: P.observe_vertices(v, f, ps, image_size=S, **CAM, **kw)
    if args.trace_only:
        for _ in range(3):
            observe(poses)
        for _ in range(3):
            observe(close)
        torch.cuda.synchronize()
        return
    emit(out, what='scene', vertices=N, faces=nf, poses=n, image_size=S, large_box=threshold)
    # ---- stages
    emit(out, what='stage pose_extrinsics + uploads', **timed(lambda: (P.pose_extrinsics(poses), torch.from_numpy(V).to(DEV),
                                                                     torch.from_numpy(F).to(DEV)), args.reps))
    bits, ids = observe(poses)
    for batch in (64, 16, 256):
        t = timed(lambda: observe(poses, batch=batch), args.reps)
        emit(out, what='stage observe_vertices', batch=batch, ms_per_pose=t['ms_median'] / n, s_per_2000_poses=t['ms_median'] / n * 2.0, **t)
    emit(out, what='stage observer_masks', masks=8, **timed(lambda: P.observer_masks(bits, ids, n, num_masks=8), args.reps))
    emit(out, what='stage observer_counts', **timed(lambda: P.observer_counts(bits, n), args.reps))
    per_vertex, per_pose = P.observer_counts(bits, n)
    emit(out, what='result', vertices_observed=int((per_vertex > 0).sum()), mean_poses_per_vertex=float(per_vertex.double().mean()),
         mean_vertices_per_pose=float(per_pose.double().mean()))
    # ---- the bound of DESIGN.md's count, per pose
    bytes_pose = N * (24 + 24) + nf * (12 + 3 * 24) + S * S * 8 * 2
    emit(out, what='bound', bytes_per_pose=bytes_pose, transform=N * 48, cull=nf * 84, keys=S * S * 16,
         ms_per_pose_at_hbm_copy_rate=bytes_pose / (HBM_COPY_TBS * 1e12) * 1e3,
         s_per_2000_poses=bytes_pose / (HBM_COPY_TBS * 1e12) * 2000)
    pairs, kept, large = box_statistics(v, f, poses, threshold)
    emit(out, what='large-face share', poses='scene', pairs=pairs, kept=kept, large=large, share_of_kept=large / max(kept, 1),
         share_of_pairs=large / max(pairs, 1))
    pairs, kept, large = box_statistics(v, f, close, threshold)
    emit(out, what='large-face share', poses='close-up', pairs=pairs, kept=kept, large=large, share_of_kept=large / max(kept, 1),
         share_of_pairs=large / max(pairs, 1))
    # ---- close-up poses: the large-face kernel on (several thresholds) and off, alternating
    never = 1 << 40
    ref_bits, _ = observe(close, large_box=never)
    rows = {}
    for rep in range(args.reps + 1):
        for lb in (never,) + THRESHOLDS:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            got, _ = observe(close, large_box=lb)
            b.record()
            b.synchronize()
            if rep:                                                           # (round 0 is the warm-up)
                rows.setdefault(lb, []).append(a.elapsed_time(b))
            assert torch.equal(got.view(torch.int32), ref_bits.view(torch.int32))
    for lb, ts in rows.items():
        emit(out, what='close-up observe_vertices', poses=16, large_box='never' if lb == never else lb, ms_median=statistics.median(ts),
             ms_min=min(ts), ms_max=max(ts), ms_per_pose=statistics.median(ts) / 16)
    rows = {}
    for rep in range(args.reps + 1):
        for lb in (never,) + THRESHOLDS:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            got, _ = observe(poses, large_box=lb)
            b.record()
            b.synchronize()
            if rep:
                rows.setdefault(lb, []).append(a.elapsed_time(b))
            assert torch.equal(got.view(torch.int32), bits.view(torch.int32))
    for lb, ts in rows.items():
        emit(out, what='scene observe_vertices by threshold', poses=n, large_box='never' if lb == never else lb,
             ms_median=statistics.median(ts), ms_min=min(ts), ms_max=max(ts), ms_per_pose=statistics.median(ts) / n)


if __name__ == '__main__':
    main()
