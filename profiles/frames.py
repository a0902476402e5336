"""Timing of the frame-colour path (csrc/stin_frames.hip, preprocessing.FrameColors) on one GPU.

    python profiles/frames.py [--out FILE] [--side 448] [--frames 64] [--reps 9]

Scene: tests/_levels_oracle.grid_mesh(side, 1, spacing=0.02) - 200 704 vertices at side 448, the benchmark's mesh size - under
`frames` cameras that walk 1.6 m above the surface looking ahead and down, at ScanNet's sizes: depth 480 x 640, colour 968 x 1296.
The depth frames are the analytic height field of grid_mesh (Newton on the ray parameter, in torch on the device: scene set-up, no
kernel of the path) in millimetres; the colour frames are random bytes.
* each entry point between two device events, median / min / max of `reps` calls after a warm-up: stin_frames_depth_edges_u16,
  stin_frames_accumulate_f64 in depth mode and in observer-bits mode (bits from observe_vertices at S = 256), each on the owner
  route and on the split route, and stin_frames_finish_f32; FrameColors.add as a whole (host inversion of the poses, uploads, both
  kernels);
* the accumulate pass at N / 4 and N / 16 vertices, where the host rule splits the poses further;
* us per pose, the time of a 2 000-frame scan extrapolated from it, and the accumulate pass's byte bound: N 24 bytes of vertices
  and N 28 bytes of sums per batch plus the frames read once, over the measured HBM copy rate;
* the share of (vertex, pose) pairs that are coloured (from the counts: a statistic).
Never reads the reference.  Prints one JSON line per measurement."""
import argparse
import ctypes
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
from surface_texture_inpainting_net_amd.plan import _ptr, _stream  # noqa: E402

DEV = 'cuda:0'
DEPTH_CAM = (577.87, 577.87, 319.5, 239.5)                 # ScanNet's depth camera, 480 x 640
COLOR_CAM = (1170.19, 1165.37, 647.5, 483.5)               # and its colour camera, 968 x 1296
HD, WD, HC, WC = 480, 640, 968, 1296
HBM_COPY_TBS = 6.29                                        # measured float4 copy rate of the MI355X (8.0 TB/s spec)


def emit(f, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if f is not None:
        f.write(line + '\n')
        f.flush()


def timed(fn, reps, warm=2):
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


def walk_poses(V, n):
    lo, hi, c = V.min(axis=0), V.max(axis=0), V.mean(axis=0)
    t = np.linspace(0.0, 1.0, n + 1)
    path = np.stack([lo[0] + (0.1 + 0.8 * t) * (hi[0] - lo[0]), c[1] + 0.3 * (hi[1] - lo[1]) * np.sin(2 * np.pi * t), np.full_like(t, 1.6)], 1)
    return np.stack([OO.look_at(path[i], path[i] + (path[i + 1] - path[i]) / np.linalg.norm(path[i + 1] - path[i]) + [0, 0, -1.5])
                     for i in range(n)])


def render_height_field(poses, lo, hi):
    """uint16 millimetres [P, HD, WD] on the device: z-depth of z = 0.4 sin(1.3 x) cos(0.9 y) over [lo, hi], 0 elsewhere."""
    fx, fy, cx, cy = DEPTH_CAM
    ii, jj = torch.meshgrid(torch.arange(HD, dtype=torch.float64, device=DEV), torch.arange(WD, dtype=torch.float64, device=DEV), indexing='ij')
    D = torch.stack([(jj - cx) / fx, (ii - cy) / fy, torch.ones_like(ii)], dim=2).reshape(-1, 3)
    out = torch.zeros(len(poses), HD * WD, dtype=torch.int32, device=DEV)
    for p, pose in enumerate(poses):
        R, e = torch.from_numpy(pose[:3, :3].copy()).to(DEV), pose[:3, 3]
        d = D @ R.T
        t = torch.full((D.shape[0],), float(e[2]), dtype=torch.float64, device=DEV) / (-d[:, 2]).clamp(min=0.2)
        for _ in range(8):
            x, y = e[0] + t * d[:, 0], e[1] + t * d[:, 1]
            sx, cx_, sy, cy_ = torch.sin(1.3 * x), torch.cos(1.3 * x), torch.sin(0.9 * y), torch.cos(0.9 * y)
            g = e[2] + t * d[:, 2] - 0.4 * sx * cy_
            t = t - g / (d[:, 2] - 0.4 * (1.3 * cx_ * cy_ * d[:, 0] - 0.9 * sx * sy * d[:, 1]))
        x, y = e[0] + t * d[:, 0], e[1] + t * d[:, 1]
        mm = torch.round(t * 1000.0)
        ok = (x >= lo[0]) & (x <= hi[0]) & (y >= lo[1]) & (y <= hi[1]) & (g.abs() < 1e-6) & (mm > 0) & (mm < 65535)
        out[p] = torch.where(ok, mm, torch.zeros_like(mm)).to(torch.int32)
    return torch.from_numpy(out.reshape(len(poses), HD, WD).cpu().numpy().astype(np.uint16)).to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--side', type=int, default=448)          # 448^2 = 200 704 vertices
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--reps', type=int, default=9)
    args = ap.parse_args()
    out = open(args.out, 'a') if args.out else None
    lib, C = _lib.load(), _lib.CONSTANTS
    mesh = LO.grid_mesh(args.side, 1, spacing=0.02)
    V, F = mesh['vertices'], mesh['faces']
    N, B = V.shape[0], args.frames
    poses = walk_poses(V, B)
    v, f = torch.from_numpy(V).to(DEV), torch.from_numpy(F).to(DEV)
    depth = render_height_field(poses, V.min(axis=0), V.max(axis=0))
    color = torch.randint(0, 256, (B, HC, WC, 3), dtype=torch.uint8, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    emit(out, what='scene', vertices=N, frames=B, depth_size=[HD, WD], color_size=[HC, WC], depth_pixels_measured=float(np.count_nonzero(depth.cpu().numpy())) / depth.numel())
    fc = P.FrameColors(v, COLOR_CAM, DEPTH_CAM)
    # ---- the edge pass
    t = timed(lambda: fc.depth_edges(depth), args.reps)
    emit(out, what='stin_frames_depth_edges_u16', frames=B, us_per_pose=t['ms_median'] / B * 1e3, s_per_2000_poses=t['ms_median'] / B * 2.0,
         bytes_per_pose=HD * WD * (2 + 1 + 1 + 1), ms_at_hbm_copy_rate=B * HD * WD * 5 / (HBM_COPY_TBS * 1e12) * 1e3, **t)
    edge = fc.depth_edges(depth)
    emit(out, what='edge share', share=float(edge.float().mean()))
    # ---- the accumulate pass, entry point alone
    RT, valid = P.pose_extrinsics(poses)
    rt_d, valid_d = torch.from_numpy(RT).to(DEV), torch.from_numpy(valid).to(DEV)
    bits, _ = P.observe_vertices(v, f, poses, fx=COLOR_CAM[0], fy=COLOR_CAM[1], width=WC, height=HC, image_size=256)
    cameras = (ctypes.c_double * 8)(*(COLOR_CAM + DEPTH_CAM))
    params = (ctypes.c_double * 5)(1000.0, 3.0, 2.5, 0.03, 0.01)
    words = int(bits.shape[1])
    v64 = v.contiguous()

    def accumulate(n, mode, route, total, count):
        d, e, bt = (depth, edge, None) if mode == 'depth' else (None, None, bits)
        _lib.check(lib.stin_frames_accumulate_f64(_ptr(v64), n, _ptr(rt_d), _ptr(valid_d), B, 0, _ptr(color), HC, WC, _ptr(d), _ptr(e), HD, WD,
                                                  cameras, params, _ptr(bt), words, 10, route, _ptr(total), _ptr(count), None, 0,
                                                  _stream(v64)), 'stin_frames_accumulate_f64')

    routes = (('auto', C['STIN_FRAMES_ROUTE_AUTO']), ('owner', C['STIN_FRAMES_ROUTE_OWNER']), ('split', C['STIN_FRAMES_ROUTE_SPLIT']))
    frame_bytes = B * (HD * WD * 3 + HC * WC * 3)
    for n in (N, N // 4, N // 16):
        for mode in ('depth', 'bits'):
            results = {}
            for name, route in routes:
                total = torch.zeros(N, 3, dtype=torch.int64, device=DEV)
                count = torch.zeros(N, dtype=torch.int32, device=DEV)
                t = timed(lambda: accumulate(n, mode, route, total, count), args.reps)
                calls = args.reps + 2
                total.zero_(), count.zero_()
                accumulate(n, mode, route, total, count)
                results[name] = (total.clone(), count.clone())
                bound = (n * 52 + (frame_bytes if mode == 'depth' else B * HC * WC * 3 + n * words * 4)) / (HBM_COPY_TBS * 1e12) * 1e3
                emit(out, what='stin_frames_accumulate_f64', vertices=n, mode=mode, route=name, calls_timed=calls,
                     us_per_pose=t['ms_median'] / B * 1e3, s_per_2000_poses=t['ms_median'] / B * 2.0, ms_byte_bound=bound,
                     times_the_bound=t['ms_median'] / bound, pairs_coloured_share=float(count[:n].double().mean()) / B, **t)
            assert all(torch.equal(results['auto'][k], results[r][k]) for r in ('owner', 'split') for k in (0, 1)), 'routes disagree'
    # ---- finish, and add() as a whole
    total = torch.zeros(N, 3, dtype=torch.int64, device=DEV)
    count = torch.zeros(N, dtype=torch.int32, device=DEV)
    accumulate(N, 'depth', 0, total, count)
    colors = torch.empty(N, 3, dtype=torch.float32, device=DEV)
    t = timed(lambda: _lib.check(lib.stin_frames_finish_f32(_ptr(total), _ptr(count), N, 0.0, 0.0, 0.0, _ptr(colors), None, _stream(v64)),
                                 'stin_frames_finish_f32'), args.reps)
    emit(out, what='stin_frames_finish_f32', vertices=N, **t)
    emit(out, what='result', vertices_coloured=int((count > 0).sum()), mean_frames_per_vertex=float(count.double().mean()))
    t = timed(lambda: P.FrameColors(v, COLOR_CAM, DEPTH_CAM).add(poses, color, depth=depth), args.reps)
    emit(out, what='FrameColors + add (depth mode, host work included)', frames=B, us_per_pose=t['ms_median'] / B * 1e3,
         s_per_2000_poses=t['ms_median'] / B * 2.0, **t)
    t = timed(lambda: P.FrameColors(v, COLOR_CAM).add(poses, color, bits=bits), args.reps)
    emit(out, what='FrameColors + add (bits mode, host work included)', frames=B, us_per_pose=t['ms_median'] / B * 1e3,
         s_per_2000_poses=t['ms_median'] / B * 2.0, **t)


if __name__ == '__main__':
    main()
