"""Timing of the render path (csrc/stin_render.hip on csrc/stin_raster.hip, views.render_mesh) on one GPU.

    python profiles/render.py [--out FILE] [--side 448] [--poses 16] [--reps 9] [--trace-only [--trace-size 480x640]]

Scene: profiles/frames.py's - tests/_levels_oracle.grid_mesh(side, 1, spacing=0.02), 200 704 vertices at side 448, under cameras that
walk 1.6 m above the surface looking ahead and down - rendered with vertex colours at ScanNet's two frame sizes: 480 x 640 through
its depth camera and 968 x 1296 through its colour camera, `poses` poses in one batch.
* stages: stin_render_poses_f64 with the stage masks CLEAR, + TRANSFORM, + RASTER, + LARGE, + RESOLVE, each between two device
  events, median / min / max of `reps` calls after a warm-up; a stage's time is the DIFFERENCE of two neighbouring medians (a
  rasteriser cannot be timed alone: it needs cleared keys, or every atomic is skipped);
* the whole call by `large_box` (1 = every face through the wavefront route, 2^40 = every face on its own lane) - the sweep that
  chose STIN_RENDER_LARGE_BOX - and that the images agree;
* the resolve pass's byte bound: pixels x (8 key + 3 + 2 + 4, or 12 + 2 + 4 for float32 colour) over the measured copy rate;
* the yardstick: preprocessing.observe_vertices on the same scene and poses at S = 256, per pose, scaled by the pixel count;
* what the images hold: the share of covered pixels and the covered centres per visible face (from the face ids: a statistic).
--trace-only: 5 whole calls per size and nothing else, for a `rocprofv3 --kernel-trace --stats` run of its own (per-kernel times:
k_raster_clear / k_raster_transform / k_raster / k_raster_large / k_render_resolve) at --trace-size (480x640 or 968x1296).
Never reads the reference.  Prints one JSON line per measurement."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'profiles'))

import _levels_oracle as LO  # noqa: E402
from frames import COLOR_CAM, DEPTH_CAM, HBM_COPY_TBS, emit, timed, walk_poses  # noqa: E402
from surface_texture_inpainting_net_amd import _lib, preprocessing as P, views  # noqa: E402
from surface_texture_inpainting_net_amd.plan import _ptr, _stream  # noqa: E402

DEV = 'cuda:0'
SIZES = (('480x640', DEPTH_CAM, 480, 640), ('968x1296', COLOR_CAM, 968, 1296))
BOXES = (1, 4, 8, 16, 32, 64, 128, 256, 1024, 2 ** 40)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--side', type=int, default=448)          # 448^2 = 200 704 vertices
    ap.add_argument('--poses', type=int, default=16)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--trace-only', action='store_true')
    ap.add_argument('--trace-size', default='480x640', choices=[s[0] for s in SIZES])
    args = ap.parse_args()
    out = open(args.out, 'a') if args.out else None
    lib, C = _lib.load(), _lib.CONSTANTS
    mesh = LO.grid_mesh(args.side, 1, spacing=0.02)
    V, F = mesh['vertices'], mesh['faces']
    N, nf, B = V.shape[0], F.shape[0], args.poses
    poses = walk_poses(V, B)
    v, f = torch.from_numpy(V).to(DEV).double().contiguous(), torch.from_numpy(F).to(DEV).long().contiguous()
    lo, hi = V.min(axis=0), V.max(axis=0)
    colors = torch.from_numpy(((V - lo) / np.maximum(hi - lo, 1e-9)).astype(np.float32)).to(DEV).contiguous()
    RT, valid = P.pose_extrinsics(poses)
    rt_d, valid_d = torch.from_numpy(RT).to(DEV), torch.from_numpy(valid).to(DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    bg = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    emit(out, what='scene', vertices=N, faces=nf, poses=B, default_large_box=C['STIN_RENDER_LARGE_BOX'])
    stage = [C['STIN_RENDER_STAGE_' + s] for s in ('CLEAR', 'TRANSFORM', 'RASTER', 'LARGE', 'RESOLVE')]
    for name, cam, H, W in SIZES:
        ws_bytes = lib.stin_render_workspace_bytes(N, nf, H, W, B)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        camera = (ctypes.c_double * 4)(*cam)
        u8 = torch.empty(B, H, W, 3, dtype=torch.uint8, device=DEV)
        f32 = torch.empty(B, H, W, 3, dtype=torch.float32, device=DEV)
        depth = torch.empty(B, H, W, dtype=torch.uint16, device=DEV)
        face = torch.empty(B, H, W, dtype=torch.int32, device=DEV)

        def call(stages=0, large_box=0, float_colour=False):
            _lib.check(lib.stin_render_poses_f64(_ptr(v), N, _ptr(f), nf, _ptr(colors), 3, _ptr(rt_d), _ptr(valid_d), B, camera, H, W, 0.01,
                                                 1000.0, bg, B, large_box, stages, _ptr(f32) if float_colour else None,
                                                 None if float_colour else _ptr(u8), _ptr(depth), _ptr(face), _ptr(status), _ptr(ws), ws_bytes,
                                                 _stream(v)), 'stin_render_poses_f64')

        if args.trace_only:
            if name != args.trace_size:
                continue
            for _ in range(5):
                call()
            torch.cuda.synchronize()
            continue
        call()
        torch.cuda.synchronize()
        hit = face >= 0
        visible = int(torch.unique(face[hit]).numel() if bool(hit.any()) else 0)
        pairs = sum(int(torch.unique(face[p][face[p] >= 0]).numel()) for p in range(B))
        emit(out, what='images', size=name, workspace_MB=ws_bytes / 1e6, covered_share=float(hit.float().mean()), faces_seen_by_any_pose=visible,
             face_pose_pairs_that_win_a_pixel=pairs, centres_per_winning_pair=float(hit.sum()) / max(pairs, 1), status=int(status.item()))
        # ---- stages: cumulative masks, differences of medians
        mask, prev = 0, 0.0
        for s, label in zip(stage, ('clear', 'transform', 'raster (thread per face)', 'raster_large (wavefront per face)', 'resolve (uint8 colour)')):
            mask |= s
            t = timed(lambda: call(stages=mask), args.reps)
            extra = {}
            if label.startswith('resolve'):
                bound = B * H * W * (8 + 3 + 2 + 4) / (HBM_COPY_TBS * 1e12) * 1e3
                extra = dict(ms_byte_bound=bound, times_the_bound=(t['ms_median'] - prev) / bound)
            if label == 'clear':
                bound = B * H * W * 8 / (HBM_COPY_TBS * 1e12) * 1e3
                extra = dict(ms_byte_bound=bound, times_the_bound=t['ms_median'] / bound)
            emit(out, what='stage', size=name, stage=label, mask=mask, ms_cumulative=t['ms_median'], ms_stage=t['ms_median'] - prev,
                 us_per_pose=(t['ms_median'] - prev) / B * 1e3, ms_min=t['ms_min'], ms_max=t['ms_max'], **extra)
            prev = t['ms_median']
        whole_u8 = prev
        t4 = timed(lambda: call(stages=mask & ~stage[4]), args.reps)
        t5 = timed(lambda: call(float_colour=True), args.reps)
        bound = B * H * W * (8 + 12 + 2 + 4) / (HBM_COPY_TBS * 1e12) * 1e3
        emit(out, what='stage', size=name, stage='resolve (float32 colour)', ms_stage=t5['ms_median'] - t4['ms_median'],
             us_per_pose=(t5['ms_median'] - t4['ms_median']) / B * 1e3, ms_byte_bound=bound, times_the_bound=(t5['ms_median'] - t4['ms_median']) / bound)
        # ---- the large_box sweep, whole calls; the images must agree
        call()
        ref = (u8.clone(), depth.clone(), face.clone())
        for sweep in (0, 1):                                  # twice, in turn: the spread between the two is the noise of a figure
            for box in BOXES:
                t = timed(lambda: call(large_box=box), args.reps)
                agree = all(torch.equal(a, b) for a, b in zip(ref, (u8, depth, face)))
                emit(out, what='large_box', size=name, sweep=sweep, large_box=box, us_per_pose=t['ms_median'] / B * 1e3, images_agree=agree, **t)
                assert agree, 'the images depend on large_box'
        # ---- the yardstick: observe_vertices at S = 256 on the same scene and poses, scaled by the pixel count
        if name == SIZES[0][0]:
            obs = timed(lambda: P.observe_vertices(v, f, poses, fx=COLOR_CAM[0], fy=COLOR_CAM[1], width=1296, height=968, image_size=256, batch=B),
                        args.reps)
        rm = timed(lambda: views.render_mesh(v, f, colors, poses, cam, H, W, depth=True, face_ids=True, batch=B), args.reps)
        scale = H * W / (256.0 * 256.0)
        emit(out, what='yardstick', size=name, observe_vertices_S256_us_per_pose=obs['ms_median'] / B * 1e3, pixel_ratio=scale,
             scaled_yardstick_us_per_pose=obs['ms_median'] / B * 1e3 * scale, render_entry_point_us_per_pose=whole_u8 / B * 1e3,
             render_mesh_with_host_work_us_per_pose=rm['ms_median'] / B * 1e3,
             entry_point_over_scaled_yardstick=whole_u8 / (obs['ms_median'] * scale))


if __name__ == '__main__':
    main()
