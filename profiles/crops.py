"""Training crops on the GPU (csrc/stin_crop.hip): all crops of a scene in one batched call, one crop from a resident scene, and
the numpy restatement they are checked against.  Run on an MI355X:

    python profiles/crops.py --out DIR [--reps 20] [--sections gpu,cpu] [--trace-only]

1. preprocessing.crop_scene on the 200 704-vertex jittered grid and irregular Delaunay scenes (3 levels) and the 1 M-vertex grid
   scene, scaled to an 8 m extent, block 3.0, stride 1.5 (the shipped 3-D inpainting recipe): device events around the call (which
   ends in a synchronise of its own: it reads the count table and the status word), median of `reps` after warm-up -
   all grid crops in one call, and ONE crop (`positions=[(x, y)]`) including scene_io.sample_from_tensors on the device.
2. tests/_crop_oracle.crop_scene (numpy, one process) on the same 200 k scenes, all grid crops: wall clock, and its crops compared
   with the GPU's (bit-exact).
--trace-only: 5 grid calls and 5 single-crop calls on the 200 k grid scene and nothing else (for a rocprofv3 --kernel-trace
--stats run of its own).  Writes DIR/crops.json.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _crop_oracle as CO  # noqa: E402
from surface_texture_inpainting_net_amd import preprocessing as P, scene_io  # noqa: E402

DEV = 'cuda:0'
BLOCK, STRIDE, EXTENT = 3.0, 1.5, 8.0


def _median_ms(fn, reps, warm=3):
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
    return statistics.median(ts), min(ts), max(ts)


def _one_crop(resident, mask, centre):
    (_, crop), = P.crop_scene(resident, BLOCK, STRIDE, positions=[centre])
    return scene_io.sample_from_tensors(crop, mask[crop['vertices'][0][:, 9].long()], 3, cropped=True)


def gpu_section(reps, scenes):
    out = {}
    for name, n0, irregular in scenes:
        saved = CO.synthetic_scene(n0, 3, 5, irregular=irregular, extent=EXTENT)
        resident = CO.scene_to(saved, DEV)
        n = int(saved['vertices'][0].shape[0])
        mask = (torch.arange(n, device=DEV) % 4 == 0).long()
        crops = P.crop_scene(resident, BLOCK, STRIDE)
        sizes = [int(c['vertices'][0].shape[0]) for _, c in crops]
        t_all = _median_ms(lambda: P.crop_scene(resident, BLOCK, STRIDE), reps)
        t_ref = _median_ms(lambda: P.crop_scene(resident, BLOCK, STRIDE, reference_dilated_labels=True), max(3, reps // 4))
        t_one = _median_ms(lambda: _one_crop(resident, mask, (EXTENT / 2 + 0.3, EXTENT / 2 - 0.2)), reps)
        out[name] = dict(vertices=n, levels=3, directed_edges=int(saved['edges'][0].shape[0]), crops=len(crops),
                         crop_vertices_min_max=[min(sizes), max(sizes)], ms_all_grid_crops_one_call=t_all[0],
                         ms_all_grid_crops_min_max=t_all[1:], ms_all_grid_crops_reference_dilated_labels=t_ref[0],
                         ms_one_crop_with_sample_from_tensors=t_one[0], ms_one_crop_min_max=t_one[1:])
        print(name, out[name], flush=True)
        del resident
    return out


def cpu_section(scenes):
    out = {}
    for name, n0, irregular in scenes:
        saved = CO.synthetic_scene(n0, 3, 5, irregular=irregular, extent=EXTENT)
        got = P.crop_scene(CO.scene_to(saved, DEV), BLOCK, STRIDE)
        stats = {}
        t0 = time.perf_counter()
        want = CO.crop_scene(saved, BLOCK, STRIDE, stats=stats)
        dt = time.perf_counter() - t0
        same = [c for c, _ in got] == [c for c, _ in want] and all(CO.same_crop(a, b) is None for (_, a), (_, b) in zip(got, want))
        out[name] = dict(vertices=int(saved['vertices'][0].shape[0]), crops=len(want), restatement_s=dt, stats=stats,
                         gpu_equals_restatement=bool(same), cpus_visible=os.cpu_count(),
                         torch_threads=torch.get_num_threads(),
                         note='tests/_crop_oracle.crop_scene: numpy, one process; crops one after another')
        print(name, out[name], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--sections', default='gpu,cpu')
    ap.add_argument('--trace-only', action='store_true')
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    assert torch.cuda.is_available(), 'profiles/crops.py measures on the GPU only'
    if args.trace_only:
        resident = CO.scene_to(CO.synthetic_scene(200_000, 3, 5, extent=EXTENT), DEV)
        mask = (torch.arange(resident['vertices'][0].shape[0], device=DEV) % 4 == 0).long()
        for _ in range(5):
            P.crop_scene(resident, BLOCK, STRIDE)
        for _ in range(5):
            _one_crop(resident, mask, (EXTENT / 2 + 0.3, EXTENT / 2 - 0.2))
        torch.cuda.synchronize()
        return
    res = {'device': torch.cuda.get_device_name(0), 'block': BLOCK, 'stride': STRIDE, 'extent': EXTENT}
    secs = args.sections.split(',')
    if 'gpu' in secs:
        res['gpu'] = gpu_section(args.reps, [('grid_200k', 200_000, False), ('irregular_200k', 200_000, True),
                                             ('grid_1m', 1_000_000, False)])
    if 'cpu' in secs:
        res['cpu'] = cpu_section([('grid_200k', 200_000, False), ('irregular_200k', 200_000, True)])
    with open(os.path.join(args.out, 'crops.json'), 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
