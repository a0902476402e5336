"""What the image-graph loader and step metrics cost per training step at the shape of experiments/2d_inpainting config 1
(B = 4 images of 128 x 128 = 65 536 vertices, end_level 3, circle radius 18, ngf 64, 9 blocks, n_levels 2, random masks and
augmentation).  Run on an MI355X:

    python profiles/imagegraph.py --out DIR [--steps 40] [--windows 7]

One model, one TrainStep(use_mask_weighted_loss=False); the variants alternate window by window on the same box:
    fixed           the same resident sample with its cached plan every step (what the parent commit can run too)
    loader          batches from ImageGraphLoader (one record copy + one launch per batch, shared resident plan)
    loader_metrics  the same with metrics.ImageStepMetrics recording a row per step
A window is `steps` steps on the host clock ending in a synchronise; the figure is the median window (min / max beside it).
Also: device-event medians of build_samples and ImageStepMetrics.update alone, and the bytes the sample kernel moves.
Writes DIR/imagegraph.json only.
"""
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

from surface_texture_inpainting_net_amd import imagegraph as IG, metrics  # noqa: E402
from surface_texture_inpainting_net_amd import surfacetextureinpaintingnet as S  # noqa: E402
from surface_texture_inpainting_net_amd.train_step import TrainStep  # noqa: E402

DEV = 'cuda:0'
CFG = dict(input_nc=4, output_nc=3, ngf=64, filter_type='edgeconv', norm='instance', n_blocks=9, n_levels=2, pooling_type='max')
LOADER = dict(img_size=128, end_level=3, batch_size=4, circle_radius=18, crop_half_width=16, num_circles=4, is_train=True,
              random_mask=True, random_augmentation=True, seed=0)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--images', type=int, default=64)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    assert torch.cuda.is_available(), 'profiles/imagegraph.py measures on the GPU only'
    rng = np.random.RandomState(0)
    shapes = [(128, 128), (128, 171), (160, 128), (128, 129)]
    images = [rng.randint(0, 256, size=shapes[i % 4] + (3,)).astype(np.uint8) for i in range(args.images)]
    ld = IG.ImageGraphLoader(images, DEV, **LOADER)
    torch.manual_seed(0)
    net = S.define_G(**CFG).to(DEV)
    tracker = metrics.ImageStepMetrics(DEV, capacity=args.steps * (args.windows + 2))
    step = TrainStep(net, lr=1.4e-4, use_mask_weighted_loss=False, freeze_gc=True)
    fixed = next(iter(ld.epoch(0)))

    def batches(n, epoch0):
        e = epoch0
        while n > 0:
            for s in ld.epoch(e):
                if n == 0:
                    break
                yield s
                n -= 1
            e += 1

    def window(name, w):
        step.metrics = tracker if name == 'loader_metrics' else None
        it = [fixed] * args.steps if name == 'fixed' else batches(args.steps, 1 + 100 * w)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in it:
            step(s)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    names = ('fixed', 'loader', 'loader_metrics')
    for name in names:                                           # warm-up: code objects, plans of both batch sizes, pinned blocks
        window(name, 0)
    times = {n: [] for n in names}
    for w in range(args.windows):
        for name in names:
            times[name].append(window(name, 1 + w))
    step.metrics = None
    step.finish()
    res = {'device': torch.cuda.get_device_name(0), 'steps_per_window': args.steps, 'windows': args.windows,
           'vertices': int(fixed.x.shape[0]), 'edges_level0': int(fixed.edge_index.shape[1])}
    for n in names:
        res['ms_per_step_' + n] = dict(median=statistics.median(times[n]), min=min(times[n]), max=max(times[n]))
    res['loader_minus_fixed_ms'] = res['ms_per_step_loader']['median'] - res['ms_per_step_fixed']['median']
    res['metrics_minus_loader_ms'] = res['ms_per_step_loader_metrics']['median'] - res['ms_per_step_loader']['median']
    recs = ld.records_for(0, [0, 1, 2, 3])
    t = _median_ms(lambda: IG.build_samples(ld.pool, recs, 128, 18), 50)
    n = 4 * 128 * 128
    res['build_samples_device_ms'] = dict(median=t[0], min=t[1], max=t[2])
    res['build_samples_bytes'] = dict(per_pixel=3 + 12 + 16 + 1, per_batch=n * (3 + 12 + 16 + 1))
    with torch.no_grad():
        out = net(fixed)
    t = _median_ms(lambda: tracker.update(out, fixed), 50)
    res['image_metrics_device_ms'] = dict(median=t[0], min=t[1], max=t[2])
    res['image_metrics_bytes_per_batch'] = n * (12 + 12 + 1)
    t = _median_ms(lambda: IG.grid_levels(128, 3, 4, DEV), 20)
    res['grid_levels_device_ms'] = dict(median=t[0], min=t[1], max=t[2])
    rows = tracker.rows()
    res['last_row'] = dict(zip(tracker.KEYS, [float(v) for v in rows[-1, :4]]))
    with open(os.path.join(args.out, 'imagegraph.json'), 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
