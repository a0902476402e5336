"""Circle masks and training augmentation on the GPU (csrc/stin_mask.hip): cost per mask, cost inside the loader-fed resident
step, and the CPU heap BFS they replace.  Run on an MI355X:

    python profiles/augment.py --out DIR [--reps 20] [--quick]

1. One circle mask (R 16, frac 0.25) at 200 k and 1 M vertices on the jittered grid and the irregular Delaunay mesh: GPU time
   of preprocessing.circle_masks with a prebuilt adjacency (device events, median of `reps`), the launches it makes (init +
   max_iters batch launches + the value pass) and the batches the rule actually needed; also 16 masks of a scene in one call,
   and the adjacency build alone.
2. The loader-fed resident training step at 200 k vertices (bench.py's headline model, SceneLoader with the graph + plan
   resident) with and without augment = the shipped train_transform + CircleMask(16, 0.25): host clock over 3 epochs of 3
   scenes ending in a synchronise, after one untimed epoch.
3. The CPU heap BFS of the reference (tests/_mask_oracle.py) for the same mask at 200 k vertices (centres of a GPU mask).
Writes DIR/augment.json only.
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from surface_texture_inpainting_net_amd import augment, preprocessing as P  # noqa: E402
from surface_texture_inpainting_net_amd.synthetic import make_synthetic_mesh  # noqa: E402

DEV = 'cuda:0'


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


def masks_section(reps, sizes):
    out = {}
    for n0 in sizes:
        for kind in ('grid', 'irregular'):
            s = make_synthetic_mesh(n0, 1, seed=5, dilations=(), irregular=(kind == 'irregular'))
            n = int(s.x.shape[0])
            ei = s.edge_index.to(DEV)
            adj = P.mask_adjacency(ei, n)
            t_adj = _median_ms(lambda: P.mask_adjacency(ei, n, check=False), reps)
            seeds = iter(range(10 ** 6))
            t1 = _median_ms(lambda: P.circle_masks(ei, n, 16, 0.25, 1, next(seeds), adjacency=adj), reps)
            t16 = _median_ms(lambda: P.circle_masks(ei, n, 16, 0.25, 16, next(seeds), adjacency=adj), max(3, reps // 4))
            m, info = P.circle_masks(ei, n, 16, 0.25, 4, 7, adjacency=adj, return_centres=True)
            out['%s_%d' % (kind, n)] = dict(
                vertices=n, directed_edges=int(ei.shape[1]), ms_one_mask=t1[0], ms_one_mask_min_max=t1[1:],
                ms_16_masks_one_call=t16[0], ms_adjacency_build=t_adj[0],
                launches_per_call=1 + 32 + 1, batches_needed=info['batches'].reshape(-1).tolist(),
                masked_fraction=[float((m[i] > 0).float().mean()) for i in range(4)])
            print(kind, n, out['%s_%d' % (kind, n)], flush=True)
    return out


def step_section(reps_epochs=3, scenes=3, vertices=200_000):
    import bench
    from surface_texture_inpainting_net_amd import surfacetextureinpaintingnet as S
    from surface_texture_inpainting_net_amd.loader import SceneLoader
    from surface_texture_inpainting_net_amd.train_step import TrainStep
    cfg = dict(bench.CONFIG_3D)
    torch.manual_seed(0)
    net = S.define_G(**cfg).to(DEV)
    step = TrainStep(net, lr=7e-5, amsgrad=True, freeze_gc=True)
    items = [make_synthetic_mesh(vertices, 3, seed=1000 + i) for i in range(scenes)]
    comp = augment.from_config([{'type': 'CoordsNormalization', 'args': {'max_sizes': [1.5, 1.5, 1.5]}},
                                {'type': 'RandomLinearTransformation', 'args': {'flip': True}},
                                {'type': 'RandomRotation', 'args': {}}], circle_mask=augment.CircleMask(16, 0.25))
    out = {}
    order = [('plain', None), ('augment', comp), ('plain_again', None), ('augment_again', comp)]
    for name, aug in order:
        ld = SceneLoader(items, DEV, shuffle=False, cache_bytes=32 << 30, model=net, end_level=3, augment=aug)
        for smp in ld.epoch(0):
            step(smp)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for e in range(reps_epochs):
            for smp in ld.epoch(1 + e):
                step(smp)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out[name] = dict(ms_per_step=dt / (reps_epochs * scenes) * 1e3)
        print(name, out[name], flush=True)
    step.finish()
    # the augmentation alone on a resident sample, device events (what it adds to the compute stream)
    ld = SceneLoader(items[:1], DEV, shuffle=False, cache_bytes=32 << 30, model=net, end_level=3, augment=comp)
    list(ld.epoch(0))
    smp = next(iter(ld.epoch(1)))
    from surface_texture_inpainting_net_amd.loader import _ADJ_KEY
    adj = ld.cache._d[0][0][_ADJ_KEY]
    t = _median_ms(lambda: ld._augment([0], smp, None, adj), 20)
    out['augment_alone_device_ms'] = t[0]
    out['augment_alone_min_max'] = t[1:]
    return out


def cpu_section(vertices=200_000):
    from _mask_oracle import adjacency, heap_bfs_mask
    s = make_synthetic_mesh(vertices, 1, seed=5, dilations=())
    n = int(s.x.shape[0])
    m, info = P.circle_masks(s.edge_index.to(DEV), n, 16, 0.25, 1, 3, return_centres=True)
    cs = torch.cat(info['centres'][0][0]).cpu().numpy()
    adj = adjacency(s.edge_index.numpy(), n)
    t0 = time.perf_counter()
    want = heap_bfs_mask(adj, 16, cs)
    dt = time.perf_counter() - t0
    assert np.array_equal(want, m[0].cpu().numpy())
    return dict(vertices=n, centres=int(cs.size), heap_bfs_s=dt,
                note='tests/_mask_oracle.heap_bfs_mask (the reference loop without repeated pushes), one CPU thread; '
                     'the reference itself re-pushes every node from each neighbour and is slower still')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--sections', default='masks,step,cpu')
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    assert torch.cuda.is_available(), 'profiles/augment.py measures on the GPU only'
    res = {'device': torch.cuda.get_device_name(0)}
    secs = args.sections.split(',')
    if 'masks' in secs:
        res['masks'] = masks_section(5 if args.quick else args.reps, (200_000, 1_000_000))
    if 'step' in secs:
        res['step'] = step_section()
    if 'cpu' in secs:
        res['cpu'] = cpu_section()
    with open(os.path.join(args.out, 'augment.json'), 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
