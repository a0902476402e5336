"""Wall time and decision rounds of the surface samples (csrc/stin_surface.hip: preprocessing.sample_surface / poisson_disk /
surface_centres / circle_masks_on_surface) on one GPU, with the numpy oracle's CPU time at the sizes it finishes beside them.

    python profiles/surface_samples.py [--out FILE] [--side 448] [--candidates 100000 1000000] [--spacing 0.2 0.05] [--reps 3]
                                       [--oracle-seconds 60]

Mesh: tests/_levels_oracle.grid_mesh(side, 1, spacing 0.02) - 448^2 = 200 704 vertices (make_synthetic_mesh's size) with faces.
Every figure is wall clock (time.perf_counter between device synchronisations) around the Python call a user makes, host reads
included: one warm-up call, then the median of `reps`.  Times are recorded, not gated: nothing earlier exists to compare with.

* sample_surface at every candidate count (weights, scan and draw);
* poisson_disk on those samples at every spacing: kept points, decision rounds, rounds launched, the grid;
* surface_centres (draw, thinning, nearest vertex, first occurrences) at every (candidates, spacing);
* circle_masks_on_surface (radius 16, four masks) beside circle_masks on the same mesh;
* the numpy oracle's poisson_disk (brute force) and sample_surface on the CPU, each size only while the one before it took less
  than --oracle-seconds / 10.
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
import _surface_oracle as SO  # noqa: E402
from surface_texture_inpainting_net_amd import _lib, preprocessing as P  # noqa: E402

DEV = 'cuda:0'


def emit(f, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if f is not None:
        f.write(line + '\n')
        f.flush()


def wall(fn, reps):
    ts, out = [], None
    for i in range(1 + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if i >= 1:
            ts.append((time.perf_counter() - t0) * 1e3)
    return out, statistics.median(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--side', type=int, default=448)
    ap.add_argument('--candidates', type=int, nargs='+', default=[100_000, 1_000_000])
    ap.add_argument('--spacing', type=float, nargs='+', default=[0.2, 0.05])
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--oracle-seconds', type=float, default=60.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('profiles/surface_samples.py measures on a GPU; none is visible')
    f = open(args.out, 'a') if args.out else None
    props = torch.cuda.get_device_properties(0)
    emit(f, what='device', name=props.name, cus=int(props.multi_processor_count), lib=_lib.LIB_PATH)
    mesh = LO.grid_mesh(args.side, 1, spacing=0.02)
    Vn, Fn = mesh['vertices'], mesh['faces']
    V, F = torch.from_numpy(Vn).to(DEV), torch.from_numpy(Fn).to(DEV)
    n = int(V.shape[0])
    _, _, _, _, st = P._surface_mesh(V, F, 'profile')
    emit(f, what='mesh', vertices=n, faces=int(F.shape[0]), area=P._surface_area(st))
    for C in args.candidates:
        (pts, _, _), ms, ts = wall(lambda: P.sample_surface(V, F, C, seed=1), args.reps)
        emit(f, what='sample_surface', candidates=C, ms_median=ms, ms_all=ts)
        for s in args.spacing:
            (kept, info), ms, ts = wall(lambda: P.poisson_disk(pts, s, return_info=True), args.reps)
            emit(f, what='poisson_disk', candidates=C, spacing=s, kept=int(kept.numel()), rounds=info['rounds'],
                 launched=info['launched'], grid=list(info['grid']), ms_median=ms, ms_all=ts)
            ids, ms, ts = wall(lambda: P.surface_centres(V, F, C, seed=1, spacing=s), args.reps)
            emit(f, what='surface_centres', candidates=C, spacing=s, centres=int(ids.numel()), ms_median=ms, ms_all=ts)
    ei = P.edges_from_faces(F, n)
    for s in args.spacing:
        (_, info), ms, ts = wall(lambda: P.circle_masks_on_surface(V, F, radius=16, num_masks=4, seed=1, spacing=s, edge_index=ei,
                                                                   return_centres=True), args.reps)
        emit(f, what='circle_masks_on_surface', radius=16, masks=4, spacing=s, candidates=info['candidates'],
             batches=info['batches'][:, 0].tolist(), centres=info['sizes'].sum(dim=(1, 2)).tolist(),
             share=(info['masked'][:, 0].double() / n).tolist(), exhausted=info['exhausted'][:, 0].tolist(), ms_median=ms, ms_all=ts)
    (_, info), ms, ts = wall(lambda: P.circle_masks(ei, n, radius=16, num_masks=4, seed=1, return_centres=True), args.reps)
    emit(f, what='circle_masks', radius=16, masks=4, batches=info['batches'][:, 0].tolist(),
         centres=info['sizes'].sum(dim=(1, 2)).tolist(), share=(info['masked'][:, 0].double() / n).tolist(), ms_median=ms, ms_all=ts)
    # ---- the numpy oracle on the CPU
    for s in args.spacing:
        last = 0.0
        for C in (1_000, 10_000, 100_000, 1_000_000):
            if last > args.oracle_seconds / 10 or C > max(args.candidates):
                break
            t0 = time.perf_counter()
            p, _, _ = SO.sample_surface(Vn, Fn, C, 1)
            t1 = time.perf_counter()
            kept = SO.poisson_disk(p, s)
            last = time.perf_counter() - t1
            got = P.poisson_disk(torch.from_numpy(p).to(DEV), s).cpu().numpy()
            emit(f, what='oracle (numpy, CPU)', candidates=C, spacing=s, kept=int(len(kept)), sample_surface_ms=(t1 - t0) * 1e3,
                 poisson_disk_ms=last * 1e3, equal_to_device=bool(np.array_equal(kept, got)))


if __name__ == '__main__':
    main()
