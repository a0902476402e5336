"""Wall time of mesh clustering (preprocessing.cluster_mesh, csrc/stin_cluster.hip) on one GPU, for profiles/r25_mesh_cluster.md.

    python profiles/mesh_cluster.py [--side 450] [--spacing 0.05] [--cell 0.12] [--out FILE]

One mesh of about 200 k vertices (tests/_levels_oracle.grid_mesh(450, 7, spacing=0.05)).  Per figure: a warm-up call, then the
median of 5 calls, each bracketed by a device synchronisation (host clock):
* cluster_mesh, and its stages from its own `profile` dict (which adds a synchronisation per stage);
* vertex_clustering on the same vertices and the mesh's edges - the comparable figure the project has;
* graph_levels(mesh, [cell, '30', '30'], ...) - the clustering level and two QEM levels.
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _levels_oracle as LO  # noqa: E402
from surface_texture_inpainting_net_amd import preprocessing as P  # noqa: E402

DEV = 'cuda:0'


def emit(f, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if f is not None:
        f.write(line + '\n')
        f.flush()


def timed(fn, reps=5):
    fn()                                                                 # warm-up
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return out, float(np.median(times)), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', type=int, default=450)
    ap.add_argument('--spacing', type=float, default=0.05)
    ap.add_argument('--cell', type=float, default=0.12)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('profiles/mesh_cluster.py measures on the GPU only')
    f = open(args.out, 'a') if args.out else None
    mesh = LO.grid_mesh(args.side, 7, spacing=args.spacing)
    m = {k: torch.from_numpy(v).to(DEV) for k, v in mesh.items()}
    n, nf = int(m['vertices'].shape[0]), int(m['faces'].shape[0])

    (v, fc, t, nc), med, times = timed(lambda: P.cluster_mesh(m['vertices'], m['faces'], args.cell))
    emit(f, what='cluster_mesh', vertices=[n, nc], faces=[nf, int(fc.shape[0])], cell=args.cell, s_median=med, s_all=times)
    stages = []
    for _ in range(5):
        prof = {}
        P.cluster_mesh(m['vertices'], m['faces'], args.cell, profile=prof)
        stages.append(prof)
    emit(f, what='cluster_mesh stages', s_median={k: float(np.median([s[k] for s in stages])) for k in stages[0]})

    ei = P._mesh_edges(m['faces'], n).t().contiguous()
    (c32, tr, ce), med, times = timed(lambda: P.vertex_clustering(m['vertices'], ei, args.cell))
    emit(f, what='vertex_clustering', vertices=[n, int(c32.shape[0])], edges=[int(ei.shape[1]), int(ce.shape[0])], s_median=med,
         s_all=times, same_trace=bool(torch.equal(tr, t)), same_positions=bool(torch.equal(v.float(), c32)))

    levels = [str(args.cell), '30', '30']
    out, med, times = timed(lambda: P.graph_levels(m, levels, [0, 0, 1], [2, 4]))
    emit(f, what='graph_levels', levels=levels, vertices=[n] + [int(x.shape[0]) for x in out['vertices']], s_median=med, s_all=times)


if __name__ == '__main__':
    main()
