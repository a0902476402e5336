"""Timing of the graph level generation path (csrc/stin_levels.hip, preprocessing.graph_levels) on one GPU.

    python profiles/levels.py [--cpu] [--out FILE]

* stin_nearest_f64 at 200 704 x 200 704 and 60 025 x 200 704 (queries x points), HIP events around `reps` calls after a warm-up,
  with the chunk count the host picks and with chunks = 1;
* graph_levels for a three-level synthetic mesh in both modes (vertex clustering; decimator mode with synthetic trace files),
  wall clock around a synchronised call;
* --cpu: tests/_levels_oracle.py (the numpy restatement; the reference itself is not on the GPU machine) on a slice of the same
  nearest-neighbour inputs and on the same graph_levels inputs, as the CPU figure.
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
from surface_texture_inpainting_net_amd import _lib, preprocessing as P  # noqa: E402

DEV = 'cuda:0'


def emit(f, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if f is not None:
        f.write(line + '\n')
        f.flush()


def time_nearest(q, p, chunks, warmup=2, reps=5):
    for _ in range(warmup):
        P.nearest(q, p, chunks=chunks)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        P.nearest(q, p, chunks=chunks)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)


def trace_file(fine, coarse, path, seed):
    """A synthetic decimator trace: one row per coarse vertex (shuffled) naming the fine vertices nearest to it, a fifth left out."""
    rng = np.random.default_rng(seed)
    owner = P.nearest(torch.from_numpy(fine).to(DEV), torch.from_numpy(coarse).to(DEV)).cpu().numpy()
    order = np.argsort(owner, kind='stable')
    ptr = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=coarse.shape[0]))])
    with open(path, 'w') as f:
        for c in rng.permutation(coarse.shape[0]):
            fields = ['%.6g' % x for x in coarse[c]]
            for m in order[ptr[c]:ptr[c + 1]]:
                if rng.uniform() > 0.2:
                    fields += ['%.6g' % x for x in fine[m]]
            f.write(';'.join(fields) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cpu', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--side', type=int, default=448)            # 448^2 = 200 704 vertices
    args = ap.parse_args()
    f = open(args.out, 'a') if args.out else None
    lib = _lib.load()
    rng = np.random.default_rng(0)
    pts = rng.uniform(0, 8, (200704, 3))
    for nq in (200704, 60025):
        qs = rng.uniform(0, 8, (nq, 3))
        q, p = torch.from_numpy(qs).to(DEV), torch.from_numpy(pts).to(DEV)
        auto = int(lib.stin_nearest_chunks(nq, pts.shape[0]))
        for chunks in sorted({auto, 1}):
            t = time_nearest(q, p, chunks)
            emit(f, what='stin_nearest_f64', Q=nq, P=pts.shape[0], chunks=chunks, auto=chunks == auto, ms_min=t[0], ms_median=t[len(t) // 2],
                 ms_all=t, pairs_per_s=nq * pts.shape[0] / (t[0] * 1e-3))
        if args.cpu:
            k = 2000
            t0 = time.perf_counter()
            want = LO.nearest(qs[:k], pts)
            dt = time.perf_counter() - t0
            got = P.nearest(q[:k], p).cpu().numpy()
            emit(f, what='numpy restatement nearest', Q=k, P=pts.shape[0], s=dt, scaled_to_Q=nq, s_scaled=dt * nq / k,
                 equal=bool(np.array_equal(got, want)))
    # ---- graph_levels, three levels, both modes
    side = args.side
    mesh = LO.grid_mesh(side, 1, spacing=0.02)
    n = mesh['vertices'].shape[0]
    labels = rng.integers(0, 21, n)
    m = {k: torch.from_numpy(v).to(DEV) for k, v in mesh.items()}
    lab = torch.from_numpy(labels).to(DEV)
    import tempfile
    with tempfile.TemporaryDirectory() as root:
        c1, c2 = LO.grid_mesh(side // 2, 2, spacing=0.04), LO.grid_mesh(side // 4, 3, spacing=0.08)
        trace_file(mesh['vertices'], c1['vertices'], os.path.join(root, 'l1.csv'), 4)
        trace_file(c1['vertices'], c2['vertices'], os.path.join(root, 'l2.csv'), 5)
        t0 = time.perf_counter()
        rows = [P.read_trace_csv(os.path.join(root, 'l%d.csv' % i)) for i in (1, 2)]
        emit(f, what='read_trace_csv (host)', rows=[int(r[0].shape[0]) for r in rows], entries=[int(r[1].shape[0]) for r in rows],
             s=time.perf_counter() - t0)
    modes = {'vertex clustering': [0.04, 0.08, 0.16],
             'decimator': ['100'] + [dict(vertices=c['vertices'], faces=c['faces'], normals=c['normals'], csv=r)
                                     for c, r in ((c1, rows[0]), (c2, rows[1]))]}
    for name, levels in modes.items():
        lv = [{k: (v if k == 'csv' else torch.from_numpy(v).to(DEV)) for k, v in x.items()} if isinstance(x, dict) else x for x in levels]
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = P.graph_levels(m, lv, [0, 0, 1], [2, 4], labels=lab)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        emit(f, what='graph_levels', mode=name, vertices=[n] + [int(v.shape[0]) for v in out['vertices']], s_first=times[0],
             s_min=min(times[1:]), s_all=times)
        if args.cpu and side <= 160:
            t0 = time.perf_counter()
            want = LO.graph_levels(mesh, levels, [0, 0, 1], [2, 4], labels=labels)
            emit(f, what='numpy restatement graph_levels', mode=name, s=time.perf_counter() - t0,
                 traces_equal=all(bool(np.array_equal(a.cpu().numpy(), b)) for a, b in zip(out['traces'], want['traces'])))


if __name__ == '__main__':
    main()
