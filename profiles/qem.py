"""Timing of the QEM decimator (csrc/stin_qem.hip, preprocessing.decimate_qem) on one GPU.

    python profiles/qem.py [--side 448] [--percent 30 30 30] [--out FILE]

The hierarchy of `--level_params 100 30 30 30` on the benchmark's grid mesh (448^2 = 200 704 vertices): level '100' is the mesh
itself, every further level decimates the previous one.  Per level, after one untimed warm-up call on the same input:
* wall clock around a synchronised decimate_qem call (`reps` times; the minimum and all values);
* rounds, vertices and faces in and out;
* one further call with profile= : wall seconds per stage summed over the rounds, each stage bracketed by a device synchronisation
  ('structures' = the sorts that build the unique edges and the two CSRs, 'edges' = placement, cost and validity, 'select' = the
  two minimum passes and the host read of the selected count, 'collapse', 'remap' = face remap and compaction; 'setup' = range check
  and vertex quadrics, 'finish' = trace).  The synchronisations make the split add up to more than the unprofiled call.
* vertex_normals of the result.
Then graph_levels(mesh, ['100'] + percentages) end to end.  Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', type=int, default=448)
    ap.add_argument('--percent', type=int, nargs='+', default=[30, 30, 30])
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    f = open(args.out, 'a') if args.out else None
    mesh = LO.grid_mesh(args.side, 1, spacing=0.02)
    m = {k: torch.from_numpy(v).to(DEV) for k, v in mesh.items()}
    v, faces = m['vertices'], m['faces']
    total = 0.0
    for level, pct in enumerate(args.percent, 1):
        warm, _ = wall(lambda: P.decimate_qem(v, faces, percent=pct))
        times = []
        for _ in range(args.reps):
            dt, out = wall(lambda: P.decimate_qem(v, faces, percent=pct))
            times.append(dt)
        prof = {}
        P.decimate_qem(v, faces, percent=pct, profile=prof)
        rounds, n_target = prof.pop('rounds'), prof.pop('n_target')
        tn, _ = wall(lambda: P.vertex_normals(out[0], out[1]))
        tn, _ = wall(lambda: P.vertex_normals(out[0], out[1]))
        emit(f, what='decimate_qem', level=level, percent=pct, vertices_in=int(v.shape[0]), faces_in=int(faces.shape[0]),
             vertices_out=int(out[3]), faces_out=int(out[1].shape[0]), n_target=n_target, rounds=rounds, s_first=warm, s_min=min(times),
             s_all=times, stage_s={k: round(x, 6) for k, x in prof.items()},
             stage_ms_per_round={k: round(1e3 * x / max(rounds, 1), 4) for k, x in prof.items() if k not in ('setup', 'finish')},
             vertex_normals_s=tn)
        total += min(times)
        v, faces = out[0], out[1]
    emit(f, what='decimate_qem total', levels=args.percent, s_sum_of_min=total)
    levels = ['100'] + [str(p) for p in args.percent]
    dil = [0] * len(levels)
    dil[-1] = 1
    times = []
    for _ in range(2):
        dt, out = wall(lambda: P.graph_levels(m, levels, dil, [2, 4]))
        times.append(dt)
    emit(f, what='graph_levels', levels=levels, vertices=[int(x.shape[0]) for x in out['vertices']], s_first=times[0], s_second=times[1])


if __name__ == '__main__':
    main()
