"""Wall time, rounds and work inflation of the geodesic circle masks (csrc/stin_geodesic.hip: preprocessing.geodesic_adjacency /
geodesic_distance / circle_mask_from_centres_geodesic / circle_masks_geodesic) on one GPU, beside the hop pass on the same mesh and
centres and the oracle's heap Dijkstra on the CPU.

    python profiles/geodesic.py [--out FILE] [--side 448] [--radius-edges 16] [--levels 1 2 4 8] [--reps 5] [--no-oracle]

Mesh: tests/_levels_oracle.grid_mesh(side, 1, spacing 0.02) - 448^2 = 200 704 jittered vertices with faces.  Centres: the ones
`circle_masks(radius=16, frac 0.25)` draws for one mask of that mesh (the circle-mask workload's).  Radius: --radius-edges mean edge
lengths.  Every time is wall clock (time.perf_counter between device synchronisations) around the Python call a user makes, host
reads included: one warm-up call, then the median of `reps`.  Times are recorded, not gated.

* geodesic_adjacency (CSR + lengths) and the parent's mask_adjacency;
* circle_mask_from_centres_geodesic with a ready adjacency, per `levels`: ms, rounds that found work, rounds launched, directed
  edges relaxed, and relaxed / (directed edges whose tail lies inside the radius) = the schedule's work inflation (1.0 = every
  vertex inside expanded exactly once, Dijkstra's count);
* the same distance with max_rounds = the rounds it needs (no host read between the launches);
* circle_mask_from_centres (hop radius --radius-edges) on the same centres: the yardstick;
* circle_masks_geodesic with four masks;
* the oracle's heap Dijkstra on the CPU, and whether its bytes equal the device's.
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

import _geodesic_oracle as GO  # noqa: E402
import _levels_oracle as LO  # noqa: E402
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
    ap.add_argument('--radius-edges', type=int, default=16)
    ap.add_argument('--levels', type=int, nargs='+', default=[1, 2, 4, 8])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-oracle', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('profiles/geodesic.py measures on a GPU; none is visible')
    f = open(args.out, 'a') if args.out else None
    props = torch.cuda.get_device_properties(0)
    emit(f, what='device', name=props.name, cus=int(props.multi_processor_count), lib=_lib.LIB_PATH)
    mesh = LO.grid_mesh(args.side, 1, spacing=0.02)
    Vn, Fn = mesh['vertices'], mesh['faces']
    V, F = torch.from_numpy(Vn).to(DEV), torch.from_numpy(Fn).to(DEV)
    n = int(V.shape[0])
    ei = P.edges_from_faces(F, n)
    _, ms_hop_adj, ts = wall(lambda: P.mask_adjacency(ei, n), args.reps)
    emit(f, what='mask_adjacency', ms_median=ms_hop_adj, ms_all=ts)
    adj, ms, ts = wall(lambda: P.geodesic_adjacency(V, edge_index=ei), args.reps)
    rowptr, col, length = adj
    mean_edge = float(length.mean())
    radius = args.radius_edges * mean_edge
    emit(f, what='geodesic_adjacency', vertices=n, directed_edges=int(col.numel()), mean_edge=mean_edge,
         min_edge=float(length.min()), max_edge=float(length.max()), radius=radius, ms_median=ms, ms_all=ts)
    _, info = P.circle_masks(ei, n, radius=args.radius_edges, num_masks=1, seed=1, return_centres=True)
    centres = torch.cat(info['centres'][0][0])
    emit(f, what='centres', count=int(centres.numel()), batches=int(info['batches'][0, 0]))

    dist = P.geodesic_distance(V, centres, max_distance=radius, adjacency=adj)
    inside = torch.isfinite(dist)
    deg = (rowptr[1:] - rowptr[:-1]).long()
    inside_edges = int(deg[inside].sum())
    emit(f, what='inside', vertices=int(inside.sum()), share=float(inside.double().mean()), directed_edges=inside_edges)
    for lv in args.levels:
        (_, gi), ms, ts = wall(lambda: P.geodesic_distance(V, centres, max_distance=radius, adjacency=adj, levels=lv, return_info=True),
                               args.reps)
        same = bool(torch.equal(P.geodesic_distance(V, centres, max_distance=radius, adjacency=adj, levels=lv), dist))
        emit(f, what='geodesic_distance', levels=lv, rounds=gi['rounds'], launched=gi['launched'], relaxed=gi['relaxed'],
             inflation=gi['relaxed'] / max(inside_edges, 1), equal_to_default=same, ms_median=ms, ms_all=ts)
        k = gi['rounds']
        (_, st), ms, ts = wall(lambda: P.geodesic_distance(V, centres, max_distance=radius, adjacency=adj, levels=lv, max_rounds=k),
                               args.reps)
        emit(f, what='geodesic_distance, max_rounds (no host read)', levels=lv, max_rounds=k, status=st.tolist(), ms_median=ms, ms_all=ts)
    mk, ms, ts = wall(lambda: P.circle_mask_from_centres_geodesic(V, centres, radius, adjacency=adj), args.reps)
    emit(f, what='circle_mask_from_centres_geodesic (ready adjacency)', levels=P.GEODESIC_LEVELS, masked=int((mk > 0).sum()),
         ms_median=ms, ms_all=ts)
    mk2, ms, ts = wall(lambda: P.circle_mask_from_centres_geodesic(V, centres, radius, edge_index=ei), args.reps)
    emit(f, what='circle_mask_from_centres_geodesic (from edge_index)', equal=bool(torch.equal(mk, mk2)), ms_median=ms, ms_all=ts)
    hop, ms, ts = wall(lambda: P.circle_mask_from_centres(ei, n, args.radius_edges, centres), args.reps)
    emit(f, what='circle_mask_from_centres (hop, from edge_index)', masked=int((hop > 0).sum()), ms_median=ms, ms_all=ts,
         ms_minus_adjacency=ms - ms_hop_adj)
    (_, info), ms, ts = wall(lambda: P.circle_masks_geodesic(V, F, radius, num_masks=4, seed=1, spacing=0.2, edge_index=ei,
                                                             return_centres=True), args.reps)
    emit(f, what='circle_masks_geodesic', masks=4, spacing=0.2, batches=info['batches'][:, 0].tolist(),
         centres=info['sizes'].sum(dim=(1, 2)).tolist(), share=(info['masked'][:, 0].double() / n).tolist(),
         exhausted=info['exhausted'][:, 0].tolist(), ms_median=ms, ms_all=ts)
    if args.no_oracle:
        return
    t0 = time.perf_counter()
    oadj = GO.weighted_adjacency(Vn, ei.cpu().numpy())
    t1 = time.perf_counter()
    want = GO.dijkstra(oadj, centres.cpu().numpy(), radius)
    t2 = time.perf_counter()
    emit(f, what='oracle (heap Dijkstra, CPU)', adjacency_ms=(t1 - t0) * 1e3, dijkstra_ms=(t2 - t1) * 1e3,
         equal_to_device=bool(want.tobytes() == dist.cpu().numpy().tobytes()))


if __name__ == '__main__':
    main()
