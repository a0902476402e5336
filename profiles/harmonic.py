"""Wall time, iterations and traffic of the harmonic fill (csrc/stin_harmonic.hip: preprocessing.harmonic_fill / harmonic_inpaint)
on one GPU, and its l1 / psnr beside knn_inpaint's on a synthetic scene.

    python profiles/harmonic.py [--out FILE] [--side 448] [--radius 16] [--reps 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python profiles/harmonic.py --traced
    python profiles/harmonic.py --trace DIR/run_kernel_trace.csv

Mesh: tests/_levels_oracle.grid_mesh(side, 1, spacing 0.02) - 448^2 = 200 704 jittered vertices with faces.  Mask: the first of
`circle_masks(radius=16, frac 0.25, seed 1)` (the shipped circle masks).  Colours: a smooth synthetic texture of the positions in
[-1, 1] (three channels, wavelengths from 2.5 to 0.4 units: a hole of 16 hops is 0.4 units across).  Every time is wall clock
(time.perf_counter between device synchronisations) around the Python call a user makes: one warm-up call, then the median of `reps`.

* harmonic_adjacency (the sorted CSR) beside mask_adjacency;
* harmonic_fill with a ready adjacency, uniform and inverse-length weights, tol 1e-6: ms, iterations per channel, unknowns;
* the same iterations with no host read (max_iterations = K, iterations_per_sync=None), and K = 0 (reach, setup and finish alone):
  their difference over K is the time of one iteration, launches included;
* the compulsory bytes of one iteration, counted from the shapes;
* l1, psnr and psnr_mask_only (metrics.StepMetrics) of harmonic_inpaint (uniform, inverse-length) and knn_inpaint(k=3).
--traced runs the no-host-read call three times for a kernel trace; --trace sums the kernel time and the gaps of the last
iteration stream in such a trace.  Times are recorded, not gated.  Prints one JSON line per measurement."""
import argparse
import csv
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


def trace_summary(path):
    """The last uninterrupted run of k_harm_product / k_harm_update launches of a kernel trace: span, kernel time, gaps."""
    rows = []
    for r in csv.DictReader(open(path)):
        rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']))
    rows.sort()
    it = [i for i, r in enumerate(rows) if 'k_harm_product' in r[2] or 'k_harm_update' in r[2]]
    hi = it[-1]
    lo = hi
    while lo - 1 >= 0 and ('k_harm_product' in rows[lo - 1][2] or 'k_harm_update' in rows[lo - 1][2]):
        lo -= 1
    seg = rows[lo:hi + 1]
    span = seg[-1][1] - seg[0][0]
    prod = [e - s for s, e, n in seg if 'k_harm_product' in n]
    upd = [e - s for s, e, n in seg if 'k_harm_update' in n]
    gaps = [seg[i + 1][0] - seg[i][1] for i in range(len(seg) - 1)]
    emit(None, what='iteration stream (last call of the trace)', launches=len(seg), iterations=len(prod), span_us=span / 1e3,
         kernel_us=(sum(prod) + sum(upd)) / 1e3, gap_us=sum(gaps) / 1e3, gap_share=sum(gaps) / span,
         product_us_median=statistics.median(prod) / 1e3, update_us_median=statistics.median(upd) / 1e3,
         gap_us_median=statistics.median(gaps) / 1e3, us_per_iteration=span / 1e3 / max(len(prod), 1))


class Sample:
    pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--side', type=int, default=448)
    ap.add_argument('--radius', type=int, default=16)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--traced', action='store_true')
    ap.add_argument('--trace', default=None)
    args = ap.parse_args()
    if args.trace:
        return trace_summary(args.trace)
    if not torch.cuda.is_available():
        raise SystemExit('profiles/harmonic.py measures on a GPU; none is visible')
    import _levels_oracle as LO
    from surface_texture_inpainting_net_amd import _lib, metrics, preprocessing as P
    f = open(args.out, 'a') if args.out else None
    props = torch.cuda.get_device_properties(0)
    emit(f, what='device', name=props.name, cus=int(props.multi_processor_count), lib=_lib.LIB_PATH)
    mesh = LO.grid_mesh(args.side, 1, spacing=0.02)
    Vn = mesh['vertices']
    V, F = torch.from_numpy(Vn).to(DEV), torch.from_numpy(mesh['faces']).to(DEV)
    n = int(V.shape[0])
    ei = P.edges_from_faces(F, n)
    x, y = Vn[:, 0], Vn[:, 1]
    color = np.stack([0.6 * np.sin(2.5 * x) * np.cos(2.0 * y) + 0.4 * np.sin(9.0 * x + 1.0) * np.sin(7.0 * y),
                      0.7 * np.cos(1.5 * x + 2.0 * y) + 0.3 * np.sin(15.0 * y),
                      0.5 * np.sin(4.0 * (x - y)) + 0.5 * np.cos(6.0 * x) * np.cos(5.0 * y)], axis=1).astype(np.float32)
    color = torch.from_numpy(color).to(DEV)
    mask = P.circle_masks(ei, n, radius=args.radius, frac_masked_vertices=0.25, num_masks=1, seed=1)[0]
    masked = mask > 0
    emit(f, what='scene', vertices=n, directed_slots=2 * int(ei.shape[1]), masked=int(masked.sum()), share=float(masked.double().mean()))
    if not args.traced:
        _, ms, ts = wall(lambda: P.mask_adjacency(ei, n), args.reps)
        emit(f, what='mask_adjacency', ms_median=ms, ms_all=ts)
        _, ms, ts = wall(lambda: P.harmonic_adjacency(ei, n), args.reps)
        emit(f, what='harmonic_adjacency (sorted rows)', ms_median=ms, ms_all=ts)
        _, ms, ts = wall(lambda: P.harmonic_adjacency(ei, n, vertices=V), args.reps)
        emit(f, what='harmonic_adjacency (sorted rows, with lengths)', ms_median=ms, ms_all=ts)
    adj = P.harmonic_adjacency(ei, n, vertices=V)
    results = {}
    for weights in ('uniform', 'inverse_length'):
        (out, info), ms, ts = wall(lambda: P.harmonic_fill(color, masked, adjacency=adj, weights=weights, return_info=True), args.reps)
        results[weights] = out
        K = max(info['iterations'])
        n_u = info['n_unknown']
        rowptr, col = adj[0], adj[1]
        deg = (rowptr[1:] - rowptr[:-1]).long()
        slots_u = int(deg[masked].sum())
        emit(f, what='harmonic_fill, ready adjacency, tol 1e-6, 16 iterations per host read', weights=weights, unknowns=n_u,
             unreached=info['n_unreached'], iterations=info['iterations'], flags=info['flags'], rr=info['rr'], bb=info['bb'],
             ms_median=ms, ms_all=ts)
        if args.traced:
            for _ in range(3):
                P.harmonic_fill(color, masked, adjacency=adj, weights=weights, max_iterations=K, iterations_per_sync=None)
            torch.cuda.synchronize()
            break
        (o2, st), msK, tsK = wall(lambda: P.harmonic_fill(color, masked, adjacency=adj, weights=weights, max_iterations=K,
                                                          iterations_per_sync=None), args.reps)
        _, ms0, ts0 = wall(lambda: P.harmonic_fill(color, masked, adjacency=adj, weights=weights, max_iterations=0,
                                                   iterations_per_sync=None), args.reps)
        C = 3
        wbytes = 8 if weights != 'uniform' else 0
        # every array of an iteration once: product reads z, p_old, d, unk, rowptr, ucol (+ weight) and writes p, q; update reads
        # p, q, x, r, d and writes x, r, z
        product = n_u * (2 * 8 * C + 8 + 4 + 4) + slots_u * (4 + wbytes) + n_u * 2 * 8 * C
        update = n_u * (4 * 8 * C + 8) + n_u * 3 * 8 * C
        gathered = slots_u * 2 * 8 * C                               # what the product's gathers ask the caches for on top
        emit(f, what='harmonic_fill, no host read', weights=weights, max_iterations=K, equal_bytes=bool(torch.equal(o2, out)),
             ms_median=msK, ms_all=tsK, ms_median_zero_iterations=ms0, ms_all_zero_iterations=ts0,
             us_per_iteration=(msK - ms0) * 1e3 / max(K, 1), compulsory_bytes_product=product, compulsory_bytes_update=update,
             gathered_bytes_product=gathered, slots_of_unknown_rows=slots_u)
    if args.traced:
        return
    _, ms, ts = wall(lambda: P.harmonic_fill(color, masked, edge_index=ei), args.reps)
    emit(f, what='harmonic_fill, from edge_index (uniform)', ms_median=ms, ms_all=ts)
    # ---- quality beside the k-nearest baseline
    s = Sample()
    s.pos, s.color, s.mask, s.edge_index = V.float(), color, mask.reshape(-1, 1), ei
    m = metrics.StepMetrics(DEV, capacity=8)
    keys = metrics.StepMetrics.KEYS
    preds = {'harmonic_inpaint (uniform)': P.harmonic_inpaint(s), 'harmonic_inpaint (inverse_length)': P.harmonic_inpaint(s, weights='inverse_length'),
             'knn_inpaint (k=3)': P.knn_inpaint(s, k=3), 'constant 0': torch.zeros_like(color)}
    assert torch.equal(preds['harmonic_inpaint (uniform)'], results['uniform'])
    for name, pred in preds.items():
        row = m.update(pred, s, composite=True).cpu().tolist()
        emit(f, what='quality', prediction=name, **{k: row[keys.index(k)] for k in ('l1', 'mse', 'psnr', 'psnr_mask_only', 'graph_tv', 'graph_lap_var')})
    _, ms, ts = wall(lambda: P.knn_inpaint(s, k=3), args.reps)
    emit(f, what='knn_inpaint (k=3)', ms_median=ms, ms_all=ts)
    _, ms, ts = wall(lambda: P.harmonic_inpaint(s), args.reps)
    emit(f, what='harmonic_inpaint (uniform, from the sample)', ms_median=ms, ms_all=ts)


if __name__ == '__main__':
    main()
