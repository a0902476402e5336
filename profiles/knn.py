"""Timing of the k-nearest-neighbour path (csrc/stin_knn.hip, preprocessing.knn / fill_unseen_colors) on one GPU, with the parent's
stin_nearest_f64 on the same shapes in the same run as the yardstick.

    python profiles/knn.py [--out FILE] [--side 448] [--reps 7] [--only KERNELS]

* stin_nearest_f64 and stin_knn_f64 with k = 1, 3, 8, 16 on the vertices of the synthetic mesh (tests/_levels_oracle.grid_mesh:
  448^2 = 200 704 vertices in random order) at three shapes: all vertices against all; 60 025 queries against all; the fill's
  shape - the 25 % of the vertices marked unseen as queries (an index list) against the full array with point_valid.
  HIP events around one call (outputs, workspace and flag word allocated beforehand, no host read inside), two warm-up calls, the
  median of `reps` calls; nearest and the four k alternate inside every repetition.
* beside each time the fp64 vector-ALU bound: pairs x 9 operations (3 subtractions, 3 multiplications, 2 additions, 1 compare - the
  kernel's header comment; nearest has two selects more) over CUs x 64 lanes x clock, with the clock the device reports, and the
  achieved fraction.  Invalid points are counted as pairs: the kernel does their arithmetic.
* FrameColors.result() next to result(knn=3) on the same mesh with 25 % of the counts zero: wall clock around a synchronised call.
* --only kernels: just one nearest and one knn call per k at the first shape, for a `rocprofv3 --kernel-trace --stats` run.
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
KS = (1, 3, 8, 16)
OPS_PER_PAIR = 9


def emit(f, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if f is not None:
        f.write(line + '\n')
        f.flush()


class Case:
    """One shape: the queries (all rows, or an index list), the points, the validity bytes, and buffers for every call."""

    def __init__(self, name, q, p, q_index=None, valid=None):
        self.name, self.q, self.p, self.q_index, self.valid = name, q, p, q_index, valid
        self.nq = int(q.shape[0]) if q_index is None else int(q_index.numel())
        self.flags = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.idx = torch.empty(int(q.shape[0]), max(KS), dtype=torch.int64, device=DEV)
        self.d2 = torch.empty(int(q.shape[0]), max(KS), dtype=torch.float64, device=DEV)

    def nearest(self):
        if self.valid is not None:
            return False                                               # nearest cannot restrict the points in place
        P._nearest_launch(self.q, self.p, self.idx.view(-1), self.flags, q_index=self.q_index, n_queries=self.nq, d2=self.d2.view(-1))
        return True

    def knn(self, k):
        P._knn_launch(self.q, self.p, k, self.idx.view(-1)[:self.q.shape[0] * k].view(-1, k),
                      self.d2.view(-1)[:self.q.shape[0] * k].view(-1, k), self.flags, p_valid=self.valid, q_index=self.q_index)
        return True


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    ran = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) if ran else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--side', type=int, default=448)            # 448^2 = 200 704 vertices
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--only', default=None, choices=[None, 'kernels'])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('profiles/knn.py measures on a GPU; none is visible (nothing is timed on the CPU)')
    f = open(args.out, 'a') if args.out else None
    lib = _lib.load()
    props = torch.cuda.get_device_properties(0)
    cus, ghz = int(props.multi_processor_count), float(getattr(props, 'clock_rate', 2400000)) / 1e6
    rate = cus * 64 * ghz * 1e9                                          # fp64 vector operations per second, non-FMA
    emit(f, what='device', name=props.name, cus=cus, clock_ghz=ghz, fp64_vector_ops_per_s=rate)
    rng = np.random.default_rng(0)
    mesh = LO.grid_mesh(args.side, 1, spacing=0.02)
    V = torch.from_numpy(mesh['vertices']).to(DEV)
    n = int(V.shape[0])
    unseen = rng.uniform(size=n) < 0.25
    some = torch.from_numpy(np.sort(rng.permutation(n)[:int(round(n * 60025 / 200704))])).to(DEV)
    cases = [Case('all x all', V, V),
             Case('60 025 x all', V[some].contiguous(), V),
             Case('fill: unseen x all, point_valid', V, V, q_index=torch.from_numpy(np.flatnonzero(unseen)).to(DEV),
                  valid=torch.from_numpy((~unseen).astype(np.uint8)).to(DEV))]
    if args.only == 'kernels':
        c = cases[0]
        c.nearest()
        for k in KS:
            c.knn(k)
        torch.cuda.synchronize()
        return
    for c in cases:
        calls = [('stin_nearest_f64', 0, c.nearest)] + [('stin_knn_f64', k, (lambda k=k: c.knn(k))) for k in KS]
        for _ in range(2):
            for _, _, fn in calls:
                fn()
        torch.cuda.synchronize()
        times = {(w, k): [] for w, k, _ in calls}
        for _ in range(args.reps):                                       # alternate: drift hits every arm alike
            for w, k, fn in calls:
                t = timed(fn)
                if t is not None:
                    times[(w, k)].append(t)
        assert int(c.flags.item()) == 0
        pairs = c.nq * int(c.p.shape[0])
        bound_ms = pairs * OPS_PER_PAIR / rate * 1e3
        med = {key: sorted(v)[len(v) // 2] for key, v in times.items() if v}
        for (w, k), v in times.items():
            if not v:
                emit(f, what=w, shape=c.name, note='not applicable: no validity mask in stin_nearest_f64')
                continue
            chunks = int(lib.stin_knn_chunks(c.nq, int(c.p.shape[0]), k)) if k else int(lib.stin_nearest_chunks(c.nq, int(c.p.shape[0])))
            emit(f, what=w, k=k, shape=c.name, Q=c.nq, P=int(c.p.shape[0]), chunks=chunks, ms_median=med[(w, k)], ms_min=min(v),
                 ms_all=v, pairs=pairs, valu_bound_ms=bound_ms, achieved_fraction=bound_ms / med[(w, k)],
                 ratio_to_nearest=med[(w, k)] / med[('stin_nearest_f64', 0)] if ('stin_nearest_f64', 0) in med else None,
                 ratio_to_k1=med[(w, k)] / med[('stin_knn_f64', 1)] if k else None)
    # ---- FrameColors.result() and result(knn=3), end to end (allocations, the index list, the flag read)
    fc = P.FrameColors(V, (500.0, 500.0, 319.5, 239.5))
    fc.count = torch.from_numpy(np.where(unseen, 0, rng.integers(1, 40, n)).astype(np.int32)).to(DEV)
    fc.sum = (torch.from_numpy(rng.integers(0, 16711680, (n, 3))).to(DEV) * fc.count[:, None].long()).contiguous()
    for knn in (0, 3):
        ts = []
        for i in range(2 + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            colors, _ = fc.result(knn=knn)
            torch.cuda.synchronize()
            if i >= 2:
                ts.append((time.perf_counter() - t0) * 1e3)
        emit(f, what='FrameColors.result', knn=knn, N=n, unseen=int(unseen.sum()), ms_median=sorted(ts)[len(ts) // 2], ms_all=ts)


if __name__ == '__main__':
    main()
