"""Segmentation objective on the GPU: the native forward (loss + confusion, csrc/stin_seg.hip) and backward against the aten
sequence they replace, plus two end-to-end figures of the segmentation experiment.  Run on an MI355X:

    python profiles/seg_objective.py [--out seg_objective.json] [--reps 30] [--quick]

1. Kernels at N = 200 k and 1 M, C = 21: native = stin_seg_ce_fwd_f32 (loss + confusion, one launch + the fixed-order sum)
   + stin_seg_ce_bwd_f32; aten = F.cross_entropy(weight, ignore_index=0) forward + backward, then argmax + bincount (the
   device part of ConfusionMatrixDCM.add).  Median of `reps` timings (device events) after warm-up; bytes = the compulsory
   traffic of the native pair (logits read twice, targets read twice, dlogits written once) and its share of 6.29 TB/s.
2. Training step at config_scmnet_segmentation.json (feature_number 9, 3 propagation steps, filters [64] * 4, 21 classes,
   4 collated crops, 4 levels) with the native Objective + ConfusionMatrix vs aten weighted cross entropy + the reference's
   per-step confusion update (.cpu().numpy() + np.bincount).  Host clock over `reps` steps ending in a synchronise.
3. One evaluation pass over a 200 k-vertex scene through original_index_traces: native rows= path vs output[traces] +
   aten cross entropy + the reference's confusion update.
--quick: fewer repetitions (the rocprofv3 --kernel-trace --stats run).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from surface_texture_inpainting_net_amd import scene_io, segmentation as seg  # noqa: E402
from surface_texture_inpainting_net_amd.data import collate  # noqa: E402
from surface_texture_inpainting_net_amd.synthetic import make_synthetic_mesh  # noqa: E402

DEV = 'cuda:0'
C = 21
HBM = 6.29e12


def _median_ms(fn, reps, warm=5):
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


def _ref_conf_update(conf, out, labels):
    """ConfusionMatrixDCM.add as the reference runs it every step: max on the device, .cpu().numpy(), np.bincount."""
    _, pred = out.detach().max(1)
    p, t = pred.cpu().numpy(), labels.cpu().numpy()
    conf += np.bincount(p + C * t, minlength=C * C).reshape(C, C)


def kernels(reps):
    res = []
    w = (torch.rand(C, generator=torch.Generator().manual_seed(0)) * 70).to(DEV)
    w[0] = 0.0
    for N in (200_000, 1_000_000):
        g = torch.Generator().manual_seed(N)
        z = (torch.randn(N, C, generator=g) * 2).to(DEV).requires_grad_()
        y = torch.randint(0, C, (N,), generator=g).to(DEV)
        crit = seg.CrossEntropyLoss(w, ignore_index=0)
        cm = seg.ConfusionMatrix(C, DEV)

        def native():
            crit(z, y, confusion=cm).backward()

        def aten():
            F.cross_entropy(z, y, weight=w, ignore_index=0).backward()
            torch.bincount(z.detach().argmax(1) + C * y, minlength=C * C)

        def native_fwd():
            with torch.no_grad():
                crit(z.detach(), y, confusion=cm)

        # the two sequences alternate so that both see the same clocks / neighbours
        t_n, t_a, t_f = [], [], []
        for _ in range(3):
            t_n.append(_median_ms(native, reps))
            t_a.append(_median_ms(aten, reps))
            t_f.append(_median_ms(native_fwd, reps))
        z.grad = None
        nat = statistics.median(t[0] for t in t_n)
        at = statistics.median(t[0] for t in t_a)
        fw = statistics.median(t[0] for t in t_f)
        nbytes = 3 * N * C * 4 + 2 * N * 8
        # numerics of the timed problem: native vs aten (fp32) loss and gradient
        z.grad = None
        ln = crit(z, y)
        ln.backward()
        gn = z.grad.clone()
        z.grad = None
        la = F.cross_entropy(z, y, weight=w, ignore_index=0)
        la.backward()
        ga = z.grad.clone()
        z.grad = None
        cm.reset()
        cm.add(z.detach(), y)
        want = torch.bincount(z.detach().argmax(1) + C * y, minlength=C * C).reshape(C, C)
        res.append(dict(N=N, C=C, native_fwd_bwd_ms=nat, aten_fwd_bwd_argmax_bincount_ms=at, native_fwd_only_ms=fw,
                        speedup=at / nat, native_bytes=nbytes, native_TBps=nbytes / (nat * 1e-3) / 1e12,
                        native_frac_of_6p29=nbytes / (nat * 1e-3) / HBM,
                        loss_rel_diff_vs_aten=abs(float(ln) - float(la)) / abs(float(la)),
                        grad_maxabs_diff_over_scale=float((gn - ga).abs().max() / ga.abs().max()),
                        confusion_equal=bool(torch.equal(cm.matrix, want)),
                        spread_ms=dict(native=[t[1:] for t in t_n], aten=[t[1:] for t in t_a])))
        print(json.dumps(res[-1]), flush=True)
    return res


def _crop(i, n):
    s = make_synthetic_mesh(n, 4, seed=100 + i, dilations=())
    labels = torch.from_numpy(np.random.default_rng(i).integers(0, C, size=s.x.shape[0]))
    return scene_io.label_sample_from_tensors(scene_io.label_graph_tensors(s, labels), 4, True)


def train_step(reps, crop_vertices):
    from surface_texture_inpainting_net_amd.singleconvmeshnet import SingleConvMeshNet
    from surface_texture_inpainting_net_amd.train_step import TrainStep
    batch = collate([_crop(i, crop_vertices) for i in range(4)]).to(DEV)
    w = (torch.rand(C, generator=torch.Generator().manual_seed(1)) * 70).to(DEV)
    w[0] = 0.0
    out = {}
    for kind in ('native', 'aten', 'native', 'aten'):
        torch.manual_seed(49)
        net = SingleConvMeshNet(9, 3, [64] * 4, num_classes=C).to(DEV)
        if kind == 'native':
            cm = seg.ConfusionMatrix(C, DEV)
            step = TrainStep(net, lr=1e-3, loss_fn=seg.Objective(seg.CrossEntropyLoss(w, ignore_index=0), cm))
            run = lambda: step(batch)  # noqa: E731
        else:
            conf = np.zeros((C, C), dtype=np.int64)

            def loss_fn(m, s):
                o = m(s)
                loss_fn.out = o
                return F.cross_entropy(o, s.labels, weight=w, ignore_index=0)
            step = TrainStep(net, lr=1e-3, loss_fn=loss_fn)

            def run():
                loss = step(batch)
                _ref_conf_update(conf, loss_fn.out, batch.labels)
                float(loss)                                     # loss.item() of the reference's loop
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            run()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / reps
        step.finish()
        out.setdefault(kind, []).append(ms)
        step.close()
    r = dict(vertices=int(batch.x.shape[0]), crops=4, native_step_ms=min(out['native']), aten_step_ms=min(out['aten']),
             runs_ms=out)
    print(json.dumps(r), flush=True)
    return r


def eval_pass(reps):
    from surface_texture_inpainting_net_amd.singleconvmeshnet import SingleConvMeshNet
    s = make_synthetic_mesh(200_000, 4, seed=7, dilations=())
    n0 = s.x.shape[0]
    rng = np.random.default_rng(7)
    orig = np.concatenate([rng.permutation(n0), rng.integers(0, n0, size=n0 // 3)])
    saved = scene_io.label_graph_tensors(s, torch.from_numpy(rng.integers(0, C, size=orig.size)), torch.from_numpy(orig))
    b = scene_io.label_sample_from_tensors(saved, 4, False).to(DEV)
    torch.manual_seed(49)
    net = SingleConvMeshNet(9, 3, [64] * 4, num_classes=C).to(DEV).eval()
    w = (torch.rand(C, generator=torch.Generator().manual_seed(1)) * 70).to(DEV)
    crit = seg.CrossEntropyLoss(w, ignore_index=0)
    cm = seg.ConfusionMatrix(C, DEV)
    conf = np.zeros((C, C), dtype=np.int64)

    def native():
        with torch.no_grad():
            out = net(b)
            loss = crit(out, b.labels, rows=b.original_index_traces, confusion=cm)
        return float(loss)

    def aten():
        with torch.no_grad():
            out = net(b)
            full = out[b.original_index_traces]
            loss = F.cross_entropy(full, b.labels, weight=w, ignore_index=0)
            _ref_conf_update(conf, full, b.labels)
        return float(loss)

    def timed(fn):
        fn()
        fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    tn, ta = [], []
    for _ in range(2):
        tn.append(timed(native))
        ta.append(timed(aten))
    ln, la = native(), aten()
    r = dict(level0_vertices=int(n0), original_vertices=int(orig.size), native_eval_ms=min(tn), aten_eval_ms=min(ta),
             loss_native=ln, loss_aten=la, runs_ms=dict(native=tn, aten=ta))
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='write the results as one JSON file here (they are always printed)')
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--crop-vertices', type=int, default=20_000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    reps = 5 if a.quick else a.reps
    res = dict(device=torch.cuda.get_device_name(0), kernels=kernels(reps))
    if not a.quick:
        res['train_step'] = train_step(max(20, reps // 2), a.crop_vertices)
        res['eval_pass'] = eval_pass(max(10, reps // 3))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
