"""Wall time of the view metrics (csrc/stin_view_metrics.hip: views.view_metrics) on one GPU, beside the bytes the pass must read.

    python profiles/view_metrics.py [--out FILE] [--poses 128] [--height 480] [--width 640] [--channels 3] [--reps 5] [--calls 20]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python profiles/view_metrics.py --traced

Images: synthetic.  `b` is a smooth colour field of the pixel position, different for every pose; `a` is `b` plus noise inside a
disc (the inpainted region) and equal to it elsewhere; `covered` is a larger disc (the mesh's silhouette) and `region` the
inner one.  What the kernel does per window does not depend on the pixel values, only on the masks: a window that is not counted
skips the fp64 evaluation, so the masked call is the cheaper one.
Every time is wall clock (time.perf_counter between device synchronisations) around `calls` back-to-back calls of the Python
function a user makes - one call is too short a window - after one warm-up round; the median of `reps` rounds, per call.
* view_metrics without masks, with `covered` only, with both masks; the derived figures are included (a few small torch kernels);
* the same for the bare library call (no torch kernels), which is the kernel plus the memset of the table;
* the compulsory bytes: P H W (2 K + masks) read once, and the time they take at the 6.3 TB/s a streaming read reaches on this
  part; the halo re-reads (26 x 42 staged for 16 x 32 owned: 2.1 x) are served by L2 and are not in that figure.
--traced makes three calls of each kind for a kernel trace.  Times are recorded, not gated.  Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = 'cuda:0'
STREAM_BYTES_PER_S = 6.3e12                                # what a 16-byte-per-lane streaming read reaches on an MI355X


def emit(f, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if f is not None:
        f.write(line + '\n')
        f.flush()


def wall(fn, reps, calls):
    ts, out = [], None
    for i in range(1 + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            out = fn()
        torch.cuda.synchronize()
        if i >= 1:
            ts.append((time.perf_counter() - t0) * 1e3 / calls)
    return out, statistics.median(ts), ts


def scene(P, H, W, K):
    g = torch.Generator(device=DEV).manual_seed(0)
    y = torch.arange(H, device=DEV, dtype=torch.float32).view(1, H, 1, 1)
    x = torch.arange(W, device=DEV, dtype=torch.float32).view(1, 1, W, 1)
    p = torch.arange(P, device=DEV, dtype=torch.float32).view(P, 1, 1, 1)
    k = torch.arange(K, device=DEV, dtype=torch.float32).view(1, 1, 1, K)
    field = 0.5 + 0.25 * torch.sin(0.02 * x + 0.3 * p + k) + 0.25 * torch.cos(0.015 * y - 0.2 * p + 2.0 * k)
    r2 = ((y - H / 2) / (H / 2)) ** 2 + ((x - W / 2) / (W / 2)) ** 2
    covered = (r2 < 0.9).expand(P, H, W, 1)[..., 0].contiguous()
    region = (r2 < 0.25).expand(P, H, W, 1)[..., 0].contiguous()
    b = (field * 255.0).round().clamp(0, 255).to(torch.uint8)
    noise = 0.1 * torch.randn(P, H, W, K, device=DEV, generator=g)
    a = ((field + noise * region[..., None]) * 255.0).round().clamp(0, 255).to(torch.uint8)
    return a, b, covered.view(torch.uint8), region.view(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--poses', type=int, default=128)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--channels', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--traced', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('profiles/view_metrics.py measures on a GPU; none is visible')
    from surface_texture_inpainting_net_amd import _lib, views
    from surface_texture_inpainting_net_amd.plan import _ptr, _stream
    f = open(args.out, 'a') if args.out else None
    props = torch.cuda.get_device_properties(0)
    emit(f, what='device', name=props.name, cus=int(props.multi_processor_count), lib=_lib.LIB_PATH)
    P, H, W, K = args.poses, args.height, args.width, args.channels
    a, b, covered, region = scene(P, H, W, K)
    emit(f, what='scene', poses=P, height=H, width=W, channels=K, covered_share=float(covered.double().mean()),
         region_share=float(region.double().mean()), windows_per_pose=(H - 10) * (W - 10), workgroups=P * ((H + 15) // 16) * ((W + 31) // 32))
    lib = _lib.load()
    table = torch.empty(P, 5, dtype=torch.int64, device=DEV)

    def bare(cov, reg):
        _lib.check(lib.stin_view_metrics_u8(_ptr(a), _ptr(b), _ptr(cov), _ptr(reg), P, H, W, K, _ptr(table), 0, 0, _stream(a)))
        return table
    kinds = (('no masks', None, None), ('covered', covered, None), ('covered and region', covered, region))
    for name, cov, reg in kinds:
        if args.traced:
            for _ in range(3):
                views.view_metrics(a, b, cov, reg)
            torch.cuda.synchronize()
            continue
        m, ms, ts = wall(lambda: views.view_metrics(a, b, cov, reg), args.reps, args.calls)
        _, ms_bare, ts_bare = wall(lambda: bare(cov, reg), args.reps, args.calls)
        assert torch.equal(table, m.table)
        use = torch.ones(P, H, W, dtype=torch.bool, device=DEV)
        for t in (cov, reg):
            if t is not None:
                use &= t != 0
        d = (a.long() - b.long()) * use[..., None]
        assert torch.equal(m.table[:, 0], use.sum(dim=(1, 2))) and torch.equal(m.table[:, 1], d.abs().sum(dim=(1, 2, 3)))
        assert torch.equal(m.table[:, 2], (d * d).sum(dim=(1, 2, 3)))      # the pixel sums, against torch
        nbytes = P * H * W * (2 * K + (cov is not None) + (reg is not None))
        total = m.total()
        emit(f, what='view_metrics', masks=name, ms_per_call=ms, ms_all=ts, ms_per_call_library_only=ms_bare, ms_all_library_only=ts_bare,
             us_per_pose=ms_bare * 1e3 / P, compulsory_bytes=nbytes, ms_of_those_bytes_at_6_3_TB_s=nbytes / STREAM_BYTES_PER_S * 1e3,
             times_the_byte_bound=ms_bare / (nbytes / STREAM_BYTES_PER_S * 1e3), windows_counted=total['n_win'], psnr=total['psnr'],
             ssim=total['ssim'])


if __name__ == '__main__':
    main()
