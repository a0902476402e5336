"""Timing of the image resize (csrc/stin_resize.hip, preprocessing.resize_u8 / resize_pool_u8) on one GPU, with the route a user
would write with torch today on the same inputs in the same run as the yardstick (there is no parent implementation).

    python profiles/resize.py [--out FILE] [--reps 15] [--frames 64] [--images 256]

* LINEAR  [frames, 968, 1296, 3] -> 480 x 640: the colour frames of a scan to the depth size, one launch for the batch.
* AREA    `images` images of 512 x 768 x 3 at odd byte offsets of one pool -> 256 x 384 each, one launch (the image-graph loader).
* the torch route on the same bytes: permute to [B, C, H, W], .float(), F.interpolate (bilinear with align_corners=False, or
  area), round, clamp, .to(uint8), permute back and make contiguous.
HIP events around the launch alone (the job table uploaded and the output allocated beforehand) and around the whole Python call;
three warm-up calls, the median of `reps` calls, the arms alternating inside every repetition.  Beside each time the byte bound:
(bytes read + bytes written) over the measured streaming rate of the chip's HBM (6.29 TB/s, float4 copy), and the achieved fraction.
The results are compared once: the kernel's against tests/_resize_oracle.py (equal) and torch's against the kernel's (max difference).
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _resize_oracle as RO  # noqa: E402
from surface_texture_inpainting_net_amd import _lib, preprocessing as P  # noqa: E402
from surface_texture_inpainting_net_amd.plan import _ptr, _stream  # noqa: E402

DEV = 'cuda:0'
HBM_BYTES_PER_S = 6.29e12


def emit(f, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if f is not None:
        f.write(line + '\n')
        f.flush()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def torch_route(batch, h, w, mode):
    x = batch.permute(0, 3, 1, 2).float()
    y = F.interpolate(x, size=(h, w), mode='bilinear', align_corners=False) if mode == 'linear' else F.interpolate(x, size=(h, w), mode='area')
    return y.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


class Launch:
    """The bare stin_resize_u8 call on buffers made beforehand."""

    def __init__(self, pool, jobs, out_bytes, mode):
        self.pool, self.n, self.mode = pool, len(jobs), _lib.CONSTANTS[P.RESIZE_MODES[mode]]
        self.table = torch.tensor(jobs, dtype=torch.int64).to(DEV)
        self.out = torch.empty(out_bytes, dtype=torch.uint8, device=DEV)
        self.lib = _lib.load()

    def __call__(self):
        _lib.check(self.lib.stin_resize_u8(_ptr(self.pool), self.pool.numel(), _ptr(self.out), self.out.numel(), _ptr(self.table), self.n,
                                           3, self.mode, _stream(self.pool)), 'stin_resize_u8')
        return self.out


def measure(f, name, arms, reps, bytes_moved, **info):
    for _ in range(3):
        for _, fn in arms:
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k, _ in arms}
    for _ in range(reps):
        for k, fn in arms:
            times[k].append(timed(fn)[0])
    bound_ms = bytes_moved / HBM_BYTES_PER_S * 1e3
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    for k, v in times.items():
        emit(f, what=name, arm=k, ms_median=med[k], ms_min=min(v), ms_max=max(v), bytes_read_and_written=bytes_moved, byte_bound_ms=bound_ms,
             achieved_fraction_of_byte_bound=bound_ms / med[k], ratio_to_kernel=med[k] / med['kernel'], **info)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--images', type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('profiles/resize.py measures on a GPU; none is visible (nothing is timed on the CPU)')
    f = open(args.out, 'a') if args.out else None
    props = torch.cuda.get_device_properties(0)
    emit(f, what='device', name=props.name, cus=int(props.multi_processor_count),
         clock_ghz=float(getattr(props, 'clock_rate', 0)) / 1e6, hbm_bytes_per_s_assumed=HBM_BYTES_PER_S)
    g = torch.Generator(device=DEV).manual_seed(0)

    # ---- frames: LINEAR, a uniform batch
    B, H, W, h, w = args.frames, 968, 1296, 480, 640
    frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=DEV, generator=g)
    jobs = [(b * H * W * 3, H, W, b * h * w * 3, h, w) for b in range(B)]
    launch = Launch(frames.view(-1), jobs, B * h * w * 3, 'linear')
    got = P.resize_u8(frames, (h, w))
    assert torch.equal(got.view(-1), launch())
    assert got[B - 1].cpu().numpy().tobytes() == RO.linear(frames[B - 1].cpu().numpy(), h, w).tobytes()
    diff = (torch_route(frames[:2], h, w, 'linear').int() - got[:2].int()).abs()
    emit(f, what='frames LINEAR: torch route against the kernel', max_abs_difference=int(diff.max()), differing_fraction=float((diff > 0).float().mean()))
    measure(f, 'frames LINEAR %d x [%d, %d, 3] -> %d x %d' % (B, H, W, h, w),
            [('kernel', launch), ('resize_u8', lambda: P.resize_u8(frames, (h, w))), ('torch', lambda: torch_route(frames, h, w, 'linear'))],
            args.reps, B * (H * W + h * w) * 3, frames=B, per_frame_note='ms_median / frames is the time per frame')

    # ---- images: AREA, ragged offsets
    del frames, launch, got
    n, H, W, h, w = args.images, 512, 768, 256, 384
    jobs, at, out_at = [], 0, 0
    for i in range(n):
        at += 1 + (i % 13)                                               # odd gaps: no image starts aligned
        jobs.append((at, H, W, out_at, h, w))
        at += H * W * 3
        out_at += h * w * 3
    pool = torch.randint(0, 256, (at,), dtype=torch.uint8, device=DEV, generator=g)
    launch = Launch(pool, jobs, out_at, 'area')
    got = P.resize_pool_u8(pool, jobs, out_at, 3, 'area')
    assert torch.equal(got, launch())
    so = jobs[n - 1][0]
    last = pool[so:so + H * W * 3].view(H, W, 3)
    assert got[jobs[n - 1][3]:].cpu().numpy().tobytes() == RO.area(last.cpu().numpy(), h, w).tobytes()
    batch = torch.stack([pool[j[0]:j[0] + H * W * 3].view(H, W, 3) for j in jobs])      # what the torch route needs first (not timed)
    diff = (torch_route(batch[:2], h, w, 'area').int() - got[:2 * h * w * 3].view(2, h, w, 3).int()).abs()
    emit(f, what='images AREA: torch route against the kernel', max_abs_difference=int(diff.max()), differing_fraction=float((diff > 0).float().mean()))
    measure(f, 'images AREA %d x [%d, %d, 3] -> %d x %d, ragged pool' % (n, H, W, h, w),
            [('kernel', launch), ('resize_pool_u8', lambda: P.resize_pool_u8(pool, jobs, out_at, 3, 'area')),
             ('torch', lambda: torch_route(batch, h, w, 'area'))],
            args.reps, n * (H * W + h * w) * 3, images=n)


if __name__ == '__main__':
    main()
