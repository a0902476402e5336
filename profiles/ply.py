"""Wall time of reading a PLY mesh file (scene_io.read_ply, csrc/stin_ply.hip) on one GPU: the device decode, the host decode and
the test suite's structured-dtype parse plus upload, on a generated file in the ScanNet layout.

    python profiles/ply.py [--out FILE] [--vertices 1000000] [--faces 2000000] [--reps 7] [--dir DIR]

File: float x y z, uchar red green blue alpha (16-byte vertex records), `list uchar int vertex_indices` (13-byte face records),
binary little endian - about 16 N + 13 F bytes, 42 MB at the defaults; the device path writes 24 N + 24 N + 3 N + 8 N + 24 F bytes
of tensors.  It is written once and read back before the first measurement, so every read comes from the page cache.  Every time
is wall clock (time.perf_counter between device synchronisations) around the Python call a user makes: one warm-up call, then the
median of `reps`.  The kernels' share of the device path comes from hip events around the two decode launches alone, on buffers
that are already on the device (median of `reps`), beside the time of the upload alone.  Times are recorded, not gated.  Prints
one JSON line per measurement."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
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


def write_scannet_layout(path, n, nf, seed=0):
    rng = np.random.default_rng(seed)
    vert = np.empty(n, dtype=[('xyz', '<f4', 3), ('rgba', 'u1', 4)])
    vert['xyz'] = rng.standard_normal((n, 3)).astype(np.float32)
    vert['rgba'] = rng.integers(0, 256, (n, 4)).astype(np.uint8)
    face = np.empty(nf, dtype=[('n', 'u1'), ('ids', '<i4', 3)])
    face['n'], face['ids'] = 3, rng.integers(0, n, (nf, 3))
    header = ('ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n'
              'property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nelement face %d\n'
              'property list uchar int vertex_indices\nend_header\n' % (n, nf))
    with open(path, 'wb') as out:
        out.write(header.encode('ascii') + vert.tobytes() + face.tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--vertices', type=int, default=1000000)
    ap.add_argument('--faces', type=int, default=2000000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--dir', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('profiles/ply.py measures on a GPU; none is visible')
    import _ply_oracle as PO
    from surface_texture_inpainting_net_amd import _lib, scene_io as IO
    from surface_texture_inpainting_net_amd.plan import _ptr, _stream
    f = open(args.out, 'a') if args.out else None
    props = torch.cuda.get_device_properties(0)
    emit(f, what='device', name=props.name, cus=int(props.multi_processor_count), lib=_lib.LIB_PATH)
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        path = os.path.join(tmp, 'scan.ply')
        write_scannet_layout(path, args.vertices, args.faces)
        size = os.path.getsize(path)
        blob = open(path, 'rb').read()                                     # the file is in the page cache from here on
        emit(f, what='file', vertices=args.vertices, faces=args.faces, bytes=size)
        dev_mesh, ms_dev, ts = wall(lambda: IO.read_ply(path, device=DEV, decode='device'), args.reps)
        emit(f, what="read_ply(decode='device')", ms_median=ms_dev, ms_all=ts)
        host_mesh, ms_host, ts = wall(lambda: IO.read_ply(path, device=DEV, decode='host'), args.reps)
        emit(f, what="read_ply(decode='host')", ms_median=ms_host, ms_all=ts)

        def restated():                                                    # the test suite's parse: structured dtypes, then uploads
            m = PO.decode(open(path, 'rb').read())
            flat = dict(m, alpha=m['vertex_properties']['alpha'])
            return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in flat.items() if isinstance(v, np.ndarray)}
        ref, ms_np, ts = wall(restated, args.reps)
        emit(f, what='tests/_ply_oracle.decode (structured dtypes) + upload', ms_median=ms_np, ms_all=ts)
        same = all(torch.equal(dev_mesh[k], host_mesh[k]) and torch.equal(dev_mesh[k], ref[k]) for k in ('vertices', 'faces', 'colors', 'colors_u8'))
        same = same and torch.equal(dev_mesh['vertex_properties']['alpha'], ref['alpha'])
        emit(f, what='equal', device_host_structured=bool(same))
        # ---- the parts of the device path
        _, ms_read, ts = wall(lambda: np.fromfile(path, dtype=np.uint8), args.reps)
        emit(f, what='np.fromfile (page cache)', ms_median=ms_read, ms_all=ts)
        raw = np.fromfile(path, dtype=np.uint8)
        buf, ms_up, ts = wall(lambda: torch.from_numpy(raw).to(DEV), args.reps)
        emit(f, what='upload of the file bytes (pageable)', ms_median=ms_up, ms_all=ts, GBps=size / ms_up / 1e6)
        header = IO.read_ply_header(blob[:4096])
        vertex, face = IO._ply_plan(header)
        layout, K = IO._ply_device_layout(size, header, vertex, face)
        lib = _lib.load()
        n, nf = args.vertices, args.faces
        v = torch.empty(n, 3, dtype=torch.float64, device=DEV)
        c = torch.empty(n, 3, dtype=torch.float64, device=DEV)
        u = torch.empty(n, 3, dtype=torch.uint8, device=DEV)
        a = torch.empty(n, dtype=torch.int64, device=DEV)
        faces = torch.empty(nf, 3, dtype=torch.int64, device=DEV)
        status = torch.empty(4, dtype=torch.int64, device=DEV)
        C = _lib.CONSTANTS
        rows = [(4 * i, C['STIN_PLY_FLOAT32'], _ptr(v), C['STIN_PLY_TO_F64'], 3, i) for i in range(3)]
        rows += [(12 + i, C['STIN_PLY_UINT8'], _ptr(c), C['STIN_PLY_TO_UNORM_F64'], 3, i) for i in range(3)]
        rows += [(12 + i, C['STIN_PLY_UINT8'], _ptr(u), C['STIN_PLY_TO_U8'], 3, i) for i in range(3)]
        rows += [(15, C['STIN_PLY_UINT8'], _ptr(a), C['STIN_PLY_TO_I64'], 1, 0)]
        table = (ctypes.c_int64 * (6 * len(rows)))(*[w for r in rows for w in r])
        kernel_ms = {'stin_ply_decode': [], 'stin_ply_faces': []}
        for i in range(1 + args.reps):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            _lib.check(lib.stin_ply_decode(_ptr(buf), size, layout['vertex'][0], 16, n, 0, table, len(rows), _stream(buf)))
            e[1].record()
            _lib.check(lib.stin_ply_faces(_ptr(buf), size, layout['face'][0], 13, nf, 0, 0, C['STIN_PLY_UINT8'], C['STIN_PLY_INT32'], 3, n,
                                          _ptr(faces), _ptr(status), _stream(buf)))
            e[2].record()
            torch.cuda.synchronize()
            if i >= 1:
                kernel_ms['stin_ply_decode'].append(e[0].elapsed_time(e[1]))
                kernel_ms['stin_ply_faces'].append(e[1].elapsed_time(e[2]))
        assert status.tolist()[0] == 0 and torch.equal(v, dev_mesh['vertices']) and torch.equal(faces, dev_mesh['faces'])
        kd, kf = statistics.median(kernel_ms['stin_ply_decode']), statistics.median(kernel_ms['stin_ply_faces'])
        moved_d, moved_f = 16 * n + (24 + 24 + 3 + 8) * n, 13 * nf + 24 * nf
        emit(f, what='kernels (hip events)', decode_ms=kd, faces_ms=kf, decode_GBps=moved_d / kd / 1e6, faces_GBps=moved_f / kf / 1e6,
             share_of_device_path=(kd + kf) / ms_dev, decode_ms_all=kernel_ms['stin_ply_decode'], faces_ms_all=kernel_ms['stin_ply_faces'])


if __name__ == '__main__':
    main()
