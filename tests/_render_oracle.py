"""numpy restatement of the render contract (include/stin_hip.h, "Render"; views.render_mesh): the yardstick of tests/test_render.py
and tests/test_render_gpu.py.

No golden file from the reference is possible: its visualiser (utils/ColorCompletionVisualizer.py) is an Open3D window, and Open3D is
not installed here.  So the contract is restated the OTHER way round from the kernels - per pose and per pixel, a gather over all
faces in vectorised fp64, the minimum key, then the resolve of the winners - sharing only the formulas (and
preprocessing.pose_extrinsics, the host step both sides start from).  The kernels have to reproduce it bit for bit.

* `render`     the contract -> Render(color_f32 [P, H, W, K], color_u8 [P, H, W, K], depth uint16 [P, H, W], face int32 [P, H, W],
               status): status carries STIN_RENDER_BAD_INDEX only (which faces take the large-face route is the kernels' business).
* `quantise`   float32 -> uint8 by the contract's rule.
* `look_at`, `orbit`, `wall`, `icosphere`, `render_walls`   the scene builders of the other oracles, passed on.
"""
import collections

import numpy as np

from surface_texture_inpainting_net_amd.preprocessing import pose_extrinsics
from _frames_oracle import render_sphere, render_walls  # noqa: F401
from _observers_oracle import look_at, orbit, wall  # noqa: F401
from _qem_oracle import icosphere  # noqa: F401

NO_FACE = np.uint64(0xFFFFFFFFFFFFFFFF)
BAD_INDEX = 1
CHUNK = 2048                                                              # pixels per gather: CHUNK x F doubles at a time

Render = collections.namedtuple('Render', 'color_f32 color_u8 depth face status')


def edge(px, py, qx, qy, rx, ry):
    return (qx - px) * (ry - py) - (qy - py) * (rx - px)


def screen(V, rt, cam):
    fx, fy, cx, cy = (np.float64(c) for c in cam)
    x, y, z = V[:, 0], V[:, 1], V[:, 2]
    with np.errstate(all='ignore'):
        xv = ((rt[0] * x + rt[1] * y) + rt[2] * z) + rt[3]
        yv = ((rt[4] * x + rt[5] * y) + rt[6] * z) + rt[7]
        zv = ((rt[8] * x + rt[9] * y) + rt[10] * z) + rt[11]
        X = fx * xv / zv + cx
        Y = fy * yv / zv + cy
    return X, Y, zv


def quantise(c32):
    t = np.asarray(c32, dtype=np.float32).astype(np.float64)
    with np.errstate(all='ignore'):
        t = np.where(t > 0.0, t, 0.0)                                     # !(t > 0) -> 0: NaN too
        t = np.where(t > 1.0, 1.0, t)
        return np.rint(t * 255.0).astype(np.uint8)


def millimetres(zp, depth_scale):
    with np.errstate(all='ignore'):
        mm = np.rint(zp * np.float64(depth_scale))
        ok = np.isfinite(mm) & (mm > 0.0) & (mm < 65535.0)
    return np.where(ok, mm, 0.0).astype(np.uint16)


def pose_keys(X, Y, Z, F, N, H, W, z_near):
    """The key of every pixel of one pose, uint64 [H W]: min over the faces of bits(float32(depth)) << 32 | face id."""
    keys = np.full(H * W, NO_FACE, dtype=np.uint64)
    if F.shape[0] == 0 or N == 0:
        return keys
    with np.errstate(all='ignore'):
        in_range = ((F >= 0) & (F < N)).all(axis=1)
        G = np.where(in_range[:, None], F, 0)
        ax, ay, az = X[G[:, 0]], Y[G[:, 0]], Z[G[:, 0]]
        bx, by, bz = X[G[:, 1]], Y[G[:, 1]], Z[G[:, 1]]
        cx, cy, cz = X[G[:, 2]], Y[G[:, 2]], Z[G[:, 2]]
        area2 = edge(ax, ay, bx, by, cx, cy)
        keep = in_range & ~((az < z_near) | (bz < z_near) | (cz < z_near))
        keep &= np.isfinite(ax) & np.isfinite(ay) & np.isfinite(bx) & np.isfinite(by) & np.isfinite(cx) & np.isfinite(cy)
        keep &= area2 != 0.0
        ids = np.flatnonzero(keep)
        if ids.size == 0:
            return keys
        ax, ay, az, bx, by, bz, cx, cy, cz, area2 = (a[ids][None, :] for a in (ax, ay, az, bx, by, bz, cx, cy, cz, area2))
        for s in range(0, H * W, CHUNK):
            pix = np.arange(s, min(s + CHUNK, H * W))
            px, py = (pix % W).astype(np.float64)[:, None], (pix // W).astype(np.float64)[:, None]   # centre of (row i, column j) = (j, i)
            wa = edge(bx, by, cx, cy, px, py)
            wb = edge(cx, cy, ax, ay, px, py)
            wc = edge(ax, ay, bx, by, px, py)
            cover = ((area2 > 0.0) & (wa >= 0.0) & (wb >= 0.0) & (wc >= 0.0)) | ((area2 < 0.0) & (wa <= 0.0) & (wb <= 0.0) & (wc <= 0.0))
            la, lb, lc = wa / area2, wb / area2, wc / area2
            zp = 1.0 / ((la / az + lb / bz) + lc / cz)
            depth = zp.astype(np.float32).view(np.uint32).astype(np.uint64)
            k = (depth << np.uint64(32)) | ids.astype(np.uint64)[None, :]
            keys[pix] = np.where(cover, k, NO_FACE).min(axis=1)
    return keys


def render(V, F, C, poses, camera, height, width, background=(0, 0, 0), z_near=0.01, depth_scale=1000.0):
    V = np.asarray(V, dtype=np.float64)
    V = V.reshape(-1, V.shape[-1])[:, :3]
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    C = np.asarray(C, dtype=np.float32)
    C = C.reshape(V.shape[0], C.shape[1] if C.ndim == 2 else 1)
    RT, valid = pose_extrinsics(poses)
    P, N, K, H, W = RT.shape[0], V.shape[0], C.shape[1], int(height), int(width)
    bg = np.asarray(background, dtype=np.float32).reshape(K)
    c32 = np.empty((P, H * W, K), dtype=np.float32)
    c32[:] = bg
    depth = np.zeros((P, H * W), dtype=np.uint16)
    face = np.full((P, H * W), -1, dtype=np.int32)
    status = BAD_INDEX if F.size and (((F < 0) | (F >= N)).any()) else 0
    for p in range(P):
        if not valid[p]:
            continue
        X, Y, Z = screen(V, RT[p], camera)
        keys = pose_keys(X, Y, Z, F, N, H, W, z_near)
        hit = np.flatnonzero(keys != NO_FACE)
        if hit.size == 0:
            continue
        f = (keys[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        ia, ib, ic = F[f, 0], F[f, 1], F[f, 2]
        px, py = (hit % W).astype(np.float64), (hit // W).astype(np.float64)
        with np.errstate(all='ignore'):
            ax, ay, az, bx, by, bz, cx, cy, cz = X[ia], Y[ia], Z[ia], X[ib], Y[ib], Z[ib], X[ic], Y[ic], Z[ic]
            area2 = edge(ax, ay, bx, by, cx, cy)
            la, lb, lc = edge(bx, by, cx, cy, px, py) / area2, edge(cx, cy, ax, ay, px, py) / area2, edge(ax, ay, bx, by, px, py) / area2
            zp = 1.0 / ((la / az + lb / bz) + lc / cz)
            qa, qb, qc = ((la / az) * zp)[:, None], ((lb / bz) * zp)[:, None], ((lc / cz) * zp)[:, None]
            val = (qa * C[ia].astype(np.float64) + qb * C[ib].astype(np.float64)) + qc * C[ic].astype(np.float64)
            c32[p, hit] = val.astype(np.float32)
        depth[p, hit] = millimetres(zp, depth_scale)
        face[p, hit] = f.astype(np.int32)
    return Render(c32.reshape(P, H, W, K), quantise(c32).reshape(P, H, W, K), depth.reshape(P, H, W), face.reshape(P, H, W), status)
