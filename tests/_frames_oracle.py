"""numpy restatement of the frame-colour contract (include/stin_hip.h, "Frame colours"; preprocessing.FrameColors): the yardstick of
tests/test_frames.py and tests/test_frames_gpu.py.

No golden file from the reference is possible: its texture_map_optimization.py hands the work to Open3D's colour-map pipeline, and
neither open3d nor cv2 is installed here.  So the contract is restated the OTHER way round from the kernel - per pose, vectorised
over all vertices, where the kernel runs per vertex over the poses - sharing only the formulas (and preprocessing.pose_extrinsics,
the host step both sides start from).  The kernels have to reproduce it bit for bit.

* `depth_edges`   raw uint16 [B, H, W] -> the depth-discontinuity mask uint8 [B, H, W].
* `accumulate`    -> (sum int64 [N, 3], count int32 [N], seen bool [N, P]).
* `finish`        -> (colours float32 [N, 3], observed bool [N]).
* `colors`        the three in a row -> (colours, count, seen, sum).
* `pack_seen`     bool [N, P] -> uint32 [N, ceil(P / 32)].
* `render_sphere`, `render_walls`   analytic z-depth of a sphere / of rectangles, uint16 millimetres, 0 where nothing is hit.
"""
import numpy as np

from surface_texture_inpainting_net_amd.preprocessing import pose_extrinsics

def truncated(raw, depth_scale, depth_trunc):
    raw = np.asarray(raw, dtype=np.uint16)
    return np.where(raw.astype(np.float64) / depth_scale > depth_trunc, 0, raw).astype(np.int64)


def depth_edges(raw, depth_scale=1000.0, depth_trunc=3.0, discontinuity_threshold=0.1, half_kernel=3):
    r = truncated(raw, depth_scale, depth_trunc)
    B, H, W = r.shape
    q = np.pad(r, ((0, 0), (1, 1), (1, 1)), mode='edge')                 # indices clamped to the image

    def at(di, dj):
        return q[:, 1 + di:1 + di + H, 1 + dj:1 + dj + W]
    gx = (at(-1, 1) + 2 * at(0, 1) + at(1, 1)) - (at(-1, -1) + 2 * at(0, -1) + at(1, -1))
    gy = (at(1, -1) + 2 * at(1, 0) + at(1, 1)) - (at(-1, -1) + 2 * at(-1, 0) + at(-1, 1))
    T = float(discontinuity_threshold) * float(depth_scale)
    edge0 = (gx * gx + gy * gy).astype(np.float64) > T * T
    k = int(half_kernel)
    z = np.pad(edge0, ((0, 0), (k, k), (k, k)), mode='constant')         # outside the image: not part of the window
    edge = np.zeros_like(edge0)
    for di in range(2 * k + 1):
        for dj in range(2 * k + 1):
            edge |= z[:, di:di + H, dj:dj + W]
    return edge.astype(np.uint8)


def project(cam, xv, yv, zv):
    fx, fy, cx, cy = (np.float64(c) for c in cam)
    return fx * xv / zv + cx, fy * yv / zv + cy


def accumulate(V, poses, color, color_camera, depth=None, depth_camera=None, bits=None, first_pose=0, num_poses=None, depth_scale=1000.0,
               depth_trunc=3.0, max_depth=2.5, depth_threshold=0.03, discontinuity_threshold=0.1, half_kernel=3, margin=10, z_near=0.01,
               into=None):
    """One batch (or the whole scan).  into = (sum, count, seen) of earlier batches; else fresh zeros with num_poses columns of seen."""
    V = np.asarray(V, dtype=np.float64)
    V = V.reshape(-1, V.shape[-1])[:, :3]
    color = np.asarray(color, dtype=np.uint8)
    RT, valid = pose_extrinsics(poses)
    B, N = RT.shape[0], V.shape[0]
    P = first_pose + B if num_poses is None else int(num_poses)
    if into is None:
        into = (np.zeros((N, 3), dtype=np.int64), np.zeros(N, dtype=np.int32), np.zeros((N, P), dtype=bool))
    total, count, seen = into
    assert (depth is None) != (bits is None)
    Hc, Wc = color.shape[1:3]
    depth_camera = color_camera if depth_camera is None else depth_camera
    if depth is not None:
        r = truncated(depth, depth_scale, depth_trunc)
        edge = depth_edges(depth, depth_scale, depth_trunc, discontinuity_threshold, half_kernel)
        Hd, Wd = r.shape[1:3]
    x, y, z = V[:, 0], V[:, 1], V[:, 2]
    for b in range(B):
        if not valid[b]:
            continue
        p, m = first_pose + b, RT[b]
        with np.errstate(all='ignore'):
            xv = ((m[0] * x + m[1] * y) + m[2] * z) + m[3]
            yv = ((m[4] * x + m[5] * y) + m[6] * z) + m[7]
            zv = ((m[8] * x + m[9] * y) + m[10] * z) + m[11]
            u, v = project(color_camera, xv, yv, zv)
            ok = ~(zv < z_near) & np.isfinite(u) & np.isfinite(v)
            if depth is not None:
                ud, vd = project(depth_camera, xv, yv, zv)
                ok &= np.isfinite(ud) & np.isfinite(vd)
                ui, vi = np.rint(ud), np.rint(vd)
                ok &= (ui >= 0) & (ui < Wd) & (vi >= 0) & (vi < Hd)
                ii, jj = np.where(ok, vi, 0).astype(np.int64), np.where(ok, ui, 0).astype(np.int64)
                rr = r[b, ii, jj]
                d = rr.astype(np.float64) / depth_scale
                ok &= (rr != 0) & ~(d > max_depth) & (edge[b, ii, jj] == 0) & (np.abs(zv - d) < depth_threshold)
            else:
                ok &= ((np.asarray(bits, dtype=np.uint32)[:, p >> 5] >> np.uint32(p & 31)) & np.uint32(1)).astype(bool)
            ok &= (u >= margin) & (u <= Wc - 1 - margin) & (v >= margin) & (v <= Hc - 1 - margin)
        ids = np.flatnonzero(ok)
        if ids.size == 0:
            continue
        u, v = u[ids], v[ids]
        x0, y0 = np.floor(u), np.floor(v)
        a, c = u - x0, v - y0
        x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, Wc - 1), np.minimum(y0 + 1, Hc - 1)
        img = color[b].astype(np.float64)
        w00, w01, w10, w11 = ((1.0 - a) * (1.0 - c))[:, None], (a * (1.0 - c))[:, None], ((1.0 - a) * c)[:, None], (a * c)[:, None]
        val = (w00 * img[y0, x0] + w01 * img[y0, x1]) + (w10 * img[y1, x0] + w11 * img[y1, x1])
        total[ids] += np.rint(val * 65536.0).astype(np.int64)
        count[ids] += 1
        seen[ids, p] = True
    return total, count, seen


def finish(total, count, fill=(0, 0, 0)):
    with np.errstate(all='ignore'):
        c = (total.astype(np.float64) / (count.astype(np.float64) * 16711680.0)[:, None]).astype(np.float32)
    observed = count > 0
    c[~observed] = np.asarray(fill, dtype=np.float32)
    return c, observed


def colors(V, poses, color, color_camera, fill=(0, 0, 0), **kw):
    total, count, seen = accumulate(V, poses, color, color_camera, **kw)
    return finish(total, count, fill)[0], count, seen, total


def pack_seen(seen):
    """bool [N, P] -> uint32 [N, ceil(P / 32)], bit (p & 31) of word (p >> 5)"""
    N, P = seen.shape
    words = (P + 31) // 32
    padded = np.zeros((N, words * 32), dtype=np.uint64)
    padded[:, :P] = seen
    return (padded.reshape(N, words, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


# ------------------------------------------------------------------------------------------------------------------- scenes
def rays(H, W, cam):
    """Direction (x, y, 1) in camera space through the centre of every pixel, [H, W, 3]."""
    fx, fy, cx, cy = cam
    ii, jj = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    return np.stack([(jj - cx) / fx, (ii - cy) / fy, np.ones_like(ii)], axis=2)


def millimetres(z):
    with np.errstate(all='ignore'):
        mm = np.rint(z * 1000.0)
    return np.where(np.isfinite(z) & (mm > 0) & (mm < 65535), mm, 0).astype(np.uint16)


def render_sphere(poses, H, W, cam, centre=(0.0, 0.0, 0.0), radius=1.0):
    """z-depth of the sphere's near surface seen from every (valid) pose, uint16 millimetres [P, H, W]; 0 where it is missed."""
    RT, valid = pose_extrinsics(poses)
    D = rays(H, W, cam)
    out = np.zeros((len(RT), H, W), dtype=np.uint16)
    for p in np.flatnonzero(valid):
        E = RT[p].reshape(3, 4)
        c = E[:, :3] @ np.asarray(centre, dtype=np.float64) + E[:, 3]
        dd, dc = (D * D).sum(axis=2), D @ c
        disc = dc * dc - dd * (c @ c - radius * radius)
        with np.errstate(all='ignore'):
            t = (dc - np.sqrt(disc)) / dd                                # D has z = 1: the ray parameter IS the z-depth
        out[p] = millimetres(np.where((disc >= 0) & (t > 0), t, np.inf))
    return out


def render_walls(poses, H, W, cam, walls):
    """walls: (origin, u, v, size) as for _observers_oracle.wall (u, v orthonormal): nearest z-depth per pixel, uint16 mm [P, H, W]."""
    RT, valid = pose_extrinsics(poses)
    D = rays(H, W, cam)
    out = np.zeros((len(RT), H, W), dtype=np.uint16)
    for p in np.flatnonzero(valid):
        E = RT[p].reshape(3, 4)
        best = np.full((H, W), np.inf)
        for origin, u, v, size in walls:
            o = E[:, :3] @ np.asarray(origin, dtype=np.float64) + E[:, 3]
            uc, vc = E[:, :3] @ np.asarray(u, dtype=np.float64), E[:, :3] @ np.asarray(v, dtype=np.float64)
            n = np.cross(uc, vc)
            with np.errstate(all='ignore'):
                t = (n @ o) / (D @ n)
            hit = t[:, :, None] * D - o
            inside = (np.abs(hit @ uc) <= size / 2) & (np.abs(hit @ vc) <= size / 2) & (t > 0)
            best = np.where(inside & (t < best), t, best)
        out[p] = millimetres(best)
    return out
