"""numpy restatement of the colour-map optimisation contract (include/stin_hip.h, "Colour-map optimisation";
preprocessing.optimize_poses_rigid): the yardstick of tests/test_colormap.py and tests/test_colormap_gpu.py.

Restated the OTHER way round from the kernels - per pose, vectorised over all vertices, the terms of every pair laid out as an
array [N, 28] and summed by array operations in the contract's order (lane sums, halving tree, tiles ascending), where the kernel
runs per vertex over the poses and folds in registers, LDS and shuffles.  It shares the formulas and preprocessing.pose_extrinsics,
the host step both sides start from.  The kernels have to reproduce it byte for byte.

* `gradients`     colour uint8 [B, H, W, 3] -> int32 [B, H, W, 4] = (G, gx, gy, 0).
* `accumulate`    the bits mode of stin_frames_accumulate_f64 at given extrinsics -> (sum int64 [N, 3], count int32 [N]).
* `proxy`         sum, count -> fp64 [N].
* `normal`        -> (rows fp64 [B, 28], counts int32 [B]).
* `increment`     x [6] -> D(x) [4, 4].
* `update`        one Gauss-Newton update of the extrinsics on the host.
* `optimize`      the whole iteration -> (poses [P, 4, 4], info), as preprocessing.optimize_poses_rigid returns them.
"""
import numpy as np

from surface_texture_inpainting_net_amd.preprocessing import pose_extrinsics

U = 4                                                                  # STIN_COLORMAP_U
LANES = 256
ROW = 28
NOT_FREE, INVALID, FEW_PAIRS, SINGULAR = 1, 2, 4, 8


def gradients(color):
    color = np.asarray(color, dtype=np.uint8)
    c = color.astype(np.int32)
    G = 299 * c[..., 0] + 587 * c[..., 1] + 114 * c[..., 2]
    B, H, W = G.shape
    q = np.pad(G, ((0, 0), (1, 1), (1, 1)), mode='edge')                 # indices clamped to the image

    def at(di, dj):
        return q[:, 1 + di:1 + di + H, 1 + dj:1 + dj + W]
    gx = (at(-1, 1) + 2 * at(0, 1) + at(1, 1)) - (at(-1, -1) + 2 * at(0, -1) + at(1, -1))
    gy = (at(1, -1) + 2 * at(1, 0) + at(1, 1)) - (at(-1, -1) + 2 * at(-1, 0) + at(-1, 1))
    return np.stack([G, gx, gy, np.zeros_like(G)], axis=3).astype(np.int32)


def _pairs(V, m, valid, p, camera, bits, z_near, margin, H, W):
    """The pair set of one pose -> (ids, xv, yv, zv, u, v) of the contributing vertices."""
    none = np.zeros(0, dtype=np.int64)
    if not valid:
        return none, none, none, none, none, none
    fx, fy, cx, cy = (np.float64(c) for c in camera)
    x, y, z = V[:, 0], V[:, 1], V[:, 2]
    with np.errstate(all='ignore'):
        xv = ((m[0] * x + m[1] * y) + m[2] * z) + m[3]
        yv = ((m[4] * x + m[5] * y) + m[6] * z) + m[7]
        zv = ((m[8] * x + m[9] * y) + m[10] * z) + m[11]
        u, v = fx * xv / zv + cx, fy * yv / zv + cy
        ok = ((np.asarray(bits, dtype=np.uint32)[:, p >> 5] >> np.uint32(p & 31)) & np.uint32(1)).astype(bool)
        ok &= ~(zv < z_near) & np.isfinite(u) & np.isfinite(v)
        ok &= (u >= margin) & (u <= W - 1 - margin) & (v >= margin) & (v <= H - 1 - margin)
    ids = np.flatnonzero(ok)
    return ids, xv[ids], yv[ids], zv[ids], u[ids], v[ids]


def _sample(img, u, v):
    """img fp64 [H, W, K]; the bilinear expression of "Frame colours" -> [n, K]"""
    H, W = img.shape[:2]
    x0, y0 = np.floor(u), np.floor(v)
    a, c = u - x0, v - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    w00, w01, w10, w11 = ((1.0 - a) * (1.0 - c))[:, None], (a * (1.0 - c))[:, None], ((1.0 - a) * c)[:, None], (a * c)[:, None]
    return (w00 * img[y0, x0] + w01 * img[y0, x1]) + (w10 * img[y1, x0] + w11 * img[y1, x1])


def accumulate(V, RT, valid, color, camera, bits, z_near=0.01, margin=10, first_pose=0):
    V = np.asarray(V, dtype=np.float64)[:, :3]
    color = np.asarray(color, dtype=np.uint8)
    H, W = color.shape[1:3]
    total, count = np.zeros((V.shape[0], 3), dtype=np.int64), np.zeros(V.shape[0], dtype=np.int32)
    for b in range(RT.shape[0]):
        ids, _, _, _, u, v = _pairs(V, RT[b], valid[b], first_pose + b, camera, bits, z_near, margin, H, W)
        if ids.size == 0:
            continue
        total[ids] += np.rint(_sample(color[b].astype(np.float64), u, v) * 65536.0).astype(np.int64)
        count[ids] += 1
    return total, count


def proxy(total, count):
    num = 299 * total[:, 0] + 587 * total[:, 1] + 114 * total[:, 2]
    with np.errstate(all='ignore'):
        out = num.astype(np.float64) / (count.astype(np.float64) * 16711680000.0)
    return np.where(count > 0, out, 0.0)


def ordered_sum(T):
    """T [N, K]: the terms of every vertex (zeros where a pair does not contribute) -> [K], in the contract's order."""
    N, K = T.shape
    tiles = (N + LANES * U - 1) // (LANES * U)
    padded = np.zeros((tiles * U * LANES, K), dtype=T.dtype)
    padded[:N] = T
    t = padded.reshape(tiles, U, LANES, K)                               # vertex base + l + 256 i is [tile, i, l]
    x = np.zeros((tiles, LANES, K), dtype=T.dtype)
    for i in range(U):
        x = x + t[:, i]
    s = LANES // 2
    while s >= 1:
        x[:, :s] = x[:, :s] + x[:, s:2 * s]
        s //= 2
    out = np.zeros(K, dtype=T.dtype)
    for tile in range(tiles):
        out = out + x[tile, 0]
    return out


def normal(V, RT, valid, images, camera, bits, prox, z_near=0.01, margin=10, first_pose=0):
    V = np.asarray(V, dtype=np.float64)[:, :3]
    fx, fy = np.float64(camera[0]), np.float64(camera[1])
    B, H, W = images.shape[:3]
    rows, counts = np.zeros((B, ROW), dtype=np.float64), np.zeros(B, dtype=np.int32)
    for b in range(B):
        ids, xv, yv, zv, u, v = _pairs(V, RT[b], valid[b], first_pose + b, camera, bits, z_near, margin, H, W)
        if ids.size == 0:
            continue
        s = _sample(images[b, :, :, :3].astype(np.float64), u, v)
        I, dIdx, dIdy = s[:, 0] / 255000.0, s[:, 1] / 2040000.0, s[:, 2] / 2040000.0
        r = I - prox[ids]
        iz = 1.0 / zv
        v0 = (dIdx * fx) * iz
        v1 = (dIdy * fy) * iz
        v2 = -((v0 * xv + v1 * yv) * iz)
        J = [(-zv * v1) + yv * v2, zv * v0 - xv * v2, (-yv * v0) + xv * v1, v0, v1, v2]
        T = np.zeros((V.shape[0], ROW), dtype=np.float64)
        k = 0
        for i in range(6):
            for j in range(i, 6):
                T[ids, k] = J[i] * J[j]
                k += 1
        for i in range(6):
            T[ids, 21 + i] = J[i] * r
        T[ids, 27] = r * r
        rows[b] = ordered_sum(T)
        counts[b] = ids.size
    return rows, counts


def increment(x):
    x = np.asarray(x, dtype=np.float64).reshape(6)
    c, s = np.cos(x[:3]), np.sin(x[:3])
    cx, cy, cz, sx, sy, sz = c[0], c[1], c[2], s[0], s[1], s[2]
    return np.array([[cz * cy, (cz * sy) * sx - sz * cx, (cz * sy) * cx + sz * sx, x[3]],
                     [sz * cy, (sz * sy) * sx + cz * cx, (sz * sy) * cx - cz * sx, x[4]],
                     [-sy, cy * sx, cy * cx, x[5]],
                     [0.0, 0.0, 0.0, 1.0]], dtype=np.float64)


def solve(row):
    """One 28-row -> x [6], or None when the 6 x 6 is singular or x is not finite."""
    A = np.zeros((6, 6), dtype=np.float64)
    iu = np.triu_indices(6)
    A[iu] = row[:21]
    A.T[iu] = row[:21]
    try:
        x = np.linalg.solve(A, -row[21:27])
    except np.linalg.LinAlgError:
        return None
    return x if np.isfinite(x).all() else None


def update(E, valid, free, rows, counts, min_pairs, status):
    """E [P, 4, 4] in place; -> bool [P], which poses moved"""
    moved = np.zeros(len(E), dtype=bool)
    for p in range(len(E)):
        if not (free[p] and valid[p]):
            continue
        if counts[p] < min_pairs:
            status[p] |= FEW_PAIRS
            continue
        x = solve(rows[p])
        if x is None:
            status[p] |= SINGULAR
            continue
        E[p] = increment(x) @ np.ascontiguousarray(E[p])
        moved[p] = True
    return moved


def optimize(V, poses, color, camera, bits, iterations=30, free=None, min_pairs=16, margin=10, z_near=0.01, steps=None):
    """-> (poses [P, 4, 4], info); steps: a list that receives every x applied, as (iteration, pose, x)."""
    V = np.asarray(V, dtype=np.float64)[:, :3]
    poses = np.array(poses, dtype=np.float64).reshape(-1, 4, 4)
    P = len(poses)
    free = np.ones(P, dtype=bool) if free is None else np.asarray(free, dtype=bool)
    RT, valid = pose_extrinsics(poses)
    images = gradients(color)
    E = np.zeros((P, 4, 4), dtype=np.float64)
    E[:, :3, :] = RT.reshape(P, 3, 4)
    E[:, 3, 3] = 1.0
    status = (np.where(free, 0, NOT_FREE) | np.where(valid != 0, 0, INVALID)).astype(np.int32)
    residual, pairs = np.zeros((iterations + 1, P), dtype=np.float64), np.zeros((iterations + 1, P), dtype=np.int64)
    ever = np.zeros(P, dtype=bool)
    for it in range(iterations + 1):
        rt = np.ascontiguousarray(E[:, :3, :]).reshape(P, 12)
        total, count = accumulate(V, rt, valid, color, camera, bits, z_near, margin)
        rows, counts = normal(V, rt, valid, images, camera, bits, proxy(total, count), z_near, margin)
        residual[it], pairs[it] = rows[:, 27], counts
        if it < iterations:
            if steps is not None:
                steps.extend((it, p, solve(rows[p])) for p in range(P) if free[p] and valid[p] and counts[p] >= min_pairs)
            ever |= update(E, valid, free, rows, counts, min_pairs, status)
    out = poses.copy()
    for p in np.flatnonzero(ever):
        out[p] = np.linalg.inv(E[p])
    return out, dict(residual=residual, pairs=pairs, status=status)
