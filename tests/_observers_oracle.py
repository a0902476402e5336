"""numpy restatement of the observer-mask contract (include/stin_hip.h, "Observer masks"; preprocessing.observe_vertices): the
yardstick of tests/test_observers.py and tests/test_observers_gpu.py.

No golden file from the reference is possible or needed: its `observers` path cannot run (its pytorch3d imports are commented out
while compute_observed_vertex_map still calls them, and process_frame_observers returns one array where the writer iterates over a
list), and neither pytorch3d nor open3d is installed here.  So the contract is restated the OTHER way round from the kernels - per
pose and per pixel, a gather over all faces in vectorised fp64, the minimum key, then the vertices of the winners - sharing only the
formulas (and preprocessing.pose_extrinsics, the host step both sides start from).  The kernels have to reproduce it bit for bit.

* `observe`        the contract -> (bits uint32 [N, words], valid_pose_ids, face_ids int64 [P, S, S] with -1 for an empty pixel).
* `masks`          popcount(bits & visible) >= min_num_poses, optionally inverted -> (mask int64 [M, N], count int32 [M, N]).
* `look_at`, `orbit`, `wall`   small scene builders.
"""
import numpy as np

from surface_texture_inpainting_net_amd.preprocessing import pose_extrinsics

NO_FACE = np.uint64(0xFFFFFFFFFFFFFFFF)


def edge(px, py, qx, qy, rx, ry):
    return (qx - px) * (ry - py) - (qy - py) * (rx - px)


def screen(V, rt, sx, sy, S):
    x, y, z = V[:, 0], V[:, 1], V[:, 2]
    with np.errstate(all='ignore'):
        xv = ((rt[0] * x + rt[1] * y) + rt[2] * z) + rt[3]
        yv = ((rt[4] * x + rt[5] * y) + rt[6] * z) + rt[7]
        zv = ((rt[8] * x + rt[9] * y) + rt[10] * z) + rt[11]
        X = (sx * xv / zv + 1.0) * (0.5 * S) - 0.5
        Y = (sy * yv / zv + 1.0) * (0.5 * S) - 0.5
    return X, Y, zv


def pose_keys(V, F, rt, sx, sy, S, z_near):
    """The key of every pixel of one pose, uint64 [S, S]: min over the faces of bits(float32(depth)) << 32 | face id."""
    N = V.shape[0]
    keys = np.full(S * S, NO_FACE, dtype=np.uint64)
    if F.shape[0] == 0 or N == 0:
        return keys.reshape(S, S)
    with np.errstate(all='ignore'):
        X, Y, Z = screen(V, rt, sx, sy, S)
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
            return keys.reshape(S, S)
        ax, ay, az, bx, by, bz, cx, cy, cz, area2 = (a[ids][None, :] for a in (ax, ay, az, bx, by, bz, cx, cy, cz, area2))
        ii, jj = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing='ij')
        px, py = jj.reshape(-1, 1), ii.reshape(-1, 1)                     # centre of pixel (row i, column j) = (X, Y) = (j, i)
        wa = edge(bx, by, cx, cy, px, py)
        wb = edge(cx, cy, ax, ay, px, py)
        wc = edge(ax, ay, bx, by, px, py)
        cover = ((area2 > 0.0) & (wa >= 0.0) & (wb >= 0.0) & (wc >= 0.0)) | ((area2 < 0.0) & (wa <= 0.0) & (wb <= 0.0) & (wc <= 0.0))
        la, lb, lc = wa / area2, wb / area2, wc / area2
        zp = 1.0 / ((la / az + lb / bz) + lc / cz)
        depth = zp.astype(np.float32).view(np.uint32).astype(np.uint64)
        k = (depth << np.uint64(32)) | ids.astype(np.uint64)[None, :]
        keys = np.where(cover, k, NO_FACE).min(axis=1)
    return keys.reshape(S, S)


def observe(V, F, poses, fx, fy, width, height, image_size=256, z_near=0.01):
    V = np.asarray(V, dtype=np.float64)[:, :3]
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    RT, valid = pose_extrinsics(poses)
    P, N, S = RT.shape[0], V.shape[0], int(image_size)
    sx, sy = 2.0 * float(fx) / float(width), 2.0 * float(fy) / float(height)
    bits = np.zeros((N, (P + 31) // 32), dtype=np.uint32)
    face_ids = np.full((P, S, S), -1, dtype=np.int64)
    for p in range(P):
        if not valid[p]:
            continue
        keys = pose_keys(V, F, RT[p], sx, sy, S, z_near)
        hit = keys != NO_FACE
        face_ids[p][hit] = (keys[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        seen = np.unique(F[np.unique(face_ids[p][hit])].reshape(-1))
        bits[seen, p >> 5] |= np.uint32(1 << (p & 31))
    return bits, np.flatnonzero(valid).astype(np.int64), face_ids


def unpack(bits, num_poses):
    """uint32 [N, words] -> bool [N, num_poses]"""
    b = np.asarray(bits, dtype=np.uint32)
    return ((b[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(b.shape[0], -1)[:, :num_poses]


def masks(bits, visible, min_num_poses, invert=False):
    visible = np.asarray(visible, dtype=bool)
    seen = unpack(bits, visible.shape[1])
    count = (seen[None, :, :] & visible[:, None, :]).sum(axis=2).astype(np.int32)
    return ((count >= min_num_poses) ^ bool(invert)).astype(np.int64), count


# ------------------------------------------------------------------------------------------------------------------- scenes
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """Camera-to-world [4, 4] of a camera at `eye` looking at `target`: camera +z forward, +x right, +y down (the image's rows)."""
    eye, target, up = (np.asarray(a, dtype=np.float64) for a in (eye, target, up))
    fwd = target - eye
    fwd = fwd / np.linalg.norm(fwd)
    right = np.cross(fwd, up)
    if np.linalg.norm(right) < 1e-9:                                      # looking along `up`
        right = np.cross(fwd, np.array([0.0, 1.0, 0.0]))
    right = right / np.linalg.norm(right)
    down = np.cross(fwd, right)
    M = np.eye(4)
    M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = right, down, fwd, eye
    return M


def orbit(n, radius, height=0.0, target=(0.0, 0.0, 0.0), phase=0.1):
    """n poses on a circle of `radius` around `target` at `height` above it, all looking at it."""
    t = np.asarray(target, dtype=np.float64)
    return np.stack([look_at(t + [radius * np.cos(a), radius * np.sin(a), height], t)
                     for a in phase + 2 * np.pi * np.arange(n) / max(n, 1)]) if n else np.zeros((0, 4, 4))


def wall(k, size, origin=(0.0, 0.0, 0.0), u=(1.0, 0.0, 0.0), v=(0.0, 1.0, 0.0)):
    """A k x k quad grid (2 k k triangles, (k + 1)^2 vertices) spanning origin +/- size / 2 along u and v."""
    o, u, v = (np.asarray(a, dtype=np.float64) for a in (origin, u, v))
    s = (np.arange(k + 1) / k - 0.5) * size
    gi, gj = np.meshgrid(np.arange(k + 1), np.arange(k + 1), indexing='ij')
    V = o + s[gi.ravel()][:, None] * u + s[gj.ravel()][:, None] * v
    ids = np.arange((k + 1) ** 2).reshape(k + 1, k + 1)
    a, b, c, d = ids[:-1, :-1].ravel(), ids[1:, :-1].ravel(), ids[:-1, 1:].ravel(), ids[1:, 1:].ravel()
    return V, np.concatenate([np.stack([a, b, d], 1), np.stack([a, d, c], 1)]).astype(np.int64)
