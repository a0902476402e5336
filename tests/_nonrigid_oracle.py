"""numpy restatement of the non-rigid colour-map optimisation contract (include/stin_hip.h, "Non-rigid colour-map optimisation";
preprocessing.optimize_poses_nonrigid): the yardstick of tests/test_nonrigid.py and tests/test_nonrigid_gpu.py.

Restated the OTHER way round from the kernels - per pose, vectorised over all vertices, the (J, r) of every pair laid out as arrays
and the terms of every cell summed in ascending vertex id by a plain sequential loop, where the kernels sort keys and run one
workgroup per (pose, cell).  It shares the rigid restatement's formulas (tests/_colormap_oracle.py) and
preprocessing.pose_extrinsics, the host step both sides start from.  The kernels have to reproduce it byte for byte.

* `lattice`       H, W, S -> (Ah, Aw).
* `pairs`         the pair set of one pose with cells, weights and warped positions.
* `accumulate`    stin_nonrigid_accumulate_f64 -> (sum int64 [N, 3], count int32 [N]).
* `terms`         one pose -> (ids, cell, z [n, 15] = (J[14], r)).
* `normal`        -> (blocks fp64 [B, cells, 120], counts int32 [B, cells]).
* `assemble`      one pose's blocks -> (A upper triangle, b) of the (6 + 2 Ah Aw) system.
* `update`        one Gauss-Newton update of extrinsics and flow on the host.
* `optimize`      the whole iteration -> (poses, flow, info), as preprocessing.optimize_poses_nonrigid returns them.
"""
import numpy as np

import _colormap_oracle as CO
from surface_texture_inpainting_net_amd.preprocessing import pose_extrinsics

LOCAL = 14
BLOCK = 120
NOT_FREE, INVALID, FEW_PAIRS, SINGULAR = CO.NOT_FREE, CO.INVALID, CO.FEW_PAIRS, CO.SINGULAR
TRI = [(i, j) for i in range(LOCAL) for j in range(i, LOCAL)]            # the 105 entries of the triangle, row-major


def lattice(H, W, S):
    return -(-(H - 1) // S) + 1, -(-(W - 1) // S) + 1


def pairs(V, m, valid, p, camera, bits, flow_p, S, z_near, margin, H, W):
    """-> dict of arrays over the contributing vertices of one pose: ids, xv, yv, zv, u, v, uw, vw, ci, cj, w [n, 4]"""
    ids, xv, yv, zv, u, v = CO._pairs(V, m, valid, p, camera, bits, z_near, margin, H, W)
    Ah, Aw = lattice(H, W, S)
    gu, gv = u / np.float64(S), v / np.float64(S)
    cj = np.minimum(np.floor(gu).astype(np.int64), Aw - 2)
    ci = np.minimum(np.floor(gv).astype(np.int64), Ah - 2)
    a, b = gu - cj.astype(np.float64), gv - ci.astype(np.float64)
    w = np.stack([(1.0 - a) * (1.0 - b), a * (1.0 - b), (1.0 - a) * b, a * b], axis=1)
    f = np.asarray(flow_p, dtype=np.float64).reshape(Ah, Aw, 2)
    f00, f01, f10, f11 = f[ci, cj], f[ci, cj + 1], f[ci + 1, cj], f[ci + 1, cj + 1]
    with np.errstate(all='ignore'):
        uw = u + ((w[:, 0] * f00[:, 0] + w[:, 1] * f01[:, 0]) + (w[:, 2] * f10[:, 0] + w[:, 3] * f11[:, 0]))
        vw = v + ((w[:, 0] * f00[:, 1] + w[:, 1] * f01[:, 1]) + (w[:, 2] * f10[:, 1] + w[:, 3] * f11[:, 1]))
        ok = np.isfinite(uw) & np.isfinite(vw) & (uw >= margin) & (uw <= W - 1 - margin) & (vw >= margin) & (vw <= H - 1 - margin)
    out = dict(ids=ids, xv=xv, yv=yv, zv=zv, u=u, v=v, uw=uw, vw=vw, ci=ci, cj=cj, w=w)
    return {k: x[ok] for k, x in out.items()}


def accumulate(V, RT, valid, color, camera, bits, flow, S, z_near=0.01, margin=10, first_pose=0):
    V = np.asarray(V, dtype=np.float64)[:, :3]
    color = np.asarray(color, dtype=np.uint8)
    H, W = color.shape[1:3]
    total, count = np.zeros((V.shape[0], 3), dtype=np.int64), np.zeros(V.shape[0], dtype=np.int32)
    for b in range(RT.shape[0]):
        q = pairs(V, RT[b], valid[b], first_pose + b, camera, bits, flow[b], S, z_near, margin, H, W)
        if q['ids'].size == 0:
            continue
        total[q['ids']] += np.rint(CO._sample(color[b].astype(np.float64), q['uw'], q['vw']) * 65536.0).astype(np.int64)
        count[q['ids']] += 1
    return total, count


def intensity(image, uw, vw):
    """image int32 [H, W, 4] -> (I, dIdx, dIdy) at the given positions"""
    s = CO._sample(image[:, :, :3].astype(np.float64), uw, vw)
    return s[:, 0] / 255000.0, s[:, 1] / 2040000.0, s[:, 2] / 2040000.0


def terms(V, m, valid, p, image, camera, bits, prox, flow_p, S, z_near, margin):
    """One pose -> (ids ascending, cell [n], z [n, 15]): the 14 entries of J and r of every contributing pair."""
    H, W = image.shape[:2]
    fx, fy = np.float64(camera[0]), np.float64(camera[1])
    q = pairs(V, m, valid, p, camera, bits, flow_p, S, z_near, margin, H, W)
    ids, xv, yv, zv, w = q['ids'], q['xv'], q['yv'], q['zv'], q['w']
    I, dIdx, dIdy = intensity(image, q['uw'], q['vw'])
    iz = 1.0 / zv
    v0 = (dIdx * fx) * iz
    v1 = (dIdy * fy) * iz
    v2 = -((v0 * xv + v1 * yv) * iz)
    z = np.zeros((ids.size, LOCAL + 1), dtype=np.float64)
    z[:, 0], z[:, 1], z[:, 2] = (-zv * v1) + yv * v2, zv * v0 - xv * v2, (-yv * v0) + xv * v1
    z[:, 3], z[:, 4], z[:, 5] = v0, v1, v2
    for k in range(4):
        z[:, 6 + 2 * k], z[:, 7 + 2 * k] = dIdx * w[:, k], dIdy * w[:, k]
    z[:, LOCAL] = I - prox[ids]
    Aw = lattice(H, W, S)[1]
    return ids, q['ci'] * (Aw - 1) + q['cj'], z


def block_terms(z):
    """z [n, 15] -> the 120 terms of every pair [n, 120]"""
    T = np.zeros((z.shape[0], BLOCK), dtype=np.float64)
    for k, (i, j) in enumerate(TRI):
        T[:, k] = z[:, i] * z[:, j]
    for i in range(LOCAL):
        T[:, 105 + i] = z[:, i] * z[:, LOCAL]
    T[:, 119] = z[:, LOCAL] * z[:, LOCAL]
    return T


def normal(V, RT, valid, images, camera, bits, prox, flow, S, z_near=0.01, margin=10, first_pose=0):
    V = np.asarray(V, dtype=np.float64)[:, :3]
    B, H, W = images.shape[:3]
    Ah, Aw = lattice(H, W, S)
    cells = (Ah - 1) * (Aw - 1)
    blocks, counts = np.zeros((B, cells, BLOCK), dtype=np.float64), np.zeros((B, cells), dtype=np.int32)
    for b in range(B):
        ids, cell, z = terms(V, RT[b], valid[b], first_pose + b, images[b], camera, bits, prox, flow[b], S, z_near, margin)
        T = block_terms(z)
        assert (np.diff(ids) > 0).all()
        for c in np.unique(cell):
            acc = np.zeros(BLOCK, dtype=np.float64)
            for row in T[cell == c]:                                     # ascending vertex id, one after another
                acc = acc + row
            blocks[b, c], counts[b, c] = acc, int((cell == c).sum())
    return blocks, counts


def unknowns(ci, cj, Aw):
    """The global unknowns of a cell's 14 local ones."""
    anchors = [ci * Aw + cj, ci * Aw + cj + 1, (ci + 1) * Aw + cj, (ci + 1) * Aw + cj + 1]
    return list(range(6)) + [6 + 2 * a + c for a in anchors for c in (0, 1)]


def assemble(blocks_p, Ah, Aw):
    """blocks [cells, 120] of one pose -> (A [n, n] symmetric, b [n], e), n = 6 + 2 Ah Aw"""
    n = 6 + 2 * Ah * Aw
    A, rhs, e = np.zeros((n, n), dtype=np.float64), np.zeros(n, dtype=np.float64), np.float64(0.0)
    for c in range((Ah - 1) * (Aw - 1)):
        g = unknowns(c // (Aw - 1), c % (Aw - 1), Aw)
        for k, (i, j) in enumerate(TRI):
            A[g[i], g[j]] = A[g[i], g[j]] + blocks_p[c, k]
        for i in range(LOCAL):
            rhs[g[i]] = rhs[g[i]] + blocks_p[c, 105 + i]
        e = e + blocks_p[c, 119]
    A = np.triu(A) + np.triu(A, 1).T
    return A, rhs, e


def update(E, flow, valid, free, blocks, counts, n_vertices, anchor_weight, min_pairs, status):
    """E [P, 4, 4] and flow [P, Ah, Aw, 2] in place; -> bool [P], which poses moved"""
    P, Ah, Aw = flow.shape[:3]
    moved = np.zeros(P, dtype=bool)
    for p in range(P):
        if not (free[p] and valid[p]):
            continue
        n_p = int(counts[p].sum())
        if n_p < min_pairs:
            status[p] |= FEW_PAIRS
            continue
        A, rhs, _ = assemble(blocks[p], Ah, Aw)
        with np.errstate(all='ignore'):
            wgt = (np.float64(anchor_weight) * np.float64(n_p)) / np.float64(n_vertices)
        w2 = wgt * wgt
        f = flow[p].reshape(-1)
        for k in range(f.size):
            A[6 + k, 6 + k] = A[6 + k, 6 + k] + w2
            rhs[6 + k] = rhs[6 + k] + w2 * f[k]
        try:
            x = np.linalg.solve(A, -rhs)
        except np.linalg.LinAlgError:
            x = None
        if x is None or not np.isfinite(x).all():
            status[p] |= SINGULAR
            continue
        E[p] = CO.increment(x[:6]) @ np.ascontiguousarray(E[p])
        flow[p] = flow[p] + x[6:].reshape(Ah, Aw, 2)
        moved[p] = True
    return moved


def residuals(blocks):
    """blocks [P, cells, 120] -> e [P]: r r over the cells ascending, from +0.0"""
    e = np.zeros(blocks.shape[0], dtype=np.float64)
    for c in range(blocks.shape[1]):
        e = e + blocks[:, c, 119]
    return e


def optimize(V, poses, color, camera, bits, S, iterations=30, anchor_weight=0.316, free=None, min_pairs=16, margin=10, z_near=0.01):
    """-> (poses [P, 4, 4], flow [P, Ah, Aw, 2], info)"""
    V = np.asarray(V, dtype=np.float64)[:, :3]
    poses = np.array(poses, dtype=np.float64).reshape(-1, 4, 4)
    P = len(poses)
    H, W = color.shape[1:3]
    Ah, Aw = lattice(H, W, S)
    free = np.ones(P, dtype=bool) if free is None else np.asarray(free, dtype=bool)
    RT, valid = pose_extrinsics(poses)
    images = CO.gradients(color)
    E = np.zeros((P, 4, 4), dtype=np.float64)
    E[:, :3, :] = RT.reshape(P, 3, 4)
    E[:, 3, 3] = 1.0
    flow = np.zeros((P, Ah, Aw, 2), dtype=np.float64)
    status = (np.where(free, 0, NOT_FREE) | np.where(valid != 0, 0, INVALID)).astype(np.int32)
    residual, npairs = np.zeros((iterations + 1, P), dtype=np.float64), np.zeros((iterations + 1, P), dtype=np.int64)
    flow_norm = np.zeros((iterations + 1, P), dtype=np.float64)
    ever = np.zeros(P, dtype=bool)
    for it in range(iterations + 1):
        rt = np.ascontiguousarray(E[:, :3, :]).reshape(P, 12)
        total, count = accumulate(V, rt, valid, color, camera, bits, flow, S, z_near, margin)
        blocks, counts = normal(V, rt, valid, images, camera, bits, CO.proxy(total, count), flow, S, z_near, margin)
        residual[it], npairs[it] = residuals(blocks), counts.sum(axis=1)
        flow_norm[it] = np.abs(flow).reshape(P, -1).max(axis=1)
        if it < iterations:
            ever |= update(E, flow, valid, free, blocks, counts, V.shape[0], anchor_weight, min_pairs, status)
    out = poses.copy()
    for p in np.flatnonzero(ever):
        out[p] = np.linalg.inv(E[p])
    return out, flow, dict(residual=residual, pairs=npairs, status=status, flow_norm=flow_norm)
