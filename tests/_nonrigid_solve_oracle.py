"""numpy restatement of the non-rigid solve contract (include/stin_hip.h, "Non-rigid solve"; preprocessing.nonrigid_solve and
optimize_poses_nonrigid(solver='banded')): the yardstick of tests/test_nonrigid_solve.py and tests/test_nonrigid_solve_gpu.py.

Restated the OTHER way round from the kernel: the system is assembled densely by the non-rigid restatement's own `assemble`
(tests/_nonrigid_oracle.py), permuted, and factored LEFT-looking, one entry of L after another by plain Python loops over the
envelope, where the kernel gathers band storage and factors right-looking through a sliding window.  Every entry receives its
subtractions in ascending pivot order either way, so the kernel has to reproduce x byte for byte.  Python floats are IEEE doubles
and `t - a * b` is two roundings.

* `envelope`   Ah, Aw -> (m, n, w, lo [n]).
* `system`     one pose -> (M [n, n] permuted, symmetric; r [n] = -b permuted), regularised: exactly what the host update builds.
* `factor_solve`  M, r, lo -> x permuted, or None (SINGULAR).
* `solve`      -> x [P, n], residual [P], pairs [P], status [P] (FEW_PAIRS / SINGULAR of this call only).
* `update`     NO.update's signature on top of `solve`.
* `optimize`   NO.optimize's loop with that update.
"""
import math

import numpy as np

import _colormap_oracle as CO
import _nonrigid_oracle as NO
from surface_texture_inpainting_net_amd.preprocessing import pose_extrinsics

FEW_PAIRS, SINGULAR = NO.FEW_PAIRS, NO.SINGULAR


def envelope(Ah, Aw):
    m = 2 * Ah * Aw
    n, w = m + 6, 2 * Aw + 3
    lo = [max(0, i - w) for i in range(m)] + [0] * 6
    return m, n, w, lo


def system(blocks_p, flow_p, n_pairs, n_vertices, anchor_weight):
    """-> (A [n, n] symmetric, b [n]) in the ORIGINAL order of the unknowns: the restatement's assembly and regulariser."""
    Ah, Aw = flow_p.shape[:2]
    A, rhs, _ = NO.assemble(blocks_p, Ah, Aw)
    with np.errstate(all='ignore'):
        wgt = (np.float64(anchor_weight) * np.float64(n_pairs)) / np.float64(n_vertices)
        w2 = wgt * wgt
        f = flow_p.reshape(-1)
        for k in range(f.size):
            A[6 + k, 6 + k] = A[6 + k, 6 + k] + w2
            rhs[6 + k] = rhs[6 + k] + w2 * f[k]
    return A, rhs


def factor_solve(M, r, lo):
    """M: list of rows (the permuted matrix; only the envelope of the lower triangle is read), r = -b permuted -> x permuted as a
    list, or None when a pivot is not > 0."""
    n = len(r)
    L = [[0.0] * n for _ in range(n)]
    for i in range(n):
        Li, Mi = L[i], M[i]
        for j in range(lo[i], i + 1):
            Lj = L[j]
            t = Mi[j]
            for k in range(max(lo[i], lo[j]), j):
                t = t - Li[k] * Lj[k]
            if j < i:
                Li[j] = t / Lj[j]
            elif not t > 0:
                return None
            else:
                Li[i] = math.sqrt(t)
    y = [0.0] * n
    for i in range(n):
        t, Li = r[i], L[i]
        for k in range(lo[i], i):
            t = t - Li[k] * y[k]
        y[i] = t / Li[i]
    x = [0.0] * n
    for i in range(n - 1, -1, -1):
        t = y[i]
        for k in range(n - 1, i, -1):
            if lo[k] <= i:
                t = t - L[k][i] * x[k]
        x[i] = t / L[i][i]
    return x


def solve(blocks, counts, flow, valid, free, n_vertices, anchor_weight, min_pairs):
    """-> x float64 [P, n], residual float64 [P], pairs int64 [P], status int32 [P]"""
    P, Ah, Aw = flow.shape[:3]
    m, n, w, lo = envelope(Ah, Aw)
    q = np.concatenate([np.arange(6, n), np.arange(6)])
    x = np.zeros((P, n), dtype=np.float64)
    status = np.zeros(P, dtype=np.int32)
    pairs = np.array([int(np.asarray(counts[p], dtype=np.int64).sum()) for p in range(P)], dtype=np.int64).reshape(P)
    with np.errstate(all='ignore'):
        residual = NO.residuals(np.asarray(blocks, dtype=np.float64))
    for p in range(P):
        if not (free[p] and valid[p]):
            continue
        if pairs[p] < min_pairs:
            status[p] |= FEW_PAIRS
            continue
        with np.errstate(all='ignore'):
            A, b = system(blocks[p], flow[p], int(pairs[p]), n_vertices, anchor_weight)
        xq = factor_solve(A[np.ix_(q, q)].tolist(), (-b[q]).tolist(), lo)
        if xq is None or not np.isfinite(xq).all():
            status[p] |= SINGULAR
            continue
        x[p, q] = xq
    return x, residual, pairs, status


def update(E, flow, valid, free, blocks, counts, n_vertices, anchor_weight, min_pairs, status):
    """NO.update with the banded solve: E [P, 4, 4] and flow [P, Ah, Aw, 2] in place; -> bool [P], which poses moved"""
    P, Ah, Aw = flow.shape[:3]
    x, _, _, st = solve(blocks, counts, flow, valid, free, n_vertices, anchor_weight, min_pairs)
    status |= st
    moved = np.zeros(P, dtype=bool)
    for p in range(P):
        if st[p] != 0 or not (free[p] and valid[p]):
            continue
        E[p] = CO.increment(x[p, :6]) @ np.ascontiguousarray(E[p])
        flow[p] = flow[p] + x[p, 6:].reshape(Ah, Aw, 2)
        moved[p] = True
    return moved


def optimize(V, poses, color, camera, bits, S, iterations=30, anchor_weight=0.316, free=None, min_pairs=16, margin=10, z_near=0.01):
    """NO.optimize with the banded update -> (poses [P, 4, 4], flow [P, Ah, Aw, 2], info)"""
    V = np.asarray(V, dtype=np.float64)[:, :3]
    poses = np.array(poses, dtype=np.float64).reshape(-1, 4, 4)
    P = len(poses)
    H, W = color.shape[1:3]
    Ah, Aw = NO.lattice(H, W, S)
    free = np.ones(P, dtype=bool) if free is None else np.asarray(free, dtype=bool)
    RT, valid = pose_extrinsics(poses)
    images = CO.gradients(color)
    E = np.zeros((P, 4, 4), dtype=np.float64)
    E[:, :3, :] = RT.reshape(P, 3, 4)
    E[:, 3, 3] = 1.0
    flow = np.zeros((P, Ah, Aw, 2), dtype=np.float64)
    status = (np.where(free, 0, NO.NOT_FREE) | np.where(valid != 0, 0, NO.INVALID)).astype(np.int32)
    residual, npairs = np.zeros((iterations + 1, P), dtype=np.float64), np.zeros((iterations + 1, P), dtype=np.int64)
    flow_norm = np.zeros((iterations + 1, P), dtype=np.float64)
    ever = np.zeros(P, dtype=bool)
    for it in range(iterations + 1):
        rt = np.ascontiguousarray(E[:, :3, :]).reshape(P, 12)
        total, count = NO.accumulate(V, rt, valid, color, camera, bits, flow, S, z_near, margin)
        blocks, counts = NO.normal(V, rt, valid, images, camera, bits, CO.proxy(total, count), flow, S, z_near, margin)
        residual[it], npairs[it] = NO.residuals(blocks), counts.sum(axis=1)
        flow_norm[it] = np.abs(flow).reshape(P, -1).max(axis=1)
        if it < iterations:
            ever |= update(E, flow, valid, free, blocks, counts, V.shape[0], anchor_weight, min_pairs, status)
    out = poses.copy()
    for p in np.flatnonzero(ever):
        out[p] = np.linalg.inv(E[p])
    return out, flow, dict(residual=residual, pairs=npairs, status=status, flow_norm=flow_norm, solver='banded')
