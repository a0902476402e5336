"""The row kernels' summation contract restated in torch-CPU float32 (tests/test_row_geometry_gpu.py).

Every row adds its CSR slots one after the other in fp32 - slot position t = 0 .. max_degree - 1, vectorised over the rows that
still have a slot t - with separate multiplies and adds (no fused multiply-add; torch's CPU add and mul are separate passes),
then divides by the degree.  bf16 operands are widened first; the caller rounds the fp32 result with .to(torch.bfloat16)."""
import torch

BLOCK = 256      # threads per block of the row kernels
TI_ITER = 4      # row groups per block of the translation-invariant backward


def sweep_graph(n, seed, first=0):
    """edge_index [2, E]: vertex i has in-degree (i + first) mod 14 (two full trips plus a remainder of the largest U = 6, and
    U - 1, U, U + 1 of every U in the table), sources seeded random."""
    deg = (torch.arange(n) + first) % 14
    dst = torch.repeat_interleave(torch.arange(n), deg)
    src = torch.randint(0, n, (dst.numel(),), generator=torch.Generator().manual_seed(seed))
    return torch.stack([src, dst])


def csr(key, val, n):
    """CSR grouped by key, entries in their original order (the plan kernels' stable sort) -> rowptr [n + 1], col [E], order [E]"""
    order = torch.sort(key, stable=True).indices
    rowptr = torch.zeros(n + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(torch.bincount(key, minlength=n), 0)
    return rowptr, (val[order] if val is not None else None), order


def _trips(rowptr):
    """(rows, slots) of slot position t = 0, 1, ...: the rows whose degree exceeds t and their t-th CSR slot"""
    deg = rowptr[1:] - rowptr[:-1]
    for t in range(int(deg.max()) if deg.numel() else 0):
        rows = (deg > t).nonzero().flatten()
        yield rows, rowptr[rows] + t


def _count(rowptr):
    return (rowptr[1:] - rowptr[:-1]).clamp(min=1).float()


def edge_fwd(A, B, rowptr, col):
    """out[i] = (sum over slots of relu(A[i] + B[col[e]])) / max(deg, 1)"""
    a, b = A.float(), B.float()
    acc = torch.zeros_like(a)
    for rows, e in _trips(rowptr):
        acc[rows] = acc[rows] + torch.relu(a[rows] + b[col[e]])
    return acc / _count(rowptr)[:, None]


def edge_bwd_dst(A, B, G, rowptr, col):
    """dA[i] = G[i] * (1 / deg) * #(slots with A[i] + B[col[e]] > 0), evaluated left to right"""
    a, b = A.float(), B.float()
    cnt = torch.zeros_like(a)
    for rows, e in _trips(rowptr):
        cnt[rows] = cnt[rows] + (a[rows] + b[col[e]] > 0).float()
    s = 1.0 / _count(rowptr)
    return G.float() * s[:, None] * cnt


def edge_bwd_src(A, B, G, inv_deg, rowptr_src, col_src):
    """dB[j] = sum over the source-CSR slots (j -> i) of [A[i] + B[j] > 0] ? inv_deg[i] * G[i] : 0"""
    a, b, g = A.float(), B.float(), G.float()
    acc = torch.zeros_like(b)
    for rows, e in _trips(rowptr_src):
        i = col_src[e]
        acc[rows] = acc[rows] + torch.where(a[i] + b[rows] > 0, inv_deg[i][:, None] * g[i], torch.zeros(()))
    return acc


def segment_sum(src, rowptr, col, mean):
    """out[i] = sum over slots of src[col[e]] (src[e] for col None), / max(deg, 1) for the mean"""
    v = src.float()
    acc = torch.zeros(rowptr.numel() - 1, v.shape[1])
    for rows, e in _trips(rowptr):
        acc[rows] = acc[rows] + v[col[e] if col is not None else e]
    return acc / _count(rowptr)[:, None] if mean else acc


def ti_colsum(dA, H):
    """Per-block column sums of dA as k_edge_bwd_mask_ti forms them: a lane group (row slot r of the block) adds the rows it
    visits in its TI_ITER iterations in ascending order, then the block folds its row slots in ascending order."""
    rpb = BLOCK // (32 if H == 128 else 64)
    n = dA.shape[0]
    nblk = -(-(-(-n // rpb)) // TI_ITER)
    pad = torch.zeros(nblk * TI_ITER * rpb, H)
    pad[:n] = dA
    pad = pad.view(nblk, TI_ITER, rpb, H)
    lane = pad[:, 0]
    for it in range(1, TI_ITER):
        lane = lane + pad[:, it]
    out = lane[:, 0]
    for r in range(1, rpb):
        out = out + lane[:, r]
    return out


def fold_rows(x):
    """rows added in ascending order in fp32"""
    t = torch.zeros(x.shape[1])
    for r in range(x.shape[0]):
        t = t + x[r]
    return t
