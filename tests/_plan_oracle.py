"""Graph plans restated in numpy, from the contract alone: the plan, renumbering and id sections of include/stin_hip.h and the
docstrings of plan.py.  No import of the package, no torch, no knowledge of HOW the library builds a plan (counting sort, radix
sort, batches, workspaces): buckets filled in pair order, stable argsorts, explicit loops.  Everything is an integer or
1 / max(1, d) in fp32, so every comparison against this file is an equality.  tests/test_plan_oracle.py checks the file
itself (typed-out cases, properties, the torch formulation of the renumbering); tests/test_plan_exact_gpu.py holds the
library to it."""
import numpy as np


def _i64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int64).reshape(-1))


def csr(key, val, n, val_limit):
    """(key, val) pairs grouped by key in [0, n) -> rowptr int32 [n + 1], col int32, perm int32, inv_deg fp32 [n],
    narrow int32 [E], bad.  A pair whose key is outside [0, n) or whose val is outside [0, val_limit) is dropped (and sets bad);
    the others keep their original order inside a row.  col = val (the pair id when val is None), perm = the pair id,
    inv_deg = 1 / max(1, degree), narrow = the key as int32, 0 where the pair was dropped."""
    key = _i64(key)
    val = None if val is None else _i64(val)
    rows = [[] for _ in range(n)]
    narrow = np.zeros(key.size, dtype=np.int32)
    bad = False
    for e in range(key.size):
        k = int(key[e])
        ok = 0 <= k < n
        if val is not None:
            ok = ok and 0 <= int(val[e]) < val_limit
        if not ok:
            bad = True
            continue
        rows[k].append(e)
        narrow[e] = k
    rowptr = np.zeros(n + 1, dtype=np.int32)
    perm = []
    for r in range(n):
        perm.extend(rows[r])
        rowptr[r + 1] = len(perm)
    perm = np.asarray(perm, dtype=np.int32).reshape(-1)
    col = perm.copy() if val is None else val[perm].astype(np.int32)
    deg = np.asarray([max(len(r), 1) for r in rows], dtype=np.float32).reshape(-1)
    inv_deg = (np.float32(1) / deg).astype(np.float32)
    return rowptr, col, perm, inv_deg, narrow, bad


class EdgePair:
    """Both CSRs of one directed edge set: *_dst rows = targets (col = sources), *_src rows = sources (col = targets)."""
    __slots__ = ('rowptr_dst', 'col_dst', 'perm_dst', 'inv_deg', 'rowptr_src', 'col_src', 'perm_src', 'xslot', 'w_src', 'bad')


def edge_pair(src, dst, n):
    """An edge with either endpoint outside [0, n) is dropped from BOTH CSRs.  xslot[s] = the destination-CSR slot of the edge
    that sits at source-CSR slot s; w_src[s] = inv_deg_dst[col_src[s]]."""
    src, dst = _i64(src), _i64(dst)
    p = EdgePair()
    p.rowptr_dst, p.col_dst, p.perm_dst, p.inv_deg, _, bad_d = csr(dst, src, n, n)
    p.rowptr_src, p.col_src, p.perm_src, _, _, bad_s = csr(src, dst, n, n)
    p.bad = bad_d or bad_s
    slot_of_edge = {}
    for t in range(p.perm_dst.size):
        slot_of_edge[int(p.perm_dst[t])] = t
    p.xslot = np.asarray([slot_of_edge[int(e)] for e in p.perm_src], dtype=np.int32).reshape(-1)
    p.w_src = np.asarray([p.inv_deg[int(c)] for c in p.col_src], dtype=np.float32).reshape(-1)
    return p


def pool_map(trace, n_fine, n_coarse):
    """trace int64 [n_fine]: fine vertex -> coarse vertex.  -> children CSR (rowptr, col = fine ids ascending, inv_count),
    the narrowed int32 trace (0 where out of range), bad."""
    trace = _i64(trace)
    assert trace.size == n_fine
    rowptr, col, _, inv_count, narrow, bad = csr(trace, None, n_coarse, 0)
    return rowptr, col, inv_count, narrow, bad


def morton_codes(pos):
    """pos [n, 3] -> int64 [n]: 10 bits per axis on the bounding box, x in bits 0, 3, 6 ..., y in 1, 4 ..., z in 2, 5 ....
    The quantisation in fp32, one operation at a time: (pos - lo) / max(hi - lo, 1e-20) * 1024, truncate, clamp to [0, 1023]."""
    pos = np.asarray(pos, dtype=np.float32)
    lo = pos.min(axis=0, keepdims=True)
    hi = pos.max(axis=0, keepdims=True)
    ext = np.maximum((hi - lo).astype(np.float32), np.float32(1e-20))
    t = ((pos - lo).astype(np.float32) / ext).astype(np.float32)
    t = (t * np.float32(1024.0)).astype(np.float32)
    q = np.clip(t.astype(np.int64), 0, 1023)
    code = np.zeros(pos.shape[0], dtype=np.int64)
    for bit in range(10):
        for axis in range(3):
            code |= ((q[:, axis] >> bit) & 1) << (3 * bit + axis)
    return code


def _rank_of(order):
    n = order.size
    rank = np.empty(n + 1, dtype=np.int64)
    rank[order] = np.arange(n)
    rank[n] = n
    return rank


def vertex_order(pos, traces, sizes):
    """pos [sizes[0], 3]; traces[l - 1] = the level l - 1 -> l map, int64 [sizes[l - 1]].  -> (ranks, order0): ranks[l] int64
    [n_l + 1] old id -> new id with ranks[l][n_l] = n_l, order0 int64 [n_0] new -> old.  Level 0: stable sort by Morton code
    (tied codes keep id order).  Level l >= 1: stable sort by the smallest new id among a vertex's children; trace entries
    outside [0, n_l) are skipped; childless vertices come last, in id order."""
    assert len(traces) == len(sizes) - 1
    code = morton_codes(pos)
    assert code.size == sizes[0]
    order0 = np.argsort(code, kind='stable')
    ranks = [_rank_of(order0)]
    for lvl in range(1, len(sizes)):
        nf, nc = sizes[lvl - 1], sizes[lvl]
        trace = _i64(traces[lvl - 1])
        assert trace.size == nf
        first = np.full(nc, nf, dtype=np.int64)                 # nf = larger than every new fine id: childless
        for v in range(nf):
            c = int(trace[v])
            if 0 <= c < nc and ranks[-1][v] < first[c]:
                first[c] = ranks[-1][v]
        ranks.append(_rank_of(np.argsort(first, kind='stable')))
    return ranks, order0


def relabel(ids, rank, limit):
    """out[i] = rank[ids[i]], or limit where ids[i] is outside [0, limit).  int64, same shape as ids."""
    a = np.asarray(ids, dtype=np.int64)
    flat = a.reshape(-1)
    out = np.empty(flat.size, dtype=np.int64)
    for i in range(flat.size):
        v = int(flat[i])
        out[i] = int(rank[v]) if 0 <= v < limit else limit
    return out.reshape(a.shape)


def relabel_trace(trace, rank_coarse, limit, rank_fine):
    """-> (coarse_new, fine_new, trace_new): coarse_new[v] / fine_new[v] = the new ids of trace[v] / v for v in ORIGINAL order
    (int64), trace_new int32 [n_fine] = new fine id -> new coarse id, 0 where the trace entry is out of range."""
    trace = _i64(trace)
    coarse_new = relabel(trace, rank_coarse, limit)
    fine_new = np.asarray(rank_fine, dtype=np.int64)[:trace.size].copy()
    trace_new = np.zeros(trace.size, dtype=np.int32)
    for v in range(trace.size):
        trace_new[fine_new[v]] = coarse_new[v] if coarse_new[v] < limit else 0
    return coarse_new, fine_new, trace_new


def norm_group_ids(batch, ptr_sum):
    """gid[r] = batch[r] (int32); sid[r] = the number of boundaries ptr_sum[1 .. B] that are <= r (int32)."""
    batch = _i64(batch)
    bounds = [int(v) for v in np.asarray(ptr_sum).reshape(-1)[1:]]
    sid = np.asarray([sum(1 for b in bounds if b <= r) for r in range(batch.size)], dtype=np.int32).reshape(-1)
    return batch.astype(np.int32), sid


def batch_pool(batch, trace, n_coarse):
    """scatter_max(batch, trace) with dim_size n_coarse: the largest graph id among a coarse vertex's children, 0 for none."""
    batch, trace = _i64(batch), _i64(trace)
    out = np.zeros(n_coarse, dtype=np.int64)
    seen = np.zeros(n_coarse, dtype=bool)
    for v in range(trace.size):
        c = int(trace[v])
        if not seen[c] or batch[v] > out[c]:
            out[c] = batch[v]
            seen[c] = True
    return out


def batch_unpool(batch_coarse, trace):
    """The coarse-to-fine gather batch[trace]."""
    return _i64(batch_coarse)[_i64(trace)]


# ------------------------------------------------------------------------------------------ inputs of the renumbering tests
def positions(kind, n, seed):
    """The two position families of the renumbering tests.  'lattice': multiples of 1/8 in a box of extents 8 x 4 x 2 anchored at
    (-4, 0, 1) with both ends of every axis present, drawn from few sites so that many points coincide - every fp32 operation of
    the quantisation is exact.  'normal': seeded normal positions."""
    rng = np.random.default_rng(seed)
    if kind == 'normal':
        return rng.standard_normal((n, 3)).astype(np.float32)
    ext = np.array([8.0, 4.0, 2.0])
    sites = max(2, min(n // 3, 40))
    cells = rng.integers(0, (ext * 8).astype(np.int64) + 1, size=(sites, 3))
    cells[0], cells[1] = 0, (ext * 8).astype(np.int64)
    pick = rng.integers(0, sites, n)
    pick[:min(n, 2)] = [0, 1][:min(n, 2)]
    return (cells[pick] / 8.0 + np.array([-4.0, 0.0, 1.0])).astype(np.float32)
