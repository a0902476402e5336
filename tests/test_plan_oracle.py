"""tests/_plan_oracle.py checked on its own (no GPU): typed-out cases where every expected array was worked out by hand from
include/stin_hip.h, properties that hold for every graph, and the renumbering against the torch formulation of
plan.GraphPlan._ensure_order (its expressions copied here and run on CPU tensors - the class itself asserts a GPU sample), which
anchors the fp32 quantisation of the numpy version."""
import numpy as np
import pytest
import torch

import _plan_oracle as O

F = np.float32


def _eq(got, want, dtype):
    got = np.asarray(got)
    assert got.dtype == dtype, got.dtype
    assert np.array_equal(got, np.asarray(want, dtype=dtype)), (got, want)


# ----------------------------------------------------------------------------------------------------------- typed-out cases
#        e0      e1 (dup)  e2 (loop)  e3      e4 (source 5: dropped)  e5
SRC6 = [1,      1,        3,         2,      5,                      0]
DST6 = [2,      2,        3,         0,      1,                      2]


def test_literal_six_edges_csr():
    """4 vertices, grouped by target: row 1 is empty because its only edge is the dropped one."""
    rowptr, col, perm, inv_deg, narrow, bad = O.csr(DST6, SRC6, 4, 4)
    _eq(rowptr, [0, 1, 1, 4, 5], np.int32)
    _eq(perm, [3, 0, 1, 5, 2], np.int32)
    _eq(col, [2, 1, 1, 0, 3], np.int32)
    _eq(inv_deg, [1, 1, F(1) / F(3), 1], np.float32)
    _eq(narrow, [2, 2, 3, 0, 0, 2], np.int32)            # e4: key 1 is in range, its value is not - the PAIR is dropped: 0
    assert bad is True


def test_literal_six_edges_pair():
    p = O.edge_pair(SRC6, DST6, 4)
    _eq(p.rowptr_dst, [0, 1, 1, 4, 5], np.int32)
    _eq(p.col_dst, [2, 1, 1, 0, 3], np.int32)
    _eq(p.inv_deg, [1, 1, F(1) / F(3), 1], np.float32)
    _eq(p.rowptr_src, [0, 1, 3, 4, 5], np.int32)
    _eq(p.perm_src, [5, 0, 1, 3, 2], np.int32)
    _eq(p.col_src, [2, 2, 2, 0, 3], np.int32)
    _eq(p.xslot, [3, 1, 2, 0, 4], np.int32)
    _eq(p.w_src, [F(1) / F(3), F(1) / F(3), F(1) / F(3), 1, 1], np.float32)
    assert p.bad is True


def test_literal_keys_without_values():
    rowptr, col, perm, inv_deg, narrow, bad = O.csr([2, 0, 2, 7, -1, 0], None, 3, 0)
    _eq(rowptr, [0, 2, 2, 4], np.int32)
    _eq(col, [1, 5, 0, 2], np.int32)
    _eq(perm, [1, 5, 0, 2], np.int32)
    _eq(inv_deg, [0.5, 1, 0.5], np.float32)
    _eq(narrow, [2, 0, 2, 0, 0, 0], np.int32)
    assert bad is True
    rowptr, col, perm, inv_deg, narrow, bad = O.csr([], [], 3, 3)
    _eq(rowptr, [0, 0, 0, 0], np.int32)
    assert col.size == 0 and perm.size == 0 and narrow.size == 0 and bad is False
    _eq(inv_deg, [1, 1, 1], np.float32)


TRACE75 = [0, 0, 0, 2, 4, 4, 2]                         # 7 fine -> 5 coarse; clusters 1 and 3 are empty


def test_literal_seven_to_five_trace():
    rowptr, col, inv_count, narrow, bad = O.pool_map(TRACE75, 7, 5)
    _eq(rowptr, [0, 3, 3, 5, 5, 7], np.int32)
    _eq(col, [0, 1, 2, 3, 6, 4, 5], np.int32)
    _eq(inv_count, [F(1) / F(3), 1, 0.5, 1, 0.5], np.float32)
    _eq(narrow, TRACE75, np.int32)
    assert bad is False
    pooled = O.batch_pool([0, 0, 1, 1, 2, 3, 1], TRACE75, 5)
    _eq(pooled, [1, 0, 1, 0, 3], np.int64)
    _eq(O.batch_unpool(pooled, TRACE75), [1, 1, 1, 1, 3, 3, 1], np.int64)


def test_literal_renumbering():
    """x = 3 1 2 1 0 4 2 on a box [0, 4]: quantised 768 256 512 256 0 1023 512, so the ties (ids 1, 3 and 2, 6) keep id order."""
    pos = np.zeros((7, 3), dtype=np.float32)
    pos[:, 0] = [3, 1, 2, 1, 0, 4, 2]
    b8, b9 = 1 << 24, 1 << 27                            # bit k of x sits at code bit 3 k
    _eq(O.morton_codes(pos), [b9 | b8, b8, b9, b8, 0, 0x09249249, b9], np.int64)
    pos[:, 1] = pos[:, 0]                                # the same along y: one bit higher
    _eq(O.morton_codes(pos), [3 * (b9 | b8), 3 * b8, 3 * b9, 3 * b8, 0, 3 * 0x09249249, 3 * b9], np.int64)
    pos[:, 1] = 0
    ranks, order0 = O.vertex_order(pos, [TRACE75], [7, 5])
    _eq(order0, [4, 1, 3, 2, 6, 0, 5], np.int64)
    _eq(ranks[0], [5, 1, 3, 2, 0, 6, 4, 7], np.int64)
    _eq(ranks[1], [1, 3, 2, 4, 0, 5], np.int64)          # first child: 1, -, 2, -, 0 -> 4, 0, 2 then the childless 1, 3
    coarse_new, fine_new, trace_new = O.relabel_trace(TRACE75, ranks[1], 5, ranks[0])
    _eq(coarse_new, [1, 1, 1, 2, 0, 0, 2], np.int64)
    _eq(fine_new, [5, 1, 3, 2, 0, 6, 4], np.int64)
    _eq(trace_new, [0, 1, 2, 1, 2, 1, 0], np.int32)
    _eq(O.relabel([[-1, 5, 2 ** 40], [3, 0, 4]], ranks[1], 5), [[5, 5, 5], [4, 1, 0]], np.int64)
    coarse_new, fine_new, trace_new = O.relabel_trace([0, 9, 0, 2, -4, 4, 2], ranks[1], 5, ranks[0])
    _eq(coarse_new, [1, 5, 1, 2, 5, 0, 2], np.int64)
    _eq(trace_new, [0, 0, 2, 1, 2, 1, 0], np.int32)      # new fine ids 1 and 0 (old 1 and 4) carry the bad entries: 0


def test_literal_norm_group_ids():
    gid, sid = O.norm_group_ids([0, 0, 0, 1, 1, 2, 2], [0, 2, 4, 7])
    _eq(gid, [0, 0, 0, 1, 1, 2, 2], np.int32)
    _eq(sid, [0, 0, 1, 1, 2, 2, 2], np.int32)
    gid, sid = O.norm_group_ids([0, 2, 2], [0, 0, 1, 3])  # an empty first slice: its boundary counts for every row
    _eq(sid, [1, 2, 2], np.int32)


# ------------------------------------------------------------------------------------------------- properties on random graphs
@pytest.mark.parametrize('n,e,seed', [(1, 40, 0), (7, 1, 1), (13, 300, 2), (257, 2000, 3), (600, 500, 4)])
def test_pair_properties(n, e, seed):
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(-1, n + 1, e), rng.integers(-1, n + 1, e)          # a few out of range on both sides
    p = O.edge_pair(src, dst, n)
    ok = (src >= 0) & (src < n) & (dst >= 0) & (dst < n)
    kept = np.flatnonzero(ok)
    assert p.bad == bool((~ok).any())
    assert int(p.rowptr_dst[-1]) == int(p.rowptr_src[-1]) == kept.size == p.xslot.size
    # perm is the stable argsort of the key (over the surviving pairs)
    assert np.array_equal(p.perm_dst, kept[np.argsort(dst[kept], kind='stable')])
    assert np.array_equal(p.perm_src, kept[np.argsort(src[kept], kind='stable')])
    assert np.array_equal(p.rowptr_dst, np.concatenate([[0], np.cumsum(np.bincount(dst[kept], minlength=n))]))
    assert np.array_equal(p.col_dst, src[p.perm_dst]) and np.array_equal(p.col_src, dst[p.perm_src])
    # xslot is a bijection onto the valid destination slots
    assert np.array_equal(np.sort(p.xslot), np.arange(kept.size))
    row_of_src_slot = np.repeat(np.arange(n), np.diff(p.rowptr_src))
    row_of_dst_slot = np.repeat(np.arange(n), np.diff(p.rowptr_dst))
    assert np.array_equal(p.col_dst[p.xslot], row_of_src_slot)                 # the edge's source, seen from the target's row
    assert np.array_equal(row_of_dst_slot[p.xslot], p.col_src)                 # its destination row is its target
    assert np.array_equal(p.perm_dst[p.xslot], p.perm_src)                     # it IS the same edge
    deg = np.maximum(np.bincount(dst[kept], minlength=n), 1)
    assert np.array_equal(p.inv_deg, (1.0 / deg).astype(np.float32))
    assert np.array_equal(p.w_src, p.inv_deg[p.col_src])


@pytest.mark.parametrize('n,e,limit,seed', [(5, 60, 9, 0), (300, 1000, 300, 1), (64, 64, 1, 2)])
def test_csr_properties(n, e, limit, seed):
    rng = np.random.default_rng(seed)
    key, val = rng.integers(-2, n + 2, e), rng.integers(-1, limit + 1, e)
    rowptr, col, perm, inv_deg, narrow, bad = O.csr(key, val, n, limit)
    ok = (key >= 0) & (key < n) & (val >= 0) & (val < limit)
    kept = np.flatnonzero(ok)
    assert np.array_equal(perm, kept[np.argsort(key[kept], kind='stable')])
    assert np.array_equal(col, val[perm]) and np.array_equal(narrow, np.where(ok, key, 0))
    assert np.array_equal(key[perm], np.repeat(np.arange(n), np.diff(rowptr)))
    assert bad == bool((~ok).any())
    rowptr2, col2, perm2, _, _, _ = O.csr(key, None, n, 0)
    assert np.array_equal(col2, perm2) and int(rowptr2[-1]) == int(((key >= 0) & (key < n)).sum())


# ------------------------------------------------------------------------------- the renumbering against the torch formulation
def _torch_order(pos, traces, sizes):
    """The expressions of plan.GraphPlan._ensure_order (framework formulation), on CPU tensors."""
    pos = torch.from_numpy(np.asarray(pos)).to(torch.float32)
    lo, hi = pos.amin(0, keepdim=True), pos.amax(0, keepdim=True)
    q = ((pos - lo) / (hi - lo).clamp_min(1e-20) * 1024.0).to(torch.int64).clamp_(0, 1023)

    def spread(v):                                    # 10 bits -> every third bit
        v = (v | (v << 16)) & 0x030000FF
        v = (v | (v << 8)) & 0x0300F00F
        v = (v | (v << 4)) & 0x030C30C3
        return (v | (v << 2)) & 0x09249249
    code = spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2)
    order = torch.argsort(code, stable=True)
    n = order.numel()
    rank = torch.empty(n + 1, dtype=torch.int64)
    rank[order] = torch.arange(n)
    rank[n] = n
    ranks = [rank]
    for lvl in range(1, len(sizes)):
        nc = sizes[lvl]
        tr = torch.from_numpy(np.asarray(traces[lvl - 1], dtype=np.int64))
        ok = (tr >= 0) & (tr < nc)
        first = torch.full((nc,), n, dtype=torch.int64)
        first.scatter_reduce_(0, torch.where(ok, tr, 0), torch.where(ok, ranks[-1][:-1], n), 'amin', include_self=True)
        c_order = torch.argsort(first, stable=True)
        c_rank = torch.empty(nc + 1, dtype=torch.int64)
        c_rank[c_order] = torch.arange(nc)
        c_rank[nc] = nc
        ranks.append(c_rank)
        n = nc
    return [r.numpy() for r in ranks], order.numpy(), code.numpy()


@pytest.mark.parametrize('kind', ['lattice', 'normal'])
@pytest.mark.parametrize('n0', [1, 2, 255, 257, 3000])
def test_vertex_order_equals_the_torch_formulation(kind, n0):
    rng = np.random.default_rng(n0)
    pos = O.positions(kind, n0, n0 + 1)
    n1, n2 = max(1, n0 // 3), max(1, n0 // 9)
    t1, t2 = rng.integers(0, max(1, n1 - n1 // 4), n0), rng.integers(-1, n2 + 1, n1)   # childless coarse ids, bad entries
    ranks, order0 = O.vertex_order(pos, [t1, t2], [n0, n1, n2])
    want_ranks, want_order, want_code = _torch_order(pos, [t1, t2], [n0, n1, n2])
    assert np.array_equal(O.morton_codes(pos), want_code)
    assert np.array_equal(order0, want_order)
    for got, want in zip(ranks, want_ranks):
        assert np.array_equal(got, want)
    for r, n in zip(ranks, (n0, n1, n2)):
        assert r.shape == (n + 1,) and r[n] == n and np.array_equal(np.sort(r[:n]), np.arange(n))
    assert np.array_equal(ranks[0][order0], np.arange(n0))                     # rank[order] == arange
    if kind == 'lattice' and n0 >= 255:
        assert np.unique(O.morton_codes(pos)).size <= n0 // 3                  # the ties the family is there for


def test_vertex_order_variations_equal_the_torch_formulation():
    rng = np.random.default_rng(5)
    for kind in ('lattice', 'normal'):
        pos = O.positions(kind, 500, 9)
        flat = pos.copy()
        flat[:, 1] = 0.25                                                     # one axis constant: extent 0 -> clamp_min(1e-20)
        for p in (flat, pos):
            tr = rng.integers(0, 100, 500)
            ranks, order0 = O.vertex_order(p, [tr], [500, 120])               # coarse ids 100 .. 119 are childless
            want_ranks, want_order, _ = _torch_order(p, [tr], [500, 120])
            assert np.array_equal(order0, want_order)
            assert np.array_equal(ranks[1], want_ranks[1])
            assert np.array_equal(ranks[1][100:120], np.arange(100, 120))     # childless: last, in id order
        q = np.clip(((pos - pos.min(0)) / (pos.max(0) - pos.min(0)) * 1024).astype(np.int64), 0, 1023)
        assert (q.max(0) == 1023).all()                                       # points exactly on the box maximum clamp to 1023
