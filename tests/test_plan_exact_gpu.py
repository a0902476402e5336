"""Graph plans held to tests/_plan_oracle.py, the numpy restatement of the contract: every array the plan code hands to the
kernels - row pointers, columns, permutations, 1 / max(1, degree), the cross map and source weights of the saved-mask backward,
narrowed traces, the renumbering's ranks and relabelled index arrays, norm group ids, per-level batch vectors - must EQUAL the
restatement, on every build route (STIN_PLAN_SORT = 0, 1, unset) and in every batched form.  Nothing here compares one route
of the library with another, and nothing depends on how a plan is built (block sizes, workspace layout, counter order), so
these tests are meant to stay green across a rewrite of the build.

Outputs of the raw builds live in the middle of sentinel-filled buffers: the prefix up to rowptr[-1] equals the restatement, the
slots behind it still hold the sentinel (dropped pairs leave them unwritten) and the guards around the view are untouched.  A
guard is as long as twice the batch's pair count, so even a slot computed from another job's offsets stays inside the buffer."""
import ctypes

import numpy as np
import pytest
import torch

import _plan_oracle as O
from surface_texture_inpainting_net_amd import _lib
from surface_texture_inpainting_net_amd import functional as SF
from surface_texture_inpainting_net_amd import plan as P
from surface_texture_inpainting_net_amd.data import collate
from surface_texture_inpainting_net_amd.synthetic import make_synthetic_mesh

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ISENT, FSENT = -77, -7.0
ROUTES = ['0', '1', None]
ROUTE_IDS = ['counting', 'sort', 'default']


def _set_route(monkeypatch, route):
    if route is None:
        monkeypatch.delenv('STIN_PLAN_SORT', raising=False)
    else:
        monkeypatch.setenv('STIN_PLAN_SORT', route)


def _other(route):
    return '0' if route == '1' else '1'                  # (unset takes the counting route at these sizes)


def _dev(a, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


class Guarded:
    """n elements in the middle of a buffer filled with a sentinel, `guard` elements on either side."""

    def __init__(self, n, dtype, guard):
        self.n, self.g = n, guard
        self.sent = FSENT if dtype.is_floating_point else ISENT
        self.wide = torch.full((2 * guard + max(n, 1),), self.sent, dtype=dtype, device=DEV)
        self.view = self.wide[guard:guard + n]

    def host(self):
        return self.view.cpu().numpy()

    def guards_untouched(self):
        w = self.wide
        return bool((w[:self.g] == self.sent).all()) and bool((w[self.g + self.n:] == self.sent).all())

    def untouched(self):
        return bool((self.wide == self.sent).all())


class Spec:
    """One plan job on host arrays + what the restatement says it must produce (computed once, shared by every run).
    Non-pair: rows = a, values = b (None: the pair id).  Pair: a = targets, b = sources, both CSRs."""

    def __init__(self, a, b, N, b_limit=0, pair=False, perm=False, narrow=False, inv_deg=True, xslot=True, w_src=True):
        self.a = np.asarray(a, dtype=np.int64).reshape(-1)
        self.b = None if b is None else np.asarray(b, dtype=np.int64).reshape(-1)
        self.E, self.N, self.pair = self.a.size, N, pair
        self.b_limit = N if pair else b_limit
        self.perm, self.narrow, self.inv_deg = perm, narrow, inv_deg or (pair and w_src)
        self.xslot, self.w_src = pair and (xslot or w_src), pair and w_src
        self._want = None

    def want(self):
        if self._want is None:
            w = {}
            w['rowptr0'], w['col0'], w['perm0'], w['inv_deg0'], w['narrow_out'], w['bad'] = O.csr(self.a, self.b, self.N, self.b_limit)
            if self.pair:
                p = O.edge_pair(self.b, self.a, self.N)
                assert np.array_equal(p.rowptr_dst, w['rowptr0']) and np.array_equal(p.col_dst, w['col0'])
                w['rowptr1'], w['col1'], w['xslot'], w['w_src'] = p.rowptr_src, p.col_src, p.xslot, p.w_src
            self._want = w
        return self._want


class Bound:
    """The device side of one Spec for one run: inputs and guarded outputs."""

    def __init__(self, spec, guard, null_rowptr0=False):
        s = self.spec = spec
        self.a = _dev(s.a)
        self.b = None if s.b is None else _dev(s.b)
        i32, f32 = torch.int32, torch.float32
        o = self.out = {}
        if not null_rowptr0:
            o['rowptr0'] = Guarded(s.N + 1, i32, guard)
        o['col0'] = Guarded(s.E, i32, guard)
        if s.perm:
            o['perm0'] = Guarded(s.E, i32, guard)
        if s.inv_deg:
            o['inv_deg0'] = Guarded(s.N, f32, guard)
        if s.narrow:
            o['narrow_out'] = Guarded(s.E, i32, guard)
        if s.pair:
            o['rowptr1'] = Guarded(s.N + 1, i32, guard)
            o['col1'] = Guarded(s.E, i32, guard)
            if s.xslot:
                o['xslot'] = Guarded(s.E, i32, guard)
            if s.w_src:
                o['w_src'] = Guarded(s.E, f32, guard)

    def add(self, jobs):
        s, v = self.spec, lambda k: self.out[k].view if k in self.out else None
        jobs.add(self.a, self.b, s.E, s.N, s.b_limit, int(s.pair), v('rowptr0'), v('col0'), v('perm0'), v('inv_deg0'), v('rowptr1'),
                 v('col1'), v('xslot'), v('w_src'), narrow_out=v('narrow_out'))

    def check(self, tag):
        w = self.spec.want()
        valid = int(w['rowptr0'][-1])
        for name, g in self.out.items():
            got, want = g.host(), w[name]
            if name in ('col0', 'perm0', 'col1', 'xslot', 'w_src'):          # entries: a prefix, dropped pairs leave the rest alone
                assert want.size == valid, (tag, name)
                assert np.array_equal(got[:valid], want), (tag, name)
                assert (got[valid:] == g.sent).all(), (tag, name, 'slots behind rowptr[-1] were written')
            else:
                assert got.shape == want.shape and np.array_equal(got, want), (tag, name)
            assert g.guards_untouched(), (tag, name, 'guard')

    def untouched(self):
        return all(g.untouched() for g in self.out.values())


def _build_once(specs, tag):
    """The specs as ONE PlanJobs (run() splits it when it must); every output against the restatement; -> the bad flag."""
    guard = 2 * sum(s.E for s in specs) + 8
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    jobs = P.PlanJobs()
    bound = [Bound(s, guard) for s in specs]
    for b in bound:
        b.add(jobs)
    jobs.run(bad, torch.device(DEV))
    torch.cuda.synchronize()
    for i, b in enumerate(bound):
        b.check((tag, 'job %d of %d' % (i, len(bound))))
    return int(bad.item())


def _exact(specs, route, monkeypatch, tag=''):
    """Under `route`, then the other route on the same-sized problem (the caching allocator hands its workspace back with that
    route's leftovers), then `route` again: each run against the restatement."""
    want_bad = any(s.want()['bad'] for s in specs)
    for r in (route, _other(route), route):
        _set_route(monkeypatch, r)
        bad = _build_once(specs, (tag, 'STIN_PLAN_SORT', r))
        assert (bad != 0) == want_bad, (tag, r, bad)


def _three_forms(src, dst, n):
    """A family as a non-pair job, a pair job and a pool job with narrow_out."""
    return [Spec(dst, src, n, b_limit=n, perm=True), Spec(dst, src, n, pair=True), Spec(dst, None, n, narrow=True)]


# ------------------------------------------------------------------------------------------------------------ graph families
def _family(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == 'uniform':
        n, e = 4099, 30011
        return rng.integers(0, n, e), rng.integers(0, n, e), n
    if name == 'hub':                                         # vertex 7: target of 1 500 edges, source of 1 500 others
        n, h = 2000, 7
        src = np.concatenate([rng.integers(0, n, 1500), np.full(1500, h), rng.integers(0, n, 500)])
        dst = np.concatenate([np.full(1500, h), rng.integers(0, n, 1500), rng.integers(0, n, 500)])
        mix = rng.permutation(src.size)
        return src[mix], dst[mix], n
    if name == 'into_row_0':
        return rng.integers(0, 300, 1000), np.zeros(1000, dtype=np.int64), 300
    if name == 'into_last_row':
        return rng.integers(0, 300, 1000), np.full(1000, 299), 300
    if name == 'ends_empty':                                  # rows 0 and n - 1 empty on both sides
        return rng.integers(1, 499, 3000), rng.integers(1, 499, 3000), 500
    if name == 'loops_and_duplicates':
        v = rng.integers(0, 3, 700)
        return v, v.copy(), 3
    if name == 'no_edges_n1':
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 1
    if name == 'no_edges_n1000':
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 1000
    if name == 'one_vertex':
        return np.zeros(300, dtype=np.int64), np.zeros(300, dtype=np.int64), 1
    raise KeyError(name)


FAMILIES = ['uniform', 'hub', 'into_row_0', 'into_last_row', 'ends_empty', 'loops_and_duplicates', 'no_edges_n1', 'no_edges_n1000',
            'one_vertex']
_FAMILY_SPECS = {}


def _family_specs(name):
    if name not in _FAMILY_SPECS:
        _FAMILY_SPECS[name] = _three_forms(*_family(name))
    return _FAMILY_SPECS[name]


@pytest.mark.parametrize('route', ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize('family', FAMILIES)
def test_single_jobs_on_graph_families(family, route, monkeypatch):
    for form, spec in zip(('csr', 'pair', 'pool'), _family_specs(family)):
        assert not spec.want()['bad']
        _exact([spec], route, monkeypatch, (family, form))


# --------------------------------------------------------------------------------------------------------------- block edges
_BLOCK_SPECS = {}


def _block_specs(e, where):
    if (e, where) not in _BLOCK_SPECS:
        rng = np.random.default_rng(e + where)
        sizes = [100, 300, 77]
        sizes[where] = e
        specs = []
        for i, (ne, n) in enumerate(zip(sizes, (37, 64, 129))):
            a, b = rng.integers(0, n, ne), rng.integers(0, n, ne)
            specs.append(Spec(a, b, n, pair=True, narrow=True) if i != 1 else Spec(a, b, n, b_limit=n, perm=True))
        _BLOCK_SPECS[(e, where)] = specs
    return _BLOCK_SPECS[(e, where)]


@pytest.mark.parametrize('route', ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize('where', [0, 1], ids=['first', 'middle'])
@pytest.mark.parametrize('e', [255, 256, 257, 512])
def test_pair_counts_at_the_edges_of_a_block(e, where, route, monkeypatch):
    """A job whose pair count is one short of, exactly, or one past a multiple of the 256-thread block, as the first and the
    middle job of a batch: the next job's first pair is the first thread of a block, or is not."""
    _exact(_block_specs(e, where), route, monkeypatch, (e, where))


# -------------------------------------------------------------------------------------------------------- out-of-range pairs
def _bad_case(name):
    rng = np.random.default_rng(11)
    n, e = 50, 400
    src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
    if name == 'negative_source':
        src[123] = -1
    elif name == 'target_equal_n':
        dst[200] = n
    elif name == 'both_in_one_edge':
        src[77], dst[77] = -5, n + 3
    elif name == 'first_and_last_edge':
        src[0], dst[e - 1] = n, -1
    elif name == 'all_edges':
        src = src + n
    return src, dst, n


BAD_CASES = ['negative_source', 'target_equal_n', 'both_in_one_edge', 'first_and_last_edge', 'all_edges']
_BAD_SPECS = {}


@pytest.mark.parametrize('route', ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize('case', BAD_CASES)
def test_out_of_range_pairs_are_flagged_and_left_out(case, route, monkeypatch):
    if case not in _BAD_SPECS:
        src, dst, n = _bad_case(case)
        _BAD_SPECS[case] = _three_forms(src, dst, n) + [Spec(src, None, n, narrow=True)]      # (pool forms on either endpoint)
    specs = _BAD_SPECS[case]
    assert specs[0].want()['bad'] and specs[1].want()['bad']   # (a pool form is bad only when ITS endpoint is)
    assert specs[2].want()['bad'] or specs[3].want()['bad']
    for form, spec in zip(('csr', 'pair', 'pool', 'pool_src'), specs):
        _exact([spec], route, monkeypatch, (case, form))      # asserts the flag: non-zero exactly where the restatement says
    if case == 'all_edges':
        assert not specs[0].want()['rowptr0'].any() and not specs[1].want()['rowptr1'].any()
    _exact(specs[:3], route, monkeypatch, (case, 'batch'))


# ------------------------------------------------------------------------------------------------------- sort bit boundaries
_BIT_SPECS = {}


def _bit_spec(N, pair):
    if (N, pair) not in _BIT_SPECS:
        rng = np.random.default_rng(N)
        e = 2000
        a, b = rng.integers(0, N, e), rng.integers(0, N, e)
        a[5], a[1500], b[9], b[1999] = N - 1, N - 1, N - 1, N - 1     # entries in the last row of either side
        a[700], b[700] = 3, N                                          # one dropped pair (its target row 3 is in range)
        _BIT_SPECS[(N, pair)] = Spec(a, b, N, pair=True, narrow=True) if pair else Spec(a, b, N, b_limit=N, perm=True, narrow=True)
    return _BIT_SPECS[(N, pair)]


@pytest.mark.parametrize('route', ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize('N,pair', [(1022, False), (1023, False), (1024, False), (511, True), (512, True)])
def test_counter_totals_around_a_power_of_two(N, pair, route, monkeypatch):
    """The number of counters of the batch ((pair ? 2 : 1) N + 1 = 1023, 1024, 1025) on either side of 2^10: a key one past
    the last row (the dropped pair) must still sort behind the last row."""
    spec = _bit_spec(N, pair)
    w = spec.want()
    last = w['rowptr1'] if pair else w['rowptr0']
    assert w['bad'] and last[-1] - last[-2] >= 2
    _exact([spec], route, monkeypatch, (N, pair))


# ------------------------------------------------------------------------------------------------------------------- batches
def _random_spec(rng, kind, n, e, spoil=False):
    a, b = rng.integers(0, max(n, 1), e), rng.integers(0, max(n, 1), e)
    if spoil and e > 2:
        a[e // 2], b[1] = n, -1
    if kind == 'pair':
        return Spec(a, b, n, pair=True)
    if kind == 'pair_bare':
        return Spec(a, b, n, pair=True, xslot=False, w_src=False, inv_deg=False)
    if kind == 'pair_xslot':
        return Spec(a, b, n, pair=True, w_src=False, perm=True)
    if kind == 'pool':
        return Spec(a, None, n, narrow=True)
    if kind == 'ids':
        return Spec(a, None, n, perm=True, inv_deg=False)
    return Spec(a, b, n, b_limit=max(n, 1), perm=True, narrow=(kind == 'csr_narrow'))


_SIXTEEN = []


def _sixteen():
    if not _SIXTEEN:
        rng = np.random.default_rng(16)
        plan = [('pair', 5, 0), ('pair', 4099, 9000), ('pool', 300, 1000), ('csr', 7, 513), ('pair', 1, 40), ('pool', 1000, 3000),
                ('ids', 64, 256), ('csr', 1000, 0), ('pair_bare', 33, 700), ('pair_xslot', 65, 511), ('csr_narrow', 2, 257),
                ('pair', 129, 1025, True), ('pool', 40, 90, True), ('pair', 2000, 5000), ('csr', 3, 255), ('pair', 0, 0)]
        _SIXTEEN.extend(_random_spec(rng, *p) for p in plan)
    return _SIXTEEN


@pytest.mark.parametrize('route', ROUTES, ids=ROUTE_IDS)
def test_a_full_batch_of_sixteen_mixed_jobs(route, monkeypatch):
    """Exactly STIN_PLAN_MAX_JOBS jobs: pair / non-pair / val = None / narrow_out / perm0 mixed, an empty job first, in the middle
    and last (the last with N = 0), row counts from 0 to 4099."""
    specs = _sixteen()
    assert len(specs) == P.JOBS_MAX == 16
    assert specs[0].E == 0 and specs[7].E == 0 and specs[15].E == 0 and specs[15].N == 0
    _exact(specs, route, monkeypatch, 'sixteen')


_MANY = {}


def _many(k):
    if k not in _MANY:
        rng = np.random.default_rng(k)
        kinds = ['pair', 'pool', 'csr', 'pair_xslot', 'ids', 'csr_narrow', 'pair_bare']
        _MANY[k] = [_random_spec(rng, kinds[i % len(kinds)], int(rng.integers(1, 400)), int(rng.integers(0, 900)) if i % 11 != 3 else 0)
                    for i in range(k)]
    return _MANY[k]


@pytest.mark.parametrize('route', ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize('k', [17, 33])
def test_more_jobs_than_one_batch_holds(k, route, monkeypatch):
    """PlanJobs.run splits at STIN_PLAN_MAX_JOBS: one job past one batch, and one past two."""
    _exact(_many(k), route, monkeypatch, k)


def _raw_call(bound, n_jobs, ws_short=0):
    lib = _lib.load()
    jobs = P.PlanJobs()
    for b in bound:
        b.add(jobs)
    ws_bytes = lib.stin_plan_build_workspace_bytes(jobs.total_e, jobs.total_cnt)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    blob = b''.join(jobs.blobs)
    buf = ctypes.create_string_buffer(blob, len(blob))
    rc = lib.stin_plan_build_many(buf, n_jobs, P._ptr(bad), P._ptr(ws), ws_bytes - ws_short, P._stream(ws))
    torch.cuda.synchronize()
    return rc, int(bad.item())


@pytest.mark.parametrize('route', ROUTES, ids=ROUTE_IDS)
def test_refusals_write_nothing(route, monkeypatch):
    _set_route(monkeypatch, route)
    C = _lib.CONSTANTS
    specs = _many(17)
    guard = 2 * sum(s.E for s in specs) + 8
    bound = [Bound(s, guard) for s in specs]
    assert _raw_call(bound, 17) == (C['STIN_E_SIZE'], 0)                       # one job more than a batch holds
    assert all(b.untouched() for b in bound)
    assert _raw_call(bound[:3], 3, ws_short=1) == (C['STIN_E_WORKSPACE'], 0)   # a workspace one byte short
    assert all(b.untouched() for b in bound)
    holed = [Bound(specs[0], guard), Bound(specs[1], guard, null_rowptr0=True), Bound(specs[2], guard)]
    assert _raw_call(holed, 3) == (C['STIN_E_NULL'], 0)                        # rowptr0 of the middle job missing
    assert all(b.untouched() for b in holed)
    rc, bad = _raw_call(bound[:16], 16)                                        # ... and the same buffers are filled when all is well
    assert rc == 0
    for i, b in enumerate(bound[:16]):
        b.check(('after the refusals', i))
    assert (bad != 0) == any(s.want()['bad'] for s in specs[:16])


# ---------------------------------------------------------------------------------- EdgeSet / PoolMap as the model builds them
def _np(t):
    return t.cpu().numpy()


def _check_edge_set(es, p, tag):
    nv = int(p.rowptr_dst[-1])
    assert np.array_equal(_np(es.by_dst.rowptr), p.rowptr_dst), tag
    assert np.array_equal(_np(es.by_src.rowptr), p.rowptr_src), tag
    assert np.array_equal(_np(es.by_dst.col)[:nv], p.col_dst), tag
    assert np.array_equal(_np(es.by_src.col)[:nv], p.col_src), tag
    assert np.array_equal(_np(es.xslot)[:nv], p.xslot), tag
    assert np.array_equal(_np(es.w_src)[:nv], p.w_src), tag
    assert np.array_equal(_np(es.inv_deg), p.inv_deg) and es.inv_deg is es.by_dst.inv_deg, tag
    assert es.w_src.dtype == torch.float32 and es.xslot.dtype == torch.int32, tag


def _check_children(pm, rowptr, col, inv_count, trace, tag):
    nv = int(rowptr[-1])
    assert np.array_equal(_np(pm.children.rowptr), rowptr), tag
    assert np.array_equal(_np(pm.children.col)[:nv], col), tag
    assert np.array_equal(_np(pm.inv_count), inv_count) and pm.inv_count is pm.children.inv_deg, tag
    assert pm.trace.dtype == torch.int32 and np.array_equal(_np(pm.trace), trace), tag


_CLASS_CASES = {}


def _class_case(name):
    if name not in _CLASS_CASES:
        if name in BAD_CASES:
            src, dst, n = _bad_case(name)
        else:
            src, dst, n = _family(name)
        rng = np.random.default_rng(len(name))
        nf = dst.size                                              # dst read as a trace: n_fine = E fine vertices -> n coarse
        rank_c = np.append(rng.permutation(n), n)
        rank_f = np.append(rng.permutation(nf), nf)
        ren = O.relabel_trace(dst, rank_c, n, rank_f)
        _CLASS_CASES[name] = dict(src=src, dst=dst, n=n, pair=O.edge_pair(src, dst, n), pool=O.pool_map(dst, nf, n), ren=ren,
                                  ren_csr=O.csr(ren[0], ren[1], n, nf), rank_c=rank_c, rank_f=rank_f)
    return _CLASS_CASES[name]


@pytest.mark.parametrize('route', ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize('name', FAMILIES + ['negative_source', 'first_and_last_edge', 'all_edges'])
def test_edge_sets_and_pool_maps_as_the_model_builds_them(name, route, monkeypatch):
    c = _class_case(name)
    n, nf = c['n'], c['dst'].size
    for r in (route, _other(route)):
        _set_route(monkeypatch, r)
        bad = torch.zeros(1, dtype=torch.int32, device=DEV)
        es = P.EdgeSet(torch.stack([_dev(c['src']), _dev(c['dst'])]), n, bad)
        _check_edge_set(es, c['pair'], (name, r))
        assert (int(bad.item()) != 0) == c['pair'].bad
        bad.zero_()
        pm = P.PoolMap(_dev(c['dst']), nf, n, bad)
        rowptr, col, inv_count, narrow, pool_bad = c['pool']
        _check_children(pm, rowptr, col, inv_count, narrow, (name, r, 'pool'))
        assert (int(bad.item()) != 0) == pool_bad
        bad.zero_()
        coarse_new, fine_new, trace_new = c['ren']
        pr = P.PoolMap(_dev(c['dst']), nf, n, bad, renumbered=(_dev(coarse_new), _dev(fine_new), _dev(trace_new, torch.int32)))
        rowptr_r, col_r, _, inv_r, _, ren_bad = c['ren_csr']
        _check_children(pr, rowptr_r, col_r, inv_r, trace_new, (name, r, 'renumbered'))
        assert (int(bad.item()) != 0) == ren_bad == pool_bad
        # the docstring's promise: the children list of a coarse vertex keeps the original order of its members
        for cv in list(range(min(n, 40))) + [n - 1]:
            kids = col[rowptr[cv]:rowptr[cv + 1]]
            new = c['rank_c'][cv]
            assert np.array_equal(col_r[rowptr_r[new]:rowptr_r[new + 1]], c['rank_f'][kids]), (name, cv)


# ---------------------------------------------------------------------------------------------------------------- renumbering
def _order_case(kind, n0, variant):
    """-> (x [n0, C] fp32, first position column, traces, sizes)"""
    rng = np.random.default_rng(n0 + len(variant))
    pos = O.positions(kind, n0, n0 + 1).copy()
    n1, n2 = max(1, n0 // 3), max(1, n0 // 9)
    t1, t2 = rng.integers(0, n1, n0), rng.integers(0, n2, n1)
    x, col = pos, 0
    if variant == 'constant_axis':
        pos[:, 2] = pos[0, 2]
    elif variant == 'columns_6_to_9':
        x = rng.standard_normal((n0, 10)).astype(np.float32)
        x[:, 6:9] = pos
        col = 6
    elif variant == 'holes':                                  # childless coarse vertices and out-of-range trace entries
        t1 = rng.integers(0, max(1, n1 - n1 // 3), n0)
        t1[::7] = n1 + (np.arange(t1[::7].size) % 3) * 2 ** 33
        t2 = rng.integers(-1, n2 + 1, n1)
    return x, col, pos, [t1, t2], [n0, n1, n2]


def _run_vertex_order(x, col, traces, sizes, want_order=(True, False, True)):
    lib = _lib.load()
    st = _lib.STRUCTS['stin_order_level_t']
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    guard = max(sizes) + 8
    ranks = [Guarded(n + 1, torch.int32, guard) for n in sizes]
    orders = [Guarded(n, torch.int32, guard) if w else None for n, w in zip(sizes, want_order)]
    trs = [None] + [_dev(t) for t in traces]
    ws_bytes = lib.stin_vertex_order_workspace_bytes(max(sizes))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    blob = b''.join(st.pack(n=n, trace=P._ptr(trs[l]), rank=P._ptr(ranks[l].view), order=P._ptr(orders[l].view) if orders[l] else 0)
                    for l, n in enumerate(sizes))
    buf = ctypes.create_string_buffer(blob, len(blob))
    _lib.check(lib.stin_vertex_order_f32(xd.data_ptr() + 4 * col, xd.stride(0), buf, len(sizes), P._ptr(ws), ws_bytes, P._stream(ws)),
               'stin_vertex_order_f32')
    torch.cuda.synchronize()
    return ranks, orders


@pytest.mark.parametrize('variant', ['plain', 'constant_axis', 'columns_6_to_9', 'holes'])
@pytest.mark.parametrize('kind', ['lattice', 'normal'])
@pytest.mark.parametrize('n0', [1, 2, 255, 257, 3000])
def test_vertex_order_on_three_levels(n0, kind, variant):
    """stin_vertex_order_f32 against the restatement.  The lattice family needs no rounding at all (multiples of 1/8, extents that
    are powers of two) and is full of coincident points - tied codes keep id order - with several points on the box maximum."""
    x, col, pos, traces, sizes = _order_case(kind, n0, variant)
    want_ranks, want_order0 = O.vertex_order(pos, traces, sizes)
    ranks, orders = _run_vertex_order(x, col, traces, sizes)
    for lvl, (g, want) in enumerate(zip(ranks, want_ranks)):
        assert np.array_equal(g.host(), want), (lvl, 'rank')
        assert g.guards_untouched(), lvl
    assert np.array_equal(orders[0].host(), want_order0) and orders[0].guards_untouched()
    inv2 = np.argsort(want_ranks[2][:-1], kind='stable')
    assert np.array_equal(orders[2].host(), inv2) and orders[2].guards_untouched()
    if kind == 'lattice' and n0 >= 255:
        codes = O.morton_codes(pos)
        assert np.unique(codes).size <= n0 // 3 and (codes == codes.max()).sum() >= 2


def _relabel_jobs():
    """16 jobs: edge arrays and traces, ids at -1, at limit and at 2^40, an n = 0 job in the middle (job 7)."""
    rng = np.random.default_rng(77)
    jobs = []
    for i in range(16):
        limit, nf = int(rng.integers(1, 300)), int(rng.integers(1, 500))
        rank = np.append(rng.permutation(limit), limit).astype(np.int32)
        if i == 7:
            jobs.append(dict(ids=np.zeros(0, dtype=np.int64), rank=rank, limit=limit, rank_fine=None))
        elif i % 3 == 1:                                      # a trace [nf] with the fine level's ranks
            ids = rng.integers(0, limit, nf)
            ids[::5] = np.resize([-1, limit, 2 ** 40], ids[::5].size)
            jobs.append(dict(ids=ids, rank=rank, limit=limit, rank_fine=np.append(rng.permutation(nf), nf).astype(np.int32)))
        else:                                                 # an edge array [2, E]
            ids = rng.integers(0, limit, (2, nf))
            ids[0, ::4] = np.resize([limit, 2 ** 40, -1, -2 ** 40], ids[0, ::4].size)
            jobs.append(dict(ids=ids, rank=rank, limit=limit, rank_fine=None))
    return jobs


def test_relabel_batch_with_an_empty_job_in_the_middle():
    lib = _lib.load()
    st = _lib.STRUCTS['stin_relabel_job_t']
    jobs, blobs, outs, keep = _relabel_jobs(), [], [], []
    assert len(jobs) == _lib.CONSTANTS['STIN_RELABEL_MAX_JOBS'] and jobs[7]['ids'].size == 0
    for j in jobs:
        n = j['ids'].size
        ids, rank = _dev(j['ids'].reshape(-1)), _dev(j['rank'], torch.int32)
        out = Guarded(n, torch.int64, 600)
        fine = trace = rf = None
        if j['rank_fine'] is not None:
            rf, fine, trace = _dev(j['rank_fine'], torch.int32), Guarded(n, torch.int64, 600), Guarded(n, torch.int32, 600)
        keep.append((ids, rank, rf))
        outs.append((out, fine, trace))
        blobs.append(st.pack(ids=P._ptr(ids), n=n, rank=P._ptr(rank), limit=j['limit'], out=P._ptr(out.view), rank_fine=P._ptr(rf),
                             fine_out=P._ptr(fine.view) if fine else 0, trace_out=P._ptr(trace.view) if trace else 0))
    buf = ctypes.create_string_buffer(b''.join(blobs), len(blobs) * st.size)
    _lib.check(lib.stin_relabel_many_i64(buf, len(blobs), P._stream(keep[0][0])), 'stin_relabel_many_i64')
    torch.cuda.synchronize()
    for i, (j, (out, fine, trace)) in enumerate(zip(jobs, outs)):
        if j['rank_fine'] is None:
            assert np.array_equal(out.host(), O.relabel(j['ids'], j['rank'], j['limit']).reshape(-1)), i
        else:
            coarse_new, fine_new, trace_new = O.relabel_trace(j['ids'], j['rank'], j['limit'], j['rank_fine'])
            assert np.array_equal(out.host(), coarse_new), i
            assert np.array_equal(fine.host(), fine_new) and fine.guards_untouched(), i
            assert np.array_equal(trace.host(), trace_new) and trace.guards_untouched(), i
        assert out.guards_untouched(), i


_SAMPLE = {}


def _sample():
    """The smoke-sized synthetic sample, its restated renumbering and both restated plans (computed once, never modified)."""
    if not _SAMPLE:
        s = make_synthetic_mesh(3000, 3, seed=23, dilations=(2, 4))
        sizes = [int(v) for v in s.num_vertices.reshape(-1)]
        edges = [('edge_index', 0), ('hierarchy_edge_index_1', 1), ('hierarchy_edge_index_2', 2), ('hierarchy_dil_2_edge_index_2', 2),
                 ('hierarchy_dil_4_edge_index_2', 2)]
        traces = [s['hierarchy_trace_index_%d' % l].numpy() for l in (1, 2)]
        ranks, order0 = O.vertex_order(s.x[:, 6:9].numpy(), traces, sizes)
        plain, moved = {}, {}
        for key, lvl in edges:
            ei = s[key].numpy()
            plain[key] = O.edge_pair(ei[0], ei[1], sizes[lvl])
            ej = O.relabel(ei, ranks[lvl], sizes[lvl])
            moved[key] = O.edge_pair(ej[0], ej[1], sizes[lvl])
        for lvl in (1, 2):
            plain[lvl] = O.pool_map(traces[lvl - 1], sizes[lvl - 1], sizes[lvl])[:4]
            coarse_new, fine_new, trace_new = O.relabel_trace(traces[lvl - 1], ranks[lvl], sizes[lvl], ranks[lvl - 1])
            rowptr, col, _, inv_count, _, _ = O.csr(coarse_new, fine_new, sizes[lvl], sizes[lvl - 1])
            moved[lvl] = (rowptr, col, inv_count, trace_new)
        _SAMPLE.update(s=s, sizes=sizes, edges=edges, ranks=ranks, order0=order0, plain=plain, moved=moved)
    return _SAMPLE


def test_twenty_arrays_through_relabel_many(monkeypatch):
    """GraphPlan._relabel_many issues one launch per 16 arrays: 20 arrays take two."""
    c = _sample()
    s = c['s'].to(DEV)
    monkeypatch.setattr(P, 'REORDER_IMPL', 'hip')
    pl = P.GraphPlan(s, positions=(6, 9), reorder=True)
    pl._ensure_order()
    assert pl._hip_order()
    for lvl, want in enumerate(c['ranks']):
        assert pl._ranks[lvl].dtype == torch.int32 and np.array_equal(_np(pl._ranks[lvl]), want), lvl
    assert np.array_equal(_np(pl.order0), c['order0']) and np.array_equal(_np(pl.rank0), c['ranks'][0][:-1])
    items = []
    for rep in range(4):
        for key, lvl in c['edges'][:3]:
            ei = s[key].clone()
            ei[rep % 2, rep::17] = (-1, c['sizes'][lvl], 2 ** 40, 0)[rep]
            items.append(('e', ei, lvl))
        for lvl in (1, 2):
            tr = s['hierarchy_trace_index_%d' % lvl].clone()
            tr[rep::13] = (0, -1, c['sizes'][lvl], 2 ** 40)[rep]
            items.append(('p', tr, lvl))
    assert len(items) == 20
    outs = pl._relabel_many(items)
    torch.cuda.synchronize()
    for i, ((kind, t, lvl), got) in enumerate(zip(items, outs)):
        if kind == 'e':
            assert np.array_equal(_np(got), O.relabel(_np(t), c['ranks'][lvl], c['sizes'][lvl])), i
        else:
            want = O.relabel_trace(_np(t), c['ranks'][lvl], c['sizes'][lvl], c['ranks'][lvl - 1])
            for g, w in zip(got, want):
                assert np.array_equal(_np(g), w), i
            assert got[2].dtype == torch.int32 and got[0].dtype == torch.int64


# ---------------------------------------------------------------------------------------------------------------- whole plans
@pytest.mark.parametrize('sort', ['0', '1'], ids=['counting', 'sort'])
@pytest.mark.parametrize('reorder,impl', [(False, 'hip'), (True, 'torch'), (True, 'hip')], ids=['as_given', 'renumbered_torch', 'renumbered_hip'])
def test_whole_plans(reorder, impl, sort, monkeypatch):
    """Every structure GraphPlan.ensure builds for a three-level sample with dilated sets against the restatement's plan of the
    same sample - relabelled by the restatement's OWN ranks when the plan renumbers - and what _ensure_order promises: every
    destination row and every children list, mapped back through the order, lists the same members in the same sequence as the
    plan of the sample as given."""
    c = _sample()
    s = c['s'].to(DEV)
    monkeypatch.setenv('STIN_PLAN_SORT', sort)
    monkeypatch.setattr(P, 'REORDER_IMPL', impl)
    pl = P.GraphPlan(s, positions=(6, 9), reorder=reorder)
    pl.ensure(c['edges'], [1, 2])
    pl.validate()
    torch.cuda.synchronize()
    want = c['moved'] if reorder else c['plain']
    if reorder:
        for lvl, r in enumerate(c['ranks']):
            assert np.array_equal(_np(pl._ranks[lvl]).astype(np.int64), r), lvl
        assert np.array_equal(_np(pl.order0), c['order0']) and np.array_equal(_np(pl.rank0), c['ranks'][0][:-1])
    else:
        assert pl._ranks is None and pl.order0 is None
    for key, lvl in c['edges']:
        _check_edge_set(pl._edges[key], want[key], key)
    for lvl in (1, 2):
        _check_children(pl._pools[lvl], *want[lvl], tag=lvl)
    if not reorder:
        return
    orders = [np.argsort(_np(r)[:-1].astype(np.int64), kind='stable') for r in pl._ranks]     # new -> old, from the PLAN's ranks
    for key, lvl in c['edges']:
        got, base, order = pl._edges[key].by_dst, c['plain'][key], orders[lvl]
        rowptr, col = _np(got.rowptr), _np(got.col)
        for new in range(c['sizes'][lvl]):
            old = order[new]
            assert np.array_equal(order[col[rowptr[new]:rowptr[new + 1]]], base.col_dst[base.rowptr_dst[old]:base.rowptr_dst[old + 1]]), (key, new)
    for lvl in (1, 2):
        got, (b_rowptr, b_col, _, b_trace) = pl._pools[lvl], c['plain'][lvl]
        rowptr, col = _np(got.children.rowptr), _np(got.children.col)
        for new in range(c['sizes'][lvl]):
            old = orders[lvl][new]
            assert np.array_equal(orders[lvl - 1][col[rowptr[new]:rowptr[new + 1]]], b_col[b_rowptr[old]:b_rowptr[old + 1]]), (lvl, new)
        assert np.array_equal(orders[lvl][_np(got.trace)[_np(pl._ranks[lvl - 1])[:-1].astype(np.int64)]], b_trace), lvl


# ------------------------------------------------------------------------------------------------------------------------ ids
@pytest.mark.parametrize('quirk', [True, False], ids=['linspace_slices', 'true_ranges'])
@pytest.mark.parametrize('counts', [[37], [10, 27], [300, 1, 213], [5, 0, 9], [40, 3, 0, 77, 13, 256, 12]],
                         ids=['B1', 'B2', 'B3', 'B3_empty_graph', 'B7'])
def test_norm_group_ids(counts, quirk):
    """NormGroups.gid / sid: graph id per row, and the slice of the sums - the reference's linspace(0, N, B + 1) slices with the
    quirk, the true ranges without.  Unequal counts, a graph of zero vertices, row counts that B does not divide."""
    B, n = len(counts), sum(counts)
    assert B == 1 or n % B != 0
    batch = np.repeat(np.arange(B), counts)
    ng = P.NormGroups(n, torch.device(DEV), _dev(batch), torch.tensor(counts, dtype=torch.int64), linspace_quirk=quirk)
    torch.cuda.synchronize()
    true_ptr = np.concatenate([[0], np.cumsum(counts)])
    sum_ptr = torch.linspace(0, n, B + 1, dtype=torch.int).numpy().astype(np.int64) if quirk else true_ptr
    assert np.array_equal(_np(ng.ptr_true), true_ptr) and np.array_equal(_np(ng.ptr_sum), sum_ptr)
    assert sum_ptr[0] == 0 and sum_ptr[-1] == n and (np.diff(sum_ptr) >= 0).all()
    assert ng.quirk == bool((sum_ptr != true_ptr).any())
    gid, sid = O.norm_group_ids(batch, sum_ptr)
    assert ng.gid.dtype == torch.int32 and np.array_equal(_np(ng.gid), gid)
    assert ng.sid.dtype == torch.int32 and np.array_equal(_np(ng.sid), sid)
    if quirk and B > 1:
        assert ng.quirk and ng.sid is not ng.gid


def test_batch_vectors_of_a_batched_sample():
    """GraphPlan.batch_vector (SF.batch_pool going down the levels) and SF.batch_unpool against scatter_max(batch, trace) and
    batch[trace] on three graphs of unequal size."""
    s = collate([make_synthetic_mesh(n, 3, seed=30 + i, dilations=(2,)) for i, n in enumerate((400, 900, 150))])
    sizes = [int(v) for v in s.num_vertices.sum(0)]
    sd = s.to(DEV)
    pl = P.GraphPlan(sd)
    want = s.batch.numpy()
    assert np.array_equal(_np(pl.batch_vector(0)), want)
    for lvl in (1, 2):
        trace = s['hierarchy_trace_index_%d' % lvl].numpy()
        coarse = O.batch_pool(want, trace, sizes[lvl])
        got = pl.batch_vector(lvl)
        assert got.dtype == torch.int64 and np.array_equal(_np(got), coarse), lvl
        up = SF.batch_unpool(got, pl.pool(lvl))
        assert up.dtype == torch.int64 and np.array_equal(_np(up), O.batch_unpool(coarse, trace)), lvl
        assert np.array_equal(_np(up), want)                      # (a graph's vertices pool into that graph)
        want = coarse
    pl.validate()
    # a coarse vertex without children takes 0, and the largest id wins among mixed children (no graph structure needed)
    trace = np.array([0, 0, 0, 2, 4, 4, 2])
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    pm = P.PoolMap(_dev(trace), 7, 5, bad)
    for bvec in ([0, 0, 1, 1, 2, 3, 1], [5, 9, 2, 7, 7, 1, 8], [3, 3, 3, 3, 3, 3, 3]):
        got = SF.batch_pool(_dev(np.array(bvec)), pm)
        assert np.array_equal(_np(got), O.batch_pool(bvec, trace, 5)), bvec
