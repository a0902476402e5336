"""The norm kernels (csrc/stin_norm.hip) held to tests/_norm_oracle.py, the numpy restatement of include/stin_hip.h: every
reduction mode and post-operation on the one-launch and on the two-stage route, the fold-trip boundaries of both finalisers and of
the ticket kernel's own fold, the elementwise passes at 8, 4 and 1 channels per lane, the fold forms, the BatchNorm passes.  Every
assertion is EQUALITY with the restatement, compared as integer views - never with a second run or another route of the library.

How that can hold to the bit: x, gout and res are integers in [-8, 8], mean is an integer, so every fp64 sum is exact in any
order; the posts and the elementwise passes are a few IEEE operations that numpy repeats one by one; and wherever an ELU branch is
evaluated rstd is 128 or more, so that xc * rstd is > 0, 0 or <= -128, where exp and expm1 round to 1, 1, 0 and n, 0, -1
(test_elu_values_on_the_lattice checks those against literal constants first).

Every output, and the workspace itself, lies inside a buffer of 0x5A bytes that is compared whole; the workspace has 128 KB of
guard behind it and may change only where the route query says partials are written.  Shapes come from tests/_norm_table.py and
are checked through stin_colreduce_route with the device's CU count before they run."""
import numpy as np
import pytest
import torch

import _norm_oracle as O
import _norm_table as T
from surface_texture_inpainting_net_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 1024                      # bytes on either side of an output
WS_GUARD = 160 * 1024             # bytes on either side of a workspace
K = _lib.CONSTANTS
F = np.float32
EPS = 2.0 ** -14                  # 1 / sqrt(0 + eps) = 128
ONE, TWO = T.ONE, T.TWO
S = O                             # modes and posts by the oracle's names (equal to the header's: test_constants)


@pytest.fixture(autouse=True)
def _end_the_run_after_a_device_fault():
    """A kernel fault poisons the process: end the run instead of launching the remaining tests on a faulted device."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit('device fault, run ended: %s' % e, returncode=3)


def lib():
    return _lib.load()


def cu_count():
    return torch.cuda.get_device_properties(torch.device(DEV)).multi_processor_count


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


class Box:
    """nbytes of device memory in the middle of a 0x5A-filled buffer; `offset` bytes move it off its 16-byte alignment."""

    def __init__(self, nbytes, offset=0, guard=GUARD):
        self.n, self.lo = int(nbytes), guard + offset
        self.wide = torch.full((2 * guard + 16 + (self.n + 15) // 16 * 16,), 0x5A, dtype=torch.uint8, device=DEV)
        assert self.wide.data_ptr() % 256 == 0
        self.ptr = self.wide.data_ptr() + self.lo

    @classmethod
    def of(cls, array, offset=0):
        array = np.ascontiguousarray(array)
        box = cls(array.nbytes, offset)
        box.wide[box.lo:box.lo + box.n] = torch.from_numpy(array.reshape(-1).view(np.uint8).copy()).to(DEV)
        return box

    def holds(self, expected):
        """The first expected.nbytes bytes equal `expected`, every other byte of the buffer still holds the sentinel."""
        expected = np.ascontiguousarray(expected).reshape(-1).view(np.uint8)
        assert expected.size <= self.n
        want = torch.full_like(self.wide, 0x5A, device='cpu')
        want[self.lo:self.lo + expected.size] = torch.from_numpy(expected.copy())
        return torch.equal(self.wide.view(torch.int16), want.to(DEV).view(torch.int16))

    def untouched(self):
        return self.holds(np.zeros(0, np.uint8))

    def untouched_outside(self, lo, hi):
        """Only bytes [lo, hi) of the box itself may differ from the sentinel (a workspace: its partials)."""
        got = self.wide.cpu().numpy()
        return bool((got[:self.lo + lo] == 0x5A).all()) and bool((got[self.lo + hi:] == 0x5A).all())


def sentinel(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8).fill(0x5A)
    return a


def spread(rows, ld):
    """[N, C] -> the (N - 1) ld + C elements it occupies at row pitch ld, sentinel between the rows."""
    n, c = rows.shape
    if n == 0:
        return rows.reshape(-1)
    out = sentinel(n * ld, rows.dtype)
    out.reshape(n, ld)[:, :c] = rows
    return out[:(n - 1) * ld + c]


def rows_box(a, ld, bf16=False, offset=0):
    """An input matrix on the device at row pitch ld (bf16: as bf16 rows; the values are exact in bf16)"""
    a = np.asarray(a, F)
    if bf16:
        bits = O.round_bf16(a)
        assert np.array_equal(O.bf16_to_f32(bits), a)
        return Box.of(spread(bits, ld), offset)
    return Box.of(spread(a, ld), offset)


def p(b):
    return None if b is None else b.ptr


def vecbox(a, dtype=F):
    return None if a is None else Box.of(np.asarray(a, dtype))


def ints(rng, shape, lo=-8, hi=8):
    return rng.integers(lo, hi + 1, shape).astype(F)


def dyadic(rng, shape):
    return rng.choice(np.array([-2, -1.5, -1, -0.5, -0.25, 0.25, 0.5, 1, 1.5, 2], F), shape)


def test_constants():
    names = ('SUM', 'CSQ', 'DOT_ELU', 'COEF_XC', 'MOMENTS', 'DOT_BN', 'DOT_BN_RELU')
    assert tuple(K['STIN_RED_' + n] for n in names) == tuple(getattr(O, 'RED_' + n) for n in names)
    names = ('NONE', 'SCALE', 'RSTD', 'NORM_COEF')
    assert tuple(K['STIN_POST_' + n] for n in names) == tuple(getattr(O, 'POST_' + n) for n in names)


# ------------------------------------------------------------------------------------------------ elementwise runners
def run_fwd(x, mean, rstd, gid=None, res=None, act=1, pad=4, row_map=None, bf16=False, offset=0, want_rc=0):
    """stin_norm_act_res_fwd_{f32,bf16} / _map_f32 on pitched rows (pitch C + pad; the residual C + 2 pad) against the restatement"""
    N, C = x.shape
    ldx, ldy, ldres = C + pad, C + pad, C + 2 * pad
    bx, br = rows_box(x, ldx, bf16, offset), (None if res is None else rows_box(res, ldres, bf16, offset))
    elem = 2 if bf16 else 4
    by = Box(max((N - 1) * ldy + C, 0) * elem if N else 0, offset)
    bm, bs, bg = vecbox(mean), vecbox(rstd), vecbox(gid, np.int32)
    sfx = '_bf16' if bf16 else '_f32'
    if row_map is not None:
        bmap = vecbox(row_map, np.int32)
        rc = lib().stin_norm_act_res_fwd_map_f32(bx.ptr, ldx, bm.ptr, bs.ptr, p(bg), p(br), ldres, bmap.ptr, N, C, act, by.ptr, ldy, stream())
    else:
        rc = getattr(lib(), 'stin_norm_act_res_fwd' + sfx)(bx.ptr, ldx, bm.ptr, bs.ptr, p(bg), p(br), ldres if br else 0, N, C, act, by.ptr, ldy,
                                                         stream())
    assert rc == want_rc, rc
    if rc != 0:
        assert by.untouched()
        return
    want = O.norm_act_res_fwd(x, mean, rstd, gid, res, act, row_map)
    assert by.holds(spread(O.round_bf16(want) if bf16 else want, ldy))


def run_bwd(x, gout, mean, rstd, a, k, m, gid=None, sid=None, act=1, pad=4, bf16=False, offset=0, want_rc=0):
    N, C = x.shape
    ldx, ldg, lddx = C + pad, C + 2 * pad, C + pad
    bx, bg = rows_box(x, ldx, bf16, offset), rows_box(gout, ldg, bf16, offset)
    bd = Box((max((N - 1) * lddx + C, 0) if N else 0) * (2 if bf16 else 4), offset)
    v = [vecbox(t) for t in (mean, rstd, a, k, m)]
    bgid, bsid = vecbox(gid, np.int32), vecbox(sid, np.int32)
    rc = getattr(lib(), 'stin_norm_act_bwd' + ('_bf16' if bf16 else '_f32'))(bx.ptr, ldx, bg.ptr, ldg, *[t.ptr for t in v], p(bgid), p(bsid), N, C,
                                                                           act, bd.ptr, lddx, stream())
    assert rc == want_rc, rc
    if rc != 0:
        assert bd.untouched()
        return
    want = O.norm_act_bwd(x, gout, mean, rstd, a, k, m, gid, sid, act)
    assert bd.holds(spread(O.round_bf16(want) if bf16 else want, lddx))


def test_elu_values_on_the_lattice():
    """ELU and ELU' at n = 0, -128, -1024, 2^-20, 3 through the forward and the backward kernel, against literal constants: the
    values the lattice of every other test relies on (the device's exp(-128) is +0, its expm1(-128) is -1)."""
    x = np.array([[0, -1, -8, 2.0 ** -27, 3.0 / 128]] * 3, F)
    for C, pad in ((5, 1), (5, 3)):                      # one channel per lane
        run_fwd(x[:, :C], np.zeros((1, C), F), np.full((1, C), 128, F), act=1, pad=pad)
    x8 = np.concatenate([x, x[:, :3]], axis=1)           # four channels per lane
    zero, one, r = np.zeros((1, 8), F), np.ones((1, 8), F), np.full((1, 8), 128, F)
    N = 3
    bx, by, bd = Box.of(x8), Box(N * 8 * 4), Box(N * 8 * 4)
    bz, bo, br, bg = Box.of(zero), Box.of(one), Box.of(r), Box.of(np.ones((N, 8), F))
    assert lib().stin_norm_act_res_fwd_f32(bx.ptr, 8, bz.ptr, br.ptr, None, None, 0, N, 8, 1, by.ptr, 8, stream()) == 0
    assert lib().stin_norm_act_bwd_f32(bx.ptr, 8, bg.ptr, 8, bz.ptr, br.ptr, bo.ptr, bz.ptr, bz.ptr, None, None, N, 8, 1, bd.ptr, 8, stream()) == 0
    elu = np.array([0, -1, -1, 2.0 ** -20, 3, 0, -1, -1], F)
    grad = np.array([1, 0, 0, 1, 1, 1, 0, 0], F)
    assert by.holds(np.tile(elu, (N, 1)))
    assert bd.holds(np.tile(grad, (N, 1)))               # g = 1, a = 1, k = m = 0:  dx = 1 * (1 * ELU') + 0 * xc + 0
    # the restatement gives the same constants
    assert np.array_equal(O.elu(x8[0] * F(128)), elu) and np.array_equal(O.elu_grad(x8[0] * F(128)), grad)


# ------------------------------------------------------------------------------------------------ the reductions
def operands(rng, mode, N, C, G, Sn):
    """Integer rows and the per-group vectors of a mode: mean integer, rstd in {128, 256, 512} (the ELU lattice), coef dyadic;
    BatchNorm modes: rstd in {1/4, 1/2, 1}, gamma and beta such that gamma n + beta takes both signs and 0"""
    d = dict(x=ints(rng, (N, C)))
    if mode in (S.RED_DOT_ELU, S.RED_DOT_BN, S.RED_DOT_BN_RELU):
        d['gout'] = ints(rng, (N, C))
    if mode in (S.RED_DOT_BN, S.RED_DOT_BN_RELU):
        d['mean'] = ints(rng, (C,), -3, 3)
        d['rstd'] = rng.choice(np.array([0.25, 0.5, 1], F), (C,))
        d['coef'] = np.stack([rng.choice(np.array([0.5, -0.5, 1, 2], F), C), rng.choice(np.array([-1, 0, 0.5, 1], F), C)])
        d['coef'][:, 0], d['rstd'][0] = (0.5, -1), 0.5                  # column 0: z = 0 at x - mean = 4
    elif mode not in (S.RED_SUM, S.RED_MOMENTS):
        d['mean'] = ints(rng, (G, C), -3, 3)
        if mode == S.RED_DOT_ELU:
            d['rstd'] = rng.choice(np.array([128, 256, 512], F), (G, C))
        if mode == S.RED_COEF_XC:
            d['coef'] = dyadic(rng, (Sn, C))
    return d


def run_colreduce(mode, d, *, lens=None, post=S.POST_NONE, gid=None, sid=None, eps=EPS, pad=0, offset=0, bf16=False, family=None,
                  width=None, chunks=None, repeat=1):
    """One stin_colreduce_* call against the restatement.  lens: the rows of each range (None: one range, ptr = NULL).  Asserts the
    route the call takes (family / width / chunks where given), both outputs, and that the workspace changed only where the route
    writes partials.  -> the route."""
    x = d['x']
    N, C = x.shape
    B = 1 if lens is None else len(lens)
    ptr = None if lens is None else np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    assert ptr is None or ptr[-1] == N
    inv = (1.0 / np.maximum(np.asarray([N] if lens is None else lens, np.float64), 1.0)).astype(F)
    nout = 2 if mode in O.TWO_OUTPUTS else 1
    ldx, ldg = C + pad, C + 2 * pad
    vec = int(C % 4 == 0 and pad % 4 == 0 and offset % (8 if bf16 else 16) == 0)
    rc, rt = T.route(lib(), N, C, B, nout, vec, 0 if bf16 else 1, cu_count())
    assert rc == 0
    for name, want in (('family', family), ('width', width), ('chunks', chunks)):
        assert want is None or rt[name] == want, (name, rt)
    bx = rows_box(x, ldx, bf16, offset)
    bg = rows_box(d['gout'], ldg, bf16, offset) if 'gout' in d else None
    bptr, bgid, bsid = vecbox(ptr, np.int32), vecbox(gid, np.int32), vecbox(sid, np.int32)
    bm, bs, bc, binv = vecbox(d.get('mean')), vecbox(d.get('rstd')), vecbox(d.get('coef')), vecbox(inv)
    out0, out1 = Box(B * C * 4), Box(B * C * 4)
    ws_bytes = lib().stin_colreduce_workspace_bytes(C, B)
    ws = Box(ws_bytes, 0, WS_GUARD)
    assert rt['partial'] * 8 + 256 <= ws_bytes
    fn = lib().stin_colreduce_bf16 if bf16 else lib().stin_colreduce_f32
    for _ in range(repeat):
        rc = fn(mode, bx.ptr, ldx, p(bg), ldg if bg else 0, N, C, p(bptr), B, p(bgid), p(bsid), p(bm), p(bs), p(bc), post, binv.ptr, float(eps),
                out0.ptr, out1.ptr, ws.ptr, ws_bytes, stream())
        assert rc == 0, rc
    w0, w1 = O.colreduce(mode, x, d.get('gout'), ptr, B, gid, sid, d.get('mean'), d.get('rstd'), d.get('coef'), post, inv, eps)
    assert out0.holds(w0), (mode, post, rt)
    assert out1.holds(w1) if w1 is not None else out1.untouched(), (mode, post, rt)
    first = -ws.ptr % 256                                   # the partials start on the next 256 bytes
    assert ws.untouched_outside(first, first + rt['partial'] * 8), rt
    return rt


RAGGED = (0, 1, 3, 700, 4097)                               # rows of five ranges: an empty one, one row, three rows


def ids_of(rng, lens, G, Sn):
    """Row ids that are NOT the range index: gid by other boundaries (the linspace-slice quirk), sid scattered"""
    N = int(np.sum(lens))
    gid = np.minimum(np.arange(N) * G // max(N, 1), G - 1).astype(np.int32)
    gid[::7] = (gid[::7] + 1) % G
    return gid, rng.integers(0, Sn, N).astype(np.int32)


LEGAL_POSTS = {S.RED_SUM: (0, 1, 2), S.RED_CSQ: (0, 1, 2), S.RED_COEF_XC: (0, 1, 2), S.RED_DOT_ELU: (0, 1, 2, 3), S.RED_MOMENTS: (0,),
               S.RED_DOT_BN: (0, 1, 2), S.RED_DOT_BN_RELU: (0, 1, 2)}
# (name, C, pad, lens, family, width): the one-launch route with dead lanes in the last column group; the two-stage route at one
# channel per lane; the two-stage route at four (more than 512 (range, column group) pairs)
MODE_ROUTES = (('one-launch', 20, 4, RAGGED, ONE, 16), ('two-stage-scalar', 7, 1, RAGGED, TWO, 1),
               ('two-stage-vec', 8, 0, tuple(np.random.default_rng(5).integers(0, 7, 513)), TWO, 4))


@pytest.mark.parametrize('route', MODE_ROUTES, ids=lambda r: r[0])
@pytest.mark.parametrize('mode', [S.RED_SUM, S.RED_CSQ, S.RED_DOT_ELU, S.RED_COEF_XC, S.RED_MOMENTS])
def test_every_mode_and_post_on_each_route(mode, route):
    """Every mode x every legal post, gid / sid given (and different from the range index) and NULL.  POST_RSTD on sums that may
    be negative runs with eps = 2^20, which keeps the square root's argument positive."""
    _, C, pad, lens, family, width = route
    rng = np.random.default_rng(100 * mode + C)
    B, N = len(lens), int(np.sum(lens))
    d = operands(rng, mode, N, C, B, B)
    gid, sid = ids_of(rng, lens, B, B)
    for post in LEGAL_POSTS[mode]:
        eps = EPS if mode in (S.RED_CSQ, S.RED_MOMENTS) or post != S.POST_RSTD else 2.0 ** 20
        run_colreduce(mode, d, lens=lens, post=post, gid=gid, sid=sid, eps=eps, pad=pad, family=family, width=width)
    if mode not in (S.RED_SUM, S.RED_MOMENTS):
        d1 = dict(d, mean=d['mean'][:1], rstd=d['rstd'][:1]) if 'rstd' in d else dict(d, mean=d['mean'][:1])
        run_colreduce(mode, d1, lens=lens, gid=None, sid=None if mode != S.RED_COEF_XC else sid, pad=pad, family=family)
        if mode == S.RED_COEF_XC:
            run_colreduce(mode, d, lens=lens, gid=gid, sid=None, pad=pad, family=family)


@pytest.mark.parametrize('route', [('one-launch', 20, 4, ONE), ('two-stage-scalar', 6, 1, TWO)], ids=lambda r: r[0])
@pytest.mark.parametrize('mode', [S.RED_DOT_BN, S.RED_DOT_BN_RELU])
def test_batchnorm_backward_sums(mode, route):
    """DOT_BN / DOT_BN_RELU (one range, gid NULL) with gamma n + beta on both sides of 0 and at 0"""
    _, C, pad, family = route
    rng = np.random.default_rng(mode + C)
    d = operands(rng, mode, 1500, C, 1, 1)
    z = d['coef'][0][None] * ((d['x'] - d['mean'][None]) * d['rstd'][None]) + d['coef'][1][None]
    assert (z > 0).any() and (z < 0).any() and (z == 0).any()
    for post in LEGAL_POSTS[mode]:
        run_colreduce(mode, d, post=post, eps=2.0 ** 20, pad=pad, family=family)


@pytest.mark.parametrize('C,width', [(4, 16), (16, 16), (20, 16), (128, 32), (132, 32), (256, 64), (260, 64), (512, 64)])
def test_one_launch_route_at_every_column_group_width(C, width):
    """B = 1 with ptr = NULL, three row chunks; at C = 20, 132, 260 the dead lanes of the last column group must add nothing."""
    rng = np.random.default_rng(C)
    N = T.rows_for_chunks(C, 3) + 5
    for mode, post in ((S.RED_MOMENTS, 0), (S.RED_DOT_ELU, S.POST_NORM_COEF), (S.RED_CSQ, S.POST_RSTD)):
        run_colreduce(mode, operands(rng, mode, N, C, 1, 1), post=post, family=ONE, width=width, chunks=3)


def test_one_launch_route_with_every_ticket_word_of_the_row_in_use():
    """B * ncg = 512 exactly: 512 ranges (empty ones among them) of a 16-channel matrix"""
    rng = np.random.default_rng(512)
    lens = rng.integers(0, 6, 512)
    gid, sid = ids_of(rng, lens, 512, 2)
    for mode in (S.RED_MOMENTS, S.RED_DOT_ELU):
        rt = run_colreduce(mode, operands(rng, mode, int(lens.sum()), 16, 512, 2), lens=lens, gid=gid, family=ONE, width=16, chunks=1)
        assert rt['gz'] * rt['ncg'] == 512


def chunk_counts(C):
    """Row-chunk counts around the fold trip of k_colreduce_t (16 partials in flight per thread, PARTS = 256 / GC threads per column)
    and the CU cap, whatever the device's CU count makes of it"""
    parts = 256 // (64 if C >= 256 else 16)
    cap = T.route(lib(), 10 ** 7, C, 1, 2, 1, 1, cu_count())[1]['chunks']
    return sorted({1, 2, 16 * parts - 1, 16 * parts, 16 * parts + 1, cap} & set(range(1, cap + 1))), cap


@pytest.mark.parametrize('C', [256, 16])
def test_one_launch_fold_trip_boundaries(C):
    """R = 1, 2, 16 PARTS - 1, 16 PARTS, 16 PARTS + 1 and the CU cap; the last chunk holds one row, and it contributes"""
    rng = np.random.default_rng(C + 1)
    counts, cap = chunk_counts(C)
    for R in counts:
        N = T.rows_for_chunks(C, R) + (8 * 512 if R == cap else 0)
        for mode in (S.RED_MOMENTS, S.RED_SUM):
            d = operands(rng, mode, N, C, 1, 1)
            d['x'][-1] = 7
            run_colreduce(mode, d, family=ONE, chunks=R)


def test_ticket_words_are_ready_for_the_next_launch_of_their_slot():
    """Every launch takes the next of 128 slot rows, so the 129th uses the words of the first again: 300 launches in a row on one
    stream, then one with other data into fresh buffers - its result must be the restatement's, so the words had been reset."""
    rng = np.random.default_rng(9)
    d = operands(rng, S.RED_MOMENTS, 1100, 16, 1, 1)
    run_colreduce(S.RED_MOMENTS, d, family=ONE, chunks=3, repeat=300)
    d2 = operands(rng, S.RED_DOT_ELU, 1100, 16, 1, 1)
    run_colreduce(S.RED_DOT_ELU, d2, family=ONE, chunks=3, repeat=2)
    run_colreduce(S.RED_MOMENTS, operands(rng, S.RED_MOMENTS, 1100, 16, 1, 1), family=ONE, chunks=3)


def test_four_channels_300_ranges_two_outputs_stays_inside_the_workspace():
    """C = 4, B = 300, MOMENTS and DOT_ELU: the shape whose one-launch partial (300 x 32 doubles) would not fit the workspace of
    8192 doubles; the route query sends it to the two-stage route, and the workspace guard keeps its sentinel."""
    rng = np.random.default_rng(300)
    lens = rng.integers(0, 30, 300)
    gid, _ = ids_of(rng, lens, 300, 1)
    for mode in (S.RED_MOMENTS, S.RED_DOT_ELU):
        run_colreduce(mode, operands(rng, mode, int(lens.sum()), 4, 300, 1), lens=lens, gid=gid, family=TWO, width=4)
    run_colreduce(S.RED_SUM, operands(rng, S.RED_SUM, int(lens.sum()), 4, 300, 1), lens=lens, family=ONE, width=16, chunks=1)


@pytest.mark.parametrize('C,B', [(16, 513), (8, 1025)])
def test_two_stage_route_past_the_ticket_row_and_past_the_slab_count(C, B):
    rng = np.random.default_rng(B)
    lens = rng.integers(0, 5, B)
    lens[-1] = 3
    gid, sid = ids_of(rng, lens, B, B)
    for mode in (S.RED_MOMENTS, S.RED_DOT_ELU, S.RED_COEF_XC):
        run_colreduce(mode, operands(rng, mode, int(lens.sum()), C, B, B), lens=lens, gid=gid, sid=sid, family=TWO, width=4, chunks=1)


@pytest.mark.parametrize('C,pad,offset', [(1, 0, 0), (3, 0, 0), (7, 2, 0), (256, 1, 0), (256, 0, 4)])
def test_two_stage_route_at_one_channel_per_lane(C, pad, offset):
    """C = 1, 3, 7; C = 256 at ldx = 257; C = 256 with the base one float off"""
    rng = np.random.default_rng(C + pad + offset)
    for mode, post in ((S.RED_MOMENTS, 0), (S.RED_DOT_ELU, S.POST_NORM_COEF), (S.RED_CSQ, S.POST_SCALE)):
        run_colreduce(mode, operands(rng, mode, 1000, C, 1, 1), post=post, pad=pad, offset=offset, family=TWO, width=1)


@pytest.mark.parametrize('nch', [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1024])
def test_two_stage_finalisers_at_every_fold_trip_boundary(nch):
    """C = 256 at ldx = 257 (one channel per lane, one row lane), N = 8 nch: nch chunks of eight rows, folded by k_moments_final
    (MOMENTS) and k_colreduce_final (DOT_ELU: both outputs; SUM).  Every chunk, the last included, holds rows that contribute."""
    rng = np.random.default_rng(nch)
    for mode in (S.RED_MOMENTS, S.RED_DOT_ELU, S.RED_SUM):
        d = operands(rng, mode, 8 * nch, 256, 1, 1)
        d['x'][-1] = 7
        run_colreduce(mode, d, pad=1, family=TWO, width=1, chunks=nch)


@pytest.mark.parametrize('C', [16, 3])
def test_no_rows(C):
    """N = 0 for every mode: the sums are 0, the posts still run"""
    rng = np.random.default_rng(C)
    for mode in range(7):
        for post in LEGAL_POSTS[mode]:
            run_colreduce(mode, operands(rng, mode, 0, C, 1, 1), post=post, eps=2.0 ** 20, family=TWO, chunks=1)


def test_colreduce_refusals_leave_every_buffer_alone():
    C, N, B = 8, 40, 2
    rng = np.random.default_rng(1)
    bx, bg = Box.of(ints(rng, (N, C))), Box.of(ints(rng, (N, C)))
    bptr, binv = vecbox([0, 10, 40], np.int32), vecbox([0.1, 1 / 30.0])
    bm, bs, bc = vecbox(np.zeros((B, C), F)), vecbox(np.full((B, C), 128, F)), vecbox(np.ones((2, C), F))
    out0, out1 = Box(B * C * 4), Box(B * C * 4)
    nb = lib().stin_colreduce_workspace_bytes(C, B)
    ws = Box(nb, 0, WS_GUARD)
    E = {n: K['STIN_E_' + n] for n in ('NULL', 'SIZE', 'WORKSPACE', 'UNSUPPORTED')}
    ok = dict(mode=S.RED_DOT_ELU, x=bx.ptr, ldx=C, gout=bg.ptr, ldg=C, N=N, C=C, ptr=bptr.ptr, B=B, gid=None, sid=None, mean=bm.ptr,
              rstd=bs.ptr, coef=bc.ptr, post=0, inv=binv.ptr, eps=EPS, out0=out0.ptr, out1=out1.ptr, ws=ws.ptr, nb=nb)
    cases = [(dict(mode=7), 'UNSUPPORTED'), (dict(mode=-1), 'UNSUPPORTED'), (dict(N=-1), 'SIZE'), (dict(C=0), 'SIZE'), (dict(B=0), 'SIZE'),
             (dict(ldx=C - 1), 'SIZE'), (dict(ptr=None), 'SIZE'), (dict(x=None), 'NULL'), (dict(out0=None), 'NULL'), (dict(ws=None), 'NULL'),
             (dict(post=4), 'UNSUPPORTED'), (dict(mode=S.RED_SUM, post=S.POST_NORM_COEF), 'UNSUPPORTED'),
             (dict(post=S.POST_SCALE, inv=None), 'NULL'), (dict(mode=S.RED_CSQ, mean=None), 'NULL'),
             (dict(mode=S.RED_MOMENTS, out1=None), 'NULL'), (dict(mode=S.RED_MOMENTS, inv=None), 'NULL'), (dict(gout=None), 'NULL'),
             (dict(rstd=None), 'NULL'), (dict(out1=None), 'NULL'), (dict(ldg=C - 1), 'NULL'), (dict(mode=S.RED_COEF_XC, coef=None), 'NULL'),
             (dict(mode=S.RED_DOT_BN), 'NULL'), (dict(mode=S.RED_DOT_BN_RELU, B=1, ptr=None, gid=bptr.ptr), 'NULL'),
             (dict(nb=nb - 1), 'WORKSPACE')]
    for change, err in cases:
        a = dict(ok, **change)
        rc = lib().stin_colreduce_f32(a['mode'], a['x'], a['ldx'], a['gout'], a['ldg'], a['N'], a['C'], a['ptr'], a['B'], a['gid'], a['sid'],
                                      a['mean'], a['rstd'], a['coef'], a['post'], a['inv'], a['eps'], a['out0'], a['out1'], a['ws'], a['nb'],
                                      stream())
        assert rc == E[err], (change, rc)
    assert out0.untouched() and out1.untouched() and ws.untouched()


# ------------------------------------------------------------------------------------------------ bf16 rows
@pytest.mark.parametrize('C,pad,family', [(16, 8, ONE), (12, 4, ONE), (16, 0, TWO)])
def test_colreduce_on_bf16_rows(C, pad, family):
    rng = np.random.default_rng(C + pad)
    lens = RAGGED if family == ONE else rng.integers(0, 5, 513)
    gid, sid = ids_of(rng, lens, len(lens), len(lens))
    for mode, post in ((S.RED_MOMENTS, 0), (S.RED_DOT_ELU, S.POST_NORM_COEF), (S.RED_COEF_XC, S.POST_SCALE)):
        run_colreduce(mode, operands(rng, mode, int(np.sum(lens)), C, len(lens), len(lens)), lens=lens, post=post, gid=gid, sid=sid, pad=pad, bf16=True,
                      family=family)


def test_bf16_rows_refused_where_no_vector_fits():
    """C % 4 != 0, a pitch that is no multiple of 4, rows that start on 4 bytes: STIN_E_UNSUPPORTED, nothing written"""
    rng = np.random.default_rng(6)
    for C, pad, offset in ((6, 0, 0), (8, 2, 0), (8, 0, 4)):
        x, g = ints(rng, (30, C)), ints(rng, (30, C))
        z, r = np.zeros((1, C), F), np.full((1, C), 128, F)
        run_fwd(x, z, r, res=g, pad=pad, bf16=True, offset=offset, want_rc=K['STIN_E_UNSUPPORTED'])
        run_bwd(x, g, z, r, r, z, z, pad=pad, bf16=True, offset=offset, want_rc=K['STIN_E_UNSUPPORTED'])
        bx, bm = rows_box(x, C + pad, True, offset), vecbox(z)
        out0, out1, ws = Box(C * 4), Box(C * 4), Box(lib().stin_colreduce_workspace_bytes(C, 1), 0, WS_GUARD)
        rc = lib().stin_colreduce_bf16(S.RED_CSQ, bx.ptr, C + pad, None, 0, 30, C, None, 1, None, None, bm.ptr, None, None, 0, None, 0.0,
                                       out0.ptr, out1.ptr, ws.ptr, ws.n, stream())
        assert rc == K['STIN_E_UNSUPPORTED']
        assert out0.untouched() and out1.untouched() and ws.untouched()


@pytest.mark.parametrize('C,pad,offset,cls', [(16, 8, 0, 8), (64, 0, 0, 8), (16, 4, 0, 4), (12, 4, 0, 4), (16, 0, 8, 4)])
def test_elementwise_passes_on_bf16_rows(C, pad, offset, cls):
    """Eight channels per lane (C % 8 == 0, 16-byte rows), four (C = 12; a pitch of 4; rows on 8 bytes); the output is the exact
    result rounded to nearest-even once (n + res reaches 2051: 12 significant bits)"""
    assert lib().stin_norm_lane_class(C, 2, 16 if offset == 0 else offset, 1, int(np.gcd(C + pad, np.gcd(C + 2 * pad, 8)))) == cls
    rng = np.random.default_rng(C + pad + offset)
    N, G = 301, 3
    x, g, res = ints(rng, (N, C)), ints(rng, (N, C)), ints(rng, (N, C))
    mean, rstd = ints(rng, (G, C), -3, 3), rng.choice(np.array([128, 256], F), (G, C))
    gid, sid = rng.integers(0, G, N).astype(np.int32), rng.integers(0, G, N).astype(np.int32)
    for act in (0, 1):
        run_fwd(x, mean, rstd, gid, res, act, pad, bf16=True, offset=offset)
        run_fwd(x, mean, rstd, gid, None, act, pad, bf16=True, offset=offset)
        run_bwd(x, g, mean, rstd, dyadic(rng, (G, C)), dyadic(rng, (G, C)), dyadic(rng, (G, C)), gid, sid, act, pad, bf16=True, offset=offset)


# ------------------------------------------------------------------------------------------------ elementwise, fp32
@pytest.mark.parametrize('pad', [4, 1])
@pytest.mark.parametrize('C', [1, 3, 4, 20, 256])
def test_elementwise_passes_on_fp32_rows(C, pad):
    """ld = C + 4 (four channels per lane where C % 4 == 0) and C + 1 (one); res NULL and given; act 0 and 1; N = 0, 1, 301"""
    assert lib().stin_norm_lane_class(C, 4, 16, 1, 4 if pad == 4 else 1) == (4 if C % 4 == 0 and pad == 4 else 1)
    rng = np.random.default_rng(10 * C + pad)
    G = 3
    for N in (0, 1, 301):
        x, g, res = ints(rng, (N, C)), ints(rng, (N, C)), ints(rng, (N, C))
        mean, rstd = ints(rng, (G, C), -3, 3), rng.choice(np.array([128, 256, 512], F), (G, C))
        gid, sid = rng.integers(0, G, N).astype(np.int32), rng.integers(0, G, N).astype(np.int32)
        a, k, m = dyadic(rng, (G, C)), dyadic(rng, (G, C)), dyadic(rng, (G, C))
        for act in (0, 1):
            run_fwd(x, mean, rstd, gid, res, act, pad)
            run_fwd(x, mean[:1], rstd[:1], None, None, act, pad)
            run_bwd(x, g, mean, rstd, a, k, m, gid, sid, act, pad)
            run_bwd(x, g, mean[:1], rstd[:1], a[:1], k, m, None, sid, act, pad)
            run_bwd(x, g, mean, rstd, a, k[:1], m[:1], gid, None, act, pad)


@pytest.mark.parametrize('C,pad', [(20, 4), (3, 1), (256, 4)])
def test_forward_with_the_residual_through_a_row_map(C, pad):
    """Repeated and out-of-order map entries: the rows of the residual that the map names, not the rows of the output"""
    rng = np.random.default_rng(C)
    N, M = 301, 301
    row_map = rng.integers(0, M, N).astype(np.int32)
    row_map[:4] = (M - 1, 0, 0, M - 1)
    x, res = ints(rng, (N, C)), ints(rng, (M, C))
    mean, rstd = ints(rng, (2, C), -3, 3), rng.choice(np.array([128, 256], F), (2, C))
    for act in (0, 1):
        run_fwd(x, mean, rstd, rng.integers(0, 2, N).astype(np.int32), res, act, pad, row_map=row_map)


# ------------------------------------------------------------------------------------------------ folds of given partials
def int_partials(rng, groups, totals0, totals1):
    """[groups][2][C] fp64 integers whose sums over the groups are the given totals; the last group is what is left, never 0"""
    part = rng.integers(-1000, 1001, (groups, 2, len(totals0))).astype(np.float64)
    part[-1, 0] = totals0 - part[:-1, 0].sum(axis=0)
    part[-1, 1] = totals1 - part[:-1, 1].sum(axis=0)
    if groups > 1:
        fix = part[-1] == 0
        part[-1][fix] += 1
        part[-2][fix] -= 1
    return part


GROUPS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1024]


@pytest.mark.parametrize('groups', GROUPS)
def test_moments_final_and_norm_coef_from_partials(groups):
    """stin_moments_final_f32 (fold_lane_moments: 256 partials per trip, pairs of strides) and stin_norm_coef_from_partials_f32
    (fold_lane_sum: 512 per trip, groups of four strides) on integer partials, C = 5 and 64"""
    rng = np.random.default_rng(groups)
    for C in (5, 64):
        mu = rng.integers(-3, 4, C).astype(np.float64)
        part = int_partials(rng, groups, 4096 * mu, 4096 * (mu * mu + rng.integers(-2, 3, C)))      # var in -2 .. 2: the clamp too
        bp, binv = Box.of(part), vecbox([1.0 / 4096])
        bmean, brstd = Box(C * 4), Box(C * 4)
        assert lib().stin_moments_final_f32(bp.ptr, groups, C, binv.ptr, EPS, bmean.ptr, brstd.ptr, stream()) == 0
        mean, rstd = O.moments_final(part, [1.0 / 4096], EPS)
        assert bmean.holds(mean) and brstd.holds(rstd)
        assert (rstd == 128).any() and (rstd != 128).any() or C == 5
        r = rng.choice(np.array([128, 256, 0.5], F), (1, C))
        br, bk, bm = Box.of(r), Box(C * 4), Box(C * 4)
        assert lib().stin_norm_coef_from_partials_f32(bp.ptr, groups, C, br.ptr, binv.ptr, bk.ptr, bm.ptr, stream()) == 0
        k, m = O.norm_coef_from_partials(part, r, [1.0 / 4096])
        assert bk.holds(k) and bm.holds(m)


def fold_rows(C, groups):
    """A power-of-two row count (inv_cnt exact) at which the fold forms serve (N, C, groups) on this device"""
    for N in (512, 4096, 32768, 131072, 262144):
        if lib().stin_norm_fold_rows(N, C, groups) > 0:
            return N
    raise AssertionError('no row count for C = %d, groups = %d' % (C, groups))


@pytest.mark.parametrize('C', [32, 64, 256])
@pytest.mark.parametrize('groups', [1, 16, 17, 257])
def test_fold_forms(groups, C):
    """stin_norm_act_res_fwd_fold_f32, its _map form and stin_norm_act_bwd_fold_f32 on integer partials [groups][2][C].  The moment
    partials add up to mean = an integer and var <= 0 exactly, so rstd = 1 / sqrt(eps) = 128 and the ELU stays on its lattice."""
    rng = np.random.default_rng(groups + C)
    N = fold_rows(C, groups)
    mu = rng.integers(-3, 4, C).astype(np.float64)
    part = int_partials(rng, groups, N * mu, N * (mu * mu - rng.integers(0, 3, C)))
    x, res, g = ints(rng, (N, C)), ints(rng, (N, C)), ints(rng, (N, C))
    bp, binv = Box.of(part), vecbox([1.0 / N])
    bx, bres, bg = rows_box(x, C + 4), rows_box(res, C + 8), rows_box(g, C + 8)
    mean, rstd, y = O.norm_fwd_fold(part, x, res, [1.0 / N], EPS)
    assert np.array_equal(rstd, np.full((1, C), 128, F))
    for with_res in (1, 0):
        bmean, brstd, by = Box(C * 4), Box(C * 4), Box(((N - 1) * (C + 4) + C) * 4)
        assert lib().stin_norm_act_res_fwd_fold_f32(bp.ptr, groups, bx.ptr, C + 4, bres.ptr if with_res else None, C + 8, binv.ptr, EPS, N, C,
                                                    bmean.ptr, brstd.ptr, by.ptr, C + 4, stream()) == 0
        want = y if with_res else O.norm_fwd_fold(part, x, None, [1.0 / N], EPS)[2]
        assert bmean.holds(mean) and brstd.holds(rstd) and by.holds(spread(want, C + 4))
    M = 77
    row_map = rng.integers(0, M, N).astype(np.int32)
    row_map[:4] = (M - 1, 0, 0, M - 1)
    small = ints(rng, (M, C))
    bsmall, bmap = rows_box(small, C + 8), vecbox(row_map, np.int32)
    bmean, brstd, by = Box(C * 4), Box(C * 4), Box(((N - 1) * (C + 4) + C) * 4)
    assert lib().stin_norm_act_res_fwd_fold_map_f32(bp.ptr, groups, bx.ptr, C + 4, bsmall.ptr, C + 8, bmap.ptr, binv.ptr, EPS, N, C, bmean.ptr,
                                                    brstd.ptr, by.ptr, C + 4, stream()) == 0
    assert bmean.holds(mean) and brstd.holds(rstd) and by.holds(spread(O.norm_fwd_fold(part, x, small, [1.0 / N], EPS, row_map)[2], C + 4))
    # backward: partials of (dy xc, dy), any integers; mean integer, rstd = 128 given
    pb = int_partials(rng, groups, rng.integers(-9, 10, C).astype(np.float64), rng.integers(-9, 10, C).astype(np.float64))
    mean_b, rstd_b = ints(rng, (1, C), -3, 3), rng.choice(np.array([128, 256], F), (1, C))
    bpb, bmu, brs, bd = Box.of(pb), Box.of(mean_b), Box.of(rstd_b), Box(((N - 1) * (C + 4) + C) * 4)
    assert lib().stin_norm_act_bwd_fold_f32(bpb.ptr, groups, bx.ptr, C + 4, bg.ptr, C + 8, bmu.ptr, brs.ptr, binv.ptr, N, C, bd.ptr, C + 4,
                                            stream()) == 0
    assert bd.holds(spread(O.norm_bwd_fold(pb, x, g, mean_b, rstd_b, [1.0 / N]), C + 4))
    assert bmu.holds(mean_b) and brs.holds(rstd_b)


def test_fold_forms_decline_where_the_fold_does_not_pay():
    """(N, C, groups) = (64, 32, 257): stin_norm_fold_rows is 0, the entry points answer STIN_E_UNSUPPORTED and write nothing"""
    N, C, groups = 64, 32, 257
    assert lib().stin_norm_fold_rows(N, C, groups) == 0
    rng = np.random.default_rng(3)
    bp, binv, bx, bo = Box.of(np.ones((groups, 2, C))), vecbox([1.0 / N]), Box.of(ints(rng, (N, C))), Box.of(ints(rng, (N, C)))
    bmean, brstd, by, bmap = Box.of(np.zeros(C, F)), Box.of(np.ones(C, F)), Box(N * C * 4), vecbox(np.zeros(N), np.int32)
    E = K['STIN_E_UNSUPPORTED']
    assert lib().stin_norm_act_res_fwd_fold_f32(bp.ptr, groups, bx.ptr, C, bo.ptr, C, binv.ptr, EPS, N, C, bmean.ptr, brstd.ptr, by.ptr, C, stream()) == E
    assert lib().stin_norm_act_res_fwd_fold_map_f32(bp.ptr, groups, bx.ptr, C, bo.ptr, C, bmap.ptr, binv.ptr, EPS, N, C, bmean.ptr, brstd.ptr, by.ptr,
                                                    C, stream()) == E
    assert lib().stin_norm_act_bwd_fold_f32(bp.ptr, groups, bx.ptr, C, bo.ptr, C, bmean.ptr, brstd.ptr, binv.ptr, N, C, by.ptr, C, stream()) == E
    assert by.untouched() and bmean.holds(np.zeros(C, F)) and brstd.holds(np.ones(C, F))


# ------------------------------------------------------------------------------------------------ BatchNorm passes
@pytest.mark.parametrize('C,pad', [(1, 0), (6, 1), (64, 4), (64, 1)])
def test_batchnorm_forward_and_backward_passes(C, pad):
    rng = np.random.default_rng(C + pad)
    N = 301
    x, g = ints(rng, (N, C)), ints(rng, (N, C))
    mean, rstd = ints(rng, (C,), -3, 3), rng.choice(np.array([0.25, 0.5, 1], F), C)
    gamma, beta = rng.choice(np.array([0.5, -0.5, 1, 2], F), C), rng.choice(np.array([-1, 0, 0.5, 1], F), C)
    gamma[0], beta[0], rstd[0] = 0.5, -1, 0.5
    P, Q, inv_n = ints(rng, (C,), -50, 50), ints(rng, (C,), -50, 50), 1.0 / N
    ld = C + pad
    bx, bg = rows_box(x, ld), rows_box(g, ld)
    v = [vecbox(t) for t in (mean, rstd, gamma, beta, P, Q)]
    for act in (0, 1):
        by, bd = Box(((N - 1) * ld + C) * 4), Box(((N - 1) * ld + C) * 4)
        assert lib().stin_bn_act_fwd_f32(bx.ptr, ld, *[t.ptr for t in v[:4]], N, C, act, by.ptr, ld, stream()) == 0
        assert by.holds(spread(O.bn_act_fwd(x, mean, rstd, gamma, beta, act), ld))
        assert lib().stin_bn_act_bwd_f32(bx.ptr, ld, bg.ptr, ld, *[t.ptr for t in v], inv_n, N, C, act, bd.ptr, ld, stream()) == 0
        assert bd.holds(spread(O.bn_act_bwd(x, g, mean, rstd, gamma, beta, P, Q, inv_n, act), ld))
    by = Box(64)
    assert lib().stin_bn_act_fwd_f32(bx.ptr, ld, *[t.ptr for t in v[:4]], 0, C, 1, by.ptr, ld, stream()) == 0 and by.untouched()


@pytest.mark.parametrize('C', [1, 5, 64, 300])
def test_batchnorm_running_statistics(C):
    """Among the rstd values 128 and 64: 1 / rstd^2 - eps < 0 at eps = 1e-3, the variance is raised to 0"""
    rng = np.random.default_rng(C)
    mean, rstd = rng.standard_normal(C).astype(F), rng.choice(np.array([128, 64, 0.5, 1.25, 3], F), C)
    rstd[0] = 128
    rm, rv = rng.standard_normal(C).astype(F), rng.random(C).astype(F)
    eps, unbias, momentum = 1e-3, 301.0 / 300.0, 0.1
    bmean, brstd, brm, brv = Box.of(mean), Box.of(rstd), Box.of(rm), Box.of(rv)
    assert lib().stin_bn_running_stats_f32(bmean.ptr, brstd.ptr, C, eps, unbias, momentum, brm.ptr, brv.ptr, stream()) == 0
    wm, wv = O.bn_running_stats(mean, rstd, eps, unbias, momentum, rm, rv)
    assert F(1) / (F(128) * F(128)) - F(eps) < 0
    assert brm.holds(wm) and brv.holds(wv) and bmean.holds(mean) and brstd.holds(rstd)
