"""The pack, glue and train-step kernels held to tests/_param_oracle.py, the numpy restatement of include/stin_hip.h: the weight
operand layouts the GEMMs decode (plain, bf16 rows, k-group, MFMA fragment order), the EdgeConv pack (one job and a table of jobs)
and unpack, stin_gemm_split_weights_f32, the SingleConvMeshNet layer passes, the padding and the SAGE column update, the norm
backward coefficients, Adam, the masked L1 loss and the two graph metrics.  Everything is EQUAL to the restatement, compared as
integer views; the one exception is the weight 0.99^mask of the loss, whose bits are the device library's powf (see
test_masked_l1_weighted_within_the_powf_bound).  Nothing here compares one route of the library with another and nothing depends
on how a kernel divides its work, so these tests are meant to stay green across a rework of the pack or of the operand staging -
and to go red when a layout drifts while producer and consumer still agree with each other.

Every output lives inside a larger buffer of 0x5A bytes: guard bytes before and after it and, where a leading dimension exceeds
the width, between the rows.  The whole buffer is compared, so a write outside the contract fails the same assertion."""
import numpy as np
import pytest
import torch

import _param_oracle as O
from surface_texture_inpainting_net_amd import _lib
from surface_texture_inpainting_net_amd import functional as SF

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 1024                                              # bytes on either side (a multiple of 16: the output keeps its alignment)
F16, BF16, WB16, FRAG = O.GEMM_F16X3, O.GEMM_BF16X3, O.GEMM_W_BF16, O.GEMM_W_FRAG
C = _lib.CONSTANTS


@pytest.fixture(autouse=True)
def _end_the_run_after_a_device_fault():
    """A kernel fault poisons the process: end the run instead of launching the remaining tests on a faulted device."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit('device fault, run ended: %s' % e, returncode=3)


def sentinel(shape, dtype):
    """A numpy array whose every byte is 0x5A (fp32: 1.5e16, bf16 / fp16: finite too)."""
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


class Box:
    """nbytes of device memory in the middle of a 0x5A-filled buffer; `offset` bytes move it off its 16-byte alignment."""

    def __init__(self, nbytes, offset=0):
        self.n, self.lo = int(nbytes), GUARD + offset
        self.wide = torch.full((2 * GUARD + 16 + (self.n + 15) // 16 * 16,), 0x5A, dtype=torch.uint8, device=DEV)
        assert self.wide.data_ptr() % 16 == 0
        self.ptr = self.wide.data_ptr() + self.lo

    @classmethod
    def of(cls, array, offset=0):
        """A box that holds `array` (an input, or the state a kernel updates in place)."""
        array = np.ascontiguousarray(array)
        box = cls(array.nbytes, offset)
        box.wide[box.lo:box.lo + box.n] = torch.from_numpy(array.reshape(-1).view(np.uint8).copy()).to(DEV)
        return box

    def holds(self, expected):
        """The first expected.nbytes bytes equal `expected`, every other byte of the buffer - the rest of the output where the
        contract writes less than the buffer (bf16 rows), the guards - still holds the sentinel.  Compared as int16 views."""
        expected = np.ascontiguousarray(expected).reshape(-1).view(np.uint8)
        assert expected.size <= self.n
        want = torch.full_like(self.wide, 0x5A, device='cpu')
        want[self.lo:self.lo + expected.size] = torch.from_numpy(expected.copy())
        return torch.equal(self.wide.view(torch.int16), want.to(DEV).view(torch.int16))

    def untouched(self):
        return self.holds(np.zeros(0, np.uint8))

    def read(self, dtype):
        return self.wide[self.lo:self.lo + self.n].cpu().numpy().view(dtype).copy()


def dev(a):
    """The array on the device.  The caller keeps the tensor until the result is read: a temporary's memory is handed to the next one."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return 0 if t is None else (t.ptr if isinstance(t, Box) else SF._ptr(t))


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def call(name, *args):
    SF._call(name, *args, stream())


def status(name, *args):
    """The status a call answers (the refusals: nothing may be raised, nothing launched)."""
    return int(getattr(_lib.load(), name)(*args, stream()))


def domain(rng, shape):
    """Multiples of 2^-8 between 2^-7 and 256 in magnitude, both signs, up to 17 significant bits (both pieces of either split are in
    use), every seventh value exactly a bf16 / fp16 number (lo piece = 0).  Differences of two such values are exact and either 0
    or inside F16X3's documented domain 2^-9 <= |w| < 1023, so the packed Wa - Wb stays inside it too."""
    k = np.rint(np.exp2(rng.uniform(1, 16, shape))) * rng.choice([-1.0, 1.0], shape)
    w = (k * 2.0 ** -8).astype(np.float32).reshape(-1)
    w[::7] = (w[::7].view(np.uint32) & 0xFFFF0000).view(np.float32)
    w[3::7] = (w[3::7].view(np.uint32) & 0xFFFFE000).view(np.float32)
    w[w == 0] = 0.5
    return w.reshape(shape)


def graph(rng, N, mean_deg=3):
    """Destination CSR with empty rows (about a third), self loops and repeated edges.  The last row has three entries, the first of
    them from row 0: whatever owns the last row - the 257th block partial of a 65537-row sum - contributes."""
    deg = rng.integers(0, 2 * mean_deg + 1, N) * (rng.random(N) > 0.33)
    if N > 1:
        deg[-1] = 3
    rowptr = np.zeros(N + 1, np.int32)
    np.cumsum(deg, out=rowptr[1:])
    col = rng.integers(0, max(N, 1), int(rowptr[-1])).astype(np.int32)
    rows = np.repeat(np.arange(N), deg)
    loops = rng.random(col.size) < 0.1
    col[loops] = rows[loops]                                               # self loops
    rep = np.nonzero((rng.random(col.size) < 0.2) & (np.arange(col.size) > 0))[0]
    rep = rep[rows[rep] == rows[rep - 1]]
    col[rep] = col[rep - 1]                                                # repeated edges
    if N > 1:
        col[rowptr[N - 1]] = 0
    return rowptr, col


# ------------------------------------------------------------------ stin_edgeconv_pack_f32 / _many
class PackCase:
    """Host parameters of one block, the five boxed device operands and what the restatement says they must hold."""

    def __init__(self, Cin, Cp, H, Cout, shortcut, ti, fwd, bwd, b1=True, bs=True, seed=0):
        self.args = (Cin, Cp, H, Cout, int(shortcut), ti)
        self.fwd, self.bwd = fwd, bwd
        rng = np.random.default_rng(seed + 7 * Cin + H)
        gen = domain if ((fwd | bwd) & (F16 | BF16)) else (lambda r, s: r.standard_normal(s).astype(np.float32))
        self.host = dict(W1=gen(rng, (H, Cin if ti else 2 * Cin)), b1=gen(rng, (H,)) if b1 else None,
                         Ws=gen(rng, (Cout, Cin)) if shortcut else None, bs=gen(rng, (Cout,)) if shortcut and bs else None,
                         W2=gen(rng, (Cout, H)))
        self.dev = {k: (None if v is None else dev(v)) for k, v in self.host.items()}
        Yw = O.yw_of(H, Cout, shortcut, ti)
        self.elems = Yw * Cp + H * Cout
        self.boxes = {'wcat': Box(4 * Yw * Cp), 'bcat': Box(4 * Yw), 'wcatT': Box(4 * Yw * Cp), 'w2T': Box(4 * H * Cout),
                      'w2s': Box(4 * H * Cout) if fwd else None}               # (no forward split: the block passes no w2s)
        self._want = None

    @property
    def want(self):
        if self._want is None:
            h = self.host
            self._want = O.edgeconv_pack(h['W1'], h['b1'], h['Ws'], h['bs'], h['W2'], *self.args, self.fwd, self.bwd)
        return self._want

    def call_args(self):
        d, b = self.dev, self.boxes
        return (ptr(d['W1']), ptr(d['b1']), ptr(d['Ws']), ptr(d['bs']), ptr(d['W2']), *self.args, ptr(b['wcat']), ptr(b['bcat']),
                ptr(b['wcatT']), ptr(b['w2T']), ptr(b['w2s']), self.fwd, self.bwd)

    def job(self):
        d, b = self.dev, self.boxes
        Cin, Cp, H, Cout, sc, ti = self.args
        return SF._PACK_JOB.pack(W1=ptr(d['W1']), b1=ptr(d['b1']), Ws=ptr(d['Ws']), bs=ptr(d['bs']), W2=ptr(d['W2']), wcat=ptr(b['wcat']),
                                 bcat=ptr(b['bcat']), wcatT=ptr(b['wcatT']), w2T=ptr(b['w2T']), w2s=ptr(b['w2s']), Cin=Cin, Cp=Cp, H=H,
                                 Cout=Cout, has_shortcut=sc, trans_inv=ti, fwd_split=self.fwd, bwd_split=self.bwd)

    def wrong(self):
        """Names of the operands that do not hold the restatement's bytes (or wrote outside them)."""
        return [k for k, b in self.boxes.items() if b is not None and not b.holds(self.want[k])]

    def untouched(self):
        return all(b.untouched() for b in self.boxes.values() if b is not None)


SPLIT, SPLIT_FRAG = (F16, BF16), (F16 | FRAG, BF16 | FRAG)
PACK_CASES = {                                             # (Cin, Cp, H, Cout, shortcut, trans_inv, (fwd, bwd)[, b1, bs])
    'tiny plain': (3, 4, 2, 4, True, 0, (0, 0)),
    'padded 10->12 plain': (10, 12, 8, 4, True, 0, (0, 0)),
    'padded 10->12 split': (10, 12, 8, 4, True, 0, SPLIT),
    'padded 10->12 split, b1 NULL': (10, 12, 8, 4, True, 0, SPLIT, False, True),
    'padded 10->16 bf16 rows, eight-wide': (10, 16, 8, 8, True, 1, (WB16, WB16)),
    'padded 10->16 bf16 rows, bs NULL': (10, 16, 8, 8, True, 1, (WB16, WB16), True, False),
    'padded 10->16 compact split, eight-wide': (10, 16, 16, 8, False, 2, SPLIT),
    'compact, b1 NULL': (10, 16, 16, 8, False, 2, SPLIT, False, True),
    'wcat 320x128 + wcatT 128x320 fragment': (128, 128, 128, 64, True, 0, SPLIT_FRAG),
    'w2s 256x512 + w2T 512x256 fragment': (64, 64, 512, 256, False, 1, SPLIT_FRAG),
    'compact, wcat 320x128 fragment': (128, 128, 320, 64, False, 2, SPLIT_FRAG),
}


def _pack_case(spec, seed=0):
    Cin, Cp, H, Cout, sc, ti, (fwd, bwd) = spec[:7]
    b1, bs = spec[7:] if len(spec) > 7 else (True, True)
    return PackCase(Cin, Cp, H, Cout, sc, ti, fwd, bwd, b1, bs, seed)


def test_pack_cases_reach_the_layouts_they_name():
    frag = lambda name: {k for k, (nc, kk) in _operand_shapes(PACK_CASES[name]).items() if O.frag_shape(nc, kk)}
    assert frag('wcat 320x128 + wcatT 128x320 fragment') == {'wcat', 'wcatT'}
    assert frag('w2s 256x512 + w2T 512x256 fragment') == {'w2s', 'w2T'}
    assert frag('compact, wcat 320x128 fragment') == {'wcat', 'wcatT'}      # (its transpose 128 x 320 is a fragment shape as well)
    assert not frag('padded 10->12 split')


def _operand_shapes(spec):
    Cin, Cp, H, Cout, sc, ti = spec[:6]
    Yw = O.yw_of(H, Cout, sc, ti)
    return {'wcat': (Yw, Cp), 'wcatT': (Cp, Yw), 'w2T': (H, Cout), 'w2s': (Cout, H)}


@pytest.mark.parametrize('pack8', ['0', '1'])
@pytest.mark.parametrize('name', list(PACK_CASES))
def test_edgeconv_pack_writes_the_restated_bytes(name, pack8, monkeypatch):
    """All five operands, byte for byte, on both pack routes (STIN_PACK8): the zero padding columns Cin .. Cp - 1, NULL biases as
    zeros, no b1 in bcat in compact mode, each operand in fragment order exactly where ITS shape takes it, bf16 rows in the first
    half of their buffer and nothing in the second."""
    monkeypatch.setenv('STIN_PACK8', pack8)
    case = _pack_case(PACK_CASES[name])
    call('stin_edgeconv_pack_f32', *case.call_args())
    assert case.wrong() == []


def test_edgeconv_pack_refusals_write_nothing():
    def refused(spec, code, drop_w2s=False, ti=None):
        case = _pack_case(spec)
        args = list(case.call_args())
        if drop_w2s:
            args[15] = 0
        if ti is not None:
            args[10] = ti
        return status('stin_edgeconv_pack_f32', *args) == code and case.untouched()

    assert refused((4, 4, 4, 4, True, 0, SPLIT), C['STIN_E_ALIGN'], drop_w2s=True)          # a forward split without w2s
    assert refused((4, 4, 2, 4, True, 0, (F16, 0)), C['STIN_E_ALIGN'])                      # ... with H % 4 != 0
    assert refused((4, 4, 4, 4, True, 0, (0, 0)), C['STIN_E_UNSUPPORTED'], ti=3)
    assert refused((4, 4, 4, 6, True, 0, (0, BF16)), C['STIN_E_ALIGN'])                     # Yw = 14
    assert refused((4, 4, 6, 4, False, 2, (0, BF16)), C['STIN_E_ALIGN'])                    # compact: Yw = H = 6
    assert refused((4, 4, 3, 4, False, 1, (0, BF16)), C['STIN_E_ALIGN'])                    # Yw = 6


@pytest.mark.parametrize('pack8', ['0', '1'])
def test_edgeconv_pack_many_writes_every_jobs_restated_bytes(pack8, monkeypatch):
    """Four jobs of different sizes and modes in one table - eight-wide bf16 rows, elementwise split, compact split, a tiny plain
    one without w2s - built with the package's own record packer; the grid is sized by the largest job, so the smaller ones must ignore the surplus threads."""
    monkeypatch.setenv('STIN_PACK8', pack8)
    cases = [_pack_case(PACK_CASES[n], seed=s) for s, n in enumerate(('padded 10->16 bf16 rows, eight-wide', 'padded 10->12 split',
                                                                      'padded 10->16 compact split, eight-wide', 'tiny plain'))]
    table = torch.frombuffer(bytearray(b''.join(c.job() for c in cases)), dtype=torch.uint8).to(DEV)
    call('stin_edgeconv_pack_many_f32', ptr(table), 0, max(c.elems for c in cases))
    torch.cuda.synchronize()
    assert all(c.untouched() for c in cases)                                 # n_jobs = 0 writes nothing
    call('stin_edgeconv_pack_many_f32', ptr(table), len(cases), max(c.elems for c in cases))
    assert [c.wrong() for c in cases] == [[] for _ in cases]


# ------------------------------------------------------------------ stin_edgeconv_unpack_grads_f32
UNPACK_VARIANTS = [(True, True, False), (False, False, False), (True, False, False), (False, True, False), (True, True, True)]


@pytest.mark.parametrize('ti', [0, 1, 2])
@pytest.mark.parametrize('Cin,Cp,H,Cout', [(5, 8, 6, 7), (10, 12, 8, 4), (10, 12, 16, 8), (6, 6, 4, 4)])
def test_edgeconv_unpack_equals_the_restatement(Cin, Cp, H, Cout, ti):
    """dwb is [Yw, Cp + 1]: Cin columns used, junk in the padding columns, the bias gradient in column Cp.  With / without
    shortcut and dw2b, NULL bias outputs; in compact mode db1 is handed over and must keep its sentinel.  (10, 12, 16, 8) spreads
    n1 + ns + n2 (528 threads for trans_inv = 0, 368 otherwise) over more than one block, the other shapes end inside the first."""
    rng = np.random.default_rng(100 * ti + Cin + H)
    for shortcut, second, null_bias in UNPACK_VARIANTS:
        Yw = O.yw_of(H, Cout, shortcut, ti)
        dwb = rng.standard_normal((Yw, Cp + 1)).astype(np.float32)
        dw2b = rng.standard_normal((Cout, H + 1)).astype(np.float32) if second else None
        want = O.edgeconv_unpack(dwb, dw2b, Cin, Cp, H, Cout, shortcut, ti)
        ld1 = Cin if ti else 2 * Cin
        sizes = {'dW1': H * ld1, 'db1': H, 'dWs': Cout * Cin, 'dbs': Cout, 'dW2': Cout * H, 'db2': Cout}
        boxes = {k: Box(4 * n) for k, n in sizes.items()}
        null = {'db1', 'dbs', 'db2'} if null_bias else set()
        if not shortcut:
            null |= {'dWs', 'dbs'}
        if not second:
            null |= {'dW2', 'db2'}
        a, b = dev(dwb), (dev(dw2b) if second else None)
        call('stin_edgeconv_unpack_grads_f32', ptr(a), ptr(b), Cin, Cp, H, Cout, int(shortcut), ti,
             *[0 if k in null else boxes[k].ptr for k in ('dW1', 'db1', 'dWs', 'dbs', 'dW2', 'db2')])
        for k, box in boxes.items():
            expect = np.zeros(0, np.float32) if (k in null or want[k] is None) else want[k]
            assert box.holds(expect), (k, shortcut, second, null_bias)


# ------------------------------------------------------------------ stin_gemm_split_weights_f32
def _split_case(rng, Nc, K, mode, ldw, ldo, gen=domain):
    W = gen(rng, (Nc, K))
    src = rng.standard_normal((Nc, ldw)).astype(np.float32)                 # junk between the rows of the source
    src[:, :K] = W
    frag = bool(mode & FRAG) and O.frag_shape(Nc, K)
    box = Box(4 * (Nc * K if frag else (Nc - 1) * ldo + K))
    d = dev(src)
    call('stin_gemm_split_weights_f32', ptr(d), ldw, Nc, K, mode, box.ptr, ldo)
    torch.cuda.synchronize()
    return W, box


@pytest.mark.parametrize('prec', [F16, BF16])
@pytest.mark.parametrize('Nc,K,frag,pitched', [(1, 4, 0, True), (5, 8, 0, True), (5, 8, FRAG, True), (96, 128, FRAG, False), (128, 256, 0, False),
                                               (128, 256, FRAG, False), (320, 128, 0, True), (320, 128, FRAG, True), (256, 512, 0, False),
                                               (256, 512, FRAG, False)])
def test_split_weights_equals_the_restatement(Nc, K, frag, pitched, prec):
    """The tool most GEMM tests build their operands with: k-group form at ldo > K (sentinel between the rows), fragment order where
    the shape takes it (ldo ignored), the k-group form when the flag meets a shape that does not (96 x 128, 5 x 8)."""
    rng = np.random.default_rng(Nc + K + prec)
    ldw, ldo = (K + 3, K + 4) if pitched else (K, K)
    W, box = _split_case(rng, Nc, K, prec | frag, ldw, ldo)
    assert box.holds(O.encode(W, prec | frag, ld=ldo, fill=0x5A5A))
    if frag:
        assert O.frag_shape(Nc, K) == (not np.array_equal(O.encode(W, prec | frag, ld=ldo), O.encode(W, prec, ld=ldo)))


def test_w_is_frag_equals_the_restated_rule():
    lib = _lib.load()
    for Nc in (32, 96, 127, 128, 129, 255, 256, 257, 288, 319, 320, 321, 352, 512, 1024):
        for K in (16, 64, 127, 128, 129, 192, 255, 256, 257, 320, 448, 511, 512, 576, 1024):
            assert bool(lib.stin_gemm_w_is_frag(Nc, K)) == O.frag_shape(Nc, K), (Nc, K)


def test_split_weights_below_the_f16_domain_keeps_the_absolute_bound():
    """|w| < 2^-9 lies outside F16X3's documented domain: the header promises the absolute accuracy 2^-31 there and no bits."""
    rng = np.random.default_rng(3)
    tiny = lambda r, s: (np.exp2(r.uniform(-30, -9, s)) * r.choice([-1.0, 1.0], s)).astype(np.float32)
    W, box = _split_case(rng, 5, 8, F16, 8, 12, gen=tiny)
    got = box.read(np.uint16)
    assert np.all(np.abs(O.decode(got, 5, 8, F16, ld=12) - W.astype(np.float64)) <= 2.0 ** -31)
    owned = np.zeros(got.size, bool)
    hi, lo, _ = O.split_layout(5, 8, F16, 12)
    owned[hi.reshape(-1)] = owned[lo.reshape(-1)] = True
    assert np.all(got[~owned] == 0x5A5A) and box.holds(got)                  # between the rows and around the buffer


# ------------------------------------------------------------------ stin_adam_f32
ADAM_N = (1, 3, 4, 5, 7, 1023, 1024, 1027, 1026)


@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('amsgrad', [1, 0])
@pytest.mark.parametrize('offset', [0, 4], ids=['aligned', 'offset by one float'])
def test_adam_equals_the_restatement(offset, amsgrad, wd):
    """p, m, v, vmax after each of four calls: steps 1, 2, 3 (a x 100 gradient spike: amsgrad's max takes over), then step = 1000.
    16-byte aligned bases take the float4 kernel with its 0 .. 3 ragged elements (n < 4: the scalar kernel), bases offset by one
    float the scalar kernel; amsgrad = 0 passes vmax = NULL."""
    lr, b1, b2, eps = 7e-5, 0.9, 0.999, 1e-8
    for n in ADAM_N:
        rng = np.random.default_rng(n)
        state = [rng.standard_normal(n).astype(np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32),
                 np.zeros(n, np.float32) if amsgrad else None]
        boxes = [None if s is None else Box.of(s, offset) for s in state]
        for step, scale in ((1, 0.1), (2, 0.1), (3, 10.0), (1000, 0.1)):
            g = (rng.standard_normal(n) * scale).astype(np.float32)
            gbox = Box.of(g, offset)
            call('stin_adam_f32', boxes[0].ptr, gbox.ptr, boxes[1].ptr, boxes[2].ptr, ptr(boxes[3]), n, lr, b1, b2, eps, wd, step, amsgrad)
            state = list(O.adam(state[0], g, state[1], state[2], state[3], lr, b1, b2, eps, wd, step, amsgrad))
            for name, box, want in zip('p m v vmax'.split(), boxes, state):
                assert box is None or box.holds(want), (name, n, step)
            assert gbox.holds(g)


# ------------------------------------------------------------------ stin_masked_l1_loss_f32
LOSS_SHAPES = [(1, 1), (85, 3), (64, 4), (86, 3), (21846, 3)]              # 1, 1, 1, 2 and 257 block partials


def _loss_inputs(N, Cc):
    rng = np.random.default_rng(N + Cc)
    out = rng.uniform(-1, 1, (N, Cc)).astype(np.float32)
    color = rng.uniform(-1, 1, (N, Cc)).astype(np.float32)
    mask = rng.choice(np.array([0, 0, 0, 1, 2, 16, 17, 64, 300]), N).astype(np.int64)
    if N > 1:
        mask[:9] = [0, 1, 2, 16, 17, 64, 300, 0, 5][:min(N, 9)]
        out[1::4] = color[1::4]                                              # rows where out == color exactly (several with mask > 0)
        mask[-1], out[-1] = 2, color[-1] + np.float32(0.75)                  # the last block partial (the 257th of 21846 x 3) counts
    else:
        mask[0] = 17
    return out, color, mask


def _masked_l1(out, color, mask, use_weight):
    N, Cc = out.shape
    lib = _lib.load()
    ws = torch.empty(int(lib.stin_masked_l1_workspace_bytes(N, Cc)), dtype=torch.uint8, device=DEV)
    loss, grad = Box(4), Box(4 * N * Cc)
    o, c, m = dev(out), dev(color), dev(mask)
    call('stin_masked_l1_loss_f32', ptr(o), ptr(c), ptr(m), N, Cc, use_weight, loss.ptr, grad.ptr, ptr(ws), ws.numel())
    torch.cuda.synchronize()
    return loss, grad


@pytest.mark.parametrize('N,Cc', LOSS_SHAPES)
def test_masked_l1_unweighted_equals_the_restatement(N, Cc):
    """Loss and gradient, bit for bit: fp64 terms, the 256-wide tree per block, the finaliser's stride-256 accumulation over the
    block partials (257 of them at 21846 x 3) and the same tree, one cast."""
    out, color, mask = _loss_inputs(N, Cc)
    want_grad, want_loss = O.masked_l1(out, color, mask, 0)
    loss, grad = _masked_l1(out, color, mask, 0)
    assert loss.holds(np.array([want_loss], np.float32)), (loss.read(np.float32), want_loss)
    assert grad.holds(want_grad)


POWF_ULPS = 2                                              # measured + 1, see the test below


def _step(w, k):
    """w moved by k units in the last place."""
    return (w.view(np.int32) + np.int32(k)).view(np.float32)


def test_masked_l1_weighted_within_the_powf_bound(capsys):
    """use_weight = 1: the weight is powf(0.99f, (float)mask) of the device library, the one number here that cannot be derived
    offline.  Measured on the MI355X: over mask = 1 .. 512 the device's weight lies at most 1 ulp (first at mask = 13) from
    f32(f32(0.99)^mask) evaluated in fp64 and rounded once (recovered exactly from the gradient of N = 512, C = 1, out - color = 1:
    grad = fl(w * 2^-9) = w * 2^-9).  The bound is that distance plus one ulp, which the rounding of w * inv can hide: POWF_ULPS = 2.
    Every non-zero gradient entry must then equal +-fl(w' * inv) for a w' within POWF_ULPS of the fp64 power - never compared with a
    second run of the kernel - and the loss lies within the matching bound of the restated sum: a term fl(|d| w') differs from
    fl(|d| w) by at most (2 POWF_ULPS + 2) u relatively (w' / w - 1 <= POWF_ULPS 2 u, one rounding each), all terms are >= 0, and
    the two final casts add 2 u: (2 POWF_ULPS + 4) u with u = 2^-24."""
    power = lambda m: np.power(np.float64(np.float32(0.99)), np.asarray(m, dtype=np.float64)).astype(np.float32)
    m = np.arange(1, 513, dtype=np.int64)
    _, grad = _masked_l1(np.ones((512, 1), np.float32), np.zeros((512, 1), np.float32), m, 1)
    w_dev = grad.read(np.float32) * np.float32(512.0)
    dist = np.abs(w_dev.view(np.int32).astype(np.int64) - power(m).view(np.int32).astype(np.int64))
    with capsys.disabled():
        print('\n[powf] largest distance of the device weight from the fp64 power over mask = 1 .. 512: %d ulp (mask = %d)'
              % (dist.max(), m[dist.argmax()]))
    assert dist.max() + 1 <= POWF_ULPS
    for N, Cc in LOSS_SHAPES:
        out, color, mask = _loss_inputs(N, Cc)
        w = power(mask)
        want_grad, want_loss = O.masked_l1(out, color, mask, 1, w)
        loss, grad = _masked_l1(out, color, mask, 1)
        got = grad.read(np.float32).reshape(N, Cc)
        assert grad.holds(got)                                               # (the guards)
        zero = want_grad == 0
        assert np.all(got.view(np.int32)[zero] == 0)                         # mask <= 0 or out == color: +0
        inv = np.float32(1.0) / np.float32(N * Cc)
        ok = zero.copy()
        for k in range(-POWF_ULPS, POWF_ULPS + 1):
            ok |= got == (np.sign(want_grad) * _step(w, k)[:, None]) * inv
        assert np.all(ok)
        got_loss = float(loss.read(np.float32)[0])
        assert loss.holds(np.array([got_loss], np.float32))
        assert abs(got_loss - float(want_loss)) <= (2 * POWF_ULPS + 4) * 2.0 ** -24 * float(want_loss)


# ------------------------------------------------------------------ stin_total_variation_f32 / stin_graph_laplace_f32
@pytest.mark.parametrize('N', [1, 255, 256, 257, 65537])
def test_total_variation_equals_the_restatement(N):
    """C = 1, 3, 5 at ldx = C + 2 (junk between the rows); 1, 1, 1, 2 and 257 block partials; empty rows, self loops, repeated edges."""
    lib = _lib.load()
    rng = np.random.default_rng(N)
    rowptr, col = graph(rng, N)
    if N == 1:
        rowptr, col = np.array([0, 2], np.int32), np.array([0, 0], np.int32)
    for Cc in (1, 3, 5):
        xw = rng.standard_normal((N, Cc + 2)).astype(np.float32)
        ws = torch.empty(int(lib.stin_total_variation_workspace_bytes(N)), dtype=torch.uint8, device=DEV)
        out = Box(4)
        x, rp, cl = dev(xw), dev(rowptr), dev(col)
        call('stin_total_variation_f32', ptr(x), Cc + 2, ptr(rp), ptr(cl), N, Cc, out.ptr, ptr(ws), ws.numel())
        want = O.total_variation(xw[:, :Cc], rowptr, col)
        assert out.holds(np.array([want], np.float32)), (Cc, out.read(np.float32), want)


@pytest.mark.parametrize('N', [0, 1, 300])
def test_graph_laplace_equals_the_restatement(N):
    """C = 1, 3, 5 at ldx = C + 2 and ldo = C + 1 through the C ABI: the column between the output rows keeps its sentinel."""
    rng = np.random.default_rng(N + 1)
    rowptr, col = graph(rng, N)
    if N == 1:
        rowptr, col = np.array([0, 3], np.int32), np.array([0, 0, 0], np.int32)
    for Cc in (1, 3, 5):
        xw = rng.standard_normal((max(N, 1), Cc + 2)).astype(np.float32)[:N]
        out = Box(4 * max((N - 1) * (Cc + 1) + Cc, 0) + 64)
        x, rp, cl = dev(xw), dev(rowptr), dev(col)
        call('stin_graph_laplace_f32', ptr(x) if N else 0, Cc + 2, ptr(rp), ptr(cl) if col.size else 0, N, Cc, out.ptr, Cc + 1)
        want = O.graph_laplace(xw[:, :Cc], rowptr, col) if N else np.zeros((0, Cc), np.float32)
        assert out.holds(spread(want, Cc + 1)), Cc


# ------------------------------------------------------------------ stin_pad_rows_*, stin_cols_axpy_rowmask_*
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('N,Cin,Cp,ldx', [(1, 10, 12, 10), (257, 10, 16, 13), (5, 4, 4, 6), (0, 10, 12, 10)])
def test_pad_rows_equals_the_restatement(N, Cin, Cp, ldx, bf16):
    rng = np.random.default_rng(N + Cp)
    x = rng.standard_normal((max(N, 1), ldx)).astype(np.float32)[:N]
    if bf16:
        x = O.bf16_bits(x)
    out = Box(x.itemsize * N * Cp + 32)
    d = dev(x)
    call('stin_pad_rows_bf16' if bf16 else 'stin_pad_rows_f32', ptr(d) if N else 0, ldx, N, Cin, Cp, out.ptr)
    assert out.holds(O.pad_rows(x, Cin, Cp))


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('alpha', [-1.0, 0.5])
@pytest.mark.parametrize('N', [1, 43, 300])
def test_cols_axpy_rowmask_equals_the_restatement(N, alpha, bf16):
    """Columns [3, 9) of 10-wide destination rows from 12-wide source rows (and the other way round): fl(d + fl(alpha s)), in bf16
    rounded once more; rows without in-edges and the columns outside the slice keep their bits; c1 == c0 writes nothing."""
    rng = np.random.default_rng(N)
    rowptr, _ = graph(rng, N)
    if N == 1:
        rowptr = np.array([0, 2], np.int32)
    name = 'stin_cols_axpy_rowmask_bf16' if bf16 else 'stin_cols_axpy_rowmask_f32'
    for ldd, lds in ((10, 12), (12, 10)):
        dst, src = (rng.standard_normal((N, ld)).astype(np.float32) for ld in (ldd, lds))
        if bf16:
            dst, src = O.bf16_bits(dst), O.bf16_bits(src)
        box, s, rp = Box.of(dst), dev(src), dev(rowptr)
        call(name, box.ptr, ldd, ptr(s), lds, ptr(rp), N, 3, 3, alpha)
        torch.cuda.synchronize()
        assert box.holds(dst)
        call(name, box.ptr, ldd, ptr(s), lds, ptr(rp), N, 3, 9, alpha)
        want = O.cols_axpy_rowmask(dst, src, rowptr, 3, 9, alpha, bf16)
        assert box.holds(want)
        if N > 1:
            empty = np.diff(rowptr) == 0
            assert empty.any() and not empty.all() and np.array_equal(want[empty], dst[empty])


# ------------------------------------------------------------------ SingleConvMeshNet layer passes
SCMN_SHAPES = [(1, 1, 1), (3, 2, 5), (9, 32, 21), (4, 1, 300)]             # the last: h2 * cout is the largest output


@pytest.mark.parametrize('ti', [0, 1])
@pytest.mark.parametrize('cin,h2,cout', SCMN_SHAPES)
def test_scmn_pack_equals_the_restatement(cin, h2, cout, ti):
    rng = np.random.default_rng(cin + h2 + cout)
    r = lambda *s: rng.standard_normal(s).astype(np.float32)
    host = [r(h2, cin if ti else 2 * cin), r(cout, h2), r(h2), r(h2), r(cout), r(cout)]
    want = O.scmn_pack(*host, cin, h2, cout, ti)
    boxes = {k: Box(v.nbytes) for k, v in want.items()}
    d = [dev(a) for a in host]
    call('stin_scmn_pack_f32', *[ptr(t) for t in d], cin, h2, cout, ti, *[boxes[k].ptr for k in ('wcat', 'wcatT', 'w2T', 'gb1', 'gb2')])
    assert [k for k, b in boxes.items() if not b.holds(want[k].astype(np.float32))] == []


@pytest.mark.parametrize('ti', [0, 1])
@pytest.mark.parametrize('cin,h2,cout', SCMN_SHAPES)
def test_scmn_unpack_equals_the_restatement(cin, h2, cout, ti):
    rng = np.random.default_rng(cin + h2)
    dwcat = rng.standard_normal((2 * h2, cin)).astype(np.float32)
    want = O.scmn_unpack(dwcat, cin, h2, ti)
    box = Box(want.nbytes)
    d = dev(dwcat)
    call('stin_scmn_unpack_f32', ptr(d), cin, h2, ti, box.ptr)
    assert want.dtype == np.float32 and box.holds(want)


#               extra ld, base offset (bytes), res, rowptr, relu / g_eff
LAYER_CONFIGS = [(0, 0, True, True, 1), (4, 0, True, True, 1), (4, 0, False, False, 0), (3, 0, True, True, 1), (1, 0, False, True, 0),
                 (4, 4, True, False, 1), (0, 4, True, True, 0)]


@pytest.mark.parametrize('Cc', [4, 6, 64])
def test_bn_affine_res_equals_the_restatement(Cc):
    """N = 0, 1, 257 x leading dimensions C, C + 4, C + 3, C + 1 x a base offset by one float (the one-channel route for C % 4 == 0)
    x res / rowptr present or NULL x relu: gamma * ((x - mean) * rstd) + beta, * has_in, res + ., relu, each operation rounded."""
    for N in (0, 1, 257):
        for extra, off, has_res, has_rp, relu in LAYER_CONFIGS:
            rng = np.random.default_rng(N + Cc + extra)
            ld = Cc + extra
            xw, rw = (rng.standard_normal((N, ld)).astype(np.float32) for _ in range(2))
            mean, rstd, gamma, beta = (rng.standard_normal(Cc).astype(np.float32) for _ in range(4))
            rowptr, _ = graph(rng, N)
            if N == 257:
                xw[3, 1], xw[5, 0] = np.float32('nan'), np.float32('inf')
            want = O.bn_affine_res(xw[:, :Cc], mean, rstd, gamma, beta, rowptr if has_rp else None, rw[:, :Cc] if has_res else None, relu)
            xb, rb = Box.of(xw, off), Box.of(rw, off)
            y = Box(4 * max((N - 1) * ld + Cc, 0) + 64, off)
            coef, rp = [dev(a) for a in (mean, rstd, gamma, beta)], dev(rowptr)
            call('stin_bn_affine_res_fwd_f32', xb.ptr, ld, *[ptr(t) for t in coef], ptr(rp) if has_rp else 0, rb.ptr if has_res else 0,
                 ld, N, Cc, relu, y.ptr, ld)
            assert y.holds(spread(want, ld)), (N, extra, off, has_res, has_rp, relu)


@pytest.mark.parametrize('Cc', [4, 6, 64])
def test_relu_mask_bwd_equals_the_restatement(Cc):
    """Same grid; y holds +0, -0 and NaN (all three fail y > 0); the last flag of a configuration is relu AND whether g_eff is
    asked for; both outputs are contiguous [N, C]."""
    for N in (0, 1, 257):
        for extra, off, want_eff, has_rp, relu in LAYER_CONFIGS:
            rng = np.random.default_rng(N + Cc + extra + 1)
            ld = Cc + extra
            gw, yw = (rng.standard_normal((N, ld)).astype(np.float32) for _ in range(2))
            if N:
                yw[0, :3] = [0.0, -0.0, np.float32('nan')][:min(3, ld)]
            rowptr, _ = graph(rng, N)
            g_eff, g_in = O.relu_mask_bwd(gw[:, :Cc], yw[:, :Cc], rowptr if has_rp else None, relu)
            gb, yb = Box.of(gw, off), Box.of(yw, off)
            eff, gin = Box(4 * N * Cc + 64, off), Box(4 * N * Cc + 64, off)
            rp = dev(rowptr)
            call('stin_relu_mask_bwd_f32', gb.ptr, ld, yb.ptr if relu else 0, ld, ptr(rp) if has_rp else 0, N, Cc, relu,
                 eff.ptr if want_eff else 0, gin.ptr)
            assert gin.holds(g_in), (N, extra, off, want_eff, has_rp, relu)
            assert eff.holds(g_eff if want_eff else np.zeros(0, np.float32)), (N, extra, off, want_eff, has_rp, relu)


# ------------------------------------------------------------------ stin_norm_bwd_coef_f32 / _m_quirk_f32
@pytest.mark.parametrize('B,Cc', [(1, 1), (3, 64), (2, 257)])
def test_norm_bwd_coefficients_equal_the_restatement(B, Cc):
    rng = np.random.default_rng(B + Cc)
    T1, S0, Uq = (rng.standard_normal((B, Cc)).astype(np.float32) for _ in range(3))
    rstd = rng.uniform(0.1, 30.0, (B, Cc)).astype(np.float32)
    inv_cnt = (1.0 / rng.integers(1, 5000, B)).astype(np.float32)
    d = {k: dev(v) for k, v in dict(T1=T1, S0=S0, U=Uq, rstd=rstd, ic=inv_cnt).items()}
    k, m, mq = Box(4 * B * Cc), Box(4 * B * Cc), Box(4 * B * Cc)
    call('stin_norm_bwd_coef_f32', ptr(d['T1']), ptr(d['S0']), ptr(d['rstd']), ptr(d['ic']), B, Cc, k.ptr, m.ptr)
    call('stin_norm_bwd_coef_m_quirk_f32', ptr(d['S0']), ptr(d['U']), ptr(d['rstd']), ptr(d['ic']), B, Cc, mq.ptr)
    want_k, want_m = O.norm_bwd_coef(T1, S0, rstd, inv_cnt)
    assert want_k.dtype == np.float32 and k.holds(want_k) and m.holds(want_m)
    assert mq.holds(O.norm_bwd_coef_m_quirk(S0, Uq, rstd, inv_cnt))
