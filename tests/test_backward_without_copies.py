"""The backward half without its two row copies (stin_net_op_t::x_from_src / g_in_dy, functional.USE_WGRAD_MAP / USE_G_IN_DY):
 * a block behind an unpool step never materialises x_up = x_c[trace]: the one backward reader of x, the packed weight-gradient
   product dY^T [x | 1], reads x_c through the trace (stin_edgeconv_wgrad_map, the mapped producer of k_gemm_tn_ws);
 * the op behind a shortcut block writes its input gradient straight into the shortcut columns of that block's dY = [dA | dB | g].
Only addresses change, so every comparison here is torch.equal.

The whole-network runs use ngf = 64, the narrowest network whose blocks take the one-node path at all (it needs H = 2 Cout in
{128, 256, ...}: functional.edge_mask_supported); there both decoder blocks are mapped, and the gather fall-back is reached through
the predicate saying 0 (STIN_TN_WS=0).  The ngf = 8 and ngf = 16 networks run block by block through the per-op functions - no flag
can engage - and are compared across the switches all the same."""
import ctypes
import functools
import os
import struct
import subprocess
import sys

import pytest
import torch

from surface_texture_inpainting_net_amd import _lib
from surface_texture_inpainting_net_amd import functional as SF
from surface_texture_inpainting_net_amd import surfacetextureinpaintingnet as S
from surface_texture_inpainting_net_amd.plan import _ptr, _stream
from surface_texture_inpainting_net_amd.synthetic import make_synthetic_mesh

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_C = _lib.CONSTANTS
BF16X3 = 2


# ------------------------------------------------------------------------------------------------ 1. the mapped product
def _wgrad_case(n_in, N, Cp, H, Cout, seed):
    """Operands of one block's weight gradients: dagg, hE (+ indicator column), dY = [dA | dB | g], coarse rows and a trace."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    Yw = 2 * H + Cout
    dagg = torch.randn(N, Cout, generator=g, device=DEV)
    hE = torch.randn(N, H + 4, generator=g, device=DEV)
    hE[:, H] = (torch.arange(N, device=DEV) % 5 != 0).float()
    hE[:, H + 1:] = 0
    dY = torch.randn(N, Yw, generator=g, device=DEV)
    # the coarse rows sit at the head of a LARGER allocation whose other rows are huge: an index read from behind the trace
    # lands on one of them - a wrong sum, never a fault
    extra = 64
    x_big = torch.full((n_in + extra, Cp), 3.0e30, device=DEV)
    x_big[:n_in] = torch.randn(n_in, Cp, generator=g, device=DEV)
    cg = torch.Generator().manual_seed(seed)
    used = torch.tensor([c for c in range(n_in) if c % 7 != 3])            # coarse rows nobody maps to
    t = used[torch.randint(0, len(used), (N,), generator=cg)]
    t[:5] = t[5]                                                            # repeated rows
    t[7], t[N - 1] = 0, n_in - 1
    assert 0 in t.tolist() and n_in - 1 in t.tolist() and len(torch.unique(t)) < n_in
    trace_buf = torch.full((N + 64,), n_in + extra - 1, dtype=torch.int32, device=DEV)     # the poison behind the N entries
    trace_buf[:N] = t.to(torch.int32).to(DEV)
    return dagg, hE, dY, x_big, trace_buf


def _grads(Cin, H, Cout):
    z = lambda *s: torch.full(s, float('nan'), device=DEV)
    return [z(H, Cin), z(H), z(Cout, H), z(Cout), z(Cout, Cin), z(Cout)]


@pytest.mark.gpu
@pytest.mark.parametrize('n_in,N,Cp,H,Cout', [(97, 331, 32, 32, 32), (1201, 3975, 128, 64, 64)])
def test_mapped_weight_gradient_equals_the_product_on_gathered_rows(n_in, N, Cp, H, Cout):
    """(a) 331 rows (no multiple of 4 or 32), Nc = Yw = 96: one partial tile, one partial chunk.  (b) 3975 rows, Nc = 192 (two
    tiles of dY's columns), K = 128: several row chunks of which the last is partial.  All six gradients, bit for bit."""
    lib = _lib.load()
    Yw = 2 * H + Cout
    dagg, hE, dY, x_big, trace_buf = _wgrad_case(n_in, N, Cp, H, Cout, seed=N)
    assert lib.stin_edgeconv_wgrad_map_supported(N, Cp, H, Cout, 1, BF16X3) == 1
    # chunk count of the packed product, from the workspace query: chunks x (Nc Kq + roundup4(Nc)) floats + 256 bytes
    chunks = (lib.stin_gemm_tn_workspace_bytes(N, Yw, Cp, 1) - 256) // (4 * (Yw * Cp + Yw))
    if N > 1000:
        assert chunks >= 2 and N % 32 != 0, chunks                # (chunks are whole 32-row slabs: the last one is partial)
    ws_bytes = lib.stin_edgeconv_wgrad_workspace_bytes(N, Cp, H, Cout, 1)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    trace = trace_buf[:N]
    x_f = x_big[trace.long()].contiguous()
    assert float(x_f.abs().max()) < 1e3
    want, got = _grads(Cp, H, Cout), _grads(Cp, H, Cout)
    rc = lib.stin_edgeconv_wgrad_ti(0, _ptr(dagg), Cout, _ptr(hE), H + 4, _ptr(dY), Yw, _ptr(x_f), Cp, N, Cp, Cp, H, Cout, 1, 1, BF16X3,
                                    *[_ptr(t) for t in want], 0, 0, _ptr(ws), ws_bytes, _stream(dY))
    assert rc == 0
    torch.cuda.synchronize()
    rc = lib.stin_edgeconv_wgrad_map(0, _ptr(dagg), Cout, _ptr(hE), H + 4, _ptr(dY), Yw, _ptr(x_big), Cp, N, Cp, Cp, H, Cout, 1, 1, BF16X3,
                                     *[_ptr(t) for t in got], _ptr(trace_buf), n_in, _ptr(ws), ws_bytes, _stream(dY))
    assert rc == 0
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(got, want)):
        assert bool(torch.isfinite(b).all()) and float(b.abs().max()) > 0, i
        assert torch.equal(a, b), i


# ------------------------------------------------------------------------------------------------ 2. the predicate (no GPU)
def test_map_predicate_and_the_unsupported_call():
    """Cp = 16 runs on the skinny kernel (no mapped variant): predicate 0 and STIN_E_UNSUPPORTED from the call, before any launch;
    Cp = 32 is the producer / consumer kernel's.  STIN_TN_WS=0 takes every shape off that kernel."""
    lib = _lib.load()
    N, H, Cout = 700, 32, 32
    assert lib.stin_edgeconv_wgrad_map_supported(N, 16, H, Cout, 1, BF16X3) == 0
    assert lib.stin_edgeconv_wgrad_map_supported(N, 32, H, Cout, 1, BF16X3) == 1
    assert lib.stin_edgeconv_wgrad_map_supported(N, 32, H, Cout, 1, 0) == 0                  # exact-fp32 products: another kernel
    assert lib.stin_edgeconv_wgrad_map_supported(0, 32, H, Cout, 1, BF16X3) == 0
    old = os.environ.get('STIN_TN_WS')
    os.environ['STIN_TN_WS'] = '0'
    try:
        assert lib.stin_edgeconv_wgrad_map_supported(N, 32, H, Cout, 1, BF16X3) == 0
    finally:
        if old is None:
            del os.environ['STIN_TN_WS']
        else:
            os.environ['STIN_TN_WS'] = old
    # host memory stands in for the operands: the call must refuse before it launches anything
    Yw = 2 * H + Cout
    f = lambda *s: torch.zeros(*s)
    ws_bytes = lib.stin_edgeconv_wgrad_workspace_bytes(N, 16, H, Cout, 1)
    ws = torch.zeros(ws_bytes + 256, dtype=torch.uint8)
    trace = torch.zeros(N, dtype=torch.int32)
    out = [f(H, 16), f(H), f(Cout, H), f(Cout), f(Cout, 16), f(Cout)]
    rc = lib.stin_edgeconv_wgrad_map(0, f(N, Cout).data_ptr(), Cout, f(N, H + 4).data_ptr(), H + 4, f(N, Yw).data_ptr(), Yw,
                                     f(97, 16).data_ptr(), 16, N, 16, 16, H, Cout, 1, 1, BF16X3, *[t.data_ptr() for t in out],
                                     trace.data_ptr(), 97, ws.data_ptr(), ws_bytes, None)
    assert rc == _C['STIN_E_UNSUPPORTED']
    assert all(float(t.abs().max()) == 0.0 for t in out)


# ------------------------------------------------------------------------------------------------ 3. the network
def _cfg(ngf):
    return dict(input_nc=10, output_nc=3, ngf=ngf, filter_type='edgeconvtransinv', norm='instance', n_blocks=2, n_levels=2,
                pooling_type='max', dilations=[1, 2])


@functools.lru_cache(maxsize=None)
def _sample(batched):
    from surface_texture_inpainting_net_amd.data import collate
    if batched:
        return collate([make_synthetic_mesh(n, 3, seed=40 + i, dilations=(2,)) for i, n in enumerate((300, 450))]).to(DEV)
    return make_synthetic_mesh(700, 3, seed=40, dilations=(2,)).to(DEV)


def _ops(raw, n):
    op = _lib.STRUCTS['stin_net_op_t']
    return [dict(zip(op.fields, struct.unpack(op.format, raw[i * op.size:(i + 1) * op.size]))) for i in range(n)]


def _train(ngf, batched, use_map, use_gdy):
    """One training forward + loss + backward -> dict(res = [loss, dx, parameter gradients], skipped, arena, ops, raw)."""
    s = _sample(batched)
    old = (SF.USE_WGRAD_MAP, SF.USE_G_IN_DY, SF._call)
    SF.USE_WGRAD_MAP, SF.USE_G_IN_DY = use_map, use_gdy
    tables, arenas = [], []

    def spy(name, *a, **kw):
        if name == 'stin_net_bwd':
            tables.append((bytes(a[1].raw), int(a[2])))
        return old[2](name, *a, **kw)

    def pack(t):
        if t.dtype == torch.uint8 and t.dim() == 1:
            arenas.append(t.numel())
        return t
    SF._call = spy
    try:
        torch.manual_seed(17)
        net = S.define_G(**_cfg(ngf)).to(DEV)
        x = s.x.clone().requires_grad_(True)
        s2 = type(s)(**{k: (x if k == 'x' else s[k]) for k in s.keys()})
        s2._nv_host = s._nv_host
        k0 = SF.NetFn.gathers_skipped
        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            out = net(s2)
        skipped = SF.NetFn.gathers_skipped - k0
        loss = out.float().square().mean()
        loss.backward()
        torch.cuda.synchronize()
        res = [loss.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in net.parameters()]
    finally:
        SF.USE_WGRAD_MAP, SF.USE_G_IN_DY, SF._call = old
    raw, n = max(tables, key=lambda t: t[1]) if tables else (b'', 0)
    return dict(res=res, skipped=skipped, arena=max(arenas) if arenas else 0, ops=_ops(raw, n), raw=raw)


@functools.lru_cache(maxsize=None)
def _all_off(ngf, batched):
    return _train(ngf, batched, False, False)


def _same(a, b):
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        assert bool(torch.isfinite(v).all()), i
        assert torch.equal(u, v), i


@pytest.mark.gpu
@pytest.mark.parametrize('batched', [False, True])
@pytest.mark.parametrize('ngf', [8, 16])
def test_narrow_networks_do_not_change_with_the_switches(ngf, batched):
    """H < 128: these networks run block by block on the per-op functions (the bitwise reference), whatever the switches say."""
    want = _all_off(ngf, batched)
    for use_map, use_gdy in ((True, False), (False, True), (True, True)):
        got = _train(ngf, batched, use_map, use_gdy)
        _same(got['res'], want['res'])
        assert got['skipped'] == want['skipped'] == 0


@pytest.mark.gpu
@pytest.mark.parametrize('batched', [False, True])
def test_network_without_the_backward_copies_equals_all_off_bitwise(batched):
    """ngf = 64: the graph part is one NetFn node; both decoder blocks read x through the trace, every shortcut block gets its g
    written into its dY.  Loss, input gradient and every parameter gradient for each switch combination against all-off; the
    gathers not launched, the arena bytes not reserved, and exactly which ops are redirected (host-only predicate)."""
    lib = _lib.load()
    want = _all_off(64, batched)
    ops_off = want['ops']
    kinds = [o['kind'] for o in ops_off]
    BLOCK, POOL, UNPOOL = _C['STIN_OP_BLOCK'], _C['STIN_OP_POOL_MAX'], _C['STIN_OP_UNPOOL']
    assert kinds.count(UNPOOL) == 2 and kinds.count(POOL) == 2 and want['skipped'] == 0
    assert not any(o['x_from_src'] or o['g_in_dy'] for o in ops_off) and sum(o['y_from_src'] for o in ops_off) == 2
    n = len(ops_off)
    buf = ctypes.create_string_buffer(want['raw'], len(want['raw']))
    assert [lib.stin_net_bwd_g_in_dy(0, buf, n, i) for i in range(n)] == [0] * n
    for use_map, use_gdy in ((True, False), (False, True), (True, True)):
        got = _train(64, batched, use_map, use_gdy)
        _same(got['res'], want['res'])
        ops = got['ops']
        assert [o['kind'] for o in ops] == kinds
        mapped = [o for o in ops if o['x_from_src']]
        assert len(mapped) == (2 if use_map else 0) == got['skipped']
        for o in mapped:                                            # ... and neither the block nor the unpool op holds the rows
            assert o['x'] == 0 and o['y_from_src'] == 1
        assert want['arena'] - got['arena'] == sum(o['n_out'] * o['Cin'] * 4 for o in mapped)
        assert all((o['n_out'] * o['Cin'] * 4) % 256 == 0 for o in mapped)
        # redirected: exactly the ops behind a shortcut block - a pool step (behind the compact first block too), an unpool step, a block
        buf = ctypes.create_string_buffer(got['raw'], len(got['raw']))
        red = [i for i in range(n) if lib.stin_net_bwd_g_in_dy(0, buf, n, i)]
        expect = [i for i in range(1, n) if ops[i - 1]['kind'] == BLOCK and ops[i - 1]['has_shortcut']] if use_gdy else []
        assert red == expect and 0 not in red
        if use_gdy:
            assert {ops[i]['kind'] for i in red} == {BLOCK, POOL, UNPOOL}
            assert ops[0]['trans_inv'] == _C['STIN_TI_COMPACT'] and ops[0]['has_shortcut'] and 1 in red and ops[1]['kind'] == POOL
            assert sum(o['g_in_dy'] for o in ops) == sum(1 for o in ops if o['kind'] == BLOCK and o['has_shortcut']) == 5
            for v in (-1, n, n + 3):
                assert lib.stin_net_bwd_g_in_dy(0, buf, n, v) == 0
            assert [lib.stin_net_bwd_g_in_dy(1, buf, n, i) for i in range(n)] == [0] * n          # bf16 rows: never


@pytest.mark.gpu
def test_shapes_off_the_producer_consumer_kernel_keep_the_gather():
    """The predicate says 0 (here: STIN_TN_WS=0 puts every product on the four-wave kernel) -> no flag, the gather runs, x is kept."""
    want = _all_off(64, False)
    old = os.environ.get('STIN_TN_WS')
    os.environ['STIN_TN_WS'] = '0'
    try:
        got = _train(64, False, True, True)
    finally:
        if old is None:
            del os.environ['STIN_TN_WS']
        else:
            os.environ['STIN_TN_WS'] = old
    assert got['skipped'] == 0 and not any(o['x_from_src'] for o in got['ops']) and got['arena'] == want['arena']
    # (the four-wave kernel's slabs equal the producer / consumer kernel's: tests/test_hip_parity.py - so do the gradients)
    _same(got['res'], want['res'])


# ------------------------------------------------------------------------------------------------ 4. STIN_UNPOOL_COMMUTE=0
_CHILD = r"""
import os, sys
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, 'tests'))
import torch
import test_backward_without_copies as T
from surface_texture_inpainting_net_amd import functional as SF
assert not SF.USE_UNPOOL_COMMUTE and SF.USE_WGRAD_MAP and SF.USE_G_IN_DY
r = T._train(64, False, True, True)
assert r['skipped'] == 0 and not any(o['x_from_src'] or o['y_from_src'] for o in r['ops'])
torch.save([t.cpu() for t in r['res']] + [torch.tensor(r['arena'])], sys.argv[1])
print('OK')
"""


@pytest.mark.gpu
def test_unpool_commute_switch_turns_the_mapped_backward_off(tmp_path):
    """STIN_UNPOOL_COMMUTE=0 in a fresh interpreter: no commutation, hence no mapped weight gradient and the full arena of the
    un-commuted plan - and the same bits as all-off."""
    want = _all_off(64, False)
    path = str(tmp_path / 'child.pt')
    env = dict(os.environ, STIN_UNPOOL_COMMUTE='0')
    r = subprocess.run([sys.executable, '-c', _CHILD % (ROOT, ROOT), path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'OK' in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    got = torch.load(path)
    assert int(got[-1]) > want['arena']                       # (Y of the two decoder blocks over the fine rows)
    _same([t.to(DEV) for t in got[:-1]], want['res'])


# ------------------------------------------------------------------------------------------------ 5. under checkpoint
@pytest.mark.gpu
def test_decoder_pair_under_non_reentrant_checkpoint():
    """unpool -> block -> unpool -> block as ONE NetFn inside torch.utils.checkpoint(use_reentrant=False): the first pass is a
    no-grad forward, backward recomputes with grad and is handed the RECOMPUTED saved tensors - which must hold the coarse rows the
    mapped weight gradient reads.  Gradients equal the un-checkpointed run's."""
    from torch.utils.checkpoint import checkpoint
    s = _sample(False)
    torch.manual_seed(23)
    net = S.define_G(**_cfg(64)).to(DEV)
    plan = S.plan_for(s, linspace_quirk=net.compat_linspace_norm, validation=net.plan_validation, positions=net.position_channels)
    plan.ensure(*net._plan_items())
    d1, d2 = list(net.decoder_blocks)
    steps = [('unpool', plan.pool(2)), ('block', d1, plan.edges('hierarchy_edge_index_1', 1), net._norm_arg(plan, 1)),
             ('unpool', plan.pool(1)), ('block', d2, plan.edges('edge_index', 0), net._norm_arg(plan, 0))]
    params = list(d1.parameters()) + list(d2.parameters())
    g = torch.Generator(device=DEV).manual_seed(5)
    x0 = torch.randn(plan.pool(2).n_coarse, 256, generator=g, device=DEV)
    assert SF.net_eligible(steps, x0) and SF.USE_WGRAD_MAP and SF.USE_G_IN_DY

    def run(ckpt):
        for p in params:
            p.grad = None
        x = x0.clone().requires_grad_(True)
        k0 = SF.NetFn.gathers_skipped
        y = checkpoint(lambda t: SF.run_net(t, steps), x, use_reentrant=False) if ckpt else SF.run_net(x, steps)
        y.square().mean().backward()
        torch.cuda.synchronize()
        return [y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in params], SF.NetFn.gathers_skipped - k0
    plain, k_plain = run(False)
    ck, k_ck = run(True)
    assert k_plain == 2 and k_ck == 4                              # (the no-grad pass and the recomputation skip both gathers each)
    _same(ck, plain)
