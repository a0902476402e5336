"""The plan of a functional.NetFn (plan_net: shapes, decisions, arena layout) on a machine without a GPU: real GraphResnetBlock
modules on the CPU, SimpleNamespace objects for the edge sets, norm groups and pool maps - the planner reads their integer
attributes only.  Op list: block(10 -> 64, shortcut) . pool . block(64 -> 128, shortcut) . unpool . block(128 -> 64, shortcut) .
block(64 -> 64); 700 fine and 211 coarse rows, H = 128 / 256, prime edge counts.  The training layout must keep every slot apart;
the no-grad layout shares regions between ops, so there every op's own reads and writes must stay apart - the aliasing no GPU
test looks at."""
import itertools
from types import SimpleNamespace as NS

import pytest
import torch

from surface_texture_inpainting_net_amd import _lib
from surface_texture_inpainting_net_amd import functional as SF
from surface_texture_inpainting_net_amd import modules as M
from surface_texture_inpainting_net_amd import surfacetextureinpaintingnet as S

N_FINE, N_COARSE, E_FINE, E_COARSE = 700, 211, 4201, 1259
BLOCK, POOL, UNPOOL = SF.OP_BLOCK, SF.OP_POOL_MAX, SF.OP_UNPOOL


def _block(dim_in, dim_out, trans_inv=False):
    kw = dict(module=M.EdgeConvTransInv, double_input=False) if trans_inv else {}
    return S.GraphResnetBlock(dim_in, dim_out, M.get_gcn_filter, M.FastInstanceNorm, False, True, **kw)


def _steps(mid=128, decoder_trans_inv=False):
    """The op list of the module docstring; `mid`: the width between the encoder and the decoder block."""
    fine, coarse = NS(n_edges=E_FINE), NS(n_edges=E_COARSE)
    one = NS(B=1, quirk=False)
    pool = NS(n_fine=N_FINE, n_coarse=N_COARSE)
    first = _block(10, 64, trans_inv=True)
    first.unbounded_input = True
    return [('block', first, fine, one), ('pool', pool), ('block', _block(64, mid), coarse, one), ('unpool', pool),
            ('block', _block(mid, 64, decoder_trans_inv), fine, one), ('block', _block(64, 64), fine, one)]


def _plan(need_grad, b16=False, **kw):
    steps = _steps(**kw)
    plan = SF.plan_net(steps, [p for st in steps if st[0] == 'block' for p in st[1].fused_params()], N_FINE, 10, b16, need_grad)
    assert [op.kind for op in plan.ops] == [BLOCK, POOL, BLOCK, UNPOOL, BLOCK, BLOCK]
    assert (plan.n_rows, plan.width) == (N_FINE, 64)
    assert [op.shape.H for op in plan.ops if op.kind == BLOCK] == [128, 2 * kw.get('mid', 128), 128, 128]
    return plan


def _up256(n):
    return (n + 255) // 256 * 256


def _apart(slots):
    return all(a.offset + a.nbytes <= b.offset or b.offset + b.nbytes <= a.offset for a, b in itertools.combinations(slots, 2))


def _own(op):
    """The Slots of an op's own buffers by the record's field names (mean: mean | rstd, wcatT: wcatT | w2T), without its input."""
    return {k: s for k, (s, at) in op.rel.items() if k != 'x' and s is not None and at == 0}


def _mapped_on_the_producer_consumer_kernel():
    return _lib.load().stin_edgeconv_wgrad_map_supported(N_FINE, 128, 128, 64, 1, int(SF.PREC_BWD)) == 1


def test_block_shape_is_what_the_three_functions_it_calls_say():
    for b16, unbounded in itertools.product((False, True), repeat=2):
        sh = SF.block_shape((128, 10), (64, 128), True, True, unbounded, b16)
        prec = SF.forward_precision(unbounded)
        ti = SF.trans_inv_mode(True, b16, 128)
        assert sh == (10, 16 if b16 else 12, 128, 64, True, ti, SF.block_yw(128, 64, True, ti), prec) + SF.block_split_modes(prec, b16, 64)
    assert SF.block_shape((256, 128), (128, 256), True, False, False, False, width=64).Cin == 64       # [x_i, x_j - x_i]: W1 is 2 Cin wide
    with pytest.raises(AssertionError):
        SF.block_shape((256, 128), (128, 256), True, False, False, False, width=128)


def test_training_layout_keeps_every_slot_apart():
    assert _mapped_on_the_producer_consumer_kernel()
    plan = _plan(True)
    slots = plan.arena.slots
    assert all(s.offset % 256 == 0 and s.nbytes > 0 for s in slots) and _apart(slots)
    last = max(slots, key=lambda s: s.offset)
    assert plan.arena.nbytes == _up256(last.offset + last.nbytes) == sum(_up256(s.nbytes) for s in slots)
    # every buffer of every op is one of them: 7 per block (they pack for themselves: + 2), the arg-max rows, the outputs
    named = [s for op in plan.ops for s in list(_own(op).values()) + [op.out] * (op.out is not None)]
    assert sorted(map(id, named)) == sorted(map(id, slots))
    for op in plan.ops:
        assert sorted(_own(op)) == (['Y', 'agg', 'fwd_ws', 'hE', 'mask', 'mean', 'wcatT'] if op.kind == BLOCK else ['arg'] * (op.kind == POOL))
        if op.kind == BLOCK:
            assert op.rel['mask'][0].nbytes == op.edges.n_edges * (op.shape.H // 32) * 4
            assert op.rel['rstd'] == (op.rel['mean'][0], op.shape.Cout * 4) and op.rel['w2T'] == (op.rel['wcatT'][0], op.shape.Yw * op.shape.Cp * 4)
    # every op reads the rows the op in front wrote
    assert [op.rel['x'][0] for op in plan.ops] == [None] + [op.out for op in plan.ops[:-1]]
    assert plan.ops[-1].out is None and all(op.out is not None for op in plan.ops[:3])


def test_decoder_block_reads_the_coarse_rows_in_both_directions():
    assert _mapped_on_the_producer_consumer_kernel()
    plan = _plan(True)
    unpool, dec = plan.ops[3], plan.ops[4]
    assert dec.src is unpool and dec.x_from_src and unpool.writes_no_rows and unpool.out is None and dec.rel['x'][0] is None
    assert dec.rel['Y'][0].nbytes == N_COARSE * dec.shape.Yw * 4                      # Y holds the coarse rows only
    assert [op.src for op in plan.ops if op.kind == BLOCK and op is not dec] == [None] * 3
    assert not any(op.writes_no_rows for op in plan.ops if op.kind == POOL)


def test_without_the_mapped_weight_gradient_the_unpooled_rows_are_back(monkeypatch):
    with_map = _plan(True)
    monkeypatch.setattr(SF, 'USE_WGRAD_MAP', False)
    plan = _plan(True)
    unpool, dec = plan.ops[3], plan.ops[4]
    assert dec.src is unpool and not dec.x_from_src and not unpool.writes_no_rows
    assert unpool.out is not None and unpool.out.nbytes == N_FINE * 128 * 4
    assert plan.arena.nbytes - with_map.arena.nbytes == _up256(N_FINE * 128 * 4)


@pytest.mark.parametrize('case', ['switch', 'bf16', 'compact', 'width'])
def test_where_the_first_product_stays_on_the_unpooled_rows(case, monkeypatch):
    """USE_UNPOOL_COMMUTE = False, bf16 storage, a compact translation-invariant decoder block, a width that is no multiple of 4."""
    if case == 'switch':
        monkeypatch.setattr(SF, 'USE_UNPOOL_COMMUTE', False)
    kw = dict(compact=dict(decoder_trans_inv=True), width=dict(mid=126)).get(case, {})
    for need_grad in (True, False):
        plan = _plan(need_grad, b16=case == 'bf16', **kw)
        unpool, dec = plan.ops[3], plan.ops[4]
        if case == 'compact':
            assert dec.shape.ti == SF.TI_MODE_COMPACT
        assert dec.src is None and not dec.x_from_src and not unpool.writes_no_rows and unpool.out is not None
        assert dec.rel['Y'][0].nbytes == N_FINE * dec.shape.Yw * (2 if case == 'bf16' else 4)


@pytest.mark.parametrize('b16', [False, True])
def test_no_grad_layout_keeps_what_one_op_touches_apart(b16):
    """Temporaries restart per op and outputs alternate between two regions: within ONE op's launch sequence its temporaries, its
    input, its output and - for a block on the coarse rows - the unpool step's input must not overlap."""
    plan = _plan(False, b16=b16)
    ops = plan.ops
    assert (ops[4].src is ops[3]) == (not b16)
    tmp_bytes, out_bytes = [], []
    for i, op in enumerate(ops):
        tmps = list(_own(op).values())
        assert tmps or op.kind == UNPOOL
        touched = tmps + [op.out] * (op.out is not None)
        if op.rel['x'][0] is not None:
            assert op.rel['x'][0] is ops[i - 1].out
            touched.append(op.rel['x'][0])                       # its input rows
        if op.kind == BLOCK and op.src is not None:
            assert ops[i - 1] is op.src and op.src.out is None and op.src.writes_no_rows
            touched.append(ops[i - 2].out)                       # the unpool step's input: the rows Y is computed from
        assert all(s.offset % 256 == 0 for s in touched) and _apart(touched), i
        assert all(s.offset + s.nbytes <= plan.arena.nbytes for s in touched)
        tmp_bytes.append(sum(_up256(s.nbytes) for s in tmps))
        out_bytes.append(_up256(op.out.nbytes) if op.out is not None else 0)
    assert all(op.rel['mask'][0] is None for op in ops if op.kind == BLOCK)
    assert (ops[3].out is None) == (not b16) and ops[-1].out is None
    # [kept | out 0 | out 1 | temporaries] with nothing kept
    assert plan.arena.nbytes == 2 * max(out_bytes) + max(tmp_bytes)
