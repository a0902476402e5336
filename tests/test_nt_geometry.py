"""The routes of the NT products, asked of the host-only query stin_gemm_nt_geometry (no GPU): every point of tests/_nt_table.py
must reach the kernel family, tile, parameter, grid and LDS its line names, or the refusal it names.  tests/test_nt_routes_gpu.py
runs the launchable points on the GPU; this file is the check that they aim where they say - a change of a route rule shows up here
first."""
import ctypes

import pytest

import _nt_table as T
from surface_texture_inpainting_net_amd import _lib

_C = _lib.CONSTANTS


def test_constants_of_the_table():
    assert (T.F32, T.X3, T.X6, T.F16) == tuple(_C['STIN_GEMM_' + n] for n in ('F32', 'BF16X3', 'BF16X6', 'F16X3'))
    assert (T.PRE, T.FRAG, T.WB16) == (_C['STIN_GEMM_W_PRESPLIT'], _C['STIN_GEMM_W_FRAG'], _C['STIN_GEMM_W_BF16'])
    families = ('NONE', 'TILED', 'STREAM', 'STRIP', 'WIDE', 'PANEL', 'B16_TILED', 'B16_GLDS')
    assert tuple(_C['STIN_NT_' + n] for n in families) == (T.NONE, T.TILED, T.STREAM, T.STRIP, T.WIDE, T.PANEL, T.B16_TILED, T.B16_GLDS)
    parts = ('BIAS', 'ROW_MASK', 'RESIDUAL', 'COLSTATS', 'DOTELU', 'BN_TF', 'BN_BWD_STATS', 'BN_BWD_APPLY', 'OUT_F32', 'STREAM_ONLY')
    assert tuple(_C['STIN_NT_PART_' + n] for n in parts) == (T.BIAS, T.MASK, T.RES, T.COLSTATS, T.DOTELU, T.BN_TF, T.BWD_STATS, T.BWD_APPLY,
                                                             T.OUT_F32, T.STREAM_ONLY)
    assert tuple(_C['STIN_NT_ALIGN_' + n] for n in ('IN', 'OUT', 'TF', 'BIAS')) == (T.A_IN, T.A_OUT, T.A_TF, T.A_BIAS)
    assert (T.E_ALIGN, T.E_UNSUPPORTED) == (_C['STIN_E_ALIGN'], _C['STIN_E_UNSUPPORTED'])


@pytest.mark.parametrize('p', T.POINTS, ids=lambda p: p.id)
def test_point_reaches_its_route(p, monkeypatch):
    lib = _lib.load()
    T.set_env(monkeypatch, p.env)
    rc, g = T.geometry(lib, p)
    assert rc == p.rc, (p.id, rc, g)
    if rc != 0:
        assert set(g.values()) == {-77}, (p.id, g)            # a refusal writes nothing
        return
    assert g['family'] == p.family, (p.id, g)
    assert (g['bm'], g['bn']) == p.tile, (p.id, g)
    assert (g['param'], g['vec'], g['vec_out'], g['groups']) == (p.param, p.vec, p.vec_out, p.groups), (p.id, g)
    if p.grid is not None:
        assert (g['gx'], g['gy']) == p.grid, (p.id, g)
    if p.lds is not None:
        assert g['lds'] == p.lds, (p.id, g)
    assert 0 <= g['lds'] <= 160 * 1024


@pytest.mark.parametrize('p', [p for p in T.POINTS if p.storage == 0 and p.cu == 256 and p.parts & (T.COLSTATS | T.BWD_STATS)],
                         ids=lambda p: p.id)
def test_groups_entry_points_return_the_table_number(p, monkeypatch):
    """The three *_groups queries answer for the ALIGNED form of a shape, without its bias / mask / residual: the count the launch of the
    point then writes.  The one point whose launch is refused (column statistics with a residual on a panel shape) still has a count."""
    lib = _lib.load()
    T.set_env(monkeypatch, p.env)
    if p.parts & T.BWD_STATS:
        fn = lib.stin_gemm_nt_bn_bwd_groups
    else:
        fn = lib.stin_gemm_nt_dotelu_groups if p.parts & T.DOTELU else lib.stin_gemm_nt_colstats_groups
    want = {'panel-colstats-residual': 128}.get(p.id, p.groups)          # 4091 rows in row blocks of 64: 64 x 2
    assert fn(p.M, p.Nc, p.K, p.prec) == want, p.id
    if p.parts & T.BWD_STATS:
        monkeypatch.setenv('STIN_NT_BNBWD', '0')
        assert fn(p.M, p.Nc, p.K, p.prec) == 0


def test_table_covers_every_family_parameter_and_switch():
    ok = [p for p in T.POINTS if p.rc == 0]
    assert {p.family for p in ok} == set(range(8))
    assert {p.param for p in ok if p.family == T.PANEL} == set(range(2, 10))
    assert {p.param for p in ok if p.family == T.STRIP} == {21, 22, 41}
    assert {(p.tile[0], p.param) for p in ok if p.family == T.WIDE} == {(128, 2), (64, 1)}
    assert {p.param for p in ok if p.family == T.STREAM} == {2, 4}
    assert {p.tile for p in ok if p.family == T.TILED} == {(128, 32), (64, 64), (128, 128)}
    assert {p.tile for p in ok if p.family == T.B16_TILED} == {(128, 32), (64, 64), (128, 64)}
    assert {p.tile for p in ok if p.family == T.B16_GLDS} == {(128, 128), (256, 256)}
    assert {(p.family, p.vec_out) for p in ok if p.family in (T.STRIP, T.WIDE)} == {(T.STRIP, 0), (T.STRIP, 1), (T.WIDE, 0), (T.WIDE, 1)}
    assert {k for p in T.POINTS for k in p.env} | {'STIN_NT_BNBWD'} == set(T.SWITCHES)
    assert {p.rc for p in T.POINTS} == {0, T.E_ALIGN, T.E_UNSUPPORTED}


def test_query_argument_errors_and_no_write_on_error():
    lib = _lib.load()
    out = (ctypes.c_int32 * 10)(*([77] * 10))
    at = ctypes.addressof(out)
    al = T.A_IN | T.A_OUT | T.A_TF | T.A_BIAS
    assert lib.stin_gemm_nt_geometry(0, 100, 64, 64, T.X3, 0, al, 256, None) == _C['STIN_E_NULL']
    assert lib.stin_gemm_nt_geometry(2, 100, 64, 64, T.X3, 0, al, 256, at) == _C['STIN_E_UNSUPPORTED']
    assert lib.stin_gemm_nt_geometry(0, -1, 64, 64, T.X3, 0, al, 256, at) == _C['STIN_E_SIZE']
    assert lib.stin_gemm_nt_geometry(0, 100, 0, 64, T.X3, 0, al, 256, at) == _C['STIN_E_SIZE']
    assert lib.stin_gemm_nt_geometry(0, 100, 64, 64, T.X3, 0, al, 0, at) == _C['STIN_E_SIZE']             # cu > 0
    assert lib.stin_gemm_nt_geometry(0, 100, 64, 64, 1, 0, al, 256, at) == _C['STIN_E_UNSUPPORTED']       # no such precision
    assert lib.stin_gemm_nt_geometry(0, 100, 64, 64, T.F32 | T.PRE, 0, al, 256, at) == _C['STIN_E_UNSUPPORTED']
    assert lib.stin_gemm_nt_geometry(0, 100, 64, 64, T.X3 | T.PRE, T.BN_TF, al, 256, at) == _C['STIN_E_UNSUPPORTED']
    assert list(out) == [77] * 10
