"""The routes of the norm kernels, asked of the host-only queries stin_colreduce_route and stin_norm_lane_class (no GPU): every
point of tests/_norm_table.py must reach the route, chunk count, grid and partial size its line names, or the refusal it names, at
256 and at 64 compute units; and over a sweep of shapes no route may write more fp64 partials than the workspace
stin_colreduce_workspace_bytes(C, B) holds.  tests/test_norm_exact_gpu.py runs the routes on the GPU; this file is the check that
its shapes aim where they say, and the statement of the workspace bound."""
import ctypes

import pytest

import _norm_table as T
from surface_texture_inpainting_net_amd import _lib

_C = _lib.CONSTANTS

SWEEP_C = (1, 3, 4, 8, 12, 16, 20, 64, 128, 132, 256, 260, 512, 1024)
SWEEP_B = (1, 2, 255, 256, 257, 511, 512, 513, 1024, 1025, 8192)


def test_constants_of_the_table():
    assert (T.ONE, T.TWO) == (_C['STIN_COLREDUCE_ONE_LAUNCH'], _C['STIN_COLREDUCE_TWO_STAGE'])
    assert (T.E_NULL, T.E_SIZE, T.E_UNSUPPORTED) == (_C['STIN_E_NULL'], _C['STIN_E_SIZE'], _C['STIN_E_UNSUPPORTED'])


@pytest.mark.parametrize('cu', [256, 64])
@pytest.mark.parametrize('p', T.ROUTES, ids=lambda p: p.id)
def test_point_reaches_its_route(p, cu):
    rc, g = T.route(_lib.load(), p.N, p.C, p.B, p.nout, p.vec, p.f32, cu)
    want = p.want[cu]
    if isinstance(want, int):
        assert rc == want, (p.id, rc, g)
        assert set(g.values()) == {-77}, (p.id, g)            # a refusal writes nothing
        return
    assert rc == 0, (p.id, rc)
    family, width, chunks, grid, partial, ncg = want
    assert (g['family'], g['width'], g['chunks'], g['ncg']) == (family, width, chunks, ncg), (p.id, g)
    assert (g['gx'], g['gy'], g['gz']) == grid, (p.id, g)
    assert g['partial'] == partial, (p.id, g)
    assert g['partial'] * 8 + 256 <= _lib.load().stin_colreduce_workspace_bytes(p.C, p.B), (p.id, g)


@pytest.mark.parametrize('p', T.LANES, ids=lambda p: p.id)
def test_lane_class_of_the_elementwise_passes(p):
    assert _lib.load().stin_norm_lane_class(p.C, p.elem, p.data_align, p.stats16, p.ld_align) == p.want, p.id


def test_table_covers_every_route_width_and_refusal():
    ok = [p for p in T.ROUTES if not isinstance(p.want[256], int)]
    assert {(p.want[256][0], p.want[256][1]) for p in ok} == {(T.ONE, 16), (T.ONE, 32), (T.ONE, 64), (T.TWO, 4), (T.TWO, 1)}
    assert {p.want[256] for p in T.ROUTES if isinstance(p.want[256], int)} == {T.E_SIZE, T.E_UNSUPPORTED}
    assert any(p.want[256] != p.want[64] for p in ok)        # the CU cap is reached somewhere
    assert {p.want for p in T.LANES} == {8, 4, 1, T.E_UNSUPPORTED}
    assert {p.nout for p in ok} == {1, 2} and {p.f32 for p in ok} == {0, 1}


def sweep_points():
    """(N, C, B, nout, vec4): the sweep, on the vector route wherever C allows it and on the scalar route for every C"""
    for C in SWEEP_C:
        for B in SWEEP_B:
            for N in sorted({0, 1, B, 100 * B, 10 ** 6}):
                for nout in (1, 2):
                    for vec in ((0, 1) if C % 4 == 0 else (0,)):
                        yield N, C, B, nout, vec


@pytest.mark.parametrize('cu', [256, 64, 8, 1024])
def test_no_route_writes_past_the_workspace(cu):
    """partial doubles * 8 + 256 <= stin_colreduce_workspace_bytes(C, B) at every point of the sweep.  The 256 bytes are what
    rounding the caller's pointer up to 256 may cost.  (Before the route rule was corrected this failed at C = 4, vec4, two outputs,
    B = 257, 511 and 512 with N >= B: the one-launch partial of B x 32 doubles against 8192.)"""
    lib = _lib.load()
    bad, n = [], 0
    for N, C, B, nout, vec in sweep_points():
        rc, g = T.route(lib, N, C, B, nout, vec, 1, cu)
        assert rc == 0, (N, C, B, nout, vec, rc)
        assert g['partial'] > 0 and g['chunks'] >= 1
        n += 1
        if g['partial'] * 8 + 256 > lib.stin_colreduce_workspace_bytes(C, B):
            bad.append((N, C, B, nout, vec, g['family'], g['partial']))
    assert n == (14 + 12) * (10 * 5 + 4) * 2                # 12 of the 14 widths also on the vector route; N = 1 = B once
    assert bad == [], bad


def test_one_launch_grid_and_partial_agree_over_the_sweep():
    """The figures of an answer are consistent with each other: one launch - grid (R, ncg, B), at most 512 ticket words, partial
    = B ncg R nout GC; two stages - grid (nch, B), partial = B nch nout C."""
    lib = _lib.load()
    for N, C, B, nout, vec in sweep_points():
        _, g = T.route(lib, N, C, B, nout, vec, 1, 256)
        if g['family'] == T.ONE:
            assert vec and N > 0 and g['width'] == (64 if C >= 256 else 32 if C >= 128 else 16)
            assert g['ncg'] == -(-C // g['width']) and B * g['ncg'] <= 512
            assert (g['gx'], g['gy'], g['gz']) == (g['chunks'], g['ncg'], B)
            assert g['partial'] == B * g['ncg'] * g['chunks'] * nout * g['width']
        else:
            assert g['family'] == T.TWO and g['width'] == (4 if vec else 1) and g['ncg'] == 0
            assert (g['gx'], g['gy'], g['gz']) == (g['chunks'], B, 1) and g['chunks'] <= max(1, 1024 // B)
            assert g['partial'] == B * g['chunks'] * nout * C


def test_query_argument_errors_and_no_write_on_error():
    lib = _lib.load()
    out = (ctypes.c_int64 * 8)(*([77] * 8))
    at = ctypes.addressof(out)
    assert lib.stin_colreduce_route(100, 16, 1, 1, 1, 1, 256, None) == _C['STIN_E_NULL']
    assert lib.stin_colreduce_route(100, 0, 1, 1, 1, 1, 256, at) == _C['STIN_E_SIZE']
    assert lib.stin_colreduce_route(100, 16, 1, 1, 1, 1, 0, at) == _C['STIN_E_SIZE']                    # cu > 0
    assert lib.stin_colreduce_route(100, 16, 1, 0, 1, 1, 256, at) == _C['STIN_E_SIZE']
    assert lib.stin_colreduce_route(100, 16, 1, 1, 0, 0, 256, at) == _C['STIN_E_UNSUPPORTED']
    assert list(out) == [77] * 8
    assert lib.stin_norm_lane_class(0, 4, 16, 1, 4) == _C['STIN_E_SIZE']
    assert lib.stin_norm_lane_class(16, 3, 16, 1, 4) == _C['STIN_E_SIZE']
    assert lib.stin_norm_lane_class(16, 4, 0, 1, 4) == _C['STIN_E_SIZE']
