"""CPU-only checks of the host logic: the C-ABI library loads and exports every symbol the header
declares, the ctypes table matches the header, collation rules, synthetic mesh invariants, and the
module surface (state_dict keys / seeded init / parameter counts) against the golden records."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from _golden import GOLDEN, ModelFixture, load_npz
from surface_texture_inpainting_net_amd import _lib
from surface_texture_inpainting_net_amd import surfacetextureinpaintingnet as S
from surface_texture_inpainting_net_amd.data import HierarchicalBatch, collate
from surface_texture_inpainting_net_amd.synthetic import make_synthetic_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'stin_hip.h')


def _header_symbols():
    src = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(stin_[a-z0-9_]+)\s*\(', src)))


def test_library_exports_every_declared_symbol():
    assert os.path.exists(_lib.LIB_PATH), 'build the extension first: python -c "import __graft_entry__ as g; g.build()"'
    lib = ctypes.CDLL(_lib.LIB_PATH)
    syms = _header_symbols()
    assert len(syms) >= 18
    for name in syms:
        assert hasattr(lib, name), 'libstin_hip.so lacks %s' % name
    assert set(syms) == set(_lib.SIGNATURES.keys())


_I, _L, _Z, _U, _F, _D, _P = (ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_float, ctypes.c_double,
                              ctypes.c_void_p)


@pytest.mark.parametrize('name,want', [
    ('stin_csr_workspace_bytes', (_Z, [_L, _L])),                                             # a size_t return
    ('stin_error_string', (ctypes.c_char_p, [_I])),                                           # the const char* return
    ('stin_circle_mask_run', (_I, [_P, _P, _L, _P, _I, _I, _I, _D, _U, _P, _I, _P, _L, _P, _P, _P, _P, _L, _P, _Z, _P])),
    ('stin_adam_f32', (_I, [_P, _P, _P, _P, _P, _L, _D, _D, _D, _D, _D, _I, _I, _P])),        # doubles by value
    ('stin_cols_axpy_rowmask_f32', (_I, [_P, _L, _P, _L, _P, _L, _I, _I, _F, _P])),           # a float by value
    ('stin_net_fwd', (_I, [_I, _P, _I, _P])),                                                 # a struct pointer
    ('stin_dilated_walk_f64', (_I, [_P, _P, _P, _P, _P, _L, _L, _P, _I, _P, _P])),            # the host `dilations` array
])
def test_derived_signatures_match_hand_written_ones(name, want):
    assert _lib.SIGNATURES[name] == want


def test_longest_prototype_is_read_argument_by_argument():
    res, args = _lib.SIGNATURES['stin_edgeconv_wgrad_ti']
    assert res is _I and len(args) == 28 == max(len(a) for _, a in _lib.SIGNATURES.values())
    other = {0: _I, 2: _L, 4: _L, 6: _L, 8: _L, 9: _L, 10: _I, 11: _I, 12: _I, 13: _I, 14: _I, 15: _I, 16: _I, 24: _L, 26: _Z}
    assert args == [other.get(i, _P) for i in range(28)]


def test_a_block_is_reached_through_the_op_record_only():
    """The positional whole-block entry points are gone: a block's operands are the named fields of stin_net_op_t.  The size
    and offset helpers its callers lay their buffers out with stay."""
    assert 'stin_edgeconv_block_fwd' not in _lib.SIGNATURES and 'stin_edgeconv_block_bwd' not in _lib.SIGNATURES
    for name in ('stin_edgeconv_block_fwd_workspace_bytes', 'stin_edgeconv_block_fwd_pack_offsets',
                 'stin_edgeconv_block_bwd_workspace_bytes', 'stin_net_fwd', 'stin_net_bwd'):
        assert name in _lib.SIGNATURES


def test_struct_layouts_have_the_sizes_the_c_side_asserts():
    """The same literals as the static_asserts of csrc/stin_common.h."""
    sizes = {'stin_plan_job_t': 120, 'stin_order_level_t': 32, 'stin_relabel_job_t': 64, 'stin_pack_job_t': 112,
             'stin_net_op_t': 480, 'stin_crop_seg_t': 128}
    assert {k: v.size for k, v in _lib.STRUCTS.items()} == sizes
    common = open(os.path.join(ROOT, 'surface_texture_inpainting_net_amd', 'csrc', 'stin_common.h')).read()
    for name, size in sizes.items():
        assert 'static_assert(sizeof(%s) == %d,' % (name, size) in common
    assert _lib.STRUCTS['stin_net_op_t'].format == '<' + 'i' * 16 + 'f' + 'i' + 'q' * 7 + 'Q' * 2 + 'Q' * 42
    assert _lib.STRUCTS['stin_plan_job_t'].format == '<QQqqqQQQQQQQQQii'
    assert _lib.STRUCTS['stin_crop_seg_t'].format == '<' + 'q' * 8 + 'Q' * 5 + 'q' * 3                # `int64_t reserved[3]`


def test_constants_come_from_the_header():
    c = _lib.CONSTANTS
    assert c['STIN_E_WORKSPACE'] == -4 and c['STIN_E_NULL'] == -1 and c['STIN_OK'] == 0 and c['STIN_VERSION'] == 102
    assert c['STIN_GEMM_W_FRAG'] == 0x400 and c['STIN_BLOCK_PACKED'] == 0x800 and c['STIN_GEMM_F16X3'] == 4
    assert c['STIN_SEG_MAX_CLASSES'] == 128 and c['STIN_CROP_TRACE'] == 4 and c['STIN_PLAN_MAX_JOBS'] == 16
    assert all(k.startswith('STIN_') and isinstance(v, int) for k, v in c.items()) and 'STIN_HIP_H' not in c
    from surface_texture_inpainting_net_amd import functional as F
    assert (F.GEMM_F32, F.GEMM_BF16X3, F.GEMM_BF16X6, F.GEMM_F16X3, F.GEMM_W_PRESPLIT, F.GEMM_W_BF16) == (0, 2, 3, 4, 0x100, 0x200)


_SMALL_HEADER = """/* a header in the style of stin_hip.h; stin_ghost(int) in a comment is no prototype */
#ifndef STIN_HIP_H
#define STIN_HIP_H
#include <stdint.h>
#define STIN_E_SIZE (-2)   /* comment */
#define STIN_FLAG 0x10
typedef void* stin_stream_t;
typedef struct stin_job {
    const float *a, *b;
    int64_t n[2];
    int32_t k, reserved;
} stin_job_t;
size_t stin_bytes(void);
int stin_run(const stin_job_t* jobs, int n_jobs, float eps,
             stin_stream_t stream);
#endif
"""


def test_header_reader_is_strict():
    from surface_texture_inpainting_net_amd import _abi
    sig, structs, consts = _abi.parse_header(_SMALL_HEADER)
    assert sig == {'stin_bytes': (_Z, []), 'stin_run': (_I, [_P, _I, _F, _P])}
    assert structs['stin_job_t'].format == '<QQqqii' and consts == {'STIN_E_SIZE': -2, 'STIN_FLAG': 16}

    def broken(old, new, line):
        assert old in _SMALL_HEADER
        with pytest.raises(_lib.StinLibraryError, match=r':%d: ' % line):
            _abi.parse_header(_SMALL_HEADER.replace(old, new))
    broken('int n_jobs', 'long n_jobs', 14)                                     # a type the reader does not know
    broken('float eps', 'stin_job_t job', 14)                                   # a struct by value
    broken('size_t stin_bytes(void);', 'size_t stin_bytes(void)', 13)           # a prototype without its `;`
    broken('const stin_job_t* jobs', 'const stin_job_t*', 14)                   # a parameter without a name
    broken('int n_jobs', 'int dims[3]', 14)                                     # array parameters: pointers in C
    broken('int n_jobs', 'const int dilations[]', 14)
    broken('stin_stream_t stream)', 'stin_stream_t stream,)', 15)               # an empty parameter
    broken('size_t stin_bytes(void);', 'size_t stin_bytes();', 13)
    broken('stin_run(', 'stin_bytes(', 14)                                      # a second declaration
    broken('size_t stin_bytes(void);', '#ifdef __cplusplus\nint stin_hidden(long x);\n#endif', 14)     # read, not skipped
    broken('#include <stdint.h>', '#ifndef STIN_OTHER', 4)                      # a conditional besides the include guard
    broken('int32_t k, reserved;', 'int32_t k : 8, reserved;', 11)              # a bit-field
    broken('int64_t n[2];', 'int64_t n[2]', 10)                                 # a field without its `;`
    broken('size_t stin_bytes(void);', 'static inline int stin_twice(int x) { return 2 * x; }', 13)
    broken('size_t stin_bytes(void);', 'float* stin_buffer(void);', 13)         # a pointer return other than const char*
    broken('int32_t k, reserved;', 'int32_t k;', 12)                            # the C layout would pad: 28 bytes packed, 32 in C
    broken('#define STIN_FLAG 0x10', '#define STIN_FLAG (1 << 4)', 6)           # not an integer literal
    broken('#include <stdint.h>', '#if 0', 4)                                   # a directive that could hide declarations
    with pytest.raises(_lib.StinLibraryError, match='nope.h'):
        _abi.read_header(os.path.join(ROOT, 'include', 'nope.h'))


def test_records_pack_by_field_name_only():
    import struct
    from surface_texture_inpainting_net_amd import _abi
    job = _abi.parse_header(_SMALL_HEADER)[1]['stin_job_t']
    assert job.fields == ('a', 'b', 'n', 'k', 'reserved') and job.size == 40
    assert job.pack(a=1, n=(2, 3), k=4) == struct.pack('<QQqqii', 1, 0, 2, 3, 4, 0)
    assert job.pack() == bytes(40)
    with pytest.raises(_lib.StinLibraryError, match=r'stin_job_t.*\bm\b'):
        job.pack(a=1, m=2)                                                      # an unknown field: record and field are named
    with pytest.raises(_lib.StinLibraryError, match='stin_job_t'):
        job.pack(n=(2, 3, 4))                                                   # an array field takes exactly its length
    with pytest.raises(_lib.StinLibraryError, match='stin_job_t'):
        job.pack(n=2)
    with pytest.raises(TypeError):
        job.pack(1, 0, 2, 3, 4, 0)                                              # there is no positional pack
    with pytest.raises(_lib.StinLibraryError, match=r':11: '):
        _abi.parse_header(_SMALL_HEADER.replace('int32_t k, reserved;', 'int32_t a, reserved;'))      # a second field `a`


def test_net_op_field_names_sit_where_the_header_puts_them():
    """Positions counted by hand in include/stin_hip.h."""
    import struct
    op = _lib.STRUCTS['stin_net_op_t']
    f = op.fields
    assert len(f) == 69 and f[0] == 'kind' and f[16] == 'eps' and f[18] == 'n_out' and f[27] == 'x' and f[-1] == 'ev_edge1'
    assert f.index('trace') == 57
    row = [0] * 69
    row[0], row[16], row[57] = 2, 0.5, 7
    assert op.pack(kind=2, eps=0.5, trace=7) == struct.pack(op.format, *row)


def test_named_packs_equal_the_positional_argument_lists():
    """A block op, a pool op and a plan job as the call sites name them, against the argument lists the call sites passed by
    POSITION before the records were packed by name (every value distinct).  The one place where positions are written down: a
    reordered header fails here."""
    import struct
    op, job = _lib.STRUCTS['stin_net_op_t'], _lib.STRUCTS['stin_plan_job_t']
    block = (0, 10, 12, 128, 64, 1, 2, 4, 0xC04, 0x402, 3, 1, 1, 0, 0, 0, 1.5e-5, 0,
             5000, 5001, 13, 65, 14, 321, 132, 4096, 8192,
             0x1000, 0x1100, 0x1200,
             0x2000, 0x2100, 0x2200, 0x2300, 0x2400, 0x2500, 0x2600, 0x2700, 0x2800,
             0x3000, 0x3100, 0x3200, 0x3300, 0x3400, 0x3500,
             0x4000, 0x4100, 0x4200, 0x4300, 0x4400,
             0x5000, 0x5100, 0x5200, 0x5300, 0x5400, 0x5500, 0, 0,
             0x6000, 0x6100, 0x6200, 0x6300, 0x6400, 0x6500, 0x6600, 0x6700, 0x6800, 0x6900, 0x6A00)
    assert op.pack(kind=0, Cin=10, Cp=12, H=128, Cout=64, has_shortcut=1, trans_inv=2, prec_fwd=4, fwd_split=0xC04, bwd_split=0x402,
                   B=3, slice_quirk=1, use_side=1, eps=1.5e-5, n_out=5000, n_in=5001, ldx=13, ldo=65, lddx=14, ldy=321, ldh=132,
                   fwd_ws_bytes=4096, bwd_ws_bytes=8192, x=0x1000, out=0x1100, dx=0x1200, W1=0x2000, b1=0x2100, W2=0x2200,
                   b2=0x2300, Ws=0x2400, bs=0x2500, wcatT=0x2600, w2T=0x2700, fwd_ws=0x2800, rowptr_dst=0x3000, col_dst=0x3100,
                   rowptr_src=0x3200, col_src=0x3300, xslot=0x3400, w_src=0x3500, ptr_sum=0x4000, ptr_true=0x4100, gid=0x4200,
                   sid=0x4300, inv_cnt=0x4400, Y=0x5000, hE=0x5100, mask=0x5200, agg=0x5300, mean=0x5400, rstd=0x5500,
                   dW1=0x6000, db1=0x6100, dW2=0x6200, db2=0x6300, dWs=0x6400, dbs=0x6500, bwd_ws=0x6600, ev_dy=0x6700,
                   ev_done=0x6800, ev_edge0=0x6900, ev_edge1=0x6A00) == struct.pack(op.format, *block)
    pool = (1, 256, 256, 0, 256, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0,
            1250, 5000, 257, 258, 259, 0, 0, 0, 0,
            0x1000, 0x1100, 0x1200,
            0, 0, 0, 0, 0, 0, 0, 0, 0,
            0x3000, 0x3100, 0, 0, 0, 0,
            0, 0, 0, 0, 0,
            0, 0, 0, 0, 0, 0,
            0x5600, 0x5700,
            0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    assert op.pack(kind=1, Cin=256, Cp=256, Cout=256, n_out=1250, n_in=5000, ldx=257, ldo=258, lddx=259, x=0x1000, out=0x1100,
                   dx=0x1200, rowptr_dst=0x3000, col_dst=0x3100, arg=0x5600, trace=0x5700) == struct.pack(op.format, *pool)
    plan = (0x100, 0x200, 30000, 5000, 4999, 0x300, 0x400, 0x500, 0x600, 0x700, 0x800, 0x900, 0xA00, 0xB00, 1, 0)
    assert job.pack(a=0x100, b=0x200, E=30000, N=5000, b_limit=4999, rowptr0=0x300, col0=0x400, perm0=0x500, inv_deg0=0x600,
                    rowptr1=0x700, col1=0x800, xslot=0x900, w_src=0xA00, narrow_out=0xB00, pair=1) == struct.pack(job.format, *plan)


def test_the_header_declares_no_chain_entry_point():
    assert not [n for n in list(_lib.SIGNATURES) + list(_lib.STRUCTS) if 'chain' in n]


def test_no_struct_format_is_typed_by_hand():
    """Record layouts come from STRUCTS (the header), never from a format string in the package."""
    pkg = os.path.join(ROOT, 'surface_texture_inpainting_net_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dirpath, f)).read().replace('"', "'")
                for call in ("struct.Struct('<", "struct.pack('<", "struct.unpack('<", "struct.pack_into('<"):
                    assert call not in src, '%s holds a struct format literal' % f


def test_library_host_only_entry_points():
    lib = _lib.load()                       # no GPU needed for these calls
    assert lib.stin_version() == 102
    assert lib.stin_error_string(0) == b'ok'
    assert b'workspace' in lib.stin_error_string(-4)
    assert lib.stin_colreduce_workspace_bytes(64, 1) >= 1024 * 2 * 64 * 8
    assert lib.stin_colreduce_workspace_bytes(0, 1) == 0


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', str(tmp_path / 'nope.so'))
    with pytest.raises(_lib.StinLibraryError):
        _lib.load()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, 'surface_texture_inpainting_net_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dirpath, f)).read()
                assert 'oracle' not in src.replace('# oracle', ''), '%s mentions the oracle' % f


def test_state_dict_layout_and_param_counts():
    rec = json.load(open(os.path.join(GOLDEN, 'param_counts.json')))
    base = dict(output_nc=3, ngf=64, norm='instance', pooling_type='max')
    n = S.define_G(input_nc=10, filter_type='edgeconvtransinv', n_blocks=9, n_levels=2, **base)
    assert sum(p.numel() for p in n.parameters()) == rec['3d_transinv_nl2_nb9'] == 4202051
    assert {k: list(v.shape) for k, v in n.state_dict().items()} == rec['3d_state_dict_keys']
    n1 = S.define_G(input_nc=4, filter_type='edgeconv', n_blocks=9, n_levels=1, **base)
    assert sum(p.numel() for p in n1.parameters()) == rec['c1_edgeconv_nl1_nb9'] == 1050691
    n3 = S.define_G(input_nc=10, filter_type='edgeconvtransinv', n_blocks=9, n_levels=3, **base)
    assert sum(p.numel() for p in n3.parameters()) == rec['3d_transinv_nl3_nb9'] == 16794947
    for m in n.modules():
        if isinstance(m, torch.nn.Linear) and m.bias is not None:
            assert float(m.bias.abs().max()) == 0.0


@pytest.mark.parametrize('name', ['g1_imagegraph_edgeconv', 'g2_3level_transinv_max', 'g5_sageconv', 'g6_graphnorm'])
def test_reference_state_dicts_load(name):
    fx = ModelFixture(name)
    net = S.define_G(**fx.cfg)
    missing, unexpected = net.load_state_dict(fx.state_dict, strict=True)
    assert not missing and not unexpected


def test_error_behaviour_matches_reference():
    with pytest.raises(NotImplementedError):
        S.define_G(input_nc=3, output_nc=3, ngf=8, filter_type='gatconv')
    with pytest.raises(AssertionError):
        S.SurfaceTextureInpaintingNet(3, 3, 'edgeconv', n_blocks=-1)
    net = S.SurfaceTextureInpaintingNet(3, 3, 'edgeconv', ngf=8, pooling_type='median')
    with pytest.raises(ValueError):
        net._pooling(torch.zeros(2, 8), None)
    s = HierarchicalBatch(x=torch.zeros(2, 3))
    with pytest.raises(KeyError):
        s['hierarchy_trace_index_1']
    with pytest.raises(AttributeError):
        s.edge_index


def test_fused_weight_restructure_is_exact_algebra():
    """A_i + B_j must equal W1 [x_i ; x_j - x_i] + b1 (and W1 (x_j - x_i) + b1 for TransInv)."""
    from surface_texture_inpainting_net_amd import modules as M
    torch.manual_seed(3)
    x = torch.randn(50, 6, dtype=torch.float64)
    i, j = torch.randint(0, 50, (200,)), torch.randint(0, 50, (200,))
    for mod, din in ((None, True), (M.EdgeConvTransInv, False)):
        f = M.get_gcn_filter(6, 8, module=mod, double_input=din).double()
        torch.nn.init.normal_(f.nn[0].bias)
        sc = torch.nn.Linear(6, 8).double()
        wcat, bcat, w2e = f.fused_weights(sc)
        Y = x @ wcat.t() + bcat
        H = 16
        feat = (x[j] - x[i]) if mod is not None else torch.cat([x[i], x[j] - x[i]], 1)
        want = feat @ f.nn[0].weight.t() + f.nn[0].bias
        assert torch.allclose(Y[i, :H] + Y[j, H:2 * H], want, atol=1e-12)
        assert torch.allclose(Y[:, 2 * H:], sc(x), atol=1e-12)
        assert torch.equal(w2e[:, :H], f.nn[2].weight) and torch.equal(w2e[:, H], f.nn[2].bias)
        assert float(w2e[:, H + 1:].abs().max()) == 0.0


def test_collate_matches_reference_collation():
    """g3_graphs.npz holds the two single graphs, g3_batch2_unequal.npz the batch the REFERENCE's
    HierarchicalData.__inc__ + PyG collate produced from them."""
    z = load_npz('g3_graphs')
    graphs = []
    for gi in range(2):
        graphs.append(HierarchicalBatch(**{k.split('.', 1)[1]: torch.from_numpy(v) for k, v in z.items()
                                           if k.startswith('g%d.' % gi)}))
    got = collate(graphs)
    want = ModelFixture('g3_batch2_unequal').sample()
    for k in want.keys():
        assert torch.equal(got[k], want[k]), k
    assert got.num_vertices.shape == (2, 3) and got.num_vertices.dtype == torch.int32


def test_collate_dilated_offsets_fixed_vs_reference_quirk():
    a = make_synthetic_mesh(150, 2, seed=1, dilations=(2,))
    b = make_synthetic_mesh(200, 2, seed=2, dilations=(2,))
    key = 'hierarchy_dil_2_edge_index_1'
    fixed = collate([a, b])
    quirk = collate([a, b], fix_dilated_offsets=False)
    n1_a, n0_a = int(a.num_vertices[0, 1]), int(a.num_vertices[0, 0])
    ea = a[key].shape[1]
    assert torch.equal(fixed[key][:, ea:], b[key] + n1_a)          # correct: offset by N_level
    assert torch.equal(quirk[key][:, ea:], b[key] + n0_a)          # reference: offset by N0
    assert int(fixed[key].max()) < int(fixed.num_vertices.sum(0)[1])


def test_synthetic_mesh_invariants():
    s = make_synthetic_mesh(2500, 3, seed=5, dilations=(2, 4))
    nv = s.num_vertices[0].tolist()
    assert nv[0] == 2500 and nv[1] == int(0.3 * nv[0]) and nv[2] == int(0.3 * nv[1])
    ei = s.edge_index
    assert ei.dtype == torch.int64 and int(ei.max()) < nv[0] and bool((ei[0] != ei[1]).all())
    key = ei[0] * nv[0] + ei[1]
    assert torch.equal(key, torch.sort(key).values), 'edges grouped by source, sorted'
    rev = torch.sort(ei[1] * nv[0] + ei[0]).values
    assert torch.equal(rev, key), 'symmetric edge set'
    for lvl in (1, 2):
        tr = s['hierarchy_trace_index_%d' % lvl]
        assert tr.shape[0] == nv[lvl - 1] and int(tr.max()) == nv[lvl] - 1
        assert int(torch.bincount(tr, minlength=nv[lvl]).min()) >= 1
        e = s['hierarchy_edge_index_%d' % lvl]
        assert int(e.max()) < nv[lvl] and bool((e[0] != e[1]).all())
    assert s.x.shape == (2500, 10) and s.mask.shape == (2500, 1) and s.color.shape == (2500, 3)
    assert 0.15 < float((s.mask > 0).float().mean()) < 0.35
    big = make_synthetic_mesh(200_000, 1, seed=0, dilations=())
    assert big.x.shape[0] == 200_704 and big.edge_index.shape[1] == 1_200_642


def test_scene_io_round_trip_in_reference_schema(tmp_path):
    """Write a synthetic scene in the reference's graphs/<scene>.pt + masks/...npz schema and read it back the way
    ScanNetGraphColorDataSet.__getitem__ assembles a sample (feature layout, key names, dilation fall-back)."""
    from surface_texture_inpainting_net_amd.scene_io import load_scene, save_scene_like_reference
    s = make_synthetic_mesh(400, 3, seed=9, dilations=(2, 4))
    gp, mp = str(tmp_path / 'scene0000_00.pt'), str(tmp_path / '0.npz')
    save_scene_like_reference(s, gp, mp, dilation_dists=(2, 4, 8))      # dist 8 is empty -> falls back to dist 4
    t = load_scene(gp, mp, end_level=3)
    assert t['name'] == 'scene0000_00'
    for k in ('edge_index', 'hierarchy_edge_index_1', 'hierarchy_edge_index_2', 'hierarchy_trace_index_1',
              'hierarchy_trace_index_2', 'hierarchy_dil_2_edge_index_2', 'hierarchy_dil_4_edge_index_2', 'mask', 'batch'):
        assert torch.equal(t[k], s[k]), k
    assert torch.equal(t['hierarchy_dil_8_edge_index_2'], s['hierarchy_dil_4_edge_index_2'])
    assert torch.equal(t.num_vertices, s.num_vertices) and t.num_vertices.dtype == torch.int32
    assert torch.allclose(t.color, s.color, atol=1e-6)
    assert torch.allclose(t.x, s.x, atol=1e-6)          # [rgb*known, normal, pos/1.5, known]
    t2 = load_scene(gp, mp, end_level=2)
    assert t2.num_vertices.shape == (1, 2) and 'hierarchy_trace_index_2' not in t2


def test_scene_reader_locality_order_is_a_consistent_renumbering(tmp_path):
    """load_scene(locality_order=True): the same scene with the vertices of every level renumbered (Morton order of the
    positions, first-child order above).  A relabelling must be invisible to the network: the CPU oracle on the renumbered
    sample gives the rows of the original output in the new order (same weights), edge lists keep their order, and the
    numbering is more local than the file's."""
    from oracle import stin_oracle
    from surface_texture_inpainting_net_amd.scene_io import load_scene, save_scene_like_reference
    s = make_synthetic_mesh(900, 3, seed=12, dilations=(2,))
    gp, mp = str(tmp_path / 'scene0001_00.pt'), str(tmp_path / '0.npz')
    save_scene_like_reference(s, gp, mp, dilation_dists=(2,))
    a = load_scene(gp, mp, end_level=3)
    b = load_scene(gp, mp, end_level=3, locality_order=True)
    order = b['vertex_order']
    assert sorted(order.tolist()) == list(range(a.x.shape[0]))
    assert torch.equal(b.x, a.x[order]) and torch.equal(b.color, a.color[order]) and torch.equal(b.mask, a.mask[order])
    rank = torch.empty_like(order)
    rank[order] = torch.arange(order.numel())
    assert torch.equal(b.edge_index, rank[a.edge_index])                       # same edges, same order, new names
    spread = lambda e: float((e[0] - e[1]).abs().float().mean())
    assert spread(b.edge_index) < 0.5 * spread(a.edge_index)
    assert spread(b['hierarchy_edge_index_1']) < 0.6 * spread(a['hierarchy_edge_index_1'])
    cfg = dict(input_nc=10, output_nc=3, ngf=8, filter_type='edgeconvtransinv', norm='instance', n_blocks=2, n_levels=2,
               pooling_type='max', dilations=[1, 2])
    torch.manual_seed(3)
    net = stin_oracle.define_G(**cfg)
    with torch.no_grad():
        ya, yb = net(a), net(b)
    assert float((yb - ya[order]).abs().max()) <= 2e-5


def test_cpu_tensors_are_rejected_not_silently_computed():
    """No CPU / eager fallback: a CPU sample must fail loudly, never produce an answer."""
    s = make_synthetic_mesh(100, 2, seed=3, dilations=())
    net = S.define_G(input_nc=10, output_nc=3, ngf=8, filter_type='edgeconv', norm='instance', n_blocks=1, n_levels=1,
                     pooling_type='max')
    with pytest.raises((AssertionError, TypeError)):
        net(s)


def test_environment_switches_are_the_documented_ones():
    """Round 6 pruned the STIN_* environment switches from 73 to 29: every switch the product reads is in
    that list, and the list names nothing the product no longer reads."""
    import glob
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, 'surface_texture_inpainting_net_amd')
    found = set()
    for path in glob.glob(os.path.join(pkg, 'csrc', '*')):
        if path.endswith(('.hip', '.inc', '.h')):
            found |= set(re.findall(r'getenv\("(STIN_[A-Z0-9_]+)"\)', open(path).read()))
    for path in glob.glob(os.path.join(pkg, '*.py')):
        found |= set(re.findall(r"environ(?:\.get)?[\(\[]\s*'(STIN_[A-Z0-9_]+)'", open(path).read()))
    design = open(os.path.join(root, 'DESIGN.md')).read()
    sec = design[design.index('### 5b. Environment switches'):design.index('## 6. Measurement')]
    documented = set(re.findall(r'`(STIN_[A-Z0-9_]+)`', sec))
    assert found == documented, (sorted(found - documented), sorted(documented - found))
    assert len(found) <= 30
