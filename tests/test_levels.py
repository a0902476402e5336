"""Graph level generation, CPU part: the numpy restatement tests/_levels_oracle.py against fixture g19 (the outputs of the
reference's own csv2npy, get_color_and_labels, nearest_neighbor_interpolation_for_unassigned_traces and process_frame, see
tests/tools/make_golden_levels.py), bit for bit and including which cases raise; the host-side pieces of the product
(read_trace_csv, remap_scannet_labels, LevelError); and the new C symbols.  The GPU part is tests/test_levels_gpu.py."""
import json
import os
import re

import numpy as np
import pytest

import _levels_oracle as LO
from _golden import load_npz
from surface_texture_inpainting_net_amd import _lib
from surface_texture_inpainting_net_amd import preprocessing as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['stin_nearest_chunks', 'stin_nearest_workspace_bytes', 'stin_nearest_f64', 'stin_trace_workspace_bytes',
               'stin_trace_scatter_i64', 'stin_trace_unassigned_i64', 'stin_trace_check_i64', 'stin_cluster_mean_f32']
N_SCENES = 3


@pytest.fixture(scope='module')
def g():
    return load_npz('g19_levels')


def scene_inputs(g, i):
    """-> (mesh dict, levels, dilated, dists, labels or None, meta) of fixture scene i, numpy arrays (csv as text)."""
    p = 's%d.' % i
    meta = json.loads(bytes(g[p + 'meta']).decode())
    mesh = {k: g[p + 'mesh.' + k] for k in ('vertices', 'faces', 'colors', 'normals')}
    levels = []
    for l, x in enumerate(meta['levels']):
        if x in ('qem', 'ext'):
            lv = {k: g[p + 'lv%d.%s' % (l, k)] for k in ('vertices', 'faces', 'normals')}
            if x == 'qem':
                lv['csv'] = bytes(g[p + 'lv%d.csv' % l]).decode()
            levels.append(lv)
        else:
            levels.append(x)
    labels = g[p + 'labels'].astype(np.int64) if meta['train'] else None
    return mesh, levels, meta['dilated'], meta['dists'], labels, meta


def check_scene(g, i, out, levels, meta, dilated=True):
    """out (numpy / lists) against the reference's file of scene i: keys, dtypes, shapes, values; edges as sorted row sets."""
    p = 's%d.' % i
    assert sorted(out) == sorted(['vertices', 'edges', 'traces', 'dilated_edges', 'dilation_dists'] + (['labels'] if meta['train'] else []))
    assert list(out['dilation_dists']) == meta['dists']
    for k in ('vertices', 'edges', 'traces', 'dilated_edges'):
        assert len(out[k]) == len(levels)
    for l in range(len(levels)):
        v = np.asarray(out['vertices'][l])
        assert v.dtype == np.float32 and v.shape == g[p + 'out.v%d' % l].shape and np.array_equal(v, g[p + 'out.v%d' % l]), l
        assert v.shape[1] == (10 if l == 0 else 3)
        e = np.asarray(out['edges'][l])
        assert e.dtype == np.int64 and np.array_equal(LO.sorted_rows(e), g[p + 'out.e%d' % l]), l
        t = np.asarray(out['traces'][l])
        assert t.dtype == np.int64 and np.array_equal(t, g[p + 'out.t%d' % l]), l
        d = out['dilated_edges'][l]
        assert (d is None) == (int(g[p + 'out.dl%d' % l]) == 0)
        if d is None or not dilated:
            continue
        assert len(d) == len(meta['dists'])
        for j, s in enumerate(d):
            key = p + 'out.d%d.%d' % (l, j)
            if key not in g:
                assert isinstance(s, list) and len(s) == 0
            else:
                s = np.asarray(s)
                assert s.dtype == np.int64 and np.array_equal(s, g[key]), (l, j)
    if meta['train']:
        lab = np.asarray(out['labels'])
        assert lab.dtype == np.int64 and np.array_equal(lab, g[p + 'out.labels'])


def test_restated_nearest_is_the_first_minimum():
    pts = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 2, 0]], dtype=np.float64)
    q = np.array([[0.9, 0, 0], [0.5, 0, 0], [0, 1.9, 0]], dtype=np.float64)
    idx, d2, gap = LO.nearest(q, pts, return_sq_dist=True, return_gap=True)
    assert idx.tolist() == [1, 0, 3] and gap == 0.0
    assert np.array_equal(d2, LO.sq_dist(q, pts)[np.arange(3), idx])
    assert np.array_equal(LO.nearest(q, pts, block=1), idx)


@pytest.mark.parametrize('k', [0, 1])
def test_restated_trace_equals_csv2npy(g, k):
    p = 'csv%d.' % k
    rows = LO.read_trace_csv(g[p + 'text'])
    assert float(g[p + 'gap']) > 0
    assert (np.diff(rows[2]) == 0).any()
    trace = LO.trace_from_rows(rows, g[p + 'old'], g[p + 'new'])
    assert trace.dtype == np.int64 and np.array_equal(trace, g[p + 'trace'])
    named = np.unique(LO.nearest(rows[1], g[p + 'old'])).shape[0]
    assert g[p + 'old'].shape[0] - named >= 0.1 * g[p + 'old'].shape[0]


@pytest.mark.parametrize('case', ['old_twice', 'new_twice', 'new_twice_empty_first', 'uncovered'])
def test_restated_trace_raises_where_the_reference_does(g, case):
    p = 'err.%s.' % case
    rows = LO.read_trace_csv(g[p + 'text'])
    if int(g[p + 'raises']):
        with pytest.raises(LO.LevelError):
            LO.trace_from_rows(rows, g[p + 'old'], g[p + 'new'])
    else:
        assert np.array_equal(LO.trace_from_rows(rows, g[p + 'old'], g[p + 'new']), g[p + 'trace'])
    assert int(g[p + 'raises']) == (0 if case == 'new_twice_empty_first' else 1)


def test_restated_colors_fill_and_labels(g):
    reps = [g['cl.c%d' % i] for i in range(3)]
    for i, o in enumerate(LO.colors_and_labels(g['cl.orig'], reps)):
        assert o.dtype == g['cl.out%d' % i].dtype and np.array_equal(o, g['cl.out%d' % i])
    assert (g['fu.trace_in'] == -1).sum() > 100
    assert np.array_equal(LO.fill_unassigned(g['fu.new'], g['fu.old'], g['fu.trace_in']), g['fu.trace_out'])
    for i in range(N_SCENES):
        if 's%d.labels' % i in g:
            raw = g['s%d.labels_raw' % i]
            assert raw.max() > 40
            assert np.array_equal(LO.remap_scannet_labels(raw), g['s%d.labels' % i])


@pytest.mark.parametrize('i', range(N_SCENES))
def test_restated_scene_equals_process_frame(g, i):
    mesh, levels, dilated, dists, labels, meta = scene_inputs(g, i)
    assert float(g['s%d.gap' % i]) > 0
    out = LO.graph_levels(mesh, levels, dilated, dists, labels=labels, reference_vc_normals=True)
    check_scene(g, i, out, levels, meta)
    if meta['vc']:                                              # the default normals: other dilated sets, nothing else
        other = LO.graph_levels(mesh, levels, dilated, dists, labels=labels)
        check_scene(g, i, other, levels, meta, dilated=False)
        assert any(not np.array_equal(a, b) for da, db in zip(other['dilated_edges'], out['dilated_edges']) if da is not None
                   for a, b in zip(da, db))


def test_fixture_covers_what_the_issue_lists(g):
    metas = [json.loads(bytes(g['s%d.meta' % i]).decode()) for i in range(N_SCENES)]
    assert any(m['train'] and not m['vc'] and len(m['levels']) == 3 and m['dilated'][-1] == 1 for m in metas)
    assert any(not m['train'] for m in metas)
    assert any(m['vc'] and 1 in m['dilated'] for m in metas)
    assert any('100' in m['levels'] for m in metas) and any('qem' in m['levels'] for m in metas) and any('ext' in m['levels'] for m in metas)


def test_read_trace_csv(g, tmp_path):
    text = bytes(g['csv1.text']).decode()
    assert text.endswith('\n') and ';' in text
    want = LO.read_trace_csv(text)
    for name, body in (('a.csv', text), ('b.csv', text.rstrip('\n')), ('c.csv', text.replace('\n', '\r\n') + '\n')):
        path = tmp_path / name
        path.write_bytes(body.encode())
        got = P.read_trace_csv(str(path))
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and np.array_equal(a, b), name
    new_xyz, old_xyz, ptr = got
    assert new_xyz.shape == (400, 3) and ptr.shape == (401,) and ptr[-1] == old_xyz.shape[0]
    zero = np.flatnonzero(np.diff(ptr) == 0)
    assert zero.size >= 1
    lines = text.split('\n')
    assert lines[zero[0]].count(';') == 2 and [float(x) for x in lines[zero[0]].split(';')] == new_xyz[zero[0]].tolist()
    k = int(np.argmax(np.diff(ptr)))
    f = [float(x) for x in lines[k].split(';')]
    assert f[:3] == new_xyz[k].tolist() and f[3:] == old_xyz[ptr[k]:ptr[k + 1]].reshape(-1).tolist()
    # a trailing separator leaves fields short of a triple: ignored, as the reference's len(row) // 3 - 1 does
    path = tmp_path / 'd.csv'
    path.write_text('1;2;3;4;5;6;\n7;8;9\n')
    n, o, q = P.read_trace_csv(str(path))
    assert n.tolist() == [[1, 2, 3], [7, 8, 9]] and o.tolist() == [[4, 5, 6]] and q.tolist() == [0, 1, 1]
    path.write_text('')
    n, o, q = P.read_trace_csv(str(path))
    assert n.shape == (0, 3) and o.shape == (0, 3) and q.tolist() == [0]


def test_remap_scannet_labels():
    import torch
    ids = np.arange(0, 60)
    want = LO.remap_scannet_labels(ids)
    got = P.remap_scannet_labels(ids)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    t = P.remap_scannet_labels(torch.from_numpy(ids).int())
    assert t.dtype == torch.int64 and np.array_equal(t.numpy(), want)
    assert want[[1, 12, 13, 14, 16, 24, 28, 33, 34, 36, 39, 40, 41, 59]].tolist() == [1, 12, 0, 13, 14, 15, 16, 17, 18, 19, 20, 0, 0, 0]
    assert sorted(set(want.tolist())) == list(range(21)) and len(P.SCANNET_CLASS_REMAP) == 41
    assert issubclass(P.LevelError, ValueError)


def test_new_symbols_are_declared_bound_and_exported():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'stin_hip.h')).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.stin_nearest_workspace_bytes(1000, 1) == 0
    assert lib.stin_nearest_workspace_bytes(1000, 4) >= 4 * 1000 * 12
    assert lib.stin_nearest_workspace_bytes(0, 4) == 0
    assert lib.stin_trace_workspace_bytes(100, 10) >= 100 * 4 + 4 * 10 * 4
    assert lib.stin_nearest_chunks(0, 10) == 1 and lib.stin_nearest_chunks(10, 0) == 1


def test_the_kernel_source_keeps_to_vector_stores():
    src = open(os.path.join(ROOT, 'surface_texture_inpainting_net_amd', 'csrc', 'stin_levels.hip')).read().lower()
    assert 'asm' not in src and '__builtin_amdgcn_s_' not in src
    assert 'stin_levels.hip' in open(os.path.join(ROOT, 'surface_texture_inpainting_net_amd', 'csrc', 'Makefile')).read()


def test_cpu_tensors_are_refused():
    import torch
    with pytest.raises(TypeError):
        P.nearest(torch.zeros(3, 3, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.float64))
    with pytest.raises(TypeError):
        P.graph_levels(dict(vertices=torch.zeros(3, 3, dtype=torch.float64), faces=torch.zeros(1, 3, dtype=torch.int64),
                            colors=torch.zeros(3, 3), normals=torch.zeros(3, 3)), [0.1], [0], [2])
