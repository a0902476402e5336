"""Graph level generation on the GPU (csrc/stin_levels.hip through preprocessing.nearest / trace_from_csv / colors_and_labels /
fill_unassigned_trace / graph_levels and scene_io.write_graph_levels): bit-exact (np.array_equal, nothing excluded: index work and
fp64 comparisons in one fixed expression) against what the reference's own functions returned (tests/golden/g19_levels*.npz) and
against the numpy restatement tests/_levels_oracle.py on other inputs."""
import numpy as np
import pytest
import torch

import _levels_oracle as LO
from _golden import load_npz
from surface_texture_inpainting_net_amd import preprocessing as P, scene_io
from test_levels import N_SCENES, check_scene, scene_inputs

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

NET = dict(input_nc=10, output_nc=3, ngf=64, filter_type='edgeconvtransinv', norm='instance', n_blocks=3, n_levels=2,
           pooling_type='max', dilations=[1, 2, 4])


@pytest.fixture(scope='module')
def g():
    return load_npz('g19_levels')


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(out):
    """A graph_levels dict with numpy arrays (empty dilated sets stay empty lists)."""
    def h(x):
        if torch.is_tensor(x):
            return x.cpu().numpy()
        if isinstance(x, list):
            return [h(y) for y in x]
        return x
    return {k: h(v) for k, v in out.items()}


def scene_to_dev(mesh, levels, labels):
    m = {k: dev(v) for k, v in mesh.items()}
    lv = [{k: (LO.read_trace_csv(v) if k == 'csv' else dev(v)) for k, v in x.items()} if isinstance(x, dict) else x for x in levels]
    return m, lv, None if labels is None else dev(labels)


def csv_rows(text):
    return LO.read_trace_csv(text)


def check_nearest(q, p, **kw):
    want, wd = LO.nearest(q, p, return_sq_dist=True)
    got, gd = P.nearest(dev(q), dev(p), return_sq_dist=True, **kw)
    assert got.dtype == torch.int64 and got.shape == (q.shape[0],) and gd.dtype == torch.float64
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(gd.cpu().numpy(), wd)
    assert torch.equal(P.nearest(dev(q), dev(p), **kw), got)
    return got


def test_nearest_on_the_fixture(g):
    for k in (0, 1):
        p = 'csv%d.' % k
        new_xyz, old_xyz, _ = csv_rows(g[p + 'text'])
        check_nearest(new_xyz, g[p + 'new'])
        check_nearest(old_xyz, g[p + 'old'])
        check_nearest(g[p + 'old'], g[p + 'new'])
    for i in range(3):
        check_nearest(g['cl.c%d' % i].astype(np.float64), g['cl.orig'][:, :3])


@pytest.mark.parametrize('nq,npts,seed', [(1024, 512, 0), (1025, 513, 1), (20011, 30029, 2), (1, 7, 3), (4099, 1, 4), (37, 5003, 5),
                                           (300, 70001, 6)])
def test_nearest_against_restatement_on_random_sets(nq, npts, seed):
    """Q and P on and off the tile sizes (1024 queries per workgroup, 512 points per stage), P == 1, and few queries, which the
    host sends down the chunked path (asserted through the library's own choice)."""
    from surface_texture_inpainting_net_amd import _lib
    rng = np.random.default_rng(seed)
    q, p = rng.normal(0, 3, (nq, 3)), rng.normal(0, 3, (npts, 3))
    check_nearest(q, p)
    if nq <= 300 and npts >= 5003:
        assert _lib.load().stin_nearest_chunks(nq, npts) > 1
    for chunks in (1, 2, 7, 64):
        check_nearest(q, p, chunks=chunks)


def test_nearest_ties_empty_and_types():
    rng = np.random.default_rng(9)
    base = rng.normal(0, 1, (700, 3))
    p = np.concatenate([base, base[::-1], base])                      # every point three times: the lowest index must win
    q = np.concatenate([base[rng.permutation(700)[:333]], rng.normal(0, 1, (50, 3))])
    for chunks in (None, 1, 3, 5):
        got = check_nearest(q, p, **({} if chunks is None else dict(chunks=chunks)))
        assert int(got[:333].max()) < 700
    # a grid: exact ties between distinct points
    gx = np.stack(np.meshgrid(np.arange(8.0), np.arange(8.0), np.arange(4.0), indexing='ij'), -1).reshape(-1, 3)
    check_nearest(gx[:-1] + 0.5, gx)
    check_nearest(gx[:-1] + 0.5, gx, chunks=2)
    # Q == 0 is a no-op, also with P == 0
    out = P.nearest(torch.zeros(0, 3, dtype=torch.float64, device=DEV), dev(base))
    assert out.shape == (0,) and out.dtype == torch.int64
    assert P.nearest(torch.zeros(0, 3, dtype=torch.float64, device=DEV), torch.zeros(0, 3, dtype=torch.float64, device=DEV)).shape == (0,)
    with pytest.raises(ValueError):
        P.nearest(dev(base), torch.zeros(0, 3, dtype=torch.float64, device=DEV))
    # float32 is promoted; wider rows: the first three columns count
    q32, p32 = base[:100].astype(np.float32), rng.normal(0, 1, (300, 5)).astype(np.float32)
    got = P.nearest(dev(q32), dev(p32))
    assert np.array_equal(got.cpu().numpy(), LO.nearest(q32.astype(np.float64), p32[:, :3].astype(np.float64)))
    # non-finite input is reported, not trapped; the next call is clean
    bad = base.copy()
    bad[5, 1] = np.nan
    with pytest.raises(ValueError):
        P.nearest(dev(bad), dev(base))
    bad[5, 1] = np.inf
    with pytest.raises(ValueError):
        P.nearest(dev(base), dev(bad))
    check_nearest(base[:10], base)


def test_trace_colors_and_fill_on_the_fixture(g):
    for k in (0, 1):
        p = 'csv%d.' % k
        rows = csv_rows(g[p + 'text'])
        t = P.trace_from_csv(rows, dev(g[p + 'old']), dev(g[p + 'new']))
        assert t.dtype == torch.int64 and t.is_cuda and np.array_equal(t.cpu().numpy(), g[p + 'trace'])
        assert torch.equal(P.trace_from_csv(rows, dev(g[p + 'old']), dev(g[p + 'new'])), t)
    orig = dev(g['cl.orig'])
    outs = P.colors_and_labels(orig, [dev(g['cl.c%d' % i]) for i in range(3)])
    for i, o in enumerate(outs):
        assert o.dtype == torch.float64 and np.array_equal(o.cpu().numpy(), g['cl.out%d' % i])
    t_in = dev(g['fu.trace_in'])
    t = P.fill_unassigned_trace(dev(g['fu.new']), dev(g['fu.old']), t_in)
    assert t.dtype == torch.int64 and np.array_equal(t.cpu().numpy(), g['fu.trace_out'])
    assert np.array_equal(t_in.cpu().numpy(), g['fu.trace_in'])                       # the input is left alone
    full = dev(g['fu.trace_out'])
    assert torch.equal(P.fill_unassigned_trace(dev(g['fu.new']), dev(g['fu.old']), full), full.long())


def test_trace_from_csv_reads_a_file(g, tmp_path):
    path = tmp_path / 'trace.csv'
    path.write_bytes(bytes(g['csv1.text']))
    t = P.trace_from_csv(str(path), dev(g['csv1.old']), dev(g['csv1.new']))
    assert np.array_equal(t.cpu().numpy(), g['csv1.trace'])


def test_level_errors_and_a_clean_call_after_each(g):
    for case in ('old_twice', 'new_twice', 'uncovered'):
        p = 'err.%s.' % case
        assert int(g[p + 'raises']) == 1
        with pytest.raises(P.LevelError):
            P.trace_from_csv(csv_rows(g[p + 'text']), dev(g[p + 'old']), dev(g[p + 'new']))
        p = 'err.new_twice_empty_first.'                                  # tolerated by the reference: must succeed
        t = P.trace_from_csv(csv_rows(g[p + 'text']), dev(g[p + 'old']), dev(g[p + 'new']))
        assert np.array_equal(t.cpu().numpy(), g[p + 'trace'])


@pytest.mark.parametrize('i', range(N_SCENES))
def test_graph_levels_equal_process_frame(g, i):
    mesh, levels, dilated, dists, labels, meta = scene_inputs(g, i)
    m, lv, lab = scene_to_dev(mesh, levels, labels)
    out = P.graph_levels(m, lv, dilated, dists, labels=lab, reference_vc_normals=True)
    assert all(v.is_cuda for v in out['vertices'] + out['edges'] + out['traces'])
    check_scene(g, i, host(out), levels, meta)
    again = host(P.graph_levels(m, lv, dilated, dists, labels=lab, reference_vc_normals=True))
    check_scene(g, i, again, levels, meta)
    for l in range(len(levels)):                                          # two runs: bit-identical, edge order included
        assert np.array_equal(again['edges'][l], host(out)['edges'][l])
        e = host(out)['edges'][l]
        assert np.array_equal(e, LO.sorted_rows(e))                       # sorted by (row 0, row 1)
    if meta['vc']:
        other = host(P.graph_levels(m, lv, dilated, dists, labels=lab))
        check_scene(g, i, other, levels, meta, dilated=False)             # everything but the dilated sets equals the fixture
        want = LO.graph_levels(mesh, levels, dilated, dists, labels=labels)
        differs = 0
        for l, sets in enumerate(other['dilated_edges']):
            for j, s in enumerate(sets or []):
                assert np.array_equal(np.asarray(s), np.asarray(want['dilated_edges'][l][j])), (l, j)
                differs += int(not np.array_equal(np.asarray(s), np.asarray(host(out)['dilated_edges'][l][j])))
        assert differs >= 1


@pytest.mark.parametrize('vc', [True, False])
def test_graph_levels_against_restatement_on_a_larger_mesh(vc):
    mesh = LO.grid_mesh(70, 41, spacing=0.1)
    labels = np.random.default_rng(1).integers(0, 21, mesh['vertices'].shape[0])
    if vc:
        levels = [0.2, 0.4, 0.8]
    else:
        levels = ['100', dict(LO.grid_mesh(35, 42, spacing=0.2)), dict(LO.grid_mesh(17, 43, spacing=0.4))]
        for lv in levels[1:]:
            lv.pop('colors')                                               # externally clustered meshes: nearest-vertex traces
    want = LO.graph_levels(mesh, levels, [0, 0, 1], [2, 4], labels=labels)
    m, lv, lab = scene_to_dev(mesh, levels, labels)
    got = host(P.graph_levels(m, lv, [0, 0, 1], [2, 4], labels=lab))
    for k in ('vertices', 'edges', 'traces'):
        for l in range(3):
            assert got[k][l].dtype == want[k][l].dtype and np.array_equal(got[k][l], want[k][l]), (k, l)
    assert np.array_equal(got['labels'], want['labels']) and got['dilated_edges'][:2] == [None, None]
    for a, b in zip(got['dilated_edges'][2], want['dilated_edges'][2]):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_the_chain_from_mesh_to_network(tmp_path):
    """write_graph_levels -> load_label_scene -> write_crops -> write_circle_masks -> load_scene -> one forward pass."""
    from surface_texture_inpainting_net_amd import surfacetextureinpaintingnet as S
    mesh = LO.grid_mesh(120, 51, spacing=0.05)
    n = mesh['vertices'].shape[0]
    labels = P.remap_scannet_labels(np.random.default_rng(2).integers(0, 45, n))
    path = scene_io.write_graph_levels(str(tmp_path / 'graphs'), 'scene0000_00', mesh, [0.1, 0.2, 0.4], [0, 0, 1], [2, 4],
                                       labels=labels, device=DEV)
    saved = torch.load(path, weights_only=False)
    assert all(not t.is_cuda for t in saved['vertices'] + saved['edges'] + saved['traces']) and saved['vertices'][0].shape[1] == 10
    assert saved['traces'][0].shape == (n,) and saved['labels'].shape == (n,) and saved['dilation_dists'] == [2, 4]
    full = scene_io.load_label_scene(path, end_level=3, is_train=False)
    assert full.x.shape == (saved['vertices'][0].shape[0], 9) and full.original_index_traces.shape == (n,)
    assert full.num_vertices.tolist() == [[v.shape[0] for v in saved['vertices']]]
    crops = scene_io.write_crops(path, str(tmp_path / 'cropped'), 3.0, 1.5, min_coarsest=20, device=DEV)
    assert len(crops) >= 4
    ei = P.edges_from_faces(dev(mesh['faces']), n)
    masks = P.circle_masks(ei, n, radius=6, frac_masked_vertices=0.25, num_masks=2, seed=3)
    mpaths = scene_io.write_circle_masks(crops[0], str(tmp_path / 'masks'), masks)
    assert len(mpaths) >= 1
    s = scene_io.load_scene(crops[0], mpaths[0], end_level=3, cropped=True)
    assert s.x.shape[1] == 10 and int((s.mask > 0).sum()) > 0
    torch.manual_seed(0)
    net = S.define_G(**NET).to(DEV)
    with torch.no_grad():
        out = net(s.to(DEV))
    assert out.shape == (s.x.shape[0], 3) and bool(torch.isfinite(out).all())
