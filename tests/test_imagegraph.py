"""imagegraph (the 2-D image-graph experiment) on CPU tensors against tests/golden/g20_imagegraph.npz, which the reference's own
ImageGraphTextureDataSet and transforms produced (tests/tools/make_golden_imagegraph.py), and metrics.ImageStepMetrics against an
fp64 evaluation of its definitions and piq's literal fp32 PSNR formula.

Bars: index tensors, x / color / mask and the draws are exact.  ImageStepMetrics: rtol 1e-5 of fp64 (fp32 terms summed in double
leave ~1e-7; the bar of test_step_metrics_gpu.py); psnr within 1e-4 dB of piq's fp32 formula (that file's PSNR bar)."""
import json
import random

import numpy as np
import pytest
import torch

from surface_texture_inpainting_net_amd import imagegraph as IG
from surface_texture_inpainting_net_amd import metrics
from surface_texture_inpainting_net_amd.data import HierarchicalBatch, collate
from _golden import load_npz

_Z = {}


def g20():
    if not _Z:
        z = load_npz('g20_imagegraph')
        _Z['z'] = z
        _Z['cases'] = json.loads(bytes(z['cases']).decode())
    return _Z['z'], _Z['cases']


def case_ids():
    return ['%d-%s-%s' % (c['index'], c['tag'], 'random' if c['random_placement'] else 'fixed') for c in g20()[1]]


def grids():
    return sorted({(c['S'], c['L']) for c in g20()[1]})


def level_key(l, kind='edge'):
    if kind == 'edge':
        return 'edge_index' if l == 0 else 'hierarchy_edge_index_%d' % l
    return 'hierarchy_trace_index_%d' % l


def pair_rows(ei):
    """[2, E] -> sorted list of (src, dst)."""
    return sorted(map(tuple, ei.t().tolist()))


def assert_defined_order(ei, s, batch):
    """image-major, source row-major, neighbours up / left / right / down."""
    src, dst = ei[0], ei[1]
    assert ei.shape == (2, batch * 4 * s * (s - 1)) and ei.dtype == torch.int64
    assert bool((src[1:] >= src[:-1]).all()), 'sources non-decreasing'
    rank = {-s: 0, -1: 1, 1: 2, s: 3}
    code = torch.tensor([rank[int(v)] for v in (dst - src)])
    same = src[1:] == src[:-1]
    assert bool((code[1:][same] > code[:-1][same]).all()), 'neighbour order up, left, right, down'
    assert bool((src // (s * s) == dst // (s * s)).all()), 'no edge crosses images'


def record_of(z, c, offset=0):
    j = c['index']
    return IG.ImageRecord(offset, c['h'], c['w'], int(z['%d.k' % j]), bool(z['%d.flip' % j]), [tuple(v) for v in z['%d.starts' % j].tolist()])


def reference_sample(z, c):
    """The reference's single sample as a HierarchicalBatch (its edge order)."""
    j, g = c['index'], 'G%d_%d.' % (c['S'], c['L'])
    s = HierarchicalBatch(x=torch.from_numpy(z['%d.x' % j]), color=torch.from_numpy(z['%d.color' % j]),
                          mask=torch.from_numpy(z['%d.mask' % j]), edge_index=torch.from_numpy(z[g + 'edge0']).t().contiguous(),
                          num_vertices=torch.from_numpy(z[g + 'num_vertices']))
    for l in range(1, c['L']):
        s[level_key(l)] = torch.from_numpy(z[g + 'edge%d' % l]).t().contiguous()
        s[level_key(l, 'trace')] = torch.from_numpy(z[g + 'trace%d' % l])
    return s


@pytest.mark.parametrize('S,L', grids())
def test_grid_levels_equal_the_reference_graph_per_level(S, L):
    z, _ = g20()
    g = 'G%d_%d.' % (S, L)
    got = IG.grid_levels(S, L, 1, 'cpu')
    assert got['num_vertices'].dtype == torch.int32 and torch.equal(got['num_vertices'], torch.from_numpy(z[g + 'num_vertices'])[None])
    assert torch.equal(got['batch'], torch.zeros(S * S, dtype=torch.int64))
    for l in range(L):
        s = S // 2 ** l
        ei = got[level_key(l)]
        assert_defined_order(ei, s, 1)
        assert pair_rows(ei) == sorted(map(tuple, z[g + 'edge%d' % l].tolist()))
        if l > 0:
            assert torch.equal(got[level_key(l, 'trace')], torch.from_numpy(z[g + 'trace%d' % l]))
    assert set(got) == {'num_vertices', 'batch'} | {level_key(l) for l in range(L)} | {level_key(l, 'trace') for l in range(1, L)}


@pytest.mark.parametrize('S,L', grids())
def test_grid_levels_of_two_images_equal_the_collated_reference_samples(S, L):
    z, cases = g20()
    two = [c for c in cases if (c['S'], c['L']) == (S, L)][:2]
    want = collate([reference_sample(z, c) for c in two])
    got = IG.grid_levels(S, L, 2, 'cpu')
    assert torch.equal(got['num_vertices'], want['num_vertices']) and torch.equal(got['batch'], want['batch'])
    for l in range(L):
        assert_defined_order(got[level_key(l)], S // 2 ** l, 2)
        assert pair_rows(got[level_key(l)]) == pair_rows(want[level_key(l)])
        if l > 0:
            assert torch.equal(got[level_key(l, 'trace')], want[level_key(l, 'trace')])


def test_draw_image_params_replays_every_recorded_draw():
    z, cases = g20()
    ks, flips = set(), set()
    for c in cases:
        j = c['index']
        k, flip, starts = IG.draw_image_params(random.Random(c['py_seed']), np.random.RandomState(c['np_seed']), c['S'], c['chw'], c['R'],
                                               4, is_train=c['random_placement'], random_mask=c['random_placement'],
                                               random_augmentation=True)
        assert (k, flip) == (int(z['%d.k' % j]), bool(z['%d.flip' % j])), c
        assert starts == [tuple(v) for v in z['%d.starts' % j].tolist()], c
        ks.add(k)
        flips.add(flip)
    assert ks == {0, 1, 2, 3} and flips == {False, True}, 'the fixture covers every rotation and both flip values'
    # the fixed placement keeps Python's precedence and floor division: S = 18 gives -5 and +4
    assert IG.draw_image_params(random.Random(0), np.random.RandomState(0), 18, 3, 2, 4)[2] == [(2, 2), (11, 2), (2, 11), (11, 11)]
    # without augmentation nothing is drawn for the transforms
    r = random.Random(5)
    assert IG.draw_image_params(r, None, 16, 2, 2, 4, True, True, False)[:2] == (0, False)


@pytest.mark.parametrize('i', range(12), ids=case_ids())
def test_build_samples_equals_the_reference_sample(i):
    z, cases = g20()
    c = cases[i]
    pool = torch.from_numpy(z['%d.img' % i].reshape(-1).copy())
    x, color, mask = IG.build_samples(pool, [record_of(z, c)], c['S'], c['R'])
    assert x.dtype == torch.float32 and color.dtype == torch.float32 and mask.dtype == torch.bool
    assert x.shape == (c['S'] ** 2, 4) and color.shape == (c['S'] ** 2, 3) and mask.shape == (c['S'] ** 2, 1)
    assert torch.equal(color, torch.from_numpy(z['%d.color' % i]))
    assert torch.equal(mask, torch.from_numpy(z['%d.mask' % i]))
    assert torch.equal(x, torch.from_numpy(z['%d.x' % i]))             # (the sign of a zero is not pinned: torch.equal)


def batch_of_three(z, cases, random_placement):
    """The D0..D2 items (16x21, 19x16, 16x16) in one pool behind 5 bytes of padding -> pool, records, the cases."""
    three = [c for c in cases if c['tag'].startswith('D') and c['random_placement'] == random_placement]
    assert [(c['h'], c['w']) for c in three] == [(16, 21), (19, 16), (16, 16)]
    parts, recs, at = [np.zeros(5, dtype=np.uint8)], [], 5
    for c in three:
        recs.append(record_of(z, c, at))
        parts.append(z['%d.img' % c['index']].reshape(-1))
        at += parts[-1].size
    return torch.from_numpy(np.concatenate(parts)), recs, three


@pytest.mark.parametrize('random_placement', [True, False])
def test_build_samples_batched_from_one_pool(random_placement):
    z, cases = g20()
    pool, recs, three = batch_of_three(z, cases, random_placement)
    x, color, mask = IG.build_samples(pool, recs, 16, 2)
    for name, got in (('x', x), ('color', color), ('mask', mask)):
        assert torch.equal(got, torch.cat([torch.from_numpy(z['%d.%s' % (c['index'], name)]) for c in three])), name


def test_errors():
    img = np.zeros((16, 21, 3), dtype=np.uint8)
    pool = torch.from_numpy(img.reshape(-1))
    ok = [(2, 2), (10, 2), (2, 10), (10, 10)]
    IG.build_samples(pool, [IG.ImageRecord(0, 16, 21, 0, False, ok)], 16, 2)
    for bad in ((-1, 2), (2, -1), (13, 2), (2, 13)):                             # a window outside the image
        with pytest.raises(ValueError):
            IG.build_samples(pool, [IG.ImageRecord(0, 16, 21, 0, False, ok[:3] + [bad])], 16, 2)
    with pytest.raises(ValueError):                                              # min(h, w) != S: Rescale is out of scope
        IG.build_samples(pool, [IG.ImageRecord(0, 16, 21, 0, False, ok)], 15, 2)
    with pytest.raises(ValueError):                                              # an image outside the pool
        IG.build_samples(pool, [IG.ImageRecord(1, 16, 21, 0, False, ok)], 16, 2)
    with pytest.raises(ValueError):
        IG.grid_levels(18, 3, 1, 'cpu')                                          # 18 is not divisible by 4
    with pytest.raises(ValueError):
        IG.grid_levels(16, 6, 1, 'cpu')                                          # 16 is not divisible by 32
    with pytest.raises(ValueError):
        IG.ImageGraphLoader([img], 'cpu', 18, 2, 1, 2, 3)                        # the loader checks min(h, w) at upload
    with pytest.raises(ValueError):
        IG.ImageGraphLoader([img], 'cpu', 16, 6, 1, 2, 2)


def test_loader_on_the_cpu_path():
    """The loader's host logic without a device: coverage, rank partition, reproducibility, keys."""
    rng = np.random.RandomState(3)
    images = [rng.randint(0, 256, size=hw + (3,)).astype(np.uint8) for hw in ((16, 21), (19, 16), (16, 16), (16, 17), (30, 16))]
    kw = dict(img_size=16, end_level=3, batch_size=2, circle_radius=2, crop_half_width=2, random_mask=True, random_augmentation=True, seed=7)
    ld = IG.ImageGraphLoader(images, 'cpu', **kw)
    assert len(ld) == 5 and ld.steps_per_epoch() == 3
    for e in (0, 1):
        assert sorted(i for ids in ld.batch_ids(e) for i in ids) == list(range(5))
    a, b = list(ld.epoch(0)), list(IG.ImageGraphLoader(images, 'cpu', **kw).epoch(0))
    assert [s.x.shape[0] for s in a] == [512, 512, 256]
    assert all(torch.equal(s.x, t.x) and torch.equal(s.mask, t.mask) for s, t in zip(a, b))
    assert not all(torch.equal(s.x, t.x) for s, t in zip(a, ld.epoch(1)))
    ranks = [IG.ImageGraphLoader(images, 'cpu', rank=r, world_size=2, **kw) for r in (0, 1)]
    ids = [[i for b in ld.batch_ids(0) for i in b] for ld in ranks]
    assert len(ids[0]) == len(ids[1]) == 3 and set(ids[0]) | set(ids[1]) == set(range(5))
    # an item's parameters do not depend on the batch it lands in
    one = IG.ImageGraphLoader(images, 'cpu', **dict(kw, batch_size=1))
    assert one.params_for(0, 3) == ld.params_for(0, 3) and one.params_for(0, 3) != one.params_for(1, 3)
    s = a[0]
    assert set(s.keys()) == {'x', 'color', 'mask', 'edge_index', 'hierarchy_edge_index_1', 'hierarchy_edge_index_2',
                             'hierarchy_trace_index_1', 'hierarchy_trace_index_2', 'num_vertices', 'batch'}
    assert s.num_graphs == 2 and s.mask.dtype == torch.bool and int(s.mask.sum()) > 0


# ------------------------------------------------------------------------------------------------------------------ metrics
def fp64_image_row(out, color, mask, B, composite, data_range=2.0):
    out, color = out.double(), color.double()
    P = torch.where(mask.reshape(-1, 1), out, color) if composite else out
    d = P - color
    mse_b = (d * d).reshape(B, -1).mean(dim=1)
    return torch.stack([d.abs().mean(), d.abs().mean(), (d * d).mean(), (-10 * torch.log10(mse_b / data_range ** 2 + 1e-8)).mean()])


def piq_psnr_fp32(out, color, mask, B, composite):
    """piq.psnr(output + 1, color + 1, data_range=2), literally, in fp32: x / data_range, mean over each image, mean over the batch."""
    P = torch.where(mask.reshape(-1, 1), out, color) if composite else out
    x, y = ((P + 1) / 2).reshape(B, -1), ((color + 1) / 2).reshape(B, -1)
    return (-10 * torch.log10(torch.mean((x - y) ** 2, dim=1) + 1e-8)).mean()


def metric_case(B=3, S=18, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = B * S * S
    out = torch.rand(n, 3, generator=g) * 2 - 1
    color = torch.rand(n, 3, generator=g) * 2 - 1
    mask = torch.rand(n, 1, generator=g) < 0.3
    s = HierarchicalBatch(color=color, mask=mask, num_vertices=torch.tensor([[S * S, S * S // 4]] * B, dtype=torch.int32))
    return out, s


@pytest.mark.parametrize('composite', [True, False])
def test_image_step_metrics_against_fp64_and_piq(composite):
    out, s = metric_case()
    t = metrics.ImageStepMetrics('cpu')
    assert t.KEYS == ('loss', 'l1', 'mse', 'psnr')
    row = t.update(out, s, composite=composite)
    want = fp64_image_row(out, s.color, s.mask, 3, composite)
    print('row', row.tolist(), 'fp64', want.tolist())
    assert torch.allclose(row[:4].double(), want, rtol=1e-5, atol=0)
    assert abs(float(row[3]) - float(piq_psnr_fp32(out, s.color, s.mask, 3, composite))) <= 1e-4
    assert float(row[4]) == float(s.mask.sum()) and bool((row[5:] == 0).all())
    assert float(t.update(out, s, loss=torch.tensor(0.625), composite=composite)[0]) == 0.625
    assert len(t) == 2 and t.rows().shape == (2, 8)
    res = t.result()
    assert set(res) == set(t.KEYS) and abs(res['psnr'] - float(row[3])) < 1e-6


def test_an_image_equal_to_its_target_contributes_exactly_80_db():
    out, s = metric_case(B=2)
    n = out.shape[0] // 2
    t = metrics.ImageStepMetrics('cpu')
    assert float(t.update(s.color.clone(), s, composite=False)[3]) == 80.0
    out[:n] = s.color[:n]                                              # image 0 exact, image 1 random
    row = t.update(out, s, composite=False)
    other = -10 * torch.log10(((out[n:] - s.color[n:]).double() ** 2).mean() / 4 + 1e-8)
    assert abs(float(row[3]) - (80.0 + float(other)) / 2) <= 1e-5 * (80.0 + float(other)) / 2
    # with the composite an empty mask leaves nothing to differ
    s.mask = torch.zeros_like(s.mask)
    row = t.update(out, s)
    assert float(row[3]) == 80.0 and float(row[1]) == 0.0 and float(row[4]) == 0.0
