"""imagegraph on the GPU (csrc/stin_image.hip): the three kernels against the CPU path bit for bit, every rotation / flip
combination from an unaligned pool, the resident loader, the metrics kernel against fp64 and TrainStep with ImageStepMetrics.

Bars: index tensors and x / color / mask exact (integer work and one fp32 multiply, multiply, subtract per channel without
contraction); metrics rtol 1e-5 of fp64 (fp32 terms, fp64 sums: ~1e-7), the masked count exact, the same bits on a second call."""
import numpy as np
import pytest
import torch

from surface_texture_inpainting_net_amd import imagegraph as IG
from surface_texture_inpainting_net_amd import metrics
from surface_texture_inpainting_net_amd.data import HierarchicalBatch
from surface_texture_inpainting_net_amd.train_step import TrainStep
from test_imagegraph import (batch_of_three, case_ids, fp64_image_row, g20, grids, level_key, metric_case, piq_psnr_fp32,
                             record_of)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CFG = dict(input_nc=4, output_nc=3, ngf=8, filter_type='edgeconv', norm='instance', n_blocks=2, n_levels=1, pooling_type='max')


def random_images(shapes, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, size=hw + (3,)).astype(np.uint8) for hw in shapes]


@pytest.mark.parametrize('B', [1, 2, 3])
@pytest.mark.parametrize('S,L', grids() + [(128, 3)])
def test_grid_levels_kernel_equals_the_cpu_path_in_the_defined_order(S, L, B):
    want = IG.grid_levels(S, L, B, 'cpu')
    got = IG.grid_levels(S, L, B, DEV)
    assert set(got) == set(want)
    for k, v in want.items():
        assert got[k].is_cuda and got[k].dtype == v.dtype and got[k].is_contiguous(), k
        assert torch.equal(got[k].cpu(), v), k


def test_grid_levels_with_a_one_pixel_level():
    want, got = IG.grid_levels(4, 3, 2, 'cpu'), IG.grid_levels(4, 3, 2, DEV)
    assert got['hierarchy_edge_index_2'].shape == (2, 0)
    assert all(torch.equal(got[k].cpu(), v) for k, v in want.items())


@pytest.mark.parametrize('i', range(12), ids=case_ids())
def test_sample_kernel_equals_the_reference_sample(i):
    z, cases = g20()
    c = cases[i]
    pool = torch.from_numpy(z['%d.img' % i].reshape(-1).copy()).to(DEV)
    x, color, mask = IG.build_samples(pool, [record_of(z, c)], c['S'], c['R'])
    assert x.is_cuda and mask.dtype == torch.bool and mask.shape == (c['S'] ** 2, 1)
    assert torch.equal(color.cpu(), torch.from_numpy(z['%d.color' % i]))
    assert torch.equal(mask.cpu(), torch.from_numpy(z['%d.mask' % i]))
    assert torch.equal(x.cpu(), torch.from_numpy(z['%d.x' % i]))


@pytest.mark.parametrize('random_placement', [True, False])
def test_sample_kernel_batched_from_one_pool(random_placement):
    z, cases = g20()
    pool, recs, three = batch_of_three(z, cases, random_placement)
    x, color, mask = IG.build_samples(pool.to(DEV), recs, 16, 2)
    for name, got in (('x', x), ('color', color), ('mask', mask)):
        assert torch.equal(got.cpu(), torch.cat([torch.from_numpy(z['%d.%s' % (c['index'], name)]) for c in three])), name


def test_all_eight_rotation_flip_combinations_from_an_unaligned_pool():
    S, R = 18, 2
    images = random_images([(19, 18), (18, 23), (18, 18)], 8)
    offsets = np.cumsum([0] + [im.size for im in images])
    assert offsets[1] == 1026 and offsets[1] % 4 != 0
    pool = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images]))
    starts = [[(2, 2), (11, 2), (2, 11), (11, 11)], [(0, 0), (14, 14), (7, 7), (8, 6)], [(14, 0), (0, 14), (3, 9), (3, 10)]]
    dev_pool = pool.to(DEV)
    for k in range(4):
        for flip in (False, True):
            recs = [IG.ImageRecord(int(offsets[b]), im.shape[0], im.shape[1], (k + b) % 4, flip ^ (b == 1), starts[b])
                    for b, im in enumerate(images)]
            want = IG.build_samples(pool, recs, S, R)
            got = IG.build_samples(dev_pool, recs, S, R)
            for name, a, b in zip(('x', 'color', 'mask'), got, want):
                assert torch.equal(a.cpu(), b), (name, k, flip)


def test_build_samples_does_not_synchronise_the_host():
    z, cases = g20()
    pool, recs, _ = batch_of_three(z, cases, True)
    pool = pool.to(DEV)
    IG.build_samples(pool, recs, 16, 2)                         # (pinned staging block, code object)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        x, _, _ = IG.build_samples(pool, recs, 16, 2)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert bool(torch.isfinite(x).all())


@pytest.fixture(scope='module')
def loader_kw():
    return dict(img_size=16, end_level=3, batch_size=2, circle_radius=2, crop_half_width=2, random_mask=True,
                random_augmentation=True, seed=11)


@pytest.fixture(scope='module')
def five_images():
    return random_images([(16, 21), (19, 16), (16, 16), (16, 17), (30, 16)], 5)


def test_loader_epochs_ranks_and_reproducibility(five_images, loader_kw):
    ld = IG.ImageGraphLoader(five_images, DEV, **loader_kw)
    cpu = IG.ImageGraphLoader(five_images, 'cpu', **loader_kw)
    epochs = [list(ld.epoch(e)) for e in (0, 1)]
    for e, batches in enumerate(epochs):
        ids = [i for b in ld.batch_ids(e) for i in b]
        assert sorted(ids) == list(range(5)), 'every image once per epoch'
        assert [s.num_graphs for s in batches] == [2, 2, 1]
        for s, t in zip(batches, cpu.epoch(e)):                 # the device batches are the CPU path's batches
            assert all(torch.equal(s[k].cpu(), t[k]) for k in ('x', 'color', 'mask', 'num_vertices', 'batch', 'hierarchy_trace_index_2'))
    again = list(IG.ImageGraphLoader(five_images, DEV, **loader_kw).epoch(0))
    assert all(torch.equal(a.x, b.x) and torch.equal(a.mask, b.mask) for a, b in zip(epochs[0], again)), 'same (seed, epoch)'
    assert not all(torch.equal(a.x, b.x) for a, b in zip(epochs[0], epochs[1])), 'different epochs differ'
    ranks = [IG.ImageGraphLoader(five_images, DEV, rank=r, world_size=2, **loader_kw) for r in (0, 1)]
    ids = [[i for b in r.batch_ids(0) for i in b] for r in ranks]
    assert len(ids[0]) == len(ids[1]) == 3 and set(ids[0]) | set(ids[1]) == set(range(5)), 'two ranks partition the epoch'
    assert len(set(ids[0]) & set(ids[1])) == 1, 'padded by one wrapped item, as DistributedSampler'
    plans = [s._plan_cache for b in epochs for s in b]
    assert all(p is not None for p in plans)
    assert plans[0] is plans[1] is plans[3] is plans[4] and plans[2] is plans[5] and plans[0] is not plans[2], \
        'batches of equal size share one plan object'


def test_model_output_through_the_shared_plan_is_the_output_without_it(five_images, loader_kw):
    from surface_texture_inpainting_net_amd import surfacetextureinpaintingnet as S
    torch.manual_seed(3)
    net = S.define_G(**CFG).to(DEV)
    ld = IG.ImageGraphLoader(five_images, DEV, **loader_kw)
    with torch.no_grad():
        for s in list(ld.epoch(0)) + list(ld.epoch(1))[:1]:     # (the last one re-uses a plan an earlier batch has filled)
            plain = HierarchicalBatch(**{k: s[k].clone() for k in s.keys()})
            assert plain._plan_cache is None
            got, want = net(s), net(plain)
            assert got.shape == (s.x.shape[0], 3) and bool(torch.isfinite(got).all())
            assert torch.equal(got, want)


@pytest.mark.parametrize('composite', [True, False])
def test_metrics_kernel_against_fp64(composite):
    out, s = metric_case(B=3, S=18, seed=4)
    wide = torch.zeros(out.shape[0], 7, device=DEV)
    wide[:, 2:5] = out.to(DEV)
    view = wide[:, 2:5]                                          # leading dimension 7 > 3
    sd = HierarchicalBatch(color=s.color.to(DEV), mask=s.mask.to(DEV), num_vertices=s.num_vertices.to(DEV))
    t = metrics.ImageStepMetrics(DEV)
    row = t.update(view, sd, composite=composite).clone()
    want = fp64_image_row(out, s.color, s.mask, 3, composite)
    print('row', row.tolist(), 'fp64', want.tolist())
    assert torch.allclose(row[:4].cpu().double(), want, rtol=1e-5, atol=0)
    assert abs(float(row[3]) - float(piq_psnr_fp32(out, s.color, s.mask, 3, composite))) <= 1e-4
    assert float(row[4]) == float(s.mask.sum()) and bool((row[5:] == 0).all())
    assert torch.equal(t.update(view, sd, composite=composite), row), 'the same bits on a second call'
    assert torch.equal(t.update(out.to(DEV), sd, composite=composite), row), 'a contiguous output gives the same bits'
    cpu_row = metrics.ImageStepMetrics('cpu').update(out, s, composite=composite)
    assert torch.allclose(row.cpu(), cpu_row, rtol=1e-5, atol=0)
    assert float(t.update(view, sd, loss=torch.tensor(0.625, device=DEV), composite=composite)[0]) == 0.625
    # an image equal to its target contributes exactly 80 dB
    assert float(t.update(sd.color.clone(), sd, composite=False)[3]) == 80.0


def test_metrics_c_entry_rejects_bad_arguments():
    from surface_texture_inpainting_net_amd import _lib
    from surface_texture_inpainting_net_amd.plan import _ptr, _stream
    lib = _lib.load()
    out, s = metric_case(B=3, S=18, seed=4)
    out, color, mask = out.to(DEV), s.color.to(DEV), s.mask.to(DEV).view(torch.uint8)
    n = out.shape[0]
    row = torch.full((8,), -7.0, device=DEV)
    ws_bytes = lib.stin_image_metrics_workspace_bytes(n, 3)
    assert ws_bytes > 0 and lib.stin_image_metrics_workspace_bytes(n, 5) == 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)

    def call(**kw):
        a = dict(out=_ptr(out), ldo=3, color=_ptr(color), mask=_ptr(mask), n=n, b=3, c=3, row=_ptr(row), ws=_ptr(ws), ws_bytes=ws_bytes)
        a.update(kw)
        return lib.stin_image_metrics_f32(a['out'], a['ldo'], a['color'], a['mask'], a['n'], a['b'], a['c'], 1, 2.0, 0, a['row'],
                                          a['ws'], a['ws_bytes'], _stream(out))
    assert call(ws_bytes=ws_bytes - 1) == -4
    assert all(call(**{k: 0}) == -1 for k in ('out', 'color', 'mask', 'row', 'ws'))
    assert call(b=5) == -2 and call(c=5) == -2 and call(ldo=2) == -2 and call(n=0) == -2
    torch.cuda.synchronize()
    assert bool((row == -7.0).all()), 'a rejected call enqueues nothing'
    assert call() == 0 and float(row[4]) == float(s.mask.sum())


def test_train_step_records_image_step_metrics(five_images, loader_kw):
    from surface_texture_inpainting_net_amd import surfacetextureinpaintingnet as S
    torch.manual_seed(9)
    net = S.define_G(**CFG).to(DEV)
    t = metrics.ImageStepMetrics(DEV)
    step = TrainStep(net, lr=1e-3, use_mask_weighted_loss=False, metrics=t)
    ld = IG.ImageGraphLoader(five_images, DEV, **loader_kw)
    losses = [step(s) for s in ld.epoch(0)]
    step.finish()
    rows = t.rows()
    assert rows.shape == (3, 8) and len(t) == 3 and bool(torch.isfinite(rows).all())
    assert all(bool(torch.isfinite(v)) for v in losses)
    assert [float(v) for v in rows[:, 0]] == [float(v) for v in losses], 'column 0 is the step\'s own loss'
    print('loss', rows[:, 0].tolist(), 'l1', rows[:, 1].tolist())
    assert torch.allclose(rows[:, 1], rows[:, 0], rtol=1e-5, atol=0), 'l1 of the composite is the unweighted masked L1 loss'
    assert set(t.result()) == {'loss', 'l1', 'mse', 'psnr'}
