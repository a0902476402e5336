"""metrics.StepMetrics on the GPU (csrc/stin_metrics.hip, stin_inpaint_metrics_f32): the reference fixture, a full-size scene
against an fp64 evaluation, determinism, no host synchronisation, TrainStep(metrics=...), evaluate and the C entry's argument checks.

Bars: rtol 1e-5 on every column (the bar of the CPU tests against the reference); the PSNR columns additionally atol 1e-4 dB -
fp32 terms, fp64 sums and one final cast leave a relative error of about 4e-7 in the sums, which is about 2e-6 dB."""
import math

import pytest
import torch

from surface_texture_inpainting_net_amd import metrics
from surface_texture_inpainting_net_amd.synthetic import make_synthetic_mesh
from surface_texture_inpainting_net_amd.train_step import TrainStep
from test_step_metrics import CASES, KEYS, assert_row, g18, g18_case

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PSNR_ATOL = 1e-4
CFG = dict(input_nc=10, output_nc=3, ngf=16, filter_type='edgeconvtransinv', norm='instance', n_blocks=2, n_levels=2,
           pooling_type='max', dilations=[1, 1])


def fp64_row(out, color, mask, edge_index, use_weight=True, data_range=2.0):
    """The seven metrics of the trainer evaluated in float64 with torch on the CPU (an independent formulation: scatter-add
    Laplacian, boolean indexing for the masked PSNR)."""
    out, color = out.detach().cpu().double(), color.detach().cpu().double()
    m = mask.detach().cpu().reshape(-1)
    ei = edge_index.detach().cpu()
    P = torch.where((m > 0)[:, None], out, color)
    n, C = P.shape
    d = (P - color).abs()
    w = torch.pow(torch.tensor(0.99, dtype=torch.float64), m.double())[:, None] if use_weight else 1.0
    gray = 0.299 * P[:, 0] + 0.587 * P[:, 1] + 0.114 * P[:, 2]
    agg = torch.zeros(n, dtype=torch.float64).index_add_(0, ei[1], gray[ei[0]])
    deg = torch.zeros(n, dtype=torch.float64).index_add_(0, ei[1], torch.ones(ei.shape[1], dtype=torch.float64))
    lap = agg - deg * gray

    def psnr(a, b):
        return -10 * torch.log10(((a / data_range - b / data_range) ** 2).mean() + 1e-8)
    return torch.stack([(d * w).mean(), d.mean(), (d * d).mean(), (P[ei[0]] - P[ei[1]]).abs().sum() / (n * C),
                        lap.var(unbiased=False), psnr(P, color), psnr(P[m > 0], color[m > 0])])


@pytest.mark.parametrize('layout', [0, 1])
@pytest.mark.parametrize('tag', CASES)
def test_every_fixture_case_on_the_device(tag, layout, monkeypatch):
    monkeypatch.setattr(metrics.StepMetrics, 'LAYOUT', layout)
    z = g18()
    out, s = g18_case(z, tag, DEV)
    t = metrics.StepMetrics(DEV)
    row = t.update(out, s)
    assert row.is_cuda and row.shape == (8,) and len(t) == 1
    assert_row(row[:7].cpu(), z[tag + '.row'], tag, PSNR_ATOL)
    assert float(row[7]) == float((s.mask > 0).sum())
    if tag + '.loss_unweighted' in z:
        plain = metrics.StepMetrics(DEV, use_mask_weighted_loss=False).update(out, s)
        want = z[tag + '.row'].clone()
        want[0] = z[tag + '.loss_unweighted'][0]
        assert_row(plain[:7].cpu(), want, tag, PSNR_ATOL)
    # a loss computed elsewhere is copied; other dtypes are converted; a strided output view is read through its leading dimension
    assert float(t.update(out, s, loss=torch.tensor(0.625, device=DEV))[0]) == 0.625
    assert torch.equal(t.update(out.double(), s)[1:6], row[1:6])
    wide = torch.zeros(out.shape[0], 7, device=DEV)
    wide[:, 2:5] = out
    assert torch.equal(t.update(wide[:, 2:5], s)[:6], row[:6])
    # the same sample with a cached plan takes the plan's edge set
    from surface_texture_inpainting_net_amd.plan import plan_for
    plan_for(s).edges('edge_index', 0)
    assert torch.equal(t.update(out, s)[:6], row[:6])


def test_result_and_growth_on_the_device():
    z = g18()
    t = metrics.StepMetrics(DEV, capacity=2)
    first = None
    for tag in ('A0', 'A1', 'A2', 'B', 'C'):
        row = t.update(*g18_case(z, tag, DEV))
        first = row if first is None else first
        if tag in ('A1', 'A2'):
            res = t.result()
            name = 'D.avg%d' % len(t)
            assert_row(torch.tensor([res[k] for k in KEYS], dtype=torch.float64), z[name], name, PSNR_ATOL)
    rows = t.rows()
    assert rows.shape == (5, 8) and not rows.is_cuda and torch.equal(rows[0], first.cpu())
    for i, tag in enumerate(('A0', 'A1', 'A2', 'B', 'C')):
        assert_row(rows[i, :7], z[tag + '.row'], tag, PSNR_ATOL)
    t.reset()
    assert len(t) == 0


@pytest.fixture(scope='module')
def big():
    from surface_texture_inpainting_net_amd import surfacetextureinpaintingnet as S
    from surface_texture_inpainting_net_amd.loader import SceneLoader
    s = make_synthetic_mesh(200_000, 3, seed=0, dilations=())
    torch.manual_seed(0)
    net = S.define_G(**CFG).to(DEV)
    g = torch.Generator().manual_seed(18)
    out = (torch.rand(s.color.shape[0], 3, generator=g) * 2 - 1).to(DEV)
    want = fp64_row(out, s.color, s.mask, s.edge_index)
    plain = s.to(DEV)
    from surface_texture_inpainting_net_amd.plan import plan_for
    plan_for(plain).edges('edge_index', 0)
    ld = SceneLoader([s], DEV, shuffle=False, model=net)
    list(ld.epoch(0))
    resident = next(iter(ld.epoch(1)))                      # from the graph cache, with its locality-ordered plan
    return out, want, plain, resident


def test_full_size_scene_against_fp64_with_a_plain_and_a_locality_ordered_plan(big, monkeypatch):
    out, want, plain, resident = big
    assert out.shape[0] == 200_704
    assert plain._plan_cache.order0 is None
    resident._plan_cache.edges('edge_index', 0)
    order0 = resident._plan_cache.order0
    assert order0 is not None and not torch.equal(order0.long(), torch.arange(out.shape[0], device=DEV)), \
        'the loader\'s resident plan is locality-ordered'
    got = {}
    for layout in (0, 1):
        monkeypatch.setattr(metrics.StepMetrics, 'LAYOUT', layout)
        for name, s in (('plain', plain), ('resident', resident)):
            t = metrics.StepMetrics(DEV)
            got[name, layout] = t.update(out, s).clone()
            again = t.update(out, s)
            assert torch.equal(again, got[name, layout]), 'two calls on the same inputs give the same bits'
    for name in ('plain', 'resident'):
        assert torch.equal(got[name, 0], got[name, 1]), 'the two kernel layouts give the same bits'
        assert_row(got[name, 1][:7].cpu(), want, name, PSNR_ATOL)
        assert float(got[name, 1][7]) == float((plain.mask > 0).sum())
    # the two plans walk the rows in different orders: same values within the bars
    assert_row(got['resident', 1][:7].cpu(), got['plain', 1][:7].cpu().double(), 'resident-vs-plain', PSNR_ATOL)


def test_update_does_not_synchronise_the_host(big):
    out, _, plain, resident = big
    t = metrics.StepMetrics(DEV, capacity=2)
    for s in (plain, resident):
        t.update(out, s)                                    # (workspace allocation, lazy plan pieces)
    loss = torch.tensor(0.5, device=DEV)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for s in (plain, resident, plain):                  # (crosses a table growth)
            t.update(out, s, loss=loss)
            t.update(out, s)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert len(t) == 8 and bool(torch.isfinite(t.rows()).all())


def test_train_step_with_metrics_is_the_same_step():
    from surface_texture_inpainting_net_amd import surfacetextureinpaintingnet as S
    meshes = [make_synthetic_mesh(3000 + 500 * i, 3, seed=20 + i, dilations=()) for i in range(3)]

    def run(with_metrics):
        torch.manual_seed(5)
        net = S.define_G(**CFG).to(DEV)
        t = metrics.StepMetrics(DEV) if with_metrics else None
        step = TrainStep(net, lr=1e-3, metrics=t) if with_metrics else TrainStep(net, lr=1e-3)
        losses = []
        for i, m in enumerate(meshes):
            losses.append(step(m.to(DEV)))
            assert t is None or len(t) == i + 1
        step.finish()
        return losses, [p.detach().clone() for p in net.parameters()], t

    l0, w0, _ = run(False)
    l1, w1, t = run(True)
    assert all(torch.equal(a, b) for a, b in zip(l0, l1))
    assert all(torch.equal(a, b) for a, b in zip(w0, w1)), 'recording metrics must not change the step'
    rows = t.rows()
    assert rows.shape == (3, 8) and bool(torch.isfinite(rows).all())
    assert [float(v) for v in rows[:, 0]] == [float(v) for v in l1], 'column 0 is the step\'s own loss'
    assert all(float(rows[i, 7]) == float((m.mask > 0).sum()) for i, m in enumerate(meshes))
    net = S.define_G(**CFG).to(DEV)
    with pytest.raises(ValueError):
        TrainStep(net, graph=True, metrics=metrics.StepMetrics(DEV))
    with pytest.raises(ValueError):
        TrainStep(net, loss_fn=lambda m, s: m(s).sum(), metrics=metrics.StepMetrics(DEV))


def test_train_step_rows_equal_the_torch_formulation():
    """The rows TrainStep records are the metrics of the network output of that step."""
    from surface_texture_inpainting_net_amd import surfacetextureinpaintingnet as S
    m = make_synthetic_mesh(3000, 3, seed=31, dilations=())
    torch.manual_seed(6)
    net = S.define_G(**CFG).to(DEV)
    s = m.to(DEV)
    with torch.no_grad():
        out = net(s)
    t = metrics.StepMetrics(DEV)
    TrainStep(net, lr=1e-3, metrics=t)(s)
    assert_row(t.rows()[0, :7], fp64_row(out, s.color, s.mask, s.edge_index), 'train-step', PSNR_ATOL)


def test_evaluate_equals_manual_updates_bit_for_bit():
    from surface_texture_inpainting_net_amd import surfacetextureinpaintingnet as S
    torch.manual_seed(7)
    net = S.define_G(**CFG).to(DEV)
    scenes = [make_synthetic_mesh(3000 + 400 * i, 3, seed=50 + i, dilations=()).to(DEV) for i in range(3)]
    net.train()
    t = metrics.evaluate(net, scenes)
    assert net.training and len(t) == 3
    manual = metrics.StepMetrics(DEV)
    net.eval()
    with torch.no_grad():
        for s in scenes:
            manual.update(net(s), s)
    assert torch.equal(t.rows(), manual.rows())
    assert bool(torch.isfinite(t.rows()).all())


def test_c_entry_rejects_bad_arguments():
    from surface_texture_inpainting_net_amd import _lib
    from surface_texture_inpainting_net_amd.plan import _ptr, _stream
    lib = _lib.load()
    z = g18()
    out, s = g18_case(z, 'A0', DEV)
    n = out.shape[0]
    e = metrics._edges(s.edge_index, n)
    mask = s.mask.reshape(-1).contiguous()
    row = torch.full((8,), -7.0, device=DEV)
    ws_bytes = lib.stin_inpaint_metrics_workspace_bytes(n)
    assert ws_bytes > 0 and lib.stin_inpaint_metrics_workspace_bytes(0) == 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)

    def call(**kw):
        a = dict(out=_ptr(out), ldo=3, color=_ptr(s.color), mask=_ptr(mask), rowptr=_ptr(e.by_dst.rowptr), col=_ptr(e.by_dst.col),
                 perm=0, n=n, c=3, composite=1, use_weight=1, data_range=2.0, loss=0, layout=1, row=_ptr(row), ws=_ptr(ws),
                 ws_bytes=ws_bytes)
        a.update(kw)
        return lib.stin_inpaint_metrics_f32(a['out'], a['ldo'], a['color'], a['mask'], a['rowptr'], a['col'], a['perm'], a['n'], a['c'],
                                            a['composite'], a['use_weight'], a['data_range'], a['loss'], a['layout'], a['row'],
                                            a['ws'], a['ws_bytes'], _stream(out))
    E_NULL, E_SIZE, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -4, -5
    assert call(ws_bytes=ws_bytes - 1) == E_WORKSPACE
    for k in ('out', 'color', 'mask', 'rowptr', 'col', 'row', 'ws'):
        assert call(**{k: 0}) == E_NULL, k
    assert call(c=2) == E_SIZE and call(c=4) == E_SIZE and call(n=0) == E_SIZE and call(n=(1 << 24) + 1) == E_SIZE
    assert call(ldo=2) == E_SIZE and call(data_range=0.0) == E_SIZE
    assert call(layout=2) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((row == -7.0).all()), 'a rejected call enqueues nothing'
    assert call() == 0
    assert_row(row[:7].cpu(), z['A0.row'], 'A0', PSNR_ATOL)


def test_single_channel_on_the_device():
    z = g18()
    out, s = g18_case(z, 'A0', DEV)
    s.color = s.color[:, :1].contiguous()
    row = metrics.StepMetrics(DEV).update(out[:, :1], s)
    cpu_out, cpu_s = g18_case(z, 'A0')
    cpu_s.color = cpu_s.color[:, :1].contiguous()
    want = metrics.StepMetrics('cpu').update(cpu_out[:, :1], cpu_s)
    assert math.isnan(float(row[4])) and math.isnan(float(want[4]))
    cols = [0, 1, 2, 3, 5, 6]
    assert torch.allclose(row[cols].cpu(), want[cols], rtol=1e-5, atol=0) and float(row[7]) == float(want[7])
