"""metrics.StepMetrics / metrics.evaluate / TrainStep(metrics=...) on CPU tensors: the inpainting trainer's seven step metrics
(trainers/inpainting3d_trainer.py:254-271) against tests/golden/g18_inpaint_metrics.npz, which the reference's own
_graph_forward / compute_loss / _update_metrics and MetricTracker produced (tests/tools/make_golden_inpaint_metrics.py).
rtol 1e-5 is the bar test_graph_metrics_against_reference_fixture uses for these quantities against the reference."""
import math

import pytest
import torch

from _golden import load_npz
from oracle import stin_oracle
from surface_texture_inpainting_net_amd import metrics
from surface_texture_inpainting_net_amd.data import HierarchicalBatch
from surface_texture_inpainting_net_amd.synthetic import make_synthetic_mesh
from surface_texture_inpainting_net_amd.train_step import TrainStep

KEYS = ('loss', 'l1', 'mse', 'graph_tv', 'graph_lap_var', 'psnr', 'psnr_mask_only')
CASES = ('A0', 'A1', 'A2', 'B', 'C')
CFG = dict(input_nc=10, output_nc=3, ngf=8, filter_type='edgeconvtransinv', norm='instance', n_blocks=2, n_levels=1,
           pooling_type='max')


def g18():
    return {k: torch.from_numpy(v) if v.dtype.kind in 'fi' else v for k, v in load_npz('g18_inpaint_metrics').items()}


def g18_case(z, tag, device='cpu'):
    """-> (network output, sample) of one recorded step."""
    n = z[tag + '.color'].shape[0]
    s = HierarchicalBatch(x=torch.zeros(n, 10), color=z[tag + '.color'].clone(), mask=z[tag + '.mask'].clone(),
                          edge_index=z[tag + '.ei'].clone(), num_vertices=torch.tensor([n]))
    out = z[tag + '.out'].clone()
    return (out, s) if device == 'cpu' else (out.to(device), s.to(device))


def assert_row(got, want, tag, psnr_atol=0.0):
    """Seven columns against the fixture's row: rtol 1e-5 (the PSNR columns also get psnr_atol dB); equal_nan only where the
    fixture itself is NaN."""
    got, want = got.double().reshape(-1), want.double().reshape(-1)
    for i, k in enumerate(KEYS):
        g, w = float(got[i]), float(want[i])
        print('%s %-15s got %.9g want %.9g' % (tag, k, g, w))
        if math.isnan(w):
            assert (tag, k) in (('A2', 'psnr_mask_only'), ('D.avg3', 'psnr_mask_only')), 'the fixture is NaN only there'
            assert math.isnan(g), (tag, k, g)
        else:
            atol = psnr_atol if k.startswith('psnr') else 0.0
            assert abs(g - w) <= atol + 1e-5 * abs(w), (tag, k, g, w)


def test_keys_are_the_trainers_metric_names_in_order():
    z = g18()
    assert tuple(str(k) for k in z['keys']) == KEYS == metrics.StepMetrics.KEYS


@pytest.mark.parametrize('tag', CASES)
def test_every_fixture_case_on_cpu_tensors(tag):
    z = g18()
    out, s = g18_case(z, tag)
    t = metrics.StepMetrics('cpu')
    row = t.update(out, s)
    assert row.shape == (8,) and row.dtype == torch.float32 and len(t) == 1
    assert_row(row[:7], z[tag + '.row'], tag)
    assert float(row[7]) == float((s.mask > 0).sum())
    # the composite is formed by update(): handing in the composite itself with composite=False is the same step
    pred = torch.where((s.mask > 0).expand_as(s.color), out, s.color)
    same = t.update(pred, s, composite=False)
    cols = [i for i in range(8) if not (tag == 'A2' and i == 6)]
    assert torch.equal(same[cols], row[cols]) and (tag != 'A2' or math.isnan(float(same[6])))
    # a loss computed elsewhere is copied into column 0
    assert float(t.update(out, s, loss=torch.tensor(0.625))[0]) == 0.625
    # use_mask_weighted_loss=False changes the loss column only
    if tag + '.loss_unweighted' in z:
        plain = metrics.StepMetrics('cpu', use_mask_weighted_loss=False).update(out, s)
        want = z[tag + '.row'].clone()
        want[0] = z[tag + '.loss_unweighted'][0]
        assert_row(plain[:7], want, tag)
        if tag != 'A2':
            assert float(plain[0]) > float(row[0])


def test_all_zero_mask_step_is_psnr_80_loss_0_and_nan_mask_only():
    z = g18()
    out, s = g18_case(z, 'A2')
    row = metrics.StepMetrics('cpu').update(out, s)
    assert float(row[0]) == 0.0 and float(row[1]) == 0.0 and float(row[2]) == 0.0
    assert abs(float(row[5]) - 80.0) <= 1e-4 and math.isnan(float(row[6])) and float(row[7]) == 0.0


def test_directed_edges_pin_the_aggregation_side():
    z = g18()
    out, s = g18_case(z, 'C')
    a = metrics.StepMetrics('cpu').update(out, s)
    s.edge_index = s.edge_index.flip(0)
    b = metrics.StepMetrics('cpu').update(out, s)
    assert abs(float(a[3]) - float(b[3])) <= 1e-6 * float(a[3])           # total variation does not see the direction
    assert abs(float(a[4]) - float(b[4])) > 1e-3 * float(a[4])            # the Laplacian does


def test_result_is_the_reference_trackers_average_including_the_nan():
    z = g18()
    t = metrics.StepMetrics('cpu')
    for i, tag in enumerate(('A0', 'A1', 'A2')):
        t.update(*g18_case(z, tag))
        if i >= 1:
            res = t.result()
            assert tuple(res) == KEYS and all(isinstance(v, float) for v in res.values())
            assert_row(torch.tensor([res[k] for k in KEYS], dtype=torch.float64), z['D.avg%d' % (i + 1)], 'D.avg%d' % (i + 1))
    rows = t.rows()
    assert rows.shape == (3, 8) and rows.device.type == 'cpu' and rows.dtype == torch.float32
    for i, tag in enumerate(('A0', 'A1', 'A2')):
        assert_row(rows[i, :7], z[tag + '.row'], tag)


def test_table_grows_past_its_capacity_and_reset_starts_over():
    z = g18()
    t = metrics.StepMetrics('cpu', capacity=2)
    order = ('A0', 'A1', 'B', 'C', 'A0')
    first = t.update(*g18_case(z, order[0]))
    keep = first.clone()
    for tag in order[1:]:
        t.update(*g18_case(z, tag))
    assert len(t) == 5 and t.table.shape[0] >= 5
    rows = t.rows()
    assert rows.shape == (5, 8) and torch.equal(rows[0], keep) and torch.equal(rows[4], keep)
    for i, tag in enumerate(order):
        assert_row(rows[i, :7], z[tag + '.row'], tag)
    t.reset()
    assert len(t) == 0 and t.rows().shape == (0, 8)
    t.update(*g18_case(z, 'B'))
    assert len(t) == 1
    assert_row(t.rows()[0, :7], z['B.row'], 'B')


def test_single_channel_leaves_the_laplace_column_nan():
    z = g18()
    out, s = g18_case(z, 'A0')
    s.color = s.color[:, :1].contiguous()
    row = metrics.StepMetrics('cpu').update(out[:, :1].contiguous(), s)
    assert math.isnan(float(row[4])) and all(math.isfinite(float(row[i])) for i in (0, 1, 2, 3, 5, 6, 7))


def test_evaluate_restores_the_mode_and_records_one_row_per_sample():
    torch.manual_seed(3)
    net = stin_oracle.define_G(**CFG)
    scenes = [make_synthetic_mesh(200 + 30 * i, 2, seed=40 + i, dilations=()) for i in range(3)]
    for mode in (True, False):
        net.train(mode)
        t = metrics.evaluate(net, scenes)
        assert net.training is mode and len(t) == 3
    with torch.no_grad():
        net.eval()
        manual = metrics.StepMetrics('cpu')
        for s in scenes:
            manual.update(net(s), s)
    assert torch.equal(manual.rows(), t.rows())
    # the per-scene losses are the trainer's masked weighted L1
    for i, s in enumerate(scenes):
        want = stin_oracle.compute_loss(stin_oracle.graph_forward(net, s), s.color, s.mask)
        assert abs(float(t.rows()[i, 0]) - float(want)) <= 1e-5 * float(want)
    # an existing tracker is continued; keyword arguments reach a new one
    assert len(metrics.evaluate(net, scenes[:1], tracker=t)) == 4
    assert metrics.evaluate(net, scenes[:1], use_mask_weighted_loss=False).use_mask_weighted_loss is False


@pytest.mark.parametrize('accumulate', [1, 2])
def test_cpu_train_step_records_a_row_per_call_and_leaves_the_step_alone(accumulate):
    scenes = [make_synthetic_mesh(200 + 40 * i, 2, seed=i, dilations=()) for i in range(3)]
    runs = []
    for with_metrics in (False, True):
        torch.manual_seed(5)
        net = stin_oracle.define_G(**CFG)
        t = metrics.StepMetrics('cpu') if with_metrics else None
        step = TrainStep(net, lr=1e-3, amsgrad=True, accumulate=accumulate, metrics=t) if with_metrics else \
            TrainStep(net, lr=1e-3, amsgrad=True, accumulate=accumulate)
        losses = []
        for i, s in enumerate(scenes):
            losses.append(step(s))
            if t is not None:
                assert len(t) == i + 1
                assert float(t.rows()[i, 0]) == float(losses[-1])
        runs.append((losses, [p.detach().clone() for p in net.parameters()], t))
    (l0, p0, _), (l1, p1, t) = runs
    assert all(torch.equal(a, b) for a, b in zip(l0, l1))
    assert all(torch.equal(a, b) for a, b in zip(p0, p1)), 'recording metrics must not change the step'
    assert t.rows().shape == (3, 8) and bool(torch.isfinite(t.rows()).all())


def test_train_step_refuses_metrics_with_a_loss_hook():
    net = stin_oracle.define_G(**CFG)
    with pytest.raises(ValueError):
        TrainStep(net, loss_fn=lambda m, s: m(s).sum(), metrics=metrics.StepMetrics('cpu'))
