"""The segmentation objective and metrics on the GPU (csrc/stin_seg.hip through segmentation.py): loss and dlogits against
torch in fp64, bit-reproducibility, the confusion matrix exactly against the g15 fixture and np.bincount, deferred label
errors, no host synchronisation, SingleConvMeshNet training steps with the native objective, and label scenes through the
GPU loader (resident cache + locality renumbering)."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _golden import load_npz
from surface_texture_inpainting_net_amd import scene_io, segmentation as seg
from surface_texture_inpainting_net_amd.data import collate
from surface_texture_inpainting_net_amd.synthetic import make_synthetic_mesh

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def metrics():
    return load_npz('g15_segmentation_metrics')


def _problem(N, C, seed, ignore_index):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, C, generator=g) * 2.0 + torch.randn(1, C, generator=g)
    y = torch.randint(0, C, (N,), generator=g)
    y[torch.rand(N, generator=g) < 0.1] = ignore_index
    return z, y


def _ref(z, y, w, ignore_index):
    zz = z.double().requires_grad_()
    loss = F.cross_entropy(zz, y, weight=None if w is None else w.double(), ignore_index=ignore_index)
    loss.backward()
    return loss.detach(), zz.grad


def _native(z, y, w, ignore_index):
    zd = z.to(DEV).requires_grad_()
    loss = seg.cross_entropy(zd, y.to(DEV), None if w is None else w.to(DEV), ignore_index)
    loss.backward()
    return loss.detach().cpu(), zd.grad.cpu()


@pytest.mark.parametrize('N', [1, 63, 64, 65, 4097, 200_000])
@pytest.mark.parametrize('C', [2, 3, 21, 64, 128])
def test_loss_and_grad_match_torch_fp64(metrics, N, C):
    for wi, wkind in enumerate(('none', 'random', 'table')):
        for ignore_index in (-100, 0, 5):
            if wkind == 'table' and C != 21:
                continue
            z, y = _problem(N, C, seed=N * 7 + C * 3 + wi, ignore_index=ignore_index)
            w = {'none': None, 'random': torch.rand(C, generator=torch.Generator().manual_seed(C)) + 0.1,
                 'table': torch.from_numpy(metrics['weight'])}[wkind]
            want, gwant = _ref(z, y, w, ignore_index)
            got, ggot = _native(z, y, w, ignore_index)
            tag = (N, C, wkind, ignore_index)
            if not torch.isfinite(want):                    # every target ignored / zero weight: NaN in both
                assert torch.isnan(got), tag
                continue
            assert abs(float(got) - float(want)) <= 1e-6 * abs(float(want)) + 1e-30, (tag, float(got), float(want))
            scale = float(gwant.abs().max())
            assert float((ggot.double() - gwant).abs().max()) <= 2e-6 * scale + 1e-30, tag
            got2, ggot2 = _native(z, y, w, ignore_index)
            assert torch.equal(got, got2) and torch.equal(ggot, ggot2), tag       # same bits run to run


def test_all_ignored_matches_torch_cpu():
    z = torch.randn(300, 21)
    y = torch.zeros(300, dtype=torch.long)
    w = torch.rand(21)
    zc = z.clone().requires_grad_()
    want = F.cross_entropy(zc, y, weight=w, ignore_index=0)
    want.backward()
    got, g = _native(z, y, w, 0)
    assert torch.isnan(want) and torch.isnan(got)
    assert torch.equal(g, zc.grad) and float(g.abs().max()) == 0.0


def _bincount_conf(z, y, C):
    """ConfusionMatrixDCM.add: first arg-max (a NaN is maximal, the first NaN wins), np.bincount over pred + C * target."""
    zn = z.numpy()
    pred = np.argmax(zn, 1)
    nan = np.isnan(zn)
    pred = np.where(nan.any(1), np.argmax(nan, 1), pred)
    return np.bincount(pred + C * y.numpy(), minlength=C * C).reshape(C, C).astype(np.int64)


def test_confusion_matches_fixture_and_bincount(metrics):
    C = 21
    w = torch.from_numpy(metrics['weight']).to(DEV)
    crit = seg.CrossEntropyLoss(weight=w, ignore_index=0)
    cm = seg.ConfusionMatrix(C, DEV)
    za, ya, zb, yb = (torch.from_numpy(metrics[k]) for k in ('za', 'ya', 'zb', 'yb'))
    loss = crit(za.to(DEV), ya.to(DEV), confusion=cm)               # loss + matrix, one launch
    assert abs(float(loss) - float(metrics['loss_a'])) <= 1e-6 * abs(float(metrics['loss_a']))
    assert np.array_equal(cm.value().numpy(), metrics['conf_a'])
    cm.add(zb.to(DEV), yb.to(DEV))                                  # accumulation
    assert np.array_equal(cm.value().numpy(), metrics['conf_ab'])
    assert np.array_equal(cm.value().numpy(), _bincount_conf(za, ya, C) + _bincount_conf(zb, yb, C))
    # evaluation through original_index_traces: rows, no [N_orig, C] gather
    ze, tr, ye = (torch.from_numpy(metrics[k]) for k in ('ze', 'tr', 'ye'))
    ce = seg.ConfusionMatrix(C, DEV)
    with torch.no_grad():
        le = crit(ze.to(DEV), ye.to(DEV), rows=tr.to(DEV), confusion=ce)
    assert abs(float(le) - float(metrics['loss_e'])) <= 1e-6 * abs(float(metrics['loss_e']))
    assert np.array_equal(ce.value().numpy(), metrics['conf_e'])
    ce2 = seg.ConfusionMatrix(C, DEV).add(ze.to(DEV), ye.to(DEV), rows=tr.to(DEV))
    assert np.array_equal(ce2.value().numpy(), metrics['conf_e'])
    got = seg.scores(ce.value(), 0)
    assert np.isnan(got['iou'][17]) and abs(got['mean_iou'] - float(metrics['conf_e.ig0.mean_iou'])) <= 1e-12
    ce.reset()
    assert int(ce.value().abs().sum()) == 0


@pytest.mark.parametrize('C', [3, 21, 128])
def test_confusion_ties_and_nan_rows(C):
    g = torch.Generator().manual_seed(C)
    N = 5000
    z = torch.randint(-2, 3, (N, C), generator=g).float()          # many ties: the first index wins
    y = torch.randint(0, C, (N,), generator=g)
    nan_rows = torch.randperm(N, generator=g)[:200]
    z[nan_rows, torch.randint(0, C, (200,), generator=g)] = float('nan')
    z[nan_rows[:50], torch.randint(0, C, (50,), generator=g)] = float('nan')     # two NaNs in some rows
    cm = seg.ConfusionMatrix(C, DEV).add(z.to(DEV), y.to(DEV))
    assert np.array_equal(cm.value().numpy(), _bincount_conf(z, y, C))
    ref = torch.zeros(C, C, dtype=torch.int64)
    pred = z.max(1)[1]
    ref.view(-1).index_add_(0, y * C + pred, torch.ones(N, dtype=torch.int64))
    assert torch.equal(cm.value(), ref)                             # torch.max(dim) agrees


def test_ignored_valid_class_is_counted_in_matrix_only():
    z = torch.randn(1000, 5)
    y = torch.randint(0, 5, (1000,))
    cm = seg.ConfusionMatrix(5, DEV)
    loss = seg.cross_entropy(z.to(DEV), y.to(DEV), ignore_index=0, confusion=cm)
    assert abs(float(loss) - float(F.cross_entropy(z.double(), y, ignore_index=0))) <= 1e-6 * float(loss)
    assert np.array_equal(cm.value().numpy(), _bincount_conf(z, y, 5))


def test_out_of_range_labels_raise_deferred():
    C = 21
    crit = seg.CrossEntropyLoss(ignore_index=0)
    z = torch.randn(700, C, device=DEV)
    y = torch.randint(0, C, (700,), device=DEV)
    bad = y.clone()
    bad[123] = C + 4
    bad[500] = -3
    crit(z, bad)                                                   # no fault, no sync: the flag is set on the device
    with pytest.raises(IndexError):
        crit(z, y)                                                 # the next call of the criterion reports it
    good = crit(z, y)                                              # the flag went back clean
    torch.cuda.synchronize()
    crit(z, y)
    assert torch.isfinite(good)
    # the bad rows add nothing: the loss equals torch's over the remaining rows
    keep = torch.ones(700, dtype=torch.bool)
    keep[[123, 500]] = False
    cm = seg.ConfusionMatrix(C, DEV)
    with pytest.raises(IndexError):
        lb = seg.cross_entropy(z, bad, ignore_index=0, confusion=cm)
        cm.value()
    zc, yc = z.cpu()[keep], y.cpu()[keep]
    want = F.cross_entropy(zc.double(), yc, ignore_index=0)
    assert abs(float(lb) - float(want)) <= 1e-6 * float(want)
    assert np.array_equal(cm.matrix.cpu().numpy(), _bincount_conf(zc, yc, C))
    # a matrix-only add flags every target outside [0, C), and a gather index outside the logits
    cm2 = seg.ConfusionMatrix(C, DEV).add(z, torch.full((700,), -100, device=DEV))
    with pytest.raises(IndexError):
        cm2.value()
    rows = torch.arange(700, device=DEV)
    rows[3] = 700
    with torch.no_grad():
        seg.cross_entropy(z, y, rows=rows)
    with pytest.raises(IndexError):
        seg.check_deferred()
    torch.cuda.synchronize()                                       # the device is fine


def test_rows_with_requires_grad_raises_and_bad_shapes():
    z = torch.randn(10, 4, device=DEV, requires_grad=True)
    with pytest.raises(ValueError):
        seg.cross_entropy(z, torch.zeros(12, dtype=torch.long, device=DEV), rows=torch.zeros(12, dtype=torch.long, device=DEV))
    with pytest.raises(ValueError):
        seg.cross_entropy(torch.randn(4, 129, device=DEV), torch.zeros(4, dtype=torch.long, device=DEV))
    with pytest.raises(ValueError):
        seg.cross_entropy(torch.randn(4, 3, device=DEV, dtype=torch.float64), torch.zeros(4, dtype=torch.long, device=DEV))
    with pytest.raises(NotImplementedError):
        seg.CrossEntropyLoss(reduction='none')


def test_loss_and_confusion_make_no_host_sync():
    C = 21
    w = torch.rand(C, device=DEV)
    crit = seg.CrossEntropyLoss(weight=w, ignore_index=0)
    cm = seg.ConfusionMatrix(C, DEV)
    z = torch.randn(50_000, C, device=DEV, requires_grad=True)
    y = torch.randint(0, C, (50_000,), device=DEV)
    tr = torch.randint(0, 50_000, (70_000,), device=DEV)
    ye = torch.randint(0, C, (70_000,), device=DEV)
    crit(z, y, confusion=cm).backward()                            # warm-up (first launches, pinned flag buffer)
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            probe.item()                                           # the mode works on this build
        for _ in range(3):
            crit(z, y, confusion=cm).backward()
            cm.add(z.detach(), y)
            with torch.no_grad():
                crit(z.detach(), ye, rows=tr, confusion=cm)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    cm.value()


def _scmn_sample(n, seed, C, dev=DEV):
    s = make_synthetic_mesh(n, 3, seed=seed, dilations=())
    g = torch.Generator().manual_seed(seed)
    s['labels'] = torch.randint(0, C, (s.x.shape[0],), generator=g)
    return s.to(dev)


def test_train_steps_with_objective_match_aten_cross_entropy(metrics):
    """Three TrainStep steps with Objective(CrossEntropyLoss) + ConfusionMatrix against the same steps with aten weighted cross
    entropy: the first step's gradients to fp32 noise, losses to 1e-5 relative, parameters to 1e-4 of the parameters' scale
    (largest magnitude in the model).  Adam (amsgrad) turns ulp-level gradient differences into +-lr updates of parameters
    whose exact gradient is zero (the Linear biases in front of BatchNorm) and from step 2 on the two runs see slightly
    different weights (measured with the CPU oracle: gradient rel-L2 5e-7 at step 1, 4e-4 at step 2), so lr is kept small
    enough that three such updates stay inside the parameter tolerance."""
    from surface_texture_inpainting_net_amd.singleconvmeshnet import SingleConvMeshNet
    from surface_texture_inpainting_net_amd.train_step import TrainStep
    C = 21
    w = torch.from_numpy(metrics['weight']).to(DEV)
    torch.manual_seed(3)
    net_a = SingleConvMeshNet(10, 2, [32, 64, 64], num_classes=C).to(DEV)
    net_b = copy.deepcopy(net_a)
    p0 = [p.detach().clone() for p in net_a.parameters()]
    cm = seg.ConfusionMatrix(C, DEV)
    lr = 5e-5
    step_a = TrainStep(net_a, lr=lr, loss_fn=seg.Objective(seg.CrossEntropyLoss(w, ignore_index=0), cm))
    step_b = TrainStep(net_b, lr=lr, loss_fn=lambda m, s: F.cross_entropy(m(s), s.labels, weight=w, ignore_index=0))
    for k in range(3):
        s = _scmn_sample(6000, 30 + k, C)
        la = step_a(s)
        lb = step_b(s)
        if k == 0:
            ga, gb = step_a.bucket.flat.double(), step_b.bucket.flat.double()
            assert float((ga - gb).norm() / gb.norm()) <= 1e-5
        assert abs(float(la) - float(lb)) <= 1e-5 * abs(float(lb)), (k, float(la), float(lb))
    scale = max(float(p.detach().abs().max()) for p in net_b.parameters())
    for (n, pa), pb, q in zip(net_a.named_parameters(), net_b.parameters(), p0):
        assert float((pa.detach() - pb.detach()).abs().max()) <= 1e-4 * scale, n
    assert max(float((pa.detach() - q).abs().max()) for pa, q in zip(net_a.parameters(), p0)) >= lr   # the steps did move
    step_a.finish()
    assert int(cm.value().sum()) == 3 * s.x.shape[0]


def _label_crop(i, C=21, n=3000, levels=4, is_train=True):
    s = make_synthetic_mesh(n, levels, seed=70 + i, dilations=())
    rng = np.random.default_rng(i)
    if is_train:
        saved = scene_io.label_graph_tensors(s, torch.from_numpy(rng.integers(0, C, size=s.x.shape[0])))
    else:
        n0 = s.x.shape[0]
        orig = np.concatenate([rng.permutation(n0), rng.integers(0, n0, size=n0 // 2)])
        saved = scene_io.label_graph_tensors(s, torch.from_numpy(rng.integers(0, C, size=orig.size)), torch.from_numpy(orig))
    return saved


def test_experiment_configuration_step_is_finite(metrics):
    """config_scmnet_segmentation.json: feature_number 9, 3 propagation steps, filters [64] * 4, 21 classes, 4 collated crops,
    end_level 4."""
    from surface_texture_inpainting_net_amd.singleconvmeshnet import SingleConvMeshNet
    from surface_texture_inpainting_net_amd.train_step import TrainStep
    torch.manual_seed(49)
    net = SingleConvMeshNet(9, 3, [64] * 4, num_classes=21).to(DEV)
    cm = seg.ConfusionMatrix(21, DEV)
    step = TrainStep(net, lr=1e-3, loss_fn=seg.Objective(seg.CrossEntropyLoss(torch.from_numpy(metrics['weight']), 0), cm))
    batch = collate([scene_io.label_sample_from_tensors(_label_crop(i), 4, True) for i in range(4)]).to(DEV)
    assert batch.num_vertices.shape == (4, 4)
    loss = step(batch)
    step.finish()
    assert torch.isfinite(loss)
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
    assert int(cm.value().sum()) == batch.x.shape[0]
    assert np.isfinite(seg.scores(cm.value(), 0)['overall_accuracy'])


def test_eval_scene_through_gpu_loader_cache_and_renumbering():
    """Evaluation scenes (batch 1) keep original_index_traces and labels unchanged through SceneLoader's resident graph cache,
    also when the loader's plan renumbers the vertices by locality (a model with plan hooks, positions in x[:, 6:9]); and the
    loader takes SingleConvMeshNet (no plan hooks) with its cache on.  The evaluation loss through `rows` equals the loss of
    the materialised gather."""
    from surface_texture_inpainting_net_amd.loader import SceneLoader
    from surface_texture_inpainting_net_amd.plan import GraphPlan
    from surface_texture_inpainting_net_amd.singleconvmeshnet import SingleConvMeshNet
    saved = _label_crop(9, is_train=False)
    cpu = scene_io.label_sample_from_tensors(saved, 4, False)
    item = functools.partial(scene_io.label_sample_from_tensors, saved, 4, False)

    class _Renumbering:                                            # the plan hook of a model whose plan renumbers by locality
        def build_plan(self, sample, inputs_ready=True, after=None, reorder=None):
            plan = GraphPlan(sample, positions=(6, 9), reorder=reorder)
            return plan.prefetch([('edge_index', 0), ('hierarchy_edge_index_1', 1)], [1], inputs_ready=inputs_ready, join=False,
                                 after=after)

    stinet = _Renumbering()
    scmn = SingleConvMeshNet(9, 1, [16, 16, 16, 16], num_classes=21).to(DEV).eval()
    crit = seg.CrossEntropyLoss(ignore_index=0)
    for model in (stinet, scmn):
        loader = SceneLoader([item], DEV, batch_size=1, shuffle=False, model=model)
        assert loader.cache is not None and loader.locality_order
        for epoch in range(3):                                     # miss, then resident hits
            (b,) = list(loader.epoch(epoch))
            assert torch.equal(b.original_index_traces.cpu(), cpu.original_index_traces)
            assert torch.equal(b.labels.cpu(), cpu.labels)
            if model is stinet:
                plan = b._plan_cache
                assert plan is not None and plan.order0 is not None  # the plan did renumber
            else:
                with torch.no_grad():
                    out = model(b)
                    got = crit(out, b.labels, rows=b.original_index_traces)
                    want = F.cross_entropy(out[b.original_index_traces].double(), b.labels, ignore_index=0)
                assert abs(float(got) - float(want)) <= 1e-6 * float(want)
        assert len(loader.cache) == 1 and loader.cache.hits >= 2
