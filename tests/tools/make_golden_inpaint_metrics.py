"""Generate tests/golden/g18_inpaint_metrics.npz by RUNNING THE REFERENCE'S OWN CODE for the inpainting trainer's step metrics.

Runs only where the reference tree exists (read-only; nothing is copied from it), through oracle/ref_import.py and the PyG
shim, in the manner of tests/tools/make_golden_segmentation.py.  The trainer's unbound methods Inpainting3DTrainer._graph_forward,
compute_loss and _update_metrics (trainers/inpainting3d_trainer.py:127-137, :254-271) run on a stub `self` that carries exactly
what they read (l1_metric, l2_metric, laplace_var_metric, criterion, a model that returns the recorded network output and a
recording _update_batch_epoch_metric); the averages come from the reference's utils.util.MetricTracker.  The fixture holds DATA only:

  A0 A1 A2  three single-scene steps on 400-vertex synthetic meshes, random network output in [-1, 1], the mesh's own multi-valued
            mask (values up to 16: the 0.99^mask weights matter); A2 has an all-zero mask (psnr_mask_only NaN, psnr 80, loss 0)
  B         one batch of two unequal scenes through data.collate
  C         a directed, asymmetric random edge list (total variation does not see the direction, the Laplacian does)
  D.avg2 / D.avg3   MetricTracker.result() after A0, A1 and after A0, A1, A2 (NaN in psnr_mask_only)
  <case>.out / .color / .mask / .ei = the step's inputs, .row = the seven values _update_metrics handed to the tracker (float64,
  the trainer's order), .loss_unweighted = the loss with use_mask_weighted_loss = False (the other six do not depend on it).

    python tests/tools/make_golden_inpaint_metrics.py          # rewrites tests/golden/g18_inpaint_metrics.npz
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

_REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, _REPO)
warnings.filterwarnings('ignore')

from oracle import ref_import  # noqa: E402
from surface_texture_inpainting_net_amd.data import collate  # noqa: E402
from surface_texture_inpainting_net_amd.synthetic import make_synthetic_mesh  # noqa: E402

OUT = os.path.join(_REPO, 'tests', 'golden')
KEYS = ('loss', 'l1', 'mse', 'graph_tv', 'graph_lap_var', 'psnr', 'psnr_mask_only')
MAX_FILE_BYTES = 1 << 20


def _np(t):
    return t.detach().cpu().numpy().copy()


class _Stub:
    """`self` of the trainer's methods: what they read, nothing else."""

    def __init__(self, trainer_mod, tracker):
        gm = ref_import.load_module('utils.metrics.graph_metrics')
        self.l1_metric = torch.nn.L1Loss()
        self.l2_metric = torch.nn.MSELoss()
        self.laplace_var_metric = gm.GraphLaplaceVariance()
        self.criterion = torch.nn.L1Loss(reduction='none')
        self.models = {}
        self.tracker = tracker
        self.recorded = {}
        self.T = trainer_mod.Inpainting3DTrainer

    def _update_batch_epoch_metric(self, name, score, type, write=True):
        self.recorded[name] = float(score)
        if self.tracker is not None:
            self.tracker.update(name, float(score), write=False)

    def step(self, out, data, use_weight):
        """One validation step of the trainer (:229-235) with `out` as the network's output -> the seven recorded values."""
        self.models['graph'] = lambda d: out.clone()
        self.recorded = {}
        with torch.no_grad():
            pred = self.T._graph_forward(self, data, data.color)
            loss = self.T.compute_loss(self, pred, data.color, weights=data.mask if use_weight else None).item()
            self.T._update_metrics(self, pred, data.color, data.mask, data.edge_index, loss, 'valid')
        return np.asarray([self.recorded[k] for k in KEYS], dtype=np.float64)


def main():
    trainer_mod = ref_import.load_trainer3d_module()
    util = ref_import.load_module('utils.util')
    g = torch.Generator().manual_seed(1818)
    d = {'keys': np.asarray(KEYS)}

    def scene(n0, seed):
        s = make_synthetic_mesh(n0, 1, seed=seed, dilations=())
        assert int(s.mask.max()) > 8                            # multi-valued: the weights matter
        return s

    def record(tag, data, stub, weighted_only=False):
        n = int(data.color.shape[0])
        out = torch.rand(n, 3, generator=g) * 2 - 1
        row = stub.step(out, data, True)
        d[tag + '.out'], d[tag + '.color'] = _np(out), _np(data.color)
        d[tag + '.mask'], d[tag + '.ei'] = _np(data.mask), _np(data.edge_index)
        d[tag + '.row'] = row
        if not weighted_only:
            plain = _Stub(trainer_mod, None).step(out, data, False)
            assert np.array_equal(plain[1:], row[1:], equal_nan=True)
            d[tag + '.loss_unweighted'] = plain[:1]
        return row

    tracker = util.MetricTracker(*KEYS)
    stub = _Stub(trainer_mod, tracker)
    a = [scene(400, 181), scene(400, 182), scene(400, 183)]
    a[2].mask = torch.zeros_like(a[2].mask)
    for i, s in enumerate(a):
        row = record('A%d' % i, s, stub)
        if i >= 1:
            res = tracker.result()
            d['D.avg%d' % (i + 1)] = np.asarray([float(res[k]) for k in KEYS], dtype=np.float64)
    assert np.isnan(row[6]) and row[0] == 0.0 and abs(row[5] - 80.0) < 1e-4, row
    assert np.isnan(d['D.avg3'][6]) and not np.isnan(d['D.avg2']).any()

    record('B', collate([scene(400, 184), scene(250, 185)]), _Stub(trainer_mod, None))

    c = scene(400, 186)
    n = int(c.color.shape[0])
    c.edge_index = torch.randint(0, n, (2, 5 * n), generator=g)
    rc = record('C', c, _Stub(trainer_mod, None))
    flipped = types.SimpleNamespace(color=c.color, mask=c.mask, edge_index=c.edge_index.flip(0))
    rf = _Stub(trainer_mod, None).step(torch.from_numpy(d['C.out']), flipped, True)
    assert rf[3] == rc[3] and abs(rf[4] - rc[4]) > 1e-3 * abs(rc[4]), (rf, rc)      # the case does pin the aggregation side

    path = os.path.join(OUT, 'g18_inpaint_metrics.npz')
    np.savez_compressed(path, **d)
    assert os.path.getsize(path) <= MAX_FILE_BYTES, os.path.getsize(path)
    print('g18_inpaint_metrics', len(d), 'arrays', os.path.getsize(path), 'bytes')
    for k in sorted(d):
        if k.endswith('.row') or k.startswith('D.'):
            print(k, d[k])


if __name__ == '__main__':
    if not ref_import.available():
        sys.exit('the reference tree is needed to regenerate the g18 fixture')
    main()
