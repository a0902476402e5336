"""Generate tests/golden/g15_segmentation*.npz by RUNNING THE REFERENCE'S OWN CODE for the segmentation experiment.

Runs only where the reference tree exists (read-only; nothing is copied from it), through oracle/ref_import.py and the
PyG shim, in the manner of oracle/make_golden.py:g11_scene_reader.  The fixtures hold DATA only:

  g15_segmentation_reader.npz  two synthetic label-graph files (a training crop and a full evaluation scene with a trace to
                               an original mesh) - the saved tensors - and the samples ScanNetLabelDataSet.__getitem__
                               (datasets/scannetlabelgraph_dataloader.py:62-101) assembled from them;
  g15_segmentation_metrics.npz seeded logits [3000, 21] without ties, labels that include class 0, one class that never
                               occurs (a NaN IoU), the trainer's class-weight table, ConfusionMatrixDCM.add applied twice
                               (accumulation) with and without an original_index_traces gather, the IoUDCM.value dicts of the
                               resulting matrices, and the trainer criterion's losses.

    python tests/tools/make_golden_segmentation.py            # rewrites tests/golden/g15_segmentation*.npz
"""
import ast
import importlib
import os
import sys
import tempfile
import warnings

import numpy as np
import torch

_REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, _REPO)
warnings.filterwarnings('ignore')

from oracle import ref_import  # noqa: E402
from surface_texture_inpainting_net_amd.scene_io import label_graph_tensors  # noqa: E402
from surface_texture_inpainting_net_amd.synthetic import make_synthetic_mesh  # noqa: E402

OUT = os.path.join(_REPO, 'tests', 'golden')
NUM_CLASSES = 21
ABSENT_CLASS = 17          # never a label and never predicted: its IoU is 0 / 0 = NaN
MAX_FILE_BYTES = 1 << 20


def _np(t):
    return t.detach().cpu().numpy().copy() if torch.is_tensor(t) else np.asarray(t)


def _label_dataset_module():
    ref_import.load_scannet_color_dataset_module()          # the same stubs (open3d, torchvision, easydict, PyG loaders)
    return importlib.import_module('datasets.scannetlabelgraph_dataloader')


def _class_weights():
    """The literal table of ScanNetGraphDataLoader.__init__ (train_class_weights), read as data from the reference's source."""
    path = os.path.join(ref_import.REFERENCE_ROOT, 'datasets', 'scannetlabelgraph_dataloader.py')
    tree = ast.parse(open(path).read())
    for node in ast.walk(tree):
        if (isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Attribute)
                and node.targets[0].attr == 'train_class_weights' and isinstance(node.value, ast.Call)):
            return np.asarray(ast.literal_eval(node.value.args[0]), dtype=np.float32)
    raise RuntimeError('class-weight table not found')


def _save(name, d):
    path = os.path.join(OUT, name + '.npz')
    np.savez_compressed(path, **d)
    assert os.path.getsize(path) <= MAX_FILE_BYTES, (path, os.path.getsize(path))
    print(name, len(d), 'arrays', os.path.getsize(path), 'bytes')


def g15_reader():
    mod = _label_dataset_module()
    d = {}
    with tempfile.TemporaryDirectory() as root:
        for tag, is_train, n0, seed in (('crop', True, 400, 151), ('full', False, 500, 152)):
            s = make_synthetic_mesh(n0, 4, seed=seed, dilations=())
            rng = np.random.default_rng(seed)
            n = int(s.x.shape[0])
            orig = None
            if is_train:
                labels = rng.integers(0, NUM_CLASSES, size=n)
            else:                                          # an original mesh of 1.6 x the vertices, each mapped to a level-0 vertex
                orig = rng.integers(0, n, size=int(1.6 * n))
                orig[:n] = rng.permutation(n)              # every level-0 vertex is hit
                labels = rng.integers(0, NUM_CLASSES, size=orig.size)
            saved = label_graph_tensors(s, torch.from_numpy(labels), None if orig is None else torch.from_numpy(orig))
            name = 'scene0042_00_3.pt' if is_train else 'scene0042_00.pt'
            torch.save(saved, os.path.join(root, name))
            ds = object.__new__(mod.ScanNetLabelDataSet)   # the index (glob over ScanNet split files) is not under test
            ds._root_dir, ds._end_level, ds._is_train, ds._benchmark = root, 4, is_train, False
            ds._transform = None                           # config_scmnet_segmentation.json: empty transform lists
            ds.index2filenames = np.asarray([name])
            smp = ds[0]
            assert smp.name == name
            for k in smp.keys:
                v = smp[k]
                if torch.is_tensor(v):
                    d['%s.s.%s' % (tag, k)] = _np(v)
            d['%s.s.num_vertices' % tag] = np.asarray(smp.num_vertices, dtype=np.int64)
            d['%s.name' % tag] = np.asarray(name)
            for k in ('vertices', 'edges', 'traces'):
                for i, v in enumerate(saved[k]):
                    d['%s.f.%s.%d' % (tag, k, i)] = _np(v)
            d['%s.f.labels' % tag] = _np(saved['labels'])
    _save('g15_segmentation_reader', d)


def g15_metrics():
    cm_mod = ref_import.load_module('utils.metrics.confusionmatrix_dcm')
    iou_mod = ref_import.load_module('utils.metrics.metrics_dcm')
    w = _class_weights()
    assert w.shape == (NUM_CLASSES,)
    g = torch.Generator().manual_seed(1515)
    d = {'weight': w}

    def logits_labels(n):
        z = torch.randn(n, NUM_CLASSES, generator=g) * 2.0
        z[:, ABSENT_CLASS] -= 100.0                         # never the arg-max
        top2 = z.topk(2, dim=1).values
        assert bool((top2[:, 0] > top2[:, 1]).all())        # no ties
        y = torch.randint(0, NUM_CLASSES - 1, (n,), generator=g)
        y[y >= ABSENT_CLASS] += 1                           # never the absent class
        y[:7] = 0                                           # class 0 (the ignore class) present
        return z, y

    za, ya = logits_labels(3000)
    zb, yb = logits_labels(1100)
    d.update(za=_np(za), ya=_np(ya), zb=_np(zb), yb=_np(yb))
    # evaluation: logits of 1500 level-0 vertices read through an original_index_traces gather of 2600 original vertices
    ze, _ = logits_labels(1500)
    tr = torch.randint(0, 1500, (2600,), generator=g)
    _, ye = logits_labels(2600)
    d.update(ze=_np(ze), tr=_np(tr), ye=_np(ye))

    crit = torch.nn.CrossEntropyLoss(ignore_index=0, weight=torch.from_numpy(w))        # trainers/segmentation_trainer.py:54
    d['loss_a'] = _np(crit(za, ya))
    d['loss_e'] = _np(crit(ze[tr], ye))

    cm = cm_mod.ConfusionMatrixDCM(NUM_CLASSES)
    cm.add(za, ya)
    d['conf_a'] = cm.value(normalized=False).copy()
    cm.add(zb, yb)
    d['conf_ab'] = cm.value(normalized=False).copy()
    ce = cm_mod.ConfusionMatrixDCM(NUM_CLASSES)
    ce.add(ze[tr], ye)                                      # full_prediction = output[data.original_index_traces] (:221-229)
    d['conf_e'] = ce.value(normalized=False).copy()
    for key in ('conf_ab', 'conf_e'):
        for ig_tag, ig in (('ig0', 0), ('none', None)):
            res = iou_mod.IoUDCM(ignore_index=ig).value(d[key].copy())
            for k, v in res.items():
                d['%s.%s.%s' % (key, ig_tag, k)] = np.asarray(v, dtype=np.float64)
    assert np.isnan(d['conf_ab.ig0.iou'][ABSENT_CLASS]) and np.isnan(d['conf_ab.ig0.iou'][0])
    _save('g15_segmentation_metrics', d)


if __name__ == '__main__':
    if not ref_import.available():
        sys.exit('the reference tree is needed to regenerate the g15 fixtures')
    g15_reader()
    g15_metrics()
