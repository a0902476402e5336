"""Generate tests/golden/g17_crops*.npz by RUNNING THE REFERENCE'S OWN preprocessing/crop_training_samples.py `process_frame`.

Runs only where the reference tree exists (read-only; nothing is copied from it), through oracle/ref_import.py, in the manner of
make_golden_masks.py.  The fixture holds DATA only, one file per scene (g17_crops.npz, g17_crops.part2.npz, ...; tests/_golden.py
`load_npz` merges them), keys `s{i}.*`:

  block, stride, extent          the settings of the run;
  v.{l}, e.{l}, t.{l}, d.{l}.{j} the scene (vertices float32, edges / traces / dilated sets int32; a missing d key = empty list,
                                 dl.{l} = 1 where the level has dilated sets at all), labels (label scenes), dists;
  xs, ys                         get_sampling_positions;
  counters                       the numbers in the names of the files the reference wrote, ascending;
  c{k}.kept.{l}                  scene rows of crop k's vertices (the crop's vertices are v.{l}[kept]), and
  c{k}.e.{l}, c{k}.d.{l}.{j}, c{k}.t.{l}, c{k}.labels   what the reference stored (dilated sets with ITS labelling).

Every array is also compared with tests/_crop_oracle.py (bit-exact), and the coverage the tests rely on is asserted: size-rejected
positions, redirected trace entries, a repair event, a label scene, a crop where the reference's dilated labels differ from the
level's ids, no two vertices of a level at one position, no nearest-neighbour ties, missing vertices visited in ascending order.

    python tests/tools/make_golden_crops.py            # rewrites tests/golden/g17_crops*.npz
"""
import glob
import importlib
import os
import sys
import tempfile
import types
import warnings

import numpy as np
import torch

_REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, _REPO)
sys.path.insert(0, os.path.join(_REPO, 'tests'))
warnings.filterwarnings('ignore')

from oracle import ref_import  # noqa: E402
import _crop_oracle as CO  # noqa: E402

OUT = os.path.join(_REPO, 'tests', 'golden')
MAX_FILE_BYTES = 1 << 20
# (n0, levels, seed, irregular, extent, block, stride, n_labels)
SCENES = [(3000, 3, 1, False, 4.0, 2.0, 1.0, 0),
          (3000, 3, 2, True, 4.0, 2.0, 1.0, 0),
          (6000, 4, 3, True, 5.0, 2.5, 1.0, 0),
          (3000, 3, 1, False, 4.0, 2.0, 1.0, 21)]


def _crop_module():
    ref_import.setup()
    ref_import._stub('open3d')
    ref_import._stub('termcolor', colored=lambda s, *a, **k: s)
    if 'utils' not in sys.modules or not hasattr(sys.modules['utils'], '__path__'):
        m = types.ModuleType('utils')
        m.__path__ = [os.path.join(ref_import.REFERENCE_ROOT, 'utils')]
        sys.modules['utils'] = m
    return importlib.import_module('preprocessing.crop_training_samples')


class _Recorder:
    """Stands in for sklearn's BallTree inside the reference module: same answers, and a record of what the fixture must not
    contain (nearest-neighbour ties) and of the order in which missing vertices are visited."""
    ties = 0
    visits = []

    def __init__(self, X):
        from sklearn.neighbors import BallTree
        self.X = np.array(X)
        self.tree = BallTree(X)

    def query(self, Q, k=1):
        Q = np.asarray(Q)
        if k == 1:
            for i in range(0, Q.shape[0], 512):
                d = CO._d2(Q[i:i + 512], self.X)
                _Recorder.ties += int(((d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
        else:
            _Recorder.visits.append(np.array(Q))
        return self.tree.query(Q, k=k)


def _rows_of(sub, full):
    """Index in `full` ([N, 3], unique rows) of every row of `sub`."""
    key = {r.tobytes(): i for i, r in enumerate(np.ascontiguousarray(full))}
    return np.asarray([key[r.tobytes()] for r in np.ascontiguousarray(sub)], dtype=np.int64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b)


def run_scene(mod, idx, spec, cover):
    n0, levels, seed, irregular, extent, block, stride, n_labels = spec
    saved = CO.synthetic_scene(n0, levels, seed, irregular=irregular, extent=extent, n_labels=n_labels, dilations=(2, 4, 8, 16))
    sc = CO.scene_to_numpy(saved)
    for l, v in enumerate(sc['vertices']):
        assert np.unique(v[:, :3], axis=0).shape[0] == v.shape[0], 'two vertices of level %d share a position' % l
    p = 's%d.' % idx
    d = {p + 'block': np.asarray(block), p + 'stride': np.asarray(stride), p + 'extent': np.asarray(extent),
         p + 'dists': np.asarray(saved['dilation_dists'])}
    for l in range(levels):
        d[p + 'v.%d' % l] = sc['vertices'][l]
        d[p + 'e.%d' % l] = sc['edges'][l].astype(np.int32)
        d[p + 't.%d' % l] = sc['traces'][l].astype(np.int32)
        d[p + 'dl.%d' % l] = np.asarray(0 if sc['dilated_edges'][l] is None else 1)
        for j, s in enumerate(sc['dilated_edges'][l] or []):
            if len(s):
                d[p + 'd.%d.%d' % (l, j)] = s.astype(np.int32)
    if n_labels:
        d[p + 'labels'] = sc['labels'].astype(np.int32)
    _Recorder.ties, _Recorder.visits = 0, []
    mod.BallTree = _Recorder
    cwd = os.getcwd()
    ref = {}
    with tempfile.TemporaryDirectory() as root:
        os.chdir(root)
        try:
            os.makedirs('in')
            os.makedirs('out')
            torch.save(saved, os.path.join('in', 'scene%04d_00.pt' % idx))
            mod.args = types.SimpleNamespace(block_size=block, stride=stride, out_path='out/')
            mod.process_frame(os.path.join('in', 'scene%04d_00.pt' % idx))
            for f in glob.glob('out/*.pt'):
                ref[int(f.rsplit('_', 1)[1][:-3])] = torch.load(f, weights_only=False)
        finally:
            os.chdir(cwd)
    assert _Recorder.ties == 0, 'nearest-neighbour ties in the fixture scene'
    for q in _Recorder.visits:                                  # rows of a level >= 1, in the order the reference visited them
        for v in sc['vertices'][1:]:
            try:
                rows = _rows_of(q[:, :3].astype(v.dtype), v[:, :3])
            except KeyError:
                continue
            assert np.all(np.diff(rows) > 0), 'the reference visited the missing vertices out of order'
            break
        else:
            raise AssertionError('repair query not found in the scene')
    xs, ys = mod.get_sampling_positions(sc['vertices'][0], stride)
    oxs, oys = CO.crop_positions(sc['vertices'][0], stride)
    assert _same(xs, oxs) and _same(ys, oys) and oxs.dtype == np.float64
    d[p + 'xs'], d[p + 'ys'] = np.asarray(xs), np.asarray(ys)
    stats = {}
    mine = CO.crop_scene(saved, block, stride, reference_dilated_labels=True, stats=stats, return_kept=True)
    fixed = CO.crop_scene(saved, block, stride)
    assert [c for c, _, _ in mine] == sorted(ref), ('counters', [c for c, _, _ in mine], sorted(ref))
    d[p + 'counters'] = np.asarray(sorted(ref), dtype=np.int64)
    for k, ((cnt, crop, kept), (_, fcrop)) in enumerate(zip(mine, fixed)):
        r = ref[cnt]
        assert sorted(r) == sorted(crop), (sorted(r), sorted(crop))
        q = p + 'c%d.' % k
        for l in range(levels):
            rv = r['vertices'][l]
            assert rv.dtype == torch.float32 and _same(rv.numpy(), crop['vertices'][l])
            assert _same(_rows_of(rv.numpy()[:, :3], sc['vertices'][l][:, :3]), kept[l])
            d[q + 'kept.%d' % l] = kept[l].astype(np.int32)
            assert r['edges'][l].dtype == torch.int64 and _same(r['edges'][l].numpy(), crop['edges'][l])
            d[q + 'e.%d' % l] = crop['edges'][l].astype(np.int32)
            if r['dilated_edges'][l] is None:
                assert crop['dilated_edges'][l] is None
            else:
                for j, s in enumerate(r['dilated_edges'][l]):
                    mj = crop['dilated_edges'][l][j]
                    if len(s) == 0 and not torch.is_tensor(s):
                        assert len(mj) == 0
                        continue
                    assert s.dtype == torch.int64 and _same(s.numpy().reshape(-1, 2), mj)
                    d[q + 'd.%d.%d' % (l, j)] = np.asarray(mj).astype(np.int32)
                    if not _same(mj, fcrop['dilated_edges'][l][j]):
                        cover['dilated_differs'] += 1
        for l in range(levels - 1):
            assert r['traces'][l].dtype == torch.int64 and _same(r['traces'][l].numpy(), crop['traces'][l])
            d[q + 't.%d' % l] = crop['traces'][l].astype(np.int32)
        if n_labels:
            assert r['labels'].dtype == torch.int64 and _same(r['labels'].numpy(), crop['labels'])
            d[q + 'labels'] = crop['labels'].astype(np.int32)
            cover['label_scenes'] += 1 if k == 0 else 0
        assert r['dilation_dists'] == saved['dilation_dists']
    cover['size'] += stats.get('size', 0)
    cover['redirected'] += stats.get('redirected', 0)
    cover['repairs'] += stats.get('repairs', 0)
    cover['repair_visits'] += len(_Recorder.visits)
    cover['crops'] += len(mine)
    print('scene %d: %d crops, counters %s, %s' % (idx, len(mine), sorted(ref), stats))
    return d


def main():
    mod = _crop_module()
    cover = dict(size=0, redirected=0, repairs=0, repair_visits=0, label_scenes=0, dilated_differs=0, crops=0)
    for f in glob.glob(os.path.join(OUT, 'g17_crops*.npz')):
        os.remove(f)
    for idx, spec in enumerate(SCENES):
        d = run_scene(mod, idx, spec, cover)
        path = os.path.join(OUT, 'g17_crops.npz' if idx == 0 else 'g17_crops.part%d.npz' % (idx + 1))
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) <= MAX_FILE_BYTES, (path, os.path.getsize(path))
        print(os.path.basename(path), len(d), 'arrays', os.path.getsize(path), 'bytes')
    print(cover)
    assert cover['size'] >= 2 and cover['redirected'] >= 100 and cover['repairs'] >= 1 and cover['label_scenes'] >= 1
    assert cover['dilated_differs'] >= 1 and cover['repair_visits'] >= 1


if __name__ == '__main__':
    if not ref_import.available():
        sys.exit('the reference tree is needed to regenerate the g17 fixture')
    main()
