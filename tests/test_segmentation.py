"""The segmentation experiment on the CPU: the label-graph reader against the reference's own dataset (g15 fixtures),
label scenes through loader.SceneLoader, scores() against IoUDCM, the CPU path of the objective / confusion matrix, and the
matrix's all_reduce over two gloo ranks."""
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from _golden import load_npz
from surface_texture_inpainting_net_amd import scene_io, segmentation as seg
from surface_texture_inpainting_net_amd.data import collate
from surface_texture_inpainting_net_amd.synthetic import make_synthetic_mesh

K = 21
SCORE_KEYS = ('iou', 'mean_iou', 'precision_per_class', 'mean_precision', 'overall_precision', 'overall_accuracy')


@pytest.fixture(scope='module')
def reader():
    return load_npz('g15_segmentation_reader')


@pytest.fixture(scope='module')
def metrics():
    return load_npz('g15_segmentation_metrics')


def _saved(z, tag):
    out = {}
    for k in ('vertices', 'edges', 'traces'):
        n = len([f for f in z if f.startswith('%s.f.%s.' % (tag, k))])
        out[k] = [torch.from_numpy(z['%s.f.%s.%d' % (tag, k, i)]) for i in range(n)]
    out['labels'] = torch.from_numpy(z['%s.f.labels' % tag])
    return out


@pytest.mark.parametrize('tag,is_train', [('crop', True), ('full', False)])
def test_label_reader_matches_reference_dataset(reader, tmp_path, tag, is_train):
    """ScanNetLabelDataSet.__getitem__ (datasets/scannetlabelgraph_dataloader.py:62-101) for both trace conventions."""
    name = str(reader['%s.name' % tag])
    path = tmp_path / name
    torch.save(_saved(reader, tag), path)
    s = scene_io.load_label_scene(str(path), end_level=4, is_train=is_train)
    assert s.name == name
    want = {k[len(tag) + 3:]: v for k, v in reader.items() if k.startswith(tag + '.s.')}
    for k, v in want.items():
        got = s[k]
        if k == 'num_vertices':
            assert got.dtype == torch.int32 and got.shape == (1, 4)
            assert got.reshape(-1).tolist() == v.tolist()
            continue
        assert got.dtype == torch.from_numpy(v).dtype, k
        assert torch.equal(got, torch.from_numpy(v)), k
    extra = set(s.keys()) - set(want) - {'name', 'batch'}
    assert not extra, extra
    assert ('original_index_traces' in s) == (not is_train)
    assert s.x.shape[1] == 9 and torch.equal(s.batch, torch.zeros(s.x.shape[0], dtype=torch.long))


def _crop_items(tmp_path, n=4):
    items, samples = [], []
    for i in range(n):
        s = make_synthetic_mesh(150 + 40 * i, 4, seed=40 + i, dilations=())
        labels = torch.from_numpy(np.random.default_rng(i).integers(0, K, size=s.x.shape[0]))
        p = tmp_path / ('scene%04d_00_%d.pt' % (i, i))
        torch.save(scene_io.label_graph_tensors(s, labels), p)
        items.append(functools.partial(scene_io.load_label_scene, str(p), 4, True))
        samples.append(scene_io.load_label_scene(str(p), 4, True))
    return items, samples


def test_label_crops_collate_through_scene_loader(tmp_path):
    """4 training crops per step (train_batch_size 4): labels concatenated and NOT incremented (HierarchicalData.__inc__
    returns 0 for labels), traces / edges offset by the level sizes."""
    from surface_texture_inpainting_net_amd.loader import SceneLoader
    items, samples = _crop_items(tmp_path)
    loader = SceneLoader(items, 'cpu', batch_size=4, shuffle=False, cache_bytes=0)
    batches = list(loader.epoch(0))
    assert len(batches) == 1
    b = batches[0]
    assert torch.equal(b.labels, torch.cat([s.labels for s in samples]))
    want = collate(samples)
    for k in want.keys():
        if torch.is_tensor(want[k]):
            assert torch.equal(b[k], want[k]), k
    nv = torch.stack([s.num_vertices.reshape(-1) for s in samples])
    assert torch.equal(b.num_vertices, nv.int())
    off = int(samples[0].num_vertices.reshape(-1)[1])
    assert torch.equal(b.hierarchy_trace_index_1[samples[0].x.shape[0]:][:5], samples[1].hierarchy_trace_index_1[:5] + off)


def test_eval_scene_keeps_original_index_traces_through_scene_loader(reader, tmp_path):
    from surface_texture_inpainting_net_amd.loader import SceneLoader
    p = tmp_path / 'scene0042_00.pt'
    torch.save(_saved(reader, 'full'), p)
    loader = SceneLoader([functools.partial(scene_io.load_label_scene, str(p), 4, False)], 'cpu', batch_size=1, shuffle=False)
    for epoch in range(2):
        (b,) = list(loader.epoch(epoch))
        assert torch.equal(b.original_index_traces, torch.from_numpy(reader['full.s.original_index_traces']))
        assert torch.equal(b.labels, torch.from_numpy(reader['full.s.labels']))


def _assert_scores(got, z, prefix):
    for k in SCORE_KEYS:
        want = z['%s.%s' % (prefix, k)]
        g = np.asarray(got[k], dtype=np.float64)
        assert g.shape == want.shape, k
        assert np.array_equal(np.isnan(g), np.isnan(want)), k
        assert np.allclose(g[~np.isnan(g)], want[~np.isnan(want)], rtol=1e-12, atol=0), k


@pytest.mark.parametrize('key', ['conf_ab', 'conf_e'])
@pytest.mark.parametrize('ig_tag,ig', [('ig0', 0), ('none', None)])
def test_scores_match_iou_dcm(metrics, key, ig_tag, ig):
    conf = metrics[key].copy()
    before = conf.copy()
    _assert_scores(seg.scores(conf, ig), metrics, '%s.%s' % (key, ig_tag))
    assert np.array_equal(conf, before)                    # the caller's matrix is left as it is (the reference zeroes it)
    t = torch.from_numpy(conf.astype(np.int64))
    _assert_scores(seg.scores(t, ig), metrics, '%s.%s' % (key, ig_tag))
    assert np.array_equal(t.numpy(), before)
    if ig == 0:
        assert np.isnan(seg.scores(conf, 0)['iou'][17])     # the class that never occurs


def test_cpu_path_matches_fixture(metrics):
    w = torch.from_numpy(metrics['weight'])
    crit = seg.CrossEntropyLoss(weight=w, ignore_index=0)
    cm = seg.ConfusionMatrix(K, 'cpu')
    za = torch.from_numpy(metrics['za'])
    loss = crit(za, torch.from_numpy(metrics['ya']), confusion=cm)
    assert torch.equal(loss, torch.from_numpy(metrics['loss_a']))
    assert np.array_equal(cm.value().numpy(), metrics['conf_a'])
    cm.add(torch.from_numpy(metrics['zb']), torch.from_numpy(metrics['yb']))
    assert cm.value().dtype == torch.int64 and np.array_equal(cm.value().numpy(), metrics['conf_ab'])
    ce = seg.ConfusionMatrix(K, 'cpu')
    ze, tr, ye = (torch.from_numpy(metrics[k]) for k in ('ze', 'tr', 'ye'))
    with torch.no_grad():
        le = crit(ze, ye, rows=tr, confusion=ce)
    assert torch.allclose(le, torch.from_numpy(metrics['loss_e']), rtol=1e-6)
    assert np.array_equal(ce.value().numpy(), metrics['conf_e'])
    _assert_scores(seg.scores(ce.value(), 0), metrics, 'conf_e.ig0')


def test_cpu_path_rejects_bad_labels_and_options():
    with pytest.raises(NotImplementedError):
        seg.CrossEntropyLoss(reduction='sum')
    cm = seg.ConfusionMatrix(3, 'cpu')
    with pytest.raises(IndexError):
        cm.add(torch.randn(4, 3), torch.tensor([0, 1, 3, 2]))
    with pytest.raises(ValueError):
        seg.ConfusionMatrix(129, 'cpu')


def test_objective_wraps_a_torch_criterion():
    w = torch.rand(K)
    obj = seg.Objective(torch.nn.CrossEntropyLoss(weight=w, ignore_index=0))
    assert isinstance(obj.criterion, seg.CrossEntropyLoss) and obj.criterion.ignore_index == 0
    assert torch.equal(obj.criterion.weight, w)

    class _M(torch.nn.Module):
        def forward(self, s):
            return s.x

    s = make_synthetic_mesh(50, 1, seed=0, dilations=())
    s['x'] = torch.randn(s.x.shape[0], K)
    s['labels'] = torch.randint(0, K, (s.x.shape[0],))
    want = torch.nn.functional.cross_entropy(s.x, s.labels, weight=w, ignore_index=0)
    assert torch.equal(obj(_M(), s), want)


def _free_port():
    so = socket.socket()
    so.bind(('127.0.0.1', 0))
    p = so.getsockname()[1]
    so.close()
    return p


def _allreduce_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    g = torch.Generator().manual_seed(rank)
    z, y = torch.randn(500 + 100 * rank, K, generator=g), torch.randint(0, K, (500 + 100 * rank,), generator=g)
    cm = seg.ConfusionMatrix(K, 'cpu')
    cm.add(z, y)
    torch.save({'own': cm.value().clone(), 'z': z, 'y': y}, os.path.join(out_dir, 'r%d.pt' % rank))
    cm.all_reduce()
    torch.save({'own': torch.load(os.path.join(out_dir, 'r%d.pt' % rank))['own'], 'sum': cm.value(), 'z': z, 'y': y},
               os.path.join(out_dir, 'r%d.pt' % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_confusion_all_reduce_two_gloo_ranks(tmp_path):
    mp.spawn(_allreduce_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r = [torch.load(tmp_path / ('r%d.pt' % i)) for i in range(2)]
    assert torch.equal(r[0]['sum'], r[1]['sum']) and r[0]['sum'].dtype == torch.int64
    assert torch.equal(r[0]['sum'], r[0]['own'] + r[1]['own'])
    want = np.zeros((K, K), dtype=np.int64)
    for q in r:
        pred = q['z'].argmax(1).numpy()
        want += np.bincount(pred + K * q['y'].numpy(), minlength=K * K).reshape(K, K)
    assert np.array_equal(r[0]['sum'].numpy(), want)
