"""Circle masks and training augmentation on the CPU: the heap-BFS oracle and the batch-size rule against the reference's own
process_frame_circles (g16 fixture, recorded centres), the host-drawn matrices against the reference transform classes, the mask
writer against approve_and_write_out_mask, load_scene reading the writer's files, and from_config."""
import json
import os

import numpy as np
import pytest
import torch

from _golden import load_npz
from _mask_oracle import adjacency, heap_bfs_mask, rule_sizes
from surface_texture_inpainting_net_amd import augment, scene_io
from surface_texture_inpainting_net_amd.synthetic import make_synthetic_mesh


@pytest.fixture(scope='module')
def g16():
    return load_npz('g16_circle_masks')


def _batches(z, r):
    return [z['circ.R%d.batch.%d' % (r, i)] for i in range(int(z['circ.R%d.nbatches' % r]))]


def _split_by_mask(z, r):
    """The recorded centre batches, grouped per mask by replaying the rule (a mask ends where the rule says stop)."""
    n = z['mesh.pos'].shape[0]
    adj = adjacency(z['mesh.edge_index'], n)
    out, cur, mask, total = [], [], np.zeros(n, dtype=np.int64), 0
    for b in _batches(z, r):
        heap_bfs_mask(adj, r, b, mask)
        cur.append(b)
        total += len(b)
        masked = int((mask > 0).sum())
        k = int(total * (0.25 / (masked / n) - 1))
        if masked / n >= 0.25 or k <= 0:
            out.append((cur, mask))
            cur, mask, total = [], np.zeros(n, dtype=np.int64), 0
    assert not cur
    return out


@pytest.mark.parametrize('r', [16, 4])
def test_heap_oracle_reproduces_reference_masks(g16, r):
    per_mask = _split_by_mask(g16, r)
    assert len(per_mask) == 2
    for i, (_, mask) in enumerate(per_mask):
        assert np.array_equal(mask, g16['circ.R%d.mask.%d' % (r, i)]), (r, i)


@pytest.mark.parametrize('r', [16, 4])
def test_batch_rule_reproduces_recorded_sizes(g16, r):
    n = g16['mesh.pos'].shape[0]
    adj = adjacency(g16['mesh.edge_index'], n)
    for batches, _ in _split_by_mask(g16, r):
        mask, counts = np.zeros(n, dtype=np.int64), []
        for b in batches:
            heap_bfs_mask(adj, r, b, mask)
            counts.append(int((mask > 0).sum()))
        assert rule_sizes(counts, n, 0.25) == [len(b) for b in batches]


def test_host_matrices_are_bitwise_the_reference_classes(g16):
    for sd in g16['tf.seeds'].tolist():
        p = augment.Compose([augment.RandomLinearTransformation(flip=True)]).draw(torch.Generator().manual_seed(sd))
        assert torch.equal(p.lin, torch.from_numpy(g16['tf.lin.%d' % sd])), sd
        p = augment.Compose([augment.RandomRotation()]).draw(torch.Generator().manual_seed(sd))
        assert torch.equal(p.rot, torch.from_numpy(g16['tf.rot.%d' % sd])), sd


def test_reference_composition_restated(g16):
    """CoordsNormalization (the reader's) then the two draws of one generator, in CPU fp32: the shipped train_transform."""
    x = torch.from_numpy(g16['tf.comp.x_in']).clone()
    x[:, 6:9] = x[:, 6:9] / torch.tensor([1.5, 1.5, 1.5])
    comp = augment.from_config([{'type': 'CoordsNormalization', 'args': {'max_sizes': [1.5, 1.5, 1.5]}},
                                {'type': 'RandomLinearTransformation', 'args': {'flip': True}},
                                {'type': 'RandomRotation', 'args': {}}])
    p = comp.draw(torch.Generator().manual_seed(int(g16['tf.seeds'][0])))
    got = augment.apply_reference(x, p)
    assert torch.equal(got, torch.from_numpy(g16['tf.comp.x_out']))


def test_item_draws_depend_on_seed_epoch_item_only():
    comp = augment.Compose([augment.RandomLinearTransformation(), augment.RandomRotation(), augment.CircleMask()])
    a = comp.params_for(5, 2, 17)
    torch.manual_seed(0)
    b = comp.params_for(5, 2, 17)
    assert torch.equal(a.lin, b.lin) and torch.equal(a.rot, b.rot) and a.mask_seed == b.mask_seed
    c = comp.params_for(5, 3, 17)
    d = comp.params_for(5, 2, 18)
    assert not torch.equal(a.lin, c.lin) and not torch.equal(a.lin, d.lin)
    assert a.mask_seed != c.mask_seed and a.mask_seed != d.mask_seed
    state = torch.random.get_rng_state()
    comp.params_for(1, 1, 1)
    assert torch.equal(state, torch.random.get_rng_state())        # nothing drawn from the global RNG


def test_writer_matches_reference_files(g16, tmp_path):
    masks = np.stack([g16['circ.R16.mask.0'], g16['circ.R16.mask.1']])
    got = {}
    for tag, sub in (('full', 'graph_levels/pp/train/masks/rad_16/scene0007_00'),
                     ('crop', 'cropped/pp/train/masks/rad_16/scene0007_00_2')):
        ids = torch.from_numpy(g16['write.%s.ids' % tag])
        v0 = torch.zeros(ids.numel(), 10)
        v0[:, 9] = ids
        gp = tmp_path / ('%s.pt' % tag)
        torch.save({'vertices': [v0], 'edges': [], 'traces': []}, gp)
        for p in scene_io.write_circle_masks(str(gp), str(tmp_path / sub), masks):
            got['data/generated/' + os.path.relpath(p, tmp_path)] = np.load(p)['vertex_mask']
    want = [str(f) for f in g16['write.files']]
    assert sorted(got) == sorted(want)
    for i, f in enumerate(want):
        assert got[f].dtype == g16['write.file.%d' % i].dtype
        assert np.array_equal(got[f], g16['write.file.%d' % i]), f


def test_load_scene_reads_written_masks(tmp_path):
    s = make_synthetic_mesh(800, 3, seed=4, dilations=(2, 4))
    gp, mp = tmp_path / 'scene0001_00.pt', tmp_path / 'orig.npz'
    scene_io.save_scene_like_reference(s, str(gp), str(mp))
    rng = np.random.default_rng(0)
    n = int(s.x.shape[0])
    masks = np.where(rng.random((3, n)) < 0.3, rng.integers(1, 17, (3, n)), 0)
    masks[1] = 0                                                     # rejected: nothing masked
    written = scene_io.write_circle_masks(str(gp), str(tmp_path / 'masks'), masks)
    assert [os.path.basename(p) for p in written] == ['000000.npz', '000002.npz']
    for p, m in zip(written, masks[[0, 2]]):
        smp = scene_io.load_scene(str(gp), p)
        assert torch.equal(smp.mask.reshape(-1), torch.from_numpy(m))
        known = (smp.mask == 0).float()
        assert torch.equal(smp.x[:, 9:10], known)


def test_from_config_parses_shipped_and_rejects_unknown():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g16_train_transform.json')
    shipped = json.load(open(path))
    comp = augment.from_config(shipped, circle_mask=augment.CircleMask(16, 0.25))
    assert [type(t).__name__ for t in comp.transforms] == ['RandomLinearTransformation', 'RandomRotation', 'CircleMask']
    assert comp.transforms[0].flip and comp.transforms[0].pertubation_factor == 0.1
    with pytest.raises(ValueError):
        augment.from_config([{'type': 'CoordsNormalization', 'args': {'max_sizes': [1.0, 1.5, 1.5]}}])
    with pytest.raises(ValueError):
        augment.from_config([{'type': 'MoveToOrigin', 'args': {}}])
    with pytest.raises(ValueError):
        augment.from_config([{'type': 'RandomRotation', 'args': {}}, {'type': 'RandomLinearTransformation', 'args': {}}])
