"""Training crops, CPU side: the numpy restatement (tests/_crop_oracle.py) against what the reference's own process_frame wrote
(tests/golden/g17_crops*.npz), the sampling positions, the file-counter rule, and a crop through the reader and the model."""
import numpy as np
import torch

import _crop_oracle as CO
from _golden import load_npz
from surface_texture_inpainting_net_amd import preprocessing as P, scene_io


def _fixture():
    z = load_npz('g17_crops')
    assert CO.fixture_scene_count(z) == 4
    return z


def test_restatement_matches_the_reference_bit_exact():
    z = _fixture()
    crops = redirected = repairs = size = labelled = 0
    for i in range(CO.fixture_scene_count(z)):
        saved, block, stride = CO.fixture_scene(z, i)
        stats = {}
        got = CO.crop_scene(saved, block, stride, reference_dilated_labels=True, stats=stats, return_kept=True)
        want = CO.fixture_crops(z, i)
        assert [c for c, _, _ in got] == [c for c, _, _ in want]
        for (_, a, ka), (_, b, kb) in zip(got, want):
            assert CO.same_crop(a, b) is None, (i, CO.same_crop(a, b))
            assert all(np.array_equal(x, y) for x, y in zip(ka, kb))
        crops += len(got)
        redirected += stats.get('redirected', 0)
        repairs += stats.get('repairs', 0)
        size += stats.get('size', 0)
        labelled += 'labels' in saved
    # the fixture covers what the GPU tests lean on
    assert crops == 27 and size >= 2 and redirected >= 100 and repairs >= 1 and labelled >= 1


def test_fixed_dilated_labels_differ_from_the_reference_and_are_rows_of_the_scene():
    z = _fixture()
    differ = 0
    for i in range(CO.fixture_scene_count(z)):
        saved, block, stride = CO.fixture_scene(z, i)
        fixed = CO.crop_scene(saved, block, stride, return_kept=True)
        for (_, a, kept), (_, b, _) in zip(fixed, CO.fixture_crops(z, i)):
            for l, sets in enumerate(a['dilated_edges']):
                for j, s in enumerate(sets or []):
                    if len(s) == 0:
                        continue
                    differ += not np.array_equal(s, b['dilated_edges'][l][j])
                    full = saved['dilated_edges'][l][j].numpy()
                    n = saved['vertices'][l].shape[0]
                    assert np.isin(kept[l][s[:, 0]] * n + kept[l][s[:, 1]], full[:, 0] * n + full[:, 1]).all()
    assert differ >= 1


def test_crop_positions_match_the_reference():
    z = _fixture()
    for i in range(CO.fixture_scene_count(z)):
        saved, _, stride = CO.fixture_scene(z, i)
        for xs, ys in (CO.crop_positions(saved['vertices'][0].numpy(), stride), P.crop_positions(saved['vertices'][0], stride)):
            assert xs.dtype == np.float64 and ys.dtype == np.float64
            assert np.array_equal(xs, z['s%d.xs' % i]) and np.array_equal(ys, z['s%d.ys' % i])


def test_counter_rule():
    """+ 1 per grid position, + 2 for a position rejected by size: the counters of the files the reference wrote."""
    z = _fixture()
    saved, block, stride = CO.fixture_scene(z, 0)
    sc = CO.scene_to_numpy(saved)
    xs, ys = CO.crop_positions(sc['vertices'][0], stride)
    counter, want = 0, []
    for box in CO.crop_boxes([(x, y) for x in xs for y in ys], block):
        what, _, _ = CO.crop_one(sc, box, None)
        if what == 'ok':
            want.append(counter)
        counter += 2 if what == 'size' else 1
    assert want == z['s0.counters'].tolist() and len(want) == 8 and counter == len(xs) * len(ys) + 8
    # explicit positions: the counter is the list index, rejected ones leave gaps
    centres = [(x, y) for x in xs for y in ys]
    got = CO.crop_scene(saved, block, stride, positions=centres)
    ok = [i for i, box in enumerate(CO.crop_boxes(centres, block)) if CO.crop_one(sc, box, None)[0] == 'ok']
    assert [c for c, _ in got] == ok


def test_fixture_crop_through_reader_and_model():
    from oracle import stin_oracle
    z = _fixture()
    saved, block, stride = CO.fixture_scene(z, 0)
    _, crop = CO.crop_scene(saved, block, stride)[0]
    crop = {k: ([torch.from_numpy(a) for a in v] if k in ('vertices', 'edges', 'traces') else
                [None if x is None else [torch.from_numpy(y) if len(y) else [] for y in x] for x in v] if k == 'dilated_edges' else v)
            for k, v in crop.items()}
    n0 = crop['vertices'][0].shape[0]
    mask = (torch.arange(n0) % 4 == 0).long() * 3
    s = scene_io.sample_from_tensors(crop, mask, 3, cropped=True)
    assert s.x.shape == (n0, 10) and s.num_vertices.tolist() == [[v.shape[0] for v in crop['vertices']]]
    torch.manual_seed(0)
    net = stin_oracle.define_G(input_nc=10, output_nc=3, ngf=16, filter_type='edgeconvtransinv', norm='instance', n_blocks=2,
                               n_levels=2, pooling_type='max', dilations=[1, 2, 4])
    assert net(s).shape == (n0, 3)
