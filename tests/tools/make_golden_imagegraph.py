"""Generate tests/golden/g20_imagegraph.npz by RUNNING THE REFERENCE'S OWN CODE for the 2-D image-graph dataset.

Runs only where the reference tree exists (read-only; nothing is copied from it), through oracle/ref_import.py, in the manner of
tests/tools/make_golden_inpaint_metrics.py.  The reference's ImageGraphTextureDataSet.__getitem__ builds every sample, through
the reference's own CenterCrop, RandomRotation, RandomFlip and ToTensor; `io.imread` of the stubbed skimage.io returns arrays from
a dict and the first transform applies the normalise expression that img_as_float32 followed by `* 2.0 - 1` gives on a float32
array (skimage itself is not installed):  v = float32(u8) * float32(1 / 255);  v * 2 - 1.

The fixture holds DATA only.  `cases` is a JSON list; sample j has
    j.img                 the uint8 H x W x 3 input
    j.x / j.color / j.mask  the reference's sample (x holds negative zeros: color * False)
    j.k / j.flip / j.starts  the draws, recovered by wrapping random.choice / np.random.choice / random.random
and per distinct (img_size, end_level) `G<S>_<L>.edge<l>` (the reference's edge list, [E, 2] in its set order), `.trace<l>`,
`.num_vertices`.  A numpy replay of every sample from (img, k, flip, starts) must reproduce color and mask exactly, and
np.rot90 must equal what the reference's ndimage.rotate made - both are asserted here.

    python tests/tools/make_golden_imagegraph.py          # rewrites tests/golden/g20_imagegraph.npz
"""
import contextlib
import io as _io
import json
import os
import random
import sys
import warnings

import numpy as np
import torch

_REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, _REPO)
warnings.filterwarnings('ignore')

from oracle import ref_import  # noqa: E402

OUT = os.path.join(_REPO, 'tests', 'golden')
MAX_FILE_BYTES = 1 << 20

# (img_size, end_level, circle_radius, crop_half_width, input h, input w); every circle stays inside the image for the fixed and
# for any random placement (|offset| <= int((S / 2 - chw) * 0.95))
CASES = [
    dict(tag='A', S=16, L=3, R=2, chw=2, h=16, w=21),
    dict(tag='B', S=18, L=2, R=2, chw=3, h=23, w=18),        # the asymmetric // 4 offsets (-5, +4); 324 pixels
    dict(tag='C', S=16, L=3, R=3, chw=2, h=16, w=16),        # overlapping circles
    dict(tag='D0', S=16, L=3, R=2, chw=2, h=16, w=21),       # D0..D2: one batch of three images of different h, w
    dict(tag='D1', S=16, L=3, R=2, chw=2, h=19, w=16),
    dict(tag='D2', S=16, L=3, R=2, chw=2, h=16, w=16),
]


class _Normalize:
    def __call__(self, sample):
        v = sample['color'].astype(np.float32) * np.float32(1.0 / 255.0)
        return {'color': v * np.float32(2.0) - np.float32(1.0)}


class _Compose:
    def __init__(self, ts):
        self.ts = ts

    def __call__(self, sample):
        for t in self.ts:
            sample = t(sample)
        return sample


@contextlib.contextmanager
def _recording(log):
    """Wrap the global generators' draws the reference makes (random.choice, np.random.choice, random.random)."""
    keep = random.choice, np.random.choice, random.random

    def choice(seq):
        v = keep[0](seq)
        log['angle'] = v
        return v

    def np_choice(*a, **k):
        v = keep[1](*a, **k)
        log['flip'] = bool(v)
        return v

    def rnd():
        v = keep[2]()
        log.setdefault('u', []).append(v)
        return v

    random.choice, np.random.choice, random.random = choice, np_choice, rnd
    try:
        yield
    finally:
        random.choice, np.random.choice, random.random = keep


def _replay(img, S, R, k, flip, starts):
    v = img.astype(np.float32) * np.float32(1.0 / 255.0)
    v = v * np.float32(2.0) - np.float32(1.0)
    h, w = img.shape[:2]
    h0, w0 = int((h - S) / 2), int((w - S) / 2)
    v = np.rot90(v[h0:h0 + S, w0:w0 + S], k, axes=(0, 1))
    if flip:
        v = np.flip(v, axis=1)
    a = np.arange(2 * R) - R
    circle = (a[:, None] ** 2 + a[None, :] ** 2) <= R * R
    m = np.zeros((S, S), dtype=bool)
    for r0, c0 in starts:
        assert 0 <= r0 and r0 + 2 * R <= S and 0 <= c0 and c0 + 2 * R <= S, (r0, c0)
        m[r0:r0 + 2 * R, c0:c0 + 2 * R] |= circle
    return np.ascontiguousarray(v).reshape(-1, 3), m.reshape(-1, 1)


def main():
    mod = ref_import.load_imagegraph_dataset_class()
    rng = np.random.RandomState(2020)
    d, cases, images = {}, [], {}
    mod.io.imread = lambda path: images[str(path)]
    seen_k, seen_flip, datasets = set(), set(), {}

    def dataset(c, random_placement):
        key = (c['S'], c['L'], c['R'], c['chw'], random_placement)
        if key not in datasets:
            tf = _Compose([_Normalize(), mod.CenterCrop((c['S'], c['S'])), mod.RandomRotation(), mod.RandomFlip(flip_axis=1),
                           mod.ToTensor()])
            with contextlib.redirect_stdout(_io.StringIO()):
                datasets[key] = mod.ImageGraphTextureDataSet(
                    sorted(images), c['L'], is_train=random_placement, benchmark=False, img_size=c['S'], crop_half_width=c['chw'],
                    circle_radius=c['R'], transform=tf, random_mask=random_placement)
        return datasets[key]

    for c in CASES:
        images[c['tag']] = rng.randint(0, 256, size=(c['h'], c['w'], 3)).astype(np.uint8)
    names = sorted(images)

    def run(c, random_placement, seed):
        log = {}
        random.seed(seed)
        np.random.seed(seed + 1000)
        with _recording(log):
            s = dataset(c, random_placement)[names.index(c['tag'])]
        return s, log

    j = 0
    for c in CASES:
        for random_placement in (True, False):
            # seeds: the first that adds a rotation not seen yet, then one that adds a flip value, else the sample's number
            seed = j
            for cand in range(200):
                _, log = run(c, random_placement, cand)
                if (len(seen_k) < 4 and log['angle'] // 90 not in seen_k) or (len(seen_k) == 4 and len(seen_flip) < 2
                                                                             and log['flip'] not in seen_flip):
                    seed = cand
                    break
            s, log = run(c, random_placement, seed)
            S, R = c['S'], c['R']
            k, flip = log['angle'] // 90, log['flip']
            seen_k.add(k)
            seen_flip.add(flip)
            if random_placement:
                u = log['u']
                assert len(u) == 8
                offs = [int((S / 2 - c['chw']) * (v * 2.0 - 1.0) * 0.95) for v in u]
                starts = [(S // 2 - R + offs[2 * i], S // 2 - R + offs[2 * i + 1]) for i in range(4)]
            else:
                assert 'u' not in log
                starts = [(S // 2 - R + ((i % 2) * 2 - 1) * S // 4, S // 2 - R + ((i // 2) * 2 - 1) * S // 4) for i in range(4)]
            color, mask = _replay(images[c['tag']], S, R, k, flip, starts)
            assert np.array_equal(color, s.color.numpy()) and np.array_equal(mask, s.mask.numpy()), (c, seed)
            assert s.x.dtype == torch.float32 and s.color.dtype == torch.float32 and s.mask.dtype == torch.bool
            assert torch.equal(s.x, torch.cat([s.color * ~s.mask, s.mask], dim=-1))
            p = '%d.' % j
            d[p + 'img'], d[p + 'x'], d[p + 'color'], d[p + 'mask'] = images[c['tag']], s.x.numpy(), s.color.numpy(), s.mask.numpy()
            d[p + 'k'], d[p + 'flip'] = np.int64(k), np.bool_(flip)
            d[p + 'starts'] = np.asarray(starts, dtype=np.int64)
            cases.append(dict(c, index=j, random_placement=random_placement, py_seed=seed, np_seed=seed + 1000))
            g = 'G%d_%d.' % (S, c['L'])
            if g + 'num_vertices' not in d:
                d[g + 'num_vertices'] = s.num_vertices.numpy()
                d[g + 'edge0'] = s.edge_index.t().contiguous().numpy()
                for l in range(1, c['L']):
                    d[g + 'edge%d' % l] = s['hierarchy_edge_index_%d' % l].t().contiguous().numpy()
                    d[g + 'trace%d' % l] = s['hierarchy_trace_index_%d' % l].numpy()
            j += 1
    assert seen_k == {0, 1, 2, 3} and seen_flip == {False, True}, (seen_k, seen_flip)
    assert any((d['%d.x' % i] == 0).any() and np.signbit(d['%d.x' % i][d['%d.x' % i] == 0]).any() for i in range(j))
    d['cases'] = np.frombuffer(json.dumps(cases).encode(), dtype=np.uint8)
    path = os.path.join(OUT, 'g20_imagegraph.npz')
    np.savez_compressed(path, **d)
    assert os.path.getsize(path) <= MAX_FILE_BYTES, os.path.getsize(path)
    print('g20_imagegraph', len(d), 'arrays', os.path.getsize(path), 'bytes')
    for c in cases:
        print(c['index'], c['tag'], 'random' if c['random_placement'] else 'fixed', 'seed', c['py_seed'], 'k', int(d['%d.k' % c['index']]),
              'flip', bool(d['%d.flip' % c['index']]), d['%d.starts' % c['index']].tolist())


if __name__ == '__main__':
    if not ref_import.available():
        sys.exit('the reference tree is needed to regenerate the g20 fixture')
    main()
