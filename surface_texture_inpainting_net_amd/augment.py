"""Training augmentation of the 3-D inpainting recipe on the device.

The shipped config (experiments/3d_inpainting/config/config_stinet_surfacetextureinpainting.json:52-73) trains with
``[CoordsNormalization(1.5, 1.5, 1.5), RandomLinearTransformation(flip=True), RandomRotation()]``, applied by the dataset to
every item (datasets/scannetcolorgraph_dataloader.py:153-154).  ``scene_io.load_scene`` already applies the normalisation;
this module provides the other two, and ``CircleMask``: a fresh circle mask per visit (preprocessing.circle_masks), the
way the reference's 2-D dataset draws random circles per item.

Randomness is drawn on the host from a CPU ``torch.Generator`` seeded by (seed, epoch, item index), in the reference's
order: ``randn(3, 3)`` for M = I + 0.1 randn (M[0, 0] negated with flip), then ``rand(1)`` for theta = rand * 2 pi in fp32,
then the mask seed.  Rz is built as transform/random_rotation.py:14-16 builds it (math.cos / math.sin of that theta, rounded
to fp32), so with a generator in the same state both matrices are bitwise the reference classes' matrices.  Nothing is drawn
from the global RNG.  The device work is one circle-mask pass (stin_circle_mask_run) and ONE per-vertex rewrite
(stin_augment_rewrite_f32) of the uploaded sample: x[:, 0:3] = colour * known, x[:, 9] = known, mask; normal @ Rz;
(pos @ M) @ Rz.  loader.SceneLoader(augment=...) applies it to the device copy of every training batch.
"""
import ctypes
import math

import torch

from . import _lib
from .plan import _ptr, _stream


class Params:
    """One item's draws: lin (fp32 [3, 3] or None), rot (fp32 [3, 3] or None), theta (fp32 tensor or None), mask_seed."""

    def __init__(self, lin=None, rot=None, theta=None, mask_seed=None):
        self.lin, self.rot, self.theta, self.mask_seed = lin, rot, theta, mask_seed


class RandomLinearTransformation:
    """transform/random_linear_transformation.py: x[:, 6:9] @ M, M = I + pertubation_factor * randn(3, 3), M[0, 0] *= -1 with
    flip (the reference's spelling of the argument is kept)."""

    def __init__(self, flip=True, pertubation_factor=0.1):
        self.flip, self.pertubation_factor = bool(flip), float(pertubation_factor)

    def draw(self, g, p):
        m = torch.eye(3) + torch.randn(3, 3, generator=g) * self.pertubation_factor
        if self.flip:
            m[0, 0] *= -1
        p.lin = m


class RandomRotation:
    """transform/random_rotation.py: a rotation about the height axis, x[:, 3:6] @ Rz and x[:, 6:9] @ Rz."""

    def draw(self, g, p):
        theta = torch.rand(1, generator=g) * 2 * math.pi
        p.theta = theta
        p.rot = torch.FloatTensor([[math.cos(theta), math.sin(theta), 0],
                                   [-math.sin(theta), math.cos(theta), 0],
                                   [0, 0, 1]])


class CircleMask:
    """A new circle mask per visit: preprocessing.circle_masks(radius, frac_masked_vertices) on level 0 of the sample,
    seeded by the item's draw.  Replaces the sample's mask and the x columns that depend on it."""

    def __init__(self, radius=16, frac_masked_vertices=0.25, max_iters=32):
        if int(radius) < 1:
            raise ValueError('radius must be >= 1')
        self.radius, self.frac, self.max_iters = int(radius), float(frac_masked_vertices), int(max_iters)

    def draw(self, g, p):
        p.mask_seed = int(torch.randint(0, 1 << 62, (1,), generator=g))


def item_generator(seed, epoch, index):
    """The CPU generator of one item of one epoch (independent of ranks, workers and batching)."""
    h = 0
    for v in (int(seed), int(epoch), int(index)):
        h = (h * 0x100000001B3 + (v & 0xFFFFFFFFFFFFFFFF) + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        h ^= h >> 31
    return torch.Generator().manual_seed(h & ((1 << 63) - 1))


class Compose:
    """The transforms of one training item, in order.  The fused device pass needs the linear transformation (if any) before
    the rotation (if any), the shipped order; at most one of each kind."""

    def __init__(self, transforms):
        self.transforms = list(transforms)
        kinds = [type(t) for t in self.transforms]
        for k in (RandomLinearTransformation, RandomRotation, CircleMask):
            if kinds.count(k) > 1:
                raise ValueError('at most one %s per Compose' % k.__name__)
        if RandomLinearTransformation in kinds and RandomRotation in kinds and \
                kinds.index(RandomRotation) < kinds.index(RandomLinearTransformation):
            raise ValueError('RandomRotation before RandomLinearTransformation is not supported by the fused pass')
        self.mask = next((t for t in self.transforms if isinstance(t, CircleMask)), None)

    def draw(self, generator):
        p = Params()
        for t in self.transforms:
            t.draw(generator, p)
        return p

    def params_for(self, seed, epoch, index):
        return self.draw(item_generator(seed, epoch, index))

    def apply_(self, sample, params, adjacency=None, ptr=None, rows=None):
        """Rewrite the DEVICE sample in place (x, mask).  params: one Params, or one per graph of a collated batch (then rows:
        the host list of vertex ranges [(begin, end), ...] and ptr: the device [B + 1] vertex offsets).  adjacency: the level-0
        preprocessing.mask_adjacency of the sample (built here when None).  No host synchronisation."""
        from . import preprocessing
        lib = _lib.load()
        plist = params if isinstance(params, (list, tuple)) else [params]
        x = sample['x']
        n = int(x.shape[0])
        if rows is None:
            rows = [(0, n)]
        if len(rows) != len(plist):
            raise ValueError('one Params per graph')
        dist = None
        if self.mask is not None:
            if adjacency is None:
                adjacency = preprocessing.mask_adjacency(sample['edge_index'], n, check=False)
            dist, _, _, _ = preprocessing._circle_dist(adjacency, n, self.mask.radius, self.mask.frac, 1, 0,
                                                       ptr if len(plist) > 1 else None, self.mask.max_iters,
                                                       graph_seeds=[p.mask_seed for p in plist])
            mask = sample['mask']
            if mask.dtype != torch.int64 or mask.numel() != n or not mask.is_contiguous():
                mask = torch.empty(n, 1, dtype=torch.int64, device=x.device)
            sample['mask'] = mask.view(n, 1)
        if x.dtype != torch.float32 or x.stride(1) != 1 or x.shape[1] < 10:
            raise TypeError('x must be fp32 [N, >= 10] with unit column stride')
        color = sample['color'] if dist is not None else None
        if color is not None and (color.dtype != torch.float32 or color.stride(1) != 1):
            raise TypeError('color must be fp32 [N, 3] with unit column stride')
        for (b, e), p in zip(rows, plist):
            if e <= b:
                continue
            lin = (ctypes.c_float * 9)(*p.lin.reshape(-1).tolist()) if p.lin is not None else None
            rot = (ctypes.c_float * 9)(*p.rot.reshape(-1).tolist()) if p.rot is not None else None
            _lib.check(lib.stin_augment_rewrite_f32(_ptr(x[b:e]), x.stride(0), _ptr(color[b:e]) if color is not None else None,
                                                    color.stride(0) if color is not None else 0,
                                                    _ptr(dist[0, b:e]) if dist is not None else None,
                                                    self.mask.radius if dist is not None else 0,
                                                    _ptr(sample['mask'][b:e]) if dist is not None else None, e - b, lin, rot,
                                                    _stream(x)), 'stin_augment_rewrite_f32')
        return sample


def apply_reference(x, params):
    """The reference composition in CPU fp32 (what the fused pass is checked against): x[:, 6:9] @ M, then x[:, 3:6] @ Rz and
    x[:, 6:9] @ Rz, exactly as the transform classes write it.  Returns a new tensor."""
    x = x.clone()
    if params.lin is not None:
        x[:, 6:9] = x[:, 6:9] @ params.lin
    if params.rot is not None:
        x[:, 3:6] = x[:, 3:6] @ params.rot
        x[:, 6:9] = x[:, 6:9] @ params.rot
    return x


_KNOWN = {'RandomLinearTransformation': RandomLinearTransformation, 'RandomRotation': RandomRotation}


def from_config(train_transform_list, max_sizes=(1.5, 1.5, 1.5), circle_mask=None):
    """The reference's ``train_transform`` JSON entries ([{'type': ..., 'args': {...}}, ...]) -> Compose.
    CoordsNormalization is accepted only with the reader's max_sizes (scene_io.load_scene already applies it); any other
    unknown entry raises ValueError.  circle_mask (a CircleMask, optional) is appended last: its seed is drawn after the
    matrices."""
    out = []
    for ent in train_transform_list:
        kind, args = ent['type'], dict(ent.get('args') or {})
        if kind == 'CoordsNormalization':
            got = [float(v) for v in args.get('max_sizes', ())]
            if got != [float(v) for v in max_sizes]:
                raise ValueError('CoordsNormalization(%s) differs from the reader\'s max_sizes %s' % (got, list(max_sizes)))
            continue
        if kind not in _KNOWN:
            raise ValueError('train_transform entry %r has no device equivalent' % kind)
        out.append(_KNOWN[kind](**args))
    if circle_mask is not None:
        out.append(circle_mask)
    return Compose(out)
