"""The 2-D image-graph inpainting experiment (experiments/2d_inpainting, config 1) in front of the network.

The reference's ImageGraphTextureDataSet (datasets/imagegraph_dataloader.py:21-160) treats an S x S image as a graph: every pixel a
vertex, 4-connected edges, `end_level` levels of 2x decimation with "fake traces" (np.repeat).  Per item its CPU workers read a PNG,
run Normalize / Rescale / CenterCrop / RandomRotation / RandomFlip, paint `num_circles` circle masks with Python loops and hand
(x, color, mask) to the PyG collate; the batch is then copied to the device.  Here the images stay resident on the device as raw
bytes, the graph and its plan are built once per batch size, and ONE launch per batch (stin_image_samples_u8) builds the samples:

    grid_levels        the graph tensors under the reference's keys (one launch, stin_grid_levels_i64)
    draw_image_params  the reference's random draws of one item, in its order, from its generators
    build_samples      x / color / mask of a batch from the resident byte pool
    rescale_size       the size the reference's Rescale gives an image
    ImageGraphLoader   epochs of HierarchicalBatch objects with a resident, shared GraphPlan
    (metrics.ImageStepMetrics: the 2-D trainer's step metrics as rows of a device table)

Every function takes CPU tensors too and then runs a torch / numpy path with the same semantics.

`Rescale` (cv2.INTER_AREA) is ImageGraphLoader(..., rescale=True): every larger image is area-resized to rescale_size once, at
construction, in one launch (preprocessing.resize_pool_u8: the exact area average in integers, include/stin_hip.h "Image resize",
not pinned against cv2; on the bytes, where the reference runs it after Normalize on float32 - at most half a grey level apart).
Without it an image must already have min(h, w) == img_size, as the reference's images have after its Rescale(img_size, img_size).
Out of scope: PNG decoding (the caller's business: `images` are uint8 arrays).  The edge ORDER is defined here (the reference iterates a Python set): image-major, then the source
vertex in row-major order, then its neighbours up, left, right, down.
"""
import collections
import random

import numpy as np
import torch

from . import augment
from .data import HierarchicalBatch
from .loader import shard_indices

ImageRecord = collections.namedtuple('ImageRecord', 'offset h w k flip starts')
ImageRecord.__doc__ = """One item of build_samples: byte offset of the raw h x w x 3 uint8 image in the pool, rotation k (0..3, quarter
turns of np.rot90), flip (along axis 1), starts = [(row_start, col_start), ...] of the circle windows."""


def _check_levels(img_size, end_level, batch):
    img_size, end_level, batch = int(img_size), int(end_level), int(batch)
    if img_size < 1 or end_level < 1 or batch < 1:
        raise ValueError('img_size, end_level and batch must be positive')
    if img_size % (2 ** (end_level - 1)) != 0:
        raise ValueError('img_size %d is not divisible by 2**(end_level - 1) = %d' % (img_size, 2 ** (end_level - 1)))
    return img_size, end_level, batch


def _grid_edges_cpu(s, batch):
    """[2, batch * 4 s (s - 1)] int64 in the defined order."""
    r, c = np.divmod(np.arange(s * s, dtype=np.int64), s)
    v = r * s + c
    valid = np.stack([r > 0, c > 0, c < s - 1, r < s - 1], axis=1)               # up, left, right, down
    dst = np.stack([v - s, v - 1, v + 1, v + s], axis=1)
    src = np.broadcast_to(v[:, None], dst.shape)
    one = np.stack([src[valid], dst[valid]])                                    # (boolean indexing walks row-major: source-major)
    off = (np.arange(batch, dtype=np.int64) * (s * s))[None, :, None]
    return torch.from_numpy((one[:, None, :] + off).reshape(2, batch * one.shape[1]))


def grid_levels(img_size, end_level, batch=1, device='cpu'):
    """The graph part of a batch of `batch` image graphs -> dict: edge_index, hierarchy_edge_index_{l}, hierarchy_trace_index_{l}
    (l = 1 .. end_level - 1), num_vertices ([batch, end_level] int32), batch ([batch S S] int64): what data.collate makes of the
    reference's samples, with the edge order defined in the module docstring.  On a GPU device: one launch, no synchronisation."""
    S, L, B = _check_levels(img_size, end_level, batch)
    device = torch.device(device)
    sides = [S // 2 ** l for l in range(L)]
    out = {}
    if device.type != 'cuda':
        for l, s in enumerate(sides):
            out['edge_index' if l == 0 else 'hierarchy_edge_index_%d' % l] = _grid_edges_cpu(s, B)
            if l > 0:
                sf = sides[l - 1]
                b, p = np.divmod(np.arange(B * sf * sf, dtype=np.int64), sf * sf)
                r, c = np.divmod(p, sf)
                out['hierarchy_trace_index_%d' % l] = torch.from_numpy(b * s * s + (r // 2) * s + (c // 2))
        out['num_vertices'] = torch.tensor([[s * s for s in sides]] * B, dtype=torch.int32)
        out['batch'] = torch.arange(B, dtype=torch.int64).repeat_interleave(S * S)
        return out
    from . import _lib
    from . import functional as SF
    from .plan import _ptr, _stream
    lib = _lib.load()
    if L > _lib.CONSTANTS['STIN_GRID_MAX_LEVELS']:
        raise ValueError('end_level above %d' % _lib.CONSTANTS['STIN_GRID_MAX_LEVELS'])
    elems = lib.stin_grid_levels_elems(B, S, L)
    if elems <= 0:
        raise ValueError('grid of %d images of side %d over %d levels is not supported' % (B, S, L))
    flat = torch.empty(elems, dtype=torch.int64, device=device)
    nv = torch.empty(B, L, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        SF._call('stin_grid_levels_i64', B, S, L, _ptr(flat), elems, _ptr(nv), _stream(flat))
    at = 0
    for l, s in enumerate(sides):
        e = B * 4 * s * (s - 1)
        out['edge_index' if l == 0 else 'hierarchy_edge_index_%d' % l] = flat[at:at + 2 * e].view(2, e)
        at += 2 * e
        if l > 0:
            n = B * sides[l - 1] ** 2
            out['hierarchy_trace_index_%d' % l] = flat[at:at + n]
            at += n
    out['num_vertices'] = nv
    out['batch'] = flat[at:at + B * S * S]
    return out


def draw_image_params(py_rng, np_rng, img_size, crop_half_width, circle_radius, num_circles=4, is_train=True, random_mask=False,
                      random_augmentation=False):
    """One item's draws -> (k, flip, starts) in the reference's order from the reference's generators: RandomRotation's
    py_rng.choice([0, 90, 180, 270]) and RandomFlip's np_rng.choice(a=[False, True]) (with random_augmentation: both are in the
    training transform list, imagegraph_dataloader.py:308-312), then __getitem__'s two py_rng.random() per circle (:127-138; with
    is_train and random_mask, else the fixed placement).  With random.Random(s) and np.random.RandomState(t) the result is what the
    reference produces after random.seed(s); np.random.seed(t).  The expressions keep Python's precedence and floor division."""
    S, R = int(img_size), int(circle_radius)
    k, flip = 0, False
    if random_augmentation:
        k = py_rng.choice([0, 90, 180, 270]) // 90
        flip = bool(np_rng.choice(a=[False, True]))
    starts = []
    for i in range(int(num_circles)):
        if is_train and random_mask:
            x_offset = int((S / 2 - crop_half_width) * (py_rng.random() * 2.0 - 1.0) * 0.95)
            y_offset = int((S / 2 - crop_half_width) * (py_rng.random() * 2.0 - 1.0) * 0.95)
        else:
            x_offset = ((i % 2) * 2 - 1) * S // 4
            y_offset = ((i // 2) * 2 - 1) * S // 4
        starts.append((S // 2 - R + x_offset, S // 2 - R + y_offset))
    return k, flip, starts


def rescale_size(h, w, img_size):
    """(new_h, new_w) of the reference's Rescale(img_size, img_size).__call__ for an h x w image (imagegraph_dataloader.py:197-209):
    the shorter side becomes img_size, the longer one int(img_size * longer / shorter) - Python's true division, then truncation."""
    h, w, output_size = int(h), int(w), int(img_size)
    if h > w:
        new_h, new_w = output_size * h / w, output_size
    else:
        new_h, new_w = output_size, output_size * w / h
    return int(new_h), int(new_w)


def circle_template(circle_radius):
    """bool [2R, 2R]: (r - R)^2 + (c - R)^2 <= R^2 (imagegraph_dataloader.py:35-39)."""
    R = int(circle_radius)
    a = np.arange(2 * R, dtype=np.int64) - R
    return (a[:, None] ** 2 + a[None, :] ** 2) <= R * R


def _check_records(pool_bytes, records, S, R):
    records = [r if isinstance(r, ImageRecord) else ImageRecord(*r) for r in records]
    if not records:
        raise ValueError('no records')
    nc = len(records[0].starts)
    for r in records:
        if min(int(r.h), int(r.w)) != S:
            raise ValueError('image of %d x %d: min(h, w) must equal img_size %d (resize it first: ImageGraphLoader(rescale=True) or '
                             'preprocessing.resize_u8)' % (r.h, r.w, S))
        if int(r.offset) < 0 or int(r.offset) + int(r.h) * int(r.w) * 3 > pool_bytes:
            raise ValueError('image at offset %d (%d x %d x 3 bytes) lies outside the pool of %d bytes' % (r.offset, r.h, r.w, pool_bytes))
        if int(r.k) not in (0, 1, 2, 3):
            raise ValueError('rotation k must be 0..3')
        if len(r.starts) != nc:
            raise ValueError('every record of a batch needs the same number of circles')
        for a, b in r.starts:
            if not (0 <= int(a) and int(a) + 2 * R <= S and 0 <= int(b) and int(b) + 2 * R <= S):
                raise ValueError('circle window at (%d, %d) of side %d lies outside the %d x %d image' % (a, b, 2 * R, S, S))
    return records, nc


def _build_samples_cpu(pool, records, S, R):
    circle = circle_template(R)
    colors, masks = [], []
    raw = pool.numpy()
    for r in records:
        img = raw[r.offset:r.offset + r.h * r.w * 3].reshape(r.h, r.w, 3)
        img = img.astype(np.float32) * np.float32(1.0 / 255.0)                   # img_as_float32
        img = img * np.float32(2.0) - np.float32(1.0)
        h0, w0 = int((r.h - S) / 2), int((r.w - S) / 2)
        img = img[h0:h0 + S, w0:w0 + S, :]
        img = np.rot90(img, int(r.k), axes=(0, 1))
        if r.flip:
            img = np.flip(img, axis=1)
        m = np.zeros((S, S), dtype=bool)
        for a, b in r.starts:
            m[a:a + 2 * R, b:b + 2 * R] |= circle
        colors.append(torch.from_numpy(np.ascontiguousarray(img)).reshape(-1, 3))
        masks.append(torch.from_numpy(m).reshape(-1, 1))
    color, mask = torch.cat(colors), torch.cat(masks)
    return torch.cat([color * ~mask, mask.float()], dim=-1), color, mask


def _pack_records(records, nc):
    """int64 [B, HEAD + 2 nc] host array in the layout of stin_image_samples_u8."""
    rows = [[int(r.offset), int(r.h), int(r.w), int(r.k), int(bool(r.flip))] + [int(v) for ab in r.starts for v in ab] for r in records]
    return np.asarray(rows, dtype=np.int64).reshape(len(records), 5 + 2 * nc)


def build_samples(pool, records, img_size, circle_radius):
    """x [B S S, 4] f32, color [B S S, 3] f32, mask [B S S, 1] bool of the items `records` (ImageRecord or the same tuples) whose raw
    uint8 images lie in `pool` (1-D uint8 tensor).  A GPU pool: the records travel in one non-blocking copy from pinned memory, ONE
    launch builds the batch, nothing synchronises.  ValueError: min(h, w) != img_size (Rescale happens before: ImageGraphLoader(rescale=True)), an image outside the
    pool, a circle window outside the image (the reference would fail with a shape mismatch, or wrap a negative index)."""
    S, R = int(img_size), int(circle_radius)
    if pool.dtype != torch.uint8 or pool.dim() != 1 or not pool.is_contiguous():
        raise TypeError('pool must be a contiguous 1-D uint8 tensor')
    records, nc = _check_records(pool.numel(), records, S, R)
    if not pool.is_cuda:
        return _build_samples_cpu(pool, records, S, R)
    from . import _lib
    from . import functional as SF
    from .plan import _ptr, _stream
    if _lib.CONSTANTS['STIN_IMAGE_RECORD_HEAD'] != 5:
        raise _lib.StinError('record layout of stin_image_samples_u8 changed')
    B, n = len(records), len(records) * S * S
    host = torch.empty(B, 5 + 2 * nc, dtype=torch.int64, pin_memory=True)
    host.numpy()[...] = _pack_records(records, nc)
    dev = pool.device
    rec = host.to(dev, non_blocking=True)
    x = torch.empty(n, 4, dtype=torch.float32, device=dev)
    color = torch.empty(n, 3, dtype=torch.float32, device=dev)
    mask = torch.empty(n, 1, dtype=torch.bool, device=dev)
    with torch.cuda.device(dev):
        SF._call('stin_image_samples_u8', _ptr(pool), pool.numel(), _ptr(rec), B, S, R, nc, _ptr(x), _ptr(color), _ptr(mask), _stream(x))
    return x, color, mask


class ImageGraphLoader:
    """Epochs of image-graph batches, resident on `device`: ``for sample in loader.epoch(e): loss = step(sample)``.

    images: list of uint8 H x W x 3 arrays with min(H, W) == img_size, uploaded once into one byte pool.  rescale=True is the
    reference's Rescale(img_size, img_size): an image with min(H, W) > img_size is area-resized to rescale_size(H, W, img_size) on
    the device, all images in one launch into the resident pool (an image of the right size is copied, a smaller one is a
    ValueError); the default keeps refusing every other size.  The graph tensors and
    the GraphPlan built from them are made once per distinct batch size (the last batch of an epoch may be smaller) and shared by
    every batch of that size through `_plan_cache`, the way loader.SceneLoader keeps a scene's plan resident.  Sharding over ranks:
    loader.shard_indices.  An item's rotation, flip and circle positions come from generators seeded by (seed, epoch, item index)
    alone (augment.item_generator): the same (seed, epoch) gives the same batches whatever the batch size, rank count or order.
    Per batch: one small non-blocking copy of the records, one kernel launch, no host synchronisation."""

    def __init__(self, images, device, img_size, end_level, batch_size, circle_radius, crop_half_width, num_circles=4, is_train=True,
                 random_mask=False, random_augmentation=False, shuffle=True, seed=0, rank=0, world_size=1, model=None, rescale=False):
        self.device = torch.device(device)
        # model (optional): the network the batches are for - the resident plan takes its instance-norm convention
        # (compat_linspace_norm) from it, as surfacetextureinpaintingnet.build_plan does; None = the network's default
        self.linspace_quirk = bool(getattr(model, 'compat_linspace_norm', True))
        self.img_size, self.end_level, self.batch_size = _check_levels(img_size, end_level, batch_size)
        self.circle_radius, self.crop_half_width, self.num_circles = int(circle_radius), crop_half_width, int(num_circles)
        self.is_train, self.random_mask, self.random_augmentation = bool(is_train), bool(random_mask), bool(random_augmentation)
        self.shuffle, self.seed, self.rank, self.world_size = bool(shuffle), int(seed), int(rank), int(world_size)
        self.items, parts, jobs, at, raw_at = [], [], [], 0, 0
        for img in images:
            img = np.ascontiguousarray(img)
            if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
                raise TypeError('images must be uint8 arrays of shape H x W x 3')
            H, W = int(img.shape[0]), int(img.shape[1])
            h, w = H, W
            if rescale and min(H, W) > self.img_size:
                h, w = rescale_size(H, W, self.img_size)
            if min(h, w) != self.img_size:
                raise ValueError('image of %d x %d: min(h, w) must %s img_size %d%s' % (
                    H, W, 'be at least' if rescale else 'equal', self.img_size,
                    '' if rescale else ' (rescale=True resizes larger images as the reference\'s Rescale does)'))
            self.items.append((at, h, w))
            jobs.append((raw_at, H, W, at, h, w))
            parts.append(img.reshape(-1))
            at += h * w * 3
            raw_at += img.size
        if not self.items:
            raise ValueError('no images')
        self.pool = torch.from_numpy(np.concatenate(parts)).to(self.device)
        if rescale and at != raw_at:
            # one launch over every image (those of the right size are copied: equal sizes are the identity); the raw upload is
            # released when this returns
            from . import preprocessing
            self.pool = preprocessing.resize_pool_u8(self.pool, jobs, at, channels=3, mode='area')
        self._graphs = {}                                    # batch size -> (graph tensors, host num_vertices, GraphPlan or None)

    def __len__(self):
        return len(self.items)

    def steps_per_epoch(self):
        n = len(shard_indices(len(self.items), 0, self.seed, False, self.rank, self.world_size))
        return (n + self.batch_size - 1) // self.batch_size

    def params_for(self, epoch, index):
        """(k, flip, starts) of item `index` in `epoch`: independent of ranks and batching."""
        g = augment.item_generator(self.seed, epoch, index)
        s, t = (int(v) for v in torch.randint(0, 1 << 32, (2,), generator=g))
        return draw_image_params(random.Random(s), np.random.RandomState(t), self.img_size, self.crop_half_width, self.circle_radius,
                                 self.num_circles, self.is_train, self.random_mask, self.random_augmentation)

    def records_for(self, epoch, ids):
        return [ImageRecord(*self.items[i], *self.params_for(epoch, i)) for i in ids]

    def batch_ids(self, epoch):
        idx = shard_indices(len(self.items), epoch, self.seed, self.shuffle, self.rank, self.world_size)
        return [idx[b:b + self.batch_size] for b in range(0, len(idx), self.batch_size)]

    def _graph(self, B):
        ent = self._graphs.get(B)
        if ent is None:
            tensors = grid_levels(self.img_size, self.end_level, B, self.device)
            nv_host = torch.tensor([[(self.img_size // 2 ** l) ** 2 for l in range(self.end_level)]] * B, dtype=torch.int32)
            ent = self._graphs[B] = [tensors, nv_host, None]
        return ent

    def batch(self, epoch, ids):
        """The HierarchicalBatch of the items `ids` in `epoch` (reference keys: x, color, mask, edge_index, hierarchy_*, num_vertices, batch)."""
        x, color, mask = build_samples(self.pool, self.records_for(epoch, ids), self.img_size, self.circle_radius)
        ent = self._graph(len(ids))
        out = HierarchicalBatch(x=x, color=color, mask=mask, **ent[0])
        out._nv_host = ent[1]
        if self.device.type == 'cuda':
            if ent[2] is None:
                from .plan import GraphPlan
                # (validate=False: the indices were generated in range by stin_grid_levels_i64 - no flag read-back, no host sync)
                ent[2] = GraphPlan(out, linspace_quirk=self.linspace_quirk, validate=False)
            ent[2]._sample = out                             # the index tensors are the same objects for every batch of this size
            out._plan_cache = ent[2]
        return out

    def epoch(self, epoch=0):
        for ids in self.batch_ids(epoch):
            yield self.batch(int(epoch), ids)
