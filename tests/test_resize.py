"""Image resize on the CPU: the numpy restatement of the contract (tests/_resize_oracle.py, written from include/stin_hip.h) against
independent references - torch's fp64 bilinear and area interpolation, a restatement of the area average by pixel replication,
typed-out cases - and the package's CPU paths against that restatement: resize_u8 / resize_pool_u8, imagegraph.rescale_size,
ImageGraphLoader(rescale=True), scene_io.scan_frame_files / read_frames."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _resize_oracle as RO
from surface_texture_inpainting_net_amd import _lib, imagegraph as IG, preprocessing as P, scene_io

LINEAR_SHAPES = [(968, 1296, 480, 640), (37, 53, 16, 21), (5, 7, 11, 13), (3, 2, 1, 1), (1, 1, 4, 4), (97, 131, 96, 64)]
AREA_SHAPES = [(37, 53, 16, 21), (100, 151, 32, 48), (64, 96, 16, 24), (9, 9, 1, 1)]
# |out - exact bilinear| <= 0.5 (the one rounding) + 255 (2^-12 + 2^-12 + 2^-24) (each coefficient is within 2^-12 of the exact one)
LINEAR_BOUND = 0.625
assert 0.5 + 255 * (2.0 ** -12 + 2.0 ** -12 + 2.0 ** -24) < LINEAR_BOUND


@functools.lru_cache(maxsize=None)
def image(H, W, C=3, seed=0):
    img = np.random.default_rng(1000 * seed + 7 * H + W + C).integers(0, 256, (H, W, C), dtype=np.uint8)
    img.setflags(write=False)
    return img


def torch_resize(img, h, w, mode):
    x = torch.from_numpy(np.array(img)).permute(2, 0, 1)[None].double()
    kw = dict(align_corners=False) if mode == 'bilinear' else {}
    return F.interpolate(x, size=(h, w), mode=mode, **kw)[0].permute(1, 2, 0).numpy()


# ------------------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize('H,W,h,w', LINEAR_SHAPES)
def test_oracle_linear_is_within_the_derived_bound_of_fp64_bilinear(H, W, h, w):
    img = image(H, W)
    err = float(np.abs(RO.linear(img, h, w).astype(np.float64) - torch_resize(img, h, w, 'bilinear')).max())
    print('linear %d x %d -> %d x %d: max |oracle - fp64 bilinear| = %.4f' % (H, W, h, w, err))
    assert err < LINEAR_BOUND


@pytest.mark.parametrize('C', [1, 3, 4])
def test_oracle_equal_sizes_are_the_identity(C):
    for H, W in ((1, 1), (5, 7), (37, 53)):
        img = image(H, W, C)
        assert RO.linear(img, H, W).tobytes() == img.tobytes()
        assert RO.area(img, H, W).tobytes() == img.tobytes()


def area_by_replication(img, h, w):
    """Every source pixel h times down and w times across: the H x W blocks of that image are the output cells, exactly."""
    H, W, C = img.shape
    big = np.repeat(np.repeat(img.astype(np.int64), h, axis=0), w, axis=1)               # [H h, W w, C]
    S = big.reshape(h, H, w, W, C).sum(axis=(1, 3))
    return ((2 * S + W * H) // (2 * W * H)).astype(np.uint8)


@pytest.mark.parametrize('H,W,h,w', AREA_SHAPES)
def test_oracle_area_equals_the_replication_form(H, W, h, w):
    img = image(H, W)
    assert RO.area(img, h, w).tobytes() == area_by_replication(img, h, w).tobytes()


@pytest.mark.parametrize('H,W,h,w', [(64, 96, 16, 24), (64, 96, 32, 32), (9, 9, 1, 1), (30, 20, 10, 10)])
def test_oracle_area_at_integer_factors_is_torchs_area_mode(H, W, h, w):
    img = image(H, W)
    assert np.abs(RO.area(img, h, w).astype(np.float64) - torch_resize(img, h, w, 'area')).max() <= 0.5


def test_oracle_typed_out_cases():
    two = np.array([[[1], [2]], [[3], [4]]], dtype=np.uint8)                             # mean 2.5: the tie rounds up
    assert RO.area(two, 1, 1).tolist() == [[[3]]]
    assert RO.area(np.array([[[0], [1]], [[1], [0]]], dtype=np.uint8), 1, 1).tolist() == [[[1]]]          # 0.5 -> 1
    assert RO.area(np.array([[[0], [0]], [[1], [0]]], dtype=np.uint8), 1, 1).tolist() == [[[0]]]          # 0.25 -> 0
    ramp = (np.arange(6, dtype=np.uint8) * 10).reshape(1, 6, 1)                          # 0 10 20 30 40 50
    assert RO.area(ramp, 1, 3).reshape(-1).tolist() == [5, 25, 45]
    assert RO.area(ramp, 1, 4).reshape(-1).tolist() == [3, 17, 33, 47]                   # cells of 1.5 pixels: 5 / 1.5, 25 / 1.5, 50 / 1.5, 70 / 1.5
    assert RO.linear(ramp, 1, 3).reshape(-1).tolist() == [5, 25, 45]                     # centres at 0.5, 2.5, 4.5
    # enlarging by two: centres at -0.25 (clamped to the first pixel), 0.25, 0.75, ...: 0, 2.5 -> 3 (halves up), 7.5 -> 8, ...
    assert RO.linear(ramp, 1, 12).reshape(-1).tolist() == [0, 3, 8, 13, 18, 23, 28, 33, 38, 43, 48, 50]
    s, t, a, b = RO.linear_axis(4, 2)                                                    # centres at 0.5 and 2.5
    assert s.tolist() == [0, 2] and t.tolist() == [1, 3] and a.tolist() == [1024, 1024] and b.tolist() == [1024, 1024]
    s, t, a, b = RO.linear_axis(2, 4)                                                    # centres at -0.25, 0.25, 0.75, 1.25
    assert s.tolist() == [0, 0, 0, 1] and b.tolist() == [0, 512, 1536, 0] and t.tolist() == [1, 1, 1, 1]


# ---------------------------------------------------------------------------------------------------- the package's CPU paths
@pytest.mark.parametrize('H,W,h,w,C', [s + (C,) for s in LINEAR_SHAPES + [(97, 131, 24, 17), (200, 3, 3, 3), (3, 200, 3, 3)]
                                       for C in (1, 3, 4) if C == 3 or s[0] * s[1] < 100000])          # the frame shape once
def test_cpu_path_equals_the_oracle(H, W, h, w, C):
    img = image(H, W, C)
    got = P.resize_u8(torch.from_numpy(np.array(img)), (h, w), 'linear')
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, C)
    assert got.numpy().tobytes() == RO.linear(img, h, w).tobytes()
    if h <= H and w <= W:
        assert P.resize_u8(torch.from_numpy(np.array(img)), (h, w), 'area').numpy().tobytes() == RO.area(img, h, w).tobytes()


@pytest.mark.parametrize('H,W,h,w', AREA_SHAPES)
def test_cpu_area_path_equals_the_oracle_batched(H, W, h, w):
    imgs = np.stack([image(H, W, 3, seed) for seed in (0, 1)])
    got = P.resize_u8(torch.from_numpy(imgs), (h, w), mode='area')
    assert tuple(got.shape) == (2, h, w, 3)
    for b in range(2):
        assert got[b].numpy().tobytes() == RO.area(imgs[b], h, w).tobytes()


def test_cpu_pool_is_ragged_and_leaves_other_bytes_alone():
    shapes = [(7, 9, 3, 4), (12, 5, 12, 5), (20, 31, 6, 11)]
    parts, jobs, at, out_at = [np.full(3, 9, np.uint8)], [], 3, 5
    for i, (H, W, h, w) in enumerate(shapes):
        parts.append(image(H, W, 3, i).reshape(-1))
        jobs.append((at, H, W, out_at, h, w))
        at += H * W * 3
        out_at += h * w * 3 + 7
    pool = torch.from_numpy(np.concatenate(parts))
    out = torch.full((out_at,), 0xA5, dtype=torch.uint8)
    got = P.resize_pool_u8(pool, jobs, out_at, channels=3, mode='area', out=out)
    assert got is out
    want = np.full(out_at, 0xA5, dtype=np.uint8)
    for i, (so, H, W, do, h, w) in enumerate(jobs):
        want[do:do + h * w * 3] = RO.area(image(H, W, 3, i), h, w).reshape(-1)
    assert out.numpy().tobytes() == want.tobytes()
    fresh = P.resize_pool_u8(pool, jobs, out_at, channels=3, mode='area')             # without `out`: zeros where no job writes
    covered = np.zeros(out_at, dtype=bool)
    for so, H, W, do, h, w in jobs:
        covered[do:do + h * w * 3] = True
    assert fresh.numpy().tobytes() == np.where(covered, want, 0).astype(np.uint8).tobytes()


def test_resize_u8_errors():
    img = torch.zeros(4, 6, 3, dtype=torch.uint8)
    top = _lib.CONSTANTS['STIN_RESIZE_MAX_SIDE']
    assert top == 16384
    with pytest.raises(TypeError):
        P.resize_u8(img.float(), (2, 3))
    with pytest.raises(TypeError):
        P.resize_u8(img.numpy(), (2, 3))
    with pytest.raises(ValueError):
        P.resize_u8(img[0], (2, 3))                                                      # rank 2
    with pytest.raises(ValueError):
        P.resize_u8(torch.zeros(4, 6, 2, dtype=torch.uint8), (2, 3))                     # C = 2
    with pytest.raises(ValueError):
        P.resize_u8(img, (0, 3))
    with pytest.raises(ValueError):
        P.resize_u8(torch.zeros(0, 6, 3, dtype=torch.uint8), (2, 3))                     # an empty source side
    with pytest.raises(ValueError):
        P.resize_u8(img, (2, top + 1))
    with pytest.raises(ValueError):
        P.resize_u8(img, (5, 6), mode='area')                                            # AREA does not enlarge
    with pytest.raises(ValueError):
        P.resize_u8(img, (2, 3), mode='cubic')
    with pytest.raises(ValueError):
        P.resize_u8(img, (2, 3, 4))
    with pytest.raises(ValueError):
        P.resize_pool_u8(img.view(-1), [(0, 4, 6, 0, 2, 3)], 17, channels=3)             # result outside the output bytes
    with pytest.raises(ValueError):
        P.resize_pool_u8(img.view(-1), [(1, 4, 6, 0, 2, 3)], 18, channels=3)             # image outside the pool
    assert tuple(P.resize_u8(torch.zeros(0, 4, 6, 3, dtype=torch.uint8), (2, 3)).shape) == (0, 2, 3, 3)
    assert tuple(P.resize_u8(img, (5, 6), mode='linear').shape) == (5, 6, 3)


def reference_rescale_size(h, w, output_size):
    if h > w:
        new_h, new_w = output_size * h / w, output_size
    else:
        new_h, new_w = output_size, output_size * w / h
    return int(new_h), int(new_w)


@pytest.mark.parametrize('h,w,S,want', [(968, 1296, 256, (256, 342)), (1296, 968, 256, (342, 256)), (512, 512, 128, (128, 128)),
                                        (100, 151, 32, (32, 48)), (151, 100, 32, (48, 32)), (37, 53, 16, (16, 22)),
                                        (480, 640, 96, (96, 128)), (30, 16, 16, (30, 16)), (7, 3, 3, (7, 3)), (3, 7, 2, (2, 4))])
def test_rescale_size_is_the_references_expression(h, w, S, want):
    assert IG.rescale_size(h, w, S) == reference_rescale_size(h, w, S) == want


LOADER_KW = dict(img_size=16, end_level=3, batch_size=2, circle_radius=2, crop_half_width=2, random_mask=True,
                 random_augmentation=True, seed=11)
LOADER_SHAPES = [(16, 21), (37, 53), (16, 16), (64, 40), (33, 17)]


def loader_images():
    return [np.array(image(h, w, 3, i)) for i, (h, w) in enumerate(LOADER_SHAPES)]


def test_loader_rescale_on_the_cpu_pool_is_the_oracles():
    images = loader_images()
    with pytest.raises(ValueError):
        IG.ImageGraphLoader(images, 'cpu', **LOADER_KW)                                  # the default keeps refusing
    with pytest.raises(ValueError):
        IG.ImageGraphLoader(images, 'cpu', rescale=False, **LOADER_KW)
    ld = IG.ImageGraphLoader(images, 'cpu', rescale=True, **LOADER_KW)
    want, at = [], 0
    for img, (offset, h, w) in zip(images, ld.items):
        assert (h, w) == (IG.rescale_size(*img.shape[:2], 16) if min(img.shape[:2]) > 16 else img.shape[:2]) and offset == at
        want.append(RO.area(img, h, w).reshape(-1))
        at += h * w * 3
    assert [(h, w) for _, h, w in ld.items] == [(16, 21), (16, 22), (16, 16), (25, 16), (31, 16)]
    assert ld.pool.numpy().tobytes() == np.concatenate(want).tobytes()
    assert ld.pool[:16 * 21 * 3].numpy().tobytes() == images[0].tobytes()                # the right size: copied
    batches = list(ld.epoch(0))
    assert sum(int(b.num_vertices.shape[0]) for b in batches) == 5
    with pytest.raises(ValueError):
        IG.ImageGraphLoader(images + [np.zeros((15, 40, 3), np.uint8)], 'cpu', rescale=True, **LOADER_KW)     # too small to rescale
    same = [np.array(image(16, 16 + i, 3, i)) for i in range(3)]
    a, b = IG.ImageGraphLoader(same, 'cpu', **LOADER_KW), IG.ImageGraphLoader(same, 'cpu', rescale=True, **LOADER_KW)
    assert a.items == b.items and torch.equal(a.pool, b.pool)


# ------------------------------------------------------------------------------------------------------------------ scan files
def test_scan_frame_files_are_in_natural_order(tmp_path):
    for kind, ext in (('color', '.jpg'), ('depth', '.png'), ('pose', '.txt')):
        os.makedirs(tmp_path / kind)
        for name in ('10', '2', '1', '100', '20'):
            (tmp_path / kind / (name + ext)).write_bytes(b'')
        (tmp_path / kind / 'notes.md').write_bytes(b'')
    (tmp_path / 'color' / '3.png').write_bytes(b'')                                    # another extension: not a colour frame
    files = scene_io.scan_frame_files(str(tmp_path))
    assert sorted(files) == ['color', 'depth', 'pose']
    for kind, ext in (('color', '.jpg'), ('depth', '.png'), ('pose', '.txt')):
        assert [os.path.basename(f) for f in files[kind]] == [n + ext for n in ('1', '2', '10', '20', '100')]
        assert all(os.path.dirname(f) == str(tmp_path / kind) for f in files[kind])
    os.makedirs(tmp_path / 'b' / 'color'), os.makedirs(tmp_path / 'b' / 'depth'), os.makedirs(tmp_path / 'b' / 'pose')
    for name in ('frame-000010.color.jpg', 'frame-9.color.jpg', 'frame-000002.color.jpg'):
        (tmp_path / 'b' / 'color' / name).write_bytes(b'')
    assert [os.path.basename(f) for f in scene_io.scan_frame_files(tmp_path / 'b')['color']] == \
        ['frame-000002.color.jpg', 'frame-9.color.jpg', 'frame-000010.color.jpg']


def test_read_frames_reads_back_what_pillow_wrote(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(5)
    depth = rng.integers(0, 65536, (3, 12, 16)).astype(np.uint16)
    depth[0, 0, :4] = 65535
    depth[2, 5, 5] = 65535
    smooth = np.stack([np.add.outer(np.arange(24) * 5, np.arange(32) * 3) % 256] * 3, axis=2).astype(np.uint8)
    smooth[..., 1] = 255 - smooth[..., 0]
    smooth[..., 2] = 40
    color_files, depth_files = [], []
    for i in range(3):
        color_files.append(str(tmp_path / ('%d.jpg' % i)))
        Image.fromarray(np.roll(smooth, 3 * i, axis=1)).save(color_files[-1], quality=95)
        depth_files.append(str(tmp_path / ('%d.png' % i)))
        Image.fromarray(depth[i]).save(depth_files[-1])
    color, got = scene_io.read_frames(color_files, depth_files)
    assert color.dtype == np.uint8 and color.shape == (3, 24, 32, 3) and got.dtype == np.uint16 and got.shape == (3, 12, 16)
    assert got.tobytes() == np.where(depth == 65535, 0, depth).astype(np.uint16).tobytes()
    for i in range(3):                                                                   # JPEG is lossy; the decoder is Pillow's own
        with Image.open(color_files[i]) as im:
            assert color[i].tobytes() == np.asarray(im.convert('RGB')).tobytes()
        assert np.abs(color[i].astype(int) - np.roll(smooth, 3 * i, axis=1)).mean() < 8  # RGB order, right frame
    Image.fromarray(smooth[:10]).save(str(tmp_path / 'short.jpg'))
    with pytest.raises(ValueError):
        scene_io.read_frames(color_files + [str(tmp_path / 'short.jpg')], depth_files)
