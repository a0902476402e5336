"""Image resize on the GPU (csrc/stin_resize.hip through preprocessing.resize_u8 / resize_pool_u8, imagegraph.ImageGraphLoader(rescale=True)
and preprocessing.scan_vertex_colors): byte equality with the numpy restatement of the contract (tests/_resize_oracle.py) for both modes
and every channel count, with sources and results at odd addresses of buffers whose other bytes must keep their sentinel; footprints
larger than any tile, row segments longer than a staged chunk, the 64-bit sums, the frame shape, a ragged pool in one call."""
import functools
import os

import numpy as np
import pytest
import torch

import _frames_oracle as FO
import _observers_oracle as OO
import _resize_oracle as RO
from surface_texture_inpainting_net_amd import imagegraph as IG, preprocessing as P, scene_io

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
ORACLE = {'linear': RO.linear, 'area': RO.area}


@functools.lru_cache(maxsize=None)
def image(H, W, C=3, seed=0):
    img = np.random.default_rng(1000 * seed + 7 * H + W + C).integers(0, 256, (H, W, C), dtype=np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def want(mode, H, W, C, seed, h, w):
    out = ORACLE[mode](image(H, W, C, seed), h, w)
    out.setflags(write=False)
    return out


def run_pool(images, sizes, mode, shift=3):
    """One resize_pool_u8 call on device buffers laid out to be awkward: both buffers start `shift` bytes into their allocations (no
    16-byte alignment anywhere), the first image starts at byte 0 of the pool and the last one ends at its last byte, odd gaps lie
    between the images and between the results, the last result ends at the last output byte.  -> the results, after checking that
    every byte that is not a result - inside the output, before it and behind it - kept the sentinel."""
    C = images[0].shape[2]
    rng = np.random.default_rng(len(images))
    parts, jobs, at, out_at = [], [], 0, 37
    for i, (img, (h, w)) in enumerate(zip(images, sizes)):
        if i:
            gap = rng.integers(0, 256, 5 + 2 * i, dtype=np.uint8)
            parts.append(gap)
            at += gap.size
            out_at += 7 + 2 * i
        parts.append(np.asarray(img).reshape(-1))
        jobs.append((at, img.shape[0], img.shape[1], out_at, h, w))
        at += img.size
        out_at += h * w * C
    pool_all = torch.zeros(shift + at + 64, dtype=torch.uint8, device=DEV)
    pool = pool_all[shift:shift + at]
    pool.copy_(torch.from_numpy(np.concatenate(parts)))
    out_all = torch.full((shift + out_at + 64,), SENTINEL, dtype=torch.uint8, device=DEV)
    out = out_all[shift:shift + out_at]
    assert P.resize_pool_u8(pool, jobs, out_at, channels=C, mode=mode, out=out) is out
    got = out_all.cpu().numpy()
    untouched = np.ones(got.size, dtype=bool)
    results = []
    for so, H, W, do, h, w in jobs:
        results.append(got[shift + do:shift + do + h * w * C].reshape(h, w, C))
        untouched[shift + do:shift + do + h * w * C] = False
    assert (got[untouched] == SENTINEL).all(), 'a byte outside the results was written'
    return results


def check_one(mode, H, W, C, h, w, seed=0):
    got, = run_pool([image(H, W, C, seed)], [(h, w)], mode)
    assert got.tobytes() == want(mode, H, W, C, seed, h, w).tobytes(), (mode, H, W, C, h, w)


# 1 x 1 source, 1 x 1 output, identity, rows of 159 bytes, an integer factor, footprints larger than any tile along either axis
COMMON = [(1, 1, 1, 1), (3, 2, 1, 1), (37, 53, 1, 1), (5, 7, 5, 7), (37, 53, 37, 53), (37, 53, 16, 21), (64, 96, 16, 24), (200, 3, 3, 3),
          (3, 200, 3, 3)]


@pytest.mark.parametrize('C', [1, 3, 4])
@pytest.mark.parametrize('mode', ['linear', 'area'])
def test_both_modes_at_odd_addresses_with_untouched_guards(mode, C):
    for H, W, h, w in COMMON:
        check_one(mode, H, W, C, h, w)


@pytest.mark.parametrize('C', [1, 3, 4])
def test_linear_enlarges_and_skips_pixels(C):
    for H, W, h, w in [(1, 1, 4, 4), (5, 7, 11, 13), (97, 131, 24, 17), (97, 131, 96, 64), (3, 2, 9, 300)]:
        check_one('linear', H, W, C, h, w)


@pytest.mark.parametrize('C', [1, 3, 4])
@pytest.mark.parametrize('mode', ['linear', 'area'])
def test_several_tiles_steps_and_chunks(mode, C):
    """1000 output columns are four column tiles and 19 output rows three row tiles; 40 rows of 4.5 KB are staged in more than one
    step; and a tile whose row segment is longer than the 32 KB that are staged at a time takes it in chunks, with pixels that
    straddle the chunk ends (3 and 4 channels: one channel never has 32 KB in a row)."""
    check_one(mode, 2, 6000, C, 2, 1000)
    check_one(mode, 40, 1500, C, 19, 300)
    if C > 1:
        check_one(mode, 2, 36000 // C, C, 2, 250)


def test_ragged_pool_in_one_call_equals_the_single_image_results():
    shapes = [(37, 53, 16, 21), (64, 96, 16, 24), (9, 9, 1, 1), (16, 16, 16, 16), (100, 151, 32, 48)]
    for mode in ('area', 'linear'):
        images = [image(H, W, 3, i) for i, (H, W, _, _) in enumerate(shapes)]
        together = run_pool(images, [s[2:] for s in shapes], mode)
        for i, ((H, W, h, w), got) in enumerate(zip(shapes, together)):
            alone, = run_pool([images[i]], [(h, w)], mode, shift=1)
            assert got.tobytes() == alone.tobytes() == want(mode, H, W, 3, i, h, w).tobytes(), (mode, i)


def test_area_sums_beyond_32_bits():
    """510 W H > 2^31 at 2100 x 2100: the sums are 64-bit; all-255 must come out as 255."""
    white = np.full((2100, 2100, 3), 255, dtype=np.uint8)
    got = P.resize_u8(torch.from_numpy(white).to(DEV), (3, 3), 'area')
    assert got.cpu().numpy().tobytes() == np.full((3, 3, 3), 255, dtype=np.uint8).tobytes()
    check_one('area', 2100, 2100, 3, 3, 3)


def test_area_on_either_side_of_the_narrow_division():
    """W H = 2^22 is where the final division changes width: one image just below it, one on it."""
    check_one('area', 2047, 2048, 1, 3, 3)
    check_one('area', 2048, 2048, 1, 3, 3)


def test_the_frame_shape():
    frames = np.stack([image(968, 1296, 3, s) for s in (0, 1)])
    dev = torch.from_numpy(frames).to(DEV)
    got = P.resize_u8(dev, (480, 640))
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (2, 480, 640, 3)
    for b in range(2):
        assert got[b].cpu().numpy().tobytes() == want('linear', 968, 1296, 3, b, 480, 640).tobytes()
    alone = P.resize_u8(dev[1], (480, 640), mode='linear')
    assert tuple(alone.shape) == (480, 640, 3) and torch.equal(alone, got[1])


def test_errors_and_empty_batches_on_the_device():
    img = torch.zeros(4, 6, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        P.resize_u8(img, (5, 6), mode='area')
    with pytest.raises(ValueError):
        P.resize_u8(img, (0, 6))
    assert tuple(P.resize_u8(img[None][:0], (2, 3)).shape) == (0, 2, 3, 3)
    assert torch.equal(P.resize_u8(img + 7, (4, 6), 'area'), img + 7)


LOADER_KW = dict(img_size=16, end_level=3, batch_size=2, circle_radius=2, crop_half_width=2, random_mask=True,
                 random_augmentation=True, seed=11)


def test_loader_rescale_on_the_device_equals_the_cpu_loader():
    images = [np.array(image(h, w, 3, i)) for i, (h, w) in enumerate([(16, 21), (37, 53), (16, 16), (64, 40), (33, 17)])]
    with pytest.raises(ValueError):
        IG.ImageGraphLoader(images, DEV, **LOADER_KW)
    cpu = IG.ImageGraphLoader(images, 'cpu', rescale=True, **LOADER_KW)
    ld = IG.ImageGraphLoader(images, DEV, rescale=True, **LOADER_KW)
    assert ld.items == cpu.items and ld.pool.is_cuda and torch.equal(ld.pool.cpu(), cpu.pool)
    ids = ld.batch_ids(0)[0]
    a, b = ld.batch(0, ids), cpu.batch(0, ids)
    for name in ('x', 'color', 'mask'):
        assert torch.equal(getattr(a, name).cpu(), getattr(b, name)), name
    recs = ld.records_for(0, [1, 3, 4])                                                  # the three resized images
    for got, ref in zip(IG.build_samples(ld.pool, recs, 16, 2), IG.build_samples(cpu.pool, recs, 16, 2)):
        assert torch.equal(got.cpu(), ref)


# ------------------------------------------------------------------------------------------------------------- a tiny scan
SCAN_KW = dict(margin=1, half_kernel=1, discontinuity_threshold=10.0, depth_threshold=0.3)


def write_scan(root):
    from PIL import Image
    poses = OO.orbit(3, 2.5, 0.5)
    intrinsic = np.eye(4)
    intrinsic[0, 0], intrinsic[1, 1], intrinsic[0, 2], intrinsic[1, 2] = 12.0, 12.0, 15.0, 12.0       # of the 24 x 32 colour frames
    cam = P.frame_intrinsics(intrinsic, 32, 24, 16, 12)
    assert cam == (6.0, 6.0, 7.5, 5.5)
    depth = FO.render_sphere(poses, 12, 16, cam)
    for kind in ('color', 'depth', 'pose', 'intrinsic'):
        os.makedirs(os.path.join(root, kind))
    np.savetxt(os.path.join(root, 'intrinsic', 'intrinsic_color.txt'), intrinsic)
    ii, jj = np.meshgrid(np.arange(24), np.arange(32), indexing='ij')
    for p, frame in enumerate((8, 9, 10)):                                               # 8 < 9 < 10 only in natural order
        rgb = np.stack([(ii * 9 + 20 * p) % 256, (jj * 7 + 50) % 256, (ii + jj) * 4 % 256], axis=2).astype(np.uint8)
        Image.fromarray(rgb).save(os.path.join(root, 'color', '%d.jpg' % frame), quality=90)
        Image.fromarray(depth[p]).save(os.path.join(root, 'depth', '%d.png' % frame))
        np.savetxt(os.path.join(root, 'pose', '%d.txt' % frame), poses[p])
    return poses, cam


@pytest.mark.parametrize('batch', [1, 3])
def test_scan_vertex_colors_equals_the_same_steps_by_hand(tmp_path, batch):
    pytest.importorskip('PIL')
    root = str(tmp_path / 'scan')
    poses, cam = write_scan(root)
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) / np.sqrt(3.0)
    V = torch.from_numpy(corners).to(DEV)
    colors, count = P.scan_vertex_colors(V, root, width=16, height=12, trajectory_slice=slice(None), batch=batch, **SCAN_KW)
    files = scene_io.scan_frame_files(root)
    assert [os.path.basename(f) for f in files['pose']] == ['8.txt', '9.txt', '10.txt']
    color, depth = scene_io.read_frames(files['color'], files['depth'])
    assert color.shape == (3, 24, 32, 3) and depth.shape == (3, 12, 16)
    small = P.resize_u8(torch.from_numpy(color).to(DEV), (12, 16))
    fc = P.FrameColors(V, cam, **SCAN_KW)
    fc.add(poses, small, torch.from_numpy(depth).to(DEV))
    want_colors, want_count = fc.result()
    assert int(want_count.sum()) > 0, 'the scan colours something'
    assert colors.cpu().numpy().tobytes() == want_colors.cpu().numpy().tobytes() and torch.equal(count, want_count)
    ref = FO.colors(corners, poses, np.stack([RO.linear(c, 12, 16) for c in color]), cam, depth=depth, **SCAN_KW)
    assert colors.cpu().numpy().tobytes() == ref[0].tobytes() and count.cpu().numpy().tobytes() == ref[1].tobytes()
    with pytest.raises(ValueError):
        P.scan_vertex_colors(V, root, width=16, height=13, trajectory_slice=slice(None), **SCAN_KW)      # depth is 12 x 16
    every_other, _ = P.scan_vertex_colors(V, root, width=16, height=12, trajectory_slice=slice(None, None, 2), batch=batch, **SCAN_KW)
    by_hand, _ = P.vertex_colors_from_frames(V, poses[::2], small[::2].contiguous(), torch.from_numpy(depth[::2].copy()).to(DEV),
                                             color_camera=cam, **SCAN_KW)
    assert torch.equal(every_other, by_hand)
