"""View metrics on the GPU (csrc/stin_view_metrics.hip through views.view_metrics): the int64 table equals the numpy restatement of
the contract (tests/_viewmetrics_oracle.py) byte for byte - at image sizes on both sides of every tile edge, with 1, 3 and 4
channels, images that start at an odd byte of a larger buffer, masks with holes, empty masks, no masks, extreme images - and the
derived figures equal the oracle's; result_view_metrics on the rendered icosphere."""
import functools

import numpy as np
import pytest
import torch

import _render_oracle as RO
import _viewmetrics_oracle as VO
from surface_texture_inpainting_net_amd import views

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

SIZES = [(10, 10), (11, 11), (12, 23), (33, 97), (45, 70)]               # no window; one; a strip; across the 16 x 32 tile both ways


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def images(seed, P, H, W, K):
    """Two noisy images that agree in places (so that windows of every quality occur) with masks: `covered` has holes, one pose
    none at all; `region` is random, empty for one pose."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=(P, H, W, K), dtype=np.uint8)
    b = np.where(rng.random((P, H, W, 1)) < 0.5, a, rng.integers(0, 256, size=(P, H, W, K))).astype(np.uint8)
    cov = (rng.random((P, H, W)) < 0.995).astype(np.uint8) * rng.integers(1, 256, size=(P, H, W)).astype(np.uint8)
    reg = (rng.random((P, H, W)) < 0.6).astype(np.uint8)
    if P > 1:
        cov[1] = 0
        reg[P - 1] = 0
    return a, b, cov, reg


def same(got, want):
    assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == want.shape
    assert got.cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize('P', [1, 5])
@pytest.mark.parametrize('K', [1, 3, 4])
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_table_equals_the_oracle(size, K, P):
    H, W = size
    a, b, cov, reg = images(100 * H + 10 * K + P, P, H, W, K)
    for c, r in ((cov, reg), (None, None), (cov, None), (None, reg)):
        want = VO.table(a, b, c, r)
        got = views.view_metrics(dev(a), dev(b), dev(c), dev(r))
        same(got.table, want)
        d = VO.derived(want, K)
        for key in ('l1', 'mse', 'ssim'):                                 # one fp64 division each: the same bits
            assert np.array_equal(getattr(got, key).cpu().numpy(), d[key], equal_nan=True), key
        np.testing.assert_allclose(got.psnr.cpu().numpy(), d['psnr'], rtol=1e-14, equal_nan=True)    # (two log10 routines: an ulp)
    full = VO.table(a, b, None, None)
    assert full[:, 0].tolist() == [H * W] * P and full[:, 3].tolist() == [max(H - 10, 0) * max(W - 10, 0)] * P
    if H >= 33 and P > 1:                                                 # the masks took windows away, and whole poses
        masked = VO.table(a, b, cov, reg)
        assert 0 < masked[0, 3] < full[0, 3] and masked[1].tolist() == [0] * 5 and masked[P - 1].tolist() == [0] * 5


@pytest.mark.parametrize('K', [1, 3, 4])
@pytest.mark.parametrize('shift', [1, 7, 16])
def test_images_and_masks_inside_a_larger_buffer_at_an_odd_byte(K, shift):
    P, H, W = 2, 33, 45
    a, b, cov, reg = images(7 + K, P, H, W, K)
    want = VO.table(a, b, cov, reg)

    def inside(x, fill):
        buf = torch.full((shift + x.size + 5,), fill, dtype=torch.uint8, device=DEV)
        buf[shift:shift + x.size] = dev(x.reshape(-1))
        view = buf[shift:shift + x.size].view(x.shape)
        assert view.data_ptr() % 16 == shift % 16 and view.is_contiguous()
        return view
    got = views.view_metrics(inside(a, 3), inside(b, 250), inside(cov, 1), inside(reg, 1))
    same(got.table, want)
    same(views.view_metrics(inside(a, 3), dev(b), None, inside(reg, 1)).table, VO.table(a, b, None, reg))


def test_masks_may_be_bool_or_int32_and_images_may_have_no_channel_axis():
    a, b, cov, reg = images(11, 3, 20, 40, 1)
    want = VO.table(a, b, cov, reg)
    same(views.view_metrics(dev(a)[..., 0], dev(b)[..., 0], dev(cov) != 0, dev(reg).to(torch.int32) * -5).table, want)
    face_ids = torch.where(dev(cov) != 0, 7, -1).to(torch.int32)          # what RenderResult.face_ids >= 0 hands over
    same(views.view_metrics(dev(a), dev(b), face_ids >= 0, dev(reg)).table, want)
    with pytest.raises(ValueError):
        views.view_metrics(dev(a), dev(b)[:, :, :39])
    with pytest.raises(ValueError):
        views.view_metrics(dev(a), dev(b), dev(cov)[:2])
    with pytest.raises(ValueError):
        views.view_metrics(torch.zeros(1, 12, 12, 5, dtype=torch.uint8, device=DEV), torch.zeros(1, 12, 12, 5, dtype=torch.uint8, device=DEV))
    with pytest.raises(TypeError):
        views.view_metrics(dev(a).float(), dev(b).float())
    with pytest.raises(TypeError):
        views.view_metrics(dev(a), dev(b), covered=torch.ones(3, 20, 40, dtype=torch.uint8))
    none = views.view_metrics(torch.zeros(0, 20, 40, 3, dtype=torch.uint8, device=DEV), torch.zeros(0, 20, 40, 3, dtype=torch.uint8, device=DEV))
    assert tuple(none.table.shape) == (0, 5) and tuple(none.ssim.shape) == (0,)


def test_extreme_images_and_an_image_against_itself():
    H, W = 33, 40
    y, x = np.mgrid[0:H, 0:W]
    zero, full = np.zeros((1, H, W, 3), dtype=np.uint8), np.full((1, H, W, 3), 255, dtype=np.uint8)
    board = np.broadcast_to((((y + x) % 2) * 255).astype(np.uint8)[None, :, :, None], (1, H, W, 3)).copy()
    for a, b in ((zero, zero), (full, full), (zero, full), (full, zero), (board, 255 - board), (board, zero), (board, full), (board, board)):
        same(views.view_metrics(dev(a), dev(b)).table, VO.table(a, b))
    got = views.view_metrics(dev(zero), dev(full))
    assert got.psnr.tolist() == [0.0] and got.l1.tolist() == [1.0] and got.ssim.tolist()[0] == pytest.approx(9.999005e-5, rel=1e-6)
    assert views.view_metrics(dev(board), dev(255 - board)).ssim.tolist()[0] < 0       # anti-correlated
    t = dev(images(5, 2, H, W, 3)[0])
    me = views.view_metrics(t, t)                                         # a is b
    assert me.table.tolist() == [[H * W, 0, 0, 23 * 30, 3 * 23 * 30 * (1 << 32)]] * 2
    assert me.ssim.tolist() == [1.0, 1.0] and me.psnr.tolist() == [float('inf')] * 2 and me.mse.tolist() == [0.0, 0.0]


def test_the_same_call_twice_gives_the_same_bytes():
    a, b, cov, reg = (dev(t) for t in images(3, 5, 45, 70, 3))
    first = views.view_metrics(a, b, cov, reg).table.cpu().numpy().tobytes()
    for _ in range(3):
        assert views.view_metrics(a, b, cov, reg).table.cpu().numpy().tobytes() == first


# ------------------------------------------------------------------------------------------------------- the rendered icosphere
CAM, H, W = (60.0, 58.2, 64 / 2 - 0.5, 48 / 2 - 0.5), 48, 64


@functools.lru_cache(maxsize=None)
def sphere():
    V, F = RO.icosphere(2, 3, jitter=0.0)
    V = V / np.linalg.norm(V, axis=1, keepdims=True)
    rng = np.random.default_rng(0)
    gt = (0.8 * V).astype(np.float32)                                     # colours in [-1, 1]
    pred = np.clip(gt + 0.3 * rng.standard_normal(gt.shape), -1, 1).astype(np.float32)
    mask = (V[:, 2] > 0).astype(np.int64)[:, None]                        # one hemisphere is inpainted
    return dev(V), dev(F), dev(pred), dev(gt), dev(mask), RO.orbit(12, 3.0, 0.8)


def test_result_view_metrics_of_equal_colours_is_perfect_wherever_the_sphere_is_seen():
    V, F, pred, gt, mask, poses = sphere()
    m = views.result_view_metrics(V, F, gt, gt, mask, poses, CAM, H, W, region='all')
    assert tuple(m.table.shape) == (12, 5) and m.channels == 3
    assert (m.table[:, 0] > 0).all() and (m.table[:, 3] > 0).all()       # every pose sees it
    assert (m.ssim == 1.0).all() and torch.isposinf(m.psnr).all() and (m.table[:, 1:3] == 0).all()
    assert (m.table[:, 4] == 3 * m.table[:, 3] * (1 << 32)).all()


def test_result_view_metrics_does_not_depend_on_chunk_and_equals_the_oracle_on_the_rendered_images():
    V, F, pred, gt, mask, poses = sphere()
    tables = {region: [views.result_view_metrics(V, F, pred, gt, mask, poses, CAM, H, W, region=region, chunk=chunk).table.cpu().numpy()
                       for chunk in (1, 5, 12)] for region in ('mask', 'all')}
    for region in tables:
        assert all(t.tobytes() == tables[region][0].tobytes() for t in tables[region])
    by_mask, by_all = tables['mask'][0], tables['all'][0]
    assert ((0 < by_mask[:, 0]) & (by_mask[:, 0] < by_all[:, 0])).all()
    assert (by_mask[:, 3] <= by_all[:, 3]).all() and (by_mask[:, 3] < by_all[:, 3]).any()
    colorings = views.result_colorings(pred, gt, mask)
    shown = views.render_mesh(V, F, colorings['pred'], poses, CAM, H, W, face_ids=True)
    truth = views.render_mesh(V, F, colorings['gt'], poses, CAM, H, W)
    where = views.render_mesh(V, F, (mask.reshape(-1) > 0).float(), poses, CAM, H, W)
    host = lambda t: t.cpu().numpy()
    covered = host(shown.face_ids) >= 0
    assert by_all.tobytes() == VO.table(host(shown.color), host(truth), covered, None).tobytes()
    assert by_mask.tobytes() == VO.table(host(shown.color), host(truth), covered, host(where)[..., 0]).tobytes()
    m = views.result_view_metrics(V, F, pred, gt, mask, poses, CAM, H, W, region='all')
    assert (m.ssim > 0.0).all() and (m.ssim < 1.0).all() and (m.psnr > 5.0).all() and (m.psnr < 40.0).all()
    with pytest.raises(ValueError):
        views.result_view_metrics(V, F, pred, gt, mask, poses, CAM, H, W, region='inside')
