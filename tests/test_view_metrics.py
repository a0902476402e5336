"""View metrics without a GPU: the numpy restatement of the contract (tests/_viewmetrics_oracle.py) held to closed forms - equal
images, constant images, symmetry, pose order, the window count, what one uncovered pixel removes, what `region` selects - its taps
to the rounded Gaussian, its values to a plain float64 Gaussian-weight SSIM written here; the ABI; the derived figures and the JSON
file of write_result_views on a hand-made table."""
import json
import math

import numpy as np
import pytest
import torch

import _viewmetrics_oracle as VO
from surface_texture_inpainting_net_amd import _lib, views

ONE = 1 << 32


def noise(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------------- the taps
def test_taps_are_the_rounded_gaussian_with_the_centre_raised_by_one():
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2.0 * 1.5 ** 2))
    want = np.rint(65536.0 * g / g.sum()).astype(np.int64)
    assert int(want.sum()) == 65535
    want[5] += 1
    assert VO.TAPS.tolist() == want.tolist() == [67, 498, 2359, 7167, 13960, 17434, 13960, 7167, 2359, 498, 67]
    assert int(VO.TAPS.sum()) == 65536 and int(VO.W2.sum()) == ONE
    assert _lib.CONSTANTS['STIN_VIEW_METRICS_WINDOW'] == 11 == VO.WIN
    assert int(VO.TAPS.max()) * 255 * 255 * 11 < 2 ** 63 and 65536 * 65025 < 2 ** 32 and ONE * 65025 < 2 ** 48     # the header's bounds


# --------------------------------------------------------------------------------------------------------------- closed forms
def test_equal_images_have_ssim_one_and_infinite_psnr():
    a = noise(1, (2, 17, 23, 3))
    w = VO.windows(a, a)
    assert w.counted.all() and w.counted.shape == (2, 7, 13) and (w.q == ONE).all()
    t = VO.table(a, a)
    assert t.tolist() == [[17 * 23, 0, 0, 7 * 13, 3 * 7 * 13 * ONE]] * 2
    d = VO.derived(t, 3)
    assert np.isposinf(d['psnr']).all() and (d['ssim'] == 1.0).all() and (d['l1'] == 0.0).all() and (d['mse'] == 0.0).all()


@pytest.mark.parametrize('x,y', [(0, 255), (255, 0), (10, 200), (128, 128), (1, 0)])
def test_constant_images_have_the_closed_form(x, y):
    a, b = np.full((1, 12, 13, 1), x, dtype=np.uint8), np.full((1, 12, 13, 1), y, dtype=np.uint8)
    w = VO.windows(a, b)
    fx, fy = float(x), float(y)
    # every moment is exact (S = 2^32 x: ma = x, va = c = 0), so v is this expression as fp64 evaluates it
    want = ((2.0 * fx * fy + VO.C1) * (2.0 * 0.0 + VO.C2)) / ((fx * fx + fy * fy + VO.C1) * (0.0 + 0.0 + VO.C2))
    assert (w.v == want).all() and w.v.shape == (1, 2, 3, 1)
    assert want == pytest.approx((2 * x * y + VO.C1) / (x * x + y * y + VO.C1), rel=1e-15)
    assert (w.q == int(np.rint(want * ONE))).all()
    if (x, y) == (0, 255):
        assert want == pytest.approx(9.999005e-5, rel=1e-6)
        t = VO.table(a, b)
        assert t[0, :4].tolist() == [156, 156 * 255, 156 * 65025, 6]
        assert VO.derived(t, 1)['psnr'][0] == 0.0 and VO.derived(t, 1)['l1'][0] == 1.0


def test_symmetric_in_the_two_images_and_rows_follow_the_poses():
    a, b = noise(2, (4, 14, 19, 3)), noise(3, (4, 14, 19, 3))
    cov, reg = noise(4, (4, 14, 19)) > 3, noise(5, (4, 14, 19)) > 100
    t = VO.table(a, b, cov, reg)
    assert (t[:, 3] > 0).any() and t.tobytes() == VO.table(b, a, cov, reg).tobytes()
    order = np.array([2, 0, 3, 1])
    assert VO.table(a[order], b[order], cov[order], reg[order]).tobytes() == t[order].tobytes()
    for p in range(4):                                                    # a pose on its own is its row
        assert VO.table(a[p:p + 1], b[p:p + 1], cov[p:p + 1], reg[p:p + 1]).tobytes() == t[p:p + 1].tobytes()


def test_window_counts():
    assert VO.table(noise(6, (1, 11, 11, 3)), noise(7, (1, 11, 11, 3)))[0, 3] == 1
    assert VO.table(noise(6, (1, 10, 30, 3)), noise(7, (1, 10, 30, 3)))[0, [0, 3, 4]].tolist() == [300, 0, 0]
    assert VO.table(noise(6, (1, 30, 10)), noise(7, (1, 30, 10)))[0, [0, 3, 4]].tolist() == [300, 0, 0]
    assert VO.table(noise(6, (1, 12, 23, 4)), noise(7, (1, 12, 23, 4)))[0, 3] == 2 * 13
    assert math.isnan(VO.derived(VO.table(noise(6, (1, 10, 30, 3)), noise(7, (1, 10, 30, 3))), 3)['ssim'][0])


@pytest.mark.parametrize('hole,lost', [((20, 25), 121), ((0, 0), 1), ((3, 25), 4 * 11), ((39, 49), 1), ((20, 47), 11 * 3)])
def test_one_uncovered_pixel_removes_exactly_the_windows_that_contain_it(hole, lost):
    a, b = noise(8, (1, 40, 50, 1)), noise(9, (1, 40, 50, 1))
    cov = np.ones((1, 40, 50), dtype=np.uint8)
    full = VO.windows(a, b)
    cov[0, hole[0], hole[1]] = 0
    w = VO.windows(a, b, cov)
    gone = full.counted & ~w.counted
    assert int(gone.sum()) == lost and not (w.counted & ~full.counted).any()
    ys, xs = np.nonzero(gone[0])                                          # corners (y, x) whose window [y, y + 11) x [x, x + 11) holds the hole
    assert (ys <= hole[0]).all() and (ys + 11 > hole[0]).all() and (xs <= hole[1]).all() and (xs + 11 > hole[1]).all()
    t, t_full = VO.table(a, b, cov), VO.table(a, b)
    assert t[0, 0] == t_full[0, 0] - 1 and t[0, 3] == t_full[0, 3] - lost
    assert t[0, 4] == t_full[0, 4] - int(full.q[gone].sum())


def test_region_selects_windows_by_their_centre_pixel_only():
    a, b = noise(10, (1, 20, 22, 3)), noise(11, (1, 20, 22, 3))
    full = VO.windows(a, b)
    reg = np.zeros((1, 20, 22), dtype=np.uint8)
    reg[0, 9, 12] = 200                                                   # the centre of the window at corner (4, 7)
    t = VO.table(a, b, None, reg)
    d = a[0, 9, 12].astype(np.int64) - b[0, 9, 12].astype(np.int64)
    assert t[0].tolist() == [1, int(np.abs(d).sum()), int((d * d).sum()), 1, int(full.q[0, 4, 7].sum())]
    reg[:] = 1
    reg[0, 9, 12] = 0                                                     # every other window stays, though each one near it contains the pixel
    t = VO.table(a, b, None, reg)
    assert t[0, 3] == 10 * 12 - 1 and t[0, 4] == int(full.q.sum()) - int(full.q[0, 4, 7].sum())
    reg[:] = 0
    reg[0, 2, 2] = 1                                                      # in the region, but no window's centre
    assert VO.table(a, b, None, reg)[0, [0, 3, 4]].tolist() == [1, 0, 0]


# ------------------------------------------------------------------------------------------------------- against float weights
def float_ssim(a, b):
    """SSIM of every 'valid' window with the float64 Gaussian of sigma 1.5, normalised to 1: the textbook form, [H - 10, W - 10]."""
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2.0 * 1.5 ** 2))
    g2 = np.outer(g / g.sum(), g / g.sum())
    H, W = a.shape
    out = np.empty((H - 10, W - 10))
    for y in range(H - 10):
        for x in range(W - 10):
            pa, pb = a[y:y + 11, x:x + 11].astype(np.float64), b[y:y + 11, x:x + 11].astype(np.float64)
            ma, mb = (g2 * pa).sum(), (g2 * pb).sum()
            va, vb, c = (g2 * pa * pa).sum() - ma * ma, (g2 * pb * pb).sum() - mb * mb, (g2 * pa * pb).sum() - ma * mb
            out[y, x] = ((2 * ma * mb + VO.C1) * (2 * c + VO.C2)) / ((ma * ma + mb * mb + VO.C1) * (va + vb + VO.C2))
    return out


def ramp_pair(step_x, step_y, bump):
    y, x = np.mgrid[0:24, 0:29]
    a = np.clip(step_x * x + step_y * y, 0, 255)
    b = np.clip(a + bump * ((x + 2 * y) % 3), 0, 255)
    return a.astype(np.uint8), b.astype(np.uint8)


# measured on these inputs against float_ssim (the test prints both): noise 5.090e-05, ramps 3.068e-06; the bounds are twice that
NOISE_MEASURED, RAMP_MEASURED = 5.090e-5, 3.068e-6


def test_integer_taps_stay_close_to_float_gaussian_weights():
    """The only difference is the rounding of the taps to 2^-16 (and q's to 2^-32): a 2-D weight is off by up to 4e-6, which moves
    a covariance of noise (121 products of about 16 000, signs at random) by a few tenths against variances of about 11 000 -
    measured NOISE_MEASURED on the noise images, RAMP_MEASURED on the ramps.  The bounds are twice the measured maxima: the factor
    covers inputs of the same kind with another seed or slope."""
    worst_noise = 0.0
    for seed in (20, 21, 22):
        a, b = noise(seed, (24, 29)), noise(seed + 100, (24, 29))
        w = VO.windows(a[None], b[None])
        worst_noise = max(worst_noise, float(np.abs(w.v[0, :, :, 0] - float_ssim(a, b)).max()))
        assert np.abs(w.q - w.v * ONE).max() <= 0.5
    worst_ramp = 0.0
    for step_x, step_y, bump in ((8, 1, 1), (3, 7, 2), (9, 9, 1), (1, 2, 3)):
        a, b = ramp_pair(step_x, step_y, bump)
        w = VO.windows(a[None], b[None])
        worst_ramp = max(worst_ramp, float(np.abs(w.v[0, :, :, 0] - float_ssim(a, b)).max()))
    print('integer taps against float weights: noise %.3e, ramps %.3e' % (worst_noise, worst_ramp))
    assert worst_noise <= 2 * NOISE_MEASURED and worst_ramp <= 2 * RAMP_MEASURED


# ------------------------------------------------------------------------------------------------------------------------ ABI
def test_entry_points_are_declared_exported_and_check_their_arguments():
    lib = _lib.load()                                                     # no GPU needed: these calls return before a launch
    C = _lib.CONSTANTS
    assert 'stin_view_metrics_u8' in _lib.SIGNATURES and 'stin_view_metrics_workspace_bytes' in _lib.SIGNATURES
    assert C['STIN_VIEW_METRICS_COLS'] == 5 == len(VO.COLUMNS) == len(views.VIEW_METRICS_COLUMNS) and C['STIN_VERSION'] == 102
    assert tuple(views.VIEW_METRICS_COLUMNS) == VO.COLUMNS
    assert len(_lib.SIGNATURES['stin_view_metrics_u8'][1]) == 12
    assert lib.stin_view_metrics_workspace_bytes(128, 480, 640, 3) >= 0
    E_NULL, E_SIZE = C['STIN_E_NULL'], C['STIN_E_SIZE']

    def call(a=64, b=64, P=1, H=16, W=16, K=3, table=64):
        return lib.stin_view_metrics_u8(a, b, None, None, P, H, W, K, table, None, 0, None)
    big = C['STIN_RENDER_MAX_SIZE'] + 1
    assert call(H=0) == E_SIZE and call(W=0) == E_SIZE and call(H=big) == E_SIZE and call(W=big) == E_SIZE
    assert call(K=0) == E_SIZE and call(K=5) == E_SIZE and call(P=-1) == E_SIZE and call(P=2 ** 31 - 1) == E_SIZE
    assert call(a=None) == E_NULL and call(b=None) == E_NULL and call(table=None) == E_NULL          # (the pointers are never followed)
    assert call(a=None, b=None, table=None, P=0) == 0                     # nothing to do, nothing launched


def test_cpu_tensors_and_bad_arguments_are_refused():
    a = torch.zeros(1, 12, 12, 3, dtype=torch.uint8)
    with pytest.raises(TypeError):
        views.view_metrics(a, a)
    with pytest.raises(TypeError):
        views.view_metrics(a.numpy(), a.numpy())


# ------------------------------------------------------------------------------------------- derived figures and the JSON file
TABLE = [[100, 2550, 65025, 40, 3 * 40 * ONE // 2], [50, 0, 0, 0, 0], [0, 0, 0, 0, 0], [10, 30, 90, 4, -ONE]]


def hand_made():
    return views.ViewMetrics.from_table(torch.tensor(TABLE, dtype=torch.int64), 3)


def test_derived_figures_of_a_hand_made_table():
    m = hand_made()
    want = VO.derived(np.array(TABLE), 3)
    assert m.channels == 3 and m.table.dtype == torch.int64 and tuple(m) == (m.table, m.l1, m.mse, m.psnr, m.ssim)
    for key in ('l1', 'mse', 'ssim'):
        got = getattr(m, key)
        assert got.dtype == torch.float64 and np.array_equal(got.numpy(), want[key], equal_nan=True), key
    np.testing.assert_allclose(m.psnr.numpy(), want['psnr'], rtol=1e-14, equal_nan=True)      # (two log10 routines: an ulp)
    assert m.l1.tolist()[0] == 2550 / (255 * 3 * 100) and m.mse.tolist()[0] == pytest.approx(1 / 300)
    assert m.psnr.tolist()[0] == pytest.approx(10 * math.log10(300)) and m.ssim.tolist()[0] == 0.5
    assert m.psnr.tolist()[1] == math.inf and math.isnan(m.ssim.tolist()[1]) and m.mse.tolist()[1] == 0.0
    assert all(math.isnan(getattr(m, key).tolist()[2]) for key in ('l1', 'mse', 'psnr', 'ssim'))
    assert m.ssim.tolist()[3] == -1 / 12
    total = m.total()
    assert total['poses'] == 4 and total['channels'] == 3
    assert [total[k] for k in VO.COLUMNS] == [160, 2580, 65115, 44, 3 * 40 * ONE // 2 - ONE]
    assert total['l1'] == 2580 / (255.0 * 3 * 160) and total['mse'] == pytest.approx(65115 / (65025.0 * 3 * 160), rel=1e-15)
    assert total['psnr'] == pytest.approx(10 * math.log10(1 / total['mse'])) and total['ssim'] == pytest.approx((60 - 1) / (3 * 44), rel=1e-15)
    empty = views.ViewMetrics.from_table(torch.zeros(0, 5, dtype=torch.int64), 3).total()
    assert empty['n_pix'] == 0 and math.isnan(empty['psnr']) and math.isnan(empty['ssim'])
    exact = views.ViewMetrics.from_table(torch.tensor([[5, 0, 0, 0, 0]]), 3).total()
    assert exact['psnr'] == math.inf and exact['mse'] == 0.0


def test_write_result_views_writes_the_metrics_file_and_keeps_its_default(tmp_path):
    V = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=torch.float64)
    F = torch.tensor([[0, 1, 2], [0, 2, 3]])
    colorings = {'pred': torch.rand(4, 3), 'gt': torch.rand(4, 3)}
    before = views.write_result_views(str(tmp_path / 'a'), 'scene', V, F, colorings)
    assert [p[len(str(tmp_path / 'a')) + 1:] for p in before] == ['scene_pred.ply', 'scene_gt.ply']
    after = views.write_result_views(str(tmp_path / 'b'), 'scene', V, F, colorings, metrics=hand_made())
    assert [p[len(str(tmp_path / 'b')) + 1:] for p in after] == ['scene_pred.ply', 'scene_gt.ply', 'scene_view_metrics.json']
    for name in ('scene_pred.ply', 'scene_gt.ply'):                       # the other files do not change
        assert (tmp_path / 'a' / name).read_bytes() == (tmp_path / 'b' / name).read_bytes()
    assert sorted(p.name for p in (tmp_path / 'a').iterdir()) == ['scene_gt.ply', 'scene_pred.ply']
    doc = json.loads((tmp_path / 'b' / 'scene_view_metrics.json').read_text())
    assert doc['columns'] == list(VO.COLUMNS) and doc['channels'] == 3 and doc['table'] == TABLE
    assert all(isinstance(v, int) for row in doc['table'] for v in row)
    assert doc['l1'][0] == 2550 / (255 * 3 * 100) and doc['ssim'] == [0.5, None, None, -1 / 12]
    assert doc['psnr'][1] is None and doc['psnr'][2] is None and doc['psnr'][0] == pytest.approx(10 * math.log10(300))
    m = hand_made().total()
    assert doc['total'] == m and doc['total']['n_win'] == 44
