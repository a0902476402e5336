"""The "View metrics" contract of include/stin_hip.h in numpy, by brute force: every window is one 121-tap sum with the 2-D weight
w[i] w[j] over its 11 x 11 pixels (int64), its coverage is a test of all 121 mask bytes, and v is evaluated in fp64 in the order the
header writes it.  Nothing here is separable, tiled or staged: it shares no code and no structure with csrc/stin_view_metrics.hip."""
import collections

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

TAPS = np.array([67, 498, 2359, 7167, 13960, 17434, 13960, 7167, 2359, 498, 67], dtype=np.int64)
WIN = 11
W2 = TAPS[:, None] * TAPS[None, :]                                       # sums to 2^32
C1, C2 = 6.5025, 58.5225
ONE = 1 << 32
COLUMNS = ('n_pix', 'sum_abs', 'sum_sq', 'n_win', 'ssim_q')

Windows = collections.namedtuple('Windows', 'counted v q')               # [P, H - 10, W - 10] bool, [P, H - 10, W - 10, K] fp64 / int64


def _images(a, b, covered, region):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape == b.shape and a.ndim in (3, 4)
    if a.ndim == 3:
        a, b = a[..., None], b[..., None]
    shape = a.shape[:3]
    cov = np.ones(shape, dtype=bool) if covered is None else np.asarray(covered) != 0
    reg = np.ones(shape, dtype=bool) if region is None else np.asarray(region) != 0
    assert cov.shape == shape and reg.shape == shape and 1 <= a.shape[3] <= 4
    return a.astype(np.int64), b.astype(np.int64), cov, reg


def _weighted(x):
    """[P, H, W, K] int64 -> [P, H - 10, W - 10, K]: sum of W2 times the 11 x 11 pixels from each corner on."""
    win = sliding_window_view(x, (WIN, WIN), axis=(1, 2))               # [P, H - 10, W - 10, K, 11, 11]
    return (win * W2).sum(axis=(-2, -1))


def ssim_value(Sa, Sb, Saa, Sbb, Sab):
    """v of the header from the five integer moments (arrays or scalars), fp64."""
    s = 2.0 ** -32
    Sa, Sb, Saa, Sbb, Sab = (np.asarray(t, dtype=np.int64).astype(np.float64) for t in (Sa, Sb, Saa, Sbb, Sab))
    ma = Sa * s
    mb = Sb * s
    va = Saa * s - ma * ma
    vb = Sbb * s - mb * mb
    c = Sab * s - ma * mb
    return ((2.0 * ma * mb + C1) * (2.0 * c + C2)) / ((ma * ma + mb * mb + C1) * (va + vb + C2))


def windows(a, b, covered=None, region=None):
    """Every 'valid' window of every pose: whether it is counted, its v and its q per channel."""
    a, b, cov, reg = _images(a, b, covered, region)
    P, H, W, K = a.shape
    if H < WIN or W < WIN:
        e = np.zeros((P, max(H - WIN + 1, 0), max(W - WIN + 1, 0)), dtype=bool)
        return Windows(e, np.zeros(e.shape + (K,)), np.zeros(e.shape + (K,), dtype=np.int64))
    all_covered = sliding_window_view(cov, (WIN, WIN), axis=(1, 2)).all(axis=(-2, -1))
    counted = all_covered & reg[:, WIN // 2:H - WIN // 2, WIN // 2:W - WIN // 2]
    v = ssim_value(_weighted(a), _weighted(b), _weighted(a * a), _weighted(b * b), _weighted(a * b))
    q = np.rint(v * float(ONE)).astype(np.int64)                         # np.rint: ties to even
    return Windows(counted, v, q)


def table(a, b, covered=None, region=None):
    """-> int64 [P, 5]: n_pix, sum_abs, sum_sq, n_win, ssim_q."""
    w = windows(a, b, covered, region)
    a, b, cov, reg = _images(a, b, covered, region)
    use = (cov & reg)[..., None]
    d = (a - b) * use
    out = np.zeros((a.shape[0], 5), dtype=np.int64)
    out[:, 0] = (cov & reg).sum(axis=(1, 2))
    out[:, 1] = np.abs(d).sum(axis=(1, 2, 3))
    out[:, 2] = (d * d).sum(axis=(1, 2, 3))
    out[:, 3] = w.counted.sum(axis=(1, 2))
    out[:, 4] = (w.q * w.counted[..., None]).sum(axis=(1, 2, 3))
    return out


def derived(tab, K):
    """l1, mse, psnr, ssim per row of a table, fp64, in [0, 1] colour units; NaN on a zero denominator, psnr inf at mse 0."""
    t = np.asarray(tab, dtype=np.int64).astype(np.float64)
    with np.errstate(all='ignore'):
        pix = (255.0 * K) * t[:, 0]
        mse = t[:, 2] / (255.0 * pix)
        return {'l1': t[:, 1] / pix, 'mse': mse, 'psnr': 10.0 * np.log10(1.0 / mse), 'ssim': t[:, 4] / ((float(ONE) * K) * t[:, 3])}
