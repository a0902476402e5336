"""Numpy restatement of the "Image resize" contract of include/stin_hip.h, written from the header alone: it shares no code with the
package.  linear(img, h, w) and area(img, h, w) take a uint8 [H, W, C] array and return uint8 [h, w, C]."""
import numpy as np

MAX_SIDE = 16384


def _check(img, h, w):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] in (1, 3, 4)
    H, W = img.shape[:2]
    assert all(1 <= v <= MAX_SIDE for v in (H, W, h, w))
    return img, H, W


def linear_axis(n_in, n_out):
    """-> (s, t, a, b): first tap, second tap, their weights (a + b = 2048), one entry per output index."""
    d = np.arange(n_out, dtype=np.int64)
    num = (2 * d + 1) * n_in - n_out
    den = 2 * n_out
    s = np.floor_divide(num, den)                    # floor, also below zero
    r = num - s * den
    b = (4096 * r + den) // (2 * den)
    low, high = s < 0, s >= n_in - 1
    s = np.where(low, 0, s)
    s = np.where(high, n_in - 1, s)
    b = np.where(low | high, 0, b)
    t = np.minimum(s + 1, n_in - 1)
    return s, t, 2048 - b, b


def linear(img, h, w):
    img, H, W = _check(img, h, w)
    sy, ty, ay, by = linear_axis(H, h)
    sx, tx, ax, bx = linear_axis(W, w)
    v = img.astype(np.int64)
    ax, bx = ax[None, :, None], bx[None, :, None]
    top = ax * v[sy][:, sx] + bx * v[sy][:, tx]
    bottom = ax * v[ty][:, sx] + bx * v[ty][:, tx]
    out = (ay[:, None, None] * top + by[:, None, None] * bottom + (1 << 21)) >> 22
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def area_overlap(n_in, n_out):
    """int64 [n_out, n_in]: o(j, x) = max(0, min((x + 1) n_out, (j + 1) n_in) - max(x n_out, j n_in))."""
    j = np.arange(n_out, dtype=np.int64)[:, None]
    x = np.arange(n_in, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((x + 1) * n_out, (j + 1) * n_in) - np.maximum(x * n_out, j * n_in))


def area(img, h, w):
    img, H, W = _check(img, h, w)
    assert h <= H and w <= W, 'AREA does not enlarge'
    ox = area_overlap(W, w)                          # [w, W]
    v = img.astype(np.int64)
    out = np.empty((h, w, img.shape[2]), dtype=np.uint8)
    for i in range(h):
        y = np.arange(H, dtype=np.int64)
        oy = np.maximum(0, np.minimum((y + 1) * h, (i + 1) * H) - np.maximum(y * h, i * H))
        rows = np.flatnonzero(oy)
        band = np.tensordot(oy[rows], v[rows], axes=(0, 0))          # [W, C], int64
        S = ox @ band                                                # [w, C]
        out[i] = ((2 * S + W * H) // (2 * W * H)).astype(np.uint8)
    return out
