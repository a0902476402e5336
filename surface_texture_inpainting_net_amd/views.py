"""Headless result views: what the reference's `config['vis']` branch of Inpainting3DTrainer._eval (trainers/inpainting3d_trainer.py
:100-121) shows in an Open3D window (utils/ColorCompletionVisualizer.py: unlit vertex colours, five colourings on key presses, a
screenshot key `P`, a "save the PLYs" key `D`), for machines without a display and without Open3D.

* ``render_mesh``        a vertex-coloured mesh through a pinhole camera from a scan's poses -> colour, depth and face-id images, a
                         depth-tested triangle rasteriser in HIP (csrc/stin_render.hip; contract: include/stin_hip.h, "Render").  Its
                         depth images are the raw uint16 format ``preprocessing.FrameColors`` reads: rendering a coloured mesh and
                         feeding the frames back recovers the colours.
* ``result_colorings``   the visualiser's colourings (rgb, pred, gt, mask, diff) from the trainer's tensors, in plain torch.
* ``write_png``, ``write_ply``   8-bit PNG (stdlib zlib + struct) and binary little-endian PLY with uchar colours.
* ``write_result_views`` one PLY per colouring (the `D` key) and, with poses, one PNG per colouring and pose (the `P` key, from the
                         scan's own viewpoints).
* ``view_metrics``       PSNR and SSIM of two sets of such images, per pose, in one HIP pass (csrc/stin_view_metrics.hip; contract:
                         include/stin_hip.h, "View metrics"); ``result_view_metrics`` renders prediction and ground truth from every
                         pose, a chunk of poses at a time, and measures them.  Not pinned against skimage or piq: the 11 x 11 window
                         has integer taps, and there is no padding, no luma conversion and no multi-scale SSIM.

Out of scope: lighting, anti-aliasing, textures, clipping at the near plane (a face that crosses it is dropped), reading
images, the interactive viewer, SemSegVisualizer's palette (pass label colours as vertex colours), a CPU fallback.  Faces come from
the caller: graphs/<scene>.pt holds none.  Mesh files - write_ply's own included - are read by scene_io.read_ply, whose dict holds the
vertices, faces and colours render_mesh takes."""
import collections
import ctypes
import json
import math
import os
import struct
import zlib

import torch

from . import _lib
from .plan import _ptr, _stream
from .preprocessing import _camera4, _xyz64, pose_extrinsics

RenderResult = collections.namedtuple('RenderResult', 'color depth face_ids status')

VIEWS = ('rgb', 'pred', 'gt', 'mask', 'diff')
VIEW_METRICS_COLUMNS = ('n_pix', 'sum_abs', 'sum_sq', 'n_win', 'ssim_q')


class ViewMetrics(collections.namedtuple('ViewMetrics', 'table l1 mse psnr ssim')):
    """view_metrics' result: `table` int64 [P, 5] (VIEW_METRICS_COLUMNS: the exact integer sums of every pose) and what follows from it
    per pose, fp64 [P] on the table's device, in [0, 1] colour units: l1 = sum_abs / (255 K n_pix), mse = sum_sq / (255^2 K n_pix),
    psnr = 10 log10(1 / mse) in dB (inf where mse == 0; the trainer's psnr(data_range=2) of the same colours in [-1, 1]),
    ssim = ssim_q / (2^32 K n_win).  A pose with a zero denominator has NaN.  `channels` is K."""

    def __new__(cls, table, l1, mse, psnr, ssim, channels=3):
        self = super().__new__(cls, table, l1, mse, psnr, ssim)
        self.channels = int(channels)
        return self

    @classmethod
    def from_table(cls, table, channels):
        """The derived figures in torch, on the table's device: no read-back."""
        t = table.double()
        pix, win = (255.0 * channels) * t[:, 0], (4294967296.0 * channels) * t[:, 3]
        mse = t[:, 2] / (255.0 * pix)
        return cls(table, t[:, 1] / pix, mse, 10.0 * torch.log10(1.0 / mse), t[:, 4] / win, channels)

    def total(self):
        """The scene's figures from the column sums - every pixel and every window weighs the same, whichever pose it is in (a
        micro-average) - as a dict of Python ints and floats.  One read-back."""
        n_pix, sum_abs, sum_sq, n_win, ssim_q = (int(v) for v in self.table.sum(dim=0).cpu().tolist())
        K, nan = self.channels, float('nan')
        l1 = sum_abs / (255.0 * K * n_pix) if n_pix else nan
        mse = sum_sq / (255.0 * (255.0 * K * n_pix)) if n_pix else nan
        psnr = nan if not n_pix else float('inf') if sum_sq == 0 else 10.0 * math.log10(1.0 / mse)
        return {'poses': int(self.table.shape[0]), 'channels': K, 'n_pix': n_pix, 'sum_abs': sum_abs, 'sum_sq': sum_sq, 'n_win': n_win,
                'ssim_q': ssim_q, 'l1': l1, 'mse': mse, 'psnr': psnr, 'ssim': ssim_q / (4294967296.0 * K * n_win) if n_win else nan}


def render_mesh(vertices, faces, colors, poses, camera, height, width, *, dtype=torch.uint8, background=(0, 0, 0), depth=False,
                face_ids=False, z_near=0.01, depth_scale=1000.0, batch=16, large_box=None):
    """Images of a vertex-coloured mesh from camera poses, on the GPU (csrc/stin_render.hip).  vertices [N, >= 3] float, faces [F, 3]
    int, colors [N, K] float, 1 <= K <= 4, in [0, 1] (CUDA tensors); poses [P, 4, 4] camera-to-world (array or tensor, any device:
    they are inverted on the host by preprocessing.pose_extrinsics); camera = (fx, fy, cx, cy) in pixels of the height x width image
    (preprocessing.frame_intrinsics).
    -> the colour images [P, height, width, K], uint8 (default) or float32 (dtype); with depth=True and / or face_ids=True a
    RenderResult(color, depth uint16 [P, H, W] in 1 / depth_scale units with 0 = nothing there, face_ids int32 [P, H, W] with -1 =
    nothing there, status int: bit STIN_RENDER_BAD_INDEX - a face had an index outside [0, N) and was skipped; bit
    STIN_RENDER_LARGE_FACE - informational), the fields not asked for being None.

    The contract (include/stin_hip.h, "Render"; restated per pixel in numpy by the test suite, which this reproduces bit for bit),
    fp64: view = E [x y z 1], E the inverse pose; X = fx xv / zv + cx, Y = fy yv / zv + cy, pixel (row i, column j) centred at (j, i).
    A face with a corner nearer than z_near is DROPPED, not clipped; coverage is inclusive on every edge and takes both orientations;
    the nearest face wins a pixel after its depth is rounded to fp32, the lowest face id on a tie.  Colours are interpolated
    perspective-correctly, unlit, one sample at the pixel centre; uint8 = rint(255 clamp(c, 0, 1)), NaN -> 0.  A pixel nobody covers
    and every pixel of a pose with a non-finite entry get `background`.  The result depends neither on `batch` (poses per pass:
    batch * H * W * 8 bytes of keys and batch * N * 24 bytes of screen coordinates) nor on `large_box` (faces whose clamped box holds
    more centres go to a wavefront each; default STIN_RENDER_LARGE_BOX)."""
    C = _lib.CONSTANTS
    if not (torch.is_tensor(faces) and faces.is_cuda):
        raise TypeError('faces must be a CUDA tensor (no CPU fallback exists)')
    if not (torch.is_tensor(colors) and colors.is_cuda):
        raise TypeError('colors must be a CUDA tensor (no CPU fallback exists)')
    if not (torch.is_tensor(vertices) and vertices.is_cuda):
        raise TypeError('vertices must be a CUDA tensor (no CPU fallback exists)')
    if dtype not in (torch.uint8, torch.float32):
        raise TypeError('dtype must be torch.uint8 or torch.float32')
    if not colors.is_floating_point() or colors.dim() not in (1, 2) or colors.shape[0] != vertices.shape[0]:
        raise ValueError('colors must be float [N, K]')
    K = 1 if colors.dim() == 1 else int(colors.shape[1])
    if not 1 <= K <= 4:
        raise ValueError('colors must have 1 to 4 channels')
    bg = tuple(float(b) for b in background)
    if len(bg) != K and len(set(bg)) == 1:                                # one grey level for every channel, such as the default
        bg = bg[:1] * K
    if len(bg) != K:
        raise ValueError('background must have %d entries' % K)
    cam = _camera4(camera, 'camera')
    H, W, B = int(height), int(width), int(batch)
    if not 1 <= H <= C['STIN_RENDER_MAX_SIZE'] or not 1 <= W <= C['STIN_RENDER_MAX_SIZE'] or not 1 <= B <= C['STIN_RENDER_MAX_BATCH']:
        raise ValueError('height and width must be in [1, %d] and batch in [1, %d]' % (C['STIN_RENDER_MAX_SIZE'], C['STIN_RENDER_MAX_BATCH']))
    if not float(z_near) > 0.0 or not float(depth_scale) > 0.0:
        raise ValueError('z_near and depth_scale must be positive')
    lib = _lib.load()
    v = _xyz64(vertices, 'vertices')
    c = colors.reshape(int(v.shape[0]), K).float().contiguous()
    RT, valid = pose_extrinsics(poses)
    n, dev, P = int(v.shape[0]), v.device, int(RT.shape[0])
    f = faces.long().reshape(-1, 3).contiguous()
    F = int(f.shape[0])
    B = max(1, min(B, P))
    color = torch.empty(P, H, W, K, dtype=dtype, device=dev)
    dep = torch.empty(P, H, W, dtype=torch.uint16, device=dev) if depth else None
    fid = torch.empty(P, H, W, dtype=torch.int32, device=dev) if face_ids else None
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if P:
        rt_d, valid_d = torch.from_numpy(RT).to(dev), torch.from_numpy(valid).to(dev)
        ws_bytes = lib.stin_render_workspace_bytes(n, F, H, W, B)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        camera_h = (ctypes.c_double * C['STIN_RENDER_CAMERA_DOUBLES'])(*cam)
        bg_h = (ctypes.c_float * K)(*bg)
        _lib.check(lib.stin_render_poses_f64(_ptr(v) if n else None, n, _ptr(f) if F else None, F, _ptr(c) if n else None, K, _ptr(rt_d),
                                             _ptr(valid_d), P, camera_h, H, W, float(z_near), float(depth_scale), bg_h, B,
                                             int(large_box) if large_box is not None else 0, 0,
                                             _ptr(color) if dtype == torch.float32 else None, _ptr(color) if dtype == torch.uint8 else None,
                                             _ptr(dep), _ptr(fid), _ptr(status), _ptr(ws), ws_bytes, _stream(v)), 'stin_render_poses_f64')
    if not (depth or face_ids):
        return color
    return RenderResult(color, dep, fid, int(status.item()))


def result_colorings(pred, gt, mask, rgb=None):
    """The visualiser's colourings from the trainer's tensors -> dict of float32 [N, 3] in [0, 1] on the inputs' device.  pred, gt [N, 3]
    in [-1, 1] (the network's output and data.color), mask [N] or [N, 1] (data.mask; inpainted where mask > 0) - what _eval hands over
    as pred / 2 + 0.5, gt / 2 + 0.5 and mask > 0.
      'pred', 'gt'   the two, in [0, 1];
      'mask'         gt, black where the mask is set (where(mask, 0, gt));
      'diff'         the reference's heat vector of d = mean over the channels of |gt - pred| (of the [0, 1] colours): with ratio = 4 d,
                     r = max(0, ratio - 1), b = max(0, 1 - ratio), g = 1 - r - b - blue at 0, green at 0.25, red at 0.5; clamped to
                     [0, 1] beyond that (the reference leaves that to Open3D); 0.25 grey outside the mask;
      'rgb'          when given: the mesh's own colours, passed through (float32, [0, 1])."""
    if not (torch.is_tensor(pred) and torch.is_tensor(gt) and torch.is_tensor(mask)):
        raise TypeError('pred, gt and mask must be tensors')
    if pred.dim() != 2 or pred.shape[1] != 3 or pred.shape != gt.shape:
        raise ValueError('pred and gt must both be [N, 3]')
    if mask.numel() != pred.shape[0]:
        raise ValueError('mask must have one entry per vertex')
    p, g = pred.detach().float() / 2.0 + 0.5, gt.detach().float() / 2.0 + 0.5
    m = (mask.detach().reshape(-1, 1) > 0).expand_as(g)
    ratio = 4.0 * (g - p).abs().mean(dim=1)
    zero = torch.zeros_like(ratio)
    r, b = torch.maximum(zero, ratio - 1.0), torch.maximum(zero, 1.0 - ratio)
    heat = torch.stack([r, 1.0 - r - b, b], dim=1).clamp_(0.0, 1.0)
    out = {'pred': p, 'gt': g, 'mask': torch.where(m, torch.zeros_like(g), g), 'diff': torch.where(m, heat, torch.full_like(heat, 0.25))}
    if rgb is not None:
        if rgb.shape != g.shape:
            raise ValueError('rgb must be [N, 3]')
        out['rgb'] = rgb.detach().float()
    return out


def _mask_u8(m, shape, name):
    """A [P, H, W] mask as contiguous bytes: uint8 as it is, bool and integer masks as `!= 0`."""
    if m is None:
        return None
    if not (torch.is_tensor(m) and m.is_cuda):
        raise TypeError('%s must be a CUDA tensor (no CPU fallback exists)' % name)
    if tuple(m.shape) != tuple(shape):
        raise ValueError('%s must be [P, H, W] like the images' % name)
    if m.dtype != torch.uint8:
        m = (m != 0).view(torch.uint8)
    return m.contiguous()


def view_metrics(a, b, covered=None, region=None):
    """PSNR and SSIM of the images `a` against `b`, per pose, on the GPU (csrc/stin_view_metrics.hip).  a, b: CUDA uint8 [P, H, W, K],
    1 <= K <= 4, or [P, H, W]; covered, region: optional CUDA masks [P, H, W], uint8, bool or integer (non-zero = set; for instance
    RenderResult.face_ids >= 0).  -> ViewMetrics(table int64 [P, 5], l1, mse, psnr, ssim fp64 [P]), all on the device: nothing is
    read back.

    The contract (include/stin_hip.h, "View metrics"; restated in numpy by the test suite, which `table` reproduces byte for byte):
    n_pix, sum_abs = sum |a - b| and sum_sq = sum (a - b)^2 over the pixels that are covered and in the region; SSIM over 11 x 11
    windows with the INTEGER taps of a sigma 1.5 Gaussian scaled to 2^16, no padding (a window counts when it lies inside the image,
    all its 121 pixels are covered and its centre is in the region; none in an image under 11 pixels), per channel (no luma
    conversion), one scale; every window's value is rounded to 2^-32 and summed as an integer, so the table does not depend on how
    the work is split.  It is a contract of the project's own, not pinned against skimage or piq."""
    if not (torch.is_tensor(a) and a.is_cuda and torch.is_tensor(b) and b.is_cuda):
        raise TypeError('a and b must be CUDA tensors (no CPU fallback exists)')
    if a.dtype != torch.uint8 or b.dtype != torch.uint8:
        raise TypeError('a and b must be uint8 images')
    if a.shape != b.shape or a.dim() not in (3, 4):
        raise ValueError('a and b must both be [P, H, W, K] or [P, H, W]')
    P, H, W = (int(n) for n in a.shape[:3])
    K = 1 if a.dim() == 3 else int(a.shape[3])
    C = _lib.CONSTANTS
    if not 1 <= K <= 4:
        raise ValueError('the images must have 1 to 4 channels')
    if not 1 <= H <= C['STIN_RENDER_MAX_SIZE'] or not 1 <= W <= C['STIN_RENDER_MAX_SIZE']:
        raise ValueError('height and width must be in [1, %d]' % C['STIN_RENDER_MAX_SIZE'])
    cov, reg = _mask_u8(covered, a.shape[:3], 'covered'), _mask_u8(region, a.shape[:3], 'region')
    lib = _lib.load()
    a, b = a.contiguous(), b.contiguous()
    table = torch.empty(P, C['STIN_VIEW_METRICS_COLS'], dtype=torch.int64, device=a.device)
    if P:
        ws_bytes = lib.stin_view_metrics_workspace_bytes(P, H, W, K)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=a.device) if ws_bytes else None
        _lib.check(lib.stin_view_metrics_u8(_ptr(a), _ptr(b), _ptr(cov), _ptr(reg), P, H, W, K, _ptr(table), _ptr(ws), ws_bytes, _stream(a)),
                   'stin_view_metrics_u8')
    return ViewMetrics.from_table(table, K)


def result_view_metrics(vertices, faces, pred, gt, mask, poses, camera, height, width, *, region='mask', chunk=32, **render):
    """How good a prediction is as seen from the scan's cameras: result_colorings(pred, gt, mask)['pred'] against ['gt'], rendered by
    render_mesh from every pose (camera, height, width and further keywords are its) and measured by view_metrics -> ViewMetrics for
    the P poses.  A pixel is covered where a face was drawn (face_ids >= 0).  region='mask': only what the inpainted vertices reach -
    (mask > 0) is rendered as a one-channel colour on a black background, and a pixel is in the region where that image is non-zero;
    region='all': every covered pixel.  Poses are rendered `chunk` at a time, so at most 3 chunk H W 4 bytes of images exist at
    once; the result does not depend on `chunk`."""
    if region not in ('mask', 'all'):
        raise ValueError("region must be 'mask' or 'all'")
    if int(chunk) < 1:
        raise ValueError('chunk must be positive')
    colorings = result_colorings(pred, gt, mask)
    inpainted = (mask.detach().reshape(-1) > 0).float()
    P = len(poses)
    tables = []
    for p0 in range(0, P, int(chunk)):
        some = poses[p0:p0 + int(chunk)]
        shown = render_mesh(vertices, faces, colorings['pred'], some, camera, height, width, face_ids=True, **render)
        truth = render_mesh(vertices, faces, colorings['gt'], some, camera, height, width, **render)
        where = None
        if region == 'mask':
            where = render_mesh(vertices, faces, inpainted, some, camera, height, width, **dict(render, background=(0.0,)))[..., 0]
        tables.append(view_metrics(shown.color, truth, shown.face_ids >= 0, where).table)
    if not tables:
        tables.append(torch.zeros(0, len(VIEW_METRICS_COLUMNS), dtype=torch.int64, device=colorings['pred'].device))
    return ViewMetrics.from_table(torch.cat(tables), 3)


def _chunk(tag, data):
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path, image_u8):
    """An 8-bit PNG: image_u8 uint8 [H, W] or [H, W, 1] (grey) or [H, W, 3] (RGB), tensor on any device or array.  Stdlib only
    (zlib, struct): filter type 0 on every row, one IDAT chunk."""
    import numpy as np
    a = image_u8.detach().cpu().numpy() if torch.is_tensor(image_u8) else np.asarray(image_u8)
    if a.dtype != np.uint8:
        raise TypeError('image_u8 must be uint8')
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in (1, 3) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError('image_u8 must be [H, W], [H, W, 1] or [H, W, 3]')
    h, w, ch = a.shape
    rows = np.zeros((h, 1 + w * ch), dtype=np.uint8)                      # a filter byte (0 = none) in front of every row
    rows[:, 1:] = a.reshape(h, w * ch)
    ihdr = struct.pack('>IIBBBBB', w, h, 8, 0 if ch == 1 else 2, 0, 0, 0)
    with open(path, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n' + _chunk(b'IHDR', ihdr) + _chunk(b'IDAT', zlib.compress(rows.tobytes(), 6)) + _chunk(b'IEND', b''))


def _colors_u8(colors):
    """float [N, 3] in [0, 1] -> uint8 by the renderer's rule (rint(255 clamp(c)), NaN -> 0); uint8 passes through.  numpy."""
    import numpy as np
    c = colors.detach().cpu().numpy() if torch.is_tensor(colors) else np.asarray(colors)
    if c.dtype == np.uint8:
        return c
    t = c.astype(np.float32).astype(np.float64)
    with np.errstate(all='ignore'):
        t = np.where(t > 0.0, t, 0.0)
        t = np.where(t > 1.0, 1.0, t)
        return np.rint(t * 255.0).astype(np.uint8)


def write_ply(path, vertices, faces, colors):
    """A binary little-endian PLY: vertices [N, >= 3] (written as float x y z), colors [N, 3] float in [0, 1] or uint8 (uchar red green
    blue), faces [F, 3] (uchar count + three int indices).  Tensors on any device or arrays."""
    import numpy as np
    to_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    v, f, c = to_np(vertices), to_np(faces).reshape(-1, 3), _colors_u8(colors)
    if v.ndim != 2 or v.shape[1] < 3 or c.shape != (v.shape[0], 3):
        raise ValueError('vertices must be [N, >= 3] and colors [N, 3]')
    vert = np.empty(v.shape[0], dtype=[('xyz', '<f4', 3), ('rgb', 'u1', 3)])
    vert['xyz'], vert['rgb'] = v[:, :3], c
    face = np.empty(f.shape[0], dtype=[('n', 'u1'), ('ids', '<i4', 3)])
    face['n'], face['ids'] = 3, f
    header = ('ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n'
              'property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\nproperty list uchar int vertex_indices\n'
              'end_header\n' % (v.shape[0], f.shape[0]))
    with open(path, 'wb') as out:
        out.write(header.encode('ascii') + vert.tobytes() + face.tobytes())


def _finite(values):
    """Floats for a JSON file: a value that is not finite (NaN, inf) becomes null - the integer rows beside it say which it was."""
    return [v if math.isfinite(v) else None for v in values]


def write_result_views(out_dir, name, vertices, faces, colorings, poses=None, camera=None, height=None, width=None, metrics=None,
                       **render):
    """The visualiser's `D` key - one PLY per colouring, <out_dir>/<name>_<view>.ply - and, with poses, its `P` key from the scan's own
    viewpoints: <name>_<view>_<pose id>.png, rendered by render_mesh (camera, height, width and further keywords are its).
    colorings: result_colorings' dict (any dict of [N, 3] float colours).  metrics: a ViewMetrics (result_view_metrics) to write
    beside them as <name>_view_metrics.json - 'columns' and 'table' (the integer row of every pose), 'l1', 'mse', 'psnr', 'ssim' per
    pose and 'total' (ViewMetrics.total()); a figure that is not finite is written as null.  -> the list of the files written."""
    if poses is not None and (camera is None or height is None or width is None):
        raise ValueError('rendering from poses needs camera, height and width')
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for view, colors in colorings.items():
        path = os.path.join(out_dir, '%s_%s.ply' % (name, view))
        write_ply(path, vertices, faces, colors)
        written.append(path)
        if poses is None:
            continue
        images = render_mesh(vertices, faces, colors, poses, camera, height, width, **render).cpu()
        for p in range(int(images.shape[0])):
            path = os.path.join(out_dir, '%s_%s_%d.png' % (name, view, p))
            write_png(path, images[p])
            written.append(path)
    if metrics is not None:
        path = os.path.join(out_dir, '%s_view_metrics.json' % name)
        doc = {'columns': list(VIEW_METRICS_COLUMNS), 'channels': metrics.channels, 'table': metrics.table.cpu().tolist()}
        for key in ('l1', 'mse', 'psnr', 'ssim'):
            doc[key] = _finite(getattr(metrics, key).cpu().tolist())
        total = metrics.total()
        doc['total'] = dict(zip(total, _finite(total.values())))
        with open(path, 'w') as f:
            json.dump(doc, f, indent=1, allow_nan=False)
        written.append(path)
    return written
