"""The segmentation experiment's objective and metrics on the HIP kernels of csrc/stin_seg.hip.

The reference trainer (trainers/segmentation_trainer.py) trains SingleConvMeshNet with
``torch.nn.CrossEntropyLoss(ignore_index=0, weight=class_weights)`` over 21 classes (:54) and reports mIoU, mPrec, oPrec
and oAccuracy from a confusion matrix (ConfusionMatrixDCM + IoUDCM, :125-166, :206-235) that it builds with ``.cpu().numpy()``
and ``np.bincount`` on every step - one host synchronisation per step.  Here:

* ``cross_entropy`` / ``CrossEntropyLoss``: the weighted, ignore-index cross entropy ('mean' reduction) as one forward launch
  (plus a one-block fixed-order sum) and one backward launch; the same forward launch can add the step's arg-max counts to a
  device confusion matrix.  ``rows`` reads logits row rows[i] for target i: the evaluation's
  ``output[data.original_index_traces]`` without the [N_original, C] copy (no gradient through that path).
* ``ConfusionMatrix``: int64 [K, K] on the device (rows = target, columns = prediction, the reference's layout);
  ``value()`` is the only host synchronisation.
* ``scores``: IoUDCM.value's dict, same formulas.  Unlike the reference it does not zero the caller's matrix in place.
* ``Objective``: ``TrainStep(loss_fn=Objective(CrossEntropyLoss(...), ConfusionMatrix(...)))``.

Out-of-range labels (neither in [0, C) nor ignore_index) contribute nothing on the GPU and set a device flag; it is copied
to pinned host memory behind an event after every launch and raised as IndexError at the next call of this module on that
device (or by ``ConfusionMatrix.value()``), without a per-step synchronisation - the deferred pattern of
plan.GraphPlan.validate.  CPU tensors take plain torch ops, as metrics.py does.
"""
import warnings

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from .plan import _ptr, _stream

MIN_CLASSES = _lib.CONSTANTS['STIN_SEG_MIN_CLASSES']
MAX_CLASSES = _lib.CONSTANTS['STIN_SEG_MAX_CLASSES']      # the per-block C x C int32 histogram is 64 KB of LDS there


class _DeferredFlag:
    """One device word per GPU that the kernels set on an out-of-range label; checked one launch later."""

    def __init__(self, device):
        self.dev = torch.zeros(1, dtype=torch.int32, device=device)
        self.host = torch.zeros(1, dtype=torch.int32, pin_memory=True)
        self.event = None

    def check(self):
        """Raise if a launch since the last check saw a bad label.  Waits for THAT launch only (it is a step behind the host)."""
        if self.event is None:
            return
        self.event.synchronize()
        self.event = None
        if int(self.host[0]) != 0:
            self.host[0] = 0
            self.dev.zero_()
            raise IndexError('segmentation: a target is outside [0, num_classes) and is not ignore_index (or a rows index is '
                             'outside the logits), reported by the deferred check of an earlier call')

    def launched(self):
        self.host.copy_(self.dev, non_blocking=True)
        self.event = torch.cuda.current_stream(self.dev.device).record_event()


_FLAGS = {}


def _flag(device):
    key = device.index if device.index is not None else torch.cuda.current_device()
    f = _FLAGS.get(key)
    if f is None:
        f = _FLAGS[key] = _DeferredFlag(torch.device('cuda', key))
    return f


def check_deferred(device=None):
    """Resolve the pending label check of `device` (all GPUs when None); raises IndexError for a bad label."""
    for k, f in list(_FLAGS.items()):
        if device is None or torch.device(device).index in (None, k):
            f.check()


def _num_classes(logits):
    if logits.dim() != 2:
        raise ValueError('logits must be [N, C], got shape %s' % (tuple(logits.shape),))
    C = int(logits.shape[1])
    if not MIN_CLASSES <= C <= MAX_CLASSES:
        raise ValueError('segmentation kernels support %d <= C <= %d classes, got %d' % (MIN_CLASSES, MAX_CLASSES, C))
    return C


def _gpu_args(logits, target, weight, rows):
    """Validate shapes / dtypes (metadata only: no device sync) -> (logits, ld, target, weight, rows)."""
    if logits.dtype != torch.float32:
        raise ValueError('GPU logits must be float32, got %s' % logits.dtype)
    C = _num_classes(logits)
    if logits.stride(1) != 1 or (logits.shape[0] > 1 and logits.stride(0) < C):
        logits = logits.contiguous()
    ld = logits.stride(0) if logits.shape[0] > 1 else max(C, logits.stride(0))
    target = target.reshape(-1)
    if target.dtype != torch.int64:
        target = target.long()
    target = target.contiguous()
    if rows is not None:
        rows = rows.reshape(-1).long().contiguous()
        if rows.numel() != target.numel():
            raise ValueError('rows has %d entries for %d targets' % (rows.numel(), target.numel()))
    elif target.numel() != logits.shape[0]:
        raise ValueError('%d targets for %d logits rows' % (target.numel(), logits.shape[0]))
    if target.numel() == 0:
        raise ValueError('empty batch')
    if weight is not None:
        weight = weight.reshape(-1).to(device=logits.device, dtype=torch.float32).contiguous()
        if weight.numel() != C:
            raise ValueError('weight has %d entries for %d classes' % (weight.numel(), C))
    for t in (target, rows, weight):
        if t is not None and t.device != logits.device:
            raise ValueError('all tensors must be on %s' % logits.device)
    return logits, ld, target, weight, rows


def _conf_tensor(confusion, C, device):
    if confusion is None:
        return None
    m = confusion.matrix if isinstance(confusion, ConfusionMatrix) else confusion
    if m.dtype != torch.int64 or tuple(m.shape) != (C, C) or not m.is_contiguous() or m.device != device:
        raise ValueError('confusion must be a contiguous int64 [%d, %d] tensor on %s' % (C, C, device))
    return m


def _launch_fwd(logits, ld, target, weight, ignore_index, rows, conf, want_loss):
    """One forward launch (+ the fixed-order sum when want_loss) -> (loss [] fp32, den [1] fp64) or (None, None)."""
    flag = _flag(logits.device)
    flag.check()
    lib = _lib.load()
    N = target.numel()
    M = logits.shape[0]
    loss = den = ws = None
    ws_bytes = 0
    if want_loss:
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        den = torch.empty(1, dtype=torch.float64, device=logits.device)
        ws_bytes = lib.stin_seg_ce_workspace_bytes(N)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=logits.device)
    _lib.check(lib.stin_seg_ce_fwd_f32(_ptr(logits), ld, M, _ptr(rows), _ptr(target), N, logits.shape[1], _ptr(weight),
                                       int(ignore_index), _ptr(loss), _ptr(den), _ptr(conf), _ptr(flag.dev), _ptr(ws), ws_bytes,
                                       _stream(logits)), 'stin_seg_ce_fwd_f32')
    flag.launched()
    return loss, den


class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, weight, ignore_index, conf):
        logits, ld, target, weight, _ = _gpu_args(logits, target, weight, None)
        loss, den = _launch_fwd(logits, ld, target, weight, ignore_index, None, conf, True)
        ctx.save_for_backward(logits, target, weight, den)
        ctx.ld, ctx.ignore_index = ld, ignore_index
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, target, weight, den = ctx.saved_tensors
        N, C = target.numel(), logits.shape[1]
        g = g.reshape(1).to(torch.float32).contiguous()
        dlogits = torch.empty(N, C, dtype=torch.float32, device=logits.device)
        _lib.check(_lib.load().stin_seg_ce_bwd_f32(_ptr(logits), ctx.ld, _ptr(target), N, C, _ptr(weight), int(ctx.ignore_index),
                                                   _ptr(g), _ptr(den), _ptr(dlogits), C, _stream(logits)), 'stin_seg_ce_bwd_f32')
        return dlogits, None, None, None, None


def _cpu_confusion_add(conf, logits, target):
    """ConfusionMatrixDCM.add on CPU tensors (arg-max of torch.max, np.bincount's layout); bad labels raise here."""
    C = logits.shape[1]
    target = target.reshape(-1).long()
    pred = logits.detach().max(1)[1]
    if target.numel() and (int(target.min()) < 0 or int(target.max()) >= C):
        raise IndexError('segmentation: a target is outside [0, %d)' % C)
    conf += torch.bincount(pred + C * target, minlength=C * C).reshape(C, C).to(conf.dtype)


def cross_entropy(logits, target, weight=None, ignore_index=-100, rows=None, confusion=None):
    """torch.nn.functional.cross_entropy(logits[rows] if rows is not None else logits, target, weight, ignore_index=...,
    reduction='mean') -> 0-d loss on the logits' device.  confusion (ConfusionMatrix or int64 [C, C] tensor): the same
    launch adds the (target, arg-max) counts; a target equal to ignore_index that is a valid class is counted, as the
    reference's matrix does.  Differentiable unless `rows` is given (evaluation: pass rows under torch.no_grad())."""
    if not logits.is_cuda:
        x = logits if rows is None else logits[rows]
        loss = F.cross_entropy(x, target, weight=weight, ignore_index=ignore_index)
        if confusion is not None:
            _cpu_confusion_add(_conf_tensor_cpu(confusion, x.shape[1]), x, target)
        return loss
    C = _num_classes(logits)
    conf = _conf_tensor(confusion, C, logits.device)
    if rows is not None:
        if torch.is_grad_enabled() and logits.requires_grad:
            raise ValueError('cross_entropy(rows=...) has no backward (evaluation path): call it under torch.no_grad() '
                             'or with detached logits')
        logits, ld, target, weight, rows = _gpu_args(logits, target, weight, rows)
        return _launch_fwd(logits, ld, target, weight, ignore_index, rows, conf, True)[0]
    return _CrossEntropyFn.apply(logits, target, weight, int(ignore_index), conf)


def _conf_tensor_cpu(confusion, C):
    m = confusion.matrix if isinstance(confusion, ConfusionMatrix) else confusion
    if tuple(m.shape) != (C, C):
        raise ValueError('confusion must be [%d, %d]' % (C, C))
    return m


class CrossEntropyLoss(torch.nn.Module):
    """Drop-in for torch.nn.CrossEntropyLoss(weight, ignore_index) of the segmentation trainer (reduction 'mean' only);
    forward(input, target, rows=None, confusion=None) - see cross_entropy."""

    def __init__(self, weight=None, ignore_index=-100, reduction='mean'):
        super().__init__()
        if reduction != 'mean':
            raise NotImplementedError("CrossEntropyLoss: only reduction='mean' (the trainer's) is implemented")
        self.register_buffer('weight', None if weight is None else torch.as_tensor(weight, dtype=torch.float32))
        self.ignore_index = int(ignore_index)
        self.reduction = reduction

    def forward(self, input, target, rows=None, confusion=None):
        w = self.weight
        if w is not None and w.device != input.device:
            w = w.to(input.device)
        return cross_entropy(input, target, w, self.ignore_index, rows, confusion)


class ConfusionMatrix:
    """ConfusionMatrixDCM on the device: int64 [K, K], rows = target, columns = arg-max prediction."""

    def __init__(self, num_classes, device='cuda'):
        self.num_classes = int(num_classes)
        if not MIN_CLASSES <= self.num_classes <= MAX_CLASSES:
            raise ValueError('segmentation kernels support %d <= K <= %d classes, got %d'
                             % (MIN_CLASSES, MAX_CLASSES, self.num_classes))
        self.device = torch.device(device)
        self.matrix = torch.zeros(self.num_classes, self.num_classes, dtype=torch.int64, device=self.device)

    def add(self, logits, target, rows=None):
        """Add the counts of (target, first arg-max of the logits row) - of logits[rows] when rows is given."""
        if logits.shape[-1] != self.num_classes:
            raise ValueError('logits have %d classes, the matrix %d' % (logits.shape[-1], self.num_classes))
        if not logits.is_cuda:
            _cpu_confusion_add(self.matrix, logits if rows is None else logits[rows], target)
            return self
        logits, ld, target, _, rows = _gpu_args(logits.detach(), target, None, rows)
        # (a matrix-only launch has no ignore_index: every target outside [0, K) is an error, as in ConfusionMatrixDCM.add)
        _launch_fwd(logits, ld, target, None, -100, rows, _conf_tensor(self, self.num_classes, logits.device), False)
        return self

    def reset(self):
        self.matrix.zero_()
        return self

    def all_reduce(self, group=None):
        """Sum the matrices of all ranks (int64, exact)."""
        import torch.distributed as dist
        dist.all_reduce(self.matrix, op=dist.ReduceOp.SUM, group=group)
        return self

    def value(self):
        """-> host int64 [K, K] (the one host synchronisation); raises IndexError for a bad label of an earlier call."""
        out = self.matrix.cpu()
        if self.matrix.is_cuda:
            check_deferred(self.matrix.device)
        return out


def scores(conf, ignore_index=None):
    """IoUDCM(ignore_index).value(conf): per-class IoU, its nanmean, 'precision' per class (TP / (TP + FN), the reference's
    name), its nanmean, overall precision and accuracy (both TP.sum() / conf.sum()).  The ignored classes' rows and columns
    are zeroed in a COPY: the caller's matrix is left as it is."""
    m = (conf.detach().cpu().numpy() if torch.is_tensor(conf) else np.asarray(conf)).copy()
    if ignore_index is not None:
        idx = (ignore_index,) if isinstance(ignore_index, (int, np.integer)) else tuple(ignore_index)
        m[:, idx] = 0
        m[idx, :] = 0
    tp = np.diag(m)
    fp = np.sum(m, 0) - tp
    fn = np.sum(m, 1) - tp
    with np.errstate(divide='ignore', invalid='ignore'):
        iou = tp / (tp + fp + fn)
        precision = tp / (tp + fn)
        overall_precision = np.sum(tp) / np.sum(m)
        overall_accuracy = np.sum(tp) / np.sum(m)
    with warnings.catch_warnings():                         # nanmean of an all-NaN vector: NaN, as the reference
        warnings.simplefilter('ignore', RuntimeWarning)
        mean_iou, mean_precision = np.nanmean(iou), np.nanmean(precision)
    return {'iou': iou, 'mean_iou': mean_iou, 'precision_per_class': precision, 'mean_precision': mean_precision,
            'overall_precision': overall_precision, 'overall_accuracy': overall_accuracy}


class Objective:
    """loss_fn for train_step.TrainStep: (model, sample) -> criterion(model(sample), sample.labels), with the step's
    confusion counts added by the same launch when a ConfusionMatrix is given.  A torch.nn.CrossEntropyLoss criterion is
    taken over with its weight and ignore_index."""

    def __init__(self, criterion, confusion=None):
        if isinstance(criterion, torch.nn.CrossEntropyLoss) and not isinstance(criterion, CrossEntropyLoss):
            criterion = CrossEntropyLoss(criterion.weight, criterion.ignore_index, criterion.reduction)
        self.criterion = criterion
        self.confusion = confusion

    def __call__(self, model, sample):
        return self.criterion(model(sample), sample.labels, confusion=self.confusion)
