"""Per-step graph metrics of the reference trainer on the HIP segment-sum kernel
(reference utils/metrics/graph_metrics.py:6-74, called every step at
trainers/inpainting3d_trainer.py:254-263).  GraphLaplaceOperator there is a PyG MessagePassing with
aggr='add' - a literal scatter-add of [E, 2] rows - which is exactly stin_segment_sum_f32 over the
destination CSR of the plan that the forward pass has already built (no second sort)."""
import torch

from . import functional as SF
from .plan import EdgeSet


def _edges(edge_index, n):
    if isinstance(edge_index, EdgeSet):
        return edge_index
    bad = torch.zeros(1, dtype=torch.int32, device=edge_index.device)
    return EdgeSet(edge_index, n, bad)


def grayscale(x):
    return 0.299 * x[:, 0:1] + 0.587 * x[:, 1:2] + 0.114 * x[:, 2:3]


def graph_laplace(x, edge_index):
    """sum_{j in N(i)} x_j - deg_i x_i   (graph_metrics.py:6-16): one HIP pass over the destination CSR (stin_graph_laplace_f32; the
    metric is evaluated under no_grad by the trainer); a tensor that needs a gradient takes the differentiable segment-sum form."""
    e = _edges(edge_index, x.shape[0])
    if x.is_cuda and x.dtype == torch.float32 and not (torch.is_grad_enabled() and x.requires_grad):
        from .plan import _ptr, _stream
        xm, ldx = SF._mat(x.detach())
        out = torch.empty(xm.shape[0], xm.shape[1], dtype=torch.float32, device=x.device)
        SF._call('stin_graph_laplace_f32', _ptr(xm), ldx, _ptr(e.by_dst.rowptr), _ptr(e.by_dst.col), xm.shape[0], xm.shape[1], _ptr(out),
                 out.stride(0), _stream(xm))
        return out
    xi = torch.cat([x.new_ones(x.shape[0], 1), x], dim=1).contiguous()
    prop = SF.segment_sum(xi, e.by_dst.rowptr, e.by_dst.col, e.n, mean=False)
    return prop[:, 1:] - prop[:, 0:1] * x


def graph_laplace_variance(x, edge_index):
    """graph_metrics.py:19-31."""
    with torch.no_grad():
        return torch.var(graph_laplace(grayscale(x), edge_index), dim=0, unbiased=False)


def graph_total_variation(x, edge_index):
    """sum_e |x_src - x_dst| / (N * C)   (graph_metrics.py:34-38): one HIP pass over the destination CSR (each vertex walks
    its in-edges), fp64 partial sums in a fixed order - no [E, C] temporaries, no host sync."""
    from . import _lib
    from .plan import _ptr, _stream
    e = _edges(edge_index, x.shape[0])
    x, ldx = SF._mat(x.detach().float())
    n, c = x.shape
    lib = _lib.load()
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    ws_bytes = lib.stin_total_variation_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    SF._call('stin_total_variation_f32', _ptr(x), ldx, _ptr(e.by_dst.rowptr), _ptr(e.by_dst.col), n, c, _ptr(out), _ptr(ws),
             ws_bytes, _stream(x))
    return out[0]


def psnr(x, y, data_range=1.0, convert_to_greyscale=False):
    """graph_metrics.py:41-74."""
    x = x / data_range
    y = y / data_range
    if x.size(1) == 3 and convert_to_greyscale:
        x, y = grayscale(x), grayscale(y)
    mse = torch.mean((x - y) ** 2, dim=[0, 1])
    return -10 * torch.log10(mse + 1e-8)


# ---------------------------------------------------------------------------------------------------------------------------------
# The trainer's per-step metrics without a host round trip (trainers/inpainting3d_trainer.py:254-271): one HIP call per step
# writes a row of a device table, the host reads the table once per epoch.
def _step_row_torch(out, color, mask, edge_index, composite, use_weight, data_range, loss):
    """The row stin_inpaint_metrics_f32 writes, through torch (CPU tensors): fp32 terms, L_i by fp32 adds in edge order, sums in
    double, one final cast.  -> float32 [8]."""
    m = mask.reshape(-1)
    inside = m > 0
    out = out.float()
    P = torch.where(inside[:, None], out, color) if composite else out
    n, C = P.shape
    d = P - color
    a, q = d.abs(), d * d
    w = torch.pow(0.99, m.float())[:, None] if use_weight else torch.ones(n, 1)
    cnt = int(inside.sum())
    mse = q.double().sum() / (n * C)
    mse_in = q[inside].double().sum() / (cnt * C) if cnt else torch.tensor(float('nan'), dtype=torch.float64)
    src, dst = edge_index[0], edge_index[1]
    tv = (P[src] - P[dst]).abs().sum(dim=1).double().sum() / (n * C)
    if C == 3:
        g = grayscale(P)[:, 0]
        s = torch.zeros(n).index_add_(0, dst, g[src])                   # (CPU index_add_: sequential, edge order)
        deg = torch.zeros(n).index_add_(0, dst, torch.ones(dst.numel()))
        lap_var = (s - deg * g).double().var(unbiased=False)
    else:
        lap_var = torch.tensor(float('nan'), dtype=torch.float64)
    r2 = float(data_range) ** 2
    row = torch.stack([(a * w).double().sum() / (n * C), a.double().sum() / (n * C), mse, tv, lap_var,
                       -10 * torch.log10(mse / r2 + 1e-8), -10 * torch.log10(mse_in / r2 + 1e-8),
                       torch.tensor(float(cnt), dtype=torch.float64)]).float()
    if loss is not None:
        row[0] = torch.as_tensor(loss, dtype=torch.float32).reshape(())
    return row


class StepMetrics:
    """The reference's MetricTracker for the inpainting trainer's seven step metrics, kept on the device: ``update`` is one HIP
    call (stin_inpaint_metrics_f32, no host synchronisation) that writes row ``len(self)`` of a ``[capacity, 8]`` table,
    ``rows()`` / ``result()`` read the table back once - per epoch, not per metric and step.  Column 8 of a row is the number of
    masked vertices of that step.  CPU tensors take a torch path with the same semantics."""

    KEYS = ('loss', 'l1', 'mse', 'graph_tv', 'graph_lap_var', 'psnr', 'psnr_mask_only')
    # kernel layout (include/stin_hip.h): 1 = P rows staged in CSR row order, 16 bytes per edge; 0 = one pass, 32 bytes per edge.
    # The two give identical bits; which is faster: profiles/r09_step_metrics.md.
    LAYOUT = 1

    def __init__(self, device, capacity=1024, use_mask_weighted_loss=True, data_range=2.0):
        self.device = torch.device(device)
        self.use_mask_weighted_loss = bool(use_mask_weighted_loss)
        self.data_range = float(data_range)
        self.table = torch.zeros(max(1, int(capacity)), 8, dtype=torch.float32, device=self.device)
        self._n = 0
        self._ws = None

    def __len__(self):
        return self._n

    def reset(self):
        self._n = 0

    def _row(self):
        """The next row of the table as a device view (the table doubles, with a device-side copy, when it is full)."""
        if self._n == self.table.shape[0]:
            grown = torch.zeros(2 * self.table.shape[0], 8, dtype=torch.float32, device=self.device)
            grown[:self._n].copy_(self.table)
            self.table = grown
        self._n += 1
        return self.table[self._n - 1]

    def update(self, out, sample, loss=None, composite=True):
        """One step: ``out`` = the raw network output [N, C] (composite=True forms where(mask > 0, out, color) itself; False takes
        ``out`` as the prediction), ``sample`` supplies color, mask and the level-0 edges (the cached plan's edge set in the
        plan's own vertex order when there is one - no second sort), ``loss`` = a loss computed elsewhere (0-dim tensor on the
        device), else the masked weighted L1 of the trainer is computed.  -> the row, a device view [8]."""
        out = out.detach()
        if out.dtype != torch.float32:
            out = out.float()
        color, mask = sample.color, sample.mask.reshape(-1)
        if not out.is_cuda:
            row = self._row()
            row.copy_(_step_row_torch(out, color, mask, sample.edge_index, composite, self.use_mask_weighted_loss,
                                      self.data_range, None if loss is None else loss.detach() if torch.is_tensor(loss) else loss))
            return row
        from . import _lib
        from .plan import _ptr, _stream
        n = out.shape[0]
        plan = getattr(sample, '_plan_cache', None)
        perm = None
        if plan is not None and plan.device == out.device:
            e = plan.edges('edge_index', 0)
            perm = plan.order0
        else:
            e = _edges(sample.edge_index, n)
        out, ldo = SF._mat(out)
        color, _ = SF._mat(color if color.is_contiguous() else color.contiguous())
        if mask.dtype != torch.int64 or not mask.is_contiguous():
            mask = mask.to(torch.int64).contiguous()
        if loss is not None:
            loss = loss.detach()
            if loss.dtype != torch.float32 or loss.device != out.device:
                loss = loss.to(out.device, torch.float32)
        lib = _lib.load()
        ws_bytes = lib.stin_inpaint_metrics_workspace_bytes(n)
        if self._ws is None or self._ws.numel() < ws_bytes:
            self._ws = torch.empty(ws_bytes, dtype=torch.uint8, device=out.device)
        row = self._row()
        SF._call('stin_inpaint_metrics_f32', _ptr(out), ldo, _ptr(color), _ptr(mask), _ptr(e.by_dst.rowptr), _ptr(e.by_dst.col),
                 _ptr(perm), n, out.shape[1], int(bool(composite)), int(self.use_mask_weighted_loss), self.data_range,
                 _ptr(loss), self.LAYOUT, _ptr(row), _ptr(self._ws), self._ws.numel(), _stream(out))
        return row

    def rows(self):
        """-> [steps, 8] CPU tensor, one copy (this is the epoch's one host synchronisation)."""
        return self.table[:self._n].cpu()

    def result(self):
        """{key: mean of the per-step values, in double}: MetricTracker.result() of the reference for n = 1 updates (a NaN step
        makes the average NaN, as there)."""
        r = self.rows().double()
        return {k: (float(r[:, i].sum() / r.shape[0]) if r.shape[0] else 0.0) for i, k in enumerate(self.KEYS)}


def _image_row_torch(out, color, mask, num_images, composite, data_range, loss):
    """The row stin_image_metrics_f32 writes, through torch (CPU tensors): fp32 terms, sums in double, one final cast.
    -> float32 [8]."""
    inside = mask.reshape(-1) != 0
    out = out.float()
    P = torch.where(inside[:, None], out, color) if composite else out
    n, C = P.shape
    d = P - color
    sq = (d * d).double().reshape(num_images, -1).sum(dim=1)
    mse_b = sq / (n // num_images * C)
    psnr = (-10 * torch.log10(mse_b / float(data_range) ** 2 + 1e-8)).sum() / num_images
    l1 = d.abs().double().sum() / (n * C)
    zero = torch.zeros((), dtype=torch.float64)
    row = torch.stack([l1, l1, sq.sum() / (n * C), psnr, inside.sum().double(), zero, zero, zero]).float()
    if loss is not None:
        row[0] = torch.as_tensor(loss, dtype=torch.float32).reshape(())
    return row


class ImageStepMetrics(StepMetrics):
    """StepMetrics' sibling for the 2-D image-graph experiment: the graph branch of Inpainting2DTrainer logs l1, mse and piq's psnr
    of every step with one .item() each (trainers/inpainting2d_trainer.py:382-398; lpips needs a VGG and is out of scope).  ``update``
    is one HIP call (stin_image_metrics_f32, no host synchronisation) that writes a row of the ``[capacity, 8]`` device table:
    loss, l1, mse, psnr, then the number of masked pixels.  psnr has piq's semantics - the MEAN over the images of the batch of
    -10 log10(mse_b / data_range^2 + 1e-8) - not the whole-batch value of StepMetrics.  The mask is read as it is stored (bool or
    uint8): no int64 copy.  The images of a batch have equal sizes (sample.num_graphs of them).  Same update / rows / result
    surface, so TrainStep(metrics=ImageStepMetrics(...), use_mask_weighted_loss=False) records it."""

    KEYS = ('loss', 'l1', 'mse', 'psnr')

    def __init__(self, device, capacity=1024, data_range=2.0):
        super().__init__(device, capacity, use_mask_weighted_loss=False, data_range=data_range)

    def update(self, out, sample, loss=None, composite=True):
        """One step: ``out`` = the network output [N, C] (composite=True forms where(mask, out, color) itself), ``sample`` supplies
        color, mask and the number of images; ``loss`` = a loss computed elsewhere (0-dim tensor), else column l1 is copied.
        -> the row, a device view [8]."""
        out = out.detach()
        if out.dtype != torch.float32:
            out = out.float()
        color, mask = sample.color, sample.mask.reshape(-1)
        n, B = out.shape[0], int(sample.num_graphs)
        if n % B != 0:
            raise ValueError('%d rows are not %d images of equal size' % (n, B))
        if loss is not None and torch.is_tensor(loss):
            loss = loss.detach()
        if not out.is_cuda:
            row = self._row()
            row.copy_(_image_row_torch(out, color, mask, B, composite, self.data_range, loss))
            return row
        from . import _lib
        from .plan import _ptr, _stream
        out, ldo = SF._mat(out)
        color, _ = SF._mat(color if color.is_contiguous() else color.contiguous())
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        elif mask.dtype != torch.uint8:
            mask = (mask != 0).view(torch.uint8)
        if not mask.is_contiguous():
            mask = mask.contiguous()
        if loss is not None:
            loss = torch.as_tensor(loss)
            if loss.dtype != torch.float32 or loss.device != out.device:
                loss = loss.to(out.device, torch.float32)
        ws_bytes = _lib.load().stin_image_metrics_workspace_bytes(n, B)
        if self._ws is None or self._ws.numel() < ws_bytes:
            self._ws = torch.empty(ws_bytes, dtype=torch.uint8, device=out.device)
        row = self._row()
        SF._call('stin_image_metrics_f32', _ptr(out), ldo, _ptr(color), _ptr(mask), n, B, out.shape[1], int(bool(composite)),
                 self.data_range, _ptr(loss), _ptr(row), _ptr(self._ws), self._ws.numel(), _stream(out))
        return row


def evaluate(model, samples, tracker=None, **tracker_kw):
    """The body of the trainer's _valid_epoch / _eval (:204-252, :89-125): eval mode, no_grad, one tracker row per sample;
    the previous train / eval mode is restored.  -> the tracker (per-scene losses: ``tracker.rows()[:, 0]``)."""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for sample in samples:
                if tracker is None:
                    tracker = StepMetrics(sample.color.device, **tracker_kw)
                tracker.update(model(sample), sample)
    finally:
        model.train(was_training)
    if tracker is None:
        tracker = StepMetrics(next(model.parameters()).device, **tracker_kw)
    return tracker
