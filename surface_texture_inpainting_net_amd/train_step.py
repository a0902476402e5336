"""The training step the reference's Inpainting3DTrainer runs around the hot path
(trainers/inpainting3d_trainer.py:127-137, :156-177, :199-201), restated for one process per GPU:

    out  = model(data)                                   # the HIP hot path
    pred = where(mask > 0, out, color)
    loss = mean(|pred - color| * 0.99 ** mask)           # use_mask_weighted_loss
    (loss / num_cumulated_train_batches).backward()      # gradients accumulate over `accumulate` scenes (:170-172)
    every `accumulate`-th scene: [all-reduce grads]; Adam(lr 7e-5, wd 0, amsgrad).step(); zero_grad(set_to_none)
    lr_scheduler.step() per epoch (StepLR(20000, 0.5), :199-201) -> works on TrainStep.optimizer / set_lr()

Data parallelism (new in this build; the reference asserts n_gpu == 1): one scene per rank, ONE
flat fp32 gradient bucket summed with RCCL over xGMI (torch.distributed backend "nccl"); the 1 / world factor rides on
the loss gradient (exact for 2 / 4 / 8 ranks), so the all-reduced bucket IS the mean of per-scene means - the
reference's num_cumulated_train_batches semantics (:170-177) - without a separate division pass.  Large buckets (the
67 M-parameter 5-level network: 268 MB) are reduced in segments as the backward pass completes them, on RCCL's own
stream beside the remaining backward kernels (FlatGradBucket.enable_overlap).
"""
import torch
import torch.distributed as dist


def graph_forward(model, data):
    out = model(data)
    return torch.where((data.mask > 0).expand_as(data.color), out, data.color)


def compute_loss(output, target, weights=None):
    loss = (output - target).abs()
    if weights is not None:
        loss = loss * torch.pow(0.99, weights.squeeze()).unsqueeze(1)
    return loss.mean()


def _world(group=None):
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(group)
    return 1


class FlatGradBucket:
    """All parameter gradients as views into ONE contiguous fp32 buffer (16.8 MB for the 3-level
    config): a single large all-reduce per step instead of 74 small ones."""

    def __init__(self, params):
        self.params = [p for p in params if p.requires_grad]
        n = sum(p.numel() for p in self.params)
        dev = self.params[0].device
        self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
        self.views, self.offsets = [], []
        off = 0
        for i, p in enumerate(self.params):
            v = self.flat[off:off + p.numel()].view_as(p)
            self.views.append(v)
            self.offsets.append(off)
            p.grad = v
            off += p.numel()
            if dev.type == 'cuda':
                # the whole-block backward (functional.NetFn) writes this parameter's gradient straight
                # into its bucket view while the bucket is `accepting`, instead of handing a fresh tensor to autograd
                p._stin_slot = (self, i)
        self.accepting = False
        self.written = [False] * len(self.params)
        self.acc = None                       # gradient accumulation over several backward passes (TrainStep(accumulate=k))
        # overlapped all-reduce (enable_overlap): segments = contiguous parameter ranges [lo, hi) in the order the
        # backward pass completes them (reverse parameter order), each reduced as soon as its last gradient is written
        self.overlap_min_bytes = None
        self.segments = None
        self._seg_next = 0
        self._seg_work = []
        self._group = None
        self._comm_stream = None
        self.allreduce_log = None             # list: (start, end) HIP events of the end-of-backward all-reduces (bench: allreduce_us)
        self.overlap_log = None               # list: (segment, HIP event on the communication stream in front of its all-reduce)
        self.backward_end = None              # with overlap_log: HIP event on the compute stream behind the last backward kernel

    def zero(self):
        self.flat.zero_()
        for p, v in zip(self.params, self.views):  # re-attach (zero_grad(set_to_none=True) safe)
            p.grad = v

    def detach_grads(self):
        """Before backward: leave .grad unset so autograd STORES each gradient instead of launching one
        accumulate-add per parameter (74 tiny kernels per step)."""
        for p in self.params:
            p.grad = None
        self.written = [False] * len(self.params)
        self.accepting = True
        self._seg_next = 0
        self._seg_work = []

    def gather_grads(self):
        """After backward: copy all gradients into the flat bucket with one multi-tensor copy and point
        .grad back at the bucket views (parameters without a gradient get zeros)."""
        self.accepting = False
        views, grads = [], []
        for i, p in enumerate(self.params):
            v = self.views[i]
            if p.grad is not None:
                if self.written[i]:
                    raise RuntimeError('a parameter received a gradient both directly in its bucket view and through autograd '
                                       '(a weight used by two blocks?): unsupported by the direct-write path')
                views.append(v)
                grads.append(p.grad)
            elif not self.written[i]:
                v.zero_()
            p.grad = v
        if views:
            torch._foreach_copy_(views, grads)

    # ---- gradient accumulation (reference :170-177) -------------------------------------------------------------------
    def accumulate(self, first, last):
        """Called after gather_grads() of every micro-batch of an accumulation window: the direct-write path OVERWRITES
        the bucket, so the running sum lives in `acc` (same left-to-right summation order as autograd's `.grad +=`)."""
        if first and last:
            return
        if self.acc is None:
            self.acc = torch.empty_like(self.flat)
        if first:
            self.acc.copy_(self.flat)
        elif last:
            torch.add(self.acc, self.flat, out=self.flat)
        else:
            self.acc.add_(self.flat)

    # ---- all-reduce -----------------------------------------------------------------------------------------------------
    def enable_overlap(self, group=None, min_bytes=32 << 20):
        """Reduce the bucket in segments of >= min_bytes while the backward pass is still running.  The segments are
        learned from the first step (which parameters the block backward writes directly); a bucket smaller than
        2 * min_bytes keeps the single tail all-reduce (16.8 MB at 3 levels: ~100 us, nothing to hide)."""
        self.overlap_min_bytes = int(min_bytes)
        self._group = group
        if self.flat.is_cuda and self._comm_stream is None:
            self._comm_stream = torch.cuda.Stream(device=self.flat.device)

    def _learn_segments(self):
        """Runs of directly written parameters, walked in reverse parameter order (= completion order of the backward
        pass), cut into segments of >= overlap_min_bytes.  Parameters that reach the bucket through autograd (the tail
        Linears, generic filters) are copied in by gather_grads() after backward and belong to the tail all-reduce."""
        segs, hi, nbytes = [], None, 0
        for i in range(len(self.params) - 1, -1, -1):
            if not self.written[i]:
                hi, nbytes = None, 0
                continue
            if hi is None:
                hi, nbytes = i + 1, 0
            nbytes += self.params[i].numel() * 4
            if nbytes >= self.overlap_min_bytes:
                segs.append((i, hi))
                hi, nbytes = None, 0
        total = self.flat.numel() * 4
        self.segments = segs if total >= 2 * self.overlap_min_bytes else []

    def _seg_slice(self, seg):
        lo, hi = seg
        return self.flat[self.offsets[lo]:self.offsets[hi - 1] + self.params[hi - 1].numel()]

    def wants_block_events(self):
        """True while segments are waiting to be reduced during this backward pass: functional.NetFn then asks stin_net_bwd for one
        completion event per block."""
        return bool(self.segments) and self._seg_next < len(self.segments) and self.accepting and _world(self._group) > 1

    def blocks_done(self, items, side_event=None):
        """functional.NetFn.backward, after ONE C call has enqueued the backward kernels of every block of the node: items =
        [(parameter slot indices of a block, the event recorded when that block's gradient writes are complete, or None)].
        Each segment whose parameters are all written goes to RCCL on the communication stream behind the events of exactly its
        blocks - NOT behind the compute stream's current position, which would be the end of the whole backward pass (the
        round-3 regression).  A segment that also holds parameters written by an earlier node (every block its own node: a
        segment spans several) has no event for those: it waits for the compute stream's position AND for `side_event`, the
        weight-gradient side stream's newest event while any block of this backward pass has work there (else None) - the
        block completing the segment may have stayed on the compute stream while an earlier one did not."""
        if not self.segments or self._seg_next >= len(self.segments) or _world(self._group) == 1:
            return
        ev_of = {}
        for idxs, ev in items:
            for i in idxs:
                ev_of[i] = ev
        dev = self.flat.device
        cs = self._comm_stream
        while self._seg_next < len(self.segments):
            lo, hi = self.segments[self._seg_next]
            if not all(self.written[lo:hi]):
                break
            if all(i in ev_of and ev_of[i] is not None for i in range(lo, hi)):
                for ev in {id(ev_of[i]): ev_of[i] for i in range(lo, hi)}.values():
                    cs.wait_event(ev)
            else:                                                # a parameter written by some other node: the conservative order
                cs.wait_stream(torch.cuda.current_stream(dev))
                if side_event is not None:
                    cs.wait_event(side_event)
            if self.overlap_log is not None:
                e = torch.cuda.Event(enable_timing=True)
                e.record(cs)
                self.overlap_log.append((self._seg_next, e))
            with torch.cuda.stream(cs):
                w = dist.all_reduce(self._seg_slice((lo, hi)), op=dist.ReduceOp.SUM, group=self._group, async_op=True)
            self._seg_work.append(w)
            self._seg_next += 1

    def all_reduce(self, group=None, timed=False):
        """Sum the bucket over the ranks (the loss gradient already carries 1 / world).  Segments launched during the
        backward pass are only waited for; the rest of the bucket goes out in contiguous pieces now."""
        if _world(group) == 1:
            return
        done = self.segments[:self._seg_next] if self.segments else []
        for w in self._seg_work:
            w.wait()                                            # the compute stream waits for RCCL's stream
        if self._comm_stream is not None and self._seg_work:
            torch.cuda.current_stream(self.flat.device).wait_stream(self._comm_stream)
        self._seg_work = []
        ev = None
        if timed and self.flat.is_cuda:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        if not done:
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=group)
        else:
            # the complement of the reduced segments, as contiguous flat ranges
            n = self.flat.numel()
            cuts = sorted((self.offsets[lo], self.offsets[hi - 1] + self.params[hi - 1].numel()) for lo, hi in done)
            at = 0
            for a, b in cuts + [(n, n)]:
                if a > at:
                    dist.all_reduce(self.flat[at:a], op=dist.ReduceOp.SUM, group=group)
                at = max(at, b)
        if ev is not None:
            ev[1].record()
            if self.allreduce_log is not None and len(self.allreduce_log) < 256:
                self.allreduce_log.append(ev)
        if self.overlap_min_bytes is not None and self.segments is None:
            self._learn_segments()

    def all_reduce_mean(self, group=None):
        """Stand-alone form (gradients NOT pre-scaled by 1 / world): sum, then divide."""
        if _world(group) > 1:
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=group)
            self.flat.div_(_world(group))


def broadcast_parameters(model, src=0, group=None):
    """Identical replicas: rank `src`'s parameters to every rank (one flat broadcast)."""
    if _world(group) == 1:
        return
    ps = [p.data for p in model.parameters()] + [b.data for b in model.buffers()]
    flat = torch.cat([p.reshape(-1).float() for p in ps])
    dist.broadcast(flat, src=src, group=group)
    off = 0
    for p in ps:
        p.copy_(flat[off:off + p.numel()].view_as(p).to(p.dtype))
        off += p.numel()


def replicas_identical(model, group=None):
    """SURVEY §8e validation: parameters bit-identical across ranks (rank 0's flat copy compared on every rank, the
    verdicts AND-reduced).  -> bool, the same on every rank."""
    if _world(group) == 1:
        return True
    ps = [p.data for p in model.parameters()]
    mine = torch.cat([p.reshape(-1).float() for p in ps])
    ref = mine.clone()
    dist.broadcast(ref, src=0, group=group)
    ok = torch.tensor([1 if torch.equal(mine.view(torch.int32), ref.view(torch.int32)) else 0], dtype=torch.int32,
                      device=mine.device)
    dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=group)
    return bool(int(ok.item()))


class FlatAdam(torch.optim.Optimizer):
    """Adam(amsgrad) over ONE flat parameter buffer: the parameters are re-pointed at views of `flat_p`, the moments
    live in flat buffers of the same size, and the update is a single HIP launch (stin_adam_f32) on the bucket's
    flat gradient - instead of torch's ~15 multi-tensor kernels per step.  Same arithmetic as
    torch.optim.Adam(lr, betas, eps, weight_decay, amsgrad) (bias corrections in double on the host like torch).

    A real torch.optim.Optimizer: `param_groups[0]['lr']` is what step() uses, so torch's LR schedulers (the reference's
    StepLR, inpainting3d_trainer.py:46-48, :199-201) drive it unchanged, and state_dict() / load_state_dict() speak
    torch.optim.Adam's per-parameter layout ('step', 'exp_avg', 'exp_avg_sq', 'max_exp_avg_sq' keyed by parameter
    index) - the 'optimizer' entry of a reference checkpoint (base_trainer.py:150, :199) loads and saves unchanged."""

    def __init__(self, bucket, lr=7e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=True):
        self.bucket = bucket
        self.flat_p = torch.empty_like(bucket.flat)
        off = 0
        for p in bucket.params:
            n = p.numel()
            self.flat_p[off:off + n].copy_(p.data.reshape(-1))
            p.data = self.flat_p[off:off + n].view_as(p)
            off += n
        self.exp_avg = torch.zeros_like(bucket.flat)
        self.exp_avg_sq = torch.zeros_like(bucket.flat)
        self.max_exp_avg_sq = torch.zeros_like(bucket.flat)
        self.step_count = 0
        super().__init__(bucket.params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad))
        if len(self.param_groups) != 1:
            raise ValueError('FlatAdam runs one parameter group')

    # the hyper-parameters live in param_groups[0] (schedulers write there); attribute access for convenience
    @property
    def lr(self):
        return self.param_groups[0]['lr']

    @lr.setter
    def lr(self, value):
        self.param_groups[0]['lr'] = float(value)

    def zero_grad(self, set_to_none=True):
        self.bucket.zero()

    @torch.no_grad()
    def step(self, closure=None):
        from . import functional as SF
        g = self.param_groups[0]
        self.step_count += 1
        SF.adam_step(self.flat_p, self.bucket.flat, self.exp_avg, self.exp_avg_sq, self.max_exp_avg_sq, g['lr'],
                     g['betas'][0], g['betas'][1], g['eps'], g['weight_decay'], self.step_count, g['amsgrad'])

    def _views(self, flat):
        out, off = [], 0
        for p in self.bucket.params:
            out.append(flat[off:off + p.numel()].view_as(p))
            off += p.numel()
        return out

    def state_dict(self):
        """torch.optim.Adam's layout: {'state': {i: {'step', 'exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'}}, 'param_groups'}
        (empty 'state' before the first step, like torch)."""
        groups = [{k: v for k, v in g.items() if k != 'params'} for g in self.param_groups]
        groups[0]['params'] = list(range(len(self.bucket.params)))
        state = {}
        if self.step_count > 0:
            m, v, vm = self._views(self.exp_avg), self._views(self.exp_avg_sq), self._views(self.max_exp_avg_sq)
            for i in range(len(self.bucket.params)):
                state[i] = {'step': torch.tensor(float(self.step_count)), 'exp_avg': m[i].clone(), 'exp_avg_sq': v[i].clone()}
                if self.param_groups[0]['amsgrad']:
                    state[i]['max_exp_avg_sq'] = vm[i].clone()
        return {'state': state, 'param_groups': groups}

    def load_state_dict(self, sd):
        groups = sd['param_groups']
        if len(groups) != 1 or len(groups[0]['params']) != len(self.bucket.params):
            raise ValueError('optimizer state_dict does not match the parameter list (%d groups, %d parameters expected)'
                             % (1, len(self.bucket.params)))
        for k, v in groups[0].items():
            if k != 'params':
                self.param_groups[0][k] = v
        state = sd['state']
        m, v, vm = self._views(self.exp_avg), self._views(self.exp_avg_sq), self._views(self.max_exp_avg_sq)
        steps = set()
        for buf in (self.exp_avg, self.exp_avg_sq, self.max_exp_avg_sq):
            buf.zero_()
        for j, i in enumerate(groups[0]['params']):
            st = state.get(i, state.get(str(i)))
            if st is None:
                continue
            steps.add(int(float(st['step'])))
            m[j].copy_(st['exp_avg'])
            v[j].copy_(st['exp_avg_sq'])
            if 'max_exp_avg_sq' in st:
                vm[j].copy_(st['max_exp_avg_sq'])
        if len(steps) > 1:
            raise ValueError('per-parameter step counts differ (%s): one flat update cannot continue them' % sorted(steps))
        self.step_count = steps.pop() if steps else 0


from .data import sample_keys as _keys  # noqa: E402


def _sample_signature(sample):
    """What a captured step depends on besides tensor CONTENTS: every tensor's name / shape / dtype and the per-graph level
    sizes (the host-side num_vertices table: instance-norm row ranges are built from it on the host)."""
    sig = []
    keys = _keys(sample)
    for k in sorted(keys):
        v = sample[k]
        if torch.is_tensor(v):
            sig.append((k, tuple(v.shape), str(v.dtype)))
        elif isinstance(v, (bool, int, float)):          # structural scalars; labels such as `name` do not shape the step
            sig.append((k, v))
    nv = getattr(sample, '_nv_host', None)
    if nv is None and 'num_vertices' in keys:
        nv = sample['num_vertices'].detach().cpu()            # foreign sample types: one host sync per step
    return tuple(sig), (None if nv is None else tuple(int(x) for x in nv.reshape(-1)))


class _CapturedStep:
    """plan build + forward + masked L1 + backward of ONE sample signature as a HIP graph: static input tensors the
    incoming sample is copied into, the loss tensor and the plan's out-of-range flag as outputs."""

    def __init__(self, owner, sample, grad_scale, pool):
        from .data import HierarchicalBatch
        from .plan import GraphPlan, check_deferred
        dev = owner.bucket.flat.device
        keys = _keys(sample)
        self.keys = [k for k in keys if torch.is_tensor(sample[k])]
        static = HierarchicalBatch(**{k: (sample[k].clone() if torch.is_tensor(sample[k]) else sample[k]) for k in keys})
        static._nv_host = getattr(sample, '_nv_host', None)
        if static._nv_host is None and 'num_vertices' in keys:
            static._nv_host = sample['num_vertices'].detach().cpu()
        self.static = static
        self.dst = [static[k] for k in self.keys]
        model = owner.model.module if hasattr(owner.model, 'module') else owner.model
        check_deferred(wait=True)                       # nothing of an earlier step may be polled from inside the capture
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, pool=pool):
            # the plan is part of the step (the sample's indices change from replay to replay); its index validation
            # cannot poll an event from inside a capture, so the flag is an output checked after every replay
            plan = GraphPlan(static, linspace_quirk=getattr(model, 'compat_linspace_norm', True), validate=False)
            static._plan_cache = plan
            self.loss = owner.forward_backward(static, grad_scale)
            self.bad = plan._bad
        self.keep = getattr(model, '_pack_set', None)   # the graph holds raw pointers into the model's packed-operand buffers
        # index validation: the plan's flag lives inside the capture (plan._flag_word: a memset node re-zeroes it at the start
        # of every replay), so replays add it into a running total; the total travels to pinned host memory whenever the
        # previous copy has landed (the host never waits)
        self.bad_total = torch.zeros(1, dtype=torch.int32, device=dev)
        self.flag_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.flag_event = None
        self.pool = self.graph.pool()

    def run(self, sample):
        src = [sample[k] for k in self.keys]
        if any(a.data_ptr() != b.data_ptr() for a, b in zip(self.dst, src)):
            torch._foreach_copy_(self.dst, src)
        self.graph.replay()
        self.bad_total.add_(self.bad)
        if self._check(wait=False):
            self.flag_host.copy_(self.bad_total, non_blocking=True)
            self.flag_event = torch.cuda.current_stream().record_event()
        return self.loss.clone()                        # the graph's own output tensor is overwritten by the next replay

    def _check(self, wait):
        """-> True when no flag copy is in flight any more (raises if one of the replays so far saw a bad index)."""
        if self.flag_event is not None:
            if not wait and not self.flag_event.query():
                return False
            self.flag_event.synchronize()
            self.flag_event = None
        if int(self.flag_host[0]) != 0:
            self.flag_host.zero_()
            self.bad_total.zero_()
            raise IndexError('edge / trace index out of range for the level sizes in sample.num_vertices '
                             '(reported after the captured step that used the sample)')
        return True

    def finish(self):
        self._check(wait=True)
        self.flag_host.copy_(self.bad_total, non_blocking=True)
        self.flag_event = torch.cuda.current_stream().record_event()
        self._check(wait=True)


class TrainStep:
    """model + Adam(amsgrad) + flat-bucket gradient all-reduce; ``step(sample) -> loss`` (a 0-dim
    tensor, no host sync).  On the GPU the loss (+ its gradient) and the optimizer update are one HIP
    kernel each; on the CPU (the gloo tests of the harness) the same arithmetic runs through torch.

    accumulate = the reference's num_cumulated_train_batches (:170-177): the loss of every call is divided by it, the
    gradients of `accumulate` consecutive calls are summed, and only the last call of a window all-reduces and runs the
    optimizer.  `optimizer` is a torch.optim.Optimizer either way (LR schedulers attach to it; set_lr() for manual
    schedules).

    graph=True (GPU, accumulate == 1): plan build + forward + loss + backward are captured into ONE HIP graph per sample
    signature (tensor shapes + per-graph level sizes) and replayed - ~420 kernel launches become one graph launch, which is
    what a launch-bound step (a 20k-vertex crop, a batch of crops) needs.  The first step of a signature runs eagerly
    (warm-up: lazy initialisations, host-side constants, index validation), the second captures, later ones copy the
    sample into the graph's input tensors and replay.  The gradient all-reduce and the Adam update stay outside the
    graph (Adam's bias corrections are host scalars that change every step).  Up to `graph_cache` signatures are kept
    (least recently used dropped), all in one memory pool.

    metrics = a metrics.StepMetrics: every call also records the trainer's seven step metrics (inpainting3d_trainer.py:254-271)
    as one row of the tracker's device table; the step itself - loss, gradients, parameters - is unchanged."""

    def __init__(self, model, lr=7e-5, weight_decay=0.0, amsgrad=True, use_mask_weighted_loss=True, group=None,
                 accumulate=1, overlap_allreduce_min_bytes=None, time_allreduce=False, graph=False, graph_cache=8,
                 loss_fn=None, freeze_gc=False, metrics=None):
        self.model = model
        # metrics (optional, a metrics.StepMetrics): one row of the trainer's seven step metrics per call, written on the device
        # right after the loss (every micro-step of an accumulation window: the reference logs every batch) - no host sync
        if metrics is not None and (loss_fn is not None or graph):
            raise ValueError('metrics= records the inpainting trainer\'s step metrics: it needs the default loss (loss_fn=None) '
                             'and an eager step (graph=False)')
        self.metrics = metrics
        # freeze_gc: the model, the optimizer state and whatever the data pipeline has built so far are long-lived; Python's
        # cyclic collector would otherwise re-scan that heap in the young-generation collections the ~100 k short-lived
        # objects of every step trigger, and its generation-2 passes land in the first tens of steps: measured at the
        # headline size 8.8 ms per step over the first 35 steps instead of 7.5 (host stalls of several ms while the GPU
        # drains its queue).  gc.freeze() moves everything alive now into the permanent generation (cycles created later are
        # still collected).  OPT-IN (round 4; bench.py opts in): it is a process-wide side effect, and an object frozen here that
        # later becomes cyclic garbage - an EARLIER TrainStep's parameter <-> bucket cycle in a sweep or k-fold run - would never
        # be collected; call gc.unfreeze() (or TrainStep.close()) when such a run drops a model.
        self._froze_gc = bool(freeze_gc)
        if freeze_gc:
            import gc
            gc.collect()
            gc.freeze()
        # loss_fn(model, sample) -> scalar loss: any other objective on the same flat-bucket / all-reduce / Adam step, e.g. the
        # segmentation trainer's cross entropy around SingleConvMeshNet (trainers/segmentation_trainer.py:139-148 - the
        # reference's only multi-GPU user).  None = the inpainting trainer's masked weighted L1 (the fused HIP loss kernel).
        self.loss_fn = loss_fn
        # overlap_allreduce_min_bytes (e.g. 32 << 20): reduce the bucket in segments of at least that size while backward is
        # still running (FlatGradBucket.enable_overlap).  OPT-IN since round 3: the path is tested bit-for-bit against the
        # single tail all-reduce with two gloo ranks on one GPU, but has never run over RCCL on more than one GPU.
        self.group = group
        self.use_mask_weighted_loss = use_mask_weighted_loss
        self.accumulate = max(1, int(accumulate))
        self._micro = 0
        self.time_allreduce = time_allreduce
        broadcast_parameters(model, 0, group)
        # a training loop must not stall the host once per step: out-of-range indices of a scene are reported by the
        # NEXT step (or by finish()) instead of inside the forward call that used them
        if hasattr(model, 'plan_validation'):
            model.plan_validation = 'deferred'
        self.bucket = FlatGradBucket(model.parameters())
        self.on_gpu = self.bucket.flat.is_cuda
        self.graph = bool(graph)
        if self.graph and not (self.on_gpu and self.accumulate == 1):
            raise ValueError('graph=True needs a GPU model and accumulate == 1')
        if self.graph:
            from . import graph_replay_safe
            GRAPH_REPLAY_SAFE = graph_replay_safe()
            import os
            if not GRAPH_REPLAY_SAFE or os.environ.get('DEBUG_CLR_GRAPH_PACKET_CAPTURE') != '0':
                raise RuntimeError('graph=True: ROCm 7.2 graph replays fault unless DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 is in the '
                                   'environment when the HIP runtime initialises (surface_texture_inpainting_net_amd/'
                                   '__init__.py): call surface_texture_inpainting_net_amd.enable_graph_replay() - or export '
                                   'STIN_GRAPH_REPLAY=1 / the variable itself - before the first GPU call')
        import collections
        self._captured = collections.OrderedDict()      # signature -> 'warm' | _CapturedStep
        self._graph_cache = max(1, int(graph_cache))
        self._graph_pool = None
        if self.on_gpu:
            self.optimizer = FlatAdam(self.bucket, lr=lr, weight_decay=weight_decay, amsgrad=amsgrad)
            if overlap_allreduce_min_bytes and _world(group) > 1 and self.accumulate == 1 and not self.graph:
                self.bucket.enable_overlap(group, overlap_allreduce_min_bytes)     # (RCCL calls are not captured)
        else:
            self.optimizer = torch.optim.Adam(self.bucket.params, lr=lr, weight_decay=weight_decay, amsgrad=amsgrad)

    def set_lr(self, lr):
        for g in self.optimizer.param_groups:
            g['lr'] = float(lr)

    def prefetch(self, sample):
        """Start building the CSR plan of a sample a LATER call will train on (the loader's next batch, already resident
        on the GPU): the build runs on the plan side streams beside the step being enqueued / executed and the compute
        stream waits for it only when that sample's forward starts."""
        model = self.model.module if hasattr(self.model, 'module') else self.model
        if getattr(sample, '_plan_cache', None) is None and hasattr(model, 'build_plan'):
            sample._plan_cache = model.build_plan(sample)
        return sample

    def forward_backward(self, sample, grad_scale=1.0):
        """One forward + loss + backward; the bucket then holds d(loss * grad_scale)/dw of THIS sample."""
        self.bucket.detach_grads()
        try:
            if self.loss_fn is not None:
                loss = self.loss_fn(self.model, sample)
            elif self.on_gpu:
                from . import functional as SF
                out = self.model(sample)
                loss = SF.masked_l1_loss(out, sample.color, sample.mask, self.use_mask_weighted_loss)
                if self.metrics is not None:
                    self.metrics.update(out.detach(), sample, loss=loss.detach())
            else:
                pred = graph_forward(self.model, sample)
                loss = compute_loss(pred, sample.color, sample.mask if self.use_mask_weighted_loss else None)
                if self.metrics is not None:            # (pred is already the composite; forming it again changes nothing)
                    self.metrics.update(pred.detach(), sample, loss=loss.detach())
            if grad_scale == 1.0:
                if self.loss_fn is None and self.on_gpu and loss.dtype == torch.float32 and loss.dim() == 0:
                    from . import functional as SF
                    loss.backward(SF.unit_seed(loss.device))     # (recognised by the fused loss: no seed fill, no multiply)
                else:
                    loss.backward()
            else:
                loss.backward(torch.full_like(loss, grad_scale))
        finally:
            self.bucket.accepting = False           # also when forward / backward raised: no stray direct writes later
            if self.on_gpu:
                from . import functional as SF
                SF.wgrad_side_settle(self.bucket.flat.device)   # an aborted backward never ran its end-of-backward join
                if self.bucket.overlap_log is not None:         # (tests / bench: where the backward pass ends on the compute stream)
                    self.bucket.backward_end = torch.cuda.Event(enable_timing=True)
                    self.bucket.backward_end.record()
        self.bucket.gather_grads()
        return loss.detach()

    def _graphed_forward_backward(self, sample, grad_scale):
        sig = _sample_signature(sample)
        ent = self._captured.get(sig)
        if ent is None:                                  # first visit: eager (also validates the indices the usual way)
            loss = self.forward_backward(sample, grad_scale)
            self._captured[sig] = 'warm'                 # only a COMPLETED eager step is a warm-up (lazy inits, constant uploads)
            while len(self._captured) > self._graph_cache:
                _, old = self._captured.popitem(last=False)
                if old != 'warm':
                    old.finish()                         # its replays' out-of-range flag is reported before the entry goes
            return loss
        self._captured.move_to_end(sig)
        if ent == 'warm':
            ent = self._captured[sig] = _CapturedStep(self, sample, grad_scale, self._graph_pool)
            if self._graph_pool is None:
                self._graph_pool = ent.pool
        return ent.run(sample)

    def close(self):
        """Undo the constructor's process-wide side effect (freeze_gc=True) and break the parameter <-> bucket cycle so that a
        dropped model's flat buffers are released by reference counting."""
        if self._froze_gc:
            import gc
            gc.unfreeze()
            self._froze_gc = False
        for p in self.bucket.params:
            if hasattr(p, '_stin_slot'):
                del p._stin_slot

    def finish(self):
        """Resolve the deferred index checks of the steps run so far (waits for the GPU)."""
        if self.on_gpu:
            from .plan import check_deferred
            check_deferred(wait=True)
            for ent in self._captured.values():
                if ent != 'warm':
                    ent.finish()

    def __call__(self, sample):
        k = self.accumulate
        first, last = self._micro == 0, self._micro == k - 1
        scale = 1.0 / (k * _world(self.group))
        loss = self._graphed_forward_backward(sample, scale) if self.graph else self.forward_backward(sample, scale)
        self.bucket.accumulate(first, last)
        self._micro = 0 if last else self._micro + 1
        if last:
            self.bucket.all_reduce(self.group, timed=self.time_allreduce)
            self.optimizer.step()
        return loss
