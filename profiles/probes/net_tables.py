"""The op tables functional.NetFn hands to stin_net_fwd / stin_net_bwd, the arena bytes and the backward scratch bytes, as JSON -
made comparable between two trees (profiles/r16_net_plan.md): run it in a checkout of each and diff the two files.

    python profiles/probes/net_tables.py OUT.json

It uses only what every tree since the stin_net_op_t records has: the functional._call spy, _lib.STRUCTS['stin_net_op_t'],
saved_tensors_hooks and a wrapped torch.empty (the arena and the scratch buffer are the node's 1-D uint8 allocations).  A field
value inside the arena becomes ['arena', offset], inside the backward scratch buffer ['scratch', offset], any other value of at
least 2^32 - a device pointer or an event handle - ['ext', order of first appearance within that call's table]; the rest stays
literal.  (Per call, not per case: all buffers of one table are alive together, while a tensor backward allocates may get the
address of one the forward's table named and autograd has freed since - which the allocator decides by event timing.)"""
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from surface_texture_inpainting_net_amd import _lib  # noqa: E402
from surface_texture_inpainting_net_amd import functional as SF  # noqa: E402
from surface_texture_inpainting_net_amd import surfacetextureinpaintingnet as S  # noqa: E402
from surface_texture_inpainting_net_amd.synthetic import make_synthetic_mesh  # noqa: E402

DEV = 'cuda:0'
OP = _lib.STRUCTS['stin_net_op_t']


class Capture:
    """While active: every stin_net_fwd / stin_net_bwd table of the process, decoded and normalised, in call order."""

    def __init__(self):
        self.calls, self.ext, self.arenas, self.saved, self.last_u8 = [], {}, [], [], None

    def _value(self, v, scratch):
        if not isinstance(v, int) or v < 2 ** 32:
            return v
        for p, n in self.arenas:
            if p <= v < p + n:
                return ['arena', v - p]
        if scratch is not None and scratch[0] <= v < scratch[0] + scratch[1]:
            return ['scratch', v - scratch[0]]
        return ['ext', self.ext.setdefault(v, len(self.ext))]

    def _spy(self, name, *a, **kw):
        if name in ('stin_net_fwd', 'stin_net_bwd'):
            raw, n = bytes(a[1].raw), int(a[2])
            self.ext = {}
            fwd = name == 'stin_net_fwd'
            if fwd:                         # the arena: the node's last 1-D uint8 allocation before the call
                self.arenas.append(self.last_u8)
            scratch = None if fwd else self.last_u8
            ops = [{f: self._value(v, scratch) for f, v in zip(OP.fields, struct.unpack(OP.format, raw[i * OP.size:(i + 1) * OP.size]))}
                   for i in range(n)]
            call = dict(name=name, storage=int(a[0]), n_ops=n, ops=ops)
            if fwd:
                call['arena_bytes'] = self.last_u8[1]
            else:
                call.update(scratch_bytes=scratch[1], g=self._value(int(a[3]), scratch), ldg=int(a[4]), prec_bwd=int(a[5]),
                            side_stream=int(a[7] != 0))
            self.calls.append(call)
        return self._call(name, *a, **kw)

    def _empty(self, *a, **kw):
        t = self._torch_empty(*a, **kw)
        if t.dtype == torch.uint8 and t.dim() == 1:
            self.last_u8 = (t.data_ptr(), t.numel())
        return t

    def _pack(self, t):
        if t.dtype == torch.uint8 and t.dim() == 1:
            self.saved.append((t.data_ptr(), t.numel()))
        return t

    def __enter__(self):
        self._call, self._torch_empty = SF._call, torch.empty
        SF._call, torch.empty = self._spy, self._empty
        self._hooks = torch.autograd.graph.saved_tensors_hooks(self._pack, lambda t: t)
        self._hooks.__enter__()
        return self

    def __exit__(self, *exc):
        self._hooks.__exit__(*exc)
        SF._call, torch.empty = self._call, self._torch_empty

    def result(self):
        """The calls; what the spy took for the arena of a training forward must be the 1-D uint8 tensor the node saved."""
        assert not self.saved or all(a in self.saved for a in self.arenas), (self.saved, self.arenas)
        return self.calls


def _cfg(filter_type, n_levels, n_blocks):
    return dict(input_nc=10, output_nc=3, ngf=64, filter_type=filter_type, norm='instance', n_blocks=n_blocks, n_levels=n_levels,
                pooling_type='max', dilations=[1, 2, 4][:n_blocks])


def _sample(batched, n_levels, dilations):
    from surface_texture_inpainting_net_amd.data import collate
    if batched:
        return collate([make_synthetic_mesh(n, n_levels + 1, seed=40 + i, dilations=dilations)
                        for i, n in enumerate((300, 450))]).to(DEV)
    return make_synthetic_mesh(700, n_levels + 1, seed=40, dilations=dilations).to(DEV)


def network_case(batched=False, grad=True, bf16=False, commute=True, wgrad_map=True, filter_type='edgeconvtransinv', n_levels=2,
                 n_blocks=2):
    s = _sample(batched, n_levels, (2, 4)[:n_blocks - 1])
    old = SF.USE_UNPOOL_COMMUTE, SF.USE_WGRAD_MAP
    SF.USE_UNPOOL_COMMUTE, SF.USE_WGRAD_MAP = commute, wgrad_map
    try:
        torch.manual_seed(17)
        net = S.define_G(**_cfg(filter_type, n_levels, n_blocks)).to(DEV)
        if bf16:
            net.set_activation_dtype(torch.bfloat16)
        with Capture() as cap:
            if grad:
                x = s.x.clone().requires_grad_(True)
                s2 = type(s)(**{k: (x if k == 'x' else s[k]) for k in s.keys()})
                s2._nv_host = s._nv_host
                net(s2).float().square().mean().backward()
            else:
                with torch.no_grad():
                    net(s)
            torch.cuda.synchronize()
        return cap.result()
    finally:
        SF.USE_UNPOOL_COMMUTE, SF.USE_WGRAD_MAP = old


def block_case(dim_in, dim_out):
    """One GraphResnetBlock on its own (a one-op node that packs for itself), forward and backward."""
    s = _sample(False, 2, (2,))
    torch.manual_seed(17)
    net = S.define_G(**_cfg('edgeconvtransinv', 2, 2)).to(DEV)
    blk = {(10, 64): net.input_blocks[0], (64, 64): net.output_blocks[0]}[(dim_in, dim_out)]
    assert (blk.dim_in, blk.dim_out) == (dim_in, dim_out) and blk._prepacked is None
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(s.x.shape[0], dim_in, generator=g, device=DEV).requires_grad_(True)
    with Capture() as cap:
        blk(x, s.edge_index).square().mean().backward()
        torch.cuda.synchronize()
    return cap.result()


def main(path):
    cases = {}
    for batched in (False, True):
        tag = 'batched' if batched else 'single'
        cases['train_' + tag] = network_case(batched)
        cases['no_grad_' + tag] = network_case(batched, grad=False)
        cases['bf16_' + tag] = network_case(batched, bf16=True)
        cases['no_commute_' + tag] = network_case(batched, commute=False)
        cases['no_wgrad_map_' + tag] = network_case(batched, wgrad_map=False)
    cases['edgeconv_3_levels'] = network_case(filter_type='edgeconv', n_levels=3, n_blocks=3)
    cases['block_10_64'] = block_case(10, 64)
    cases['block_64_64'] = block_case(64, 64)
    for name, calls in cases.items():
        assert calls, name
        print('%-24s %s' % (name, ', '.join('%s x%d' % (c['name'][9:], c['n_ops']) for c in calls)), flush=True)
    with open(path, 'w') as f:
        json.dump(cases, f, indent=1, sort_keys=True)
    print('wrote', path)


if __name__ == '__main__':
    main(sys.argv[1])
