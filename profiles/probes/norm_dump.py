"""Every output of the entry points of csrc/stin_norm.hip on seeded inputs, in one .npz - made comparable between two builds of
the library (profiles/r18_norm_once.md): run it once per build and compare the files byte for byte.

    STIN_LIB_PATH=/path/to/other/libstin_hip.so python profiles/probes/norm_dump.py A.npz
    python profiles/probes/norm_dump.py B.npz
    python profiles/probes/norm_dump.py --compare A.npz B.npz

The cases are the smallest that reach every branch: the one-launch column reduction at its three column-group widths (and a
partly live last group), the two-stage route at 4 and at 1 channels per lane, every mode and post-op, ranges that are empty, one
row long and no multiple of the rows in flight; the chunk-list folds at the boundaries of their pair / quad grouping and of their
256- and 512-entry trips; the fold-inside-the-launch forms; the elementwise passes at 1, 4 and 8 channels per lane."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from surface_texture_inpainting_net_amd import _lib  # noqa: E402
from surface_texture_inpainting_net_amd import functional as SF  # noqa: E402
from surface_texture_inpainting_net_amd.plan import _ptr, _stream  # noqa: E402

DEV = 'cuda:0'
FILL = -7.0                       # what an output holds where the kernel writes nothing
OUT = {}
MODE_NAMES = {SF.RED_SUM: 'sum', SF.RED_CSQ: 'csq', SF.RED_DOT_ELU: 'dot_elu', SF.RED_COEF_XC: 'coef_xc', SF.RED_MOMENTS: 'moments',
              SF.RED_DOT_BN: 'dot_bn', SF.RED_DOT_BN_RELU: 'dot_bn_relu'}
POST_NAMES = {SF.POST_NONE: 'none', SF.POST_SCALE: 'scale', SF.POST_RSTD: 'rstd', SF.POST_NORM_COEF: 'norm_coef'}


def keep(name, *tensors):
    torch.cuda.synchronize()
    for i, t in enumerate(tensors):
        t = t.view(torch.int16) if t.dtype == torch.bfloat16 else t
        assert name + '/%d' % i not in OUT, name
        OUT[name + '/%d' % i] = t.cpu().numpy()


class Rand:
    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def normal(self, *shape, scale=1.0, shift=0.0, dtype=torch.float32):
        return (torch.randn(*shape, generator=self.g) * scale + shift).to(DEV).to(dtype)

    def ints(self, hi, n):
        return torch.randint(0, hi, (n,), generator=self.g).to(torch.int32).to(DEV)


def filled(*shape, dtype=torch.float32):
    return torch.full(shape, FILL, dtype=dtype, device=DEV)


def colreduce(name, mode, post, x, ldx, C, cuts, rnd, gids=True):
    """One stin_colreduce call on the rows x[:, :C] (pitch ldx) over the ranges `cuts` (None: all rows, B = 1)."""
    N, dtype = x.shape[0], x.dtype
    B = len(cuts) - 1 if cuts is not None else 1
    ptr = torch.tensor(cuts, dtype=torch.int32, device=DEV) if cuts is not None else None
    lens = torch.tensor([b - a for a, b in zip(cuts, cuts[1:])] if cuts is not None else [N])
    inv = (1.0 / lens.clamp(min=1).double()).float().to(DEV)
    gid = sid = None
    if gids and cuts is not None:
        gid = torch.repeat_interleave(torch.arange(B), lens).to(torch.int32)
        gid = torch.cat([gid, torch.zeros(N - gid.numel(), dtype=torch.int32)]).to(DEV)
        sid = rnd.ints(B, N)
    bn = mode in (SF.RED_DOT_BN, SF.RED_DOT_BN_RELU)
    gout = rnd.normal(N, ldx, dtype=dtype) if mode == SF.RED_DOT_ELU or bn else None
    mean = rnd.normal(B, C, scale=0.2, shift=0.3)
    rstd = rnd.normal(B, C, scale=0.05, shift=0.6)
    coef = rnd.normal(2 if bn else B, C)
    out = filled(2, B, C)
    ws_bytes = _lib.load().stin_colreduce_workspace_bytes(C, B)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV)
    SF._call('stin_colreduce' + SF._sfx(x), mode, _ptr(x), ldx, _ptr(gout), ldx, N, C, _ptr(ptr), B, _ptr(gid),
             _ptr(sid if mode == SF.RED_COEF_XC else None), _ptr(mean), _ptr(rstd), _ptr(coef), post, _ptr(inv), float(SF.EPS),
             _ptr(out[0]), _ptr(out[1]), _ptr(ws), ws_bytes, _stream(x))
    keep('colreduce%s/%s/%s/%s' % (SF._sfx(x), name, MODE_NAMES[mode], POST_NAMES[post]), out)


POSTS = {SF.RED_SUM: (SF.POST_NONE, SF.POST_SCALE), SF.RED_CSQ: (SF.POST_NONE, SF.POST_SCALE, SF.POST_RSTD),
         SF.RED_DOT_ELU: (SF.POST_NONE, SF.POST_NORM_COEF), SF.RED_COEF_XC: (SF.POST_NONE,), SF.RED_MOMENTS: (SF.POST_NONE,),
         SF.RED_DOT_BN: (SF.POST_NONE, SF.POST_SCALE), SF.RED_DOT_BN_RELU: (SF.POST_NONE, SF.POST_SCALE)}


def colreduce_cases():
    rnd = Rand(1)
    N = 1000
    ragged, ragged_sum = [0, 613, 614, N], [0, 0, 1, N]      # one range of 1 row; SUM: one of 0 rows
    for C in (32, 36, 128, 256):                             # one launch: GC 16 / 16 with a partly live last group / 32 / 64
        x = rnd.normal(N, C, scale=1.7, shift=0.3)
        for mode, posts in POSTS.items():
            bn = mode in (SF.RED_DOT_BN, SF.RED_DOT_BN_RELU)
            for post in posts:
                colreduce('ticket_C%d' % C, mode, post, x, C, C, None if bn else (ragged_sum if mode == SF.RED_SUM else ragged), rnd)
    for C in (32, 256):                                      # bf16 rows
        x = rnd.normal(N, C, scale=1.7, shift=0.3, dtype=torch.bfloat16)
        for mode in (SF.RED_SUM, SF.RED_MOMENTS, SF.RED_DOT_ELU):
            colreduce('ticket_C%d' % C, mode, SF.POST_NONE, x, C, C, ragged_sum if mode == SF.RED_SUM else ragged, rnd)
    # two stages at 4 channels per lane: more (range, column group) pairs than ticket words
    B, C = 257, 32
    lens = torch.randint(2, 1200, (B,), generator=rnd.g)
    lens[1] = 1
    lens_sum = lens.clone()
    lens_sum[0] = 0
    x = rnd.normal(int(lens.sum()), C, scale=1.7, shift=0.3)
    for mode, post in ((SF.RED_SUM, SF.POST_SCALE), (SF.RED_CSQ, SF.POST_RSTD), (SF.RED_DOT_ELU, SF.POST_NORM_COEF),
                       (SF.RED_MOMENTS, SF.POST_NONE), (SF.RED_COEF_XC, SF.POST_NONE)):
        cuts = [0] + torch.cumsum(lens_sum if mode == SF.RED_SUM else lens, 0).tolist()
        colreduce('two_stage_B257', mode, post, x, C, C, cuts, rnd)
    # two stages at 1 channel per lane: rows that are no multiple of 4 channels / not 16-byte aligned
    C = 7
    for ldx in (C, C + 1):
        x = rnd.normal(N, ldx, scale=1.7, shift=0.3)
        for mode in (SF.RED_SUM, SF.RED_MOMENTS):
            colreduce('scalar_ld%d' % ldx, mode, SF.POST_NONE, x, ldx, C, ragged_sum if mode == SF.RED_SUM else ragged, rnd)


def finals_cases():
    rnd = Rand(2)
    for C in (20, 256):
        for groups in (1, 16, 17, 33, 63, 64, 65, 256, 257, 512, 513, 942):
            pm = torch.stack([rnd.normal(groups, C, scale=5.0).double(), rnd.normal(groups, C).double().abs() * 40 + 60], 1).contiguous()
            inv = torch.full((1,), 1.0 / (groups * 80), device=DEV)
            keep('moments_final/C%d/g%d' % (C, groups), *SF.moments_final(pm, inv))
            pb = rnd.normal(groups, 2, C, scale=3.0).double().contiguous()
            rstd = rnd.normal(1, C, scale=0.05, shift=0.6)
            keep('norm_coef_from_partials/C%d/g%d' % (C, groups), *SF.norm_coef_from_partials(pb, rstd, inv))


def fold_cases():
    rnd = Rand(3)
    lib = _lib.load()
    for N, C, groups in ((333, 32, 3), (5000, 64, 40), (1806, 256, 58)):
        assert lib.stin_norm_fold_rows(N, C, groups) > 0, (N, C, groups)
        x, res, go = rnd.normal(N, C, scale=1.7, shift=0.3), rnd.normal(N, C), rnd.normal(N, C)
        coarse, row_map = rnd.normal(N // 3 + 1, C), rnd.ints(N // 3 + 1, N)
        inv = torch.full((1,), 1.0 / N, device=DEV)
        cuts = torch.linspace(0, N, groups + 1).long().tolist()
        pm = torch.stack([torch.stack([x[a:b].double().sum(0), x[a:b].double().pow(2).sum(0)]) for a, b in zip(cuts, cuts[1:])]).contiguous()
        pb = rnd.normal(groups, 2, C, scale=3.0).double().contiguous()
        tag = 'N%d_C%d_g%d' % (N, C, groups)
        mean, rstd, y = filled(1, C), filled(1, C), filled(N, C)
        SF._call('stin_norm_act_res_fwd_fold_f32', _ptr(pm), groups, _ptr(x), C, _ptr(res), C, _ptr(inv), float(SF.EPS), N, C, _ptr(mean),
                 _ptr(rstd), _ptr(y), C, _stream(x))
        keep('fold_fwd/' + tag, mean, rstd, y)
        m2, r2, y2 = filled(1, C), filled(1, C), filled(N, C)
        SF._call('stin_norm_act_res_fwd_fold_map_f32', _ptr(pm), groups, _ptr(x), C, _ptr(coarse), C, _ptr(row_map), _ptr(inv),
                 float(SF.EPS), N, C, _ptr(m2), _ptr(r2), _ptr(y2), C, _stream(x))
        keep('fold_fwd_map/' + tag, m2, r2, y2)
        dx = filled(N, C)
        SF._call('stin_norm_act_bwd_fold_f32', _ptr(pb), groups, _ptr(x), C, _ptr(go), C, _ptr(mean), _ptr(rstd), _ptr(inv), N, C,
                 _ptr(dx), C, _stream(x))
        keep('fold_bwd/' + tag, dx)


def elementwise_cases():
    rnd = Rand(4)
    N, B = 333, 3
    for dtype in (torch.float32, torch.bfloat16):
        sfx = '_bf16' if dtype == torch.bfloat16 else '_f32'
        for C in ((7, 36, 64) if dtype == torch.float32 else (36, 64)):          # 1 / 4 / 4 (fp32), 4 / 8 (bf16) channels per lane
            x, res, go = (rnd.normal(N, C, scale=1.7, shift=0.3, dtype=dtype), rnd.normal(N, C, dtype=dtype),
                          rnd.normal(N, C, dtype=dtype))
            coarse, row_map = rnd.normal(N // 3 + 1, C, dtype=dtype), rnd.ints(N // 3 + 1, N)
            for with_gid in (False, True):
                G = B if with_gid else 1
                gid, sid = (rnd.ints(B, N), rnd.ints(B, N)) if with_gid else (None, None)
                mean, rstd = rnd.normal(G, C, scale=0.2, shift=0.3), rnd.normal(G, C, scale=0.05, shift=0.6)
                a, k, m = rnd.normal(G, C, shift=0.6), rnd.normal(G, C, scale=0.1), rnd.normal(G, C, scale=0.1)
                for act in (0, 1):
                    tag = '%s/C%d/gid%d/act%d' % (sfx[1:], C, with_gid, act)
                    for r in (None, res):
                        y = filled(N, C, dtype=dtype)
                        SF._call('stin_norm_act_res_fwd' + sfx, _ptr(x), C, _ptr(mean), _ptr(rstd), _ptr(gid), _ptr(r), C, N, C, act,
                                 _ptr(y), C, _stream(x))
                        keep('norm_fwd/%s/res%d' % (tag, r is not None), y)
                    if dtype == torch.float32:
                        y = filled(N, C)
                        SF._call('stin_norm_act_res_fwd_map_f32', _ptr(x), C, _ptr(mean), _ptr(rstd), _ptr(gid), _ptr(coarse), C,
                                 _ptr(row_map), N, C, act, _ptr(y), C, _stream(x))
                        keep('norm_fwd_map/' + tag, y)
                    dx = filled(N, C, dtype=dtype)
                    SF._call('stin_norm_act_bwd' + sfx, _ptr(x), C, _ptr(go), C, _ptr(mean), _ptr(rstd), _ptr(a), _ptr(k), _ptr(m),
                             _ptr(gid), _ptr(sid), N, C, act, _ptr(dx), C, _stream(x))
                    keep('norm_bwd/' + tag, dx)


def bn_cases():
    rnd = Rand(5)
    N, E = 333, 1200
    for C in (7, 32):
        x, go, edge_rows = rnd.normal(N, C, scale=1.7, shift=0.3), rnd.normal(N, C), rnd.normal(E, C, scale=1.7, shift=0.3)
        mean, rstd = rnd.normal(C, scale=0.2, shift=0.3), rnd.normal(C, scale=0.05, shift=0.6)
        gamma, beta, P, Q = rnd.normal(C, shift=1.0), rnd.normal(C, scale=0.3), rnd.normal(C), rnd.normal(C)
        dst = rnd.ints(N, E)
        inv_deg = 1.0 / torch.bincount(dst.long(), minlength=N).clamp(min=1).float()
        for act in (0, 1):
            y, dx = filled(N, C), filled(N, C)
            SF._call('stin_bn_act_fwd_f32', _ptr(x), C, _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), N, C, act, _ptr(y), C, _stream(x))
            SF._call('stin_bn_act_bwd_f32', _ptr(x), C, _ptr(go), C, _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(P), _ptr(Q),
                     1.0 / N, N, C, act, _ptr(dx), C, _stream(x))
            keep('bn/C%d/act%d' % (C, act), y, dx)
        dm = filled(E, C)
        SF._call('stin_bn_mean_bwd_f32', _ptr(edge_rows), C, _ptr(go), C, _ptr(dst), _ptr(inv_deg), _ptr(mean), _ptr(rstd), _ptr(gamma),
                 _ptr(P), _ptr(Q), 1.0 / E, E, C, _ptr(dm), C, _stream(x))
        run_mean, run_var = rnd.normal(C), rnd.normal(C).abs() + 0.5
        SF._call('stin_bn_running_stats_f32', _ptr(mean), _ptr(rstd), C, 1e-5, N / (N - 1), 0.1, _ptr(run_mean), _ptr(run_var), _stream(x))
        keep('bn/C%d/mean_bwd_running' % C, dm, run_mean, run_var)


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    assert sorted(a.files) == sorted(b.files), 'different case lists'
    differ = [k for k in a.files if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
    unwritten = [k for k in a.files if a[k].dtype == np.float32 and a[k].size and bool((a[k] == FILL).all())]
    print('%d arrays of %d cases: %d differ%s' % (len(a.files), len({k.rsplit('/', 1)[0] for k in a.files}), len(differ),
                                                   ''.join('\n  ' + k for k in differ)))
    print('arrays no kernel wrote to: %s' % (unwritten or 'none'))
    return 1 if differ else 0


def main(path):
    colreduce_cases()
    finals_cases()
    fold_cases()
    elementwise_cases()
    bn_cases()
    np.savez(path, **OUT)
    print('%s: %d arrays of %d cases, library %s' % (path, len(OUT), len({k.rsplit('/', 1)[0] for k in OUT}), _lib.LIB_PATH))


if __name__ == '__main__':
    if sys.argv[1] == '--compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main(sys.argv[1])
