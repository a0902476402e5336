"""The trainer-side harness around the hot path: gradient accumulation, optimizer state in
torch.optim.Adam's layout, LR schedulers, size-balanced rank sharding, the self-launching multi-rank bench, the
segmented (overlapped) all-reduce and torch.utils.checkpoint compatibility of the fused block.

CPU tests use the oracle as the model (tests may); the harness code under test is the one bench.py runs over RCCL.
"""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

from oracle import stin_oracle
from surface_texture_inpainting_net_amd.loader import shard_indices
from surface_texture_inpainting_net_amd.synthetic import make_synthetic_mesh
from surface_texture_inpainting_net_amd.train_step import FlatAdam, FlatGradBucket, TrainStep, compute_loss, graph_forward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(input_nc=10, output_nc=3, ngf=8, filter_type='edgeconvtransinv', norm='instance', n_blocks=2, n_levels=1,
           pooling_type='max')
DEV = 'cuda:0'


# ------------------------------------------------------------------------------------------------- CPU: host logic
def test_size_balanced_sharding_covers_every_item_and_groups_similar_sizes():
    g = torch.Generator().manual_seed(1)
    for n, world in ((16, 4), (37, 8), (5, 2), (1201, 8)):
        sizes = (torch.rand(n, generator=g) * 350_000 + 50_000).tolist()
        for epoch in (0, 1):
            parts = [shard_indices(n, epoch, seed=3, rank=r, world_size=world, sizes=sizes) for r in range(world)]
            assert len({len(p) for p in parts}) == 1, 'every rank runs the same number of steps'
            seen = sorted(i for p in parts for i in p)
            assert set(seen) == set(range(n)) and len(seen) == (n + world - 1) // world * world
            # the ranks of one step get neighbours in size: no step mixes items more than one bucket apart in rank order
            order = sorted(range(n), key=lambda i: (-sizes[i], i))
            pos = {i: k for k, i in enumerate(order)}
            for step in range(len(parts[0])):
                ks = [pos[parts[r][step]] for r in range(world)]
                full = max(ks) - min(ks) < world or min(ks) // world != max(ks) // world     # wrap-around padding bucket
                assert full
            if n >= 3 * world:
                def mean_spread(pp):
                    return sum(max(sizes[pp[r][s]] for r in range(world)) - min(sizes[pp[r][s]] for r in range(world))
                               for s in range(len(pp[0]))) / len(pp[0])
                plain = [shard_indices(n, epoch, seed=3, rank=r, world_size=world) for r in range(world)]
                assert mean_spread(parts) < 0.5 * mean_spread(plain)      # (the one padded bucket wraps around to the largest)
        a = shard_indices(n, 0, 3, True, 0, world, sizes)
        assert a == shard_indices(n, 0, 3, True, 0, world, sizes)
    # no rank always draws the largest item of its bucket
    sizes = list(range(64, 0, -1))
    firsts = [sum(1 for s in range(8) if shard_indices(64, e, 0, True, r, 8, sizes)[s] % 8 == 0) for e in range(4) for r in range(8)]
    assert max(firsts) < 8 * 1 + 1 and len(set(firsts)) > 1


def test_train_step_accumulates_like_the_reference_loop():
    """Reference inpainting3d_trainer.py:170-177: loss / num_cum, backward every batch, optimizer step + zero_grad every
    num_cum-th batch."""
    k = 3
    scenes = [make_synthetic_mesh(200 + 40 * i, 2, seed=i, dilations=()) for i in range(2 * k)]
    torch.manual_seed(5)
    ref = stin_oracle.define_G(**CFG)
    torch.manual_seed(5)
    net = stin_oracle.define_G(**CFG)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3, amsgrad=True)
    step = TrainStep(net, lr=1e-3, amsgrad=True, accumulate=k)
    for i, s in enumerate(scenes):
        loss = compute_loss(graph_forward(ref, s), s.color, s.mask) / k
        loss.backward()
        if (i + 1) % k == 0:
            opt.step()
            opt.zero_grad(set_to_none=True)
        got = step(s)
        assert abs(float(got) / k - float(loss)) <= 1e-7
        for p, q in zip(net.parameters(), ref.parameters()):
            assert torch.allclose(p, q, rtol=0, atol=1e-7), i
    assert not torch.equal(next(iter(net.parameters())), next(iter(stin_oracle.define_G(**CFG).parameters())))


def test_flat_adam_state_dict_speaks_torch_adam_layout():
    torch.manual_seed(0)
    lin = torch.nn.Sequential(torch.nn.Linear(5, 4), torch.nn.Linear(4, 2))
    ref = torch.optim.Adam(lin.parameters(), lr=3e-4, amsgrad=True)
    for _ in range(3):
        lin(torch.randn(7, 5)).pow(2).sum().backward()
        ref.step()
        ref.zero_grad()
    sd = ref.state_dict()
    bucket = FlatGradBucket(lin.parameters())
    opt = FlatAdam(bucket, lr=1.0)
    assert isinstance(opt, torch.optim.Optimizer) and opt.state_dict()['state'] == {}
    opt.load_state_dict(sd)
    assert opt.step_count == 3 and opt.lr == 3e-4
    want = torch.cat([sd['state'][i]['exp_avg_sq'].reshape(-1) for i in range(4)])
    assert torch.equal(opt.exp_avg_sq, want)
    out = opt.state_dict()
    assert out['param_groups'][0]['params'] == [0, 1, 2, 3] and out['param_groups'][0]['amsgrad'] is True
    for i in range(4):
        for key in ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'):
            assert torch.equal(out['state'][i][key], sd['state'][i][key])
        assert float(out['state'][i]['step']) == 3.0
    fresh = torch.optim.Adam(lin.parameters(), lr=1.0, amsgrad=True)
    fresh.load_state_dict(out)                                   # torch accepts what FlatAdam emits
    assert fresh.param_groups[0]['lr'] == 3e-4
    # LR schedulers drive it like any optimizer (reference: StepLR(20000, 0.5) stepped per epoch)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5)
    opt.step_count, opt.step = 0, (lambda *a, **k: None)         # no HIP launch on the CPU: only the schedule is under test
    for _ in range(4):
        sched.step()
    assert abs(opt.lr - 3e-4 * 0.25) < 1e-12


def test_bench_refuses_a_world_size_mismatch_and_too_few_gpus():
    env = dict(os.environ, WORLD_SIZE='2', RANK='0', LOCAL_RANK='0')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '4'], env=env, capture_output=True, text=True)
    assert r.returncode == 2 and 'WORLD_SIZE=2 but --gpus 4' in r.stderr
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '64'], env=env, capture_output=True, text=True)
    assert r.returncode == 2 and 'RCCL needs one device per rank' in r.stderr


def _bench_outputs(stdout):
    """-> (compact line, detail object): rank 0 prints ONE compact JSON line whose `detail` key names the file with the full object."""
    lines = [ln for ln in stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, 'rank 0 prints ONE json line'
    assert len(lines[0]) < 4096
    line = json.loads(lines[0])
    return line, json.load(open(line['detail']))


def test_bench_compact_line_is_short_and_carries_the_contract_keys():
    """Round 5's line grew to 20 KB and the driver's bounded stdout tail lost its head (BENCH_r05.parsed null): the final line is built
    by bench.compact_line from the detail object, stays under 4 KB whatever the detail holds and carries the graded keys."""
    sys.path.insert(0, ROOT)
    import bench
    prose = 'x' * 5000
    detail = {'metric': 'vertices/sec forward+backward on 200k-vert ScanNet mesh; scatter-add GB/s vs HBM roofline', 'value': 27.7e6,
              'unit': 'vertices/s', 'n_gpus': 1, 'steps': 20, 'warmup': 3, 'ms_per_step': 7.2512345678, 'higher_is_better': True,
              'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
              'config': {'workload': prose, 'vertices_per_gpu': 200704, 'edges_per_gpu': 1200642, 'levels': 3, 'parallelism': 'dp1',
                         'hip_graph': False, 'crops_per_step': None, 'params': 1},
              'roofline': {'bound': 'hbm', 'kernel': 'stin_edge_relu_mean_fwd_f32[N=200704,E=1200642,H=128]', 'achieved': 6900.123456789,
                           'peak': 8000.0, 'unit': 'GB/s', 'frac': 0.8625, 'avg_us': 119.4, 'algorithmic_bytes': 825.85e6, 'traffic': 841e6,
                           'traffic_over_algorithmic': 0.996, 'traffic_unit': prose, 'convention': prose, 'selection': prose, 'each_us': [1.0] * 8},
              'cpu_baseline': {'value': 10274.0, 'unit': 'vertices/s', 'cores': 16, 'kind': 'port', 'cpu_model': 'AMD EPYC 9575F 64-Core Processor',
                               'sample_vertices': 200704, 'passes_s': [20.5, 19.5, 16.9], 'sample': prose, 'quick_sample': {'sample': prose}},
              'gemm_precision': {'fwd': 'fp16x3', 'bwd': 'bf16x3', 'note': prose},
              'exact_fp32': {'ms_per_step': 10.59, 'note': prose}, 'hbm_honest': {'frac_of_hbm_peak': 0.776, 'traffic_over_algorithmic': 1.015},
              'scatter_add': {'frac_of_hbm_peak': 0.616}, 'gpu_idle': {'idle_ms_per_step': 0.17, 'method': prose},
              'gemm': {'ms_per_step': 3.6, 'time_weighted_frac_of_roofline': 0.43, 'kernels': [{'note': prose}] * 24},
              'distributed': {'replicas_bit_identical': True, 'ms_per_step_per_rank': [7.25], 'allreduce_us': None},
              'edge_kernels': [{'note': prose}] * 6, 'dtype_tolerance': {'note': prose}, 'loss': 0.1234567891}
    text = bench.compact_line(detail, '/tmp/x.json')
    assert len(text) < 4096 and '\n' not in text
    line = json.loads(text)
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype',
              'data', 'config', 'roofline', 'cpu_baseline'):
        assert k in line, k
    assert line['metric'] == detail['metric'] and line['value'] == 27.7e6 and abs(line['ms_per_step'] - 7.25123) < 1e-9
    assert set(line['config']) >= {'workload', 'vertices_per_gpu', 'edges_per_gpu', 'levels', 'parallelism'} and 'model' not in line['config']
    assert set(line['roofline']) == {'bound', 'kernel', 'achieved', 'peak', 'unit', 'frac', 'avg_us', 'algorithmic_bytes', 'traffic',
                                     'traffic_over_algorithmic'}
    assert line['roofline']['bound'] == 'hbm' and abs(line['roofline']['frac'] - 0.8625) < 1e-9
    assert set(line['cpu_baseline']) == {'value', 'unit', 'cores', 'kind', 'cpu_model', 'sample_vertices', 'sample'}
    assert line['cpu_baseline']['kind'] == 'port' and len(line['cpu_baseline']['sample']) < 120
    assert line['exact_fp32_ms_per_step'] == 10.59 and line['hbm_honest_frac'] == 0.776 and line['scatter_add_frac'] == 0.616
    assert line['gpu_idle_ms'] == 0.17 and line['gemm_precision'] == 'fp16x3/bf16x3' and line['detail'] == '/tmp/x.json'
    assert all(len(v) < 200 for v in line.values() if isinstance(v, str))
    # a run without the secondary legs / the CPU leg: the keys stay, as nulls
    bare = {k: detail[k] for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'config', 'roofline')}
    line = json.loads(bench.compact_line(bare))
    assert line['cpu_baseline'] is None and line['exact_fp32_ms_per_step'] is None and line['roofline']['frac'] == 0.8625


def test_bench_dump_outputs_full_within_budget_and_a_seeded_sample_beyond(tmp_path):
    """bench.dump_outputs: loss (float64) + flat gradient bucket + flattened parameters (float32) in full while they fit the
    budget; beyond it the same fixed, seeded, ascending sample of entries of both, with the files inside the budget."""
    import types
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    torch.manual_seed(0)
    params = [torch.randn(300, 7), torch.randn(50)]
    step = types.SimpleNamespace(bucket=types.SimpleNamespace(flat=torch.randn(2150), params=params))
    flat_params = torch.cat([p.reshape(-1) for p in params])
    loss = torch.tensor(0.25)

    def load(d):
        return {n: np.load(os.path.join(d, n + '.npy')) for n in ('loss', 'grads', 'params')}

    bench.dump_outputs(str(tmp_path / 'full'), loss, step)
    full = load(str(tmp_path / 'full'))
    assert full['loss'].dtype == np.float64 and full['loss'].tolist() == [0.25]
    assert full['grads'].dtype == np.float32 and np.array_equal(full['grads'], step.bucket.flat.numpy())
    assert full['params'].dtype == np.float32 and np.array_equal(full['params'], flat_params.numpy())
    budget = 8 + 3 * 128 + 8 * 1000                                  # room for 1000 of the 2150 entries
    for tag in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / tag), loss, step, budget=budget)
    a, b = load(str(tmp_path / 'a')), load(str(tmp_path / 'b'))
    idx = bench.dump_sample_index(2150, 1000).numpy()
    assert len(idx) == 1000 and np.all(np.diff(idx) > 0)
    assert np.array_equal(a['grads'], step.bucket.flat.numpy()[idx]) and np.array_equal(a['params'], flat_params.numpy()[idx])
    assert all(np.array_equal(a[n], b[n]) for n in a) and a['loss'].tolist() == [0.25]
    assert sum(os.path.getsize(str(tmp_path / 'a' / (n + '.npy'))) for n in a) <= budget
    # the sample the default budget takes (5 levels: 537 MB of gradients + parameters) fits the 64 MB the option promises
    k = (bench.DUMP_BUDGET_BYTES - 8 - 3 * 128) // 8
    assert bench.DUMP_BUDGET_BYTES <= 64_000_000 and 8 + 3 * 128 + 8 * k <= bench.DUMP_BUDGET_BYTES


# ------------------------------------------------------------------------------------------------- GPU
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.gpu
def test_bench_plain_run_is_the_headline_alone_and_dumps_the_last_step(tmp_path):
    """A plain `bench.py --gpus 1` run: the contract keys are there, everything --full measures is null, no detail file is written,
    and --dump-outputs leaves loss (float64) and the flat gradient bucket / parameters (float32, one entry per parameter)."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    detail, dump = tmp_path / 'd.json', tmp_path / 'dump'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                        '--vertices', '3000', '--detail', str(detail), '--dump-outputs', str(dump)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line['steps'] == 3 and line['warmup'] == 1 and line['ms_per_step'] > 0 and line['value'] > 0
    assert line['unit'] == 'vertices/s' and line['higher_is_better'] is True and line['dtype'] == 'f32'
    assert line['detail'] is None and not detail.exists()
    assert line['cpu_baseline'] is None and all(v is None for v in line['roofline'].values())
    for k in ('exact_fp32_ms_per_step', 'hbm_honest_frac', 'scatter_add_frac', 'gpu_idle_ms', 'fwd_loss_bwd_only_ms',
              'inference_ms', 'edge_stage_ms_per_step', 'gemm_ms_per_step_standalone'):
        assert line[k] is None, k
    loss, grads, params = (np.load(str(dump / (n + '.npy'))) for n in ('loss', 'grads', 'params'))
    assert loss.dtype == np.float64 and loss.shape == (1,) and abs(float(loss[0]) - line['loss']) <= 1e-5 * abs(line['loss'])
    assert grads.dtype == np.float32 and params.dtype == np.float32 and grads.shape == params.shape == (4_202_051,)
    assert np.isfinite(grads).all() and np.isfinite(params).all() and np.abs(grads).max() > 0


@pytest.mark.gpu
def test_bench_self_launches_two_ranks_from_a_plain_python_invocation(tmp_path):
    """`python bench.py --gpus 2 --backend gloo` on a 1-GPU box: the parent starts two ranks itself, the line reports the
    all-reduced rank count, per-rank times, the all-reduce bracket and bit-identical replicas."""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--backend', 'gloo', '--full', '--steps', '3',
                        '--warmup', '1', '--vertices', '20000', '--no-cpu-baseline', '--detail', str(tmp_path / 'd.json')], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line, out = _bench_outputs(r.stdout)
    assert line['n_gpus'] == 2 and line['replicas_bit_identical'] is True and len(line['ms_per_step_per_rank']) == 2
    assert line['value'] == pytest.approx(out['value'], rel=1e-5) and line['config']['parallelism'] == 'dp2'
    assert out['n_gpus'] == 2 and out['distributed']['world_size'] == 2 and out['distributed']['backend'] == 'gloo'
    assert len(out['distributed']['ms_per_step_per_rank']) == 2 and out['distributed']['replicas_bit_identical'] is True
    assert out['distributed']['allreduce_us']['bytes'] == 4 * out['config']['params']
    assert out['value'] > 0 and abs(out['ms_per_step'] - max(out['distributed']['ms_per_step_per_rank'])) < 1e-6


@pytest.mark.gpu
def test_bench_eight_rank_self_launch_dry_run_on_one_gpu(tmp_path):
    """The 8-rank path the driver's scaling run takes (`python bench.py --gpus 8`), dry-run on ONE device with gloo: the
    self-launch (free port, 127.0.0.1 rendezvous), the core-affinity shares (cores // 8 per rank), OMP_NUM_THREADS, the
    all-reduced rank count, per-rank times and bit-identical replicas - everything but RCCL itself."""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '8', '--backend', 'gloo', '--full', '--steps', '2',
                        '--warmup', '1', '--vertices', '3000', '--no-cpu-baseline', '--detail', str(tmp_path / 'd.json')], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line, out = _bench_outputs(r.stdout)
    assert line['n_gpus'] == 8 and line['scaling'] == 'weak' and len(line['ms_per_step_per_rank']) == 8
    d = out['distributed']
    assert out['n_gpus'] == 8 and d['world_size'] == 8 and d['ranks_counted_by_allreduce'] == 8
    assert len(d['ms_per_step_per_rank']) == 8 and d['replicas_bit_identical'] is True
    ncpu = len(os.sched_getaffinity(0))
    assert d['cores_per_rank'] == max(1, ncpu // 8)
    assert out['scaling'] == 'weak' and out['config']['parallelism'] == 'dp8'
    assert abs(out['ms_per_step'] - max(d['ms_per_step_per_rank'])) < 1e-6
    assert abs(out['value'] - 8 * out['config']['vertices_per_gpu'] * out['steps'] / (out['ms_per_step'] * 1e-3 * out['steps'])) < 1e-3 * out['value']


@pytest.mark.gpu
def test_bench_two_rank_unequal_scenes_reports_the_straggler_figures(tmp_path):
    """`bench.py --gpus N --unequal-scenes` (round 5: BASELINE config 4 as the reference trains it - scenes of 150 k ... 200 k
    vertices, one per rank) on two gloo ranks sharing one device: the line carries the per-rank scene sizes, every rank's time inside
    the all-reduce bracket and north_star's 1 / 2 / 4 / 8 table row; replicas stay bit-identical."""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--backend', 'gloo', '--full', '--steps', '2', '--warmup', '1',
                        '--unequal-scenes', '--no-cpu-baseline', '--no-secondary', '--detail', str(tmp_path / 'd.json')], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    _, out = _bench_outputs(r.stdout)
    s, row = out['straggler'], out['scaling_table_row']
    assert s['vertices_per_rank'] == [150000, 200000] and len(s['allreduce_bracket_us_per_rank']) == 2
    assert all(v > 0 for v in s['allreduce_bracket_us_per_rank'])
    assert row['gpus'] == 2 and row['hbm_roofline_GBps'] == 16000.0 and 0 < row['frac_of_n_gpu_hbm_roofline'] < 1
    assert abs(row['vertices_per_s'] - out['value']) < 1e-6 * out['value'] and out['distributed']['replicas_bit_identical'] is True
    # the two ranks' scenes differ: value counts both (150 544 + 200 704 vertices per step)
    assert abs(out['value'] * out['ms_per_step'] * 1e-3 - (150544 + 200704)) < 1.0


def _scmn_xent(model, sample):
    return torch.nn.functional.cross_entropy(model(sample), sample.labels)


def _scmn_gpu_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from surface_texture_inpainting_net_amd.singleconvmeshnet import SingleConvMeshNet
    torch.manual_seed(3 + rank)                      # different init per rank: the flat broadcast must make the replicas equal
    net = SingleConvMeshNet(10, 1, [16, 32], num_classes=5).to(DEV)
    step = TrainStep(net, lr=1e-3, loss_fn=_scmn_xent)
    s = make_synthetic_mesh(2500 + 700 * rank, 2, seed=rank, dilations=()).to(DEV)
    s['labels'] = torch.randint(0, 5, (s.x.shape[0],), generator=torch.Generator().manual_seed(rank)).to(DEV)
    losses = [float(step(s)) for _ in range(3)]
    step.finish()
    torch.save({'loss': losses, 'grad': step.bucket.flat.cpu(), 'p': torch.cat([p.detach().reshape(-1) for p in net.parameters()]).cpu()},
               os.path.join(out_dir, 'scmn%d.pt' % rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_singleconvmeshnet_data_parallel_step_with_a_loss_hook(tmp_path):
    """TrainStep(loss_fn=cross entropy) around the HIP SingleConvMeshNet on two ranks (gloo, both on cuda:0): the reference's
    only multi-GPU model (trainers/segmentation_trainer.py:34-35, :139-148) on the flat-bucket all-reduce + FlatAdam step."""
    import torch.multiprocessing as mp
    mp.spawn(_scmn_gpu_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r = [torch.load(tmp_path / ('scmn%d.pt' % i)) for i in range(2)]
    assert torch.equal(r[0]['p'], r[1]['p']) and torch.equal(r[0]['grad'], r[1]['grad'])
    assert all(torch.isfinite(torch.tensor(x['loss'])).all() for x in r)
    assert r[0]['loss'][2] < r[0]['loss'][0]          # (three Adam steps on the same scene reduce its loss)


def _overlap_worker(rank, world, port, out_dir, min_bytes, mix=False, per_block=False):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    torch.cuda.set_device(0)
    if mix:
        # force the MIX the advisor flagged: every block takes the weight-gradient side stream except the ones above
        # max-work (here the level-0 decoder block), so a segment can be completed by a block that did not use the stream
        from surface_texture_inpainting_net_amd import functional as SF
        SF.WGRAD_MIN_WORK, SF.WGRAD_MAX_WORK = 0.0, 6e7
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from surface_texture_inpainting_net_amd import surfacetextureinpaintingnet as S
    cfg = dict(input_nc=10, output_nc=3, ngf=64, filter_type='edgeconvtransinv', norm='instance', n_blocks=3, n_levels=2,
               pooling_type='max', dilations=[1, 2, 1])
    torch.manual_seed(7)
    net = S.define_G(**cfg).to(DEV)
    step = TrainStep(net, lr=1e-3, overlap_allreduce_min_bytes=min_bytes)
    s = make_synthetic_mesh(3000 + 500 * rank, 3, seed=rank, dilations=(2,)).to(DEV)
    grads, segs, early = [], [], []
    from surface_texture_inpainting_net_amd import functional as SF2
    if per_block:                         # every fused block outside the bottleneck chain is a one-op node of its own: a segment
        SF2.USE_NET_CALL = False          # spans several nodes, each of which sees only its own blocks' events
    else:
        assert SF2.USE_NET_CALL, 'the test is about the whole-network node (functional.NetFn)'
    for _ in range(3):
        step.bucket.overlap_log = []
        step(s)
        torch.cuda.synchronize()
        grads.append(step.bucket.flat.clone().cpu())
        segs.append(len(step.bucket.segments or []))
        # segments whose all-reduce was handed over BEFORE the last backward kernel had completed on the GPU (event order):
        # the communication stream reached the segment's start marker earlier than the compute stream reached backward's end
        early.append(sum(1 for _, e in step.bucket.overlap_log if e.elapsed_time(step.bucket.backward_end) > 0.0))
    step.finish()
    torch.save({'grads': grads, 'segs': segs, 'early': early, 'p': torch.cat([p.detach().reshape(-1) for p in net.parameters()]).cpu()},
               os.path.join(out_dir, 'r%d_%d%s%s.pt' % (rank, min_bytes, '_mix' if mix else '', '_pb' if per_block else '')))
    dist.barrier()
    dist.destroy_process_group()


def _ddp_worker(rank, world, port, out_dir, use_ddp):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from surface_texture_inpainting_net_amd import functional as SF
    from surface_texture_inpainting_net_amd import surfacetextureinpaintingnet as S
    cfg = dict(input_nc=10, output_nc=3, ngf=32, filter_type='edgeconvtransinv', norm='instance', n_blocks=2, n_levels=1,
               pooling_type='max')
    torch.manual_seed(11)                                   # same initial weights on both ranks and in both modes
    net = S.define_G(**cfg).to(DEV)
    s = make_synthetic_mesh(2500 + 700 * rank, 2, seed=20 + rank, dilations=()).to(DEV)
    if use_ddp:
        ddp = torch.nn.parallel.DistributedDataParallel(net, device_ids=[0])
        loss = SF.masked_l1_loss(ddp(s), s.color, s.mask, True)
        loss.backward()
        torch.cuda.synchronize()
        grad = torch.cat([p.grad.reshape(-1) for p in net.parameters()]).cpu()
    else:
        step = TrainStep(net, lr=1e-3)
        loss = step.forward_backward(s, 1.0 / world)
        step.bucket.all_reduce(step.group)
        torch.cuda.synchronize()
        grad = step.bucket.flat.clone().cpu()
        step.finish()
    torch.save({'grad': grad, 'loss': float(loss)}, os.path.join(out_dir, '%s%d.pt' % ('ddp' if use_ddp else 'ts', rank)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_distributed_data_parallel_wrapper_equals_the_flat_bucket_step(tmp_path):
    """`torch.nn.parallel.DistributedDataParallel(model)` - how the reference's only multi-GPU user wraps its
    model (trainers/segmentation_trainer.py:34-35) - also works around this build's model: two ranks (gloo, both on cuda:0),
    unequal scenes; DDP's averaged gradients equal TrainStep's flat-bucket all-reduce bit for bit (two ranks: (a + b) / 2 ==
    a / 2 + b / 2 in binary floating point), and both ranks hold the same gradients.  Under DDP the blocks stay on one stream
    (its reducer hooks read a gradient as soon as autograd produces it)."""
    import torch.multiprocessing as mp
    for use_ddp in (True, False):
        mp.spawn(_ddp_worker, args=(2, _free_port(), str(tmp_path), use_ddp), nprocs=2, join=True)
    ddp = [torch.load(tmp_path / ('ddp%d.pt' % r)) for r in range(2)]
    ts = [torch.load(tmp_path / ('ts%d.pt' % r)) for r in range(2)]
    assert torch.equal(ddp[0]['grad'], ddp[1]['grad']) and torch.equal(ts[0]['grad'], ts[1]['grad'])
    assert float(ddp[0]['grad'].abs().max()) > 0
    assert torch.equal(ddp[0]['grad'], ts[0]['grad'])
    assert ddp[0]['loss'] == ts[0]['loss'] and ddp[1]['loss'] == ts[1]['loss']


@pytest.mark.gpu
def test_segmented_allreduce_during_backward_equals_the_single_tail_allreduce(tmp_path):
    """Two ranks (gloo, both on cuda:0): with a small segment size the bucket is reduced in pieces while the backward
    pass is still running; gradients and parameters must equal the single end-of-backward all-reduce."""
    import torch.multiprocessing as mp
    res = {}
    for min_bytes in (0, 256 << 10):
        mp.spawn(_overlap_worker, args=(2, _free_port(), str(tmp_path), min_bytes), nprocs=2, join=True)
        res[min_bytes] = [torch.load(tmp_path / ('r%d_%d.pt' % (r, min_bytes))) for r in range(2)]
    assert res[0][0]['segs'] == [0, 0, 0]
    assert res[256 << 10][0]['segs'][1] >= 2, 'segments are learned from the first step and used from the second on'
    # round 4: through the ONE-node backward (functional.NetFn / stin_net_bwd) the segments are launched behind per-block events
    # recorded inside the C call - at least two of them before the call's last kernel has completed on the GPU
    for r in range(2):
        assert res[256 << 10][r]['early'][1] >= 2 and res[256 << 10][r]['early'][2] >= 2, res[256 << 10][r]['early']
    for r in range(2):
        for a, b in zip(res[0][r]['grads'], res[256 << 10][r]['grads']):
            assert torch.equal(a, b)                      # two ranks: a + b is order-independent -> bit-identical
        assert torch.equal(res[0][r]['p'], res[256 << 10][r]['p'])
    assert torch.equal(res[0][0]['p'], res[0][1]['p']) and torch.equal(res[0][0]['grads'][2], res[0][1]['grads'][2])
    # blocks on and off the weight-gradient side stream inside one segment (STIN_WGRAD_MIN_WORK = 0, one block above
    # STIN_WGRAD_MAX_WORK): the segment's all-reduce must still wait for the side stream's newest event
    mp.spawn(_overlap_worker, args=(2, _free_port(), str(tmp_path), 256 << 10, True), nprocs=2, join=True)
    for r in range(2):
        mixed = torch.load(tmp_path / ('r%d_%d_mix.pt' % (r, 256 << 10)))
        assert mixed['segs'][1] >= 2
        for a, b in zip(res[0][r]['grads'], mixed['grads']):
            assert torch.equal(a, b)
        assert torch.equal(res[0][r]['p'], mixed['p'])
    # the same mix with every block a node of its own (USE_NET_CALL off): a segment completed by a block that stayed on the
    # compute stream holds gradients an EARLIER node left on the side stream - its all-reduce must wait for that stream too
    mp.spawn(_overlap_worker, args=(2, _free_port(), str(tmp_path), 256 << 10, True, True), nprocs=2, join=True)
    for r in range(2):
        mixed = torch.load(tmp_path / ('r%d_%d_mix_pb.pt' % (r, 256 << 10)))
        assert mixed['segs'][1] >= 2
        for a, b in zip(res[0][r]['grads'], mixed['grads']):
            assert torch.equal(a, b)
        assert torch.equal(res[0][r]['p'], mixed['p'])


@pytest.mark.gpu
def test_train_step_accumulation_on_the_gpu_matches_the_oracle_loop():
    from surface_texture_inpainting_net_amd import surfacetextureinpaintingnet as S
    cfg = dict(input_nc=10, output_nc=3, ngf=8, filter_type='edgeconvtransinv', norm='instance', n_blocks=2, n_levels=2,
               pooling_type='max', dilations=[1, 2])
    k = 2
    scenes = [make_synthetic_mesh(900 + 100 * i, 3, seed=i, dilations=(2,)) for i in range(2 * k)]
    torch.manual_seed(11)
    ref = stin_oracle.define_G(**cfg)
    net = S.define_G(**cfg)
    net.load_state_dict(ref.state_dict())
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3, amsgrad=True)
    step = TrainStep(net.to(DEV), lr=1e-3, amsgrad=True, accumulate=k)
    sched = torch.optim.lr_scheduler.StepLR(step.optimizer, step_size=1, gamma=0.5)
    sched_ref = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    for i, s in enumerate(scenes):
        (compute_loss(graph_forward(ref, s), s.color, s.mask) / k).backward()
        if (i + 1) % k == 0:
            if i + 1 == k:                                          # the accumulated gradient itself, before the update
                want = torch.cat([p.grad.reshape(-1) for p in ref.parameters()])
            opt.step()
            opt.zero_grad(set_to_none=True)
            sched_ref.step()
        step(s.to(DEV))
        if i + 1 == k:
            got = step.bucket.flat.cpu()
            assert float((got - want).abs().max()) <= 2e-5 * float(want.abs().max())
        if (i + 1) % k == 0:
            sched.step()
    step.finish()
    assert step.optimizer.lr == opt.param_groups[0]['lr'] == 1e-3 * 0.25
    for (name, p), q in zip(net.named_parameters(), ref.parameters()):
        # Adam normalises the step: |delta| ~ lr per entry, sign-stable except where the gradient is ~0
        assert float((p.detach().cpu() - q.detach()).abs().max()) <= 2.5e-3, name
    sd = step.optimizer.state_dict()
    assert float(sd['state'][0]['step']) == 2.0 and len(sd['state']) == len(list(net.parameters()))


@pytest.mark.gpu
@pytest.mark.parametrize('use_reentrant', [True, False])
def test_fused_block_survives_torch_checkpoint(use_reentrant):
    """The reference wraps 13 of its 15 blocks in torch.utils.checkpoint (models/surfacetextureinpaintingnet.py:429,438,
    451,454).  A caller doing the same to this build's fused block must get identical results."""
    from torch.utils.checkpoint import checkpoint
    from surface_texture_inpainting_net_amd import modules as M
    from surface_texture_inpainting_net_amd import surfacetextureinpaintingnet as S
    from surface_texture_inpainting_net_amd.plan import EdgeSet
    torch.manual_seed(3)
    n = 5000
    blk = S.GraphResnetBlock(64, 128, M.get_gcn_filter, M.FastInstanceNorm, False, True).to(DEV)
    blk2 = S.GraphResnetBlock(128, 128, M.get_gcn_filter, M.FastInstanceNorm, False, True).to(DEV)
    g = torch.Generator().manual_seed(4)
    ei = torch.randint(0, n, (2, 6 * n), generator=g).to(DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    edges = EdgeSet(ei, n, bad)
    x0 = torch.randn(n, 64, generator=g).to(DEV)

    def run(wrapped):
        for m in (blk, blk2):
            m.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        if wrapped:
            h = checkpoint(blk, x, edges, None, use_reentrant=use_reentrant, preserve_rng_state=False)
            y = checkpoint(blk2, h, edges, None, use_reentrant=use_reentrant, preserve_rng_state=False)
        else:
            y = blk2(blk(x, edges, None), edges, None)
        y.square().mean().backward()
        torch.cuda.synchronize()
        return y.detach().clone(), x.grad.clone(), [p.grad.clone() for m in (blk, blk2) for p in m.parameters()]

    y0, gx0, gp0 = run(False)
    for _ in range(2):                                   # twice: no state may leak from one checkpointed pass into the next
        y1, gx1, gp1 = run(True)
        assert torch.equal(y0, y1) and torch.equal(gx0, gx1)
        for a, b in zip(gp0, gp1):
            assert torch.equal(a, b)


@pytest.mark.gpu
def test_plan_prefetched_one_step_ahead_gives_the_same_training_run():
    """TrainStep.prefetch builds the next sample's CSR plan on side streams while the current step runs; the compute
    stream joins it at first use.  Losses and weights after 4 steps must equal the run that builds every plan in place."""
    from surface_texture_inpainting_net_amd import surfacetextureinpaintingnet as S
    cfg = dict(input_nc=10, output_nc=3, ngf=32, filter_type='edgeconvtransinv', norm='instance', n_blocks=3, n_levels=2,
               pooling_type='max', dilations=[1, 2, 4])
    meshes = [make_synthetic_mesh(3000 + 500 * i, 3, seed=20 + i, dilations=(2, 4)) for i in range(3)]

    def run(prefetch):
        torch.manual_seed(5)
        net = S.define_G(**cfg).to('cuda:0')
        step = TrainStep(net, lr=1e-3)
        samples = [m.to('cuda:0') for m in meshes]
        losses = []
        for k in range(4):
            s = samples[k % 3]
            s._plan_cache = None if not prefetch else s._plan_cache
            if prefetch and k == 0:
                step.prefetch(s)
            nxt = samples[(k + 1) % 3]
            nxt._plan_cache = None
            if prefetch:
                step.prefetch(nxt)                       # before the step that overlaps it is enqueued
                assert nxt._plan_cache is not None and nxt._plan_cache._pending
            losses.append(float(step(s)))
            assert not (s._plan_cache._pending)
        step.finish()
        return losses, [p.detach().clone() for p in net.parameters()]

    l0, w0 = run(False)
    l1, w1 = run(True)
    assert l0 == l1
    assert all(torch.equal(a, b) for a, b in zip(w0, w1))


@pytest.mark.gpu
@pytest.mark.parametrize('batched', [False, True])
def test_captured_step_equals_the_eager_step(batched):
    """TrainStep(graph=True): plan build + forward + loss + backward replayed as one HIP graph.  Same kernels in the same
    order on the same data -> losses and weights bit-identical to the eager run, also when the sample changes between
    replays (same signature, different indices / features) and when a second signature gets its own graph."""
    from surface_texture_inpainting_net_amd import surfacetextureinpaintingnet as S
    from surface_texture_inpainting_net_amd.data import collate
    cfg = dict(input_nc=10, output_nc=3, ngf=32, filter_type='edgeconvtransinv', norm='instance', n_blocks=3, n_levels=2,
               pooling_type='max', dilations=[1, 2, 4])

    def variants(seed, n):
        base = make_synthetic_mesh(n, 3, seed=seed, dilations=(2, 4))
        if batched:
            base = collate([base, make_synthetic_mesh(n // 2, 3, seed=seed + 50, dilations=(2, 4))])
        out = []
        for r in range(3):                              # same shapes: permuted edge order + different features
            g = torch.Generator().manual_seed(100 * seed + r)
            s = type(base)(**{k: base[k] for k in base.keys()})
            s._nv_host = getattr(base, '_nv_host', None)
            perm = torch.randperm(base.edge_index.shape[1], generator=g)
            s['edge_index'] = base.edge_index[:, perm].contiguous()
            s['x'] = base.x * (1.0 + 0.1 * r)
            out.append(s)
        return out

    seqs = variants(1, 3000) + variants(2, 3600)        # two signatures
    order = [0, 1, 2, 0, 3, 4, 5, 1, 3]

    def run(graph):
        torch.manual_seed(5)
        net = S.define_G(**cfg).to('cuda:0')
        step = TrainStep(net, lr=1e-3, graph=graph)
        samples = [s.to('cuda:0') for s in seqs]
        losses = [float(step(samples[i])) for i in order]
        step.finish()
        return losses, [p.detach().clone() for p in net.parameters()], step

    from surface_texture_inpainting_net_amd import functional as SF
    # (a per-kernel eager step between replays - what bench.py's bracketed steps are - must not invalidate what the graphs captured)
    def run_mixed():
        torch.manual_seed(5)
        net = S.define_G(**cfg).to('cuda:0')
        step = TrainStep(net, lr=1e-3, graph=True)
        samples = [s.to('cuda:0') for s in seqs]
        losses = []
        for n, i in enumerate(order):
            if n == 5:
                SF0.KernelTimer.start(['none'], max_records=4)
                step.graph = False
            losses.append(float(step(samples[i])))
            if n == 5:
                SF0.KernelTimer.stop()
                step.graph = True
        step.finish()
        return losses

    from surface_texture_inpainting_net_amd import functional as SF0
    l0, w0, _ = run(False)
    assert run_mixed() == l0
    l1, w1, st = run(True)
    assert sum(1 for v in st._captured.values() if v != 'warm') == 2
    assert l0 == l1, (l0, l1)
    old_min, SF.WGRAD_MIN_WORK = SF.WGRAD_MIN_WORK, 0.0     # ... and with the weight-gradient side stream forked inside the capture
    try:
        l1, w1, st = run(True)
    finally:
        SF.WGRAD_MIN_WORK = old_min
    assert l0 == l1, (l0, l1)
    assert all(torch.equal(a, b) for a, b in zip(w0, w1))


@pytest.mark.gpu
def test_captured_step_reports_out_of_range_indices():
    from surface_texture_inpainting_net_amd import surfacetextureinpaintingnet as S
    cfg = dict(input_nc=10, output_nc=3, ngf=16, filter_type='edgeconvtransinv', norm='instance', n_blocks=1, n_levels=1,
               pooling_type='max')
    torch.manual_seed(0)
    net = S.define_G(**cfg).to('cuda:0')
    step = TrainStep(net, graph=True)
    good = make_synthetic_mesh(2000, 2, seed=1).to('cuda:0')
    for _ in range(3):
        step(good)
    bad = type(good)(**{k: good[k] for k in good.keys()})
    bad._nv_host = good._nv_host
    ei = good.edge_index.clone()
    ei[0, 7] = good.x.shape[0] + 5
    bad['edge_index'] = ei
    step(bad)                                           # replay on the bad indices: the kernels leave the pair out
    with pytest.raises(IndexError):
        step.finish()
    # ... and the flag does not stick: the captured plan's flag is re-zeroed by every replay, so good samples after the bad
    # one report nothing (a pool word that kept its 1 would raise here for ever)
    for _ in range(3):
        step(good)
    step.finish()
    with pytest.raises(IndexError):                     # (reported by the next call whose flag copy has landed, finish() at the latest)
        step(bad)
        step(good)
        step.finish()
    step(good)
    step.finish()


@pytest.mark.gpu
def test_flag_pool_wraps_without_losing_or_inventing_reports(monkeypatch):
    """The eager plans' out-of-range flags are words of a round-robin pool: a word dirtied by a plan that never validated comes
    back clean when its half of the pool is entered again, and a plan built inside a capture does not take a pool word."""
    from surface_texture_inpainting_net_amd import plan as P
    monkeypatch.setattr(P, 'FLAG_POOL', 8)
    P._FLAG_POOLS.clear()
    dev = torch.device('cuda:0')
    words = [P._flag_word(dev) for _ in range(3)]
    words[1].fill_(1)                                    # a plan that saw a bad index and was dropped without validating
    seen = {w.data_ptr() for w in words}
    for _ in range(8):
        w = P._flag_word(dev)
        assert int(w.item()) == 0, 'a recycled word must be clean'
        seen.add(w.data_ptr())
    assert len(seen) == 8
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        inside = P._flag_word(dev)
    pool = P._FLAG_POOLS[dev.index][0]
    assert not (pool.data_ptr() <= inside.data_ptr() < pool.data_ptr() + 4 * 8)
    P._FLAG_POOLS.clear()


def test_graph_mode_guards_and_sample_signature():
    """Host logic of TrainStep(graph=True) that needs no GPU: it refuses CPU models and gradient accumulation, and the capture
    key separates samples by tensor shapes / dtypes and by the per-graph level sizes, not by tensor contents."""
    from surface_texture_inpainting_net_amd.train_step import _sample_signature
    net = stin_oracle.define_G(input_nc=10, output_nc=3, ngf=8, filter_type='edgeconv', norm='instance', n_blocks=1, n_levels=1,
                               pooling_type='max')
    with pytest.raises(ValueError):
        TrainStep(net, graph=True)
    a = make_synthetic_mesh(300, 2, seed=1)
    b = make_synthetic_mesh(300, 2, seed=1)
    b['x'] = b.x * 2.0                                           # other contents, same signature
    c = make_synthetic_mesh(340, 2, seed=1)
    assert _sample_signature(a) == _sample_signature(b)
    assert _sample_signature(a) != _sample_signature(c)
    d = make_synthetic_mesh(300, 2, seed=1)
    d['num_vertices'] = d.num_vertices + 0                       # same values
    d._nv_host = None
    assert _sample_signature(a)[1] == _sample_signature(d)[1]
