"""Generate tests/golden/g19_levels*.npz by RUNNING THE REFERENCE'S OWN preprocessing/graph_level_generation.py.

Runs only where the reference tree exists (read-only; nothing is copied from it), through oracle/ref_import.load_preprocessing(),
in the manner of make_golden_crops.py.  The fixture holds DATA only (inputs, the CSV text as bytes, expected arrays):

  g19_levels.npz        the functions on synthetic contractions
    csv{k}.text/old/new/trace/gap      csv2npy: the decimator trace file (uint8 bytes), both vertex sets, the reference's trace
    cl.orig, cl.c{i}, cl.out{i}        get_color_and_labels
    fu.new/old/trace_in/trace_out      nearest_neighbor_interpolation_for_unassigned_traces
    err.{case}.text/old/new/raises     the cases csv2npy refuses (raises = 1) and the tolerated one (raises = 0, .trace)
  g19_levels.part{N}.npz  process_frame end to end, one scene per file, keys s{i}.*
    meta (json bytes: mode, train, levels, dilated, dists), mesh.vertices/faces/colors/normals, labels_raw, labels,
    lv{l}.vertices/faces/normals/csv   what the stand-in decimator handed the reference for level l (decimator mode)
    out.v{l}, out.e{l} (rows sorted by (row 0, row 1)), out.t{l}, out.dl{l}, out.d{l}.{j}, out.labels, gap

process_frame runs under in-memory stand-ins for the open3d mesh object and PlyData, and `quadric_error_metric` /
`trimesh_clustering` are replaced by a stand-in contraction (2 x 2 blocks of a jittered grid mesh) that returns a coarse triangle
mesh and writes the trace CSV: vcglib's tools do not exist here and the python around them is what the fixture pins.

Asserted here, because the tests lean on it: every nearest-neighbour query the reference made has a strictly positive gap between
the best and the second-best squared distance (the minimum is recorded) and the brute-force argmin of tests/_levels_oracle.py
gives the reference's answer; no two vertices of a level share a position; the CSVs have shuffled rows, ~6 significant digits,
>= 10 % unnamed old vertices and zero-trace rows; tests/_levels_oracle.py reproduces every expected array.

    python tests/tools/make_golden_levels.py            # rewrites tests/golden/g19_levels*.npz
"""
import glob
import json
import os
import sys
import tempfile
import types
import warnings

import numpy as np
import torch

_REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, _REPO)
sys.path.insert(0, os.path.join(_REPO, 'tests'))
warnings.filterwarnings('ignore')

from oracle import ref_import  # noqa: E402
import _levels_oracle as LO  # noqa: E402

OUT = os.path.join(_REPO, 'tests', 'golden')
MAX_FILE_BYTES = 1 << 20


# ------------------------------------------------------------------------------------------------ synthetic meshes
class Mesh:
    """In-memory stand-in for open3d.geometry.TriangleMesh (the attributes process_frame touches) + the grid coordinates the
    stand-in contraction works on."""

    def __init__(self, vertices, ij, colors=None):
        self.vertices = np.asarray(vertices, dtype=np.float64)
        self.ij = np.asarray(ij, dtype=np.int64)
        self.triangles = grid_faces(self.ij)
        self.vertex_colors = colors if colors is not None else np.zeros_like(self.vertices)
        self.vertex_normals = face_normals(self.vertices, self.triangles)

    def compute_vertex_normals(self):
        return self

    def has_vertices(self):
        return self.vertices.shape[0] > 0


def grid_faces(ij):
    side_i, side_j = ij[:, 0].max() + 1, ij[:, 1].max() + 1
    ids = np.full((side_i, side_j), -1, dtype=np.int64)
    ids[ij[:, 0], ij[:, 1]] = np.arange(ij.shape[0])
    a, b, c, d = ids[:-1, :-1].ravel(), ids[1:, :-1].ravel(), ids[:-1, 1:].ravel(), ids[1:, 1:].ravel()
    return np.concatenate([np.stack([a, b, d], 1), np.stack([a, d, c], 1)]).astype(np.int32)


def face_normals(v, f):
    n = np.zeros_like(v)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    for k in range(3):
        np.add.at(n, f[:, k], fn)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def make_mesh(side, seed, spacing=0.25):
    rng = np.random.default_rng(seed)
    gi, gj = np.meshgrid(np.arange(side), np.arange(side), indexing='ij')
    ij = np.stack([gi.ravel(), gj.ravel()], 1)
    ij = ij[rng.permutation(ij.shape[0])]
    xy = ij * spacing + rng.uniform(-0.3, 0.3, ij.shape) * spacing
    z = 0.4 * np.sin(xy[:, 0] * 1.3) * np.cos(xy[:, 1] * 0.9) + rng.normal(0, 0.02, ij.shape[0])
    return Mesh(np.column_stack([xy, z]), ij, rng.uniform(0, 1, (ij.shape[0], 3)))


def contract(mesh, rng, csv_path=None, drop=0.25, zero_rows=3):
    """2 x 2 grid blocks -> one coarse vertex each (near their centre of gravity), ids in random order; optionally the trace
    file: one row per coarse vertex in shuffled order, ~6 significant digits, members dropped at random (left to the nearest-
    neighbour fill), a few rows with no member at all."""
    cij = mesh.ij // 2
    side_j = cij[:, 1].max() + 1
    key = cij[:, 0] * side_j + cij[:, 1]
    uniq, inv = np.unique(key, return_inverse=True)
    perm = rng.permutation(uniq.shape[0])
    cluster = perm[inv]                                           # coarse id of every fine vertex
    nc = uniq.shape[0]
    pos = np.zeros((nc, 3))
    for k in range(3):
        pos[:, k] = np.bincount(cluster, weights=mesh.vertices[:, k], minlength=nc) / np.bincount(cluster, minlength=nc)
    pos += rng.normal(0, 0.004, pos.shape)
    ij = np.zeros((nc, 2), dtype=np.int64)
    ij[cluster] = cij
    coarse = Mesh(pos, ij)
    text = None
    if csv_path is not None:
        lines = []
        empty = set(rng.choice(nc, size=zero_rows, replace=False).tolist())
        for c in rng.permutation(nc):
            members = np.flatnonzero(cluster == c)
            keep = [] if c in empty else [m for m in members if rng.uniform() > drop]
            fields = ['%.6g' % x for x in pos[c]]
            for m in keep:
                fields += ['%.6g' % x for x in mesh.vertices[m]]
            lines.append(';'.join(fields))
        text = '\n'.join(lines) + '\n'
        with open(csv_path, 'w') as f:
            f.write(text)
    return coarse, text


# ------------------------------------------------------------------------------------------------ recording the reference
class Recorder:
    """Stands in for sklearn's BallTree inside the reference module: its answers, checked against the brute-force argmin, and the
    smallest gap between the best and the second-best squared distance over every query made."""
    gap = np.inf
    queries = 0

    def __init__(self, X):
        from sklearn.neighbors import BallTree
        self.X = np.array(X, dtype=np.float64)
        self.tree = BallTree(X)

    def query(self, Q, k=1):
        Q = np.asarray(Q, dtype=np.float64)
        dist, ind = self.tree.query(Q, k=k)
        mine, gap = LO.nearest(Q, self.X, return_gap=True)
        assert np.array_equal(mine, ind.reshape(-1)), 'argmin restatement differs from BallTree'
        assert gap > 0, 'nearest-neighbour tie in the fixture'
        Recorder.gap = min(Recorder.gap, gap)
        Recorder.queries += Q.shape[0]
        return dist, ind


def no_shared_positions(v, what):
    assert np.unique(np.asarray(v)[:, :3], axis=0).shape[0] == np.asarray(v).shape[0], 'two vertices of %s share a position' % what


def text_bytes(t):
    return np.frombuffer(t.encode(), dtype=np.uint8).copy()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ part 1: the functions
def run_functions(glg):
    d = {}
    glg.BallTree = Recorder
    with tempfile.TemporaryDirectory() as root:
        for k, (side, seed) in enumerate([(78, 11), (40, 12)]):
            Recorder.gap, Recorder.queries = np.inf, 0
            rng = np.random.default_rng(seed)
            fine = make_mesh(side, seed)
            path = os.path.join(root, 'c%d.csv' % k)
            coarse, text = contract(fine, rng, path)
            no_shared_positions(fine.vertices, 'the fine mesh')
            no_shared_positions(coarse.vertices, 'the coarse mesh')
            want = glg.csv2npy(path, fine.vertices, coarse.vertices)
            new_xyz, old_xyz, ptr = LO.read_trace_csv(text)
            counts = np.diff(ptr)
            named = np.unique(LO.nearest(old_xyz, fine.vertices)).shape[0]
            assert (fine.vertices.shape[0] - named) >= 0.1 * fine.vertices.shape[0], 'too few unnamed old vertices'
            assert (counts == 0).sum() >= 1, 'no zero-trace row'
            assert not np.array_equal(LO.nearest(new_xyz, coarse.vertices), np.arange(new_xyz.shape[0])), 'rows are not shuffled'
            assert np.abs(new_xyz - coarse.vertices[LO.nearest(new_xyz, coarse.vertices)]).max() > 0, 'coordinates match exactly'
            mine = LO.trace_from_rows((new_xyz, old_xyz, ptr), fine.vertices, coarse.vertices)
            assert np.array_equal(mine, want)
            p = 'csv%d.' % k
            d[p + 'text'], d[p + 'old'], d[p + 'new'] = text_bytes(text), fine.vertices, coarse.vertices
            d[p + 'trace'], d[p + 'gap'] = np.asarray(want, dtype=np.int32), np.asarray(Recorder.gap)
            print('csv2npy %d: %d -> %d vertices, %d unnamed, %d zero-trace rows, %d queries, min gap %.3e'
                  % (k, fine.vertices.shape[0], coarse.vertices.shape[0], fine.vertices.shape[0] - named, (counts == 0).sum(),
                     Recorder.queries, Recorder.gap))
            if k == 1:
                keep = (fine, coarse, text, want)
        fine, coarse, text, want = keep
        # get_color_and_labels and the unassigned fill, on the second contraction
        Recorder.gap = np.inf
        rng = np.random.default_rng(5)
        orig = np.column_stack([fine.vertices, fine.vertex_colors, fine.vertex_normals, np.arange(fine.vertices.shape[0]),
                                rng.integers(0, 21, fine.vertices.shape[0])])
        coarser, _ = contract(coarse, rng)
        reps = [fine.vertices, coarse.vertices, coarser.vertices.astype(np.float32)]
        outs = glg.get_color_and_labels(orig, reps)
        mine = LO.colors_and_labels(orig, reps)
        d['cl.orig'] = orig
        for i, (r, o, m) in enumerate(zip(reps, outs, mine)):
            assert same(o, m)
            d['cl.c%d' % i], d['cl.out%d' % i] = r, o
        t_in = np.array(want, dtype=np.int32)
        t_in[rng.uniform(size=t_in.shape[0]) < 0.2] = -1
        t_out = glg.nearest_neighbor_interpolation_for_unassigned_traces(coarse.vertices, fine.vertices, t_in.copy())
        assert np.array_equal(LO.fill_unassigned(coarse.vertices, fine.vertices, t_in), t_out)
        full = np.array(want, dtype=np.int32)
        assert np.array_equal(glg.nearest_neighbor_interpolation_for_unassigned_traces(coarse.vertices, fine.vertices, full.copy()), full)
        d['fu.new'], d['fu.old'], d['fu.trace_in'], d['fu.trace_out'] = coarse.vertices, fine.vertices, t_in, np.asarray(t_out, np.int32)
        d['fu.gap'] = np.asarray(Recorder.gap)
        # the cases csv2npy refuses, on a small contraction
        rng = np.random.default_rng(7)
        fine = make_mesh(12, 21)
        coarse, text = contract(fine, rng, os.path.join(root, 'e.csv'), drop=0.2, zero_rows=2)
        rows = text.strip('\n').split('\n')
        with_traces = [r for r in rows if r.count(';') >= 5]
        without = [r for r in rows if r.count(';') == 2]
        first = with_traces[0].split(';')
        cases = {
            # an old vertex named by two entries: the first old vertex of one row repeated at the end of another
            'old_twice': rows[:-1] + [rows[-1] + ';' + ';'.join(first[3:6])] if rows[-1] != with_traces[0] else
            rows[:-2] + [rows[-2] + ';' + ';'.join(first[3:6]), rows[-1]],
            # a row resolves to a new vertex that an earlier row WITH old vertices took
            'new_twice': rows + [';'.join(first[:3])],
            # the same new vertex twice, the earlier row WITHOUT old vertices: tolerated
            'new_twice_empty_first': [';'.join(first[:3])] + rows,
            # a zero-trace row taken out: its new vertex has no row; far away from every old vertex it is nobody's nearest
            'uncovered': None,
        }
        far_new = coarse.vertices.copy()
        victim = LO.nearest(LO.read_trace_csv(without[0] + '\n')[0], coarse.vertices)[0]
        far_new[victim] += np.array([0.0, 0.0, 50.0])
        for name, lines in cases.items():
            new_v = coarse.vertices
            if name == 'uncovered':
                lines, new_v = [r for r in rows if r != without[0]], far_new
            t = '\n'.join(lines) + '\n'
            path = os.path.join(root, name + '.csv')
            with open(path, 'w') as f:
                f.write(t)
            raised, got = 0, None
            try:
                got = glg.csv2npy(path, fine.vertices, new_v)
            except (glg.QEMError, AssertionError):
                raised = 1
            try:
                mine = LO.trace_from_rows(LO.read_trace_csv(t), fine.vertices, new_v)
                assert not raised and np.array_equal(mine, got), name
            except LO.LevelError:
                assert raised, name
            assert raised == (0 if name == 'new_twice_empty_first' else 1), (name, raised)
            p = 'err.%s.' % name
            d[p + 'text'], d[p + 'old'], d[p + 'new'], d[p + 'raises'] = text_bytes(t), fine.vertices, new_v, np.asarray(raised)
            if not raised:
                d[p + 'trace'] = np.asarray(got, dtype=np.int32)
            print('case %-22s raises=%d' % (name, raised))
    return d


# ------------------------------------------------------------------------------------------------ part 2: process_frame
SCENES = [
    # (side, seed, vertex_clustering, train, level_params, dilated_levels)
    dict(side=40, seed=31, vc=False, train=True, params=['100', '25', '25'], dilated=[0, 0, 1]),
    dict(side=32, seed=32, vc=False, train=False, params=['0.5', '25'], dilated=[0, 1]),
    dict(side=40, seed=33, vc=True, train=True, params=['0.4', '0.8', '1.6'], dilated=[0, 1, 0]),
]
DISTS = [2, 3, 4]


def run_scene(glg, idx, spec):
    store, records = {}, []
    rng = np.random.default_rng(spec['seed'] + 100)
    mesh = make_mesh(spec['side'], spec['seed'])
    n = mesh.vertices.shape[0]
    raw_labels = np.random.default_rng(spec['seed']).integers(0, 45, n)       # some beyond 40: the corrupted-id rule

    def read_mesh(path):
        return store[path]

    def write_mesh(path, m):
        store[path] = m
        return True

    def decimate(path, ratio):
        coarse, text = contract(store[path], rng, path.replace('.ply', '.csv'))
        store[path] = coarse
        records.append(dict(kind='qem', vertices=coarse.vertices, faces=coarse.triangles, normals=coarse.vertex_normals, csv=text))
        return coarse

    def system(cmd):
        if cmd.startswith('trimesh_clustering '):
            path = cmd.split()[1]
            coarse, _ = contract(store[path], rng)
            store[path] = coarse
            records.append(dict(kind='ext', vertices=coarse.vertices, faces=coarse.triangles, normals=coarse.vertex_normals))
            return 0
        raise AssertionError('unexpected command: ' + cmd)

    class Ply:
        @staticmethod
        def read(path):
            return {'vertex': {'label': raw_labels}}

    Recorder.gap, Recorder.queries = np.inf, 0
    glg.BallTree = Recorder
    glg.open3d = types.SimpleNamespace(io=types.SimpleNamespace(read_triangle_mesh=read_mesh, write_triangle_mesh=write_mesh))
    glg.PlyData = Ply
    glg.quadric_error_metric = decimate
    glg.graph_dilation.tqdm = lambda it: it
    real_system, cwd = os.system, os.getcwd()
    with tempfile.TemporaryDirectory() as root:
        os.chdir(root)
        os.system = system
        try:
            scene = 'scene%04d_00' % idx
            os.makedirs(os.path.join('in', scene))
            os.makedirs('out')
            file_path = 'in/%s/%s_vh_clean_2.ply' % (scene, scene)
            store[file_path] = mesh
            glg.args = types.SimpleNamespace(level_params=list(spec['params']), dilated_levels=[str(x) for x in spec['dilated']],
                                             dilation_dists=list(DISTS), train=spec['train'], dataset='scannet', out_path='out/',
                                             vertex_clustering=spec['vc'], verbose_out_path=None)
            import contextlib
            import io
            with contextlib.redirect_stdout(io.StringIO()):
                glg.process_frame(file_path, global_params={'mapping': {}})
            ref = torch.load('out/%s.pt' % scene, weights_only=False)
        finally:
            os.system = real_system
            os.chdir(cwd)
    assert Recorder.gap > 0
    # ---- the same scene as this project's interface takes it
    levels, rec = [], iter(records)
    for prm in spec['params']:
        if spec['vc']:
            levels.append(float(prm))
        elif prm == '100':
            levels.append('100')
        else:
            r = next(rec)
            assert r['kind'] == ('qem' if prm.isdigit() else 'ext')
            levels.append({k: v for k, v in r.items() if k != 'kind'})
    labels = LO.remap_scannet_labels(raw_labels) if spec['train'] else None
    m = dict(vertices=mesh.vertices, faces=mesh.triangles, colors=mesh.vertex_colors, normals=mesh.vertex_normals)
    mine = LO.graph_levels(m, levels, spec['dilated'], list(DISTS), labels=labels, reference_vc_normals=True)
    p = 's%d.' % idx
    d = {p + 'meta': text_bytes(json.dumps(dict(vc=spec['vc'], train=spec['train'], dilated=spec['dilated'], dists=DISTS,
                                                 levels=[x if not isinstance(x, dict) else ('qem' if 'csv' in x else 'ext')
                                                         for x in levels]))),
         p + 'gap': np.asarray(Recorder.gap), p + 'labels_raw': raw_labels.astype(np.int32)}
    for k, v in m.items():
        d[p + 'mesh.' + k] = v
    if labels is not None:
        d[p + 'labels'] = labels.astype(np.int32)
    for l, x in enumerate(levels):
        if isinstance(x, dict):
            for k, v in x.items():
                d[p + 'lv%d.%s' % (l, k)] = text_bytes(v) if k == 'csv' else v
    assert sorted(ref) == sorted(mine), (sorted(ref), sorted(mine))
    assert ref['dilation_dists'] == DISTS
    no_shared_positions(mesh.vertices, 'the mesh')
    n_dil = 0
    for l in range(len(levels)):
        rv = ref['vertices'][l]
        assert rv.dtype == torch.float32 and same(rv.numpy(), mine['vertices'][l]), ('vertices', l)
        no_shared_positions(rv.numpy(), 'level %d' % l)
        d[p + 'out.v%d' % l] = rv.numpy()
        assert ref['edges'][l].dtype == torch.int64 and ref['traces'][l].dtype == torch.int64
        re_ = LO.sorted_rows(ref['edges'][l].numpy())
        assert same(re_, mine['edges'][l]), ('edges', l)
        assert np.unique(re_, axis=0).shape[0] == re_.shape[0]
        d[p + 'out.e%d' % l] = re_.astype(np.int32)
        assert same(ref['traces'][l].numpy(), mine['traces'][l]), ('traces', l)
        d[p + 'out.t%d' % l] = mine['traces'][l].astype(np.int32)
        rd = ref['dilated_edges'][l]
        d[p + 'out.dl%d' % l] = np.asarray(0 if rd is None else 1)
        assert (rd is None) == (mine['dilated_edges'][l] is None)
        for j, s in enumerate(rd or []):
            mj = mine['dilated_edges'][l][j]
            if not torch.is_tensor(s):
                assert len(s) == 0 and len(mj) == 0
                continue
            assert s.dtype == torch.int64 and same(s.numpy(), mj), ('dilated', l, j)
            d[p + 'out.d%d.%d' % (l, j)] = mj.astype(np.int32)
            n_dil += 1
    if spec['train']:
        assert ref['labels'].dtype == torch.int64 and same(ref['labels'].numpy(), mine['labels'])
        d[p + 'out.labels'] = mine['labels'].astype(np.int32)
        assert ref['vertices'][0].shape[1] == 10
    else:
        assert 'labels' not in ref and ref['vertices'][0].shape[1] == 10
    assert n_dil >= 1, 'no dilated set in the scene'
    differs = 0
    if spec['vc']:                                   # the default normals must give other dilated sets than the reference's rows
        other = LO.graph_levels(m, levels, spec['dilated'], list(DISTS), labels=labels)
        for l in range(len(levels)):
            for a, b in zip(other['dilated_edges'][l] or [], mine['dilated_edges'][l] or []):
                differs += int(not same(a, b))
        assert differs >= 1
    print('scene %d: levels %s, vertices %s, %d dilated sets, %d queries, min gap %.3e%s'
          % (idx, spec['params'], [int(v.shape[0]) for v in ref['vertices']], n_dil, Recorder.queries, Recorder.gap,
             ', %d sets differ with the default normals' % differs if spec['vc'] else ''))
    return d


def main():
    _, glg = ref_import.load_preprocessing()
    for f in glob.glob(os.path.join(OUT, 'g19_levels*.npz')):
        os.remove(f)
    parts = [run_functions(glg)] + [run_scene(glg, i, s) for i, s in enumerate(SCENES)]
    for i, d in enumerate(parts):
        path = os.path.join(OUT, 'g19_levels.npz' if i == 0 else 'g19_levels.part%d.npz' % (i + 1))
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) <= MAX_FILE_BYTES, (path, os.path.getsize(path))
        print(os.path.basename(path), len(d), 'arrays', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    if not ref_import.available():
        sys.exit('the reference tree is needed to regenerate the g19 fixture')
    main()
