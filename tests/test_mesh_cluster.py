"""Mesh clustering, the part that needs no GPU: the header declares the entry points and the Python view binds them, the public
function refuses CPU tensors, graph_levels knows a cell-size level from the others, and the numpy restatement of the contract
(tests/_meshcluster_oracle.py) has the properties the contract promises."""
import numpy as np
import pytest
import torch

import _levels_oracle as LO
import _meshcluster_oracle as MO

SEED = 7


def test_header_declares_the_entry_points_and_the_python_view_binds_them():
    from surface_texture_inpainting_net_amd import _lib
    for name in ('stin_voxel_cluster_mean_f64', 'stin_face_cluster_workspace_bytes', 'stin_face_cluster_i64'):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['stin_voxel_cluster_mean_f64'][1]) == len(_lib.SIGNATURES['stin_voxel_cluster_f64'][1]) == 9
    assert len(_lib.SIGNATURES['stin_face_cluster_i64'][1]) == 10
    assert max(len(a) for _, a in _lib.SIGNATURES.values()) == 28 and _lib.CONSTANTS['STIN_VERSION'] == 102


def test_entry_point_exists_and_refuses_cpu_tensors():
    from surface_texture_inpainting_net_amd import preprocessing as P
    m = LO.grid_mesh(6, SEED)
    with pytest.raises(TypeError):
        P.cluster_mesh(torch.from_numpy(m['vertices']), torch.from_numpy(m['faces']), 0.6)


def test_a_cell_size_level_is_told_from_the_others():
    from surface_texture_inpainting_net_amd import preprocessing as P
    assert P._cell_size('0.04') == 0.04 and P._cell_size('12.5') == 12.5 and P._cell_size(0.3) == 0.3 and P._cell_size('1e-2') == 0.01
    for other in ('100', '30', '0', '101', 'x', '-3', '', '0.0', 'nan', 'inf', '1_0', ' 0.04', 0.0, -0.5, float('inf'), float('nan'),
                  30, True, None, {}):
        assert P._cell_size(other) is None
    assert P._qem_percent('0.04') is None


def test_the_restatement_keeps_its_promises():
    m = LO.grid_mesh(12, SEED)
    V, F = m['vertices'], m['faces']
    pos, out, trace, nc, info = MO.cluster_mesh(V, F, 0.6, return_info=True)
    assert trace.shape == (V.shape[0],) and trace.dtype == np.int64 and np.array_equal(np.unique(trace), np.arange(nc))   # total, onto
    assert pos.shape == (nc, 3) and pos.dtype == np.float64 and out.dtype == np.int64
    assert info['degenerate'] > 0 and info['merged'] > 0                # the case holds what the rules are about
    assert out.shape[0] == info['faces_in'] - info['degenerate'] - info['merged']
    assert MO.distinct(out).all()                                       # three distinct corners
    assert np.unique(np.sort(out, axis=1), axis=0).shape[0] == out.shape[0]          # no two faces share a vertex set
    assert MO.is_subsequence(out, trace[F])                             # images of input faces, order and orientation kept
    for c in range(nc):                                                 # positions: the members' mean
        assert np.allclose(pos[c], V[trace == c].mean(axis=0), rtol=0, atol=1e-12)
    bins = V // 0.6
    assert all(np.unique(bins[trace == c], axis=0).shape[0] == 1 for c in range(nc))
    assert np.array_equal(np.unique(bins, axis=0), bins[np.array([np.flatnonzero(trace == c)[0] for c in range(nc)])])


def test_of_two_opposite_faces_on_one_triple_the_lower_id_keeps_its_orientation():
    # two vertices per cell along x: cells 0, 1, 2 are the vertex pairs (0, 1), (2, 3), (4, 5)
    V = np.array([[0.1, 0, 0], [0.2, 0, 0], [1.1, 1, 0], [1.2, 1, 0], [2.1, 0, 1], [2.2, 0, 1]], dtype=np.float64)
    V[:, 1:] *= 0.1                                                     # y and z stay inside cell 0
    F = np.array([[4, 0, 2], [1, 5, 3], [0, 1, 2], [5, 1, 2]])           # images (2, 0, 1), (0, 2, 1): opposite; one degenerate; (2, 0, 1)
    pos, out, trace, nc, info = MO.cluster_mesh(V, F, 1.0, return_info=True)
    assert nc == 3 and np.array_equal(trace, [0, 0, 1, 1, 2, 2])
    assert np.array_equal(out, [[2, 0, 1]])
    assert info == dict(faces_in=4, degenerate=1, merged=2, merged_opposite=1)
    _, out, _, _ = MO.cluster_mesh(V, F[[1, 0, 2, 3]], 1.0)
    assert np.array_equal(out, [[0, 2, 1]])


@pytest.mark.parametrize('side,cell', [(13, 0.6), (24, 0.3), (12, 100.0)])
def test_the_torch_route_for_the_faces_follows_the_restatement(side, cell):
    """The route cluster_mesh takes for its faces beyond 2^21 clusters is plain torch: it runs on CPU tensors as well."""
    from surface_texture_inpainting_net_amd import preprocessing as P
    m = LO.grid_mesh(side, SEED)
    _, out, trace, _, info = MO.cluster_mesh(m['vertices'], m['faces'], cell, return_info=True)
    assert info['merged'] > 0 and info['degenerate'] > 0
    got = P._cluster_faces_torch(torch.from_numpy(m['faces']), torch.from_numpy(trace))
    assert np.array_equal(got.numpy(), out)
    assert P._cluster_faces_torch(torch.from_numpy(m['faces'][:1]), torch.zeros_like(torch.from_numpy(trace))).shape == (0, 3)


def test_the_restatement_refuses_what_the_contract_refuses():
    m = LO.grid_mesh(6, SEED)
    G = m['faces'].copy()
    G[3, 2] = m['vertices'].shape[0]
    with pytest.raises(IndexError):
        MO.cluster_mesh(m['vertices'], G, 0.6)
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError):
            MO.cluster_mesh(m['vertices'], m['faces'], bad)
