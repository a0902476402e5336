"""CPU oracle of the circle masks (test helper): the heap BFS of the reference's process_frame_circles
(preprocessing/observed_texture_map_generation.py:570-584) restated over an edge list, and its batch-size rule (:586-591)."""
import heapq

import numpy as np


def adjacency(edge_index, n):
    """Undirected neighbour sets of an [2, E] edge list (both directions; self loops and duplicates harmless)."""
    adj = [set() for _ in range(n)]
    for a, b in np.asarray(edge_index).T:
        adj[int(a)].add(int(b))
        adj[int(b)].add(int(a))
    return adj


def heap_bfs_mask(adj, radius, centres, mask=None):
    """mask[v] = max over the centres of (radius - heap distance), visited nodes at distance radius get 0 - the reference's loop,
    with one change that leaves every value as it is: a node is not pushed again at a distance it already has in the heap."""
    n = len(adj)
    mask = np.zeros(n, dtype=np.int64) if mask is None else mask
    for index in centres:
        seen = set()
        pushed = {int(index): 0}
        visited = []
        heapq.heappush(visited, (0, int(index)))
        while len(visited) > 0:
            next_dist, next_idx = heapq.heappop(visited)
            seen.add(next_idx)
            mask[next_idx] = max(radius - next_dist, mask[next_idx])
            if next_dist <= radius - 1:
                for neighbor_idx in adj[next_idx]:
                    if neighbor_idx not in seen and pushed.get(neighbor_idx, radius + 2) > next_dist + 1:
                        pushed[neighbor_idx] = next_dist + 1
                        heapq.heappush(visited, (next_dist + 1, neighbor_idx))
    return mask


def next_batch_size(total, masked, n, frac):
    """(finished, next sample_num_points) after a batch, as the reference computes them (fp64, int() truncation)."""
    cur = np.int64(masked) / n
    k = int(total * (frac / cur - 1))
    return bool(np.int64(masked) / n >= frac or k <= 0), k


def rule_sizes(counts, n, frac):
    """The batch sizes the rule gives for a sequence of masked counts after each batch (first batch 10)."""
    sizes, total, k = [], 0, 10
    for c in counts:
        sizes.append(k)
        total += k
        done, k = next_batch_size(total, c, n, frac)
        if done:
            break
    return sizes
