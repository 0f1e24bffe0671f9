"""[EXTENSION] X9 goal / path distance field: the plain reference of include/gridvision_hip.h's definition.  The step table
restated, the field as a heap Dijkstra that settles one cell after the other (no tiles, no scans, no rounds), the sampler
as loops over trajectories and poses.  getIndex and the grid geometry are traj_ref's."""
import heapq

import numpy as np

import traj_ref

BLOCKED = 0xFFFFFFFF
UNREACHABLE = 0xFFFFFFFE
SCORE_DTYPE = np.dtype([("sum", np.uint64), ("last", np.uint32), ("best", np.uint32), ("best_pose", np.int32),
                        ("n_bad", np.int32)])
get_index = traj_ref.get_index
grid = traj_ref.grid


def step_table(obstacle_cost, cost_weight):
    """step[v]: 0 for a blocked cell (v >= obstacle_cost), else 1 + cost_weight * v"""
    return np.array([0 if v >= obstacle_cost else 1 + cost_weight * v for v in range(256)], np.uint32)


def config_ok(obstacle_cost, cost_weight, G, flags=0):
    """what gv_set_nav_config accepts on a grid of G cells"""
    return (1 <= obstacle_cost <= 255 and 0 <= cost_weight <= 255 and flags == 0
            and (1 + cost_weight * (obstacle_cost - 1)) * (G - 1) <= 0xFFFFFFFD)


def seed_cells(g, seeds_xy):
    """the OccupancyGrid.data-order entries the seeds name, off-map and non-finite ones dropped, duplicates kept"""
    G = g.nx * g.ny
    out = []
    for x, y in np.asarray(seeds_xy, np.float32).reshape(-1, 2):
        c = get_index(g, np.float64(x), np.float64(y))
        if c is not None:
            out.append(G - 1 - (c[1] * g.nx + c[0]))
    return out


def field(cost, nx, ny, step, seeds):
    """cost: uint8 (G,) in OccupancyGrid.data order; seeds: data-order entries (seed_cells).  Returns (field uint32 (G,),
    n_seeds_used): seeds on blocked cells are skipped."""
    cost = np.asarray(cost, np.uint8).reshape(-1)
    assert cost.size == nx * ny
    st = [int(v) for v in np.asarray(step)[cost]]
    dist = [BLOCKED if s == 0 else UNREACHABLE for s in st]
    heap, used = [], 0
    for c in seeds:
        if st[c] != 0:
            used += 1
            if dist[c] != 0:
                dist[c] = 0
                heap.append((0, c))
    heapq.heapify(heap)
    while heap:
        d, c = heapq.heappop(heap)
        if d != dist[c]:
            continue
        y, x = divmod(c, nx)
        for ok, n in ((x > 0, c - 1), (x + 1 < nx, c + 1), (y > 0, c - nx), (y + 1 < ny, c + nx)):
            if ok and st[n] != 0 and d + st[n] < dist[n]:
                dist[n] = d + st[n]
                heapq.heappush(heap, (dist[n], n))
    return np.array(dist, np.uint32), used


def score(g, fld, poses):
    """fld: uint32 (G,) in data order; poses float32 (K, P, 3).  Returns SCORE_DTYPE (K,)."""
    poses = np.asarray(poses, np.float32)
    K, P = poses.shape[:2]
    G = g.nx * g.ny
    out = np.zeros(K, SCORE_DTYPE)
    for k in range(K):
        total, last, best, best_pose, n_bad = 0, BLOCKED, UNREACHABLE, -1, 0
        for p in range(P):
            c = get_index(g, np.float64(poses[k, p, 0]), np.float64(poses[k, p, 1]))
            v = BLOCKED if c is None else int(fld[G - 1 - (c[1] * g.nx + c[0])])
            if v >= UNREACHABLE:
                n_bad += 1
            else:
                total += v
                if v < best:
                    best, best_pose = v, p
            if p == P - 1:
                last = v
        out[k] = (total, last, best, best_pose, n_bad)
    return out
