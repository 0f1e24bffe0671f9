"""[EXTENSION] X7 trajectory scoring: the plain reference of include/gridvision_hip.h's definition.  numpy fp64 sin / cos,
getIndex restated operation by operation, grid_map's LineIterator as the Python loop it is (no closed form, no lanes),
the pose cost as a maximum over a list of cells.  Everything the library computes in parallel is computed here one cell
after the other."""
import math
from collections import namedtuple

import numpy as np

KEEP_POSE_COST = 1 << 0
DEVICE_POSES = 1 << 1
SCORE_DTYPE = np.dtype([("max_cost", np.int32), ("first_collision", np.int32), ("cost_sum", np.uint32),
                        ("n_off_map", np.int32)])

# vertices: tuple of (x, y) in metres in the robot frame, () for the circular robot
Fp = namedtuple("Fp", "vertices collision_cost off_map_cost", defaults=(253, 255))
Grid = namedtuple("Grid", "nx ny res len_x len_y pos_x pos_y off_x off_y")


def grid(grid_x, grid_y, res):
    """the geometry gv_create(grid_x, grid_y, res) gives (src/occupancy_grid.cpp:10-11)"""
    nx, ny = int(math.floor(grid_x / res + 0.5)), int(math.floor(grid_y / res + 0.5))
    len_x, len_y = nx * res, ny * res
    return Grid(nx, ny, res, len_x, len_y, float(grid_x // 3), 0.0, 0.5 * len_x, 0.5 * len_y)


def get_index(g, x, y):
    """grid_map::getIndexFromPosition as the project restates it: (ix, iy) or None"""
    x, y = float(x), float(y)
    tx = -((x - g.pos_x) - g.off_x)
    ty = -((y - g.pos_y) - g.off_y)
    if not (tx >= 0.0 and ty >= 0.0 and tx < g.len_x and ty < g.len_y):
        return None
    vx = ((x - g.off_x) - g.pos_x) / g.res
    vy = ((y - g.off_y) - g.pos_y) / g.res
    jx, jy = int(-vx), int(-vy)
    if jx < 0 or jy < 0 or jx >= g.nx or jy >= g.ny:
        return None
    return jx, jy


def line(sx, sy, ex, ey):
    """grid_map::LineIterator((sx, sy), (ex, ey)), both ends included"""
    ddx, ddy = abs(ex - sx), abs(ey - sy)
    stepx, stepy = (1 if ex >= sx else -1), (1 if ey >= sy else -1)
    inc1x, inc1y, inc2x, inc2y = stepx, stepy, stepx, stepy
    if ddx >= ddy:
        inc1x = inc2y = 0
        den, num, add, ncells = ddx, ddx // 2, ddy, ddx + 1
    else:
        inc2x = inc1y = 0
        den, num, add, ncells = ddy, ddy // 2, ddx, ddy + 1
    out = []
    cx, cy = sx, sy
    for _ in range(ncells):
        out.append((cx, cy))
        num += add
        if num >= den:
            num -= den
            cx += inc1x
            cy += inc1y
        cx += inc2x
        cy += inc2y
    return out


def world_vertices(fp, x, y, yaw):
    """fp64, one operation at a time: wx = x + (c vx - s vy), wy = y + (s vx + c vy)"""
    x, y, yaw = np.float64(np.float32(x)), np.float64(np.float32(y)), np.float64(np.float32(yaw))
    with np.errstate(invalid="ignore"):
        c, s = np.cos(yaw), np.sin(yaw)
        out = []
        for vx, vy in fp.vertices:
            vx, vy = np.float64(vx), np.float64(vy)
            out.append((float(x + (c * vx - s * vy)), float(y + (s * vx + c * vy))))
    return out


def pose_vertex_cells(g, fp, x, y, yaw):
    """[centre cell, vertex cells ...] as (ix, iy), or None for an off-map pose"""
    cells = [get_index(g, np.float64(np.float32(x)), np.float64(np.float32(y)))]
    if fp.vertices:
        cells += [get_index(g, wx, wy) for wx, wy in world_vertices(fp, x, y, yaw)]
    return None if any(c is None for c in cells) else cells


def pose_edges(g, fp, x, y, yaw):
    """[(sx, sy, ex, ey)] of an on-map pose, [] for the circular robot; None off the map"""
    vc = pose_vertex_cells(g, fp, x, y, yaw)
    if vc is None:
        return None
    v = vc[1:]
    return [(*v[i], *v[(i + 1) % len(v)]) for i in range(len(v))]


def pose_cells(g, fp, x, y, yaw):
    """the cells of a pose as iy * nx + ix: the centre, then the outline edge by edge; None off the map"""
    vc = pose_vertex_cells(g, fp, x, y, yaw)
    if vc is None:
        return None
    out = [vc[0][1] * g.nx + vc[0][0]]
    for sx, sy, ex, ey in pose_edges(g, fp, x, y, yaw):
        out += [cy * g.nx + cx for cx, cy in line(sx, sy, ex, ey)]
    return out


def all_cells(g, fp, poses):
    """pose_cells of every pose of poses (K, P, 3): K lists of P entries (a numpy array of cells, or None off the map);
    they do not depend on the costmap, so tests that score one family against several costmaps compute them once"""
    poses = np.asarray(poses, np.float32)
    out = []
    for k in range(poses.shape[0]):
        row = []
        for p in range(poses.shape[1]):
            c = pose_cells(g, fp, *poses[k, p])
            row.append(None if c is None else np.array(c, np.int64))
        out.append(row)
    return out


def score(g, fp, cost, poses, cells=None):
    """cost: uint8 (G,) in OccupancyGrid.data order; poses float32 (K, P, 3); cells: all_cells(g, fp, poses) where the
    caller has them already.  Returns (scores SCORE_DTYPE (K,), pose_cost uint8 (K, P))."""
    poses = np.asarray(poses, np.float32)
    K, P = poses.shape[:2]
    cost = np.asarray(cost, np.uint8).reshape(-1)
    G = g.nx * g.ny
    assert cost.size == G
    if cells is None:
        cells = all_cells(g, fp, poses)
    scores = np.zeros(K, SCORE_DTYPE)
    pose_cost = np.zeros((K, P), np.uint8)
    for k in range(K):
        mx, first, total, n_off = 0, -1, 0, 0
        for p in range(P):
            c = cells[k][p]
            if c is None:
                pc = centre = fp.off_map_cost
                n_off += 1
            else:
                centre = int(cost[G - 1 - c[0]])
                pc = int(cost[G - 1 - c].max())
            pose_cost[k, p] = pc
            total += centre
            mx = max(mx, pc)
            if first < 0 and pc >= fp.collision_cost:
                first = p
        scores[k] = (mx, first, total, n_off)
    return scores, pose_cost
