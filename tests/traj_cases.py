"""[EXTENSION] X7 trajectory scoring: the grids, footprints and pose families that test_traj_host.py checks for what they
claim and test_gpu_traj.py scores on the device, and the guard that keeps them independent of the libm.

The device's fp64 sin / cos need not equal numpy's in the last bit.  A last-bit difference moves a vertex by some 1e-15 m;
it can change a cell only where the vertex sits that close to a cell border or to the map's edge.  guard_violations()
therefore demands, for every pose with yaw != 0, that every vertex's pre-truncation quotient lies at least 1e-9 from an
integer and every bounds term at least 1e-9 from 0 and from the map length.  A drawn trajectory that violates it is
drawn again with the next seed (REDRAWN counts them), never tolerated.  Poses with yaw == 0.0f are exempt: c = 1 and
s = 0 are exact on any libm, c * vx - s * vy is vx exactly, and these poses carry the cases ON the borders.  Poses with a
NaN or infinite yaw are exempt as well: sin and cos of them are NaN on any libm, and every vertex is off the map."""
import math

import numpy as np

import traj_ref as ref

GUARD = 1e-9
REDRAWN = {}   # family name -> trajectories drawn again because a pose violated the guard

# name -> (grid_x, grid_y, resolution) of gv_create and the (nx, ny) it gives
GRIDS = {
    "500x200": ((50, 20, 0.1), (500, 200)),
    "250x100": ((25, 10, 0.1), (250, 100)),     # nx % 4 != 0
    "200x200": ((10, 10, 0.05), (200, 200)),
}


def grid_of(name):
    (gx, gy, res), (nx, ny) = GRIDS[name]
    g = ref.grid(gx, gy, res)
    assert (g.nx, g.ny) == (nx, ny)
    return g


def _poly16():
    r = [1.2, 1.0, 1.3, 0.9, 1.25, 1.05, 1.15, 0.95, 1.3, 1.0, 1.2, 0.9, 1.1, 1.3, 0.95, 1.2]
    return tuple((r[i] * math.cos(2 * math.pi * i / 16), r[i] * math.sin(2 * math.pi * i / 16)) for i in range(16))


# vertices in metres, robot frame (x forward)
FOOTPRINTS = {
    "point": (),
    "triangle": ((0.6, 0.0), (-0.3, 0.35), (-0.3, -0.35)),
    "rect": ((3.4, 1.0), (-1.1, 1.0), (-1.1, -1.0), (3.4, -1.0)),          # 4.5 m x 2.0 m, origin off-centre
    "poly16": _poly16(),
    "tiny": ((0.02, 0.0), (-0.01, 0.015), (-0.01, -0.015)),                # smaller than a cell
    "long": ((14.0, 0.4), (-1.0, 0.4), (-1.0, -0.4), (14.0, -0.4)),       # 150-cell edges at 0.1 m
    "diamond": ((0.5, 0.0), (0.0, 0.5), (-0.5, 0.0), (0.0, -0.5)),         # at yaw 0: ddx == ddy on every edge
    # yaw-0 border cases: vertex 0 is the pose's own position, the others point into the map from that side
    "in_from_+x": ((0.0, 0.0), (-0.5, 0.2), (-0.5, -0.2)),
    "in_from_-x": ((0.0, 0.0), (0.5, -0.2), (0.5, 0.2)),
    "in_from_+y": ((0.0, 0.0), (-0.2, -0.5), (0.2, -0.5)),
    "in_from_-y": ((0.0, 0.0), (0.2, 0.5), (-0.2, 0.5)),
    # 40.0f + (40.7 - 40.0) is the double 40.7 exactly: getIndex((40.7, 0)) = (2, 100) on the 500 x 200 map, where
    # decimal arithmetic says 3
    "canary": ((40.7 - 40.0, 0.0), (-0.5, 0.3), (-0.5, -0.3)),
}


def fp_of(name, collision_cost=253, off_map_cost=255):
    return ref.Fp(FOOTPRINTS[name], collision_cost, off_map_cost)


def guard_violations(g, fp, poses):
    """poses (..., 3) float32: the (pose, vertex) pairs that sit within GUARD of a cell border or of the map's edge;
    yaw == 0 and non-finite yaws are exempt (module docstring)"""
    bad = []
    for i, (x, y, yaw) in enumerate(np.asarray(poses, np.float32).reshape(-1, 3)):
        if yaw == 0.0 or not np.isfinite(yaw) or not fp.vertices:
            continue
        for v, (wx, wy) in enumerate(ref.world_vertices(fp, x, y, yaw)):
            if not (math.isfinite(wx) and math.isfinite(wy)):
                continue   # a non-finite centre: off the map whatever sin and cos give
            for w, pos, off, length in ((wx, g.pos_x, g.off_x, g.len_x), (wy, g.pos_y, g.off_y, g.len_y)):
                t = -((w - pos) - off)
                q = -(((w - off) - pos) / g.res)
                if abs(t) < GUARD or abs(t - length) < GUARD or abs(q - round(q)) < GUARD:
                    bad.append((i, v))
    return bad


def arcs(family, g, fp, K, P, seed, box, step, yaw_range=(-math.pi, math.pi), max_curv=0.4):
    """K arcs of P poses: start uniform in box = (x0, x1, y0, y1), constant step and curvature, yaw never 0.  A
    trajectory with a pose that violates the guard is drawn again with the next seed."""
    out = np.zeros((K, P, 3), np.float32)
    s = seed
    for k in range(K):
        while True:
            rng = np.random.default_rng(s)
            s += 1
            x, y = rng.uniform(box[0], box[1]), rng.uniform(box[2], box[3])
            yaw, curv = rng.uniform(*yaw_range), rng.uniform(-max_curv, max_curv)
            t = np.zeros((P, 3), np.float32)
            for p in range(P):
                t[p] = (x, y, yaw)
                x, y, yaw = x + step * math.cos(yaw), y + step * math.sin(yaw), yaw + step * curv
            if (t[:, 2] != 0).all() and not guard_violations(g, fp, t):
                break
            REDRAWN[family] = REDRAWN.get(family, 0) + 1
        out[k] = t
    REDRAWN.setdefault(family, 0)
    return out


def _ulp(v, up):
    return np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf))


def border_poses(g):
    """yaw-0 poses on the 500 x 200 map: footprint name -> (1, P, 3).  Centres and vertices exactly on cell borders in
    both axes, the canary, and per side of the map the outer edge itself, one float32 ulp inside and one outside it."""
    x_hi, x_lo = g.pos_x + g.off_x, g.pos_x - g.off_x      # 41, -9: x_hi is on the map (tx == 0), x_lo is not (tx == len)
    y_hi, y_lo = g.pos_y + g.off_y, g.pos_y - g.off_y      # 10, -10
    on_borders = [(16.0, 0.0), (16.5, 0.5), (20.0, -3.0), (1.0, 7.0), (30.5, -9.5)]   # multiples of 0.5: exact in fp32
    fam = {
        "in_from_+x": [(x_hi, 0.25), (_ulp(x_hi, False), 0.25), (_ulp(x_hi, True), 0.25)] + on_borders,
        "in_from_-x": [(x_lo, 0.25), (_ulp(x_lo, True), 0.25), (_ulp(x_lo, False), 0.25)] + on_borders,
        "in_from_+y": [(3.25, y_hi), (3.25, _ulp(y_hi, False)), (3.25, _ulp(y_hi, True))] + on_borders,
        "in_from_-y": [(3.25, y_lo), (3.25, _ulp(y_lo, True)), (3.25, _ulp(y_lo, False))] + on_borders,
        "canary": [(40.0, 0.0), (16.0, 0.0)],
        "point": [(x_hi, 0.25), (_ulp(x_hi, True), 0.25), (x_lo, 0.25), (_ulp(x_lo, True), 0.25), (3.25, y_hi),
                  (3.25, _ulp(y_hi, True)), (3.25, y_lo), (3.25, _ulp(y_lo, True)), (40.7, 0.0)] + on_borders,
        "diamond": [(16.05, 0.05), (30.25, -4.35)],        # cell centres: every edge has ddx == ddy == 5
    }
    return {k: np.array([[(x, y, 0.0) for x, y in v]], np.float32) for k, v in fam.items()}


def leaving_poses(g):
    """(3, 64, 3): straight runs along +x with yaw 0.05 that leave the map at pose 0, at pose 31 and at pose 63 (the
    poses before that one are on the map with the triangle footprint, it and those after it are not)"""
    out = np.zeros((3, 64, 3), np.float32)
    x_hi = g.pos_x + g.off_x
    for k, at in enumerate((0, 31, 63)):
        for p in range(64):
            out[k, p] = (x_hi - 0.5 + 0.25 * (p - at), 1.23 + 0.01 * p, 0.05)   # the front vertex is 0.6 m ahead
    return out


def nonfinite_poses():
    """(8, 3, 3) on the 250 x 100 map: pose 1 of trajectory k has a NaN / infinite x, y or yaw; trajectory 0 has none"""
    base = np.array([(5.03, 1.02, 0.3), (5.23, 1.07, 0.32), (5.43, 1.13, 0.34)], np.float32)
    out = np.repeat(base[None], 8, axis=0)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    for k, (col, v) in enumerate([(0, nan), (0, inf), (0, -inf), (1, nan), (1, -inf), (2, nan), (2, inf)], start=1):
        out[k, 1, col] = v
    return out


_CACHE = {}


def families():
    """name -> dict(grid, fp (a FOOTPRINTS name), poses float32 (K, P, 3)).  Between them K takes 1, 3, 64, 65, 257 and
    P takes 1, 2, 63, 64, 65, 130."""
    if _CACHE:
        return _CACHE
    g5, g2, gs = grid_of("500x200"), grid_of("250x100"), grid_of("200x200")
    mid5 = (0.0, 32.0, -4.0, 4.0)

    def add(name, grid, fp, poses):
        _CACHE[name] = dict(grid=grid, fp=fp, poses=np.ascontiguousarray(poses, np.float32))

    add("rect_3x130", "500x200", "rect", arcs("rect_3x130", g5, fp_of("rect"), 3, 130, 100, mid5, 0.04))
    add("triangle_64x63", "500x200", "triangle", arcs("triangle_64x63", g5, fp_of("triangle"), 64, 63, 200, mid5, 0.1))
    add("point_257x2", "500x200", "point", arcs("point_257x2", g5, fp_of("point"), 257, 2, 300, (-9.5, 41.5, -10.5, 10.5), 0.3))
    add("poly16_65x1", "250x100", "poly16", arcs("poly16_65x1", g2, fp_of("poly16"), 65, 1, 400, (-3.0, 19.0, -3.5, 3.5), 0.1))
    add("tiny_1x64", "250x100", "tiny", arcs("tiny_1x64", g2, fp_of("tiny"), 1, 64, 500, (0.0, 15.0, -3.0, 3.0), 0.037))
    add("rect_3x65_fine", "200x200", "rect", arcs("rect_3x65_fine", gs, fp_of("rect"), 3, 65, 600, (1.5, 4.5, -1.0, 1.0), 0.02))
    add("long_3x2", "500x200", "long", arcs("long_3x2", g5, fp_of("long"), 3, 2, 700, (-7.0, 20.0, -2.0, 2.0), 0.2,
                                          yaw_range=(-0.4, 0.4)))
    add("long_steep_1x2", "500x200", "long", arcs("long_steep_1x2", g5, fp_of("long"), 1, 2, 750, (15.0, 17.0, -8.0, -7.0), 0.2,
                                                  yaw_range=(1.2, 1.5)))
    for fp, poses in border_poses(g5).items():
        add("border_" + fp, "500x200", fp, poses)
    add("leaving_3x64", "500x200", "triangle", leaving_poses(g5))
    add("nonfinite_8x3", "250x100", "triangle", nonfinite_poses())
    add("nonfinite_point_8x3", "250x100", "point", nonfinite_poses())
    return _CACHE
