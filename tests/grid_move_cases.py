"""Grids, motions and planted layers for gv_grid_move off the multiple-of-4 path: what tests/test_gpu_grid_move.py moves
on the device and tests/test_grid_move_cases_host.py proves on the CPU to be what it claims.  Nothing here touches a GPU.

Why these grids.  launch_grid_move takes k_grid_move4 for nx % 4 == 0 and k_grid_move1 otherwise; a row block is 4 rows,
a workgroup 64 lanes wide; k_copy_segments moves 16 bytes a lane and the rest by a byte tail.  get_index_fast takes its
exact division only for a quotient within 1e-6 of an integer: under a quarter turn about the base origin that is every
in-map source of a grid where exactly one of nx, ny is odd (BORDER_GRIDS), since (pos_x + off_x + off_y) / res is then
a half-integer and the source of a cell centre lies on a cell border on both axes."""
import math
from collections import namedtuple

import numpy as np

Grid = namedtuple("Grid", "name args nx ny pos_x pos_y")


def _grid(gx, gy, res, nx, ny):
    return Grid("%dx%d@%g" % (nx, ny, res), (gx, gy, res), nx, ny, float(gx // 3), 0.0)


# gv_create arguments and the (nx, ny) they must give (asserted against host::grid_params and against the handle)
GRIDS = [
    _grid(1, 1, 1.0, 1, 1), _grid(3, 1, 1.0, 3, 1), _grid(4, 1, 1.0, 4, 1),   # G < 16: tail only, one lane
    _grid(5, 2, 0.2, 25, 10),        # nx odd, ny even, ny % 4 != 0, G % 16 != 0
    _grid(25, 10, 0.2, 125, 50),     # the same parity, two blocks in x
    _grid(5, 2, 0.04, 125, 50),      # ... at another res and pos_x
    _grid(50, 20, 0.3, 167, 67),     # both odd: k_grid_move1, G odd, all three segments have tails
    _grid(25, 10, 0.1, 250, 100),    # nx % 4 == 2
    _grid(50, 20, 0.1, 500, 200),    # k_grid_move4
    _grid(150, 7, 0.5, 300, 14),     # k_grid_move4 with ny % 4 == 2, nx / 4 = 75: a second, partial block in x; 8 tail bytes
]
GRID = {g.name: g for g in GRIDS}
BORDER_GRIDS = ("25x10@0.2", "125x50@0.2", "125x50@0.04")


def geom(g):
    return g.nx, g.ny, g.args[2], g.pos_x, g.pos_y


def corner_radius(g):
    ox, oy = 0.5 * (g.nx * g.args[2]), 0.5 * (g.ny * g.args[2])
    return max(math.hypot(x, y) for x in (g.pos_x - ox, g.pos_x + ox) for y in (g.pos_y - oy, g.pos_y + oy))


# ---------------------------------------------------------------------------------------------------- motions --
Q = math.sin(math.pi / 4), math.cos(math.pi / 4)   # a quarter turn as the quaternion (0, 0, +-Q[0], Q[1])
Motion = namedtuple("Motion", "name tf cells quarter")   # cells: (kx, ky) of a pure whole-cell translation, else None


def _yaw_tf(yaw, tx=0.0, ty=0.0):
    return (0.0, 0.0, math.sin(0.5 * yaw), math.cos(0.5 * yaw), tx, ty, 0.0)


def motions(g):
    res, nx, ny = g.args[2], g.nx, g.ny
    out, seen = [], set()
    for name, (kx, ky) in (("t+x", (2, 0)), ("t-x", (-3, 0)), ("t+y", (0, 1)), ("t-y", (0, -2)), ("t+x-y", (3, -2)),
                           ("t_keep_one", (nx - 1, ny - 1)), ("t_keep_one_neg", (-(nx - 1), -(ny - 1))),
                           ("t_keep_none_x", (nx, 0)), ("t_keep_none_y", (0, -ny)), ("t_keep_none", (-nx, ny))):
        if (kx, ky) != (0, 0) and (kx, ky) not in seen:   # (1 x 1: nx - 1 cells is no move at all)
            seen.add((kx, ky))
            out.append(Motion(name, (0.0, 0.0, 0.0, 1.0, kx * res, ky * res, 0.7), (kx, ky), False))
    for sign, tag in ((1.0, "+q"), (-1.0, "-q")):
        for kx, ky in ((0, 0), (3, -2), (7, 5)):
            out.append(Motion("%s_%d_%d" % (tag, kx, ky), (0.0, 0.0, sign * Q[0], Q[1], kx * res, ky * res, 0.0), None, True))
    th = 0.5 * res / corner_radius(g)   # the planner applies a yaw from here on
    out += [Motion("half_turn", (0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0), None, False),
            Motion("half_turn_t", (0.0, 0.0, 1.0, 0.0, 2 * res, -res, 0.0), None, False),
            Motion("yaw_1.01th", _yaw_tf(1.01 * th), None, False),
            Motion("yaw_3th", _yaw_tf(3.0 * th), None, False),
            Motion("yaw_-1.5th", _yaw_tf(-1.5 * th, 1.3 * res, 0.4 * res), None, False),
            Motion("far_away", (0.0, 0.0, 0.0, 1.0, 1e15, -1e15, 0.0), None, False)]
    if 0.3 > th:   # (the one-cell grid turns from 0.71 rad on)
        out += [Motion("yaw_0.3", _yaw_tf(0.3), None, False),
                Motion("yaw_0.3_t", _yaw_tf(0.3, 2.4 * res, -1.3 * res), None, False)]
    return out


SCENES = [(g.name, m.name) for g in GRIDS for m in motions(g)]


def scene(key):
    g = GRID[key[0]]
    return g, next(m for m in motions(g) if m.name == key[1])


def is_border(key):
    return key[0] in BORDER_GRIDS and scene(key)[1].quarter


# --------------------------------------------------------------------------------------------- planted layers --
RAMP = 29   # levels of the ramp: int8 12, 15, ..., 96


def ramp_log_odds(nx, ny):
    """log-odds whose next update_map (decay -0.2, clamp to [-2, 3.6], sigmoid, 100 * p truncated) gives cell (ix, iy)
    the int8 12 + 3 * ((ix + 3 * iy) % 29): no cell shares a level with any of its eight neighbours (their levels are
    1 .. 4 steps away), and every level's p sits half a unit of int8 away from a truncation step"""
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny))
    p = (12.5 + 3.0 * ((ix + 3 * iy) % RAMP)) / 100.0
    return (np.log(p / (1.0 - p)) + 0.2).astype(np.float32).reshape(-1)


def origin_cell(g):
    """the cell that holds the base origin, which every rotation here turns about"""
    res = g.args[2]
    return int((0.5 * (g.ny * res) + g.pos_y) / res) * g.nx + int((0.5 * (g.nx * res) + g.pos_x) / res)


def special_log_odds(G, c0=0):
    """G float32 words, no two with the same bits: NaNs of different payloads (quiet and signalling, both signs), both
    infinities, -0.0, both clamps and subnormals, the rest small ordinary values of both signs.  The one-of-a-kind
    values sit in every second cell behind cell c0."""
    k = np.arange(G, dtype=np.uint32)
    w = np.uint32(0x3D000000) + 2 * k + ((k & np.uint32(1)) << np.uint32(31))
    nan = k % 7 == 3
    w = np.where(nan & (k % 2 == 0), np.uint32(0x7FC00000) | k, w)              # quiet, payload k
    w = np.where(nan & (k % 2 == 1), np.uint32(0xFF800000) | (k + 1), w)        # signalling, negative, payload k + 1
    fixed = np.array([0x7F800000, 0xFF800000, 0x80000000, 0xC0000000, 0x40666666, 0x00000001, 0x807FFFFF, 0x00400000,
                      0x7FFFFFFF, 0xFFC00000, 0x7F800001], np.uint32)   # +-inf, -0.0, -2.0f, 3.6f, subnormals, NaNs
    slots = (c0 + 1 + 2 * np.arange(len(fixed))) % G   # (a tiny grid takes as many as fit)
    slots, first = np.unique(slots, return_index=True)
    w = w.copy()
    w[slots] = fixed[first]
    return w.view(np.float32)


def check_planted(state, nx, ny):
    """what makes any wrong source index visible: every log-odds word distinct, every cell's int8 and occupancy different
    from its eight neighbours'"""
    lo, occ, i8 = state
    G = nx * ny
    assert len(np.unique(lo.view(np.uint32))) == G
    if G >= 64:
        bits = lo.view(np.uint32)
        assert np.isnan(lo).sum() >= 2 and len(np.unique(bits[np.isnan(lo)])) == np.isnan(lo).sum()
        assert np.isposinf(lo).any() and np.isneginf(lo).any() and (bits == 0x80000000).any()
        assert (lo == np.float32(-2.0)).any() and (lo == np.float32(3.6)).any()
        assert ((bits & 0x7F800000) == 0).sum() >= 4   # -0.0 and three subnormals
    for layer in (occ.view(np.uint32).reshape(ny, nx), i8[::-1].reshape(ny, nx)):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dx, dy) != (0, 0) and abs(dx) < nx and abs(dy) < ny:
                    a = layer[max(dy, 0):ny + min(dy, 0), max(dx, 0):nx + min(dx, 0)]
                    b = layer[max(-dy, 0):ny + min(-dy, 0), max(-dx, 0):nx + min(-dx, 0)]
                    assert (a != b).all(), (dx, dy)


def plant(h, g):
    """through the public calls of a handle (or anything with the same four): the ramp, one map update so that occupancy
    and int8 follow it, then the special log-odds on top, infinities and clamps next to the base origin where turn after
    turn leaves them on the map; returns the readback, checked"""
    h.set_log_odds(ramp_log_odds(h.nx, h.ny))
    h.update_map()
    h.set_log_odds(special_log_odds(h.nx * h.ny, origin_cell(g)))
    state = h.log_odds(), h.occupancy(), h.to_occupancy_grid()[0]
    check_planted(state, h.nx, h.ny)
    return state
