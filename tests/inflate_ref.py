"""[EXTENSION] X6 inflated costmap: the plain reference the tests hold gv_inflate to (include/gridvision_hip.h has the
definition; oracle/ has no such step).

  cost_table(cfg, res)    the definition line by line with math.sqrt / math.exp
  dist2(lethal, d2max)    the minimum over EVERY offset (dx, dy) with dx^2 + dy^2 <= d2max of a shifted copy of the
                          zero-padded lethal mask: no rows-then-columns decomposition, no tiles, nothing in common with
                          the kernels
  costmap(i8, cfg, res)   the two combined, on the packed int8 layer in OccupancyGrid.data order

Arrays are (ny, nx) in data order: element [y, x] is byte y * nx + x of what gv_to_occupancy_grid returns."""
import collections
import math

import numpy as np

KEEP_DIST2 = 1 << 0
OCCUPANCY_SCALE = 1 << 1
NONE = 65535

# radii in metres, scaling in 1/m, lethal iff int8 >= thr
Cfg = collections.namedtuple("Cfg", "inscribed inflation scaling thr flags", defaults=(65, 0))


def d2max_of(cfg, res):
    """the largest q with sqrt(q) * res <= inflation radius"""
    q = 0
    while math.sqrt(float(q + 1)) * res <= cfg.inflation:
        q += 1
    return q


def cost_table(cfg, res):
    n = d2max_of(cfg, res) + 1
    out = np.zeros(n, np.uint8)
    for q in range(n):
        dist = math.sqrt(float(q)) * res
        if q == 0:
            c = 254
        elif dist <= cfg.inscribed:
            c = 253
        elif dist > cfg.inflation:
            c = 0
        else:
            c = int(252.0 * math.exp(-cfg.scaling * (dist - cfg.inscribed)))   # truncation, as (uint8_t)
        if cfg.flags & OCCUPANCY_SCALE:
            c = 0 if c == 0 else 99 if c == 253 else 100 if c == 254 else 1 + (97 * (c - 1)) // 251
        out[q] = c
    return out


def dist2(lethal, d2max):
    """uint16 (ny, nx): the smallest dx^2 + dy^2 <= d2max to a lethal cell of the map, NONE without one"""
    lethal = np.asarray(lethal, dtype=bool)
    ny, nx = lethal.shape
    r = math.isqrt(d2max)
    pad = np.zeros((ny + 2 * r, nx + 2 * r), dtype=bool)
    pad[r:r + ny, r:r + nx] = lethal
    offs = sorted(((dx * dx + dy * dy, dx, dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1)
                   if dx * dx + dy * dy <= d2max), reverse=True)
    out = np.full((ny, nx), NONE, np.uint16)
    for q, dx, dy in offs:   # farthest first: a nearer one overwrites
        out[pad[r + dy:r + dy + ny, r + dx:r + dx + nx]] = q
    return out


def costmap(i8, nx, ny, cfg, res):
    """(cost uint8 (ny, nx), dist2 uint16 (ny, nx)) of the packed layer i8 (G int8 in data order)"""
    lethal = np.asarray(i8, dtype=np.int8).reshape(ny, nx) >= cfg.thr
    table = cost_table(cfg, res)
    d2 = dist2(lethal, len(table) - 1)
    has = d2 != NONE
    cost = np.where(has, table[np.where(has, d2, 0)], 0).astype(np.uint8)
    return cost, d2
