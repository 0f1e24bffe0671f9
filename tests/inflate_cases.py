"""[EXTENSION] X6 inflated costmap: the parameter sets and the lethal-mask fixtures that test_inflate_host.py checks for
what they claim and test_gpu_inflate.py plants on the device.  Masks are bool (ny, nx) in OccupancyGrid.data order."""
import math

import numpy as np

from inflate_ref import Cfg

# (resolution, Cfg): P1 Rc 5 / d2max 30, P2 Rc 30 / d2max 918, P3 Rc 63 (the cap) / d2max 4019, P4 no inscribed ring,
# P5 = P1's ring on 0.2 m cells (the 1000 x 1000 grid of the pipelined-frame and tick cases).  Each keeps every
# sqrt(q) * res >= 1e-9 m away from both radii and every 252 * factor >= 1e-6 away from an integer
# (test_inflate_host.py asserts it), so no libm can move a table entry.
PSETS = {
    "P1": (0.1, Cfg(0.35, 0.55, 10.0)),
    "P2": (0.1, Cfg(0.52, 3.03, 3.0)),
    "P3": (0.05, Cfg(0.31, 3.17, 1.5)),
    "P4": (0.25, Cfg(0.0, 2.1, 2.0)),
    "P5": (0.2, Cfg(0.5, 1.1, 5.0)),
}
D2MAX = {"P1": 30, "P2": 918, "P3": 4019}

# name -> (grid_x, grid_y, resolution) of gv_create and the (nx, ny) it gives
GRIDS = {
    "500x200": ((50, 20, 0.1), (500, 200)),
    "250x100": ((25, 10, 0.1), (250, 100)),     # nx % 4 != 0
    "200x200": ((10, 10, 0.05), (200, 200)),    # P3
    "200x80": ((50, 20, 0.25), (200, 80)),      # P4
    "2000x2000": ((200, 200, 0.1), (2000, 2000)),   # P1 only
}


def ring_offsets(d2max):
    """per kind of separation, (inside, outside): the offset of that kind with the largest dx^2 + dy^2 <= d2max and the
    one with the smallest > d2max.  (30 and 31, 4019 and 4020 are no sums of two squares: no pair of cells is exactly
    d2max or d2max + 1 apart there, these are the nearest distances that exist.)"""
    r = math.isqrt(d2max)
    diag = [(dx * dx + dy * dy, dx, dy) for dx in range(1, r + 2) for dy in range(1, dx + 1)]
    inside = max(o for o in diag if o[0] <= d2max)
    outside = min(o for o in diag if o[0] > d2max)
    return {"h": ((r, 0), (r + 1, 0)), "v": ((0, r), (0, r + 1)), "d": (inside[1:], outside[1:])}


def single_cell(nx, ny):
    m = np.zeros((ny, nx), bool)
    m[ny // 2, nx // 2] = True
    return m


def border_fixture(nx, ny, rc):
    """a lethal cell in each corner and one on each edge: mid-edge at the top, the bottom and the right; the right one,
    (nx-1, ny//2), is the last byte of its row, and the next byte of the layer, (0, ny//2+1), is free and more than rc
    from every lethal cell (the left edge's cell sits rc + 1 rows further down)"""
    m = np.zeros((ny, nx), bool)
    for y in (0, ny - 1):
        for x in (0, nx // 2, nx - 1):
            m[y, x] = True
    m[ny // 2, nx - 1] = True
    m[ny // 2 + 2 + rc, 0] = True
    return m


def seam_fixture(nx, ny, d2max, anchors, spacing):
    """anchors: (x, y, sx, sy) -- a lethal cell and the side its probes lie on (sx, sy = +-1).  Each gets the six probes
    of ring_offsets (inside / outside for a horizontal, a vertical and a diagonal separation).  Returns (mask, probes):
    probes = [(x, y, d2 to its own anchor)], off-map ones left out.  `spacing`: anchors closer than that in both axes
    are refused (a probe's nearest lethal cell must be its own anchor; test_inflate_host.py checks the outcome)."""
    m = np.zeros((ny, nx), bool)
    probes = []
    for i, (x, y, sx, sy) in enumerate(anchors):
        assert 0 <= x < nx and 0 <= y < ny
        for (x2, y2, _, _) in anchors[:i]:
            assert max(abs(x - x2), abs(y - y2)) >= spacing, (x, y, x2, y2)
        m[y, x] = True
        for pair in ring_offsets(d2max).values():
            for dx, dy in pair:
                px, py = x + sx * dx, y + sy * dy
                if 0 <= px < nx and 0 <= py < ny:
                    probes.append((px, py, dx * dx + dy * dy))
    return m, probes


def seam_anchors_p1():
    """2000 x 2000, Rc 5: every multiple of 32 up to 256 as a line in x and as a line in y; per line an anchor on the
    last cell before it with probes across it, and one on the first cell after it with probes back across it"""
    out = []
    for k, line in enumerate(range(32, 257, 32)):
        out.append((line - 1, 300 + 32 * k, +1, +1))     # x line: across to the right
        out.append((line, 316 + 32 * k, -1, -1))         # ... and back to the left
        out.append((600 + 32 * k, line - 1, +1, +1))     # y line: across downwards
        out.append((616 + 32 * k, line, -1, -1))         # ... and back
    return out


def seam_anchors_p3(k):
    """200 x 200, Rc 63, k = 1, 2, 3: the lines 32 k (crossed to the right and downwards from the cell before them in
    both axes) and 32 (k + 3) (crossed to the left and upwards from the cell on them); the two anchors are 97 cells
    apart in both axes, farther from each other's probes than those are from their own anchor"""
    a, b = 32 * k, 32 * (k + 3)
    return [(a - 1, a - 1, +1, +1), (b, b, -1, -1)]


def random_mask(nx, ny, density, seed):
    return np.random.default_rng(seed).random((ny, nx)) < density


def row_and_column(nx, ny):
    m = np.zeros((ny, nx), bool)
    m[ny // 3, :] = True
    m[:, (2 * nx) // 3] = True
    return m


def threshold_fixture(nx, ny, seed=5):
    """int8 (G,) in data order holding every value of -1 .. 100 (the -1 of a NaN occupancy included) many times over"""
    rng = np.random.default_rng(seed)
    v = rng.integers(-1, 101, nx * ny).astype(np.int8)
    v[:102] = np.arange(-1, 101, dtype=np.int8)
    return rng.permutation(v)
