"""[EXTENSION] X9 goal / path distance field: the maps and seed lists that test_nav_host.py checks for what they claim and
test_gpu_nav.py solves on the device.

A case is a lethal mask in OccupancyGrid.data order (row y, column x of entry y * nx + x: the order of the costmap and of
the field), the inflation it is planted with, and two seed lists in world coordinates: one goal, and a 300-point path
with points off the map, on blocked cells, non-finite ones and duplicates.  With the EXACT inflation only a planted cell
has a cost, so only planted cells block; the INFLATION sets of test_gpu_traj.py give the cost gradient that the weights
act on.  Masks are planted on the device as test_gpu_traj._plant does; cost_of() is the same costmap from inflate_ref,
for the host tests."""
import numpy as np

import inflate_ref
import traj_cases as tc
import traj_ref

EXACT = (0.0, 0.0, 1.0, 65)
INFLATION = {0.1: (0.35, 0.55, 10.0, 65), 0.05: (0.12, 0.3, 8.0, 65)}   # test_gpu_traj.INFLATION
GRIDS = dict(tc.GRIDS)
GRIDS["200x80"] = ((10, 4, 0.05), (200, 80))
CONFIGS = [(253, 0), (253, 3), (254, 0), (254, 3)]   # (obstacle_cost, cost_weight)
PATH_POINTS = 300


def grid_of(name):
    (gx, gy, res), (nx, ny) = GRIDS[name]
    g = traj_ref.grid(gx, gy, res)
    assert (g.nx, g.ny) == (nx, ny)
    return g


def world_of(g, x, y):
    """the centre, in world coordinates, of the cell behind data-order entry (column x, row y)"""
    ix, iy = g.nx - 1 - x, g.ny - 1 - y
    return (g.pos_x + g.off_x) - (ix + 0.5) * g.res, (g.pos_y + g.off_y) - (iy + 0.5) * g.res


def cost_of(g, mask, inflation):
    """uint8 (G,): the costmap gv_inflate gives for lethal = mask (inflate_ref's definition)"""
    i8 = np.where(mask.reshape(-1), 97, 11).astype(np.int8)
    cfg = inflate_ref.Cfg(*inflation)
    return inflate_ref.costmap(i8, g.nx, g.ny, cfg, g.res)[0].reshape(-1)


def serpentine(nx, ny):
    """walls on every odd row, the gap alternating between the two ends: one corridor nx * ny / 2 cells long"""
    m = np.zeros((ny, nx), bool)
    m[1::2, :] = True
    for i, y in enumerate(range(1, ny, 2)):
        m[y, nx - 1 if i % 2 == 0 else 0] = False
    return m


def in_tile(nx, ny):
    """a closed box around cells 66..125 (both axes) of tile (1, 1), inside it a serpentine of period 2 with its gaps
    inside the box: some 1800 steps that never leave one 64 x 64 tile"""
    m = np.zeros((ny, nx), bool)
    m[65, 65:127] = m[126, 65:127] = True
    m[65:127, 65] = m[65:127, 126] = True
    for i, y in enumerate(range(67, 126, 2)):
        m[y, 66:126] = True
        m[y, 125 if i % 2 == 0 else 66] = False
    return m


def staircase(nx, ny):
    """a one-cell-thick diagonal from border to border (through the tile corners at 64 and 128): diagonal neighbours
    only, which 4-connected motion cannot pass"""
    assert nx == ny
    return np.eye(ny, dtype=bool)


def pocket(nx, ny):
    """a closed box, rows 30..60 and columns 40..90"""
    m = np.zeros((ny, nx), bool)
    m[30, 40:91] = m[60, 40:91] = True
    m[30:61, 40] = m[30:61, 90] = True
    return m


def random_mask(nx, ny, density, seed):
    return np.random.default_rng(seed).random((ny, nx)) < density


def largest_component_cell(cost, nx, ny, obstacle_cost=253):
    """(x, y) of the cell of the largest 4-connected component of cells below obstacle_cost that lies nearest the map's
    centre; and that component's share of the map"""
    from scipy import ndimage
    free = cost.reshape(ny, nx) < obstacle_cost
    lab, n = ndimage.label(free)
    assert n >= 1
    sizes = np.bincount(lab.reshape(-1))[1:]
    big = 1 + int(np.argmax(sizes))
    ys, xs = np.nonzero(lab == big)
    i = int(np.argmin((ys - ny // 2) ** 2 + (xs - nx // 2) ** 2))
    return (int(xs[i]), int(ys[i])), sizes[big - 1] / float(nx * ny)


def path_seeds(g, cost, seed, anchor):
    """(300, 2) float32: 270 centres of cells below cost 253 around a walk that starts at `anchor`, 8 centres of cells
    of cost >= 254 (where the map has that many), 8 points off the map, 4 non-finite ones, and duplicates of the first
    points to fill up; then (n_off, n_nonfinite) for the test's arithmetic"""
    rng = np.random.default_rng(seed)
    c2 = cost.reshape(g.ny, g.nx)
    pts = []
    x, y = anchor
    while len(pts) < 270:
        x = int(np.clip(x + rng.integers(-3, 4), 0, g.nx - 1))
        y = int(np.clip(y + rng.integers(-3, 4), 0, g.ny - 1))
        if c2[y, x] < 253:
            pts.append(world_of(g, x, y))
    ys, xs = np.nonzero(c2 >= 254)
    for i in rng.permutation(len(xs))[:8]:
        pts.append(world_of(g, int(xs[i]), int(ys[i])))
    x_hi, y_hi = g.pos_x + g.off_x, g.pos_y + g.off_y
    off = [(x_hi + 0.5, 0.0), (x_hi - g.len_x - 0.5, 0.0), (0.0, y_hi + 0.5), (0.0, y_hi - g.len_y - 0.5),
           (1e6, 1e6), (-1e6, 0.0), (x_hi - g.len_x, 0.0), (0.0, y_hi - g.len_y)]   # the last two: ON the far edges, off
    nonfinite = [(np.nan, 0.0), (0.0, np.nan), (np.inf, 0.0), (0.0, -np.inf)]
    pts += off + nonfinite
    pts += pts[:PATH_POINTS - len(pts)]
    out = np.array(pts, np.float32)
    assert out.shape == (PATH_POINTS, 2)
    return out, len(off), len(nonfinite)


_CACHE = {}


def cases():
    """name -> dict(grid, mask (ny, nx) bool, inflation, goal (1, 2) float32, goal_cell (x, y), path (300, 2) float32,
    n_off, n_nonfinite, cost uint8 (G,) from inflate_ref)"""
    if _CACHE:
        return _CACHE

    def add(name, grid, mask, inflation, goal_cell=None):
        g = grid_of(grid)
        cost = cost_of(g, mask, inflation)
        share = None
        if goal_cell is None:
            goal_cell, share = largest_component_cell(cost, g.nx, g.ny)
        path, n_off, n_nonfinite = path_seeds(g, cost, len(_CACHE) + 1, goal_cell)
        _CACHE[name] = dict(grid=grid, mask=mask, inflation=inflation, goal_cell=goal_cell, share=share,
                            goal=np.array([world_of(g, *goal_cell)], np.float32), path=path, n_off=n_off,
                            n_nonfinite=n_nonfinite, cost=cost)

    add("serpentine_200x80", "200x80", serpentine(200, 80), EXACT, (0, 0))
    add("comb_250x100", "250x100", serpentine(100, 250).T.copy(), EXACT, (0, 0))
    add("in_tile_200x200", "200x200", in_tile(200, 200), EXACT, (66, 66))
    add("staircase", "200x200", staircase(200, 200), EXACT, (150, 20))
    add("pocket_outside", "250x100", pocket(250, 100), EXACT, (10, 10))
    add("pocket_inside", "250x100", pocket(250, 100), EXACT, (65, 45))
    add("random_0.3", "500x200", random_mask(500, 200, 0.3, 17), EXACT)
    add("random_5e-4", "500x200", random_mask(500, 200, 5e-4, 23), INFLATION[0.1])
    add("random_2e-3", "200x200", random_mask(200, 200, 2e-3, 29), INFLATION[0.05])
    return _CACHE
