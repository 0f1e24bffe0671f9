"""[EXTENSION] X17 path extraction: the start lists that test_path_host.py walks with the host twin and
test_gpu_path.py on the device, over the maps of nav_cases.cases() and over empty maps.

On a nav case the starts are the farthest reachable cell of the goal's field and random reachable ones.  On the empty
250 x 100 map (ragged 64-tiles, and narrower than four 64-cell windows) a field is |dx| + |dy| from its goal, so every
path is known in closed form: with the four straight candidates it runs along x first (x-1 and x+1 are tried first), with
GV_PATH_DIAGONAL it takes min(|dx|, |dy|) diagonal steps first.  EMPTY_GOALS puts the goal at the centre, in the four
corners and in the middle of the four borders, which gives straight runs of 99 to 249 cells in all eight directions
(three 64-cell windows and more) and paths that run along a border for their whole length."""
import numpy as np

import nav_cases as nc
import nav_ref
import path_ref

CONFIGS = [(253, 0), (253, 3)]
NAV_CAP = 16384            # room for the comb's 12625 cells
NAV_RANDOM_STARTS = 7
EMPTY_GRID = "250x100"
FLUSH_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129)   # cells: around the 64-cell flush of the kernel
_FIELDS = {}


def nav_field(name, cfg):
    """nav_ref's field of a nav case from its goal (cached): what the host tests walk"""
    key = (name, cfg)
    if key not in _FIELDS:
        c = nc.cases()[name]
        g = nc.grid_of(c["grid"])
        _FIELDS[key] = nav_ref.field(c["cost"], g.nx, g.ny, nav_ref.step_table(*cfg), nav_ref.seed_cells(g, c["goal"]))[0]
    return _FIELDS[key]


def nav_starts(g, field, seed):
    """(1 + NAV_RANDOM_STARTS, 2) float32: the centre of the farthest reachable cell (the lowest entry among equals),
    then of random reachable cells"""
    reach = np.flatnonzero(field < path_ref.UNREACHABLE)
    assert len(reach) > NAV_RANDOM_STARTS
    far = int(reach[np.argmax(field[reach])])
    pick = np.random.default_rng(seed).choice(reach, NAV_RANDOM_STARTS, replace=False)
    return np.array([nc.world_of(g, int(e) % g.nx, int(e) // g.nx) for e in [far, *pick]], np.float32)


def empty_field(g, goal):
    """the field of the empty map from one goal cell with weight 0: |dx| + |dy|"""
    ys, xs = np.mgrid[0:g.ny, 0:g.nx]
    return (np.abs(xs - goal[0]) + np.abs(ys - goal[1])).astype(np.uint32).reshape(-1)


def empty_goals(g):
    nx, ny = g.nx, g.ny
    return {"centre": (nx // 2, ny // 2), "nw": (0, 0), "ne": (nx - 1, 0), "sw": (0, ny - 1), "se": (nx - 1, ny - 1),
            "w": (0, ny // 2), "e": (nx - 1, ny // 2), "n": (nx // 2, 0), "s": (nx // 2, ny - 1)}


def empty_start_cells(g, name):
    """the start cells (entry coordinates) walked towards goal `name` of the empty map"""
    nx, ny = g.nx, g.ny
    gx, gy = empty_goals(g)[name]
    # the four corners, a cell on every border, and one cell inside each: windows clipped on one and on two sides
    cells = [(0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1), (1, 1), (nx - 2, 1), (1, ny - 2), (nx - 2, ny - 2),
             (0, 37), (nx - 1, 61), (77, 0), (190, ny - 1), (1, 37), (nx - 2, 61), (77, 1), (190, ny - 2)]
    if name == "centre":
        for n in FLUSH_LENGTHS:   # n cells: n - 1 steps, some of them along y
            dx = min(n - 1, 100)
            cells.append((gx - dx, gy + (n - 1 - dx)))
            cells.append((gx + dx, gy - (n - 1 - dx)))
    else:
        # the straight run of its direction; a corner goal gets the two borders that meet there (paths that stay on a
        # border for their whole length) and the pure diagonal (with GV_PATH_DIAGONAL: ny - 1 diagonal steps)
        far_x, far_y = nx - 1 - gx if gx in (0, nx - 1) else gx, ny - 1 - gy if gy in (0, ny - 1) else gy
        cells += [(far_x, gy), (gx, far_y)]
        if gx in (0, nx - 1) and gy in (0, ny - 1):
            cells.append((gx + (ny - 1) * (1 if gx == 0 else -1), far_y))
    return cells


def empty_starts(g, name):
    return np.array([nc.world_of(g, x, y) for x, y in empty_start_cells(g, name)], np.float32)
