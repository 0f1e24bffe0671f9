"""[EXTENSION] X17 path extraction from the distance field: the plain reference of include/gridvision_hip_path.h's
definition.  A Python loop over the eight candidates with the rules one after the other, the centre expression in numpy
float64 rounded once to float32.  It takes ANY uint32 field, so the GPU tests feed it the field read back from the
device.  getIndex and the grid geometry are traj_ref's."""
import numpy as np

import traj_ref

BLOCKED = 0xFFFFFFFF
UNREACHABLE = 0xFFFFFFFE
DIAGONAL = 1 << 0
REACHED, TRUNCATED, OFF_MAP, BLOCKED_START, UNREACHABLE_START, STUCK = range(6)
INFO_DTYPE = np.dtype([("status", np.int32), ("n_cells", np.int32), ("start_value", np.uint32), ("end_value", np.uint32),
                       ("start_entry", np.int32), ("end_entry", np.int32), ("n_diagonal", np.int32), ("reserved", np.uint32)])
MAX_STARTS, MAX_CAP, MAX_CELLS = 256, 65536, 1 << 20
STRAIGHT = ((-1, 0), (1, 0), (0, -1), (0, 1))
DIAGONALS = ((-1, -1), (1, -1), (-1, 1), (1, 1))
get_index = traj_ref.get_index
grid = traj_ref.grid


def start_entry(g, x, y):
    """the data-order entry of a start through getIndex on ((double)x, (double)y); -1 off the map or non-finite"""
    c = get_index(g, np.float64(np.float32(x)), np.float64(np.float32(y)))
    return -1 if c is None else g.nx * g.ny - 1 - (c[1] * g.nx + c[0])


def centre(g, x, y):
    """(X, Y) float32 of the cell behind entry coordinates (x, y): fp64, rounded once"""
    ix, iy = np.float64(g.nx - 1 - x), np.float64(g.ny - 1 - y)
    X = (np.float64(g.pos_x) + np.float64(g.off_x)) - (ix + np.float64(0.5)) * np.float64(g.res)
    Y = (np.float64(g.pos_y) + np.float64(g.off_y)) - (iy + np.float64(0.5)) * np.float64(g.res)
    return np.float32(X), np.float32(Y)


def walk(field, nx, ny, e0, cap, diagonal):
    """one descent from entry e0 (-1: off the map) over field (a list of G ints): (record tuple, [entries])"""
    if e0 < 0:
        return (OFF_MAP, 0, BLOCKED, BLOCKED, -1, -1, 0, 0), []
    v = field[e0]
    if v == BLOCKED:
        return (BLOCKED_START, 0, v, v, e0, -1, 0, 0), []
    if v == UNREACHABLE:
        return (UNREACHABLE_START, 0, v, v, e0, -1, 0, 0), []
    v0 = v
    y, x = divmod(e0, nx)
    cells, n_diag = [e0], 0
    status = REACHED
    while v != 0:
        if len(cells) == cap:
            status = TRUNCATED
            break
        best, nxt = v, None
        for dx, dy in STRAIGHT:
            cx, cy = x + dx, y + dy
            if 0 <= cx < nx and 0 <= cy < ny and field[cy * nx + cx] < best:
                best, nxt = field[cy * nx + cx], (cx, cy, 0)
        if diagonal:
            for dx, dy in DIAGONALS:
                cx, cy = x + dx, y + dy
                if not (0 <= cx < nx and 0 <= cy < ny):
                    continue
                if field[y * nx + cx] == BLOCKED or field[cy * nx + x] == BLOCKED:
                    continue
                if field[cy * nx + cx] < best:
                    best, nxt = field[cy * nx + cx], (cx, cy, 1)
        if nxt is None:
            status = STUCK
            break
        x, y, v = nxt[0], nxt[1], best
        n_diag += nxt[2]
        cells.append(y * nx + x)
    return (status, len(cells), v0, v, e0, cells[-1], n_diag, 0), cells


def paths(g, field, starts, cap, flags=0):
    """field uint32 (G,) in data order, starts (S, 2) float32.  Returns (info INFO_DTYPE (S,), [entries int32 (n_s,)],
    [xy float32 (n_s, 2)])"""
    starts = np.asarray(starts, np.float32).reshape(-1, 2)
    assert 1 <= len(starts) <= MAX_STARTS and 1 <= cap <= MAX_CAP and len(starts) * cap <= MAX_CELLS and flags in (0, DIAGONAL)
    fl = np.asarray(field, np.uint32).reshape(-1).tolist()
    assert len(fl) == g.nx * g.ny
    info = np.zeros(len(starts), INFO_DTYPE)
    ents, xys = [], []
    for s, (sx, sy) in enumerate(starts):
        rec, cells = walk(fl, g.nx, g.ny, start_entry(g, sx, sy), cap, bool(flags & DIAGONAL))
        info[s] = rec
        ents.append(np.array(cells, np.int32))
        xys.append(np.array([centre(g, e % g.nx, e // g.nx) for e in cells], np.float32).reshape(-1, 2))
    return info, ents, xys
