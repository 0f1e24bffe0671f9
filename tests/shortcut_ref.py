"""[EXTENSION] X21 shortcuts and waypoints: the plain Python reference of include/gridvision_hip_shortcut.h, written from
the header alone.  It reads nothing of the library: the line iterator's stepping loop (num += minor ...), not the closed
form; plain Python lists and integers in the walk, no numpy; the centre expression is path_ref's (numpy float64 rounded
once).  It takes ANY cost array and ANY entry lists.  Everything is in OccupancyGrid.data order, entry e = y * nx + x."""
import numpy as np

import path_ref

NO_CORNER = 1 << 0
OK, TRUNCATED, EMPTY = range(3)
MAX_WINDOW, MAX_SPACING, MAX_WCAP, MAX_CELLS = 4096, 65535, 65536, 1 << 20
INFO_DTYPE = np.dtype([("status", np.int32), ("n_waypoints", np.int32), ("n_anchors", np.int32), ("n_src", np.int32),
                       ("n_steps", np.int32), ("n_diag_steps", np.int32), ("max_cost_seen", np.int32), ("end_entry", np.int32)])
assert INFO_DTYPE.itemsize == 32
grid = path_ref.grid
centre = path_ref.centre


def config(max_cost=252, window=64, spacing=0):
    return dict(max_cost=max_cost, window=window, spacing=spacing)


def line(p, q):
    """the cells of the iterator from p to q, both included: major + 1 of them"""
    (px, py), (qx, qy) = p, q
    ddx, ddy = abs(qx - px), abs(qy - py)
    sx, sy = (1 if qx >= px else -1), (1 if qy >= py else -1)
    x_major = ddx >= ddy
    major, minor = (ddx, ddy) if x_major else (ddy, ddx)
    num = major // 2
    x, y = px, py
    cells = [(x, y)]
    for _ in range(major):
        num += minor
        step_minor = num >= major
        if step_minor:
            num -= major
        if x_major:
            x += sx
            y += sy if step_minor else 0
        else:
            y += sy
            x += sx if step_minor else 0
        cells.append((x, y))
    assert cells[-1] == (qx, qy)
    return cells


def visible(cost, nx, max_cost, no_corner, p, q):
    cells = line(p, q)
    for i, (x, y) in enumerate(cells):
        if cost[y * nx + x] > max_cost:
            return False
        if no_corner and i >= 1:
            xp, yp = cells[i - 1]
            if xp != x and yp != y and (cost[y * nx + xp] > max_cost or cost[yp * nx + x] > max_cost):
                return False
    return True


def anchors(cost, nx, cfg, no_corner, cells):
    """the whole anchor chain of a path given as [(x, y)]"""
    n = len(cells)
    out = [0]
    a = 0
    while a < n - 1:
        nxt = a + 1
        for j in range(min(a + cfg["window"], n - 1), a + 1, -1):
            if visible(cost, nx, cfg["max_cost"], no_corner, cells[a], cells[j]):
                nxt = j
                break
        out.append(nxt)
        a = nxt
    return out


def one(cost, nx, cfg, no_corner, entries, wcap):
    """one path, entries a list of ints: (record tuple, [(entry, index)])"""
    n = len(entries)
    if n == 0:
        return (EMPTY, 0, 0, 0, 0, 0, 0, -1), []
    cells = [(e % nx, e // nx) for e in entries]
    ways = []
    n_steps = n_diag = seen = 0
    a = 0
    while a < n - 1 and len(ways) < wcap:
        b = a + 1
        for j in range(min(a + cfg["window"], n - 1), a + 1, -1):
            if visible(cost, nx, cfg["max_cost"], no_corner, cells[a], cells[j]):
                b = j
                break
        seg = line(cells[a], cells[b])
        m = len(seg) - 1
        n_steps += m
        n_diag += min(abs(cells[b][0] - cells[a][0]), abs(cells[b][1] - cells[a][1]))
        seen = max([seen] + [cost[y * nx + x] for x, y in seg])
        ways.append((entries[a], a))                           # the segment is entered
        if cfg["spacing"] > 0:
            for i in range(cfg["spacing"], m, cfg["spacing"]):
                if len(ways) < wcap:
                    ways.append((seg[i][1] * nx + seg[i][0], -1))
        a = b
    status = TRUNCATED
    if a == n - 1 and len(ways) < wcap:
        ways.append((entries[n - 1], n - 1))
        seen = max(seen, cost[entries[n - 1]])
        status = OK
    n_anchors = sum(1 for _, i in ways if i >= 0)
    return (status, len(ways), n_anchors, n, n_steps, n_diag, seen, ways[-1][0]), ways


def shortcut(g, cost, cfg, src, wcap, flags=0):
    """cost uint8 (G,) or (ny, nx); src a list of S entry lists.  Returns (info INFO_DTYPE (S,), [entries int32 (n_s,)],
    [index int32 (n_s,)], [xy float32 (n_s, 2)])"""
    assert 1 <= wcap <= MAX_WCAP and len(src) * wcap <= MAX_CELLS and flags in (0, NO_CORNER)
    assert 0 <= cfg["max_cost"] <= 254 and 1 <= cfg["window"] <= MAX_WINDOW and 0 <= cfg["spacing"] <= MAX_SPACING
    cl = np.asarray(cost, np.uint8).reshape(-1).tolist()
    assert len(cl) == g.nx * g.ny
    info = np.zeros(len(src), INFO_DTYPE)
    ents, idxs, xys = [], [], []
    for s, path in enumerate(src):
        rec, ways = one(cl, g.nx, cfg, bool(flags & NO_CORNER), [int(e) for e in path], wcap)
        info[s] = rec
        ents.append(np.array([e for e, _ in ways], np.int32))
        idxs.append(np.array([i for _, i in ways], np.int32))
        xys.append(np.array([centre(g, e % g.nx, e // g.nx) for e, _ in ways], np.float32).reshape(-1, 2))
    return info, ents, idxs, xys
