"""[EXTENSION] X19 frontier clusters: the plain Python reference of include/gridvision_hip_frontier.h.  It reads nothing of
the library: explicit class tests, a breadth-first flood over frontier cells only, plain Python integers for the records.
Everything is in OccupancyGrid.data order, entry e = y * nx + x."""
from collections import deque

import numpy as np

import path_ref

NONE = 0xFFFFFFFF
USE_FIELD = 1 << 0
UNREACHABLE = 0xFFFFFFFE
MAX_CAP = 4096
RECORD_DTYPE = np.dtype([("label", np.int32), ("n_cells", np.int32), ("min_x", np.int32), ("max_x", np.int32),
                         ("min_y", np.int32), ("max_y", np.int32), ("sum_x", np.uint64), ("sum_y", np.uint64),
                         ("centre_entry", np.int32), ("field_entry", np.int32), ("field_min", np.uint32),
                         ("goal_entry", np.int32), ("goal_x", np.float32), ("goal_y", np.float32)])
INFO_DTYPE = np.dtype([(n, np.int32) for n in ("n_frontier_cells", "n_components", "n_clusters", "n_written", "best", "largest")] +
                      [("flags", np.uint32), ("reserved", np.uint32)])
assert RECORD_DTYPE.itemsize == 64 and INFO_DTYPE.itemsize == 32
grid = path_ref.grid
NEIGHBOURS8 = tuple((dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0))


def config(free_max=25, unknown_min=40, unknown_max=60, max_cost=256, min_cells=1):
    return dict(free_max=free_max, unknown_min=unknown_min, unknown_max=unknown_max, max_cost=max_cost, min_cells=min_cells)


def frontier_mask(occ, cfg, cost=None):
    """bool (ny, nx): the frontier cells of the int8 layer occ (ny, nx)"""
    v = occ.astype(np.int32)
    free = (v >= 0) & (v <= cfg["free_max"])
    unknown = (v >= cfg["unknown_min"]) & (v <= cfg["unknown_max"])
    beside = np.zeros_like(unknown)
    beside[:, 1:] |= unknown[:, :-1]
    beside[:, :-1] |= unknown[:, 1:]
    beside[1:, :] |= unknown[:-1, :]
    beside[:-1, :] |= unknown[1:, :]
    f = free & beside
    if cfg["max_cost"] < 256:
        f &= cost.reshape(occ.shape).astype(np.int32) < cfg["max_cost"]
    return f


def frontier(g, occ, cfg, cap, flags=0, cost=None, field=None):
    """occ int8 (G,) or (ny, nx), cost uint8, field uint32.  Returns (info INFO_DTYPE record, records RECORD_DTYPE (cap,)
    with zeros behind the written ones, labels uint32 (G,))"""
    nx, ny = g.nx, g.ny
    assert 1 <= cap <= MAX_CAP and flags in (0, USE_FIELD)
    occ = np.asarray(occ, np.int8).reshape(ny, nx)
    f = frontier_mask(occ, cfg, cost)
    fl = None if field is None else np.asarray(field, np.uint32).reshape(-1).tolist()
    labels = np.full(nx * ny, NONE, np.uint32)
    seen = np.zeros(nx * ny, bool)
    is_f = f.reshape(-1)
    comps = []
    for e0 in np.flatnonzero(is_f).tolist():      # ascending: a component's first cell is its smallest entry
        if seen[e0]:
            continue
        seen[e0] = True
        cells, q = [], deque([e0])
        while q:
            e = q.popleft()
            cells.append(e)
            y, x = divmod(e, nx)
            for dx, dy in NEIGHBOURS8:
                qx, qy = x + dx, y + dy
                if 0 <= qx < nx and 0 <= qy < ny:
                    n = qy * nx + qx
                    if is_f[n] and not seen[n]:
                        seen[n] = True
                        q.append(n)
        labels[cells] = e0
        comps.append((e0, cells))
    info = np.zeros(1, INFO_DTYPE)[0]
    info["n_frontier_cells"] = int(is_f.sum())
    info["n_components"] = len(comps)
    info["largest"] = max([len(c) for _, c in comps], default=0)
    info["flags"] = flags
    clusters = [(l, c) for l, c in comps if len(c) >= cfg["min_cells"]]
    info["n_clusters"] = len(clusters)
    written = clusters[:cap]
    info["n_written"] = len(written)
    recs = np.zeros(cap, RECORD_DTYPE)
    for i, (label, cells) in enumerate(written):
        xs, ys = [e % nx for e in cells], [e // nx for e in cells]
        n = len(cells)
        sx, sy = sum(xs), sum(ys)
        cx, cy = sx // n, sy // n
        centre = min(((x - cx) ** 2 + (y - cy) ** 2, e) for x, y, e in zip(xs, ys, cells))[1]
        fmin, fent = UNREACHABLE, -1
        if flags & USE_FIELD:
            reach = [(fl[e], e) for e in cells if fl[e] < UNREACHABLE]
            if reach:
                fmin, fent = min(reach)
        goal = fent if fent >= 0 else centre
        gxy = path_ref.centre(g, goal % nx, goal // nx)
        recs[i] = (label, n, min(xs), max(xs), min(ys), max(ys), sx, sy, centre, fent, fmin, goal, gxy[0], gxy[1])
    if flags & USE_FIELD:
        keys = [(int(r["field_min"]), i) for i, r in enumerate(recs[:len(written)]) if r["field_entry"] >= 0]
    else:
        keys = [(-int(r["n_cells"]), i) for i, r in enumerate(recs[:len(written)])]
    info["best"] = min(keys)[1] if keys else -1
    return info, recs, labels
