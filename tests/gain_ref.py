"""[EXTENSION] X20 information gain: the plain Python reference of include/gridvision_hip_gain.h, written from the header
alone.  It reads nothing of the library: its own enumeration of the ring, side by side; the line iterator's stepping loop
(num += minor ...), not the closed form; Python sets for the seen cells; plain Python integers for the records.
Everything is in OccupancyGrid.data order, entry e = y * nx + x."""
import numpy as np

import path_ref

USE_FIELD, DEVICE_ENTRIES = 1 << 0, 1 << 1
INVALID, UNREACHABLE_BIT, BELOW_MIN = 1 << 0, 1 << 1, 1 << 2
NAV_UNREACHABLE, NAV_BLOCKED = 0xFFFFFFFE, 0xFFFFFFFF
NO_OPAQUE = 0xFFFFFFFF
MAX_N, MAX_RADIUS = 4096, 255
RECORD_DTYPE = np.dtype([("entry", np.int32), ("status", np.uint32), ("n_unknown", np.int32), ("n_free", np.int32),
                         ("n_opaque", np.int32), ("rays_opaque", np.int32), ("rays_off_map", np.int32), ("rays_range", np.int32),
                         ("nearest_opaque_d2", np.uint32), ("dist", np.uint32), ("score", np.int64)])
INFO_DTYPE = np.dtype([("n_candidates", np.int32), ("n_ranked", np.int32), ("best", np.int32), ("best_entry", np.int32),
                       ("best_score", np.int64), ("flags", np.uint32), ("radius", np.int32)])
assert RECORD_DTYPE.itemsize == 48 and INFO_DTYPE.itemsize == 32
grid = path_ref.grid


def config(free_max=25, unknown_min=40, unknown_max=60, radius=8, min_gain=0, w_gain=1, w_dist=0):
    return dict(free_max=free_max, unknown_min=unknown_min, unknown_max=unknown_max, radius=radius, min_gain=min_gain,
                w_gain=w_gain, w_dist=w_dist)


def ring(R):
    """the 8R offsets, ray 0 first: along the top side, down the right one, back along the bottom, up the left"""
    out = []
    for j in range(2 * R):
        out.append((-R + j, -R))
    for j in range(2 * R):
        out.append((R, -R + j))
    for j in range(2 * R):
        out.append((R - j, R))
    for j in range(2 * R):
        out.append((-R, R - j))
    return out


def klass(cfg, v):
    if 0 <= v <= cfg["free_max"]:
        return "F"
    if cfg["unknown_min"] <= v <= cfg["unknown_max"]:
        return "U"
    return "O"


def cast(nx, ny, occ, cfg, cx, cy):
    """the rays of candidate (cx, cy) over occ, a flat list of G ints.  Returns (seen set of (x, y), [rays_opaque,
    rays_off_map, rays_range], nearest_opaque_d2)"""
    R = cfg["radius"]
    seen = set()
    rays = [0, 0, 0]
    nearest = NO_OPAQUE
    for ox, oy in ring(R):
        ddx, ddy = abs(ox), abs(oy)
        sx, sy = (1 if ox >= 0 else -1), (1 if oy >= 0 else -1)
        x_major = ddx >= ddy
        major, minor = (ddx, ddy) if x_major else (ddy, ddx)
        num = major // 2
        x, y = cx, cy
        how = 2                                  # passes cell R without stopping: range
        for _ in range(R):
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
            if not (0 <= x < nx and 0 <= y < ny):
                how = 1
                break
            d2 = (x - cx) ** 2 + (y - cy) ** 2
            if d2 > R * R:
                how = 2
                break
            seen.add((x, y))
            if klass(cfg, occ[y * nx + x]) == "O":
                how = 0
                nearest = min(nearest, d2)
                break
        rays[how] += 1
    return seen, rays, nearest


def gain(g, occ, cfg, entries, flags=0, field=None):
    """occ int8 (G,) or (ny, nx), field uint32 (G,), entries any integers.  Returns (info INFO_DTYPE record, records
    RECORD_DTYPE (n,))"""
    nx, ny = g.nx, g.ny
    G = nx * ny
    entries = [int(e) for e in np.asarray(entries).reshape(-1)]
    assert 1 <= len(entries) <= MAX_N and flags in (0, USE_FIELD)
    occ = np.asarray(occ, np.int8).reshape(-1).tolist()
    recs = np.zeros(len(entries), RECORD_DTYPE)
    ranked = []
    for i, e in enumerate(entries):
        if not 0 <= e < G:
            recs[i] = (e, INVALID, 0, 0, 0, 0, 0, 0, 0, 0, 0)
            continue
        cx, cy = e % nx, e // nx
        seen, rays, nearest = cast(nx, ny, occ, cfg, cx, cy)
        assert (cx, cy) not in seen and sum(rays) == 8 * cfg["radius"]
        n = {"U": 0, "F": 0, "O": 0}
        for x, y in seen:
            n[klass(cfg, occ[y * nx + x])] += 1
        dist = int(field[e]) if flags & USE_FIELD else 0
        lost = bool(flags & USE_FIELD) and dist >= NAV_UNREACHABLE
        status = (UNREACHABLE_BIT if lost else 0) | (BELOW_MIN if n["U"] < cfg["min_gain"] else 0)
        score = 0 if lost else cfg["w_gain"] * n["U"] - cfg["w_dist"] * dist
        recs[i] = (e, status, n["U"], n["F"], n["O"], rays[0], rays[1], rays[2], nearest, dist, score)
        if status == 0:
            ranked.append((-score, i))
    info = np.zeros(1, INFO_DTYPE)[0]
    info["n_candidates"] = len(entries)
    info["n_ranked"] = len(ranked)
    best = min(ranked)[1] if ranked else -1
    info["best"] = best
    info["best_entry"] = entries[best] if best >= 0 else -1
    info["best_score"] = int(recs[best]["score"]) if best >= 0 else 0
    info["flags"] = flags
    info["radius"] = cfg["radius"]
    return info, recs


def frontier_gain(g, occ, cfg, frontier_info, frontier_recs, flags=0, field=None):
    """the frontier form: the candidates are goal_entry of the written records; zero records behind them"""
    n, cap = int(frontier_info["n_written"]), len(frontier_recs)
    out = np.zeros(cap, RECORD_DTYPE)
    if n == 0:
        info = np.zeros(1, INFO_DTYPE)[0]
        info["best"] = info["best_entry"] = -1
        info["flags"], info["radius"] = flags, cfg["radius"]
        return info, out
    info, recs = gain(g, occ, cfg, frontier_recs["goal_entry"][:n], flags, field)
    out[:n] = recs
    return info, out
