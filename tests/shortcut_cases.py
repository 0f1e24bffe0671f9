"""[EXTENSION] X21 shortcuts and waypoints: the fixtures of test_shortcut_host.py and test_gpu_shortcut.py.  A case is a
lethal mask in data order (ny, nx) with the inflation that turns it into a costmap, a configuration, the call's flags and
wcap, and S paths twice over: as entry lists for the host tests (`paths`; an empty list is an EMPTY source), and as the
goal cell, the start cells (None: a start off the map) and the path flags from which gv_nav_path makes the resident
paths on the device.  `same`: the device's paths are these very lists (an L on an open map: the descent's tie rule takes
x first), which the GPU test asserts, so that the edge a fixture is named for is met on the device too.  A case with
`gpu` False has paths no descent gives (cells far apart, lines in both directions) and is for the twin alone.  Every
case comes with a check that it is what its name claims (check(name, ...) below, run against shortcut_ref).  Small maps
only: 130 x 70, 250 x 100 (nx % 4 != 0 on both), one 640 x 640."""
import functools

import numpy as np

import nav_cases as nc
import shortcut_ref as ref

GRIDS = {"130x70": ((13, 7, 0.1), (130, 70)), "250x100": ((25, 10, 0.1), (250, 100)), "640x640": ((64, 64, 0.1), (640, 640))}
EXACT = nc.EXACT                  # cost 254 on the mask, 0 elsewhere
GRADED = nc.INFLATION[0.1]        # inscribed 0.35 m, inflation 0.55 m: 253 within 3 cells, decaying to 0 at 5.5
NAV_CONFIG = (253, 0)             # every cell below 253 can be walked, at the same price
PATH_DIAGONAL = 1


@functools.lru_cache(maxsize=None)
def grid_of(name):
    (gx, gy, res), (nx, ny) = GRIDS[name]
    g = ref.grid(gx, gy, res)
    assert (g.nx, g.ny) == (nx, ny)
    return g


def ent(grid, x, y):
    return y * GRIDS[grid][1][0] + x


def l_path(grid, start, goal):
    """the 4-connected L from start to goal, x first: what the descent of an open map gives"""
    (x, y), (gx, gy) = start, goal
    cells = [(x, y)]
    while x != gx:
        x += 1 if gx > x else -1
        cells.append((x, y))
    while y != gy:
        y += 1 if gy > y else -1
        cells.append((x, y))
    return [ent(grid, cx, cy) for cx, cy in cells]


def mask_of(grid, lethal=()):
    nx, ny = GRIDS[grid][1]
    m = np.zeros((ny, nx), bool)
    for x, y in lethal:
        m[y, x] = True
    return m


_COSTS = {}


def cost_of(grid, mask, inflation):
    key = (grid, mask.tobytes(), inflation)
    if key not in _COSTS:
        _COSTS[key] = nc.cost_of(grid_of(grid), mask, inflation) if inflation != EXACT else np.where(mask.reshape(-1), 254, 0).astype(np.uint8)
    return _COSTS[key]


def _case(grid, mask, goal, starts, wcap=256, flags=0, inflation=EXACT, path_flags=0, paths=None, same=True, gpu=True, cap=1024, **cfg):
    if paths is None:
        paths = [l_path(grid, s, goal) if s is not None else [] for s in starts]
    assert len(paths) == len(starts) and all(len(p) <= cap for p in paths)
    return dict(grid=grid, mask=mask, inflation=inflation, cost=cost_of(grid, mask, inflation), cfg=ref.config(**cfg), flags=flags, wcap=wcap,
                goal=goal, starts=list(starts), path_flags=path_flags, paths=paths, same=same, gpu=gpu, cap=cap)


def _sprinkle(grid, seed, density, keep_free=()):
    nx, ny = GRIDS[grid][1]
    m = np.random.default_rng(seed).random((ny, nx)) < density
    for x, y in keep_free:
        m[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = False
    return m


def _full(c, wcap=ref.MAX_WCAP):
    return ref.shortcut(grid_of(c["grid"]), c["cost"], c["cfg"], c["paths"], wcap, c["flags"])


OCTANT_ENDS = [(40, 0), (40, 9), (40, 31), (40, 40), (31, 40), (9, 40), (0, 40), (-9, 40), (-31, 40), (-40, 40), (-40, 31), (-40, 9), (-40, 0),
               (-40, -9), (-40, -31), (-40, -40), (-31, -40), (-9, -40), (0, -40), (9, -40), (31, -40), (40, -40), (40, -31), (40, -9)]


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    g130, g250, g640 = "130x70", "250x100", "640x640"
    e130, e250 = mask_of(g130), mask_of(g250)
    # W = 1: no candidate is ever tested; with spacing 1 the waypoints are the path itself
    c["w1_spacing1"] = _case(g130, e130, (40, 30), [(5, 5)], window=1, spacing=1)
    # either side of a batch of 64 candidates (a window of W has W - 1 of them: 65 | 66 and 129 | 130 are the kernel's own edges)
    trap = mask_of(g250, [(190, 20), (200, 40), (180, 8), (120, 5)] + [(x, 30) for x in range(150, 203)])   # inside the L's triangle, off the L
    for W in (63, 64, 65, 66, 127, 128, 129, 130):
        c["w%d" % W] = _case(g250, trap, (203, 60), [(3, 3)], window=W, spacing=0)
    # path lengths 0 (EMPTY, next to good ones), 1, 2, 64, 65, and an end nearer than W
    c["lengths"] = _case(g250, e250, (125, 50), [(120, 50), None, (125, 50), (125, 49), (62, 50), (61, 50), (125, 60), None], window=64, spacing=3)
    # the pillar: from (20, 20) the cells 13 and 14 of the path are hidden, 15 is not
    c["pillar"] = _case(g130, mask_of(g130, [(26, 22)]), (30, 25), [(20, 20)], window=64)
    wall = mask_of(g250)
    wall[:, 120] = True
    wall[50, 120] = False
    gap_path = l_path(g250, (30, 20), (119, 50)) + [ent(g250, 120, 50)] + l_path(g250, (121, 50), (220, 80))
    c["wall_gap"] = _case(g250, wall, (220, 80), [(30, 20)], window=256, spacing=4, paths=[gap_path], same=False)
    pair = mask_of(g130, [(42, 31), (41, 32)])
    c["diagonal_pair"] = _case(g130, pair, (43, 33), [(40, 30)], window=64)
    c["diagonal_pair_no_corner"] = _case(g130, pair, (43, 33), [(40, 30)], window=64, flags=ref.NO_CORNER)
    # cost == max_cost and cost == max_cost + 1: the largest cost on the line from the first to the last cell of the path
    one = mask_of(g130, [(70, 34)])
    graded = cost_of(g130, one, GRADED)
    L = l_path(g130, (40, 40), (80, 26))
    top = max(int(graded[y * 130 + x]) for x, y in ref.line((40, 40), (80, 26)))
    assert 0 < top < 252 and all(int(graded[e]) == 0 for e in L)
    c["cost_at_max"] = _case(g130, one, (80, 26), [(40, 40)], inflation=GRADED, max_cost=top, window=64)
    c["cost_above_max"] = _case(g130, one, (80, 26), [(40, 40)], inflation=GRADED, max_cost=top - 1, window=64)
    # a path whose own cells all exceed max_cost: four cells from a wall, in its inflation band
    band = mask_of(g130)
    band[30, 10:121] = True
    c["path_above_max"] = _case(g130, band, (100, 34), [(30, 34)], inflation=GRADED, max_cost=100, window=64, spacing=2)
    # lines in all eight octants, shallow and steep, and both ways along the same cells: three-cell paths p, p, q
    lethal = _sprinkle(g130, 5, 0.01)
    p = (65, 35)
    far = [(p[0] + dx * 3 // 4, p[1] + dy * 3 // 4) for dx, dy in OCTANT_ENDS]
    both = [[ent(g130, *p), ent(g130, *p), ent(g130, *q)] for q in far] + [[ent(g130, *q), ent(g130, *q), ent(g130, *p)] for q in far]
    c["octants_both_ways"] = _case(g130, lethal, p, [p] * len(both), wcap=32, window=4, spacing=3, paths=both, same=False, gpu=False)
    c["octants_both_ways_no_corner"] = dict(c["octants_both_ways"], flags=ref.NO_CORNER)
    # ... and on the device: 8-connected descents to one goal from all round it, over scattered lethal cells
    goal = (125, 50)
    ring = [(goal[0] + dx, goal[1] + dy) for dx, dy in OCTANT_ENDS]
    scattered = _sprinkle(g250, 6, 0.004, keep_free=[goal] + ring)
    for name, fl in (("octants", 0), ("octants_no_corner", ref.NO_CORNER)):
        c[name] = _case(g250, scattered, goal, ring, wcap=64, flags=fl, window=64, spacing=3, path_flags=PATH_DIAGONAL, same=False)
    # segments with 63 / 64 / 65 and 129 waypoints between their anchors: spacing 1 over straight runs of 64, 65, 66 and 130
    c["between_63_64_65_129"] = _case(g250, e250, (200, 50), [(200 - m, 50) for m in (64, 65, 66, 130)], window=130, spacing=1)
    # spacing 1, 2, = major and > major on the L of major 10
    for sp in (1, 2, 10, 11):
        c["spacing_%d" % sp] = _case(g130, e130, (30, 25), [(20, 20)], window=64, spacing=sp)
    # wcap: an exact fit, the last slot on an anchor, the last slot inside a segment
    base = _case(g130, e130, (60, 40), [(10, 10)], window=9, spacing=2)
    idx = _full(base)[2][0].tolist()
    n_all = len(idx)
    on_anchor = max(k for k in range(2, n_all) if idx[k - 1] >= 0)
    mid = max(k for k in range(2, n_all) if idx[k - 1] < 0)
    for name, k in (("wcap_exact", n_all), ("wcap_on_anchor", on_anchor), ("wcap_mid_segment", mid), ("wcap_1", 1)):
        c[name] = dict(base, wcap=k)
    # 256 short paths
    rng = np.random.default_rng(7)
    spots = [(int(rng.integers(0, 250)), int(rng.integers(0, 100))) for _ in range(256)]
    many = _sprinkle(g250, 8, 0.003, keep_free=[goal] + spots)
    c["s256"] = _case(g250, many, goal, spots, wcap=48, window=16, spacing=3, same=False)
    # a whole path along the map's edge: row 0, then column 0
    c["map_edge"] = _case(g250, e250, (0, 99), [(249, 0)], window=64, spacing=5)
    c["map_edge_far_corner"] = _case(g250, e250, (249, 0), [(0, 99)], window=4096, spacing=5)
    # 640 x 640: long 8-connected descents over a random map, a wide window
    centre = (320, 320)
    corners = [(5, 5), (634, 5), (5, 634), (634, 634), (320, 10), (10, 300)]
    big = _sprinkle(g640, 9, 0.002, keep_free=[centre] + corners)
    c["random_640"] = _case(g640, big, centre, corners, wcap=512, flags=ref.NO_CORNER, window=256, spacing=7, path_flags=PATH_DIAGONAL, same=False,
                            cap=2048)
    return c


def check(name, case, info, ents, idxs, xys):
    """the fixture is what its name claims, by the reference's result"""
    cfg, paths = case["cfg"], case["paths"]
    nx = GRIDS[case["grid"]][1][0]
    anchors_of = lambda s: [i for i in idxs[s].tolist() if i >= 0]   # noqa: E731
    for s, p in enumerate(paths):
        r = info[s]
        assert int(r["n_src"]) == len(p) and int(r["n_waypoints"]) == len(ents[s]) <= case["wcap"]
        assert int(r["n_anchors"]) == len(anchors_of(s))
        if len(p) == 0:
            assert r.tolist() == (ref.EMPTY, 0, 0, 0, 0, 0, 0, -1)
        else:
            assert int(r["end_entry"]) == int(ents[s][-1]) and int(ents[s][0]) == p[0]
            assert (int(r["status"]) == ref.OK) == (int(idxs[s][-1]) == len(p) - 1 and int(ents[s][-1]) == p[-1])
    r0 = info[0]
    if name == "w1_spacing1":
        assert ents[0].tolist() == paths[0] and idxs[0].tolist() == list(range(len(paths[0])))
        assert int(r0["n_steps"]) == len(paths[0]) - 1 and int(r0["n_diag_steps"]) == 0
    elif name in ("w63", "w64", "w65", "w66", "w127", "w128", "w129", "w130"):
        W = cfg["window"]
        a = anchors_of(0)
        assert a[0] == 0 and a[1] == W and (W - 1 + 63) // 64 == {63: 1, 64: 1, 65: 1, 66: 2, 127: 2, 128: 2, 129: 2, 130: 3}[W]
        assert any(b - a_ < min(W, len(paths[0]) - 1 - a_) for a_, b in zip(a, a[1:]))        # a lethal cell cost a shortcut somewhere
    elif name == "lengths":
        assert [len(p) for p in paths] == [6, 0, 1, 2, 64, 65, 11, 0]
        assert info["status"].tolist() == [ref.OK, ref.EMPTY, ref.OK, ref.OK, ref.OK, ref.OK, ref.OK, ref.EMPTY]
        assert info["n_waypoints"].tolist() == [3, 0, 1, 2, 22, 23, 5, 0] and anchors_of(4) == [0, 63] and anchors_of(5) == [0, 64]
        assert info[2].tolist() == (ref.OK, 1, 1, 1, 0, 0, 0, paths[2][0])
    elif name == "pillar":
        cost = case["cost"].tolist()
        cells = [(e % nx, e // nx) for e in paths[0]]
        vis = [ref.visible(cost, nx, cfg["max_cost"], False, cells[0], cells[j]) for j in range(1, 16)]
        assert vis == [True] * 12 + [False, False, True] and anchors_of(0) == [0, 15]
    elif name == "wall_gap":
        gap = ent(case["grid"], 120, 50)
        a = anchors_of(0)
        assert int(r0["status"]) == ref.OK and 3 <= len(a) <= 6 and int(r0["max_cost_seen"]) == 0
        assert any(abs(paths[0][i] - gap) <= 2 for i in a)                                     # an anchor at the gap's mouth
    elif name == "diagonal_pair":
        assert anchors_of(0) == [0, 6]
    elif name == "diagonal_pair_no_corner":
        assert anchors_of(0) == [0, 3, 6]
    elif name == "cost_at_max":
        assert anchors_of(0) == [0, len(paths[0]) - 1] and int(r0["max_cost_seen"]) == cfg["max_cost"]
    elif name == "cost_above_max":
        assert len(anchors_of(0)) > 2 and int(r0["max_cost_seen"]) <= cfg["max_cost"]
    elif name == "path_above_max":
        n = len(paths[0])
        cost = case["cost"]
        assert all(int(cost[e]) > cfg["max_cost"] for e in paths[0])
        assert anchors_of(0) == list(range(n)) and int(r0["n_waypoints"]) == n and int(r0["n_steps"]) == n - 1
        assert int(r0["max_cost_seen"]) == max(int(cost[e]) for e in paths[0]) > cfg["max_cost"]
    elif name in ("octants_both_ways", "octants_both_ways_no_corner"):
        half = len(paths) // 2
        seen = {len(anchors_of(s)) for s in range(len(paths))}
        assert seen == {2, 3}                                                                  # some lines are blocked, some are not
        cost = case["cost"].tolist()
        differs = 0
        for s in range(half):
            p, q = (paths[s][0] % nx, paths[s][0] // nx), (paths[s][2] % nx, paths[s][2] // nx)
            assert abs(q[0] - p[0]) != abs(q[1] - p[1]) or s % 6 == 3                          # shallow, steep and the diagonals
            differs += ref.line(p, q) != ref.line(q, p)[::-1]
            assert ref.visible(cost, nx, cfg["max_cost"], bool(case["flags"]), p, q) == (len(anchors_of(s)) == 2)
        assert differs > 0                                                                     # the line is directional
    elif name in ("octants", "octants_no_corner"):
        assert len(paths) == 24 and (info["status"] == ref.OK).all()
    elif name == "between_63_64_65_129":
        assert [len(e) - 2 for e in ents] == [63, 64, 65, 129] and all(anchors_of(s) == [0, len(paths[s]) - 1] for s in range(4))
    elif name.startswith("spacing_"):
        sp = cfg["spacing"]
        assert anchors_of(0) == [0, 15] and int(r0["n_steps"]) == 10 and int(r0["n_diag_steps"]) == 5
        assert int(r0["n_waypoints"]) == {1: 11, 2: 6, 10: 2, 11: 2}[sp]
    elif name == "wcap_exact":
        assert int(r0["status"]) == ref.OK and int(r0["n_waypoints"]) == case["wcap"]
    elif name == "wcap_on_anchor":
        assert int(r0["status"]) == ref.TRUNCATED and int(r0["n_waypoints"]) == case["wcap"] and int(idxs[0][-1]) >= 0
    elif name == "wcap_mid_segment":
        assert int(r0["status"]) == ref.TRUNCATED and int(r0["n_waypoints"]) == case["wcap"] and int(idxs[0][-1]) == -1
    elif name == "wcap_1":
        assert r0.tolist() == (ref.TRUNCATED, 1, 1, len(paths[0]), 9, 0, 0, paths[0][0])
    elif name == "s256":
        assert len(paths) == 256 and (info["status"] != ref.EMPTY).all() and (info["status"] == ref.TRUNCATED).any()
    elif name in ("map_edge", "map_edge_far_corner"):
        xs, ys = np.asarray(paths[0]) % nx, np.asarray(paths[0]) // nx
        assert ((xs == xs[-1]) | (ys == ys[0])).all() and {int(xs[-1]), int(ys[0])} <= {0, 249, 99}
        assert int(r0["status"]) == ref.OK and (len(anchors_of(0)) == 2) == (name == "map_edge_far_corner")
    elif name == "random_640":
        assert (info["status"] == ref.OK).all() and (info["n_anchors"] > 2).any() and int(info["n_src"].max()) > 600
    else:
        raise AssertionError(name)
