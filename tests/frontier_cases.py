"""[EXTENSION] X19 frontier clusters: the fixtures of test_frontier_host.py and test_gpu_frontier.py.  A case is a packed
int8 layer in data order (ny, nx) made of values a planted log-odds layer can reach (11..97, 50, -1), a configuration,
the caps to call with, and for the host tests a synthetic costmap or field.  Every case comes with a check that it is
what its name claims (check(name, ...) below, run by the host tests against frontier_ref).  Tiles and bitmap words are 64
wide: 130 x 70, 200 x 80 and 128 x 128 reach every edge; one case is 640 x 640 (100 tiles)."""
import functools

import numpy as np

import frontier_ref as ref

GRIDS = {"130x70": ((13, 7, 0.1), (130, 70)), "200x80": ((20, 8, 0.1), (200, 80)), "128x128": ((128, 128, 1.0), (128, 128)),
         "640x640": ((64, 64, 0.1), (640, 640))}
FREE, UNKNOWN, OCC = 11, 50, 97
CFG = ref.config()            # FREE 0..25, UNKNOWN 40..60
BLOCKED = 0xFFFFFFFF


def grid_of(name):
    return ref.grid(*GRIDS[name][0])


def shape(grid, cells):
    """an occupied layer in which exactly `cells` [(x, y)] are frontier cells: they are FREE, and each gets an UNKNOWN
    4-neighbour that is none of them"""
    nx, ny = GRIDS[grid][1]
    occ = np.full((ny, nx), OCC, np.int8)
    S = set(cells)
    for x, y in S:
        occ[y, x] = FREE
    for x, y in sorted(S, key=lambda c: (c[1], c[0])):
        nb = [(x, y - 1), (x - 1, y), (x + 1, y), (x, y + 1)]
        nb = [(a, b) for a, b in nb if 0 <= a < nx and 0 <= b < ny and (a, b) not in S]
        if not any(occ[b, a] == UNKNOWN for a, b in nb):
            assert nb, (x, y)
            occ[nb[0][1], nb[0][0]] = UNKNOWN
    assert set(zip(*np.nonzero(ref.frontier_mask(occ, CFG))[::-1])) == S
    return occ


def _case(grid, occ, cfg=CFG, caps=(64,), cost=None, field=None):
    return dict(grid=grid, occ=occ, cfg=dict(cfg), caps=tuple(caps), cost=cost, field=field)


def _serpentine():
    cells = []
    for k, y in enumerate(range(64, 126, 2)):            # corridors on every other row of tile (1, 1) of 128 x 128
        cells += [(x, y) for x in range(64, 127)]
        if y + 2 < 126:
            cells.append((126 if k % 2 == 0 else 64, y + 1))
    return cells


def _blobs(seed=19):
    nx, ny = GRIDS["640x640"][1]
    rng = np.random.default_rng(seed)
    occ = np.full((ny, nx), UNKNOWN, np.int8)
    yy, xx = np.mgrid[0:ny, 0:nx]
    for _ in range(60):
        cx, cy, r = rng.integers(0, nx), rng.integers(0, ny), rng.integers(6, 70)
        occ[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = FREE
    for _ in range(40):
        cx, cy, r = rng.integers(0, nx), rng.integers(0, ny), rng.integers(2, 14)
        occ[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = UNKNOWN
    occ[rng.random((ny, nx)) < 0.01] = OCC
    occ[rng.random((ny, nx)) < 0.002] = -1
    return occ


def _field_case():
    """four horizontal runs on 200 x 80 and a synthetic field: run 0 has a tie of its smallest value and a blocked and an
    unreachable cell, run 1 is wholly unreachable, runs 2 and 3 tie in field_min and in n_cells"""
    nx, ny = GRIDS["200x80"][1]
    runs = [[(x, 10) for x in range(20, 90)], [(x, 30) for x in range(50, 80)], [(x, 50) for x in range(10, 50)],
            [(x, 50) for x in range(120, 160)]]
    occ = shape("200x80", [c for r in runs for c in r])
    field = np.full(ny * nx, ref.UNREACHABLE, np.uint32)
    for x, y in runs[0]:
        field[y * nx + x] = 7 + abs(x - 55)
    field[10 * nx + 54] = field[10 * nx + 56] = 5          # the tie: the smaller entry wins
    field[10 * nx + 55] = BLOCKED
    field[10 * nx + 40] = ref.UNREACHABLE
    for r in runs[2:]:
        for x, y in r:
            field[y * nx + x] = 3 + (x - r[0][0])
    return _case("200x80", occ, caps=(8, 3), field=field)


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    c["corner_diagonals"] = _case("200x80", shape("200x80", [(63, 63), (64, 64), (128, 63), (127, 64)]))
    c["border_runs"] = _case("200x80", shape("200x80", [(x, 20) for x in range(50, 81)] + [(20, y) for y in range(50, 80)] +
                                              [(x, 63) for x in range(100, 140)] + [(x, 66) for x in range(100, 140)]))
    c["no_wrap"] = _case("130x70", shape("130x70", [(129, 10), (0, 11), (129, 69), (0, 0)]))
    c["u_across_tiles"] = _case("200x80", shape("200x80", [(10, y) for y in range(30, 71)] + [(20, y) for y in range(30, 71)] +
                                                 [(x, 70) for x in range(11, 20)]))
    c["comb"] = _case("200x80", shape("200x80", [(x, y) for x in range(3, 61, 3) for y in range(10, 66)] + [(x, 66) for x in range(3, 61)]))
    c["staircase"] = _case("200x80", shape("200x80", [(30 + i, 2 + i) for i in range(76)]))
    c["serpentine"] = _case("128x128", shape("128x128", _serpentine()))
    nx, ny = GRIDS["200x80"][1]
    yy, xx = np.mgrid[0:ny, 0:nx]
    c["checkerboard"] = _case("200x80", np.where((xx + yy) % 2 == 0, FREE, UNKNOWN).astype(np.int8))
    dots = np.full((ny, nx), UNKNOWN, np.int8)
    dots[1::3, 1::3] = FREE
    c["isolated_dots"] = _case("200x80", dots, caps=(4096, 64))
    for name, v in (("none_all_free", FREE), ("none_all_unknown", UNKNOWN), ("none_all_occupied", OCC)):
        c[name] = _case("130x70", np.full((70, 130), v, np.int8))
    edges = np.full((70, 130), OCC, np.int8)
    vals = [CFG["free_max"], CFG["free_max"] + 1, CFG["unknown_min"] - 1, CFG["unknown_min"], CFG["unknown_max"],
            CFG["unknown_max"] + 1, -1]
    for i, a in enumerate(vals):                          # every ordered pair of the edge values side by side
        for j, b in enumerate(vals):
            edges[2 + 3 * i, 2 + 3 * j], edges[2 + 3 * i, 3 + 3 * j] = a, b
            edges[30 + 4 * i, 60 + 2 * j], edges[31 + 4 * i, 60 + 2 * j] = a, b
    c["class_edges"] = _case("130x70", edges)
    m = 4
    c["min_cells_edges"] = _case("200x80", shape("200x80", [(x, 5) for x in range(10, 10 + m - 1)] + [(x, 15) for x in range(60, 60 + m)] +
                                                  [(x, 25) for x in range(62, 62 + m + 1)]), cfg=ref.config(min_cells=m))
    c["cap_edges"] = _case("200x80", shape("200x80", [(10 + 30 * k + i, 8 + 12 * k) for k in range(5) for i in range(2 + k)]), caps=(1, 4, 5, 6))
    wall = np.full((ny, nx), FREE, np.int8)               # unknown above row 10: the frontier is row 10, the whole width
    wall[0:10, :] = UNKNOWN
    wall[12:21, 100] = OCC                                # a wall two cells under its middle
    cost = np.zeros((ny, nx), np.uint8)
    cost[8:14, 95:106] = 120
    cost[12:21, 100] = 254
    for mc in (1, 253, 256):
        c["cost_gate_%d" % mc] = _case("200x80", wall, cfg=ref.config(max_cost=mc), cost=cost.reshape(-1))
    ring = [(x, y) for x in range(36, 45) for y in range(36, 45) if x in (36, 44) or y in (36, 44)]
    c["ring"] = _case("130x70", shape("130x70", ring))
    c["field"] = _field_case()
    c["blobs_640"] = _case("640x640", _blobs(), cfg=ref.config(min_cells=3), caps=(4096, 16))
    return c


def check(name, case, info, recs, labels):
    """the fixture is what its name claims, by the reference's result for its first cap (without the field)"""
    nx = GRIDS[case["grid"]][1][0]
    n = [int(r["n_cells"]) for r in recs[:int(info["n_written"])]]
    ent = lambda x, y: y * nx + x   # noqa: E731
    if name == "corner_diagonals":
        assert n == [2, 2] and labels[ent(64, 64)] == ent(63, 63) and labels[ent(127, 64)] == ent(128, 63)
    elif name == "border_runs":
        assert n == [31, 30, 40, 40]
    elif name == "no_wrap":
        assert n == [1, 1, 1, 1] and labels[ent(0, 11)] != labels[ent(129, 10)]
    elif name == "u_across_tiles":
        assert n == [91] and labels[ent(20, 30)] == ent(10, 30)
    elif name == "comb":
        assert n == [20 * 56 + 58]
    elif name == "staircase":
        assert n == [76] and int(recs[0]["max_x"]) - int(recs[0]["min_x"]) == 75 > 64
    elif name == "serpentine":
        assert n == [31 * 63 + 30]
    elif name == "checkerboard":
        assert n == [8000] and int(info["n_components"]) == 1
    elif name == "isolated_dots":
        assert int(info["n_components"]) == 67 * 27 == int(info["n_clusters"]) and int(info["largest"]) == 1
    elif name.startswith("none_"):
        assert info.tobytes() == np.zeros(1, ref.INFO_DTYPE).tobytes()[:16] + np.int32(-1).tobytes() + bytes(12)
    elif name == "class_edges":
        assert int(info["n_frontier_cells"]) == 2 * 2 * 2   # FREE: 25 only; UNKNOWN: 40 and 60; both orders, both directions
    elif name == "min_cells_edges":
        assert n == [4, 5] and int(info["n_components"]) == 3 and int(info["n_clusters"]) == 2
    elif name == "cap_edges":
        assert int(info["n_clusters"]) == 5 and n == [2] and int(recs[0]["label"]) == ent(10, 8)
    elif name == "cost_gate_1":
        assert n == [95, 94]
    elif name in ("cost_gate_253", "cost_gate_256"):
        assert n == [200]
    elif name == "ring":
        r = recs[0]
        assert n == [32] and (int(r["sum_x"]) // 32, int(r["sum_y"]) // 32) == (40, 40) and labels[ent(40, 40)] == ref.NONE
        assert int(r["centre_entry"]) == ent(40, 36)
    elif name == "field":
        assert n == [70, 30, 40, 40] and int(info["n_clusters"]) == 4
    elif name == "blobs_640":
        assert int(info["n_clusters"]) > 100 and int(info["largest"]) > 64 and int(info["n_components"]) > int(info["n_clusters"])
    else:
        raise AssertionError(name)
