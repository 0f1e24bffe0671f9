"""host::SectorPlan (csrc/gv_host_math.hpp) through the test hook gv_test_sector_plan, on the CPU: how the library cuts the
eight wedges around the origin cell into workgroups of k_ray_sectors, and whether what the kernel relies on holds.

The plan's violations() is the library's own list of those preconditions.  Here the defaults are swept and never
violate it; its closed-form column-width bound is checked against the kernel's col_bounds rule evaluated column by
column in numpy; the host twin of the kernel's blockIdx decode covers every (octant, sector) exactly once; a rank's
share of the dispatch partitions it; every (scene set, knob set) pair tests/test_gpu_ray_ends.py runs is accepted and
the two it excludes are refused for their column width; and the sector counts tests/ray_cases.py builds its boundary
scenes on are the ones the library picks."""
import functools

import numpy as np
import pytest

import ray_cases as rc
import traj_ref

MAX_STAT_SLOTS = 8 << 12      # kMaxStatSlots
LDS_MAX = 160 * 1024          # kSectorLdsMax: the LDS of a CU
GRIDS = ((64, 64), (1024, 1024), (2000, 2000), (5100, 80), (4200, 4200), (8000, 8000))
POINTS = (0, 1, 10 ** 3, 10 ** 6, 10 ** 7)


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


@pytest.fixture
def knobs(monkeypatch):
    """set(tune): the environment holds exactly this knob set"""
    def set_(tune):
        for k in rc.KNOBS + ("GV_LOG2S_OCT",):
            monkeypatch.delenv(k, raising=False)
        for k, v in tune.items():
            monkeypatch.setenv(k, v)
    set_({})
    return set_


def origins(nx, ny):
    """corners, edge midpoints, centre, the scene sets' origins, and 511 / 512 / 513 cells from each edge"""
    mx, my = nx // 2, ny // 2
    o = [(0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1), (mx, 0), (mx, ny - 1), (0, my), (nx - 1, my), (mx, my)]
    o += [org for _, org in rc.SETS.values()]
    for d in (511, 512, 513):
        o += [(d, my), (nx - 1 - d, my), (mx, d), (mx, ny - 1 - d)]
    return sorted({(x, y) for x, y in o if 0 <= x < nx and 0 <= y < ny})


def sweep():
    return [(nx, ny, cx, cy, n) for nx, ny in GRIDS for cx, cy in origins(nx, ny) for n in POINTS]


def wedge(nx, ny, cx, cy, o):
    """(len, jmaxo, xmaj, bmin) of octant o: the kernel's make_octant"""
    xmaj, pmaj, pmin = (o >> 2) & 1, (o >> 1) & 1, o & 1
    lx, ly = (nx - 1 - cx, cx), (ny - 1 - cy, cy)
    ln, jmax = (lx[0 if pmaj else 1], ly[0 if pmin else 1]) if xmaj else (ly[0 if pmaj else 1], lx[0 if pmin else 1])
    return ln, jmax, xmaj, 0 if pmin else 1


@functools.lru_cache(maxsize=None)
def widest_column(ln, jmax, xmaj, bmin, log2s, a_first):
    """the widest column a_first .. ln of any sector of a wedge, straight from the kernel's col_bounds"""
    S = 1 << log2s
    a = np.arange(a_first, ln + 1, dtype=np.int64)[:, None]
    s = np.arange(S, dtype=np.int64)[None, :]
    bmaxa = a if xmaj else a - 1
    blo = (a * s + S - 1) >> log2s
    bhi = ((a * (s + 1) + S - 1) >> log2s) - 1
    bhi = np.where(s == S - 1, bmaxa, bhi)
    blo = np.maximum(blo, bmin)
    bhi = np.minimum(np.minimum(bhi, bmaxa), jmax)
    return int(np.max(bhi - blo + 1))


def check_width(P, nx, ny, cx, cy):
    """6b: with no violation, no column of any sector is wider than one 32-bit word"""
    for o in range(8):
        ln, jmax, xmaj, bmin = wedge(nx, ny, cx, cy, o)
        assert ln == P["len"][o]
        if ln < 1:
            continue
        # (the width does not decrease with a: all columns up to 1024 cells, the last 64 of a longer wedge)
        a_first = 1 if max(nx, ny) <= 1024 else max(1, ln - 63)
        w = widest_column(ln, jmax, xmaj, bmin, P["log2s_oct"][o], a_first)
        assert w <= 32, (nx, ny, cx, cy, o, ln, P["log2s_oct"][o], w)


def check_decode(P):
    """6c: the dispatch order covers the wedges exactly once"""
    wg, nh, S = P["wg"], P["n_helpers"], [1 << l for l in P["log2s_oct"]]
    assert len(wg) == P["total_workgroups"] == P["wg_base"][8] + nh and nh in (0, 16)
    octant, sector, helper, part, nparts, slot, idle = wg.T
    assert np.array_equal(helper, (np.arange(len(wg)) < nh).astype(np.int32)) and np.array_equal(part, helper)
    main = wg[nh:]
    pairs = sorted(map(tuple, main[:, :2].tolist()))
    assert pairs == [(o, s) for o in range(8) for s in range(S[o])]   # every (octant, sector) once, those with len >= 1 included
    order = list(dict.fromkeys(main[:, 0].tolist()))                   # octants in dispatch order
    if P["reorder"]:
        assert order == sorted(range(8), key=lambda o: -P["len"][o])   # descending length, stable
        for o in range(8):
            if S[o] >= 8:
                assert main[main[:, 0] == o][:4, 1].tolist() == [0, S[o] // 2 - 1, S[o] - 1, S[o] // 2]
    else:
        assert order == list(range(8)) and np.array_equal(main[:, 1], np.concatenate([np.arange(S[o]) for o in range(8)]))
    for b in range(nh):   # helper 2q + e: the octant at dispatch position q, sector e ? S - 1 : 0
        o = order[b >> 1]
        assert (octant[b], sector[b]) == (o, S[o] - 1 if b & 1 else 0)
    # no knob reaches a one-sector octant (an override must be > 0: S >= 2), so no helper is ever idle
    assert not idle.any()
    last = np.array([S[o] - 1 for o in octant])
    assert np.array_equal(nparts, np.where((nh > 0) & ((sector == 0) | (sector == last)), 2, 1))
    assert len(set(slot.tolist())) == len(slot) and slot.min() >= 0
    assert slot.max() < P["stat_slots"] <= MAX_STAT_SLOTS


def check_rank_shares(P):
    """6d: the launcher's rule grid = (total - first + stride - 1) / stride, first = rank, stride = world"""
    total = P["total_workgroups"]
    for world in (1, 2, 3, 8):
        seen = np.zeros(total, np.int32)
        for rank in range(world):
            grid = (total - rank + world - 1) // world if rank < total else 0
            np.add.at(seen, rank + np.arange(grid) * world, 1)
        assert (seen == 1).all()


def test_defaults_never_violate(gvamd, knobs):
    """6a - 6d over grids from 64 x 64 to 8000 x 8000, origins on corners, edges, the centre and 511 .. 513 cells from an
    edge, and clouds of 0 to 10^7 points"""
    cases = sweep()
    assert len(cases) > 500
    for nx, ny, cx, cy, n in cases:
        P = gvamd.sector_plan(nx, ny, cx, cy, n)
        assert P["violations"] == 0, (nx, ny, cx, cy, n, P["violated"])
        assert P["imax"] == max(cx, nx - 1 - cx, cy, ny - 1 - cy)
        assert P["ch"] == min(c for c in (4, 8, 16) if c * 512 >= P["imax"])
        assert P["cap"] in (2048, 4096)
        assert P["marks_words"] % 2 == 0 and P["marks_words"] >= P["imax"] + 1
        assert P["lds_bytes"] <= LDS_MAX
        check_width(P, nx, ny, cx, cy)
        check_decode(P)
        check_rank_shares(P)


@pytest.mark.parametrize("tune", [{"GV_SECTOR_HELPERS": "1"}, {"GV_SECTOR_HELPERS": "0"}, {"GV_SECTOR_REORDER": "0"},
                                  {"GV_SECTOR_REORDER": "0", "GV_SECTOR_HELPERS": "1"}, {"GV_LOG2S": "1", "GV_SECTOR_HELPERS": "1"}],
                         ids=["helpers1", "helpers0", "reorder0", "reorder0_helpers1", "two_sectors"])
def test_decode_under_the_dispatch_knobs(gvamd, knobs, tune):
    """6c and 6d with the helpers forced on and off, in natural order, and with two sectors per octant (G64 under
    GV_LOG2S=1: sectors 0 and S - 1 are all there is, both have helpers, columns exactly 32 cells wide)"""
    knobs(tune)
    grids = ((64, 64),) if "GV_LOG2S" in tune else GRIDS
    for nx, ny in grids:
        for cx, cy in origins(nx, ny):
            for n in (10 ** 3, 10 ** 7):
                P = gvamd.sector_plan(nx, ny, cx, cy, n)
                assert P["violations"] == 0
                check_width(P, nx, ny, cx, cy)
                check_decode(P)
                check_rank_shares(P)
    if "GV_LOG2S" in tune:
        assert P["log2s_oct"] == [1] * 8 and (P["wg"][:, 4] == 2).all()


def gpu_pairs():
    """((grid, origin), knob set name, knob set): what tests/test_gpu_ray_ends.py runs, and what it excludes"""
    centre = rc.SETS["g1024_centre"]
    run = [(rc.SETS[n], t, rc.TUNE_BD[t]) for n in rc.SETS for t in rc.TUNE_BD if not (t.startswith("log2s") and n == "g5100")]
    run += [(centre, t, rc.TAILS_B[t]) for t in rc.TAILS_B]
    run += [(rc.SETS[n], t, rc.TUNE_C[t]) for n in rc.SETS for t in rc.TUNE_C]
    run += [(centre, t, rc.TUNE_C[t]) for t in rc.TUNE_C if t != "cap2048"]
    run += [(centre, t, rc.TUNE_BD[t]) for t in rc.TUNE_BD]
    run += [((rc.G4200, (0, 0)), "defaults", {})]
    run += [((rc.G64, o), "defaults", {}) for o in rc.origins_a(rc.G64).values()]
    excluded = [(rc.SETS["g5100"], t, rc.TUNE_BD[t]) for t in ("log2s5", "log2s6")]
    return run, excluded


def test_gpu_suite_knob_sets(gvamd, knobs):
    """6e: the plan accepts every (scene set, knob set) pair the GPU suite runs, for clouds from a single end to the
    densest band scene, and keeps its columns within 32 cells there; the pairs the suite excludes by hand (GV_LOG2S = 5
    and 6 on G5100: 32 or 64 sectors for a wedge of 4990 columns) it refuses for their column width"""
    run, excluded = gpu_pairs()
    assert len(run) >= 80
    for (grid, (cx, cy)), name, tune in run:
        g = traj_ref.grid(*grid)
        knobs(tune)
        for n in (1, 100, 10 ** 4, 10 ** 5, 2 * 10 ** 5):
            P = gvamd.sector_plan(g.nx, g.ny, cx, cy, n, workgroups=False)
            assert P["violations"] == 0, (grid, name, n, P["violated"])
            check_width(P, g.nx, g.ny, cx, cy)
    for (grid, (cx, cy)), name, tune in excluded:
        g = traj_ref.grid(*grid)
        knobs(tune)
        P = gvamd.sector_plan(g.nx, g.ny, cx, cy, 1000, workgroups=False)
        assert "wide_column" in P["violated"], (name, P["violated"])
        assert P["len"][4] == 4990 and P["len"][4] // (1 << P["log2s_oct"][4]) + 1 > 32


def test_knobs_can_violate_each_condition(gvamd, knobs):
    """the bits a sweep knob can reach, each through the knob that reaches it"""
    for tune, bit, grid in (({"GV_LOG2S": "13"}, "sector_count", (64, 64)), ({"GV_LOG2S": "12", "GV_SECTOR_HELPERS": "1"}, "workgroups", (64, 64)),
                            ({"GV_CAP": "70000"}, "cap", (64, 64)), ({"GV_CAP": "32768"}, "lds", (64, 64)),
                            ({"GV_LOG2S": "3"}, "wide_column", (1024, 1024))):
        knobs(tune)
        P = gvamd.sector_plan(*grid, grid[0] // 2, grid[1] // 2, 1000, workgroups=False)
        assert bit in P["violated"], (tune, P["violated"])


def test_scene_assumptions(gvamd, knobs):
    """6f: the sector counts tests/ray_cases.py places its boundary scenes by"""
    g = traj_ref.grid(*rc.G64)
    for cx, cy in rc.origins_a(rc.G64).values():   # "64 x 64 cells: one tile, 8 sectors per octant"
        P = gvamd.sector_plan(g.nx, g.ny, cx, cy, 1, workgroups=False)
        assert all(P["log2s_oct"][o] == 3 for o in range(8) if P["len"][o] >= 1)
    g = traj_ref.grid(*rc.G1024)
    for n in (1, 10 ** 5):   # T_LOG2S, and family_b_short's "first level boundary, S / 2 = 16"
        P = gvamd.sector_plan(g.nx, g.ny, *rc.O1024_CENTRE, n, workgroups=False)
        assert sorted(set(P["len"])) == [511, 512] and P["log2s_oct"] == [rc.T_LOG2S] * 8 and rc.T_LOG2S == 5
    for grid, org in ((rc.G5100, rc.O5100), (rc.G4200, (0, 0))):   # "runs k_ray_sectors<16>"
        g = traj_ref.grid(*grid)
        assert gvamd.sector_plan(g.nx, g.ny, *org, 3000, workgroups=False)["ch"] == 16
