"""[EXTENSION] X9 goal / path distance field, host side (no GPU): the header, the binding and the struct layouts; the
library's step table and its error cases; nav_ref's Dijkstra against scipy's on every fixture and against |dx| + |dy| on
empty maps; the fixtures of nav_cases.py reaching the edges they are named for; and a simulation of the device's solver
(64 x 64 tiles relaxed by directional scans, rounds, a pass cap) against the same reference, which also counts the
passes that the kernel's cap is taken from."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nav_cases as nc
import nav_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GV_ERR_BAD_ARG = 1
PASS_CAP = 40   # kNavPassCap of gv_launch_planner.hpp

LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "gridvision_hip.h"
int main(void)
{
  printf("%zu %zu %zu %zu ", sizeof(gv_nav_config), offsetof(gv_nav_config, obstacle_cost), offsetof(gv_nav_config, cost_weight),
         offsetof(gv_nav_config, flags));
  printf("%zu %zu %zu ", sizeof(gv_nav_info), offsetof(gv_nav_info, n_seeds_used), offsetof(gv_nav_info, rounds));
  printf("%zu %zu %zu %zu %zu %zu ", sizeof(gv_nav_score), offsetof(gv_nav_score, sum), offsetof(gv_nav_score, last),
         offsetof(gv_nav_score, best), offsetof(gv_nav_score, best_pose), offsetof(gv_nav_score, n_bad));
  printf("%lu %lu\n", (unsigned long)GV_NAV_BLOCKED, (unsigned long)GV_NAV_UNREACHABLE);
  return 0;
}
"""

NAMES = ["gv_nav_step_table", "gv_set_nav_config", "gv_nav_field", "gv_get_nav_field", "gv_device_nav_field",
         "gv_score_nav_async", "gv_score_nav"]


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


_FIELDS = {}


def want_field(name, cfg, seeds="goal"):
    """nav_ref's field of a fixture on the host costmap, computed once"""
    key = (name, cfg, seeds)
    if key not in _FIELDS:
        c = nc.cases()[name]
        g = nc.grid_of(c["grid"])
        _FIELDS[key] = ref.field(c["cost"], g.nx, g.ny, ref.step_table(*cfg), ref.seed_cells(g, c[seeds]))
    return _FIELDS[key]


def test_header_binding_and_layout(gvamd, tmp_path):
    """fails without the feature: the symbols, the bindings and the structs are new"""
    txt = open(os.path.join(ROOT, "include", "gridvision_hip.h")).read()
    for sig in (r"int gv_nav_step_table\(const gv_nav_config \*cfg, uint32_t table\[256\]\);",
                r"int gv_set_nav_config\(gv_handle h, const gv_nav_config \*cfg\);",
                r"int gv_nav_field\(gv_handle h, const float \*seeds_xy, int32_t S, gv_nav_info \*info[^)]*\);",
                r"int gv_get_nav_field\(gv_handle h, uint32_t \*out\);",
                r"int gv_device_nav_field\(gv_handle h, uint32_t \*\*field\);",
                r"int gv_score_nav_async\(gv_handle h, const float \*poses, int32_t K, int32_t P, uint32_t flags, "
                r"gv_nav_score \*scores\);",
                r"int gv_score_nav\(gv_handle h, const float \*poses, int32_t K, int32_t P, uint32_t flags, gv_nav_score \*scores\);"):
        assert re.search(sig, txt), sig
    assert "WAITS ON THE HOST" in txt and "convergence is data dependent" in txt
    assert "0xFFFFFFFD" in txt and "weights 0..4" in txt
    lib = gvamd.load()
    for name in NAMES:
        assert name in gvamd.ABI_SYMBOLS and hasattr(lib, name), name
    assert lib.gv_abi_version() == 4
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(LAYOUT)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", exe])
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert C.sizeof(gvamd.NavConfig) == out[0] == 12
    assert [getattr(gvamd.NavConfig, n).offset for n, _ in gvamd.NavConfig._fields_] == out[1:4]
    assert C.sizeof(gvamd.NavInfo) == out[4] == 8
    assert [getattr(gvamd.NavInfo, n).offset for n, _ in gvamd.NavInfo._fields_] == out[5:7]
    assert gvamd.NAV_SCORE_DTYPE.itemsize == out[7] == 24 == ref.SCORE_DTYPE.itemsize
    assert [gvamd.NAV_SCORE_DTYPE.fields[n][1] for n in gvamd.NAV_SCORE_DTYPE.names] == out[8:13]
    assert gvamd.NAV_SCORE_DTYPE == ref.SCORE_DTYPE
    assert (gvamd.NAV_BLOCKED, gvamd.NAV_UNREACHABLE) == (out[13], out[14]) == (ref.BLOCKED, ref.UNREACHABLE)


@pytest.mark.parametrize("obstacle_cost", [1, 253, 254, 255])
@pytest.mark.parametrize("cost_weight", [0, 1, 255])
def test_step_table_equals_the_reference(gvamd, obstacle_cost, cost_weight):
    got = gvamd.nav_step_table(gvamd.NavConfig(obstacle_cost, cost_weight, 0))
    want = ref.step_table(obstacle_cost, cost_weight)
    assert got.dtype == np.uint32 and got.tobytes() == want.tobytes()
    assert (got[obstacle_cost:] == 0).all() and (got[:obstacle_cost] >= 1).all() and got[0] == 1
    if cost_weight == 0:
        assert (got[:obstacle_cost] == 1).all()           # MapGridCritic's hop count


def test_error_cases_touch_no_device(gvamd):
    lib = gvamd.load()
    table = np.full(256, 7, np.uint32)
    p = table.ctypes.data_as(C.c_void_p)
    ok = gvamd.NavConfig(253, 3, 0)
    assert lib.gv_nav_step_table(C.byref(ok), p) == 0 and table[252] == 1 + 3 * 252
    table[:] = 7
    assert lib.gv_nav_step_table(None, p) == GV_ERR_BAD_ARG and lib.gv_nav_step_table(C.byref(ok), None) == GV_ERR_BAD_ARG
    for oc, w, fl in ((0, 0, 0), (256, 0, 0), (-1, 0, 0), (253, -1, 0), (253, 256, 0), (253, 0, 1)):
        bad = gvamd.NavConfig(oc, w, fl)
        assert lib.gv_nav_step_table(C.byref(bad), p) == GV_ERR_BAD_ARG, (oc, w, fl)
        assert lib.gv_set_nav_config(None, C.byref(bad)) == GV_ERR_BAD_ARG
    assert (table == 7).all()
    assert lib.gv_set_nav_config(None, C.byref(ok)) == GV_ERR_BAD_ARG and lib.gv_set_nav_config(None, None) == GV_ERR_BAD_ARG
    seeds = np.zeros(2, np.float32)
    sc = np.zeros(1, gvamd.NAV_SCORE_DTYPE)
    ps = np.zeros(3, np.float32)
    assert lib.gv_nav_field(None, seeds.ctypes.data_as(C.c_void_p), C.c_int32(1), None) == GV_ERR_BAD_ARG
    assert lib.gv_get_nav_field(None, p) == GV_ERR_BAD_ARG and lib.gv_device_nav_field(None, p) == GV_ERR_BAD_ARG
    for f in (lib.gv_score_nav, lib.gv_score_nav_async):
        assert f(None, ps.ctypes.data_as(C.c_void_p), C.c_int32(1), C.c_int32(1), C.c_uint32(0),
                 sc.ctypes.data_as(C.c_void_p)) == GV_ERR_BAD_ARG
    # the overflow rule of gv_set_nav_config, restated by the reference: 2000 x 2000 with obstacle cost 253
    assert [w for w in range(8) if ref.config_ok(253, w, 2000 * 2000)] == [0, 1, 2, 3, 4]
    assert ref.config_ok(255, 255, 200 * 80) and not ref.config_ok(255, 255, 500 * 200)


def _scipy_field(cost, nx, ny, step, seeds):
    """the same field from scipy.sparse.csgraph.dijkstra: an edge into every traversable cell from each of its
    traversable neighbours, weighted with the step of the cell entered"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    st = np.asarray(step, np.int64)[cost].reshape(ny, nx)
    idx = np.arange(nx * ny).reshape(ny, nx)
    rows, cols, w = [], [], []
    for src, dst in ((np.s_[:, :-1], np.s_[:, 1:]), (np.s_[:, 1:], np.s_[:, :-1]), (np.s_[:-1, :], np.s_[1:, :]),
                     (np.s_[1:, :], np.s_[:-1, :])):
        ok = (st[src] != 0) & (st[dst] != 0)
        rows.append(idx[src][ok]); cols.append(idx[dst][ok]); w.append(st[dst][ok])
    graph = coo_matrix((np.concatenate(w).astype(np.float64), (np.concatenate(rows), np.concatenate(cols))),
                       shape=(nx * ny, nx * ny)).tocsr()
    out = np.where(st.reshape(-1) == 0, ref.BLOCKED, ref.UNREACHABLE).astype(np.uint32)
    src = sorted({c for c in seeds if st.reshape(-1)[c] != 0})
    if src:
        d = dijkstra(graph, directed=True, indices=src, min_only=True)
        reach = np.isfinite(d) & (st.reshape(-1) != 0)
        out[reach] = d[reach].astype(np.uint32)      # integer sums below 2^32: exact in fp64
    return out


CASES = ["serpentine_200x80", "comb_250x100", "in_tile_200x200", "staircase", "pocket_outside", "pocket_inside",
         "random_0.3", "random_5e-4", "random_2e-3"]


def test_every_case_is_listed():
    assert sorted(CASES) == sorted(nc.cases())


@pytest.mark.parametrize("seeds", ["goal", "path"])
@pytest.mark.parametrize("name", CASES)
def test_reference_equals_scipy(name, seeds):
    c = nc.cases()[name]
    g = nc.grid_of(c["grid"])
    for cfg in ((253, 0), (254, 3)):
        got, used = want_field(name, cfg, seeds)
        cells = ref.seed_cells(g, c[seeds])
        want = _scipy_field(c["cost"], g.nx, g.ny, ref.step_table(*cfg), cells)
        assert got.tobytes() == want.tobytes(), (name, cfg)
        if seeds == "path":
            n_blocked = int((c["cost"][cells] >= 254).sum())
            assert len(cells) == nc.PATH_POINTS - c["n_off"] - c["n_nonfinite"] and n_blocked >= 1
            assert used == len(cells) - n_blocked < len(cells)
            assert len(set(cells)) < len(cells)                       # duplicates
        else:
            assert used == 1


@pytest.mark.parametrize("grid", ["250x100", "200x80"])
def test_reference_on_the_empty_map_is_the_closed_form(grid):
    g = nc.grid_of(grid)
    cost = np.zeros(g.nx * g.ny, np.uint8)
    ys, xs = np.mgrid[0:g.ny, 0:g.nx]
    for sx, sy in ((g.nx // 2, g.ny // 2), (0, 0), (g.nx - 1, g.ny - 1), (0, g.ny // 2), (g.nx // 2, 0)):
        seeds = ref.seed_cells(g, np.array([nc.world_of(g, sx, sy)], np.float32))
        assert seeds == [sy * g.nx + sx]
        got, used = ref.field(cost, g.nx, g.ny, ref.step_table(253, 0), seeds)
        assert used == 1 and np.array_equal(got.reshape(g.ny, g.nx), np.abs(xs - sx) + np.abs(ys - sy))
    got3, _ = ref.field(cost + 2, g.nx, g.ny, ref.step_table(253, 3), seeds)
    assert np.array_equal(got3, got * 7)                             # every cell costs 1 + 3 * 2


def test_fixtures_reach_their_edges():
    cs = nc.cases()
    finite = lambda f: f[f < ref.UNREACHABLE]
    f, _ = want_field("serpentine_200x80", (253, 0))
    assert int(finite(f).max()) == 8039
    f, _ = want_field("comb_250x100", (253, 0))
    assert int(finite(f).max()) == 12624
    # the in-tile path: at least 1500 steps, every reachable cell inside tile (1, 1), everything outside the box unreachable
    f, _ = want_field("in_tile_200x200", (253, 0))
    f2 = f.reshape(200, 200)
    ys, xs = np.nonzero(f2 < ref.UNREACHABLE)
    assert int(finite(f).max()) >= 1500 and ys.min() >= 64 and ys.max() < 128 and xs.min() >= 64 and xs.max() < 128
    assert (f2[:65] == ref.UNREACHABLE).all() and (f2[127:] == ref.UNREACHABLE).all()
    # the staircase: the seed is above the diagonal (x > y); no cell below it is reached
    f2 = want_field("staircase", (253, 0))[0].reshape(200, 200)
    ys, xs = np.mgrid[0:200, 0:200]
    assert (f2[xs < ys] == ref.UNREACHABLE).all() and (f2[xs > ys] < ref.UNREACHABLE).all() and (f2[xs == ys] == ref.BLOCKED).all()
    assert int((f2 == ref.UNREACHABLE).sum()) == 199 * 200 // 2
    # the pocket, from either side
    out = want_field("pocket_outside", (253, 0))[0].reshape(100, 250)
    ins = want_field("pocket_inside", (253, 0))[0].reshape(100, 250)
    assert (out[31:60, 41:90] == ref.UNREACHABLE).all() and (ins[31:60, 41:90] < ref.UNREACHABLE).all()
    assert (out[:30] < ref.UNREACHABLE).all() and (ins[:30] == ref.UNREACHABLE).all()
    for name in ("random_0.3", "random_5e-4", "random_2e-3"):
        for cfg in ((253, 0), (254, 3)):
            f, _ = want_field(name, cfg)
            assert int((f < ref.UNREACHABLE).sum()) * 10 >= f.size, name
        assert cs[name]["share"] >= 0.1
    # the cost gradient is there for the weights to act on, and acts
    assert len(set(cs["random_5e-4"]["cost"].tolist())) > 5 and len(set(cs["random_2e-3"]["cost"].tolist())) > 5
    assert want_field("random_5e-4", (253, 0))[0].tobytes() != want_field("random_5e-4", (253, 3))[0].tobytes()
    assert want_field("random_2e-3", (253, 3))[0].tobytes() != want_field("random_2e-3", (254, 3))[0].tobytes()


def test_why_the_seed_is_taken_from_the_largest_component():
    """0.3 masks leave about two thirds of 500 x 200 reachable from a central seed; at 0.41, just above the site
    percolation threshold of the square lattice, the component of a given free cell can be a handful of cells"""
    g = nc.grid_of("500x200")
    c = nc.cases()["random_0.3"]
    assert 0.6 < c["share"] < 0.75
    from scipy import ndimage
    small = 1 << 30
    for seed in range(4):
        m = nc.random_mask(g.nx, g.ny, 0.41, seed)
        lab, _ = ndimage.label(~m)
        centre = lab[g.ny // 2 - 2:g.ny // 2 + 3, g.nx // 2 - 2:g.nx // 2 + 3]
        sizes = np.bincount(lab.reshape(-1))
        small = min([small] + [int(sizes[v]) for v in centre.reshape(-1) if v])
    assert small < 50


# ------------------------------------------------------------------------------- the device's solver, simulated --
def simulate_tiles(cost, nx, ny, step, seeds, cap=PASS_CAP, T=64):
    """gv_navfield.hip's algorithm in numpy, one valid schedule of it (every tile of a round reads the field as the
    round before left it): rounds over active tiles; a tile loads its cells and a one-cell halo, runs passes of four
    directional scans (the vector index is the lane: a row for the horizontal scans, a column for the vertical ones)
    until a pass changes nothing or the cap is hit, stores what changed, marks the neighbours behind a changed border
    and itself when capped.  Returns (field, rounds, the most passes a tile ran in one round)."""
    INF = np.int64(1) << 62
    st = np.asarray(step, np.int64)[np.asarray(cost).reshape(-1)].reshape(ny, nx)
    tyn, txn = -(-ny // T), -(-nx // T)
    S = np.zeros((tyn * T + 2, txn * T + 2), np.int64)
    S[1:ny + 1, 1:nx + 1] = st
    D = np.full(S.shape, INF, np.int64)
    active = np.zeros((tyn, txn), bool)
    for c in seeds:
        y, x = divmod(c, nx)
        if st[y, x]:
            D[y + 1, x + 1] = 0
            active[y // T, x // T] = True
    rounds = most = 0
    while True:
        rounds += 1
        tiles = np.argwhere(active)
        active = np.zeros_like(active)
        changed_tiles = 0
        if len(tiles):
            B = np.stack([D[ty * T:ty * T + T + 2, tx * T:tx * T + T + 2] for ty, tx in tiles]).copy()
            W = np.stack([S[ty * T + 1:ty * T + T + 1, tx * T + 1:tx * T + T + 1] for ty, tx in tiles])
            passes = np.zeros(len(tiles), int)
            capped = np.zeros(len(tiles), bool)

            def relax(dst, src, w):
                cand = src + w
                m = (w != 0) & (src < INF) & (cand < dst)
                dst[m] = cand[m]
                return m.any(axis=1)

            for p in range(1, cap + 1):
                ch = np.zeros(len(tiles), bool)
                for x in range(1, T + 1):                       # left to right, lane = row
                    ch |= relax(B[:, 1:T + 1, x], B[:, 1:T + 1, x - 1], W[:, :, x - 1])
                for x in range(T, 0, -1):                       # right to left
                    ch |= relax(B[:, 1:T + 1, x], B[:, 1:T + 1, x + 1], W[:, :, x - 1])
                for y in range(1, T + 1):                       # down, lane = column
                    ch |= relax(B[:, y, 1:T + 1], B[:, y - 1, 1:T + 1], W[:, y - 1, :])
                for y in range(T, 0, -1):                       # up
                    ch |= relax(B[:, y, 1:T + 1], B[:, y + 1, 1:T + 1], W[:, y - 1, :])
                passes[ch] = p
                if not ch.any():
                    break
                capped = ch if p == cap else capped
            most = max(most, int(np.minimum(passes + 1, cap).max()))   # the last pass of a tile under the cap changes nothing
            for i, (ty, tx) in enumerate(tiles):
                old = D[ty * T + 1:ty * T + T + 1, tx * T + 1:tx * T + T + 1]
                new = B[i, 1:T + 1, 1:T + 1]
                diff = new != old
                if diff.any() or capped[i]:
                    changed_tiles += 1
                if capped[i]:
                    active[ty, tx] = True
                if diff[0].any() and ty > 0:
                    active[ty - 1, tx] = True
                if diff[-1].any() and ty + 1 < tyn:
                    active[ty + 1, tx] = True
                if diff[:, 0].any() and tx > 0:
                    active[ty, tx - 1] = True
                if diff[:, -1].any() and tx + 1 < txn:
                    active[ty, tx + 1] = True
                old[...] = new
        if changed_tiles == 0:
            break
    d = D[1:ny + 1, 1:nx + 1]
    out = np.where(st == 0, ref.BLOCKED, np.where(d >= INF, ref.UNREACHABLE, d)).astype(np.uint32)
    return out.reshape(-1), rounds, most


@pytest.mark.parametrize("name", CASES)
def test_simulated_tile_relaxation_equals_the_reference(name):
    c = nc.cases()[name]
    g = nc.grid_of(c["grid"])
    for cfg in ((253, 0), (253, 3)):
        want, _ = want_field(name, cfg)
        got, rounds, most = simulate_tiles(c["cost"], g.nx, g.ny, ref.step_table(*cfg), ref.seed_cells(g, c["goal"]))
        assert got.tobytes() == want.tobytes(), (name, cfg)
        print("%s %s: rounds %d, most passes of a tile in a round %d" % (name, cfg, rounds, most))
        assert most <= PASS_CAP and rounds >= 2
        if name == "in_tile_200x200":
            # where the kernel's cap comes from: 30 corridors, a pass per turn, one more pass that changes nothing
            assert rounds == 2 and 30 <= most <= 33


def test_simulation_with_a_low_cap_is_still_exact():
    """a tile that hits the cap marks itself and goes on in the next round"""
    c = nc.cases()["in_tile_200x200"]
    g = nc.grid_of(c["grid"])
    want, _ = want_field("in_tile_200x200", (253, 0))
    got, rounds, most = simulate_tiles(c["cost"], g.nx, g.ny, ref.step_table(253, 0), ref.seed_cells(g, c["goal"]), cap=3)
    assert got.tobytes() == want.tobytes() and most == 3 and rounds >= 10
