"""The scenes of tests/grid_move_cases.py, checked on the CPU with the planner's own cos / sin / tx / ty (the g++ driver of
test_grid_move_host.py; never Python's cos).  The grids are what gv_create makes of their arguments; the planted layers
show any wrong source index; the quarter turns on the mixed-parity grids put every in-map source on a cell border, where
get_index_fast's exact division decides, and a good number exactly on the map's outer edge; np_move agrees there with
the oracle's getIndex source by source, with array slicing on every translation, and with the numpy emulation of the
kernels on every scene; and every mutant of the emulation changes a layer of a named scene.
tests/test_gpu_grid_move.py runs the same scenes through gv_grid_move."""
import subprocess

import numpy as np
import pytest

import grid_move_cases as gc
import grid_move_ref as R
import oracle_lib as ol
from test_grid_move_host import _run, driver  # noqa: F401  (the fixture compiles the planner's driver)

_PLAN, _STATE = {}, {}


def plan(exe, key):
    """what gv_grid_move reports for the scene on a fresh residue"""
    if key not in _PLAN:
        g, m = gc.scene(key)
        row = _run(exe, (g.nx, g.ny, g.args[2], g.pos_x, g.pos_y), [m.tf])[0]
        _PLAN[key] = dict(applied=row["applied"], cos_yaw=row["c"], sin_yaw=row["s"], tx=row["tx"], ty=row["ty"])
    return _PLAN[key]


class OracleHandle:
    """the four public calls plant() needs, on the CPU oracle's grid"""

    def __init__(self, g):
        self.og = ol.OGrid(*g.args)
        self.nx, self.ny = self.og.nx, self.og.ny

    def set_log_odds(self, a):
        self.og.log_odds[:] = a

    def update_map(self):
        self.og.update_map()

    def log_odds(self):
        return self.og.log_odds.copy()

    def occupancy(self):
        return self.og.occupancy.copy()

    def to_occupancy_grid(self):
        return self.og.to_occupancy_grid()


def state(name):
    if name not in _STATE:
        _STATE[name] = gc.plant(OracleHandle(gc.GRID[name]), gc.GRID[name])
    return _STATE[name]


def test_grids_are_what_gv_create_makes(driver):
    for g in gc.GRIDS:
        out = subprocess.run([driver, "geometry", str(g.args[0]), str(g.args[1]), repr(g.args[2])], capture_output=True,
                             text=True, check=True).stdout.split()
        nx, ny, G = (int(v) for v in out[:3])
        res, pos_x, pos_y, len_x, len_y, off_x, off_y, inv_res = (float.fromhex(v) for v in out[3:])
        assert (nx, ny, G, res, pos_x, pos_y) == (g.nx, g.ny, g.nx * g.ny, g.args[2], g.pos_x, g.pos_y), g.name
        assert (len_x, len_y, off_x, off_y, inv_res) == (nx * res, ny * res, 0.5 * (nx * res), 0.5 * (ny * res), 1.0 / res)
        og = ol.OGrid(*g.args)
        assert (og.nx, og.ny, og.g.pos_x, og.g.pos_y, og.g.len_x, og.g.len_y) == (nx, ny, pos_x, pos_y, len_x, len_y)
    by = {(g.nx, g.ny): g for g in gc.GRIDS}
    for n in ((1, 1), (3, 1), (4, 1)):
        assert n in by and n[0] * n[1] < 16
    assert 250 % 16 and 10 % 4 and sum(g.nx == 125 and g.ny == 50 for g in gc.GRIDS) == 2
    assert 167 % 4 and (167 * 67) % 2 == 1 and (167 * 67 * 4) % 16 and 250 % 4 == 2 and 500 % 4 == 0
    for name in gc.BORDER_GRIDS:
        assert (gc.GRID[name].nx + gc.GRID[name].ny) % 2 == 1
    own = by[(300, 14)]
    assert own.nx % 4 == 0 and own.ny % 4 and (own.nx // 4) % 64 and own.nx // 4 > 64 and (own.nx * own.ny) % 16


@pytest.mark.parametrize("g", gc.GRIDS, ids=lambda g: g.name)
def test_planted_layers_show_any_wrong_source(g):
    lo, occ, i8 = state(g.name)   # plant() has checked them
    assert (i8 >= 12).all() and (i8 <= 96).all() and ((i8 - 12) % 3 == 0).all()
    want = 12 + 3 * ((np.arange(g.nx)[None, :] + 3 * np.arange(g.ny)[:, None]) % gc.RAMP)
    assert np.array_equal(i8[::-1].reshape(g.ny, g.nx), want)
    if g.nx * g.ny >= gc.RAMP * 3:
        assert len(np.unique(i8)) == gc.RAMP


def test_every_grid_has_every_motion(driver):
    for g in gc.GRIDS:
        ms = gc.motions(g)
        names = [m.name for m in ms]
        assert len(set(names)) == len(names)
        cells = {m.cells for m in ms if m.cells}
        for want in ((g.nx - 1, g.ny - 1), (g.nx, 0), (0, -g.ny), (-g.nx, g.ny)):
            assert want in cells or want == (0, 0)
        if g.nx > 3:
            assert any(kx > 0 and ky == 0 for kx, ky in cells) and any(kx < 0 and ky == 0 for kx, ky in cells)
            assert any(ky > 0 and kx == 0 for kx, ky in cells) and any(ky < 0 and kx == 0 for kx, ky in cells)
        assert sum(m.quarter for m in ms) == 6
        for m in ms:
            p = plan(driver, (g.name, m.name))
            assert p["applied"], (g.name, m.name)
            if m.cells:
                assert (p["cos_yaw"], p["sin_yaw"]) == (1.0, 0.0)
                assert (p["tx"], p["ty"]) == (g.args[2] * m.cells[0], g.args[2] * m.cells[1])
            else:
                assert p["sin_yaw"] != 0.0 or m.name == "far_away", (g.name, m.name)   # above the planner's threshold
            if m.quarter:
                assert abs(p["sin_yaw"]) == 1.0 and 0.0 < abs(p["cos_yaw"]) < 1e-15   # the planner's cos is not 0


# ------------------------------------------------------------------------------------------ the border scenes --
def border_stats(key, p):
    g, _ = gc.scene(key)
    nx, ny, res, pos_x, pos_y = gc.geom(g)
    src, sx, sy = R.np_sources(nx, ny, res, pos_x, pos_y, p)
    inside, fx, ex, fy, ey = R.fast_quotients(nx, ny, res, pos_x, pos_y, sx, sy)
    near = (np.abs(fx - np.rint(fx)) < 1e-6, np.abs(fy - np.rint(fy)) < 1e-6)
    ux, uy = -((sx - pos_x) - 0.5 * (nx * res)), -((sy - pos_y) - 0.5 * (ny * res))
    on_x, on_y = (ux == 0.0) | (ux == nx * res), (uy == 0.0) | (uy == ny * res)
    edge = (on_x & (uy >= 0.0) & (uy <= ny * res)) | (on_y & (ux >= 0.0) & (ux <= nx * res))
    return dict(inside=int(inside.sum()), near=int((near[0] & inside).sum() + (near[1] & inside).sum()),
                both=bool((near[0] & near[1])[inside].all()),
                trunc_differs=int((inside & ((np.trunc(fx) != np.trunc(ex)) | (np.trunc(fy) != np.trunc(ey)))).sum()),
                edge=int(edge.sum()), src=src, sx=sx, sy=sy)


BORDER_SCENES = [k for k in gc.SCENES if gc.is_border(k)]


def test_border_scenes_are_the_quarter_turns_on_three_grids():
    assert len(BORDER_SCENES) == 18 and {k[0] for k in BORDER_SCENES} == set(gc.BORDER_GRIDS)


@pytest.mark.parametrize("key", BORDER_SCENES, ids="-".join)
def test_border_scene_decides_by_the_exact_division(driver, key):
    g, _ = gc.scene(key)
    st = border_stats(key, plan(driver, key))
    assert st["inside"] >= 50 and st["both"] and st["near"] == 2 * st["inside"], st
    assert st["trunc_differs"] >= 20, st
    og = ol.OGrid(*g.args)   # np_move's index rule against the oracle's getIndex, source by source
    for c, (x, y, j) in enumerate(zip(st["sx"].tolist(), st["sy"].tolist(), st["src"].tolist())):
        ok, jx, jy = og.get_index(x, y)
        assert (jy * g.nx + jx if ok else -1) == j, (c, x, y)


@pytest.mark.parametrize("name", gc.BORDER_GRIDS)
def test_border_grid_has_sources_on_the_outer_edge(driver, name):
    edge = {k[1]: border_stats(k, plan(driver, k))["edge"] for k in BORDER_SCENES if k[0] == name}
    assert max(edge.values()) >= 10, edge


def test_far_edge_is_refused_twice(driver):
    """why the far_edge_le mutant changes both tests of the far edge: a source exactly on it, let through by the first
    test, has the exact quotient nx (ny) and is refused by the index range test"""
    n = 0
    for key in BORDER_SCENES:
        g, _ = gc.scene(key)
        nx, ny, res, pos_x, pos_y = gc.geom(g)
        st = border_stats(key, plan(driver, key))
        _, _, ex, _, ey = R.fast_quotients(nx, ny, res, pos_x, pos_y, st["sx"], st["sy"])
        ux, uy = -((st["sx"] - pos_x) - 0.5 * (nx * res)), -((st["sy"] - pos_y) - 0.5 * (ny * res))
        assert (ex[ux == nx * res] == nx).all() and (ey[uy == ny * res] == ny).all(), key
        n += int((ux == nx * res).sum() + (uy == ny * res).sum())
    assert n >= 100


def test_parity_is_what_makes_a_border_scene(driver):
    """where the parities of nx and ny agree, a quarter turn puts no quotient near an integer"""
    for key in gc.SCENES:
        g, m = gc.scene(key)
        if m.quarter and key[0] not in gc.BORDER_GRIDS and g.nx > 4:
            assert border_stats(key, plan(driver, key))["near"] == 0, key


# ------------------------------------------------------------------------------------- references against each other --
@pytest.mark.parametrize("g", gc.GRIDS, ids=lambda g: g.name)
def test_np_move_equals_slicing_on_translations(driver, g):
    n = 0
    for m in gc.motions(g):
        if m.cells:
            p = plan(driver, (g.name, m.name))
            got, want = R.np_move(state(g.name), *gc.geom(g), p), R.slice_move(state(g.name), g.nx, g.ny, *m.cells)
            assert not R.same(got, want), (g.name, m.name)
            kept = max(g.nx - abs(m.cells[0]), 0) * max(g.ny - abs(m.cells[1]), 0)
            assert int((R.np_sources(*gc.geom(g), p)[0] >= 0).sum()) == kept
            n += 1
    assert n >= (2 if g.nx * g.ny == 1 else 8)


@pytest.mark.parametrize("g", gc.GRIDS, ids=lambda g: g.name)
def test_emulation_as_written_equals_np_move(driver, g):
    for m in gc.motions(g):
        p = plan(driver, (g.name, m.name))
        want = R.np_move(state(g.name), *gc.geom(g), p)
        got = R.emulate(state(g.name), *gc.geom(g), p)
        assert not R.same(got, want), (g.name, m.name, R.first_difference(got, want, g.nx, R.np_sources(*gc.geom(g), p)[0]))
        if m.name == "far_away":
            assert not want[0].any() and (want[1] == 0.5).all() and (want[2] == 50).all()
        elif g.nx * g.ny >= 250 and m.name != "yaw_1.01th":   # (half a cell at the far corner moves no cell centre across a border)
            assert R.same(want, state(g.name)) == list(R.LAYERS)   # the move changes every layer


@pytest.mark.parametrize("name", ["25x10@0.2", "167x67@0.3"])
def test_four_quarter_turns_keep_non_finite_values_aboard(driver, name):
    """the chain tests/test_gpu_grid_move.py runs, with the residue carried from turn to turn as the handle carries it"""
    g = gc.GRID[name]
    rows = _run(driver, (g.nx, g.ny, g.args[2], g.pos_x, g.pos_y), [(0.0, 0.0, gc.Q[0], gc.Q[1], 0.0, 0.0, 0.0)] * 4)
    st = state(name)
    for k, row in enumerate(rows):
        p = dict(cos_yaw=row["c"], sin_yaw=row["s"], tx=row["tx"], ty=row["ty"])
        assert row["applied"] and abs(row["s"]) == 1.0
        want = R.np_move(st, *gc.geom(g), p)
        assert not R.same(R.emulate(st, *gc.geom(g), p), want), (name, k)
        assert R.same(want, st) == list(R.LAYERS)
        st = want
        assert np.isnan(st[0]).any() and np.isinf(st[0]).any(), k
    assert len(np.unique(st[0].view(np.uint32))) >= 20   # and a patch of the planted map around the base origin


# the scenes every mutant runs on: all of every grid below 12000 cells, and the reference's grid for k_grid_move4
MUTANT_SCENES = [k for k in gc.SCENES if gc.GRID[k[0]].nx * gc.GRID[k[0]].ny < 12000] + \
                [("500x200@0.1", "t+x-y"), ("500x200@0.1", "yaw_0.3_t")]
# a scene that must see the mutant
SEEN_BY = {
    "always_fast": ("25x10@0.2", "+q_0_0"),
    "exact_uses_product": ("125x50@0.04", "-q_7_5"),
    "sin_negated": ("167x67@0.3", "yaw_3th"),
    "source_transposed": ("25x10@0.2", "t+y"),
    "far_edge_le": ("25x10@0.2", "+q_0_0"),
    "near_edge_gt": ("25x10@0.2", "+q_0_0"),
    "packed_not_reversed": ("300x14@0.5", "t+x"),
    "fill_i8_0": ("3x1@1", "t+x"),
    "fill_occ_0": ("3x1@1", "t+x"),
    "last_row_block_skipped": ("25x10@0.2", "t+x"),
    "drop_tail_log_odds": ("167x67@0.3", "t+x"),
    "drop_tail_occupancy": ("167x67@0.3", "t+x"),
    "drop_tail_int8": ("300x14@0.5", "t+x"),
    "occ_segment_unrounded": ("167x67@0.3", "t+x"),
}


def _seen(exe, mutant):
    found = {}
    for key in MUTANT_SCENES:
        g, _ = gc.scene(key)
        p = plan(exe, key)
        layers = R.same(R.emulate(state(key[0]), *gc.geom(g), p, mutant), R.np_move(state(key[0]), *gc.geom(g), p))
        if layers:
            found[key] = layers
    return found


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_is_seen_by_a_named_scene(driver, mutant):
    found = _seen(driver, mutant)
    assert SEEN_BY[mutant] in found, (mutant, sorted(found)[:8])
    if mutant in ("always_fast", "exact_uses_product"):   # only the border scenes reach the fallback
        assert set(found) <= set(BORDER_SCENES) and len(found) == len(BORDER_SCENES), sorted(found)
        assert all(v == list(R.LAYERS) for v in found.values())
    if mutant.startswith("drop_tail_"):
        assert all(v == [mutant[len("drop_tail_"):]] for v in found.values())
    if mutant == "fill_i8_0":
        assert all(v == ["int8"] for v in found.values())
    if mutant in ("fill_occ_0", "occ_segment_unrounded"):
        assert all(v == ["occupancy"] for v in found.values())
    if mutant == "packed_not_reversed":
        assert all(gc.GRID[k[0]].nx % 4 == 0 and v == ["int8"] for k, v in found.items())
    if mutant == "last_row_block_skipped":
        assert all(gc.GRID[k[0]].ny % 4 for k in found)


def test_set_of_mutants_is_the_listed_one():
    assert set(SEEN_BY) == set(R.MUTANTS) and len(R.MUTANTS) == 14
