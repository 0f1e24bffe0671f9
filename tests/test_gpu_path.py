"""[EXTENSION] X17 path extraction on the device: gv_nav_path against path_ref (a plain Python walk) run on the device's own
field read-back, and against the host twin, with zero tolerance.  Every call is made three times and gives the same
bytes; every comparison is tobytes() equality of the records, of the entries and of the cell centres up to n_cells.
Grids of at most 500 x 200, plus one call at 2000 x 2000.  Then gv_nav_field_from_path against gv_nav_field over the
path's own centres, the destinations, the ordering and state rules of the header, and the example."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nav_cases as nc
import path_cases as pc
import path_ref as ref
from planner_util import first_diff, hip_runtime, plant

pytestmark = pytest.mark.gpu

GV_ERR_BAD_ARG, GV_ERR_STATE = 1, 5
HERE = os.path.dirname(os.path.abspath(__file__))
_HANDLES = {}   # grid name -> handle, shared by the cases of the module


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    yield m
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()


def _handle(gvamd, grid):
    if grid not in _HANDLES:
        (gx, gy, res), (nx, ny) = nc.GRIDS[grid]
        h = gvamd.GridVisionHIP(gx, gy, res)
        assert (h.nx, h.ny) == (nx, ny)
        _HANDLES[grid] = h
    h = _HANDLES[grid]
    h.reset()
    return h


def _resident(h):
    """(info (S,), entries (S, cap), xy (S, cap, 2)) of the resident paths, through gv_device_nav_path's pointers"""
    hip = hip_runtime()
    d = h.device_nav_path()
    S, cap = d["S"], d["cap"]
    info, ent, xy = np.zeros(S, ref.INFO_DTYPE), np.zeros((S, cap), np.int32), np.zeros((S, cap, 2), np.float32)
    h.synchronize()
    for dst, src in ((info, d["info"]), (ent, d["entries"]), (xy, d["xy"])):
        assert hip.hipMemcpy(dst.ctypes.data, src, dst.nbytes, 2) == 0   # hipMemcpyDeviceToHost
    return info, ent, xy


def _same(got, want, tag):
    info, ent, xy = got
    winfo, wents, wxys = want
    assert info.tobytes() == winfo.tobytes(), (tag, first_diff(info.view(np.uint32), winfo.view(np.uint32)), info[:4], winfo[:4])
    for s in range(len(winfo)):
        n = int(winfo[s]["n_cells"])
        if ent is not None:
            assert ent[s, :n].tobytes() == wents[s].tobytes(), (tag, s, first_diff(ent[s, :n], wents[s]))
        if xy is not None:
            assert xy[s, :n].tobytes() == wxys[s].tobytes(), (tag, s, first_diff(xy[s, :n].view(np.uint32), wxys[s].view(np.uint32)))


def _walk(gvamd, h, grid, starts, cap, flags, tag, field=None):
    """three calls, each equal to path_ref on the device's own field and to the twin on it; returns path_ref's result"""
    g = nc.grid_of(grid)
    field = h.nav_field_array() if field is None else field
    want = ref.paths(g, field, starts, cap, flags)
    twin = gvamd.nav_path_host(*nc.GRIDS[grid][0], field, starts, cap, flags)
    _same(twin, want, (tag, "twin"))
    for rep in range(3):
        info, xy = h.nav_path(starts, cap, flags)
        assert info.dtype == ref.INFO_DTYPE
        _same((info, None, xy), want, (tag, rep, "returned"))
        _same(_resident(h), want, (tag, rep, "resident"))
    return want


# ------------------------------------------------------------------------------------------------- the nav cases --
@pytest.mark.parametrize("name", list(nc.cases()))
def test_nav_cases(gvamd, name):
    c = nc.cases()[name]
    g = nc.grid_of(c["grid"])
    h = _handle(gvamd, c["grid"])
    cost = plant(h, c["mask"], c["inflation"])
    assert cost.tobytes() == c["cost"].tobytes()          # the host tests walked fields of the same costmap
    for cfg in pc.CONFIGS:
        h.set_nav_config(*cfg)
        h.nav_field(c["goal"])
        field = h.nav_field_array()
        starts = pc.nav_starts(g, field, 100 + len(name))
        for flags in (0, ref.DIAGONAL):
            info = _walk(gvamd, h, c["grid"], starts, pc.NAV_CAP, flags, (name, cfg, flags), field)[0]
            assert (info["status"] == ref.REACHED).all() and (info["end_value"] == 0).all()
            if cfg[1] == 0 and flags == 0:
                assert (info["n_cells"] == info["start_value"].astype(np.int64) + 1).all()
        if name == "serpentine_200x80" and cfg == (253, 0):
            assert int(info[0]["n_cells"]) == 8040
        if name == "comb_250x100" and cfg == (253, 0):
            assert int(info[0]["n_cells"]) == 12625


# ------------------------------------------------------------------------------------------------- the empty map --
@pytest.mark.parametrize("goal", ["centre", "nw", "ne", "sw", "se", "w", "e", "n", "s"])
def test_empty_map(gvamd, goal):
    """250 x 100: the corners, the borders and one cell inside each (windows clipped on one and on two sides), the flush
    boundaries, straight runs over three windows and more in all eight directions, paths along a border for their whole
    length; against the closed forms as well"""
    g = nc.grid_of(pc.EMPTY_GRID)
    h = _handle(gvamd, pc.EMPTY_GRID)
    plant(h, np.zeros((g.ny, g.nx), bool), nc.EXACT)
    gx, gy = pc.empty_goals(g)[goal]
    h.set_nav_config(253, 0)
    h.nav_field(np.array([nc.world_of(g, gx, gy)], np.float32))
    field = h.nav_field_array()
    assert field.tobytes() == pc.empty_field(g, (gx, gy)).tobytes()
    cells, starts = pc.empty_start_cells(g, goal), pc.empty_starts(g, goal)
    for flags in (0, ref.DIAGONAL):
        info = _walk(gvamd, h, pc.EMPTY_GRID, starts, 512, flags, (goal, flags), field)[0]
        for (x, y), r in zip(cells, info):
            dx, dy = abs(x - gx), abs(y - gy)
            want = (max(dx, dy) + 1, min(dx, dy)) if flags else (dx + dy + 1, 0)
            assert (int(r["status"]), int(r["n_cells"]), int(r["n_diagonal"])) == (ref.REACHED,) + want, (goal, flags, x, y)


def test_start_counts(gvamd):
    """S = 1, 2 and 256, duplicate starts, and S * cap exactly 2^20"""
    name = "random_5e-4"
    c = nc.cases()[name]
    g = nc.grid_of(c["grid"])
    h = _handle(gvamd, c["grid"])
    plant(h, c["mask"], c["inflation"])
    h.set_nav_config(253, 3)
    h.nav_field(c["goal"])
    field = h.nav_field_array()
    reach = np.flatnonzero(field < ref.UNREACHABLE)
    pick = np.random.default_rng(8).choice(reach, 200, replace=False)
    many = np.array([nc.world_of(g, int(e) % g.nx, int(e) // g.nx) for e in pick], np.float32)
    many = np.concatenate([many, many[:50], many[:6]])            # 256 starts, 56 of them duplicates
    assert len(many) == 256
    for S, cap, flags in ((1, 1024, 0), (2, 1024, ref.DIAGONAL), (256, 1024, 0), (256, 4096, ref.DIAGONAL)):
        info = _walk(gvamd, h, c["grid"], many[:S], cap, flags, ("count", S, cap), field)[0]
        assert (info["status"] == ref.REACHED).all()
    assert 256 * 4096 == ref.MAX_CELLS
    assert info[:50].tobytes() == info[200:250].tobytes()


def test_starts_that_walk_nowhere_write_nothing(gvamd):
    """starts off the map, non-finite, on blocked and on unreachable cells between good ones: their records, and not a
    byte of the entries and centres beyond what the good ones wrote"""
    c = nc.cases()["pocket_outside"]
    g = nc.grid_of(c["grid"])
    h = _handle(gvamd, c["grid"])
    plant(h, c["mask"], c["inflation"])
    h.set_nav_config(253, 0)
    h.nav_field(c["goal"])
    field = h.nav_field_array()
    w = lambda x, y: nc.world_of(g, x, y)   # noqa: E731
    x_hi = g.pos_x + g.off_x
    starts = np.array([w(200, 80), (x_hi + 0.5, 0.0), w(40, 30), w(65, 45), (np.nan, 0.0), w(5, 95), (0.0, np.inf), w(90, 60), (1e6, 1e6),
                       w(249, 0), w(50, 50)], np.float32)
    cap = 700
    want = ref.paths(g, field, starts, cap, 0)
    assert want[0]["status"].tolist() == [ref.REACHED, ref.OFF_MAP, ref.BLOCKED_START, ref.UNREACHABLE_START, ref.OFF_MAP, ref.REACHED,
                                          ref.OFF_MAP, ref.BLOCKED_START, ref.OFF_MAP, ref.REACHED, ref.UNREACHABLE_START]
    _walk(gvamd, h, c["grid"], starts, cap, 0, "mixed", field)
    # the same call again over resident buffers filled with a pattern, and into a pinned destination filled with another
    hip = hip_runtime()
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    d = h.device_nav_path()
    S = len(starts)
    assert (d["S"], d["cap"]) == (S, cap)
    h.synchronize()
    assert hip.hipMemset(d["entries"], 0x5A, S * cap * 4) == 0 and hip.hipMemset(d["xy"], 0x5A, S * cap * 8) == 0
    pin_info, pin_xy = gvamd.PinnedI8(S * 32), gvamd.PinnedF32(S * cap * 2)
    try:
        pin_xy.array[:] = -7.0
        info = pin_info.array.view(ref.INFO_DTYPE)
        h.nav_path_async(starts, cap, info, pin_xy.array)
        h.synchronize()
        assert h.device_nav_path() == d                           # the same buffers
        got = _resident(h)
        _same(got, want, "mixed, pattern")
        _same((info, None, pin_xy.array.reshape(S, cap, 2)), want, "mixed, pinned")
        for s in range(S):
            n = int(want[0][s]["n_cells"])
            assert (got[1][s, n:] == 0x5A5A5A5A).all() and (got[2][s, n:].view(np.uint32) == 0x5A5A5A5A).all(), s
            assert (pin_xy.array.reshape(S, cap, 2)[s, n:] == -7.0).all(), s
    finally:
        pin_info.close()
        pin_xy.close()


def test_truncation(gvamd):
    c = nc.cases()["in_tile_200x200"]
    g = nc.grid_of(c["grid"])
    h = _handle(gvamd, c["grid"])
    plant(h, c["mask"], c["inflation"])
    h.set_nav_config(253, 0)
    h.nav_field(c["goal"])
    field = h.nav_field_array()
    starts = pc.nav_starts(g, field, 4)[:2]
    n = int(ref.paths(g, field, starts[:1], 4096)[0][0]["n_cells"])
    assert n == 1830
    for cap, status in ((n - 1, ref.TRUNCATED), (n, ref.REACHED), (n + 1, ref.REACHED), (1, ref.TRUNCATED), (64, ref.TRUNCATED),
                        (65, ref.TRUNCATED)):
        info = _walk(gvamd, h, c["grid"], starts, cap, 0, ("cap", cap), field)[0]
        assert (int(info[0]["status"]), int(info[0]["n_cells"])) == (status, min(cap, n)), cap


def test_destinations(gvamd):
    """info and paths_xy into pageable and pinned memory (aligned, and pinned but not aligned: the copy command), and
    paths_xy NULL followed by gv_get_nav_path"""
    c = nc.cases()["random_2e-3"]
    g = nc.grid_of(c["grid"])
    h = _handle(gvamd, c["grid"])
    plant(h, c["mask"], c["inflation"])
    h.set_nav_config(253, 3)
    h.nav_field(c["goal"])
    field = h.nav_field_array()
    starts = pc.nav_starts(g, field, 6)
    S, cap = len(starts), 600
    want = ref.paths(g, field, starts, cap, ref.DIAGONAL)
    pin_i, pin_x = gvamd.PinnedI8(S * 32 + 16), gvamd.PinnedF32(S * cap * 2 + 4)
    try:
        for rep in range(3):
            for i_off, x_off in ((0, 0), (4, 1), (0, 1), (4, 0)):
                pin_i.array[:] = 77
                pin_x.array[:] = -7.0
                info = pin_i.array[i_off:i_off + S * 32].view(ref.INFO_DTYPE)
                xy = pin_x.array[x_off:x_off + S * cap * 2]
                h.nav_path_async(starts, cap, info, xy, ref.DIAGONAL)
                h.synchronize()
                _same((info, None, xy.reshape(S, cap, 2)), want, ("pinned", rep, i_off, x_off))
                assert (pin_i.array[i_off + S * 32:] == 77).all() and (pin_x.array[x_off + S * cap * 2:] == -7.0).all()
            info, xy = np.zeros(S, ref.INFO_DTYPE), np.zeros(S * cap * 2, np.float32)
            h.nav_path_async(starts, cap, info, xy, ref.DIAGONAL)
            h.synchronize()
            _same((info, None, xy.reshape(S, cap, 2)), want, ("pageable", rep))
            info, none = h.nav_path(starts, cap, ref.DIAGONAL, keep_xy=False)
            assert none is None and info.tobytes() == want[0].tobytes()
            for s in range(S):
                n = int(want[0][s]["n_cells"])
                rec, ent, xy_s = h.nav_path_get(s)
                assert rec.tobytes() == want[0][s].tobytes() and ent.tobytes() == want[1][s].tobytes() and xy_s.tobytes() == want[2][s].tobytes()
                rec, ent, xy_s = h.nav_path_get(s, cap_out=5)
                assert rec.tobytes() == want[0][s].tobytes() and ent.tobytes() == want[1][s][:5].tobytes() and len(xy_s) == min(n, 5)
    finally:
        pin_i.close()
        pin_x.close()


def test_2000x2000_wall_with_one_gap(gvamd):
    """the one call at that size: the wall of test_gpu_nav.py over every row of column 1200 but one, the start in the far
    corner; the path goes through the gap and is start_value + 1 cells long"""
    h = gvamd.GridVisionHIP(200, 200, 0.1)
    try:
        nx, ny = h.nx, h.ny
        assert (nx, ny) == (2000, 2000)
        g = ref.grid(200, 200, 0.1)
        xw, yg, sx, sy = 1200, 1700, 300, 250
        mask = np.zeros((ny, nx), bool)
        mask[:, xw] = True
        mask[yg, xw] = False
        plant(h, mask, nc.EXACT)
        h.set_nav_config(253, 0)
        h.nav_field(np.array([nc.world_of(g, sx, sy)], np.float32))
        field = h.nav_field_array()
        start = np.array([nc.world_of(g, nx - 1, 0)], np.float32)
        for flags in (0, ref.DIAGONAL):
            want = ref.paths(g, field, start, 8192, flags)
            for rep in range(3):
                info, xy = h.nav_path(start, 8192, flags)
                _same((info, None, xy), want, ("2000", flags, rep))
                _same(_resident(h), want, ("2000", flags, rep, "resident"))
            assert int(info[0]["status"]) == ref.REACHED and yg * nx + xw in want[1][0].tolist()
            if flags == 0:
                assert int(info[0]["n_cells"]) == int(info[0]["start_value"]) + 1 == (nx - 1 - xw) + yg + (xw - sx) + (yg - sy) + 1
    finally:
        h.close()


# ----------------------------------------------------------------------------------------- the field from a path --
def _field_from_path(h, s, tag):
    """gv_nav_field_from_path(s) against gv_nav_field over the read-back centres of path s; the resident paths survive.
    Returns (field, n_seeds_used)."""
    before = _resident(h)
    rec, _, xy = h.nav_path_get(s)
    a = h.nav_field_from_path(s)
    fa = h.nav_field_array()
    after = _resident(h)
    assert h.nav_path_get(s)[0].tobytes() == rec.tobytes()
    n = int(rec["n_cells"])
    b = h.nav_field(xy if n else np.array([(1e6, 0.0)], np.float32))
    fb = h.nav_field_array()
    assert fa.tobytes() == fb.tobytes(), (tag, first_diff(fa, fb))
    assert a["n_seeds_used"] == b["n_seeds_used"], (tag, a, b)
    assert before[0].tobytes() == after[0].tobytes()
    for k in range(len(before[0])):
        m = int(before[0][k]["n_cells"])
        assert before[1][k, :m].tobytes() == after[1][k, :m].tobytes() and before[2][k, :m].tobytes() == after[2][k, :m].tobytes()
    assert _resident(h)[0].tobytes() == before[0].tobytes()       # ... and gv_nav_field leaves them alone too
    return fa, a["n_seeds_used"]


@pytest.mark.parametrize("name,cfg", [("serpentine_200x80", (253, 0)), ("random_5e-4", (253, 3))])
def test_field_from_path(gvamd, name, cfg):
    c = nc.cases()[name]
    g = nc.grid_of(c["grid"])
    h = _handle(gvamd, c["grid"])
    plant(h, c["mask"], c["inflation"])
    h.set_nav_config(*cfg)
    h.nav_field(c["goal"])
    goal_field = h.nav_field_array()
    starts = np.concatenate([pc.nav_starts(g, goal_field, 9)[:3], np.array([(1e6, 0.0)], np.float32)])
    for rep in range(3):
        h.nav_field(c["goal"])
        info, _ = h.nav_path(starts, pc.NAV_CAP, ref.DIAGONAL, keep_xy=False)
        assert info["status"].tolist() == [ref.REACHED] * 3 + [ref.OFF_MAP]
        fields = []
        for s in range(4):
            f, used = _field_from_path(h, s, (name, rep, s))
            assert used == int(info[s]["n_cells"])
            fields.append(f)
        # n_cells == 0 is "no usable seed": nothing is 0, nothing is reached
        assert not (fields[3] == 0).any() and (fields[3] >= ref.UNREACHABLE).all()
        assert int((fields[0] == 0).sum()) == int(info[0]["n_cells"])


def test_field_from_path_skips_cells_blocked_since(gvamd):
    """a wall planted across the resident path and a new gv_inflate: the path's cells inside the wall are skipped as
    gv_nav_field skips such seeds, and both sides agree again"""
    g = nc.grid_of(pc.EMPTY_GRID)
    h = _handle(gvamd, pc.EMPTY_GRID)
    plant(h, np.zeros((g.ny, g.nx), bool), nc.EXACT)
    h.set_nav_config(253, 0)
    h.nav_field(np.array([nc.world_of(g, 125, 50)], np.float32))
    info, _ = h.nav_path(np.array([nc.world_of(g, 3, 4), nc.world_of(g, 240, 90)], np.float32), 512, 0, keep_xy=False)
    n0, n1 = int(info[0]["n_cells"]), int(info[1]["n_cells"])
    assert (n0, n1) == (122 + 46 + 1, 115 + 40 + 1)
    _, used = _field_from_path(h, 0, "open")
    assert used == n0
    wall = np.zeros((g.ny, g.nx), bool)
    wall[:, 60:63] = True          # path 0 runs along row 4 from x = 3 to 125: three of its cells are in the wall
    wall[50:, 200] = True          # path 1 runs along row 90 from x = 240 down to 125: one cell
    plant(h, wall, nc.EXACT)
    f0, used0 = _field_from_path(h, 0, "wall 0")
    f1, used1 = _field_from_path(h, 1, "wall 1")
    assert (used0, used1) == (n0 - 3, n1 - 1)
    assert int((f0 == 0).sum()) == n0 - 3 and int((f1 == 0).sum()) == n1 - 1


# ------------------------------------------------------------------------------------------- ordering and state --
def _code(gvamd, call):
    with pytest.raises(gvamd.GVError) as e:
        call()
    return e.value.code


def test_ordering_state_and_arguments(gvamd):
    c = nc.cases()["pocket_outside"]
    g = nc.grid_of(c["grid"])
    (gx, gy, res), _ = nc.GRIDS[c["grid"]]
    h = gvamd.GridVisionHIP(gx, gy, res)
    lib = gvamd.load()
    try:
        starts = np.array([nc.world_of(g, 200, 80), nc.world_of(g, 3, 3)], np.float32)
        path = lambda: h.nav_path(starts, 512)   # noqa: E731
        # before the first field: no path call, no resident path
        assert _code(gvamd, path) == GV_ERR_STATE
        plant(h, c["mask"], c["inflation"])
        h.set_nav_config(253, 0)
        assert _code(gvamd, path) == GV_ERR_STATE
        for call in (h.device_nav_path, lambda: h.nav_path_get(0), lambda: h.nav_field_from_path(0)):
            assert _code(gvamd, call) == GV_ERR_STATE
        # a 1-rank communicator changes nothing
        h.comm_init(gvamd.GridVisionHIP.comm_unique_id(), 0, 1)
        h.nav_field(c["goal"])
        first = _walk(gvamd, h, c["grid"], starts, 512, 0, "first field")
        # a path call behind a second gv_nav_field sees the new field
        h.nav_field(np.array([nc.world_of(g, 240, 5)], np.float32))
        second = _walk(gvamd, h, c["grid"], starts, 512, 0, "second field")
        assert first[0].tobytes() != second[0].tobytes() and int(second[0][0]["end_entry"]) == 5 * g.nx + 240
        # arguments: state unchanged
        before = _resident(h)
        info = np.zeros(257, ref.INFO_DTYPE)
        many = np.zeros((257, 2), np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731

        def raw(S=2, cap=512, flags=0, st=many, inf=info, fn=lib.gv_nav_path):
            return fn(h._h, p(st), C.c_int32(S), C.c_int32(cap), C.c_uint32(flags), p(inf), None)

        for fn in (lib.gv_nav_path, lib.gv_nav_path_async):
            for kw in (dict(S=0), dict(S=257), dict(cap=0), dict(cap=65537), dict(S=17, cap=65536), dict(flags=2), dict(st=None),
                       dict(inf=None)):
                assert raw(fn=fn, **kw) == GV_ERR_BAD_ARG, kw
        assert lib.gv_nav_path(None, p(many), C.c_int32(1), C.c_int32(1), C.c_uint32(0), p(info), None) == GV_ERR_BAD_ARG
        assert _code(gvamd, lambda: h.nav_path_get(2)) == GV_ERR_BAD_ARG and _code(gvamd, lambda: h.nav_path_get(-1)) == GV_ERR_BAD_ARG
        assert _code(gvamd, lambda: h.nav_field_from_path(2)) == GV_ERR_BAD_ARG
        assert _code(gvamd, lambda: h.nav_field_from_path(-1)) == GV_ERR_BAD_ARG
        after = _resident(h)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
        # no configuration: the field from a path is refused, the path call (which reads the field alone) is not
        h.set_nav_config(None)
        assert _code(gvamd, lambda: h.nav_field_from_path(0)) == GV_ERR_STATE
        _walk(gvamd, h, c["grid"], starts, 512, ref.DIAGONAL, "no configuration")
        h.set_nav_config(253, 0)
        # gv_reset invalidates the field and the resident paths
        h.reset()
        for call in (path, h.device_nav_path, lambda: h.nav_path_get(0), lambda: h.nav_field_from_path(0)):
            assert _code(gvamd, call) == GV_ERR_STATE
        plant(h, c["mask"], c["inflation"])
        assert _code(gvamd, lambda: h.nav_field_from_path(0)) == GV_ERR_STATE      # a costmap, still no resident path
        h.nav_field(c["goal"])
        assert _code(gvamd, h.device_nav_path) == GV_ERR_STATE                     # a field, still no resident path
        again = _walk(gvamd, h, c["grid"], starts, 512, 0, "after reset")
        assert again[0].tobytes() == first[0].tobytes()
    finally:
        h.close()


def test_path_during_a_pending_tick(gvamd):
    """tick_enqueue, inflate, nav_field, nav_path_async, tick_wait: the path is that of the tick's grid, as a twin handle
    walks it after its tick"""
    from gvamd import synth
    from test_gpu_parity import _ground_scene, make_handle
    P5 = (0.5, 1.1, 5.0, 80)
    hA, tfs = make_handle(gvamd, 2, perturbed=True)
    hB, _ = make_handle(gvamd, 2, perturbed=True)
    x, y, z, _, b = _ground_scene(tfs, seed=9)
    seeds = np.array([(40.0, 0.0)], np.float32)
    starts = np.array([(0.0, 0.0), (10.0, 30.0), (-20.0, -15.0), (1e6, 0.0)], np.float32)
    cap = 2048
    gc = synth.CONFIGS[2]["grid"]
    g = ref.grid(gc.grid_x, gc.grid_y, gc.resolution)
    assert (g.nx, g.ny) == (hA.nx, hA.ny)
    pin = gvamd.PinnedI8(4 * 32)
    try:
        for h in (hA, hB):
            h.upload_xyz(x, y, z)
            h.tick(b, k_near=4, lidar_bin=True)
            h.set_inflation(*P5)
            h.set_nav_config(253, 2)
        hA.tick_enqueue(b, k_near=4, lidar_bin=True)
        hA.inflate()
        hA.nav_field(seeds)
        info = pin.array.view(ref.INFO_DTYPE)
        hA.nav_path_async(starts, cap, info, None, ref.DIAGONAL)
        hA.tick_wait()
        hA.synchronize()
        got = _resident(hA)
        assert got[0].tobytes() == info.tobytes()
        hB.tick(b, k_near=4, lidar_bin=True)
        hB.inflate()
        hB.nav_field(seeds)
        field = hB.nav_field_array()
        _same(got, ref.paths(g, field, starts, cap, ref.DIAGONAL), "pending tick")
        assert (info["status"][:3] != ref.OFF_MAP).all() and int(info["status"][3]) == ref.OFF_MAP
    finally:
        pin.close()
        hA.close(); hB.close()


def test_path_demo(gvamd, tmp_path):
    """examples/path_demo.cpp (plain g++ over the two C headers): the path from the vehicle through the gap, the field
    seeded by it on the device, the fan of arcs scored against that field; the arc that follows the path wins and the
    demo's own host replay of the walk finds no mismatch"""
    pkg = os.path.join(os.path.dirname(HERE), "grid-vision_amd")
    exe = str(tmp_path / "path_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(pkg, "examples", "path_demo.cpp"), "-o", exe,
                           "-L" + pkg, "-lgridvision_hip", "-Wl,-rpath," + pkg])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    m = re.search(r"path cells (\d+) diagonal (\d+) status 0 length ([\d.]+) m through_gap yes\n"
                  r"path field seeds (\d+) rounds (\d+)\n"
                  r"best (\d+) curvature (-?[\d.]+) path_dist_sum (\d+) mirrored (\d+) straight (\d+) follows_path yes\n"
                  r"host check ok \(0 mismatches\)", out.stdout)
    assert m, out.stdout
    cells, diag, length, seeds, rounds, best, curv, dist, mirrored, straight = (float(v) for v in m.groups())
    assert cells == seeds > 220 and 0 < diag < cells and length > 22.0 and rounds >= 1
    assert best != 20 and curv > 0 and dist < mirrored
