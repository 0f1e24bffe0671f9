"""[EXTENSION] X19 frontier clusters on the device: gvx_frontier against frontier_ref (a plain Python flood) and against the
host twin, both run on the device's own read-back of the packed layer, costmap and field, with zero tolerance: every
comparison is tobytes() equality of the info record, of all `cap` records and of the G labels.  Every case is planted
through gv_set_log_odds + gv_update_map (the log-odds clamp to [-2, 3.6], so any packed value in 11..97 is reachable; 0.0
gives 50, NaN gives -1), every call is made twice and gives the same bytes.  Then the destinations, gv_grid_move, a
pending tick, gv_reset, the errors and gvx_nav_field_from_frontier against gv_nav_field over the same cells' centres."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frontier_cases as fc
import frontier_ref as ref
import nav_cases as nc
from planner_util import first_diff, hip_runtime

pytestmark = pytest.mark.gpu

GV_ERR_BAD_ARG, GV_ERR_STATE = 1, 5
INFLATION = (0.35, 0.55, 10.0, 65)
_HANDLES = {}


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
        (gx, gy, res), (nx, ny) = fc.GRIDS[grid]
        h = gvamd.GridVisionHIP(gx, gy, res)
        assert (h.nx, h.ny) == (nx, ny)
        _HANDLES[grid] = h
    h = _HANDLES[grid]
    h.reset()
    return h


def plant_occ(h, occ):
    """the packed layer occ (data order) through the log-odds layer; returns the int8 read-back, which equals it"""
    v = np.asarray(occ, np.int8).reshape(-1).astype(np.float64)
    p = (v + 0.5) / 100.0
    with np.errstate(invalid="ignore", divide="ignore"):
        lo = np.where(v < 0, np.nan, np.where(v == 50, 0.0, np.log(p / (1.0 - p))))
    lo = lo.astype(np.float32) + np.float32(0.2)         # the update adds the decay of -0.2 before it clamps
    h.set_log_odds(lo[::-1])                             # cell = G - 1 - entry
    h.update_map()
    i8 = h.to_occupancy_grid()[0]
    assert i8.tobytes() == np.asarray(occ, np.int8).tobytes(), first_diff(i8, occ)
    return i8


def _resident(h, cap):
    hip = hip_runtime()
    d = h.device_frontier()
    assert d["cap"] == cap
    info, recs, labels = np.zeros(1, ref.INFO_DTYPE), np.zeros(cap, ref.RECORD_DTYPE), np.zeros(h.G, np.uint32)
    h.synchronize()
    for dst, src in ((info, d["info"]), (recs, d["records"]), (labels, d["labels"])):
        assert hip.hipMemcpy(dst.ctypes.data, src, dst.nbytes, 2) == 0   # hipMemcpyDeviceToHost
    return info[0], recs, labels


def _same(got, want, tag):
    for k, name in enumerate(("info", "records", "labels")):
        if got[k] is not None:
            a, b = np.atleast_1d(got[k]), np.atleast_1d(want[k])
            assert a.tobytes() == b.tobytes(), (tag, name, first_diff(a.view(np.uint32), b.view(np.uint32)), got[0], want[0])


def _frontier(gvamd, h, grid, cfg, cap, flags, tag, i8=None, reps=2):
    """`reps` calls, each equal to frontier_ref and to the twin on the device's own layers; returns frontier_ref's result"""
    g = fc.grid_of(grid)
    i8 = h.to_occupancy_grid()[0] if i8 is None else i8
    cost = h.costmap() if cfg["max_cost"] < 256 else None
    field = h.nav_field_array() if flags & ref.USE_FIELD else None
    want = ref.frontier(g, i8, cfg, cap, flags, cost, field)
    c = gvamd.FrontierConfig.of(**cfg)
    _same(gvamd.frontier_host(*fc.GRIDS[grid][0], i8, c, cap, flags, cost, field), want, (tag, "twin"))
    h.set_frontier_config(c)
    for rep in range(reps):
        info, recs = h.frontier(cap, flags)
        assert info.dtype == ref.INFO_DTYPE and recs.dtype == ref.RECORD_DTYPE
        _same((info, recs, h.frontier_labels()), want, (tag, rep, "returned"))
        _same(_resident(h, cap), want, (tag, rep, "resident"))
    return want


# ---------------------------------------------------------------------------------------------------- the cases --
@pytest.mark.parametrize("name", list(fc.cases()))
def test_cases(gvamd, name):
    c = fc.cases()[name]
    h = _handle(gvamd, c["grid"])
    i8 = plant_occ(h, c["occ"])
    if c["cfg"]["max_cost"] < 256:
        h.set_inflation(*INFLATION)
        h.inflate()
    for k, cap in enumerate(c["caps"]):
        want = _frontier(gvamd, h, c["grid"], c["cfg"], cap, 0, (name, cap), i8)
        if k == 0 and c["cost"] is None:
            fc.check(name, c, *want)
        if name == "cap_edges":
            assert int(want[0]["n_written"]) == min(cap, 5) and (np.diff(want[1]["label"][:min(cap, 5)]) > 0).all()
    if name == "class_edges":
        e = c["cfg"]
        vals = set(np.unique(i8).tolist())
        for lo, hi in ((e["free_max"], e["free_max"] + 1), (e["unknown_min"] - 1, e["unknown_min"]), (e["unknown_max"], e["unknown_max"] + 1)):
            assert lo in vals and hi in vals, (lo, hi)       # the read-back lands on both sides of every class edge
        assert -1 in vals
    if name.startswith("cost_gate"):
        n = int(want[0]["n_clusters"])
        assert n == (1 if c["cfg"]["max_cost"] == 256 else 2), n   # the inflated wall removes the middle of the frontier


# ---------------------------------------------------------------------------------------------------- the field --
def _field_map():
    """200 x 80, free everywhere but: two unknown strips of one size along the top border (a tie of the largest cluster),
    an unknown blob inside a closed box of walls (a cluster no field reaches), an unknown strip under a wall (cells the
    inflation blocks), two unknown cells at one distance from a seed (a tie of field_min)"""
    occ = np.full((80, 200), fc.FREE, np.int8)
    occ[0:4, 20:90] = fc.UNKNOWN
    occ[0:4, 100:170] = fc.UNKNOWN
    occ[30:51, 100:131] = fc.OCC
    occ[33:48, 103:128] = fc.FREE
    occ[38:43, 112:119] = fc.UNKNOWN
    occ[57, 150:171] = fc.OCC
    occ[60:65, 150:171] = fc.UNKNOWN
    occ[70, 30] = occ[70, 50] = fc.UNKNOWN
    seeds = [(40, 20), (70, 20), (40, 70)]
    return occ, seeds


def test_field_and_best(gvamd):
    grid = "200x80"
    g = fc.grid_of(grid)
    h = _handle(gvamd, grid)
    occ, seeds = _field_map()
    i8 = plant_occ(h, occ)
    h.set_inflation(*INFLATION)
    h.inflate()
    h.set_nav_config(253, 0)
    h.nav_field(np.array([nc.world_of(g, x, y) for x, y in seeds], np.float32))
    field = h.nav_field_array()
    cfg = ref.config()
    for cap in (16, 2):
        info, recs, labels = _frontier(gvamd, h, grid, cfg, cap, ref.USE_FIELD, ("field", cap), i8)
        plain = _frontier(gvamd, h, grid, cfg, cap, 0, ("no field", cap), i8)
        assert (plain[1]["field_entry"][:int(plain[0]["n_written"])] == -1).all()
        assert (plain[1]["goal_entry"] == plain[1]["centre_entry"]).all()
    n = int(info["n_written"])
    assert n == 2 and int(info["n_clusters"]) == 6
    info, recs, labels = _frontier(gvamd, h, grid, cfg, 16, ref.USE_FIELD, "field", i8, reps=1)
    r = recs[:int(info["n_written"])]
    # a cluster no field reaches: the goal falls back to the centre
    lost = np.flatnonzero(r["field_entry"] < 0)
    assert len(lost) == 1 and (r["goal_entry"][lost] == r["centre_entry"][lost]).all() and (r["field_min"][lost] == ref.UNREACHABLE).all()
    # a cluster with blocked cells that is reached all the same
    blocked = [k for k in range(len(r)) if (field[labels == np.uint32(r["label"][k])] == fc.BLOCKED).any() and r["field_entry"][k] >= 0]
    assert blocked
    # a tie inside a cluster goes to the smaller entry
    tied = [k for k in range(len(r)) if r["field_entry"][k] >= 0 and (field[labels == np.uint32(r["label"][k])] == r["field_min"][k]).sum() > 1]
    assert tied and all(int(r["field_entry"][k]) == int(np.flatnonzero((labels == np.uint32(r["label"][k])) & (field == r["field_min"][k]))[0])
                        for k in tied)
    # best under both rules, each with a tie that goes to the smaller index
    fm = r["field_min"].astype(np.int64)
    assert (fm == fm.min()).sum() >= 2 and int(info["best"]) == int(np.flatnonzero(fm == fm.min())[0])
    plain = _frontier(gvamd, h, grid, cfg, 16, 0, "no field", i8, reps=1)
    nc_ = plain[1]["n_cells"][:int(plain[0]["n_written"])]
    assert (nc_ == nc_.max()).sum() >= 2 and int(plain[0]["best"]) == int(np.argmax(nc_))


# -------------------------------------------------------------------------------------------- the destinations --
def test_destinations(gvamd):
    """info and out into pageable memory, into pinned 16-byte aligned memory (written by the kernel) and into pinned
    memory that is not aligned (the copy command); nothing is written past either"""
    name = "border_runs"
    c = fc.cases()[name]
    h = _handle(gvamd, c["grid"])
    i8 = plant_occ(h, c["occ"])
    cap = 6
    want = _frontier(gvamd, h, c["grid"], c["cfg"], cap, 0, name, i8, reps=1)
    pin_i, pin_r = gvamd.PinnedI8(32 + 32), gvamd.PinnedI8(cap * 64 + 32)
    try:
        for rep in range(2):
            for off in (0, 16, 4):
                pin_i.array[:] = 77
                pin_r.array[:] = 77
                info = pin_i.array[off:off + 32].view(ref.INFO_DTYPE)
                out = pin_r.array[off:off + cap * 64].view(ref.RECORD_DTYPE)
                h.frontier_async(cap, info, out)
                h.synchronize()
                _same((info[0], out, None), want, ("pinned", rep, off))
                assert (pin_i.array[off + 32:] == 77).all() and (pin_r.array[off + cap * 64:] == 77).all()
                assert (pin_i.array[:off] == 77).all() and (pin_r.array[:off] == 77).all()
            info, out = np.zeros(1, ref.INFO_DTYPE), np.zeros(cap, ref.RECORD_DTYPE)
            h.frontier_async(cap, info, out)
            h.synchronize()
            _same((info[0], out, None), want, ("pageable", rep))
    finally:
        pin_i.close()
        pin_r.close()


# ------------------------------------------------------------------------------------- gv_grid_move, gv_reset --
def test_after_grid_move(gvamd):
    """an all-free map scrolls: the border that scrolls in holds the prior (50), and the frontier runs along it"""
    grid = "200x80"
    h = _handle(gvamd, grid)
    plant_occ(h, np.full((80, 200), fc.FREE, np.int8))
    cfg = ref.config()
    assert int(_frontier(gvamd, h, grid, cfg, 8, 0, "before", reps=1)[0]["n_frontier_cells"]) == 0
    assert h.grid_move((0.0, 0.0, 0.0, 1.0, 1.2, -0.5, 0.0))["applied"]
    i8 = h.to_occupancy_grid()[0]
    assert 0 < (i8 == 50).sum() < 200 * 80 // 2 and ((i8 == 50) | (i8 == fc.FREE)).all()
    info = _frontier(gvamd, h, grid, cfg, 8, 0, "moved", i8)[0]
    assert int(info["n_frontier_cells"]) > 200 and int(info["n_clusters"]) == 1    # one L along the two borders
    h.set_frontier_config(None)
    h.set_frontier_config(gvamd.FrontierConfig.of(**cfg))


def _code(gvamd, call):
    with pytest.raises(gvamd.GVError) as e:
        call()
    return e.value.code


def test_state_and_arguments(gvamd):
    c = fc.cases()["cost_gate_1"]
    (gx, gy, res), _ = fc.GRIDS[c["grid"]]
    h = gvamd.GridVisionHIP(gx, gy, res)
    lib = gvamd.load()
    try:
        call = lambda flags=0: h.frontier(8, flags)   # noqa: E731
        # no configuration; then a configuration that needs a costmap, a call that needs a field
        assert _code(gvamd, call) == GV_ERR_STATE
        for get in (h.frontier_labels, h.device_frontier, lambda: h.nav_field_from_frontier(-1)):
            assert _code(gvamd, get) == GV_ERR_STATE
        i8 = plant_occ(h, c["occ"])
        h.set_frontier_config(gvamd.FrontierConfig.of(**c["cfg"]))
        assert _code(gvamd, call) == GV_ERR_STATE                         # max_cost < 256 and no costmap
        h.set_frontier_config(gvamd.FrontierConfig.of(**ref.config()))
        assert _code(gvamd, lambda: call(ref.USE_FIELD)) == GV_ERR_STATE  # no field
        first = _frontier(gvamd, h, c["grid"], ref.config(), 8, 0, "first", i8)
        assert _code(gvamd, lambda: h.nav_field_from_frontier(-1)) == GV_ERR_STATE   # a frontier, no nav configuration
        # rejected configurations leave the one in force alone
        for bad in (dict(free_max=-1), dict(free_max=101), dict(free_max=40), dict(unknown_min=61), dict(unknown_max=101),
                    dict(max_cost=0), dict(max_cost=257), dict(min_cells=0), dict(min_cells=(1 << 20) + 1), dict(flags=1)):
            assert _code(gvamd, lambda: h.set_frontier_config(gvamd.FrontierConfig.of(**{**ref.config(), **bad}))) == GV_ERR_BAD_ARG, bad
        r = gvamd.FrontierConfig.of(**ref.config())
        r.reserved[1] = 1
        assert _code(gvamd, lambda: h.set_frontier_config(r)) == GV_ERR_BAD_ARG
        # arguments: state unchanged
        before = _resident(h, 8)
        info, out = np.zeros(1, ref.INFO_DTYPE), np.zeros(4097, ref.RECORD_DTYPE)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
        for fn in (lib.gvx_frontier, lib.gvx_frontier_async):
            for cap, flags, i, o in ((0, 0, info, out), (4097, 0, info, out), (-1, 0, info, out), (8, 2, info, out), (8, 0, None, out),
                                     (8, 0, info, None)):
                assert fn(h._h, C.c_int32(cap), C.c_uint32(flags), p(i), p(o)) == GV_ERR_BAD_ARG, (cap, flags)
            assert fn(None, C.c_int32(8), C.c_uint32(0), p(info), p(out)) == GV_ERR_BAD_ARG
        assert lib.gvx_get_frontier_labels(h._h, None) == GV_ERR_BAD_ARG
        h.set_nav_config(253, 0)
        h.set_inflation(*INFLATION)
        h.inflate()
        for k in (-2, 8, 4096):
            assert _code(gvamd, lambda: h.nav_field_from_frontier(k)) == GV_ERR_BAD_ARG, k
        _same(_resident(h, 8), before, "after the refused calls")
        _same(_frontier(gvamd, h, c["grid"], ref.config(), 8, 0, "again", i8, reps=1), first, "again")
        # gv_reset invalidates the resident result and keeps the configuration
        h.reset()
        for get in (h.frontier_labels, h.device_frontier, lambda: h.nav_field_from_frontier(-1)):
            assert _code(gvamd, get) == GV_ERR_STATE
        info, _ = h.frontier(8)
        assert int(info["n_frontier_cells"]) == 0 and int(info["best"]) == -1   # the prior is unknown everywhere
        h.set_frontier_config(None)
        assert _code(gvamd, call) == GV_ERR_STATE
    finally:
        h.close()


# ------------------------------------------------------------------------------------------- a pending tick --
def test_frontier_during_a_pending_tick(gvamd):
    """tick_enqueue, frontier_async, tick_wait: the clusters are those of the tick's grid, as a twin handle finds them
    after its tick"""
    from gvamd import synth
    from test_gpu_parity import _ground_scene, make_handle
    hA, tfs = make_handle(gvamd, 2, perturbed=True)
    hB, _ = make_handle(gvamd, 2, perturbed=True)
    x, y, z, _, b = _ground_scene(tfs, seed=9)
    gc = synth.CONFIGS[2]["grid"]
    g = ref.grid(gc.grid_x, gc.grid_y, gc.resolution)
    cap = 256
    pin_i, pin_r = gvamd.PinnedI8(32), gvamd.PinnedI8(cap * 64)
    try:
        # the twin first: after two ticks a never-observed cell holds the prior less two decays, the most frequent value
        # of the layer; that value is UNKNOWN here and everything below it FREE
        hB.upload_xyz(x, y, z)
        hB.tick(b, k_near=4, lidar_bin=True, lidar_raymarch=True)
        hB.tick(b, k_near=4, lidar_bin=True, lidar_raymarch=True)
        i8 = hB.to_occupancy_grid()[0]
        vals, counts = np.unique(i8, return_counts=True)
        u = int(vals[np.argmax(counts)])
        assert 11 < u <= 50 and (i8 < u).any()
        cfg = ref.config(free_max=u - 1, unknown_min=u, unknown_max=u, min_cells=2)
        want = ref.frontier(g, i8, cfg, cap)
        assert int(want[0]["n_frontier_cells"]) > 0 and int(want[0]["n_clusters"]) > 0
        hA.upload_xyz(x, y, z)
        hA.tick(b, k_near=4, lidar_bin=True, lidar_raymarch=True)
        hA.set_frontier_config(gvamd.FrontierConfig.of(**cfg))
        hA.tick_enqueue(b, k_near=4, lidar_bin=True, lidar_raymarch=True)
        info, out = pin_i.array.view(ref.INFO_DTYPE), pin_r.array.view(ref.RECORD_DTYPE)
        hA.frontier_async(cap, info, out)
        hA.tick_wait()
        hA.synchronize()
        _same((info[0], out, hA.frontier_labels()), want, "pending tick")
        _same(_resident(hA, cap), want, "pending tick, resident")
    finally:
        pin_i.close()
        pin_r.close()
        hA.close(); hB.close()


# ----------------------------------------------------------------------------------- the field from a frontier --
@pytest.mark.parametrize("name,cap", [("isolated_dots", 16), ("cost_gate_253", 4), ("blobs_640", 4096)])
def test_nav_field_from_frontier(gvamd, name, cap):
    """k = -1, every written k and k >= n_written against gv_nav_field over the same cells' centres; then gv_nav_path
    from a start ends on a cell of a written cluster"""
    c = fc.cases()[name]
    grid = c["grid"]
    g = fc.grid_of(grid)
    nx = g.nx
    h = _handle(gvamd, grid)
    i8 = plant_occ(h, c["occ"])
    h.set_inflation(*INFLATION)
    h.inflate()
    h.set_nav_config(253, 2)
    info, recs, labels = _frontier(gvamd, h, grid, c["cfg"], cap, 0, name, i8, reps=1)
    n = int(info["n_written"])
    assert n == min(cap, int(info["n_clusters"])) and n >= 2
    for k in sorted(set([-1, 0, n - 1] + ([n, cap - 1] if n < cap else []))):
        want_labels = recs["label"][:n] if k < 0 else recs["label"][k:k + 1] if k < n else recs["label"][:0]
        cells = np.flatnonzero(np.isin(labels, want_labels.astype(np.uint32)))
        assert len(cells) <= 65536
        a = h.nav_field_from_frontier(k)
        fa = h.nav_field_array()
        xy = np.array([nc.world_of(g, int(e) % nx, int(e) // nx) for e in cells], np.float32) if len(cells) else np.array([(1e6, 0.0)], np.float32)
        b = h.nav_field(xy)
        fb = h.nav_field_array()
        assert fa.tobytes() == fb.tobytes(), (name, k, first_diff(fa, fb))
        assert a["n_seeds_used"] == b["n_seeds_used"], (name, k, a, b)
        if k >= n:
            assert a["n_seeds_used"] == 0 and not (fa == 0).any()
        _same(_resident(h, cap), (info, recs, labels), (name, k, "the resident frontier survives"))
    h.nav_field_from_frontier(-1)
    field = h.nav_field_array()
    reach = np.flatnonzero((field > 0) & (field < 2000))
    assert len(reach)
    e = int(reach[len(reach) // 2])
    pinfo, _ = h.nav_path(np.array([nc.world_of(g, e % nx, e // nx)], np.float32), 4096, 0, keep_xy=False)
    assert int(pinfo[0]["status"]) == 0 and int(labels[int(pinfo[0]["end_entry"])]) in recs["label"][:n].tolist()


def test_frontier_demo(gvamd, tmp_path):
    """examples/frontier_demo.cpp (plain g++ over the C headers): the clusters of a seen disc, the field seeded by them on
    the device, the path from the vehicle that ends on a frontier cell, and the demo's own host replay finds no mismatch"""
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "grid-vision_amd")
    exe = str(tmp_path / "frontier_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(pkg, "examples", "frontier_demo.cpp"), "-o", exe,
                           "-L" + pkg, "-lgridvision_hip", "-Wl,-rpath," + pkg])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    m = re.search(r"frontier cells (\d+) components (\d+) clusters (\d+) written (\d+) largest (\d+) best (\d+)\n", out.stdout)
    assert m, out.stdout
    cells, comps, clusters, written, largest, best = (int(v) for v in m.groups())
    assert cells >= largest > 50 and comps >= clusters == written >= 1 and 0 <= best < written
    m = re.search(r"frontier field seeds (\d+) rounds (\d+)\npath cells (\d+) status 0 ends_on_frontier yes\n", out.stdout)
    assert m and 0 < int(m.group(1)) <= cells and int(m.group(3)) > 10, out.stdout
    assert "nearest cluster" in out.stdout and "host check ok (0 mismatches)" in out.stdout, out.stdout
