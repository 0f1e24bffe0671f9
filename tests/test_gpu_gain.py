"""[EXTENSION] X20 information gain on the device: gvx2_gain and gvx2_frontier_gain against gain_ref (a plain Python
reference written from the header) and against the host twin, both run on the device's own read-back of the packed layer
and of the field, with zero tolerance: every comparison is tobytes() equality of the info record and of all records, as
returned and as resident.  Every case is planted through gv_set_log_odds + gv_update_map as X19's are, every call is made
twice and gives the same bytes.  Then the destinations and the two kinds of entries, the frontier form, gv_reset, a
pending tick, gv_grid_move, the errors, and gvx2_nav_field_from_gain against gv_nav_field over the same cell's centre."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frontier_ref
import gain_cases as gc
import gain_ref as ref
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
        (gx, gy, res), (nx, ny) = gc.GRIDS[grid]
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


def make_field(h, grid, seeds):
    """the costmap and X9's field from the seed cells; returns the field's read-back"""
    g = gc.grid_of(grid)
    h.set_inflation(*INFLATION)
    h.inflate()
    h.set_nav_config(253, 0)
    h.nav_field(np.array([nc.world_of(g, x, y) for x, y in seeds], np.float32))
    return h.nav_field_array()


def _resident(h, n):
    hip = hip_runtime()
    d = h.device_gain()
    assert d["n"] == n
    info, recs = np.zeros(1, ref.INFO_DTYPE), np.zeros(n, ref.RECORD_DTYPE)
    h.synchronize()
    for dst, src in ((info, d["info"]), (recs, d["records"])):
        assert hip.hipMemcpy(dst.ctypes.data, src, dst.nbytes, 2) == 0   # hipMemcpyDeviceToHost
    return info[0], recs


def _same(got, want, tag):
    for k, name in enumerate(("info", "records")):
        a, b = np.atleast_1d(got[k]), np.atleast_1d(want[k])
        assert a.tobytes() == b.tobytes(), (tag, name, first_diff(a.view(np.uint32), b.view(np.uint32)), got[0], want[0])


def _gain(gvamd, h, grid, cfg, entries, flags, tag, i8=None, field=None, reps=2):
    """`reps` calls, each equal to gain_ref and to the twin on the device's own layers; returns gain_ref's result"""
    i8 = h.to_occupancy_grid()[0] if i8 is None else i8
    field = h.nav_field_array() if flags & ref.USE_FIELD and field is None else field
    entries = np.asarray(entries).astype(np.int32)
    want = ref.gain(gc.grid_of(grid), i8, cfg, entries, flags, field)
    c = gvamd.GainConfig.of(**cfg)
    _same(gvamd.gain_host(*gc.GRIDS[grid][0], i8, c, entries, flags, field if flags else None), want, (tag, "twin"))
    h.set_gain_config(c)
    for rep in range(reps):
        info, recs = h.gain(entries, flags)
        assert info.dtype == ref.INFO_DTYPE and recs.dtype == ref.RECORD_DTYPE
        _same((info, recs), want, (tag, rep, "returned"))
        _same(_resident(h, len(entries)), want, (tag, rep, "resident"))
    return want


# ---------------------------------------------------------------------------------------------------- the cases --
@pytest.mark.parametrize("name", list(gc.cases()))
def test_cases(gvamd, name):
    c = gc.cases()[name]
    h = _handle(gvamd, c["grid"])
    i8 = plant_occ(h, c["occ"])
    field = make_field(h, c["grid"], c["seeds"]) if c["flags"] else None
    want = _gain(gvamd, h, c["grid"], c["cfg"], c["entries"], c["flags"], name, i8, field)
    gc.check(name, c, *want)                     # with a field: the device's own, not the host tests' synthetic one
    if c["flags"]:
        _gain(gvamd, h, c["grid"], c["cfg"], c["entries"], 0, (name, "no field"), i8, reps=1)


# -------------------------------------------------------------------------------------------- the destinations --
def test_destinations_and_entries(gvamd):
    """info and out into pageable memory, into pinned 16-byte aligned memory (written by the kernel) and into pinned
    memory that is not aligned (the copy command), nothing written past either; entries from the host and from the device"""
    name = "r33"
    c = gc.cases()[name]
    h = _handle(gvamd, c["grid"])
    i8 = plant_occ(h, c["occ"])
    entries = c["entries"].astype(np.int32)
    n = len(entries)
    want = _gain(gvamd, h, c["grid"], c["cfg"], entries, 0, name, i8, reps=1)
    hip = hip_runtime()
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), entries.nbytes) == 0
    pin_i, pin_r = gvamd.PinnedI8(32 + 32), gvamd.PinnedI8(n * 48 + 32)
    try:
        assert hip.hipMemcpy(dev, entries.ctypes.data, entries.nbytes, 1) == 0   # hipMemcpyHostToDevice
        for rep in range(2):
            for off in (0, 16, 4):
                for from_device in (False, True):
                    pin_i.array[:] = 77
                    pin_r.array[:] = 77
                    info = pin_i.array[off:off + 32].view(ref.INFO_DTYPE)
                    out = pin_r.array[off:off + n * 48].view(ref.RECORD_DTYPE)
                    if from_device:
                        h.gain_async(None, info, out, device_ptr=dev.value, n=n)
                    else:
                        scratch = entries.copy()
                        h.gain_async(scratch, info, out)
                        scratch[:] = -7                       # host entries were copied before the call returned
                    h.synchronize()
                    flags = ref.DEVICE_ENTRIES if from_device else 0
                    assert int(info[0]["flags"]) == flags
                    info[0]["flags"] = 0
                    _same((info[0], out), want, ("pinned", rep, off, from_device))
                    assert (pin_i.array[off + 32:] == 77).all() and (pin_r.array[off + n * 48:] == 77).all()
                    assert (pin_i.array[:off] == 77).all() and (pin_r.array[:off] == 77).all()
            info, out = np.zeros(1, ref.INFO_DTYPE), np.zeros(n, ref.RECORD_DTYPE)
            h.gain_async(entries, info, out)
            h.synchronize()
            _same((info[0], out), want, ("pageable", rep))
            info, out = h.gain(None, device_ptr=dev.value, n=n)
            assert int(info["flags"]) == ref.DEVICE_ENTRIES and out.tobytes() == want[1].tobytes()
    finally:
        pin_i.close()
        pin_r.close()
        hip.hipFree(dev)


# ------------------------------------------------------------------------------------------- the frontier form --
def _frontier_map():
    """200 x 80: free ground, an unknown band on the right behind a wall with a doorway, unknown pockets on the left"""
    occ = np.full((80, 200), gc.FREE, np.int8)
    occ[:, 150:] = gc.UNKNOWN
    occ[:, 149] = gc.OCC
    occ[30:34, 149] = gc.FREE
    occ[10:14, 20:26] = gc.UNKNOWN
    occ[60:70, 40:44] = gc.UNKNOWN
    occ[40, 90] = gc.UNKNOWN
    return occ


@pytest.mark.parametrize("use_field", [False, True])
def test_frontier_gain(gvamd, use_field):
    """gvx_frontier_async then gvx2_frontier_gain with no wait in between equals the list call over the records' goal_entry;
    caps above and below n_clusters; zero records behind n_written"""
    grid = "200x80"
    g = gc.grid_of(grid)
    h = _handle(gvamd, grid)
    i8 = plant_occ(h, _frontier_map())
    field = make_field(h, grid, [(100, 40)]) if use_field else None
    fcfg = frontier_ref.config(min_cells=1)
    cfg = ref.config(radius=20, w_gain=4, w_dist=1, min_gain=1)
    h.set_frontier_config(gvamd.FrontierConfig.of(**fcfg))
    h.set_gain_config(gvamd.GainConfig.of(**cfg))
    fflags = frontier_ref.USE_FIELD if use_field else 0
    flags = ref.USE_FIELD if use_field else 0
    n_clusters = int(frontier_ref.frontier(g, i8, fcfg, 64, fflags, None, field)[0]["n_clusters"])
    assert n_clusters == 4
    for cap in (64, n_clusters, 2, 1):
        finfo, frecs, _ = frontier_ref.frontier(g, i8, fcfg, cap, fflags, None, field)
        want = ref.frontier_gain(g, i8, cfg, finfo, frecs, flags, field)
        n = int(finfo["n_written"])
        assert n == min(cap, n_clusters) and int(want[0]["n_candidates"]) == n
        assert want[1][n:].tobytes() == bytes(48 * (cap - n))
        for rep in range(2):
            fi, fr = np.zeros(1, frontier_ref.INFO_DTYPE), np.zeros(cap, frontier_ref.RECORD_DTYPE)
            info, out = np.zeros(1, ref.INFO_DTYPE), np.zeros(cap, ref.RECORD_DTYPE)
            h.frontier_async(cap, fi, fr, fflags)
            h.frontier_gain_async(info, out, flags)                # no wait in between
            h.synchronize()
            assert fr.tobytes() == frecs.tobytes()
            _same((info[0], out), want, ("frontier", cap, rep))
            _same(_resident(h, cap), want, ("frontier", cap, rep, "resident"))
        info, out = h.frontier_gain(flags)
        _same((info, out), want, ("frontier, waited", cap))
        # the same candidates as a list
        listed = _gain(gvamd, h, grid, cfg, frecs["goal_entry"][:n], flags, ("list", cap), i8, field, reps=1)
        assert listed[1].tobytes() == want[1][:n].tobytes() and listed[0].tobytes() == want[0].tobytes()
    # the doorway's cluster is one of the smallest and reveals the most: by gain it is the best one, by size it is not
    finfo, frecs, _ = frontier_ref.frontier(g, i8, fcfg, 64, fflags, None, field)
    info, out = ref.frontier_gain(g, i8, cfg, finfo, frecs, flags, field)
    door = int(np.flatnonzero(frecs["goal_entry"][:4] % 200 == 149)[0])
    assert int(np.argmax(out["n_unknown"][:4])) == door and int(frecs[door]["n_cells"]) == 4 < int(frecs["n_cells"][:4].max())
    if not use_field:
        assert int(info["best"]) == door and int(finfo["best"]) != door


def test_frontier_gain_without_clusters(gvamd):
    """an all-free map: no cluster, no candidate, zero records, best -1"""
    grid = "130x70"
    h = _handle(gvamd, grid)
    plant_occ(h, np.full((70, 130), gc.FREE, np.int8))
    h.set_frontier_config(gvamd.FrontierConfig.of(**frontier_ref.config()))
    h.set_gain_config(gvamd.GainConfig.of(**ref.config(radius=9)))
    h.frontier(8)
    info, out = h.frontier_gain()
    assert info.tolist() == (0, 0, -1, -1, 0, 0, 9) and out.tobytes() == bytes(8 * 48)
    h.set_inflation(*INFLATION)
    h.inflate()
    h.set_nav_config(253, 0)
    a = h.nav_field_from_gain(-1)                                  # no best: no usable seed
    assert a["n_seeds_used"] == 0 and not (h.nav_field_array() == 0).any()


# ------------------------------------------------------------------------------------- state and the arguments --
def _code(gvamd, call):
    with pytest.raises(gvamd.GVError) as e:
        call()
    return e.value.code


def test_state_and_arguments(gvamd):
    c = gc.cases()["duplicates"]
    (gx, gy, res), _ = gc.GRIDS[c["grid"]]
    h = gvamd.GridVisionHIP(gx, gy, res)
    lib = gvamd.load()
    entries = c["entries"].astype(np.int32)
    n = len(entries)
    try:
        call = lambda flags=0: h.gain(entries, flags)   # noqa: E731
        # no configuration; nothing resident
        assert _code(gvamd, call) == GV_ERR_STATE and _code(gvamd, h.frontier_gain) == GV_ERR_STATE
        for get in (h.device_gain, lambda: h.nav_field_from_gain(-1)):
            assert _code(gvamd, get) == GV_ERR_STATE
        i8 = plant_occ(h, c["occ"])
        h.set_gain_config(gvamd.GainConfig.of(**c["cfg"]))
        assert _code(gvamd, lambda: call(ref.USE_FIELD)) == GV_ERR_STATE     # no field
        assert _code(gvamd, h.frontier_gain) == GV_ERR_STATE                 # no resident frontier
        first = _gain(gvamd, h, c["grid"], c["cfg"], entries, 0, "first", i8)
        assert _code(gvamd, lambda: h.nav_field_from_gain(-1)) == GV_ERR_STATE   # a gain, no nav configuration
        # rejected configurations leave the one in force alone
        for bad in (dict(free_max=-1), dict(free_max=101), dict(free_max=40), dict(unknown_min=61), dict(unknown_max=101), dict(radius=0),
                    dict(radius=256), dict(min_gain=-1), dict(min_gain=(1 << 20) + 1), dict(w_gain=65536), dict(w_gain=-1), dict(w_dist=65536),
                    dict(w_dist=-1), dict(reserved=1)):
            assert _code(gvamd, lambda: h.set_gain_config(gvamd.GainConfig.of(**{**ref.config(), **bad}))) == GV_ERR_BAD_ARG, bad
        # arguments: state unchanged
        before = _resident(h, n)
        info, out = np.zeros(1, ref.INFO_DTYPE), np.zeros(4097, ref.RECORD_DTYPE)
        many = np.zeros(4097, np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
        for fn in (lib.gvx2_gain, lib.gvx2_gain_async):
            for k, e, flags, i, o in ((0, many, 0, info, out), (4097, many, 0, info, out), (-1, many, 0, info, out), (n, entries, 4, info, out),
                                      (n, entries, 8, info, out), (n, None, 0, info, out), (n, entries, 0, None, out), (n, entries, 0, info, None)):
                assert fn(h._h, C.c_int32(k), p(e), C.c_uint32(flags), p(i), p(o)) == GV_ERR_BAD_ARG, (k, flags)
            assert fn(None, C.c_int32(n), p(entries), C.c_uint32(0), p(info), p(out)) == GV_ERR_BAD_ARG
        for fn in (lib.gvx2_frontier_gain, lib.gvx2_frontier_gain_async):
            for flags, i, o in ((ref.DEVICE_ENTRIES, info, out), (4, info, out), (0, None, out), (0, info, None)):
                assert fn(h._h, C.c_uint32(flags), p(i), p(o)) == GV_ERR_BAD_ARG, flags
        h.set_nav_config(253, 0)
        h.set_inflation(*INFLATION)
        h.inflate()
        for k in (-2, n, 4096):
            assert _code(gvamd, lambda: h.nav_field_from_gain(k)) == GV_ERR_BAD_ARG, k
        _same(_resident(h, n), before, "after the refused calls")
        _same(_gain(gvamd, h, c["grid"], c["cfg"], entries, 0, "again", i8, reps=1), first, "again")
        # n = 4096 of the list call's own range, and the largest radius on a small map
        _gain(gvamd, h, c["grid"], ref.config(radius=255), entries[:1], 0, "R 255 on 200 x 80", i8, reps=1)
        # gv_reset invalidates the resident result and keeps the configuration
        h.set_gain_config(gvamd.GainConfig.of(**c["cfg"]))
        h.reset()
        for get in (h.device_gain, lambda: h.nav_field_from_gain(-1)):
            assert _code(gvamd, get) == GV_ERR_STATE
        info, recs = h.gain(entries)
        assert (recs["n_free"] == 0).all() and (recs["n_opaque"] == 0).all() and (recs["n_unknown"] > 0).all()   # the prior is unknown
        h.set_gain_config(None)
        assert _code(gvamd, call) == GV_ERR_STATE
    finally:
        h.close()


def test_after_grid_move(gvamd):
    """an all-free map scrolls: the border that scrolls in holds the prior (50), which the rays of a candidate beside it
    count; the configuration survives the move"""
    grid = "200x80"
    h = _handle(gvamd, grid)
    plant_occ(h, np.full((80, 200), gc.FREE, np.int8))
    cfg = ref.config(radius=15)
    entries = [gc.ent(grid, x, y) for x, y in ((5, 5), (194, 74), (100, 40), (5, 74), (194, 5))]
    before = _gain(gvamd, h, grid, cfg, entries, 0, "before", reps=1)
    assert (before[1]["n_unknown"] == 0).all()
    assert h.grid_move((0.0, 0.0, 0.0, 1.0, 1.2, -0.5, 0.0))["applied"]
    i8 = h.to_occupancy_grid()[0]
    assert 0 < (i8 == 50).sum() < 200 * 80 // 2 and ((i8 == 50) | (i8 == gc.FREE)).all()
    info, recs = h.gain(np.array(entries, np.int32))             # the configuration is still in force
    want = _gain(gvamd, h, grid, cfg, entries, 0, "moved", i8)
    _same((info, recs), want, "moved, before the configuration was set again")
    assert (want[1]["n_unknown"] > 0).any() and int(want[1][2]["n_unknown"]) == 0


# ------------------------------------------------------------------------------------------- a pending tick --
def test_gain_during_a_pending_tick(gvamd):
    """tick_enqueue, gain_async, tick_wait: the records are those of the tick's grid, as a twin handle finds them after
    its tick"""
    from gvamd import synth
    from test_gpu_parity import _ground_scene, make_handle
    hA, tfs = make_handle(gvamd, 2, perturbed=True)
    hB, _ = make_handle(gvamd, 2, perturbed=True)
    x, y, z, _, b = _ground_scene(tfs, seed=9)
    gcfg = synth.CONFIGS[2]["grid"]
    g = ref.grid(gcfg.grid_x, gcfg.grid_y, gcfg.resolution)
    n = 64
    pin_i, pin_r = gvamd.PinnedI8(32), gvamd.PinnedI8(n * 48)
    try:
        hB.upload_xyz(x, y, z)
        hB.tick(b, k_near=4, lidar_bin=True, lidar_raymarch=True)
        hB.tick(b, k_near=4, lidar_bin=True, lidar_raymarch=True)
        i8 = hB.to_occupancy_grid()[0]
        vals, counts = np.unique(i8, return_counts=True)
        u = int(vals[np.argmax(counts)])                 # never-observed cells: the prior less two decays
        assert 11 < u <= 50 and (i8 < u).any()
        cfg = ref.config(free_max=u - 1, unknown_min=u, unknown_max=u, radius=40)
        seen = np.flatnonzero(i8 < u)
        entries = seen[np.linspace(0, len(seen) - 1, n).astype(np.int64)].astype(np.int32)
        want = ref.gain(g, i8, cfg, entries)
        assert (want[1]["n_unknown"] > 0).any() and (want[1]["n_free"] > 0).any()
        hA.upload_xyz(x, y, z)
        hA.tick(b, k_near=4, lidar_bin=True, lidar_raymarch=True)
        hA.set_gain_config(gvamd.GainConfig.of(**cfg))
        hA.tick_enqueue(b, k_near=4, lidar_bin=True, lidar_raymarch=True)
        info, out = pin_i.array.view(ref.INFO_DTYPE), pin_r.array.view(ref.RECORD_DTYPE)
        hA.gain_async(entries, info, out)
        hA.tick_wait()
        hA.synchronize()
        _same((info[0], out), want, "pending tick")
        _same(_resident(hA, n), want, "pending tick, resident")
    finally:
        pin_i.close()
        pin_r.close()
        hA.close(); hB.close()


# --------------------------------------------------------------------------------------- the field from a gain --
def test_nav_field_from_gain(gvamd):
    """k = -1 (the resident best) and every k against gv_nav_field over the same cell's centre; an INVALID record and a
    candidate on a blocked cell seed nothing; then gv_nav_path from a start ends on the chosen goal"""
    name = "use_field_unreachable"
    c = gc.cases()[name]
    grid = c["grid"]
    g = gc.grid_of(grid)
    nx = g.nx
    h = _handle(gvamd, grid)
    i8 = plant_occ(h, c["occ"])
    field = make_field(h, grid, c["seeds"])
    entries = np.concatenate([c["entries"], [-1]]).astype(np.int32)     # reachable, on an occupied cell, reachable, invalid
    cfg = dict(c["cfg"], w_gain=50)
    info, recs = _gain(gvamd, h, grid, cfg, entries, ref.USE_FIELD, name, i8, field, reps=1)
    best = int(info["best"])
    assert best == 0 and int(recs[1]["status"]) == ref.UNREACHABLE_BIT and int(recs[3]["status"]) == ref.INVALID
    for k in (-1, 0, 1, 2, 3):
        e = int(entries[best if k < 0 else k])
        a = h.nav_field_from_gain(k)
        fa = h.nav_field_array()
        xy = np.array([nc.world_of(g, e % nx, e // nx)], np.float32) if e >= 0 else np.array([(1e6, 0.0)], np.float32)
        b = h.nav_field(xy)
        fb = h.nav_field_array()
        assert fa.tobytes() == fb.tobytes(), (k, first_diff(fa, fb))
        assert a["n_seeds_used"] == b["n_seeds_used"] == (1 if k in (-1, 0, 2) else 0), (k, a, b)
        _same(_resident(h, len(entries)), (info, recs), (k, "the resident gain survives"))
    h.nav_field_from_gain(-1)
    pinfo, _ = h.nav_path(np.array([nc.world_of(g, 10, 40)], np.float32), 4096, 0, keep_xy=False)
    assert int(pinfo[0]["status"]) == 0 and int(pinfo[0]["end_entry"]) == int(info["best_entry"])


def test_gain_demo(gvamd, tmp_path):
    """examples/gain_demo.cpp (plain g++ over the C headers): by size the long frontier in front of a wall wins, by gain the
    doorway into the unmapped hall; the field seeded with it on the device, the path from the vehicle that ends on it, and
    the demo's own host replay finds no mismatch"""
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "grid-vision_amd")
    exe = str(tmp_path / "gain_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(pkg, "examples", "gain_demo.cpp"), "-o", exe,
                           "-L" + pkg, "-lgridvision_hip", "-Wl,-rpath," + pkg])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    m = re.search(r"clusters (\d+) written (\d+) largest (\d+) best by size (\d+)\n", out.stdout)
    assert m, out.stdout
    clusters, written, largest, by_size = (int(v) for v in m.groups())
    m = re.search(r"candidates (\d+) ranked (\d+) best by gain (\d+) entry (\d+) score (-?\d+)\n", out.stdout)
    assert m, out.stdout
    cands, ranked, by_gain = (int(v) for v in m.groups()[:3])
    assert clusters == written == cands >= 2 and ranked >= 1 and largest >= 100 and by_gain != by_size, out.stdout
    rows = {int(r[0]): (int(r[1]), int(r[2])) for r in re.findall(r"cluster (\d+): (\d+) cells, .*unknown in sight (\d+),", out.stdout)}
    assert rows[by_size][0] == largest and rows[by_gain][0] < 20 and rows[by_gain][1] > rows[by_size][1], out.stdout
    m = re.search(r"goal field seeds 1 rounds (\d+)\npath cells (\d+) status 0 ends_on_goal yes\n", out.stdout)
    assert m and int(m.group(2)) > 50, out.stdout
    assert "host check ok (0 mismatches)" in out.stdout, out.stdout
