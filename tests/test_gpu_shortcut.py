"""[EXTENSION] X21 shortcuts and waypoints on the device: gvx3_shortcut against shortcut_ref (a plain Python reference) and
against the host twin, both run on the device's own resident paths and costmap read back, with zero tolerance: every
comparison is tobytes() equality of the records and of entries, index and cell centres up to n_waypoints.  The costmaps of
shortcut_cases.py are planted through the library's own inflate path, the paths come from gv_nav_field and gv_nav_path.
Then the destinations, the getters, the call inside a pending tick, gvx3_nav_field_from_shortcut against gv_nav_field over
the downloaded waypoints, the state errors, and the source paths, which every call must leave as they were."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nav_cases as nc
import path_ref
import shortcut_cases as sc
import shortcut_ref as ref
from planner_util import first_diff, hip_runtime, plant
from test_shortcut_host import packed, same

pytestmark = pytest.mark.gpu

GV_ERR_BAD_ARG, GV_ERR_STATE = 1, 5
HERE = os.path.dirname(os.path.abspath(__file__))
OFF_MAP = (1e6, 0.0)
GPU_CASES = [n for n, c in sc.cases().items() if c["gpu"]]
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
        (gx, gy, res), (nx, ny) = sc.GRIDS[grid]
        h = gvamd.GridVisionHIP(gx, gy, res)
        assert (h.nx, h.ny) == (nx, ny)
        _HANDLES[grid] = h
    h = _HANDLES[grid]
    h.reset()
    return h


def _download(dsts_srcs):
    hip = hip_runtime()
    for dst, src in dsts_srcs:
        assert hip.hipMemcpy(dst.ctypes.data, src, dst.nbytes, 2) == 0   # hipMemcpyDeviceToHost


def _source(h):
    """(info (S,), entries (S, cap)) of the resident paths, through gv_device_nav_path's pointers"""
    d = h.device_nav_path()
    info, ent = np.zeros(d["S"], path_ref.INFO_DTYPE), np.zeros((d["S"], d["cap"]), np.int32)
    h.synchronize()
    _download(((info, d["info"]), (ent, d["entries"])))
    return info, ent


def _resident(h):
    """(info (S,), entries (S, wcap), index (S, wcap), xy (S, wcap, 2)) of the resident waypoints, through
    gvx3_device_shortcut's pointers"""
    d = h.device_shortcut()
    S, wcap = d["S"], d["wcap"]
    info, ent, idx, xy = np.zeros(S, ref.INFO_DTYPE), np.zeros((S, wcap), np.int32), np.zeros((S, wcap), np.int32), np.zeros((S, wcap, 2), np.float32)
    h.synchronize()
    _download(((info, d["info"]), (ent, d["entries"]), (idx, d["index"]), (xy, d["xy"])))
    return info, ent, idx, xy


def _paths(h, c):
    """plant the case's costmap, solve the field from its goal, walk its starts: the device's own costmap and paths"""
    g = sc.grid_of(c["grid"])
    cost = plant(h, c["mask"], c["inflation"])
    assert cost.tobytes() == c["cost"].tobytes()                  # the host tests shortcut over the same costmap
    h.set_nav_config(*sc.NAV_CONFIG)
    h.nav_field(np.array([nc.world_of(g, *c["goal"])], np.float32))
    starts = np.array([nc.world_of(g, *s) if s is not None else OFF_MAP for s in c["starts"]], np.float32)
    h.nav_path(starts, c["cap"], c["path_flags"], keep_xy=False)
    info, ent = _source(h)
    paths = [ent[s, :int(info[s]["n_cells"])].tolist() for s in range(len(info))]
    assert [len(p) == 0 for p in paths] == [s is None for s in c["starts"]]
    assert all(int(r["status"]) == path_ref.REACHED for r, s in zip(info, c["starts"]) if s is not None)
    return cost, paths, (info, ent)


def _want(gvamd, c, cost, paths, wcap=None, flags=None, cfg=None):
    """the reference's result over the device's paths and costmap, which the twin's must equal"""
    wcap = c["wcap"] if wcap is None else wcap
    flags = c["flags"] if flags is None else flags
    cfg = c["cfg"] if cfg is None else cfg
    want = ref.shortcut(sc.grid_of(c["grid"]), cost, cfg, paths, wcap, flags)
    src, n = packed(paths, c["cap"])
    same(gvamd.shortcut_host(*sc.GRIDS[c["grid"]][0], cost, gvamd.ShortcutConfig.of(**cfg), src, n, wcap, flags), want, "twin")
    return want


def _unchanged(h, before, tag):
    after = _source(h)
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes(), tag


# ------------------------------------------------------------------------------------------------------ the cases --
@pytest.mark.parametrize("name", GPU_CASES)
def test_cases(gvamd, name):
    c = sc.cases()[name]
    h = _handle(gvamd, c["grid"])
    cost, paths, source = _paths(h, c)
    if c["same"]:
        assert paths == c["paths"]                                # the edge the fixture is named for is met here too
    want = _want(gvamd, c, cost, paths)
    if c["same"]:
        sc.check(name, c, *want)
    h.set_shortcut_config(gvamd.ShortcutConfig.of(**c["cfg"]))
    for rep in range(2):
        info, xy = h.shortcut(c["wcap"], c["flags"])
        assert info.dtype == ref.INFO_DTYPE
        same((info, None, None, xy), want, (name, rep, "returned"))
        same(_resident(h), want, (name, rep, "resident"))
    for s in range(len(paths)):                                   # gvx3_get_shortcut agrees with the device pointers
        rec, ent, idx, xy_s = h.shortcut_get(s)
        assert rec.tobytes() == want[0][s].tobytes() and ent.tobytes() == want[1][s].tobytes()
        assert idx.tobytes() == want[2][s].tobytes() and xy_s.tobytes() == want[3][s].tobytes()
    _unchanged(h, source, name)
    other = c["flags"] ^ ref.NO_CORNER                            # the same resident paths under the other flag
    info, xy = h.shortcut(c["wcap"], other)
    same((info, None, None, xy), _want(gvamd, c, cost, paths, flags=other), (name, "other flag"))
    _unchanged(h, source, (name, "other flag"))


def test_waypoints_behind_the_written_ones_are_left_alone(gvamd):
    """resident buffers and a pinned destination filled with a pattern: nothing is stored past n_waypoints, for the paths
    that truncate, that fit and that are empty alike"""
    c = sc.cases()["lengths"]
    h = _handle(gvamd, c["grid"])
    cost, paths, source = _paths(h, c)
    S = len(paths)
    cfg = ref.config(window=4, spacing=2)
    h.set_shortcut_config(gvamd.ShortcutConfig.of(**cfg))
    wcap = 20
    want = _want(gvamd, c, cost, paths, wcap=wcap, cfg=cfg)
    assert {ref.OK, ref.TRUNCATED, ref.EMPTY} == set(want[0]["status"].tolist())
    h.shortcut(wcap)
    hip = hip_runtime()
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    d = h.device_shortcut()
    assert (d["S"], d["wcap"]) == (S, wcap)
    for key, width in (("entries", 4), ("index", 4), ("xy", 8)):
        assert hip.hipMemset(d[key], 0x5A, S * wcap * width) == 0
    pin_info, pin_xy = gvamd.PinnedI8(S * 32), gvamd.PinnedF32(S * wcap * 2)
    try:
        pin_xy.array[:] = -7.0
        info = pin_info.array.view(ref.INFO_DTYPE)
        h.shortcut_async(wcap, info, pin_xy.array)
        h.synchronize()
        assert h.device_shortcut() == d                           # the same buffers
        got = _resident(h)
        same(got, want, "pattern")
        same((info, None, None, pin_xy.array.reshape(S, wcap, 2)), want, "pinned")
        for s in range(S):
            n = int(want[0][s]["n_waypoints"])
            assert (got[1][s, n:] == 0x5A5A5A5A).all() and (got[2][s, n:] == 0x5A5A5A5A).all(), s
            assert (got[3][s, n:].view(np.uint32) == 0x5A5A5A5A).all() and (pin_xy.array.reshape(S, wcap, 2)[s, n:] == -7.0).all(), s
    finally:
        pin_info.close()
        pin_xy.close()
    _unchanged(h, source, "pattern")


def test_destinations(gvamd):
    """info and way_xy into pageable and pinned memory (aligned, and pinned but not aligned: the copy command), way_xy
    NULL followed by gvx3_get_shortcut with a short cap_out"""
    c = sc.cases()["octants_no_corner"]
    h = _handle(gvamd, c["grid"])
    cost, paths, source = _paths(h, c)
    S, wcap = len(paths), c["wcap"]
    want = _want(gvamd, c, cost, paths)
    h.set_shortcut_config(gvamd.ShortcutConfig.of(**c["cfg"]))
    pin_i, pin_x = gvamd.PinnedI8(S * 32 + 16), gvamd.PinnedF32(S * wcap * 2 + 4)
    try:
        for i_off, x_off in ((0, 0), (4, 1), (0, 1), (4, 0)):
            pin_i.array[:] = 77
            pin_x.array[:] = -7.0
            info = pin_i.array[i_off:i_off + S * 32].view(ref.INFO_DTYPE)
            xy = pin_x.array[x_off:x_off + S * wcap * 2]
            h.shortcut_async(wcap, info, xy, c["flags"])
            h.synchronize()
            same((info, None, None, xy.reshape(S, wcap, 2)), want, ("pinned", i_off, x_off))
            assert (pin_i.array[i_off + S * 32:] == 77).all() and (pin_x.array[x_off + S * wcap * 2:] == -7.0).all()
        info, xy = np.zeros(S, ref.INFO_DTYPE), np.zeros(S * wcap * 2, np.float32)
        h.shortcut_async(wcap, info, xy, c["flags"])
        h.synchronize()
        same((info, None, None, xy.reshape(S, wcap, 2)), want, "pageable")
        info, none = h.shortcut(wcap, c["flags"], keep_xy=False)
        assert none is None and info.tobytes() == want[0].tobytes()
        for s in range(S):
            n = int(want[0][s]["n_waypoints"])
            rec, ent, idx, xy_s = h.shortcut_get(s, cap_out=3)
            assert rec.tobytes() == want[0][s].tobytes() and ent.tobytes() == want[1][s][:3].tobytes()
            assert idx.tobytes() == want[2][s][:3].tobytes() and xy_s.tobytes() == want[3][s][:3].tobytes() and len(ent) == min(n, 3)
    finally:
        pin_i.close()
        pin_x.close()
    _unchanged(h, source, "destinations")


# ----------------------------------------------------------------------------------- the field from the waypoints --
def _field_from_shortcut(h, s, tag):
    """gvx3_nav_field_from_shortcut(s) against gv_nav_field over the read-back centres of shortcut s; the resident
    waypoints and paths survive both.  Returns (field, n_seeds_used)."""
    before, source = _resident(h), _source(h)
    rec, _, _, xy = h.shortcut_get(s)
    a = h.nav_field_from_shortcut(s)
    fa = h.nav_field_array()
    n = int(rec["n_waypoints"])
    b = h.nav_field(xy if n else np.array([OFF_MAP], np.float32))
    fb = h.nav_field_array()
    assert fa.tobytes() == fb.tobytes(), (tag, first_diff(fa, fb))
    assert a["n_seeds_used"] == b["n_seeds_used"], (tag, a, b)
    after = _resident(h)
    assert before[0].tobytes() == after[0].tobytes()
    for k in range(len(before[0])):
        m = int(before[0][k]["n_waypoints"])
        assert all(x[k, :m].tobytes() == y[k, :m].tobytes() for x, y in zip(before[1:], after[1:])), (tag, k)
    _unchanged(h, source, tag)
    return fa, a["n_seeds_used"]


def test_field_from_shortcut(gvamd):
    """spacing 1: the PathDist field of the straightened path; an empty source is "no usable seed"; a truncated shortcut
    seeds with what was written"""
    c = sc.cases()["lengths"]
    h = _handle(gvamd, c["grid"])
    cost, paths, _ = _paths(h, c)
    goal_field = h.nav_field_array()
    for cfg, wcap in ((ref.config(window=64, spacing=1), 128), (ref.config(window=8, spacing=3), 6)):
        h.set_shortcut_config(gvamd.ShortcutConfig.of(**cfg))
        want = _want(gvamd, c, cost, paths, wcap=wcap, cfg=cfg)
        info, _ = h.shortcut(wcap, keep_xy=False)
        assert info.tobytes() == want[0].tobytes()
        for s in range(len(paths)):
            f, used = _field_from_shortcut(h, s, (wcap, s))
            n = int(info[s]["n_waypoints"])
            assert used == n == int((f == 0).sum())
            if n == 0:
                assert (f >= path_ref.UNREACHABLE).all()
        assert (wcap == 6) == (ref.TRUNCATED in info["status"].tolist())
    assert h.nav_field_array().tobytes() != goal_field.tobytes()


def test_field_from_shortcut_skips_waypoints_blocked_since(gvamd):
    """a wall planted across the resident waypoints and a new gv_inflate: the waypoints inside it are skipped as
    gv_nav_field skips such seeds"""
    c = sc.cases()["between_63_64_65_129"]
    h = _handle(gvamd, c["grid"])
    _paths(h, c)
    h.set_shortcut_config(gvamd.ShortcutConfig.of(**c["cfg"]))
    info, _ = h.shortcut(c["wcap"], keep_xy=False)
    wall = sc.mask_of(c["grid"])
    wall[:, 150:153] = True                                       # every path runs along row 50 through x = 150 .. 152
    plant(h, wall, sc.EXACT)
    for s in range(4):
        f, used = _field_from_shortcut(h, s, ("wall", s))
        assert used == int(info[s]["n_waypoints"]) - 3 == int((f == 0).sum())


# ------------------------------------------------------------------------------------------- ordering and state --
def _code(gvamd, call):
    with pytest.raises(gvamd.GVError) as e:
        call()
    return e.value.code


def test_state_errors_and_arguments(gvamd):
    c = sc.cases()["pillar"]
    g = sc.grid_of(c["grid"])
    (gx, gy, res), _ = sc.GRIDS[c["grid"]]
    h = gvamd.GridVisionHIP(gx, gy, res)
    lib = gvamd.load()
    try:
        cfg = gvamd.ShortcutConfig.of(**c["cfg"])
        cut = lambda: h.shortcut(64)   # noqa: E731
        getters = (h.device_shortcut, lambda: h.shortcut_get(0), lambda: h.nav_field_from_shortcut(0))
        info1 = np.zeros(256, ref.INFO_DTYPE)
        raw = lambda wcap=64, flags=0, inf=info1, fn=lib.gvx3_shortcut: fn(h._h, C.c_int32(wcap), C.c_uint32(flags),   # noqa: E731
                                                                           inf.ctypes.data_as(C.c_void_p) if inf is not None else None, None)
        # nothing yet: no configuration, no path, no costmap
        assert raw() == GV_ERR_STATE
        h.set_shortcut_config(cfg)
        assert raw() == GV_ERR_STATE                              # no resident path
        plant(h, c["mask"], c["inflation"])
        h.set_nav_config(*sc.NAV_CONFIG)
        assert raw() == GV_ERR_STATE
        h.nav_field(np.array([nc.world_of(g, *c["goal"])], np.float32))
        assert raw() == GV_ERR_STATE                              # a field, still no path
        starts = np.array([nc.world_of(g, *c["starts"][0])], np.float32)
        h.nav_path(starts, c["cap"], 0, keep_xy=False)
        for call in getters:
            assert _code(gvamd, call) == GV_ERR_STATE             # a path, no shortcut yet
        h.set_shortcut_config(None)
        assert raw() == GV_ERR_STATE                              # no configuration
        # the ranges of the configuration: refused, and the one in force stays
        h.set_shortcut_config(cfg)
        for k in (dict(max_cost=255), dict(window=0), dict(window=4097), dict(spacing=65536), dict(max_cost=-1)):
            assert _code(gvamd, lambda: h.set_shortcut_config(gvamd.ShortcutConfig.of(**{**c["cfg"], **k}))) == GV_ERR_BAD_ARG
        # a 1-rank communicator changes nothing
        h.comm_init(gvamd.GridVisionHIP.comm_unique_id(), 0, 1)
        cost, (pinfo, pent) = h.costmap(), _source(h)
        paths = [pent[0, :int(pinfo[0]["n_cells"])].tolist()]
        want = _want(gvamd, c, cost, paths, wcap=64)
        assert want[2][0].tolist() == [0, 15]
        info, xy = cut()
        same((info, None, None, xy), want, "first")
        # arguments: state unchanged
        before = _resident(h)
        for fn in (lib.gvx3_shortcut, lib.gvx3_shortcut_async):
            for kw in (dict(wcap=0), dict(wcap=65537), dict(wcap=-3), dict(flags=2), dict(inf=None)):
                assert raw(fn=fn, **kw) == GV_ERR_BAD_ARG, kw
        assert _code(gvamd, lambda: h.shortcut_get(1)) == GV_ERR_BAD_ARG and _code(gvamd, lambda: h.shortcut_get(-1)) == GV_ERR_BAD_ARG
        assert _code(gvamd, lambda: h.nav_field_from_shortcut(1)) == GV_ERR_BAD_ARG
        assert _code(gvamd, lambda: h.nav_field_from_shortcut(-1)) == GV_ERR_BAD_ARG
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, _resident(h)))
        # S * wcap above 2^20 is known only with the resident paths: 17 paths
        h.nav_path(np.repeat(starts, 17, axis=0), 64, 0, keep_xy=False)
        assert raw(wcap=65536) == GV_ERR_BAD_ARG and raw(wcap=61680) == 0 and h.device_shortcut()["S"] == 17
        h.nav_path(starts, c["cap"], 0, keep_xy=False)
        # the call reads the costmap as it stands: a new inflate with the pillar gone, the old path
        plant(h, sc.mask_of(c["grid"]), sc.EXACT)
        h.nav_field(np.array([nc.world_of(g, *c["goal"])], np.float32))
        info, _ = cut()
        same((info, None, None, None), _want(gvamd, c, h.costmap(), paths, wcap=64), "new costmap")
        # no nav configuration: the field from a shortcut is refused, the shortcut call is not
        h.set_nav_config(None)
        assert _code(gvamd, lambda: h.nav_field_from_shortcut(0)) == GV_ERR_STATE
        cut()
        h.set_nav_config(*sc.NAV_CONFIG)
        # gv_reset invalidates the paths and the waypoints and keeps the configuration
        h.reset()
        for call in (cut,) + getters:
            assert _code(gvamd, call) == GV_ERR_STATE
        plant(h, c["mask"], c["inflation"])
        h.nav_field(np.array([nc.world_of(g, *c["goal"])], np.float32))
        h.nav_path(starts, c["cap"], 0, keep_xy=False)
        assert _code(gvamd, h.device_shortcut) == GV_ERR_STATE
        info, xy = cut()
        same((info, None, None, xy), want, "after reset")
    finally:
        h.close()


def test_shortcut_demo(gvamd, tmp_path):
    """examples/shortcut_demo.cpp (plain g++ over the C headers): the staircase through the doorway becomes a handful of
    anchors, the straightened path is shorter, the field is seeded by every waypoint, and the demo's own replay with the
    host twin finds no mismatch"""
    pkg = os.path.join(os.path.dirname(HERE), "grid-vision_amd")
    exe = str(tmp_path / "shortcut_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(pkg, "examples", "shortcut_demo.cpp"), "-o", exe,
                           "-L" + pkg, "-lgridvision_hip", "-Wl,-rpath," + pkg])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    m = re.search(r"path cells (\d+) diagonal (\d+) status 0\n"
                  r"waypoints (\d+) anchors (\d+) status 0 steps (\d+) diagonal (\d+) max_cost_seen (\d+)\n"
                  r"waypoint field seeds (\d+) rounds (\d+)\n", out.stdout)
    assert m, out.stdout
    cells, _, ways, anchors, steps, _, seen, seeds, rounds = (int(v) for v in m.groups())
    assert 3 <= anchors <= 12 and anchors < ways == seeds and steps < cells and seen <= 128 and rounds >= 1
    m = re.search(r"straightened length ([\d.]+) m, staircase ([\d.]+) m\nhost check ok \(0 mismatches\)", out.stdout)
    assert m and float(m.group(1)) < float(m.group(2)), out.stdout


def test_shortcut_during_a_pending_tick(gvamd):
    """tick_enqueue, inflate, nav_field, nav_path_async, shortcut_async, tick_wait: the waypoints are those of the tick's
    grid, as a second handle makes them after its tick, and as the reference makes them from that handle's costmap and
    paths"""
    from gvamd import synth
    from test_gpu_parity import _ground_scene, make_handle
    P5 = (0.5, 1.1, 5.0, 80)
    hA, tfs = make_handle(gvamd, 2, perturbed=True)
    hB, _ = make_handle(gvamd, 2, perturbed=True)
    x, y, z, _, b = _ground_scene(tfs, seed=9)
    seeds = np.array([(40.0, 0.0)], np.float32)
    starts = np.array([(0.0, 0.0), (10.0, 30.0), (-20.0, -15.0), OFF_MAP], np.float32)
    cap, wcap = 2048, 256
    gcfg = synth.CONFIGS[2]["grid"]
    g = ref.grid(gcfg.grid_x, gcfg.grid_y, gcfg.resolution)
    assert (g.nx, g.ny) == (hA.nx, hA.ny)
    cfg = ref.config(max_cost=180, window=128, spacing=6)
    pin_p, pin_s = gvamd.PinnedI8(4 * 32), gvamd.PinnedI8(4 * 32)
    try:
        for h in (hA, hB):
            h.upload_xyz(x, y, z)
            h.tick(b, k_near=4, lidar_bin=True)
            h.set_inflation(*P5)
            h.set_nav_config(253, 2)
            h.set_shortcut_config(gvamd.ShortcutConfig.of(**cfg))
        hA.tick_enqueue(b, k_near=4, lidar_bin=True)
        hA.inflate()
        hA.nav_field(seeds)
        hA.nav_path_async(starts, cap, pin_p.array.view(path_ref.INFO_DTYPE), None, path_ref.DIAGONAL)
        info = pin_s.array.view(ref.INFO_DTYPE)
        hA.shortcut_async(wcap, info, None, ref.NO_CORNER)
        hA.tick_wait()
        hA.synchronize()
        got = _resident(hA)
        assert got[0].tobytes() == info.tobytes()
        hB.tick(b, k_near=4, lidar_bin=True)
        hB.inflate()
        hB.nav_field(seeds)
        hB.nav_path(starts, cap, path_ref.DIAGONAL, keep_xy=False)
        pinfo, pent = _source(hB)
        paths = [pent[s, :int(pinfo[s]["n_cells"])].tolist() for s in range(4)]
        want = ref.shortcut(g, hB.costmap(), cfg, paths, wcap, ref.NO_CORNER)
        same(got, want, "pending tick")
        assert info["status"].tolist()[3] == ref.EMPTY and (info["n_src"][:3] == pinfo["n_cells"][:3]).all()
    finally:
        pin_p.close()
        pin_s.close()
        hA.close(); hB.close()
