"""[EXTENSION] X9 goal / path distance field on the device: gv_nav_field against nav_ref (a heap Dijkstra, one cell after
the other) and gv_score_nav against nav_ref's loops, with zero tolerance.  Walls are planted by planner_util.plant,
inflated on the device, and the costmap() READBACK goes to the reference.  Every comparison is tobytes() equality, every
call is made three times with the same bytes.  Then the 2000 x 2000 map against a closed form, the sampler's input and
output paths, the ordering and state rules of the header, the pass cap's own path, and the example."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nav_cases as nc
import nav_ref as ref
import traj_cases as tc
from planner_util import first_diff, hip_runtime, plant
from test_gpu_parity import _ground_scene, make_handle

pytestmark = pytest.mark.gpu

GV_ERR_BAD_ARG, GV_ERR_STATE = 1, 5
HERE = os.path.dirname(os.path.abspath(__file__))
_HANDLES = {}   # grid name -> handle, shared by the cases of the module
_WANT = {}      # (costmap bytes, config, seed bytes) -> nav_ref.field


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    yield m
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()
    _WANT.clear()


def _handle(gvamd, grid):
    if grid not in _HANDLES:
        (gx, gy, res), (nx, ny) = nc.GRIDS[grid]
        h = gvamd.GridVisionHIP(gx, gy, res)
        assert (h.nx, h.ny) == (nx, ny)
        _HANDLES[grid] = h
    h = _HANDLES[grid]
    h.reset()
    return h


def _want(g, cost, cfg, seeds):
    key = (hash(cost.tobytes()), g.nx, g.ny, cfg, np.asarray(seeds, np.float32).tobytes())
    if key not in _WANT:
        _WANT[key] = ref.field(cost, g.nx, g.ny, ref.step_table(*cfg), ref.seed_cells(g, seeds))
    return _WANT[key]


def _solve(h, g, cost, cfg, seeds, tag=""):
    """three calls, each equal to the reference byte for byte; returns (field, the last call's info)"""
    want, used = _want(g, cost, cfg, seeds)
    h.set_nav_config(*cfg)
    for rep in range(3):
        info = h.nav_field(seeds)
        got = h.nav_field_array()
        assert got.dtype == np.uint32 and got.tobytes() == want.tobytes(), (tag, cfg, rep, first_diff(got, want))
        assert info["n_seeds_used"] == used and info["rounds"] >= 1, (tag, cfg, rep, info)
    return want, info


CASES = ["serpentine_200x80", "comb_250x100", "in_tile_200x200", "staircase", "pocket_outside", "pocket_inside",
         "random_0.3", "random_5e-4", "random_2e-3"]


def test_every_case_is_solved():
    assert sorted(CASES) == sorted(nc.cases())


@pytest.mark.parametrize("seeds", ["goal", "path"])
@pytest.mark.parametrize("name", CASES)
def test_fixtures(gvamd, name, seeds):
    c = nc.cases()[name]
    g = nc.grid_of(c["grid"])
    h = _handle(gvamd, c["grid"])
    cost = plant(h, c["mask"], c["inflation"])
    assert cost.tobytes() == c["cost"].tobytes()          # the host tests ran on the same costmap
    for cfg in nc.CONFIGS:
        want, info = _solve(h, g, cost, cfg, c[seeds], tag=(name, seeds))
        if seeds == "path":
            cells = ref.seed_cells(g, c["path"])
            n_blocked = int((cost[cells] >= 254).sum())
            assert len(cells) == nc.PATH_POINTS - c["n_off"] - c["n_nonfinite"]
            assert info["n_seeds_used"] == len(cells) - n_blocked < len(cells)
        else:
            assert info["n_seeds_used"] == 1
            if name == "serpentine_200x80":
                assert int(want[want < ref.UNREACHABLE].max()) == 8039 and info["rounds"] >= 2
            if name == "staircase":
                assert int((want == ref.UNREACHABLE).sum()) == 199 * 200 // 2


def test_empty_and_full_map(gvamd):
    """250 x 100: ragged last tiles in both axes.  The empty map is |dx| + |dy| from a seed at the centre, at a corner
    and on each border; the full map is blocked everywhere and no seed is used."""
    g = nc.grid_of("250x100")
    h = _handle(gvamd, "250x100")
    cost = plant(h, np.zeros((g.ny, g.nx), bool), nc.EXACT)
    ys, xs = np.mgrid[0:g.ny, 0:g.nx]
    for sx, sy in ((g.nx // 2, g.ny // 2), (0, 0), (g.nx - 1, g.ny - 1), (0, g.ny // 2), (g.nx - 1, g.ny // 2), (g.nx // 2, 0),
                   (g.nx // 2, g.ny - 1)):
        seeds = np.array([nc.world_of(g, sx, sy)], np.float32)
        want, _ = _solve(h, g, cost, (253, 0), seeds, tag=("empty", sx, sy))
        assert np.array_equal(want.reshape(g.ny, g.nx), np.abs(xs - sx) + np.abs(ys - sy))
    cost = plant(h, np.ones((g.ny, g.nx), bool), nc.EXACT)
    want, info = _solve(h, g, cost, (253, 0), seeds, tag="full")
    assert (want == ref.BLOCKED).all() and info["n_seeds_used"] == 0
    # no usable seed on a map with free cells: unreachable everywhere, not an error
    cost = plant(h, np.zeros((g.ny, g.nx), bool), nc.EXACT)
    want, info = _solve(h, g, cost, (253, 0), np.array([(1e6, 0.0), (np.nan, 0.0)], np.float32), tag="no seed")
    assert (want == ref.UNREACHABLE).all() and info["n_seeds_used"] == 0


def test_2000x2000_wall_with_one_gap(gvamd):
    """the one case at that size: a wall over every row of column 1200 but one, weight 0, against the closed form
    through the gap (a Python Dijkstra over 4 M cells is too slow for a test)"""
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
        ys, xs = np.mgrid[0:ny, 0:nx]
        to_gap = abs(xw - sx) + abs(yg - sy)
        want = np.where(xs < xw, np.abs(xs - sx) + np.abs(ys - sy), to_gap + (xs - xw) + np.abs(ys - yg)).astype(np.uint32)
        want[mask] = ref.BLOCKED
        h.set_nav_config(253, 0)
        seeds = np.array([nc.world_of(g, sx, sy)], np.float32)
        assert ref.seed_cells(g, seeds) == [sy * nx + sx]
        for rep in range(3):
            info = h.nav_field(seeds)
            got = h.nav_field_array()
            assert got.tobytes() == want.tobytes(), (rep, first_diff(got, want))
            assert info["n_seeds_used"] == 1
        # the overflow rule: (1 + w * 252) * (G - 1) <= 0xFFFFFFFD admits the weights 0..4 here
        h.set_nav_config(253, 4)
        with pytest.raises(gvamd.GVError) as e:
            h.set_nav_config(253, 5)
        assert e.value.code == GV_ERR_BAD_ARG
        h.nav_field(seeds)                                   # the configuration in force is still (253, 4)
        assert h.nav_field_array().tobytes() == want.tobytes()    # every free cell costs 0: weight 4 changes nothing
    finally:
        h.close()


def test_pass_cap_path(gvamd):
    """GV_NAV_PASS_CAP=3 (read at gv_create): the tile of the in-tile serpentine hits the cap round after round, marks
    itself active and goes on; the field is the same"""
    c = nc.cases()["in_tile_200x200"]
    g = nc.grid_of(c["grid"])
    (gx, gy, res), _ = nc.GRIDS[c["grid"]]
    os.environ["GV_NAV_PASS_CAP"] = "3"
    try:
        h = gvamd.GridVisionHIP(gx, gy, res)
    finally:
        del os.environ["GV_NAV_PASS_CAP"]
    try:
        cost = plant(h, c["mask"], c["inflation"])
        want, info = _solve(h, g, cost, (253, 0), c["goal"], tag="cap 3")
        assert info["rounds"] >= 10
        h2 = _handle(gvamd, c["grid"])
        plant(h2, c["mask"], c["inflation"])
        _, info2 = _solve(h2, g, cost, (253, 0), c["goal"], tag="cap 40")
        assert info2["rounds"] < info["rounds"]
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------------- sampler --
SAMPLER = [("rect_3x130", "random_5e-4"), ("point_257x2", "random_0.3"), ("leaving_3x64", "random_5e-4"),
           ("nonfinite_8x3", "comb_250x100")]


@pytest.mark.parametrize("family,case", SAMPLER)
def test_sampler_paths(gvamd, family, case):
    """host poses, pinned poses and device poses; pageable, pinned 8-aligned and pinned unaligned destinations: the same
    bytes every way, three times"""
    f, c = tc.families()[family], nc.cases()[case]
    assert f["grid"] == c["grid"]
    g = nc.grid_of(c["grid"])
    h = _handle(gvamd, c["grid"])
    cost = plant(h, c["mask"], c["inflation"])
    fld, _ = _solve(h, g, cost, (253, 3), c["goal"], tag=case)
    poses = f["poses"]
    K, P = poses.shape[:2]
    want = ref.score(g, fld, poses)
    if family == "leaving_3x64":
        assert want["n_bad"].min() >= 1 and int(want["last"][0]) == ref.BLOCKED
    if family == "nonfinite_8x3":
        assert (want["n_bad"][1:6] >= 1).all()               # a NaN or infinite x or y; the yaw (6, 7) is never read
        assert want[6].tobytes() == want[0].tobytes() == want[7].tobytes()
    if family == "point_257x2":
        assert (want["best_pose"] == -1).any() and (want["best_pose"] >= 0).any()
    hip, dptr = hip_runtime(), C.c_void_p()
    assert hip.hipMalloc(C.byref(dptr), poses.nbytes) == 0
    pin_s, pin_in = gvamd.PinnedI8(K * 24 + 16), gvamd.PinnedF32(poses.size)
    try:
        assert hip.hipMemcpy(dptr, poses.ctypes.data, poses.nbytes, 1) == 0   # hipMemcpyHostToDevice
        pin_in.array[:] = poses.reshape(-1)
        for rep in range(3):
            got = h.score_nav(poses)
            assert got.dtype == ref.SCORE_DTYPE and got.tobytes() == want.tobytes(), (rep, first_diff(got.view(np.uint32), want.view(np.uint32)))
            assert h.score_nav(poses, device_ptr=dptr.value).tobytes() == want.tobytes(), ("device poses", rep)
            for src, dev in ((pin_in.array, None), (poses, None), (None, dptr.value)):
                pin_s.array[:] = 77
                aligned = pin_s.array[:K * 24].view(ref.SCORE_DTYPE)
                h.score_nav_async(src, K, P, aligned, device_ptr=dev)
                h.synchronize()
                assert aligned.tobytes() == want.tobytes() and (pin_s.array[K * 24:] == 77).all(), ("pinned", rep)
                odd = pin_s.array[4:4 + K * 24].view(ref.SCORE_DTYPE)      # pinned, not 8-byte aligned: the copy command
                h.score_nav_async(src, K, P, odd, device_ptr=dev)
                h.synchronize()
                assert odd.tobytes() == want.tobytes(), ("pinned, unaligned", rep)
                page = np.zeros(K, ref.SCORE_DTYPE)
                h.score_nav_async(src, K, P, page, device_ptr=dev)
                h.synchronize()
                assert page.tobytes() == want.tobytes(), ("pageable", rep)
    finally:
        hip.hipFree(dptr)
        pin_s.close()
        pin_in.close()


def test_samplers_back_to_back_share_the_pose_copy(gvamd):
    """gv_score_trajectories_async (3 x 65: across the 64-pose chunk), gv_score_nav_async (5 x 130, other poses: the
    handle's device copy of host poses grows while the first call may be in flight) and gv_score_trajectories_async
    (2 x 1) with no synchronisation between them, pageable poses and destinations: every record equals the reference
    of its own poses.  Then the same with the middle call's poses read from device memory."""
    import traj_ref
    c = nc.cases()["random_5e-4"]
    g, fp = nc.grid_of(c["grid"]), tc.fp_of("rect")
    h = _handle(gvamd, c["grid"])
    cost = plant(h, c["mask"], c["inflation"])
    fld, _ = _solve(h, g, cost, (253, 3), c["goal"], tag="shared poses")
    h.set_footprint(tc.FOOTPRINTS["rect"])
    box = (0.0, 32.0, -4.0, 4.0)
    first = tc.arcs("shared_first", g, fp, 3, 65, 900, box, 0.04)
    middle = tc.arcs("shared_middle", g, tc.fp_of("point"), 5, 130, 910, box, 0.1)
    last = tc.arcs("shared_last", g, fp, 2, 1, 920, box, 0.04)
    want_first, want_last = traj_ref.score(g, fp, cost, first), traj_ref.score(g, fp, cost, last)
    want_middle = ref.score(g, fld, middle)
    assert first.tobytes() != middle[:3, :65].tobytes()
    hip, dptr = hip_runtime(), C.c_void_p()
    assert hip.hipMalloc(C.byref(dptr), middle.nbytes) == 0
    try:
        assert hip.hipMemcpy(dptr, middle.ctypes.data, middle.nbytes, 1) == 0   # hipMemcpyHostToDevice
        for dev in (None, dptr.value):
            s1, p1 = np.zeros(3, traj_ref.SCORE_DTYPE), np.full(3 * 65, 77, np.uint8)
            s2 = np.zeros(5, ref.SCORE_DTYPE)
            s3, p3 = np.zeros(2, traj_ref.SCORE_DTYPE), np.full(2, 77, np.uint8)
            h.score_trajectories_async(first, 3, 65, s1, p1)
            h.score_nav_async(None if dev else middle, 5, 130, s2, device_ptr=dev)
            h.score_trajectories_async(last, 2, 1, s3, p3)
            h.synchronize()
            for name in traj_ref.SCORE_DTYPE.names:
                assert np.array_equal(s1[name], want_first[0][name]), (dev is not None, "first", name, s1, want_first[0])
                assert np.array_equal(s3[name], want_last[0][name]), (dev is not None, "last", name, s3, want_last[0])
            for name in ref.SCORE_DTYPE.names:
                assert np.array_equal(s2[name], want_middle[name]), (dev is not None, "middle", name, s2, want_middle)
            assert p1.tobytes() == want_first[1].tobytes(), (dev is not None, "first", first_diff(p1, want_first[1]))
            assert p3.tobytes() == want_last[1].tobytes(), (dev is not None, "last", first_diff(p3, want_last[1]))
    finally:
        hip.hipFree(dptr)


# ------------------------------------------------------------------------------------------- ordering and state --
def _code(gvamd, call):
    with pytest.raises(gvamd.GVError) as e:
        call()
    return e.value.code


def test_snapshot_config_change_and_reset(gvamd):
    c1, c2 = nc.cases()["pocket_outside"], nc.cases()["comb_250x100"]
    g = nc.grid_of("250x100")
    h = _handle(gvamd, "250x100")
    poses = tc.families()["nonfinite_8x3"]["poses"]
    cost1 = plant(h, c1["mask"], c1["inflation"])
    f1, _ = _solve(h, g, cost1, (253, 0), c1["goal"])
    # a second gv_inflate of another map, a move and a changed configuration do not touch the field: it is a snapshot
    cost2 = plant(h, c2["mask"], c2["inflation"])
    assert cost2.tobytes() != cost1.tobytes()
    h.set_nav_config(254, 3)
    assert h.grid_move([0.0, 0.0, 0.0, 1.0, 3 * g.res, -2 * g.res, 0.0])["applied"]
    assert h.nav_field_array().tobytes() == f1.tobytes()
    assert h.score_nav(poses).tobytes() == ref.score(g, f1, poses).tobytes()
    # the next field is that of the costmap of the last gv_inflate (the move did not change it) and of the new configuration
    f2, _ = _solve(h, g, cost2, (254, 3), c1["goal"])
    assert f2.tobytes() != f1.tobytes()
    # a configuration change between two fields of one costmap
    c3 = nc.cases()["random_5e-4"]
    g5 = nc.grid_of("500x200")
    h5 = _handle(gvamd, "500x200")
    cost3 = plant(h5, c3["mask"], c3["inflation"])
    a, _ = _solve(h5, g5, cost3, (253, 0), c3["goal"])
    b, _ = _solve(h5, g5, cost3, (253, 3), c3["goal"])
    assert a.tobytes() != b.tobytes()
    # turned off: GV_ERR_STATE for the solver, the field stays readable
    h5.set_nav_config(None)
    assert _code(gvamd, lambda: h5.nav_field(c3["goal"])) == GV_ERR_STATE
    assert h5.nav_field_array().tobytes() == b.tobytes()
    # gv_reset invalidates the field and the costmap, and keeps the configuration
    h.reset()
    for call in (h.nav_field_array, h.device_nav_field, lambda: h.score_nav(poses), lambda: h.nav_field(c1["goal"])):
        assert _code(gvamd, call) == GV_ERR_STATE
    cost1b = plant(h, c1["mask"], c1["inflation"])
    info = h.nav_field(c1["goal"])
    assert info["n_seeds_used"] == 1 and h.nav_field_array().tobytes() == _want(g, cost1b, (254, 3), c1["goal"])[0].tobytes()
    assert h.device_nav_field()


def test_state_and_argument_rules(gvamd):
    (gx, gy, res), _ = nc.GRIDS["200x80"]
    h = gvamd.GridVisionHIP(gx, gy, res)
    lib = gvamd.load()
    g = nc.grid_of("200x80")
    c = nc.cases()["serpentine_200x80"]
    poses = np.zeros((2, 3, 3), np.float32)
    try:
        solve = lambda: h.nav_field(c["goal"])
        assert _code(gvamd, solve) == GV_ERR_STATE                    # no configuration, no costmap
        h.set_nav_config(253, 0)
        assert _code(gvamd, solve) == GV_ERR_STATE                    # a configuration, no gv_inflate yet
        assert _code(gvamd, h.nav_field_array) == GV_ERR_STATE and _code(gvamd, h.device_nav_field) == GV_ERR_STATE
        assert _code(gvamd, lambda: h.score_nav(poses)) == GV_ERR_STATE
        h.set_nav_config(None)
        cost = plant(h, c["mask"], c["inflation"])
        assert _code(gvamd, solve) == GV_ERR_STATE                    # a costmap, no configuration
        # a rejected configuration leaves the one in force alone
        h.set_nav_config(253, 3)
        for oc, w, fl in ((0, 0, 0), (256, 0, 0), (253, -1, 0), (253, 256, 0), (253, 0, 1)):
            assert _code(gvamd, lambda: h.set_nav_config(gvamd.NavConfig(oc, w, fl))) == GV_ERR_BAD_ARG
        h.nav_field(c["goal"])
        want = _want(g, cost, (253, 3), c["goal"])[0]
        assert h.nav_field_array().tobytes() == want.tobytes()
        # argument limits of gv_nav_field
        s = np.zeros((65537, 2), np.float32)
        nav = lambda seeds, S, inf=None: lib.gv_nav_field(h._h, seeds.ctypes.data_as(C.c_void_p) if seeds is not None else None,
                                                          C.c_int32(S), inf)
        assert nav(s, 0) == nav(s, -1) == nav(s, 65537) == nav(None, 1) == GV_ERR_BAD_ARG
        assert nav(np.ascontiguousarray(c["goal"]), 1) == 0           # info may be NULL
        assert lib.gv_get_nav_field(h._h, None) == GV_ERR_BAD_ARG and lib.gv_device_nav_field(h._h, None) == GV_ERR_BAD_ARG
        assert h.nav_field_array().tobytes() == want.tobytes()
        # ... and of gv_score_nav
        sc = np.full(6 * 4, 7, np.int32).view(ref.SCORE_DTYPE)

        def raw(K, P, flags=0, ps=poses, out=True):
            return lib.gv_score_nav(h._h, ps.ctypes.data_as(C.c_void_p) if ps is not None else None, C.c_int32(K), C.c_int32(P),
                                    C.c_uint32(flags), sc.ctypes.data_as(C.c_void_p) if out else None)

        assert raw(2, 0) == raw(2, 4097) == raw(-1, 3) == raw((1 << 20) + 1, 3) == GV_ERR_BAD_ARG
        assert raw(2, 3, flags=gvamd.TRAJ_KEEP_POSE_COST) == raw(2, 3, flags=4) == GV_ERR_BAD_ARG
        assert raw(2, 3, ps=None) == raw(2, 3, out=False) == GV_ERR_BAD_ARG
        assert raw(0, 3) == 0 and (sc.view(np.int32) == 7).all()      # K == 0: a successful no-op
        assert raw(2, 3) == 0 and sc[:2].tobytes() == ref.score(g, want, poses).tobytes()
        # the configuration is kept through gv_set_log_odds and gv_reset; gv_reset invalidates the field
        h.reset()
        assert _code(gvamd, h.nav_field_array) == GV_ERR_STATE
        cost = plant(h, c["mask"], c["inflation"])
        h.nav_field(c["goal"])
        assert h.nav_field_array().tobytes() == want.tobytes()
    finally:
        h.close()


def test_field_during_a_pending_tick(gvamd):
    """tick_enqueue, inflate, nav_field, tick_wait: the field is that of the tick's grid, as a twin handle computes it
    after its tick, not that of the grid before it"""
    P5 = (0.5, 1.1, 5.0, 80)
    hA, tfs = make_handle(gvamd, 2, perturbed=True)
    hB, _ = make_handle(gvamd, 2, perturbed=True)
    x, y, z, _, b = _ground_scene(tfs, seed=9)
    seeds = np.array([(40.0, 0.0), (10.0, 30.0), (-20.0, -15.0), (66.0, 0.0)], np.float32)
    try:
        for h in (hA, hB):
            h.upload_xyz(x, y, z)
            h.tick(b, k_near=4, lidar_bin=True)
            h.set_inflation(*P5)
            h.set_nav_config(253, 2)
        hB.inflate()
        hB.nav_field(seeds)
        before = hB.nav_field_array()
        hA.tick_enqueue(b, k_near=4, lidar_bin=True)
        hA.inflate()
        infoA = hA.nav_field(seeds)
        got = hA.nav_field_array()
        hA.tick_wait()
        hB.tick(b, k_near=4, lidar_bin=True)
        hB.inflate()
        infoB = hB.nav_field(seeds)
        want = hB.nav_field_array()
        assert want.tobytes() != before.tobytes()
        assert got.tobytes() == want.tobytes() and infoA["n_seeds_used"] == infoB["n_seeds_used"] >= 1
    finally:
        hA.close(); hB.close()


def test_nav_demo(gvamd, tmp_path):
    """examples/nav_demo.cpp (plain g++ over the C ABI): a wall with one gap, the goal behind it, a fan of 41 arcs scored
    for obstacles and for the distance to the goal; the arc through the gap wins, the straight one collides, and the
    demo's own host replay of every record finds no mismatch"""
    pkg = os.path.join(os.path.dirname(HERE), "grid-vision_amd")
    exe = str(tmp_path / "nav_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(pkg, "examples", "nav_demo.cpp"), "-o", exe,
                           "-L" + pkg, "-lgridvision_hip", "-Wl,-rpath," + pkg])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    m = re.search(r"trajectories 41 poses 40 collisions (\d+)\nfield rounds (\d+) seeds 1\n"
                  r"best (\d+) curvature (-?[\d.]+) goal_dist (\d+) through_gap yes\n"
                  r"straight first_collision (\d+) goal_dist (\d+)\nhost check ok \(0 mismatches\)", out.stdout)
    assert m, out.stdout
    collisions, rounds, best, curv, dist, straight, straight_dist = (float(v) for v in m.groups())
    assert 0 < collisions < 41 and rounds >= 2 and best != 20 and curv > 0    # the gap is to the left
    assert dist > straight_dist          # the straight arc ends nearer the goal -- behind the wall it ran into
