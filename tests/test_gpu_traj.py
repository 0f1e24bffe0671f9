"""[EXTENSION] X7 trajectory scoring on the device: gv_score_trajectories against traj_ref (one cell after the other, the
line as a loop) with zero tolerance.  Obstacles are planted with set_log_odds + update_map as test_gpu_inflate.py does,
inflated on the device, and the costmap() READBACK goes to the reference: the device is held to its own costmap, which
test_gpu_inflate.py pins.  Every comparison is tobytes() equality of the score records and of the pose costs, every call
is made three times with the same bytes.  Then the input and output paths (device poses, pinned and pageable
destinations), the ordering against pipelined frames, a pending tick, a footprint change and a second inflate, the state
rules of the header, and the example."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import traj_cases as tc
import traj_ref as ref
from gvamd import synth
from planner_util import first_diff, hip_runtime, plant
from test_gpu_parity import _ground_scene, make_handle

pytestmark = pytest.mark.gpu

GV_ERR_BAD_ARG, GV_ERR_STATE = 1, 5
HERE = os.path.dirname(os.path.abspath(__file__))
# (inscribed, inflation, scaling, threshold) per resolution; EXACT: only a lethal cell itself has a cost (d2max 0)
INFLATION = {0.1: (0.35, 0.55, 10.0, 65), 0.05: (0.12, 0.3, 8.0, 65)}
EXACT = (0.0, 0.0, 1.0, 65)
_RES = {size: geometry[2] for geometry, size in tc.GRIDS.values()}
_HANDLES = {}  # grid name -> handle, shared by the cases of the module
_CELLS = {}    # family -> traj_ref.all_cells: they do not depend on the costmap


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    yield m
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()
    _CELLS.clear()


def _handle(gvamd, grid):
    if grid not in _HANDLES:
        (gx, gy, res), (nx, ny) = tc.GRIDS[grid]
        h = gvamd.GridVisionHIP(gx, gy, res)
        assert (h.nx, h.ny) == (nx, ny)
        _HANDLES[grid] = h
    h = _HANDLES[grid]
    h.reset()
    return h


def _plant(h, mask, inflation=None):
    """planner_util.plant with the module's inflation for the grid's resolution unless one is given"""
    return plant(h, mask, inflation or INFLATION[_RES[(h.nx, h.ny)]])


def _want(name, cost, collision=253, off_map=255):
    f = tc.families()[name]
    g, fp = tc.grid_of(f["grid"]), tc.fp_of(f["fp"], collision, off_map)
    if name not in _CELLS:
        _CELLS[name] = ref.all_cells(g, fp, f["poses"])
    return ref.score(g, fp, cost, f["poses"], _CELLS[name])


def _check(h, name, cost, collision=253, off_map=255, tag=""):
    """score three times with and without the pose costs; records and pose costs equal the reference byte for byte"""
    f = tc.families()[name]
    want_s, want_p = _want(name, cost, collision, off_map)
    h.set_footprint(tc.FOOTPRINTS[f["fp"]], collision, off_map)
    for rep in range(3):
        got_s, got_p = h.score_trajectories(f["poses"], keep_pose_cost=True)
        assert got_p.dtype == np.uint8 and got_p.tobytes() == want_p.tobytes(), (name, tag, rep, "pose_cost", first_diff(got_p, want_p))
        assert got_s.dtype == ref.SCORE_DTYPE and got_s.tobytes() == want_s.tobytes(), (name, tag, rep, first_diff(got_s, want_s))
        only = h.score_trajectories(f["poses"])
        assert only.tobytes() == want_s.tobytes(), (name, tag, rep, "without pose costs")
    return want_s, want_p


def _random_mask(nx, ny, density, seed):
    return np.random.default_rng(seed).random((ny, nx)) < density


FAMILIES = ["rect_3x130", "triangle_64x63", "point_257x2", "poly16_65x1", "tiny_1x64", "rect_3x65_fine", "long_3x2",
            "long_steep_1x2", "border_in_from_+x", "border_in_from_-x", "border_in_from_+y", "border_in_from_-y",
            "border_canary", "border_point", "border_diamond", "leaving_3x64", "nonfinite_8x3", "nonfinite_point_8x3"]


def test_every_family_is_scored():
    assert sorted(FAMILIES) == sorted(tc.families())


@pytest.mark.parametrize("density", [5e-4, 0.3])
@pytest.mark.parametrize("name", FAMILIES)
def test_random_masks(gvamd, name, density):
    h = _handle(gvamd, tc.families()[name]["grid"])
    cost = _plant(h, _random_mask(h.nx, h.ny, density, seed=17))
    s, p = _check(h, name, cost, tag=density)
    if density == 0.3 and name in ("rect_3x130", "triangle_64x63", "long_3x2"):
        assert (s["first_collision"] >= 0).any() and s["max_cost"].min() >= 254   # 255: a pose that left the map
    if name == "leaving_3x64":
        assert s["n_off_map"].tolist() == [64, 33, 1]
    if name.startswith("nonfinite"):
        # with the point footprint a NaN or infinite yaw is never read: trajectories 6 and 7 stay on the map
        assert s["n_off_map"].tolist() == ([0] + [1] * 7 if name == "nonfinite_8x3" else [0] + [1] * 5 + [0, 0])


@pytest.mark.parametrize("name", ["rect_3x130", "poly16_65x1", "rect_3x65_fine", "point_257x2"])
def test_row_empty_and_full(gvamd, name):
    h = _handle(gvamd, tc.families()[name]["grid"])
    row = np.zeros((h.ny, h.nx), bool)
    row[h.ny // 2 - 3, :] = True
    _check(h, name, _plant(h, row), tag="row")
    s, p = _check(h, name, _plant(h, np.zeros((h.ny, h.nx), bool)), tag="empty")
    on = s["n_off_map"] == 0
    assert (s["max_cost"][on] == 0).all() and (s["first_collision"][on] == -1).all() and (s["cost_sum"][on] == 0).all()
    s, p = _check(h, name, _plant(h, np.ones((h.ny, h.nx), bool)), tag="full")
    assert (s["max_cost"] >= 254).all() and (s["first_collision"] == 0).all()


@pytest.mark.parametrize("collision", [253, 254, 255])
@pytest.mark.parametrize("off_map", [0, 255])
def test_thresholds(gvamd, collision, off_map):
    h = _handle(gvamd, "500x200")
    cost = _plant(h, _random_mask(h.nx, h.ny, 2e-3, seed=23))
    assert {253, 254} <= set(cost.tolist())
    s, _ = _check(h, "triangle_64x63", cost, collision, off_map, tag=(collision, off_map))
    l, _ = _check(h, "leaving_3x64", cost, collision, off_map, tag=(collision, off_map))
    if collision == 255:     # no cell costs 255: only an off-map pose of cost 255 collides
        assert (s["first_collision"][s["n_off_map"] == 0] == -1).all()
        assert l["first_collision"].tolist() == ([0, 31, 63] if off_map == 255 else [-1, -1, -1])
    if collision == 253:
        assert (s["first_collision"] >= 0).any()


def test_outline_ends_and_interior(gvamd):
    """one lethal cell, only it has a cost (d2max 0): on the outline's first cell (vertex 0's cell, also the last cell of
    the closing edge), on the cells next to it at either end of the outline, which only one outline index touches, on
    the last cell of edge 0, and strictly inside the footprint, where it must not count"""
    h = _handle(gvamd, "500x200")
    g, fp = tc.grid_of("500x200"), tc.fp_of("rect")
    pose = np.array([[(12.03, 1.04, 0.4)]], np.float32)
    assert tc.guard_violations(g, fp, pose) == []
    cells = ref.pose_cells(g, fp, *pose[0, 0])
    n0 = len(ref.line(*ref.pose_edges(g, fp, *pose[0, 0])[0]))
    inside = ref.get_index(g, 12.03 + 1.2, 1.04 + 0.5)        # 1.3 m ahead of the origin: inside the 4.5 m x 2 m outline
    inside = inside[1] * g.nx + inside[0]
    assert inside not in cells and cells[1] == cells[-1] and cells.count(cells[2]) == 1 and cells.count(cells[-2]) == 1
    h.set_footprint(fp.vertices, 253, 255)
    for tag, cell, hit in (("first = last", cells[1], True), ("second", cells[2], True), ("last but one", cells[-2], True),
                           ("end of edge 0", cells[n0], True), ("centre", cells[0], True), ("inside", inside, False)):
        mask = np.zeros(g.nx * g.ny, bool)
        mask[g.nx * g.ny - 1 - cell] = True
        cost = _plant(h, mask.reshape(g.ny, g.nx), EXACT)
        assert int((cost != 0).sum()) == 1
        want_s, want_p = ref.score(g, fp, cost, pose)
        for _ in range(3):
            got_s, got_p = h.score_trajectories(pose, keep_pose_cost=True)
            assert got_s.tobytes() == want_s.tobytes() and got_p.tobytes() == want_p.tobytes(), tag
        assert int(got_s["max_cost"][0]) == (254 if hit else 0) and int(got_s["first_collision"][0]) == (0 if hit else -1), tag
        assert int(got_s["cost_sum"][0]) == (254 if tag == "centre" else 0), tag


@pytest.mark.parametrize("name", ["rect_3x130", "triangle_64x63", "poly16_65x1"])
def test_device_poses_and_destinations(gvamd, name):
    """poses read in place from a hipMalloc buffer, results into pinned memory (written by the kernel) and into pageable
    memory (the copy command), pinned poses: the same bytes every way"""
    f = tc.families()[name]
    h = _handle(gvamd, f["grid"])
    cost = _plant(h, _random_mask(h.nx, h.ny, 0.02, seed=31))
    want_s, want_p = _want(name, cost)
    h.set_footprint(tc.FOOTPRINTS[f["fp"]])
    poses = f["poses"]
    K, P = poses.shape[:2]
    hip, dptr = hip_runtime(), C.c_void_p()
    assert hip.hipMalloc(C.byref(dptr), poses.nbytes) == 0
    pin_s, pin_p, pin_in = gvamd.PinnedI8(K * 16 + 16), gvamd.PinnedI8(K * P), gvamd.PinnedF32(poses.size)
    try:
        assert hip.hipMemcpy(dptr, poses.ctypes.data, poses.nbytes, 1) == 0   # hipMemcpyHostToDevice
        pin_in.array[:] = poses.reshape(-1)
        for rep in range(3):
            got_s, got_p = h.score_trajectories(poses, keep_pose_cost=True, device_ptr=dptr.value)
            assert got_s.tobytes() == want_s.tobytes() and got_p.tobytes() == want_p.tobytes(), ("device poses", rep)
            for src, dev in ((pin_in.array, None), (poses, None), (None, dptr.value)):
                scores = pin_s.array[:K * 16].view(ref.SCORE_DTYPE)
                pin_s.array[:] = 77
                pin_p.array[:] = 77
                h.score_trajectories_async(src, K, P, scores, pin_p.array.view(np.uint8), device_ptr=dev)
                h.synchronize()
                assert scores.tobytes() == want_s.tobytes() and pin_p.array.tobytes() == want_p.tobytes(), ("pinned", rep)
                odd = pin_s.array[8:8 + K * 16].view(ref.SCORE_DTYPE)      # pinned, not 16-byte aligned: the copy command
                h.score_trajectories_async(src, K, P, odd, None, device_ptr=dev)
                h.synchronize()
                assert odd.tobytes() == want_s.tobytes(), ("pinned, unaligned", rep)
    finally:
        hip.hipFree(dptr)
        for p in (pin_s, pin_p, pin_in):
            p.close()


# ------------------------------------------------------------------------------------------------------ ordering --
P5 = (0.5, 1.1, 5.0, 80)   # on 0.2 m cells; threshold 80: a cell the lidar hit is lethal after two updates, not after one


def _big_family(K, P, seed):
    cfg = synth.CONFIGS[2]["grid"]
    assert cfg.resolution == 0.2
    g, fp = ref.grid(cfg.grid_x, cfg.grid_y, cfg.resolution), tc.fp_of("rect")
    poses = tc.arcs("ordering", g, fp, K, P, seed, (g.pos_x - 60.0, g.pos_x + 60.0, -60.0, 60.0), 0.5)
    return g, fp, poses


def _pinned_out(gvamd, K, P):
    ps, pp = gvamd.PinnedI8(K * 16), gvamd.PinnedI8(K * P)
    ps.array[:] = 77
    pp.array[:] = 77
    return ps, pp


def test_score_between_pipelined_frames(gvamd):
    """A: frame 1, inflate, score into buffers 1, frame 2 (other detections), inflate, score into buffers 2, one
    synchronize.  B: the two frames one by one.  Each result is the reference of its own costmap."""
    hA, _ = make_handle(gvamd, 2)
    hB, _ = make_handle(gvamd, 2)
    g, fp, traj = _big_family(65, 20, 900)
    K, P = traj.shape[:2]
    x, y, z, _ = synth.cloud_uniform(2)
    flags = gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH
    poses = [synth.lshape_poses(2, 12, seed_extra=1), synth.lshape_poses(2, 30, seed_extra=2)]
    outs = [_pinned_out(gvamd, K, P) for _ in range(2)]
    try:
        for h in (hA, hB):
            h.upload_xyz(x, y, z)
            h.set_inflation(*P5)
            h.set_footprint(fp.vertices)
        costs = []
        for i in range(2):
            hA.set_detections_async(flags, poses=poses[i])
            hA.enqueue_frame()
            hA.inflate()
            hA.score_trajectories_async(traj, K, P, outs[i][0].array.view(ref.SCORE_DTYPE), outs[i][1].array.view(np.uint8))
            hB.set_detections(flags, poses=poses[i])
            hB.enqueue_frame()
            hB.synchronize()
            hB.inflate()
            costs.append(hB.costmap())
        hA.synchronize()
        cells = ref.all_cells(g, fp, traj)
        want = [ref.score(g, fp, c, traj, cells) for c in costs]
        assert want[0][0].tobytes() != want[1][0].tobytes() and want[0][1].tobytes() != want[1][1].tobytes()
        for i in range(2):
            assert outs[i][0].array.tobytes() == want[i][0].tobytes(), i
            assert outs[i][1].array.tobytes() == want[i][1].tobytes(), i
    finally:
        for o in outs:
            o[0].close(); o[1].close()
        hA.close(); hB.close()


def test_score_during_a_pending_tick(gvamd):
    """tick_enqueue, inflate, score, tick_wait: the scores are those of the tick's grid, not of the grid before it"""
    hA, tfs = make_handle(gvamd, 2, perturbed=True)
    hB, _ = make_handle(gvamd, 2, perturbed=True)
    g, fp, traj = _big_family(65, 20, 950)
    K, P = traj.shape[:2]
    x, y, z, _, b = _ground_scene(tfs, seed=9)
    ps, pp = _pinned_out(gvamd, K, P)
    try:
        for h in (hA, hB):
            h.upload_xyz(x, y, z)
            h.tick(b, k_near=4, lidar_bin=True)
            h.set_inflation(*P5)
            h.set_footprint(fp.vertices)
        hB.inflate()
        before = hB.costmap()
        hA.tick_enqueue(b, k_near=4, lidar_bin=True)
        hA.inflate()
        hA.score_trajectories_async(traj, K, P, ps.array.view(ref.SCORE_DTYPE), pp.array.view(np.uint8))
        hA.tick_wait()
        hA.synchronize()
        hB.tick(b, k_near=4, lidar_bin=True)
        hB.inflate()
        cost = hB.costmap()
        cells = ref.all_cells(g, fp, traj)
        want, stale = ref.score(g, fp, cost, traj, cells), ref.score(g, fp, before, traj, cells)
        assert want[1].tobytes() != stale[1].tobytes()
        assert ps.array.tobytes() == want[0].tobytes() and pp.array.tobytes() == want[1].tobytes()
    finally:
        ps.close(); pp.close()
        hA.close(); hB.close()


def test_footprint_change_and_second_inflate_in_flight(gvamd):
    """score, set_footprint, score, set_inflation, inflate, score -- enqueued back to back, one synchronize: every call
    keeps the footprint it was enqueued with and reads the costmap of the inflate before it"""
    h = _handle(gvamd, "500x200")
    g = tc.grid_of("500x200")
    traj = tc.families()["rect_3x130"]["poses"]
    K, P = traj.shape[:2]
    mask = _random_mask(h.nx, h.ny, 3e-3, seed=41)
    second = (0.52, 3.03, 3.0, 65)
    cost2 = _plant(h, mask, second)
    cost1 = _plant(h, mask)
    assert cost1.tobytes() != cost2.tobytes()
    rect, tri = tc.fp_of("rect"), tc.fp_of("triangle", 200, 7)
    outs = [_pinned_out(gvamd, K, P) for _ in range(3)]
    try:
        def enqueue(i):
            h.score_trajectories_async(traj, K, P, outs[i][0].array.view(ref.SCORE_DTYPE), outs[i][1].array.view(np.uint8))
        h.set_footprint(rect.vertices, rect.collision_cost, rect.off_map_cost)
        enqueue(0)
        h.set_footprint(tri.vertices, tri.collision_cost, tri.off_map_cost)
        enqueue(1)
        h.set_inflation(*second)
        h.inflate()
        enqueue(2)
        h.synchronize()
        want = [ref.score(g, rect, cost1, traj), ref.score(g, tri, cost1, traj), ref.score(g, tri, cost2, traj)]
        assert len({w[1].tobytes() for w in want}) == 3
        for i in range(3):
            assert outs[i][0].array.tobytes() == want[i][0].tobytes(), i
            assert outs[i][1].array.tobytes() == want[i][1].tobytes(), i
    finally:
        for o in outs:
            o[0].close(); o[1].close()


def test_state_rules(gvamd):
    (gx, gy, res), _ = tc.GRIDS["250x100"]
    h = gvamd.GridVisionHIP(gx, gy, res)
    g, tri = tc.grid_of("250x100"), tc.fp_of("triangle")
    traj = tc.families()["nonfinite_8x3"]["poses"]
    lib = gvamd.load()

    def code(call):
        with pytest.raises(gvamd.GVError) as e:
            call()
        return e.value.code

    def raw(K, P, flags=0, poses=traj, scores=True, pose_cost=None):
        sc = np.full(max(K, 1) if 0 < K < 100 else 1, 7, np.int32).repeat(4).view(ref.SCORE_DTYPE)
        rc = lib.gv_score_trajectories(h._h, poses.ctypes.data_as(C.c_void_p) if poses is not None else None, C.c_int32(K),
                                       C.c_int32(P), C.c_uint32(flags), sc.ctypes.data_as(C.c_void_p) if scores else None,
                                       pose_cost)
        return rc, sc

    try:
        score = lambda: h.score_trajectories(traj)
        mask = _random_mask(h.nx, h.ny, 0.05, seed=5)
        assert code(score) == GV_ERR_STATE                          # no footprint, no costmap
        h.set_footprint(tri.vertices)
        assert code(score) == GV_ERR_STATE                          # a footprint, no gv_inflate yet
        h.set_footprint(None)
        cost = _plant(h, mask)
        assert code(score) == GV_ERR_STATE                          # a costmap, no footprint
        h.set_footprint(tri.vertices)
        want = ref.score(g, tri, cost, traj)[0]
        assert score().tobytes() == want.tobytes()
        # a rejected footprint leaves the one in force alone
        for bad in (tri.vertices[:2], tri.vertices[:1], ((float("nan"), 0.0),) + tri.vertices[1:]):
            assert code(lambda: h.set_footprint(bad)) == GV_ERR_BAD_ARG
        for cc, oc in ((0, 255), (256, 255), (253, -1), (253, 256)):
            assert code(lambda: h.set_footprint(tri.vertices, cc, oc)) == GV_ERR_BAD_ARG
        f = gvamd.Footprint.of(tri.vertices, flags=2)
        assert code(lambda: h.set_footprint(f)) == GV_ERR_BAD_ARG
        f = gvamd.Footprint.of(tc.FOOTPRINTS["poly16"])
        f.n_vertices = 17
        assert code(lambda: h.set_footprint(f)) == GV_ERR_BAD_ARG
        assert score().tobytes() == want.tobytes()
        # argument limits
        assert raw(8, 0)[0] == raw(8, 4097)[0] == raw(-1, 3)[0] == raw((1 << 20) + 1, 3)[0] == GV_ERR_BAD_ARG
        assert raw(8, 3, flags=4)[0] == raw(8, 3, flags=ref.KEEP_POSE_COST)[0] == GV_ERR_BAD_ARG
        assert raw(8, 3, poses=None)[0] == raw(8, 3, scores=False)[0] == GV_ERR_BAD_ARG
        rc, sc = raw(0, 3)                                          # K == 0: a successful no-op
        assert rc == 0 and (sc.view(np.int32) == 7).all()
        rc, sc = raw(8, 3)
        assert rc == 0 and sc.tobytes() == want.tobytes()
        # the footprint is kept through gv_set_log_odds, gv_grid_move and gv_reset; gv_reset invalidates the costmap
        cost_b = _plant(h, np.zeros((h.ny, h.nx), bool))            # the empty map: other scores than `want`
        assert score().tobytes() == ref.score(g, tri, cost_b, traj)[0].tobytes() != want.tobytes()
        assert h.grid_move([0.0, 0.0, 0.0, 1.0, 3 * res, -2 * res, 0.0])["applied"]
        assert score().tobytes() == ref.score(g, tri, cost_b, traj)[0].tobytes()   # the costmap is a snapshot
        h.inflate()
        assert score().tobytes() == ref.score(g, tri, h.costmap(), traj)[0].tobytes()
        h.reset()
        assert code(score) == GV_ERR_STATE
        cost_c = _plant(h, mask)
        assert score().tobytes() == ref.score(g, tri, cost_c, traj)[0].tobytes()
        h.set_footprint(None)
        assert code(score) == GV_ERR_STATE
    finally:
        h.close()


def test_planner_demo(gvamd, tmp_path):
    """examples/planner_demo.cpp (plain g++ over the C ABI): ticks of the flow with inflate_costmap, a fan of 41 arcs
    scored on the device, the best one picked, and the demo's own host replay of every record"""
    pkg = os.path.join(os.path.dirname(HERE), "grid-vision_amd")
    exe = str(tmp_path / "planner_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(pkg, "examples", "planner_demo.cpp"), "-o", exe,
                           "-L" + pkg, "-lgridvision_hip", "-Wl,-rpath," + pkg])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    m = re.search(r"trajectories 41 poses 40 collisions (\d+)\nbest (\d+) curvature (-?[\d.]+) cost_sum (\d+) max_cost (\d+)\n"
                  r"straight first_collision (-?\d+) max_cost (\d+)\nhost check ok \(0 mismatches\)", out.stdout)
    assert m, out.stdout
    collisions, best, curv, cost_sum, max_cost, straight, straight_max = (float(v) for v in m.groups())
    assert 0 < collisions < 41 and max_cost < 253 and best != 20        # some arcs pass the wall, the straight one does not
    assert straight >= 0 and straight_max >= 253
