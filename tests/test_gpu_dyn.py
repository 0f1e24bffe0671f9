"""[EXTENSION] X13 scoring against predicted moving objects on the device.

gv_score_dynamic against dyn_ref (the header's text with Python floats) and against the library's host twin on every
family of dyn_cases: the exact families (every off_x 0, or every yaw exactly 0) by tobytes(), min_dist2 included; the
general-yaw families after dyn_cases' guard -- the integer fields and the pose costs exactly, min_dist2 within
dyn_ref.DIST_TOL * (1 + d2), nearest_object where the runner-up is farther than that.  Every scoring call is made three
times and returns the same bytes.

Paths: device poses, pinned aligned / pinned misaligned / pageable destinations, the stream order of
gv_set_moving_objects and of a configuration change between two asynchronous scorings, a pending tick, the state and
argument rules.

Control step and MPPI: unset against a handle that never heard of X13, set with zero objects, with objects against
gv_control_select_dyn over the three device records and against dyn_ref; gv_mppi_cycle against its three calls."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dyn_cases as dc
import dyn_ref as ref
import rollout_ref
import traj_cases as tc
from planner_util import first_diff, hip_runtime, plant
from test_gpu_parity import _ground_scene, make_handle

pytestmark = pytest.mark.gpu

GV_ERR_BAD_ARG, GV_ERR_STATE = 1, 5
GRID = "500x200"
INFLATION = (0.35, 0.55, 10.0, 65)      # test_gpu_rollout.INFLATION[0.1]
SEEDS = np.array([(30.0 - 0.5 * i, -2.0 + 0.1 * i) for i in range(40)], np.float32)   # test_gpu_rollout.SEEDS
FAN_START, FAN_DT = (2.0, 0.3, 0.1), 0.25
W = rollout_ref.weights
_HANDLES = {}


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    yield m
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()


def _handle(gvamd, name="main"):
    """a 500 x 200 handle, X13 switched off and its set emptied"""
    if name not in _HANDLES:
        (gx, gy, res), (nx, ny) = tc.GRIDS[GRID]
        _HANDLES[name] = gvamd.GridVisionHIP(gx, gy, res)
    h = _HANDLES[name]
    h.set_dyn_config(None)
    h.set_moving_objects(None)
    return h


def _code(gvamd, call):
    with pytest.raises(gvamd.GVError) as e:
        call()
    return e.value.code


def _cw(gvamd, w, flags=0):
    return gvamd.CriticWeights(*[w[n] for n in rollout_ref.WEIGHTS], flags)


def _by_name(name):
    return next(c for c in dc.cases(True) + dc.cases(False) if c["name"] == name)


def _setup(h, gvamd, c):
    h.set_dyn_config(ref.to_struct(gvamd, c["cfg"]))
    h.set_moving_objects(c["objs"])


# ------------------------------------------------------------------------------------------------------- scoring --
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "general"])
def test_device_equals_reference_and_host_twin(gvamd, exact):
    h = _handle(gvamd)
    for c in dc.cases(exact):
        r = dc.want(c)
        if not exact:
            assert c["redrawn"] <= 0.01 * c["poses"].shape[0], (c["name"], c["redrawn"])
        _setup(h, gvamd, c)
        first = None
        for rep in range(3):
            scores, pc = h.score_dynamic(c["poses"], keep_pose_cost=True)
            if first is None:
                first = (scores.tobytes(), pc.tobytes())
                dc.compare(c, r, scores, pc, "device")
            assert (scores.tobytes(), pc.tobytes()) == first, (c["name"], rep, "the same call, other bytes")
            assert h.score_dynamic(c["poses"]).tobytes() == first[0], (c["name"], rep, "without the pose costs")
        if exact:
            twin, twin_pc = gvamd.dyn_score_poses(ref.to_struct(gvamd, c["cfg"]), c["objs"], c["poses"], keep_pose_cost=True)
            assert (twin.tobytes(), twin_pc.tobytes()) == first, (c["name"], first_diff(np.frombuffer(first[1], np.uint8), twin_pc))


def test_arrival_and_identical_objects_on_the_device(gvamd):
    h = _handle(gvamd)
    c = _by_name("arrives_at_37")
    _setup(h, gvamd, c)
    s = h.score_dynamic(c["poses"])
    assert s["first_collision"][0] == 37 and s["max_cost"][0] == 254 and s["nearest_object"][0] == 0
    c = _by_name("identical_objects")
    _setup(h, gvamd, c)
    assert (h.score_dynamic(c["poses"])["nearest_object"] == 2).all()
    c = _by_name("no_objects")
    _setup(h, gvamd, c)
    s = h.score_dynamic(c["poses"])
    assert s.tobytes() == np.array([(0, -1, 0, -1, np.inf)] * 3, ref.SCORE_DTYPE).tobytes()


@pytest.mark.parametrize("name", ["n128_two_circles", "general_K65_P65_n1", "nonfinite"])
def test_device_poses_and_destinations(gvamd, name):
    """poses read in place from a hipMalloc buffer; records into pinned memory aligned to 8 bytes (written by the kernel),
    into pinned memory that is not (the copy command) and into pageable memory: the same bytes every way"""
    h = _handle(gvamd)
    c = _by_name(name)
    dc.want(c)
    _setup(h, gvamd, c)
    poses = c["poses"]
    K, P = poses.shape[:2]
    want_s, want_p = h.score_dynamic(poses, keep_pose_cost=True)
    hip, dptr = hip_runtime(), C.c_void_p()
    assert hip.hipMalloc(C.byref(dptr), poses.nbytes) == 0
    pin_s, pin_p, pin_in = gvamd.PinnedI8(K * 24 + 16), gvamd.PinnedI8(K * P + 8), gvamd.PinnedF32(poses.size)
    try:
        assert hip.hipMemcpy(dptr, poses.ctypes.data, poses.nbytes, 1) == 0   # hipMemcpyHostToDevice
        pin_in.array[:] = poses.reshape(-1)
        for rep in range(3):
            got_s, got_p = h.score_dynamic(poses, keep_pose_cost=True, device_ptr=dptr.value)
            assert got_s.tobytes() == want_s.tobytes() and got_p.tobytes() == want_p.tobytes(), ("device poses", rep)
            for off_s, off_p in ((0, 0), (8, 1), (4, 3), (12, 0)):
                pin_s.array[:] = 77
                pin_p.array[:] = 77
                s = pin_s.array[off_s:off_s + K * 24].view(ref.SCORE_DTYPE)
                p = pin_p.array[off_p:off_p + K * P].view(np.uint8)
                h.score_dynamic_async(pin_in.array.reshape(K, P, 3), K, P, s, p)
                h.synchronize()
                assert s.tobytes() == want_s.tobytes() and p.tobytes() == want_p.tobytes(), ("pinned", rep, off_s, off_p)
                pin_s.array[:] = 77
                pin_p.array[:] = 77
                h.score_dynamic_async(None, K, P, s, device_ptr=dptr.value)
                h.synchronize()
                assert s.tobytes() == want_s.tobytes() and (pin_p.array == 77).all(), ("no pose costs without the flag", rep)
            s, p = np.zeros(K, ref.SCORE_DTYPE), np.full(K * P, 7, np.uint8)
            h.score_dynamic_async(poses, K, P, s, p)
            h.synchronize()
            assert s.tobytes() == want_s.tobytes() and p.tobytes() == want_p.tobytes(), ("pageable", rep)
    finally:
        hip.hipFree(dptr)
        for q in (pin_s, pin_p, pin_in):
            q.close()


def test_set_and_configuration_are_stream_ordered(gvamd):
    """score, gv_set_moving_objects, score, gv_set_dyn_config, score, both again, score -- enqueued back to back, one
    synchronize: every scoring keeps the set and the configuration (and its table) it was enqueued with"""
    h = _handle(gvamd)
    a, b = _by_name("dt_zero"), _by_name("general_K3_P257_n64")
    poses = a["poses"]
    K, P = poses.shape[:2]
    cfg2 = dict(a["cfg"], radius=0.25, influence_radius=2.5, quantum=0.05, t0=0.5, dt=0.05, off_x=(0.0,))
    objs3 = dc.random_objects(np.random.default_rng(77), 5)
    steps = [(a["cfg"], a["objs"]), (a["cfg"], b["objs"]), (cfg2, b["objs"]), (a["cfg"], objs3), (cfg2, dc.objects(np.zeros((0, 7))))]
    want = [ref.score(cfg, objs, poses) for cfg, objs in steps]
    assert len({w["scores"].tobytes() for w in want}) == len(steps)
    pins = [(gvamd.PinnedI8(K * 24), gvamd.PinnedI8(K * P)) for _ in steps]
    try:
        for rep in range(2):
            for ps, pp in pins:
                ps.array[:] = 77
                pp.array[:] = 77
            for (cfg, objs), (ps, pp) in zip(steps, pins):
                h.set_dyn_config(ref.to_struct(gvamd, cfg))
                h.set_moving_objects(objs)
                h.score_dynamic_async(poses, K, P, ps.array.view(ref.SCORE_DTYPE), pp.array)
            h.set_dyn_config(None)                   # does not reach what is enqueued
            h.synchronize()
            for i, (w, (ps, pp)) in enumerate(zip(want, pins)):
                assert ps.array.tobytes() == w["scores"].tobytes(), (rep, i)
                assert pp.array.tobytes() == w["pose_cost"].tobytes(), (rep, i)
    finally:
        for ps, pp in pins:
            ps.close(); pp.close()


def test_scoring_during_a_pending_tick(gvamd):
    h, tfs = make_handle(gvamd, 2, perturbed=True)
    c = _by_name("dt_zero")
    want = dc.want(c)
    x, y, z, _, b = _ground_scene(tfs, seed=9)
    K, P = c["poses"].shape[:2]
    ps = gvamd.PinnedI8(K * 24)
    try:
        h.upload_xyz(x, y, z)
        h.tick(b, k_near=4, lidar_bin=True)
        ps.array[:] = 77
        h.tick_enqueue(b, k_near=4, lidar_bin=True)
        _setup(h, gvamd, c)
        h.score_dynamic_async(c["poses"], K, P, ps.array.view(ref.SCORE_DTYPE))
        sync = h.score_dynamic(c["poses"])
        h.tick_wait()
        h.synchronize()
        assert ps.array.tobytes() == want["scores"].tobytes() == sync.tobytes()
    finally:
        ps.close()
        h.close()


# --------------------------------------------------------------------------------------------------------- rules --
def test_state_and_argument_rules(gvamd):
    import test_dyn_host as th
    h = _handle(gvamd, "rules")
    lib = h._lib
    c = _by_name("dt_zero")
    poses = c["poses"]
    K, P = poses.shape[:2]
    scores, pc = np.zeros(K, ref.SCORE_DTYPE), np.zeros(K * P, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None

    def raw(fn, hh=h, src=poses, k=K, pp=P, flags=0, s=scores, cost=None):
        return fn(hh._h if hh else None, p(src), C.c_int32(k), C.c_int32(pp), C.c_uint32(flags), p(s), p(cost))

    # the state after gv_create: no configuration, no objects; GV_ERR_STATE from both forms, K == 0 included
    for fn in (lib.gv_score_dynamic, lib.gv_score_dynamic_async):
        assert raw(fn) == GV_ERR_STATE and raw(fn, k=0) == GV_ERR_STATE
    assert "gv_set_dyn_config" in lib.gv_last_error(h._h).decode()
    h.set_moving_objects(c["objs"])                         # allowed without a configuration
    h.set_dyn_config(ref.to_struct(gvamd, c["cfg"]))
    want = dc.want(c)["scores"]
    assert h.score_dynamic(poses).tobytes() == want.tobytes()
    for fn in (lib.gv_score_dynamic, lib.gv_score_dynamic_async):
        assert raw(fn, k=0) == 0                            # a no-op
        assert raw(fn, hh=None) == raw(fn, src=None) == raw(fn, s=None) == GV_ERR_BAD_ARG
        assert raw(fn, pp=0) == raw(fn, pp=4097) == raw(fn, k=-1) == raw(fn, k=(1 << 20) + 1) == GV_ERR_BAD_ARG
        assert raw(fn, flags=4) == raw(fn, flags=gvamd.TRAJ_KEEP_POSE_COST) == GV_ERR_BAD_ARG   # unknown flag; the flag without pose_cost
        assert raw(fn, flags=gvamd.TRAJ_KEEP_POSE_COST, cost=pc) == 0
    h.synchronize()
    # a rejected configuration or set leaves the one in force alone
    assert lib.gv_set_dyn_config(None, C.byref(ref.to_struct(gvamd, c["cfg"]))) == GV_ERR_BAD_ARG
    for bad in th._bad_configs():
        assert lib.gv_set_dyn_config(h._h, C.byref(ref.to_struct(gvamd, dict(c["cfg"], **bad)))) == GV_ERR_BAD_ARG, bad
    objs = c["objs"]
    assert lib.gv_set_moving_objects(None, p(objs), C.c_int32(1)) == GV_ERR_BAD_ARG
    assert lib.gv_set_moving_objects(h._h, None, C.c_int32(1)) == lib.gv_set_moving_objects(h._h, p(objs), C.c_int32(-1)) == GV_ERR_BAD_ARG
    big = dc.random_objects(np.random.default_rng(1), 129)
    assert lib.gv_set_moving_objects(h._h, p(big), C.c_int32(129)) == GV_ERR_BAD_ARG
    for f, v in (("px", np.nan), ("qw", np.inf), ("length", -1.0), ("width", np.nan)):
        o = objs.copy(); o["pose"][f][3] = v
        assert lib.gv_set_moving_objects(h._h, p(o), C.c_int32(len(o))) == GV_ERR_BAD_ARG, f
    o = objs.copy(); o["vy"][0] = -np.inf
    assert lib.gv_set_moving_objects(h._h, p(o), C.c_int32(len(o))) == GV_ERR_BAD_ARG
    assert h.score_dynamic(poses).tobytes() == want.tobytes()
    # both are kept through gv_reset; NULL turns the configuration off, and setting it again finds the set still there
    h.reset()
    assert h.score_dynamic(poses).tobytes() == want.tobytes()
    h.set_dyn_config(None)
    assert _code(gvamd, lambda: h.score_dynamic(poses)) == GV_ERR_STATE
    h.set_dyn_config(ref.to_struct(gvamd, c["cfg"]))
    assert h.score_dynamic(poses).tobytes() == want.tobytes()
    for g in th.GOOD_EDGES:
        h.set_dyn_config(ref.to_struct(gvamd, dict(c["cfg"], **g)))
    h.set_moving_objects(big[:128])
    h.set_moving_objects(None)
    assert (h.score_dynamic(poses)["nearest_object"] == -1).all()


# -------------------------------------------------------------------------------------- control step and MPPI --
def _fan(K, seed):
    rng = np.random.default_rng(seed)
    u = np.zeros((K, 2), np.float32)
    u[:, 0] = rng.uniform(0.5, 6.0, K)
    u[:, -1] = rng.uniform(-0.6, 0.6, K)
    return u


CONTROL_OBJS = [(12.0, -6.0, np.pi / 2, 4.5, 2.0, 0.0, 3.0), (6.0, 4.0, 0.3, 2.0, 1.0, 0.5, -1.5), (20.0, 2.0, -0.4, 4.5, 2.0, -2.0, 0.2)]


def _control_cfg(w_sum, w_max=0):
    return ref.config(off_x=(0.0,), radius=0.4, influence_radius=2.0, cost_scaling_factor=2.0, quantum=0.05, t0=FAN_DT, dt=FAN_DT,
                      w_sum=w_sum, w_max=w_max)


def _scene(h, mask):
    plant(h, mask, INFLATION)
    h.set_footprint(tc.FOOTPRINTS["point"])
    h.set_nav_config(253, 2)
    h.nav_field(SEEDS)
    h.set_motion_model(rollout_ref.DIFF, FAN_DT)
    h.rollout(FAN_START, _fan(65, 7), constant=True, P=20)


def _step(h, gvamd, w):
    r, t = h.control_step(_cw(gvamd, w), keep_totals=True)
    return np.array([r]).tobytes(), t.tobytes()


@pytest.mark.parametrize("w", [W(1, 1), W(3, 7, 11, 13, 17)], ids=["traj", "all"])
def test_control_step_unset_and_zero_objects(gvamd, w):
    """unset: the bytes of a second handle that never heard of X13; set with zero objects: the same result and totals"""
    h, twin = _handle(gvamd), _handle(gvamd, "twin")
    mask = np.random.default_rng(17).random((h.ny, h.nx)) < 5e-4
    for q in (h, twin):
        q.reset()
        _scene(q, mask)
    want = _step(twin, gvamd, w)
    h.set_dyn_config(ref.to_struct(gvamd, _control_cfg(9, 5)))
    h.set_moving_objects(dc.objects(CONTROL_OBJS))
    h.set_dyn_config(None)
    assert _step(h, gvamd, w) == want                                       # unset again: X13 leaves no trace
    h.set_dyn_config(ref.to_struct(gvamd, _control_cfg(9, 5)))
    assert _step(h, gvamd, w) != want                                       # (the objects do change the totals)
    h.set_moving_objects(None)
    assert _step(h, gvamd, w) == want                                       # zero objects: every dyn record {0, -1, 0, -1, +inf}


def test_control_step_with_objects(gvamd):
    h = _handle(gvamd)
    h.reset()
    _scene(h, np.zeros((h.ny, h.nx), bool))
    poses = h.rollout_array()
    ptr, K, P = h.device_rollout()
    objs = dc.objects(CONTROL_OBJS)
    h.set_moving_objects(objs)
    traj, nav = h.score_trajectories(poses, device_ptr=ptr), h.score_nav(poses, device_ptr=ptr)
    best = {}
    for w_sum, w_max in ((0, 0), (50, 0), (1, 3)):
        cfg = _control_cfg(w_sum, w_max)
        h.set_dyn_config(ref.to_struct(gvamd, cfg))
        dyn = h.score_dynamic(poses, device_ptr=ptr)
        want_d = ref.score(cfg, objs, poses)["scores"]                       # one circle at the centre: an exact family
        assert dyn.tobytes() == want_d.tobytes(), first_diff(dyn["cost_sum"], want_d["cost_sum"])
        alone = (dyn["first_collision"] >= 0) & (traj["first_collision"] < 0)
        assert alone.any() and ((dyn["first_collision"] < 0) & (traj["first_collision"] < 0)).any()
        for w in (W(1, 1), W(3, 7, 11, 13, 17)):
            nv = nav if rollout_ref.nav_used(w) else None
            want_r, want_t = ref.select(w, traj, nv, dyn, cfg)
            twin_r, twin_t = gvamd.control_select_dyn(_cw(gvamd, w), traj, nv, dyn, ref.to_struct(gvamd, cfg), keep_totals=True)
            assert np.array([twin_r]).tobytes() == want_r.tobytes() and twin_t.tobytes() == want_t.tobytes()
            for rep in range(3):
                assert _step(h, gvamd, w) == (want_r.tobytes(), want_t.tobytes()), (w_sum, w_max, w, rep)
            assert (want_t[alone] == ref.U64).all()                          # rejected by the dyn record alone
            if not rollout_ref.nav_used(w):
                best[(w_sum, w_max)] = int(want_r[0]["best"])
    assert best[(0, 0)] != best[(50, 0)] and best[(0, 0)] >= 0 and best[(50, 0)] >= 0   # the best changes only because of w_sum


def test_mppi_cycle_with_objects(gvamd):
    """gv_mppi_cycle with objects: the bytes of sample + rollout + update, whose result and totals are the control step's;
    the nominal that avoids the objects differs from the one without them"""
    h = _handle(gvamd)
    h.reset()
    _scene(h, np.zeros((h.ny, h.nx), bool))
    K, P = 257, 20
    nom = np.zeros((P, 2), np.float32)
    nom[:, 0] = 2.0
    cfg = gvamd.MppiConfig.of([0.5, 0.3], [-0.5, -1.0], [4.0, 1.0], 300.0)
    h.set_mppi(cfg)
    w = _cw(gvamd, W(1, 1))

    def three():
        h.mppi_set_nominal(nom)
        h.mppi_sample(K, 4, 0)
        ptr, k, p, cn = h.device_controls()
        h.rollout(FAN_START, (K, P, cn), device_ptr=ptr)
        step_r, step_t = h.control_step(w, keep_totals=True)
        r, t, out = h.mppi_update(w)
        assert np.array([r]).tobytes() == np.array([step_r]).tobytes() and t.tobytes() == step_t.tobytes()
        return r, t, out

    r0, t0, free = three()
    h.set_dyn_config(ref.to_struct(gvamd, _control_cfg(20, 1)))
    h.set_moving_objects(dc.objects([(8.0, 1.8, 0.2, 1.0, 1.0, -0.2, 0.0)]))   # a box drifting along the left of the path: about
    r, t, avoid = three()                                                      # half of the samples brush it
    dyn = h.score_dynamic(h.rollout_array(), device_ptr=h.device_rollout()[0])
    assert (dyn["first_collision"] >= 0).any() and 1 < r["n_valid"] < r0["n_valid"] and t.tobytes() != t0.tobytes()
    assert (t[dyn["first_collision"] >= 0] == ref.U64).all()
    assert avoid.tobytes() != free.tobytes()
    for rep in range(3):
        h.mppi_set_nominal(nom)
        r2, t2, out2 = h.mppi_cycle(FAN_START, K, 4, 0, w)
        assert np.array([r2]).tobytes() == np.array([r]).tobytes() and t2.tobytes() == t.tobytes(), rep
        assert out2.tobytes() == avoid.tobytes() == h.mppi_nominal().tobytes(), rep


def test_dynamic_demo(gvamd, tmp_path):
    """examples/dynamic_demo.cpp (plain g++ over the C ABI): a crossing car rejects the fastest straight trajectory, a
    slower one is chosen, and the host twins replay the records and the selection"""
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "grid-vision_amd")
    exe = str(tmp_path / "dynamic_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(pkg, "examples", "dynamic_demo.cpp"), "-o", exe,
                           "-L" + pkg, "-lgridvision_hip", "-Wl,-rpath," + pkg])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert re.search(r"without objects: best 0 \(3\.0 m/s\) admitted 7", out.stdout), out.stdout
    assert re.search(r"trajectory 0 \(3\.0 m/s\): max cost 254 first collision \d+ .* REJECTED", out.stdout), out.stdout
    m = re.search(r"with the car: best (\d) ", out.stdout)
    assert m and int(m.group(1)) > 0, out.stdout
    assert "dyn records equal the host's, selection equals the host's" in out.stdout and "dynamic check ok" in out.stdout
