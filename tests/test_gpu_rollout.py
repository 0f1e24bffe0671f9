"""[EXTENSION] X10 rollout and control step on the device.

Rollout: gv_rollout against rollout_ref (the header's loop with Python floats and the C library's sin / cos).  The exact
families of rollout_cases do not depend on the libm and are compared by tobytes().  The general families depend on fp64
sincos in the last bit: every finite component must equal the reference or one of its two float32 neighbours, NaN
positions must be equal, and at most 1e-4 of a family's components may be a neighbour rather than equal -- a condition
that comes from the reference's own error (a last-bit difference of sin or cos reaches a float32 pose only when the fp64
value lies within about 2^-44 of a rounding midpoint), not from a measurement.  Every call is made three times with the
same bytes.

Input and output paths: device controls from hipMalloc, pinned and pageable host controls; device_rollout() fed to
score_trajectories(device_ptr=) and score_nav against traj_ref / nav_ref on the rollout_array() read-back.

Control step: result and totals by bytes against rollout_ref.select over traj_ref / nav_ref records of the read-back
poses, the costmap() read-back and the nav_field_array() read-back: the device is held to its own poses, costmap and
field, which test_gpu_traj.py, test_gpu_inflate.py and test_gpu_nav.py pin.  traj_ref computes the footprint's vertices
with numpy's sin / cos; like traj_cases' families the read-back poses must keep every vertex 1e-9 away from a cell
border (traj_cases.guard_violations), which the tests assert."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nav_ref
import rollout_cases as rc
import rollout_ref as ref
import traj_cases as tc
import traj_ref
from planner_util import first_diff, hip_runtime, plant
from test_gpu_parity import _ground_scene, make_handle

pytestmark = pytest.mark.gpu

GV_ERR_BAD_ARG, GV_ERR_STATE = 1, 5
HERE = os.path.dirname(os.path.abspath(__file__))
INFLATION = {0.1: (0.35, 0.55, 10.0, 65), 0.05: (0.12, 0.3, 8.0, 65)}   # test_gpu_traj.INFLATION
GRID = "500x200"
NEIGHBOUR_CAP = 1e-4
_HANDLES = {}
_CELLS = {}     # pose bytes + footprint -> traj_ref.all_cells
SHARE = {}      # (kind, model, constant) -> (components, neighbours) of a family that passed: _family_share's cache

ALL_ON = ref.weights(3, 7, 11, 13, 17)
WEIGHT_SETS = [ref.weights(1, 1), ref.weights(1, 0), ref.weights(0, 1), ref.weights(w_nav_last=1), ref.weights(w_nav_sum=1),
               ref.weights(w_nav_best=1), ALL_ON]


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    yield m
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()
    _CELLS.clear()


def _handle(gvamd, grid=GRID):
    if grid not in _HANDLES:
        (gx, gy, res), (nx, ny) = tc.GRIDS[grid]
        h = gvamd.GridVisionHIP(gx, gy, res)
        assert (h.nx, h.ny) == (nx, ny)
        _HANDLES[grid] = h
    h = _HANDLES[grid]
    h.reset()
    return h


def _code(gvamd, call):
    with pytest.raises(gvamd.GVError) as e:
        call()
    return e.value.code


def _cw(gvamd, w, flags=0):
    return gvamd.CriticWeights(*[w[n] for n in ref.WEIGHTS], flags)


def _roll(h, gvamd, c):
    h.set_motion_model(c["model"], c["dt"])
    h.rollout(c["start"], c["controls"], constant=c["constant"], P=c["P"])
    return h.rollout_array()


def _compare(kind, name, got, want):
    """exact kinds: bytes.  General kinds: NaN positions equal, every other component the reference or a float32
    neighbour of it; returns (components, neighbours)."""
    assert got.dtype == np.float32 and got.shape == want.shape, name
    if kind in rc.EXACT:
        assert got.tobytes() == want.tobytes(), (name, first_diff(got, want))
        return got.size, 0
    g, w = got.reshape(-1), want.reshape(-1)
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan), (name, "NaN positions")
    g, w = g[~nan], w[~nan]
    same = g.view(np.uint32) == w.view(np.uint32)
    with np.errstate(over="ignore", invalid="ignore"):
        near = (g == np.nextafter(w, np.float32(np.inf))) | (g == np.nextafter(w, np.float32(-np.inf)))
    assert (same | near).all(), (name, first_diff(g[~(same | near)], w[~(same | near)]))
    return int(g.size), int((~same).sum())


# ------------------------------------------------------------------------------------------------------- rollout --
def _family_share(gvamd, kind, model, constant):
    """every case of the family three times against the reference (_compare asserts); (components, neighbours) of the
    family, computed once per process"""
    key = (kind, model, constant)
    if key not in SHARE:
        h = _handle(gvamd)
        n = near = 0
        for c in rc.family(kind, model, constant):
            want = rc.want(c)
            first = None
            for rep in range(3):
                got = _roll(h, gvamd, c)
                a, b = _compare(kind, c["name"], got, want)
                if first is None:
                    first, n, near = got.tobytes(), n + a, near + b
                assert got.tobytes() == first, (c["name"], rep, "the same call, other bytes")
            assert h.device_rollout()[1:] == (len(c["controls"]), c["P"])
        print("neighbour share", kind, model, constant, near, "of", n)
        SHARE[key] = (n, near)
    return SHARE[key]


@pytest.mark.parametrize("constant", [False, True], ids=["steps", "const"])
@pytest.mark.parametrize("model", rc.MODELS, ids=["diff", "omni"])
@pytest.mark.parametrize("kind", rc.KINDS)
def test_rollout_equals_the_reference(gvamd, kind, model, constant):
    n, near = _family_share(gvamd, kind, model, constant)
    assert near <= NEIGHBOUR_CAP * n, (kind, near, n)


@pytest.mark.parametrize("kind", rc.KINDS)
def test_neighbour_share_per_kind(gvamd, kind):
    """the cap over a whole kind (both models, both control forms); the figures go to DESIGN 4.13.  Every part is rolled
    out here unless test_rollout_equals_the_reference has done so in this process: the test stands alone in any order."""
    parts = [_family_share(gvamd, kind, model, constant) for model in rc.MODELS for constant in (False, True)]
    n, near = sum(p[0] for p in parts), sum(p[1] for p in parts)
    print("neighbour share of kind", kind, near, "of", n)
    assert near <= NEIGHBOUR_CAP * n, (kind, near, n)


@pytest.mark.parametrize("constant", [False, True], ids=["steps", "const"])
def test_control_sources(gvamd, constant):
    """device controls read in place from a hipMalloc buffer, pinned host controls, pageable host controls, synchronous
    and asynchronous: the same bytes every way"""
    h = _handle(gvamd)
    c = rc.family("random", ref.OMNI, constant)[3]     # 65 x 65
    u = c["controls"]
    h.set_motion_model(c["model"], c["dt"])
    want = _roll(h, gvamd, c)
    _compare("random", c["name"], want, rc.want(c))
    hip, dptr = hip_runtime(), C.c_void_p()
    assert hip.hipMalloc(C.byref(dptr), u.nbytes) == 0
    pin = gvamd.PinnedF32(u.size)
    other = np.zeros((3, 2, 3), np.float32)
    try:
        assert hip.hipMemcpy(dptr, u.ctypes.data, u.nbytes, 1) == 0   # hipMemcpyHostToDevice
        pin.array[:] = u.reshape(-1)
        pinned = pin.array.reshape(u.shape)
        for rep in range(3):
            for src, dev in ((u.shape, dptr.value), (pinned, None), (u, None)):
                for sync in (True, False):
                    h.rollout(c["start"], other, P=2)              # something else in the buffer first
                    (h.rollout if sync else h.rollout_async)(c["start"], src, constant=constant, device_ptr=dev, P=c["P"])
                    assert h.rollout_array().tobytes() == want.tobytes(), (rep, dev is not None, sync)
    finally:
        hip.hipFree(dptr)
        pin.close()


def _cells(g, fp, poses):
    key = (poses.tobytes(), fp.vertices)
    if key not in _CELLS:
        assert tc.guard_violations(g, fp, poses) == []
        _CELLS[key] = traj_ref.all_cells(g, fp, poses)
    return _CELLS[key]


def _fan(model, K, P, seed, constant=True):
    """controls of a fan from START that stays on and leaves the 500 x 200 map: dt 0.25"""
    rng = np.random.default_rng(seed)
    n = K if constant else K * P
    u = np.zeros((n, ref.n_controls(model)), np.float32)
    u[:, 0] = rng.uniform(0.5, 6.0, n)
    if model == ref.OMNI:
        u[:, 1] = rng.uniform(-0.5, 0.5, n)
    u[:, -1] = rng.uniform(-0.6, 0.6, n)
    return u if constant else u.reshape(K, P, -1)


FAN_START, FAN_DT = (2.0, 0.3, 0.1), 0.25
SEEDS = np.array([(30.0 - 0.5 * i, -2.0 + 0.1 * i) for i in range(40)], np.float32)   # a path: some seed is on a free cell


def _random_mask(nx, ny, density, seed):
    return np.random.default_rng(seed).random((ny, nx)) < density


def _scene(h, mask, fp_name="triangle", nav_cfg=(253, 2)):
    """plant and inflate the mask, solve the field from SEEDS; returns (costmap, field) read-backs"""
    cost = plant(h, mask, INFLATION[0.1])
    h.set_footprint(tc.FOOTPRINTS[fp_name])
    h.set_nav_config(*nav_cfg)
    h.nav_field(SEEDS)
    return cost, h.nav_field_array()


def _records(g, fp, cost, field, poses):
    return traj_ref.score(g, fp, cost, poses, _cells(g, fp, poses))[0], nav_ref.score(g, field, poses)


def test_resident_rollout_feeds_the_samplers(gvamd):
    """device_rollout() as the device poses of score_trajectories and score_nav: the records of the read-back poses"""
    h = _handle(gvamd)
    g, fp = tc.grid_of(GRID), tc.fp_of("triangle")
    cost, field = _scene(h, _random_mask(h.nx, h.ny, 5e-4, seed=17))
    for model, constant in ((ref.DIFF, True), (ref.OMNI, False)):
        h.set_motion_model(model, FAN_DT)
        h.rollout(FAN_START, _fan(model, 65, 20, 7, constant), constant=constant, P=20)
        poses = h.rollout_array()
        ptr, K, P = h.device_rollout()
        assert (K, P) == (65, 20) and ptr
        want_t, want_n = _records(g, fp, cost, field, poses)
        assert (want_t["n_off_map"] == 0).any() and ((want_t["n_off_map"] > 0).any() or not constant)   # the fan leaves the map
        for rep in range(3):
            got_t = h.score_trajectories(poses, device_ptr=ptr)
            got_n = h.score_nav(poses, device_ptr=ptr)
            assert got_t.tobytes() == want_t.tobytes(), (rep, first_diff(got_t, want_t))
            assert got_n.tobytes() == want_n.tobytes(), (rep, first_diff(got_n, want_n))
        assert h.rollout_array().tobytes() == poses.tobytes()      # the scoring calls leave the rollout alone


# -------------------------------------------------------------------------------------------------- control step --
def _check_step(h, gvamd, w, traj, nav, tag):
    want_r, want_t = ref.select(w, traj, nav)
    for rep in range(3):
        got_r, got_t = h.control_step(_cw(gvamd, w), keep_totals=True)
        assert np.array([got_r]).tobytes() == want_r.tobytes(), (tag, w, rep, got_r, want_r)
        assert got_t.dtype == np.uint64 and got_t.tobytes() == want_t.tobytes(), (tag, w, rep, first_diff(got_t, want_t))
        only = h.control_step(_cw(gvamd, w))
        assert np.array([only]).tobytes() == want_r.tobytes(), (tag, w, rep, "without totals")
    return want_r[0], want_t


@pytest.mark.parametrize("model,constant", [(ref.DIFF, True), (ref.OMNI, False)], ids=["diff_const", "omni_steps"])
@pytest.mark.parametrize("scene", ["sparse", "dense", "empty", "full"])
def test_control_step_maps_and_weights(gvamd, scene, model, constant):
    h = _handle(gvamd)
    g, fp = tc.grid_of(GRID), tc.fp_of("triangle")
    mask = {"sparse": lambda: _random_mask(h.nx, h.ny, 5e-4, seed=17), "dense": lambda: _random_mask(h.nx, h.ny, 0.3, seed=17),
            "empty": lambda: np.zeros((h.ny, h.nx), bool), "full": lambda: np.ones((h.ny, h.nx), bool)}[scene]()
    cost, field = _scene(h, mask)
    h.set_motion_model(model, FAN_DT)
    h.rollout(FAN_START, _fan(model, 65, 20, 7, constant), constant=constant, P=20)
    poses = h.rollout_array()
    traj, nav = _records(g, fp, cost, field, poses)
    for w in WEIGHT_SETS:
        r, t = _check_step(h, gvamd, w, traj, nav, scene)
        if scene in ("full", "dense"):
            assert (r["best"], r["n_valid"], r["best_total"]) == (-1, 0, ref.U64)
        if scene == "sparse":
            assert 0 < r["n_valid"] and r["best"] >= 0
        if scene == "empty" and not ref.nav_used(w):
            assert 0 < r["n_valid"] and r["best_total"] == 0     # every admitted total is 0: the smallest index wins
            assert r["best"] == int(np.flatnonzero(t == 0)[0])


@pytest.mark.parametrize("place", [0, 63, 64, 1023, 1024, 1025])
def test_tie_goes_to_the_smallest_index(gvamd, place):
    """K = 2049 constant controls, P = 2: the best control row copied to another k ties with it exactly"""
    h = _handle(gvamd)
    g, fp = tc.grid_of(GRID), tc.fp_of("point")
    cost, field = _scene(h, _random_mask(h.nx, h.ny, 5e-4, seed=17), "point")
    h.set_motion_model(ref.DIFF, FAN_DT)
    u = _fan(ref.DIFF, 2049, 2, 11)
    w = ref.weights(1, 0, 1, 0, 0)

    def step(controls):
        h.rollout(FAN_START, controls, constant=True, P=2)
        poses = h.rollout_array()
        return _check_step(h, gvamd, w, *_records(g, fp, cost, field, poses), place)[0]

    base = step(u)
    b = int(base["best"])
    assert b >= 0 and b not in (0, 63, 64, 1023, 1024, 1025)
    v = u.copy()
    v[place] = u[b]
    r = step(v)
    assert r["best"] == min(place, b) and r["best_total"] == base["best_total"]
    if place < b:                                   # ... and all six at once: still the smallest
        for k in (0, 63, 64, 1023, 1024, 1025):
            v[k] = u[b]
        assert step(v)["best"] == 0


def test_destinations(gvamd):
    """result and totals into pinned memory (written by the kernel), into pinned memory that is not aligned (the copy
    command) and into pageable memory"""
    h = _handle(gvamd)
    g, fp = tc.grid_of(GRID), tc.fp_of("triangle")
    cost, field = _scene(h, _random_mask(h.nx, h.ny, 5e-4, seed=17))
    h.set_motion_model(ref.DIFF, FAN_DT)
    h.rollout(FAN_START, _fan(ref.DIFF, 65, 20, 7), constant=True, P=20)
    K = 65
    want_r, want_t = ref.select(ALL_ON, *_records(g, fp, cost, field, h.rollout_array()))
    pin_r, pin_t = gvamd.PinnedI8(16 + 16), gvamd.PinnedI8(K * 8 + 8)
    try:
        for rep in range(3):
            for off_r, off_t in ((0, 0), (8, 4), (0, 4), (8, 0)):
                pin_r.array[:] = 77
                pin_t.array[:] = 77
                res = pin_r.array[off_r:off_r + 16].view(ref.RESULT_DTYPE)
                tot = pin_t.array[off_t:off_t + K * 8].view(np.uint64)
                h.control_step_async(_cw(gvamd, ALL_ON), res, tot)
                h.synchronize()
                assert res.tobytes() == want_r.tobytes() and tot.tobytes() == want_t.tobytes(), (rep, off_r, off_t)
                pin_r.array[:] = 77
                pin_t.array[:] = 77
                h.control_step_async(_cw(gvamd, ALL_ON), res)
                h.synchronize()
                assert res.tobytes() == want_r.tobytes() and (pin_t.array == 77).all()    # no totals without the flag
            res, tot = np.full(1, 7, ref.RESULT_DTYPE), np.full(K, 7, np.uint64)
            h.control_step_async(_cw(gvamd, ALL_ON), res, tot)
            h.synchronize()
            assert res.tobytes() == want_r.tobytes() and tot.tobytes() == want_t.tobytes(), (rep, "pageable")
    finally:
        pin_r.close()
        pin_t.close()


def test_sequence_with_one_synchronize(gvamd):
    """rollout, control step, set_footprint, control step, set_motion_model, a second rollout, control step -- enqueued
    back to back, one synchronize: every call keeps the configuration it was enqueued with and reads the rollout before it"""
    h = _handle(gvamd)
    g, tri, dia = tc.grid_of(GRID), tc.fp_of("triangle"), tc.fp_of("diamond", 200, 7)
    cost, field = _scene(h, _random_mask(h.nx, h.ny, 2e-3, seed=23))
    u1, u2 = _fan(ref.DIFF, 65, 20, 7), _fan(ref.DIFF, 64, 20, 8, constant=False)
    h.set_motion_model(ref.DIFF, FAN_DT)
    h.rollout(FAN_START, u1, constant=True, P=20)
    p1 = h.rollout_array()
    h.set_motion_model(ref.DIFF, 0.2)
    h.rollout(FAN_START, u2)
    p2 = h.rollout_array()
    want = [ref.select(ALL_ON, *_records(g, fp, cost, field, p)) for fp, p in ((tri, p1), (dia, p1), (dia, p2))]
    assert len({w[1].tobytes() for w in want}) == 3
    outs = [(gvamd.PinnedI8(16), gvamd.PinnedI8(65 * 8)) for _ in range(3)]
    try:
        for o in outs:
            o[0].array[:] = 77
            o[1].array[:] = 77

        def enqueue(i, K):
            h.control_step_async(_cw(gvamd, ALL_ON), outs[i][0].array.view(ref.RESULT_DTYPE), outs[i][1].array[:K * 8].view(np.uint64))
        h.set_footprint(tri.vertices, tri.collision_cost, tri.off_map_cost)
        h.set_motion_model(ref.DIFF, FAN_DT)
        h.rollout_async(FAN_START, u1, constant=True, P=20)
        h.set_motion_model(ref.OMNI, 3.0)                    # does not reach the rollout already enqueued
        enqueue(0, 65)
        h.set_footprint(dia.vertices, dia.collision_cost, dia.off_map_cost)
        enqueue(1, 65)
        h.set_motion_model(ref.DIFF, 0.2)
        h.rollout_async(FAN_START, u2)
        enqueue(2, 64)
        h.synchronize()
        assert h.rollout_array().tobytes() == p2.tobytes()
        for i, K in enumerate((65, 65, 64)):
            assert outs[i][0].array.tobytes() == want[i][0].tobytes(), i
            assert outs[i][1].array[:K * 8].tobytes() == want[i][1].tobytes(), i
    finally:
        for o in outs:
            o[0].close(); o[1].close()


def test_control_step_during_a_pending_tick(gvamd):
    """tick_enqueue, inflate, rollout, control step, tick_wait against a twin handle that does one thing after the other:
    the step reads the costmap of the tick's grid"""
    P5 = (0.5, 1.1, 5.0, 80)   # test_gpu_traj.P5
    hA, tfs = make_handle(gvamd, 2, perturbed=True)
    hB, _ = make_handle(gvamd, 2, perturbed=True)
    from gvamd import synth
    cfg = synth.CONFIGS[2]["grid"]
    g, fp = traj_ref.grid(cfg.grid_x, cfg.grid_y, cfg.resolution), tc.fp_of("rect")
    x, y, z, _, b = _ground_scene(tfs, seed=9)
    rng = np.random.default_rng(3)
    K, P = 129, 20
    u = np.stack([rng.uniform(2.0, 6.0, K), rng.uniform(-0.25, 0.25, K)], axis=1).astype(np.float32)
    start = (2.0, 0.7, 0.05)      # the scene lies ahead of the base: x in 1 .. 60 m
    w = ref.weights(1, 2)
    pr, pt = gvamd.PinnedI8(16), gvamd.PinnedI8(K * 8)
    try:
        for h in (hA, hB):
            h.upload_xyz(x, y, z)
            h.tick(b, k_near=4, lidar_bin=True)
            h.set_inflation(*P5)
            h.set_footprint(fp.vertices)
            h.set_motion_model(ref.DIFF, 0.5)
        hB.inflate()
        before = hB.costmap()
        pr.array[:] = 77
        pt.array[:] = 77
        hA.tick_enqueue(b, k_near=4, lidar_bin=True)
        hA.inflate()
        hA.rollout_async(start, u, constant=True, P=P)
        hA.control_step_async(_cw(gvamd, w), pr.array.view(ref.RESULT_DTYPE), pt.array.view(np.uint64))
        hA.tick_wait()
        hA.synchronize()
        hB.tick(b, k_near=4, lidar_bin=True)
        hB.inflate()
        cost = hB.costmap()
        hB.rollout(start, u, constant=True, P=P)
        twin_r, twin_t = hB.control_step(_cw(gvamd, w), keep_totals=True)
        poses = hA.rollout_array()
        assert poses.tobytes() == hB.rollout_array().tobytes()
        cells = _cells(g, fp, poses)
        want_r, want_t = ref.select(w, traj_ref.score(g, fp, cost, poses, cells)[0])
        stale_r, stale_t = ref.select(w, traj_ref.score(g, fp, before, poses, cells)[0])
        assert want_t.tobytes() != stale_t.tobytes()
        assert pr.array.tobytes() == want_r.tobytes() == np.array([twin_r]).tobytes()
        assert pt.array.tobytes() == want_t.tobytes() == twin_t.tobytes()
    finally:
        pr.close(); pt.close()
        hA.close(); hB.close()


# --------------------------------------------------------------------------------------------------------- rules --
def test_control_step_without_a_rollout(gvamd):
    """a fresh handle with everything else a control step needs -- footprint, costmap, field -- and no rollout:
    GV_ERR_STATE from both forms, nothing launched (K = P = 0), with and without a motion model; after the first rollout
    the same calls succeed"""
    (gx, gy, res), _ = tc.GRIDS["250x100"]
    h = gvamd.GridVisionHIP(gx, gy, res)
    g, tri = tc.grid_of("250x100"), tc.fp_of("triangle")
    res_out, tot = np.full(1, 7, ref.RESULT_DTYPE), np.full(4, 7, np.uint64)
    try:
        cost = plant(h, _random_mask(h.nx, h.ny, 1e-3, seed=5), INFLATION[0.1])
        h.set_footprint(tri.vertices)
        h.set_nav_config(253, 1)
        h.nav_field(np.array([(8.0, 0.5), (9.0, 0.0), (10.0, -0.5)], np.float32))

        def refused():
            for w in (ref.weights(1, 1), ALL_ON):
                for call in (lambda: h.control_step(_cw(gvamd, w)), lambda: h.control_step(_cw(gvamd, w), keep_totals=True),
                             lambda: h.control_step_async(_cw(gvamd, w), res_out),
                             lambda: h.control_step_async(_cw(gvamd, w), res_out, tot)):
                    with pytest.raises(gvamd.GVError) as e:
                        call()
                    assert e.value.code == GV_ERR_STATE and "no rollout" in str(e.value), str(e.value)
            h.synchronize()
            assert res_out.tobytes() == np.full(1, 7, ref.RESULT_DTYPE).tobytes() and (tot == 7).all()   # nothing was written

        refused()
        h.set_motion_model(ref.DIFF, 0.1)
        refused()                                                                       # a model is not a rollout
        assert _code(gvamd, h.device_rollout) == GV_ERR_STATE
        u = np.zeros((4, 3, 2), np.float32)
        u[:, :, 0] = 1.0
        u[:, :, 1] = np.linspace(-0.5, 0.5, 12).reshape(4, 3)
        h.rollout((5.0, 1.0, 0.3), u)
        poses = h.rollout_array()
        assert tc.guard_violations(g, tri, poses) == []
        traj, nav = traj_ref.score(g, tri, cost, poses)[0], nav_ref.score(g, h.nav_field_array(), poses)
        want_r, want_t = ref.select(ALL_ON, traj, nav)
        h.control_step_async(_cw(gvamd, ALL_ON), res_out, tot)
        h.synchronize()
        assert res_out.tobytes() == want_r.tobytes() and tot.tobytes() == want_t.tobytes()
        assert np.array([h.control_step(_cw(gvamd, ALL_ON))]).tobytes() == want_r.tobytes()
    finally:
        h.close()


def test_state_and_argument_rules(gvamd):
    (gx, gy, res), _ = tc.GRIDS["250x100"]
    h = gvamd.GridVisionHIP(gx, gy, res)
    lib = gvamd.load()
    g, tri = tc.grid_of("250x100"), tc.fp_of("triangle")
    code = lambda call: _code(gvamd, call)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    u = np.zeros((4, 3, 2), np.float32)
    u[:, :, 0] = 1.0
    u[:, :, 1] = np.linspace(-0.5, 0.5, 12).reshape(4, 3)
    start = (5.0, 1.0, 0.3)

    def raw(start_=start, controls=u, K=4, P=3, flags=0, fn=lib.gv_rollout):
        s = (C.c_double * 3)(*start_) if start_ is not None else None
        return fn(h._h, s, p(controls), C.c_int32(K), C.c_int32(P), C.c_uint32(flags))

    try:
        # ---- the motion model and the rollout
        assert code(lambda: h.rollout(start, u)) == GV_ERR_STATE                       # no motion model
        assert code(h.device_rollout) == code(h.rollout_array) == GV_ERR_STATE          # no rollout yet
        assert lib.gv_get_rollout(h._h, p(np.zeros(36, np.float32))) == GV_ERR_STATE
        h.set_motion_model(ref.DIFF, 0.1)
        assert code(h.device_rollout) == GV_ERR_STATE
        h.rollout(start, u)
        want = ref.rollout(ref.DIFF, 0.1, start, u)
        got = h.rollout_array()
        _compare("random", "rules", got, want)
        ptr, K, P = h.device_rollout()
        assert (K, P) == (4, 3) and ptr
        # a rejected model leaves the one in force alone
        for model, dt, fl in ((2, 0.1, 0), (-1, 0.1, 0), (0, 0.0, 0), (0, -0.1, 0), (0, float("inf"), 0), (0, float("nan"), 0), (0, 0.1, 1)):
            assert code(lambda: h.set_motion_model(gvamd.MotionModel(model, dt, fl))) == GV_ERR_BAD_ARG
        h.rollout(start, u)
        assert h.rollout_array().tobytes() == got.tobytes()
        # argument limits
        assert raw(start_=None) == raw(controls=None) == GV_ERR_BAD_ARG
        for i in range(3):
            for v in (float("nan"), float("inf")):
                s = list(start); s[i] = v
                assert raw(start_=s) == GV_ERR_BAD_ARG
        assert raw(P=0) == raw(P=4097) == raw(K=-1) == raw(K=(1 << 20) + 1) == raw(flags=4) == GV_ERR_BAD_ARG
        assert raw(K=(1 << 12) + 1, P=4096, flags=ref.CONSTANT) == GV_ERR_BAD_ARG      # K * P > 2^24
        assert raw(fn=lib.gv_rollout_async, P=0) == GV_ERR_BAD_ARG
        assert lib.gv_device_rollout(h._h, None, None, None) == lib.gv_get_rollout(h._h, None) == GV_ERR_BAD_ARG
        assert lib.gv_set_motion_model(None, None) == GV_ERR_BAD_ARG
        # K == 0: a successful no-op that leaves the previous rollout in place
        assert raw(K=0) == 0 and raw(K=0, P=7, fn=lib.gv_rollout_async) == 0
        assert h.device_rollout() == (ptr, 4, 3) and h.rollout_array().tobytes() == got.tobytes()
        # a smaller rollout keeps the pointer; the buffer is kept through gv_reset, gv_set_log_odds and gv_grid_move
        h.rollout(start, u[:2, :2])
        assert h.device_rollout() == (ptr, 2, 2) and h.rollout_array().tobytes() == got[:2, :2].tobytes()
        h.rollout(start, u)
        h.reset()
        assert h.device_rollout() == (ptr, 4, 3) and h.rollout_array().tobytes() == got.tobytes()
        h.rollout(start, u)                                                             # the model too
        assert h.rollout_array().tobytes() == got.tobytes()
        # a larger rollout grows the buffer: the pointer may change, and the getter reports the one in force
        big = np.zeros((300, 130, 2), np.float32)
        big[:, :, 0] = np.linspace(0.5, 2.0, 300, dtype=np.float32)[:, None]
        big[:, :, 1] = np.linspace(-0.4, 0.4, 130, dtype=np.float32)[None, :]
        h.rollout(start, big)
        ptr2, K, P = h.device_rollout()
        assert (K, P) == (300, 130) and ptr2
        grown = h.rollout_array()
        _compare("random", "grown", grown, ref.rollout(ref.DIFF, 0.1, start, big))
        direct = np.zeros_like(grown)
        assert hip_runtime().hipMemcpy(direct.ctypes.data, ptr2, direct.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        assert direct.tobytes() == grown.tobytes()
        h.rollout(start, u)                                                             # smaller again: it stays there
        assert h.device_rollout() == (ptr2, 4, 3) and h.rollout_array().tobytes() == got.tobytes()
        # a null handle
        null = C.c_void_p(None)
        assert raw(fn=lambda _h, *a: lib.gv_rollout(null, *a)) == GV_ERR_BAD_ARG
        assert raw(fn=lambda _h, *a: lib.gv_rollout_async(null, *a)) == GV_ERR_BAD_ARG
        out_p, out_k = C.c_void_p(), C.c_int32()
        assert lib.gv_device_rollout(null, C.byref(out_p), C.byref(out_k), C.byref(out_k)) == GV_ERR_BAD_ARG
        assert lib.gv_get_rollout(null, p(np.zeros(36, np.float32))) == GV_ERR_BAD_ARG
        mm = gvamd.MotionModel(ref.DIFF, 0.1, 0)
        assert lib.gv_set_motion_model(null, C.byref(mm)) == GV_ERR_BAD_ARG
        for fn in (lib.gv_control_step, lib.gv_control_step_async):
            cw0, r0 = _cw(gvamd, ref.weights(1, 1)), np.zeros(1, ref.RESULT_DTYPE)
            assert fn(null, C.byref(cw0), C.c_uint32(0), p(r0), None) == GV_ERR_BAD_ARG
        # ---- the control step
        cw = _cw(gvamd, ALL_ON)
        step = lambda w=ref.weights(1, 1): h.control_step(_cw(gvamd, w))
        assert code(step) == GV_ERR_STATE                                               # no footprint, no costmap
        h.set_footprint(tri.vertices)
        assert code(step) == GV_ERR_STATE                                               # no costmap
        cost = plant(h, _random_mask(h.nx, h.ny, 1e-3, seed=5), INFLATION[0.1])
        assert h.rollout_array().tobytes() == got.tobytes()                             # gv_set_log_odds kept it
        h.rollout(start, u[:2, :2])
        h.rollout(start, u)                                                             # ... and the model
        assert h.rollout_array().tobytes() == got.tobytes()
        poses = h.rollout_array()
        traj = traj_ref.score(g, tri, cost, poses)[0]
        assert np.array([step()]).tobytes() == ref.select(ref.weights(1, 1), traj)[0].tobytes()
        assert code(lambda: step(ALL_ON)) == GV_ERR_STATE                               # a nav weight, no field
        h.set_nav_config(253, 1)
        h.nav_field(np.array([(8.0, 0.5), (9.0, 0.0), (10.0, -0.5)], np.float32))
        nav = nav_ref.score(g, h.nav_field_array(), poses)
        assert np.array([step(ALL_ON)]).tobytes() == ref.select(ALL_ON, traj, nav)[0].tobytes()
        h.set_footprint(None)
        assert code(step) == GV_ERR_STATE                                               # no footprint
        h.set_footprint(tri.vertices)
        rbuf = np.zeros(1, ref.RESULT_DTYPE)
        tot = np.zeros(4, np.uint64)
        rawstep = lambda w=cw, flags=0, r=rbuf, t=None: lib.gv_control_step(h._h, C.byref(w) if w is not None else None,
                                                                          C.c_uint32(flags), p(r), p(t))
        assert rawstep() == 0 and rawstep(flags=1, t=tot) == 0
        assert rawstep(w=None) == rawstep(r=None) == rawstep(flags=2) == rawstep(flags=1, t=None) == GV_ERR_BAD_ARG
        assert rawstep(w=_cw(gvamd, ALL_ON, 1)) == GV_ERR_BAD_ARG
        for name in ref.WEIGHTS:
            w = dict(ALL_ON); w[name] = 65536
            assert rawstep(w=_cw(gvamd, w)) == GV_ERR_BAD_ARG, name
        assert rawstep(t=tot) == 0                                                      # totals ignored without the flag
        assert h.grid_move([0.0, 0.0, 0.0, 1.0, 3 * res, -2 * res, 0.0])["applied"]
        assert h.rollout_array().tobytes() == got.tobytes()                             # gv_grid_move kept it
        h.rollout(start, u[:2, :2])
        h.rollout(start, u)                                                             # ... and the model
        assert h.rollout_array().tobytes() == got.tobytes()
        h.reset()                                                                      # the costmap and the field are gone
        assert code(step) == GV_ERR_STATE
        # NULL turns the model off; the rollout it made stays
        h.set_motion_model(None)
        assert code(lambda: h.rollout(start, u)) == GV_ERR_STATE
        assert h.rollout_array().tobytes() == got.tobytes()
    finally:
        h.close()


def test_controller_demo(gvamd, tmp_path):
    """examples/controller_demo.cpp (plain g++ over the C ABI): ticks of the flow with inflate_costmap, the field from a
    goal behind the wall, a fan of 41 constant controls rolled out and selected on the device, and the demo's own host
    replay of the choice and of every total"""
    pkg = os.path.join(os.path.dirname(HERE), "grid-vision_amd")
    exe = str(tmp_path / "controller_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(pkg, "examples", "controller_demo.cpp"), "-o", exe,
                           "-L" + pkg, "-lgridvision_hip", "-Wl,-rpath," + pkg])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    m = re.search(r"trajectories 41 poses 40 admitted (\d+)\nfield rounds \d+ seeds 1\nbest (\d+) w (-?[\d.]+) total (\d+)\n"
                  r"straight total (\d+)\npose floats that differ from the host rollout (\d+) of 4920\n"
                  r"host check ok \(0 mismatches\)", out.stdout)
    assert m, out.stdout
    admitted, best, straight = int(m.group(1)), int(m.group(2)), int(m.group(5))
    assert 0 < admitted < 41 and best != 20 and straight == ref.U64   # some arcs pass the wall, the straight one does not
