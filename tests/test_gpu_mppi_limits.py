"""[EXTENSION] X12 MPPI limits and control cost on the device.

Constraint: the chain holds no library call, so the device must equal the library's host twin gv_mppi_constrain (which
test_mppi_limits_host.py holds to mppi_limits_ref byte for byte) BY BYTES, given the same f.  f is the device's own: a
sampling with the limits off, read back; the same seed and iteration with the limits on must give the twin's bytes on it.

Control cost: gv_get_mppi_control_costs against gv_mppi_control_costs on the device's read-back controls and nominal, by
bytes (a fixed order of sums).  The new nominal against mppi_limits_ref.average_cc fed the device's own read-backs
(controls, totals, g, the old nominal) inside test_gpu_mppi._check_nominal's bound, unchanged:
  |got - want| <= 2^-24 |want| + (2 K + 16) 2^-53 A,   A = sum e_k |u| / S
-- derived there for the reordering of the K-term sums; the new inputs of the weights (g, m) are bit-identical on both
sides, so nothing is added to it.  result and totals by bytes against gv_control_step."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mppi_limits_ref as lref
import mppi_ref as ref
import rollout_ref
import traj_cases as tc
from planner_util import first_diff, plant
from test_gpu_parity import _ground_scene, make_handle

pytestmark = pytest.mark.gpu

GV_ERR_BAD_ARG, GV_ERR_STATE = 1, 5
DIFF, OMNI = rollout_ref.DIFF, rollout_ref.OMNI
INFLATION = (0.35, 0.55, 10.0, 65)      # test_gpu_mppi.INFLATION
GRID = "500x200"
SHAPES = [(1, 130), (3, 64), (64, 63), (65, 65), (257, 2), (65, 1)]   # (K, P): rollout_cases.SHAPES
START = (2.0, 0.3, 0.1)
SEEDS = np.array([(30.0 - 0.5 * i, -2.0 + 0.1 * i) for i in range(40)], np.float32)   # test_gpu_mppi.SEEDS
ALL_ON = rollout_ref.weights(3, 7, 11, 13, 17)
INF, NAN = float("inf"), float("nan")
F = np.float32
_HANDLES = []


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    yield m
    for h in _HANDLES:
        h.close()
    _HANDLES.clear()


def _new_scene_handle(gvamd):
    """test_gpu_mppi's 500 x 200 scene: planted obstacles, the costmap, a footprint and the field"""
    (gx, gy, res), (nx, ny) = tc.GRIDS[GRID]
    h = gvamd.GridVisionHIP(gx, gy, res)
    assert (h.nx, h.ny) == (nx, ny)
    mask = np.random.default_rng(17).random((h.ny, h.nx)) < 5e-4
    plant(h, mask, INFLATION)
    h.set_footprint(tc.FOOTPRINTS["triangle"])
    h.set_nav_config(253, 2)
    h.nav_field(SEEDS)
    _HANDLES.append(h)
    return h


@pytest.fixture(scope="module")
def scene(gvamd):
    return _new_scene_handle(gvamd)


def _code(gvamd, call):
    with pytest.raises(gvamd.GVError) as e:
        call()
    return e.value.code


def _cw(gvamd, w, flags=0):
    return gvamd.CriticWeights(*[w[n] for n in rollout_ref.WEIGHTS], flags)


def _nominal(P, Cn, seed=0, base=0.3):
    rng = np.random.default_rng(100 + seed)
    return (base + rng.uniform(-0.05, 0.05, (P, Cn))).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- constraint --
SIGMA, LO, HI = [0.2, 0.2, 0.2], [-0.1, -0.5, 0.1], [0.6, 0.9, 0.45]
# (name, rate_up, rate_down, u_prev, radius): the edge families of test_mppi_limits_host.py
FAMILIES = [
    ("rates", [2.0, 3.0, 1.5], [4.0, 3.0, 0.5], [0.25, -0.1, 0.3], 0.0),
    ("zero", [0.0] * 3, [0.0] * 3, [0.3, -0.2, 0.2], 0.0),
    ("up-free", [INF] * 3, [1.0] * 3, [0.3, 0.0, 0.3], 0.0),
    ("down-free", [1.0] * 3, [INF] * 3, [0.3, 0.0, 0.3], 0.0),
    ("nan-one-channel", [0.5] * 3, [0.5] * 3, [0.3, NAN, 0.3], 0.0),
    ("outside-the-box", [1.0] * 3, [1.0] * 3, [1.5, -1.4, 1.0], 0.0),
    ("neutral", [INF] * 3, [INF] * 3, [NAN] * 3, 0.0),
    ("radius", [INF] * 3, [INF] * 3, [NAN] * 3, 0.4),
    ("radius-and-rates", [2.0, 4.0, 1.0], [2.0, 4.0, 1.0], [0.0, 0.0, 0.0], 0.4),
]


@pytest.mark.parametrize("shift", [False, True], ids=["plain", "shift"])
@pytest.mark.parametrize("model", [DIFF, OMNI], ids=["diff", "omni"])
def test_constraint_equals_the_host_twin(gvamd, scene, model, shift):
    h = scene
    Cn = rollout_ref.n_controls(model)
    dt = 0.1
    mm = gvamd.MotionModel(model, dt, 0)
    h.set_motion_model(model, dt)
    h.set_mppi(gvamd.MppiConfig.of(SIGMA[:Cn], LO[:Cn], HI[:Cn], 1.0))
    ps, changed = set(), {}
    for i, (K, P) in enumerate(SHAPES + [(130, 33)]):
        seed, it = 1 + i % 3, 5 + i
        h.mppi_set_nominal(_nominal(P, Cn, i))
        h.set_mppi_limits(None)
        h.mppi_sample(K, seed, it, shift)
        f = h.controls_array()                                         # f, as the device's own libm made it
        for name, up, dn, prev, radius in FAMILIES:
            if radius > 0 and model != DIFF:
                continue
            lim = gvamd.MppiLimits.of(up, dn, prev, radius)
            want = gvamd.mppi_constrain(lim, mm, f)
            h.set_mppi_limits(lim)
            for rep in range(3 if name == "rates" else 1):
                h.mppi_sample(K, seed, it, shift, wait=rep != 1)
                got = h.controls_array()
                assert got.tobytes() == want.tobytes(), (name, K, P, rep, first_diff(got, want))
            changed[name] = changed.get(name, False) or (want != f).any()
            if name == "zero":
                assert (got == np.float32(prev[:Cn])).all()
            if name == "neutral":
                assert got.tobytes() == f.tobytes()
            if name == "outside-the-box" and P >= 63:
                inside = (got >= np.float32(LO[:Cn])) & (got <= np.float32(HI[:Cn]))
                assert not inside[:, 0].all() and inside[:, -1].all()
            if name == "radius":
                assert (np.abs(got[:, :, 1]) <= (np.abs(got[:, :, 0]) * F(1.0 / 0.4)).astype(F)).all()
        assert h.device_controls()[1:] == (K, P, Cn)
        ps.add(P)
    assert {63, 64, 65, 130} <= ps                                      # the chunk edges of the kernel's walk
    assert all(v for n, v in changed.items() if n != "neutral") and not changed["neutral"], changed


def test_radius_edges_are_exact(gvamd, scene):
    """v = 0 (w becomes a zero of the definition's sign), v < 0, and |w| exactly on the bound, made by clamps and sigma 0"""
    h = scene
    K, P, dt, r = 65, 64, 0.1, 0.5
    mm = gvamd.MotionModel(DIFF, dt, 0)
    h.set_motion_model(DIFF, dt)
    lim = gvamd.MppiLimits.of(min_turn_radius=r)
    nom = _nominal(P, 2, 3)
    nom[::2, 1] *= -1
    for name, cfg in (("v=0", gvamd.MppiConfig.of([0.2, 0.3], [0.0, -1.0], [0.0, 1.0])),
                      ("v<0", gvamd.MppiConfig.of([0.2, 0.3], [-0.5, -1.0], [-0.1, 1.0])),
                      ("on-the-bound", gvamd.MppiConfig.of([0.0, 0.0], [0.25, -0.5], [0.25, 0.5]))):
        h.set_mppi(cfg)
        if name == "on-the-bound":
            nom[:, 0], nom[::2, 1], nom[1::2, 1] = 0.25, 0.5, -0.5
        h.mppi_set_nominal(nom)
        h.set_mppi_limits(None)
        h.mppi_sample(K, 4, 2)
        f = h.controls_array()
        h.set_mppi_limits(lim)
        h.mppi_sample(K, 4, 2)
        got = h.controls_array()
        assert got.tobytes() == gvamd.mppi_constrain(lim, mm, f).tobytes(), name
        if name == "v=0":
            assert (f[:, :, 0] == 0).all() and (got[:, :, 1] == 0).all() and (f[:, :, 1] != 0).all()
            assert np.array_equal(np.signbit(got[:, :, 1]), f[:, :, 1] < 0) and np.signbit(got[:, :, 1]).any() and not np.signbit(got[:, :, 1]).all()
        elif name == "v<0":
            assert (got[:, :, 0] < 0).all() and (got[:, :, 1] != f[:, :, 1]).any()
            assert (np.abs(got[:, :, 1]) <= (np.abs(got[:, :, 0]) * F(1.0 / r)).astype(F)).all()
        else:
            assert (np.abs(f[:, :, 1]) == F(0.5)).all() and got.tobytes() == f.tobytes()


# ------------------------------------------------------------------------------------------- update with gamma --
def _mppi_setup(h, gvamd, model, P, lam, dt=None, sigma=(0.5, 0.3, 0.3), seed=0):
    """test_gpu_mppi._mppi_setup"""
    Cn = rollout_ref.n_controls(model)
    dt = dt if dt is not None else (0.25 if P <= 64 else 0.12)
    nom = np.zeros((P, Cn), np.float32)
    nom[:, 0] = 1.0 + np.random.default_rng(seed).uniform(-0.1, 0.1, P)
    nom[:, -1] = 0.02
    sg = [sigma[0]] + ([sigma[1]] if Cn == 3 else []) + [sigma[2]]
    cfg = gvamd.MppiConfig.of(sg, [-0.5] * Cn, [2.5] * Cn, lam)
    h.set_motion_model(model, dt)
    h.set_mppi(cfg)
    h.mppi_set_nominal(nom)
    return nom, cfg


def _limits(gvamd, model, gamma, radius=None):
    """rate limits that bind on about half the steps, a radius for DIFF, gamma"""
    Cn = rollout_ref.n_controls(model)
    radius = (1.5 if model == DIFF else 0.0) if radius is None else radius
    return gvamd.MppiLimits.of([3.0] * Cn, [4.0] * Cn, [0.9] + [0.0] * (Cn - 1), radius, gamma)


def _three_calls(h, K, seed, it, w, gvamd, start=START, shift=False):
    h.mppi_sample(K, seed, it, shift)
    ptr, k, P, Cn = h.device_controls()
    assert k == K
    h.rollout(start, (K, P, Cn), device_ptr=ptr)
    step_r, step_t = h.control_step(_cw(gvamd, w), keep_totals=True)
    r, t, nom = h.mppi_update(_cw(gvamd, w))
    assert np.array([r]).tobytes() == np.array([step_r]).tobytes() and t.tobytes() == step_t.tobytes()
    return r, t, nom


def _check_nominal(got, lam, controls, totals, g, old, K, tag):
    """test_gpu_mppi._check_nominal with the control costs in the reference's weights; the bound is unchanged"""
    want32, want, A = lref.average_cc(lam, controls, totals, g, old, bound=True)
    bound = 2.0 ** -24 * np.abs(want) + (2 * K + 16) * 2.0 ** -53 * A
    err = np.abs(got.astype(np.float64) - want)
    print(tag, "worst error / bound", float((err / np.maximum(bound, 1e-300)).max()), "differs from the sequential float32 in",
          int((got != want32).sum()), "of", got.size)
    assert (err <= bound).all(), (tag, first_diff(got, want32))


def _x_of(totals, g):
    adm = totals != np.uint64(ref.U64)
    best = int(totals[adm].min())
    return adm, np.array([float(int(t) - best) + float(v) if a else np.inf for t, v, a in zip(totals, g, adm)])


CASES = [(1, 1, DIFF, False), (2, 20, OMNI, True), (63, 7, DIFF, True), (64, 64, OMNI, False), (65, 130, OMNI, True),
         (256, 56, DIFF, False), (257, 33, OMNI, False)]   # (K, P, model, shift): K from 1 to 257, P * C from 2 to 390


@pytest.mark.parametrize("K,P,model,shift", CASES, ids=["%dx%d" % c[:2] for c in CASES])
def test_control_cost_update_equals_the_reference(gvamd, scene, K, P, model, shift):
    h = scene
    lam, gamma = 500.0, 20.0
    old, cfg = _mppi_setup(h, gvamd, model, P, lam, seed=K)
    lim = _limits(gvamd, model, gamma)
    h.set_mppi_limits(lim)
    first = None
    for rep in range(3):
        h.mppi_set_nominal(old)
        r, t, nom = _three_calls(h, K, 7, 3, ALL_ON, gvamd, shift=shift)
        u, g = h.controls_array(), h.mppi_control_costs()
        assert nom.tobytes() == h.mppi_nominal().tobytes()
        if first is None:
            first = (np.array([r]).tobytes(), t.tobytes(), nom.tobytes(), g.tobytes())
            want_g = gvamd.mppi_control_costs(cfg, lim, u, old, shift)
            assert g.dtype == np.float64 and g.tobytes() == want_g.tobytes(), first_diff(g, want_g)
            if K > 1:
                assert (g != 0).any()
            if K >= 63:
                assert 0 < r["n_valid"] and (t == np.uint64(ref.U64)).any() == (r["n_valid"] < K)
            _check_nominal(nom, lam, u, t, g, old, K, (K, P))
            if K == 1:
                assert nom.tobytes() == (u[0] if r["n_valid"] else old).tobytes()      # one trajectory: exact
            if r["n_valid"] > 1:
                plain = ref.average(lam, u, t, old)
                assert nom.tobytes() != plain.tobytes()                               # gamma shows in the nominal
        assert (np.array([r]).tobytes(), t.tobytes(), nom.tobytes(), g.tobytes()) == first, (rep, "the same calls, other bytes")
    # gamma 0 with the same limits: X11's update on the constrained controls, and the costs are gone
    h.set_mppi_limits(_limits(gvamd, model, 0.0))
    h.mppi_set_nominal(old)
    r0, t0, nom0 = _three_calls(h, K, 7, 3, ALL_ON, gvamd, shift=shift)
    assert h.controls_array().tobytes() == u.tobytes() and t0.tobytes() == t.tobytes()
    assert nom0.tobytes() == h.mppi_nominal().tobytes()
    if r0["n_valid"]:
        want32, want, A = ref.average(lam, u, t0, old, bound=True)
        assert (np.abs(nom0.astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + (2 * K + 16) * 2.0 ** -53 * A).all()
    assert _code(gvamd, h.mppi_control_costs) == GV_ERR_STATE


def test_control_cost_alone_and_beating_the_best_total(gvamd, scene):
    h = scene
    K, P, lam = 257, 33, 500.0
    # every critic weight zero: every admitted total is 0 and the weights are g's alone
    old, cfg = _mppi_setup(h, gvamd, DIFF, P, lam, seed=3)
    lim = _limits(gvamd, DIFF, 50.0)
    h.set_mppi_limits(lim)
    r, t, nom = _three_calls(h, K, 2, 1, rollout_ref.weights(), gvamd)
    u, g = h.controls_array(), h.mppi_control_costs()
    adm, x = _x_of(t, g)
    assert r["n_valid"] > 1 and (t[adm] == 0).all() and r["best"] == int(np.flatnonzero(adm)[0])
    assert g.tobytes() == gvamd.mppi_control_costs(cfg, lim, u, old).tobytes()
    assert np.array_equal(x[adm], g[adm]) and x[adm].min() < 0                      # m is a negative g
    _check_nominal(nom, lam, u, t, g, old, K, "zero weights")
    # a g negative enough to beat the best total: the trajectory that attains m is not `best`
    lim = _limits(gvamd, DIFF, 20000.0)
    h.set_mppi_limits(lim)
    h.mppi_set_nominal(old)
    r, t, nom = _three_calls(h, K, 2, 1, ALL_ON, gvamd)
    u, g = h.controls_array(), h.mppi_control_costs()
    adm, x = _x_of(t, g)
    print("best", int(r["best"]), "total", int(r["best_total"]), "argmin x", int(np.argmin(x)), "m", float(x.min()))
    assert int(np.argmin(x)) != int(r["best"]) and x.min() < 0 and int(t[np.argmin(x)]) > int(r["best_total"])
    assert g.tobytes() == gvamd.mppi_control_costs(cfg, lim, u, old).tobytes()
    _check_nominal(nom, lam, u, t, g, old, K, "g beats the best total")
    # a cold temperature: only the trajectory that attains m has a weight, and it is not the best total's
    if (x == x.min()).sum() == 1:
        old2, cfg2 = _mppi_setup(h, gvamd, DIFF, P, 1e-300, seed=3)
        r2, t2, nom2 = _three_calls(h, K, 2, 1, ALL_ON, gvamd)
        assert t2.tobytes() == t.tobytes() and nom2.tobytes() == u[int(np.argmin(x))].tobytes()


def test_nobody_admitted_keeps_the_nominal_and_writes_g(gvamd, scene):
    h = scene
    K = 65
    old, cfg = _mppi_setup(h, gvamd, OMNI, 20, 100.0)
    lim = _limits(gvamd, OMNI, 20.0)
    h.set_mppi_limits(lim)
    _three_calls(h, K, 9, 0, ALL_ON, gvamd)                                        # other costs in the buffer first
    stale = h.mppi_control_costs()
    h.mppi_set_nominal(old)
    r, t, nom = _three_calls(h, K, 1, 0, ALL_ON, gvamd, start=(1000.0, 1000.0, 0.0))   # off the map
    assert (r["best"], r["n_valid"], r["best_total"]) == (-1, 0, ref.U64) and (t == np.uint64(ref.U64)).all()
    assert nom.tobytes() == old.tobytes() == h.mppi_nominal().tobytes()
    g = h.mppi_control_costs()
    assert g.tobytes() == gvamd.mppi_control_costs(cfg, lim, h.controls_array(), old).tobytes() and g.tobytes() != stale.tobytes()


# --------------------------------------------------------------------------------------------------------- cycle --
def test_limits_off_equals_a_handle_that_never_set_them(gvamd, scene):
    hA, hB = scene, _new_scene_handle(gvamd)                                       # hB never sees gv_set_mppi_limits
    K, P = 257, 33
    out = {}
    for tag, h in (("never", hB), ("null", hA), ("neutral", hA)):
        old, cfg = _mppi_setup(h, gvamd, OMNI, P, 500.0, seed=5)
        if tag == "null":
            h.set_mppi_limits(_limits(gvamd, OMNI, 20.0))
            h.mppi_cycle(START, K, 4, 0, _cw(gvamd, ALL_ON))                       # limits and gamma on once
            h.mppi_set_nominal(old)
            h.set_mppi_limits(None)
        elif tag == "neutral":
            h.set_mppi_limits(gvamd.MppiLimits.of())
        r, t, nom = h.mppi_cycle(START, K, 4, 0, _cw(gvamd, ALL_ON))
        out[tag] = (h.controls_array().tobytes(), h.rollout_array().tobytes(), np.array([r]).tobytes(), t.tobytes(), nom.tobytes(),
                    h.mppi_nominal().tobytes())
        assert r["n_valid"] > 1 and nom.tobytes() != old.tobytes()
        assert _code(gvamd, h.mppi_control_costs) == GV_ERR_STATE
    assert out["null"] == out["never"] and out["neutral"] == out["never"]


@pytest.mark.parametrize("model", [DIFF, OMNI], ids=["diff", "omni"])
def test_cycle_equals_the_three_calls(gvamd, scene, model):
    h = scene
    K, P = 257, 33
    old, cfg = _mppi_setup(h, gvamd, model, P, 500.0, seed=5)
    lim = _limits(gvamd, model, 20.0)
    h.set_mppi_limits(lim)
    r, t, nom = _three_calls(h, K, 4, 0, ALL_ON, gvamd)
    u, poses, g = h.controls_array(), h.rollout_array(), h.mppi_control_costs()
    assert r["n_valid"] > 1 and nom.tobytes() != old.tobytes()
    h.mppi_set_nominal(old)
    assert (_unconstrained(h, K, 4, 0) != u).any()                                 # the limits bind here
    h.set_mppi_limits(lim)
    h.rollout(START, np.zeros((2, 2, rollout_ref.n_controls(model)), np.float32))  # something else in the rollout buffer
    for rep in range(3):
        h.mppi_set_nominal(old)
        r2, t2, nom2 = h.mppi_cycle(START, K, 4, 0, _cw(gvamd, ALL_ON))
        assert np.array([r2]).tobytes() == np.array([r]).tobytes() and t2.tobytes() == t.tobytes(), rep
        assert nom2.tobytes() == nom.tobytes() == h.mppi_nominal().tobytes(), rep
        assert h.controls_array().tobytes() == u.tobytes() and h.rollout_array().tobytes() == poses.tobytes(), rep
        assert h.mppi_control_costs().tobytes() == g.tobytes(), rep
    # the second cycle shifts: its control cost reads the nominal advanced by one step
    r3, t3, nom3 = h.mppi_cycle(START, K, 4, 1, _cw(gvamd, ALL_ON), shift=True)
    u3, g3 = h.controls_array(), h.mppi_control_costs()
    assert g3.tobytes() == gvamd.mppi_control_costs(cfg, lim, u3, nom, True).tobytes()
    assert g3.tobytes() != gvamd.mppi_control_costs(cfg, lim, u3, nom, False).tobytes()
    _check_nominal(nom3, 500.0, u3, t3, g3, nom, K, "second cycle")


def test_cycle_during_a_pending_tick(gvamd):
    """test_gpu_mppi.test_cycle_during_a_pending_tick with limits and gamma on: tick_enqueue, inflate, the cycle, tick_wait
    against a twin handle that does one thing after the other"""
    P5 = (0.5, 1.1, 5.0, 80)   # test_gpu_traj.P5
    hA, tfs = make_handle(gvamd, 2, perturbed=True)
    hB, _ = make_handle(gvamd, 2, perturbed=True)
    x, y, z, _, b = _ground_scene(tfs, seed=9)
    K, P = 129, 5
    start = (2.0, 0.7, 0.05)
    w = rollout_ref.weights(1, 2)
    nom = np.zeros((P, 2), np.float32)
    nom[:, 0] = 1.5
    cfg = gvamd.MppiConfig.of([0.5, 0.1], [0.0, -1.0], [3.0, 1.0], 200.0)
    lim = gvamd.MppiLimits.of([1.0, 0.5], [1.0, 0.5], [1.2, 0.0], 6.0, 10.0)
    pr, pt, pn = gvamd.PinnedI8(16), gvamd.PinnedI8(K * 8), gvamd.PinnedI8(P * 8)
    try:
        for h in (hA, hB):
            h.upload_xyz(x, y, z)
            h.tick(b, k_near=4, lidar_bin=True)
            h.set_inflation(*P5)
            h.set_footprint(tc.FOOTPRINTS["point"], collision_cost=254)
            h.set_motion_model(DIFF, 0.5)
            h.set_mppi(cfg)
            h.set_mppi_limits(lim)
            h.mppi_set_nominal(nom)
        for buf in (pr, pt, pn):
            buf.array[:] = 77
        hA.tick_enqueue(b, k_near=4, lidar_bin=True)
        hA.inflate()
        hA.mppi_cycle_async(start, K, 8, 0, _cw(gvamd, w), pr.array.view(rollout_ref.RESULT_DTYPE), pt.array.view(np.uint64),
                            pn.array.view(np.float32))
        hA.tick_wait()
        hA.synchronize()
        hB.tick(b, k_near=4, lidar_bin=True)
        hB.inflate()
        twin_r, twin_t, twin_n = hB.mppi_cycle(start, K, 8, 0, _cw(gvamd, w))
        assert twin_r["n_valid"] > 1
        assert pr.array.tobytes() == np.array([twin_r]).tobytes()
        assert pt.array.tobytes() == twin_t.tobytes() and pn.array.tobytes() == twin_n.tobytes()
        assert hA.mppi_nominal().tobytes() == twin_n.tobytes() and hA.controls_array().tobytes() == hB.controls_array().tobytes()
        assert hA.mppi_control_costs().tobytes() == hB.mppi_control_costs().tobytes()
    finally:
        pr.close(); pt.close(); pn.close()
        hA.close(); hB.close()


def _unconstrained(h, K, seed, it):
    """f of a sampling on h: the limits off for one call.  The caller is done with h's limits."""
    h.set_mppi_limits(None)
    h.mppi_sample(K, seed, it)
    return h.controls_array()


# --------------------------------------------------------------------------------------------------------- rules --
def test_state_rules(gvamd, scene):
    h = scene
    lib = gvamd.load()
    code = lambda call: _code(gvamd, call)
    K, P = 8, 5
    h.set_mppi_limits(None)
    old, cfg = _mppi_setup(h, gvamd, OMNI, P, 50.0)
    cw = _cw(gvamd, ALL_ON)
    # a radius under OMNI: refused at the sampling and at the cycle, nothing enqueued
    h.mppi_sample(K, 1, 0)
    before = (h.controls_array().tobytes(), h.device_controls())
    h.set_mppi_limits(gvamd.MppiLimits.of(min_turn_radius=1.0))                   # the setter cannot know the model
    assert code(lambda: h.mppi_sample(K + 1, 1, 1)) == GV_ERR_STATE
    assert "GV_MOTION_DIFF" in (lib.gv_last_error(h._h) or b"").decode()
    assert code(lambda: h.mppi_sample(K + 1, 1, 1, wait=False)) == GV_ERR_STATE
    assert code(lambda: h.mppi_cycle(START, K + 1, 1, 1, cw)) == GV_ERR_STATE
    assert (h.controls_array().tobytes(), h.device_controls()) == before and h.mppi_nominal().tobytes() == old.tobytes()
    h.set_motion_model(DIFF, 0.25)
    h.mppi_set_nominal(old[:, :2].copy())
    h.mppi_sample(K, 1, 0)                                                        # fine under DIFF
    h.set_motion_model(OMNI, 0.25)
    h.mppi_set_nominal(old)
    # the getter before a gamma update
    h.set_mppi_limits(None)
    h.mppi_cycle(START, K, 1, 0, cw)
    out = np.zeros(K)
    assert lib.gv_get_mppi_control_costs(h._h, out.ctypes.data_as(C.c_void_p)) == GV_ERR_STATE
    assert lib.gv_get_mppi_control_costs(h._h, None) == GV_ERR_BAD_ARG
    # a rejected struct keeps the old one
    good = _limits(gvamd, OMNI, 20.0)
    h.set_mppi_limits(good)
    h.mppi_set_nominal(old)
    want = h.mppi_cycle(START, K, 1, 0, cw)
    want = (want[2].tobytes(), h.controls_array().tobytes(), h.mppi_control_costs().tobytes())
    for bad in (gvamd.MppiLimits.of([-1.0]), gvamd.MppiLimits.of([1.0, NAN]), gvamd.MppiLimits.of([1.0] * 3, [1.0, 1.0, -0.5]),
                gvamd.MppiLimits.of(min_turn_radius=-1.0), gvamd.MppiLimits.of(min_turn_radius=INF), gvamd.MppiLimits.of(gamma=-1.0),
                gvamd.MppiLimits.of(gamma=NAN), gvamd.MppiLimits.of(flags=1)):
        assert code(lambda: h.set_mppi_limits(bad)) == GV_ERR_BAD_ARG
    assert lib.gv_set_mppi_limits(None, C.byref(good)) == GV_ERR_BAD_ARG
    h.mppi_set_nominal(old)
    got = h.mppi_cycle(START, K, 1, 0, cw)
    assert (got[2].tobytes(), h.controls_array().tobytes(), h.mppi_control_costs().tobytes()) == want
    u = h.controls_array()
    h.mppi_set_nominal(old)
    f = _unconstrained(h, K, 1, 0)
    assert u.tobytes() == gvamd.mppi_constrain(good, gvamd.MotionModel(OMNI, 0.25, 0), f).tobytes() != f.tobytes()


def test_limits_survive_reset(gvamd):
    (gx, gy, res), _ = tc.GRIDS["250x100"]
    h = gvamd.GridVisionHIP(gx, gy, res)
    try:
        K, P = 8, 5
        nom = np.zeros((P, 2), np.float32)
        nom[:, 0] = 1.0
        h.set_motion_model(DIFF, 0.2)
        h.set_mppi(gvamd.MppiConfig.of([0.3, 0.2], [-1.0, -1.0], [2.0, 1.0], 50.0))
        h.mppi_set_nominal(nom)
        h.mppi_sample(K, 1, 0)
        f = h.controls_array()
        lim = gvamd.MppiLimits.of([1.0, 1.0], [1.0, 1.0], [0.8, 0.0], 2.0)
        h.set_mppi_limits(lim)
        h.mppi_sample(K, 1, 0)
        got = h.controls_array()
        assert got.tobytes() == gvamd.mppi_constrain(lim, gvamd.MotionModel(DIFF, 0.2, 0), f).tobytes() != f.tobytes()
        h.reset()
        plant(h, np.random.default_rng(5).random((h.ny, h.nx)) < 1e-3, INFLATION)     # gv_set_log_odds
        h.mppi_sample(K, 1, 0)
        assert h.controls_array().tobytes() == got.tobytes()
    finally:
        h.close()


def test_mppi_limits_demo(gvamd, tmp_path):
    """examples/mppi_limits_demo.cpp (plain g++ over the C ABI): mppi_demo's scene for a car-like base, ten gv_mppi_cycle
    calls with limits and gamma, trajectory 0 checked against the limits after each, and the host replay of the last
    average"""
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "grid-vision_amd")
    exe = str(tmp_path / "mppi_limits_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(pkg, "examples", "mppi_limits_demo.cpp"), "-o", exe,
                           "-L" + pkg, "-lgridvision_hip", "-Wl,-rpath," + pkg])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    its = re.findall(r"iteration (\d) admitted (\d+) best (-?\d+) total (\d+) trajectory 0: .* violations (\d+)\n", out.stdout)
    assert [int(i[0]) for i in its] == list(range(10)) and all(0 < int(i[1]) <= 512 and int(i[4]) == 0 for i in its), out.stdout
    assert "control costs equal the host's" in out.stdout
    assert re.search(r"limits check ok \(0 violations, 0 mismatches\)", out.stdout), out.stdout
