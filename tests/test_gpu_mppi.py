"""[EXTENSION] X11 MPPI sampling and softmax update on the device.

Sampling: gv_mppi_sample against the library's host twin gv_mppi_sample_controls (which test_mppi_host.py holds to
mppi_ref byte for byte).  The two differ in the library that computes log, sin and cos, in the last bit of an fp64 value;
every component must equal the twin's or be one of its two float32 neighbours, and at most 1e-4 of a family's components
may be a neighbour -- the cap of test_gpu_rollout.py, for the same reason: a last-bit fp64 difference reaches a float32
only near a rounding midpoint.  That argument needs v = nominal + sigma * z not to cancel: each family first satisfies
min |v| / |sigma z| >= 2^-24 (mppi_ref computes both), so a last-bit difference of sigma * z moves v by less than a
float32 step.  Row 0 and sigma = 0 do not depend on the libm and are compared by bytes.

Update: result and totals by bytes against gv_control_step on the same rollout; the new nominal against mppi_ref.average
fed the device's own read-backs (controls_array(), the totals).  With want the reference's fp64 quotient N / S,
  |got - want| <= 2^-24 |want| + (2 K + 16) 2^-53 A,   A = sum e_k |u| / S:
the float32 rounding of the device's own quotient, and the standard bound of a reordered fp64 sum of K terms in numerator
and denominator plus an ulp of exp.  The cases that do not depend on the order of the sums are compared by bytes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mppi_ref as ref
import rollout_ref
import traj_cases as tc
from planner_util import first_diff, plant
from test_gpu_parity import _ground_scene, make_handle

pytestmark = pytest.mark.gpu

GV_ERR_BAD_ARG, GV_ERR_STATE = 1, 5
DIFF, OMNI = rollout_ref.DIFF, rollout_ref.OMNI
INFLATION = (0.35, 0.55, 10.0, 65)      # test_gpu_rollout.INFLATION[0.1]
GRID = "500x200"
NEIGHBOUR_CAP = 1e-4
SHAPES = [(1, 130), (3, 64), (64, 63), (65, 65), (257, 2), (65, 1)]   # (K, P): rollout_cases.SHAPES
START = (2.0, 0.3, 0.1)
SEEDS = np.array([(30.0 - 0.5 * i, -2.0 + 0.1 * i) for i in range(40)], np.float32)   # test_gpu_rollout.SEEDS
ALL_ON = rollout_ref.weights(3, 7, 11, 13, 17)
INF = float("inf")
_HANDLES = {}
_SCENE = {}


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    yield m
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()
    _SCENE.clear()


def _handle(gvamd, grid=GRID):
    if grid not in _HANDLES:
        (gx, gy, res), (nx, ny) = tc.GRIDS[grid]
        h = gvamd.GridVisionHIP(gx, gy, res)
        assert (h.nx, h.ny) == (nx, ny)
        _HANDLES[grid] = h
    return _HANDLES[grid]


def _scene_handle(gvamd):
    """the 500 x 200 handle with planted obstacles, the costmap, a footprint and the field: made once"""
    h = _handle(gvamd)
    if GRID not in _SCENE:
        h.reset()
        mask = np.random.default_rng(17).random((h.ny, h.nx)) < 5e-4
        plant(h, mask, INFLATION)
        h.set_footprint(tc.FOOTPRINTS["triangle"])
        h.set_nav_config(253, 2)
        h.nav_field(SEEDS)
        _SCENE[GRID] = True
    return h


def _code(gvamd, call):
    with pytest.raises(gvamd.GVError) as e:
        call()
    return e.value.code


def _cw(gvamd, w, flags=0):
    return gvamd.CriticWeights(*[w[n] for n in rollout_ref.WEIGHTS], flags)


def _nominal(P, Cn, seed=0, base=0.3):
    rng = np.random.default_rng(100 + seed)
    return (base + rng.uniform(-0.05, 0.05, (P, Cn))).astype(np.float32)


def _neighbours(got, want, tag):
    """every component equal or a float32 neighbour; returns (components, neighbours)"""
    assert got.dtype == np.float32 and got.shape == want.shape, tag
    g, w = got.reshape(-1), want.reshape(-1)
    same = g.view(np.uint32) == w.view(np.uint32)
    near = (g == np.nextafter(w, np.float32(np.inf))) | (g == np.nextafter(w, np.float32(-np.inf)))
    assert (same | near).all(), (tag, first_diff(g[~(same | near)], w[~(same | near)]))
    return int(g.size), int((~same).sum())


# ------------------------------------------------------------------------------------------------------ sampling --
SIGMA, LO, HI = [0.2, 0.2, 0.2], [-0.1, -0.5, 0.1], [0.6, 0.9, 0.45]


@pytest.mark.parametrize("shift", [False, True], ids=["plain", "shift"])
@pytest.mark.parametrize("model", [DIFF, OMNI], ids=["diff", "omni"])
def test_sampling_equals_the_host_twin(gvamd, model, shift):
    h = _handle(gvamd)
    Cn = rollout_ref.n_controls(model)
    cfg = gvamd.MppiConfig.of(SIGMA[:Cn], LO[:Cn], HI[:Cn], 1.0)
    h.set_motion_model(model, 0.1)
    h.set_mppi(cfg)
    n = near = 0
    for i, (K, P) in enumerate(SHAPES):
        seed, it = 1 + i % 3, 5 + i
        nom = _nominal(P, Cn, i)
        _, v, noise = ref.sample(SIGMA, LO[:Cn], HI[:Cn], nom, K, seed, it, ref.SHIFT if shift else 0, parts=True)
        if K > 1:
            guard = (v[1:] / noise[1:]).min()
            print("cancellation guard", K, P, "2^%.1f" % np.log2(guard))
            assert guard >= 2.0 ** -24, (K, P, guard)
        want = gvamd.mppi_sample_controls(cfg, nom, K, seed, it, shift)
        h.mppi_set_nominal(nom)
        assert h.mppi_nominal().tobytes() == nom.tobytes()
        first = None
        for rep in range(3):
            h.mppi_sample(K, seed, it, shift, wait=rep != 1)
            got = h.controls_array()
            a, b = _neighbours(got, want, (K, P, rep))
            if first is None:
                first, n, near = got.tobytes(), n + a, near + b
            assert got.tobytes() == first, (K, P, rep, "the same call, other bytes")
        assert h.device_controls()[1:] == (K, P, Cn)
        assert got[0].tobytes() == want[0].tobytes()                  # row 0: the clamped nominal, no libm
        if K > 1:
            h.mppi_sample(K, seed, it + 1, shift)
            other = h.controls_array()
            assert other[0].tobytes() == got[0].tobytes() and (other[1:] != got[1:]).any()   # another iteration
            _neighbours(other, gvamd.mppi_sample_controls(cfg, nom, K, seed, it + 1, shift), (K, P, "next"))
    print("neighbour share", model, shift, near, "of", n)
    assert near <= NEIGHBOUR_CAP * n, (near, n)


def test_sigma_zero_and_clamps_are_exact(gvamd):
    h = _handle(gvamd)
    h.set_motion_model(OMNI, 0.1)
    K, P = 65, 64
    nom = _nominal(P, 3, 1)
    for lo, hi in (([-INF] * 3, [INF] * 3), ([-INF, 0.29, -INF], [INF, INF, 0.31]), ([0.3, 0.25, -1.0], [0.3, 0.25, 1.0])):
        cfg = gvamd.MppiConfig.of([0.0] * 3, lo, hi, 1.0)
        h.set_mppi(cfg)
        h.mppi_set_nominal(nom)
        h.mppi_sample(K, 3, 9)
        got = h.controls_array()
        row = np.clip(nom, np.float32(lo), np.float32(hi)).astype(np.float32)
        assert all(got[k].tobytes() == row.tobytes() for k in range(K)), (lo, hi)
    # a clamp that cuts about half: where the host twin clamps the device clamps (the clamp value itself is exact)
    cfg = gvamd.MppiConfig.of([0.2] * 3, [-INF, 0.25, 0.3], [INF, 0.25, INF], 1.0)
    flat = np.full((P, 3), 0.3, np.float32)
    h.set_mppi(cfg)
    h.mppi_set_nominal(flat)
    h.mppi_sample(K, 2, 0)
    got, want = h.controls_array(), gvamd.mppi_sample_controls(cfg, flat, K, 2, 0)
    _neighbours(got, want, "half")
    assert (got[:, :, 1] == np.float32(0.25)).all() and (got[:, :, 2] >= np.float32(0.3)).all()
    assert 0.4 < (got[1:, :, 2] == np.float32(0.3)).mean() < 0.6


# -------------------------------------------------------------------------------------------------------- update --
def _mppi_setup(h, gvamd, model, P, lam, dt=None, sigma=(0.5, 0.3, 0.3), seed=0):
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


def _three_calls(h, K, seed, it, w, gvamd, start=START, shift=False):
    h.mppi_sample(K, seed, it, shift)
    ptr, k, P, Cn = h.device_controls()
    assert k == K
    h.rollout(start, (K, P, Cn), device_ptr=ptr)
    step_r, step_t = h.control_step(_cw(gvamd, w), keep_totals=True)
    r, t, nom = h.mppi_update(_cw(gvamd, w))
    assert np.array([r]).tobytes() == np.array([step_r]).tobytes() and t.tobytes() == step_t.tobytes()
    return r, t, nom


def _check_nominal(got, lam, controls, totals, old, K, tag):
    want32, want, A = ref.average(lam, controls, totals, old, bound=True)
    bound = 2.0 ** -24 * np.abs(want) + (2 * K + 16) * 2.0 ** -53 * A
    err = np.abs(got.astype(np.float64) - want)
    print(tag, "worst error / bound", float((err / np.maximum(bound, 1e-300)).max()), "differs from the sequential float32 in",
          int((got != want32).sum()), "of", got.size)
    assert (err <= bound).all(), (tag, first_diff(got, want32))


CASES = [(1, 1, DIFF), (2, 20, OMNI), (63, 7, DIFF), (64, 64, OMNI), (65, 130, OMNI), (255, 20, DIFF), (256, 56, DIFF),
         (257, 33, OMNI), (1025, 20, DIFF), (4097, 130, OMNI)]   # (K, P, model): P * C from 2 to 390


@pytest.mark.parametrize("K,P,model", CASES, ids=["%dx%d" % c[:2] for c in CASES])
def test_update_equals_the_reference(gvamd, K, P, model):
    h = _scene_handle(gvamd)
    lam = 500.0
    old, cfg = _mppi_setup(h, gvamd, model, P, lam, seed=K)
    first = None
    for rep in range(3):
        h.mppi_set_nominal(old)
        r, t, nom = _three_calls(h, K, 7, 3, ALL_ON, gvamd)
        u = h.controls_array()
        assert nom.tobytes() == h.mppi_nominal().tobytes()
        if first is None:
            first = (np.array([r]).tobytes(), t.tobytes(), nom.tobytes())
            if K >= 63:
                assert 0 < r["n_valid"] and (t == np.uint64(ref.U64)).any() == (r["n_valid"] < K)
            _check_nominal(nom, lam, u, t, old, K, (K, P))
            if K == 1:
                assert nom.tobytes() == (u[0] if r["n_valid"] else old).tobytes()      # one trajectory: exact
            lo, hi = np.float32(-0.5), np.float32(2.5)
            assert (nom >= lo).all() and (nom <= hi).all()
        assert (np.array([r]).tobytes(), t.tobytes(), nom.tobytes()) == first, (rep, "the same calls, other bytes")


@pytest.mark.parametrize("lam", [1e-300, 1e300, 1.0])
def test_update_extreme_temperatures_and_zero_weights(gvamd, lam):
    h = _scene_handle(gvamd)
    K, P = 257, 33
    for w in (ALL_ON, rollout_ref.weights()):                      # every weight zero: every admitted total is 0
        old, cfg = _mppi_setup(h, gvamd, DIFF, P, lam, seed=3)
        r, t, nom = _three_calls(h, K, 2, 1, w, gvamd)
        u = h.controls_array()
        assert r["n_valid"] > 1
        _check_nominal(nom, lam, u, t, old, K, (lam, w["w_cost_sum"]))
        adm = t != np.uint64(ref.U64)
        if lam == 1e-300 and (t[adm] == r["best_total"]).sum() == 1:
            assert nom.tobytes() == u[int(r["best"])].tobytes()    # only the best has a weight: exact
        if not any(w.values()):
            assert (t[adm] == 0).all() and r["best"] == int(np.flatnonzero(adm)[0])
            mean = u[adm].astype(np.float64).sum(axis=0) / adm.sum()
            A = np.abs(u[adm]).astype(np.float64).sum(axis=0) / adm.sum()
            assert (np.abs(nom - mean) <= 2.0 ** -24 * np.abs(mean) + (2 * K + 16) * 2.0 ** -53 * A).all()


def test_every_trajectory_rejected(gvamd):
    h = _scene_handle(gvamd)
    old, cfg = _mppi_setup(h, gvamd, OMNI, 20, 100.0)
    r, t, nom = _three_calls(h, 65, 1, 0, ALL_ON, gvamd, start=(1000.0, 1000.0, 0.0))   # off the map
    assert (r["best"], r["n_valid"], r["best_total"]) == (-1, 0, ref.U64) and (t == np.uint64(ref.U64)).all()
    assert nom.tobytes() == old.tobytes() == h.mppi_nominal().tobytes()


def test_cycle_equals_the_three_calls_and_shift_reads_its_nominal(gvamd):
    h = _scene_handle(gvamd)
    K, P = 257, 33
    old, cfg = _mppi_setup(h, gvamd, OMNI, P, 500.0, seed=5)
    r, t, nom = _three_calls(h, K, 4, 0, ALL_ON, gvamd)
    u, poses = h.controls_array(), h.rollout_array()
    assert r["n_valid"] > 1 and nom.tobytes() != old.tobytes()
    h.mppi_set_nominal(old)
    h.rollout(START, np.zeros((2, 2, 3), np.float32))              # something else in the rollout buffer
    for rep in range(3):
        h.mppi_set_nominal(old)
        r2, t2, nom2 = h.mppi_cycle(START, K, 4, 0, _cw(gvamd, ALL_ON))
        assert np.array([r2]).tobytes() == np.array([r]).tobytes() and t2.tobytes() == t.tobytes(), rep
        assert nom2.tobytes() == nom.tobytes() == h.mppi_nominal().tobytes(), rep
        assert h.controls_array().tobytes() == u.tobytes() and h.rollout_array().tobytes() == poses.tobytes(), rep
        assert h.device_rollout()[1:] == (K, P)
    # the second cycle samples around the first one's nominal, advanced by one step
    r3, t3, nom3 = h.mppi_cycle(START, K, 4, 1, _cw(gvamd, ALL_ON), shift=True)
    u3 = h.controls_array()
    want = gvamd.mppi_sample_controls(cfg, nom, K, 4, 1, shift=True)
    _neighbours(u3, want, "shift")
    pn = np.minimum(np.arange(P) + 1, P - 1)
    assert u3[0].tobytes() == np.clip(nom[pn], np.float32(-0.5), np.float32(2.5)).astype(np.float32).tobytes()
    _check_nominal(nom3, 500.0, u3, t3, nom, K, "second cycle")
    assert h.mppi_cycle(START, 0, 4, 2, _cw(gvamd, ALL_ON))[2].tobytes() == np.zeros_like(nom).tobytes()   # K == 0: nothing runs
    assert h.mppi_nominal().tobytes() == nom3.tobytes() and h.device_controls()[1] == K


def test_destinations(gvamd):
    """result, totals and nominal_out into pinned memory (written by a kernel), into pinned memory that is not aligned and
    into pageable memory (copy commands), and no nominal_out at all (the read-back)"""
    h = _scene_handle(gvamd)
    K, P = 65, 20
    old, cfg = _mppi_setup(h, gvamd, DIFF, P, 500.0, seed=9)
    want_r, want_t, want_n = _three_calls(h, K, 6, 0, ALL_ON, gvamd)
    want_r = np.array([want_r]).tobytes()
    assert want_n.tobytes() != old.tobytes()
    pin_r, pin_t, pin_n = gvamd.PinnedI8(32), gvamd.PinnedI8(K * 8 + 8), gvamd.PinnedI8(P * 2 * 4 + 8)
    try:
        for rep in range(2):
            for off_r, off_t, off_n in ((0, 0, 0), (8, 4, 4), (0, 4, 0), (8, 0, 4)):
                for buf in (pin_r, pin_t, pin_n):
                    buf.array[:] = 77
                res = pin_r.array[off_r:off_r + 16].view(rollout_ref.RESULT_DTYPE)
                tot = pin_t.array[off_t:off_t + K * 8].view(np.uint64)
                non = pin_n.array[off_n:off_n + P * 8].view(np.float32)
                h.mppi_set_nominal(old)
                h.mppi_update_async(_cw(gvamd, ALL_ON), res, tot, non)
                h.synchronize()
                assert res.tobytes() == want_r and tot.tobytes() == want_t.tobytes() and non.tobytes() == want_n.tobytes(), (rep, off_r, off_t, off_n)
                for buf in (pin_r, pin_t, pin_n):
                    buf.array[:] = 77
                h.mppi_set_nominal(old)
                h.mppi_update_async(_cw(gvamd, ALL_ON), res)
                h.synchronize()
                assert res.tobytes() == want_r and (pin_t.array == 77).all() and (pin_n.array == 77).all()
                assert h.mppi_nominal().tobytes() == want_n.tobytes()
            res, tot, non = np.full(1, 7, rollout_ref.RESULT_DTYPE), np.full(K, 7, np.uint64), np.full(P * 2, 7, np.float32)
            h.mppi_set_nominal(old)
            h.mppi_cycle_async(START, K, 6, 0, _cw(gvamd, ALL_ON), res, tot, non)
            h.synchronize()
            assert res.tobytes() == want_r and tot.tobytes() == want_t.tobytes() and non.tobytes() == want_n.tobytes(), (rep, "pageable")
    finally:
        pin_r.close(); pin_t.close(); pin_n.close()


def test_cycle_during_a_pending_tick(gvamd):
    """tick_enqueue, inflate, the cycle, tick_wait against a twin handle that does one thing after the other: the cycle
    reads the costmap of the tick's grid"""
    P5 = (0.5, 1.1, 5.0, 80)   # test_gpu_traj.P5
    hA, tfs = make_handle(gvamd, 2, perturbed=True)
    hB, _ = make_handle(gvamd, 2, perturbed=True)
    x, y, z, _, b = _ground_scene(tfs, seed=9)
    K, P = 129, 5                         # few poses: the tick's second layer of returns leaves some trajectories admitted
    start = (2.0, 0.7, 0.05)
    w = rollout_ref.weights(1, 2)
    nom = np.zeros((P, 2), np.float32)
    nom[:, 0] = 1.5                       # a few metres ahead of the base
    cfg = gvamd.MppiConfig.of([0.5, 0.1], [0.0, -1.0], [3.0, 1.0], 200.0)
    pr, pt, pn = gvamd.PinnedI8(16), gvamd.PinnedI8(K * 8), gvamd.PinnedI8(P * 8)
    try:
        for h in (hA, hB):
            h.upload_xyz(x, y, z)
            h.tick(b, k_near=4, lidar_bin=True)
            h.set_inflation(*P5)
            h.set_footprint(tc.FOOTPRINTS["point"], collision_cost=254)   # only a lethal centre cell rejects
            h.set_motion_model(DIFF, 0.5)
            h.set_mppi(cfg)
            h.mppi_set_nominal(nom)
        hB.inflate()
        hB.mppi_sample(K, 8, 0)
        hB.rollout(start, (K, P, 2), device_ptr=hB.device_controls()[0])
        stale_t = hB.control_step(_cw(gvamd, w), keep_totals=True)[1]
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
        print("admitted on the stale costmap", int((stale_t != np.uint64(ref.U64)).sum()), "on the tick's", int(twin_r["n_valid"]), "of", K)
        assert twin_t.tobytes() != stale_t.tobytes()
        assert pr.array.tobytes() == np.array([twin_r]).tobytes()
        assert pt.array.tobytes() == twin_t.tobytes() and pn.array.tobytes() == twin_n.tobytes()
        assert hA.mppi_nominal().tobytes() == twin_n.tobytes() and hA.controls_array().tobytes() == hB.controls_array().tobytes()
    finally:
        pr.close(); pt.close(); pn.close()
        hA.close(); hB.close()


# --------------------------------------------------------------------------------------------------------- rules --
def test_state_and_argument_rules(gvamd):
    (gx, gy, res), _ = tc.GRIDS["250x100"]
    h = gvamd.GridVisionHIP(gx, gy, res)
    lib = gvamd.load()
    code = lambda call: _code(gvamd, call)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    null = C.c_void_p(None)
    K, P = 8, 5
    nom = np.zeros((P, 2), np.float32)
    nom[:, 0] = 1.0
    good = gvamd.MppiConfig.of([0.3, 0.2], [-1.0, -1.0], [2.0, 1.0], 50.0)
    cw = _cw(gvamd, rollout_ref.weights(1, 1))
    start = (5.0, 1.0, 0.3)
    rbuf, tot, nout = np.zeros(1, rollout_ref.RESULT_DTYPE), np.zeros(K, np.uint64), np.zeros(P * 2, np.float32)

    def update(w=cw, flags=0, r=rbuf, t=None, n=None, fn=lib.gv_mppi_update, hh=h._h):
        return fn(hh, C.byref(w) if w is not None else None, C.c_uint32(flags), p(r), p(t), p(n))

    def cycle(start_=start, K_=K, sflags=0, w=cw, flags=0, r=rbuf, t=None, n=None, fn=lib.gv_mppi_cycle, hh=h._h):
        s = (C.c_double * 3)(*start_) if start_ is not None else None
        return fn(hh, s, C.c_int32(K_), C.c_uint64(1), C.c_uint64(0), C.c_uint32(sflags), C.byref(w) if w is not None else None,
                  C.c_uint32(flags), p(r), p(t), p(n))

    def sample(K_=K, flags=0, fn=lib.gv_mppi_sample, hh=h._h):
        return fn(hh, C.c_int32(K_), C.c_uint64(1), C.c_uint64(0), C.c_uint32(flags))

    try:
        # ---- configuration: a rejected one leaves the one in force alone
        assert lib.gv_set_mppi(null, C.byref(good)) == GV_ERR_BAD_ARG
        for bad in (gvamd.MppiConfig.of([-0.1, 0.2]), gvamd.MppiConfig.of([INF, 0.2]), gvamd.MppiConfig.of([0.1, 0.1], [1.0, 0.0], [0.0, 1.0]),
                    gvamd.MppiConfig.of([0.1, 0.1], [float("nan"), 0.0], [1.0, 1.0]), gvamd.MppiConfig.of([0.1, 0.1], lambda_=0.0),
                    gvamd.MppiConfig.of([0.1, 0.1], lambda_=INF), gvamd.MppiConfig.of([0.1, 0.1], flags=1),
                    gvamd.MppiConfig.of([0.1, 0.1, -1.0])):
            assert code(lambda: h.set_mppi(bad)) == GV_ERR_BAD_ARG
        # ---- the nominal and the sampling
        assert lib.gv_mppi_set_nominal(h._h, p(nom), C.c_int32(P)) == GV_ERR_STATE      # no motion model
        assert lib.gv_get_mppi_nominal(h._h, p(nout), None) == GV_ERR_STATE
        h.set_motion_model(DIFF, 0.2)
        assert sample() == GV_ERR_STATE                                                 # no configuration
        h.set_mppi(good)
        assert sample() == GV_ERR_STATE and "no nominal" in (lib.gv_last_error(h._h) or b"").decode()
        assert lib.gv_mppi_set_nominal(h._h, None, C.c_int32(P)) == lib.gv_mppi_set_nominal(h._h, p(nom), C.c_int32(0)) == GV_ERR_BAD_ARG
        assert lib.gv_mppi_set_nominal(h._h, p(nom), C.c_int32(4097)) == lib.gv_mppi_set_nominal(null, p(nom), C.c_int32(P)) == GV_ERR_BAD_ARG
        for v in (float("nan"), INF):
            bad = nom.copy(); bad[2, 1] = v
            assert lib.gv_mppi_set_nominal(h._h, p(bad), C.c_int32(P)) == GV_ERR_BAD_ARG
        h.mppi_set_nominal(nom)
        assert lib.gv_get_mppi_nominal(h._h, None, None) == lib.gv_get_mppi_nominal(null, p(nout), None) == GV_ERR_BAD_ARG
        assert code(h.device_controls) == GV_ERR_STATE and lib.gv_get_controls(h._h, p(np.zeros(80, np.float32))) == GV_ERR_STATE
        assert sample(K_=-1) == sample(K_=(1 << 20) + 1) == sample(flags=2) == sample(hh=null) == GV_ERR_BAD_ARG
        assert sample(fn=lib.gv_mppi_sample_async, flags=2) == GV_ERR_BAD_ARG
        assert sample(K_=0) == 0 and code(h.device_controls) == GV_ERR_STATE              # K == 0: a successful no-op
        assert sample() == 0
        ptr, k, pp, cc = h.device_controls()
        assert (k, pp, cc) == (K, P, 2) and ptr
        got = h.controls_array()
        assert got.tobytes() != np.zeros_like(got).tobytes()
        assert lib.gv_device_controls(h._h, None, None, None, None) == lib.gv_get_controls(h._h, None) == GV_ERR_BAD_ARG
        assert lib.gv_get_controls(null, p(got)) == GV_ERR_BAD_ARG
        for bad in (gvamd.MppiConfig.of([-0.1, 0.2]), gvamd.MppiConfig.of([0.1, 0.1], lambda_=-1.0)):
            assert code(lambda: h.set_mppi(bad)) == GV_ERR_BAD_ARG
        assert sample() == 0 and h.controls_array().tobytes() == got.tobytes()           # the old configuration is in force
        assert sample(K_=4) == 0 and h.device_controls() == (ptr, 4, P, 2)               # a smaller sampling keeps the pointer
        assert h.controls_array().tobytes() == got[:4].tobytes()
        h.reset()                                                                       # the buffers and the configuration stay
        assert h.device_controls() == (ptr, 4, P, 2) and h.mppi_nominal().tobytes() == nom.tobytes()
        assert sample() == 0 and h.controls_array().tobytes() == got.tobytes()
        assert sample(K_=300) == 0 and h.device_controls()[1:] == (300, P, 2)            # a larger one may move it
        assert h.controls_array()[:K].tobytes() == got.tobytes()
        h.set_motion_model(OMNI, 0.2)
        assert sample() == GV_ERR_STATE and cycle() == GV_ERR_STATE                      # the nominal has another C
        h.set_motion_model(DIFF, 0.2)
        assert sample() == 0
        # ---- the update and the cycle
        assert update() == cycle() == GV_ERR_STATE                                      # no footprint
        h.set_footprint(tc.FOOTPRINTS["triangle"])
        assert update() == GV_ERR_STATE and "no rollout" in (lib.gv_last_error(h._h) or b"").decode()
        assert cycle() == GV_ERR_STATE                                                  # no costmap
        plant(h, np.random.default_rng(5).random((h.ny, h.nx)) < 1e-3, INFLATION)
        assert h.controls_array().tobytes() == got.tobytes() and h.mppi_nominal().tobytes() == nom.tobytes()   # gv_set_log_odds kept them
        assert update() == GV_ERR_STATE                                                 # still no rollout
        h.rollout(start, np.zeros((K + 1, P, 2), np.float32))
        assert update() == GV_ERR_STATE                                                 # a rollout of another K
        h.rollout(start, (K, P, 2), device_ptr=h.device_controls()[0])
        step = h.control_step(cw, keep_totals=True)
        assert update(flags=1, t=tot, n=nout) == 0
        assert rbuf.tobytes() == np.array([step[0]]).tobytes() and tot.tobytes() == step[1].tobytes()
        assert nout.tobytes() == h.mppi_nominal().tobytes()
        assert update(w=_cw(gvamd, ALL_ON)) == cycle(w=_cw(gvamd, ALL_ON)) == GV_ERR_STATE   # a nav weight, no field
        h.set_nav_config(253, 1)
        h.nav_field(np.array([(8.0, 0.5), (9.0, 0.0), (10.0, -0.5)], np.float32))
        assert update(w=_cw(gvamd, ALL_ON)) == cycle(w=_cw(gvamd, ALL_ON)) == 0
        assert update(w=None) == update(r=None) == update(flags=2) == update(flags=1, t=None) == update(hh=null) == GV_ERR_BAD_ARG
        assert update(w=_cw(gvamd, ALL_ON, 1)) == update(fn=lib.gv_mppi_update_async, flags=2) == GV_ERR_BAD_ARG
        w = dict(ALL_ON); w["w_nav_sum"] = 65536
        assert update(w=_cw(gvamd, w)) == cycle(w=_cw(gvamd, w)) == GV_ERR_BAD_ARG
        assert cycle(start_=None) == cycle(K_=-1) == cycle(K_=(1 << 20) + 1) == cycle(sflags=2) == cycle(flags=2) == GV_ERR_BAD_ARG
        assert cycle(w=None) == cycle(r=None) == cycle(flags=1, t=None) == cycle(hh=null) == GV_ERR_BAD_ARG
        assert cycle(start_=(0.0, float("nan"), 0.0)) == cycle(fn=lib.gv_mppi_cycle_async, start_=(INF, 0.0, 0.0)) == GV_ERR_BAD_ARG
        assert cycle(K_=0) == 0 and update(t=tot) == 0                                   # totals ignored without the flag
        h.mppi_set_nominal(np.zeros((P + 1, 2), np.float32))
        assert update() == GV_ERR_STATE                                                 # a nominal of another P
        assert cycle() == 0 and update() == 0                                           # the cycle samples P + 1 steps itself
        h.set_mppi(None)
        assert update() == cycle() == sample() == GV_ERR_STATE                           # NULL turns the configuration off
        h.set_mppi(good)
        h.set_footprint(None)
        assert update() == cycle() == GV_ERR_STATE
        h.set_footprint(tc.FOOTPRINTS["triangle"])
        assert update() == 0
        h.reset()                                                                      # the costmap and the field are gone
        assert update() == cycle() == GV_ERR_STATE
    finally:
        h.close()


def test_mppi_demo(gvamd, tmp_path):
    """examples/mppi_demo.cpp (plain g++ over the C ABI): ticks of the flow with inflate_costmap, the field from a goal
    behind the wall, six gv_mppi_cycle calls of 512 x 40 from one start, and the demo's own host replay of the last
    average"""
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "grid-vision_amd")
    exe = str(tmp_path / "mppi_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(pkg, "examples", "mppi_demo.cpp"), "-o", exe,
                           "-L" + pkg, "-lgridvision_hip", "-Wl,-rpath," + pkg])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    its = re.findall(r"iteration (\d) admitted (\d+) best (-?\d+) total (\d+)\n", out.stdout)
    assert [int(i[0]) for i in its] == list(range(6)) and all(0 < int(i[1]) <= 512 and int(i[2]) >= 0 for i in its), out.stdout
    m = re.search(r"nominal floats that differ from the host average (\d+) of 80\nhost check ok \(0 mismatches\)", out.stdout)
    assert m, out.stdout
