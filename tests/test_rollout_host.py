"""[EXTENSION] X10 rollout and control step, host side (no GPU): the header, the binding and the struct layouts; the
library's host twin of the rollout (gv_rollout_poses: the kernel's arithmetic text compiled for the host) against
rollout_ref on every fixture family, byte for byte -- the host's C library computes sin and cos on both sides, NaN entries
are compared by position; the host twin of the selection (gv_control_select) against rollout_ref's loop on crafted
records; the argument errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nav_ref
import rollout_cases as rc
import rollout_ref as ref
import traj_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GV_ERR_BAD_ARG = 1
U64 = ref.U64

LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "gridvision_hip.h"
int main(void)
{
  printf("%zu %zu %zu %zu ", sizeof(gv_motion_model), offsetof(gv_motion_model, model), offsetof(gv_motion_model, dt),
         offsetof(gv_motion_model, flags));
  printf("%zu %zu %zu %zu %zu %zu %zu ", sizeof(gv_critic_weights), offsetof(gv_critic_weights, w_cost_sum),
         offsetof(gv_critic_weights, w_max_cost), offsetof(gv_critic_weights, w_nav_last), offsetof(gv_critic_weights, w_nav_sum),
         offsetof(gv_critic_weights, w_nav_best), offsetof(gv_critic_weights, flags));
  printf("%zu %zu %zu %zu ", sizeof(gv_control_result), offsetof(gv_control_result, best), offsetof(gv_control_result, n_valid),
         offsetof(gv_control_result, best_total));
  printf("%d %d %d %d %d\n", (int)GV_MOTION_DIFF, (int)GV_MOTION_OMNI, (int)GV_ROLLOUT_DEVICE_CONTROLS, (int)GV_ROLLOUT_CONSTANT,
         (int)GV_CONTROL_KEEP_TOTALS);
  return 0;
}
"""

NAMES = ["gv_set_motion_model", "gv_rollout_async", "gv_rollout", "gv_device_rollout", "gv_get_rollout", "gv_rollout_poses",
         "gv_control_step_async", "gv_control_step", "gv_control_select"]


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


def _cw(gvamd, w, flags=0):
    return gvamd.CriticWeights(*[w[n] for n in ref.WEIGHTS], flags)


def test_header_binding_and_layout(gvamd, tmp_path):
    txt = open(os.path.join(ROOT, "include", "gridvision_hip.h")).read()
    for sig in (r"int gv_set_motion_model\(gv_handle h, const gv_motion_model \*m\);",
                r"int gv_rollout_async\(gv_handle h, const double start\[3\], const float \*controls, int32_t K, int32_t P, uint32_t flags\);",
                r"int gv_rollout\(gv_handle h, const double start\[3\], const float \*controls, int32_t K, int32_t P, uint32_t flags\);",
                r"int gv_device_rollout\(gv_handle h, float \*\*poses, int32_t \*K, int32_t \*P\);",
                r"int gv_get_rollout\(gv_handle h, float \*poses_out\);",
                r"int gv_rollout_poses\(const gv_motion_model \*m, const double start\[3\], const float \*controls, int32_t K, "
                r"int32_t P,\s*uint32_t flags, float \*poses_out\);",
                r"int gv_control_step_async\(gv_handle h, const gv_critic_weights \*w, uint32_t flags, gv_control_result \*result,\s*"
                r"uint64_t \*totals\);",
                r"int gv_control_step\(gv_handle h, const gv_critic_weights \*w, uint32_t flags, gv_control_result \*result, "
                r"uint64_t \*totals\);",
                r"int gv_control_select\(const gv_critic_weights \*w, const gv_traj_score \*traj, const gv_nav_score \*nav, "
                r"int32_t K,\s*gv_control_result \*result, uint64_t \*totals"):
        assert re.search(sig, txt), sig
    for phrase in ("the yaw BEFORE the step", "T = T + w * dt", "IT MAY CHANGE WHEN THE BUFFER", "< 2^61",
                   "gv_set_motion_model, gv_rollout*"):
        assert phrase in txt, phrase
    lib = gvamd.load()
    for name in NAMES:
        assert name in gvamd.ABI_SYMBOLS and hasattr(lib, name), name
    assert lib.gv_abi_version() == 4
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(LAYOUT)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", exe])
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert C.sizeof(gvamd.MotionModel) == out[0]
    assert [getattr(gvamd.MotionModel, n).offset for n, _ in gvamd.MotionModel._fields_] == out[1:4]
    assert C.sizeof(gvamd.CriticWeights) == out[4]
    assert [getattr(gvamd.CriticWeights, n).offset for n, _ in gvamd.CriticWeights._fields_] == out[5:11]
    assert gvamd.CONTROL_RESULT_DTYPE.itemsize == out[11] == 16 == ref.RESULT_DTYPE.itemsize
    assert [gvamd.CONTROL_RESULT_DTYPE.fields[n][1] for n in ("best", "n_valid", "best_total")] == out[12:15]
    assert [gvamd.MOTION_DIFF, gvamd.MOTION_OMNI, gvamd.ROLLOUT_DEVICE_CONTROLS, gvamd.ROLLOUT_CONSTANT,
            gvamd.CONTROL_KEEP_TOTALS] == out[15:20] == [ref.DIFF, ref.OMNI, ref.DEVICE_CONTROLS, ref.CONSTANT, ref.KEEP_TOTALS]


def test_families_cover_the_shapes():
    ks, ps = set(), set()
    for kind in rc.KINDS:
        for model in rc.MODELS:
            for constant in (False, True):
                for c in rc.family(kind, model, constant):
                    u = c["controls"]
                    assert u.dtype == np.float32 and u.shape[-1] == ref.n_controls(model) and u.ndim == (2 if constant else 3)
                    if kind != "nonfinite":
                        ks.add(len(u)); ps.add(c["P"])
    assert ks == {1, 3, 64, 65, 257} and ps == {1, 2, 63, 64, 65, 130}


@pytest.mark.parametrize("constant", [False, True], ids=["steps", "const"])
@pytest.mark.parametrize("model", rc.MODELS, ids=["diff", "omni"])
@pytest.mark.parametrize("kind", rc.KINDS)
def test_rollout_poses_equal_the_reference(gvamd, kind, model, constant):
    for c in rc.family(kind, model, constant):
        want = rc.want(c)
        got = gvamd.rollout_poses(gvamd.MotionModel(c["model"], c["dt"], 0), c["start"], c["controls"], c["constant"], c["P"])
        assert got.dtype == np.float32 and got.shape == want.shape, c["name"]
        if kind in rc.EXACT:
            assert got.tobytes() == want.tobytes(), c["name"]
        else:
            assert rc.same_but_nan_payload(got, want), c["name"]


def test_the_families_are_what_they_claim():
    for model in rc.MODELS:
        for constant in (False, True):
            for c in rc.family("zeros", model, constant):
                w = rc.want(c)
                assert (w == np.array(c["start"], np.float32)).all(), c["name"]
            for c in rc.family("straight", model, constant):
                w = rc.want(c)
                assert (w[:, :, 2] == 0).all() and (w[:, -1, 0] != np.float32(c["start"][0])).any(), c["name"]
            for c in rc.family("spin", model, constant):
                assert (rc.want(c)[:, :, 2] > 1e5).all(), c["name"]
            g = traj_ref.grid(50, 20, 0.1)
            for c in rc.family("leaving", model, constant):
                w = rc.want(c)
                if c["P"] >= 63:   # every trajectory has a pose off the map
                    assert all(any(traj_ref.get_index(g, *q[:2]) is None for q in t) for t in w), c["name"]
                assert traj_ref.get_index(g, *w[0, 0, :2]) is not None, c["name"]
            for c in rc.family("nonfinite", model, constant):
                w = rc.want(c)
                assert (~np.isfinite(w[:, -1])).any(axis=1).all(), c["name"]   # every trajectory ends non-finite somewhere
                if not constant:
                    assert np.isfinite(w[2::3, :63]).all() and np.isfinite(w[1::3, :31]).all(), c["name"]


# ------------------------------------------------------------------------------------------------ control select --
def _traj(rows):
    return np.array(rows, traj_ref.SCORE_DTYPE)   # (max_cost, first_collision, cost_sum, n_off_map)


def _nav(rows):
    return np.array(rows, nav_ref.SCORE_DTYPE)    # (sum, last, best, best_pose, n_bad)


def _check(gvamd, w, traj, nav):
    want_r, want_t = ref.select(w, traj, nav)
    got_r, got_t = gvamd.control_select(_cw(gvamd, w), traj, nav, keep_totals=True)
    assert np.array([got_r]).tobytes() == want_r.tobytes(), (w, got_r, want_r)
    assert got_t.dtype == np.uint64 and got_t.tobytes() == want_t.tobytes(), w
    only = gvamd.control_select(_cw(gvamd, w), traj, nav)
    assert np.array([only]).tobytes() == want_r.tobytes()
    return want_r[0], want_t


ALL_ON = ref.weights(3, 7, 11, 13, 17)
WEIGHT_SETS = [ref.weights(1, 0), ref.weights(0, 1), ref.weights(5, 9), ref.weights(w_nav_last=2), ref.weights(w_nav_sum=3),
               ref.weights(w_nav_best=4), ALL_ON]


def test_select_rejection_rules(gvamd):
    traj = _traj([(10, -1, 100, 0), (5, -1, 50, 0), (254, 0, 1, 0), (7, -1, 60, 2), (5, 3, 0, 0)])
    nav = _nav([(40, 4, 2, 3, 0), (400, 90, 80, 0, 1), (1, 1, 1, 0, 0), (30, 3, 1, 2, 0), (0, 0, 0, 0, 0)])
    # without a nav weight only first_collision rejects: 0, 1 and 3 are admitted, n_bad and n_off_map do not count
    r, t = _check(gvamd, ref.weights(1, 1), traj, nav)
    assert (r["best"], r["n_valid"], r["best_total"]) == (1, 3, 55) and t.tolist() == [110, 55, U64, 67, U64]
    r, t = _check(gvamd, ref.weights(1, 1), traj, None)
    assert r["best"] == 1
    # with one: n_bad > 0 rejects 1 as well
    r, t = _check(gvamd, ref.weights(1, 1, 1, 0, 0), traj, nav)
    assert (r["best"], r["n_valid"]) == (3, 2) and t.tolist() == [114, U64, U64, 70, U64]
    for w in WEIGHT_SETS:
        _check(gvamd, w, traj, nav)


def test_select_ties_take_the_smallest_index(gvamd):
    K = 2049
    rng = np.random.default_rng(5)
    for w in (ref.weights(1, 1), ALL_ON):
        for places in ([0], [63], [64], [1023], [1024], [1025], [63, 64], [1023, 1024, 1025], [2048, 1025], [0, 2048]):
            traj = np.zeros(K, traj_ref.SCORE_DTYPE)
            traj["max_cost"] = rng.integers(10, 200, K); traj["first_collision"] = -1; traj["cost_sum"] = rng.integers(500, 9000, K)
            nav = np.zeros(K, nav_ref.SCORE_DTYPE)
            nav["sum"] = rng.integers(1000, 50000, K); nav["last"] = rng.integers(100, 900, K); nav["best"] = rng.integers(100, 900, K)
            for k in places:
                traj[k] = (1, -1, 2, 0)
                nav[k] = (3, 1, 1, 0, 0)
            r, _ = _check(gvamd, w, traj, nav)
            assert r["best"] == min(places) and r["n_valid"] == K, (w, places)


def test_select_all_rejected_one_and_none(gvamd):
    traj = _traj([(254, 0, 9, 0), (254, 5, 9, 0), (255, 1, 9, 1)])
    r, t = _check(gvamd, ref.weights(1, 1), traj, None)
    assert (r["best"], r["n_valid"], r["best_total"]) == (-1, 0, U64) and t.tolist() == [U64] * 3
    r, t = _check(gvamd, ALL_ON, _traj([(4, -1, 9, 0)]), _nav([(20, 5, 3, 1, 0)]))
    assert (r["best"], r["n_valid"], r["best_total"]) == (0, 1, 3 * 9 + 7 * 4 + 11 * 5 + 13 * 20 + 17 * 3)
    r, t = _check(gvamd, ALL_ON, _traj([(4, -1, 9, 0)]), _nav([(20, 5, 3, 1, 1)]))
    assert r["best"] == -1
    r, t = _check(gvamd, ALL_ON, _traj([]), _nav([]))          # K == 0
    assert (r["best"], r["n_valid"], r["best_total"]) == (-1, 0, U64) and len(t) == 0


def test_select_largest_records_stay_below_2_61(gvamd):
    big = 0xFFFFFFFD
    traj = _traj([(255, -1, 4096 * 255, 0), (255, -1, 4096 * 255, 0), (0, -1, 0, 0)])
    nav = _nav([(4096 * big, big, big, 0, 0), (4096 * big, big, big - 1, 0, 0), (0, 0, 0, 0, 0)])
    top = ref.weights(*[65535] * 5)
    r, t = _check(gvamd, top, traj, nav)
    assert int(t[0]) == 65535 * (4096 * 255 + 255 + 4098 * big) < (1 << 61) and int(t[0]) > (1 << 60)
    assert r["best"] == 2 and int(t[1]) == int(t[0]) - 65535
    r, t = _check(gvamd, top, traj[:2], nav[:2])
    assert r["best"] == 1 and r["best_total"] == t[1]
    r, t = _check(gvamd, ref.weights(), traj, nav)                       # every weight 0: every total 0, the first wins
    assert (r["best"], r["n_valid"], r["best_total"]) == (0, 3, 0)
    _check(gvamd, ref.weights(65535, 0, 0, 65535, 0), traj, nav)


def test_select_argument_errors(gvamd):
    lib = gvamd.load()
    traj = _traj([(10, -1, 100, 0), (5, -1, 50, 0)])
    nav = _nav([(40, 4, 2, 3, 0), (400, 90, 80, 0, 0)])
    res = np.zeros(1, ref.RESULT_DTYPE)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None

    def raw(w, t=traj, n=nav, K=2, r=res, flags=0):
        return lib.gv_control_select(C.byref(_cw(gvamd, w, flags)) if w is not None else None, p(t), p(n), C.c_int32(K), p(r), None)

    assert raw(ALL_ON) == 0
    assert raw(ref.weights(1, 1), n=None) == 0                           # nav == NULL without a nav weight
    for w in (ref.weights(w_nav_last=1), ref.weights(w_nav_sum=1), ref.weights(w_nav_best=1)):
        assert raw(w, n=None) == GV_ERR_BAD_ARG                         # ... and with one
    assert raw(None) == raw(ALL_ON, t=None) == raw(ALL_ON, r=None) == GV_ERR_BAD_ARG
    assert raw(ALL_ON, K=-1) == raw(ALL_ON, K=(1 << 20) + 1) == raw(ALL_ON, flags=1) == GV_ERR_BAD_ARG
    for name in ref.WEIGHTS:
        w = dict(ALL_ON); w[name] = 65536
        assert raw(w) == GV_ERR_BAD_ARG, name
        w[name] = 65535
        assert raw(w) == 0, name


def test_rollout_poses_argument_errors(gvamd):
    lib = gvamd.load()
    u = np.zeros((2, 3, 2), np.float32)
    out = np.zeros((2, 3, 3), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None

    def raw(model=ref.DIFF, dt=0.05, mflags=0, start=(0.0, 0.0, 0.0), controls=u, K=2, P=3, flags=0, dst=out, m=True):
        mm = gvamd.MotionModel(model, dt, mflags)
        s = (C.c_double * 3)(*start) if start is not None else None
        return lib.gv_rollout_poses(C.byref(mm) if m else None, s, p(controls), C.c_int32(K), C.c_int32(P), C.c_uint32(flags), p(dst))

    assert raw() == 0 and raw(K=0) == 0 and raw(flags=ref.CONSTANT) == 0
    assert raw(m=False) == raw(start=None) == raw(controls=None) == raw(dst=None) == GV_ERR_BAD_ARG
    assert raw(model=2) == raw(model=-1) == raw(dt=0.0) == raw(dt=-1.0) == raw(dt=float("inf")) == raw(dt=float("nan")) == GV_ERR_BAD_ARG
    assert raw(mflags=1) == raw(flags=ref.DEVICE_CONTROLS) == raw(flags=4) == GV_ERR_BAD_ARG
    for i in range(3):
        for v in (float("nan"), float("inf"), -float("inf")):
            s = [0.0, 0.0, 0.0]; s[i] = v
            assert raw(start=s) == GV_ERR_BAD_ARG
    assert raw(P=0) == raw(P=4097) == raw(K=-1) == raw(K=(1 << 20) + 1) == GV_ERR_BAD_ARG
    assert raw(K=(1 << 12) + 1, P=4096, controls=u, dst=out, flags=ref.CONSTANT) == GV_ERR_BAD_ARG   # K * P > 2^24
