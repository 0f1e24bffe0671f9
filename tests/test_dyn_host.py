"""[EXTENSION] X13 scoring against predicted moving objects, host side (no GPU): the header, the binding and the struct
layouts; gv_dyn_cost_table against inflation_cost_table; the library's host twin (gv_dyn_score_poses: the kernel's
arithmetic text compiled for the host) against dyn_ref on every family of dyn_cases -- exact families byte for byte,
general-yaw families after dyn_cases' guard (numpy and the C library may differ in the last bit of sin and cos); the host
twin of the selection with the third record (gv_control_select_dyn) against dyn_ref.select; the argument errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dyn_cases as dc
import dyn_ref as ref
import nav_ref
import rollout_ref
import traj_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GV_ERR_BAD_ARG = 1

LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "gridvision_hip.h"
int main(void)
{
  printf("%zu %zu %zu %zu ", sizeof(gv_moving_object), offsetof(gv_moving_object, pose), offsetof(gv_moving_object, vx),
         offsetof(gv_moving_object, vy));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu ", sizeof(gv_dyn_config), offsetof(gv_dyn_config, n_circles),
         offsetof(gv_dyn_config, off_x), offsetof(gv_dyn_config, radius), offsetof(gv_dyn_config, influence_radius),
         offsetof(gv_dyn_config, cost_scaling_factor), offsetof(gv_dyn_config, quantum), offsetof(gv_dyn_config, t0),
         offsetof(gv_dyn_config, dt), offsetof(gv_dyn_config, collision_cost), offsetof(gv_dyn_config, w_sum),
         offsetof(gv_dyn_config, w_max), offsetof(gv_dyn_config, flags));
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(gv_dyn_score), offsetof(gv_dyn_score, max_cost), offsetof(gv_dyn_score, first_collision),
         offsetof(gv_dyn_score, cost_sum), offsetof(gv_dyn_score, nearest_object), offsetof(gv_dyn_score, min_dist2));
  return 0;
}
"""

NAMES = ["gv_dyn_cost_table", "gv_set_dyn_config", "gv_set_moving_objects", "gv_score_dynamic_async", "gv_score_dynamic",
         "gv_dyn_score_poses", "gv_control_select_dyn"]


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_header_binding_and_layout(gvamd, tmp_path):
    txt = open(os.path.join(ROOT, "include", "gridvision_hip.h")).read()
    for sig in (r"int gv_dyn_cost_table\(const gv_dyn_config \*cfg, uint8_t \*table, int32_t cap, int32_t \*n\);",
                r"int gv_set_dyn_config\(gv_handle h, const gv_dyn_config \*cfg\);",
                r"int gv_set_moving_objects\(gv_handle h, const gv_moving_object \*objs, int32_t n\);",
                r"int gv_score_dynamic_async\(gv_handle h, const float \*poses, int32_t K, int32_t P, uint32_t flags, "
                r"gv_dyn_score \*scores,\s*uint8_t \*pose_cost\);",
                r"int gv_score_dynamic\(gv_handle h, const float \*poses, int32_t K, int32_t P, uint32_t flags, "
                r"gv_dyn_score \*scores,\s*uint8_t \*pose_cost\);",
                r"int gv_dyn_score_poses\(const gv_dyn_config \*cfg, const gv_moving_object \*objs, int32_t n, const float \*poses, "
                r"int32_t K,\s*int32_t P, gv_dyn_score \*scores, uint8_t \*pose_cost",
                r"int gv_control_select_dyn\(const gv_critic_weights \*w, const gv_traj_score \*traj, const gv_nav_score \*nav,\s*"
                r"const gv_dyn_score \*dyn, const gv_dyn_config \*cfg, int32_t K, gv_control_result \*result,\s*uint64_t \*totals"):
        assert re.search(sig, txt), sig
    for phrase in ("X13.", "THE QUATERNION IS USED AS GIVEN", "ox = x_j + vx_j * t", "a NaN lands on 0.0",
                   "gv_set_dyn_config, gv_set_moving_objects and gv_score_dynamic* may be called"):
        assert phrase in txt, phrase
    lib = gvamd.load()
    for name in NAMES:
        assert name in gvamd.ABI_SYMBOLS and hasattr(lib, name), name
    assert lib.gv_abi_version() == 4        # additive: the version stays
    declared = sorted(set(re.findall(r"\b(gv_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))))
    assert sorted(gvamd.ABI_SYMBOLS) == declared and not [f for f in declared if not hasattr(lib, f)]
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(LAYOUT)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", exe])
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    mo = gvamd.MOVING_OBJECT_DTYPE
    assert mo.itemsize == out[0] == 96 and [mo.fields[n][1] for n in ("pose", "vx", "vy")] == out[1:4]
    assert C.sizeof(gvamd.DynConfig) == out[4]
    assert [getattr(gvamd.DynConfig, n).offset for n, _ in gvamd.DynConfig._fields_] == out[5:17]
    sd = gvamd.DYN_SCORE_DTYPE
    assert sd.itemsize == out[17] == 24 == ref.SCORE_DTYPE.itemsize
    assert [sd.fields[n][1] for n in ("max_cost", "first_collision", "cost_sum", "nearest_object", "min_dist2")] == out[18:23]
    assert sd == ref.SCORE_DTYPE


CONFIGS = [dc.BASE, ref.config(radius=0.0, influence_radius=0.0, quantum=0.05), ref.config(radius=0.3, influence_radius=3.15, quantum=0.05),
           ref.config(radius=0.45, influence_radius=1.0, cost_scaling_factor=0.0, quantum=0.02),
           ref.config(radius=1.0, influence_radius=6.3, cost_scaling_factor=10.0, quantum=0.1)]


@pytest.mark.parametrize("i", range(len(CONFIGS)))
def test_cost_table_is_the_inflation_table(gvamd, i):
    cfg = CONFIGS[i]
    got = gvamd.dyn_cost_table(ref.to_struct(gvamd, cfg))
    want = gvamd.inflation_cost_table(gvamd.Inflation(cfg["radius"], cfg["influence_radius"], cfg["cost_scaling_factor"], 100, 0),
                                      cfg["quantum"])
    assert got.dtype == np.uint8 and got.tobytes() == want.tobytes() and got[0] == 254
    if cfg is dc.BASE:
        assert len(got) == 145 and (got[1:26] == 253).all() and got[26] < 253 and got[144] > 0


def test_families_cover_the_shapes():
    ks, ps, ns, cs = set(), set(), set(), set()
    for c in dc.cases(True) + dc.cases(False):
        K, P = c["poses"].shape[:2]
        assert c["poses"].dtype == np.float32 and c["poses"].shape[2] == 3
        ks.add(K); ps.add(P); ns.add(len(c["objs"])); cs.add(len(c["cfg"]["off_x"]))
        if c["exact"]:
            yaw = c["poses"][:, :, 2]
            assert all(v == 0.0 for v in c["cfg"]["off_x"]) or ((yaw == 0) | ~np.isfinite(yaw)).all(), c["name"]
        else:
            assert c["cfg"]["off_x"] == (-1.0, 0.5, 2.0)
    assert ks == {1, 3, 9, 65} and ps == {1, 3, 63, 64, 65, 257} and ns >= {0, 1, 64, 65, 128} and cs >= {1, 2, 8}


def test_the_families_are_what_they_claim():
    by = {c["name"]: c for c in dc.cases(True)}
    r = dc.want(by["radius_edge_corner"])
    assert (r["scores"]["min_dist2"][:2] <= 0.390625).all() and (r["pose_cost"][:2, :3] == 253).all() and (r["pose_cost"][:, 3:] == 0).all()
    assert (r["obj_min"][:2, 0] < 0.390625).all()            # the pose one ulp inside
    r = dc.want(by["integer_u_table_end"])
    tab = ref.table(by["integer_u_table_end"]["cfg"])
    assert r["pose_cost"][0, :13].tolist() == [int(tab[k * k]) for k in range(13)] and r["pose_cost"][0, 12] == tab[144] > 0
    assert r["pose_cost"][0, 13] == 0 and r["pose_cost"][0, 14] == 0 and r["pose_cost"][0, 15] == tab[144]
    r = dc.want(by["inside"])
    assert r["scores"][0].tolist() == (254, 0, 254, 0, 0.0)
    r = dc.want(by["arrives_at_37"])
    assert r["scores"]["first_collision"][0] == 37 and (r["pose_cost"][0, :37] < 253).all() and r["pose_cost"][0, 37] == 254
    r = dc.want(by["identical_objects"])
    assert (r["scores"]["nearest_object"] == 2).all() and (r["obj_min"][:, 2] == r["obj_min"][:, 5]).all()
    for name in ("no_objects", "no_objects_one_pose"):
        r = dc.want(by[name])
        s = r["scores"]
        assert (s["max_cost"] == 0).all() and (s["first_collision"] == -1).all() and (s["cost_sum"] == 0).all()
        assert (s["nearest_object"] == -1).all() and np.isposinf(s["min_dist2"]).all()
    r = dc.want(by["nonfinite"])
    s = r["scores"]
    # a NaN coordinate, and a NaN or infinite yaw under an off-centre circle, put the pose "inside" every object
    for k in (0, 6, 7, 8):
        assert r["pose_cost"][k, 1] == 254 and s["min_dist2"][k] == 0.0 and s["nearest_object"][k] == 0, k


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "general"])
def test_host_twin_equals_the_reference(gvamd, exact):
    for c in dc.cases(exact):
        r = dc.want(c)
        K = c["poses"].shape[0]
        if not exact:
            assert c["redrawn"] <= 0.01 * K, (c["name"], c["redrawn"])
        cfg = ref.to_struct(gvamd, c["cfg"])
        scores, pc = gvamd.dyn_score_poses(cfg, c["objs"], c["poses"], keep_pose_cost=True)
        dc.compare(c, r, scores, pc, "host twin")
        only = gvamd.dyn_score_poses(cfg, c["objs"], c["poses"])
        assert only.tobytes() == scores.tobytes(), c["name"]


# ------------------------------------------------------------------------------------------------ control select --
def _cw(gvamd, w, flags=0):
    return gvamd.CriticWeights(*[w[n] for n in rollout_ref.WEIGHTS], flags)


def _dyn(rows):
    return np.array(rows, ref.SCORE_DTYPE)    # (max_cost, first_collision, cost_sum, nearest_object, min_dist2)


def _check(gvamd, w, traj, nav, dyn, cfg):
    want_r, want_t = ref.select(w, traj, nav, dyn, cfg)
    got_r, got_t = gvamd.control_select_dyn(_cw(gvamd, w), traj, nav, dyn, ref.to_struct(gvamd, cfg) if cfg else None, keep_totals=True)
    assert np.array([got_r]).tobytes() == want_r.tobytes(), (w, got_r, want_r)
    assert got_t.tobytes() == want_t.tobytes(), w
    return want_r[0], want_t


def test_select_with_the_dyn_record(gvamd):
    W = rollout_ref.weights
    traj = np.array([(10, -1, 100, 0), (5, -1, 50, 0), (254, 0, 1, 0), (7, -1, 60, 2), (5, -1, 40, 0)], traj_ref.SCORE_DTYPE)
    nav = np.array([(40, 4, 2, 3, 0), (400, 90, 80, 0, 0), (1, 1, 1, 0, 0), (30, 3, 1, 2, 0), (0, 0, 0, 0, 1)], nav_ref.SCORE_DTYPE)
    dyn = _dyn([(0, -1, 0, -1, np.inf), (254, 3, 900, 1, 0.0), (0, -1, 0, 0, 9.0), (100, -1, 30, 2, 0.5), (20, -1, 5, 0, 1.0)])
    cfg = ref.config(w_sum=2, w_max=3)
    # without a nav weight: 1 is rejected by the dyn record alone, 2 by the traj record
    r, t = _check(gvamd, W(1, 1), traj, None, dyn, cfg)
    assert t.tolist() == [110, ref.U64, ref.U64, 67 + 60 + 300, 45 + 10 + 60] and (r["best"], r["n_valid"]) == (0, 3)
    # ... with one, 4 is rejected by the nav record as well
    r, t = _check(gvamd, W(1, 1, 1, 0, 0), traj, nav, dyn, cfg)
    assert t.tolist() == [114, ref.U64, ref.U64, 70 + 360, ref.U64]
    # cfg == NULL: gv_control_select itself, dyn is not read
    r0, t0 = _check(gvamd, W(1, 1), traj, None, None, None)
    want_r, want_t = rollout_ref.select(W(1, 1), traj, None)
    assert t0.tobytes() == want_t.tobytes() and t0.tolist() == [110, 55, ref.U64, 67, 45]
    # the best changes only because of w_sum
    r, t = _check(gvamd, W(1, 0), traj[[0, 4]], None, _dyn([(0, -1, 70, 0, 1.0), (0, -1, 5, 0, 1.0)]), ref.config(w_sum=0, w_max=0))
    assert r["best"] == 1                                           # 100 against 40 ...
    r, t = _check(gvamd, W(1, 0), traj[[4, 0]], None, _dyn([(0, -1, 70, 0, 1.0), (0, -1, 5, 0, 1.0)]), ref.config(w_sum=1, w_max=0))
    assert r["best"] == 1 and t.tolist() == [110, 105]              # ... 40 + 70 against 100 + 5
    # the largest records: the bound of the static_assert
    big = 0xFFFFFFFD
    top = W(*[65535] * 5)
    r, t = _check(gvamd, top, np.array([(255, -1, 4096 * 255, 0)], traj_ref.SCORE_DTYPE),
                  np.array([(4096 * big, big, big, 0, 0)], nav_ref.SCORE_DTYPE), _dyn([(255, -1, 4096 * 255, 0, 0.0)]),
                  ref.config(w_sum=65535, w_max=65535, collision_cost=255))
    assert int(t[0]) == 65535 * (2 * (4096 * 255 + 255) + 4098 * big) < (1 << 61)
    _check(gvamd, W(1, 1), traj[:0], None, dyn[:0], cfg)            # K == 0


def test_select_dyn_argument_errors(gvamd):
    lib = gvamd.load()
    W = rollout_ref.weights
    traj = np.array([(10, -1, 100, 0)], traj_ref.SCORE_DTYPE)
    nav = np.array([(40, 4, 2, 3, 0)], nav_ref.SCORE_DTYPE)
    dyn = _dyn([(0, -1, 0, -1, np.inf)])
    res = np.zeros(1, ref.RESULT_DTYPE)

    def raw(w=W(1, 1), t=traj, n=None, d=dyn, cfg=ref.config(), K=1, r=res):
        c = ref.to_struct(gvamd, cfg) if cfg else None
        return lib.gv_control_select_dyn(C.byref(_cw(gvamd, w)) if w else None, _p(t), _p(n), _p(d), C.byref(c) if c else None,
                                         C.c_int32(K), _p(r), None)

    assert raw() == 0 and raw(d=None, cfg=None) == 0 and raw(w=W(1, 1, 1), n=nav) == 0
    assert raw(d=None) == raw(w=None) == raw(t=None) == raw(r=None) == raw(K=-1) == raw(K=(1 << 20) + 1) == GV_ERR_BAD_ARG
    assert raw(w=W(1, 1, 1)) == GV_ERR_BAD_ARG                              # a nav weight without nav records
    assert raw(cfg=ref.config(w_sum=65536)) == raw(cfg=ref.config(w_max=65536)) == GV_ERR_BAD_ARG
    assert raw(cfg=ref.config(w_sum=65535, w_max=65535)) == 0


def _bad_configs():
    nan, inf = float("nan"), float("inf")
    bad = [dict(off_x=()), dict(off_x=(0.0,) * 9), dict(collision_cost=0), dict(collision_cost=256), dict(w_sum=65536), dict(w_max=65536),
           dict(flags=1), dict(dt=-0.1), dict(radius=-0.1), dict(radius=2.0, influence_radius=1.0), dict(cost_scaling_factor=-1.0),
           dict(quantum=0.0), dict(quantum=-0.1), dict(influence_radius=8.01, quantum=0.125)]      # Rc = 64
    for f in ("radius", "influence_radius", "cost_scaling_factor", "quantum", "t0", "dt"):
        bad += [{f: nan}, {f: inf}, {f: -inf}]
    bad += [dict(off_x=(0.0, v)) for v in (nan, inf, -inf)]
    return bad


GOOD_EDGES = [dict(off_x=(0.0,) * 8), dict(collision_cost=1), dict(collision_cost=255), dict(w_sum=65535, w_max=65535), dict(dt=0.0),
              dict(radius=0.0, influence_radius=0.0), dict(influence_radius=7.99, quantum=0.125), dict(t0=-5.0)]


def test_config_and_argument_errors_of_the_host_calls(gvamd):
    lib = gvamd.load()
    table, n = np.zeros(4096, np.uint8), C.c_int32(0)

    def tab(cfg, t=table, cap=4096):
        return lib.gv_dyn_cost_table(C.byref(ref.to_struct(gvamd, cfg)) if cfg else None, _p(t), C.c_int32(cap), C.byref(n))

    assert tab(dc.BASE) == 0 and n.value == 145
    assert tab(None) == tab(dc.BASE, t=None) == tab(dc.BASE, cap=144) == GV_ERR_BAD_ARG and tab(dc.BASE, cap=145) == 0
    for b in _bad_configs():
        assert tab(dict(dc.BASE, **b)) == GV_ERR_BAD_ARG, b
    for g in GOOD_EDGES:
        assert tab(dict(dc.BASE, **g)) == 0, g
    # a non-finite off_x past n_circles is not read
    c = ref.to_struct(gvamd, dc.BASE)
    c.off_x[1] = float("nan")
    assert lib.gv_dyn_cost_table(C.byref(c), _p(table), C.c_int32(4096), C.byref(n)) == 0

    poses = np.zeros((2, 3, 3), np.float32)
    scores = np.zeros(2, ref.SCORE_DTYPE)
    objs = dc.objects([(1.0, 2.0, 0.3, 2.0, 1.0, 0.5, 0.5)] * 2)

    def raw(cfg=dc.BASE, o=objs, n_obj=2, p=poses, K=2, P=3, s=scores):
        return lib.gv_dyn_score_poses(C.byref(ref.to_struct(gvamd, cfg)) if cfg else None, _p(o), C.c_int32(n_obj), _p(p), C.c_int32(K),
                                      C.c_int32(P), _p(s), None)

    assert raw() == 0 and raw(K=0) == 0 and raw(o=None, n_obj=0) == 0
    assert raw(cfg=None) == raw(p=None) == raw(s=None) == raw(o=None) == raw(n_obj=-1) == GV_ERR_BAD_ARG
    assert raw(P=0) == raw(P=4097) == raw(K=-1) == raw(K=(1 << 20) + 1) == raw(cfg=dict(dc.BASE, flags=2)) == GV_ERR_BAD_ARG
    big = dc.objects([(1.0, 2.0, 0.3, 2.0, 1.0, 0.5, 0.5)] * 129)
    assert raw(o=big, n_obj=129) == GV_ERR_BAD_ARG and raw(o=big, n_obj=128) == 0
    for f in ("px", "py", "qx", "qy", "qz", "qw", "length", "width"):
        for v in (float("nan"), float("inf"), -float("inf")):
            o = objs.copy(); o["pose"][f][1] = v
            assert raw(o=o) == GV_ERR_BAD_ARG, (f, v)
    for f in ("vx", "vy"):
        o = objs.copy(); o[f][0] = float("nan")
        assert raw(o=o) == GV_ERR_BAD_ARG, f
    for f in ("length", "width"):
        o = objs.copy(); o["pose"][f][0] = -0.1
        assert raw(o=o) == GV_ERR_BAD_ARG, f
        o["pose"][f][0] = 0.0
        assert raw(o=o) == 0, f
    o = objs.copy(); o["pose"]["pz"][0] = float("nan"); o["pose"]["height"][1] = float("inf")      # ignored fields
    assert raw(o=o) == 0
