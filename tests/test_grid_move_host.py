"""[EXTENSION] X3 ego motion, host side: the planner of gv_grid_move (gv_host_math.hpp, namespace host) against a
plain-Python restatement of include/gridvision_hip.h's rule -- planar yaw of the normalised quaternion, residue
composition E <- E o D, the r_max threshold on the yaw, whole-cell snapping of the translation, E <- S^-1 o E -- over
random motion sequences, and the invariant that the applied resamples and the final residue compose to the input
motion.  A small driver is compiled with plain g++ (no GPU, no ROS), as test_host_side.py builds viz_demo."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grid-vision_amd", "csrc")

DRIVER = r"""
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "gv_host_math.hpp"
using namespace gv;
int main(int argc, char **argv)
{
  if (argc > 1 && std::strcmp(argv[1], "layout") == 0) {
    std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(gv_grid_move_info), offsetof(gv_grid_move_info, applied),
                offsetof(gv_grid_move_info, cos_yaw), offsetof(gv_grid_move_info, sin_yaw), offsetof(gv_grid_move_info, tx),
                offsetof(gv_grid_move_info, ty), offsetof(gv_grid_move_info, res_yaw), offsetof(gv_grid_move_info, res_x),
                offsetof(gv_grid_move_info, res_y));
    return 0;
  }
  if (argc > 4 && std::strcmp(argv[1], "geometry") == 0) {   // host::grid_params of gv_create's arguments
    GridParams p{};
    if (!host::grid_params((uint8_t)std::atoi(argv[2]), (uint8_t)std::atoi(argv[3]), std::atof(argv[4]), p)) return 3;
    std::printf("%d %d %d %a %a %a %a %a %a %a %a\n", p.nx, p.ny, p.G, p.res, p.pos_x, p.pos_y, p.len_x, p.len_y, p.off_x,
                p.off_y, p.inv_res);
    return 0;
  }
  GridParams g{};
  if (std::scanf("%d %d %lf %lf %lf", &g.nx, &g.ny, &g.res, &g.pos_x, &g.pos_y) != 5) return 2;
  g.G = g.nx * g.ny;
  g.len_x = (double)g.nx * g.res;
  g.len_y = (double)g.ny * g.res;
  g.off_x = 0.5 * g.len_x;
  g.off_y = 0.5 * g.len_y;
  g.inv_res = 1.0 / g.res;
  host::Se2 e{0.0, 0.0, 0.0};
  gv_transform m;
  while (std::scanf("%lf %lf %lf %lf %lf %lf %lf", &m.qx, &m.qy, &m.qz, &m.qw, &m.tx, &m.ty, &m.tz) == 7) {
    host::Se2 d;
    if (!host::se2_from_motion(m, d)) { std::printf("bad\n"); continue; }
    const host::GridMoveStep st = host::plan_grid_move(e, d, g);
    e = st.residue;
    std::printf("%d %a %a %a %a %a %a %a %a %a\n", st.applied ? 1 : 0, d.yaw, st.yaw, st.c, st.s, st.tx, st.ty,
                st.residue.yaw, st.residue.x, st.residue.y);
  }
  return 0;
}
"""

# (nx, ny, res, pos_x, pos_y) as gv_create makes them: the reference's 50 x 20 m at 0.1 m, a 200 m square, a coarse one
GRIDS = [(500, 200, 0.1, 16.0, 0.0), (2000, 2000, 0.1, 66.0, 0.0), (200, 200, 0.5, 33.0, 0.0)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("grid_move_host")
    src, exe = str(d / "plan.cpp"), str(d / "plan")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-I" + CSRC, src, "-o", exe])
    return exe


def _run(exe, grid, motions):
    lines = ["%d %d %r %r %r" % grid] + [" ".join(repr(float(v)) for v in m) for m in motions]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60, check=True)
    rows = []
    for ln in out.stdout.splitlines():
        if ln == "bad":
            rows.append(None)
            continue
        f = ln.split()
        rows.append(dict(applied=bool(int(f[0])), **dict(zip(("d_yaw", "yaw", "c", "s", "tx", "ty", "r_yaw", "r_x", "r_y"),
                                                              (float.fromhex(v) for v in f[1:])))))
    assert len(rows) == len(motions)
    return rows


# ------------------------------------------------------------------------------------- the Python restatement --

def _wrap(a):
    if a > math.pi:
        a -= 2.0 * math.pi
    elif a <= -math.pi:
        a += 2.0 * math.pi
    return a


def _compose(a, b):
    c, s = math.cos(a[0]), math.sin(a[0])
    return (_wrap(a[0] + b[0]), a[1] + (c * b[1] - s * b[2]), a[2] + (s * b[1] + c * b[2]))


def _yaw(m):
    qx, qy, qz, qw = m[:4]
    n = math.sqrt(((qx * qx + qy * qy) + qz * qz) + qw * qw)
    qx, qy, qz, qw = qx / n, qy / n, qz / n, qw / n
    return math.atan2(2.0 * (qw * qz + qx * qy), 1.0 - 2.0 * (qy * qy + qz * qz))


def _cround(v):
    """std::round: halves away from zero"""
    t = float(math.trunc(v))
    if abs(v - t) >= 0.5:
        t += math.copysign(1.0, v)
    return t


def _r_max(grid):
    nx, ny, res, px, py = grid
    ox, oy = 0.5 * (nx * res), 0.5 * (ny * res)
    return max(math.sqrt(x * x + y * y) for x in (px - ox, px + ox) for y in (py - oy, py + oy))


def _plan(grid, motions):
    res = grid[2]
    r_max = _r_max(grid)
    e = (0.0, 0.0, 0.0)
    out = []
    for m in motions:
        e = _compose(e, (_yaw(m), m[4], m[5]))
        yaw = e[0] if abs(e[0]) * r_max >= 0.5 * res else 0.0
        tx, ty = res * _cround(e[1] / res), res * _cround(e[2] / res)
        c, s = (1.0, 0.0) if yaw == 0.0 else (math.cos(yaw), math.sin(yaw))
        dx, dy = e[1] - tx, e[2] - ty
        e = (_wrap(e[0] - yaw), c * dx + s * dy, c * dy - s * dx)
        out.append(dict(applied=yaw != 0.0 or tx != 0.0 or ty != 0.0, yaw=yaw, c=c, s=s, tx=tx, ty=ty,
                        r_yaw=e[0], r_x=e[1], r_y=e[2]))
    return out


def _quat(roll, pitch, yaw):
    """tf2 setRPY"""
    cy, sy = math.cos(yaw * 0.5), math.sin(yaw * 0.5)
    cp, sp = math.cos(pitch * 0.5), math.sin(pitch * 0.5)
    cr, sr = math.cos(roll * 0.5), math.sin(roll * 0.5)
    return (sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy)


def _motions(seed, n):
    """a vehicle-like sequence: mostly small steps (a few cm to a metre, up to ~1 deg), some sub-cell creeps, some
    large jumps and turns, a little roll / pitch / z noise and a non-unit quaternion scale"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        kind = rng.integers(0, 10)
        if kind < 6:
            yaw, t = rng.normal(0.0, 0.01), rng.normal(0.0, 0.4, 2)
        elif kind < 8:
            yaw, t = rng.normal(0.0, 1e-4), rng.uniform(-0.04, 0.04, 2)
        else:
            yaw, t = rng.uniform(-math.pi, math.pi), rng.uniform(-30.0, 30.0, 2)
        q = np.array(_quat(rng.normal(0.0, 0.01), rng.normal(0.0, 0.01), yaw)) * rng.uniform(0.5, 2.0)
        out.append((*q, t[0], t[1], rng.normal(0.0, 0.1)))
    return out


def _close(a, b, tol=1e-12):
    return abs(a - b) <= tol * max(1.0, abs(a), abs(b))


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_planner_matches_restatement(driver, grid, seed):
    motions = _motions(seed, 300)
    got, want = _run(driver, grid, motions), _plan(grid, motions)
    n_applied = n_rot = 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert _close(g["d_yaw"], _yaw(motions[i])), i
        assert g["applied"] == w["applied"], i
        for k in ("yaw", "c", "s", "r_yaw", "r_x", "r_y"):
            assert _close(g[k], w[k]), (i, k, g[k], w[k])
        for k in ("tx", "ty"):   # whole cells, the same number of them
            assert g[k] == w[k], (i, k, g[k], w[k])
            assert _cround(g[k] / grid[2]) * grid[2] == g[k]
        assert abs(g["r_x"]) <= 0.5 * grid[2] * (1 + 1e-9) + 1e-12 or g["yaw"] != 0.0
        n_applied += g["applied"]
        n_rot += g["yaw"] != 0.0
    assert 0 < n_rot < n_applied < len(motions)   # every branch ran


def test_sub_cell_steps_accumulate(driver):
    """3 cm per tick at 0.1 m cells: nothing for the first calls, then one-cell moves; the residue is what is left"""
    grid = GRIDS[0]
    rows = _run(driver, grid, [(0.0, 0.0, 0.0, 1.0, 0.03, 0.0, 0.0)] * 30)
    applied = [r["applied"] for r in rows]
    assert applied[:1] == [False] and any(applied)
    assert sum(r["tx"] for r in rows) + rows[-1]["r_x"] == pytest.approx(0.9, abs=1e-12)
    assert all(r["yaw"] == 0.0 and r["c"] == 1.0 and r["s"] == 0.0 for r in rows)
    assert all(abs(r["r_x"]) <= 0.05 + 1e-12 for r in rows)


def test_yaw_threshold_is_half_a_cell_at_the_far_corner(driver):
    for grid in GRIDS:
        th = 0.5 * grid[2] / _r_max(grid)
        below = (0.0, 0.0, math.sin(0.45 * th), math.cos(0.45 * th), 0.0, 0.0, 0.0)   # 0.9 th per call
        rows = _run(driver, grid, [below, below])
        assert not rows[0]["applied"] and rows[0]["r_yaw"] == pytest.approx(0.9 * th, rel=1e-9)
        assert rows[1]["applied"] and rows[1]["yaw"] == pytest.approx(1.8 * th, rel=1e-9) and rows[1]["r_yaw"] == 0.0


def test_applied_moves_and_residue_compose_to_the_motion(driver):
    """S_1 o S_2 o ... o S_n o E_n == D_1 o ... o D_n (what the layers moved by plus what is still owed)"""
    for grid in GRIDS:
        for seed in (4, 5):
            motions = _motions(seed, 200)
            rows = _run(driver, grid, motions)
            total, moved = (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)
            for m, r in zip(motions, rows):
                total = _compose(total, (r["d_yaw"], m[4], m[5]))
                moved = _compose(moved, (r["yaw"], r["tx"], r["ty"]))
            back = _compose(moved, (rows[-1]["r_yaw"], rows[-1]["r_x"], rows[-1]["r_y"]))
            assert abs(_wrap(back[0] - total[0])) <= 1e-12
            assert abs(back[1] - total[1]) <= 1e-12 * max(1.0, abs(total[1]))
            assert abs(back[2] - total[2]) <= 1e-12 * max(1.0, abs(total[2]))


def test_non_finite_motion_is_rejected(driver):
    bad = [(0.0, 0.0, 0.0, 1.0, float("nan"), 0.0, 0.0), (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, float("inf")),
           (0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0), (float("-inf"), 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)]
    ok = (0.0, 0.0, 0.0, 1.0, 0.23, 0.0, 0.0)
    rows = _run(driver, GRIDS[0], [bad[0], ok, bad[1], bad[2], bad[3]])
    assert rows[0] is None and rows[2] is None and rows[3] is None and rows[4] is None
    assert rows[1]["applied"] and rows[1]["tx"] == pytest.approx(0.2) and rows[1]["r_x"] == pytest.approx(0.03)


def test_header_declares_grid_move_and_the_binding_matches_its_layout(driver):
    txt = open(os.path.join(ROOT, "include", "gridvision_hip.h")).read()
    assert re.search(r"int gv_grid_move\(gv_handle h, const gv_transform \*motion, gv_grid_move_info \*info\);", txt)
    import gvamd
    assert "gv_grid_move" in gvamd.ABI_SYMBOLS
    out = subprocess.run([driver, "layout"], capture_output=True, text=True, check=True).stdout.split()
    size, offs = int(out[0]), [int(v) for v in out[1:]]
    assert C.sizeof(gvamd.GridMoveInfo) == size
    assert [getattr(gvamd.GridMoveInfo, n).offset for n, _ in gvamd.GridMoveInfo._fields_] == offs
