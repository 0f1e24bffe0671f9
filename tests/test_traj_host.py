"""[EXTENSION] X7 trajectory scoring, host side (no GPU): the header, the binding and the struct layouts; traj_ref's line
against the oracle's march and its getIndex against the oracle's on every edge and vertex of every fixture; the library's
own geometry (gv_footprint_cells, the host twin of the kernel's closed form) against traj_ref cell for cell on every
fixture pose; the guard that makes the fixtures independent of the libm; the error cases; and the fixtures of
traj_cases.py reaching the edges they are named for."""
import ctypes as C
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib as ol
import traj_cases as tc
import traj_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GV_ERR_BAD_ARG = 1

LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "gridvision_hip.h"
int main(void)
{
  printf("%zu %zu %zu %zu %zu %zu %zu ", sizeof(gv_footprint), offsetof(gv_footprint, n_vertices), offsetof(gv_footprint, vx),
         offsetof(gv_footprint, vy), offsetof(gv_footprint, collision_cost), offsetof(gv_footprint, off_map_cost),
         offsetof(gv_footprint, flags));
  printf("%zu %zu %zu %zu %zu %d %d\n", sizeof(gv_traj_score), offsetof(gv_traj_score, max_cost),
         offsetof(gv_traj_score, first_collision), offsetof(gv_traj_score, cost_sum), offsetof(gv_traj_score, n_off_map),
         (int)GV_TRAJ_KEEP_POSE_COST, (int)GV_TRAJ_DEVICE_POSES);
  return 0;
}
"""

NAMES = ["gv_set_footprint", "gv_score_trajectories_async", "gv_score_trajectories", "gv_footprint_cells"]


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


@pytest.fixture(scope="module")
def fixture_poses():
    """[(family, grid name, Grid, Fp, (x, y, yaw))] of every fixture pose"""
    out = []
    for name, f in tc.families().items():
        g, fp = tc.grid_of(f["grid"]), tc.fp_of(f["fp"])
        out += [(name, f["grid"], g, fp, tuple(p)) for p in f["poses"].reshape(-1, 3)]
    return out


def _cfp(gvamd, fp):
    return gvamd.Footprint.of(fp.vertices, fp.collision_cost, fp.off_map_cost)


def test_header_binding_and_layout(gvamd, tmp_path):
    txt = open(os.path.join(ROOT, "include", "gridvision_hip.h")).read()
    for sig in (r"int gv_set_footprint\(gv_handle h, const gv_footprint \*fp\);",
                r"int gv_score_trajectories_async\(gv_handle h, const float \*poses, int32_t K, int32_t P, uint32_t flags,\s*"
                r"gv_traj_score \*scores, uint8_t \*pose_cost\);",
                r"int gv_score_trajectories\(gv_handle h, const float \*poses, int32_t K, int32_t P, uint32_t flags,\s*"
                r"gv_traj_score \*scores, uint8_t \*pose_cost\);",
                r"int gv_footprint_cells\(uint8_t grid_x, uint8_t grid_y, double resolution, const gv_footprint \*fp, float x, "
                r"float y,\s*float yaw, int32_t \*cells, int32_t cap, int32_t \*n\);"):
        assert re.search(sig, txt), sig
    assert "DIRECTION OF AN EDGE MATTERS" in txt
    lib = gvamd.load()
    for name in NAMES:
        assert name in gvamd.ABI_SYMBOLS and hasattr(lib, name), name
    assert lib.gv_abi_version() == 4
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(LAYOUT)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", exe])
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert C.sizeof(gvamd.Footprint) == out[0]
    assert [getattr(gvamd.Footprint, n).offset for n, _ in gvamd.Footprint._fields_] == out[1:7]
    assert gvamd.TRAJ_SCORE_DTYPE.itemsize == out[7] == 16 == ref.SCORE_DTYPE.itemsize
    assert [gvamd.TRAJ_SCORE_DTYPE.fields[n][1] for n in gvamd.TRAJ_SCORE_DTYPE.names] == out[8:12]
    assert gvamd.TRAJ_SCORE_DTYPE == ref.SCORE_DTYPE
    assert (gvamd.TRAJ_KEEP_POSE_COST, gvamd.TRAJ_DEVICE_POSES) == (out[12], out[13]) == (ref.KEEP_POSE_COST, ref.DEVICE_POSES)


def test_reference_line_equals_the_oracle_march(fixture_poses):
    """every edge of every fixture: the cells of ref.line are the cells gvo_march_ends marks from the start cell's
    centre to the end cell, end included (kind 2)"""
    grids, seen = {}, set()
    for _, gname, g, fp, pose in fixture_poses:
        edges = ref.pose_edges(g, fp, *pose)
        for e in edges or []:
            if (gname, e) in seen:
                continue
            seen.add((gname, e))
            if gname not in grids:
                grids[gname] = ol.OGrid(*tc.GRIDS[gname][0])
            og = grids[gname]
            sx, sy, ex, ey = e
            m = np.zeros(16, np.float32)
            m[3] = (g.pos_x + g.off_x) - (sx + 0.5) * g.res     # the start cell's centre
            m[7] = (g.pos_y + g.off_y) - (sy + 0.5) * g.res
            assert og.get_index(float(m[3]), float(m[7])) == (True, sx, sy)
            miss = og.march_ends(m, [ex], [ey], [2])
            want = ref.line(sx, sy, ex, ey)
            assert len(set(want)) == len(want) == max(abs(ex - sx), abs(ey - sy)) + 1
            assert want[0] == (sx, sy) and want[-1] == (ex, ey)
            assert sorted(np.flatnonzero(miss).tolist()) == sorted(cy * g.nx + cx for cx, cy in want), e
    assert len(seen) > 3000


def test_reference_get_index_equals_the_oracle(fixture_poses):
    grids, n = {}, 0
    for _, gname, g, fp, (x, y, yaw) in fixture_poses:
        if gname not in grids:
            grids[gname] = ol.OGrid(*tc.GRIDS[gname][0])
        pts = [(float(np.float64(x)), float(np.float64(y)))] + ref.world_vertices(fp, x, y, yaw)
        for wx, wy in pts:
            ok, ix, iy = grids[gname].get_index(wx, wy)
            want = ref.get_index(g, wx, wy)
            assert (want is None and not ok) or want == (ix, iy), (wx, wy, want, ok, ix, iy)
            n += 1
    assert n > 10000
    g = tc.grid_of("500x200")
    assert ref.get_index(g, 40.7, 0.0) == (2, 100)     # the canary: in decimal arithmetic (41 - 40.7) / 0.1 is cell 3
    assert (Fraction(41) - Fraction("40.7")) / Fraction("0.1") == 3


def test_library_footprint_cells_equal_the_reference(gvamd, fixture_poses):
    """fails without the feature: gvamd.footprint_cells is the library's own geometry code"""
    n_on = n_off = 0
    for name, gname, g, fp, (x, y, yaw) in fixture_poses:
        gx, gy, res = tc.GRIDS[gname][0]
        got = gvamd.footprint_cells(gx, gy, res, _cfp(gvamd, fp), x, y, yaw)
        want = ref.pose_cells(g, fp, x, y, yaw)
        if want is None:
            assert got is None, (name, x, y, yaw)
            n_off += 1
        else:
            assert got is not None and got.dtype == np.int32 and got.tolist() == want, (name, x, y, yaw)
            n_on += 1
    assert n_on > 4000 and n_off > 60


@pytest.mark.parametrize("gx,gy,res,verts,pose", [
    # a 510000 x 2000 strip: edges of 480000 cells, den / 2 + i * add up to 7.7e8
    (255, 1, 0.0005, ((120.0, 0.4), (-120.0, -0.4), (-120.0, 0.4)), (85.0, 0.0, 0.0)),
    # a 32600 x 32600 map: nearly diagonal edges, quotients up to 29000
    (163, 163, 0.005, ((75.0, 70.0), (-75.0, -72.5), (-70.0, 74.0)), (54.0, 0.0, 0.0)),
])
def test_closed_form_on_the_longest_lines_a_map_holds(gvamd, gx, gy, res, verts, pose):
    """yaw 0 (exact on any libm): the library's closed form, with its reciprocal-product division, against the loop at
    the largest operands gv_create's size limit (2^30 cells) admits"""
    g, fp = ref.grid(gx, gy, res), ref.Fp(verts)
    assert g.nx * g.ny <= 1 << 30
    want = ref.pose_cells(g, fp, *pose)
    assert want is not None and len(want) > 80000
    got = gvamd.footprint_cells(gx, gy, res, _cfp(gvamd, fp), *pose)
    assert got is not None and np.array_equal(got, np.array(want, np.int64))


def test_guard_holds_on_every_fixture():
    fams = tc.families()
    total = 0
    for name, f in fams.items():
        g, fp = tc.grid_of(f["grid"]), tc.fp_of(f["fp"])
        assert tc.guard_violations(g, fp, f["poses"]) == [], name
        total += f["poses"].shape[0] * f["poses"].shape[1]
    print("fixture poses %d, trajectories drawn again for the guard: %s" % (total, tc.REDRAWN))
    assert sum(tc.REDRAWN.values()) <= 3   # a violation has probability ~1e-8 per vertex: redraws are rare, not routine
    # the guard does reject what it must: a vertex 1e-10 m from a cell border
    g = tc.grid_of("500x200")
    target = (g.pos_x + g.off_x - 300 * g.res) - 1e-10
    near = ref.Fp((((target - 5.0) / math.cos(float(np.float32(0.3))), 0.0), (-0.3, 0.35), (-0.3, -0.35)))
    assert abs(ref.world_vertices(near, 5.0, 1.0, 0.3)[0][0] - target) < 1e-12
    assert tc.guard_violations(g, near, np.array([(5.0, 1.0, 0.3)], np.float32)) == [(0, 0)]


def test_sizes_cover_the_issue():
    fams = tc.families()
    assert {f["poses"].shape[0] for f in fams.values()} >= {1, 3, 64, 65, 257}
    assert {f["poses"].shape[1] for f in fams.values()} >= {1, 2, 63, 64, 65, 130}
    assert {f["fp"] for f in fams.values()} >= {"point", "triangle", "rect", "poly16", "tiny", "long"}
    assert len(tc.FOOTPRINTS["poly16"]) == 16
    r = tc.FOOTPRINTS["rect"]
    assert (r[0][0] - r[1][0], r[0][1] - r[3][1]) == (4.5, 2.0) and r[0][0] != -r[1][0]


def test_fixture_families_reach_their_edges(fixture_poses):
    longest = {"x": 0, "y": 0}
    signs, diag, one_cell, folded, tiny_multi = set(), 0, 0, 0, 0
    for name, gname, g, fp, pose in fixture_poses:
        edges = ref.pose_edges(g, fp, *pose)
        if not edges:
            continue
        if len({e[:2] for e in edges}) == 1:
            folded += 1                                  # every vertex in one cell
            assert ref.pose_cells(g, fp, *pose)[1:] == [edges[0][1] * g.nx + edges[0][0]] * len(edges)
        elif name == "tiny_1x64":
            tiny_multi += 1
        for sx, sy, ex, ey in edges:
            ddx, ddy = abs(ex - sx), abs(ey - sy)
            axis = "x" if ddx >= ddy else "y"
            longest[axis] = max(longest[axis], max(ddx, ddy) + 1)
            if ddx and ddy:
                signs.add((ex > sx, ey > sy))
            diag += ddx == ddy and ddx > 0
            one_cell += ddx == 0 and ddy == 0
    assert longest["x"] > 128 and longest["y"] > 128, longest      # the long footprint, shallow and steep
    assert signs == {(True, True), (True, False), (False, True), (False, False)}
    assert diag >= 8 and one_cell >= 10 and folded >= 5 and tiny_multi >= 5
    # an edge longer than 64 cells and no longer than 128: the rectangle's long side on the 0.05 m map
    fine = [max(abs(e[2] - e[0]), abs(e[3] - e[1])) + 1 for n, gn, g, fp, p in fixture_poses if n == "rect_3x65_fine"
            for e in (ref.pose_edges(g, fp, *p) or [])]
    assert any(64 < m <= 128 for m in fine)
    # the direction of an edge matters: some fixture edge's cells differ from those of the reversed edge
    assert any(sorted(ref.line(*e)) != sorted(ref.line(e[2], e[3], e[0], e[1]))
               for n, gn, g, fp, p in fixture_poses if n == "rect_3x130" for e in (ref.pose_edges(g, fp, *p) or []))


def test_border_leaving_and_nonfinite_fixtures_hold_what_they_claim():
    fams = tc.families()
    g = tc.grid_of("500x200")
    on = lambda fam, i: ref.pose_cells(g, tc.fp_of(fams[fam]["fp"]), *fams[fam]["poses"][0, i]) is not None
    # per side: the edge itself, one ulp inside, one ulp outside.  +x and +y edges belong to the map (t == 0), -x and -y
    # edges do not (t == length)
    assert [on("border_in_from_+x", i) for i in range(3)] == [True, True, False]
    assert [on("border_in_from_-x", i) for i in range(3)] == [False, True, False]
    assert [on("border_in_from_+y", i) for i in range(3)] == [True, True, False]
    assert [on("border_in_from_-y", i) for i in range(3)] == [False, True, False]
    assert [on("border_point", i) for i in range(9)] == [True, False, False, True, True, False, False, True, True]
    assert all(on("border_in_from_+x", i) for i in range(3, 8))
    cells = ref.pose_vertex_cells(g, tc.fp_of("canary"), 40.0, 0.0, 0.0)
    assert cells[1] == (2, 100) and float(np.float32(40.0)) + tc.FOOTPRINTS["canary"][0][0] == 40.7
    for x, y in ((16.0, 0.0), (16.5, 0.5), (20.0, -3.0)):   # exactly on a cell border in both axes
        qx, qy = (g.pos_x + g.off_x - x) / g.res, (g.pos_y + g.off_y - y) / g.res
        assert abs(qx - round(qx)) < 1e-9 and abs(qy - round(qy)) < 1e-9
    # leaving: on the map before `at`, off from it on
    lp, tri = fams["leaving_3x64"]["poses"], tc.fp_of("triangle")
    for k, at in enumerate((0, 31, 63)):
        assert [ref.pose_cells(g, tri, *lp[k, p]) is not None for p in range(64)] == [p < at for p in range(64)]
    # non-finite: trajectory 0 is clean; pose 1 of the others is off the map with the triangle; with the point footprint
    # a NaN or infinite yaw (trajectories 6, 7) scores the centre
    g2 = tc.grid_of("250x100")
    nf = fams["nonfinite_8x3"]["poses"]
    for k in range(8):
        tri_on = [ref.pose_cells(g2, tri, *nf[k, p]) is not None for p in range(3)]
        pt_on = [ref.pose_cells(g2, tc.fp_of("point"), *nf[k, p]) is not None for p in range(3)]
        assert tri_on == [True, k == 0, True] and pt_on == [True, k in (0, 6, 7), True]


def test_error_cases_touch_no_device(gvamd):
    lib = gvamd.load()
    ok = gvamd.Footprint.of(tc.FOOTPRINTS["triangle"])
    n = C.c_int32(-7)
    cells = np.full(64, -3, np.int32)
    p = cells.ctypes.data_as(C.c_void_p)

    def call(fp, gx=50, gy=20, res=0.1, x=5.0, cap=64, out=p, np_=None):
        return lib.gv_footprint_cells(C.c_uint8(gx), C.c_uint8(gy), C.c_double(res), C.byref(fp) if fp is not None else None,
                                      C.c_float(x), C.c_float(0.0), C.c_float(0.3), out, C.c_int32(cap),
                                      C.byref(n) if np_ is None else np_)

    assert call(ok) == 0 and n.value == len(ref.pose_cells(tc.grid_of("500x200"), tc.fp_of("triangle"), 5.0, 0.0, 0.3))
    assert call(ok, x=100.0) == 0 and n.value == -1
    assert call(ok, cap=3) == GV_ERR_BAD_ARG and n.value > 3                      # *n says how many
    assert call(ok, out=None) == GV_ERR_BAD_ARG
    assert call(None) == GV_ERR_BAD_ARG and call(ok, np_=C.POINTER(C.c_int32)()) == GV_ERR_BAD_ARG   # null fp, null n
    for gx, gy, res in ((0, 20, 0.1), (50, 0, 0.1), (50, 20, 0.0), (50, 20, -1.0), (50, 20, float("nan")), (50, 20, float("inf"))):
        assert call(ok, gx, gy, res) == GV_ERR_BAD_ARG
    tri = tc.FOOTPRINTS["triangle"]
    bad = [gvamd.Footprint.of(tri[:1]), gvamd.Footprint.of(tri[:2]), gvamd.Footprint.of(tri, collision_cost=0),
           gvamd.Footprint.of(tri, collision_cost=256), gvamd.Footprint.of(tri, off_map_cost=-1),
           gvamd.Footprint.of(tri, off_map_cost=256), gvamd.Footprint.of(tri, flags=1),
           gvamd.Footprint.of(((float("nan"), 0.0),) + tri[1:]), gvamd.Footprint.of(tri[:2] + ((0.0, float("inf")),))]
    f17 = gvamd.Footprint.of(tc.FOOTPRINTS["poly16"])
    f17.n_vertices = 17
    fneg = gvamd.Footprint.of(tri)
    fneg.n_vertices = -1
    for b in bad + [f17, fneg]:
        assert call(b) == GV_ERR_BAD_ARG, b.n_vertices
        assert lib.gv_set_footprint(None, C.byref(b)) == GV_ERR_BAD_ARG
    nanpast = gvamd.Footprint.of(tri)
    nanpast.vx[5] = float("nan")                   # past n_vertices: never read
    assert call(nanpast) == 0
    assert call(gvamd.Footprint.of((), collision_cost=255, off_map_cost=0)) == 0 and n.value == 1
    assert lib.gv_set_footprint(None, C.byref(ok)) == GV_ERR_BAD_ARG and lib.gv_set_footprint(None, None) == GV_ERR_BAD_ARG
    sc = np.zeros(1, gvamd.TRAJ_SCORE_DTYPE)
    ps = np.zeros(3, np.float32)
    for f in (lib.gv_score_trajectories, lib.gv_score_trajectories_async):
        assert f(None, ps.ctypes.data_as(C.c_void_p), C.c_int32(1), C.c_int32(1), C.c_uint32(0),
                 sc.ctypes.data_as(C.c_void_p), None) == GV_ERR_BAD_ARG
