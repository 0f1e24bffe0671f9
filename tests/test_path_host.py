"""[EXTENSION] X17 path extraction from the distance field, host side (no GPU): the new header, the exports, the binding and
the record's layout; every cell centre back through getIndex to its own cell; the library's host twin (gv_nav_path_host:
the kernel's arithmetic text compiled for the host) against path_ref on every nav case, records, entries and centres byte
for byte; known answers; every status; the cap's edges; the argument errors; the twin under the sanitizers as a
stand-alone program; the kernel's register budget from the compiler's remarks.

test_reference_known_answers exercises path_ref and the fixtures alone: it is the reference's self-check and calls
nothing of the library, so it alone of this file would pass on a tree without the feature; every other test here needs
the new header, the new symbols or the new sources.

Register figures on record (profiles/x17/kernel_resources.txt): k_nav_path 34 VGPRs, 60 SGPRs, 512 bytes of LDS, no
scratch, no spill; k_nav_seeds_path 10 VGPRs, 16 SGPRs."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import nav_cases as nc
import nav_ref
import path_cases as pc
import path_ref as ref
import traj_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grid-vision_amd", "csrc")
GV_ERR_BAD_ARG = 1
NAMES = ["gv_nav_path_async", "gv_nav_path", "gv_nav_path_host", "gv_get_nav_path", "gv_device_nav_path", "gv_nav_field_from_path"]

LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "gridvision_hip_path.h"
#define O(f) printf("%zu ", offsetof(gv_nav_path_info, f))
int main(void)
{
  printf("%zu ", sizeof(gv_nav_path_info));
  O(status); O(n_cells); O(start_value); O(end_value); O(start_entry); O(end_entry); O(n_diagonal); O(reserved);
  printf("%d %d %d %d %d %d %d\n", (int)GV_PATH_DIAGONAL, GV_PATH_REACHED, GV_PATH_TRUNCATED, GV_PATH_OFF_MAP, GV_PATH_BLOCKED,
         GV_PATH_UNREACHABLE, GV_PATH_STUCK);
  return 0;
}
"""


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


def _declared(path):
    txt = open(path).read()
    return sorted(set(re.findall(r"\b(gv_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))))


def test_header_binding_and_layout(gvamd, tmp_path):
    inc = os.path.join(ROOT, "include")
    assert _declared(os.path.join(inc, "gridvision_hip_path.h")) == sorted(NAMES) == sorted(gvamd.PATH_SYMBOLS)
    main_txt = open(os.path.join(inc, "gridvision_hip.h")).read()
    main = _declared(os.path.join(inc, "gridvision_hip.h"))
    assert main == sorted(gvamd.ABI_SYMBOLS) and len(main) == 123 and not set(main) & set(NAMES)
    assert main_txt.count('#include "gridvision_hip_path.h"') == 1
    lib = gvamd.load()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.gv_abi_version() == 4
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "123 entry points" in readme and "gridvision_hip_path.h" in readme
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(LAYOUT)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + inc, src, "-o", exe])
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    for dt in (gvamd.NAV_PATH_INFO_DTYPE, ref.INFO_DTYPE):
        assert dt.itemsize == out[0] == 32
        assert [dt.fields[n][1] for n in dt.names] == out[1:9] == [0, 4, 8, 12, 16, 20, 24, 28]
        assert dt.names == ("status", "n_cells", "start_value", "end_value", "start_entry", "end_entry", "n_diagonal", "reserved")
    assert out[9:] == [gvamd.PATH_DIAGONAL, gvamd.PATH_REACHED, gvamd.PATH_TRUNCATED, gvamd.PATH_OFF_MAP, gvamd.PATH_BLOCKED,
                       gvamd.PATH_UNREACHABLE, gvamd.PATH_STUCK] == [ref.DIAGONAL, ref.REACHED, ref.TRUNCATED, ref.OFF_MAP,
                                                                    ref.BLOCKED_START, ref.UNREACHABLE_START, ref.STUCK]
    assert (gvamd.PATH_MAX_STARTS, gvamd.PATH_MAX_CAP, gvamd.PATH_MAX_CELLS) == (ref.MAX_STARTS, ref.MAX_CAP, ref.MAX_CELLS)
    assert (gvamd.NAV_BLOCKED, gvamd.NAV_UNREACHABLE) == (ref.BLOCKED, ref.UNREACHABLE) == (nav_ref.BLOCKED, nav_ref.UNREACHABLE)
    # the new sources are part of both build recipes
    from gvamd import build as b
    cmake = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    cmake_globs = "file(GLOB GV_HIP_SOURCES RELATIVE ${GV_CSRC} CONFIGURE_DEPENDS ${GV_CSRC}/*.hip)" in cmake   # every .hip of csrc/
    for s in ("gv_api_path.hip", "gv_navpath.hip"):
        assert s in b.SOURCES and cmake_globs and os.path.exists(os.path.join(CSRC, s))


def _round_trip_failures(gvamd, grid, cells):
    """how many of `cells` (entry coordinates) the twin's centre does not take back to its own cell through getIndex"""
    (gx, gy, res), _ = grid
    g = traj_ref.grid(gx, gy, res)
    Xs = [float(ref.centre(g, x, 0)[0]) for x in range(g.nx)]      # the axes are independent: a centre per column and row
    Ys = [float(ref.centre(g, 0, y)[1]) for y in range(g.ny)]
    assert Xs == [float(np.float32(nc.world_of(g, x, 0)[0])) for x in range(g.nx)]
    assert Ys == [float(np.float32(nc.world_of(g, 0, y)[1])) for y in range(g.ny)]
    bad = 0
    for x, y in cells:
        bad += traj_ref.get_index(g, Xs[x], Ys[y]) != (g.nx - 1 - x, g.ny - 1 - y)
    return bad


def test_every_centre_names_its_own_cell(gvamd):
    for name, grid in nc.GRIDS.items():
        nx, ny = grid[1]
        assert _round_trip_failures(gvamd, grid, ((x, y) for y in range(ny) for x in range(nx))) == 0, name
    rng = np.random.default_rng(5)
    big = ((200, 200, 0.1), (2000, 2000))
    cells = [(int(x), int(y)) for x, y in rng.integers(0, 2000, (4000, 2))]
    cells += [(i, j) for i in range(2000) for j in (0, 1999)] + [(j, i) for i in range(2000) for j in (0, 1999)]
    assert _round_trip_failures(gvamd, big, cells) == 0
    # and the twin writes those centres: one path across the whole 2000-cell diagonal of the big grid
    g = traj_ref.grid(200, 200, 0.1)
    ys, xs = np.mgrid[0:2000, 0:2000]
    field = (xs + ys).astype(np.uint32).reshape(-1)
    start = np.array([nc.world_of(g, 1999, 1999)], np.float32)
    info, ent, xy = gvamd.nav_path_host(200, 200, 0.1, field, start, 4096, gvamd.PATH_DIAGONAL)
    assert (int(info[0]["status"]), int(info[0]["n_cells"]), int(info[0]["n_diagonal"])) == (ref.REACHED, 2000, 1999)
    want = np.array([ref.centre(g, i, i) for i in range(1999, -1, -1)], np.float32)
    assert xy[0, :2000].tobytes() == want.tobytes() and ent[0, :2000].tolist() == [i * 2000 + i for i in range(1999, -1, -1)]


def _equal(got, want, tag):
    info, ent, xy = got
    winfo, wents, wxys = want
    assert info.dtype == ref.INFO_DTYPE and info.tobytes() == winfo.tobytes(), (tag, info, winfo)
    for s in range(len(winfo)):
        n = int(winfo[s]["n_cells"])
        assert ent[s, :n].tobytes() == wents[s].tobytes(), (tag, s)
        assert xy[s, :n].tobytes() == wxys[s].tobytes(), (tag, s)


@pytest.mark.parametrize("name", list(nc.cases()))
def test_host_twin_equals_reference(gvamd, name):
    c = nc.cases()[name]
    g = nc.grid_of(c["grid"])
    geo = nc.GRIDS[c["grid"]][0]
    for cfg in pc.CONFIGS:
        field = pc.nav_field(name, cfg)
        step = nav_ref.step_table(*cfg)
        starts = pc.nav_starts(g, field, 100 + len(name))
        for flags in (0, ref.DIAGONAL):
            want = ref.paths(g, field, starts, pc.NAV_CAP, flags)
            assert (want[0]["status"] == ref.REACHED).all() and (want[0]["end_value"] == 0).all(), (name, cfg, flags)
            _equal(gvamd.nav_path_host(*geo, field, starts, pc.NAV_CAP, flags), want, (name, cfg, flags))
            info, ent, _ = gvamd.nav_path_host(*geo, field, starts, pc.NAV_CAP, flags, keep_xy=False)
            assert info.tobytes() == want[0].tobytes()
            for s, cells in enumerate(want[1]):
                vals = field[cells].astype(np.int64)
                assert (np.diff(vals) < 0).all() and int(info[s]["start_value"]) == vals[0]
                if flags == 0:   # 4-connected: the field falls by exactly the step of the cell left, down to the seed
                    assert int(vals[0]) == int(step[c["cost"][cells[:-1]]].astype(np.int64).sum()), (name, cfg, s)
                    assert int(info[s]["n_diagonal"]) == 0
                    if cfg[1] == 0:
                        assert int(info[s]["n_cells"]) == int(vals[0]) + 1
        if name in ("serpentine_200x80", "comb_250x100"):   # every diagonal's flanks are walls or the move gains nothing
            a, b = ref.paths(g, field, starts, pc.NAV_CAP, 0), ref.paths(g, field, starts, pc.NAV_CAP, ref.DIAGONAL)
            assert a[0].tobytes() == b[0].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1]))


def test_reference_known_answers():
    """path_ref alone on what the fixtures state: the longest paths of the corridor maps, the closed forms of the empty map"""
    for name, n in (("serpentine_200x80", 8040), ("comb_250x100", 12625), ("in_tile_200x200", 1830)):
        g = nc.grid_of(nc.cases()[name]["grid"])
        field = pc.nav_field(name, (253, 0))
        info, ents, _ = ref.paths(g, field, pc.nav_starts(g, field, 1)[:1], pc.NAV_CAP)
        assert int(info[0]["n_cells"]) == n == int(info[0]["start_value"]) + 1 and int(info[0]["status"]) == ref.REACHED
        assert int(field[ents[0][-1]]) == 0
    g = nc.grid_of(pc.EMPTY_GRID)
    for goal_name, (gx, gy) in pc.empty_goals(g).items():
        field = pc.empty_field(g, (gx, gy))
        cells = pc.empty_start_cells(g, goal_name)
        starts = pc.empty_starts(g, goal_name)
        for flags in (0, ref.DIAGONAL):
            info, ents, xys = ref.paths(g, field, starts, 512, flags)
            for (x, y), r, e in zip(cells, info, ents):
                dx, dy = abs(x - gx), abs(y - gy)
                assert int(r["status"]) == ref.REACHED and int(r["start_entry"]) == y * g.nx + x and int(r["end_entry"]) == gy * g.nx + gx
                if flags:
                    assert (int(r["n_cells"]), int(r["n_diagonal"])) == (max(dx, dy) + 1, min(dx, dy)), (goal_name, x, y)
                else:
                    assert (int(r["n_cells"]), int(r["n_diagonal"])) == (dx + dy + 1, 0)
                    assert e[:dx + 1].tolist() == [y * g.nx + x + (i if gx > x else -i) for i in range(dx + 1)]   # along x first
    # the families the module promises: flush boundaries, three windows in all eight directions, whole-border paths
    lengths = {abs(x - 125) + abs(y - 50) + 1 for x, y in pc.empty_start_cells(g, "centre")}
    assert set(pc.FLUSH_LENGTHS) <= lengths
    runs = set()
    for goal_name, (gx, gy) in pc.empty_goals(g).items():
        for x, y in pc.empty_start_cells(g, goal_name):
            dx, dy = gx - x, gy - y
            if max(abs(dx), abs(dy)) >= 96 and (dx == 0 or dy == 0 or abs(dx) == abs(dy)):
                runs.add((np.sign(dx), np.sign(dy)))
    assert len(runs) == 8, runs


def _stuck_field(g):
    """a ramp along row 10 that ends in a plateau: 9 8 7 7 7 ..; everything else a higher plateau of 50, one blocked and
    one unreachable cell"""
    f = np.full((g.ny, g.nx), 50, np.uint32)
    f[10, 20:23] = (9, 8, 7)
    f[10, 23:40] = 7
    f[30, 30] = ref.BLOCKED
    f[31, 31] = ref.UNREACHABLE
    return f.reshape(-1)


def test_every_status(gvamd):
    g = nc.grid_of("200x80")
    geo = nc.GRIDS["200x80"][0]
    field = _stuck_field(g)
    cells = [(20, 10), (100, 60), (30, 30), (31, 31)]
    starts = np.array([nc.world_of(g, *c) for c in cells] + [(1e6, 0.0), (np.nan, 0.0), (0.0, np.inf)], np.float32)
    for flags in (0, ref.DIAGONAL):
        want = ref.paths(g, field, starts, 8, flags)
        _equal(gvamd.nav_path_host(*geo, field, starts, 8, flags), want, ("stuck", flags))
        info = want[0]
        assert info["status"].tolist() == [ref.STUCK, ref.STUCK, ref.BLOCKED_START, ref.UNREACHABLE_START] + [ref.OFF_MAP] * 3
        assert info["n_cells"].tolist() == [3, 1, 0, 0, 0, 0, 0] and int(info[0]["end_value"]) == 7
        assert int(info[0]["end_entry"]) == 10 * g.nx + 22 and int(info[1]["end_entry"]) == int(info[1]["start_entry"])
        assert info["start_entry"].tolist()[2:] == [30 * g.nx + 30, 31 * g.nx + 31, -1, -1, -1]
        assert info["end_entry"].tolist()[2:] == [-1] * 5 and (info["reserved"] == 0).all()
        assert info["start_value"].tolist()[2:] == [ref.BLOCKED, ref.UNREACHABLE] + [ref.BLOCKED] * 3
        assert info["end_value"].tolist()[2:] == info["start_value"].tolist()[2:]
    # a cut corner: the diagonal neighbour is lower but one flank is blocked
    f = np.full((g.ny, g.nx), 50, np.uint32)
    f[20, 20], f[21, 21], f[20, 21] = 10, 0, ref.BLOCKED
    one = np.array([nc.world_of(g, 20, 20)], np.float32)
    got = gvamd.nav_path_host(*geo, f.reshape(-1), one, 8, ref.DIAGONAL)
    _equal(got, ref.paths(g, f.reshape(-1), one, 8, ref.DIAGONAL), "corner")
    assert int(got[0][0]["status"]) == ref.STUCK
    f[20, 21] = 50
    got = gvamd.nav_path_host(*geo, f.reshape(-1), one, 8, ref.DIAGONAL)
    assert (int(got[0][0]["status"]), int(got[0][0]["n_cells"]), int(got[0][0]["n_diagonal"])) == (ref.REACHED, 2, 1)


def test_cap_edges(gvamd):
    name = "pocket_inside"
    c = nc.cases()[name]
    g = nc.grid_of(c["grid"])
    geo = nc.GRIDS[c["grid"]][0]
    field = pc.nav_field(name, (253, 0))
    start = pc.nav_starts(g, field, 3)[:1]
    n = int(ref.paths(g, field, start, 4096)[0][0]["n_cells"])
    assert n > 3
    for cap, status, cells in ((n - 1, ref.TRUNCATED, n - 1), (n, ref.REACHED, n), (n + 1, ref.REACHED, n), (1, ref.TRUNCATED, 1)):
        want = ref.paths(g, field, start, cap)
        got = gvamd.nav_path_host(*geo, field, start, cap)
        _equal(got, want, ("cap", cap))
        assert (int(got[0][0]["status"]), int(got[0][0]["n_cells"])) == (status, cells), cap
        assert int(got[0][0]["end_value"]) == int(field[got[1][0, cells - 1]])
    goal = gvamd.nav_path_host(*geo, field, c["goal"], 1)          # a start on the seed: one cell, reached, also at cap 1
    assert (int(goal[0][0]["status"]), int(goal[0][0]["n_cells"]), int(goal[0][0]["start_value"])) == (ref.REACHED, 1, 0)


def test_argument_errors(gvamd):
    lib = gvamd.load()
    g = nc.grid_of("200x80")
    field = pc.empty_field(g, (5, 5))
    starts = np.zeros((257, 2), np.float32)
    info = np.zeros(257, gvamd.NAV_PATH_INFO_DTYPE)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731

    def call(S=1, cap=4, flags=0, field_=field, starts_=starts, info_=info, gx=10, gy=4, res=0.05):
        return lib.gv_nav_path_host(C.c_uint8(gx), C.c_uint8(gy), C.c_double(res), p(field_), p(starts_), C.c_int32(S), C.c_int32(cap),
                                    C.c_uint32(flags), p(info_), None, None)

    assert call() == 0 and call(S=256, cap=4096) == 0 and call(S=16, cap=65536) == 0 and call(flags=1) == 0
    before = info.tobytes()
    for kw in (dict(S=0), dict(S=-1), dict(S=257), dict(cap=0), dict(cap=-1), dict(cap=65537), dict(S=17, cap=65536),
               dict(S=256, cap=4097), dict(flags=2), dict(flags=3), dict(field_=None), dict(starts_=None), dict(info_=None),
               dict(gx=0), dict(gy=0), dict(res=0.0), dict(res=float("nan"))):
        assert call(**kw) == GV_ERR_BAD_ARG, kw
    assert info.tobytes() == before
    with pytest.raises(gvamd.GVError) as e:
        gvamd.nav_path_host(10, 4, 0.05, field, starts[:1], 0)
    assert e.value.code == GV_ERR_BAD_ARG


SAN_MAIN = r"""
// the host twin on a 20 x 10 field under the sanitizers: starts in every corner and on every border (the neighbour tests
// of path_next at the array's ends), off the map, on a blocked cell; caps 1, 7 and 64; both connectivities
#include <cstdio>
#include <cstdint>
#include <vector>
#include "gridvision_hip_path.h"
int main()
{
  const int nx = 20, ny = 10;
  std::vector<uint32_t> field((size_t)nx * ny);
  for (int y = 0; y < ny; ++y)
    for (int x = 0; x < nx; ++x) field[(size_t)y * nx + x] = (uint32_t)((x > 13 ? x - 13 : 13 - x) + (y > 4 ? y - 4 : 4 - y));
  for (int y = 2; y < 8; ++y) field[(size_t)y * nx + 9] = GV_NAV_BLOCKED;
  field[3] = GV_NAV_UNREACHABLE;
  // cell centres of the geometry gv_create(2, 1, 0.1) gives: the map's centre is (0, 0)
  std::vector<float> starts;
  const int cells[][2] = {{0, 0}, {19, 0}, {0, 9}, {19, 9}, {7, 0}, {7, 9}, {0, 5}, {19, 5}, {8, 5}, {9, 5}, {3, 0}, {13, 4}};
  for (const auto &c : cells) {
    starts.push_back((float)(1.0 - ((double)(nx - 1 - c[0]) + 0.5) * 0.1));
    starts.push_back((float)(0.5 - ((double)(ny - 1 - c[1]) + 0.5) * 0.1));
  }
  starts.push_back(5.0f); starts.push_back(0.0f);
  const int S = (int)starts.size() / 2;
  uint64_t h = 1469598103934665603ull;
  const int caps[] = {1, 7, 64};
  for (int cap : caps)
    for (uint32_t flags = 0; flags < 2; ++flags) {
      std::vector<gv_nav_path_info> info((size_t)S);
      std::vector<int32_t> entries((size_t)S * cap);      // exactly the room the call may use
      std::vector<float> xy((size_t)S * cap * 2);
      if (gv_nav_path_host(2, 1, 0.1, field.data(), starts.data(), S, cap, flags, info.data(), entries.data(), xy.data())) return 2;
      if (gv_nav_path_host(2, 1, 0.1, field.data(), starts.data(), S, cap, flags, info.data(), nullptr, nullptr)) return 3;
      for (int s = 0; s < S; ++s) {
        const unsigned char *b = (const unsigned char *)&info[(size_t)s];
        for (size_t i = 0; i < sizeof(gv_nav_path_info); ++i) h = (h ^ b[i]) * 1099511628211ull;
        for (int k = 0; k < info[(size_t)s].n_cells; ++k) h = (h ^ (uint64_t)(uint32_t)entries[(size_t)s * cap + k]) * 1099511628211ull;
      }
    }
  std::printf("%llu\n", (unsigned long long)h);
  return 0;
}
"""


def test_twin_under_the_sanitizers(gvamd, tmp_path):
    src, exe = str(tmp_path / "san.cpp"), str(tmp_path / "san")
    with open(src, "w") as f:
        f.write(SAN_MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), src, "-x", "c++", os.path.join(CSRC, "gv_api_planner_host.hip"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    # the same calls through the library, the same digest
    nx, ny = 20, 10
    g = traj_ref.grid(2, 1, 0.1)
    assert (g.nx, g.ny) == (nx, ny)
    ys, xs = np.mgrid[0:ny, 0:nx]
    field = (np.abs(xs - 13) + np.abs(ys - 4)).astype(np.uint32)
    field[2:8, 9] = ref.BLOCKED
    field[0, 3] = ref.UNREACHABLE
    cells = [(0, 0), (19, 0), (0, 9), (19, 9), (7, 0), (7, 9), (0, 5), (19, 5), (8, 5), (9, 5), (3, 0), (13, 4)]
    starts = np.array([ref.centre(g, *c) for c in cells] + [(5.0, 0.0)], np.float32)
    h = 1469598103934665603
    statuses = set()
    for cap in (1, 7, 64):
        for flags in (0, 1):
            info, ent, xy = gvamd.nav_path_host(2, 1, 0.1, field, starts, cap, flags)
            _equal((info, ent, xy), ref.paths(g, field.reshape(-1), starts, cap, flags), ("san", cap, flags))
            statuses |= set(info["status"].tolist())
            for s in range(len(starts)):
                for v in info[s].tobytes():
                    h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
                for e in ent[s, :int(info[s]["n_cells"])]:
                    h = ((h ^ int(np.uint32(e))) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    # (the wall makes the closed form no geodesic field: the start beside it walks into a local minimum and is stuck)
    assert statuses == {ref.REACHED, ref.TRUNCATED, ref.OFF_MAP, ref.BLOCKED_START, ref.UNREACHABLE_START, ref.STUCK}
    assert int(r.stdout.strip()) == h


def _have_hipcc() -> bool:
    return any(c and os.path.exists(c) for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")))


@pytest.mark.skipif(not _have_hipcc(), reason="hipcc not installed")
def test_kernel_resources(tmp_path):
    """gv_navpath.hip device-only with the library's flags: no scratch and no spill of either kind; the 128-cell buffer
    of collected cells is the kernel's whole LDS; at most 64 vector registers, so that registers allow the 8 wavefronts
    per SIMD the hardware has slots for"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    _, text = kr.compile_file("gv_navpath.hip", str(tmp_path))
    rows = {k: v for k, v in kr.parse_remarks(text).items()}
    path = [v for k, v in rows.items() if "k_nav_path" in k]
    seeds = [v for k, v in rows.items() if "k_nav_seeds_path" in k]
    assert len(path) == 1 and len(seeds) == 1, sorted(rows)
    for r in path + seeds:
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert path[0]["lds"] == 128 * 4 and path[0]["vgprs"] <= 64, path[0]
