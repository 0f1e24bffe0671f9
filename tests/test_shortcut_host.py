"""[EXTENSION] X21 shortcuts and waypoints without a GPU: the header, the binding and the struct layouts;
gvx3_shortcut_host (the library's host twin) against shortcut_ref, a plain Python reference written from the header, on
every fixture of shortcut_cases.py, byte for byte; the hand-computed answers of the definition; the error table; the twin
as a stand-alone program under AddressSanitizer and UBSan; and the host file as plain C++.
test_fixtures_are_what_they_claim and test_known_answers_of_the_reference are the only tests here that pass without the
feature: they exercise the fixtures and the reference alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import shortcut_cases as sc
import shortcut_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grid-vision_amd", "csrc")
INC = os.path.join(ROOT, "include")
HDR = "gridvision_hip_shortcut.h"
NAMES = ["gvx3_set_shortcut_config", "gvx3_shortcut_async", "gvx3_shortcut", "gvx3_shortcut_host", "gvx3_get_shortcut",
         "gvx3_device_shortcut", "gvx3_nav_field_from_shortcut"]
GV_ERR_BAD_ARG = 1

LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "gridvision_hip_shortcut.h"
#define O(t, f) printf("%zu ", offsetof(t, f))
int main(void)
{
  printf("%zu ", sizeof(gvx3_shortcut_config));
  O(gvx3_shortcut_config, max_cost); O(gvx3_shortcut_config, window); O(gvx3_shortcut_config, spacing); O(gvx3_shortcut_config, reserved);
  printf("%zu ", sizeof(gvx3_shortcut_info));
  O(gvx3_shortcut_info, status); O(gvx3_shortcut_info, n_waypoints); O(gvx3_shortcut_info, n_anchors); O(gvx3_shortcut_info, n_src);
  O(gvx3_shortcut_info, n_steps); O(gvx3_shortcut_info, n_diag_steps); O(gvx3_shortcut_info, max_cost_seen); O(gvx3_shortcut_info, end_entry);
  printf("%u %d %d %d %d %d %d %d\n", GVX3_SHORTCUT_NO_CORNER, GVX3_SHORTCUT_OK, GVX3_SHORTCUT_TRUNCATED, GVX3_SHORTCUT_EMPTY,
         GVX3_SHORTCUT_MAX_WINDOW, GVX3_SHORTCUT_MAX_SPACING, GVX3_SHORTCUT_MAX_WCAP, GVX3_SHORTCUT_MAX_CELLS);
  return 0;
}
"""

# the twin over a case written to a file by the test: what the sanitizers watch
SAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "gridvision_hip_shortcut.h"
int main(int argc, char **argv)
{
  if (argc != 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t hd[7];   // grid_x, grid_y, G, S, cap, wcap, flags
  double res;
  gvx3_shortcut_config cfg;
  if (std::fread(hd, sizeof(hd), 1, f) != 1 || std::fread(&res, sizeof(res), 1, f) != 1 || std::fread(&cfg, sizeof(cfg), 1, f) != 1) return 4;
  const size_t G = (size_t)hd[2], S = (size_t)hd[3], cap = (size_t)hd[4], wcap = (size_t)hd[5];
  std::vector<uint8_t> cost(G);
  std::vector<int32_t> n(S), src(S * cap);
  if (std::fread(cost.data(), 1, G, f) != G) return 5;
  if (std::fread(n.data(), 4, S, f) != S) return 6;
  if (std::fread(src.data(), 4, S * cap, f) != S * cap) return 7;
  std::fclose(f);
  // exactly as large as the call may write: a store past wcap waypoints of a path is a store past the block
  std::vector<gvx3_shortcut_info> info(S);
  std::vector<int32_t> entries(S * wcap), index(S * wcap);
  std::vector<float> xy(2 * S * wcap);
  const int rc = gvx3_shortcut_host((uint8_t)hd[0], (uint8_t)hd[1], res, cost.data(), &cfg, src.data(), n.data(), hd[3], hd[4], hd[5],
                                    (uint32_t)hd[6], info.data(), entries.data(), index.data(), xy.data());
  if (rc) return 10 + rc;
  FILE *o = std::fopen(argv[2], "wb");
  if (!o) return 8;
  std::fwrite(info.data(), sizeof(gvx3_shortcut_info), S, o);
  for (size_t s = 0; s < S; ++s) {
    const size_t k = (size_t)info[s].n_waypoints;
    std::fwrite(entries.data() + s * wcap, 4, k, o);
    std::fwrite(index.data() + s * wcap, 4, k, o);
    std::fwrite(xy.data() + 2 * s * wcap, 4, 2 * k, o);
  }
  std::fclose(o);
  return 0;
}
"""


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


@pytest.fixture(scope="module")
def wanted():
    """the reference's result of every case, computed once"""
    return {name: ref.shortcut(sc.grid_of(c["grid"]), c["cost"], c["cfg"], c["paths"], c["wcap"], c["flags"]) for name, c in sc.cases().items()}


def packed(paths, cap):
    """(src_entries int32 (S, cap), src_n int32 (S,)) of entry lists; the slots past a path's cells hold a poison entry"""
    src = np.full((len(paths), cap), -12345, np.int32)
    for s, p in enumerate(paths):
        src[s, :len(p)] = p
    return src, np.array([len(p) for p in paths], np.int32)


def same(got, want, tag):
    """byte equality of the records and of entries, index and xy up to n_waypoints"""
    info, ent, idx, xy = got
    winfo, wents, widxs, wxys = want
    assert np.asarray(info).tobytes() == winfo.tobytes(), (tag, info[:4], winfo[:4])
    for s in range(len(winfo)):
        n = int(winfo[s]["n_waypoints"])
        if ent is not None:
            assert ent[s, :n].tobytes() == wents[s].tobytes(), (tag, s, ent[s, :n][:8], wents[s][:8])
        if idx is not None:
            assert idx[s, :n].tobytes() == widxs[s].tobytes(), (tag, s, idx[s, :n][:8], widxs[s][:8])
        if xy is not None:
            assert xy[s, :n].tobytes() == wxys[s].tobytes(), (tag, s)


def twin(gvamd, c, paths=None, wcap=None, flags=None, cfg=None, cost=None):
    src, n = packed(c["paths"] if paths is None else paths, c["cap"])
    return gvamd.shortcut_host(*sc.GRIDS[c["grid"]][0], c["cost"] if cost is None else cost, gvamd.ShortcutConfig.of(**(cfg or c["cfg"])), src, n,
                               c["wcap"] if wcap is None else wcap, c["flags"] if flags is None else flags)


# -------------------------------------------------------------------------- the fixtures and the reference alone --
@pytest.mark.parametrize("name", list(sc.cases()))
def test_fixtures_are_what_they_claim(wanted, name):
    c = sc.cases()[name]
    (gx, gy, res), (nx, ny) = sc.GRIDS[c["grid"]]
    g = sc.grid_of(c["grid"])
    assert (g.nx, g.ny) == (nx, ny) == c["mask"].shape[::-1] and (nx % 4 != 0 or c["grid"] == "640x640")
    assert c["cost"].shape == (nx * ny,) and np.array_equal(c["cost"] == 254, c["mask"].reshape(-1))
    assert 1 <= len(c["paths"]) <= 256 and len(c["paths"]) * c["wcap"] <= ref.MAX_CELLS
    for p, s in zip(c["paths"], c["starts"]):
        assert all(0 <= e < nx * ny for e in p) and (len(p) == 0) == (s is None)
        if c["gpu"] and p:
            assert p[0] == sc.ent(c["grid"], *s) and p[-1] == sc.ent(c["grid"], *c["goal"])   # where the device's descent starts and ends
    sc.check(name, c, *wanted[name])


def test_the_cases_the_feature_was_asked_to_cover():
    cs = sc.cases()
    assert {c["cfg"]["window"] for c in cs.values()} >= {1, 63, 64, 65, 127, 128, 129, 4096}
    assert {c["cfg"]["spacing"] for c in cs.values()} >= {0, 1, 2, 10, 11}
    assert {"pillar", "wall_gap", "diagonal_pair", "diagonal_pair_no_corner", "cost_at_max", "cost_above_max", "path_above_max",
            "octants_both_ways", "octants", "between_63_64_65_129", "wcap_exact", "wcap_on_anchor", "wcap_mid_segment", "s256", "map_edge",
            "lengths", "w1_spacing1", "random_640"} <= set(cs)
    assert [n for n, c in cs.items() if c["grid"] == "640x640"] == ["random_640"]
    assert len(cs["s256"]["paths"]) == 256 and not cs["octants_both_ways"]["gpu"]


def _hand(lethal, path, wcap=64, flags=0, **cfg):
    """the reference on a 130 x 70 map, cells as (x, y): (record, [(x, y)], [index])"""
    cost = np.where(sc.mask_of("130x70", lethal).reshape(-1), 254, 0).astype(np.uint8)
    info, ents, idxs, _ = ref.shortcut(sc.grid_of("130x70"), cost, ref.config(**cfg), [[y * 130 + x for x, y in path]], wcap, flags)
    return info[0], [(int(e) % 130, int(e) // 130) for e in ents[0]], idxs[0].tolist()


L16 = [(x, 0) for x in range(11)] + [(10, y) for y in range(1, 6)]             # (0,0) .. (10,0), (10,1) .. (10,5)
PAIR = [(0, 0), (1, 0), (2, 0), (3, 0), (3, 1), (3, 2), (3, 3)]


def test_known_answers_of_the_reference():
    """the answers worked out by hand in the definition, on the 16-cell L"""
    r, w, i = _hand([], L16, window=64, spacing=0)
    assert (w, i) == ([(0, 0), (10, 5)], [0, 15]) and r.tolist() == (ref.OK, 2, 2, 16, 10, 5, 0, 5 * 130 + 10)
    r, w, i = _hand([], L16, window=64, spacing=4)
    assert (w, i) == ([(0, 0), (4, 2), (8, 4), (10, 5)], [0, -1, -1, 15])
    r, w, i = _hand([], L16, window=64, spacing=5)
    assert w == [(0, 0), (5, 3), (10, 5)]
    r, w, i = _hand([], L16, window=4, spacing=0)
    assert i == [0, 4, 8, 12, 15] and (int(r["n_steps"]), int(r["n_diag_steps"])) == (13, 2)
    r, w, i = _hand([], L16, wcap=7, window=64, spacing=1)
    assert int(r["status"]) == ref.TRUNCATED and w[-1] == (6, 3) and len(w) == 7 and int(r["end_entry"]) == 3 * 130 + 6
    # the pillar at (6, 2): 1 .. 12 visible from cell 0, 13 and 14 not, 15 again
    cost = np.where(sc.mask_of("130x70", [(6, 2)]).reshape(-1), 254, 0).tolist()
    assert [ref.visible(cost, 130, 252, False, (0, 0), q) for q in L16[1:]] == [True] * 12 + [False, False, True]
    assert _hand([(6, 2)], L16, window=64)[2] == [0, 15]
    # the diagonal pair
    assert _hand([(2, 1), (1, 2)], PAIR, window=64)[2] == [0, 6]
    assert _hand([(2, 1), (1, 2)], PAIR, window=64, flags=ref.NO_CORNER)[2] == [0, 3, 6]
    # the line is directional
    assert ref.line((0, 0), (2, 1)) == [(0, 0), (1, 1), (2, 1)] and ref.line((2, 1), (0, 0)) == [(2, 1), (1, 0), (0, 0)]


# --------------------------------------------------------------------------------------- header, binding, layout --
def _declared(path, prefix):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(%s_[a-z0-9_]+)\s*\(" % prefix, txt)))


def test_header_binding_and_layout(gvamd, tmp_path):
    hdr = os.path.join(INC, HDR)
    assert _declared(hdr, "gvx3") == sorted(NAMES) == sorted(gvamd.SHORTCUT_SYMBOLS)
    assert _declared(hdr, "gv") == [] and _declared(hdr, "gvx") == [] and _declared(hdr, "gvx2") == []
    others = (gvamd.ABI_SYMBOLS + gvamd.MATCH_SYMBOLS + gvamd.SEARCH_SYMBOLS + gvamd.PATH_SYMBOLS + gvamd.FRONTIER_SYMBOLS +
              gvamd.GAIN_SYMBOLS)
    assert not set(NAMES) & set(others)
    txt = open(hdr).read()
    assert '#include "gridvision_hip.h"' in txt and "owns its prefix" in txt.lower() and "gridvision_hip_gain.h" not in txt
    for other in os.listdir(INC):                                              # included by nothing
        if other != HDR:
            assert HDR not in open(os.path.join(INC, other)).read(), other
    from gvamd import build as b
    nm = subprocess.run(["nm", "-D", "--defined-only", b.LIB], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (gvx3_[A-Za-z0-9_]+)$", nm, flags=re.M)) == sorted(NAMES)
    assert sorted(re.findall(r" T (gvx2_[A-Za-z0-9_]+)$", nm, flags=re.M)) == sorted(gvamd.GAIN_SYMBOLS)       # gvx2_ untouched
    assert sorted(re.findall(r" T (gvx_[A-Za-z0-9_]+)$", nm, flags=re.M)) == sorted(gvamd.FRONTIER_SYMBOLS)    # gvx_ untouched
    exported = set(re.findall(r" [A-Za-z] (gv_[A-Za-z0-9_]+)$", nm, flags=re.M))
    assert not {s for s in exported if "shortcut" in s}                        # no new gv_ symbol
    lib = gvamd.load()
    assert all(hasattr(lib, s) for s in NAMES) and lib.gv_abi_version() == 4
    assert hdr in b._headers()
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(LAYOUT)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + INC, src, "-o", exe])
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert C.sizeof(gvamd.ShortcutConfig) == out[0] == 32
    assert [getattr(gvamd.ShortcutConfig, n).offset for n, _ in gvamd.ShortcutConfig._fields_] == out[1:5] == [0, 4, 8, 12]
    info_off = [0, 4, 8, 12, 16, 20, 24, 28]
    assert out[5] == 32 and out[6:14] == info_off
    for dt in (gvamd.SHORTCUT_INFO_DTYPE, ref.INFO_DTYPE):
        assert dt.itemsize == 32 and [dt.fields[n][1] for n in dt.names] == info_off
    assert gvamd.SHORTCUT_INFO_DTYPE == ref.INFO_DTYPE
    consts = [gvamd.SHORTCUT_NO_CORNER, gvamd.SHORTCUT_OK, gvamd.SHORTCUT_TRUNCATED, gvamd.SHORTCUT_EMPTY, gvamd.SHORTCUT_MAX_WINDOW,
              gvamd.SHORTCUT_MAX_SPACING, gvamd.SHORTCUT_MAX_WCAP, gvamd.SHORTCUT_MAX_CELLS]
    assert out[14:22] == consts == [ref.NO_CORNER, ref.OK, ref.TRUNCATED, ref.EMPTY, ref.MAX_WINDOW, ref.MAX_SPACING, ref.MAX_WCAP, ref.MAX_CELLS]


# ------------------------------------------------------------------------------------------ twin against reference --
@pytest.mark.parametrize("name", list(sc.cases()))
def test_twin_against_reference(gvamd, wanted, name):
    c = sc.cases()[name]
    same(twin(gvamd, c), wanted[name], name)
    other = c["flags"] ^ ref.NO_CORNER                                         # and the same paths under the other flag
    want = ref.shortcut(sc.grid_of(c["grid"]), c["cost"], c["cfg"], c["paths"], c["wcap"], other)
    same(twin(gvamd, c, flags=other), want, (name, "other flag"))


def test_twin_gives_the_hand_computed_answers(gvamd):
    """the table of the definition through the twin itself"""
    g = "130x70"
    base = dict(grid=g, cap=64, wcap=64, flags=0)

    def run(lethal, path, wcap=64, flags=0, **cfg):
        cost = np.where(sc.mask_of(g, lethal).reshape(-1), 254, 0).astype(np.uint8)
        info, ent, idx, _ = twin(gvamd, base, paths=[[y * 130 + x for x, y in path]], wcap=wcap, flags=flags, cfg=ref.config(**cfg), cost=cost)
        n = int(info[0]["n_waypoints"])
        return info[0], [(int(e) % 130, int(e) // 130) for e in ent[0, :n]], idx[0, :n].tolist()

    r, w, i = run([], L16, window=64, spacing=0)
    assert (w, i) == ([(0, 0), (10, 5)], [0, 15]) and r.tolist() == (ref.OK, 2, 2, 16, 10, 5, 0, 5 * 130 + 10)
    assert run([], L16, window=64, spacing=4)[1:] == ([(0, 0), (4, 2), (8, 4), (10, 5)], [0, -1, -1, 15])
    assert run([], L16, window=64, spacing=5)[1] == [(0, 0), (5, 3), (10, 5)]
    r, w, i = run([], L16, window=4, spacing=0)
    assert i == [0, 4, 8, 12, 15] and (int(r["n_steps"]), int(r["n_diag_steps"])) == (13, 2)
    r, w, i = run([], L16, wcap=7, window=64, spacing=1)
    assert int(r["status"]) == ref.TRUNCATED and w[-1] == (6, 3) and len(w) == 7
    assert run([(6, 2)], L16, window=64)[2] == [0, 15]
    assert run([(2, 1), (1, 2)], PAIR, window=64)[2] == [0, 6]
    assert run([(2, 1), (1, 2)], PAIR, window=64, flags=ref.NO_CORNER)[2] == [0, 3, 6]


def test_twin_errors(gvamd):
    """the error table of the calls that touch no device"""
    lib = gvamd.load()
    c = sc.cases()["lengths"]
    S, cap = len(c["paths"]), 70
    src, n = packed(c["paths"], cap)
    info = np.zeros(257, ref.INFO_DTYPE)
    ent, idx, xy = np.zeros(1 << 20, np.int32), np.zeros(1 << 20, np.int32), np.zeros(2 << 20, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731

    def host(gx=25, gy=10, res=0.1, co=c["cost"], cfg=c["cfg"], sr=src, sn=n, S=S, cap=cap, wcap=64, flags=0, inf=info, e=ent, i=idx, x=xy):
        q = gvamd.ShortcutConfig.of(**cfg) if isinstance(cfg, dict) else cfg
        return lib.gvx3_shortcut_host(C.c_uint8(gx), C.c_uint8(gy), C.c_double(res), p(co), C.byref(q) if q is not None else None, p(sr), p(sn),
                                      C.c_int32(S), C.c_int32(cap), C.c_int32(wcap), C.c_uint32(flags), p(inf), p(e), p(i), p(x))

    assert host() == 0 and host(e=None, i=None, x=None) == 0 and host(flags=ref.NO_CORNER) == 0 and host(wcap=1) == 0
    assert host(wcap=65536) == 0 and host(S=1) == 0                            # 8 * 65536 <= 2^20
    off, neg, long_ = src.copy(), src.copy(), n.copy()
    off[4, 10] = 250 * 100
    neg[0, 0] = -1
    long_[3] = cap + 1
    bad = [dict(co=None), dict(cfg=None), dict(sr=None), dict(sn=None), dict(inf=None), dict(flags=2), dict(wcap=0), dict(wcap=65537), dict(wcap=-1),
           dict(S=0), dict(S=257), dict(cap=0), dict(cap=65537), dict(gx=0), dict(gy=0), dict(res=0.0), dict(res=float("nan")), dict(res=-0.1),
           dict(sr=off), dict(sr=neg), dict(sn=long_), dict(sn=-n - 1)]
    bad += [dict(cfg={**ref.config(), **k}) for k in (dict(max_cost=-1), dict(max_cost=255), dict(window=0), dict(window=4097), dict(spacing=-1),
                                                     dict(spacing=65536))]
    for kw in bad:
        assert host(**kw) == GV_ERR_BAD_ARG, kw
    many = np.zeros((17, 4), np.int32)
    assert host(sr=many, sn=np.ones(17, np.int32), S=17, cap=4, wcap=65536) == GV_ERR_BAD_ARG      # S * wcap above 2^20
    assert host(sr=many, sn=np.ones(17, np.int32), S=16, cap=4, wcap=65536) == 0
    poison = src.copy()
    poison[4, 64:] = 1 << 30                                                   # behind a path's cells nothing is read
    assert host(sr=poison) == 0
    for k in range(5):
        q = gvamd.ShortcutConfig.of(**ref.config())
        q.reserved[k] = 1
        assert host(cfg=q) == GV_ERR_BAD_ARG
    for edge in (dict(max_cost=0), dict(max_cost=254), dict(window=1), dict(window=4096), dict(spacing=0), dict(spacing=65535)):
        assert host(cfg={**ref.config(), **edge}) == 0, edge
    # the handle calls refuse a null handle before anything else
    assert lib.gvx3_set_shortcut_config(None, None) == GV_ERR_BAD_ARG
    for fn in (lib.gvx3_shortcut, lib.gvx3_shortcut_async):
        assert fn(None, C.c_int32(8), C.c_uint32(0), p(info), None) == GV_ERR_BAD_ARG
    assert lib.gvx3_get_shortcut(None, C.c_int32(0), None, None, None, C.c_int32(0), None) == GV_ERR_BAD_ARG
    assert lib.gvx3_device_shortcut(None, None, None, None, None, None, None) == GV_ERR_BAD_ARG
    assert lib.gvx3_nav_field_from_shortcut(None, C.c_int32(0), None) == GV_ERR_BAD_ARG


# --------------------------------------------------------------------------------- plain C++, and the sanitizers --
def test_host_file_is_plain_cpp(tmp_path):
    """g++ alone compiles gv_api_shortcut_host.hip and gv_shortcut.hpp given only the public include directory"""
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + INC, "-x", "c++", "-c",
                           os.path.join(CSRC, "gv_api_shortcut_host.hip"), "-o", str(tmp_path / "host.o")])
    one = str(tmp_path / "hdr.cpp")
    with open(one, "w") as f:
        f.write('#include "%s"\n' % os.path.join(CSRC, "gv_shortcut.hpp"))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + INC, "-c", one, "-o", str(tmp_path / "hdr.o")])
    for name in ("gv_shortcut.hpp", "gv_api_shortcut_host.hip"):
        txt = open(os.path.join(CSRC, name)).read()
        assert "__HIPCC__" not in txt and "hip_runtime" not in txt and "gv_context.hpp" not in txt, name
    assert '#include "gv_shortcut.hpp"' in open(os.path.join(CSRC, "gv_launch_shortcut.hpp")).read()     # the kernels compile that text
    for name in ("gv_shortcut.hip", "gv_api_shortcut_host.hip"):
        txt = open(os.path.join(CSRC, name)).read()
        assert "shortcut_visible_chunk(" in txt and "shortcut_waypoint(" in txt and "line_cell(" in txt, name


def test_twin_under_sanitizers(tmp_path, wanted):
    """the twin as a stand-alone program with its own main under AddressSanitizer and UBSan, its output blocks exactly
    S * wcap long, over cases that run along the map's edges and into its corners, truncate at wcap, have empty sources and
    256 paths; its bytes are the reference's"""
    exe, src = str(tmp_path / "twin_san"), str(tmp_path / "main.cpp")
    with open(src, "w") as f:
        f.write(SAN_MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-I" + INC, src, "-x", "c++", os.path.join(CSRC, "gv_api_shortcut_host.hip"), "-o", exe])
    for name in ("map_edge", "map_edge_far_corner", "lengths", "wcap_mid_segment", "wcap_1", "s256", "octants_both_ways_no_corner", "w130"):
        c = sc.cases()[name]
        (gx, gy, res), (nx, ny) = sc.GRIDS[c["grid"]]
        cfg = c["cfg"]
        S = len(c["paths"])
        cap = max(max(len(p) for p in c["paths"]), 1)                          # no slack behind the longest path either
        srcs, n = packed(c["paths"], cap)
        inp, outp = str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))
        with open(inp, "wb") as f:
            f.write(np.array([gx, gy, nx * ny, S, cap, c["wcap"], c["flags"]], np.int32).tobytes())
            f.write(np.float64(res).tobytes())
            f.write(np.array([cfg["max_cost"], cfg["window"], cfg["spacing"], 0, 0, 0, 0, 0], np.int32).tobytes())
            f.write(c["cost"].tobytes())
            f.write(n.tobytes())
            f.write(srcs.tobytes())
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (name, r.returncode, r.stderr[-2000:])
        info, ents, idxs, xys = wanted[name]
        want = info.tobytes() + b"".join(e.tobytes() + i.tobytes() + x.tobytes() for e, i, x in zip(ents, idxs, xys))
        assert open(outp, "rb").read() == want, name
