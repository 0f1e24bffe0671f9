"""[EXTENSION] X20 information gain without a GPU: the header, the binding and the struct layouts; gvx2_gain_host (the
library's host twin) against gain_ref, a plain Python reference written from the header, on every fixture of
gain_cases.py, byte for byte; hand-computed answers; the error table; the twin as a stand-alone program under
AddressSanitizer and UBSan; and the host file as plain C++.  test_fixtures_are_what_they_claim and
test_known_answers_of_the_reference are the only tests here that pass without the feature: they exercise the fixtures and
the reference alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gain_cases as gc
import gain_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grid-vision_amd", "csrc")
INC = os.path.join(ROOT, "include")
NAMES = ["gvx2_set_gain_config", "gvx2_gain_async", "gvx2_gain", "gvx2_frontier_gain_async", "gvx2_frontier_gain", "gvx2_gain_host",
         "gvx2_device_gain", "gvx2_nav_field_from_gain"]
GV_ERR_BAD_ARG = 1

LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "gridvision_hip_gain.h"
#define O(t, f) printf("%zu ", offsetof(t, f))
int main(void)
{
  printf("%zu ", sizeof(gvx2_gain_config));
  O(gvx2_gain_config, free_max); O(gvx2_gain_config, unknown_min); O(gvx2_gain_config, unknown_max); O(gvx2_gain_config, radius);
  O(gvx2_gain_config, min_gain); O(gvx2_gain_config, w_gain); O(gvx2_gain_config, w_dist); O(gvx2_gain_config, reserved);
  printf("%zu ", sizeof(gvx2_gain_record));
  O(gvx2_gain_record, entry); O(gvx2_gain_record, status); O(gvx2_gain_record, n_unknown); O(gvx2_gain_record, n_free);
  O(gvx2_gain_record, n_opaque); O(gvx2_gain_record, rays_opaque); O(gvx2_gain_record, rays_off_map); O(gvx2_gain_record, rays_range);
  O(gvx2_gain_record, nearest_opaque_d2); O(gvx2_gain_record, dist); O(gvx2_gain_record, score);
  printf("%zu ", sizeof(gvx2_gain_info));
  O(gvx2_gain_info, n_candidates); O(gvx2_gain_info, n_ranked); O(gvx2_gain_info, best); O(gvx2_gain_info, best_entry);
  O(gvx2_gain_info, best_score); O(gvx2_gain_info, flags); O(gvx2_gain_info, radius);
  printf("%u %u %u %u %u %d %d %u\n", GVX2_GAIN_USE_FIELD, GVX2_GAIN_DEVICE_ENTRIES, GVX2_GAIN_INVALID, GVX2_GAIN_UNREACHABLE,
         GVX2_GAIN_BELOW_MIN, GVX2_GAIN_MAX_N, GVX2_GAIN_MAX_RADIUS, GVX2_GAIN_NO_OPAQUE);
  return 0;
}
"""

# the twin over a case written to a file by the test: what the sanitizers watch
SAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "gridvision_hip_gain.h"
int main(int argc, char **argv)
{
  if (argc != 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t hd[6];   // grid_x, grid_y, G, n, flags, have_field
  double res;
  gvx2_gain_config cfg;
  if (std::fread(hd, sizeof(hd), 1, f) != 1 || std::fread(&res, sizeof(res), 1, f) != 1 || std::fread(&cfg, sizeof(cfg), 1, f) != 1) return 4;
  const size_t G = (size_t)hd[2], n = (size_t)hd[3];
  std::vector<int8_t> occ(G);
  std::vector<uint32_t> field(hd[5] ? G : 0);
  std::vector<int32_t> entries(n);
  if (std::fread(occ.data(), 1, G, f) != G) return 5;
  if (hd[5] && std::fread(field.data(), 4, G, f) != G) return 6;
  if (std::fread(entries.data(), 4, n, f) != n) return 7;
  std::fclose(f);
  std::vector<gvx2_gain_record> out(n);
  gvx2_gain_info info;
  const int rc = gvx2_gain_host((uint8_t)hd[0], (uint8_t)hd[1], res, occ.data(), hd[5] ? field.data() : nullptr, &cfg, hd[3],
                                entries.data(), (uint32_t)hd[4], &info, out.data());
  if (rc) return 10 + rc;
  FILE *o = std::fopen(argv[2], "wb");
  if (!o) return 8;
  std::fwrite(&info, sizeof(info), 1, o);
  std::fwrite(out.data(), sizeof(gvx2_gain_record), out.size(), o);
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
    return {name: ref.gain(gc.grid_of(c["grid"]), c["occ"], c["cfg"], c["entries"], c["flags"], c["field"]) for name, c in gc.cases().items()}


def _same(got, want, tag):
    for a, b, name in zip(got, want, ("info", "records")):
        a, b = np.atleast_1d(a), np.atleast_1d(b)
        assert a.tobytes() == b.tobytes(), (tag, name, a[:4], b[:4])


# -------------------------------------------------------------------------- the fixtures and the reference alone --
@pytest.mark.parametrize("name", list(gc.cases()))
def test_fixtures_are_what_they_claim(wanted, name):
    c = gc.cases()[name]
    (gx, gy, res), (nx, ny) = gc.GRIDS[c["grid"]]
    g = gc.grid_of(c["grid"])
    assert (g.nx, g.ny) == (nx, ny) == c["occ"].shape[::-1]
    assert set(np.unique(c["occ"]).tolist()) <= {11, 50, 97, -1}               # what a planted log-odds layer can reach
    assert 1 <= c["cfg"]["radius"] <= ref.MAX_RADIUS and 1 <= len(c["entries"]) <= ref.MAX_N
    gc.check(name, c, *wanted[name])


def test_the_cases_the_feature_was_asked_to_cover():
    names = set(gc.cases())
    radii = {c["cfg"]["radius"] for c in gc.cases().values()}
    assert {1, 31, 32, 33, 100, 255, 4} <= radii
    assert {"open_unknown", "shadows", "wall_gap", "diagonal_pair", "on_opaque_and_unknown", "nan_is_opaque", "bad_entries", "duplicates",
            "n1", "n4096_r4", "min_gain_below", "min_gain_at", "min_gain_above", "w_dist_0", "w_gain_0_nearest", "score_tie",
            "all_unranked", "use_field_unreachable"} <= names
    big = gc.cases()["r255"]
    assert big["grid"] == "640x640" and len(big["entries"]) <= 4 and gc.cases()["r100_taller_than_map"]["grid"] == "130x70"


def test_known_answers_of_the_reference():
    """by hand, on an all-unknown 130 x 70 map around (65, 35)"""
    g = gc.grid_of("130x70")
    occ = np.full((70, 130), gc.UNKNOWN, np.int8)
    e = gc.ent("130x70", 65, 35)
    # R = 1: eight rays of one step; the four diagonal neighbours have d2 = 2 > 1
    info, recs = ref.gain(g, occ, ref.config(radius=1), [e])
    assert recs[0].tolist() == (e, 0, 4, 0, 0, 0, 0, 8, ref.NO_OPAQUE, 0, 4) and info.tolist() == (1, 1, 0, e, 4, 0, 1)
    # R = 2: 16 rays; the axis rays see two cells each, the diagonals and the knight rays one diagonal neighbour
    info, recs = ref.gain(g, occ, ref.config(radius=2, w_gain=3), [e])
    assert recs[0].tolist() == (e, 0, 12, 0, 0, 0, 0, 16, ref.NO_OPAQUE, 0, 36)
    assert ref.ring(2) == [(-2, -2), (-1, -2), (0, -2), (1, -2), (2, -2), (2, -1), (2, 0), (2, 1), (2, 2), (1, 2), (0, 2), (-1, 2), (-2, 2),
                           (-2, 1), (-2, 0), (-2, -1)]
    # R = 2 in the corner (0, 0): of the 16 rays only those into the quadrant x >= 0, y >= 0 stay on the map for a step:
    # ends (2, 0), (2, 1), (2, 2), (1, 2), (0, 2); the other eleven leave the map at their first cell
    info, recs = ref.gain(g, occ, ref.config(radius=2), [0])
    assert recs[0].tolist() == (0, 0, 5, 0, 0, 0, 11, 5, ref.NO_OPAQUE, 0, 5)
    # an occupied cell right of the candidate: the axis ray ends on it (d2 = 1), (67, 35) lies in its shadow
    occ[35, 66] = gc.OCC
    info, recs = ref.gain(g, occ, ref.config(radius=2), [e])
    assert recs[0].tolist() == (e, 0, 10, 0, 1, 1, 0, 15, 1, 0, 10)


# --------------------------------------------------------------------------------------- header, binding, layout --
def _declared(path, prefix):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(%s_[a-z0-9_]+)\s*\(" % prefix, txt)))


def test_header_binding_and_layout(gvamd, tmp_path):
    hdr = os.path.join(INC, "gridvision_hip_gain.h")
    assert _declared(hdr, "gvx2") == sorted(NAMES) == sorted(gvamd.GAIN_SYMBOLS)
    assert _declared(hdr, "gv") == [] and _declared(hdr, "gvx") == []
    others = gvamd.ABI_SYMBOLS + gvamd.MATCH_SYMBOLS + gvamd.SEARCH_SYMBOLS + gvamd.PATH_SYMBOLS + gvamd.FRONTIER_SYMBOLS
    assert not set(NAMES) & set(others)
    txt = open(hdr).read()
    assert '#include "gridvision_hip_frontier.h"' in txt and "owns its prefix" in txt.lower()
    for other in os.listdir(INC):                                              # included by nothing
        if other != "gridvision_hip_gain.h":
            assert "gridvision_hip_gain.h" not in open(os.path.join(INC, other)).read(), other
    from gvamd import build as b
    nm = subprocess.run(["nm", "-D", "--defined-only", b.LIB], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (gvx2_[A-Za-z0-9_]+)$", nm, flags=re.M)) == sorted(NAMES)
    assert sorted(re.findall(r" T (gvx_[A-Za-z0-9_]+)$", nm, flags=re.M)) == sorted(gvamd.FRONTIER_SYMBOLS)   # gvx_ untouched
    exported = set(re.findall(r" [A-Za-z] (gv_[A-Za-z0-9_]+)$", nm, flags=re.M))
    assert not {s for s in exported if "gain" in s}                            # no new gv_ symbol
    lib = gvamd.load()
    assert all(hasattr(lib, s) for s in NAMES) and lib.gv_abi_version() == 4
    assert hdr in b._headers()
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(LAYOUT)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + INC, src, "-o", exe])
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert C.sizeof(gvamd.GainConfig) == out[0] == 32
    assert [getattr(gvamd.GainConfig, n).offset for n, _ in gvamd.GainConfig._fields_] == out[1:9] == [0, 4, 8, 12, 16, 20, 24, 28]
    rec_off = [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40]
    assert out[9] == 48 and out[10:21] == rec_off
    info_off = [0, 4, 8, 12, 16, 24, 28]
    assert out[21] == 32 and out[22:29] == info_off
    for dt in (gvamd.GAIN_DTYPE, ref.RECORD_DTYPE):
        assert dt.itemsize == 48 and [dt.fields[n][1] for n in dt.names] == rec_off
    for dt in (gvamd.GAIN_INFO_DTYPE, ref.INFO_DTYPE):
        assert dt.itemsize == 32 and [dt.fields[n][1] for n in dt.names] == info_off
    assert gvamd.GAIN_DTYPE == ref.RECORD_DTYPE and gvamd.GAIN_INFO_DTYPE == ref.INFO_DTYPE
    consts = [gvamd.GAIN_USE_FIELD, gvamd.GAIN_DEVICE_ENTRIES, gvamd.GAIN_INVALID, gvamd.GAIN_UNREACHABLE, gvamd.GAIN_BELOW_MIN,
              gvamd.GAIN_MAX_N, gvamd.GAIN_MAX_RADIUS, gvamd.GAIN_NO_OPAQUE]
    assert out[29:37] == consts == [ref.USE_FIELD, ref.DEVICE_ENTRIES, ref.INVALID, ref.UNREACHABLE_BIT, ref.BELOW_MIN, ref.MAX_N,
                                    ref.MAX_RADIUS, ref.NO_OPAQUE]


# ------------------------------------------------------------------------------------------ twin against reference --
@pytest.mark.parametrize("name", list(gc.cases()))
def test_twin_against_reference(gvamd, wanted, name):
    c = gc.cases()[name]
    cfg = gvamd.GainConfig.of(**c["cfg"])
    geo = gc.GRIDS[c["grid"]][0]
    _same(gvamd.gain_host(*geo, c["occ"], cfg, c["entries"].astype(np.int32), c["flags"], c["field"]), wanted[name], name)
    if c["flags"]:                                                             # and without the field: dist 0, nobody unreachable
        want = ref.gain(gc.grid_of(c["grid"]), c["occ"], c["cfg"], c["entries"])
        _same(gvamd.gain_host(*geo, c["occ"], cfg, c["entries"].astype(np.int32)), want, (name, "no field"))
        assert (want[1]["dist"] == 0).all() and not (want[1]["status"] & ref.UNREACHABLE_BIT).any()


def test_twin_errors(gvamd):
    """the error table of the calls that touch no device"""
    lib = gvamd.load()
    c = gc.cases()["use_field_unreachable"]
    occ, field = c["occ"].reshape(-1), c["field"]
    ent = c["entries"].astype(np.int32)
    info, out = np.zeros(1, ref.INFO_DTYPE), np.zeros(4097, ref.RECORD_DTYPE)
    many = np.zeros(4097, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731

    def host(gx=20, gy=8, res=0.1, o=occ, fi=None, cfg=c["cfg"], n=len(ent), e=ent, flags=0, inf=info, rec=out):
        q = gvamd.GainConfig.of(**cfg) if isinstance(cfg, dict) else cfg
        return lib.gvx2_gain_host(C.c_uint8(gx), C.c_uint8(gy), C.c_double(res), p(o), p(fi), C.byref(q) if q is not None else None,
                                  C.c_int32(n), p(e), C.c_uint32(flags), p(inf), p(rec))

    assert host() == 0 and host(fi=field, flags=ref.USE_FIELD) == 0 and host(n=4096, e=many) == 0 and host(n=1) == 0
    bad = [dict(o=None), dict(cfg=None), dict(inf=None), dict(rec=None), dict(e=None), dict(flags=ref.USE_FIELD), dict(flags=ref.DEVICE_ENTRIES),
           dict(flags=4), dict(n=0), dict(n=4097, e=many), dict(n=-1), dict(gx=0), dict(gy=0), dict(res=0.0), dict(res=float("nan")),
           dict(res=-0.1)]
    bad += [dict(cfg={**ref.config(), **k}) for k in (dict(free_max=-1), dict(free_max=101), dict(free_max=40), dict(unknown_min=61),
                                                     dict(unknown_max=101), dict(unknown_min=-1), dict(radius=0), dict(radius=256),
                                                     dict(radius=-1), dict(min_gain=-1), dict(min_gain=(1 << 20) + 1), dict(w_gain=-1),
                                                     dict(w_gain=65536), dict(w_dist=-1), dict(w_dist=65536))]
    for kw in bad:
        assert host(**kw) == GV_ERR_BAD_ARG, kw
    q = gvamd.GainConfig.of(**ref.config())
    q.reserved = 1
    assert host(cfg=q) == GV_ERR_BAD_ARG
    for edge in (dict(free_max=0, unknown_min=1, unknown_max=1), dict(free_max=99, unknown_min=100, unknown_max=100), dict(min_gain=1 << 20),
                 dict(radius=1), dict(radius=255), dict(w_gain=0, w_dist=0), dict(w_gain=65535, w_dist=65535), dict(min_gain=0)):
        assert host(cfg={**ref.config(), **edge}) == 0, edge
    # the handle calls refuse a null handle before anything else
    assert lib.gvx2_set_gain_config(None, None) == GV_ERR_BAD_ARG
    for fn in (lib.gvx2_gain, lib.gvx2_gain_async):
        assert fn(None, C.c_int32(1), p(ent), C.c_uint32(0), p(info), p(out)) == GV_ERR_BAD_ARG
    for fn in (lib.gvx2_frontier_gain, lib.gvx2_frontier_gain_async):
        assert fn(None, C.c_uint32(0), p(info), p(out)) == GV_ERR_BAD_ARG
    assert lib.gvx2_device_gain(None, None, None, None) == GV_ERR_BAD_ARG
    assert lib.gvx2_nav_field_from_gain(None, C.c_int32(-1), None) == GV_ERR_BAD_ARG


# --------------------------------------------------------------------------------- plain C++, and the sanitizers --
def test_host_file_is_plain_cpp(tmp_path):
    """g++ alone compiles gv_api_gain_host.hip and gv_gain.hpp given only the public include directory"""
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + INC, "-x", "c++", "-c",
                           os.path.join(CSRC, "gv_api_gain_host.hip"), "-o", str(tmp_path / "host.o")])
    one = str(tmp_path / "hdr.cpp")
    with open(one, "w") as f:
        f.write('#include "%s"\n' % os.path.join(CSRC, "gv_gain.hpp"))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + INC, "-c", one, "-o", str(tmp_path / "hdr.o")])
    for name in ("gv_gain.hpp", "gv_api_gain_host.hip"):
        txt = open(os.path.join(CSRC, name)).read()
        assert "__HIPCC__" not in txt and "hip_runtime" not in txt and "gv_context.hpp" not in txt, name
    assert '#include "gv_gain.hpp"' in open(os.path.join(CSRC, "gv_launch_gain.hpp")).read()        # the kernels compile that text
    assert "gain_walk(" in open(os.path.join(CSRC, "gv_gain.hip")).read() and "gain_walk(" in open(os.path.join(CSRC, "gv_api_gain_host.hip")).read()


def test_twin_under_sanitizers(tmp_path, wanted):
    """the twin as a stand-alone program with its own main under AddressSanitizer and UBSan, over cases that reach the map's
    corners with a window taller than the map, the field, invalid entries and the largest n; its bytes are the reference's"""
    exe, src = str(tmp_path / "twin_san"), str(tmp_path / "main.cpp")
    with open(src, "w") as f:
        f.write(SAN_MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-I" + INC, src, "-x", "c++", os.path.join(CSRC, "gv_api_gain_host.hip"), "-o", exe])
    for name in ("r100_taller_than_map", "use_field_unreachable", "bad_entries", "n4096_r4", "r1"):
        c = gc.cases()[name]
        (gx, gy, res), (nx, ny) = gc.GRIDS[c["grid"]]
        G = nx * ny
        cfg = c["cfg"]
        inp, outp = str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))
        with open(inp, "wb") as f:
            f.write(np.array([gx, gy, G, len(c["entries"]), c["flags"], c["field"] is not None], np.int32).tobytes())
            f.write(np.float64(res).tobytes())
            f.write(np.array([cfg["free_max"], cfg["unknown_min"], cfg["unknown_max"], cfg["radius"], cfg["min_gain"], cfg["w_gain"],
                              cfg["w_dist"], 0], np.int32).tobytes())
            f.write(c["occ"].astype(np.int8).tobytes())
            if c["field"] is not None:
                f.write(np.asarray(c["field"], np.uint32).tobytes())
            f.write(c["entries"].astype(np.int32).tobytes())
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (name, r.returncode, r.stderr[-2000:])
        info, recs = wanted[name]
        assert open(outp, "rb").read() == info.tobytes() + recs.tobytes(), name
