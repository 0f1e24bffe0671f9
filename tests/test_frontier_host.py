"""[EXTENSION] X19 frontier clusters without a GPU: the header, the binding and the struct layouts; gvx_frontier_host (the
library's host twin) against frontier_ref, a plain Python flood, on every fixture of frontier_cases.py, byte for byte;
the labels against scipy.ndimage.label; the error table; the twin as a stand-alone program under AddressSanitizer and
UBSan; and the host file as plain C++.  test_fixtures_are_what_they_claim, test_field_fixture_is_what_it_claims and
test_reference_against_scipy are the only tests here that pass without the feature: they exercise the fixtures and the
reference alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frontier_cases as fc
import frontier_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grid-vision_amd", "csrc")
INC = os.path.join(ROOT, "include")
NAMES = ["gvx_set_frontier_config", "gvx_frontier_async", "gvx_frontier", "gvx_frontier_host", "gvx_get_frontier_labels",
         "gvx_device_frontier", "gvx_nav_field_from_frontier"]
GV_ERR_BAD_ARG = 1

LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "gridvision_hip_frontier.h"
#define O(t, f) printf("%zu ", offsetof(t, f))
int main(void)
{
  printf("%zu ", sizeof(gvx_frontier_config));
  O(gvx_frontier_config, free_max); O(gvx_frontier_config, unknown_min); O(gvx_frontier_config, unknown_max);
  O(gvx_frontier_config, max_cost); O(gvx_frontier_config, min_cells); O(gvx_frontier_config, flags); O(gvx_frontier_config, reserved);
  printf("%zu ", sizeof(gvx_frontier_record));
  O(gvx_frontier_record, label); O(gvx_frontier_record, n_cells); O(gvx_frontier_record, min_x); O(gvx_frontier_record, max_x);
  O(gvx_frontier_record, min_y); O(gvx_frontier_record, max_y); O(gvx_frontier_record, sum_x); O(gvx_frontier_record, sum_y);
  O(gvx_frontier_record, centre_entry); O(gvx_frontier_record, field_entry); O(gvx_frontier_record, field_min);
  O(gvx_frontier_record, goal_entry); O(gvx_frontier_record, goal_x); O(gvx_frontier_record, goal_y);
  printf("%zu ", sizeof(gvx_frontier_info));
  O(gvx_frontier_info, n_frontier_cells); O(gvx_frontier_info, n_components); O(gvx_frontier_info, n_clusters);
  O(gvx_frontier_info, n_written); O(gvx_frontier_info, best); O(gvx_frontier_info, largest); O(gvx_frontier_info, flags);
  O(gvx_frontier_info, reserved);
  printf("%u %u %d\n", GVX_FRONTIER_USE_FIELD, GVX_FRONTIER_NONE, GVX_FRONTIER_MAX_CAP);
  return 0;
}
"""

# the twin over a case written to a file by the test: what the sanitizers watch
SAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "gridvision_hip_frontier.h"
int main(int argc, char **argv)
{
  if (argc != 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t hd[8];   // grid_x, grid_y, G, cap, flags, have_cost, have_field, unused
  double res;
  gvx_frontier_config cfg;
  if (std::fread(hd, sizeof(hd), 1, f) != 1 || std::fread(&res, sizeof(res), 1, f) != 1 || std::fread(&cfg, sizeof(cfg), 1, f) != 1) return 4;
  const size_t G = (size_t)hd[2];
  std::vector<int8_t> occ(G);
  std::vector<uint8_t> cost(hd[5] ? G : 0);
  std::vector<uint32_t> field(hd[6] ? G : 0), labels(G);
  if (std::fread(occ.data(), 1, G, f) != G) return 5;
  if (hd[5] && std::fread(cost.data(), 1, G, f) != G) return 6;
  if (hd[6] && std::fread(field.data(), 4, G, f) != G) return 7;
  std::fclose(f);
  std::vector<gvx_frontier_record> out((size_t)hd[3]);
  gvx_frontier_info info;
  const int rc = gvx_frontier_host((uint8_t)hd[0], (uint8_t)hd[1], res, occ.data(), hd[5] ? cost.data() : nullptr,
                                   hd[6] ? field.data() : nullptr, &cfg, hd[3], (uint32_t)hd[4], &info, out.data(), labels.data());
  if (rc) return 10 + rc;
  FILE *o = std::fopen(argv[2], "wb");
  if (!o) return 8;
  std::fwrite(&info, sizeof(info), 1, o);
  std::fwrite(out.data(), sizeof(gvx_frontier_record), out.size(), o);
  std::fwrite(labels.data(), 4, G, o);
  std::fclose(o);
  return 0;
}
"""


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


def _want(c, cap, flags=0):
    return ref.frontier(fc.grid_of(c["grid"]), c["occ"], c["cfg"], cap, flags, c["cost"], c["field"] if flags else None)


def _same(got, want, tag):
    for a, b, name in zip(got, want, ("info", "records", "labels")):
        a, b = np.atleast_1d(a), np.atleast_1d(b)
        assert a.tobytes() == b.tobytes(), (tag, name, a[:4], b[:4])


# -------------------------------------------------------------------------- the fixtures and the reference alone --
@pytest.mark.parametrize("name", list(fc.cases()))
def test_fixtures_are_what_they_claim(name):
    c = fc.cases()[name]
    (gx, gy, res), (nx, ny) = fc.GRIDS[c["grid"]]
    g = fc.grid_of(c["grid"])
    assert (g.nx, g.ny) == (nx, ny) == c["occ"].shape[::-1]
    assert set(np.unique(c["occ"]).tolist()) <= set(range(11, 98)) | {-1}      # what a planted log-odds layer can reach
    fc.check(name, c, *_want(c, c["caps"][0]))


def test_field_fixture_is_what_it_claims():
    c = fc.cases()["field"]
    nx = fc.GRIDS[c["grid"]][1][0]
    info, recs, labels = _want(c, 8, ref.USE_FIELD)
    assert recs["n_cells"][:4].tolist() == [70, 30, 40, 40]
    assert int(recs[0]["field_min"]) == 5 and int(recs[0]["field_entry"]) == 10 * nx + 54          # the tie: the smaller entry
    assert int(recs[1]["field_entry"]) == -1 and int(recs[1]["goal_entry"]) == int(recs[1]["centre_entry"])
    assert int(recs[1]["field_min"]) == ref.UNREACHABLE and int(recs[0]["goal_entry"]) == int(recs[0]["field_entry"])
    assert int(recs[2]["field_min"]) == int(recs[3]["field_min"]) == 3 and int(info["best"]) == 2    # best: a tie, the smaller index
    plain = _want(c, 8)
    assert int(plain[0]["best"]) == 0 and (plain[1]["field_entry"][:4] == -1).all()
    assert int(_want(c, 3, ref.USE_FIELD)[0]["best"]) == 2 and int(_want(c, 2, ref.USE_FIELD)[0]["best"]) == 0
    tie = dict(c, occ=np.where(np.arange(80)[:, None] < 20, fc.OCC, c["occ"]).astype(np.int8))       # without run 0: 30, 40, 40
    assert _want(tie, 8)[1]["n_cells"][:3].tolist() == [30, 40, 40] and int(_want(tie, 8)[0]["best"]) == 1


@pytest.mark.parametrize("name", list(fc.cases()))
def test_reference_against_scipy(name):
    """the reference's components are scipy.ndimage.label's with the 8-connected structure, each named by its smallest entry"""
    from scipy import ndimage
    c = fc.cases()[name]
    _, _, labels = _want(c, c["caps"][0])
    mask = ref.frontier_mask(c["occ"], c["cfg"], c["cost"])
    lab, n = ndimage.label(mask, structure=np.ones((3, 3), int))
    flat = lab.reshape(-1)
    first = np.full(n + 1, -1, np.int64)
    idx = np.flatnonzero(flat)
    first[flat[idx][::-1]] = idx[::-1]                     # the smallest entry of every scipy label
    want = np.where(flat > 0, first[flat], ref.NONE).astype(np.uint32)
    assert labels.tobytes() == want.tobytes()


# --------------------------------------------------------------------------------------- header, binding, layout --
def _declared(path, prefix):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(%s_[a-z0-9_]+)\s*\(" % prefix, txt)))


def test_header_binding_and_layout(gvamd, tmp_path):
    hdr = os.path.join(INC, "gridvision_hip_frontier.h")
    assert _declared(hdr, "gvx") == sorted(NAMES) == sorted(gvamd.FRONTIER_SYMBOLS) and _declared(hdr, "gv") == []
    assert not set(NAMES) & set(gvamd.ABI_SYMBOLS + gvamd.MATCH_SYMBOLS + gvamd.SEARCH_SYMBOLS + gvamd.PATH_SYMBOLS)
    txt = open(hdr).read()
    assert '#include "gridvision_hip.h"' in txt and "gridvision_hip_frontier.h" not in open(os.path.join(INC, "gridvision_hip.h")).read()
    from gvamd import build as b
    nm = subprocess.run(["nm", "-D", "--defined-only", b.LIB], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (gvx_[A-Za-z0-9_]+)$", nm, flags=re.M)) == sorted(NAMES)
    exported = set(re.findall(r" [A-Za-z] (gv_[A-Za-z0-9_]+)$", nm, flags=re.M))
    assert not {s for s in exported if "frontier" in s}                        # no new gv_ symbol
    lib = gvamd.load()
    assert all(hasattr(lib, s) for s in NAMES) and lib.gv_abi_version() == 4
    assert hdr in b._headers()
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(LAYOUT)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + INC, src, "-o", exe])
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert C.sizeof(gvamd.FrontierConfig) == out[0] == 32
    assert [getattr(gvamd.FrontierConfig, n).offset for n, _ in gvamd.FrontierConfig._fields_] == out[1:8] == [0, 4, 8, 12, 16, 20, 24]
    rec_off = [0, 4, 8, 12, 16, 20, 24, 32, 40, 44, 48, 52, 56, 60]
    assert out[8] == 64 and out[9:23] == rec_off
    assert out[23] == 32 and out[24:32] == [0, 4, 8, 12, 16, 20, 24, 28]
    for dt in (gvamd.FRONTIER_DTYPE, ref.RECORD_DTYPE):
        assert dt.itemsize == 64 and [dt.fields[n][1] for n in dt.names] == rec_off
    for dt in (gvamd.FRONTIER_INFO_DTYPE, ref.INFO_DTYPE):
        assert dt.itemsize == 32 and [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert gvamd.FRONTIER_DTYPE == ref.RECORD_DTYPE and gvamd.FRONTIER_INFO_DTYPE == ref.INFO_DTYPE
    assert out[32:] == [gvamd.FRONTIER_USE_FIELD, gvamd.FRONTIER_NONE, gvamd.FRONTIER_MAX_CAP] == [ref.USE_FIELD, ref.NONE, ref.MAX_CAP]


# ------------------------------------------------------------------------------------------ twin against reference --
@pytest.mark.parametrize("name", list(fc.cases()))
def test_twin_against_reference(gvamd, name):
    c = fc.cases()[name]
    cfg = gvamd.FrontierConfig.of(**c["cfg"])
    geo = fc.GRIDS[c["grid"]][0]
    for cap in c["caps"]:
        for flags in ((0, ref.USE_FIELD) if c["field"] is not None else (0,)):
            got = gvamd.frontier_host(*geo, c["occ"], cfg, cap, flags, c["cost"], c["field"] if flags else None)
            _same(got, _want(c, cap, flags), (name, cap, flags))
    info, recs, none = gvamd.frontier_host(*geo, c["occ"], cfg, c["caps"][0], 0, c["cost"], keep_labels=False)
    assert none is None and info.tobytes() == _want(c, c["caps"][0])[0].tobytes()


def test_twin_errors(gvamd):
    """the error table of the calls that touch no device"""
    lib = gvamd.load()
    c = fc.cases()["cost_gate_1"]
    occ, cost = c["occ"].reshape(-1), c["cost"]
    field = np.zeros(occ.size, np.uint32)
    info, out = np.zeros(1, ref.INFO_DTYPE), np.zeros(4097, ref.RECORD_DTYPE)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731

    def host(gx=20, gy=8, res=0.1, o=occ, co=cost, fi=None, cfg=c["cfg"], cap=8, flags=0, inf=info, rec=out):
        q = gvamd.FrontierConfig.of(**cfg) if isinstance(cfg, dict) else cfg
        return lib.gvx_frontier_host(C.c_uint8(gx), C.c_uint8(gy), C.c_double(res), p(o), p(co), p(fi), C.byref(q) if q is not None else None,
                                     C.c_int32(cap), C.c_uint32(flags), p(inf), p(rec), None)

    assert host() == 0 and host(rec=None) == 0 and host(fi=field, flags=ref.USE_FIELD) == 0
    assert host(co=None, cfg=ref.config()) == 0                                          # max_cost 256: no costmap
    bad = [dict(o=None), dict(cfg=None), dict(inf=None), dict(co=None), dict(flags=ref.USE_FIELD), dict(flags=2), dict(cap=0),
           dict(cap=4097), dict(cap=-1), dict(gx=0), dict(gy=0), dict(res=0.0), dict(res=float("nan")), dict(res=-0.1)]
    bad += [dict(cfg={**ref.config(), **k}) for k in (dict(free_max=-1), dict(free_max=101), dict(free_max=40), dict(unknown_min=61),
                                                     dict(unknown_max=101), dict(unknown_min=-1), dict(max_cost=0), dict(max_cost=257),
                                                     dict(min_cells=0), dict(min_cells=(1 << 20) + 1))]
    for kw in bad:
        assert host(**kw) == GV_ERR_BAD_ARG, kw
    q = gvamd.FrontierConfig.of(**ref.config())
    q.flags = 1
    assert host(cfg=q) == GV_ERR_BAD_ARG
    q.flags, q.reserved[0] = 0, 7
    assert host(cfg=q) == GV_ERR_BAD_ARG
    for edge in (dict(free_max=0, unknown_min=1, unknown_max=1), dict(free_max=99, unknown_min=100, unknown_max=100), dict(min_cells=1 << 20),
                 dict(max_cost=1)):
        assert host(cfg={**ref.config(), **edge}) == 0, edge
    # the handle calls refuse a null handle before anything else
    assert lib.gvx_set_frontier_config(None, None) == GV_ERR_BAD_ARG
    assert lib.gvx_frontier(None, C.c_int32(8), C.c_uint32(0), p(info), p(out)) == GV_ERR_BAD_ARG
    assert lib.gvx_frontier_async(None, C.c_int32(8), C.c_uint32(0), p(info), p(out)) == GV_ERR_BAD_ARG
    assert lib.gvx_get_frontier_labels(None, p(field)) == GV_ERR_BAD_ARG
    assert lib.gvx_device_frontier(None, None, None, None, None) == GV_ERR_BAD_ARG
    assert lib.gvx_nav_field_from_frontier(None, C.c_int32(-1), None) == GV_ERR_BAD_ARG


# --------------------------------------------------------------------------------- plain C++, and the sanitizers --
def test_host_file_is_plain_cpp(tmp_path):
    """g++ alone compiles gv_api_frontier_host.hip and gv_frontier.hpp given only the public include directory"""
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + INC, "-x", "c++", "-c",
                           os.path.join(CSRC, "gv_api_frontier_host.hip"), "-o", str(tmp_path / "host.o")])
    one = str(tmp_path / "hdr.cpp")
    with open(one, "w") as f:
        f.write('#include "%s"\n' % os.path.join(CSRC, "gv_frontier.hpp"))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + INC, "-c", one, "-o", str(tmp_path / "hdr.o")])
    for name in ("gv_frontier.hpp", "gv_api_frontier_host.hip"):
        txt = open(os.path.join(CSRC, name)).read()
        assert "__HIPCC__" not in txt and "hip_runtime" not in txt and "gv_context.hpp" not in txt, name


def test_twin_under_sanitizers(tmp_path):
    """the twin as a stand-alone program with its own main under AddressSanitizer and UBSan, over cases that reach the map's
    corners, the costmap, the field and the largest cap; its bytes are the reference's"""
    exe, src = str(tmp_path / "twin_san"), str(tmp_path / "main.cpp")
    with open(src, "w") as f:
        f.write(SAN_MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-I" + INC, src, "-x", "c++", os.path.join(CSRC, "gv_api_frontier_host.hip"), "-o", exe])
    for name, cap, flags in (("no_wrap", 64, 0), ("checkerboard", 1, 0), ("isolated_dots", 4096, 0), ("cost_gate_1", 8, 0),
                             ("field", 3, ref.USE_FIELD), ("class_edges", 64, 0), ("none_all_unknown", 5, 0)):
        c = fc.cases()[name]
        (gx, gy, res), (nx, ny) = fc.GRIDS[c["grid"]]
        G = nx * ny
        field = c["field"] if flags else None
        inp, outp = str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))
        with open(inp, "wb") as f:
            f.write(np.array([gx, gy, G, cap, flags, c["cost"] is not None, field is not None, 0], np.int32).tobytes())
            f.write(np.float64(res).tobytes())
            f.write(bytes(ref_config_bytes(c["cfg"])))
            f.write(c["occ"].astype(np.int8).tobytes())
            if c["cost"] is not None:
                f.write(np.asarray(c["cost"], np.uint8).tobytes())
            if field is not None:
                f.write(np.asarray(field, np.uint32).tobytes())
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (name, r.returncode, r.stderr[-2000:])
        raw = open(outp, "rb").read()
        info, recs, labels = _want(c, cap, flags)
        assert raw == info.tobytes() + recs.tobytes() + labels.tobytes(), name


def ref_config_bytes(cfg):
    return np.array([cfg["free_max"], cfg["unknown_min"], cfg["unknown_max"], cfg["max_cost"], cfg["min_cells"], 0, 0, 0], np.int32).tobytes()
