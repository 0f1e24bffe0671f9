"""[EXTENSION] X16 scan-to-costmap matching, host side (no GPU): the new header, the binding and the struct layouts; the
rotation table against math.cos / math.sin; match_ref's own known answers on the families that state one; every
family reaching the edge it names; the library's host twin (gv_match_scan_host: the kernels' arithmetic text compiled
for the host) against match_ref on every family, record and volume byte for byte; the argument errors of the host-only
functions.

test_reference_known_answers and test_the_families_are_what_they_claim exercise match_ref and the fixtures alone: they
are the reference's self-check and call nothing of the library, so they alone of this file would pass on a tree without
the feature; every other test here needs the new symbols."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import match_cases as mc
import match_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GV_ERR_BAD_ARG = 1

LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "gridvision_hip_match.h"
#define O(t, f) printf("%zu ", offsetof(t, f))
int main(void)
{
  printf("%zu ", sizeof(gv_match_config));
  O(gv_match_config, wx); O(gv_match_config, wy); O(gv_match_config, wt); O(gv_match_config, stride);
  O(gv_match_config, yaw_step); O(gv_match_config, min_points); O(gv_match_config, flags);
  printf("%zu ", sizeof(gv_match_guess));
  O(gv_match_guess, x); O(gv_match_guess, y); O(gv_match_guess, yaw);
  printf("%zu ", sizeof(gv_match_result));
  O(gv_match_result, best_t); O(gv_match_result, best_j); O(gv_match_result, best_i); O(gv_match_result, valid);
  O(gv_match_result, n_used); O(gv_match_result, best_score); O(gv_match_result, guess_score); O(gv_match_result, reserved);
  O(gv_match_result, x); O(gv_match_result, y); O(gv_match_result, yaw); O(gv_match_result, reserved2);
  printf("%d %d\n", (int)GV_MATCH_USE_BAND, (int)GV_MATCH_KEEP_SCORES);
  return 0;
}
"""

NAMES = ["gv_set_match_config", "gv_match_scan_async", "gv_match_scan", "gv_match_scan_host", "gv_match_rotations", "gv_match_motion"]


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


def lib_cfg(gvamd, c):
    return gvamd.MatchConfig(c.wx, c.wy, c.wt, c.stride, c.yaw_step, c.min_points, c.flags)


def _declared(path):
    txt = open(path).read()
    return sorted(set(re.findall(r"\b(gv_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))))


def test_header_binding_and_layout(gvamd, tmp_path):
    inc = os.path.join(ROOT, "include")
    assert _declared(os.path.join(inc, "gridvision_hip_match.h")) == sorted(NAMES) == sorted(gvamd.MATCH_SYMBOLS)
    main = _declared(os.path.join(inc, "gridvision_hip.h"))
    assert main == sorted(gvamd.ABI_SYMBOLS) and len(main) == 123 and not set(main) & set(NAMES)
    assert "gridvision_hip_match.h" in open(os.path.join(inc, "gridvision_hip.h")).read()
    lib = gvamd.load()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.gv_abi_version() == 4
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "123 entry points" in readme and "gridvision_hip_match.h" in readme
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(LAYOUT)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + inc, src, "-o", exe])
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert C.sizeof(gvamd.MatchConfig) == out[0] == 32
    assert [getattr(gvamd.MatchConfig, n).offset for n, _ in gvamd.MatchConfig._fields_] == out[1:8] == [0, 4, 8, 12, 16, 24, 28]
    assert [n for n, _ in gvamd.MatchConfig._fields_] == ["wx", "wy", "wt", "stride", "yaw_step", "min_points", "flags"]
    assert C.sizeof(gvamd.MatchGuess) == out[8] == 24 and out[9:12] == [0, 8, 16]
    for dt in (gvamd.MATCH_RESULT_DTYPE, ref.RESULT_DTYPE):
        assert dt.itemsize == out[12] == 64
        assert [dt.fields[n][1] for n in dt.names] == out[13:25] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56]
        assert dt.names == ("best_t", "best_j", "best_i", "valid", "n_used", "best_score", "guess_score", "reserved", "x", "y",
                            "yaw", "reserved2")
    assert out[25:] == [gvamd.MATCH_USE_BAND, gvamd.MATCH_KEEP_SCORES] == [ref.USE_BAND, ref.KEEP_SCORES] == [1, 1]
    assert f"#define GV_MATCH_CHUNK {mc.CHUNK}\n" in open(os.path.join(ROOT, "grid-vision_amd", "csrc", "gv_match.hpp")).read()


@pytest.mark.parametrize("wt,step,yaw", [(0, 0.0, 0.3), (3, 0.02, 0.1), (32, 0.01, -2.5), (32, 0.0981747704, 1000.25), (5, 1e-12, 3.0)])
def test_rotations_are_libm_rounded_once(gvamd, wt, step, yaw):
    cfg = gvamd.MatchConfig.of(wx=1, wy=1, wt=wt, yaw_step=step)
    got = gvamd.match_rotations(cfg, (0.5, -0.25, yaw))
    want = np.array([[np.float32(math.cos(yaw + float(t - wt) * step)), np.float32(math.sin(yaw + float(t - wt) * step))]
                     for t in range(2 * wt + 1)], np.float32)
    assert got.shape == (2 * wt + 1, 2) and got.tobytes() == want.tobytes()
    assert got.tobytes() == ref.rotations(ref.Cfg(1, 1, wt, step), (0.5, -0.25, yaw)).tobytes()


def test_reference_known_answers():
    """families A, C and E: match_ref alone gives what the fixtures state"""
    for c in mc.family_a():
        r, vol = mc.want(c)
        assert (int(r["best_t"][0]), int(r["best_j"][0]), int(r["best_i"][0])) == c["best"], c["name"]
        assert int(r["n_used"][0]) == c["n_used"] and int(r["best_score"][0]) == c["n_used"] * 254 and int(r["valid"][0]) == 1
        assert (vol == vol.max()).sum() == 1, c["name"]
        geo = mc.geo_of(c["grid"])
        t, j, i = c["best"]
        assert r["x"][0] == c["guess"][0] - float(i) * geo.res and r["y"][0] == c["guess"][1] - float(j) * geo.res
        assert r["yaw"][0] == c["guess"][2] + float(t) * c["cfg"].yaw_step
    c = mc.by_name("c_borders")
    r, vol = mc.want(c)
    assert int(r["n_used"][0]) == c["n_used"] == len(c["x"]) - 3
    geo = mc.geo_of("small")
    bx, by = ref.used_points(mc.m_base(c["tf"]), c["x"], c["y"], c["z"], c["cfg"], None)
    ux, uy, ok = ref.cells(geo, c["guess"], np.float32(1.0), np.float32(0.0), bx, by)
    assert (~ok).sum() == c["n_far"]
    got = list(zip(ux[ok].tolist(), uy[ok].tolist()))
    assert got[:len(mc.C_EDGE_CELLS) + len(mc.C_OFF_CELLS)] == mc.C_EDGE_CELLS + mc.C_OFF_CELLS
    # x = 2.5, 3.5 (the map's end: cell 0), -1.5 (the other end: cell nx, off the map), y = 1.5 and -1.5 likewise
    assert got[-6:] == [(10, 15), (0, 15), (50, 15), (25, 0), (25, 30), (10, 10)]
    for c in mc.family_e():
        r, _ = mc.want(c)
        if "n_used" in c:
            assert int(r["n_used"][0]) == c["n_used"], c["name"]
    c = mc.by_name("e_band_on")
    m = mc.m_base(c["tf"])
    bz = ref.base_points(m, c["x"], c["y"], c["z"])[2][:6]
    zg, zm = np.float32(mc.BAND[0]), np.float32(mc.BAND[1])
    assert bz.tolist() == [zg, np.nextafter(zg, np.float32(-1)), np.nextafter(zg, np.float32(9)), zm, np.nextafter(zm, np.float32(-1)),
                           np.nextafter(zm, np.float32(9))]
    assert (~(bz < zg) & ~(bz > zm)).tolist() == c["edge_used"]
    n_on, n_off = int(mc.want(c)[0]["n_used"][0]), int(mc.want(mc.by_name("e_band_off"))[0]["n_used"][0])
    bz_all = ref.base_points(m, c["x"], c["y"], c["z"])[2]
    assert n_off == 2500 and n_on == int((~(bz_all < zg) & ~(bz_all > zm)).sum()) and 700 < n_on < 1200
    assert int(mc.want(mc.by_name("e_stride_1024"))[0]["n_used"][0]) == 3


def test_the_families_are_what_they_claim():
    assert {n[0] for n in mc.names()} == set("abcdef")
    for c in mc.family_b():
        r, vol = mc.want(c)
        assert (int(r["best_t"][0]), int(r["best_j"][0]), int(r["best_i"][0])) == c["best"], c["name"]
        assert int(r["valid"][0]) == c["valid"], c["name"]
        if c["name"] == "b_zero":
            assert not vol.any()
        elif "flat" in c:
            assert (vol == c["flat"]).all()
        else:
            assert (vol == vol.max()).sum() >= 2 and vol.max() == 3 * 254, c["name"]   # a tie the rules have to break
    c = mc.by_name("b_nearer")
    vol = mc.want(c)[1]
    assert vol[0, 3, 3 + 1] == vol[0, 3, 3 - 3] == vol.max()          # the farther maximum has the lower linear index
    c = mc.by_name("c_borders")
    vol = mc.want(c)[1]
    assert len({vol[t].tobytes() for t in range(3)}) == 3             # the yaw candidates move points across cells
    for c in mc.family_d():
        r, vol = mc.want(c)
        assert vol.shape == (2 * c["cfg"].wt + 1, 2 * c["cfg"].wy + 1, 2 * c["cfg"].wx + 1)
        if "best" in c:
            assert (int(r["best_t"][0]), int(r["best_j"][0]), int(r["best_i"][0])) == c["best"], c["name"]
        if "full" in c:
            assert vol.shape == (1, 1, 1) and int(vol[0, 0, 0]) == c["full"] == int(r["guess_score"][0])
        if c.get("same_yaws"):
            # every yaw ties: the Chebyshev rule cannot tell those within the best shift's distance apart, the index does
            reach = max(abs(int(r["best_j"][0])), abs(int(r["best_i"][0])))
            assert all(vol[t].tobytes() == vol[0].tobytes() for t in range(vol.shape[0])) and vol.any()
            assert int(r["best_t"][0]) == -min(c["cfg"].wt, reach)
    vol = mc.want(mc.by_name("d_full"))[1]
    assert vol.size == 65 ** 3 == 274625 and len(np.unique(vol)) > 1000
    # d_full has points whose window lies on the map whole, across its border and off it: every path of the score pass
    c = mc.by_name("d_full")
    geo = mc.geo_of("big")
    bx, by = ref.used_points(mc.m_base(c["tf"]), c["x"], c["y"], c["z"], c["cfg"], None)
    ux, uy, ok = ref.cells(geo, c["guess"], *ref.rotations(c["cfg"], c["guess"])[32], bx, by)
    whole = (ux - 32 >= 0) & (ux + 32 < geo.nx) & (uy - 32 >= 0) & (uy + 32 < geo.ny)
    assert ok.all() and 20 < whole.sum() < 280
    for c in mc.family_f():
        r, vol = mc.want(c)
        assert int(r["n_used"][0]) == c["n_used"], c["name"]
        if "valid" in c:
            assert int(r["valid"][0]) == c["valid"] and int(r["best_score"][0]) > 0, c["name"]
    assert {c["n_used"] for c in mc.family_f()} >= {0, 1, 63, 64, 65, mc.CHUNK - 1, mc.CHUNK, mc.CHUNK + 1, 10000}
    r, vol = mc.want(mc.by_name("f_n0"))
    assert not vol.any() and int(r["valid"][0]) == 0 and (int(r["best_t"][0]), int(r["best_j"][0]), int(r["best_i"][0])) == (0, 0, 0)
    c = mc.by_name("f_one_cell")
    bx, by = ref.used_points(mc.m_base(c["tf"]), c["x"], c["y"], c["z"], c["cfg"], None)
    ux, uy, ok = ref.cells(geo, c["guess"], *ref.rotations(c["cfg"], c["guess"])[1], bx, by)
    assert ok.all() and set(zip(ux.tolist(), uy.tolist())) == {c["one_cell"]}
    assert int(mc.want(c)[1][1, 2, 2]) % 10000 == 0 and int(mc.want(c)[1][1, 2, 2]) > 0


@pytest.mark.parametrize("name", mc.names())
def test_host_twin_equals_reference(gvamd, name):
    c = mc.by_name(name)
    geo = mc.geo_of(c["grid"])
    cost = mc.cost_of(c["mask"], c["inflation"], geo.res)
    want_r, want_v = mc.want(c)
    got_r, got_v = gvamd.match_scan_host(*mc.GRIDS[c["grid"]], cost, c["x"], c["y"], c["z"], c["tf"], lib_cfg(gvamd, c["cfg"]),
                                         c["guess"], band=c["band"], keep_scores=True)
    assert got_v.dtype == np.uint32 and got_v.shape == want_v.shape
    bad = np.flatnonzero(got_v.reshape(-1) != want_v.reshape(-1))
    assert got_v.tobytes() == want_v.tobytes(), (name, len(bad), bad[:4], got_v.reshape(-1)[bad[:4]], want_v.reshape(-1)[bad[:4]])
    assert np.asarray(got_r).tobytes() == want_r.tobytes(), (name, got_r, want_r)
    only = gvamd.match_scan_host(*mc.GRIDS[c["grid"]], cost, c["x"], c["y"], c["z"], c["tf"], lib_cfg(gvamd, c["cfg"]), c["guess"],
                                 band=c["band"])
    assert np.asarray(only).tobytes() == want_r.tobytes()


def test_motion_of_a_result(gvamd):
    for name in ("a_big_+3-2+2", "a_small_-3+2+2", "b_zero"):
        r = mc.want(mc.by_name(name))[0]
        m = gvamd.match_motion(r)
        got = np.array([m.qx, m.qy, m.qz, m.qw, m.tx, m.ty, m.tz], np.float64)
        assert got.tobytes() == np.array(ref.motion(r[0]), np.float64).tobytes(), name
    lib = gvamd.load()
    r = mc.want(mc.by_name("b_zero"))[0].copy()
    out = gvamd.Transform()
    assert lib.gv_match_motion(None, C.byref(out)) == GV_ERR_BAD_ARG
    assert lib.gv_match_motion(r.ctypes.data_as(C.c_void_p), None) == GV_ERR_BAD_ARG
    r["yaw"] = np.nan
    assert lib.gv_match_motion(r.ctypes.data_as(C.c_void_p), C.byref(out)) == GV_ERR_BAD_ARG


BAD_CONFIGS = [dict(wx=-1), dict(wx=33), dict(wy=-1), dict(wy=33), dict(wt=-1), dict(wt=33), dict(yaw_step=float("nan")),
               dict(yaw_step=float("inf")), dict(yaw_step=-0.01), dict(wt=1, yaw_step=0.0), dict(stride=0), dict(stride=1025),
               dict(min_points=0), dict(flags=2)]


def test_error_table(gvamd):
    lib = gvamd.load()
    c = mc.by_name("b_mirror_i")
    geo = mc.geo_of(c["grid"])
    cost = mc.cost_of(c["mask"], c["inflation"], geo.res)
    good = lib_cfg(gvamd, c["cfg"])
    args = lambda cfg, guess=c["guess"], band=None: (*mc.GRIDS[c["grid"]], cost, c["x"], c["y"], c["z"], c["tf"], cfg, guess)   # noqa: E731
    gvamd.match_scan_host(*args(good))
    gvamd.match_scan_host(*args(gvamd.MatchConfig.of(wx=32, wy=32, wt=0, yaw_step=0.0, stride=1024, min_points=2 ** 31 - 1, use_band=True)))
    for kw in BAD_CONFIGS:
        base = dict(wx=2, wy=2, wt=1, yaw_step=0.01, stride=1, min_points=1, flags=0)
        base.update(kw)
        cfg = gvamd.MatchConfig.of(**base)
        with pytest.raises(gvamd.GVError) as e:
            gvamd.match_scan_host(*args(cfg))
        assert e.value.code == GV_ERR_BAD_ARG, kw
        with pytest.raises(gvamd.GVError) as e:
            gvamd.match_rotations(cfg, c["guess"])
        assert e.value.code == GV_ERR_BAD_ARG, kw
    for k in range(3):
        for v in (float("nan"), float("inf"), float("-inf")):
            guess = list(c["guess"])
            guess[k] = v
            with pytest.raises(gvamd.GVError) as e:
                gvamd.match_scan_host(*args(good, guess))
            assert e.value.code == GV_ERR_BAD_ARG
            with pytest.raises(gvamd.GVError):
                gvamd.match_rotations(good, guess)
    with pytest.raises(gvamd.GVError):
        gvamd.match_scan_host(0, 3, 0.1, *args(good)[3:])                        # a geometry gv_create rejects
    with pytest.raises(gvamd.GVError):
        gvamd.match_scan_host(*args(good), band=(2.0, 1.0))                      # a band gv_set_height_band rejects
    # the raw call: null pointers, unknown flags, GV_MATCH_KEEP_SCORES without a destination
    x, y, z = c["x"], c["y"], c["z"]
    tf, q = gvamd.make_tf(c["tf"]), gvamd.MatchGuess(*c["guess"])
    res = np.zeros(1, gvamd.MATCH_RESULT_DTYPE)
    vol = np.zeros(good.shape, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                   # noqa: E731

    def call(cost_=p(cost), x_=p(x), y_=p(y), z_=p(z), n=len(x), tf_=C.byref(tf), cfg_=C.byref(good), q_=C.byref(q), flags=0,
             res_=p(res), vol_=None):
        return lib.gv_match_scan_host(C.c_uint8(5), C.c_uint8(3), C.c_double(0.1), cost_, x_, y_, z_, C.c_size_t(n), tf_, None, cfg_,
                                      q_, C.c_uint32(flags), res_, vol_)

    assert call() == 0 and call(flags=1, vol_=p(vol)) == 0 and call(n=0, x_=None, y_=None, z_=None) == 0
    before = res.tobytes()
    for kw in (dict(cost_=None), dict(x_=None), dict(y_=None), dict(z_=None), dict(tf_=None), dict(cfg_=None), dict(q_=None),
               dict(res_=None), dict(flags=2), dict(flags=3, vol_=p(vol)), dict(flags=1)):
        assert call(**kw) == GV_ERR_BAD_ARG, kw
    assert res.tobytes() == before
    assert lib.gv_match_rotations(None, C.byref(q), p(np.zeros(130, np.float32))) == GV_ERR_BAD_ARG
    assert lib.gv_match_rotations(C.byref(good), None, p(np.zeros(130, np.float32))) == GV_ERR_BAD_ARG
    assert lib.gv_match_rotations(C.byref(good), C.byref(q), None) == GV_ERR_BAD_ARG


SANITIZED_MAIN = r"""
// gv_match_scan_host with GV_MATCH_KEEP_SCORES under AddressSanitizer and UBSan: reads one scene and a list of
// configurations from the file the test wrote, prints the 64 bytes of every record and its volume in hex
#include <cstdio>
#include <cstring>
#include <vector>
#include "gridvision_hip_match.h"
int main(int argc, char **argv)
{
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t head[5];
  double real[11];
  float zs[2];
  if (std::fread(head, sizeof(head), 1, f) != 1 || std::fread(real, sizeof(real), 1, f) != 1 || std::fread(zs, sizeof(zs), 1, f) != 1) return 2;
  const int32_t n = head[2], n_cfg = head[3];
  const int nx = (int)(head[0] / real[0] + 0.5), ny = (int)(head[1] / real[0] + 0.5);
  std::vector<uint8_t> cost((size_t)nx * ny);                // exactly the bytes the call may read
  std::vector<float> x((size_t)n), y((size_t)n), z((size_t)n);
  std::vector<gv_match_config> cfg((size_t)n_cfg);
  if (std::fread(cost.data(), 1, cost.size(), f) != cost.size()) return 2;
  for (auto *v : {&x, &y, &z})
    if (n && std::fread(v->data(), sizeof(float), (size_t)n, f) != (size_t)n) return 2;
  if (std::fread(cfg.data(), sizeof(gv_match_config), (size_t)n_cfg, f) != (size_t)n_cfg) return 2;
  std::fclose(f);
  const gv_transform tf{real[1], real[2], real[3], real[4], real[5], real[6], real[7]};
  const gv_match_guess q{real[8], real[9], real[10]};
  gv_height_band band;
  std::memset(&band, 0, sizeof(band));
  band.z_ground = zs[0];
  band.z_max = zs[1];
  for (const gv_match_config &c : cfg) {
    gv_match_result r;
    std::memset(&r, 0xAB, sizeof(r));
    std::vector<uint32_t> vol((size_t)(2 * c.wt + 1) * (size_t)(2 * c.wy + 1) * (size_t)(2 * c.wx + 1), 0xABABABABu);   // exactly the volume
    const int rc = gv_match_scan_host((uint8_t)head[0], (uint8_t)head[1], real[0], cost.data(), x.data(), y.data(), z.data(), (size_t)n,
                                      &tf, head[4] ? &band : nullptr, &c, &q, GV_MATCH_KEEP_SCORES, &r, vol.data());
    if (rc) { std::printf("rc %d\n", rc); return 3; }
    const unsigned char *b = (const unsigned char *)&r, *d = (const unsigned char *)vol.data();
    for (size_t i = 0; i < sizeof(r); ++i) std::printf("%02x", b[i]);
    for (size_t i = 0; i < vol.size() * sizeof(uint32_t); ++i) std::printf("%02x", d[i]);
    std::printf("\n");
  }
  return 0;
}
"""


def test_host_twin_under_sanitizers(gvamd, tmp_path):
    """gv_api_match_host.hip's gv_match_scan_host compiled by g++ with -fsanitize=address,undefined into a stand-alone
    program with its own main (nothing is loaded into Python), the costmap and the volume in heap blocks of exactly their
    sizes: every case of family c (the edge and off-map cells of the 50 x 30 grid) and one case each of families a and e
    under their own configurations (held to match_ref, record and volume), and over family c's scene the widest windows
    along each axis, 65 x 65 x 1, 1 x 1 x 65 and 65 x 1 x 3 (held to the library's twin through the binding)"""
    src, exe = str(tmp_path / "san.cpp"), str(tmp_path / "san")
    with open(src, "w") as f:
        f.write(SANITIZED_MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), src, "-x", "c++",
                           os.path.join(ROOT, "grid-vision_amd", "csrc", "gv_api_match_host.hip"), "-o", exe])
    wide = ((32, 32, 0), (0, 0, 32), (32, 0, 1))
    runs = [(c, [c["cfg"]] + [c["cfg"]._replace(wx=wx, wy=wy, wt=wt) for wx, wy, wt in wide]) for c in mc.family_c()]
    runs += [(mc.by_name("a_small_+3-2+2"), None), (mc.by_name("e_band_on"), None)]
    for c, cfgs in runs:
        cfgs = cfgs or [c["cfg"]]
        geo = mc.geo_of(c["grid"])
        cost = mc.cost_of(c["mask"], c["inflation"], geo.res)
        assert cost.size == geo.nx * geo.ny
        gx, gy, res = mc.GRIDS[c["grid"]]
        path = str(tmp_path / (c["name"] + ".bin"))
        with open(path, "wb") as f:
            f.write(np.array([gx, gy, len(c["x"]), len(cfgs), c["band"] is not None], np.int32).tobytes())
            f.write(np.array([res, *c["tf"], *c["guess"]], np.float64).tobytes())
            f.write(np.array(c["band"] or (0.0, 0.0), np.float32).tobytes())
            f.write(cost.tobytes())
            for a in (c["x"], c["y"], c["z"]):
                f.write(np.ascontiguousarray(a, np.float32).tobytes())
            for k in cfgs:
                f.write(bytes(lib_cfg(gvamd, k)))
        out = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and not out.stderr, (c["name"], out.stdout[-500:], out.stderr[-4000:])
        lines = out.stdout.split()
        assert len(lines) == len(cfgs)
        want_r, want_v = mc.want(c)
        assert lines[0] == (want_r.tobytes() + want_v.tobytes()).hex(), c["name"]
        for k, line in zip(cfgs, lines):
            rec, vol = gvamd.match_scan_host(gx, gy, res, cost, c["x"], c["y"], c["z"], c["tf"], lib_cfg(gvamd, k), c["guess"], band=c["band"],
                                             keep_scores=True)
            assert vol.shape == (2 * k.wt + 1, 2 * k.wy + 1, 2 * k.wx + 1)
            assert line == (np.asarray(rec).tobytes() + vol.tobytes()).hex(), (c["name"], k)


def test_one_text_for_both_matchers(gvamd, tmp_path):
    """What the two matchers share lives once: gv_match_rules.hpp and gv_api_match_host.hip are plain C++ that g++ alone
    compiles given only the public include directory (no HIP header, no handle, no __HIPCC__ split), gv_api_search.hip
    is gone, both build recipes name the files, and the library exports what it exported: the four *_SYMBOLS lists and
    the test hooks, nothing else of the C ABI's namespace."""
    csrc = os.path.join(ROOT, "grid-vision_amd", "csrc")
    inc = "-I" + os.path.join(ROOT, "include")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", inc, "-x", "c++", "-c",
                           os.path.join(csrc, "gv_api_match_host.hip"), "-o", str(tmp_path / "host.o")])
    one = str(tmp_path / "rules.cpp")
    with open(one, "w") as f:
        f.write('#include "%s"\n' % os.path.join(csrc, "gv_match_rules.hpp"))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", inc, "-c", one, "-o", str(tmp_path / "rules.o")])
    for name in ("gv_match_rules.hpp", "gv_api_match_host.hip"):
        txt = open(os.path.join(csrc, name)).read()
        assert "__HIPCC__" not in txt and "hip_runtime" not in txt and "gv_context.hpp" not in txt, name
    assert not os.path.exists(os.path.join(csrc, "gv_api_search.hip"))
    from gvamd import build as b
    cmake = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    cmake_globs = "file(GLOB GV_HIP_SOURCES RELATIVE ${GV_CSRC} CONFIGURE_DEPENDS ${GV_CSRC}/*.hip)" in cmake   # every .hip of csrc/
    for s in ("gv_api_match.hip", "gv_api_match_host.hip", "gv_match.hip", "gv_search.hip"):
        assert s in b.SOURCES and cmake_globs and os.path.exists(os.path.join(csrc, s)), s
    assert "gv_api_search.hip" not in b.SOURCES and "gv_api_search.hip" not in cmake
    hooks_txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(csrc, "gv_test_hooks.h")).read(), flags=re.S)
    hooks = set(re.findall(r"\b(gv_test_[a-z0-9_]+)\s*\(", hooks_txt))
    nm = subprocess.run(["nm", "-D", "--defined-only", b.LIB], capture_output=True, text=True, check=True).stdout
    exported = re.findall(r" [A-Za-z] (gv_[A-Za-z0-9_]+)$", nm, flags=re.M)
    want = gvamd.ABI_SYMBOLS + gvamd.MATCH_SYMBOLS + gvamd.SEARCH_SYMBOLS + gvamd.PATH_SYMBOLS + sorted(hooks)
    assert len(want) == len(set(want)) and sorted(exported) == sorted(want), sorted(set(exported) ^ set(want))
