"""[EXTENSION] X18 wide-window scan matching by branch and bound, host side (no GPU): the new header, the binding and the
struct layouts; the fixtures' self-checks; the library's host twin gv_match_search_host against search_ref on every
case, record and stats byte for byte, and against X16's twin gv_match_scan_host on every family of match_cases at every
block size; the error table; the twin under AddressSanitizer and UBSan in a stand-alone program.

test_fixtures_are_what_they_claim and test_reference_gives_the_exhaustive_selection exercise search_ref and the
fixtures alone: they call nothing of the library, so they alone of this file would pass on a tree without the feature."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import match_cases as mc
import match_ref as mref
import search_cases as sc
import search_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grid-vision_amd", "csrc")
GV_ERR_BAD_ARG = 1

LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "gridvision_hip_search.h"
#define O(t, f) printf("%zu ", offsetof(t, f))
int main(void)
{
  printf("%zu ", sizeof(gv_search_config));
  O(gv_search_config, wx); O(gv_search_config, wy); O(gv_search_config, wt); O(gv_search_config, stride);
  O(gv_search_config, yaw_step); O(gv_search_config, min_points); O(gv_search_config, flags); O(gv_search_config, block_log2);
  O(gv_search_config, reserved);
  printf("%zu ", sizeof(gv_search_stats));
  O(gv_search_stats, n_blocks); O(gv_search_stats, n_survivors); O(gv_search_stats, n_scored); O(gv_search_stats, seed_block);
  O(gv_search_stats, lower_score); O(gv_search_stats, bound_max); O(gv_search_stats, bound_sum);
  printf("%d\n", (int)GV_SEARCH_USE_BAND);
  return 0;
}
"""

NAMES = ["gv_set_search_config", "gv_match_search_async", "gv_match_search", "gv_match_search_host"]
MATCH_NAMES = ["gv_set_match_config", "gv_match_scan_async", "gv_match_scan", "gv_match_scan_host", "gv_match_rotations", "gv_match_motion"]


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


def lib_cfg(gvamd, c):
    return gvamd.SearchConfig(c.wx, c.wy, c.wt, c.stride, c.yaw_step, c.min_points, c.flags, c.block_log2, 0)


def _declared(path):
    txt = open(path).read()
    return sorted(set(re.findall(r"\b(gv_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))))


def test_header_binding_and_layout(gvamd, tmp_path):
    inc = os.path.join(ROOT, "include")
    assert _declared(os.path.join(inc, "gridvision_hip_search.h")) == sorted(NAMES) == sorted(gvamd.SEARCH_SYMBOLS)
    assert _declared(os.path.join(inc, "gridvision_hip_match.h")) == sorted(MATCH_NAMES) == sorted(gvamd.MATCH_SYMBOLS)
    main = _declared(os.path.join(inc, "gridvision_hip.h"))
    assert main == sorted(gvamd.ABI_SYMBOLS) and len(main) == 123 and not set(main) & set(NAMES)
    assert '#include "gridvision_hip_match.h"' in open(os.path.join(inc, "gridvision_hip_search.h")).read()
    lib = gvamd.load()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.gv_abi_version() == 4
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "123 entry points" in readme and "gridvision_hip_search.h" in readme
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(LAYOUT)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + inc, src, "-o", exe])
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert C.sizeof(gvamd.SearchConfig) == out[0] == 40
    assert [getattr(gvamd.SearchConfig, n).offset for n, _ in gvamd.SearchConfig._fields_] == out[1:10] == [0, 4, 8, 12, 16, 24, 28, 32, 36]
    assert [n for n, _ in gvamd.SearchConfig._fields_] == ["wx", "wy", "wt", "stride", "yaw_step", "min_points", "flags", "block_log2",
                                                           "reserved"]
    for dt in (gvamd.SEARCH_STATS_DTYPE, ref.STATS_DTYPE):
        assert dt.itemsize == out[10] == 32
        assert [dt.fields[n][1] for n in dt.names] == out[11:18] == [0, 4, 8, 12, 16, 20, 24]
        assert dt.names == ("n_blocks", "n_survivors", "n_scored", "seed_block", "lower_score", "bound_max", "bound_sum")
    assert out[18:] == [gvamd.SEARCH_USE_BAND] == [ref.USE_BAND] == [1]


def _best(a):
    r = a.record
    return int(r["best_t"][0]), int(r["best_j"][0]), int(r["best_i"][0])


def test_reference_gives_the_exhaustive_selection():
    """the header's proof, exercised: on every case the record over the survivors and the centre is match_ref's selection
    over the whole volume, and no score of a block is above the block's bound"""
    for c in sc.cases():
        a = sc.want(c)
        cfg = c["cfg"]
        assert _best(a) == mref.select(a.volume, ref.match_cfg(cfg)), c["name"]
        geo = mc.geo_of(c["grid"])
        full = mref.scan(geo, mc.cost_of(c["mask"], c["inflation"], geo.res), mc.m_base(c["tf"]), c["x"], c["y"], c["z"],
                         ref.match_cfg(cfg), c["guess"], c["band"])[0] if a.volume.size <= 65 ** 2 * 3 else None
        assert full is None or full.tobytes() == a.record.tobytes(), c["name"]
        NT, NBY, NBX = a.bounds.shape
        for J in range(NBY):
            for I in range(NBX):
                wj, wi = ref.block_window(cfg, J, I)
                assert (a.volume[:, wj, wi].reshape(NT, -1).max(axis=1) <= a.bounds[:, J, I]).all(), (c["name"], J, I)


def test_fixtures_are_what_they_claim():
    names = sc.names()
    assert len(names) == len(set(names)) and {n.split("_")[0] for n in names} >= {"w", "border", "n", "band", "tie", "zero", "flat",
                                                                                 "loose", "pruning"}
    # every block size at every named window width
    for lg in sc.SIZES:
        S = 1 << lg
        got = {c["edge"]: c["cfg"] for c in sc.windows() if c["cfg"].block_log2 == lg}
        assert set(got) == {"one", "narrow", "rem1", "remS1", "wide"}
        assert (got["one"].wx, got["one"].wy) == (0, 0) and got["one"].wt > 0
        assert 0 < got["narrow"].wx < S and got["narrow"].wy % S == 0 and got["narrow"].wt == 0
        assert (2 * got["rem1"].wx + 1) % S == 1 and (2 * got["remS1"].wx + 1) % S == S - 1
        assert (got["wide"].wx, got["wide"].wy) == (128, 128) and mc.geo_of("big").nx < 257
    for c in sc.windows():
        a = sc.want(c)
        assert int(a.record["n_used"][0]) == len(mc._wall("big")) and int(a.record["best_score"][0]) > 0, c["name"]
        assert a.volume.shape[0] <= 3 and len(c["x"]) <= 300
    # the borders: the points sit in the cells the case names, on the map's ends and up to S cells off it on every side
    for c in sc.borders():
        S = 1 << c["cfg"].block_log2
        geo = mc.geo_of("small")
        a = sc.want(c)
        assert int(a.record["n_used"][0]) == c["n_used"]
        bx, by = mref.used_points(mc.m_base(c["tf"]), c["x"], c["y"], c["z"], ref.match_cfg(c["cfg"]), None)
        ux, uy, ok = mref.cells(geo, c["guess"], np.float32(1.0), np.float32(0.0), bx, by)
        assert (~ok).sum() == c["n_far"]                                   # cells beyond 2^30
        got = list(zip(ux[ok].tolist(), uy[ok].tolist()))
        assert got == c["cells"]
        xs, ys = {p[0] for p in got}, {p[1] for p in got}
        assert {0, geo.nx - 1, -1, -S, geo.nx, geo.nx - 1 + S} <= xs and {0, geo.ny - 1, -1, -S, geo.ny, geo.ny - 1 + S} <= ys
        M = ref.pooled(geo, mc.cost_of(c["mask"], c["inflation"], geo.res), S)
        assert M[:S - 1].any() and M[:, :S - 1].any() and M.shape == (geo.ny + S - 1, geo.nx + S - 1)   # the aprons hold costs
        assert len({a.volume[t].tobytes() for t in range(3)}) > 1
    assert [c["n_used"] for c in sc.counts()] == [0, 1, 63, 64, 65, sc.CHUNK - 1, sc.CHUNK, sc.CHUNK + 1]
    for c in sc.counts():
        assert int(sc.want(c).record["n_used"][0]) == c["n_used"], c["name"]
    a0 = sc.want(sc.by_name("n_0"))
    assert _best(a0) == (0, 0, 0) and int(a0.record["valid"][0]) == 0 and int(a0.stats["n_survivors"][0]) == 0
    on, off, strided = (sc.want(sc.by_name(n)) for n in ("band_on", "band_off", "band_stride"))
    assert int(off.record["n_used"][0]) == 900 and 150 < int(on.record["n_used"][0]) < 500
    bz = sc.by_name("band_on")["z"][:6]
    assert [bool(v) for v in (~(bz < np.float32(0.25)) & ~(bz > np.float32(1.75)))] == [True, False, True, True, True, False]
    assert int(strided.record["n_used"][0]) == 129 and int(strided.record["valid"][0]) == 1
    assert on.record.tobytes() != off.record.tobytes() and on.stats.tobytes() != off.stats.tobytes()
    # the tie: the nearer of two equal alignments lies outside the seed, in a block whose bound equals L
    c = sc.by_name("tie")
    a = sc.want(c)
    assert _best(a) == c["best"] and (a.volume == a.volume.max()).sum() == 2 and a.volume.max() == 3 * 254
    assert a.best_block != int(a.stats["seed_block"][0])
    assert int(a.bounds.reshape(-1)[a.best_block]) == int(a.stats["lower_score"][0]) == 3 * 254
    strict = mref.select(np.where(np.repeat(np.repeat((a.bounds > int(a.stats["lower_score"][0])), 4, 1), 4, 2)[:, :17, :17], a.volume, 0),
                         ref.match_cfg(c["cfg"]))
    assert strict != c["best"]                                            # a prune with > loses it
    # the loose seed: the largest bound does not hold the optimum
    a = sc.want(sc.by_name("loose_seed"))
    assert a.best_block != int(a.stats["seed_block"][0])
    assert int(a.bounds.reshape(-1)[a.best_block]) < int(a.stats["bound_max"][0])
    assert int(a.stats["lower_score"][0]) < int(a.record["best_score"][0])
    # the pruning case: few survivors, the planted displacement
    c = sc.by_name("pruning")
    a = sc.want(c)
    assert _best(a) == c["best"] and int(a.record["best_score"][0]) == len(sc.PRUNE_CELLS) * 254
    assert int(a.stats["n_survivors"][0]) <= int(a.stats["n_blocks"][0]) // 8
    assert int(a.stats["n_blocks"][0]) == 3 * 33 * 33 and (c["cfg"].wx, c["cfg"].wy, c["cfg"].block_log2) == (128, 128, 3)
    # the degenerate ends
    c = sc.by_name("zero")
    a = sc.want(c)
    assert not a.volume.any() and _best(a) == (0, 0, 0) and int(a.record["valid"][0]) == 0 and int(a.stats["n_survivors"][0]) == 0
    assert a.record["x"][0] == c["guess"][0] and a.record["y"][0] == c["guess"][1] and a.record["yaw"][0] == c["guess"][2]
    a = sc.want(sc.by_name("flat"))
    assert (a.volume == 3 * 254).all() and int(a.stats["n_survivors"][0]) == int(a.stats["n_blocks"][0]) > 1
    assert int(a.stats["n_scored"][0]) == a.volume.size and _best(a) == (0, 0, 0)


@pytest.mark.parametrize("name", sc.names())
def test_host_twin_equals_reference(gvamd, name):
    c = sc.by_name(name)
    geo = mc.geo_of(c["grid"])
    cost = mc.cost_of(c["mask"], c["inflation"], geo.res)
    a = sc.want(c)
    rec, stats = gvamd.match_search_host(*sc.GRIDS[c["grid"]], cost, c["x"], c["y"], c["z"], c["tf"], lib_cfg(gvamd, c["cfg"]), c["guess"],
                                         band=c["band"])
    assert np.asarray(stats).tobytes() == a.stats.tobytes(), (name, stats, a.stats)
    assert np.asarray(rec).tobytes() == a.record.tobytes(), (name, rec, a.record)


@pytest.mark.parametrize("name", mc.names())
def test_host_twin_equals_the_exhaustive_twin(gvamd, name):
    """every family of match_cases, the configuration mapped field by field, every block size"""
    c = mc.by_name(name)
    geo = mc.geo_of(c["grid"])
    cost = mc.cost_of(c["mask"], c["inflation"], geo.res)
    m = c["cfg"]
    want = gvamd.match_scan_host(*mc.GRIDS[c["grid"]], cost, c["x"], c["y"], c["z"], c["tf"],
                                 gvamd.MatchConfig(m.wx, m.wy, m.wt, m.stride, m.yaw_step, m.min_points, m.flags), c["guess"], band=c["band"])
    for lg in sc.SIZES:
        cfg = gvamd.SearchConfig(m.wx, m.wy, m.wt, m.stride, m.yaw_step, m.min_points, m.flags, lg, 0)
        rec, stats = gvamd.match_search_host(*mc.GRIDS[c["grid"]], cost, c["x"], c["y"], c["z"], c["tf"], cfg, c["guess"], band=c["band"])
        assert np.asarray(rec).tobytes() == np.asarray(want).tobytes(), (name, lg, rec, want)
        S = 1 << lg
        assert int(stats["n_blocks"]) == (2 * m.wt + 1) * -(-(2 * m.wy + 1) // S) * -(-(2 * m.wx + 1) // S)
        assert int(stats["n_survivors"]) <= int(stats["n_blocks"]) and int(stats["lower_score"]) <= int(rec["best_score"]) <= int(stats["bound_max"])


BAD_CONFIGS = [dict(wx=-1), dict(wx=129), dict(wy=-1), dict(wy=129), dict(wt=-1), dict(wt=33), dict(yaw_step=float("nan")),
               dict(yaw_step=float("inf")), dict(yaw_step=-0.01), dict(wt=1, yaw_step=0.0), dict(stride=0), dict(stride=1025),
               dict(min_points=0), dict(flags=2), dict(block_log2=0), dict(block_log2=5), dict(reserved=1), dict(reserved=-1)]


def test_error_table(gvamd):
    lib = gvamd.load()
    c = sc.by_name("tie")
    geo = mc.geo_of(c["grid"])
    cost = mc.cost_of(c["mask"], c["inflation"], geo.res)
    good = lib_cfg(gvamd, c["cfg"])
    args = lambda cfg, guess=c["guess"]: (*sc.GRIDS[c["grid"]], cost, c["x"], c["y"], c["z"], c["tf"], cfg, guess)   # noqa: E731
    gvamd.match_search_host(*args(good))
    gvamd.match_search_host(*args(gvamd.SearchConfig.of(wx=128, wy=128, wt=0, yaw_step=0.0, stride=1024, min_points=2 ** 31 - 1,
                                                        use_band=True, block_log2=4)))
    gvamd.match_search_host(*args(gvamd.SearchConfig.of(wx=0, wy=0, wt=32, yaw_step=0.01, block_log2=1)))
    for kw in BAD_CONFIGS:
        base = dict(wx=2, wy=2, wt=1, yaw_step=0.01, stride=1, min_points=1, flags=0, block_log2=2, reserved=0)
        base.update(kw)
        with pytest.raises(gvamd.GVError) as e:
            gvamd.match_search_host(*args(gvamd.SearchConfig.of(**base)))
        assert e.value.code == GV_ERR_BAD_ARG, kw
    for k in range(3):
        for v in (float("nan"), float("inf"), float("-inf")):
            guess = list(c["guess"])
            guess[k] = v
            with pytest.raises(gvamd.GVError) as e:
                gvamd.match_search_host(*args(good, guess))
            assert e.value.code == GV_ERR_BAD_ARG
    with pytest.raises(gvamd.GVError):
        gvamd.match_search_host(0, 3, 0.1, *args(good)[3:])                      # a geometry gv_create rejects
    with pytest.raises(gvamd.GVError):
        gvamd.match_search_host(*args(good), band=(2.0, 1.0))                    # a band gv_set_height_band rejects
    # the raw call: null pointers and call flags; nothing is written on error
    x, y, z = c["x"], c["y"], c["z"]
    tf, q = gvamd.make_tf(c["tf"]), gvamd.MatchGuess(*c["guess"])
    res, stats = np.zeros(1, gvamd.MATCH_RESULT_DTYPE), np.zeros(1, gvamd.SEARCH_STATS_DTYPE)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                   # noqa: E731

    def call(cost_=p(cost), x_=p(x), y_=p(y), z_=p(z), n=len(x), tf_=C.byref(tf), cfg_=C.byref(good), q_=C.byref(q), flags=0,
             res_=p(res), stats_=p(stats)):
        return lib.gv_match_search_host(C.c_uint8(5), C.c_uint8(3), C.c_double(0.1), cost_, x_, y_, z_, C.c_size_t(n), tf_, None, cfg_,
                                        q_, C.c_uint32(flags), res_, stats_)

    assert call() == 0 and call(stats_=None) == 0 and call(n=0, x_=None, y_=None, z_=None) == 0
    assert call() == 0
    before = res.tobytes(), stats.tobytes()
    assert res.tobytes() == sc.want(c).record.tobytes() and stats.tobytes() == sc.want(c).stats.tobytes()
    for kw in (dict(cost_=None), dict(x_=None), dict(y_=None), dict(z_=None), dict(tf_=None), dict(cfg_=None), dict(q_=None),
               dict(res_=None), dict(flags=1), dict(flags=2), dict(flags=1 << 31)):
        assert call(**kw) == GV_ERR_BAD_ARG, kw
    assert (res.tobytes(), stats.tobytes()) == before
    assert lib.gv_set_search_config(None, C.byref(good)) == GV_ERR_BAD_ARG
    # the older configuration still refuses what it refused
    for kw in (dict(wx=33), dict(flags=2)):
        with pytest.raises(gvamd.GVError):
            gvamd.match_rotations(gvamd.MatchConfig.of(**dict(dict(wx=2, wy=2, wt=1, yaw_step=0.01), **kw)), c["guess"])


def test_kernel_resources(tmp_path):
    """gv_search.hip device-only with the library's flags: no scratch and no spill of either kind in any kernel, all
    four instantiations of the bound pass included"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    _, text = kr.compile_file("gv_search.hip", str(tmp_path))
    rows = kr.parse_remarks(text)
    for k in ("k_search_pool_rows", "k_search_pool_cols", "k_search_seed", "k_search_fine", "k_search_prune", "k_search_select",
              "k_search_record"):
        assert sum(k in name for name in rows) == 1, (k, sorted(rows))
    assert sum("k_search_bound" in name for name in rows) == 4
    for name, r in rows.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)


SANITIZED_MAIN = r"""
// gv_match_search_host under AddressSanitizer and UBSan: reads one scene and a list of configurations from the file
// the test wrote, prints the 64 + 32 bytes of every answer in hex
#include <cstdio>
#include <cstring>
#include <vector>
#include "gridvision_hip_search.h"
int main(int argc, char **argv)
{
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t head[4];
  double real[11];
  if (std::fread(head, sizeof(head), 1, f) != 1 || std::fread(real, sizeof(real), 1, f) != 1) return 2;
  const int32_t n = head[2], n_cfg = head[3];
  const int nx = (int)(head[0] / real[0] + 0.5), ny = (int)(head[1] / real[0] + 0.5);
  std::vector<uint8_t> cost((size_t)nx * ny);                // exactly the bytes the call may read
  std::vector<float> x((size_t)n), y((size_t)n), z((size_t)n);
  std::vector<gv_search_config> cfg((size_t)n_cfg);
  if (std::fread(cost.data(), 1, cost.size(), f) != cost.size()) return 2;
  for (auto *v : {&x, &y, &z})
    if (n && std::fread(v->data(), sizeof(float), (size_t)n, f) != (size_t)n) return 2;
  if (std::fread(cfg.data(), sizeof(gv_search_config), (size_t)n_cfg, f) != (size_t)n_cfg) return 2;
  std::fclose(f);
  const gv_transform tf{real[1], real[2], real[3], real[4], real[5], real[6], real[7]};
  const gv_match_guess q{real[8], real[9], real[10]};
  for (const gv_search_config &c : cfg) {
    gv_match_result r;
    gv_search_stats st;
    std::memset(&r, 0xAB, sizeof(r));
    std::memset(&st, 0xAB, sizeof(st));
    const int rc = gv_match_search_host((uint8_t)head[0], (uint8_t)head[1], real[0], cost.data(), x.data(), y.data(), z.data(), (size_t)n,
                                        &tf, nullptr, &c, &q, 0, &r, &st);
    if (rc) { std::printf("rc %d\n", rc); return 3; }
    const unsigned char *b = (const unsigned char *)&r, *d = (const unsigned char *)&st;
    for (size_t i = 0; i < sizeof(r); ++i) std::printf("%02x", b[i]);
    for (size_t i = 0; i < sizeof(st); ++i) std::printf("%02x", d[i]);
    std::printf("\n");
  }
  return 0;
}
"""


def test_host_twin_under_sanitizers(gvamd, tmp_path):
    """gv_api_match_host.hip's host twin compiled by g++ with -fsanitize=address,undefined into a stand-alone program with its
    own main (nothing is loaded into Python) and run on the border cases: each case's own configuration (held to
    search_ref) and, over the same scene, the 257 x 257 window and the narrowest ones at every block size (held to the
    library's twin)"""
    src, exe = str(tmp_path / "san.cpp"), str(tmp_path / "san")
    with open(src, "w") as f:
        f.write(SANITIZED_MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), src, "-x", "c++", os.path.join(CSRC, "gv_api_match_host.hip"), "-o", exe])
    for c in sc.borders():
        geo = mc.geo_of(c["grid"])
        cost = mc.cost_of(c["mask"], c["inflation"], geo.res)
        cfgs = [c["cfg"]] + [c["cfg"]._replace(wx=wx, wy=wy, wt=wt, block_log2=lg)
                             for lg in sc.SIZES for wx, wy, wt in ((128, 128, 0), (0, 0, 1), (128, 1, 1), (3, 128, 0))]
        gx, gy, res = sc.GRIDS[c["grid"]]
        path = str(tmp_path / (c["name"] + ".bin"))
        with open(path, "wb") as f:
            f.write(np.array([gx, gy, len(c["x"]), len(cfgs)], np.int32).tobytes())
            f.write(np.array([res, *c["tf"], *c["guess"]], np.float64).tobytes())
            f.write(cost.tobytes())
            for a in (c["x"], c["y"], c["z"]):
                f.write(np.ascontiguousarray(a, np.float32).tobytes())
            for k in cfgs:
                f.write(bytes(lib_cfg(gvamd, k)))
        out = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and not out.stderr, (c["name"], out.stdout[-500:], out.stderr[-4000:])
        lines = out.stdout.split()
        assert len(lines) == len(cfgs)
        a = sc.want(c)
        assert lines[0] == (a.record.tobytes() + a.stats.tobytes()).hex(), c["name"]
        for k, line in zip(cfgs, lines):
            rec, stats = gvamd.match_search_host(gx, gy, res, cost, c["x"], c["y"], c["z"], c["tf"], lib_cfg(gvamd, k), c["guess"])
            assert line == (np.asarray(rec).tobytes() + np.asarray(stats).tobytes()).hex(), (c["name"], k)
