"""[EXTENSION] X6 inflated costmap, host side (no GPU): the header, the binding and the struct layout; the library's
host-only cost table against inflate_ref.cost_table byte for byte, with the margins that make the table independent of
the libm; its error cases; the null-handle returns; inflate_ref.dist2 against scipy's exact Euclidean distance
transform; and the fixtures of inflate_cases.py holding what they claim."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import inflate_cases as ic
import inflate_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GV_ERR_BAD_ARG = 1

LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "gridvision_hip.h"
int main(void)
{
  printf("%zu %zu %zu %zu %zu %zu %d %d\n", sizeof(gv_inflation), offsetof(gv_inflation, inscribed_radius),
         offsetof(gv_inflation, inflation_radius), offsetof(gv_inflation, cost_scaling_factor),
         offsetof(gv_inflation, lethal_threshold), offsetof(gv_inflation, flags), (int)GV_INFLATE_KEEP_DIST2,
         (int)GV_INFLATE_OCCUPANCY_SCALE);
  return 0;
}
"""

SIGNATURES = [
    r"int gv_inflation_cost_table\(const gv_inflation \*cfg, double resolution,\s*uint8_t \*table, int32_t cap, int32_t \*n\);",
    r"int gv_set_inflation\(gv_handle h, const gv_inflation \*cfg\);",
    r"int gv_inflate\(gv_handle h\);",
    r"int gv_get_costmap\(gv_handle h, uint8_t \*out\);",
    r"int gv_get_obstacle_dist2\(gv_handle h, uint16_t \*out\);",
    r"int gv_publish_costmap_async\(gv_handle h, uint8_t \*data\);",
]
NAMES = ["gv_inflation_cost_table", "gv_set_inflation", "gv_inflate", "gv_get_costmap", "gv_get_obstacle_dist2",
         "gv_publish_costmap_async"]


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


def _cfg(gvamd, c):
    return gvamd.Inflation(c.inscribed, c.inflation, c.scaling, c.thr, c.flags)


def _table_rc(gvamd, cfg, res, cap=4096, table=True):
    """(status, n, bytes) of a raw gv_inflation_cost_table call"""
    lib = gvamd.load()
    buf = np.full(4096, 7, np.uint8)
    n = C.c_int32(-1)
    rc = lib.gv_inflation_cost_table(C.byref(cfg), C.c_double(res), buf.ctypes.data_as(C.c_void_p) if table else None,
                                     C.c_int32(cap), C.byref(n))
    return rc, n.value, buf


def test_header_binding_and_layout(gvamd, tmp_path):
    txt = open(os.path.join(ROOT, "include", "gridvision_hip.h")).read()
    for sig in SIGNATURES:
        assert re.search(sig, txt), sig
    assert re.search(r"double inscribed_radius;.*?double inflation_radius;.*?double cost_scaling_factor;.*?"
                     r"int32_t lethal_threshold;.*?int32_t flags;.*?\} gv_inflation;", txt, flags=re.S)
    lib = gvamd.load()
    for name in NAMES:
        assert name in gvamd.ABI_SYMBOLS and hasattr(lib, name), name
    assert lib.gv_abi_version() == 4
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(LAYOUT)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", exe])
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert C.sizeof(gvamd.Inflation) == out[0]
    assert [getattr(gvamd.Inflation, n).offset for n, _ in gvamd.Inflation._fields_] == out[1:6]
    assert (gvamd.INFLATE_KEEP_DIST2, gvamd.INFLATE_OCCUPANCY_SCALE) == (out[6], out[7]) == (ref.KEEP_DIST2, ref.OCCUPANCY_SCALE)


@pytest.mark.parametrize("name", sorted(ic.PSETS))
@pytest.mark.parametrize("flags", [0, ref.OCCUPANCY_SCALE, ref.KEEP_DIST2 | ref.OCCUPANCY_SCALE])
def test_table_equals_the_reference(gvamd, name, flags):
    res, cfg = ic.PSETS[name]
    cfg = cfg._replace(flags=flags)
    want = ref.cost_table(cfg, res)
    got = gvamd.inflation_cost_table(_cfg(gvamd, cfg), res)
    assert got.dtype == np.uint8 and got.tobytes() == want.tobytes()
    d2max = ref.d2max_of(cfg, res)
    assert len(got) == d2max + 1
    if name in ic.D2MAX:
        assert d2max == ic.D2MAX[name] and math.isqrt(d2max) == {"P1": 5, "P2": 30, "P3": 63}[name]
    if name == "P4":
        assert math.isqrt(d2max) == 8 and 253 not in got[1:]   # no inscribed ring
    if name == "P3" and not flags:
        assert len(set(got.tolist()) | {0}) == 246   # distinct values of a costmap: the table's and the 0 beyond it
    lethal, inscribed = (100, 99) if flags & ref.OCCUPANCY_SCALE else (254, 253)
    assert got[0] == lethal and (got[1:] < lethal).all() and (np.diff(got.astype(int)) <= 0).all()
    assert ((got == inscribed) == (np.sqrt(np.arange(len(got), dtype=np.float64)) * res <= cfg.inscribed))[1:].all()


def test_p1_prefix_and_end(gvamd):
    res, cfg = ic.PSETS["P1"]
    got = gvamd.inflation_cost_table(_cfg(gvamd, cfg), res)
    assert got[:13].tolist() == [254] + [253] * 12 and got[13] < 253
    assert len(got) == 31 and (got > 0).all()          # every q <= 30 has a cost ...
    assert math.sqrt(31.0) * res > cfg.inflation       # ... and q = 31 lies outside: cost 0 exactly for q > 30


def test_margins_make_the_table_libm_proof():
    """every dist at least 1e-9 m from both radii, every 252 * factor at least 1e-6 from an integer"""
    worst_r, worst_f = math.inf, math.inf
    for name, (res, cfg) in ic.PSETS.items():
        d2max = ref.d2max_of(cfg, res)
        for q in range(1, d2max + 2):
            dist = math.sqrt(float(q)) * res
            worst_r = min(worst_r, abs(dist - cfg.inflation), abs(dist - cfg.inscribed))
            if cfg.inscribed < dist <= cfg.inflation:
                v = 252.0 * math.exp(-cfg.scaling * (dist - cfg.inscribed))
                worst_f = min(worst_f, v - math.floor(v), math.ceil(v) - v)
    print("nearest dist to a radius %.3e m, nearest 252 * factor to an integer %.3e" % (worst_r, worst_f))
    assert worst_r >= 1e-9
    assert worst_f >= 1e-6


def test_canary_fp64_radii(gvamd):
    """3 * 0.1 > 0.3 in fp64: q = 9 is outside the inscribed ring, 251 and not 253; 5 * 0.1 == 0.5 exactly: q = 25 is
    inside the radius and the table's last entry, (uint8_t)(252 * exp(-10 * (0.5 - 0.3))) = (uint8_t)34.10 = 34"""
    cfg = ref.Cfg(0.3, 0.5, 10.0)
    got = gvamd.inflation_cost_table(_cfg(gvamd, cfg), 0.1)
    assert got.tobytes() == ref.cost_table(cfg, 0.1).tobytes()
    assert math.sqrt(9.0) * 0.1 > 0.3 and math.sqrt(25.0) * 0.1 == 0.5
    assert len(got) == 26 and got[8] == 253 and got[9] == 251 and got[25] == 34 == int(252.0 * math.exp(-10.0 * (0.5 - 0.3)))


def test_table_error_cases(gvamd):
    ok = gvamd.Inflation(0.35, 0.55, 10.0, 65, 0)
    rc, n, _ = _table_rc(gvamd, ok, 0.1)
    assert (rc, n) == (0, 31)
    nan, inf = float("nan"), float("inf")
    bad = [gvamd.Inflation(nan, 0.55, 10.0, 65, 0), gvamd.Inflation(0.35, nan, 10.0, 65, 0),
           gvamd.Inflation(0.35, 0.55, nan, 65, 0), gvamd.Inflation(0.35, inf, 10.0, 65, 0),
           gvamd.Inflation(-inf, 0.55, 10.0, 65, 0), gvamd.Inflation(0.35, 0.55, inf, 65, 0),
           gvamd.Inflation(-0.1, 0.55, 10.0, 65, 0), gvamd.Inflation(0.35, 0.55, -1.0, 65, 0),
           gvamd.Inflation(-0.2, -0.1, 10.0, 65, 0),
           gvamd.Inflation(0.35, 0.3, 10.0, 65, 0),                       # inflation < inscribed
           gvamd.Inflation(0.35, 0.55, 10.0, 0, 0), gvamd.Inflation(0.35, 0.55, 10.0, 101, 0),
           gvamd.Inflation(0.35, 0.55, 10.0, 65, 4), gvamd.Inflation(0.35, 0.55, 10.0, 65, -1)]
    for b in bad:
        rc, n, buf = _table_rc(gvamd, b, 0.1)
        assert rc == GV_ERR_BAD_ARG and (buf == 7).all(), [getattr(b, k) for k, _ in b._fields_]
    for res in (0.0, -0.1, nan, inf):
        assert _table_rc(gvamd, ok, res)[0] == GV_ERR_BAD_ARG
    assert _table_rc(gvamd, gvamd.Inflation(0.0, 3.2, 1.0, 65, 0), 0.05)[0] == GV_ERR_BAD_ARG    # Rc = 64
    rc, n, _ = _table_rc(gvamd, gvamd.Inflation(0.0, 3.2 - 1e-9, 1.0, 65, 0), 0.05)             # Rc = 63: the cap
    assert (rc, n) == (0, 4096)
    rc, n, buf = _table_rc(gvamd, ok, 0.1, cap=30)   # cap = n - 1
    assert rc == GV_ERR_BAD_ARG and n == 31 and (buf == 7).all()
    assert _table_rc(gvamd, ok, 0.1, cap=31)[0] == 0
    assert _table_rc(gvamd, ok, 0.1, table=False)[0] == GV_ERR_BAD_ARG
    lib = gvamd.load()
    assert lib.gv_inflation_cost_table(None, C.c_double(0.1), None, C.c_int32(0), None) == GV_ERR_BAD_ARG


def test_null_handle_touches_no_device(gvamd):
    lib = gvamd.load()
    cfg = gvamd.Inflation(0.35, 0.55, 10.0, 65, 0)
    buf = np.zeros(16, np.uint16)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.gv_set_inflation(None, C.byref(cfg)) == GV_ERR_BAD_ARG
    assert lib.gv_set_inflation(None, None) == GV_ERR_BAD_ARG
    assert lib.gv_inflate(None) == GV_ERR_BAD_ARG
    assert lib.gv_get_costmap(None, p) == GV_ERR_BAD_ARG
    assert lib.gv_get_obstacle_dist2(None, p) == GV_ERR_BAD_ARG
    assert lib.gv_publish_costmap_async(None, p) == GV_ERR_BAD_ARG


# ------------------------------------------------------------------------------- the reference's second opinion --

def _edt2(lethal):
    from scipy import ndimage
    return np.rint(ndimage.distance_transform_edt(~lethal) ** 2).astype(np.int64)


@pytest.mark.parametrize("density", [5e-4, 0.3])
@pytest.mark.parametrize("d2max", [30, 4019])
def test_reference_dist2_equals_scipy_edt(density, d2max):
    nx, ny = (200, 120) if d2max == 4019 else (500, 200)
    lethal = ic.random_mask(nx, ny, density, seed=d2max + int(density * 1e4))
    assert lethal.any() and not lethal.all()
    got, want = ref.dist2(lethal, d2max), _edt2(lethal)
    inside = want <= d2max
    assert inside.any() and (density > 0.1 or (~inside).any())
    assert np.array_equal(got[inside], want[inside])
    assert (got[~inside] == ref.NONE).all()


def test_reference_dist2_of_an_empty_mask():
    assert (ref.dist2(np.zeros((7, 9), bool), 30) == ref.NONE).all()
    assert (ref.dist2(np.ones((7, 9), bool), 30) == 0).all()


# ------------------------------------------------------------------------------------------ the fixtures' claims --

def _check_seam(mask, probes, d2max, lines):
    """every probe's nearest lethal cell is its own anchor; the inside ones read their distance, the outside ones none;
    every line is crossed by an inside and an outside pair in each kind of separation that can cross it"""
    true = _edt2(mask)
    got = ref.dist2(mask, d2max)
    n_in = n_out = 0
    for x, y, d in probes:
        assert true[y, x] == d, (x, y, d, true[y, x])
        if d <= d2max:
            assert got[y, x] == d
            n_in += 1
        else:
            assert got[y, x] == ref.NONE
            n_out += 1
    assert n_in and n_out
    ring = ic.ring_offsets(d2max)
    assert all(i[0] ** 2 + i[1] ** 2 <= d2max < o[0] ** 2 + o[1] ** 2 for i, o in ring.values())
    ys, xs = np.nonzero(mask)
    pr = {(x, y) for x, y, _ in probes}
    for line in lines:
        for axis, kinds in ((0, "hd"), (1, "vd")):
            for kind in kinds:
                for which in (0, 1):
                    dx, dy = ring[kind][which]
                    hit = False
                    for ax, ay in zip(xs.tolist(), ys.tolist()):
                        for s in (+1, -1):
                            p = (ax + s * dx, ay + s * dy)
                            a0, p0 = (ax, p[0]) if axis == 0 else (ay, p[1])
                            hit |= p in pr and min(a0, p0) < line <= max(a0, p0)
                    assert hit, (line, axis, kind, which)


def test_seam_fixture_p1_reaches_its_edges():
    mask, probes = ic.seam_fixture(2000, 2000, 30, ic.seam_anchors_p1(), spacing=16)
    sub = mask[:700, :1000]   # every anchor and probe lies here (the transform of the whole 2000 x 2000 adds nothing)
    assert mask.sum() == sub.sum() == 32 and all(x < 1000 and y < 700 for x, y, _ in probes)
    assert sorted({d for _, _, d in probes}) == [25, 29, 32, 36]   # 30 and 31 are no sums of two squares
    _check_seam(sub, probes, 30, range(32, 257, 32))


@pytest.mark.parametrize("k", [1, 2, 3])
def test_seam_fixture_p3_reaches_its_edges(k):
    mask, probes = ic.seam_fixture(200, 200, 4019, ic.seam_anchors_p3(k), spacing=97)
    assert mask.sum() == 2
    assert {d for _, _, d in probes} >= {63 * 63, 64 * 64}
    inside, outside = ic.ring_offsets(4019)["d"]
    assert inside[0] ** 2 + inside[1] ** 2 == 4018 and outside[0] ** 2 + outside[1] ** 2 == 4021   # 4019, 4020: no sums of two squares
    _check_seam(mask, probes, 4019, (32 * k, 32 * (k + 3)))


def test_border_fixture_reaches_its_edges():
    for nx, ny, d2max in ((500, 200, 30), (250, 100, 918), (200, 200, 4019), (200, 80, 70)):
        rc = math.isqrt(d2max)
        m = ic.border_fixture(nx, ny, rc)
        for y in (0, ny - 1):
            for x in (0, nx - 1):
                assert m[y, x]
        assert m[0, nx // 2] and m[ny - 1, nx // 2] and m[ny // 2, nx - 1] and m[:, 0].sum() == 3 and m.sum() == 8
        y = ny // 2
        assert m[y, nx - 1] and not m[y + 1, 0]
        d2 = ref.dist2(m, d2max)
        assert d2[y, nx - 1] == 0 and d2[y + 1, 0] == ref.NONE   # nothing wraps into the next row
        assert d2[y + 1, nx - 1] == 1


def test_threshold_fixture_holds_every_value():
    v = ic.threshold_fixture(500, 200)
    assert v.dtype == np.int8 and v.size == 100000
    assert sorted(set(v.tolist())) == list(range(-1, 101))
