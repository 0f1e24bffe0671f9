"""[EXTENSION] X11 MPPI sampling and softmax update, host side (no GPU): the header, the binding and the struct layout;
gv_mppi_words against Random123's known answers; the library's host twin of the sampling (gv_mppi_sample_controls: the
kernel's arithmetic text compiled for the host) against mppi_ref byte for byte -- the host's C library computes log, sin
and cos on both sides; its statistics inside five-sigma bounds; the host twin of the average (gv_mppi_average) against
mppi_ref's sequential sums on crafted totals; the argument errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mppi_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GV_ERR_BAD_ARG = 1
U64 = ref.U64
INF = float("inf")
SHAPES = [(1, 130), (3, 64), (64, 63), (65, 65), (257, 2), (65, 1)]   # (K, P): rollout_cases.SHAPES

LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "gridvision_hip.h"
int main(void)
{
  printf("%zu %zu %zu %zu %zu %zu %d\n", sizeof(gv_mppi_config), offsetof(gv_mppi_config, sigma), offsetof(gv_mppi_config, u_min),
         offsetof(gv_mppi_config, u_max), offsetof(gv_mppi_config, lambda), offsetof(gv_mppi_config, flags), (int)GV_MPPI_SHIFT);
  return 0;
}
"""

NAMES = ["gv_set_mppi", "gv_mppi_set_nominal", "gv_get_mppi_nominal", "gv_mppi_sample_async", "gv_mppi_sample",
         "gv_device_controls", "gv_get_controls", "gv_mppi_update_async", "gv_mppi_update", "gv_mppi_cycle_async",
         "gv_mppi_cycle", "gv_mppi_words", "gv_mppi_sample_controls", "gv_mppi_average"]


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


def _nominal(P, Cn, seed=0, base=0.3):
    rng = np.random.default_rng(100 + seed)
    return (base + rng.uniform(-0.05, 0.05, (P, Cn))).astype(np.float32)


def test_header_binding_and_layout(gvamd, tmp_path):
    txt = open(os.path.join(ROOT, "include", "gridvision_hip.h")).read()
    for sig in (r"int gv_set_mppi\(gv_handle h, const gv_mppi_config \*cfg\);",
                r"int gv_mppi_set_nominal\(gv_handle h, const float \*nominal, int32_t P\);",
                r"int gv_get_mppi_nominal\(gv_handle h, float \*out[^,]*, int32_t \*P[^)]*\);",
                r"int gv_mppi_sample_async\(gv_handle h, int32_t K, uint64_t seed, uint64_t iteration, uint32_t flags\);",
                r"int gv_mppi_sample\(gv_handle h, int32_t K, uint64_t seed, uint64_t iteration, uint32_t flags\);",
                r"int gv_device_controls\(gv_handle h, float \*\*controls, int32_t \*K, int32_t \*P, int32_t \*C\);",
                r"int gv_get_controls\(gv_handle h, float \*out\);",
                r"int gv_mppi_update_async\(gv_handle h, const gv_critic_weights \*w, uint32_t flags, gv_control_result \*result,\s*"
                r"uint64_t \*totals, float \*nominal_out",
                r"int gv_mppi_update\(gv_handle h, const gv_critic_weights \*w, uint32_t flags, gv_control_result \*result, "
                r"uint64_t \*totals,\s*float \*nominal_out",
                r"int gv_mppi_cycle_async\(gv_handle h, const double start\[3\], int32_t K, uint64_t seed, uint64_t iteration,\s*"
                r"uint32_t sample_flags, const gv_critic_weights \*w, uint32_t flags, gv_control_result \*result,\s*"
                r"uint64_t \*totals, float \*nominal_out",
                r"int gv_mppi_cycle\(gv_handle h, const double start\[3\], int32_t K, uint64_t seed, uint64_t iteration, "
                r"uint32_t sample_flags,",
                r"int gv_mppi_words\(uint64_t seed, uint64_t iteration, uint32_t k, uint32_t p, uint32_t words\[4\]\);",
                r"int gv_mppi_sample_controls\(const gv_mppi_config \*cfg, int32_t C, const float \*nominal, int32_t K, int32_t P, "
                r"uint64_t seed,\s*uint64_t iteration, uint32_t flags, float \*controls_out\);",
                r"int gv_mppi_average\(const gv_mppi_config \*cfg, int32_t C, const float \*controls, const uint64_t \*totals, "
                r"int32_t K,\s*int32_t P, const float \*nominal_in, float \*nominal_out\);"):
        assert re.search(sig, txt), sig
    for phrase in ("Philox4x32-10", "0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "6.283185307179586",
                   "pn = min(p + 1, P - 1)", "e_k = exp(-(x_k / lambda))", "no floating-point atomics"):
        assert phrase in txt, phrase
    lib = gvamd.load()
    for name in NAMES:
        assert name in gvamd.ABI_SYMBOLS and hasattr(lib, name), name
    assert lib.gv_abi_version() == 4
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(LAYOUT)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", exe])
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert C.sizeof(gvamd.MppiConfig) == out[0]
    assert [getattr(gvamd.MppiConfig, n).offset for n, _ in gvamd.MppiConfig._fields_] == out[1:6]
    assert gvamd.MPPI_SHIFT == out[6] == ref.SHIFT


KAT = [(0, 0, 0, 0, "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       (0x299f31d0a4093822, 0x0370734413198a2e, 0x243f6a88, 0x85a308d3, "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("seed,iteration,k,p,want", KAT)
def test_words_known_answers(gvamd, seed, iteration, k, p, want):
    want = [int(w, 16) for w in want.split()]
    assert gvamd.mppi_words(seed, iteration, k, p).tolist() == want
    assert ref.words(seed, iteration, k, p).tolist() == want


def test_words_equal_the_reference_on_a_block(gvamd):
    seed, it = 0x0123456789ABCDEF, (7 << 32) | 5
    want = ref.words(seed, it, np.arange(40)[:, None], np.arange(9)[None, :])
    for k in range(40):
        for p in range(9):
            assert gvamd.mppi_words(seed, it, k, p).tolist() == want[k, p].tolist(), (k, p)
    assert gvamd.load().gv_mppi_words(C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_uint32(0), None) == GV_ERR_BAD_ARG


@pytest.mark.parametrize("shift", [False, True], ids=["plain", "shift"])
@pytest.mark.parametrize("Cn", [2, 3], ids=["diff", "omni"])
def test_sample_controls_equal_the_reference(gvamd, Cn, shift):
    sigma, lo, hi = [0.2, 0.35, 0.1], [-0.1, -0.5, 0.1], [0.6, 0.9, 0.45]
    cfg = gvamd.MppiConfig.of(sigma[:Cn], lo[:Cn], hi[:Cn], 1.0)
    ks, ps = set(), set()
    for i, (K, P) in enumerate(SHAPES):
        nom = _nominal(P, Cn, i)
        want = ref.sample(sigma, lo[:Cn], hi[:Cn], nom, K, 11 + i, 3 + i, ref.SHIFT if shift else 0)
        got = gvamd.mppi_sample_controls(cfg, nom, K, 11 + i, 3 + i, shift)
        assert got.dtype == np.float32 and got.shape == (K, P, Cn)
        assert got.tobytes() == want.tobytes(), (K, P)
        pn = np.minimum(np.arange(P) + 1, P - 1) if shift else np.arange(P)
        assert got[0].tobytes() == np.clip(nom[pn], np.float32(lo[:Cn]), np.float32(hi[:Cn])).astype(np.float32).tobytes()   # row 0
        if K > 1 and P > 1:
            assert (got[1:] != got[0]).any()
        ks.add(K); ps.add(P)
    assert ks == {1, 3, 64, 65, 257} and ps == {1, 2, 63, 64, 65, 130}


def test_sample_sigma_zero_and_clamps(gvamd):
    K, P, Cn = 65, 64, 3
    nom = _nominal(P, Cn, 1)
    # sigma = 0: K copies of the clamped nominal
    cfg = gvamd.MppiConfig.of([0.0] * 3, [-INF, 0.29, -INF], [INF, INF, 0.31], 1.0)
    got = gvamd.mppi_sample_controls(cfg, nom, K, 1, 0)
    row = np.clip(nom, np.float32([-INF, 0.29, -INF]), np.float32([INF, INF, 0.31])).astype(np.float32)
    assert all(got[k].tobytes() == row.tobytes() for k in range(K))
    assert got.tobytes() == ref.sample([0.0] * 3, [-INF, 0.29, -INF], [INF, INF, 0.31], nom, K, 1, 0).tobytes()
    # infinite clamps change nothing; u_min == u_max pins a channel; a clamp at the nominal cuts about half
    sigma = [0.2, 0.2, 0.2]
    lo, hi = [-INF, 0.25, 0.3], [INF, 0.25, INF]
    cfg = gvamd.MppiConfig.of(sigma, lo, hi, 1.0)
    got = gvamd.mppi_sample_controls(cfg, np.full((P, Cn), 0.3, np.float32), K, 2, 0)
    want = ref.sample(sigma, lo, hi, np.full((P, Cn), 0.3, np.float32), K, 2, 0)
    assert got.tobytes() == want.tobytes()
    free = gvamd.mppi_sample_controls(gvamd.MppiConfig.of(sigma), np.full((P, Cn), 0.3, np.float32), K, 2, 0)
    assert free[:, :, 0].tobytes() == got[:, :, 0].tobytes() and (got[:, :, 1] == np.float32(0.25)).all()
    cut = (got[1:, :, 2] == np.float32(0.3)).mean()
    assert 0.4 < cut < 0.6 and (got[:, :, 2] >= np.float32(0.3)).all()
    assert np.array_equal(got[:, :, 2], np.maximum(free[:, :, 2], np.float32(0.3)))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_sample_statistics(gvamd, seed):
    """sigma 1, nominal 0, no clamp: the n samples of rows k >= 1 are standard normal; five-sigma bounds on their mean and
    variance (the variance of a normal sample's variance is 2 / n)"""
    K, P, Cn = 257, 130, 3
    got = gvamd.mppi_sample_controls(gvamd.MppiConfig.of([1.0] * 3), np.zeros((P, Cn), np.float32), K, seed, 0)
    assert (got[0] == 0).all()
    for c in range(Cn):
        z = got[1:, :, c].astype(np.float64).reshape(-1)
        n = z.size
        print("seed", seed, "channel", c, "mean", z.mean(), "of", 5 / np.sqrt(n), "var - 1", z.var() - 1, "of", 5 * np.sqrt(2 / n))
        assert abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1) <= 5 * np.sqrt(2 / n)
    z = got[1:].astype(np.float64).reshape(-1)
    assert abs(z.mean()) <= 5 / np.sqrt(z.size) and abs(z.var() - 1) <= 5 * np.sqrt(2 / z.size)
    other = gvamd.mppi_sample_controls(gvamd.MppiConfig.of([1.0] * 3), np.zeros((P, Cn), np.float32), K, seed, 1)
    assert (other[1:] != got[1:]).mean() > 0.99                    # another iteration: other samples


# ------------------------------------------------------------------------------------------------------- average --
def _avg_case(gvamd, lam, totals, K=9, P=5, Cn=3, seed=0, lo=-0.2, hi=0.8):
    rng = np.random.default_rng(seed)
    u = rng.uniform(lo, hi, (K, P, Cn)).astype(np.float32)
    nom = _nominal(P, Cn, seed)
    t = np.array(totals, np.uint64)
    cfg = gvamd.MppiConfig.of([0.1] * 3, [lo] * 3, [hi] * 3, lam)
    got = gvamd.mppi_average(cfg, u, t, nom)
    want = ref.average(lam, u, t, nom)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (lam, totals)
    assert (got >= np.float32(lo)).all() and (got <= np.float32(hi)).all()
    return u, nom, got


def test_average_crafted_totals(gvamd):
    K = 9
    u, nom, got = _avg_case(gvamd, 10.0, [U64] * K)
    assert got.tobytes() == nom.tobytes()                                         # every trajectory rejected
    u, nom, got = _avg_case(gvamd, 10.0, [U64] * 4 + [12345] + [U64] * 4)
    assert got.tobytes() == u[4].tobytes()                                        # one admitted: its controls
    u, nom, got = _avg_case(gvamd, 10.0, [77] * K)
    mean = u.astype(np.float64).sum(axis=0) / K                                   # all equal: the plain mean
    assert np.abs(got - mean).max() <= 2.0 ** -24 * np.abs(mean).max() + 16 * 2.0 ** -53
    u, nom, got = _avg_case(gvamd, 1e-300, [5, 9, 5, U64, 6, 5, 1000, 7, 8])
    tied = (u[0].astype(np.float64) + u[2] + u[5]) / 3.0                          # ties at the minimum: the mean of the tied
    assert got.tobytes() == tied.astype(np.float32).tobytes()
    u, nom, got = _avg_case(gvamd, 1e300, [5, 9, 5, U64, 6, 5, 1000, 7, 8])
    mean = np.delete(u, 3, axis=0).astype(np.float64).sum(axis=0) / 8             # lambda 1e300: every weight is 1
    assert np.abs(got - mean).max() <= 2.0 ** -24 + 16 * 2.0 ** -53
    big = (1 << 60) + 12345
    _avg_case(gvamd, 3.0, [big + d for d in (4, 0, 9, 2, 1, 30, 3, 0, 6)])       # totals near 2^60: exact differences
    _avg_case(gvamd, 2.0 ** 58, [big, 5, U64, big - 1, 1 << 59, 0, 17, big + 1, 3], seed=4)
    for seed in range(4):                                                         # random totals, larger shapes
        rng = np.random.default_rng(seed)
        K, P = [(64, 7), (65, 63), (257, 2), (3, 130)][seed]
        t = rng.integers(1000, 5000, K).astype(np.uint64)
        t[rng.random(K) < 0.2] = U64
        _avg_case(gvamd, 300.0, t.tolist(), K=K, P=P, Cn=2 + seed % 2, seed=seed)


def test_argument_errors(gvamd):
    lib = gvamd.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    K, P, Cn = 4, 3, 2
    nom = np.full((P, Cn), 0.3, np.float32)
    out = np.zeros((K, P, Cn), np.float32)
    tot = np.array([5, 6, U64, 7], np.uint64)
    nout = np.zeros((P, Cn), np.float32)
    good = dict(sigma=[0.2, 0.2, 0.0], lo=[-1.0, -1.0, 0.0], hi=[1.0, 1.0, 0.0], lam=2.0, flags=0)

    def cfg(**kw):
        d = dict(good); d.update(kw)
        return gvamd.MppiConfig.of(d["sigma"], d["lo"], d["hi"], d["lam"], d["flags"])

    def sample(c=cfg(), Cn_=Cn, nominal=nom, K_=K, P_=P, flags=0, dst=out, null_cfg=False):
        return lib.gv_mppi_sample_controls(None if null_cfg else C.byref(c), C.c_int32(Cn_), p(nominal), C.c_int32(K_), C.c_int32(P_),
                                           C.c_uint64(1), C.c_uint64(2), C.c_uint32(flags), p(dst))

    def average(c=cfg(), Cn_=Cn, controls=out, totals=tot, K_=K, P_=P, nin=nom, dst=nout, null_cfg=False):
        return lib.gv_mppi_average(None if null_cfg else C.byref(c), C.c_int32(Cn_), p(controls), p(totals), C.c_int32(K_), C.c_int32(P_),
                                   p(nin), p(dst))

    assert sample() == 0 and sample(K_=0) == 0 and sample(flags=ref.SHIFT) == 0 and average() == 0 and average(K_=0) == 0
    assert nout.tobytes() == nom.tobytes()                                        # K == 0: nobody admitted
    assert sample(null_cfg=True) == sample(nominal=None) == sample(dst=None) == GV_ERR_BAD_ARG
    assert average(null_cfg=True) == average(controls=None) == average(totals=None) == average(nin=None) == average(dst=None) == GV_ERR_BAD_ARG
    for fn in (sample, average):
        assert fn(Cn_=1) == fn(Cn_=4) == fn(P_=0) == fn(P_=4097) == fn(K_=-1) == fn(K_=(1 << 20) + 1) == GV_ERR_BAD_ARG
        assert fn(K_=(1 << 12) + 1, P_=4096) == GV_ERR_BAD_ARG                    # K * P > 2^24 (checked before any access)
        for bad in (dict(sigma=[-0.1, 0.2]), dict(sigma=[0.1, INF]), dict(sigma=[float("nan"), 0.1]), dict(lo=[0.5, -1.0], hi=[0.4, 1.0]),
                    dict(lo=[float("nan"), -1.0]), dict(hi=[1.0, float("nan")]), dict(lam=0.0), dict(lam=-1.0), dict(lam=INF),
                    dict(lam=float("nan")), dict(flags=1)):
            assert fn(c=cfg(**bad)) == GV_ERR_BAD_ARG, bad
        assert fn(c=cfg(lo=[-INF, -INF], hi=[INF, INF])) == 0                     # infinite clamps are allowed
        assert fn(c=cfg(lo=[0.3, -1.0], hi=[0.3, 1.0])) == 0                      # and u_min == u_max
        assert fn(c=cfg(sigma=[0.2, 0.2, -1.0])) == 0                             # the third channel is not read with C == 2
        assert fn(Cn_=3, c=cfg(sigma=[0.2, 0.2, -1.0]), nominal=np.zeros((P, 3), np.float32)) == GV_ERR_BAD_ARG if fn is sample else True
    assert sample(flags=2) == GV_ERR_BAD_ARG
    for v in (float("nan"), INF, -INF):
        bad = nom.copy(); bad[1, 1] = v
        assert sample(nominal=bad) == GV_ERR_BAD_ARG
