"""[EXTENSION] X12 MPPI limits and control cost, host side (no GPU): the header, the binding and the struct layout; the
library's host twin of the chain (gv_mppi_constrain: the kernel's arithmetic text compiled for the host) against
mppi_limits_ref byte for byte and at every edge of the definition, each checked to be reached; gv_mppi_control_costs
against the reference's 64 partial sums and tree byte for byte; gv_mppi_average_cc against the reference's sequential sums
on crafted totals and costs; the argument errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mppi_limits_ref as lref
import mppi_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GV_ERR_BAD_ARG = 1
U64 = ref.U64
INF, NAN = float("inf"), float("nan")
F = np.float32
DIFF, OMNI = 0, 1
SHAPES = [(1, 130), (3, 64), (64, 63), (65, 65), (257, 2), (65, 1)]   # (K, P): rollout_cases.SHAPES

LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "gridvision_hip.h"
int main(void)
{
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(gv_mppi_limits), offsetof(gv_mppi_limits, rate_up), offsetof(gv_mppi_limits, rate_down),
         offsetof(gv_mppi_limits, u_prev), offsetof(gv_mppi_limits, min_turn_radius), offsetof(gv_mppi_limits, gamma),
         offsetof(gv_mppi_limits, flags));
  return 0;
}
"""

NAMES = ["gv_set_mppi_limits", "gv_mppi_constrain", "gv_get_mppi_control_costs", "gv_mppi_control_costs", "gv_mppi_average_cc"]


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


def _model(gvamd, model, dt):
    return gvamd.MotionModel(model, dt, 0)


def _f(K, P, Cn, seed=0, lo=-0.4, hi=1.2):
    """controls as a sampling leaves them: independent per (k, p), trajectory 0 smooth"""
    rng = np.random.default_rng(200 + seed)
    f = rng.uniform(lo, hi, (K, P, Cn)).astype(F)
    f[0] = (0.3 + 0.01 * np.arange(P)[:, None] % 0.2).astype(F)
    return f


def test_header_binding_and_layout(gvamd, tmp_path):
    txt = open(os.path.join(ROOT, "include", "gridvision_hip.h")).read()
    for sig in (r"int gv_set_mppi_limits\(gv_handle h, const gv_mppi_limits \*lim\);",
                r"int gv_mppi_constrain\(const gv_mppi_limits \*lim, const gv_motion_model \*m, float \*controls(?: /\*[^*]*\*/)?,\s*"
                r"int32_t K, int32_t P\);",
                r"int gv_get_mppi_control_costs\(gv_handle h, double \*out\);",
                r"int gv_mppi_control_costs\(const gv_mppi_config \*cfg, const gv_mppi_limits \*lim, int32_t C, const float \*controls,\s*"
                r"const float \*nominal, int32_t K, int32_t P, uint32_t sample_flags, double \*g_out\);",
                r"int gv_mppi_average_cc\(const gv_mppi_config \*cfg, int32_t C, const float \*controls, const uint64_t \*totals,\s*"
                r"const double \*control_costs[^,]*, int32_t K, int32_t P,\s*const float \*nominal_in, float \*nominal_out\);"):
        assert re.search(sig, txt), sig
    for phrase in ("lo = s[c] - dn[c];  hi = s[c] + up[c]", "b = fabsf(q[0]) * inv_r", "THIS DEFINITION DOES NOT",
                   "IT IS NOT PASSED THROUGH THE CHAIN AGAIN", "q_c    = sigma[c] > 0 ? gamma / (sigma[c] * sigma[c]) : 0.0",
                   "for w = 32, 16, 8, 4, 2, 1:  a_l = a_l + a_(l+w)", "e_k = exp(-((x_k - m) / lambda))"):
        assert phrase in txt, phrase
    assert "control-cost\n * term, coloured noise and acceleration limits are not part of it" not in txt
    lib = gvamd.load()
    for name in NAMES:
        assert name in gvamd.ABI_SYMBOLS and hasattr(lib, name), name
    assert lib.gv_abi_version() == 4
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(LAYOUT)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", exe])
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert C.sizeof(gvamd.MppiLimits) == out[0]
    assert [getattr(gvamd.MppiLimits, n).offset for n, _ in gvamd.MppiLimits._fields_] == out[1:7]
    m = gvamd.MppiLimits.of()
    assert all(v == INF for v in list(m.rate_up) + list(m.rate_down)) and all(np.isnan(v) for v in m.u_prev)
    assert (m.min_turn_radius, m.gamma, m.flags) == (0.0, 0.0, 0)


# --------------------------------------------------------------------------------------------------------- chain --
def _both(gvamd, model, dt, f, up, dn, prev, radius=0.0):
    """the host twin and the reference on a copy of f each; they must agree by bytes"""
    lim = gvamd.MppiLimits.of(up, dn, prev, radius)
    got = gvamd.mppi_constrain(lim, _model(gvamd, model, dt), f)
    want = lref.constrain(list(lim.rate_up), list(lim.rate_down), list(lim.u_prev), radius, dt, f)
    assert got.dtype == np.float32 and got.shape == f.shape
    assert got.tobytes() == want.tobytes()
    return got


@pytest.mark.parametrize("model", [DIFF, OMNI], ids=["diff", "omni"])
def test_constrain_equals_the_reference(gvamd, model):
    Cn = 2 if model == DIFF else 3
    ks, ps = set(), set()
    for i, (K, P) in enumerate(SHAPES):
        f = _f(K, P, Cn, i)
        up, dn, prev = [2.0, 3.0, 1.5][:Cn], [4.0, 3.0, 0.5][:Cn], [0.25, -0.1, 0.6][:Cn]
        got = _both(gvamd, model, 0.1, f, up, dn, prev, radius=0.8 if model == DIFF else 0.0)
        assert (got != f).any()                                               # the limits bind
        if K * P > 100:
            assert (got == f).any()                                           # and not everywhere
        ks.add(K); ps.add(P)
    assert ks == {1, 3, 64, 65, 257} and ps == {1, 2, 63, 64, 65, 130}


def test_chain_rate_edges(gvamd):
    K, P, Cn, dt = 5, 40, 3, 0.1
    f = _f(K, P, Cn, 7)
    # rate 0 both ways: every control equals u_prev exactly
    prev = [0.3, -0.2, 0.7]
    got = _both(gvamd, OMNI, dt, f, [0.0] * 3, [0.0] * 3, prev)
    assert (got == np.float32(prev)).all()
    # one direction +inf: the value may rise freely, and falls by at most dn a step
    got = _both(gvamd, OMNI, dt, f, [INF] * 3, [1.0] * 3, prev)
    dn = F(1.0 * dt)
    steps = np.diff(np.concatenate([np.broadcast_to(np.float32(prev), (K, 1, Cn)), got], axis=1), axis=1)
    assert (got >= f).all() and (got > f).any() and (got == f).any()          # only ever raised to lo
    assert (steps > 2 * dn).any()                                             # a rise no finite rate of this size allows
    before = np.concatenate([np.broadcast_to(np.float32(prev), (K, 1, Cn)), got[:, :-1]], axis=1)
    assert (got >= (before - dn).astype(F)).all()
    # u_prev NaN on one channel only: step 0 of that channel is free, the others are held
    got = _both(gvamd, OMNI, dt, f, [0.5] * 3, [0.5] * 3, [0.3, NAN, 0.7])
    assert got[:, 0, 1].tobytes() == f[:, 0, 1].tobytes()
    assert (got[:, 0, 0] != f[:, 0, 0]).any() and (got[:, 0, 2] != f[:, 0, 2]).any()
    assert (got[:, 1:, 1] != f[:, 1:, 1]).any()                               # later steps of the free channel are limited
    # q lies between s and f, for every step
    before = np.concatenate([np.broadcast_to(np.float32([0.3, 0.0, 0.7]), (K, 1, Cn)), got[:, :-1]], axis=1)
    before[:, 0, 1] = f[:, 0, 1]
    assert ((got >= np.minimum(before, f)) & (got <= np.maximum(before, f))).all()
    # the neutral struct changes no byte; so do infinite rates with a finite u_prev
    assert _both(gvamd, OMNI, dt, f, [], [], []).tobytes() == f.tobytes()
    assert _both(gvamd, OMNI, dt, f, [INF] * 3, [INF] * 3, prev).tobytes() == f.tobytes()
    assert _both(gvamd, DIFF, dt, f[:, :, :2].copy(), [], [], []).tobytes() == f[:, :, :2].tobytes()


def test_chain_walks_into_the_clamp_box_and_stays(gvamd):
    """u_prev outside [u_min, u_max]: f lies in the box (the X11 clamp made it), the chain comes in at the rate and never
    leaves again"""
    K, P, dt = 9, 50, 0.1
    lo, hi = F(-0.1), F(0.6)
    f = np.clip(_f(K, P, 2, 3), lo, hi).astype(F)
    got = _both(gvamd, DIFF, dt, f, [1.0, 1.0], [1.0, 1.0], [1.5, -0.9])
    inside = (got >= lo) & (got <= hi)
    assert not inside[:, 0].all()                                             # it starts outside
    assert inside[:, -1].all()                                                # and arrives
    first_in = inside.argmax(axis=1)                                          # (K, C)
    for k in range(K):
        for c in range(2):
            assert inside[k, first_in[k, c]:, c].all(), (k, c)
            assert first_in[k, c] >= 7                                        # 0.9 or 0.8 away at 0.1 a step


def test_chain_radius_edges(gvamd):
    dt, r = 0.1, 0.5
    inv_r = F(1.0 / r)
    f = _f(6, 30, 2, 11, lo=-1.0, hi=1.0)
    f[1, :, 0] = 0.0                                                          # v = 0
    f[2, :, 0] = -np.abs(f[2, :, 0]) - F(0.1)                                 # v < 0
    f[3, :, 0] = 0.25
    f[3, ::2, 1] = F(0.25) * inv_r                                            # |w| exactly on the bound
    f[3, 1::2, 1] = -(F(0.25) * inv_r)
    got = _both(gvamd, DIFF, dt, f, [], [], [], radius=r)
    assert got[:, :, 0].tobytes() == f[:, :, 0].tobytes()                     # v is never touched by the radius
    b = (np.abs(got[:, :, 0]) * inv_r).astype(F)
    assert (np.abs(got[:, :, 1]) <= b).all() and (got[:, :, 1] != f[:, :, 1]).any()
    # v = 0: w is a zero, of the sign the definition's branches give
    w0 = got[1, :, 1]
    assert (w0 == 0).all()
    neg = f[1, :, 1] < 0
    assert neg.any() and (~neg).any()
    assert np.signbit(w0[neg]).all() and not np.signbit(w0[~neg & (f[1, :, 1] > 0)]).any()
    # v < 0: the bound is |v| / r
    assert (np.abs(got[2, :, 1]) <= (np.abs(f[2, :, 0]) * inv_r).astype(F)).all() and (got[2, :, 1] != f[2, :, 1]).any()
    # on the bound: unchanged
    assert got[3].tobytes() == f[3].tobytes()
    # radius and rates together
    _both(gvamd, DIFF, dt, f, [2.0, 4.0], [2.0, 4.0], [0.0, 0.0], radius=r)


# -------------------------------------------------------------------------------------------------- control cost --
# (K, P, C): J = P * C of 2, 3, 63, 64, 66, 66, 128, 390.  J = 65 has no (P, C) with C of 2 or 3; the first J past the 64
# lanes that exists is 66, taken both ways.
COST_SHAPES = [(3, 1, 2), (3, 1, 3), (5, 21, 3), (5, 32, 2), (4, 33, 2), (4, 22, 3), (3, 64, 2), (3, 130, 3)]


def test_cost_shapes_cover_the_tree():
    assert sorted(P * Cn for _, P, Cn in COST_SHAPES) == [2, 3, 63, 64, 66, 66, 128, 390]


@pytest.mark.parametrize("shift", [False, True], ids=["plain", "shift"])
@pytest.mark.parametrize("K,P,Cn", COST_SHAPES, ids=["%dx%dx%d" % s for s in COST_SHAPES])
def test_control_costs_equal_the_reference(gvamd, K, P, Cn, shift):
    sigma = [0.2, 0.35, 0.1][:Cn]
    rng = np.random.default_rng(P * 7 + Cn)
    nom = (0.3 + rng.uniform(-0.2, 0.2, (P, Cn))).astype(F)
    u = (nom[None] + rng.normal(0, 0.2, (K, P, Cn))).astype(F)
    cfg = gvamd.MppiConfig.of(sigma, lambda_=1.0)
    lim = gvamd.MppiLimits.of(gamma=0.015)
    got = gvamd.mppi_control_costs(cfg, lim, u, nom, shift)
    want = lref.control_costs(0.015, sigma, u, nom, ref.SHIFT if shift else 0)
    assert got.dtype == np.float64 and got.tobytes() == want.tobytes(), (K, P, Cn)
    assert (got != 0).all()
    if P > 1:
        other = gvamd.mppi_control_costs(cfg, lim, u, nom, not shift)
        assert (other != got).any()                                           # the shift reads another nominal row
    # gamma 0: every cost is 0
    zero = gvamd.mppi_control_costs(cfg, gvamd.MppiLimits.of(), u, nom, shift)
    assert (zero == 0).all()


def test_control_costs_skip_a_channel_without_noise(gvamd):
    K, P, Cn = 4, 21, 3
    rng = np.random.default_rng(5)
    nom = (0.3 + rng.uniform(-0.2, 0.2, (P, Cn))).astype(F)
    u = (nom[None] + rng.normal(0, 0.2, (K, P, Cn))).astype(F)
    sigma = [0.2, 0.0, 0.1]
    lim = gvamd.MppiLimits.of(gamma=2.0)
    got = gvamd.mppi_control_costs(gvamd.MppiConfig.of(sigma), lim, u, nom)
    assert got.tobytes() == lref.control_costs(2.0, sigma, u, nom).tobytes()
    u2 = u.copy()
    u2[:, :, 1] += 5.0                                                        # the skipped channel does not count
    assert gvamd.mppi_control_costs(gvamd.MppiConfig.of(sigma), lim, u2, nom).tobytes() == got.tobytes()
    assert gvamd.mppi_control_costs(gvamd.MppiConfig.of([0.2, 0.3, 0.1]), lim, u2, nom).tobytes() != got.tobytes()


# ------------------------------------------------------------------------------------------------------- average --
def _avg_case(gvamd, lam, totals, g, K=9, P=5, Cn=3, seed=0, lo=-0.2, hi=0.8):
    rng = np.random.default_rng(seed)
    u = rng.uniform(lo, hi, (K, P, Cn)).astype(F)
    nom = (0.3 + np.random.default_rng(100 + seed).uniform(-0.05, 0.05, (P, Cn))).astype(F)
    t = np.array(totals, np.uint64)
    g = np.array(g, np.float64)
    cfg = gvamd.MppiConfig.of([0.1] * 3, [lo] * 3, [hi] * 3, lam)
    got = gvamd.mppi_average_cc(cfg, u, t, g, nom)
    want = lref.average_cc(lam, u, t, g, nom)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (lam, totals)
    return u, nom, got


def test_average_cc_null_costs_is_the_average(gvamd):
    for seed, (K, P) in enumerate([(64, 7), (65, 63), (257, 2), (3, 130)]):
        rng = np.random.default_rng(seed)
        Cn = 2 + seed % 2
        u = rng.uniform(-0.2, 0.8, (K, P, Cn)).astype(F)
        nom = rng.uniform(0.2, 0.4, (P, Cn)).astype(F)
        t = rng.integers(1000, 5000, K).astype(np.uint64)
        t[rng.random(K) < 0.2] = U64
        cfg = gvamd.MppiConfig.of([0.1] * Cn, lambda_=300.0)
        want = gvamd.mppi_average(cfg, u, t, nom)
        assert gvamd.mppi_average_cc(cfg, u, t, None, nom).tobytes() == want.tobytes()
        assert want.tobytes() == ref.average(300.0, u, t, nom).tobytes()
        # costs that are all equal cancel in x - m only up to the rounding of total + g: zeros cancel exactly
        assert gvamd.mppi_average_cc(cfg, u, t, np.zeros(K), nom).tobytes() == want.tobytes()


def test_average_cc_crafted(gvamd):
    K = 9
    rng = np.random.default_rng(1)
    g = rng.normal(0, 20, K)
    u, nom, got = _avg_case(gvamd, 10.0, [U64] * K, g)
    assert got.tobytes() == nom.tobytes()                                         # every trajectory rejected
    u, nom, got = _avg_case(gvamd, 10.0, [U64] * 4 + [12345] + [U64] * 4, g)
    assert got.tobytes() == u[4].tobytes()                                        # one admitted: its controls
    # all totals equal: the weights are g's alone
    u, nom, got = _avg_case(gvamd, 10.0, [77] * K, g)
    e = np.exp(-(g - g.min()) / 10.0)
    mean = (e[:, None, None] * u.astype(np.float64)).sum(axis=0) / e.sum()
    assert np.abs(got - mean).max() <= 2.0 ** -24 * np.abs(mean).max() + 64 * 2.0 ** -53
    assert np.abs(got - u.astype(np.float64).mean(axis=0)).max() > 1e-3           # and not the plain mean
    # a trajectory whose g is negative enough to beat the smallest total: with a cold lambda it takes all the weight
    totals = [500, 9, 700, U64, 60, 5, 1000, 70, 80]
    gg = np.zeros(K); gg[2] = -800.0
    u, nom, got = _avg_case(gvamd, 1e-300, totals, gg)
    assert got.tobytes() == u[2].tobytes()
    u, nom, got = _avg_case(gvamd, 1e-300, totals, np.zeros(K))
    assert got.tobytes() == u[5].tobytes()                                        # without it the best total does
    gg[3] = -1e9                                                                  # a rejected trajectory's g is not read
    u, nom, got = _avg_case(gvamd, 1e-300, totals, gg)
    assert got.tobytes() == u[2].tobytes()
    _avg_case(gvamd, 25.0, totals, gg)
    big = (1 << 60) + 12345
    _avg_case(gvamd, 3.0, [big + d for d in (4, 0, 9, 2, 1, 30, 3, 0, 6)], rng.normal(0, 3, K))
    for seed in range(4):                                                         # random totals, larger shapes
        r = np.random.default_rng(seed)
        Kk, P = [(64, 7), (65, 63), (257, 2), (3, 130)][seed]
        t = r.integers(1000, 5000, Kk).astype(np.uint64)
        t[r.random(Kk) < 0.2] = U64
        _avg_case(gvamd, 300.0, t.tolist(), r.normal(0, 400, Kk), K=Kk, P=P, Cn=2 + seed % 2, seed=seed)


# ------------------------------------------------------------------------------------------------------- errors --
def test_argument_errors(gvamd):
    lib = gvamd.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    K, P, Cn = 4, 3, 2
    nom = np.full((P, Cn), 0.3, F)
    u = np.full((K, P, Cn), 0.25, F)
    tot = np.array([5, 6, U64, 7], np.uint64)
    g = np.zeros(K)
    nout = np.zeros((P, Cn), F)
    cfg = gvamd.MppiConfig.of([0.2, 0.2], [-1.0, -1.0], [1.0, 1.0], 2.0)
    good = dict(up=[1.0, INF, 0.0], dn=[0.0, 2.0, INF], prev=[0.1, NAN, 0.0], radius=0.0, gamma=1.0, flags=0)

    def lim(**kw):
        d = dict(good); d.update(kw)
        return gvamd.MppiLimits.of(d["up"], d["dn"], d["prev"], d["radius"], d["gamma"], d["flags"])

    def constrain(l=lim(), model=DIFF, dt=0.1, mflags=0, ctl=u, K_=K, P_=P, null_lim=False, null_model=False):
        m = gvamd.MotionModel(model, dt, mflags)
        return lib.gv_mppi_constrain(None if null_lim else C.byref(l), None if null_model else C.byref(m), p(ctl.copy() if ctl is not None else None),
                                     C.c_int32(K_), C.c_int32(P_))

    def costs(c=cfg, l=lim(), Cn_=Cn, ctl=u, nominal=nom, K_=K, P_=P, flags=0, dst=g, null_cfg=False, null_lim=False):
        return lib.gv_mppi_control_costs(None if null_cfg else C.byref(c), None if null_lim else C.byref(l), C.c_int32(Cn_), p(ctl), p(nominal),
                                         C.c_int32(K_), C.c_int32(P_), C.c_uint32(flags), p(dst))

    def average(c=cfg, Cn_=Cn, ctl=u, totals=tot, gg=g, K_=K, P_=P, nin=nom, dst=nout, null_cfg=False):
        return lib.gv_mppi_average_cc(None if null_cfg else C.byref(c), C.c_int32(Cn_), p(ctl), p(totals), p(gg), C.c_int32(K_), C.c_int32(P_),
                                      p(nin), p(dst))

    assert constrain() == 0 and constrain(K_=0) == 0 and costs() == 0 and costs(K_=0) == 0 and costs(flags=ref.SHIFT) == 0
    assert average() == 0 and average(gg=None) == 0 and average(K_=0) == 0
    assert nout.tobytes() == nom.tobytes()                                        # K == 0: nobody admitted
    assert constrain(null_lim=True) == constrain(null_model=True) == constrain(ctl=None) == GV_ERR_BAD_ARG
    assert constrain(model=2) == constrain(dt=0.0) == constrain(dt=NAN) == constrain(mflags=1) == GV_ERR_BAD_ARG
    assert constrain(l=lim(radius=0.5)) == 0 and constrain(l=lim(radius=0.5), model=OMNI, ctl=np.zeros((K, P, 3), F)) == GV_ERR_BAD_ARG
    assert costs(null_cfg=True) == costs(null_lim=True) == costs(ctl=None) == costs(nominal=None) == costs(dst=None) == GV_ERR_BAD_ARG
    assert costs(flags=2) == costs(c=gvamd.MppiConfig.of([-0.1, 0.2])) == GV_ERR_BAD_ARG
    assert average(null_cfg=True) == average(ctl=None) == average(totals=None) == average(nin=None) == average(dst=None) == GV_ERR_BAD_ARG
    assert average(c=gvamd.MppiConfig.of([0.1, 0.1], lambda_=0.0)) == GV_ERR_BAD_ARG
    for fn in (constrain, costs, average):
        assert fn(P_=0) == fn(P_=4097) == fn(K_=-1) == fn(K_=(1 << 20) + 1) == GV_ERR_BAD_ARG
        assert fn(K_=(1 << 12) + 1, P_=4096) == GV_ERR_BAD_ARG                    # K * P > 2^24 (checked before any access)
    for fn in (costs, average):
        assert fn(Cn_=1) == fn(Cn_=4) == GV_ERR_BAD_ARG
    for fn in (constrain, costs):
        for bad in (dict(up=[-1.0, 1.0, 1.0]), dict(up=[1.0, NAN, 1.0]), dict(dn=[1.0, 1.0, -0.5]), dict(dn=[NAN, 1.0, 1.0]),
                    dict(up=[1.0, 1.0, -INF]), dict(radius=-0.1), dict(radius=INF), dict(radius=NAN), dict(gamma=-1.0), dict(gamma=INF),
                    dict(gamma=NAN), dict(flags=1)):
            assert fn(l=lim(**bad)) == GV_ERR_BAD_ARG, bad                        # all three channels are checked
        assert fn(l=lim(up=[INF] * 3, dn=[INF] * 3, prev=[INF, -INF, NAN])) == 0   # any u_prev is allowed
    assert lib.gv_set_mppi_limits(None, C.byref(lim())) == lib.gv_get_mppi_control_costs(None, p(g)) == GV_ERR_BAD_ARG
