"""The grid pass (A7-A9 + the X2 hit/free rule): a plain host reference the tests hold the three HIP kernels
(k_finalize_tiles, k_finalize_vec4, k_finalize_scalar) and the oracle to, bit for bit.

  l  = l0 + decay (-0.2f); k times l += 0.85f; then hit -> l += 1.2f, else miss -> l += -0.4f  (sequential fp32 adds)
  l  = clamp(l, -2, 3.6)                      (l < -2 ? -2 : l, then l > 3.6 ? 3.6 : l: a NaN stays NaN)
  p  = 1.0f / (1.0f + e),  e = exp(-l) rounded to fp32 CORRECTLY (not the host's expf)
  i8 = (int8)(clamp01(p) * 100.0f), NaN -> -1

The correctly rounded exp: fp64 exp, and where that lies within a few fp64 ulps of an fp32 rounding midpoint, again
in np.longdouble (80-bit on x86-64); where even that cannot decide, both fp32 neighbours are returned and either one
is accepted.

From the prior 0 every log-odds value the pass can hold is an fp32 multiple of 2^-27 in [-2, 3.6] (the set is
closed under the four adds and the clamp): N_REACHABLE = 107,374,183 values, enumerated in ascending order by
reachable().  (As fp32 bit patterns the multiples are one more: -0, which no add produces -- in round to nearest
x + y is -0 only when both are.)  Not every member is the output of a pass: an odd multiple of 2^-27 in
(-(0.2f - 0.125), 0.125) never is.  The constants are multiples of 2^-26, so is any operand of magnitude >= 0.125, and
from a smaller one only -0.2f stays that small, landing in (-0.325, -0.075).  The sigmoid never sees these
N_NOT_OUTPUT values.
plan() picks for every other value a start l0 and a cell recipe that lands exactly on it.
The no-counts recipes (decay, rectangles) reach all but a few values; the rest need the frame's miss (just above -0.5
with an odd last bit, for instance, decay ties to even and the rectangle and hit adds start from a coarser binade).
TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import ctypes
import ctypes.util

import numpy as np

F32 = np.float32
U32 = np.uint32
DECAY, RECT, OCC, FREE = F32(-0.2), F32(0.85), F32(1.2), F32(-0.4)
LO, HI = F32(-2.0), F32(3.6)

# recipes: the adds after l0, and what produces them on the device
RECIPES = ("decay", "rect1", "rect2", "hit", "miss")   # update_map / 1 or 2 whole-map poses / a frame hit / miss
CHAINS = {"decay": (DECAY,), "rect1": (DECAY, RECT), "rect2": (DECAY, RECT, RECT), "hit": (DECAY, OCC),
          "miss": (DECAY, FREE)}
NO_COUNTS = ("decay", "rect1", "rect2")


def _bits(x):
    return int(np.array(x, F32).view(np.uint32))


# ------------------------------------------------------------------------------------------- per-cell update --
def cell_update(l0, k=0, hit=None, miss=None):
    """fp32 restatement of gv_gridpass.hip cell_update: l0 array, k int or int array of covering rectangles,
    hit / miss bool arrays (None: the no-counts form)"""
    l = np.asarray(l0, F32) + DECAY
    k = np.broadcast_to(np.asarray(k), l.shape)
    for r in range(int(k.max()) if k.size else 0):
        l = np.where(k > r, l + RECT, l)
    if hit is not None or miss is not None:
        h = np.zeros(l.shape, bool) if hit is None else np.asarray(hit, bool)
        m = np.zeros(l.shape, bool) if miss is None else np.asarray(miss, bool)
        l = np.where(h, l + OCC, np.where(m, l + FREE, l))
    return clamp(l)


def clamp(l):
    l = np.asarray(l, F32)
    l = np.where(l < LO, LO, l)
    return np.where(l > HI, HI, l).astype(F32)


def apply_recipe(l0, recipe):
    l = np.asarray(l0, F32)
    for c in CHAINS[recipe]:
        l = l + c
    return clamp(l)


# ------------------------------------------------------------------------------------- correctly rounded exp --
def _near_mid(e_hi, e32, tol):
    """|e_hi - midpoint(e32, either fp32 neighbour)| <= tol, in e_hi's precision (fp32 values and their midpoints
    are exact in fp64 and longdouble)"""
    t = e_hi.dtype.type
    up = np.nextafter(e32, F32(np.inf)).astype(t)
    dn = np.nextafter(e32, F32(0)).astype(t)
    e = e32.astype(t)
    return (np.abs(e_hi - (e + up) / 2) <= tol) | (np.abs(e_hi - (e + dn) / 2) <= tol)


def exp_neg_cr(l):
    """exp(-l) correctly rounded to fp32, for a float32 array l (flattened): (a, b, n_hard) with a == b except where
    even the 80-bit exp cannot decide the rounding (then a < b are the two fp32 neighbours); n_hard: how many inputs
    needed the longdouble pass"""
    l = np.asarray(l, F32).reshape(-1)
    x = -l.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        e64 = np.exp(x)
        e32 = e64.astype(F32)
        fin = np.isfinite(e32) & (e32 > 0)
        hard = np.zeros(l.shape, bool)
        hard[fin] = _near_mid(e64[fin], e32[fin], 4 * np.spacing(e64[fin]))
    a, b = e32.copy(), e32.copy()
    idx = np.nonzero(hard)[0]
    if len(idx):
        el = np.exp(x[idx].astype(np.longdouble))
        e32h = el.astype(F32)
        a[idx] = e32h
        b[idx] = e32h
        und = _near_mid(el, e32h, 4 * np.spacing(el))
        if und.any():
            # within 4 ulps of the 80-bit exp from a midpoint: either side of it
            j = idx[und]
            below = el[und] < e32h[und].astype(np.longdouble)
            a[j] = np.where(below, np.nextafter(e32h[und], F32(0)), e32h[und])
            b[j] = np.where(below, e32h[und], np.nextafter(e32h[und], F32(np.inf)))
    return a, b, len(idx)


def sigmoid_cr(l):
    """1.0f / (1.0f + e) with e = exp(-l) correctly rounded: (p_a, p_b, n_hard); p_a == p_b but at undecidable
    inputs, where either is accepted"""
    a, b, n_hard = exp_neg_cr(l)
    one = F32(1.0)
    with np.errstate(over="ignore", invalid="ignore"):
        return (one / (one + a)).astype(F32), (one / (one + b)).astype(F32), n_hard


def pack_i8(p):
    """toOccupancyGrid's int8 of one occupancy value (the cell order data[G-1-cell] is the caller's)"""
    p = np.asarray(p, F32)
    v = (p - F32(0.0)) / (F32(1.0) - F32(0.0))
    nan = np.isnan(v)
    c = np.clip(np.where(nan, F32(0), v), F32(0), F32(1))
    out = np.trunc(F32(0.0) + c * F32(100.0)).astype(np.int8)
    out[nan] = -1
    return out


def occupancy_grid(p):
    """the int8 data array of toOccupancyGrid for a whole grid's occupancy (cell order reversed)"""
    return pack_i8(p)[::-1].copy()


def occupancy_ok(p, l):
    """bool mask: p (float32) is the correctly rounded occupancy of log-odds l (either neighbour at an undecidable
    case); a NaN log-odds wants a NaN"""
    pa, pb, _ = sigmoid_cr(l)
    return _same(p, pa) | _same(p, pb)


def _same(a, b):
    """bit-equal, or both NaN (a NaN's payload is not part of the contract)"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return (a.view(U32) == b.view(U32)) | (np.isnan(a) & np.isnan(b))


_EXPF = None


def host_expf():
    """the host libm's expf, the one the oracle calls (one value per call)"""
    global _EXPF
    if _EXPF is None:
        f = ctypes.CDLL(ctypes.util.find_library("m")).expf
        f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float]
        _EXPF = f
    return _EXPF


def check_layers(lo, occ, i8, o_lo, o_occ, o_i8, want_lo=None, tag=""):
    """One grid after the pass against the oracle's after the same pass on the same start:
      log-odds bit-equal to the oracle's (and to want_lo, the restatement, if given);
      int8 bit-equal to the oracle's and to the pack of occ;
      occupancy bit-equal to the correctly rounded occupancy of the log-odds, and to the oracle's wherever the
      host's expf is correctly rounded.
    NaN log-odds / occupancy compare as NaN.  Returns (n_hard, n_occ_differs_from_oracle)."""
    bad = np.nonzero(~_same(lo, o_lo))[0]
    assert len(bad) == 0, f"{tag} log-odds differ from the oracle at {len(bad)} cells, first {bad[:4]}: " \
                          f"{lo[bad[:4]]} vs {o_lo[bad[:4]]}"
    if want_lo is not None:
        bad = np.nonzero(~_same(lo, want_lo))[0]
        assert len(bad) == 0, f"{tag} log-odds differ from the restatement at {len(bad)} cells, first {bad[:4]}"
    pa, pb, n_hard = sigmoid_cr(lo)
    bad = np.nonzero(~(_same(occ, pa) | _same(occ, pb)))[0]
    assert len(bad) == 0, f"{tag} occupancy not correctly rounded at {len(bad)} cells, first {bad[:4]}: " \
                          f"l={lo[bad[:4]]!r} p={occ[bad[:4]]!r} want {pa[bad[:4]]!r}"
    bad = np.nonzero(i8 != o_i8)[0]
    assert len(bad) == 0, f"{tag} int8 differs from the oracle at {len(bad)} cells, first {bad[:4]}"
    assert np.array_equal(i8, occupancy_grid(occ)), f"{tag} int8 is not the pack of occupancy"
    d = np.nonzero(~_same(occ, o_occ))[0]
    expf = host_expf()
    for i in d:
        e = F32(expf(float(-lo[i])))
        ea, eb, _ = exp_neg_cr(lo[i:i + 1])
        assert e != ea[0] and e != eb[0], f"{tag} occupancy differs from the oracle at l={lo[i]!r}, where the " \
                                          f"host's expf is correctly rounded"
    return n_hard, len(d)


# ------------------------------------------------------------------------------------------- reachable set --
_B_2M4 = _bits(2.0 ** -4)
_NA = _bits(2.0) - _B_2M4 + 1              # [-2, -2^-4]: every fp32
_NB = 2 * (1 << 23) - 1                    # (-2^-4, 2^-4): k * 2^-27, |k| < 2^23
_NC = _bits(3.6) - _B_2M4 + 1              # [2^-4, 3.6]: every fp32
N_REACHABLE = _NA + _NB + _NC


def reachable(i0=0, i1=N_REACHABLE):
    """values [i0, i1) of the reachable set in ascending order, as float32"""
    return values(np.arange(i0, min(i1, N_REACHABLE), dtype=np.int64))


def values(i):
    """the reachable values of index array i (0 <= i < N_REACHABLE, ascending order of the set), as float32"""
    i = np.asarray(i, np.int64)
    out = np.empty(i.shape, F32)
    a = i < _NA
    out[a] = (np.uint32(_bits(-2.0)) - i[a].astype(U32)).view(F32)
    b = (i >= _NA) & (i < _NA + _NB)
    out[b] = (i[b] - _NA - ((1 << 23) - 1)).astype(F32) * F32(2.0 ** -27)
    c = i >= _NA + _NB
    out[c] = (np.uint32(_B_2M4) + (i[c] - _NA - _NB).astype(np.uint32)).view(F32)
    return out


def chunks(size=1 << 24):
    for i0 in range(0, N_REACHABLE, size):
        yield i0, reachable(i0, i0 + size)


_ODD_BOUND = float(np.float32(0.2)) - 0.125


def pass_output(v):
    """False for the members of the reachable set no pass can output (see the module docstring)"""
    v = np.asarray(v, F32)
    k = v.astype(np.float64) * 2.0 ** 27
    d = v.astype(np.float64)
    return ~((d > -_ODD_BOUND) & (d < 0.125) & (np.fmod(k, 2.0) != 0))


N_NOT_OUTPUT = (int(_ODD_BOUND * 2 ** 27) + 1) // 2 + (1 << 23)


def on_grid(v):
    """v is an fp32 multiple of 2^-27 in [-2, 3.6]"""
    v = np.asarray(v, F32)
    s = v.astype(np.float64) * 2.0 ** 27
    return (v >= LO) & (v <= HI) & (s == np.floor(s))


# -------------------------------------------------------------------------------------------------- planner --
def _steps(u, d):
    to = F32(np.inf) if d > 0 else F32(-np.inf)
    for _ in range(abs(d)):
        u = np.nextafter(u, to)
    return u


def _invert_add(v, c):
    """u with fl(u + c) == v (float32), searched from fl(v - c) within +-2 ulps; (u, found)"""
    u0 = (v - c).astype(F32)
    u = np.full(v.shape, np.nan, F32)
    found = np.zeros(v.shape, bool)
    for d in (0, 1, -1, 2, -2):
        cand = _steps(u0, d)
        good = ~found & ((cand + c) == v)
        u[good] = cand[good]
        found |= good
    return u, found


def _invert_chain(v, chain):
    u, ok = v, np.ones(v.shape, bool)
    for c in reversed(chain):
        u, f = _invert_add(u, c)
        ok &= f
    return u, ok


def plan(v, recipes=RECIPES, partial=False):
    """for float32 reachable values v: (l0 float32, recipe index into RECIPES (uint8)); every value gets the first
    recipe of `recipes` whose inverse exists (254: not a pass output).  The clamp bounds come from far-out starts.
    Raises if a plan does not land exactly on its value, or (unless partial: recipe 255 then) if an output is left
    without a plan."""
    v = np.asarray(v, F32)
    l0 = np.full(v.shape, np.nan, F32)
    rec = np.full(v.shape, 255, np.uint8)
    out = pass_output(v)
    rec[~out] = 254
    todo = (v > LO) & (v < HI) & out
    rec[v == LO], l0[v == LO] = RECIPES.index(recipes[0]), F32(-10.0)
    rec[v == HI], l0[v == HI] = RECIPES.index(recipes[0]), F32(10.0)
    for r in recipes:
        if not todo.any():
            break
        idx = np.nonzero(todo)[0]
        u, ok = _invert_chain(v[idx], CHAINS[r])
        l0[idx[ok]] = u[ok]
        rec[idx[ok]] = RECIPES.index(r)
        todo[idx[ok]] = False
    if todo.any() and not partial:
        raise AssertionError(f"{int(todo.sum())} values without a plan, e.g. {v[todo][:8]}")
    for i, r in enumerate(RECIPES):
        m = rec == i
        if m.any():
            got = apply_recipe(l0[m], r)
            assert np.array_equal(got.view(np.uint32), v[m].view(np.uint32)), f"plan {r} misses its value"
    return l0, rec
