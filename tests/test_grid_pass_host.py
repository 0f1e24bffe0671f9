"""tests/grid_pass_ref.py on the host: the correctly rounded sigmoid against np.longdouble, the hard-case finder on
constructed inputs, the closure of the reachable 2^-27 set and the planner's coverage of it, the oracle's grid pass
against the reference over the whole set (it may differ only where the host's expf is not correctly rounded, never in
int8), and the oracle's rectangles of poses with a negative length or width (the block of |length| x |width|)."""
import ctypes as C

import numpy as np
import pytest

import grid_pass_ref as R
import oracle_lib as ol
from gvamd import synth

F32 = np.float32


def test_sigmoid_matches_longdouble_on_a_sample():
    st = synth.Stream(2027, 1)
    l = np.concatenate([R.values(st.integers(400_000, 0, R.N_REACHABLE)), st.uniform(400_000, -2.0, 3.6),
                        np.array([-2.0, 3.6, 0.0, -1.8, 3.8], F32)]).astype(F32)
    a, b, _ = R.exp_neg_cr(l)
    want = np.exp(-l.astype(np.longdouble)).astype(F32)
    dec = a == b
    assert dec.mean() > 0.9999
    assert np.array_equal(a[dec], want[dec])
    assert np.all((want[~dec] == a[~dec]) | (want[~dec] == b[~dec]))
    one = F32(1.0)
    pa, _, _ = R.sigmoid_cr(l)
    assert np.array_equal(pa[dec], one / (one + want[dec]))
    assert R.occupancy_ok(one / (one + want), l).all()
    # one ulp off is caught everywhere
    assert not R.occupancy_ok(np.nextafter(pa, F32(2.0)), l).any()
    assert not R.occupancy_ok(np.nextafter(pa, F32(0.0)), l).any()
    # NaN in, NaN out; its int8 is -1
    pn, _, _ = R.sigmoid_cr(np.array([np.nan], F32))
    assert np.isnan(pn[0]) and R.pack_i8(pn)[0] == -1


def test_hard_case_finder_on_constructed_midpoints():
    e32 = np.array([1.0, 0.75, 2.5, 7.389056, 0.13533528, 1.0000001], F32)
    up = np.nextafter(e32, F32(np.inf)).astype(np.float64)
    dn = np.nextafter(e32, F32(0)).astype(np.float64)
    for mid in ((e32 + up) / 2, (e32 + dn) / 2):
        for k in (-4, -1, 0, 1, 4):
            e64 = mid + k * np.spacing(mid)
            assert R._near_mid(e64, e64.astype(F32), 4 * np.spacing(e64)).all(), k
        for k in (-40, 40):
            e64 = mid + k * np.spacing(mid)
            assert not R._near_mid(e64, e64.astype(F32), 4 * np.spacing(e64)).any(), k
        el = mid.astype(np.longdouble) + np.spacing(mid.astype(np.longdouble))
        assert R._near_mid(el, el.astype(F32), 4 * np.spacing(el)).all()


def test_reachable_set_is_closed_and_counted():
    assert R.N_REACHABLE == 107_374_183        # the fp32 multiples of 2^-27 in [-2, 3.6] but -0
    n, prev = 0, None
    for i0, v in R.chunks():
        assert R.on_grid(v).all() and np.all(np.diff(v) > 0)
        assert prev is None or prev < v[0]
        prev = v[-1]
        n += len(v)
        for c in (R.DECAY, R.RECT, R.OCC, R.FREE):
            assert R.on_grid(R.clamp(v + c)).all(), c
    assert n == R.N_REACHABLE
    assert R.values([0])[0] == F32(-2.0) and R.values([R.N_REACHABLE - 1])[0] == F32(3.6)
    assert R.on_grid(np.array([0.0], F32))[0]                       # the prior
    # nothing between two neighbours of the set is on the grid
    v = R.reachable(R.N_REACHABLE // 2 - (1 << 20), R.N_REACHABLE // 2 + (1 << 20))
    nxt = np.nextafter(v[:-1], F32(np.inf))
    assert not R.on_grid(nxt[nxt < v[1:]]).any()


def test_planner_covers_every_reachable_value():
    counts = {r: 0 for r in R.RECIPES}
    no_counts_short = 0
    for i0, v in R.chunks():
        _, rec = R.plan(v)                       # raises unless every value lands exactly
        for i, r in enumerate(R.RECIPES):
            counts[r] += int((rec == i).sum())
        _, rec = R.plan(v, R.NO_COUNTS, partial=True)
        no_counts_short += int((rec == 255).sum())
    assert sum(counts.values()) == R.N_REACHABLE - R.N_NOT_OUTPUT
    assert counts["rect1"] + counts["rect2"] > 0, "decay alone reaches every value"
    assert counts["miss"] > 0 and no_counts_short == counts["hit"] + counts["miss"]
    print(f"planner: {R.N_REACHABLE} values, {R.N_NOT_OUTPUT} no pass outputs, {counts}; {no_counts_short} need a "
          f"frame's hit or miss")
    # the values no pass outputs: no start within +-2 ulps of the inverse lands on them
    v = R.reachable(R.N_REACHABLE // 2 - 4096, R.N_REACHABLE // 2 + 4096)
    odd = ~R.pass_output(v)
    assert odd.sum() == 4096
    for r in R.RECIPES:
        assert not R._invert_chain(v[odd], R.CHAINS[r])[1].any(), r
    # the frame's recipes first: most values land through a hit, the rest still land
    _, rec = R.plan(R.reachable(R.N_REACHABLE - (1 << 22)), ("hit", "miss") + R.NO_COUNTS)
    assert (rec == R.RECIPES.index("hit")).sum() > (1 << 21)


def test_oracle_differs_only_where_host_expf_is_not_correctly_rounded():
    og = ol.OGrid(200, 200, 0.05)        # 16 M cells
    n_hard = n_diff = n = 0
    for i0, v in R.chunks(og.G):
        m = len(v)
        og.log_odds[:m] = v
        og.log_odds[m:] = 0.0
        ol.lib().gvo_clamp_and_sigmoid(C.byref(og.g))
        lo, occ = og.log_odds[:m].copy(), og.occupancy[:m].copy()
        assert np.array_equal(lo, v)
        pa, pb, nh = R.sigmoid_cr(lo)
        n_hard += nh
        d = np.nonzero(~(R._same(occ, pa) | R._same(occ, pb)))[0]
        expf = R.host_expf()
        for i in d:
            e = F32(expf(float(-lo[i])))
            ea, eb, _ = R.exp_neg_cr(lo[i:i + 1])
            assert e != ea[0] and e != eb[0], f"oracle occupancy differs at l={lo[i]!r}, expf correctly rounded"
            assert occ[i] == F32(1.0) / (F32(1.0) + e)
        n_diff += len(d)
        assert np.array_equal(R.pack_i8(occ), R.pack_i8(pa)), "int8 differs"
        assert np.array_equal(R.pack_i8(pb), R.pack_i8(pa))
        n += m
    assert n == R.N_REACHABLE
    print(f"oracle vs correctly rounded occupancy over {n} reachable values: {n_diff} differ (the host's expf), "
          f"{n_hard} fp64 hard cases, int8 never")


@pytest.mark.parametrize("sx,sy", [(-1, 1), (1, -1), (-1, -1)])
def test_oracle_negative_length_width_fill_the_abs_block(sx, sy):
    st = synth.Stream(77, 3 + sx + 2 * sy)
    a, b = ol.OGrid(50, 20, 0.1), ol.OGrid(50, 20, 0.1)
    n = 40
    p = np.zeros(n, synth.LSHAPE_DTYPE)
    p["px"] = st.uniform(n, a.g.pos_x - 20, a.g.pos_x + 20)
    p["py"] = st.uniform(n, -8, 8)
    p["qw"] = 1.0
    p["length"] = st.uniform(n, 0.0, 6.0)
    p["width"] = st.uniform(n, 0.0, 3.0)
    q = p.copy()
    q["length"] *= sx
    q["width"] *= sy
    a.update_map_poses(p)
    b.update_map_poses(q)
    assert np.array_equal(a.log_odds, b.log_odds)
    assert np.count_nonzero(a.log_odds > -0.2) > 100
