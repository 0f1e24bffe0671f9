"""The references (tests/wave_ref.py) and the inputs (tests/wave_cases.py) of tests/test_gpu_wave.py, proven on the CPU to
be what they claim: the scan references against numpy's own scans, the tree against ransac_ref.tree_sum64 (which
tests/test_ransac_host.py holds to tree_sum64 of oracle/ransac.c), the tree inputs sensitive to the order of the
additions, every lane hot once in every op's lists, the append masks with lane 0 silent and lane 0 inactive; and the
argument rules of the hook gv_test_wave that need no device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import ransac_ref
import wave_cases as wc
import wave_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS_H = os.path.join(ROOT, "grid-vision_amd", "csrc", "gv_test_hooks.h")


def _lo(v):
    return np.asarray(v, np.uint64) & np.uint64(wr.M32)


def test_op_lists_agree_with_the_header():
    """the enum of gv_test_hooks.h, the binding's WAVE_OPS and the case lists name the same ops in the same order, the
    families cover each op once, and the sentinels are the header's"""
    import gvamd
    txt = open(HOOKS_H).read()
    enum = re.search(r"typedef enum gv_test_wave_op \{(.*?)\} gv_test_wave_op;", txt, flags=re.S).group(1)
    names = re.findall(r"GV_TEST_WAVE_([A-Z0-9_]+)", enum)
    assert names[-1] == "OPS" and names[:-1] == gvamd.WAVE_OPS == wc.OPS
    assert "GV_TEST_WAVE_SCAN_ADD = 0" in enum
    assert sorted(op for f in wc.FAMILIES.values() for op in f) == sorted(wc.OPS)
    assert f"#define GV_TEST_WAVE_INACTIVE 0x{wr.INACTIVE:X}ull" in txt and f"#define GV_TEST_WAVE_SKIPPED 0x{wr.SKIPPED:X}ull" in txt
    assert (gvamd.WAVE_INACTIVE, gvamd.WAVE_SKIPPED, gvamd.WAVE_ALL_LANES) == (wr.INACTIVE, wr.SKIPPED, wr.ALL_LANES)


@pytest.mark.parametrize("op", ["SCAN_ADD", "SCAN_MAX", "SCAN_MIN", "REDUCE_ADD", "REDUCE_MAX", "REDUCE_MIN"])
def test_scan_references_equal_numpy(op):
    """np.cumsum / np.maximum.accumulate / np.minimum.accumulate in uint64, reduced mod 2^32, over every list of the op"""
    acc = {"ADD": np.cumsum, "MAX": np.maximum.accumulate, "MIN": np.minimum.accumulate}[op.split("_")[1]]
    for lst in wc.lists(op):
        want, care = wr.expected(op, lst.values, lst.active, lst.arg)
        s = acc(_lo(lst.values), axis=1, dtype=np.uint64) if op.endswith("ADD") else acc(_lo(lst.values), axis=1)
        s = s & np.uint64(wr.M32)
        assert care.all()
        assert np.array_equal(want, s if op.startswith("SCAN") else np.repeat(s[:, 63:], 64, axis=1)), lst.name


@pytest.mark.parametrize("op", [o for o in wc.OPS if o.startswith(("GROUP_SUM", "SUM_", "MAX", "MIN_KEY", "SUM64"))])
def test_reduction_references_equal_numpy(op):
    for lst in wc.lists(op):
        want, _ = wr.expected(op, lst.values, lst.active, lst.arg)
        v = np.asarray(lst.values, np.uint64)
        if op.startswith("GROUP_SUM"):
            g = int(op.split("_")[2])
            s = np.repeat(_lo(v).reshape(-1, 64 // g, g).sum(axis=2, dtype=np.uint64) & np.uint64(wr.M32), g, axis=1)
        elif op in ("SUM_I32", "SUM_U32"):
            s = np.repeat((_lo(v).sum(axis=1, dtype=np.uint64) & np.uint64(wr.M32))[:, None], 64, axis=1)
        elif op == "MAX_I32":
            s = np.repeat(_lo(v).astype(np.uint32).view(np.int32).max(axis=1).astype(np.int32).view(np.uint32).astype(np.uint64)[:, None], 64, axis=1)
        elif op == "MAX_U32":
            s = np.repeat(_lo(v).max(axis=1)[:, None], 64, axis=1)
        elif op == "MAX64":
            s = np.repeat(v.max(axis=1)[:, None], 64, axis=1)
        elif op == "MIN_KEY":
            s = np.repeat(v.min(axis=1)[:, None], 64, axis=1)
        else:   # SUM64: numpy's uint64 sum wraps mod 2^64
            with np.errstate(over="ignore"):
                s = np.repeat(v.sum(axis=1, dtype=np.uint64)[:, None], 64, axis=1)
        on = ((lst.active[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)   # group_sum: groups off
        assert np.array_equal(want[on], s[on]) and (want[~on] == np.uint64(wr.INACTIVE)).all(), lst.name


def test_move_references_known_answers():
    """the ops that only move values, by hand: lane l holds l"""
    v = [list(range(64))]
    w, _ = wr.expected("SHIFT_DOWN_4", v, None, 99)
    assert list(w[0]) == list(range(4, 64)) + [99] * 4
    w, _ = wr.expected("SHFL_XOR64", v, None, 37)
    assert list(w[0]) == [l ^ 37 for l in range(64)] and w[0][0] == 37 and w[0][63] == 26
    w, _ = wr.expected("DPP_F64_SHL_2", v, None, 0)
    assert list(w[0][:16]) == list(range(2, 16)) + [0, 0] and list(w[0][48:]) == list(range(50, 64)) + [0, 0]
    w, _ = wr.expected("BCAST_U64", v, [1 << 9 | 1], 9)
    assert w[0][0] == 9 and w[0][9] == 9 and w[0][1] == wr.INACTIVE
    vals = [[1 if l in (3, 10, 40) else 0 for l in range(64)]]
    w, _ = wr.expected("RANK_LEADER", vals, [wr.ALL_LANES ^ (1 << 3)], 0)     # lane 3 asks but is inactive: lane 10 leads
    assert w[0][3] == wr.INACTIVE and w[0][0] == (10 << 32) and w[0][10] == (10 << 32) and w[0][11] == (10 << 32) | 1
    assert w[0][41] == (10 << 32) | 2 and w[0][63] == (10 << 32) | 2


def test_tree_reference_is_the_oracles_tree():
    """wave_ref.tree == ransac_ref.tree_sum64 on 64 values, by bits, over every tree input; the two ops share their lists"""
    lists = wc.lists("BUTTERFLY")
    twin = wc.lists("TREE_SHFL")
    assert [l.name for l in lists] == [l.name for l in twin] and all(np.array_equal(a.values, b.values) for a, b in zip(lists, twin))
    for lst in lists:
        f = lst.values.view(np.float64)
        s = wr.tree(f)
        with np.errstate(invalid="ignore", over="ignore"):
            o = np.array([ransac_ref.tree_sum64(row) for row in f], np.float64)
        both_nan = np.isnan(s) & np.isnan(o)
        assert np.array_equal(s.view(np.uint64)[~both_nan], o.view(np.uint64)[~both_nan]), lst.name
        assert np.array_equal(np.isnan(s), np.isnan(o))
        want, care = wr.expected("BUTTERFLY", lst.values)
        assert not care[:, 1:].any() and np.array_equal(care[:, 0], ~np.isnan(s))
        assert np.array_equal(wr.nan_lanes("BUTTERFLY", lst.values), np.isnan(s))
    names = [n for l in lists for n in l.names]
    assert any("a NaN" in n for n in names) and any("subnormal" in n for n in names) and any("-0.0" in n for n in names)
    e = lists[1].values.view(np.float64)
    assert np.isnan(wr.tree(e)).sum() == 2 and np.isinf(wr.tree(e)).sum() == 3
    canc = [w for w, n in enumerate(lists[1].names) if n.startswith("cancellation")]   # they do lose bits: not the exact sum
    inexact = [w for w in canc if wr.tree(e[w:w + 1])[0] != math.fsum(e[w].tolist())]
    assert len(canc) == 13 and len(inexact) >= 7, inexact


def test_tree_inputs_tell_the_orders_apart():
    """On at least half of the random tree waves the tree's bits differ from each wrong order ransac_ref.STEP_ORDERS models
    -- the two cross-row steps swapped, the four row steps reversed -- and from the sequential sum.  (STEP_ORDERS places
    its wrong tuples at the level where the product kernel would have them; on 64 values there is one level, so the wrong
    tuple of each name is taken whichever level it is filed under.)"""
    f = wc.tree_random()
    assert f.shape == (64, 64) and np.isfinite(f).all()
    drawn = np.ones(f.shape, bool)
    drawn[np.arange(64), wc.cancel_lane()] = False          # the cancelling lane is computed, not drawn
    e = (np.frexp(np.abs(f))[1] - 1)[drawn]
    assert -40 <= e.min() <= -32 and 32 <= e.max() <= 40    # the list's exponents are spread over +-40
    assert all(abs(math.fsum(row.tolist())) <= np.spacing(np.abs(row).max()) for row in f)   # the exact sum is below an ulp
    ref = wr.tree(f).view(np.uint64)
    right = (32, 16, 8, 4, 2, 1)
    for name in ("rows-swapped", "dpp-reversed"):
        wrong = [t for t in (ransac_ref.STEP_ORDERS[name](0), ransac_ref.STEP_ORDERS[name](1)) if t != right]
        assert len(wrong) == 1 and sorted(wrong[0]) == sorted(right)
        other = np.array([ransac_ref.tree_sum64_steps(row, lambda level: wrong[0]) for row in f]).view(np.uint64)
        assert (other != ref).sum() >= 32, (name, int((other != ref).sum()))
    steps = np.array([ransac_ref.tree_sum64_steps(row, ransac_ref.STEP_ORDERS["steps"]) for row in f]).view(np.uint64)
    assert np.array_equal(steps, ref)
    seq = np.array([np.cumsum(row)[-1] for row in f]).view(np.uint64)
    assert (seq != ref).sum() >= 32


@pytest.mark.parametrize("op", wc.OPS)
def test_lists_cover_every_lane_and_every_shape(op):
    """every op has a list whose 64 waves single out lanes 0 .. 63 in turn and a random list of 64 waves, both run under all
    three workgroup shapes; no list is larger than the hook takes; a full-wavefront op has no partial mask; the reference
    accepts every list"""
    ls = wc.lists(op)
    shaped = [l for l in ls if l.all_shapes]
    assert all(1 <= len(l.values) <= 4096 and l.values.shape[1] == 64 and l.active.shape == (len(l.values),) for l in ls)
    for lst in ls:
        want, care = wr.expected(op, lst.values, lst.active, lst.arg)
        assert want.shape == lst.values.shape == care.shape
        if wr.FULL_ONLY(op):
            assert (lst.active == np.uint64(wr.ALL_LANES)).all()
        assert all(wr.mask_ok(op, a, lst.arg) for a in lst.active)
    if op in ("RANK_LEADER", "APPEND", "APPEND_ALL"):
        m = shaped[0]
        singles = [w for w, n in enumerate(m.names) if n.startswith("only lane")]
        assert [int(np.flatnonzero(m.values[w] & np.uint64(1))[0]) for w in singles] == list(range(64))
        assert sum("random" in n for n in m.names) >= 64
        return
    hots = [l for l in shaped if len(l.values) == 64 and "hot" in l.name]
    assert hots and any(l.name == "random" and len(l.values) == 64 for l in shaped)
    for h in hots:
        for i in range(64):
            row = h.values[i]
            others = np.delete(row, i)
            assert (others == others[0]).all() and row[i] != others[0], (h.name, i)
    if op.startswith("GROUP_SUM"):   # each group alone, each group missing, an idle wavefront: as k_radius_sorted's points leave
        g = int(op.split("_")[2])
        part = [l for l in ls if l.name == "whole groups inactive"][0]
        full = (1 << g) - 1
        alone = {int(a) for a in part.active if bin(int(a)).count("1") == g}
        assert alone == {full << s for s in range(0, 64, g)}
        assert {int(a) ^ wr.ALL_LANES for a in part.active if bin(int(a)).count("1") == 64 - g} == alone and 0 in {int(a) for a in part.active}
        assert not wr.mask_ok(op, wr.ALL_LANES ^ 1) and not wr.mask_ok(op, 1 << 63) and wr.mask_ok(op, 0)
    if op.startswith("SHIFT_DOWN"):
        for lst in ls:   # the fill is no datum and not 0
            assert lst.arg != 0 and not (_lo(lst.values) == np.uint64(lst.arg & wr.M32)).any()
        assert {l.arg for l in ls} == {wc.FILL, wc.FILL_NEG}
    if op == "SHFL_XOR64":
        assert sorted({l.arg for l in ls}) == [1, 2, 4, 8, 16, 32, 37]
    if op.startswith("BCAST"):
        assert {l.arg for l in ls} >= {0, 1, 15, 16, 31, 32, 47, 63} and (op != "BCAST_U64" or {l.arg for l in ls} == set(range(64)))
        assert any((l.active != np.uint64(wr.ALL_LANES)).any() for l in ls)
        assert all(((l.active >> np.uint64(l.arg)) & np.uint64(1)).all() for l in ls)


def test_key_lists_separate_the_halves():
    """64-bit extrema: lists whose keys differ only in the high word, only in the low word, and lists where the halves
    disagree, so that a comparison of swapped halves picks another lane; the 64-bit sum has a carry across the halves"""
    for op in ("MIN_KEY", "MAX64"):
        names = [l.name for l in wc.lists(op)]
        assert any("high word only" in n for n in names) and any("low word only" in n for n in names)
        for lst in wc.lists(op):
            v = lst.values
            if "high word only" in lst.name:
                assert (_lo(v) == _lo(v)[:, :1]).all() and ((v >> np.uint64(32)) != (v >> np.uint64(32))[:, :1]).any(axis=1).all()
            if "low word only" in lst.name:
                assert ((v >> np.uint64(32)) == (v >> np.uint64(32))[:, :1]).all() and (_lo(v) != _lo(v)[:, :1]).any(axis=1).all()
            if "disagree" in lst.name:
                sw = (v << np.uint64(32)) | (v >> np.uint64(32))
                pick = np.argmin if op == "MIN_KEY" else np.argmax
                assert (pick(sw, axis=1) != pick(v, axis=1)).all()
    carry = wc.lists("SUM64")[1].values[0]
    assert (_lo(carry) == np.uint64(wr.M32)).all()
    assert int(_lo(carry).sum(dtype=np.uint64)) >> 32 != 0


def test_append_masks_reach_their_edges():
    """every lane / none / each single lane / lanes 0 and 63 / alternating / random; 256 waves to a counter; "lane 0 not
    appending" and, for wave_append, "lane 0 inactive" in half of the partial waves with the appending lanes a subset of the
    active ones; wave_append_all keeps lane 0 active"""
    names = [n for _, n in wc.append_masks()]
    for what in ("every lane", "no lane", "only lane 0 ", "only lane 63 ", "lanes 0 and 63", "even lanes", "odd lanes", "random"):
        assert any(what in n for n in names), what
    for op in ("APPEND", "APPEND_ALL", "RANK_LEADER"):
        full, part = wc.lists(op)
        assert len(full.values) == 256 and len(part.values) == 256
        assert (full.active == np.uint64(wr.ALL_LANES)).all()
        lane0_silent = ((full.values[:, 0] & np.uint64(1)) == 0) & (full.values & np.uint64(1)).any(axis=1)
        assert lane0_silent.sum() >= 63
        lane0_off = (part.active & np.uint64(1)) == 0
        assert lane0_off.sum() == (0 if op == "APPEND_ALL" else 128)
        asked = np.array([sum(((int(x) & 1) << l) for l, x in enumerate(row)) for row in part.values], dtype=np.uint64)
        assert ((asked & ~part.active) != 0).any()            # lanes that ask but are inactive exist, and must not count
        assert ((asked & part.active) != 0).sum() >= 200      # most waves still append
        assert ((asked & part.active) == 0).any()             # ... and some have nothing to append
        assert (part.active == 0).any() == (op != "APPEND_ALL")   # an idle wavefront, where lane 0 may be inactive


def test_check_append_accepts_any_wave_order_and_names_what_is_wrong():
    """check_append on outputs built by hand: two orders of the waves pass; a shared base, a place out of order, a lost
    place and a wrong counter are each reported with the wave and the lane"""
    full, _ = wc.lists("APPEND")
    v, a = full.values[60:70], full.active[60:70]

    def run(order):
        out, base = np.zeros(v.shape, np.uint64), 0
        for w in order:
            app = [l for l in range(64) if int(v[w, l]) & 1]
            for l in range(64):
                out[w, l] = (base << 32) | (base + sum(1 for x in app if x < l)) if app else wr.SKIPPED
            base += len(app)
        return out, base
    for order in (range(10), reversed(range(10))):
        out, total = run(order)
        assert wr.check_append("APPEND", v, a, out, total) == []
    out, total = run(range(10))
    assert any("counter" in b for b in wr.check_append("APPEND", v, a, out, total + 1))
    bad = out.copy()
    bad[4] = out[5]                                  # wave 4 (every lane appends) reports wave 5's base
    msgs = wr.check_append("APPEND", v, a, bad, total)
    assert any("not 0.." in b for b in msgs) and any(re.search(r"wave [45] lane \d+: place 0x[0-9a-f]+ is also wave [45] lane", b) for b in msgs)
    bad = out.copy()
    bad[4, 7], bad[4, 8] = out[4, 8], out[4, 7]      # two lanes exchanged: places no longer ascend
    msgs = wr.check_append("APPEND", v, a, bad, total)
    assert any("wave 4 lane 7" in b for b in msgs) and any("wave 4 lane 8" in b for b in msgs)
    bad = out.copy()
    bad[2, 0] = wr.INACTIVE
    assert any("wave 2 lane 0" in b for b in wr.check_append("APPEND", v, a, bad, total))


def test_hook_argument_rules_without_a_device():
    """gv_test_wave with a null handle or null pointers: GV_ERR_BAD_ARG before any device call (there is no device here);
    the header declares the hook as the issue states it"""
    import gvamd
    lib = gvamd.load()
    txt = re.sub(r"/\*.*?\*/", "", open(HOOKS_H).read(), flags=re.S)
    assert re.search(r"int gv_test_wave\(gv_handle h, int32_t op, int32_t arg, int32_t threads\s*,\s*const uint64_t \*in\s*,\s*"
                     r"const uint64_t \*active\s*,\s*int64_t n_waves,\s*uint64_t \*out\s*,\s*uint32_t \*counter_out\);", txt)
    v, a, out, cnt = np.zeros(64, np.uint64), np.full(1, wr.ALL_LANES, np.uint64), np.zeros(64, np.uint64), C.c_uint32(7)
    p = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    call = lambda h, i, m, o, c: lib.gv_test_wave(h, C.c_int32(0), C.c_int32(0), C.c_int32(256), i, m, C.c_int64(1), o, c)   # noqa: E731
    assert call(None, None, None, None, None) == 1
    assert call(None, p(v), p(a), p(out), C.byref(cnt)) == 1
    assert cnt.value == 7 and not out.any()
