"""Plain references of the helpers of csrc/gv_wave.hpp, one per op of the test hook gv_test_wave (csrc/gv_test_hooks.h):
what every lane of a wavefront must hold after the helper ran on 64 values.  numpy and Python integers only; the integer
ops are exact arithmetic mod 2^32 / 2^64 written as loops over the 64 lanes (tests/test_wave_ref_host.py holds them to
numpy's own scans), the trees are the loop t[:off] += t[off:2*off], off = 32 .. 1, in float64 (held there to
ransac_ref.tree_sum64, the oracle's order).

expected(op, values, active, arg) -> (want, care): (W, 64) uint64 and (W, 64) bool.  `care` is False where the header
promises nothing (the trees outside lane 0, a NaN's payload) and for the append ops, whose places depend on the order
the wavefronts reach the counter in: check_append holds those to their properties instead."""
import collections

import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
INACTIVE = 0xA5A5A5A5A5A5A5A5     # GV_TEST_WAVE_INACTIVE
SKIPPED = 0x5A5A5A5A5A5A5A5A      # GV_TEST_WAVE_SKIPPED
ALL_LANES = M64

FULL_ONLY = lambda op: not (op in ("RANK_LEADER", "APPEND", "APPEND_ALL") or op.startswith(("BCAST_", "GROUP_SUM_")))   # noqa: E731


def mask_ok(op, active, arg=0):
    """the hook's rule for one wavefront's active mask (csrc/gv_test_hooks.h): all 64 lanes for the helpers defined for a full
    wavefront; whole aligned groups for group_sum; the source lane for wave_bcast; lane 0 for wave_append_all"""
    a = int(active)
    if FULL_ONLY(op):
        return a == ALL_LANES
    if op.startswith("GROUP_SUM_"):
        g = int(op[len("GROUP_SUM_"):])
        return all(((a >> s) & ((1 << g) - 1)) in (0, (1 << g) - 1) for s in range(0, 64, g))
    if op.startswith("BCAST_"):
        return bool((a >> arg) & 1)
    if op == "APPEND_ALL":
        return bool(a & 1)
    return True


def _signed(x):
    return x - (1 << 32) if x & 0x80000000 else x


def _scan(v, f):
    out, acc = [], None
    for x in v:
        acc = x if acc is None else f(acc, x)
        out.append(acc)
    return out


_ADD32 = lambda a, b: (a + b) & M32   # noqa: E731
_OPS32 = {"ADD": _ADD32, "MAX": max, "MIN": min}


def tree(values_f64):
    """lane 0 of the fixed-order trees: (W, 64) float64 -> (W,) float64"""
    t = np.array(values_f64, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        off = 32
        while off:
            t[:, :off] += t[:, off:2 * off]
            off >>= 1
    return t[:, 0].copy()


def wave_expected(op, v, arg):
    """one full wavefront: v = 64 Python ints (the uint64 inputs) -> 64 ints, for every op that is a function of the
    wavefront's values alone (not the trees, not the ops that take an active mask)"""
    lo = [x & M32 for x in v]
    kind, _, tail = op.partition("_")
    if kind == "SCAN":
        return _scan(lo, _OPS32[tail])
    if kind == "REDUCE":
        return [_scan(lo, _OPS32[tail])[-1]] * 64
    if op.startswith("SHIFT_DOWN_"):
        h = int(op[len("SHIFT_DOWN_"):])
        return [lo[l + h] if l + h < 64 else arg & M32 for l in range(64)]
    if op.startswith("GROUP_SUM_"):
        g = int(op[len("GROUP_SUM_"):])
        return [sum(lo[l - l % g:l - l % g + g]) & M32 for l in range(64)]
    if op == "MIN_KEY":
        return [min(v)] * 64
    if op == "MAX64":
        return [max(v)] * 64
    if op == "SUM64":
        return [sum(v) & M64] * 64
    if op in ("SUM_I32", "SUM_U32"):
        return [sum(lo) & M32] * 64
    if op == "MAX_I32":
        return [max(lo, key=_signed)] * 64
    if op == "MAX_U32":
        return [max(lo)] * 64
    if op == "SHFL_XOR64":
        return [v[l ^ arg] for l in range(64)]
    if op.startswith("DPP_F64_SHL_"):
        k = int(op[len("DPP_F64_SHL_"):])
        return [v[l + k] if l % 16 + k < 16 else 0 for l in range(64)]   # outside its row: +0.0
    raise ValueError(op)


def expected(op, values, active=None, arg=0):
    values = np.asarray(values, np.uint64)
    W = len(values)
    active = np.full(W, ALL_LANES, np.uint64) if active is None else np.asarray(active, np.uint64)
    want, care = np.zeros((W, 64), np.uint64), np.ones((W, 64), bool)
    assert all(mask_ok(op, a, arg) for a in active), op + ": an active mask the helper's contract does not cover"
    if op in ("BUTTERFLY", "TREE_SHFL"):
        s = tree(values.view(np.float64))
        want[:, 0] = s.view(np.uint64)
        care[:, 1:] = False
        care[:, 0] = ~np.isnan(s)          # a NaN is held to being a NaN (nan_lanes), not to its payload
        return want, care
    for w in range(W):
        v, a = [int(x) for x in values[w]], int(active[w])
        on = [(a >> l) & 1 for l in range(64)]
        if op == "RANK_LEADER" or op.startswith("APPEND"):
            app = [l for l in range(64) if on[l] and v[l] & 1]
            if op != "RANK_LEADER":
                care[w] = False
                row = [0] * 64
            elif not app:
                row = [SKIPPED] * 64
            else:
                row = [(app[0] << 32) | sum(1 for x in app if x < l) for l in range(64)]
        elif op == "BCAST_U64" or op == "BCAST_F64":
            assert on[arg]
            row = [v[arg]] * 64
        elif op == "BCAST_I32":
            assert on[arg]
            row = [v[arg] & M32] * 64
        else:
            row = wave_expected(op, v, arg)
        want[w] = [row[l] if on[l] else INACTIVE for l in range(64)]
    return want, care


def nan_lanes(op, values):
    """(W,) bool: the wavefronts whose tree sum is a NaN (lane 0 must then be a NaN, any payload)"""
    return np.isnan(tree(np.asarray(values, np.uint64).view(np.float64)))


def check_append(op, values, active, out, counter):
    """The properties of wave_append / wave_append_all over every wavefront of one launch (one shared counter; the order of
    the wavefronts is free).  Returns a list of complaints, each naming the wave and the lane; empty when all hold:
    an inactive lane holds INACTIVE, the active lanes of a wave without an appending lane hold SKIPPED, every active lane of
    any other wave reports the same base (high word) and base + its rank among the appending lanes (low word), so places
    ascend with the lane; the places of all waves together are exactly 0 .. total-1; the counter ends at total."""
    values, active, out = np.asarray(values, np.uint64), np.asarray(active, np.uint64), np.asarray(out, np.uint64)
    bad, places = [], []
    for w in range(len(values)):
        a = int(active[w])
        on = [l for l in range(64) if (a >> l) & 1]
        app = [l for l in on if int(values[w, l]) & 1]
        for l in range(64):
            got = int(out[w, l])
            if l not in on:
                if got != INACTIVE:
                    bad.append(f"{op} wave {w} lane {l}: inactive lane holds {got:#018x}, want {INACTIVE:#018x}")
            elif not app:
                if got != SKIPPED:
                    bad.append(f"{op} wave {w} lane {l}: no lane appends, got {got:#018x}, want {SKIPPED:#018x}")
        if not app:
            continue
        base = int(out[w, app[0]]) >> 32
        for l in on:
            got, rank = int(out[w, l]), sum(1 for x in app if x < l)
            want = (base << 32) | ((base + rank) & M32)
            if got != want:
                bad.append(f"{op} wave {w} lane {l}: got {got:#018x}, want {want:#018x} (base {base:#x} of the first "
                           f"appending lane {app[0]}, rank {rank})")
        places += [(int(out[w, l]) & M32, w, l) for l in app]
    total = len(places)
    if sorted(p for p, _, _ in places) != list(range(total)):
        holders = collections.defaultdict(list)
        for p, w, l in places:
            holders[p].append((w, l))
        for p in sorted(p for p, hs in holders.items() if len(hs) > 1)[:4]:
            (w0, l0), (w1, l1) = holders[p][:2]
            bad.append(f"{op} wave {w1} lane {l1}: place {p:#x} is also wave {w0} lane {l0}'s ({len(holders[p])} lanes hold it)")
        for p in sorted(p for p in holders if p >= total)[:4]:
            w, l = holders[p][0]
            bad.append(f"{op} wave {w} lane {l}: place {p:#x} is past the {total} lanes that appended")
        missing = [p for p in range(total) if p not in holders][:8]
        bad.append(f"{op}: the {total} places are not 0..{total - 1}: nobody holds {missing}")
    if counter != total:
        bad.append(f"{op}: the counter ended at {counter}, {total} lanes appended")
    return bad
