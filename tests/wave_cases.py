"""Inputs of tests/test_gpu_wave.py: per op of the test hook gv_test_wave (csrc/gv_test_hooks.h), lists of wavefronts of 64
uint64 values chosen so that the helper's lane mapping shows in its result.  numpy only; tests/test_wave_ref_host.py
proves on the CPU that the lists are what they claim (every lane hot once, fills that no datum equals, tree inputs whose
sum depends on the order of the additions, append masks with lane 0 silent and lane 0 inactive).

lists(op) -> [WaveList]: one launch each.  `names[w]` says what wave w is (a failure quotes it); `all_shapes` lists run
with 64, 256 and 1024 threads to a workgroup, the others with 256."""
import math
from collections import namedtuple

import numpy as np

from wave_ref import ALL_LANES, M32, M64

WaveList = namedtuple("WaveList", "name arg values active names all_shapes")

OPS = ["SCAN_ADD", "SCAN_MAX", "SCAN_MIN", "REDUCE_ADD", "REDUCE_MAX", "REDUCE_MIN",
       "SHIFT_DOWN_1", "SHIFT_DOWN_2", "SHIFT_DOWN_4", "SHIFT_DOWN_8", "GROUP_SUM_8", "GROUP_SUM_16", "MIN_KEY",
       "SUM_I32", "SUM_U32", "MAX_I32", "MAX_U32", "MAX64", "SUM64", "SHFL_XOR64", "BUTTERFLY", "TREE_SHFL",
       "DPP_F64_SHL_1", "DPP_F64_SHL_2", "DPP_F64_SHL_4", "DPP_F64_SHL_8", "RANK_LEADER",
       "BCAST_U64", "BCAST_I32", "BCAST_F64", "APPEND", "APPEND_ALL"]
FAMILIES = {
    "dpp_scans": ["SCAN_ADD", "SCAN_MAX", "SCAN_MIN", "REDUCE_ADD", "REDUCE_MAX", "REDUCE_MIN", "SHIFT_DOWN_1", "SHIFT_DOWN_2",
                  "SHIFT_DOWN_4", "SHIFT_DOWN_8", "GROUP_SUM_8", "GROUP_SUM_16", "MIN_KEY"],
    "xor_butterflies": ["SUM_I32", "SUM_U32", "MAX_I32", "MAX_U32", "MAX64", "SUM64", "SHFL_XOR64"],
    "trees": ["BUTTERFLY", "TREE_SHFL"],
    "dpp_wrappers": ["DPP_F64_SHL_1", "DPP_F64_SHL_2", "DPP_F64_SHL_4", "DPP_F64_SHL_8"],
    "appends": ["RANK_LEADER", "BCAST_U64", "BCAST_I32", "BCAST_F64", "APPEND", "APPEND_ALL"],
}
SHAPES = (64, 256, 1024)

FILL = 0x7E57F111            # wave_shift_down's fill: no datum of its lists, not 0
FILL_NEG = 0x8BADF00D        # the same with the sign bit set (arg is an int32)
XOR_OFFSETS = (1, 2, 4, 8, 16, 32, 37)
BCAST_LANES_ALL = tuple(range(64))
BCAST_LANES_FEW = (0, 1, 15, 16, 31, 32, 47, 63)
HOT32 = 0x9E3779B1           # odd, sign bit set
HOT64 = (0x9E3779B1 << 32) | 0x85EBCA6B
PI_BITS = 0x400921FB54442D18


def _u64(rows):
    return np.array(rows, dtype=np.uint64).reshape(-1, 64)


def _full(n):
    return np.full(n, ALL_LANES, np.uint64)


def _mk(name, rows, names, arg=0, active=None, all_shapes=False):
    v = _u64(rows)
    assert len(names) == len(v)
    return WaveList(name, arg, v, _full(len(v)) if active is None else np.array(active, dtype=np.uint64), list(names), all_shapes)


def hot(bg, value, name="one-hot", arg=0):
    """64 waves: wave i is `bg` everywhere but lane i, which holds value(i)"""
    rows = [[value(i) if l == i else bg for l in range(64)] for i in range(64)]
    return _mk(name, rows, [f"{name}: lane {i} holds {value(i):#x}, the others {bg:#x}" for i in range(64)], arg, all_shapes=True)


def rand64(seed, n=64):
    return np.random.default_rng(seed).integers(0, 1 << 64, size=(n, 64), dtype=np.uint64)


def random_list(seed, bits, arg=0, n=64):
    v = rand64(seed, n)
    if bits == 32:   # the high word is garbage a 32-bit op must not read
        v = (v & np.uint64(M32)) | (np.uint64(0xC0FFEE00) << np.uint64(32))
    return _mk("random", v, [f"random wave {w} (seed {seed})" for w in range(n)], arg, all_shapes=True)


def ties(bg, extreme, name):
    pairs = [(0, 63), (15, 16), (31, 32), (47, 48), (7, 8), (0, 1), (62, 63), (20, 41)]
    rows = [[extreme if l in p else bg for l in range(64)] for p in pairs]
    return rows, [f"{name}: lanes {p[0]} and {p[1]} both hold {extreme:#x}, the others {bg:#x}" for p in pairs]


def _signed_mix():
    """negatives and positives: the signed and the unsigned maximum differ, the sum wraps through zero"""
    a = [(-(l + 1)) & M32 if l % 3 else l + 1 for l in range(64)]
    b = [0x80000000 if l % 2 else 0x7FFFFFFF for l in range(64)]
    c = [(-1) & M32] * 64
    c[17] = 7
    return [a, b, c], ["signed mix: -(l+1), l+1 at every third lane", "signed mix: INT_MIN / INT_MAX alternating",
                       "signed mix: -1 everywhere, 7 at lane 17"]


def _add32_lists(group=0):
    sm, sn = _signed_mix()
    rows = [[M32] * 64, [1] * 64, [l + 1 for l in range(64)]] + sm
    names = ["all 0xFFFFFFFF (the sum wraps)", "all ones", "lane l holds l + 1"] + sn
    out = [hot(0, lambda i: HOT32), _mk("edges", rows, names), random_list(101, 32)]
    if group:   # group_sum as k_radius_sorted calls it: whole groups of the wavefront already gone, the others still summing
        n = 64 // group
        r = np.random.default_rng(109)
        pick = [1 << k for k in range(n)] + [((1 << n) - 1) ^ (1 << k) for k in range(n)] + [0]
        pick += [int(r.integers(0, 1 << n)) for _ in range(64 - len(pick))]
        act = [sum(((1 << group) - 1) << (group * k) for k in range(n) if (p >> k) & 1) for p in pick]
        v = random_list(110, 32).values[:len(act)]
        out.append(_mk("whole groups inactive", v, [f"random values, lanes {a:#018x} active (groups of {group})" for a in act],
                       active=act))
    return out


def _max32_lists(signed):
    bg, val = (0x80000005, lambda i: 0xFFFFFFF0 - i) if signed else (0, lambda i: 0x80000000 | (i + 1))
    t, tn = ties(bg, 0x7FFFFFF0 if signed else 0xFFFFFFF0, "tie")
    sm, sn = _signed_mix()
    rows = t + [[0] * 64] + sm
    return [hot(bg, val, "maximum-hot"), _mk("edges", rows, tn + ["all zeros (OpMax's identity)"] + sn), random_list(102, 32)]


def _min32_lists():
    t, tn = ties(M32, 3, "tie")
    sm, sn = _signed_mix()
    rows = t + [[M32] * 64, [0] * 64] + sm
    return [hot(M32, lambda i: 0x1000 + i, "minimum-hot"),
            _mk("edges", rows, tn + ["all 0xFFFFFFFF (OpMin's identity)", "all zeros"] + sn), random_list(103, 32)]


def _key_lists(want_min):
    """64-bit extrema: keys that differ only in the high word, only in the low word, and whose halves disagree"""
    c = 0x12345678
    if want_min:
        hi = hot((M32 << 32) | c, lambda i: (5 << 32) | c, "minimum-hot, high word only")
        lo = hot((c << 32) | M32, lambda i: (c << 32) | 5, "minimum-hot, low word only")
        dis = hot((M32 << 32) | 1, lambda i: (5 << 32) | 0xFFFFFFF0, "minimum-hot, halves disagree")
        t, tn = ties(M64, (7 << 32) | 9, "tie")
        rows, names = t + [[M64] * 64, [0] * 64], tn + ["all ones", "all zeros"]
    else:
        hi = hot((1 << 32) | c, lambda i: (0xFFFFFFF0 << 32) | c, "maximum-hot, high word only")
        lo = hot((c << 32) | 1, lambda i: (c << 32) | 0xFFFFFFF0, "maximum-hot, low word only")
        dis = hot((1 << 32) | 0xFFFFFFF0, lambda i: (0xFFFFFFF0 << 32) | 1, "maximum-hot, halves disagree")
        t, tn = ties(0, (7 << 32) | 9, "tie")
        rows, names = t + [[0] * 64, [M64] * 64], tn + ["all zeros", "all ones"]
    return [hi, lo, dis, _mk("edges", rows, names), random_list(104 + want_min, 64)]


def _sum64_lists():
    carry = [[((l + 1) << 32) | M32 for l in range(64)], [M32] * 64, [M64] * 64]
    names = ["every low word 0xFFFFFFFF, high word l + 1 (the carry crosses the halves)", "all 0x00000000FFFFFFFF",
             "all ones (wraps mod 2^64)"]
    return [hot(0, lambda i: HOT64), _mk("edges", carry, names), random_list(106, 64)]


def _iota64():
    return [(l << 32) | (~l & M32) for l in range(64)]


def _move_lists(arg, seed):
    """ops that only move values between lanes: one-hot, every lane its own value, random bits (NaN patterns included)"""
    return [hot(0, lambda i: PI_BITS, arg=arg), _mk("edges", [_iota64()], ["lane l holds (l << 32) | ~l"], arg),
            random_list(seed, 64, arg)]


# ---- the trees

def _f64_rows(rows):
    return np.array(rows, dtype=np.float64).reshape(-1, 64).view(np.uint64)


def tree_random(seed=7, n=64, centre=32, spread=8):
    """n waves of doubles whose binary exponents are spread over +-(centre + spread) = +-40: random 53-bit mantissas and
    signs; wave w draws its exponents uniformly within `spread` of a centre of its own in [-centre, centre]; then one lane
    of the wave (cancel_lane) is replaced by minus the exact sum of the other 63.
    Why this shape: with exponents uniform over +-40 inside ONE wave the few largest values decide the sum, and two orders
    of the additions agree in all 64 bits on more than half of the waves (measured on the reference alone: 27 of 64 differ
    for the swapped cross-row steps).  Values of like magnitude round at every addition, and the cancelling lane makes the
    result the accumulated rounding error itself, which the final rounding cannot hide: the orders then differ on about 45
    of 64 waves (tests/test_wave_ref_host.py asserts at least half, per wrong order)."""
    r = np.random.default_rng(seed)
    m = 1.0 + r.integers(0, 1 << 52, size=(n, 64)).astype(np.float64) / float(1 << 52)
    c = r.integers(-centre, centre + 1, size=(n, 1))
    e = c + r.integers(-spread, spread + 1, size=(n, 64))
    s = np.where(r.integers(0, 2, size=(n, 64)) == 1, -1.0, 1.0)
    f = np.ldexp(m, e) * s
    for w, p in enumerate(cancel_lane(seed, n)):
        f[w, p] = 0.0
        f[w, p] = -math.fsum(f[w].tolist())
    return f


def cancel_lane(seed=7, n=64):
    return [int(p) for p in np.random.default_rng(seed + 1000).integers(0, 64, size=n)]


def tree_edges():
    rows, names = [], []
    for k in range(3):   # periods that are no power of two: partners of a step differ in magnitude
        rows.append([[1e16, 1.0, -1e16][(l + k) % 3] for l in range(64)])
        names.append(f"cancellation: 1e16, 1, -1e16 repeating from phase {k}")
    for k in range(2):
        rows.append([[1e16, 1.0, -1e16, 3.0, 1e-3][(l + k) % 5] for l in range(64)])
        names.append(f"cancellation: 1e16, 1, -1e16, 3, 1e-3 repeating from phase {k}")
    for i, j in [(0, 32), (0, 16), (0, 8), (0, 1), (63, 0), (31, 33), (15, 16), (40, 7)]:
        rows.append([1e16 if l == i else -1e16 if l == j else 1.0 for l in range(64)])
        names.append(f"cancellation: 1e16 at lane {i}, -1e16 at lane {j}, ones elsewhere")
    rows += [[-0.0] * 64, [0.0] * 64, [-0.0 if l == 0 else 0.0 for l in range(64)], [-0.0 if l else 0.0 for l in range(64)]]
    names += ["all -0.0", "all +0.0", "-0.0 at lane 0 only", "+0.0 at lane 0, -0.0 elsewhere"]
    inf = float("inf")
    rows += [[inf if l == 21 else 1.0 for l in range(64)], [-inf if l == 63 else 1.0 for l in range(64)],
             [inf if l == 3 else -inf if l == 44 else 1.0 for l in range(64)],
             [float("nan") if l == 5 else 1.0 for l in range(64)], [1e308] * 64]
    names += ["+inf at lane 21", "-inf at lane 63", "+inf at lane 3 and -inf at lane 44 (a NaN)", "a NaN at lane 5",
              "all 1e308 (overflows to +inf)"]
    sub, nrm = 5e-324, 2.2250738585072014e-308
    rows += [[sub] * 64, [sub * (l + 1) for l in range(64)], [nrm if l % 2 else -sub * 3 for l in range(64)]]
    names += ["all the smallest subnormal", "subnormals (l + 1) * 2^-1074", "the smallest normal against -3 * 2^-1074"]
    return _f64_rows(rows), names


def _tree_lists():
    oh = hot(0, lambda i: int(np.float64(1.5 + i / 64.0).view(np.uint64)))
    e, en = tree_edges()
    r = tree_random()
    return [oh, _mk("edges", e, en),
            _mk("random", r.view(np.uint64), [f"random doubles, exponents within +-40, one lane cancels the rest, wave {w}" for w in range(len(r))],
                all_shapes=True)]


# ---- ballots: (appending lanes, active lanes) per wave; a lane appends when bit 0 of its value is set

def _bits(lanes):
    m = 0
    for l in lanes:
        m |= 1 << l
    return m


def _mask_rows(masks, junk_seed):
    """values whose bit 0 is the mask's bit of the lane; the other 63 bits are random"""
    j = rand64(junk_seed, len(masks)) & np.uint64(M64 ^ 1)
    b = np.array([[(m >> l) & 1 for l in range(64)] for m in masks], dtype=np.uint64)
    return j | b


def append_masks():
    """256 (mask, name): every lane, none, each single lane, lanes 0 and 63, alternating, random"""
    r = np.random.default_rng(11)
    out = [(1 << i, f"only lane {i} appends") for i in range(64)]
    out += [(ALL_LANES, "every lane appends")] * 48 + [(0, "no lane appends")] * 16
    out += [(_bits([0, 63]), "lanes 0 and 63 append")] * 16
    out += [(_bits(range(0, 64, 2)), "the even lanes append")] * 16 + [(_bits(range(1, 64, 2)), "the odd lanes append")] * 16
    while len(out) < 256:
        m = int(r.integers(0, 1 << 64, dtype=np.uint64))
        out.append((m, f"random lanes {m:#018x} append"))
    return out


def partial_masks(keep_lane0):
    """256 (appending mask, active mask, name): the values ask for the appending mask's lanes, random lanes are active,
    only active lanes can append; lane 0 is inactive in every second wave unless keep_lane0"""
    r = np.random.default_rng(12 + keep_lane0)
    out = []
    for w in range(256):
        asked = ALL_LANES if w % 4 == 0 else int(r.integers(0, 1 << 64, dtype=np.uint64))
        act = int(r.integers(0, 1 << 64, dtype=np.uint64))
        if w % 16 == 5:
            act = 1 << int(r.integers(1, 64))          # one active lane, not lane 0
        if w % 16 == 11:
            act = 0                                    # an idle wavefront
        if keep_lane0:
            act |= 1
        elif w % 2:
            act &= ~1 & M64
        else:
            act |= 1
        out.append((asked, act, f"lanes {asked:#018x} ask to append, lanes {act:#018x} are active"))
    return out


def _ballot_lists(op):
    am = append_masks()
    full = _mk("masks", _mask_rows([m for m, _ in am], 21), [n for _, n in am], all_shapes=True)
    pm = partial_masks(op == "APPEND_ALL")   # wave_append_all: lane 0 is known to be active
    part = _mk("partial", _mask_rows([m for m, _, _ in pm], 22), [n for _, _, n in pm], active=[a for _, a, _ in pm])
    return [full, part]


def _bcast_lists(op):
    lanes = BCAST_LANES_ALL if op == "BCAST_U64" else BCAST_LANES_FEW
    out = _move_lists(37, 31)
    r = np.random.default_rng(32)
    for src in lanes:
        v = np.vstack([_u64([_iota64()]), rand64(400 + src, 7)])
        act = [ALL_LANES] * 4 + [int(r.integers(0, 1 << 64, dtype=np.uint64)) | (1 << src) for _ in range(3)] + [1 << src]
        out.append(_mk(f"source lane {src}", v, [f"source lane {src}, active lanes {a:#018x}" for a in act], src, active=act))
    return out


def lists(op):
    if op in ("SCAN_ADD", "REDUCE_ADD", "SUM_I32", "SUM_U32"):
        return _add32_lists()
    if op.startswith("GROUP_SUM_"):
        return _add32_lists(int(op[len("GROUP_SUM_"):]))
    if op in ("SCAN_MAX", "REDUCE_MAX", "MAX_U32"):
        return _max32_lists(False)
    if op == "MAX_I32":
        return _max32_lists(True)
    if op in ("SCAN_MIN", "REDUCE_MIN"):
        return _min32_lists()
    if op.startswith("SHIFT_DOWN_"):
        return [hot(0, lambda i: HOT32, arg=FILL), _mk("edges", [[l + 1 for l in range(64)]], ["lane l holds l + 1"], FILL),
                random_list(107, 32, FILL), random_list(108, 32, FILL_NEG)]
    if op == "MIN_KEY":
        return _key_lists(True)
    if op == "MAX64":
        return _key_lists(False)
    if op == "SUM64":
        return _sum64_lists()
    if op == "SHFL_XOR64":
        return [l for o in XOR_OFFSETS for l in _move_lists(o, 200 + o)]
    if op in ("BUTTERFLY", "TREE_SHFL"):
        return _tree_lists()
    if op.startswith("DPP_F64_SHL_"):
        return _move_lists(0, 300 + int(op[-1]))
    if op in ("RANK_LEADER", "APPEND", "APPEND_ALL"):
        return _ballot_lists(op)
    if op.startswith("BCAST_"):
        return _bcast_lists(op)
    raise ValueError(op)
