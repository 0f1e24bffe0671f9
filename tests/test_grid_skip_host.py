"""When does a grid pass leave a cell's log-odds as it was, bit for bit?  The tile grid pass does not rewrite a tile
row whose log-odds all came back unchanged, so this decides what it may skip.  With tests/grid_pass_ref.py's
restatement of the update: only at the two clamps, -2.0 (decay, a miss) and 3.6 (a hit or a rectangle), for every
fp32 start in [-2.0, 3.6], k = 0..3 covering rectangles and every hit / miss / counts combination.  No chain of the
adds sums to zero (the smallest, decay + rectangle + miss, is +0.25), and the clamps return a start only to itself."""
import itertools

import numpy as np

import grid_pass_ref as R

F32 = np.float32
U32 = np.uint32
KS = (0, 1, 2, 3)
# counts off (update_map / update_map_poses), or a frame's (hit, miss) of a cell
COMBOS = [(None, None)] + list(itertools.product((False, True), repeat=2))
TAILS = {"none": None, "hit": R.OCC, "miss": R.FREE}


def _tail(hit, miss):
    """the add after decay and rectangles: a hit wins over a miss (grid_pass_ref.cell_update)"""
    return "hit" if hit else ("miss" if miss else "none")


def _update(v, k, hit, miss):
    n = len(v)
    return R.cell_update(v, k, None if hit is None else np.full(n, hit), None if miss is None else np.full(n, miss))


def _same_bits(a, b):
    return np.asarray(a, F32).view(U32) == np.asarray(b, F32).view(U32)


def _stays(clamp, k, tail):
    """the one chain each that holds a cell at a clamp"""
    return (clamp == R.LO and k == 0 and tail != "hit") or (clamp == R.HI and (k > 0 or tail == "hit"))


def _check_chunk_all_combos(v):
    """the restated update itself, every combination: unchanged only at a clamp, and there exactly when expected"""
    for k in KS:
        for hit, miss in COMBOS:
            out = _update(v, k, hit, miss)
            same = _same_bits(out, v)
            at_clamp = (v == R.LO) | (v == R.HI)
            assert not (same & ~at_clamp).any(), (k, hit, miss, v[same & ~at_clamp][:4])
            for c in (R.LO, R.HI):
                m = v == c
                if m.any():
                    assert same[m].all() == _stays(c, k, _tail(hit, miss)), (k, hit, miss, c)


def _fp32_range(lo_bits, hi_bits, step=1 << 24):
    """fp32 values with bit patterns [lo_bits, hi_bits], in chunks"""
    for b0 in range(lo_bits, hi_bits + 1, step):
        yield np.arange(b0, min(b0 + step, hi_bits + 1), dtype=np.int64).astype(U32).view(F32)


def test_examples_of_the_issue():
    v = np.array([-2.0, 3.6], F32)
    assert _same_bits(_update(v[:1], 0, None, None), v[:1]).all()           # unobserved at the floor
    assert _same_bits(_update(v[:1], 0, False, True), v[:1]).all()          # free at the floor
    assert _same_bits(_update(v[1:], 0, True, False), v[1:]).all()          # hit every frame
    assert _same_bits(_update(v[1:], 1, None, None), v[1:]).all()           # under a rectangle
    assert not _same_bits(_update(v[1:], 0, False, True), v[1:]).any()      # the ceiling decays
    assert not _same_bits(_update(v[:1], 0, True, False), v[:1]).any()      # a hit lifts the floor
    # bits, not values: -0.0 and 0.0 are different cells to the comparison, a NaN is itself
    z = np.array([0.0, -0.0], F32)
    assert (z[0] == z[1]) and not _same_bits(z[:1], z[1:]).any()
    n = np.array([0x7FC00001], U32).view(F32)
    assert not (n == n).any() and _same_bits(n, n).all()


def test_every_combination_on_windows_and_a_sample():
    """grid_pass_ref.cell_update as it stands, all 4 x 5 combinations: 2^16 fp32 values at each end of the range and
    around 0, every binade edge, and 2^21 values spread over all fp32 of [-2, 3.6]"""
    w = 1 << 16
    lo_b, hi_b = int(R.LO.view(U32)), int(R.HI.view(U32))
    parts = [np.arange(lo_b - w, lo_b + 1, dtype=np.int64).astype(U32).view(F32),     # up to -2.0 (negative: descending bits)
             np.arange(hi_b - w, hi_b + 1, dtype=np.int64).astype(U32).view(F32),     # up to 3.6
             np.arange(0, w, dtype=np.int64).astype(U32).view(F32),                   # 0 and the subnormals
             (np.arange(0, w, dtype=np.int64) + 0x80000000).astype(U32).view(F32)]    # -0 ...
    edges = np.array([s * 2.0 ** e for e in range(-126, 2) for s in (-1.0, 1.0)], F32)
    parts += [np.nextafter(edges, F32(-np.inf)), edges, np.nextafter(edges, F32(np.inf))]
    n_pos, n_neg = hi_b + 1, lo_b - 0x80000000 + 1
    i = np.linspace(0, n_pos + n_neg - 1, 1 << 21).astype(np.int64)
    parts.append(np.where(i < n_pos, i, i - n_pos + 0x80000000).astype(U32).view(F32))
    v = np.concatenate(parts)
    v = v[(v >= R.LO) & (v <= R.HI)]
    assert (v == R.LO).any() and (v == R.HI).any() and len(v) > (1 << 21)
    _check_chunk_all_combos(v)


def test_sweep_every_fp32_start_between_the_clamps():
    """every fp32 value of [-2.0, 3.6] through the 12 distinct chains of the 20 combinations (counts off, or on with
    neither flag, add nothing after the rectangles; hit and miss together are a hit): the chains are evaluated add by
    add as cell_update does and held to it on the head of every chunk.
    The values below 2^-28 in magnitude are not enumerated (1.6e9 bit patterns): fp32 addition is monotone, both ends
    of that block round to DECAY itself under the first add, so every value in it continues exactly as 0.0 does."""
    tiny = F32(2.0 ** -28)
    ends = np.array([-tiny, tiny, 0.0, -0.0], F32)
    assert _same_bits(ends + R.DECAY, np.full(4, R.DECAY)).all()
    for k in KS:
        for hit, miss in COMBOS:
            out = _update(ends, k, hit, miss)
            assert _same_bits(out, out[2]).all() and (np.abs(out) > tiny).all()     # as from 0.0, and out of the block
    n = unchanged = 0
    tiny_b = int(tiny.view(U32))
    ranges = [(tiny_b, int(R.HI.view(U32))), (0x80000000 + tiny_b, int(R.LO.view(U32)))]
    for b0, b1 in ranges:
        for v in _fp32_range(b0, b1):
            at_clamp = (v == R.LO) | (v == R.HI)
            head = v[:256]
            a = v + R.DECAY
            for k in KS:
                if k:
                    a = a + R.RECT
                for name, c in TAILS.items():
                    out = R.clamp(a if c is None else a + c)
                    same = out.view(U32) == v.view(U32)
                    assert not (same & ~at_clamp).any(), (k, name, v[same & ~at_clamp][:4])
                    unchanged += int(same.sum())
                    hm = {"none": (None, None), "hit": (True, True), "miss": (False, True)}[name]
                    assert _same_bits(out[:256], _update(head, k, *hm)).all()
            n += len(v)
    assert n == (ranges[0][1] - ranges[0][0] + 1) + (ranges[1][1] - ranges[1][0] + 1)
    # -2.0 stays under k = 0 with no add or a miss, 3.6 under every chain with a rectangle or a hit
    assert unchanged == 2 + (len(KS) * len(TAILS) - 2)
    print(f"\n{n} fp32 starts x 12 chains: unchanged only at the clamps ({unchanged} start-chain pairs)")
