"""The wavefront primitives of csrc/gv_wave.hpp, lane by lane, against the plain references of tests/wave_ref.py: every
helper, in every instantiation the header offers, runs on the device through the probe kernel k_test_wave (test hook
gv_test_wave, csrc/gv_test_wave.hip) over the lists of tests/wave_cases.py -- which tests/test_wave_ref_host.py proves to
single out every lane, to reach the identities, ties, wraps and carries, and to tell the orders of the tree's additions
apart -- and is compared bit for bit.  No tolerances.  Every list runs with 256 threads to a workgroup, the one-hot and
random lists also with 64 and 1024: a wavefront's result does not depend on which wavefront of its workgroup it is.
The appends are held to their properties (the order of the wavefronts at the counter is free), the trees to lane 0 (all
the header promises) and to each other.  A failure names the op, what the wave holds, the lane, and got / want in hex.
An idiom swap between two forms of gv_wave.hpp must keep this file green."""
import ctypes as C

import numpy as np
import pytest

import wave_cases as wc
import wave_ref as wr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    import gvamd
    h = gvamd.GridVisionHIP(20, 20, 0.5)
    yield h
    h.close()


def _shapes(lst):
    return wc.SHAPES if lst.all_shapes else (256,)


def _complain(op, lst, threads, out, want, care):
    """the first differing lane that the reference cares about, named"""
    bad = (out != want) & care
    if not bad.any():
        return None
    w, l = (int(x) for x in np.argwhere(bad)[0])
    return (f"{op} (arg {lst.arg:#x}, {threads} threads, list '{lst.name}'): {int(bad.sum())} lanes differ, first: wave {w} "
            f"[{lst.names[w]}] lane {l}: got {int(out[w, l]):#018x} want {int(want[w, l]):#018x}\n"
            f"  in   {[hex(int(x)) for x in lst.values[w]]}\n  got  {[hex(int(x)) for x in out[w]]}\n"
            f"  want {[hex(int(x)) for x in want[w]]}")


def _run_exact(handle, op):
    for lst in wc.lists(op):
        want, care = wr.expected(op, lst.values, lst.active, lst.arg)
        for threads in _shapes(lst):
            out, counter = handle.test_wave(op, lst.values, lst.active, lst.arg, threads)
            msg = _complain(op, lst, threads, out, want, care)
            assert msg is None, msg
            assert counter == 0, f"{op}: the append counter moved ({counter}) under an op that does not append"


@pytest.mark.parametrize("op", wc.FAMILIES["dpp_scans"])
def test_dpp_scans(handle, op):
    """wave_scan / wave_reduce<OpAdd, OpMax, OpMin>, wave_shift_down<1, 2, 4, 8> (the top H lanes read the fill),
    group_sum<8> (no kernel of the product instantiates it) and <16>, also with whole groups of the wavefront inactive (how
    k_radius_sorted calls it), wave_min_key: every lane"""
    _run_exact(handle, op)


@pytest.mark.parametrize("op", wc.FAMILIES["xor_butterflies"])
def test_xor_butterflies(handle, op):
    """wave_sum / wave_max<int, unsigned>, wave_max64, wave_sum64, shfl_xor64 for o = 1 .. 32 and 37: every lane"""
    _run_exact(handle, op)


@pytest.mark.parametrize("op", wc.FAMILIES["dpp_wrappers"])
def test_dpp_wrappers(handle, op):
    """dpp_f64<row_shl:1, 2, 4, 8>: the bits of lane + k inside the row of 16, +0.0 from outside it"""
    _run_exact(handle, op)


@pytest.mark.parametrize("op", wc.FAMILIES["trees"])
def test_fixed_order_trees(handle, op, record_property):
    """wave_butterfly / wave_tree_sum_shfl: lane 0 by bits against the tree t[:off] += t[off:2*off], off = 32 .. 1 (a NaN
    where the reference is a NaN, whatever its payload).  The other lanes hold partial sums the header promises nothing
    about: they are recorded (the first wave of each list as a property of the test's report, the failing wave in a
    failure's text), not asserted."""
    for lst in wc.lists(op):
        want, care = wr.expected(op, lst.values, lst.active, lst.arg)
        nan = wr.nan_lanes(op, lst.values)
        for threads in _shapes(lst):
            out, _ = handle.test_wave(op, lst.values, lst.active, lst.arg, threads)
            if threads == 256:
                record_property(f"{op} '{lst.name}' wave 0 lanes 0..63", " ".join(f"{int(x):016x}" for x in out[0]))
            msg = _complain(op, lst, threads, out, want, care)
            assert msg is None, msg
            got_nan = np.isnan(out[:, 0].copy().view(np.float64))
            assert np.array_equal(got_nan[nan], np.ones(int(nan.sum()), bool)), \
                f"{op} ({threads} threads, list '{lst.name}'): lane 0 is no NaN in waves {np.flatnonzero(nan & ~got_nan)}"


def test_tree_twins_agree_in_lane_0(handle):
    """the DPP form and the shuffle form of the one tree leave the same bits in lane 0, on every wave of every list"""
    for a, b in zip(wc.lists("BUTTERFLY"), wc.lists("TREE_SHFL")):
        oa, _ = handle.test_wave("BUTTERFLY", a.values)
        ob, _ = handle.test_wave("TREE_SHFL", b.values)
        both_nan = np.isnan(oa[:, 0].copy().view(np.float64)) & np.isnan(ob[:, 0].copy().view(np.float64))
        bad = np.flatnonzero((oa[:, 0] != ob[:, 0]) & ~both_nan)
        assert len(bad) == 0, (f"list '{a.name}': wave {bad[0]} [{a.names[bad[0]]}] lane 0: wave_butterfly "
                               f"{int(oa[bad[0], 0]):#018x}, wave_tree_sum_shfl {int(ob[bad[0], 0]):#018x}")


@pytest.mark.parametrize("op", ["RANK_LEADER", "BCAST_U64", "BCAST_I32", "BCAST_F64"])
def test_rank_leader_bcast(handle, op):
    """wave_rank + wave_leader over __ballot(in & 1) and wave_bcast<unsigned long long, int, double> from every source
    lane, exactly, also with some lanes inactive"""
    _run_exact(handle, op)


@pytest.mark.parametrize("op", ["APPEND", "APPEND_ALL"])
def test_appends(handle, op):
    """wave_append (any subset of the lanes active, lane 0 inactive in half of the partial waves) and wave_append_all (lane
    0 active), 256 wavefronts to one counter: wave_ref.check_append's properties"""
    for lst in wc.lists(op):
        for threads in _shapes(lst):
            out, counter = handle.test_wave(op, lst.values, lst.active, lst.arg, threads)
            bad = wr.check_append(op, lst.values, lst.active, out, counter)
            assert not bad, f"{op} ({threads} threads, list '{lst.name}'): {len(bad)} complaints, first:\n  " + "\n  ".join(
                b + (f" [{lst.names[int(b.split('wave ')[1].split()[0])]}]" if "wave " in b else "") for b in bad[:6])


def test_argument_rules(handle):
    """GV_ERR_BAD_ARG and nothing launched (out and the counter keep what they held) for: a null pointer; n_waves, threads,
    op or arg out of range; a partial mask under an op defined for a full wavefront; a partly active group under group_sum; an
    inactive source lane; lane 0 inactive under wave_append_all.  The same arguments made right are accepted."""
    lib, h = handle._lib, handle._h
    v = np.arange(128, dtype=np.uint64).reshape(2, 64)
    full = np.full(2, wr.ALL_LANES, np.uint64)
    p = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731

    def call(op, arg=0, threads=256, values=v, active=full, n=2, out_null=False, cnt_null=False):
        out, cnt = np.full((2, 64), 0x77, np.uint64), C.c_uint32(0x77)
        rc = lib.gv_test_wave(h, C.c_int32(wc.OPS.index(op) if isinstance(op, str) else op), C.c_int32(arg), C.c_int32(threads),
                              p(values) if values is not None else None, p(active) if active is not None else None,
                              C.c_int64(n), None if out_null else p(out), None if cnt_null else C.byref(cnt))
        if rc:
            assert (out == 0x77).all() and cnt.value == 0x77, "a refused call wrote its outputs"
        return rc
    assert call("SCAN_ADD") == 0
    assert call("SCAN_ADD", values=None) == 1 and call("SCAN_ADD", active=None) == 1
    assert call("SCAN_ADD", out_null=True) == 1 and call("SCAN_ADD", cnt_null=True) == 1
    assert call("SCAN_ADD", n=0) == 1 and call("SCAN_ADD", n=-1) == 1 and call("SCAN_ADD", n=4097) == 1
    for t in (0, 32, 128, 512, 2048, -64):
        assert call("SCAN_ADD", threads=t) == 1, t
    assert call(-1) == 1 and call(len(wc.OPS)) == 1
    assert call("SHFL_XOR64", arg=0) == 1 and call("SHFL_XOR64", arg=64) == 1 and call("SHFL_XOR64", arg=63) == 0
    for op in ("BCAST_U64", "BCAST_I32", "BCAST_F64"):
        assert call(op, arg=-1) == 1 and call(op, arg=64) == 1 and call(op, arg=63) == 0
        assert call(op, arg=5, active=np.array([wr.ALL_LANES, wr.ALL_LANES ^ (1 << 5)], np.uint64)) == 1
        assert call(op, arg=5, active=np.array([wr.ALL_LANES, 1 << 5], np.uint64)) == 0
    part = np.array([wr.ALL_LANES, wr.ALL_LANES ^ (1 << 63)], np.uint64)
    for op in wc.OPS:   # lane 63 off: also a group of group_sum broken
        assert call(op, arg=1, active=part) == (0 if all(wr.mask_ok(op, a, 1) for a in part) else 1), op
    assert not wr.mask_ok("GROUP_SUM_8", part[1]) and not wr.mask_ok("SCAN_ADD", part[1]) and wr.mask_ok("APPEND", part[1])
    rows = np.array([0xFFFF00000000FF00, 0], np.uint64)       # whole groups of 8: group_sum<8> takes it, <16> does not
    assert call("GROUP_SUM_8", active=rows) == 0 and call("GROUP_SUM_16", active=rows) == 1 and call("SUM_U32", active=rows) == 1
    assert call("GROUP_SUM_16", active=np.array([0xFFFF00000000FFFF, wr.ALL_LANES], np.uint64)) == 0
    no0 = np.array([wr.ALL_LANES, wr.ALL_LANES ^ 1], np.uint64)
    assert call("APPEND_ALL", active=no0) == 1 and call("APPEND", active=no0) == 0 and call("RANK_LEADER", active=no0) == 0
