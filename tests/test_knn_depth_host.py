"""The two CPU implementations of buildKDTree + computeDepthForBoundingBoxes pinned to each other, and the conditions
the kNN fixtures must meet (tests/knn_depth_ref.py).

knn_depth_ref sorts every candidate on (distance, index); the oracle keeps k of them by a stable insertion.  On every
scene family tests/test_gpu_knn_depth.py runs they agree bit for bit, in distances and depth; the device suite rests
on both.  The fixture conditions are asserted here from the reference alone (and, for the buffer's overflow half, from
its model of today's scan), so that a generator which stops producing ties or stops overfilling a buffer fails on the
CPU instead of silently weakening the GPU test."""
import numpy as np
import pytest

import knn_depth_ref as R
import oracle_lib as ol
from gvamd import synth

F32 = np.float32
K = ol.set_intrinsic(synth.FX, synth.FY, synth.CX, synth.CY)


def camera_frame(c):
    """row A1 under the identity transform: an infinite coordinate times a zero matrix entry gives NaN"""
    return ol.transform_cloud(ol.tf_to_matrix4f(R.IDENT_TF), c.x, c.y, c.z)


def check_against_oracle(c):
    cam = camera_frame(c)
    ref = R.knn_depth(K, *cam, c.boxes, c.ks)
    u, v, d = ol.project_points(K, *cam)
    for k in c.ks:
        od, od2 = ol.depth_for_bboxes(u, v, d, c.boxes, k)
        assert not np.isnan(ref[k][0]).any() and not np.isnan(ref[k][1]).any(), (c.tag, k)
        assert ref[k][1].tobytes() == od2.tobytes(), (c.tag, k, "distances")
        assert ref[k][0].tobytes() == od.tobytes(), (c.tag, k, "depth")
    return ref


FAMILIES = {"lattice": R.lattice_cases, "shell": R.shell_cases, "scan": R.scan_cases, "overflow": R.overflow_cases,
            "median": R.median_cases, "nonfinite": R.nonfinite_cases, "scale": R.scale_cases, "tick": R.tick_cases}


def test_camera_and_identity():
    assert np.array_equal(K, R.K_SYNTH)
    assert np.array_equal(ol.tf_to_matrix4f(R.IDENT_TF).reshape(4, 4), np.eye(4, dtype=F32))
    st, dy = ol.filter_bboxes(R.make_boxes([(0.0, 0.0, 1.0, 1.0)]))
    assert len(st) == 1 and len(dy) == 0


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_reference_equals_oracle(family):
    n = 0
    for c in FAMILIES[family]():
        check_against_oracle(c)
        n += 1
    assert n > 0


@pytest.mark.parametrize("n", R.RAGGED_N)
def test_reference_equals_oracle_ragged(n):
    for c in R.ragged_cases(n):
        check_against_oracle(c)
        if "front" in c.meta:
            assert len(R.project(K, *camera_frame(c))[0]) == c.meta["front"]


def test_reference_equals_oracle_empty_cloud():
    e = np.zeros(0, F32)
    check_against_oracle(R.Case("empty", e, e, e, R.make_boxes(R.RAGGED_BOXES), R.RAGGED_KS))


# ----------------------------------------------------------------------------------------- fixture conditions --

def lattice_conditions(cases):
    """3(a), shared with the GPU test: exact projection, >= 30 % of the (box, k) queries tie across the k-th place,
    >= 20 queries whose depth depends on the tie rule, every k has at least 200 boxes.  Returns the figures."""
    queries = ties = differ = 0
    boxes_per_k = {k: 0 for k in R.ALL_K}
    for c in cases:
        j, i, m = c.meta["jim"]
        u, v, d, idx = R.project(R.K_SYNTH, c.x, c.y, c.z)
        assert len(idx) == len(c.x)
        assert np.array_equal(u, (5 * j + 320).astype(F32)) and np.array_equal(v, (5 * i + 240).astype(F32))
        assert np.array_equal(d, (5 * m).astype(F32))
        lower, higher, kth = R.tie_stats(c)
        for k in c.ks:
            boxes_per_k[k] += len(c.boxes)
            queries += len(c.boxes)
            ties += int(kth[k].sum())
            differ += int((lower[k][0] != higher[k][0]).sum())
            r = lower[k][1]
            assert np.array_equal(r, np.round(r / 25) * 25) and np.isfinite(r).all()   # 25 (j'^2 + i'^2 + m^2)
    assert min(boxes_per_k.values()) >= 200 and sorted(boxes_per_k) == list(range(1, 33))
    assert ties >= 0.30 * queries, (ties, queries)
    assert differ >= 20, differ
    return queries, ties, differ


def shell_conditions(cases):
    """3(a) pure shell, shared with the GPU test: the depth depends on the tie rule for >= 4 of the 32 k in every
    (seed, r) and for >= a quarter of all (seed, r, k)"""
    total = n = 0
    for c in cases:
        lower, higher, _ = R.tie_stats(c)
        differ = sum(int(lower[k][0][0] != higher[k][0][0]) for k in c.ks)
        assert len(c.ks) == 32 and differ >= 4, (c.tag, differ)
        d2 = lower[32][1][0]
        assert (d2 == F32(25 * R.SHELL)).all()            # the whole top-k lies on the shell: index alone decides
        total += differ
        n += len(c.ks)
    assert 4 * total >= n, (total, n)
    return total, n


def test_lattice_fixture_conditions():
    queries, ties, differ = lattice_conditions(list(R.lattice_cases()))
    print(f"lattice: {ties} of {queries} queries tie across the k-th place, {differ} depend on the tie rule")


def test_shell_fixture_conditions():
    j, i, m = R.shell_jim()
    assert len(j) == 128 and len(set(m.tolist())) == 9
    cases = list(R.shell_cases())
    assert {(c.meta["seed"], c.meta["rep"]) for c in cases} == {(s, r) for s in (1, 2, 3, 4) for r in (1, 3)}
    total, n = shell_conditions(cases)
    print(f"shell: the depth depends on the tie rule in {total} of {n} (seed, r, k)")


def test_scan_fixture_conditions():
    base = R.scan_base()
    n = len(base.x)
    per = R.chunk_len(n)
    assert 59_000 <= n <= 61_000
    seen = set()
    for c in R.scan_cases(base):
        assert len(c.x) == n
        order = c.meta["order"]
        seen.add(order)
        u, v, d, idx = R.project(R.K_SYNTH, c.x, c.y, c.z)
        r = R.distances(u, v, d, c.boxes[0])
        assert not np.isnan(r).any() and 0.85 * n < len(r) < 0.95 * n   # a tenth of the cloud is behind the camera
        if order == "descending":
            assert (np.diff(r.astype(np.float64)) < 0).all()   # every point beats all earlier ones: every step merges
        elif order == "ascending":
            assert (np.diff(r.astype(np.float64)) > 0).all()
        elif order != "shuffle":
            (k,) = c.ks
            at = np.sort(R.knn_depth(R.K_SYNTH, c.x, c.y, c.z, c.boxes[:1], k)[k][2][0])
            assert len(at) == k
            if order == "first64":
                assert at[-1] < 64
            elif order == "last":
                assert at[0] == n - k
            elif order == "chunk-edges":
                assert (np.minimum(at % per, per - at % per) <= 1).all()
            elif order == "strides":
                assert (np.minimum((at % per) % 64, 64 - (at % per) % 64) <= 1).all()
            else:
                lists = {(a // per, ((a % per) % 256) // 64) for a in at.tolist()}
                assert order == "one-per-list" and len(lists) == k
    assert seen == {"ascending", "descending", "shuffle", "first64", "last", "chunk-edges", "strides", "one-per-list"}


def test_overflow_fixture_conditions():
    """the reference places the whole top-k inside the run; the run is consecutive, inside one chunk and starts in the
    middle of a wavefront's 64 indices; under today's scan it overfills a buffer, and leaving the overflow half behind
    changes what a caller sees on the fixtures named below"""
    cases = list(R.overflow_cases())
    assert sorted({c.meta["run"][1] - c.meta["run"][0] for c in cases}) == sorted(R.RUNS)
    bites = set()
    for c in cases:
        lo, hi = c.meta["run"]
        per = R.chunk_len(len(c.x))
        assert hi - lo >= 64 and lo // per == (hi - 1) // per and (lo % per) % 64 not in (0, 63)
        ref = R.knn_depth(R.K_SYNTH, c.x, c.y, c.z, c.boxes, c.ks)
        for k in c.ks:
            at = ref[k][2][0]
            assert ((at >= lo) & (at < hi)).all(), (c.tag, k)
            if "ramp" in c.tag:
                assert np.array_equal(at, np.arange(hi - 1, hi - 1 - k, -1))
            else:
                assert np.array_equal(at, np.arange(lo, lo + k)) and len(set(ref[k][1][0].tolist())) == 1
        if "equal" in c.tag:
            assert len(set(c.z[lo:hi].tolist())) == 1
        elif hi - lo >= 65:
            assert len(set(c.z[lo:hi].tolist())) >= 8
        k = 32
        keys, max_fill, over = R.scan_model(R.K_SYNTH, c.x, c.y, c.z, c.boxes[0], k)
        assert np.array_equal(keys[:, 1], ref[k][2][0]) and np.array_equal(keys[:, 0].astype(F32), ref[k][1][0])
        assert max_fill > 64 and over >= 64, (c.tag, max_fill, over)
        left, _, _ = R.scan_model(R.K_SYNTH, c.x, c.y, c.z, c.boxes[0], k, move_rest=False)
        depth = np.sort(c.z[left[:, 1].astype(np.int64)])[len(left) // 2]
        if depth != ref[k][0][0] or not np.array_equal(left[:, 0].astype(F32), ref[k][1][0]):
            bites.add(c.tag)
    assert {"overflow-ramp-129", "overflow-ramp-256", "overflow-shell-5000"} <= bites, bites


def test_scan_model_equals_reference():
    """the model of today's scan finds the reference's neighbours on the scan orders too (it is only ever used for
    fixture conditions, but a wrong model would make those worthless), and they overfill buffers as well"""
    base = R.scan_base()
    for c in R.scan_cases(base):
        if c.meta["order"] not in ("descending", "ascending", "shuffle", "one-per-list"):
            continue
        k = c.ks[-1]
        ref = R.knn_depth(R.K_SYNTH, c.x, c.y, c.z, c.boxes[:2], k)
        for b in (0, 1):
            keys, max_fill, over = R.scan_model(R.K_SYNTH, c.x, c.y, c.z, c.boxes[b], k)
            assert np.array_equal(keys[:, 1], ref[k][2][b]) and np.array_equal(keys[:, 0].astype(F32), ref[k][1][b])
            assert max_fill > 64 and over > 0, (c.tag, b, max_fill, over)


def test_median_fixture_conditions():
    seen = set()
    for c in R.median_cases():
        cnt, pat = c.meta["cnt"], c.meta["pattern"]
        (k,) = c.ks
        ref = R.knn_depth(R.K_SYNTH, c.x, c.y, c.z, c.boxes, k)[k]
        want = c.meta.get("near", np.arange(cnt))
        assert np.array_equal(ref[2][0][:cnt], want) and (ref[2][0][cnt:] == -1).all()   # nearest first, as laid out
        dep = c.z[ref[2][0][:cnt]].astype(np.float64)
        step = np.diff(dep)
        assert {"increasing": (step > 0).all(), "decreasing": (step < 0).all(), "equal": (step == 0).all(),
                "repeated": cnt < 4 or (len(set(dep.tolist())) == 3 and (step > 0).any() and (step < 0).any())}[pat]
        assert ref[0][0] == np.sort(c.z[ref[2][0][:cnt]])[cnt // 2]
        seen.add((cnt, pat, k == 32))
    assert len(seen) == 32 * 4 * 2 - 4   # cnt = 32 "among" has k = 32 too


def test_nonfinite_fixture_conditions():
    sprinkled, alone, nine = R.nonfinite_cases()
    cam = camera_frame(alone)
    assert np.isnan(cam[0]).sum() >= 6 and np.isnan(cam[2]).sum() >= 6    # inf times a zero matrix entry
    u, v, d, idx = R.project(K, *cam)
    assert np.isnan(d).any()                                             # a NaN z passes `z <= 0`
    assert (alone.z[:2] == 0).all() and not np.isin([0, 1], idx).any()   # +0.0 and -0.0 do not
    assert np.isin([2, 3, 4, 5, 6, 7, 8], idx).all()                     # subnormal, FLT_MIN and 1e-30 do
    r = R.distances(u, v, d, alone.boxes[0])
    assert np.isinf(r).sum() >= 8 and np.isnan(r).sum() >= 6 and np.isfinite(r).sum() >= 6
    ref = R.knn_depth(K, *cam, alone.boxes, 32)[32]
    nb = len(R.NONFINITE_BOXES)
    assert (ref[0][1:3] == -1).all() and np.isinf(ref[1][1:3]).all() and (ref[2][1:3] == -1).all()   # a NaN bound
    assert (ref[0][5:7] == -1).all() and (ref[2][5:7] == -1).all()                                     # inf - inf
    for b in (3, 4, 7):   # an infinite centre: every candidate is +inf away, the lowest indices win
        cand = idx[~np.isnan(R.distances(u, v, d, alone.boxes[b]))]
        assert np.array_equal(ref[2][b][:len(cand)], cand[:32]) and np.isinf(ref[1][b]).all() and ref[0][b] > 0
    assert R.centre(16777216.0, 16777219.0) == F32(16777218.0)           # 16777217.5: one narrowing, to even
    assert R.centre(50.1, 70.7000001) != F32(F32(50.1) + (F32(70.7000001) - F32(50.1)) / F32(2))   # all-fp32 is one ulp off
    assert len(alone.boxes) == nb + 3
    # the nine-point cloud: 3 finite-distance and 6 inf-distance candidates; the latter enter the median
    cam = camera_frame(nine)
    ref = R.knn_depth(K, *cam, nine.boxes[:1], R.ALL_K)
    moved = 0
    for k in R.ALL_K:
        d2, at = ref[k][1][0], ref[k][2][0]
        cnt = min(k, 9)
        assert (at[:cnt] >= 0).all() and np.isfinite(d2[:min(cnt, 3)]).all() and np.isinf(d2[3:]).all()
        finite_only = np.sort(nine.z[at[:min(cnt, 3)]])
        moved += int(ref[k][0][0] != finite_only[len(finite_only) // 2])
    assert moved >= 20, moved
