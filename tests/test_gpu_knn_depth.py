"""gv_compute_depth_for_bboxes (k_project_uvd, k_knn_stage1, k_knn_stage2 of gv_knn_pca.hip) held bit for bit to the
plain reference of tests/knn_depth_ref.py at the places where a selection kernel goes wrong and smooth random clouds
never look: equal distances at different depths across the k-th place (the tie rule "lower index wins" is visible only
through the median), every k from 1 to 32, scan orders that defeat the running threshold, runs that overfill a
wavefront's buffer, ragged cloud sizes and fewer candidates than k, the median at every count, non-finite and
overflowing points, degenerate boxes, the same kernels inside gv_tick, and a million points.

cam_lidar is the identity, so camera coordinates are the uploaded ones (tests/test_knn_depth_host.py pins the
reference to the oracle on every scene here and asserts the fixtures' own conditions).  Every comparison is bit-exact
and every call is made three times and must repeat its bytes: this path has no tolerance."""
import time

import numpy as np
import pytest

import knn_depth_ref as R
import oracle_lib as ol
from gvamd import synth
from test_knn_depth_host import camera_frame, lattice_conditions, shell_conditions

pytestmark = pytest.mark.gpu
F32 = np.float32
K = ol.set_intrinsic(synth.FX, synth.FY, synth.CX, synth.CY)
GV_ERR_BAD_ARG = 1
_T0 = time.time()


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    yield m
    print(f"\ntest_gpu_knn_depth: {time.time() - _T0:.1f} s from import to the last test")


def _handle(gvamd):
    h = gvamd.GridVisionHIP(100, 100, 0.5)
    h.set_transforms(R.IDENT_TF, R.IDENT_TF, R.IDENT_TF)
    return h


def _call(h, boxes, k):
    """three calls, the same bytes"""
    depths, d2 = h.compute_depth_for_bboxes(boxes, k)
    for _ in range(2):
        a, b = h.compute_depth_for_bboxes(boxes, k)
        assert a.tobytes() == depths.tobytes() and b.tobytes() == d2.tobytes(), ("not repeatable", k)
    return depths, d2


def _check(h, c, expected=None):
    """upload the case's cloud and hold every k to the reference (or to `expected`: {k: (depths, d2)})"""
    h.upload_xyz(c.x, c.y, c.z)
    ref = expected or R.knn_depth(K, *camera_frame(c), c.boxes, c.ks)
    for k in c.ks:
        depths, d2 = _call(h, c.boxes, k)
        assert np.array_equal(d2, ref[k][1]), (c.tag, k, "distances")
        assert np.array_equal(depths, ref[k][0]), (c.tag, k, "depth")
    return ref


# ------------------------------------------------------------------------------------------------ (a) ties --

def test_lattice_ties_every_k(gvamd):
    """exact-lattice clouds: squared distances are 25 (j'^2 + i'^2 + m^2), so equal distances at different depths are
    everywhere; every k, 200 boxes per k"""
    cases = list(R.lattice_cases())
    queries, ties, differ = lattice_conditions(cases)
    print(f"\nlattice: {ties} of {queries} queries tie across the k-th place, {differ} depths depend on the tie rule")
    with _handle(gvamd) as h:
        for c in cases:
            _check(h, c)


def test_pure_shell_every_k(gvamd):
    """the nearest points are one whole shell of 128 lattice points at 9 depths, repeated and shuffled: the top-k is
    decided by index alone"""
    cases = list(R.shell_cases())
    total, n = shell_conditions(cases)
    print(f"\nshell: the depth depends on the tie rule in {total} of {n} (seed, r, k)")
    with _handle(gvamd) as h:
        for c in cases:
            _check(h, c)


# ----------------------------------------------------------------------------------------- (b) scan orders --

def test_scan_orders(gvamd):
    """one cloud of about 60,000 points in the orders that defeat the threshold: ascending, descending (every point
    beats all earlier ones, every step merges), the k nearest in the first 64 indices, in the last ones, around every
    chunk boundary, around the 64- and 256-index strides, one per (chunk, wavefront) list, and a shuffle"""
    n = 0
    with _handle(gvamd) as h:
        for c in R.scan_cases():
            if c.meta["order"] == "descending":
                u, v, d, _ = R.project(K, *camera_frame(c))
                assert (np.diff(R.distances(u, v, d, c.boxes[0]).astype(np.float64)) < 0).all()
            _check(h, c)
            n += 1
    assert n == 3 + 5 * len(R.SCAN_KS)


# ------------------------------------------------------------------------------------- (c) buffer overflow --

def test_buffer_overflow_runs(gvamd):
    """129 (then 64 .. 5,000) points of equal, winning distance at consecutive indices inside one chunk, with equal and
    with differing depths: one wavefront step admits 64 of them onto a buffer that is not empty.  Then the same with
    falling distance, where the entries that wait in the buffer's second half are the winners."""
    with _handle(gvamd) as h:
        for c in R.overflow_cases():
            ref = _check(h, c)
            lo, hi = c.meta["run"]
            for k in c.ks:
                assert ((ref[k][2] >= lo) & (ref[k][2] < hi)).all(), (c.tag, k)   # the whole top-k inside the run


# ------------------------------------------------------------------------ (d) ragged sizes, few candidates --

@pytest.mark.parametrize("n", R.RAGGED_N)
def test_ragged_sizes_and_few_candidates(gvamd, n):
    """per = ceil(n / 32) leaves the last chunks empty for small n; fewer candidates than k per list, and fewer than k
    overall with cnt even and odd: -1 and inf fills"""
    with _handle(gvamd) as h:
        for c in R.ragged_cases(n):
            ref = _check(h, c)
            if c.meta.get("front") == 0:
                for k in c.ks:
                    assert (ref[k][0] == -1).all() and np.isinf(ref[k][1]).all()


def test_empty_cloud(gvamd):
    """gv_cloud_upload_xyz accepts n = 0: every depth is -1 and every distance inf"""
    e = np.zeros(0, F32)
    with _handle(gvamd) as h:
        _check(h, R.Case("front", [0.1, -0.2], [0.0, 0.1], [3.0, 4.0], R.make_boxes(R.RAGGED_BOXES), (2,)))
        h.upload_xyz(e, e, e)   # raises unless GV_OK
        for k in R.RAGGED_KS:
            depths, d2 = _call(h, R.make_boxes(R.RAGGED_BOXES), k)
            assert (depths == -1).all() and np.isinf(d2).all() and d2.shape == (3, k)


def test_box_counts_and_nothing_stale(gvamd):
    """nb in {0, 1, 2, 300}: the partial lists' buffer grows; then smaller nb and other k on the same handle, k
    alternating between calls: nothing stale leaks from the larger buffer"""
    rng = np.random.default_rng(8)
    j, i, m = R._lattice_draw(rng, 5000)
    x, y, z = R.lattice_xyz(j, i, m)
    boxes = R.lattice_boxes(rng.integers(-40, 41, 300), rng.integers(-30, 31, 300), rng.integers(1, 40, 300),
                            rng.integers(1, 40, 300))
    cam = ol.transform_cloud(ol.tf_to_matrix4f(R.IDENT_TF), x, y, z)
    ref = R.knn_depth(K, *cam, boxes, R.ALL_K)
    with _handle(gvamd) as h:
        h.upload_xyz(x, y, z)
        for nb, k in ((0, 4), (1, 3), (2, 32), (300, 32), (2, 1), (300, 5), (1, 32), (0, 32), (2, 31), (300, 1), (1, 2),
                      (300, 32), (2, 32), (2, 1), (2, 32), (1, 1), (300, 17), (1, 16)):
            depths, d2 = _call(h, boxes[:nb], k)
            assert d2.shape == (nb, k)
            assert np.array_equal(d2, ref[k][1][:nb]), (nb, k)
            assert np.array_equal(depths, ref[k][0][:nb]), (nb, k)
        for k in (0, 33):
            with pytest.raises(gvamd.GVError) as e:
                h.compute_depth_for_bboxes(boxes[:2], k)
            assert e.value.code == GV_ERR_BAD_ARG


# ---------------------------------------------------------------------------------------------- (e) median --

def test_median_every_count(gvamd):
    """neighbour depths with repeated values, all equal, rising and falling in distance order, cnt from 1 to 32, both as
    cnt < k = 32 and as k = cnt: the reference's sorted[cnt // 2]"""
    n = 0
    with _handle(gvamd) as h:
        for c in R.median_cases():
            _check(h, c)
            n += 1
    assert n == 32 * len(R.MEDIAN_PATTERNS) * 2


# ------------------------------------------------------------------------------------------ (f) non-finite --

def test_nonfinite_points_and_degenerate_boxes(gvamd):
    """z of +-0, subnormal, FLT_MIN; NaN and +-inf in each coordinate; u that overflows fp32 (distance +inf: a real
    candidate, and part of the median when fewer than k finite ones exist); FLT_MAX; boxes with a NaN bound (depth -1),
    infinite bounds (every distance +inf: the lowest indices win), inverted, far outside, negative, and with an fp64
    centre that is no fp32 value.  Every k."""
    with _handle(gvamd) as h:
        for c in R.nonfinite_cases():
            ref = _check(h, c)
            if c.tag == "nonfinite-nine":
                for k in range(4, 33):
                    assert np.isinf(ref[k][1][0][3:]).all() and (ref[k][2][0][:min(k, 9)] >= 0).all()


# ------------------------------------------------------------------------------------------------ (g) tick --

@pytest.mark.parametrize("dynamic", [False, True], ids=["static", "one-dynamic"])
@pytest.mark.parametrize("vision", [True, False], ids=["vision", "pca"])
def test_tick_runs_the_same_kernels(gvamd, vision, dynamic):
    """gv_tick on a tie scene and on an overflow scene, k_near in {1, 10, 32}: the static boxes' depths equal the
    reference and base_points_xyz equals gv_convert_pixels_to_3d of them.  Every box static; and, so that the pose
    branch really runs and the kNN goes to its own stream beside it, once more with one dynamic box added."""
    with _handle(gvamd) as h:
        for c in R.tick_cases():
            boxes = c.boxes
            net = None
            if dynamic:
                car = np.zeros(1, synth.BBOX_DTYPE)
                car[0] = (300.0, 220.0, 330.0, 250.0, 0.4, 9)
                boxes = np.concatenate([c.boxes[:3], car, c.boxes[3:]])
                net = synth.network_outputs(1) if vision else None
            st, dy = gvamd.filter_bboxes(boxes)       # which labels are static is that function's business
            assert st.tobytes() == c.boxes.tobytes() and len(dy) == int(dynamic)
            h.upload_xyz(c.x, c.y, c.z)
            ks = (1, 10, 32)
            ref = R.knn_depth(K, *camera_frame(c), st, ks)
            for k in ks:
                r = h.tick(boxes, k_near=k, vision=vision, net=net)
                assert r["n_static"] == len(st) and r["n_dynamic"] == len(dy)
                assert r["static_bboxes"].tobytes() == st.tobytes()
                assert np.array_equal(r["depths"], ref[k][0]), (c.tag, k)
                assert (r["depths"] > 0).all()
                assert r["base_points"].tobytes() == h.convert_pixels_to_3d(st, r["depths"]).tobytes(), (c.tag, k)
                assert np.array_equal(h.compute_depth_for_bboxes(st, k)[0], r["depths"])


# ----------------------------------------------------------------------------------------------- (h) scale --

@pytest.mark.timeout(600)
def test_a_million_points(gvamd):
    """the descending order and the 5,000-point run at 1,000,000 points, k in {10, 32}; expected values from the oracle
    (tests/test_knn_depth_host.py holds the full sort to it at this size too)"""
    with _handle(gvamd) as h:
        for c in R.scale_cases():
            assert len(c.x) == 1_000_000
            u, v, d = ol.project_points(K, *camera_frame(c))
            _check(h, c, {k: ol.depth_for_bboxes(u, v, d, c.boxes, k) for k in c.ks})
