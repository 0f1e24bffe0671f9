"""The vision-orientation post-process (k_vision and qr_solve_4x3 of gv_detections.hip) held bit for bit to the plain
reference of tests/vision_ref.py, set by set: the test hook gv_test_vision_sets returns the solution and the residual
of all 64 constraint sets of every box and the set the arg-min chose, so a wrong corner decode, a wrong pivot
permutation or a wrong tie rule shows on the lane where it happens and not only when that lane wins.

The device's contract: the six trig values are evaluated in fp64 and rounded once, everything else is the reference's
fp32 operation order, and the lowest set index wins on equal residuals.  Every comparison is against trig="fp64" with
zero tolerance -- finite values and infinities by their bytes, NaN by class -- and every call is made three times and
must repeat its bytes.  tests/test_vision_host.py pins the same reference to the oracle on every scene used here and
asserts what the scenes reach: the four corner-multiplier branches, alpha on and next to every threshold, the six
pivot patterns, rank 2, the small-tail and the down-date branch of the QR, 4-, 16- and 64-way ties of the minimum,
boxes without any finite residual."""
import time

import numpy as np
import pytest

import vision_ref as R
from gvamd import synth

pytestmark = pytest.mark.gpu
_T0 = time.time()
POSE7 = ("px", "py", "pz", "qx", "qy", "qz", "qw")


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    yield m
    print(f"\ntest_gpu_vision: {time.time() - _T0:.1f} s from import to the last test")


def _handle(gvamd, cam=0):
    """the small grid of the call-site tests, 50 m x 20 m at 0.25 m, with camera `cam` of vision_ref.CAMS"""
    fx, fy, cx, cy = R.CAMS[cam]
    h = gvamd.GridVisionHIP(50, 20, 0.25, fx=fx, fy=fy, cx=cx, cy=cy, image_w=R.IMG_W, image_h=R.IMG_H)
    tfs = synth.transforms()
    h.set_transforms(tfs["cam_lidar"], tfs["base_cam"], tfs["base_lidar"])
    return h


def _sets(h, sc, sl=slice(None)):
    """three calls, the same bytes"""
    args = (sc.orient[sl], sc.conf[sl], sc.dims[sl], sc.boxes[sl])
    sets, winner = h.vision_sets(*args)
    poses = h.vision_post_process(*args)
    for _ in range(2):
        s2, w2 = h.vision_sets(*args)
        p2 = h.vision_post_process(*args)
        assert s2.tobytes() == sets.tobytes() and w2.tobytes() == winner.tobytes(), (sc.tag, "sets not repeatable")
        assert p2.tobytes() == poses.tobytes(), (sc.tag, "poses not repeatable")
    return sets, winner, poses


def _check(h, sc, sl=slice(None)):
    """all 64 sets, the winner and the emitted poses of scene `sc` (or its slice) against the reference"""
    ref = R.reference(sc)
    sets, winner, poses = _sets(h, sc, sl)
    idx = np.arange(len(sc.boxes))[sl]
    want = np.concatenate([ref.loc[idx], ref.err[idx][..., None]], -1)
    ok = R.same_class_or_bytes(sets, want)
    if not ok.all():
        i, lane, f = (int(v[0]) for v in np.nonzero(~ok))
        pytest.fail(f"{sc.tag}: box {idx[i]} {sc.boxes[idx[i]]} lane {lane} field {f}: device {sets[i, lane]!r} reference "
                    f"{want[i, lane]!r}; {int((~ok.all(-1)).sum())} sets of {int((~ok.all((1, 2))).sum())} boxes differ; "
                    f"alpha {ref.alpha[idx[i]]!r} theta {ref.theta_ray[idx[i]]!r} pivots {ref.pivots[idx[i]]} "
                    f"rank {ref.rank[idx[i]]}")
    assert np.array_equal(winner, ref.winner[idx]), (sc.tag, "winner", np.flatnonzero(winner != ref.winner[idx])[:8])
    first = int(ref.valid[:idx[0]].sum()) if len(idx) else 0
    want_poses = ref.poses[first:first + int(ref.valid[idx].sum())]
    eq = R.poses_equal(poses, want_poses)
    assert len(poses) == len(want_poses) and eq.all(), (sc.tag, "poses", len(poses), len(want_poses), np.flatnonzero(~eq)[:8])
    return sets, winner, poses


# ------------------------------------------------------------------------------------- (a) boxes x cameras --

@pytest.mark.parametrize("cam", range(len(R.CAMS)))
def test_edge_boxes_every_camera(gvamd, cam):
    """the twelve edge boxes (zero area, zero width, zero height, inverted, far outside, one pixel) under every label,
    on the four cameras that together take all six pivot patterns, rank 2 and both rare QR branches; then 40
    ordinary boxes on the same camera"""
    with _handle(gvamd, cam) as h:
        _check(h, R.edge_scene(cam))
        _check(h, R.random_scene(cam, 40, 30 + cam))


# ------------------------------------------------------------------------------------------ (b) thresholds --

def test_alpha_canaries(gvamd):
    """alpha exactly on -92, -90, -88 and 0 degrees and on the nearest values computeAlpha can return on either side of
    all seven thresholds, in both bins; orientation pairs off the unit circle, (+-0, +-0) and equal confidences"""
    found, missing = R.canaries()
    assert found and not missing
    with _handle(gvamd) as h:
        _check(h, R.canary_scene())


def test_box_centre_on_the_image_centre(gvamd):
    """theta_ray's sign: the box centre on orig_w / 2, one ulp left and one ulp right of it"""
    with _handle(gvamd) as h:
        _check(h, R.centre_scene())


# ------------------------------------------------------------------------------------------ (c) non-finite --

def test_nonfinite_inputs_leave_neighbours_alone(gvamd):
    """NaN and +-Inf in one field at a time, a negative length, boxes of a million pixels, each between good boxes:
    location 0 where no residual is below FLT_MAX, valid / dims / orientation as the reference says; the good boxes'
    sets and poses are the bytes they have in a batch of their own"""
    sc, good = R.nonfinite_scene()
    ref = R.reference(sc)
    none = ref.winner == 64
    assert none.sum() >= 10 and (ref.best_loc[none] == 0).all()
    with _handle(gvamd) as h:
        sets, winner, poses = _check(h, sc)
        alone = R.scene("nonfinite-good", sc.cam, sc.orient[good], sc.conf[good], sc.dims[good], sc.boxes[good])
        s2, w2, p2 = _check(h, alone)
        assert sets[good].tobytes() == s2.tobytes() and winner[good].tobytes() == w2.tobytes()
        emitted = np.cumsum(ref.valid) - 1                      # index of box i in the emitted list
        assert ref.valid[good].all() and poses[emitted[good]].tobytes() == p2.tobytes()


# ----------------------------------------------------------------------------------------- (d) batch sizes --

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 200])
def test_batch_sizes_on_a_fresh_handle(gvamd, n):
    """the shared output buffer starts at 64 boxes and grows to n + n / 4"""
    sc = R.random_scene(0, 200, 40)
    with _handle(gvamd) as h:
        sets, winner, poses = _check(h, sc, slice(0, n))
        assert sets.shape == (n, 64, 4) and winner.shape == (n,)


def test_large_batch_then_small(gvamd):
    """200 boxes, then 5 others, then 65, on one handle: nothing stale from the larger call"""
    sc = R.random_scene(0, 200, 40)
    with _handle(gvamd) as h:
        _check(h, sc)
        _check(h, sc, slice(100, 105))
        _check(h, sc, slice(3, 68))
        _check(h, R.centre_scene())


# ------------------------------------------------------------------------------------- (e) the call sites --

def _call_site_scene():
    """the default camera's edge boxes and the non-finite batch as one detection set"""
    a, b = R.edge_scene(0), R.nonfinite_scene()[0]
    return R.scene("edges+nonfinite", 0, *(np.concatenate([getattr(a, k), getattr(b, k)]) for k in ("orient", "conf", "dims", "boxes")))


def test_frame_vision_orient_layers(gvamd):
    """process_frame(FRAME_VISION_ORIENT) with the edge batch: the three layers equal those of a second handle fed
    update_map_poses(transform_lshape_objects(reference poses))"""
    sc = _call_site_scene()
    ref = R.reference(sc)
    with _handle(gvamd) as hA, _handle(gvamd) as hB:
        base = hB.transform_lshape_objects(ref.poses)
        hB.update_map_poses(base)
        hB.synchronize()
        x, y, z, _ = synth.cloud_uniform(1, 1000)
        hA.upload_xyz(x, y, z)
        hA.process_frame(gvamd.FRAME_VISION_ORIENT, bboxes=sc.boxes, net=(sc.orient, sc.conf, sc.dims))
        lo = hB.log_odds()
        assert np.count_nonzero(lo > 0) > 20, "fixture: the poses mark cells of the map"
        assert hA.log_odds().tobytes() == lo.tobytes()
        assert hA.occupancy().tobytes() == hB.occupancy().tobytes()
        assert hA.to_occupancy_grid()[0].tobytes() == hB.to_occupancy_grid()[0].tobytes()


def test_tick_vision_poses(gvamd):
    """tick(vision=True) on the batch: the dynamic boxes' poses are the bytes of the standalone call's, moved to the base
    frame, and the reference's"""
    sc = _call_site_scene()
    st, dy = gvamd.filter_bboxes(sc.boxes)
    dyn = np.array([int(l) in R.CLASS_DIMS for l in sc.boxes["label"]])
    assert dy.tobytes() == sc.boxes[dyn].tobytes() and len(st) > 0
    net = (sc.orient[dyn], sc.conf[dyn], sc.dims[dyn])
    ref = R.reference(sc)
    with _handle(gvamd) as h:
        x, y, z, _ = synth.cloud_uniform(1, 1000)
        h.upload_xyz(x, y, z)
        alone = h.transform_lshape_objects(h.vision_post_process(*net, dy))
        want = h.transform_lshape_objects(ref.poses)
        assert len(alone) == len(dy) == len(want) and R.poses_equal(alone, want).all()
        for _ in range(3):
            r = h.tick(sc.boxes, k_near=4, vision=True, net=net)
            assert r["n_dynamic"] == len(dy) and r["n_static"] == len(st)
            assert r["poses"].tobytes() == alone.tobytes()
