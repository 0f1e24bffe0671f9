"""The RANSAC ground plane (k_ransac_count_all -> k_ransac_moments -> k_ransac_mask, gv_ransac.hip, and the ground test fused into
k_pose_classify; gv_cloudops.hip) held to tests/ransac_ref.py with NO tolerance on the fixtures of tests/ransac_cases.py,
which tests/test_ransac_host.py proves to reach their edges: through the test hook gv_test_ransac_state the winner's count
as the counting pass left it (best_count), the sampled plane's 16 bytes, the inlier count of the moments pass (m, always
equal to best_count), the refined plane's 16 bytes, n_inliers and the mask byte for byte.  Every call is made three times
and must repeat its bytes.

Fixtures B and D, and E at 65 and 4097 points, also go through gv_compute_bbox_pose_ground_removed (the hook's flag):
the same state, and the selected points of gv_test_bbox_pose_nodes equal the reference's non-ground points as
tests/pose_ref.py classifies them.  B goes once through gv_tick's PCA branch."""
import time

import numpy as np
import pytest

import pose_ref as P
import ransac_cases as RC
from gvamd import synth

pytestmark = pytest.mark.gpu
_T0 = time.time()


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    yield m
    print(f"\ntest_gpu_ransac: {time.time() - _T0:.1f} s from import to the last test")


def _handle(gvamd, case):
    h = gvamd.GridVisionHIP(100, 100, 0.5)
    if np.array_equal(case.tf, RC.IDENT_TF):
        h.set_transforms(RC.IDENT_TF, RC.IDENT_TF, RC.IDENT_TF)
    else:
        tfs = synth.transforms(True)
        h.set_transforms(tfs["cam_lidar"], tfs["base_cam"], tfs["base_lidar"])
    return h


def _state_bytes(st):
    return (st["plane"].tobytes(), st["refined"].tobytes(), st["m"], st["n_inliers"], st["best_count"])


def _hold_state(tag, st, r):
    assert st["best_count"] == r.best_count, (tag, "best_count", st["best_count"], r.best_count)
    assert st["plane"].tobytes() == r.plane.tobytes(), (tag, "plane", st["plane"], r.plane)
    assert st["m"] == r.m, (tag, "m", st["m"], r.m)
    assert st["best_count"] == st["m"], (tag, "the count pass and the moments pass disagree", st["best_count"], st["m"])
    assert st["refined"].tobytes() == r.refined.tobytes(), (tag, "refined", st["refined"], r.refined, r.margin)
    assert st["n_inliers"] == r.n_inliers, (tag, "n_inliers", st["n_inliers"], r.n_inliers)


def _segment(h, case):
    """the case through the hook's gv_segment_ground_plane path, three times"""
    r = RC.reference(case)
    first = None
    for _ in range(3):
        st = h.ransac_state(case.thr, case.iters, case.seed)
        now = _state_bytes(st) + (st["mask"].tobytes(),)
        assert first is None or now == first, (case.tag, "not repeatable")
        first = now
    _hold_state(case.tag, st, r)
    bad = np.flatnonzero(st["mask"] != r.mask)
    assert not len(bad), (case.tag, "mask", len(bad), bad[:8])
    assert set(np.unique(st["mask"])) <= {0, 1}


def _check(gvamd, case):
    with _handle(gvamd, case) as h:
        h.upload_xyz(case.x, case.y, case.z)
        _segment(h, case)


def _pose_path(h, case, boxes):
    """gv_compute_bbox_pose_ground_removed on the resident cloud: state, valid, poses, and the selected points"""
    r = RC.reference(case)
    cam = RC.camera(case)
    n = len(case.x)
    res = P.run(*cam, boxes, drop=r.mask.astype(bool))
    empty = r.best_count == 0 or r.n_inliers == 0 or r.n_inliers == n
    first = None
    for _ in range(3):
        st = h.ransac_state(bboxes=boxes)
        poses, valid, nodes, keep = h.bbox_pose_nodes(boxes, ground_removed=True)
        ms = P.multiset_of(nodes["id"], nodes["x"], nodes["y"], nodes["z"], keep)
        now = _state_bytes(st) + (st["poses"].tobytes(), st["valid"].tobytes(), st["n_poses"], ms.tobytes())
        assert first is None or now == first, (case.tag, "not repeatable")
        first = now
        assert poses.tobytes() == st["poses"].tobytes() and valid.tobytes() == st["valid"].tobytes()
    if n >= 3:
        _hold_state(case.tag + " (pose path)", st, r)
        want = P.multiset(res, *cam)
        assert ms.shape == want.shape, (case.tag, "selected points", len(ms), len(want))
        bad = np.flatnonzero((ms != want).any(axis=1))
        assert not len(bad), (case.tag, "ids / keep flags", len(bad), ms[bad[:4]].tolist(), want[bad[:4]].tolist())
    else:
        assert _state_bytes(st) == (bytes(16), bytes(16), 0, 0, 0) and len(nodes) == 0
    if empty:
        assert st["n_poses"] == -1 and not st["valid"].any(), case.tag
    else:
        assert np.array_equal(st["valid"], res.valid) and st["n_poses"] == res.valid.sum(), case.tag
        for f in ("px", "py", "pz", "length", "width", "height"):
            assert st["poses"][f].tobytes() == res.poses[f].tobytes(), (case.tag, f)
    return st, res


@pytest.mark.parametrize("case", RC.threshold_cases(), ids=lambda c: c.tag)
def test_threshold_edge(gvamd, case):
    _check(gvamd, case)


def test_rounding_sensitive(gvamd):
    """B: the segment call, the pose path and the tick's PCA branch"""
    case = RC.rounding_case()
    boxes = P.grid_boxes(4, 3)
    with _handle(gvamd, case) as h:
        h.upload_xyz(case.x, case.y, case.z)
        _segment(h, case)
        st, res = _pose_path(h, case, boxes)
        assert res.valid.sum() >= 1
        # the threshold-edge points inside a box land on their reference side (the multiset above holds all of them)
        r = RC.reference(case)
        e = case.meta["refined_edge"]
        assert (res.ids[e][r.mask[e] == 1] == -1).all()
        want = h.transform_lshape_objects(st["poses"][st["valid"].astype(bool)])
        t = h.tick(boxes, k_near=4)
        assert not t["pca_empty"] and t["poses"].tobytes() == want.tobytes()


@pytest.mark.parametrize("case", RC.tie_cases(), ids=lambda c: c.tag)
def test_ties(gvamd, case):
    _check(gvamd, case)


@pytest.mark.parametrize("case", RC.degenerate_cases(), ids=lambda c: c.tag)
def test_degenerate(gvamd, case):
    with _handle(gvamd, case) as h:
        h.upload_xyz(case.x, case.y, case.z)
        if len(case.x) >= 3:
            _segment(h, case)
        else:
            st = h.ransac_state(case.thr, case.iters, case.seed)
            assert _state_bytes(st) == (bytes(16), bytes(16), 0, 0, 0) and not st["mask"].any()
        _pose_path(h, case, RC.boxes())


def test_one_handle_sequence(gvamd):
    """failing and good clouds and other iteration counts take turns on ONE handle: every result equals the reference
    (which is what a fresh handle gives): the counts and the ticket are cleared inside the kernels"""
    seq = RC.handle_sequence()
    with _handle(gvamd, seq[0]) as h:
        for case in seq:
            h.upload_xyz(case.x, case.y, case.z)
            _segment(h, case)


@pytest.mark.parametrize("case", RC.sum_cases(), ids=lambda c: c.tag)
def test_sum_order(gvamd, case):
    with _handle(gvamd, case) as h:
        h.upload_xyz(case.x, case.y, case.z)
        _segment(h, case)
        if len(case.x) in (65, 4097):
            _pose_path(h, case, RC.boxes())


@pytest.mark.parametrize("case", RC.step_cases(), ids=lambda c: c.tag)
def test_butterfly_steps(gvamd, case):
    """G: the fixtures on which two butterfly steps in another order change the refined plane's bytes"""
    _check(gvamd, case)


def test_general_tree(gvamd):
    """F: 4098 workgroups, the ping-pong tree 4098 -> 65 -> 2 -> 1 (the one test that takes longer, by construction)"""
    _check(gvamd, RC.general_case())
