"""The per-box cloud path of gv_compute_bbox_pose (k_pose_classify -> k_cell_scan -> k_cell_scatter -> k_radius_sorted
-> k_pca_cov -> k_pca_extent, gv_cloudops.hip) held point by point to tests/pose_ref.py: the box id and the keep flag
of EVERY selected point (read back through the test hook gv_test_bbox_pose_nodes, compared as a sorted multiset: the
order inside a bucket is arbitrary, and equal points carry equal flags), `valid`, and px, py, pz, length, width and
height byte for byte, at the edges tests/test_pose_host.py proves the fixtures reach: the radius predicate at R2F and
one ulp above it, neighbour counts of 10 / 11 / 12, the deciding neighbour in each of the 27 cells at every residue of
the bucket's low bits, negative cells, cells across zero and on faces, runs of every length around the walk's steps,
the cell-by-cell branch at 3e6 m and at 1e30, both clamps of the sums, the branches of the 2 x 2 eigen step, and the
table sizes (64 / 128 boxes, several boxes per wavefront, 32 / 128 selected points).

Every family runs on a fresh handle (4096 buckets: every bucket is shared by far cells and other boxes) and on a handle
whose table an earlier 1.1 M-point call grew to 2^20 buckets (block offsets read from global memory).  Every call is
made three times and must repeat its bytes.

The one tolerance: qy = sin(hp) and qw = cos(hp) of the reference's float64 hp, evaluated in extended precision and
rounded to float64, within QUAT_ULPS float64 ulps (the device's sin / cos are not correctly rounded).  A wrong angle
cannot hide there: one float32 ulp of the angle moves qy by more than 1e9 float64 ulps."""
import time

import numpy as np
import pytest

import oracle_lib as ol
import pose_ref as P
from knn_depth_ref import IDENT_TF

pytestmark = pytest.mark.gpu
# measured over all families on an MI355X: 1 ulp at the most (Tolerances); twice that, never below 2
QUAT_ULPS = 2.0
_T0 = time.time()
_SEEN = {"ulps": 0.0, "boxes": 0}


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    yield m
    print(f"\ntest_gpu_pose: {time.time() - _T0:.1f} s from import to the last test; sin / cos of hp within "
          f"{_SEEN['ulps']:.2f} float64 ulps of extended precision over {_SEEN['boxes']} poses")


def _handle(gvamd):
    h = gvamd.GridVisionHIP(100, 100, 0.5)
    h.set_transforms(IDENT_TF, IDENT_TF, IDENT_TF)
    return h


@pytest.fixture(scope="module")
def grown(gvamd):
    """a handle whose bucket table one call on 1.1 M points (all behind the camera: nothing selected) grew to 2^20"""
    h = _handle(gvamd)
    h.upload_xyz(*P.behind_camera_cloud())
    poses, valid, nodes, keep = h.bbox_pose_nodes(P.make_boxes([(0.0, 0.0, 640.0, 480.0)]))
    assert len(nodes) == 0 and not valid.any()
    yield h
    h.close()


def _call(h, boxes, ground=False):
    """three calls, the same bytes: poses, valid and the sorted multiset of (id, x, y, z, keep)"""
    out = None
    for _ in range(3):
        poses, valid, nodes, keep = h.bbox_pose_nodes(boxes, ground_removed=ground)
        assert set(np.unique(keep)) <= {0, 1}
        ms = P.multiset_of(nodes["id"], nodes["x"], nodes["y"], nodes["z"], keep)
        now = (poses.tobytes(), valid.tobytes(), ms.tobytes())
        assert out is None or now == out[0], "not repeatable"
        out = (now, poses, valid, ms)
    return out[1:]


def _hold(tag, got, res, cam):
    """the hook's multiset, valid and the poses against the reference's"""
    poses, valid, ms = got
    want = P.multiset(res, *cam)
    assert ms.shape == want.shape, (tag, "selected points", len(ms), len(want))
    bad = np.flatnonzero((ms != want).any(axis=1))
    assert not len(bad), (tag, "ids / keep flags", len(bad), ms[bad[:4]].tolist(), want[bad[:4]].tolist())
    assert np.array_equal(valid, res.valid), (tag, "valid")
    for f in ("px", "py", "pz", "length", "width", "height"):
        assert poses[f].tobytes() == res.poses[f].tobytes(), (tag, f, np.flatnonzero(poses[f] != res.poses[f])[:4])
    assert (poses["qx"] == 0).all() and (poses["qz"] == 0).all(), tag
    for b in np.flatnonzero(res.valid):
        s, c = P.sincos_extended(res.rects[b].hp)
        u = max(P.ulps64(poses["qy"][b], s), P.ulps64(poses["qw"][b], c))
        _SEEN["ulps"], _SEEN["boxes"] = max(_SEEN["ulps"], u), _SEEN["boxes"] + 1
        assert u <= QUAT_ULPS, (tag, int(b), u, poses["qy"][b], s, poses["qw"][b], c)
    inv = res.valid == 0
    assert (poses["qy"][inv] == 0).all() and (poses["qw"][inv] == 0).all(), tag


def _check(h, scene):
    cam, res = P.reference(scene)
    h.upload_xyz(scene.x, scene.y, scene.z)
    _hold(scene.tag, _call(h, scene.boxes), res, cam)


@pytest.mark.parametrize("table", ["fresh", "grown"])
@pytest.mark.parametrize("fam", P.FAMILIES)
def test_family(gvamd, grown, fam, table):
    h = _handle(gvamd) if table == "fresh" else grown
    try:
        for s in P.family(fam):
            assert table == "grown" or len(s.x) <= 8192      # a fresh handle keeps 4096 buckets up to there
            _check(h, s)
    finally:
        if table == "fresh":
            h.close()


def test_no_boxes_and_no_points(gvamd):
    """what launches nothing reports nothing"""
    s = P.family("sizes")[0]
    e = np.zeros(0, np.float32)
    with _handle(gvamd) as h:
        h.upload_xyz(s.x, s.y, s.z)
        poses, valid, nodes, keep = h.bbox_pose_nodes(s.boxes[:0])
        assert len(poses) == len(valid) == len(nodes) == len(keep) == 0
        h.upload_xyz(e, e, e)
        poses, valid, nodes, keep = h.bbox_pose_nodes(s.boxes)
        assert len(nodes) == 0 and not valid.any() and poses.tobytes() == bytes(poses.nbytes)


@pytest.mark.parametrize("fam,which", [("sizes", 6), ("count-edge", 0)], ids=["nb-129", "count-edge"])
def test_ground_removed(gvamd, fam, which):
    """gv_compute_bbox_pose_ground_removed on a family plus a planted plane: ids and flags on the points the oracle's
    ground mask leaves (the device's own mask is held to the oracle's first, so a difference here is the path's)"""
    s = P.with_plane(P.family(fam)[which])
    cam = P.camera_frame(s.x, s.y, s.z)
    m, ground, _ = ol.segment_ground_plane(*cam)
    assert 5000 <= m < len(s.x)
    res = P.run(*cam, s.boxes, drop=ground.astype(bool))
    assert res.valid.sum() >= 20 and (res.ids[ground.astype(bool)] == -1).all()
    with _handle(gvamd) as h:
        h.upload_xyz(s.x, s.y, s.z)
        dm, dmask, _ = h.segment_ground_plane()
        assert dm == m and np.array_equal(dmask, ground)
        _hold(s.tag, _call(h, s.boxes, ground=True), res, cam)
        assert h.compute_bbox_pose_ground_removed(s.boxes)[2] == res.valid.sum()


def test_tick_pca_branch(gvamd):
    """gv_tick's PCA branch (ground removal, then the same kernels with the poses handed on in device memory) against
    the call sequence on the same handle, whose hook output is held to the reference"""
    s = P.with_plane(P.family("sizes")[3])      # 65 boxes
    cam = P.camera_frame(s.x, s.y, s.z)
    _, ground, _ = ol.segment_ground_plane(*cam)
    res = P.run(*cam, s.boxes, drop=ground.astype(bool))
    with _handle(gvamd) as h:
        h.upload_xyz(s.x, s.y, s.z)
        st, dy = gvamd.filter_bboxes(s.boxes)
        assert len(st) == 0 and len(dy) == len(s.boxes)
        for _ in range(2):
            got = _call(h, s.boxes, ground=True)
            _hold(s.tag, got, res, cam)
            want = h.transform_lshape_objects(got[0][got[1].astype(bool)])
            r = h.tick(s.boxes, k_near=4)
            assert not r["pca_empty"] and len(r["poses"]) == res.valid.sum() >= 50
            assert r["poses"].tobytes() == want.tobytes()


def test_nothing_stale_after_a_large_call(gvamd):
    """the largest family, then small ones on the same handle (fewer boxes, fewer selected points, none at all), then
    the large one again: keep, nodes and the accumulators carry nothing over"""
    big = P.family("cells")[0]
    small = {s.tag: s for s in P.family("sizes")}
    with _handle(gvamd) as h:
        for s in (big, small["selected-1"], small["nb-300"], small["nb-1"], big, small["selected-0"], small["cloud-1"],
                  small["nb-129"], P.family("degenerate")[0], big):
            _check(h, s)


def _result_bytes(r):
    """a call's outputs (a tuple, or a tick's dict) as a list of byte strings"""
    vals = [r[k] for k in sorted(r)] if isinstance(r, dict) else list(r)
    return [np.asarray(v).tobytes() for v in vals]


def test_calls_share_one_result_block(gvamd):
    """kNN depth, the two pose calls, the ground plane and both ticks take turns on ONE handle: they share the result
    block (regrown by the 300-box pose, 300 * 81 + 56 bytes, with earlier calls' sequence numbers behind it), the
    sequence counter and the pose scratch.  Every step's outputs equal, byte for byte, those of the same call on a fresh
    handle given the same cloud.  Between the PCA tick's enqueue and its wait the calls that would reuse the block are
    refused with GV_ERR_STATE and leave the tick's result as it is."""
    from gvamd import synth
    sizes = {s.tag: s for s in P.family("sizes")}
    one, many, plane = sizes["nb-1"], sizes["nb-300"], P.with_plane(sizes["nb-129"])
    for s in (one, many, plane):
        assert len(s.x) <= 8192                       # a fresh handle's 4096 buckets
    assert 300 * 81 + 56 > 16384 - 64                 # the first block does not hold the 300-box pose
    static = P.grid_boxes(4, 3, 3)
    static["label"] = 5                               # gv_filter_bboxes: static
    mixed = np.concatenate([plane.boxes[:40], static])   # the dynamic boxes first: first match wins
    net = synth.network_outputs(40)
    refused = {}

    def knn(h):
        return h.compute_depth_for_bboxes(static, 4)

    def ground(h):
        m, mask, coeff = h.segment_ground_plane()
        return np.int64(m), mask, coeff

    def pca_tick_with_refusals(h):
        h.tick_enqueue(mixed, k_near=4)
        for name, call in (("depth", lambda: knn(h)), ("pose", lambda: h.compute_bbox_pose(one.boxes)),
                           ("ground", lambda: h.segment_ground_plane()),
                           ("pose_ground_removed", lambda: h.compute_bbox_pose_ground_removed(plane.boxes))):
            with pytest.raises(gvamd.GVError) as e:
                call()
            refused[name] = (e.value.code, str(e.value))
        return h.tick_wait()

    steps = [("knn", plane, knn, knn),
             ("pose nb-1", one, lambda h: h.compute_bbox_pose(one.boxes), None),
             ("pose nb-300", many, lambda h: h.compute_bbox_pose(many.boxes), None),
             ("ground plane", plane, ground, None),
             ("pose ground removed", plane, lambda h: h.compute_bbox_pose_ground_removed(plane.boxes), None),
             ("vision tick", plane, lambda h: h.tick(mixed, k_near=4, vision=True, net=net), None),
             ("pca tick", plane, pca_tick_with_refusals, lambda h: h.tick(mixed, k_near=4)),
             ("knn again", plane, knn, None),
             ("pose nb-1 again", one, lambda h: h.compute_bbox_pose(one.boxes), None)]
    got = {}
    with _handle(gvamd) as shared:
        for tag, s, call, alone in steps:
            shared.upload_xyz(s.x, s.y, s.z)
            got[tag] = call(shared)
            with _handle(gvamd) as fresh:
                fresh.upload_xyz(s.x, s.y, s.z)
                want = (alone or call)(fresh)
            assert _result_bytes(got[tag]) == _result_bytes(want), tag
    for name, (code, msg) in refused.items():
        assert code == 5 and "a tick is pending: call gv_tick_wait first" in msg, (name, code, msg)
    assert len(refused) == 4
    # the steps computed something: depths, 300 boxes' worth of poses, a plane, poses from both ticks
    assert (got["knn"][0] > 0).all()
    for tag, s in (("pose nb-1", one), ("pose nb-300", many)):
        assert np.array_equal(got[tag][1], P.reference(s)[1].valid) and got[tag][1].any(), tag
    assert 5000 <= int(got["ground plane"][0]) < len(plane.x) and got["pose ground removed"][2] >= 20
    assert got["vision tick"]["n_static"] == 3 and got["vision tick"]["n_dynamic"] == 40
    assert not got["pca tick"]["pca_empty"] and len(got["pca tick"]["poses"]) > 0 and len(got["pca tick"]["depths"]) == 3
