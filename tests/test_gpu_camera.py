"""The projection and the box test at cameras other than gvamd.synth's 640 x 480 with fx = fy = cx = 320: image sizes at
which the box-test tables no longer fit the partition kernel's LDS (the frame appends a k_points pass of its own) or
k_pose_classify's (its tables stay in global memory), images that end inside a 16 x 16 tile, fx != fy, and principal
points that are no integers or lie outside the image.  Cameras, scenes and box sets come from tests/camera_cases.py;
tests/test_camera_host.py proves on the CPU what they reach and which table path every case here takes.

Everything is compared bit for bit with the CPU oracle (ids, counts, cell indices, hit and free counts, the three grid
layers as test_gpu_parity.check_grid holds them, kNN depths and distances, back-projected points, intrinsics) or with
tests/pose_ref.py under test_gpu_pose._hold, whose quaternion rule (QUAT_ULPS) is the only tolerance; the tick's poses
against the ORACLE's own PCA are held as test_gpu_parity._check_pose holds them everywhere else."""
import time

import numpy as np
import pytest

import camera_cases as cc
import knn_depth_ref as R
import oracle_lib as ol
import pose_ref as P
from gvamd import synth
from test_gpu_parity import _base_poses, _check_pose, _pose_reference, check_grid, oracle_frame
from test_gpu_pose import _call, _hold

pytestmark = pytest.mark.gpu

FRAME_CASES, PIPELINE_CASES, SHARD_CASES, POSE_CASES = cc.FRAME_CASES, cc.PIPELINE_CASES, cc.SHARD_CASES, cc.POSE_CASES
STALE_CASE = cc.STALE_CASE
TILE_GRID, GENERIC_GRID = (100, 100, 0.5), (50, 20, 0.3)      # nx % 4 == 0: the tile path; 167 x 67 cells: the generic one
_T0 = time.time()


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    yield m
    print(f"\ntest_gpu_camera: {time.time() - _T0:.1f} s from import to the last test")


def _handle(gvamd, cam, tfs, grid=TILE_GRID):
    h = gvamd.GridVisionHIP(*grid, **cc.create_args(cam))
    h.set_transforms(tfs["cam_lidar"], tfs["base_cam"], tfs["base_lidar"])
    return h


def _camera(cam):
    return (cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h)


def _full(gvamd):
    return (gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH | gvamd.FRAME_BBOX_TEST | gvamd.FRAME_KEEP_CELL_IDX
            | gvamd.FRAME_KEEP_COUNTS)


def _hold_frame(h, og, s, boxes, poses, tag, cell=True):
    """one oracle frame on og, and the handle's last frame and grid against it"""
    hits, cells, miss, ids, _ = oracle_frame(og, s.tfs, s.x, s.y, s.z, boxes, poses, camera=_camera(s.cam))
    got = h.bbox_id()
    bad = np.flatnonzero(got != ids)
    assert not len(bad), (tag, "bbox_id", len(bad), bad[:4].tolist(), got[bad[:4]].tolist(), ids[bad[:4]].tolist())
    if cell:
        assert np.array_equal(h.cell_idx(), cells), (tag, "cell_idx")
    assert np.array_equal(h.hits(), hits), (tag, "hits")
    assert np.array_equal(h.miss(), miss), (tag, "miss")
    assert check_grid(h, og)[0] == 0, tag
    return ids


# ------------------------------------------------------------------------------------ 1. the standalone box test --

@pytest.mark.parametrize("cam_name,nb,perturbed", cc.STANDALONE_CASES)
def test_standalone_box_test(gvamd, cam_name, nb, perturbed):
    """gv_extract_cloud_per_bbox (k_bbox_prepare + k_points<false, false, true, false>): ids and counts"""
    s, g, bs = cc.scene(cam_name, perturbed), cc.geo(cam_name, perturbed), cc.box_set(cam_name, perturbed, nb)
    want = g.ids(bs.boxes)
    with _handle(gvamd, s.cam, s.tfs) as h:
        h.upload_xyz(s.x, s.y, s.z)
        ids, counts = h.extract_cloud_per_bbox(bs.boxes)
    bad = np.flatnonzero(ids != want)
    assert not len(bad), (len(bad), bad[:4].tolist(), ids[bad[:4]].tolist(), want[bad[:4]].tolist(),
                          g.u[bad[:4]].tolist(), g.v[bad[:4]].tolist())
    assert np.array_equal(counts, np.bincount(want[want >= 0], minlength=nb))


# ------------------------------------------------------------------------------------------------------ 2. frames --

@pytest.mark.parametrize("grid", [TILE_GRID, GENERIC_GRID], ids=["tile-grid", "generic-grid"])
@pytest.mark.parametrize("cam_name,nb", FRAME_CASES)
def test_frame(gvamd, cam_name, nb, grid):
    """gv_process_frame with the box test: fused into k_bin_partition or as the k_points pass behind it (which of the
    two: test_camera_host.test_path_table).  Without KEEP_CELL_IDX and without the ray stage -- other instantiations of
    both kernels -- the ids are the same."""
    B, R_, X, KC = gvamd.FRAME_BIN, gvamd.FRAME_RAYMARCH, gvamd.FRAME_BBOX_TEST, gvamd.FRAME_KEEP_COUNTS
    poses = cc.grid_poses(grid)
    for perturbed in (False, True):
        s, bs = cc.scene(cam_name, perturbed), cc.box_set(cam_name, perturbed, nb)
        og = ol.OGrid(*grid)
        with _handle(gvamd, s.cam, s.tfs, grid) as h:
            h.upload_xyz(s.x, s.y, s.z)
            h.process_frame(_full(gvamd), bboxes=bs.boxes, poses=poses)
            ids = _hold_frame(h, og, s, bs.boxes, poses, (cam_name, nb, perturbed, "full"))
            assert (ids >= 0).sum() > len(ids) // 4 and h.hits().sum() > 0 and h.miss().sum() > 0
            h.process_frame(B | R_ | X | KC, bboxes=bs.boxes, poses=poses)
            _hold_frame(h, og, s, bs.boxes, poses, (cam_name, nb, perturbed, "no cell_idx"), cell=False)
            h.process_frame(B | X | KC, bboxes=bs.boxes, poses=poses)
            assert np.array_equal(h.bbox_id(), ids), (cam_name, nb, perturbed, "bin + box test")
            assert np.array_equal(h.hits(), og.bin_points(ol.tf_to_matrix4f(s.tfs["base_lidar"]), s.x, s.y, s.z)[0])


# ------------------------------------------------------------------------------ 3. the extra pass in the pipeline --

@pytest.mark.parametrize("cam_name,sets,pipeline,lanes",
                         [(c, sets, p, l) for c, sets in PIPELINE_CASES
                          for p, l in ((("1", "3"), ("1", "2"), ("0", "3"), ("0", "2")) if c == "kitti" else (("1", "3"),))])
def test_extra_pass_in_the_pipeline(gvamd, monkeypatch, cam_name, sets, pipeline, lanes):
    """frames in flight whose detection sets alternate between the two box counts (at kitti: fused, unfused) and whose
    clouds alternate between two sizes, one synchronize at the end: the last frame's ids and the grid of all of them.
    Five frames that start with the first set, then five that start with the second, so that either kind is last once."""
    monkeypatch.setenv("GV_PIPELINE", pipeline)
    monkeypatch.setenv("GV_LANES", lanes)
    full = cc.scene(cam_name, True)
    clouds = [cc.prefix(full, cc.SMALL_SIZES[0]), cc.prefix(full, cc.SMALL_SIZES[1])]
    boxes = [cc.box_set(cam_name, True, nb).boxes for nb in sets]
    flags = gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH | gvamd.FRAME_BBOX_TEST
    poses = cc.grid_poses(TILE_GRID)
    og = ol.OGrid(*TILE_GRID)
    with _handle(gvamd, full.cam, full.tfs) as h:
        for start in (0, 1):
            for f in range(5):
                s, b = clouds[f % 2], boxes[(start + f) % 2]
                h.upload_xyz(s.x, s.y, s.z)
                h.set_detections_async(flags, bboxes=b, poses=poses)
                h.enqueue_frame()
            h.synchronize()
            for f in range(5):
                s, b = clouds[f % 2], boxes[(start + f) % 2]
                hits, _, miss, ids, _ = oracle_frame(og, s.tfs, s.x, s.y, s.z, b, poses, camera=_camera(s.cam))
            assert np.array_equal(h.bbox_id(), ids), (start, "bbox_id")
            assert (ids >= 64).any() == (len(b) > 64) and (ids >= 0).sum() > len(ids) // 4
            assert np.array_equal(h.hits(), hits) and np.array_equal(h.miss(), miss), start
            assert check_grid(h, og)[0] == 0, start


# ---------------------------------------------------------------------------------------------- 4. sharded slices --

@pytest.mark.parametrize("cam_name,nb,world", SHARD_CASES)
def test_sharded_slices(gvamd, cam_name, nb, world):
    """every rank's unfused box test of its point slice (the `lo` offset of bbox_points_args): the union equals the
    plain frame and the oracle"""
    s, bs = cc.scene(cam_name, False), cc.box_set(cam_name, False, nb)
    assert len(s.x) % world != 0
    poses = cc.grid_poses(TILE_GRID)
    flags = gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH | gvamd.FRAME_BBOX_TEST | gvamd.FRAME_KEEP_CELL_IDX
    og = ol.OGrid(*TILE_GRID)
    with _handle(gvamd, s.cam, s.tfs) as h, _handle(gvamd, s.cam, s.tfs) as plain:
        for hh in (h, plain):
            hh.upload_xyz(s.x, s.y, s.z)
        for frame in range(2):
            h.frame_sharded_emulated(world, flags, bboxes=bs.boxes, poses=poses)
            plain.process_frame(flags, bboxes=bs.boxes, poses=poses)
            _, cell, _, ids, _ = oracle_frame(og, s.tfs, s.x, s.y, s.z, bs.boxes, poses, camera=_camera(s.cam))
            assert np.array_equal(h.bbox_id(), ids) and np.array_equal(plain.bbox_id(), ids), frame
            assert np.array_equal(h.cell_idx(), cell), frame
            assert check_grid(h, og)[0] == 0 and np.array_equal(h.log_odds(), plain.log_odds()), frame
        # every third of the cloud holds matches of both mask words: a slice that read another slice's points shows
        for part in np.array_split(ids, 3):
            assert (part >= 64).any() and ((part >= 0) & (part < 64)).any() and (part < 0).any()


# ---------------------------------------------------------------------------------------------- 5. per-box clouds --

@pytest.fixture(scope="module")
def grown(gvamd):
    """per camera, a handle whose bucket table one call on 1.1 M points behind the camera grew to 2^20 buckets"""
    handles = {}

    def get(cam):
        if cam.name not in handles:
            h = _handle(gvamd, cam, {k: P.IDENT_TF for k in ("cam_lidar", "base_cam", "base_lidar")})
            h.upload_xyz(*P.behind_camera_cloud())
            poses, valid, nodes, keep = h.bbox_pose_nodes(P.make_boxes([(0.0, 0.0, float(cam.w), float(cam.h))]))
            assert len(nodes) == 0 and not valid.any()
            handles[cam.name] = h
        return handles[cam.name]

    yield get
    for h in handles.values():
        h.close()


IDENT = {k: P.IDENT_TF for k in ("cam_lidar", "base_cam", "base_lidar")}


@pytest.mark.parametrize("table", ["fresh", "grown"])
@pytest.mark.parametrize("cam_name,nb", POSE_CASES)
def test_per_box_clouds(gvamd, grown, cam_name, nb, table):
    """gv_compute_bbox_pose through the test hook: every selected point's box and keep flag, valid and the pose fields,
    three calls with the same bytes, k_pose_classify with its tables in LDS or in global memory"""
    cam, s = cc.CAMERAS[cam_name], cc.pose_scene(cam_name, nb)
    camf, res = P.reference(s, K=cc.K_of(cam), w=cam.w, h=cam.h)
    h = _handle(gvamd, cam, IDENT) if table == "fresh" else grown(cam)
    try:
        h.upload_xyz(s.x, s.y, s.z)
        _hold(s.tag, _call(h, s.boxes), res, camf)
    finally:
        if table == "fresh":
            h.close()


def test_per_box_clouds_ground_removed(gvamd):
    """gv_compute_bbox_pose_ground_removed at kitti on a scene plus a planted plane"""
    cam = cc.CAMERAS["kitti"]
    s = P.with_plane(cc.pose_scene("kitti", 64))
    camf = P.camera_frame(s.x, s.y, s.z)
    m, ground, _ = ol.segment_ground_plane(*camf)
    assert 5000 <= m < len(s.x)
    res = P.run(*camf, s.boxes, drop=ground.astype(bool), K=cc.K_of(cam), w=cam.w, h=cam.h)
    assert res.valid.sum() >= 20 and (res.ids[ground.astype(bool)] == -1).all()
    with _handle(gvamd, cam, IDENT) as h:
        h.upload_xyz(s.x, s.y, s.z)
        dm, dmask, _ = h.segment_ground_plane()
        assert dm == m and np.array_equal(dmask, ground)
        _hold(s.tag, _call(h, s.boxes, ground=True), res, camf)
        assert h.compute_bbox_pose_ground_removed(s.boxes)[2] == res.valid.sum()


# --------------------------------------------------------------------------------- 6. kNN depth, back-projection --

def _pixel_points(tfs, boxes, depths, kinv):
    return np.array([ol.tf_point(tfs["base_cam"], ol.pixel_to_3d(
        np.float32(bb["x_min"] + ((bb["x_max"] - bb["x_min"]) / np.float32(2.0))),
        np.float32(bb["y_min"] + ((bb["y_max"] - bb["y_min"]) / np.float32(2.0))), dep, kinv))
        for bb, dep in zip(boxes, depths)]).reshape(-1, 3)


@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("cam_name", cc.KNN_CAMERAS)
def test_knn_depth_and_back_projection(gvamd, cam_name, perturbed):
    """gv_compute_depth_for_bboxes (k_project_uvd: the full 3 x 3 form) against knn_depth_ref as test_gpu_knn_depth
    accepts it -- distances and depths equal, every call three times --, gv_convert_pixels_to_3d (Kinv) and
    gv_get_intrinsics against the oracle"""
    s, g = cc.scene(cam_name, perturbed), cc.geo(cam_name, perturbed)
    boxes = cc.box_set(cam_name, perturbed, 64).boxes
    finite = np.isfinite(boxes["x_max"])
    K = cc.K_of(s.cam)
    ref = R.knn_depth(K, g.cx, g.cy, g.cz, boxes, cc.KNN_KS)
    with _handle(gvamd, s.cam, s.tfs) as h:
        k, ki = h.intrinsics()
        assert k.tolist() == K.tolist() and ki.tolist() == ol.k_inverse(K).tolist()
        h.upload_xyz(s.x, s.y, s.z)
        for kk in cc.KNN_KS:
            depths, d2 = h.compute_depth_for_bboxes(boxes, kk)
            for _ in range(2):
                a, b = h.compute_depth_for_bboxes(boxes, kk)
                assert a.tobytes() == depths.tobytes() and b.tobytes() == d2.tobytes(), ("not repeatable", kk)
            assert np.array_equal(d2, ref[kk][1]), (kk, "distances")
            assert np.array_equal(depths, ref[kk][0]), (kk, "depth")
            assert (depths[finite] > 0).all()
            pts = h.convert_pixels_to_3d(boxes[finite], depths[finite])
            assert pts.tobytes() == _pixel_points(s.tfs, boxes[finite], depths[finite], ki).tobytes(), kk


# ------------------------------------------------------------------------------------------------------ 7. one tick --

def _tick_oracle(s, b, st, k_near=4):
    g = cc.Geo(s.cam, s.tfs, s.x, s.y, s.z)
    K = cc.K_of(s.cam)
    u, v, d = ol.project_points(K, g.cx, g.cy, g.cz)
    edepth, _ = ol.depth_for_bboxes(u, v, d, st, k_near)
    return g, K, edepth, _pixel_points(s.tfs, st, edepth, ol.k_inverse(K))


def test_tick_pca_branch_with_lidar_binning(gvamd):
    """hd720, 70 detections: gv_tick on handle A equals the call sequence on its twin B (depths, points, poses, grid
    layers, the packed grid it delivered) and the oracle (depths and points bit for bit, poses as _check_pose holds
    them, the grid of the oracle's frame fed with the tick's poses)"""
    s, b = cc.tick_scene("hd720", 70)
    st, dy = gvamd.filter_bboxes(b)
    assert len(b) == 70 and len(st) >= 10 and len(dy) >= 40
    g, K, edepth, epts = _tick_oracle(s, b, st)
    _, emask, _ = ol.segment_ground_plane(g.cx, g.cy, g.cz)
    keep = emask == 0
    _, ref = _pose_reference(g.cx[keep], g.cy[keep], g.cz[keep], K, b,
                             lambda a, c, e: ol.radius_outlier(a, c, e, 0.4, 10).astype(bool), image=(s.cam.w, s.cam.h))
    want = _base_poses(s.tfs, [e for ok, e, _, _ in ref if ok])
    assert len(want) >= 30
    og = ol.OGrid(*TILE_GRID)
    flags = gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH
    with _handle(gvamd, s.cam, s.tfs) as hA, _handle(gvamd, s.cam, s.tfs) as hB:
        pin = gvamd.PinnedI8(hA.G)
        try:
            for h in (hA, hB):
                h.upload_xyz(s.x, s.y, s.z)
            for tick in range(2):
                r = hA.tick(b, k_near=4, lidar_bin=True, lidar_raymarch=True, grid_out=pin.array)
                bdepth = hB.compute_depth_for_bboxes(st, 4)[0]
                bpts = hB.convert_pixels_to_3d(st, bdepth)
                pp, valid, npz = hB.compute_bbox_pose_ground_removed(b)
                bposes = hB.transform_lshape_objects(pp[valid.astype(bool)])
                hB.process_frame(flags | gvamd.FRAME_KEEP_COUNTS, poses=bposes)
                assert r["n_static"] == len(st) and r["n_dynamic"] == len(dy) and r["pca_empty"] is False
                assert r["depths"].tobytes() == bdepth.tobytes() and np.array_equal(r["depths"], edepth)
                assert r["base_points"].tobytes() == np.ascontiguousarray(bpts).tobytes()
                assert np.array_equal(r["base_points"], epts)
                assert r["poses"].tobytes() == bposes.tobytes() and npz == len(bposes)
                assert np.array_equal(hA.log_odds(), hB.log_odds()) and np.array_equal(hA.occupancy(), hB.occupancy())
                i8 = hA.to_occupancy_grid()[0]
                assert np.array_equal(i8, hB.to_occupancy_grid()[0]) and np.array_equal(pin.array, i8)
                assert np.array_equal(hA.hits(), hB.hits())
                assert len(r["poses"]) == len(want)
                for i, (p, e) in enumerate(zip(r["poses"], want)):
                    _check_pose(p, e, ("pca", i))
                hits, _, miss, _, _ = oracle_frame(og, s.tfs, s.x, s.y, s.z, None, r["poses"])
                assert np.array_equal(hA.hits(), hits)
                assert check_grid(hA, og)[0] == 0
        finally:
            pin.close()


def test_tick_vision_branch(gvamd):
    """kitti: the orientation-network branch of gv_tick (theta_ray and the constraint sets read fx, cx, cy and the image
    size) against the call sequence and the oracle's post-process"""
    s, b = cc.tick_scene("kitti", 70)
    cam = s.cam
    st, dy = gvamd.filter_bboxes(b)
    net = synth.network_outputs(len(dy))
    g, K, edepth, epts = _tick_oracle(s, b, st)
    want = _base_poses(s.tfs, ol.post_process(ol.make_cam(cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h), *net, dy))
    assert len(want) == len(dy) >= 40
    og = ol.OGrid(*TILE_GRID)
    with _handle(gvamd, cam, s.tfs) as hA, _handle(gvamd, cam, s.tfs) as hB:
        for h in (hA, hB):
            h.upload_xyz(s.x, s.y, s.z)
        r = hA.tick(b, k_near=4, vision=True, net=net)
        bdepth = hB.compute_depth_for_bboxes(st, 4)[0]
        bposes = hB.transform_lshape_objects(hB.vision_post_process(*net, dy))
        hB.update_map_poses(bposes)
        assert r["n_static"] == len(st) and r["n_dynamic"] == len(dy) and r["pca_empty"] is False
        assert r["depths"].tobytes() == bdepth.tobytes() and np.array_equal(r["depths"], edepth)
        assert r["base_points"].tobytes() == np.ascontiguousarray(hB.convert_pixels_to_3d(st, bdepth)).tobytes()
        assert np.array_equal(r["base_points"], epts)
        assert r["poses"].tobytes() == bposes.tobytes() and len(r["poses"]) == len(want)
        for i, (p, e) in enumerate(zip(r["poses"], want)):
            _check_pose(p, e, ("vision", i))
        assert np.array_equal(hA.log_odds(), hB.log_odds())
        og.update_map_poses(r["poses"])
        assert check_grid(hA, og)[0] == 0


# ------------------------------------------------------------------------- 8. nothing stale between table sizes --

def test_nothing_stale_between_table_sizes(gvamd):
    """one kitti handle: a 257-box call (five mask words, ensure_det grows), a 1-box call, a 64-box frame (one mask
    word again, fused), then the 257 boxes once more: each equals the oracle"""
    cam_name, sizes = STALE_CASE
    s, g = cc.scene(cam_name, True), cc.geo(cam_name, True)
    sets = {nb: cc.box_set(cam_name, True, nb).boxes for nb in sizes}
    poses = cc.grid_poses(TILE_GRID)
    og = ol.OGrid(*TILE_GRID)
    with _handle(gvamd, s.cam, s.tfs) as h:
        h.upload_xyz(s.x, s.y, s.z)
        for nb in sizes[:2]:
            ids, counts = h.extract_cloud_per_bbox(sets[nb])
            want = g.ids(sets[nb])
            assert np.array_equal(ids, want), nb
            assert np.array_equal(counts, np.bincount(want[want >= 0], minlength=nb)), nb
        h.process_frame(_full(gvamd), bboxes=sets[sizes[2]], poses=poses)
        _hold_frame(h, og, s, sets[sizes[2]], poses, "frame")
        assert np.array_equal(h.extract_cloud_per_bbox(sets[sizes[0]])[0], g.ids(sets[sizes[0]]))
        h.process_frame(_full(gvamd), bboxes=sets[sizes[0]], poses=poses)
        _hold_frame(h, og, s, sets[sizes[0]], poses, "frame-257")
