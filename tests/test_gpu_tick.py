"""The node's tick between gv_tick_enqueue and gv_tick_wait (include/gridvision_hip.h: cloud uploads, gv_frame_* and the
grid getters may be called there, ordered behind the tick on gv_stream), the result reflecting the handle's state at
enqueue, and computeBBoxPose's empty segmented cloud (cloud_detections.cpp:307-309) against the oracle.

The pattern is twin handles: hA gets the calls in between, hB runs the same tick with nothing in between and makes the
same later calls after its wait.  Everything the two return is compared byte for byte."""
import functools

import numpy as np
import pytest

import oracle_lib as ol
from gvamd import synth
from test_gpu_parity import _base_poses, _check_pose, _ground_scene, _large_scene, _pose_reference, check_grid, make_handle

pytestmark = pytest.mark.gpu

GV_ERR_STATE = 5


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


@functools.lru_cache(maxsize=None)
def _scene(n_total=1_000_000, seed=17):
    """_large_scene of the perturbed transforms (make_handle(..., perturbed=True)), made once per module"""
    return _large_scene(synth.transforms(True), n_total=n_total, seed=seed)


def _same_result(ra, rb, tag):
    for k in ("n_static", "n_dynamic", "pca_empty"):
        assert ra[k] == rb[k], (tag, k, ra[k], rb[k])
    for k in ("static_bboxes", "depths", "base_points", "poses"):
        assert ra[k].tobytes() == rb[k].tobytes(), (tag, k)


def _grid_state(h, hits=False):
    s = {"log_odds": h.log_odds(), "occupancy": h.occupancy(), "i8": h.to_occupancy_grid()[0]}
    if hits:
        s["hits"] = h.hits()
    return s


def _same_grid(a, b, tag):
    assert a.keys() == b.keys(), tag
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (tag, k)


# ---------------------------------------------------------------------------------------- uploads in between --

class _Uploads:
    """One upload pattern: the host buffers (pinned where the call is asynchronous) live as long as this object, so
    both handles upload the same bytes and nothing is freed before upload_wait."""

    def __init__(self, gvamd, pattern):
        x, y, z, _ = _scene()
        self.pins, self.calls = [], []

        def sub(lo, n):   # the scene is shuffled: any slice holds ground, objects and clutter
            return x[lo:lo + n], y[lo:lo + n], z[lo:lo + n]

        def pinned(a):
            p = gvamd.PinnedF32(len(a))
            p.array[:] = a
            self.pins.append(p)
            return p.array

        def xyz_async(c):
            px, py, pz = (pinned(a) for a in c)
            self.calls.append(lambda h: h.upload_xyz_async(px, py, pz))
            self.last = c

        def xyz_sync(c):
            cx, cy, cz = (np.array(a, np.float32) for a in c)
            self.calls.append(lambda h: h.upload_xyz(cx, cy, cz))
            self.last = c

        def pc2_async(c):
            n = len(c[0])
            p = gvamd.PinnedF32(4 * n)
            self.pins.append(p)
            rec = p.array.reshape(n, 4)
            rec[:, 0], rec[:, 1], rec[:, 2] = c
            rec[:, 3] = np.arange(n, dtype=np.float32)   # intensity: bytes the de-interleave must skip
            data = p.array.view(np.uint8)
            self.calls.append(lambda h: h.upload_pointcloud2_async(data, n, 16, 0, 4, 8))
            self.last = c

        if pattern == "xyz_async":
            for lo, n in ((0, 3001), (5000, 4500), (12000, 2222)):
                xyz_async(sub(lo, n))
        elif pattern == "xyz_sync_wrap":   # the third lands in the tick's set, the fourth goes past it
            for lo, n in ((0, 2500), (5000, 3333), (9000, 4096), (15000, 1801)):
                xyz_sync(sub(lo, n))
        elif pattern == "pointcloud2_async":
            for lo, n in ((0, 2900), (4000, 3700), (9000, 4101)):
                pc2_async(sub(lo, n))
        elif pattern == "grow":   # the third is larger than the tick's set: that set is reallocated
            big = _scene(1_500_000, 31)[:3]
            for c in (sub(0, 3000), sub(5000, 4444), big):
                xyz_async(c)
        else:
            raise ValueError(pattern)

    def push(self, h):
        for call in self.calls:
            call(h)

    def close(self):
        for p in self.pins:
            p.close()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("pattern", ["xyz_async", "xyz_sync_wrap", "pointcloud2_async", "grow"])
@pytest.mark.parametrize("lidar", [False, True], ids=["pca", "pca_lidar"])
def test_tick_uploads_between_enqueue_and_wait(gvamd, lidar, pattern):
    """Clouds uploaded while a tick is pending: the tick reads the cloud it was enqueued on to the end (the third upload
    rotates back into the tick's set and must wait for the tick on the device), its result and its grid equal the twin's
    tick with nothing in between, the last upload ends up resident and intact, and the two handles go on identically."""
    hA, tfs = make_handle(gvamd, 3, perturbed=True)
    hB, _ = make_handle(gvamd, 3, perturbed=True)
    x, y, z, b = _scene()
    st, dy = gvamd.filter_bboxes(b)
    assert len(st) >= 5 and len(dy) >= 20   # static boxes: the kNN runs on a lane beside the pose branch
    kw = dict(k_near=4, lidar_bin=lidar, lidar_raymarch=lidar)
    ups = _Uploads(gvamd, pattern)
    pins = [gvamd.PinnedI8(hA.G) for _ in range(4)]
    try:
        for h in (hA, hB):
            h.upload_xyz(x, y, z)
        hA.tick_enqueue(b, grid_out=pins[0].array, **kw)
        ups.push(hA)
        rA = hA.tick_wait()
        gA = _grid_state(hA, lidar)
        rB = hB.tick(b, grid_out=pins[1].array, **kw)
        gB = _grid_state(hB, lidar)
        ups.push(hB)
        assert not rA["pca_empty"] and len(rA["poses"]) >= 20 and len(rA["depths"]) == len(st)
        _same_result(rA, rB, pattern)
        assert pins[0].array.tobytes() == pins[1].array.tobytes()
        assert np.array_equal(pins[0].array, gA["i8"])
        _same_grid(gA, gB, pattern)
        for h in (hA, hB):
            h.upload_wait()
        # the resident cloud is the last upload, bit for bit
        lx, ly, lz = ups.last
        ex, ey, ez = ol.transform_cloud(ol.tf_to_matrix4f(tfs["cam_lidar"]), lx, ly, lz)
        for h in (hA, hB):
            assert h.n == len(lx)
            gx, gy, gz = h.transform_lidar_to_camera()
            assert np.array_equal(gx, ex) and np.array_equal(gy, ey) and np.array_equal(gz, ez)
        # and on it the two handles agree call for call
        dA, d2A = hA.compute_depth_for_bboxes(st, 4)
        dB, d2B = hB.compute_depth_for_bboxes(st, 4)
        assert dA.tobytes() == dB.tobytes() and d2A.tobytes() == d2B.tobytes()
        mA, maskA, cA = hA.segment_ground_plane()
        mB, maskB, cB = hB.segment_ground_plane()
        assert mA == mB and maskA.tobytes() == maskB.tobytes() and cA.tobytes() == cB.tobytes()
        r2A = hA.tick(b, grid_out=pins[2].array, **kw)
        r2B = hB.tick(b, grid_out=pins[3].array, **kw)
        _same_result(r2A, r2B, (pattern, "next tick"))
        assert pins[2].array.tobytes() == pins[3].array.tobytes()
        _same_grid(_grid_state(hA, lidar), _grid_state(hB, lidar), (pattern, "next tick"))
    finally:
        for p in pins:
            p.close()
        hA.close(); hB.close()
        ups.close()


# ------------------------------------------------------------------------------------ state at enqueue --

@pytest.mark.parametrize("case", ["cloud_of_m_points", "all_ground_then_smaller_cloud", "base_cam_set"])
def test_tick_result_uses_state_at_enqueue(gvamd, case):
    """gv_tick_wait reports the tick that was enqueued: the cloud size that decides "empty segmented cloud" and the
    camera->base transform of the poses and base points are the handle's at enqueue, not whatever was uploaded or set
    while the tick ran.
      cloud_of_m_points              a cloud of exactly m points (m = the tick's inlier count) uploaded in between
      all_ground_then_smaller_cloud  an all-ground tick (empty segmented cloud), a smaller cloud uploaded in between
      base_cam_set                   a new camera->base transform set in between: in effect from the next tick on"""
    hA, tfs = make_handle(gvamd, 2, perturbed=True)
    hB, _ = make_handle(gvamd, 2, perturbed=True)
    x, y, z, K, b = _ground_scene(tfs, seed=9)
    st, dy = gvamd.filter_bboxes(b)
    assert len(st) >= 1 and len(dy) >= 5
    pinA, pinB = gvamd.PinnedI8(hA.G), gvamd.PinnedI8(hB.G)
    try:
        for h in (hA, hB):
            h.upload_xyz(x, y, z)
        # m = the tick's own inlier count: its pose branch is computeBBoxPose with ground removal, call for call
        pp, valid, npz = hB.compute_bbox_pose_ground_removed(b)
        m = hB.segment_ground_plane()[0]
        assert npz >= 5 and 0 < m < len(x)
        want_poses = hB.transform_lshape_objects(pp[valid.astype(bool)])
        r0 = hB.tick(b, k_near=4)
        assert not r0["pca_empty"] and r0["poses"].tobytes() == want_poses.tobytes()
        hA.tick(b, k_near=4)   # the twins stay twins
        if case == "all_ground_then_smaller_cloud":
            rng = np.random.default_rng(4)
            n = 20_000
            gx_, gy_ = rng.uniform(1.0, 60.0, n).astype(np.float32), rng.uniform(-30.0, 30.0, n).astype(np.float32)
            for h in (hA, hB):
                h.upload_xyz(gx_, gy_, np.full(n, -1.5, np.float32))
        between = {"cloud_of_m_points": lambda h: h.upload_xyz(x[-m:], y[-m:], z[-m:]),
                   "all_ground_then_smaller_cloud": lambda h: h.upload_xyz(x[:5000], y[:5000], z[:5000]),
                   "base_cam_set": lambda h: h.set_transforms(base_cam=synth.transforms(False)["base_cam"])}[case]
        assert not np.array_equal(synth.transforms(False)["base_cam"], tfs["base_cam"])
        hA.tick_enqueue(b, k_near=4, grid_out=pinA.array)
        between(hA)
        rA = hA.tick_wait()
        rB = hB.tick(b, k_near=4, grid_out=pinB.array)
        between(hB)
        if case == "all_ground_then_smaller_cloud":
            assert rB["pca_empty"] and len(rB["poses"]) == 0
        else:
            assert not rB["pca_empty"] and len(rB["poses"]) >= 5 and len(rB["base_points"]) == len(st)
        _same_result(rA, rB, case)
        assert pinA.array.tobytes() == pinB.array.tobytes()
        _same_grid(_grid_state(hA), _grid_state(hB), case)
        # the next tick runs on what was uploaded / set in between, on both
        r2A = hA.tick(b, k_near=4, grid_out=pinA.array)
        r2B = hB.tick(b, k_near=4, grid_out=pinB.array)
        _same_result(r2A, r2B, (case, "next tick"))
        if case == "base_cam_set":
            assert r2A["poses"].tobytes() != rA["poses"].tobytes()   # the new transform is in effect now
        assert pinA.array.tobytes() == pinB.array.tobytes()
        _same_grid(_grid_state(hA), _grid_state(hB), (case, "next tick"))
    finally:
        pinA.close(); pinB.close()
        hA.close(); hB.close()


# ------------------------------------------------------------------------------ frames and getters in between --

def test_tick_frames_and_getters_between_enqueue_and_wait(gvamd):
    """gv_frame_*, the grid getters, gv_publish_grid_async and gv_update_map_poses between enqueue and wait are ordered
    behind the tick: the tick's own result and grid_out are those of the tick alone, every getter sees the grid with
    the tick applied, and the final grid equals the twin making the same calls after its wait.  The calls that would
    reuse the tick's result block or detection set are refused."""
    hA, tfs = make_handle(gvamd, 3, perturbed=True)
    hB, _ = make_handle(gvamd, 3, perturbed=True)
    x, y, z, b = _scene()
    flags = gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH
    poses = synth.lshape_poses(3, 8)
    outA, outB, pubA, pubB = (gvamd.PinnedI8(hA.G) for _ in range(4))

    def later(h, pub):
        h.set_detections(flags)
        h.enqueue_frame()
        h.enqueue_frame()
        lo = h.log_odds()
        i8 = h.to_occupancy_grid()[0]
        h.publish_grid_async(pub.array)
        h.update_map_poses(poses)
        return lo, i8

    try:
        for h in (hA, hB):
            h.upload_xyz(x, y, z)
        hA.tick_enqueue(b, k_near=4, grid_out=outA.array)
        loA, i8A = later(hA, pubA)
        for call in (lambda: hA.compute_depth_for_bboxes(b, 4), lambda: hA.compute_bbox_pose(b),
                     lambda: hA.segment_ground_plane(), lambda: hA.tick_enqueue(b, k_near=4)):
            with pytest.raises(gvamd.GVError) as e:
                call()
            assert e.value.code == GV_ERR_STATE
        rA = hA.tick_wait()
        finA = _grid_state(hA, hits=True)
        rB = hB.tick(b, k_near=4, grid_out=outB.array)
        tickB = _grid_state(hB)
        loB, i8B = later(hB, pubB)
        finB = _grid_state(hB, hits=True)
        assert not rA["pca_empty"] and len(rA["poses"]) >= 20
        _same_result(rA, rB, "frames and getters in between")
        # grid_out is the tick alone: not the frames enqueued behind it
        assert outA.array.tobytes() == outB.array.tobytes()
        assert np.array_equal(outB.array, tickB["i8"])
        assert not np.array_equal(outA.array, finA["i8"])
        # every getter saw the tick (and the frames queued before it), as the twin's after its wait
        assert loA.tobytes() == loB.tobytes() and i8A.tobytes() == i8B.tobytes()
        assert not np.array_equal(loB, tickB["log_odds"])
        assert pubA.array.tobytes() == pubB.array.tobytes() and np.array_equal(pubA.array, i8A)
        _same_grid(finA, finB, "final grid")
    finally:
        for p in (outA, outB, pubA, pubB):
            p.close()
        hA.close(); hB.close()


# ---------------------------------------------------------------------------- empty segmented cloud vs oracle --

def _point_in_dynamic_frustum(tfs, dy, K, height):
    """a lidar point `height` above the ground plane of _empty_case_cloud that projects into a dynamic box"""
    gx_, gy_ = np.meshgrid(np.arange(1.5, 60.0, 0.25), np.arange(-30.0, 30.0, 0.25))
    px, py = gx_.ravel().astype(np.float32), gy_.ravel().astype(np.float32)
    pz = np.full(len(px), -1.5 + height, np.float32)
    cx, cy, cz = ol.transform_cloud(ol.tf_to_matrix4f(tfs["cam_lidar"]), px, py, pz)
    ids = ol.extract_cloud_per_bbox(K, cx, cy, cz, dy, synth.IMG_W, synth.IMG_H)
    i = int(np.nonzero(ids >= 0)[0][0])
    return px[i], py[i], pz[i]


def _empty_case_cloud(kind, tfs, dy, K):
    rng = np.random.default_rng(8)
    f = np.float32
    if kind in ("all_ground", "ground_plus_one"):
        n = 20_000
        x, y, z = rng.uniform(1.0, 60.0, n).astype(f), rng.uniform(-30.0, 30.0, n).astype(f), np.full(n, -1.5, f)
        if kind == "ground_plus_one":
            p = _point_in_dynamic_frustum(tfs, dy, K, 1.0)
            x, y, z = np.append(x, p[0]), np.append(y, p[1]), np.append(z, p[2])
        return x, y, z
    if kind == "collinear":   # along the lidar x axis = the camera's optical axis: every sample's normal is exactly zero
        n = 3000
        return rng.uniform(2.0, 50.0, n).astype(f), np.full(n, 0.7, f), np.full(n, -0.4, f)
    if kind == "identical":
        n = 2000
        return np.full(n, 12.0, f), np.full(n, -0.8, f), np.full(n, -0.6, f)
    if kind == "three_points":
        return np.array([8.0, 14.0, 11.0], f), np.array([-1.0, 0.5, 2.0], f), np.array([-1.2, -0.3, 0.4], f)
    n = int(kind[1:])   # "n0", "n1", "n2"
    return np.array([9.0, 15.0][:n], f), np.array([0.3, -0.6][:n], f), np.array([-0.5, 0.2][:n], f)


@pytest.mark.parametrize("kind", ["all_ground", "ground_plus_one", "collinear", "identical", "three_points", "n0", "n1",
                                  "n2"])
def test_tick_empty_segmented_cloud_vs_oracle(gvamd, kind):
    """computeBBoxPose returns {} when the segmented cloud is empty (cloud_detections.cpp:307-309): no plane (em == 0,
    fewer than three points) or every point on it (em == n).  The tick's pca_empty is exactly that case, together with
    gv_compute_bbox_pose_ground_removed's -1; its poses are then empty and the grid is the decay-only updateMap.
    Depths and base points are the oracle's and the call sequence's, bit for bit.  The orientation-network branch
    never reports an empty segmented cloud."""
    hA, tfs = make_handle(gvamd, 2, perturbed=False)
    hB, _ = make_handle(gvamd, 2, perturbed=False)
    g = synth.CONFIGS[2]["grid"]
    og = ol.OGrid(g.grid_x, g.grid_y, g.resolution)
    K = ol.set_intrinsic(synth.FX, synth.FY, synth.CX, synth.CY)
    b = synth.detections(3, 12)
    st, dy = gvamd.filter_bboxes(b)
    assert len(st) >= 3 and len(dy) >= 2
    x, y, z = _empty_case_cloud(kind, tfs, dy, K)
    n = len(x)
    cx, cy, cz = ol.transform_cloud(ol.tf_to_matrix4f(tfs["cam_lidar"]), x, y, z)
    em, emask, _ = ol.segment_ground_plane(cx, cy, cz)
    want_em = {"all_ground": n, "ground_plus_one": n - 1, "collinear": 0, "identical": 0, "three_points": 3}.get(kind, 0)
    assert em == want_em, (kind, em)
    empty = em == 0 or em == n or n < 3
    # oracle: kNN depths of the static boxes and their base-frame points (convertPixelsTo3D)
    u, v, d = ol.project_points(K, cx, cy, cz)
    edepth, _ = ol.depth_for_bboxes(u, v, d, st, 4)
    kinv = ol.k_inverse(K)
    epts = np.array([ol.tf_point(tfs["base_cam"], ol.pixel_to_3d(
        np.float32(bb["x_min"] + ((bb["x_max"] - bb["x_min"]) / np.float32(2.0))),
        np.float32(bb["y_min"] + ((bb["y_max"] - bb["y_min"]) / np.float32(2.0))), dep, kinv)) for bb, dep in zip(st, edepth)])
    pin = gvamd.PinnedI8(hA.G)
    try:
        for h in (hA, hB):
            h.upload_xyz(x, y, z)
        r = hA.tick(b, k_near=4, grid_out=pin.array)
        # the call sequence on the twin
        bdepth = hB.compute_depth_for_bboxes(st, 4)[0]
        bpts = hB.convert_pixels_to_3d(st, bdepth)
        pp, valid, npz = hB.compute_bbox_pose_ground_removed(b)
        assert r["n_static"] == len(st) and r["n_dynamic"] == len(dy)
        assert r["pca_empty"] == empty, (kind, em, n)
        assert (npz == -1) == empty, (kind, npz)
        assert r["depths"].tobytes() == bdepth.tobytes() and np.array_equal(r["depths"], edepth)
        assert r["base_points"].tobytes() == np.ascontiguousarray(bpts).tobytes() and np.array_equal(r["base_points"], epts)
        assert r["poses"].tobytes() == hB.transform_lshape_objects(pp[valid.astype(bool)]).tobytes()
        if empty:
            assert len(r["poses"]) == 0
            og.update_map()
        else:
            keep = emask == 0
            _, ref = _pose_reference(cx[keep], cy[keep], cz[keep], K, b, lambda a, c, e: ol.radius_outlier(a, c, e, 0.4, 10).astype(bool))
            want = _base_poses(tfs, [e for ok, e, _, _ in ref if ok])
            assert len(r["poses"]) == len(want)
            for i, (p, e) in enumerate(zip(r["poses"], want)):
                _check_pose(p, e, (kind, i))
            og.update_map_poses(r["poses"])
        nlo, _, _ = check_grid(hA, og)
        assert nlo == 0
        assert np.array_equal(pin.array, hA.to_occupancy_grid()[0])
        # the orientation-network branch on the same cloud: poses from the network, never "empty segmented cloud"
        rv = hA.tick(b, k_near=4, vision=True, net=synth.network_outputs(len(dy)))
        assert rv["pca_empty"] is False
    finally:
        pin.close()
        hA.close(); hB.close()
