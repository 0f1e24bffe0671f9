"""[EXTENSION] X15 the tick's detection list on the device and the tracker fed from it.

The reference is always the host path: gv_tick_wait's poses, and gv_track_update with those poses as host detections on
a second handle.  A 640 x 480 camera, clouds of a few thousand points, a 200 x 200 grid; every tick is made three times
and must give the same bytes.

Vision branch: a tick's dynamic boxes are exactly the four classes the orientation post-process keeps (gv_filter_bboxes
and k_vision switch on the same labels), so every dynamic box of a vision tick is valid and the list's selection is
exercised there by the counts alone; the validity patterns run on the PCA branch (boxes without points, boxes with too
few) and, with every pattern, on the host twin (test_tick_track_host.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tick_track_cases as cases
from gvamd import synth
from test_gpu_parity import make_handle

pytestmark = pytest.mark.gpu

GV_ERR_BAD_ARG, GV_ERR_STATE = 1, 5
UNIT = 2.0 ** -53
# The vision branch's quaternion starts from the device's fp64 sincos(-orient / 2) instead of the host's sin and cos.
# Largest |difference| of a quaternion component against gv_tick_wait's over every box of test_vision_list, measured on
# the MI355X, in units of 2^-53; the bound is twice that (as test_gpu_pose.py does for its sin and cos).
Q_MEASURED_UNITS = 1.5
Q_BOUND_UNITS = 2.0 * Q_MEASURED_UNITS
_HANDLES = {}


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    yield m
    for h, _ in _HANDLES.values():
        h.close()
    _HANDLES.clear()


def _handle(gvamd, name, perturbed=True):
    """a 200 x 200 handle, kept for the module; the tracker and X13 off, the tracks empty"""
    if name not in _HANDLES:
        _HANDLES[name] = make_handle(gvamd, 1, perturbed=perturbed)
    h, tfs = _HANDLES[name]
    h.set_track_config(None)
    h.set_dyn_config(None)
    h.set_moving_objects(None)
    return h, tfs


def _code(gvamd, call):
    with pytest.raises(gvamd.GVError) as e:
        call()
    return e.value.code


def _thrice(h, boxes, **kw):
    """the flagged tick three times: (result, (records, n, n_total)) of the last, all three equal"""
    seen = []
    for _ in range(3):
        h.tick_enqueue(boxes, keep_dets=True, **kw)
        r = h.tick_wait()
        lst = h.tick_dets()
        seen.append((r["poses"].tobytes(), r["pca_empty"], lst[0].tobytes(), lst[1], lst[2]))
    assert seen[0] == seen[1] == seen[2]
    return r, lst


def _q_units(a, b):
    if not len(a):
        return 0.0
    d = [np.abs(a[k] - b[k]) for k in cases.Q]
    assert all(np.isfinite(x).all() for x in d)
    return float(max(x.max() for x in d) / UNIT)


def _check_list(lst, poses, q_bound=None, tag=None):
    """the list against gv_tick_wait's poses: counts, zero tail, bytes (q_bound: the quaternion by tolerance)"""
    rec, n, n_total = lst
    assert n_total == len(poses) and n == min(n_total, 128), (tag, n, n_total, len(poses))
    assert not rec[n:].tobytes().strip(b"\0"), tag
    if q_bound is None:
        assert rec[:n].tobytes() == poses[:n].tobytes(), tag
        return 0.0
    for k in cases.NOT_Q:
        assert rec[k][:n].tobytes() == poses[k][:n].tobytes(), (tag, k)
    worst = _q_units(rec[:n], poses[:n])
    return worst


def _small_cloud(h, n=3000):
    x, y, z, _ = synth.cloud_uniform(1, n)
    h.upload_xyz(x, y, z)


def _vision_boxes(nd, seed=0):
    """nd dynamic boxes with a static one after every third, and their network outputs (one box's residuals all NaN)"""
    n_all = nd + nd // 3 + (1 if nd == 0 else 0)
    b = synth.detections(3, n_all, seed_extra=seed)
    dyn = 0
    for i in range(n_all):
        static = i % 4 == 3 or nd == 0
        b["label"][i] = cases.STATIC_LABEL if static else cases.DYNAMIC_LABELS[dyn % 4]
        dyn += 0 if static else 1
    assert dyn == nd
    orient, conf, dims = synth.network_outputs(max(nd, 1), seed=11 + seed)
    orient, conf, dims = orient[:nd].copy(), conf[:nd].copy(), dims[:nd].copy()
    if nd >= 5:
        dims[3] = np.nan
    return b, (orient, conf, dims)


# ------------------------------------------------------------------------------------------------- 1 vision list --
def test_vision_list(gvamd):
    h, _ = _handle(gvamd, "a")
    _small_cloud(h)
    worst = 0.0
    for nd in cases.COUNTS:
        b, net = _vision_boxes(nd, seed=nd)
        r, lst = _thrice(h, b, k_near=4, vision=True, net=net)
        assert len(r["poses"]) == nd and r["n_dynamic"] == nd and r["n_static"] == len(b) - nd
        w = _check_list(lst, r["poses"], q_bound=Q_BOUND_UNITS, tag=nd)
        print(f"vision list, {nd} dynamic boxes: quaternion differs from gv_tick_wait's by at most {w:.3f} x 2^-53")
        worst = max(worst, w)
        if nd >= 5:
            assert np.isnan(lst[0]["length"][3]) and lst[0]["px"][3] == r["poses"]["px"][3]
    print(f"vision list: largest quaternion difference over all boxes {worst:.3f} x 2^-53 (bound {Q_BOUND_UNITS})")
    assert worst <= Q_BOUND_UNITS
    # the network did not run for every box: no poses, an empty list
    b, net = _vision_boxes(5)
    h.tick_enqueue(b, k_near=4, vision=True, keep_dets=True)
    r = h.tick_wait()
    assert len(r["poses"]) == 0
    _check_list(h.tick_dets(), r["poses"])


# ---------------------------------------------------------------------------------------------------- 2 PCA list --
@pytest.mark.parametrize("pattern", [p for p in cases.PATTERNS if p != "empty"])
def test_pca_list_patterns(gvamd, pattern):
    h, tfs = _handle(gvamd, "a")
    for n_all in cases.COUNTS:
        valid = cases.validity(pattern, n_all)
        x, y, z, b = cases.pca_scene(tfs, valid, seed=n_all)
        h.upload_xyz(x, y, z)
        r, lst = _thrice(h, b, k_near=4)
        assert not r["pca_empty"] or r["n_dynamic"] == 0, (pattern, n_all)
        want = int(valid.sum()) if r["n_dynamic"] else 0      # computeBBoxPose runs when a dynamic box is there
        assert len(r["poses"]) == want, (pattern, n_all, len(r["poses"]), want)
        _check_list(lst, r["poses"], tag=(pattern, n_all))


def test_pca_list_special_scenes(gvamd):
    h, tfs = _handle(gvamd, "a")
    # some boxes valid, some with too few points for the radius filter, some with none
    valid = cases.validity("alternating", 40)
    x, y, z, b = cases.pca_scene(tfs, valid, seed=5, few=(1, 5, 9))
    h.upload_xyz(x, y, z)
    r, lst = _thrice(h, b, k_near=4)
    assert len(r["poses"]) == 20 and not r["pca_empty"]
    _check_list(lst, r["poses"], tag="few")
    # all ground: the device poses exist, the list is empty
    gx, gy, gz = cases.ground(tfs["cam_lidar"], 4000, 9)
    h.upload_xyz(gx, gy, gz)
    r, lst = _thrice(h, cases.grid_boxes(12), k_near=4)
    assert r["pca_empty"] and len(r["poses"]) == 0
    _check_list(lst, r["poses"], tag="all ground")
    # a cloud of two points
    h.upload_xyz(gx[:2], gy[:2], gz[:2])
    r, lst = _thrice(h, cases.grid_boxes(12), k_near=2)
    assert r["pca_empty"] and len(r["poses"]) == 0
    _check_list(lst, r["poses"], tag="two points")
    # no boxes; static boxes only
    x, y, z, b = cases.pca_scene(tfs, np.ones(8, np.uint8), seed=6)
    h.upload_xyz(x, y, z)
    r, lst = _thrice(h, None, k_near=4)
    assert len(r["poses"]) == 0
    _check_list(lst, r["poses"], tag="no boxes")
    b["label"] = cases.STATIC_LABEL
    r, lst = _thrice(h, b, k_near=4)
    assert len(r["poses"]) == 0 and r["n_static"] == 8
    _check_list(lst, r["poses"], tag="static only")


def test_host_twin_equals_public_transform(gvamd):
    """the list's host twin against gv_transform_lshape_objects applied to the valid poses in order, cut at 128, byte for
    byte (the handle only lends its transform), on every branch of the basis -> quaternion step"""
    reached = set()
    for t, tf in enumerate(cases.branch_transforms()):
        h, _ = _handle(gvamd, "tf")
        h.set_transforms(base_cam=tf)
        for cam in (cases.cam_poses(150, 10 + t), cases.pitch_poses(90, 20 + t), cases.cam_poses(40, 30 + t, unit_q=False)):
            cam["px"][0], cam["py"][1], cam["pz"][2] = np.nan, np.inf, -np.inf
            reached |= {cases.quat_branch(tf, p) for p in cam}
            valid = cases.validity("alternating", len(cam))
            got, n, n_total = gvamd.tick_dets_host(cam, valid, tf)
            want = h.transform_lshape_objects(cam[valid.astype(bool)])
            assert n_total == len(want) and got[:n].tobytes() == want[:128].tobytes(), t
    assert reached >= {"trace", 0, 1, 2}, reached


# ------------------------------------------------------------------------------------------------ 3 track sequence --
DYN = dict(off_x=(0.0,), radius=0.5, influence_radius=2.5, cost_scaling_factor=1.0, quantum=0.125, t0=0.1, dt=0.1)


def _score_poses(h, K=5, P=12):
    p = np.zeros((K, P, 3), np.float32)
    p[:, :, 0] = h.pos_x - 10.0 + 2.0 * np.arange(P)[None, :]
    p[:, :, 1] = h.pos_y - 4.0 + 2.0 * np.arange(K)[:, None]
    return p


@pytest.mark.parametrize("branch", ["pca", "vision"])
def test_track_sequence(gvamd, branch):
    """8 ticks of two crossing objects, odd ticks with an ego motion: the device path on one handle (tick with the flag,
    update from the list enqueued before the tick's wait, fed to X13) and the host path on the other"""
    (hA, tfs), (hB, _) = _handle(gvamd, "a"), _handle(gvamd, "b")
    q_bound = Q_BOUND_UNITS if branch == "vision" else None
    for h in (hA, hB):
        h.set_track_config(gvamd.TrackConfig.of(gate=2.0 if branch == "pca" else 6.0))
        h.set_dyn_config(gvamd.DynConfig.of(**DYN))
        if branch == "vision":
            _small_cloud(h)
    net = tuple(a[:2] for a in synth.network_outputs(2, seed=5))
    poses = _score_poses(hA)
    matched = 0
    for t in range(8):
        if branch == "pca":
            x, y, z, b = cases.moving_scene(tfs, t)
            for h in (hA, hB):
                h.upload_xyz(x, y, z)
            kw = dict(k_near=4)
        else:
            b = cases.moving_boxes(t, half=(60, 45), rows=(150.0, 330.0))
            kw = dict(k_near=4, vision=True, net=net)
        motion, dt = cases.ego_motion(t), 0.1
        info_a, tracks_a = np.zeros(1, gvamd.TRACK_INFO_DTYPE), np.zeros(gvamd.TRACK_SLOTS, gvamd.TRACK_DTYPE)
        hA.tick_enqueue(b, keep_dets=True, **kw)
        hA.track_update_async(None, dt, motion, feed=True, info=info_a, tracks=tracks_a, from_tick=True)
        rA = hA.tick_wait()
        hA.synchronize()
        rB = hB.tick(b, **kw)
        assert len(rB["poses"]) == 2 and rA["poses"].tobytes() == rB["poses"].tobytes(), (branch, t)
        info_b, tracks_b = hB.track_update(rB["poses"][:128], dt, motion, feed=True)
        assert info_a.tobytes() == np.array([info_b]).tobytes(), (branch, t, info_a, info_b)
        (sa, ida), (sb, idb) = hA.get_tracks(), hB.get_tracks()
        assert ida == idb and len(sa) == len(sb) == int(info_b["n_tracks"])
        for got, want in ((sa, sb), (tracks_a[:len(tracks_b)], tracks_b)):
            if q_bound is None:
                assert got.tobytes() == want.tobytes(), (branch, t)
            else:
                for k in got.dtype.names:
                    if k not in cases.Q:
                        assert got[k].tobytes() == want[k].tobytes(), (branch, t, k)
                assert _q_units(got, want) <= q_bound, (branch, t, _q_units(got, want))
        assert not tracks_a[len(tracks_b):].tobytes().strip(b"\0")
        assert hA.score_dynamic(poses).tobytes() == hB.score_dynamic(poses).tobytes(), (branch, t)
        matched += int(info_b["n_matched"])
        print(f"{branch} tick {t}: {dict(zip(info_b.dtype.names, info_b.tolist()))}")
    if branch == "pca":
        assert matched >= 10 and int(info_b["n_exported"]) == 2      # the two objects are tracked, not born again each tick


# ----------------------------------------------------------------------------------------------------------- 4 order --
def _pca_tick_inputs(tfs, seed):
    valid = cases.validity("alternating", 30)
    return cases.pca_scene(tfs, valid, seed=seed)


def test_order(gvamd):
    (hA, tfs), (hB, _) = _handle(gvamd, "a"), _handle(gvamd, "b")
    cfg = gvamd.TrackConfig.of(gate=2.0)
    x, y, z, b = _pca_tick_inputs(tfs, 21)
    x2, y2, z2, b2 = cases.pca_scene(tfs, cases.validity("all", 9), seed=22)
    # between enqueue and wait == after the wait; twice from one list == the host path fed the list twice
    for h in (hA, hB):
        h.set_track_config(cfg)
        h.upload_xyz(x, y, z)
    hA.tick_enqueue(b, k_near=4, keep_dets=True)
    hA.track_update_async(None, 0.1, from_tick=True)
    hA.track_update_async(None, 0.1, from_tick=True)
    rA = hA.tick_wait()
    hB.tick_enqueue(b, k_near=4, keep_dets=True)
    rB = hB.tick_wait()
    hB.track_update(None, 0.1, from_tick=True)
    hB.track_update(None, 0.1, from_tick=True)
    assert len(rA["poses"]) == 15 and rA["poses"].tobytes() == rB["poses"].tobytes()
    (sa, ida), (sb, idb) = hA.get_tracks(), hB.get_tracks()
    assert sa.tobytes() == sb.tobytes() and ida == idb == 16 and (sa["hits"] == 2).all()
    hB.set_tracks(None, 1)
    hB.track_update(rB["poses"], 0.1)
    hB.track_update(rB["poses"], 0.1)
    assert hB.get_tracks()[0].tobytes() == sa.tobytes()
    # tick A, update, wait, tick B of another scene, then synchronise: the tracks are those of A's list
    hA.set_tracks(None, 1)
    hA.tick_enqueue(b, k_near=4, keep_dets=True)
    hA.track_update_async(None, 0.1, from_tick=True)
    hA.tick_wait()
    hA.upload_xyz(x2, y2, z2)
    hA.tick_enqueue(b2, k_near=4, keep_dets=True)
    hA.synchronize()
    r2 = hA.tick_wait()
    hB.set_tracks(None, 1)
    hB.track_update(rB["poses"], 0.1)
    assert hA.get_tracks()[0].tobytes() == hB.get_tracks()[0].tobytes() and len(r2["poses"]) == 9
    # and the next update reads B's list
    hA.track_update(None, 0.1, from_tick=True)
    hB.track_update(r2["poses"], 0.1)
    assert hA.get_tracks()[0].tobytes() == hB.get_tracks()[0].tobytes()


# ---------------------------------------------------------------------------------------------------------- 5 errors --
def test_errors(gvamd):
    h, tfs = _handle(gvamd, "err")
    lib = gvamd.load()
    z = cases.pitch_poses(2, 1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def upd(dets, n, flags):
        return lib.gv_track_update(h._h, dets, C.c_int32(n), C.c_double(0.1), None, C.c_uint32(flags), None, None)

    x, y, zz, b = _pca_tick_inputs(tfs, 31)
    h.upload_xyz(x, y, zz)
    assert upd(None, 0, gvamd.TRACK_TICK_DETS) == GV_ERR_STATE                     # no configuration
    h.set_track_config(gvamd.TrackConfig.of(gate=2.0))
    if not h._lib.gv_test_tick_dets(h._h, p(np.zeros(128, synth.LSHAPE_DTYPE)), C.byref(C.c_int32()), C.byref(C.c_int32())):
        pytest.fail("a handle that never ran a flagged tick has a list")
    assert upd(None, 0, gvamd.TRACK_TICK_DETS) == GV_ERR_STATE                     # no tick enqueued yet
    h.tick(b, k_near=4)
    assert upd(None, 0, gvamd.TRACK_TICK_DETS) == GV_ERR_STATE                     # the last tick had no flag
    h.track_update(z, 0.1)
    before = h.get_tracks()
    assert len(before[0]) == 2
    h.tick(b, k_near=4, keep_dets=True)
    assert upd(p(z), 2, gvamd.TRACK_TICK_DETS) == GV_ERR_BAD_ARG                   # dets with the flag
    assert upd(p(z), 0, gvamd.TRACK_TICK_DETS) == GV_ERR_BAD_ARG
    assert upd(None, 0, gvamd.TRACK_TICK_DETS | gvamd.TRACK_DEVICE_DETS) == GV_ERR_BAD_ARG
    assert upd(None, 0, gvamd.TRACK_TICK_DETS | 8) == GV_ERR_BAD_ARG              # an unknown flag
    assert upd(None, 0, 8) == GV_ERR_BAD_ARG
    h.tick(b, k_near=4)                                                            # flagged, then unflagged
    assert upd(None, 0, gvamd.TRACK_TICK_DETS) == GV_ERR_STATE
    assert _code(gvamd, h.tick_dets) == GV_ERR_STATE
    h.tick_enqueue(b, k_near=4)
    assert upd(None, 0, gvamd.TRACK_TICK_DETS) == GV_ERR_STATE                     # pending and unflagged
    h.tick_wait()
    h.set_track_config(None)
    h.tick(b, k_near=4, keep_dets=True)
    assert upd(None, 0, gvamd.TRACK_TICK_DETS) == GV_ERR_STATE                     # a list, but no configuration
    h.set_track_config(gvamd.TrackConfig.of(gate=2.0))
    h.set_tracks(*before)
    after = h.get_tracks()
    assert after[0].tobytes() == before[0].tobytes() and after[1] == before[1]
    for call in (lambda: upd(p(z), 2, gvamd.TRACK_TICK_DETS), lambda: upd(None, 0, gvamd.TRACK_TICK_DETS | 1)):
        assert call() == GV_ERR_BAD_ARG
        now = h.get_tracks()
        assert now[0].tobytes() == before[0].tobytes() and now[1] == before[1]       # every refused call left the tracks alone
    assert upd(None, 0, gvamd.TRACK_TICK_DETS) == 0                                # and the good call goes through
    assert len(h.get_tracks()[0]) >= 15


def test_refused_updates_leave_the_tracks(gvamd):
    """after each STATE error the resident tracks are what they were"""
    h, tfs = _handle(gvamd, "err")
    x, y, z, b = _pca_tick_inputs(tfs, 32)
    h.upload_xyz(x, y, z)
    h.set_track_config(gvamd.TrackConfig.of(gate=2.0))
    h.set_tracks(None, 1)
    h.track_update(cases.pitch_poses(3, 2), 0.1)
    before = h.get_tracks()
    h.tick(b, k_near=4)
    assert _code(gvamd, lambda: h.track_update(None, 0.1, from_tick=True)) == GV_ERR_STATE
    h.tick(b, k_near=4, keep_dets=True)
    h.tick(b, k_near=4)
    assert _code(gvamd, lambda: h.track_update_async(None, 0.1, from_tick=True)) == GV_ERR_STATE
    now = h.get_tracks()
    assert now[0].tobytes() == before[0].tobytes() and now[1] == before[1] and len(now[0]) == 3


# --------------------------------------------------------------------------------------------- 6 nothing else moves --
@pytest.mark.parametrize("branch", ["pca", "pca_lidar", "vision"])
def test_flag_changes_nothing_else(gvamd, branch):
    (hA, tfs), (hB, _) = _handle(gvamd, "a"), _handle(gvamd, "b")
    pins = [gvamd.PinnedI8(hA.G) for _ in range(2)]
    try:
        if branch == "vision":
            b, net = _vision_boxes(40, seed=3)
            kw = dict(k_near=4, vision=True, net=net)
            for h in (hA, hB):
                _small_cloud(h)
        else:
            x, y, z, b = cases.pca_scene(tfs, cases.validity("alternating", 40), seed=41)
            kw = dict(k_near=4, lidar_bin=branch == "pca_lidar", lidar_raymarch=branch == "pca_lidar")
            for h in (hA, hB):
                h.upload_xyz(x, y, z)
        for h in (hA, hB):
            h.reset()
        for rep in range(3):
            hA.tick_enqueue(b, grid_out=pins[0].array, keep_dets=True, **kw)
            rA = hA.tick_wait()
            hB.tick_enqueue(b, grid_out=pins[1].array, **kw)
            rB = hB.tick_wait()
            for k in ("n_static", "n_dynamic", "pca_empty"):
                assert rA[k] == rB[k], (branch, k)
            for k in ("static_bboxes", "depths", "base_points", "poses"):
                assert rA[k].tobytes() == rB[k].tobytes(), (branch, k)
            assert len(rA["poses"]) > 0 and len(rA["depths"]) > 0
            assert pins[0].array.tobytes() == pins[1].array.tobytes(), branch
            assert hA.log_odds().tobytes() == hB.log_odds().tobytes() and hA.to_occupancy_grid()[0].tobytes() == hB.to_occupancy_grid()[0].tobytes()
    finally:
        for q in pins:
            q.close()


# ------------------------------------------------------------------------------------------------------------ 7 flow --
def test_tick_track_demo(gvamd, tmp_path):
    """examples/tick_track_demo.cpp (plain g++ over the C ABI): one tick sequence through the host path and the device
    path on two handles, then tick -> update(feed) -> gv_mppi_cycle_async with one wait, then the frame flow with and
    without FlowParams::track_on_device"""
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "grid-vision_amd")
    exe = str(tmp_path / "tick_track_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(pkg, "examples", "tick_track_demo.cpp"), "-o", exe,
                           "-L" + pkg, "-lgridvision_hip", "-Wl,-rpath," + pkg])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert "tracks agree on every tick" in out.stdout and "one wait" in out.stdout, out.stdout
    assert "flow tracks agree" in out.stdout and "tick track check ok" in out.stdout, out.stdout      # FlowParams::track_on_device
