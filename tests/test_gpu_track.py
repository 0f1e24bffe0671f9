"""[EXTENSION] X14 the tracker over the tick's boxes on the device.

gv_track_update against the library's host twin gv_track_step (and so, by test_track_host.py, against track_ref) on
every family of track_cases, byte for byte: the info record, the tracks output, and the resident state read back with
gv_get_tracks.  Paths: pinned aligned / pinned misaligned / pageable destinations, device detections, five updates
enqueued without a wait, two handles, a pending tick, the state and argument rules.

The feed (GV_TRACK_FEED_DYNAMIC), always with every off_x 0 so that no sin or cos is involved: gv_score_dynamic after a
fed update against gv_dyn_score_poses over the twin's exported objects, a fed empty set, the stream order of fed and
host-set object sets, and the control step against gv_control_select_dyn over the reference records."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dyn_cases as dc
import dyn_ref
import rollout_ref
import track_cases as tc
import track_ref as ref
from planner_util import hip_runtime
from test_gpu_dyn import CONTROL_OBJS, _control_cfg, _cw, _scene, _step
from test_gpu_parity import _ground_scene, make_handle
from test_gpu_tick import _same_result

pytestmark = pytest.mark.gpu

GV_ERR_BAD_ARG, GV_ERR_STATE = 1, 5
W = rollout_ref.weights
EMPTY_RECORD = (0, -1, 0, -1, np.inf)
_HANDLES = {}


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    yield m
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()


def _handle(gvamd, name="main"):
    """a 500 x 200 handle with the tracker and X13 switched off and both sets emptied"""
    if name not in _HANDLES:
        _HANDLES[name] = gvamd.GridVisionHIP(50, 20, 0.1)
    h = _HANDLES[name]
    h.set_track_config(None)
    h.set_dyn_config(None)
    h.set_moving_objects(None)
    return h


def _code(gvamd, call):
    with pytest.raises(gvamd.GVError) as e:
        call()
    return e.value.code


def _twin(gvamd, c, n_steps=None):
    """the host twin over the case: per step (tracks, next_id, info array of 1, objs)"""
    cfg = ref.to_struct(gvamd, c["cfg"])
    tracks, next_id, out = c["tracks"], c["next_id"], []
    for s in c["steps"][:n_steps]:
        tracks, next_id, info, objs = gvamd.track_step(cfg, tracks, next_id, s["dets"], s["dt"], s["motion"])
        out.append((tracks, next_id, np.array([info]), objs))
    return out


def _load(h, gvamd, c):
    h.set_track_config(ref.to_struct(gvamd, c["cfg"]))
    h.set_tracks(c["tracks"], c["next_id"])


def _padded(tracks):
    out = np.zeros(128, ref.TRACK_DTYPE)
    out[:len(tracks)] = tracks
    return out.tobytes()


# -------------------------------------------------------------------------------------------------------- update --
@pytest.mark.parametrize("name", [c["name"] for c in tc.cases()])
def test_device_equals_host_twin(gvamd, name):
    c = tc.by_name(name)
    h = _handle(gvamd)
    _load(h, gvamd, c)
    got0, id0 = h.get_tracks()
    assert got0.tobytes() == np.ascontiguousarray(c["tracks"]).tobytes() and id0 == c["next_id"]
    for k, (s, (tracks, next_id, info, _), want) in enumerate(zip(c["steps"], _twin(gvamd, c), tc.want(c))):
        got_info, got_tracks = h.track_update(s["dets"], s["dt"], s["motion"])
        assert np.array([got_info]).tobytes() == info.tobytes() == want["info"].tobytes(), (name, k, got_info, info)
        assert got_tracks.tobytes() == tracks.tobytes() == want["tracks"].tobytes(), (name, k)
        state, nid = h.get_tracks()
        assert state.tobytes() == tracks.tobytes() and nid == next_id == want["next_id"], (name, k)


@pytest.mark.parametrize("name", ["filter", "chain_128", "invalid_dets"])
def test_destinations_and_device_detections(gvamd, name):
    """info and tracks into pinned memory aligned to 8 bytes (written by the kernel), into pinned memory that is not
    (the copy command) and into pageable memory; detections read in place from a hipMalloc buffer; either output left
    out: the same bytes every way, and the records of tracks behind the live ones are zero"""
    c = tc.by_name(name)
    h = _handle(gvamd)
    s = c["steps"][0]
    tracks, _, info, _ = _twin(gvamd, c, 1)[0]
    want_i, want_t = info.tobytes(), _padded(tracks)
    z = np.ascontiguousarray(s["dets"])
    hip, dptr = hip_runtime(), C.c_void_p()
    assert hip.hipMalloc(C.byref(dptr), max(z.nbytes, 80)) == 0
    pin_i, pin_t = gvamd.PinnedI8(40 + 16), gvamd.PinnedI8(128 * 128 + 16)
    try:
        assert hip.hipMemcpy(dptr, z.ctypes.data, z.nbytes, 1) == 0   # hipMemcpyHostToDevice
        for off in (0, 8, 4):
            for device in (False, True):
                pin_i.array[:] = 77
                pin_t.array[:] = 77
                i = pin_i.array[off:off + 40].view(ref.INFO_DTYPE)
                t = pin_t.array[off:off + 128 * 128].view(ref.TRACK_DTYPE)
                _load(h, gvamd, c)
                if device:
                    h.track_update_async(None, s["dt"], s["motion"], info=i, tracks=t, device_ptr=dptr.value, n=len(z))
                else:
                    h.track_update_async(z, s["dt"], s["motion"], info=i, tracks=t)
                h.synchronize()
                assert i.tobytes() == want_i and t.tobytes() == want_t, ("pinned", off, device)
        i, t = np.zeros(1, ref.INFO_DTYPE), np.full(128, 7, np.uint8).repeat(128).view(ref.TRACK_DTYPE)
        _load(h, gvamd, c)
        h.track_update_async(z, s["dt"], s["motion"], info=i, tracks=t)
        h.synchronize()
        assert i.tobytes() == want_i and t.tobytes() == want_t, "pageable"
        for keep in ("info", "tracks", None):
            pin_i.array[:] = 77
            pin_t.array[:] = 77
            i = pin_i.array[:40].view(ref.INFO_DTYPE)
            t = pin_t.array[:128 * 128].view(ref.TRACK_DTYPE)
            _load(h, gvamd, c)
            h.track_update_async(z, s["dt"], s["motion"], info=i if keep == "info" else None, tracks=t if keep == "tracks" else None)
            h.synchronize()
            assert (i.tobytes() == want_i) if keep == "info" else (pin_i.array == 77).all(), keep
            assert (t.tobytes() == want_t) if keep == "tracks" else (pin_t.array == 77).all(), keep
            assert h.get_tracks()[0].tobytes() == tracks.tobytes(), keep
    finally:
        hip.hipFree(dptr)
        pin_i.close()
        pin_t.close()


@pytest.mark.parametrize("name", ["ego_sequence", "filter"])
def test_five_updates_without_a_wait_and_two_handles(gvamd, name):
    """five updates enqueued back to back equal five twin steps, on two handles alike"""
    c = tc.by_name(name)
    want = _twin(gvamd, c, 5)
    hs = [_handle(gvamd), _handle(gvamd, "twin")]
    pins = [[(gvamd.PinnedI8(40), gvamd.PinnedI8(128 * 128)) for _ in range(5)] for _ in hs]
    try:
        for h, pp in zip(hs, pins):
            _load(h, gvamd, c)
            for s, (pi, pt) in zip(c["steps"], pp):
                pi.array[:] = 77
                pt.array[:] = 77
                h.track_update_async(np.ascontiguousarray(s["dets"]), s["dt"], s["motion"], info=pi.array.view(ref.INFO_DTYPE),
                                     tracks=pt.array.view(ref.TRACK_DTYPE))
        for h, pp in zip(hs, pins):
            h.synchronize()
            for k, ((tracks, _, info, _), (pi, pt)) in enumerate(zip(want, pp)):
                assert pi.array.tobytes() == info.tobytes() and pt.array.tobytes() == _padded(tracks), (name, k)
            state, nid = h.get_tracks()
            assert state.tobytes() == want[-1][0].tobytes() and nid == want[-1][1]
        assert pins[0][-1][1].array.tobytes() == pins[1][-1][1].array.tobytes()
    finally:
        for pp in pins:
            for pi, pt in pp:
                pi.close()
                pt.close()


def test_three_set_tracks_without_a_wait(gvamd):
    """The staging slots at their reuse edge: the third gv_set_tracks on a fresh handle fills the slot the first one used,
    which is the one host wait of the mechanism; the state is the last one's.  An update between the second and the third
    reads the second's.  (The same edge of the inflation table is test_gpu_inflate.py::test_reconfiguration_in_flight's,
    that of X13's object set and cost table test_gpu_dyn.py::test_set_and_configuration_are_stream_ordered's, that of the
    host detections test_five_updates_without_a_wait_and_two_handles'.)"""
    h = gvamd.GridVisionHIP(8, 8, 0.1)
    states = [(tc.tracks_at([(0.0, 0.0), (2.0, 1.0), (4.0, -1.0)], slots=[0, 5, 127]), 7),
              (tc.tracks_at([(1.0, 1.0)], slots=[3], v=[(0.5, -0.5)]), 0xFFFFFFFF),
              (tc.tracks_at([(-1.0, 0.5), (3.0, 3.0)], slots=[1, 2], first_id=40), 42)]
    cfg = ref.to_struct(gvamd, ref.config())
    twin_tracks, _, twin_info, _ = gvamd.track_step(cfg, states[1][0], states[1][1], tc.boxes_at([(1.0, 1.0)]), 0.0)
    pi, pt = gvamd.PinnedI8(40), gvamd.PinnedI8(128 * 128)
    try:
        h.set_track_config(cfg)
        for k, (tracks, next_id) in enumerate(states):
            h.set_tracks(tracks, next_id)
            if k == 1:
                h.track_update_async(tc.boxes_at([(1.0, 1.0)]), 0.0, info=pi.array.view(ref.INFO_DTYPE), tracks=pt.array.view(ref.TRACK_DTYPE))
        got, nid = h.get_tracks()
        assert got.tobytes() == np.ascontiguousarray(states[2][0]).tobytes() and nid == 42
        assert pi.array.tobytes() == np.array([twin_info]).tobytes() and pt.array.tobytes() == _padded(twin_tracks)
    finally:
        pi.close()
        pt.close()
        h.close()


def test_update_during_a_pending_tick(gvamd):
    """an update (and the other tracker calls) between gv_tick_enqueue and gv_tick_wait: the tick's result is that of the
    tick alone, the update's that of the twin"""
    h, tfs = make_handle(gvamd, 2, perturbed=True)
    other, _ = make_handle(gvamd, 2, perturbed=True)        # the same tick with nothing in between
    c = tc.by_name("ego_sequence")
    want = _twin(gvamd, c, 2)
    x, y, z, _, b = _ground_scene(tfs, seed=9)
    pi, pt = gvamd.PinnedI8(40), gvamd.PinnedI8(128 * 128)
    try:
        for q in (h, other):
            q.upload_xyz(x, y, z)
        alone = other.tick(b, k_near=4, lidar_bin=True)
        h.tick_enqueue(b, k_near=4, lidar_bin=True)
        _load(h, gvamd, c)
        s0, s1 = c["steps"][:2]
        h.track_update_async(np.ascontiguousarray(s0["dets"]), s0["dt"], s0["motion"], info=pi.array.view(ref.INFO_DTYPE),
                             tracks=pt.array.view(ref.TRACK_DTYPE))
        mid, _ = h.get_tracks()
        info1, tracks1 = h.track_update(s1["dets"], s1["dt"], s1["motion"])
        r = h.tick_wait()
        h.synchronize()
        _same_result(r, alone, "tracker calls in between")
        assert pi.array.tobytes() == want[0][2].tobytes() and pt.array.tobytes() == _padded(want[0][0])
        assert mid.tobytes() == want[0][0].tobytes()
        assert np.array([info1]).tobytes() == want[1][2].tobytes() and tracks1.tobytes() == want[1][0].tobytes()
    finally:
        pi.close()
        pt.close()
        h.close()
        other.close()


def test_state_and_argument_rules(gvamd):
    h = _handle(gvamd)
    z = tc.boxes_at([(1.0, 1.0), (5.0, 5.0)])
    assert _code(gvamd, lambda: h.track_update(z, 0.1)) == GV_ERR_STATE                  # no configuration
    got, nid = h.get_tracks()
    assert len(got) == 0 and nid == 1                                                      # the state after gv_create
    good = ref.config()
    h.set_track_config(ref.to_struct(gvamd, good))
    for bad in (dict(gate=0.0), dict(gate=np.nan), dict(sigma_accel=-1.0), dict(sigma_meas=0.0), dict(sigma_v0=np.inf),
                dict(min_speed=-1.0), dict(confirm_hits=0), dict(confirm_hits=256), dict(max_misses=-1), dict(max_misses=256), dict(flags=1)):
        assert _code(gvamd, lambda: h.set_track_config(ref.to_struct(gvamd, dict(good, **bad)))) == GV_ERR_BAD_ARG, bad
    info, tracks = h.track_update(z, 0.1)                                                  # the good configuration is in force
    assert int(info["n_born"]) == 2 and tracks["id"].tolist() == [1, 2]
    for dt in (-0.1, np.nan, np.inf):
        assert _code(gvamd, lambda: h.track_update(z, dt)) == GV_ERR_BAD_ARG
    assert _code(gvamd, lambda: h.track_update(z, 0.1, (0.0, 0.0, 0.0, 1.0, 0.0, np.inf, 0.0))) == GV_ERR_BAD_ARG
    lib = gvamd.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.gv_track_update(h._h, p(z), C.c_int32(129), C.c_double(0.1), None, C.c_uint32(0), None, None) == GV_ERR_BAD_ARG
    assert lib.gv_track_update(h._h, None, C.c_int32(1), C.c_double(0.1), None, C.c_uint32(0), None, None) == GV_ERR_BAD_ARG
    assert lib.gv_track_update(h._h, p(z), C.c_int32(2), C.c_double(0.1), None, C.c_uint32(4), None, None) == GV_ERR_BAD_ARG
    assert lib.gv_track_update(None, p(z), C.c_int32(2), C.c_double(0.1), None, C.c_uint32(0), None, None) == GV_ERR_BAD_ARG
    for slots in ([1, 1], [2, 1], [-1, 0], [0, 128]):
        assert _code(gvamd, lambda: h.set_tracks(tc.tracks_at([(0.0, 0.0), (1.0, 1.0)], slots=slots), 5)) == GV_ERR_BAD_ARG
    assert lib.gv_set_tracks(h._h, None, C.c_int32(1), C.c_uint32(1)) == GV_ERR_BAD_ARG
    assert lib.gv_set_tracks(h._h, p(np.zeros(129, ref.TRACK_DTYPE)), C.c_int32(129), C.c_uint32(1)) == GV_ERR_BAD_ARG
    got, nid = h.get_tracks()
    assert got.tobytes() == tracks.tobytes() and nid == 3                                  # every refused call left the state alone
    n, out = C.c_int32(-1), np.full(128, 7, np.uint8)
    assert lib.gv_get_tracks(h._h, p(out), C.c_int32(1), C.byref(n), None) == GV_ERR_BAD_ARG and n.value == 2 and (out == 7).all()
    assert lib.gv_get_tracks(h._h, None, C.c_int32(0), C.byref(n), None) == GV_ERR_BAD_ARG and n.value == 2
    h.reset()                                                                              # kept through gv_reset
    assert h.get_tracks()[0].tobytes() == tracks.tobytes()
    h.set_tracks(None, 77)                                                                 # n == 0 empties the state
    assert h.get_tracks() [1] == 77 and len(h.get_tracks()[0]) == 0
    h.track_update(z, 0.1)
    h.set_track_config(None)                                                               # off: the state after gv_create
    got, nid = h.get_tracks()
    assert len(got) == 0 and nid == 1
    h.set_track_config(ref.to_struct(gvamd, good))
    info, tracks = h.track_update(z, 0.1)
    assert int(info["n_born"]) == 2 and tracks["id"].tolist() == [1, 2] and int(info["next_id"]) == 3


# ---------------------------------------------------------------------------------------------------------- feed --
DYN_CFG = dyn_ref.config(off_x=(0.0,), radius=0.5, influence_radius=2.5, cost_scaling_factor=1.0, quantum=0.125, t0=0.1, dt=0.1)


def _poses(seed, K=9, P=33, span=40.0):
    rng = np.random.default_rng(seed)
    p = np.zeros((K, P, 3), np.float32)
    p[:, :, 0] = rng.uniform(-5.0, span, (K, 1)) + np.cumsum(rng.uniform(-0.3, 0.6, (K, P)), axis=1)
    p[:, :, 1] = rng.uniform(-6.0, 6.0, (K, 1)) + np.cumsum(rng.uniform(-0.3, 0.3, (K, P)), axis=1)
    return p


@pytest.mark.parametrize("name,n_steps,n_exp", [("chain_128", 1, 128), ("filter", 12, 3), ("non_finite_states", 2, 5), ("min_speed_edge", 2, 3),
                                                ("confirm_then_delete", 2, 0)])
def test_fed_set_scores_like_the_twins_objects(gvamd, name, n_steps, n_exp):
    c = tc.by_name(name)
    h = _handle(gvamd)
    h.set_dyn_config(dyn_ref.to_struct(gvamd, DYN_CFG))
    h.set_moving_objects(dc.objects(CONTROL_OBJS))           # replaced by the feed
    _load(h, gvamd, c)
    objs = _twin(gvamd, c, n_steps)[-1][3]
    assert len(objs) == n_exp
    for s in c["steps"][:n_steps]:
        h.track_update_async(np.ascontiguousarray(s["dets"]), s["dt"], s["motion"], feed=True)
    poses = _poses(3, span=380.0 if name == "chain_128" else 40.0)
    got, got_pc = h.score_dynamic(poses, keep_pose_cost=True)
    want, want_pc = gvamd.dyn_score_poses(dyn_ref.to_struct(gvamd, DYN_CFG), objs, poses, keep_pose_cost=True)
    assert got.tobytes() == want.tobytes() and got_pc.tobytes() == want_pc.tobytes(), name
    if n_exp == 0:
        assert got.tobytes() == np.array([EMPTY_RECORD] * len(poses), dyn_ref.SCORE_DTYPE).tobytes()      # a fed empty set
    else:
        assert (got["nearest_object"] >= 0).all() and (got["max_cost"] > 0).any()
    h.set_moving_objects(objs)                                # the same set from the host: the same rows
    assert h.score_dynamic(poses).tobytes() == want.tobytes()


def test_fed_and_host_sets_are_stream_ordered(gvamd):
    """score, fed update, score, gv_set_moving_objects, score, fed update of no tracks, score -- enqueued without a wait:
    each score has its own set"""
    h = _handle(gvamd)
    c = tc.by_name("filter")
    cfg = dyn_ref.to_struct(gvamd, DYN_CFG)
    h.set_dyn_config(cfg)
    poses = _poses(5)
    K, P = poses.shape[:2]
    set_a, set_c = dc.objects(CONTROL_OBJS), dc.objects(CONTROL_OBJS[:1])
    twin = _twin(gvamd, c, 12)
    want = [gvamd.dyn_score_poses(cfg, o, poses) for o in (set_a, twin[10][3], set_c, twin[11][3])]
    want.append(np.array([EMPTY_RECORD] * K, dyn_ref.SCORE_DTYPE))
    assert len({w.tobytes() for w in want}) == 5
    pins = [gvamd.PinnedI8(K * 24) for _ in want]
    try:
        _load(h, gvamd, c)
        for s in c["steps"][:10]:
            h.track_update_async(np.ascontiguousarray(s["dets"]), s["dt"], s["motion"])
        for q in pins:
            q.array[:] = 77
        out = [q.array.view(dyn_ref.SCORE_DTYPE) for q in pins]
        s10, s11 = c["steps"][10], c["steps"][11]
        h.set_moving_objects(set_a)
        h.score_dynamic_async(poses, K, P, out[0])
        h.track_update_async(np.ascontiguousarray(s10["dets"]), s10["dt"], s10["motion"], feed=True)
        h.score_dynamic_async(poses, K, P, out[1])
        h.set_moving_objects(set_c)
        h.score_dynamic_async(poses, K, P, out[2])
        h.track_update_async(np.ascontiguousarray(s11["dets"]), s11["dt"], s11["motion"], feed=True)
        h.score_dynamic_async(poses, K, P, out[3])
        h.set_tracks(None, 1)
        h.track_update_async(None, 0.1, feed=True)
        h.score_dynamic_async(poses, K, P, out[4])
        h.synchronize()
        for k, (o, w) in enumerate(zip(out, want)):
            assert o.tobytes() == w.tobytes(), k
    finally:
        for q in pins:
            q.close()


def test_control_step_after_a_fed_update(gvamd):
    """the control step with a fed set equals gv_control_select_dyn over the device's X7 and X9 records and the reference's
    X13 records of the twin's exported objects"""
    h = _handle(gvamd)
    h.reset()
    _scene(h, np.zeros((h.ny, h.nx), bool))
    poses = h.rollout_array()
    ptr, K, P = h.device_rollout()
    start = dc.objects(CONTROL_OBJS)
    tracks = tc.tracks_at(np.stack([start["pose"]["px"], start["pose"]["py"]], 1), v=np.stack([start["vx"], start["vy"]], 1), hits=3)
    for n in ("qz", "qw", "length", "width"):
        tracks[n] = start["pose"][n]
    c = tc.case("control", ref.config(max_misses=5), [tc.step(None, 0.0)], tracks, 4)
    objs = _twin(gvamd, c)[0][3]
    assert objs.tobytes() != start.tobytes() and len(objs) == 3          # pz and height differ: neither is read
    traj, nav = h.score_trajectories(poses, device_ptr=ptr), h.score_nav(poses, device_ptr=ptr)
    for w_sum, w_max in ((50, 0), (1, 3)):
        cfg = _control_cfg(w_sum, w_max)
        h.set_dyn_config(dyn_ref.to_struct(gvamd, cfg))
        h.set_moving_objects(None)
        _load(h, gvamd, c)
        h.track_update_async(None, 0.0, feed=True)
        want_d = dyn_ref.score(cfg, objs, poses)["scores"]
        assert h.score_dynamic(poses, device_ptr=ptr).tobytes() == want_d.tobytes()
        assert (want_d["first_collision"] >= 0).any() and (want_d["first_collision"] < 0).any()
        for w in (W(1, 1), W(3, 7, 11, 13, 17)):
            nv = nav if rollout_ref.nav_used(w) else None
            want_r, want_t = gvamd.control_select_dyn(_cw(gvamd, w), traj, nv, want_d, dyn_ref.to_struct(gvamd, cfg), keep_totals=True)
            assert _step(h, gvamd, w) == (np.array([want_r]).tobytes(), want_t.tobytes()), (w_sum, w_max, w)


def test_track_demo(gvamd, tmp_path):
    """examples/track_demo.cpp (plain g++ over the C ABI): three boxes tracked for 20 ticks, the crossing car's track
    rejects the fastest trajectory, the host twin replays tracks and records"""
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "grid-vision_amd")
    exe = str(tmp_path / "track_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(pkg, "examples", "track_demo.cpp"), "-o", exe,
                           "-L" + pkg, "-lgridvision_hip", "-Wl,-rpath," + pkg])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert re.search(r"tick  0: 3 tracks, 0 confirmed, 0 exported, 0 matched, 3 born", out.stdout), out.stdout
    assert re.search(r"tick 19: 3 tracks, 3 confirmed, 3 exported, 3 matched, 0 born", out.stdout), out.stdout
    assert re.search(r"track id 1 slot 0 hits 20 at \(9\.00, -6\.00\) velocity \(0\.00, 3\.00\)", out.stdout), out.stdout
    assert re.search(r"track id 2 slot 1 hits 20 at \(20\.50, 3\.00\) velocity \(-5\.00, 0\.00\)", out.stdout), out.stdout
    assert "parked car exported with velocity (0.00, 0.00)" in out.stdout
    assert re.search(r"trajectory 0 \(3\.0 m/s\): max cost 254 first collision \d+ nearest 0 .* REJECTED", out.stdout), out.stdout
    m = re.search(r"with the tracked cars: best (\d) ", out.stdout)
    assert m and int(m.group(1)) > 0, out.stdout
    assert "tracks equal the host's, records against the fed set equal the host's" in out.stdout and "track check ok" in out.stdout
