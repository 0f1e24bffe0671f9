"""[EXTENSION] X16 scan-to-costmap matching on the device: gv_match_scan / gv_match_scan_async through the binding
against match_ref with zero tolerance, record and score volume, on every family of match_cases.  The map is planted with
set_log_odds + update_map and inflated on the device as test_gpu_inflate.py does; its costmap() read-back must equal
the fixture's (inflate_ref), and the reference is the one computed from that.  Every call is made three times with the
same bytes, into pageable and into pinned destinations.  Then the ordering rules (a second inflate and a configuration
change behind an enqueued match, a pending tick, gv_grid_move, the 0..100 scale), the state rules of the header, and
the example."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import match_cases as mc
import match_ref as ref
from planner_util import first_diff, plant_grid

pytestmark = pytest.mark.gpu

GV_ERR_BAD_ARG, GV_ERR_STATE, GV_ERR_TF = 1, 5, 6
HERE = os.path.dirname(os.path.abspath(__file__))
_HANDLES = {}


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    yield m
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()


def _handle(gvamd, grid):
    if grid not in _HANDLES:
        h = gvamd.GridVisionHIP(*mc.GRIDS[grid])
        geo = mc.geo_of(grid)
        assert (h.nx, h.ny, h.pos_x, h.pos_y) == (geo.nx, geo.ny, geo.pos_x, geo.pos_y)
        _HANDLES[grid] = h
    h = _HANDLES[grid]
    h.reset()
    return h


def lib_cfg(gvamd, c):
    return gvamd.MatchConfig(c.wx, c.wy, c.wt, c.stride, c.yaw_step, c.min_points, c.flags)


def _inflate(h, inflation):
    ins, infl, scaling, thr, occ = inflation
    h.set_inflation(ins, infl, scaling, thr, occupancy_scale=occ)
    h.inflate()


def _plant(h, mask, inflation):
    """the mask planted and inflated on the device; its read-back is the fixture's costmap"""
    plant_grid(h, mask)
    _inflate(h, inflation)
    cost = h.costmap()
    want = mc.cost_of(mask, inflation, mc.geo_of("small" if h.nx == 50 else "big").res)
    assert cost.tobytes() == want.tobytes(), first_diff(cost, want)
    return cost


def _load(h, gvamd, c):
    h.set_transforms(base_lidar=c["tf"])
    if c["band"] is None:
        h.set_height_band(None)
    else:
        h.set_height_band(c["band"][0], c["band"][1], True)
    h.upload_xyz(c["x"], c["y"], c["z"])
    h.set_match_config(lib_cfg(gvamd, c["cfg"]))


class _Pinned:
    """a pinned record and a pinned volume"""

    def __init__(self, gvamd, n_scores):
        self.r, self.v = gvamd.PinnedI8(64), gvamd.PinnedI8(4 * n_scores)
        self.rec, self.vol = self.r.array.view(gvamd.MATCH_RESULT_DTYPE), self.v.array.view(np.uint32)

    def close(self):
        self.rec = self.vol = None
        self.r.close(); self.v.close()


def _check(h, gvamd, c, want, tag=""):
    """three times each: the waited call, the enqueued call into pageable memory, the enqueued call into pinned memory"""
    want_r, want_v = want
    name = c["name"]
    pin = _Pinned(gvamd, want_v.size)
    try:
        for rep in range(3):
            got_r, got_v = h.match_scan(c["guess"], keep_scores=True)
            assert got_v.tobytes() == want_v.tobytes(), (name, tag, rep, "volume", first_diff(got_v, want_v))
            assert np.asarray(got_r).tobytes() == want_r.tobytes(), (name, tag, rep, got_r, want_r)
            assert np.asarray(h.match_scan(c["guess"])).tobytes() == want_r.tobytes(), (name, tag, rep, "without the volume")
            rec, vol = np.full(16, 7, np.int32).view(gvamd.MATCH_RESULT_DTYPE), np.full(want_v.size, 7, np.uint32)
            pin.rec.view(np.int32)[:] = 7
            pin.vol[:] = 7
            h.match_scan_async(c["guess"], rec, vol)
            h.match_scan_async(c["guess"], pin.rec, pin.vol)
            h.synchronize()
            assert vol.tobytes() == want_v.tobytes() == pin.vol.tobytes(), (name, tag, rep, "async", first_diff(vol, want_v),
                                                                            first_diff(pin.vol, want_v))
            assert rec.tobytes() == want_r.tobytes() == pin.rec.tobytes(), (name, tag, rep, "async", rec, pin.rec, want_r)
            pin.rec.view(np.int32)[:] = 7
            h.match_scan_async(c["guess"], pin.rec)            # a pinned record alone: the volume stays on the device
            h.synchronize()
            assert pin.rec.tobytes() == want_r.tobytes(), (name, tag, rep, "pinned record alone")
    finally:
        pin.close()


@pytest.mark.parametrize("name", mc.names())
def test_families(gvamd, name):
    c = mc.by_name(name)
    h = _handle(gvamd, c["grid"])
    _plant(h, c["mask"], c["inflation"])
    _load(h, gvamd, c)
    _check(h, gvamd, c, mc.want(c))


def test_occupancy_scale(gvamd):
    """the costmap on the 0..100 scale: the sums are those of the bytes as they lie"""
    c = dict(mc.by_name("d_rect"), inflation=mc.SOFT_100)
    h = _handle(gvamd, c["grid"])
    cost = _plant(h, c["mask"], c["inflation"])
    assert cost.max() == 100
    want = mc.want(c, cost)
    assert int(want[0]["best_score"][0]) == int(want[0]["n_used"][0]) * 100
    _load(h, gvamd, c)
    _check(h, gvamd, c, want)


def test_second_inflate_and_config_change_in_flight(gvamd):
    """match, set_match_config, match, set_inflation, inflate, match -- enqueued back to back, one synchronize: every call
    keeps the configuration it was enqueued with and reads the costmap of the inflate before it"""
    c = mc.by_name("d_rect")
    h = _handle(gvamd, c["grid"])
    cost2 = _plant(h, c["mask"], mc.EXACT)
    cost1 = _plant(h, c["mask"], mc.SOFT)
    assert cost1.tobytes() != cost2.tobytes()
    _load(h, gvamd, c)
    cfg_a, cfg_b = c["cfg"], ref.Cfg(2, 6, 2, 0.01, stride=2)
    pins = [_Pinned(gvamd, 11 * 5 * 3), _Pinned(gvamd, 5 * 13 * 5), _Pinned(gvamd, 5 * 13 * 5)]
    try:
        h.match_scan_async(c["guess"], pins[0].rec, pins[0].vol)
        h.set_match_config(lib_cfg(gvamd, cfg_b))
        h.match_scan_async(c["guess"], pins[1].rec, pins[1].vol)
        _inflate(h, mc.EXACT)
        h.match_scan_async(c["guess"], pins[2].rec, pins[2].vol)
        h.synchronize()
        want = [mc.want(dict(c, cfg=cfg), cost) for cfg, cost in ((cfg_a, cost1), (cfg_b, cost1), (cfg_b, cost2))]
        assert want[1][1].tobytes() != want[2][1].tobytes()
        for i in range(3):
            assert pins[i].vol.tobytes() == want[i][1].tobytes(), (i, first_diff(pins[i].vol, want[i][1]))
            assert pins[i].rec.tobytes() == want[i][0].tobytes(), (i, pins[i].rec, want[i][0])
    finally:
        for p in pins:
            p.close()


def test_uploads_behind_enqueued_matches(gvamd):
    """The host runs ahead of the public stream: eight heavy matches (65^3 candidates over 20 000 points) keep the stream
    busy, then four light matches, each behind an upload of its own cloud, nothing waited for in between.  The three
    cloud sets rotate, so the third upload goes into the heavy cloud's set and the fourth into the first light cloud's
    while their matches are still enqueued: every upload into a set must wait for the matches that read it.  Each light
    match equals the reference of its own cloud; the last heavy match equals the first."""
    c = mc.by_name("d_rect")
    h = _handle(gvamd, c["grid"])
    cost = _plant(h, c["mask"], mc.SOFT)
    h.set_transforms(base_lidar=c["tf"])
    h.set_height_band(None)
    heavy_cfg, light_cfg = ref.Cfg(32, 32, 32, 0.01), c["cfg"]
    hx, hy, hz = mc._scatter(20000, 55)
    for _ in range(3):                       # every cloud set holds 20 000 points: no upload below grows one
        h.upload_xyz(hx, hy, hz)
    poses = [(0.7 - 0.1 * k, -0.4 + 0.1 * (k % 2), 0.1 + 0.02 * (k - 1)) for k in range(4)]
    lights = [dict(c, x=x, y=y, z=z) for x, y, z in (mc._wall_cloud("big", p, c["tf"]) for p in poses)]
    want = [mc.want(lc, cost) for lc in lights]
    assert len({w[0].tobytes() for w in want}) == 4 and len({w[1].tobytes() for w in want}) == 4
    heavy = [_Pinned(gvamd, 1) for _ in range(3)]
    pins = [_Pinned(gvamd, want[0][1].size) for _ in range(4)]
    try:
        h.set_match_config(lib_cfg(gvamd, heavy_cfg))
        h.match_scan_async(c["guess"], heavy[0].rec)
        h.synchronize()
        assert int(heavy[0].rec["n_used"][0]) == 20000 and int(heavy[0].rec["best_score"][0]) > 0
        for i in range(8):
            h.match_scan_async(c["guess"], heavy[1 if i < 7 else 2].rec)
        h.set_match_config(lib_cfg(gvamd, light_cfg))
        for lc, p in zip(lights, pins):
            h.upload_xyz(lc["x"], lc["y"], lc["z"])
            h.match_scan_async(c["guess"], p.rec, p.vol)
        h.upload_xyz(hx, hy, hz)             # and one more round of the rotation behind the light matches
        h.synchronize()
        assert heavy[2].rec.tobytes() == heavy[0].rec.tobytes() == heavy[1].rec.tobytes()
        for i in range(4):
            assert pins[i].vol.tobytes() == want[i][1].tobytes(), (i, first_diff(pins[i].vol, want[i][1]))
            assert pins[i].rec.tobytes() == want[i][0].tobytes(), (i, pins[i].rec, want[i][0])
    finally:
        for p in heavy + pins:
            p.close()


def test_uploads_behind_both_matchers(gvamd):
    """The two matchers share one reader event and one mask over the cloud sets.  Two heavy scans (65^3 candidates over
    20 000 points) and two heavy searches keep the public stream busy, then four light calls -- scan, search, scan, search
    -- each behind an upload of its own small cloud into a pinned record of its own, then the heavy cloud once more, and
    one synchronize at the end: every upload into a set waits for the last point pass of either matcher that read it.
    Every record (and every search's stats) equals the host twin's bytes for the cloud its call was enqueued behind.
    The issue's 129 x 129 x 9 heavy search is narrowed to 129 x 129 x 3: its twin took 6.0 s on one core beside the heavy
    scan's 3.6 s, at three yaw candidates 1.8 s."""
    c = mc.by_name("d_rect")
    h = _handle(gvamd, c["grid"])
    cost = _plant(h, c["mask"], mc.SOFT)
    h.set_transforms(base_lidar=c["tf"])
    h.set_height_band(None)
    grid, guess = mc.GRIDS[c["grid"]], c["guess"]
    heavy_scan, heavy_search = gvamd.MatchConfig(32, 32, 32, 1, 0.01, 1, 0), gvamd.SearchConfig(64, 64, 1, 1, 0.01, 1, 0, 2, 0)
    light_scan, light_search = lib_cfg(gvamd, c["cfg"]), gvamd.SearchConfig(9, 6, 1, 1, 0.02, 1, 0, 2, 0)
    hx, hy, hz = mc._scatter(20000, 55)
    for _ in range(3):                       # every cloud set holds 20 000 points: no upload below grows one
        h.upload_xyz(hx, hy, hz)
    lights = [mc._scatter(n, 60 + n) for n in (300, 367, 433, 500)]

    def twin(cfg, x, y, z):
        if isinstance(cfg, gvamd.SearchConfig):
            rec, stats = gvamd.match_search_host(*grid, cost, x, y, z, c["tf"], cfg, guess)
            return np.asarray(rec).tobytes(), np.asarray(stats).tobytes()
        return np.asarray(gvamd.match_scan_host(*grid, cost, x, y, z, c["tf"], cfg, guess)).tobytes(), None

    def enqueue(cfg, p):
        if isinstance(cfg, gvamd.SearchConfig):
            h.set_search_config(cfg)
            h.match_search_async(guess, p.rec, p.stats)
        else:
            h.set_match_config(cfg)
            h.match_scan_async(guess, p.rec)

    class Pin(_Pinned):
        def __init__(self):
            super().__init__(gvamd, 1)
            self.s = gvamd.PinnedI8(32)
            self.stats = self.s.array.view(gvamd.SEARCH_STATS_DTYPE)

        def close(self):
            self.stats = None
            self.s.close()
            super().close()

    calls = [(heavy_scan, (hx, hy, hz)), (heavy_scan, (hx, hy, hz)), (heavy_search, (hx, hy, hz)), (heavy_search, (hx, hy, hz))]
    calls += [(cfg, pts) for cfg, pts in zip((light_scan, light_search, light_scan, light_search), lights)]
    pins = [Pin() for _ in calls]
    try:
        for p in pins:
            p.rec.view(np.int32)[:] = 7
            p.stats.view(np.int32)[:] = 7
        for k, ((cfg, pts), p) in enumerate(zip(calls, pins)):
            if k >= 4:
                h.upload_xyz(*pts)
            enqueue(cfg, p)
        h.upload_xyz(hx, hy, hz)             # and one more round of the rotation behind the light calls
        h.synchronize()
        want = {}
        for k, ((cfg, pts), p) in enumerate(zip(calls, pins)):
            key = (bytes(cfg), pts[0].tobytes())
            if key not in want:
                want[key] = twin(cfg, *pts)
            rec, stats = want[key]
            assert p.rec.tobytes() == rec, (k, p.rec)
            assert stats is None or p.stats.tobytes() == stats, (k, p.stats)
        assert len({p.rec.tobytes() for p in pins}) == 6                 # two heavy kinds, four light clouds
        assert all(int(p.rec["n_used"][0]) == len(pts[0]) and int(p.rec["best_score"][0]) > 0 for (_, pts), p in zip(calls, pins))
    finally:
        for p in pins:
            p.close()


def test_match_during_a_pending_tick(gvamd):
    """tick_enqueue, inflate, match, tick_wait: the match reads the tick's grid, not the grid before it"""
    from gvamd import synth
    from test_gpu_parity import _ground_scene, make_handle
    hA, tfs = make_handle(gvamd, 2, perturbed=True)
    hB, _ = make_handle(gvamd, 2, perturbed=True)
    g = synth.CONFIGS[2]["grid"]
    geo = ref.geometry(g.grid_x, g.grid_y, g.resolution)
    assert (geo.nx, geo.ny, geo.pos_x) == (hA.nx, hA.ny, hA.pos_x)
    x, y, z, _, b = _ground_scene(tfs, seed=9)
    cfg = ref.Cfg(3, 4, 2, 0.01, stride=16)
    guess = (0.25, -0.15, 0.01)
    pin = _Pinned(gvamd, 5 * 9 * 7)
    try:
        for h in (hA, hB):
            h.upload_xyz(x, y, z)
            h.set_inflation(0.35, 0.55, 10.0, 65)
            h.set_match_config(lib_cfg(gvamd, cfg))
        hB.inflate()
        before = hB.costmap()            # of the empty grid: the tick's lidar update is what puts the scan on the map
        assert not before.any()
        hA.tick_enqueue(b, k_near=4, lidar_bin=True)
        hA.inflate()
        hA.match_scan_async(guess, pin.rec, pin.vol)
        hA.tick_wait()
        hA.synchronize()
        hB.tick(b, k_near=4, lidar_bin=True)
        hB.inflate()
        cost = hB.costmap()
        m = mc.m_base(tfs["base_lidar"])
        want, stale = ref.scan(geo, cost, m, x, y, z, cfg, guess), ref.scan(geo, before, m, x, y, z, cfg, guess)
        assert want[1].tobytes() != stale[1].tobytes() and int(want[0]["best_score"][0]) > 0
        assert pin.vol.tobytes() == want[1].tobytes(), first_diff(pin.vol, want[1])
        assert pin.rec.tobytes() == want[0].tobytes()
    finally:
        pin.close()
        hA.close(); hB.close()


def test_match_feeds_grid_move(gvamd):
    """the loop the call closes: match, gv_match_motion, gv_grid_move, inflate, match again from a zero guess"""
    c = mc.by_name("a_big_+3-2+2")
    h = _handle(gvamd, c["grid"])
    _plant(h, c["mask"], mc.SOFT)
    _load(h, gvamd, c)
    rec = h.match_scan(c["guess"])
    assert (int(rec["best_t"]), int(rec["best_j"]), int(rec["best_i"])) == c["best"]
    m = gvamd.match_motion(rec)
    info = h.grid_move([m.qx, m.qy, m.qz, m.qw, m.tx, m.ty, m.tz])
    assert info["applied"]
    h.inflate()
    cost = h.costmap()
    zero = dict(c, guess=(0.0, 0.0, 0.0))
    want = mc.want(zero, cost)
    _check(h, gvamd, zero, want, tag="after gv_grid_move")
    # the map now sits at the scan's frame up to the move's sub-cell residue: the best shift is within one cell and step
    assert max(abs(int(want[0]["best_t"][0])), abs(int(want[0]["best_j"][0])), abs(int(want[0]["best_i"][0]))) <= 1
    assert int(want[0]["best_score"][0]) > int(0.8 * 254 * c["n_used"])


def test_state_rules(gvamd):
    lib = gvamd.load()
    c = mc.by_name("b_mirror_i")
    h = gvamd.GridVisionHIP(*mc.GRIDS[c["grid"]])
    good = lib_cfg(gvamd, c["cfg"])

    def code(call):
        with pytest.raises(gvamd.GVError) as e:
            call()
        return e.value.code

    def raw(guess=c["guess"], flags=0, result=True, scores=None, handle=True, fn=None):
        q = gvamd.MatchGuess(*guess) if guess is not None else None
        res = np.full(16, 7, np.int32)
        rc = (fn or lib.gv_match_scan)(h._h if handle else None, C.byref(q) if q is not None else None, C.c_uint32(flags),
                                       res.ctypes.data_as(C.c_void_p) if result else None, scores)
        return rc, res

    try:
        scan = lambda: h.match_scan(c["guess"])                      # noqa: E731
        for fn in (lib.gv_match_scan, lib.gv_match_scan_async):
            assert raw(handle=False, fn=fn)[0] == GV_ERR_BAD_ARG
        assert lib.gv_set_match_config(None, C.byref(good)) == GV_ERR_BAD_ARG
        assert code(scan) == GV_ERR_TF                               # no base_from_lidar
        h.set_transforms(base_lidar=c["tf"])
        assert code(scan) == GV_ERR_STATE                            # no configuration
        h.set_match_config(good)
        assert code(scan) == GV_ERR_STATE                            # no cloud
        h.upload_xyz(c["x"], c["y"], c["z"])
        assert code(scan) == GV_ERR_STATE                            # no gv_inflate yet
        h.set_match_config(None)
        cost = _plant(h, c["mask"], c["inflation"])
        assert code(scan) == GV_ERR_STATE                            # a costmap, no configuration
        h.set_match_config(good)
        want = mc.want(c)[0]
        assert np.asarray(scan()).tobytes() == want.tobytes()
        # a rejected configuration leaves the one in force alone
        for kw in (dict(wx=33), dict(wy=-1), dict(wt=33), dict(yaw_step=float("nan")), dict(wt=1, yaw_step=0.0), dict(stride=0),
                   dict(stride=1025), dict(min_points=0), dict(flags=2)):
            base = dict(wx=2, wy=2, wt=0, yaw_step=0.0, stride=1, min_points=1, flags=0)
            base.update(kw)
            assert code(lambda: h.set_match_config(gvamd.MatchConfig.of(**base))) == GV_ERR_BAD_ARG, kw
        assert np.asarray(scan()).tobytes() == want.tobytes()
        # arguments: state unchanged, nothing written
        for kw in (dict(guess=None), dict(result=False), dict(flags=2), dict(flags=1), dict(guess=(float("nan"), 0.0, 0.0)),
                   dict(guess=(0.0, float("inf"), 0.0)), dict(guess=(0.0, 0.0, float("-inf")))):
            rc, res = raw(**kw)
            assert rc == GV_ERR_BAD_ARG and (res == 7).all(), kw
        rc, res = raw()
        assert rc == 0 and res.tobytes() == want.tobytes()
        # the configuration is kept through gv_set_log_odds, gv_grid_move and gv_reset; gv_reset invalidates the costmap
        cost_b = _plant(h, np.zeros((h.ny, h.nx), bool), c["inflation"])
        assert np.asarray(scan()).tobytes() == mc.want(c, cost_b)[0].tobytes() != want.tobytes()
        assert h.grid_move([0.0, 0.0, 0.0, 1.0, 0.3, -0.2, 0.0])["applied"]
        assert np.asarray(scan()).tobytes() == mc.want(c, cost_b)[0].tobytes()     # the costmap is a snapshot
        h.reset()
        assert code(scan) == GV_ERR_STATE
        _plant(h, c["mask"], c["inflation"])
        assert np.asarray(scan()).tobytes() == want.tobytes()
        assert cost.tobytes() == h.costmap().tobytes()
    finally:
        h.close()


def test_match_demo(gvamd, tmp_path):
    """examples/match_demo.cpp (plain g++ over the two headers): a wall scene seen from a displaced pose, matched, the
    motion fed to gv_grid_move, the recovered pose printed and checked against the host twin"""
    root = os.path.dirname(HERE)
    pkg = os.path.join(root, "grid-vision_amd")
    exe = str(tmp_path / "match_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(root, "include"), os.path.join(pkg, "examples", "match_demo.cpp"),
                           "-o", exe, "-L" + pkg, "-lgridvision_hip", "-Wl,-rpath," + pkg])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    m = re.search(r"recovered pose x (-?[\d.]+) y (-?[\d.]+) yaw (-?[\d.]+) \(true (-?[\d.]+) (-?[\d.]+) (-?[\d.]+)\)", out.stdout)
    assert m and "host twin ok" in out.stdout and "grid moved" in out.stdout, out.stdout
    x, y, yaw, tx, ty, tyaw = (float(v) for v in m.groups())
    assert abs(x - tx) <= 0.051 and abs(y - ty) <= 0.051 and abs(yaw - tyaw) <= 0.0101
