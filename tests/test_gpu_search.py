"""[EXTENSION] X18 wide-window scan matching by branch and bound on the device: gv_match_search / gv_match_search_async
through the binding against search_ref with zero tolerance, record and stats, on every case of search_cases.  The map is
planted and inflated on the device as test_gpu_match.py does; its costmap() read-back must equal the fixture's, and the
reference is the one computed from that.  Every call is made three times with the same bytes, into pageable and into
pinned destinations, with and without the stats.  Then every family of match_cases against gv_match_scan on the same
handle, the ordering rules (a configuration change and a second inflate behind enqueued searches, an upload into a
cloud set an enqueued search reads, a pending tick), the state rules of the header, and the example."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import match_cases as mc
import search_cases as sc
import search_ref as ref
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
    return gvamd.SearchConfig(c.wx, c.wy, c.wt, c.stride, c.yaw_step, c.min_points, c.flags, c.block_log2, 0)


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
    if isinstance(c["cfg"], ref.Cfg):
        h.set_search_config(lib_cfg(gvamd, c["cfg"]))


class _Pinned:
    """a pinned record and pinned stats"""

    def __init__(self, gvamd):
        self.r, self.s = gvamd.PinnedI8(64), gvamd.PinnedI8(32)
        self.rec, self.stats = self.r.array.view(gvamd.MATCH_RESULT_DTYPE), self.s.array.view(gvamd.SEARCH_STATS_DTYPE)

    def fill(self):
        self.r.array[:] = 7
        self.s.array[:] = 7

    def close(self):
        self.rec = self.stats = None
        self.r.close(); self.s.close()


def _check(h, gvamd, c, want_r, want_s, tag=""):
    """three times each: the waited call, the enqueued call into pageable memory, the enqueued call into pinned memory,
    and each without the stats"""
    name = c["name"]
    pin = _Pinned(gvamd)
    try:
        for rep in range(3):
            got_r, got_s = h.match_search(c["guess"])
            assert np.asarray(got_s).tobytes() == want_s.tobytes(), (name, tag, rep, got_s, want_s)
            assert np.asarray(got_r).tobytes() == want_r.tobytes(), (name, tag, rep, got_r, want_r)
            assert np.asarray(h.match_search(c["guess"], keep_stats=False)).tobytes() == want_r.tobytes(), (name, tag, rep, "stats = NULL")
            rec, stats = np.full(16, 7, np.int32).view(gvamd.MATCH_RESULT_DTYPE), np.full(8, 7, np.int32).view(gvamd.SEARCH_STATS_DTYPE)
            pin.fill()
            h.match_search_async(c["guess"], rec, stats)
            h.match_search_async(c["guess"], pin.rec, pin.stats)
            h.synchronize()
            assert stats.tobytes() == want_s.tobytes() == pin.stats.tobytes(), (name, tag, rep, "async", stats, pin.stats, want_s)
            assert rec.tobytes() == want_r.tobytes() == pin.rec.tobytes(), (name, tag, rep, "async", rec, pin.rec, want_r)
            rec2 = np.full(16, 7, np.int32).view(gvamd.MATCH_RESULT_DTYPE)
            pin.fill()
            h.match_search_async(c["guess"], rec2)
            h.match_search_async(c["guess"], pin.rec)             # a pinned record alone
            h.synchronize()
            assert rec2.tobytes() == want_r.tobytes() == pin.rec.tobytes(), (name, tag, rep, "async, stats = NULL")
            assert (pin.s.array == 7).all()
    finally:
        pin.close()


@pytest.mark.parametrize("name", sc.names())
def test_cases(gvamd, name):
    c = sc.by_name(name)
    h = _handle(gvamd, c["grid"])
    _plant(h, c["mask"], c["inflation"])
    _load(h, gvamd, c)
    a = sc.want(c)
    _check(h, gvamd, c, a.record, a.stats)


@pytest.mark.parametrize("name", mc.names())
def test_families_against_the_exhaustive_call(gvamd, name):
    """every family of match_cases: the search's record is the record gv_match_scan gives on the same handle, at every
    block size; and the stats are the host twin's"""
    c = mc.by_name(name)
    h = _handle(gvamd, c["grid"])
    cost = _plant(h, c["mask"], c["inflation"])
    _load(h, gvamd, c)
    m = c["cfg"]
    h.set_match_config(gvamd.MatchConfig(m.wx, m.wy, m.wt, m.stride, m.yaw_step, m.min_points, m.flags))
    want = np.asarray(h.match_scan(c["guess"]))
    assert want.tobytes() == mc.want(c)[0].tobytes()
    for lg in sc.SIZES:
        cfg = gvamd.SearchConfig(m.wx, m.wy, m.wt, m.stride, m.yaw_step, m.min_points, m.flags, lg, 0)
        h.set_search_config(cfg)
        rec, stats = h.match_search(c["guess"])
        assert np.asarray(rec).tobytes() == want.tobytes(), (name, lg, rec, want)
        twin = gvamd.match_search_host(*mc.GRIDS[c["grid"]], cost, c["x"], c["y"], c["z"], c["tf"], cfg, c["guess"], band=c["band"])
        assert np.asarray(stats).tobytes() == np.asarray(twin[1]).tobytes(), (name, lg, stats, twin[1])
    assert np.asarray(h.match_scan(c["guess"])).tobytes() == want.tobytes()      # the two configurations are independent


def test_config_change_and_second_inflate_in_flight(gvamd):
    """search, set_search_config, search, set_inflation, inflate, search -- enqueued back to back, one synchronize: every
    call keeps the configuration it was enqueued with and reads (and pools) the costmap of the inflate before it"""
    c = sc.by_name("w_s8_remS1")
    h = _handle(gvamd, c["grid"])
    cost2 = _plant(h, c["mask"], mc.EXACT)
    cost1 = _plant(h, c["mask"], mc.SOFT)
    assert cost1.tobytes() != cost2.tobytes()
    _load(h, gvamd, c)
    cfg_a, cfg_b = c["cfg"], ref.Cfg(40, 23, 1, 0.01, stride=2, block_log2=2)
    pins = [_Pinned(gvamd) for _ in range(3)]
    try:
        for p in pins:
            p.fill()
        h.match_search_async(c["guess"], pins[0].rec, pins[0].stats)
        h.set_search_config(lib_cfg(gvamd, cfg_b))
        h.match_search_async(c["guess"], pins[1].rec, pins[1].stats)
        _inflate(h, mc.EXACT)
        h.match_search_async(c["guess"], pins[2].rec, pins[2].stats)
        h.synchronize()
        want = [sc.want(dict(c, cfg=cfg), cost) for cfg, cost in ((cfg_a, cost1), (cfg_b, cost1), (cfg_b, cost2))]
        assert len({w.stats.tobytes() for w in want}) == 3
        for i in range(3):
            assert pins[i].stats.tobytes() == want[i].stats.tobytes(), (i, pins[i].stats, want[i].stats)
            assert pins[i].rec.tobytes() == want[i].record.tobytes(), (i, pins[i].rec, want[i].record)
    finally:
        for p in pins:
            p.close()


def test_uploads_behind_enqueued_searches(gvamd):
    """The host runs ahead of the public stream: six heavy searches (257 x 257 x 33 candidates in blocks of 2 x 2 over 20 000 points) keep
    the stream busy, then four light searches, each behind an upload of its own cloud, nothing waited for in between.
    The three cloud sets rotate, so the third upload goes into the heavy cloud's set and the fourth into the first light
    cloud's while their searches are still enqueued: an upload into a set waits for the searches that read it."""
    c = sc.by_name("w_s4_rem1")
    h = _handle(gvamd, c["grid"])
    cost = _plant(h, c["mask"], mc.SOFT)
    h.set_transforms(base_lidar=c["tf"])
    h.set_height_band(None)
    heavy_cfg, light_cfg = ref.Cfg(128, 128, 16, 0.01, block_log2=1), c["cfg"]
    hx, hy, hz = mc._scatter(20000, 55)
    for _ in range(3):                       # every cloud set holds 20 000 points: no upload below grows one
        h.upload_xyz(hx, hy, hz)
    poses = [(0.7 - 0.1 * k, -0.4 + 0.1 * (k % 2), 0.1 + 0.02 * (k - 1)) for k in range(4)]
    lights = [dict(c, x=x, y=y, z=z) for x, y, z in (mc._wall_cloud("big", p, c["tf"]) for p in poses)]
    want = [sc.want(lc, cost) for lc in lights]
    assert len({w.record.tobytes() for w in want}) == 4
    heavy = [_Pinned(gvamd) for _ in range(3)]
    pins = [_Pinned(gvamd) for _ in range(4)]
    try:
        h.set_search_config(lib_cfg(gvamd, heavy_cfg))
        h.match_search_async(c["guess"], heavy[0].rec, heavy[0].stats)
        h.synchronize()
        assert int(heavy[0].rec["n_used"][0]) == 20000 and int(heavy[0].rec["best_score"][0]) > 0
        for i in range(6):
            k = 1 if i < 5 else 2
            h.match_search_async(c["guess"], heavy[k].rec, heavy[k].stats)
        h.set_search_config(lib_cfg(gvamd, light_cfg))
        for lc, p in zip(lights, pins):
            h.upload_xyz(lc["x"], lc["y"], lc["z"])
            h.match_search_async(c["guess"], p.rec, p.stats)
        h.upload_xyz(hx, hy, hz)             # and one more round of the rotation behind the light searches
        h.synchronize()
        assert heavy[2].rec.tobytes() == heavy[0].rec.tobytes() == heavy[1].rec.tobytes()
        assert heavy[2].stats.tobytes() == heavy[0].stats.tobytes() == heavy[1].stats.tobytes()
        for i in range(4):
            assert pins[i].stats.tobytes() == want[i].stats.tobytes(), (i, pins[i].stats, want[i].stats)
            assert pins[i].rec.tobytes() == want[i].record.tobytes(), (i, pins[i].rec, want[i].record)
    finally:
        for p in heavy + pins:
            p.close()


def test_search_during_a_pending_tick(gvamd):
    """tick_enqueue, inflate, search, tick_wait: the search reads the tick's grid, not the grid before it"""
    from gvamd import synth
    from test_gpu_parity import _ground_scene, make_handle
    import match_ref as mref
    hA, tfs = make_handle(gvamd, 2, perturbed=True)
    hB, _ = make_handle(gvamd, 2, perturbed=True)
    g = synth.CONFIGS[2]["grid"]
    geo = mref.geometry(g.grid_x, g.grid_y, g.resolution)
    assert (geo.nx, geo.ny, geo.pos_x) == (hA.nx, hA.ny, hA.pos_x)
    x, y, z, _, b = _ground_scene(tfs, seed=9)
    cfg = ref.Cfg(21, 12, 1, 0.01, stride=64, block_log2=3)
    guess = (0.25, -0.15, 0.01)
    pin = _Pinned(gvamd)
    try:
        for h in (hA, hB):
            h.upload_xyz(x, y, z)
            h.set_inflation(0.35, 0.55, 10.0, 65)
            h.set_search_config(lib_cfg(gvamd, cfg))
        hB.inflate()
        before = hB.costmap()            # of the empty grid: the tick's lidar update is what puts the scan on the map
        assert not before.any()
        hA.tick_enqueue(b, k_near=4, lidar_bin=True)
        hA.inflate()
        hA.match_search_async(guess, pin.rec, pin.stats)
        hA.tick_wait()
        hA.synchronize()
        hB.tick(b, k_near=4, lidar_bin=True)
        hB.inflate()
        cost = hB.costmap()
        m = mc.m_base(tfs["base_lidar"])
        want, stale = ref.search(geo, cost, m, x, y, z, cfg, guess), ref.search(geo, before, m, x, y, z, cfg, guess)
        assert want.stats.tobytes() != stale.stats.tobytes() and int(want.record["best_score"][0]) > 0
        assert pin.stats.tobytes() == want.stats.tobytes(), (pin.stats, want.stats)
        assert pin.rec.tobytes() == want.record.tobytes(), (pin.rec, want.record)
    finally:
        pin.close()
        hA.close(); hB.close()


def test_state_rules(gvamd):
    lib = gvamd.load()
    c = sc.by_name("tie")
    h = gvamd.GridVisionHIP(*mc.GRIDS[c["grid"]])
    good = lib_cfg(gvamd, c["cfg"])

    def code(call):
        with pytest.raises(gvamd.GVError) as e:
            call()
        return e.value.code

    def raw(guess=c["guess"], flags=0, result=True, handle=True, fn=None):
        q = gvamd.MatchGuess(*guess) if guess is not None else None
        res, stats = np.full(16, 7, np.int32), np.full(8, 7, np.int32)
        rc = (fn or lib.gv_match_search)(h._h if handle else None, C.byref(q) if q is not None else None, C.c_uint32(flags),
                                         res.ctypes.data_as(C.c_void_p) if result else None, stats.ctypes.data_as(C.c_void_p))
        return rc, res, stats

    try:
        search = lambda: h.match_search(c["guess"])                  # noqa: E731
        for fn in (lib.gv_match_search, lib.gv_match_search_async):
            assert raw(handle=False, fn=fn)[0] == GV_ERR_BAD_ARG
        assert lib.gv_set_search_config(None, C.byref(good)) == GV_ERR_BAD_ARG
        assert code(search) == GV_ERR_TF                             # no base_from_lidar
        h.set_transforms(base_lidar=c["tf"])
        assert code(search) == GV_ERR_STATE                          # no configuration
        h.set_match_config(gvamd.MatchConfig.of(wx=2, wy=2, wt=0, yaw_step=0.0))
        assert code(search) == GV_ERR_STATE                          # X16's configuration is not this one's
        h.set_search_config(good)
        assert code(search) == GV_ERR_STATE                          # no cloud
        h.upload_xyz(c["x"], c["y"], c["z"])
        assert code(search) == GV_ERR_STATE                          # no gv_inflate yet
        h.set_search_config(None)
        cost = _plant(h, c["mask"], c["inflation"])
        assert code(search) == GV_ERR_STATE                          # a costmap, no configuration
        h.set_search_config(good)
        a = sc.want(c)
        got = search()
        assert np.asarray(got[0]).tobytes() == a.record.tobytes() and np.asarray(got[1]).tobytes() == a.stats.tobytes()
        # a rejected configuration leaves the one in force alone
        for kw in (dict(wx=129), dict(wy=-1), dict(wt=33), dict(yaw_step=float("nan")), dict(wt=1, yaw_step=0.0), dict(stride=0),
                   dict(stride=1025), dict(min_points=0), dict(flags=2), dict(block_log2=0), dict(block_log2=5), dict(reserved=1)):
            base = dict(wx=2, wy=2, wt=0, yaw_step=0.0, stride=1, min_points=1, flags=0, block_log2=2)
            base.update(kw)
            assert code(lambda: h.set_search_config(gvamd.SearchConfig.of(**base))) == GV_ERR_BAD_ARG, kw
        assert np.asarray(search()[1]).tobytes() == a.stats.tobytes()
        # arguments: state unchanged, nothing written
        for kw in (dict(guess=None), dict(result=False), dict(flags=1), dict(flags=2), dict(guess=(float("nan"), 0.0, 0.0)),
                   dict(guess=(0.0, float("inf"), 0.0)), dict(guess=(0.0, 0.0, float("-inf")))):
            rc, res, stats = raw(**kw)
            assert rc == GV_ERR_BAD_ARG and (res == 7).all() and (stats == 7).all(), kw
        rc, res, stats = raw()
        assert rc == 0 and res.tobytes() == a.record.tobytes() and stats.tobytes() == a.stats.tobytes()
        # X16's call still refuses its flag 2, and its configuration wx = 33
        q, r16 = gvamd.MatchGuess(*c["guess"]), np.full(16, 7, np.int32)
        assert lib.gv_match_scan(h._h, C.byref(q), C.c_uint32(2), r16.ctypes.data_as(C.c_void_p), None) == GV_ERR_BAD_ARG
        assert code(lambda: h.set_match_config(gvamd.MatchConfig.of(wx=33, wy=2, wt=0, yaw_step=0.0))) == GV_ERR_BAD_ARG
        # the configuration is kept through gv_set_log_odds, gv_grid_move and gv_reset; gv_reset invalidates the costmap
        cost_b = _plant(h, np.zeros((h.ny, h.nx), bool), c["inflation"])
        assert np.asarray(search()[0]).tobytes() == sc.want(c, cost_b).record.tobytes() != a.record.tobytes()
        assert h.grid_move([0.0, 0.0, 0.0, 1.0, 0.3, -0.2, 0.0])["applied"]
        assert np.asarray(search()[0]).tobytes() == sc.want(c, cost_b).record.tobytes()     # the costmap is a snapshot
        h.reset()
        assert code(search) == GV_ERR_STATE
        _plant(h, c["mask"], c["inflation"])
        assert np.asarray(search()[1]).tobytes() == a.stats.tobytes()
        assert cost.tobytes() == h.costmap().tobytes()
    finally:
        h.close()


def test_search_demo(gvamd, tmp_path):
    """examples/search_demo.cpp (plain g++ over the C headers): a corner scene seen from a pose 8 m and 0.1 rad off,
    recovered with one call and checked against the host twin"""
    root = os.path.dirname(HERE)
    pkg = os.path.join(root, "grid-vision_amd")
    exe = str(tmp_path / "search_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(root, "include"), os.path.join(pkg, "examples", "search_demo.cpp"),
                           "-o", exe, "-L" + pkg, "-lgridvision_hip", "-Wl,-rpath," + pkg])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    m = re.search(r"recovered pose x (-?[\d.]+) y (-?[\d.]+) yaw (-?[\d.]+) \(true (-?[\d.]+) (-?[\d.]+) (-?[\d.]+)\)", out.stdout)
    assert m and "host twin ok" in out.stdout, out.stdout
    x, y, yaw, tx, ty, tyaw = (float(v) for v in m.groups())
    assert abs(x - tx) <= 0.051 and abs(y - ty) <= 0.051 and abs(yaw - tyaw) <= 0.0101
    assert np.hypot(tx, ty) >= 8.0 and abs(tyaw) >= 0.1
