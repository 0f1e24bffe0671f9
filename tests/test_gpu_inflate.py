"""[EXTENSION] X6 inflated costmap on the device: gv_inflate against inflate_ref (every offset of the disc, no
decomposition) with zero tolerance.  Patterns are planted with set_log_odds + update_map, the packed int8 is read back
with to_occupancy_grid and THAT readback goes to the reference: the device is held to its own grid, which other tests
pin.  Every comparison is tobytes() equality of costmap(), and of obstacle_dist2() where kept, and every inflate is
made three times with the same bytes.  Then the ordering against pipelined frames and a pending tick (the twin-handle
pattern of test_gpu_tick.py), reconfiguration with passes in flight, and the state rules of the header."""
import ctypes as C

import numpy as np
import pytest

import inflate_cases as ic
import inflate_ref as ref
from grid_move_ref import np_move
from gvamd import synth
from planner_util import plant_grid
from test_gpu_parity import _ground_scene, make_handle

pytestmark = pytest.mark.gpu

GV_ERR_STATE = 5
_REF = {}      # (grid bytes, nx, ny, cfg, res) -> (cost, dist2): one reference per grid and configuration
_HANDLES = {}  # grid name -> handle, shared by the cases of the module


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    yield m
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()
    _REF.clear()


def _handle(gvamd, grid):
    if grid not in _HANDLES:
        (gx, gy, res), (nx, ny) = ic.GRIDS[grid]
        h = gvamd.GridVisionHIP(gx, gy, res)
        assert (h.nx, h.ny) == (nx, ny)
        _HANDLES[grid] = h
    h = _HANDLES[grid]
    h.reset()
    return h, ic.GRIDS[grid][0][2]


def _want(i8, nx, ny, cfg, res):
    key = (i8.tobytes(), nx, ny, cfg, res)
    if key not in _REF:
        _REF[key] = ref.costmap(i8, nx, ny, cfg, res)
    return _REF[key]


def _set(h, cfg):
    h.set_inflation(cfg.inscribed, cfg.inflation, cfg.scaling, cfg.thr, keep_dist2=bool(cfg.flags & ref.KEEP_DIST2),
                    occupancy_scale=bool(cfg.flags & ref.OCCUPANCY_SCALE))


def _check(h, i8, cfg, res, tag=""):
    """inflate three times; cost and dist2 equal the reference of i8 byte for byte each time"""
    cost, d2 = _want(i8, h.nx, h.ny, cfg._replace(flags=cfg.flags & ~ref.KEEP_DIST2), res)
    _set(h, cfg._replace(flags=cfg.flags | ref.KEEP_DIST2))
    for rep in range(3):
        h.inflate()
        got_c, got_d = h.costmap(), h.obstacle_dist2()
        assert got_d.dtype == np.uint16 and got_d.tobytes() == d2.tobytes(), (tag, rep, "dist2", _first_diff(got_d, d2, h.nx))
        assert got_c.dtype == np.uint8 and got_c.tobytes() == cost.tobytes(), (tag, rep, "cost", _first_diff(got_c, cost, h.nx))
    return cost, d2


def _first_diff(got, want, nx):
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    if not len(bad):
        return None
    b = int(bad[0])
    return dict(n=len(bad), x=b % nx, y=b // nx, got=int(got.reshape(-1)[b]), want=int(want.reshape(-1)[b]))


# grid -> the parameter set it runs with
CASES = [("500x200", "P1"), ("500x200", "P2"), ("250x100", "P1"), ("250x100", "P2"), ("200x200", "P3"), ("200x80", "P4"),
         ("2000x2000", "P1")]


@pytest.mark.parametrize("grid,pset", CASES)
def test_single_cell(gvamd, grid, pset):
    h, res = _handle(gvamd, grid)
    pres, cfg = ic.PSETS[pset]
    assert pres == res
    i8 = plant_grid(h, ic.single_cell(h.nx, h.ny))
    cost, d2 = _check(h, i8, cfg, res, (grid, pset))
    table = ref.cost_table(cfg, res)
    assert (cost == 254).sum() == 1 and (d2 != ref.NONE).sum() > 4 and int(d2[d2 != ref.NONE].max()) <= len(table) - 1
    r = int(np.sqrt(len(table) - 1))   # the whole disc is on the map: every distance that exists shows its cost
    reach = {dx * dx + dy * dy for dx in range(r + 1) for dy in range(r + 1) if dx * dx + dy * dy < len(table)}
    assert set(d2[d2 != ref.NONE].tolist()) == reach
    assert set(cost.reshape(-1).tolist()) == {int(table[q]) for q in reach} | {0}


@pytest.mark.parametrize("grid,pset", [("500x200", "P1"), ("500x200", "P2"), ("250x100", "P1"), ("250x100", "P2"),
                                       ("200x200", "P3"), ("200x80", "P4")])
def test_borders(gvamd, grid, pset):
    h, res = _handle(gvamd, grid)
    _, cfg = ic.PSETS[pset]
    rc = int(np.sqrt(ref.d2max_of(cfg, res)))
    i8 = plant_grid(h, ic.border_fixture(h.nx, h.ny, rc))
    cost, d2 = _check(h, i8, cfg, res, (grid, pset))
    y = h.ny // 2
    assert cost[y, h.nx - 1] == 254 and cost[y + 1, 0] == 0 and d2[y + 1, 0] == ref.NONE   # the reference: no wrap


def test_seams_p1(gvamd):
    h, res = _handle(gvamd, "2000x2000")
    mask, probes = ic.seam_fixture(h.nx, h.ny, 30, ic.seam_anchors_p1(), spacing=16)
    i8 = plant_grid(h, mask)
    cost, d2 = _check(h, i8, ic.PSETS["P1"][1], res, "seams P1")
    for x, y, d in probes:
        assert d2[y, x] == (d if d <= 30 else ref.NONE)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_seams_p3(gvamd, k):
    h, res = _handle(gvamd, "200x200")
    mask, probes = ic.seam_fixture(h.nx, h.ny, 4019, ic.seam_anchors_p3(k), spacing=97)
    i8 = plant_grid(h, mask)
    cost, d2 = _check(h, i8, ic.PSETS["P3"][1], res, ("seams P3", k))
    for x, y, d in probes:
        assert d2[y, x] == (d if d <= 4019 else ref.NONE)


@pytest.mark.parametrize("grid,pset", [("500x200", "P1"), ("500x200", "P2"), ("250x100", "P2"), ("200x200", "P3"),
                                       ("200x80", "P4"), ("2000x2000", "P1")])
@pytest.mark.parametrize("density", [5e-4, 0.3])
def test_random_masks(gvamd, grid, pset, density):
    h, res = _handle(gvamd, grid)
    i8 = plant_grid(h, ic.random_mask(h.nx, h.ny, density, seed=11))
    _check(h, i8, ic.PSETS[pset][1], res, (grid, pset, density))


@pytest.mark.parametrize("grid,pset", [("500x200", "P2"), ("250x100", "P1"), ("200x200", "P3")])
def test_row_column_empty_and_full(gvamd, grid, pset):
    h, res = _handle(gvamd, grid)
    cfg = ic.PSETS[pset][1]
    _check(h, plant_grid(h, ic.row_and_column(h.nx, h.ny)), cfg, res, "row and column")
    cost, d2 = _check(h, plant_grid(h, np.zeros((h.ny, h.nx), bool)), cfg, res, "empty")
    assert not cost.any() and (d2 == ref.NONE).all()
    cost, d2 = _check(h, plant_grid(h, np.ones((h.ny, h.nx), bool)), cfg, res, "full")
    assert (cost == 254).all() and not d2.any()


def _write_packed_layer(h, i8):
    """the packed layer written in place through gv_device_layers' pointer (the grid pass clamps log-odds to
    [-2, 3.6], so it can only give 11 .. 97 and -1)"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.synchronize()
    assert hip.hipMemcpy(h.device_layers()[0], i8.ctypes.data, i8.size, 1) == 0   # hipMemcpyHostToDevice


@pytest.mark.parametrize("thr", [1, 50, 51, 100])
def test_threshold(gvamd, thr):
    h, res = _handle(gvamd, "500x200")
    cfg = ic.PSETS["P1"][1]._replace(thr=thr)
    # through the grid pass: a ramp over the clamp range and NaN cells -> every int8 the pass can give, and -1
    lo = np.linspace(-2.4, 4.0, h.G).astype(np.float32)
    lo[::97] = np.nan
    np.random.default_rng(3).shuffle(lo)
    h.set_log_odds(lo)
    h.update_map()
    ramp = h.to_occupancy_grid()[0]
    assert sorted(set(ramp.tolist())) == [-1] + list(range(11, 98))
    # every value of 0 .. 100 and -1: written into the packed layer directly
    full = ic.threshold_fixture(h.nx, h.ny)
    for name, i8 in (("ramp", ramp), ("full", full)):
        if name == "full":
            _write_packed_layer(h, full)
            assert h.to_occupancy_grid()[0].tobytes() == full.tobytes()
        cost, d2 = _check(h, i8, cfg, res, (name, thr))
        lethal = i8.reshape(h.ny, h.nx) >= thr
        assert np.array_equal(d2 == 0, lethal) and np.array_equal(cost == 254, lethal)
        assert (i8 == -1).any() and not lethal[i8.reshape(h.ny, h.nx) == -1].any()


def test_flags(gvamd):
    h, res = _handle(gvamd, "250x100")
    cfg = ic.PSETS["P2"][1]
    i8 = plant_grid(h, ic.random_mask(h.nx, h.ny, 2e-3, seed=4))
    plain, _ = _check(h, i8, cfg, res, "plain")
    scaled, _ = _check(h, i8, cfg._replace(flags=ref.OCCUPANCY_SCALE), res, "occupancy scale")
    assert scaled.max() == 100 and plain.max() == 254 and np.array_equal(scaled == 0, plain == 0)
    _set(h, cfg._replace(flags=ref.OCCUPANCY_SCALE))   # without KEEP_DIST2
    for _ in range(3):
        h.inflate()
        assert h.costmap().tobytes() == scaled.tobytes()
        with pytest.raises(gvamd.GVError) as e:
            h.obstacle_dist2()
        assert e.value.code == GV_ERR_STATE


P5 = ic.PSETS["P5"][1]._replace(thr=50)


def _want_p5(h, i8, cfg=P5):
    return _want(i8, h.nx, h.ny, cfg, ic.PSETS["P5"][0])[0]


def test_inflate_between_pipelined_frames(gvamd):
    """A: frame 1, inflate, publish to buffer 1, frame 2 (other detections), inflate, publish to buffer 2, one
    synchronize.  B: the two frames one by one.  Each buffer is the reference of its own grid."""
    hA, _ = make_handle(gvamd, 2)
    hB, _ = make_handle(gvamd, 2)
    assert synth.CONFIGS[2]["grid"].resolution == ic.PSETS["P5"][0]
    x, y, z, _ = synth.cloud_uniform(2)
    flags = gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH
    poses = [synth.lshape_poses(2, 12, seed_extra=1), synth.lshape_poses(2, 30, seed_extra=2)]
    pins = [gvamd.PinnedI8(hA.G), gvamd.PinnedI8(hA.G)]
    try:
        for h in (hA, hB):
            h.upload_xyz(x, y, z)
        _set(hA, P5)
        grids = []
        for i in range(2):
            pins[i].array[:] = 77
            hA.set_detections_async(flags, poses=poses[i])
            hA.enqueue_frame()
            hA.inflate()
            hA.publish_costmap_async(pins[i].array)
            hB.set_detections(flags, poses=poses[i])
            hB.enqueue_frame()
            hB.synchronize()
            grids.append(hB.to_occupancy_grid()[0])
        hA.synchronize()
        assert grids[0].tobytes() != grids[1].tobytes()
        want = [_want_p5(hB, g) for g in grids]
        assert want[0].tobytes() != want[1].tobytes() and (want[0] == 254).any()
        for i in range(2):
            assert pins[i].array.view(np.uint8).tobytes() == want[i].tobytes(), i
        assert hA.costmap().tobytes() == want[1].tobytes()
    finally:
        for p in pins:
            p.close()
        hA.close(); hB.close()


def test_inflate_during_a_pending_tick(gvamd):
    """tick_enqueue, inflate, publish, tick_wait: the costmap is that of the tick's grid.  Threshold 80: a cell the
    lidar hit reads 73 after one tick and 88 after two, so the grid before the pending tick has another costmap."""
    cfg = P5._replace(thr=80)
    hA, tfs = make_handle(gvamd, 2, perturbed=True)
    hB, _ = make_handle(gvamd, 2, perturbed=True)
    x, y, z, K, b = _ground_scene(tfs, seed=9)
    pin = gvamd.PinnedI8(hA.G)
    try:
        for h in (hA, hB):
            h.upload_xyz(x, y, z)
            h.tick(b, k_near=4, lidar_bin=True)
        before = hB.to_occupancy_grid()[0]
        _set(hA, cfg)
        pin.array[:] = 77
        hA.tick_enqueue(b, k_near=4, lidar_bin=True)
        hA.inflate()
        hA.publish_costmap_async(pin.array)
        rA = hA.tick_wait()
        hA.synchronize()
        rB = hB.tick(b, k_near=4, lidar_bin=True)
        assert len(rA["poses"]) == len(rB["poses"]) >= 1
        grid = hB.to_occupancy_grid()[0]
        assert grid.tobytes() != before.tobytes() and hA.to_occupancy_grid()[0].tobytes() == grid.tobytes()
        want = _want_p5(hB, grid, cfg)
        assert (want == 254).any() and want.tobytes() != _want_p5(hB, before, cfg).tobytes()
        assert pin.array.view(np.uint8).tobytes() == want.tobytes()
        assert hA.costmap().tobytes() == want.tobytes()
    finally:
        pin.close()
        hA.close(); hB.close()


def test_reconfiguration_in_flight(gvamd):
    """inflate with P1, publish, set P2, inflate, publish, (and P1 again: the first table's slot is reused), one
    synchronize: each buffer matches its own table"""
    h, res = _handle(gvamd, "500x200")
    i8 = plant_grid(h, ic.random_mask(h.nx, h.ny, 1e-3, seed=21))
    cfgs = [ic.PSETS["P1"][1], ic.PSETS["P2"][1], ic.PSETS["P1"][1]._replace(flags=ref.OCCUPANCY_SCALE)]
    want = [_want(i8, h.nx, h.ny, c, res)[0] for c in cfgs]
    pins = [gvamd.PinnedI8(h.G) for _ in cfgs]
    try:
        for c, p in zip(cfgs, pins):
            p.array[:] = 77
            _set(h, c)
            h.inflate()
            h.publish_costmap_async(p.array)
        h.synchronize()
        for k, (w, p) in enumerate(zip(want, pins)):
            assert p.array.view(np.uint8).tobytes() == w.tobytes(), k
        assert len({w.tobytes() for w in want}) == 3
    finally:
        for p in pins:
            p.close()


def test_state_rules(gvamd):
    (gx, gy, res), _ = ic.GRIDS["250x100"]
    h = gvamd.GridVisionHIP(gx, gy, res)
    cfg = ic.PSETS["P1"][1]

    def state_error(call):
        with pytest.raises(gvamd.GVError) as e:
            call()
        return e.value.code == GV_ERR_STATE

    pin = gvamd.PinnedI8(h.G)
    try:
        assert state_error(h.inflate)                       # nothing set
        assert state_error(h.costmap) and state_error(h.obstacle_dist2)
        assert state_error(lambda: h.publish_costmap_async(pin.array))
        _set(h, cfg._replace(flags=ref.KEEP_DIST2))
        assert state_error(h.costmap)                       # set, not inflated yet
        with pytest.raises(gvamd.GVError) as e:             # a rejected configuration leaves the one in force alone
            h.set_inflation(0.35, 0.2, 10.0, 65)
        assert e.value.code == 1
        i8 = plant_grid(h, ic.random_mask(h.nx, h.ny, 2e-3, seed=8))
        want, want_d = _want(i8, h.nx, h.ny, cfg, res)
        h.inflate()
        assert h.costmap().tobytes() == want.tobytes() and h.obstacle_dist2().tobytes() == want_d.tobytes()
        # a later map update leaves the snapshot alone until the next inflate
        i8b = plant_grid(h, ic.random_mask(h.nx, h.ny, 2e-3, seed=9))
        assert i8b.tobytes() != i8.tobytes()
        assert h.costmap().tobytes() == want.tobytes()
        h.inflate()
        want_b = _want(i8b, h.nx, h.ny, cfg, res)[0]
        assert h.costmap().tobytes() == want_b.tobytes() != want.tobytes()
        # gv_reset invalidates the costmap and keeps the configuration; so does gv_grid_move keep it
        h.reset()
        assert state_error(h.costmap) and state_error(h.obstacle_dist2)
        plant_grid(h, ic.random_mask(h.nx, h.ny, 2e-3, seed=9))
        planted = h.log_odds(), h.occupancy(), h.to_occupancy_grid()[0]
        info = h.grid_move([0.0, 0.0, 0.0, 1.0, 3 * res, -2 * res, 0.0])
        assert info["applied"]
        h.inflate()
        moved = h.to_occupancy_grid()[0]
        assert moved.tobytes() != i8b.tobytes()
        want_moved = np_move(planted, h.nx, h.ny, res, h.pos_x, h.pos_y, info)   # nx % 4 == 2: k_grid_move1
        assert (h.log_odds().tobytes(), h.occupancy().tobytes(), moved.tobytes()) == tuple(a.tobytes() for a in want_moved)
        assert h.costmap().tobytes() == _want(moved, h.nx, h.ny, cfg, res)[0].tobytes()
        h.set_inflation(None)
        assert state_error(h.inflate)
        assert h.costmap().tobytes() == _want(moved, h.nx, h.ny, cfg, res)[0].tobytes()   # the snapshot stays readable
    finally:
        pin.close()
        h.close()
