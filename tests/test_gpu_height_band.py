"""[EXTENSION] X4 height band on the device: gv_set_height_band classifies every binned point by its fp32 base-frame z
(obstacle / clearing ground return / dropped) in the partition pass of the tile path and in the generic points pass.
Hits, miss, cell_idx and bbox_id bit-exact against the band composed from the oracle (height_band_ref.py), log-odds
bit-equal; the band off -- never set, NULL, {-inf, +inf, 0 / 1} -- gives the bytes of today."""
import ctypes as C

import numpy as np
import pytest

import grid_pass_ref
import height_band_ref as ref
import oracle_lib as ol
from gvamd import synth

pytestmark = pytest.mark.gpu

INF = float("inf")


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


def _flags(gvamd, bbox=True):
    f = gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH | gvamd.FRAME_KEEP_CELL_IDX | gvamd.FRAME_KEEP_COUNTS
    return f | (gvamd.FRAME_BBOX_TEST if bbox else 0)


def _handle(gvamd, grid, tfs):
    h = gvamd.GridVisionHIP(*grid)
    h.set_transforms(tfs["cam_lidar"], tfs["base_cam"], tfs["base_lidar"])
    return h


def _check_grid(h, og):
    """log-odds and int8 bit-equal; occupancy correctly rounded, and the oracle's where the host's expf is"""
    grid_pass_ref.check_layers(h.log_odds(), h.occupancy(), h.to_occupancy_grid()[0], og.log_odds, og.occupancy,
                               og.to_occupancy_grid()[0])


def _ids(tfs, x, y, z, bboxes):
    cx, cy, cz = ol.transform_cloud(ol.tf_to_matrix4f(tfs["cam_lidar"]), x, y, z)
    K = ol.set_intrinsic(synth.FX, synth.FY, synth.CX, synth.CY)
    return ol.extract_cloud_per_bbox(K, cx, cy, cz, bboxes, synth.IMG_W, synth.IMG_H)


def _set(h, band):
    if band is None:
        h.set_height_band(None)
    else:
        h.set_height_band(*band)


def _under_sensor(tfs, n=64, seed=3):
    """lidar-frame points straight below the sensor: base z around 0, in the sensor's own cell"""
    st = synth.Stream(seed, 7)
    m = ol.tf_to_matrix4f(tfs["base_lidar"]).reshape(4, 4)
    zz = -float(m[2, 3]) + st.uniform(n, -0.05, 0.05)
    return st.uniform(n, -0.02, 0.02), st.uniform(n, -0.02, 0.02), zz.astype(np.float32)


def _clouds(tfs, config, kind):
    if kind == "uniform":
        x, y, z, _ = synth.cloud_uniform(config, 60_000, seed_extra=5)   # base z over [-0.2, 5.8]: across every band
    else:
        x, y, z, _ = synth.scene_with_objects(tfs, n_total=200_000, n_obj=10, per=2000)
    ux, uy, uz = _under_sensor(tfs)
    return np.concatenate([x, ux]), np.concatenate([y, uy]), np.concatenate([z, uz])


def _bands(tfs, x, y, z):
    """thresholds exactly on points' base-frame z (inclusivity), both clearing modes, a band that drops everything,
    one that makes every point ground"""
    bz = ol.transform_cloud(ol.tf_to_matrix4f(tfs["base_lidar"]), x, y, z)[2]
    fin = np.sort(bz[np.isfinite(bz)])
    lo, hi = float(fin[int(0.3 * len(fin))]), float(fin[int(0.85 * len(fin))])
    assert np.count_nonzero(bz == np.float32(lo)) and np.count_nonzero(bz == np.float32(hi))
    return [(lo, hi, 1), (lo, hi, 0), (0.3, 2.5, 1), (-1e9, -1e9, 1), (1e9, 1e9, 1), (1e9, 1e9, 0)]


def _run_cases(gvamd, h, og, tfs, x, y, z, bboxes=None):
    h.upload_xyz(x, y, z)
    m_base = ol.tf_to_matrix4f(tfs["base_lidar"])
    ids = _ids(tfs, x, y, z, bboxes) if bboxes is not None else None
    for band in _bands(tfs, x, y, z) + [None]:
        _set(h, band)
        h.process_frame(_flags(gvamd, bboxes is not None), bboxes=bboxes)
        hits, cell, miss = ref.frame(og, m_base, x, y, z, band)
        assert np.array_equal(h.cell_idx(), cell), band
        assert np.array_equal(h.hits(), hits), band
        assert np.array_equal(h.miss(), miss.astype(np.int32)), band
        if ids is not None:
            assert np.array_equal(h.bbox_id(), ids), band
        _check_grid(h, og)
        if band == (1e9, 1e9, 0):
            assert hits.sum() == 0 and miss.sum() == 0
        if band == (1e9, 1e9, 1):
            assert hits.sum() == 0 and miss.sum() > 0


def test_band_off_is_bit_for_bit_today(gvamd):
    """never set, NULL after a band, {-inf, +inf, 0} and {-inf, +inf, 1}: the same bytes everywhere"""
    config = 2
    tfs = synth.transforms(True)
    g = synth.CONFIGS[config]["grid"]
    x, y, z, _ = synth.cloud_uniform(config)
    bboxes, poses = synth.detections(3, 20), synth.lshape_poses(config, 20)
    outs = []
    for mode in ("never", "null", "inf0", "inf1"):
        h = _handle(gvamd, (g.grid_x, g.grid_y, g.resolution), tfs)
        if mode == "null":
            h.set_height_band(0.5, 1.0, True)
            h.set_height_band(None)
        elif mode != "never":
            h.set_height_band(-INF, INF, mode == "inf1")
        h.upload_xyz(x, y, z)
        for _ in range(2):
            h.process_frame(_flags(gvamd), bboxes=bboxes, poses=poses)
        outs.append([h.hits(), h.miss(), h.cell_idx(), h.bbox_id(), h.log_odds(), h.occupancy(), h.to_occupancy_grid()[0]])
        h.close()
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("grid,config,perturbed", [((200, 200, 0.2), 2, True), ((200, 200, 0.1), 3, True),
                                                   ((200, 200, 0.2), 2, False)])
@pytest.mark.parametrize("cloud", ["uniform", "scene"])
def test_tile_path_matches_composition(gvamd, grid, config, perturbed, cloud):
    tfs = synth.transforms(perturbed)
    h = _handle(gvamd, grid, tfs)
    og = ol.OGrid(*grid)
    x, y, z = _clouds(tfs, config, cloud)
    _run_cases(gvamd, h, og, tfs, x, y, z, synth.detections(3, 20))
    h.close()


@pytest.mark.parametrize("setup", ["odd", "simple"])
def test_generic_path_matches_composition(gvamd, monkeypatch, setup):
    """nx % 4 != 0 (k_points + the literal march), and GV_RAY_IMPL=simple on a tile-path grid"""
    tfs = synth.transforms(True)
    if setup == "odd":
        grid = (50, 20, 0.3)
        tfs["base_lidar"] = np.array([0.0, 0.0, 0.0, 1.0, 50 / 3.0 + 1.7, -20 * 0.21, 1.8])
    else:
        grid = (200, 200, 0.2)
        monkeypatch.setenv("GV_RAY_IMPL", "simple")
    h = _handle(gvamd, grid, tfs)
    og = ol.OGrid(*grid)
    st = synth.Stream(77, grid[0])
    n = 40_000
    lx, ly = og.g.len_x, og.g.len_y
    ux, uy, uz = _under_sensor(tfs)
    x = np.concatenate([st.uniform(n, -0.8 * lx, 0.8 * lx), ux])
    y = np.concatenate([st.uniform(n, -0.8 * ly, 0.8 * ly), uy])
    z = np.concatenate([st.uniform(n, -2.5, 2.5), uz])
    _run_cases(gvamd, h, og, tfs, x, y, z, synth.detections(3, 10))
    h.close()


def test_scene_ground_patch_is_cleared(gvamd):
    """what the band is for: scene_with_objects at 1 M points, config-3 grid, four frames.  Without the band the ground
    returns (45 % of the points) put the whole patch above 0.5; with the band and clearing the patch's cells away from
    the obstacles end below it"""
    grid = (200, 200, 0.1)
    tfs = synth.transforms(False)
    x, y, z, _ = synth.scene_with_objects(tfs)
    m_base = ol.tf_to_matrix4f(tfs["base_lidar"])
    bx, by, bz = ol.transform_cloud(m_base, x, y, z)
    flags = gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH | gvamd.FRAME_KEEP_CELL_IDX | gvamd.FRAME_KEEP_COUNTS
    occ, hits = {}, {}
    for band in (None, (0.6, 2.5, 1)):
        h = _handle(gvamd, grid, tfs)
        _set(h, band)
        h.upload_xyz(x, y, z)
        for _ in range(4):
            h.process_frame(flags)
        occ[band], hits[band] = h.occupancy(), h.hits()
        cell = h.cell_idx()
        h.close()
    # the ground patch: cells that hold ground returns (base z < 0.6) inside x 5..85 m, |y| < 55 m
    g = (bz < 0.6) & (bx > 5) & (bx < 85) & (np.abs(by) < 55) & (cell >= 0)
    patch = np.zeros(len(occ[None]), bool)
    patch[cell[g]] = True
    away = patch & (hits[(0.6, 2.5, 1)] == 0)   # no obstacle return in the cell
    assert away.sum() > 100_000
    assert np.mean(occ[None][patch] > 0.5) == 1.0
    assert np.mean(occ[(0.6, 2.5, 1)][away] < 0.5) == 1.0


@pytest.mark.parametrize("lanes", [2, 3])
def test_pipelined_frames_keep_their_band(gvamd, monkeypatch, lanes):
    """frames in flight on two / three lanes, the band changed between enqueues: each frame uses the band it was
    enqueued with"""
    monkeypatch.setenv("GV_LANES", str(lanes))
    config = 2
    g = synth.CONFIGS[config]["grid"]
    tfs = synth.transforms(True)
    h = _handle(gvamd, (g.grid_x, g.grid_y, g.resolution), tfs)
    og = ol.OGrid(g.grid_x, g.grid_y, g.resolution)
    x, y, z = _clouds(tfs, config, "uniform")
    m_base = ol.tf_to_matrix4f(tfs["base_lidar"])
    bands = _bands(tfs, x, y, z)[:3] + [None]
    h.upload_xyz(x, y, z)
    flags = gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH | gvamd.FRAME_KEEP_COUNTS
    h.set_detections(flags)
    for f in range(14):
        band = bands[f % len(bands)]
        _set(h, band)
        h.enqueue_frame()
        hits, _, _ = ref.frame(og, m_base, x, y, z, band)
    h.synchronize()
    assert np.array_equal(h.hits(), hits)
    _check_grid(h, og)
    h.close()


def test_tick_uses_the_band_of_its_enqueue(gvamd):
    """gv_tick with lidar_bin + lidar_raymarch under a band equals the fused frame fed with the tick's poses and the
    same band, and the composition; a band set between tick_enqueue and tick_wait applies from the next tick on"""
    config = 2
    g = synth.CONFIGS[config]["grid"]
    grid = (g.grid_x, g.grid_y, g.resolution)
    tfs = synth.transforms(True)
    hA, hB = _handle(gvamd, grid, tfs), _handle(gvamd, grid, tfs)
    og = ol.OGrid(*grid)
    x, y, z, b = synth.scene_with_objects(tfs, n_total=200_000, n_obj=10, per=2000)
    m_base = ol.tf_to_matrix4f(tfs["base_lidar"])
    for h in (hA, hB):
        h.upload_xyz(x, y, z)
    st, dy = gvamd.filter_bboxes(b)
    net = synth.network_outputs(len(dy))
    flags = gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH | gvamd.FRAME_KEEP_COUNTS
    b1, b2 = (0.3, 2.5, 1), (0.1, 1.5, 0)
    hA.set_height_band(*b1)
    hA.tick_enqueue(b, k_near=4, vision=True, net=net, lidar_bin=True, lidar_raymarch=True)
    hA.set_height_band(*b2)                    # the pending tick keeps b1
    r = hA.tick_wait()
    for band, res in ((b1, r), (b2, None)):
        if res is None:
            res = hA.tick(b, k_near=4, vision=True, net=net, lidar_bin=True, lidar_raymarch=True)
        hB.set_height_band(*band)
        hB.process_frame(flags, poses=res["poses"])
        hits, _, _ = ref.frame(og, m_base, x, y, z, band, poses=res["poses"])
        assert np.array_equal(hA.log_odds(), hB.log_odds())
        assert np.array_equal(hA.to_occupancy_grid()[0], hB.to_occupancy_grid()[0])
        assert np.array_equal(hA.hits(), hB.hits())
        assert np.array_equal(hA.hits(), hits)
        _check_grid(hA, og)
    hA.close(); hB.close()


def test_sharded_frames_take_the_band(gvamd):
    """the sharded frame at world 1 and its one-device emulation at world 2 and 3 bin through the same partition launch:
    with a band they equal the plain frame"""
    config = 2
    g = synth.CONFIGS[config]["grid"]
    grid = (g.grid_x, g.grid_y, g.resolution)
    tfs = synth.transforms(True)
    x, y, z = _clouds(tfs, config, "scene")
    bboxes = synth.detections(3, 20)
    poses = synth.lshape_poses(config, 10)
    flags = gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH | gvamd.FRAME_BBOX_TEST | gvamd.FRAME_KEEP_CELL_IDX
    band = (0.3, 2.5, 1)
    ha = _handle(gvamd, grid, tfs)
    hb = _handle(gvamd, grid, tfs)
    hb.comm_init(gvamd.GridVisionHIP.comm_unique_id(), 0, 1)
    hc = [_handle(gvamd, grid, tfs) for _ in (2, 3)]
    for h in [ha, hb] + hc:
        h.set_height_band(*band)
        h.upload_xyz(x, y, z)
    for _ in range(2):
        ha.process_frame(flags, bboxes=bboxes, poses=poses)
        hb.process_frame_sharded(flags, bboxes=bboxes, poses=poses)
        for w, h in zip((2, 3), hc):
            h.frame_sharded_emulated(w, flags, bboxes=bboxes, poses=poses)
        want = [ha.log_odds(), ha.to_occupancy_grid()[0], ha.bbox_id()]
        for h in [hb] + hc:
            got = [h.log_odds(), h.to_occupancy_grid()[0], h.bbox_id()]
            for a, c in zip(want, got):
                assert np.array_equal(a, c)
        for h in hc:
            assert np.array_equal(h.cell_idx(), ha.cell_idx())
    hb.comm_destroy()
    for h in [ha, hb] + hc:
        h.close()


def test_bad_arguments_and_persistence(gvamd):
    """GV_ERR_BAD_ARG leaves the band as it was; the band survives reset, set_log_odds and grid_move"""
    config = 1
    g = synth.CONFIGS[config]["grid"]
    grid = (g.grid_x, g.grid_y, g.resolution)
    tfs = synth.transforms(True)
    h = _handle(gvamd, grid, tfs)
    x, y, z, _ = synth.cloud_uniform(config)
    h.upload_xyz(x, y, z)
    m_base = ol.tf_to_matrix4f(tfs["base_lidar"])
    band = (0.5, 3.0, 1)
    h.set_height_band(*band)
    lib = gvamd.load()
    for bad in ((float("nan"), 1.0, 1), (0.0, float("nan"), 0), (2.0, 1.0, 1), (0.0, 1.0, 2), (0.0, 1.0, -1)):
        with pytest.raises(gvamd.GVError) as e:
            h.set_height_band(*bad)
        assert e.value.code == 1
    assert lib.gv_set_height_band(None, C.byref(gvamd.HeightBand(0.0, 1.0, 1))) == 1
    flags = _flags(gvamd, bbox=False)
    for step in ("bad args", "reset", "set_log_odds", "grid_move"):
        if step == "reset":
            h.reset()
        elif step == "set_log_odds":
            h.set_log_odds(np.zeros(h.G, np.float32))
        elif step == "grid_move":
            h.grid_move((0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0))
        h.process_frame(flags)
        og = ol.OGrid(*grid)
        hits, cell, miss = ref.frame(og, m_base, x, y, z, band)
        assert np.array_equal(h.hits(), hits), step
        assert np.array_equal(h.miss(), miss.astype(np.int32)), step
        assert np.array_equal(h.cell_idx(), cell), step
    # +-inf are allowed, and equal to the band off
    h.set_height_band(-INF, INF, False)
    h.process_frame(flags)
    og = ol.OGrid(*grid)
    hits, _, _ = ref.frame(og, m_base, x, y, z, None)
    assert np.array_equal(h.hits(), hits)
    h.close()
