"""The grid pass bit for bit (tests/grid_pass_ref.py) through k_finalize_tiles (nx % 4 == 0), k_finalize_vec4
(GV_RAY_IMPL=simple) and k_finalize_scalar (nx % 4 != 0), with and without counts: log-odds and int8 bit-equal to the
restatement and the oracle, occupancy bit-equal to the correctly rounded reference and to the oracle's wherever the
host's expf is correctly rounded.

Sweep A runs every log-odds value a pass can output (grid_pass_ref: 93,952,410 of the 107,374,183 reachable values)
through each kernel; sweep B mixes hits, misses and up to 70 overlapping
rectangles per tile (the overflow branch of k_finalize_tiles) over random and edge starts, serial, pipelined and
sharded; sweep C the non-finite and extreme starts.  The rectangle tests hold poses with a negative or NaN size,
corners on cell and map edges, and a whole-map pose to the oracle through every path that makes rectangles."""
import time

import numpy as np
import pytest

import grid_pass_ref as R
import oracle_lib as ol
from gvamd import synth
from test_gpu_parity import check_grid, make_handle

pytestmark = pytest.mark.gpu
F32 = np.float32
IDENT = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])

# kernel -> grid (grid_x, grid_y, resolution), GV_RAY_IMPL
SWEEP_GRIDS = {"tiles": ((200, 200, 0.05), None),        # 4000 x 4000 = 16 M cells
               "vec4": ((200, 200, 0.05), "simple"),
               "scalar": ((255, 255, 0.07), None)}       # 3643 x 3643: nx % 4 == 3
SMALL_GRIDS = {"tiles": ((50, 20, 0.1), None),           # 500 x 200: neither side a multiple of 64
               "vec4": ((50, 20, 0.1), "simple"),
               "scalar": ((50, 20, 0.3), None)}          # 167 x 67


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


def _env(monkeypatch, impl, pipeline=None):
    if impl:
        monkeypatch.setenv("GV_RAY_IMPL", impl)
    else:
        monkeypatch.delenv("GV_RAY_IMPL", raising=False)
    if pipeline is not None:
        monkeypatch.setenv("GV_PIPELINE", pipeline)


def _handle(gvamd, grid):
    """identity transforms: lidar = base frame, the sensor at the base origin"""
    h = gvamd.GridVisionHIP(*grid)
    h.set_transforms(IDENT, IDENT, IDENT)
    return h


def _poses(rows):
    """(px, py, length, width) rows -> LSHAPE_DTYPE"""
    p = np.zeros(len(rows), synth.LSHAPE_DTYPE)
    for i, (px, py, ln, wd) in enumerate(rows):
        p[i] = (px, py, 0.0, 0.0, 0.0, 0.0, 1.0, ln, wd, 1.5)
    return p


def _whole_map(og, sign=1.0):
    """corners half a cell inside the map: the block is every cell"""
    return _poses([(og.g.pos_x, og.g.pos_y, sign * (og.g.len_x - og.g.res), sign * (og.g.len_y - og.g.res))])


def _centres(og, cells):
    """fp32 centres of flat cells (index (0,0) is the +x,+y corner)"""
    iy, ix = np.divmod(np.asarray(cells, np.int64), og.nx)
    x = og.g.pos_x + 0.5 * og.g.len_x - (ix + 0.5) * og.g.res
    y = og.g.pos_y + 0.5 * og.g.len_y - (iy + 0.5) * og.g.res
    return x.astype(F32), y.astype(F32), np.zeros(len(x), F32)


def _rect_counts(og, poses):
    """rectangles covering each cell, by the oracle's getIndex of the four corners (all inside, or none)"""
    k = np.zeros((og.ny, og.nx), np.int32)
    for p in poses:
        hx, hy = float(p["length"]) / 2.0, float(p["width"]) / 2.0
        px, py = float(p["px"]), float(p["py"])
        idx = [og.get_index(cx, cy) for cx, cy in ((px - hx, py - hy), (px + hx, py - hy), (px + hx, py + hy),
                                                     (px - hx, py + hy))]
        if all(i[0] for i in idx):
            xs, ys = [i[1] for i in idx], [i[2] for i in idx]
            k[min(ys):max(ys) + 1, min(xs):max(xs) + 1] += 1
    return k.reshape(-1)


def _check(h, og, want_lo=None, tag=""):
    return R.check_layers(h.log_odds(), h.occupancy(), h.to_occupancy_grid()[0], og.log_odds, og.occupancy,
                          og.to_occupancy_grid()[0], want_lo, tag)


# ----------------------------------------------------------------------------------------------- sweep A --
_PLAN = {}


def _plan_all():
    """every reachable value's start and recipe (decay and rectangles first, a frame's hit or miss where they cannot
    land), grouped by recipe; made once per module"""
    if not _PLAN:
        v, l0, rec = [], [], []
        for _, vc in R.chunks():
            a, r = R.plan(vc)
            v.append(vc), l0.append(a), rec.append(r)
        v, l0, rec = np.concatenate(v), np.concatenate(l0), np.concatenate(rec)
        for i, r in enumerate(R.RECIPES):
            m = rec == i
            _PLAN[r] = (v[m], l0[m])
    return _PLAN


class _Sweep:
    """one handle of a kernel form and its oracle grid: run() starts every cell from l0 and runs one pass of the
    recipe, then checks the whole grid and that the planned cells landed on their values"""

    def __init__(self, gvamd, grid, counts):
        self.gv, self.h, self.og = gvamd, _handle(gvamd, grid), ol.OGrid(*grid)
        self.G, self.counts = self.h.G, counts
        self.m_base = ol.tf_to_matrix4f(IDENT)
        self.hard = self.diff = self.cells = 0
        self._miss = None

    def miss_frame(self):
        """a cloud on the map's border cells: rays from the origin make nearly every other cell a miss"""
        if self._miss is None:
            og = self.og
            iy, ix = np.meshgrid(np.arange(og.ny), np.arange(og.nx), indexing="ij")
            border = ((ix == 0) | (iy == 0) | (ix == og.nx - 1) | (iy == og.ny - 1)).reshape(-1)
            x, y, z = _centres(og, np.nonzero(border)[0])
            hits, _ = og.bin_points(self.m_base, x, y, z)
            miss, _ = og.raymarch(self.m_base, x, y, z)
            self._miss = (x, y, z, hits, miss)
        return self._miss

    def run(self, v, l0, recipe):
        h, og, gv, G = self.h, self.og, self.gv, self.G
        start = np.zeros(G, F32)
        hits = miss = None
        if recipe == "miss":
            x, y, z, hits, miss = self.miss_frame()
            cells = np.nonzero((miss > 0) & (hits == 0))[0][:len(v)]
        else:
            cells = np.arange(len(v))
        start[cells] = l0[:len(cells)]
        h.set_log_odds(start)
        og.log_odds[:] = start
        k = {"rect1": 1, "rect2": 2}.get(recipe, 0)
        poses = np.concatenate([_whole_map(og)] * k) if k else None
        if not self.counts:
            if k:
                h.update_map_poses(poses)
                og.update_map_poses(poses)
            else:
                h.update_map()
                og.update_map()
        else:
            flags = gv.FRAME_BIN
            if recipe == "hit":
                x, y, z = _centres(og, np.arange(G))
                hits, miss = np.ones(G, np.int32), None
            elif recipe == "miss":
                flags |= gv.FRAME_RAYMARCH
            else:
                x, y, z = np.array([1e4], F32), np.zeros(1, F32), np.zeros(1, F32)   # outside: no hit
                hits = np.zeros(G, np.int32)
            h.upload_xyz(x, y, z)
            h.process_frame(flags, poses=poses)
            og.frame_update(poses, hits, miss)
        want = R.cell_update(start, k, None if hits is None else hits > 0, None if miss is None else miss > 0)
        nh, nd = _check(h, og, want, recipe)
        lo = h.log_odds()
        assert np.array_equal(lo[cells].view(np.uint32), v[:len(cells)].view(np.uint32)), f"{recipe}: plan missed"
        self.hard += nh
        self.diff += nd
        self.cells += len(cells)
        return len(cells)


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("counts", [False, True])
@pytest.mark.parametrize("kernel", ["tiles", "vec4", "scalar"])
def test_sweep_a_every_reachable_value(gvamd, monkeypatch, kernel, counts):
    """every reachable log-odds value, start by start: the no-counts form (update_map, update_map_poses) takes every
    value decay and rectangles land on, the counts form (frames) every value"""
    grid, impl = SWEEP_GRIDS[kernel]
    _env(monkeypatch, impl)
    t0 = time.time()
    plan = _plan_all()
    t1 = time.time()
    s = _Sweep(gvamd, grid, counts)
    covered = 0
    for r in R.RECIPES:
        v, l0 = plan[r]
        if not counts and r not in R.NO_COUNTS:
            continue
        i = 0
        while i < len(v):
            n = s.run(v[i:i + s.G], l0[i:i + s.G], r)
            assert n > 0
            i += n
        covered += len(v)
    short = sum(len(plan[r][0]) for r in R.RECIPES if r not in R.NO_COUNTS)
    assert covered == R.N_REACHABLE - R.N_NOT_OUTPUT - (0 if counts else short)
    print(f"\nsweep A {kernel} counts={counts}: {covered} of {R.N_REACHABLE} reachable values, all "
          f"{R.N_REACHABLE - R.N_NOT_OUTPUT} pass outputs "
          f"({'' if counts else f'{short} only a frame reaches; '}{s.cells} planned cells), {s.hard} fp64 hard cases, "
          f"occupancy differs from the oracle's host expf at {s.diff} cells; plan {t1 - t0:.1f} s, sweep "
          f"{time.time() - t1:.1f} s")
    s.h.close()


# ----------------------------------------------------------------------------------------------- sweep C --
def _specials():
    bits = [0x7FC00000, 0xFFC00000, 0x7FC00001, 0xFFC0BEEF, 0x7FFFFFFF, 0xFFFFFFFF,   # quiet NaNs, payloads
            0x7F800000, 0xFF800000, 0x00000000, 0x80000000,                            # +-inf, +-0
            0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00400000,                # subnormals
            0x7F7FFFFF, 0xFF7FFFFF]                                                    # +-FLT_MAX
    v = list(np.array(bits, np.uint32).view(F32))
    for c in (F32(-2.0) + F32(0.2), F32(3.6) + F32(0.2), F32(-2.0), F32(3.6), F32(-1.8), F32(3.8), F32(-0.8)):
        v += [np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf))]
    return np.array(v, F32)


@pytest.mark.parametrize("kernel", ["tiles", "vec4", "scalar"])
def test_sweep_c_non_finite_and_extreme_starts(gvamd, monkeypatch, kernel):
    grid, impl = SMALL_GRIDS[kernel]
    _env(monkeypatch, impl)
    h, og = _handle(gvamd, grid), ol.OGrid(*grid)
    G = h.G
    sp = _specials()
    start = np.resize(sp, G)
    m_base = ol.tf_to_matrix4f(IDENT)
    cells = np.arange(0, G, 3)
    x, y, z = _centres(og, cells)
    for step in ("decay", "rect1", "frame", "frame_rects"):
        h.set_log_odds(start)
        og.log_odds[:] = start
        if step == "decay":
            h.update_map(); og.update_map()
            want = R.cell_update(start)
        elif step == "rect1":
            p = _whole_map(og)
            h.update_map_poses(p); og.update_map_poses(p)
            want = R.cell_update(start, 1)
        else:
            p = np.concatenate([_whole_map(og)] * 2) if step == "frame_rects" else None
            h.upload_xyz(x, y, z)
            h.process_frame(gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH, poses=p)
            hits, _ = og.bin_points(m_base, x, y, z)
            miss, _ = og.raymarch(m_base, x, y, z)
            og.frame_update(p, hits, miss)
            want = R.cell_update(start, 2 if p is not None else 0, hits > 0, miss > 0)
            assert (hits > 0).any() and ((miss > 0) & (hits == 0)).any()
        _check(h, og, want, f"{kernel} {step}")
        lo, i8 = h.log_odds(), h.to_occupancy_grid()[0][::-1]
        nan = np.isnan(start)
        assert np.isnan(lo[nan]).all() and (i8[nan] == -1).all()
        assert not np.isnan(lo[~nan]).any()
    h.close()


# ----------------------------------------------------------------------------------------------- sweep B --
def _crowded_poses(og, st):
    """70 small rectangles inside the first 64 x 64 tile (+x,+y corner) mixed with 8 invalid ones, rectangles across
    tile borders, and random overlapping ones: k from 0 to well above 6"""
    res, hx, hy = og.g.res, og.g.pos_x + 0.5 * og.g.len_x, og.g.pos_y + 0.5 * og.g.len_y
    rows = []
    n = 70
    cx = hx - st.uniform(n, 8, 56).astype(np.float64) * res
    cy = hy - st.uniform(n, 8, 56).astype(np.float64) * res
    ln, wd = st.uniform(n, 1, 14).astype(np.float64) * res, st.uniform(n, 1, 14).astype(np.float64) * res
    rows += list(zip(cx, cy, ln, wd))
    rows += [(hx - 2 * res, hy - 10 * res, 8 * res, 2 * res)] * 4          # a corner beyond the + edge: skipped
    rows += [(hx - 30 * res, hy - 30 * res, np.nan, 4 * res)] * 4          # NaN: skipped
    for t in (64, 128):                                                    # across tile borders
        rows += [(hx - t * res, hy - t * res, 7.0 * res, 9.0 * res), (hx - t * res, hy - 20 * res, 3 * res, 5 * res)]
    m = 30
    rows += list(zip(st.uniform(m, og.g.pos_x - 0.4 * og.g.len_x, og.g.pos_x + 0.4 * og.g.len_x).astype(np.float64),
                     st.uniform(m, -0.4 * og.g.len_y, 0.4 * og.g.len_y).astype(np.float64),
                     st.uniform(m, -3.0, 6.0).astype(np.float64), st.uniform(m, -2.0, 4.0).astype(np.float64)))
    p = _poses(rows)
    k = _rect_counts(og, p)
    tile = k.reshape(og.ny, og.nx)[:64, :64]
    assert tile.max() > 6 and 0 in tile
    return p, k


def _edge_starts(G, st):
    edges = np.array([-2.0, 3.6, -1.8, 3.8, 0.0, -0.6, 2.75, -0.49999997, 1.9999999], F32)
    v = R.values(st.integers(G, 0, R.N_REACHABLE))
    v[::7] = np.resize(edges, len(v[::7]))
    return v


@pytest.mark.parametrize("mode", ["tiles_pipelined", "tiles_serial", "vec4", "scalar", "shard2", "shard3", "shard8"])
def test_sweep_b_frames_with_crowded_rectangles(gvamd, monkeypatch, mode):
    kernel = "scalar" if mode == "scalar" else ("vec4" if mode == "vec4" else "tiles")
    grid, impl = SMALL_GRIDS[kernel]
    _env(monkeypatch, impl, "0" if mode == "tiles_serial" else "1")
    h, og = _handle(gvamd, grid), ol.OGrid(*grid)
    st = synth.Stream(31337, len(mode))
    poses, k = _crowded_poses(og, st)
    start = _edge_starts(h.G, st)
    h.set_log_odds(start)
    og.log_odds[:] = start
    m_base = ol.tf_to_matrix4f(IDENT)
    lx, ly = og.g.len_x, og.g.len_y
    flags = gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH
    for f in range(3):
        n = 30_000
        x = st.uniform(n, og.g.pos_x - 0.6 * lx, og.g.pos_x + 0.6 * lx)
        y = st.uniform(n, -0.6 * ly, 0.6 * ly)
        z = st.uniform(n, -1.0, 1.0)
        l0 = og.log_odds.copy()
        h.upload_xyz(x, y, z)
        if mode.startswith("shard"):
            h.frame_sharded_emulated(int(mode[5:]), flags, poses=poses)
        else:
            h.set_detections(flags, poses=poses)
            h.enqueue_frame()
            h.synchronize()
        hits, _ = og.bin_points(m_base, x, y, z)
        miss, _ = og.raymarch(m_base, x, y, z)
        og.frame_update(poses, hits, miss)
        want = R.cell_update(l0, k, hits > 0, miss > 0)
        _check(h, og, want, f"{mode} frame {f}")
    h.close()


# ---------------------------------------------------------------------------------------------- rectangles --
def _edge_case_poses(og):
    """negative / NaN / inf / zero sizes, corners on cell edges and on the map's + (inside) and - (outside) edges"""
    res = og.g.res
    hx, hy = og.g.pos_x + 0.5 * og.g.len_x, og.g.pos_y + 0.5 * og.g.len_y      # the + edges (inside)
    lx = og.g.pos_x - 0.5 * og.g.len_x                                         # the - edge (outside)
    cx, cy = og.g.pos_x + 3.3 * res, og.g.pos_y - 2.1 * res
    nan, inf = float("nan"), float("inf")
    rows = [(cx, cy, -2.0, 1.0), (cx, cy, 1.5, -3.0), (cx, cy, -2.5, -0.7), (cx + 7 * res, cy, -0.0, 0.0),
            (cx, cy + 9 * res, 0.0, 0.0), (cx, cy, nan, 1.0), (cx, cy, 1.0, nan), (nan, cy, 1.0, 1.0),
            (cx, cy, inf, 1.0), (cx, cy, -inf, 1.0), (inf, cy, 1.0, 1.0), (cx, cy, 1e300, 1.0),
            (hx - 10 * res - 2 * res, cy, 4 * res, 6 * res),      # corners on cell edges
            (hx - 2 * res, hy - 3 * res, 4 * res, 2 * res),       # a corner on the + edges: inside
            (hx - 2 * res, hy - 3 * res, -4 * res, -2 * res),
            (lx + 2 * res, cy, 4 * res, 2 * res),                 # a corner on the - edge: outside
            (lx + 2 * res, cy, -4 * res, 2 * res),
            (lx + 2.5 * res, cy, 4 * res, 2 * res)]
    return np.concatenate([_poses(rows), _whole_map(og), _whole_map(og, -1.0)])


@pytest.mark.parametrize("kernel", ["tiles", "vec4", "scalar"])
def test_rectangle_edges_update_map_poses_and_frames(gvamd, monkeypatch, kernel):
    """negative sizes fill the block of |length| x |width| (the reference's min / max of the corner indices): through
    update_map_poses, the binning frame (rectangles folded into the partition launch) and the frame without binning"""
    grid, impl = ((20, 20, 0.25), None) if kernel == "tiles" else (((20, 20, 0.25), "simple") if kernel == "vec4"
                                                                   else ((21, 20, 0.3), None))
    _env(monkeypatch, impl)
    h, og = _handle(gvamd, grid), ol.OGrid(*grid)
    poses = _edge_case_poses(og)
    k = _rect_counts(og, poses)
    neg = poses[(poses["length"] < 0) & np.isfinite(poses["length"])]
    assert _rect_counts(og, neg).sum() > 0, "negative-length poses must cover cells"
    m_base = ol.tf_to_matrix4f(IDENT)
    x, y, z = _centres(og, np.arange(0, h.G, 5))
    for step in range(4):
        l0 = og.log_odds.copy()
        if step < 2:
            h.update_map_poses(poses)
            og.update_map_poses(poses)
            want = R.cell_update(l0, k)
        else:
            flags = gvamd.FRAME_BIN if step == 2 else 0
            h.upload_xyz(x, y, z)
            h.process_frame(flags, poses=poses)
            hits = og.bin_points(m_base, x, y, z)[0] if flags else None
            og.frame_update(poses, hits, None)
            want = R.cell_update(l0, k, None if hits is None else hits > 0, None)
        _check(h, og, want, f"{kernel} step {step}")
    # update_map_points: an unknown label's depth is -1, a reversed box
    pts = np.array([[og.g.pos_x, 0.5, 0.0], [og.g.pos_x - 3.0, -1.0, 0.0]], np.float64)
    bb = np.zeros(2, synth.BBOX_DTYPE)
    bb["label"] = [9, 14]
    l0 = og.log_odds.copy()
    h.update_map_points(pts, bb)
    og.update_map_points(pts, bb)
    _check(h, og, None, f"{kernel} points")
    assert np.count_nonzero(og.log_odds != R.cell_update(l0)) > 0
    h.close()


def _negative_net(nb, seed=7):
    orient, conf, dims = synth.network_outputs(nb, seed=seed)
    dims[::2, 2] = -6.0          # length = dims[2] + class average < 0 for every class
    dims[1::4, 0] = -4.0         # and some widths
    return orient, conf, dims


def test_vision_negative_length_post_process_and_frame(gvamd):
    """vision_post_process keeps the oracle's negative length; the frame with FRAME_VISION_ORIENT fills its block"""
    config = 2
    h, tfs = make_handle(gvamd, config)
    g = synth.CONFIGS[config]["grid"]
    og = ol.OGrid(g.grid_x, g.grid_y, g.resolution)
    nb = 20
    bboxes = synth.detections(3, nb)
    orient, conf, dims = _negative_net(nb)
    got = h.vision_post_process(orient, conf, dims, bboxes)
    want = ol.post_process(ol.make_cam(synth.FX, synth.FY, synth.CX, synth.CY, synth.IMG_W, synth.IMG_H), orient,
                           conf, dims, bboxes)
    assert len(got) == len(want) and (got["length"] < 0).sum() >= 3
    assert np.array_equal(got["length"], want["length"]) and np.array_equal(got["width"], want["width"])
    base = h.transform_lshape_objects(got)
    assert _rect_counts(og, base[base["length"] < 0]).sum() > 0, "fixture: negative boxes inside the map"
    x, y, z, _ = synth.cloud_uniform(config, 20_000)
    h.upload_xyz(x, y, z)
    h.process_frame(gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH | gvamd.FRAME_VISION_ORIENT, bboxes=bboxes,
                    net=(orient, conf, dims))
    m_base = ol.tf_to_matrix4f(tfs["base_lidar"])
    hits, _ = og.bin_points(m_base, x, y, z)
    miss, _ = og.raymarch(m_base, x, y, z)
    og.frame_update(base, hits, miss)
    check_grid(h, og)
    h.close()


def test_tick_negative_length(gvamd):
    """the tick's vision branch with negative lengths, and its PCA branch's "no pose" boxes: the grid equals the
    oracle's update with the tick's poses"""
    config = 2
    g = synth.CONFIGS[config]["grid"]
    tfs = synth.transforms(True)
    h, _ = make_handle(gvamd, config, perturbed=True)
    og = ol.OGrid(g.grid_x, g.grid_y, g.resolution)
    x, y, z, b = synth.scene_with_objects(tfs, n_total=200_000, n_obj=10, per=2000)
    h.upload_xyz(x, y, z)
    st, dy = gvamd.filter_bboxes(b)
    r = h.tick(b, k_near=4, vision=True, net=_negative_net(len(dy)))
    assert (r["poses"]["length"] < 0).sum() >= 2
    og.update_map_poses(r["poses"])
    check_grid(h, og)
    # PCA branch: boxes without points carry the NaN "no pose" marker on the device and add nothing
    bad = b.copy()
    bad["x_min"][::2] = 5000.0
    bad["x_max"][::2] = 5001.0
    r = h.tick(bad, k_near=4)
    og.update_map_poses(r["poses"])
    check_grid(h, og)
    h.close()
