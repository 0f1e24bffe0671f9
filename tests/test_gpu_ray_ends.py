"""The sector ray stage end by end: the scenes of tests/ray_cases.py (single ends on every cell, single long ends on
and beside every sector boundary, rings and bands with gaps, lines that crowd one slope bucket, a and b beyond 4096)
through one frame each, miss and hit grids bit-equal to the oracle's literal march.  No tolerances.  The knobs of the
handle move the kernel's thresholds across the scenes; tests/test_ray_cases_host.py proves on the CPU that the scenes
are what they claim to be.

GV_LOG2S: a column of a sector is one 32-bit word of cell bits, and the last sector of an x-major octant is
floor(a / S) + 1 cells wide at column a, so a wedge of 512 columns needs S = 32: GV_LOG2S=5 is the smallest value the
kernel's w <= 32 allows on G1024 (4 would do for 511 columns only; 3 gives 64 cells and more).  5 is also what the host
picks for 511 / 512 columns, so GV_LOG2S=6 runs beside it: sector boundaries the defaults do not have.  The library's
own plan says the same: tests/test_sector_plan_host.py::test_gpu_suite_knob_sets asks it, on the CPU, about every (scene
set, knob set) pair run here and about the two excluded ones; test_wide_column_is_refused runs an excluded pair."""
import numpy as np
import pytest

import oracle_lib as ol
import ray_cases as rc
from gvamd import synth
from ray_cases import KNOBS, SETS, TAILS_B, TUNE_BD, TUNE_C
from test_gpu_parity import check_grid

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


@pytest.fixture(scope="module")
def cache():
    """scene lists with the oracle's results, computed once and shared by the tuning sets; freed with the module"""
    c = {}
    yield c
    c.clear()


def flags(gvamd):
    return gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH | gvamd.FRAME_KEEP_COUNTS


def make_handle(gvamd, monkeypatch, geo, tune):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in tune.items():
        monkeypatch.setenv(k, v)
    h = gvamd.GridVisionHIP(*geo.grid)
    assert (h.nx, h.ny) == (geo.nx, geo.ny)
    tfs = synth.transforms(False)
    h.set_transforms(tfs["cam_lidar"], tfs["base_cam"], geo.tf)
    return h


def differing(geo, got, want):
    """the first differing cells as (octant, a, b, got, want) relative to the origin: names the ray"""
    bad = np.flatnonzero(got != want)
    return len(bad), [(*geo.octant_ab(int(i) % geo.nx, int(i) // geo.nx), int(got[i]), int(want[i])) for i in bad[:6]]


def run_frame(gvamd, h, geo, x, y, z, want_miss, want_hits, tag):
    """one frame of the cloud; miss and hit grids against the oracle's"""
    h.upload_xyz(x, y, z)
    h.process_frame(flags(gvamd))
    miss, hits = h.miss(), h.hits()
    if not np.array_equal(miss, want_miss):
        pytest.fail(f"{tag}: miss grid differs at (count, [(octant, a, b, got, want)]) {differing(geo, miss, want_miss)}")
    if not np.array_equal(hits, want_hits):
        pytest.fail(f"{tag}: hit counts differ at {differing(geo, hits, want_hits)}")


# ---- references: the oracle's march of every scene, computed once per scene list and shared by the tuning sets
class SceneSet:
    """what a scene list needs to run again: the clouds (a gap scene as a bit mask over the points of its gap-less
    scene) and the oracle's miss and hit grids in compact form"""

    def __init__(self, geo, scenes, parents, dense):
        self.geo, self.dense = geo, dense
        self.names = [s.name for s in scenes]
        og = rc.oracle_grid(geo)
        self.refs = rc.map_threads(lambda s: self._compact(og, s), scenes)
        cell = lambda s: s.ends[:, 1].astype(np.int64) * geo.nx + s.ends[:, 0]
        self.clouds = []
        for s, p in zip(scenes, parents):
            if p is None:
                self.clouds.append((s.x, s.y))
            else:
                keep = np.isin(cell(scenes[p]), cell(s))
                assert np.array_equal(scenes[p].x[keep], s.x) and np.array_equal(scenes[p].y[keep], s.y)
                self.clouds.append((p, np.packbits(keep)))

    def _compact(self, og, scene):
        miss, hits = rc.oracle_miss(og, scene), rc.oracle_hits(og, scene)
        cells = np.flatnonzero(hits)
        return (np.packbits(miss) if self.dense else np.flatnonzero(miss).astype(np.int32)), cells, hits[cells]

    def __len__(self):
        return len(self.names)

    def cloud(self, i):
        a, b = self.clouds[i]
        if isinstance(a, int):
            x, y = self.clouds[a]
            keep = np.unpackbits(b, count=len(x)).astype(bool)
            a, b = x[keep], y[keep]
        return a, b, np.zeros(len(a), np.float32)

    def want(self, i):
        m, cells, counts = self.refs[i]
        G = self.geo.nx * self.geo.ny
        if self.dense:
            miss = np.unpackbits(m, count=G).astype(np.int32)
        else:
            miss = np.zeros(G, np.int32)
            miss[m] = 1
        hits = np.zeros(G, np.int32)
        hits[cells] = counts
        return miss, hits


def scene_set(cache, key, build, dense):
    """build() -> (geo, scenes, parents or None)"""
    if key not in cache:
        geo, scenes, parents = build()
        cache[key] = SceneSet(geo, scenes, parents or [None] * len(scenes), dense)
    return cache[key]


def run_scenes(gvamd, monkeypatch, ss, tune):
    h = make_handle(gvamd, monkeypatch, ss.geo, tune)
    try:
        for i in range(len(ss)):
            run_frame(gvamd, h, ss.geo, *ss.cloud(i), *ss.want(i), ss.names[i])
    finally:
        h.close()
    return len(ss)


# ------------------------------------------------------------------ family A
def run_family_a(gvamd, monkeypatch, grid, origin, tune):
    geo, scene = rc.family_a(grid, origin)
    og = rc.oracle_grid(geo)
    m_base = ol.tf_to_matrix4f(scene.tf)
    h = make_handle(gvamd, monkeypatch, geo, tune)
    z = np.zeros(1, np.float32)
    try:
        for f in range(len(scene.ends)):   # one frame per end, one handle
            x, y = scene.x[f:f + 1], scene.y[f:f + 1]
            want_miss = og.raymarch(m_base, x, y, z)[0].astype(np.int32)
            want_hits = og.bin_points(m_base, x, y, z)[0]
            run_frame(gvamd, h, geo, x, y, z, want_miss, want_hits, f"{scene.name} frame {f} end {scene.ends[f].tolist()}")
    finally:
        h.close()
    assert len(scene.ends) >= geo.nx * geo.ny + 2 * (geo.nx + geo.ny) - 4


@pytest.mark.parametrize("origin", ["centre", "corner", "edge", "near_corner"])
def test_single_end_every_cell(gvamd, monkeypatch, origin):
    """G64, the tile path: every cell a hit end, every border cell a clipped end, the origin cell's own clipped ends"""
    run_family_a(gvamd, monkeypatch, rc.G64, origin, {})


@pytest.mark.parametrize("origin", ["centre", "corner"])
def test_single_end_every_cell_generic_path(gvamd, monkeypatch, origin):
    """G62: nx % 4 != 0, the literal per-ray kernels"""
    run_family_a(gvamd, monkeypatch, rc.G62, origin, {})


def test_single_end_every_cell_simple_impl(gvamd, monkeypatch):
    run_family_a(gvamd, monkeypatch, rc.G64, "edge", {"GV_RAY_IMPL": "simple"})


# ------------------------------------------------------------------ family B
# (GV_LOG2S on G1024 only: 32 or 64 sectors cannot hold a wedge of 4990 columns -- the sector plan's width bit, asserted
# for exactly these pairs by tests/test_sector_plan_host.py::test_gpu_suite_knob_sets)
@pytest.mark.parametrize("name,tune", [(n, t) for n in SETS for t in TUNE_BD if not (t.startswith("log2s") and n == "g5100")])
def test_single_long_ends(gvamd, monkeypatch, cache, name, tune):
    """at most one end per octant and frame, on and beside every boundary a power-of-two sector count can have;
    g5100 runs k_ray_sectors<16> (a wedge of 4990 columns)"""
    ss = scene_set(cache, ("B", name), lambda: (*rc.family_b(*SETS[name])[:2], None), dense=False)
    assert run_scenes(gvamd, monkeypatch, ss, TUNE_BD[tune]) > 200


def test_wide_column_is_refused(gvamd, monkeypatch):
    """G5100 under GV_LOG2S=5: columns 156 cells wide.  The frame is refused on the host (GV_ERR_BAD_ARG, the message
    names the column width) before any kernel of the ray stage is launched, and the handle closes cleanly"""
    geo = rc.Geo(*SETS["g5100"])
    h = make_handle(gvamd, monkeypatch, geo, TUNE_BD["log2s5"])
    try:
        x, y = geo.hit_point(geo.origin[0] - 40, geo.origin[1] + 3)
        h.upload_xyz(np.array([x], np.float32), np.array([y], np.float32), np.zeros(1, np.float32))
        with pytest.raises(gvamd.GVError) as e:
            h.process_frame(gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH)
        assert e.value.code == 1 and gvamd.STATUS[1] == "GV_ERR_BAD_ARG"
        assert "column" in str(e.value) and "wider than 32 cells" in str(e.value)
        h.synchronize()
    finally:
        h.close()


@pytest.mark.parametrize("tune", list(TAILS_B))
def test_single_ends_beside_the_threshold_column(gvamd, monkeypatch, cache, tune):
    """single ends of every reach from 3 to 40 on G1024: a sector with one end has its threshold column T at the end's
    reach or at the first level boundary (16), so ends one, two and three columns past T occur; these columns are
    narrow (below 2 S) and taken beside the threshold computation, under every tail setting"""
    ss = scene_set(cache, ("B2",), lambda: (*rc.family_b_short()[:2], None), dense=False)
    assert run_scenes(gvamd, monkeypatch, ss, TAILS_B[tune]) == len(ss) > 30


# ------------------------------------------------------------------ family C
def c_set(cache, name, bases):
    def build():
        geo = rc.Geo(*SETS[name])
        keys = [(b, 0, None) for b in bases] + [k for k in rc.family_c_keys() if k[0] in bases]
        return geo, [rc.family_c_scene(geo, k) for k in keys], [None if not k[1] else bases.index(k[0]) for k in keys]
    return scene_set(cache, ("C", name, bases), build, dense=True)


@pytest.mark.parametrize("tune", list(TUNE_C))
@pytest.mark.parametrize("name", list(SETS))
def test_shadows(gvamd, monkeypatch, cache, name, tune):
    """rings and bands of long ends with gaps of 1 to 3 border cells in all eight octants: the cells only the removed
    rays crossed must stay unfree, whichever tail policy, group count and helper setting the sector takes"""
    groups = [("band",)] if tune == "cap2048" else [("ring", "clipped_ring"), ("band",)]
    n = sum(run_scenes(gvamd, monkeypatch, c_set(cache, name, bases), TUNE_C[tune]) for bases in groups)
    assert n == 64 * sum(len(b) for b in groups)   # per base: the gap-less scene and 3 widths x 21 positions


@pytest.mark.parametrize("base", ["ring", "band"])
@pytest.mark.parametrize("world", [2, 3])
def test_shadows_sharded_emulated(gvamd, monkeypatch, cache, world, base):
    """the ring and band scenes of G1024, origin (300, 700), through every rank of a sharded frame on one device: the
    miss getter does not exist there, so each frame starts from the prior and the layers are compared"""
    ss = c_set(cache, "g1024_off", ("ring", "clipped_ring") if base == "ring" else ("band",))
    pick = [i for i, n in enumerate(ss.names) if n.startswith(f"C-{base}-")]
    assert len(pick) == 64
    h = make_handle(gvamd, monkeypatch, ss.geo, {})
    try:
        for i in pick:
            h.reset()
            h.upload_xyz(*ss.cloud(i))
            h.frame_sharded_emulated(world, gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH)
            og = rc.oracle_grid(ss.geo)   # oracle_frame on a grid at the prior
            miss, hits = ss.want(i)
            og.frame_update(None, hits, miss.astype(np.uint8))
            assert check_grid(h, og)[0] == 0
    finally:
        h.close()


@pytest.mark.parametrize("tune", [t for t in TUNE_C if t != "cap2048"])
def test_threshold_column(gvamd, monkeypatch, cache, tune):
    """wall cells that are the longest ends of their slope-bucket group, with long ends up to the edges of their own
    slope interval: the first column past the sector's threshold column T, where the tail begins, holds an unfree
    interior cell"""
    ss = scene_set(cache, ("T",), lambda: (*rc.family_t()[:2], None), dense=True)
    assert run_scenes(gvamd, monkeypatch, ss, TUNE_C[tune]) == len(rc.T_COLUMNS)


# ------------------------------------------------------------------ family D
@pytest.mark.parametrize("tune", list(TUNE_BD))
def test_crowded_slopes_at_the_thresholds(gvamd, monkeypatch, cache, tune):
    """8, 9, 23, 24, 25 and 64 ends on one rational slope per octant (a full row of eight; 15, 16 and 17 overflow
    entries around the same-slope merge's minimum), the longest placed last or in the middle, two strangers beside"""
    ss = scene_set(cache, ("D",), lambda: (*rc.family_d()[:2], None), dense=False)
    assert run_scenes(gvamd, monkeypatch, ss, TUNE_BD[tune]) == 60


# ------------------------------------------------------------------ family E
def test_long_diagonal(gvamd, monkeypatch):
    """G4200, corner origin: ends with a and b beyond 4096 (k_ray_sectors<16>; the long-ray march's a/2 + i*b beyond
    2^24) over 3000 short ends near the origin.  The only test that allocates this grid."""
    geo, scene, long_ab = rc.family_e()
    og = rc.oracle_grid(geo)
    want_miss, want_hits = rc.oracle_miss(og, scene).astype(np.int32), rc.oracle_hits(og, scene)
    del og
    h = make_handle(gvamd, monkeypatch, geo, {})
    try:
        run_frame(gvamd, h, geo, scene.x, scene.y, scene.z, want_miss, want_hits, scene.name)
    finally:
        h.close()
