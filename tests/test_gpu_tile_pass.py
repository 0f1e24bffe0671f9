"""The tile pass (k_bin_tiles, gv_binning.hip) segment by segment and its end bitmaps bit by bit: the scenes of
tests/tile_cases.py -- which tests/test_tile_cases_host.py proves to reach every gather branch, share count, round and
role-scan range they claim, and to see the mutants they exist for -- run through k_bin_partition and k_bin_tiles.
hits() and cell_idx() are compared element for element with the oracle, miss() wherever the frame marches (families A,
B, C), and the four end bitmaps, read back raw through the test hook gv_test_end_bitmaps and decoded here, bit for bit,
padding included, in every frame; the N and the T decoding of one frame must agree.  No tolerances.  A failure names
the tile, the chunk and the (r, L) of the first segment that feeds the first differing cell."""
import numpy as np
import pytest

import ray_cases as rc
import tile_cases as tc
from gvamd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


def make_handle(gvamd, monkeypatch, scene):
    for k in rc.KNOBS:
        monkeypatch.delenv(k, raising=False)
    geo = rc.Geo(scene.grid, scene.origin)
    h = gvamd.GridVisionHIP(*scene.grid)
    assert (h.nx, h.ny) == (geo.nx, geo.ny)
    tfs = synth.transforms(False)
    h.set_transforms(tfs["cam_lidar"], tfs["base_cam"], scene.tf)
    h.set_height_band(*tc.BAND)
    return h


def _first_cell(lay, got, want):
    """where two per-cell arrays first differ, and the segments that feed that cell"""
    i = int(np.flatnonzero(np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1))[0])
    ix, iy = i % lay.geo.nx, i // lay.geo.nx
    return f"got {np.asarray(got).reshape(-1)[i]} want {np.asarray(want).reshape(-1)[i]} at {lay.describe(ix, iy)}"


def _first_bit(lay, got, want):
    ys, xs = np.nonzero(got != want)
    iy, ix = int(ys[0]), int(xs[0])
    where = lay.describe(ix, iy) if ix < lay.geo.nx and iy < lay.geo.ny else f"padding bit ({ix}, {iy})"
    return f"{len(ys)} bits differ, first: got {int(got[iy, ix])} want {int(want[iy, ix])} at {where}"


def run_frame(gvamd, h, key):
    """one synchronous frame of reference(key) on handle h, every output against the oracle's"""
    scene, exp, lay = tc.reference(key)
    tag = scene.name
    h.upload_xyz(scene.x, scene.y, scene.z)
    flags = gvamd.FRAME_BIN | gvamd.FRAME_KEEP_COUNTS | gvamd.FRAME_KEEP_CELL_IDX | (gvamd.FRAME_RAYMARCH if scene.ray else 0)
    h.process_frame(flags)
    hits = h.hits()
    nz, want_nz = np.flatnonzero(hits), np.flatnonzero(exp.hits)      # (a 16 M cell grid is compared through its non-zeros)
    if not (np.array_equal(nz, want_nz) and np.array_equal(hits[nz], exp.hits[nz])):
        pytest.fail(f"{tag}: hits differ in {int((hits != exp.hits).sum())} cells, first: {_first_cell(lay, hits, exp.hits)}")
    cell = h.cell_idx()
    if not np.array_equal(cell, exp.cell):
        i = int(np.flatnonzero(cell != exp.cell)[0])
        pytest.fail(f"{tag}: cell_idx differs at point {i} (chunk {i // lay.chunk}): got {cell[i]} want {exp.cell[i]}")
    if scene.march:
        miss = h.miss()
        if not np.array_equal(miss, exp.miss):
            pytest.fail(f"{tag}: miss differs in {int((miss != exp.miss).sum())} cells, first: {_first_cell(lay, miss, exp.miss)}")
    hn, cn, ht, ct, (nxw, nyw, nx_pad, ny_pad) = h.test_end_bitmaps()
    assert (nx_pad, ny_pad) == exp.hit_bm.shape[::-1] and (nxw, nyw) == (nx_pad // 32, ny_pad // 32)
    assert len(hn) == len(cn) == nxw * ny_pad and len(ht) == len(ct) == nyw * nx_pad
    maps = {"hitN": tc.decode_n(hn, nxw, ny_pad), "clipN": tc.decode_n(cn, nxw, ny_pad),
            "hitT": tc.decode_t(ht, nyw, nx_pad), "clipT": tc.decode_t(ct, nyw, nx_pad)}
    for name, got in maps.items():
        want = exp.hit_bm if name.startswith("hit") else exp.clip_bm
        if not np.array_equal(got, want):
            pytest.fail(f"{tag}: {name} {_first_bit(lay, got, want)}")
    assert np.array_equal(maps["hitN"], maps["hitT"]) and np.array_equal(maps["clipN"], maps["clipT"])


def run_frames(gvamd, monkeypatch, keys):
    h = make_handle(gvamd, monkeypatch, tc.scene_of(keys[0]))
    try:
        for key in keys:
            run_frame(gvamd, h, key)
    finally:
        h.close()


def test_hook_needs_a_binned_frame_on_the_tile_path(gvamd, monkeypatch):
    """GV_ERR_STATE before the first binned frame and on a handle off the tile path (nx % 4 != 0); sizes without arrays"""
    import ctypes as C
    scene = tc.scene_of(("Csparse",))
    h = make_handle(gvamd, monkeypatch, scene)
    try:
        with pytest.raises(gvamd.GVError):
            h.test_end_bitmaps()
        run_frame(gvamd, h, ("Csparse",))
        g = [C.c_int32() for _ in range(4)]
        assert h._lib.gv_test_end_bitmaps(h._h, None, None, None, None, *[C.byref(v) for v in g]) == 0
        assert [v.value for v in g] == [12, 12, 384, 384]
        one = np.zeros(12 * 384, np.uint32)
        assert h._lib.gv_test_end_bitmaps(h._h, one.ctypes.data_as(C.c_void_p), None, None, None, *[C.byref(v) for v in g]) == 1
    finally:
        h.close()
    h = gvamd.GridVisionHIP(*rc.G62)
    try:
        tfs = synth.transforms(False)
        h.set_transforms(tfs["cam_lidar"], tfs["base_cam"], rc.Geo(rc.G62, (30, 30)).tf)
        h.upload_xyz(np.zeros(4, np.float32), np.zeros(4, np.float32), np.zeros(4, np.float32))
        h.process_frame(gvamd.FRAME_BIN | gvamd.FRAME_KEEP_COUNTS)
        with pytest.raises(gvamd.GVError):
            h.test_end_bitmaps()
    finally:
        h.close()


@pytest.mark.parametrize("sel", tc.A_KINDS)
def test_family_a_segments(gvamd, monkeypatch, sel):
    """every residue r with r + L at 32 | 33 and 128 | 129 and the lengths around them, hits only, clipped ends only, mixed"""
    run_frames(gvamd, monkeypatch, [("A", sel)])


@pytest.mark.parametrize("sel", ("hit", "ground"))
def test_family_b_bitmap_geometry(gvamd, monkeypatch, sel):
    """one end per word-edge cell of every tile, clipped ends on all four borders and corners; then a sparse frame on the
    same handle, whose bitmaps equal the reference of that frame alone"""
    run_frames(gvamd, monkeypatch, [("B", sel, 0), ("B", sel, 1)])


@pytest.mark.parametrize("name", list(tc.C_SPECS))
def test_family_c_shares(gvamd, monkeypatch, name):
    """tile totals at the steps of bin_splits, helpers with and without a share, several shared tiles with different k"""
    run_frames(gvamd, monkeypatch, [("C", name)])


def test_family_c_consecutive_frames_then_sparse(gvamd, monkeypatch):
    """three crowded frames and a sparse one on one handle: tickets, totals and slabs are reused, nothing survives"""
    run_frames(gvamd, monkeypatch, [("C", name) for name in tc.C_SEQUENCE] + [("Csparse",)])


@pytest.mark.parametrize("n", tc.D_SIZES)
def test_family_d_rounds_and_chunk_size(gvamd, monkeypatch, n):
    """more than 1024 chunks: listed segments in round 0 and again in round 1; the last cloud at chunk 2048, the first at 4096"""
    run_frames(gvamd, monkeypatch, [("D", n)])


def test_family_e_more_than_1024_tiles(gvamd, monkeypatch):
    """1037 tiles, bin only: two lanes' worth of tiles per thread in the role scan, crowded tiles in both ranges"""
    run_frames(gvamd, monkeypatch, [("E",)])
