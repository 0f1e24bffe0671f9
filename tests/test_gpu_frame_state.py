"""Which of hits() / miss() / cell_idx() / bbox_id() is valid after which call, and that a valid getter reads the
buffers of the call that made it valid.

Every frame form ends by recording what it left behind (gv_context::LastFrame): the buffer set, the stream whose count
grid and per-point outputs it wrote, and which of the four outputs exist.  The forms differ on purpose -- the generic
frame keeps its counts only with KEEP_COUNTS, the sharded frame's emulation has no whole count grid and no whole miss
grid, the sharded frame itself keeps its band's count totals only with KEEP_COUNTS and never a miss grid, the tick
writes no per-point output and leaves those of the call before it alone -- and the standalone calls change single flags.  The tables below pin that step by step on one handle, so that every step starts from the
history of the steps before it; a getter that is not valid raises GV_ERR_STATE (5), ray_stats() never raises.  The
values behind a valid getter are held to a fresh handle that ran only the step in question: after a history of other
calls the last frame ran on another lane and another buffer set than the fresh handle's."""
import numpy as np
import pytest

from gvamd import synth

pytestmark = pytest.mark.gpu
TILE_GRID = (50, 20, 0.1)      # 500 x 200 cells: the tile path
GENERIC_GRID = (50, 20, 0.3)   # 167 x 67 cells, nx % 4 != 0: the generic path
GETTERS = ("hits", "miss", "cell_idx", "bbox_id")
ALL = set(GETTERS)
N_POINTS = 4000


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    monkeypatch.delenv("GV_PIPELINE", raising=False)
    monkeypatch.delenv("GV_RAY_IMPL", raising=False)


def _inputs(grid):
    """about 4000 points inside the map, in front of the camera, and four boxes"""
    st = synth.Stream(2718, 1)
    px = float(grid[0] // 3)
    x = st.uniform(N_POINTS, px - 0.45 * grid[0], px + 0.45 * grid[0])
    y = st.uniform(N_POINTS, -0.45 * grid[1], 0.45 * grid[1])
    z = st.uniform(N_POINTS, -1.0, 1.0)
    return (x, y, z), synth.detections(3, 4)


def _handle(gv, grid, cloud):
    tfs = synth.transforms(False)
    h = gv.GridVisionHIP(*grid)
    assert (h.nx % 4 == 0) == (grid == TILE_GRID)
    h.set_transforms(tfs["cam_lidar"], tfs["base_cam"], tfs["base_lidar"])
    h.upload_xyz(*cloud)
    return h


def _available(gv, h):
    got = set()
    for name in GETTERS:
        try:
            getattr(h, name)()
            got.add(name)
        except gv.GVError as e:
            assert e.code == 5, f"{name}() failed with {e}"
    h.ray_stats()
    return got


def _expect(gv, h, want, step):
    got = _available(gv, h)
    assert got == set(want), f"after {step}: available {sorted(got)}, expected {sorted(want)}"


def _arrays(h, names=GETTERS):
    return {n: getattr(h, n)() for n in names}


def _same(a, b, what):
    for n in b:
        assert np.array_equal(a[n], b[n]), f"{what}: {n}() differs from the fresh handle's"


_FRESH = {}


def _fresh(gv, key):
    """what a fresh handle holds that ran only the step `key`; computed once, never changed"""
    if key in _FRESH:
        return _FRESH[key]
    grid = GENERIC_GRID if key == "generic_all" else TILE_GRID
    cloud, boxes = _inputs(grid)
    rm = gv.FRAME_BIN | gv.FRAME_RAYMARCH
    with _handle(gv, grid, cloud) as h:
        if key == "tile_all":
            h.process_frame(rm | gv.FRAME_KEEP_CELL_IDX | gv.FRAME_BBOX_TEST, bboxes=boxes)
            out = _arrays(h)
        elif key == "generic_all":
            h.process_frame(rm | gv.FRAME_KEEP_COUNTS | gv.FRAME_KEEP_CELL_IDX | gv.FRAME_BBOX_TEST, bboxes=boxes)
            out = _arrays(h)
        else:
            assert key == "tile_three"
            h.set_detections(rm)
            for _ in range(3):
                h.enqueue_frame()
            h.synchronize()
            out = _arrays(h, ("hits", "miss"))
    assert out["hits"].sum() > N_POINTS // 2 and out["miss"].any(), "the inputs exercise nothing"
    if "bbox_id" in out:
        assert (out["bbox_id"] >= 0).any() and (out["cell_idx"] >= 0).any(), "the inputs exercise nothing"
    for a in out.values():
        a.setflags(write=False)
    _FRESH[key] = out
    return out


def _first_rows(gv, h, boxes):
    """the first three rows of the tile-path table"""
    rm = gv.FRAME_BIN | gv.FRAME_RAYMARCH
    _expect(gv, h, (), "create, transforms, upload")
    h.process_frame(rm)
    _expect(gv, h, ("hits", "miss"), "process_frame(BIN|RAYMARCH)")
    h.process_frame(rm | gv.FRAME_KEEP_CELL_IDX | gv.FRAME_BBOX_TEST, bboxes=boxes)
    _expect(gv, h, ALL, "process_frame(BIN|RAYMARCH|KEEP_CELL_IDX|BBOX_TEST)")


def test_tile_path_step_by_step(gvamd):
    gv = gvamd
    cloud, boxes = _inputs(TILE_GRID)
    rm = gv.FRAME_BIN | gv.FRAME_RAYMARCH
    with _handle(gv, TILE_GRID, cloud) as h:
        _first_rows(gv, h, boxes)
        _same(_arrays(h), _fresh(gv, "tile_all"), "all four after a frame before it")
        h.upload_xyz(*cloud)
        _expect(gv, h, ("hits", "miss"), "upload_xyz")
        h.extract_cloud_per_bbox(boxes)
        _expect(gv, h, ("hits", "miss", "bbox_id"), "extract_cloud_per_bbox")
        h.process_frame(gv.FRAME_BBOX_TEST, bboxes=boxes)
        _expect(gv, h, ("bbox_id",), "process_frame(BBOX_TEST)")
        h.tick(None, lidar_bin=True, lidar_raymarch=True)
        _expect(gv, h, ("hits", "miss", "bbox_id"), "tick(lidar_bin, lidar_raymarch)")
        h.frame_sharded_emulated(2, rm | gv.FRAME_KEEP_CELL_IDX | gv.FRAME_BBOX_TEST, bboxes=boxes)
        _expect(gv, h, ("cell_idx", "bbox_id"), "frame_sharded_emulated(2)")
        # the record after this whole history: the all-four frame and the pipelined frames once more
        h.process_frame(rm | gv.FRAME_KEEP_CELL_IDX | gv.FRAME_BBOX_TEST, bboxes=boxes)
        _expect(gv, h, ALL, "the all-four frame at the end")
        _same(_arrays(h), _fresh(gv, "tile_all"), "all four after the whole table")


def test_three_pipelined_frames(gvamd):
    gv = gvamd
    cloud, boxes = _inputs(TILE_GRID)
    rm = gv.FRAME_BIN | gv.FRAME_RAYMARCH
    with _handle(gv, TILE_GRID, cloud) as h:
        # a history that leaves the lanes and buffer sets somewhere else than a fresh handle's
        h.process_frame(rm | gv.FRAME_KEEP_CELL_IDX | gv.FRAME_BBOX_TEST, bboxes=boxes)
        h.extract_cloud_per_bbox(boxes)
        h.tick(None, lidar_bin=True, lidar_raymarch=True)
        h.process_frame(gv.FRAME_BBOX_TEST, bboxes=boxes)
        h.set_detections(rm)
        for _ in range(3):
            h.enqueue_frame()
        h.synchronize()
        _expect(gv, h, ("hits", "miss"), "three enqueue_frame(BIN|RAYMARCH) + synchronize")
        _same(_arrays(h, ("hits", "miss")), _fresh(gv, "tile_three"), "three pipelined frames after a history")


def test_sharded_frame_one_rank_step_by_step(gvamd):
    """The product's sharded frame on a real one-rank communicator: its tile pass writes hits[] only with KEEP_COUNTS
    (one band, a one-rank reduce: the totals are the plain frame's), its free-cell bitmaps are a band's, so miss() is
    never valid after it; the per-point outputs are the plain frame's.  Leaving the communicator gives the plain frame
    back."""
    gv = gvamd
    cloud, boxes = _inputs(TILE_GRID)
    rm = gv.FRAME_BIN | gv.FRAME_RAYMARCH
    fresh = _fresh(gv, "tile_all")
    with _handle(gv, TILE_GRID, cloud) as h:
        h.comm_init(gv.GridVisionHIP.comm_unique_id(), 0, 1)
        h.process_frame_sharded(rm)
        _expect(gv, h, (), "process_frame_sharded(BIN|RAYMARCH)")
        h.process_frame_sharded(rm | gv.FRAME_KEEP_COUNTS)
        _expect(gv, h, ("hits",), "process_frame_sharded(BIN|RAYMARCH|KEEP_COUNTS)")
        _same(_arrays(h, ("hits",)), {"hits": fresh["hits"]}, "sharded KEEP_COUNTS frame")
        h.process_frame_sharded(rm | gv.FRAME_KEEP_COUNTS | gv.FRAME_KEEP_CELL_IDX | gv.FRAME_BBOX_TEST, bboxes=boxes)
        names = ("hits", "cell_idx", "bbox_id")
        _expect(gv, h, names, "process_frame_sharded(BIN|RAYMARCH|KEEP_COUNTS|KEEP_CELL_IDX|BBOX_TEST)")
        _same(_arrays(h, names), {n: fresh[n] for n in names}, "sharded frame that keeps everything it can")
        h.comm_destroy()
        h.process_frame(rm | gv.FRAME_KEEP_CELL_IDX | gv.FRAME_BBOX_TEST, bboxes=boxes)
        _expect(gv, h, ALL, "comm_destroy, then the all-four frame")
        _same(_arrays(h), fresh, "all four after the communicator is gone")


def test_serial_tile_path(gvamd, monkeypatch):
    gv = gvamd
    cloud, boxes = _inputs(TILE_GRID)
    monkeypatch.setenv("GV_PIPELINE", "0")   # read by gv_create
    with _handle(gv, TILE_GRID, cloud) as h:
        _first_rows(gv, h, boxes)
        _same(_arrays(h), _fresh(gv, "tile_all"), "all four, serial frames")


def test_generic_path_step_by_step(gvamd):
    gv = gvamd
    cloud, boxes = _inputs(GENERIC_GRID)
    rm = gv.FRAME_BIN | gv.FRAME_RAYMARCH
    with _handle(gv, GENERIC_GRID, cloud) as h:
        _expect(gv, h, (), "create, transforms, upload")
        h.process_frame(rm)
        _expect(gv, h, (), "process_frame(BIN|RAYMARCH)")
        h.process_frame(rm | gv.FRAME_KEEP_COUNTS)
        _expect(gv, h, ("hits", "miss"), "process_frame(BIN|RAYMARCH|KEEP_COUNTS)")
        h.process_frame(rm | gv.FRAME_KEEP_COUNTS | gv.FRAME_KEEP_CELL_IDX | gv.FRAME_BBOX_TEST, bboxes=boxes)
        _expect(gv, h, ALL, "process_frame(BIN|RAYMARCH|KEEP_COUNTS|KEEP_CELL_IDX|BBOX_TEST)")
        _same(_arrays(h), _fresh(gv, "generic_all"), "all four after two frames before it")
        h.process_frame(rm)
        _expect(gv, h, (), "process_frame(BIN|RAYMARCH) again")
