"""The tile grid pass leaves a tile row (64 cells) alone whose log-odds it did not change by a bit, while the handle
knows occupancy and the int8 grid to derive from the log-odds (gv_context::layers_in_step).  Every sequence below is
held to the oracle after EVERY step -- log-odds bit-equal, occupancy correctly rounded, int8 equal
(grid_pass_ref.check_layers) -- on tile-path grids whose sides are not multiples of 64, and then repeated in fresh
child processes with GV_GRID_SKIP=0 (every pass dense), GV_PIPELINE=0 and both: the three layers after every step must
be byte-identical to the skipping, pipelined run's.

A sequence is a generator: it drives the handle and yields (handle, tag, oracle_step) after every step;
oracle_step(og) makes the same step on the oracle grid (and returns LO_ONLY right after set_log_odds, where the other
two layers are stale).  The child process (python tests/test_gpu_grid_skip.py NAME) runs the same generator without the oracle and prints one digest per
step."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(_ROOT, "tests"), os.path.join(_ROOT, "grid-vision_amd")]

import grid_pass_ref as R
import oracle_lib as ol
from gvamd import synth

pytestmark = pytest.mark.gpu
F32 = np.float32
U32 = np.uint32
IDENT = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
GRID = (50, 20, 0.1)             # 500 x 200 cells: 7.8 x 3.1 tiles
LO_ONLY = "log-odds only"
TICK_CONFIG = 2                  # 1000 x 1000 cells: 15.6 tiles a side


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


# ------------------------------------------------------------------------------------------------ helpers --
def _handle(gv):
    h = gv.GridVisionHIP(*GRID)
    h.set_transforms(IDENT, IDENT, IDENT)
    return h, {"base_lidar": IDENT}


def _cloud(h, seed, n=30_000, spread=0.6):
    st = synth.Stream(4242, seed)
    lx, ly, px = GRID[0], GRID[1], h.pos_x
    return (st.uniform(n, px - spread * lx, px + spread * lx), st.uniform(n, -spread * ly, spread * ly),
            st.uniform(n, -1.0, 1.0))


def _poses(h, seed, n=12):
    st = synth.Stream(777, seed)
    lx, ly = GRID[0], GRID[1]
    p = np.zeros(n, synth.LSHAPE_DTYPE)
    p["px"] = st.uniform(n, h.pos_x - 0.4 * lx, h.pos_x + 0.4 * lx).astype(np.float64)
    p["py"] = st.uniform(n, -0.4 * ly, 0.4 * ly).astype(np.float64)
    p["qw"] = 1.0
    p["length"] = st.uniform(n, 0.3, 6.0).astype(np.float64)
    p["width"] = st.uniform(n, 0.3, 3.0).astype(np.float64)
    p["height"] = 1.5
    return p


def _frame(gv, h, tfs, cloud, poses, upload=True):
    """one frame through gv_frame_enqueue (the lanes unless GV_PIPELINE=0) and what the oracle does for it"""
    x, y, z = cloud
    if upload:
        h.upload_xyz(x, y, z)
    h.set_detections(gv.FRAME_BIN | gv.FRAME_RAYMARCH, poses=poses)
    h.enqueue_frame()
    h.synchronize()
    return _oracle_frame(tfs, cloud, poses)


def _oracle_frame(tfs, cloud, poses):
    def step(og):
        m_base = ol.tf_to_matrix4f(tfs["base_lidar"])
        hits, _ = og.bin_points(m_base, *cloud)
        miss, _ = og.raymarch(m_base, *cloud)
        og.frame_update(poses, hits, miss)
    return step


def _oracle_set(start):
    """set_log_odds replaces one layer: the other two are stale until the next pass, only the log-odds compare"""
    def step(og):
        og.log_odds[:] = start
        return LO_ONLY
    return step


def _tf(yaw, tx, ty):
    return np.array([0.0, 0.0, np.sin(0.5 * yaw), np.cos(0.5 * yaw), tx, ty, 0.0])


def _special_start(G, nx):
    """clamp values, NaNs, +-inf, -0.0 and reachable values cell by cell; whole rows at either clamp (a pass that
    compared log-odds alone would skip them and leave the occupancy of the frames before)"""
    bits = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000], U32).view(F32)
    sp = np.concatenate([bits, np.array([-2.0, 3.6, -2.0, 3.6, -1.8, 3.4, 0.65, -0.6], F32)])
    st = synth.Stream(99, 5)
    v = R.values(st.integers(G, 0, R.N_REACHABLE))
    v[::3] = np.resize(sp, len(v[::3]))
    v = v.reshape(-1, nx)
    v[10:60] = F32(-2.0)
    v[70:120] = F32(3.6)
    v[130:150, : nx // 2] = F32(-2.0)
    return v.reshape(-1).copy()


# ---------------------------------------------------------------------------------------------- sequences --
def seq_one_cloud(gv):
    """(a) 15 frames of one cloud and one set of poses: the cells saturate on the way"""
    h, tfs = _handle(gv)
    cloud, poses = _cloud(h, 1), _poses(h, 1)
    for f in range(15):
        step = _frame(gv, h, tfs, cloud, poses, upload=f == 0)
        yield h, f"frame {f}", step
    h.close()


def seq_alternating(gv):
    """(b) two clouds alternating, the poses change every frame"""
    h, tfs = _handle(gv)
    clouds = (_cloud(h, 2), _cloud(h, 3, spread=0.35))
    for f in range(10):
        step = _frame(gv, h, tfs, clouds[f & 1], _poses(h, 10 + f // 2))
        yield h, f"frame {f}", step
    h.close()


def seq_set_log_odds(gv):
    """(c) frames, then set_log_odds with clamp values, NaN, +-inf and -0.0 in it, then three frames; once more
    with every cell at a clamp"""
    h, tfs = _handle(gv)
    cloud, poses = _cloud(h, 4), _poses(h, 4)
    for f in range(4):
        step = _frame(gv, h, tfs, cloud, poses, upload=f == 0)
        yield h, f"warm {f}", step
    start = _special_start(h.G, h.nx)
    h.set_log_odds(start)
    yield h, "set_log_odds", _oracle_set(start)
    for f in range(3):
        yield h, f"after set {f}", _frame(gv, h, tfs, cloud, poses, upload=False)
    flat = np.where(np.arange(h.G) % 1000 < 500, F32(-2.0), F32(3.6)).astype(F32)
    h.set_log_odds(flat)
    yield h, "set_log_odds clamps", _oracle_set(flat)
    for f in range(3):
        yield h, f"after clamps {f}", _frame(gv, h, tfs, cloud, poses, upload=False)
    h.close()


def seq_interleaved(gv):
    """(d) reset, grid_move and update_map_poses (and update_map) between frames"""
    from test_gpu_grid_move import np_move
    h, tfs = _handle(gv)
    cloud, poses = _cloud(h, 5), _poses(h, 5)
    geom = (h.nx, h.ny, GRID[2], h.pos_x, h.pos_y)

    def move(yaw, tx, ty):
        info = h.grid_move(_tf(yaw, tx, ty))
        assert info["applied"]

        def step(og):
            lo, occ, _ = np_move((og.log_odds.copy(), og.occupancy.copy(), og.to_occupancy_grid()[0]), *geom, info)
            og.log_odds[:] = lo
            og.occupancy[:] = occ
        return step

    def reset():
        h.reset()

        def step(og):
            og.log_odds[:] = 0.0
            og.occupancy[:] = 0.5
        return step

    def map_poses(p):
        h.update_map_poses(p)
        return lambda og: og.update_map_poses(p)

    def plain():
        h.update_map()
        return lambda og: og.update_map()

    for f in range(6):
        yield h, f"frame {f}", _frame(gv, h, tfs, cloud, poses, upload=f == 0)
    yield h, "move 1", move(0.0, 1.3, -0.4)
    for f in range(2):
        yield h, f"frame after move {f}", _frame(gv, h, tfs, cloud, poses, upload=False)
    yield h, "update_map_poses", map_poses(_poses(h, 6))
    yield h, "update_map", plain()
    yield h, "move 2", move(0.04, -0.7, 0.9)
    yield h, "update_map_poses after move", map_poses(_poses(h, 6))
    yield h, "frame", _frame(gv, h, tfs, cloud, poses, upload=False)
    yield h, "reset", reset()
    for f in range(8):
        yield h, f"frame after reset {f}", _frame(gv, h, tfs, cloud, poses, upload=False)
    yield h, "move 3", move(0.0, 0.5, 0.0)
    for f in range(3):
        yield h, f"plain after move {f}", plain()
    h.close()


def seq_tick(gv):
    """(e) ticks with grid_out between frames: the PCA tick's plain update and the lidar tick's own grid pass; the
    tick's grid_out is the int8 grid right behind its pass"""
    from test_gpu_parity import make_handle
    tfs = synth.transforms(True)
    h, _ = make_handle(gv, TICK_CONFIG, perturbed=True)
    x, y, z, b = synth.scene_with_objects(tfs, n_total=200_000, n_obj=10, per=2000)
    cloud = (x, y, z)
    pin = gv.PinnedI8(h.G)
    try:
        h.upload_xyz(x, y, z)
        for f in range(5):
            yield h, f"frame {f}", _frame(gv, h, tfs, cloud, None, upload=False)
        for t, lidar in enumerate((False, True, True, False, True)):
            r = h.tick(b, k_near=4, lidar_bin=lidar, lidar_raymarch=lidar, grid_out=pin.array)
            assert np.array_equal(pin.array, h.to_occupancy_grid()[0]), f"tick {t}: grid_out"
            p = r["poses"].copy()
            step = _oracle_frame(tfs, cloud, p) if lidar else (lambda og, p=p: og.update_map_poses(p))
            yield h, f"tick {t} lidar={lidar}", step
            yield h, f"frame after tick {t}", _frame(gv, h, tfs, cloud, None, upload=False)
    finally:
        pin.close()
    h.close()


def seq_burst(gv):
    """(g) frames in flight on the lanes with no host wait between them: one step after 5, one after 17"""
    h, tfs = _handle(gv)
    cloud, poses = _cloud(h, 7), _poses(h, 7)
    h.upload_xyz(*cloud)
    h.set_detections(gv.FRAME_BIN | gv.FRAME_RAYMARCH, poses=poses)
    inner = _oracle_frame(tfs, cloud, poses)
    for n in (5, 17):
        for _ in range(n):
            h.enqueue_frame()
        h.synchronize()

        def step(og, n=n):
            for _ in range(n):
                inner(og)
        yield h, f"{n} frames", step
    h.close()


SEQUENCES = {"one_cloud": seq_one_cloud, "alternating": seq_alternating, "set_log_odds": seq_set_log_odds,
             "interleaved": seq_interleaved, "tick": seq_tick, "burst": seq_burst}


def _layers(h):
    return h.log_odds(), h.occupancy(), h.to_occupancy_grid()[0]


def _digest(layers):
    d = hashlib.sha1()
    for a in layers:
        d.update(np.ascontiguousarray(a).tobytes())
    return d.hexdigest()


# ------------------------------------------------------------------------------ against the oracle, in process --
_RUNS = {}


def _checked_run(gv, name):
    """the sequence in this process (skipping, pipelined), every step held to the oracle; the digests per step and
    the share of tile rows of 64 cells whose log-odds a step left as they were"""
    if name in _RUNS:
        return _RUNS[name]
    assert os.environ.get("GV_GRID_SKIP", "1") != "0" and os.environ.get("GV_PIPELINE", "1") != "0"
    if name == "tick":
        g = synth.CONFIGS[TICK_CONFIG]["grid"]
        og = ol.OGrid(g.grid_x, g.grid_y, g.resolution)
    else:
        og = ol.OGrid(*GRID)
    digests, still = [], []
    prev = None
    for h, tag, step in SEQUENCES[name](gv):
        lo, occ, i8 = _layers(h)
        if step(og) == LO_ONLY:
            assert np.array_equal(lo.view(U32), og.log_odds.view(U32)), f"{name} {tag}"
        else:
            R.check_layers(lo, occ, i8, og.log_odds, og.occupancy, og.to_occupancy_grid()[0], None, f"{name} {tag}")
        if prev is not None and h.nx % 4 == 0:
            same = (prev.view(U32) == lo.view(U32)).reshape(h.ny, h.nx)
            pad = (-h.nx) % 64
            rows = np.pad(same, ((0, 0), (0, pad)), constant_values=True).reshape(h.ny, -1, 64).all(axis=2)
            still.append(float(rows.mean()))
        prev = lo
        digests.append(_digest((lo, occ, i8)))
    _RUNS[name] = (digests, still)
    return _RUNS[name]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name", list(SEQUENCES))
def test_every_step_against_the_oracle(gvamd, name):
    digests, still = _checked_run(gvamd, name)
    assert len(digests) >= 2
    print(f"\n{name}: {len(digests)} steps, share of unchanged tile rows per step: "
          + " ".join(f"{s:.2f}" for s in still))
    if name == "one_cloud":
        # the sequence does reach the state the skip is for, and starts from one where nothing can be skipped
        assert still[0] < 0.05 and still[-1] > 0.5, still


# -------------------------------------------------------------------------- the same in fresh child processes --
def _child_run(name, env_extra):
    env = dict(os.environ)
    env.pop("GV_GRID_SKIP", None)
    env.pop("GV_PIPELINE", None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, f"child {name} {env_extra}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    line = [l for l in r.stdout.splitlines() if l.startswith("DIGESTS ")][-1]
    return json.loads(line[len("DIGESTS "):])


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("env", [{"GV_GRID_SKIP": "0"}, {"GV_PIPELINE": "0"}, {"GV_GRID_SKIP": "0", "GV_PIPELINE": "0"}],
                         ids=["dense", "serial", "dense_serial"])
@pytest.mark.parametrize("name", list(SEQUENCES))
def test_layers_byte_identical_in_a_fresh_process(gvamd, name, env):
    want, _ = _checked_run(gvamd, name)
    got = _child_run(name, env)
    assert len(got) == len(want)
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, f"{name} {env}: layers differ from the skipping pipelined run after steps {bad[:8]}"


def _child_main(name):
    import gvamd as gv
    gv.load(build_if_missing=False)
    out = [_digest(_layers(h)) for h, _, _ in SEQUENCES[name](gv)]
    print("DIGESTS " + json.dumps(out), flush=True)


if __name__ == "__main__":
    _child_main(sys.argv[1])
