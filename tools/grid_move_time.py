"""Device time of gv_grid_move ([EXTENSION] X3): HIP events on the handle's stream around N back-to-back moves, each
one applied (a whole-cell shift plus a yaw above the half-cell threshold), on the 2000 x 2000 and the reference's
500 x 200 grid filled with non-trivial layers.  Prints one line per grid; --out FILE writes them there too.

Per-move time = event interval / N.  The moves are enqueued from Python: where a move's device time is below the
host's enqueue cost (the small grid), the interval is bound by the host and is an upper bound -- take the kernel times
of a `rocprofv3 --kernel-trace --stats` run of this script for the device side there."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "grid-vision_amd"))

import gvamd  # noqa: E402
from gvamd import synth  # noqa: E402

hip = C.CDLL("libamdhip64.so")


def _poses(h, res, n, seed):
    rng = np.random.default_rng(seed)
    lx, ly = h.nx * res, h.ny * res
    p = np.zeros(n, dtype=synth.LSHAPE_DTYPE)
    p["px"] = rng.uniform(h.pos_x - 0.5 * lx, h.pos_x + 0.5 * lx, n)
    p["py"] = rng.uniform(h.pos_y - 0.5 * ly, h.pos_y + 0.5 * ly, n)
    p["qw"] = 1.0
    p["length"] = rng.uniform(0.5, 0.1 * lx, n)
    p["width"] = rng.uniform(0.5, 0.1 * ly, n)
    p["height"] = 1.5
    return p


def _tf(yaw, tx, ty):
    return [0.0, 0.0, np.sin(0.5 * yaw), np.cos(0.5 * yaw), tx, ty, 0.0]


def time_grid(gx, gy, res, n, warmup):
    h = gvamd.GridVisionHIP(gx, gy, res)
    for t in range(8):
        h.update_map_poses(_poses(h, res, 40, t))
    # back and forth: one cell in x and 0.5 degrees, then back; every call resamples
    fwd, back = _tf(np.radians(0.5), res, 0.0), _tf(np.radians(-0.5), -res, 0.0)
    for i in range(warmup):
        h.grid_move(fwd if i % 2 == 0 else back)
    h.synchronize()
    s = C.c_void_p(h.stream())
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    applied = 0
    assert hip.hipEventRecord(e0, s) == 0
    for i in range(n):
        applied += h.grid_move(fwd if i % 2 == 0 else back)["applied"]
    assert hip.hipEventRecord(e1, s) == 0
    assert hip.hipEventSynchronize(e1) == 0
    ms = C.c_float()
    assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    nx, ny, G = h.nx, h.ny, h.G
    h.close()
    us = 1000.0 * ms.value / n
    moved = 4 * 9 * G   # bytes: gather (9 G read, 9 G written) + copy back (the same again)
    return (f"grid {gx} x {gy} m at {res} m: {nx} x {ny} cells, {n} moves ({applied} applied): {us:.2f} us per move, "
            f"{moved / 1e6:.1f} MB moved per move, {moved / (us * 1e-6) / 1e9:.0f} GB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--moves", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [time_grid(200, 200, 0.1, a.moves, a.warmup), time_grid(50, 20, 0.1, a.moves, a.warmup)]
    for ln in lines:
        print(ln, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
