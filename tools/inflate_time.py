"""Device time of gv_inflate ([EXTENSION] X6): HIP events on the handle's stream around N back-to-back passes on the
2000 x 2000 and the 500 x 200 grid after the 12-tick fill of tests/test_gpu_grid_move.py, with the parameter sets P1 and
P2 (0.1 m cells) and P3 (Rc = 63, on grids of its own 0.05 m resolution), plus P1 with the dist2 layer kept.
One line per case: per call in us, bytes moved (G read + G/8 bitmap + G written, + 2 G with dist2), the rate that gives,
and the share of tiles whose window holds no lethal cell (computed here from the grid's readback).

Per-call time = event interval / N.  The passes are enqueued from Python: where a pass is shorter than the host's
enqueue cost (the small grid) the interval is an upper bound -- the kernel times are the device side.  For those run
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/inflate_time.py
and then `python tools/inflate_time.py --trace DIR`, which reads the trace (no GPU) and prints, per case in the same
order, the mean duration of each kernel over the timed passes.  --out FILE appends what is printed."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "grid-vision_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import planner_time_common as common  # noqa: E402

# (label, (grid_x, grid_y, res), (inscribed, inflation, scaling), keep_dist2)
P1, P2, P3 = (0.35, 0.55, 10.0), (0.52, 3.03, 3.0), (0.31, 3.17, 1.5)
CASES = [
    ("2000x2000 P1", (200, 200, 0.1), P1, False),
    ("2000x2000 P1 +dist2", (200, 200, 0.1), P1, True),
    ("2000x2000 P2", (200, 200, 0.1), P2, False),
    ("2000x2000 P3", (100, 100, 0.05), P3, False),
    ("500x200 P1", (50, 20, 0.1), P1, False),
    ("500x200 P2", (50, 20, 0.1), P2, False),
    ("500x200 P3", (25, 10, 0.05), P3, False),
]
THRESHOLD = 65
KERNELS = ("k_lethal_bits", "k_inflate_tiles")


def empty_share(lethal, rc):
    """share of the 64 x 64 tiles whose window (the tile grown by rc cells) holds no lethal cell"""
    ny, nx = lethal.shape
    s = np.zeros((ny + 1, nx + 1), np.int64)
    s[1:, 1:] = np.cumsum(np.cumsum(lethal, axis=0), axis=1)
    empty = total = 0
    for y0 in range(0, ny, 64):
        for x0 in range(0, nx, 64):
            ya, yb = max(y0 - rc, 0), min(y0 + 64 + rc, ny)
            xa, xb = max(x0 - rc, 0), min(x0 + 64 + rc, nx)
            empty += (s[yb, xb] - s[ya, xb] - s[yb, xa] + s[ya, xa]) == 0
            total += 1
    return empty / total


def time_case(label, grid, pset, keep, n, warmup):
    import gvamd
    from gvamd import synth
    hip = common.load_hip()
    gx, gy, res = grid
    h = gvamd.GridVisionHIP(gx, gy, res)
    for t in range(12):
        h.update_map_poses(common.fill_poses(synth, h, res, 40, 100 + t))
    cfg = gvamd.Inflation(pset[0], pset[1], pset[2], THRESHOLD, gvamd.INFLATE_KEEP_DIST2 if keep else 0)
    table = gvamd.inflation_cost_table(cfg, res)
    rc = int(np.sqrt(len(table) - 1))
    lethal = h.to_occupancy_grid()[0].reshape(h.ny, h.nx) >= THRESHOLD
    h.set_inflation(cfg)
    for _ in range(warmup):
        h.inflate()
    h.synchronize()
    us = common.event_us_per_call(hip, h, n, h.inflate)
    cost = h.costmap()
    G = h.G
    h.close()
    moved = G + G // 8 + G + (2 * G if keep else 0)
    return (f"{label:20s} {h.nx} x {h.ny} cells at {res} m, Rc {rc:2d}, d2max {len(table) - 1:4d}, lethal {lethal.mean() * 100:5.2f} %, "
            f"cost > 0 {np.count_nonzero(cost) / G * 100:5.2f} %, empty tiles {empty_share(lethal, rc) * 100:5.1f} %: "
            f"{n} passes, {us:7.2f} us per call, {moved / 1e6:6.2f} MB moved, {moved / (us * 1e-6) / 1e9:6.0f} GB/s")


def kernel_times(trace_dir, n, warmup):
    """per case and kernel: mean duration in us of the timed dispatches, from rocprofv3's kernel trace of one run of
    this script (dispatch order = CASES order, warmup + n passes of two kernels each)"""
    per = common.kernel_durations(trace_dir, KERNELS)
    lines = []
    for i, (label, _, _, _) in enumerate(CASES):
        parts = []
        for k in KERNELS:
            d = per[k][i * (warmup + n) + warmup:(i + 1) * (warmup + n)]
            assert len(d) == n, (k, label, len(d), len(per[k]))
            parts.append(f"{k} {np.mean(d):7.2f} us (min {np.min(d):7.2f})")
        lines.append(f"{label:20s} " + ", ".join(parts))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace run of this script: print kernel times")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace:
        lines = ["per kernel (rocprofv3 --kernel-trace of the same script):"] + kernel_times(a.trace, a.passes, a.warmup)
    else:
        lines = ["per call (HIP events around %d back-to-back gv_inflate):" % a.passes]
        for c in CASES:
            lines.append(time_case(*c, a.passes, a.warmup))
            print(lines[-1], flush=True)
    if a.trace:
        print("\n".join(lines), flush=True)
    if a.out:
        common.append_out(a.out, lines)


if __name__ == "__main__":
    main()
