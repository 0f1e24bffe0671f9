"""Time of matching the resident scan to the resident costmap ([EXTENSION] X16) on the 2000 x 2000 grid at 0.1 m:
the 1 M-point scene_with_objects cloud (the tick legs' workload), the map made of that scan itself (three lidar frames),
inflated with P1, the inflation of the other planner tools.  Two shapes: stride 32 with a 21 x 21 x 21 window and
stride 8 with a 41 x 41 x 41 window (yaw step 0.005 rad), the guess a few cells and steps off the truth.

Per shape, by the protocol of tools/traj_score_time.py:
  device    HIP events on the handle's stream around N back-to-back gv_match_scan_async calls into a pinned record,
            interval / N: the memset, the point pass, the score pass and the selection;
  host      wall clock of a waited gv_match_scan (median of N): what a caller that needs the pose observes;
  twin      gv_match_scan_host on one core (wall clock, one call), whose record must equal the device's or the script
            says so;
  reads     n_used * NT * NY * NX cost reads (the bound: candidates off the map read nothing) over the device time.

Kernel times come from a separate run:
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/match_time.py
and then `python tools/match_time.py --trace DIR` (no GPU).  --out FILE appends what is printed."""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "grid-vision_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import planner_time_common as common  # noqa: E402

GRID = (200, 200, 0.1)
P1 = (0.35, 0.55, 10.0, 65)
SHAPES = [(32, 10), (8, 20)]          # (stride, window half-width in cells and yaw steps)
YAW_STEP = 0.005
GUESS = (0.3, -0.2, 0.015)            # three cells, two cells, three yaw steps off
KERNELS = ["k_match_points", "k_match_score", "k_match_select"]


def run(n, warmup, twin):
    import gvamd
    from gvamd import synth
    hip = common.load_hip()
    gx, gy, res = GRID
    h = gvamd.GridVisionHIP(gx, gy, res)
    tfs = synth.transforms(perturbed=True)
    h.set_transforms(tfs["cam_lidar"], tfs["base_cam"], tfs["base_lidar"])
    x, y, z, _ = synth.scene_with_objects(tfs)
    h.upload_xyz(x, y, z)
    for _ in range(3):
        h.process_frame(gvamd.FRAME_BIN)
    h.set_inflation(*P1)
    h.inflate()
    cost = h.costmap()
    lines = [f"{len(x)} points, {h.nx} x {h.ny} cells, {int((cost == 254).sum())} lethal cells, {int((cost > 0).sum())} with a cost"]
    print(lines[-1], flush=True)
    pin = gvamd.PinnedI8(64)
    rec = pin.array.view(gvamd.MATCH_RESULT_DTYPE)
    for stride, w in SHAPES:
        cfg = gvamd.MatchConfig.of(wx=w, wy=w, wt=w, yaw_step=YAW_STEP, stride=stride, min_points=100)
        h.set_match_config(cfg)
        for _ in range(warmup):
            h.match_scan_async(GUESS, rec)
        us_dev = common.event_us_per_call(hip, h, n, lambda: h.match_scan_async(GUESS, rec))
        walls = []
        for _ in range(n):
            t0 = time.perf_counter()
            got = h.match_scan(GUESS)
            walls.append((time.perf_counter() - t0) * 1e6)
        n_used, cand = int(got["n_used"]), int(np.prod(cfg.shape))
        reads = n_used * cand
        line = (f"stride {stride:2d}, window {cfg.shape[0]} x {cfg.shape[1]} x {cfg.shape[2]}: {n_used} used points, {cand} candidates, "
                f"{reads:.3e} cost reads | device {us_dev:9.1f} us per call ({n} calls), {reads / us_dev * 1e-3:7.1f} G reads/s | "
                f"host-observed median {np.median(walls):9.1f} us, min {np.min(walls):9.1f} us | best shift "
                f"({int(got['best_t'])}, {int(got['best_j'])}, {int(got['best_i'])}) score {int(got['best_score'])} guess score "
                f"{int(got['guess_score'])}")
        if twin:
            t0 = time.perf_counter()
            want = gvamd.match_scan_host(gx, gy, res, cost, x, y, z, tfs["base_lidar"], cfg, GUESS)
            host_ms = (time.perf_counter() - t0) * 1e3
            same = np.asarray(want).tobytes() == np.asarray(got).tobytes()
            line += (f" | host twin on one core {host_ms:9.1f} ms, {reads / host_ms * 1e-6:5.2f} G reads/s, record "
                     f"{'equal' if same else 'DIFFERS'}")
        lines.append(line)
        print(line, flush=True)
    pin.close()
    h.close()
    return lines


def kernel_times(trace_dir):
    d = common.kernel_durations(trace_dir, KERNELS)
    return [f"{k}: {len(v)} dispatches, mean {np.mean(v):9.2f} us, min {np.min(v):9.2f} us, max {np.max(v):9.2f} us"
            for k, v in d.items() if v]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-twin", action="store_true", help="skip gv_match_scan_host (seconds on one core at the larger shape)")
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace run of this script: print kernel times")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace:
        lines = ["per kernel (rocprofv3 --kernel-trace of the same script, both shapes together):"] + kernel_times(a.trace)
        print("\n".join(lines), flush=True)
    else:
        head = "tools/match_time.py: scene_with_objects on 2000 x 2000 cells at 0.1 m, P1, yaw step %g, guess %s:" % (YAW_STEP, GUESS)
        print(head, flush=True)
        lines = [head] + run(a.calls, a.warmup, not a.no_twin)
    if a.out:
        common.append_out(a.out, lines)


if __name__ == "__main__":
    main()
