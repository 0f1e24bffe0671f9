"""Device time of gv_score_trajectories_async ([EXTENSION] X7): HIP events on the handle's stream around N back-to-back
calls on the 2000 x 2000 grid after the 12-tick fill of tools/inflate_time.py, inflated with P1, with the 4.5 m x 2.0 m
rectangle footprint.  Shapes K x P = 2000 x 56 (an MPPI batch) and 250 x 20 (a DWB fan); poses from pinned host memory
(copied per call) and from device memory (read in place); with and without the per-pose costs.  Results land in pinned
memory, written by the kernel.  One line per case: per call in us, poses and outline cells per call, cells per second.

Per-call time = event interval / N.  The calls are enqueued from Python: where a call is shorter than the host's enqueue
cost the interval is an upper bound -- the kernel time is the device side.  For that run
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/traj_score_time.py
and then `python tools/traj_score_time.py --trace DIR`, which reads the trace (no GPU) and prints the kernel's mean
duration per case in the same order.

Beside them the host alternative the call replaces, for the same trajectories: gv_get_costmap (the 4 MB download) and a
one-core loop over gv_footprint_cells -- the library's own geometry -- and the downloaded bytes.  The loop is driven from
Python, a ctypes call and a numpy lookup per pose: the time spent INSIDE gv_footprint_cells is printed separately, it is
what a C++ planner would pay for the geometry (examples/planner_demo.cpp has that loop in C++).  The loop's records must
equal the device's byte for byte, or the script fails.  --out FILE appends what is printed."""
from __future__ import annotations

import argparse
import ctypes as C
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
RECT = ((3.4, 1.0), (-1.1, 1.0), (-1.1, -1.0), (3.4, -1.0))
SHAPES = [(2000, 56), (250, 20)]
# (label, device poses, keep pose costs)
MODES = [("pinned poses", False, False), ("pinned poses +pose_cost", False, True), ("device poses", True, False),
         ("device poses +pose_cost", True, True)]
KERNEL = "k_score_trajectories"


def host_alternative(gvamd, h, fp, poses):
    """(records, pose costs, seconds of gv_get_costmap, seconds inside gv_footprint_cells, seconds of the whole loop)"""
    lib = gvamd.load()
    t0 = time.perf_counter()
    cost = h.costmap()
    t_get = time.perf_counter() - t0
    K, P = poses.shape[:2]
    G = h.G
    scores = np.zeros(K, gvamd.TRAJ_SCORE_DTYPE)
    pose_cost = np.zeros((K, P), np.uint8)
    cells = np.zeros(4096, np.int32)
    n = C.c_int32(0)
    cp, npn = cells.ctypes.data_as(C.c_void_p), C.byref(n)
    gx, gy, res = C.c_uint8(GRID[0]), C.c_uint8(GRID[1]), C.c_double(GRID[2])
    fpp = C.byref(fp)
    t_cells = 0.0
    t0 = time.perf_counter()
    for k in range(K):
        mx, first, total, n_off = 0, -1, 0, 0
        for p in range(P):
            x, y, yaw = poses[k, p]
            a = time.perf_counter()
            rc = lib.gv_footprint_cells(gx, gy, res, fpp, C.c_float(x), C.c_float(y), C.c_float(yaw), cp, C.c_int32(4096), npn)
            t_cells += time.perf_counter() - a
            assert rc == 0
            if n.value < 0:
                pc = centre = fp.off_map_cost
                n_off += 1
            else:
                c = cost[G - 1 - cells[:n.value]]
                centre, pc = int(c[0]), int(c.max())
            pose_cost[k, p] = pc
            total += centre
            mx = max(mx, pc)
            if first < 0 and pc >= fp.collision_cost:
                first = p
        scores[k] = (mx, first, total, n_off)
    return scores, pose_cost, t_get, t_cells, time.perf_counter() - t0


def count_cells(gvamd, fp, poses, stride=7):
    """cells the call reads (the centre and the outline of every on-map pose), estimated from every stride-th pose"""
    total = 0
    for k in range(poses.shape[0]):
        for p in range(0, poses.shape[1], stride):
            c = gvamd.footprint_cells(*GRID, fp, *poses[k, p])
            total += 0 if c is None else len(c)
    return total * stride


def run(n, warmup):
    import gvamd
    from gvamd import synth
    hip = common.load_hip()
    gx, gy, res = GRID
    h = gvamd.GridVisionHIP(gx, gy, res)
    for t in range(12):
        h.update_map_poses(common.fill_poses(synth, h, res, 40, 100 + t))
    h.set_inflation(*P1)
    h.inflate()
    fp = gvamd.Footprint.of(RECT)
    h.set_footprint(fp)
    lines = []
    for K, P in SHAPES:
        poses = common.arcs(h, K, P, seed=K, start=(-20.0, 5.0))
        pin_in, pin_s, pin_p = gvamd.PinnedF32(poses.size), gvamd.PinnedI8(K * 16), gvamd.PinnedI8(K * P)
        pin_in.array[:] = poses.reshape(-1)
        dptr = common.device_copy(hip, poses)
        scores, pc = pin_s.array.view(gvamd.TRAJ_SCORE_DTYPE), pin_p.array.view(np.uint8)
        want_s, want_p, t_get, t_cells, t_loop = host_alternative(gvamd, h, fp, poses)
        n_cells = None
        for label, device, keep in MODES:
            def call():
                h.score_trajectories_async(None if device else pin_in.array, K, P, scores, pc if keep else None,
                                           device_ptr=dptr.value if device else None)
            for _ in range(warmup):
                call()
            h.synchronize()
            assert scores.tobytes() == want_s.tobytes(), (K, P, label, "the host loop's records differ from the device's")
            if keep:
                assert pc.tobytes() == want_p.tobytes(), (K, P, label, "pose costs differ")
            us = common.event_us_per_call(hip, h, n, call)
            if n_cells is None:
                n_cells = count_cells(gvamd, fp, poses)
            lines.append(f"{K:5d} x {P:2d} {label:24s}: {n} calls, {us:8.2f} us per call, {K * P} poses, ~{n_cells / 1e6:5.2f} M cells, "
                         f"{n_cells / (us * 1e-6) / 1e9:6.2f} G cells/s")
            print(lines[-1], flush=True)
        lines.append(f"{K:5d} x {P:2d} host alternative        : gv_get_costmap {t_get * 1e6:8.1f} us + one-core loop {t_loop * 1e3:8.2f} ms "
                     f"({t_cells * 1e3:8.2f} ms of it inside gv_footprint_cells, the rest Python and numpy); records and pose "
                     f"costs equal the device's byte for byte; off-map poses {int(want_s['n_off_map'].sum())}, "
                     f"colliding trajectories {int((want_s['first_collision'] >= 0).sum())}")
        print(lines[-1], flush=True)
        hip.hipFree(dptr)
        for p in (pin_in, pin_s, pin_p):
            p.close()
    h.close()
    return lines


def kernel_times(trace_dir, n, warmup):
    """per case: mean duration in us of the timed dispatches of the kernel, from rocprofv3's kernel trace of one run of
    this script (dispatch order = SHAPES x MODES order, warmup + n dispatches each)"""
    d = common.kernel_durations(trace_dir, [KERNEL])[KERNEL]
    lines, i = [], 0
    for K, P in SHAPES:
        for label, _, _ in MODES:
            part = d[i * (warmup + n) + warmup:(i + 1) * (warmup + n)]
            assert len(part) == n, (K, P, label, len(part), len(d))
            lines.append(f"{K:5d} x {P:2d} {label:24s}: {KERNEL} {np.mean(part):8.2f} us (min {np.min(part):8.2f})")
            i += 1
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace run of this script: print kernel times")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace:
        lines = ["per kernel (rocprofv3 --kernel-trace of the same script):"] + kernel_times(a.trace, a.calls, a.warmup)
        print("\n".join(lines), flush=True)
    else:
        print("per call (HIP events around %d back-to-back gv_score_trajectories_async), 2000 x 2000 cells at 0.1 m, P1, "
              "rectangle footprint:" % a.calls, flush=True)
        lines = ["per call (HIP events around %d back-to-back gv_score_trajectories_async), 2000 x 2000 cells at 0.1 m, P1, "
                 "rectangle footprint:" % a.calls] + run(a.calls, a.warmup)
    if a.out:
        common.append_out(a.out, lines)


if __name__ == "__main__":
    main()
