"""Time of one MPPI iteration with its two ends on the device ([EXTENSION] X11): gv_mppi_cycle_async -- sampling, rollout,
both samplers, selection, softmax average -- on the scene of tools/control_step_time.py (the 2000 x 2000 grid after the
12-tick fill, inflated with P1, the 4.5 m x 2.0 m rectangle footprint, a goal field).  Shapes K x P = 2000 x 56 and
250 x 20, diff drive.  The result, the totals and the new nominal land in pinned memory, written by the kernels.

Two figures per shape, the protocol of tools/control_step_time.py:
  events   HIP events on the handle's stream around N back-to-back cycles, interval / N;
  cycle    wall clock of N cycles each ended by gv_synchronize, / N: what a controller waits from seed to nominal.
The yardstick is the same iteration done the way the library allowed before, by the same wall clock on the same handle:
gv_mppi_sample_controls on one core into pinned memory, gv_rollout_async + gv_control_step_async with totals into pinned
memory, gv_synchronize, gv_mppi_average on the host.  It is timed with and without its host sampling; the device cycle
must not be slower than the yardstick WITHOUT the sampling, or the script fails.  The device's new nominal is checked
against gv_mppi_average over the device's own read-backs.

Kernel times come from a separate run:
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/mppi_time.py
and then `python tools/mppi_time.py --trace DIR` (no GPU), which prints the mean duration of the seven kernels per shape.
--out FILE appends what is printed.

--limits ([EXTENSION] X12) is the leg with gv_set_mppi_limits in force: rate limits on (v, w) from a measured velocity, a
minimum turning radius and gamma > 0, so every cycle also dispatches k_mppi_constrain and k_mppi_control_cost (and one
8-byte memset).  The same two figures per shape; the check is gv_mppi_average_cc over the device's own read-backs, the
control costs included, and those against gv_mppi_control_costs by bytes.  The host yardstick has no such path and is
left out, so with --limits (also behind --trace) every kernel is dispatched warmup + 1 + 2 n times per shape.  Without
the flag the script is what it was and runs against a library that has no limits (tools/lib_ab.py's GV_LIB_AB)."""
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
RECT = ((3.4, 1.0), (-1.1, 1.0), (-1.1, -1.0), (3.4, -1.0))
SHAPES = [(2000, 56), (250, 20)]
DT = 0.1
WEIGHTS = (1, 2, 4, 0, 1)     # cost_sum, max_cost, nav last, nav sum, nav best
SIGMA, U_MIN, U_MAX, LAMBDA = (0.4, 0.35), (0.0, -1.0), (4.0, 1.0), 1000.0
SEED = 42
KERNELS = ["k_mppi_sample", "k_rollout", "k_score_trajectories", "k_score_nav", "k_control_select", "k_mppi_partial",
           "k_mppi_finish"]
LIMIT_KERNELS = ["k_mppi_sample", "k_mppi_constrain", "k_rollout", "k_score_trajectories", "k_score_nav", "k_control_select",
                 "k_mppi_control_cost", "k_mppi_partial", "k_mppi_finish"]
RATE_UP, RATE_DOWN, U_PREV, RADIUS, GAMMA = (1.5, 0.8), (3.0, 0.8), (2.4, 0.0), 4.0, 30.0
YARD = ("k_rollout", "k_score_trajectories", "k_score_nav", "k_control_select")   # the yardstick dispatches these too


def run(n, warmup, limits=False):
    import gvamd
    from gvamd import synth
    hip = common.load_hip()
    gx, gy, res = GRID
    h = gvamd.GridVisionHIP(gx, gy, res)
    for t in range(12):
        h.update_map_poses(common.fill_poses(synth, h, res, 40, 100 + t))
    h.set_inflation(*P1)
    h.inflate()
    h.set_footprint(gvamd.Footprint.of(RECT))
    h.set_nav_config(253, 1)
    start = (h.pos_x - 20.0, h.pos_y + 5.0, 0.3)
    info = h.nav_field(np.array([(h.pos_x + 30.0, h.pos_y + 20.0)], np.float32))
    h.set_motion_model(gvamd.MotionModel(gvamd.MOTION_DIFF, DT, 0))
    cfg = gvamd.MppiConfig.of(SIGMA, U_MIN, U_MAX, LAMBDA)
    h.set_mppi(cfg)
    lim = None
    if limits:
        lim = gvamd.MppiLimits.of(RATE_UP, RATE_DOWN, U_PREV, RADIUS, GAMMA)
        h.set_mppi_limits(lim)
    w = gvamd.CriticWeights(*WEIGHTS, 0)
    lines = [f"goal field: {info['n_seeds_used']} seed used, {info['rounds']} rounds"]
    slower = []
    for K, P in SHAPES:
        nominal = np.zeros((P, 2), np.float32)
        nominal[:, 0] = 2.5
        pin_r, pin_t, pin_n = gvamd.PinnedI8(16), gvamd.PinnedI8(K * 8), gvamd.PinnedF32(P * 2)
        res_d, tot_d, nom_d = pin_r.array.view(gvamd.CONTROL_RESULT_DTYPE), pin_t.array.view(np.uint64), pin_n.array
        pin_u = gvamd.PinnedF32(K * P * 2)
        src = pin_u.array.reshape(K, P, 2)
        state = dict(it=0, nominal=nominal.copy())

        def cycle():
            h.mppi_cycle_async(start, K, SEED, state["it"], w, res_d, tot_d, nom_d)
            state["it"] += 1

        def yardstick(sample=True):
            if sample:
                src[:] = gvamd.mppi_sample_controls(cfg, state["nominal"], K, SEED, state["it"])
            h.rollout_async(start, src)
            h.control_step_async(w, res_d, tot_d)
            h.synchronize()
            state["nominal"] = gvamd.mppi_average(cfg, src, tot_d, state["nominal"])
            state["it"] += 1

        h.mppi_set_nominal(nominal)
        for _ in range(warmup):
            cycle()
        h.synchronize()
        before = h.mppi_nominal()
        cycle()
        h.synchronize()
        got = nom_d.reshape(P, 2).copy()
        if limits:
            g = h.mppi_control_costs()
            assert g.tobytes() == gvamd.mppi_control_costs(cfg, lim, h.controls_array(), before).tobytes(), (K, P, "control costs")
            want = gvamd.mppi_average_cc(cfg, h.controls_array(), tot_d, g, before)
        else:
            want = gvamd.mppi_average(cfg, h.controls_array(), tot_d, before)
        differ = int((got.view(np.uint32) != want.view(np.uint32)).sum())
        assert np.abs(got - want).max() <= 1e-6 * (1.0 + np.abs(want).max()), (K, P, "the device's average is off the host's")
        admitted = int(res_d["n_valid"][0])
        if not limits:
            yardstick()
        us = common.event_us_per_call(hip, h, n, cycle)
        h.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            cycle()
            h.synchronize()
        wall = (time.perf_counter() - t0) / n * 1e6
        if limits:
            lines.append(f"{K:5d} x {P:2d}: {n} cycles, events {us:8.2f} us, cycle {wall:8.2f} us | limits and gamma on | {admitted} of {K} "
                         f"admitted, nominal floats that differ from the host average {differ} of {got.size}")
            print(lines[-1], flush=True)
            for p in (pin_r, pin_t, pin_n, pin_u):
                p.close()
            continue
        t0 = time.perf_counter()
        for _ in range(n):
            yardstick()
        wall_y = (time.perf_counter() - t0) / n * 1e6
        t0 = time.perf_counter()
        for _ in range(n):
            yardstick(sample=False)
        wall_ns = (time.perf_counter() - t0) / n * 1e6
        lines.append(f"{K:5d} x {P:2d}: {n} cycles, events {us:8.2f} us, cycle {wall:8.2f} us | yardstick cycle {wall_y:9.2f} us, "
                     f"without its host sampling {wall_ns:8.2f} us | {admitted} of {K} admitted, nominal floats that differ from "
                     f"the host average {differ} of {got.size}")
        print(lines[-1], flush=True)
        if wall > wall_ns:
            slower.append((K, P, wall, wall_ns))
        for p in (pin_r, pin_t, pin_n, pin_u):
            p.close()
    h.close()
    return lines, slower


def kernel_times(trace_dir, n, warmup, limits=False):
    """per shape: mean duration in us of the events loop's dispatches of each kernel from rocprofv3's kernel trace of one
    run of this script.  Per shape the cycle dispatches every kernel warmup + 1 + 2 n times (warm-up, the checked cycle,
    the events loop, the wall-clock loop); the yardstick dispatches four of them once behind the checked cycle and 2 n
    times at the end of the shape."""
    kernels = LIMIT_KERNELS if limits else KERNELS
    d = common.kernel_durations(trace_dir, kernels)
    own, extra = warmup + 1 + 2 * n, 1 + 2 * n
    lines = []
    for i, (K, P) in enumerate(SHAPES):
        parts = []
        for k in kernels:
            yard = k in YARD and not limits
            first = i * (own + (extra if yard else 0)) + warmup + 1 + (1 if yard else 0)
            part = d[k][first:first + n]
            assert len(part) == n, (K, P, k, len(part), len(d[k]))
            parts.append(f"{k} {np.mean(part):7.2f} (min {np.min(part):7.2f})")
        lines.append(f"{K:5d} x {P:2d}: " + ", ".join(parts) + " us")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace run of this script: print kernel times")
    ap.add_argument("--limits", action="store_true", help="the leg with gv_set_mppi_limits (rates, radius, gamma) in force")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    slower = []
    if a.trace:
        lines = ["per kernel (rocprofv3 --kernel-trace of the same script):"] + kernel_times(a.trace, a.calls, a.warmup, a.limits)
        print("\n".join(lines), flush=True)
    else:
        head = ("per MPPI iteration (gv_mppi_cycle_async; %d cycles), 2000 x 2000 cells at 0.1 m, P1, rectangle footprint, goal "
                "field, weights %s, sigma %s, lambda %g%s:" % (a.calls, WEIGHTS, SIGMA, LAMBDA, ", limits and gamma on" if a.limits else ""))
        print(head, flush=True)
        lines, slower = run(a.calls, a.warmup, a.limits)
        lines = [head] + lines
    if a.out:
        common.append_out(a.out, lines)
    if slower:
        sys.exit("the device cycle is slower than the yardstick without its host sampling: %s" % (slower,))


if __name__ == "__main__":
    main()
