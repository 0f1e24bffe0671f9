"""Time of one control cycle with the rollout and the selection on the device ([EXTENSION] X10): gv_rollout_async +
gv_control_step_async on the 2000 x 2000 grid after the 12-tick fill of tools/inflate_time.py, inflated with P1, with the
4.5 m x 2.0 m rectangle footprint and a goal field.  Shapes K x P = 2000 x 56 (an MPPI batch) and 250 x 20 (a DWB fan), for
constant controls from pinned host memory, per-step controls from pinned host memory and per-step controls from device
memory.  The 16-byte result lands in pinned memory, written by the kernel.

Two figures per case, the protocol of tools/traj_score_time.py plus a wall clock:
  events   HIP events on the handle's stream around N back-to-back cycles, interval / N: the device side's rate (an upper
           bound where the host's enqueue cost is longer than the device work);
  cycle    wall clock of N cycles each ended by gv_synchronize, / N: what a controller waits from controls to choice.
The yardstick is the same job done the way the library allowed before, timed by the same wall clock on the same handle:
gv_rollout_poses on one core, gv_score_trajectories_async and gv_score_nav_async with pinned host poses and pinned
records, gv_synchronize, gv_control_select on the host.  Its choice and its totals must equal the device's wherever the
host's and the device's poses are the same bytes, or the script fails; the script prints how many pose floats differ.

Kernel times come from a separate run:
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/control_step_time.py
and then `python tools/control_step_time.py --trace DIR` (no GPU), which prints the mean duration of the four kernels per
case in the same order.  --out FILE appends what is printed."""
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
# (label, constant controls, device controls)
MODES = [("constant, pinned controls", True, False), ("per step, pinned controls", False, False),
         ("per step, device controls", False, True)]
KERNELS = ["k_rollout", "k_score_trajectories", "k_score_nav", "k_control_select"]
WEIGHTS = (1, 2, 4, 0, 1)     # cost_sum, max_cost, nav last, nav sum, nav best


def controls(K, P, seed, constant):
    """diff-drive samples around 2.5 m/s as a sampling controller draws them: 0.25 m a step at DT"""
    rng = np.random.default_rng(seed)
    n = K if constant else K * P
    u = np.stack([rng.normal(2.5, 0.4, n), rng.normal(0.0, 0.35, n)], axis=1).astype(np.float32)
    return u if constant else u.reshape(K, P, 2)


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
    h.set_footprint(gvamd.Footprint.of(RECT))
    h.set_nav_config(253, 1)
    start = (h.pos_x - 20.0, h.pos_y + 5.0, 0.3)
    info = h.nav_field(np.array([(h.pos_x + 30.0, h.pos_y + 20.0)], np.float32))
    model = gvamd.MotionModel(gvamd.MOTION_DIFF, DT, 0)
    h.set_motion_model(model)
    w = gvamd.CriticWeights(*WEIGHTS, 0)
    lines = [f"goal field: {info['n_seeds_used']} seed used, {info['rounds']} rounds"]
    for K, P in SHAPES:
        pin_r, pin_t = gvamd.PinnedI8(16), gvamd.PinnedI8(K * 8)
        res_d, tot_d = pin_r.array.view(gvamd.CONTROL_RESULT_DTYPE), pin_t.array.view(np.uint64)
        pin_poses, pin_ts, pin_ns = gvamd.PinnedF32(K * P * 3), gvamd.PinnedI8(K * 16), gvamd.PinnedI8(K * 24)
        ts, ns = pin_ts.array.view(gvamd.TRAJ_SCORE_DTYPE), pin_ns.array.view(gvamd.NAV_SCORE_DTYPE)
        for label, constant, device in MODES:
            u = controls(K, P, K + int(constant), constant)
            pin_u = gvamd.PinnedF32(u.size)
            pin_u.array[:] = u.reshape(-1)
            src = pin_u.array.reshape(u.shape)
            dptr = common.device_copy(hip, u) if device else None

            def cycle(totals=None):
                if device:
                    h.rollout_async(start, u.shape, constant=constant, device_ptr=dptr.value, P=P)
                else:
                    h.rollout_async(start, src, constant=constant, P=P)
                h.control_step_async(w, res_d, totals)

            def yardstick():
                poses = gvamd.rollout_poses(model, start, src, constant, P)
                pin_poses.array[:] = poses.reshape(-1)
                h.score_trajectories_async(pin_poses.array, K, P, ts)
                h.score_nav_async(pin_poses.array, K, P, ns)
                h.synchronize()
                return poses, gvamd.control_select(w, ts, ns, keep_totals=True)

            for _ in range(warmup):
                cycle()
            cycle(tot_d)
            h.synchronize()
            got_r, got_t = res_d.copy(), tot_d.copy()
            dev_poses = h.rollout_array()
            host_poses, (want_r, want_t) = yardstick()
            differ = int((dev_poses.view(np.uint32) != host_poses.view(np.uint32)).sum())
            same = (dev_poses.view(np.uint32) == host_poses.view(np.uint32)).all(axis=(1, 2))
            assert (got_t[same] == want_t[same]).all(), (K, P, label, "a total differs on equal poses")
            if differ == 0:
                assert got_r.tobytes() == np.array([want_r]).tobytes(), (K, P, label, "the choice differs")
            us = common.event_us_per_call(hip, h, n, cycle)
            h.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                cycle()
                h.synchronize()
            wall = (time.perf_counter() - t0) / n * 1e6
            t0 = time.perf_counter()
            for _ in range(n):
                yardstick()
            wall_y = (time.perf_counter() - t0) / n * 1e6
            t0 = time.perf_counter()
            for _ in range(20):
                gvamd.rollout_poses(model, start, src, constant, P)
            t_roll = (time.perf_counter() - t0) / 20 * 1e6
            lines.append(f"{K:5d} x {P:2d} {label:26s}: {n} cycles, events {us:8.2f} us, cycle {wall:8.2f} us | yardstick cycle "
                         f"{wall_y:8.2f} us ({t_roll:8.2f} us of it gv_rollout_poses on one core) | best {int(got_r['best'][0])} of "
                         f"{int(got_r['n_valid'][0])} admitted, pose floats that differ from the host's {differ} of {dev_poses.size}")
            print(lines[-1], flush=True)
            if dptr is not None:
                hip.hipFree(dptr)
            pin_u.close()
        for p in (pin_r, pin_t, pin_poses, pin_ts, pin_ns):
            p.close()
    h.close()
    return lines


def kernel_times(trace_dir, n, warmup):
    """per case: mean duration in us of the timed dispatches of each kernel from rocprofv3's kernel trace of one run of
    this script.  Per case k_rollout and k_control_select are dispatched warmup + 1 + 2 n times (warm-up, the checked
    cycle, the events loop, the wall-clock loop); the two samplers once more per yardstick cycle: one behind the checked
    cycle, n at the end of the case."""
    d = common.kernel_durations(trace_dir, KERNELS)
    own, extra = warmup + 1 + 2 * n, 1 + n
    lines, i = [], 0
    for K, P in SHAPES:
        for label, _, _ in MODES:
            parts = []
            for k in KERNELS:
                sampler = k in ("k_score_trajectories", "k_score_nav")
                base = i * (own + (extra if sampler else 0))
                # the events loop: the n dispatches behind the warmup and the checked cycle (and, for the samplers, the
                # yardstick's checked cycle)
                first = base + warmup + 1 + (1 if sampler else 0)
                part = d[k][first:first + n]
                assert len(part) == n, (K, P, label, k, len(part), len(d[k]))
                parts.append(f"{k} {np.mean(part):7.2f} (min {np.min(part):7.2f})")
            lines.append(f"{K:5d} x {P:2d} {label:26s}: " + ", ".join(parts) + " us")
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
        head = ("per cycle (gv_rollout_async + gv_control_step_async; %d cycles), 2000 x 2000 cells at 0.1 m, P1, rectangle "
                "footprint, goal field, weights %s:" % (a.calls, WEIGHTS,))
        print(head, flush=True)
        lines = [head] + run(a.calls, a.warmup)
    if a.out:
        common.append_out(a.out, lines)


if __name__ == "__main__":
    main()
