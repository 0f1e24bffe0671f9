"""Time of scoring trajectories against predicted moving objects ([EXTENSION] X13) on the 2000 x 2000 grid of
tools/control_step_time.py (12-tick fill, P1, rectangle footprint, goal field).  Shapes K x P = 2000 x 56 (an MPPI batch)
and 250 x 20 (a DWB fan), 3 circles (off_x -1, 0.5, 2: the yaw is read), 16 and 64 objects.

Per case, by the protocol of tools/traj_score_time.py (HIP events on the handle's stream around N back-to-back calls,
interval / N; device poses, pinned records):
  dyn       gv_score_dynamic_async;
  traj      gv_score_trajectories_async on the same batch in the same run: the yardstick;
  step      gv_control_step_async over the resident rollout of the same shape without and with the dyn configuration;
  host      gv_dyn_score_poses on one core (wall clock, 3 calls).
The device's records must equal the host twin's in the integer fields wherever they can be compared exactly (the script
counts the trajectories whose records differ: a last bit of sin or cos can move a cost) or the script says so.

Kernel times come from a separate run:
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/dyn_score_time.py
and then `python tools/dyn_score_time.py --trace DIR` (no GPU).  --out FILE appends what is printed."""
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
OBJECTS = [16, 64]
DT = 0.1
WEIGHTS = (1, 2, 4, 0, 1)
KERNELS = ["k_score_dynamic", "k_score_trajectories"]


def objects(gvamd, h, n, seed):
    """n cars and pedestrians ahead of the start of the rollouts (which run some 14 m in 5.6 s), up to 3 m/s"""
    rng = np.random.default_rng(seed)
    rows = np.stack([h.pos_x - 20.0 + rng.uniform(6, 40, n), h.pos_y + 5.0 + rng.uniform(-20, 25, n), rng.uniform(-3.1, 3.1, n),
                     rng.uniform(0.5, 4.5, n), rng.uniform(0.5, 2.0, n), rng.uniform(-3, 3, n), rng.uniform(-3, 3, n)], axis=1)
    return gvamd.moving_objects(rows)


def controls(K, P, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.normal(2.5, 0.4, K * P), rng.normal(0.0, 0.35, K * P)], axis=1).astype(np.float32).reshape(K, P, 2)


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
    h.nav_field(np.array([(h.pos_x + 30.0, h.pos_y + 20.0)], np.float32))
    h.set_motion_model(gvamd.MotionModel(gvamd.MOTION_DIFF, DT, 0))
    w = gvamd.CriticWeights(*WEIGHTS, 0)
    cfg = gvamd.DynConfig.of(off_x=(-1.0, 0.5, 2.0), radius=1.1, influence_radius=3.0, cost_scaling_factor=2.0, quantum=0.05, t0=DT,
                             dt=DT, collision_cost=253, w_sum=1, w_max=2)
    lines = []
    for K, P in SHAPES:
        h.rollout(start, controls(K, P, K))
        poses = h.rollout_array()
        ptr = h.device_rollout()[0]
        pin_d, pin_t, pin_r = gvamd.PinnedI8(K * 24), gvamd.PinnedI8(K * 16), gvamd.PinnedI8(16)
        ds, ts = pin_d.array.view(gvamd.DYN_SCORE_DTYPE), pin_t.array.view(gvamd.TRAJ_SCORE_DTYPE)
        res_d = pin_r.array.view(gvamd.CONTROL_RESULT_DTYPE)
        h.set_dyn_config(None)
        for _ in range(warmup):
            h.control_step_async(w, res_d)
        step_off = common.event_us_per_call(hip, h, n, lambda: h.control_step_async(w, res_d))
        for _ in range(warmup):
            h.score_trajectories_async(None, K, P, ts, device_ptr=ptr)
        us_traj = common.event_us_per_call(hip, h, n, lambda: h.score_trajectories_async(None, K, P, ts, device_ptr=ptr))
        for n_obj in OBJECTS:
            objs = objects(gvamd, h, n_obj, 7 + n_obj)
            h.set_dyn_config(cfg)
            h.set_moving_objects(objs)
            for _ in range(warmup):
                h.score_dynamic_async(None, K, P, ds, device_ptr=ptr)
            h.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                twin = gvamd.dyn_score_poses(cfg, objs, poses)
            host_ms = (time.perf_counter() - t0) / 3 * 1e3
            differ = int(sum((ds[f] != twin[f]).sum() for f in ("max_cost", "first_collision", "cost_sum")))
            far = float(np.max(np.abs(ds["min_dist2"] - twin["min_dist2"]) / (1.0 + twin["min_dist2"])))
            us_dyn = common.event_us_per_call(hip, h, n, lambda: h.score_dynamic_async(None, K, P, ds, device_ptr=ptr))
            for _ in range(warmup):
                h.control_step_async(w, res_d)
            step_on = common.event_us_per_call(hip, h, n, lambda: h.control_step_async(w, res_d))
            h.synchronize()
            lines.append(f"{K:5d} x {P:2d}, {n_obj:2d} objects: {n} calls, dyn {us_dyn:8.2f} us | traj (yardstick) {us_traj:8.2f} us | "
                         f"control step without {step_off:8.2f} us, with {step_on:8.2f} us | host twin on one core {host_ms:8.2f} ms | "
                         f"{int((ds['first_collision'] >= 0).sum())} of {K} collide, integer fields that differ from the host's {differ}, "
                         f"largest relative min_dist2 difference {far:.1e}")
            print(lines[-1], flush=True)
        for p in (pin_d, pin_t, pin_r):
            p.close()
    h.close()
    return lines


def kernel_times(trace_dir):
    d = common.kernel_durations(trace_dir, KERNELS)
    return [f"{k}: {len(v)} dispatches, mean {np.mean(v):7.2f} us, min {np.min(v):7.2f} us" for k, v in d.items() if v]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace run of this script: print kernel times")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace:
        lines = ["per kernel (rocprofv3 --kernel-trace of the same script, all cases together):"] + kernel_times(a.trace)
        print("\n".join(lines), flush=True)
    else:
        head = ("per call (%d calls, HIP events), 2000 x 2000 cells at 0.1 m, P1, rectangle footprint, goal field, 3 circles, "
                "weights %s:" % (a.calls, WEIGHTS,))
        print(head, flush=True)
        lines = [head] + run(a.calls, a.warmup)
    if a.out:
        common.append_out(a.out, lines)


if __name__ == "__main__":
    main()
