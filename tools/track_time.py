"""Time of one update of the tracker over the tick's boxes ([EXTENSION] X14), device against the path a caller had before
it: the same step on one host core plus gv_set_moving_objects.

Cases: 8, 64 and 128 tracks in steady state with a detection near every track ("typical": the association ends after
a round or two), and the 128-chain of tests/track_cases.py (one pair per round: the kernel's worst case).

Per case:
  device   gv_track_update_async with GV_TRACK_FEED_DYNAMIC, detections already in device memory (GV_TRACK_DEVICE_DETS)
           and host detections (a copy command in front of the kernel): HIP events on the handle's stream around N
           back-to-back calls, interval / N (tools/planner_time_common.py).  The state is reloaded by gv_set_tracks in
           front of every call, so every call does the same work; the reload alone is timed the same way and
           subtracted.
  host     gv_track_step on one core followed by gv_set_moving_objects of its exported objects (wall clock around N
           calls, the stream drained after the last): what the parent commit needs for the same result.
The device's tracks must equal the host twin's bytes or the script says so.  --out FILE appends what is printed."""
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

DT = 0.05


def boxes(gvamd, xy):
    from gvamd import synth
    z = np.zeros(len(xy), synth.LSHAPE_DTYPE)
    z["px"], z["py"], z["qw"], z["length"], z["width"], z["height"] = xy[:, 0], xy[:, 1], 1.0, 4.5, 2.0, 1.5
    return z


def tracks_at(gvamd, xy, v):
    t = np.zeros(len(xy), gvamd.TRACK_DTYPE)
    t["slot"], t["id"], t["hits"], t["det"] = np.arange(len(xy)), 1 + np.arange(len(xy)), 5, -1
    t["x"], t["y"], t["vx"], t["vy"] = xy[:, 0], xy[:, 1], v[:, 0], v[:, 1]
    t["qw"], t["length"], t["width"] = 1.0, 4.5, 2.0
    t["p00"], t["p01"], t["p11"] = 0.05, 0.02, 0.5
    return t


def typical(gvamd, n, seed):
    """n tracks on a 6 m lattice with up to 5 m/s, a detection within 0.3 m of where each will be, in shuffled order"""
    rng = np.random.default_rng(seed)
    xy = np.stack([6.0 * (np.arange(n) % 12), 6.0 * (np.arange(n) // 12)], 1) + rng.uniform(-1.0, 1.0, (n, 2))
    v = rng.uniform(-5.0, 5.0, (n, 2))
    z = xy + v * DT + rng.normal(0.0, 0.1, (n, 2))
    return tracks_at(gvamd, xy, v), boxes(gvamd, z[rng.permutation(n)]), gvamd.TrackConfig.of(gate=2.0)


def chain(gvamd, n):
    gaps = 1.0 + np.arange(2 * n - 1) / 256.0
    pos = np.concatenate([[0.0], np.cumsum(gaps)])
    zero = np.zeros(n)
    return (tracks_at(gvamd, np.stack([pos[0::2], zero], 1), np.zeros((n, 2))), boxes(gvamd, np.stack([pos[1::2], zero], 1)),
            gvamd.TrackConfig.of(gate=3.0))


def run(n_calls, warmup):
    import gvamd
    hip = common.load_hip()
    h = gvamd.GridVisionHIP(50, 20, 0.1)
    h.set_dyn_config(gvamd.DynConfig.of())
    lines = []
    for name, (tracks, dets, cfg) in [("typical,   8 tracks", typical(gvamd, 8, 1)), ("typical,  64 tracks", typical(gvamd, 64, 2)),
                                      ("typical, 128 tracks", typical(gvamd, 128, 3)), ("chain,   128 tracks", chain(gvamd, 128))]:
        dt = 0.0 if name.startswith("chain") else DT
        h.set_track_config(cfg)
        twin_t, _, twin_i, twin_o = gvamd.track_step(cfg, tracks, 1000, dets, dt)
        h.set_tracks(tracks, 1000)
        info, got = h.track_update(dets, dt, feed=True)
        same = got.tobytes() == twin_t.tobytes() and np.array([info]).tobytes() == np.array([twin_i]).tobytes()
        dptr = common.device_copy(hip, dets)

        def reload():
            h.set_tracks(tracks, 1000)

        def dev():
            reload()
            h.track_update_async(None, dt, feed=True, device_ptr=dptr.value, n=len(dets))

        def dev_host_dets():
            reload()
            h.track_update_async(dets, dt, feed=True)

        for f in (reload, dev, dev_host_dets):
            for _ in range(warmup):
                f()
        us_reload = common.event_us_per_call(hip, h, n_calls, reload)
        us_dev = common.event_us_per_call(hip, h, n_calls, dev) - us_reload
        us_dev_h = common.event_us_per_call(hip, h, n_calls, dev_host_dets) - us_reload
        h.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_calls):
            _, _, _, objs = gvamd.track_step(cfg, tracks, 1000, dets, dt)
            h.set_moving_objects(objs)
        h.synchronize()
        us_host = (time.perf_counter() - t0) / n_calls * 1e6
        t0 = time.perf_counter()
        for _ in range(n_calls):
            gvamd.track_step(cfg, tracks, 1000, dets, dt)
        us_step = (time.perf_counter() - t0) / n_calls * 1e6
        hip.hipFree(dptr)
        lines.append(f"{name}: {n_calls} calls, device update {us_dev:7.2f} us (host detections {us_dev_h:7.2f} us; the state reload "
                     f"subtracted from both {us_reload:6.2f} us) | host step + gv_set_moving_objects {us_host:7.2f} us "
                     f"(the step alone {us_step:7.2f} us) | matched {int(info['n_matched'])} exported {int(info['n_exported'])}, "
                     f"tracks {'equal' if same else 'DIFFER FROM'} the host twin's")
        print(lines[-1], flush=True)
    h.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    head = "per call (%d calls): device by HIP events on the handle's stream, host by wall clock through the Python binding:" % a.calls
    print(head, flush=True)
    lines = [head] + run(a.calls, a.warmup)
    if a.out:
        common.append_out(a.out, lines)


if __name__ == "__main__":
    main()
