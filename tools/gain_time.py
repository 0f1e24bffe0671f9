"""Time of ranking exploration goals by information gain on the device ([EXTENSION] X20).

Shape: the 2000 x 2000 grid at 0.1 m as X19's explored-disc map (tools/frontier_time.py: free inside a disc of 80 m about
the centre, unknown outside it, walls inside) with 400 never-observed pockets of 3 x 3 cells inside the disc, so that the
frontier has more than 256 clusters.  Six runs, EACH IN A PROCESS OF ITS OWN (this script starts them one after the
other and prints their lines):
  frontier  gvx_frontier_async (cap 256, USE_FIELD) once, then gvx2_frontier_gain_async: 256 candidates,
  list      gvx2_gain_async over 4096 free cells spread over the disc, host entries,
each at R = 50, 127 and 255, with GVX2_GAIN_USE_FIELD.

Per run, by the protocol of tools/frontier_time.py:
  device    HIP events on the handle's stream around N back-to-back calls into pinned destinations, interval / N;
  host      wall clock of a waited call (median of N);
  parent    what a caller does today: gv_to_occupancy_grid (the layer to the host) plus gvx2_gain_host on one core (the
            same arithmetic) over the same candidates, wall clock; its bytes must equal the device's or the script FAILS;
  digest    sha1 over the info and the records.

Kernel times come from a separate run:
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/gain_time.py --one list --radius 127
and then `python tools/gain_time.py --trace DIR` (no GPU).  --out FILE appends what is printed."""
from __future__ import annotations

import argparse
import hashlib
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "grid-vision_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import planner_time_common as common  # noqa: E402
from frontier_time import GEO, INFLATION, median_us, shapes  # noqa: E402

CAP, N_LIST = 256, 4096
RADII = (50, 127, 255)
KERNELS = ["k_gain_rays", "k_gain_finish", "k_nav_seeds_gain"]


def disc_with_pockets(n=2000):
    """X19's explored disc (log-odds, data order) with 400 unknown pockets inside it"""
    lo = shapes(n)[0][1].copy()
    rng = np.random.default_rng(20)
    for _ in range(400):
        r, a = 700.0 * np.sqrt(rng.random()), 2.0 * np.pi * rng.random()
        x, y = int(n // 2 + r * np.cos(a)), int(n // 2 + r * np.sin(a))
        lo[y - 1:y + 2, x - 1:x + 2] = 0.0
    return lo


def list_entries(i8, n=2000):
    """4096 free cells spread over the disc, in entry order"""
    free = np.flatnonzero(i8 == 11)
    return np.ascontiguousarray(free[np.linspace(0, len(free) - 1, N_LIST).astype(np.int64)], np.int32)


def digest(info, recs):
    d = hashlib.sha1(np.atleast_1d(info).tobytes())
    d.update(recs.tobytes())
    return d.hexdigest()[:12]


def run_one(mode, radius, n, warmup):
    import gvamd
    hip = common.load_hip()
    h = gvamd.GridVisionHIP(*GEO)
    lo = disc_with_pockets()
    h.set_log_odds(np.ascontiguousarray((lo.reshape(-1) + np.float32(0.2))[::-1]))   # cell = G - 1 - entry; the update adds -0.2
    h.update_map()
    h.set_inflation(*INFLATION)
    h.inflate()
    h.set_nav_config(253, 0)
    h.nav_field(np.array([(h.pos_x, h.pos_y)], np.float32))
    cfg = gvamd.GainConfig.of(radius=radius, min_gain=1, w_gain=10, w_dist=1)
    h.set_gain_config(cfg)
    flags = gvamd.GAIN_USE_FIELD
    i8 = h.to_occupancy_grid()[0]
    field = h.nav_field_array()
    slots = CAP if mode == "frontier" else N_LIST
    pin_i, pin_r = gvamd.PinnedI8(32), gvamd.PinnedI8(slots * 48)
    info, recs = pin_i.array.view(gvamd.GAIN_INFO_DTYPE), pin_r.array.view(gvamd.GAIN_DTYPE)
    if mode == "frontier":
        h.set_frontier_config(gvamd.FrontierConfig.of(min_cells=3))
        finfo, frecs = h.frontier(CAP, gvamd.FRONTIER_USE_FIELD)
        entries = np.ascontiguousarray(frecs["goal_entry"][:int(finfo["n_written"])], np.int32)
        call = lambda: h.frontier_gain_async(info, recs, flags)   # noqa: E731
        waited = lambda: h.frontier_gain(flags)                   # noqa: E731
    else:
        entries = list_entries(i8)
        call = lambda: h.gain_async(entries, info, recs, flags)   # noqa: E731
        waited = lambda: h.gain(entries, flags)                   # noqa: E731
    for _ in range(warmup):
        call()
    us_dev = common.event_us_per_call(hip, h, n, call)
    us_host = median_us(n, waited)
    call()
    h.synchronize()
    got = (info[0].copy(), recs[:len(entries)].copy())
    us_get = median_us(3, lambda: h.to_occupancy_grid())
    t0 = time.perf_counter()
    twin = gvamd.gain_host(*GEO, i8, cfg, entries, flags, field)
    us_twin = (time.perf_counter() - t0) * 1e6
    same = twin[0].tobytes() == got[0].tobytes() and twin[1].tobytes() == got[1].tobytes()
    assert (recs[len(entries):].view(np.uint8) == 0).all()
    I = got[0]
    line = (f"{mode} R {radius}: {int(I['n_candidates'])} candidates, {int(I['n_ranked'])} ranked, best {int(I['best'])} with score "
            f"{int(I['best_score'])}, unknown cells in sight {int(got[1]['n_unknown'].min())}..{int(got[1]['n_unknown'].max())} | device "
            f"{us_dev:10.1f} us per call ({n} calls) | host-observed median {us_host:10.1f} us | parent: gv_to_occupancy_grid {us_get:8.1f} us + "
            f"gvx2_gain_host on one core {us_twin:12.1f} us = {us_get + us_twin:12.1f} us, result {'equal' if same else 'DIFFERS'} | "
            f"digest {digest(*got)}")
    print(line, flush=True)
    pin_i.close()
    pin_r.close()
    h.close()
    return 0 if same else 1


def kernel_times(trace_dir):
    d = common.kernel_durations(trace_dir, KERNELS)
    return [f"{k}: {len(v)} dispatches, mean {np.mean(v):9.2f} us, min {np.min(v):9.2f} us, max {np.max(v):9.2f} us"
            for k, v in d.items() if v]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--one", choices=("frontier", "list"), default=None, help="one run in this process (with --radius)")
    ap.add_argument("--radius", type=int, default=127)
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace run of this script: print kernel times")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.one:
        return run_one(a.one, a.radius, a.calls, a.warmup)
    if a.trace:
        lines = ["per kernel (rocprofv3 --kernel-trace of `--one list --radius 127`):"] + kernel_times(a.trace)
        print("\n".join(lines), flush=True)
    else:
        lines = ["tools/gain_time.py: 2000 x 2000 at 0.1 m, explored disc with 400 pockets, USE_FIELD, pinned destinations, a process per run:"]
        print(lines[0], flush=True)
        rc = 0
        for mode in ("frontier", "list"):
            for radius in RADII:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", mode, "--radius", str(radius), "--calls", str(a.calls),
                                    "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=900)
                print(r.stdout, end="", flush=True)
                lines += r.stdout.splitlines()
                if r.returncode:
                    print(r.stderr[-2000:], flush=True)
                    lines.append(f"{mode} R {radius}: FAILED with exit status {r.returncode}")
                    rc = 1
                    break          # nothing more is started on the device behind a run that failed
            if rc:
                break
        if a.out:
            common.append_out(a.out, lines)
        return rc
    if a.out:
        common.append_out(a.out, lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
