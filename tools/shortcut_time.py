"""Time of pulling resident paths tight and thinning them to waypoints on the device ([EXTENSION] X21).

Shapes: the 2000 x 2000 grid at 0.1 m of tools/nav_path_time.py with the goal at the centre -- a straight path on the
empty map (the starts on the goal's row and, for S = 256, on the rows about it), the L from the corner (S = 256: cells
spread along the two borders that meet there), the wall-with-one-gap map -- and X17's 200 x 80 serpentine (one corridor
of 8040 cells; S = 256: cells spread along it).  4-connected paths.  Each with S = 1 and S = 256, W = 64 and 256, spacing
0 and 5, wcap 4096.

Per run, by the protocol of tools/nav_path_time.py:
  device    HIP events on the handle's stream around N back-to-back gvx3_shortcut_async calls into a pinned record, the
            waypoints staying resident (way_xy NULL), interval / N: the one kernel;
  host      wall clock of a waited gvx3_shortcut (median of N);
  parent    what a caller does today: gv_get_nav_path of every path and gv_get_costmap (both to the host) plus
            gvx3_shortcut_host on one core (the same arithmetic), wall clock each, median of 3; its records and waypoints
            must equal the device's or the script FAILS;
  digest    sha1 over the records and the entries and indices up to n_waypoints.

Kernel times come from a separate run:
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/shortcut_time.py
and then `python tools/shortcut_time.py --trace DIR` (no GPU).  --out FILE appends what is printed."""
from __future__ import annotations

import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "grid-vision_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import planner_time_common as common  # noqa: E402
from nav_path_time import median_us, plant, serpentine, world_of  # noqa: E402

KERNELS = ["k_shortcut", "k_nav_seeds_shortcut"]
WCAP = 4096


def shapes():
    """(name, geometry, mask, goal cell, {1: [start cell], 256: [start cells]} or None: spread along the corridor, cap)"""
    big = (200, 200, 0.1)
    n = 2000
    empty = np.zeros((n, n), bool)
    wall = np.zeros((n, n), bool)
    wall[:, 1200] = True
    wall[1700, 1200] = False
    rows = [(n - 1, n // 2 + i - 128) for i in range(256)]
    spread = [(n - 1, 0)] + [(n - 1 - 15 * i, 0) for i in range(1, 128)] + [(n - 1, 15 * i) for i in range(1, 129)]
    assert len(rows) == len(spread) == 256
    return [("straight, empty 2000^2", big, empty, (n // 2, n // 2), {1: [(n - 1, n // 2)], 256: rows}, 4096),
            ("L from the corner, empty 2000^2", big, empty, (n // 2, n // 2), {1: spread[:1], 256: spread}, 4096),
            ("wall with one gap 2000^2", big, wall, (300, 250), {1: spread[:1], 256: spread}, 4096),
            ("serpentine 200 x 80", (10, 4, 0.05), serpentine(200, 80), (0, 0), None, 4096)]


def digest(info, ent, idx):
    d = hashlib.sha1(info.tobytes())
    for s in range(len(info)):
        k = int(info[s]["n_waypoints"])
        d.update(np.ascontiguousarray(ent[s, :k]).tobytes())
        d.update(np.ascontiguousarray(idx[s, :k]).tobytes())
    return d.hexdigest()[:12]


def resident(gvamd, hip, h):
    """(info, entries, index) of the resident waypoints through gvx3_device_shortcut's pointers"""
    d = h.device_shortcut()
    info = np.zeros(d["S"], gvamd.SHORTCUT_INFO_DTYPE)
    ent, idx = np.zeros((d["S"], d["wcap"]), np.int32), np.zeros((d["S"], d["wcap"]), np.int32)
    h.synchronize()
    for dst, src in ((info, d["info"]), (ent, d["entries"]), (idx, d["index"])):
        assert hip.hipMemcpy(dst.ctypes.data, src, dst.nbytes, 2) == 0
    return info, ent, idx


def run(n, warmup):
    import gvamd
    hip = common.load_hip()
    lines, handles, planted = [], {}, {}
    failed = False
    for name, geo, mask, goal, starts_of, cap in shapes():
        if geo not in handles:
            handles[geo] = gvamd.GridVisionHIP(*geo)
        h = handles[geo]
        res = geo[2]
        if planted.get(geo) is not mask:
            plant(h, mask)
            planted[geo] = mask
        h.set_nav_config(253, 0)
        h.nav_field(np.array([world_of(h, res, *goal)], np.float32))
        if starts_of is None:
            f = h.nav_field_array()
            order = np.argsort(np.where(f < gvamd.NAV_UNREACHABLE, f, 0))[::-1]
            far = [(int(e) % h.nx, int(e) // h.nx) for e in order[:8040:31][:256]]
            starts_of = {1: far[:1], 256: far}
        for S in (1, 256):
            starts = np.array([world_of(h, res, *c) for c in starts_of[S]], np.float32)
            assert len(starts) == S
            pinfo, _ = h.nav_path(starts, cap, 0, keep_xy=False)
            pin = gvamd.PinnedI8(S * 32)
            rec = pin.array.view(gvamd.SHORTCUT_INFO_DTYPE)
            for W in (64, 256):
                for spacing in (0, 5):
                    cfg = gvamd.ShortcutConfig.of(max_cost=252, window=W, spacing=spacing)
                    h.set_shortcut_config(cfg)
                    for _ in range(warmup):
                        h.shortcut_async(WCAP, rec)
                    us_dev = common.event_us_per_call(hip, h, n, lambda: h.shortcut_async(WCAP, rec))
                    us_host = median_us(n, lambda: h.shortcut(WCAP, keep_xy=False))
                    got = resident(gvamd, hip, h)
                    src, cost = [None], [None]

                    def download():
                        e = np.zeros((S, cap), np.int32)
                        k = np.zeros(S, np.int32)
                        for s in range(S):
                            p = h.nav_path_get(s)[1]
                            e[s, :len(p)] = p
                            k[s] = len(p)
                        src[0] = (e, k)
                        cost[0] = h.costmap()

                    us_get = median_us(3, download)
                    twin = [None]
                    us_twin = median_us(3, lambda: twin.__setitem__(0, gvamd.shortcut_host(*geo, cost[0], cfg, src[0][0], src[0][1], WCAP)))
                    same = twin[0][0].tobytes() == got[0].tobytes() and digest(twin[0][0], twin[0][1], twin[0][2]) == digest(*got)
                    failed = failed or not same
                    I = got[0]
                    line = (f"{name}, S = {S}, W = {W}, spacing {spacing}: {int(pinfo['n_cells'].sum())} path cells (longest "
                            f"{int(pinfo['n_cells'].max())}) -> {int(I['n_waypoints'].sum())} waypoints, {int(I['n_anchors'].sum())} anchors, statuses "
                            f"{sorted(set(I['status'].tolist()))} | device {us_dev:9.1f} us per call ({n} calls) | host-observed median {us_host:9.1f} us | "
                            f"parent: gv_get_nav_path x {S} + gv_get_costmap {us_get:10.1f} us + gvx3_shortcut_host on one core {us_twin:10.1f} us = "
                            f"{us_get + us_twin:10.1f} us, result {'equal' if same else 'DIFFERS'} | digest {digest(*got)}")
                    lines.append(line)
                    print(line, flush=True)
            pin.close()
    for h in handles.values():
        h.close()
    return lines, failed


def kernel_times(trace_dir):
    d = common.kernel_durations(trace_dir, KERNELS)
    return [f"{k}: {len(v)} dispatches, mean {np.mean(v):9.2f} us, min {np.min(v):9.2f} us, max {np.max(v):9.2f} us"
            for k, v in d.items() if v]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace run of this script: print kernel times")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    failed = False
    if a.trace:
        lines = ["per kernel (rocprofv3 --kernel-trace of this script):"] + kernel_times(a.trace)
        print("\n".join(lines), flush=True)
    else:
        head = "tools/shortcut_time.py: 4-connected paths, max_cost 252, wcap 4096, pinned records, waypoints resident:"
        print(head, flush=True)
        lines, failed = run(a.calls, a.warmup)
        lines = [head] + lines
    if a.out:
        common.append_out(a.out, lines)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
