"""Time of walking paths down the distance field on the device ([EXTENSION] X17) and of seeding the next field with one.

Shapes: the 2000 x 2000 grid at 0.1 m with the goal at the centre, as an empty map with the start in a corner (some 2000
cells 4-connected, 1000 with diagonals) and as the wall-with-one-gap map of tests/test_gpu_nav.py, each with S = 1 and
S = 64 starts (the 64: the corner and cells spread along the two borders that meet there); and the 200 x 80 serpentine
(one corridor, 8040 cells) with S = 1.

Per shape, by the protocol of tools/traj_score_time.py:
  device    HIP events on the handle's stream around N back-to-back gv_nav_path_async calls into a pinned record, the
            paths staying resident (paths_xy NULL), interval / N: the copy of the start cells and the kernel;
  host      wall clock of a waited gv_nav_path (median of N): what a caller that needs the record observes;
  parent    what the library offered for the same result before: gv_get_nav_field (the whole field to the host) plus the
            walk on one core (gv_nav_path_host, the same arithmetic), wall clock each, median of 5; its records and
            entries must equal the device's or the script says so;
  digest    sha1 over the records and the entries up to n_cells: equal between the builds of an A/B.
For the second half, on the S = 1 shapes: gv_nav_field_from_path against gv_get_nav_path + gv_nav_field over the
read-back centres (wall clock, median of 5; the fields must be equal).

--ab runs the whole script twice in alternation against two builds of the library, the shipped one (the neighbours
straight from global memory) and one built with -DGV_PATH_WINDOW (a 64 x 64 window of the field in LDS) into tools/_ab/
by --build-window (no GPU needed); every run is a process of its own under a time limit (GV_LIB_AB, as tools/lib_ab.py
does).

Kernel times come from a separate run:
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/nav_path_time.py
and then `python tools/nav_path_time.py --trace DIR` (no GPU).  --out FILE appends what is printed."""
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

EXACT = (0.0, 0.0, 1.0, 65)           # only a planted cell has a cost
WINDOW_LIB = os.path.join(ROOT, "tools", "_ab", "libgridvision_hip_path_window.so")
KERNELS = ["k_nav_path", "k_nav_seeds_path", "k_nav_relax", "k_nav_init"]


def world_of(h, res, x, y):
    """the centre of the cell behind data-order entry (column x, row y)"""
    ix, iy = h.nx - 1 - x, h.ny - 1 - y
    return (h.pos_x + 0.5 * h.nx * res) - (ix + 0.5) * res, (h.pos_y + 0.5 * h.ny * res) - (iy + 0.5) * res


def plant(h, mask):
    lo = np.where(mask.reshape(-1)[::-1], np.float32(10.0), np.float32(-10.0)).astype(np.float32)   # cell = G - 1 - entry
    h.set_log_odds(lo)
    h.update_map()
    h.set_inflation(*EXACT)
    h.inflate()


def serpentine(nx, ny):
    m = np.zeros((ny, nx), bool)
    m[1::2, :] = True
    for i, y in enumerate(range(1, ny, 2)):
        m[y, nx - 1 if i % 2 == 0 else 0] = False
    return m


def shapes():
    """(name, geometry, mask, goal cell, [start cells], cap)"""
    big = (200, 200, 0.1)
    n = 2000
    corner = [(n - 1, 0)]
    spread = corner + [(n - 1 - 60 * i, 0) for i in range(1, 32)] + [(n - 1, 60 * i) for i in range(1, 33)]
    assert len(spread) == 64
    empty = np.zeros((n, n), bool)
    wall = np.zeros((n, n), bool)
    wall[:, 1200] = True
    wall[1700, 1200] = False
    return [("empty 2000^2, S = 1", big, empty, (n // 2, n // 2), corner, 4096),
            ("empty 2000^2, S = 64", big, empty, (n // 2, n // 2), spread, 4096),
            ("wall with one gap 2000^2, S = 1", big, wall, (300, 250), corner, 8192),
            ("wall with one gap 2000^2, S = 64", big, wall, (300, 250), spread, 8192),
            ("serpentine 200 x 80, S = 1", (10, 4, 0.05), serpentine(200, 80), (0, 0), None, 16384)]   # None: the farthest cell


def digest(info, entries):
    d = hashlib.sha1(info.tobytes())
    for s in range(len(info)):
        d.update(np.ascontiguousarray(entries[s, :int(info[s]["n_cells"])]).tobytes())
    return d.hexdigest()[:12]


def median_us(n, call):
    walls = []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        walls.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(walls))


def run(n, warmup):
    import gvamd
    hip = common.load_hip()
    lines = []
    handles = {}
    planted = {}
    for name, geo, mask, goal, cells, cap in shapes():
        if geo not in handles:
            handles[geo] = gvamd.GridVisionHIP(*geo)
        h = handles[geo]
        res = geo[2]
        if planted.get(geo) is not mask:
            plant(h, mask)
            planted[geo] = mask
        h.set_nav_config(253, 0)
        goal_xy = np.array([world_of(h, res, *goal)], np.float32)
        h.nav_field(goal_xy)
        if cells is None:
            f = h.nav_field_array()
            far = int(np.argmax(np.where(f < gvamd.NAV_UNREACHABLE, f, 0)))
            cells = [(far % h.nx, far // h.nx)]
        starts = np.array([world_of(h, res, *c) for c in cells], np.float32)
        S = len(starts)
        pin = gvamd.PinnedI8(S * 32)
        rec = pin.array.view(gvamd.NAV_PATH_INFO_DTYPE)
        for flags, tag in ((0, "4-connected"), (gvamd.PATH_DIAGONAL, "diagonal")):
            for _ in range(warmup):
                h.nav_path_async(starts, cap, rec, None, flags)
            us_dev = common.event_us_per_call(hip, h, n, lambda: h.nav_path_async(starts, cap, rec, None, flags))
            us_host = median_us(n, lambda: h.nav_path(starts, cap, flags, keep_xy=False))
            info = rec.copy()
            entries = np.zeros((S, cap), np.int32)
            for s in range(S):
                e = h.nav_path_get(s)[1]
                entries[s, :len(e)] = e
            cells_total = int(info["n_cells"].sum())
            field = [None]
            us_get = median_us(5, lambda: field.__setitem__(0, h.nav_field_array()))
            twin = [None]
            us_walk = median_us(5, lambda: twin.__setitem__(0, gvamd.nav_path_host(*geo, field[0], starts, cap, flags, keep_xy=True)))
            same = twin[0][0].tobytes() == info.tobytes() and digest(twin[0][0], twin[0][1]) == digest(info, entries)
            line = (f"{name}, {tag}: {cells_total} cells (longest {int(info['n_cells'].max())}), statuses {sorted(set(info['status'].tolist()))} | "
                    f"device {us_dev:8.1f} us per call ({n} calls), {us_dev * 1e3 / max(int(info['n_cells'].max()), 1):6.1f} ns per step of the "
                    f"longest | host-observed median {us_host:8.1f} us | parent: gv_get_nav_field {us_get:9.1f} us + walk on one core "
                    f"{us_walk:8.1f} us = {us_get + us_walk:9.1f} us, result {'equal' if same else 'DIFFERS'} | digest {digest(info, entries)}")
            lines.append(line)
            print(line, flush=True)
        if S == 1:   # the second half: the path as the seeds of the next field
            h.nav_path(starts, cap, 0, keep_xy=False)
            fa = [None]

            def on_device():
                h.nav_field_from_path(0)

            def through_host():
                xy = h.nav_path_get(0)[2]
                h.nav_field(xy)

            us_a = median_us(5, on_device)
            fa[0] = h.nav_field_array()
            us_b = median_us(5, through_host)
            same = fa[0].tobytes() == h.nav_field_array().tobytes()
            line = (f"{name}, field from the path: gv_nav_field_from_path {us_a:9.1f} us | gv_get_nav_path + gv_nav_field {us_b:9.1f} us, "
                    f"field {'equal' if same else 'DIFFERS'}")
            lines.append(line)
            print(line, flush=True)
        pin.close()
    for h in handles.values():
        h.close()
    return lines


def kernel_times(trace_dir):
    d = common.kernel_durations(trace_dir, KERNELS)
    return [f"{k}: {len(v)} dispatches, mean {np.mean(v):9.2f} us, min {np.min(v):9.2f} us, max {np.max(v):9.2f} us"
            for k, v in d.items() if v]


def build_window():
    from gvamd import build as b
    os.makedirs(os.path.dirname(WINDOW_LIB), exist_ok=True)
    return b.build(lib=WINDOW_LIB, extra=["-DGV_PATH_WINDOW"], obj_dir=os.path.join(ROOT, "tools", "_ab", "obj_path_window"))


def ab(calls, warmup, out, limit):
    """two alternating rounds, a process of its own per run, each under `limit` seconds; stops at the first that fails"""
    assert os.path.exists(WINDOW_LIB), "build it first: python tools/nav_path_time.py --build-window"
    for rnd in range(2):
        for label, lib in (("direct from global memory (shipped)", None), ("LDS window (-DGV_PATH_WINDOW)", WINDOW_LIB)):
            head = f"--- A/B round {rnd + 1}: {label}"
            print(head, flush=True)
            if out:
                common.append_out(out, [head])
            env = dict(os.environ)
            env.pop("GV_LIB_AB", None)
            if lib:
                env["GV_LIB_AB"] = lib
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--calls", str(calls), "--warmup", str(warmup)]
            if out:
                cmd += ["--out", out]
            rc = subprocess.run(cmd, env=env).returncode
            if rc != 0:
                print(f"run ended with status {rc}: stopping", flush=True)
                return rc
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace run of this script: print kernel times")
    ap.add_argument("--build-window", action="store_true", help="build the -DGV_PATH_WINDOW library into tools/_ab/ (no GPU)")
    ap.add_argument("--ab", action="store_true", help="two alternating rounds, shipped against the window build")
    ap.add_argument("--limit", type=int, default=240, help="seconds a run of --ab may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.build_window:
        print(build_window())
        return 0
    if a.ab:
        return ab(a.calls, a.warmup, a.out, a.limit)
    if a.trace:
        lines = ["per kernel (rocprofv3 --kernel-trace of the same script, every shape together):"] + kernel_times(a.trace)
        print("\n".join(lines), flush=True)
    else:
        head = "tools/nav_path_time.py: goal field with (253, 0), paths resident (paths_xy NULL), pinned records:"
        print(head, flush=True)
        lines = [head] + run(a.calls, a.warmup)
    if a.out:
        common.append_out(a.out, lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
