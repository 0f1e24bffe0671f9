"""Time of finding frontier clusters on the device ([EXTENSION] X19) and of seeding the distance field with them.

Shapes: the 2000 x 2000 grid at 0.1 m as an explored-disc map (free inside a disc of 80 m about the centre, unknown
outside it, walls inside) and as the checkerboard worst case (free and unknown alternate: one 8-connected component of two
million cells over every tile).

Per shape, by the protocol of tools/nav_path_time.py:
  device    HIP events on the handle's stream around N back-to-back gvx_frontier_async calls into pinned destinations,
            interval / N, without and with GVX_FRONTIER_USE_FIELD;
  host      wall clock of a waited gvx_frontier (median of N);
  parent    what a caller does today: gv_to_occupancy_grid (the layer to the host) plus gvx_frontier_host on one core (the
            same arithmetic), wall clock each, median of 3; its bytes must equal the device's or the script says so;
  seeds     gvx_nav_field_from_frontier(-1), wall clock (median of 3), and the rounds it took;
  digest    sha1 over the info, the written records and the labels.

Kernel times come from a separate run:
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/frontier_time.py
and then `python tools/frontier_time.py --trace DIR` (no GPU).  --out FILE appends what is printed."""
from __future__ import annotations

import argparse
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "grid-vision_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import planner_time_common as common  # noqa: E402

INFLATION = (0.35, 0.55, 10.0, 65)
GEO = (200, 200, 0.1)
CAP = 256
KERNELS = ["k_frontier_cells", "k_frontier_merge", "k_frontier_flatten", "k_frontier_count", "k_frontier_roots", "k_frontier_scan",
           "k_frontier_ranks", "k_frontier_sums", "k_frontier_centre", "k_frontier_finish", "k_nav_seeds_frontier"]


def shapes(n=2000):
    """(name, log-odds layer in data order: -10 free, 0 unknown, +10 occupied)"""
    yy, xx = np.mgrid[0:n, 0:n]
    disc = np.where((xx - n // 2) ** 2 + (yy - n // 2) ** 2 <= 800 ** 2, -10.0, 0.0).astype(np.float32)
    rng = np.random.default_rng(19)
    for _ in range(40):                                   # walls inside the disc
        x0, y0, length = rng.integers(300, 1700), rng.integers(300, 1700), rng.integers(20, 200)
        if rng.random() < 0.5:
            disc[y0, x0:x0 + length] = 10.0
        else:
            disc[y0:y0 + length, x0] = 10.0
    board = np.where((xx + yy) % 2 == 0, -10.0, 0.0).astype(np.float32)
    return [("explored disc 2000^2", disc), ("checkerboard 2000^2", board)]


def digest(info, recs, labels):
    d = hashlib.sha1(np.atleast_1d(info).tobytes())
    d.update(recs.tobytes())
    d.update(labels.tobytes())
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
    h = gvamd.GridVisionHIP(*GEO)
    cfg = gvamd.FrontierConfig.of(min_cells=3)
    h.set_frontier_config(cfg)
    h.set_nav_config(253, 0)
    pin_i, pin_r = gvamd.PinnedI8(32), gvamd.PinnedI8(CAP * 64)
    info, recs = pin_i.array.view(gvamd.FRONTIER_INFO_DTYPE), pin_r.array.view(gvamd.FRONTIER_DTYPE)
    lines = []
    for name, lo in shapes():
        h.set_log_odds(np.ascontiguousarray((lo.reshape(-1) + np.float32(0.2))[::-1]))   # cell = G - 1 - entry; the update adds -0.2
        h.update_map()
        h.set_inflation(*INFLATION)
        h.inflate()
        centre = np.array([(h.pos_x, h.pos_y)], np.float32)
        h.nav_field(centre)
        for flags, tag in ((0, "no field"), (gvamd.FRONTIER_USE_FIELD, "USE_FIELD")):
            for _ in range(warmup):
                h.frontier_async(CAP, info, recs, flags)
            us_dev = common.event_us_per_call(hip, h, n, lambda: h.frontier_async(CAP, info, recs, flags))
            us_host = median_us(n, lambda: h.frontier(CAP, flags))
            got = (info[0].copy(), recs.copy(), h.frontier_labels())
            i8 = [None]
            us_get = median_us(3, lambda: i8.__setitem__(0, h.to_occupancy_grid()[0]))
            field = h.nav_field_array() if flags else None
            twin = [None]
            us_twin = median_us(3, lambda: twin.__setitem__(0, gvamd.frontier_host(*GEO, i8[0], cfg, CAP, flags, None, field)))
            same = digest(*twin[0]) == digest(*got)
            I = got[0]
            line = (f"{name}, {tag}: {int(I['n_frontier_cells'])} frontier cells, {int(I['n_components'])} components, "
                    f"{int(I['n_clusters'])} clusters, largest {int(I['largest'])}, best {int(I['best'])} | device {us_dev:9.1f} us per call "
                    f"({n} calls) | host-observed median {us_host:9.1f} us | parent: gv_to_occupancy_grid {us_get:9.1f} us + "
                    f"gvx_frontier_host on one core {us_twin:11.1f} us = {us_get + us_twin:11.1f} us, result {'equal' if same else 'DIFFERS'} | "
                    f"digest {digest(*got)}")
            lines.append(line)
            print(line, flush=True)
        h.frontier(CAP, 0)
        nav = [None]
        us_seed = median_us(3, lambda: nav.__setitem__(0, h.nav_field_from_frontier(-1)))
        line = f"{name}, gvx_nav_field_from_frontier(-1): {us_seed:9.1f} us, {nav[0]['n_seeds_used']} seeds, {nav[0]['rounds']} rounds"
        lines.append(line)
        print(line, flush=True)
    pin_i.close()
    pin_r.close()
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
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace run of this script: print kernel times")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace:
        lines = ["per kernel (rocprofv3 --kernel-trace of the same script, both shapes together):"] + kernel_times(a.trace)
        print("\n".join(lines), flush=True)
    else:
        head = f"tools/frontier_time.py: 2000 x 2000 at 0.1 m, cap {CAP}, min_cells 3, pinned destinations:"
        print(head, flush=True)
        lines = [head] + run(a.calls, a.warmup)
    if a.out:
        common.append_out(a.out, lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
