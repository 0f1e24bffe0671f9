"""Time of gv_nav_field and gv_score_nav ([EXTENSION] X9) on the 2000 x 2000 and the 500 x 200 grid after the 12-tick fill
of tools/inflate_time.py, inflated with P1.

Per call: wall time (the call waits on the host, so the host's clock is the call's time) and rounds of gv_nav_field for a
goal at the map's centre and for a 300-seed path, at cost weights 0 and 3: the median of N calls.  Beside each the host
alternative it replaces, timed in the same process: gv_get_costmap (the download) plus scipy.sparse.csgraph.dijkstra on
one core over the same cells and steps (the graph's construction is timed apart: a planner would keep it).  The two
fields must be equal, or the script fails.

gv_score_nav_async: HIP events on the handle's stream around M back-to-back calls, K x P = 2000 x 56 and 250 x 20, poses
from pinned host memory and from device memory, records into pinned memory.

Per kernel: run
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/nav_field_time.py
and then `python tools/nav_field_time.py --trace DIR`, which reads the trace (no GPU) and prints count, mean and total
per kernel.  `--resources` prints the compiler's resource report of gv_navfield.hip (no GPU).  --out FILE appends what
is printed."""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "grid-vision_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import planner_time_common as common  # noqa: E402

GRIDS = [(200, 200, 0.1), (50, 20, 0.1)]
P1 = (0.35, 0.55, 10.0, 65)
WEIGHTS = [0, 3]
OBSTACLE_COST = 253
SHAPES = [(2000, 56), (250, 20)]
KERNELS = ["k_nav_init", "k_nav_seeds", "k_nav_relax", "k_score_nav"]


def world_of(h, res, x, y):
    """the centre of the cell behind data-order entry (column x, row y)"""
    ix, iy = h.nx - 1 - x, h.ny - 1 - y
    return (h.pos_x + 0.5 * h.nx * res) - (ix + 0.5) * res, (h.pos_y + 0.5 * h.ny * res) - (iy + 0.5) * res


def seed_lists(h, res, cost):
    """{"goal": (1, 2), "path": (300, 2)} float32: the free cell nearest the centre; 300 free cells nearest a diagonal line"""
    c2 = cost.reshape(h.ny, h.nx)
    ys, xs = np.nonzero(c2 < OBSTACLE_COST)
    i = int(np.argmin((ys - h.ny // 2) ** 2 + (xs - h.nx // 2) ** 2))
    goal = np.array([world_of(h, res, int(xs[i]), int(ys[i]))], np.float32)
    path = []
    for t in np.linspace(0.1, 0.9, 300):
        x, y = int(t * h.nx), int((0.2 + 0.6 * t) * h.ny)
        j = int(np.argmin(np.abs(ys - y) * 4096 + np.abs(xs - x))) if c2[y, x] >= OBSTACLE_COST else None
        path.append(world_of(h, res, x, y) if j is None else world_of(h, res, int(xs[j]), int(ys[j])))
    return {"goal": goal, "path": np.array(path, np.float32)}


def host_graph(cost, nx, ny, step):
    from scipy.sparse import coo_matrix
    st = step.astype(np.int64)[cost].reshape(ny, nx)
    idx = np.arange(nx * ny, dtype=np.int64).reshape(ny, nx)
    rows, cols, w = [], [], []
    for src, dst in ((np.s_[:, :-1], np.s_[:, 1:]), (np.s_[:, 1:], np.s_[:, :-1]), (np.s_[:-1, :], np.s_[1:, :]),
                     (np.s_[1:, :], np.s_[:-1, :])):
        ok = (st[src] != 0) & (st[dst] != 0)
        rows.append(idx[src][ok]); cols.append(idx[dst][ok]); w.append(st[dst][ok])
    g = coo_matrix((np.concatenate(w).astype(np.float64), (np.concatenate(rows), np.concatenate(cols))), shape=(nx * ny, nx * ny))
    return g.tocsr(), st.reshape(-1)


def host_field(graph, st, cells):
    from scipy.sparse.csgraph import dijkstra
    out = np.where(st == 0, 0xFFFFFFFF, 0xFFFFFFFE).astype(np.uint32)
    src = sorted({int(c) for c in cells if st[c] != 0})
    if src:
        d = dijkstra(graph, directed=True, indices=src, min_only=True)
        reach = np.isfinite(d) & (st != 0)
        out[reach] = d[reach].astype(np.uint32)
    return out


def seed_entries(gvamd, grid, h, seeds):
    """data-order entries of the seeds through the library's own getIndex (gv_footprint_cells with the point footprint)"""
    fp = gvamd.Footprint.of(())
    out = []
    for x, y in seeds:
        c = gvamd.footprint_cells(*grid, fp, float(x), float(y), 0.0)
        if c is not None:
            out.append(h.G - 1 - int(c[0]))
    return out


def run(n, m, warmup):
    import gvamd
    from gvamd import synth
    hip = common.load_hip()
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    for grid in GRIDS:
        gx, gy, res = grid
        h = gvamd.GridVisionHIP(gx, gy, res)
        for t in range(12):
            h.update_map_poses(common.fill_poses(synth, h, res, 40, 100 + t))
        h.set_inflation(*P1)
        h.inflate()
        h.synchronize()
        t_get = []
        for _ in range(5):
            t0 = time.perf_counter()
            cost = h.costmap()
            t_get.append(time.perf_counter() - t0)
        seeds = seed_lists(h, res, cost)
        say(f"{h.nx} x {h.ny}: gv_get_costmap {np.median(t_get) * 1e3:.2f} ms (median of 5); blocked cells "
            f"{int((cost >= OBSTACLE_COST).sum())} of {h.G}")
        for w in WEIGHTS:
            h.set_nav_config(OBSTACLE_COST, w)
            t0 = time.perf_counter()
            graph, st = host_graph(cost, h.nx, h.ny, gvamd.nav_step_table(gvamd.NavConfig(OBSTACLE_COST, w, 0)))
            t_graph = time.perf_counter() - t0
            for kind in ("goal", "path"):
                s = seeds[kind]
                for _ in range(warmup):
                    h.nav_field(s)
                ts, rounds = [], set()
                for _ in range(n):
                    t0 = time.perf_counter()
                    info = h.nav_field(s)
                    ts.append(time.perf_counter() - t0)
                    rounds.add(info["rounds"])
                got = h.nav_field_array()
                t0 = time.perf_counter()
                want = host_field(graph, st, seed_entries(gvamd, grid, h, s))
                t_dij = time.perf_counter() - t0
                assert got.tobytes() == want.tobytes(), (grid, w, kind, "the host's field differs from the device's")
                reach = int((got < 0xFFFFFFFE).sum())
                say(f"{h.nx:4d} x {h.ny:4d} weight {w} {kind:4s}: gv_nav_field median {np.median(ts) * 1e3:8.3f} ms (min {np.min(ts) * 1e3:8.3f}, "
                    f"{n} calls), rounds {sorted(rounds)}, seeds used {info['n_seeds_used']}, reachable {reach}; host: download "
                    f"{np.median(t_get) * 1e3:.2f} ms + dijkstra {t_dij * 1e3:9.1f} ms (graph built once in {t_graph * 1e3:.0f} ms); fields equal")
        # the sampler, against the last field
        for K, P in SHAPES:
            poses = common.arcs(h, K, P, seed=K, start=(-4.0, 1.0))
            pin_in, pin_s = gvamd.PinnedF32(poses.size), gvamd.PinnedI8(K * 24)
            pin_in.array[:] = poses.reshape(-1)
            dptr = common.device_copy(hip, poses)
            scores = pin_s.array.view(gvamd.NAV_SCORE_DTYPE)
            want = h.score_nav(poses)
            for label, device in (("pinned poses", False), ("device poses", True)):
                def call():
                    h.score_nav_async(None if device else pin_in.array, K, P, scores, device_ptr=dptr.value if device else None)
                for _ in range(warmup):
                    call()
                h.synchronize()
                assert scores.tobytes() == want.tobytes()
                us = common.event_us_per_call(hip, h, m, call)
                say(f"{h.nx:4d} x {h.ny:4d} gv_score_nav_async {K:5d} x {P:2d} {label:12s}: {m} calls, {us:8.2f} us per call, "
                    f"bad poses {int(want['n_bad'].sum())} of {K * P}")
            hip.hipFree(dptr)
            pin_in.close()
            pin_s.close()
        h.close()
    return lines


def kernel_times(trace_dir):
    per = common.kernel_durations(trace_dir, KERNELS)
    lines = []
    for k in KERNELS:
        d = np.array(per[k])
        if len(d):
            lines.append(f"{k:12s}: {len(d):7d} dispatches, mean {d.mean():8.2f} us, median {np.median(d):8.2f}, max {d.max():8.2f}, "
                         f"total {d.sum() / 1e3:9.2f} ms")
    return lines


def resources():
    """the kernels of gv_navfield.hip as tools/kernel_resources.py compiles and reads them"""
    import kernel_resources as kr
    fields = (("sgprs", "TotalSGPRs"), ("vgprs", "VGPRs"), ("scratch", "ScratchSize [bytes/lane]"), ("waves", "Occupancy [waves/SIMD]"),
              ("sgpr_spill", "SGPRs Spill"), ("vgpr_spill", "VGPRs Spill"), ("lds", "LDS Size [bytes/block]"))
    with tempfile.TemporaryDirectory() as d:
        res = kr.parse_remarks(kr.compile_file("gv_navfield.hip", d)[1])
    lines = []
    for sym, r in res.items():
        name = [k for k in KERNELS if k in sym]
        lines.append((name[0] if name else sym) + ":" + "".join(f" {label} {r[key]};" for key, label in fields if key in r))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--score-calls", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace run of this script: print kernel times")
    ap.add_argument("--resources", action="store_true", help="the compiler's resource report of gv_navfield.hip")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace:
        lines = ["per kernel (rocprofv3 --kernel-trace of the same script):"] + kernel_times(a.trace)
        print("\n".join(lines), flush=True)
    elif a.resources:
        lines = ["compiler resource report (gfx950):"] + resources()
        print("\n".join(lines), flush=True)
    else:
        head = "gv_nav_field per call (host clock, the call waits), gv_score_nav_async by HIP events; P1 costmap, obstacle cost 253:"
        print(head, flush=True)
        lines = [head] + run(a.calls, a.score_calls, a.warmup)
    if a.out:
        common.append_out(a.out, lines)


if __name__ == "__main__":
    main()
