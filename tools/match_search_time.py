"""Time of the wide-window search ([EXTENSION] X18, gv_match_search) against the exhaustive gv_match_scan (X16), on the
scene of tools/match_time.py, on the same build and in the same run: the 2000 x 2000 grid at 0.1 m, the 1 M-point
scene_with_objects cloud, the map made of that scan itself (three lidar frames), inflated with P1.

  narrow   stride 32 with a 21 x 21 x 21 window and stride 8 with 41 x 41 x 41 (match_time.py's two shapes): the
           exhaustive call, then the search at S = 4, 8, 16;
  wide     stride 8 with 257 x 257 x 41 (no exhaustive call has this window): the search at S = 4, 8, 16, and once, at the
           S that scores the fewest candidates, the alternative it replaces: the costmap's download plus
           gv_match_search_host on one core.
Per line, by the protocol of tools/traj_score_time.py: HIP events on the handle's stream around N back-to-back *_async
calls into pinned destinations, interval / N; then n_survivors / n_blocks and n_scored of the search, and whether the
record equals the exhaustive call's (narrow) or the twin's (wide).

Kernel times (the pool pass and the bound pass separately) come from a separate run:
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/match_search_time.py --no-twin
and then `python tools/match_search_time.py --trace DIR` (no GPU).  --resources FILE writes the compiler's register
account of gv_search.hip (no GPU).  --out FILE appends what is printed."""
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

GRID = (200, 200, 0.1)
P1 = (0.35, 0.55, 10.0, 65)
NARROW = [(32, 10), (8, 20)]          # (stride, window half-width in cells and yaw steps): tools/match_time.py's
WIDE = (8, 128, 20)                   # stride, wx = wy, wt
SIZES = (2, 3, 4)                     # block_log2
YAW_STEP = 0.005
GUESS = (0.3, -0.2, 0.015)
TWIN_LIMIT = 3e10                     # cost reads of the twin's fine pass above which the one-core run is skipped (minutes)
KERNELS = ["k_match_points", "k_match_score", "k_match_select", "k_search_pool_rows", "k_search_pool_cols", "k_search_bound",
           "k_search_seed", "k_search_fine", "k_search_prune", "k_search_select", "k_search_record"]


def _search_line(gvamd, hip, h, cfg, n, warmup, rec, stats):
    h.set_search_config(cfg)
    for _ in range(warmup):
        h.match_search_async(GUESS, rec, stats)
    us = common.event_us_per_call(hip, h, n, lambda: h.match_search_async(GUESS, rec, stats))
    got_r, got_s = h.match_search(GUESS)
    return us, got_r, got_s, (f"  search S {1 << cfg.block_log2:2d}: device {us:9.1f} us per call ({n} calls) | {int(got_s['n_survivors'])} of "
                              f"{int(got_s['n_blocks'])} blocks survive ({100.0 * int(got_s['n_survivors']) / int(got_s['n_blocks']):.2f} %), "
                              f"{int(got_s['n_scored'])} of {int(np.prod(cfg.shape))} candidates scored, L {int(got_s['lower_score'])} "
                              f"bound max {int(got_s['bound_max'])} best {int(got_r['best_score'])}")


def run(n, warmup, twin):
    import gvamd
    from gvamd import synth
    hip = common.load_hip()
    gx, gy, res = GRID
    h = gvamd.GridVisionHIP(gx, gy, res)
    tfs = synth.transforms(perturbed=True)
    h.set_transforms(tfs["cam_lidar"], tfs["base_cam"], tfs["base_lidar"])
    x, y, z, _ = synth.scene_with_objects(tfs)
    h.upload_xyz(x, y, z)
    for _ in range(3):
        h.process_frame(gvamd.FRAME_BIN)
    h.set_inflation(*P1)
    h.inflate()
    cost = h.costmap()
    lines = [f"{len(x)} points, {h.nx} x {h.ny} cells, {int((cost == 254).sum())} lethal cells, {int((cost > 0).sum())} with a cost"]
    print(lines[-1], flush=True)
    pr, ps = gvamd.PinnedI8(64), gvamd.PinnedI8(32)
    rec, stats = pr.array.view(gvamd.MATCH_RESULT_DTYPE), ps.array.view(gvamd.SEARCH_STATS_DTYPE)

    def say(line):
        lines.append(line)
        print(line, flush=True)

    for stride, w in NARROW:
        mcfg = gvamd.MatchConfig.of(wx=w, wy=w, wt=w, yaw_step=YAW_STEP, stride=stride, min_points=100)
        h.set_match_config(mcfg)
        for _ in range(warmup):
            h.match_scan_async(GUESS, rec)
        us_scan = common.event_us_per_call(hip, h, n, lambda: h.match_scan_async(GUESS, rec))
        want = h.match_scan(GUESS)
        say(f"stride {stride:2d}, window {mcfg.shape[0]} x {mcfg.shape[1]} x {mcfg.shape[2]}, {int(want['n_used'])} used points: exhaustive "
            f"gv_match_scan {us_scan:9.1f} us per call ({n} calls), best shift ({int(want['best_t'])}, {int(want['best_j'])}, "
            f"{int(want['best_i'])})")
        for lg in SIZES:
            cfg = gvamd.SearchConfig.of(wx=w, wy=w, wt=w, yaw_step=YAW_STEP, stride=stride, min_points=100, block_log2=lg)
            us, got_r, _, line = _search_line(gvamd, hip, h, cfg, n, warmup, rec, stats)
            same = np.asarray(got_r).tobytes() == np.asarray(want).tobytes()
            say(line + f" | {us_scan / us:5.2f} x the exhaustive call's speed, record {'equal' if same else 'DIFFERS'}")
    stride, w, wt = WIDE
    say(f"stride {stride:2d}, window {2 * wt + 1} x {2 * w + 1} x {2 * w + 1} ({(2 * wt + 1) * (2 * w + 1) ** 2} candidates): the search alone")
    got = {}
    for lg in SIZES:
        cfg = gvamd.SearchConfig.of(wx=w, wy=w, wt=wt, yaw_step=YAW_STEP, stride=stride, min_points=100, block_log2=lg)
        us, got_r, got_s, line = _search_line(gvamd, hip, h, cfg, n, warmup, rec, stats)
        got[lg] = (cfg, got_r, got_s)
        say(line + f" | best shift ({int(got_r['best_t'])}, {int(got_r['best_j'])}, {int(got_r['best_i'])})")
    assert len({np.asarray(r).tobytes() for _, r, _ in got.values()}) == 1, "the record depends on S"
    cfg, got_r, got_s = min(got.values(), key=lambda v: int(v[2]["n_scored"]))   # the twin at the S that prunes best
    work = int(got_s["n_scored"]) * int(got_r["n_used"])
    if twin and work > TWIN_LIMIT:
        say(f"  the alternative at S {1 << cfg.block_log2}: skipped, {work:.2e} cost reads in the twin's fine pass alone (limit {TWIN_LIMIT:.0e})")
    elif twin:
        t0 = time.perf_counter()
        down = h.costmap()
        t1 = time.perf_counter()
        want_r, want_s = gvamd.match_search_host(gx, gy, res, down, x, y, z, tfs["base_lidar"], cfg, GUESS)
        t2 = time.perf_counter()
        same = np.asarray(want_r).tobytes() == np.asarray(got_r).tobytes() and np.asarray(want_s).tobytes() == np.asarray(got_s).tobytes()
        say(f"  the alternative at S {1 << cfg.block_log2}: costmap download {(t1 - t0) * 1e3:7.2f} ms + gv_match_search_host on one core "
            f"{(t2 - t1) * 1e3:9.1f} ms, record and stats {'equal' if same else 'DIFFER'}")
    pr.close()
    ps.close()
    h.close()
    return lines


def kernel_times(trace_dir):
    d = common.kernel_durations(trace_dir, KERNELS)
    return [f"{k}: {len(v)} dispatches, mean {np.mean(v):9.2f} us, min {np.min(v):9.2f} us, max {np.max(v):9.2f} us"
            for k, v in d.items() if v]


def resources():
    import kernel_resources as kr
    with tempfile.TemporaryDirectory() as tmp:
        _, text = kr.compile_file("gv_search.hip", tmp)
    rows = kr.parse_remarks(text)
    out = ["gv_search.hip, device-only compile with the library's flags for gfx950 (the compiler's",
           "-Rpass-analysis=kernel-resource-usage remarks, tools/kernel_resources.compile_file / parse_remarks)", "",
           f"{'kernel':44s} VGPRs  SGPRs  scratch [bytes/lane]  SGPR spill  VGPR spill  LDS [bytes/block]  waves/SIMD"]
    for name in sorted(rows):
        r = rows[name]
        short = name[name.index("k_search"):] if "k_search" in name else name
        out.append(f"{short[:44]:44s} {r.get('vgprs', -1):5d}  {r.get('sgprs', -1):5d}  {r.get('scratch', -1):20d}  {r.get('sgpr_spill', -1):10d}  "
                   f"{r.get('vgpr_spill', -1):10d}  {r.get('lds', -1):17d}  {r.get('waves', -1):10d}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-twin", action="store_true", help="skip the download and gv_match_search_host at the wide shape")
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace run of this script: print kernel times")
    ap.add_argument("--resources", default=None, help="write the register account of gv_search.hip to this file (no GPU)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.resources:
        lines = resources()
        print("\n".join(lines), flush=True)
        with open(a.resources, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    if a.trace:
        lines = ["per kernel (rocprofv3 --kernel-trace of the same script with --no-twin, every shape and S together):"] + kernel_times(a.trace)
        print("\n".join(lines), flush=True)
    else:
        head = "tools/match_search_time.py: scene_with_objects on 2000 x 2000 cells at 0.1 m, P1, yaw step %g, guess %s:" % (YAW_STEP, GUESS)
        print(head, flush=True)
        lines = [head] + run(a.calls, a.warmup, not a.no_twin)
    if a.out:
        common.append_out(a.out, lines)


if __name__ == "__main__":
    main()
