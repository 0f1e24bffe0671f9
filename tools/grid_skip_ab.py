"""A/B of two library builds for the grid pass that writes only what changed (GV_GRID_SKIP): the parent
build against this one, and this one with GV_GRID_SKIP=0.  Builds are chosen with GV_LIB_AB, as in tools/lib_ab.py;
every GPU step is a process of its own under `timeout -k 10`, and the first step that fails ends the run.

  python3 tools/grid_skip_ab.py --parent tools/_ab/parent.so [--new shipped] [--out profiles/x5/grid_skip.txt]
                                [--sections identity,headline,fresh,mixed,stats,pmc,full]

  identity  bench.py --dump-outputs on parent / new / new GV_GRID_SKIP=0: the six arrays must be equal
  headline  bench.py and bench.py --plain --min-reps 15, parent and new alternating, --runs each
  fresh     reset + time_frame_stages(3), 20 times: the grid pass when every row changes
  mixed     pipelined frame on the lidar-like cloud and on two alternating clouds, with the share of tile rows written
  stats     rocprofv3 --kernel-trace --stats, serial and pipelined, both builds (csv beside --out)
  pmc       WRITE_SIZE / FETCH_SIZE / SQ_INSTS_VALU of k_finalize_tiles per dispatch, counters in runs of their own
  full      bench.py --full --no-cpu-baseline on both builds: its PMC figures, lidar_like and with_h2d legs
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCPROF = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
BENCH = os.path.join(ROOT, "bench.py")
OUT = None


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def env_of(lib, skip=None, extra=None):
    env = dict(os.environ)
    env.pop("GV_GRID_SKIP", None)
    env.pop("GV_LIB_AB", None)
    if lib != "shipped":
        env["GV_LIB_AB"] = os.path.abspath(lib)
    if skip is not None:
        env["GV_GRID_SKIP"] = skip
    env.update(extra or {})
    return env


def gpu_step(cmd, env, limit, what):
    """one GPU process under its own time limit; anything but exit 0 ends the whole run"""
    p = subprocess.run(["timeout", "-k", "10", str(limit), *cmd], env=env, cwd="/tmp", stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        say(f"FAILED ({p.returncode}): {what}\n{p.stderr[-1500:]}")
        sys.exit(1)
    return p.stdout


def bench(args, env, limit=300):
    out = gpu_step([sys.executable, BENCH, "--gpus", "1", *args], env, limit, "bench.py " + " ".join(args))
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def mmm(v):
    return f"median {statistics.median(v):.4f} min {min(v):.4f} max {max(v):.4f} (n={len(v)})"


# ------------------------------------------------------------------------------------------------ children --
def _handle(cloud="uniform", seed_extra=0):
    sys.path.insert(0, os.path.join(ROOT, "grid-vision_amd"))
    import gvamd
    from gvamd import synth
    g = synth.CONFIGS[3]["grid"]
    tfs = synth.transforms(True)
    fn = synth.cloud_lidar_like if cloud == "lidar" else synth.cloud_uniform
    x, y, z, _ = fn(3, seed_extra=seed_extra)
    h = gvamd.GridVisionHIP(g.grid_x, g.grid_y, g.resolution)
    h.set_transforms(tfs["cam_lidar"], tfs["base_cam"], tfs["base_lidar"])
    h.upload_xyz(x, y, z)
    h.set_detections(gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH | gvamd.FRAME_BBOX_TEST, bboxes=synth.detections(3),
                     poses=synth.lshape_poses(3))
    return gvamd, synth, h, (x, y, z)


def _rows_written(h, before, after):
    """share of the tile rows (64 cells of a row) in which a log-odds value changed: what the pass writes"""
    import numpy as np
    same = (before.view(np.uint32) == after.view(np.uint32)).reshape(h.ny, h.nx)
    pad = (-h.nx) % 64
    rows = np.pad(same, ((0, 0), (0, pad)), constant_values=True).reshape(h.ny, -1, 64).all(axis=2)
    return 1.0 - float(rows.mean())


def child_fresh():
    _, _, h, _ = _handle()
    h.enqueue_frame()
    h.synchronize()
    fin = []
    for _ in range(20):
        h.reset()
        fin.append(h.time_frame_stages(3)["finalize"] * 1e3)
    print("RESULT " + json.dumps(fin))
    h.close()


def child_mixed():
    import time
    import numpy as np
    kind = os.environ["AB_KIND"]
    gvamd, synth, h, c0 = _handle("lidar" if kind == "lidar" else "uniform")
    clouds = [c0]
    if kind == "alternating":
        x, y, z, _ = synth.cloud_uniform(3, seed_extra=1)
        clouds.append((x, y, z))
    pins = []
    for c in clouds:
        n = len(c[0])
        p = gvamd.PinnedF32(3 * n)
        p.array[:n], p.array[n:2 * n], p.array[2 * n:] = c
        pins.append((p, n))

    def one(f):
        if len(clouds) > 1:
            p, n = pins[f % len(pins)]
            h.upload_xyz_async(p.array[:n], p.array[n:2 * n], p.array[2 * n:])
        h.enqueue_frame()

    for f in range(40):
        one(f)
    h.synchronize()
    share = []
    for f in range(4):
        before = h.log_odds()
        one(f)
        h.synchronize()
        share.append(_rows_written(h, before, h.log_odds()))
    reps = []
    steps = 200
    for _ in range(9):
        t0 = time.perf_counter()
        for f in range(steps):
            one(f)
        h.synchronize()
        reps.append((time.perf_counter() - t0) / steps * 1e6)
    print("RESULT " + json.dumps({"us_per_frame": reps, "rows_written": share}))
    h.close()
    for p, _ in pins:
        p.close()


def run_child(name, env, limit=200):
    out = gpu_step([sys.executable, os.path.abspath(__file__)], dict(env, AB_CHILD=name), limit, f"child {name}")
    return json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:])


# ------------------------------------------------------------------------------------------------ sections --
def sec_identity(a, builds):
    import numpy as np
    say("\n== identity: bench.py --dump-outputs, default steps and warm-up")
    dirs = {}
    for tag, env in builds.items():
        d = os.path.join(a.work, "dump_" + tag)
        shutil.rmtree(d, ignore_errors=True)
        bench(["--dump-outputs", d], env)
        dirs[tag] = d
    names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(dirs["parent"], "*.npy")))
    ok = len(names) == 6
    for n in names:
        arrs = [np.load(os.path.join(d, n)) for d in dirs.values()]
        eq = all(np.array_equal(arrs[0], x, equal_nan=True) and arrs[0].tobytes() == x.tobytes() for x in arrs[1:])
        ok &= eq
        say(f"  {n:20s} {arrs[0].size:8d} values  {'equal' if eq else 'DIFFERENT'} across {', '.join(dirs)}")
    say("  identity:", "holds" if ok else "BROKEN")
    if not ok:
        sys.exit(1)


def sec_headline(a, builds):
    for title, args in (("bench.py (one region of 200 steps)", []), ("bench.py --plain --min-reps 15", ["--plain", "--min-reps", "15"])):
        say(f"\n== headline: {title}, parent and new alternating, ms_per_step")
        v = {"parent": [], "new": []}
        for r in range(a.runs):
            for tag in ("parent", "new"):
                v[tag].append(bench(args, builds[tag])["ms_per_step"])
        for tag in v:
            say(f"  {tag:7s} {mmm(v[tag])}   runs: " + " ".join(f"{x:.4f}" for x in v[tag]))
        gain = (statistics.median(v["parent"]) - statistics.median(v["new"])) * 1e3
        say(f"  median gain {gain:.2f} us per frame; slowest new {max(v['new']):.4f} vs fastest parent {min(v['parent']):.4f} ms")


def sec_fresh(a, builds):
    say("\n== nothing saturated: reset + time_frame_stages(3), 20 times; grid pass (finalize) us")
    for tag, env in builds.items():
        fin = run_child("fresh", env)
        say(f"  {tag:12s} {mmm(fin)}")


def sec_mixed(a, builds):
    for kind in ("lidar", "alternating"):
        say(f"\n== mixed: pipelined frame, {kind} cloud(s) at config-3 size, us per frame (9 x 200 frames"
            + (", a cloud upload per frame" if kind == "alternating" else "") + ")")
        for tag, env in builds.items():
            r = run_child("mixed", dict(env, AB_KIND=kind))
            say(f"  {tag:12s} {mmm(r['us_per_frame'])}   tile rows written per frame: "
                + " ".join(f"{s:.3f}" for s in r["rows_written"]))


def sec_stats(a, builds):
    say("\n== rocprofv3 --kernel-trace --stats (bench.py --plain --steps 100 --warmup 30)")
    for tag in ("parent", "new"):
        for mode, pe in (("serial", {"GV_PIPELINE": "0"}), ("pipelined", {})):
            d = os.path.join(a.work, f"stats_{tag}_{mode}")
            shutil.rmtree(d, ignore_errors=True)
            gpu_step([ROCPROF, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, BENCH,
                      "--plain", "--steps", "100", "--warmup", "30"], dict(builds[tag], TMPDIR="/tmp", **pe), 250,
                     f"kernel stats {tag} {mode}")
            src = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if src:
                dst = os.path.join(os.path.dirname(OUT), f"{tag}_{mode}_kernel_stats.csv")
                shutil.copy(src[0], dst)
                for r in csv.DictReader(open(dst)):
                    if "k_finalize_tiles" in r["Name"]:
                        say(f"  {tag:7s} {mode:9s} k_finalize_tiles: calls {r['Calls']} average {float(r['AverageNs']) / 1e3:.2f} us "
                            f"({r['Percentage']} % of kernel time)")


def sec_pmc(a, builds):
    say("\n== PMC of k_finalize_tiles (serial frames, bench.py --steps 10 --warmup 30, one counter group per run):\n"
        "   mean over the last 10 dispatches (saturated) and over the first 3 (every row changes)")
    for tag in ("parent", "new"):
        line = []
        for grp in ("WRITE_SIZE", "FETCH_SIZE", "SQ_INSTS_VALU"):
            d = os.path.join(a.work, f"pmc_{tag}_{grp}")
            shutil.rmtree(d, ignore_errors=True)
            gpu_step([ROCPROF, "--pmc", grp, "--output-format", "csv", "-d", d, "--", sys.executable, BENCH,
                      "--steps", "10", "--warmup", "30"],
                     dict(builds[tag], GV_PIPELINE="0", TMPDIR="/tmp"), 250, f"pmc {tag} {grp}")
            rows = []
            for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                for r in csv.DictReader(open(f)):
                    if "k_finalize_tiles" in r["Kernel_Name"] and r["Counter_Name"] == grp:
                        rows.append((int(r["Dispatch_Id"]), float(r["Counter_Value"])))
            vals = [v for _, v in sorted(rows)]
            scale = {"WRITE_SIZE": 1024 / 1e6, "FETCH_SIZE": 2 * 1024 / 1e6, "SQ_INSTS_VALU": 1e-6}[grp]
            unit = "M wave-instr" if grp == "SQ_INSTS_VALU" else "MB"
            if len(vals) >= 13:
                line.append(f"{grp} first3 {statistics.mean(vals[:3]) * scale:.2f} last10 {statistics.mean(vals[-10:]) * scale:.2f} {unit}"
                            f" ({len(vals)} dispatches)")
        say(f"  {tag:7s} " + "; ".join(line))


def sec_full(a, builds):
    say("\n== bench.py --full --no-cpu-baseline: its own PMC child passes (13 frames from reset) and the mixed legs")
    for tag in ("parent", "new"):
        j = bench(["--full", "--no-cpu-baseline"], builds[tag], limit=900)
        json.dump(j, open(os.path.join(a.work, f"full_{tag}.json"), "w"))
        k = [e for e in j.get("kernels", []) if e["stage"] == "finalize"]
        w = j.get("with_h2d", {})
        ll = j.get("lidar_like", {})
        say(f"  {tag:7s} ms_per_step {j['ms_per_step']:.4f}; finalize write_bytes {k[0].get('write_bytes') if k else None} "
            f"fetch_bytes {k[0].get('fetch_bytes') if k else None} stage {k[0]['ms'] * 1e3 if k else 0:.1f} us")
        say(f"          lidar_like: " + json.dumps({q: ll.get(q) for q in ("value", "ms_per_step", "repetitions") if q in ll}))
        say(f"          with_h2d: " + json.dumps({q: v for q, v in w.items() if isinstance(v, (int, float))}))


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--new", default="shipped")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "x5", "grid_skip.txt"))
    ap.add_argument("--work", default="/tmp/grid_skip_ab")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sections", default="identity,headline,fresh,mixed,stats,pmc,full")
    a = ap.parse_args()
    OUT = os.path.abspath(a.out)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    a.work = os.path.abspath(a.work)
    os.makedirs(a.work, exist_ok=True)
    builds = {"parent": env_of(a.parent), "new": env_of(a.new), "new_dense": env_of(a.new, skip="0")}
    say(f"grid_skip_ab: parent {a.parent}, new {a.new}; sections {a.sections}")
    for s in a.sections.split(","):
        {"identity": sec_identity, "headline": sec_headline, "fresh": sec_fresh, "mixed": sec_mixed, "stats": sec_stats,
         "pmc": sec_pmc, "full": sec_full}[s](a, builds)


if __name__ == "__main__":
    child = os.environ.get("AB_CHILD")
    if child:
        {"fresh": child_fresh, "mixed": child_mixed}[child]()
    else:
        main()
