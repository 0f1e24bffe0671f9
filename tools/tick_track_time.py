"""[EXTENSION] X15 what it costs and saves to feed the tracker from the tick's list on the device, on the 1 M-point,
40-box scene of tools/tick_run.py, both pose branches.  Host clock around work that ends in a device synchronise, per
tick, N ticks per block; the variants of a comparison alternate block by block in one process (R blocks each), and the
median, the least and the largest block are printed, so the spread stands beside every difference.

python3 tools/tick_track_time.py [--ticks N] [--blocks R] [--out FILE]
  paths   host path (what the parent does): gv_tick_enqueue, gv_tick_wait, gv_track_update_async with the first 128
          poses as host detections and GV_TRACK_FEED_DYNAMIC, gv_synchronize;
          device path: gv_tick_enqueue with GV_TICK_KEEP_DETS, gv_track_update_async with GV_TRACK_TICK_DETS and the
          feed, gv_tick_wait, gv_synchronize (the update sits behind the tick's event);
  tick    gv_tick alone without and with GV_TICK_KEEP_DETS.
python3 tools/tick_track_time.py ab a.so b.so ... [--rounds Q]
  the unflagged gv_tick of other builds of the library (the parent's, built into tools/_ab/), every build in a process
  of its own as tools/lib_ab.py runs them (GV_LIB_AB), Q rounds over the list so that the builds alternate."""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "grid-vision_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import planner_time_common as common  # noqa: E402


def setup(branch):
    import gvamd
    from gvamd import synth
    g = synth.CONFIGS[3]["grid"]
    tfs = synth.transforms(True)
    x, y, z, b = synth.scene_with_objects(tfs)
    h = gvamd.GridVisionHIP(g.grid_x, g.grid_y, g.resolution)
    h.set_transforms(tfs["cam_lidar"], tfs["base_cam"], tfs["base_lidar"])
    h.upload_xyz(x, y, z)
    _, dy = gvamd.filter_bboxes(b)
    pin = gvamd.PinnedI8(h.G)
    kw = dict(k_near=4, vision=branch == "vision", net=synth.network_outputs(len(dy)) if branch == "vision" else None, grid_out=pin.array)
    return gvamd, h, b, kw, pin


def blocks(variants, ticks, n_blocks, warmup=5):
    """{name: [us per tick of every block]}, the variants alternating block by block"""
    for f in variants.values():
        for _ in range(warmup):
            f()
    out = {k: [] for k in variants}
    for _ in range(n_blocks):
        for name, f in variants.items():
            t0 = time.perf_counter()
            for _ in range(ticks):
                f()
            out[name].append((time.perf_counter() - t0) / ticks * 1e6)
    return out


def fmt(v):
    return f"median {np.median(v):8.1f} us (least {min(v):8.1f}, largest {max(v):8.1f})"


def run(ticks, n_blocks):
    lines = []
    for branch in ("pca", "vision"):
        gvamd, h, b, kw, pin = setup(branch)
        h.set_track_config(gvamd.TrackConfig.of(gate=2.0))
        h.set_dyn_config(gvamd.DynConfig.of())

        def host_path():
            h.tick_enqueue(b, **kw)
            r = h.tick_wait()
            h.track_update_async(np.ascontiguousarray(r["poses"][:128]), 0.05, feed=True)
            h.synchronize()

        def device_path():
            h.tick_enqueue(b, keep_dets=True, **kw)
            h.track_update_async(None, 0.05, feed=True, from_tick=True)
            h.tick_wait()
            h.synchronize()

        def tick_plain():
            h.tick(b, **kw)

        def tick_keep():
            h.tick(b, keep_dets=True, **kw)

        # the two paths leave the same tracks (PCA: by bytes; vision: the quaternions within DESIGN 4.18's bound)
        h.set_tracks(None, 1)
        host_path()
        ta = h.get_tracks()[0]
        h.set_tracks(None, 1)
        device_path()
        tb = h.get_tracks()[0]
        same = len(ta) == len(tb) and all(ta[k].tobytes() == tb[k].tobytes() for k in ta.dtype.names if k not in ("qx", "qy", "qz", "qw"))
        p = blocks({"host": host_path, "device": device_path}, ticks, n_blocks)
        t = blocks({"plain": tick_plain, "keep": tick_keep}, ticks, n_blocks)
        lines += [f"{branch}: {len(ta)} tracks, the two paths {'agree' if same else 'DISAGREE'}; {n_blocks} blocks of {ticks} ticks each, alternating",
                  f"  tick + wait + host update(feed) + synchronise    {fmt(p['host'])}",
                  f"  tick(keep) + update(from tick, feed) + one wait  {fmt(p['device'])}",
                  f"  tick alone, without the flag                     {fmt(t['plain'])}",
                  f"  tick alone, with GV_TICK_KEEP_DETS               {fmt(t['keep'])}"]
        for ln in lines[-5:]:
            print(ln, flush=True)
        pin.close()
        h.close()
    return lines


def ab_child(ticks, n_blocks):
    for branch in ("pca", "vision"):
        gvamd, h, b, kw, pin = setup(branch)
        t = blocks({"plain": lambda: h.tick(b, **kw)}, ticks, n_blocks)
        print(f"{os.path.basename(os.environ.get('GV_LIB_AB', 'shipped')):24s} {branch:6s} unflagged tick {fmt(t['plain'])}", flush=True)
        pin.close()
        h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="paths")
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if os.environ.get("AB_CHILD"):
        ab_child(a.ticks, a.blocks)
    elif a.mode == "ab":
        for _ in range(a.rounds):
            for lib in a.libs:
                env = dict(os.environ, AB_CHILD="1")
                if lib != "shipped":
                    env["GV_LIB_AB"] = os.path.abspath(lib)
                subprocess.run([sys.executable, os.path.abspath(__file__), "--ticks", str(a.ticks), "--blocks", str(a.blocks)], env=env, check=False)
    else:
        lines = run(a.ticks, a.blocks)
        if a.out:
            common.append_out(a.out, lines)


if __name__ == "__main__":
    main()
