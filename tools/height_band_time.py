"""Cost of the [EXTENSION] X4 height band: scene_with_objects at 1 M points on the 2000 x 2000 grid (config 3), the
headline frame flags (bin + ray march + bbox test), band off against the band with clearing.  Per band: the pipelined
frame (gv_time_frames, K frames after a warm-up) and the per-kernel stage times (gv_time_frame_stages: partition, tile
pass, sector stage, grid pass from their own dispatch packets), each the median of --reps runs, and how the band
classified the points.  Prints one block; --out FILE writes it there too.

python3 tools/height_band_time.py [--frames 200] [--reps 5] [--band both|off|on] [--out profiles/x4/height_band.txt]
(--band off / on: one band per process, for a `rocprofv3 --kernel-trace --stats` run of each)"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "grid-vision_amd"))

import gvamd  # noqa: E402
from gvamd import synth  # noqa: E402

BANDS = {"off": None, "on (0.3 / 2.5 m, clears)": (0.3, 2.5, True)}


def _base_z(tfs, x, y, z):
    """fp32 base-frame z as the partition pass computes it (only used for the class counts printed here)"""
    q = synth._quat_to_matrix(tfs["base_lidar"][:4]).astype(np.float32)
    t = np.float32(tfs["base_lidar"][6])
    return q[2, 0] * x + (q[2, 1] * y + (q[2, 2] * z + t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--band", choices=("both", "off", "on"), default="both")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g = synth.CONFIGS[3]["grid"]
    tfs = synth.transforms(False)
    x, y, z, boxes = synth.scene_with_objects(tfs)
    bz = _base_z(tfs, x, y, z)
    flags = gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH | gvamd.FRAME_BBOX_TEST
    lines = [f"tools/height_band_time.py: scene_with_objects, {len(x)} points, {g.nx} x {g.ny} cells, "
             f"flags bin | raymarch | bbox test, {len(boxes)} boxes, K = {a.frames} frames, median of {a.reps} runs"]
    res = {}
    for name, band in BANDS.items():
        if a.band != "both" and (band is None) != (a.band == "off"):
            continue
        h = gvamd.GridVisionHIP(g.grid_x, g.grid_y, g.resolution)
        h.set_transforms(tfs["cam_lidar"], tfs["base_cam"], tfs["base_lidar"])
        if band is not None:
            h.set_height_band(*band)
        h.upload_xyz(x, y, z)
        h.set_detections(flags, bboxes=boxes)
        h.time_frames(20)
        frame = [h.time_frames(a.frames) / a.frames * 1e3 for _ in range(a.reps)]
        stages = [h.time_frame_stages(50) for _ in range(a.reps)]
        h.close()
        st = {k: float(np.median([s[k] for s in stages])) * 1e3 for k in stages[0]}
        res[name] = (float(np.median(frame)), st)
        if band is None:
            cls = f"{len(x)} obstacles"
        else:
            gnd, above = int(np.count_nonzero(bz < band[0])), int(np.count_nonzero(bz > band[1]))
            cls = f"{len(x) - gnd - above} obstacles, {gnd} ground returns (ray ends), {above} above the band"
        lines.append(f"band {name}: {cls}")
        lines.append(f"  pipelined frame {res[name][0]:8.2f} us   (runs: {', '.join(f'{v:.2f}' for v in frame)})")
        lines.append("  stages (us): " + ", ".join(f"{k} {v:.2f}" for k, v in st.items()))
    off, on = res.get("off"), res.get("on (0.3 / 2.5 m, clears)")
    if off and on:
        lines.append(f"ratio on / off: pipelined frame {on[0] / off[0]:.3f}; "
                     + ", ".join(f"{k} {on[1][k] / off[1][k]:.3f}" for k in off[1] if off[1][k] > 0))
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
