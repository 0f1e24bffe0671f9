#!/usr/bin/env python3
"""bench.py -- frames/sec of the grid-vision per-frame hot path on MI355X.

A "step" is one contract-complete frame: points pass (transform + cell index + ray ends + bbox test),
int32 hit counts per cell, Bresenham free-space ray stage, and the grid pass (decay, rectangles,
hit/miss, clamp, sigmoid, int8 pack) over one synthetic cloud that is already resident in HBM when the
timed region starts.

N=1   BASELINE.json configs[2]: 1M-point cloud, 2000x2000 @ 0.1 m grid, 50 bboxes + 50 poses.
N>1   configs[3]: one independent 1M-point frame stream per GPU (no data-path collective;
      torch.distributed only for the barrier and the max-over-ranks).  Run plainly (no torchrun
      environment) with --gpus N, the script launches the N ranks itself; it never reports fewer GPUs
      than it was asked for.

Prints ONE JSON line on rank 0.  A plain run sets up, warms up (--warmup W frames), times ONE region of
exactly --steps K frames, optionally writes what the last frame produced (--dump-outputs DIR) and prints the
headline.  With --full the line also carries what takes runs of its own: the K-step region repeated
(median reported), per-kernel times and rooflines, and (N=1) `with_h2d` (a fresh cloud + fresh detections
every frame, host->device copy included), `tick`, `pca_path`, `lidar_like`, `beyond_l3` (config 5 on one
GPU: working set past the 256 MiB Infinity Cache), PMC traffic measured in this very run (rocprofv3 child
passes) and the CPU baselines.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import shutil
import socket
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "grid-vision_amd"))

import numpy as np  # noqa: E402

HBM_PEAK_GBPS = 8000.0            # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
# VALU issue peak (MI355X_MICROARCH.md: 256 CUs x 4 SIMD-32, a wave64 VALU instruction issues over 2
# cycles with >= 2 waves per SIMD, 2.4 GHz): 1024 x 2.4e9 / 2 wave-instructions per second
VALU_PEAK_GWIPS = 1024 * 2.4 / 2.0
PCIE_SPEC_GBPS = 63.0             # PCIe Gen5 x16 (MI355X_MICROARCH.md)

KERNEL_OF = {"detections": "k_rects_from_poses", "points": "k_bin_partition", "ray_ends": "k_bin_tiles",
             "ray_march": "k_ray_sectors", "finalize": "k_finalize_tiles"}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--config", type=int, default=0, help="0 = 3 at N=1 / 4 at N>1; 5 = one sharded 10M-point frame")
    ap.add_argument("--cloud", choices=["uniform", "lidar"], default="uniform")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: repetitions, stage times, rooflines, PMC passes, extra legs, CPU baselines")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step produced as DIR/<name>.npy (float32)")
    ap.add_argument("--plain", action="store_true",
                    help="repetitions of the timed region + stage times only, even with --full (profiling runs)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-pmc", action="store_true", help="skip the rocprofv3 child passes (traffic = null)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--min-reps", type=int, default=5,
                    help="with --full or --plain: repetitions of the K-step timed region (median reported)")
    ap.add_argument("--force-sharded", action="store_true",
                    help="config 5 through the sharded (RCCL) frame even with one rank: rehearses the code path on one GPU")
    ap.add_argument("--slice-of", type=int, default=0,
                    help="(PMC child passes) with --force-sharded on one rank: keep only the first 1 / W of the points, what a rank of a W-rank job bins")
    ap.add_argument("--rehearsal", action="store_true",
                    help="allow more ranks than GPUs (ranks share devices, gloo barrier): reported as rehearsal")
    return ap.parse_args()


# --------------------------------------------------------------------------- CPU baselines --
def cpu_baseline(config, cloud_fn, tfs, bboxes, poses, budget_s):
    """The CPU oracle (a port: the reference itself cannot be built here) timed on this box's host
    cores, single thread like the reference node, on a bounded sample: whole frames of the same
    workload until ~budget_s have elapsed."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as ol
    from gvamd import synth
    g = synth.CONFIGS[config]["grid"]
    og = ol.OGrid(g.grid_x, g.grid_y, g.resolution)
    x, y, z, _ = cloud_fn(config)
    m_base = ol.tf_to_matrix4f(tfs["base_lidar"])
    m_cam = ol.tf_to_matrix4f(tfs["cam_lidar"])
    K = ol.set_intrinsic(synth.FX, synth.FY, synth.CX, synth.CY)

    def frame():
        hits, _ = og.bin_points(m_base, x, y, z)
        miss, _ = og.raymarch(m_base, x, y, z, dedupe=False)   # per-point march, like a LineIterator user
        cx, cy, cz = ol.transform_cloud(m_cam, x, y, z)
        ol.extract_cloud_per_bbox(K, cx, cy, cz, bboxes, synth.IMG_W, synth.IMG_H)
        og.frame_update(poses, hits, miss)
        og.to_occupancy_grid()

    frame()   # warm-up (page-in)
    t0 = time.perf_counter()
    n = 0
    while True:
        frame()
        n += 1
        if time.perf_counter() - t0 >= budget_s or n >= 50:
            break
    dt = time.perf_counter() - t0
    return {"value": n / dt, "unit": "frames/s", "cores": 1, "kind": "port",
            "sample": f"{n} whole frames of the same workload (per-point Bresenham, 1M rays, no de-duplication), {dt:.1f} s"}


def cpu_baseline_all_cores(config, cloud_fn, tfs, bboxes, poses, budget_s):
    """the same oracle on every host core.  The points are split into one chunk per
    thread (ctypes releases the GIL inside the C calls); each thread bins, ray-marches and bbox-tests
    its chunk into private grids, which are then summed / OR-ed and finalised once."""
    from concurrent.futures import ThreadPoolExecutor
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as ol
    from gvamd import synth
    cores = max(1, min(len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1), 32))
    g = synth.CONFIGS[config]["grid"]
    og = ol.OGrid(g.grid_x, g.grid_y, g.resolution)
    workers = [ol.OGrid(g.grid_x, g.grid_y, g.resolution) for _ in range(cores)]   # geometry holders
    x, y, z, _ = cloud_fn(config)
    m_base = ol.tf_to_matrix4f(tfs["base_lidar"])
    m_cam = ol.tf_to_matrix4f(tfs["cam_lidar"])
    K = ol.set_intrinsic(synth.FX, synth.FY, synth.CX, synth.CY)
    cuts = [len(x) * k // cores for k in range(cores + 1)]

    def chunk(k):
        sl = slice(cuts[k], cuts[k + 1])
        w = workers[k]
        hits, _ = w.bin_points(m_base, x[sl], y[sl], z[sl])
        miss, _ = w.raymarch(m_base, x[sl], y[sl], z[sl], dedupe=False)
        cx, cy, cz = ol.transform_cloud(m_cam, x[sl], y[sl], z[sl])
        ol.extract_cloud_per_bbox(K, cx, cy, cz, bboxes, synth.IMG_W, synth.IMG_H)
        return hits, miss

    pool = ThreadPoolExecutor(cores)

    def frame():
        parts = list(pool.map(chunk, range(cores)))
        hits, miss = parts[0]
        for h2, m2 in parts[1:]:
            hits = hits + h2
            miss = np.maximum(miss, m2)
        og.frame_update(poses, hits, miss)
        og.to_occupancy_grid()

    frame()
    t0 = time.perf_counter()
    n = 0
    while True:
        frame()
        n += 1
        if time.perf_counter() - t0 >= budget_s or n >= 100:
            break
    dt = time.perf_counter() - t0
    pool.shutdown()
    return {"value": n / dt, "unit": "frames/s", "cores": cores, "kind": "port",
            "sample": f"{n} whole frames, points split over {cores} threads with private grids, reduced and finalised once, {dt:.1f} s"}


def measured_copy_rate(torch):
    """device-to-device copy rate of this box (read + write bytes / time): the second peak of SURVEY 8(d)"""
    n = 256 << 20
    a_ = torch.empty(n, dtype=torch.uint8, device="cuda")
    b_ = torch.empty(n, dtype=torch.uint8, device="cuda")
    for _ in range(3):
        b_.copy_(a_)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        b_.copy_(a_)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 10
    del a_, b_
    return 2.0 * n / (ms * 1e-3) / 1e9


# ------------------------------------------------------------------------- extra GPU legs --
def timed_frames(h, steps, warmup):
    for _ in range(warmup):
        h.enqueue_frame()
    h.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        h.enqueue_frame()
    h.synchronize()
    return time.perf_counter() - t0


class DpmSampler:
    """Clock / link state of THIS GPU (sysfs entry found through its PCI bus id: the host's other GPUs are
    visible too) sampled by a thread while a leg runs: transitions of (sclk, socclk, fclk, PCIe link) with
    their time.  Evidence for the time structure of the streamed legs (profiles/r03/h2d_notes.md)."""
    FILES = ("pp_dpm_sclk", "pp_dpm_socclk", "pp_dpm_fclk", "current_link_speed", "current_link_width")

    def __init__(self, device=0, period=0.01):
        import ctypes
        import threading
        self.dir = None
        try:
            hip = ctypes.CDLL("libamdhip64.so")
            buf = ctypes.create_string_buffer(64)
            if hip.hipDeviceGetPCIBusId(buf, 64, device) == 0:
                d = "/sys/bus/pci/devices/" + buf.value.decode().lower()
                if os.path.exists(os.path.join(d, "pp_dpm_sclk")):
                    self.dir = d
        except OSError:
            pass
        self.period, self.log, self._stop = period, [], False
        self.t0 = time.perf_counter()
        self._th = threading.Thread(target=self._run, daemon=True)

    def _read(self):
        st = []
        for f in self.FILES:
            try:
                txt = open(os.path.join(self.dir, f)).read()
            except OSError:
                st.append(None)
                continue
            if f.startswith("pp_dpm"):
                cur = [ln.split(":")[1].strip(" *") for ln in txt.splitlines() if ln.strip().endswith("*")]
                st.append(cur[0] if cur else None)
            else:
                st.append(txt.strip())
        return st

    def _run(self):
        last = None
        while not self._stop:
            st = self._read()
            # sclk moves in small steps while it ramps: log a change of >= 100 MHz or of anything else
            def mhz(v):
                try:
                    return int(v.lower().replace("mhz", ""))
                except (AttributeError, ValueError):
                    return -1
            if last is None or st[1:] != last[1:] or abs(mhz(st[0]) - mhz(last[0])) >= 100:
                self.log.append([round(time.perf_counter() - self.t0, 3)] + st)
                last = st
            time.sleep(self.period)

    def __enter__(self):
        if self.dir:
            self._th.start()
        return self

    def __exit__(self, *a):
        self._stop = True
        if self.dir:
            self._th.join()

    def mark(self):
        return round(time.perf_counter() - self.t0, 3)


def stream_frames(one, frames, chunk=50):
    """Enqueue `frames` streamed frames with no host wait; the host timestamp taken every `chunk` frames
    gives the device's period per chunk (gv_frame_enqueue blocks on the frame four back: the host runs at
    most four frames ahead of the device)."""
    series, t_prev = [], time.perf_counter()
    for f in range(frames):
        one(f)
        if (f + 1) % chunk == 0:
            t = time.perf_counter()
            series.append((t - t_prev) / chunk * 1e6)
            t_prev = t
    return series


def stream_until_stable(one, chunk=50, need=4, tol=0.03, max_frames=4000):
    """Warm-up that ends when the last `need` chunk periods agree within `tol` (the streamed frame has a
    slow start of box-dependent length, profiles/r03/h2d_notes.md) or after max_frames."""
    series, t_prev, f = [], time.perf_counter(), 0
    while f < max_frames:
        for _ in range(chunk):
            one(f)
            f += 1
        t = time.perf_counter()
        series.append((t - t_prev) / chunk * 1e6)
        t_prev = t
        last = series[-need:]
        if len(series) > need and max(last) <= min(last) * (1.0 + tol):
            break
    return series, f


def leg_with_h2d(gvamd, synth, g, tfs, config, flags, local_rank, steps):
    """host-to-device copy INCLUDED.  grid_vision_node.cpp:103-106,108-244: a new cloud and
    new detections arrive for every frame.  Six distinct clouds sit in pinned host memory; every frame
    does gv_cloud_upload_*_async + gv_frame_set_detections_async + gv_frame_enqueue with no host wait
    (three resident clouds in rotation, copy stream).  Sub-legs: SoA block (12 B/point), the same plus the
    packed grid back to the host every frame, PointCloud2 bytes with point_step 16 and 32, the copy alone,
    and the node's own operating point: one cloud every 50 ms, upload -> frame -> grid on the host."""
    n_sets = 6
    pins, dets, blocks = [], [], []
    for f in range(n_sets):
        x, y, z, _ = synth.cloud_uniform(config, seed_extra=100 + f)
        blk = gvamd.PinnedF32(3 * len(x))   # x | y | z back to back in one pinned block: one DMA per cloud
        n0 = len(x)
        blk.array[:n0], blk.array[n0:2 * n0], blk.array[2 * n0:] = x, y, z
        blocks.append(blk)
        pins.append((blk.array[:n0], blk.array[n0:2 * n0], blk.array[2 * n0:]))
        dets.append((synth.detections(config, seed_extra=f), synth.lshape_poses(config, seed_extra=f)))
    h = gvamd.GridVisionHIP(g.grid_x, g.grid_y, g.resolution, device=local_rank)
    h.set_transforms(tfs["cam_lidar"], tfs["base_cam"], tfs["base_lidar"])
    n = len(pins[0][0])
    G = h.G
    outs = [gvamd.PinnedF32((G + 3) // 4) for _ in range(2)]

    def one(f):
        px, py, pz = pins[f % n_sets]
        h.upload_xyz_async(px, py, pz)
        h.set_detections_async(flags, bboxes=dets[f % n_sets][0], poses=dets[f % n_sets][1])
        h.enqueue_frame()

    def one_pub(f):   # + publishOccupancyGrid (grid_vision_node.cpp:265-278): 4 MB device-to-host for every frame, written by
        one(f)        # a kernel on the public stream (gv_publish_grid_async): the copy engines stay with the uploads
        h.publish_grid_async(outs[f % 2].array.view("int8")[:G])

    def one_pub_unscheduled(f):   # round 3's form: a copy command on the public stream right behind the grid pass
        one(f)
        h.to_occupancy_grid_async(outs[f % 2].array.view("int8")[:G])

    def copy_only(f):   # the same loop with a frame that does next to nothing: the period is the copy engine's
        px, py, pz = pins[f % n_sets]
        h.upload_xyz_async(px, py, pz)
        h.set_detections_async(0)
        h.enqueue_frame()

    def timed(fn, frames):
        warm, nwarm = stream_until_stable(fn)
        h.synchronize()
        t0 = time.perf_counter()
        series = stream_frames(fn, frames)
        t_host = time.perf_counter() - t0
        h.synchronize()
        dt = time.perf_counter() - t0
        return {"frames_per_s": frames / dt, "us_per_frame": dt / frames * 1e6, "host_us_per_frame": t_host / frames * 1e6,
                "warmup_frames": nwarm, "warmup_series_us": [round(v, 1) for v in warm],
                "series_us": [round(v, 1) for v in series]}

    with DpmSampler(local_rank) as dpm:
        marks = {"soa_begin": dpm.mark()}
        soa = timed(one, steps)
        marks["pub_begin"] = dpm.mark()
        pub = timed(one_pub, max(150, steps // 2))
        pub_un = timed(one_pub_unscheduled, max(150, steps // 2))
        marks["copy_only_begin"] = dpm.mark()
        cpy = timed(copy_only, 200)
        marks["end"] = dpm.mark()
    res = {"value": soa["frames_per_s"], "unit": "frames/s", "ms_per_step": soa["us_per_frame"] * 1e-3, "steps": steps,
           "warmup_frames": soa["warmup_frames"], "warmup_series_us": soa["warmup_series_us"], "series_us": soa["series_us"],
           "host_us_per_frame": soa["host_us_per_frame"]}
    h2d_gbps = 12.0 * n / (cpy["us_per_frame"] * 1e-6) / 1e9
    res.update({"h2d_GBps_measured": h2d_gbps, "h2d_GBps_spec": PCIE_SPEC_GBPS,
                "copy_bound_frames_per_s": cpy["frames_per_s"], "frac_of_copy_bound": soa["frames_per_s"] / cpy["frames_per_s"],
                "copy_only_series_us": cpy["series_us"],
                "with_grid_download_frames_per_s": pub["frames_per_s"], "with_grid_download_series_us": pub["series_us"],
                "with_grid_download_frac_of_serial_copy_bound": pub["frames_per_s"] * cpy["us_per_frame"] * (1.0 + G / (12.0 * n)) * 1e-6,
                "with_grid_download_copy_command_frames_per_s": pub_un["frames_per_s"],
                "with_grid_download_copy_command_series_us": pub_un["series_us"],
                "dpm": {"columns": ["t_s", "sclk", "socclk", "fclk", "link_speed", "link_width"], "transitions": dpm.log[:60],
                        "marks_s": marks, "sysfs": dpm.dir}})

    # PointCloud2 wire format (grid_vision_node.cpp:103-106): interleaved points, de-interleaved on the device
    pc2 = {}
    for step_b in (16, 32):
        raws = []
        for f in range(3):
            r = gvamd.PinnedF32(n * step_b // 4)
            v = r.array.view(np.float32).reshape(n, step_b // 4)
            px, py, pz = pins[f]
            v[:, 0], v[:, 1], v[:, 2] = px, py, pz
            v[:, 3:] = 0.5   # intensity (+ ring / time padding for point_step 32)
            raws.append(r)

        def one_pc2(f, raws=raws, step_b=step_b):
            h.upload_pointcloud2_async(raws[f % 3].array.view(np.uint8), n, step_b, 0, 4, 8)
            h.set_detections_async(flags, bboxes=dets[f % n_sets][0], poses=dets[f % n_sets][1])
            h.enqueue_frame()
        r = timed(one_pc2, 200)
        pc2[f"point_step_{step_b}"] = {"frames_per_s": r["frames_per_s"], "us_per_frame": r["us_per_frame"],
                                       "h2d_GBps": step_b * n / (r["us_per_frame"] * 1e-6) / 1e9,
                                       "series_us": r["series_us"], "warmup_frames": r["warmup_frames"]}
        h.synchronize()
        for r_ in raws:
            r_.close()
    res["pointcloud2"] = pc2

    # the reference's operating point: a 50 ms wall timer (grid_vision_node.cpp:49-50); per tick one new cloud
    # (PointCloud2, point_step 16, :103-106), new detections, the frame, and the grid on the host (:265-278);
    # latency = host-observed upload call -> grid bytes in pinned host memory.  The device idles (and clocks
    # down) between ticks, which is what a 20 Hz caller sees.
    raw = gvamd.PinnedF32(n * 4)
    v = raw.array.view(np.float32).reshape(n, 4)
    v[:, 0], v[:, 1], v[:, 2], v[:, 3] = pins[0][0], pins[0][1], pins[0][2], 0.5
    lat_pc2, lat_soa = [], []
    period = 0.050
    t_next = time.perf_counter()
    for f in range(130):
        t_next += period
        while time.perf_counter() < t_next:
            time.sleep(0.0005)
        t0 = time.perf_counter()
        if f % 2 == 0:
            h.upload_pointcloud2_async(raw.array.view(np.uint8), n, 16, 0, 4, 8)
        else:
            px, py, pz = pins[f % n_sets]
            h.upload_xyz_async(px, py, pz)
        h.set_detections_async(flags, bboxes=dets[f % n_sets][0], poses=dets[f % n_sets][1])
        h.enqueue_frame()
        h.to_occupancy_grid_async(outs[f % 2].array.view("int8")[:G])
        h.synchronize()
        (lat_pc2 if f % 2 == 0 else lat_soa).append((time.perf_counter() - t0) * 1e3)
    def pct(a, q):
        a = sorted(a[5:])   # the first ticks include first-touch costs
        return a[min(len(a) - 1, int(q * len(a)))]
    res["latency_20hz"] = {"period_ms": 50.0, "frames": len(lat_pc2) + len(lat_soa) - 10,
                           "pointcloud2_step16_ms": {"p50": pct(lat_pc2, 0.5), "p99": pct(lat_pc2, 0.99), "max": max(lat_pc2[5:])},
                           "soa_ms": {"p50": pct(lat_soa, 0.5), "p99": pct(lat_soa, 0.99), "max": max(lat_soa[5:])},
                           "note": "one cloud every 50 ms (grid_vision_node.cpp:49-50): upload + detections + frame + 4 MB "
                                   "OccupancyGrid.data back in pinned host memory, host clock around the whole tick"}
    raw.close()
    for o in outs:
        o.close()
    h.close()
    pins = None
    for blk in blocks:
        blk.close()
    res["note"] = ("fresh 1M-point cloud (12 MB, one pinned host block, one DMA) + fresh detections every frame, async "
                   "ingest on a copy stream (three resident clouds), no host wait between frames; warm-up runs until four "
                   "consecutive 50-frame periods agree within 3 %; never the headline")
    return res


def leg_cloud(gvamd, synth, g, tfs, config, flags, bboxes, poses, local_rank, steps, cloud_fn, n=None):
    x, y, z, _ = cloud_fn(config) if n is None else cloud_fn(config, n)
    h = gvamd.GridVisionHIP(g.grid_x, g.grid_y, g.resolution, device=local_rank)
    h.set_transforms(tfs["cam_lidar"], tfs["base_cam"], tfs["base_lidar"])
    h.upload_xyz(x, y, z)
    h.set_detections(flags, bboxes=bboxes, poses=poses)
    # median of fifteen K-step regions behind 60 warm-up frames (a fresh handle: every buffer set of every lane is
    # touched for the first time), like the headline
    reps = [timed_frames(h, steps, 60 if r == 0 else 0) for r in range(15)]
    dt = float(np.median(reps))
    stages = h.time_frame_stages(10)
    h.close()
    return {"value": steps / dt, "unit": "frames/s", "ms_per_step": dt / steps * 1e3, "steps": steps, "stage_ms": stages,
            "ms_per_step_min": min(reps) / steps * 1e3, "ms_per_step_max": max(reps) / steps * 1e3, "points": len(x)}


class CpuTick:
    """The oracle's timerCallback from filterBBoxes on (grid_vision_node.cpp:153-244), single thread like the reference
    node: the CPU baseline beside the tick legs and the per-call figures of `pca_path`.  kind "port"; the radius filter is
    the oracle's cell-grid form (oracle/cloud_detections.c: identical keep flags; PCL answers the same query through a
    KD-tree, the all-pairs statement would take minutes on a 20 k-point box)."""

    def __init__(self, synth, g, tfs, x, y, z, b):
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle_lib as ol
        self.ol, self.synth, self.tfs = ol, synth, tfs
        self.og = ol.OGrid(g.grid_x, g.grid_y, g.resolution)
        self.x, self.y, self.z, self.b = x, y, z, b
        self.m_cam = ol.tf_to_matrix4f(tfs["cam_lidar"])
        self.K = ol.set_intrinsic(synth.FX, synth.FY, synth.CX, synth.CY)
        self.Kinv = ol.k_inverse(self.K)
        self.cam = ol.make_cam()
        self.ms = {}

    def _t(self, key, t0):
        self.ms[key] = self.ms.get(key, 0.0) + (time.perf_counter() - t0) * 1e3

    def knn(self, cx, cy, cz, st, k):
        ol = self.ol
        u, v, d = ol.project_points(self.K, cx, cy, cz)              # buildKDTree's projection (:8-33)
        dep, _ = ol.depth_for_bboxes(u, v, d, st, k)                 # exact kNN + upper median (:43-87)
        f = np.float32
        pts = [ol.tf_point(self.tfs["base_cam"], ol.pixel_to_3d(f(bb["x_min"] + ((bb["x_max"] - bb["x_min"]) / f(2.0))),
                                                                f(bb["y_min"] + ((bb["y_max"] - bb["y_min"]) / f(2.0))), dp, self.Kinv))
               for bb, dp in zip(st, dep)]
        return dep, pts

    def bbox_pose(self, cx, cy, cz):
        """computeBBoxPose (cloud_detections.cpp:300-321) on ALL boxes"""
        ol, synth = self.ol, self.synth
        t0 = time.perf_counter()
        m, mask, _ = ol.segment_ground_plane(cx, cy, cz)             # :105-138
        self._t("segment_ground_plane", t0)
        if m == 0 or m == len(cx):
            return []
        keep = mask == 0
        sx, sy, sz = cx[keep], cy[keep], cz[keep]                    # ExtractIndices(negative)
        t0 = time.perf_counter()
        ids = ol.extract_cloud_per_bbox(self.K, sx, sy, sz, self.b, synth.IMG_W, synth.IMG_H)   # :250-298
        self._t("extract_cloud_per_bbox", t0)
        t0 = time.perf_counter()
        poses = []
        order = np.argsort(ids, kind="stable")                       # per-box clouds in cloud order
        cuts = np.searchsorted(ids[order], np.arange(len(self.b) + 1))
        for i in range(len(self.b)):
            sel = order[cuts[i]:cuts[i + 1]]
            bx, by, bz = sx[sel], sy[sel], sz[sel]
            kp = ol.radius_outlier_grid(bx, by, bz, 0.4, 10).astype(bool)   # :150-154
            ok, e = ol.pca_bbox(bx[kp], by[kp], bz[kp])                     # :156-247
            if ok:
                poses.append(e)
        self._t("radius_filter_pca", t0)
        return poses

    def tick(self, vision, net, k_near=4):
        ol = self.ol
        t_all = time.perf_counter()
        t0 = time.perf_counter()
        cx, cy, cz = ol.transform_cloud(self.m_cam, self.x, self.y, self.z)   # transformLidarToCamera (:280-307)
        self._t("transform_lidar_to_camera", t0)
        st, dy = ol.filter_bboxes(self.b)
        t0 = time.perf_counter()
        self.knn(cx, cy, cz, st, k_near)
        self._t("knn_depth", t0)
        if vision:
            t0 = time.perf_counter()
            cam_poses = ol.post_process(self.cam, net[0], net[1], net[2], dy)   # :449-510
            self._t("vision_post_process", t0)
        else:
            cam_poses = self.bbox_pose(cx, cy, cz)
        t0 = time.perf_counter()
        base = np.zeros(len(cam_poses), dtype=self.synth.LSHAPE_DTYPE)
        for i, e in enumerate(cam_poses):
            o = ol.tf_pose(self.tfs["base_cam"], [e[k] for k in ("px", "py", "pz", "qx", "qy", "qz", "qw")])
            base[i] = tuple(o.tolist()) + (e["length"], e["width"], e["height"])
        self.og.update_map_poses(base)                                # :65-105
        self.og.to_occupancy_grid()                                   # :265-278
        self._t("update_map_and_pack", t0)
        self._t("tick", t_all)
        return len(base)

    def timed(self, vision, net, budget_s, max_ticks=20):
        self.tick(vision, net)   # page-in
        self.ms = {}
        n, t0 = 0, time.perf_counter()
        while True:
            self.tick(vision, net)
            n += 1
            if time.perf_counter() - t0 >= budget_s or n >= max_ticks:
                break
        dt = time.perf_counter() - t0
        return {"value": dt / n * 1e3, "unit": "ms/tick", "cores": 1, "kind": "port",
                "sample": f"{n} whole ticks of the same scene and boxes, {dt:.1f} s",
                "phases_ms": {k: round(v / n, 3) for k, v in self.ms.items() if k != "tick"}}


def leg_tick(gvamd, synth, g, tfs, local_rank, cpu_seconds):
    """The reference's per-frame flow as ONE measured unit (round-3 verdict, missing #2): gv_tick = timerCallback from
    filterBBoxes on (grid_vision_node.cpp:153-244), both branches, at BASELINE configs[2] size on a scene with objects.
    back_to_back: cloud resident, ticks one after the other, host clock around enqueue + the one host wait, the 4 MB
    OccupancyGrid.data delivered to pinned host memory inside it.  at_20hz: the node's operating point -- a 50 ms timer,
    a fresh cloud from pinned host memory every tick (cloudCallback), then the tick; the device idles and clocks down in
    between.  cpu_baseline: the oracle's same flow, one thread."""
    x, y, z, b = synth.scene_with_objects(tfs)
    n = len(x)
    h = gvamd.GridVisionHIP(g.grid_x, g.grid_y, g.resolution, device=local_rank)
    h.set_transforms(tfs["cam_lidar"], tfs["base_cam"], tfs["base_lidar"])
    blk = gvamd.PinnedF32(3 * n)
    blk.array[:n], blk.array[n:2 * n], blk.array[2 * n:] = x, y, z
    h.upload_xyz(x, y, z)
    st, dy = gvamd.filter_bboxes(b)
    net = synth.network_outputs(len(dy))
    pin = gvamd.PinnedI8(h.G)
    out = {"points": n, "bboxes": len(b), "static_bboxes": len(st), "dynamic_bboxes": len(dy), "k_near": 4, "host_waits_per_tick": 1}

    def pct(a, q):
        a = sorted(a)
        return a[min(len(a) - 1, int(q * len(a)))]

    for name, vision in (("vision", True), ("pca", False)):
        kw = dict(k_near=4, vision=vision, net=net if vision else None, grid_out=pin.array)
        for _ in range(5):
            r = h.tick(b, **kw)
        ts = []
        for _ in range(40):
            t0 = time.perf_counter()
            r = h.tick(b, **kw)
            ts.append((time.perf_counter() - t0) * 1e3)
        kw0 = dict(kw, grid_out=None)   # a node that updates the map and does not publish the grid this tick
        ts0 = []
        for _ in range(25):
            t0 = time.perf_counter()
            h.tick(b, **kw0)
            ts0.append((time.perf_counter() - t0) * 1e3)
        ts0 = ts0[5:]
        lat = []
        period = 0.050
        t_next = time.perf_counter()
        for f in range(65):
            t_next += period
            while time.perf_counter() < t_next:
                time.sleep(0.0005)
            t0 = time.perf_counter()
            h.upload_xyz_async(blk.array[:n], blk.array[n:2 * n], blk.array[2 * n:])
            h.tick(b, **kw)
            lat.append((time.perf_counter() - t0) * 1e3)
        lat = lat[5:]   # the first ticks include first-touch costs
        res = {"ms": float(np.median(ts)), "ms_min": min(ts), "p50": pct(ts, 0.5), "p99": pct(ts, 0.99),
               "ms_without_grid_download": float(np.median(ts0)),
               "at_20hz_ms": {"p50": pct(lat, 0.5), "p99": pct(lat, 0.99), "max": max(lat), "ticks": len(lat),
                              "includes": "12 MB cloud upload from pinned host memory + tick + 4 MB grid to pinned host memory"},
               "valid_poses": int(len(r["poses"])), "depths": int(len(r["depths"]))}
        if cpu_seconds > 0:
            res["cpu_baseline"] = CpuTick(synth, g, tfs, x, y, z, b).timed(vision, net, cpu_seconds)
            res["gpu_over_cpu"] = res["cpu_baseline"]["value"] / res["ms"]
        out[name] = res
    pin.close()
    h.close()
    blk.close()
    out["note"] = ("host-observed milliseconds per tick; ms = median of 40 back-to-back ticks (cloud resident); every tick ends with "
                   "depths, poses and OccupancyGrid.data on the host after ONE host wait (gv_tick_wait)")
    return out


def leg_pca_path(gvamd, synth, g, tfs, config, bboxes, local_rank, reps=10, cpu_seconds=0.0):
    """The reference's other hot loops on the same cloud (cloud_detections.cpp:8-87 kNN depth, :105-138 RANSAC
    ground removal, :140-247 radius filter + PCA rectangle): host-observed time per call through the C ABI
    (each call ends with its results on the host), on the uniform and on the lidar-like config-3 cloud."""
    out = {}

    def objects(_config):
        x, y, z, b = synth.scene_with_objects(tfs)
        return x, y, z, b
    for name, fn in (("objects", objects), ("lidar_like", synth.cloud_lidar_like)):
        x, y, z, b4 = fn(config)
        if name == "objects":
            bboxes_saved, bboxes = bboxes, b4   # the scene's own boxes (each around an object)
        h = gvamd.GridVisionHIP(g.grid_x, g.grid_y, g.resolution, device=local_rank)
        h.set_transforms(tfs["cam_lidar"], tfs["base_cam"], tfs["base_lidar"])
        h.upload_xyz(x, y, z)
        calls = {"compute_depth_for_bboxes_k10": lambda: h.compute_depth_for_bboxes(bboxes, 10),
                 "segment_ground_plane": lambda: h._lib.gv_segment_ground_plane(h._h, gvamd.C.c_double(0.04), gvamd.C.c_int32(50),
                                                                                gvamd.C.c_uint64(12345), None, None, None),
                 "compute_bbox_pose": lambda: h.compute_bbox_pose(bboxes),
                 "compute_bbox_pose_ground_removed": lambda: h.compute_bbox_pose_ground_removed(bboxes)}
        res = {}
        for cname, call in calls.items():
            call()
            call()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                r = call()
                ts.append((time.perf_counter() - t0) * 1e3)
            res[cname + "_ms"] = float(np.median(ts))
        _, valid, npz = h.compute_bbox_pose_ground_removed(bboxes)
        res["valid_poses"] = int(np.sum(valid))
        res["points"] = len(x)
        res["bboxes"] = len(bboxes)
        h.close()
        if cpu_seconds > 0:
            # the oracle's same calls on this box's host cores, one thread (kind "port"): median of a few runs each
            ct = CpuTick(synth, g, tfs, x, y, z, bboxes)
            cx, cy, cz = ct.ol.transform_cloud(ct.m_cam, x, y, z)

            def med(fn_, n_):
                ts_ = []
                for _ in range(n_):
                    t0_ = time.perf_counter()
                    fn_()
                    ts_.append((time.perf_counter() - t0_) * 1e3)
                return float(np.median(ts_))
            res["cpu_baseline"] = {
                "compute_depth_for_bboxes_k10_ms": med(lambda: ct.knn(cx, cy, cz, bboxes, 10), 3),
                "segment_ground_plane_ms": med(lambda: ct.ol.segment_ground_plane(cx, cy, cz), 3),
                "compute_bbox_pose_ground_removed_ms": med(lambda: ct.bbox_pose(cx, cy, cz), 3),
                "cores": 1, "kind": "port",
                "sample": "the oracle's calls on the same camera-frame cloud and boxes, median of 3 runs each; the radius filter "
                          "in its cell-grid form (identical keep flags)"}
        if name == "objects":
            bboxes = bboxes_saved
        out[name] = res
    out["note"] = ("host-observed milliseconds per C-ABI call (median of %d), results back on the host; "
                   "compute_bbox_pose_ground_removed = RANSAC + bbox test + radius filter + PCA rectangle; "
                   "objects = synth.scene_with_objects (40 dense objects, each in a box of its own); the uniform cloud of earlier "
                   "rounds loses every point to the radius filter (valid_poses 0) and is no longer timed" % reps)
    return out


def pmc_child_passes(config, budget_note, sharded_world=0):
    """HBM traffic and issue counters of every kernel, measured in THIS run: the script runs itself
    (--plain, serial frame so that dispatches do not overlap) under `rocprofv3 --pmc`, one counter group
    per pass and no trace domain (MI355X_MICROARCH.md, rocprofv3 PMC slots / HBM).  FETCH_SIZE is in KB
    and is doubled: gfx950 tallies 128-byte read requests at 64 bytes."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None, "rocprofv3 not found"
    groups = ["FETCH_SIZE", "WRITE_SIZE", "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVES",
              "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAVE_CYCLES SQ_WAIT_ANY"]
    res = {}
    tmp = tempfile.mkdtemp(prefix="gv_pmc_", dir="/tmp")
    env = dict(os.environ, GV_PIPELINE="0", TMPDIR="/tmp")
    env.pop("WORLD_SIZE", None)
    errs = []
    try:
        for k, grp in enumerate(groups):
            d = os.path.join(tmp, f"p{k}")
            cmd = [rocprof, "--pmc", *grp.split(), "--output-format", "csv", "-d", d, "--", sys.executable,
                   os.path.join(ROOT, "bench.py"), "--plain", "--steps", "10", "--warmup", "3", "--config", str(config)]
            if sharded_world:
                # the sharded frame's kernels on ONE rank's share of the points, through a 1-rank communicator (a
                # profiler child cannot join the job's communicator): same kernels, same per-rank point count; the
                # sector stage runs all of its workgroups here, 1 / world of them in the job
                cmd += ["--force-sharded", "--slice-of", str(sharded_world)]
            try:
                p = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=150)
            except subprocess.TimeoutExpired:
                errs.append(f"pass {grp}: timeout")
                continue
            if p.returncode != 0:
                errs.append(f"pass {grp}: rc {p.returncode}: {p.stderr.decode(errors='replace')[-200:]}")
                continue
            for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                acc = {}
                for r in csv.DictReader(open(f)):
                    name = r["Kernel_Name"]
                    if "gv::" not in name:
                        continue
                    short = name.split("gv::")[1].split("(")[0].split("<")[0]
                    acc.setdefault((short, r["Counter_Name"]), []).append(float(r["Counter_Value"]))
                for (short, c), v in acc.items():
                    res.setdefault(short, {})[c] = sum(v) / len(v)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for cs in res.values():
        if "FETCH_SIZE" in cs:
            cs["fetch_bytes"] = cs["FETCH_SIZE"] * 1024 * 2
        if "WRITE_SIZE" in cs:
            cs["write_bytes"] = cs["WRITE_SIZE"] * 1024
        if "fetch_bytes" in cs and "write_bytes" in cs:
            cs["hbm_bytes"] = cs["fetch_bytes"] + cs["write_bytes"]
    return (res or None), ("; ".join(errs) if errs else None)


# ------------------------------------------------------------------------------- outputs --
DUMP_CAP = 1 << 21   # elements per array: six float32 arrays are at most 48 MiB of data


def dump_outputs(h, out_dir, grid_only):
    """What the timed frame returned in its last step, as float32 DIR/<name>.npy: the grid layers (log-odds,
    occupancy, the int8 occupancy grid) and, unless the frame is sharded (whose counts stay per band), the int32
    hit counts, the miss grid and the per-point bbox ids.  Counts and ids are below 2^24 (at most 10 M points), so
    float32 holds them exactly.  An array longer than DUMP_CAP is a fixed seeded sample of its positions (sorted;
    the same positions for every array of that length), so that two builds compare output for output."""
    os.makedirs(out_dir, exist_ok=True)
    outs = {"log_odds": h.log_odds(), "occupancy": h.occupancy(), "occupancy_grid": h.to_occupancy_grid()[0]}
    if not grid_only:
        outs.update(hits=h.hits(), miss=h.miss(), bbox_id=h.bbox_id())
    for name, v in outs.items():
        if v.size > DUMP_CAP:
            v = v[np.sort(np.random.default_rng(0).choice(v.size, DUMP_CAP, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), v.astype(np.float32))


# ------------------------------------------------------------------------------ launcher --
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def spawn_ranks(a):
    """--gpus N without a torchrun environment: this parent (which has not touched the GPU) starts the
    N ranks and relays their single JSON line; it never falls back to one GPU."""
    import torch
    ndev = torch.cuda.device_count()   # does not initialise the GPU
    if ndev < a.gpus and not a.rehearsal:
        print(f"bench.py: --gpus {a.gpus} but only {ndev} GPU(s) visible; refusing to report a smaller job "
              f"(use --rehearsal to share devices)", file=sys.stderr)
        return 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__), *sys.argv[1:]]
    return subprocess.call(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")))


def main():
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(a))
    # RCCL (and some HIP runtime paths) print banners on stdout; the contract is ONE JSON line
    # there, so everything incidental goes to stderr and the result line to the real stdout.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != max(a.gpus, 1):
        print(f"bench.py: --gpus {a.gpus} does not match WORLD_SIZE {world}", file=sys.stderr)
        sys.exit(2)
    import torch
    dist = None
    ndev = torch.cuda.device_count()
    rehearsal = ndev < world
    if rehearsal and not a.rehearsal:
        print(f"bench.py: {world} ranks but only {ndev} GPU(s) visible (use --rehearsal to share devices)", file=sys.stderr)
        sys.exit(2)
    if world > 1:
        import torch.distributed as dist
        if not rehearsal:
            torch.cuda.set_device(local_rank)
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))   # nccl == RCCL
        else:
            # rehearsal on a box with fewer GPUs than ranks: ranks share devices, gloo for the barrier
            local_rank = local_rank % max(ndev, 1)
            torch.cuda.set_device(local_rank)
            dist.init_process_group(backend="gloo")
    else:
        torch.cuda.set_device(0)
        local_rank = 0

    import gvamd
    from gvamd import synth
    config = a.config or (3 if world == 1 else 4)
    cfg = synth.CONFIGS[config]
    g = cfg["grid"]
    cloud_fn = synth.cloud_uniform if a.cloud == "uniform" else synth.cloud_lidar_like
    tfs = synth.transforms(perturbed=True)
    bboxes = synth.detections(config)
    poses = synth.lshape_poses(config)
    sharded = config == 5 and (world > 1 or a.force_sharded)
    if config == 5:
        # configs[4]: ONE 10M-point frame (half lidar-like, half uniform); with world > 1 the points are
        # partitioned N/world per rank and the exchange happens inside the library (RCCL)
        xa, ya, za, _ = synth.cloud_lidar_like(config, cfg["n"] // 2)
        xb, yb, zb, _ = synth.cloud_uniform(config, cfg["n"] - cfg["n"] // 2)
        xf, yf, zf = np.concatenate([xa, xb]), np.concatenate([ya, yb]), np.concatenate([za, zb])
        lo_i, hi_i = (len(xf) * rank // world, len(xf) * (rank + 1) // world) if sharded else (0, len(xf))
        if sharded and world == 1 and a.slice_of > 1:
            hi_i = len(xf) // a.slice_of
        x, y, z = xf[lo_i:hi_i], yf[lo_i:hi_i], zf[lo_i:hi_i]
        N_total = len(xf)
    else:
        x, y, z, _ = cloud_fn(config, seed_extra=rank)
        N_total = len(x)
    N, G = len(x), g.nx * g.ny

    h = gvamd.GridVisionHIP(g.grid_x, g.grid_y, g.resolution, device=local_rank)
    h.set_transforms(tfs["cam_lidar"], tfs["base_cam"], tfs["base_lidar"])
    h.upload_xyz(x, y, z)   # resident in HBM before the timed region
    flags = gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH | gvamd.FRAME_BBOX_TEST
    h.set_detections(flags, bboxes=bboxes, poses=poses)
    if sharded:
        uid = [gvamd.GridVisionHIP.comm_unique_id() if rank == 0 else None]
        if dist is not None:
            dist.broadcast_object_list(uid, src=0)
        h.comm_init(uid[0], rank, world)
        # what RCCL itself reports, from every rank: the line must show that `world` ranks on `world` devices took part
        info = h.comm_info()
        infos = [info]
        if dist is not None:
            infos = [None] * world
            dist.all_gather_object(infos, info)

    def barrier():
        h.synchronize()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def step():
        if sharded:
            h.enqueue_frame_sharded()   # asynchronous, collective: exchanges of frame f overlap the binning of f + 1
        else:
            h.enqueue_frame()

    # W untimed warm-up steps, then a region of EXACTLY K steps bracketed by barrier + synchronize on both
    # sides and reduced by MAX over ranks.  A plain run times that one region.  With --full (or --plain) the
    # region is repeated and `value` is the median repetition (a single K = 20 region is ~1 ms long and
    # inherits whatever clock state the warm-up left: round-2 verdict), the spread is printed next to it: at
    # least --min-reps repetitions, more until 0.25 s have been timed (at most 200).
    extra = a.full or a.plain           # repetitions, stage times, kernel rooflines, sharded step times
    everything = a.full and not a.plain   # + PMC passes, copy rate, the other legs, CPU baselines
    for _ in range(a.warmup):
        step()
    barrier()
    reps = []
    while not reps or (extra and (len(reps) < a.min_reps or (sum(reps) < 0.25 and len(reps) < 200))):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        barrier()
        dt_r = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([dt_r], dtype=torch.float64, device="cpu" if rehearsal else "cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt_r = float(t.item())
        reps.append(dt_r)
    dt = float(np.median(reps))
    frames = a.steps if sharded else a.steps * world   # sharded: all ranks work on the same frame
    fps = frames / dt
    if a.dump_outputs and rank == 0:
        dump_outputs(h, a.dump_outputs, grid_only=sharded)
    shard_extra = None
    if sharded and extra:
        # collective extras: per-step device times (frames one at a time) and the H2D-inclusive rate -- every rank
        # uploads only ITS N / world slice per frame, so the ingest bandwidth of the job is `world` PCIe links
        steps_ms = h.time_frame_sharded_stages(5)
        blk = gvamd.PinnedF32(3 * N)
        blk.array[:N], blk.array[N:2 * N], blk.array[2 * N:] = x, y, z

        def one_h2d():
            h.upload_xyz_async(blk.array[:N], blk.array[N:2 * N], blk.array[2 * N:])
            h.enqueue_frame_sharded()
        for _ in range(8):
            one_h2d()
        barrier()
        th0 = time.perf_counter()
        nh = 30
        for _ in range(nh):
            one_h2d()
        barrier()
        dth = time.perf_counter() - th0
        if dist is not None:
            t = torch.tensor([dth], dtype=torch.float64, device="cpu" if rehearsal else "cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dth = float(t.item())
        h.synchronize()
        blk.close()
        shard_extra = {"steps_ms": steps_ms, "steps_ms_sum": sum(steps_ms.values()),
                       "with_h2d_frames_per_s": nh / dth, "with_h2d_ms_per_frame": dth / nh * 1e3,
                       "h2d_bytes_per_rank_per_frame": 12 * N,
                       "note": "steps: device time of each step with frames run one at a time (no overlap); with_h2d: a fresh "
                               "cloud slice from pinned host memory per rank and frame, asynchronous"}

    out = None
    if rank == 0:
        bytes_frame = 12.0 * N + 13.0 * G
        # Algorithmic bytes per launch.  SURVEY 8(d): 12 B/point in, 13 B/cell
        # grid traffic; the int32 hit counts are row X1's output (4 B/cell).  The ray stage moves no
        # algorithmic bytes: it is priced against the VALU issue rate instead.
        alg = {"points": 12.0 * N, "ray_ends": 4.0 * G, "finalize": 13.0 * G, "ray_march": 0.0,
               "detections": 120.0 * (len(bboxes) + len(poses))}
        out = {
            "metric": f"frames/sec into grid ({N_total // 1000000}M-pt cloud / {g.nx}x{g.ny} @ {g.resolution} m grid)",
            "value": fps, "unit": "frames/s", "n_gpus": world if not rehearsal else min(world, max(ndev, 1)),
            "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": dt / a.steps * 1e3,
            "repetitions": {"n": len(reps), "of_steps": a.steps, "value_is": "median",
                            "ms_per_step_min": min(reps) / a.steps * 1e3, "ms_per_step_max": max(reps) / a.steps * 1e3,
                            "ms_per_step_first": reps[0] / a.steps * 1e3},
            "higher_is_better": True, "scaling": "strong" if sharded else "weak",
            "vs_baseline": None, "dtype": "i32 hit counts / f64 cell index / f32 log-odds", "data": "synthetic",
            "config": {"workload": f"BASELINE configs[{config - 1}]: {N}-point {a.cloud if config != 5 else 'lidar-like + uniform'} cloud per GPU, "
                                   f"{g.nx}x{g.ny} @ {g.resolution} m grid, {len(bboxes)} bboxes + {len(poses)} poses, "
                                   "bin (int32 hit counts) + ray-march + bbox test + grid pass, inputs resident in HBM",
                       "points": N, "cells": G,
                       "parallelism": (f"points-sharded x{world} + RCCL bitmap OR-exchange" if sharded else f"frame-per-gpu x{world}"),
                       "devices_visible": ndev},
            "mpoints_per_s": N_total * fps / 1e6,
            "frame_roofline": {"algorithmic_bytes": bytes_frame, "achieved_GBps": bytes_frame * fps / world / 1e9,
                               "frac_of_hbm_peak": bytes_frame * fps / world / 1e9 / HBM_PEAK_GBPS},
        }
        if rehearsal:
            out["rehearsal"] = True
        if sharded:
            # what RCCL reported on every rank (gathered at set-up): proof of how many ranks took part
            out["sharded"] = dict(shard_extra or {}, rccl_ranks=int(infos[0][0]),
                                  rccl=[{"rank": int(i[1]), "device": int(i[2]), "ranks_seen": int(i[0])} for i in infos])
        if extra:
            # per-kernel device time (gv_time_frame_stages: serial frames, so every kernel runs alone): each kernel
            # carries a start and an end HIP event on its own dispatch packet (hipExtLaunchKernelGGL), so the
            # figure is the kernel's duration as rocprofv3 reports it (profiles/rNN/serial_kernel_stats.csv), not
            # an interval between event records.  In the timed region two frames run side by side and every kernel
            # is stretched by its neighbours (profiles/rNN/pipelined_kernel_stats.csv); `value` comes from there.
            stages = h.time_frame_stages(max(10, min(a.steps, 50)))
            n_rays, n_visits = h.ray_stats()
            out["stage_ms"], out["stage_ms_sum"] = stages, sum(stages.values())
            out["ray_march"] = {"rays": n_rays, "equivalent_cell_visits": n_visits,
                                "mcell_visits_per_s": (n_visits / (stages["ray_march"] * 1e-3) / 1e6) if stages["ray_march"] > 0 else None}
            pmc, pmc_err = (None, "skipped")
            if everything and not a.no_pmc and not rehearsal:
                # (at N > 1 too: the other ranks idle at the closing barrier while rank 0's children profile the same
                #  workload on its own GPU, so that the roofline object is filled at every N)
                h.synchronize()
                pmc, pmc_err = pmc_child_passes(3 if config == 4 else config, "", sharded_world=world if sharded else 0)
            kernels = []
            for st, ms in stages.items():
                if st == "detections":
                    continue   # the rectangles ride the partition launch: no kernel of their own (the slot times two event records)
                kn = KERNEL_OF[st]
                c = (pmc or {}).get(kn, {})
                e = {"stage": st, "kernel": kn, "ms": ms, "traffic": c.get("hbm_bytes"),
                     "fetch_bytes": c.get("fetch_bytes"), "write_bytes": c.get("write_bytes")}
                if st == "ray_march":
                    # LDS / issue / latency kernel: no algorithmic HBM bytes; fraction of the VALU issue peak
                    iv = c.get("SQ_INSTS_VALU")
                    e.update({"bound": "valu-issue/lds", "unit": "Gwave-instr/s", "peak": VALU_PEAK_GWIPS,
                              "achieved": (iv / (ms * 1e-3) / 1e9) if iv and ms > 0 else None,
                              "valu_wave_instructions": iv,
                              "lds_bank_conflict_ratio": (c["SQ_LDS_BANK_CONFLICT"] / c["SQ_LDS_IDX_ACTIVE"])
                              if c.get("SQ_LDS_IDX_ACTIVE") else None,
                              "mcell_visits_per_s": out["ray_march"]["mcell_visits_per_s"]})
                else:
                    e.update({"bound": "hbm", "unit": "GB/s", "peak": HBM_PEAK_GBPS, "algorithmic_bytes": alg[st],
                              "achieved": alg[st] / (ms * 1e-3) / 1e9 if ms > 0 else None})
                e["frac"] = (e["achieved"] / e["peak"]) if e.get("achieved") else None
                kernels.append(e)
            out["kernels"] = kernels
            dom = max(kernels, key=lambda k: k["ms"])
            out["roofline"] = {k: dom.get(k) for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic")}
            out["roofline"]["kernel_ms"] = dom["ms"]
            out["roofline"]["note"] = ("dominant kernel by HIP-event time; traffic = PMC HBM bytes per launch measured in this run "
                                       "(rocprofv3 child passes, FETCH_SIZE doubled)" + (f"; pmc: {pmc_err}" if pmc_err else ""))
            hbm = [k for k in kernels if k["bound"] == "hbm" and k["stage"] != "detections"]
            # the HBM roofline entry: the kernel that moves the most algorithmic bytes (the grid pass, 13 B/cell); the
            # partition and tile passes are priced against HBM too in kernels[] but are issue / latency bound
            dom_hbm = max(hbm, key=lambda k: k["algorithmic_bytes"])
            out["roofline_hbm"] = {k: dom_hbm.get(k) for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic")}
            out["roofline_hbm"]["kernel_ms"] = dom_hbm["ms"]
            out["roofline_hbm"]["algorithmic_bytes"] = dom_hbm["algorithmic_bytes"]
            # three lanes x ~50 MB per frame sit in the 256 MiB Infinity Cache at config 3 (FETCH_SIZE counts its hits): the
            # fraction is then an L3-resident one; config 5 (beyond_l3 leg, ~0.5 GB per frame) is the HBM figure
            out["roofline_hbm"]["l3_resident"] = bool(bytes_frame * 4 < 256 * 2 ** 20)
        if everything:
            try:
                copy_gbps = measured_copy_rate(torch)
                out["frame_roofline"]["measured_copy_GBps"] = copy_gbps
                out["frame_roofline"]["frac_of_measured_copy"] = bytes_frame * fps / world / 1e9 / copy_gbps
            except Exception as e:   # never fail the bench line over the auxiliary peak
                print("copy-rate measurement failed:", e, file=sys.stderr)
        if everything and world == 1 and config == 3:
            # the legs below make handles of their own: the headline's handle goes first, or its five streams keep
            # sharing the process's four hardware queues with theirs (measured: the lidar-like leg 17.7 k instead of
            # 21.5 k frames/s with both handles alive)
            h.close()
            h = None
            try:
                out["with_h2d"] = leg_with_h2d(gvamd, synth, g, tfs, config, flags, local_rank, 300)
            except Exception as e:
                out["with_h2d"] = {"error": str(e)}
            cpu_s = 0.0 if a.no_cpu_baseline else min(a.cpu_seconds, 6.0)
            try:
                out["tick"] = leg_tick(gvamd, synth, g, tfs, local_rank, cpu_s)
            except Exception as e:
                out["tick"] = {"error": repr(e)}
            try:
                out["pca_path"] = leg_pca_path(gvamd, synth, g, tfs, config, bboxes, local_rank, cpu_seconds=cpu_s)
            except Exception as e:
                out["pca_path"] = {"error": repr(e)}
            try:
                out["lidar_like"] = leg_cloud(gvamd, synth, g, tfs, config, flags, bboxes, poses, local_rank,
                                              min(a.steps, 200), synth.cloud_lidar_like)
                out["lidar_like"]["note"] = "SURVEY 8(d) config 3(b): range ~ Exp(15 m), 64 rings: hundreds of hits per cell near the sensor"
            except Exception as e:
                out["lidar_like"] = {"error": str(e)}
            try:
                c5 = synth.CONFIGS[5]

                def cloud_config5(cfg_id):   # half lidar-like, half uniform (as the sharded run uses)
                    n5 = synth.CONFIGS[cfg_id]["n"]
                    xa, ya, za, ia = synth.cloud_lidar_like(cfg_id, n5 // 2)
                    xb, yb, zb, ib = synth.cloud_uniform(cfg_id, n5 - n5 // 2)
                    return np.concatenate([xa, xb]), np.concatenate([ya, yb]), np.concatenate([za, zb]), np.concatenate([ia, ib])
                leg = leg_cloud(gvamd, synth, c5["grid"], tfs, 5, gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH, None, None,
                                local_rank, 20, cloud_config5)
                b5 = 12.0 * leg["points"] + 13.0 * c5["grid"].nx * c5["grid"].ny
                leg.update({"algorithmic_bytes": b5, "achieved_GBps": b5 * leg["value"] / 1e9,
                            "frac_of_hbm_peak": b5 * leg["value"] / 1e9 / HBM_PEAK_GBPS,
                            "note": "BASELINE configs[4] workload on ONE GPU (10M points, half lidar-like + half uniform, 4000x4000 grid): ~0.5 GB touched "
                                    "per frame, past the 256 MiB Infinity Cache"})
                out["beyond_l3"] = leg
            except Exception as e:
                out["beyond_l3"] = {"error": str(e)}
        if everything and not a.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(config, cloud_fn, tfs, bboxes, poses, a.cpu_seconds)
            out["gpu_over_cpu"] = fps / out["cpu_baseline"]["value"]
            out["cpu_baseline_all_cores"] = cpu_baseline_all_cores(config, cloud_fn, tfs, bboxes, poses, a.cpu_seconds)
            out["gpu_over_cpu_all_cores"] = fps / out["cpu_baseline_all_cores"]["value"]
        else:
            out["cpu_baseline"] = None
    if h is not None:
        h.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        sys.stdout.flush()
        os.write(real_stdout, (json.dumps(out) + "\n").encode())


if __name__ == "__main__":
    main()
