"""What tools/inflate_time.py, traj_score_time.py and nav_field_time.py share: the map fill, the rollouts, the HIP runtime
through ctypes with an event timer, and the reader of a rocprofv3 kernel trace."""
from __future__ import annotations

import csv
import ctypes as C
import glob
import os

import numpy as np


def fill_poses(synth, h, res, n, seed):
    """n L-shape poses over the map and a little beyond it: one tick of the 12-tick fill of tests/test_gpu_grid_move.py"""
    rng = np.random.default_rng(seed)
    lx, ly = h.nx * res, h.ny * res
    p = np.zeros(n, dtype=synth.LSHAPE_DTYPE)
    p["px"] = rng.uniform(h.pos_x - 0.55 * lx, h.pos_x + 0.55 * lx, n)
    p["py"] = rng.uniform(h.pos_y - 0.55 * ly, h.pos_y + 0.55 * ly, n)
    p["qw"] = 1.0
    p["length"] = rng.uniform(0.5, 0.1 * lx, n)
    p["width"] = rng.uniform(0.5, 0.1 * ly, n)
    p["height"] = 1.5
    return p


def arcs(h, K, P, seed, start, step=0.25):
    """K constant-curvature rollouts of P poses from one start pose, `start` = (dx, dy) from the map's centre, as a
    sampling controller makes them: float32 (K, P, 3)"""
    rng = np.random.default_rng(seed)
    curv = rng.uniform(-0.3, 0.3, K)
    yaw0 = 0.3 + rng.normal(0.0, 0.05, K)
    s = step * np.arange(P)[None, :]
    yaw = yaw0[:, None] + curv[:, None] * s
    x = h.pos_x + start[0] + np.cumsum(step * np.cos(yaw), axis=1)
    y = h.pos_y + start[1] + np.cumsum(step * np.sin(yaw), axis=1)
    return np.ascontiguousarray(np.stack([x, y, yaw], axis=2), np.float32)


def load_hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


def device_copy(hip, a):
    """the array's bytes in a device allocation of their own (hipFree it)"""
    dptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(dptr), a.nbytes) == 0
    assert hip.hipMemcpy(dptr, a.ctypes.data, a.nbytes, 1) == 0
    return dptr


def event_us_per_call(hip, h, n, call):
    """HIP events on the handle's stream around n back-to-back call()s: the interval / n in us"""
    s = C.c_void_p(h.stream())
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    assert hip.hipEventRecord(e0, s) == 0
    for _ in range(n):
        call()
    assert hip.hipEventRecord(e1, s) == 0
    assert hip.hipEventSynchronize(e1) == 0
    ms = C.c_float()
    assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    return 1000.0 * ms.value / n


def kernel_durations(trace_dir, kernels):
    """{kernel: [duration in us of every dispatch whose name holds it, in start order]} from the *kernel_trace.csv files
    of a rocprofv3 --kernel-trace run"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no *kernel_trace.csv under " + trace_dir
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return {k: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if k in r["Kernel_Name"]]
            for k in kernels}


def append_out(path, lines):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        f.write("\n".join(lines) + "\n")
