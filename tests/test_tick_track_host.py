"""[EXTENSION] X15 the tick's detection list, host side (no GPU): the two flag values in the header and the binding; the
list's host twin (gv_test_tick_dets_host: the selection and the camera->base arithmetic of k_tick_dets, the same text
compiled for the host) against the oracle's tf2 pose transform on every branch of the basis -> quaternion step, byte for
byte; and the selection at its edges against a plain loop.

gv_transform_lshape_objects, the public call the twin must equal, reads the transform from a handle and a handle needs a
device: test_gpu_tick_track.py::test_host_twin_equals_public_transform holds the twin to it on the same inputs.  Here the
reference is the oracle (oracle/transforms.c), which that public call equals bit for bit (test_gpu_parity.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import tick_track_cases as cases
from gvamd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FLAGS = r"""
#include <stdio.h>
#include "gridvision_hip.h"
int main(void)
{
  printf("%d %d %d %d %d %d\n", (int)GV_TICK_VISION_ORIENT, (int)GV_TICK_LIDAR_BIN, (int)GV_TICK_LIDAR_RAYMARCH, (int)GV_TICK_KEEP_DETS,
         (int)GV_TRACK_TICK_DETS, (int)(GV_TRACK_DEVICE_DETS | GV_TRACK_FEED_DYNAMIC));
  return 0;
}
"""


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


def test_header_and_binding(gvamd, tmp_path):
    txt = open(os.path.join(ROOT, "include", "gridvision_hip.h")).read()
    src, exe = str(tmp_path / "flags.c"), str(tmp_path / "flags")
    with open(src, "w") as f:
        f.write(FLAGS)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", exe])
    assert subprocess.check_output([exe], text=True).split() == ["1", "2", "4", "8", "4", "3"]
    assert (gvamd.TICK_KEEP_DETS, gvamd.TRACK_TICK_DETS, gvamd.TICK_DETS) == (8, 4, 128)
    declared = sorted(set(re.findall(r"\b(gv_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))))
    assert len(declared) == 123 and sorted(gvamd.ABI_SYMBOLS) == declared      # two flag values, no function
    assert gvamd.load().gv_abi_version() == 4
    for phrase in ("grid_vision_node.cpp:204", ":227", "GV_TICK_KEEP_DETS", "GV_TRACK_TICK_DETS"):
        assert phrase in txt, phrase
    lib = gvamd.load()
    assert hasattr(lib, "gv_test_tick_dets") and hasattr(lib, "gv_test_tick_dets_host")     # hooks, outside the ABI
    hooks = open(os.path.join(ROOT, "grid-vision_amd", "csrc", "gv_test_hooks.h")).read()
    assert "gv_test_tick_dets(" in hooks and "gv_test_tick_dets_host(" in hooks


def _oracle_base(tf, cam):
    out = cam.copy()
    for i, p in enumerate(cam):
        o = ol.tf_pose(tf, [p[k] for k in ("px", "py", "pz") + cases.Q])
        for k, v in zip(("px", "py", "pz") + cases.Q, o):
            out[i][k] = v
    return out


def test_host_twin_equals_the_tf2_pose_transform(gvamd):
    """all candidates valid: the twin's records are the oracle's doTransform(Pose) of the camera poses, in order, cut at
    128 -- random unit quaternions, pitch-only quaternions as the pose branches make them, non-unit quaternions, and
    non-finite positions; every branch of getRotation is reached"""
    reached = set()
    for t, tf in enumerate(cases.branch_transforms()):
        for fam, cam in (("unit", cases.cam_poses(150, 10 + t)), ("pitch", cases.pitch_poses(90, 20 + t)),
                         ("scaled", cases.cam_poses(40, 30 + t, unit_q=False))):
            reached |= {cases.quat_branch(tf, p) for p in cam}
            got, n, n_total = gvamd.tick_dets_host(cam, np.ones(len(cam), np.uint8), tf)
            want = _oracle_base(tf, cam)
            assert (n, n_total) == (min(len(cam), 128), len(cam)), (t, fam)
            assert got[:n].tobytes() == want[:n].tobytes(), (t, fam)
            assert not got[n:].tobytes().strip(b"\0"), (t, fam)
        bad = cases.cam_poses(8, 40 + t)
        bad["px"][0], bad["py"][1], bad["pz"][2], bad["px"][3] = np.nan, np.inf, -np.inf, np.inf
        bad["py"][3] = -np.inf
        got, n, _ = gvamd.tick_dets_host(bad, np.ones(8, np.uint8), tf)
        want = _oracle_base(tf, bad)
        assert n == 8
        for k in synth.LSHAPE_DTYPE.names:      # a NaN's sign is the compiler's choice: equal values, NaN where NaN
            assert np.array_equal(got[k][:8], want[k], equal_nan=True), (t, k)
        for k in cases.Q + ("length", "width", "height"):
            assert got[k][:8].tobytes() == want[k].tobytes(), (t, k)
    assert reached >= {"trace", 0, 1, 2}, reached


@pytest.mark.parametrize("pattern", cases.PATTERNS)
def test_selection_edges(gvamd, pattern):
    tf = synth.transforms(True)["base_cam"]
    for n_cand in cases.COUNTS:
        cam = cases.pitch_poses(n_cand, 50 + n_cand)
        valid = cases.validity(pattern, n_cand)
        base, _, _ = gvamd.tick_dets_host(cam, np.ones(n_cand, np.uint8), tf) if n_cand <= 128 else (None, 0, 0)
        if base is None:      # every candidate in the base frame, 128 at a time
            base = np.concatenate([gvamd.tick_dets_host(cam[i:i + 128], np.ones(len(cam[i:i + 128]), np.uint8), tf)[0][:len(cam[i:i + 128])]
                                   for i in range(0, n_cand, 128)])
        want, wn, wt = cases.reference_list(base, valid, pattern == "empty")
        got, n, n_total = gvamd.tick_dets_host(cam, valid, tf, empty=pattern == "empty")
        assert (n, n_total) == (wn, wt), (pattern, n_cand)
        assert got.tobytes() == want.tobytes(), (pattern, n_cand)
        assert not got[n:].tobytes().strip(b"\0")
        if pattern == "first_128_invalid" and n_cand == 300:
            assert (n, n_total) == (128, 172)
        if pattern == "exactly_128_spread" and n_cand == 300:
            assert (n, n_total) == (128, 128) and valid.sum() == 128 and not valid.all()
        if pattern == "alternating" and n_cand == 300:
            assert (n, n_total) == (128, 150)


def test_twin_argument_rules(gvamd):
    import ctypes as C
    lib = gvamd.load()
    tf = gvamd.make_tf(synth.transforms(False)["base_cam"])
    out, n, nt = np.zeros(128, synth.LSHAPE_DTYPE), C.c_int32(), C.c_int32()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    args = (C.byref(tf), p(out), C.byref(n), C.byref(nt))
    assert lib.gv_test_tick_dets_host(None, None, C.c_int32(0), C.c_int32(0), *args) == 0 and (n.value, nt.value) == (0, 0)
    assert lib.gv_test_tick_dets_host(None, None, C.c_int32(1), C.c_int32(0), *args) == 1
    assert lib.gv_test_tick_dets_host(None, None, C.c_int32(-1), C.c_int32(0), *args) == 1
    assert lib.gv_test_tick_dets_host(None, None, C.c_int32(16384), C.c_int32(0), *args) == 1
    assert lib.gv_test_tick_dets_host(None, None, C.c_int32(0), C.c_int32(0), None, p(out), C.byref(n), C.byref(nt)) == 1
