"""What the planner-side GPU tests (test_gpu_inflate.py, test_gpu_traj.py, test_gpu_nav.py) share: planting a map, the
HIP runtime for device poses, and the first difference of two arrays for an assertion's message.  A plain module: the
handles and references stay with the test modules."""
import ctypes as C

import numpy as np


def hip_runtime():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


def plant_grid(h, mask):
    """lethal (97) where the data-order mask says so, free (11) elsewhere; returns the int8 readback"""
    lo = np.where(mask.reshape(-1)[::-1], np.float32(10.0), np.float32(-10.0)).astype(np.float32)   # cell = G-1-byte
    h.set_log_odds(lo)
    h.update_map()
    i8 = h.to_occupancy_grid()[0]
    assert np.array_equal(i8.reshape(mask.shape) >= 65, mask)
    return i8


def plant(h, mask, inflation):
    """plant_grid, then gv_inflate with inflation = (inscribed, inflation, scaling, threshold); returns the costmap readback"""
    plant_grid(h, mask)
    h.set_inflation(*inflation)
    h.inflate()
    cost = h.costmap()
    assert np.array_equal(cost.reshape(mask.shape) == 254, mask)
    return cost


def first_diff(got, want):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    bad = np.flatnonzero(got != want)
    return None if not len(bad) else dict(n=len(bad), at=int(bad[0]), got=got[bad[0]], want=want[bad[0]])
