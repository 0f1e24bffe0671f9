"""[EXTENSION] X10 rollout and control step: the plain reference of include/gridvision_hip.h's definition.  The rollout as
the loop the header writes, with Python floats (IEEE doubles, one rounding per operation, nothing contracted) and
math.sin / math.cos -- the C library's, NOT numpy's vectorised fp64 trig, which need not equal it.  The selection as a
Python loop over the structured records, in Python integers masked to 64 bits."""
import math

import numpy as np

DIFF, OMNI = 0, 1
DEVICE_CONTROLS, CONSTANT = 1 << 0, 1 << 1
KEEP_TOTALS = 1 << 0
RESULT_DTYPE = np.dtype([("best", np.int32), ("n_valid", np.int32), ("best_total", np.uint64)])
U64 = (1 << 64) - 1
WEIGHTS = ("w_cost_sum", "w_max_cost", "w_nav_last", "w_nav_sum", "w_nav_best")


def n_controls(model):
    return 3 if model == OMNI else 2


def _cos(t):
    return math.cos(t) if math.isfinite(t) else math.nan   # math.cos(inf) raises; IEEE says NaN


def _sin(t):
    return math.sin(t) if math.isfinite(t) else math.nan


def rollout(model, dt, start, controls, constant=False, P=None):
    """controls float32 (K, P, C), or (K, C) with constant and P given.  Returns float32 (K, P, 3): pose p is the state
    after step p."""
    controls = np.asarray(controls, np.float32)
    K = controls.shape[0]
    P = int(P) if constant else controls.shape[1]
    assert controls.shape[-1] == n_controls(model)
    dt = float(dt)
    out = np.zeros((K, P, 3), np.float64)
    for k in range(K):
        X, Y, T = (float(v) for v in start)
        for p in range(P):
            u = [float(v) for v in (controls[k] if constant else controls[k, p])]   # float32 widened to double
            c, s = _cos(T), _sin(T)
            if model == DIFF:
                d = u[0] * dt
                X = X + d * c
                Y = Y + d * s
            else:
                a, b = u[0] * dt, u[1] * dt
                X = X + (a * c - b * s)
                Y = Y + (a * s + b * c)
            T = T + u[-1] * dt
            out[k, p] = (X, Y, T)
    with np.errstate(over="ignore", invalid="ignore"):
        return out.astype(np.float32)   # round to nearest even; beyond float32's range: infinity


def weights(w_cost_sum=0, w_max_cost=0, w_nav_last=0, w_nav_sum=0, w_nav_best=0):
    return dict(w_cost_sum=w_cost_sum, w_max_cost=w_max_cost, w_nav_last=w_nav_last, w_nav_sum=w_nav_sum,
                w_nav_best=w_nav_best)


def nav_used(w):
    return bool(w["w_nav_last"] or w["w_nav_sum"] or w["w_nav_best"])


def select(w, traj, nav=None):
    """w: weights(); traj / nav: the structured records of traj_ref / nav_ref (nav may be None without a nav weight).
    Returns (RESULT_DTYPE record array of 1, uint64 totals (K,))."""
    used = nav_used(w)
    assert nav is not None or not used
    best, best_total, n_valid = -1, U64, 0
    totals = []
    for k in range(len(traj)):
        rejected = int(traj[k]["first_collision"]) >= 0 or (used and int(nav[k]["n_bad"]) > 0)
        if rejected:
            totals.append(U64)
            continue
        total = w["w_cost_sum"] * int(traj[k]["cost_sum"]) + w["w_max_cost"] * (int(traj[k]["max_cost"]) & 0xFFFFFFFF)
        if used:
            total += (w["w_nav_last"] * int(nav[k]["last"]) + w["w_nav_sum"] * int(nav[k]["sum"])
                      + w["w_nav_best"] * int(nav[k]["best"]))
        total &= U64
        totals.append(total)
        n_valid += 1
        if best < 0 or total < best_total:   # the first k of the smallest total: a later equal one does not replace it
            best, best_total = k, total
    res = np.zeros(1, RESULT_DTYPE)
    res[0] = (best, n_valid, best_total)
    return res, np.array(totals, np.uint64).reshape(-1)
