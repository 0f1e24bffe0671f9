"""[EXTENSION] X12 MPPI limits and control cost: the plain reference of include/gridvision_hip.h's definition.
The chain in numpy float32 scalars, one operation per line (every np.float32 operation rounds once; nothing can be
contracted); the control cost in Python floats (IEEE doubles) with the 64 partial sums and the tree written out; the
average with the control cost as sequential fp64 sums over the admitted trajectories in index order, like
mppi_ref.average."""
import math

import numpy as np

from mppi_ref import SHIFT, U64

F = np.float32
LANES = 64


def chain_constants(rate_up, rate_down, min_turn_radius, dt):
    """up[3], dn[3] float32 and inv_r float32 of one call"""
    with np.errstate(over="ignore"):
        up = [F(float(r) * float(dt)) for r in rate_up]
        dn = [F(float(r) * float(dt)) for r in rate_down]
    inv_r = F(1.0 / float(min_turn_radius)) if min_turn_radius > 0 else F(0.0)
    return up, dn, inv_r


def constrain(rate_up, rate_down, u_prev, min_turn_radius, dt, controls):
    """controls float32 (K, P, C) = f.  Returns the constrained float32 (K, P, C)."""
    f = np.asarray(controls, F)
    K, P, C = f.shape
    up, dn, inv_r = chain_constants(rate_up, rate_down, min_turn_radius, dt)
    out = np.empty_like(f)
    with np.errstate(invalid="ignore"):
        for k in range(K):
            s = [F(u_prev[c]) for c in range(C)]
            for p in range(P):
                q = [F(f[k, p, c]) for c in range(C)]
                for c in range(C):
                    if not np.isnan(s[c]):
                        lo = F(s[c] - dn[c])
                        hi = F(s[c] + up[c])
                        q[c] = lo if q[c] < lo else q[c]
                        q[c] = hi if q[c] > hi else q[c]
                if inv_r > 0:
                    b = F(np.abs(q[0]) * inv_r)
                    nb = F(-b)
                    q[1] = nb if q[1] < nb else q[1]
                    q[1] = b if q[1] > b else q[1]
                s = list(q)
                for c in range(C):
                    out[k, p, c] = q[c]
    return out


def control_costs(gamma, sigma, controls, nominal, flags=0):
    """g (K,) fp64 of float32 controls (K, P, C) around the float32 nominal (P, C) their sampling read"""
    u = np.asarray(controls, F)
    nom = np.asarray(nominal, F)
    K, P, C = u.shape
    J = P * C
    qc = []
    for c in range(C):
        s = float(sigma[c])
        qc.append(float(gamma) / (s * s) if s > 0 else 0.0)
    g = np.zeros(K, np.float64)
    for k in range(K):
        a = [0.0] * LANES
        for l in range(LANES):
            for j in range(l, J, LANES):
                p, c = divmod(j, C)
                pn = min(p + 1, P - 1) if flags & SHIFT else p
                n = float(nom[pn, c])
                d = float(u[k, p, c]) - n
                t = n * d
                t = qc[c] * t
                a[l] = a[l] + t
        w = LANES // 2
        while w >= 1:
            for l in range(w):
                a[l] = a[l] + a[l + w]
            w //= 2
        g[k] = a[0]
    return g


def weights_cc(totals, g, lam):
    """(e (K,) fp64 with -1 for a rejected trajectory) or None when every trajectory is rejected"""
    t = [int(v) for v in totals]
    admitted = [v for v in t if v != U64]
    if not admitted:
        return None
    best = min(admitted)
    x = [float(v - best) + float(g[k]) if v != U64 else None for k, v in enumerate(t)]
    m = min(v for v in x if v is not None)
    e = np.full(len(t), -1.0)
    for k, v in enumerate(x):
        if v is not None:
            e[k] = math.exp(-((v - m) / float(lam)))
    return e


def average_cc(lam, controls, totals, g, nominal, bound=False):
    """mppi_ref.average with x_k = (double)(total_k - best_total) + g_k and m = min x_k in the exponent"""
    controls = np.asarray(controls, F)
    nominal = np.asarray(nominal, F)
    e = weights_cc(totals, g, lam)
    if e is None:
        return (nominal.copy(), nominal.astype(np.float64), np.zeros(nominal.shape)) if bound else nominal.copy()
    N, A, S = np.zeros(nominal.shape), np.zeros(nominal.shape), 0.0
    for k in range(len(controls)):
        if e[k] >= 0.0:
            u = controls[k].astype(np.float64)
            S = S + float(e[k])
            N = N + float(e[k]) * u
            A = A + float(e[k]) * np.abs(u)
    out = (N / S).astype(F)
    return (out, N / S, A / S) if bound else out
