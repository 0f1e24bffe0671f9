"""[EXTENSION] X11 MPPI sampling and softmax update: the plain reference of include/gridvision_hip.h's definition.
Philox4x32-10 in numpy uint64 arithmetic (every product of two 32-bit words fits), Box-Muller with Python floats (IEEE
doubles, one rounding per operation, nothing contracted) and math.log / math.sin / math.cos / math.exp -- the C library's,
NOT numpy's vectorised fp64 functions, which need not equal it -- the clamp in float32, and the average as sequential fp64
sums over the admitted trajectories in index order."""
import math

import numpy as np

SHIFT = 1 << 0
U64 = (1 << 64) - 1
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
TWO_PI = 6.283185307179586


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two ints.  Returns uint32 (..., 4)."""
    c = [np.asarray(v, np.uint64) & LO for v in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & LO, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & LO]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def words(seed, iteration, k, p):
    """the words of pose (k, p): counter (k, p, iteration_lo, iteration_hi), key (seed_lo, seed_hi)"""
    return philox4x32_10((k, p, iteration & 0xFFFFFFFF, (iteration >> 32) & 0xFFFFFFFF), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def _uniform(r):
    return (float(r) + 0.5) * 2.0 ** -32


def normals(r, C):
    """z_0 .. z_{C-1} of one pose's four words"""
    R = math.sqrt(-2.0 * math.log(_uniform(r[0])))
    A = TWO_PI * _uniform(r[1])
    z = [R * math.cos(A), R * math.sin(A)]
    if C == 3:
        R2 = math.sqrt(-2.0 * math.log(_uniform(r[2])))
        A2 = TWO_PI * _uniform(r[3])
        z.append(R2 * math.cos(A2))
    return z


def sample(sigma, u_min, u_max, nominal, K, seed, iteration, flags=0, parts=False):
    """nominal float32 (P, C).  Returns float32 (K, P, C); with parts also the fp64 (K, P, C) arrays of |v| and
    |sigma * z| before the rounding (rows k >= 1), for the cancellation guard."""
    nominal = np.asarray(nominal, np.float32)
    P, C = nominal.shape
    lo, hi = np.asarray(u_min, np.float32), np.asarray(u_max, np.float32)
    w = words(seed, iteration, np.arange(K)[:, None], np.arange(P)[None, :]) if K else np.zeros((0, P, 4), np.uint32)
    v = np.zeros((K, P, C), np.float64)
    noise = np.zeros((K, P, C), np.float64)
    for k in range(K):
        for p in range(P):
            pn = min(p + 1, P - 1) if flags & SHIFT else p
            z = normals([int(t) for t in w[k, p]], C) if k else None
            for c in range(C):
                if k:
                    noise[k, p, c] = float(sigma[c]) * z[c]
                    v[k, p, c] = float(nominal[pn, c]) + noise[k, p, c]
                else:
                    v[k, p, c] = float(nominal[pn, c])
    with np.errstate(over="ignore"):
        f = v.astype(np.float32)
    f = np.where(f < lo[:C], lo[:C], f)
    f = np.where(f > hi[:C], hi[:C], f).astype(np.float32)
    return (f, np.abs(v), np.abs(noise)) if parts else f


def weights(totals, lam):
    """(e (K,) fp64 with -1 for a rejected trajectory, best_total) or (None, U64) when every trajectory is rejected"""
    t = [int(v) for v in totals]
    admitted = [v for v in t if v != U64]
    if not admitted:
        return None, U64
    best = min(admitted)
    e = np.full(len(t), -1.0)
    for k, v in enumerate(t):
        if v != U64:
            e[k] = math.exp(-(float(v - best) / float(lam)))
    return e, best


def average(lam, controls, totals, nominal, bound=False):
    """controls float32 (K, P, C), totals uint64 (K,), nominal float32 (P, C).  The new nominal float32 (P, C): all
    columns at once, trajectory after trajectory, which is the sequential sum of every column.  With bound also the
    fp64 quotient N / S before its rounding to float32 and A = sum e_k |u| / S per component (fp64), the scale of the
    reordering bound."""
    controls = np.asarray(controls, np.float32)
    nominal = np.asarray(nominal, np.float32)
    e, _ = weights(totals, lam)
    if e is None:
        return (nominal.copy(), nominal.astype(np.float64), np.zeros(nominal.shape)) if bound else nominal.copy()
    N, A, S = np.zeros(nominal.shape), np.zeros(nominal.shape), 0.0
    for k in range(len(controls)):
        if e[k] >= 0.0:
            u = controls[k].astype(np.float64)
            S = S + float(e[k])
            N = N + float(e[k]) * u
            A = A + float(e[k]) * np.abs(u)
    out = (N / S).astype(np.float32)
    return (out, N / S, A / S) if bound else out
