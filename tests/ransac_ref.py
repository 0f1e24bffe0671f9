"""The RANSAC ground plane (k_ransac_count_all -> k_ransac_moments -> k_ransac_mask, gv_ransac.hip / k_pose_classify, gv_cloudops.hip)
restated in numpy and Python floats, no C: the contract the device is held to byte for byte (tests/test_gpu_ransac.py)
and that tests/test_ransac_host.py holds to oracle/ransac.c on every fixture.

  draws       hypothesis t takes the points splitmix64(seed + 3 t + k) mod n, k = 0, 1, 2
  transform   ox = x m0 + (y m1 + (z m2 + m3)), every operation one float32 operation (xform34)
  plane       finiteness of the nine coordinates; the ratios r = (p1 - p0) / (p2 - p0) and r0 != r1 or r2 != r1; the cross
              product; len = sqrt((a + b) + c), len > 0 and finite; three divides; d = -1 (((n0 p0x) + n1 p0y) + n2 p0z)
  inlier      fabs((((a x) + b y) + c z) + d) < thr_f, thr_f the smallest float32 >= the fp64 threshold
  selection   the inlier count of EVERY hypothesis; the highest wins, the lowest index among equals, none if all are zero
  moments     count, Sx Sy Sz, Qxx Qxy Qxz Qyy Qyz Qzz of the winner's inliers in fp64 (products of two float32 are exact),
              every sum by the fixed 64-ary butterfly tree over the cloud order, at least one level
  refinement  centroid, Q / m - c c^T, the closed-form eigenvector of oracle/ransac.c, narrowed to float32; fewer than
              three inliers keep the sampled plane
  mask        inliers of the refined plane, and their number

Two switches exist only so that the CPU test can prove a fixture is sensitive: `sum` ("tree", "sequential", "fsum", and
"rows-swapped" / "dpp-reversed": the tree with two of its steps in another order, what a slip in the kernel would give) and
`contract` (the distance with its multiply-adds fused: product exact in fp64, one rounding)."""
import math
from collections import namedtuple

import numpy as np

F32 = np.float32
U64 = np.uint64

Result = namedtuple("Result", "best_index best_count plane m refined mask n_inliers counts margin moments")


# ------------------------------------------------------------------------------------------------- the draws --

def splitmix64(z):
    z = np.asarray(z, U64)
    with np.errstate(over="ignore"):
        z = z + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def draws(n, iters, seed):
    """int64[iters, 3]: the point indices hypothesis t samples"""
    with np.errstate(over="ignore"):
        c = U64(seed) + U64(3) * np.arange(iters, dtype=U64)[:, None] + np.arange(3, dtype=U64)[None, :]
    return (splitmix64(c) % U64(n)).astype(np.int64)


# ---------------------------------------------------------------------------------------- transform and plane --

def xform34(m, x, y, z):
    """the device's transform: m = float32[12] (or the oracle's 4 x 4 as float32[16]), one float32 operation each"""
    m = np.asarray(m, F32).reshape(-1)
    x, y, z = (np.ascontiguousarray(a, F32) for a in (x, y, z))
    with np.errstate(all="ignore"):
        return tuple(x * m[4 * r] + (y * m[4 * r + 1] + (z * m[4 * r + 2] + m[4 * r + 3])) for r in range(3))


def planes_of(cx, cy, cz, idx):
    """float32[iters, 4] planes of the samples idx[iters, 3] (camera frame), ok[iters]; an unusable sample's plane is NaN"""
    P = np.stack([cx[idx], cy[idx], cz[idx]], axis=2).astype(F32)   # [t, k, coordinate]
    p0, p1, p2 = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        ok = np.isfinite(P).all(axis=(1, 2))
        a, b = p1 - p0, p2 - p0
        r = a / b
        ok &= (r[:, 0] != r[:, 1]) | (r[:, 2] != r[:, 1])
        n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                      a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        ok &= (ln > 0) & np.isfinite(ln)
        n = n / ln[:, None]
        d = F32(-1.0) * (((n[:, 0] * p0[:, 0]) + n[:, 1] * p0[:, 1]) + n[:, 2] * p0[:, 2])
    pl = np.concatenate([n, d[:, None]], axis=1).astype(F32)
    pl[~ok] = np.nan
    return pl, ok


def ceil_to_float(thr):
    """the smallest float32 >= the fp64 threshold: for a float32 f, f < thr_f <=> (double) f < thr"""
    f = F32(thr)
    return f if float(f) >= float(thr) else np.nextafter(f, F32(np.inf))


def distance(pl, cx, cy, cz, contract=False):
    """float32 signed distance (((a x) + b y) + c z) + d; contract: the two multiply-adds fused"""
    a, b, c, d = (F32(v) for v in pl)
    with np.errstate(all="ignore"):
        if not contract:
            return (((a * cx) + b * cy) + c * cz) + d
        t = a * cx
        t = (np.float64(b) * cy.astype(np.float64) + t.astype(np.float64)).astype(F32)
        t = (np.float64(c) * cz.astype(np.float64) + t.astype(np.float64)).astype(F32)
        return t + d


def inliers(pl, cx, cy, cz, thr_f, contract=False):
    with np.errstate(all="ignore"):
        return np.abs(distance(pl, cx, cy, cz, contract)) < thr_f   # NaN -> False


# -------------------------------------------------------------------------------------------------- the sums --

def tree_sum64(v):
    """the 64-ary butterfly tree over v (fp64): groups of 64 consecutive values, the last padded with +0.0, reduced by
    t[i] += t[i + off], off = 32 .. 1; the group sums form the next level; at least one level"""
    v = np.asarray(v, np.float64)
    if len(v) == 0:
        return 0.0
    while True:
        g = (len(v) + 63) // 64
        t = np.zeros(g * 64, np.float64)
        t[:len(v)] = v
        t = t.reshape(g, 64)
        off = 32
        while off:
            t[:, :off] += t[:, off:2 * off]
            off >>= 1
        v = t[:, 0].copy()
        if g == 1:
            return float(v[0])


def tree_sum64_steps(v, steps_of_level):
    """tree_sum64 with the butterfly's steps taken as the device takes them -- v[i] += v[i + off] across the 64 values
    for off >= 16, inside each row of 16 for off < 16 -- in the order steps_of_level(level) gives: the planted mistakes
    "cross-row steps swapped" and "row steps reversed" as a sum order of their own"""
    v = np.asarray(v, np.float64)
    level = 0
    while True:
        g = (len(v) + 63) // 64
        t = np.zeros(g * 64, np.float64)
        t[:len(v)] = v
        t = t.reshape(g, 64)
        for off in steps_of_level(level):
            new = t.copy()
            if off >= 16:
                new[:, :64 - off] = t[:, :64 - off] + t[:, off:]
            else:
                rows, nrows = t.reshape(g, 4, 16), new.reshape(g, 4, 16)
                nrows[:, :, :16 - off] = rows[:, :, :16 - off] + rows[:, :, off:]
            t = new
        v = t[:, 0].copy()
        level += 1
        if g == 1:
            return float(v[0])


STEP_ORDERS = {"steps": lambda level: (32, 16, 8, 4, 2, 1),                                         # = "tree"
               "rows-swapped": lambda level: (32, 16, 8, 4, 2, 1) if level == 0 else (16, 32, 8, 4, 2, 1),   # wave_butterfly
               "dpp-reversed": lambda level: (32, 16, 1, 2, 4, 8) if level == 0 else (32, 16, 8, 4, 2, 1)}   # the level-0 sum


def _sum(v, how):
    if how == "tree":
        return tree_sum64(v)
    if how in STEP_ORDERS:
        return tree_sum64_steps(v, STEP_ORDERS[how])
    nz = v[v != 0.0]   # a zero changes no sequential or exact sum
    if how == "sequential":
        return float(np.cumsum(nz)[-1]) if len(nz) else 0.0
    if how == "fsum":
        return math.fsum(nz.tolist())
    raise ValueError(how)


def raw_moments(cx, cy, cz, inl, how="tree"):
    """Sx Sy Sz Qxx Qxy Qxz Qyy Qyz Qzz of the points inl marks, a non-inlier contributing +0.0"""
    X, Y, Z = (np.where(inl, a, F32(0)).astype(np.float64) for a in (cx, cy, cz))
    out = []
    for k in range(9):
        v = (X, Y, Z, None, None, None, None, None, None)[k]
        if v is None:
            p, q = ((X, X), (X, Y), (X, Z), (Y, Y), (Y, Z), (Z, Z))[k - 3]
            v = p * q
        out.append(_sum(v, how))
    return out


# -------------------------------------------------------------------------------------------- the eigenvector --

def smallest_eigenvector3(cov):
    """oracle/ransac.c gvo_smallest_eigenvector3, operation for operation in Python floats (fp64)"""
    a = [[cov[0], cov[1], cov[2]], [cov[1], cov[3], cov[4]], [cov[2], cov[4], cov[5]]]
    scale = 0.0
    for i in range(3):
        for j in range(3):
            if abs(a[i][j]) > scale:
                scale = abs(a[i][j])
    if not (scale > 2.2250738585072014e-308):
        scale = 1.0
    a = [[a[i][j] / scale for j in range(3)] for i in range(3)]
    c0 = (((a[0][0] * a[1][1]) * a[2][2] + (2.0 * a[0][1]) * a[0][2] * a[1][2]) - (a[0][0] * a[1][2]) * a[1][2]
          - (a[1][1] * a[0][2]) * a[0][2]) - (a[2][2] * a[0][1]) * a[0][1]
    c1 = ((((a[0][0] * a[1][1] - a[0][1] * a[0][1]) + a[0][0] * a[2][2]) - a[0][2] * a[0][2]) + a[1][1] * a[2][2]) \
        - a[1][2] * a[1][2]
    c2 = (a[0][0] + a[1][1]) + a[2][2]
    c2_over_3 = c2 * (1.0 / 3.0)
    a_over_3 = (c2 * c2_over_3 - c1) * (1.0 / 3.0)
    if a_over_3 < 0.0:
        a_over_3 = 0.0
    half_b = 0.5 * (c0 + c2_over_3 * (2.0 * c2_over_3 * c2_over_3 - c1))
    q = a_over_3 * a_over_3 * a_over_3 - half_b * half_b
    if q < 0.0:
        q = 0.0
    rho = math.sqrt(a_over_3)
    theta = math.atan2(math.sqrt(q), half_b) * (1.0 / 3.0)
    cos_theta, sin_theta = math.cos(theta), math.sin(theta)
    r0 = c2_over_3 + 2.0 * rho * cos_theta
    r1 = c2_over_3 - rho * (cos_theta + 1.7320508075688772 * sin_theta)
    r2 = c2_over_3 - rho * (cos_theta - 1.7320508075688772 * sin_theta)
    lam = r0
    if r1 < lam:
        lam = r1
    if r2 < lam:
        lam = r2
    if lam <= 0.0:
        lam = 0.0
    a[0][0] -= lam
    a[1][1] -= lam
    a[2][2] -= lam
    v1 = [a[0][1] * a[1][2] - a[0][2] * a[1][1], a[0][2] * a[1][0] - a[0][0] * a[1][2], a[0][0] * a[1][1] - a[0][1] * a[1][0]]
    v2 = [a[0][1] * a[2][2] - a[0][2] * a[2][1], a[0][2] * a[2][0] - a[0][0] * a[2][2], a[0][0] * a[2][1] - a[0][1] * a[2][0]]
    v3 = [a[1][1] * a[2][2] - a[1][2] * a[2][1], a[1][2] * a[2][0] - a[1][0] * a[2][2], a[1][0] * a[2][1] - a[1][1] * a[2][0]]
    l1 = (v1[0] * v1[0] + v1[1] * v1[1]) + v1[2] * v1[2]
    l2 = (v2[0] * v2[0] + v2[1] * v2[1]) + v2[2] * v2[2]
    l3 = (v3[0] * v3[0] + v3[1] * v3[1]) + v3[2] * v3[2]
    if l1 >= l2 and l1 >= l3:
        n, len2 = v1, l1
    elif l2 >= l1 and l2 >= l3:
        n, len2 = v2, l2
    else:
        n, len2 = v3, l3
    ln = math.sqrt(len2)
    big = 0
    if abs(n[1]) > abs(n[big]):
        big = 1
    if abs(n[2]) > abs(n[big]):
        big = 2
    with np.errstate(all="ignore"):
        sg = float(np.float64(-1.0) / np.float64(ln)) if n[big] < 0 else float(np.float64(1.0) / np.float64(ln))
    return [n[0] * sg, n[1] * sg, n[2] * sg]


def f32_boundary_margin(v):
    """relative distance of the fp64 value v from the nearest float32 rounding boundary (the midpoint of two neighbouring
    float32 values): how far v is from narrowing to another float32"""
    v = float(v)
    if v == 0.0 or not math.isfinite(v):
        return math.inf
    f = F32(v)
    lo, hi = float(np.nextafter(f, F32(-np.inf))), float(np.nextafter(f, F32(np.inf)))
    f = float(f)
    return min(abs(v - 0.5 * (f + lo)), abs(v - 0.5 * (f + hi))) / abs(v)


def refine(cx, cy, cz, pl, inl, how="tree"):
    """(refined float32[4], margins[4], moments) from the inliers inl of the sampled plane pl"""
    m = int(np.count_nonzero(inl))
    if m < 3:
        return np.asarray(pl, F32).copy(), [math.inf] * 4, None
    mom = raw_moments(cx, cy, cz, inl, how)
    dm = float(m)
    c = [mom[0] / dm, mom[1] / dm, mom[2] / dm]
    cov = [mom[3] / dm - c[0] * c[0], mom[4] / dm - c[0] * c[1], mom[5] / dm - c[0] * c[2],
           mom[6] / dm - c[1] * c[1], mom[7] / dm - c[1] * c[2], mom[8] / dm - c[2] * c[2]]
    nv = smallest_eigenvector3(cov)
    vals = [nv[0], nv[1], nv[2], -((nv[0] * c[0] + nv[1] * c[1]) + nv[2] * c[2])]
    with np.errstate(all="ignore"):
        return np.array(vals, np.float64).astype(F32), [f32_boundary_margin(v) for v in vals], mom


# ------------------------------------------------------------------------------------------------ whole call --

def all_counts(planes, cx, cy, cz, thr_f, contract=False, chunk=1 << 22):
    """int64[iters]: the inlier count of every hypothesis (a NaN plane collects none)"""
    out = np.zeros(len(planes), np.int64)
    for t in np.flatnonzero(~np.isnan(planes[:, 0])):
        for s in range(0, len(cx), chunk):
            e = s + chunk
            out[t] += np.count_nonzero(inliers(planes[t], cx[s:e], cy[s:e], cz[s:e], thr_f, contract))
    return out


def select(counts):
    """(index, count) of the highest count, the lowest index among equals; (-1, 0) if all are zero"""
    if len(counts) == 0 or counts.max() == 0:
        return -1, 0
    t = int(np.argmax(counts))   # the first of the maxima
    return t, int(counts[t])


def segment(x, y, z, tf, threshold=0.04, iters=50, seed=12345, sum="tree", contract=False):
    """the whole call on the uploaded (lidar-frame) cloud x, y, z under the float32 lidar -> camera matrix tf (its 12 or
    16 entries by rows, as the library derives them from cam_lidar): a Result"""
    n = len(x)
    zero = np.zeros(4, F32)
    mask = np.zeros(n, np.uint8)
    if n < 3:
        return Result(-1, 0, zero, 0, zero.copy(), mask, 0, np.zeros(iters, np.int64), [math.inf] * 4, None)
    cx, cy, cz = xform34(tf, x, y, z)
    thr_f = ceil_to_float(threshold)
    planes, _ = planes_of(cx, cy, cz, draws(n, iters, seed))
    counts = all_counts(planes, cx, cy, cz, thr_f, contract)
    best, bc = select(counts)
    if bc == 0:
        return Result(-1, 0, zero, 0, zero.copy(), mask, 0, counts, [math.inf] * 4, None)
    pl = planes[best].copy()
    inl = inliers(pl, cx, cy, cz, thr_f, contract)
    refined, margin, mom = refine(cx, cy, cz, pl, inl, sum)
    mask = inliers(refined, cx, cy, cz, thr_f, contract).astype(np.uint8)
    return Result(best, bc, pl, int(np.count_nonzero(inl)), refined, mask, int(mask.sum()), counts, margin, mom)
