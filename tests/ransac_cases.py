"""Fixture families for the RANSAC ground plane (tests/test_ransac_host.py proves on the CPU that each reaches its edge,
tests/test_gpu_ransac.py holds the device to tests/ransac_ref.py on them).  Every family is deterministic; a case is
(tag, x, y, z in the lidar frame, cam_lidar transform, threshold, iterations, seed, meta).

  A threshold   the plane z = 0 exactly (identity transform, integer x and y, so |distance| = |z| for the sampled AND the
                refined plane), points with |z| = pred(thr_f), thr_f, succ(thr_f) in both signs, for a threshold whose
                float lies below it (0.04), above it (0.3), on it (0.5) and in the denormal range (2^-140)
  B rounding    a tilted noisy ground under the perturbed transform with points whose side of the sampled plane, and
                others whose side of the refined plane, depends on whether a multiply-add is fused
  C ties        parallel exact planes of equal population: tied hypotheses on DIFFERENT planes, across lanes and launches
  D degenerate  collinear / identical / tiny / all-NaN clouds, non-finite points that hypotheses draw, an infinite x
                that is still infinite, not NaN, when it meets a zero normal component
  E sum order   a 2 m patch 1 km and 10 km from the origin at the sizes where the sum tree changes shape
  G steps       the patch 65 km out, once across a power of two: two butterfly steps in another order change bytes
  F general     16 781 313 points: 4098 workgroups, the ping-pong tree with levels 4098 -> 65 -> 2 -> 1

Edge points are written into slots no hypothesis draws (undrawn()), so the hypotheses stay what they were."""
from collections import namedtuple

import numpy as np

import oracle_lib as ol
import ransac_ref as R
from gvamd import synth
from knn_depth_ref import IDENT_TF

F32 = np.float32
Case = namedtuple("Case", "tag x y z tf thr iters seed meta")
POSE = dict(thr=0.04, iters=50, seed=12345)   # what gv_compute_bbox_pose_ground_removed and the tick fix
PERTURBED_TF = synth.transforms(True)["cam_lidar"]
_REF, _MAT = {}, {}


def matrix(case):
    key = tuple(np.asarray(case.tf, np.float64))
    if key not in _MAT:
        _MAT[key] = ol.tf_to_matrix4f(case.tf)
    return _MAT[key]


def reference(case, **kw):
    """ransac_ref.segment of the case; the default (tree, not contracted) result is computed once and shared"""
    if kw:
        return R.segment(case.x, case.y, case.z, matrix(case), case.thr, case.iters, case.seed, **kw)
    if case.tag not in _REF:
        _REF[case.tag] = R.segment(case.x, case.y, case.z, matrix(case), case.thr, case.iters, case.seed)
    return _REF[case.tag]


def camera(case):
    return R.xform34(matrix(case), case.x, case.y, case.z)


def undrawn(n, iters, seed):
    """bool[n]: the slots no hypothesis samples"""
    free = np.ones(n, bool)
    free[R.draws(n, iters, seed).reshape(-1)] = False
    return free


def _case(tag, x, y, z, tf, thr=0.04, iters=50, seed=12345, **meta):
    x, y, z = (np.ascontiguousarray(a, F32) for a in (x, y, z))
    return Case(tag, x, y, z, np.asarray(tf, np.float64), float(thr), int(iters), int(seed), meta)


# ------------------------------------------------------------------------------------------- A: threshold edge --

THRESHOLDS = (("0.04", 0.04), ("0.3", 0.3), ("0.5", 0.5), ("denormal", 2.0 ** -140))
EDGE_PER = 40   # points per distance and sign


def _flat_cloud(rng, n, n_ground):
    """integer x, y; z = 0 on n_ground points and 1 <= |z| <= 5 on the rest, in a random order"""
    x = rng.integers(-50, 51, n).astype(F32)
    y = rng.integers(-50, 51, n).astype(F32)
    z = np.zeros(n, F32)
    k = n - n_ground
    z[n_ground:] = (rng.uniform(1.0, 5.0, k) * rng.choice([-1.0, 1.0], k)).astype(F32)
    p = rng.permutation(n)
    return x[p], y[p], z[p]


def threshold_case(name, thr, n=3000):
    rng = np.random.default_rng(101)
    x, y, z = _flat_cloud(rng, n, 1800)
    thr_f = R.ceil_to_float(thr)
    dist = {"pred": np.nextafter(thr_f, F32(0)), "at": thr_f, "succ": np.nextafter(thr_f, F32(np.inf))}
    free = np.flatnonzero(undrawn(n, 50, 12345) & (z != 0))
    assert len(free) >= 6 * EDGE_PER
    edge, k = {}, 0
    for key, e in dist.items():
        pos, neg = free[k:k + EDGE_PER], free[k + EDGE_PER:k + 2 * EDGE_PER]
        k += 2 * EDGE_PER
        z[pos], z[neg] = e, -e
        x[neg], y[neg] = x[pos], y[pos]   # mirror pairs: Sz, Qxz and Qyz stay exactly zero, the refined plane is z = 0
        edge[key] = np.concatenate([pos, neg])
    return _case("threshold-" + name, x, y, z, IDENT_TF, thr, edge=edge, thr_f=thr_f, dist=dist)


def threshold_cases():
    return [threshold_case(name, thr) for name, thr in THRESHOLDS]


# -------------------------------------------------------------------------------------- B: rounding-sensitive --

N_FLIP = 96       # >= 64 asked for
N_SAMPLED = 400   # on the sampled plane: enough to keep the winner ahead of the hypotheses next to it


def _crossings(m, pl, thr_f, x, y, sign, zlo=-40.0, zhi=40.0):
    """lidar z, per (x, y), of the two neighbouring floats between which the signed distance to pl crosses sign * thr_f
    (float32 bisection); ok marks the columns that had a crossing"""
    def f(zl):
        return R.distance(pl, *R.xform34(m, x, y, zl)).astype(np.float64) - sign * float(thr_f)
    lo, hi = np.full(len(x), zlo, F32), np.full(len(x), zhi, F32)
    flo, fhi = f(lo), f(hi)
    ok = np.isfinite(flo) & np.isfinite(fhi) & ((flo < 0) != (fhi < 0))
    for _ in range(64):
        mid = ((lo.astype(np.float64) + hi.astype(np.float64)) * 0.5).astype(F32)
        s = (f(mid) < 0) == (flo < 0)
        lo, hi = np.where(s, mid, lo), np.where(s, hi, mid)
    return lo, hi, ok


def _flip_points(m, pl, thr_f, rng, count, xr, yr, accept=None):
    """count lidar points that are inliers of pl as the contract rounds (every product and sum on its own) and outliers
    with the multiply-adds fused"""
    xs, ys, zs = [], [], []
    for _ in range(40):
        if sum(len(a) for a in xs) >= count:
            break
        k = 20000
        x = rng.uniform(*xr, k).astype(F32)
        y = rng.uniform(*yr, k).astype(F32)
        for sign in (1.0, -1.0):
            lo, hi, ok = _crossings(m, pl, thr_f, x, y, sign)
            for zl in (lo, hi):
                cam = R.xform34(m, x, y, zl)
                take = ok & R.inliers(pl, *cam, thr_f) & ~R.inliers(pl, *cam, thr_f, contract=True)
                if accept is not None:
                    take &= accept(cam)
                xs.append(x[take]); ys.append(y[take]); zs.append(zl[take])
    assert sum(len(a) for a in xs) >= count, "too few rounding-sensitive points"
    return tuple(np.concatenate(a)[:count] for a in (xs, ys, zs))


def ground_scene(rng, n_ground=60_000, n_clusters=8, pts_per=300, n_clutter=6000):
    """a tilted ground with 2 cm noise (lidar z up), clusters above it and clutter; returns x, y, z and the clutter's
    index range"""
    gx = rng.uniform(1.0, 60.0, n_ground)
    gy = rng.uniform(-40.0, 40.0, n_ground)
    gz = -1.3 + 0.01 * gx + rng.uniform(-0.02, 0.02, n_ground)
    xs, ys, zs = [gx], [gy], [gz]
    for _ in range(n_clusters):
        c = rng.uniform(6.0, 45.0)
        cy, cz = rng.uniform(-0.5, 0.5) * c, rng.uniform(-0.6, 0.5)
        xs.append(c + rng.uniform(-0.7, 0.7, pts_per))
        ys.append(cy + rng.uniform(-0.5, 0.5, pts_per))
        zs.append(cz + rng.uniform(-0.4, 0.4, pts_per))
    xs.append(rng.uniform(-20, 60, n_clutter)); ys.append(rng.uniform(-40, 40, n_clutter)); zs.append(rng.uniform(-2, 3, n_clutter))
    x, y, z = (np.concatenate(a).astype(F32) for a in (xs, ys, zs))
    return x, y, z, (len(x) - n_clutter, len(x))


ROUNDING_RNG = 202   # the scene's generator seed (the first tried)


def rounding_case(rng_seed=None):
    rng = np.random.default_rng(ROUNDING_RNG if rng_seed is None else rng_seed)
    x0, y0, z0, (c0, c1) = ground_scene(rng)
    m = ol.tf_to_matrix4f(PERTURBED_TF)
    thr_f = R.ceil_to_float(0.04)
    free = np.flatnonzero(undrawn(len(x0), POSE["iters"], POSE["seed"]))
    free = free[(free >= c0) & (free < c1) & (z0[free] > 0.5)]   # clutter well above the ground: no plane's inliers
    s_slots, r_slots = free[:N_SAMPLED], free[N_SAMPLED:N_SAMPLED + N_FLIP]
    planes, _ = R.planes_of(*R.xform34(m, x0, y0, z0), R.draws(len(x0), 50, 12345))   # no slot below is drawn
    winner = R.segment(x0, y0, z0, m, 0.04, 50, 12345).best_index
    for _ in range(4):   # the planted points may hand the lead to a neighbouring hypothesis: then plant for that one
        x, y, z = x0.copy(), y0.copy(), z0.copy()
        # 1. the sampled plane's points, inside the scene
        x[s_slots], y[s_slots], z[s_slots] = _flip_points(m, planes[winner], thr_f, rng, N_SAMPLED, (1.0, 60.0), (-40.0, 40.0))
        mid = R.segment(x, y, z, m, 0.04, 50, 12345)
        # 2. the refined plane's points: outliers of the sampled plane (by half a threshold at least, fused or not), which
        # is centimetres away far from the centroid -- the moments and the refined plane do not move
        # ... and inside the image, so that the ground test of k_pose_classify decides whether a box selects them
        def off_sampled(cam):
            with np.errstate(all="ignore"):
                u, v = 320.0 + 320.0 * cam[0] / cam[2], 240.0 + 320.0 * cam[1] / cam[2]
            seen = (cam[2] > 1.0) & (u > 1.0) & (u < 639.0) & (v > 1.0) & (v < 479.0)
            return seen & (np.abs(R.distance(mid.plane, *cam).astype(np.float64)) > 1.5 * float(thr_f))
        x[r_slots], y[r_slots], z[r_slots] = _flip_points(m, mid.refined, thr_f, rng, N_FLIP, (-150.0, 250.0), (-200.0, 200.0),
                                                          accept=off_sampled)
        end = R.segment(x, y, z, m, 0.04, 50, 12345)
        if end.best_index == mid.best_index == winner and end.refined.tobytes() == mid.refined.tobytes():
            break
        winner = end.best_index
    else:
        raise AssertionError("two hypotheses keep trading the lead: take another scene seed")
    case = _case("rounding", x, y, z, PERTURBED_TF, sampled_edge=s_slots, refined_edge=r_slots, winner=winner)
    _REF[case.tag] = end
    return case


# --------------------------------------------------------------------------------------------------- C: ties --

PLANE_Z = (0.0, 1.0)


def tie_cloud(n, per_plane, rng_seed):
    """per_plane points on each of the planes z = 0 and z = 1 (integer x, y), the rest clutter at 3 <= z <= 50"""
    rng = np.random.default_rng(rng_seed)
    x = rng.integers(-50, 51, n).astype(F32)
    y = rng.integers(-50, 51, n).astype(F32)
    z = rng.uniform(3.0, 50.0, n).astype(F32)
    cls = np.zeros(n, np.int8)
    p = rng.permutation(n)
    for k, pz in enumerate(PLANE_Z):
        s = p[k * per_plane:(k + 1) * per_plane]
        z[s], cls[s] = pz, k + 1
    clutter = cls == 0
    x[clutter] = rng.uniform(-50, 50, clutter.sum()).astype(F32)
    y[clutter] = rng.uniform(-50, 50, clutter.sum()).astype(F32)
    return x, y, z, cls


def plane_hypotheses(x, y, cls, iters, seed):
    """int8[iters]: 1 or 2 where hypothesis t samples three non-collinear points of that plane, else 0"""
    idx = R.draws(len(x), iters, seed)
    c = cls[idx]
    same = (c[:, 0] == c[:, 1]) & (c[:, 1] == c[:, 2]) & (c[:, 0] > 0)
    ax, ay = x[idx[:, 1]] - x[idx[:, 0]], y[idx[:, 1]] - y[idx[:, 0]]
    bx, by = x[idx[:, 2]] - x[idx[:, 0]], y[idx[:, 2]] - y[idx[:, 0]]
    return np.where(same & (ax * by - ay * bx != 0), c[:, 0], 0).astype(np.int8)


def tie_relation(kind, hyp):
    """(t1, t2) of the tie `kind` asks for among the plane hypotheses hyp, or None.  t1: the first of them (the winner),
    t2: a later one on the OTHER plane with
      'lane'    t1 % 64 > t2 % 64, both in the first launch when there are two
      'launch'  t1 < 2048 <= t2
      'second'  t1 >= 2048 and t1 % 64 > t2 % 64"""
    good = np.flatnonzero(hyp)
    if not len(good):
        return None
    t1 = int(good[0])
    later = good[(good > t1) & (hyp[good] != hyp[t1])]
    if kind == "lane":
        later = later[(later % 64 < t1 % 64) & (later < 2048)]
    elif kind == "launch":
        later = later[later >= 2048] if t1 < 2048 else later[:0]
    elif kind == "second":
        later = later[later % 64 < t1 % 64] if t1 >= 2048 else later[:0]
    return (t1, int(later[0])) if len(later) else None


# (tag, n, points per plane, iterations, relation, seed): the seeds are the first that find_tie_seed finds
TIES = (("dense-50", 2000, 1000, 50, "any", 12345),
        ("lane-4096", 2000, 160, 4096, "lane", 66),
        ("launch-4096", 2000, 160, 4096, "launch", 2),
        ("second-4096", 2000, 160, 4096, "second", 9796))


def find_tie_seed(n, per_plane, iters, kind, start=1, tries=200_000):
    x, y, z, cls = tie_cloud(n, per_plane, 303)
    for seed in range(start, start + tries):
        hyp = plane_hypotheses(x, y, cls, iters, seed)
        if kind == "any":
            good = np.flatnonzero(hyp)
            if len(good) >= 2 and good[0] >= 1 and (hyp[good] != hyp[good[0]]).any():
                return seed
        elif tie_relation(kind, hyp) is not None:
            return seed
    raise AssertionError("no seed")


def tie_case(tag, n, per_plane, iters, kind, seed):
    x, y, z, cls = tie_cloud(n, per_plane, 303)
    return _case("tie-" + tag, x, y, z, IDENT_TF, 0.04, iters, seed, cls=cls, kind=kind, per_plane=per_plane)


def tie_cases():
    return [tie_case(*t) for t in TIES]


# ------------------------------------------------------------------------------- D: degenerate and non-finite --

def _good_cloud(n=5000, rng_seed=404):
    return _flat_cloud(np.random.default_rng(rng_seed), n, 3000)


def nonfinite_case():
    """the good cloud with NaN, +inf and -inf written into slots that hypotheses DO draw (never the winner's)"""
    x, y, z = _good_cloud()
    idx = R.draws(len(x), POSE["iters"], POSE["seed"])
    base = R.segment(x, y, z, ol.tf_to_matrix4f(IDENT_TF), 0.04, 50, 12345)
    keep = set(idx[base.best_index].tolist())
    hit = []
    for t, (val, coord) in zip((t for t in range(POSE["iters"]) if not (set(idx[t].tolist()) & keep)),
                               [(np.nan, 0), (np.inf, 1), (-np.inf, 2), (np.nan, 2), (np.inf, 0), (-np.inf, 1)] * 2):
        s = idx[t][len(hit) % 3]
        (x, y, z)[coord][s] = val
        hit.append(int(s))
    free = np.flatnonzero(undrawn(len(x), 50, 12345))[:30]
    for k, s in enumerate(free):   # and more of them that nobody draws
        (x, y, z)[k % 3][s] = (np.nan, np.inf, -np.inf)[(k // 3) % 3]
    return _case("nonfinite", x, y, z, IDENT_TF, planted=np.array(hit), base=base)


INF_X_PLANE = 8.0   # a power of two: c * Sy is the tree sum of the c * y exactly, so the refined plane is exact too


def inf_x_case(n=5000, n_plane=3000):
    """The plane camera x = 8 exactly under the PERTURBED transform, whose first column has no zero: a point with lidar
    x = +-inf is (+-inf, +-inf, +-inf) in the camera frame, no NaN yet, and the planes' normal is (+-1, 0, 0) with y and z
    components exactly 0 (three samples of equal camera x) -- 0 * inf = NaN INSIDE the plane evaluation.  The plane's
    points are found by bisection on lidar y until the float32 camera x is 8.0 itself."""
    rng = np.random.default_rng(405)
    m = ol.tf_to_matrix4f(PERTURBED_TF)
    c = F32(INF_X_PLANE)
    xs, ys, zs = [], [], []
    while sum(len(a) for a in xs) < n_plane:
        k = 4 * n_plane
        x = rng.uniform(10.0, 60.0, k).astype(F32)
        z = rng.uniform(-3.0, 3.0, k).astype(F32)
        lo, hi = np.full(k, -40.0, F32), np.full(k, 40.0, F32)      # camera x falls as lidar y rises
        for _ in range(64):
            mid = ((lo.astype(np.float64) + hi.astype(np.float64)) * 0.5).astype(F32)
            above = R.xform34(m, x, mid, z)[0] > c
            lo, hi = np.where(above, mid, lo), np.where(above, hi, mid)
        hit = R.xform34(m, x, hi, z)[0] == c
        xs.append(x[hit]); ys.append(hi[hit]); zs.append(z[hit])
    x, y, z = (np.concatenate(a)[:n_plane] for a in (xs, ys, zs))
    k = n - n_plane
    x = np.concatenate([x, rng.uniform(10.0, 60.0, k).astype(F32)])
    y = np.concatenate([y, rng.uniform(-30.0, 30.0, k).astype(F32)])
    z = np.concatenate([z, rng.uniform(-3.0, 3.0, k).astype(F32)])
    near = np.abs(R.xform34(m, x, y, z)[0] - c) < 1.0     # no chance inlier: the plane's inliers all have camera x = 8
    near[:n_plane] = False
    y[near] += F32(15.0)
    p = rng.permutation(n)
    x, y, z = x[p], y[p], z[p]
    on_plane = R.xform34(m, x, y, z)[0] == c
    free = np.flatnonzero(undrawn(n, 50, 12345) & on_plane)[:40]
    x[free[:20]], x[free[20:]] = np.inf, -np.inf
    return _case("inf-x", x, y, z, PERTURBED_TF, planted=free)


def degenerate_cases():
    i = np.arange(500, dtype=F32)
    out = [_case("collinear", i, 2 * i, 3 * i, IDENT_TF, fails=True),
           _case("identical", np.full(300, 2.5), np.full(300, -1.25), np.full(300, 7.0), IDENT_TF, fails=True),
           _case("collinear-3", i[:3], 2 * i[:3], 3 * i[:3], IDENT_TF, fails=True),
           _case("two-points", [1.0, 2.0], [0.0, 5.0], [3.0, 4.0], IDENT_TF, fails=True),
           _case("all-nan", *(np.full(1000, np.nan),) * 3, IDENT_TF, fails=True),
           nonfinite_case(), inf_x_case()]
    return out


def handle_sequence():
    """(case, iterations) steps for ONE handle: failing, good, failing, the good cloud with 4096 and with 7 iterations"""
    x, y, z = _good_cloud()
    good = {it: _case(f"good-{it}", x, y, z, IDENT_TF, 0.04, it, 12345) for it in (50, 4096, 7)}
    d = {c.tag: c for c in degenerate_cases()}
    return [d["collinear"], good[50], d["all-nan"], good[4096], good[7], d["identical"], good[50]]


# ---------------------------------------------------------------------------------------------- E: sum order --

SUM_SIZES = (64, 65, 4096, 4097, 262_144, 262_145, 300_000)
SUM_DISTANCES = (("1km", 1000.0), ("10km", 10000.0))
# (distance, n) -> the generator seed, where 505 + n had to be replaced: the first seed (tried in the order 505 + n,
# 1000 k + n) whose refined plane differs in float32 bytes under BOTH other sum orders with the 2^-40 margin kept
SUM_RNG = {("1km", 65): 25065, ("1km", 4096): 31096, ("1km", 4097): 18097, ("1km", 262_144): 279_144,
           ("1km", 262_145): 270_145, ("1km", 300_000): 329_000, ("10km", 4096): 4601, ("10km", 4097): 4602,
           ("10km", 262_144): 262_649, ("10km", 262_145): 265_145}
# No seed was found that makes these sensitive (3000 generator seeds tried for each): with 43 or 44 inliers, float32 values
# of one binade, the squares' sums are exact in fp64 and the cross terms differ by an fp64 ulp or two, which the
# cancellation does not lift to a float32 bit.  The host test asserts that they are NOT sensitive, so that nobody counts on them.
SUM_INSENSITIVE = ("sum-1km-64", "sum-10km-64", "sum-10km-65")


def far_patch(rng, n, dist, outliers):
    """a 2 m patch `dist` metres down the lidar's x axis: z = -1.5 + 0.01 (x - dist) with 1 cm noise; the first
    `outliers` points lie off it.  ONE generator call per coordinate."""
    x = dist + rng.uniform(0.0, 2.0, n)
    y = rng.uniform(-1.0, 1.0, n)
    w = rng.uniform(-1.0, 1.0, n)
    z = -1.5 + 0.01 * (x - dist) + 0.01 * np.sqrt(3.0) * w   # uniform noise of 1 cm rms
    z[:outliers] = 1.0 + 2.0 * w[:outliers]
    return x.astype(F32), y.astype(F32), z.astype(F32)


def sum_case(name, dist, n):
    rng = np.random.default_rng(SUM_RNG.get((name, n), 505 + n))
    x, y, z = far_patch(rng, n, dist, n // 3)
    return _case(f"sum-{name}-{n}", x, y, z, PERTURBED_TF)


def sum_cases():
    return [sum_case(name, d, n) for name, d in SUM_DISTANCES for n in SUM_SIZES]


# --------------------------------------------------------------------------------------- G: butterfly steps --
# Two steps of the butterfly taken in another order (ransac_ref's "rows-swapped" and "dpp-reversed") move a sum by an fp64
# ulp or two.  The E patches do not lift that to a float32 bit; a patch 65 km out does.  "dpp-reversed" touches the sum of
# 64 consecutive points only: while all coordinates share a binade that sum rounds once, in its last add, whatever the
# order -- so the second patch straddles 2^16 in the far camera coordinate (camera z from 65535.1 to 65537.4).
# (tag, distance, n, generator seed, the orders whose refined float32 bytes differ from the tree's)
STEPS = (("steps-65535m-4097", 65535.0, 4097, 1, ("rows-swapped",)),
         ("steps-65535m-300000", 65535.0, 300_000, 1, ("rows-swapped",)),
         ("steps-straddle-4097", 65715.5, 4097, 7, ("rows-swapped", "dpp-reversed")),
         ("steps-straddle-4097b", 65715.5, 4097, 6, ("dpp-reversed",)))


def step_cases():
    out = []
    for tag, dist, n, rng_seed, orders in STEPS:
        x, y, z = far_patch(np.random.default_rng(rng_seed), n, dist, n // 3)
        out.append(_case(tag, x, y, z, PERTURBED_TF, orders=orders))
    return out


# ------------------------------------------------------------------------------------------- F: general tree --

GENERAL_N = 4096 * 4096 + 4097
GENERAL = dict(iters=4, seed=7)
GENERAL_DIST = 10000.0   # at 1 km the exactly rounded sums give the tree's float32 bytes for every seed tried (1 .. 13)


def general_case():
    rng = np.random.default_rng(606)
    x, y, z = far_patch(rng, GENERAL_N, GENERAL_DIST, GENERAL_N // 3)
    return _case("general-tree", x, y, z, PERTURBED_TF, 0.04, GENERAL["iters"], GENERAL["seed"])


def boxes():
    """a few boxes over the image for the pose path: its quarters and one box in the middle (first match wins)"""
    from pose_ref import make_boxes
    return make_boxes([(300.0, 220.0, 340.0, 260.0), (0.0, 0.0, 320.0, 240.0), (320.0, 0.0, 640.0, 240.0),
                       (0.0, 240.0, 320.0, 480.0), (320.0, 240.0, 640.0, 480.0)])
