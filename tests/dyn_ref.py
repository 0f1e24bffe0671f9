"""[EXTENSION] X13 reference: scoring poses against predicted moving objects, the definition of
include/gridvision_hip.h restated with scalar fp64 values and plain Python loops (a Python float is an IEEE double and
every operation below is one rounded operation: nothing can be contracted).  cos and sin are numpy's.  The cost table
comes from the existing inflation_cost_table wrapper, so the table is not restated here.

score() also returns what the general-yaw tests need to judge a comparison: per trajectory whether some in-range
(pose, circle, object) has u within GUARD * (1 + u) of an integer (the cost could then differ by a last bit of sin or
cos), and every object's own minimum of d2 (for the runner-up test of nearest_object).  Two kinds of pair are not
guarded because no last bit can move their table entry: u > T + 1 (the cost is 0 on either side), and u < 0.5, the
neighbourhood of the integer 0 -- u is never negative, so a centre inside or a hair outside a rectangle reads table[0]
whichever way the bit falls."""
import math

import numpy as np

SCORE_DTYPE = np.dtype([("max_cost", np.int32), ("first_collision", np.int32), ("cost_sum", np.uint32),
                        ("nearest_object", np.int32), ("min_dist2", np.float64)])
assert SCORE_DTYPE.itemsize == 24
GUARD = 1e-9
DIST_TOL = 1e-12      # on min_dist2, times (1 + d2): 100 times what a last-bit difference of sin or cos can do
MAX_OBJECTS, MAX_CIRCLES = 128, 8


def config(off_x=(0.0,), radius=0.5, influence_radius=1.5, cost_scaling_factor=1.0, quantum=0.125, t0=0.0, dt=0.1,
           collision_cost=253, w_sum=1, w_max=0, flags=0):
    return dict(off_x=tuple(float(v) for v in off_x), radius=float(radius), influence_radius=float(influence_radius),
                cost_scaling_factor=float(cost_scaling_factor), quantum=float(quantum), t0=float(t0), dt=float(dt),
                collision_cost=int(collision_cost), w_sum=int(w_sum), w_max=int(w_max), flags=int(flags))


def to_struct(gvamd, cfg):
    c = gvamd.DynConfig()
    c.n_circles = len(cfg["off_x"])
    for i, v in enumerate(cfg["off_x"][:8]):
        c.off_x[i] = v
    for n in ("radius", "influence_radius", "cost_scaling_factor", "quantum", "t0", "dt", "collision_cost", "w_sum", "w_max", "flags"):
        setattr(c, n, cfg[n])
    return c


_TABLES = {}


def table(cfg):
    """the cost table of the configuration: gv_inflation_cost_table's, as the definition says"""
    import gvamd
    key = (cfg["radius"], cfg["influence_radius"], cfg["cost_scaling_factor"], cfg["quantum"])
    if key not in _TABLES:
        _TABLES[key] = gvamd.inflation_cost_table(gvamd.Inflation(key[0], key[1], key[2], 100, 0), key[3])
    return _TABLES[key]


def object_rows(objs):
    """(x, y, vx, vy, c, s, hl, hw) per object, Python floats"""
    rows = []
    for o in objs:
        q = o["pose"]
        qx, qy, qz, qw = float(q["qx"]), float(q["qy"]), float(q["qz"]), float(q["qw"])
        c = 1.0 - 2.0 * (qy * qy + qz * qz)
        s = 2.0 * (qw * qz + qx * qy)
        rows.append((float(q["px"]), float(q["py"]), float(o["vx"]), float(o["vy"]), c, s, 0.5 * float(q["length"]),
                     0.5 * float(q["width"])))
    return rows


def score(cfg, objs, poses):
    """dict(scores (K,), pose_cost (K, P) uint8, guarded (K,) bool, obj_min (K, n) float64)"""
    poses = np.asarray(poses, np.float32)
    K, P = poses.shape[:2]
    tab = table(cfg)
    T = len(tab)
    tab = [int(v) for v in tab]
    rows = object_rows(objs)
    n = len(rows)
    off = cfg["off_x"]
    need_yaw = any(v != 0.0 for v in off)
    q = cfg["quantum"]
    inv_q2 = 1.0 / (q * q)
    t0, dt, coll = cfg["t0"], cfg["dt"], cfg["collision_cost"]
    inf = math.inf
    scores = np.zeros(K, SCORE_DTYPE)
    pose_cost = np.zeros((K, P), np.uint8)
    guarded = np.zeros(K, bool)
    obj_min = np.full((K, n), inf)
    with np.errstate(invalid="ignore"):
        cs, sn = np.cos(poses[:, :, 2].astype(np.float64)), np.sin(poses[:, :, 2].astype(np.float64))
    for k in range(K):
        mx, first, total = 0, -1, 0
        om = [inf] * n
        guard = False
        for p in range(P):
            t = t0 + float(p) * dt
            x, y = float(poses[k, p, 0]), float(poses[k, p, 1])
            centres = []
            for o in off:
                if o == 0.0:
                    centres.append((x, y))
                else:
                    centres.append((x + float(cs[k, p]) * o, y + float(sn[k, p]) * o))
            m2 = inf
            for j in range(n):
                xj, yj, vxj, vyj, c, s, hl, hw = rows[j]
                ox = xj + vxj * t
                oy = yj + vyj * t
                for ax, ay in centres:
                    dx = ax - ox
                    dy = ay - oy
                    lx = c * dx + s * dy
                    ly = c * dy - s * dx
                    ex = math.fabs(lx) - hl
                    ex = ex if ex > 0.0 else 0.0
                    ey = math.fabs(ly) - hw
                    ey = ey if ey > 0.0 else 0.0
                    d2 = ex * ex + ey * ey
                    if d2 < om[j]:
                        om[j] = d2
                    if d2 < m2:
                        m2 = d2
                    u = d2 * inv_q2
                    if 0.5 < u <= T + 1 and abs(u - round(u)) <= GUARD * (1.0 + u):
                        guard = True
            u = m2 * inv_q2
            cost = tab[int(u)] if u < float(T) else 0
            pose_cost[k, p] = cost
            mx = max(mx, cost)
            total += cost
            if cost >= coll and first < 0:
                first = p
        md = min(om) if n else inf
        nearest = om.index(md) if n else -1
        scores[k] = (mx, first, total & 0xFFFFFFFF, nearest, md)
        guarded[k] = guard
        obj_min[k] = om
    return dict(scores=scores, pose_cost=pose_cost, guarded=guarded, obj_min=obj_min)


def nearest_is_clear(obj_min_row):
    """the runner-up object is farther than the nearest by more than the margin a last bit of sin or cos allows"""
    v = np.sort(obj_min_row)
    return len(v) < 2 or not (v[1] - v[0] <= DIST_TOL * (1.0 + v[1]))


# ---- the control step's combine and select with the third record (rollout_ref.select restated with it)
U64 = 0xFFFFFFFFFFFFFFFF
RESULT_DTYPE = np.dtype([("best", np.int32), ("n_valid", np.int32), ("best_total", np.uint64)])


def select(w, traj, nav, dyn, cfg):
    """(result (1,), totals (K,) uint64); nav None without a nav weight; dyn / cfg None: the two records alone"""
    nav_used = bool(w["w_nav_last"] or w["w_nav_sum"] or w["w_nav_best"])
    K = len(traj)
    totals = np.full(K, U64, np.uint64)
    best, best_total, nvalid = -1, U64, 0
    for k in range(K):
        if int(traj[k]["first_collision"]) >= 0:
            continue
        v = w["w_cost_sum"] * int(traj[k]["cost_sum"]) + w["w_max_cost"] * (int(traj[k]["max_cost"]) & 0xFFFFFFFF)
        if nav_used:
            if int(nav[k]["n_bad"]) > 0:
                continue
            v += w["w_nav_last"] * int(nav[k]["last"]) + w["w_nav_sum"] * int(nav[k]["sum"]) + w["w_nav_best"] * int(nav[k]["best"])
        if cfg is not None:
            if int(dyn[k]["first_collision"]) >= 0:
                continue
            v += cfg["w_sum"] * int(dyn[k]["cost_sum"]) + cfg["w_max"] * (int(dyn[k]["max_cost"]) & 0xFFFFFFFF)
        totals[k] = v
        nvalid += 1
        if best < 0 or v < best_total:
            best, best_total = k, v
    res = np.zeros(1, RESULT_DTYPE)
    res[0] = (best, nvalid, best_total if best >= 0 else U64)
    return res, totals
