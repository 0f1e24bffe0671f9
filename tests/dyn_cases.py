"""[EXTENSION] X13 fixture families of test_dyn_host.py and test_gpu_dyn.py: a case is dict(name, cfg, objs, poses, exact).

Exact families have every off_x == 0 or every yaw exactly 0 (or not finite: cos and sin of a NaN or an infinity are NaN
in every library), so no library result can differ and device, host twin and reference are compared by tobytes().
General families have random yaws with off_x = (-1, 0.5, 2); want() redraws a trajectory that has an in-range u within
dyn_ref.GUARD of an integer with the next seed and counts the redraws.

Shapes: P in {1, 63, 64, 65, 257}, K in {1, 3, 65}, 0 / 1 / 64 / 65 / 128 objects, 1 / 2 / 8 circles, spread over the
families so that the reference's Python loops stay below a million (pose, circle, object) tests in all."""
import numpy as np

import dyn_ref as ref

F32 = np.float32
MOVING_OBJECT_DTYPE = None   # gvamd's, set by _dtype()


def _dtype():
    global MOVING_OBJECT_DTYPE
    if MOVING_OBJECT_DTYPE is None:
        import gvamd
        MOVING_OBJECT_DTYPE = gvamd.MOVING_OBJECT_DTYPE
    return MOVING_OBJECT_DTYPE


def objects(rows, quat=None):
    """rows of (px, py, yaw, length, width, vx, vy); quat: (qx, qy, qz, qw) rows that replace the yaw's quaternion"""
    rows = np.asarray(rows, np.float64).reshape(-1, 7)
    o = np.zeros(len(rows), _dtype())
    o["pose"]["px"], o["pose"]["py"] = rows[:, 0], rows[:, 1]
    o["pose"]["pz"], o["pose"]["height"] = 7.0, 1.5       # ignored
    o["pose"]["qz"], o["pose"]["qw"] = np.sin(0.5 * rows[:, 2]), np.cos(0.5 * rows[:, 2])
    if quat is not None:
        quat = np.asarray(quat, np.float64).reshape(-1, 4)
        for i, n in enumerate(("qx", "qy", "qz", "qw")):
            o["pose"][n] = quat[:, i]
    o["pose"]["length"], o["pose"]["width"] = rows[:, 3], rows[:, 4]
    o["vx"], o["vy"] = rows[:, 5], rows[:, 6]
    return o


def random_objects(rng, n, speed=3.0):
    span = 8.0 if n <= 16 else 20.0       # a crowd gets a larger scene: some poses stay clear of every object
    rows = np.stack([rng.uniform(-span, span, n), rng.uniform(-span, span, n), rng.uniform(-3.2, 3.2, n), rng.uniform(0.3, 4.5, n),
                     rng.uniform(0.3, 2.0, n), rng.uniform(-speed, speed, n), rng.uniform(-speed, speed, n)], axis=1)
    return objects(rows)


def random_poses(rng, K, P, yaw=True):
    """K wandering trajectories: a start in the scene, steps of up to 0.3 m; yaw random or exactly 0"""
    start = rng.uniform(-6, 6, (K, 1, 2))
    steps = rng.uniform(-0.3, 0.3, (K, P, 2)).cumsum(axis=1)
    poses = np.zeros((K, P, 3), F32)
    poses[:, :, :2] = (start + steps).astype(F32)
    if yaw:
        poses[:, :, 2] = rng.uniform(-7.0, 7.0, (K, P)).astype(F32)
    return poses


def _ulp(v, up):
    return np.nextafter(F32(v), F32(np.inf if up else -np.inf))


BASE = ref.config(radius=0.625, influence_radius=1.5, quantum=0.125)   # inv_q2 = 64, T = 145, table[25] the last 253
FAR = (90.0, 90.0, 0.0)    # a filler pose that costs 0


def _filled(K, P, special):
    """(K, P, 3) of FAR with special[(k, p)] = (x, y, yaw)"""
    poses = np.tile(np.array(FAR, F32), (K, P, 1))
    for (k, p), v in special.items():
        poses[k, p] = v
    return poses


def exact_cases():
    out = []
    box = objects([(0.0, 0.0, 0.0, 2.0, 1.0, 0.0, 0.0)])     # hl = 1, hw = 0.5, at rest

    # d2 == radius^2 exactly (u == 25): along an edge (ex = 0.625) and at a corner (ex = 0.375, ey = 0.5), and x one
    # float32 ulp either side
    sp = {}
    for k, (x, y) in enumerate([(1.625, 0.25), (1.375, 1.0)]):
        sp[(k, 0)] = (x, y, 0.0)
        sp[(k, 1)] = (_ulp(x, False), y, 0.0)
        sp[(k, 2)] = (_ulp(x, True), y, 0.0)
    out.append(dict(name="radius_edge_corner", cfg=BASE, objs=box, poses=_filled(3, 63, sp), exact=True))

    # u an exact integer k^2 from a point object (length = width = 0): the whole table up to its last entry u = 144,
    # then u = 145 == T (12^2 + 1^2) and u = 169: both cost 0
    point = objects([(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)])
    sp = {(0, k): (0.125 * k, 0.0, 0.0) for k in range(14)}
    sp[(0, 14)] = (1.5, 0.125, 0.0)
    sp[(0, 15)] = (1.5, 0.0, 0.0)
    cfg = dict(BASE, collision_cost=255)
    out.append(dict(name="integer_u_table_end", cfg=cfg, objs=point, poses=_filled(1, 64, sp), exact=True))

    # a centre inside the rectangle: 254
    out.append(dict(name="inside", cfg=BASE, objs=box, poses=_filled(1, 1, {(0, 0): (0.5, -0.25, 0.0)}), exact=True))

    rng = np.random.default_rng(131)
    # rotated objects: non-trivial unit quaternions (a yaw, and a general rotation), and non-unit ones, used as given
    o = random_objects(rng, 65)
    quat = rng.normal(size=(65, 4))
    quat[:22] /= np.linalg.norm(quat[:22], axis=1, keepdims=True)      # unit, general
    quat[22:44] *= 0.7                                                  # not unit
    o2 = objects(np.stack([o["pose"]["px"], o["pose"]["py"], np.zeros(65), o["pose"]["length"], o["pose"]["width"], o["vx"], o["vy"]], axis=1),
                 quat)
    o2[44:] = o[44:]                                                    # plain yaws
    cfg8 = dict(BASE, off_x=(-1.0, -0.5, 0.0, 0.25, 0.5, 1.0, 1.5, 2.0), t0=0.35)
    out.append(dict(name="rotated_8_circles_yaw0", cfg=cfg8, objs=o2, poses=random_poses(rng, 1, 64, yaw=False), exact=True))
    # one object, many trajectories, random yaws that are never read (off_x == 0)
    out.append(dict(name="one_object_K65", cfg=dict(BASE, t0=-0.5), objs=random_objects(rng, 1), poses=random_poses(rng, 65, 63), exact=True))
    # 128 objects, two circles at yaw 0, negative and zero velocities, P past four chunks
    o = random_objects(rng, 128)
    o["vx"][:40] = -np.abs(o["vx"][:40]); o["vy"][:40] = -np.abs(o["vy"][:40])
    o["vx"][40:60] = 0.0; o["vy"][40:60] = 0.0
    out.append(dict(name="n128_two_circles", cfg=dict(BASE, off_x=(0.0, 1.25)), objs=o, poses=random_poses(rng, 3, 257, yaw=False), exact=True))
    # dt == 0: every pose at t0
    out.append(dict(name="dt_zero", cfg=dict(BASE, t0=2.0, dt=0.0), objs=random_objects(rng, 64), poses=random_poses(rng, 3, 65), exact=True))

    # an object that crosses the path and reaches it only at pose 37 of 65: first_collision == 37
    path = np.zeros((1, 65, 3), F32)
    path[0, :, 0] = (0.1 * np.arange(65)).astype(F32)
    crossing = objects([(3.7, -37.0, 0.0, 0.2, 0.2, 0.0, 10.0)])
    out.append(dict(name="arrives_at_37", cfg=dict(BASE, radius=0.3), objs=crossing, poses=path, exact=True))

    # two identical objects at indices 2 and 5, the others farther: nearest_object == 2
    rows = [(40.0 + 3 * j, 40.0, 0.3, 1.0, 1.0, 0.0, 0.0) for j in range(8)]
    rows[2] = rows[5] = (1.0, 2.0, 0.4, 2.0, 1.0, 0.5, -0.25)
    out.append(dict(name="identical_objects", cfg=BASE, objs=objects(rows), poses=random_poses(rng, 3, 64), exact=True))

    # no objects
    out.append(dict(name="no_objects", cfg=BASE, objs=objects(np.zeros((0, 7))), poses=random_poses(rng, 3, 65), exact=True))
    out.append(dict(name="no_objects_one_pose", cfg=BASE, objs=objects(np.zeros((0, 7))), poses=random_poses(rng, 1, 1), exact=True))

    # NaN and +-inf in each pose component, two circles (one off the centre), the finite yaws exactly 0
    K = 9
    poses = random_poses(rng, K, 3, yaw=False)
    poses[:, :, :2] *= F32(0.3)
    for i in range(3):
        for m, v in enumerate((np.nan, np.inf, -np.inf)):
            poses[3 * i + m, 1, i] = v
    out.append(dict(name="nonfinite", cfg=dict(BASE, off_x=(0.0, 0.5)), objs=random_objects(rng, 8, speed=0.5), poses=poses, exact=True))
    return out


GENERAL_OFF = (-1.0, 0.5, 2.0)
GENERAL_SHAPES = [("general_K65_P65_n1", 65, 65, 1), ("general_K3_P257_n64", 3, 257, 64), ("general_K3_P63_n128", 3, 63, 128),
                  ("general_K1_P64_n65", 1, 64, 65)]


def general_cases():
    out = []
    for i, (name, K, P, n) in enumerate(GENERAL_SHAPES):
        rng = np.random.default_rng(500 + i)
        cfg = dict(BASE, off_x=GENERAL_OFF, t0=0.2, dt=0.05)
        out.append(dict(name=name, cfg=cfg, objs=random_objects(rng, n), poses=random_poses(rng, K, P), exact=False, seed=900 + 10 * i))
    return out


_WANT = {}


def want(c):
    """dyn_ref.score of the case, once per process.  A general case comes back with its guarded trajectories redrawn
    (c["poses"] is replaced) and c["redrawn"] counting them."""
    if c["name"] not in _WANT:
        r = ref.score(c["cfg"], c["objs"], c["poses"])
        redrawn = 0
        if not c["exact"]:
            seed = c["seed"]
            K, P = c["poses"].shape[:2]
            for k in np.flatnonzero(r["guarded"]):
                while True:
                    seed += 1
                    redrawn += 1
                    c["poses"][k] = random_poses(np.random.default_rng(seed), 1, P)[0]
                    one = ref.score(c["cfg"], c["objs"], c["poses"][k:k + 1])
                    if not one["guarded"][0]:
                        break
                for key in ("scores", "pose_cost", "guarded", "obj_min"):
                    r[key][k] = one[key][0]
        c["redrawn"] = redrawn
        _WANT[c["name"]] = (r, c)
    r, first = _WANT[c["name"]]
    if first is not c:
        c["poses"], c["redrawn"] = first["poses"], first["redrawn"]
    return r


_CASES = {}


def cases(exact):
    if exact not in _CASES:
        _CASES[exact] = exact_cases() if exact else general_cases()
    return _CASES[exact]


def compare(c, r, scores, pose_cost, tag):
    """scores / pose_cost of the device or the host twin against the reference result r of case c"""
    name = (c["name"], tag)
    assert scores.dtype == ref.SCORE_DTYPE and scores.shape == r["scores"].shape, name
    if c["exact"]:
        assert scores.tobytes() == r["scores"].tobytes(), (name, scores[:4], r["scores"][:4])
        assert pose_cost.tobytes() == r["pose_cost"].tobytes(), name
        return
    w = r["scores"]
    for f in ("max_cost", "first_collision", "cost_sum"):
        assert np.array_equal(scores[f], w[f]), (name, f)
    assert np.array_equal(pose_cost, r["pose_cost"]), name
    d, e = scores["min_dist2"], w["min_dist2"]
    assert (np.abs(d - e) <= ref.DIST_TOL * (1.0 + e)).all(), (name, d, e)
    clear = np.array([ref.nearest_is_clear(row) for row in r["obj_min"]])
    assert np.array_equal(scores["nearest_object"][clear], w["nearest_object"][clear]), name
