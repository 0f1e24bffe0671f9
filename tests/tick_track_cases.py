"""[EXTENSION] X15 inputs and plain references for the tick's detection list (test_tick_track_host.py,
test_gpu_tick_track.py): validity patterns, the list as a literal loop, transforms that reach every branch of the
basis -> quaternion step, and small scenes for the tick (a 640 x 480 camera, a few thousand points)."""
import numpy as np

from gvamd import synth

LIST = 128
COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 300)
PATTERNS = ("all", "none", "alternating", "last_only", "first_128_invalid", "exactly_128_spread", "empty")
Q = ("qx", "qy", "qz", "qw")
NOT_Q = ("px", "py", "pz", "length", "width", "height")


def validity(pattern, n):
    """the valid flags of n candidates; `empty` is all valid with the empty-cloud outcome on top"""
    v = np.zeros(n, np.uint8)
    if pattern in ("all", "empty"):
        v[:] = 1
    elif pattern == "alternating":
        v[::2] = 1
    elif pattern == "last_only":
        v[-1:] = 1
    elif pattern == "first_128_invalid":
        v[128:] = 1
    elif pattern == "exactly_128_spread":   # (up to) 128 valid ones with invalid ones between them, the last candidate valid
        idx = np.unique(np.round(np.linspace(0, n - 1, min(n, 128))).astype(int)) if n else np.zeros(0, int)
        v[idx] = 1
    elif pattern != "none":
        raise ValueError(pattern)
    return v


def reference_list(base_poses, valid, empty):
    """(records, n, n_total) by a plain loop over candidates already in the base frame"""
    out = np.zeros(LIST, synth.LSHAPE_DTYPE)
    m = 0
    for c in range(len(valid)):
        if empty or not valid[c]:
            continue
        if m < LIST:
            out[m] = base_poses[c]
        m += 1
    return out, min(m, LIST), m


def cam_poses(n, seed, unit_q=True):
    rng = np.random.default_rng(seed)
    p = np.zeros(n, synth.LSHAPE_DTYPE)
    for k, s in (("px", 20.0), ("py", 3.0), ("pz", 40.0)):
        p[k] = rng.normal(0.0, s, n)
    q = rng.normal(0.0, 1.0, (n, 4))
    if unit_q:
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    for i, k in enumerate(Q):
        p[k] = q[:, i]
    p["length"], p["width"], p["height"] = rng.uniform(0.2, 6.0, n), rng.uniform(0.2, 3.0, n), rng.uniform(0.0, 2.5, n)
    return p


def pitch_poses(n, seed):
    """camera-frame poses as the two pose branches make them: the quaternion of setRPY(0, pitch, 0)"""
    rng = np.random.default_rng(seed)
    p = cam_poses(n, seed)
    a = rng.uniform(-np.pi, np.pi, n)
    p["qx"], p["qz"] = 0.0, 0.0
    p["qy"], p["qw"] = np.sin(0.5 * a), np.cos(0.5 * a)
    return p


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def quat_branch(tf, pose):
    """which branch of Matrix3x3::getRotation the product basis takes: 'trace', or 0, 1, 2 for the largest diagonal entry
    (None next to a branch edge, where this float evaluation is no witness)"""
    q = np.array([pose[k] for k in Q], np.float64)
    if not np.isfinite(q).all() or not q.any():
        return None
    m = _rot(np.asarray(tf[:4], np.float64) / np.linalg.norm(tf[:4])) @ _rot(q / np.linalg.norm(q))
    tr, d = np.trace(m), np.diag(m)
    if abs(tr) < 1e-6:
        return None
    if tr > 0:
        return "trace"
    o = np.sort(d)
    return int(np.argmax(d)) if o[2] - o[1] > 1e-6 else None


def branch_transforms():
    """base <- camera transforms: the project's two, and half turns (slightly off) about x, y and z, which with poses near
    the identity leave the trace negative and the largest diagonal entry at 0, 1 and 2"""
    out = [tuple(synth.transforms(p)["base_cam"]) for p in (False, True)]
    for axis in range(3):
        q = np.array([0.03, -0.02, 0.025, 0.04])
        q[axis] = 1.0
        q /= np.linalg.norm(q)
        out.append(tuple(q) + (1.5 - axis, 0.25 * axis, 1.1))
    return out


# ------------------------------------------------------------------------------------------------ tick scenes --
CELL = 16          # pixels: box c of a scene sits in cell (c % 40, c // 40) of the image's upper 208 rows
COLS = synth.IMG_W // CELL
MAX_BOXES = COLS * 13
STATIC_LABEL, DYNAMIC_LABELS = 5, (9, 0, 1, 2)


def _cam_to_lidar(tf_cl, pc):
    """lidar points (float32) of camera-frame points under camera <- lidar tf_cl"""
    r = _rot(np.asarray(tf_cl[:4], np.float64))
    return ((pc - np.asarray(tf_cl[4:], np.float64)) @ r).astype(np.float32)   # R^T (p - t), row vectors


def grid_boxes(n, static_every=4):
    """n boxes, one per 16 x 16 pixel cell (2 pixels of margin), every static_every-th of a static class"""
    assert n <= MAX_BOXES
    b = np.zeros(n, synth.BBOX_DTYPE)
    c = np.arange(n)
    b["x_min"], b["y_min"] = CELL * (c % COLS) + 2, CELL * (c // COLS) + 2
    b["x_max"], b["y_max"] = b["x_min"] + CELL - 4, b["y_min"] + CELL - 4
    b["confidence"] = np.linspace(0.95, 0.6, n, dtype=np.float32) if n else 0.0
    b["label"] = [STATIC_LABEL if static_every and i % static_every == static_every - 1 else DYNAMIC_LABELS[i % 4] for i in range(n)]
    return b


def ground(tf_cl, n, seed, z=-1.3):
    """an exact plane of n lidar points, z up: all of it is ground to the 0.04 m test"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(2.0, 30.0, n).astype(np.float32), rng.uniform(-10.0, 10.0, n).astype(np.float32), np.full(n, z, np.float32))


def clusters(tf_cl, boxes, points_per, seed, depths=None):
    """points_per[i] lidar points behind the centre of box i (at depths[i], 7 .. 10 m when None), within 0.06 m of the
    ray through it and 0.15 m along the view: under 3 pixels from the centre (14 pass RadiusOutlierRemoval(0.4, 10); 5 do not)"""
    rng = np.random.default_rng(seed)
    pts = []
    for i, b in enumerate(boxes):
        k = int(points_per[i])
        zc = rng.uniform(7.0, 10.0) if depths is None else float(depths[i])
        if k == 0:
            continue
        u, v = 0.5 * (b["x_min"] + b["x_max"]), 0.5 * (b["y_min"] + b["y_max"])
        pc = np.empty((k, 3))
        pc[:, 2] = zc + rng.uniform(-0.15, 0.15, k)
        pc[:, 0] = (u - synth.CX) / synth.FX * pc[:, 2] + rng.uniform(-0.06, 0.06, k)
        pc[:, 1] = (v - synth.CY) / synth.FY * pc[:, 2] + rng.uniform(-0.06, 0.06, k)
        pts.append(pc)
    if not pts:
        return tuple(np.zeros(0, np.float32) for _ in range(3))
    p = _cam_to_lidar(tf_cl, np.concatenate(pts))
    return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()


def pca_scene(tfs, valid, seed=1, few=(), n_ground=5000):
    """(x, y, z, boxes): ground, 30 points of clutter, a cluster of 14 points in every box whose flag is set and of 5 in
    the boxes of `few`"""
    n = len(valid)
    boxes = grid_boxes(n)
    per = np.where(np.asarray(valid, bool), 14, 0)
    per[list(few)] = 5
    cx, cy, cz = clusters(tfs["cam_lidar"], boxes, per, seed)
    gx, gy, gz = ground(tfs["cam_lidar"], n_ground, seed + 100)
    rng = np.random.default_rng(seed + 200)   # behind the camera and off the plane: in no box, and the segmented cloud is never empty
    ox, oy, oz = (rng.uniform(lo, hi, 30).astype(np.float32) for lo, hi in ((-6.0, -3.0), (-2.0, 2.0), (0.0, 1.0)))
    return np.concatenate([cx, gx, ox]), np.concatenate([cy, gy, oy]), np.concatenate([cz, gz, oz]), boxes


def moving_boxes(tick, n_ticks=8, half=(7, 7), rows=(120.0, 60.0)):
    """two boxes of half[0] x half[1] pixels half size that cross in the image, in different rows, of dynamic classes"""
    s = tick / (n_ticks - 1.0)
    b = np.zeros(2, synth.BBOX_DTYPE)
    u = (200.0 + 240.0 * s, 440.0 - 240.0 * s)
    for i, v in enumerate(rows):
        b[i] = (round(u[i]) - half[0], v - half[1], round(u[i]) + half[0], v + half[1], 0.9, DYNAMIC_LABELS[i])
    return b


def moving_scene(tfs, tick):
    """(x, y, z, boxes) of the PCA branch's tick: the two boxes' clusters at 8 and 10 m and the ground"""
    boxes = moving_boxes(tick)
    cx, cy, cz = clusters(tfs["cam_lidar"], boxes, (14, 14), 300 + tick, depths=(8.0, 10.0))
    gx, gy, gz = ground(tfs["cam_lidar"], 3000, 77)
    return np.concatenate([cx, gx]), np.concatenate([cy, gy]), np.concatenate([cz, gz]), boxes


def ego_motion(tick):
    """base_prev <- base_now of the odd ticks; None on the even ones"""
    if tick % 2 == 0:
        return None
    yaw = 0.01 * tick
    return (0.0, 0.0, np.sin(0.5 * yaw), np.cos(0.5 * yaw), 0.05 * tick, -0.02, 0.0)
