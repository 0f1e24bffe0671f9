"""Cameras, scenes and box sets of tests/test_gpu_camera.py: the projection, the box test, the kNN depth and the per-box
cloud path at cameras other than gvamd.synth's 640 x 480, fx = fy = cx = 320.  tests/test_camera_host.py asserts, from
the oracle alone, that every scene and box set reaches what it was built for, and that the cases below take the table
paths they are listed for.  No expected value lives here: every expectation is the oracle's on the float32 points.

A scene is made by aiming at pixel targets (u, v, depth) and inverting the camera and synth.transforms(perturbed) in
fp64; the inversion is inexact after rounding to float32, which is why nothing is read off the targets.

The box test keeps one 64-bit mask word per 16 x 16-pixel tile and 64 boxes; the two table sizes that decide which
kernel runs are frame_table_bytes() (fused into k_bin_partition while <= kBinBBoxLdsMax, gv_binning.hip) and
classify_table_bytes() (k_pose_classify<true> while <= 48 KB, gv_cloudops.hip).

TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import oracle_lib as ol
import pose_ref as P
from gvamd import synth
from gvamd.synth import BBOX_DTYPE

F32 = np.float32
NEAR = 2.5e-4                                  # "a few float ulps" at the scale of an image bound (ulp(1920) = 1.2e-4)
DEPTHS = (0.0011, 0.5, 2.5, 7.0, 60.0)
NEAR_DEPTHS = (0.5, 2.5, 7.0)
CHUNK = 2048                                   # points per partition workgroup
SCENE_SIZES = {False: 10 * CHUNK + 2048 + 512 + 37, True: 12 * CHUNK}   # ends inside a chunk / on a chunk boundary
SMALL_SIZES = (2048 + 512 + 37, 4096)          # prefixes of a (shuffled) scene: the pipeline's two clouds
BOX_SIZES = (1, 64, 65, 128, 129, 257)         # 257: the first count with five mask words

Camera = namedtuple("Camera", "name w h fx fy cx cy")


def _camera(name, w, h, fx, fy, cx, cy):
    """gv_cam_params holds floats: every intrinsic is rounded to float32 once, for gv_create and for the oracle alike"""
    return Camera(name, w, h, *(float(F32(t)) for t in (fx, fy, cx, cy)))


CAMERAS = {c.name: c for c in (
    _camera("synth", 640, 480, 320.0, 320.0, 320.0, 240.0),            # control: today's camera through the same code
    _camera("kitti", 1242, 375, 721.5377, 721.5377, 609.5593, 172.854),   # W % 16 = 10, H % 16 = 7, 78 x 24 tiles
    _camera("hd720", 1280, 720, 910.25, 905.5, 651.3, 349.7),          # 3600 tiles: a frame is never fused
    _camera("hd1080", 1920, 1080, 1400.6, 1398.2, 967.4, 531.9),       # 8160 tiles: classify never in LDS; H % 16 = 8
    _camera("tiny", 17, 9, 11.3, 7.9, 8.2, 4.6),                       # 2 x 1 tiles, both ragged
    _camera("pixel", 1, 1, 0.75, 0.75, 0.5, 0.5),                      # one tile, u, v in [0, 1)
    _camera("offaxis", 640, 480, 500.5, 250.25, -50.5, 600.25),        # principal point outside the image, fx = 2 fy
)}
LARGE_SET_CAMERAS = ("synth", "kitti", "hd720")


def box_sizes(cam):
    return BOX_SIZES if cam.name in LARGE_SET_CAMERAS else BOX_SIZES[:4]


def K_of(cam):
    return ol.set_intrinsic(cam.fx, cam.fy, cam.cx, cam.cy)


def create_args(cam):
    """keyword arguments of gvamd.GridVisionHIP for this camera"""
    return dict(fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, image_w=cam.w, image_h=cam.h)


def tiles(cam):
    return (cam.w + 15) // 16, (cam.h + 15) // 16


def mask_words(nb):
    return max(1, (nb + 63) // 64)


def frame_table_bytes(cam, nb):
    """bin_bbox_lds (gv_binning.hip): what the fused box test stages in k_bin_partition's LDS"""
    tx, ty = tiles(cam)
    return 16 + 16 * ((nb + 3) & ~3) + 8 * tx * ty * mask_words(nb)


def classify_table_bytes(cam, nb):
    """launch_pose_cells (gv_cloudops.hip): thresholds and tile masks of k_pose_classify<true>"""
    tx, ty = tiles(cam)
    return 16 * ((nb + 3) & ~3) + 8 * tx * ty * mask_words(nb)


# --------------------------------------------------------------------------------------------- the oracle's view --

class Geo:
    """the oracle's view of a cloud at a camera: camera coordinates, the float projection, what is in the image"""

    def __init__(self, cam, tfs, x, y, z):
        self.cam = cam
        self.m_base, self.m_cam = ol.tf_to_matrix4f(tfs["base_lidar"]), ol.tf_to_matrix4f(tfs["cam_lidar"])
        self.cx, self.cy, self.cz = ol.transform_cloud(self.m_cam, x, y, z)
        with np.errstate(all="ignore"):
            X, Y, Z = (a.astype(np.float64) for a in (self.cx, self.cy, self.cz))
            # (float)(K row . p / z), src/cloud_detections.cpp:268-273 (test_camera_host holds this to gvo_project_points)
            self.u = ((cam.fx * X + cam.cx * Z) / Z).astype(F32)
            self.v = ((cam.fy * Y + cam.cy * Z) / Z).astype(F32)
            self.front = np.isfinite(self.cx) & np.isfinite(self.cy) & np.isfinite(self.cz) & ~(self.cz <= F32(0.001))
            self.inimg = self.front & ~((self.u < 0) | (self.u >= cam.w) | (self.v < 0) | (self.v >= cam.h))

    def ids(self, boxes):
        return ol.extract_cloud_per_bbox(K_of(self.cam), self.cx, self.cy, self.cz, boxes, self.cam.w, self.cam.h)


def lidar_of(cam, tfs, u, v, d):
    """lidar-frame float32 points that project near (u, v) at camera depth d: camera and cam_lidar inverted in fp64"""
    u, v, d = (np.asarray(a, np.float64) for a in (u, v, d))
    tf = tfs["cam_lidar"]
    r, t = synth._quat_to_matrix(tf[:4]), np.asarray(tf[4:7], np.float64)
    pc = np.stack([(u - cam.cx) * d / cam.fx, (v - cam.cy) * d / cam.fy, d], axis=1)
    pl = (pc - t[None, :]) @ r               # r^T (pc - t)
    return pl[:, 0].astype(F32), pl[:, 1].astype(F32), pl[:, 2].astype(F32)


def near_bounds(cam):
    """[(axis, bound)]: the image borders, the start of the ragged last tile and a handful of interior multiples of 16"""
    out = []
    for axis, ext in ((0, cam.w), (1, cam.h)):
        nt = (ext + 15) // 16
        inner = {16, 16 * (nt // 2), 16 * (nt - 1), 16 * (ext // 16)}
        out += [(axis, 0.0), (axis, float(ext))] + [(axis, float(m)) for m in sorted(inner) if 0 < m < ext]
    return out


def _near(cam, tfs, rng, n, axis, bound, above):
    """n points whose oracle projection lies within NEAR of u = bound (axis 0) or v = bound (axis 1) on the asked side,
    the other coordinate well inside the image: candidates aimed within NEAR of the bound, kept by what they project to"""
    out = [np.zeros(0, F32)] * 3
    ext = (cam.w, cam.h)
    for _ in range(200):
        m = 64 * n
        p = bound + rng.uniform(-NEAR, NEAR, m)
        other = rng.uniform(0.25, 0.75, m) * ext[1 - axis]
        d = rng.choice(NEAR_DEPTHS, m)
        x, y, z = lidar_of(cam, tfs, p if axis == 0 else other, other if axis == 0 else p, d)
        g = Geo(cam, tfs, x, y, z)
        q, o = ((g.u, g.v) if axis == 0 else (g.v, g.u))
        keep = g.front & (np.abs(q.astype(np.float64) - bound) <= NEAR) & ((q >= bound) == above) & (o >= 0) & (o < ext[1 - axis])
        out = [np.concatenate([a, b[keep]]) for a, b in zip(out, (x, y, z))]
        if len(out[0]) >= n:
            return tuple(a[:n] for a in out)
    raise AssertionError(("no points near", cam.name, axis, bound, above))


Scene = namedtuple("Scene", "cam perturbed tfs x y z")
SPECIALS = [(a, val) for a in range(3) for val in (np.nan, np.inf, -np.inf)]


@functools.lru_cache(maxsize=None)
def scene(cam_name, perturbed):
    """the cloud of one camera and transform set, shuffled (any prefix is a mixture too)"""
    cam, tfs, n = CAMERAS[cam_name], synth.transforms(perturbed), SCENE_SIZES[perturbed]
    rng = np.random.default_rng([sorted(CAMERAS).index(cam_name), int(perturbed), 20261])
    parts = []
    for axis, bound in near_bounds(cam):
        for above in (False, True):
            parts.append(_near(cam, tfs, rng, 16, axis, bound, above))

    def aimed(m, d, lo=-0.1, hi=1.1):
        return lidar_of(cam, tfs, rng.uniform(lo, hi, m) * cam.w, rng.uniform(lo, hi, m) * cam.h, d)

    parts.append(aimed(400, rng.uniform(0.0009, 0.0011, 400), 0.2, 0.8))        # cz on both sides of 0.001
    parts.append(aimed(n // 16, -rng.uniform(0.2, 30.0, n // 16)))               # behind the camera
    for axis, val in SPECIALS:                                                   # NaN and +-inf coordinates
        p = list(aimed(8, rng.choice(DEPTHS[1:], 8)))
        p[axis] = np.full(8, val, F32)
        parts.append(tuple(p))
    rest = n - sum(len(p[0]) for p in parts)
    assert rest > n // 2
    parts.append(aimed(rest, rng.choice(DEPTHS, rest)))
    x, y, z = (np.concatenate([p[i] for p in parts]) for i in range(3))
    perm = rng.permutation(n)
    return Scene(cam, perturbed, tfs, x[perm], y[perm], z[perm])


@functools.lru_cache(maxsize=None)
def geo(cam_name, perturbed):
    s = scene(cam_name, perturbed)
    return Geo(s.cam, s.tfs, s.x, s.y, s.z)


def prefix(s, n):
    return Scene(s.cam, s.perturbed, s.tfs, s.x[:n], s.y[:n], s.z[:n])


# ------------------------------------------------------------------------------------------------------ box sets --

BoxSet = namedtuple("BoxSet", "boxes roles exact")
# the fixed places of a set of 64 boxes or more; the exact-bound boxes come first so that no earlier box takes their
# points, the box over the whole image comes LAST so that first match leaves every other box its points and the last
# mask word of every set still gets matches
N_EXACT = 40
ROLES = ("ragged_col", "ragged_row", "strip_col", "strip_row", "out_left", "out_right", "out_top", "out_bottom",
         "pixel_col", "nan", "empty", "overlap_a", "overlap_b")
NO_MATCH_ROLES = ("strip_col", "strip_row", "out_left", "out_right", "out_top", "out_bottom", "nan", "empty")
EDGES = ("x_min", "x_max", "y_min", "y_max")


@functools.lru_cache(maxsize=None)
def box_set(cam_name, perturbed, nb):
    """nb boxes with fractional fp64 bounds for scene(cam_name, perturbed).  One box: the whole image and beyond.  64 or
    more: see ROLES; `exact` lists (box, point, edge) of the boxes one of whose bounds is the oracle's float u or v of
    that cloud point."""
    cam, g = CAMERAS[cam_name], geo(cam_name, perturbed)
    W, H = float(cam.w), float(cam.h)
    tx, ty = tiles(cam)
    rng = np.random.default_rng([sorted(CAMERAS).index(cam_name), int(perturbed), nb, 7])
    b = np.zeros(nb, BBOX_DTYPE)
    b["confidence"] = np.linspace(0.99, 0.5, nb)
    b["label"] = 9
    whole = (-30.0, -30.0, 2 * W, 2 * H)
    if nb == 1:
        b[0] = whole + (0.99, 9)
        return BoxSet(b, {"whole": 0}, [])
    assert nb >= N_EXACT + len(ROLES) + 2
    rows, exact = [], []
    inside = np.flatnonzero(g.inimg)
    pick = rng.choice(inside, N_EXACT, replace=False)
    for k, p in enumerate(pick):
        u, v = float(g.u[p]), float(g.v[p])
        e = EDGES[k // (N_EXACT // 4)]
        bw, bh = rng.uniform(0.02, 0.06) * W, rng.uniform(0.02, 0.06) * H
        fu, fv = rng.uniform(0.2, 0.8), rng.uniform(0.2, 0.8)
        x0, y0 = u - fu * bw, v - fv * bh
        r = {"x_min": (u, y0, u + bw, y0 + bh), "x_max": (u - bw, y0, u, y0 + bh),
             "y_min": (x0, v, x0 + bw, v + bh), "y_max": (x0, v - bh, x0 + bw, v)}[e]
        rows.append(r)
        exact.append((k, int(p), e))
    named = {
        # from 3.5 px before the last tile column (row) to beyond the image
        "ragged_col": (16.0 * (tx - 1) - 3.5, 0.35 * H, W + 40.25, 0.65 * H),
        "ragged_row": (0.35 * W, 16.0 * (ty - 1) - 3.5, 0.65 * W, H + 40.25),
        # wholly inside the padding between the image and the end of its last tile: no point may ever get it
        "strip_col": (W + 0.5, -5.0, 16.0 * tx + 5.0, H + 5.0),
        "strip_row": (-5.0, H + 0.5, W + 5.0, 16.0 * ty + 5.0),
        "out_left": (-90.5, 0.1 * H, -0.25, 0.9 * H), "out_right": (16.0 * tx + 7.5, 0.1 * H, 16.0 * tx + 99.0, 0.9 * H),
        "out_top": (0.1 * W, -77.75, 0.9 * W, -0.125), "out_bottom": (0.1 * W, 16.0 * ty + 6.5, 0.9 * W, 16.0 * ty + 80.0),
        "pixel_col": (W - 1.0, 0.55 * H, W, H + 3.5),
        "nan": (0.2 * W, 0.2 * H, np.nan, 0.8 * H),
        "empty": (0.6 * W, 0.2 * H, 0.6 * W - 1.0, 0.8 * H),
        "overlap_a": (0.3031 * W, 0.3017 * H, 0.5073 * W, 0.5529 * H),
        "overlap_b": (0.4067 * W, 0.3541 * H, 0.6013 * W, 0.6097 * H),
    }
    roles = {}
    for name in ROLES:
        roles[name] = len(rows)
        rows.append(named[name])
    side = np.sqrt(0.6 / max(nb, 64))          # the random boxes together cover about half the image, whatever nb
    while len(rows) < nb - 1:
        cu, cv = rng.uniform(-0.05, 1.05) * W, rng.uniform(-0.05, 1.05) * H
        hw, hh = 0.5 * rng.uniform(0.5, 1.5) * side * W, 0.5 * rng.uniform(0.5, 1.5) * side * H
        rows.append((cu - hw, cv - hh, cu + hw, cv + hh))
    roles["whole"] = len(rows)
    rows.append(whole)
    for i, r in enumerate(rows):
        b[i]["x_min"], b[i]["y_min"], b[i]["x_max"], b[i]["y_max"] = r
    return BoxSet(b, roles, exact)


def inside(g, bb):
    """the points whose pixel box bb contains, by the reference's comparison (cloud_detections.cpp:280-288)"""
    u, v = g.u.astype(np.float64), g.v.astype(np.float64)
    with np.errstate(all="ignore"):
        return g.inimg & (u >= bb["x_min"]) & (u <= bb["x_max"]) & (v >= bb["y_min"]) & (v <= bb["y_max"])


def containing(g, boxes):
    """(first, last) index of the boxes that contain each point's pixel, -1: none"""
    n = len(g.u)
    first, last = np.full(n, -1), np.full(n, -1)
    for i, bb in enumerate(boxes):
        m = inside(g, bb)
        first[m & (first < 0)] = i
        last[m] = i
    return first, last


def grid_poses(grid):
    """three rectangles in the base frame of GridVisionHIP(*grid); the last one crosses the border and is skipped"""
    gx, gy, res = grid
    px = float(gx // 3)
    p = np.zeros(3, dtype=synth.LSHAPE_DTYPE)
    p["px"], p["py"], p["qw"] = [px - 0.1 * gx, px + 0.2 * gx, px + 0.5 * gx - 0.4], [0.1 * gy, -0.2 * gy, 0.3 * gy], 1.0
    p["length"], p["width"], p["height"] = [0.08 * gx, 0.04 * gx, 3.0], [0.1 * gy, 0.05 * gy, 0.2 * gy], 1.5
    return p


# ------------------------------------------------------------------------------------- the per-box cloud scenes --

def ray_point(cam, u, v, zc):
    return (u - cam.cx) / cam.fx * zc, (v - cam.cy) / cam.fy * zc, zc


def pose_boxes(cam, nb):
    """nb boxes of a grid that tiles the image, row major from the LAST box back: the boxes of the ragged tile row and
    column come first and are in every set"""
    cols = int(np.ceil(np.sqrt(nb * cam.w / cam.h))) if nb > 1 else 1
    cols = max(1, min(cols, nb))
    rows = (nb + cols - 1) // cols
    w, h = cam.w / cols, cam.h / rows
    r = [(c * w, q * h, (c + 1) * w, (q + 1) * h) for q in range(rows) for c in range(cols)][::-1]
    return P.make_boxes(r[:nb]), cols, rows


@functools.lru_cache(maxsize=None)
def pose_scene(cam_name, nb):
    """clusters of 12 to 40 mutually close points inside the boxes of pose_boxes (every seventh box stays empty), those
    of the last box column and row aimed 4 px inside the right and 3 px inside the lower image border (the ragged tiles
    where the camera has them: part of such a cluster falls off the image), plus background over the image and around
    it.  The cloud is in the camera frame (cam_lidar is the identity, as in test_gpu_pose) and holds 8192 points at the
    most: a fresh handle keeps its 4096 buckets."""
    cam = CAMERAS[cam_name]
    rng = np.random.default_rng([sorted(CAMERAS).index(cam_name), nb, 5])
    boxes, cols, rows = pose_boxes(cam, nb)
    hi = 41 if nb <= 128 else 25
    pts = []
    for i, b in enumerate(boxes):
        if i % 7 == 6:
            continue
        u, v = P.box_centre(b)
        if b["x_max"] >= cam.w - 1e-9 and i % 2 == 0:
            u = cam.w - 4.0
        if b["y_max"] >= cam.h - 1e-9 and i % 3 == 0:
            v = cam.h - 3.0
        # the 0.24 m of a cluster span a quarter of the box or less; neighbouring clusters are a metre apart or more
        zc = max(3.0, max(cam.fx, cam.fy) / min(cam.w / cols, cam.h / rows)) * (1.0 + 0.1 * (i % 5))
        pts.append(P._segment(rng, np.array(ray_point(cam, u, v, zc)), int(rng.integers(12, hi))))
    zc = max(3.0, max(cam.fx, cam.fy) / min(cam.w / cols, cam.h / rows)) * 1.7
    for f in (0.21, 0.52, 0.83):               # six more along the two borders, in whichever box is there
        pts.append(P._segment(rng, np.array(ray_point(cam, cam.w - 4.0, f * cam.h, zc)), int(rng.integers(12, hi))))
        pts.append(P._segment(rng, np.array(ray_point(cam, f * cam.w, cam.h - 3.0, zc)), int(rng.integers(12, hi))))
    nbg = 1200
    bu, bv, bz = rng.uniform(-0.1, 1.1, nbg) * cam.w, rng.uniform(-0.1, 1.1, nbg) * cam.h, rng.uniform(1.0, 50.0, nbg)
    pts.append(np.stack(ray_point(cam, bu, bv, bz), axis=1))
    p = np.vstack(pts)
    p = p[rng.permutation(len(p))]
    assert len(p) <= 8192
    return P._scene(f"{cam_name}-nb-{nb}", p, boxes, empty=[i for i in range(nb) if i % 7 == 6])


# ------------------------------------------------------------------------------------------- the tick's scenes --

@functools.lru_cache(maxsize=None)
def tick_scene(cam_name, nb):
    """a scene with structure for gv_tick (a uniform cloud loses every point to the radius filter): a ground plane, nb
    objects of 150 points, each aimed at a cell of its own of a grid over the image and inside a pixel box of its own
    (fp64 projection: the boxes are inputs), labels cycling so that one box in five is static, and clutter; perturbed
    transforms, shuffled.  Returns (Scene, boxes)."""
    cam, tfs = CAMERAS[cam_name], synth.transforms(True)
    rng = np.random.default_rng([sorted(CAMERAS).index(cam_name), nb, 11])
    cols = int(np.ceil(np.sqrt(nb * cam.w / cam.h)))
    rows = (nb + cols - 1) // cols
    cw, ch = cam.w / cols, cam.h / rows
    tf = tfs["cam_lidar"]
    r, t = synth._quat_to_matrix(tf[:4]), np.asarray(tf[4:7], np.float64)
    parts, rects = [], []
    for k in range(nb):
        d = rng.uniform(3.0, 5.0) * max(cam.fx / cw, cam.fy / ch)          # 1.2 m span a third of the cell or less
        c = np.stack(lidar_of(cam, tfs, [(k % cols + 0.5) * cw], [(k // cols + 0.5) * ch], [d]), axis=1)[0].astype(np.float64)
        ang = rng.uniform(0, np.pi)
        a, b_, e = rng.uniform(-0.6, 0.6, 150), rng.uniform(-0.25, 0.25, 150), rng.uniform(-0.4, 0.4, 150)
        p = np.stack([c[0] + a * np.cos(ang) - b_ * np.sin(ang), c[1] + a * np.sin(ang) + b_ * np.cos(ang), c[2] + e], axis=1)
        p = p.astype(F32)
        pc = p.astype(np.float64) @ r.T + t
        u, v = cam.fx * pc[:, 0] / pc[:, 2] + cam.cx, cam.fy * pc[:, 1] / pc[:, 2] + cam.cy
        rects.append((max(0.0, np.percentile(u, 2)) + 0.25, max(0.0, np.percentile(v, 2)) + 0.5,
                      min(cam.w - 1.0, np.percentile(u, 98)) + 0.75, min(cam.h - 1.0, np.percentile(v, 98))))
        parts.append(p)
    ng = 12_000
    gx = rng.uniform(1.0, 60.0, ng)
    parts.append(np.stack([gx, rng.uniform(-30.0, 30.0, ng), -1.75 + 0.004 * gx + rng.normal(0, 0.012, ng)], axis=1).astype(F32))
    nu = 3000
    parts.append(np.stack([rng.uniform(-20, 80, nu), rng.uniform(-45, 45, nu), rng.uniform(-2, 4, nu)], axis=1).astype(F32))
    p = np.vstack(parts)
    p = p[rng.permutation(len(p))]
    b = np.zeros(nb, BBOX_DTYPE)
    for i, rc in enumerate(rects):
        b[i] = tuple(float(F32(q)) for q in rc) + (0.99 - 0.01 * i, [9, 2, 0, 1, 5][i % 5])
    return Scene(cam, True, tfs, np.ascontiguousarray(p[:, 0]), np.ascontiguousarray(p[:, 1]), np.ascontiguousarray(p[:, 2])), b


# ---------------------------------------------------------------------------------- what test_gpu_camera.py runs --

STANDALONE_CASES = [(c, nb, pt) for c in CAMERAS for nb in box_sizes(CAMERAS[c]) for pt in (False, True)]
FRAME_CASES = [("kitti", 64), ("kitti", 65), ("hd720", 1), ("hd720", 129), ("hd1080", 64), ("tiny", 64), ("pixel", 64),
               ("offaxis", 64), ("synth", 64)]
PIPELINE_CASES = [("kitti", (64, 129)), ("hd720", (64, 129))]
SHARD_CASES = [("hd720", 65, 2), ("hd720", 65, 3)]
# hd1080 with 129 boxes: three mask words of 65 KB, more than the 160 KB of LDS a CDNA4 compute unit has -- tables that
# no launch can keep in LDS, whatever the limit in launch_pose_cells says
POSE_CASES = [("kitti", 64), ("kitti", 257), ("hd720", 64), ("hd720", 65), ("hd1080", 1), ("hd1080", 64), ("hd1080", 129),
              ("tiny", 64), ("synth", 64)]
CU_LDS_BYTES = 160 * 1024
KNN_CAMERAS = ("kitti", "offaxis", "tiny")
KNN_KS = (1, 4, 10)
STALE_CASE = ("kitti", (257, 1, 64))
