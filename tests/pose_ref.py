"""extractCloudPerBBox -> RadiusOutlierRemoval(0.4, 10) -> centroid + PCA rectangle (src/cloud_detections.cpp:140-298)
as the DEVICE promises them ("The PCA rectangle's sums"), restated in numpy and integers, and the scenes
the per-box cloud tests run.  No kernel logic lives in the reference half: no cells, no buckets, no runs.

  keep_flags()   all pairs of one box's points; d2 = ((dx*dx) + dy*dy) + dz*dz, every operation one float32 operation;
                 kept when the number of points with d2 <= R2F (the point itself included) is >= 11
  rectangle()    fix_coord: clamp to +-2047, rint(double * 2^28), summed as exact integers; means
                 float32(float64(sum) * (1 / (cnt * 2^28))); centred samples in float32; fix_prod: clamp to +-127, exact
                 fp64 product * 2^26, rint; covariance float32(float64(sum) * (1 / (cnt * 2^26))); the 2x2 eigen step in
                 float64 operation for operation; projections with every product and the one add in float32; extents
                 float32(max) - float32(min); angle float32(float64(float32(atan2) * 180.0f) / pi); hp = -angle / 2
  run()          ids (oracle_lib.extract_cloud_per_bbox, held bit-exact elsewhere) -> per box keep -> pose / valid
  multiset()     sorted rows (id, x bits, y bits, z bits, keep): what the test hook's nodes are compared with

The fixture half (families a .. g) does speak of cells: only to PLACE points where today's kernels take another path.
No expected value comes from there; tests/test_pose_host.py asserts that every family reaches what it was built for.

TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

import oracle_lib as ol
from gvamd.synth import BBOX_DTYPE, LSHAPE_DTYPE
from knn_depth_ref import IDENT_TF, K_SYNTH

F32 = np.float32
IMG_W, IMG_H = 640, 480
MIN_PTS = 10


def floor_to_float(v):
    f = F32(v)
    return f if float(f) <= v else np.nextafter(f, F32(-np.inf))


R2F = floor_to_float(0.4 * 0.4)            # the largest float not above the fp64 radius^2
R2F_UP = np.nextafter(R2F, F32(np.inf))
COORD_CLAMP, CENTRED_CLAMP = F32(2047.0), F32(127.0)
FIX_COORD, FIX_PROD = 2.0 ** 28, 2.0 ** 26


# ------------------------------------------------------------------------------------------------ reference --

def d2_rows(x, y, z, rows):
    """float32 squared distances of the points `rows` (queries) to every point: [len(rows), n]"""
    d = x[None, :] - x[rows, None]
    r = d * d
    d = y[None, :] - y[rows, None]
    r = r + d * d
    d = z[None, :] - z[rows, None]
    r = r + d * d
    assert r.dtype == F32
    return r


def neighbour_counts(x, y, z, r2=R2F):
    """number of points with d2 <= r2 per point, itself included"""
    x, y, z = (np.ascontiguousarray(a, F32) for a in (x, y, z))
    n = len(x)
    out = np.zeros(n, np.int64)
    step = max(1, 4_000_000 // max(n, 1))
    with np.errstate(all="ignore"):
        for i in range(0, n, step):
            rows = np.arange(i, min(n, i + step))
            out[rows] = np.count_nonzero(d2_rows(x, y, z, rows) <= r2, axis=1)
    return out


def keep_flags(x, y, z):
    return neighbour_counts(x, y, z) >= MIN_PTS + 1


def _fkey(a):
    """order-preserving unsigned key of float32 values (-0.0 below +0.0)"""
    b = np.ascontiguousarray(a, F32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def _fmax(a):
    return a[np.argmax(_fkey(a))]


def _fmin(a):
    return a[np.argmin(_fkey(a))]


Rect = namedtuple("Rect", "pose hp cov major atan2_fragile")


def rectangle(x, y, z):
    """pose of one box's KEPT points (float32 camera coordinates); None when there are none"""
    x, y, z = (np.ascontiguousarray(a, F32) for a in (x, y, z))
    n = len(x)
    if n == 0:
        return None
    with np.errstate(all="ignore"):
        def fix_coord(v):
            return np.rint(np.clip(v, -COORD_CLAMP, COORD_CLAMP).astype(np.float64) * FIX_COORD).astype(np.int64)

        inv = 1.0 / (float(n) * FIX_COORD)
        cy, m0, m1 = (F32(float(int(fix_coord(v).sum())) * inv) for v in (y, z, x))
        a, b = z - m0, x - m1
        assert a.dtype == F32 and b.dtype == F32

        def fix_prod(p, q):
            p = np.clip(p, -CENTRED_CLAMP, CENTRED_CLAMP).astype(np.float64)
            q = np.clip(q, -CENTRED_CLAMP, CENTRED_CLAMP).astype(np.float64)
            return int(np.rint((p * q) * FIX_PROD).astype(np.int64).sum())

        sc = 1.0 / (float(n) * FIX_PROD)
        c00, c01, c11 = (float(F32(float(s) * sc)) for s in (fix_prod(a, a), fix_prod(a, b), fix_prod(b, b)))
        # pca_axes (gv_cloudops.hip) / gvo_pca_bbox (oracle/cloud_detections.c), float64
        if c01 == 0.0:
            mjx, mjy = (1.0, 0.0) if c00 >= c11 else (0.0, 1.0)
        else:
            tr, df = c00 + c11, c00 - c11
            root = math.sqrt(df * df + 4.0 * c01 * c01)
            l1 = 0.5 * (tr + root)
            mjx, mjy = c01, l1 - c00
            if abs(l1 - c11) > abs(mjy):
                mjx, mjy = l1 - c11, c01
            nn = math.sqrt(mjx * mjx + mjy * mjy)
            mjx, mjy = mjx / nn, mjy / nn
        if mjx < 0 or (mjx == 0 and mjy < 0):
            mjx, mjy = -mjx, -mjy
        Mx, My, Nx, Ny = F32(mjx), F32(mjy), F32(-mjy), F32(mjx)
        pl = a * Mx + b * My
        pw = a * Nx + b * Ny
        assert pl.dtype == F32 and pw.dtype == F32
        length = F32(_fmax(pl) - _fmin(pl))
        width = F32(_fmax(pw) - _fmin(pw))
        t = math.atan2(float(My), float(Mx))
        # would another correctly working atan2 (a few fp64 ulps away) round to another float32?
        fragile = F32(t * (1 - 1e-15)) != F32(t * (1 + 1e-15))
        angle = F32(np.float64(F32(t) * F32(180.0)) / np.float64(math.pi))
        hp = float(-angle) * 0.5
    pose = np.zeros(1, LSHAPE_DTYPE)[0]
    for f, v in zip(("px", "py", "pz", "qx", "qy", "qz", "qw", "length", "width", "height"),
                    (m1, cy, m0, 0.0, math.sin(hp), 0.0, math.cos(hp), length, width, 0.0)):
        pose[f] = float(v)
    return Rect(pose, hp, (c00, c01, c11), (float(Mx), float(My)), bool(fragile))


def sincos_extended(hp):
    """sin and cos of the float64 hp in extended precision, rounded to float64"""
    t = np.longdouble(hp)
    return float(np.sin(t)), float(np.cos(t))


def ulps64(a, b):
    """distance of two float64 values in units of the spacing at b"""
    return abs(a - b) / np.spacing(max(abs(b), np.finfo(np.float64).tiny))


Result = namedtuple("Result", "ids keep poses valid rects")


def camera_frame(x, y, z):
    """the uploaded cloud through the identity cam_lidar, as the library's transform leaves it (-0.0 becomes +0.0)"""
    return ol.transform_cloud(ol.tf_to_matrix4f(IDENT_TF), x, y, z)


def run(cx, cy, cz, boxes, drop=None, K=K_SYNTH, w=IMG_W, h=IMG_H):
    """one whole call on a camera-frame cloud.  drop: bool mask of points removed before the split (the ground).
    K, w, h: the camera (row-major intrinsics, image size).
    ids[n] (-1: not selected), keep[n] bool, poses[nb], valid[nb], rects[nb] (Rect or None)"""
    cx, cy, cz = (np.ascontiguousarray(a, F32) for a in (cx, cy, cz))
    boxes = np.ascontiguousarray(boxes, BBOX_DTYPE)
    n, nb = len(cx), len(boxes)
    live = np.ones(n, bool) if drop is None else ~np.asarray(drop, bool)
    ids = np.full(n, -1, np.int32)
    ids[live] = ol.extract_cloud_per_bbox(K, cx[live], cy[live], cz[live], boxes, w, h)
    keep = np.zeros(n, bool)
    poses, valid, rects = np.zeros(nb, LSHAPE_DTYPE), np.zeros(nb, np.uint8), [None] * nb
    order = np.argsort(ids, kind="stable")
    bounds = np.searchsorted(ids[order], np.arange(nb + 1))
    for b in range(nb):
        sel = order[bounds[b]:bounds[b + 1]]
        if not len(sel):
            continue
        kp = keep_flags(cx[sel], cy[sel], cz[sel])
        keep[sel] = kp
        r = rectangle(cx[sel][kp], cy[sel][kp], cz[sel][kp])
        if r is not None:
            poses[b], valid[b], rects[b] = r.pose, 1, r
    return Result(ids, keep, poses, valid, rects)


def multiset_of(ids, x, y, z, keep):
    """sorted rows (id, x bits, y bits, z bits, keep) as int64[m, 5]"""
    cols = [np.asarray(ids, np.int64)] + [np.ascontiguousarray(a, F32).view(np.uint32).astype(np.int64) for a in (x, y, z)]
    cols.append(np.asarray(keep).astype(np.int64))
    rows = np.stack(cols, axis=1) if len(cols[0]) else np.zeros((0, 5), np.int64)
    return rows[np.lexsort(rows.T[::-1])]


def multiset(res, cx, cy, cz):
    s = res.ids >= 0
    return multiset_of(res.ids[s], cx[s], cy[s], cz[s], res.keep[s])


# -------------------------------------------------------------------------------------------------- fixtures --

Scene = namedtuple("Scene", "tag x y z boxes meta")
CELL = 0.5


def make_boxes(rects):
    b = np.zeros(len(rects), BBOX_DTYPE)
    for i, (u0, v0, u1, v1) in enumerate(rects):
        b[i] = (u0, v0, u1, v1, 0.9, 9)   # a label gv_filter_bboxes calls dynamic
    return b


def grid_boxes(cols, rows, count=None, w=IMG_W, h=IMG_H):
    """cols x rows boxes that tile the w x h image, row major; count: only the first ones"""
    w, h = w / cols, h / rows
    r = [(c * w, q * h, (c + 1) * w, (q + 1) * h) for q in range(rows) for c in range(cols)]
    return make_boxes(r[:count] if count is not None else r)


def box_centre(b):
    return 0.5 * (b["x_min"] + b["x_max"]), 0.5 * (b["y_min"] + b["y_max"])


def ray_point(u, v, zc, K=K_SYNTH):
    """camera point of depth zc that projects to pixel (u, v) under the intrinsics K"""
    return (u - K[2]) / K[0] * zc, (v - K[5]) / K[4] * zc, zc


def cell_of(a):
    return np.floor(np.asarray(a, F32) * F32(2.0)).astype(np.int64)


def _scene(tag, pts, boxes, **meta):
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    return Scene(tag, p[:, 0].astype(F32), p[:, 1].astype(F32), p[:, 2].astype(F32), boxes, meta)


def _segment(rng, c, m, phi=None):
    """m mutually close points: a 0.24 m segment through c in the x-z plane (direction phi from the z axis, random when
    None) with 1 cm of jitter.  Elongated on purpose: the axes of a rectangle are conditioned by the gap between its two
    eigenvalues, and the quaternion takes the angle in DEGREES as radians (cloud_detections.cpp:227, 236)"""
    phi = rng.uniform(0, np.pi) if phi is None else phi
    t = np.linspace(-0.12, 0.12, m)
    return (np.asarray(c)[None, :] + t[:, None] * np.array([np.sin(phi), 0.0, np.cos(phi)])[None, :]
            + rng.uniform(-0.01, 0.01, (m, 3)))


# ---- (a) radius edge

def _edge_point(rng, q, target):
    """a float32 point whose d2 to the float32 query q is exactly `target`"""
    q = np.asarray(q, F32)
    for _ in range(200):
        d = rng.normal(size=(512, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        d = d[np.abs(d[:, 2]) > 0.3]
        c = (q[None, :].astype(np.float64) + 0.4 * d).astype(F32)
        # walk z by whole ulps around the sphere: 33 candidates per direction
        steps = np.arange(-16, 17)
        cz = (c[:, 2:3].view(np.int32) + steps[None, :].astype(np.int32)).view(F32)
        dx, dy, dz = c[:, 0:1] - q[0], c[:, 1:2] - q[1], cz - q[2]
        r = (dx * dx + dy * dy) + dz * dz
        assert r.dtype == F32
        i, j = np.nonzero(r == target)
        if len(i):
            return np.array([c[i[0], 0], c[i[0], 1], cz[i[0], j[0]]], F32)
    raise AssertionError("no edge point found")


def radius_edge_scene(seed=1):
    """8 x 6 boxes, four depths per box: a query, nine points within 2 cm of it and ONE point whose d2 to the query is
    R2F exactly (even slots: the query is kept) or the next float above it (odd slots: dropped)"""
    rng = np.random.default_rng(seed)
    boxes = grid_boxes(8, 6)
    xs, queries = [], []
    slot = 0
    for b in boxes:
        u, v = box_centre(b)
        for zc in (5.0, 6.5, 8.0, 9.5):
            q = np.array(ray_point(u + rng.uniform(-3, 3), v + rng.uniform(-3, 3), zc + rng.uniform(-0.1, 0.1)), F32)
            near = (q[None, :].astype(np.float64) + rng.uniform(-0.012, 0.012, (9, 3))).astype(F32)
            exact = slot % 2 == 0
            e = _edge_point(rng, q, R2F if exact else R2F_UP)
            queries.append((len(xs) * 11, exact))
            xs.append(np.vstack([q[None, :], near, e[None, :]]))
            slot += 1
    return _scene("radius-edge", np.vstack(xs), boxes, queries=queries)


# ---- (b) count edge

COUNT_KINDS = (("10", 10, None), ("11", 11, None), ("12", 12, None), ("11-stolen", 11, "stolen"), ("12-stolen", 12, "stolen"),
               ("11-outside", 11, "outside"), ("12-outside", 12, "outside"), ("11-identical", 11, "same"),
               ("10-identical", 10, "same"))


def count_edge_scene(seed=2):
    """per 80 x 80 pixel cell an EARLIER box over its left 30 pixels and a later one over its left 70 (the last 10
    belong to no box); a 0.24 m segment of points at pixel 50 of the later box, 4 m away.  Variants: 10 / 11 / 12 points; the 11th
    moved 25 pixels (0.31 m) to the left, where first match gives it to the earlier box; moved 25 pixels to the right,
    out of every box; 11 and 10 identical points."""
    rng = np.random.default_rng(seed)
    first, second, pts, clusters = [], [], [], []
    cells = [(c * 80.0, r * 80.0) for r in range(6) for c in range(8)]
    zc = 4.0
    for k, (u0, v0) in enumerate(cells[:45]):
        first.append((u0, v0, u0 + 30.0, v0 + 80.0))
        second.append((u0, v0, u0 + 70.0, v0 + 80.0))
        tag, m, kind = COUNT_KINDS[k % len(COUNT_KINDS)]
        c = np.array(ray_point(u0 + 50.0, v0 + 40.0, zc + 0.3 * (k % 3)))
        # along z where the 11th point is moved sideways, so that it stays within the radius of all the others
        p = _segment(rng, c, m, None if kind in (None, "same") else 0.0)
        if kind == "same":
            p[:] = p[0]
        elif kind is not None:
            du = -25.0 if kind == "stolen" else 25.0
            p[10] = np.array(ray_point(u0 + 50.0 + du, v0 + 40.0, c[2]))
        clusters.append((tag, sum(len(t) for t in pts), m, kind))
        pts.append(p)
    boxes = make_boxes(first + second)   # every `first` box precedes every `second` one
    return _scene("count-edge", np.vstack(pts), boxes, clusters=clusters, n_first=len(first))


# ---- (c) neighbour cells

RESIDUES = (0, 3, 7)
OFFSETS = tuple((dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1))


def _cell_cluster(base, off, q=None):
    """11 points: the query and nine more in cell `base`, and one in cell base + off that all of them need"""
    base, off = np.asarray(base, np.float64), np.asarray(off, np.float64)
    frac = np.where(off > 0, 0.45, np.where(off < 0, 0.05, 0.25))        # the query, 0.05 m from the faces it looks across
    away = np.where(off > 0, -1.0, 1.0)
    q = base * CELL + frac if q is None else np.asarray(q, np.float64)
    fill = q[None, :] + away[None, :] * (np.arange(1, 10)[:, None] * 0.004)
    far = q + off * 0.1 + (0.02 if not off.any() else 0.0)
    return np.vstack([q[None, :], fill, far[None, :]])


def _block_pixels(base):
    lo, hi = (np.asarray(base, np.float64) - 1) * CELL, (np.asarray(base, np.float64) + 2) * CELL
    us = [320.0 + 320.0 * xx / zz for xx in (lo[0], hi[0]) for zz in (lo[2], hi[2])]
    vs = [240.0 + 320.0 * yy / zz for yy in (lo[1], hi[1]) for zz in (lo[2], hi[2])]
    return min(us), max(us), min(vs), max(vs)


def _pick_base(rng, res, sign, used, cols=8, rows=6):
    """a base cell with the residues `res` (mod 8), x and y cells of sign `sign`, whose 3 x 3 x 3 block projects into one
    box of the cols x rows grid and lies five cells or more from every block taken before"""
    bw, bh = IMG_W / cols, IMG_H / rows
    for _ in range(20000):
        iz = res[2] + 8 * int(rng.integers(6, 50))
        mx, my = int(0.8 * iz / 8), int(0.55 * iz / 8)
        ix = sign * (res[0] + 8 * int(rng.integers(1, max(2, mx)))) if sign > 0 else -(8 * int(rng.integers(1, max(2, mx))) - res[0])
        iy = sign * (res[1] + 8 * int(rng.integers(1, max(2, my)))) if sign > 0 else -(8 * int(rng.integers(1, max(2, my))) - res[1])
        u0, u1, v0, v1 = _block_pixels((ix, iy, iz))
        if not (2 < u0 and u1 < IMG_W - 2 and 2 < v0 and v1 < IMG_H - 2):
            continue
        if int((u0 - 1) // bw) != int((u1 + 1) // bw) or int((v0 - 1) // bh) != int((v1 + 1) // bh):
            continue
        b = np.array((ix, iy, iz))
        if len(used) and (np.abs(np.asarray(used) - b[None, :]).max(axis=1) < 6).any():
            continue
        used.append(b)
        return b
    raise AssertionError("no room for a cluster")


def neighbour_cell_scene(sign, seed=3):
    """27 residues x 27 offsets, x and y cells positive (sign = 1) or negative (-1), 48 boxes"""
    rng = np.random.default_rng(seed + (sign < 0))
    used, pts, clusters = [], [], []
    for rz in RESIDUES:
        for ry in RESIDUES:
            for rx in RESIDUES:
                for off in OFFSETS:
                    base = _pick_base(rng, (rx, ry, rz), sign, used)
                    clusters.append((tuple(int(t) for t in base), off))
                    pts.append(_cell_cluster(base, off))
    return _scene("cells-positive" if sign > 0 else "cells-negative", np.vstack(pts), grid_boxes(8, 6), clusters=clusters)


def straddle_scene(bx, by):
    """the same clusters around x = 0 and y = 0: base cell bx in x and by in y (0 or -1 each), every offset, the z
    residues in turn; one box around the image centre.  The clusters follow each other along the optical axis with an
    empty cell or more between their blocks, 108 m in all: the centred clamp stays out of it"""
    pts, clusters = [], []
    iz = 44
    for k, off in enumerate(OFFSETS):
        iz += 4
        while iz % 8 != RESIDUES[k % 3]:
            iz += 1
        clusters.append(((bx, by, iz), off))
        pts.append(_cell_cluster((bx, by, iz), off))
    return _scene(f"cells-straddle-0[{bx},{by}]", np.vstack(pts), make_boxes([(250.0, 170.0, 390.0, 310.0)]), clusters=clusters)


def face_scene():
    """points exactly ON cell faces: 11-point columns at x in {+0.0, -0.0, 0.5, -0.5, 1.0} and y in {+0.0, -0.0, 0.5,
    -0.5} with z on multiples of 1/32 from a multiple of 0.5 on, 2.5 m apart, one box"""
    cols = []
    zf = 20.0
    for fx in (0.0, -0.0, 0.5, -0.5, 1.0):
        for fy in (0.0, -0.0, 0.5, -0.5):
            cols.append(np.array([(fx, fy, zf + k / 32.0) for k in range(11)]))
            zf += 2.5
    return _scene("cells-faces", np.vstack(cols), make_boxes([(250.0, 170.0, 390.0, 310.0)]), n_face=len(cols))


def iz0_scenes():
    """base cells with iz = 0 (0.001 < z < 0.5).  A point there projects into the image only while |x| < z and
    |y| < 0.75 z, so the base cells are 0 and -1 in x and y, the offsets point at z cells 0 and 1 and, in x and y, at
    the own cell or across the coordinate's zero; the clusters all sit within a metre of the camera, so each is a scene
    of its own with one box over the whole image (32 scenes of 11 points)"""
    out = []
    box = make_boxes([(0.0, 0.0, 640.0, 480.0)])
    for bx in (0, -1):
        for by in (0, -1):
            for dz in (0, 1):
                for dy in (0, -1 if by == 0 else 1):
                    for dx in (0, -1 if bx == 0 else 1):
                        def coord(b, d):
                            return (0.10 if d == 0 else 0.03) * (1 if b == 0 else -1)
                        q = (coord(bx, dx), coord(by, dy), 0.40 if dz == 0 else 0.47)
                        p = _cell_cluster((bx, by, 0), (dx, dy, dz), q)
                        out.append(_scene(f"cells-iz0[{bx},{by}]{dx:+d}{dy:+d}{dz:+d}", p, box, clusters=[((bx, by, 0), (dx, dy, dz))]))
    return out


# ---- (d) long runs

RUN_LENGTHS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 200)


def long_run_scene(seed=4):
    """per L: a query 0.02 m below the +y and +z faces of its cell, its ten partners just across both (the row of cells
    a walk reaches last), and L points of the same box in the far corner of the query's own cell and of the cells on
    either side of it along x -- more than 0.4 m from the query, so every one of them is a candidate that fails.  Once
    with the query's x cell = 0 and once = 7 (mod 8).  Last: a query at 0.3 m of its cell on every axis with one
    point of its box in each of the 27 cells around it, exactly ten of them within the radius (ix = 0 and 7 mod 8)."""
    rng = np.random.default_rng(seed)
    used, pts, clusters = [], [], []
    for rx in (0, 7):
        for L in RUN_LENGTHS:
            base = _pick_base(rng, (rx, int(rng.choice(RESIDUES)), int(rng.choice(RESIDUES))), 1, used)
            o = base.astype(np.float64) * CELL
            q = o + np.array([0.25, 0.48, 0.48])
            partners = o[None, :] + np.array([0.25, 0.52, 0.52])[None, :] + rng.uniform(-0.015, 0.015, (10, 3))
            far = [o[None, :] + np.array([0.25 + sx * CELL, 0.03, 0.03])[None, :] + rng.uniform(-0.02, 0.02, (L, 3)) for sx in (0, -1, 1)]
            clusters.append(("run", tuple(int(t) for t in base), L, sum(len(p) for p in pts)))
            pts.append(np.vstack([q[None, :], partners] + far))
    for rx in (0, 7):
        base = _pick_base(rng, (rx, 3, 3), 1, used)
        o = base.astype(np.float64) * CELL
        q = o + 0.3
        ring = []
        for off in OFFSETS:
            off = np.asarray(off, np.float64)
            d = np.where(off > 0, 0.21, np.where(off < 0, -0.31, 0.0))
            # ten of the 26 within the radius: the six across a face, the three across an edge in (+, +) and the corner
            # (+, +, +); the others are pushed past 0.4 m
            ring.append(q + d * (1.15 if (off < 0).any() and np.count_nonzero(off) >= 2 else 1.0))
        ring = [r for r in ring if np.abs(r - q).max() > 0]
        clusters.append(("all-27", tuple(int(t) for t in base), 0, sum(len(p) for p in pts)))
        pts.append(np.vstack([q[None, :]] + [r[None, :] for r in ring]))
    return _scene("long-runs", np.vstack(pts), grid_boxes(8, 6), clusters=clusters)


# ---- (e) far points

def far_scene():
    """five boxes, one cluster each: z = 3e6 with x, y on a 0.05 m lattice (z spacing there: 0.25 m); x = 1.5e6, z = 3e6;
    eleven copies of one point at z = 1e30; 41 points 0.01 m apart across z = 2047 m; two 30-point clusters of one box
    300 m apart in z"""
    k = np.arange(-3, 4) * 0.05
    a = np.array([(xx, yy, 3.0e6 + dz) for dz in (0.0, 0.25, 0.5) for yy in k for xx in k])
    b = np.array([(1.5e6 + dx, yy, 3.0e6 + dz) for dz in (0.0, 0.25) for dx in (0.0, 0.125, 0.25) for yy in k])
    c = np.tile(np.array([(-0.5e30, 0.0, 1.0e30)]), (11, 1))
    zs = 2047.0 + np.arange(-20, 21) * 0.01
    d = np.array([(0.0, 0.5 * 2047.0, t) for t in zs])
    e = np.vstack([np.array([(0.01 * (i % 5), -0.5 * zc, zc + 0.01 * i) for i in range(30)]) for zc in (100.0, 400.0)])
    boxes = make_boxes([(290.0, 210.0, 350.0, 270.0), (450.0, 210.0, 510.0, 270.0), (130.0, 210.0, 190.0, 270.0),
                        (290.0, 370.0, 350.0, 430.0), (290.0, 50.0, 350.0, 110.0)])
    parts = (a, b, c, d, e)
    return _scene("far", np.vstack(parts), boxes, parts=[len(p) for p in parts])


# ---- (f) degenerate rectangles

DEGENERATE = ("equal", "line-z", "line-x", "square", "diagonal", "one-cluster")


def degenerate_scene():
    """six boxes on dyadic coordinates (every sum exact): 11 equal points; a line along z; a line along x; a 6 x 6 square
    lattice (c00 == c11, c01 == 0); an 8 x 3 lattice turned by 45 degrees (c00 == c11, c01 != 0: a turned SQUARE has
    c01 == 0 again); one 11-point cluster beside 7 lone points that the filter drops"""
    boxes = grid_boxes(3, 2)
    pts, parts = [], []
    for i, kind in enumerate(DEGENERATE):
        u, v = box_centre(boxes[i])
        zc = 16.0
        x0, y0 = round((u - 320.0) / 320.0 * zc * 8) / 8, round((v - 240.0) / 320.0 * zc * 8) / 8
        if kind == "equal":
            p = np.tile(np.array([(x0, y0, zc)]), (11, 1))
        elif kind == "line-z":
            p = np.array([(x0, y0, zc + k / 32.0) for k in range(24)])
        elif kind == "line-x":
            p = np.array([(x0 + k / 32.0, y0, zc) for k in range(24)])
        elif kind == "square":
            p = np.array([(x0 + j / 8.0, y0, zc + k / 8.0) for k in range(6) for j in range(6)])
        elif kind == "diagonal":
            p = np.array([(x0 + (k - j) / 16.0, y0, zc + (k + j) / 16.0) for k in range(8) for j in range(3)])
        else:
            p = np.array([(x0 + k / 64.0, y0 + (k % 3) / 64.0, zc + (k % 4) / 64.0) for k in range(11)]
                         + [(x0 - 0.5 + 0.07 * k, y0 + 0.6, zc + 1.0 + 0.9 * k) for k in range(7)])
        pts.append(p)
        parts.append(len(p))
    return _scene("degenerate", np.vstack(pts), boxes, parts=parts)


# ---- (g) sizes

NB_SIZES = (1, 63, 64, 65, 127, 128, 129, 300)
CLOUD_SIZES = (1, 4095, 4096, 4097)
SELECTED_SIZES = (0, 1, 31, 32, 33, 127, 128, 129)


def _twelve(rng, u, v, zc):
    return _segment(rng, np.array(ray_point(u, v, zc)), 12)


def nb_scene(nb, seed=5):
    """nb boxes of a 20 x 15 grid, a 12-point cluster in each -- except every seventh, which stays empty"""
    rng = np.random.default_rng(seed + nb)
    boxes = grid_boxes(20, 15, nb)
    pts = [_twelve(rng, *box_centre(b), 20.0 + (i % 5)) for i, b in enumerate(boxes) if i % 7 != 6]
    return _scene(f"nb-{nb}", np.vstack(pts), boxes, empty=[i for i in range(nb) if i % 7 == 6])


def cloud_size_scene(n, seed=6):
    """n points in all: 12-point clusters in 8 x 6 boxes as far as n reaches, the rest behind the camera"""
    rng = np.random.default_rng(seed + n)
    boxes = grid_boxes(8, 6)
    pts = np.vstack([_twelve(rng, *box_centre(b), 15.0) for b in boxes])[:n]
    rest = n - len(pts)
    back = np.stack([rng.uniform(-5, 5, rest), rng.uniform(-5, 5, rest), rng.uniform(-30, -1, rest)], axis=1)
    p = np.vstack([pts, back])
    return _scene(f"cloud-{n}", p[rng.permutation(n)] if n > 1 else p, boxes)


def selected_scene(s, seed=7):
    """one box; s points inside it (one dense cluster), 40 beside it and 40 behind the camera"""
    rng = np.random.default_rng(seed + s)
    c = np.array(ray_point(320.0, 240.0, 12.0))
    inside = c[None, :] + rng.uniform(-0.15, 0.15, (s, 3))
    beside = np.array(ray_point(600.0, 440.0, 12.0))[None, :] + rng.uniform(-0.1, 0.1, (40, 3))
    back = np.stack([rng.uniform(-5, 5, 40), rng.uniform(-5, 5, 40), rng.uniform(-30, -1, 40)], axis=1)
    p = np.vstack([inside, beside, back])
    return _scene(f"selected-{s}", p[rng.permutation(len(p))], make_boxes([(280.0, 200.0, 360.0, 280.0)]), selected=s)


# ---- the large cloud that grows a handle's bucket table, and the ground scene

def behind_camera_cloud(n=1_100_000, seed=8):
    """n points with z < 0: nothing is selected; the bucket table grows to 2^20 buckets"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-50, 50, n).astype(F32), rng.uniform(-50, 50, n).astype(F32), rng.uniform(-80, -1, n).astype(F32))


def with_plane(scene, seed=9, n_plane=6000):
    """the scene plus a planted plane y = 30 m + 1 cm of noise (below every cluster, inside the image)"""
    rng = np.random.default_rng(seed)
    pz = rng.uniform(45.0, 120.0, n_plane)
    px = rng.uniform(-0.9, 0.9, n_plane) * pz
    py = 30.0 + rng.normal(0, 0.01, n_plane)
    p = np.vstack([np.stack([scene.x, scene.y, scene.z], axis=1).astype(np.float64), np.stack([px, py, pz], axis=1)])
    p = p[rng.permutation(len(p))]
    return _scene(scene.tag + "+plane", p, scene.boxes)


FAMILIES = ("radius-edge", "count-edge", "cells", "long-runs", "far", "degenerate", "sizes")
_CACHE = {}


def family(name):
    """the scenes of one family (built once)"""
    if name not in _CACHE:
        _CACHE[name] = {
            "radius-edge": lambda: [radius_edge_scene()],
            "count-edge": lambda: [count_edge_scene()],
            "cells": lambda: [neighbour_cell_scene(1), neighbour_cell_scene(-1), face_scene()]
                             + [straddle_scene(bx, by) for bx in (0, -1) for by in (0, -1)]
                             + iz0_scenes(),
            "long-runs": lambda: [long_run_scene()],
            "far": lambda: [far_scene()],
            "degenerate": lambda: [degenerate_scene()],
            "sizes": lambda: [nb_scene(nb) for nb in NB_SIZES] + [cloud_size_scene(n) for n in CLOUD_SIZES]
                             + [selected_scene(s) for s in SELECTED_SIZES],
        }[name]()
    return _CACHE[name]


_REF = {}


def reference(scene, K=K_SYNTH, w=IMG_W, h=IMG_H):
    """(camera-frame cloud, Result) of a scene at the camera K, w, h, computed once and shared"""
    key = (scene.tag, tuple(float(t) for t in K), w, h)
    if key not in _REF:
        cam = camera_frame(scene.x, scene.y, scene.z)
        _REF[key] = (cam, run(*cam, scene.boxes, K=K, w=w, h=h))
    return _REF[key]
