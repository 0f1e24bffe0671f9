"""The partition pass (k_bin_partition, gv_binning.hip) handles four points per lane and step in straight-line code and
keeps each point's predicates -- finite, in the rectangle, obstacle / ground / above the band, in front of the camera,
in the image, in a box -- in lane masks or in the point's own values.  Whatever form they are kept in, a predicate that
leaks from one batch slot to the next, or from a live lane to a dead one, shows up here: clouds deal 37 point classes
round-robin (37 is coprime to the 64 lanes and the 512 threads, so every class lands in every batch slot, in low and
high lanes, beside every other class) and end inside a chunk, inside a slot, and on a chunk boundary.  hits, miss,
bbox_id and cell_idx are compared element for element with the CPU oracle, under every flag combination that selects
another instantiation of the kernel, with the height band clearing and with it off."""
import numpy as np
import pytest

import height_band_ref as ref
import oracle_lib as ol
from gvamd import synth

pytestmark = pytest.mark.gpu

GRID = (100, 100, 0.5)            # 200 x 200 cells: nx % 4 == 0, the tile path
RES = 0.5
X_LO, X_HI, Y_LO, Y_HI = -17.0, 83.0, -50.0, 50.0   # map rectangle: -17 < x <= 83, -50 < y <= 50 (pos_x = 33)
BAND = (0.3, 2.5, 1)              # base z = lidar z + 1.8
CHUNK, THREADS, SLOTS = 2048, 512, 4   # points per partition workgroup, threads, points per lane
SIZES = (2048 + 512 + 37, 300, 4096)
W, H = synth.IMG_W, synth.IMG_H
NEAR = 2.5e-4                     # "a few float ulps" at the scale of the image bounds (ulp(640) = 6.1e-5)
F32 = np.float32

# pixel boxes: 0 and 1 overlap (first match wins), 2 has edges on exactly representable projections (u = 320, v = 240)
BOXES = [(100, 100, 200, 200), (150, 150, 260, 260), (320, 240, 400, 300), (400, 50, 500, 120), (20, 300, 90, 400),
         (500, 300, 620, 460), (300, 10, 340, 60), (0, 0, 30, 30)]


def _boxes():
    b = np.zeros(len(BOXES), dtype=synth.BBOX_DTYPE)
    for i, (x0, y0, x1, y1) in enumerate(BOXES):
        b[i]["x_min"], b[i]["y_min"], b[i]["x_max"], b[i]["y_max"] = x0, y0, x1, y1
        b[i]["confidence"], b[i]["label"] = 0.9 - 0.01 * i, i
    return b


def _poses():
    p = np.zeros(3, dtype=synth.LSHAPE_DTYPE)
    p["px"], p["py"], p["qw"] = [10.0, 40.0, 82.5], [5.0, -20.0, 49.0], 1.0   # the last one crosses the border: skipped
    p["length"], p["width"], p["height"] = [4.0, 2.0, 3.0], [2.0, 1.0, 2.5], 1.5
    return p


class Geo:
    """the oracle's view of a cloud: base and camera coordinates, projection, box membership"""

    def __init__(self, tfs, x, y, z):
        self.m_base, self.m_cam = ol.tf_to_matrix4f(tfs["base_lidar"]), ol.tf_to_matrix4f(tfs["cam_lidar"])
        self.bx, self.by, self.bz = ol.transform_cloud(self.m_base, x, y, z)
        self.cx, self.cy, self.cz = ol.transform_cloud(self.m_cam, x, y, z)
        with np.errstate(all="ignore"):
            X, Y, Z = (a.astype(np.float64) for a in (self.cx, self.cy, self.cz))
            self.u = ((synth.FX * X + synth.CX * Z) / Z).astype(F32)   # (float)(K row . p / z), src/cloud_detections.cpp:268-273
            self.v = ((synth.FY * Y + synth.CY * Z) / Z).astype(F32)
            self.fin_b = np.isfinite(self.bx) & np.isfinite(self.by) & np.isfinite(self.bz)
            self.inmap = self.fin_b & (self.bx > X_LO) & (self.bx <= X_HI) & (self.by > Y_LO) & (self.by <= Y_HI)
            self.front = np.isfinite(self.cx) & np.isfinite(self.cy) & np.isfinite(self.cz) & ~(self.cz <= F32(0.001))
            self.inimg = self.front & ~((self.u < 0) | (self.u >= W) | (self.v < 0) | (self.v >= H))
            u, v = self.u.astype(np.float64), self.v.astype(np.float64)
            self.nbox = np.zeros(len(x), int)
            self.edge = np.zeros(len(x), bool)
            for (x0, y0, x1, y1) in BOXES:
                inside = self.inimg & (u >= x0) & (u <= x1) & (v >= y0) & (v <= y1)
                self.nbox += inside
                self.edge |= inside & ((u == x0) | (u == x1) | (v == y0) | (v == y1))


def _pixel(u, v, d):
    """lidar-frame point that projects near (u, v) at depth d with the unperturbed transforms
    (x_cam = -y, y_cam = 0.4 - z, z_cam = x - 0.3)"""
    u, v, d = (np.asarray(a, np.float64) for a in (u, v, d))
    return (d + 0.3).astype(F32), (-(u - synth.CX) * d / synth.FX).astype(F32), (0.4 - (v - synth.CY) * d / synth.FY).astype(F32)


def _steps(a, k):
    """float32 values k ulps away from a (k an int array)"""
    a = np.asarray(a, F32).copy()
    for _ in range(int(np.max(np.abs(k))) if len(k) else 0):
        up, dn = np.nextafter(a, F32(np.inf)), np.nextafter(a, F32(-np.inf))
        a = np.where(k > 0, up, np.where(k < 0, dn, a))
        k = k - np.sign(k)
    return a


def _near(tfs, rng, n, axis, bound, above):
    """n points whose projection lies within NEAR of u = bound (axis 0) or v = bound (axis 1), on the asked side, the
    other coordinate well inside the image: candidates a few ulps around the solution, kept by what they project to"""
    out = [np.zeros(0, F32)] * 3
    while len(out[0]) < n:
        m = 8 * n
        d = rng.choice([1.0, 2.5, 7.0], m)
        other = rng.uniform(0.25, 0.75, m) * (H if axis == 0 else W)
        x, y, z = _pixel(np.where(axis == 0, bound, other), np.where(axis == 0, other, bound), d)
        k = rng.integers(-4, 5, m)
        if axis == 0:
            y = _steps(y, k)
        else:
            z = _steps(z, k)
        g = Geo(tfs, x, y, z)
        p = g.u if axis == 0 else g.v
        keep = g.front & (np.abs(p.astype(np.float64) - bound) <= NEAR) & ((p >= bound) == above)
        out = [np.concatenate([o, a[keep]]) for o, a in zip(out, (x, y, z))]
    return tuple(o[:n] for o in out)


def _uniform_in_map(rng, n, zlo, zhi):
    return (rng.uniform(1.0, 80.0, n).astype(F32), rng.uniform(-45.0, 45.0, n).astype(F32), rng.uniform(zlo, zhi, n).astype(F32))


def _special(rng, n, axis, val):
    p = list(_uniform_in_map(rng, n, -1.4, 0.6))
    p[axis] = np.full(n, val, F32)
    return tuple(p)


def _cz_side(tfs, rng, n, above):
    """cz on one side of 0.001 within a few ulps, projecting to (320, 240): the corner of box 2 when in front"""
    out = [np.zeros(0, F32)] * 3
    while len(out[0]) < n:
        m = 8 * n
        x = _steps(np.full(m, 0.301, F32), rng.integers(-6, 7, m))
        y, z = np.zeros(m, F32), np.full(m, 0.4, F32)
        g = Geo(tfs, x, y, z)
        keep = (np.abs(g.cz - F32(0.001)) < 1e-6) & ((g.cz > F32(0.001)) == above)
        out = [np.concatenate([o, a[keep]]) for o, a in zip(out, (x, y, z))]
    return tuple(o[:n] for o in out)


def _edge(rng, n):
    """u = 320 exactly (y = 0) with v inside box 2, or v = 240 exactly (z = 0.4) with u inside it, alternating"""
    d = rng.uniform(1, 30, n)
    _, y, z = _pixel(rng.uniform(325, 395, n), rng.uniform(245, 295, n), d)
    first = np.arange(n) % 2 == 0
    return (d + 0.3).astype(F32), np.where(first, F32(0), y), np.where(first, z, F32(0.4))


# (name, generator(tfs, rng, n) -> x, y, z, check(Geo, oracle ids, oracle cell) -> bool per point)
CLASSES = [
    ("nan_x", lambda t, r, n: _special(r, n, 0, np.nan), lambda g, i, c: ~g.fin_b & ~g.front),
    ("nan_y", lambda t, r, n: _special(r, n, 1, np.nan), lambda g, i, c: ~g.fin_b & ~g.front),
    ("nan_z", lambda t, r, n: _special(r, n, 2, np.nan), lambda g, i, c: ~g.fin_b & ~g.front),
    ("+inf_x", lambda t, r, n: _special(r, n, 0, np.inf), lambda g, i, c: ~g.fin_b & ~g.front),
    ("-inf_x", lambda t, r, n: _special(r, n, 0, -np.inf), lambda g, i, c: ~g.fin_b & ~g.front),
    ("+inf_y", lambda t, r, n: _special(r, n, 1, np.inf), lambda g, i, c: ~g.fin_b & ~g.front),
    ("-inf_y", lambda t, r, n: _special(r, n, 1, -np.inf), lambda g, i, c: ~g.fin_b & ~g.front),
    ("+inf_z", lambda t, r, n: _special(r, n, 2, np.inf), lambda g, i, c: ~g.fin_b & ~g.front),
    ("-inf_z", lambda t, r, n: _special(r, n, 2, -np.inf), lambda g, i, c: ~g.fin_b & ~g.front),
    ("obstacle", lambda t, r, n: _uniform_in_map(r, n, -1.4, 0.6),
     lambda g, i, c: (c >= 0) & ~(g.bz < F32(BAND[0])) & ~(g.bz > F32(BAND[1]))),
    ("below_ground", lambda t, r, n: _uniform_in_map(r, n, -3.0, -1.6), lambda g, i, c: (c >= 0) & (g.bz < F32(BAND[0]))),
    ("above_z_max", lambda t, r, n: _uniform_in_map(r, n, 0.8, 3.0), lambda g, i, c: (c >= 0) & (g.bz > F32(BAND[1]))),
    ("out_x_lo", lambda t, r, n: (r.uniform(-40, -17.5, n).astype(F32), r.uniform(-45, 45, n).astype(F32), r.uniform(-1.4, 0.6, n).astype(F32)),
     lambda g, i, c: (c < 0) & g.fin_b & (g.bx <= X_LO)),
    ("out_x_hi", lambda t, r, n: (r.uniform(83.5, 110, n).astype(F32), r.uniform(-45, 45, n).astype(F32), r.uniform(-1.4, 0.6, n).astype(F32)),
     lambda g, i, c: (c < 0) & g.fin_b & (g.bx > X_HI)),
    ("out_y_lo", lambda t, r, n: (r.uniform(1, 80, n).astype(F32), r.uniform(-80, -50.5, n).astype(F32), r.uniform(-1.4, 0.6, n).astype(F32)),
     lambda g, i, c: (c < 0) & g.fin_b & (g.by <= Y_LO)),
    ("out_y_hi", lambda t, r, n: (r.uniform(1, 80, n).astype(F32), r.uniform(50.5, 80, n).astype(F32), r.uniform(-3.0, 0.6, n).astype(F32)),
     lambda g, i, c: (c < 0) & g.fin_b & (g.by > Y_HI)),
    # base x (y) exactly on a cell boundary: the quotient is an integer, get_index_fast falls back to the division
    ("boundary_x", lambda t, r, n: ((X_HI - RES * r.integers(1, 199, n)).astype(F32), r.uniform(-45, 45, n).astype(F32), r.uniform(-1.4, 0.6, n).astype(F32)),
     lambda g, i, c: (c >= 0) & (np.rint((X_HI - g.bx.astype(np.float64)) / RES) == (X_HI - g.bx.astype(np.float64)) / RES)),
    ("boundary_y", lambda t, r, n: (r.uniform(1, 80, n).astype(F32), (Y_HI - RES * r.integers(1, 199, n)).astype(F32), r.uniform(-3.0, 0.6, n).astype(F32)),
     lambda g, i, c: (c >= 0) & (np.rint((Y_HI - g.by.astype(np.float64)) / RES) == (Y_HI - g.by.astype(np.float64)) / RES)),
    ("behind_camera", lambda t, r, n: (r.uniform(-16, 0.2, n).astype(F32), r.uniform(-45, 45, n).astype(F32), r.uniform(-1.4, 0.6, n).astype(F32)),
     lambda g, i, c: np.isfinite(g.cz) & (g.cz < 0) & (i < 0)),
    ("cz_below", lambda t, r, n: _cz_side(t, r, n, False), lambda g, i, c: np.isfinite(g.cz) & (g.cz > 0) & ~g.front & (i < 0)),
    ("cz_above", lambda t, r, n: _cz_side(t, r, n, True), lambda g, i, c: g.front & (g.cz < F32(0.0011)) & (i == 2)),
    ("img_left", lambda t, r, n: _pixel(r.uniform(-300, -5, n), r.uniform(20, 460, n), r.uniform(1, 30, n)), lambda g, i, c: g.front & (g.u < 0) & (i < 0)),
    ("img_right", lambda t, r, n: _pixel(r.uniform(645, 900, n), r.uniform(20, 460, n), r.uniform(1, 30, n)), lambda g, i, c: g.front & (g.u >= W) & (i < 0)),
    ("img_top", lambda t, r, n: _pixel(r.uniform(20, 620, n), r.uniform(-300, -5, n), r.uniform(1, 30, n)), lambda g, i, c: g.front & (g.v < 0) & (i < 0)),
    ("img_bottom", lambda t, r, n: _pixel(r.uniform(20, 620, n), r.uniform(485, 800, n), r.uniform(1, 30, n)), lambda g, i, c: g.front & (g.v >= H) & (i < 0)),
    ("u~0-", lambda t, r, n: _near(t, r, n, 0, 0.0, False), lambda g, i, c: g.front & (g.u < 0) & (g.u >= -NEAR) & (i < 0)),
    ("u~0+", lambda t, r, n: _near(t, r, n, 0, 0.0, True), lambda g, i, c: g.inimg & (g.u <= NEAR)),
    ("u~W-", lambda t, r, n: _near(t, r, n, 0, float(W), False), lambda g, i, c: g.inimg & (g.u >= W - NEAR)),
    ("u~W+", lambda t, r, n: _near(t, r, n, 0, float(W), True), lambda g, i, c: g.front & (g.u >= W) & (g.u <= W + NEAR) & (i < 0)),
    ("v~0-", lambda t, r, n: _near(t, r, n, 1, 0.0, False), lambda g, i, c: g.front & (g.v < 0) & (g.v >= -NEAR) & (i < 0)),
    ("v~0+", lambda t, r, n: _near(t, r, n, 1, 0.0, True), lambda g, i, c: g.inimg & (g.v <= NEAR)),
    ("v~H-", lambda t, r, n: _near(t, r, n, 1, float(H), False), lambda g, i, c: g.inimg & (g.v >= H - NEAR)),
    ("v~H+", lambda t, r, n: _near(t, r, n, 1, float(H), True), lambda g, i, c: g.front & (g.v >= H) & (g.v <= H + NEAR) & (i < 0)),
    ("in_no_box", lambda t, r, n: _pixel(r.uniform(420, 480, n), r.uniform(150, 230, n), r.uniform(1, 30, n)), lambda g, i, c: g.inimg & (g.nbox == 0) & (i < 0)),
    ("in_one_box", lambda t, r, n: _pixel(r.uniform(410, 490, n), r.uniform(60, 110, n), r.uniform(1, 30, n)), lambda g, i, c: (g.nbox == 1) & (i == 3)),
    ("in_two_boxes", lambda t, r, n: _pixel(r.uniform(155, 195, n), r.uniform(155, 195, n), r.uniform(1, 30, n)), lambda g, i, c: (g.nbox == 2) & (i == 0)),
    # y = 0 projects to u = 320 exactly, z = 0.4 to v = 240 exactly: the x_min / y_min edges of box 2 (inclusive)
    ("on_box_edge", lambda t, r, n: _edge(r, n),
     lambda g, i, c: g.edge & (i == 2)),
]
NCLS = len(CLASSES)
assert NCLS == 37 and np.gcd(NCLS, 512) == 1 and np.gcd(NCLS, 64) == 1


def _cloud(tfs, n):
    """point i is of class i % 37; its coordinates come from that class's generator"""
    rng = np.random.default_rng(1000 + n)
    x, y, z = np.zeros(n, F32), np.zeros(n, F32), np.zeros(n, F32)
    for c, (_, gen, _) in enumerate(CLASSES):
        idx = np.arange(c, n, NCLS)
        px, py, pz = gen(tfs, rng, len(idx))
        x[idx], y[idx], z[idx] = px, py, pz
    return x, y, z


class Case:
    pass


@pytest.fixture(scope="module")
def cases():
    """clouds, oracle references (computed once, shared by every flag combination) and the check that the reference
    itself sees every class in every batch slot"""
    tfs = synth.transforms(False)
    bboxes = _boxes()
    K = ol.set_intrinsic(synth.FX, synth.FY, synth.CX, synth.CY)
    out = {}
    for n in SIZES:
        c = Case()
        c.tfs, c.bboxes = tfs, bboxes
        c.x, c.y, c.z = _cloud(tfs, n)
        g = Geo(tfs, c.x, c.y, c.z)
        c.ids = ol.extract_cloud_per_bbox(K, g.cx, g.cy, g.cz, bboxes, W, H)
        c.ref = {}
        for band in (BAND, None):
            og = ol.OGrid(*GRID)
            hits, cell, miss = ref.frame(og, g.m_base, c.x, c.y, c.z, band)
            c.ref[band] = (hits, cell, miss.astype(np.int32))
        cell = c.ref[BAND][1]
        # every point is what it was dealt as, by the oracle's own numbers ...
        cls = np.arange(n) % NCLS
        for k, (name, _, check) in enumerate(CLASSES):
            with np.errstate(all="ignore"):
                ok = check(g, c.ids, cell)
            assert ok[cls == k].all(), (n, name)
        # ... so every batch slot (512 consecutive points of a 2048-point chunk) that holds at least 37 live points
        # holds every class, beside live neighbours, and the last one beside dead lanes; and every class sits in low
        # and high lanes of a wavefront
        i = np.arange(n)
        slot = (i % CHUNK) // THREADS
        for ch in range((n + CHUNK - 1) // CHUNK):
            for s in range(SLOTS):
                m = (i // CHUNK == ch) & (slot == s)
                if m.sum() >= NCLS:
                    assert len(set(cls[m])) == NCLS, (n, ch, s)
        if n >= CHUNK:
            assert {(ch, s) for ch, s in zip(i // CHUNK, slot)} >= {(0, s) for s in range(SLOTS)}
            for k in range(NCLS):
                lanes = (i[cls == k] % 64)
                assert (lanes < 32).any() and (lanes >= 32).any(), (n, k)
        # the predicates are really exercised: hits, ray ends, clipped ends, dropped points, boxes 0, 2, 3 and none
        assert (cell >= 0).sum() > n // 4 and (cell < 0).sum() > n // 8
        assert c.ref[BAND][0].sum() > 0 and c.ref[BAND][2].sum() > 0 and c.ref[None][0].sum() > c.ref[BAND][0].sum()
        assert {-1, 0, 2, 3} <= set(c.ids.tolist())
        out[n] = c
    return out


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


def _flag_sets(gvamd):
    B, R, X, K = gvamd.FRAME_BIN, gvamd.FRAME_RAYMARCH, gvamd.FRAME_BBOX_TEST, gvamd.FRAME_KEEP_CELL_IDX
    # k_bin_partition<RAY, BBOX, KEEPCELL>: all eight
    return [B | R | X | K, B | R | X, B | R | K, B | R, B | X | K, B | X, B | K, B]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("band", [BAND, None], ids=["band_clears", "band_off"])
def test_partition_predicates_every_slot(gvamd, cases, n, band):
    c = cases[n]
    hits, cell, miss = c.ref[band]
    h = gvamd.GridVisionHIP(*GRID)
    h.set_transforms(c.tfs["cam_lidar"], c.tfs["base_cam"], c.tfs["base_lidar"])
    if band is not None:
        h.set_height_band(*band)
    h.upload_xyz(c.x, c.y, c.z)
    poses = _poses()
    for flags in _flag_sets(gvamd):
        h.process_frame(flags | gvamd.FRAME_KEEP_COUNTS, bboxes=c.bboxes if flags & gvamd.FRAME_BBOX_TEST else None, poses=poses)
        assert np.array_equal(h.hits(), hits), flags
        if flags & gvamd.FRAME_RAYMARCH:
            assert np.array_equal(h.miss(), miss), flags
        if flags & gvamd.FRAME_BBOX_TEST:
            assert np.array_equal(h.bbox_id(), c.ids), flags
        if flags & gvamd.FRAME_KEEP_CELL_IDX:
            assert np.array_equal(h.cell_idx(), cell), flags
    h.close()
