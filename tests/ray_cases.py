"""Scenes for the sector ray stage, end by end: pure numpy, no GPU, no oracle.

A scene is a grid, a base<-lidar transform (identity rotation, the sensor at the centre of a chosen origin cell), a
lidar-frame fp32 cloud and the ray ends the cloud INTENDS, one per point: (ix, iy, kind), kind HIT (the point lies at
the centre of that cell) or CLIP (the point lies outside the map on the line from the origin-cell centre through the
middle of that border cell's outer face, twice as far as the face: the slab clip lands on the face).  Whether the
intended ends are the ends the oracle finds is checked by tests/test_ray_cases_host.py, not assumed here.

Octant o (the kernel's numbering): bit 2 = the major axis is x, bit 1 = the major step is +, bit 0 = the minor step
is +; an end at octant-local offset (a, b) has major offset a and minor offset b, 0 <= b <= a.  Minor offset 0 belongs
to the + side and the diagonal to the x-major octant, as in grid_map::LineIterator."""
from collections import namedtuple

import numpy as np

import traj_ref

HIT, CLIP = 1, 2

G64 = (16, 16, 0.25)        # 64 x 64 cells: one tile, 8 sectors per octant
G62 = (31, 31, 0.5)         # 62 x 62 cells: nx % 4 != 0, the generic path
G1024 = (128, 128, 0.125)   # 1024 x 1024 cells
G5100 = (255, 4, 0.05)      # 5100 x 80 cells: an x wedge beyond 4096 columns
G4200 = (210, 210, 0.05)    # 4200 x 4200 cells: a and b both beyond 4096
O1024_CENTRE, O1024_OFF = (512, 512), (300, 700)
O5100 = (4990, 25)
BAND = 24
SETS = {"g1024_centre": (G1024, O1024_CENTRE), "g1024_off": (G1024, O1024_OFF), "g5100": (G5100, O5100)}

# ------------------------------------------------------------------ the knob sets the GPU suite runs the scenes under
# (tests/test_gpu_ray_ends.py; tests/test_sector_plan_host.py checks on the CPU that the sector plan accepts each pair run)
KNOBS = ("GV_RAY_IMPL", "GV_LOG2M", "GV_LOG2S", "GV_SECTOR_HELPERS", "GV_SECTOR_REORDER", "GV_SECTOR_REV", "GV_CAP",
         "GV_FLAT_DIRECT", "GV_MARCH_LIMIT", "GV_FLAT_K")
TUNE_BD = {"defaults": {}, "log2m4": {"GV_LOG2M": "4"}, "log2s5": {"GV_LOG2S": "5"}, "log2s6": {"GV_LOG2S": "6"},
           "helpers0": {"GV_SECTOR_HELPERS": "0"},
           "helpers1": {"GV_SECTOR_HELPERS": "1"}, "reorder0": {"GV_SECTOR_REORDER": "0"}, "rev0": {"GV_SECTOR_REV": "0"},
           "rev1": {"GV_SECTOR_REV": "1"}}
# the five tail settings of test_sector_tail_policies_agree
TAILS = ({"GV_FLAT_DIRECT": "0"}, {"GV_FLAT_DIRECT": "1000000000"}, {"GV_MARCH_LIMIT": "0"},
         {"GV_MARCH_LIMIT": "100000000", "GV_FLAT_K": "0"}, {"GV_FLAT_DIRECT": "300", "GV_MARCH_LIMIT": "3000", "GV_FLAT_K": "2"})
TAILS_B = {"defaults": {}, **{f"tail{i}": t for i, t in enumerate(TAILS)}}
TUNE_C = {"defaults": {}, "cap2048": {"GV_CAP": "2048"}, **{f"tail{i}": t for i, t in enumerate(TAILS)},
          "helpers0": {"GV_SECTOR_HELPERS": "0"}, "helpers1": {"GV_SECTOR_HELPERS": "1"}}

Scene = namedtuple("Scene", "name grid origin tf x y z ends")   # ends: int array (n, 3) of (ix, iy, kind), one row per point


class Geo:
    """cell centres, faces and the transform of one (grid, origin cell)"""

    def __init__(self, grid, origin):
        self.grid, self.origin = grid, origin
        self.g = g = traj_ref.grid(*grid)
        self.nx, self.ny, self.res = g.nx, g.ny, g.res
        self.hix, self.hiy = g.pos_x + g.off_x, g.pos_y + g.off_y
        self.lox, self.loy = self.hix - g.len_x, self.hiy - g.len_y
        assert 0 <= origin[0] < g.nx and 0 <= origin[1] < g.ny
        self.tx, self.ty = self.centre(*origin)
        self.tf = np.array([0.0, 0.0, 0.0, 1.0, self.tx, self.ty, 0.0])

    def centre(self, ix, iy):
        return self.hix - (ix + 0.5) * self.res, self.hiy - (iy + 0.5) * self.res

    def on_border(self, ix, iy):
        return ix == 0 or iy == 0 or ix == self.nx - 1 or iy == self.ny - 1

    def faces(self, ix, iy):
        """outer faces of a border cell: 'x+', 'x-', 'y+', 'y-' (the + faces are at index 0)"""
        return [f for f, on in (("x+", ix == 0), ("x-", ix == self.nx - 1), ("y+", iy == 0), ("y-", iy == self.ny - 1)) if on]

    def hit_point(self, ix, iy):
        cx, cy = self.centre(ix, iy)
        return cx - self.tx, cy - self.ty

    def clip_point(self, ix, iy, face=None):
        """lidar-frame point outside the map whose clipped end is border cell (ix, iy)"""
        face = face or self.faces(ix, iy)[0]
        fx, fy = self.centre(ix, iy)
        if face[0] == "x":
            fx = self.hix if face == "x+" else self.lox
        else:
            fy = self.hiy if face == "y+" else self.loy
        return 2.0 * (fx - self.tx), 2.0 * (fy - self.ty)

    # ---- octants
    def wedge(self, o):
        """(len, jmax): last in-map major / minor offset of octant o"""
        cx, cy = self.origin
        xmaj, pmaj, pmin = (o >> 2) & 1, (o >> 1) & 1, o & 1
        lx = (self.nx - 1 - cx, cx)
        ly = (self.ny - 1 - cy, cy)
        if xmaj:
            return lx[0 if pmaj else 1], ly[0 if pmin else 1]
        return ly[0 if pmaj else 1], lx[0 if pmin else 1]

    def cell(self, o, a, b):
        """cell of octant-local offset (a, b); b may be negative (the mirrored octant) or exceed a"""
        cx, cy = self.origin
        smaj, smin = (1 if (o >> 1) & 1 else -1), (1 if o & 1 else -1)
        return (cx + smaj * a, cy + smin * b) if (o >> 2) & 1 else (cx + smin * b, cy + smaj * a)

    def inside(self, ix, iy):
        return 0 <= ix < self.nx and 0 <= iy < self.ny

    def octant_ab(self, ix, iy):
        """(octant, a, b) of a cell as LineIterator sees the ray to it"""
        dx, dy = ix - self.origin[0], iy - self.origin[1]
        xmaj = abs(dx) >= abs(dy)
        dmaj, dmin = (dx, dy) if xmaj else (dy, dx)
        return (4 if xmaj else 0) | (2 if dmaj >= 0 else 0) | (1 if dmin >= 0 else 0), abs(dmaj), abs(dmin)

    def perimeter(self):
        nx, ny = self.nx, self.ny
        return ([(x, 0) for x in range(nx)] + [(nx - 1, y) for y in range(1, ny)] +
                [(x, ny - 1) for x in range(nx - 2, -1, -1)] + [(0, y) for y in range(ny - 2, 0, -1)])


def make_scene(geo, name, items):
    """items: (ix, iy, kind) or (ix, iy, CLIP, face), one point each, in cloud order"""
    n = len(items)
    x, y = np.zeros(n), np.zeros(n)
    ends = np.zeros((n, 3), np.int32)
    for k, it in enumerate(items):
        ix, iy, kind = it[:3]
        x[k], y[k] = geo.hit_point(ix, iy) if kind == HIT else geo.clip_point(ix, iy, *it[3:])
        ends[k] = (ix, iy, kind)
    return Scene(name, geo.grid, geo.origin, geo.tf, x.astype(np.float32), y.astype(np.float32), np.zeros(n, np.float32), ends)


def make_scene_arrays(geo, name, ends):
    """make_scene for an int array (n, 3) of (ix, iy, kind), clipped ends through their default face"""
    ends = np.ascontiguousarray(ends, np.int32).reshape(-1, 3)
    ix, iy, clip = ends[:, 0].astype(np.float64), ends[:, 1].astype(np.float64), ends[:, 2] == CLIP
    px, py = geo.hix - (ix + 0.5) * geo.res, geo.hiy - (iy + 0.5) * geo.res
    fxp, fxm = clip & (ends[:, 0] == 0), clip & (ends[:, 0] == geo.nx - 1) & (ends[:, 0] != 0)
    fy = clip & ~fxp & ~fxm
    px = np.where(fxp, geo.hix, np.where(fxm, geo.lox, px))
    py = np.where(fy & (ends[:, 1] == 0), geo.hiy, np.where(fy & (ends[:, 1] != 0), geo.loy, py))
    k = np.where(clip, 2.0, 1.0)
    x, y = k * (px - geo.tx), k * (py - geo.ty)
    return Scene(name, geo.grid, geo.origin, geo.tf, x.astype(np.float32), y.astype(np.float32), np.zeros(len(ends), np.float32), ends)


def expected_hits(geo, scene):
    """hit counts the cloud intends: one per HIT point"""
    e = scene.ends[scene.ends[:, 2] == HIT]
    return np.bincount(e[:, 1].astype(np.int64) * geo.nx + e[:, 0], minlength=geo.nx * geo.ny).astype(np.int32)


# ------------------------------------------------------------------ family A: single end, exhaustive
def origins_a(grid):
    g = traj_ref.grid(*grid)
    return {"centre": (g.nx // 2 - 1, g.ny // 2 + 2), "corner": (g.nx - 1, 0), "edge": (0, g.ny // 2), "near_corner": (1, g.ny - 2)}


def family_a(grid, origin_name):
    """one scene whose points are the FRAMES: every cell a hit end, every border cell a clipped end, and clipped ends
    in the origin cell through every face it touches.  Frame f is points [f : f + 1]."""
    geo = Geo(grid, origins_a(grid)[origin_name])
    items = [(ix, iy, HIT) for iy in range(geo.ny) for ix in range(geo.nx)]
    items += [(ix, iy, CLIP) for ix, iy in geo.perimeter()]
    items += [(*geo.origin, CLIP, f) for f in geo.faces(*geo.origin)]
    return geo, make_scene(geo, f"A-{origin_name}", items)


# ------------------------------------------------------------------ family B: single long ends
def b_majors(ln):
    c = {ln, ln - 1, ln // 2, (ln // 512) * 512} | {a for a in (511, 512, 513) if a <= ln}
    return sorted(a for a in c if a >= 1)


def b_minors(a, jmax):
    c = {0, 1, a, a - 1, a // 2, a // 2 - 1, a // 2 + 1}
    for j in range(2, 10):
        odd = np.arange(1, 1 << j, 2)
        ks = odd if j < 6 else odd[np.round(np.linspace(0, len(odd) - 1, 8)).astype(int)]
        for k in ks:
            r = int(np.floor(a * int(k) / float(1 << j) + 0.5))
            c |= {r - 1, r, r + 1}
    top = min(a, jmax)
    return sorted({min(max(b, 0), top) for b in c})


def b_octant_list(geo, o):
    """(a, b, kinds) of octant o: every end as a hit; a border end also clipped, and as both"""
    ln, jmax = geo.wedge(o)
    out = []
    for a in (b_majors(ln) if ln >= 1 else []):
        for b in b_minors(a, jmax):
            out.append((a, b, (HIT,)))
            if geo.on_border(*geo.cell(o, a, b)):
                out.append((a, b, (CLIP,)))
                out.append((a, b, (HIT, CLIP)))
    return out


def family_b(grid, origin):
    geo = Geo(grid, origin)
    lists = [b_octant_list(geo, o) for o in range(8)]
    scenes = []
    for f in range(max(len(l) for l in lists)):
        items = []
        for o in range(8):
            if f < len(lists[o]):
                a, b, kinds = lists[o][f]
                items += [(*geo.cell(o, a, b), k) for k in kinds]
        scenes.append(make_scene(geo, f"B-{f}", items))
    return geo, scenes, lists


B_SHORT = range(3, 41)


def family_b_short():
    """single short ends on G1024, centre origin: every major offset from 3 to 40, at a shallow and at a steep slope.
    A sector with one end has its threshold column at the end's reach (short ends) or at the first level boundary,
    S / 2 = 16, so the ends of reach 17, 18, 19 are the ones one, two and three columns past it."""
    geo = Geo(G1024, O1024_CENTRE)
    scenes, listed = [], []
    for a in B_SHORT:
        for b in (a // 3, a - 1):
            listed.append((a, b))
            scenes.append(make_scene(geo, f"Bs-{a}-{b}", [(*geo.cell(o, a, b), HIT) for o in range(8)]))
    return geo, scenes, listed


# ------------------------------------------------------------------ family C: shadows
C_BASES = ("ring", "clipped_ring", "band")
C_WIDTHS = (1, 2, 3)


def c_positions():
    """position kinds: (name, function of the wedge length -> minor offset at the border), plus the two straddles"""
    pos = [("b0", lambda ln: 0), ("b1", lambda ln: 1), ("len", lambda ln: ln), ("len-1", lambda ln: ln - 1),
           ("half-1", lambda ln: ln // 2 - 1), ("half", lambda ln: ln // 2), ("half+1", lambda ln: ln // 2 + 1)]
    for j, ks in ((3, (1, 3, 5, 7)), (5, (3, 11, 21, 29)), (7, (5, 43, 85, 123))):
        for k in ks:
            pos.append((f"{k}/2^{j}", lambda ln, k=k, j=j: int(np.floor(ln * k / float(1 << j) + 0.5))))
    return pos + [("axis", None), ("diag", None)]


def c_gap_cells(geo, pos_fn, pos_name, width):
    """border cells a gap removes, in all eight octants"""
    gone = set()
    if pos_fn is not None:
        for o in range(8):
            ln, jmax = geo.wedge(o)
            if ln < 1:
                continue
            b = min(max(pos_fn(ln), 0), ln, jmax)   # clipped to the map: the far column ends at jmax
            b = max(min(b, min(ln, jmax) - width + 1), 0)
            gone |= {geo.cell(o, ln, bb) for bb in range(b, min(b + width, min(ln, jmax) + 1))}
        return gone
    per = geo.perimeter()
    idx = {c: i for i, c in enumerate(per)}
    cx, cy = geo.origin
    if pos_name == "axis":   # minor offsets -1 .. width-1 around each of the four axis directions
        mids = [(0, cy), (geo.nx - 1, cy), (cx, 0), (cx, geo.ny - 1)]
    else:                    # around the border cell each of the four diagonals leaves through
        mids = []
        for sx in (-1, 1):
            for sy in (-1, 1):
                m = min(cx if sx < 0 else geo.nx - 1 - cx, cy if sy < 0 else geo.ny - 1 - cy)
                mids.append((cx + sx * m, cy + sy * m))
    for c in mids:
        for d in range(-1, width):
            gone.add(per[(idx[c] + d) % len(per)])
    return gone


def c_exit_points(geo, ix, iy):
    """where the line from the origin through each of the cells (arrays) crosses the rectangle of the border cells'
    centres, in cell units"""
    cx, cy = geo.origin
    dx, dy = (ix - cx).astype(np.float64), (iy - cy).astype(np.float64)
    lx = np.where(dx > 0, geo.nx - 1 - cx, cx).astype(np.float64)
    ly = np.where(dy > 0, geo.ny - 1 - cy, cy).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.minimum(np.where(dx != 0, lx / np.abs(dx), np.inf), np.where(dy != 0, ly / np.abs(dy), np.inf))
    return cx + t * dx, cy + t * dy


def c_base_ends(geo, base, gone=frozenset()):
    """ends (n, 3) of a base, without the border cells in `gone`.  The band also loses every cell whose direction
    from the origin lies strictly between the gap's two surviving neighbours on the border (less than one cell from
    a removed cell where it leaves the map): the gap's whole radial column, so that the inner rings do not fill the
    shadow the border ring's gap opens."""
    if base == "band":
        iy, ix = np.mgrid[0:geo.ny, 0:geo.nx]
        depth = np.minimum(np.minimum(ix, geo.nx - 1 - ix), np.minimum(iy, geo.ny - 1 - iy))
        keep = depth < BAND
        keep[geo.origin[1], geo.origin[0]] = False
        iy, ix = np.nonzero(keep)
        if gone:
            fx, fy = c_exit_points(geo, ix, iy)
            live = np.ones(len(ix), bool)
            for x, y in gone:
                live &= ~((np.abs(fx - x) < 1.0) & (np.abs(fy - y) < 1.0))
            ix, iy = ix[live], iy[live]
        return np.stack([ix, iy, np.full(len(ix), HIT)], axis=1)
    kind = HIT if base == "ring" else CLIP
    return np.array([(ix, iy, kind) for ix, iy in geo.perimeter() if (ix, iy) not in gone and (kind == CLIP or (ix, iy) != geo.origin)])


def family_c_keys():
    return [(base, w, name) for base in C_BASES for w in C_WIDTHS for name, _ in c_positions()]


def family_c_scene(geo, key):
    """key: (base, width, position name), or (base, 0, None) for the gap-less base scene"""
    base, width, pname = key
    if not width:
        return make_scene_arrays(geo, f"C-{base}-base", c_base_ends(geo, base))
    fn = dict(c_positions())[pname]
    gone = c_gap_cells(geo, fn, pname, width)
    return make_scene_arrays(geo, f"C-{base}-w{width}-{pname}", c_base_ends(geo, base, gone))


# ------------------------------------------------------------------ family C, threshold column
# The sector kernel takes every interior cell of the columns up to T for free, where T + 1 is the smallest "longest
# reach" among the aligned slope-bucket groups of the level that column asks for.  Only one kind of scene makes a cell
# of column T + 1 itself unfree: a cell (lf, j) that is a hit end (reach lf, slope at the middle of its own interval),
# every other end of reach > lf inside the cell's slope interval [(2j-1)/2lf, (2j+1)/2lf) removed, and long ends
# everywhere else, right up to the interval's two edges -- the band's 24 rings are dense enough for that.  With 32
# sectors per octant (wedges of 511 and 512 columns) and lf in (171, 256) the interval is 2 to 3 groups of 1/512 wide:
# it can hold one whole group, whose only end is then the wall cell.  Walls in every third sector of every octant.
T_COLUMNS = (200, 216, 232, 248)
T_SECTORS, T_LOG2S = tuple(range(2, 30, 3)), 5


def t_walls(geo, lf):
    """(octant, lf, j): an interior cell of column lf in each of T_SECTORS"""
    out = []
    for o in range(8):
        for s in T_SECTORS:
            jlo = (2 * lf * s + (1 << T_LOG2S)) >> (T_LOG2S + 1)
            jhi = (2 * lf * (s + 1) + (1 << T_LOG2S)) >> (T_LOG2S + 1)
            assert jhi - jlo >= 4
            out.append((o, lf, (jlo + jhi) // 2))
    return out


def family_t():
    geo = Geo(G1024, O1024_CENTRE)
    base = c_base_ends(geo, "band")
    dx, dy = base[:, 0] - geo.origin[0], base[:, 1] - geo.origin[1]
    xmaj = np.abs(dx) >= np.abs(dy)
    dmaj, dmin = np.where(xmaj, dx, dy), np.where(xmaj, dy, dx)
    octant = np.where(xmaj, 4, 0) | np.where(dmaj >= 0, 2, 0) | np.where(dmin >= 0, 1, 0)
    a, b = np.abs(dmaj).astype(np.int64), np.abs(dmin).astype(np.int64)
    scenes, walls = [], []
    for lf in T_COLUMNS:
        w = t_walls(geo, lf)
        live = np.ones(len(base), bool)
        for o, _, j in w:
            live &= ~((octant == o) & ((2 * j - 1) * a <= 2 * lf * b) & (2 * lf * b < (2 * j + 1) * a))
        cells = np.array([(*geo.cell(o, lf, j), HIT) for o, _, j in w])
        scenes.append(make_scene_arrays(geo, f"T-{lf}", np.concatenate([base[live], cells])))
        walls.append(w)
    return geo, scenes, walls


# ------------------------------------------------------------------ family D: slopes that crowd a bucket
D_SLOPES = ((0, 1), (1, 3), (1, 2), (2, 3), (1, 1))
D_COUNTS = (8, 9, 23, 24, 25, 64)


def d_line(geo, o, p, q, n, variant):
    """(a, b) of n lattice points of the line b/a = p/q in octant o, in cloud order, then two strangers beside it"""
    ln, jmax = geo.wedge(o)
    kmax = min(ln // q, jmax // p if p else ln)
    top = kmax if variant == "far" else kmax - 3
    ks = np.unique(np.round(np.linspace(kmax // 4, top, n)).astype(int))
    assert len(ks) == n and ks[0] >= 1
    ks = list(ks)
    if variant == "mid":   # the longest end in the middle of the cloud, the line's farthest lattice points unused
        ks.insert(n // 2, ks.pop())
    pts = [(k * q, k * p) for k in ks]
    A = min(ln, jmax) - 1
    B = int(np.floor(A * p / float(q) + 0.5))
    return pts, [(A, B + 1), (A, B - 1)]


def family_d():
    geo = Geo(G1024, O1024_CENTRE)
    scenes, lines = [], []
    for p, q in D_SLOPES:
        for n in D_COUNTS:
            for variant in ("far", "mid"):
                items = []
                for o in range(8):
                    pts, strangers = d_line(geo, o, p, q, n, variant)
                    lines.append((o, p, q, n, variant, pts, strangers))
                    items += [(*geo.cell(o, a, b), HIT) for a, b in pts + strangers]
                scenes.append(make_scene(geo, f"D-{p}/{q}-n{n}-{variant}", items))
    return geo, scenes, lines


# ------------------------------------------------------------------ family E: long diagonal
E_MAJORS = (4199, 4150, 4100)


def family_e():
    geo = Geo(G4200, (0, 0))
    assert geo.nx == 4200 and geo.ny == 4200
    items, long_ab = [], []
    for o in (7, 3):   # the x-major and the y-major octant a corner origin leaves
        for a in E_MAJORS:
            for b in (a, a - 1, a - 2, a // 2 + 2048):
                c = geo.cell(o, a, b)
                items.append((*c, HIT))
                long_ab.append((o, a, b))
                if geo.on_border(*c):
                    items.append((*c, CLIP))
    rng = np.random.RandomState(20261019)
    near = set()
    while len(near) < 3000:
        c = (int(rng.randint(0, 220)), int(rng.randint(0, 220)))
        if c != geo.origin:
            near.add(c)
    items += [(*c, HIT) for c in sorted(near)]
    return geo, make_scene(geo, "E", items), long_ab


# ------------------------------------------------------------------ the oracle's results of a scene
# (the only part of this module that is not plain numpy: oracle_lib is imported where it is used)
def oracle_grid(geo):
    import oracle_lib as ol
    og = ol.OGrid(*geo.grid)
    assert (og.nx, og.ny) == (geo.nx, geo.ny)
    return og


def oracle_miss(og, scene):
    """OGrid.raymarch of the scene's cloud: uint8 (G,)"""
    import oracle_lib as ol
    return og.raymarch(ol.tf_to_matrix4f(scene.tf), scene.x, scene.y, scene.z)[0]


def oracle_hits(og, scene):
    import oracle_lib as ol
    return og.bin_points(ol.tf_to_matrix4f(scene.tf), scene.x, scene.y, scene.z)[0]


def oracle_reference(og, scene):
    """(miss as packed bits, hit cells, hit counts): small enough to keep for every scene of a family"""
    hits = oracle_hits(og, scene)
    cells = np.flatnonzero(hits)
    return np.packbits(oracle_miss(og, scene)), cells, hits[cells]


def map_threads(fn, items, workers=8):
    """fn over items on a few threads (the oracle's calls release the GIL), results in order"""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=workers) as ex:
        return list(ex.map(fn, items))
