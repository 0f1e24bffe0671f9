"""Scenes for the tile pass (k_bin_tiles, gv_binning.hip), segment by segment: the clouds, the reference they are held
to, a model of the key layout the partition pass hands the tile pass, and mutants of the gather.  No GPU.

The clouds are built in POINT ORDER: the chunk a point lands in is chosen, not drawn, and a point that must produce no
key is NaN.  A scene is a grid, a base<-lidar transform (identity rotation, the sensor at the centre of the origin
cell, tests/ray_cases.py Geo), a lidar-frame fp32 cloud and the frame flags it runs under.

EXPECTED RESULTS come from the oracle as it stands: height_band_ref.compose gives hits, cell_idx and the per-point
(kind, ex, ey), OGrid.march_ends gives miss; the expected end bitmaps are hit end = cells with hits > 0, clip end =
cells holding a kind-2 end (an in-map clearing ground return, or the clipped end of an out-of-map point), all padding
zero.  The height band is BAND with ground_clears = 1 so that in-map clipped-end keys can be placed at will.

THE LAYOUT MODEL (Layout) is plain numpy and serves coverage proofs, failure messages and mutants only; it is never the
expected result.  From a cloud's per-point oracle result it derives the key count c(w, t) of chunk w in tile t, the
segment start w * chunk + sum of c(w, t') over t' < t, its residue r = start mod 8, whether it holds hit keys,
clipped-end keys or both, the tile totals and k = clamp(ceil(total / 32768), 1, 8).

THE CONSTANTS BELOW MIRROR csrc/gv_binning.hip AND csrc/gv_launch_frame.hpp AND MUST MOVE WITH THEM: bin_chunk_for, the
tile side (kBinTile), kBinSplitKeys, kBinSplitMax, kTileThreads (descriptors per round), kInLaneKeys, the four aligned
windows of 8 keys a lane loads first, and the tile numbering (jy >> 7) * tiles_x + (jx >> 7); clipped ends are counted
in the tile of the border cell they end on.

The mutants (MUTANTS, emulate) are errors a rewrite of the gather or of the write-out could make; tests/
test_tile_cases_host.py proves that each changes the hits or bitmaps of at least one scene.  `stale_padding_clip` is
"the words that reach into the padding -- whole padding rows and columns, and the word that holds the last valid
columns (rows) beside padding bits -- are not written and keep the previous frame's clip bits".
TEST INFRASTRUCTURE ONLY."""
import functools
from collections import namedtuple

import numpy as np

import height_band_ref as ref
import oracle_lib as ol
import ray_cases as rc

# ---- mirrors of gv_binning.hip / gv_launch_frame.hpp
TILE_LOG = 7
TILE = 1 << TILE_LOG
SPLIT_KEYS, SPLIT_MAX = 32768, 8
ROUND = 1024            # kTileThreads: segment descriptors per round
IN_LANE_KEYS = 128      # kInLaneKeys
FIRST_WINDOWS = 32      # four aligned windows of 8 keys


def bin_chunk_for(n):
    chunk = 2048
    while (n + chunk - 1) // chunk > 1536 and chunk < 8192:
        chunk *= 2
    return chunk


BAND = (0.0, 2.0, 1)
Z_HIT, Z_GROUND = 1.0, -1.0
G300 = (150, 150, 0.5)          # 300 x 300 cells, 3 x 3 tiles, the last tile 44 cells wide: T = 9, not a multiple of 8
O300 = (150, 150)
GE = (65, 241, 0.03125)         # 2080 x 7712 cells, 17 x 61 = 1037 tiles
OE = (1040, 3856)
EDGES = (0, 31, 32, 63, 64, 95, 96, 127)
HIT, GROUND = 1, 2
BLOCK = 2048                    # the unit the builders place points by (the chunk of every cloud up to 3,145,728 points)
A_SUMS = (1, 7, 8, 9, 24, 25, 31, 32, 33, 40, 64, 127, 128, 129, 136, 600)
A_KINDS = ("hit", "clip", "mixed")

Scene = namedtuple("Scene", "name grid origin tf x y z ray march")
Expected = namedtuple("Expected", "hits cell kind ex ey miss hit_bm clip_bm")   # *_bm: bool (ny_pad, nx_pad)


def pad_to_tiles(v):
    return (v + TILE - 1) // TILE * TILE


def tile_dims(geo):
    return pad_to_tiles(geo.nx) // TILE, pad_to_tiles(geo.ny) // TILE


def tile_extent(geo, t):
    """(x0, y0, valid width, valid height) of tile t"""
    tx, ty = t % tile_dims(geo)[0], t // tile_dims(geo)[0]
    return tx * TILE, ty * TILE, min(TILE, geo.nx - tx * TILE), min(TILE, geo.ny - ty * TILE)


# ------------------------------------------------------------------ clouds in point order
class Cloud:
    """n points, NaN until placed.  add(): the next free places of 2048-point block w"""

    def __init__(self, geo, n):
        self.geo, self.n = geo, n
        self.x, self.y, self.z = (np.full(n, np.nan, np.float32) for _ in range(3))
        self.cur = np.zeros((n + BLOCK - 1) // BLOCK, np.int64)

    def _take(self, w, m):
        pos = w * BLOCK + self.cur[w] + np.arange(m)
        self.cur[w] += m
        assert self.cur[w] <= min(BLOCK, self.n - w * BLOCK), (w, self.cur[w])
        return pos

    def put_cells(self, pos, ix, iy, kind):
        """in-map points at cell centres: HIT an obstacle, GROUND a clearing ground return (kind scalar or array)"""
        g = self.geo
        ix, iy = np.asarray(ix, np.float64), np.asarray(iy, np.float64)
        assert ((ix >= 0) & (ix < g.nx) & (iy >= 0) & (iy < g.ny)).all()
        self.x[pos] = (g.hix - (ix + 0.5) * g.res) - g.tx
        self.y[pos] = (g.hiy - (iy + 0.5) * g.res) - g.ty
        self.z[pos] = np.where(np.asarray(kind) == GROUND, Z_GROUND, Z_HIT)

    def put_base(self, pos, bx, by):
        """obstacle points at base-frame positions (out of the map: their rays are clipped on the border)"""
        self.x[pos], self.y[pos], self.z[pos] = np.asarray(bx) - self.geo.tx, np.asarray(by) - self.geo.ty, Z_HIT

    def add(self, w, ix, iy, kind):
        self.put_cells(self._take(w, len(ix)), ix, iy, kind)

    def scene(self, name, ray=True, march=True):
        g = self.geo
        return Scene(name, g.grid, g.origin, g.tf, self.x, self.y, self.z, ray, march)


def clip_base_point(geo, ix, iy):
    """base-frame point outside the map whose ray from the origin cell ends on border cell (ix, iy) (rc.Geo.clip_point)"""
    x, y = geo.clip_point(ix, iy)
    return x + geo.tx, y + geo.ty


def _pool(geo, t, rng):
    """candidate cells of tile t: the word edges of both axes, the last valid column and row, then random cells"""
    x0, y0, vw, vh = tile_extent(geo, t)
    ex = [e for e in EDGES if e < vw] + [vw - 1]
    ey = [e for e in EDGES if e < vh] + [vh - 1]
    edge = np.array([(x0 + a, y0 + b) for a in ex for b in ey])
    rnd = np.stack([x0 + rng.integers(0, vw, 256), y0 + rng.integers(0, vh, 256)], axis=1)
    both = np.concatenate([edge[rng.permutation(len(edge))][:48], rnd])
    return both[rng.permutation(len(both))]


def _kinds(sel, m, rng):
    if sel == "hit":
        return np.full(m, HIT)
    if sel == "clip":
        return np.full(m, GROUND)
    k = np.where(rng.random(m) < 0.35, GROUND, HIT)
    if m >= 2:
        k[0], k[-1] = HIT, GROUND   # mixed means mixed
    return k


class _Picker:
    """L cells of tile t, drawn from about 2L/3 candidates so that some repeat"""

    def __init__(self, geo, rng):
        self.geo, self.rng, self.pools, self.off = geo, rng, {}, {}

    def __call__(self, t, L):
        if t not in self.pools:
            self.pools[t], self.off[t] = _pool(self.geo, t, self.rng), 0
        p = self.pools[t]
        P = max(1, min(len(p), (2 * L + 2) // 3))
        idx = (self.off[t] + np.arange(P)) % len(p)
        self.off[t] = (self.off[t] + P) % len(p)
        c = p[idx][np.concatenate([np.arange(P), self.rng.integers(0, P, L - P)])] if L > P else p[idx][:L]
        return c[:, 0], c[:, 1]


# ------------------------------------------------------------------ family A: segments
def a_combos():
    return [(r, s) for s in A_SUMS for r in range(8) if s - r >= 1]


@functools.lru_cache(maxsize=None)
def family_a(sel):
    """one chunk per (r, r + L): r filler keys in a lower tile, then L keys in the target tile; three keys in the last
    tile behind empty segments; a chunk of 2048 keys in one tile; a ragged last chunk"""
    geo = rc.Geo(G300, O300)
    rng = np.random.default_rng(11 + A_KINDS.index(sel))
    combos = a_combos()
    n = (len(combos) + 2) * BLOCK + 777
    assert n >= SPLIT_KEYS and n % BLOCK
    c, pick = Cloud(geo, n), _Picker(geo, rng)
    for i, (r, s) in enumerate(combos):
        t = 1 + i % 8
        if r:
            c.add(i, *pick(0 if i % 2 else t - 1, r), _kinds(sel, r, rng))
        c.add(i, *pick(t, s - r), _kinds(sel, s - r, rng))
        if t < 7:
            c.add(i, *pick(8, 3), _kinds(sel, 3, rng))      # tiles t + 1 .. 7: L = 0 between two non-empty segments
    w = len(combos)
    c.add(w, *pick(5, BLOCK), _kinds(sel, BLOCK, rng))      # every key of the chunk in one tile
    c.add(w + 1, *pick(0, 40), _kinds(sel, 40, rng))        # tile 0 as a target: r = 0 by construction
    c.add(w + 1, *pick(2, 5), _kinds(sel, 5, rng))
    c.add(w + 2, *pick(3, 3), _kinds(sel, 3, rng))          # the ragged chunk: 777 points
    c.add(w + 2, *pick(8, 100), _kinds(sel, 100, rng))
    return c.scene(f"A-{sel}")


# ------------------------------------------------------------------ family B: bitmap geometry
def b_cells(geo):
    """every tile's corners and word edges on both axes, and two diagonals (rows 31 and 32 of column 30 differ)"""
    out = []
    for t in range(tile_dims(geo)[0] * tile_dims(geo)[1]):
        x0, y0, vw, vh = tile_extent(geo, t)
        out += [(x0 + a, y0 + b) for a in EDGES if a < vw for b in EDGES if b < vh]
        out += [(x0 + vw - 1, y0 + b) for b in (0, vh - 1)] + [(x0, y0 + vh - 1)]
        out += [(x0 + d, y0 + d) for d in range(min(vw, vh))] + [(x0 + d, y0 + d + 1) for d in range(min(vw, vh - 1))]
    return np.array(sorted(set(out)))


def b_outside(geo):
    """base-frame points beyond all four borders and all four corners"""
    lat_x = np.linspace(geo.lox + 3.0, geo.hix - 3.0, 15)
    lat_y = np.linspace(geo.loy + 3.0, geo.hiy - 3.0, 15)
    ox, oy = geo.tx, geo.ty
    pts = [(geo.hix + 10.0, v) for v in lat_y] + [(geo.lox - 10.0, v) for v in lat_y]
    pts += [(u, geo.hiy + 10.0) for u in lat_x] + [(u, geo.loy - 10.0) for u in lat_x]
    for cx in (geo.hix, geo.lox):
        for cy in (geo.hiy, geo.loy):
            pts += [(ox + 3.0 * (cx - ox), oy + 3.0 * (cy - oy)), (cx + np.sign(cx - ox) * 20.0, cy + np.sign(cy - oy) * 7.0)]
    for ix in (0, geo.nx - 1):
        for iy in (0, geo.ny - 1):
            pts += [clip_base_point(geo, ix, iy)]   # aimed at the outer face of the corner cell itself
    return np.array(pts)


@functools.lru_cache(maxsize=None)
def family_b(sel):
    """(frame 1, frame 2) for one handle: one end per chosen cell (sel 'hit' or 'ground') and the out-of-map points;
    then a different, sparse cloud"""
    geo = rc.Geo(G300, O300)
    cells, out = b_cells(geo), b_outside(geo)
    c = Cloud(geo, len(cells) + len(out) + 5)
    c.put_cells(np.arange(len(cells)), cells[:, 0], cells[:, 1], HIT if sel == "hit" else GROUND)
    c.put_base(len(cells) + np.arange(len(out)), out[:, 0], out[:, 1])
    sparse = np.array([(5, 7), (33, 64), (150, 140), (170, 171), (260, 290), (131, 31), (31, 131)])
    c2 = Cloud(geo, len(sparse) + 3)
    c2.put_cells(np.arange(len(sparse)), sparse[:, 0], sparse[:, 1], np.where(np.arange(len(sparse)) % 2, GROUND, HIT))
    c2.put_base(len(sparse) + np.arange(1), [geo.hix + 10.0], [geo.ty + 11.0])
    return c.scene(f"B-{sel}"), c2.scene(f"B-{sel}-sparse")


# ------------------------------------------------------------------ family C: shares
# name: (n, {tile: (hits, ground ends, out-of-map points that end on one border cell of the tile)})
C_SPECS = {
    "t32768_32769": (65537, {1: (32768, 0, 0), 5: (32769, 0, 0)}),
    "t65536_65537": (131073, {2: (65536, 0, 0), 6: (65537, 0, 0)}),
    "t262144_262145": (524289, {0: (262144, 0, 0), 8: (262145, 0, 0)}),
    "two_32769_all_helpers": (65538, {3: (32769, 0, 0), 7: (32769, 0, 0)}),
    "two_32769_spare_helpers": (65538 + 3 * 32768 + 11, {3: (32769, 0, 0), 7: (32769, 0, 0)}),
    "k2_k3_k5": (260000, {0: (40000, 0, 0), 4: (60000, 10000, 0), 8: (140000, 0, 0), 2: (500, 100, 0)}),
    "border_only": (110000, {3: (0, 0, 100000), 4: (3000, 0, 0)}),
    "hits40k_clips40k": (90001, {4: (40000, 40000, 0), 1: (10, 10, 0)}),
}
C_SEQUENCE = ("k2_k3_k5", "border_only", "hits40k_clips40k")   # three frames on one handle, then C_SPARSE


def _border_cell(geo, t):
    x0, y0, vw, vh = tile_extent(geo, t)
    for ix, iy in ((x0, y0 + vh // 2), (x0 + vw - 1, y0 + vh // 2), (x0 + vw // 2, y0), (x0 + vw // 2, y0 + vh - 1)):
        if geo.on_border(ix, iy):
            return ix, iy
    raise ValueError(t)


@functools.lru_cache(maxsize=None)
def family_c(name):
    """exact tile totals, the points of all tiles (and the NaN rest) shuffled over the cloud"""
    n, spec = C_SPECS[name]
    geo = rc.Geo(G300, O300)
    rng = np.random.default_rng(sorted(C_SPECS).index(name) + 300)
    c = Cloud(geo, n)
    pos = rng.permutation(n)
    at = 0
    for t, (nh, ng, no) in sorted(spec.items()):
        x0, y0, vw, vh = tile_extent(geo, t)
        m = nh + ng
        p = pos[at:at + m]
        c.put_cells(p, x0 + rng.integers(0, vw, m), y0 + rng.integers(0, vh, m), np.where(np.arange(m) < nh, HIT, GROUND))
        at += m
        if no:
            bx, by = clip_base_point(geo, *_border_cell(geo, t))
            c.put_base(pos[at:at + no], np.full(no, bx), np.full(no, by))
            at += no
    assert at <= n
    return c.scene(f"C-{name}")


@functools.lru_cache(maxsize=None)
def c_sparse():
    geo = rc.Geo(G300, O300)
    c = Cloud(geo, 40)
    cells = np.array([(1, 1), (140, 150), (299, 299), (128, 127), (127, 128), (290, 5)])
    c.put_cells(np.arange(6), cells[:, 0], cells[:, 1], [HIT, GROUND, HIT, HIT, GROUND, HIT])
    return c.scene("C-sparse")


# ------------------------------------------------------------------ family D: rounds and chunk size
D_SIZES = (2200000, 3145728, 3145729)
D_X, D_Y, D_SHARED = 4, 7, 1
D_LOW = (0, 1, 2, 37, 38, 39, 100, 101, 255, 256, 511, 512, 513, 700, 701, 900, 1001, 1021, 1022, 1023)
D_Y_LEN = (5, 20, 60, 120, 300)


def d_high(n):
    assert (n + BLOCK - 1) // BLOCK > 1061
    return tuple(range(1024, 1034)) + tuple(range(1041, 1061, 2))


@functools.lru_cache(maxsize=None)
def family_d(n):
    """tile D_X: segments of r + L about 600 in 20 blocks below 1024 and in 20 at or above; tile D_Y: keys in blocks at or
    above 1024 only, short, in-lane and listed; tile D_SHARED: 40,000 keys (k = 2).  At n = 3,145,729 the chunk is 4096
    points: two blocks each, and the segments lie in first halves, second halves and both."""
    geo = rc.Geo(G300, O300)
    rng = np.random.default_rng(n % 1000 + 7)
    c, pick = Cloud(geo, n), _Picker(geo, rng)
    for i, w in enumerate(D_LOW + d_high(n)):
        r = i % 8
        if r:
            c.add(w, *pick(2, r), np.full(r, HIT))
        L = 600 - r - i % 3
        c.add(w, *pick(D_X, L), _kinds("mixed", L, rng))
    for j, w in enumerate(range(1024, min(1084, (n - 1) // BLOCK))):
        if w in (1044, 1062):
            continue            # blocks 1045 and 1063 stand alone in the second half of a 4096-point chunk
        if j % 8:
            c.add(w, *pick(5, j % 8), np.full(j % 8, HIT))
        c.add(w, *pick(D_Y, D_Y_LEN[j % 5]), _kinds("mixed" if j % 2 else "hit", D_Y_LEN[j % 5], rng))
    for w in range(200, 240):
        c.add(w, *pick(D_SHARED, 1000), np.full(1000, HIT))
    if n % BLOCK:
        last = (n - 1) // BLOCK
        m = min(3, n - last * BLOCK)
        c.add(last, *pick(6, m), np.full(m, HIT))
    return c.scene(f"D-{n}", march=False)


# ------------------------------------------------------------------ family E: more than 1024 tiles
E_CROWDED = {1030: 70000, 300: 40000}


@functools.lru_cache(maxsize=None)
def family_e():
    """bin only: a hundred points in each of the first, last, middle and every 37th tile, two crowded tiles above 1024
    and below 512"""
    geo = rc.Geo(GE, OE)
    rng = np.random.default_rng(5)
    T = tile_dims(geo)[0] * tile_dims(geo)[1]
    assert T == 1037
    spec = {t: 100 for t in sorted({0, 1, T - 1, T - 2, T // 2, 511, 512, 1023, 1024, 1025} | set(range(0, T, 37)))}
    spec.update(E_CROWDED)
    n = sum(spec.values())
    c = Cloud(geo, n)
    pos, at = rng.permutation(n), 0
    for t, m in sorted(spec.items()):
        x0, y0, vw, vh = tile_extent(geo, t)
        c.put_cells(pos[at:at + m], x0 + rng.integers(0, vw, m), y0 + rng.integers(0, vh, m), HIT)
        at += m
    return c.scene("E", ray=False, march=False)


# ------------------------------------------------------------------ the reference
def expected(scene):
    """The oracle's result for one frame of `scene` on a fresh grid.  compose() is handed the finite points only, each
    distinct out-of-map point once (its ray end is found by one library call per point): a non-finite point has no cell
    and no end, and equal points have equal ends (test_tile_cases_host.py checks both on compose itself)."""
    geo = rc.Geo(scene.grid, scene.origin)
    og = ol.OGrid(*scene.grid)
    m_base = ol.tf_to_matrix4f(scene.tf)
    n = len(scene.x)
    fin = np.flatnonzero(np.isfinite(scene.x) & np.isfinite(scene.y) & np.isfinite(scene.z))
    xs, ys, zs = scene.x[fin], scene.y[fin], scene.z[fin]
    outm = og.bin_points(m_base, xs, ys, zs)[1] < 0
    rows = np.stack([xs[outm], ys[outm], zs[outm]], axis=1)
    uniq, inv = (np.unique(rows, axis=0, return_inverse=True) if len(rows) else (rows, np.zeros(0, np.int64)))
    inv = np.asarray(inv).reshape(-1)
    n_in = int((~outm).sum())
    rx, ry, rz = (np.concatenate([a[~outm], uniq[:, k]]).astype(np.float32) for k, a in enumerate((xs, ys, zs)))
    hits, cell_r, kind_r, ex_r, ey_r = ref.compose(og, m_base, rx, ry, rz, BAND)
    cell, kind = np.full(n, -1, np.int32), np.zeros(n, np.uint8)
    ex, ey = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for dst, src in ((cell, cell_r), (kind, kind_r), (ex, ex_r), (ey, ey_r)):
        dst[fin[~outm]] = src[:n_in]
        dst[fin[outm]] = src[n_in:][inv]
    miss = og.march_ends(m_base, ex, ey, kind).astype(np.int32) if scene.march else None
    nxp, nyp = pad_to_tiles(geo.nx), pad_to_tiles(geo.ny)
    hit_bm, clip_bm = np.zeros((nyp, nxp), bool), np.zeros((nyp, nxp), bool)
    hit_bm[:geo.ny, :geo.nx] = hits.reshape(geo.ny, geo.nx) > 0
    if scene.ray:
        e = kind == 2
        clip_bm[ey[e], ex[e]] = True
    return Expected(hits, cell, kind, ex, ey, miss, hit_bm, clip_bm)


# ------------------------------------------------------------------ the bitmaps' word layout (the test's decoding)
def decode_n(words, nxw, ny_pad):
    """N words -> bool (ny_pad, nx_pad): bit x & 31 of word (x >> 5) * ny_pad + y"""
    b = np.unpackbits(np.ascontiguousarray(words, "<u4").view(np.uint8).reshape(nxw, ny_pad, 4), axis=2, bitorder="little")
    return b.reshape(nxw, ny_pad, 32).transpose(1, 0, 2).reshape(ny_pad, nxw * 32).astype(bool)


def decode_t(words, nyw, nx_pad):
    """T words -> bool (ny_pad, nx_pad): bit y & 31 of word (y >> 5) * nx_pad + x"""
    b = np.unpackbits(np.ascontiguousarray(words, "<u4").view(np.uint8).reshape(nyw, nx_pad, 4), axis=2, bitorder="little")
    return b.reshape(nyw, nx_pad, 32).transpose(0, 2, 1).reshape(nyw * 32, nx_pad).astype(bool)


# ------------------------------------------------------------------ the layout model
class Layout:
    def __init__(self, scene, exp):
        geo = self.geo = rc.Geo(scene.grid, scene.origin)
        self.n = n = len(scene.x)
        self.chunk = bin_chunk_for(n)
        self.n_wg = (n + self.chunk - 1) // self.chunk
        self.tiles_x, self.tiles_y = tile_dims(geo)
        self.T = T = self.tiles_x * self.tiles_y
        self.n_helpers = n // SPLIT_KEYS
        has = (exp.kind > 0) if scene.ray else ((exp.kind == 1) & (exp.cell >= 0))
        self.pt = pt = np.flatnonzero(has)                          # the points that become keys, in point order
        self.kx, self.ky = exp.ex[pt].astype(np.int64), exp.ey[pt].astype(np.int64)
        self.clip = exp.kind[pt] == 2
        self.w = pt // self.chunk
        self.t = (self.ky >> TILE_LOG) * self.tiles_x + (self.kx >> TILE_LOG)
        self.seg = self.w * T + self.t
        shape = (self.n_wg, T)
        self.c = np.bincount(self.seg, minlength=self.n_wg * T).reshape(shape)
        self.n_clip = np.bincount(self.seg, weights=self.clip, minlength=self.n_wg * T).reshape(shape).astype(np.int64)
        self.n_hit = self.c - self.n_clip
        start = np.cumsum(self.c, axis=1) - self.c
        self.lo = np.arange(self.n_wg)[:, None] * self.chunk + start
        self.hi = self.lo + self.c
        self.r = self.lo % 8
        self.total = self.c.sum(axis=0)
        self.k_raw = np.maximum(1, -(-self.total // SPLIT_KEYS))
        self.k = np.minimum(self.k_raw, SPLIT_MAX)
        wb = self.lo & ~7
        self.listed = (self.c > 0) & (self.hi > wb + FIRST_WINDOWS) & (self.hi - wb > IN_LANE_KEYS)
        self.in_lane = (self.c > 0) & (self.hi > wb + FIRST_WINDOWS) & ~self.listed
        self.round = (np.arange(self.n_wg)[:, None] // self.k[None, :]) // ROUND     # of the share w % k that owns chunk w
        share = np.arange(self.n_wg)[:, None] % self.k[None, :]
        nshare = (self.n_wg - share + self.k[None, :] - 1) // self.k[None, :]
        self.rounds = (nshare + ROUND - 1) // ROUND

    def seg_kind(self):
        """per (w, t): 0 empty, 1 hit keys only, 2 clipped-end keys only, 3 both"""
        return (self.n_hit > 0) * 1 + (self.n_clip > 0) * 2

    def segments_of_cell(self, ix, iy):
        """(tile, chunk, r, L) of the segments that hold a key of cell (ix, iy)"""
        m = (self.kx == ix) & (self.ky == iy)
        return [(int(s % self.T), int(s // self.T), int(self.r.flat[s]), int(self.c.flat[s])) for s in np.unique(self.seg[m])]

    def describe(self, ix, iy):
        t = (iy >> TILE_LOG) * self.tiles_x + (ix >> TILE_LOG)
        segs = self.segments_of_cell(ix, iy)
        first = segs[0] if segs else (int(t), None, None, None)
        return (f"cell ({ix}, {iy}) tile {first[0]} (total {int(self.total[t])}, k {int(self.k[t])}): first segment chunk "
                f"{first[1]} (r, L) = ({first[2]}, {first[3]}); all segments (tile, chunk, r, L): {segs[:6]}")


# ------------------------------------------------------------------ mutants of the gather and of the write-out
MUTANTS = ("drop_key_at_wb32", "listed_at_128_one_short", "fast_path_on_clip_window", "no_nlong_reset",
           "k8_one_share_fewer", "k_uncapped", "t_rows_31_32_swapped", "stale_padding_clip")
Emulated = namedtuple("Emulated", "hits hitN clipN hitT clipT")   # bitmaps: bool (ny_pad, nx_pad)


def emulate(lay, mutant=None, prev=None):
    """The gather and the write-out of k_bin_tiles over the model's key stream (keys of a segment in point order), as
    numpy: every key carries the weight it adds to its cell's count and whether it sets its cell's clip bit.
    mutant None is the kernel as it is meant.  prev: the Emulated of the frame before (stale_padding_clip)."""
    assert mutant is None or mutant in MUTANTS
    geo, T = lay.geo, lay.T
    order = np.argsort(lay.seg, kind="stable")
    seg, clip, kx, ky, w = lay.seg[order], lay.clip[order], lay.kx[order], lay.ky[order], lay.w[order]
    t = seg % T
    first = np.flatnonzero(np.r_[True, seg[1:] != seg[:-1]])
    rank = np.arange(len(seg)) - np.repeat(first, np.diff(np.r_[first, len(seg)]))
    lo, hi = lay.lo.reshape(-1)[seg], lay.hi.reshape(-1)[seg]
    pos, wb = lo + rank, lo & ~7
    listed = lay.listed.reshape(-1)[seg]
    cnt, bit = (~clip).astype(np.int64), clip.copy()
    if mutant == "drop_key_at_wb32":
        d = ~listed & (pos == wb + FIRST_WINDOWS)
        cnt[d], bit[d] = 0, False
    elif mutant == "listed_at_128_one_short":
        d = (hi - wb == IN_LANE_KEYS) & (pos == hi - 1)
        cnt[d], bit[d] = 0, False
    elif mutant == "fast_path_on_clip_window":
        kw = pos & ~7
        d = clip & (kw >= lo) & (kw + 8 <= hi)       # counted as a plain increment of the cell, no clip bit
        cnt[d], bit[d] = 1, False
    elif mutant == "no_nlong_reset":
        rnd, rounds = lay.round.reshape(-1)[seg], lay.rounds.reshape(-1)[seg]
        d = listed & (pos >= wb + FIRST_WINDOWS)     # the list entry is walked again in every later round
        cnt[d] *= (rounds - rnd)[d]
    elif mutant == "k8_one_share_fewer":
        d = (lay.k[t] == SPLIT_MAX) & (w % SPLIT_MAX == SPLIT_MAX - 1)
        cnt[d], bit[d] = 0, False
    elif mutant == "k_uncapped":
        d = (lay.k_raw[t] > SPLIT_MAX) & (w % lay.k_raw[t] >= SPLIT_MAX)   # shares past the slab's eight are never summed
        cnt[d], bit[d] = 0, False
    nxp, nyp = pad_to_tiles(geo.nx), pad_to_tiles(geo.ny)
    hits = np.bincount(ky * geo.nx + kx, weights=cnt, minlength=geo.nx * geo.ny).astype(np.int32)
    hit = np.zeros((nyp, nxp), bool)
    hit[:geo.ny, :geo.nx] = hits.reshape(geo.ny, geo.nx) > 0
    cl = np.zeros((nyp, nxp), bool)
    cl[ky[bit], kx[bit]] = True
    hitT, clipT, clipN = hit, cl, cl
    if mutant == "t_rows_31_32_swapped":
        rows = np.arange(nyp)
        rows[31::TILE], rows[32::TILE] = np.arange(32, nyp, TILE), np.arange(31, nyp, TILE)
        hitT, clipT = hit[rows], cl[rows]
    elif mutant == "stale_padding_clip":
        old = prev if prev is not None else Emulated(None, None, np.zeros_like(cl), None, np.zeros_like(cl))
        keep_n, keep_t = np.zeros((nyp, nxp), bool), np.zeros((nyp, nxp), bool)
        keep_n[geo.ny:, :] = keep_n[:, geo.nx // 32 * 32:] = True
        keep_t[:, geo.nx:] = keep_t[geo.ny // 32 * 32:, :] = True
        clipN, clipT = np.where(keep_n, old.clipN, cl), np.where(keep_t, old.clipT, cl)
    return Emulated(hits, hit, clipN, hitT, clipT)


def differs(emu, exp):
    """does an emulated frame differ from the expected hits or bitmaps"""
    return (not np.array_equal(emu.hits, exp.hits) or not np.array_equal(emu.hitN, exp.hit_bm) or
            not np.array_equal(emu.hitT, exp.hit_bm) or not np.array_equal(emu.clipN, exp.clip_bm) or
            not np.array_equal(emu.clipT, exp.clip_bm))


# ------------------------------------------------------------------ everything computed once per process
@functools.lru_cache(maxsize=None)
def scene_of(key):
    """key: ('A', kind) | ('B', sel, frame) | ('C', name) | ('Csparse',) | ('D', n) | ('E',)"""
    fam = key[0]
    if fam == "A":
        return family_a(key[1])
    if fam == "B":
        return family_b(key[1])[key[2]]
    if fam == "C":
        return family_c(key[1])
    if fam == "Csparse":
        return c_sparse()
    if fam == "D":
        return family_d(key[1])
    assert fam == "E"
    return family_e()


@functools.lru_cache(maxsize=None)
def reference(key):
    """(scene, Expected, Layout), shared by every test that needs them and left unchanged"""
    s = scene_of(key)
    e = expected(s)
    return s, e, Layout(s, e)


ALL_KEYS = ([("A", k) for k in A_KINDS] + [("B", s, f) for s in ("hit", "ground") for f in (0, 1)] +
            [("C", name) for name in C_SPECS] + [("Csparse",)] + [("D", n) for n in D_SIZES] + [("E",)])
