"""[EXTENSION] X16 scan-to-costmap matching: the fixtures of test_match_host.py and test_gpu_match.py, family by family
(A known displacement, B ties, C borders, D windows, E selection, F counts), and the answers of match_ref for them,
computed once per process and shared.

A case is a dict: name, grid (a key of GRIDS), mask (the lethal cells, (ny, nx) bool in data order: what
planner_util.plant_grid plants), inflation (inscribed, inflation radius, scaling, threshold, occupancy_scale), tf (the
seven values of base_from_lidar), x / y / z (the lidar-frame cloud, float32), cfg (match_ref.Cfg), guess, band (None or
(z_ground, z_max)), and what the family claims about it under its own keys.
TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np

import inflate_ref
import match_ref as ref

CHUNK = 512   # kMatchChunk = GV_MATCH_CHUNK (csrc/gv_match.hpp): the points of one workgroup of the score pass

GRIDS = {"small": (5, 3, 0.1), "big": (20, 20, 0.1)}      # 50 x 30 and 200 x 200 cells
EXACT = (0.0, 0.0, 1.0, 65, False)                         # only a lethal cell itself has a cost
SOFT = (0.35, 0.55, 10.0, 65, False)
SOFT_SMALL = (0.15, 0.35, 6.0, 65, False)
SOFT_100 = (0.35, 0.55, 10.0, 65, True)                    # the 0..100 scale

TF_ROT = (0.0, 0.0, math.sin(0.15), math.cos(0.15), 0.25, -0.125, 0.5)   # a yaw of 0.3 rad and a translation
TF_FLAT = (0.0, 0.0, 0.0, 1.0, 0.25, -0.125, 0.0)                        # bz = z exactly


def geo_of(grid):
    return ref.geometry(*GRIDS[grid])


def mask_of(geo, cells):
    """cell (ix, iy) is element [ny - 1 - iy, nx - 1 - ix] of the data order"""
    m = np.zeros((geo.ny, geo.nx), bool)
    for ix, iy in cells:
        m[geo.ny - 1 - iy, geo.nx - 1 - ix] = True
    return m


def random_mask(geo, density, seed):
    return np.random.default_rng(seed).random((geo.ny, geo.nx)) < density


def cell_xy(geo, ix, iy, fx=0.5, fy=0.5):
    """grid-frame coordinates of the place (fx, fy) inside cell (ix, iy): ix grows as x falls"""
    return geo.pos_x + geo.off_x - (ix + fx) * geo.res, geo.pos_y + geo.off_y - (iy + fy) * geo.res


def to_base(pose, gx, gy):
    """base-frame coordinates of grid-frame points when the base frame sits at pose = (x, y, yaw)"""
    dx, dy = np.asarray(gx, np.float64) - pose[0], np.asarray(gy, np.float64) - pose[1]
    c, s = math.cos(pose[2]), math.sin(pose[2])
    return c * dx + s * dy, -s * dx + c * dy


def to_lidar(tf, bx, by, bz):
    """lidar-frame float32 points of base-frame points under a tf that is a yaw and a translation"""
    a = 2.0 * math.atan2(tf[2], tf[3])
    dx, dy = np.asarray(bx, np.float64) - tf[4], np.asarray(by, np.float64) - tf[5]
    c, s = math.cos(a), math.sin(a)
    z = np.broadcast_to(np.asarray(bz, np.float64) - tf[6], dx.shape)
    with np.errstate(all="ignore"):
        return (c * dx + s * dy).astype(np.float32), (-s * dx + c * dy).astype(np.float32), z.astype(np.float32)


def _case(name, grid, mask, inflation, tf, pts, cfg, guess, band=None, **claims):
    x, y, z = (np.ascontiguousarray(a, np.float32) for a in pts)
    return dict(name=name, grid=grid, mask=mask, inflation=inflation, tf=tf, x=x, y=y, z=z, cfg=cfg, guess=tuple(guess),
                band=band, **claims)


def _wall(grid):
    if grid == "big":
        return [(ix, 100) for ix in range(60, 141)] + [(60, iy) for iy in range(101, 151)]
    return [(ix, 12) for ix in range(10, 41)] + [(10, iy) for iy in range(13, 26)]


def _wall_cloud(grid, pose, tf):
    """the wall's own cell centres as the lidar sees them from `pose`"""
    geo = geo_of(grid)
    gx, gy = np.array([cell_xy(geo, ix, iy) for ix, iy in _wall(grid)]).T
    bx, by = to_base(pose, gx, gy)
    return to_lidar(tf, bx, by, 0.3)


def family_a():
    out = []
    for grid, guess in (("big", (0.7, -0.4, 0.1)), ("small", (0.2, 0.1, -0.05))):
        geo = geo_of(grid)
        # (a yaw step moves the wall's far end by more than a cell: 8 m * 0.02 and 2.4 m * 0.05)
        cfg = ref.Cfg(wx=4, wy=4, wt=3, yaw_step=0.02 if grid == "big" else 0.05)
        for i, j, t in ((3, -2, 2), (-3, -2, -2), (3, 2, -2), (-3, 2, 2)):
            pose = (guess[0] - i * geo.res, guess[1] - j * geo.res, guess[2] + t * cfg.yaw_step)
            out.append(_case(f"a_{grid}_{i:+d}{j:+d}{t:+d}", grid, mask_of(geo, _wall(grid)), EXACT, TF_ROT,
                             _wall_cloud(grid, pose, TF_ROT), cfg, guess, best=(t, j, i), n_used=len(_wall(grid))))
    return out


def family_b():
    geo = geo_of("small")
    guess = cell_xy(geo, 25, 15) + (0.2,)
    pts = to_lidar(TF_ROT, np.zeros(3), np.zeros(3), 0.3)          # three points at the base frame's origin: no yaw moves them
    mk = lambda cells: mask_of(geo, cells)                         # noqa: E731
    return [
        _case("b_zero", "small", mk([]), SOFT_SMALL, TF_ROT, pts, ref.Cfg(3, 2, 2, 0.05), guess, best=(0, 0, 0), valid=0),
        _case("b_uniform", "small", np.ones((geo.ny, geo.nx), bool), EXACT, TF_ROT, pts, ref.Cfg(3, 2, 2, 0.05), guess,
              best=(0, 0, 0), valid=1, flat=3 * 254),
        _case("b_mirror_i", "small", mk([(27, 15), (23, 15)]), EXACT, TF_ROT, pts, ref.Cfg(3, 3, 0, 0.0), guess, best=(0, 0, -2), valid=1),
        _case("b_mirror_j", "small", mk([(25, 17), (25, 13)]), EXACT, TF_ROT, pts, ref.Cfg(3, 3, 0, 0.0), guess, best=(0, -2, 0), valid=1),
        _case("b_mirror_t", "small", mk([(27, 15)]), EXACT, TF_ROT, pts, ref.Cfg(3, 3, 2, 0.05), guess, best=(-2, 0, 2), valid=1),
        _case("b_nearer", "small", mk([(26, 15), (22, 15)]), EXACT, TF_ROT, pts, ref.Cfg(3, 3, 0, 0.0), guess, best=(0, 0, 1), valid=1),
    ]


C_EDGE_CELLS = [(0, 0), (49, 0), (0, 29), (49, 29), (25, 0), (25, 29), (0, 15), (49, 15)]
C_OFF_CELLS = [(-2, 10), (51, 10), (10, -3), (10, 32), (-2, -2), (51, 31)]


def family_c():
    geo = geo_of("small")
    gx, gy = np.array([cell_xy(geo, ix, iy) for ix, iy in C_EDGE_CELLS + C_OFF_CELLS]).T
    big, nan, inf = 1e30, float("nan"), float("inf")
    # far points, points that are not finite, and points exactly on a cell border and on the map's two ends
    more = [(big, 0.0), (0.0, -big), (3e38, -3e38), (nan, 0.0), (0.0, inf), (-inf, 0.0),
            (2.5, 0.0), (3.5, 0.0), (-1.5, 0.0), (1.0, 1.5), (1.0, -1.5), (2.5, 0.5)]
    gx = np.concatenate([gx, [p[0] for p in more]])
    gy = np.concatenate([gy, [p[1] for p in more]])
    pts = to_lidar(TF_FLAT, gx, gy, 0.3)
    return [_case("c_borders", "small", random_mask(geo, 0.08, 5), SOFT_SMALL, TF_FLAT, pts, ref.Cfg(3, 3, 1, 0.01), (0.0, 0.0, 0.0),
                  n_used=len(gx) - 3, n_far=3)]


def _scatter(n, seed, x=(-3.0, 15.0), y=(-9.0, 9.0), z=(-1.0, 3.0), tf=TF_ROT):
    r = np.random.default_rng(seed)
    return to_lidar(tf, r.uniform(*x, n), r.uniform(*y, n), r.uniform(*z, n))


def family_d():
    geo = geo_of("big")
    wall, pose = mask_of(geo, _wall("big")), (0.7, -0.4, 0.1)
    return [
        _case("d_single", "big", wall, EXACT, TF_ROT, _wall_cloud("big", pose, TF_ROT), ref.Cfg(0, 0, 0, 0.0), pose,
              best=(0, 0, 0), full=len(_wall("big")) * 254),
        _case("d_rect", "big", wall, SOFT, TF_ROT, _wall_cloud("big", pose, TF_ROT), ref.Cfg(5, 2, 1, 0.02), pose, best=(0, 0, 0)),
        _case("d_full", "big", random_mask(geo, 0.02, 9), SOFT, TF_ROT, _scatter(300, 21), ref.Cfg(32, 32, 32, 0.01), (0.3, 0.2, 0.05)),
        _case("d_tiny_step", "big", random_mask(geo, 0.02, 9), SOFT, TF_ROT, _scatter(300, 22), ref.Cfg(2, 2, 2, 1e-12), (0.3, 0.2, 0.05),
              same_yaws=True),
    ]


BAND = (0.25, 1.75)


def family_e():
    geo = geo_of("big")
    mask = random_mask(geo, 0.03, 13)
    x, y, z = _scatter(2500, 31, tf=TF_FLAT)
    zg, zm = np.float32(BAND[0]), np.float32(BAND[1])
    lo, hi = np.float32(-np.inf), np.float32(np.inf)
    edge = np.array([zg, np.nextafter(zg, lo), np.nextafter(zg, hi), zm, np.nextafter(zm, lo), np.nextafter(zm, hi)], np.float32)
    zb = z.copy()
    zb[:6] = edge          # TF_FLAT: bz is z
    out = [_case(f"e_stride_{s}", "big", mask, SOFT, TF_FLAT, (x, y, z), ref.Cfg(3, 3, 1, 0.02, stride=s), (0.1, -0.2, 0.02),
                 n_used=len(range(0, 2500, s))) for s in (1, 3, 1024)]
    out.append(_case("e_band_off", "big", mask, SOFT, TF_FLAT, (x, y, zb), ref.Cfg(3, 3, 1, 0.02), (0.1, -0.2, 0.02), band=BAND, n_used=2500))
    out.append(_case("e_band_on", "big", mask, SOFT, TF_FLAT, (x, y, zb), ref.Cfg(3, 3, 1, 0.02, flags=ref.USE_BAND), (0.1, -0.2, 0.02),
                     band=BAND, edge_used=[True, False, True, True, True, False]))
    out.append(_case("e_band_unset", "big", mask, SOFT, TF_FLAT, (x, y, zb), ref.Cfg(3, 3, 1, 0.02, flags=ref.USE_BAND), (0.1, -0.2, 0.02),
                     n_used=2500))
    return out


def family_f():
    geo = geo_of("big")
    wall = mask_of(geo, _wall("big"))
    guess = (0.7, -0.4, 0.1)
    out = []
    for n in (0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1):
        x, y, z = _scatter(n if n else 4, 40 + n, x=(2.0, 11.0), y=(-6.0, 1.0))
        if n == 0:
            x = np.full(4, np.nan, np.float32)   # four selected points, none used
        out.append(_case(f"f_n{n}", "big", wall, SOFT, TF_ROT, (x, y, z), ref.Cfg(2, 2, 1, 0.02), guess, n_used=n))
    x, y, z = _scatter(64, 104, x=(2.0, 11.0), y=(-6.0, 1.0))
    out.append(_case("f_min_points_eq", "big", wall, SOFT, TF_ROT, (x, y, z), ref.Cfg(2, 2, 1, 0.02, min_points=64), guess, n_used=64, valid=1))
    out.append(_case("f_min_points_above", "big", wall, SOFT, TF_ROT, (x, y, z), ref.Cfg(2, 2, 1, 0.02, min_points=65), guess, n_used=64, valid=0))
    # 10 000 points inside one cell beside the wall's corner, the base frame at the guess
    r = np.random.default_rng(77)
    cx, cy = cell_xy(geo, 62, 102)
    bx, by = to_base(guess, cx + r.uniform(-0.04, 0.04, 10000), cy + r.uniform(-0.04, 0.04, 10000))
    out.append(_case("f_one_cell", "big", wall, SOFT, TF_ROT, to_lidar(TF_ROT, bx, by, 0.3), ref.Cfg(2, 2, 1, 0.02), guess, n_used=10000,
                     one_cell=(62, 102)))
    return out


_CASES = None
_COST = {}
_WANT = {}


def cases():
    global _CASES
    if _CASES is None:
        _CASES = family_a() + family_b() + family_c() + family_d() + family_e() + family_f()
        assert len({c["name"] for c in _CASES}) == len(_CASES)
    return _CASES


def names():
    return [c["name"] for c in cases()]


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


def inflate_cfg(inflation):
    ins, infl, scaling, thr, occ = inflation
    return inflate_ref.Cfg(ins, infl, scaling, thr, inflate_ref.OCCUPANCY_SCALE if occ else 0)


def cost_of(mask, inflation, res):
    """the costmap gv_inflate makes of the planted mask (inflate_ref), G bytes in data order"""
    key = (mask.tobytes(), mask.shape, inflation, res)
    if key not in _COST:
        table = inflate_ref.cost_table(inflate_cfg(inflation), res)
        d2 = inflate_ref.dist2(mask, len(table) - 1)
        has = d2 != inflate_ref.NONE
        _COST[key] = np.where(has, table[np.where(has, d2, 0)], 0).astype(np.uint8).reshape(-1)
    return _COST[key]


def m_base(tf):
    import oracle_lib as ol
    return ol.tf_to_matrix4f(tf)


def want(case, cost=None):
    """(record, volume) of match_ref for the case; with the fixture's own costmap the answer is computed once"""
    geo = geo_of(case["grid"])
    if cost is not None:
        return ref.scan(geo, cost, m_base(case["tf"]), case["x"], case["y"], case["z"], case["cfg"], case["guess"], case["band"])
    if case["name"] not in _WANT:
        c = cost_of(case["mask"], case["inflation"], geo.res)
        _WANT[case["name"]] = ref.scan(geo, c, m_base(case["tf"]), case["x"], case["y"], case["z"], case["cfg"], case["guess"], case["band"])
    return _WANT[case["name"]]
