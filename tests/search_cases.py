"""[EXTENSION] X18 wide-window scan matching by branch and bound: the fixtures of test_search_host.py and
test_gpu_search.py and the answers of search_ref for them, computed once per process and shared.

A case is match_cases' dict (name, grid, mask, inflation, tf, x / y / z, cfg, guess, band) with cfg a search_ref.Cfg, and
what the case claims about itself under its own keys.  The groups:
  w_*      every block size S against the window widths at which the block geometry changes: one candidate, a window
           narrower than a block, a last block one candidate wide (NX % S == 1) and S - 1 wide, the centre on a block's
           first row (wy % S == 0), and the 257 x 257 window on the 200 x 200 map
  border_* points in cells 0 and nx - 1 and up to S cells off the map on every side, far and non-finite points
  n_*      n_used around the wavefront and the chunk
  band_*   the band flag
  tie, loose_seed, pruning, zero, flat: the cases the header's rules are about
TEST INFRASTRUCTURE ONLY."""
import numpy as np

import match_cases as mc
import search_ref as ref

CHUNK = mc.CHUNK
GRIDS = mc.GRIDS
SIZES = (1, 2, 3, 4)   # block_log2


def _case(name, grid, mask, inflation, tf, pts, cfg, guess, band=None, **claims):
    return mc._case(name, grid, mask, inflation, tf, pts, cfg, guess, band, **claims)


def _wall_case(name, cfg, shift, inflation=mc.SOFT, **claims):
    """the big wall seen from a pose `shift` = (t, j, i) candidates away from the guess"""
    geo, guess = mc.geo_of("big"), (0.7, -0.4, 0.1)
    t, j, i = shift
    pose = (guess[0] - i * geo.res, guess[1] - j * geo.res, guess[2] + t * cfg.yaw_step)
    return _case(name, "big", mc.mask_of(geo, mc._wall("big")), inflation, mc.TF_ROT, mc._wall_cloud("big", pose, mc.TF_ROT), cfg, guess,
                 **claims)


def windows():
    out = []
    for lg in SIZES:
        S = 1 << lg
        out.append(_wall_case(f"w_s{S}_one", ref.Cfg(0, 0, 1, 0.02, block_log2=lg), (1, 0, 0), edge="one"))
        out.append(_wall_case(f"w_s{S}_narrow", ref.Cfg(S // 2, S, 0, 0.0, block_log2=lg), (0, 1, -(S // 2)), edge="narrow"))
        out.append(_wall_case(f"w_s{S}_rem1", ref.Cfg(S, S // 2 - 1 + S, 1, 0.02, block_log2=lg), (-1, -(S // 2), S), edge="rem1"))
        out.append(_wall_case(f"w_s{S}_remS1", ref.Cfg(S // 2 - 1 + S, S, 1, 0.02, block_log2=lg), (1, S, 1 - S), edge="remS1"))
        out.append(_wall_case(f"w_s{S}_wide", ref.Cfg(128, 128, 1 if lg == 3 else 0, 0.02, block_log2=lg), (0, 37 + lg, -(90 + lg)),
                              edge="wide"))
    return out


def borders():
    geo = mc.geo_of("small")
    out = []
    for lg in SIZES:
        S = 1 << lg
        off = []
        for k in sorted({1, S - 1, S}):
            off += [(-k, 10), (geo.nx - 1 + k, 10), (10, -k), (10, geo.ny - 1 + k), (-k, -k), (geo.nx - 1 + k, geo.ny - 1 + k)]
        cells = mc.C_EDGE_CELLS + off
        gx, gy = np.array([mc.cell_xy(geo, ix, iy) for ix, iy in cells]).T
        big, nan, inf = 1e30, float("nan"), float("inf")
        more = [(big, 0.0), (0.0, -big), (3e38, -3e38), (nan, 0.0), (0.0, inf), (-inf, 0.0)]
        gx = np.concatenate([gx, [p[0] for p in more]])
        gy = np.concatenate([gy, [p[1] for p in more]])
        mask = mc.random_mask(geo, 0.08, 5 + lg)
        mask[0, 0] = mask[0, -1] = mask[-1, 0] = mask[-1, -1] = True     # the map's corners: M's aprons are not empty
        out.append(_case(f"border_s{S}", "small", mask, mc.SOFT_SMALL, mc.TF_FLAT, mc.to_lidar(mc.TF_FLAT, gx, gy, 0.3),
                         ref.Cfg(5, 4, 1, 0.03, block_log2=lg), (0.0, 0.0, 0.0), cells=cells, n_used=len(gx) - 3, n_far=3))
    return out


def counts():
    geo = mc.geo_of("big")
    wall, guess = mc.mask_of(geo, mc._wall("big")), (0.7, -0.4, 0.1)
    out = []
    for n in (0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1):
        x, y, z = mc._scatter(n if n else 4, 140 + n, x=(2.0, 11.0), y=(-6.0, 1.0))
        if n == 0:
            x = np.full(4, np.nan, np.float32)
        out.append(_case(f"n_{n}", "big", wall, mc.SOFT, mc.TF_ROT, (x, y, z), ref.Cfg(6, 5, 1, 0.02, block_log2=2), guess, n_used=n))
    return out


def bands():
    geo = mc.geo_of("big")
    mask = mc.random_mask(geo, 0.03, 13)
    x, y, z = mc._scatter(900, 31, tf=mc.TF_FLAT)
    z[:6] = [0.25, 0.2, 0.3, 1.75, 1.7, 1.8]
    on = ref.Cfg(9, 7, 1, 0.02, flags=ref.USE_BAND, block_log2=3)
    off = on._replace(flags=0)
    g = (0.1, -0.2, 0.02)
    return [_case("band_on", "big", mask, mc.SOFT, mc.TF_FLAT, (x, y, z), on, g, band=mc.BAND),
            _case("band_off", "big", mask, mc.SOFT, mc.TF_FLAT, (x, y, z), off, g, band=mc.BAND, n_used=900),
            _case("band_stride", "big", mask, mc.SOFT, mc.TF_FLAT, (x, y, z), off._replace(stride=7, min_points=129), g, n_used=129,
                  valid=1)]


def _origin_points():
    """three points at the base frame's origin: no yaw moves them"""
    return mc.to_lidar(mc.TF_ROT, np.zeros(3), np.zeros(3), 0.3)


def tie():
    """S = 4, wx = wy = 8: the centre's block holds i = 0..3.  Lethal cells under i = +2 (the centre's block: the seed,
    nearest the centre among the equal bounds) and i = -1 (the block before it, whose bound equals L): the nearer one wins
    only if that block survives"""
    geo = mc.geo_of("small")
    guess = mc.cell_xy(geo, 25, 15) + (0.2,)
    return [_case("tie", "small", mc.mask_of(geo, [(27, 15), (24, 15)]), mc.EXACT, mc.TF_ROT, _origin_points(),
                  ref.Cfg(8, 8, 0, 0.0, block_log2=2), guess, best=(0, 0, -1))]


def degenerate():
    geo = mc.geo_of("small")
    guess = mc.cell_xy(geo, 25, 15) + (0.2,)
    return [_case("zero", "small", mc.mask_of(geo, []), mc.SOFT_SMALL, mc.TF_ROT, _origin_points(), ref.Cfg(9, 6, 2, 0.05, block_log2=2),
                  guess, best=(0, 0, 0), valid=0),
            _case("flat", "small", np.ones((geo.ny, geo.nx), bool), mc.EXACT, mc.TF_ROT, _origin_points(),
                  ref.Cfg(5, 5, 1, 0.05, block_log2=1), guess, best=(0, 0, 0), valid=1)]


def _loose(seed):
    geo = mc.geo_of("small")
    pts = mc._scatter(60, 300 + seed, x=(-1.0, 3.0), y=(-1.2, 1.2), tf=mc.TF_FLAT)
    return _case("loose_seed", "small", mc.random_mask(geo, 0.06, 200 + seed), mc.EXACT, mc.TF_FLAT, pts,
                 ref.Cfg(12, 10, 0, 0.0, block_log2=3), (0.05, -0.03, 0.1), seed=seed)


def loose_seed():
    """a sparse random field: the first seed of the generator at which the largest bound does not hold the optimum"""
    for seed in range(40):
        c = _loose(seed)
        a = _answer(c)
        if a.best_block != int(a.stats["seed_block"][0]) and int(a.bounds.reshape(-1)[a.best_block]) < int(a.stats["bound_max"][0]):
            return [c]
    raise AssertionError("no seed gives a loose bound")


PRUNE_CELLS = [(31, 47), (58, 139), (83, 61), (102, 118), (117, 33), (141, 97), (163, 152), (66, 88), (129, 171), (45, 104), (151, 58),
               (94, 160)]
PRUNE_SHIFT = (1, -43, 57)


def pruning():
    geo, guess = mc.geo_of("big"), (0.7, -0.4, 0.1)
    cfg = ref.Cfg(128, 128, 1, 0.01, block_log2=3)
    t, j, i = PRUNE_SHIFT
    pose = (guess[0] - i * geo.res, guess[1] - j * geo.res, guess[2] + t * cfg.yaw_step)
    gx, gy = np.array([mc.cell_xy(geo, ix, iy) for ix, iy in PRUNE_CELLS]).T
    bx, by = mc.to_base(pose, gx, gy)
    return [_case("pruning", "big", mc.mask_of(geo, PRUNE_CELLS), mc.EXACT, mc.TF_ROT, mc.to_lidar(mc.TF_ROT, bx, by, 0.3), cfg, guess,
                  best=PRUNE_SHIFT)]


_CASES = None
_WANT = {}


def cases():
    global _CASES
    if _CASES is None:
        _CASES = windows() + borders() + counts() + bands() + tie() + degenerate() + loose_seed() + pruning()
        assert len({c["name"] for c in _CASES}) == len(_CASES)
    return _CASES


def names():
    return [c["name"] for c in cases()]


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


def _answer(case, cost=None):
    geo = mc.geo_of(case["grid"])
    c = mc.cost_of(case["mask"], case["inflation"], geo.res) if cost is None else cost
    return ref.search(geo, c, mc.m_base(case["tf"]), case["x"], case["y"], case["z"], case["cfg"], case["guess"], case["band"])


def want(case, cost=None):
    """search_ref's Answer for the case; with the fixture's own costmap it is computed once"""
    if cost is not None:
        return _answer(case, cost)
    if case["name"] not in _WANT:
        _WANT[case["name"]] = _answer(case)
    return _WANT[case["name"]]
