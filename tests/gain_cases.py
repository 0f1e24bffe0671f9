"""[EXTENSION] X20 information gain: the fixtures of test_gain_host.py and test_gpu_gain.py.  A case is a packed int8
layer in data order (ny, nx) made of values a planted log-odds layer can reach (11, 50, 97, -1), a configuration, the
candidate entries, the call's flags and, with GAIN_USE_FIELD, the cells that seed the field on the device and a synthetic
field for the host tests.  Every case comes with a check that it is what its name claims (check(name, ...) below, run
against gain_ref).  The grids are X19's: 130 x 70, 200 x 80, 128 x 128 and 640 x 640."""
import functools

import numpy as np

import gain_ref as ref
from frontier_cases import FREE, GRIDS, OCC, UNKNOWN, grid_of   # noqa: F401

NAN = -1


def ent(grid, x, y):
    return y * GRIDS[grid][1][0] + x


def _case(grid, occ, entries, flags=0, seeds=None, **cfg):
    nx, ny = GRIDS[grid][1]
    occ = np.asarray(occ, np.int8)
    assert occ.shape == (ny, nx)
    c = dict(grid=grid, occ=occ, cfg=ref.config(**cfg), entries=np.asarray(entries, np.int64), flags=flags, seeds=seeds, field=None)
    if flags & ref.USE_FIELD:
        c["field"] = synthetic_field(grid, occ, seeds)
    return c


def synthetic_field(grid, occ, seeds):
    """for the host tests: 10 * the Manhattan distance to the nearest seed cell, BLOCKED on occupied and NaN cells"""
    nx, ny = GRIDS[grid][1]
    yy, xx = np.mgrid[0:ny, 0:nx]
    d = np.min([10 * (abs(xx - sx) + abs(yy - sy)) for sx, sy in seeds], axis=0).astype(np.uint32)
    d[(occ == OCC) | (occ == NAN)] = ref.NAV_BLOCKED
    return d.reshape(-1)


def _mixed(grid, seed):
    """free ground with unknown blobs, a few walls, scattered occupied and NaN cells"""
    nx, ny = GRIDS[grid][1]
    rng = np.random.default_rng(seed)
    occ = np.full((ny, nx), FREE, np.int8)
    yy, xx = np.mgrid[0:ny, 0:nx]
    for _ in range(max(6, nx * ny // 4000)):
        cx, cy, r = rng.integers(0, nx), rng.integers(0, ny), rng.integers(4, max(6, min(nx, ny) // 4))
        occ[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = UNKNOWN
    for _ in range(max(4, nx * ny // 8000)):
        x, y, n = rng.integers(0, nx), rng.integers(0, ny), rng.integers(3, max(5, min(nx, ny) // 5))
        if rng.random() < 0.5:
            occ[y, x:x + n] = OCC
        else:
            occ[y:y + n, x] = OCC
    occ[rng.random((ny, nx)) < 0.004] = OCC
    occ[rng.random((ny, nx)) < 0.001] = NAN
    return occ


def _spread(grid, seed, n, extra=()):
    nx, ny = GRIDS[grid][1]
    rng = np.random.default_rng(seed)
    return list(extra) + [ent(grid, int(rng.integers(0, nx)), int(rng.integers(0, ny))) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    g130, g200, g128, g640 = "130x70", "200x80", "128x128", "640x640"
    corners130 = [ent(g130, x, y) for x, y in ((0, 0), (129, 0), (0, 69), (129, 69))]
    borders130 = [ent(g130, x, y) for x, y in ((65, 0), (65, 69), (0, 35), (129, 35))]
    c["r1"] = _case(g130, _mixed(g130, 1), corners130 + borders130 + _spread(g130, 2, 12), radius=1)
    for R in (31, 32, 33):                                                     # window rows of 63, 65 and 67 bits
        c["r%d" % R] = _case(g200, _mixed(g200, R), [ent(g200, 0, 0), ent(g200, 199, 79), ent(g200, 100, 40), ent(g200, R, R),
                                                       ent(g200, 199 - R, 79 - R)] + _spread(g200, R, 5), radius=R)
    c["r100_taller_than_map"] = _case(g130, _mixed(g130, 100), corners130 + borders130 + [ent(g130, 65, 35)], radius=100)
    c["r128_ray_per_lane"] = _case(g640, _mixed(g640, 128), [ent(g640, 320, 320), ent(g640, 5, 630)], radius=128)   # 1024 rays
    c["r129_second_ray"] = _case(g640, _mixed(g640, 128), [ent(g640, 320, 320), ent(g640, 5, 630)], radius=129)     # 1032 rays
    c["r207_lds_64k"] = _case(g640, _mixed(g640, 207), [ent(g640, 300, 330)], radius=207)    # 64,740 B of bitmaps
    c["r208_lds_64k"] = _case(g640, _mixed(g640, 207), [ent(g640, 300, 330)], radius=208)    # 70,056 B
    c["r255"] = _case(g640, _mixed(g640, 255), [ent(g640, 0, 0), ent(g640, 255, 255), ent(g640, 384, 384), ent(g640, 639, 320)],
                      radius=255)
    unknown130 = np.full((70, 130), UNKNOWN, np.int8)
    c["open_unknown"] = _case(g130, unknown130, [ent(g130, 65, 35)], radius=10)
    c["known_answer_r2"] = _case(g130, unknown130, [ent(g130, 65, 35)], radius=2)
    # one opaque cell on each of the eight neighbours, a candidate each, 20 cells apart at R = 5
    nb = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]
    occ = np.full((80, 200), UNKNOWN, np.int8)
    for k, (dx, dy) in enumerate(nb):
        occ[40 + dy, 20 + 20 * k + dx] = OCC
    c["shadows"] = _case(g200, occ, [ent(g200, 20 + 20 * k, 40) for k in range(8)] + [ent(g200, 100, 10)], radius=5)
    occ = np.full((80, 200), UNKNOWN, np.int8)
    occ[:, :60] = FREE
    occ[:, 60] = OCC
    occ[40, 60] = FREE                                                          # the gap
    c["wall_gap"] = _case(g200, occ, [ent(g200, 50, 40), ent(g200, 50, 20)], radius=30)
    occ = np.full((70, 130), UNKNOWN, np.int8)
    occ[35, 66] = occ[36, 65] = OCC                                             # touching only diagonally, beside (65, 35)
    c["diagonal_pair"] = _case(g130, occ, [ent(g130, 65, 35)], radius=6)
    occ = np.full((70, 130), FREE, np.int8)
    occ[20, 30] = OCC
    occ[20, 90] = UNKNOWN
    c["on_opaque_and_unknown"] = _case(g130, occ, [ent(g130, 30, 20), ent(g130, 90, 20)], radius=8)
    occ = np.full((70, 130), UNKNOWN, np.int8)
    occ[35, 66] = NAN
    c["nan_is_opaque"] = _case(g130, occ, [ent(g130, 65, 35)], radius=4)
    G200 = 200 * 80
    c["bad_entries"] = _case(g200, _mixed(g200, 7), [-1, G200, 2 ** 31 - 1, ent(g200, 100, 40), -(2 ** 31), G200 - 1], radius=6)
    c["duplicates"] = _case(g200, _mixed(g200, 8), [ent(g200, 77, 33), ent(g200, 12, 70), ent(g200, 77, 33)], radius=9)
    c["n1"] = _case(g128, _mixed(g128, 9), [ent(g128, 64, 64)], radius=12)
    c["n4096_r4"] = _case(g128, _mixed(g128, 10), _spread(g128, 11, 4096 - 4, [0, 127, 127 * 128, 128 * 128 - 1]), radius=4)
    # min_gain at n_unknown - 1, n_unknown, n_unknown + 1: the open field at R = 3 has 28 unknown cells in sight
    for k, name in ((27, "min_gain_below"), (28, "min_gain_at"), (29, "min_gain_above")):
        c[name] = _case(g130, unknown130, [ent(g130, 65, 35)], radius=3, min_gain=k)
    # the weights, with the field: free ground, an unknown half, seeds on the left
    occ = np.full((80, 200), FREE, np.int8)
    occ[:, 120:] = UNKNOWN
    occ[30, 112] = OCC
    seeds = [(10, 40)]
    cands = [ent(g200, 110, 40), ent(g200, 60, 40), ent(g200, 118, 10), ent(g200, 60, 40)]
    c["w_dist_0"] = _case(g200, occ, cands, ref.USE_FIELD, seeds, radius=12, w_gain=3, w_dist=0)
    c["w_gain_0_nearest"] = _case(g200, occ, cands, ref.USE_FIELD, seeds, radius=12, w_gain=0, w_dist=5)
    c["score_tie"] = _case(g200, occ, [ent(g200, 60, 40), ent(g200, 110, 40), ent(g200, 110, 40)], ref.USE_FIELD, seeds, radius=12,
                           w_gain=100, w_dist=1)
    c["all_unranked"] = _case(g200, occ, [ent(g200, 110, 40), -5, ent(g200, 112, 30)], ref.USE_FIELD, seeds, radius=12, min_gain=1 << 20)
    c["use_field_unreachable"] = _case(g200, occ, [ent(g200, 110, 40), ent(g200, 112, 30), ent(g200, 60, 40)], ref.USE_FIELD, seeds,
                                       radius=12, w_gain=2, w_dist=1)
    c["weights_at_their_limits"] = _case(g200, occ, cands, ref.USE_FIELD, seeds, radius=12, w_gain=65535, w_dist=65535)
    return c


def seen_of(case, k=0):
    """the set of seen cells of candidate k, by the reference"""
    nx, ny = GRIDS[case["grid"]][1]
    e = int(case["entries"][k])
    return ref.cast(nx, ny, case["occ"].reshape(-1).tolist(), case["cfg"], e % nx, e // nx)[0]


def check(name, case, info, recs):
    """the fixture is what its name claims, by the reference's result (and, with the field, by ANY field's records)"""
    nx, ny = GRIDS[case["grid"]][1]
    R = case["cfg"]["radius"]
    valid = recs[(recs["status"] & ref.INVALID) == 0]
    assert ((valid["rays_opaque"] + valid["rays_off_map"] + valid["rays_range"]) == 8 * R).all()
    assert int(info["n_candidates"]) == len(recs) and int(info["radius"]) == R
    r0 = recs[0]
    if name == "r1":
        assert (valid["n_unknown"] + valid["n_free"] + valid["n_opaque"] <= 8).all() and int(recs[0]["rays_off_map"]) == 5
    elif name in ("r31", "r32", "r33"):
        assert ref.MAX_RADIUS >= R and (2 * R + 1 + 31) // 32 == {31: 2, 32: 3, 33: 3}[R]
        assert int(recs[3]["rays_off_map"]) == 0 and int(recs[4]["rays_off_map"]) == 0       # the window just fits
        assert int(r0["rays_off_map"]) >= 4 * R
    elif name == "r100_taller_than_map":
        assert 2 * R + 1 > ny and (recs["rays_off_map"] > 0).all() and len(recs) == 9
    elif name in ("r128_ray_per_lane", "r129_second_ray"):
        assert (8 * R <= 1024) == (name == "r128_ray_per_lane") and int(r0["rays_off_map"]) == 0
    elif name in ("r207_lds_64k", "r208_lds_64k"):
        lds = 3 * (2 * R + 1) * ((2 * R + 1 + 31) // 32) * 4
        assert (lds <= 65536) == (name == "r207_lds_64k") and int(r0["n_unknown"]) > 0
    elif name == "r255":
        assert len(recs) <= 4 and int(recs[1]["rays_off_map"]) == 0 and int(recs[2]["rays_off_map"]) == 0   # the window just fits
        assert int(r0["rays_off_map"]) > 0 and 3 * 511 * 16 * 4 == 98112
    elif name == "open_unknown":
        cx, cy = 65, 35
        seen = seen_of(case)
        assert int(r0["n_unknown"]) == len(seen) and int(r0["n_free"]) == int(r0["n_opaque"]) == 0 and int(r0["rays_range"]) == 8 * R
        assert {(cx + R, cy), (cx - R, cy), (cx, cy + R), (cx, cy - R)} <= seen                 # d2 = R^2 is inside
        assert not {(cx + R, cy + R), (cx - R, cy - R), (cx + R, cy - R), (cx - R, cy + R)} & seen
        assert all((x - cx) ** 2 + (y - cy) ** 2 <= R * R for x, y in seen) and int(r0["nearest_opaque_d2"]) == ref.NO_OPAQUE
    elif name == "known_answer_r2":
        # by hand: 16 rays of two cells; the four axis rays see both, the four diagonals leave the circle at (2, 2), the
        # eight knight rays see a diagonal neighbour and leave at their (2, 1)-like ends, d2 = 5 > 4
        want = {(65 + dx, 35 + dy) for dx, dy in ((1, 0), (2, 0), (-1, 0), (-2, 0), (0, 1), (0, 2), (0, -1), (0, -2), (1, 1), (1, -1),
                                                  (-1, 1), (-1, -1))}
        assert seen_of(case) == want and int(r0["n_unknown"]) == 12 and int(r0["rays_range"]) == 16
    elif name == "shadows":
        open_n = int(recs[8]["n_unknown"])
        for k, r in enumerate(recs[:8]):
            dx, dy = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)][k]
            assert int(r["n_opaque"]) == 1 and int(r["nearest_opaque_d2"]) == dx * dx + dy * dy and int(r["rays_opaque"]) >= 1
            assert int(r["n_unknown"]) < open_n - 1, k                                           # more than the cell itself is lost
        assert int(recs[8]["n_opaque"]) == 0
    elif name == "wall_gap":
        through = [p for p in seen_of(case, 0) if p[0] > 60]                                     # only the gap lets rays through
        assert (60, 40) in seen_of(case, 0) and int(recs[0]["n_unknown"]) == len(through) > 0
        assert all(abs(y - 40) <= 1 for _, y in through) and int(recs[0]["rays_opaque"]) > 0
        assert int(recs[1]["n_unknown"]) == 0 and not [p for p in seen_of(case, 1) if p[0] > 60]   # 20 rows up: the wall hides it all
    elif name == "diagonal_pair":
        seen = seen_of(case)
        assert {(66, 36), (67, 37), (66, 35), (65, 36)} <= seen                                  # the diagonal ray passes between them
        assert int(r0["n_opaque"]) == 2 and int(r0["nearest_opaque_d2"]) == 1
    elif name == "on_opaque_and_unknown":
        assert int(recs[0]["n_opaque"]) == 0 and int(recs[0]["status"]) == 0 and int(recs[0]["n_free"]) > 100
        assert int(recs[1]["n_unknown"]) == 0 and int(recs[1]["n_free"]) == int(recs[0]["n_free"])
    elif name == "nan_is_opaque":
        assert int(r0["n_opaque"]) == 1 and int(r0["nearest_opaque_d2"]) == 1 and int(r0["n_free"]) == 0
    elif name == "bad_entries":
        bad = recs[[0, 1, 2, 4]]
        zero = np.zeros(1, ref.RECORD_DTYPE)
        for r, e in zip(bad, (-1, nx * ny, 2 ** 31 - 1, -(2 ** 31))):
            zero[0]["entry"], zero[0]["status"] = e, ref.INVALID
            assert r.tobytes() == zero.tobytes()
        assert int(recs[3]["status"]) == 0 and int(recs[5]["status"]) == 0 and int(info["n_ranked"]) == 2
    elif name == "duplicates":
        assert recs[0].tobytes() == recs[2].tobytes() != recs[1].tobytes()
    elif name == "n1":
        assert len(recs) == 1 and int(info["best"]) == 0
    elif name == "n4096_r4":
        assert len(recs) == 4096 and int(info["n_ranked"]) == 4096
    elif name.startswith("min_gain_"):
        assert int(r0["n_unknown"]) == 28
        assert int(r0["status"]) == (ref.BELOW_MIN if name == "min_gain_above" else 0) and int(r0["score"]) == 28
        assert int(info["best"]) == (-1 if name == "min_gain_above" else 0)
    elif name == "w_dist_0":
        assert (recs["score"] == 3 * recs["n_unknown"].astype(np.int64)).all() and (recs["dist"] > 0).all()
        assert int(info["best"]) == int(np.argmax(recs["score"]))
    elif name == "w_gain_0_nearest":
        assert (recs["score"] == -5 * recs["dist"].astype(np.int64)).all()
        assert int(info["best"]) == int(np.argmin(recs["dist"])) == 1 and int(recs[3]["dist"]) == int(recs[1]["dist"])   # a tie: the smaller index
    elif name == "score_tie":
        assert int(recs[1]["score"]) == int(recs[2]["score"]) > int(recs[0]["score"]) and int(info["best"]) == 1
    elif name == "all_unranked":
        assert int(info["n_ranked"]) == 0 and int(info["best"]) == int(info["best_entry"]) == -1 and int(info["best_score"]) == 0
        assert (recs["status"] != 0).all()
    elif name == "use_field_unreachable":
        assert int(recs[1]["status"]) == ref.UNREACHABLE_BIT and int(recs[1]["score"]) == 0 and int(recs[1]["dist"]) >= ref.NAV_UNREACHABLE
        assert int(recs[1]["n_unknown"]) > 0 and int(recs[0]["status"]) == int(recs[2]["status"]) == 0 and int(info["n_ranked"]) == 2
    elif name == "weights_at_their_limits":
        assert (recs["score"] == 65535 * (recs["n_unknown"].astype(np.int64) - recs["dist"].astype(np.int64))).all()
    else:
        raise AssertionError(name)
