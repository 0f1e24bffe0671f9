"""[EXTENSION] X16 scan-to-costmap matching: the plain reference the tests hold gv_match_scan_host and gv_match_scan to
(include/gridvision_hip_match.h has the definition; oracle/ has no such step).

float32 operations one at a time (numpy float32 arrays: every product and sum is rounded on its own) for the transform
and the rotation, Python / numpy float64 for the rest, math.cos / math.sin for the table, a loop over the yaw
candidates and the window's rows with the row's candidates as an array axis, the selection by its three rules one
after the other.  No histogram, no key packing, no C: only the fp32 matrix of base_from_lidar is the oracle's
(oracle_lib.tf_to_matrix4f), as in every other reference here.

Arrays: cost is the G bytes of the costmap in data order; a volume is uint32 (NT, NY, NX).
TEST INFRASTRUCTURE ONLY."""
import collections
import math

import numpy as np

USE_BAND = 1
KEEP_SCORES = 1
CELL_LIMIT = float(2 ** 30)

RESULT_DTYPE = np.dtype([("best_t", np.int32), ("best_j", np.int32), ("best_i", np.int32), ("valid", np.int32),
                         ("n_used", np.uint32), ("best_score", np.uint32), ("guess_score", np.uint32),
                         ("reserved", np.uint32), ("x", np.float64), ("y", np.float64), ("yaw", np.float64),
                         ("reserved2", np.uint64)])

Cfg = collections.namedtuple("Cfg", "wx wy wt yaw_step stride min_points flags", defaults=(1, 1, 0))
Geo = collections.namedtuple("Geo", "nx ny G res off_x off_y pos_x pos_y")


def geometry(grid_x, grid_y, res):
    """the geometry gv_create gives (grid_map setGeometry + setPosition as the reference's constructor calls them)"""
    nx, ny = int(round(grid_x / res)), int(round(grid_y / res))
    return Geo(nx, ny, nx * ny, float(res), 0.5 * (nx * res), 0.5 * (ny * res), float(grid_x // 3), 0.0)


def base_points(m, x, y, z):
    """x*c0 + (y*c1 + (z*c2 + c3)) in float32, one rounding an operation"""
    m = np.asarray(m, np.float32).reshape(-1)
    x, y, z = (np.asarray(a, np.float32) for a in (x, y, z))
    with np.errstate(all="ignore"):
        out = [x * m[4 * r] + (y * m[4 * r + 1] + (z * m[4 * r + 2] + m[4 * r + 3])) for r in range(3)]
    assert all(o.dtype == np.float32 for o in out)
    return out


def used_points(m, x, y, z, cfg, band):
    """(bx, by) of the used points in index order"""
    sel = slice(0, None, cfg.stride)
    bx, by, bz = base_points(m, np.asarray(x, np.float32)[sel], np.asarray(y, np.float32)[sel], np.asarray(z, np.float32)[sel])
    used = np.isfinite(bx) & np.isfinite(by) & np.isfinite(bz)
    if (cfg.flags & USE_BAND) and band is not None:
        zg, zm = np.float32(band[0]), np.float32(band[1])
        used &= ~(bz < zg) & ~(bz > zm)
    return bx[used], by[used]


def theta(cfg, guess, t):
    return guess[2] + float(t - cfg.wt) * cfg.yaw_step


def rotations(cfg, guess):
    """float32 (NT, 2): (cos, sin) of every yaw candidate, libm in fp64 rounded once"""
    return np.array([[np.float32(math.cos(theta(cfg, guess, t))), np.float32(math.sin(theta(cfg, guess, t)))]
                     for t in range(2 * cfg.wt + 1)], np.float32).reshape(-1, 2)


def cells(geo, guess, c, s, bx, by):
    """(ux, uy, ok): the cells as int64, ok False where a point contributes to no candidate"""
    c, s = np.float32(c), np.float32(s)
    with np.errstate(all="ignore"):
        rx = (c * bx) - (s * by)
        ry = (s * bx) + (c * by)
        assert rx.dtype == np.float32 and ry.dtype == np.float32
        gx = rx.astype(np.float64) + guess[0]
        gy = ry.astype(np.float64) + guess[1]
        fx = np.floor(-(((gx - geo.off_x) - geo.pos_x) / geo.res))
        fy = np.floor(-(((gy - geo.off_y) - geo.pos_y) / geo.res))
        ok = (np.abs(fx) < CELL_LIMIT) & (np.abs(fy) < CELL_LIMIT)
    ux = np.where(ok, fx, 0.0).astype(np.int64)
    uy = np.where(ok, fy, 0.0).astype(np.int64)
    return ux, uy, ok


def volume(geo, cost, cfg, guess, bx, by):
    cost = np.asarray(cost, np.uint8).reshape(-1)
    assert cost.size == geo.G
    rot = rotations(cfg, guess)
    NT, NY, NX = 2 * cfg.wt + 1, 2 * cfg.wy + 1, 2 * cfg.wx + 1
    vol = np.zeros((NT, NY, NX), np.uint32)
    shift = np.arange(-cfg.wx, cfg.wx + 1, dtype=np.int64)[:, None]
    for t in range(NT):
        ux, uy, ok = cells(geo, guess, rot[t, 0], rot[t, 1], bx, by)
        ux, uy = ux[ok], uy[ok]
        for j in range(-cfg.wy, cfg.wy + 1):
            ix = ux[None, :] + shift
            iy = np.broadcast_to(uy[None, :] + j, ix.shape)
            on = (ix >= 0) & (ix < geo.nx) & (iy >= 0) & (iy < geo.ny)
            entry = np.where(on, geo.G - 1 - (iy * geo.nx + ix), 0)
            total = np.where(on, cost[entry], 0).sum(axis=1, dtype=np.uint64)
            assert (total < 2 ** 32).all()
            vol[t, j + cfg.wy, :] = total.astype(np.uint32)
    return vol


def select(vol, cfg):
    """(t, j, i) offsets of the best candidate: the largest score, then the smallest Chebyshev distance, then the
    smallest linear index"""
    NT, NY, NX = vol.shape
    t, j, i = np.meshgrid(np.arange(NT) - cfg.wt, np.arange(NY) - cfg.wy, np.arange(NX) - cfg.wx, indexing="ij")
    cheb = np.maximum(np.abs(t), np.maximum(np.abs(j), np.abs(i)))
    cand = vol == vol.max()
    cand &= cheb == cheb[cand].min()
    lin = int(np.flatnonzero(cand.reshape(-1))[0])
    return lin // (NY * NX) - cfg.wt, (lin // NX) % NY - cfg.wy, lin % NX - cfg.wx


def scan(geo, cost, m_base, x, y, z, cfg, guess, band=None):
    """(record RESULT_DTYPE[1], volume) of one match"""
    guess = tuple(float(v) for v in guess)
    bx, by = used_points(m_base, x, y, z, cfg, band)
    vol = volume(geo, cost, cfg, guess, bx, by)
    bt, bj, bi = select(vol, cfg)
    r = np.zeros(1, RESULT_DTYPE)
    r["best_t"], r["best_j"], r["best_i"] = bt, bj, bi
    r["n_used"] = len(bx)
    r["best_score"] = vol[bt + cfg.wt, bj + cfg.wy, bi + cfg.wx]
    r["guess_score"] = vol[cfg.wt, cfg.wy, cfg.wx]
    r["valid"] = 1 if (len(bx) >= cfg.min_points and int(r["best_score"][0]) > 0) else 0
    r["x"] = guess[0] - float(bi) * geo.res
    r["y"] = guess[1] - float(bj) * geo.res
    r["yaw"] = theta(cfg, guess, bt + cfg.wt)
    return r, vol


def motion(rec):
    """(qx, qy, qz, qw, tx, ty, tz) of a record's pose"""
    yaw = float(rec["yaw"])
    return (0.0, 0.0, math.sin(yaw / 2.0), math.cos(yaw / 2.0), float(rec["x"]), float(rec["y"]), 0.0)
