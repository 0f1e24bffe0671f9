"""[EXTENSION] X18 wide-window scan matching by branch and bound: the plain reference the tests hold
gv_match_search_host and gv_match_search to (include/gridvision_hip_search.h has the definition; oracle/ has no such
step).

The exhaustive volume over the wide window is match_ref's own (its points, cells, volume and selection, unchanged); on
top of it the header's rules one after the other, in numpy: M as the brute-force maximum over S * S shifted copies of
the zero-padded costmap, the bounds as sums of M under the points, the seed by its three rules, L from the volume, the
survivors, the counters, and the answer as the selection over the survivors' candidates and the centre.  Nothing is
shared with the library: no key packing, no separable pooling, no C.

Arrays: cost is the G bytes of the costmap in data order; the volume is uint32 (NT, NY, NX); B is uint32 (NT, NBY, NBX).
TEST INFRASTRUCTURE ONLY."""
import collections

import numpy as np

import match_ref as mref

USE_BAND = 1

STATS_DTYPE = np.dtype([("n_blocks", np.uint32), ("n_survivors", np.uint32), ("n_scored", np.uint32), ("seed_block", np.uint32),
                        ("lower_score", np.uint32), ("bound_max", np.uint32), ("bound_sum", np.uint64)])

Cfg = collections.namedtuple("Cfg", "wx wy wt yaw_step stride min_points flags block_log2", defaults=(1, 1, 0, 3))
Answer = collections.namedtuple("Answer", "record stats volume bounds survives best_block")


def match_cfg(cfg):
    """the X16 configuration with the same fields"""
    return mref.Cfg(cfg.wx, cfg.wy, cfg.wt, cfg.yaw_step, cfg.stride, cfg.min_points, cfg.flags)


def pooled(geo, cost, S):
    """M as (ny + S - 1, nx + S - 1): element [iy + S - 1, ix + S - 1] is M(ix, iy)"""
    c = np.asarray(cost, np.uint8).reshape(-1)[::-1].reshape(geo.ny, geo.nx)          # [iy, ix] in cell order
    pad = np.zeros((geo.ny + 2 * (S - 1), geo.nx + 2 * (S - 1)), np.uint8)
    pad[S - 1:S - 1 + geo.ny, S - 1:S - 1 + geo.nx] = c
    h, w = geo.ny + S - 1, geo.nx + S - 1
    m = np.zeros((h, w), np.uint8)
    for dy in range(S):
        for dx in range(S):
            m = np.maximum(m, pad[dy:dy + h, dx:dx + w])
    return m


def bounds(geo, M, cfg, guess, bx, by):
    S = 1 << cfg.block_log2
    NT, NY, NX = 2 * cfg.wt + 1, 2 * cfg.wy + 1, 2 * cfg.wx + 1
    NBY, NBX = -(-NY // S), -(-NX // S)
    rot = mref.rotations(match_cfg(cfg), guess)
    B = np.zeros((NT, NBY, NBX), np.uint32)
    ib = (-cfg.wx + S * np.arange(NBX, dtype=np.int64))[:, None]
    for t in range(NT):
        ux, uy, ok = mref.cells(geo, guess, rot[t, 0], rot[t, 1], bx, by)
        ux, uy = ux[ok], uy[ok]
        for J in range(NBY):
            ix = ux[None, :] + ib
            iy = np.broadcast_to(uy[None, :] + (-cfg.wy + S * J), ix.shape)
            on = (ix > -S) & (ix < geo.nx) & (iy > -S) & (iy < geo.ny)
            val = np.where(on, M[np.where(on, iy + S - 1, 0), np.where(on, ix + S - 1, 0)], 0)
            total = val.sum(axis=1, dtype=np.uint64)
            assert (total < 2 ** 32).all()
            B[t, J, :] = total.astype(np.uint32)
    return B


def block_window(cfg, J, I):
    """the slices of the volume's j and i axes that block (J, I) holds"""
    S = 1 << cfg.block_log2
    return slice(J * S, min(J * S + S, 2 * cfg.wy + 1)), slice(I * S, min(I * S + S, 2 * cfg.wx + 1))


def search(geo, cost, m_base, x, y, z, cfg, guess, band=None):
    """Answer of one search"""
    guess = tuple(float(v) for v in guess)
    mc = match_cfg(cfg)
    S = 1 << cfg.block_log2
    bx, by = mref.used_points(m_base, x, y, z, mc, band)
    vol = mref.volume(geo, cost, mc, guess, bx, by)
    NT, NY, NX = vol.shape
    B = bounds(geo, pooled(geo, cost, S), cfg, guess, bx, by)
    _, NBY, NBX = B.shape
    # the seed: the largest bound, then the block nearest the centre's block, then the smallest index
    t, J, I = np.meshgrid(np.arange(NT), np.arange(NBY), np.arange(NBX), indexing="ij")
    dist = np.maximum(np.abs(t - cfg.wt), np.maximum(np.abs(J - cfg.wy // S), np.abs(I - cfg.wx // S)))
    cand = B == B.max()
    cand &= dist == dist[cand].min()
    seed = int(np.flatnonzero(cand.reshape(-1))[0])
    st, sJ, sI = seed // (NBY * NBX), (seed // NBX) % NBY, seed % NBX
    sj, si = block_window(cfg, sJ, sI)
    lower = int(vol[st, sj, si].max())
    survives = (B > 0) & (B >= lower)
    # the candidates that are compared: the survivors' and the centre
    seen = np.zeros(vol.shape, bool)
    n_scored = 0
    for bt, bJ, bI in zip(*np.nonzero(survives)):
        wj, wi = block_window(cfg, bJ, bI)
        seen[bt, wj, wi] = True
        n_scored += (wj.stop - wj.start) * (wi.stop - wi.start)
    seen[cfg.wt, cfg.wy, cfg.wx] = True
    ct, cj, ci = np.meshgrid(np.arange(NT) - cfg.wt, np.arange(NY) - cfg.wy, np.arange(NX) - cfg.wx, indexing="ij")
    cheb = np.maximum(np.abs(ct), np.maximum(np.abs(cj), np.abs(ci)))
    pick = seen & (vol == vol[seen].max())
    pick &= cheb == cheb[pick].min()
    lin = int(np.flatnonzero(pick.reshape(-1))[0])
    bt, bj, bi = lin // (NY * NX) - cfg.wt, (lin // NX) % NY - cfg.wy, lin % NX - cfg.wx
    r = np.zeros(1, mref.RESULT_DTYPE)
    r["best_t"], r["best_j"], r["best_i"] = bt, bj, bi
    r["n_used"] = len(bx)
    r["best_score"] = vol[bt + cfg.wt, bj + cfg.wy, bi + cfg.wx]
    r["guess_score"] = vol[cfg.wt, cfg.wy, cfg.wx]
    r["valid"] = 1 if (len(bx) >= cfg.min_points and int(r["best_score"][0]) > 0) else 0
    r["x"] = guess[0] - float(bi) * geo.res
    r["y"] = guess[1] - float(bj) * geo.res
    r["yaw"] = mref.theta(mc, guess, bt + cfg.wt)
    s = np.zeros(1, STATS_DTYPE)
    s["n_blocks"] = B.size
    s["n_survivors"] = int(survives.sum())
    s["n_scored"] = n_scored
    s["seed_block"] = seed
    s["lower_score"] = lower
    s["bound_max"] = int(B.max())
    s["bound_sum"] = int(B.sum(dtype=np.uint64))
    best_block = ((bt + cfg.wt) * NBY + (bj + cfg.wy) // S) * NBX + (bi + cfg.wx) // S
    return Answer(r, s, vol, B, survives, int(best_block))
