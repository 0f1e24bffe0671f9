"""[EXTENSION] X4 height band: the reference the tests hold the library to, composed from the CPU oracle as it stands
(oracle/ has no band of its own).  include/gridvision_hip.h, gv_height_band:

  z_ground <= bz <= z_max            obstacle: a hit in map, the oracle's ray end (hit end / clipped end)
  bz < z_ground, ground_clears = 1   no hit; in map: an end at its own cell, own cell included (kind 2); out of map:
                                     the clipped end on the border (kind 2, as the oracle gives it)
  bz < z_ground, ground_clears = 0   nothing
  bz > z_max                         nothing

bz is the fp32 base-frame z of the oracle's transform (gvo_transform_cloud), compared in numpy float32.
TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

import oracle_lib as ol


def classify(m_base, x, y, z, band):
    """(obstacle, clearing ground) masks; band None = off (every point an obstacle)"""
    n = len(x)
    if band is None:
        return np.ones(n, bool), np.zeros(n, bool)
    zg, zm, clears = np.float32(band[0]), np.float32(band[1]), int(band[2])
    bz = ol.transform_cloud(m_base, x, y, z)[2]
    obs = ~(bz < zg) & ~(bz > zm)
    gnd = (bz < zg) & bool(clears)
    return obs, gnd


def compose(og, m_base, x, y, z, band):
    """hits, cell_idx and the per-point ray ends (kind, ex, ey) of one frame under the band"""
    x, y, z = ol.f32(x), ol.f32(y), ol.f32(z)
    obs, gnd = classify(m_base, x, y, z, band)
    hits, _ = og.bin_points(m_base, x[obs], y[obs], z[obs])
    _, cell = og.bin_points(m_base, x, y, z)
    n = len(x)
    kind = np.zeros(n, np.uint8)
    ex, ey = np.zeros(n, np.int32), np.zeros(n, np.int32)
    m = ol.f32(m_base).reshape(16)
    if not og.get_index(float(m[3]), float(m[7]))[0]:
        return hits, cell, kind, ex, ey   # origin outside the map: no rays this frame
    inmap = cell >= 0
    ex[inmap], ey[inmap] = cell[inmap] % og.nx, cell[inmap] // og.nx
    kind[inmap & obs] = 1
    kind[inmap & gnd] = 2
    out = np.nonzero(~inmap & (obs | gnd))[0]
    if len(out):
        k, oxe, oye = og.ray_ends(m_base, x[out], y[out], z[out])
        kind[out], ex[out], ey[out] = k, oxe, oye
    return hits, cell, kind, ex, ey


def frame(og, m_base, x, y, z, band, poses=None, raymarch=True):
    """one frame of the oracle grid under the band: returns hits, cell_idx, miss (uint8 or None)"""
    hits, cell, kind, ex, ey = compose(og, m_base, x, y, z, band)
    miss = og.march_ends(m_base, ex, ey, kind) if raymarch else None
    og.frame_update(poses, hits, miss)
    return hits, cell, miss
