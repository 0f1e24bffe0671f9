"""References of gv_grid_move (X3, gv_gridmove.hip) for tests/test_gpu_grid_move.py and tests/test_grid_move_cases_host.py.

np_move       the definition: fp64 centres and sources in include/gridvision_hip.h's operation order, grid_map getIndex
              with its exact division, the constructor state (0.0, 0.5, 50) off the map.
slice_move    a second opinion for whole-cell translations: shifted slices of the old layers, no coordinates.
emulate       the device side as gv_gridmove.hip and get_index_fast (gv_device.hpp) are written -- lanes, block guards,
              packed dwords, scratch layout, copy body and tail -- with the MUTANTS below switched in by name.

A state is (log_odds f32[G], occupancy f32[G], int8[G]): the float layers in cell order c = iy * nx + ix, the int8 in
OccupancyGrid.data order (byte G - 1 - c).  Everything is compared by bytes; nothing here touches a GPU."""
import numpy as np

LAYERS = ("log_odds", "occupancy", "int8")


def np_sources(nx, ny, res, pos_x, pos_y, info):
    """per destination cell, in cell order: the source cell jy * nx + jx (-1 off the map) and the source point (sx, sy)"""
    len_x, len_y = nx * res, ny * res
    off_x, off_y = 0.5 * len_x, 0.5 * len_y
    c, s, tx, ty = info["cos_yaw"], info["sin_yaw"], info["tx"], info["ty"]
    cx = (pos_x + off_x) - (np.arange(nx, dtype=np.float64) + 0.5) * res
    cy = (pos_y + off_y) - (np.arange(ny, dtype=np.float64) + 0.5) * res
    CX, CY = np.broadcast_to(cx[None, :], (ny, nx)), np.broadcast_to(cy[:, None], (ny, nx))
    sx = (c * CX - s * CY) + tx
    sy = (s * CX + c * CY) + ty
    ux, uy = -((sx - pos_x) - off_x), -((sy - pos_y) - off_y)
    inside = (ux >= 0.0) & (uy >= 0.0) & (ux < len_x) & (uy < len_y)
    with np.errstate(invalid="ignore"):
        jx = np.where(inside, -(((sx - off_x) - pos_x) / res), 0.0).astype(np.int64)
        jy = np.where(inside, -(((sy - off_y) - pos_y) / res), 0.0).astype(np.int64)
    inside &= (jx >= 0) & (jy >= 0) & (jx < nx) & (jy < ny)
    src = np.where(inside, jy * nx + jx, -1).reshape(-1)
    return src, sx.reshape(-1), sy.reshape(-1)


def np_move(state, nx, ny, res, pos_x, pos_y, info):
    """the resample of gv_grid_move, in numpy: fp64 centres and sources in the header's order, getIndex, gather"""
    lo, occ, i8 = state
    src = np_sources(nx, ny, res, pos_x, pos_y, info)[0]
    inside = src >= 0
    src = np.where(inside, src, 0)
    cell_i8 = i8[::-1]   # OccupancyGrid.data[G-1-c] -> cell order
    out_lo = np.where(inside, lo[src], np.float32(0.0)).astype(np.float32)
    out_occ = np.where(inside, occ[src], np.float32(0.5)).astype(np.float32)
    out_i8 = np.where(inside, cell_i8[src], np.int8(50)).astype(np.int8)[::-1].copy()
    return out_lo, out_occ, out_i8


def slice_move(state, nx, ny, kx, ky):
    """a translation by (kx, ky) whole cells: the new map is the old one shifted by kx columns and ky rows towards
    higher indices, the prior where nothing of the old map arrives"""
    lo, occ, i8 = state
    out = []
    for layer, prior in ((lo, np.float32(0.0)), (occ, np.float32(0.5)), (i8[::-1], np.int8(50))):
        old = layer.reshape(ny, nx)
        new = np.full((ny, nx), prior, dtype=layer.dtype)
        if abs(kx) < nx and abs(ky) < ny:
            new[max(ky, 0):ny + min(ky, 0), max(kx, 0):nx + min(kx, 0)] = \
                old[max(-ky, 0):ny + min(-ky, 0), max(-kx, 0):nx + min(-kx, 0)]
        out.append(new.reshape(-1))
    return out[0], out[1], out[2][::-1].copy()


def same(a, b):
    """the layers of two states that differ by bytes"""
    return [LAYERS[k] for k, (x, y) in enumerate(zip(a, b)) if x.tobytes() != y.tobytes()]


def first_difference(got, want, nx, src):
    """None, or the first differing cell in cell order of the first differing layer, with the reference's source cell"""
    G = len(src)
    for k, (x, y) in enumerate(zip(got, want)):
        if x.tobytes() == y.tobytes():
            continue
        if k == 2:
            x, y = x[::-1], y[::-1]
        xb, yb = x.view(np.uint8).reshape(G, -1), y.view(np.uint8).reshape(G, -1)
        bad = np.flatnonzero((xb != yb).any(axis=1))
        c, j = int(bad[0]), int(src[bad[0]])
        return dict(layer=LAYERS[k], n_cells=len(bad), cell=c, ix=c % nx, iy=c // nx, got=xb[c].tobytes().hex(),
                    want=yb[c].tobytes().hex(), src=j, src_ix=j % nx if j >= 0 else None, src_iy=j // nx if j >= 0 else None)
    return None


# ------------------------------------------------------------------------------------------- the device side --
MUTANTS = (
    "always_fast",              # get_index_fast never takes the exact division
    "exact_uses_product",       # its fallback multiplies by fl(1 / res) again
    "sin_negated",              # move_source rotates the other way
    "source_transposed",        # jx * ny + jy
    "far_edge_le",              # the far edge belongs to the map: tx <= len_x && ty <= len_y, and jx > nx || jy > ny in
                                # the index test (which alone would still refuse a source the first test let through)
    "near_edge_gt",             # tx > 0 && ty > 0
    "packed_not_reversed",      # k_grid_move4: byte k of the dword is cell k
    "fill_i8_0",                # off the map: int8 0 instead of 50
    "fill_occ_0",               # off the map: occupancy 0 instead of 0.5
    "last_row_block_skipped",   # ny / 4 row blocks launched instead of (ny + 3) / 4
    "drop_tail_log_odds",       # k_copy_segments without the byte tail, per segment
    "drop_tail_occupancy",
    "drop_tail_int8",
    "occ_segment_unrounded",    # gv_grid_move: the second float segment at G * 4 instead of the 256-byte rounding
)
POISON = 0xA5   # what a scratch byte nobody wrote holds, and what a 16-byte access off its alignment yields


def fast_quotients(nx, ny, res, pos_x, pos_y, sx, sy):
    """get_index_fast's first test and its two quotients per axis: (inside, fast qx, exact qx, fast qy, exact qy)"""
    len_x, len_y = nx * res, ny * res
    off_x, off_y = 0.5 * len_x, 0.5 * len_y
    inv_res = 1.0 / res
    tx, ty = -((sx - pos_x) - off_x), -((sy - pos_y) - off_y)
    inside = (tx >= 0.0) & (ty >= 0.0) & (tx < len_x) & (ty < len_y)
    dx, dy = (sx - off_x) - pos_x, (sy - off_y) - pos_y
    return inside, -dx * inv_res, -(dx / res), -dy * inv_res, -(dy / res)


def _get_index_fast(geom, sx, sy, mutant):
    nx, ny, res, pos_x, pos_y = geom
    len_x, len_y = nx * res, ny * res
    off_x, off_y = 0.5 * len_x, 0.5 * len_y
    inv_res = 1.0 / res
    tx, ty = -((sx - pos_x) - off_x), -((sy - pos_y) - off_y)
    near = (tx > 0.0) & (ty > 0.0) if mutant == "near_edge_gt" else (tx >= 0.0) & (ty >= 0.0)
    far = (tx <= len_x) & (ty <= len_y) if mutant == "far_edge_le" else (tx < len_x) & (ty < len_y)
    ok = near & far
    out = []
    for d in ((sx - off_x) - pos_x, (sy - off_y) - pos_y):
        q = -d * inv_res
        if mutant != "always_fast":
            exact = -d * inv_res if mutant == "exact_uses_product" else -(d / res)
            q = np.where(np.abs(q - np.rint(q)) < 1e-6, exact, q)
        out.append(np.where(ok, q, 0.0).astype(np.int64))   # (int)q
    jx, jy = out
    past = (jx > nx) | (jy > ny) if mutant == "far_edge_le" else (jx >= nx) | (jy >= ny)
    ok = ok & ~((jx < 0) | (jy < 0) | past)
    return ok, jx, jy


def _move_source(geom, info, ix, iy, mutant):
    nx, ny, res, pos_x, pos_y = geom
    off_x, off_y = 0.5 * (nx * res), 0.5 * (ny * res)
    hx, hy = pos_x + off_x, pos_y + off_y
    c, s = info["cos_yaw"], info["sin_yaw"]
    if mutant == "sin_negated":
        s = -s
    cx = hx - (ix.astype(np.float64) + 0.5) * res
    cy = hy - (iy.astype(np.float64) + 0.5) * res
    sx = (c * cx - s * cy) + info["tx"]
    sy = (s * cx + c * cy) + info["ty"]
    ok, jx, jy = _get_index_fast(geom, sx, sy, mutant)
    j = jx * ny + jy if mutant == "source_transposed" else jy * nx + jx
    return np.where(ok, j, -1)


def emulate(state, nx, ny, res, pos_x, pos_y, info, mutant=None):
    """gv_grid_move's device work on byte arrays: the gather into the scratch block (k_grid_move4 for nx % 4 == 0,
    k_grid_move1 otherwise, 64 x 4 lanes a workgroup), then k_copy_segments back into the resident layers"""
    assert mutant is None or mutant in MUTANTS
    geom = (nx, ny, res, pos_x, pos_y)
    G = nx * ny
    lo, occ, i8 = (np.ascontiguousarray(a).view(np.uint8).copy() for a in state)   # the resident layers
    lo_w, occ_w = lo.view(np.uint32), occ.view(np.uint32)
    fbytes = (G * 4 + 255) & ~255
    off = (0, G * 4 if mutant == "occ_segment_unrounded" else fbytes, 2 * fbytes)
    scratch = np.full(2 * fbytes + G, POISON, np.uint8)
    lo_out, occ_out = (scratch[o:o + G * 4].view(np.uint32) for o in off[:2])
    i8_out = scratch[off[2]:off[2] + G]
    fill = (np.float32(0.0).view(np.uint32), np.float32(0.0 if mutant == "fill_occ_0" else 0.5).view(np.uint32),
            np.uint8(0 if mutant == "fill_i8_0" else 50))

    def gather(ix, iy):
        src = _move_source(geom, info, ix, iy, mutant)
        ok, j = src >= 0, np.where(src >= 0, src, 0) % G   # (% G: a mutant's index past the layer stays in the arrays)
        return np.where(ok, lo_w[j], fill[0]), np.where(ok, occ_w[j], fill[1]), np.where(ok, i8[G - 1 - j], fill[2])

    gy = (ny + 3) // 4
    if mutant == "last_row_block_skipped":
        gy = ny // 4
    four = nx % 4 == 0
    gx = (nx // 4 + 63) // 64 if four else (nx + 63) // 64
    lane_x, lane_y = np.meshgrid(np.arange(gx * 64), np.arange(gy * 4))   # blockIdx * 64 + threadIdx.x, blockIdx * 4 + threadIdx.y
    ix0, iy = (lane_x * 4 if four else lane_x).reshape(-1), lane_y.reshape(-1)
    live = (ix0 < nx) & (iy < ny)
    ix0, iy = ix0[live], iy[live]
    c = iy * nx + ix0
    if four:
        packed = np.zeros(len(c), np.uint32)
        for k in range(4):
            a, b, d = gather(ix0 + k, iy)
            lo_out[c + k], occ_out[c + k] = a, b
            packed |= d.astype(np.uint32) << np.uint32(8 * (k if mutant == "packed_not_reversed" else 3 - k))
        for j in range(4):   # one dword store at i8_out + (G - 4 - c), little-endian
            i8_out[G - 4 - c + j] = (packed >> np.uint32(8 * j)).astype(np.uint8)
    else:
        a, b, d = gather(ix0, iy)
        lo_out[c], occ_out[c], i8_out[G - 1 - c] = a, b, d

    # k_copy_segments: 16 bytes a lane over a grid-stride loop (every i < n16 is some lane's), then the tail by the
    # first 256 lanes.  Its 16-byte accesses hold to their contract here: off a multiple of 16 they yield POISON.
    for name, o, dst, nbytes in (("log_odds", off[0], lo, G * 4), ("occupancy", off[1], occ, G * 4), ("int8", off[2], i8, G)):
        n16 = nbytes // 16
        dst[:n16 * 16] = scratch[o:o + n16 * 16] if o % 16 == 0 else POISON
        t = n16 * 16 + np.arange(256)
        t = t[t < nbytes]
        if mutant != "drop_tail_" + name:
            dst[t] = scratch[o + t]
    return lo.view(np.float32), occ.view(np.float32), i8.view(np.int8)
