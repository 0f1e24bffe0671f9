"""CPU side of tests/test_gpu_camera.py: from the oracle's ids and projections alone, every (camera, box set, scene) the
GPU tests use reaches what tests/camera_cases.py built it for, and the cases take the table paths they are listed for
(fused or unfused box test in the frame, k_pose_classify with its tables in LDS or in global memory), computed from the
two limits as the sources state them.  When someone changes a limit, test_path_table says which cases moved.

The shares at `pixel` (one 1 x 1 image) are the same as everywhere: scenes are aimed at pixel targets over
[-0.1 W, 1.1 W] x [-0.1 H, 1.1 H], so about 65 % of a scene's points get an id >= 0 and about 35 % get -1 at every
camera, `pixel` included (asserted below like the others)."""
import os
import re

import numpy as np
import pytest

import camera_cases as cc
import oracle_lib as ol
import pose_ref as P

CSRC = os.path.join(ol.ROOT, "grid-vision_amd", "csrc")
SETS = [(c, pt, nb) for c in cc.CAMERAS for pt in (False, True) for nb in cc.box_sizes(cc.CAMERAS[c])]


@pytest.mark.parametrize("cam_name", list(cc.CAMERAS))
@pytest.mark.parametrize("perturbed", [False, True])
def test_scene_conditions(cam_name, perturbed):
    cam, s, g = cc.CAMERAS[cam_name], cc.scene(cam_name, perturbed), cc.geo(cam_name, perturbed)
    n = len(s.x)
    assert n == cc.SCENE_SIZES[perturbed] and 20_000 <= n <= 60_000
    assert (n % cc.CHUNK == 0) == perturbed
    assert s.x.dtype == s.y.dtype == s.z.dtype == np.float32
    # Geo's projection is the oracle's own, bit for bit
    ok = np.isfinite(g.cx) & np.isfinite(g.cy) & np.isfinite(g.cz) & (g.cz > 0)
    u, v, d = ol.project_points(cc.K_of(cam), g.cx[ok], g.cy[ok], g.cz[ok])
    assert u.tobytes() == g.u[ok].tobytes() and v.tobytes() == g.v[ok].tobytes()
    # at least 10 points within NEAR on each side of each image border, and of every tile edge the scene aims at
    for axis, bound in cc.near_bounds(cam):
        p, o, ext = (g.u, g.v, cam.h) if axis == 0 else (g.v, g.u, cam.w)
        close = g.front & (np.abs(p.astype(np.float64) - bound) <= cc.NEAR) & (o >= 0) & (o < ext)
        assert (close & (p < bound)).sum() >= 10 and (close & (p >= bound)).sum() >= 10, (axis, bound)
    assert {(0, 0.0), (0, float(cam.w)), (1, 0.0), (1, float(cam.h))} <= set(cc.near_bounds(cam))
    if cam.w % 16:
        assert cam.w < 16 or (0, 16.0 * (cam.w // 16)) in cc.near_bounds(cam)
    if cam.h % 16:
        assert cam.h < 16 or (1, 16.0 * (cam.h // 16)) in cc.near_bounds(cam)
    # cz on both sides of 0.001, points behind the camera, every non-finite kind
    fin = np.isfinite(g.cz)
    assert (fin & (g.cz > 0) & (g.cz <= np.float32(0.001))).sum() >= 20
    assert (fin & (g.cz > np.float32(0.001)) & (g.cz < np.float32(0.00105))).sum() >= 20
    assert (fin & (g.cz < 0)).sum() >= n // 20
    for a in (s.x, s.y, s.z):
        assert np.isnan(a).sum() >= 8 and (a == np.inf).sum() >= 8 and (a == -np.inf).sum() >= 8
    # every depth of the list is in the image, and points are off it on all four sides
    for d in cc.DEPTHS:
        assert (g.inimg & (np.abs(g.cz - d) < 0.02 * d)).sum() >= 1000, d
    for m in (g.u < 0, g.u >= cam.w, g.v < 0, g.v >= cam.h):
        assert (g.front & m).sum() >= 500
    # the small clouds of the pipeline test are mixtures too
    for k in cc.SMALL_SIZES:
        assert 0.3 * k <= g.inimg[:k].sum() <= 0.7 * k


@pytest.mark.parametrize("cam_name,perturbed,nb", SETS)
def test_box_set_conditions(cam_name, perturbed, nb):
    cam, g = cc.CAMERAS[cam_name], cc.geo(cam_name, perturbed)
    bs = cc.box_set(cam_name, perturbed, nb)
    b = bs.boxes
    n = len(g.u)
    assert len(b) == nb
    ids = g.ids(b)
    first, last = cc.containing(g, b)
    assert np.array_equal(first, ids)                       # the reference's comparison, restated
    assert (ids < 0).sum() >= 0.05 * n and (ids >= 0).sum() >= 0.30 * n
    words = cc.mask_words(nb)
    for w in range(words):
        assert ((ids >= 64 * w) & (ids < 64 * w + 64)).sum() >= 20, ("mask word", w)
    tx, ty = cc.tiles(cam)
    with np.errstate(invalid="ignore"):
        col, row = g.u.astype(np.int64) >> 4, g.v.astype(np.int64) >> 4
    if cam.w % 16:
        assert ((ids >= 0) & (col == tx - 1)).sum() >= 20
    if cam.h % 16:
        assert ((ids >= 0) & (row == ty - 1)).sum() >= 20
    if nb == 1:
        assert bs.roles == {"whole": 0} and b[0]["x_min"] < 0 and b[0]["x_max"] > cam.w
        return
    assert b["x_min"][np.isfinite(b["x_min"])].tolist() != np.rint(b["x_min"][np.isfinite(b["x_min"])]).tolist()
    r = bs.roles
    assert r["whole"] == nb - 1 and set(cc.ROLES) <= set(r)
    for name in cc.NO_MATCH_ROLES:
        assert (ids == r[name]).sum() == 0 and (last != r[name]).all(), name
    sc, sr = b[r["strip_col"]], b[r["strip_row"]]
    assert cam.w < sc["x_min"] and sc["y_min"] < 0 and sc["y_max"] > cam.h and cam.h < sr["y_min"]
    if cam.w % 16:
        assert sc["x_min"] < 16 * tx - 1          # the strip box reaches into the last tile's padding: its mask bit is set
        assert (ids == r["ragged_col"]).sum() >= 1 and b[r["ragged_col"]]["x_max"] == cam.w + 40.25
    if cam.h % 16:
        assert sr["y_min"] < 16 * ty - 1
        assert (ids == r["ragged_row"]).sum() >= 1
    assert np.isnan(b[r["nan"]]["x_max"]) and b[r["empty"]]["x_max"] < b[r["empty"]]["x_min"]
    pc = b[r["pixel_col"]]
    assert pc["x_min"] == cam.w - 1 and ((first <= r["pixel_col"]) & (last >= r["pixel_col"]) & (g.u >= cam.w - 1)).sum() >= 1
    # overlapping boxes: first match is not last match; the planted pair shares points, which the later box never gets
    assert ((first >= 0) & (first != last)).sum() >= 1
    both = cc.inside(g, b[r["overlap_a"]]) & cc.inside(g, b[r["overlap_b"]])
    assert both.sum() >= 20 and (ids[both] < r["overlap_b"]).all()
    # exact bounds: the box's bound IS the float u (v) of its point, and on each of the four edges one such point or more
    # is matched by its own box
    hit = {e: 0 for e in cc.EDGES}
    assert len(bs.exact) == 40
    for k, p, e in bs.exact:
        assert b[k][e] == float((g.u if e[0] == "x" else g.v)[p])
        hit[e] += int(ids[p] == k)
    assert all(hit[e] >= 1 for e in cc.EDGES), hit


@pytest.mark.parametrize("cam_name,nb", cc.POSE_CASES)
def test_pose_scene_conditions(cam_name, nb):
    cam, s = cc.CAMERAS[cam_name], cc.pose_scene(cam_name, nb)
    assert len(s.boxes) == nb and len(s.x) <= 8192
    camf, res = P.reference(s, K=cc.K_of(cam), w=cam.w, h=cam.h)
    g = cc.Geo(cam, {"base_lidar": P.IDENT_TF, "cam_lidar": P.IDENT_TF}, s.x, s.y, s.z)
    assert np.array_equal(g.ids(s.boxes), res.ids)
    full = [b for b in range(nb) if b not in s.meta["empty"]]
    assert res.valid[full].sum() >= max(1, int(0.8 * len(full))) and (res.ids < 0).sum() >= 100
    assert (res.keep[res.ids >= 0] == 0).sum() >= 20          # background points that the radius filter drops
    tx, ty = cc.tiles(cam)
    sel = res.ids >= 0
    if cam.w % 16:
        assert (sel & res.keep & ((g.u.astype(np.int64) >> 4) == tx - 1)).sum() >= 10
        assert (g.front & (g.u >= cam.w) & (g.u < cam.w + 16)).sum() >= 1     # part of a cluster falls off the image
    if cam.h % 16:
        assert (sel & res.keep & ((g.v.astype(np.int64) >> 4) == ty - 1)).sum() >= 10


@pytest.mark.parametrize("cam_name", ["hd720", "kitti"])
def test_tick_scene_conditions(cam_name):
    """70 separate boxes, one in five static, every dynamic one with an oracle pose once the ground is removed"""
    s, b = cc.tick_scene(cam_name, 70)
    g = cc.Geo(s.cam, s.tfs, s.x, s.y, s.z)
    st, dy = ol.filter_bboxes(b)
    assert len(b) == 70 and len(st) == 14 and len(dy) == 56 and 20_000 <= len(s.x) <= 60_000
    m, ground, _ = ol.segment_ground_plane(g.cx, g.cy, g.cz)
    assert 11_000 <= m <= 13_500
    ids = g.ids(b)
    first, last = cc.containing(g, b)
    assert (first == last).all() and (np.bincount(ids[(ids >= 0) & (ground == 0)], minlength=70) >= 100).all()
    assert cc.mask_words(70) == 2


def _limit(path, pattern):
    m = re.search(pattern, open(os.path.join(CSRC, path)).read())
    assert m, f"{pattern} not found in {path}"
    return int(m.group(1)) * 1024


def test_path_table():
    import test_gpu_camera as T
    fuse_max = _limit("gv_launch_frame.hpp", r"kBinBBoxLdsMax\s*=\s*(\d+)\s*\*\s*1024")
    lds_max = _limit("gv_cloudops.hip", r"tab_bytes\s*<=\s*(\d+)\s*\*\s*1024")

    def fused(c, nb):
        return cc.frame_table_bytes(cc.CAMERAS[c], nb) <= fuse_max

    def in_lds(c, nb):
        return cc.classify_table_bytes(cc.CAMERAS[c], nb) <= lds_max

    assert T.FRAME_CASES is cc.FRAME_CASES and T.POSE_CASES is cc.POSE_CASES
    frames = {(c, nb): fused(c, nb) for c, nb in T.FRAME_CASES}
    frames.update({(c, nb): fused(c, nb) for c, sets in T.PIPELINE_CASES for nb in sets})
    frames.update({(c, nb): fused(c, nb) for c, nb, _ in T.SHARD_CASES})
    classify = {(c, nb): in_lds(c, nb) for c, nb in T.POSE_CASES}
    moved = "a limit moved: frames fused %s, classify in LDS %s" % (frames, classify)
    for table in (frames, classify):
        for want in (True, False):
            assert len({c for (c, nb), v in table.items() if v == want}) >= 2, moved
    assert not any(v for (c, nb), v in frames.items() if c == "hd720"), moved
    assert not any(v for (c, nb), v in classify.items() if c == "hd1080"), moved
    assert all(not fused("hd720", nb) for nb in cc.BOX_SIZES) and all(not in_lds("hd1080", nb) for nb in cc.BOX_SIZES), moved
    assert fused("synth", 64) and in_lds("synth", 64) and frames[("synth", 64)] and classify[("synth", 64)], moved
    # the thresholds the cases were chosen around
    assert fused("kitti", 64) and not fused("kitti", 65), moved
    assert in_lds("hd720", 64) and not in_lds("hd720", 65), moved
    assert in_lds("kitti", 64) and not in_lds("kitti", 257), moved
    # one classify case cannot run from LDS at all: with the limit raised or ignored its launch fails
    assert any(cc.classify_table_bytes(cc.CAMERAS[c], nb) > cc.CU_LDS_BYTES for c, nb in T.POSE_CASES), moved
    # the pipeline alternates a fused and an unfused set at kitti and runs unfused throughout at hd720
    for c, sets in T.PIPELINE_CASES:
        assert [fused(c, nb) for nb in sets] == ([True, False] if c == "kitti" else [False, False]), moved
    # the stale-table sequence shrinks from five mask words to one and changes path on the way
    c, seq = T.STALE_CASE
    assert [cc.mask_words(nb) for nb in seq] == [5, 1, 1] and fused(c, seq[2])
