"""tests/pose_ref.py without a GPU: its keep flags equal the oracle's on every box of every family, its poses lie
within the gates the device's poses are already held to (test_gpu_parity._check_pose against the oracle,
_check_pose_fp64 against fp64 numpy), and every fixture family reaches what it was built for -- a generator that stops
producing the edge it exists for fails here, on the CPU.

The oracle does NOT clamp (gvo_pca_bbox sums floats as they are): where a family reaches the +-2047 m or +-127 m
clamps or 1e30 (family e), the reference and the oracle are compared on keep flags only.  That difference IS the
device's contract ("The PCA rectangle's sums")."""
import numpy as np
import pytest

import oracle_lib as ol
import pose_ref as P
from test_gpu_parity import _check_pose, _check_pose_fp64

F32 = np.float32
ALL_SCENES = [s for f in P.FAMILIES for s in P.family(f)]
CLAMPED = ("far",)


def _box_points(scene, b):
    (cx, cy, cz), res = P.reference(scene)
    sel = res.ids == b
    return cx[sel], cy[sel], cz[sel], res.keep[sel]


def _well_conditioned(x, z):
    """_check_pose_fp64's own condition: the two eigenvalues of the fp64 covariance of (z, x) lie a thousandth apart"""
    D = np.stack([z.astype(np.float64), x.astype(np.float64)], axis=1)
    wv = np.linalg.eigvalsh(np.cov(D.T, bias=True)) if len(x) > 1 else np.zeros(2)
    return bool(wv[1] > 0 and wv[1] - wv[0] >= 1e-3 * wv[1])


def _query_row(scene, i):
    """float32 d2 of point i of the scene to the points of its own box (itself included), and their cloud indices"""
    (cx, cy, cz), res = P.reference(scene)
    assert res.ids[i] >= 0, (scene.tag, i)
    idx = np.flatnonzero(res.ids == res.ids[i])
    with np.errstate(all="ignore"):
        d = cx[idx] - cx[i]; r = d * d
        d = cy[idx] - cy[i]; r = r + d * d
        d = cz[idx] - cz[i]; r = r + d * d
    assert r.dtype == F32
    return r, idx


def test_families_are_within_the_stated_sizes():
    tags = [s.tag for s in ALL_SCENES]
    assert len(set(tags)) == len(tags)
    for s in ALL_SCENES:
        (cx, cy, cz), res = P.reference(s)
        assert len(s.x) <= 20_000 and len(s.boxes) <= 400, s.tag
        sel = res.ids >= 0
        assert (cz[sel] > 0.001).all()
    # every point of the families a .. f is selectable: z > 0.001 and inside the image (count-edge leaves its "outside
    # every box" points inside the image too)
    for f in P.FAMILIES[:-1]:
        for s in P.family(f):
            cx, cy, cz = P.reference(s)[0]
            u, v = 320.0 * cx.astype(np.float64) / cz + 320.0, 320.0 * cy.astype(np.float64) / cz + 240.0
            assert (cz > 0.001).all() and (u >= 0).all() and (u < 640).all() and (v >= 0).all() and (v < 480).all(), s.tag


@pytest.mark.parametrize("fam", P.FAMILIES)
def test_keep_flags_equal_the_oracle(fam):
    """all pairs in numpy against gvo_radius_outlier, every box of every scene (the far family included)"""
    boxes = 0
    for s in P.family(fam):
        for b in range(len(s.boxes)):
            x, y, z, kp = _box_points(s, b)
            if len(x):
                assert np.array_equal(kp, ol.radius_outlier(x, y, z, 0.4, 10).astype(bool)), (s.tag, b)
                boxes += 1
    assert boxes >= 1


@pytest.mark.parametrize("fam", [f for f in P.FAMILIES if f not in CLAMPED])
def test_poses_within_the_gates_of_the_oracle_and_fp64(fam):
    """where nothing is clamped the reference's pose is the oracle's up to the rounding the oracle's float running sums
    accumulate (_check_pose), and its centre and extents are fp64 numpy's (_check_pose_fp64).  Where the axes are ill
    conditioned (equal points, a square lattice) the oracle's own float sums decide them, and only the centre is held"""
    n = well = 0
    for s in P.family(fam):
        res = P.reference(s)[1]
        for b in range(len(s.boxes)):
            x, y, z, kp = _box_points(s, b)
            ok, e = ol.pca_bbox(x[kp], y[kp], z[kp])
            assert ok == bool(res.valid[b]), (s.tag, b)
            if ok and _well_conditioned(x[kp], z[kp]):
                _check_pose(res.poses[b], e, (s.tag, b))
                _check_pose_fp64(res.poses[b], x[kp], y[kp], z[kp], (s.tag, b))
                well += 1
            elif ok:    # equal points, isotropic lattices: the axes are anybody's; the centre is not
                for f in ("px", "py", "pz"):
                    assert res.poses[b][f] == pytest.approx(e[f], rel=1e-4, abs=1e-4), (s.tag, b, f)
                _check_pose_fp64(res.poses[b], x[kp], y[kp], z[kp], (s.tag, b))
            if ok:
                assert res.poses[b]["qx"] == 0 and res.poses[b]["qz"] == 0 and res.poses[b]["height"] == 0
                n += 1
    assert n >= 1 and well >= (2 if fam == "degenerate" else 0.75 * n), (n, well)


def test_no_box_hangs_on_the_last_bit_of_atan2():
    """float32(atan2) must not depend on which correctly working fp64 atan2 computed it: no box of any family has its
    angle within 1e-15 (relative) of a float32 rounding boundary, so none had to be replaced"""
    n = 0
    for s in ALL_SCENES:
        for r in P.reference(s)[1].rects:
            if r is not None:
                assert not r.atan2_fragile, s.tag
                n += 1
    print(f"\n{n} rectangles over {len(ALL_SCENES)} scenes, none fragile")


# ------------------------------------------------------------------------------------------ (a) radius edge --

def test_radius_edge_conditions():
    (s,) = P.family("radius-edge")
    res = P.reference(s)[1]
    kept, dropped, boxes = 0, 0, set()
    for i, exact in s.meta["queries"]:
        r, _ = _query_row(s, i)
        assert np.count_nonzero(r < P.R2F) == 10, i            # ten strictly inside, the query among them
        assert np.count_nonzero(r == P.R2F) == (1 if exact else 0), i
        assert np.count_nonzero(r == P.R2F_UP) == (0 if exact else 1), i
        assert bool(res.keep[i]) == exact, i
        kept += exact
        dropped += not exact
        boxes.add(int(res.ids[i]))
    assert kept >= 64 and dropped >= 64 and len(boxes) >= 16, (kept, dropped, len(boxes))
    assert float(P.R2F) <= 0.4 * 0.4 < float(P.R2F_UP)


# ------------------------------------------------------------------------------------------- (b) count edge --

def test_count_edge_conditions():
    (s,) = P.family("count-edge")
    (cx, cy, cz), res = P.reference(s)
    nf = s.meta["n_first"]
    kinds = set()
    for tag, o, m, kind in s.meta["clusters"]:
        idx = np.arange(o, o + m)
        body = idx if kind in (None, "same") else np.delete(idx, 10)
        assert (res.ids[body] >= nf).all() and len(set(res.ids[body])) == 1, tag
        for i in body:
            r, _ = _query_row(s, i)
            assert np.count_nonzero(r <= P.R2F) == len(r) == len(body), tag   # mutually close, and alone in their box
        assert (res.keep[body] == (len(body) >= 11)).all(), tag
        if kind == "stolen":      # first match gives the 11th point to the EARLIER box; it is within the radius of the others
            assert 0 <= res.ids[idx[10]] < nf and not res.keep[idx[10]], tag
            later = np.flatnonzero(res.ids == res.ids[body[0]])
            assert set(later) == set(body)
            with np.errstate(all="ignore"):
                d = ((cx[body] - cx[idx[10]]) ** 2 + (cy[body] - cy[idx[10]]) ** 2) + (cz[body] - cz[idx[10]]) ** 2
            assert (d < 0.9 * P.R2F).all(), tag   # 0.34 m at the most
        elif kind == "outside":
            assert res.ids[idx[10]] == -1, tag
        elif kind == "same":
            assert len(set(zip(cx[idx].tolist(), cy[idx].tolist(), cz[idx].tolist()))) == 1, tag
        kinds.add(tag)
    assert kinds == {k[0] for k in P.COUNT_KINDS}


# -------------------------------------------------------------------------------------- (c) neighbour cells --

def _cell_cluster_conditions(s, k, base, off):
    (cx, cy, cz), res = P.reference(s)
    idx = np.arange(11 * k, 11 * k + 11)
    assert len(set(res.ids[idx])) == 1 and res.ids[idx[0]] >= 0, (s.tag, k)
    cells = np.stack([P.cell_of(cx[idx]), P.cell_of(cy[idx]), P.cell_of(cz[idx])], axis=1)
    assert (cells[:10] == np.asarray(base)[None, :]).all(), (s.tag, k)
    assert (cells[10] == np.asarray(base) + np.asarray(off)).all(), (s.tag, k)
    for i in idx:   # exactly 11 neighbours each: every point needs all the others, the one in the offset cell included
        r, j = _query_row(s, i)
        assert np.count_nonzero(r <= P.R2F) == 11 and set(j[r <= P.R2F]) == set(idx), (s.tag, k)
    assert res.keep[idx].all()


@pytest.mark.parametrize("which", [0, 1])
def test_neighbour_cell_conditions(which):
    s = P.family("cells")[which]
    seen = set()
    for k, (base, off) in enumerate(s.meta["clusters"]):
        _cell_cluster_conditions(s, k, base, off)
        assert all((c > 0) == (which == 0) for c in base[:2])
        seen.add((tuple(c % 8 for c in base), off))
    assert len(seen) == 27 * 27 and {r for r, _ in seen} == {(a, b, c) for a in P.RESIDUES for b in P.RESIDUES for c in P.RESIDUES}
    assert len(set(P.reference(s)[1].ids[::11])) >= 8   # spread over boxes


@pytest.mark.parametrize("which", [3, 4, 5, 6])
def test_straddle_conditions(which):
    s = P.family("cells")[which]
    bx, by = ((0, 0), (0, -1), (-1, 0), (-1, -1))[which - 3]
    for k, (base, off) in enumerate(s.meta["clusters"]):
        _cell_cluster_conditions(s, k, base, off)
        assert base[:2] == (bx, by)
    assert [o for _, o in s.meta["clusters"]] == list(P.OFFSETS)
    assert {(b[2] % 8, o[2]) for b, o in s.meta["clusters"]} == {(r, d) for r in P.RESIDUES for d in (-1, 0, 1)}
    cz = P.reference(s)[0][2].astype(np.float64)
    assert np.abs(cz - cz.mean()).max() < 100      # no centred sample near the +-127 m clamp


def test_face_conditions():
    s = P.family("cells")[2]
    (cx, cy, cz), res = P.reference(s)
    assert s.tag == "cells-faces" and ((s.x * 2) % 1 == 0).all() and ((s.y * 2) % 1 == 0).all()     # exactly on k * 0.5
    for a in (s.x, s.y):
        assert np.count_nonzero((a == 0) & np.signbit(a)) >= 11 and np.count_nonzero((a == 0) & ~np.signbit(a)) >= 11
    assert not (np.signbit(cx) & (cx == 0)).any() and not (np.signbit(cy) & (cy == 0)).any()   # the transform leaves +0.0
    assert np.count_nonzero((cz * 2) % 1 == 0) == s.meta["n_face"] == 20
    assert res.keep.all() and (res.ids == 0).all()
    for i in range(0, len(s.x), 11):
        r, j = _query_row(s, i)
        assert set(j[r <= P.R2F]) == set(range(i, i + 11))


def test_iz0_conditions():
    scenes = P.family("cells")[7:]
    assert len(scenes) == 32
    for s in scenes:
        ((base, off),) = s.meta["clusters"]
        _cell_cluster_conditions(s, 0, base, off)
        assert base[2] == 0 and off[2] in (0, 1)


# ------------------------------------------------------------------------------------------- (d) long runs --

def test_long_run_conditions():
    (s,) = P.family("long-runs")
    (cx, cy, cz), res = P.reference(s)
    cell = np.stack([P.cell_of(cx), P.cell_of(cy), P.cell_of(cz)], axis=1)
    lengths = {0: [], 7: []}
    for kind, base, L, o in s.meta["clusters"]:
        base = np.asarray(base)
        r, j = _query_row(s, o)
        near = j[r <= P.R2F]
        if kind == "run":
            assert (cell[o] == base).all()
            assert len(near) == 11 and set(near) == set(range(o, o + 11))      # itself + the ten partners
            assert (cell[o + 1:o + 11] == base + np.array([0, 1, 1])).all()      # the row visited last
            for q, sx in enumerate((0, -1, 1)):
                far = np.arange(o + 11 + q * L, o + 11 + (q + 1) * L)
                assert (cell[far] == base + np.array([sx, 0, 0])).all() and (res.ids[far] == res.ids[o]).all()
                assert not set(far) & set(near)
            assert res.keep[o]
            lengths[base[0] % 8].append(L)
        else:
            frac = np.array([cx[o], cy[o], cz[o]], np.float64) / P.CELL - base
            assert ((frac * P.CELL >= 0.1) & (frac * P.CELL < 0.4)).all() and base[0] % 8 in (0, 7)
            block = np.arange(o, o + 27)
            assert {tuple(c) for c in cell[block] - base} == set(P.OFFSETS) and (res.ids[block] == res.ids[o]).all()
            assert len(near) == 11 and set(near) <= set(block) and res.keep[o]
            assert len({tuple(c) for c in cell[near] - base}) == 11        # every hit in another cell
    assert lengths[0] == list(P.RUN_LENGTHS) and lengths[7] == list(P.RUN_LENGTHS)
    assert sum(1 for c in s.meta["clusters"] if c[0] == "all-27") == 2


# -------------------------------------------------------------------------------------------- (e) far points --

def test_far_conditions():
    (s,) = P.family("far")
    (cx, cy, cz), res = P.reference(s)
    o = np.concatenate([[0], np.cumsum(s.meta["parts"])])
    part = [slice(o[i], o[i + 1]) for i in range(5)]
    assert (res.ids >= 0).all() and all(len(set(res.ids[p])) == 1 for p in part) and len(set(res.ids)) == 5
    reach = lambda c: F32(0.4000005) + F32(2.5e-7) * np.abs(c)      # the margin of the device's cell range
    assert (cz[part[0]] >= 3e6).all() and (reach(cz[part[0]]) > 1).all() and (np.abs(cx[part[0]]) < 1).all()
    assert len(set(cz[part[0]])) == 3 and (np.diff(sorted(set(cz[part[0]]))) == 0.25).all()
    assert (cx[part[1]] >= 1.5e6).all() and (cz[part[1]] >= 3e6).all() and len(set(cx[part[1]])) == 3
    assert (cz[part[2]] == F32(1e30)).all() and (cz[part[2]] >= 5e8).all() and res.keep[part[2]].all()
    assert cz[part[3]].min() < 2047 < cz[part[3]].max() and res.keep[part[3]].all()
    kz = cz[part[4]][res.keep[part[4]]]
    assert kz.max() - kz.min() > 254 and res.keep[part[4]].all()
    assert res.valid.all()
    # the clamps show: the reference's centre is not the fp64 mean where they engage
    assert res.poses[res.ids[o[2]]]["pz"] == 2047.0 and res.poses[res.ids[o[2]]]["px"] == -2047.0
    assert res.poses[res.ids[o[0]]]["pz"] == 2047.0
    assert res.poses[res.ids[o[3]]]["pz"] < float(np.mean(cz[part[3]].astype(np.float64))) - 0.01
    assert res.rects[res.ids[o[4]]].cov[0] == 127.0 ** 2     # every centred z beyond +-127 m: the sum is of clamped samples
    assert res.poses[res.ids[o[4]]]["length"] > 254.0          # the extents are not clamped
    assert res.keep[part[0]].any() and res.keep[part[1]].any()


# ----------------------------------------------------------------------------------- (f) degenerate rectangles --

def test_degenerate_conditions():
    (s,) = P.family("degenerate")
    res = P.reference(s)[1]
    assert res.valid.all() and (np.bincount(res.ids, minlength=6) == s.meta["parts"]).all()
    cov = {k: res.rects[i].cov for i, k in enumerate(P.DEGENERATE)}
    major = {k: res.rects[i].major for i, k in enumerate(P.DEGENERATE)}
    pose = {k: res.poses[i] for i, k in enumerate(P.DEGENERATE)}
    assert cov["equal"] == (0, 0, 0) and major["equal"] == (1, 0) and pose["equal"]["length"] == 0 == pose["equal"]["width"]
    assert cov["line-z"][0] > 0 and cov["line-z"][1:] == (0, 0) and major["line-z"] == (1, 0) and pose["line-z"]["width"] == 0
    assert cov["line-x"][2] > 0 and cov["line-x"][:2] == (0, 0) and major["line-x"] == (0, 1) and pose["line-x"]["width"] == 0
    assert cov["square"][0] == cov["square"][2] > 0 and cov["square"][1] == 0 and major["square"] == (1, 0)
    assert cov["diagonal"][0] == cov["diagonal"][2] > 0 and cov["diagonal"][1] != 0
    assert abs(major["diagonal"][0]) == pytest.approx(2 ** -0.5, abs=1e-7)
    assert pose["line-z"]["length"] == pytest.approx(23 / 32) and pose["line-x"]["length"] == pytest.approx(23 / 32)
    one = res.ids == 5
    assert res.keep[one].sum() == 11 and one.sum() == 18


# -------------------------------------------------------------------------------------------------- (g) sizes --

def test_size_conditions():
    scenes = {s.tag: s for s in P.family("sizes")}
    for nb in P.NB_SIZES:
        s = scenes[f"nb-{nb}"]
        res = P.reference(s)[1]
        cnt = np.bincount(res.ids[res.ids >= 0], minlength=nb)
        assert len(s.boxes) == nb and (res.ids >= 0).all()
        assert all(cnt[b] == (0 if b in s.meta["empty"] else 12) for b in range(nb)), nb
        assert (res.valid == (cnt == 12)).all() and (nb < 7 or len(s.meta["empty"]) >= 1)
    for n in P.CLOUD_SIZES:
        assert len(scenes[f"cloud-{n}"].x) == n
        assert (P.reference(scenes[f"cloud-{n}"])[1].ids >= 0).sum() == min(n, 576)
    for m in P.SELECTED_SIZES:
        res = P.reference(scenes[f"selected-{m}"])[1]
        assert (res.ids >= 0).sum() == m and res.keep.sum() == (m if m >= 11 else 0)


def test_behind_camera_cloud_selects_nothing_and_grows_the_table():
    x, y, z = P.behind_camera_cloud()
    assert len(x) == 1_100_000 and (z < 0).all()
    assert len(x) / 2 > 2 ** 19     # the bucket count doubles while it is below n / 2: 2^20
