"""tests/vision_ref.py -- the plain reference that tests/test_gpu_vision.py holds the device to -- pinned to the oracle,
given a second opinion, and the scenes checked for the conditions they are there for (CPU only).

  * trig="libm" equals the oracle bit for bit on every scene: alpha, theta_ray, all 64 solutions and residuals, the
    emitted poses.  This pins the restated QR and the operation order.
  * trig="fp64" -- the device's contract -- against numpy.linalg.lstsq on well-conditioned boxes.
  * the fixture conditions, from the reference's own census.
  * the trig census: where the two modes differ on the scenes, and per function over a seeded sample (DESIGN,
    Tolerances, holds the figures of glibc 2.35)."""
import math
import platform

import numpy as np

import oracle_lib as ol
import vision_ref as R
from gvamd import synth
from test_oracle_second_opinions import _constraint_sets, _pinhole_system

F = np.float32


def _ocam(sc):
    return ol.make_cam(*R.CAMS[sc.cam], R.IMG_W, R.IMG_H)


def test_libm_mode_equals_the_oracle_bit_for_bit():
    """every box of every scene, no exclusions: finite values by bytes, NaN by class"""
    bins = ol.generate_bins(2)
    n = 0
    for sc in R.all_scenes():
        ref = R.reference(sc, "libm")
        cam = _ocam(sc)
        for i in range(len(sc.boxes)):
            alpha = F(ol.compute_alpha(sc.orient[i], int(ref.argmax[i]), bins))
            theta = F(ol.compute_theta_ray(cam, sc.boxes[i]))
            assert R.same_class_or_bytes(np.array([alpha, theta]), np.array([ref.alpha[i], ref.theta_ray[i]])).all(), (sc.tag, i)
            loc, err = ol.calc_location_all(cam, ref.lwh[i].astype(np.float64), sc.boxes[i], alpha, theta)
            assert R.same_class_or_bytes(loc, ref.loc[i]).all(), (sc.tag, i, "loc")
            assert R.same_class_or_bytes(err, ref.err[i]).all(), (sc.tag, i, "err")
            n += 1
        want = ol.post_process(cam, sc.orient, sc.conf, sc.dims, sc.boxes)
        assert len(want) == len(ref.poses) and R.poses_equal(ref.poses, want).all(), (sc.tag, "poses")
    assert n > 700


def test_fp64_mode_against_numpy_lstsq():
    """well-conditioned boxes on the four cameras: all 64 solutions and residuals of the reference in the device's
    trig mode against numpy.linalg.lstsq (fp64) of the pinhole system, at the tolerances of
    test_oracle_second_opinions.test_calc_location_against_numpy_lstsq"""
    worst_loc, worst_err = 0.0, 0.0
    for ci in range(len(R.CAMS)):
        sc = R.random_scene(ci, 40, 30 + ci)
        ref = R.reference(sc)
        cam = R.cam_of(ci)
        checked = 0
        for i in range(len(sc.boxes)):
            if ref.rank[i] != 3 or ref.downdate[i] or not ref.valid[i]:
                continue
            fbox = [float(F(sc.boxes[i][k])) for k in ("x_min", "y_min", "x_max", "y_max")]
            for sid, corners in enumerate(_constraint_sets(ref.lwh[i], ref.alpha[i])):
                A, b = _pinhole_system(cam, fbox, corners, float(ref.orient[i]))
                if np.linalg.cond(A) > 1e3:
                    break
                sol, *_ = np.linalg.lstsq(A, b, rcond=None)
                res = float(np.sum((A @ sol - b) ** 2))
                scale = max(1.0, float(np.max(np.abs(sol))))
                worst_loc = max(worst_loc, float(np.max(np.abs(ref.loc[i, sid] - sol))) / scale)
                worst_err = max(worst_err, abs(float(ref.err[i, sid]) - res) / max(1.0, float(b @ b)))
            else:
                checked += 1
        assert checked >= 10, (ci, checked)
    assert worst_loc <= 1e-4, worst_loc
    assert worst_err <= 1e-5, worst_err


def test_winner_is_the_sequential_argmin():
    """the reference's winner against the loop it restates: err < best from FLT_MAX, in lane order"""
    for sc in R.all_scenes():
        ref = R.reference(sc)
        for i in range(len(sc.boxes)):
            best, who = R.FLT_MAX, 64
            for lane in range(64):
                if ref.err[i, lane] < best:
                    best, who = ref.err[i, lane], lane
            assert who == ref.winner[i], (sc.tag, i)
            assert ref.best_loc[i].tobytes() == (ref.loc[i, who] if who < 64 else np.zeros(3, F)).tobytes()


def test_canary_search_found_every_reachable_alpha():
    """computeAlpha returns fl(fl(atan2 + bin) - fl(pi)): a multiple of the sum's ulp.  -92, -90, -88 degrees and 0 are
    returned exactly, and so are both float32 neighbours of the three negative thresholds; next to 0 the sum's ulp is
    2^-22; +88, +90 and +92 degrees (the sum is in [4, 8), ulp 2^-21) lie off the lattice, so no input gives them: the
    targets there are the nearest returnable value on each side.  The search must find every target in every bin
    that can return it, and every target in at least one."""
    targets = R.reachable_alphas()
    for t in R.THRESHOLDS:
        tg = targets[t]
        assert tg[0] < t < tg[-1]
        if t < 0:
            assert tg == [np.nextafter(t, F(-9)), t, np.nextafter(t, F(9))]
        elif t == 0:
            assert tg == [F(-2.0 ** -22), F(0), F(2.0 ** -22)]
        else:   # off the lattice: no sum next to t + pi gives t, the neighbours are within 3 ulps
            assert len(tg) == 2 and all(abs(float(v) - float(t)) <= 3 * float(np.spacing(t)) for v in tg)
            s = F(np.float64(t) + np.float64(R.PI_F))
            assert F(s - R.PI_F) != t and not R.atan2_values_for(t, 0) and not R.atan2_values_for(t, 1)
            assert float(np.spacing(s)) == 4 * float(np.spacing(t))
    found, missing = R.canaries()
    assert not missing
    have = {(t, v, a) for t, v, a, _, _ in found}
    for t, tg in targets.items():
        for v in tg:
            bins = [a for a in (0, 1) if R.atan2_values_for(v, a)]
            assert bins and all((t, v, a) in have for a in bins), (t, v)
    for t, v, a, cv, sv in found:
        assert R.alpha_of(cv, sv, a) == v
    both = [(t, v) for t, tg in targets.items() for v in tg if (t, v, 0) in have and (t, v, 1) in have]
    assert len(both) >= 8      # the thresholds both bins can reach: -90 .. +90 degrees


def _census():
    rows = []
    for sc in R.all_scenes():
        ref = R.reference(sc)
        for i in range(len(sc.boxes)):
            rows.append((sc, ref, i))
    return rows


def test_fixture_conditions():
    """what the scenes are there for (conditions, not measurements)"""
    rows = _census()
    branches = {(int(r.branch[i]), int(r.switch_mult[i])) for _, r, i in rows}
    assert {b for b, _ in branches} == {0, 1, 2, 3} and {s for _, s in branches} == {1, -1}
    assert {(2, 1), (2, -1), (3, 1), (3, -1), (0, 1), (1, -1)} <= branches
    alphas = {float(r.alpha[i]) for sc, r, i in rows if sc.tag == "canaries"}
    for t, tg in R.reachable_alphas().items():
        assert all(float(v) in alphas for v in tg), t
    pivots = {tuple(int(v) for v in r.pivots[i]) for _, r, i in rows}
    assert pivots == {(0, 1, 2), (0, 2, 2), (1, 1, 2), (1, 2, 2), (2, 1, 2), (2, 2, 2)}
    assert any(r.rank[i] == 2 and r.nonzero[i] == 2 for _, r, i in rows)
    assert any(r.tail[i] for _, r, i in rows) and any(r.downdate[i] for _, r, i in rows)
    cam3 = R.reference(R.edge_scene(2))      # the third camera: the one-pixel box takes the down-date branch
    one_px = [i for i, b in enumerate(R.edge_scene(2).boxes) if (b["x_min"], b["y_min"], b["x_max"], b["y_max"]) == (320, 240, 321, 241)]
    assert one_px and all(cam3.downdate[i] for i in one_px)
    ties = {int(r.ties[i]) for _, r, i in rows}
    assert {4, 16, 64} <= ties
    assert any(np.isnan(r.err[i]).all() and r.winner[i] == 64 for _, r, i in rows)
    assert any(sc.conf[i][0] == sc.conf[i][1] and r.argmax[i] == 0 for sc, r, i in rows)
    half = F(R.IMG_W) / F(2)
    centres = {float(r.centre[i]) for sc, r, i in rows if sc.tag == "centre"}
    assert {float(half), float(np.nextafter(half, F(0)))} <= centres
    nf, good = R.nonfinite_scene()
    r = R.reference(nf)
    assert (r.lwh[:, 0] < 0).any() and np.isnan(r.lwh).any() and np.isinf(r.lwh).any()
    assert np.isnan(r.orient).any() and (np.abs(nf.boxes["x_max"] - nf.boxes["x_min"]) >= 1e6).sum() >= 3
    assert np.isfinite(r.err[good]).all() and (r.winner[good] < 64).all()
    # the call-site batch marks cells of the 50 m x 20 m map
    both = np.concatenate([R.reference(R.edge_scene(0)).poses, r.poses])
    tf = synth.transforms()["base_cam"]
    base = both.copy()
    for k, p in enumerate(both):
        o = ol.tf_pose(tf, [p[q] for q in ("px", "py", "pz", "qx", "qy", "qz", "qw")])
        for q, v in zip(("px", "py", "pz", "qx", "qy", "qz", "qw"), o):
            base[k][q] = v
    og = ol.OGrid(50, 20, 0.25)
    og.update_map_poses(base)
    assert np.count_nonzero(og.log_odds > 0) > 20


def test_trig_census():
    """where the device's contract (fp64 rounded once) and the oracle's float libm part: on the scenes, and per
    function over a seeded sample.  The figures of glibc 2.35 are in DESIGN's tolerances section; what holds for any
    correct libm is asserted: the float function is within one ulp of the rounded fp64 value."""
    rows = _census()
    d_alpha = d_theta = d_branch = d_winner = 0
    for sc in R.all_scenes():
        a, b = R.reference(sc), R.reference(sc, "libm")
        d_alpha += int((~R.same_class_or_bytes(a.alpha, b.alpha)).sum())
        d_theta += int((~R.same_class_or_bytes(a.theta_ray, b.theta_ray)).sum())
        d_branch += int((a.branch != b.branch).sum() + (a.switch_mult != b.switch_mult).sum())
        d_winner += int((a.winner != b.winner).sum())
    print(f"\n{platform.libc_ver()}: of {len(rows)} boxes alpha differs for {d_alpha}, theta_ray for {d_theta}, "
          f"the branch for {d_branch}, the winner for {d_winner}")
    rng = np.random.default_rng(1)
    n = 200_000
    x = rng.uniform(-7, 7, n).astype(F)
    ang = rng.uniform(-math.pi, math.pi, n)
    for name, args in (("atan2", (np.sin(ang).astype(F), np.cos(ang).astype(F))), ("atan", (x,)), ("tan", (x,)),
                       ("sin", (x,)), ("cos", (x,))):
        a, b = R.trig_fn(name, "fp64")(*args), R.trig_fn(name, "libm")(*args)
        diff = a != b
        print(f"  {name}f: {int(diff.sum())} of {n} differ from float(fp64 {name})")
        assert (np.abs(a.astype(np.float64) - b) <= np.spacing(np.abs(a))).all(), name
