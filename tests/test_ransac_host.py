"""CPU: tests/ransac_ref.py equals oracle/ransac.c byte for byte on every fixture of tests/ransac_cases.py, and every
fixture family reaches the edge it was built for -- so that tests/test_gpu_ransac.py, which holds the device to the same
reference on the same fixtures with no tolerance, can tell a wrong kernel from a right one.

No refined coefficient of any fixture lies within 2^-40 (relative) of a float32 rounding boundary: the only operations
where the device and glibc may differ are the fp64 atan2, cos and sin of the closed-form eigenvector, in the last bit;
they enter after the cancellation and move the eigenvalue by about 1e-16 of the matrix scale and the unit vector by as
much, four orders of magnitude below that margin."""
import time

import numpy as np
import pytest

import oracle_lib as ol
import pose_ref as P
import ransac_cases as RC
import ransac_ref as R

MARGIN = 2.0 ** -40


def _equals_oracle(case):
    r = RC.reference(case)
    em, emask, ecoeff = ol.segment_ground_plane(*RC.camera(case), case.thr, case.iters, case.seed)
    assert em == r.n_inliers, case.tag
    assert emask.tobytes() == r.mask.tobytes(), case.tag
    assert ecoeff.tobytes() == r.refined.tobytes(), (case.tag, ecoeff, r.refined)
    assert min(r.margin) > MARGIN, (case.tag, r.margin)
    assert r.best_count == r.m                      # the count pass and the moments pass evaluate one predicate
    assert r.counts.max() == r.best_count and (r.best_count == 0 or r.counts[r.best_index] == r.best_count)
    return r


def test_draws_and_transform_match_the_oracle():
    """the reference's own pieces: the transform against the oracle's, the tree sum against the C loop's definition"""
    rng = np.random.default_rng(1)
    x, y, z = (rng.uniform(-50, 50, 1000).astype(np.float32) for _ in range(3))
    for tf in (RC.IDENT_TF, RC.PERTURBED_TF):
        m = ol.tf_to_matrix4f(tf)
        for a, b in zip(R.xform34(m, x, y, z), ol.transform_cloud(m, x, y, z)):
            assert a.tobytes() == b.tobytes()
    for n in (1, 63, 64, 65, 4096, 4097, 262_145):
        v = rng.uniform(0, 1e6, n)
        t = v.copy()
        while True:   # tree_sum64 of oracle/ransac.c, one value at a time
            g = (len(t) + 63) // 64
            nxt = []
            for k in range(g):
                w = list(t[64 * k:64 * k + 64]) + [0.0] * (64 - len(t[64 * k:64 * k + 64]))
                off = 32
                while off:
                    for i in range(off):
                        w[i] = w[i] + w[i + off]
                    off >>= 1
                nxt.append(w[0])
            t = np.array(nxt)
            if g == 1:
                break
        assert R.tree_sum64(v) == t[0], n
    assert float(R.ceil_to_float(0.04)) > 0.04 > float(np.nextafter(R.ceil_to_float(0.04), np.float32(0)))
    assert float(R.ceil_to_float(0.3)) == float(np.float32(0.3)) > 0.3
    assert float(R.ceil_to_float(0.5)) == 0.5 and float(R.ceil_to_float(2.0 ** -140)) == 2.0 ** -140


@pytest.mark.parametrize("case", RC.threshold_cases(), ids=lambda c: c.tag)
def test_threshold_edge(case):
    """A: points exist at pred(thr_f), thr_f and succ(thr_f) in both signs; the sampled and the refined plane are z = 0
    exactly, so their distance IS |z|; the reference takes the first and leaves the other two"""
    r = _equals_oracle(case)
    thr_f, dist, edge = case.meta["thr_f"], case.meta["dist"], case.meta["edge"]
    assert float(dist["pred"]) < case.thr <= float(thr_f) < float(dist["succ"])
    assert float(np.nextafter(thr_f, np.float32(0))) < case.thr      # the SMALLEST float >= the threshold
    assert [abs(float(v)) for v in r.plane] == [0.0, 0.0, 1.0, 0.0] and [abs(float(v)) for v in r.refined] == [0.0, 0.0, 1.0, 0.0]
    cam = RC.camera(case)
    for key, ix in edge.items():
        assert len(ix) == 2 * RC.EDGE_PER and (np.abs(cam[2][ix]) == dist[key]).all()
        assert (cam[2][ix] > 0).sum() == (cam[2][ix] < 0).sum() == RC.EDGE_PER
        for pl in (r.plane, r.refined):
            assert (np.abs(R.distance(pl, *(a[ix] for a in cam))) == dist[key]).all()
        assert r.mask[ix].all() if key == "pred" else not r.mask[ix].any()
    on_plane = int((cam[2] == 0).sum())
    assert r.best_count == r.m == r.n_inliers == on_plane + 2 * RC.EDGE_PER
    # `<=` for `<` and a threshold rounded down would each move the counts
    assert (np.abs(cam[2]) <= thr_f).sum() == r.best_count + 2 * RC.EDGE_PER
    if float(np.float32(case.thr)) < case.thr:
        assert (np.abs(cam[2]) < np.float32(case.thr)).sum() == r.best_count - 2 * RC.EDGE_PER
    if case.tag.endswith("denormal"):
        assert 0 < float(dist["succ"]) < float(np.finfo(np.float32).tiny)


def test_rounding_sensitive():
    """B: with the multiply-adds fused the reference gives another best_count, another m, another n_inliers and another
    mask; the planted points are what they were built to be"""
    case = RC.rounding_case()
    r = _equals_oracle(case)
    assert len(case.x) >= 60_000 and (case.thr, case.iters, case.seed) == (0.04, 50, 12345)
    assert r.best_index == case.meta["winner"]
    cam, thr_f = RC.camera(case), R.ceil_to_float(case.thr)
    s, e = case.meta["sampled_edge"], case.meta["refined_edge"]
    assert len(s) >= 64 and len(e) >= 64 and not (set(s) | set(e)) & set(R.draws(len(case.x), 50, 12345).reshape(-1))
    pick = lambda ix: tuple(a[ix] for a in cam)
    assert R.inliers(r.plane, *pick(s), thr_f).all() and not R.inliers(r.plane, *pick(s), thr_f, contract=True).any()
    assert R.inliers(r.refined, *pick(e), thr_f).all() and not R.inliers(r.refined, *pick(e), thr_f, contract=True).any()
    assert not R.inliers(r.plane, *pick(e), thr_f).any() and not R.inliers(r.plane, *pick(e), thr_f, contract=True).any()
    c = RC.reference(case, contract=True)
    assert c.best_count != r.best_count and c.m != r.m and c.n_inliers != r.n_inliers
    assert c.mask.tobytes() != r.mask.tobytes()
    # the refined plane's points lie inside the image: without the ground test of k_pose_classify a box selects them
    assert (P.run(*cam, P.grid_boxes(4, 3)).ids[e] >= 0).sum() >= 64
    # one site alone: the mask pass fused and nothing else moves the mask on the refined plane's points
    assert (R.inliers(r.refined, *cam, thr_f, contract=True) != r.mask.astype(bool)).sum() >= 64


@pytest.mark.parametrize("case", RC.tie_cases(), ids=lambda c: c.tag)
def test_ties(case):
    """C: the winner ties with a later hypothesis on ANOTHER plane, in the lane / launch relation asked for"""
    r = _equals_oracle(case)
    cls, kind = case.meta["cls"], case.meta["kind"]
    hyp = RC.plane_hypotheses(case.x, case.y, cls, case.iters, case.seed)
    good = np.flatnonzero(hyp)
    assert (r.counts[good] == case.meta["per_plane"]).all() and r.best_count == case.meta["per_plane"]
    assert (np.delete(r.counts, good) < r.best_count).all()
    t1 = r.best_index
    assert t1 == good[0] >= 1
    if kind == "any":
        t2 = int(good[hyp[good] != hyp[t1]][0])
    else:
        assert RC.tie_relation(kind, hyp) is not None
        t1_, t2 = RC.tie_relation(kind, hyp)
        assert t1_ == t1
        if kind == "lane":
            assert t1 < t2 < 2048 and t1 % 64 > t2 % 64
        elif kind == "launch":
            assert t1 < 2048 <= t2
        else:
            assert 2048 <= t1 < t2 and t1 % 64 > t2 % 64 and not hyp[:2048].any()
    assert r.counts[t2] == r.counts[t1] and hyp[t2] != hyp[t1]
    # the winner shows: d, the refined d and the mask belong to t1's plane
    pz = RC.PLANE_Z[hyp[t1] - 1]
    assert abs(float(r.plane[3])) == pz and abs(float(r.refined[3])) == pz
    assert np.array_equal(r.mask.astype(bool), cls == hyp[t1])


@pytest.mark.parametrize("case", RC.degenerate_cases(), ids=lambda c: c.tag)
def test_degenerate(case):
    """D: no plane from collinear, identical, tiny and all-NaN clouds; non-finite points are drawn and never inliers"""
    r = _equals_oracle(case)
    cam = RC.camera(case)
    if case.meta.get("fails"):
        assert r.best_count == 0 and r.m == 0 and r.n_inliers == 0 and not r.mask.any() and not r.counts.any()
        assert r.plane.tobytes() == bytes(16) and r.refined.tobytes() == bytes(16)
        return
    bad = ~(np.isfinite(cam[0]) & np.isfinite(cam[1]) & np.isfinite(cam[2]))
    assert bad.sum() >= 30 and not r.mask[bad].any() and r.best_count > 2000
    if case.tag == "nonfinite":
        idx = R.draws(len(case.x), case.iters, case.seed)
        drawn_bad = bad[idx].any(axis=1)
        print(f"{int(drawn_bad.sum())} of {case.iters} hypotheses draw a non-finite point")
        assert drawn_bad.sum() >= 6 and not r.counts[drawn_bad].any() and not drawn_bad[r.best_index]
        for v in (np.nan, np.inf, -np.inf):
            col = np.stack([case.x, case.y, case.z])[:, idx.reshape(-1)]
            assert (np.isnan(col) if np.isnan(v) else col == v).any()
    else:
        planted = case.meta["planted"]
        assert len(planted) == 40 and np.isinf(case.x[planted]).all()
        assert (case.x[planted] > 0).sum() == (case.x[planted] < 0).sum() == 20
        # the transform's first column has no zero: the camera point is infinite in all three coordinates, NOT NaN ...
        assert all(np.isinf(a[planted]).all() for a in cam) and not np.isnan(np.stack(cam)).any()
        # ... and both planes are camera x = 8 with y and z components exactly zero: 0 * inf = NaN inside the evaluation
        for pl in (r.plane, r.refined):
            assert [abs(float(v)) for v in pl] == [1.0, 0.0, 0.0, RC.INF_X_PLANE]
            with np.errstate(all="ignore"):
                assert np.isnan(R.distance(pl, *(a[planted] for a in cam))).all()
        assert r.best_count == int((cam[0] == RC.INF_X_PLANE).sum()) >= 2900


def test_handle_sequence_cases():
    """the one-handle sequence alternates failing and good clouds and changes the iteration count"""
    seq = RC.handle_sequence()
    fails = [RC.reference(c).best_count == 0 for c in seq]
    assert fails == [True, False, True, False, False, True, False]
    assert [c.iters for c in seq if RC.reference(c).best_count] == [50, 4096, 7, 50]
    for c in seq:
        _equals_oracle(c)


@pytest.mark.parametrize("case", RC.sum_cases(), ids=lambda c: c.tag)
def test_sum_order(case):
    """E: sequential and exactly rounded sums give other float32 bytes than the tree"""
    r = _equals_oracle(case)
    n = len(case.x)
    assert r.best_count >= n // 2
    if case.tag in RC.SUM_INSENSITIVE:   # stated, not hidden: these three run on the device but prove nothing about order
        for how in ("sequential", "fsum"):
            assert RC.reference(case, sum=how).refined.tobytes() == r.refined.tobytes(), (case.tag, how)
        return
    for how in ("sequential", "fsum"):
        assert RC.reference(case, sum=how).refined.tobytes() != r.refined.tobytes(), (case.tag, how)


@pytest.mark.parametrize("case", RC.step_cases(), ids=lambda c: c.tag)
def test_butterfly_steps(case):
    """G: the cross-row steps of wave_butterfly swapped, and the four row steps of the level-0 sum reversed, give other
    float32 bytes than the tree -- each on the fixtures built for it, and between them on three tree shapes"""
    r = _equals_oracle(case)
    assert r.best_count >= len(case.x) // 2
    assert RC.reference(case, sum="steps").refined.tobytes() == r.refined.tobytes()      # the emulation IS the tree
    for how in case.meta["orders"]:
        assert RC.reference(case, sum=how).refined.tobytes() != r.refined.tobytes(), (case.tag, how)
    if "straddle" in case.tag:   # the inliers' far camera coordinate lies on both sides of 2^16
        cz = RC.camera(case)[2][r.mask.astype(bool)]
        assert cz.min() < 65536.0 < cz.max()


def test_butterfly_steps_cover_both_orders():
    seen = {how for c in RC.step_cases() for how in c.meta["orders"]}
    assert seen == {"rows-swapped", "dpp-reversed"}


def test_general_tree():
    """F: 4098 workgroups' worth of points, four tree levels; the other sum orders give other bytes"""
    t0 = time.time()
    case = RC.general_case()
    n = len(case.x)
    assert n == 4096 * 4096 + 4097 and case.iters <= 4
    levels = [(n + 4095) // 4096]
    while levels[-1] > 1:
        levels.append((levels[-1] + 63) // 64)
    assert levels == [4098, 65, 2, 1]
    r = _equals_oracle(case)
    assert r.best_count > n // 3      # millions of inliers in every workgroup
    for how in ("sequential", "fsum"):
        assert RC.reference(case, sum=how).refined.tobytes() != r.refined.tobytes(), how
    print(f"general tree fixture: {time.time() - t0:.1f} s")   # measured here: see DESIGN.md
