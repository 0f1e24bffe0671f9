"""buildKDTree + computeDepthForBoundingBoxes (src/cloud_detections.cpp:8-33, 43-87) in plain numpy, and the scenes
the kNN tests run.  It does not call the oracle: the oracle keeps its neighbours by an insertion loop, the device by a
selection network, this file by one full lexicographic sort on (distance, index) -- and it returns the indices.

  project()    :13-33   skip z <= 0 exactly as written (NaN passes), fp64 row products (K0*x + K1*y) + K2*z, one fp64
                        divide, narrowed once to fp32; ORIGINAL point indices are kept
  centre()     :57-58   x_min + ((x_max - x_min) / 2.0f) in fp64, narrowed once
  rank()       FLANN L2_Simple in fp32, ((du*du) + dv*dv) + dz*dz, nothing fused; NaN distances dropped; sorted on
                        (distance, index).  tie="higher" sorts on (distance, -index): it exists ONLY so that fixtures
                        can prove they are sensitive to the tie rule
  knn_depth()  :64-81   the element at position cnt // 2 of the sorted neighbour depths, -1 with no candidate

scan_model() is something else: a model of how TODAY's stage-1 kernel walks a cloud (32 chunks, 4 wavefronts, a
128-entry buffer merged 64 at a time).  No expected value comes from it.  It only tells a fixture whether it reaches
the branch it was built for (the buffer's overflow half), so that a generator which stops doing so fails on the CPU.

TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

from gvamd.synth import BBOX_DTYPE

F32 = np.float32
FLT_MAX = np.finfo(F32).max
FLT_MIN = np.finfo(F32).tiny
DENORM_MIN = F32(1.401298464324817e-45)
# the camera of gvamd.synth (fx = fy = cx = 320, cy = 240), row major as gv_get_intrinsics returns it
K_SYNTH = np.array([320.0, 0.0, 320.0, 0.0, 320.0, 240.0, 0.0, 0.0, 1.0])
IDENT_TF = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])   # (qx, qy, qz, qw, tx, ty, tz)
STATIC_LABEL = 5   # a traffic light: gv_filter_bboxes keeps it static
ALL_K = tuple(range(1, 33))


# ------------------------------------------------------------------------------------------------ reference --

def project(K, cx, cy, cz):
    """camera-frame cloud -> (u, v, depth, original index) of the points buildKDTree keeps"""
    cx, cy, cz = (np.ascontiguousarray(a, F32) for a in (cx, cy, cz))
    K = np.asarray(K, np.float64).reshape(9)
    idx = np.flatnonzero(~(cz <= 0))                      # :16, a NaN z is not <= 0
    X, Y, Z = (a[idx].astype(np.float64) for a in (cx, cy, cz))
    with np.errstate(all="ignore"):
        ix = (K[0] * X + K[1] * Y) + K[2] * Z             # :19-20
        iy = (K[3] * X + K[4] * Y) + K[5] * Z
        iz = (K[6] * X + K[7] * Y) + K[8] * Z
        u = (ix / iz).astype(F32)                         # :23
        v = (iy / iz).astype(F32)                         # :24
    return u, v, cz[idx].copy(), idx.astype(np.int64)


def centre(lo, hi):
    """:57 the box fields are doubles, 2.0f is widened, pcl::PointXYZ::x is a float"""
    lo, hi = np.float64(lo), np.float64(hi)
    with np.errstate(all="ignore"):
        return F32(lo + ((hi - lo) / np.float64(F32(2.0))))


def distances(u, v, d, box):
    """fp32 squared distance of every projected point to the box's centre (cx, cy, 0)"""
    qx, qy, qz = centre(box["x_min"], box["x_max"]), centre(box["y_min"], box["y_max"]), F32(0.0)
    with np.errstate(all="ignore"):
        t = u - qx
        r = t * t
        t = v - qy
        r = r + t * t
        t = d - qz
        r = r + t * t
    assert r.dtype == F32
    return r


def rank(u, v, d, idx, box, tie="lower"):
    """every candidate of one box as (distance, depth, index), sorted on (distance, index)"""
    assert tie in ("lower", "higher")
    r = distances(u, v, d, box)
    ok = ~np.isnan(r)
    r, dd, ii = r[ok], d[ok], idx[ok]
    order = np.lexsort((ii if tie == "lower" else -ii, r))   # the last key is the primary one
    return r[order], dd[order], ii[order]


def knn_depth(K, cx, cy, cz, boxes, ks, tie="lower"):
    """{k: (depths[nb], knn_d2[nb, k] filled with inf, indices[nb, k] filled with -1)}; one sort per box serves every k"""
    ks = [ks] if np.isscalar(ks) else list(ks)
    boxes = np.ascontiguousarray(boxes, BBOX_DTYPE)
    u, v, d, idx = project(K, cx, cy, cz)
    out = {k: (np.full(len(boxes), -1.0, F32), np.full((len(boxes), k), np.inf, F32),
               np.full((len(boxes), k), -1, np.int64)) for k in ks}
    for b, box in enumerate(boxes):
        r, dd, ii = rank(u, v, d, idx, box, tie)
        for k in ks:
            cnt = min(k, len(r))
            if cnt:
                out[k][0][b] = np.sort(dd[:cnt])[cnt // 2]   # :78-81
                out[k][1][b, :cnt] = r[:cnt]
                out[k][2][b, :cnt] = ii[:cnt]
    return out


def kth_place_tie(K, cx, cy, cz, boxes, ks):
    """{k: bool[nb]}: the k-th and the (k+1)-th distance are equal"""
    u, v, d, idx = project(K, cx, cy, cz)
    out = {k: np.zeros(len(boxes), bool) for k in ks}
    for b, box in enumerate(np.ascontiguousarray(boxes, BBOX_DTYPE)):
        r = rank(u, v, d, idx, box)[0]
        for k in ks:
            out[k][b] = len(r) > k and r[k - 1] == r[k]
    return out


# ---------------------------------------------------------------------- today's stage 1, for fixture conditions --

CHUNKS, WAVES, LANES, BATCH, BUF = 32, 4, 64, 4, 128   # gv_knn_pca.hip: knn_chunks(), kKnnWaves, wave64, kBatch, kKnnBuf


def chunk_len(n):
    return (n + CHUNKS - 1) // CHUNKS


def scan_model(K, cx, cy, cz, box, k, move_rest=True):
    """Walks the cloud as k_knn_stage1 does today and merges the 128 lists as stage 2 does.  Returns
    (keys, max_fill, over): the final (distance, index) pairs, the fullest any buffer was when a merge began, and how
    many entries waited in a buffer's second half.  move_rest=False leaves the second half where it is -- the mistake
    the overflow fixtures are built to expose; a fixture proves its worth when that changes `keys`."""
    cz = np.ascontiguousarray(cz, F32)
    n = len(cz)
    u, v, d, idx = project(K, cx, cy, cz)
    r_all = np.full(n, np.nan, F32)
    r_all[idx] = distances(u, v, d, box)
    per = chunk_len(n)
    lists, max_fill, over = [], 0, 0
    lane = np.arange(LANES)
    for c in range(CHUNKS):
        lo, hi = c * per, min(n, (c + 1) * per)
        for w in range(WAVES):
            top = np.zeros((0, 2))          # (distance, index) rows, sorted
            thresh = np.inf
            buf = np.zeros((BUF + LANES, 2))
            nbuf = 0
            base = lo
            while base < hi or nbuf:
                if base < hi:
                    steps = [base + w * LANES + lane + q * WAVES * LANES for q in range(BATCH)]
                    base += WAVES * LANES * BATCH
                else:
                    steps = [None]          # the drain after the scan: while (nbuf) merge()
                for i in steps:
                    if i is not None:
                        i = i[i < hi]
                        with np.errstate(invalid="ignore"):
                            i = i[r_all[i] <= thresh]
                        if not len(i):
                            continue
                        buf[nbuf:nbuf + len(i), 0], buf[nbuf:nbuf + len(i), 1] = r_all[i], i
                        nbuf += len(i)
                        if nbuf < LANES:
                            continue
                    elif not nbuf:
                        continue
                    take = min(nbuf, LANES)
                    max_fill = max(max_fill, nbuf)
                    over += nbuf - take
                    both = np.concatenate([top, buf[:take]])
                    if move_rest:
                        buf[:nbuf - take] = buf[take:nbuf].copy()
                    nbuf -= take
                    both = both[np.lexsort((both[:, 1], both[:, 0]))]
                    top = both[:k]
                    thresh = top[k - 1, 0] if len(top) == k else np.inf
            lists.append(top)
    allk = np.concatenate(lists)
    allk = allk[np.lexsort((allk[:, 1], allk[:, 0]))][:k]
    return allk, max_fill, over


# ---------------------------------------------------------------------------------------------------- scenes --

class Case:
    """one cloud (as uploaded; cam_lidar is the identity), its boxes and the k values it is run with"""

    def __init__(self, tag, x, y, z, boxes, ks, **meta):
        self.tag, self.ks, self.meta = tag, tuple(ks), meta
        self.x, self.y, self.z = (np.ascontiguousarray(a, F32) for a in (x, y, z))
        self.boxes = np.ascontiguousarray(boxes, BBOX_DTYPE)

    def permuted(self, tag, p, **meta):
        return Case(tag, self.x[p], self.y[p], self.z[p], self.boxes, self.ks, **{**self.meta, **meta})


def make_boxes(rows):
    """(x_min, y_min, x_max, y_max) rows -> static boxes"""
    b = np.zeros(len(rows), BBOX_DTYPE)
    for i, (x0, y0, x1, y1) in enumerate(rows):
        b[i] = (x0, y0, x1, y1, max(0.99 - 0.001 * i, 0.5), STATIC_LABEL)
    return b


def lattice_xyz(j, i, m):
    """Z = 5m, X = jZ/64, Y = iZ/64, all exact in fp32: with K_SYNTH the point projects to exactly
    u = 5j + 320, v = 5i + 240, depth 5m"""
    z = (5 * np.asarray(m)).astype(F32)
    x = np.asarray(j).astype(F32) * z / F32(64)
    y = np.asarray(i).astype(F32) * z / F32(64)
    return x, y, z


def lattice_boxes(j0, i0, hw, hh):
    """boxes centred on the lattice pixel (5 j0 + 320, 5 i0 + 240): squared distances are 25 (j'^2 + i'^2 + m^2)"""
    j0, i0, hw, hh = (np.asarray(a, np.float64) for a in (j0, i0, hw, hh))
    cu, cv = 5 * j0 + 320, 5 * i0 + 240
    return make_boxes(list(zip(cu - hw, cv - hh, cu + hw, cv + hh)))


def _lattice_draw(rng, n):
    return rng.integers(-60, 61, n), rng.integers(-44, 45, n), rng.integers(1, 13, n)


def lattice_cases(seeds=(1, 2, 3, 4), n=20_000, nb=50):
    """3(a): random lattice clouds, lattice-centred boxes, every k"""
    for seed in seeds:
        rng = np.random.default_rng(1000 + seed)
        j, i, m = _lattice_draw(rng, n)
        boxes = lattice_boxes(rng.integers(-40, 41, nb), rng.integers(-30, 31, nb), rng.integers(1, 40, nb),
                              rng.integers(1, 40, nb))
        yield Case(f"lattice-s{seed}", *lattice_xyz(j, i, m), boxes, ALL_K, jim=(j, i, m))


SHELL = 1154   # j^2 + i^2 + m^2 of the pure shell: 128 lattice points, 9 depths (|j|, |i| <= 40, m in 1..12)


def shell_jim():
    g = np.arange(-40, 41)
    j, i, m = np.meshgrid(g, g, np.arange(1, 13), indexing="ij")
    on = (j * j + i * i + m * m) == SHELL
    return j[on], i[on], m[on]


def _far_lattice(rng, n, beyond):
    """n random lattice points farther than `beyond` from the query at j = i = 0"""
    j, i, m = _lattice_draw(rng, 4 * n + 1000)
    far = (j * j + i * i + m * m) > beyond
    assert far.sum() >= n
    return j[far][:n], i[far][:n], m[far][:n]


def shell_cases(seeds=(1, 2, 3, 4), reps=(1, 3), n_far=20_000):
    """3(a) pure shell: the nearest points are one whole shell, each repeated r times in a shuffled order among
    farther points: the top-k is decided by index alone"""
    sj, si, sm = shell_jim()
    for seed in seeds:
        for r in reps:
            rng = np.random.default_rng(2000 + 10 * seed + r)
            fj, fi, fm = _far_lattice(rng, n_far, SHELL)
            j, i, m = (np.concatenate([np.tile(a, r), b]) for a, b in ((sj, fj), (si, fi), (sm, fm)))
            p = rng.permutation(len(j))
            yield Case(f"shell-s{seed}-r{r}", *lattice_xyz(j[p], i[p], m[p]), lattice_boxes([0], [0], [7], [9]), ALL_K,
                       seed=seed, rep=r)


def smooth_cloud(rng, n, behind=0.1):
    """a cloud in front of the camera with a share of points behind it (z <= 0: never projected)"""
    z = rng.uniform(2.0, 60.0, n)
    x = rng.uniform(-1.0, 1.0, n) * z
    y = rng.uniform(-0.75, 0.75, n) * z
    back = rng.random(n) < behind
    z[back] = -z[back]
    return x.astype(F32), y.astype(F32), z.astype(F32)


SCAN_BOXES = [(100.25, 80.5, 230.75, 201.0), (300.0, 200.0, 340.0, 280.0), (0.0, 0.0, 639.0, 479.0),
              (500.5, 10.25, 630.125, 90.0), (17.0, 333.0, 19.0, 470.0)]
SCAN_KS = (1, 7, 31, 32)


def scan_base(seed=5, n=64_000, target=60_011):
    """3(b) the one cloud, thinned until no two points are equally far from box 0 (a descending order then makes
    EVERY point beat all earlier ones); about 60,000 points are left, a tenth of them behind the camera"""
    rng = np.random.default_rng(seed)
    x, y, z = smooth_cloud(rng, n)
    boxes = make_boxes(SCAN_BOXES)
    u, v, d, idx = project(K_SYNTH, x, y, z)
    r = distances(u, v, d, boxes[0])
    _, first = np.unique(r, return_index=True)
    keep = np.ones(n, bool)
    keep[idx] = False
    keep[idx[first]] = True
    assert keep.sum() >= target
    keep[np.flatnonzero(keep)[target:]] = False   # 60,011: an odd size, the last chunk is shorter than the others
    return Case("scan-base", x[keep], y[keep], z[keep], boxes, SCAN_KS)


def _place(n, winners, positions, rng):
    """a permutation p (new[t] = old[p[t]]) that puts winners[t] at positions[t] and shuffles the rest around them"""
    winners, positions = np.asarray(winners), np.asarray(positions)
    assert len(winners) == len(positions) == len(set(positions.tolist())) and positions.min() >= 0 and positions.max() < n
    p = np.full(n, -1, np.int64)
    p[positions] = winners
    rest = np.setdiff1d(np.arange(n), winners)
    p[p < 0] = rng.permutation(rest)
    assert np.array_equal(np.sort(p), np.arange(n))
    return p


def scan_cases(base=None):
    """3(b): the base cloud permuted into the orders that defeat the threshold.  The placements aim at TODAY's
    decomposition (32 chunks of ceil(n/32) points, 4 wavefronts, lane i takes base + tid + q*256); expected values come
    from the reference on the permuted cloud and nothing asserted depends on the decomposition."""
    base = base or scan_base()
    n = len(base.x)
    per = chunk_len(n)
    u, v, d, idx = project(K_SYNTH, base.x, base.y, base.z)
    order = rank(u, v, d, idx, base.boxes[0])[2]              # the projected points, nearest first
    slots = np.sort(order)                                    # the points behind the camera keep their places
    for name, seq in (("ascending", order), ("descending", order[::-1])):
        p = np.arange(n)
        p[slots] = seq
        yield base.permuted(f"scan-{name}", p, order=name)
    rng = np.random.default_rng(77)
    yield base.permuted("scan-shuffle", rng.permutation(n), order="shuffle")
    for k in SCAN_KS:
        near = order[:k]
        edges = np.array([c * per + e for c in range(1, CHUNKS) for e in (-1, 0, 1)])
        strides = np.unique([c * per + s * st + e for c in (0, 13, CHUNKS - 1) for st in (64, 256) for s in range(1, 8)
                             for e in (-1, 0) if s * st + e < min(per, n - c * per)])
        lists = np.array([((t * 5) % CHUNKS) * per + (t % WAVES) * LANES + int(rng.integers(0, LANES))
                          + 256 * int(rng.integers(0, BATCH)) for t in range(k)])   # one per (chunk, wavefront) list
        for name, pos in (("first64", rng.choice(64, k, replace=False)), ("last", np.arange(n - k, n)),
                          ("chunk-edges", rng.choice(edges, k, replace=False)),
                          ("strides", rng.choice(strides, k, replace=False)), ("one-per-list", lists)):
            c = base.permuted(f"scan-{name}-k{k}", _place(n, near, pos, rng), order=name)
            c.ks = (k,)
            yield c


RUNS = (129, 64, 65, 127, 128, 256, 5000)
RUN_KS = (1, 7, 31, 32)


def overflow_case(run, depths, n=200_000, seed=9, ks=RUN_KS):
    """3(c): `run` points of equal, winning distance at consecutive indices inside one chunk, starting in the middle of a
    wavefront's 64 indices.  A few points that beat the background but not the run come just before it in every
    wavefront's slice, so each buffer already holds something when 64 of the run arrive at once.
    depths = "equal": one point repeated; "shell": the pure shell's points in turn, so the depths differ; "ramp" is not
    a run of equal distance but of strictly falling distance (one lattice point per sum of squares below the shell):
    there the entries that wait in the second half are the winners."""
    rng = np.random.default_rng(seed + run)
    per = chunk_len(n)
    start = 3 * per + 1024 + 37
    assert run <= per - 1024 - 37 and depths in ("equal", "shell", "ramp")
    j, i, m = _far_lattice(rng, n, 2500)
    if depths == "equal":
        rj, ri, rm = np.full(run, 3), np.full(run, 4), np.full(run, 5)
    elif depths == "shell":
        sj, si, sm = shell_jim()
        t = rng.permutation(len(sj))[np.arange(run) % len(sj)]
        rj, ri, rm = sj[t], si[t], sm[t]
    else:
        g = np.arange(-33, 34)
        aj, ai, am = (a.reshape(-1) for a in np.meshgrid(g, g, np.arange(1, 13), indexing="ij"))
        t = rng.permutation(len(aj))
        aj, ai, am = aj[t], ai[t], am[t]
        ss, first = np.unique(aj * aj + ai * ai + am * am, return_index=True)
        first = first[ss < SHELL][::-1][:run]              # the largest sums below the shell, falling
        assert len(first) == run
        rj, ri, rm = aj[first], ai[first], am[first]
    j[start:start + run], i[start:start + run], m[start:start + run] = rj, ri, rm
    # the primers: between the shell and the background, nearer and nearer, ten per wavefront in the last 256 indices
    # before the block the run starts in
    pj = np.arange(49, 35, -1)[:10]                       # 25 * (j^2 + 0 + 1): 2402 .. 1601 > 1154
    for w in range(WAVES):
        s = 3 * per + 768 + w * LANES
        j[s:s + 10], i[s:s + 10], m[s:s + 10] = pj, 0, 1
    return Case(f"overflow-{depths}-{run}", *lattice_xyz(j, i, m), lattice_boxes([0], [0], [3], [5]), ks,
                run=(start, start + run))


def overflow_cases(n=200_000, runs=RUNS):
    for depths in ("equal", "shell"):
        for run in runs:
            yield overflow_case(run, depths, n)
    for run in (129, 256):
        yield overflow_case(run, "ramp", n)


RAGGED_N = (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1025, 4095, 4097, 8191, 8193, 32767,
            32769)
RAGGED_KS = (1, 2, 3, 16, 31, 32)
RAGGED_BOXES = [(300.0, 200.0, 340.0, 280.0), (10.5, 20.25, 90.0, 77.0), (400.0, 100.0, 639.0, 479.0)]


def ragged_cases(n):
    """3(d): n points, all in front of the camera; then only c of them, scattered over the chunks, c running over
    {0, 1, 2, k-1, k, k+1} of every k: cnt < k with both parities, -1 and inf fills"""
    rng = np.random.default_rng(4000 + n)
    boxes = make_boxes(RAGGED_BOXES)
    x, y, z = smooth_cloud(rng, n, behind=0.0)
    yield Case(f"ragged-n{n}-all", x, y, z, boxes, RAGGED_KS)
    for c in sorted({c for k in RAGGED_KS for c in (0, 1, 2, k - 1, k, k + 1) if c <= n}):
        zz = -z
        zz[rng.choice(n, c, replace=False)] *= -1
        back = np.flatnonzero(zz < 0)
        zz[back[0::3]] = 0.0                               # behind the camera as -z, +0.0 and -0.0
        zz[back[1::3]] = -0.0
        yield Case(f"ragged-n{n}-front{c}", x, y, zz, boxes, RAGGED_KS, front=c)


MEDIAN_PATTERNS = ("repeated", "equal", "increasing", "decreasing")


def median_cases():
    """3(e): the t-th nearest point of the box at (320, 240) has a chosen depth: du = 1 + 3t pixels decides the order
    (its square grows by at least 15 per step, no depth step here moves the sum by more than 5.25).  Once as the whole
    cloud with k = 32 (cnt < k), once with k = cnt among 40 farther points."""
    box = make_boxes([(300.0, 200.0, 340.0, 280.0)])
    for cnt in range(1, 33):
        t = np.arange(cnt)
        for pat in MEDIAN_PATTERNS:
            dep = {"repeated": 2.0 + ((t * 7) % 3) * 0.5, "equal": np.full(cnt, 2.5), "increasing": 2.0 + 0.01 * t,
                   "decreasing": 3.0 - 0.01 * t}[pat].astype(F32)
            x = ((1.0 + 3.0 * t) * dep / 320.0).astype(F32)
            y = np.zeros(cnt, F32)
            yield Case(f"median-{pat}-cnt{cnt}-alone", x, y, dep, box, (32,), cnt=cnt, pattern=pat)
            fz = np.full(40, 4.0, F32)
            fx = ((150.0 + np.arange(40)) * 4.0 / 320.0).astype(F32)
            p = np.random.default_rng(cnt).permutation(cnt + 40)
            near = np.argsort(p)[:cnt]                     # where the near points went, nearest first
            yield Case(f"median-{pat}-cnt{cnt}-among", np.concatenate([x, fx])[p], np.zeros(cnt + 40, F32),
                       np.concatenate([dep, fz])[p], box, (cnt,), cnt=cnt, pattern=pat, near=near)


NONFINITE_BOXES = [
    (300.0, 200.0, 340.0, 280.0),
    (np.nan, 200.0, 340.0, 280.0), (300.0, 200.0, 340.0, np.nan),          # a NaN bound: every distance is NaN
    (300.0, 200.0, np.inf, 280.0), (300.0, 200.0, 340.0, -np.inf),         # the centre is +-inf: every distance is +inf
    (np.inf, 200.0, np.inf, 280.0), (300.0, -np.inf, 340.0, 280.0),        # inf - inf, -inf + inf: a NaN centre
    (0.0, 0.0, 1e300, 1e300),                                                # finite in fp64, inf once narrowed
    (340.0, 280.0, 300.0, 200.0),                                            # x_max < x_min, y_max < y_min
    (1.0e6, 2.0e6, 1.0e6 + 50, 2.0e6 + 50), (-5000.0, -700.0, -4000.0, -650.0),   # far outside, and negative
    (100.0000001, 50.1, 300.3333333, 70.7000001), (0.1, 0.2, 0.7000001, 0.9),      # the fp64 centre is no fp32 value
    (16777216.0, 0.0, 16777219.0, 3.0),                                      # 16777217.5 rounds once, to even
]


def special_points():
    """3(f): (x, y, z) rows"""
    big = F32(3.0e38)
    rows = [(0.5, 0.25, 0.0), (0.5, 0.25, -0.0), (0.0, 0.0, DENORM_MIN), (DENORM_MIN, 0.0, DENORM_MIN),
            (0.0, 0.0, FLT_MIN), (FLT_MIN, -FLT_MIN, FLT_MIN), (1e-30, 2e-30, 1e-30), (0.0, 1e-31, 1e-30),
            (1e-3, 0.0, DENORM_MIN)]                                         # u overflows through a subnormal z
    for bad in (np.nan, np.inf, -np.inf):
        rows += [(bad, 0.5, 5.0), (0.5, bad, 5.0), (0.5, 0.25, bad)]
    rows += [(big, 0.0, 1.0), (-big, 0.0, 2.0), (0.0, big, 3.0), (big, -big, 4.0),          # u or v overflow: d2 = +inf
             (FLT_MAX, FLT_MAX, FLT_MAX), (FLT_MAX, 0.0, 1.0), (0.0, 0.0, FLT_MAX), (-FLT_MAX, FLT_MAX, 2.0),
             (1.0e19, 0.0, 1.0e19), (0.0, 0.0, 1.9e19)]                     # dz * dz overflows
    return np.array(rows, dtype=F32)


def nonfinite_cases():
    """3(f): the special points among 2,000 lattice points (lattice boxes are added to the special ones), then alone,
    then the 9-point cloud of 3 finite-distance and 6 inf-distance candidates whose median takes the latter in"""
    rng = np.random.default_rng(6)
    sp = special_points()
    boxes = np.concatenate([make_boxes(NONFINITE_BOXES), lattice_boxes([0, -7, 12], [0, 5, -9], [4, 9, 2], [6, 3, 8])])
    j, i, m = _lattice_draw(rng, 2000)
    x, y, z = lattice_xyz(j, i, m)
    at = np.sort(rng.choice(2000, len(sp), replace=False))
    x, y, z = (np.insert(a, at, sp[:, c]) for c, a in enumerate((x, y, z)))
    yield Case("nonfinite-sprinkled", x, y, z, boxes, ALL_K)
    yield Case("nonfinite-alone", sp[:, 0], sp[:, 1], sp[:, 2], boxes, ALL_K)
    big = F32(3.0e38)
    nine = np.array([(big, 0.0, 7.0), (0.1, 0.1, 3.0), (-big, 0.0, 9.0), (0.0, big, 1.0), (0.2, -0.1, 4.0),
                     (0.0, -big, 8.0), (big, big, 2.0), (-0.3, 0.2, 5.0), (FLT_MAX, 0.0, 6.0)], dtype=F32)
    yield Case("nonfinite-nine", nine[:, 0], nine[:, 1], nine[:, 2], boxes, ALL_K, n_finite=3, n_inf=6)


SCALE_KS = (10, 32)


def scale_cases(n=1_000_000):
    """3(h): the descending order and the 5,000-point run at a million points"""
    base = scan_base(seed=15, n=n + n // 8, target=n)
    u, v, d, idx = project(K_SYNTH, base.x, base.y, base.z)
    order = rank(u, v, d, idx, base.boxes[0])[2]
    p = np.arange(len(base.x))
    p[np.sort(order)] = order[::-1]
    c = base.permuted("scale-descending", p, order="descending")
    c.ks = SCALE_KS
    yield c
    yield overflow_case(5000, "shell", n=n, ks=SCALE_KS)


def tick_cases():
    """3(g): one tie scene and one overflow scene"""
    yield next(lattice_cases(seeds=(5,), nb=24))
    yield overflow_case(129, "shell")


# ----------------------------------------------------------------------------------------- fixture conditions --

def tie_stats(case, cam=None):
    """what a tie scene is worth, from this reference alone.  Returns (lower, higher, kth): knn_depth under either tie
    rule and kth_place_tie.  cam: the camera-frame cloud (default: the cloud as uploaded, identity transform)"""
    cam = cam or (case.x, case.y, case.z)
    return (knn_depth(K_SYNTH, *cam, case.boxes, case.ks), knn_depth(K_SYNTH, *cam, case.boxes, case.ks, tie="higher"),
            kth_place_tie(K_SYNTH, *cam, case.boxes, case.ks))
