"""Plain reference of the vision-orientation post-process (postProcessOutputs -> computeAlpha / computeThetaRay /
calcLocation, src/vision_orientation.cpp:241-519) as the device runs it: k_vision and qr_solve_4x3 of
grid-vision_amd/csrc/gv_detections.hip, reached through gv_vision_post_process, GV_FRAME_VISION_ORIENT and
GV_TICK_VISION_ORIENT.  Test infrastructure only.

Every multiply, add, subtract, divide and square root is one np.float32 operation on arrays of shape (boxes, 64), in
the operation order of the kernel and of oracle/vision_orientation.c; the promotions to double are where the oracle's
notes put them (the box centre, the halved dimensions, the constants 2 pi / bins, pi and 88 / 90 / 92 degrees).  The
branches of the restated column-pivoted Householder QR are masks.  Nothing here is fused and nothing is reassociated.

The six trig evaluations -- atan2 for alpha, atan for fovx, tan, atan for theta_ray, cos and sin of the orientation --
are a parameter:
  trig="fp64"  evaluated in fp64 by the host libm and rounded once to fp32: the DEVICE's contract
  trig="libm"  the host libm's float functions, which is what the oracle calls
(glibc's float functions are not the rounded fp64 value for 1 - 16 % of the arguments: DESIGN, Tolerances.)

Besides the reference this module holds the scenes that tests/test_vision_host.py pins to the oracle and checks for
their conditions and that tests/test_gpu_vision.py runs on the device."""
from __future__ import annotations

import ctypes
import ctypes.util
import math
from types import SimpleNamespace

import numpy as np

from gvamd.synth import BBOX_DTYPE, LSHAPE_DTYPE

F = np.float32
FLT_MAX = np.finfo(np.float32).max
FLT_MIN = np.finfo(np.float32).tiny
EPS = np.finfo(np.float32).eps
PI_F = F(math.pi)
DEG88, DEG90, DEG92 = (F(a * math.pi / 180.0) for a in (88, 90, 92))   # int * double / float: fp64, narrowed once
THRESHOLDS = (-DEG92, -DEG90, -DEG88, F(0), DEG88, DEG90, DEG92)
CLASS_DIMS = {9: (3.884, 1.629, 1.526), 0: (1.763, 0.597, 1.737), 1: (2.2, 0.8, 1.5), 2: (0.842, 0.660, 1.761)}
BRANCHES = {0: (1, 1), 1: (-1, -1), 2: (-1, 1), 3: (1, -1)}   # (left_mult, right_mult) in the kernel's if / else order

_m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("cos", "sin", "tan", "atan"):
    getattr(_m, _n).restype, getattr(_m, _n).argtypes = ctypes.c_double, [ctypes.c_double]
    getattr(_m, _n + "f").restype, getattr(_m, _n + "f").argtypes = ctypes.c_float, [ctypes.c_float]
_m.atan2.restype, _m.atan2.argtypes = ctypes.c_double, [ctypes.c_double, ctypes.c_double]
_m.atan2f.restype, _m.atan2f.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]


def trig_fn(name, mode):
    """elementwise float32 -> float32: name in atan2 / atan / tan / cos / sin"""
    if mode not in ("fp64", "libm"):
        raise ValueError(mode)
    f = getattr(_m, name if mode == "fp64" else name + "f")

    def run(*args):
        args = np.broadcast_arrays(*[np.asarray(a, F) for a in args])
        out = np.empty(args[0].shape, F)
        flat = out.reshape(-1)
        cols = [a.reshape(-1).tolist() for a in args]
        for i, v in enumerate(zip(*cols)):
            flat[i] = f(*v)     # fp64: the double result, rounded once by the store
        return out
    return run


def _qr_solve(A, b):
    """Eigen::ColPivHouseholderQR<Matrix<float, 4, 3>>::solve as the kernel restates it.  A[4][3], b[4]: float32 arrays
    of one shape.  Returns x[3] and the branch census of every element."""
    a = [[np.array(A[i][j], F) for j in range(3)] for i in range(4)]
    c = [np.array(b[i], F) for i in range(4)]
    shape = c[0].shape
    zero = np.zeros(shape, F)
    ncu = []
    for j in range(3):
        s = zero
        for i in range(4):
            s = s + a[i][j] * a[i][j]
        ncu.append(np.sqrt(s))
    ncd = [v.copy() for v in ncu]
    maxn = zero
    for j in range(3):
        maxn = np.where(ncu[j] > maxn, ncu[j], maxn)
    th = (maxn * EPS) / F(4)
    threshold_helper = th * th
    downdate_thr = np.sqrt(EPS)
    nonzero = np.full(shape, 3)
    maxpivot = zero
    transp, hc = [], []
    tail_taken, downdated = np.zeros(shape, bool), np.zeros(shape, bool)
    for k in range(3):
        big, bigv = np.full(shape, k), ncu[k]
        for j in range(k + 1, 3):
            m = ncu[j] > bigv
            bigv, big = np.where(m, ncu[j], bigv), np.where(m, j, big)
        big_sq = bigv * bigv
        nonzero = np.where((nonzero == 3) & (big_sq < threshold_helper * F(4 - k)), k, nonzero)
        transp.append(big)
        for j in range(k + 1, 3):
            m = big == j
            for i in range(4):
                a[i][k], a[i][j] = np.where(m, a[i][j], a[i][k]), np.where(m, a[i][k], a[i][j])
            ncu[k], ncu[j] = np.where(m, ncu[j], ncu[k]), np.where(m, ncu[k], ncu[j])
            ncd[k], ncd[j] = np.where(m, ncd[j], ncd[k]), np.where(m, ncd[k], ncd[j])
        tail = zero
        for i in range(k + 1, 4):
            tail = tail + a[i][k] * a[i][k]
        c0 = a[k][k]
        small = tail <= FLT_MIN
        tail_taken |= small
        beta = np.sqrt(c0 * c0 + tail)
        beta = np.where(c0 >= 0, -beta, beta)
        for i in range(k + 1, 4):
            a[i][k] = np.where(small, zero, a[i][k] / (c0 - beta))
        tau = np.where(small, zero, (beta - c0) / beta)
        beta = np.where(small, c0, beta)
        hc.append(tau)
        a[k][k] = beta
        maxpivot = np.where(np.abs(beta) > maxpivot, np.abs(beta), maxpivot)
        apply = tau != 0
        for j in range(k + 1, 3):
            tmp = zero
            for i in range(k + 1, 4):
                tmp = tmp + a[i][k] * a[i][j]
            tmp = tmp + a[k][j]
            a[k][j] = np.where(apply, a[k][j] - tau * tmp, a[k][j])
            for i in range(k + 1, 4):
                a[i][j] = np.where(apply, a[i][j] - (tau * a[i][k]) * tmp, a[i][j])
        for j in range(k + 1, 3):
            live = ncu[j] != 0
            t = np.abs(a[k][j]) / ncu[j]
            t = (F(1) + t) * (F(1) - t)
            t = np.where(t < 0, zero, t)
            r = ncu[j] / ncd[j]
            t2 = (t * r) * r
            down = live & (t2 <= downdate_thr)
            downdated |= down
            s = zero
            for i in range(k + 1, 4):
                s = s + a[i][j] * a[i][j]
            fresh = np.sqrt(s)
            ncd[j] = np.where(down, fresh, ncd[j])
            ncu[j] = np.where(down, fresh, np.where(live, ncu[j] * np.sqrt(t), ncu[j]))
    perm = [np.full(shape, j) for j in range(3)]
    for k in range(3):
        tk, pk = transp[k], perm[k]
        pt = np.where(tk == 0, perm[0], np.where(tk == 1, perm[1], perm[2]))
        perm[k] = pt
        for m in range(3):
            perm[m] = np.where(tk == m, pk, perm[m])
    prethr = np.abs(maxpivot) * (EPS * F(3))
    rank = np.zeros(shape, int)
    for i in range(3):
        rank = rank + ((i < nonzero) & (np.abs(a[i][i]) > prethr))
    for k in range(3):
        apply = hc[k] != 0
        tmp = zero
        for i in range(k + 1, 4):
            tmp = tmp + a[i][k] * c[i]
        tmp = tmp + c[k]
        c[k] = np.where(apply, c[k] - hc[k] * tmp, c[k])
        for i in range(k + 1, 4):
            c[i] = np.where(apply, c[i] - (hc[k] * a[i][k]) * tmp, c[i])
    y = [zero, zero, zero]
    for i in (2, 1, 0):
        s = c[i]
        for j in range(i + 1, 3):
            s = np.where(j < rank, s - a[i][j] * y[j], s)
        y[i] = np.where(i < rank, s / a[i][i], zero)
    x = [zero, zero, zero]
    for i in range(3):
        for p in range(3):
            x[p] = np.where((i < rank) & (perm[i] == p), y[i], x[p])
    census = SimpleNamespace(transp=np.stack(transp, -1), nonzero=nonzero, rank=rank, tail=tail_taken, downdate=downdated)
    return x, census


def _col(v):
    return np.asarray(v, F).reshape(-1, 1)


def post_process(cam, orient, conf, dims, bboxes, trig="fp64"):
    """cam: anything with fx, fy, cx, cy, orig_w.  Per box: alpha, theta_ray, orient, branch (0..3: BRANCHES),
    switch_mult, argmax, lwh (nb, 3), valid, loc (nb, 64, 3), err (nb, 64) in lane order ((l*4+t)*2+r)*4+b, winner (64 =
    none), best_loc (nb, 3), ties (how many sets hold the minimum; 0 without a winner), the QR's branch census (pivots
    (nb, 3), nonzero, rank, tail, downdate) and poses: the emitted LSHAPE_DTYPE list, unknown labels skipped."""
    orient = np.ascontiguousarray(orient, F).reshape(-1, 4)
    conf = np.ascontiguousarray(conf, F).reshape(-1, 2)
    dims = np.ascontiguousarray(dims, F).reshape(-1, 3)
    b = np.ascontiguousarray(bboxes, dtype=BBOX_DTYPE)
    nb = len(b)
    assert len(orient) == len(conf) == len(dims) == nb
    atan2, atan, tan, cos, sin = (trig_fn(n, trig) for n in ("atan2", "atan", "tan", "cos", "sin"))
    rows = np.arange(nb)
    with np.errstate(all="ignore"):
        # postProcessOutputs :466-470, generateBins(2) :241-258, computeAlpha :260-275
        argmax = (conf[:, 1] > conf[:, 0]).astype(int)
        interval = F(2.0 * math.pi / 2)                     # 2.0f * M_PI / bins in fp64, narrowed once
        bins = np.where(argmax == 1, interval, F(0)) + interval / F(2)
        alpha = atan2(orient[rows, argmax * 2 + 1], orient[rows, argmax * 2])
        alpha = alpha + bins
        alpha = alpha - PI_F
        # computeThetaRay :277-292
        w = F(cam.orig_w)
        fx, fy, cx, cy = F(cam.fx), F(cam.fy), F(cam.cx), F(cam.cy)
        fovx = F(2) * atan(np.full(nb, w / (F(2) * fx), F))
        centre = ((b["x_min"] + b["x_max"]) / 2.0).astype(F)    # two doubles, / 2.0f in fp64, narrowed on assignment
        ddx = centre - w / F(2)
        sign = np.where(ddx < 0, F(-1), F(1))
        ddx = np.abs(ddx)
        theta = atan(((F(2) * ddx) * tan(fovx / F(2))) / w)
        theta = theta * sign
        # class averages and dims :472-495; an unknown label adds zeros on the device and is not emitted
        avg = np.array([CLASS_DIMS.get(int(l), (0.0, 0.0, 0.0)) for l in b["label"]], F).reshape(nb, 3)
        valid = np.array([int(l) in CLASS_DIMS for l in b["label"]], bool)
        lwh = np.stack([dims[:, 2] + avg[:, 0], dims[:, 0] + avg[:, 1], dims[:, 1] + avg[:, 2]], 1)
        # calcLocation :294-447
        orient_f = alpha + theta
        c, s = _col(cos(orient_f)), _col(sin(orient_f))
        o, l = np.zeros((nb, 1), F), np.ones((nb, 1), F)
        Rm = [c, o, s, o, l, o, -s, o, c]
        box = [_col(b[k].astype(F)) for k in ("x_min", "y_min", "x_max", "y_max")]
        hx, hy, hz = (_col((lwh[:, k].astype(np.float64) / 2.0).astype(F)) for k in range(3))
        branch = np.where((alpha < DEG92) & (alpha > DEG88), 0,
                          np.where((alpha < -DEG88) & (alpha > -DEG92), 1,
                                   np.where((alpha < DEG90) & (alpha > -DEG90), 2, 3)))
        lm = _col(np.array([BRANCHES[int(v)][0] for v in branch]))
        rm = _col(np.array([BRANCHES[int(v)][1] for v in branch]))
        switch = np.where(alpha > 0, 1, -1)
        sw = _col(switch)
        lane = np.arange(64)
        pm = lambda bit: np.where(bit != 0, F(1), F(-1)).reshape(1, 64)   # noqa: E731
        t_, b_ = (lane >> 3) & 3, lane & 3
        li, ri = pm(lane >> 5), pm((lane >> 2) & 1)
        ti, tj, bi, bj = pm(t_ >> 1), pm(t_ & 1), pm(b_ >> 1), pm(b_ & 1)
        full = lambda v: np.broadcast_to(v, (nb, 64)).astype(F)   # noqa: E731
        X = [[full(lm * hx), full(li * hy), full(-sw * hz)],
             [full(ti * hx), full(-hy), full(tj * hz)],
             [full(rm * hx), full(ri * hy), full(sw * hz)],
             [full(bi * hx), full(hy), full(bj * hz)]]
        P = [[fx, F(0), cx, F(0)], [F(0), fy, cy, F(0)], [F(0), F(0), F(1), F(0)]]
        A, bv = [], []
        for row in range(4):
            RX = [(Rm[q * 3] * X[row][0] + Rm[q * 3 + 1] * X[row][1]) + Rm[q * 3 + 2] * X[row][2] for q in range(3)]
            pM3 = [((P[q][0] * RX[0] + P[q][1] * RX[1]) + P[q][2] * RX[2]) + P[q][3] * F(1) for q in range(3)]
            idx = row & 1
            v = box[row]
            A.append([full(P[idx][cc] - v * P[2][cc]) for cc in range(3)])     # :412
            bv.append(v * pM3[2] - pM3[idx])                                     # :415
        x, cen = _qr_solve(A, bv)
        err = np.zeros((nb, 64), F)
        for row in range(4):
            rr = ((A[row][0] * x[0] + A[row][1] * x[1]) + A[row][2] * x[2]) - bv[row]
            err = err + rr * rr
    loc = np.stack(x, -1)
    # sequential "if (err < best)" from FLT_MAX :382,:424: the lowest index of the minimum, nobody when none is below
    ok = err < FLT_MAX
    masked = np.where(ok, err, np.inf)
    winner = np.where(ok.any(1), masked.argmin(1), 64) if nb else np.zeros(0, int)
    best_loc = np.where(_col(winner < 64).astype(bool), loc[rows, np.minimum(winner, 63)], F(0)).astype(F).reshape(nb, 3)
    ties = np.where(winner < 64, (ok & (err == masked.min(1, keepdims=True))).sum(1), 0) if nb else np.zeros(0, int)
    for name in ("transp", "nonzero", "rank", "tail", "downdate"):   # A is the box's alone: one census per box
        v = getattr(cen, name)
        assert (v == v[:, :1]).all(), name
    poses = np.zeros(int(valid.sum()), LSHAPE_DTYPE)
    for m, i in enumerate(np.flatnonzero(valid)):
        hp = -float(orient_f[i]) * 0.5                       # setRPY(0, -orient, 0) :440, fp64 on the host
        cp, sp = _m.cos(hp), _m.sin(hp)
        q = (0.0 * cp * 1.0 - 1.0 * sp * 0.0, 1.0 * sp * 1.0 + 0.0 * cp * 0.0, 1.0 * cp * 0.0 - 0.0 * sp * 1.0,
             1.0 * cp * 1.0 + 0.0 * sp * 0.0)
        poses[m] = (*[float(v) for v in best_loc[i]], *q, *[float(v) for v in lwh[i]])
    return SimpleNamespace(alpha=alpha, theta_ray=theta, orient=orient_f, branch=branch, switch_mult=switch,
                           argmax=argmax, lwh=lwh, valid=valid, centre=centre, loc=loc, err=err, winner=winner,
                           best_loc=best_loc, ties=ties, pivots=cen.transp[:, 0], nonzero=cen.nonzero[:, 0],
                           rank=cen.rank[:, 0], tail=cen.tail[:, 0], downdate=cen.downdate[:, 0], poses=poses)


def alpha_of(cos_v, sin_v, argmax, trig="fp64"):
    """computeAlpha alone (float32 arrays)"""
    interval = F(2.0 * math.pi / 2)
    bins = np.where(np.asarray(argmax) == 1, interval, F(0)) + interval / F(2)
    return (trig_fn("atan2", trig)(sin_v, cos_v) + bins) - PI_F


def same_class_or_bytes(got, want):
    """zero tolerance: finite values and infinities by their bytes (the sign of zero included), NaN by class"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    gn, wn = np.isnan(got), np.isnan(want)
    iv = got.view(np.uint32 if got.dtype == np.float32 else np.uint64)
    wv = want.view(iv.dtype)
    return (gn == wn) & (gn | (iv == wv))


def poses_equal(got, want):
    """the same for LSHAPE_DTYPE lists: one bool per pose"""
    if len(got) != len(want):
        return np.zeros(max(len(got), len(want)), bool)
    g = np.ascontiguousarray(got).view(np.float64).reshape(len(got), 10)
    w = np.ascontiguousarray(want).view(np.float64).reshape(len(want), 10)
    return same_class_or_bytes(g, w).all(1)


# ------------------------------------------------------------------------------------------------- scenes --
CAMS = ((320.0, 320.0, 320.0, 240.0), (500.0, 300.0, 310.0, 250.0), (200.0, 450.0, 330.0, 200.0), (50.0, 60.0, 320.0, 240.0))
IMG_W, IMG_H = 640, 480
EDGE_BOXES = ((100, 100, 300, 250), (0, 0, 639, 479), (320, 240, 320, 240), (200, 100, 200, 250), (100, 240, 300, 240),
              (-2000, -1500, 3000, 2500), (319, 100, 321, 300), (10, 470, 30, 479), (320, 0, 320, 479), (0, 240, 639, 240),
              (320, 240, 321, 241), (300, 250, 100, 100))
LABELS = (9, 0, 1, 2, 5, -1)      # the four known classes and two unknown ones
PLAIN_BOX = (100.0, 100.0, 300.0, 250.0)


def cam_of(i):
    fx, fy, cx, cy = CAMS[i]
    return SimpleNamespace(fx=fx, fy=fy, cx=cx, cy=cy, orig_w=IMG_W, orig_h=IMG_H)


def make_boxes(rects, labels):
    b = np.zeros(len(rects), BBOX_DTYPE)
    for i, (r, l) in enumerate(zip(rects, labels)):
        b[i] = (*[float(v) for v in r], 0.9, l)
    return b


def _net(rng, n):
    ang = rng.uniform(-math.pi, math.pi, 2 * n)
    orient = np.stack([np.cos(ang), np.sin(ang)], 1).astype(F).reshape(n, 4)
    return orient, rng.uniform(0, 1, (n, 2)).astype(F), rng.uniform(-0.3, 0.3, (n, 3)).astype(F)


def scene(tag, cam, orient, conf, dims, boxes):
    return SimpleNamespace(tag=tag, cam=cam, orient=np.ascontiguousarray(orient, F), conf=np.ascontiguousarray(conf, F),
                           dims=np.ascontiguousarray(dims, F), boxes=boxes)


def edge_scene(cam):
    """every edge box with every label on camera `cam`"""
    rects = [r for r in EDGE_BOXES for _ in LABELS]
    labels = [l for _ in EDGE_BOXES for l in LABELS]
    return scene(f"edges-cam{cam}", cam, *_net(np.random.default_rng(100 + cam), len(rects)), make_boxes(rects, labels))


def reachable_alphas():
    """The alphas next to the seven thresholds that computeAlpha can return at all.  alpha = fl(fl(a + bin) - pi) with
    a = atan2 in [-pi, pi] and bin = pi/2 or 3 pi/2, so the sum lies in [-pi/2, 5 pi/2] and the subtraction of two
    floats that close is exact: alpha is a multiple of the SUM's ulp, shifted by fl(pi).  Near -88 / -90 / -92 degrees
    the sum is in [1, 2) and every float32 next to the threshold is reachable: the threshold and its two neighbours.
    Near 0 the sum is in [2, 4) with ulp 2^-22, so the reachable neighbours of 0 are +-2^-22.  Near +88 / +90 / +92
    degrees the sum is in [4, 8) with ulp 2^-21, four times alpha's own: the targets are the nearest reachable value
    on each side of the threshold, and the threshold itself where it lies on that lattice.
    Returns {threshold: sorted reachable targets}, enumerated from the sums themselves."""
    out = {}
    for t in THRESHOLDS:
        s0 = F(np.float64(t) + np.float64(PI_F))
        sums = [s0]
        for _ in range(6):
            sums = [np.nextafter(sums[0], F(-np.inf))] + sums + [np.nextafter(sums[-1], F(np.inf))]
        vals = sorted({F(s - PI_F) for s in sums})
        below = max(v for v in vals if v < t)
        above = min(v for v in vals if v > t)
        out[t] = [below] + ([t] if t in vals else []) + [above]
    return out


def _bin_of(argmax):
    interval = F(2.0 * math.pi / 2)
    return (interval if argmax else F(0)) + interval / F(2)


def atan2_values_for(target, argmax):
    """the float32 atan2 results in [-fl(pi), fl(pi)] that give alpha == target in bin `argmax` (none: unreachable there,
    for the range of atan2 or because a's own ulp, 2^-22 above 2 in magnitude, is coarser than the sum's)"""
    s = np.float64(target) + np.float64(PI_F)          # the sum that gives the target: exact in fp64
    step = float(np.spacing(F(s))) / 4
    cands = sorted({F(s - np.float64(_bin_of(argmax)) + k * step) for k in range(-8, 9)})
    return [a for a in cands if -PI_F <= a <= PI_F and F(F(a + _bin_of(argmax)) - PI_F) == target]


def find_canaries(seed=20):
    """seeded search for float32 (cos, sin) pairs, on and off the unit circle, whose fp64-trig alpha is exactly each
    reachable target of each threshold, in each bin that can reach it.  Returns [(threshold, target, argmax, cos, sin)]
    and the (threshold, target, argmax) that are reachable but were not found."""
    rng = np.random.default_rng(seed)
    found, missing = [], []
    for t, targets in reachable_alphas().items():
        for target in targets:
            for argmax in (0, 1):
                values = atan2_values_for(target, argmax)
                if not values:
                    continue
                hit = None
                for _ in range(4000):
                    ang = min(max(float(rng.choice(values)) + rng.uniform(-2e-7, 2e-7), -math.pi), math.pi)
                    r = rng.uniform(0.25, 4.0)
                    cv, sv = F(r * math.cos(ang)), F(r * math.sin(ang))
                    if alpha_of(cv, sv, argmax) == target:
                        hit = (cv, sv)
                        break
                if hit:
                    found.append((t, target, argmax, *hit))
                else:
                    missing.append((t, target, argmax))
    return found, missing


_CANARIES = None


def canaries():
    global _CANARIES
    if _CANARIES is None:
        _CANARIES = find_canaries()
    return _CANARIES


def canary_scene():
    """one plain vehicle box per canary on the default camera; the other bin holds a pair that would give another
    alpha, the confidences pick the bin.  Then orientation pairs off the unit circle, (0, 0) in both signs of zero,
    and equal confidences (argmax 0) with different pairs in the two bins."""
    found, _ = canaries()
    orient, conf = [], []
    for _, _, argmax, cv, sv in found:
        pair, other = [cv, sv], [0.6, -0.8]
        orient.append(pair + other if argmax == 0 else other + pair)
        conf.append([0.8, 0.3] if argmax == 0 else [0.3, 0.8])
    for pair in ([3.0, 4.0], [1e-3, -2e-3], [1e-30, 1e-30], [0.0, 0.0], [-0.0, 0.0], [0.0, -0.0], [-0.0, -0.0], [1e30, -1e30]):
        orient.append(pair + [0.6, 0.8])
        conf.append([0.9, 0.1])
        orient.append([0.6, 0.8] + pair)
        conf.append([0.1, 0.9])
    for cv in (0.25, 0.5, 0.75):
        orient.append([0.0, 1.0, 1.0, 0.0])      # bin 0: alpha 0; bin 1 would give pi / 2
        conf.append([cv, cv])
    n = len(orient)
    dims = np.random.default_rng(21).uniform(-0.3, 0.3, (n, 3))
    return scene("canaries", 0, orient, conf, dims, make_boxes([PLAIN_BOX] * n, [9] * n))


def centre_scene():
    """box centres exactly on orig_w / 2, one ulp to the left and one to the right of it (theta_ray's sign)"""
    left = float(np.nextafter(F(320), F(0)))
    right = float(np.nextafter(F(320), F(1000)))
    rects = [(220.0, 100.0, 420.0, 250.0), (220.0, 100.0, 2 * left - 220.0, 250.0), (220.0, 100.0, 2 * right - 220.0, 250.0)]
    rects = rects * 2
    n = len(rects)
    return scene("centre", 0, *_net(np.random.default_rng(22), n), make_boxes(rects, [9, 2, 0, 1, 9, 2]))


GOOD = ((100, 100, 300, 250), (350, 120, 600, 300), (20, 200, 180, 330), (250, 50, 420, 200))
NAN, INF = float("nan"), float("inf")


def nonfinite_scene():
    """good boxes and bad ones by turns: NaN and +-Inf in one field at a time (a box edge, an orientation value, a
    dims residual), a residual that makes the length negative, and boxes of a million pixels.  Returns the scene and
    the indices of the good boxes."""
    rng = np.random.default_rng(23)
    bad = []   # (rect, orient override, dims override)
    for e in range(4):
        for v in (NAN, INF, -INF):
            r = list(PLAIN_BOX)
            r[e] = v
            bad.append((r, None, None))
    for slot in range(4):
        for v in (NAN, INF, -INF):
            bad.append((PLAIN_BOX, (slot, v), None))
    for slot in range(3):
        for v in (NAN, INF, -INF):
            bad.append((PLAIN_BOX, None, (slot, v)))
    bad.append((PLAIN_BOX, None, (2, -10.0)))                       # length 3.884 - 10 < 0
    bad.append((PLAIN_BOX, None, (0, -1.629)))                      # width 0 or next to it
    bad.append(((-1e6, -1e6, 1e6, 1e6), None, None))
    bad.append(((1e6, 1e6, 2e6, 3e6), None, None))
    bad.append(((-1e6, 100, 1e6, 250), None, None))
    bad.append(((3e38, 100, 3.2e38, 250), None, None))             # the centre's sum overflows fp32 but not fp64
    bad.append(((1e300, 100, 1e300, 250), None, None))             # (float) of the edge is Inf
    rects, labels, good = [], [], []
    n = 2 * len(bad) + 1
    orient, conf, dims = _net(rng, n)
    for i, (r, o_over, d_over) in enumerate(bad):
        good.append(len(rects))
        rects.append(GOOD[i % 4]); labels.append(LABELS[i % 4])
        k = len(rects)
        rects.append(r); labels.append(LABELS[(i // 4) % 4])
        if o_over:
            orient[k, o_over[0]] = o_over[1]
            if o_over[0] >= 2:
                conf[k] = (0.2, 0.7)
            else:
                conf[k] = (0.7, 0.2)
        if d_over:
            dims[k, d_over[0]] = d_over[1]
    good.append(len(rects))
    rects.append(GOOD[0]); labels.append(9)
    return scene("nonfinite", 0, orient, conf, dims, make_boxes(rects, labels)), np.array(good)


def random_scene(cam, n, seed):
    """ordinary boxes (inside and across the image border) with random labels: the batch-size and call-site scenes"""
    rng = np.random.default_rng(seed)
    x0, y0 = rng.uniform(-50, 560, n), rng.uniform(-30, 400, n)
    rects = np.stack([x0, y0, x0 + rng.uniform(5, 250, n), y0 + rng.uniform(5, 180, n)], 1)
    return scene(f"random-cam{cam}-{n}", cam, *_net(rng, n), make_boxes(rects, rng.choice(LABELS, n)))


def all_scenes():
    """every scene the GPU file runs, for the host file's pin to the oracle and its fixture conditions"""
    return ([edge_scene(c) for c in range(len(CAMS))] + [canary_scene(), centre_scene(), nonfinite_scene()[0]]
            + [random_scene(c, 40, 30 + c) for c in range(len(CAMS))] + [random_scene(0, 200, 40)])


_REF = {}


def reference(sc, trig="fp64"):
    """post_process of a scene, computed once per (scene, trig) and shared; callers leave it unchanged"""
    key = (sc.tag, trig)
    if key not in _REF:
        _REF[key] = post_process(cam_of(sc.cam), sc.orient, sc.conf, sc.dims, sc.boxes, trig)
    return _REF[key]
