"""[EXTENSION] X10 rollout: the fixture families that test_rollout_host.py rolls out with the library's host twin and
test_gpu_rollout.py on the device, both against rollout_ref.

Two EXACT kinds do not depend on the libm at all and are compared byte for byte everywhere:
  zeros     all-zero controls: every increment is 0 * c, every pose is (float)start;
  straight  T0 == 0 and w == 0: cos is 1 and sin is 0 on any libm, a * c - b * s is a exactly.
The GENERAL kinds depend on fp64 sin / cos in the last bit (the host's C library on both sides of the host test, the
device's against the C library's in the GPU test):
  random    random controls from (-3.25, 1.5, 0.3) on the 500 x 200 map of traj_cases;
  leaving   arcs from near that map's +x edge that leave it (dt = 0.5 s);
  spin      a fast spin from yaw 99999.5 rad: the yaw passes 10^5 rad in the first step, where the argument reduction of
            sincos takes its slow path;
  nonfinite a NaN and an infinity in every control component at steps 0, 31 and 63 of a 65-step trajectory (constant
            controls: the held control itself).
Every kind comes with both motion models, with per-step and with constant controls, and in the shapes of SHAPES, which
between them take K through 1, 3, 64, 65, 257 and P through 1, 2, 63, 64, 65, 130 (nonfinite: its own 65 steps)."""
import numpy as np

import rollout_ref as ref

SHAPES = [(1, 130), (3, 64), (64, 63), (65, 65), (257, 2), (65, 1)]   # (K, P)
KINDS = ["zeros", "straight", "random", "leaving", "spin", "nonfinite"]
EXACT = ("zeros", "straight")
MODELS = [ref.DIFF, ref.OMNI]
START = (-3.25, 1.5, 0.3)

_CACHE = {}


def _controls(kind, model, rng, n):
    """(n, C) float32 control rows of a kind"""
    C = ref.n_controls(model)
    u = np.zeros((n, C), np.float32)
    if kind == "zeros":
        return u
    lo, hi = {"straight": (-1.0, 3.0), "random": (-1.0, 3.0), "leaving": (1.5, 3.0), "spin": (-1.0, 3.0),
              "nonfinite": (0.5, 2.0)}[kind]
    u[:, 0] = rng.uniform(lo, hi, n)
    if model == ref.OMNI:
        u[:, 1] = rng.uniform(-0.5, 0.5, n)
    if kind == "spin":
        u[:, -1] = rng.uniform(20.0, 60.0, n)        # 1 .. 3 rad a step at dt = 0.05
    elif kind == "leaving":
        u[:, -1] = rng.uniform(-0.1, 0.1, n)         # wide arcs: a tight one would circle inside the map
    elif kind != "straight":
        u[:, -1] = rng.uniform(-1.5, 1.5, n)
    return u


def _nonfinite(model, constant, rng):
    C = ref.n_controls(model)
    bad = [(comp, v) for comp in range(C) for v in (np.float32(np.nan), np.float32(np.inf))]
    if constant:
        u = _controls("nonfinite", model, rng, len(bad))
        for k, (comp, v) in enumerate(bad):
            u[k, comp] = v
        return u
    steps = (0, 31, 63)
    u = _controls("nonfinite", model, rng, len(bad) * len(steps) * 65).reshape(len(bad) * len(steps), 65, C)
    for i, (comp, v) in enumerate(bad):
        for j, p in enumerate(steps):
            u[i * len(steps) + j, p, comp] = v
    return u


def family(kind, model, constant):
    """the cases of one kind: a list of dict(name, model, dt, start, controls, constant, P)"""
    key = (kind, model, constant)
    if key in _CACHE:
        return _CACHE[key]
    dt = 0.5 if kind == "leaving" else 0.05
    start = {"straight": (-3.25, 1.5, 0.0), "leaving": (38.0, 0.5, 0.3), "spin": (-3.25, 1.5, 99999.5)}.get(kind, START)
    C = ref.n_controls(model)
    out = []
    shapes = [(None, 65)] if kind == "nonfinite" else SHAPES
    for i, (K, P) in enumerate(shapes):
        rng = np.random.default_rng(1000 * KINDS.index(kind) + 100 * model + 10 * int(constant) + i)
        if kind == "nonfinite":
            u = _nonfinite(model, constant, rng)
        else:
            u = _controls(kind, model, rng, K if constant else K * P)
            u = u if constant else u.reshape(K, P, C)
        out.append(dict(name="%s_%s_%s_%dx%d" % (kind, "omni" if model else "diff", "const" if constant else "steps", len(u), P),
                        model=model, dt=dt, start=start, controls=np.ascontiguousarray(u, np.float32), constant=constant, P=P))
    _CACHE[key] = out
    return out


_WANT = {}


def want(case):
    """rollout_ref.rollout of a case, computed once"""
    if case["name"] not in _WANT:
        _WANT[case["name"]] = ref.rollout(case["model"], case["dt"], case["start"], case["controls"], case["constant"], case["P"])
    return _WANT[case["name"]]


def same_but_nan_payload(got, want_):
    """byte equality where the reference is not a NaN, a NaN where it is"""
    got, want_ = np.asarray(got, np.float32).reshape(-1), np.asarray(want_, np.float32).reshape(-1)
    nan = np.isnan(want_)
    return bool(np.array_equal(np.isnan(got), nan) and got[~nan].tobytes() == want_[~nan].tobytes())
