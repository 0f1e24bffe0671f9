"""[EXTENSION] X14 fixture families of test_track_host.py and test_gpu_track.py.  A case is dict(name, cfg, tracks,
next_id, steps): the state to load (a TRACK_DTYPE array, ascending slots) and a sequence of updates, each
dict(dets, dt, motion).  want(case) runs track_ref over it once and keeps, per step, the bytes every implementation
must give: the live records, next_id, the info record and the exported objects.

No family lets an operation make a NaN of finite or infinite inputs (inf - inf, 0 * inf): the sign of such a NaN is the
processor's choice, and device, host and reference are compared by bytes.  NaNs that are loaded travel through single
operations unchanged, which is all the non-finite families need."""
import math

import numpy as np

import track_ref as ref

_LSHAPE = None


def lshape():
    global _LSHAPE
    if _LSHAPE is None:
        from gvamd.synth import LSHAPE_DTYPE
        _LSHAPE = LSHAPE_DTYPE
    return _LSHAPE


def dets(rows):
    """rows of (px, py, yaw, length, width) -> LSHAPE_DTYPE; pz and height are set and must not matter"""
    rows = np.asarray(rows, np.float64).reshape(-1, 5)
    z = np.zeros(len(rows), lshape())
    z["px"], z["py"], z["pz"], z["height"] = rows[:, 0], rows[:, 1], 7.0, 1.5
    z["qz"], z["qw"] = np.sin(0.5 * rows[:, 2]), np.cos(0.5 * rows[:, 2])
    z["length"], z["width"] = rows[:, 3], rows[:, 4]
    return z


def boxes_at(xy):
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    return dets(np.concatenate([xy, np.zeros((len(xy), 1)), np.full((len(xy), 1), 4.0), np.full((len(xy), 1), 2.0)], axis=1))


def tracks_at(xy, slots=None, v=None, hits=1, first_id=1, p=(0.0625, 0.0, 16.0)):
    """tracks at the positions, in the given slots (default 0, 1, ..), velocity rows v (default 0), identity quaternion"""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    t = np.zeros(len(xy), ref.TRACK_DTYPE)
    t["slot"] = np.arange(len(xy)) if slots is None else slots
    t["id"] = first_id + np.arange(len(xy))
    t["hits"], t["det"] = hits, -1
    t["x"], t["y"] = xy[:, 0], xy[:, 1]
    if v is not None:
        v = np.asarray(v, np.float64).reshape(-1, 2)
        t["vx"], t["vy"] = v[:, 0], v[:, 1]
    t["qw"], t["length"], t["width"] = 1.0, 4.0, 2.0
    t["p00"], t["p01"], t["p11"] = p
    return t


def step(z=None, dt=0.1, motion=None):
    return dict(dets=z if z is not None else np.zeros(0, lshape()), dt=float(dt), motion=motion)


def case(name, cfg, steps, tracks=None, next_id=1):
    return dict(name=name, cfg=cfg, tracks=tracks if tracks is not None else np.zeros(0, ref.TRACK_DTYPE), next_id=next_id,
                steps=steps)


def chain(n):
    """positions T0 D0 T1 D1 .. on a line with strictly growing gaps, all multiples of 2^-8: detection i is closer to
    track i than to track i + 1, and track i + 1 is closer to detection i than to its own, so a round matches one pair"""
    gaps = 1.0 + np.arange(2 * n - 1) / 256.0
    pos = np.concatenate([[0.0], np.cumsum(gaps)])
    return pos[0::2], pos[1::2]


def lattice(seed, n_t, n_d, span=24):
    """n_t tracks and n_d detections on a lattice of quarter metres in a span/4 m square: equal d2 occur exactly"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, span, (n_t, 2)) * 0.25
    d = rng.integers(0, span, (n_d, 2)) * 0.25
    return t, d


def _families():
    out = []
    base = ref.config()
    three = boxes_at([(5.0, 1.0), (9.0, -2.0), (20.0, 0.5)])
    # ---- empty
    out.append(case("empty_both", base, [step(), step()]))
    out.append(case("empty_state_then_dets_then_none", base, [step(three), step(), step(three), step(), step(), step(), step()]))
    out.append(case("tracks_no_dets", base, [step(), step(), step()], tracks_at([(1.0, 1.0), (4.0, 4.0)], slots=[3, 127], hits=2), 9))
    # ---- 128 births, then a full house
    grid = [(3.0 * (i % 16), 3.0 * (i // 16)) for i in range(128)]
    far = [(1000.0 + 3.0 * (i % 16), 3.0 * (i // 16)) for i in range(128)]
    out.append(case("full_house", ref.config(gate=1.0, max_misses=1),
                    [step(boxes_at(grid)), step(boxes_at(far)), step(boxes_at(far)[:5]), step(boxes_at(far)[:7])]))
    # ---- ties
    for seed, n_t, n_d in ((1, 40, 40), (2, 64, 30), (3, 30, 128), (4, 128, 128)):
        t, d = lattice(seed, n_t, n_d, span=24 if n_t < 128 else 40)
        out.append(case(f"ties_{seed}", ref.config(gate=1.0), [step(boxes_at(d), dt=0.0)], tracks_at(t), 500))
    # ---- chains
    for n in (2, 64, 128):
        t, d = chain(n)
        out.append(case(f"chain_{n}", ref.config(gate=3.0), [step(boxes_at(np.stack([d, np.zeros(n)], 1)), dt=0.0)],
                        tracks_at(np.stack([t, np.zeros(n)], 1)), 200))
    # ---- gate: d2 == gate2 (slot 0 matches), d2 the next double above (slot 1 does not: a birth)
    g = 1.5
    edge = boxes_at([(g, 0.0), (100.0 + g, 1.5 * 2.0 ** -26)])
    out.append(case("gate_edge", ref.config(gate=g), [step(edge, dt=0.0)], tracks_at([(0.0, 0.0), (100.0, 0.0)]), 7))
    # ---- life cycle
    one = lambda k: boxes_at([(2.0 + 0.5 * k, 1.0)])
    out.append(case("confirm_then_delete", ref.config(confirm_hits=3, max_misses=2),
                    [step(one(k)) for k in range(4)] + [step() for _ in range(4)]))
    out.append(case("max_misses_0_reuse", ref.config(max_misses=0, gate=1.0),
                    [step(boxes_at([(0.0, 0.0), (10.0, 0.0)])), step(boxes_at([(50.0, 0.0), (10.0, 0.25)])), step()]))
    out.append(case("id_wrap", base, [step(three)], tracks_at([(-30.0, 0.0)], slots=[1]), 0xFFFFFFFF))
    sat = tracks_at([(0.0, 0.0), (10.0, 0.0)], hits=ref.INT_MAX)
    sat["age"], sat["misses"][1] = ref.INT_MAX, ref.INT_MAX - 1
    out.append(case("saturate", ref.config(max_misses=255), [step(boxes_at([(0.0, 0.0)]), dt=0.0)], sat, 3))
    # ---- filter: 50 updates, varying dt with dt = 0 among them; with and without process noise
    for name, sa in (("filter", 1.5), ("filter_sigma_accel_0", 0.0)):
        rng = np.random.default_rng(11)
        steps, t = [], 0.0
        for k in range(50):
            dt = (0.1, 0.05, 0.2, 0.0, 0.1)[k % 5]
            t += dt
            pts = [(2.0 + 3.0 * t, -1.0 + 0.5 * t), (30.0 - 4.0 * t, 5.0), (12.0, 12.0 + 2.0 * t * t)]
            pts = np.asarray(pts) + rng.normal(0.0, 0.1, (3, 2))
            keep = [i for i in range(3) if not (i == 1 and 20 <= k < 23)]       # the second one is missed three times
            z = dets([(pts[i][0], pts[i][1], 0.1 * k, 4.0 + 0.01 * k, 2.0) for i in keep])
            steps.append(step(z, dt))
        out.append(case(name, ref.config(gate=2.5, sigma_accel=sa, max_misses=3, min_speed=0.5), steps))
    # ---- ego motion: translation only, a quarter turn, a general motion, a non-planar quaternion
    h = math.sqrt(0.5)
    motions = [(0.0, 0.0, 0.0, 1.0, 0.5, -0.25, 0.0), (0.0, 0.0, h, h, 0.0, 0.0, 0.0),
               (0.0, 0.0, math.sin(0.05), math.cos(0.05), 0.7, 0.1, 0.02), (0.1, -0.2, 0.3, 0.9, 0.3, 0.2, 0.1)]
    moving = tracks_at([(5.0, 1.0), (9.0, -2.0), (-4.0, 6.0)], v=[(2.0, 0.0), (0.0, -1.5), (0.5, 0.5)], hits=3)
    moving["qz"], moving["qw"] = [0.0, h, 0.6], [1.0, h, 0.8]
    for k, m in enumerate(motions):
        out.append(case(f"ego_{k}", base, [step(boxes_at([(5.0, 1.0)]), 0.1, m), step(None, 0.1, m)], moving, 4))
    out.append(case("ego_sequence", ref.config(gate=3.0), [step(three if k % 2 == 0 else None, 0.1, motions[k % 4]) for k in range(8)]))
    # ---- invalid detections: NaN, inf and a negative size in each read field, each alone
    bad = boxes_at([(40.0 + 5.0 * k, 3.0) for k in range(24)])
    k = 0
    for f in ref.DET_READ:
        for v in (math.nan, math.inf, -math.inf):
            bad[k][f] = v
            k += 1
    rest = boxes_at([(5.0, 1.0), (9.0, -2.0), (20.0, 0.5), (25.0, 0.5)])
    rest["length"][0], rest["width"][1] = -0.5, -1e-300
    rest["pz"][2], rest["height"][3] = math.nan, -math.inf        # not read: both stay valid
    rest = np.concatenate([rest, boxes_at([(60.0, 60.0)])])
    rest["length"][4], rest["width"][4] = 0.0, 0.0                # zero size is valid
    out.append(case("invalid_dets", base, [step(np.concatenate([bad, rest])), step(np.concatenate([rest, bad]))]))
    # ---- non-finite track states: never a candidate, never exported
    nf = tracks_at([(0.0, 0.0), (10.0, 0.0), (20.0, 0.0), (30.0, 0.0), (40.0, 0.0)], hits=5, v=[(1.0, 0.0)] * 5)
    nf["x"][0], nf["y"][1], nf["vx"][2], nf["vy"][3] = math.inf, math.nan, -math.inf, math.nan
    near = boxes_at([(0.0, 0.0), (10.1, 0.0), (20.1, 0.0), (30.1, 0.0), (40.1, 0.0)])
    out.append(case("non_finite_states", ref.config(gate=5.0, max_misses=9), [step(near, 0.1), step(near, 0.1)], nf, 6))
    # ---- min_speed at equality: sp2 == min2 keeps the velocity, one ulp below gives (0, 0)
    ms = tracks_at([(0.0, 0.0), (10.0, 0.0), (20.0, 0.0)], hits=5, v=[(3.0, 4.0), (3.0, math.nextafter(4.0, 0.0)), (0.0, 0.0)])
    out.append(case("min_speed_edge", ref.config(min_speed=5.0, max_misses=9), [step(None, 0.0), step(None, 0.125)], ms, 4))
    return out


_CASES, _WANT = None, {}


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _families()
        assert len({c["name"] for c in _CASES}) == len(_CASES)
    return _CASES


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


def moving_object_dtype():
    import gvamd
    return gvamd.MOVING_OBJECT_DTYPE


def want(c):
    """per step dict(tracks, next_id, info, objs, n_rounds): arrays of the library's dtypes; computed once, read-only"""
    if c["name"] not in _WANT:
        state, next_id, out = ref.unpack(c["tracks"]), c["next_id"], []
        for s in c["steps"]:
            state, next_id, info, objs = ref.step(c["cfg"], state, next_id, ref.det_list(s["dets"]), s["dt"], s["motion"])
            rec = dict(tracks=ref.pack(state), next_id=next_id, info=ref.pack_info(info), objs=ref.pack_objs(objs, moving_object_dtype()))
            for a in ("tracks", "info", "objs"):
                rec[a].setflags(write=False)
            out.append(rec)
        _WANT[c["name"]] = out
    return _WANT[c["name"]]
