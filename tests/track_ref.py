"""[EXTENSION] X14 reference: one update of the tracker over the tick's boxes, the X14 text of
include/gridvision_hip.h restated with scalar fp64 values and plain Python loops (a Python float is an IEEE double and
every operation below is one rounded operation: nothing can be contracted).  The association is a literal sort of the
candidates by (d2, s, d) and a sweep.  rounds() is the other way to the same matching, the parallel rounds the device
kernel runs, written out so that the two can be compared without a GPU.

The state is a dict slot -> track, a track a dict of Python ints and floats with gv_track's field names; pack() and
unpack() go to and from the TRACK_DTYPE array (live records in ascending slot order) that the library calls take."""
import math

import numpy as np

SLOTS = 128
INT_MAX = 2 ** 31 - 1
INT_FIELDS = ("id", "slot", "hits", "misses", "age", "det")
F64_FIELDS = ("x", "y", "vx", "vy", "qx", "qy", "qz", "qw", "length", "width", "p00", "p01", "p11")
TRACK_DTYPE = np.dtype([("id", np.uint32)] + [(n, np.int32) for n in INT_FIELDS[1:]] + [(n, np.float64) for n in F64_FIELDS])
INFO_FIELDS = ("n_tracks", "n_confirmed", "n_exported", "n_matched", "n_born", "n_deleted", "n_dropped", "n_invalid")
INFO_DTYPE = np.dtype([(n, np.int32) for n in INFO_FIELDS] + [("next_id", np.uint32), ("reserved", np.uint32)])
assert TRACK_DTYPE.itemsize == 128 and INFO_DTYPE.itemsize == 40
DET_READ = ("px", "py", "qx", "qy", "qz", "qw", "length", "width")


def config(gate=2.0, sigma_accel=1.0, sigma_meas=0.25, sigma_v0=4.0, min_speed=0.0, confirm_hits=2, max_misses=2, flags=0):
    return dict(gate=float(gate), sigma_accel=float(sigma_accel), sigma_meas=float(sigma_meas), sigma_v0=float(sigma_v0),
                min_speed=float(min_speed), confirm_hits=int(confirm_hits), max_misses=int(max_misses), flags=int(flags))


def to_struct(gvamd, cfg):
    c = gvamd.TrackConfig()
    for n, v in cfg.items():
        setattr(c, n, v)
    return c


def pack(state):
    out = np.zeros(len(state), TRACK_DTYPE)
    for k, s in enumerate(sorted(state)):
        for n in INT_FIELDS + F64_FIELDS:
            out[k][n] = state[s][n]
    return out


def unpack(tracks):
    state = {}
    for r in tracks:
        t = {n: int(r[n]) for n in INT_FIELDS}
        t.update({n: float(r[n]) for n in F64_FIELDS})
        state[t["slot"]] = t
    return state


def det_list(dets):
    """the read fields of an LSHAPE_DTYPE array as dicts of Python floats"""
    return [{n: float(d[n]) for n in DET_READ} for d in dets]


def _inc(v):
    return v + 1 if v < INT_MAX else v


def _finite(v):
    return math.isfinite(v)


def candidates(state, dets, valid, gate2):
    """every (d2, s, d) inside the gate, in no particular order"""
    out = []
    for s, t in state.items():
        for d, z in enumerate(dets):
            if valid[d]:
                ex = z["px"] - t["x"]
                ey = z["py"] - t["y"]
                d2 = ex * ex + ey * ey
                if d2 <= gate2:
                    out.append((d2, s, d))
    return out


def greedy(cands):
    """the definition: the smallest remaining candidate of the total order (d2, s, d), again and again"""
    of_slot, of_det = {}, {}
    for d2, s, d in sorted(cands):
        if s not in of_slot and d not in of_det:
            of_slot[s] = d
            of_det[d] = s
    return of_slot


def rounds(cands):
    """the device's way: per round, every remaining pair that is the (d2, s, d)-minimum of both its slot and its
    detection is matched at once.  Returns (of_slot, the number of rounds that matched something)."""
    of_slot, of_det, n_rounds = {}, {}, 0
    left = list(cands)
    while left:
        row, col = {}, {}
        for c in left:
            if c[1] not in row or c < row[c[1]]:
                row[c[1]] = c
            if c[2] not in col or c < col[c[2]]:
                col[c[2]] = c
        hit = [c for c in left if row[c[1]] == c and col[c[2]] == c]
        assert hit                      # the smallest remaining candidate is always one
        for _, s, d in hit:
            of_slot[s] = d
            of_det[d] = s
        n_rounds += 1
        left = [c for c in left if c[1] not in of_slot and c[2] not in of_det]
    return of_slot, n_rounds


def step(cfg, state, next_id, dets, dt, motion=None, assoc=greedy):
    """One update.  state: dict slot -> track (not modified); dets: det_list(); motion: None or (qx, qy, qz, qw, tx, ty,
    tz).  Returns (state, next_id, info dict, objs) with objs a list of (x, y, qx, qy, qz, qw, length, width, vx, vy)."""
    q = cfg["sigma_accel"] * cfg["sigma_accel"]
    r = cfg["sigma_meas"] * cfg["sigma_meas"]
    v0 = cfg["sigma_v0"] * cfg["sigma_v0"]
    gate2 = cfg["gate"] * cfg["gate"]
    min2 = cfg["min_speed"] * cfg["min_speed"]
    dt = float(dt)
    state = {s: dict(t) for s, t in state.items()}
    # step 1
    if motion is not None:
        mx, my, mz, mw, tx, ty, _ = [float(v) for v in motion]
        ce = 1.0 - 2.0 * (my * my + mz * mz)
        se = 2.0 * (mw * mz + mx * my)
        ax, ay, az, aw = -mx, -my, -mz, mw
        for t in state.values():
            dx = t["x"] - tx
            dy = t["y"] - ty
            t["x"] = ce * dx + se * dy
            t["y"] = ce * dy - se * dx
            vx = ce * t["vx"] + se * t["vy"]
            vy = ce * t["vy"] - se * t["vx"]
            t["vx"], t["vy"] = vx, vy
            bx, by, bz, bw = t["qx"], t["qy"], t["qz"], t["qw"]
            t["qw"] = aw * bw - ax * bx - ay * by - az * bz
            t["qx"] = aw * bx + ax * bw + ay * bz - az * by
            t["qy"] = aw * by - ax * bz + ay * bw + az * bx
            t["qz"] = aw * bz + ax * by - ay * bx + az * bw
    # step 2
    dt2 = dt * dt
    for t in state.values():
        t["x"] = t["x"] + t["vx"] * dt
        t["y"] = t["y"] + t["vy"] * dt
        p00 = ((t["p00"] + (2.0 * dt) * t["p01"]) + dt2 * t["p11"]) + q * (0.25 * (dt2 * dt2))
        p01 = (t["p01"] + dt * t["p11"]) + q * (0.5 * (dt2 * dt))
        p11 = t["p11"] + q * dt2
        t["p00"], t["p01"], t["p11"] = p00, p01, p11
        t["age"] = _inc(t["age"])
        t["det"] = -1
    # step 3
    valid = [all(_finite(z[n]) for n in DET_READ) and z["length"] >= 0.0 and z["width"] >= 0.0 for z in dets]
    # step 4
    of_slot = assoc(candidates(state, dets, valid, gate2))
    if isinstance(of_slot, tuple):
        of_slot = of_slot[0]
    matched_dets = set(of_slot.values())
    # steps 5 and 6
    n_deleted = 0
    for s in sorted(state):
        t = state[s]
        if s in of_slot:
            d = of_slot[s]
            z = dets[d]
            ex = z["px"] - t["x"]
            ey = z["py"] - t["y"]
            S = t["p00"] + r
            k0 = _div(t["p00"], S)
            k1 = _div(t["p01"], S)
            t["x"] = t["x"] + k0 * ex
            t["vx"] = t["vx"] + k1 * ex
            t["y"] = t["y"] + k0 * ey
            t["vy"] = t["vy"] + k1 * ey
            p11 = t["p11"] - k1 * t["p01"]
            p01 = t["p01"] - k1 * t["p00"]
            p00 = t["p00"] - k0 * t["p00"]
            t["p00"], t["p01"], t["p11"] = p00, p01, p11
            for n in ("qx", "qy", "qz", "qw", "length", "width"):
                t[n] = z[n]
            t["hits"] = _inc(t["hits"])
            t["misses"] = 0
            t["det"] = d
        else:
            t["misses"] = _inc(t["misses"])
            if t["misses"] > cfg["max_misses"]:
                del state[s]
                n_deleted += 1
    # step 7
    n_born = n_dropped = 0
    for d, z in enumerate(dets):
        if valid[d] and d not in matched_dets:
            free = [s for s in range(SLOTS) if s not in state]
            if not free:
                n_dropped += 1
                continue
            s = free[0]
            t = dict(id=next_id, slot=s, hits=1, misses=0, age=0, det=d, x=z["px"], y=z["py"], vx=0.0, vy=0.0, p00=r, p01=0.0, p11=v0)
            for n in ("qx", "qy", "qz", "qw", "length", "width"):
                t[n] = z[n]
            state[s] = t
            next_id = (next_id + 1) & 0xFFFFFFFF
            n_born += 1
    # step 8
    objs, n_confirmed = [], 0
    for s in sorted(state):
        t = state[s]
        if t["hits"] >= cfg["confirm_hits"]:
            n_confirmed += 1
            if all(_finite(t[n]) for n in ("x", "y", "vx", "vy")):
                sp2 = t["vx"] * t["vx"] + t["vy"] * t["vy"]
                vx, vy = (0.0, 0.0) if sp2 < min2 else (t["vx"], t["vy"])
                objs.append((t["x"], t["y"], t["qx"], t["qy"], t["qz"], t["qw"], t["length"], t["width"], vx, vy))
    info = dict(n_tracks=len(state), n_confirmed=n_confirmed, n_exported=len(objs), n_matched=len(of_slot), n_born=n_born,
                n_deleted=n_deleted, n_dropped=n_dropped, n_invalid=valid.count(False), next_id=next_id, reserved=0)
    return state, next_id, info, objs


def _div(a, b):
    """a / b as IEEE gives it: Python raises on a zero divisor, which p00 == -r can make of S (then S is +0.0, r > 0)"""
    if b == 0.0:
        return math.nan if (a == 0.0 or a != a) else math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def pack_info(info):
    out = np.zeros(1, INFO_DTYPE)
    for n, v in info.items():
        out[0][n] = v
    return out


def pack_objs(objs, dtype):
    """the exported objects as the MOVING_OBJECT_DTYPE array gv_track_step writes (pz and height 0)"""
    out = np.zeros(len(objs), dtype)
    for k, o in enumerate(objs):
        p = out[k]["pose"]
        p["px"], p["py"], p["qx"], p["qy"], p["qz"], p["qw"], p["length"], p["width"] = o[:8]
        out[k]["vx"], out[k]["vy"] = o[8], o[9]
    return out
