"""[EXTENSION] X14 the tracker over the tick's boxes, host side (no GPU): the header, the binding and the struct layouts;
the library's host twin (gv_track_step: the kernel's arithmetic text compiled for the host) against track_ref on every
family of track_cases, byte for byte; the parallel rounds the kernel runs against the sorted greedy; the argument
errors; and csrc/gv_track.hpp once more in a stand-alone program under the address and undefined-behaviour sanitizers,
whose digests must equal those of the library's bytes."""
import ctypes as C
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import track_cases as tc
import track_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GV_ERR_BAD_ARG = 1

LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "gridvision_hip.h"
#define O(t, f) printf("%zu ", offsetof(t, f))
int main(void)
{
  printf("%zu ", sizeof(gv_track));
  O(gv_track, id); O(gv_track, slot); O(gv_track, hits); O(gv_track, misses); O(gv_track, age); O(gv_track, det);
  O(gv_track, x); O(gv_track, y); O(gv_track, vx); O(gv_track, vy); O(gv_track, qx); O(gv_track, qy); O(gv_track, qz);
  O(gv_track, qw); O(gv_track, length); O(gv_track, width); O(gv_track, p00); O(gv_track, p01); O(gv_track, p11);
  printf("%zu ", sizeof(gv_track_config));
  O(gv_track_config, gate); O(gv_track_config, sigma_accel); O(gv_track_config, sigma_meas); O(gv_track_config, sigma_v0);
  O(gv_track_config, min_speed); O(gv_track_config, confirm_hits); O(gv_track_config, max_misses); O(gv_track_config, flags);
  printf("%zu ", sizeof(gv_track_info));
  O(gv_track_info, n_tracks); O(gv_track_info, n_confirmed); O(gv_track_info, n_exported); O(gv_track_info, n_matched);
  O(gv_track_info, n_born); O(gv_track_info, n_deleted); O(gv_track_info, n_dropped); O(gv_track_info, n_invalid);
  O(gv_track_info, next_id); O(gv_track_info, reserved);
  printf("%d %d\n", (int)GV_TRACK_DEVICE_DETS, (int)GV_TRACK_FEED_DYNAMIC);
  return 0;
}
"""

NAMES = ["gv_set_track_config", "gv_set_tracks", "gv_get_tracks", "gv_track_update_async", "gv_track_update", "gv_track_step"]
TRACK_FIELDS = ref.INT_FIELDS + ref.F64_FIELDS


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


def test_header_binding_and_layout(gvamd, tmp_path):
    txt = open(os.path.join(ROOT, "include", "gridvision_hip.h")).read()
    upd = (r"\(gv_handle h, const gv_lshape_pose \*dets, int32_t n, double dt,\s*const gv_transform \*motion /\* may be NULL \*/, "
           r"uint32_t flags, gv_track_info \*info /\* may be NULL \*/,\s*gv_track \*tracks /\* may be NULL, room for 128 \*/\);")
    for sig in (r"int gv_set_track_config\(gv_handle h, const gv_track_config \*cfg\);",
                r"int gv_set_tracks\(gv_handle h, const gv_track \*tracks, int32_t n, uint32_t next_id\);",
                r"int gv_get_tracks\(gv_handle h, gv_track \*out, int32_t cap, int32_t \*n, uint32_t \*next_id\);",
                r"int gv_track_update_async" + upd, r"int gv_track_update" + upd,
                r"int gv_track_step\(const gv_track_config \*cfg, gv_track \*tracks, int32_t \*n_tracks, uint32_t \*next_id,\s*"
                r"const gv_lshape_pose \*dets, int32_t n, double dt, const gv_transform \*motion"):
        assert re.search(sig, txt), sig
    for phrase in ("X14.", "WITHOUT motion THE VELOCITIES ARE RELATIVE TO THE VEHICLE", "p01' = (p01 + dt*p11) + q*(0.5*(dt2*dt))",
                   "(d2, s, d)", "S = p00 + r;  k0 = p00/S;  k1 = p01/S", "gv_set_track_config, gv_set_tracks, gv_get_tracks and gv_track_update*",
                   "gv_set_dyn_config, gv_set_moving_objects and gv_score_dynamic* may be called"):
        assert phrase in txt, phrase
    lib = gvamd.load()
    for name in NAMES:
        assert name in gvamd.ABI_SYMBOLS and hasattr(lib, name), name
    assert lib.gv_abi_version() == 4        # additive: the version stays
    declared = sorted(set(re.findall(r"\b(gv_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))))
    assert sorted(gvamd.ABI_SYMBOLS) == declared and len(declared) == 123
    assert "123 entry points" in open(os.path.join(ROOT, "README.md")).read()
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(LAYOUT)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", exe])
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    for dt in (gvamd.TRACK_DTYPE, ref.TRACK_DTYPE):
        assert dt.itemsize == out[0] == 128 and [dt.fields[n][1] for n in TRACK_FIELDS] == out[1:20]
        assert dt.names == TRACK_FIELDS
    assert C.sizeof(gvamd.TrackConfig) == out[20] == 56
    assert [getattr(gvamd.TrackConfig, n).offset for n, _ in gvamd.TrackConfig._fields_] == out[21:29]
    for dt in (gvamd.TRACK_INFO_DTYPE, ref.INFO_DTYPE):
        assert dt.itemsize == out[29] == 40 and [dt.fields[n][1] for n in dt.names] == out[30:40]
        assert dt.names == ref.INFO_FIELDS + ("next_id", "reserved")
    assert out[40:] == [gvamd.TRACK_DEVICE_DETS, gvamd.TRACK_FEED_DYNAMIC] == [1, 2]


def test_the_families_are_what_they_claim():
    names = {c["name"] for c in tc.cases()}
    assert names >= {"empty_both", "full_house", "ties_4", "chain_2", "chain_64", "chain_128", "gate_edge", "confirm_then_delete",
                     "max_misses_0_reuse", "id_wrap", "filter", "filter_sigma_accel_0", "ego_0", "ego_1", "ego_2", "ego_3",
                     "invalid_dets", "non_finite_states", "min_speed_edge"}
    w = tc.want(tc.by_name("full_house"))
    assert [int(r["info"][0]["n_born"]) for r in w] == [128, 0, 5, 2] and int(w[1]["info"][0]["n_dropped"]) == 128
    assert int(w[2]["info"][0]["n_deleted"]) == 128 and w[2]["tracks"]["slot"].tolist() == [0, 1, 2, 3, 4]
    c = tc.by_name("gate_edge")
    st = ref.unpack(c["tracks"])
    z = ref.det_list(c["steps"][0]["dets"])
    d2 = [(z[i]["px"] - st[i]["x"]) ** 2 + (z[i]["py"] - st[i]["y"]) ** 2 for i in range(2)]
    assert d2 == [2.25, math.nextafter(2.25, 3.0)] and c["cfg"]["gate"] ** 2 == 2.25
    w = tc.want(c)[0]
    assert w["tracks"]["det"].tolist() == [0, -1, 1] and w["tracks"]["id"].tolist() == [1, 2, 7]
    w = tc.want(tc.by_name("confirm_then_delete"))
    assert [int(r["info"][0]["n_exported"]) for r in w] == [0, 0, 1, 1, 1, 1, 0, 0]
    assert [int(r["info"][0]["n_tracks"]) for r in w] == [1, 1, 1, 1, 1, 1, 0, 0] and int(w[6]["info"][0]["n_deleted"]) == 1
    w = tc.want(tc.by_name("max_misses_0_reuse"))
    assert w[1]["tracks"]["id"].tolist() == [3, 2] and w[1]["tracks"]["slot"].tolist() == [0, 1]    # slot 0 freed and reused
    assert int(w[1]["info"][0]["n_deleted"]) == 1 and int(w[1]["info"][0]["n_born"]) == 1 and len(w[2]["tracks"]) == 0
    w = tc.want(tc.by_name("id_wrap"))[0]
    assert sorted(w["tracks"]["id"].tolist()) == [0, 1, 1, 0xFFFFFFFF] and w["next_id"] == 2
    w = tc.want(tc.by_name("saturate"))[0]
    assert w["tracks"]["hits"].tolist() == [ref.INT_MAX] and w["tracks"]["age"].tolist() == [ref.INT_MAX]
    w = tc.want(tc.by_name("invalid_dets"))
    assert [int(r["info"][0]["n_invalid"]) for r in w] == [26, 26] and int(w[0]["info"][0]["n_born"]) == 3
    w = tc.want(tc.by_name("non_finite_states"))
    assert [int(r["info"][0]["n_matched"]) for r in w] == [1, 5] and [int(r["info"][0]["n_exported"]) for r in w] == [1, 5]
    assert int(w[1]["info"][0]["n_confirmed"]) == 9
    w = tc.want(tc.by_name("min_speed_edge"))[0]
    assert w["objs"]["vx"].tolist() == [3.0, 0.0, 0.0] and w["objs"]["vy"].tolist() == [4.0, 0.0, 0.0]
    for k in range(4):
        for r in tc.want(tc.by_name(f"ego_{k}")):
            assert np.isfinite(r["tracks"]["x"]).all()
    for c in tc.cases():        # no step of any family makes a NaN that was not loaded
        loaded = any(np.isnan(c["tracks"][n]).any() for n in ref.F64_FIELDS)
        for r in tc.want(c):
            assert loaded or not any(np.isnan(r["tracks"][n]).any() for n in ref.F64_FIELDS), c["name"]


def _assoc_inputs(c):
    st = ref.unpack(c["tracks"])
    z = ref.det_list(c["steps"][0]["dets"])
    return ref.candidates(st, z, [True] * len(z), c["cfg"]["gate"] ** 2)


@pytest.mark.parametrize("name", ["ties_1", "ties_2", "ties_3", "ties_4", "chain_2", "chain_64", "chain_128"])
def test_parallel_rounds_equal_the_sorted_greedy(name):
    cands = _assoc_inputs(tc.by_name(name))
    want = ref.greedy(cands)
    got, n_rounds = ref.rounds(cands)
    assert got == want and len(want) > 0
    if name.startswith("chain_"):
        n = int(name.split("_")[1])
        assert n_rounds == n and want == {i: i for i in range(n)}      # one pair per round
    else:
        d2 = sorted(c[0] for c in cands)
        assert any(a == b for a, b in zip(d2, d2[1:]))                  # equal distances do occur
        rng = np.random.default_rng(5)
        for _ in range(3):                                               # no order of evaluation shows
            perm = [cands[i] for i in rng.permutation(len(cands))]
            assert ref.rounds(perm)[0] == want and ref.greedy(perm) == want


def _run_twin(gvamd, c):
    cfg = ref.to_struct(gvamd, c["cfg"])
    tracks, next_id, out = c["tracks"], c["next_id"], []
    for s in c["steps"]:
        tracks, next_id, info, objs = gvamd.track_step(cfg, tracks, next_id, s["dets"], s["dt"], s["motion"])
        out.append(dict(tracks=tracks, next_id=next_id, info=np.array([info]), objs=objs))
    return out


@pytest.mark.parametrize("name", [c["name"] for c in tc.cases()])
def test_host_twin_equals_the_reference(gvamd, name):
    c = tc.by_name(name)
    for k, (got, want) in enumerate(zip(_run_twin(gvamd, c), tc.want(c))):
        assert got["info"].tobytes() == want["info"].tobytes(), (name, k, got["info"], want["info"])
        assert got["next_id"] == want["next_id"], (name, k)
        assert got["tracks"].tobytes() == want["tracks"].tobytes(), (name, k)
        assert got["objs"].tobytes() == want["objs"].tobytes(), (name, k)


def test_argument_errors(gvamd):
    lib = gvamd.load()
    good = ref.config()
    for bad in (dict(gate=0.0), dict(gate=math.inf), dict(gate=math.nan), dict(sigma_accel=-1.0), dict(sigma_meas=0.0),
                dict(sigma_meas=math.nan), dict(sigma_v0=-0.5), dict(sigma_v0=math.inf), dict(min_speed=-1.0), dict(confirm_hits=0),
                dict(confirm_hits=256), dict(max_misses=-1), dict(max_misses=256), dict(flags=1)):
        with pytest.raises(gvamd.GVError) as e:
            gvamd.track_step(ref.to_struct(gvamd, dict(good, **bad)), None, 1, tc.boxes_at([(0.0, 0.0)]), 0.1)
        assert e.value.code == GV_ERR_BAD_ARG, bad
    cfg = ref.to_struct(gvamd, good)
    z = tc.boxes_at([(0.0, 0.0)])
    for dt in (-0.1, math.nan, math.inf):
        with pytest.raises(gvamd.GVError):
            gvamd.track_step(cfg, None, 1, z, dt)
    with pytest.raises(gvamd.GVError):
        gvamd.track_step(cfg, None, 1, z, 0.1, (0.0, 0.0, 0.0, 1.0, math.nan, 0.0, 0.0))
    for slots in ([1, 1], [2, 1], [-1, 0], [0, 128]):
        with pytest.raises(gvamd.GVError):
            gvamd.track_step(cfg, tc.tracks_at([(0.0, 0.0), (1.0, 1.0)], slots=slots), 1, z, 0.1)
    buf, n_t, nid = np.zeros(128, gvamd.TRACK_DTYPE), C.c_int32(0), C.c_uint32(1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    objs, n_o = np.zeros(128, gvamd.MOVING_OBJECT_DTYPE), C.c_int32(0)
    call = lambda *a: lib.gv_track_step(*a)
    assert call(None, p(buf), C.byref(n_t), C.byref(nid), p(z), 1, C.c_double(0.1), None, None, None, None) == GV_ERR_BAD_ARG
    assert call(C.byref(cfg), None, C.byref(n_t), C.byref(nid), p(z), 1, C.c_double(0.1), None, None, None, None) == GV_ERR_BAD_ARG
    assert call(C.byref(cfg), p(buf), C.byref(n_t), C.byref(nid), None, 1, C.c_double(0.1), None, None, None, None) == GV_ERR_BAD_ARG
    assert call(C.byref(cfg), p(buf), C.byref(n_t), C.byref(nid), p(z), 129, C.c_double(0.1), None, None, None, None) == GV_ERR_BAD_ARG
    assert call(C.byref(cfg), p(buf), C.byref(n_t), C.byref(nid), p(z), 1, C.c_double(0.1), None, None, p(objs), None) == GV_ERR_BAD_ARG
    assert n_t.value == 0 and nid.value == 1                     # nothing was done
    assert call(C.byref(cfg), p(buf), C.byref(n_t), C.byref(nid), p(z), 1, C.c_double(0.1), None, None, None, None) == 0
    assert n_t.value == 1 and nid.value == 2 and call(C.byref(cfg), p(buf), C.byref(n_t), C.byref(nid), None, 0, C.c_double(0.1),
                                                       None, None, p(objs), C.byref(n_o)) == 0


# ---- csrc/gv_track.hpp under the sanitizers: a program of its own reads the families from a file, runs track_step and
# prints one FNV-1a digest per case over the bytes the library gives for it
SAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "gv_track.hpp"
static uint64_t fnv(uint64_t h, const void *p, size_t n)
{
  const unsigned char *b = static_cast<const unsigned char *>(p);
  for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}
template <typename T> static bool rd(FILE *f, T *v, size_t n = 1) { return n == 0 || fread(v, sizeof(T), n, f) == n; }
int main(int argc, char **argv)
{
  FILE *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
  int32_t n_cases = 0;
  if (!f || !rd(f, &n_cases)) return 2;
  for (int32_t c = 0; c < n_cases; ++c) {
    gv_track_config cfg;
    int32_t n_tracks = 0, n_steps = 0;
    uint32_t next_id = 0;
    if (!rd(f, &cfg) || !rd(f, &n_tracks) || !rd(f, &next_id) || n_tracks < 0 || n_tracks > gv::kTrackSlots) return 2;
    std::vector<gv_track> in((size_t)n_tracks);
    if (!rd(f, in.data(), in.size()) || !rd(f, &n_steps)) return 2;
    std::vector<gv::TrackState> st(1);
    std::memset(st.data(), 0, sizeof(gv::TrackState));
    for (const gv_track &t : in) {
      if (t.slot < 0 || t.slot >= gv::kTrackSlots) return 2;
      st[0].t[t.slot] = t;
      st[0].live[t.slot] = 1;
    }
    st[0].next_id = next_id;
    const gv::TrackParams p = gv::track_params(cfg);
    uint64_t h = 14695981039346656037ull;
    for (int32_t s = 0; s < n_steps; ++s) {
      int32_t n = 0, has_motion = 0;
      double dt = 0.0;
      gv_transform m;
      if (!rd(f, &n) || !rd(f, &dt) || !rd(f, &has_motion) || !rd(f, &m) || n < 0 || n > gv::kTrackSlots) return 2;
      std::vector<gv_lshape_pose> dets((size_t)n);          // exactly n: a read past the end is the sanitizer's to find
      if (!rd(f, dets.data(), dets.size())) return 2;
      gv_track_info info;
      std::vector<gv_moving_object> objs((size_t)gv::kTrackSlots);
      int32_t n_objs = 0;
      gv::track_step(p, st[0], dets.data(), n, dt, has_motion ? &m : nullptr, &info, objs.data(), &n_objs);
      for (int32_t k = 0; k < gv::kTrackSlots; ++k)
        if (st[0].live[k]) h = fnv(h, &st[0].t[k], sizeof(gv_track));
      h = fnv(h, &info, sizeof(info));
      h = fnv(h, objs.data(), (size_t)n_objs * sizeof(gv_moving_object));
    }
    printf("%016llx\n", (unsigned long long)h);
  }
  fclose(f);
  return 0;
}
"""


def _fnv(h, b):
    for v in b:
        h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_shared_text_under_the_sanitizers(gvamd, tmp_path):
    cases = [c for c in tc.cases() if c["name"] in ("full_house", "ties_4", "chain_128", "invalid_dets", "non_finite_states", "id_wrap",
                                                    "ego_sequence", "max_misses_0_reuse")]
    blob = [struct.pack("<i", len(cases))]
    for c in cases:
        blob += [bytes(ref.to_struct(gvamd, c["cfg"])), struct.pack("<iI", len(c["tracks"]), c["next_id"]),
                 np.ascontiguousarray(c["tracks"], gvamd.TRACK_DTYPE).tobytes(), struct.pack("<i", len(c["steps"]))]
        for s in c["steps"]:
            m = s["motion"]
            blob += [struct.pack("<idi", len(s["dets"]), s["dt"], 0 if m is None else 1), struct.pack("<7d", *(m or [0.0] * 7)),
                     np.ascontiguousarray(s["dets"]).tobytes()]
    data, src, exe = str(tmp_path / "cases.bin"), str(tmp_path / "san.cpp"), str(tmp_path / "san")
    with open(data, "wb") as f:
        f.write(b"".join(blob))
    with open(src, "w") as f:
        f.write(SAN_MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "grid-vision_amd", "csrc"), src, "-o", exe])
    r = subprocess.run([exe, data], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    want = []
    for c in cases:
        h = 14695981039346656037
        for rec in _run_twin(gvamd, c):
            h = _fnv(h, rec["tracks"].tobytes() + rec["info"].tobytes() + rec["objs"].tobytes())
        want.append("%016x" % h)
    assert r.stdout.split() == want
