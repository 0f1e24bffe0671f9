"""The planner's host-only entry points (csrc/gv_api_planner_host.hip: the twins the GPU tests hold the device calls to,
and the host-built tables), no GPU: the file itself -- not a copy of its loops -- compiled as plain C++17 by the host
compiler under the address and undefined-behaviour sanitizers and linked with a small main, a program of its own that
reads a handful of tiny cases (K <= 8, P <= 16, 3 tracks) from a file and prints one FNV-1a digest per call.  The digests
must equal those of the same calls made through the shipped library."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import track_cases as tc
import track_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grid-vision_amd", "csrc")
K, P, CH, N_OBJ, SEED = 8, 16, 2, 3, 0x1234567890ABCDEF

SAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "gridvision_hip.h"
static uint64_t g_h;
static void begin() { g_h = 14695981039346656037ull; }
static void add(const void *p, size_t n)
{
  const unsigned char *b = static_cast<const unsigned char *>(p);
  for (size_t i = 0; i < n; ++i) g_h = (g_h ^ b[i]) * 1099511628211ull;
}
static void end(int rc) { printf("%d %016llx\n", rc, (unsigned long long)g_h); }
static FILE *f;
template <typename T> static void rd(T *v, size_t n = 1) { if (n && fread(v, sizeof(T), n, f) != n) exit(2); }
int main(int argc, char **argv)
{
  f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
  if (!f) return 2;
  int32_t K, P, C, n_obj, n_tracks, n_dets;
  uint64_t seed;
  uint32_t next_id;
  double res, start[3];
  float pose[3];
  gv_inflation infl; gv_footprint fp; gv_nav_config nav; gv_motion_model mm; gv_mppi_config mc; gv_mppi_limits ml;
  gv_dyn_config dc; gv_critic_weights w; gv_track_config tcfg;
  rd(&K); rd(&P); rd(&C); rd(&n_obj); rd(&n_tracks); rd(&n_dets); rd(&seed); rd(&next_id); rd(&res); rd(start, 3); rd(pose, 3);
  rd(&infl); rd(&fp); rd(&nav); rd(&mm); rd(&mc); rd(&ml); rd(&dc); rd(&w); rd(&tcfg);
  // exactly as long as the calls may read or write: a step past an end is the sanitizer's to find
  std::vector<float> nominal((size_t)P * C), controls((size_t)K * P * C), poses((size_t)K * P * 3), nom_out((size_t)P * C);
  std::vector<gv_moving_object> objs((size_t)n_obj);
  std::vector<gv_traj_score> traj((size_t)K);
  std::vector<gv_nav_score> navs((size_t)K);
  std::vector<gv_track> tracks(128);
  std::vector<gv_lshape_pose> dets((size_t)n_dets);
  rd(nominal.data(), nominal.size()); rd(objs.data(), objs.size()); rd(traj.data(), traj.size()); rd(navs.data(), navs.size());
  rd(tracks.data(), (size_t)n_tracks); rd(dets.data(), dets.size());
  fclose(f);

  int32_t n = 0;
  int rc = gv_inflation_cost_table(&infl, res, nullptr, 0, &n);      // the length first, as a caller would
  std::vector<uint8_t> table((size_t)n);
  begin(); rc = gv_inflation_cost_table(&infl, res, table.data(), n, &n); add(&n, 4); add(table.data(), table.size()); end(rc);
  rc = gv_footprint_cells(8, 8, res, &fp, pose[0], pose[1], pose[2], nullptr, 0, &n);
  std::vector<int32_t> cells((size_t)(n > 0 ? n : 0));
  begin(); rc = gv_footprint_cells(8, 8, res, &fp, pose[0], pose[1], pose[2], cells.data(), n, &n); add(&n, 4); add(cells.data(), cells.size() * 4); end(rc);
  std::vector<uint32_t> steps(256);
  begin(); rc = gv_nav_step_table(&nav, steps.data()); add(steps.data(), 1024); end(rc);
  uint32_t words[4];
  begin(); rc = gv_mppi_words(seed, 1, 2, 3, words); add(words, 16); end(rc);
  begin(); rc = gv_mppi_sample_controls(&mc, C, nominal.data(), K, P, seed, 0, GV_MPPI_SHIFT, controls.data()); add(controls.data(), controls.size() * 4); end(rc);
  begin(); rc = gv_mppi_constrain(&ml, &mm, controls.data(), K, P); add(controls.data(), controls.size() * 4); end(rc);
  std::vector<double> g((size_t)K);
  begin(); rc = gv_mppi_control_costs(&mc, &ml, C, controls.data(), nominal.data(), K, P, GV_MPPI_SHIFT, g.data()); add(g.data(), g.size() * 8); end(rc);
  begin(); rc = gv_rollout_poses(&mm, start, controls.data(), K, P, 0, poses.data()); add(poses.data(), poses.size() * 4); end(rc);
  std::vector<float> held((size_t)K * P * 3);
  begin(); rc = gv_rollout_poses(&mm, start, controls.data(), K, P, GV_ROLLOUT_CONSTANT, held.data()); add(held.data(), held.size() * 4); end(rc);
  rc = gv_dyn_cost_table(&dc, nullptr, 0, &n);
  std::vector<uint8_t> dtable((size_t)n);
  begin(); rc = gv_dyn_cost_table(&dc, dtable.data(), n, &n); add(&n, 4); add(dtable.data(), dtable.size()); end(rc);
  std::vector<gv_dyn_score> dyn((size_t)K);
  std::vector<uint8_t> pose_cost((size_t)K * P);
  begin(); rc = gv_dyn_score_poses(&dc, objs.data(), n_obj, poses.data(), K, P, dyn.data(), pose_cost.data());
  add(dyn.data(), dyn.size() * sizeof(gv_dyn_score)); add(pose_cost.data(), pose_cost.size()); end(rc);
  begin(); rc = gv_dyn_score_poses(&dc, nullptr, 0, poses.data(), K, P, dyn.data(), nullptr); add(dyn.data(), dyn.size() * sizeof(gv_dyn_score)); end(rc);
  gv_control_result result;
  std::vector<uint64_t> totals((size_t)K);
  begin(); rc = gv_control_select(&w, traj.data(), navs.data(), K, &result, nullptr); add(&result, sizeof(result)); end(rc);
  begin(); rc = gv_control_select_dyn(&w, traj.data(), navs.data(), dyn.data(), &dc, K, &result, totals.data());
  add(&result, sizeof(result)); add(totals.data(), totals.size() * 8); end(rc);
  begin(); rc = gv_mppi_average(&mc, C, controls.data(), totals.data(), K, P, nominal.data(), nom_out.data()); add(nom_out.data(), nom_out.size() * 4); end(rc);
  begin(); rc = gv_mppi_average_cc(&mc, C, controls.data(), totals.data(), g.data(), K, P, nominal.data(), nom_out.data()); add(nom_out.data(), nom_out.size() * 4); end(rc);
  for (uint64_t &t : totals) t = UINT64_MAX;                          // every trajectory rejected: the nominal stays
  begin(); rc = gv_mppi_average_cc(&mc, C, controls.data(), totals.data(), g.data(), K, P, nominal.data(), nom_out.data()); add(nom_out.data(), nom_out.size() * 4); end(rc);
  std::vector<gv_moving_object> out_objs(128);
  for (int step = 0; step < 2; ++step) {
    gv_track_info info;
    int32_t n_objs = 0;
    begin(); rc = gv_track_step(&tcfg, tracks.data(), &n_tracks, &next_id, dets.data(), step ? 0 : n_dets, 0.05, nullptr, &info, out_objs.data(), &n_objs);
    add(&n_tracks, 4); add(&next_id, 4); add(tracks.data(), (size_t)n_tracks * sizeof(gv_track)); add(&info, sizeof(info));
    add(out_objs.data(), (size_t)n_objs * sizeof(gv_moving_object)); end(rc);
  }
  begin(); rc = gv_mppi_constrain(&ml, &mm, controls.data(), 1 << 20, 4096); end(rc);   // the shape rule: refused, nothing read
  return 0;
}
"""


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


def _inputs(gvamd):
    rng = np.random.default_rng(12)
    nominal = np.stack([rng.uniform(0.5, 1.5, P), rng.uniform(-0.4, 0.4, P)], axis=1).astype(np.float32)
    objs = gvamd.moving_objects(np.array([[1.0 + j, 0.5 * j - 0.5, 0.3 * j, 4.0, 2.0, 0.5, -0.25 * j] for j in range(N_OBJ)]))
    traj = np.zeros(K, gvamd.TRAJ_SCORE_DTYPE)
    traj["max_cost"], traj["cost_sum"] = rng.integers(0, 253, K), rng.integers(0, 4000, K)
    traj["first_collision"], traj["n_off_map"] = -1, 0
    traj["first_collision"][2], traj["max_cost"][2] = 5, 254                      # one trajectory collides
    nav = np.zeros(K, gvamd.NAV_SCORE_DTYPE)
    nav["sum"], nav["last"], nav["best"], nav["best_pose"] = rng.integers(0, 90000, K), rng.integers(0, 5000, K), rng.integers(0, 5000, K), P - 1
    nav["n_bad"][5] = 1                                                          # and one leaves the field
    case = tc.by_name("ties_4")
    tracks, dets = np.ascontiguousarray(case["tracks"], gvamd.TRACK_DTYPE)[:3], np.ascontiguousarray(case["steps"][0]["dets"])[:3]
    return dict(
        res=0.1, start=(0.5, -0.25, 0.2), pose=(0.4, -0.3, 0.7), next_id=case["next_id"],
        infl=gvamd.Inflation(0.35, 0.75, 6.0, 65, 0), fp=gvamd.Footprint.of(((0.6, 0.3), (-0.4, 0.3), (-0.4, -0.3), (0.6, -0.3))),
        nav=gvamd.NavConfig(253, 3, 0), mm=gvamd.MotionModel(gvamd.MOTION_DIFF, 0.1, 0),
        mc=gvamd.MppiConfig.of((0.3, 0.4), (-0.5, -1.5), (3.0, 1.5), 30.0),
        ml=gvamd.MppiLimits.of(rate_up=(2.0, 3.0), rate_down=(3.0, 3.0), u_prev=(1.0, 0.0), min_turn_radius=1.5, gamma=0.05),
        dc=gvamd.DynConfig.of(off_x=(-0.3, 0.3), radius=0.4, influence_radius=1.5, cost_scaling_factor=2.0, quantum=0.05, t0=0.1, dt=0.1,
                              collision_cost=253, w_sum=1, w_max=2),
        w=gvamd.CriticWeights(1, 2, 4, 0, 1, 0), tcfg=track_ref.to_struct(gvamd, case["cfg"]),
        nominal=nominal, objs=objs, traj=traj, navs=nav, tracks=tracks, dets=dets)


def _fnv(*parts):
    h = 14695981039346656037
    for b in b"".join(bytes(p) for p in parts):
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def _library_digests(gvamd, d):
    """the calls of SAN_MAIN in its order, through the shipped library"""
    lib = gvamd.load()
    i32, u32, u64, f64, f32 = C.c_int32, C.c_uint32, C.c_uint64, C.c_double, C.c_float
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    ref = C.byref
    out = []
    emit = lambda rc, *parts: out.append("%d %s" % (rc, _fnv(*parts)))   # noqa: E731
    n = i32(0)
    lib.gv_inflation_cost_table(ref(d["infl"]), f64(d["res"]), None, i32(0), ref(n))
    table = np.zeros(n.value, np.uint8)
    emit(lib.gv_inflation_cost_table(ref(d["infl"]), f64(d["res"]), p(table), n, ref(n)), n, table)
    pose = [f32(v) for v in d["pose"]]
    lib.gv_footprint_cells(C.c_uint8(8), C.c_uint8(8), f64(d["res"]), ref(d["fp"]), *pose, None, i32(0), ref(n))
    cells = np.zeros(max(n.value, 0), np.int32)
    emit(lib.gv_footprint_cells(C.c_uint8(8), C.c_uint8(8), f64(d["res"]), ref(d["fp"]), *pose, p(cells), n, ref(n)), n, cells)
    steps = np.zeros(256, np.uint32)
    emit(lib.gv_nav_step_table(ref(d["nav"]), p(steps)), steps)
    words = np.zeros(4, np.uint32)
    emit(lib.gv_mppi_words(u64(SEED), u64(1), u32(2), u32(3), p(words)), words)
    nominal, controls = d["nominal"], np.zeros((K, P, CH), np.float32)
    shift = u32(gvamd.MPPI_SHIFT)
    emit(lib.gv_mppi_sample_controls(ref(d["mc"]), i32(CH), p(nominal), i32(K), i32(P), u64(SEED), u64(0), shift, p(controls)), controls)
    emit(lib.gv_mppi_constrain(ref(d["ml"]), ref(d["mm"]), p(controls), i32(K), i32(P)), controls)
    g = np.zeros(K, np.float64)
    emit(lib.gv_mppi_control_costs(ref(d["mc"]), ref(d["ml"]), i32(CH), p(controls), p(nominal), i32(K), i32(P), shift, p(g)), g)
    start = (f64 * 3)(*d["start"])
    poses, held = np.zeros((K, P, 3), np.float32), np.zeros((K, P, 3), np.float32)
    emit(lib.gv_rollout_poses(ref(d["mm"]), start, p(controls), i32(K), i32(P), u32(0), p(poses)), poses)
    emit(lib.gv_rollout_poses(ref(d["mm"]), start, p(controls), i32(K), i32(P), u32(gvamd.ROLLOUT_CONSTANT), p(held)), held)
    lib.gv_dyn_cost_table(ref(d["dc"]), None, i32(0), ref(n))
    dtable = np.zeros(n.value, np.uint8)
    emit(lib.gv_dyn_cost_table(ref(d["dc"]), p(dtable), n, ref(n)), n, dtable)
    dyn, pose_cost = np.zeros(K, gvamd.DYN_SCORE_DTYPE), np.zeros(K * P, np.uint8)
    emit(lib.gv_dyn_score_poses(ref(d["dc"]), p(d["objs"]), i32(N_OBJ), p(poses), i32(K), i32(P), p(dyn), p(pose_cost)), dyn, pose_cost)
    emit(lib.gv_dyn_score_poses(ref(d["dc"]), None, i32(0), p(poses), i32(K), i32(P), p(dyn), None), dyn)
    result, totals = np.zeros(1, gvamd.CONTROL_RESULT_DTYPE), np.zeros(K, np.uint64)
    emit(lib.gv_control_select(ref(d["w"]), p(d["traj"]), p(d["navs"]), i32(K), p(result), None), result)
    emit(lib.gv_control_select_dyn(ref(d["w"]), p(d["traj"]), p(d["navs"]), p(dyn), ref(d["dc"]), i32(K), p(result), p(totals)), result, totals)
    assert result["n_valid"][0] == K - 2 and totals[2] == totals[5] == np.iinfo(np.uint64).max      # the cases are what they claim
    nom_out = np.zeros((P, CH), np.float32)
    emit(lib.gv_mppi_average(ref(d["mc"]), i32(CH), p(controls), p(totals), i32(K), i32(P), p(nominal), p(nom_out)), nom_out)
    emit(lib.gv_mppi_average_cc(ref(d["mc"]), i32(CH), p(controls), p(totals), p(g), i32(K), i32(P), p(nominal), p(nom_out)), nom_out)
    totals[:] = np.iinfo(np.uint64).max
    emit(lib.gv_mppi_average_cc(ref(d["mc"]), i32(CH), p(controls), p(totals), p(g), i32(K), i32(P), p(nominal), p(nom_out)), nom_out)
    assert nom_out.tobytes() == nominal.tobytes()
    tracks = np.zeros(128, gvamd.TRACK_DTYPE)
    tracks[:len(d["tracks"])] = d["tracks"]
    n_tracks, next_id, out_objs = i32(len(d["tracks"])), u32(d["next_id"]), np.zeros(128, gvamd.MOVING_OBJECT_DTYPE)
    for step in range(2):
        info, n_objs = np.zeros(1, gvamd.TRACK_INFO_DTYPE), i32(0)
        rc = lib.gv_track_step(ref(d["tcfg"]), p(tracks), ref(n_tracks), ref(next_id), p(d["dets"]), i32(0 if step else len(d["dets"])),
                               f64(0.05), None, p(info), p(out_objs), ref(n_objs))
        emit(rc, n_tracks, next_id, tracks[:n_tracks.value], info, out_objs[:n_objs.value])
    emit(lib.gv_mppi_constrain(ref(d["ml"]), ref(d["mm"]), p(controls), i32(1 << 20), i32(4096)))
    return out


def test_host_file_under_the_sanitizers(gvamd, tmp_path):
    d = _inputs(gvamd)
    head = np.array([K, P, CH, N_OBJ, len(d["tracks"]), len(d["dets"])], np.int32).tobytes() + np.uint64(SEED).tobytes() + \
        np.uint32(d["next_id"]).tobytes() + np.array((d["res"],) + d["start"], np.float64).tobytes() + np.array(d["pose"], np.float32).tobytes()
    structs = b"".join(bytes(d[k]) for k in ("infl", "fp", "nav", "mm", "mc", "ml", "dc", "w", "tcfg"))
    arrays = b"".join(np.ascontiguousarray(d[k]).tobytes() for k in ("nominal", "objs", "traj", "navs", "tracks", "dets"))
    data, src, exe = str(tmp_path / "cases.bin"), str(tmp_path / "main.cpp"), str(tmp_path / "twins")
    with open(data, "wb") as f:
        f.write(head + structs + arrays)
    with open(src, "w") as f:
        f.write(SAN_MAIN)
    san = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(san + ["-I" + os.path.join(ROOT, "include"), src, "-x", "c++", os.path.join(CSRC, "gv_api_planner_host.hip"), "-o", exe])
    r = subprocess.run([exe, data], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got, want = r.stdout.strip().split("\n"), _library_digests(gvamd, d)
    assert len(got) == 20 and got[-1].startswith("1 ") and all(g.startswith("0 ") for g in got[:-1])     # GV_ERR_BAD_ARG is 1
    assert got == want
