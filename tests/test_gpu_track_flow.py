"""[EXTENSION] X14 in the frame flow (FlowParams::track_objects with ego_motion): a tick that does not reach the tracker
(missing inputs) still moves the grid, so its motion and its dt are owed to the tracker's next update.

One C++ program over frame_flow.hpp, two modes.  `host` (no GPU): compose_motion against applying the two motions one
after the other, through the library's host twin.  `flow` (GPU): five ticks, two of them skipped, with tracks loaded
beforehand; the resident tracks must equal gv_track_step given the composed motion byte for byte, and the set the flow
fed to X13 must score like the twin's exported objects."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "grid-vision_amd")

MAIN = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "grid_vision/frame_flow.hpp"
using grid_vision::compose_motion;

static gv_transform planar(double yaw, double tx, double ty)
{
  gv_transform m{};
  m.qz = std::sin(0.5 * yaw); m.qw = std::cos(0.5 * yaw);
  m.tx = tx; m.ty = ty; m.tz = 0.0;
  return m;
}

static std::vector<gv_track> some_tracks()
{
  const double xy[3][4] = {{5.0, 1.0, 2.0, 0.0}, {9.0, -2.0, 0.0, -1.5}, {-4.0, 6.0, 0.5, 0.5}};
  std::vector<gv_track> t(3);
  for (int i = 0; i < 3; ++i) {
    t[i] = gv_track{};
    t[i].id = 1u + (uint32_t)i; t[i].slot = 2 * i; t[i].hits = 5; t[i].det = -1;
    t[i].x = xy[i][0]; t[i].y = xy[i][1]; t[i].vx = xy[i][2]; t[i].vy = xy[i][3];
    t[i].qz = std::sin(0.1 * i); t[i].qw = std::cos(0.1 * i);
    t[i].length = 4.5; t[i].width = 2.0;
    t[i].p00 = 0.05; t[i].p01 = 0.02; t[i].p11 = 0.5;
  }
  return t;
}

static int host_mode()
{
  const grid_vision::FlowParams p;
  const gv_transform a = planar(0.07, 0.4, -0.1), b = planar(-0.03, 0.25, 0.05);
  const std::vector<LShapePose> none;
  // b is the later tick's motion: one after the other (b's step second) against the product, dt = 0
  std::vector<gv_track> seq = some_tracks(), one = some_tracks();
  uint32_t id = 10;
  OccupancyGridMap::trackStep(p.track, seq, id, none, 0.0, &a);
  OccupancyGridMap::trackStep(p.track, seq, id, none, 0.0, &b);
  const gv_transform ab = compose_motion(a, b);
  OccupancyGridMap::trackStep(p.track, one, id, none, 0.0, &ab);
  double worst = 0.0;
  for (size_t i = 0; i < seq.size(); ++i) {
    const double d[] = {seq[i].x - one[i].x, seq[i].y - one[i].y, seq[i].vx - one[i].vx, seq[i].vy - one[i].vy,
                        seq[i].qz - one[i].qz, seq[i].qw - one[i].qw};
    for (double v : d) worst = std::fmax(worst, std::fabs(v));
  }
  // and the other order is another motion
  const gv_transform ba = compose_motion(b, a);
  const double other = std::fabs(ab.tx - ba.tx) + std::fabs(ab.ty - ba.ty);
  std::printf("composition differs from two steps by %.3e, from the other order by %.3e\n", worst, other);
  // a quarter turn about z then a step: known answer.  first = quarter turn with t = (1, 0), second = t (2, 0):
  // R(90 deg) (2, 0) + (1, 0) = (1, 2)
  const gv_transform q = compose_motion(planar(0.5 * M_PI, 1.0, 0.0), planar(0.0, 2.0, 0.0));
  const bool known = std::fabs(q.tx - 1.0) < 1e-15 && std::fabs(q.ty - 2.0) < 1e-15 && std::fabs(q.qz - std::sin(0.25 * M_PI)) < 1e-15;
  const bool ok = seq.size() == 3 && worst < 1e-13 && other > 1e-3 && known;
  std::printf("compose check %s\n", ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}

static int flow_mode()
{
  const CAMParams cam{224, 224, 480, 640, 320.f, 320.f, 320.f, 240.f};
  GridVisionContext ctx(50, 20, 0.1, cam);
  OccupancyGridMap grid(ctx);
  grid_vision::FlowParams p;
  p.ego_motion = true;
  p.track_objects = true;
  p.fused = false;
  grid_vision::FrameFlow flow(ctx, grid, p);
  gv_dyn_config dyn{};
  dyn.n_circles = 1; dyn.radius = 0.4; dyn.influence_radius = 2.0; dyn.cost_scaling_factor = 2.0; dyn.quantum = 0.05;
  dyn.t0 = 0.25; dyn.dt = 0.25; dyn.collision_cost = 253; dyn.w_sum = 1;
  grid.setDynConfig(dyn);
  grid.setTracks(some_tracks(), 10);

  const gv_transform mA = planar(0.02, 0.30, 0.01), mB = planar(0.05, 0.45, -0.04), mC = planar(-0.01, 0.35, 0.02);
  struct Tick { bool inputs; const gv_transform *motion; double dt; };
  const Tick ticks[] = {{true, &mA, 0.05}, {false, &mB, 0.05}, {true, &mC, 0.07}, {false, nullptr, 0.05}, {true, nullptr, 0.05}};
  const char *want_branch[] = {"no_detections", "missing_inputs", "no_detections", "missing_inputs", "no_detections"};
  bool branches = true;
  for (int i = 0; i < 5; ++i) {
    grid_vision::TickInput in;
    in.have_image = ticks[i].inputs;
    in.motion = ticks[i].motion;
    in.dt = ticks[i].dt;
    const grid_vision::TickResult r = flow.tick(in);
    branches = branches && std::strcmp(grid_vision::branch_name(r.branch), want_branch[i]) == 0;
  }
  uint32_t next_id = 0;
  const std::vector<gv_track> got = grid.getTracks(&next_id);

  // the twin: three updates; the second is owed the skipped tick's time and motion
  std::vector<gv_track> twin = some_tracks(), lost = some_tracks();
  std::vector<gv_moving_object> objs;
  const std::vector<LShapePose> none;
  uint32_t id = 10, id2 = 10;
  double dt1 = 0.0, dt2 = 0.0, dt3 = 0.0;
  dt1 += 0.05;
  dt2 += 0.05; dt2 += 0.07;
  dt3 += 0.05; dt3 += 0.05;
  const gv_transform mBC = compose_motion(mB, mC);
  OccupancyGridMap::trackStep(p.track, twin, id, none, dt1, &mA);
  OccupancyGridMap::trackStep(p.track, twin, id, none, dt2, &mBC);
  OccupancyGridMap::trackStep(p.track, twin, id, none, dt3, nullptr, &objs);
  OccupancyGridMap::trackStep(p.track, lost, id2, none, dt1, &mA);      // what dropping the skipped tick's motion gives
  OccupancyGridMap::trackStep(p.track, lost, id2, none, dt2, &mC);
  OccupancyGridMap::trackStep(p.track, lost, id2, none, dt3, nullptr);
  const bool same = got.size() == twin.size() && next_id == id && std::memcmp(got.data(), twin.data(), got.size() * sizeof(gv_track)) == 0;
  const bool not_lost = got.size() == lost.size() && std::fabs(got[0].x - lost[0].x) > 0.1;

  // the fed set scores like the twin's objects
  const int32_t K = 4, P = 12;
  std::vector<float> poses;
  for (int32_t k = 0; k < K; ++k)
    for (int32_t q = 0; q < P; ++q) {
      poses.push_back(0.8f * (float)q);
      poses.push_back(-3.0f + 2.0f * (float)k);
      poses.push_back(0.0f);
    }
  const std::vector<gv_dyn_score> rec = grid.scoreDynamic(poses, K, P);
  std::vector<gv_dyn_score> host((size_t)K);
  gv::check(gv_dyn_score_poses(&dyn, objs.data(), (int32_t)objs.size(), poses.data(), K, P, host.data(), nullptr), nullptr, "gv_dyn_score_poses");
  const bool fed = objs.size() == 3 && std::memcmp(rec.data(), host.data(), rec.size() * sizeof(gv_dyn_score)) == 0;
  bool touched = false;
  for (const gv_dyn_score &s : rec) touched = touched || s.max_cost > 0;
  std::printf("branches %s, %zu tracks %s the twin's with the composed motion (%.3f m from the twin without it), fed set %s\n",
              branches ? "as expected" : "UNEXPECTED", got.size(), same ? "equal" : "DIFFER FROM", got.empty() ? 0.0 : std::fabs(got[0].x - lost[0].x),
              fed ? "scores like the twin's objects" : "SCORES DIFFERENTLY");
  const bool ok = branches && same && not_lost && fed && touched;
  std::printf("flow track check %s\n", ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}

int main(int argc, char **argv)
{
  try {
    return argc > 1 && std::strcmp(argv[1], "flow") == 0 ? flow_mode() : host_mode();
  } catch (const gv::Error &e) {
    std::fprintf(stderr, "gv error %d: %s\n", e.code, e.what());
    return 2;
  }
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import gvamd
    gvamd.load()
    d = tmp_path_factory.mktemp("track_flow")
    src, out = str(d / "track_flow.cpp"), str(d / "track_flow")
    with open(src, "w") as f:
        f.write(MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(PKG, "include"), src, "-o", out,
                           "-L" + PKG, "-lgridvision_hip", "-Wl,-rpath," + PKG])
    return out


def test_compose_motion_on_the_host(exe):
    r = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "compose check ok" in r.stdout, (r.stdout, r.stderr)


@pytest.mark.gpu
def test_flow_owes_the_tracker_the_skipped_ticks(exe):
    r = subprocess.run([exe, "flow"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "branches as expected, 3 tracks equal the twin's with the composed motion" in r.stdout, r.stdout
    assert "fed set scores like the twin's objects" in r.stdout and "flow track check ok" in r.stdout, r.stdout
