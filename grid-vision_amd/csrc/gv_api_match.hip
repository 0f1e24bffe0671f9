// gv_api_match.hip -- [EXTENSION] X16 scan-to-costmap matching behind the C ABI of include/gridvision_hip_match.h:
// the handle's configuration, the device call (gv_match_scan_async / gv_match_scan: kernels of gv_match.hip on the
// public stream), and the host-only functions: the twin gv_match_scan_host (gv_match.hpp's text in sequential loops:
// what the GPU tests hold the device call to), the rotation table and the motion of a result.
#include <cmath>
#include <cstring>
#include <vector>

#include "gv_context.hpp"

namespace {

bool match_config_valid(const gv_match_config &c)
{
  const auto half_ok = [](int32_t w) { return w >= 0 && w <= kMatchMaxHalf; };
  return half_ok(c.wx) && half_ok(c.wy) && half_ok(c.wt) && std::isfinite(c.yaw_step) && c.yaw_step >= 0.0 &&
         (c.wt == 0 || c.yaw_step > 0.0) && c.stride >= 1 && c.stride <= kMatchMaxStride && c.min_points >= 1 &&
         (c.flags & ~(uint32_t)GV_MATCH_USE_BAND) == 0;
}

bool match_guess_valid(const gv_match_guess *q) { return q && std::isfinite(q->x) && std::isfinite(q->y) && std::isfinite(q->yaw); }

// what every form of the call refuses alike
bool match_call_ok(const gv_match_guess *guess, uint32_t flags, const gv_match_result *result, const uint32_t *scores)
{
  return match_guess_valid(guess) && result && (flags & ~(uint32_t)GV_MATCH_KEEP_SCORES) == 0 &&
         (!(flags & GV_MATCH_KEEP_SCORES) || scores);
}

MatchParams match_params(const gv_match_config &c, const gv_match_guess &q)
{
  MatchParams p{};
  p.wx = c.wx; p.wy = c.wy; p.wt = c.wt;
  p.stride = c.stride;
  p.min_points = c.min_points;
  p.use_band = (c.flags & GV_MATCH_USE_BAND) ? 1u : 0u;
  p.x = q.x; p.y = q.y; p.yaw = q.yaw;
  p.yaw_step = c.yaw_step;
  return p;
}

// (c_t, s_t): libm in fp64, rounded once
void match_rotations(const MatchParams &p, float *table)
{
  for (int32_t t = 0; t < match_nt(p); ++t) {
    const double th = match_theta(p, t);
    table[2 * t] = (float)std::cos(th);
    table[2 * t + 1] = (float)std::sin(th);
  }
}

size_t match_selected(size_t n, int32_t stride) { return (n + (size_t)stride - 1) / (size_t)stride; }

}  // namespace

extern "C" {

// handle configuration only; every call copies it into its kernel arguments
int gv_set_match_config(gv_handle h, const gv_match_config *cfg)
{
  if (!h) return GV_ERR_BAD_ARG;
  if (cfg && !match_config_valid(*cfg)) return GV_ERR_BAD_ARG;
  if (cfg) h->match.cfg = *cfg;
  h->match.set = cfg != nullptr;
  return GV_OK;
}

// One memset, three kernels and a copy per destination the device cannot write in place, all on the public stream:
// behind the last gv_inflate, and behind the upload of the cloud it reads (one event wait per upload, as a frame's).
int gv_match_scan_async(gv_handle h, const gv_match_guess *guess, uint32_t flags, gv_match_result *result, uint32_t *scores)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!match_call_ok(guess, flags, result, scores)) return GV_ERR_BAD_ARG;
  if (!h->has_bl) return GV_ERR_TF;
  gv_context::Match &m = h->match;
  const char *missing = !m.set ? "no configuration set (gv_set_match_config)" : (h->n == 0 ? "no cloud" : nullptr);
  int rc = refuse_state(h, "gv_match_scan", missing, kNeedCostmap, "there is no whole costmap");
  if (rc) return rc;
  const size_t n_sel = match_selected(h->n, m.cfg.stride);
  if (n_sel > (size_t)kMatchMaxSelected) return state_error(h, "gv_match_scan", "more than 2^24 selected points");
  if ((rc = set_device_only(h))) return rc;

  MatchArgs a{};
  a.g = h->g;
  a.p = match_params(m.cfg, *guess);
  a.m_base = h->m_base;
  a.band = h->band;
  a.x = h->cx; a.y = h->cy; a.z = h->cz;
  a.n = (uint32_t)h->n;
  a.n_sel = (uint32_t)n_sel;
  match_rotations(a.p, a.rot);
  const size_t total = (size_t)match_nt(a.p) * (size_t)match_ny(a.p) * (size_t)match_nx(a.p);
  const size_t words = (size_t)kMatchHeadWords + total;
  const bool keep = (flags & GV_MATCH_KEEP_SCORES) != 0;
  ResultDest<gv_match_result> to_result;
  if ((rc = m.pts.reserve(h, n_sel)) || (rc = m.head.reserve(h, words)) || (rc = to_result.open(h, result, 1, 8, m.d_result)))
    return rc;
  if (!m.read) GV_HIP(m.read.create(hipEventDisableTiming));
  a.pts = m.pts;
  a.head = m.head;
  a.cost = h->infl.cost;
  a.result = to_result.dev;
  a.scores_out = keep ? static_cast<uint32_t *>(pinned_device_view(scores, sizeof(uint32_t))) : nullptr;

  CloudSet &C = h->cloud[h->cloud_cur];
  if (!(C.seen & 1u)) {   // the public stream reads this cloud for the first time: behind its upload
    GV_HIP(hipStreamWaitEvent(h->stream, C.ready, 0));
    C.seen |= 1u;
    h->sb[0].lane_clean = false;
  }
  GV_HIP(hipMemsetAsync(m.head, 0, words * sizeof(uint32_t), h->stream));
  launch_match_points(a, h->stream);
  GV_HIP(hipEventRecord(m.read, h->stream));   // the cloud's last reader of this call: an upload into the set waits for it
  m.clouds |= 1u << h->cloud_cur;
  launch_match_score(a, h->stream);
  launch_match_select(a, h->stream);
  GV_HIP(hipGetLastError());
  if ((rc = to_result.copy_back(h))) return rc;
  if (keep && !a.scores_out)
    GV_HIP(hipMemcpyAsync(scores, m.head.get() + kMatchHeadWords, total * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  return GV_OK;
  GV_CATCH
}

int gv_match_scan(gv_handle h, const gv_match_guess *guess, uint32_t flags, gv_match_result *result, uint32_t *scores)
{
  return wait_scored(h, gv_match_scan_async(h, guess, flags, result, scores), 1);
}

// ---- host only: no handle, nothing enqueued

// The definition in sequential loops: the used points in index order; for every yaw candidate their cells, and every
// point adds its window into the volume, row by row (a window that lies on the map whole needs no test per cell);
// then the selection over the volume in linear order.
int gv_match_scan_host(uint8_t grid_x, uint8_t grid_y, double resolution, const uint8_t *cost, const float *x, const float *y,
                       const float *z, size_t n, const gv_transform *base_from_lidar, const gv_height_band *band,
                       const gv_match_config *cfg, const gv_match_guess *guess, uint32_t flags, gv_match_result *result,
                       uint32_t *scores)
{
  if (!cost || (n && (!x || !y || !z)) || !base_from_lidar || !cfg || !match_config_valid(*cfg) ||
      !match_call_ok(guess, flags, result, scores))
    return GV_ERR_BAD_ARG;
  if (band && (std::isnan(band->z_ground) || std::isnan(band->z_max) || band->z_ground > band->z_max)) return GV_ERR_BAD_ARG;
  try {
    GridParams g{};
    if (!host::grid_params(grid_x, grid_y, resolution, g)) return GV_ERR_BAD_ARG;
    if (match_selected(n, cfg->stride) > (size_t)kMatchMaxSelected) return GV_ERR_BAD_ARG;
    const MatchParams p = match_params(*cfg, *guess);
    const Mat34f mb = host::pcl_matrix_from_tf(*base_from_lidar);
    const HeightBand hb = band ? HeightBand{band->z_ground, band->z_max, 0} : HeightBand{-INFINITY, INFINITY, 0};
    std::vector<float> bxs, bys;
    for (size_t i = 0; i < n; i += (size_t)p.stride) {
      float bx, by, bz;
      match_base_point(mb, x[i], y[i], z[i], bx, by, bz);
      if (match_used(bx, by, bz, p.use_band, hb)) {
        bxs.push_back(bx);
        bys.push_back(by);
      }
    }
    const int32_t NT = match_nt(p), NY = match_ny(p), NX = match_nx(p);
    float rot[2 * kMatchMaxSide];
    match_rotations(p, rot);
    std::vector<uint32_t> vol((size_t)NT * (size_t)NY * (size_t)NX, 0u);
    for (int32_t t = 0; t < NT; ++t) {
      uint32_t *v = vol.data() + (size_t)t * (size_t)NY * (size_t)NX;
      for (size_t q = 0; q < bxs.size(); ++q) {
        int32_t ux = 0, uy = 0;
        if (!match_cell(g, p, rot[2 * t], rot[2 * t + 1], bxs[q], bys[q], ux, uy)) continue;
        const bool inside = ux - p.wx >= 0 && uy - p.wy >= 0 && ux + p.wx < g.nx && uy + p.wy < g.ny;
        for (int32_t j = -p.wy; j <= p.wy; ++j) {
          uint32_t *row = v + (size_t)(j + p.wy) * (size_t)NX + (size_t)p.wx;
          if (inside) {
            const uint8_t *c = cost + data_entry(g, ux, uy + j);   // cell (ux + i, uy + j) is entry c[-i]
            for (int32_t i = -p.wx; i <= p.wx; ++i) row[i] += (uint32_t)c[-i];
          } else {
            for (int32_t i = -p.wx; i <= p.wx; ++i) row[i] += match_cost(g, cost, ux + i, uy + j);
          }
        }
      }
    }
    uint64_t best = 0;
    for (uint32_t lin = 0; lin < (uint32_t)vol.size(); ++lin) {
      const int32_t t = (int32_t)(lin / (uint32_t)(NY * NX)), r = (int32_t)(lin % (uint32_t)(NY * NX));
      const uint64_t key = match_key(vol[lin], t - p.wt, r / NX - p.wy, r % NX - p.wx, lin);
      if (key > best) best = key;
    }
    const size_t centre = ((size_t)p.wt * (size_t)NY + (size_t)p.wy) * (size_t)NX + (size_t)p.wx;
    *result = match_record(g, p, match_key_lin(best), match_key_score(best), vol[centre], (uint32_t)bxs.size());
    if (flags & GV_MATCH_KEEP_SCORES) std::memcpy(scores, vol.data(), vol.size() * sizeof(uint32_t));
    return GV_OK;
  } catch (...) {
    return GV_ERR_HIP;
  }
}

int gv_match_rotations(const gv_match_config *cfg, const gv_match_guess *guess, float *table)
{
  if (!cfg || !match_config_valid(*cfg) || !match_guess_valid(guess) || !table) return GV_ERR_BAD_ARG;
  match_rotations(match_params(*cfg, *guess), table);
  return GV_OK;
}

int gv_match_motion(const gv_match_result *result, gv_transform *out)
{
  if (!result || !out || !std::isfinite(result->x) || !std::isfinite(result->y) || !std::isfinite(result->yaw)) return GV_ERR_BAD_ARG;
  const double half = result->yaw / 2.0;
  *out = gv_transform{0.0, 0.0, std::sin(half), std::cos(half), result->x, result->y, 0.0};
  return GV_OK;
}

}  // extern "C"
