// gv_api_match.hip -- [EXTENSION] the two scan matchers behind the C ABI of include/gridvision_hip_match.h and
// include/gridvision_hip_search.h: the handle's configurations and the device calls, X16 gv_match_scan_async /
// gv_match_scan (kernels of gv_match.hip) and X18 gv_match_search_async / gv_match_search (X16's point pass and the
// kernels of gv_search.hip), all on the public stream.  What both calls do before their own kernels -- the refusals, the
// wait for the cloud, the point pass and the mark it leaves for the uploads -- is one function, enqueue_scan_read.  The
// rules they share with the host-only twins are gv_match_rules.hpp's, the twins gv_api_match_host.hip's.
#include "gv_context.hpp"
#include "gv_match_rules.hpp"

namespace {

// what a call gives enqueue_scan_read once its buffers are reserved
struct ScanBlock {
  MatchParams p;
  float2 *pts;      // n_sel pairs
  uint32_t *head;   // the call's block: `words` words zeroed in front of the point pass, which counts the used points in word 0
  size_t words;
};

// the point pass over the current cloud into a call's block
MatchPointsArgs points_args(const gv_context *h, const ScanBlock &b, uint32_t n_sel)
{
  MatchPointsArgs a{};
  a.m_base = h->m_base;
  a.band = h->band;
  a.x = h->cx; a.y = h->cy; a.z = h->cz;
  a.n = (uint32_t)h->n;
  a.n_sel = n_sel;
  a.stride = b.p.stride;
  a.use_band = b.p.use_band;
  a.pts = b.pts;
  a.used = b.head;
  return a;
}

// What every call that reads the scan does before its own kernels: the state refusals in the header's order (`set` and
// `stride` are the call's configuration, `no_config` the text when there is none), the bound on the selected points,
// then `prepare(n_sel, block)` -- the call's own argument block and every reserve it makes, so that nothing is
// enqueued when one fails -- and on the public stream the wait for the cloud's upload (one event wait per upload, as
// a frame's), the memset of the call's block, the point pass and the mark for the uploads (gv_context::ScanReaders).
template <typename Prepare>
int enqueue_scan_read(gv_context *h, const char *call, const char *no_config, bool set, int32_t stride, Prepare prepare)
{
  if (!h->has_bl) return GV_ERR_TF;
  const char *missing = !set ? no_config : (h->n == 0 ? "no cloud" : nullptr);
  int rc = refuse_state(h, call, missing, kNeedCostmap, "there is no whole costmap");
  if (rc) return rc;
  const size_t n_sel = match_selected(h->n, stride);
  if (n_sel > (size_t)kMatchMaxSelected) return state_error(h, call, "more than 2^24 selected points");
  if ((rc = set_device_only(h))) return rc;
  ScanBlock b{};
  if ((rc = prepare((uint32_t)n_sel, b))) return rc;
  gv_context::ScanReaders &r = h->scan_readers;
  if (!r.read) GV_HIP(r.read.create(hipEventDisableTiming));
  if ((rc = wait_cloud(h, h->cloud[h->cloud_cur], 0))) return rc;   // the public stream reads this cloud: behind its upload
  GV_HIP(hipMemsetAsync(b.head, 0, b.words * sizeof(uint32_t), h->stream));
  launch_match_points(points_args(h, b, (uint32_t)n_sel), h->stream);
  GV_HIP(hipEventRecord(r.read, h->stream));   // the cloud's last reader of this call: an upload into the set waits for it
  r.clouds |= 1u << h->cloud_cur;
  return GV_OK;
}

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

int gv_set_search_config(gv_handle h, const gv_search_config *cfg)
{
  if (!h) return GV_ERR_BAD_ARG;
  if (cfg && !search_config_valid(*cfg)) return GV_ERR_BAD_ARG;
  if (cfg) h->search.cfg = *cfg;
  h->search.set = cfg != nullptr;
  return GV_OK;
}

// One memset, three kernels and a copy per destination the device cannot write in place, all on the public stream:
// behind the last gv_inflate, and behind the upload of the cloud it reads.
int gv_match_scan_async(gv_handle h, const gv_match_guess *guess, uint32_t flags, gv_match_result *result, uint32_t *scores)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!match_call_ok(guess, flags, result, scores)) return GV_ERR_BAD_ARG;
  gv_context::Match &m = h->match;
  const bool keep = (flags & GV_MATCH_KEEP_SCORES) != 0;
  MatchArgs a{};
  size_t total = 0;
  ResultDest<gv_match_result> to_result;
  int rc = enqueue_scan_read(h, "gv_match_scan", "no configuration set (gv_set_match_config)", m.set, m.cfg.stride,
                             [&](uint32_t n_sel, ScanBlock &b) {
    a.g = h->g;
    a.p = match_params(m.cfg, *guess);
    a.n_sel = n_sel;
    match_rotations(a.p, a.rot);
    total = (size_t)match_nt(a.p) * (size_t)match_ny(a.p) * (size_t)match_nx(a.p);
    const size_t words = (size_t)kMatchHeadWords + total;
    int rc;
    if ((rc = m.pts.reserve(h, n_sel)) || (rc = m.head.reserve(h, words)) || (rc = to_result.open(h, result, 1, 8, m.d_result)))
      return rc;
    a.pts = m.pts;
    a.head = m.head;
    a.cost = h->infl.cost;
    a.result = to_result.dev;
    a.scores_out = keep ? static_cast<uint32_t *>(pinned_device_view(scores, sizeof(uint32_t))) : nullptr;
    b = ScanBlock{a.p, m.pts, m.head, words};
    return (int)GV_OK;
  });
  if (rc) return rc;
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

// One memset, ten kernels and a copy per destination the device cannot write in place, all on the public stream:
// behind the last gv_inflate, and behind the upload of the cloud it reads, as gv_match_scan_async.
int gv_match_search_async(gv_handle h, const gv_match_guess *guess, uint32_t flags, gv_match_result *result, gv_search_stats *stats)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!search_call_ok(guess, flags, result)) return GV_ERR_BAD_ARG;
  gv_context::Search &m = h->search;
  SearchArgs a{};
  ResultDest<gv_match_result> to_result;
  ResultDest<gv_search_stats> to_stats;
  int rc = enqueue_scan_read(h, "gv_match_search", "no configuration set (gv_set_search_config)", m.set, m.cfg.stride,
                             [&](uint32_t n_sel, ScanBlock &b) {
    a.g = h->g;
    a.sp = search_params(m.cfg, *guess);
    a.n_sel = n_sel;
    a.n_blocks = search_blocks(a.sp);
    match_rotations(a.sp.p, a.rot);
    const int32_t S = search_s(a.sp);
    const size_t words = (size_t)kSearchBounds + (size_t)a.n_blocks;
    const size_t pw = (size_t)search_pool_w(a.g, S), ph = (size_t)search_pool_h(a.g, S);
    int rc;
    if ((rc = m.pts.reserve(h, n_sel)) || (rc = m.head.reserve(h, words)) || (rc = m.rows.reserve(h, pw * (size_t)a.g.ny)) ||
        (rc = m.pool.reserve(h, pw * ph)) || (rc = m.list.reserve(h, (size_t)a.n_blocks)) ||
        (rc = m.slots.reserve(h, (size_t)a.n_blocks * (size_t)S * (size_t)S)) || (rc = to_result.open(h, result, 1, 8, m.d_result)))
      return rc;
    if (stats) {
      if ((rc = to_stats.open(h, stats, 1, 8, m.d_stats))) return rc;
    } else {
      if ((rc = m.d_stats.reserve(h, 1))) return rc;
      to_stats.dev = m.d_stats;
    }
    a.pts = m.pts;
    a.head = m.head;
    a.cost = h->infl.cost;
    a.rows = m.rows;
    a.pool = m.pool;
    a.list = m.list;
    a.slots = m.slots;
    a.result = to_result.dev;
    a.stats = to_stats.dev;
    b = ScanBlock{a.sp.p, m.pts, m.head, words};
    return (int)GV_OK;
  });
  if (rc) return rc;
  launch_search_pool(a, h->stream);
  launch_search_bound(a, h->stream);
  launch_search_seed(a, h->stream);
  launch_search_fine(a, true, h->stream);
  launch_search_prune(a, h->stream);
  launch_search_fine(a, false, h->stream);
  launch_search_select(a, h->stream);
  GV_HIP(hipGetLastError());
  if ((rc = to_result.copy_back(h)) || (rc = to_stats.copy_back(h))) return rc;
  return GV_OK;
  GV_CATCH
}

int gv_match_search(gv_handle h, const gv_match_guess *guess, uint32_t flags, gv_match_result *result, gv_search_stats *stats)
{
  return wait_scored(h, gv_match_search_async(h, guess, flags, result, stats), 1);
}

}  // extern "C"
