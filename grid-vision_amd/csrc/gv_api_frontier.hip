// gv_api_frontier.hip -- [EXTENSION] X19 frontier clusters behind the C ABI of include/gridvision_hip_frontier.h: the
// configuration, the device call (gvx_frontier_async / gvx_frontier: the kernels of gv_frontier.hip on the public
// stream), the getters of the resident result, gvx_nav_field_from_frontier (gv_nav_field's solver seeded on the device:
// nav_field_begin / nav_field_relax of gv_api_planner.hip).  The host twin gvx_frontier_host is
// gv_api_frontier_host.hip's.
#include "gv_context.hpp"

extern "C" {

// handle configuration only; every call copies it into its kernel arguments
int gvx_set_frontier_config(gv_handle h, const gvx_frontier_config *cfg)
{
  if (!h) return GV_ERR_BAD_ARG;
  if (cfg && !frontier_config_valid(*cfg)) return GV_ERR_BAD_ARG;
  if (cfg) h->frontier.cfg = *cfg;
  h->frontier.set = cfg != nullptr;
  return GV_OK;
}

// One memset and ten kernels on the public stream, between the grid passes of the frames around them (set_device_only:
// the streams are not drained), then a copy per destination the last kernel cannot write in place.  No host wait once
// the buffers exist.
int gvx_frontier_async(gv_handle h, int32_t cap, uint32_t flags, gvx_frontier_info *info, gvx_frontier_record *out)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!info || !out || !frontier_call_ok(cap, flags)) return GV_ERR_BAD_ARG;
  gv_context::Frontier &f = h->frontier;
  const bool use_field = (flags & GVX_FRONTIER_USE_FIELD) != 0u;
  const unsigned needs = (f.set && f.cfg.max_cost < 256 ? kNeedCostmap : 0u) | (use_field ? kNeedField : 0u);
  int rc = refuse_state(h, "gvx_frontier", f.set ? nullptr : "no configuration set (gvx_set_frontier_config)", needs,
                        "components cross them");
  if (rc) return rc;
  if (!frontier_grid_ok(h->g.nx, h->g.ny)) return state_error(h, "gvx_frontier", "a side of the grid is above 65535 cells");
  if ((rc = set_device_only(h))) return rc;
  const size_t G = (size_t)h->g.G;
  const int32_t row_words = inflate_row_words(h->g.nx);
  const int32_t blocks_x = (row_words - 2 + 3) / 4;
  const size_t n_blocks = (size_t)blocks_x * (size_t)h->g.ny;
  f.have = false;   // until this call is enqueued whole
  if ((rc = f.bits.reserve_zeroed(h, (size_t)h->g.ny * (size_t)row_words, h->stream)) || (rc = f.parent.reserve(h, G)) ||
      (rc = f.labels.reserve(h, G)) || (rc = f.head.reserve(h, (size_t)kFrontierHead + n_blocks)) ||
      (rc = f.keys.reserve(h, 2 * (size_t)kFrontierMaxCap)) || (rc = f.rec.reserve(h, (size_t)kFrontierMaxCap)) ||
      (rc = f.info.reserve(h, 1)))
    return rc;
  GV_HIP(hipMemsetAsync(f.head, 0, ((size_t)kFrontierHead + n_blocks) * sizeof(uint32_t), h->stream));

  FrontierArgs a{};
  a.g = h->g;
  a.rule = frontier_rule(f.cfg);
  a.row_words = row_words;
  a.blocks_x = blocks_x;
  a.n_blocks = (int32_t)n_blocks;
  a.cap = cap;
  a.flags = flags;
  a.i8 = h->occ_i8;
  a.cost = h->infl.cost;
  a.field = h->nav.field;
  a.bits = f.bits;
  a.parent = f.parent;
  a.labels = f.labels;
  a.head = f.head;
  a.keys = f.keys;
  a.rec = f.rec;
  a.info = f.info;
  a.rec_out = static_cast<gvx_frontier_record *>(pinned_device_view(out, 16));
  a.info_out = static_cast<gvx_frontier_info *>(pinned_device_view(info, 16));
  launch_frontier(a, h->stream);
  GV_HIP(hipGetLastError());
  f.cap = cap;
  f.have = true;
  if (!a.info_out) GV_HIP(hipMemcpyAsync(info, f.info, sizeof(gvx_frontier_info), hipMemcpyDeviceToHost, h->stream));
  if (!a.rec_out) GV_HIP(hipMemcpyAsync(out, f.rec, (size_t)cap * sizeof(gvx_frontier_record), hipMemcpyDeviceToHost, h->stream));
  return GV_OK;
  GV_CATCH
}

int gvx_frontier(gv_handle h, int32_t cap, uint32_t flags, gvx_frontier_info *info, gvx_frontier_record *out)
{
  return wait_scored(h, gvx_frontier_async(h, cap, flags, info, out), 1);
}

int gvx_get_frontier_labels(gv_handle h, uint32_t *labels_out)
{
  if (!h || !labels_out) return GV_ERR_BAD_ARG;
  if (!h->frontier.have) return GV_ERR_STATE;
  return copy_out(h, labels_out, h->frontier.labels, (size_t)h->g.G * sizeof(uint32_t));
}

int gvx_device_frontier(gv_handle h, uint32_t **labels, gvx_frontier_record **records, gvx_frontier_info **info, int32_t *cap)
{
  if (!h) return GV_ERR_BAD_ARG;
  const gv_context::Frontier &f = h->frontier;
  if (!f.have) return GV_ERR_STATE;
  if (labels) *labels = f.labels.get();
  if (records) *records = f.rec.get();
  if (info) *info = f.info.get();
  if (cap) *cap = f.cap;
  return GV_OK;
}

// gv_nav_field with k_nav_seeds_frontier in the place of the seed copy and k_nav_seeds: the cells and which of them
// belong to a written cluster are read where the frontier call left them, behind it on the public stream.
int gvx_nav_field_from_frontier(gv_handle h, int32_t k, gv_nav_info *nav_info)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  gv_context::Frontier &f = h->frontier;
  if (f.have && (k < -1 || k >= f.cap)) return GV_ERR_BAD_ARG;
  if (!f.have) return state_error(h, "gvx_nav_field_from_frontier", "no resident frontier (gvx_frontier)");
  NavArgs a{};
  if (int rc = nav_field_begin(h, "gvx_nav_field_from_frontier", 0, a)) return rc;
  launch_nav_init(a, h->stream);
  launch_nav_seeds_frontier(a, FrontierSeedArgs{f.bits, inflate_row_words(h->g.nx), f.labels, f.parent, k}, h->stream);
  GV_HIP(hipGetLastError());
  return nav_field_relax(h, "gvx_nav_field_from_frontier", a, nav_info);
  GV_CATCH
}

}  // extern "C"
