// gv_api_shortcut.hip -- [EXTENSION] X21 shortcuts and waypoints behind the C ABI of include/gridvision_hip_shortcut.h: the
// configuration, the device call (gvx3_shortcut_async / gvx3_shortcut: k_shortcut of gv_shortcut.hip on the public
// stream), the getters of the resident waypoints, gvx3_nav_field_from_shortcut (gv_nav_field's solver seeded on the
// device: nav_field_begin / nav_field_relax of gv_api_planner.hip).  The host twin gvx3_shortcut_host is
// gv_api_shortcut_host.hip's.
#include <algorithm>

#include "gv_context.hpp"

extern "C" {

// handle configuration only; every call copies it into its kernel arguments
int gvx3_set_shortcut_config(gv_handle h, const gvx3_shortcut_config *cfg)
{
  if (!h) return GV_ERR_BAD_ARG;
  if (cfg && !shortcut_config_valid(*cfg)) return GV_ERR_BAD_ARG;
  if (cfg) h->shortcut.cfg = *cfg;
  h->shortcut.set = cfg != nullptr;
  return GV_OK;
}

// One kernel on the public stream over the resident paths and the costmap where they are, then a copy per destination the
// kernel cannot write in place.  No host wait once the buffers exist.
int gvx3_shortcut_async(gv_handle h, int32_t wcap, uint32_t flags, gvx3_shortcut_info *info, float *way_xy)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!info || !shortcut_call_ok(wcap, flags)) return GV_ERR_BAD_ARG;
  gv_context::Shortcut &c = h->shortcut;
  const gv_context::NavPath &p = h->path;
  const char *missing = !c.set ? "no configuration set (gvx3_set_shortcut_config)" : !p.have ? "no resident path (gv_nav_path)" : nullptr;
  int rc = refuse_state(h, "gvx3_shortcut", missing, kNeedCostmap, "there is no whole costmap");
  if (rc) return rc;
  if (!shortcut_room_ok(p.S, wcap)) return GV_ERR_BAD_ARG;
  if ((rc = set_device_only(h))) return rc;
  const size_t ways = (size_t)p.S * (size_t)wcap;
  c.have = false;   // until this call is enqueued whole
  if ((rc = c.entries.reserve(h, ways)) || (rc = c.index.reserve(h, ways)) || (rc = c.xy.reserve(h, 2 * ways)) ||
      (rc = c.info.reserve(h, (size_t)kPathMaxStarts)))
    return rc;

  ShortcutArgs a{};
  a.g = h->g;
  a.rule = shortcut_rule(c.cfg, flags);
  a.S = p.S; a.cap = p.cap; a.wcap = wcap;
  a.cost = h->infl.cost;
  a.src_entries = p.entries;
  a.src_info = p.info;
  a.entries = c.entries;
  a.index = c.index;
  a.xy = c.xy;
  a.info = c.info;
  a.info_out = static_cast<gvx3_shortcut_info *>(pinned_device_view(info, 16));
  a.xy_out = way_xy ? static_cast<float *>(pinned_device_view(way_xy, 8)) : nullptr;
  launch_shortcut(a, h->stream);
  GV_HIP(hipGetLastError());
  c.S = p.S; c.wcap = wcap;
  c.have = true;
  if (!a.info_out) GV_HIP(hipMemcpyAsync(info, c.info, (size_t)p.S * sizeof(gvx3_shortcut_info), hipMemcpyDeviceToHost, h->stream));
  if (way_xy && !a.xy_out) GV_HIP(hipMemcpyAsync(way_xy, c.xy, 2 * ways * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  return GV_OK;
  GV_CATCH
}

int gvx3_shortcut(gv_handle h, int32_t wcap, uint32_t flags, gvx3_shortcut_info *info, float *way_xy)
{
  return wait_scored(h, gvx3_shortcut_async(h, wcap, flags, info, way_xy), 1);
}

int gvx3_get_shortcut(gv_handle h, int32_t s, int32_t *entries, int32_t *index, float *xy, int32_t cap_out, gvx3_shortcut_info *info)
{
  if (!h || cap_out < 0) return GV_ERR_BAD_ARG;
  GV_TRY
  gv_context::Shortcut &c = h->shortcut;
  if (!c.have) return GV_ERR_STATE;
  if (s < 0 || s >= c.S) return GV_ERR_BAD_ARG;
  gvx3_shortcut_info rec{};
  int rc = copy_out(h, &rec, c.info.get() + s, sizeof(rec));
  if (rc) return rc;
  const size_t first = (size_t)s * (size_t)c.wcap, n = (size_t)std::min(std::min(std::max(rec.n_waypoints, 0), c.wcap), cap_out);
  if (entries && n && (rc = copy_out(h, entries, c.entries.get() + first, n * sizeof(int32_t)))) return rc;
  if (index && n && (rc = copy_out(h, index, c.index.get() + first, n * sizeof(int32_t)))) return rc;
  if (xy && n && (rc = copy_out(h, xy, c.xy.get() + 2 * first, 2 * n * sizeof(float)))) return rc;
  if (info) *info = rec;
  return GV_OK;
  GV_CATCH
}

int gvx3_device_shortcut(gv_handle h, int32_t **entries, int32_t **index, float **xy, gvx3_shortcut_info **info, int32_t *S, int32_t *wcap)
{
  if (!h) return GV_ERR_BAD_ARG;
  const gv_context::Shortcut &c = h->shortcut;
  if (!c.have) return GV_ERR_STATE;
  if (entries) *entries = c.entries.get();
  if (index) *index = c.index.get();
  if (xy) *xy = c.xy.get();
  if (info) *info = c.info.get();
  if (S) *S = c.S;
  if (wcap) *wcap = c.wcap;
  return GV_OK;
}

// gv_nav_field with k_nav_seeds_shortcut in the place of the seed copy and k_nav_seeds: the waypoints and their number are
// read where the shortcut call left them, behind it on the public stream.
int gvx3_nav_field_from_shortcut(gv_handle h, int32_t s, gv_nav_info *nav_info)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  gv_context::Shortcut &c = h->shortcut;
  if (c.have && (s < 0 || s >= c.S)) return GV_ERR_BAD_ARG;
  if (!c.have) return state_error(h, "gvx3_nav_field_from_shortcut", "no resident shortcut (gvx3_shortcut)");
  NavArgs a{};
  if (int rc = nav_field_begin(h, "gvx3_nav_field_from_shortcut", 0, a)) return rc;
  a.seeds = c.entries.get() + (size_t)s * (size_t)c.wcap;
  launch_nav_init(a, h->stream);
  launch_nav_seeds_shortcut(a, c.info.get() + s, c.wcap, h->stream);
  GV_HIP(hipGetLastError());
  return nav_field_relax(h, "gvx3_nav_field_from_shortcut", a, nav_info);
  GV_CATCH
}

}  // extern "C"
