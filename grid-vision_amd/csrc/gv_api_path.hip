// gv_api_path.hip -- [EXTENSION] X17 path extraction behind the C ABI of include/gridvision_hip_path.h: the device call
// (gv_nav_path_async / gv_nav_path: k_nav_path of gv_navpath.hip on the public stream), the getters of the resident
// paths, gv_nav_field_from_path (gv_nav_field's solver seeded on the device: nav_field_begin / nav_field_relax of
// gv_api_planner.hip).  The host twin gv_nav_path_host is gv_api_planner_host.hip's.
#include <algorithm>

#include "gv_context.hpp"

extern "C" {

// A copy of the start cells and one kernel on the public stream, then a copy per destination the kernel cannot write
// in place.  The starts become field entries here on the host (the exact getIndex, as gv_nav_field's seeds do).
int gv_nav_path_async(gv_handle h, const float *starts_xy, int32_t S, int32_t cap, uint32_t flags, gv_nav_path_info *info,
                      float *paths_xy)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!starts_xy || !info || !path_call_ok(S, cap, flags)) return GV_ERR_BAD_ARG;
  int rc = refuse_state(h, "gv_nav_path", nullptr, kNeedField, "there is no whole field");
  if (rc || (rc = set_device_only(h))) return rc;
  gv_context::NavPath &p = h->path;
  const size_t cells = (size_t)S * (size_t)cap;
  p.have = false;   // until this call is enqueued whole
  if ((rc = p.entries.reserve(h, cells)) || (rc = p.xy.reserve(h, 2 * cells)) || (rc = p.info.reserve(h, (size_t)kPathMaxStarts)) ||
      (rc = p.d_starts.reserve(h, (size_t)kPathMaxStarts)))
    return rc;
  int32_t start[kPathMaxStarts];
  for (int32_t s = 0; s < S; ++s) start[s] = host::nav_seed_entry(h->g, starts_xy[2 * s], starts_xy[2 * s + 1]);
  if ((rc = stage_upload(h, p.up, start, (size_t)S * sizeof(int32_t), sizeof(start), p.d_starts.get()))) return rc;

  PathArgs a{};
  a.g = h->g;
  a.field = h->nav.field;
  a.starts = p.d_starts;
  a.S = S; a.cap = cap;
  a.diagonal = flags & GV_PATH_DIAGONAL;
  a.entries = p.entries;
  a.xy = p.xy;
  a.info = p.info;
  a.info_out = static_cast<gv_nav_path_info *>(pinned_device_view(info, 16));
  a.xy_out = paths_xy ? static_cast<float *>(pinned_device_view(paths_xy, 8)) : nullptr;
  launch_nav_path(a, h->stream);
  GV_HIP(hipGetLastError());
  p.S = S; p.cap = cap;
  p.have = true;
  if (!a.info_out) GV_HIP(hipMemcpyAsync(info, p.info, (size_t)S * sizeof(gv_nav_path_info), hipMemcpyDeviceToHost, h->stream));
  if (paths_xy && !a.xy_out) GV_HIP(hipMemcpyAsync(paths_xy, p.xy, 2 * cells * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  return GV_OK;
  GV_CATCH
}

int gv_nav_path(gv_handle h, const float *starts_xy, int32_t S, int32_t cap, uint32_t flags, gv_nav_path_info *info, float *paths_xy)
{
  return wait_scored(h, gv_nav_path_async(h, starts_xy, S, cap, flags, info, paths_xy), 1);
}

int gv_get_nav_path(gv_handle h, int32_t s, int32_t *entries, float *xy, int32_t cap_out, gv_nav_path_info *info)
{
  if (!h || cap_out < 0) return GV_ERR_BAD_ARG;
  GV_TRY
  gv_context::NavPath &p = h->path;
  if (!p.have) return GV_ERR_STATE;
  if (s < 0 || s >= p.S) return GV_ERR_BAD_ARG;
  gv_nav_path_info rec{};
  int rc = copy_out(h, &rec, p.info.get() + s, sizeof(rec));
  if (rc) return rc;
  const size_t first = (size_t)s * (size_t)p.cap, n = (size_t)std::min(std::max(rec.n_cells, 0), cap_out);
  if (entries && n && (rc = copy_out(h, entries, p.entries.get() + first, n * sizeof(int32_t)))) return rc;
  if (xy && n && (rc = copy_out(h, xy, p.xy.get() + 2 * first, 2 * n * sizeof(float)))) return rc;
  if (info) *info = rec;
  return GV_OK;
  GV_CATCH
}

int gv_device_nav_path(gv_handle h, int32_t **entries, float **xy, gv_nav_path_info **info, int32_t *S, int32_t *cap)
{
  if (!h) return GV_ERR_BAD_ARG;
  const gv_context::NavPath &p = h->path;
  if (!p.have) return GV_ERR_STATE;
  if (entries) *entries = p.entries.get();
  if (xy) *xy = p.xy.get();
  if (info) *info = p.info.get();
  if (S) *S = p.S;
  if (cap) *cap = p.cap;
  return GV_OK;
}

// gv_nav_field with k_nav_seeds_path in the place of the seed copy and k_nav_seeds: the cells and their number are read
// where the path call left them, behind it on the public stream.
int gv_nav_field_from_path(gv_handle h, int32_t s, gv_nav_info *info)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  gv_context::NavPath &p = h->path;
  if (p.have && (s < 0 || s >= p.S)) return GV_ERR_BAD_ARG;
  if (!p.have) return state_error(h, "gv_nav_field_from_path", "no resident path (gv_nav_path)");
  NavArgs a{};
  if (int rc = nav_field_begin(h, "gv_nav_field_from_path", 0, a)) return rc;
  a.seeds = p.entries.get() + (size_t)s * (size_t)p.cap;
  launch_nav_init(a, h->stream);
  launch_nav_seeds_path(a, p.info.get() + s, p.cap, h->stream);
  GV_HIP(hipGetLastError());
  return nav_field_relax(h, "gv_nav_field_from_path", a, info);
  GV_CATCH
}

}  // extern "C"
