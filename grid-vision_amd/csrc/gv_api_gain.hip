// gv_api_gain.hip -- [EXTENSION] X20 information gain behind the C ABI of include/gridvision_hip_gain.h: the configuration,
// the two device calls (a list of entries; the goal cells of the resident frontier) over one enqueue path, the getter of
// the resident result, gvx2_nav_field_from_gain (gv_nav_field's solver seeded on the device: nav_field_begin /
// nav_field_relax of gv_api_planner.hip).  The kernels are gv_gain.hip's.  The host twin gvx2_gain_host is
// gv_api_gain_host.hip's.
#include "gv_context.hpp"

namespace {

// What both calls do once their own arguments hold: the refusals, the buffers, the two kernels on the public stream
// (set_device_only: the streams are not drained), then a copy per destination the kernels cannot write in place.  No host
// wait once the buffers exist.  `slots`: n of a list call (entries: where the kernel reads them), the frontier's cap of a
// frontier call (entries null).
int enqueue_gain(gv_context *h, const char *call, int32_t slots, const int32_t *entries, uint32_t flags, gvx2_gain_info *info,
                 gvx2_gain_record *out)
{
  gv_context::Gain &g = h->gain;
  g.have = false;   // until this call is enqueued whole
  int rc = GV_OK;
  if ((rc = g.rec.reserve(h, (size_t)kGainMaxN)) || (rc = g.info.reserve(h, 1))) return rc;
  GainArgs a{};
  a.g = h->g;
  a.rule = gain_rule(g.cfg);
  a.n = slots;
  a.flags = flags;
  a.i8 = h->occ_i8;
  a.field = h->nav.field;
  a.entries = entries;
  if (!entries) {
    a.frec = h->frontier.rec;
    a.finfo = h->frontier.info;
  }
  a.rec = g.rec;
  a.info = g.info;
  a.rec_out = static_cast<gvx2_gain_record *>(pinned_device_view(out, 16));
  a.info_out = static_cast<gvx2_gain_info *>(pinned_device_view(info, 16));
  if (!launch_gain(a, h->stream)) {
    GV_HIP(hipGetLastError());
    return state_error(h, call, "the device refused the ray kernel's LDS size");
  }
  GV_HIP(hipGetLastError());
  g.n = slots;
  g.have = true;
  if (!a.info_out) GV_HIP(hipMemcpyAsync(info, g.info, sizeof(gvx2_gain_info), hipMemcpyDeviceToHost, h->stream));
  if (!a.rec_out) GV_HIP(hipMemcpyAsync(out, g.rec, (size_t)slots * sizeof(gvx2_gain_record), hipMemcpyDeviceToHost, h->stream));
  return GV_OK;
}

// the state errors of both calls
int refuse_gain(gv_context *h, const char *call, uint32_t flags, bool from_frontier)
{
  const gv_context::Gain &g = h->gain;
  const char *missing = !g.set ? "no configuration set (gvx2_set_gain_config)"
                        : from_frontier && !h->frontier.have ? "no resident frontier (gvx_frontier)" : nullptr;
  int rc = refuse_state(h, call, missing, (flags & GVX2_GAIN_USE_FIELD) ? kNeedField : 0u, "windows cross them");
  if (rc) return rc;
  if (!frontier_grid_ok(h->g.nx, h->g.ny)) return state_error(h, call, "a side of the grid is above 65535 cells");
  return set_device_only(h);
}

}  // namespace

extern "C" {

// handle configuration only; every call copies it into its kernel arguments
int gvx2_set_gain_config(gv_handle h, const gvx2_gain_config *cfg)
{
  if (!h) return GV_ERR_BAD_ARG;
  if (cfg && !gain_config_valid(*cfg)) return GV_ERR_BAD_ARG;
  if (cfg) h->gain.cfg = *cfg;
  h->gain.set = cfg != nullptr;
  return GV_OK;
}

// Host entries go to the device through the staging slots (the caller's array is free on return), device entries are read
// where they are.
int gvx2_gain_async(gv_handle h, int32_t n, const int32_t *entries, uint32_t flags, gvx2_gain_info *info, gvx2_gain_record *out)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!entries || !info || !out || !gain_call_ok(n, flags, kGainListFlags)) return GV_ERR_BAD_ARG;
  int rc = refuse_gain(h, "gvx2_gain", flags, false);
  if (rc) return rc;
  gv_context::Gain &g = h->gain;
  const int32_t *dev = entries;
  if (!(flags & GVX2_GAIN_DEVICE_ENTRIES)) {
    if ((rc = g.d_entries.reserve(h, (size_t)kGainMaxN)) ||
        (rc = stage_upload(h, g.up, entries, (size_t)n * sizeof(int32_t), (size_t)kGainMaxN * sizeof(int32_t), g.d_entries.get())))
      return rc;
    dev = g.d_entries;
  }
  return enqueue_gain(h, "gvx2_gain", n, dev, flags, info, out);
  GV_CATCH
}

int gvx2_gain(gv_handle h, int32_t n, const int32_t *entries, uint32_t flags, gvx2_gain_info *info, gvx2_gain_record *out)
{
  return wait_scored(h, gvx2_gain_async(h, n, entries, flags, info, out), 1);
}

// The candidates and their number are read by the kernels where the frontier call left them, behind it on the public
// stream: the host knows only the cap.
int gvx2_frontier_gain_async(gv_handle h, uint32_t flags, gvx2_gain_info *info, gvx2_gain_record *out)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!info || !out || (flags & ~(uint32_t)GVX2_GAIN_USE_FIELD) != 0u) return GV_ERR_BAD_ARG;
  if (int rc = refuse_gain(h, "gvx2_frontier_gain", flags, true)) return rc;
  return enqueue_gain(h, "gvx2_frontier_gain", h->frontier.cap, nullptr, flags, info, out);
  GV_CATCH
}

int gvx2_frontier_gain(gv_handle h, uint32_t flags, gvx2_gain_info *info, gvx2_gain_record *out)
{
  return wait_scored(h, gvx2_frontier_gain_async(h, flags, info, out), 1);
}

int gvx2_device_gain(gv_handle h, gvx2_gain_record **records, gvx2_gain_info **info, int32_t *n)
{
  if (!h) return GV_ERR_BAD_ARG;
  const gv_context::Gain &g = h->gain;
  if (!g.have) return GV_ERR_STATE;
  if (records) *records = g.rec.get();
  if (info) *info = g.info.get();
  if (n) *n = g.n;
  return GV_OK;
}

// gv_nav_field with k_nav_seeds_gain in the place of the seed copy and k_nav_seeds: the record and, for k = -1, which one
// it is are read where the gain call left them, behind it on the public stream.
int gvx2_nav_field_from_gain(gv_handle h, int32_t k, gv_nav_info *nav_info)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  gv_context::Gain &g = h->gain;
  if (g.have && (k < -1 || k >= g.n)) return GV_ERR_BAD_ARG;
  if (!g.have) return state_error(h, "gvx2_nav_field_from_gain", "no resident gain (gvx2_gain)");
  NavArgs a{};
  if (int rc = nav_field_begin(h, "gvx2_nav_field_from_gain", 0, a)) return rc;
  launch_nav_init(a, h->stream);
  launch_nav_seeds_gain(a, GainSeedArgs{g.rec, g.info, k}, h->stream);
  GV_HIP(hipGetLastError());
  return nav_field_relax(h, "gvx2_nav_field_from_gain", a, nav_info);
  GV_CATCH
}

}  // extern "C"
