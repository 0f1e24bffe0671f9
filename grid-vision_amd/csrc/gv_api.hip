// gv_api.hip -- C ABI (include/gridvision_hip.h) over the gfx950 kernels: the handle's life, transforms, getters,
// plain map updates, grid publishing, ego motion, and the host-only helpers.  The frame pipeline is gv_api_frame.hip,
// the sharded frame gv_api_shard.hip, the kNN / RANSAC / PCA path and the tick gv_api_pose.hip, everything that makes or
// samples the costmap (inflation, the distance field, trajectory scoring) gv_api_planner.hip, the controller over them
// (rollout, control step, MPPI, moving objects, tracker) gv_api_control.hip, their host-only twins gv_api_planner_host.hip.
// One gv_context = one device + one resident grid + its HIP streams.  No exception
// leaves these files; every entry point returns a gv_status.
#include <chrono>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <vector>

#include "gv_context.hpp"

namespace {

int ensure_scratch_i32(gv_context *h, size_t n)
{
  if (n <= h->scratch_i32.cap()) return GV_OK;
  return h->scratch_i32.reserve(h, n + n / 8);
}

void refresh_origin(gv_context *h)
{
  // [EXTENSION] sensor origin = image of (0,0,0) under base<-lidar = fp32 translation column
  h->org.ox = (double)h->m_base.m[3];
  h->org.oy = (double)h->m_base.m[7];
  int ix = 0, iy = 0;
  h->org.valid = get_index(h->g, h->org.ox, h->org.oy, ix, iy) ? 1 : 0;
  h->org.cx = ix;
  h->org.cy = iy;
}

}  // namespace

namespace gv_internal __attribute__((visibility("hidden"))) {

int drain(gv_context *h)
{
  for (hipStream_t s : h->own_streams())
    if (s) GV_HIP(hipStreamSynchronize(s));
  h->pipe_busy = false;
  h->last_fin_slot = -1;
  for (auto &f : h->fs) f.fin_slot = -1;
  h->cloud_wait = false;
  for (auto &c : h->cloud) { c.seen = ~0u; c.release_slot = -1; }   // every upload landed, every reader finished
  for (auto &d : h->det) { d.seen = ~0u; d.release_slot = -1; d.readers = 0; }
  h->sh.forget_frames();
  h->scan_readers.clouds = 0u;
  return GV_OK;
}

bool sector_path(const gv_context *h) { return h->tile_path && !h->tune.force_simple; }

int set_device_only(gv_context *h)
{
  GV_HIP(hipSetDevice(h->device));
  return GV_OK;
}

// Every entry point except the streaming ones (gv_frame_enqueue, gv_*_async, the uploads) starts from
// idle streams: its work on the public stream then sees every earlier frame and upload completed.
int use_device(gv_context *h)
{
  GV_HIP(hipSetDevice(h->device));
  if (h->pipe_busy || h->cloud_wait) return drain(h);
  return GV_OK;
}

// plain grid update (A7 / A8 / A10): rectangles already in fs[0].rects
int enqueue_plain_update(gv_context *h, int32_t n_rects)
{
  if (sector_path(h)) {   // the frame's grid pass without the hit/miss rule, over every row
    GridPassJob grid;   // buffer set 0, no hit / miss rule
    grid.rects = h->fs[0].rects; grid.n_rects = n_rects;
    grid.y1 = h->g.ny;
    grid.stream = h->stream;
    grid.of_frame = false;
    return enqueue_grid_pass(h, grid);
  }
  launch_finalize(finalize_args(h, n_rects), h->stream);
  GV_HIP(hipGetLastError());
  return GV_OK;
}

// the generic grid pass over every cell with the rectangles in fs[0].rects and no hit/miss rule (a plain update); the
// generic frame adds its count grids
FinalizeArgs finalize_args(const gv_context *h, int32_t n_rects)
{
  FinalizeArgs f{};
  f.g = h->g;
  f.log_odds = h->log_odds;
  f.occupancy = h->occupancy;
  f.occ_i8 = h->occ_i8;
  f.rects = h->fs[0].rects;
  f.n_rects = n_rects;
  f.cell_begin = 0;
  f.cell_end = h->g.G;
  return f;
}

int ensure_tbuf(gv_context *h, size_t n)
{
  int rc;
  if ((rc = h->tx.reserve(h, n)) || (rc = h->ty.reserve(h, n)) || (rc = h->tz.reserve(h, n))) return rc;
  return GV_OK;
}

int copy_out(gv_context *h, void *dst, const void *src, size_t bytes)
{
  int rc = use_device(h);
  if (rc) return rc;
  GV_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
  GV_HIP(hipStreamSynchronize(h->stream));
  return GV_OK;
}

// the device's view of `p` when it is pinned host memory aligned to `align` bytes, else null (the copy command then)
void *pinned_device_view(void *p, size_t align)
{
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeHost || !at.devicePointer ||
      (reinterpret_cast<uintptr_t>(at.devicePointer) & (align - 1)) != 0) {
    (void)hipGetLastError();
    return nullptr;
  }
  return at.devicePointer;
}

// The packed grid to PINNED host memory by a small kernel on the public stream, right behind the grid pass.  Measured
// with a cloud streaming in per frame (tools/stream_run.py, profiles/r04/publish_variants.txt): hipMemcpyAsync on the
// public stream 292-349 us per frame and erratic (the download's copy engine interleaves with the upload's: one
// download in six took 300 us instead of 85); the download ordered on the upload stream between two uploads 381 us
// (steady, but every copy command costs ~25 us of engine turn-around); this kernel 262 us, within 0.3 % frame after
// frame -- the copy engines stay with the uploads, PCIe carries both directions at once.
// One layer of G bytes in OccupancyGrid.data order (the packed grid, the costmap) to the caller's memory on the public
// stream: by that kernel, else (pageable memory, or not 16-byte aligned: the kernel stores 16 bytes per lane) by a copy command.
int publish_layer_async(gv_context *h, const int8_t *src, int8_t *data)
{
  int rc = set_device_only(h);
  if (rc) return rc;
  const size_t G = (size_t)h->g.G;
  size_t body = 0;   // bytes the kernel takes
  if (int8_t *view = static_cast<int8_t *>(pinned_device_view(data, 16))) {
    body = G & ~(size_t)15;
    launch_publish_grid(src, view, body, 32, h->stream);
    GV_HIP(hipGetLastError());
  }
  if (G > body) GV_HIP(hipMemcpyAsync(data + body, src + body, G - body, hipMemcpyDeviceToHost, h->stream));
  return GV_OK;
}

// convertPixelsTo3D (grid_vision_node.cpp:309-335): B points, fp64, on the host, with the given K^-1 and camera->base
// transform (the tick's wait passes the transform it was enqueued with)
void convert_pixels_host(const double Kinv[9], const Xform64 &x_bc, const gv_bbox *bboxes, const float *depths, int32_t nb,
                                double *base_points_xyz)
{
  for (int32_t i = 0; i < nb; ++i) {
    // grid_vision_node.cpp:320-322 pixel centre (cv::Point2f), :325 pixelTo3D, :328-329 to base
    const float pcx = (float)(bboxes[i].x_min + ((bboxes[i].x_max - bboxes[i].x_min) / 2.0f));
    const float pcy = (float)(bboxes[i].y_min + ((bboxes[i].y_max - bboxes[i].y_min) / 2.0f));
    const double hx = pcx, hy = pcy, hz = 1.0;
    const double d = depths[i];
    double cam[3];
    for (int r = 0; r < 3; ++r)
      cam[r] = d * ((Kinv[r * 3] * hx + Kinv[r * 3 + 1] * hy) + Kinv[r * 3 + 2] * hz);   // cloud_detections.cpp:95
    host::apply(x_bc, cam, &base_points_xyz[3 * i]);
  }
}

}  // namespace gv_internal

// ---- gv_create, step by step.  The steps run in this order and make their HIP calls in the order written: the order
// in which streams are created and first used decides which hardware queue each lands on (profiles/r03/h2d_notes.md).
namespace {

#define GV_C(call)                                           \
  do {                                                       \
    if ((call) != 0) return GV_ERR_HIP;                      \
  } while (0)

// bitmaps are padded to whole binning tiles, so that every word belongs to exactly one tile
int32_t pad_to_tiles(int32_t n) { return kBinTile * ((n + kBinTile - 1) / kBinTile); }

// every knob of the handle, from the environment
void read_tuning(Tuning &t)
{
  auto num = [](const char *name, int &v) {
    const char *e = std::getenv(name);
    if (e) v = std::atoi(e);
    return e != nullptr;
  };
  int v = 0;
  if (num("GV_LANES", v)) t.n_lanes = (v == 2) ? 2 : 3;
  t.lane3_own_stream = std::getenv("GV_LANE3_OWN_STREAM") != nullptr;
  if (num("GV_QUEUE_PROBE", v)) t.queue_probe = v != 0;
  t.verbose = std::getenv("GV_VERBOSE") != nullptr;
  if (num("GV_TICK_KNN_LANE", v)) t.tick_knn_lane = v != 0;
  const char *impl = std::getenv("GV_RAY_IMPL");
  t.force_simple = impl && std::strcmp(impl, "simple") == 0;
  if (num("GV_PIPELINE", v)) t.no_pipeline = v == 0;
  num("GV_LOG2S", t.sec.log2s);
  if (const char *e = std::getenv("GV_LOG2S_OCT")) {
    int k = 0;
    for (const char *q = e; *q && k < 8; ++k) {
      t.sec.log2s_oct[k] = std::atoi(q);
      while (*q && *q != ',') ++q;
      if (*q == ',') ++q;
    }
  }
  if (num("GV_SECTOR_REORDER", v)) t.sec.reorder = v != 0;
  if (num("GV_SECTOR_HELPERS", v)) t.sec.helpers = v != 0;
  if (num("GV_ANYORDER", v)) t.anyorder = v != 0;
  if (num("GV_GRID_SKIP", v)) t.grid_skip = v != 0;
  num("GV_CAP", t.sec.cap);
  if (num("GV_FLAT_K", v)) t.sec.flat_k = std::max(0, v);
  if (num("GV_FLAT_DIRECT", v)) t.sec.flat_direct = (uint32_t)std::max(0, v);
  if (num("GV_MARCH_LIMIT", v)) t.sec.march_limit = (uint32_t)std::max(0, v);
  if (num("GV_LOG2M", v)) t.sec.log2m = std::min(9, std::max(4, v));
  num("GV_SECTOR_REV", t.sec.sector_rev);
  if (num("GV_NAV_PASS_CAP", v)) t.nav_pass_cap = std::max(1, v);
#ifdef GV_DIAG
  num("GV_ABLATE", t.ablate);
  if (num("GV_BIN_DBG", v)) t.bin_dbg = v > 0;
  if (num("GV_TIMELINE", v)) t.timeline = v > 0;
  if (num("GV_SECTOR_DBG", v)) t.sector_dbg = v > 0;
#endif
}

// grid_map::GridMap::setGeometry + setPosition (src/occupancy_grid.cpp:10-11), the camera, the padded grid of the
// tile path.  Host only.
bool set_geometry(gv_context *h, uint8_t grid_x, uint8_t grid_y, double resolution, const gv_cam_params *cam)
{
  GridParams &g = h->g;
  if (!host::grid_params(grid_x, grid_y, resolution, g)) return false;
  h->cam = *cam;
  host::intrinsics((double)cam->fx, (double)cam->fy, (double)cam->cx, (double)cam->cy, h->K, h->Kinv);
  for (int i = 0; i < 9; ++i) h->camk.k[i] = h->K[i];
  h->camk.W = cam->orig_w;
  h->camk.H = cam->orig_h;
  h->bt_tiles_x = std::max(1, (cam->orig_w + 15) / 16);
  h->bt_tiles_y = std::max(1, (cam->orig_h + 15) / 16);
  // packed (a,b) fields hold 13 bits each; vector stores need nx % 4 == 0
  h->tile_path = (g.nx % 4 == 0) && g.nx <= 8000 && g.ny <= 8000;
  h->nx_pad = pad_to_tiles(g.nx);
  h->ny_pad = pad_to_tiles(g.ny);
  h->nxw = h->nx_pad / 32;
  h->nyw = h->ny_pad / 32;
  h->tiles_x = h->nx_pad / kBinTile;
  h->tiles_y = h->ny_pad / kBinTile;
  h->n_tiles = h->tiles_x * h->tiles_y;
  return true;
}

int create_streams(gv_context *h)
{
  GV_C(h->stream.create());
  GV_C(h->lane[0].create());
  GV_C(h->lane[1].create());
  GV_C(h->stream_copy.create());
  if (h->tune.n_lanes == 3 && h->tune.lane3_own_stream) GV_C(h->lane[2].create());
  return GV_OK;
}

// The upload stream must not share a hardware queue with the public stream or a lane (a process gets four
// queues; a stream created when four exist joins the one with the fewest streams, ties by address -- e.g. a host
// application or framework that owns a stream already pushes one of ours onto a shared queue, and when that is
// the upload stream every cloud waits behind kernels: the 0.55-0.8-of-copy-rate regime of profiles/r03/h2d_notes.md).
// Probe: hold the three compute streams busy for 150 us each, time a 4-byte memset on the upload stream; if it had
// to wait, make another upload stream (before letting go of this one, so that it lands elsewhere) and try again.
int probe_upload_queue(gv_context *h)
{
  DevBuf<unsigned> probe;
  GV_C(probe.reserve(h, 64));
  std::vector<Stream> rejected;   // let go after the loop: a replacement made while they exist lands elsewhere
  launch_hold(1ull, h->stream);   // (the kernel's code object is loaded before anything is timed)
  // Only the handle's own streams are synchronised (a device-wide wait would stall on, and be perturbed by, every
  // other handle or application stream of the process); a stream's hardware queue is created on its first use, so
  // one untimed memset goes first.  Costs 0.3-1 ms per gv_create; GV_QUEUE_PROBE=0 skips it.
  auto sync_own = [&]() -> hipError_t {
    for (hipStream_t q : h->own_streams()) {
      const hipError_t e = q ? hipStreamSynchronize(q) : hipSuccess;
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  };
  for (int attempt = 0; attempt < 6; ++attempt) {
    GV_C(hipMemsetAsync(probe, 0, 4, h->stream_copy));   // untimed: the queue exists afterwards
    GV_C(sync_own());
    for (hipStream_t q : {(hipStream_t)h->stream, (hipStream_t)h->lane[0], (hipStream_t)h->lane[1]})
      launch_hold(15000ull, q);   // 150 us at 100 MHz
    const auto t0 = std::chrono::steady_clock::now();
    GV_C(hipMemsetAsync(probe, 0, 4, h->stream_copy));
    GV_C(hipStreamSynchronize(h->stream_copy));
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    GV_C(sync_own());
    h->upload_probe_us = us;
    if (us < 90.0) break;
    h->upload_stream_retries++;
    Stream nw;
    GV_C(nw.create());
    rejected.push_back(std::move(h->stream_copy));
    h->stream_copy = std::move(nw);
  }
  if (h->tune.verbose)
    std::fprintf(stderr, "gridvision_hip: upload stream probe %.0f us, %d replacement(s)\n", h->upload_probe_us, h->upload_stream_retries);
  return GV_OK;
}

// the view the frame code indexes, and the ordering events
int create_events(gv_context *h)
{
  h->streams[0] = h->stream;
  for (int l = 0; l < gv_context::kLanesMax; ++l) h->streams[1 + l] = h->lane[l];
  if (!h->lane[2]) h->streams[3] = h->stream_copy;   // the third lane runs on the upload stream (gv_context::lanes_now)
  // Ordering-only events between queues of this device (and a completion flag the host polls): nobody reads
  // memory on the strength of them -- results are read in stream order on the public stream or after a
  // stream synchronise -- so the kernels that carry them need no system-scope release at their end.
  for (auto &e : h->ev_fin) GV_C(e.create(hipEventDisableTiming | hipEventDisableSystemFence));
  for (auto &e : h->ev_sec) GV_C(e.create(hipEventDisableTiming | hipEventDisableSystemFence));
  GV_C(h->ev_join.create(hipEventDisableTiming));
  GV_C(h->tick.done.create(hipEventDisableTiming));
  GV_C(h->tick.fork.create(hipEventDisableTiming));
  GV_C(h->tick.join.create(hipEventDisableTiming));
  for (auto &c : h->cloud) GV_C(c.ready.create(hipEventDisableTiming));
  for (auto &d : h->det) GV_C(d.ready.create(hipEventDisableTiming));
  return GV_OK;
}

// the resident layers, the count grids and bitmaps of every stream and buffer set (zeroed on the public stream), the
// timing events
int alloc_grid(gv_context *h)
{
  const size_t G = (size_t)h->g.G;
  GV_C(h->log_odds.reserve(h, G));
  GV_C(h->occupancy.reserve(h, G));
  GV_C(h->occ_i8.reserve(h, G));
  GV_C(h->ray_count.reserve_zeroed(h, 4, h->stream));
  GV_C(h->scratch_i32.reserve(h, G));
#ifdef GV_DIAG
  if (h->tune.bin_dbg)
    for (auto &q : h->d_bin_dbg) GV_C(q.reserve_zeroed(h, 8192 * 16, h->stream));
  if (h->tune.timeline) {
    const size_t nt = gv_context::kTlFrames * 8;
    GV_C(h->d_tl.reserve(h, nt));
    std::vector<unsigned long long> init(nt);
    for (size_t i = 0; i < nt; i += 2) { init[i] = ~0ull; init[i + 1] = 0ull; }
    GV_C(hipMemcpy(h->d_tl, init.data(), nt * sizeof(unsigned long long), hipMemcpyHostToDevice));
  }
  if (h->tune.sector_dbg) GV_C(h->d_dbg.reserve_zeroed(h, kMaxStatSlots * 16, h->stream));
#endif
  const bool sectors = sector_path(h);
  const int n_streams = sectors ? 1 + h->tune.n_lanes : 1;
  for (int k = 0; k < n_streams; ++k) GV_C(h->sb[k].hits.reserve_zeroed(h, G, h->stream));
  for (int k = 0; k < (sectors ? gv_context::kSets : 1); ++k)
    GV_C(h->fs[k].stats.reserve_zeroed(h, kMaxStatSlots * 2, h->stream));
  if (sectors) {
    h->bmN_words = (size_t)h->ny_pad * h->nxw;   // multiples of 4 words (pads are multiples of 128)
    h->bmT_words = (size_t)h->nx_pad * h->nyw;
    h->ends_words = 2 * (h->bmN_words + h->bmT_words);
    for (FrameSet &f : h->fs) {
      // + slack: the sharded exchange pads the buffer to `world` equal slices (host::ShardPlan::slice)
      GV_C(f.ends.reserve_zeroed(h, h->ends_words + 1024, h->stream));
      f.hitN = f.ends;
      f.clipN = f.hitN + h->bmN_words;
      f.hitT = f.clipN + h->bmN_words;
      f.clipT = f.hitT + h->bmT_words;
      GV_C(f.free_.reserve_zeroed(h, h->bmN_words + h->bmT_words + 16, h->stream));
      f.freeN = f.free_;
      f.freeT = f.free_ + h->bmN_words;
    }
    for (int q = 0; q < n_streams; ++q) {
      for (auto &tot : h->sb[q].bin_total) GV_C(tot.reserve_zeroed(h, (size_t)h->n_tiles, h->stream));
      GV_C(h->sb[q].bin_done.reserve_zeroed(h, (size_t)h->n_tiles, h->stream));
    }
  } else {
    // generic path: byte flags of clipped ray ends and of free cells + the compacted ray list
    GV_C(h->clip_end.reserve_zeroed(h, G + 16, h->stream));
    GV_C(h->miss8.reserve_zeroed(h, G + 16, h->stream));
    GV_C(h->ray_list.reserve(h, G));
  }
  for (auto &e : h->ev) GV_C(e.create(hipEventDefault));   // timing events
  for (auto &pr : h->kt)
    for (auto &e : pr) GV_C(e.create(hipEventDefault));
  // what follows the detection count and the cloud, at its starting size
  GV_C(ensure_det_shared(h, 64));
  for (auto &d : h->det) GV_C(ensure_det(h, d, 64));
  GV_C(ensure_point_buffers(h, 0));
  return GV_OK;
}
#undef GV_C

}  // namespace

extern "C" {

int gv_abi_version(void) { return 4; }

int gv_create(gv_handle *out, uint8_t grid_x, uint8_t grid_y, double resolution, const gv_cam_params *cam,
              int device_id)
{
  if (!out) return GV_ERR_BAD_ARG;
  *out = nullptr;
  if (!cam || grid_x == 0 || grid_y == 0 || !(resolution > 0.0)) return GV_ERR_BAD_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return GV_ERR_NO_DEVICE;
  gv_context *h = new (std::nothrow) gv_context();
  if (!h) return GV_ERR_HIP;
  GV_TRY
  if (device_id < 0) {
    if (hipGetDevice(&device_id) != hipSuccess) device_id = 0;
  }
  if (device_id >= ndev) { delete h; return GV_ERR_NO_DEVICE; }
  h->device = device_id;
  if (!set_geometry(h, grid_x, grid_y, resolution, cam)) { delete h; return GV_ERR_BAD_ARG; }
  read_tuning(h->tune);
  auto fail = [&](int code) { gv_destroy(h); return code; };
  if (hipSetDevice(h->device) != hipSuccess) return fail(GV_ERR_HIP);
  int rc;
  if ((rc = create_streams(h))) return fail(rc);
  if (h->tune.queue_probe && (rc = probe_upload_queue(h))) return fail(rc);
  if ((rc = create_events(h))) return fail(rc);
  if ((rc = alloc_grid(h))) return fail(rc);
  h->sh.plan = shard_plan(h, 1);
  *out = h;
  rc = gv_reset(h);
  if (rc != GV_OK) { *out = nullptr; return fail(rc); }
  return GV_OK;
  GV_CATCH
}

// What is about order stays here; everything the handle owns goes with its members (streams last).
int gv_destroy(gv_handle h)
{
  if (!h) return GV_ERR_BAD_ARG;
  (void)hipSetDevice(h->device);
  for (hipStream_t s : h->own_streams())
    if (s) (void)hipStreamSynchronize(s);
  comm_destroy(h);
  delete h;
  return GV_OK;
}

const char *gv_last_error(gv_handle h) { return h ? h->err.c_str() : "null handle"; }

int gv_grid_geometry(gv_handle h, int32_t *nx, int32_t *ny, double *pos_x, double *pos_y)
{
  if (!h) return GV_ERR_BAD_ARG;
  if (nx) *nx = h->g.nx;
  if (ny) *ny = h->g.ny;
  if (pos_x) *pos_x = h->g.pos_x;
  if (pos_y) *pos_y = h->g.pos_y;
  return GV_OK;
}

int gv_reset(gv_handle h)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  int rc = use_device(h);
  if (rc) return rc;
  const size_t G = (size_t)h->g.G;
  launch_fill_f32(h->log_odds, kLogOddsPrior, G, h->stream);      // :12
  launch_fill_f32(h->occupancy, kInitProbability, G, h->stream);  // :13
  // toOccupancyGrid of the initial layer: (int8)(0.5f*100) = 50
  GV_HIP(hipMemsetAsync(h->occ_i8, 50, G, h->stream));
  GV_HIP(hipGetLastError());
  GV_HIP(hipStreamSynchronize(h->stream));
  h->move_residue = host::Se2{0.0, 0.0, 0.0};
  h->layers_in_step = true;   // 0.0 / 0.5 / 50: what the grid pass derives from the prior
  h->infl.have_cost = h->infl.have_dist2 = false;   // the costmap was a snapshot of the grid that is gone
  h->nav.have_field = false;                        // ... and so was the distance field over it
  h->path.have = false;                             // ... and the paths walked down that field
  h->frontier.have = false;                         // ... and the frontier clusters of that grid (X19)
  h->gain.have = false;                             // ... and the gain records of its candidates (X20)
  h->shortcut.have = false;                         // ... and the waypoints of those paths (X21)
  return GV_OK;
  GV_CATCH
}

int gv_set_transforms(gv_handle h, const gv_transform *cl, const gv_transform *bc, const gv_transform *bl)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (cl) { h->tf_cl = *cl; h->m_cam = host::pcl_matrix_from_tf(*cl); h->has_cl = true; }
  if (bc) { h->tf_bc = *bc; h->x_bc = host::xform_from_tf(*bc); h->has_bc = true; }
  if (bl) { h->tf_bl = *bl; h->m_base = host::pcl_matrix_from_tf(*bl); h->has_bl = true; refresh_origin(h); }
  return GV_OK;
  GV_CATCH
}

/* ------------------------------------------------------------------ ingest -- */
int gv_host_alloc(void **ptr, size_t bytes)
{
  if (!ptr || !bytes) return GV_ERR_BAD_ARG;
  *ptr = nullptr;
  return hipHostMalloc(ptr, bytes, hipHostMallocDefault) == hipSuccess ? GV_OK : GV_ERR_HIP;
}

int gv_host_free(void *ptr)
{
  if (!ptr) return GV_OK;
  return hipHostFree(ptr) == hipSuccess ? GV_OK : GV_ERR_HIP;
}

int gv_transform_lidar_to_camera(gv_handle h, float *x_cam, float *y_cam, float *z_cam)
{
  if (!h || !x_cam || !y_cam || !z_cam) return GV_ERR_BAD_ARG;
  if (!h->has_cl) return GV_ERR_TF;   // the reference returns nullptr (:292-297)
  GV_TRY
  int rc = use_device(h);
  if (rc) return rc;
  const size_t n = h->n;
  if ((rc = ensure_tbuf(h, n))) return rc;
  if (n) {
    TransformCloudArgs ta;
    ta.x = h->cx; ta.y = h->cy; ta.z = h->cz; ta.n = (uint32_t)n;
    ta.m = h->m_cam;
    ta.ox = h->tx; ta.oy = h->ty; ta.oz = h->tz;
    launch_transform_cloud(ta, h->stream);
    GV_HIP(hipGetLastError());
    GV_HIP(hipMemcpyAsync(x_cam, h->tx, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    GV_HIP(hipMemcpyAsync(y_cam, h->ty, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    GV_HIP(hipMemcpyAsync(z_cam, h->tz, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  }
  GV_HIP(hipStreamSynchronize(h->stream));
  return GV_OK;
  GV_CATCH
}

// device int16 ids -> caller's int32 array
static int read_back_ids(gv_context *h, int32_t *out)
{
  if (!h->n) return GV_OK;
  int rc = ensure_scratch_i32(h, h->n);
  if (rc) return rc;
  launch_i16_to_i32(h->sb[h->last.points].bbox_id, h->scratch_i32, h->n, h->stream);
  GV_HIP(hipGetLastError());
  GV_HIP(hipMemcpyAsync(out, h->scratch_i32, h->n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  GV_HIP(hipStreamSynchronize(h->stream));
  return GV_OK;
}

int gv_extract_cloud_per_bbox(gv_handle h, const gv_bbox *bboxes, int32_t nb, int32_t *bbox_id, int32_t *counts)
{
  if (!h || nb < 0 || nb > 32767 || (nb && !bboxes) || !bbox_id) return GV_ERR_BAD_ARG;
  if (!h->has_cl) return GV_ERR_TF;
  GV_TRY
  int rc = use_device(h);
  if (rc) return rc;
  if ((rc = upload_scratch_bboxes(h, bboxes, nb))) return rc;
  launch_points(bbox_points_args(h, h->det[2], 0, h->n, h->sb[h->last.points].bbox_id), h->stream);
  GV_HIP(hipGetLastError());
  if ((rc = read_back_ids(h, bbox_id))) return rc;
  GV_HIP(hipStreamSynchronize(h->stream));
  h->last.bbox_id = true;
  if (counts) {
    for (int32_t b = 0; b < nb; ++b) counts[b] = 0;
    for (size_t i = 0; i < h->n; ++i)
      if (bbox_id[i] >= 0) counts[bbox_id[i]]++;
  }
  return GV_OK;
  GV_CATCH
}

int gv_convert_pixels_to_3d(gv_handle h, const gv_bbox *bboxes, const float *depths, int32_t nb,
                            double *base_points_xyz)
{
  if (!h || nb < 0 || (nb && (!bboxes || !depths || !base_points_xyz))) return GV_ERR_BAD_ARG;
  if (!h->has_bc) return GV_ERR_TF;
  GV_TRY
  convert_pixels_host(h->Kinv, h->x_bc, bboxes, depths, nb, base_points_xyz);
  return GV_OK;
  GV_CATCH
}

int gv_transform_lshape_objects(gv_handle h, gv_lshape_pose *poses, int32_t n)
{
  if (!h || n < 0 || (n && !poses)) return GV_ERR_BAD_ARG;
  if (!h->has_bc) return GV_ERR_TF;
  GV_TRY
  for (int32_t i = 0; i < n; ++i) host::transform_pose(h->tf_bc, poses[i]);
  return GV_OK;
  GV_CATCH
}

int gv_extract_bboxes(const float *boxes, const float *scores, int32_t n, int32_t c, double conf_threshold,
                      double iou_threshold, int32_t orig_w, int32_t orig_h, int32_t resize, gv_bbox *out,
                      int32_t *n_out)
{
  gv_context *h = nullptr;
  if (!n_out || n < 0 || c <= 0 || resize <= 0 || (n && (!boxes || !scores || !out))) return GV_ERR_BAD_ARG;
  GV_TRY
  std::vector<gv_bbox> cand;
  for (int32_t i = 0; i < n; ++i) {
    int32_t best = 0;
    float mx = scores[(size_t)i * c];
    for (int32_t k = 1; k < c; ++k)
      if (scores[(size_t)i * c + k] > mx) { mx = scores[(size_t)i * c + k]; best = k; }   // :121-122
    if (mx >= conf_threshold) {                                                            // :125
      gv_bbox b;
      b.confidence = mx;
      b.label = host::object_class(best);
      b.x_min = boxes[i * 4 + 0]; b.y_min = boxes[i * 4 + 1];
      b.x_max = boxes[i * 4 + 2]; b.y_max = boxes[i * 4 + 3];
      cand.push_back(b);
    }
  }
  std::vector<gv_bbox> kept = host::nms(std::move(cand), (float)iou_threshold);   // :142
  host::denormalize(kept, orig_w, orig_h, resize);                                // :143
  for (size_t i = 0; i < kept.size(); ++i) out[i] = kept[i];
  *n_out = (int32_t)kept.size();
  return GV_OK;
  GV_CATCH
}

int gv_filter_bboxes(const gv_bbox *in, int32_t n, gv_bbox *static_out, int32_t *n_static, gv_bbox *dynamic_out,
                     int32_t *n_dynamic)
{
  if (n < 0 || !n_static || !n_dynamic || (n && (!in || !static_out || !dynamic_out))) return GV_ERR_BAD_ARG;
  int32_t ns = 0, nd = 0;
  for (int32_t i = 0; i < n; ++i) {
    const int32_t l = in[i].label;
    if (l == 9 || l == 0 || l == 1 || l == 2) dynamic_out[nd++] = in[i];   // VEHICLE, BIKE, MOTORBIKE, PERSON
    else static_out[ns++] = in[i];
  }
  *n_static = ns;
  *n_dynamic = nd;
  return GV_OK;
}

// host only, no handle: the sharded frame's bands and slices (host::ShardPlan, gv_host_math.hpp)
int gv_shard_band_rows(int32_t rank, int32_t world, int32_t ny, int32_t *y0, int32_t *y1)
{
  if (world < 1 || rank < 0 || rank >= world || ny < 1 || !y0 || !y1) return GV_ERR_BAD_ARG;
  host::shard_band_rows(rank, world, ny, pad_to_tiles(ny), *y0, *y1);
  return GV_OK;
}

int64_t gv_shard_slice_words(int64_t words, int32_t world)
{
  if (words < 0 || world < 1) return -1;
  return (int64_t)host::shard_slice_words((size_t)words, world);
}

// test hook (gv_test_hooks.h): the plan a handle over an nx x ny grid (tile path) keeps for a communicator of `world` ranks
int gv_test_shard_plan(int32_t nx, int32_t ny, int32_t world, int64_t *slice, int64_t *chunk, int32_t *equal_bands,
                       int64_t *cnt0, int32_t *rows)
{
  if (nx < 1 || ny < 1 || world < 1 || !slice || !chunk || !equal_bands || !cnt0 || !rows) return GV_ERR_BAD_ARG;
  const int32_t nx_pad = pad_to_tiles(nx), ny_pad = pad_to_tiles(ny);
  const size_t ends_words = 2 * ((size_t)ny_pad * (size_t)(nx_pad / 32) + (size_t)nx_pad * (size_t)(ny_pad / 32));   // alloc_grid's
  try {
    const host::ShardPlan P(nx, ny, nx_pad, ny_pad, nx_pad / 32, ends_words, world);
    *slice = (int64_t)P.slice;
    *chunk = (int64_t)P.chunk;
    *equal_bands = P.equal_bands ? 1 : 0;
    *cnt0 = (int64_t)P.cnt0;
    for (int r = 0; r < world; ++r) { rows[2 * r] = P.bands[(size_t)r].y0; rows[2 * r + 1] = P.bands[(size_t)r].y1; }
  } catch (...) {
    return GV_ERR_HIP;
  }
  return GV_OK;
}

// test hook (gv_test_hooks.h): the sector plan enqueue_sectors builds for this grid, origin cell and cloud size
int gv_test_sector_plan(int32_t nx, int32_t ny, int32_t cx, int32_t cy, int64_t n_points, gv_test_sector_plan_t *plan,
                        int32_t *wg, int64_t wg_cap)
{
  if (nx < 1 || ny < 1 || cx < 0 || cx >= nx || cy < 0 || cy >= ny || n_points < 0 || !plan || wg_cap < 0 || (wg_cap && !wg))
    return GV_ERR_BAD_ARG;
  Tuning t;
  read_tuning(t);
  const host::SectorPlan P(nx, ny, cx, cy, (size_t)n_points, t.sec);
  gv_test_sector_plan_t &out = *plan;
  out = gv_test_sector_plan_t{};
  for (int o = 0; o < 8; ++o) { out.len[o] = P.len[o]; out.log2s_oct[o] = P.log2s_oct[o]; out.rev_oct[o] = P.rev_oct[o]; }
  for (int k = 0; k < 9; ++k) out.wg_base[k] = P.wg_base[k];
  out.imax = P.imax; out.cap = P.cap; out.log2m = P.log2m; out.marks_words = P.marks_words;
  out.oct_perm = P.oct_perm; out.reorder = P.reorder; out.n_helpers = P.n_helpers;
  out.flat_k = P.flat_k; out.march_limit = P.march_limit; out.flat_direct = P.flat_direct;
  out.ch = P.ch; out.lds_bytes = (int64_t)P.lds_bytes;
  out.total_workgroups = P.total_workgroups; out.stat_slots = (int64_t)P.stat_slots;
  out.violations = P.violations();
  for (int64_t b = 0; b < std::min<int64_t>(wg_cap, P.total_workgroups); ++b) {
    const host::SectorPlan::Workgroup w = P.workgroup((int)b);
    const int32_t row[7] = {w.octant, w.sector, w.helper, w.part, w.nparts, w.stat_slot, w.idle};
    std::memcpy(wg + 7 * b, row, sizeof(row));
  }
  return GV_OK;
}

int gv_get_intrinsics(gv_handle h, double K[9], double K_inv[9])
{
  if (!h) return GV_ERR_BAD_ARG;
  if (K) std::memcpy(K, h->K, sizeof(h->K));
  if (K_inv) std::memcpy(K_inv, h->Kinv, sizeof(h->Kinv));
  return GV_OK;
}

int gv_update_map(gv_handle h)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  int rc = use_device(h);
  if (rc) return rc;
  if ((rc = enqueue_plain_update(h, 0))) return rc;
  GV_HIP(hipStreamSynchronize(h->stream));
  return GV_OK;
  GV_CATCH
}

int gv_update_map_poses(gv_handle h, const gv_lshape_pose *poses, int32_t n)
{
  if (!h || n < 0 || (n && !poses)) return GV_ERR_BAD_ARG;
  GV_TRY
  int rc = use_device(h);
  if (rc) return rc;
  DetSet &d = h->det[2];
  DetUpload u;
  u.poses = poses; u.n_poses = n;
  u.stream = h->stream;
  u.masks = false;
  if ((rc = upload_det(h, d, u))) return rc;
  GV_HIP(hipEventRecord(d.ready, h->stream));
  if (n) {
    RectsFromPosesArgs ra;
    ra.poses = d.poses; ra.n = n; ra.g = h->g;
    ra.from_cam = false; ra.bc = h->x_bc;
    ra.rects = h->fs[0].rects;
    launch_rects_from_poses(ra, h->stream);
  }
  if ((rc = enqueue_plain_update(h, n))) return rc;
  GV_HIP(hipStreamSynchronize(h->stream));
  return GV_OK;
  GV_CATCH
}

int gv_update_map_points(gv_handle h, const double *pts, const gv_bbox *bboxes, int32_t n)
{
  if (!h || n < 0 || (n && (!pts || !bboxes))) return GV_ERR_BAD_ARG;
  GV_TRY
  int rc = use_device(h);
  if (rc) return rc;
  if ((rc = upload_scratch_bboxes(h, bboxes, n, false))) return rc;
  if (n) {
    GV_HIP(hipMemcpyAsync(h->d_pts, pts, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    RectsFromPointsArgs ra;
    ra.pts_xyz = h->d_pts; ra.bboxes = h->det[2].bboxes; ra.n = n;
    ra.g = h->g; ra.rects = h->fs[0].rects;
    launch_rects_from_points(ra, h->stream);
  }
  if ((rc = enqueue_plain_update(h, n))) return rc;
  GV_HIP(hipStreamSynchronize(h->stream));
  return GV_OK;
  GV_CATCH
}

int gv_to_occupancy_grid(gv_handle h, int8_t *data, gv_grid_info *info)
{
  if (!h || !data) return GV_ERR_BAD_ARG;
  GV_TRY
  int rc = use_device(h);
  if (rc) return rc;
  GV_HIP(hipMemcpyAsync(data, h->occ_i8, (size_t)h->g.G, hipMemcpyDeviceToHost, h->stream));
  GV_HIP(hipStreamSynchronize(h->stream));
  if (info) {
    info->width = (uint32_t)h->g.nx;
    info->height = (uint32_t)h->g.ny;
    info->resolution = h->g.res;
    info->origin_x = h->g.pos_x - 0.5 * h->g.len_x;
    info->origin_y = h->g.pos_y - 0.5 * h->g.len_y;
  }
  return GV_OK;
  GV_CATCH
}

int gv_to_occupancy_grid_async(gv_handle h, int8_t *data)
{
  if (!h || !data) return GV_ERR_BAD_ARG;
  GV_TRY
  int rc = set_device_only(h);   // the public stream runs the grid passes: this copy sits between two of them
  if (rc) return rc;
  GV_HIP(hipMemcpyAsync(data, h->occ_i8, (size_t)h->g.G, hipMemcpyDeviceToHost, h->stream));
  return GV_OK;
  GV_CATCH
}

int gv_publish_grid_async(gv_handle h, int8_t *data)
{
  if (!h || !data) return GV_ERR_BAD_ARG;
  GV_TRY
  return publish_layer_async(h, h->occ_i8, data);
  GV_CATCH
}

int gv_get_log_odds(gv_handle h, float *out)
{
  if (!h || !out) return GV_ERR_BAD_ARG;
  return copy_out(h, out, h->log_odds, (size_t)h->g.G * sizeof(float));
}

int gv_get_occupancy(gv_handle h, float *out)
{
  if (!h || !out) return GV_ERR_BAD_ARG;
  return copy_out(h, out, h->occupancy, (size_t)h->g.G * sizeof(float));
}

int gv_set_log_odds(gv_handle h, const float *in)
{
  if (!h || !in) return GV_ERR_BAD_ARG;
  int rc = use_device(h);
  if (rc) return rc;
  h->layers_in_step = false;   // one layer replaced: the next grid pass writes every row
  GV_HIP(hipMemcpyAsync(h->log_odds, in, (size_t)h->g.G * sizeof(float), hipMemcpyHostToDevice, h->stream));
  GV_HIP(hipStreamSynchronize(h->stream));
  h->move_residue = host::Se2{0.0, 0.0, 0.0};
  return GV_OK;
}

// [EXTENSION] X3: the planner (gv_host_math.hpp) picks the whole-cell resample S and keeps the rest as residue; the
// resample is two kernels on the public stream, so it sits between the grid passes of the frames around it and
// behind a pending tick's grid download.  No host wait (the scratch allocation of the first applied move aside).
int gv_grid_move(gv_handle h, const gv_transform *motion, gv_grid_move_info *info)
{
  if (!h || !motion) return GV_ERR_BAD_ARG;
  GV_TRY
  host::Se2 d;
  if (!host::se2_from_motion(*motion, d)) return GV_ERR_BAD_ARG;
  if (int rc = refuse_state(h, "gv_grid_move", nullptr, 0, "a move crosses them")) return rc;
  const host::GridMoveStep st = host::plan_grid_move(h->move_residue, d, h->g);
  if (!std::isfinite(st.residue.x) || !std::isfinite(st.residue.y) || !std::isfinite(st.tx) || !std::isfinite(st.ty))
    return GV_ERR_BAD_ARG;   // finite fields whose sum overflows
  if (st.applied) {
    int rc = set_device_only(h);
    if (rc) return rc;
    const size_t G = (size_t)h->g.G, fbytes = (G * sizeof(float) + 255) & ~(size_t)255;
    if ((rc = h->move_scratch.reserve(h, 2 * fbytes + G))) return rc;
    uint8_t *const scratch = h->move_scratch;
    GridMoveArgs a{};
    a.g = h->g;
    a.c = st.c; a.s = st.s; a.tx = st.tx; a.ty = st.ty;
    a.lo = h->log_odds; a.occ = h->occupancy; a.i8 = h->occ_i8;
    a.lo_out = reinterpret_cast<float *>(scratch);
    a.occ_out = reinterpret_cast<float *>(scratch + fbytes);
    a.i8_out = reinterpret_cast<int8_t *>(scratch + 2 * fbytes);
    launch_grid_move(a, h->stream);
    launch_grid_move_copy_back(a, h->stream);
    GV_HIP(hipGetLastError());
  }
  h->move_residue = st.residue;
  if (info) {
    info->applied = st.applied ? 1 : 0;
    info->cos_yaw = st.c; info->sin_yaw = st.s;
    info->tx = st.tx; info->ty = st.ty;
    info->res_yaw = st.residue.yaw; info->res_x = st.residue.x; info->res_y = st.residue.y;
  }
  return GV_OK;
  GV_CATCH
}

// [EXTENSION] X4: handle configuration only, no device work.  Every binning launch copies h->band into its kernel
// arguments, so frames and ticks already enqueued keep the band they were enqueued with.
int gv_set_height_band(gv_handle h, const gv_height_band *band)
{
  if (!h) return GV_ERR_BAD_ARG;
  if (!band) {
    h->band = HeightBand{-INFINITY, INFINITY, 0};
    return GV_OK;
  }
  if (std::isnan(band->z_ground) || std::isnan(band->z_max) || band->z_ground > band->z_max ||
      (band->ground_clears != 0 && band->ground_clears != 1))
    return GV_ERR_BAD_ARG;
  h->band = HeightBand{band->z_ground, band->z_max, band->ground_clears};
  return GV_OK;
}

int gv_get_hits(gv_handle h, int32_t *out)
{
  if (!h || !out) return GV_ERR_BAD_ARG;
  if (!h->last.hits) return GV_ERR_STATE;
  return copy_out(h, out, h->sb[h->last.stream].hits, (size_t)h->g.G * sizeof(int32_t));
}

int gv_get_miss(gv_handle h, int32_t *out)
{
  if (!h || !out) return GV_ERR_BAD_ARG;
  if (!h->last.miss) return GV_ERR_STATE;
  int rc = use_device(h);
  if (rc) return rc;
  if (sector_path(h)) {
    MissToI32Args ma;
    ma.freeN = h->fs[h->last.set].freeN; ma.freeT = h->fs[h->last.set].freeT;
    ma.nx = h->g.nx; ma.ny = h->g.ny; ma.nx_pad = h->nx_pad; ma.ny_pad = h->ny_pad;
    ma.out = h->scratch_i32;
    launch_miss_to_i32(ma, h->stream);
  } else {
    launch_u8_to_i32(h->miss8, h->scratch_i32, (size_t)h->g.G, h->stream);
  }
  GV_HIP(hipGetLastError());
  return copy_out(h, out, h->scratch_i32, (size_t)h->g.G * sizeof(int32_t));
}

// test hook (gv_test_hooks.h): the four end bitmaps of the last frame's buffer set as the tile pass left them, copied out
int gv_test_end_bitmaps(gv_handle h, uint32_t *hitN, uint32_t *clipN, uint32_t *hitT, uint32_t *clipT, int32_t *nxw,
                        int32_t *nyw, int32_t *nx_pad, int32_t *ny_pad)
{
  if (!h) return GV_ERR_BAD_ARG;
  const bool arrays = hitN && clipN && hitT && clipT;
  if (!arrays && (hitN || clipN || hitT || clipT)) return GV_ERR_BAD_ARG;   // all four or none
  if (!arrays && !(nxw && nyw && nx_pad && ny_pad)) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!sector_path(h)) return state_error(h, "gv_test_end_bitmaps", "the handle is not on the tile path");
  if (!h->last.miss) return state_error(h, "gv_test_end_bitmaps", "no binned frame has run");
  if (nxw) *nxw = h->nxw;
  if (nyw) *nyw = h->nyw;
  if (nx_pad) *nx_pad = h->nx_pad;
  if (ny_pad) *ny_pad = h->ny_pad;
  if (!arrays) return GV_OK;
  const FrameSet &f = h->fs[h->last.set];
  int rc = use_device(h);
  if (rc) return rc;
  GV_HIP(hipMemcpyAsync(hitN, f.hitN, h->bmN_words * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  GV_HIP(hipMemcpyAsync(clipN, f.clipN, h->bmN_words * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  GV_HIP(hipMemcpyAsync(hitT, f.hitT, h->bmT_words * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  GV_HIP(hipMemcpyAsync(clipT, f.clipT, h->bmT_words * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  GV_HIP(hipStreamSynchronize(h->stream));
  return GV_OK;
  GV_CATCH
}

int gv_get_cell_idx(gv_handle h, int32_t *out)
{
  if (!h || !out) return GV_ERR_BAD_ARG;
  if (!h->last.cell_idx) return GV_ERR_STATE;
  return copy_out(h, out, h->sb[h->last.points].cell_idx, h->n * sizeof(int32_t));
}

int gv_get_bbox_id(gv_handle h, int32_t *out)
{
  if (!h || !out) return GV_ERR_BAD_ARG;
  if (!h->last.bbox_id) return GV_ERR_STATE;
  GV_TRY
  int rc = use_device(h);
  if (rc) return rc;
  return read_back_ids(h, out);
  GV_CATCH
}

int gv_get_ray_stats(gv_handle h, uint64_t *n_rays, uint64_t *n_visits)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  const size_t slots = h->last.stat_slots;
  std::vector<unsigned long long> st(2 * slots, 0ull);
  int rc = copy_out(h, st.data(), h->fs[h->last.set].stats, st.size() * sizeof(unsigned long long));
  if (rc) return rc;
  unsigned long long rays = 0, visits = 0;
  for (size_t i = 0; i < slots; ++i) { rays += st[2 * i]; visits += st[2 * i + 1]; }
  if (n_rays) *n_rays = rays;
  if (n_visits) *n_visits = visits;
  return GV_OK;
  GV_CATCH
}

void *gv_stream(gv_handle h) { return h ? (void *)h->stream : nullptr; }

int gv_device_layers(gv_handle h, int8_t **occ_i8, float **log_odds, float **occupancy)
{
  if (!h) return GV_ERR_BAD_ARG;
  if (occ_i8) *occ_i8 = h->occ_i8;
  if (log_odds) *log_odds = h->log_odds;
  if (occupancy) *occupancy = h->occupancy;
  return GV_OK;
}

}  // extern "C"
