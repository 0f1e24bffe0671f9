// gv_api_frame.hip -- the frame pipeline of the C ABI: cloud and detection uploads, the building blocks of the
// tile-path frame, the pipelined / serial / generic frame, gv_frame_*, stage timing and the gv_debug_* entry points.
#include <atomic>
#include <algorithm>
#include <cstring>
#include <vector>

#include "gv_context.hpp"

namespace {

// keys / table entries one binning launch over n points needs (the chunk size follows n)
void bin_needs(const gv_context *h, size_t n, size_t &keys_need, size_t &tab_need)
{
  const uint32_t chunk = bin_chunk_for(n);
  const size_t n_wg = (n + chunk - 1) / chunk;
  keys_need = n_wg * chunk + 64;   // + slack: the tile pass reads whole 16-byte windows
  tab_need = n_wg * ((size_t)h->n_tiles + 1) + 2;
}

// layout of a detection block for `cap` entries (host staging and device copy share it)
struct DetLayout {
  size_t bboxes, poses, orient, conf, dims, total;
};
DetLayout det_layout(int32_t cap)
{
  DetLayout L;
  size_t o = 0;
  L.bboxes = o; o += (size_t)cap * sizeof(gv_bbox);
  L.poses = o;  o += (size_t)cap * sizeof(gv_lshape_pose);
  L.orient = o; o += (size_t)cap * 4 * sizeof(float);
  L.conf = o;   o += (size_t)cap * 2 * sizeof(float);
  L.dims = o;   o += (size_t)cap * 3 * sizeof(float);
  L.total = (o + 15) & ~(size_t)15;
  return L;
}

// generic path: the atomics-based count grids start every frame from zero
int clear_counts(gv_context *h)
{
  const size_t G = (size_t)h->g.G;
  GV_HIP(hipMemsetAsync(h->sb[0].hits, 0, G * sizeof(int32_t), h->stream));
  GV_HIP(hipMemsetAsync(h->miss8, 0, G, h->stream));
  GV_HIP(hipMemsetAsync(h->clip_end, 0, G, h->stream));
  h->counts_dirty = false;
  return GV_OK;
}

// sector-kernel arguments: the plan's fields beside the pointers and geometry of buffer set p
void fill_sector_args(const gv_context *h, const host::SectorPlan &P, SectorArgs &sa, int p)
{
  sa.g = h->g;
  sa.org = h->org;
  for (int o = 0; o < 8; ++o) { sa.log2s_oct[o] = P.log2s_oct[o]; sa.rev_oct[o] = P.rev_oct[o]; }
  for (int k = 0; k < 9; ++k) sa.wg_base[k] = (uint16_t)P.wg_base[k];
  sa.cap = P.cap;
  sa.log2m = P.log2m;
  sa.marks_words = P.marks_words;
  sa.oct_perm = P.oct_perm;
  sa.reorder = P.reorder;
  sa.n_helpers = P.n_helpers;
  sa.flat_k = P.flat_k;
  sa.march_limit = P.march_limit;
  sa.flat_direct = P.flat_direct;
  sa.ablate = 0;
  sa.dbg = nullptr;
#ifdef GV_DIAG
  sa.ablate = h->tune.ablate;
  sa.dbg = h->d_dbg;
  sa.tl = h->tl_slot(2);
#endif
  sa.hitN = h->fs[p].hitN; sa.clipN = h->fs[p].clipN; sa.hitT = h->fs[p].hitT; sa.clipT = h->fs[p].clipT;
  sa.nxw = h->nxw; sa.nyw = h->nyw; sa.nx_pad = h->nx_pad; sa.ny_pad = h->ny_pad;
  sa.freeN = h->fs[p].freeN;
  sa.freeT = h->fs[p].freeT;
  sa.stats = h->fs[p].stats;
}

}  // namespace

namespace gv_internal __attribute__((visibility("hidden"))) {

// buffers whose size follows the cloud: per-point outputs and the binning scratch, one of each per
// buffer set.  Growing them needs the frames in flight to finish first (rare: the cloud grew).
// n_slice > 0: binning launches over slices of n_slice points will run as well (the one-device emulation of
// the sharded frame): a slice may pick a smaller chunk than the whole cloud and then needs MORE table rows
int ensure_point_buffers(gv_context *h, size_t n, size_t n_slice)
{
  const int nsets = sector_path(h) ? 1 + h->tune.n_lanes : 1;   // per-stream copies
  const bool need_idx = n > h->idx_cap || !h->idx_cap;
  size_t keys_need, tab_need;
  bin_needs(h, n, keys_need, tab_need);
  for (size_t m : {n_slice, n_slice ? n_slice - 1 : (size_t)0}) {   // slices are floor or ceil of n / world
    if (!m) continue;
    size_t k2, t2;
    bin_needs(h, m, k2, t2);
    keys_need = std::max(keys_need, k2);
    tab_need = std::max(tab_need, t2);
  }
  const size_t slots_need = n / kBinSplitKeys + 1;
  const bool need_bin = sector_path(h) && (keys_need > h->bin_keys_cap || tab_need > h->bin_tab_cap || slots_need > h->bin_slots);
  if (!need_idx && !need_bin) return GV_OK;
  int rc = drain(h);
  if (rc) return rc;
  if (need_idx) {
    const size_t want = n + n / 8 + 1024;
    h->idx_cap = 0;
    for (int k = 0; k < nsets; ++k)
      if ((rc = h->sb[k].cell_idx.reserve(h, want)) || (rc = h->sb[k].bbox_id.reserve(h, want))) return rc;
    h->last.points = 0;   // new buffers: the standalone calls write stream 0's
    h->last.cell_idx = h->last.bbox_id = false;
    h->idx_cap = want;
  }
  if (need_bin) {
    const size_t keys_want = std::max(h->bin_keys_cap, keys_need + keys_need / 8);
    const size_t tab_want = std::max(h->bin_tab_cap, tab_need + tab_need / 8);
    const size_t slots_want = slots_need > h->bin_slots ? slots_need + slots_need / 8 : h->bin_slots;
    h->bin_keys_cap = h->bin_tab_cap = h->bin_slots = 0;
    for (int k = 0; k < nsets; ++k) {
      StreamBufs &b = h->sb[k];
      if ((rc = b.bin_keys.reserve(h, keys_want)) || (rc = b.bin_tab.reserve(h, tab_want)) ||
          (rc = b.bin_scratch.reserve(h, slots_want * kBinSplitMax * ((size_t)kBinTileCells + 512))))
        return rc;
    }
    h->bin_keys_cap = keys_want;
    h->bin_tab_cap = tab_want;
    h->bin_slots = slots_want;
  }
  return GV_OK;
}

int ensure_det(gv_context *h, DetSet &d, int32_t n)
{
  if (n <= d.cap) return GV_OK;
  if (d.cap) {   // frames that read this set must be past it (rare: the count grew)
    int rc0 = drain(h);
    if (rc0) return rc0;
  }
  const int32_t want = std::max(n + n / 4, 64);
  const DetLayout L = det_layout(want);
  d.cap = 0;
  int rc = d.block.reserve(h, L.total);
  if (rc) return rc;
  d.bboxes = reinterpret_cast<gv_bbox *>(d.block + L.bboxes);
  d.poses = reinterpret_cast<gv_lshape_pose *>(d.block + L.poses);
  d.orient = reinterpret_cast<float *>(d.block + L.orient);
  d.conf = reinterpret_cast<float *>(d.block + L.conf);
  d.dims = reinterpret_cast<float *>(d.block + L.dims);
  const size_t nmask = (size_t)h->bt_tiles_x * h->bt_tiles_y * (size_t)((want + 63) / 64);
  if ((rc = d.bbox_f.reserve(h, (size_t)want)) || (rc = d.tile_mask.reserve(h, nmask)) ||
      (rc = d.stage.reserve(h, L.total, hipHostMallocDefault)))
    return rc;
  d.cap = want;
  return GV_OK;
}

// rectangles and vision outputs (all buffer sets) and centre points follow the detection count; they
// are written by the frames in flight, hence the drain
int ensure_det_shared(gv_context *h, int32_t n)
{
  if (n <= h->vout_cap) return GV_OK;
  int rc = drain(h);
  if (rc) return rc;
  const int32_t want = std::max(n + n / 4, 64);
  h->vout_cap = 0;
  for (FrameSet &f : h->fs)
    if ((rc = f.rects.reserve(h, (size_t)want))) return rc;
  for (StreamBufs &b : h->sb)
    if ((rc = b.vout.reserve(h, (size_t)want))) return rc;
  if ((rc = h->d_pts.reserve(h, (size_t)want * 3))) return rc;
  h->vout_cap = want;
  return GV_OK;
}

BBoxTest bbox_test_of(const gv_context *h, const DetSet &d)
{
  BBoxTest t;
  t.bbox_f = d.bbox_f;
  t.tile_mask = d.tile_mask;
  t.tiles_x = h->bt_tiles_x;
  t.tiles_y = h->bt_tiles_y;
  t.mask_words = d.mask_words;
  return t;
}

// Arguments of the point kernel for the bbox test alone: points [lo, lo + n) of the resident cloud against detection
// set D, ids to ids[0, n).  The generic frame fills in its binning and ray fields on top.
PointsArgs bbox_points_args(const gv_context *h, const DetSet &D, size_t lo, size_t n, int16_t *ids)
{
  PointsArgs a{};
  a.x = h->cx + lo; a.y = h->cy + lo; a.z = h->cz + lo;
  a.n = (uint32_t)n;
  a.g = h->g;
  a.m_cam = h->m_cam;
  a.cam = h->camk;
  a.bt = bbox_test_of(h, D);
  a.bbox_id = ids;
  a.do_bbox = true;
  return a;
}

// Every frame form ends here.  set / stream: whose free-cell bitmaps and statistics, whose count grid.  points: the
// stream whose per-point outputs the flags cell_idx / bbox_id speak of.  The four flags: what the form produced.
void set_last_frame(gv_context *h, int set, int stream, int points, bool hits, bool miss, bool cell_idx, bool bbox_id)
{
  h->last = LastFrame{set, stream, points, hits, miss, cell_idx, bbox_id, h->last.stat_slots};   // (the ray stage sets stat_slots)
}

// Who read what: the frame that completes ev_fin[slot] used buffer set p, cloud set CS and detection set D, the
// latter on the streams in `readers`.  on_lane: it is in flight on a lane until the next drain; quiet: it counts
// towards the frames without an upload that open the third lane (gv_context::lanes_now).
void note_frame_readers(gv_context *h, int slot, int p, CloudSet &CS, DetSet &D, uint32_t readers, bool on_lane, bool quiet)
{
  h->last_fin_slot = slot;
  h->fs[p].fin_slot = slot;
  CS.release_slot = slot;
  D.release_slot = slot;
  D.readers |= readers;
  h->frame_no++;
  if (!on_lane) return;
  h->lane_frames++;
  h->pipe_busy = true;
  if (quiet && h->quiet_frames < 0x7fffffffu) h->quiet_frames++;
}

// Upload the small per-frame arrays into detection set `d` on stream `s` and derive the bbox-test
// tables there.  The caller's arrays are copied into the set's pinned staging block first (they are
// free on return) and the block goes to the device in ONE asynchronous copy.
// masks = false: the caller's kernels read the raw boxes / poses only (kNN depth, vision orientation, plain pose
// update) -- the thresholds and tile masks of the bbox test are not rebuilt, and whoever tests points against this
// set uploads it again first (every such call does).
// n_net >= 0: the network outputs cover n_net boxes (default: nb).  nb_test >= 0: the bbox test -- thresholds, tile
// masks, d.nb -- covers the first nb_test boxes only; what follows them in the block is read by other kernels (the
// tick keeps [all | static | dynamic] boxes in one block: one copy).
int upload_det(gv_context *h, DetSet &d, const DetUpload &u)
{
  const int32_t nb = u.nb, n_poses = u.n_poses;
  const int32_t n_net = u.n_net < 0 ? nb : u.n_net, nb_test = u.nb_test < 0 ? nb : u.nb_test;
  hipStream_t s = u.stream;
  int rc = ensure_det(h, d, std::max(nb, n_poses));
  if (rc) return rc;
  if ((rc = ensure_det_shared(h, std::max(nb, n_poses)))) return rc;
  if (d.ready) GV_HIP(hipEventSynchronize(d.ready));   // the staging's previous copy has left it
  const DetLayout L = det_layout(d.cap);
  size_t used = 0;   // the block is copied up to the end of the last array in use
  auto put = [&](size_t off, const void *src, size_t bytes) {
    if (!bytes) return;
    std::memcpy(d.stage + off, src, bytes);
    used = std::max(used, off + bytes);
  };
  put(L.bboxes, u.bboxes, (size_t)nb * sizeof(gv_bbox));
  put(L.poses, u.poses, (size_t)n_poses * sizeof(gv_lshape_pose));
  if (u.orient) put(L.orient, u.orient, (size_t)n_net * 4 * sizeof(float));
  if (u.conf) put(L.conf, u.conf, (size_t)n_net * 2 * sizeof(float));
  if (u.dims) put(L.dims, u.dims, (size_t)n_net * 3 * sizeof(float));
  d.mask_words = std::max(1, (nb_test + 63) / 64);
  BBoxPrepareArgs pa;
  pa.bboxes = d.bboxes; pa.nb = nb_test;
  pa.tiles_x = h->bt_tiles_x; pa.tiles_y = h->bt_tiles_y; pa.mask_words = d.mask_words;
  pa.bbox_f = d.bbox_f; pa.tile_mask = d.tile_mask;
  if (u.fused && used) {
    // fused: ONE kernel reads the pinned staging (device visible) -- copies the block and builds the tables from the
    // staged boxes -- instead of a copy command (7 us as a blit kernel) + the table kernel behind it
    pa.bboxes = reinterpret_cast<const gv_bbox *>(d.stage + L.bboxes);
    pa.nb = u.masks ? nb_test : 0;
    pa.copy_src = d.stage; pa.copy_dst = d.block; pa.copy_bytes = used;
    launch_bbox_prepare(pa, s);
  } else {
    if (used) GV_HIP(hipMemcpyAsync(d.block, d.stage, used, hipMemcpyHostToDevice, s));
    if (u.masks) launch_bbox_prepare(pa, s);
  }
  GV_HIP(hipGetLastError());
  d.nb = nb_test;
  d.n_poses = n_poses;
  d.valid = true;
  return GV_OK;
}

// bboxes only, synchronously, into the standalone set (extractCloudPerBBox and friends)
int upload_scratch_bboxes(gv_context *h, const gv_bbox *b, int32_t nb, bool masks)
{
  if (h->tick.pending) { h->err = "a tick is pending: call gv_tick_wait first"; return GV_ERR_STATE; }
  DetSet &d = h->det[2];
  // (fused: the table kernel reads the pinned staging itself -- one launch instead of a copy command + a kernel: 6 us)
  DetUpload u;
  u.bboxes = b; u.nb = nb;
  u.stream = h->stream;
  u.masks = masks;
  u.fused = true;
  int rc = upload_det(h, d, u);
  if (rc) return rc;
  GV_HIP(hipEventRecord(d.ready, h->stream));
  return GV_OK;
}

// poses / network outputs of detection set D -> index rectangles on stream s
int32_t enqueue_rects(gv_context *h, const DetSet &D, Rect *rects, VisionOut *vout, hipStream_t s)
{
  const bool vision = frame_flags(D.flags).vision;
  RectsFromPosesArgs ra;
  ra.poses = D.poses; ra.g = h->g; ra.bc = h->x_bc; ra.rects = rects;
  if (vision && D.nb > 0) {
    VisionArgs va;
    va.orient = D.orient; va.conf = D.conf; va.dims = D.dims; va.bboxes = D.bboxes; va.nb = D.nb;
    va.cam = h->cam; va.out = vout; va.poses_cam = D.poses;
    launch_vision(va, s);
    ra.n = D.nb; ra.from_cam = true;
    launch_rects_from_poses(ra, s);
    return D.nb;
  }
  if (!vision && D.n_poses > 0) {
    ra.n = D.n_poses; ra.from_cam = false;
    launch_rects_from_poses(ra, s);
    return D.n_poses;
  }
  return 0;
}

int check_frame_flags(const gv_context *h, uint32_t fl)
{
  const FrameFlags f = frame_flags(fl);
  if (f.ray && !f.bin) return GV_ERR_BAD_ARG;
  if (f.bin && !h->has_bl) return GV_ERR_TF;
  if (f.bbox && !h->has_cl) return GV_ERR_TF;
  if (f.vision && !h->has_bc) return GV_ERR_TF;
  return GV_OK;
}

// --- building blocks of the tile-path frame (shared by the one-GPU frame, the sharded frame and its
// one-device emulation) ---

// partition + tile histogram of points [lo, lo + n) of the current cloud on stream k: that stream's hits[]
// (or not), per-point outputs and binning scratch; the end bitmaps of buffer set p; zeroes the set's
// free-cell bitmaps.  (BinningJob, gv_context.hpp, says what each field asks for.)
int enqueue_binning(gv_context *h, const BinningJob &job)
{
  const DetSet &D = job.det;
  const int p = job.set, k = job.stream;
  const size_t lo = job.lo, n = job.n;
  Rect *const fold_rects = job.fold_rects;
  const bool timed = job.timed;
  hipStream_t s = h->streams[k];
  const uint32_t chunk = bin_chunk_for(n);
  const uint32_t n_wg = (uint32_t)((n + chunk - 1) / chunk);
  {   // the partition pass writes n_wg table rows and n_wg * chunk keys: never past what was allocated
    size_t keys_need, tab_need;
    bin_needs(h, n, keys_need, tab_need);
    if (keys_need > h->bin_keys_cap || tab_need > h->bin_tab_cap || lo + n > h->idx_cap) {
      h->err = "binning scratch too small for this launch";
      return GV_ERR_STATE;
    }
  }
  BinArgs a{};
  a.x = h->cx + lo; a.y = h->cy + lo; a.z = h->cz + lo;
  a.n = (uint32_t)n;
  a.g = h->g;
  a.m_base = h->m_base;
  a.m_cam = h->m_cam;
  a.cam = h->camk;
  a.org = h->org;
  a.bt = bbox_test_of(h, D);
  a.nb = D.nb;
  a.nb_pad = (D.nb + 3) & ~3;
  a.bbox_id = h->sb[k].bbox_id + lo;
  a.cell_idx = job.keep_cell ? h->sb[k].cell_idx + lo : nullptr;
  a.do_ray = job.do_ray;
  // the fused bbox test keeps its tables in LDS; a detection set too large for that (hundreds of boxes, or a
  // large image: one mask word per 16x16-pixel tile) runs the test as a pass of its own over the cloud
  const bool bbox_fused = job.do_bbox && bin_bbox_fits(D.nb, a.bt);
  a.do_bbox = bbox_fused;
  a.chunk = chunk;
  a.n_wg = n_wg;
  a.tiles_x = h->tiles_x; a.tiles_y = h->tiles_y; a.n_tiles = h->n_tiles;
  a.keys = h->sb[k].bin_keys;
  a.tab = h->sb[k].bin_tab;
  a.tile_total = h->sb[k].bin_total[h->sb[k].bin_parity];
  a.band = h->band;
  if (fold_rects) {   // the frame's rectangles ride the partition launch
    a.rect_poses = D.poses;
    a.n_rect_poses = D.n_poses;
    a.rects_out = fold_rects;
  }
#ifdef GV_DIAG
  a.dbg = h->d_bin_dbg[0];
  a.tl = h->tl_slot(0);
#endif
  launch_bin_partition(a, s, timed ? h->kt[0][0] : nullptr, timed ? h->kt[0][1] : nullptr, job.any_order);
  h->sb[k].lane_clean = false;
  if (timed) h->kt_used[0] = n > 0 || fold_rects;
  if (job.do_bbox && !bbox_fused) launch_points(bbox_points_args(h, D, lo, n, a.bbox_id), s);
  if (job.ev_points) GV_HIP(hipEventRecord(job.ev_points, s));
  BinTileArgs t{};
  t.nx = h->g.nx; t.ny = h->g.ny;
  t.tiles_x = h->tiles_x; t.tiles_y = h->tiles_y; t.n_tiles = h->n_tiles;
  t.n_wg = n_wg;
  t.chunk = chunk;
  t.keys = h->sb[k].bin_keys;
  t.tab = h->sb[k].bin_tab;
  t.tile_total = h->sb[k].bin_total[h->sb[k].bin_parity];
  t.tile_total_next = h->sb[k].bin_total[h->sb[k].bin_parity ^ 1];
  t.done = h->sb[k].bin_done;
  t.scratch = h->sb[k].bin_scratch;
  t.split_keys = kBinSplitKeys;
  t.max_slots = (uint32_t)h->bin_slots;
  t.hits = job.write_hits ? h->sb[k].hits : nullptr;
  t.hitN = h->fs[p].hitN; t.clipN = h->fs[p].clipN; t.hitT = h->fs[p].hitT; t.clipT = h->fs[p].clipT;
  t.freeN = h->fs[p].freeN; t.freeT = h->fs[p].freeT;
  t.nxw = h->nxw; t.nyw = h->nyw; t.nx_pad = h->nx_pad; t.ny_pad = h->ny_pad;
#ifdef GV_DIAG
  t.dbg = h->d_bin_dbg[1];
  t.tl = h->tl_slot(1);
#endif
  launch_bin_tiles(t, (uint32_t)(n / kBinSplitKeys), s, timed ? h->kt[1][0] : nullptr, timed ? h->kt[1][1] : nullptr);
  if (timed) h->kt_used[1] = true;
  h->sb[k].bin_parity ^= 1;
  GV_HIP(hipGetLastError());
  return GV_OK;
}

// sector ray stage over the end bitmaps of set job.set into its free-cell bitmaps; workgroups first,
// first + stride, ... of the dispatch order (one GPU: 0, 1)
int enqueue_sectors(gv_context *h, SectorsJob &job)
{
  job.done_attached = false;
  if (!h->org.valid) return GV_OK;
  const host::SectorPlan P(h->g.nx, h->g.ny, h->org.cx, h->org.cy, h->n, h->tune.sec);
  if (const uint32_t v = P.violations()) { h->err = host::SectorPlan::violation_name(v); return GV_ERR_BAD_ARG; }
  SectorArgs sa{};
  fill_sector_args(h, P, sa, job.set);
  sa.wg_first = job.first;
  sa.wg_stride = job.stride;
  h->last.stat_slots = P.stat_slots;
  const bool launched = launch_ray_sectors(sa, {P.ch, P.lds_bytes, (int)P.total_workgroups}, job.stream, job.done, job.t0);
  job.done_attached = launched && job.done;
  GV_HIP(hipGetLastError());
  return GV_OK;
}

// The tile grid pass over rows [job.y0, job.y1) with the bitmaps of set job.set.
int enqueue_grid_pass(gv_context *h, GridPassJob &job)
{
  const int p = job.set;
  const int32_t y0 = job.y0, y1 = job.y1;
  // a sharded pass writes this rank's band whole and leaves the layers out of step (gv_context::layers_in_step)
  const bool dense = job.sharded || h->grid_pass_dense();
  FinalizeTileArgs t{};
  t.g = h->g;
  t.log_odds = h->log_odds;
  t.occupancy = h->occupancy;
  t.occ_i8 = h->occ_i8;
  t.rects = job.rects;
  t.n_rects = job.n_rects;
  t.hitN = h->fs[p].hitN;
  t.freeN = h->fs[p].freeN;
  t.freeT = h->fs[p].freeT;
  t.nx_pad = h->nx_pad;
  t.ny_pad = h->ny_pad;
  t.counts = job.counts;
  t.dense = dense;
  t.y_begin = y0;
  t.y_end = y1;
#ifdef GV_DIAG
  if (job.of_frame) t.tl = h->tl_slot(3);
#endif
  const bool ran = launch_finalize_tiles(t, job.stream, job.done, job.t0);
  if (job.sharded) h->layers_in_step = false;
  else if (ran && dense && y0 <= 0 && y1 >= h->g.ny) h->layers_in_step = true;
  job.launched = ran;
  if (!ran && job.done) GV_HIP(hipEventRecord(job.done, job.stream));
  GV_HIP(hipGetLastError());
  return GV_OK;
}

// Stream k (0 public, 1 / 2 the lanes) reads cloud C: ordered after its upload (once per upload and stream).  The
// frames' wait and the scan matchers' (gv_api_match.hip, k = 0).
int wait_cloud(gv_context *h, CloudSet &C, int k)
{
  if (!(C.seen >> k & 1u)) {
    GV_HIP(hipStreamWaitEvent(h->streams[k], C.ready, 0));
    C.seen |= 1u << k;
    h->sb[k].lane_clean = false;
  }
  return GV_OK;
}

// ... and detection set D likewise
int wait_inputs(gv_context *h, CloudSet &C, DetSet &D, int k)
{
  hipStream_t s = h->streams[k];
  if (int rc = wait_cloud(h, C, k)) return rc;
  if (!(D.seen >> k & 1u)) {
    GV_HIP(hipStreamWaitEvent(s, D.ready, 0));
    D.seen |= 1u << k;
    h->sb[k].lane_clean = false;
  }
  return GV_OK;
}

}  // namespace gv_internal

namespace {

// The tile-path frame: rectangles + partition, tile histogram + end bitmaps, sector ray stage back to
// back on one in-order stream, then the grid pass on the public stream.  pipelined: the stream of lane
// n % lanes and buffer set 1 + n % (2 * lanes) (n = lane frames so far), the grid pass behind one event.  Serial
// (GV_PIPELINE=0, stage timing): everything on the public stream, buffer set 0.  The sharded frame has its own
// enqueue (enqueue_frame_sharded).
int enqueue_frame_tiles(gv_context *h, bool pipelined, bool stage_events)
{
  DetSet &D = h->det[h->det_cur];
  const FrameFlags f = frame_flags(D.flags);
  int rc = check_frame_flags(h, D.flags);
  if (rc) return rc;
  const int p = pipelined ? 1 + (int)(h->lane_frames % (uint64_t)(2 * h->tune.n_lanes)) : 0;
  const int k = pipelined ? 1 + (int)(h->lane_frames % (uint64_t)h->lanes_now()) : 0;
  hipStream_t s = h->streams[k];
  // back-pressure: the frame that last used this buffer set (four frames ago) has finished
  if (pipelined && h->fs[p].fin_slot >= 0) GV_HIP(hipEventSynchronize(h->ev_fin[h->fs[p].fin_slot]));
  CloudSet &CS = h->cloud[h->cloud_cur];
#ifdef GV_DIAG
  auto mark = [&](hipStream_t st) {   // device timeline of the pipelined frame (gv_debug_pipeline_trace)
    if (!h->trace) return;
    Event e;
    if (e.create(hipEventDefault) != hipSuccess) return;
    (void)hipEventRecord(e, st);
    h->trace->push_back(std::move(e));
  };
#else
  auto mark = [](hipStream_t) {};
#endif
  if ((rc = wait_inputs(h, CS, D, k))) return rc;
  if (stage_events) {
    GV_HIP(hipEventRecord(h->ev[0], s));
    for (bool &u : h->kt_used) u = false;
  }

  // --- detections -> rectangles.  Base-frame poses of a binning frame ride the partition launch (one
  // extra workgroup) instead of a launch of their own; network outputs go through the vision kernels.
  Rect *rects = h->fs[p].rects;
  const bool fold_rects = f.bin && !f.vision && D.n_poses > 0;
  mark(s);
  if (!fold_rects) h->sb[k].lane_clean = false;   // (the rectangle / vision kernels go on the lane)
  const int32_t n_rects = fold_rects ? D.n_poses : enqueue_rects(h, D, rects, h->sb[k].vout, s);
  mark(s);
  if (stage_events) GV_HIP(hipEventRecord(h->ev[kStageDetections + 1], s));
  bool part_any_order = pipelined && !stage_events && h->tune.anyorder && h->sb[k].lane_clean;
#ifdef GV_DIAG
  if (h->trace) part_any_order = false;   // the trace markers are packets on the lane
#endif

  // --- points: partition by tile (+ ray ends, bbox test), then the tile histogram: hits[] + end bitmaps
  mark(s);
  if (f.bin) {
    BinningJob bin{D};
    bin.set = p; bin.stream = k;
    bin.n = h->n;
    bin.keep_cell = f.keep_cell; bin.do_ray = f.ray; bin.do_bbox = f.bbox;
    bin.write_hits = true;
    bin.fold_rects = fold_rects ? rects : nullptr;
    bin.ev_points = stage_events ? h->ev[kStagePoints + 1] : nullptr;
    bin.timed = stage_events;
    bin.any_order = part_any_order;
    if ((rc = enqueue_binning(h, bin))) return rc;
  } else {
    h->sb[k].lane_clean = false;
    if (f.bbox) launch_points(bbox_points_args(h, D, 0, h->n, h->sb[k].bbox_id), s);
    if (stage_events) GV_HIP(hipEventRecord(h->ev[kStagePoints + 1], s));
  }
  mark(s);
  mark(s); mark(s);   // (trace slot of the former bitmap kernel: the tile pass is part of the binning pair)
  if (stage_events) GV_HIP(hipEventRecord(h->ev[kStageRayCompact + 1], s));

  // --- free-space ray stage.  On a lane its completion event rides the kernel's own dispatch packet.
  const int slot = (int)(h->frame_no % (uint64_t)gv_context::kRing);
  SectorsJob sec;
  sec.set = p; sec.stream = s;
  sec.done = pipelined ? h->ev_sec[slot] : (stage_events ? h->kt[2][1] : nullptr);
  sec.t0 = stage_events ? h->kt[2][0] : nullptr;
  mark(s);
  if (f.ray && (rc = enqueue_sectors(h, sec))) return rc;
  const bool sec_event = sec.done_attached;
  if (stage_events) h->kt_used[2] = sec_event;
  // the lane now ends in a sector kernel that carries its own completion event: nothing behind it
  h->sb[k].lane_clean = pipelined && f.bin && f.ray && sec_event;
  mark(s);
  if (stage_events) GV_HIP(hipEventRecord(h->ev[kStageRayMarch + 1], s));

  // --- grid pass, on the public stream: in order behind the previous frame's and behind whatever the
  // caller queued there (the download of the previous grid, a plain map update)
  if (pipelined) {
    if (!sec_event) GV_HIP(hipEventRecord(h->ev_sec[slot], s));
    GV_HIP(hipStreamWaitEvent(h->stream, h->ev_sec[slot], 0));
    s = h->stream;
  }

  mark(s);
  // ev_fin[slot] completes with the grid pass: this frame done => every earlier frame done
  // (stage timing: the kernel carries its own start / end events, ev_fin follows as a marker)
  GridPassJob grid;
  grid.set = p; grid.stream = s;
  grid.rects = rects; grid.n_rects = n_rects;
  grid.counts = f.bin;
  grid.y1 = h->g.ny;
  grid.done = stage_events ? h->kt[3][1] : h->ev_fin[slot];
  grid.t0 = stage_events ? h->kt[3][0] : nullptr;
  if ((rc = enqueue_grid_pass(h, grid))) return rc;
  if (stage_events) {
    h->kt_used[3] = grid.launched;
    GV_HIP(hipEventRecord(h->ev_fin[slot], s));
  }
  mark(s);
  if (stage_events) GV_HIP(hipEventRecord(h->ev[kStageFinalize + 1], s));
  // cloud, detection set and buffer set remember their last user: this frame, which read D on its own stream only
  note_frame_readers(h, slot, p, CS, D, 1u << k, pipelined, true);
  // the tile pass writes every cell of hits[], and the free-cell bitmaps of set p stay until the set's next frame: a
  // BIN frame has both whether or not it kept anything
  set_last_frame(h, p, k, k, f.bin, f.bin, f.bin && f.keep_cell, f.bbox);
  return GV_OK;
}

// Generic frame: any grid shape (nx % 4 != 0, more than 8000 cells per side, GV_RAY_IMPL=simple).
// One stream; atomics-based count grids; literal per-ray march.
int enqueue_frame_generic(gv_context *h, bool stage_events)
{
  DetSet &D = h->det[h->det_cur];
  const FrameFlags f = frame_flags(D.flags);
  int rc = check_frame_flags(h, D.flags);
  if (rc) return rc;
  if (h->counts_dirty && (rc = clear_counts(h))) return rc;
  hipStream_t s = h->stream;
  CloudSet &CS = h->cloud[h->cloud_cur];
  if ((rc = wait_inputs(h, CS, D, 0))) return rc;
  if (stage_events) GV_HIP(hipEventRecord(h->ev[0], s));
  const int32_t n_rects = enqueue_rects(h, D, h->fs[0].rects, h->sb[0].vout, s);
  if (stage_events) GV_HIP(hipEventRecord(h->ev[kStageDetections + 1], s));
  int32_t *const hits = h->sb[0].hits;
  if (f.bin || f.bbox) {
    PointsArgs a = bbox_points_args(h, D, 0, h->n, h->sb[0].bbox_id);
    a.m_base = h->m_base;
    a.org = h->org;
    a.hits = hits;
    a.clip_end = h->clip_end;
    a.cell_idx = f.keep_cell ? h->sb[0].cell_idx.get() : nullptr;
    a.do_bin = f.bin; a.do_ray = f.ray; a.do_bbox = f.bbox;
    a.band = h->band;
    launch_points(a, s);
  }
  if (stage_events) GV_HIP(hipEventRecord(h->ev[kStagePoints + 1], s));
  if (f.ray && h->org.valid) {
    GV_HIP(hipMemsetAsync(h->ray_count, 0, sizeof(uint32_t), s));
    GV_HIP(hipMemsetAsync(h->fs[0].stats, 0, 2 * sizeof(unsigned long long), s));
    h->last.stat_slots = 1;
    RayCompactArgs rc_a;
    rc_a.hits = hits; rc_a.clip_end = h->clip_end; rc_a.g = h->g;
    rc_a.list = h->ray_list; rc_a.count = h->ray_count;
    launch_ray_compact(rc_a, s);
    if (stage_events) GV_HIP(hipEventRecord(h->ev[kStageRayCompact + 1], s));
    RayMarchArgs rm;
    rm.list = h->ray_list; rm.count = h->ray_count; rm.g = h->g; rm.org = h->org;
    rm.miss = h->miss8; rm.stats = h->fs[0].stats;
    launch_ray_march(rm, s);
    if (stage_events) GV_HIP(hipEventRecord(h->ev[kStageRayMarch + 1], s));
  } else if (stage_events) {
    GV_HIP(hipEventRecord(h->ev[kStageRayCompact + 1], s));
    GV_HIP(hipEventRecord(h->ev[kStageRayMarch + 1], s));
  }
  FinalizeArgs fin = finalize_args(h, n_rects);
  fin.hits = f.bin ? hits : nullptr;
  fin.miss = h->miss8;
  fin.clip_end = h->clip_end;
  fin.zero_counts = f.bin && !f.keep_counts;
  launch_finalize(fin, s);
  if (stage_events) GV_HIP(hipEventRecord(h->ev[kStageFinalize + 1], s));
  GV_HIP(hipGetLastError());
  const int slot = (int)(h->frame_no % (uint64_t)gv_context::kRing);
  GV_HIP(hipEventRecord(h->ev_fin[slot], s));   // cloud and detection set remember their last reader
  note_frame_readers(h, slot, 0, CS, D, 1u, false, false);   // everything on the public stream
  h->counts_dirty = f.bin && f.keep_counts;
  // the grid pass zeroes the count grids for the next frame unless the caller asked to keep them
  set_last_frame(h, 0, 0, 0, f.bin && f.keep_counts, f.bin && f.keep_counts, f.bin && f.keep_cell, f.bbox);
  return GV_OK;
}

// The next cloud set in rotation (read two uploads ago at the latest), grown to n points, with the copy
// stream ordered after the last frame that read it, and after a pending tick that reads it: the tick's use_device
// forgot every earlier reader, and the third upload after gv_tick_enqueue comes back to the tick's set.
int begin_cloud_upload(gv_context *h, size_t n, int &target)
{
  int rc = set_device_only(h);
  if (rc) return rc;
  if ((rc = ensure_point_buffers(h, n))) return rc;
  target = (h->cloud_cur + 1) % 3;
  h->quiet_frames = 0;   // the upload stream is in use: the frames stay off it for a while
  CloudSet &c = h->cloud[target];
  const bool tick_reads = h->tick.pending && h->tick.cloud == target;
  const bool match_reads = (h->scan_readers.clouds >> target & 1u) != 0;   // a gv_match_scan* / gv_match_search* enqueued since reads this set
  if (n > c.cap) {
    if (c.release_slot >= 0) GV_HIP(hipEventSynchronize(h->ev_fin[c.release_slot]));
    if (tick_reads) GV_HIP(hipEventSynchronize(h->tick.done));   // the tick's kernels read the block freed here
    if (match_reads) GV_HIP(hipEventSynchronize(h->scan_readers.read));
    GV_HIP(hipEventSynchronize(c.ready));
    c.cap = 0;
    const size_t want = (n + n / 8 + 1024 + 3) & ~(size_t)3;   // the arrays sit at a stride of (n + 3) & ~3 floats
    if ((rc = c.base.reserve(h, 3 * want))) return rc;
    c.cap = want;
  }
  const size_t n4 = (n + 3) & ~(size_t)3;   // 16-byte aligned arrays
  c.x = c.base;
  c.y = c.base + n4;
  c.z = c.base + 2 * n4;
  // ordered after the last frame that read this set (if the ring slot has been re-recorded since, that is
  // a later frame: it only waits longer)
  // (asked first on the host: in a streaming run that frame finished long ago, and a wait that is already
  // satisfied would still put a barrier packet -- ~6 us of queue time -- in front of every copy)
  if (c.release_slot >= 0 && hipEventQuery(h->ev_fin[c.release_slot]) != hipSuccess)
    GV_HIP(hipStreamWaitEvent(h->stream_copy, h->ev_fin[c.release_slot], 0));
  if (tick_reads) GV_HIP(hipStreamWaitEvent(h->stream_copy, h->tick.done, 0));   // on the device: the upload stays asynchronous
  if (match_reads) {   // the event of the last call: behind every earlier call's point pass on the public stream
    GV_HIP(hipStreamWaitEvent(h->stream_copy, h->scan_readers.read, 0));
    h->scan_readers.clouds &= ~(1u << target);
  }
  c.release_slot = -1;
  return GV_OK;
}

int end_cloud_upload(gv_context *h, int target, size_t n)
{
  CloudSet &c = h->cloud[target];
  GV_HIP(hipEventRecord(c.ready, h->stream_copy));
  c.seen = 0;   // every stream that reads it waits for `ready` once
  h->cloud_cur = target;
  h->cx = c.x; h->cy = c.y; h->cz = c.z;
  h->n = n;
  h->cloud_wait = true;
  h->last.cell_idx = h->last.bbox_id = false;   // they spoke of the cloud before this one
  return GV_OK;
}

// the four upload entry points: argument checks, then the copies on the upload stream; wait: until they have landed
int upload_xyz(gv_context *h, const float *x, const float *y, const float *z, size_t n, bool wait)
{
  if (!h || (n && (!x || !y || !z)) || n > 0x7fffffffu) return GV_ERR_BAD_ARG;
  GV_TRY
  int target = 0;
  int rc = begin_cloud_upload(h, n, target);
  if (rc) return rc;
  CloudSet &c = h->cloud[target];
  if (n) {
    // the copy engine does ~54 GB/s inside a copy and leaves ~10 us between copies: x, y, z laid out back to
    // back in one (pinned) block go up in a single copy
    if (y == x + n && z == y + n && (n & 3) == 0) {
      GV_HIP(hipMemcpyAsync(c.x, x, 3 * n * sizeof(float), hipMemcpyHostToDevice, h->stream_copy));
    } else {
      GV_HIP(hipMemcpyAsync(c.x, x, n * sizeof(float), hipMemcpyHostToDevice, h->stream_copy));
      GV_HIP(hipMemcpyAsync(c.y, y, n * sizeof(float), hipMemcpyHostToDevice, h->stream_copy));
      GV_HIP(hipMemcpyAsync(c.z, z, n * sizeof(float), hipMemcpyHostToDevice, h->stream_copy));
    }
  }
  if ((rc = end_cloud_upload(h, target, n))) return rc;
  if (wait) GV_HIP(hipEventSynchronize(c.ready));
  return GV_OK;
  GV_CATCH
}

int upload_pc2(gv_context *h, const uint8_t *data, size_t n, uint32_t point_step, uint32_t off_x, uint32_t off_y,
               uint32_t off_z, bool wait)
{
  if (!h || (n && !data) || n > 0x7fffffffu) return GV_ERR_BAD_ARG;
  if (point_step < 4 || off_x + 4 > point_step || off_y + 4 > point_step || off_z + 4 > point_step)
    return GV_ERR_BAD_ARG;
  GV_TRY
  int target = 0;
  int rc = begin_cloud_upload(h, n, target);
  if (rc) return rc;
  CloudSet &c = h->cloud[target];
  const size_t bytes = n * (size_t)point_step;
  if (bytes + 16 > c.raw.cap()) {
    GV_HIP(hipEventSynchronize(c.ready));   // the previous de-interleave out of this buffer is done
    if ((rc = c.raw.reserve(h, bytes + bytes / 8 + 16))) return rc;
  }
  if (n) {
    GV_HIP(hipMemcpyAsync(c.raw, data, bytes, hipMemcpyHostToDevice, h->stream_copy));
    DeinterleaveArgs da;
    da.data = c.raw; da.n = (uint32_t)n; da.point_step = point_step;
    da.off_x = off_x; da.off_y = off_y; da.off_z = off_z;
    da.x = c.x; da.y = c.y; da.z = c.z;
    launch_deinterleave(da, h->stream_copy);
    GV_HIP(hipGetLastError());
  }
  if ((rc = end_cloud_upload(h, target, n))) return rc;
  if (wait) GV_HIP(hipEventSynchronize(c.ready));
  return GV_OK;
  GV_CATCH
}

int set_detections(gv_context *h, const gv_frame_desc *d)
{
  if (d->n_bboxes < 0 || d->n_poses < 0) return GV_ERR_BAD_ARG;
  if (d->n_bboxes && !d->bboxes) return GV_ERR_BAD_ARG;
  const bool vision = d->flags & GV_FRAME_VISION_ORIENT;
  if (vision && d->n_bboxes && (!d->orient || !d->conf || !d->dims)) return GV_ERR_BAD_ARG;
  if (!vision && d->n_poses && !d->poses) return GV_ERR_BAD_ARG;
  int rc = set_device_only(h);
  if (rc) return rc;
  // The other detection set (frames already enqueued read the current one), uploaded on the stream of the
  // frame that will read it first: in order before that frame.  The frames that read the set's previous
  // contents: when all of them ran on that same lane (every frame brings new detections: two sets, two
  // lanes) the upload is already in order behind them; a set that was read on another stream as well (a
  // detection set kept for several frames is read on both lanes) waits for the grid pass of its last
  // reader, which completes after every earlier frame.
  const int target = h->det_cur ^ 1;
  DetSet &D = h->det[target];
  const int k = (sector_path(h) && !h->tune.no_pipeline) ? 1 + (int)(h->lane_frames % (uint64_t)h->lanes_now()) : 0;
  hipStream_t s = h->streams[k];
  h->sb[k].lane_clean = false;   // the upload and the table kernels go on this stream, in front of the frame's partition pass
  if (D.release_slot >= 0 && D.readers != (1u << k)) GV_HIP(hipStreamWaitEvent(s, h->ev_fin[D.release_slot], 0));
  const bool net = vision && d->n_bboxes;
  DetUpload u;
  u.bboxes = d->bboxes; u.nb = d->n_bboxes;
  if (!vision) { u.poses = d->poses; u.n_poses = d->n_poses; }
  if (net) { u.orient = d->orient; u.conf = d->conf; u.dims = d->dims; }
  u.stream = s;
  if ((rc = upload_det(h, D, u))) return rc;
  D.flags = d->flags;
  GV_HIP(hipEventRecord(D.ready, s));
  D.seen = 1u << k;
  D.release_slot = -1;
  D.readers = 0;
  h->det_cur = target;
  return GV_OK;
}

}  // namespace

extern "C" {

int gv_cloud_upload_xyz(gv_handle h, const float *x, const float *y, const float *z, size_t n)
{
  return upload_xyz(h, x, y, z, n, true);
}

int gv_cloud_upload_xyz_async(gv_handle h, const float *x, const float *y, const float *z, size_t n)
{
  return upload_xyz(h, x, y, z, n, false);
}

int gv_cloud_upload_pointcloud2(gv_handle h, const uint8_t *data, size_t n, uint32_t point_step, uint32_t off_x,
                                uint32_t off_y, uint32_t off_z)
{
  return upload_pc2(h, data, n, point_step, off_x, off_y, off_z, true);
}

int gv_cloud_upload_pointcloud2_async(gv_handle h, const uint8_t *data, size_t n, uint32_t point_step, uint32_t off_x,
                                      uint32_t off_y, uint32_t off_z)
{
  return upload_pc2(h, data, n, point_step, off_x, off_y, off_z, false);
}

int gv_cloud_upload_wait(gv_handle h)
{
  if (!h) return GV_ERR_BAD_ARG;
  int rc = set_device_only(h);
  if (rc) return rc;
  // the clouds' own `ready` events, not the upload stream: the third lane's frames run on that stream too and are
  // none of this call's business (round-3 advisor finding)
  for (auto &c : h->cloud) GV_HIP(hipEventSynchronize(c.ready));
  return GV_OK;
}

int gv_frame_set_detections(gv_handle h, const gv_frame_desc *d)
{
  if (!h || !d) return GV_ERR_BAD_ARG;
  GV_TRY
  return set_detections(h, d);
  GV_CATCH
}

// (the upload is asynchronous either way: the set's `ready` event orders the frames behind it)
int gv_frame_set_detections_async(gv_handle h, const gv_frame_desc *d) { return gv_frame_set_detections(h, d); }

int gv_frame_enqueue(gv_handle h)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!h->det[h->det_cur].valid) return GV_ERR_STATE;   // no gv_frame_set_detections yet
  if (sector_path(h) && !h->tune.no_pipeline) {
    int rc = set_device_only(h);
    if (rc) return rc;
    return enqueue_frame_tiles(h, true, false);
  }
  int rc = use_device(h);
  if (rc) return rc;
  return sector_path(h) ? enqueue_frame_tiles(h, false, false) : enqueue_frame_generic(h, false);
  GV_CATCH
}

int gv_frame_fence(gv_handle h)
{
  if (!h) return GV_ERR_BAD_ARG;
  int rc = set_device_only(h);
  if (rc) return rc;
  // Every frame ends with its grid pass on the public stream, behind an event that follows its other
  // kernels: frames are already in order there.  What is left to join is the copy stream.
  if (h->cloud_wait) {
    GV_HIP(hipEventRecord(h->ev_join, h->stream_copy));
    GV_HIP(hipStreamWaitEvent(h->stream, h->ev_join, 0));
  }
  return GV_OK;
}

int gv_synchronize(gv_handle h)
{
  if (!h) return GV_ERR_BAD_ARG;
  int rc = set_device_only(h);
  if (rc) return rc;
  return drain(h);
}

int gv_process_frame(gv_handle h, const gv_frame_desc *desc)
{
  int rc = gv_frame_set_detections(h, desc);
  if (rc) return rc;
  if ((rc = gv_frame_enqueue(h))) return rc;
  return gv_synchronize(h);
}

#ifdef GV_DIAG
// diagnostic build only (tools/native_timeline.py, GV_TIMELINE=1): reset (out == nullptr) or copy out the
// {begin, end} clock pairs of the four kernels of the last `frames` <= 4096 frames, slot = frame number % 4096
int gv_debug_timeline(gv_handle h, unsigned long long *out, size_t frames)
{
  if (!h || !h->d_tl || frames > gv_context::kTlFrames) return GV_ERR_STATE;
  GV_TRY
  int rc = use_device(h);
  if (rc) return rc;
  GV_HIP(hipDeviceSynchronize());
  const size_t n = gv_context::kTlFrames * 8;
  if (!out) {
    std::vector<unsigned long long> init(n);
    for (size_t i = 0; i < n; i += 2) { init[i] = ~0ull; init[i + 1] = 0ull; }
    GV_HIP(hipMemcpy(h->d_tl, init.data(), n * sizeof(unsigned long long), hipMemcpyHostToDevice));
    return GV_OK;
  }
  GV_HIP(hipMemcpy(out, h->d_tl, frames * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return GV_OK;
  GV_CATCH
}
uint64_t gv_debug_frame_no(gv_handle h) { return h ? h->frame_no : 0; }

// diagnostic build only (tools/sector_phases.py): copies the phase stamps of the last sector launch
int gv_debug_sector_stamps(gv_handle h, unsigned long long *out, size_t n_wg)
{
  if (!h || !out || !h->d_dbg) return GV_ERR_STATE;
  return copy_out(h, out, h->d_dbg, n_wg * 16 * sizeof(unsigned long long));
}

// diagnostic build only (tools/bin_phases.py): phase stamps of the last partition (which = 0) / tile (1) launch
int gv_debug_bin_stamps(gv_handle h, int which, unsigned long long *out, size_t n_wg)
{
  if (!h || !out || which < 0 || which > 1 || !h->d_bin_dbg[which] || n_wg > 8192) return GV_ERR_STATE;
  return copy_out(h, out, h->d_bin_dbg[which], n_wg * 16 * sizeof(unsigned long long));
}

// diagnostic build only: enqueue `frames` pipelined frames with timing events around every kernel;
// out[frame*10 + 2*k + {0,1}] = start/end in us of kernel k (rects, partition, tiles, sectors, grid pass)
int gv_debug_pipeline_trace(gv_handle h, int32_t frames, float *out)
{
  if (!h || frames <= 0 || !out) return GV_ERR_BAD_ARG;
  GV_TRY
  int rc = use_device(h);
  if (rc) return rc;
  std::vector<Event> ev;
  Event e0;
  GV_HIP(e0.create(hipEventDefault));
  GV_HIP(hipEventRecord(e0, h->stream));
  h->trace = &ev;
  for (int32_t i = 0; i < frames && rc == GV_OK; ++i) rc = gv_frame_enqueue(h);
  h->trace = nullptr;
  int rc2 = use_device(h);
  for (size_t k = 0; k < ev.size(); ++k) {
    float ms = 0.f;
    if (k < (size_t)frames * 10 && hipEventElapsedTime(&ms, e0, ev[k]) == hipSuccess) out[k] = ms * 1000.f;
  }
  return rc ? rc : rc2;
  GV_CATCH
}
#endif

int gv_time_frames(gv_handle h, int32_t frames, float *ms_total)
{
  if (!h || frames <= 0 || !ms_total) return GV_ERR_BAD_ARG;
  GV_TRY
  int rc = use_device(h);
  if (rc) return rc;
  hipEvent_t e0 = h->ev[0], e1 = h->ev[kNumStages];
  GV_HIP(hipEventRecord(e0, h->stream));
  for (int32_t i = 0; i < frames; ++i)
    if ((rc = gv_frame_enqueue(h))) return rc;
  if ((rc = gv_frame_fence(h))) return rc;
  GV_HIP(hipEventRecord(e1, h->stream));
  GV_HIP(hipEventSynchronize(e1));
  GV_HIP(hipEventElapsedTime(ms_total, e0, e1));
  return GV_OK;
  GV_CATCH
}

int gv_time_frame_stages(gv_handle h, int32_t frames, float *stage_ms)
{
  if (!h || frames <= 0 || !stage_ms) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!h->det[h->det_cur].valid) return GV_ERR_STATE;
  int rc = use_device(h);
  if (rc) return rc;
  for (int s = 0; s < kNumStages; ++s) stage_ms[s] = 0.0f;
  for (int32_t i = 0; i < frames; ++i) {
    if ((rc = sector_path(h) ? enqueue_frame_tiles(h, false, true) : enqueue_frame_generic(h, true))) return rc;
    GV_HIP(hipEventSynchronize(h->ev[kNumStages]));
    for (int s = 0; s < kNumStages; ++s) {
      float ms = 0.0f;
      // tile path: the four kernels report their own start / end (dispatch-packet timestamps, the figure
      // rocprofv3 shows); everything else is the interval between two event records on the stream
      const int kq = s - kStagePoints;   // points, tile pass ("ray ends"), sectors, grid pass
      if (sector_path(h) && kq >= 0 && kq < 4) {
        if (h->kt_used[kq]) GV_HIP(hipEventElapsedTime(&ms, h->kt[kq][0], h->kt[kq][1]));
      } else {
        GV_HIP(hipEventElapsedTime(&ms, h->ev[s], h->ev[s + 1]));
      }
      stage_ms[s] += ms;
    }
  }
  for (int s = 0; s < kNumStages; ++s) stage_ms[s] /= (float)frames;
  return GV_OK;
  GV_CATCH
}

}  // extern "C"
