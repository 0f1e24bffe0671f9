// gv_api_shard.hip -- the frame sharded by points over several GPUs (RCCL), gv_comm_*, gv_*_sharded*, gv_shard_*,
// and the one-device emulation hook of the tests.
#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "gv_context.hpp"

namespace {

// --- the frame sharded by points (BASELINE configs[4]) ---
// Every rank bins ITS slice of the cloud into private end bitmaps.  Two exchanges follow, both of the
// form "all-to-all of equal slices + local OR" (RCCL has no bitwise-OR reduction; the slices are bitmap
// words, 32 cells per word):
//   1. ray ends: the OR-ed slices are all-gathered, so every rank holds the complete end bitmaps and
//      runs only every world-th workgroup of the sector ray stage (the dispatch order is sorted by
//      expected cost, so the shares are balanced);
//   2. free cells: each rank's partial free-cell bitmaps are packed by row band and rank q receives
//      and ORs band q.
// Rank q then runs the grid pass on band q (whole 64-row blocks) and the packed int8 bands are
// broadcast.  OR and integer sums commute: the result is bit-identical to one GPU.
// The exchanges are expressed over `ShardLink`, which is RCCL in production and a set of device
// copies in the one-device emulation that the tests use to run every (rank, world).
struct ShardLink {
  gv_context *h;
  int rank, world;
  // emulation: the `world` per-rank source buffers of the current exchange (null with RCCL)
  const DevBuf<uint32_t> *emu_src = nullptr;
};

// recv[q'] (count words each) <- slice `rank` of peer q'; send holds `world` slices of count words
int shard_all_to_all(const ShardLink &L, const uint32_t *send, uint32_t *recv, size_t count, hipStream_t s)
{
  gv_context *h = L.h;
  if (L.emu_src) {
    for (int q = 0; q < L.world; ++q)
      GV_HIP(hipMemcpyAsync(recv + (size_t)q * count, L.emu_src[q] + (size_t)L.rank * count, count * sizeof(uint32_t),
                            hipMemcpyDeviceToDevice, s));
    return GV_OK;
  }
  ncclResult_t first_err = ncclGroupStart();
  for (int q = 0; q < L.world && first_err == ncclSuccess; ++q) {
    if (q == L.rank) continue;
    ncclResult_t r = ncclSend(send + (size_t)q * count, count, ncclUint32, q, h->comm, s);
    if (r == ncclSuccess) r = ncclRecv(recv + (size_t)q * count, count, ncclUint32, q, h->comm, s);
    if (r != ncclSuccess) first_err = r;
  }
  const ncclResult_t ge = ncclGroupEnd();   // always closed, also on the error path
  if (first_err == ncclSuccess) first_err = ge;
  if (first_err != ncclSuccess) {
    h->err = std::string("sharded all-to-all -> ") + ncclGetErrorString(first_err);
    return GV_ERR_RCCL;
  }
  GV_HIP(hipMemcpyAsync(recv + (size_t)L.rank * count, send + (size_t)L.rank * count, count * sizeof(uint32_t),
                        hipMemcpyDeviceToDevice, s));
  return GV_OK;
}

size_t shard_ends_slice(const gv_context *h, int world)
{
  return (size_t)gv_shard_slice_words((int64_t)h->ends_words, world);
}

int ensure_shard_scratch(gv_context *h, int world)
{
  const size_t chunk = free_band_chunk_words(h->nxw, h->nx_pad, h->ny_pad, world);
  const size_t need = std::max(shard_ends_slice(h, world) * (size_t)world, 2 * chunk * (size_t)world) + 16;
  return h->sh_xchg.reserve(h, need);
}

// exchange 1 (this rank's part): OR of everyone's slice `rank` of the end bitmaps, written back in place
int shard_or_ends_slice(const ShardLink &L, uint32_t *ends, hipStream_t s)
{
  gv_context *h = L.h;
  const size_t slice = shard_ends_slice(h, L.world);
  int rc = shard_all_to_all(L, ends, h->sh_xchg, slice, s);
  if (rc) return rc;
  launch_or_slices(h->sh_xchg, ends + (size_t)L.rank * slice, slice, L.world, s);
  GV_HIP(hipGetLastError());
  return GV_OK;
}

// exchange 2 (this rank's part): band `rank` of everyone's free-cell bitmaps OR-ed into set p
int shard_or_free_band(const ShardLink &L, int p, const uint32_t *packed, hipStream_t s)
{
  gv_context *h = L.h;
  const size_t chunk = free_band_chunk_words(h->nxw, h->nx_pad, h->ny_pad, L.world);
  uint32_t *recv = h->sh_xchg + chunk * (size_t)L.world;
  int rc = shard_all_to_all(L, packed, recv, chunk, s);
  if (rc) return rc;
  launch_unpack_free_band(recv, L.world, chunk, L.rank, h->nxw, h->nx_pad, h->ny_pad, h->fs[p].freeN, h->fs[p].freeT, s);
  GV_HIP(hipGetLastError());
  return GV_OK;
}

// The asynchronous sharded frame.  Three queues work on it: the frame's lane (binning, this rank's share of the
// sector stage, band packing), the exchange stream X (RCCL: ends exchange, free-band exchange, band broadcast,
// count reduce) and the public stream (the band's grid pass -- grid passes stay one in-order sequence).  Events
// chain the steps of ONE frame; nothing orders frame f + 1's binning (the other lane) behind frame f's
// exchanges, so they overlap.  RCCL calls are issued on X in the same order on every rank (x1, x2, x3 of frame
// f, then of f + 1).  te (optional, 7 timing events): start, binning, x1, sectors, x2, grid pass, x3 done.
int enqueue_frame_sharded(gv_context *h, const Event *te)
{
  DetSet &D = h->det[h->det_cur];
  const uint32_t fl = D.flags;
  const bool do_bin = fl & GV_FRAME_BIN, do_ray = fl & GV_FRAME_RAYMARCH, do_bbox = fl & GV_FRAME_BBOX_TEST;
  const bool keep_cell = fl & GV_FRAME_KEEP_CELL_IDX, keep_counts = fl & GV_FRAME_KEEP_COUNTS;
  int rc = check_frame_flags(h, fl);
  if (rc) return rc;
  if (!do_bin || !h->comm || !h->stream_x) return GV_ERR_STATE;
  // Its own rotation, not enqueue_frame_tiles': always lanes 0 / 1 and buffer sets 1..4, whatever GV_LANES says and
  // however long the upload stream has been quiet.  The third lane is the upload stream (gv_context::lanes_now), which
  // this form leaves to the uploads, and its back-pressure is four frames deep.
  const int p = 1 + (int)(h->lane_frames % 4u);
  const int k = 1 + (int)(h->lane_frames % 2u);
  hipStream_t s = h->streams[k], X = h->stream_x;
  h->sb[1].lane_clean = h->sb[2].lane_clean = false;   // events between the steps: every kernel of this form keeps its barrier bit
  if (h->fs[p].fin_slot >= 0) GV_HIP(hipEventSynchronize(h->ev_fin[h->fs[p].fin_slot]));   // back-pressure: four frames in flight
  CloudSet &CS = h->cloud[h->cloud_cur];
  if ((rc = wait_inputs(h, CS, D, k))) return rc;
  if ((rc = ensure_shard_scratch(h, h->world))) return rc;
  const int slot = (int)(h->frame_no % (uint64_t)gv_context::kRing);
  const Event *ev = h->ev_sh[slot];
  // Step x3 of a KEEP_COUNTS frame reduces sb[k].hits IN PLACE on the exchange stream, and nothing else orders this
  // lane's next tile pass -- which rewrites every cell of sb[k].hits -- behind it (the buffer-set back-pressure is
  // four frames deep, the lane comes round every second frame).  The lane waits for that frame's last exchange
  // (round-3 advisor finding; test_sharded_keep_counts_frames_in_flight).
  if (h->sb[k].sh_counts_slot >= 0) {
    GV_HIP(hipStreamWaitEvent(s, h->ev_fin[h->sb[k].sh_counts_slot], 0));
    h->sb[k].sh_counts_slot = -1;
  }
  if (te) GV_HIP(hipEventRecord(te[0], s));
  // --- lane: rectangles + binning of this rank's points into private end bitmaps
  Rect *rects = h->fs[p].rects;
  const bool fold_rects = !(fl & GV_FRAME_VISION_ORIENT) && D.n_poses > 0;
  const int32_t n_rects = fold_rects ? D.n_poses : enqueue_rects(h, D, rects, h->sb[k].vout, s);
  if ((rc = enqueue_binning(h, D, p, k, 0, h->n, keep_cell, do_ray, do_bbox, keep_counts, nullptr, fold_rects ? rects : nullptr)))
    return rc;
  if (te) GV_HIP(hipEventRecord(te[1], s));
  GV_HIP(hipEventRecord(ev[0], s));
  // --- X: complete end bitmaps everywhere (slices all-to-all + OR, then all-gather)
  ShardLink L{h, h->rank, h->world};
  const size_t slice = shard_ends_slice(h, h->world);
  GV_HIP(hipStreamWaitEvent(X, ev[0], 0));
  if ((rc = shard_or_ends_slice(L, h->fs[p].ends, X))) return rc;
  GV_NCCL(ncclAllGather(h->fs[p].ends + (size_t)h->rank * slice, h->fs[p].ends, slice, ncclUint32, h->comm, X));
  if (te) GV_HIP(hipEventRecord(te[2], X));
  GV_HIP(hipEventRecord(ev[1], X));
  // --- lane: this rank's share of the ray stage, its free cells packed by band
  GV_HIP(hipStreamWaitEvent(s, ev[1], 0));
  if (do_ray && (rc = enqueue_sectors(h, p, h->rank, h->world, s))) return rc;
  const size_t chunk = free_band_chunk_words(h->nxw, h->nx_pad, h->ny_pad, h->world);
  launch_pack_free_bands(h->fs[p].freeN, h->fs[p].freeT, h->nxw, h->nx_pad, h->ny_pad, h->world, chunk, h->sh_xchg, s);
  GV_HIP(hipGetLastError());
  if (te) GV_HIP(hipEventRecord(te[3], s));
  GV_HIP(hipEventRecord(ev[2], s));
  // --- X: the free cells of MY band from everyone
  GV_HIP(hipStreamWaitEvent(X, ev[2], 0));
  if ((rc = shard_or_free_band(L, p, h->sh_xchg, X))) return rc;
  if (te) GV_HIP(hipEventRecord(te[4], X));
  GV_HIP(hipEventRecord(ev[3], X));
  // --- public stream: grid pass on the band (whole 64-row blocks)
  int32_t y0, y1;
  shard_band_rows(h->rank, h->world, h->g.ny, h->ny_pad, y0, y1);
  GV_HIP(hipStreamWaitEvent(h->stream, ev[3], 0));
  if ((rc = enqueue_grid_pass(h, p, rects, n_rects, true, y0, y1, h->stream, nullptr, nullptr, nullptr, true))) return rc;
  if (te) GV_HIP(hipEventRecord(te[5], h->stream));
  GV_HIP(hipEventRecord(ev[4], h->stream));
  // --- X: packed bands to everyone (band r sits at data[G - e_r, G - b_r)); band totals of the hit counts
  GV_HIP(hipStreamWaitEvent(X, ev[4], 0));
  const size_t G = (size_t)h->g.G;
  ncclResult_t first_err = ncclGroupStart();
  for (int r = 0; r < h->world && first_err == ncclSuccess; ++r) {
    int32_t r0, r1;
    shard_band_rows(r, h->world, h->g.ny, h->ny_pad, r0, r1);
    const size_t b = (size_t)r0 * h->g.nx, e = (size_t)r1 * h->g.nx;
    if (e > b) {
      const ncclResult_t br = ncclBroadcast(h->occ_i8 + (G - e), h->occ_i8 + (G - e), e - b, ncclInt8, r, h->comm, X);
      if (br != ncclSuccess) first_err = br;
    }
  }
  ncclResult_t ge = ncclGroupEnd();   // always closed, also on the error path
  if (first_err == ncclSuccess) first_err = ge;
  if (first_err == ncclSuccess && keep_counts) {
    // reduce-scatter by band -- rank q ends with the summed counts of band q (in place, at the
    // band's rows of its hits[]; the other rows keep this rank's partial counts).  Bands are whole 64-row blocks
    // and may differ in length: equal bands are one ncclReduceScatter, otherwise one grouped ncclReduce per band.
    int32_t *hk = h->sb[k].hits;
    bool equal = true;
    size_t cnt0 = 0;
    for (int r = 0; r < h->world; ++r) {
      int32_t r0, r1;
      shard_band_rows(r, h->world, h->g.ny, h->ny_pad, r0, r1);
      const size_t c = (size_t)(r1 - r0) * h->g.nx;
      if (r == 0) cnt0 = c;
      equal = equal && c == cnt0 && (size_t)r0 * h->g.nx == (size_t)r * cnt0;
    }
    if (equal && cnt0) {
      first_err = ncclReduceScatter(hk, hk + (size_t)h->rank * cnt0, cnt0, ncclInt32, ncclSum, h->comm, X);
    } else {
      first_err = ncclGroupStart();
      for (int r = 0; r < h->world && first_err == ncclSuccess; ++r) {
        int32_t r0, r1;
        shard_band_rows(r, h->world, h->g.ny, h->ny_pad, r0, r1);
        const size_t b = (size_t)r0 * h->g.nx, e = (size_t)r1 * h->g.nx;
        if (e > b) first_err = ncclReduce(hk + b, hk + b, e - b, ncclInt32, ncclSum, r, h->comm, X);
      }
      ge = ncclGroupEnd();
      if (first_err == ncclSuccess) first_err = ge;
    }
  }
  if (first_err != ncclSuccess) {
    h->err = std::string("sharded band exchange -> ") + ncclGetErrorString(first_err);
    return GV_ERR_RCCL;
  }
  if (te) GV_HIP(hipEventRecord(te[6], X));
  GV_HIP(hipEventRecord(h->ev_fin[slot], X));
  // what the frame produced (the gathered packed grid) is visible on the public stream right behind it
  GV_HIP(hipStreamWaitEvent(h->stream, h->ev_fin[slot], 0));
  // D counts as read on the lane and on the public stream; a sharded frame never runs on the third lane and does not
  // count towards the quiet frames that open it
  note_frame_readers(h, slot, p, CS, D, (1u << k) | 1u, true, false);
  if (keep_counts) h->sb[k].sh_counts_slot = slot;
  // hits: band totals at this rank's band rows (gv_comm_band), only when kept (the tile pass writes hits[] only then);
  // miss: never, the free-cell bitmaps are complete for this rank's band only
  set_last_frame(h, p, k, k, keep_counts, false, keep_cell, do_bbox);
  return GV_OK;
}

}  // namespace

namespace gv_internal __attribute__((visibility("hidden"))) {

void comm_destroy(gv_context *h)
{
  if (h->comm) { ncclCommDestroy(h->comm); h->comm = nullptr; }
}

}  // namespace gv_internal

extern "C" {

int gv_comm_unique_id(uint8_t id_out[128])
{
  if (!id_out) return GV_ERR_BAD_ARG;
  static_assert(sizeof(ncclUniqueId) == 128, "RCCL unique id size");
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return GV_ERR_RCCL;
  std::memcpy(id_out, &id, sizeof(id));
  return GV_OK;
}

int gv_comm_init(gv_handle h, const uint8_t id[128], int32_t rank, int32_t world)
{
  if (!h || !id || world < 1 || rank < 0 || rank >= world) return GV_ERR_BAD_ARG;
  if (h->comm) return GV_ERR_STATE;
  GV_TRY
  int rc = use_device(h);
  if (rc) return rc;
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof(uid));
  GV_NCCL(ncclCommInitRank(&h->comm, world, uid, rank));
  h->rank = rank;
  h->world = world;
  h->layers_in_step = false;   // the bands change hands: the next grid pass writes every row it owns
  // the exchange stream of the sharded frame and the events that chain its steps (ordering only)
  if (!h->stream_x) GV_HIP(h->stream_x.create());
  for (auto &row : h->ev_sh)
    for (auto &e : row)
      if (!e) GV_HIP(e.create(hipEventDisableTiming));
  for (auto &e : h->sh_t)
    if (!e) GV_HIP(e.create(hipEventDefault));   // timing events
  return GV_OK;
  GV_CATCH
}

int gv_comm_info(gv_handle h, int32_t *n_ranks, int32_t *rank, int32_t *device)
{
  if (!h) return GV_ERR_BAD_ARG;
  if (!h->comm) return GV_ERR_STATE;
  int nr = 0, rk = 0, dev = 0;
  GV_NCCL(ncclCommCount(h->comm, &nr));
  GV_NCCL(ncclCommUserRank(h->comm, &rk));
  GV_NCCL(ncclCommCuDevice(h->comm, &dev));
  if (n_ranks) *n_ranks = nr;
  if (rank) *rank = rk;
  if (device) *device = dev;
  return GV_OK;
}

int gv_comm_destroy(gv_handle h)
{
  if (!h) return GV_ERR_BAD_ARG;
  if (!h->comm) return GV_OK;
  (void)hipSetDevice(h->device);
  (void)drain(h);
  comm_destroy(h);
  h->rank = 0;
  h->world = 1;
  h->layers_in_step = false;
  return GV_OK;
}

int gv_frame_enqueue_sharded(gv_handle h)
{
  if (!h) return GV_ERR_BAD_ARG;
  if (!h->comm || !sector_path(h)) return GV_ERR_STATE;
  GV_TRY
  if (!h->det[h->det_cur].valid) return GV_ERR_STATE;   // no gv_frame_set_detections yet
  int rc = set_device_only(h);
  if (rc) return rc;
  return enqueue_frame_sharded(h, nullptr);
  GV_CATCH
}

int gv_process_frame_sharded(gv_handle h, const gv_frame_desc *desc)
{
  if (!h || !desc) return GV_ERR_BAD_ARG;
  if (!h->comm) return GV_ERR_STATE;
  if (!sector_path(h)) return GV_ERR_STATE;
  int rc = gv_frame_set_detections(h, desc);
  if (rc) return rc;
  if ((rc = gv_frame_enqueue_sharded(h))) return rc;
  return gv_synchronize(h);
}

int gv_time_frame_sharded_stages(gv_handle h, int32_t frames, float stage_ms[6])
{
  if (!h || frames <= 0 || !stage_ms) return GV_ERR_BAD_ARG;
  if (!h->comm || !sector_path(h)) return GV_ERR_STATE;
  GV_TRY
  if (!h->det[h->det_cur].valid) return GV_ERR_STATE;
  int rc = use_device(h);
  if (rc) return rc;
  for (int s = 0; s < 6; ++s) stage_ms[s] = 0.0f;
  for (int32_t i = 0; i < frames; ++i) {   // one frame at a time: every step alone on the device
    if ((rc = enqueue_frame_sharded(h, h->sh_t))) return rc;
    if ((rc = drain(h))) return rc;
    for (int s = 0; s < 6; ++s) {
      float ms = 0.0f;
      GV_HIP(hipEventElapsedTime(&ms, h->sh_t[s], h->sh_t[s + 1]));
      stage_ms[s] += ms;
    }
  }
  for (int s = 0; s < 6; ++s) stage_ms[s] /= (float)frames;
  return GV_OK;
  GV_CATCH
}

int gv_shard_band_rows(int32_t rank, int32_t world, int32_t ny, int32_t *y0, int32_t *y1)
{
  if (world < 1 || rank < 0 || rank >= world || ny < 1 || !y0 || !y1) return GV_ERR_BAD_ARG;
  const int ny_pad = kBinTile * ((ny + kBinTile - 1) / kBinTile);
  shard_band_rows(rank, world, ny, ny_pad, *y0, *y1);
  return GV_OK;
}

int64_t gv_shard_slice_words(int64_t words, int32_t world)
{
  if (words < 0 || world < 1) return -1;
  return (int64_t)(((((size_t)words + (size_t)world - 1) / (size_t)world) + 3) & ~(size_t)3);
}

// the body of gv_test_frame_sharded_emulated; the caller owns the temporaries and waits for the stream
static int emulate_ranks(gv_context *h, DetSet &D, int32_t world, DevBuf<uint32_t> *ends, DevBuf<uint32_t> *packs,
                         DevBuf<uint32_t> &comb)
{
  const uint32_t fl = D.flags;
  const bool do_ray = fl & GV_FRAME_RAYMARCH, do_bbox = fl & GV_FRAME_BBOX_TEST, keep_cell = fl & GV_FRAME_KEEP_CELL_IDX;
  hipStream_t s = h->stream;
  const size_t slice = shard_ends_slice(h, world), Ep = slice * (size_t)world;
  const size_t chunk = free_band_chunk_words(h->nxw, h->nx_pad, h->ny_pad, world);
  int rc2;
  if ((rc2 = comb.reserve(h, Ep))) return rc2;
  for (int r = 0; r < world; ++r)
    if ((rc2 = ends[r].reserve(h, Ep)) || (rc2 = packs[r].reserve(h, chunk * (size_t)world))) return rc2;
  Rect *rects = h->fs[0].rects;
  if ((rc2 = wait_inputs(h, h->cloud[h->cloud_cur], D, 0))) return rc2;
  const int32_t n_rects = enqueue_rects(h, D, rects, h->sb[0].vout, s);
  for (int r = 0; r < world; ++r) {   // every rank bins its slice
    const size_t lo = h->n * (size_t)r / (size_t)world, hi = h->n * (size_t)(r + 1) / (size_t)world;
    if ((rc2 = enqueue_binning(h, D, 0, 0, lo, hi - lo, keep_cell, do_ray, do_bbox, false, nullptr))) return rc2;
    GV_HIP(hipMemcpyAsync(ends[r], h->fs[0].ends, Ep * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  }
  for (int q = 0; q < world; ++q) {   // exchange 1: rank q ORs slice q; the all-gather is the union of the slices
    ShardLink L{h, q, world, ends};
    if ((rc2 = shard_or_ends_slice(L, comb, s))) return rc2;
  }
  GV_HIP(hipMemcpyAsync(h->fs[0].ends, comb, Ep * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  for (int r = 0; r < world; ++r) {   // every rank's share of the ray stage, packed by band
    GV_HIP(hipMemsetAsync(h->fs[0].free_, 0, (h->bmN_words + h->bmT_words) * sizeof(uint32_t), s));
    if (do_ray && (rc2 = enqueue_sectors(h, 0, r, world, s))) return rc2;
    launch_pack_free_bands(h->fs[0].freeN, h->fs[0].freeT, h->nxw, h->nx_pad, h->ny_pad, world, chunk, packs[r], s);
    GV_HIP(hipGetLastError());
  }
  for (int q = 0; q < world; ++q) {   // exchange 2 + grid pass of band q
    ShardLink L{h, q, world, packs};
    if ((rc2 = shard_or_free_band(L, 0, nullptr, s))) return rc2;
    int32_t y0, y1;
    shard_band_rows(q, world, h->g.ny, h->ny_pad, y0, y1);
    if ((rc2 = enqueue_grid_pass(h, 0, rects, n_rects, true, y0, y1, s, nullptr, nullptr, nullptr, true))) return rc2;
  }
  GV_HIP(hipStreamSynchronize(s));
  return GV_OK;
}

// Test hook: the sharded frame for every rank of a `world`-GPU job, run on THIS device with the RCCL
// exchanges replaced by device copies (ShardLink emulation).  The resident cloud is the whole cloud;
// rank r takes points [n*r/world, n*(r+1)/world).  Every piece the ranks would run -- binning of a
// slice, OR of the end-bitmap slices, every world-th sector workgroup, band packing, band OR, band grid
// pass -- runs with its real (rank, world); the bands land in the one resident grid.
int gv_test_frame_sharded_emulated(gv_handle h, const gv_frame_desc *desc, int32_t world)
{
  if (!h || !desc || world < 1 || world > 16) return GV_ERR_BAD_ARG;
  if (!sector_path(h)) return GV_ERR_STATE;
  int rc = gv_frame_set_detections(h, desc);
  if (rc) return rc;
  GV_TRY
  if ((rc = use_device(h))) return rc;
  DetSet &D = h->det[h->det_cur];
  const uint32_t fl = D.flags;
  const bool do_bbox = fl & GV_FRAME_BBOX_TEST, keep_cell = fl & GV_FRAME_KEEP_CELL_IDX;
  if ((rc = check_frame_flags(h, fl))) return rc;
  if (!(fl & GV_FRAME_BIN)) return GV_ERR_STATE;
  if ((rc = ensure_shard_scratch(h, world))) return rc;
  if ((rc = ensure_point_buffers(h, h->n, (h->n + (size_t)world - 1) / (size_t)world))) return rc;
  // every rank's end bitmaps and packed free bands, and the combined end bitmaps: gone with this call
  std::vector<DevBuf<uint32_t>> ends((size_t)world), packs((size_t)world);
  DevBuf<uint32_t> comb;
  rc = emulate_ranks(h, D, world, ends.data(), packs.data(), comb);
  (void)hipStreamSynchronize(h->stream);   // on every way out, before the temporaries go
  // no whole count grid (the slices are binned without hits[]) and, as on a rank of the sharded frame, no miss grid
  set_last_frame(h, 0, 0, 0, false, false, keep_cell, do_bbox);
  return rc;
  GV_CATCH
}

int gv_comm_band(gv_handle h, int64_t *begin, int64_t *end)
{
  if (!h) return GV_ERR_BAD_ARG;
  int32_t y0, y1;
  shard_band_rows(h->rank, h->world, h->g.ny, h->ny_pad, y0, y1);
  if (begin) *begin = (int64_t)y0 * h->g.nx;
  if (end) *end = (int64_t)y1 * h->g.nx;
  return GV_OK;
}

}  // extern "C"
