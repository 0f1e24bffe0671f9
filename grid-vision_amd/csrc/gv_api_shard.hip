// gv_api_shard.hip -- the frame sharded by points over several GPUs (RCCL), gv_comm_*, gv_*_sharded*, gv_shard_*,
// and the one-device emulation hook of the tests.  Who owns which rows and how large the exchanges are: host::ShardPlan
// (gv_host_math.hpp); the communicator, its plan, the exchange stream, scratch and events: gv_context::Shard (h->sh).
#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <string>
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
  int rank;
  const host::ShardPlan &plan;   // bands, slice and chunk of this link's `world`
  // emulation: the `world` per-rank source buffers of the current exchange (null with RCCL)
  const DevBuf<uint32_t> *emu_src = nullptr;
};

// GV_OK, or GV_ERR_RCCL with h->err = the caller's label + what RCCL says
int nccl_failed(gv_context *h, const char *label, ncclResult_t r)
{
  if (r == ncclSuccess) return GV_OK;
  h->err = std::string(label) + ncclGetErrorString(r);
  return GV_ERR_RCCL;
}
// One RCCL group: item(r) for r = 0 .. world - 1 between ncclGroupStart and ncclGroupEnd.  The first error ends the
// loop and is the one reported; the group is always closed, also on the error path.
template <class Item>
int nccl_group(gv_context *h, const char *label, int world, Item item)
{
  ncclResult_t first_err = ncclGroupStart();
  for (int r = 0; r < world && first_err == ncclSuccess; ++r) first_err = item(r);
  const ncclResult_t ge = ncclGroupEnd();
  return nccl_failed(h, label, first_err == ncclSuccess ? ge : first_err);
}

// recv[q'] (count words each) <- slice `rank` of peer q'; send holds `world` slices of count words
int shard_all_to_all(const ShardLink &L, const uint32_t *send, uint32_t *recv, size_t count, hipStream_t s)
{
  gv_context *h = L.h;
  if (L.emu_src) {
    for (int q = 0; q < L.plan.world; ++q)
      GV_HIP(hipMemcpyAsync(recv + (size_t)q * count, L.emu_src[q] + (size_t)L.rank * count, count * sizeof(uint32_t),
                            hipMemcpyDeviceToDevice, s));
    return GV_OK;
  }
  ncclComm *comm = h->sh.comm;
  int rc = nccl_group(h, "sharded all-to-all -> ", L.plan.world, [&](int q) {
    if (q == L.rank) return ncclSuccess;
    const ncclResult_t r = ncclSend(send + (size_t)q * count, count, ncclUint32, q, comm, s);
    return r == ncclSuccess ? ncclRecv(recv + (size_t)q * count, count, ncclUint32, q, comm, s) : r;
  });
  if (rc) return rc;
  GV_HIP(hipMemcpyAsync(recv + (size_t)L.rank * count, send + (size_t)L.rank * count, count * sizeof(uint32_t),
                        hipMemcpyDeviceToDevice, s));
  return GV_OK;
}

// exchange 1 (this rank's part): OR of everyone's slice `rank` of the end bitmaps, written back in place
int shard_or_ends_slice(const ShardLink &L, uint32_t *ends, hipStream_t s)
{
  gv_context *h = L.h;
  const size_t slice = L.plan.slice;
  int rc = shard_all_to_all(L, ends, h->sh.xchg, slice, s);
  if (rc) return rc;
  launch_or_slices(h->sh.xchg, ends + (size_t)L.rank * slice, slice, L.plan.world, s);
  GV_HIP(hipGetLastError());
  return GV_OK;
}

// exchange 2 (this rank's part): band `rank` of everyone's free-cell bitmaps OR-ed into set p
int shard_or_free_band(const ShardLink &L, int p, const uint32_t *packed, hipStream_t s)
{
  gv_context *h = L.h;
  uint32_t *recv = h->sh.xchg + L.plan.chunk * (size_t)L.plan.world;
  int rc = shard_all_to_all(L, packed, recv, L.plan.chunk, s);
  if (rc) return rc;
  launch_unpack_free_band(recv, L.plan, L.rank, h->fs[p].freeN, h->fs[p].freeT, s);
  GV_HIP(hipGetLastError());
  return GV_OK;
}

// The two steps between and behind the exchanges, as the product frame and its emulation both run them.
// `rank`'s share of the ray stage over the complete end bitmaps of set p, its free cells packed by band into `packed`
int shard_rays_and_pack(const ShardLink &L, int p, bool do_ray, uint32_t *packed, hipStream_t s)
{
  gv_context *h = L.h;
  SectorsJob sec;
  sec.set = p; sec.stream = s;
  sec.first = L.rank; sec.stride = L.plan.world;
  int rc;
  if (do_ray && (rc = enqueue_sectors(h, sec))) return rc;
  launch_pack_free_bands(h->fs[p].freeN, h->fs[p].freeT, L.plan, packed, s);
  GV_HIP(hipGetLastError());
  return GV_OK;
}

// the grid pass on band `rank` (whole 64-row blocks) with the bitmaps of set p
int shard_band_grid_pass(const ShardLink &L, int p, const Rect *rects, int32_t n_rects, hipStream_t s)
{
  GridPassJob grid;
  grid.set = p; grid.stream = s;
  grid.rects = rects; grid.n_rects = n_rects;
  grid.counts = grid.sharded = true;
  grid.y0 = L.plan.bands[(size_t)L.rank].y0; grid.y1 = L.plan.bands[(size_t)L.rank].y1;
  return enqueue_grid_pass(L.h, grid);
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
  gv_context::Shard &S = h->sh;
  const FrameFlags f = frame_flags(D.flags);
  int rc = check_frame_flags(h, D.flags);
  if (rc) return rc;
  if (!f.bin || !S.active() || !S.stream_x) return GV_ERR_STATE;
  // Its own rotation, not enqueue_frame_tiles': always lanes 0 / 1 and buffer sets 1..4, whatever GV_LANES says and
  // however long the upload stream has been quiet.  The third lane is the upload stream (gv_context::lanes_now), which
  // this form leaves to the uploads, and its back-pressure is four frames deep.
  const int p = 1 + (int)(h->lane_frames % 4u);
  const int k = 1 + (int)(h->lane_frames % 2u);
  hipStream_t s = h->streams[k], X = S.stream_x;
  h->sb[1].lane_clean = h->sb[2].lane_clean = false;   // events between the steps: every kernel of this form keeps its barrier bit
  if (h->fs[p].fin_slot >= 0) GV_HIP(hipEventSynchronize(h->ev_fin[h->fs[p].fin_slot]));   // back-pressure: four frames in flight
  CloudSet &CS = h->cloud[h->cloud_cur];
  if ((rc = wait_inputs(h, CS, D, k))) return rc;
  if ((rc = S.xchg.reserve(h, S.plan.scratch_words()))) return rc;
  const int slot = (int)(h->frame_no % (uint64_t)gv_context::kRing);
  const Event *ev = S.ev[slot];
  // Step x3 of a KEEP_COUNTS frame reduces sb[k].hits IN PLACE on the exchange stream, and nothing else orders this
  // lane's next tile pass -- which rewrites every cell of sb[k].hits -- behind it (the buffer-set back-pressure is
  // four frames deep, the lane comes round every second frame).  The lane waits for that frame's last exchange
  // (round-3 advisor finding; test_sharded_keep_counts_frames_in_flight).
  if (S.counts_slot[k] >= 0) {
    GV_HIP(hipStreamWaitEvent(s, h->ev_fin[S.counts_slot[k]], 0));
    S.counts_slot[k] = -1;
  }
  if (te) GV_HIP(hipEventRecord(te[0], s));
  // --- lane: rectangles + binning of this rank's points into private end bitmaps
  Rect *rects = h->fs[p].rects;
  const bool fold_rects = !f.vision && D.n_poses > 0;
  const int32_t n_rects = fold_rects ? D.n_poses : enqueue_rects(h, D, rects, h->sb[k].vout, s);
  BinningJob bin{D};
  bin.set = p; bin.stream = k;
  bin.n = h->n;
  bin.keep_cell = f.keep_cell; bin.do_ray = f.ray; bin.do_bbox = f.bbox;
  bin.write_hits = f.keep_counts;
  bin.fold_rects = fold_rects ? rects : nullptr;
  if ((rc = enqueue_binning(h, bin))) return rc;
  if (te) GV_HIP(hipEventRecord(te[1], s));
  GV_HIP(hipEventRecord(ev[0], s));
  // --- X: complete end bitmaps everywhere (slices all-to-all + OR, then all-gather)
  const ShardLink L{h, S.rank, S.plan};
  uint32_t *ends = h->fs[p].ends;
  GV_HIP(hipStreamWaitEvent(X, ev[0], 0));
  if ((rc = shard_or_ends_slice(L, ends, X))) return rc;
  GV_NCCL(ncclAllGather(ends + (size_t)S.rank * S.plan.slice, ends, S.plan.slice, ncclUint32, S.comm, X));
  if (te) GV_HIP(hipEventRecord(te[2], X));
  GV_HIP(hipEventRecord(ev[1], X));
  // --- lane: this rank's share of the ray stage, its free cells packed by band
  GV_HIP(hipStreamWaitEvent(s, ev[1], 0));
  if ((rc = shard_rays_and_pack(L, p, f.ray, S.xchg, s))) return rc;
  if (te) GV_HIP(hipEventRecord(te[3], s));
  GV_HIP(hipEventRecord(ev[2], s));
  // --- X: the free cells of MY band from everyone
  GV_HIP(hipStreamWaitEvent(X, ev[2], 0));
  if ((rc = shard_or_free_band(L, p, S.xchg, X))) return rc;
  if (te) GV_HIP(hipEventRecord(te[4], X));
  GV_HIP(hipEventRecord(ev[3], X));
  // --- public stream: grid pass on the band
  GV_HIP(hipStreamWaitEvent(h->stream, ev[3], 0));
  if ((rc = shard_band_grid_pass(L, p, rects, n_rects, h->stream))) return rc;
  if (te) GV_HIP(hipEventRecord(te[5], h->stream));
  GV_HIP(hipEventRecord(ev[4], h->stream));
  // --- X: packed bands to everyone (band r sits at data[G - e_r, G - b_r)); band totals of the hit counts
  GV_HIP(hipStreamWaitEvent(X, ev[4], 0));
  const char *const x3 = "sharded band exchange -> ";
  const std::vector<host::ShardPlan::Band> &bands = S.plan.bands;
  int8_t *const top = h->occ_i8 + (size_t)h->g.G;
  if ((rc = nccl_group(h, x3, S.world, [&](int r) {
         const host::ShardPlan::Band &B = bands[(size_t)r];
         return B.e > B.b ? ncclBroadcast(top - B.e, top - B.e, B.e - B.b, ncclInt8, r, S.comm, X) : ncclSuccess;
       })))
    return rc;
  if (f.keep_counts) {
    // reduce-scatter by band -- rank q ends with the summed counts of band q (in place, at the
    // band's rows of its hits[]; the other rows keep this rank's partial counts).  Bands are whole 64-row blocks
    // and may differ in length: equal bands are one ncclReduceScatter, otherwise one grouped ncclReduce per band.
    int32_t *hk = h->sb[k].hits;
    if (S.plan.equal_bands) {
      const size_t cnt0 = S.plan.cnt0;
      rc = nccl_failed(h, x3, ncclReduceScatter(hk, hk + (size_t)S.rank * cnt0, cnt0, ncclInt32, ncclSum, S.comm, X));
    } else {
      rc = nccl_group(h, x3, S.world, [&](int r) {
        const host::ShardPlan::Band &B = bands[(size_t)r];
        return B.e > B.b ? ncclReduce(hk + B.b, hk + B.b, B.e - B.b, ncclInt32, ncclSum, r, S.comm, X) : ncclSuccess;
      });
    }
    if (rc) return rc;
  }
  if (te) GV_HIP(hipEventRecord(te[6], X));
  GV_HIP(hipEventRecord(h->ev_fin[slot], X));
  // what the frame produced (the gathered packed grid) is visible on the public stream right behind it
  GV_HIP(hipStreamWaitEvent(h->stream, h->ev_fin[slot], 0));
  // D counts as read on the lane and on the public stream; a sharded frame never runs on the third lane and does not
  // count towards the quiet frames that open it
  note_frame_readers(h, slot, p, CS, D, (1u << k) | 1u, true, false);
  if (f.keep_counts) S.counts_slot[k] = slot;
  // hits: band totals at this rank's band rows (gv_comm_band), only when kept (the tile pass writes hits[] only then);
  // miss: never, the free-cell bitmaps are complete for this rank's band only
  set_last_frame(h, p, k, k, f.keep_counts, false, f.keep_cell, f.bbox);
  return GV_OK;
}

}  // namespace

// the exchange stream of the sharded frame and the events that chain its steps (ordering only); what exists stays
int gv_context::Shard::create(gv_context *h)
{
  if (!stream_x) GV_HIP(stream_x.create());
  for (auto &row : ev)
    for (auto &e : row)
      if (!e) GV_HIP(e.create(hipEventDisableTiming));
  for (auto &e : t)
    if (!e) GV_HIP(e.create(hipEventDefault));   // timing events
  return GV_OK;
}

namespace gv_internal __attribute__((visibility("hidden"))) {

void comm_destroy(gv_context *h)
{
  if (h->sh.comm) { ncclCommDestroy(h->sh.comm); h->sh.comm = nullptr; }
}

host::ShardPlan shard_plan(const gv_context *h, int world)
{
  return host::ShardPlan(h->g.nx, h->g.ny, h->nx_pad, h->ny_pad, h->nxw, h->ends_words, world);
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
  if (h->sh.active()) return GV_ERR_STATE;
  GV_TRY
  int rc = use_device(h);
  if (rc) return rc;
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof(uid));
  GV_NCCL(ncclCommInitRank(&h->sh.comm, world, uid, rank));
  h->sh.rank = rank;
  h->sh.world = world;
  h->sh.plan = shard_plan(h, world);
  h->layers_in_step = false;   // the bands change hands: the next grid pass writes every row it owns
  return h->sh.create(h);
  GV_CATCH
}

int gv_comm_info(gv_handle h, int32_t *n_ranks, int32_t *rank, int32_t *device)
{
  if (!h) return GV_ERR_BAD_ARG;
  if (!h->sh.active()) return GV_ERR_STATE;
  int nr = 0, rk = 0, dev = 0;
  GV_NCCL(ncclCommCount(h->sh.comm, &nr));
  GV_NCCL(ncclCommUserRank(h->sh.comm, &rk));
  GV_NCCL(ncclCommCuDevice(h->sh.comm, &dev));
  if (n_ranks) *n_ranks = nr;
  if (rank) *rank = rk;
  if (device) *device = dev;
  return GV_OK;
}

int gv_comm_destroy(gv_handle h)
{
  if (!h) return GV_ERR_BAD_ARG;
  if (!h->sh.active()) return GV_OK;
  GV_TRY
  (void)hipSetDevice(h->device);
  (void)drain(h);
  comm_destroy(h);
  h->sh.rank = 0;
  h->sh.world = 1;
  h->sh.plan = shard_plan(h, 1);
  h->layers_in_step = false;
  return GV_OK;
  GV_CATCH
}

int gv_frame_enqueue_sharded(gv_handle h)
{
  if (!h) return GV_ERR_BAD_ARG;
  if (!h->sh.active() || !sector_path(h)) return GV_ERR_STATE;
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
  if (!h->sh.active() || !sector_path(h)) return GV_ERR_STATE;
  int rc = gv_frame_set_detections(h, desc);
  if (rc) return rc;
  if ((rc = gv_frame_enqueue_sharded(h))) return rc;
  return gv_synchronize(h);
}

int gv_time_frame_sharded_stages(gv_handle h, int32_t frames, float stage_ms[6])
{
  if (!h || frames <= 0 || !stage_ms) return GV_ERR_BAD_ARG;
  if (!h->sh.active() || !sector_path(h)) return GV_ERR_STATE;
  GV_TRY
  if (!h->det[h->det_cur].valid) return GV_ERR_STATE;
  int rc = use_device(h);
  if (rc) return rc;
  for (int s = 0; s < 6; ++s) stage_ms[s] = 0.0f;
  for (int32_t i = 0; i < frames; ++i) {   // one frame at a time: every step alone on the device
    if ((rc = enqueue_frame_sharded(h, h->sh.t))) return rc;
    if ((rc = drain(h))) return rc;
    for (int s = 0; s < 6; ++s) {
      float ms = 0.0f;
      GV_HIP(hipEventElapsedTime(&ms, h->sh.t[s], h->sh.t[s + 1]));
      stage_ms[s] += ms;
    }
  }
  for (int s = 0; s < 6; ++s) stage_ms[s] /= (float)frames;
  return GV_OK;
  GV_CATCH
}

// the body of gv_test_frame_sharded_emulated; the caller owns the temporaries and waits for the stream
static int emulate_ranks(gv_context *h, DetSet &D, const host::ShardPlan &plan, DevBuf<uint32_t> *ends, DevBuf<uint32_t> *packs,
                         DevBuf<uint32_t> &comb)
{
  const FrameFlags f = frame_flags(D.flags);
  const int world = plan.world;
  hipStream_t s = h->stream;
  const size_t Ep = plan.slice * (size_t)world;
  int rc2;
  if ((rc2 = comb.reserve(h, Ep))) return rc2;
  for (int r = 0; r < world; ++r)
    if ((rc2 = ends[r].reserve(h, Ep)) || (rc2 = packs[r].reserve(h, plan.chunk * (size_t)world))) return rc2;
  Rect *rects = h->fs[0].rects;
  if ((rc2 = wait_inputs(h, h->cloud[h->cloud_cur], D, 0))) return rc2;
  const int32_t n_rects = enqueue_rects(h, D, rects, h->sb[0].vout, s);
  for (int r = 0; r < world; ++r) {   // every rank bins its slice: buffer set 0, the public stream, no hits[]
    BinningJob bin{D};
    bin.lo = h->n * (size_t)r / (size_t)world;
    bin.n = h->n * (size_t)(r + 1) / (size_t)world - bin.lo;
    bin.keep_cell = f.keep_cell; bin.do_ray = f.ray; bin.do_bbox = f.bbox;
    if ((rc2 = enqueue_binning(h, bin))) return rc2;
    GV_HIP(hipMemcpyAsync(ends[r], h->fs[0].ends, Ep * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  }
  for (int q = 0; q < world; ++q)   // exchange 1: rank q ORs slice q; the all-gather is the union of the slices
    if ((rc2 = shard_or_ends_slice(ShardLink{h, q, plan, ends}, comb, s))) return rc2;
  GV_HIP(hipMemcpyAsync(h->fs[0].ends, comb, Ep * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  for (int r = 0; r < world; ++r) {   // every rank's share of the ray stage, packed by band
    GV_HIP(hipMemsetAsync(h->fs[0].free_, 0, (h->bmN_words + h->bmT_words) * sizeof(uint32_t), s));
    if ((rc2 = shard_rays_and_pack(ShardLink{h, r, plan, packs}, 0, f.ray, packs[r], s))) return rc2;
  }
  for (int q = 0; q < world; ++q) {   // exchange 2 + grid pass of band q
    const ShardLink L{h, q, plan, packs};
    if ((rc2 = shard_or_free_band(L, 0, nullptr, s)) || (rc2 = shard_band_grid_pass(L, 0, rects, n_rects, s))) return rc2;
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
  const FrameFlags f = frame_flags(D.flags);
  if ((rc = check_frame_flags(h, D.flags))) return rc;
  if (!f.bin) return GV_ERR_STATE;
  const host::ShardPlan plan = shard_plan(h, world);   // of this call's `world`, not the communicator's
  if ((rc = h->sh.xchg.reserve(h, plan.scratch_words()))) return rc;
  if ((rc = ensure_point_buffers(h, h->n, (h->n + (size_t)world - 1) / (size_t)world))) return rc;
  // every rank's end bitmaps and packed free bands, and the combined end bitmaps: gone with this call
  std::vector<DevBuf<uint32_t>> ends((size_t)world), packs((size_t)world);
  DevBuf<uint32_t> comb;
  rc = emulate_ranks(h, D, plan, ends.data(), packs.data(), comb);
  (void)hipStreamSynchronize(h->stream);   // on every way out, before the temporaries go
  // no whole count grid (the slices are binned without hits[]) and, as on a rank of the sharded frame, no miss grid
  set_last_frame(h, 0, 0, 0, false, false, f.keep_cell, f.bbox);
  return rc;
  GV_CATCH
}

int gv_comm_band(gv_handle h, int64_t *begin, int64_t *end)
{
  if (!h) return GV_ERR_BAD_ARG;
  const host::ShardPlan::Band &B = h->sh.plan.bands[(size_t)h->sh.rank];
  if (begin) *begin = (int64_t)B.b;
  if (end) *end = (int64_t)B.e;
  return GV_OK;
}

}  // extern "C"
