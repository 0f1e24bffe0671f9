// gv_context.hpp -- the host side's handle (one device + one resident grid + its HIP streams), the buffer sets it
// is made of, and what the gv_api*.hip translation units share: the error macros and the internal functions
// more than one of them calls.
#pragma once

#include <hip/hip_runtime.h>

#include <array>
#include <cmath>
#include <cstdio>
#include <new>
#include <string>
#include <vector>

#include "gv_host_math.hpp"
#include "gv_test_hooks.h"
#include "gv_launch_frame.hpp"
#include "gv_launch_pose.hpp"
#include "gv_launch_planner.hpp"
#include "gv_launch_match.hpp"
#include "gv_launch_frontier.hpp"
#include "gv_launch_gain.hpp"
#include "gv_launch_shortcut.hpp"
#include "gv_resources.hpp"

using namespace gv;

struct ncclComm;   // rccl.h is gv_api_shard.hip's alone
struct gv_context;

namespace gv_internal __attribute__((visibility("hidden"))) {

// One of the three resident clouds: frames read the current one while the copy stream fills the next
// (cloudCallback / timerCallback overlap, src/grid_vision_node.cpp:103-106,108-244).  Three, so that the
// set being filled was last read two uploads ago: its readers have long finished in a streaming run.
struct CloudSet {
  DevBuf<float> base;           // one allocation of 3 * cap floats
  float *x = nullptr, *y = nullptr, *z = nullptr;   // base, base + n, base + 2n of the cloud it holds (SoA, back to back)
  size_t cap = 0;
  DevBuf<uint8_t> raw;          // PointCloud2 bytes before the de-interleave
  Event ready;                  // copy stream: upload complete
  int release_slot = -1;        // ev_fin[release_slot]: the last frame that reads this set (-1: none since it was filled)
  uint32_t seen = ~0u;          // bit k: stream k has waited for `ready` (or the upload is known complete)
};

// Per-frame detection inputs (bboxes, poses / network outputs) and what the device derives from them.
// Sets 0/1 alternate between "read by the frames in flight" and "being uploaded"; set 2 belongs to the
// standalone entry points of the reference surface, which therefore never disturb the frame's inputs.
struct DetSet {
  DevBuf<uint8_t> block;                     // ONE device allocation = one H2D copy per frame; the arrays below point into it
  gv_bbox *bboxes = nullptr;
  gv_lshape_pose *poses = nullptr;
  float *orient = nullptr, *conf = nullptr, *dims = nullptr;
  DevBuf<float4> bbox_f;                     // float thresholds of the bbox test
  DevBuf<unsigned long long> tile_mask;      // candidate masks per 16x16-pixel tile
  int32_t cap = 0;
  int32_t mask_words = 1;
  int32_t nb = 0, n_poses = 0;
  uint32_t flags = 0;
  bool valid = false;           // a gv_frame_set_detections* call has filled this set
  PinnedBuf stage;              // pinned host copy of the caller's arrays (free to reuse on return)
  Event ready;                  // the set's last upload is complete (and has left its staging block)
  uint32_t seen = ~0u;          // bit k: stream k (0 public, 1 / 2 the lanes) is ordered after the upload
  int release_slot = -1;        // last frame that reads this set: ev_fin[release_slot] (a finished grid pass => every earlier frame finished)
  uint32_t readers = 0;         // bit k: a frame on stream k has read this set since its last upload
};

// Buffers of one frame in flight (gv_context::fs[p]: set 0 the serial frame and standalone calls, two sets per lane):
// end bitmaps, free-cell bitmaps, rectangles, ray statistics
struct FrameSet {
  DevBuf<uint32_t> ends;        // one allocation: [hitN | clipN | hitT | clipT], ends_words in all
  uint32_t *hitN = nullptr, *clipN = nullptr, *hitT = nullptr, *clipT = nullptr;
  DevBuf<uint32_t> free_;       // [freeN | freeT]: free-cell bitmaps of the ray stage
  uint32_t *freeN = nullptr, *freeT = nullptr;
  DevBuf<Rect> rects;
  DevBuf<unsigned long long> stats;
  int fin_slot = -1;            // ev_fin slot of the last frame that used the set
};

// What each stream owns (gv_context::sb[k]: 0 public, 1.. the lanes): two frames in flight write their count grid,
// per-point outputs and binning scratch side by side -- partition(f+1) of one lane runs beside tiles(f) of the other
struct StreamBufs {
  DevBuf<int32_t> hits;         // tile path: every cell written by every BIN frame
  DevBuf<int32_t> cell_idx;     // per-point outputs
  DevBuf<int16_t> bbox_id;
  DevBuf<VisionOut> vout;
  DevBuf<uint16_t> bin_keys, bin_tab;   // tile-path binning (gv_binning.hip)
  DevBuf<uint32_t> bin_total[2];
  DevBuf<uint32_t> bin_done, bin_scratch;
  int bin_parity = 0;
  // A lane's partition pass does not depend on the sector kernel queued in front of it (the previous frame of that
  // lane: other buffers), only the in-order queue says so.  When nothing else was put on the lane since that
  // sector kernel -- no wait, no upload, no table kernel -- the partition pass is launched without the barrier
  // bit (hipExtAnyOrderLaunch) and starts while the sector kernel's last workgroups still run.  lane_clean:
  // the last packet on this lane is a sector kernel.  GV_ANYORDER=0 switches it off.
  bool lane_clean = false;
};

// What the last frame left behind, for the getters and the standalone calls that go on from it.  Written in one place,
// set_last_frame (gv_api_frame.hip), which every frame form calls at its end; ensure_point_buffers, end_cloud_upload,
// gv_extract_cloud_per_bbox and enqueue_bbox_pose change single per-point flags.
struct LastFrame {
  int set = 0;                  // fs[set]: free-cell bitmaps (gv_get_miss) and ray statistics
  int stream = 0;               // sb[stream].hits: the count grid
  int points = 0;               // sb[points].cell_idx / .bbox_id: per-point outputs (a tick writes none: they stay where they were)
  bool hits = false, miss = false, cell_idx = false, bbox_id = false;   // what the getters may read
  size_t stat_slots = 1;        // ray statistics slots written by the last ray stage
};

// What a frame descriptor's flag word asks for, decoded once (frame_flags): every frame form reads these.
struct FrameFlags {
  bool bin, ray, bbox;          // GV_FRAME_BIN / RAYMARCH / BBOX_TEST
  bool keep_cell, keep_counts;  // GV_FRAME_KEEP_CELL_IDX / KEEP_COUNTS
  bool vision;                  // GV_FRAME_VISION_ORIENT: rectangles from the network outputs, not from poses
};
inline FrameFlags frame_flags(uint32_t fl)
{
  return {(fl & GV_FRAME_BIN) != 0,           (fl & GV_FRAME_RAYMARCH) != 0,    (fl & GV_FRAME_BBOX_TEST) != 0,
          (fl & GV_FRAME_KEEP_CELL_IDX) != 0, (fl & GV_FRAME_KEEP_COUNTS) != 0, (fl & GV_FRAME_VISION_ORIENT) != 0};
}

// ---- job blocks of the stage calls that the tile frame, the sharded frame, its emulation and the tick share
// (gv_api_frame.hip).  A caller names what it sets; everything else keeps the default written here.

// enqueue_binning: partition + tile histogram of points [lo, lo + n) of the current cloud
struct BinningJob {
  const DetSet &det;                // detection set: bbox-test tables, and the poses of folded rectangles
  int set = 0;                      // fs[set]: the end bitmaps written, the free-cell bitmaps zeroed
  int stream = 0;                   // streams[stream] / sb[stream]: hits[], per-point outputs, binning scratch
  size_t lo = 0, n = 0;             // the points
  bool keep_cell = false;           // write cell_idx
  bool do_ray = false;              // clip the ray ends into the end bitmaps
  bool do_bbox = false;             // bbox test (fused while its tables fit LDS, else a pass of its own)
  bool write_hits = false;          // the tile pass writes every cell of hits[]
  Rect *fold_rects = nullptr;       // non-null: det's poses become rectangles there, on the partition launch
  hipEvent_t ev_points = nullptr;   // recorded between the partition and the tile pass (stage timing)
  bool timed = false;               // the kernels carry kt[0] / kt[1]
  bool any_order = false;           // partition launched without the barrier bit (StreamBufs::lane_clean)
};

// enqueue_sectors: the sector ray stage over the end bitmaps of a set into its free-cell bitmaps
struct SectorsJob {
  int set = 0;                      // fs[set]
  int first = 0, stride = 1;        // workgroups first, first + stride, ... of the dispatch order (a rank's share)
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;        // rides the kernel's dispatch packet when the kernel is launched
  hipEvent_t t0 = nullptr;          // the kernel's start (stage timing)
  bool done_attached = false;       // out: a kernel was launched and carries `done`
};

// enqueue_grid_pass: the tile grid pass over rows [y0, y1) with the bitmaps of a set
struct GridPassJob {
  int set = 0;                      // fs[set]
  const Rect *rects = nullptr;      // index rectangles of the detections
  int32_t n_rects = 0;
  bool counts = false;              // apply the hit / miss rule (false: a plain map update)
  int32_t y0 = 0, y1 = 0;           // rows
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;        // rides the kernel's packet, or is recorded behind a pass that launched nothing
  hipEvent_t t0 = nullptr;          // the kernel's start (stage timing)
  bool sharded = false;             // a rank's band: written whole, leaves the layers out of step
  bool of_frame = true;             // false: a plain update (diagnostic build: the timeline stamps stay with the frames)
  bool launched = false;            // out: a kernel ran
};

// upload_det: the caller's arrays into a detection set, in one copy, and the bbox-test tables derived there
struct DetUpload {
  const gv_bbox *bboxes = nullptr;
  int32_t nb = 0;
  const gv_lshape_pose *poses = nullptr;
  int32_t n_poses = 0;
  const float *orient = nullptr, *conf = nullptr, *dims = nullptr;   // network outputs of n_net boxes, or null
  hipStream_t stream = nullptr;
  bool masks = true;                // false: only kernels that read the raw boxes / poses follow; no bbox-test tables
  int32_t n_net = -1;               // boxes the network outputs cover (-1: nb)
  int32_t nb_test = -1;             // the bbox test covers the first nb_test boxes only (-1: nb)
  bool fused = false;               // one kernel reads the pinned staging: copy + tables, no copy command
};

// Experiment and sweep knobs: read from the environment by read_tuning (gv_api.hip), once, at gv_create.
struct Tuning {
  int n_lanes = 3;                  // GV_LANES=2: two lanes
  bool lane3_own_stream = false;    // GV_LANE3_OWN_STREAM (experiment): the third lane on a fifth stream instead of the upload stream
  bool queue_probe = true;          // GV_QUEUE_PROBE=0: no probe of the upload stream's hardware queue
  bool verbose = false;             // GV_VERBOSE: the probe's result on stderr
  bool no_pipeline = false;         // GV_PIPELINE=0
  bool force_simple = false;        // GV_RAY_IMPL=simple
  bool tick_knn_lane = true;        // GV_TICK_KNN_LANE=0: the static boxes' kNN in line on the public stream
  bool grid_skip = true;            // GV_GRID_SKIP=0: every grid pass dense (A/B runs, tests)
  bool anyorder = true;             // GV_ANYORDER=0: no any-order partition launches (StreamBufs::lane_clean)
  host::SectorTuning sec;           // the sector ray stage's knobs: what host::SectorPlan reads (gv_host_math.hpp)
  int32_t nav_pass_cap = kNavPassCap;   // GV_NAV_PASS_CAP: passes of a tile per round of gv_nav_field (tests: the cap's own path)
#ifdef GV_DIAG
  int32_t ablate = 0;               // GV_ABLATE
  bool bin_dbg = false, timeline = false, sector_dbg = false;   // GV_BIN_DBG / GV_TIMELINE / GV_SECTOR_DBG = 1: the stamp buffers exist
#endif
};

// Result block of the synchronous kNN / RANSAC / PCA calls and of the tick: pinned, coherent and device-mapped, written
// by the call's last kernel; [0] = the sequence number of the last finished call (CallDone, gv_types.hpp), payload
// from byte kHeader (gv_api_pose.hip)
struct ResultBlock {
  static constexpr size_t kHeader = 64;
  static_assert(kHeader % 16 == 0, "the payload keeps the block's alignment (PoseBlock)");
  PinnedBuf host;
  DevBuf<unsigned> ticket;
  unsigned seq = 0;                 // of the last call begun; never 0 ("nothing published yet")
  uint8_t *payload() const { return host.get() + kHeader; }
  // room for `bytes` of payload and the CallDone of the call about to be enqueued; refused while a tick is pending
  int begin(gv_context *h, size_t bytes, CallDone &done);
  int wait(gv_context *h);          // host side of CallDone: spins until the call begun last has published
};

}  // namespace gv_internal

using namespace gv_internal;

struct __attribute__((visibility("hidden"))) gv_context {
  // Frames in flight run on LANES (three; GV_LANES=2: two): frame f does partition, tile pass and sector stage back
  // to back on the in-order stream of lane f % lanes, then its grid pass on the PUBLIC stream behind one event.
  // No event sits between the stages on a lane (a barrier packet between two kernels costs ~6 us of queue time,
  // back to back kernels of one queue follow each other with a gap of a few us that the other lanes fill), the
  // grid passes are one in-order sequence by construction (the log-odds grid is one sequence of updates), and
  // everything a frame produced is visible on the public stream right behind it.  Buffer sets 1..2*lanes rotate
  // with the frames (set 0: serial frames and standalone calls); a set is handed to frame f + 2*lanes once the
  // HOST has seen frame f finish -- back-pressure on the caller instead of a barrier on a lane.
  // Measured on config 3: one in-order stream 12.0 k frames/s; one stream per STAGE with three events per frame
  // (round 1) 14.4 k; two lanes with the grid pass on the lane behind a cross-lane wait 16.5 k; two lanes as above
  // 18.6 k in round 2, 23.5 k at the end of round 3; three lanes 24.7 k (the in-kernel timeline of the two-lane
  // form shows the lanes in step, all of them between kernels at the same moments: profiles/r03/native_timeline.txt).
  // Three lanes + public + copy are five streams on the four hardware queues a process gets by default; with
  // GPU_MAX_HW_QUEUES=8 the same five streams run slower (57 us per frame against 40).  Independent HANDLES side by
  // side (three or four grids, round 2: 15.4 / 14.3 k, tools/multi_handle.py) are a different thing: every grid
  // pays its own grid pass.
  static constexpr int kLanesMax = 3;              // three lanes by default, GV_LANES=2: two
  static constexpr int kStreams = 1 + kLanesMax;   // public + lanes
  static constexpr int kSets = 1 + 2 * kLanesMax;  // set 0: the serial frame; two sets per lane
  static constexpr int kRing = 8;   // event rings: one slot per frame, reused every 8 frames
  Tuning tune;
  int upload_stream_retries = 0;    // gv_create: upload streams replaced because they shared a hardware queue
  double upload_probe_us = 0.0;     // the last probe's wait
  // The third lane runs on the UPLOAD stream (public + two lanes + uploads are the four hardware queues a process
  // gets; a fifth stream shares one of them with whatever the runtime picks, and when that is the upload stream the
  // streamed frame drops to 0.8 of the copy rate).  It is used only while the upload stream is quiet: no cloud
  // upload for kQuietFrames frames.  With a cloud per frame the library runs on two lanes, as in round 2.
  static constexpr uint32_t kQuietFrames = 8;
  uint32_t quiet_frames = 0;        // frames enqueued since the last cloud upload
  int lanes_now() const { return (tune.n_lanes == 3 && quiet_frames >= kQuietFrames) ? 3 : 2; }
  int device = 0;
  // (the streams come before every buffer and event: members go in reverse order, the streams last)
  Stream stream, stream_copy;       // public, uploads
  Stream lane[kLanesMax];           // lane[2] exists only with GV_LANE3_OWN_STREAM
  // Multi-GPU: one large frame sharded by points (gv_api_shard.hip).  Here, with the streams, because it owns one: its
  // buffer and events go before it, and it goes behind every other buffer and event of the handle.
  struct Shard {
    ncclComm *comm = nullptr;       // (ncclComm_t)
    int32_t rank = 0, world = 1;
    host::ShardPlan plan;           // of this grid and `world`: gv_create (world 1), gv_comm_init, gv_comm_destroy
    Stream stream_x;                // the exchanges (RCCL) of the sharded frame
    DevBuf<uint32_t> xchg;          // exchange scratch, plan.scratch_words(): received slices / packed and received bands
    Event ev[kRing][5];             // per frame slot: binning, exchange 1, sectors + packing, exchange 2, grid pass done
    Event t[7];                     // stage timing of the sharded frame (gv_time_frame_sharded_stages)
    // per stream: ev_fin slot of its last sharded KEEP_COUNTS frame in flight (its last exchange reduces hits in place)
    int counts_slot[kStreams];
    Shard() { forget_frames(); }
    bool active() const { return comm != nullptr; }
    void forget_frames() { for (int &c : counts_slot) c = -1; }   // every frame in flight has finished (drain)
    int create(gv_context *h);      // the exchange stream and the events, once (gv_comm_init)
  } sh;
  hipStream_t streams[kStreams]{};  // what the frame code indexes: {stream, lane[0], lane[1], lane[2] or else stream_copy}
  // every stream the handle owns, in the order drain waits for them (null: not created)
  std::array<hipStream_t, 3 + kLanesMax> own_streams() const { return {stream_copy, stream, lane[0], lane[1], lane[2], sh.stream_x}; }
  Event ev_sec[kRing];              // lane: partition, tile pass, sector stage of frame (slot) done
  Event ev_fin[kRing];              // public stream: grid pass of frame (slot) done => that frame and every earlier one are done
  Event ev_join;                    // copy stream -> public stream (gv_frame_fence)
  uint64_t lane_frames = 0;         // lane frames enqueued so far: lane = n % lanes, buffer set = 1 + n % (2 * lanes)
  int last_fin_slot = -1;           // ev_fin slot of the most recently enqueued frame (-1: idle)
  FrameSet fs[kSets];             // per-set buffers of the frames in flight
  StreamBufs sb[kStreams];        // per-stream buffers
  size_t ends_words = 0, bmN_words = 0, bmT_words = 0;
  DevBuf<uint8_t> miss8;          // generic path only: byte miss grid of the literal march
  LastFrame last;
  uint64_t frame_no = 0;
  bool pipe_busy = false;         // lane frames enqueued since the streams were last drained
#ifdef GV_DIAG
  std::vector<Event> *trace = nullptr;        // timing events around every pipelined kernel (gv_debug_pipeline_trace)
  DevBuf<unsigned long long> d_dbg;           // GV_SECTOR_DBG=1: phase stamps of the sector kernel
  DevBuf<unsigned long long> d_bin_dbg[2];    // GV_BIN_DBG=1: phase stamps of the partition / tile kernels
  DevBuf<unsigned long long> d_tl;            // GV_TIMELINE=1: {begin, end} of the four kernels of the last kTlFrames frames
  static constexpr uint64_t kTlFrames = 4096;
  unsigned long long *tl_slot(int kernel) const
  {
    return d_tl ? d_tl.get() + ((frame_no % kTlFrames) * 4 + (uint64_t)kernel) * 2 : nullptr;
  }
#endif
  GridParams g{};
  gv_cam_params cam{};
  CamK camk{};
  double K[9]{}, Kinv[9]{};

  bool has_cl = false, has_bc = false, has_bl = false;
  gv_transform tf_cl{}, tf_bc{}, tf_bl{};
  Mat34f m_cam{}, m_base{};
  Xform64 x_bc{};
  RayOrigin org{};

  // grid state (resident across frames)
  DevBuf<float> log_odds, occupancy;
  DevBuf<int8_t> occ_i8;
  // The tile grid pass leaves a tile row alone whose log-odds it did not change by a bit (cells at a clamp: most of
  // a map in steady state).  That is right only while occupancy and occ_i8 hold what the grid pass derives from the
  // current log-odds: layers_in_step.  False after gv_set_log_odds (one layer replaced), after a sharded frame (a
  // rank writes its own band only, and bands can change) and after any change of communicator; true after gv_reset
  // (0.0 / 0.5 / 50 is such a triple) and once a dense pass over all rows has been enqueued.  gv_grid_move moves the
  // three layers together.  The flag is read when a grid pass is ENQUEUED: grid passes are one in-order sequence on
  // the public stream, so the pass that reads `true` runs behind the dense pass or the fill that made it true, and
  // gv_set_log_odds drains every stream before it copies.  A caller that writes through gv_device_layers' pointers
  // puts the layers out of step without the handle knowing.
  bool layers_in_step = false;
  bool grid_pass_dense() const { return !tune.grid_skip || !layers_in_step; }
  // [EXTENSION] X3 ego motion (gv_grid_move): the current base frame in the frame the layers are registered in, and
  // the scratch copy of the three layers the resample gathers into (allocated by the first applied move)
  host::Se2 move_residue{0.0, 0.0, 0.0};
  DevBuf<uint8_t> move_scratch;
  // [EXTENSION] X4 height band of the lidar map update (gv_set_height_band): handle configuration, copied into the
  // kernel arguments of every binning launch at enqueue
  HeightBand band{-INFINITY, INFINITY, 0};
  // Host data on its way to the device through two pinned staging slots: slot k is filled by memcpy, leaves by one copy
  // command on the public stream and is marked by an event, k alternating; it is rewritten only once its last copy has
  // left it -- two uploads ago, the one host wait that can occur here (stage_upload, gv_api_planner.hip).
  struct StageSlots {
    PinnedBuf stage[2];
    Event staged[2];
    bool staged_used[2] = {false, false};
    int slot = 0;                           // of the current contents
  };
  // ... into device slot k: a kernel already enqueued keeps reading the slot it was given, and the copy into a slot runs
  // behind every kernel that was given it (one in-order stream).  upload_slot fills the slot that is not current and
  // makes it current; so does a gv_track_update with GV_TRACK_FEED_DYNAMIC for X13's object table, whose kernel writes
  // that slot itself (no staging) before the call flips st.slot.
  struct UploadSlots {
    DevBuf<uint8_t> dev[2];
    StageSlots st;
    uint8_t *current() const { return dev[st.slot].get(); }
  };
  // [EXTENSION] X6 inflated costmap (gv_set_inflation / gv_inflate).  The configuration and its host-built table are
  // handle state; the buffers are made by the first gv_inflate (dist2 by the first one that keeps it).  A changed
  // table reaches the device with the next gv_inflate, through `table`.
  struct Inflation {
    bool set = false;
    int32_t thr = 0, flags = 0;
    host::InflationTable tab;
    bool dirty = false;               // `tab` is newer than the device slot
    UploadSlots table;
    DevBuf<unsigned long long> bits;  // lethal bitmap (guard words zero since allocation)
    DevBuf<uint8_t> cost;
    DevBuf<uint16_t> dist2;
    bool have_cost = false, have_dist2 = false;   // a gv_inflate since gv_create / gv_reset; the last one kept dist2
  } infl;
  // [EXTENSION] X7 trajectory scoring (gv_set_footprint / gv_score_trajectories*).  The footprint is handle
  // configuration, copied into the kernel arguments of every call at enqueue.  The buffers are made by the first call
  // that needs them and grow with K * P: the landing places of results whose destination the kernel cannot write
  // itself (pageable memory).  Both are used on the public stream only, so a call's kernel and copies run behind
  // those of the call before it.
  struct TrajScore {
    bool set = false;
    gv_footprint fp{};
    DevBuf<gv_traj_score> d_scores;
    DevBuf<uint8_t> d_pose_cost;
  } traj;
  // [EXTENSION] X9 goal / path distance field (gv_set_nav_config / gv_nav_field / gv_score_nav*).  The configuration is
  // handle state; the buffers are made by the first call that needs them.  gv_nav_field is the one call here that waits
  // on the host between its launches (rounds until one changes nothing), so its staging block is never in flight when
  // the next call fills it.  The sampler's buffers follow TrajScore's rules.
  struct NavField {
    static constexpr int kBatchMax = 64;    // rounds enqueued between two host waits, at most
    bool set = false;
    gv_nav_config cfg{};
    DevBuf<uint32_t> field;                 // G rounded up to a multiple of 4
    bool have_field = false;                // a gv_nav_field since gv_create / gv_reset
    DevBuf<uint32_t> flags;                 // [2][tiles]: this round's and the next round's active tiles
    DevBuf<uint32_t> counters;              // [0] seeds used, [1 + i] tiles changed by round i of the batch
    DevBuf<int32_t> d_seeds;
    PinnedBuf stage;                        // the counters' landing place, then the seed cells on their way in
    Event done;                             // public stream: a batch's counters have landed
    DevBuf<gv_nav_score> d_scores;          // the sampler: the landing place of records bound for pageable memory
  } nav;
  // [EXTENSION] X17 paths walked down that field (gv_nav_path* / gv_nav_field_from_path, gv_api_path.hip).  The resident
  // paths of the last call -- entries[S][cap], xy[S][cap][2] and the S records -- are in buffers of their own, made by
  // the first call and grown by a larger one, so a later gv_nav_field or gv_nav_field_from_path leaves them alone;
  // gv_reset invalidates them with the field.  The start cells go to `d_starts` through `up`'s staging slots.  All of
  // it is used on the public stream only: a call's copy and kernel run behind those of the call before it, and the
  // buffers double as the landing places of results bound for pageable memory.
  struct NavPath {
    DevBuf<int32_t> entries;
    DevBuf<float> xy;
    DevBuf<gv_nav_path_info> info;
    DevBuf<int32_t> d_starts;
    StageSlots up;
    int32_t S = 0, cap = 0;                 // of the resident paths
    bool have = false;                      // a path call since gv_create / gv_reset
  } path;
  // [EXTENSION] X19 frontier clusters (gvx_set_frontier_config / gvx_frontier* / gvx_nav_field_from_frontier,
  // gv_api_frontier.hip).  The configuration is handle state and travels in the kernel arguments; gv_reset keeps it.  The
  // buffers are made by the first call and grown by a larger one: the frontier bitmap (guard words zero since
  // allocation), `parent` and `labels` (the two words per cell), `head` (four counters and one count per workgroup,
  // zeroed on the stream by every call), the two keys per written cluster, and the resident records and info, which
  // double as the landing places of results bound for pageable memory.  All of it is used on the public stream only.
  // After a call `parent[label]` is a cluster's index among the written ones: what the seed kernel reads.
  struct Frontier {
    bool set = false;
    gvx_frontier_config cfg{};
    DevBuf<unsigned long long> bits;
    DevBuf<uint32_t> parent, labels, head;
    DevBuf<unsigned long long> keys;
    DevBuf<gvx_frontier_record> rec;
    DevBuf<gvx_frontier_info> info;
    int32_t cap = 0;                        // of the resident records
    bool have = false;                      // a frontier call since gv_create / gv_reset
  } frontier;
  // [EXTENSION] X20 information gain of exploration goals (gvx2_set_gain_config / gvx2_gain* / gvx2_frontier_gain* /
  // gvx2_nav_field_from_gain, gv_api_gain.hip).  The configuration is handle state and travels in the kernel arguments;
  // gv_reset keeps it.  The buffers are made by the first call, at their largest (4096 records, 4096 entries): the
  // resident records and info, which double as the landing places of results bound for pageable memory, and the device
  // copy of host entries, which come through `up`'s staging slots.  All of it is used on the public stream only.  A
  // frontier call reads Frontier's resident records and info in place.
  struct Gain {
    bool set = false;
    gvx2_gain_config cfg{};
    DevBuf<gvx2_gain_record> rec;
    DevBuf<gvx2_gain_info> info;
    DevBuf<int32_t> d_entries;
    StageSlots up;
    int32_t n = 0;                          // record slots of the resident result: n of a list call, the cap of a frontier call
    bool have = false;                      // a gain call since gv_create / gv_reset
  } gain;
  // [EXTENSION] X21 shortcuts and waypoints of the resident paths (gvx3_set_shortcut_config / gvx3_shortcut* /
  // gvx3_nav_field_from_shortcut, gv_api_shortcut.hip).  The configuration is handle state and travels in the kernel
  // arguments; gv_reset keeps it.  The resident waypoints of the last call -- entries[S][wcap], index[S][wcap],
  // xy[S][wcap][2] and the S records -- are in buffers of their own, made by the first call and grown by a larger one, so
  // NavPath's buffers, which the kernel reads in place, are left as they are; gv_reset invalidates them with the paths.
  // All of it is used on the public stream only, and the buffers double as the landing places of results bound for
  // pageable memory.
  struct Shortcut {
    bool set = false;
    gvx3_shortcut_config cfg{};
    DevBuf<int32_t> entries, index;
    DevBuf<float> xy;
    DevBuf<gvx3_shortcut_info> info;
    int32_t S = 0, wcap = 0;                // of the resident waypoints
    bool have = false;                      // a shortcut call since gv_create / gv_reset
  } shortcut;
  // [EXTENSION] X10 rollout and control step (gv_set_motion_model / gv_rollout* / gv_control_step*).  The motion model is
  // handle configuration, copied into the kernel arguments of every rollout at enqueue.  `poses` is the resident
  // rollout, a buffer of its own (d_poses below is the staging copy of host poses, which every scoring call
  // overwrites); it does not depend on the map, so gv_reset keeps it, and it moves only when a larger rollout grows it.
  // The control step's samplers write their records into traj.d_scores and nav.d_scores, which are also the landing
  // buffers of the asynchronous scoring calls: every user enqueues on the public stream only, so a control step's
  // kernels run behind the copy command that empties a landing buffer, and a later scoring call's kernel behind
  // k_control_select.  d_result / d_totals are the landing places of a result bound for memory the kernel cannot write.
  struct Rollout {
    bool set = false;                       // a motion model is in force
    gv_motion_model model{};
    DevBuf<float> poses;                    // K * P * 3
    int32_t K = 0, P = 0;                   // of the last rollout
    bool have = false;                      // a rollout since gv_create
    DevBuf<float> d_controls;               // the device copy of host controls
    DevBuf<gv_control_result> d_result;
    DevBuf<uint64_t> d_totals;
  } roll;
  // [EXTENSION] X11 MPPI sampling and softmax update (gv_set_mppi / gv_mppi_*).  The configuration is handle state, copied
  // into the kernel arguments at enqueue.  `nominal` and `controls` are buffers of their own that remember their shape;
  // neither depends on the map, so gv_reset keeps them, and `controls` moves only when a larger sampling grows it.  An
  // update has k_control_select write into roll.d_result / roll.d_totals (device memory, the control step's landing
  // places: every user enqueues on the public stream only) and reads them there; `partial` holds the chunk sums.
  struct Mppi {
    bool set = false;                       // a configuration is in force
    gv_mppi_config cfg{};
    DevBuf<float> nominal;                  // P * C
    int32_t P = 0, C = 0;                   // of the nominal
    bool have_nominal = false;              // a gv_mppi_set_nominal since gv_create
    DevBuf<float> controls;                 // K * P * C
    int32_t cK = 0, cP = 0, cC = 0;         // of the last sampling
    bool have_controls = false;             // a sampling since gv_create
    DevBuf<double> partial;                 // chunks * (P * C + 1)
    // [EXTENSION] X12 (gv_set_mppi_limits): handle state like cfg, copied into the kernel arguments at enqueue
    bool lim_set = false;                   // limits are in force
    gv_mppi_limits lim{};
    bool c_shift = false;                   // the last sampling's GV_MPPI_SHIFT, next to cK / cP / cC
    DevBuf<double> cost;                    // g[K], then x[K]
    DevBuf<uint64_t> x_min;                 // mppi_min_key of the smallest admitted x
    int32_t costK = 0;                      // of the last update with gamma > 0
    bool have_costs = false;                // the last update ran with gamma > 0
  } mppi;
  // [EXTENSION] X13 scoring against predicted moving objects (gv_set_dyn_config / gv_set_moving_objects /
  // gv_score_dynamic*).  The configuration and its host-built cost table are handle state; a changed table reaches the
  // device with the next call that scores, through `table` like Inflation's.  The object table is built on the
  // host by gv_set_moving_objects and copied on the public stream through slots of its own; n_obj travels in the kernel
  // arguments.  Neither depends on the map: gv_reset keeps both.  d_scores / d_pose_cost follow TrajScore's rules, and
  // d_scores is also where the control step's dyn sampler writes.
  struct DynScore {
    bool set = false;
    gv_dyn_config cfg{};
    host::InflationTable tab;
    bool dirty = false;                     // `tab` is newer than the device slot
    UploadSlots table;
    int32_t n_obj = 0;                      // of the set in force for the calls enqueued from now on
    UploadSlots objs;
    DevBuf<gv_dyn_score> d_scores;
    DevBuf<uint8_t> d_pose_cost;
    // [EXTENSION] X14: non-null when the set in force was written on the device by a fed gv_track_update; it points
    // at the count beside the rows of objs' current slot, and n_obj is then the bound 128.
    const int32_t *n_obj_dev = nullptr;
  } dyn;
  // [EXTENSION] X14 the tracker over the tick's boxes (gv_set_track_config / gv_set_tracks / gv_get_tracks /
  // gv_track_update*).  The configuration is handle state and travels in the kernel arguments.  The 128 slots and
  // next_id are resident in `state`, which the one update kernel rewrites in place on the public stream; `fresh` says
  // that the state is the one after gv_create (no tracks, next_id 1) whatever the block holds, so that turning the
  // tracker off needs no device work.  gv_set_tracks goes through `up`'s staging slots into `state`.
  // Host detections go through `dets`' alternating slots like X13's object table (the caller's array is free on return).  d_info and
  // d_tracks are the landing buffers of destinations that are not pinned.  gv_reset keeps all of it.
  struct Track {
    bool set = false;
    gv_track_config cfg{};
    bool fresh = true;
    DevBuf<TrackState> state;
    StageSlots up;
    UploadSlots dets;
    DevBuf<gv_track_info> d_info;
    DevBuf<gv_track> d_tracks;
  } trk;
  // [EXTENSION] X16 scan-to-costmap matching (gv_set_match_config / gv_match_scan*, gv_api_match.hip).  The
  // configuration is handle state and travels in the kernel arguments with the guess and the rotation table.  `pts`
  // (the used points' base-frame x, y) and `head` (the counter of used points, then the score volume) are the scratch
  // of one call, made by the first call that needs them and used on the public stream only: a call's memset and
  // kernels run behind those of the call before it.  d_result follows TrajScore's rules.  gv_reset keeps all of it.
  struct Match {
    bool set = false;
    gv_match_config cfg{};
    DevBuf<float2> pts;
    DevBuf<uint32_t> head;
    DevBuf<gv_match_result> d_result;
  } match;
  // [EXTENSION] X18 wide-window matching by branch and bound (gv_set_search_config / gv_match_search*,
  // gv_api_match.hip).  The configuration is handle state, independent of Match's, and travels in the kernel arguments.
  // The buffers are the scratch of one call, made by the first call that needs them, grown by a larger one and used on
  // the public stream only: `pts` and `head` as Match's (head: the counters, the pre-slots, the bounds), `rows` and
  // `pool` the costmap pooled along x and then along y (pooled per call: a call reads the costmap of the inflate before
  // it), `list` the survivors and `slots` their exact scores, n_blocks * S * S words at the worst.  d_result and d_stats
  // follow TrajScore's rules; d_stats also takes the stats nobody asked for.  gv_reset keeps all of it.
  struct Search {
    bool set = false;
    gv_search_config cfg{};
    DevBuf<float2> pts;
    DevBuf<uint32_t> head;
    DevBuf<uint8_t> rows, pool;
    DevBuf<uint32_t> list, slots;
    DevBuf<gv_match_result> d_result;
    DevBuf<gv_search_stats> d_stats;
  } search;
  // The scan readers of the cloud sets: one event and one mask for both matchers (enqueue_scan_read, gv_api_match.hip).
  // `read` marks the point pass of the last gv_match_scan* or gv_match_search* call, the one kernel of either that
  // reads the cloud; it is recorded again by every call on the one in-order stream, so whoever waits for it is behind
  // every earlier call's point pass too.  `clouds` has bit s set when a call has read cloud set s since the set was last
  // uploaded into or the streams were last drained: any number of calls may be in flight over the three sets, and an
  // upload into a set whose bit is set waits for `read` and clears that bit alone (begin_cloud_upload).  gv_reset
  // keeps both.
  struct ScanReaders {
    Event read;
    uint32_t clouds = 0;
  } scan_readers;
  // The device copy of a sampler's host poses (K * P * 3 floats), one for gv_score_trajectories* and gv_score_nav*.
  // Both enqueue on the public stream only, so a call's copy into it runs behind the kernel of the call before it;
  // and it grows by DevBuf::reserve, hipFree + hipMalloc, where hipFree waits for the device: the block a kernel in
  // flight reads is not released under it.
  DevBuf<float> d_poses;
  // per-frame count grids (sb[k].hits; generic path: sb[0].hits)
  DevBuf<uint8_t> clip_end;                 // generic path only
  DevBuf<uint32_t> ray_list;
  DevBuf<uint32_t> ray_count;               // [0] = number of list entries
  DevBuf<int32_t> scratch_i32;              // G ints (miss read-back), also max(N) ints for id read-back
  int32_t nxw = 0, nyw = 0, nx_pad = 0, ny_pad = 0;
  bool tile_path = false;                   // nx % 4 == 0 and the grid fits the packed (a,b) fields

  // tile-path binning (gv_binning.hip): what every stream's scratch holds
  int32_t tiles_x = 0, tiles_y = 0, n_tiles = 0;
  size_t bin_keys_cap = 0, bin_tab_cap = 0;
  size_t bin_slots = 0;

  // resident clouds
  CloudSet cloud[3];
  int cloud_cur = 0;
  bool cloud_wait = false;                  // an asynchronous upload may still be in flight
  float *cx = nullptr, *cy = nullptr, *cz = nullptr;   // = cloud[cloud_cur]
  size_t n = 0;
  DevBuf<float> tx, ty, tz;                 // transformed copy (A1 read-back)
  size_t idx_cap = 0;                       // per-point outputs (sb[k].cell_idx / .bbox_id) hold this many points

  // detections
  DetSet det[3];
  int det_cur = 0;
  int32_t bt_tiles_x = 1, bt_tiles_y = 1;   // 16x16-pixel tiles of the image
  int32_t vout_cap = 0;                     // rectangles, vision outputs (all sets) and centre points
  DevBuf<double> d_pts;
  // kNN depth, RANSAC ground plane, per-box radius filter + PCA rectangle (gv_api_pose.hip).  Every group of buffers is
  // made by the first call that needs it and grows through one function of gv_api_pose.hip over the buffers' own cap():
  // a group whose second allocation failed has a member without room, so the next call grows it again.
  struct Pose {
    DevBuf<Cand2> knn_partial;        // stage-1 candidate lists of the kNN
    // per point of the cloud (n + n / 8 + 1024)
    DevBuf<CellNode> nodes;           // selected points in bucket order
    DevBuf<uint8_t> keep;             // 1 = survives the radius filter
    DevBuf<uint32_t> ticket_of;       // per cloud point: its slot inside its bucket (selected points only)
    // per bbox (nb + nb / 4 + 64): integer sums / extent keys of the PCA rectangle; every call leaves them zero
    DevBuf<long long> pca_acc;
    DevBuf<unsigned> pca_ext;
    DevBuf<unsigned> pca_ticket;
    // cell buckets: counts, prefix, block offsets (BucketTable, gv_launch_pose.hpp); the counts and the ticket are zero between calls
    DevBuf<uint32_t> cellcnt, cellpre, celloff;
    BucketTable buckets() const
    {
      return {cellcnt, cellpre, celloff, (uint32_t)BucketTable::held(cellcnt.cap(), cellpre.cap(), celloff.cap())};
    }
    DevBuf<unsigned> plane_counts;    // inlier counts of the hypotheses; every pass leaves them zero
    DevBuf<uint8_t> ground;           // last ground mask (device resident)
    size_t ground_n = 0;
    DevBuf<double> rscratch;          // tree-sum partials of the plane refinement
    DevBuf<RansacState> rstate;
    ResultBlock res;
  } pose;

  // the node's tick (gv_tick_enqueue / gv_tick_wait): what the pending tick put where in the result block
  struct Tick {
    bool pending = false;
    uint32_t flags = 0;
    int32_t n_all = 0, n_static = 0, n_dynamic = 0;
    bool pca_ran = false, vision_ran = false, knn_ran = false;
    size_t off_depth = 0, off_pose = 0, off_vout = 0;
    std::vector<gv_bbox> st_boxes;   // the static boxes (host copy: convertPixelsTo3D after the wait)
    // the handle's state at enqueue that the wait reads: uploads and gv_set_transforms may come in between
    size_t n = 0;                    // points of the cloud the tick reads ("empty segmented cloud" is m == n)
    int cloud = -1;                  // its cloud set: an upload into it waits for `done` on the device
    gv_transform tf_bc{};            // camera->base of the poses and base points
    Xform64 x_bc{};
    Event done;                      // public stream: everything the tick enqueued has finished
    Event fork, join;                // the kNN depth on a lane beside the pose branch
    // [EXTENSION] X15 the detection list of a GV_TICK_KEEP_DETS tick (k_tick_dets, gv_track.hip): one block for the
    // handle's life, written only by that kernel and read in place by gv_track_update*(GV_TRACK_TICK_DETS), all on the
    // public stream.  dets_vout / dets_valid: what the pose kernels otherwise leave only in the pinned result block.
    // dets_live: the most recently enqueued tick carried the flag (cleared when a gv_tick_enqueue starts).
    DevBuf<TickDetList> dets;
    DevBuf<VisionOut> dets_vout;
    DevBuf<uint8_t> dets_valid;
    bool dets_live = false;
  } tick;

  bool counts_dirty = false;   // generic path: hits/miss/clip_end hold a kept frame

  Event ev[kNumStages + 1];
  // stage timing (gv_time_frame_stages): start / end of the partition, tile-pass, sector and grid-pass kernels,
  // taken from their own dispatch packets; kt_used: the kernel was launched in the frame just timed
  Event kt[4][2];
  bool kt_used[4]{};
  std::string err;
};

using host::kMaxStatSlots;

#define GV_HIP(call)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      char buf_[256];                                                                         \
      std::snprintf(buf_, sizeof(buf_), "%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
      h->err = buf_;                                                                          \
      return GV_ERR_HIP;                                                                      \
    }                                                                                         \
  } while (0)

#define GV_TRY try {
#define GV_CATCH                               \
  }                                            \
  catch (const std::bad_alloc &) {             \
    if (h) h->err = "host allocation failed";  \
    return GV_ERR_HIP;                         \
  }                                            \
  catch (...) {                                \
    if (h) h->err = "unexpected exception";    \
    return GV_ERR_HIP;                         \
  }

#define GV_NCCL(call)                                                                          \
  do {                                                                                         \
    ncclResult_t r_ = (call);                                                                  \
    if (r_ != ncclSuccess) {                                                                   \
      char buf_[256];                                                                          \
      std::snprintf(buf_, sizeof(buf_), "%s:%d %s -> %s", __FILE__, __LINE__, #call, ncclGetErrorString(r_)); \
      h->err = buf_;                                                                           \
      return GV_ERR_RCCL;                                                                      \
    }                                                                                          \
  } while (0)

// internal functions that more than one translation unit calls (hidden: they add nothing to the library's exports)
namespace gv_internal __attribute__((visibility("hidden"))) {
// gv_api.hip
int drain(gv_context *h);
bool sector_path(const gv_context *h);
int set_device_only(gv_context *h);
int use_device(gv_context *h);
int enqueue_plain_update(gv_context *h, int32_t n_rects);
FinalizeArgs finalize_args(const gv_context *h, int32_t n_rects);
int ensure_tbuf(gv_context *h, size_t n);
int copy_out(gv_context *h, void *dst, const void *src, size_t bytes);
void convert_pixels_host(const double Kinv[9], const Xform64 &x_bc, const gv_bbox *bboxes, const float *depths, int32_t nb,
                         double *base_points_xyz);
void *pinned_device_view(void *p, size_t align);
int publish_layer_async(gv_context *h, const int8_t *src, int8_t *data);
// gv_api_frame.hip
int ensure_point_buffers(gv_context *h, size_t n, size_t n_slice = 0);
int ensure_det(gv_context *h, DetSet &d, int32_t n);
int ensure_det_shared(gv_context *h, int32_t n);
BBoxTest bbox_test_of(const gv_context *h, const DetSet &d);
PointsArgs bbox_points_args(const gv_context *h, const DetSet &D, size_t lo, size_t n, int16_t *ids);
void set_last_frame(gv_context *h, int set, int stream, int points, bool hits, bool miss, bool cell_idx, bool bbox_id);
void note_frame_readers(gv_context *h, int slot, int p, CloudSet &CS, DetSet &D, uint32_t readers, bool on_lane, bool quiet);
int upload_det(gv_context *h, DetSet &d, const DetUpload &u);
int upload_scratch_bboxes(gv_context *h, const gv_bbox *b, int32_t nb, bool masks = true);
int32_t enqueue_rects(gv_context *h, const DetSet &D, Rect *rects, VisionOut *vout, hipStream_t s);
int check_frame_flags(const gv_context *h, uint32_t fl);
int enqueue_binning(gv_context *h, const BinningJob &job);
int enqueue_sectors(gv_context *h, SectorsJob &job);
int enqueue_grid_pass(gv_context *h, GridPassJob &job);
int wait_cloud(gv_context *h, CloudSet &C, int k);
int wait_inputs(gv_context *h, CloudSet &C, DetSet &D, int k);
// gv_api_shard.hip
void comm_destroy(gv_context *h);
host::ShardPlan shard_plan(const gv_context *h, int world);
// gv_api_planner.hip
enum : unsigned { kNeedCostmap = 1u, kNeedField = 2u, kNeedRollout = 4u };
int state_error(gv_context *h, const char *call, const char *why);
int refuse_state(gv_context *h, const char *call, const char *missing, unsigned needs, const char *sharded);
int stage_upload(gv_context *h, gv_context::StageSlots &s, const void *src, size_t bytes, size_t cap, void *dst);
int upload_slot(gv_context *h, gv_context::UploadSlots &u, const void *src, size_t bytes, size_t cap);
int wait_scored(gv_context *h, int rc, int32_t K);
int enqueue_control_scores(gv_context *h, const gv_critic_weights &w, gv_control_result *result, uint64_t *totals);
constexpr size_t kNavSeedOff = 512;   // bytes of NavField::stage in front of the seeds: the counters land there
int nav_field_begin(gv_context *h, const char *call, size_t seed_room, NavArgs &a);
int nav_field_relax(gv_context *h, const char *call, NavArgs &a, gv_nav_info *info);

// Where a kernel writes n results bound for `dst`: dst's own device view when it is pinned host memory aligned to
// `align` bytes, else `landing`, which copy_back empties into dst on the public stream behind the kernel.
template <typename T>
struct ResultDest {
  T *dev = nullptr;    // what the kernel is given
  T *host = nullptr;   // non-null: the results land in device memory and are copied here
  size_t n = 0;
  int open(gv_context *h, T *dst, size_t count, size_t align, DevBuf<T> &landing)
  {
    n = count;
    if ((dev = static_cast<T *>(pinned_device_view(dst, align)))) return GV_OK;
    if (int rc = landing.reserve(h, n)) return rc;
    dev = landing;
    host = dst;
    return GV_OK;
  }
  int copy_back(gv_context *h) const
  {
    if (host) GV_HIP(hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    return GV_OK;
  }
};
}  // namespace gv_internal
