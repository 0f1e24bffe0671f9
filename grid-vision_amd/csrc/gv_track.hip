// gv_track.hip -- [EXTENSION] X14 one update of the tracker over the tick's boxes (gv_track_update): at most 128 tracks
// against at most 128 detections (include/gridvision_hip.h has the definition; the arithmetic is gv_track.hpp's,
// shared with gv_track_step).
//
// One workgroup of four wavefronts does the whole update; nothing waits for another workgroup.  Threads 0..127 are the
// slots ("row" threads: thread s keeps the record of slot s in registers from the load to the store), threads 128..255
// the detections ("column" threads).  In LDS: the detections (10 KB), the positions of the predicted tracks and of the
// detections as four arrays of doubles (4 KB), and seven arrays of 128 ints -- 18 KB in all.
//   steps 1-3  a row thread moves and predicts its track and publishes its position; a column thread loads its
//              detection, tests it and publishes it.
//   step 4     parallel rounds.  A row thread holds the (d2, d)-minimum of its slot over the free valid detections
//              inside the gate, a column thread the (d2, s)-minimum of its detection over the free live slots; ties
//              keep the smaller index, and both call track_d2 with the same arguments, so they see the same doubles.
//              A pair that is the minimum of both is the (d2, s, d)-minimum of every candidate that shares its slot
//              or its detection: the sequential greedy matches it whatever else it does, so all such pairs are
//              matched at once.  A thread's minimum is computed again only when the partner it holds was taken (a
//              minimum changes only when it is removed), and then by its whole wavefront (64 lanes over the 128
//              partners and a shuffle tree, one requester after the other) unless more than 16 of its threads ask at
//              once, which then walk their partners alone, side by side.  The loop has the fixed bound of 128
//              rounds; a round that matches nothing ends it (the smallest remaining candidate is always such a pair,
//              so that happens only when none remains), and 128 rounds that each match a pair have matched every
//              slot.  The exit flag alternates between two LDS words, so the word a round reads is not the one the
//              next round clears; every thread reads the same word after the same barrier and leaves together.
//   steps 5-6  a row thread updates its record from the matched detection, or counts a miss and may free the slot.
//   step 7     ranks by prefix sums (wavefront ballots, the two wavefronts of a half joined through LDS): the j-th
//              unmatched valid detection goes to the j-th free slot with id next_id + j.
//   step 8     the rank among the live slots places a record in `tracks`, the rank among the exported ones its row in
//              X13's object table; the records of `tracks` behind the live ones are zeroed, each index written once.
// Bounds: n is clamped to 0..128 = the LDS rows and the column threads; detection d is read only below n; a slot
//   index is a thread index below 128; of_slot / row_best hold -1 or a detection below n, of_det / col_best -1 or a
//   slot below 128, and are used as indices only when >= 0; a rank is below its total, and every total is at most
//   128 = the rows of `tracks`, of the object table and of unm_list.
// gfx950, wave64; every store below is a plain vector store from VGPRs.
// Behind it: [EXTENSION] X15 k_tick_dets, which leaves a tick's detection list where k_track_update reads it.
#include "gv_launch_planner.hpp"   // TrackArgs
#include "gv_launch_pose.hpp"      // TickDetsArgs, RansacState: k_tick_dets belongs to the pose tick
#include "gv_device.hpp"
#include "gv_track.hpp"

namespace gv {

namespace {
constexpr int kThreads = 2 * kTrackSlots;
constexpr int kRounds = kTrackSlots;
// Up to this many threads of a wavefront that need a new minimum in one round are served by the wavefront together, one
// after the other; more walk alone, side by side.  Measured: a walk alone takes some 17 us whatever the number of lanes,
// serving one thread about 1 us.
constexpr int kServeMax = 16;

// The exclusive prefix of `flag` over the 128 threads of the caller's half (threads 0..127 or 128..255), and the half's
// total.  Every thread of the workgroup calls it; cnt_s is four LDS words, free again on return.
__device__ __forceinline__ int prefix128(bool flag, int tid, int32_t *cnt_s, int &total)
{
  const unsigned long long b = __ballot(flag);
  const int lane = tid & 63, wave = tid >> 6;
  const int below = (int)wave_rank(b, lane);
  if (lane == 0) cnt_s[wave] = __popcll(b);
  __syncthreads();
  const int first = cnt_s[wave & ~1];
  total = first + cnt_s[wave | 1];
  __syncthreads();
  return below + ((wave & 1) ? first : 0);
}
}  // namespace

__global__ void __launch_bounds__(kThreads) k_track_update(TrackArgs a)
{
  __shared__ __attribute__((aligned(16))) gv_lshape_pose det_s[kTrackSlots];
  __shared__ double tx_s[kTrackSlots], ty_s[kTrackSlots], px_s[kTrackSlots], py_s[kTrackSlots];
  __shared__ int32_t live_s[kTrackSlots], valid_s[kTrackSlots];
  __shared__ int32_t of_slot_s[kTrackSlots], of_det_s[kTrackSlots];     // the partner, -1 while free
  __shared__ int32_t row_best_s[kTrackSlots], col_best_s[kTrackSlots];
  __shared__ int32_t unm_list_s[kTrackSlots];
  __shared__ int32_t any_s[2], cnt_s[4], tot_s[4];

  const int tid = (int)threadIdx.x, i = tid & (kTrackSlots - 1);
  const bool row = tid < kTrackSlots;
  const int n = max(0, min(a.n_dev ? *a.n_dev : a.n, kTrackSlots));   // n_dev: a tick's list (X15), whose count the host never learns
  const uint32_t next_id = a.fresh ? 1u : a.state->next_id;

  // ---- steps 1 to 3
  gv_track t = {};
  bool live = false, valid = false;
  if (row) {
    live = !a.fresh && a.state->live[i] != 0;
    if (live) {
      t = a.state->t[i];
      if (a.ego.on) track_move(a.ego, t);
      track_predict(a.p, a.dt, t);
    }
    tx_s[i] = t.x;
    ty_s[i] = t.y;
    live_s[i] = live ? 1 : 0;
    of_slot_s[i] = -1;
  } else {
    gv_lshape_pose z = {};
    if (i < n) {
      z = a.dets[i];
      valid = track_det_valid(z);
    }
    det_s[i] = z;
    px_s[i] = z.px;
    py_s[i] = z.py;
    valid_s[i] = valid ? 1 : 0;
    of_det_s[i] = -1;
  }
  if (tid < 2) any_s[tid] = 0;
  __syncthreads();

  // ---- step 4
  {
    const double gate2 = a.p.gate2;
    const double mx = row ? tx_s[i] : px_s[i], my = row ? ty_s[i] : py_s[i];
    const int32_t *partner_ok = row ? valid_s : live_s, *partner_of = row ? of_det_s : of_slot_s;
    const int m = row ? n : kTrackSlots;
    const int lane = tid & 63;
    bool active = row ? live : valid;   // may still have a candidate
    int best = -1;                      // the minimum of this row / column over the free partners, while it is free
    for (int r = 0; r < kRounds; ++r) {
      // A few threads whose partner was taken are served one after the other by their whole wavefront (a wavefront is
      // all slots or all detections): lane l tests partners l and l + 64 of the requester, a shuffle tree takes the
      // lexicographic (d2, index) minimum.  `todo` is the same in every lane, so the wavefront stays together.
      const bool need = active && (best < 0 || partner_of[best] >= 0);
      unsigned long long todo = __ballot(need);
      if (__popcll(todo) > kServeMax) {
        // many at once (the first round): every thread walks its own partners, all lanes side by side
        todo = 0ull;
        if (need) {
          best = -1;
          double best_d2 = 0.0;
          for (int j = 0; j < m; ++j) {
            const bool free_j = partner_ok[j] != 0 && partner_of[j] < 0;
            const double d2 = row ? track_d2(mx, my, px_s[j], py_s[j]) : track_d2(tx_s[j], ty_s[j], mx, my);
            if (free_j && d2 <= gate2 && (best < 0 || d2 < best_d2)) {   // ascending j, strict <
              best = j;
              best_d2 = d2;
            }
          }
          if (best < 0) active = false;
        }
      }
      while (todo) {
        const int src = wave_leader(todo);
        todo &= todo - 1;
        const double qx = wave_bcast(mx, src), qy = wave_bcast(my, src);
        int bj = -1;
        double bd = 0.0;
        for (int j = lane; j < m; j += 64) {
          const bool free_j = partner_ok[j] != 0 && partner_of[j] < 0;
          const double d2 = row ? track_d2(qx, qy, px_s[j], py_s[j]) : track_d2(tx_s[j], ty_s[j], qx, qy);
          if (free_j && d2 <= gate2 && (bj < 0 || d2 < bd)) {
            bj = j;
            bd = d2;
          }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
          const double od = __shfl_xor(bd, o, 64);
          const int oj = __shfl_xor(bj, o, 64);
          if (oj >= 0 && (bj < 0 || od < bd || (od == bd && oj < bj))) {
            bj = oj;
            bd = od;
          }
        }
        if (lane == src) {
          best = bj;
          if (bj < 0) active = false;
        }
      }
      (row ? row_best_s : col_best_s)[i] = active ? best : -1;
      __syncthreads();
      if (tid == 0) any_s[(r + 1) & 1] = 0;
      if (row && active && col_best_s[best] == i) {
        of_slot_s[i] = best;
        of_det_s[best] = i;
        any_s[r & 1] = 1;
        active = false;
      }
      __syncthreads();
      if (!row && active && of_det_s[i] >= 0) active = false;
      if (!any_s[r & 1]) break;
    }
  }

  // ---- steps 5 and 6
  bool matched = false, freed = false;
  if (row && live) {
    const int d = of_slot_s[i];
    if (d >= 0) {
      track_match(a.p, det_s[d], d, t);
      matched = true;
    } else if (track_miss(a.p, t)) {
      live = false;
      freed = true;
    }
  }

  // ---- step 7
  int tot = 0;
  const bool is_free = row && !live, is_unm = !row && valid && of_det_s[i] < 0;
  int rank = prefix128(row ? is_free : is_unm, tid, cnt_s, tot);
  if (is_unm) unm_list_s[rank] = i;
  if (i == 0) tot_s[row ? 0 : 1] = tot;
  __syncthreads();
  const int n_free = tot_s[0], n_unm = tot_s[1];
  const int n_born = min(n_free, n_unm);
  if (is_free && rank < n_unm) {
    const int d = unm_list_s[rank];
    t = track_birth(a.p, det_s[d], d, next_id + (uint32_t)rank, i);
    live = true;
  }

  // ---- step 8 and the counts
  int n_tracks = 0, n_exported = 0, n_confirmed = 0, n_matched = 0, n_deleted = 0, n_invalid = 0;
  const bool exported = row && live && track_exported(a.p, t);
  const int rank_live = prefix128(row && live, tid, cnt_s, n_tracks);
  const int rank_exp = prefix128(exported, tid, cnt_s, n_exported);
  (void)prefix128(row ? (live && track_confirmed(a.p, t)) : (i < n && !valid), tid, cnt_s, tot);
  if (row) n_confirmed = tot;
  else if (i == 0) tot_s[2] = tot;
  (void)prefix128(matched, tid, cnt_s, n_matched);
  (void)prefix128(freed, tid, cnt_s, n_deleted);
  __syncthreads();
  n_invalid = tot_s[2];

  if (row) {
    a.state->live[i] = live ? 1 : 0;
    if (live) a.state->t[i] = t;
    if (a.tracks) {
      if (live) a.tracks[rank_live] = t;
      if (i >= n_tracks) a.tracks[i] = gv_track{};
    }
    if (a.feed_objs && exported) a.feed_objs[rank_exp] = dyn_object(track_export(a.p, t));
    if (i == 0) {
      const uint32_t id_after = next_id + (uint32_t)n_born;
      a.state->next_id = id_after;
      a.state->reserved = 0u;
      if (a.feed_n) *a.feed_n = n_exported;
      if (a.info) {
        gv_track_info f;
        f.n_tracks = n_tracks; f.n_confirmed = n_confirmed; f.n_exported = n_exported;
        f.n_matched = n_matched; f.n_born = n_born; f.n_deleted = n_deleted;
        f.n_dropped = n_unm - n_born; f.n_invalid = n_invalid;
        f.next_id = id_after; f.reserved = 0u;
        *a.info = f;
      }
    }
  }
}

// ---- [EXTENSION] X15 the tick's detection list (GV_TICK_KEEP_DETS) ----
// One workgroup of four wavefronts walks the candidates in chunks of 256, thread t of a chunk owning candidate c0 + t.
// A candidate that tick_det_take keeps gets its rank by an ordered compaction: the wavefront's ballot gives the kept
// lanes below it, four LDS words the kept candidates of the wavefronts before it, `base` those of the chunks before.  The
// owner of a kept candidate of rank < 128 builds the camera-frame pose, moves it to the base frame (gv_pose_math.hpp:
// the host's text) and stores the record's 80 bytes as five 16-byte vector stores; ranks from 128 on are only counted.
// The records behind the last one are zeroed, so every byte of the list is written by every launch.
// Bounds: c < n_cand <= kTickDetCandidates indexes vout / cam / valid; rank < kTickDets indexes out->p; the zeroing
// runs over [n, kTickDets).  cnt_s is double-buffered by the chunk's parity: one barrier per chunk.
namespace {
constexpr int kDetThreads = 256;

__device__ __forceinline__ void store_pose(gv_lshape_pose *dst, const gv_lshape_pose &p)
{
  static_assert(sizeof(gv_lshape_pose) == 80, "five double2");
  double2 *d = reinterpret_cast<double2 *>(dst);
  d[0] = make_double2(p.px, p.py);
  d[1] = make_double2(p.pz, p.qx);
  d[2] = make_double2(p.qy, p.qz);
  d[3] = make_double2(p.qw, p.length);
  d[4] = make_double2(p.width, p.height);
}
}  // namespace

__global__ void __launch_bounds__(kDetThreads) k_tick_dets(TickDetsArgs a)
{
  __shared__ int32_t cnt_s[2][kDetThreads / 64];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_cand = a.mode == kTickDetsNone ? 0 : max(0, min(a.n_cand, kTickDetCandidates));
  bool empty = false;
  if (a.mode == kTickDetsPca) {
    const RansacState st = *a.st;
    empty = tick_dets_empty(st.best_count, st.n_inliers, a.n_cloud);
  }
  int base = 0;
  for (int c0 = 0, it = 0; c0 < n_cand; c0 += kDetThreads, ++it) {
    const int c = c0 + tid;
    int32_t valid = 0;
    if (c < n_cand) valid = a.mode == kTickDetsVision ? a.vout[c].valid : (int32_t)a.valid[c];
    const bool take = c < n_cand && tick_det_take(empty, valid);
    const unsigned long long b = __ballot(take);
    if (lane == 0) cnt_s[it & 1][wave] = __popcll(b);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kDetThreads / 64; ++w) {
      const int k = cnt_s[it & 1][w];
      before += w < wave ? k : 0;
      total += k;
    }
    const int rank = base + before + (int)wave_rank(b, lane);
    if (take && rank < kTickDets) {
      gv_lshape_pose p;
      if (a.mode == kTickDetsVision) {
        const VisionOut vo = a.vout[c];
        double sp, cp;
        sincos((double)(-vo.orient) * 0.5, &sp, &cp);
        p = tick_vision_pose(vo, cp, sp);
      } else
        p = a.cam[c];
      store_pose(a.out->p + rank, tick_det_record(a.tf_bc, p));
    }
    base += total;
  }
  const int n = min(base, kTickDets);
  for (int i = n * 5 + tid; i < kTickDets * 5; i += kDetThreads) reinterpret_cast<double2 *>(a.out->p)[i] = make_double2(0.0, 0.0);
  if (tid == 0) {
    a.out->n = n;
    a.out->n_total = base;
    a.out->pad[0] = a.out->pad[1] = 0;
  }
}

void launch_tick_dets(const TickDetsArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL(k_tick_dets, dim3(1), dim3(kDetThreads), 0, s, a);
}

void launch_track_update(const TrackArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL(k_track_update, dim3(1), dim3(kThreads), 0, s, a);
}

}  // namespace gv
