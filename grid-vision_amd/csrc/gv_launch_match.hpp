// gv_launch_match.hpp -- launchers of the two scan matchers' kernels (gv_match.hip, gv_search.hip); gv_api_match.hip
// calls them.
// Every launcher only enqueues work on `s`; none allocates or synchronises.
#pragma once

#include <hip/hip_runtime.h>

#include "gv_types.hpp"
#include "gv_match.hpp"    // MatchParams, kMatchMaxSide
#include "gv_search.hpp"   // SearchParams, kSearchMaxS2

namespace gv {

// [EXTENSION] X16 scan-to-costmap matching (gv_match.hip; the arithmetic is gv_match.hpp's).  The configuration, the
// guess and the host-built rotation table travel by value: a call already enqueued keeps what it was enqueued with.
// `head` is one zeroed block per call: word 0 counts the used points, the volume starts at word kMatchHeadWords.
// The point pass (k_match_points) is the one kernel that reads the cloud, and both matchers run it: it has an argument
// block of its own, over the calling matcher's `pts` and the counter word of its `head`.
struct MatchPointsArgs {
  Mat34f m_base;
  HeightBand band;
  const float *x, *y, *z;       // the resident cloud (device)
  uint32_t n;                   // its points
  uint32_t n_sel;               // ceil(n / stride): the selected ones, point sel * stride each
  int32_t stride;
  uint32_t use_band;
  float2 *pts;                  // n_sel pairs (device): the used points' (bx, by), in any order
  uint32_t *used;               // their count (device), zero when the pass starts
};
void launch_match_points(const MatchPointsArgs &a, hipStream_t s);
constexpr int32_t kMatchHeadWords = 4;
struct MatchArgs {
  GridParams g;
  MatchParams p;
  uint32_t n_sel;               // ceil(n / stride): the bound on the used points
  const float2 *pts;            // the used points' (bx, by) (device)
  uint32_t *head;               // kMatchHeadWords + NT*NY*NX words (device), zero when the point pass starts
  const uint8_t *cost;          // the resident costmap
  gv_match_result *result;      // one record (device memory, or the device view of pinned host memory; 8-byte aligned)
  uint32_t *scores_out;         // null, or the device view of a pinned destination of the volume
  float rot[2 * kMatchMaxSide]; // (c_t, s_t), NT pairs
};
void launch_match_score(const MatchArgs &a, hipStream_t s);
void launch_match_select(const MatchArgs &a, hipStream_t s);
// [EXTENSION] X18 wide-window matching by branch and bound (gv_search.hip; the arithmetic is gv_search.hpp's and
// gv_match.hpp's).  The point pass is X16's, given a MatchPointsArgs over this call's `head` and `pts`.  `head` is one zeroed
// block per call: the counters below, the two pre-slots (the seed block's exact scores, then the centre block's), then
// the bounds B[n_blocks].
enum : int32_t {
  kSearchUsed = 0,        // n_used (the point pass counts here)
  kSearchSurvivors = 1,   // n_survivors
  kSearchScored = 2,      // n_scored
  kSearchLower = 3,       // L
  kSearchSeedKey = 4,     // uint64: the largest search_seed_key
  kSearchBoundSum = 6,    // uint64
  kSearchBestKey = 8,     // uint64: the largest match_key over the survivors' candidates
  kSearchPre = 16,        // 2 * kSearchMaxS2 words
  kSearchBounds = kSearchPre + 2 * kSearchMaxS2,
};
struct SearchArgs {
  GridParams g;
  SearchParams sp;
  uint32_t n_sel;               // ceil(n / stride): the bound on the used points
  uint32_t n_blocks;
  const float2 *pts;            // the used points' (bx, by) (device)
  uint32_t *head;               // kSearchBounds + n_blocks words (device), zero when the point pass starts
  const uint8_t *cost;          // the resident costmap
  uint8_t *rows;                // ny rows of nx + S - 1: the costmap pooled along x
  uint8_t *pool;                // M: (ny + S - 1) rows of nx + S - 1 (search_pool_at)
  uint32_t *list;               // n_blocks words: the survivors' block indices, in any order
  uint32_t *slots;              // n_blocks * S * S words: slot k holds the exact scores of list[k]'s block
  gv_match_result *result;      // one record (device memory, or the device view of pinned host memory)
  gv_search_stats *stats;       // likewise
  float rot[2 * kMatchMaxSide]; // (c_t, s_t), NT pairs
};
void launch_search_pool(const SearchArgs &a, hipStream_t s);
void launch_search_bound(const SearchArgs &a, hipStream_t s);
void launch_search_seed(const SearchArgs &a, hipStream_t s);
void launch_search_fine(const SearchArgs &a, bool pre, hipStream_t s);   // pre: the seed's and the centre's block
void launch_search_prune(const SearchArgs &a, hipStream_t s);
void launch_search_select(const SearchArgs &a, hipStream_t s);

}  // namespace gv
