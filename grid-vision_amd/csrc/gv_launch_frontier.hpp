// gv_launch_frontier.hpp -- launchers of the frontier kernels (gv_frontier.hip); gv_api_frontier.hip calls them.
// Every launcher only enqueues work on `s`; none allocates or synchronises.
#pragma once

#include <hip/hip_runtime.h>

#include "gv_frontier.hpp"
#include "gv_launch_planner.hpp"   // NavArgs, inflate_row_words: the seed kernel is a third one beside k_nav_seeds and k_nav_seeds_path

namespace gv {

// [EXTENSION] X19 frontier clusters.  Everything is in OccupancyGrid.data order, as in X6 and X9.  The frontier bitmap has
// the layout of X6's lethal bitmap (inflate_row_words: a zero guard word, the row's whole words, a zero guard word).
// A workgroup is four wavefronts, a wavefront one bitmap word of one row: workgroup (bx, y) has words 4 bx .. 4 bx + 3 of
// row y, so the workgroups' linear order y * blocks_x + bx is entry order.
constexpr int32_t kFrontierHead = 4;   // words of `head` in front of the per-workgroup counts
struct FrontierArgs {
  GridParams g;
  FrontierRule rule;
  int32_t row_words;            // words per bitmap row, guards included
  int32_t blocks_x, n_blocks;   // workgroups per row, and in all
  int32_t cap;
  uint32_t flags;               // of the call
  const int8_t *i8;             // the packed layer
  const uint8_t *cost;          // G, read when rule.max_cost < 256
  const uint32_t *field;        // G, read with GVX_FRONTIER_USE_FIELD
  unsigned long long *bits;     // ny * row_words words (resident: the seed kernel reads it)
  uint32_t *parent;             // G scratch: union-find parents, then root + n_cells at a root, then the rank at a root
  uint32_t *labels;             // G (resident)
  uint32_t *head;               // [0] frontier cells [1] components [2] clusters [3] largest, then n_blocks counts; zero at the start
  unsigned long long *keys;     // cap * 2: the centre key and the field key of a written cluster
  gvx_frontier_record *rec;            // cap (resident)
  gvx_frontier_info *info;      // one (resident)
  gvx_frontier_record *rec_out;        // the device view of a pinned `out`, or null: written as well
  gvx_frontier_info *info_out;  // the device view of a pinned `info`, or null: written as well
};
void launch_frontier(const FrontierArgs &a, hipStream_t s);   // every kernel of a call, in order
// the seeds of gvx_nav_field_from_frontier: launch_nav_seeds with the cells of written cluster k (-1: of every one)
struct FrontierSeedArgs {
  const unsigned long long *bits;
  int32_t row_words;
  const uint32_t *labels, *rank;   // rank[label]: the cluster's index among the written ones, or GVX_FRONTIER_NONE
  int32_t k;
};
void launch_nav_seeds_frontier(const NavArgs &a, const FrontierSeedArgs &f, hipStream_t s);

}  // namespace gv
