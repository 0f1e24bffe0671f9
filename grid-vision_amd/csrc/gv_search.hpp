// gv_search.hpp -- [EXTENSION] X18 wide-window scan matching by branch and bound (gv_match_search*): the arithmetic of
// the definition in include/gridvision_hip_search.h that X16's text (gv_match.hpp) does not already give -- the block
// geometry, the pooled costmap's layout and value, the seed's key, the survivor predicate and the stats -- one text for
// the kernels (gv_search.hip) and for the host twin (gv_match_search_host, gv_api_match_host.hip).  Plain C++ under GV_HD;
// built with -ffp-contract=off like its siblings.
#pragma once

#include "../../include/gridvision_hip_search.h"
#include "gv_match.hpp"

namespace gv {

constexpr int32_t kSearchMaxHalf = 128;                 // wx, wy
constexpr int32_t kSearchMaxBlockLog2 = 4;              // S <= 16
constexpr int32_t kSearchMaxS2 = 1 << (2 * kSearchMaxBlockLog2);   // candidates of a block, at most

// configuration + guess as a call carries them: X16's parameters (wx, wy up to 128) and the block's size
struct SearchParams {
  MatchParams p;
  int32_t block_log2;
  int32_t pad;
};

GV_HD int32_t search_s(const SearchParams &sp) { return 1 << sp.block_log2; }
GV_HD int32_t search_nbx(const SearchParams &sp) { return (match_nx(sp.p) + search_s(sp) - 1) >> sp.block_log2; }
GV_HD int32_t search_nby(const SearchParams &sp) { return (match_ny(sp.p) + search_s(sp) - 1) >> sp.block_log2; }
GV_HD uint32_t search_blocks(const SearchParams &sp) { return (uint32_t)(match_nt(sp.p) * search_nby(sp) * search_nbx(sp)); }

// block index -> (t, J, I)
GV_HD void search_block_of(const SearchParams &sp, uint32_t blk, int32_t &t, int32_t &J, int32_t &I)
{
  const uint32_t nbx = (uint32_t)search_nbx(sp), per_t = nbx * (uint32_t)search_nby(sp);
  t = (int32_t)(blk / per_t);
  const uint32_t r = blk % per_t;
  J = (int32_t)(r / nbx);
  I = (int32_t)(r % nbx);
}
// a block's origin and the number of its candidates the window holds, per axis
GV_HD int32_t search_jb(const SearchParams &sp, int32_t J) { return -sp.p.wy + (J << sp.block_log2); }
GV_HD int32_t search_ib(const SearchParams &sp, int32_t I) { return -sp.p.wx + (I << sp.block_log2); }
GV_HD int32_t search_rows(const SearchParams &sp, int32_t J)
{
  const int32_t left = match_ny(sp.p) - (J << sp.block_log2), S = search_s(sp);
  return left < S ? left : S;
}
GV_HD int32_t search_cols(const SearchParams &sp, int32_t I)
{
  const int32_t left = match_nx(sp.p) - (I << sp.block_log2), S = search_s(sp);
  return left < S ? left : S;
}

// The pooled costmap M as it is stored: row (iy + S - 1) of width nx + S - 1, column (ix + S - 1), in cell order (not
// the data order of the costmap), so that the aprons below index 0 are rows and columns like the others.
GV_HD int32_t search_pool_w(const GridParams &g, int32_t S) { return g.nx + S - 1; }
GV_HD int32_t search_pool_h(const GridParams &g, int32_t S) { return g.ny + S - 1; }
GV_HD bool search_pool_has(const GridParams &g, int32_t S, int32_t ix, int32_t iy)
{
  return ix > -S && iy > -S && ix < g.nx && iy < g.ny;
}
GV_HD size_t search_pool_at(const GridParams &g, int32_t S, int32_t ix, int32_t iy)
{
  return (size_t)(iy + S - 1) * (size_t)search_pool_w(g, S) + (size_t)(ix + S - 1);
}
// M(ix, iy), 0 where it has no cell
GV_HD uint32_t search_pooled(const GridParams &g, int32_t S, const uint8_t *pool, int32_t ix, int32_t iy)
{
  return search_pool_has(g, S, ix, iy) ? (uint32_t)pool[search_pool_at(g, S, ix, iy)] : 0u;
}

// The seed's order as one 64-bit key, larger is better: the bound, then the smaller Chebyshev distance from the block
// that holds the centre (<= 128), then the smaller block index (< 65 * 129 * 129 < 2^24).
GV_HD uint64_t search_seed_key(const SearchParams &sp, uint32_t bound, uint32_t blk)
{
  int32_t t, J, I;
  search_block_of(sp, blk, t, J, I);
  const int32_t dt = t - sp.p.wt, dj = J - (sp.p.wy >> sp.block_log2), di = I - (sp.p.wx >> sp.block_log2);
  const int32_t a = dt < 0 ? -dt : dt, b = dj < 0 ? -dj : dj, c = di < 0 ? -di : di;
  const int32_t cheb = a > b ? (a > c ? a : c) : (b > c ? b : c);
  return ((uint64_t)bound << 32) | ((uint64_t)(255 - cheb) << 24) | (uint64_t)(0xFFFFFFu - blk);
}
GV_HD uint32_t search_key_block(uint64_t key) { return 0xFFFFFFu - (uint32_t)(key & 0xFFFFFFu); }
GV_HD uint32_t search_key_bound(uint64_t key) { return (uint32_t)(key >> 32); }

// a block is scored exactly: >=, not >, since an equal score nearer the centre may sit in another block
GV_HD bool search_survives(uint32_t bound, uint32_t lower) { return bound > 0u && bound >= lower; }

// the linear index (X16's) of candidate (jj, ii) of block (t, J, I); the caller has checked jj < rows, ii < cols
GV_HD uint32_t search_lin(const SearchParams &sp, int32_t t, int32_t J, int32_t I, int32_t jj, int32_t ii)
{
  return (uint32_t)((t * match_ny(sp.p) + ((J << sp.block_log2) + jj)) * match_nx(sp.p) + ((I << sp.block_log2) + ii));
}
GV_HD uint32_t search_centre_lin(const SearchParams &sp)
{
  return (uint32_t)((sp.p.wt * match_ny(sp.p) + sp.p.wy) * match_nx(sp.p) + sp.p.wx);
}
GV_HD uint32_t search_centre_block(const SearchParams &sp)
{
  return (uint32_t)((sp.p.wt * search_nby(sp) + (sp.p.wy >> sp.block_log2)) * search_nbx(sp) + (sp.p.wx >> sp.block_log2));
}

}  // namespace gv
