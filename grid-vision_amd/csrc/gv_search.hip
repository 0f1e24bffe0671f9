// gv_search.hip -- [EXTENSION] X18 wide-window scan matching by branch and bound (gv_match_search*): the kernels.  The
// definition is in include/gridvision_hip_search.h, the arithmetic in gv_search.hpp and gv_match.hpp (shared with the
// host twin).
//
// On the public stream, behind one memset of the call's block (the counters, the two pre-slots, the bounds) and X16's
// point pass (k_match_points, over its own argument block):
//   k_search_pool_rows / k_search_pool_cols
//                    the separable sliding S x S maximum of the costmap: first along x into `rows`, then along y into
//                    M, aprons of S - 1 cells below index 0 included.  M is in cell order (search_pool_at).  A lane a
//                    byte, S loads each; run per call, so that a call reads the costmap of the inflate before it.
//   k_search_bound   k_match_score's structure over M: a workgroup per (chunk of kMatchChunk points, yaw candidate t,
//                    slice of 256 * KACC blocks).  The lanes rotate and bin the chunk's points into LDS, each with its
//                    kind: every block origin on M, some of them, or none.  Then lanes own blocks, consecutive lanes on
//                    consecutive I (their bytes of M lie S apart), and walk the points by LDS broadcast; the first kind
//                    adds pool[base + off_k] with off_k precomputed, the second tests every origin.  uint32 atomic adds
//                    into B at the end.
//   k_search_seed    the largest search_seed_key over B by a 64-bit atomic maximum, bound_sum by a 64-bit atomic add.
//   k_search_fine    exact scores of listed blocks: a fixed grid loops over (block, chunk of points) items whose number
//                    is read from device memory.  An item bins its chunk under the block's t and adds, per candidate of
//                    the block, the cost bytes under the points: lane = (slice of the points, candidate), the slices'
//                    sums meet in LDS, then one uint32 atomic add a candidate into the block's slot of S * S words.
//                    Run twice: over the seed's and the centre's block into the pre-slots, then over the survivors.
//   k_search_prune   L from the seed's pre-slot; a lane a block: it survives iff B > 0 and B >= L; a wavefront takes
//                    its places in the list with one atomic add and zeroes its survivors' slots, lanes side by side.
//   k_search_select  the largest match_key over the survivors' candidates inside the window, a 64-bit atomic maximum.
//   k_search_record  one thread: the centre candidate joins, the record and the stats are written.
// No kernel waits for another workgroup; only integer atomics; every store is a plain vector store from VGPRs.
// gfx950, wave64.
#include "gv_launch_match.hpp"
#include "gv_device.hpp"

namespace gv {

namespace {
constexpr int kThreads = 256;
constexpr int kFineGrid = 2048;      // workgroups of the fine pass: 8 a CU
constexpr int kReduceGrid = 256;     // workgroups of the seed and select reductions, at most

__device__ __forceinline__ uint64_t *head64(uint32_t *head, int word) { return reinterpret_cast<uint64_t *>(head + word); }   // word even: 8-byte aligned

__device__ __forceinline__ float2 rot_of(int t)
{
  const size_t off = offsetof(SearchArgs, rot) + (size_t)t * 8u;
  return make_float2(load_karg<float>(off), load_karg<float>(off + 4u));
}
}  // namespace

// rows[iy][ix + S - 1] = max over dx of C(ix + dx, iy), -(S-1) <= ix < nx, 0 <= iy < ny
__global__ void __launch_bounds__(kThreads) k_search_pool_rows(SearchArgs a)
{
  const int S = search_s(a.sp), pw = search_pool_w(a.g, S), nx = a.g.nx;
  const int col = (int)(blockIdx.x * (uint32_t)kThreads + threadIdx.x), iy = (int)blockIdx.y;   // iy < ny
  if (col >= pw) return;
  const int ix = col - (S - 1);
  const uint8_t *row = a.cost + (a.g.G - 1 - iy * nx);   // cell (x, iy) is row[-x], 0 <= x < nx
  uint32_t m = 0u;
  for (int dx = 0; dx < S; ++dx) {
    const int x = ix + dx;
    if (x >= 0 && x < nx) m = max(m, (uint32_t)row[-x]);
  }
  a.rows[(size_t)iy * (size_t)pw + (size_t)col] = (uint8_t)m;
}

// pool[iy + S - 1][col] = max over dy of rows[iy + dy][col], -(S-1) <= iy < ny
__global__ void __launch_bounds__(kThreads) k_search_pool_cols(SearchArgs a)
{
  const int S = search_s(a.sp), pw = search_pool_w(a.g, S), ny = a.g.ny;
  const int col = (int)(blockIdx.x * (uint32_t)kThreads + threadIdx.x), r = (int)blockIdx.y;   // r < ny + S - 1
  if (col >= pw) return;
  const int iy = r - (S - 1);
  uint32_t m = 0u;
  for (int dy = 0; dy < S; ++dy) {
    const int y = iy + dy;
    if (y >= 0 && y < ny) m = max(m, (uint32_t)a.rows[(size_t)y * (size_t)pw + (size_t)col]);
  }
  a.pool[(size_t)r * (size_t)pw + (size_t)col] = (uint8_t)m;
}

template <int KACC>
__global__ void __launch_bounds__(kThreads) k_search_bound(SearchArgs a)
{
  __shared__ int2 cell_s[kMatchChunk];
  __shared__ uint8_t kind_s[kMatchChunk];   // 0: adds nothing, 1: every block origin on M, 2: some of them
  const int tid = (int)threadIdx.x;
  const int t = (int)blockIdx.y;            // < NT
  const uint32_t n_used = a.head[kSearchUsed];
  const uint32_t p0 = blockIdx.x * (uint32_t)kMatchChunk;
  if (p0 >= n_used) return;
  const int cnt = (int)min((uint32_t)kMatchChunk, n_used - p0);
  const int lg = a.sp.block_log2, S = 1 << lg, nx = a.g.nx, ny = a.g.ny, pw = search_pool_w(a.g, S);
  const int nbx = search_nbx(a.sp), nby = search_nby(a.sp), nb = nbx * nby;
  const int wx = a.sp.p.wx, wy = a.sp.p.wy;
  const float2 cs = rot_of(t);

  for (int q = tid; q < cnt; q += kThreads) {
    const float2 b = a.pts[p0 + (uint32_t)q];
    int32_t ux = 0, uy = 0;
    uint8_t kind = 0;
    if (match_cell(a.g, a.sp.p, cs.x, cs.y, b.x, b.y, ux, uy)) {   // |ux|, |uy| < 2^30: the sums below stay in int32
      const int x0 = ux - wx, x1 = x0 + ((nbx - 1) << lg), y0 = uy - wy, y1 = y0 + ((nby - 1) << lg);   // the origins' cells
      if (x1 <= -S || y1 <= -S || x0 >= nx || y0 >= ny) kind = 0;
      else kind = (x0 > -S && y0 > -S && x1 < nx && y1 < ny) ? 1 : 2;
    }
    cell_s[q] = make_int2(ux - wx, uy - wy);   // the cell of block (0, 0)'s origin
    kind_s[q] = kind;
  }
  __syncthreads();

  // this lane's blocks; a lane past the last block takes block (0, 0) and writes nothing
  uint32_t acc[KACC];
  int off[KACC], bi[KACC], bj[KACC];
  const int first = (int)blockIdx.z * (kThreads * KACC);
#pragma unroll
  for (int k = 0; k < KACC; ++k) {
    const int b = first + tid + kThreads * k;
    const bool own = b < nb;
    bj[k] = own ? (b / nbx) << lg : 0;
    bi[k] = own ? (b % nbx) << lg : 0;
    off[k] = bj[k] * pw + bi[k];
    acc[k] = 0u;
  }

  const uint8_t *pool = a.pool;
  for (int q = 0; q < cnt; ++q) {
    const int kind = __builtin_amdgcn_readfirstlane((int)kind_s[q]);
    if (kind == 0) continue;
    const int2 u = cell_s[q];
    if (kind == 1) {
      const uint8_t *base = pool + ((size_t)(u.y + S - 1) * (size_t)pw + (size_t)(u.x + S - 1));
#pragma unroll
      for (int k = 0; k < KACC; ++k) acc[k] += (uint32_t)base[off[k]];
    } else {
#pragma unroll
      for (int k = 0; k < KACC; ++k) {
        const int ix = u.x + bi[k], iy = u.y + bj[k];
        if (search_pool_has(a.g, S, ix, iy)) acc[k] += (uint32_t)pool[search_pool_at(a.g, S, ix, iy)];
      }
    }
  }

  uint32_t *B = a.head + kSearchBounds + (size_t)t * (size_t)nb;
#pragma unroll
  for (int k = 0; k < KACC; ++k) {
    const int b = first + tid + kThreads * k;
    if (b < nb && acc[k] != 0u) atomicAdd(&B[b], acc[k]);
  }
}

__global__ void __launch_bounds__(kThreads) k_search_seed(SearchArgs a)
{
  __shared__ uint64_t key_s[kThreads / 64], sum_s[kThreads / 64];
  const int tid = (int)threadIdx.x;
  const uint32_t *B = a.head + kSearchBounds;
  uint64_t best = 0ull, sum = 0ull;
  for (uint32_t b = blockIdx.x * (uint32_t)kThreads + (uint32_t)tid; b < a.n_blocks; b += gridDim.x * (uint32_t)kThreads) {
    const uint32_t v = B[b];
    const uint64_t key = search_seed_key(a.sp, v, b);
    best = key > best ? key : best;
    sum += v;
  }
  best = wave_max64(best);
  sum = wave_sum64(sum);
  if ((tid & 63) == 0) {
    key_s[tid >> 6] = best;
    sum_s[tid >> 6] = sum;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kThreads / 64; ++w) {
      best = key_s[w] > best ? key_s[w] : best;
      sum += sum_s[w];
    }
    atomicMax((unsigned long long *)head64(a.head, kSearchSeedKey), (unsigned long long)best);
    if (sum) atomicAdd((unsigned long long *)head64(a.head, kSearchBoundSum), (unsigned long long)sum);
  }
}

// pre != 0: two blocks, the seed's (read from the seed key) into pre-slot 0 and the centre's into pre-slot 1;
// else the head[kSearchSurvivors] blocks of the list into their slots
__global__ void __launch_bounds__(kThreads) k_search_fine(SearchArgs a, int pre)
{
  __shared__ int2 cell_s[kMatchChunk];
  __shared__ uint8_t ok_s[kMatchChunk];
  __shared__ uint32_t acc_s[kSearchMaxS2];
  const int tid = (int)threadIdx.x;
  const uint32_t n_used = a.head[kSearchUsed];
  const uint32_t n_chunks = (n_used + (uint32_t)kMatchChunk - 1u) / (uint32_t)kMatchChunk;
  const uint32_t n_list = pre ? 2u : a.head[kSearchSurvivors];
  const uint64_t n_items = (uint64_t)n_list * (uint64_t)n_chunks;
  const int lg = a.sp.block_log2, S = 1 << lg, S2 = S * S, nx = a.g.nx, ny = a.g.ny;
  const int cand = tid & (S2 - 1), slice = tid >> (2 * lg), n_slices = kThreads >> (2 * lg);
  const int jj = cand >> lg, ii = cand & (S - 1);
  const int last = a.g.G - 1;
  const uint8_t *cost = a.cost;
  uint32_t *slots = pre ? a.head + kSearchPre : a.slots;
  const size_t slot_words = pre ? (size_t)kSearchMaxS2 : (size_t)S2;

  for (uint64_t it = blockIdx.x; it < n_items; it += gridDim.x) {
    const uint32_t k = (uint32_t)(it / n_chunks), chunk = (uint32_t)(it % n_chunks);
    uint32_t blk;
    if (pre) blk = k == 0u ? search_key_block(*head64(a.head, kSearchSeedKey)) : search_centre_block(a.sp);
    else blk = a.list[k];
    blk = (uint32_t)__builtin_amdgcn_readfirstlane((int)blk);
    if (blk >= a.n_blocks) continue;   // never: the list holds block indices
    int32_t t, J, I;
    search_block_of(a.sp, blk, t, J, I);
    const int jb = search_jb(a.sp, J), ib = search_ib(a.sp, I);
    const float2 cs = rot_of(t);
    const uint32_t p0 = chunk * (uint32_t)kMatchChunk;
    const int cnt = (int)min((uint32_t)kMatchChunk, n_used - p0);

    __syncthreads();   // the item before this one is done with the LDS
    for (int q = tid; q < cnt; q += kThreads) {
      const float2 b = a.pts[p0 + (uint32_t)q];
      int32_t ux = 0, uy = 0;
      uint8_t ok = 0;
      if (match_cell(a.g, a.sp.p, cs.x, cs.y, b.x, b.y, ux, uy)) {
        ux += ib;
        uy += jb;   // the cell under the block's first candidate; the block covers [ux, ux + S) x [uy, uy + S)
        ok = (ux + S > 0 && uy + S > 0 && ux < nx && uy < ny) ? 1 : 0;
      }
      cell_s[q] = make_int2(ux, uy);
      ok_s[q] = ok;
    }
    if (tid < S2) acc_s[tid] = 0u;
    __syncthreads();

    uint32_t acc = 0u;
    for (int q = slice; q < cnt; q += n_slices) {
      if (!ok_s[q]) continue;
      const int2 u = cell_s[q];
      const int ix = u.x + ii, iy = u.y + jj;
      if ((unsigned)ix < (unsigned)nx && (unsigned)iy < (unsigned)ny) acc += (uint32_t)cost[last - (iy * nx + ix)];
    }
    if (acc != 0u) atomicAdd(&acc_s[cand], acc);
    __syncthreads();
    if (tid < S2 && acc_s[tid] != 0u) atomicAdd(&slots[(size_t)k * slot_words + (size_t)tid], acc_s[tid]);
  }
}

__global__ void __launch_bounds__(kThreads) k_search_prune(SearchArgs a)
{
  __shared__ uint32_t lower_s;
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int lg = a.sp.block_log2, S = 1 << lg, S2 = S * S;
  if (tid == 0) lower_s = 0u;
  __syncthreads();
  {   // L: the largest score among the seed's candidates inside the window
    int32_t t, J, I;
    search_block_of(a.sp, search_key_block(*head64(a.head, kSearchSeedKey)), t, J, I);
    if (tid < S2 && (tid >> lg) < search_rows(a.sp, J) && (tid & (S - 1)) < search_cols(a.sp, I)) {
      const uint32_t v = a.head[kSearchPre + tid];
      if (v) atomicMax(&lower_s, v);
    }
  }
  __syncthreads();
  const uint32_t lower = lower_s;
  const uint32_t blk = blockIdx.x * (uint32_t)kThreads + (uint32_t)tid;
  if (blk == 0u) a.head[kSearchLower] = lower;
  bool keep = false;
  uint32_t n_cand = 0u;
  if (blk < a.n_blocks) {
    keep = search_survives(a.head[kSearchBounds + blk], lower);
    if (keep) {
      int32_t t, J, I;
      search_block_of(a.sp, blk, t, J, I);
      n_cand = (uint32_t)(search_rows(a.sp, J) * search_cols(a.sp, I));
    }
  }
  const unsigned long long m = __ballot(keep);
  if (m == 0ull) return;
  const int leader = wave_leader(m);
  const uint32_t total = wave_sum(n_cand);
  uint32_t base = 0u;
  if (lane == leader) {
    base = atomicAdd(&a.head[kSearchSurvivors], (uint32_t)__popcll(m));
    atomicAdd(&a.head[kSearchScored], total);
  }
  base = wave_bcast(base, leader);
  if (keep) a.list[base + wave_rank(m, lane)] = blk;   // < n_survivors <= n_blocks
  // the wavefront's slots are consecutive: base .. base + popcount, S2 words each
  const size_t words = (size_t)__popcll(m) * (size_t)S2;
  uint32_t *z = a.slots + (size_t)base * (size_t)S2;
  for (size_t w = (size_t)lane; w < words; w += 64) z[w] = 0u;
}

__global__ void __launch_bounds__(kThreads) k_search_select(SearchArgs a)
{
  __shared__ uint64_t key_s[kThreads / 64];
  const int tid = (int)threadIdx.x;
  const int lg = a.sp.block_log2, S = 1 << lg;
  const uint32_t total = a.head[kSearchSurvivors] << (2 * lg);   // <= n_blocks * S * S < 2^23
  uint64_t best = 0ull;
  for (uint32_t w = blockIdx.x * (uint32_t)kThreads + (uint32_t)tid; w < total; w += gridDim.x * (uint32_t)kThreads) {
    const uint32_t k = w >> (2 * lg);
    const int c = (int)(w & (uint32_t)(S * S - 1)), jj = c >> lg, ii = c & (S - 1);
    int32_t t, J, I;
    search_block_of(a.sp, a.list[k], t, J, I);
    if (jj >= search_rows(a.sp, J) || ii >= search_cols(a.sp, I)) continue;
    const uint64_t key = match_key(a.slots[w], t - a.sp.p.wt, search_jb(a.sp, J) + jj, search_ib(a.sp, I) + ii,
                                   search_lin(a.sp, t, J, I, jj, ii));
    best = key > best ? key : best;
  }
  best = wave_max64(best);
  if ((tid & 63) == 0) key_s[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kThreads / 64; ++w) best = key_s[w] > best ? key_s[w] : best;
    if (best) atomicMax((unsigned long long *)head64(a.head, kSearchBestKey), (unsigned long long)best);
  }
}

__global__ void __launch_bounds__(64) k_search_record(SearchArgs a)
{
  if (threadIdx.x != 0) return;
  const int lg = a.sp.block_log2, S = 1 << lg;
  const int cj = a.sp.p.wy & (S - 1), ci = a.sp.p.wx & (S - 1);   // the centre inside its block
  const uint32_t guess_score = a.head[kSearchPre + kSearchMaxS2 + cj * S + ci];
  const uint32_t centre = search_centre_lin(a.sp);
  uint64_t best = *head64(a.head, kSearchBestKey);
  const uint64_t ckey = match_key(guess_score, 0, 0, 0, centre);
  best = ckey > best ? ckey : best;
  *a.result = match_record(a.g, a.sp.p, match_key_lin(best), match_key_score(best), guess_score, a.head[kSearchUsed]);
  const uint64_t seed = *head64(a.head, kSearchSeedKey);
  gv_search_stats st;
  st.n_blocks = a.n_blocks;
  st.n_survivors = a.head[kSearchSurvivors];
  st.n_scored = a.head[kSearchScored];
  st.seed_block = search_key_block(seed);
  st.lower_score = a.head[kSearchLower];
  st.bound_max = search_key_bound(seed);
  st.bound_sum = *head64(a.head, kSearchBoundSum);
  *a.stats = st;
}

void launch_search_pool(const SearchArgs &a, hipStream_t s)
{
  const int S = search_s(a.sp);
  const uint32_t gx = ((uint32_t)search_pool_w(a.g, S) + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(k_search_pool_rows, dim3(gx, (uint32_t)a.g.ny), dim3(kThreads), 0, s, a);
  hipLaunchKernelGGL(k_search_pool_cols, dim3(gx, (uint32_t)search_pool_h(a.g, S)), dim3(kThreads), 0, s, a);
}

// the instantiation with up to KACC blocks a lane, and as many slices of blocks as that leaves
void launch_search_bound(const SearchArgs &a, hipStream_t s)
{
  const int nb = search_nbx(a.sp) * search_nby(a.sp);
  const int per_lane = (nb + kThreads - 1) / kThreads;
  const int kacc = per_lane <= 1 ? 1 : per_lane <= 2 ? 2 : per_lane <= 4 ? 4 : 8;
  const dim3 grid((a.n_sel + (uint32_t)kMatchChunk - 1) / (uint32_t)kMatchChunk, (uint32_t)match_nt(a.sp.p),
                  (uint32_t)((nb + kThreads * kacc - 1) / (kThreads * kacc)));
  if (kacc == 1) hipLaunchKernelGGL(k_search_bound<1>, grid, dim3(kThreads), 0, s, a);
  else if (kacc == 2) hipLaunchKernelGGL(k_search_bound<2>, grid, dim3(kThreads), 0, s, a);
  else if (kacc == 4) hipLaunchKernelGGL(k_search_bound<4>, grid, dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL(k_search_bound<8>, grid, dim3(kThreads), 0, s, a);
}

void launch_search_seed(const SearchArgs &a, hipStream_t s)
{
  const uint32_t g = min((a.n_blocks + kThreads - 1) / kThreads, (uint32_t)kReduceGrid);
  hipLaunchKernelGGL(k_search_seed, dim3(g), dim3(kThreads), 0, s, a);
}

void launch_search_fine(const SearchArgs &a, bool pre, hipStream_t s)
{
  hipLaunchKernelGGL(k_search_fine, dim3(pre ? 256 : kFineGrid), dim3(kThreads), 0, s, a, pre ? 1 : 0);
}

void launch_search_prune(const SearchArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL(k_search_prune, dim3((a.n_blocks + kThreads - 1) / kThreads), dim3(kThreads), 0, s, a);
}

void launch_search_select(const SearchArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL(k_search_select, dim3(kReduceGrid), dim3(kThreads), 0, s, a);
  hipLaunchKernelGGL(k_search_record, dim3(1), dim3(64), 0, s, a);
}

}  // namespace gv
