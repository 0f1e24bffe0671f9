// gv_trajscore.hip -- [EXTENSION] X7 trajectory scoring (gv_score_trajectories): the footprint cost of K trajectories
// of P poses against the resident costmap of gv_inflate (include/gridvision_hip.h has the definition).
//
// One workgroup of four wavefronts owns one whole trajectory; it walks the poses in chunks of 64.
//   phase 1  a lane per pose (the first wavefront): cos / sin of the yaw in fp64, the centre and the n vertices through
//            get_index (the exact one, two fp64 divisions a point), their cells and the number of cells of every edge
//            into LDS.  The vertex loop runs over the footprint, which is the same for every lane.  A fiftieth of the
//            kernel's time at the rectangle footprint, so the other three wavefronts wait for it.
//   phase 2  wavefront w takes the chunk's poses w, w + 4, ...: with one wavefront per trajectory 2000 trajectories
//            are two wavefronts per SIMD, and every pose's chain LDS read -> closed form -> cost read lies open (112 us
//            for the 2000 x 56 batch of DESIGN 4.11).  Pose after pose, the wavefront's lanes take the cells of the
//            pose's outline: lane j of a round owns outline cell j, finds its edge among the running totals of the
//            footprint's edges (wave-uniform values in scalar registers: at most 15 compares, no search), evaluates
//            the closed form of grid_map's LineIterator (gv_line.hpp: cell i of a line needs no cell before it; the
//            division is a fp32 reciprocal product with a remainder correction) and reads that cell's cost.  A
//            4.5 m x 2.0 m rectangle on 0.1 m cells is 134 outline cells: three rounds.  No lane walks a line.
//   results  a pose collides when any lane saw a cost >= collision_cost (one ballot); the maximum is kept per lane and
//            reduced once, at the end, by cross-lane shuffles; the cost sum, the off-map count and the first collision
//            are wave-uniform integers.  The four wavefronts' partial records meet in LDS and one thread combines them.
//            Maxima, minima and integer sums only: no order shows.  One 16-byte store per trajectory.  With pose_cost
//            kept the pose's maximum is reduced per pose, staged in LDS and stored a byte per lane after the chunk.
// Memory: consecutive poses of a trajectory are neighbours on the map, so a workgroup's cost reads stay in one
// neighbourhood of the 4 MB layer (L2 / Infinity Cache resident after gv_inflate wrote it).
// Every cell read is inside the map: an on-map pose has every vertex on the map and a line stays inside the bounding
// box of its ends; the read is guarded all the same.
// gfx950, wave64; every store below is a plain vector store from VGPRs.
#include "gv_launch_planner.hpp"
#include "gv_device.hpp"
#include "gv_line.hpp"

namespace gv {

namespace {
constexpr int kChunk = 64;                 // poses per chunk = lanes per wavefront
constexpr int kEdges = 16;                 // most vertices of a footprint
constexpr int kVerts = kEdges + 1;         // LDS cells per pose: the centre and the vertices
constexpr int kWaves = 4;                  // wavefronts per workgroup: they share a chunk's poses

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
}  // namespace

__global__ void __launch_bounds__(256) k_score_trajectories(TrajArgs a)
{
  __shared__ int2 cell_s[kChunk * kVerts];                                          // [pose][centre, vertex 0 .. n-1]
  __shared__ __attribute__((aligned(16))) int32_t ncells_s[kChunk * kEdges];       // [pose][edge]: cells of the edge, 0 past n
  __shared__ uint8_t off_s[kChunk];                                                 // the pose is off the map
  __shared__ uint8_t pcost_s[kChunk];                                               // staged pose costs
  __shared__ int4 part_s[kWaves];                                                   // the wavefronts' partial records
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = (int)blockIdx.x;
  if (k >= a.K) return;
  const int n = a.fp.n_vertices, P = a.P;
  const int nx = a.g.nx, ny = a.g.ny, last = a.g.G - 1;   // last - (iy * nx + ix) is data_entry (gv_types.hpp), G - 1 hoisted
  const float *traj = a.poses + (size_t)k * (size_t)P * 3u;

  if (tid < kChunk) {
#pragma unroll
    for (int e = 0; e < kEdges; ++e) ncells_s[tid * kEdges + e] = 0;   // the entries past n stay zero
  }

  int run_max = 0;                      // per lane: the largest cost this lane has seen
  int first = -1, n_off = 0;            // wave-uniform, over this wavefront's poses
  uint32_t sum = 0;

  for (int p0 = 0; p0 < P; p0 += kChunk) {
    const int cnt = min(kChunk, P - p0);

    // ---- phase 1: lane = pose (tid < cnt <= 64: the first wavefront)
    if (tid < cnt) {
      const float *q = traj + (size_t)(p0 + lane) * 3u;
      const double x = (double)q[0], y = (double)q[1];
      int ix = 0, iy = 0;
      bool ok = get_index(a.g, x, y, ix, iy);
      cell_s[lane * kVerts] = make_int2(ix, iy);
      if (n > 0) {
        double s, c;
        sincos((double)q[2], &s, &c);
        int fx = 0, fy = 0, px = 0, py = 0;
        for (int v = 0; v < n; ++v) {
          const double vx = a.fp.vx[v], vy = a.fp.vy[v];
          const double wx = x + (c * vx - s * vy);
          const double wy = y + (s * vx + c * vy);
          int jx = 0, jy = 0;
          ok = get_index(a.g, wx, wy, jx, jy) & ok;
          cell_s[lane * kVerts + 1 + v] = make_int2(jx, jy);
          if (v == 0) { fx = jx; fy = jy; }
          else ncells_s[lane * kEdges + v - 1] = line_cells(px, py, jx, jy);
          px = jx; py = jy;
        }
        ncells_s[lane * kEdges + n - 1] = line_cells(px, py, fx, fy);   // the closing edge: last vertex -> first
      }
      off_s[lane] = ok ? (uint8_t)0 : (uint8_t)1;
    }
    __syncthreads();

    // ---- phase 2: wavefront = every fourth pose, lane = outline cell
    for (int p = wave; p < cnt; p += kWaves) {
      int m;   // this lane's share of the pose cost
      if (uniform((int)off_s[p])) {
        m = a.fp.off_map_cost;
        sum += (uint32_t)m;
        ++n_off;
      } else {
        const int2 cc = cell_s[p * kVerts];
        m = uniform((int)a.cost[last - (cc.y * nx + cc.x)]);
        sum += (uint32_t)m;
        if (n > 0) {
          const int4 *nc = reinterpret_cast<const int4 *>(&ncells_s[p * kEdges]);
          const int4 n0 = nc[0], n1 = nc[1], n2 = nc[2], n3 = nc[3];
          const int len[kEdges] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w, n2.x, n2.y, n2.z, n2.w, n3.x, n3.y, n3.z, n3.w};
          int end[kEdges];   // end[e]: outline cells up to and including edge e (past n: the total)
          int run = 0;
#pragma unroll
          for (int e = 0; e < kEdges; ++e) { run += uniform(len[e]); end[e] = run; }
          const int total = run;
          for (int j = lane; j < total; j += 64) {
            int e = 0, start = 0;
#pragma unroll
            for (int t = 0; t < kEdges - 1; ++t) {
              if (t >= n - 1) break;                            // scalar: edges past the footprint's cost nothing
              if (j >= end[t]) { e = t + 1; start = end[t]; }   // j < total = end[n-1]: e <= n - 1
            }
            const int e1 = e + 1 == n ? 0 : e + 1;
            const int2 v0 = cell_s[p * kVerts + 1 + e], v1 = cell_s[p * kVerts + 1 + e1];
            int cx, cy;
            line_cell(v0.x, v0.y, v1.x, v1.y, (uint32_t)(j - start), cx, cy);
            if ((unsigned)cx < (unsigned)nx && (unsigned)cy < (unsigned)ny) m = max(m, (int)a.cost[last - (cy * nx + cx)]);
          }
        }
      }
      const bool collides = __ballot(m >= a.fp.collision_cost) != 0ull;
      if (collides && first < 0) first = p0 + p;
      run_max = max(run_max, m);
      if (a.pose_cost) {
        const int pc = wave_max(m);
        if (lane == 0) pcost_s[p] = (uint8_t)pc;
      }
    }
    __syncthreads();   // the pose costs are staged; every lane is done with the chunk's cells
    if (a.pose_cost && tid < cnt) a.pose_cost[(size_t)k * (size_t)P + (size_t)(p0 + tid)] = pcost_s[tid];
    __syncthreads();
  }

  run_max = wave_max(run_max);
  if (lane == 0) part_s[wave] = make_int4(run_max, first, (int)sum, n_off);
  __syncthreads();
  if (tid == 0) {
    int4 r = part_s[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      const int4 q = part_s[w];
      r.x = max(r.x, q.x);
      if (q.y >= 0 && (r.y < 0 || q.y < r.y)) r.y = q.y;
      r.z = (int)((uint32_t)r.z + (uint32_t)q.z);
      r.w += q.w;
    }
    *reinterpret_cast<int4 *>(a.scores + k) = r;
  }
}

void launch_score_trajectories(const TrajArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL(k_score_trajectories, dim3((uint32_t)a.K), dim3(64 * kWaves), 0, s, a);
}

}  // namespace gv
