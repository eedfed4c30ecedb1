// dmf_travel.hip — the travel field over a distance field of the fused grid:
// hops[x][y][z] = the least number of face-to-face steps from any seed cell through cells whose
// clearance dist2 >= radius2, DMF_NO_PATH where there is no such path; and the path back from a
// cell.  Every update is a min over valid path lengths, so the fixpoint is the BFS distance whatever
// the order in which tiles are relaxed.  The work representation is the output itself: hops is
// filled with DMF_NO_PATH, the seeds get 0, and the rounds lower values in place.  Kernels:
//  k_tr_mask   — tile_mask_pass<1> over the uint32 field: the traversable mask in the occupancy
//                layout (dmf_gridbits.hpp), one word per workgroup of its tile level ("holds a
//                traversable cell"), and the traversable count;
//  k_tr_seed   — one lane per seed: a seed inside the grid on a traversable cell gets 0 and puts its
//                tile on the first active list;
//  k_tr_round  — one round = one launch.  A workgroup of one wave takes the tiles of the active
//                list in turn (a fixed grid strides over the list, whose length is a device
//                counter).  Lane (x, y) of a tile holds the 8 z-cells of its row in registers; the
//                rows and the four x / y halo faces lie in LDS, the two z halo cells in registers.
//                The tile is relaxed to its local fixpoint (a sweep up and down z in registers,
//                one step across x and y per iteration), the lowered cells are stored, and every
//                face neighbour across which a cell changed is put on the next round's list once
//                (an atomic OR on its "queued" bit decides who appends it).  A tile has one writer
//                per round; a neighbour that reads a halo cell while it is being lowered reads an
//                upper bound either way and is activated for the next round.  No workgroup waits
//                for another;
//  k_tr_finish — one streaming pass over hops: the reached cells and the largest finite value;
//  k_tr_gather — one row of the travel cost map: the hop counts at V cells, INT_MAX for no path;
//  k_tr_path   — one lane walks target -> seed: from value k to the first face neighbour, in the
//                order -x +x -y +y -z +z, that holds k - 1.
// The host reads the next list's length after a batch of kTrBatch rounds and stops at an empty
// list; T + 2 rounds (T = the traversable cells) bound the loop: a cell whose shortest path crosses
// k tile faces is final after round k, and k < T.
#include <algorithm>
#include <climits>

#include "dmf_host.hpp"

namespace dmf {

constexpr uint32_t kTrNone = 0xffffffffu;
static_assert(kTrNone == DMF_NO_PATH, "an unreached cell of the work representation already is the result");
constexpr int kTrRoundWgs = 2048;  // workgroups of a round: 8 waves per CU stride over the active list
constexpr int kTrBatch = 32;       // rounds between two reads of the list length
constexpr int kTrCtlWords = 8;     // uint64 {traversable, reached, max hops, tile activations, cell updates, rounds with work, -, -}
constexpr size_t kTrCtlBytes = sizeof(uint64_t) * kTrCtlWords + sizeof(uint32_t) * 4;  // ... then the 4 list lengths

__global__ __launch_bounds__(kMaskThreads) void k_tr_mask(Geom g, GridTiles tl, const uint32_t* __restrict__ dist2,
                                                          uint32_t radius2, uint32_t* __restrict__ fine,
                                                          uint32_t* __restrict__ coarse,
                                                          unsigned long long* __restrict__ ntrav) {
  __shared__ uint32_t sany[16];
  __shared__ uint32_t scount;
  uint32_t* const out[1] = {fine};
  uint32_t word[1];
  if (threadIdx.x == 0) scount = 0;  // (tile_mask_pass holds the barrier that orders this)
  tile_mask_pass<1>(g, tl, dist2, out, word,
                    [=](uint32_t d, int k, uint32_t (&b)[1]) { b[0] |= (uint32_t)(d >= radius2) << k; });
  // a wave holds words 2k (lanes 0-31) and 2k + 1 (lanes 32-63) of the 32 tiles
  const int i = threadIdx.x, w = i >> 5;
  const uint64_t any = __builtin_amdgcn_ballot_w64(word[0] != 0u);
  uint32_t c = (uint32_t)__popc(word[0]);
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
  if ((i & 63) == 0) {
    sany[w] = (uint32_t)any;
    sany[w + 1] = (uint32_t)(any >> 32);
    if (c) atomicAdd(&scount, c);
  }
  __syncthreads();
  if (i == 0) {
    uint32_t a = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) a |= sany[k];
    coarse[blockIdx.x] = a;
    if (scount) atomicAdd(ntrav, (unsigned long long)scount);
  }
}

// Tile t onto a list unless its queued bit says it is there already.
__device__ inline void tr_enqueue(uint32_t t, uint32_t* __restrict__ list, uint32_t* __restrict__ queued,
                                  uint32_t* __restrict__ count) {
  const uint32_t m = 1u << (t & 31u);
  if (!(atomicOr(&queued[t >> 5], m) & m)) list[atomicAdd(count, 1u)] = t;
}

__global__ __launch_bounds__(64) void k_tr_seed(Geom g, GridTiles tl, const uint32_t* __restrict__ fine,
                                                const int32_t* __restrict__ seeds, int64_t n,
                                                uint32_t* __restrict__ hops, uint32_t* __restrict__ list,
                                                uint32_t* __restrict__ queued, uint32_t* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const int x = seeds[3 * i], y = seeds[3 * i + 1], z = seeds[3 * i + 2];
  if (x < 0 || y < 0 || z < 0 || x >= g.n[0] || y >= g.n[1] || z >= g.n[2]) return;
  const uint32_t bit = occ_index(tl.nty, tl.ntz, x, y, z);
  if (!((fine[bit >> 5] >> (bit & 31u)) & 1u)) return;
  hops[((int64_t)x * g.n[1] + y) * g.n[2] + z] = 0;
  tr_enqueue(bit >> 9, list, queued, count);
}

// Round r: the tiles cur[0 .. count[r & 3]) -> next, count[(r + 1) & 3]; count[(r + 2) & 3], which
// no workgroup of this round reads or adds to, is zeroed for the round after the next.  qcur holds
// the queued bits of cur (cleared here, tile by tile), qnext those of next.  *worked = r + 1 when
// the round has a tile.
__global__ __launch_bounds__(64) void k_tr_round(Geom g, GridTiles tl, const uint32_t* __restrict__ fine,
                                                 const uint32_t* __restrict__ coarse, uint32_t* hops,
                                                 const uint32_t* __restrict__ cur, uint32_t* __restrict__ next,
                                                 uint32_t* __restrict__ qcur, uint32_t* __restrict__ qnext,
                                                 uint32_t* count, uint32_t r, unsigned long long* __restrict__ worked,
                                                 unsigned long long* __restrict__ stats) {
  // rows s[x + 1][y + 1][z] of the tile and of its x / y halo (the corners are never read)
  __shared__ __attribute__((aligned(16))) uint32_t s[10][10][8];
  const int l = threadIdx.x, lx = l >> 3, ly = l & 7;
  const uint32_t n = count[r & 3u];
  if (blockIdx.x == 0 && l == 0) {
    count[(r + 2u) & 3u] = 0;
    if (n) *worked = r + 1ull;
  }
  const int nx = g.n[0], ny = g.n[1], nz = g.n[2];
  // a full row of 8 cells is two 16-B accesses when every row starts on 16 B
  const bool aligned = ((uintptr_t)hops & 15) == 0 && (nz & 3) == 0;
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t t = cur[i];
    const int tz = (int)(t % tl.ntz), ty = (int)((t / tl.ntz) % tl.nty), tx = (int)((t / tl.ntz) / tl.nty);
    const int X0 = tx * 8, Y0 = ty * 8, Z0 = tz * 8, X = X0 + lx, Y = Y0 + ly;
    if (l == 0) atomicAnd(&qcur[t >> 5], ~(1u << (t & 31u)));
    // the lane's 8 traversable bits: byte y & 3 of word 2 x + (y >> 2); none past the grid
    const uint32_t m = (fine[(size_t)t * 16 + 2 * lx + (ly >> 2)] >> (8 * (ly & 3))) & 0xffu;
    const int64_t base = ((int64_t)X * ny + Y) * nz + Z0;  // (only dereferenced inside the grid)
    const bool in_xy = X < nx && Y < ny, wide = m == 0xffu && aligned;
    uint32_t v[8], old[8];
    if (wide) {
      const uint4 q0 = *(const uint4*)(hops + base), q1 = *(const uint4*)(hops + base + 4);
      v[0] = q0.x; v[1] = q0.y; v[2] = q0.z; v[3] = q0.w;
      v[4] = q1.x; v[5] = q1.y; v[6] = q1.z; v[7] = q1.w;
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = (m >> k) & 1u ? hops[base + k] : kTrNone;
    }
    const uint32_t zlo = in_xy && Z0 > 0 ? hops[base - 1] : kTrNone;
    const uint32_t zhi = in_xy && Z0 + 8 < nz ? hops[base + 8] : kTrNone;
    // the four halo faces, 64 cells each: lane (a, b) reads (a along the face, z = Z0 + b)
    const int fz = Z0 + ly, fa = lx;
    const bool fzin = fz < nz;
    __syncthreads();  // the previous tile's reads of s are done
    s[0][fa + 1][ly] = X0 > 0 && Y0 + fa < ny && fzin ? hops[((int64_t)(X0 - 1) * ny + Y0 + fa) * nz + fz] : kTrNone;
    s[9][fa + 1][ly] = X0 + 8 < nx && Y0 + fa < ny && fzin ? hops[((int64_t)(X0 + 8) * ny + Y0 + fa) * nz + fz] : kTrNone;
    s[fa + 1][0][ly] = Y0 > 0 && X0 + fa < nx && fzin ? hops[((int64_t)(X0 + fa) * ny + Y0 - 1) * nz + fz] : kTrNone;
    s[fa + 1][9][ly] = Y0 + 8 < ny && X0 + fa < nx && fzin ? hops[((int64_t)(X0 + fa) * ny + Y0 + 8) * nz + fz] : kTrNone;
    uint4* const mine = (uint4*)&s[lx + 1][ly + 1][0];
    mine[0] = make_uint4(v[0], v[1], v[2], v[3]);
    mine[1] = make_uint4(v[4], v[5], v[6], v[7]);
#pragma unroll
    for (int k = 0; k < 8; ++k) old[k] = r ? v[k] : kTrNone;  // (round 0: the seeds' zeros are new to every neighbour)
    for (;;) {
      __syncthreads();  // the rows are written
      uint32_t nb[8];
      {
        const uint4* const xm = (const uint4*)&s[lx][ly + 1][0];
        const uint4* const xp = (const uint4*)&s[lx + 2][ly + 1][0];
        const uint4* const ym = (const uint4*)&s[lx + 1][ly][0];
        const uint4* const yp = (const uint4*)&s[lx + 1][ly + 2][0];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const uint4 a = xm[h], b = xp[h], c = ym[h], d = yp[h];
          nb[4 * h] = min(min(a.x, b.x), min(c.x, d.x));
          nb[4 * h + 1] = min(min(a.y, b.y), min(c.y, d.y));
          nb[4 * h + 2] = min(min(a.z, b.z), min(c.z, d.z));
          nb[4 * h + 3] = min(min(a.w, b.w), min(c.w, d.w));
        }
      }
      bool ch = false;
      uint32_t prev = zlo;  // up z: the x / y neighbours and the cell below
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        uint32_t c = min(nb[k], prev);
        c += (uint32_t)(c != kTrNone);
        if (((m >> k) & 1u) && c < v[k]) {
          v[k] = c;
          ch = true;
        }
        prev = v[k];
      }
      prev = zhi;  // down z: the cell above
#pragma unroll
      for (int k = 7; k >= 0; --k) {
        const uint32_t c = prev + (uint32_t)(prev != kTrNone);
        if (((m >> k) & 1u) && c < v[k]) {
          v[k] = c;
          ch = true;
        }
        prev = v[k];
      }
      __syncthreads();  // the rows are read
      if (ch) {
        mine[0] = make_uint4(v[0], v[1], v[2], v[3]);
        mine[1] = make_uint4(v[4], v[5], v[6], v[7]);
      }
      if (!__builtin_amdgcn_ballot_w64(ch)) break;  // (the workgroup is one wave)
    }
    uint32_t chm = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) chm |= (uint32_t)(v[k] < old[k]) << k;
    if (chm) {  // (a lowered cell is traversable, so inside the grid)
      if (wide) {
        *(uint4*)(hops + base) = make_uint4(v[0], v[1], v[2], v[3]);
        *(uint4*)(hops + base + 4) = make_uint4(v[4], v[5], v[6], v[7]);
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if ((chm >> k) & 1u) hops[base + k] = v[k];
      }
    }
    // face f = 2 * axis + (towards +): a cell on it was lowered -> the tile beyond it is active
    const bool f0 = __builtin_amdgcn_ballot_w64(chm && lx == 0) != 0, f1 = __builtin_amdgcn_ballot_w64(chm && lx == 7) != 0;
    const bool f2 = __builtin_amdgcn_ballot_w64(chm && ly == 0) != 0, f3 = __builtin_amdgcn_ballot_w64(chm && ly == 7) != 0;
    const bool f4 = __builtin_amdgcn_ballot_w64((chm & 1u) != 0) != 0, f5 = __builtin_amdgcn_ballot_w64((chm & 0x80u) != 0) != 0;
    if (l < 6) {
      const bool want = l == 0 ? f0 : l == 1 ? f1 : l == 2 ? f2 : l == 3 ? f3 : l == 4 ? f4 : f5;
      const int qx = tx + (l == 1) - (l == 0), qy = ty + (l == 3) - (l == 2), qz = tz + (l == 5) - (l == 4);
      if (want && qx >= 0 && qy >= 0 && qz >= 0 && qx < (int)tl.ntx && qy < (int)tl.nty && qz < (int)tl.ntz) {
        const uint32_t q = ((uint32_t)qx * tl.nty + (uint32_t)qy) * tl.ntz + (uint32_t)qz;
        if ((coarse[q >> 5] >> (q & 31u)) & 1u) tr_enqueue(q, next, qnext, &count[(r + 1u) & 3u]);
      }
    }
#if defined(DMF_EXP_STATS)
    if (stats) {
      uint32_t c = (uint32_t)__popc(chm);
      for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
      if (l == 0) {
        atomicAdd(&stats[0], 1ull);
        if (c) atomicAdd(&stats[1], (unsigned long long)c);
      }
    }
#endif
  }
}

// ctl[1] += the cells with a finite value, ctl[2] = max(ctl[2], the largest of them)
constexpr int kTrFinishThreads = 256, kTrFinishWgs = 4096;
__global__ __launch_bounds__(kTrFinishThreads) void k_tr_finish(int64_t ncell, const uint32_t* __restrict__ hops,
                                                                unsigned long long* __restrict__ ctl) {
  __shared__ uint32_t sc[kTrFinishThreads / 64], sm[kTrFinishThreads / 64];
  uint32_t c = 0, mx = 0;
  const int64_t ngroups = (ncell + 3) >> 2;
  for (int64_t j = (int64_t)blockIdx.x * kTrFinishThreads + threadIdx.x; j < ngroups;
       j += (int64_t)gridDim.x * kTrFinishThreads) {
    const int64_t p = 4 * j;
    for_cells4(hops + p, (int)(ncell - p < 4 ? ncell - p : 4), [&](int, uint32_t h) {
      if (h != kTrNone) {
        ++c;
        mx = h > mx ? h : mx;
      }
    });
  }
  for (int o = 32; o > 0; o >>= 1) {
    c += __shfl_down(c, o, 64);
    const uint32_t u = __shfl_down(mx, o, 64);
    mx = u > mx ? u : mx;
  }
  if ((threadIdx.x & 63) == 0) {
    sc[threadIdx.x >> 6] = c;
    sm[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t tc = 0, tm = 0;
    for (int k = 0; k < kTrFinishThreads / 64; ++k) {
      tc += sc[k];
      tm = sm[k] > tm ? sm[k] : tm;
    }
    if (tc) {
      atomicAdd(&ctl[1], (unsigned long long)tc);
      atomicMax(&ctl[2], (unsigned long long)tm);
    }
  }
}

// One lane: cells[3 i ..] = the i-th cell of the path while i < cap, *n = the path's length.
__global__ __launch_bounds__(64) void k_tr_path(Geom g, const uint32_t* __restrict__ hops,
                                                const int32_t* __restrict__ target, int32_t* __restrict__ cells,
                                                int64_t cap, unsigned long long* __restrict__ n) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int nx = g.n[0], ny = g.n[1], nz = g.n[2];
  int x = target[0], y = target[1], z = target[2];
  unsigned long long len = 0;
  if (x >= 0 && y >= 0 && z >= 0 && x < nx && y < ny && z < nz) {
    uint32_t k = hops[((int64_t)x * ny + y) * nz + z];
    while (k != kTrNone) {  // (left by break: k only descends)
      if ((int64_t)len < cap) {
        cells[3 * len] = x;
        cells[3 * len + 1] = y;
        cells[3 * len + 2] = z;
      }
      ++len;
      if (k == 0) break;
      bool found = false;
      for (int f = 0; f < 6 && !found; ++f) {
        const int qx = x + (f == 1) - (f == 0), qy = y + (f == 3) - (f == 2), qz = z + (f == 5) - (f == 4);
        if (qx < 0 || qy < 0 || qz < 0 || qx >= nx || qy >= ny || qz >= nz) continue;
        if (hops[((int64_t)qx * ny + qy) * nz + qz] == k - 1u) {
          x = qx;
          y = qy;
          z = qz;
          found = true;
        }
      }
      if (!found) break;
      --k;
    }
  }
  *n = len;
}

// One row of the travel cost map: row[j] = hops at cells[j], INT_MAX for DMF_NO_PATH or a cell outside the grid.
__global__ __launch_bounds__(256) void k_tr_gather(Geom g, const uint32_t* __restrict__ hops,
                                                   const int32_t* __restrict__ cells, int V, int32_t* __restrict__ row) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= V) return;
  const int x = cells[3 * j], y = cells[3 * j + 1], z = cells[3 * j + 2];
  uint32_t h = kTrNone;
  if (x >= 0 && y >= 0 && z >= 0 && x < g.n[0] && y < g.n[1] && z < g.n[2]) h = hops[((int64_t)x * g.n[1] + y) * g.n[2] + z];
  row[j] = h == kTrNone ? INT_MAX : (int32_t)h;  // (a hop count is below 2^31: require_travel_grid)
}

// The plain arguments first (no access to the volume: they are rejected without a device).
static int check_travel_args(const dmf_volume* v, const void* dist2, const void* seeds, int64_t n_seeds,
                             const void* hops) {
  if (!v || !dist2 || !hops) return fail(DMF_ERR_INVALID, "null argument");
  if (n_seeds < 0) return fail(DMF_ERR_INVALID, "negative seed count %lld", (long long)n_seeds);
  if (n_seeds > 0 && !seeds) return fail(DMF_ERR_INVALID, "null seeds with %lld seeds", (long long)n_seeds);
  return DMF_OK;
}
static int check_path_args(const dmf_volume* v, const void* hops, const void* target, const void* cells, int64_t cap,
                           const void* n) {
  if (!v || !hops || !target || !n) return fail(DMF_ERR_INVALID, "null argument");
  if (cap < 0) return fail(DMF_ERR_INVALID, "negative capacity %lld", (long long)cap);
  if (cap > 0 && !cells) return fail(DMF_ERR_INVALID, "null cells with capacity %lld", (long long)cap);
  return DMF_OK;
}
// ... then the volume: constructed, at most 2048 cells per axis and 2^31 in all (a hop count fits
// below DMF_NO_PATH, and a tile index in 32 bits)
static int require_travel_grid(const dmf_volume* v) {
  DMF_TRY(require_grid_2048(v, "the travel field is limited to 2048 cells per axis"));
  if (v->ncell > ((size_t)1 << 31)) return fail(DMF_ERR_RANGE, "the travel field is limited to 2^31 cells");
  return DMF_OK;
}

// Waits for its own rounds.  info3 (host, may be null) = {traversable, reached, max hops}; the same
// three go to d_info3 (device, may be null) on the stream.
static int travel_device(dmf_volume* v, const uint32_t* d_dist2, uint32_t radius2, const int32_t* d_seeds,
                         int64_t n_seeds, uint32_t* d_hops, uint64_t* d_info3, uint64_t* info3) {
  const Geom g = v->geom();
  const GridTiles tl = grid_tiles(g.n);
  const uint32_t ncoarse = (tl.ntiles + 31u) / 32u;
  void *fine, *coarse, *queue, *ctlp;
  DMF_TRY(scratch(v, kScTrFine, sizeof(uint32_t) * 16 * (size_t)tl.ntiles, &fine));
  DMF_TRY(scratch(v, kScTrCoarse, sizeof(uint32_t) * ncoarse, &coarse));
  DMF_TRY(scratch(v, kScTrQueue, sizeof(uint32_t) * 2 * ((size_t)tl.ntiles + ncoarse), &queue));
  DMF_TRY(scratch(v, kScTrCtl, kTrCtlBytes, &ctlp));
  uint32_t* const queued[2] = {(uint32_t*)queue, (uint32_t*)queue + ncoarse};
  uint32_t* const list[2] = {(uint32_t*)queue + 2 * (size_t)ncoarse, (uint32_t*)queue + 2 * (size_t)ncoarse + tl.ntiles};
  unsigned long long* const ctl = (unsigned long long*)ctlp;
  uint32_t* const count = (uint32_t*)(ctl + kTrCtlWords);
  DMF_HIP(hipMemsetAsync(ctlp, 0, kTrCtlBytes, v->stream));
  DMF_HIP(hipMemsetAsync(queue, 0, sizeof(uint32_t) * 2 * (size_t)ncoarse, v->stream));
  DMF_HIP(hipMemsetAsync(d_hops, 0xff, sizeof(uint32_t) * v->ncell, v->stream));
  hipLaunchKernelGGL(k_tr_mask, dim3(ncoarse), dim3(kMaskThreads), 0, v->stream, g, tl, d_dist2, radius2,
                     (uint32_t*)fine, (uint32_t*)coarse, ctl);
  DMF_LAUNCH_CHECK();
  if (n_seeds > 0) {
    hipLaunchKernelGGL(k_tr_seed, dim3((unsigned)((n_seeds + 63) / 64)), dim3(64), 0, v->stream, g, tl,
                       (const uint32_t*)fine, d_seeds, n_seeds, d_hops, list[0], queued[0], count);
    DMF_LAUNCH_CHECK();
  }
  struct {
    uint64_t c[kTrCtlWords];
    uint32_t count[4];
  } h;
  static_assert(sizeof(h) == kTrCtlBytes, "the control block as the device lays it out");
  DMF_HIP(hipMemcpyAsync(&h, ctlp, kTrCtlBytes, hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipStreamSynchronize(v->stream));
  const uint64_t bound = h.c[0] + 2;  // rounds
  const unsigned wgs = (unsigned)std::min<uint32_t>(tl.ntiles, kTrRoundWgs);
  uint64_t r = 0, launches = 0;
  uint32_t pending = h.count[0];
  unsigned long long* stats = nullptr;
#if defined(DMF_EXP_STATS)
  stats = ctl + 3;
#endif
  while (pending) {
    if (r >= bound)
      return fail(DMF_ERR_DEVICE_CHECK, "the travel field has not converged after %llu rounds over %llu traversable cells",
                  (unsigned long long)r, (unsigned long long)h.c[0]);
    const uint64_t nb = std::min<uint64_t>(kTrBatch, bound - r);
    for (uint64_t k = 0; k < nb; ++k, ++r) {
      const int p = (int)(r & 1);
      hipLaunchKernelGGL(k_tr_round, dim3(wgs), dim3(64), 0, v->stream, g, tl, (const uint32_t*)fine,
                         (const uint32_t*)coarse, d_hops, (const uint32_t*)list[p], list[p ^ 1], queued[p],
                         queued[p ^ 1], count, (uint32_t)r, ctl + 5, stats);
      DMF_LAUNCH_CHECK();
    }
    launches += nb;
    DMF_HIP(hipMemcpyAsync(h.count, count, sizeof(h.count), hipMemcpyDeviceToHost, v->stream));
    DMF_HIP(hipStreamSynchronize(v->stream));
    // rounds past the first empty list did nothing: the rounds that had work end at the first zero
    pending = h.count[r & 3];
  }
  hipLaunchKernelGGL(k_tr_finish, dim3((unsigned)std::min<int64_t>(((int64_t)v->ncell + 1023) / 1024, kTrFinishWgs)),
                     dim3(kTrFinishThreads), 0, v->stream, (int64_t)v->ncell, (const uint32_t*)d_hops, ctl);
  DMF_LAUNCH_CHECK();
  if (d_info3) DMF_HIP(hipMemcpyAsync(d_info3, ctlp, sizeof(uint64_t) * 3, hipMemcpyDeviceToDevice, v->stream));
  DMF_HIP(hipMemcpyAsync(h.c, ctlp, sizeof(h.c), hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipStreamSynchronize(v->stream));
  if (info3)
    for (int k = 0; k < 3; ++k) info3[k] = h.c[k];
  v->travel_stats[0] = h.c[5];
  v->travel_stats[1] = launches + 2 + (n_seeds > 0);  // the rounds launched, the mask, seed and finish passes
  v->travel_stats[2] = h.c[3];
  v->travel_stats[3] = h.c[4];
  return DMF_OK;
}

constexpr int kTrMaxCostCells = 46340;  // V * V < 2^31, the limit of dmf_tour*
static int check_cost_map_args(const dmf_volume* v, const void* dist2, const void* cells, int32_t V, const void* map) {
  if (!v || !dist2) return fail(DMF_ERR_INVALID, "null argument");
  if (V < 0) return fail(DMF_ERR_INVALID, "negative V %d", V);
  if (V > kTrMaxCostCells) return fail(DMF_ERR_RANGE, "the travel cost map is limited to %d cells, got %d", kTrMaxCostCells, V);
  if (V > 0 && (!cells || !map)) return fail(DMF_ERR_INVALID, "null argument with V = %d", V);
  return DMF_OK;
}

// One travel field per row into the scratch hop buffer, then the row's gather.
static int cost_map_device(dmf_volume* v, const uint32_t* d_dist2, uint32_t radius2, const int32_t* d_cells, int V,
                           int32_t* d_map) {
  if (V == 0) return DMF_OK;
  void* dh;
  DMF_TRY(scratch(v, kScTrHops, sizeof(uint32_t) * v->ncell, &dh));
  for (int i = 0; i < V; ++i) {
    DMF_TRY(travel_device(v, d_dist2, radius2, d_cells + 3 * (size_t)i, 1, (uint32_t*)dh, nullptr, nullptr));
    hipLaunchKernelGGL(k_tr_gather, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, v->stream, v->geom(),
                       (const uint32_t*)dh, d_cells, V, d_map + (size_t)i * V);
    DMF_LAUNCH_CHECK();
  }
  DMF_HIP(hipStreamSynchronize(v->stream));
  return DMF_OK;
}

static int path_device(dmf_volume* v, const uint32_t* d_hops, const int32_t* d_target, int32_t* d_cells, int64_t cap,
                       uint64_t* d_n) {
  hipLaunchKernelGGL(k_tr_path, dim3(1), dim3(64), 0, v->stream, v->geom(), d_hops, d_target, d_cells, cap,
                     (unsigned long long*)d_n);
  DMF_LAUNCH_CHECK();
  return DMF_OK;
}

}  // namespace dmf

using namespace dmf;

extern "C" {

int dmf_grid_travel_device(dmf_volume* v, const uint32_t* d_dist2, uint32_t radius2, const int32_t* d_seeds,
                           int64_t n_seeds, uint32_t* d_hops, uint64_t* d_info3) {
  DMF_API_BEGIN
  DMF_TRY(check_travel_args(v, d_dist2, d_seeds, n_seeds, d_hops));
  DMF_TRY(require_travel_grid(v));
  return travel_device(v, d_dist2, radius2, d_seeds, n_seeds, d_hops, d_info3, nullptr);
  DMF_API_END
}

int dmf_grid_travel(dmf_volume* v, const uint32_t* dist2, uint32_t radius2, const int32_t* seeds, int64_t n_seeds,
                    uint32_t* hops, uint64_t* info3) {
  DMF_API_BEGIN
  DMF_TRY(check_travel_args(v, dist2, seeds, n_seeds, hops));
  DMF_TRY(require_travel_grid(v));
  void *dd, *dh, *ds = nullptr;
  DMF_TRY(scratch(v, kScDfDist, sizeof(uint32_t) * v->ncell, &dd));
  DMF_TRY(scratch(v, kScTrHops, sizeof(uint32_t) * v->ncell, &dh));
  DMF_HIP(hipMemcpyAsync(dd, dist2, sizeof(uint32_t) * v->ncell, hipMemcpyHostToDevice, v->stream));
  if (n_seeds > 0) {
    DMF_TRY(scratch(v, kScHost1, sizeof(int32_t) * 3 * (size_t)n_seeds, &ds));
    DMF_HIP(hipMemcpyAsync(ds, seeds, sizeof(int32_t) * 3 * (size_t)n_seeds, hipMemcpyHostToDevice, v->stream));
  }
  DMF_TRY(travel_device(v, (const uint32_t*)dd, radius2, (const int32_t*)ds, n_seeds, (uint32_t*)dh, nullptr, info3));
  DMF_HIP(hipMemcpyAsync(hops, dh, sizeof(uint32_t) * v->ncell, hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipStreamSynchronize(v->stream));
  return DMF_OK;
  DMF_API_END
}

int dmf_grid_travel_cost_map_device(dmf_volume* v, const uint32_t* d_dist2, uint32_t radius2, const int32_t* d_cells,
                                    int32_t V, int32_t* d_map) {
  DMF_API_BEGIN
  DMF_TRY(check_cost_map_args(v, d_dist2, d_cells, V, d_map));
  DMF_TRY(require_travel_grid(v));
  return cost_map_device(v, d_dist2, radius2, d_cells, V, d_map);
  DMF_API_END
}

int dmf_grid_travel_cost_map(dmf_volume* v, const uint32_t* dist2, uint32_t radius2, const int32_t* cells, int32_t V,
                             int32_t* map) {
  DMF_API_BEGIN
  DMF_TRY(check_cost_map_args(v, dist2, cells, V, map));
  DMF_TRY(require_travel_grid(v));
  if (V == 0) return DMF_OK;
  void *dd, *dc, *dm;
  const size_t mapb = sizeof(int32_t) * (size_t)V * (size_t)V;
  DMF_TRY(scratch(v, kScDfDist, sizeof(uint32_t) * v->ncell, &dd));
  DMF_TRY(scratch(v, kScHost1, sizeof(int32_t) * 3 * (size_t)V, &dc));
  DMF_TRY(scratch(v, kScOut0, mapb, &dm));
  DMF_HIP(hipMemcpyAsync(dd, dist2, sizeof(uint32_t) * v->ncell, hipMemcpyHostToDevice, v->stream));
  DMF_HIP(hipMemcpyAsync(dc, cells, sizeof(int32_t) * 3 * (size_t)V, hipMemcpyHostToDevice, v->stream));
  DMF_TRY(cost_map_device(v, (const uint32_t*)dd, radius2, (const int32_t*)dc, V, (int32_t*)dm));
  DMF_HIP(hipMemcpyAsync(map, dm, mapb, hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipStreamSynchronize(v->stream));
  return DMF_OK;
  DMF_API_END
}

int dmf_grid_path_device(dmf_volume* v, const uint32_t* d_hops, const int32_t* d_target3, int32_t* d_cells, int64_t cap,
                         uint64_t* d_n) {
  DMF_API_BEGIN
  DMF_TRY(check_path_args(v, d_hops, d_target3, d_cells, cap, d_n));
  DMF_TRY(require_travel_grid(v));
  return path_device(v, d_hops, d_target3, d_cells, cap, d_n);
  DMF_API_END
}

int dmf_grid_path(dmf_volume* v, const uint32_t* hops, const int32_t* target3, int32_t* cells, int64_t cap, int64_t* n) {
  DMF_API_BEGIN
  DMF_TRY(check_path_args(v, hops, target3, cells, cap, n));
  DMF_TRY(require_travel_grid(v));
  // no path is longer than the grid has cells
  const int64_t dcap = std::min<int64_t>(cap, (int64_t)v->ncell);
  void *dh, *dt, *dc, *dn;
  uint64_t len = 0;
  DMF_TRY(scratch(v, kScTrHops, sizeof(uint32_t) * v->ncell, &dh));
  DMF_TRY(scratch(v, kScHost1, sizeof(int32_t) * 3, &dt));
  DMF_TRY(scratch(v, kScOut0, sizeof(int32_t) * 3 * (size_t)std::max<int64_t>(dcap, 1), &dc));
  DMF_TRY(scratch(v, kScOut3, sizeof(uint64_t), &dn));
  DMF_HIP(hipMemcpyAsync(dh, hops, sizeof(uint32_t) * v->ncell, hipMemcpyHostToDevice, v->stream));
  DMF_HIP(hipMemcpyAsync(dt, target3, sizeof(int32_t) * 3, hipMemcpyHostToDevice, v->stream));
  DMF_TRY(path_device(v, (const uint32_t*)dh, (const int32_t*)dt, (int32_t*)dc, dcap, (uint64_t*)dn));
  DMF_HIP(hipMemcpyAsync(&len, dn, sizeof(uint64_t), hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipStreamSynchronize(v->stream));
  *n = (int64_t)len;
  if ((int64_t)len > cap) {
    if (cap == 0 && !cells) return DMF_OK;  // the size query
    return fail(DMF_ERR_CAPACITY, "the path has %lld cells, capacity %lld", (long long)len, (long long)cap);
  }
  if (len) {
    DMF_HIP(hipMemcpyAsync(cells, dc, sizeof(int32_t) * 3 * (size_t)len, hipMemcpyDeviceToHost, v->stream));
    DMF_HIP(hipStreamSynchronize(v->stream));
  }
  return DMF_OK;
  DMF_API_END
}

int dmf_grid_travel_stats(const dmf_volume* v, uint64_t* stats4) {
  DMF_API_BEGIN
  if (!v || !stats4) return fail(DMF_ERR_INVALID, "null argument");
  for (int k = 0; k < 4; ++k) stats4[k] = v->travel_stats[k];
  return DMF_OK;
  DMF_API_END
}

}  // extern "C"
