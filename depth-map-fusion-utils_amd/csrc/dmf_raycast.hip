// dmf_raycast.hip — the log-odds ray-cast of a fused grid on gfx950.
// What a camera at pose T sees in a fused grid: per pixel the first cell
// of the fusion's own probe ray (depth range_mm) whose log-odds reach a threshold.  Three kernels:
//  k_rc_mask   — one streaming pass over the int16 grid: a 1-bit-per-cell mask of L >= threshold
//                in the occupancy bitmask's 8x8x8-tile layout (occ_bit, dmf_internal.hpp) and one
//                bit per tile over it (512^3: 16 MiB + 32 KiB, against 256 MiB of int16);
//  k_rc_bricks — one bit per 32^3-cell brick (4x4x4 tiles) from the tile bits;
//  k_rc_cast   — one lane per pixel: dda_setup once, then the dda_select walk.  The tile bit is
//                read when the tile changes, a mask word only inside a non-empty tile and only
//                when the word changes.  <true> also reads the brick bit when the brick changes and
//                leaves a wholly empty brick or tile in one exact jump (rc_jump) instead of cell by
//                cell.  Skipping removes loads and tests of empty cells, never cells of the
//                sequence: the reported cell is the plain walk's.
#include "dmf_dda.hpp"
#include "dmf_host.hpp"

namespace dmf {

struct RcTiles {
  uint32_t nty, ntz, ntiles;   // 8x8x8-cell tiles along y and z, and in all (x-major, as occ_bit)
  uint32_t nby, nbz, nbricks;  // 32^3-cell bricks (4x4x4 tiles) likewise
};
static RcTiles rc_tiles(const Geom& g) {
  const uint32_t ntx = ((uint32_t)g.n[0] + 7u) >> 3, nty = ((uint32_t)g.n[1] + 7u) >> 3, ntz = ((uint32_t)g.n[2] + 7u) >> 3;
  const uint32_t nbx = (ntx + 3u) >> 2, nby = (nty + 3u) >> 2, nbz = (ntz + 3u) >> 2;
  return RcTiles{nty, ntz, ntx * nty * ntz, nby, nbz, nbx * nby * nbz};
}

// One workgroup per 32 consecutive tiles = 512 mask words = one word of the tile level.  Thread
// (tile j = i & 31, word w = i >> 5) reads the word's 4 y-rows of 8 z-cells (16 B each): a wave's
// loads are 2 x 4 rows of up to 512 contiguous bytes.  The words go through LDS so that the
// workgroup's 2 KiB of the mask are stored in order.  Cells past the grid (partial tiles) are 0.
constexpr int kRcMaskThreads = 512;
constexpr int kRcDefaultWalk = 2;  // DMF_KNOB_RAYCAST_WALK = 0 (measured: DESIGN.md §5.11)
__global__ __launch_bounds__(kRcMaskThreads) void k_rc_mask(Geom g, RcTiles tl, const int16_t* __restrict__ L,
                                                            int threshold, uint32_t* __restrict__ fine,
                                                            uint32_t* __restrict__ coarse) {
  __shared__ uint32_t sw[kRcMaskThreads];
  __shared__ uint32_t sany[16];
  const int i = threadIdx.x, j = i & 31, w = i >> 5;
  const uint32_t t = blockIdx.x * 32u + (uint32_t)j;
  uint32_t word = 0;
  if (t < tl.ntiles) {
    const uint32_t tz = t % tl.ntz, r = t / tl.ntz;
    const int x = (int)(r / tl.nty) * 8 + (w >> 1), y0 = (int)(r % tl.nty) * 8 + (w & 1) * 4, z0 = (int)tz * 8;
    if (x < g.n[0]) {
#pragma unroll
      for (int dy = 0; dy < 4; ++dy) {
        const int y = y0 + dy;
        if (y < g.n[1]) {
          const int16_t* row = L + (((int64_t)x * g.n[1] + y) * g.n[2] + z0);
          uint32_t b = 0;
          if (z0 + 8 <= g.n[2] && ((uintptr_t)row & 15) == 0) {
            const uint4 q = *(const uint4*)row;
            const uint32_t u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              b |= (uint32_t)((int)(int16_t)(u[k] & 0xffffu) >= threshold) << (2 * k);
              b |= (uint32_t)((int)(int16_t)(u[k] >> 16) >= threshold) << (2 * k + 1);
            }
          } else {
            for (int k = 0; k < 8 && z0 + k < g.n[2]; ++k) b |= (uint32_t)((int)row[k] >= threshold) << k;
          }
          word |= b << (8 * dy);
        }
      }
    }
  }
  sw[j * 16 + w] = word;
  // a wave holds words 2k (lanes 0-31) and 2k + 1 (lanes 32-63) of the 32 tiles
  const uint64_t any = __builtin_amdgcn_ballot_w64(word != 0u);
  if ((i & 63) == 0) {
    sany[w] = (uint32_t)any;
    sany[w + 1] = (uint32_t)(any >> 32);
  }
  __syncthreads();
  const uint32_t o = blockIdx.x * (uint32_t)kRcMaskThreads + (uint32_t)i;
  if (o < tl.ntiles * 16u) fine[o] = sw[i];
  if (i == 0) {
    uint32_t a = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) a |= sany[k];
    coarse[blockIdx.x] = a;  // bit j = tile 32 * block + j holds a solid cell
  }
}

// One lane per brick: the OR of its 4x4x4 tile bits (tiles past the grid's last tile row are
// absent).  One workgroup per 32 bricks = one word of the brick level.
__global__ __launch_bounds__(64) void k_rc_bricks(RcTiles tl, uint32_t ntx, const uint32_t* __restrict__ coarse,
                                                  uint32_t* __restrict__ bricks) {
  const uint32_t b = blockIdx.x * 32u + (threadIdx.x & 31u);
  bool any = false;
  if (threadIdx.x < 32 && b < tl.nbricks) {
    const uint32_t bz = b % tl.nbz, r = b / tl.nbz, by = r % tl.nby, bx = r / tl.nby;
    for (uint32_t dx = 0; dx < 4; ++dx)
      for (uint32_t dy = 0; dy < 4; ++dy) {
        const uint32_t tx = bx * 4 + dx, ty = by * 4 + dy;
        if (tx >= ntx || ty >= tl.nty) continue;
        for (uint32_t tz = bz * 4; tz < bz * 4 + 4 && tz < tl.ntz; ++tz) {
          const uint32_t t = (tx * tl.nty + ty) * tl.ntz + tz;
          any |= (coarse[t >> 5] >> (t & 31u)) & 1u;
        }
      }
  }
  const uint64_t m = __builtin_amdgcn_ballot_w64(any);
  if (threadIdx.x == 0) bricks[blockIdx.x] = (uint32_t)m;
}

// floor(x / k) for 0 <= x < 2^35, 1 <= k < 2^29 with quotient < 2^12: a float estimate (within 1 of
// the quotient: three roundings of 2^-24 relative each) and exact integer correction.
__device__ inline int32_t rc_div(int64_t x, int32_t k) {
  int32_t q = (int32_t)((float)x * __builtin_amdgcn_rcpf((float)k));
  int64_t r = x - (int64_t)q * k;
  if (r < 0) { --q; r += k; }
  if (r < 0) { --q; r += k; }
  if (r >= k) { ++q; r -= k; }
  if (r >= k) { ++q; }
  return q;
}

// Exact jump out of the aligned cube of (m + 1)^3 cells (m = 7 or 31) that holds the current cell:
// the walk state after the crossing that leaves the cube, and the number of steps that takes.
// In the cube, axis a can still make r_a crossings; its (r_a + 1)-th leaves.  The earliest of the
// three leaving events in the walk's own order (crossing time, ties x < y < z) is found as
// dda_select finds the next crossing, from F_ab = E_ab + r_a K_b - r_b K_a (the crossing-time
// difference of the two leaving events); every crossing of another axis b that
// precedes that event (a*, r*) in the same order is taken with it: #{k >= 0 : k K_a* < X} for
// b > a*, <= X for b < a*, X = (h_a* + 2Q r*) |dq_b| - h_b |dq_a*| = +-E + r* K_b.  A step along a
// adds K_b to E_ab and takes K_a from E_ba, so n_a steps per axis move E_ab by n_a K_b - n_b K_a.
// A non-moving axis has K = 0, r = 0 and |E| = kNever against a moving one: it neither leaves
// nor steps.  Returns the steps; more than the ray has left means the ray ends in the cube.
__device__ inline int rc_jump(int m, int& c0, int& c1, int& c2, int st0, int st1, int st2, int32_t& E01, int32_t& E02,
                              int32_t& E12, int32_t K0, int32_t K1, int32_t K2) {
  const int r0 = st0 > 0 ? m - (c0 & m) : (st0 < 0 ? (c0 & m) : 0);
  const int r1 = st1 > 0 ? m - (c1 & m) : (st1 < 0 ? (c1 & m) : 0);
  const int r2 = st2 > 0 ? m - (c2 & m) : (st2 < 0 ? (c2 & m) : 0);
  const int64_t F01 = (int64_t)E01 + (int64_t)r0 * K1 - (int64_t)r1 * K0;
  const int64_t F02 = (int64_t)E02 + (int64_t)r0 * K2 - (int64_t)r2 * K0;
  const int64_t F12 = (int64_t)E12 + (int64_t)r1 * K2 - (int64_t)r2 * K1;
  const bool b10 = F01 > 0;
  const bool s2 = (b10 ? F12 : F02) > 0, s1 = !s2 && b10;
  // crossings of axis b before the leaving event of a*: d = h_a* |dq_b| - h_b |dq_a*|
  auto before = [](int64_t d, int rs, int32_t kb, int32_t ka, bool b_after) -> int {
    const int64_t x = d + (int64_t)rs * kb;
    if (x < 0 || ka == 0) return 0;
    const int32_t q = rc_div(x, ka);
    return b_after ? (int)(q + ((int64_t)q * ka < x ? 1 : 0)) : (int)q + 1;
  };
  int n0, n1, n2;
  if (s2) {
    n2 = r2 + 1;
    n0 = before(-(int64_t)E02, r2, K0, K2, false);
    n1 = before(-(int64_t)E12, r2, K1, K2, false);
  } else if (s1) {
    n1 = r1 + 1;
    n0 = before(-(int64_t)E01, r1, K0, K1, false);
    n2 = before((int64_t)E12, r1, K2, K1, true);
  } else {
    n0 = r0 + 1;
    n1 = before((int64_t)E01, r0, K1, K0, true);
    n2 = before((int64_t)E02, r0, K2, K0, true);
  }
  c0 += st0 * n0;
  c1 += st1 * n1;
  c2 += st2 * n2;
  E01 = (int32_t)((uint32_t)E01 + (uint32_t)n0 * (uint32_t)K1 - (uint32_t)n1 * (uint32_t)K0);
  E02 = (int32_t)((uint32_t)E02 + (uint32_t)n0 * (uint32_t)K2 - (uint32_t)n2 * (uint32_t)K0);
  E12 = (int32_t)((uint32_t)E12 + (uint32_t)n1 * (uint32_t)K2 - (uint32_t)n2 * (uint32_t)K1);
  return n0 + n1 + n2;
}

// One 64-lane workgroup per 8x8 pixel packet of one pose (neighbouring rays share tiles and
// words).  Outputs per pixel: depth (rayTraceVolume's value of the surface voxel, k_zbuffer's
// arithmetic; -1 = none) and cell (getHashId; all ones = none); either may be null.  stats (may
// be null): {rays with a non-empty sequence, rays with a surface cell}.
template <bool JUMP>
__global__ __launch_bounds__(64) void k_rc_cast(Geom g, RcTiles tl, CamP cam, const PoseX* __restrict__ poses,
                                                int range_mm, int packets_x, const uint32_t* __restrict__ fine,
                                                const uint32_t* __restrict__ coarse,
                                                const uint32_t* __restrict__ bricks, int32_t* __restrict__ depth,
                                                uint64_t* __restrict__ cell, unsigned long long* __restrict__ stats) {
  stats = stat_slot(stats);
  const int l = threadIdx.x;
  const int pr = (blockIdx.x / packets_x) * 8 + (l >> 3), pc = (blockIdx.x % packets_x) * 8 + (l & 7);
  const bool in_image = pr < cam.H && pc < cam.W;
  const PoseX& T = poses[blockIdx.y];
  Ray R;
  R.left = 0;
  if (in_image) {
    float pcam[3], E[3];
    project(cam, pr, pc, range_mm, pcam);
    xform(T.f, pcam[0], pcam[1], pcam[2], E);
    const bool inside = endpoint_inside(g, E);
    const float O[3] = {T.f[3], T.f[7], T.f[11]};
    if (!dda_setup(g, O, E, inside, R)) R.left = 0;
  }
  int32_t E01 = R.E01, E02 = R.E02, E12 = R.E12;
  const int32_t K0 = R.K[0], K1 = R.K[1], K2 = R.K[2];
  const int st0 = R.st[0], st1 = R.st[1], st2 = R.st[2];
  int c0 = R.c[0], c1 = R.c[1], c2 = R.c[2], left = R.left;
  const bool entered = left > 0;
  bool found = false, tile_solid = false, brick_solid = false;
  uint32_t last_t = 0xffffffffu, last_b = 0xffffffffu, last_w = 0xffffffffu, word = 0;
  while (left > 0) {
    const uint32_t t = (((uint32_t)c0 >> 3) * tl.nty + ((uint32_t)c1 >> 3)) * tl.ntz + ((uint32_t)c2 >> 3);
    if (t != last_t) {
      last_t = t;
      if (JUMP) {  // (the cell-by-cell walk has no use for the brick level: it would only add a test)
        const uint32_t b = (((uint32_t)c0 >> 5) * tl.nby + ((uint32_t)c1 >> 5)) * tl.nbz + ((uint32_t)c2 >> 5);
        if (b != last_b) {
          last_b = b;
          brick_solid = (bricks[b >> 5] >> (b & 31u)) & 1u;
        }
      }
      tile_solid = (!JUMP || brick_solid) && ((coarse[t >> 5] >> (t & 31u)) & 1u);
      if (JUMP && !tile_solid) {
        // every cell up to the crossing that leaves the empty cube is empty
        const int n = rc_jump(brick_solid ? 7 : 31, c0, c1, c2, st0, st1, st2, E01, E02, E12, K0, K1, K2);
        if (n >= left) break;  // the ray ends inside it
        left -= n;
        continue;
      }
    }
    if (tile_solid) {
      const uint32_t wi = (t << 4) | (((uint32_t)c0 & 7u) << 1) | (((uint32_t)c1 & 7u) >> 2);
      if (wi != last_w) {
        last_w = wi;
        word = fine[wi];
      }
      if ((word >> ((((uint32_t)c1 & 3u) << 3) | ((uint32_t)c2 & 7u))) & 1u) {
        found = true;
        break;
      }
    }
    if (--left == 0) break;
    bool s0, s1, s2;
    dda_select(E01, E02, E12, K0, K1, K2, s0, s1, s2);
    c0 += s0 ? st0 : 0;
    c1 += s1 ? st1 : 0;
    c2 += s2 ? st2 : 0;
  }
  if (in_image) {
    int32_t d = -1;
    uint64_t h = ~0ull;
    if (found) {
      h = hash_id(c0, c1, c2);
      // the voxel centre from the cell index as reverseRayTraceFast forms it, then k_zbuffer's depth
      const float x = (float)((double)c0 * g.dl[0] + g.mn[0]), y = (float)((double)c1 * g.dl[1] + g.mn[1]),
                  z = (float)((double)c2 * g.dl[2] + g.mn[2]);
      float tc[3];
      xform(T.i, (float)((double)x + g.hdl[0]), (float)((double)y + g.hdl[1]), (float)((double)z + g.hdl[2]), tc);
      d = to_int_x86((double)roundf(tc[2] * 1000.0f));
    }
    const int64_t o = ((int64_t)blockIdx.y * cam.H + pr) * cam.W + pc;
    if (depth) depth[o] = d;
    if (cell) cell[o] = h;
  }
  if (stats) {
    unsigned long long ne = entered ? 1 : 0, nf = found ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) {
      ne += __shfl_down(ne, o, 64);
      nf += __shfl_down(nf, o, 64);
    }
    if (l == 0) {
      if (ne) atomicAdd(&stats[0], ne);
      if (nf) atomicAdd(&stats[1], nf);
    }
  }
}

// The plain arguments first (no access to the volume: they are rejected without a device), then
// what the fusion checks (constructed, camera, P in 1..65535, grid size).
static int check_raycast(const dmf_volume* v, const dmf_camera* cam, const void* logodds, const void* poses, int32_t P,
                         int32_t range_mm) {
  if (!v || !cam || !logodds || !poses) return fail(DMF_ERR_INVALID, "null argument");
  if (range_mm < 1 || range_mm > 65535) return fail(DMF_ERR_INVALID, "range_mm %d out of range [1,65535]", range_mm);
  if (P < 0) return fail(DMF_ERR_INVALID, "negative pose count %d", P);
  return check_fuse_call(v, cam, P);
}

static int raycast_device(dmf_volume* v, const dmf_camera* cam, const int16_t* d_logodds, const float* d_poses,
                          int32_t P, int32_t threshold, int32_t range_mm, int32_t* d_depth, uint64_t* d_cell,
                          uint64_t* d_stats) {
  const CamP cp = cam_params(cam);
  const Geom g = v->geom();
  const RcTiles tl = rc_tiles(g);
  PoseX* tab = nullptr;
  DMF_TRY(pose_table(v, d_poses, P, true, &tab));
  // the tile words, then the brick words, in one buffer
  const uint32_t ncoarse = (tl.ntiles + 31u) / 32u, nbw = (tl.nbricks + 31u) / 32u;
  void *fine, *coarse;
  DMF_TRY(scratch(v, kScRcFine, sizeof(uint32_t) * 16 * (size_t)tl.ntiles, &fine));
  DMF_TRY(scratch(v, kScRcCoarse, sizeof(uint32_t) * ((size_t)ncoarse + nbw), &coarse));
  uint32_t* const bricks = (uint32_t*)coarse + ncoarse;
  unsigned long long* st = nullptr;
  if (d_stats) DMF_TRY(stats_begin(v, &st));
  hipLaunchKernelGGL(k_rc_mask, dim3(ncoarse), dim3(kRcMaskThreads), 0, v->stream, g, tl, d_logodds, threshold,
                     (uint32_t*)fine, (uint32_t*)coarse);
  DMF_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_rc_bricks, dim3(nbw), dim3(64), 0, v->stream, tl, ((uint32_t)g.n[0] + 7u) >> 3,
                     (const uint32_t*)coarse, bricks);
  DMF_LAUNCH_CHECK();
  const int pkx = (cp.W + 7) / 8;
  const dim3 grid((unsigned)(pkx * ((cp.H + 7) / 8)), (unsigned)P);
  // DMF_KNOB_RAYCAST_WALK (dmf_diag.h): 1 = cell by cell, 2 = empty bricks and tiles jumped
  const int64_t kw = v->knob[DMF_KNOB_RAYCAST_WALK];
  if (((kw == 1 || kw == 2) ? (int)kw : kRcDefaultWalk) == 2) {
    hipLaunchKernelGGL(k_rc_cast<true>, grid, dim3(64), 0, v->stream, g, tl, cp, tab, range_mm, pkx,
                       (const uint32_t*)fine, (const uint32_t*)coarse, (const uint32_t*)bricks, d_depth, d_cell, st);
  } else {
    hipLaunchKernelGGL(k_rc_cast<false>, grid, dim3(64), 0, v->stream, g, tl, cp, tab, range_mm, pkx,
                       (const uint32_t*)fine, (const uint32_t*)coarse, (const uint32_t*)bricks, d_depth, d_cell, st);
  }
  DMF_LAUNCH_CHECK();
  if (d_stats) DMF_TRY(stats_end(v, st, d_stats, 2));
  return DMF_OK;
}

}  // namespace dmf

using namespace dmf;

extern "C" {

int dmf_raycast_logodds_device(dmf_volume* v, const dmf_camera* cam, const int16_t* d_logodds, const float* d_poses,
                               int32_t P, int32_t threshold, int32_t range_mm, int32_t* d_depth, uint64_t* d_cell,
                               uint64_t* d_stats) {
  DMF_API_BEGIN
  DMF_TRY(check_raycast(v, cam, d_logodds, d_poses, P, range_mm));
  return raycast_device(v, cam, d_logodds, d_poses, P, threshold, range_mm, d_depth, d_cell, d_stats);
  DMF_API_END
}

int dmf_raycast_logodds(dmf_volume* v, const dmf_camera* cam, const int16_t* logodds, const float* poses, int32_t P,
                        int32_t threshold, int32_t range_mm, int32_t* depth, uint64_t* cell) {
  DMF_API_BEGIN
  DMF_TRY(check_raycast(v, cam, logodds, poses, P, range_mm));
  const size_t n = (size_t)P * (size_t)cam->height * (size_t)cam->width;
  void *dl, *dp, *dd = nullptr, *dc = nullptr;
  DMF_TRY(scratch(v, kScOut2, sizeof(int16_t) * v->ncell, &dl));
  DMF_TRY(scratch(v, kScHost2, sizeof(float) * 12 * (size_t)P, &dp));
  if (depth) DMF_TRY(scratch(v, kScOut0, sizeof(int32_t) * n, &dd));
  if (cell) DMF_TRY(scratch(v, kScOut1, sizeof(uint64_t) * n, &dc));
  DMF_HIP(hipMemcpyAsync(dl, logodds, sizeof(int16_t) * v->ncell, hipMemcpyHostToDevice, v->stream));
  DMF_HIP(hipMemcpyAsync(dp, poses, sizeof(float) * 12 * (size_t)P, hipMemcpyHostToDevice, v->stream));
  DMF_TRY(raycast_device(v, cam, (const int16_t*)dl, (const float*)dp, P, threshold, range_mm, (int32_t*)dd,
                         (uint64_t*)dc, nullptr));
  if (depth) DMF_HIP(hipMemcpyAsync(depth, dd, sizeof(int32_t) * n, hipMemcpyDeviceToHost, v->stream));
  if (cell) DMF_HIP(hipMemcpyAsync(cell, dc, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipStreamSynchronize(v->stream));
  return DMF_OK;
  DMF_API_END
}

}  // extern "C"
