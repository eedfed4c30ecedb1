// dmf_raycast.hip — the log-odds ray-cast of a fused grid on gfx950.
// What a camera at pose T sees in a fused grid: per pixel the first cell
// of the fusion's own probe ray (depth range_mm) whose log-odds reach a threshold.  Three kernels:
//  k_rc_mask   — one streaming pass over the int16 grid: a 1-bit-per-cell mask of L >= threshold
//                in the occupancy bitmask's 8x8x8-tile layout (the tile mask pass and the layout
//                are dmf_gridbits.hpp's, shared with dmf_surface.hip) and one bit per tile over
//                it (512^3: 16 MiB + 32 KiB, against 256 MiB of int16);
//  k_rc_bricks — one bit per 32^3-cell brick (4x4x4 tiles) from the tile bits;
//  k_rc_cast   — one lane per pixel: dda_setup once, then the walk of dmf_dda.hpp.  The tile bit is
//                read when the tile changes, a mask word only inside a non-empty tile and only
//                when the word changes.  <true> also reads the brick bit when the brick changes and
//                leaves a wholly empty brick or tile in one exact jump (rc_jump, dmf_dda.hpp) instead of cell by
//                cell.  Skipping removes loads and tests of empty cells, never cells of the
//                sequence: the reported cell is the plain walk's.
#include "dmf_dda.hpp"
#include "dmf_host.hpp"

namespace dmf {

// The mask pass (tile_mask_pass, dmf_gridbits.hpp) with one mask, and over it one word of the tile
// level per workgroup: bit j = tile 32 * block + j holds a solid cell.
constexpr int kRcDefaultWalk = 2;  // DMF_KNOB_RAYCAST_WALK = 0 (measured: DESIGN.md §5.11)
__global__ __launch_bounds__(kMaskThreads) void k_rc_mask(Geom g, GridTiles tl, const int16_t* __restrict__ L,
                                                          int threshold, uint32_t* __restrict__ fine,
                                                          uint32_t* __restrict__ coarse) {
  __shared__ uint32_t sany[16];
  uint32_t* const out[1] = {fine};
  uint32_t word[1];
  tile_mask_pass<1>(g, tl, L, out, word,
                    [=](int c, int k, uint32_t (&b)[1]) { b[0] |= (uint32_t)(c >= threshold) << k; });
  // a wave holds words 2k (lanes 0-31) and 2k + 1 (lanes 32-63) of the 32 tiles
  const int i = threadIdx.x, w = i >> 5;
  const uint64_t any = __builtin_amdgcn_ballot_w64(word[0] != 0u);
  if ((i & 63) == 0) {
    sany[w] = (uint32_t)any;
    sany[w + 1] = (uint32_t)(any >> 32);
  }
  __syncthreads();
  if (i == 0) {
    uint32_t a = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) a |= sany[k];
    coarse[blockIdx.x] = a;
  }
}

// One workgroup per 32 bricks = one word of the brick level (brick_word, dmf_gridbits.hpp).
__global__ __launch_bounds__(64) void k_rc_bricks(GridTiles tl, const uint32_t* __restrict__ coarse,
                                                  uint32_t* __restrict__ bricks) {
  const uint32_t m = brick_word(tl, coarse);
  if (threadIdx.x == 0) bricks[blockIdx.x] = m;
}

// One 64-lane workgroup per 8x8 pixel packet of one pose (neighbouring rays share tiles and
// words).  Outputs per pixel: depth (rayTraceVolume's value of the surface voxel, k_zbuffer's
// arithmetic; -1 = none) and cell (getHashId; all ones = none); either may be null.  stats (may
// be null): {rays with a non-empty sequence, rays with a surface cell}.
template <bool JUMP>
__global__ __launch_bounds__(64) void k_rc_cast(Geom g, GridTiles tl, CamP cam, const PoseX* __restrict__ poses,
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
  Walk W(R);
  const bool entered = W.left > 0;
  bool found = false, tile_solid = false, brick_solid = false;
  uint32_t last_t = 0xffffffffu, last_b = 0xffffffffu, last_w = 0xffffffffu, word = 0;
  while (W.left > 0) {
    const uint32_t t = occ_tile(tl.nty, tl.ntz, W.c0, W.c1, W.c2);
    if (t != last_t) {
      last_t = t;
      if (JUMP) {  // (the cell-by-cell walk has no use for the brick level: it would only add a test)
        const uint32_t b = occ_brick(tl, W.c0, W.c1, W.c2);
        if (b != last_b) {
          last_b = b;
          brick_solid = (bricks[b >> 5] >> (b & 31u)) & 1u;
        }
      }
      tile_solid = (!JUMP || brick_solid) && ((coarse[t >> 5] >> (t & 31u)) & 1u);
      if (JUMP && !tile_solid) {
        // every cell up to the crossing that leaves the empty cube is empty
        const int n = rc_jump(brick_solid ? 7 : 31, W);
        if (n >= W.left) break;  // the ray ends inside it
        W.left -= n;
        continue;
      }
    }
    if (tile_solid) {
      const uint32_t bit = occ_index(tl.nty, tl.ntz, W.c0, W.c1, W.c2), wi = bit >> 5;
      if (wi != last_w) {
        last_w = wi;
        word = fine[wi];
      }
      if ((word >> (bit & 31u)) & 1u) {
        found = true;
        break;
      }
    }
    if (--W.left == 0) break;
    W.step();
  }
  if (in_image) {
    int32_t d = -1;
    uint64_t h = ~0ull;
    if (found) {
      h = hash_id(W.c0, W.c1, W.c2);
      float cen[3], tc[3];
      cell_centre(g, W.c0, W.c1, W.c2, cen);
      xform(T.i, cen[0], cen[1], cen[2], tc);
      d = to_int_x86((double)roundf(tc[2] * 1000.0f));  // k_zbuffer's depth of the voxel centre
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
int check_raycast(const dmf_volume* v, const dmf_camera* cam, const void* logodds, const void* poses, int32_t P,
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
  const GridTiles tl = grid_tiles(g.n);
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
  hipLaunchKernelGGL(k_rc_mask, dim3(ncoarse), dim3(kMaskThreads), 0, v->stream, g, tl, d_logodds, threshold,
                     (uint32_t*)fine, (uint32_t*)coarse);
  DMF_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_rc_bricks, dim3(nbw), dim3(64), 0, v->stream, tl, (const uint32_t*)coarse, bricks);
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
  DMF_TRY(upload_grid(v, logodds, &dl));
  DMF_TRY(scratch(v, kScHost2, sizeof(float) * 12 * (size_t)P, &dp));
  if (depth) DMF_TRY(scratch(v, kScOut0, sizeof(int32_t) * n, &dd));
  if (cell) DMF_TRY(scratch(v, kScOut1, sizeof(uint64_t) * n, &dc));
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
