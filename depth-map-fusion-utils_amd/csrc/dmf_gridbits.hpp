// dmf_gridbits.hpp — the occupancy bitmask's 8x8x8-tile layout and the step from an int16 log-odds
// grid to threshold bits, shared by the point-cloud occupancy (occ_bit, dmf_internal.hpp) and the
// fused grid's consumers (dmf_raycast.hip, dmf_surface.hip, dmf_distance.hip, dmf_travel.hip): the
// tile counts of a grid, cell -> tile and bit index, the 8-cell loaders (int16 log-odds, uint32
// distance field), and the tile mask pass.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dmf_geom.hpp"

namespace dmf {

// Layout: 8x8x8-cell tiles of 512 bits (16 words = 64 B), tiles x-major over the grid padded to
// whole tiles.  Word w of a tile holds x & 7 = w >> 1 and the four y rows (w & 1) * 4 .. + 3, one
// byte of 8 z-cells each: bit (x & 7) * 64 + (y & 7) * 8 + (z & 7) of the tile.
__host__ __device__ inline uint32_t tiles8(int n) { return ((uint32_t)n + 7u) >> 3; }

struct GridTiles {
  uint32_t ntx, nty, ntz, ntiles;  // 8x8x8-cell tiles per axis and in all
  uint32_t nby, nbz, nbricks;      // 32^3-cell bricks (4x4x4 tiles) along y and z, and in all (x-major likewise)
};
inline GridTiles grid_tiles(const int n[3]) {
  const uint32_t ntx = tiles8(n[0]), nty = tiles8(n[1]), ntz = tiles8(n[2]);
  const uint32_t nbx = (ntx + 3u) >> 2, nby = (nty + 3u) >> 2, nbz = (ntz + 3u) >> 2;
  return GridTiles{ntx, nty, ntz, ntx * nty * ntz, nby, nbz, nbx * nby * nbz};
}

// Cell -> tile index, -> bit index in the mask (word = index >> 5, bit of the word = index & 31),
// and -> brick index (the level over the tile bits).
__host__ __device__ inline uint32_t occ_tile(uint32_t nty, uint32_t ntz, int x, int y, int z) {
  return (((uint32_t)x >> 3) * nty + ((uint32_t)y >> 3)) * ntz + ((uint32_t)z >> 3);
}
__host__ __device__ inline uint32_t occ_index(uint32_t nty, uint32_t ntz, int x, int y, int z) {
  return (occ_tile(nty, ntz, x, y, z) << 9) | (((uint32_t)x & 7u) << 6) | (((uint32_t)y & 7u) << 3) |
         ((uint32_t)z & 7u);
}
__device__ inline uint32_t occ_brick(const GridTiles& tl, int x, int y, int z) {
  return (((uint32_t)x >> 5) * tl.nby + ((uint32_t)y >> 5)) * tl.nbz + ((uint32_t)z >> 5);
}

// Up to 8 consecutive int16 cells at p, of which the first nvalid exist: f(k, value) for each of
// them, in order.  One 16-B load when all 8 exist and p is 16-B aligned (a grid base that is not
// makes every group take the cell-by-cell loop); cells past nvalid are not read.
template <class F>
__device__ inline void for_cells8(const int16_t* __restrict__ p, int nvalid, F&& f) {
  if (nvalid >= 8 && ((uintptr_t)p & 15) == 0) {
    const uint4 q = *(const uint4*)p;
    const uint32_t u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      f(2 * k, (int)(int16_t)(u[k] & 0xffffu));
      f(2 * k + 1, (int)(int16_t)(u[k] >> 16));
    }
  } else {
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)  // (the rare path: kept small)
    for (int k = 0; k < 8 && k < nvalid; ++k) f(k, (int)p[k]);
  }
}

// The uint32 counterpart (the distance field's cells): up to 4 consecutive cells at p, of which
// the first nvalid exist, in one 16-B load when all 4 exist and p is 16-B aligned; and 8 cells as
// two such groups, so that the tile mask pass reads either grid.
template <class F>
__device__ inline void for_cells4(const uint32_t* __restrict__ p, int nvalid, F&& f) {
  if (nvalid >= 4 && ((uintptr_t)p & 15) == 0) {
    const uint4 q = *(const uint4*)p;
    f(0, q.x);
    f(1, q.y);
    f(2, q.z);
    f(3, q.w);
  } else {
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)  // (the rare path: kept small)
    for (int k = 0; k < 4 && k < nvalid; ++k) f(k, p[k]);
  }
}
template <class F>
__device__ inline void for_cells8(const uint32_t* __restrict__ p, int nvalid, F&& f) {
  for_cells4(p, nvalid, f);
  if (nvalid > 4) for_cells4(p + 4, nvalid - 4, [&](int k, uint32_t c) { f(k + 4, c); });
}

// The tile mask pass: NM 1-bit-per-cell masks of an int16 (or uint32) grid in the layout above, one
// streaming pass.  One workgroup of kMaskThreads per 32 consecutive tiles = 512 words of each mask.
// Thread (tile j = i & 31, word w = i >> 5) reads the word's 4 y-rows of 8 z-cells (16 B each): a
// wave's loads are 2 x 4 rows of up to 512 contiguous bytes.  classify(value, k, b) sets bit k of
// b[m] where the cell belongs to mask m; cells past the grid (partial tiles) belong to none.  The
// words go through LDS so that the workgroup's NM x 2 KiB are stored in order, out[m][word index].
// word[] returns the thread's own words (tile j, word w); the call holds one workgroup barrier.
constexpr int kMaskThreads = 512;
template <int NM, class T, class F>
__device__ inline void tile_mask_pass(const Geom& g, const GridTiles& tl, const T* __restrict__ L,
                                      uint32_t* const (&out)[NM], uint32_t (&word)[NM], F&& classify) {
  __shared__ uint32_t sw[NM][kMaskThreads];
  const int i = threadIdx.x, j = i & 31, w = i >> 5;
  const uint32_t t = blockIdx.x * 32u + (uint32_t)j;
  for (int m = 0; m < NM; ++m) word[m] = 0;
  if (t < tl.ntiles) {
    const uint32_t tz = t % tl.ntz, r = t / tl.ntz;
    const int x = (int)(r / tl.nty) * 8 + (w >> 1), y0 = (int)(r % tl.nty) * 8 + (w & 1) * 4, z0 = (int)tz * 8;
    if (x < g.n[0]) {
#pragma unroll
      for (int dy = 0; dy < 4; ++dy) {
        const int y = y0 + dy;
        if (y < g.n[1]) {
          uint32_t b[NM] = {};
          for_cells8(L + (((int64_t)x * g.n[1] + y) * g.n[2] + z0), g.n[2] - z0,
                     [&](int k, auto c) { classify(c, k, b); });
          for (int m = 0; m < NM; ++m) word[m] |= b[m] << (8 * dy);
        }
      }
    }
  }
  for (int m = 0; m < NM; ++m) sw[m][j * 16 + w] = word[m];
  __syncthreads();
  const uint32_t o = blockIdx.x * (uint32_t)kMaskThreads + (uint32_t)i;
  if (o < tl.ntiles * 16u) {
    for (int m = 0; m < NM; ++m) out[m][o] = sw[m][i];
  }
}

// One word of the brick level over a tile level: lane k < 32 of a 64-lane workgroup ORs the 4x4x4
// tile bits of brick 32 * block + k (tiles past the grid's last tile row are absent); every lane
// returns the word.
__device__ inline uint32_t brick_word(const GridTiles& tl, const uint32_t* __restrict__ coarse) {
  const uint32_t b = blockIdx.x * 32u + (threadIdx.x & 31u);
  bool any = false;
  if (threadIdx.x < 32 && b < tl.nbricks) {
    const uint32_t bz = b % tl.nbz, r = b / tl.nbz, by = r % tl.nby, bx = r / tl.nby;
    for (uint32_t dx = 0; dx < 4; ++dx)
      for (uint32_t dy = 0; dy < 4; ++dy) {
        const uint32_t tx = bx * 4 + dx, ty = by * 4 + dy;
        if (tx >= tl.ntx || ty >= tl.nty) continue;
        for (uint32_t tz = bz * 4; tz < bz * 4 + 4 && tz < tl.ntz; ++tz) {
          const uint32_t t = (tx * tl.nty + ty) * tl.ntz + tz;
          any |= (coarse[t >> 5] >> (t & 31u)) & 1u;
        }
      }
  }
  return (uint32_t)__builtin_amdgcn_ballot_w64(any);
}

}  // namespace dmf
