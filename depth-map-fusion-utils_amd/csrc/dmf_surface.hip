// dmf_surface.hip — the fused grid's surface as an oriented cloud, in order (DESIGN.md §4.2,
// §5.12): the cells of an int16 log-odds grid that are solid (L >= occ_threshold) and have a free
// (L <= free_threshold) face neighbour, in ascending x-major cell index (= ascending getHashId),
// each with its hash, voxel centre and a normal from the face neighbours' log-odds.  An ordered,
// exact stream compaction in which almost every cell is rejected:
//  k_sf_mask    — one streaming pass over the grid (the tile mask pass of dmf_gridbits.hpp, shared
//                 with dmf_raycast.hip): the solid and the free 1-bit-per-cell masks in the
//                 occupancy bitmask's 8x8x8-tile layout, and the number of solid cells;
//  k_sf_surface — bit level: surface = solid & (free shifted along -x, +x, -y, +y, -z, +z), the
//                 shifts carried across words and tiles; the surface mask, and the number of
//                 surface cells of every (x, y) row of the grid (the unit of the output order);
//  (rocPRIM)    — exclusive scan of the row counts: each row's first output position;
//  k_sf_emit    — one workgroup per tile column (8 x 8 rows): the rank of every surface bit in its
//                 row from the surface words' byte popcounts; for set bits only, the six
//                 neighbours' int16 values, then hash, centre and normal at base + rank < cap.
// The grid is read once in full and once more around the surface cells; the bit passes work on
// 1/16 of its bytes.
#include "dmf_host.hpp"

namespace dmf {

// The mask pass (tile_mask_pass, dmf_gridbits.hpp) with two masks, solid and free, and the number
// of solid cells.  Cells past the grid (partial tiles) are neither solid nor free.
__global__ __launch_bounds__(kMaskThreads) void k_sf_mask(Geom g, GridTiles tl, const int16_t* __restrict__ L,
                                                          int occ_thr, int free_thr, uint32_t* __restrict__ solid,
                                                          uint32_t* __restrict__ free_,
                                                          unsigned long long* __restrict__ nsolid) {
  __shared__ uint32_t scount;
  const int i = threadIdx.x;
  if (i == 0) scount = 0;
  uint32_t* const out[2] = {solid, free_};
  uint32_t word[2];
  tile_mask_pass<2>(g, tl, L, out, word, [=](int c, int k, uint32_t (&b)[2]) {
    b[0] |= (uint32_t)(c >= occ_thr) << k;
    b[1] |= (uint32_t)(c <= free_thr) << k;
  });
  uint32_t c = (uint32_t)__popc(word[0]);
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
  if ((i & 63) == 0 && c) atomicAdd(&scount, c);
  __syncthreads();
  if (i == 0 && scount) atomicAdd(nsolid, (unsigned long long)scount);
}

// A tile column (tx, ty) is the 8 x 8 (x, y) rows of the tiles (tx, ty, 0 .. ntz - 1).  Thread
// (word w = i & 15, tile i >> 4 of a chunk of kSfChunk tiles): a wave reads 4 whole tiles, 256
// contiguous bytes of a mask.  Word w of a tile holds x & 7 = w >> 1 and the four y rows
// (w & 1) * 4 .. + 3, one byte of 8 z-cells each.
constexpr int kSfThreads = 256, kSfChunk = kSfThreads / 16;

// The surface word of (tile t = (tx, ty, tz), word w): the solid bits with a free face neighbour.
// A neighbour word outside the grid's tiles contributes no bit.
__device__ inline uint32_t sf_word(const GridTiles& tl, const uint32_t* __restrict__ solid,
                                   const uint32_t* __restrict__ free_, uint32_t tx, uint32_t ty, uint32_t tz, uint32_t t,
                                   uint32_t w) {
  const uint32_t s = solid[t * 16u + w];
  if (s == 0u) return 0u;
  const uint32_t F = free_[t * 16u + w];
  // z: bits of a byte; bit 7 of the tile below and bit 0 of the tile above carry in
  const uint32_t Fzm = tz > 0u ? free_[(t - 1u) * 16u + w] : 0u;
  const uint32_t Fzp = tz + 1u < tl.ntz ? free_[(t + 1u) * 16u + w] : 0u;
  uint32_t nb = ((F & 0x7f7f7f7fu) << 1) | ((Fzm >> 7) & 0x01010101u);
  nb |= ((F >> 1) & 0x7f7f7f7fu) | ((Fzp & 0x01010101u) << 7);
  // y: bytes of a word; the other word of the same x, in this tile or in the tile beside it
  uint32_t Fym, Fyp;
  if (w & 1u) {
    Fym = free_[t * 16u + w - 1u];
    Fyp = ty + 1u < tl.nty ? free_[(t + tl.ntz) * 16u + w - 1u] : 0u;
  } else {
    Fym = ty > 0u ? free_[(t - tl.ntz) * 16u + w + 1u] : 0u;
    Fyp = free_[t * 16u + w + 1u];
  }
  nb |= (F << 8) | (Fym >> 24);
  nb |= (F >> 8) | (Fyp << 24);
  // x: whole words
  const uint32_t xs = tl.nty * tl.ntz;
  nb |= (w >> 1) > 0u ? free_[t * 16u + w - 2u] : (tx > 0u ? free_[(t - xs) * 16u + w + 14u] : 0u);
  nb |= (w >> 1) < 7u ? free_[t * 16u + w + 2u] : (tx + 1u < tl.ntx ? free_[(t + xs) * 16u + w - 14u] : 0u);
  return s & nb;
}

// One workgroup per tile column: the surface words, and counts[x * ydim + y] for the column's
// rows inside the grid (every row of the grid is written by exactly one workgroup).
__global__ __launch_bounds__(kSfThreads) void k_sf_surface(Geom g, GridTiles tl, const uint32_t* __restrict__ solid,
                                                           const uint32_t* __restrict__ free_,
                                                           uint32_t* __restrict__ surf, int32_t* __restrict__ counts) {
  __shared__ uint32_t cnt[64];
  const uint32_t i = threadIdx.x, w = i & 15u;
  const uint32_t tx = blockIdx.x / tl.nty, ty = blockIdx.x % tl.nty;
  if (i < 64u) cnt[i] = 0;
  __syncthreads();
  const uint32_t row0 = (w >> 1) * 8u + (w & 1u) * 4u;
  for (uint32_t tz = i >> 4; tz < tl.ntz; tz += (uint32_t)kSfChunk) {
    const uint32_t t = (tx * tl.nty + ty) * tl.ntz + tz;
    const uint32_t s = sf_word(tl, solid, free_, tx, ty, tz, t, w);
    surf[t * 16u + w] = s;
    if (s) {
#pragma unroll
      for (uint32_t b = 0; b < 4u; ++b) {
        const uint32_t c = (uint32_t)__popc((s >> (8u * b)) & 0xffu);
        if (c) atomicAdd(&cnt[row0 + b], c);
      }
    }
  }
  __syncthreads();
  if (i < 64u) {
    const int x = (int)(tx * 8u + (i >> 3)), y = (int)(ty * 8u + (i & 7u));
    if (x < g.n[0] && y < g.n[1]) counts[(int64_t)x * g.n[1] + y] = (int32_t)cnt[i];
  }
}

// {surface cells, solid cells} of the grid: the scan's total and the mask pass's counter.
__global__ void k_sf_totals(const int32_t* __restrict__ bases, int64_t nrows,
                            const unsigned long long* __restrict__ nsolid, unsigned long long* __restrict__ count) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    count[0] = (unsigned long long)bases[nrows];
    count[1] = *nsolid;
  }
}

// One workgroup per tile column.  The rank of a surface bit in its (x, y) row = the set bits of
// the row's bytes in the tiles below it + those below it in its byte.  The four byte popcounts
// of a word travel as four 16-bit fields (a row has at most 2048 cells): an inclusive scan over
// the lanes of equal w (stride 16) in the wave, the waves' totals through LDS, the chunks' totals
// in a register.  bases = the exclusive scan of the row counts.
__global__ __launch_bounds__(kSfThreads) void k_sf_emit(Geom g, GridTiles tl, const int16_t* __restrict__ L,
                                                        const uint32_t* __restrict__ surf,
                                                        const int32_t* __restrict__ bases, int64_t cap,
                                                        uint64_t* __restrict__ hash, float* __restrict__ xyz,
                                                        float* __restrict__ nrm) {
  __shared__ int32_t rbase[64];
  __shared__ unsigned long long wtot[kSfThreads / 64][16];
  const uint32_t i = threadIdx.x, w = i & 15u, lane = i & 63u, wave = i >> 6;
  const uint32_t tx = blockIdx.x / tl.nty, ty = blockIdx.x % tl.nty;
  int any = 0;
  if (i < 64u) {
    const int x = (int)(tx * 8u + (i >> 3)), y = (int)(ty * 8u + (i & 7u));
    int32_t b = 0;
    if (x < g.n[0] && y < g.n[1]) {
      const int64_t r = (int64_t)x * g.n[1] + y;
      b = bases[r];
      any = bases[r + 1] > b;
    }
    rbase[i] = b;
  }
  if (!__syncthreads_or(any)) return;  // no surface cell in the column: L is not touched
  const int x = (int)(tx * 8u + (w >> 1)), yw = (int)(ty * 8u + (w & 1u) * 4u);
  const uint32_t row0 = (w >> 1) * 8u + (w & 1u) * 4u;
  const int64_t sx = (int64_t)g.n[1] * g.n[2], sy = g.n[2];
  unsigned long long carry = 0;
  for (uint32_t tz0 = 0; tz0 < tl.ntz; tz0 += (uint32_t)kSfChunk) {
    const uint32_t tz = tz0 + (i >> 4);
    uint32_t s = 0;
    if (tz < tl.ntz) s = surf[((tx * tl.nty + ty) * tl.ntz + tz) * 16u + w];
    const unsigned long long p = (unsigned long long)__popc(s & 0xffu) | (unsigned long long)__popc(s & 0xff00u) << 16 |
                                 (unsigned long long)__popc(s & 0xff0000u) << 32 |
                                 (unsigned long long)__popc(s & 0xff000000u) << 48;
    unsigned long long v = p, u = __shfl_up(v, 16, 64);
    if (lane >= 16u) v += u;
    u = __shfl_up(v, 32, 64);
    if (lane >= 32u) v += u;
    if (lane >= 48u) wtot[wave][w] = v;
    __syncthreads();
    unsigned long long before = carry + (v - p);
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)(kSfThreads / 64); ++k) {
      const unsigned long long tk = wtot[k][w];
      if (k < wave) before += tk;
      carry += tk;
    }
    __syncthreads();  // (the next chunk overwrites wtot)
    const uint32_t word = s;
    while (s) {
      const uint32_t k = (uint32_t)__ffs((int)s) - 1u, yb = k >> 3;
      const uint32_t below = (uint32_t)__popc(word & ((1u << k) - 1u) & (0xffu << (8u * yb)));
      s &= s - 1u;
      const int64_t rank = (int64_t)rbase[row0 + yb] + (int64_t)((before >> (16u * yb)) & 0xffffu) + below;
      if (rank >= cap) continue;
      const int y = yw + (int)yb, z = (int)(tz * 8u + (k & 7u));
      const int64_t c = ((int64_t)x * g.n[1] + y) * g.n[2] + z;
      // N(c - e_a) - N(c + e_a); outside the grid 0
      const int gx = (x > 0 ? (int)L[c - sx] : 0) - (x + 1 < g.n[0] ? (int)L[c + sx] : 0);
      const int gy = (y > 0 ? (int)L[c - sy] : 0) - (y + 1 < g.n[1] ? (int)L[c + sy] : 0);
      const int gz = (z > 0 ? (int)L[c - 1] : 0) - (z + 1 < g.n[2] ? (int)L[c + 1] : 0);
      if (hash) hash[rank] = hash_id(x, y, z);
      if (xyz) {
        float cen[3];
        cell_centre(g, x, y, z, cen);
        xyz[3 * rank] = cen[0];
        xyz[3 * rank + 1] = cen[1];
        xyz[3 * rank + 2] = cen[2];
      }
      if (nrm) {
        float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
        if (gx | gy | gz) {
          const float a = (float)gx, b = (float)gy, d = (float)gz;
          const float q = sqrtf(sum3(a * a, b * b, d * d));
          n0 = a / q; n1 = b / q; n2 = d / q;
        }
        nrm[3 * rank] = n0;
        nrm[3 * rank + 1] = n1;
        nrm[3 * rank + 2] = n2;
      }
    }
  }
}

// The plain arguments first (no access to the volume: they are rejected without a device).
static int check_surface_args(const dmf_volume* v, const void* logodds, int64_t cap) {
  if (!v || !logodds) return fail(DMF_ERR_INVALID, "null argument");
  if (cap < 0) return fail(DMF_ERR_INVALID, "negative capacity %lld", (long long)cap);
  return DMF_OK;
}
static const char kSfGridLimit[] = "surface extraction is limited to 2048 cells per axis";

// Masks, row counts and their scan (left in the volume's scratch for surface_emit);
// d_count[2] = {surface cells, solid cells}.
int surface_count(dmf_volume* v, const int16_t* d_logodds, int32_t occ, int32_t free_thr, uint64_t* d_count) {
  const Geom g = v->geom();
  const GridTiles tl = grid_tiles(g.n);
  const size_t words = 16 * (size_t)tl.ntiles;
  const int64_t nrows = (int64_t)g.n[0] * g.n[1];
  void *solid, *free_, *surf, *counts, *bases, *tot;
  DMF_TRY(scratch(v, kScSfSolid, sizeof(uint32_t) * words, &solid));
  DMF_TRY(scratch(v, kScSfFree, sizeof(uint32_t) * words, &free_));
  DMF_TRY(scratch(v, kScSfSurf, sizeof(uint32_t) * words, &surf));
  DMF_TRY(scratch(v, kScSfCounts, sizeof(int32_t) * (size_t)(nrows + 1), &counts));
  DMF_TRY(scratch(v, kScSfBases, sizeof(int32_t) * (size_t)(nrows + 1), &bases));
  DMF_TRY(scratch(v, kScSfTotals, sizeof(unsigned long long), &tot));
  DMF_HIP(hipMemsetAsync(tot, 0, sizeof(unsigned long long), v->stream));
  DMF_HIP(hipMemsetAsync((int32_t*)counts + nrows, 0, sizeof(int32_t), v->stream));
  hipLaunchKernelGGL(k_sf_mask, dim3((tl.ntiles + 31u) / 32u), dim3(kMaskThreads), 0, v->stream, g, tl, d_logodds,
                     occ, free_thr, (uint32_t*)solid, (uint32_t*)free_, (unsigned long long*)tot);
  DMF_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_sf_surface, dim3(tl.ntx * tl.nty), dim3(kSfThreads), 0, v->stream, g, tl,
                     (const uint32_t*)solid, (const uint32_t*)free_, (uint32_t*)surf, (int32_t*)counts);
  DMF_LAUNCH_CHECK();
  DMF_TRY(exclusive_scan_i32(v, (const int32_t*)counts, (int32_t*)bases, (size_t)(nrows + 1)));
  hipLaunchKernelGGL(k_sf_totals, dim3(1), dim3(64), 0, v->stream, (const int32_t*)bases, nrows,
                     (const unsigned long long*)tot, (unsigned long long*)d_count);
  DMF_LAUNCH_CHECK();
  return DMF_OK;
}

// After surface_count on the same grid: the first min(count, cap) entries of the given outputs.
int surface_emit(dmf_volume* v, const int16_t* d_logodds, uint64_t* d_hash, float* d_xyz, float* d_nrm,
                        int64_t cap) {
  if (cap <= 0 || (!d_hash && !d_xyz && !d_nrm)) return DMF_OK;
  const Geom g = v->geom();
  const GridTiles tl = grid_tiles(g.n);
  void *surf, *bases;
  DMF_TRY(scratch(v, kScSfSurf, 0, &surf));
  DMF_TRY(scratch(v, kScSfBases, 0, &bases));
  hipLaunchKernelGGL(k_sf_emit, dim3(tl.ntx * tl.nty), dim3(kSfThreads), 0, v->stream, g, tl, d_logodds,
                     (const uint32_t*)surf, (const int32_t*)bases, cap, d_hash, d_xyz, d_nrm);
  DMF_LAUNCH_CHECK();
  return DMF_OK;
}

// Upload the host grid, count, and read the counts back (synchronises).
int surface_count_host(dmf_volume* v, const int16_t* logodds, int32_t occ, int32_t free_thr, void** d_grid,
                              uint64_t cnt[2]) {
  void* dc;
  DMF_TRY(upload_grid(v, logodds, d_grid));
  DMF_TRY(scratch(v, kScOut3, sizeof(uint64_t) * 2, &dc));
  DMF_TRY(surface_count(v, (const int16_t*)*d_grid, occ, free_thr, (uint64_t*)dc));
  DMF_HIP(hipMemcpyAsync(cnt, dc, sizeof(uint64_t) * 2, hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipStreamSynchronize(v->stream));
  return DMF_OK;
}

}  // namespace dmf

using namespace dmf;

extern "C" {

int dmf_grid_surface_device(dmf_volume* v, const int16_t* d_logodds, int32_t occ_threshold, int32_t free_threshold,
                            uint64_t* d_hash, float* d_xyz, float* d_normals, int64_t cap, uint64_t* d_count) {
  DMF_API_BEGIN
  DMF_TRY(check_surface_args(v, d_logodds, cap));
  if (!d_count) return fail(DMF_ERR_INVALID, "null d_count");
  if (!d_hash && !d_xyz && !d_normals) return fail(DMF_ERR_INVALID, "every output is null");
  DMF_TRY(require_grid_2048(v, kSfGridLimit));
  DMF_TRY(surface_count(v, d_logodds, occ_threshold, free_threshold, d_count));
  return surface_emit(v, d_logodds, d_hash, d_xyz, d_normals, cap);
  DMF_API_END
}

int dmf_grid_surface(dmf_volume* v, const int16_t* logodds, int32_t occ_threshold, int32_t free_threshold,
                     uint64_t* hash, float* xyz, float* normals, int64_t cap, int64_t* n, int64_t* n_solid) {
  DMF_API_BEGIN
  DMF_TRY(check_surface_args(v, logodds, cap));
  DMF_TRY(require_grid_2048(v, kSfGridLimit));
  void* dl;
  uint64_t cnt[2] = {0, 0};
  DMF_TRY(surface_count_host(v, logodds, occ_threshold, free_threshold, &dl, cnt));
  const int64_t m = (int64_t)cnt[0];
  if (n) *n = m;
  if (n_solid) *n_solid = (int64_t)cnt[1];
  const bool outputs = hash || xyz || normals;
  if (cap < m) {
    if (cap == 0 && !outputs) return DMF_OK;  // the size query
    return fail(DMF_ERR_CAPACITY, "need %lld entries", (long long)m);
  }
  if (m == 0 || !outputs) return DMF_OK;
  void *dh = nullptr, *dx = nullptr, *dn = nullptr;
  if (hash) DMF_TRY(scratch(v, kScSfHash, sizeof(uint64_t) * (size_t)m, &dh));
  if (xyz) DMF_TRY(scratch(v, kScSfXyz, sizeof(float) * 3 * (size_t)m, &dx));
  if (normals) DMF_TRY(scratch(v, kScSfNrm, sizeof(float) * 3 * (size_t)m, &dn));
  DMF_TRY(surface_emit(v, (const int16_t*)dl, (uint64_t*)dh, (float*)dx, (float*)dn, m));
  if (hash) DMF_HIP(hipMemcpyAsync(hash, dh, sizeof(uint64_t) * (size_t)m, hipMemcpyDeviceToHost, v->stream));
  if (xyz) DMF_HIP(hipMemcpyAsync(xyz, dx, sizeof(float) * 3 * (size_t)m, hipMemcpyDeviceToHost, v->stream));
  if (normals) DMF_HIP(hipMemcpyAsync(normals, dn, sizeof(float) * 3 * (size_t)m, hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipStreamSynchronize(v->stream));
  return DMF_OK;
  DMF_API_END
}

int dmf_volume_integrate_surface(dmf_volume* v, const int16_t* logodds, int32_t occ_threshold, int32_t free_threshold,
                                 int64_t* n) {
  DMF_API_BEGIN
  DMF_TRY(check_surface_args(v, logodds, 0));
  DMF_TRY(require_grid_2048(v, kSfGridLimit));
  void* dl;
  uint64_t cnt[2] = {0, 0};
  DMF_TRY(surface_count_host(v, logodds, occ_threshold, free_threshold, &dl, cnt));
  const int64_t m = (int64_t)cnt[0];
  if (n) *n = m;
  if (m == 0) return DMF_OK;
  // (the integration's own scratch is kScOut0..3 and kScHost1..2: the cloud lives in slots of its own)
  void *dx, *dn;
  DMF_TRY(scratch(v, kScSfXyz, sizeof(float) * 3 * (size_t)m, &dx));
  DMF_TRY(scratch(v, kScSfNrm, sizeof(float) * 3 * (size_t)m, &dn));
  DMF_TRY(surface_emit(v, (const int16_t*)dl, nullptr, (float*)dx, (float*)dn, m));
  return dmf_volume_integrate_device(v, (const float*)dx, (const float*)dn, m);
  DMF_API_END
}

}  // extern "C"
