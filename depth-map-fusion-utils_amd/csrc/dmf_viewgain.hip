// dmf_viewgain.hip — view gain over a fused log-odds grid and next-best-view selection on gfx950
// (DESIGN.md §4.5, §5.15).  Which cells that nobody has observed yet would a camera at pose p see?
// Cell classes of the int16 grid: solid (L >= occ), free (not solid, L <= free), unknown (neither).
// Per pixel the ray-cast's own cell sequence (§4.1) up to its first solid cell; seen[p] = the
// unknown cells of those stretches as a bitmask in the occupancy layout (dmf_gridbits.hpp), which
// is what greedy_cover (dmf_cover.hip) takes.  Kernels:
//  k_vg_mask   — tile_mask_pass<2>: the solid and the unknown mask in one pass over the grid, and
//                one word per workgroup of two tile levels: "holds a solid cell" and "holds a solid
//                or an unknown cell" (not wholly free);
//  k_vg_bricks — the brick level over each of the two tile levels (brick_word);
//  k_vg_cast   — one lane per pixel, 64 lanes = one 8x8 packet of one pose (k_rc_cast's shape).
//                <false>: cell by cell, one atomic OR per unknown visible cell (the A/B reference).
//                <true>: a wholly free brick or tile is left in one rc_jump; a tile without a solid
//                cell is walked on the unknown word alone; the bits of the current mask word are
//                collected in a register and leave in one atomic OR when the word changes or the
//                ray ends (none when there are no bits); <true, true>, the default, reads the mask
//                word first and skips an atomic that would add nothing (rays of a packet share
//                most of their cells: 13 visits per distinct cell on the bench scene, §5.15);
//  k_vg_count  — gain[p] = popcount of seen[p].
#include <algorithm>

#include "dmf_dda.hpp"
#include "dmf_host.hpp"

namespace dmf {

constexpr int kVgDefaultWalk = 3;  // DMF_KNOB_VIEWGAIN_WALK = 0 (measured: DESIGN.md §5.15)
constexpr size_t kVgBatchBytes = (size_t)256 << 20;  // the scratch masks of one internal pose batch

// fine[0] = solid, fine[1] = unknown; coarse_s / coarse_n: bit j = tile 32 * block + j holds a
// solid / a solid or unknown cell.  Solid wins where the thresholds cross.
__global__ __launch_bounds__(kMaskThreads) void k_vg_mask(Geom g, GridTiles tl, const int16_t* __restrict__ L, int occ,
                                                          int free_, uint32_t* __restrict__ solid,
                                                          uint32_t* __restrict__ unknown,
                                                          uint32_t* __restrict__ coarse_s,
                                                          uint32_t* __restrict__ coarse_n) {
  __shared__ uint32_t sany[2][16];
  uint32_t* const out[2] = {solid, unknown};
  uint32_t word[2];
  tile_mask_pass<2>(g, tl, L, out, word, [=](int c, int k, uint32_t (&b)[2]) {
    const bool s = c >= occ;
    b[0] |= (uint32_t)s << k;
    b[1] |= (uint32_t)(!s && c > free_) << k;
  });
  // a wave holds words 2k (lanes 0-31) and 2k + 1 (lanes 32-63) of the 32 tiles
  const int i = threadIdx.x, w = i >> 5;
  const uint64_t any_s = __builtin_amdgcn_ballot_w64(word[0] != 0u);
  const uint64_t any_n = __builtin_amdgcn_ballot_w64((word[0] | word[1]) != 0u);
  if ((i & 63) == 0) {
    sany[0][w] = (uint32_t)any_s;
    sany[0][w + 1] = (uint32_t)(any_s >> 32);
    sany[1][w] = (uint32_t)any_n;
    sany[1][w + 1] = (uint32_t)(any_n >> 32);
  }
  __syncthreads();
  if (i < 2) {
    uint32_t a = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) a |= sany[i][k];
    (i ? coarse_n : coarse_s)[blockIdx.x] = a;
  }
}

// blockIdx.y = level: the level's tile words at coarse + y * ncoarse, its brick words at bricks + y * nbw
__global__ __launch_bounds__(64) void k_vg_bricks(GridTiles tl, const uint32_t* __restrict__ coarse, uint32_t ncoarse,
                                                  uint32_t* __restrict__ bricks, uint32_t nbw) {
  const uint32_t m = brick_word(tl, coarse + (size_t)blockIdx.y * ncoarse);
  if (threadIdx.x == 0) bricks[(size_t)blockIdx.y * nbw + blockIdx.x] = m;
}

__device__ inline void vg_or(uint32_t* p, uint32_t bits) {
  __hip_atomic_fetch_or(p, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// seen: this launch's first pose's mask, words32 uint32 per pose (bit i of the layout = bit i & 31
// of word i >> 5: the uint64 words of the ABI, little-endian).  TEST (with ACC): the word is read
// first and the atomic skipped when it already holds the bits (a stale read only costs the atomic).
// stats (may be null): {rays with a non-empty sequence, rays stopped by a solid cell, unknown
// visible cells over all rays}.
template <bool ACC, bool TEST>
__global__ __launch_bounds__(64) void k_vg_cast(Geom g, GridTiles tl, CamP cam, const PoseX* __restrict__ poses,
                                                int range_mm, int packets_x, const uint32_t* __restrict__ solid,
                                                const uint32_t* __restrict__ unknown,
                                                const uint32_t* __restrict__ coarse_s,
                                                const uint32_t* __restrict__ coarse_n,
                                                const uint32_t* __restrict__ bricks_n, uint32_t* __restrict__ seen,
                                                size_t words32, unsigned long long* __restrict__ stats) {
  stats = stat_slot(stats);
  const int l = threadIdx.x;
  const int pr = (blockIdx.x / packets_x) * 8 + (l >> 3), pc = (blockIdx.x % packets_x) * 8 + (l & 7);
  const bool in_image = pr < cam.H && pc < cam.W;
  const PoseX& T = poses[blockIdx.y];
  uint32_t* const mine = seen + (size_t)blockIdx.y * words32;
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
  bool stopped = false, tile_n = false, tile_s = false, brick_n = false;
  uint32_t last_t = 0xffffffffu, last_b = 0xffffffffu, last_w = 0xffffffffu, sword = 0, uword = 0;
  uint32_t acc = 0, visits = 0;  // acc: the unknown visible bits of word last_w not yet written
  auto flush = [&]() {
    if (ACC && acc) {
      if (!TEST || (mine[last_w] & acc) != acc) vg_or(mine + last_w, acc);
      acc = 0;
    }
  };
  while (W.left > 0) {
    const uint32_t t = occ_tile(tl.nty, tl.ntz, W.c0, W.c1, W.c2);
    if (t != last_t) {
      last_t = t;
      if (ACC) {
        const uint32_t b = occ_brick(tl, W.c0, W.c1, W.c2);
        if (b != last_b) {
          last_b = b;
          brick_n = (bricks_n[b >> 5] >> (b & 31u)) & 1u;
        }
      }
      tile_n = (!ACC || brick_n) && ((coarse_n[t >> 5] >> (t & 31u)) & 1u);
      if (ACC && !tile_n) {
        // every cell up to the crossing that leaves the wholly free cube is free: nothing to mark
        const int n = rc_jump(brick_n ? 7 : 31, W);
        if (n >= W.left) break;  // the ray ends inside it
        W.left -= n;
        continue;
      }
      tile_s = tile_n && ((coarse_s[t >> 5] >> (t & 31u)) & 1u);
    }
    if (tile_n) {
      const uint32_t bit = occ_index(tl.nty, tl.ntz, W.c0, W.c1, W.c2), wi = bit >> 5;
      if (wi != last_w) {
        flush();
        last_w = wi;
        sword = tile_s ? solid[wi] : 0u;  // a tile without a solid cell: its solid words are not read
        uword = unknown[wi];
      }
      const uint32_t m = 1u << (bit & 31u);
      if (sword & m) {
        stopped = true;
        break;
      }
      if (uword & m) {
        ++visits;
        if (ACC) acc |= m;
        else vg_or(mine + wi, m);
      }
    }
    if (--W.left == 0) break;
    W.step();
  }
  flush();
  if (stats) {
    unsigned long long ne = entered ? 1 : 0, ns = stopped ? 1 : 0, nv = visits;
    for (int o = 32; o > 0; o >>= 1) {
      ne += __shfl_down(ne, o, 64);
      ns += __shfl_down(ns, o, 64);
      nv += __shfl_down(nv, o, 64);
    }
    if (l == 0) {
      if (ne) atomicAdd(&stats[0], ne);
      if (ns) atomicAdd(&stats[1], ns);
      if (nv) atomicAdd(&stats[2], nv);
    }
  }
}

// gain[p] += the set bits of pose p's mask (gain zeroed by the caller).  Grid (chunks, poses): the
// workgroups of a pose stride over its words together (one workgroup per pose read a 16-MiB mask
// in 2 ms, §5.15).
constexpr int kVgCountWords = 256 * 16;  // words per workgroup and round
__global__ __launch_bounds__(256) void k_vg_count(const uint64_t* __restrict__ seen, int64_t words,
                                                  unsigned long long* __restrict__ gain) {
  const uint64_t* m = seen + (int64_t)blockIdx.y * words;
  unsigned long long c = 0;
  for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (int64_t)gridDim.x * 256) c += __popcll(m[w]);
  __shared__ unsigned long long part[4];
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long n = part[0] + part[1] + part[2] + part[3];
    if (n) atomicAdd(&gain[blockIdx.y], n);
  }
}

static int64_t vg_words(const dmf_volume* v) {
  const Geom g = v->geom();
  return 8 * (int64_t)grid_tiles(g.n).ntiles;
}

// The ray-cast's checks, and at least one output; nothing of the volume is read before a plain
// argument is refused.
static int check_viewgain(const dmf_volume* v, const dmf_camera* cam, const void* logodds, const void* poses, int32_t P,
                          int32_t range_mm, bool any_output) {
  if (!v || !cam || !logodds || !poses) return fail(DMF_ERR_INVALID, "null argument");
  if (!any_output) return fail(DMF_ERR_INVALID, "null output");
  return check_raycast(v, cam, logodds, poses, P, range_mm);
}

// Masks into d_seen (P x words) when given, else into scratch in pose batches; d_gain (P, may be
// null when d_seen is given); d_stats += 3 counters (may be null).
static int viewgain_device(dmf_volume* v, const dmf_camera* cam, const int16_t* d_logodds, const float* d_poses,
                           int32_t P, int32_t occ, int32_t free_, int32_t range_mm, uint64_t* d_seen, uint64_t* d_gain,
                           uint64_t* d_stats) {
  const CamP cp = cam_params(cam);
  const Geom g = v->geom();
  const GridTiles tl = grid_tiles(g.n);
  PoseX* tab = nullptr;
  DMF_TRY(pose_table(v, d_poses, P, true, &tab));
  // both tile levels (solid, not wholly free), then both brick levels, in one buffer
  const uint32_t ncoarse = (tl.ntiles + 31u) / 32u, nbw = (tl.nbricks + 31u) / 32u;
  const size_t fine_bytes = sizeof(uint32_t) * 16 * (size_t)tl.ntiles;
  void *solid, *unknown, *coarse;
  DMF_TRY(scratch(v, kScVgSolid, fine_bytes, &solid));
  DMF_TRY(scratch(v, kScVgUnknown, fine_bytes, &unknown));
  DMF_TRY(scratch(v, kScVgCoarse, sizeof(uint32_t) * 2 * ((size_t)ncoarse + nbw), &coarse));
  uint32_t* const coarse_s = (uint32_t*)coarse;
  uint32_t* const coarse_n = coarse_s + ncoarse;
  uint32_t* const bricks = coarse_s + 2 * (size_t)ncoarse;
  const int64_t words = 8 * (int64_t)tl.ntiles;
  const size_t pose_bytes = sizeof(uint64_t) * (size_t)words;
  int batch = P;
  uint64_t* masks = d_seen;
  if (!masks) {
    const int64_t cap = v->knob[DMF_KNOB_VIEWGAIN_BATCH];
    const int64_t b = cap > 0 ? cap : (int64_t)std::max<size_t>(1, kVgBatchBytes / pose_bytes);
    batch = (int)std::min<int64_t>(P, b);
    void* m;
    DMF_TRY(scratch(v, kScVgSeen, pose_bytes * (size_t)batch, &m));
    masks = (uint64_t*)m;
  }
  unsigned long long* st = nullptr;
  if (d_stats) DMF_TRY(stats_begin(v, &st));
  hipLaunchKernelGGL(k_vg_mask, dim3(ncoarse), dim3(kMaskThreads), 0, v->stream, g, tl, d_logodds, occ, free_,
                     (uint32_t*)solid, (uint32_t*)unknown, coarse_s, coarse_n);
  DMF_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_vg_bricks, dim3(nbw, 2), dim3(64), 0, v->stream, tl, (const uint32_t*)coarse_s, ncoarse, bricks,
                     nbw);
  DMF_LAUNCH_CHECK();
  const uint32_t* const bricks_n = bricks + nbw;
  const int pkx = (cp.W + 7) / 8;
  // DMF_KNOB_VIEWGAIN_WALK (dmf_diag.h): 1 = plain, 2 = jumps + one atomic per word, 3 = 2 with a read first
  const int64_t kw = v->knob[DMF_KNOB_VIEWGAIN_WALK];
  const int walk = (kw >= 1 && kw <= 3) ? (int)kw : kVgDefaultWalk;
  for (int p0 = 0; p0 < P; p0 += batch) {
    const int n = std::min(batch, P - p0);
    uint64_t* const m = d_seen ? masks + (size_t)p0 * words : masks;
    DMF_HIP(hipMemsetAsync(m, 0, pose_bytes * (size_t)n, v->stream));
    const dim3 grid((unsigned)(pkx * ((cp.H + 7) / 8)), (unsigned)n);
#define DMF_VG_CAST(ACC, TEST)                                                                                     \
  hipLaunchKernelGGL((k_vg_cast<ACC, TEST>), grid, dim3(64), 0, v->stream, g, tl, cp, tab + p0, range_mm, pkx,     \
                     (const uint32_t*)solid, (const uint32_t*)unknown, (const uint32_t*)coarse_s,                  \
                     (const uint32_t*)coarse_n, bricks_n, (uint32_t*)m, (size_t)words * 2, st)
    if (walk == 1) DMF_VG_CAST(false, false);
    else if (walk == 2) DMF_VG_CAST(true, false);
    else DMF_VG_CAST(true, true);
#undef DMF_VG_CAST
    DMF_LAUNCH_CHECK();
    if (d_gain) {
      DMF_HIP(hipMemsetAsync(d_gain + p0, 0, sizeof(uint64_t) * (size_t)n, v->stream));
      const unsigned chunks = (unsigned)std::min<int64_t>((words + kVgCountWords - 1) / kVgCountWords, 1024);
      hipLaunchKernelGGL(k_vg_count, dim3(chunks, (unsigned)n), dim3(256), 0, v->stream, (const uint64_t*)m, words,
                         (unsigned long long*)(d_gain + p0));
      DMF_LAUNCH_CHECK();
    }
  }
  if (d_stats) DMF_TRY(stats_end(v, st, d_stats, 3));
  return DMF_OK;
}

// The masks of all P poses in scratch (an allocation that fails: DMF_ERR_NOMEM), the set cover
// over them, and each pose's own gain to the host when asked for.
static int next_best_views(dmf_volume* v, const dmf_camera* cam, const int16_t* d_logodds, const float* d_poses,
                           int32_t P, int32_t occ, int32_t free_, int32_t range_mm, int32_t min_gain,
                           int32_t* selected, int32_t* nselected, uint64_t* gain) {
  const int64_t words = vg_words(v);
  void *masks, *dg = nullptr;
  if (scratch(v, kScVgSeen, sizeof(uint64_t) * (size_t)words * (size_t)P, &masks) != DMF_OK) {
    (void)hipGetLastError();
    return fail(DMF_ERR_NOMEM, "the masks of %d poses need %zu bytes of device memory", P,
                sizeof(uint64_t) * (size_t)words * (size_t)P);
  }
  if (gain) DMF_TRY(scratch(v, kScVgGain, sizeof(uint64_t) * (size_t)P, &dg));
  DMF_TRY(viewgain_device(v, cam, d_logodds, d_poses, P, occ, free_, range_mm, (uint64_t*)masks, (uint64_t*)dg,
                          nullptr));
  if (gain) DMF_HIP(hipMemcpyAsync(gain, dg, sizeof(uint64_t) * (size_t)P, hipMemcpyDeviceToHost, v->stream));
  return greedy_cover(v, (const uint64_t*)masks, P, words, min_gain, selected, nselected);  // (synchronises)
}

}  // namespace dmf

using namespace dmf;

extern "C" {

int dmf_view_gain_words(const dmf_volume* v, int64_t* words) {
  DMF_API_BEGIN
  if (!v || !words) return fail(DMF_ERR_INVALID, "null argument");
  if (!v->constructed) return fail(DMF_ERR_STATE, "constructVolume() has not been called");
  *words = vg_words(v);
  return DMF_OK;
  DMF_API_END
}

int dmf_view_mask_index(const dmf_volume* v, int32_t x, int32_t y, int32_t z, uint64_t* bit) {
  DMF_API_BEGIN
  if (!v || !bit) return fail(DMF_ERR_INVALID, "null argument");
  if (!v->constructed) return fail(DMF_ERR_STATE, "constructVolume() has not been called");
  const Geom g = v->geom();
  if (x < 0 || y < 0 || z < 0 || x >= g.n[0] || y >= g.n[1] || z >= g.n[2])
    return fail(DMF_ERR_INVALID, "cell (%d, %d, %d) outside the grid", x, y, z);
  const GridTiles tl = grid_tiles(g.n);
  *bit = occ_index(tl.nty, tl.ntz, x, y, z);
  return DMF_OK;
  DMF_API_END
}

int dmf_view_gain_device(dmf_volume* v, const dmf_camera* cam, const int16_t* d_logodds, const float* d_poses, int32_t P,
                         int32_t occ_threshold, int32_t free_threshold, int32_t range_mm, uint64_t* d_seen,
                         uint64_t* d_gain, uint64_t* d_stats) {
  DMF_API_BEGIN
  DMF_TRY(check_viewgain(v, cam, d_logodds, d_poses, P, range_mm, d_seen || d_gain));
  return viewgain_device(v, cam, d_logodds, d_poses, P, occ_threshold, free_threshold, range_mm, d_seen, d_gain,
                         d_stats);
  DMF_API_END
}

int dmf_view_gain(dmf_volume* v, const dmf_camera* cam, const int16_t* logodds, const float* poses, int32_t P,
                  int32_t occ_threshold, int32_t free_threshold, int32_t range_mm, uint64_t* seen, uint64_t* gain) {
  DMF_API_BEGIN
  DMF_TRY(check_viewgain(v, cam, logodds, poses, P, range_mm, seen || gain));
  const size_t mask_bytes = sizeof(uint64_t) * (size_t)vg_words(v) * (size_t)P;
  void *dl, *dp, *ds = nullptr, *dg = nullptr;
  DMF_TRY(upload_grid(v, logodds, &dl));
  DMF_TRY(scratch(v, kScHost2, sizeof(float) * 12 * (size_t)P, &dp));
  if (seen) DMF_TRY(scratch(v, kScVgSeen, mask_bytes, &ds));
  if (gain) DMF_TRY(scratch(v, kScVgGain, sizeof(uint64_t) * (size_t)P, &dg));
  DMF_HIP(hipMemcpyAsync(dp, poses, sizeof(float) * 12 * (size_t)P, hipMemcpyHostToDevice, v->stream));
  DMF_TRY(viewgain_device(v, cam, (const int16_t*)dl, (const float*)dp, P, occ_threshold, free_threshold, range_mm,
                          (uint64_t*)ds, (uint64_t*)dg, nullptr));
  if (seen) DMF_HIP(hipMemcpyAsync(seen, ds, mask_bytes, hipMemcpyDeviceToHost, v->stream));
  if (gain) DMF_HIP(hipMemcpyAsync(gain, dg, sizeof(uint64_t) * (size_t)P, hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipStreamSynchronize(v->stream));
  return DMF_OK;
  DMF_API_END
}

int dmf_next_best_views_device(dmf_volume* v, const dmf_camera* cam, const int16_t* d_logodds, const float* d_poses,
                               int32_t P, int32_t occ_threshold, int32_t free_threshold, int32_t range_mm,
                               int32_t min_gain, int32_t* selected, int32_t* nselected, uint64_t* gain) {
  DMF_API_BEGIN
  DMF_TRY(check_viewgain(v, cam, d_logodds, d_poses, P, range_mm, selected && nselected));
  return next_best_views(v, cam, d_logodds, d_poses, P, occ_threshold, free_threshold, range_mm, min_gain, selected,
                         nselected, gain);
  DMF_API_END
}

int dmf_next_best_views(dmf_volume* v, const dmf_camera* cam, const int16_t* logodds, const float* poses, int32_t P,
                        int32_t occ_threshold, int32_t free_threshold, int32_t range_mm, int32_t min_gain,
                        int32_t* selected, int32_t* nselected, uint64_t* gain) {
  DMF_API_BEGIN
  DMF_TRY(check_viewgain(v, cam, logodds, poses, P, range_mm, selected && nselected));
  void *dl, *dp;
  DMF_TRY(upload_grid(v, logodds, &dl));
  DMF_TRY(scratch(v, kScHost2, sizeof(float) * 12 * (size_t)P, &dp));
  DMF_HIP(hipMemcpyAsync(dp, poses, sizeof(float) * 12 * (size_t)P, hipMemcpyHostToDevice, v->stream));
  return next_best_views(v, cam, (const int16_t*)dl, (const float*)dp, P, occ_threshold, free_threshold, range_mm,
                         min_gain, selected, nselected, gain);
  DMF_API_END
}

}  // extern "C"
