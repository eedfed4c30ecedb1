// dmf_trace.hip — RayTracingEngine (RayTracingEngine.hpp:27-564) on gfx950.
//
//  * reverse visibility (reverseRayTraceFast :136-226, reverseRayTrace :45-134):
//    one lane per (occupied voxel, pose), the reference 1 mm march toward the
//    camera over the N-bit occupancy mask; results are per-pose ballot bitmasks in
//    occupied_cells_ order, compacted order-preservingly into the good lists.
//  * forward depth-plane march (rayTrace* :229-494): one lane per lattice pixel,
//    first occupied sample per pixel; list outputs are ordered by the reference
//    loop key (z_depth, r, c) through a per-voxel atomicMin + radix sort.
//  * z-buffer splat rayTraceVolume (:498-564).
// (The greedy set cover over the reverse march's masks is dmf_cover.hip, the planner's
// willCollide and cost map dmf_collide.hip.)
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "dmf_host.hpp"

namespace dmf {

// Register budget of k_reverse_x: its registers kept for 6 waves per SIMD (round 6: the next
// sample computed while a sample's loads are in flight needs 4 more VGPRs; at 7 waves 2 spill:
// 4.49-4.51 ms at 6 waves vs 4.56 at 7 with the spill and 4.54-4.56 without the precompute at 7,
// DESIGN.md §5.5; round 5: 7 waves, 72 VGPRs, 5.19 vs 5.21 ms at 6; 8 waves spilled and lost).
// The forward marches carry no occupancy attribute.
constexpr int kRevWaves = 6;
// The marches' empty-space jumps evaluate no landing sample: the reverse march's target is
// computed from the cube's faces moved in by Geom::jmarg (round 6: 5.19 -> 4.77 ms per 128
// poses, samples 937M -> 649M, DESIGN.md §5.5, profiles/r06y); the forward marches check the
// line's point at the landing against the cube shrunk by twice the rounding margin and take the
// entry jump's target as computed (round 6: 6.16 -> 5.51 ms per 128 poses, samples 1.10G ->
// 0.77G, DESIGN.md §5.6, profiles/r06z).
// The reverse march computes sample s + 1 while sample s's occupancy and distance loads are in
// flight (used when the step is a plain step; a jump or the centroid's cell recomputes; round 6).

struct EnumList {
  const float* axes;  // xs | ys | zs (float-accumulated, RayTracingEngine.hpp:54-56)
  int32_t nax[3];
  const uint32_t* list;  // occupied enumeration indices (i*ny+j)*nz+k, enumeration order
};

__device__ inline void wave_add_u64(unsigned long long* dst, unsigned long long x) {
  for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
  if ((threadIdx.x & 63) == 0 && x) atomicAdd(dst, x);
}

// Element e of a reverse march's list -> the voxel's centre; returns its slot.
// kEnum = false: reverseRayTraceFast over occupied_cells_ (e = the slot)
// kEnum = true : reverseRayTrace over the float-accumulated enumeration list
template <bool kEnum>
__device__ inline int64_t rev_item(const Geom& g, const DevVol& vd, const EnumList& el, int64_t e, float cen[3]) {
  if (!kEnum) {
    const uint64_t h = vd.hash[e];
    const int xid = (int)(h >> 40), yid = (int)((h >> 20) & 0xFFFFF), zid = (int)(h & 0xFFFFF);
    cell_centre(g, xid, yid, zid, cen);
    return e;
  }
  float x, y, z;
  enum_xyz(el.axes, el.nax, el.list[e], &x, &y, &z);
  const int32_t slot = vd.slot_of[lin_index(g, bin_axis(g, 0, x), bin_axis(g, 1, y), bin_axis(g, 2, z))];
  centre_of_corner(g, x, y, z, cen);
  return slot;
}

// "Some point of the slot carries a normal within 90 degrees of v" (RayTracingEngine.hpp:205-215)
__device__ inline bool slot_faces(const DevVol& vd, int64_t slot, const float v[3], float dstar) {
  bool faces = false;
  const int32_t a = vd.off[slot], b = vd.off[slot + 1];
  for (int32_t j = a; j < b; ++j) {
    const float4 n = vd.nrm[j];
    if (n.w != 0.0f && angle_ok(n.x, n.y, n.z, v, dstar)) { faces = true; break; }
  }
  return faces;
}

// The reverse 1 mm march (RayTracingEngine.hpp:81-103 / :172-200).  Returns true if
// an occupied voxel other than the centroid's is hit before leaving the volume.
// `capped` reports a march that never left (v == 0 or NaN: the reference loops
// forever there) — treated as occluded and counted as a hazard.
//
// kSkip: empty-space skipping over 8^3 bricks, exact.  Each sample coordinate is a
// monotone function of the step index (RN(v*fd), /1000 and + cen are monotone), so
// if samples s and j both lie inside one empty brick and inside the volume, every
// sample between them does too: none can hit an occupied cell, leave the volume or
// be the centroid cell (an occupied cell).  j is estimated from the brick faces and
// then verified by evaluating sample j exactly; on failure the march steps normally.
template <bool kSkip>
__device__ inline bool reverse_march(const Geom& g, const DevVol& vd, const float cen[3], const float v[3], int cx,
                                     int cy, int cz, int depth0, int max_steps, int64_t& samples, bool& capped) {
  capped = false;
  float rv[3] = {0.f, 0.f, 0.f};  // 1000 / v (estimate only)
  if (kSkip) {
#pragma unroll
    for (int a = 0; a < 3; ++a) rv[a] = v[a] != 0.0f ? 1000.0f / v[a] : 0.0f;
  }
  uint32_t known_full = 0xffffffffu;  // last brick found occupied (or not skippable)
  for (int s = 0; s < max_steps; ++s) {
    float p[3];
    march_sample(cen, v, depth0 + s, p);
    ++samples;
    if (!valid_points(g, p[0], p[1], p[2])) return false;
    const int a = bin_axis(g, 0, p[0]), b = bin_axis(g, 1, p[1]), c = bin_axis(g, 2, p[2]);
    if (a == cx && b == cy && c == cz) continue;  // hash == centroid_hash
    if (!valid_coords(g, a, b, c)) return false;
    if (occ_test(vd.occ, occ_bit(g, a, b, c))) return true;
    if (kSkip) {
      const uint32_t bl = ((uint32_t)(a >> vd.bsh) * (uint32_t)vd.nb[1] + (uint32_t)(b >> vd.bsh)) *
                              (uint32_t)vd.nb[2] + (uint32_t)(c >> vd.bsh);
      if (bl == known_full) continue;
      if (((vd.brick[bl >> 5] >> (bl & 31)) & 1u) == 0u) {
        // last depth still inside the brick along each moving axis (estimate)
        const int cell[3] = {a, b, c};
        float fdmax = 3.0e38f;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
          if (v[ax] == 0.0f) continue;
          const int lo = (cell[ax] >> vd.bsh) << vd.bsh;
          const int hi = min(lo + (1 << vd.bsh), g.n[ax]);  // exclusive
          const float face = (float)(g.mn[ax] + (double)(v[ax] > 0.0f ? hi : lo) * g.dl[ax]);
          fdmax = fminf(fdmax, (face - cen[ax]) * rv[ax]);
        }
        const float jf = floorf(fdmax) - (float)depth0 - 2.0f;
        if (jf > (float)(s + 1) && jf < (float)max_steps) {
          const int j = (int)jf;
          float q[3];
          march_sample(cen, v, depth0 + j, q);
          ++samples;
          if (valid_points(g, q[0], q[1], q[2])) {
            const int qa = bin_axis(g, 0, q[0]), qb = bin_axis(g, 1, q[1]), qc = bin_axis(g, 2, q[2]);
            if ((qa >> vd.bsh) == (a >> vd.bsh) && (qb >> vd.bsh) == (b >> vd.bsh) &&
                (qc >> vd.bsh) == (c >> vd.bsh) && valid_coords(g, qa, qb, qc)) {
              s = j;  // samples s+1 .. j lie inside the empty brick
              continue;
            }
          }
        }
      }
      known_full = bl;  // occupied brick, or estimate failed: step through it
    }
  }
  capped = true;
  return true;
}

// One lane per element of the list (rev_item) and pose.
template <bool kEnum, bool kSkip>
__global__ __launch_bounds__(256) void k_reverse(Geom g, DevVol vd, CamP cam, const PoseX* __restrict__ poses,
                                                 int64_t nelem, EnumList el, int depth0, int max_steps, float dstar,
                                                 int viz, int normal_test, uint64_t* __restrict__ vis_mask,
                                                 uint64_t* __restrict__ good_mask, int64_t words,
                                                 unsigned long long* __restrict__ stats, int* __restrict__ found,
                                                 unsigned long long* __restrict__ hazards) {
  stats = stat_slot(stats);
  const int p = blockIdx.y;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool vis = false, good = false;
  int64_t samples = 0;
  if (e < nelem) {
    float cen[3];
    const int64_t slot = rev_item<kEnum>(g, vd, el, e, cen);
    const PoseX& T = poses[p];
    float t[3];
    xform(T.i, cen[0], cen[1], cen[2], t);
    int r, c;
    if (deproject_valid(cam, t[0], t[1], t[2], r, c)) {
      const float d[3] = {T.f[3] - cen[0], T.f[7] - cen[1], T.f[11] - cen[2]};
      float v[3];
      normalized(d, v);
      bool capped;
      const bool collided = reverse_march<kSkip>(g, vd, cen, v, bin_axis(g, 0, cen[0]), bin_axis(g, 1, cen[1]),
                                          bin_axis(g, 2, cen[2]), depth0, max_steps, samples, capped);
      if (capped) atomicAdd(hazards, 1ull);
      if (!collided) {
        vis = true;
        const double zz = (double)t[2];
        if (zz >= kZMin && zz <= kZMax) good = !normal_test || slot_faces(vd, slot, v, dstar);
      }
    }
    if (viz) {
      if (vis) vd.view[slot] = 1;
      if (good) vd.good[slot] = 1;
    }
  }
  const uint64_t vb = __ballot(vis), gb = __ballot(good);
  const int64_t w = e >> 6;
  if ((threadIdx.x & 63) == 0 && w < words) {
    if (vis_mask) vis_mask[(int64_t)p * words + w] = vb;
    if (good_mask) good_mask[(int64_t)p * words + w] = gb;
    if (vb) atomicOr(&found[p], 1);
  }
  if (stats) {
    wave_add_u64(&stats[0], (unsigned long long)samples);
    wave_add_u64(&stats[1], (unsigned long long)(e < nelem ? 1 : 0));
  }
}

// ---- persistent reverse visibility (work queue per wave) -----------------------
// Same per-(voxel, pose) semantics as k_reverse<kEnum, true>; the march lengths of
// neighbouring voxels differ by orders of magnitude (outside the frustum: 0 samples,
// occluded: tens, visible: hundreds), so one lane per voxel leaves most lanes of a
// wave idle.  Here each wave owns kItems consecutive voxels of one pose and keeps
// its lanes busy: a lane that finishes records its result bits in LDS and takes the
// next voxel; refills run when at least kRefill lanes are idle (the setup is
// divergent code, so it is batched).
struct RevLane {
  float cen[3], v[3], rv[3];
  uint32_t cob;         // occupancy bit of the centroid's cell (0xffffffff: outside the grid)
  int s;                // next sample index
  uint32_t known_full;  // last brick found occupied / not skippable
  int item;             // local item index, -1 = idle
  int32_t slot;
  float tz;             // camera-frame z of the centroid (z-range test)
  uint32_t occi, occw;  // cached occupancy word
  float pn[3];          // sample pns, computed ahead
  int pns;
};

// Diagnostic build (DMF_EXP_STATS): sample categories into stats[2..12]
#if defined(DMF_EXP_STATS)
#define DMF_RS(i, x) (rst[(i) - 2] += (unsigned long long)(x))
#else
#define DMF_RS(i, x) ((void)0)
#endif
constexpr int kRevStatN = 11;

// One sample of the reverse march (RayTracingEngine.hpp:172-200): 0 = continue,
// 1 = collided, 2 = left the volume (visible), 3 = capped (collided, hazard).
//
// validPoints (x > min and x < max in double) is the exact float test
// vlo <= x <= vhi.  Empty-space skipping: the brick distance field d gives an empty
// cube of bricks of radius d - 1 around the current brick; every sample coordinate is
// a monotone function of the step index, so if samples s and j both lie in that cube
// (and inside the volume) so does every sample between them — none can hit an
// occupied cell, the centroid's cell (occupied) or leave the volume.  j is computed from the
// cube's faces moved in by Geom::jmarg, which puts sample j inside the cube without evaluating
// it.
__device__ inline int rev_step(const Geom& g, const DevVol& vd, RevLane& L, int depth0, int max_steps,
                               int64_t& samples, unsigned long long* rst) {
  (void)rst;
  if (L.s >= max_steps) return 3;
  float p[3];
  // sample s was computed by the previous step while that step's loads were in flight
  if (L.pns == L.s) {
    p[0] = L.pn[0];
    p[1] = L.pn[1];
    p[2] = L.pn[2];
  } else {
    march_sample(L.cen, L.v, depth0 + L.s, p);
  }
  ++samples;
  int a, b, c;
  if (!valid_points_f(g, p)) return 2;
  bin_point(g, p, a, b, c);
  // (the reference tests the centroid's hash before validCoords; the centroid's cell is inside
  // the grid, so testing validCoords first and then the cell by its occupancy bit, which is
  // one-to-one on the grid, takes the same branches with one compare instead of three)
  if (!valid_coords(g, a, b, c)) return 2;
  const uint32_t ob = occ_bit(g, a, b, c);
  if (ob == L.cob) { DMF_RS(2, 1); ++L.s; return 0; }
  // the brick's distance is loaded together with the occupancy word, before the occupancy test:
  // one memory latency per empty sample instead of two (round 6: 4.67 -> 4.56 ms per 128 poses,
  // DESIGN.md §5.5; the load is wasted on occupied samples and in known-full bricks)
  const int ba = a >> vd.bsh, bb = b >> vd.bsh, bc = c >> vd.bsh;
  const uint32_t bl = ((uint32_t)ba * (uint32_t)vd.nb[1] + (uint32_t)bb) * (uint32_t)vd.nb[2] + (uint32_t)bc;
  const int dpre = vd.bdist[bl];
  if ((ob >> 5) != L.occi) { L.occi = ob >> 5; L.occw = vd.occ[L.occi]; }
  march_sample(L.cen, L.v, depth0 + L.s + 1, L.pn);  // the next sample, while the loads are in flight
  L.pns = L.s + 1;
  if ((L.occw >> (ob & 31)) & 1u) return 1;
  if (bl != L.known_full) {
    const int d = dpre;
    if (d > 0) {
      // the jump target from the cube's exit faces moved toward the sample by g.jmarg: no
      // sample of the jump is evaluated here; the target j is the next one marched, and the
      // samples s+1 .. j-1 lie inside the empty cube (the moved face is
      // farther inside than every rounding of the face, the samples and their bins, so sample
      // j is inside the cube; the samples before it follow by monotonicity)
      const int R = d - 1;  // bricks within R of this one are empty
      const int bx[3] = {ba, bb, bc};
      float fdmax = 3.0e38f;
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) {
        if (L.v[ax] == 0.0f) continue;
        const int cf = L.v[ax] > 0.0f ? min((bx[ax] + R + 1) << vd.bsh, g.n[ax]) : max(bx[ax] - R, 0) << vd.bsh;
        const float face = (float)(g.mn[ax] + (double)cf * g.dl[ax]);
        const float fin = L.v[ax] > 0.0f ? face - g.jmarg[ax] : face + g.jmarg[ax];
        fdmax = fminf(fdmax, (fin - L.cen[ax]) * L.rv[ax]);
      }
      const float jf = floorf(fdmax) - (float)depth0 - 2.0f;
      if (jf > (float)(L.s + 1) && jf < (float)max_steps && jf < 4194304.0f) {
        DMF_RS(4, 1);
        DMF_RS(5, 1);
        DMF_RS(6, (int)jf - L.s);
        L.s = (int)jf;
        return 0;
      }
    } else {
      DMF_RS(12, 1);
    }
    L.known_full = bl;  // occupied brick, or the jump failed: step through it
  }
  DMF_RS(3, 1);
  ++L.s;
  return 0;
}

// kOrder (reverseRayTraceFast only): the wave's items are the occupied voxels in SPATIAL
// order (order[k] = the slot of the k-th voxel along a 3D Morton curve of its cell,
// ensure_spatial_order), so that a wave's 64 lanes start in neighbouring voxels: their rays
// toward the camera are near-parallel, cross the same bricks and end alike (all occluded or
// all visible).  The result bits are then in item order: vis_mask / good_mask receive
// item-ordered words, which k_mask_to_slots permutes into occupied_cells_ order (the output
// is a per-slot bitmask, so the processing order is free).
// One wave's work queue over items [base, base + nitems) of pose T: result bits into the
// wave's LDS words lvis / lgood (item-indexed, zeroed by the caller); returns the lane's "some
// item visible".  Shared by k_reverse_q (a grid of (item chunk, pose)) and k_reverse_x (per-XCD
// unit queues).
template <bool kEnum, int kItems, int kRefill, int kBurst, bool kOrder>
__device__ inline bool rev_wave(const Geom& g, const DevVol& vd, const CamP& cam, const PoseX& T, const EnumList& el,
                                const uint32_t* __restrict__ order, int64_t base, int nitems, int depth0,
                                int max_steps, float dstar, int viz, int normal_test, uint32_t* lvis, uint32_t* lgood,
                                int64_t& samples, int64_t& rays, unsigned long long& ncap, unsigned long long* rst) {
  [[maybe_unused]] const int l = threadIdx.x & 63;  // (diagnostic-build statistics)
  bool any_vis = false;
  RevLane L;
  L.item = -1;
  int next = 0;  // wave-uniform queue head
  while (true) {
    const uint64_t idle = __builtin_amdgcn_ballot_w64(L.item < 0);
    const int nidle = __builtin_popcountll(idle);
    if (next < nitems && (nidle >= kRefill || nidle == 64)) {
      if (L.item < 0) {
        const int it = next + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32),
                                                             __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
        if (it < nitems) {
          const int64_t e = base + it;
          ++rays;
          float cen[3];
          // (spatial order: item e of the wave's queue is the voxel of slot order[e])
          const int32_t slot = (int32_t)rev_item<kEnum>(g, vd, el, kOrder ? (int32_t)order[e] : e, cen);
          float t[3];
          xform(T.i, cen[0], cen[1], cen[2], t);
          int r, c;
          if (deproject_valid(cam, t[0], t[1], t[2], r, c)) {
            const float d[3] = {T.f[3] - cen[0], T.f[7] - cen[1], T.f[11] - cen[2]};
            normalized(d, L.v);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
              L.cen[a] = cen[a];
              L.rv[a] = L.v[a] != 0.0f ? 1000.0f / L.v[a] : 0.0f;
            }
            {
              const int cx = bin_axis(g, 0, cen[0]), cy = bin_axis(g, 1, cen[1]), cz = bin_axis(g, 2, cen[2]);
              L.cob = valid_coords(g, cx, cy, cz) ? occ_bit(g, cx, cy, cz) : 0xffffffffu;
            }
            L.s = 0;
            L.known_full = 0xffffffffu;
            L.occi = 0xffffffffu;
            L.pns = -1;
            L.item = it;
            L.slot = slot;
            L.tz = t[2];
            DMF_RS(9, 1);
          }
        }
      }
      next += nidle;
    }
    if (__builtin_amdgcn_ballot_w64(L.item >= 0) == 0) {
      if (next >= nitems) break;
      continue;
    }
    // march: up to kBurst samples per busy lane
    int st = 0;
#pragma unroll 1
    for (int b = 0; b < kBurst; ++b) {
      DMF_RS(10, l == 0);
      DMF_RS(11, L.item >= 0 && st == 0);
      if (L.item >= 0 && st == 0) st = rev_step(g, vd, L, depth0, max_steps, samples, rst);
      if (__builtin_amdgcn_ballot_w64(L.item >= 0 && st == 0) == 0) break;
    }
    if (L.item >= 0 && st != 0) {
      DMF_RS(7, st == 1);
      DMF_RS(8, st == 2);
      if (st == 3) ++ncap;
      if (st == 2) {
        any_vis = true;
        bool good = false;
        const double zz = (double)L.tz;
        if (zz >= kZMin && zz <= kZMax) good = !normal_test || slot_faces(vd, L.slot, L.v, dstar);
        atomicOr(&lvis[L.item >> 5], 1u << (L.item & 31));
        if (good) atomicOr(&lgood[L.item >> 5], 1u << (L.item & 31));
        if (viz) {
          vd.view[L.slot] = 1;
          if (good) vd.good[L.slot] = 1;
        }
      }
      L.item = -1;
    }
  }
  return any_vis;
}

// The end of a queue kernel: each wave adds its capped marches to the hazards and its counters
// to the statistics.
__device__ inline void rev_finish(unsigned long long ncap, int64_t samples, int64_t rays, const unsigned long long* rst,
                                  unsigned long long* hazards, unsigned long long* stats) {
  wave_add_u64(hazards, ncap);
  if (stats) {
    wave_add_u64(&stats[0], (unsigned long long)samples);
    wave_add_u64(&stats[1], (unsigned long long)rays);
#if defined(DMF_EXP_STATS)
#pragma unroll
    for (int i = 0; i < kRevStatN; ++i) wave_add_u64(&stats[2 + i], rst[i]);
#endif
  }
}

template <bool kEnum, int kItems, int kRefill, int kBurst, bool kOrder = false>
__global__ __launch_bounds__(256) void k_reverse_q(Geom g, DevVol vd, CamP cam, const PoseX* __restrict__ poses,
                                                   int64_t nelem, EnumList el, const uint32_t* __restrict__ order,
                                                   int depth0, int max_steps, float dstar, int viz, int normal_test,
                                                   uint64_t* __restrict__ vis_mask, uint64_t* __restrict__ good_mask,
                                                   int64_t words, unsigned long long* __restrict__ stats,
                                                   int* __restrict__ found, unsigned long long* __restrict__ hazards) {
  static_assert(kItems % 64 == 0, "whole mask words per wave");
  static_assert(!(kEnum && kOrder), "spatial order: occupied_cells_ items only");
  stats = stat_slot(stats);
  __shared__ uint32_t lvis[4][kItems / 32], lgood[4][kItems / 32];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  for (int i = l; i < kItems / 32; i += 64) { lvis[w][i] = 0; lgood[w][i] = 0; }
  const int p = blockIdx.y;
  const int64_t base = ((int64_t)blockIdx.x * 4 + w) * kItems;
  const int nitems = (int)max<int64_t>(0, min<int64_t>(kItems, nelem - base));
  int64_t samples = 0, rays = 0;
  unsigned long long ncap = 0;
  unsigned long long rst[kRevStatN] = {};
  __syncthreads();
  const bool any_vis = rev_wave<kEnum, kItems, kRefill, kBurst, kOrder>(
      g, vd, cam, poses[p], el, order, base, nitems, depth0, max_steps, dstar, viz, normal_test, lvis[w], lgood[w],
      samples, rays, ncap, rst);
  __syncthreads();
  const int64_t w0 = base >> 6;
  for (int i = l; i < kItems / 64; i += 64) {
    if (w0 + i < words) {
      const uint64_t vb = (uint64_t)lvis[w][2 * i] | ((uint64_t)lvis[w][2 * i + 1] << 32);
      const uint64_t gb = (uint64_t)lgood[w][2 * i] | ((uint64_t)lgood[w][2 * i + 1] << 32);
      if (vis_mask) vis_mask[(int64_t)p * words + w0 + i] = vb;
      if (good_mask) good_mask[(int64_t)p * words + w0 + i] = gb;
    }
  }
  if (__builtin_amdgcn_ballot_w64(any_vis) != 0 && l == 0) atomicOr(&found[p], 1);
  rev_finish(ncap, samples, rays, rst, hazards, stats);
}

// reverseRayTraceFast with per-XCD work queues (spatial order only).  A unit is one wave's
// 64 consecutive items of the Morton order for one pose.  The Morton range is cut into 8
// contiguous eighths, one queue per eighth, units pose-major inside it; workgroup b serves the
// queue of its XCD group b % 8 (blocks b and b + 8 share an XCD's L2 under the observed
// round-robin placement -- a speed choice only, any placement gives the same bits), so the
// waves resident on one XCD march rays from one region of the surface toward one camera at a
// time and share its L2 lines of the occupancy bitmask and distance field.  A wave whose queue
// is empty takes units from the next groups' queues (work stealing at the tail), so uneven
// march work per eighth cannot idle an XCD; every wave exits once all 8 queues are drained.
// heads[8]: the queues' unit counters (zeroed before the launch).
// kWg: a unit is the workgroup's 4 consecutive waves' worth of items (256, as one workgroup of
// k_reverse_q), taken by the workgroup together: its waves share the CU's L1 lines as in
// k_reverse_q, at the price of a barrier per unit; else one wave's 64 items per unit.
template <int kItems, int kRefill, int kBurst, bool kWg>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kRevWaves))) void k_reverse_x(Geom g, DevVol vd, CamP cam, const PoseX* __restrict__ poses, int P,
                                                   int64_t nelem, const uint32_t* __restrict__ order, int depth0,
                                                   int max_steps, float dstar, int viz, uint64_t* __restrict__ vis_mask,
                                                   uint64_t* __restrict__ good_mask, int64_t words,
                                                   unsigned int* __restrict__ heads,
                                                   unsigned long long* __restrict__ stats, int* __restrict__ found,
                                                   unsigned long long* __restrict__ hazards) {
  static_assert(kItems == 64, "one mask word per wave and unit");
  stats = stat_slot(stats);
  __shared__ uint32_t lvis[4][2], lgood[4][2];
  __shared__ uint32_t s_unit;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int grp = (int)(blockIdx.x & 7u);
  const EnumList el{};
  int64_t samples = 0, rays = 0;
  unsigned long long ncap = 0;
  unsigned long long rst[kRevStatN] = {};
  constexpr int kPer = kWg ? 4 : 1;  // mask words per unit
  const int64_t nwu = (words + kPer - 1) / kPer;
  for (int q = 0; q < 8; ++q) {
    const int gq = (grp + q) & 7;
    const int64_t c0 = nwu * gq / 8, nch = nwu * (gq + 1) / 8 - c0;
    const uint32_t nunits = (uint32_t)(nch * P);
    for (;;) {
      uint32_t u = 0;
      if (kWg) {
        if (threadIdx.x == 0) s_unit = atomicAdd(&heads[gq], 1u);
        __syncthreads();
        u = s_unit;
        __syncthreads();  // every wave has read it before the next unit's write
      } else {
        if (l == 0) u = atomicAdd(&heads[gq], 1u);
        u = (uint32_t)__builtin_amdgcn_readfirstlane((int)u);
      }
      if (u >= nunits) break;
      const int p = (int)(u / (uint32_t)nch);
      const int64_t c = (c0 + (int64_t)(u - (uint32_t)p * (uint32_t)nch)) * kPer + (kWg ? w : 0);
      if (l < 2) { lvis[w][l] = 0; lgood[w][l] = 0; }
      __builtin_amdgcn_wave_barrier();
      const int64_t base = c * kItems;
      const int nitems = (int)max<int64_t>(0, min<int64_t>(kItems, nelem - base));
      const bool any_vis = rev_wave<false, kItems, kRefill, kBurst, true>(
          g, vd, cam, poses[p], el, order, base, nitems, depth0, max_steps, dstar, viz, 1, lvis[w], lgood[w],
          samples, rays, ncap, rst);
      __builtin_amdgcn_wave_barrier();
      if (l == 0 && c < words) {
        const uint64_t vb = (uint64_t)lvis[w][0] | ((uint64_t)lvis[w][1] << 32);
        const uint64_t gb = (uint64_t)lgood[w][0] | ((uint64_t)lgood[w][1] << 32);
        if (vis_mask) vis_mask[(int64_t)p * words + c] = vb;
        if (good_mask) good_mask[(int64_t)p * words + c] = gb;
      }
      if (__builtin_amdgcn_ballot_w64(any_vis) != 0 && l == 0) atomicOr(&found[p], 1);
    }
  }
  rev_finish(ncap, samples, rays, rst, hazards, stats);
}

// Item-ordered result bits (k_reverse_q<*, kOrder>) -> occupied_cells_ order: one wave per
// output word of 64 slots, all P poses; lane l takes slot 64 w + l, whose item is rank[slot].
__global__ __launch_bounds__(256) void k_mask_to_slots(const uint64_t* __restrict__ vis_items,
                                                       const uint64_t* __restrict__ good_items,
                                                       const uint32_t* __restrict__ rank, int64_t V, int64_t words,
                                                       int P, uint64_t* __restrict__ vis, uint64_t* __restrict__ good) {
  const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int l = threadIdx.x & 63;
  if (w >= words) return;
  const int64_t s = w * 64 + l;
  const uint32_t k = s < V ? rank[s] : 0u;
  for (int p = 0; p < P; ++p) {
    const int64_t row = (int64_t)p * words;
    bool bv = false, bg = false;
    if (s < V) {
      bv = (vis_items[row + (k >> 6)] >> (k & 63)) & 1ull;
      bg = (good_items[row + (k >> 6)] >> (k & 63)) & 1ull;
    }
    const uint64_t mv = __builtin_amdgcn_ballot_w64(bv), mg = __builtin_amdgcn_ballot_w64(bg);
    if (l == 0) {
      vis[row + w] = mv;
      good[row + w] = mg;
    }
  }
}

// 3D Morton key of an occupied voxel (21 bits per axis; the hash holds 20) and the slot as value.
__device__ inline uint64_t morton_spread(uint64_t x) {
  x &= 0x1fffffull;
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}
__global__ void k_morton_keys(const uint64_t* __restrict__ hash, int64_t V, uint64_t* __restrict__ keys,
                              uint64_t* __restrict__ vals) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= V) return;
  const uint64_t h = hash[s];
  keys[s] = morton_spread(h >> 40) << 2 | morton_spread((h >> 20) & 0xFFFFF) << 1 | morton_spread(h & 0xFFFFF);
  vals[s] = (uint64_t)s;
}
__global__ void k_order_store(const uint64_t* __restrict__ vals, int64_t V, uint32_t* __restrict__ order,
                              uint32_t* __restrict__ rank) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= V) return;
  const uint32_t s = (uint32_t)vals[k];
  order[k] = s;
  rank[s] = (uint32_t)k;
}

// The occupied voxels in spatial (3D Morton) order, rebuilt after an integration changed them.
static int ensure_spatial_order(dmf_volume* v) {
  if (v->sorder_valid) return DMF_OK;
  const int64_t V = v->V;
  if (V > v->sorder_cap) {
    if (v->d_sorder) DMF_HIP(hipFree(v->d_sorder));
    v->d_sorder = nullptr;
    v->sorder_cap = 0;
    DMF_HIP(hipMalloc((void**)&v->d_sorder, sizeof(uint32_t) * 2 * (size_t)V));
    v->sorder_cap = V;
  }
  void *keys, *vals;
  DMF_TRY(scratch(v, kScOut2, sizeof(uint64_t) * (size_t)V, &keys));
  DMF_TRY(scratch(v, kScOut3, sizeof(uint64_t) * (size_t)V, &vals));
  const dim3 blk(256), grd((unsigned)((V + 255) / 256));
  hipLaunchKernelGGL(k_morton_keys, grd, blk, 0, v->stream, v->d_hash, V, (uint64_t*)keys, (uint64_t*)vals);
  DMF_LAUNCH_CHECK();
  DMF_TRY(sort_pairs_u64(v, (uint64_t*)keys, (uint64_t*)vals, (size_t)V, 63));
  hipLaunchKernelGGL(k_order_store, grd, blk, 0, v->stream, (const uint64_t*)vals, V, v->d_sorder,
                     v->d_sorder + v->sorder_cap);
  DMF_LAUNCH_CHECK();
  v->sorder_valid = true;
  return DMF_OK;
}

static int max_march_steps(const dmf_volume* v) {
  const double dx = v->xmax - v->xmin, dy = v->ymax - v->ymin, dz = v->zmax - v->zmin;
  const double diag_mm = std::sqrt(dx * dx + dy * dy + dz * dz) * 1000.0;
  const double s = std::ceil(diag_mm * 1.01) + 64;
  return s > 2e9 ? 2000000000 : (int)s;
}

// Runs k_reverse for P poses; masks land in scratch kScOut0 (vis | good).
static int run_reverse(dmf_volume* v, const dmf_camera* cam, const float* poses, int P, bool poses_on_device,
                       int viz, bool enumerate, uint64_t** d_vis, uint64_t** d_good, int64_t* words_out,
                       int64_t* nelem_out, std::vector<int>* found_h, uint64_t* d_stats) {
  DMF_TRY(require_constructed(v));
  DMF_TRY(check_camera(cam));
  if (P <= 0 || P > 65535) return fail(DMF_ERR_INVALID, "pose count %d out of range [1,65535]", P);
  if (enumerate) DMF_TRY(ensure_enumeration(v));
  PoseX* tab;
  DMF_TRY(pose_table(v, poses, P, poses_on_device, &tab));
  const int64_t nelem = enumerate ? v->nenum : v->V;
  const int64_t words = (nelem + 63) / 64;
  void *masks, *aux;
  DMF_TRY(scratch(v, kScOut0, sizeof(uint64_t) * (size_t)std::max<int64_t>(2 * P * words, 1), &masks));
  const size_t found_bytes = ((sizeof(int) * P + 7) / 8) * 8;
  DMF_TRY(scratch(v, kScHost2, found_bytes + 2 * sizeof(unsigned long long), &aux));
  int* found = (int*)aux;
  unsigned long long* hz = (unsigned long long*)((char*)aux + found_bytes);
  DMF_HIP(hipMemsetAsync(aux, 0, found_bytes + 2 * sizeof(unsigned long long), v->stream));
  uint64_t* vis = (uint64_t*)masks;
  uint64_t* good = vis + P * words;
  unsigned long long* st = nullptr;
  if (d_stats) DMF_TRY(stats_begin(v, &st));
  if (nelem > 0) {
    EnumList el{v->d_axes, {v->nax[0], v->nax[1], v->nax[2]}, v->d_enum};
    const dim3 grid((unsigned)((nelem + 255) / 256), (unsigned)P);
    const int depth0 = enumerate ? 1 : 50;  // :81 vs :172
    // DMF_KNOB_REVERSE_KERNEL (dmf_diag.h): 0 = default (the work-queue march with the brick
    // distance field, items in spatial order for reverseRayTraceFast, per-XCD unit queues),
    // 1 = lane per (voxel, pose), 2 = the same with brick skipping, 3 = the work queue in
    // occupied_cells_ order, 4 = per-XCD queues of per-wave units, 5 = the spatial-order work
    // queue on a (chunk, pose) grid (the default until round 5)
    const int64_t kr = v->knob[DMF_KNOB_REVERSE_KERNEL];
    // work-queue shape (items per wave, refill threshold, burst): 512 / 8 / 8 in enumeration
    // or insertion order; in spatial order smaller queues pay (neighbouring lanes agree, so
    // the per-wave tail is the cost): 64 / 8 / 16 measured 5.54 ms vs 5.94 at 128 / 8 / 16 and
    // 6.51 at 512 / 8 / 8 (profiles/r04/reverse_queue_sweep.json)
    constexpr int kRevItems = 512, kRevRefill = 8, kRevBurst = 8;
    // the spatial-order queue's shape (round 5, per-XCD queues: burst 32 5.24-5.25 ms vs 16 5.29-5.32, 24 5.25-5.26, 8 5.39-5.41;
    // refill 4 / 12 / 16 at burst 16 within +-0.5 %: profiles/r05j/.  Round 6, after the
    // unchecked jumps: burst 64 4.67-4.69 ms vs 32 4.71-4.72, 48 4.71-4.74, 96 4.68-4.70, 128 4.68;
    // refill 4 / 16 at burst 32 +-0.2 %: profiles/r06ab/, r06ac/)
    constexpr int kSpItems = 64, kSpRefill = 8, kSpBurst = 64;
    const dim3 gridq((unsigned)((nelem + 4 * kRevItems - 1) / (4 * kRevItems)), (unsigned)P);
    const dim3 gridqs((unsigned)((nelem + 4 * kSpItems - 1) / (4 * kSpItems)), (unsigned)P);
    const Geom g = v->geom();
    const DevVol dv = v->dev();
    const CamP cp = cam_params(cam);
    const int ms = max_march_steps(v);
    if (kr == 1 || kr == 2) {
      const auto kfn = enumerate ? (kr == 2 ? k_reverse<true, true> : k_reverse<true, false>)
                                 : (kr == 2 ? k_reverse<false, true> : k_reverse<false, false>);
      hipLaunchKernelGGL(kfn, grid, dim3(256), 0, v->stream, g, dv, cp, tab, nelem, el, depth0, ms, v->dstar, viz,
                         enumerate ? 0 : 1, vis, good, words, st, found, hz);
    } else {
      DMF_TRY(ensure_brick_dist(v));
      // the queue kernel writes every mask word it owns; words past the last wave stay 0
      if (enumerate) {
        hipLaunchKernelGGL((k_reverse_q<true, kRevItems, kRevRefill, kRevBurst>), gridq, dim3(256), 0, v->stream, g, dv, cp, tab, nelem,
                           el, nullptr, depth0, ms, v->dstar, viz, 0, vis, good, words, st, found, hz);
      } else if (kr == 3) {
        hipLaunchKernelGGL((k_reverse_q<false, kRevItems, kRevRefill, kRevBurst>), gridq, dim3(256), 0, v->stream, g, dv, cp, tab,
                           nelem, el, nullptr, depth0, ms, v->dstar, viz, 1, vis, good, words, st, found, hz);
      } else {
        DMF_TRY(ensure_spatial_order(v));
        void* items;
        // item-ordered masks, then 8 queue heads (k_reverse_x)
        DMF_TRY(scratch(v, kScRevItems, sizeof(uint64_t) * (size_t)(2 * P * words) + 64, &items));
        uint64_t* vis_i = (uint64_t*)items;
        uint64_t* good_i = vis_i + P * words;
        if (kr != 5) {
          // default: per-XCD unit queues (persistent: as many workgroups as the device holds at
          // once), a unit = the workgroup's 256 items (kr 4: a wave's 64) -- 5.30 vs 5.56 ms per
          // 128 poses (k_reverse_q's (chunk, pose) grid, kr 5), L2 hit rate 0.56 -> 0.83, beyond-L2
          // bytes 8.1 -> 3.3 GB; per-wave units 10.3 ms (the CU's waves no longer share L1 lines:
          // L2 requests x1.6).  DESIGN.md §5.5, profiles/r05b/
          unsigned int* heads = (unsigned int*)(good_i + P * words);
          DMF_HIP(hipMemsetAsync(heads, 0, 8 * sizeof(unsigned int), v->stream));
          const auto kfn = kr != 4 ? k_reverse_x<kSpItems, kSpRefill, kSpBurst, true>
                                   : k_reverse_x<kSpItems, kSpRefill, kSpBurst, false>;
          int per_cu = 0;
          DMF_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)kfn, 256, 0));
          int ncu = 0;
          DMF_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, v->device));
          const unsigned nwg = (unsigned)(std::max(ncu, 8) * std::max(per_cu, 1));
          hipLaunchKernelGGL(kfn, dim3(nwg), dim3(256), 0, v->stream, g, dv, cp, tab, P, nelem,
                             (const uint32_t*)v->d_sorder, depth0, ms, v->dstar, viz, vis_i, good_i, words, heads, st,
                             found, hz);
        } else {
          hipLaunchKernelGGL((k_reverse_q<false, kSpItems, kSpRefill, kSpBurst, true>), gridqs, dim3(256), 0, v->stream, g,
                             dv, cp, tab, nelem, el, (const uint32_t*)v->d_sorder, depth0, ms, v->dstar, viz, 1, vis_i,
                             good_i, words, st, found, hz);
        }
        DMF_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_mask_to_slots, dim3((unsigned)((words * 64 + 255) / 256)), dim3(256), 0, v->stream,
                           (const uint64_t*)vis_i, (const uint64_t*)good_i, (const uint32_t*)(v->d_sorder + v->sorder_cap),
                           nelem, words, P, vis, good);
      }
    }
    DMF_LAUNCH_CHECK();
  }
#if defined(DMF_EXP_STATS)
  if (d_stats) DMF_TRY(stats_end(v, st, d_stats, 2 + kRevStatN));
#else
  if (d_stats) DMF_TRY(stats_end(v, st, d_stats, 2));
#endif
  if (found_h) {
    found_h->assign(P, 0);
    unsigned long long hzh = 0;
    DMF_HIP(hipMemcpyAsync(found_h->data(), found, sizeof(int) * P, hipMemcpyDeviceToHost, v->stream));
    DMF_HIP(hipMemcpyAsync(&hzh, hz, sizeof(hzh), hipMemcpyDeviceToHost, v->stream));
    DMF_HIP(hipStreamSynchronize(v->stream));
    v->hazards += (int64_t)hzh;
  }
  *d_vis = vis;
  *d_good = good;
  *words_out = words;
  *nelem_out = nelem;
  return DMF_OK;
}

static int reverse_lists(dmf_volume* v, const dmf_camera* cam, const float* poses, int32_t P, int32_t viz,
                         bool enumerate, uint8_t* found, int64_t* counts, uint64_t* hashes, int64_t cap) {
  if (!poses || !counts) return fail(DMF_ERR_INVALID, "null argument");
  uint64_t *vis, *good;
  int64_t words, nelem;
  std::vector<int> fh;
  DMF_TRY(run_reverse(v, cam, poses, P, false, viz, enumerate, &vis, &good, &words, &nelem, &fh, nullptr));
  if (found)
    for (int p = 0; p < P; ++p) found[p] = fh[p] ? 1 : 0;
  uint64_t* d_list;
  int64_t total = 0;
  DMF_TRY(compact_masks(v, good, P, words, nelem, counts, &d_list, &total,
                        enumerate ? kValueEnumCentroidHash : kValueSlotHash));
  if (total > cap) return fail(DMF_ERR_CAPACITY, "need %lld hashes", (long long)total);
  if (total > 0) {
    if (!hashes) return fail(DMF_ERR_INVALID, "null hashes");
    DMF_HIP(hipMemcpyAsync(hashes, d_list, sizeof(uint64_t) * total, hipMemcpyDeviceToHost, v->stream));
  }
  DMF_HIP(hipStreamSynchronize(v->stream));
  return DMF_OK;
}

// ---------------------------------------------------------------- forward march
// First occupied sample per lattice pixel (RayTracingEngine.hpp:280-308 loop body).
//
// Empty-space skipping (kSkip), exact.  Sample k is w_k = T * project(r, c, zd_k) in the
// reference's float/double arithmetic; the same expression in exact arithmetic is the
// line L(zd) = t + zd * dir (project is linear in zd).  A rounding-error bound
// eps_a(zd) = 8u (|t_a| + zd * 0.001 (|m_a0 ux| + |m_a1 uy| + |m_a2|)), u = 2^-24, covers
// |w_k - L(zd_k)| on each axis (5 roundings of float terms on inputs within u of exact;
// 8u leaves room).  Hence, with every margin delta = 2 eps(zd_j) + 1e-9 m:
//  * entry: samples whose exact point lies before the line enters the volume box grown by
//    delta are outside the volume (validPoints false, the reference `continue`s) — jump to
//    the last of them;
//  * bricks: if samples s and j both lie inside an empty cube of bricks (L-inf brick
//    distance field, as the reverse march) shrunk by delta, their exact points lie inside it
//    shrunk by eps and, the cube being convex, so do the exact points of every sample in
//    between; those samples are therefore inside the cube: no hit, no hazard — jump to j.
// j is estimated from the line and then verified by evaluating sample j exactly.
// The march of lattice pixel (ri, ci) of one pose: k_out / slot_out [ri * C + ci].
template <bool kSkip>
__device__ inline void fwd_ray(const Geom& g, const DevVol& vd, const CamP& cam, const PoseX* __restrict__ pose,
                               int zstart, int zdelta, int rdelta, int cdelta, int R, int C, int ri, int ci,
                               int32_t* __restrict__ k_out, int32_t* __restrict__ slot_out,
                               unsigned long long* __restrict__ hazards, int64_t& samples) {
  const int64_t idx = (int64_t)ri * C + ci;
  if (ri < R && ci < C) {
    const int r = ri * rdelta, c = ci * cdelta;
    int32_t kk = -1, sl = -1;
    const float* m = pose->f;
    // the exact line (double estimates) and the error-bound coefficients
    double dir[3], eA[3], eB[3];
    float fdir[3], frd[3];  // float copies for the jump estimates (verified exactly)
    int dmin_jump = 1 << 30;  // smallest brick distance d whose cube holds >= 2 more samples
    if (kSkip) {
      const double ux = ((double)c - cam.cx) / cam.fx, uy = ((double)r - cam.cy) / cam.fy;
      double step = 0.0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double m0 = m[4 * a], m1 = m[4 * a + 1], m2 = m[4 * a + 2];
        dir[a] = 0.001 * (m0 * ux + m1 * uy + m2);
        eA[a] = 0x1p-21 * fabs((double)m[4 * a + 3]);
        eB[a] = 0x1p-21 * 0.001 * (fabs(m0 * ux) + fabs(m1 * uy) + fabs(m2));
        fdir[a] = (float)dir[a];
        frd[a] = dir[a] != 0.0 ? (float)(1.0 / dir[a]) : 0.0f;
        step = fmax(step, fabs(dir[a]) * zdelta / g.dl[a]);  // cells per sample along axis a
      }
      // the cube reaches (d - 1) bricks of 2^bsh cells beyond the current brick on every side
      dmin_jump = 1 + (int)ceil(2.0 * step / (double)(1 << vd.bsh)) + 1;
    }
    auto margin = [&](int a, double zd) { return 2.0 * (eA[a] + zd * eB[a]) + 1e-9; };
    const int last_k = (int)((kZMax * 1000 - 1 - zstart) / zdelta);  // samples k = 0..last_k
    uint32_t known_full = 0xffffffffu;  // last brick found occupied (or not skippable)
    bool entered = false;
    int k = 0;
    for (int zd = zstart; (double)zd < kZMax * 1000; zd += zdelta, ++k) {
      float pc[3], w[3];
      project(cam, r, c, zd, pc);
      xform(m, pc[0], pc[1], pc[2], w);
      ++samples;
      if (!valid_points_f(g, w)) {
        if (kSkip && !entered) {
          // jump to the last sample before the line enters the volume grown by the margin
          entered = true;  // (once: after the entry the march proceeds normally)
          double tin = -1e300, tout = 1e300;
          const double zmax = kZMax * 1000;
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            const double dm = margin(a, zmax);
            const double lo = g.mn[a] - dm, hi = g.mx[a] + dm, t0 = (double)m[4 * a + 3];
            if (dir[a] == 0.0) {
              if (t0 <= lo || t0 >= hi) tout = -1e300;  // never enters
            } else {
              const double ta = (lo - t0) / dir[a], tb = (hi - t0) / dir[a];
              tin = fmax(tin, fmin(ta, tb));
              tout = fmin(tout, fmax(ta, tb));
            }
          }
          int kj = tout < tin ? last_k : (int)floor((tin - (double)zstart) / zdelta) - 1;
          kj = min(kj, last_k);
          if (kj > k) {
            const int zj = zstart + kj * zdelta;
            // zj is a whole step before the line enters the volume grown by the margin, so every
            // sample up to it is outside the volume: no sample is evaluated to check it
            k = kj;
            zd = zj;
          }
        }
        continue;
      }
      entered = true;
      int a, b, cc;
      bin_point(g, w, a, b, cc);
      if (!valid_coords(g, a, b, cc)) {  // reference indexes voxels_ unguarded here (UB)
        atomicAdd(hazards, 1ull);
        continue;
      }
      if (occ_test(vd.occ, occ_bit(g, a, b, cc))) {
        kk = k;
        sl = vd.slot_of[lin_index(g, a, b, cc)];
        break;
      }
      if (!kSkip) continue;
      const int ba = a >> vd.bsh, bb = b >> vd.bsh, bc = cc >> vd.bsh;
      const uint32_t bl = ((uint32_t)ba * (uint32_t)vd.nb[1] + (uint32_t)bb) * (uint32_t)vd.nb[2] + (uint32_t)bc;
      if (bl == known_full) continue;
      const int d = vd.bdist[bl];
      if (d >= dmin_jump) {  // (smaller cubes cannot hold two more samples: not worth a try)
        const int Rb = d - 1;  // bricks within Rb of this one are empty
        const int bx[3] = {ba, bb, bc};
        double lo[3], hi[3];
        float zexit = 3.0e38f;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
          lo[ax] = g.mn[ax] + (double)(max(bx[ax] - Rb, 0) << vd.bsh) * g.dl[ax];
          hi[ax] = g.mn[ax] + (double)min((bx[ax] + Rb + 1) << vd.bsh, g.n[ax]) * g.dl[ax];
          if (fdir[ax] != 0.0f)
            zexit = fminf(zexit, ((float)(fdir[ax] > 0.0f ? hi[ax] : lo[ax]) - m[4 * ax + 3]) * frd[ax]);
        }
        int kj = min((int)floorf((zexit - (float)zstart) / (float)zdelta) - 1, last_k);
        if (kj > k + 1) {
          const int zj = zstart + kj * zdelta;
          bool ok = true;
          // sample j is not evaluated: the line's point at zj inside the cube shrunk by 2 delta
          // puts sample j inside it shrunk by delta (its rounding is within eps of the line)
#pragma unroll
          for (int ax = 0; ax < 3; ++ax) {
            const double dm = margin(ax, (double)zj), lq = (double)m[4 * ax + 3] + (double)zj * dir[ax];
            ok = ok && (double)w[ax] >= lo[ax] + dm && (double)w[ax] <= hi[ax] - dm && lq >= lo[ax] + 2.0 * dm &&
                 lq <= hi[ax] - 2.0 * dm;
          }
          if (ok) {  // samples k+1 .. kj lie inside the empty cube
            k = kj;
            zd = zj;
            continue;
          }
        }
      }
      known_full = bl;  // occupied brick, or the jump failed: step through it
    }
    k_out[idx] = kk;
    slot_out[idx] = sl;
  }
}

template <bool kSkip>
__global__ __launch_bounds__(256) void k_forward(Geom g, DevVol vd, CamP cam, const PoseX* __restrict__ pose,
                                                 int zstart, int zdelta, int rdelta, int cdelta, int R, int C,
                                                 int32_t* __restrict__ k_out, int32_t* __restrict__ slot_out,
                                                 unsigned long long* __restrict__ hazards,
                                                 unsigned long long* __restrict__ stats) {
  stats = stat_slot(stats);
  // a wave marches an 8x8 tile of lattice pixels (fwd_threads): neighbouring rays in both
  // directions reach similar depths and read the same bitmask tiles (a row of 64 pixels
  // spans 8x the angle); outputs stay row-major (idx)
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int tpr = (C + 7) >> 3, ln = (int)(t & 63);
  const int64_t tile = t >> 6;
  const int ri = (int)(tile / tpr) * 8 + (ln >> 3), ci = (int)(tile % tpr) * 8 + (ln & 7);
  // grid.y = pose index of a batched launch (one pose: grid.y = 1)
  int64_t samples = 0;
  fwd_ray<kSkip>(g, vd, cam, pose + blockIdx.y, zstart, zdelta, rdelta, cdelta, R, C, ri, ci,
                 k_out + (int64_t)blockIdx.y * R * C, slot_out + (int64_t)blockIdx.y * R * C, hazards, samples);
  if (stats) wave_add_u64(&stats[0], (unsigned long long)samples);
#if defined(DMF_EXP_STATS)
  // diagnostic build: 64 x the wave's longest march (lane-samples the wave occupies), so that
  // stats[0] / stats[1] is the march's lane utilisation
  if (stats) {
    unsigned long long mx = (unsigned long long)samples;
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned long long)__shfl_xor(mx, o, 64));
    if ((threadIdx.x & 63) == 0) atomicAdd(&stats[1], 64ull * mx);
  }
#endif
}

// ---- forward march with per-wave lane refill (fwd_kernel knob 2) -----------------------
// fwd_ray's loop, split into a per-pixel setup and one loop iteration (fwd_step), so that a lane
// whose ray has ended takes the next pixel of its wave's queue while the others march on: the
// k_reverse_q pattern on the forward march.  Same arithmetic, same outputs.
struct FwdLane {
  double dir[3], eA[3], eB[3];
  float fdir[3], frd[3];
  int k, zd, dmin_jump;
  uint32_t known_full;
  bool entered;
};

template <bool kSkip>
__device__ inline void fwd_setup(const Geom& g, const DevVol& vd, const CamP& cam, const float* m, int zstart,
                                 int zdelta, int r, int c, FwdLane& L) {
  L.dmin_jump = 1 << 30;
  if (kSkip) {
    const double ux = ((double)c - cam.cx) / cam.fx, uy = ((double)r - cam.cy) / cam.fy;
    double step = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double m0 = m[4 * a], m1 = m[4 * a + 1], m2 = m[4 * a + 2];
      L.dir[a] = 0.001 * (m0 * ux + m1 * uy + m2);
      L.eA[a] = 0x1p-21 * fabs((double)m[4 * a + 3]);
      L.eB[a] = 0x1p-21 * 0.001 * (fabs(m0 * ux) + fabs(m1 * uy) + fabs(m2));
      L.fdir[a] = (float)L.dir[a];
      L.frd[a] = L.dir[a] != 0.0 ? (float)(1.0 / L.dir[a]) : 0.0f;
      step = fmax(step, fabs(L.dir[a]) * zdelta / g.dl[a]);
    }
    L.dmin_jump = 1 + (int)ceil(2.0 * step / (double)(1 << vd.bsh)) + 1;
  }
  L.known_full = 0xffffffffu;
  L.entered = false;
  L.k = 0;
  L.zd = zstart;
}

// One iteration of fwd_ray's loop for pixel (r, c): 0 = march on, 1 = hit (kk, sl), 2 = the
// march left the depth range without a hit.
template <bool kSkip>
__device__ inline int fwd_step(const Geom& g, const DevVol& vd, const CamP& cam, const float* m, int zstart, int zdelta,
                               int last_k, int r, int c, FwdLane& L, int32_t& kk, int32_t& sl,
                               unsigned long long* __restrict__ hazards, int64_t& samples) {
  if (!((double)L.zd < kZMax * 1000)) return 2;
  auto margin = [&](int a, double zd) { return 2.0 * (L.eA[a] + zd * L.eB[a]) + 1e-9; };
  float pc[3], w[3];
  project(cam, r, c, L.zd, pc);
  xform(m, pc[0], pc[1], pc[2], w);
  ++samples;
  if (!valid_points_f(g, w)) {
    if (kSkip && !L.entered) {
      L.entered = true;
      double tin = -1e300, tout = 1e300;
      const double zmax = kZMax * 1000;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double dm = margin(a, zmax);
        const double lo = g.mn[a] - dm, hi = g.mx[a] + dm, t0 = (double)m[4 * a + 3];
        if (L.dir[a] == 0.0) {
          if (t0 <= lo || t0 >= hi) tout = -1e300;
        } else {
          const double ta = (lo - t0) / L.dir[a], tb = (hi - t0) / L.dir[a];
          tin = fmax(tin, fmin(ta, tb));
          tout = fmin(tout, fmax(ta, tb));
        }
      }
      int kj = tout < tin ? last_k : (int)floor((tin - (double)zstart) / zdelta) - 1;
      kj = min(kj, last_k);
      if (kj > L.k) {
        const int zj = zstart + kj * zdelta;
        L.k = kj;  // (as fwd_ray)
        L.zd = zj;
      }
    }
    L.zd += zdelta;
    ++L.k;
    return 0;
  }
  L.entered = true;
  int a, b, cc;
  bin_point(g, w, a, b, cc);
  if (!valid_coords(g, a, b, cc)) {
    atomicAdd(hazards, 1ull);
    L.zd += zdelta;
    ++L.k;
    return 0;
  }
  if (occ_test(vd.occ, occ_bit(g, a, b, cc))) {
    kk = L.k;
    sl = vd.slot_of[lin_index(g, a, b, cc)];
    return 1;
  }
  if (kSkip) {
    const int ba = a >> vd.bsh, bb = b >> vd.bsh, bc = cc >> vd.bsh;
    const uint32_t bl = ((uint32_t)ba * (uint32_t)vd.nb[1] + (uint32_t)bb) * (uint32_t)vd.nb[2] + (uint32_t)bc;
    if (bl != L.known_full) {
      bool jumped = false;
      const int d = vd.bdist[bl];
      if (d >= L.dmin_jump) {
        const int Rb = d - 1;
        const int bx[3] = {ba, bb, bc};
        double lo[3], hi[3];
        float zexit = 3.0e38f;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
          lo[ax] = g.mn[ax] + (double)(max(bx[ax] - Rb, 0) << vd.bsh) * g.dl[ax];
          hi[ax] = g.mn[ax] + (double)min((bx[ax] + Rb + 1) << vd.bsh, g.n[ax]) * g.dl[ax];
          if (L.fdir[ax] != 0.0f)
            zexit = fminf(zexit, ((float)(L.fdir[ax] > 0.0f ? hi[ax] : lo[ax]) - m[4 * ax + 3]) * L.frd[ax]);
        }
        int kj = min((int)floorf((zexit - (float)zstart) / (float)zdelta) - 1, last_k);
        if (kj > L.k + 1) {
          const int zj = zstart + kj * zdelta;
          bool ok = true;
#pragma unroll
          for (int ax = 0; ax < 3; ++ax) {  // (as fwd_ray)
            const double dm = margin(ax, (double)zj), lq = (double)m[4 * ax + 3] + (double)zj * L.dir[ax];
            ok = ok && (double)w[ax] >= lo[ax] + dm && (double)w[ax] <= hi[ax] - dm && lq >= lo[ax] + 2.0 * dm &&
                 lq <= hi[ax] - 2.0 * dm;
          }
          if (ok) {
            L.k = kj;
            L.zd = zj;
            jumped = true;
          }
        }
      }
      if (!jumped) L.known_full = bl;
    }
  }
  L.zd += zdelta;
  ++L.k;
  return 0;
}

// Each wave owns kUnit consecutive 8x8 tiles of one pose (grid.y) and keeps its lanes busy:
// a lane whose ray has ended writes its outputs and takes the next pixel of the unit (tile
// order: neighbouring rays together) when at least kRefill lanes are idle; between refills
// every busy lane marches up to kBurst samples.
template <bool kSkip, int kUnit, int kRefill, int kBurst>
__global__ __launch_bounds__(256) void k_forward_q(Geom g, DevVol vd, CamP cam,
                                                                const PoseX* __restrict__ pose, int zstart, int zdelta,
                                                                int rdelta, int cdelta, int R, int C,
                                                                int32_t* __restrict__ k_out, int32_t* __restrict__ slot_out,
                                                                unsigned long long* __restrict__ hazards,
                                                                unsigned long long* __restrict__ stats) {
  stats = stat_slot(stats);
  const int w = threadIdx.x >> 6;
  const int tpr = (C + 7) >> 3;
  const int64_t ntiles = (int64_t)((R + 7) >> 3) * tpr;
  const int64_t t0 = ((int64_t)blockIdx.x * 4 + w) * kUnit;
  if (t0 >= ntiles) return;
  const int nitems = (int)min<int64_t>(ntiles - t0, kUnit) * 64;
  const float* m = pose[blockIdx.y].f;
  int32_t* const ko = k_out + (int64_t)blockIdx.y * R * C;
  int32_t* const so = slot_out + (int64_t)blockIdx.y * R * C;
  const int last_k = (int)((kZMax * 1000 - 1 - zstart) / zdelta);
  int64_t samples = 0;
  [[maybe_unused]] unsigned long long busy = 0, slots = 0;  // (diagnostic build: lane utilisation)
  FwdLane L;
  int item = -1, r = 0, c = 0;
  int64_t idx = 0;
  int next = 0;  // wave-uniform queue head
  while (true) {
    const uint64_t idle = __builtin_amdgcn_ballot_w64(item < 0);
    const int nidle = __builtin_popcountll(idle);
    if (next < nitems && (nidle >= kRefill || nidle == 64)) {
      if (item < 0) {
        const int it = next + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32),
                                                             __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
        if (it < nitems) {
          const int64_t tile = t0 + (it >> 6);
          const int ln = it & 63;
          const int ri = (int)(tile / tpr) * 8 + (ln >> 3), ci = (int)(tile % tpr) * 8 + (ln & 7);
          if (ri < R && ci < C) {
            item = it;
            idx = (int64_t)ri * C + ci;
            r = ri * rdelta;
            c = ci * cdelta;
            fwd_setup<kSkip>(g, vd, cam, m, zstart, zdelta, r, c, L);
          }
        }
      }
      next += nidle;
    }
    if (__builtin_amdgcn_ballot_w64(item >= 0) == 0) {
      if (next >= nitems) break;
      continue;
    }
    int st = 0;
    int32_t kk = -1, sl = -1;
#pragma unroll 1
    for (int b = 0; b < kBurst; ++b) {
#if defined(DMF_EXP_STATS)
      if ((threadIdx.x & 63) == 0) slots += 64;
      if (item >= 0 && st == 0) ++busy;
#endif
      if (item >= 0 && st == 0) st = fwd_step<kSkip>(g, vd, cam, m, zstart, zdelta, last_k, r, c, L, kk, sl, hazards, samples);
      if (__builtin_amdgcn_ballot_w64(item >= 0 && st == 0) == 0) break;
    }
    if (item >= 0 && st != 0) {
      ko[idx] = kk;
      so[idx] = sl;
      item = -1;
    }
  }
  if (stats) wave_add_u64(&stats[0], (unsigned long long)samples);
#if defined(DMF_EXP_STATS)
  // diagnostic build: busy lane-iterations against 64 x burst iterations (stats[0] / stats[1]
  // of k_forward is the same utilisation of its lane-per-pixel march)
  if (stats) {
    wave_add_u64(&stats[2], busy);
    wave_add_u64(&stats[3], slots);
  }
#endif
}

// The batched forward march with per-XCD unit queues (as k_reverse_x): a unit is one
// workgroup's 4 consecutive 8x8 tiles (row-major tile order) of one pose; the tile range is
// cut into 8 contiguous bands of rows, one queue per band, units pose-major inside it, and
// workgroup b serves the queue of its XCD group b % 8 first (a speed choice: the waves of one
// XCD then march one slab of one frustum at a time and share its L2 lines of the occupancy
// bitmask and distance field), then steals from the other queues.  heads[8] zeroed before.
template <bool kSkip>
__global__ __launch_bounds__(256) void k_forward_x(Geom g, DevVol vd, CamP cam, const PoseX* __restrict__ pose, int P,
                                                   int zstart, int zdelta, int rdelta, int cdelta, int R, int C,
                                                   int32_t* __restrict__ k_out, int32_t* __restrict__ slot_out,
                                                   unsigned int* __restrict__ heads,
                                                   unsigned long long* __restrict__ hazards,
                                                   unsigned long long* __restrict__ stats) {
  stats = stat_slot(stats);
  __shared__ uint32_t s_unit;
  const int w = threadIdx.x >> 6, ln = threadIdx.x & 63;
  const int tpr = (C + 7) >> 3;
  const int64_t ntiles = (int64_t)((R + 7) >> 3) * tpr, nwu = (ntiles + 3) / 4;
  const int grp = (int)(blockIdx.x & 7u);
  int64_t samples = 0;
  for (int q = 0; q < 8; ++q) {
    const int gq = (grp + q) & 7;
    const int64_t u0 = nwu * gq / 8, nch = nwu * (gq + 1) / 8 - u0;
    const uint32_t nunits = (uint32_t)(nch * P);
    for (;;) {
      if (threadIdx.x == 0) s_unit = atomicAdd(&heads[gq], 1u);
      __syncthreads();
      const uint32_t u = s_unit;
      __syncthreads();  // every wave has read it before the next unit's write
      if (u >= nunits) break;
      const int p = (int)(u / (uint32_t)nch);
      const int64_t tile = (u0 + (int64_t)(u - (uint32_t)p * (uint32_t)nch)) * 4 + w;
      if (tile < ntiles) {
        const int ri = (int)(tile / tpr) * 8 + (ln >> 3), ci = (int)(tile % tpr) * 8 + (ln & 7);
        fwd_ray<kSkip>(g, vd, cam, pose + p, zstart, zdelta, rdelta, cdelta, R, C, ri, ci,
                       k_out + (int64_t)p * R * C, slot_out + (int64_t)p * R * C, hazards, samples);
      }
    }
  }
  if (stats) wave_add_u64(&stats[0], (unsigned long long)samples);
}

// k_forward_q's shape: tiles per wave unit, refill threshold, samples per burst
constexpr int kFwdUnit = 4, kFwdRefill = 16, kFwdBurst = 8;

// DMF_KNOB_FWD_SKIP = -1 (dmf_diag.h) disables the forward march's empty-space skipping (A/B)
static bool fwd_skip(const dmf_volume* v) { return v->knob[DMF_KNOB_FWD_SKIP] >= 0; }

// Launches k_forward over the R x C lattice of P poses: whole 8x8 tiles per pose, 4 to a workgroup.
// The caller checks the launch.
static int launch_forward(dmf_volume* v, const dmf_camera* cam, const PoseX* tab, int P, int zstart, int zdelta,
                          int rdelta, int cdelta, int R, int C, int32_t* k_out, int32_t* slot_out,
                          unsigned long long* hazards, unsigned long long* stats) {
  const int64_t threads = (int64_t)((R + 7) / 8) * ((C + 7) / 8) * 64;
  const dim3 grid((unsigned)((threads + 255) / 256), (unsigned)P);
  const bool skip = fwd_skip(v);
  if (skip) DMF_TRY(ensure_brick_dist(v));
  hipLaunchKernelGGL(skip ? k_forward<true> : k_forward<false>, grid, dim3(256), 0, v->stream, v->geom(), v->dev(),
                     cam_params(cam), tab, zstart, zdelta, rdelta, cdelta, R, C, k_out, slot_out, hazards, stats);
  return DMF_OK;
}

enum FwdMode { kTrace = 0, kClassify = 1, kGoodPoints = 2, kPoints = 3, kMinimum = 4 };

// Side effects of the first hit per pixel (RayTracingEngine.hpp:299-305, 351-371,
// 420-440, 480-489, 256-259).
__global__ void k_forward_post(Geom g, DevVol vd, CamP cam, const PoseX* __restrict__ pose, int mode, int zstart,
                               int zdelta, int rdelta, int cdelta, int R, int C, int view_arg, float dstar,
                               const int32_t* __restrict__ k_in, const int32_t* __restrict__ slot_in,
                               unsigned long long* __restrict__ minkey, int* __restrict__ kmin,
                               int* __restrict__ found) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)R * C) return;
  const int32_t kk = k_in[idx];
  if (kk < 0) return;
  const int32_t slot = slot_in[idx];
  *found = 1;
  if (mode == kMinimum) {
    atomicMin(kmin, kk);
    return;
  }
  if (mode == kTrace) {
    vd.view[slot] = 1;
    return;
  }
  const unsigned long long key = (unsigned long long)kk * (unsigned long long)((int64_t)R * C) + (unsigned long long)idx;
  if (mode == kPoints) {
    atomicMin(&minkey[slot], key);
    return;
  }
  // classify / good points: pseudo-centroid = sample + delta/2, v toward the camera
  const int zd = zstart + kk * zdelta;
  const int r = (int)(idx / C) * rdelta, c = (int)(idx % C) * cdelta;
  float pc[3], w[3];
  project(cam, r, c, zd, pc);
  xform(pose->f, pc[0], pc[1], pc[2], w);
  float cen[3];
  centre_of_corner(g, w[0], w[1], w[2], cen);
  const float d[3] = {pose->f[3] - cen[0], pose->f[7] - cen[1], pose->f[11] - cen[2]};
  float v[3];
  normalized(d, v);
  const bool ok = zd >= 250 && zd <= 600 && slot_faces(vd, slot, v, dstar);
  if (mode == kClassify) {
    if (vd.view[slot] == 0) vd.view[slot] = view_arg;
    if (ok) vd.good[slot] = 1;
  } else if (ok) {
    atomicMin(&minkey[slot], key);
  }
}

__global__ void k_minkey_flags(const unsigned long long* __restrict__ minkey, int64_t V, uint8_t* __restrict__ flags) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s < V) flags[s] = minkey[s] != ~0ull;
}

__global__ void k_minkey_pairs(const uint32_t* __restrict__ slots, const unsigned long long* __restrict__ nsel,
                               const unsigned long long* __restrict__ minkey, const uint64_t* __restrict__ hash,
                               uint64_t* __restrict__ keys, uint64_t* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if ((unsigned long long)i >= *nsel) return;
  const uint32_t s = slots[i];
  keys[i] = minkey[s];
  vals[i] = hash[s];
}

struct FwdResult {
  int found = 0;
  int minimum = -1;
  int64_t n = 0;
  uint64_t* d_list = nullptr;
};

static int run_forward(dmf_volume* v, const dmf_camera* cam, const float* pose, int mode, int zstart, int zdelta,
                       int rdelta, int cdelta, int view_arg, FwdResult* res) {
  DMF_TRY(require_constructed(v));
  DMF_TRY(check_camera(cam));
  if (!pose) return fail(DMF_ERR_INVALID, "null pose");
  if (zdelta <= 0) return fail(DMF_ERR_INVALID, "zdelta must be > 0 (the reference loops forever)");
  if (rdelta <= 0 || cdelta <= 0) return fail(DMF_ERR_INVALID, "bad pixel stride");
  PoseX* tab;
  DMF_TRY(pose_table(v, pose, 1, false, &tab));
  const int R = (cam->height + rdelta - 1) / rdelta, C = (cam->width + cdelta - 1) / cdelta;
  const int64_t RC = (int64_t)R * C;
  void *kb, *sb, *aux;
  DMF_TRY(scratch(v, kScOut0, sizeof(int32_t) * RC, &kb));
  DMF_TRY(scratch(v, kScOut1, sizeof(int32_t) * RC, &sb));
  DMF_TRY(scratch(v, kScHost2, 64, &aux));
  int* found = (int*)aux;
  int* kmin = found + 1;
  unsigned long long* hz = (unsigned long long*)((char*)aux + 16);
  DMF_HIP(hipMemsetAsync(aux, 0, 64, v->stream));
  DMF_HIP(hipMemsetAsync(kmin, 0x7f, sizeof(int), v->stream));
  const CamP cp = cam_params(cam);
  const Geom g = v->geom();
  const dim3 grid((unsigned)((RC + 255) / 256));
  DMF_TRY(launch_forward(v, cam, tab, 1, zstart, zdelta, rdelta, cdelta, R, C, (int32_t*)kb, (int32_t*)sb, hz,
                         nullptr));
  DMF_LAUNCH_CHECK();
  unsigned long long* minkey = nullptr;
  if ((mode == kPoints || mode == kGoodPoints) && v->V > 0) {
    void* mk;
    DMF_TRY(scratch(v, kScOut2, sizeof(unsigned long long) * v->V, &mk));
    minkey = (unsigned long long*)mk;
    DMF_HIP(hipMemsetAsync(minkey, 0xff, sizeof(unsigned long long) * v->V, v->stream));
  }
  hipLaunchKernelGGL(k_forward_post, grid, dim3(256), 0, v->stream, g, v->dev(), cp, tab, mode, zstart, zdelta,
                     rdelta, cdelta, R, C, view_arg, v->dstar, (const int32_t*)kb, (const int32_t*)sb, minkey, kmin,
                     found);
  DMF_LAUNCH_CHECK();
  int hf[2];
  unsigned long long hzh = 0;
  DMF_HIP(hipMemcpyAsync(hf, aux, sizeof(hf), hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipMemcpyAsync(&hzh, hz, sizeof(hzh), hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipStreamSynchronize(v->stream));
  v->hazards += (int64_t)hzh;
  res->found = hf[0];
  res->minimum = (hf[1] == 0x7f7f7f7f) ? -1 : zstart + hf[1] * zdelta;
  res->n = 0;
  if (minkey) {
    // slots with a key, ordered by the reference loop key (k, r, c)
    void *fl, *sel, *ns, *kk2;
    DMF_TRY(scratch(v, kScOut3, v->V + 16, &fl));
    DMF_TRY(scratch(v, kScOut0, sizeof(uint32_t) * v->V, &sel));
    DMF_TRY(scratch(v, kScHost1, 16, &ns));
    hipLaunchKernelGGL(k_minkey_flags, dim3((unsigned)((v->V + 255) / 256)), dim3(256), 0, v->stream, minkey, v->V,
                       (uint8_t*)fl);
    DMF_LAUNCH_CHECK();
    size_t bytes = 0;
    auto it = rocprim::counting_iterator<uint32_t>(0);
    DMF_HIP(rocprim::select(nullptr, bytes, it, (uint8_t*)fl, (uint32_t*)sel, (unsigned long long*)ns, (size_t)v->V,
                            v->stream));
    void* tmp;
    DMF_TRY(scratch(v, kScTmp, bytes, &tmp));
    DMF_HIP(rocprim::select(tmp, bytes, it, (uint8_t*)fl, (uint32_t*)sel, (unsigned long long*)ns, (size_t)v->V,
                            v->stream));
    unsigned long long n = 0;
    DMF_HIP(hipMemcpyAsync(&n, ns, sizeof(n), hipMemcpyDeviceToHost, v->stream));
    DMF_HIP(hipStreamSynchronize(v->stream));
    if (n > 0) {
      DMF_TRY(scratch(v, kScOut1, sizeof(uint64_t) * n, &kk2));
      void* vals;
      DMF_TRY(scratch(v, kScHost0, sizeof(uint64_t) * n, &vals));
      hipLaunchKernelGGL(k_minkey_pairs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, v->stream,
                         (const uint32_t*)sel, (const unsigned long long*)ns, minkey, v->d_hash, (uint64_t*)kk2,
                         (uint64_t*)vals);
      DMF_LAUNCH_CHECK();
      int end_bit = 1;
      const unsigned long long maxkey = (unsigned long long)((1000 - zstart) / zdelta + 2) * (unsigned long long)RC;
      while (end_bit < 64 && (1ull << end_bit) <= maxkey) ++end_bit;
      DMF_TRY(sort_pairs_u64(v, (uint64_t*)kk2, (uint64_t*)vals, n, end_bit));
      res->d_list = (uint64_t*)vals;
      res->n = (int64_t)n;
    }
  }
  return DMF_OK;
}

static int forward_list_api(dmf_volume* v, const dmf_camera* cam, const float* pose, int mode, int zdelta, int sparse,
                            uint8_t* found, uint64_t* hashes, int64_t cap, int64_t* n) {
  const int s = sparse ? 5 : 1;  // RayTracingEngine.hpp:387-392 / 452-457
  FwdResult res;
  DMF_TRY(run_forward(v, cam, pose, mode, 10, zdelta, s, s, 1, &res));
  if (found) *found = res.found ? 1 : 0;
  if (n) *n = res.n;
  if (res.n > cap) return fail(DMF_ERR_CAPACITY, "need %lld hashes", (long long)res.n);
  if (res.n > 0) {
    if (!hashes) return fail(DMF_ERR_INVALID, "null hashes");
    DMF_HIP(hipMemcpyAsync(hashes, res.d_list, sizeof(uint64_t) * res.n, hipMemcpyDeviceToHost, v->stream));
    DMF_HIP(hipStreamSynchronize(v->stream));
  }
  return DMF_OK;
}

// ---------------------------------------------------------------- rayTraceVolume
// z-buffer over the float-accumulated enumeration (RayTracingEngine.hpp:509-536),
// then view marking where the voxel's depth equals the pixel minimum (:540-563).
__global__ void k_zbuffer(Geom g, DevVol vd, CamP cam, const PoseX* __restrict__ pose, EnumList el, int64_t n,
                          int pass, int* __restrict__ zbuf, unsigned long long* __restrict__ hazards) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  float x, y, z, cen[3], t[3];
  enum_xyz(el.axes, el.nax, el.list[e], &x, &y, &z);
  centre_of_corner(g, x, y, z, cen);
  xform(pose->i, cen[0], cen[1], cen[2], t);
  int r, c;
  if (!deproject_valid(cam, t[0], t[1], t[2], r, c)) return;
  const int d = to_int_x86((double)roundf(t[2] * 1000.0f));
  int* px = &zbuf[(int64_t)r * cam.W + c];
  if (pass == 0) {
    if (d == -1) atomicAdd(hazards, 1ull);  // collides with the reference's -1 "unset" marker (:529)
    atomicMin(px, d);
  } else if (*px == d) {
    vd.view[vd.slot_of[lin_index(g, bin_axis(g, 0, x), bin_axis(g, 1, y), bin_axis(g, 2, z))]] = 1;
  }
}

__global__ void k_zbuf_out(const int* __restrict__ z, int64_t n, int* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = z[i] == 0x7fffffff ? -1 : z[i];
}

}  // namespace dmf

using namespace dmf;

extern "C" {

int dmf_reverse_ray_trace_fast(dmf_volume* v, const dmf_camera* cam, const float* poses, int32_t P, int32_t viz,
                               uint8_t* found, int64_t* counts, uint64_t* hashes, int64_t cap) {
  DMF_API_BEGIN
  return reverse_lists(v, cam, poses, P, viz, false, found, counts, hashes, cap);
  DMF_API_END
}

int dmf_reverse_ray_trace(dmf_volume* v, const dmf_camera* cam, const float* poses, int32_t P, int32_t viz,
                          uint8_t* found, int64_t* counts, uint64_t* hashes, int64_t cap) {
  DMF_API_BEGIN
  return reverse_lists(v, cam, poses, P, viz, true, found, counts, hashes, cap);
  DMF_API_END
}

int dmf_reverse_visibility_device(dmf_volume* v, const dmf_camera* cam, const float* d_poses, int32_t P, int32_t viz,
                                  uint64_t* d_visible, uint64_t* d_good, uint64_t* d_stats) {
  DMF_API_BEGIN
  uint64_t *vis, *good;
  int64_t words, nelem;
  DMF_TRY(run_reverse(v, cam, d_poses, P, true, viz, false, &vis, &good, &words, &nelem, nullptr, d_stats));
  const size_t bytes = sizeof(uint64_t) * (size_t)P * words;
  if (bytes) {
    if (d_visible) DMF_HIP(hipMemcpyAsync(d_visible, vis, bytes, hipMemcpyDeviceToDevice, v->stream));
    if (d_good) DMF_HIP(hipMemcpyAsync(d_good, good, bytes, hipMemcpyDeviceToDevice, v->stream));
  }
  return DMF_OK;
  DMF_API_END
}

int dmf_greedy_set_cover(dmf_volume* v, const dmf_camera* cam, const float* poses, int32_t P, int32_t min_gain,
                         int32_t* selected, int32_t* nselected) {
  DMF_API_BEGIN
  if (!poses || !selected || !nselected) return fail(DMF_ERR_INVALID, "null argument");
  uint64_t *vis, *good;
  int64_t words, nelem;
  DMF_TRY(run_reverse(v, cam, poses, P, false, 0, false, &vis, &good, &words, &nelem, nullptr, nullptr));
  return greedy_cover(v, good, P, words, min_gain, selected, nselected);
  DMF_API_END
}

int dmf_ray_trace(dmf_volume* v, const dmf_camera* cam, const float* pose, int32_t zdelta, int32_t sparse) {
  DMF_API_BEGIN
  const int s = sparse ? 5 : 1;  // RayTracingEngine.hpp:274-279
  FwdResult res;
  return run_forward(v, cam, pose, kTrace, 10, zdelta, s, s, 1, &res);
  DMF_API_END
}

int dmf_ray_trace_and_classify(dmf_volume* v, const dmf_camera* cam, const float* pose, int32_t zdelta, int32_t view,
                               int32_t sparse) {
  DMF_API_BEGIN
  const int s = sparse ? 5 : 1;  // :321-326
  FwdResult res;
  return run_forward(v, cam, pose, kClassify, 10, zdelta, s, s, view, &res);
  DMF_API_END
}

int dmf_ray_trace_and_get_minimum(dmf_volume* v, const dmf_camera* cam, const float* pose, int32_t zdelta,
                                  int32_t sparse, int32_t* minimum) {
  DMF_API_BEGIN
  if (!minimum) return fail(DMF_ERR_INVALID, "null output");
  const int s = sparse ? 10 : 1;  // :233-238
  FwdResult res;
  DMF_TRY(run_forward(v, cam, pose, kMinimum, 5, zdelta, s, s, 1, &res));
  *minimum = res.minimum;
  return DMF_OK;
  DMF_API_END
}

int dmf_ray_trace_and_get_points(dmf_volume* v, const dmf_camera* cam, const float* pose, int32_t zdelta,
                                 int32_t sparse, uint8_t* found, uint64_t* hashes, int64_t cap, int64_t* n) {
  DMF_API_BEGIN
  return forward_list_api(v, cam, pose, kPoints, zdelta, sparse, found, hashes, cap, n);
  DMF_API_END
}

int dmf_ray_trace_and_get_good_points(dmf_volume* v, const dmf_camera* cam, const float* pose, int32_t zdelta,
                                      int32_t sparse, uint8_t* found, uint64_t* hashes, int64_t cap, int64_t* n) {
  DMF_API_BEGIN
  return forward_list_api(v, cam, pose, kGoodPoints, zdelta, sparse, found, hashes, cap, n);
  DMF_API_END
}

__global__ void k_first_hit_hash(const int32_t* __restrict__ slot, const uint64_t* __restrict__ hash, int64_t n,
                                 uint64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = slot[i] >= 0 ? hash[slot[i]] : 0;
}

int dmf_forward_first_hits_device(dmf_volume* v, const dmf_camera* cam, const float* d_poses, int32_t P,
                                  int32_t zstart, int32_t zdelta, int32_t rdelta, int32_t cdelta, int32_t* d_k,
                                  int32_t* d_slot, uint64_t* d_stats) {
  DMF_API_BEGIN
  DMF_TRY(require_constructed(v));
  DMF_TRY(check_camera(cam));
  if (!d_poses || !d_k || !d_slot) return fail(DMF_ERR_INVALID, "null argument");
  if (P <= 0 || P > 65535) return fail(DMF_ERR_INVALID, "pose count %d out of range [1,65535]", P);
  if (zdelta <= 0 || rdelta <= 0 || cdelta <= 0) return fail(DMF_ERR_INVALID, "bad strides");
  PoseX* tab;
  DMF_TRY(pose_table(v, d_poses, P, true, &tab));
  const int R = (cam->height + rdelta - 1) / rdelta, C = (cam->width + cdelta - 1) / cdelta;
  void* aux;
  DMF_TRY(scratch(v, kScHost2, 64, &aux));
  DMF_HIP(hipMemsetAsync(aux, 0, 64, v->stream));
  unsigned long long* st = nullptr;
  if (d_stats) DMF_TRY(stats_begin(v, &st));
  if (v->knob[DMF_KNOB_FWD_KERNEL] == 1) {
    // per-XCD unit queues (k_forward_x; persistent: the workgroups the device holds at once)
    unsigned int* heads = (unsigned int*)aux + 8;
    const bool skip = fwd_skip(v);
    if (skip) DMF_TRY(ensure_brick_dist(v));
    const auto kfn = skip ? k_forward_x<true> : k_forward_x<false>;
    int per_cu = 0, ncu = 0;
    DMF_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)kfn, 256, 0));
    DMF_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, v->device));
    const dim3 grid((unsigned)(std::max(ncu, 8) * std::max(per_cu, 1)));
    hipLaunchKernelGGL(kfn, grid, dim3(256), 0, v->stream, v->geom(), v->dev(), cam_params(cam), tab, P, zstart,
                       zdelta, rdelta, cdelta, R, C, d_k, d_slot, heads, (unsigned long long*)aux, st);
  } else if (v->knob[DMF_KNOB_FWD_KERNEL] == 2) {
    // per-wave lane refill over units of kFwdUnit tiles (k_forward_q)
    const int64_t ntiles = (int64_t)((R + 7) / 8) * ((C + 7) / 8), nunits = (ntiles + kFwdUnit - 1) / kFwdUnit;
    const dim3 grid((unsigned)((nunits + 3) / 4), (unsigned)P);
    const bool skip = fwd_skip(v);
    if (skip) DMF_TRY(ensure_brick_dist(v));
    hipLaunchKernelGGL((skip ? k_forward_q<true, kFwdUnit, kFwdRefill, kFwdBurst>
                             : k_forward_q<false, kFwdUnit, kFwdRefill, kFwdBurst>),
                       grid, dim3(256), 0, v->stream, v->geom(), v->dev(), cam_params(cam), tab, zstart, zdelta, rdelta,
                       cdelta, R, C, d_k, d_slot, (unsigned long long*)aux, st);
  } else {
    DMF_TRY(launch_forward(v, cam, tab, P, zstart, zdelta, rdelta, cdelta, R, C, d_k, d_slot,
                           (unsigned long long*)aux, st));
  }
  DMF_LAUNCH_CHECK();
#if defined(DMF_EXP_STATS)
  if (d_stats) DMF_TRY(stats_end(v, st, d_stats, 4));
#else
  if (d_stats) DMF_TRY(stats_end(v, st, d_stats, 1));
#endif
  return DMF_OK;
  DMF_API_END
}

int dmf_forward_first_hits(dmf_volume* v, const dmf_camera* cam, const float* pose, int32_t zstart, int32_t zdelta,
                           int32_t rdelta, int32_t cdelta, int32_t* k_out, uint64_t* hash_out) {
  DMF_API_BEGIN
  DMF_TRY(require_constructed(v));
  DMF_TRY(check_camera(cam));
  if (!pose || !k_out || !hash_out) return fail(DMF_ERR_INVALID, "null argument");
  if (zdelta <= 0 || rdelta <= 0 || cdelta <= 0) return fail(DMF_ERR_INVALID, "bad strides");
  PoseX* tab;
  DMF_TRY(pose_table(v, pose, 1, false, &tab));
  const int R = (cam->height + rdelta - 1) / rdelta, C = (cam->width + cdelta - 1) / cdelta;
  const int64_t RC = (int64_t)R * C;
  void *kb, *sb, *hb, *aux;
  DMF_TRY(scratch(v, kScOut0, sizeof(int32_t) * RC, &kb));
  DMF_TRY(scratch(v, kScOut1, sizeof(int32_t) * RC, &sb));
  DMF_TRY(scratch(v, kScOut2, sizeof(uint64_t) * RC, &hb));
  DMF_TRY(scratch(v, kScHost2, 64, &aux));
  DMF_HIP(hipMemsetAsync(aux, 0, 64, v->stream));
  const dim3 grid((unsigned)((RC + 255) / 256));
  DMF_TRY(launch_forward(v, cam, tab, 1, zstart, zdelta, rdelta, cdelta, R, C, (int32_t*)kb, (int32_t*)sb,
                         (unsigned long long*)aux, nullptr));
  DMF_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_first_hit_hash, grid, dim3(256), 0, v->stream, (const int32_t*)sb, v->d_hash, RC,
                     (uint64_t*)hb);
  DMF_LAUNCH_CHECK();
  DMF_HIP(hipMemcpyAsync(k_out, kb, sizeof(int32_t) * RC, hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipMemcpyAsync(hash_out, hb, sizeof(uint64_t) * RC, hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipStreamSynchronize(v->stream));
  return DMF_OK;
  DMF_API_END
}

int dmf_ray_trace_volume(dmf_volume* v, const dmf_camera* cam, const float* pose, int32_t* depth_out) {
  DMF_API_BEGIN
  DMF_TRY(require_constructed(v));
  DMF_TRY(check_camera(cam));
  if (!pose) return fail(DMF_ERR_INVALID, "null pose");
  DMF_TRY(ensure_enumeration(v));
  PoseX* tab;
  DMF_TRY(pose_table(v, pose, 1, false, &tab));
  const int64_t HW = (int64_t)cam->height * cam->width;
  void *zb, *aux;
  DMF_TRY(scratch(v, kScOut0, sizeof(int) * HW, &zb));
  DMF_TRY(scratch(v, kScHost2, 64, &aux));
  DMF_HIP(hipMemsetD32Async((hipDeviceptr_t)zb, 0x7fffffff, HW, v->stream));
  DMF_HIP(hipMemsetAsync(aux, 0, 64, v->stream));
  EnumList el{v->d_axes, {v->nax[0], v->nax[1], v->nax[2]}, v->d_enum};
  const int64_t n = v->nenum;
  if (n > 0) {
    const dim3 grid((unsigned)((n + 255) / 256));
    for (int pass = 0; pass < 2; ++pass) {
      hipLaunchKernelGGL(k_zbuffer, grid, dim3(256), 0, v->stream, v->geom(), v->dev(), cam_params(cam), tab, el, n,
                         pass, (int*)zb, (unsigned long long*)aux);
      DMF_LAUNCH_CHECK();
    }
  }
  unsigned long long hz = 0;
  DMF_HIP(hipMemcpyAsync(&hz, aux, sizeof(hz), hipMemcpyDeviceToHost, v->stream));
  if (depth_out) {
    void* ob;
    DMF_TRY(scratch(v, kScOut1, sizeof(int) * HW, &ob));
    hipLaunchKernelGGL(k_zbuf_out, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, v->stream, (const int*)zb, HW,
                       (int*)ob);
    DMF_LAUNCH_CHECK();
    DMF_HIP(hipMemcpyAsync(depth_out, ob, sizeof(int) * HW, hipMemcpyDeviceToHost, v->stream));
  }
  DMF_HIP(hipStreamSynchronize(v->stream));
  v->hazards += (int64_t)hz + v->enum_hazards;
  return DMF_OK;
  DMF_API_END
}

}  // extern "C"
