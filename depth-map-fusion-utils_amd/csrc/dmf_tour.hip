// dmf_tour.hip — an open tour over a V x V int32 cost map: the nearest-
// neighbour construction and the first-improvement 2-opt of the reference's TSPSolver.hpp:76-98 and
// :136-156, exact.  map[a][b] is the cost of going from a to b; INT_MAX is "no edge"; a path's
// length is INT_MAX when it holds such an edge, else the sum of its edges (int64 here).
// The reference rebuilds and re-sums the whole path for each candidate (i, k).  Here four inclusive
// prefix arrays over the current path p carry what a candidate needs:
//   Fs[j] = sum of map[p[t-1]][p[t]], t = 1..j      Fc[j] = how many of those are INT_MAX
//   Bs[j] = sum of map[p[t]][p[t-1]], t = 1..j      Bc[j] = likewise
// (an INT_MAX entry adds 0 to a sum and 1 to a count; index 0 holds 0).  Reversing positions i..k
// keeps the edges before i and after k + 1, turns the edges inside round (Bs[k] - Bs[i]) and brings
// two new ones, map[p[i-1]][p[k]] and map[p[i]][p[k+1]]: two gathers, in rows p[i-1] and p[i].
// Kernels:
//  k_to_nn     — one workgroup builds the whole path: V - 1 dependent steps, each an argmin over the
//                unvisited entries of one row (key = value, then index; the visited bits in LDS);
//  k_to_check  — is the path a permutation of 0..V-1?  (an atomic OR per entry on a bit array);
//  k_to_prefix — one workgroup: the four prefix arrays of the path;
//  k_to_sweep  — one round's scan: workgroup i, lanes over k; the improving candidates' least
//                i * V + k goes to ctl->best by one atomic min per wave.  A workgroup whose first key
//                is above the best seen so far leaves at once, and so does every one after `done`;
//  k_to_apply  — one workgroup: nothing improved -> done and converged; else the segment is
//                reversed, the prefix arrays are rebuilt, the new length is checked to be strictly
//                below the old one (else: fault and done) and best is cleared;
//  k_to_info   — the five info words.
// The host enqueues kToBatch rounds (sweep, apply) and then reads `done`; rounds past it are two
// launches that return at their first branch.  The loop ends because every applied round is checked, on
// the device, to have strictly shortened the path: no path comes twice and there are finitely many.
#include <algorithm>
#include <climits>

#include "dmf_host.hpp"

namespace dmf {

constexpr int kToMaxV = 46340;  // V * V < 2^31: a candidate's key i * V + k fits the uint32 `best`
constexpr uint32_t kToNone = 0xffffffffu;
constexpr int kToBatch = 32;       // rounds between two reads of `done`
constexpr int kToWide = 1024;      // threads of the one-workgroup kernels
constexpr int kToSweepThreads = 256;
constexpr int kToBitWords = (kToMaxV + 31) / 32;

struct ToCtl {
  uint32_t best, done, converged, invalid, forced, fault;
  unsigned long long improvements, ahead;
};
static_assert(sizeof(ToCtl) == 40, "the control block as the host reads it");

struct ToPre {
  long long* fs;
  long long* bs;
  uint32_t* fc;
  uint32_t* bc;
  uint32_t* seen;
};

__device__ inline unsigned long long to_min64(unsigned long long a, unsigned long long b) { return a < b ? a : b; }

// The whole construction.  A candidate's key is (value with the sign bit flipped, index): its least
// is the smallest entry below INT_MAX at the lowest index; where no unvisited entry is below
// INT_MAX the lowest unvisited index is taken and counted.
__global__ __launch_bounds__(kToWide) void k_to_nn(const int32_t* __restrict__ map, int V, int32_t* __restrict__ path,
                                                   ToCtl* __restrict__ ctl) {
  __shared__ uint32_t visited[kToBitWords];
  __shared__ unsigned long long skey[kToWide / 64];
  __shared__ uint32_t sfree[kToWide / 64];
  __shared__ int scur;
  const int t = threadIdx.x;
  for (int w = t; w < kToBitWords; w += kToWide) visited[w] = w == 0 ? 1u : 0u;
  if (t == 0) {
    scur = 0;
    path[0] = 0;
  }
  uint32_t forced = 0;
  __syncthreads();
  for (int step = 1; step < V; ++step) {
    const int32_t* const row = map + (size_t)scur * V;
    unsigned long long key = ~0ull;
    uint32_t free_ = kToNone;
    for (int j = t; j < V; j += kToWide) {
      if ((visited[j >> 5] >> (j & 31)) & 1u) continue;
      free_ = min(free_, (uint32_t)j);
      const int32_t c = row[j];
      if (c != INT_MAX) key = to_min64(key, ((unsigned long long)((uint32_t)c ^ 0x80000000u) << 32) | (uint32_t)j);
    }
    for (int o = 32; o > 0; o >>= 1) {
      key = to_min64(key, __shfl_down(key, o, 64));
      free_ = min(free_, (uint32_t)__shfl_down(free_, o, 64));
    }
    if ((t & 63) == 0) {
      skey[t >> 6] = key;
      sfree[t >> 6] = free_;
    }
    __syncthreads();  // the partial minima are written; every read of scur and visited is done
    if (t == 0) {
      for (int w = 1; w < kToWide / 64; ++w) {
        key = to_min64(key, skey[w]);
        free_ = min(free_, sfree[w]);
      }
      const bool dead = key == ~0ull;
      const uint32_t pick = dead ? free_ : (uint32_t)key;
      forced += dead;
      path[step] = (int32_t)pick;
      visited[pick >> 5] |= 1u << (pick & 31u);
      scur = (int)pick;
    }
    __syncthreads();
  }
  if (t == 0) ctl->forced = forced;
}

__global__ __launch_bounds__(256) void k_to_check(const int32_t* __restrict__ path, int V, uint32_t* __restrict__ seen,
                                                  ToCtl* __restrict__ ctl) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= V) return;
  const int32_t p = path[i];
  bool bad = p < 0 || p >= V;
  if (!bad) {
    const uint32_t m = 1u << (p & 31);
    bad = (atomicOr(&seen[p >> 5], m) & m) != 0;
  }
  if (bad) atomicOr(&ctl->invalid, 1u);
}

// The four prefix arrays of `path`, by one workgroup of kToWide threads: thread t owns the
// positions [t * per, (t + 1) * per), sums them, the sums are scanned across the workgroup, and
// the positions are written in a second walk.
__device__ inline void to_rebuild(const int32_t* __restrict__ map, int V, const int32_t* path, const ToPre& pre) {
  __shared__ long long wf[kToWide / 64], wb[kToWide / 64];
  __shared__ uint32_t wcf[kToWide / 64], wcb[kToWide / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int per = (V + kToWide - 1) / kToWide;
  const int j0 = min(t * per, V), j1 = min(j0 + per, V);
  long long f = 0, b = 0;
  uint32_t cf = 0, cb = 0;
  for (int j = max(j0, 1); j < j1; ++j) {
    const int32_t u = path[j - 1], x = path[j];
    const int32_t ef = map[(size_t)u * V + x], eb = map[(size_t)x * V + u];
    f += ef == INT_MAX ? 0 : ef;
    cf += ef == INT_MAX;
    b += eb == INT_MAX ? 0 : eb;
    cb += eb == INT_MAX;
  }
  // inclusive scan over the lanes of a wave, then over the waves
  long long sf = f, sb = b;
  uint32_t scf = cf, scb = cb;
  for (int o = 1; o < 64; o <<= 1) {
    const long long af = __shfl_up(sf, o, 64), ab = __shfl_up(sb, o, 64);
    const uint32_t acf = __shfl_up(scf, o, 64), acb = __shfl_up(scb, o, 64);
    if (lane >= o) {
      sf += af;
      sb += ab;
      scf += acf;
      scb += acb;
    }
  }
  __syncthreads();  // (a second call: the previous one's reads of the wave totals are done)
  if (lane == 63) {
    wf[w] = sf;
    wb[w] = sb;
    wcf[w] = scf;
    wcb[w] = scb;
  }
  __syncthreads();
  long long of = sf - f, ob = sb - b;  // exclusive: what lies before this thread's positions
  uint32_t ocf = scf - cf, ocb = scb - cb;
  for (int k = 0; k < w; ++k) {
    of += wf[k];
    ob += wb[k];
    ocf += wcf[k];
    ocb += wcb[k];
  }
  for (int j = j0; j < j1; ++j) {
    if (j > 0) {
      const int32_t u = path[j - 1], x = path[j];
      const int32_t ef = map[(size_t)u * V + x], eb = map[(size_t)x * V + u];
      of += ef == INT_MAX ? 0 : ef;
      ocf += ef == INT_MAX;
      ob += eb == INT_MAX ? 0 : eb;
      ocb += eb == INT_MAX;
    }
    pre.fs[j] = of;
    pre.bs[j] = ob;
    pre.fc[j] = ocf;
    pre.bc[j] = ocb;
  }
}

__global__ __launch_bounds__(kToWide) void k_to_prefix(const int32_t* __restrict__ map, int V,
                                                       const int32_t* __restrict__ path, ToPre pre) {
  to_rebuild(map, V, path, pre);
}

// Workgroup blockIdx.x takes i = blockIdx.x + 1 (V - 2 workgroups: i = V - 1 has no k).
__global__ __launch_bounds__(kToSweepThreads) void k_to_sweep(const int32_t* __restrict__ map, int V,
                                                              const int32_t* __restrict__ path, ToPre pre,
                                                              ToCtl* ctl) {
  const int i = (int)blockIdx.x + 1;
  if (ctl->done) return;
  const uint32_t first = (uint32_t)i * (uint32_t)V + (uint32_t)i + 1u;
  // any value read here is an upper bound of the round's result: best is only lowered
  if (__hip_atomic_load(&ctl->best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < first) return;
  const long long total = pre.fs[V - 1];
  const uint32_t totalc = pre.fc[V - 1];
  const long long cur = totalc ? (long long)INT_MAX : total;
  const int32_t* const rowa = map + (size_t)path[i - 1] * V;
  const int32_t* const rowb = map + (size_t)path[i] * V;
  const long long head = pre.fs[i - 1] - pre.bs[i];
  const uint32_t headc = pre.fc[i - 1] - pre.bc[i];  // (mod 2^32, as every count below: the end result is exact)
  uint32_t key = kToNone;
  for (int k = i + 1 + (int)threadIdx.x; k < V; k += kToSweepThreads) {
    const int32_t e1 = rowa[path[k]];
    long long s = head + pre.bs[k] + (e1 == INT_MAX ? 0 : e1);
    uint32_t c = headc + pre.bc[k] + (uint32_t)(e1 == INT_MAX);
    if (k + 1 < V) {
      const int32_t e2 = rowb[path[k + 1]];
      s += (e2 == INT_MAX ? 0 : e2) + (total - pre.fs[k + 1]);
      c += (uint32_t)(e2 == INT_MAX) + (totalc - pre.fc[k + 1]);
    }
    if ((c ? (long long)INT_MAX : s) < cur) {
      key = (uint32_t)i * (uint32_t)V + (uint32_t)k;
      break;  // (a lane's k only grow)
    }
  }
  for (int o = 32; o > 0; o >>= 1) key = min(key, (uint32_t)__shfl_down(key, o, 64));
  if ((threadIdx.x & 63) == 0 && key != kToNone) atomicMin(&ctl->best, key);
}

__global__ __launch_bounds__(kToWide) void k_to_apply(const int32_t* __restrict__ map, int V, int32_t* path, ToPre pre,
                                                      ToCtl* ctl, unsigned long long max_rounds) {
  if (ctl->done) return;
  const uint32_t best = ctl->best;
  if (best == kToNone) {
    if (threadIdx.x == 0) {
      ctl->done = 1;
      ctl->converged = 1;
    }
    return;
  }
  const int i = (int)(best / (uint32_t)V), k = (int)(best % (uint32_t)V);
  const long long was = pre.fc[V - 1] ? (long long)INT_MAX : pre.fs[V - 1];  // (read before the rebuild's first barrier)
  for (int h = threadIdx.x; h < (k - i + 1) / 2; h += kToWide) {
    const int32_t a = path[i + h], b = path[k - h];
    path[i + h] = b;
    path[k - h] = a;
  }
  __syncthreads();  // (the workgroup's own stores: visible to it past the barrier)
  to_rebuild(map, V, path, pre);
  __syncthreads();  // the last position's sums are written
  if (threadIdx.x == 0) {
    // what the scan promised, checked on the rebuilt sums: a strictly shorter path.  It is what ends
    // the solve (no path comes twice), so a round that breaks it -- a map changed under the call --
    // stops the solve with a fault instead of trusting the next scan
    if (!((pre.fc[V - 1] ? (long long)INT_MAX : pre.fs[V - 1]) < was)) {
      ctl->fault = 1;
      ctl->done = 1;
    }
    const unsigned long long n = ctl->improvements + 1;
    ctl->improvements = n;
    // the candidates ahead of (i, k) in the scan: rows 1 .. i - 1 in full, then k - i - 1
    ctl->ahead += (unsigned long long)(i - 1) * (unsigned long long)(V - 1) -
                  (unsigned long long)(i - 1) * (unsigned long long)i / 2 + (unsigned long long)(k - i - 1);
    ctl->best = kToNone;
    if (max_rounds && n >= max_rounds) ctl->done = 1;
  }
}

// info[5] = {forced picks, improvements, converged, the sum of the path's edges below INT_MAX, its INT_MAX edges}
__global__ __launch_bounds__(64) void k_to_info(int V, ToPre pre, const ToCtl* __restrict__ ctl,
                                                unsigned long long* __restrict__ info) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  info[0] = ctl->forced;
  info[1] = ctl->improvements;
  info[2] = ctl->converged;
  info[3] = V > 0 ? (unsigned long long)pre.fs[V - 1] : 0ull;
  info[4] = V > 0 ? pre.fc[V - 1] : 0u;
}

// The plain arguments first (no access to the volume).
static int check_tour_args(const dmf_volume* v, const void* map, int32_t V, const void* path, int64_t max_rounds) {
  if (!v) return fail(DMF_ERR_INVALID, "null volume");
  if (V < 0) return fail(DMF_ERR_INVALID, "negative V %d", V);
  if (V > kToMaxV) return fail(DMF_ERR_RANGE, "a tour is limited to %d nodes, got %d", kToMaxV, V);
  if (V > 0 && (!map || !path)) return fail(DMF_ERR_INVALID, "null argument");
  if (max_rounds < 0) return fail(DMF_ERR_INVALID, "negative max_rounds %lld", (long long)max_rounds);
  return DMF_OK;
}

enum { kToNN = 1, kToTwoOpt = 2 };

// what & kToNN: d_path is built; what & kToTwoOpt: d_path (given, or just built) is improved.
// Waits for its own rounds; d_info (device, may be null) is complete when it returns.
static int tour_device(dmf_volume* v, const int32_t* d_map, int V, int32_t* d_path, int64_t max_rounds, int what,
                       uint64_t* d_info) {
  void *ctlp, *prep;
  const size_t nv = (size_t)std::max(V, 1), bitw = (nv + 31) / 32;
  DMF_TRY(scratch(v, kScToCtl, sizeof(ToCtl), &ctlp));
  DMF_TRY(scratch(v, kScToPre, nv * 24 + bitw * 4, &prep));
  ToCtl* const ctl = (ToCtl*)ctlp;
  ToPre pre;
  pre.fs = (long long*)prep;
  pre.bs = pre.fs + nv;
  pre.fc = (uint32_t*)(pre.bs + nv);
  pre.bc = pre.fc + nv;
  pre.seen = pre.bc + nv;
  ToCtl h = {kToNone, 0, 0, 0, 0, 0, 0, 0};
  DMF_HIP(hipMemcpyAsync(ctlp, &h, sizeof(h), hipMemcpyHostToDevice, v->stream));
  for (int k = 0; k < 4; ++k) v->tour_stats[k] = 0;
  if (V > 0) {
    if (what & kToNN) {
      hipLaunchKernelGGL(k_to_nn, dim3(1), dim3(kToWide), 0, v->stream, d_map, V, d_path, ctl);
      DMF_LAUNCH_CHECK();
    } else {
      DMF_HIP(hipMemsetAsync(pre.seen, 0, bitw * 4, v->stream));
      hipLaunchKernelGGL(k_to_check, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, v->stream,
                         (const int32_t*)d_path, V, pre.seen, ctl);
      DMF_LAUNCH_CHECK();
      DMF_HIP(hipMemcpyAsync(&h, ctlp, sizeof(h), hipMemcpyDeviceToHost, v->stream));
      DMF_HIP(hipStreamSynchronize(v->stream));
      if (h.invalid) return fail(DMF_ERR_INVALID, "the path is not a permutation of 0..%d", V - 1);
    }
    hipLaunchKernelGGL(k_to_prefix, dim3(1), dim3(kToWide), 0, v->stream, d_map, V, (const int32_t*)d_path, pre);
    DMF_LAUNCH_CHECK();
  }
  if ((what & kToTwoOpt) && V >= 3) {
    uint64_t rounds = 0, batches = 0;
    do {
      for (int r = 0; r < kToBatch; ++r) {
        hipLaunchKernelGGL(k_to_sweep, dim3((unsigned)(V - 2)), dim3(kToSweepThreads), 0, v->stream, d_map, V,
                           (const int32_t*)d_path, pre, ctl);
        DMF_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_to_apply, dim3(1), dim3(kToWide), 0, v->stream, d_map, V, d_path, pre, ctl,
                           (unsigned long long)max_rounds);
        DMF_LAUNCH_CHECK();
      }
      rounds += kToBatch;
      ++batches;
      DMF_HIP(hipMemcpyAsync(&h, ctlp, sizeof(h), hipMemcpyDeviceToHost, v->stream));
      DMF_HIP(hipStreamSynchronize(v->stream));
    } while (!h.done);
    if (h.fault)
      return fail(DMF_ERR_DEVICE_CHECK, "a 2-opt round did not shorten the path (round %llu): was the map changed under the call?",
                  (unsigned long long)h.improvements);
    v->tour_stats[0] = rounds;
    v->tour_stats[1] = batches;
    v->tour_stats[2] = h.improvements;
    v->tour_stats[3] = h.ahead;
  } else if (what & kToTwoOpt) {
    // V < 3 has no candidate: the scan that finds nothing is empty
    h.converged = 1;
    DMF_HIP(hipMemcpyAsync(&ctl->converged, &h.converged, sizeof(uint32_t), hipMemcpyHostToDevice, v->stream));
  }
  if (d_info) {
    hipLaunchKernelGGL(k_to_info, dim3(1), dim3(64), 0, v->stream, V, pre, (const ToCtl*)ctl,
                       (unsigned long long*)d_info);
    DMF_LAUNCH_CHECK();
  }
  DMF_HIP(hipStreamSynchronize(v->stream));  // (h was the source of the copies above)
  return DMF_OK;
}

// The host forms: map and path through scratch, info back.
static int tour_host(dmf_volume* v, const int32_t* map, int V, int32_t* path, int64_t max_rounds, int what,
                     uint64_t* info) {
  void *dm = nullptr, *dp = nullptr, *di;
  const size_t mapb = sizeof(int32_t) * (size_t)V * (size_t)V, pathb = sizeof(int32_t) * (size_t)V;
  DMF_TRY(scratch(v, kScToInfo, sizeof(uint64_t) * 5, &di));
  if (V > 0) {
    DMF_TRY(scratch(v, kScToMap, mapb, &dm));
    DMF_TRY(scratch(v, kScToPath, pathb, &dp));
    DMF_HIP(hipMemcpyAsync(dm, map, mapb, hipMemcpyHostToDevice, v->stream));
    if (!(what & kToNN)) DMF_HIP(hipMemcpyAsync(dp, path, pathb, hipMemcpyHostToDevice, v->stream));
  }
  DMF_TRY(tour_device(v, (const int32_t*)dm, V, (int32_t*)dp, max_rounds, what, (uint64_t*)di));
  if (V > 0) DMF_HIP(hipMemcpyAsync(path, dp, pathb, hipMemcpyDeviceToHost, v->stream));
  if (info) DMF_HIP(hipMemcpyAsync(info, di, sizeof(uint64_t) * 5, hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipStreamSynchronize(v->stream));
  return DMF_OK;
}

}  // namespace dmf

using namespace dmf;

extern "C" {

int dmf_tour_nearest_neighbour_device(dmf_volume* v, const int32_t* d_map, int32_t V, int32_t* d_path, uint64_t* d_info5) {
  DMF_API_BEGIN
  DMF_TRY(check_tour_args(v, d_map, V, d_path, 0));
  DMF_TRY(activate(v));
  return tour_device(v, d_map, V, d_path, 0, kToNN, d_info5);
  DMF_API_END
}

int dmf_tour_nearest_neighbour(dmf_volume* v, const int32_t* map, int32_t V, int32_t* path, uint64_t* info5) {
  DMF_API_BEGIN
  DMF_TRY(check_tour_args(v, map, V, path, 0));
  DMF_TRY(activate(v));
  return tour_host(v, map, V, path, 0, kToNN, info5);
  DMF_API_END
}

int dmf_tour_two_opt_device(dmf_volume* v, const int32_t* d_map, int32_t V, int32_t* d_path, int64_t max_rounds,
                            uint64_t* d_info5) {
  DMF_API_BEGIN
  DMF_TRY(check_tour_args(v, d_map, V, d_path, max_rounds));
  DMF_TRY(activate(v));
  return tour_device(v, d_map, V, d_path, max_rounds, kToTwoOpt, d_info5);
  DMF_API_END
}

int dmf_tour_two_opt(dmf_volume* v, const int32_t* map, int32_t V, int32_t* path, int64_t max_rounds, uint64_t* info5) {
  DMF_API_BEGIN
  DMF_TRY(check_tour_args(v, map, V, path, max_rounds));
  DMF_TRY(activate(v));
  return tour_host(v, map, V, path, max_rounds, kToTwoOpt, info5);
  DMF_API_END
}

int dmf_tour_device(dmf_volume* v, const int32_t* d_map, int32_t V, int32_t* d_path, int64_t max_rounds,
                    uint64_t* d_info5) {
  DMF_API_BEGIN
  DMF_TRY(check_tour_args(v, d_map, V, d_path, max_rounds));
  DMF_TRY(activate(v));
  return tour_device(v, d_map, V, d_path, max_rounds, kToNN | kToTwoOpt, d_info5);
  DMF_API_END
}

int dmf_tour(dmf_volume* v, const int32_t* map, int32_t V, int32_t* path, int64_t max_rounds, uint64_t* info5) {
  DMF_API_BEGIN
  DMF_TRY(check_tour_args(v, map, V, path, max_rounds));
  DMF_TRY(activate(v));
  return tour_host(v, map, V, path, max_rounds, kToNN | kToTwoOpt, info5);
  DMF_API_END
}

int dmf_tour_stats(const dmf_volume* v, uint64_t* stats4) {
  DMF_API_BEGIN
  if (!v || !stats4) return fail(DMF_ERR_INVALID, "null argument");
  for (int k = 0; k < 4; ++k) stats4[k] = v->tour_stats[k];
  return DMF_OK;
  DMF_API_END
}

}  // extern "C"
