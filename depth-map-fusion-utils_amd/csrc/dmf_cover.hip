// dmf_cover.hip — greedySetCover (Algorithms.hpp:38-86) over per-pose bitmasks on gfx950: the
// reverse march's good masks (dmf_trace.hip) or the view-gain masks (dmf_viewgain.hip).
#include <algorithm>

#include "dmf_host.hpp"

namespace dmf {

// The reference scans the remaining set ids in increasing order and keeps the
// strictly largest |set \ covered|; with sets as bitmasks over occupied slots that
// difference size is popcount(good[p] & ~covered).  One iteration = gain, pick,
// merge; every kernel returns at once after the stop condition.
struct CoverCtl {
  int done;
  int sel;
  int nsel;
};

__global__ __launch_bounds__(256) void k_cover_gain(const uint64_t* __restrict__ masks, int64_t words,
                                                    const uint64_t* __restrict__ covered,
                                                    const uint8_t* __restrict__ removed,
                                                    unsigned long long* __restrict__ gain,
                                                    const CoverCtl* __restrict__ ctl) {
  if (ctl->done) return;
  const int p = blockIdx.x;
  if (removed[p]) {
    if (threadIdx.x == 0) gain[p] = 0;
    return;
  }
  const uint64_t* m = masks + (int64_t)p * words;
  unsigned long long c = 0;
  for (int64_t w = threadIdx.x; w < words; w += blockDim.x) c += __popcll(m[w] & ~covered[w]);
  __shared__ unsigned long long part[4];
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) gain[p] = part[0] + part[1] + part[2] + part[3];
}

// The pick's order: the larger gain, and among equal gains the smaller index.
__device__ __forceinline__ bool cover_better(unsigned long long g, int p, unsigned long long bg, int bp) {
  return g > bg || (g == bg && p < bp);
}

__global__ __launch_bounds__(256) void k_cover_pick(const unsigned long long* __restrict__ gain, int P, int min_gain,
                                                    uint8_t* __restrict__ removed, int32_t* __restrict__ selected,
                                                    CoverCtl* __restrict__ ctl) {
  if (ctl->done) return;
  // argmax with ties to the smallest index, over the pair (gain, index): the gain keeps all its
  // 64 bits (up to 64 * words), so the two do not share one key
  unsigned long long g = 0;
  int p = P;
  for (int q = threadIdx.x; q < P; q += blockDim.x)
    if (cover_better(gain[q], q, g, p)) { g = gain[q]; p = q; }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long tg = __shfl_down(g, o, 64);
    const int tp = __shfl_down(p, o, 64);
    if (cover_better(tg, tp, g, p)) { g = tg; p = tp; }
  }
  __shared__ unsigned long long part_g[4];
  __shared__ int part_p[4];
  if ((threadIdx.x & 63) == 0) { part_g[threadIdx.x >> 6] = g; part_p[threadIdx.x >> 6] = p; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i)
      if (cover_better(part_g[i], part_p[i], g, p)) { g = part_g[i]; p = part_p[i]; }
    // selected == -1, or max_points < 5 (a signed compare: min_gain <= 0 stops at "adds nothing" alone)
    if (g == 0 || (min_gain > 0 && g < (unsigned long long)min_gain)) {
      ctl->done = 1;
    } else {
      ctl->sel = p;
      selected[ctl->nsel++] = p;
      removed[p] = 1;
    }
  }
}

__global__ __launch_bounds__(256) void k_cover_merge(const uint64_t* __restrict__ masks, int64_t words,
                                                     uint64_t* __restrict__ covered, const CoverCtl* __restrict__ ctl) {
  if (ctl->done) return;
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w < words) covered[w] |= masks[(int64_t)ctl->sel * words + w];
}

int greedy_cover(dmf_volume* v, const uint64_t* d_masks, int P, int64_t words, int min_gain, int32_t* selected,
                 int32_t* nselected) {
  if (P <= 0) { *nselected = 0; return DMF_OK; }
  void *cov, *aux;
  const size_t cov_bytes = sizeof(uint64_t) * (size_t)std::max<int64_t>(words, 1);
  DMF_TRY(scratch(v, kScTmp, cov_bytes, &cov));
  const size_t gain_off = 64, rem_off = gain_off + sizeof(unsigned long long) * P,
               sel_off = rem_off + ((size_t)P + 7) / 8 * 8;
  DMF_TRY(scratch(v, kScCount, sel_off + sizeof(int32_t) * P, &aux));
  CoverCtl* ctl = (CoverCtl*)aux;
  unsigned long long* gain = (unsigned long long*)((char*)aux + gain_off);
  uint8_t* removed = (uint8_t*)aux + rem_off;
  int32_t* sel = (int32_t*)((char*)aux + sel_off);
  DMF_HIP(hipMemsetAsync(cov, 0, cov_bytes, v->stream));
  DMF_HIP(hipMemsetAsync(aux, 0, sel_off, v->stream));
  const unsigned mb = (unsigned)((words + 255) / 256);
  for (int it = 0; it < P; it += 8) {
    for (int k = it; k < std::min(P, it + 8); ++k) {
      hipLaunchKernelGGL(k_cover_gain, dim3((unsigned)P), dim3(256), 0, v->stream, d_masks, words,
                         (const uint64_t*)cov, removed, gain, ctl);
      hipLaunchKernelGGL(k_cover_pick, dim3(1), dim3(256), 0, v->stream, gain, P, min_gain, removed, sel, ctl);
      if (mb) hipLaunchKernelGGL(k_cover_merge, dim3(mb), dim3(256), 0, v->stream, d_masks, words, (uint64_t*)cov, ctl);
    }
    DMF_LAUNCH_CHECK();
    CoverCtl h;
    DMF_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, v->stream));
    DMF_HIP(hipStreamSynchronize(v->stream));
    if (h.done) break;
  }
  CoverCtl h;
  DMF_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipStreamSynchronize(v->stream));
  if (h.nsel) DMF_HIP(hipMemcpy(selected, sel, sizeof(int32_t) * h.nsel, hipMemcpyDeviceToHost));
  *nselected = h.nsel;
  return DMF_OK;
}

}  // namespace dmf

using namespace dmf;

extern "C" {

int dmf_greedy_set_cover_masks_device(dmf_volume* v, const uint64_t* d_masks, int32_t P, int64_t words,
                                      int32_t min_gain, int32_t* selected, int32_t* nselected) {
  DMF_API_BEGIN
  DMF_TRY(require_constructed(v));
  if (!selected || !nselected || (P > 0 && !d_masks)) return fail(DMF_ERR_INVALID, "null argument");
  if (P < 0 || P > 65535 || words < 0) return fail(DMF_ERR_INVALID, "bad set count / width");
  return greedy_cover(v, d_masks, P, words, min_gain, selected, nselected);
  DMF_API_END
}

}  // extern "C"
