// dmf_distance.hip — the exact squared Euclidean distance field of a fused log-odds grid and the
// clearance of path segments in it.  dist2[x][y][z] = the least
// (x-x')^2 + (y-y')^2 + (z-z')^2 over the solid cells (L >= threshold), in cell-index units, by a
// separable transform in integers (Felzenszwalb & Huttenlocher's lower envelope of parabolas):
//  k_df_z     — one streaming pass over the grid.  A workgroup takes whole (x, y) rows, up to
//               kDfZCells contiguous cells: 16-B loads (for_cells8, dmf_gridbits.hpp) make the rows'
//               solid bits in LDS, a wave scan
//               over the words gives every word the nearest set bit before and after it, and each
//               cell's squared distance to the nearest solid cell OF ITS ROW (clz / ctz in its own
//               word, else the word's neighbours, cut at the row's ends) is stored 16 B per lane.
//               A row without a solid cell is infinite (kDfInf); the solid cells are counted;
//  k_df_axis  — the pass along y, then the same kernel along x, in place.  One lane per column of
//               the pass axis, lanes adjacent in memory (along z, and for x over the whole (y, z)
//               plane), so every step of the walk is one coalesced row access.  A lane builds the
//               lower envelope of its column's finite sites, then fills the column from it.  The
//               envelope's stack lives in a global scratch laid out [entry][column], lane-adjacent
//               like the grid itself; the top entry stays in registers and the newest 16 entries
//               of every lane also in LDS, where a pop finds them.  Infinite sites are
//               skipped: they never enter the stack or the arithmetic, and a column without a
//               finite site is left as it is, infinite for the next pass.  kDfInf = DMF_NO_DIST, so
//               what is still infinite after the last pass already is the result;
//  k_df_clear — one lane per segment: the fusion's own ray (endpoint acceptance, clip, quantisation,
//               dda_setup and the Walk of dmf_dda.hpp), the minimum of dist2 over its cells.
// All arithmetic is int32 / uint32: d^2 <= 3 * 2047^2 < 2^24, and a separator's numerator
// f(q) + q^2 - f(v) - v^2 stays below 2^25 in magnitude.
#include "dmf_dda.hpp"
#include "dmf_host.hpp"

namespace dmf {

constexpr uint32_t kDfInf = 0xffffffffu;  // "no solid cell yet"; = DMF_NO_DIST
static_assert(kDfInf == DMF_NO_DIST, "what stays infinite after the last pass is the result");

constexpr int kDfZThreads = 256;
constexpr int kDfZCells = 4096;  // cells of a workgroup's whole rows (at least one row: <= 2048 cells)
constexpr int kDfZWords = 192;   // 3 words per lane of the scanning wave; the span needs <= 130
constexpr int kDfFar = 1 << 20;  // a position no cell of a span has
static_assert((kDfZCells + 14 + 31) / 32 + 1 <= kDfZWords, "span plus its alignment slack");

// The rows [r0, r1) of a workgroup are the contiguous cells [lo, hi).  Bit positions are relative
// to a0 = lo rounded down to 8 cells, so that every 8-cell group is a 16-B aligned load whatever
// the row length; the up to 7 cells before lo and after hi belong to other rows (or lie past the
// grid, where nothing is read) and are cut off by the row's own ends.
__global__ __launch_bounds__(kDfZThreads) void k_df_z(int64_t ncell, int nz, int rows_per_wg, int64_t nrows,
                                                      const int16_t* __restrict__ L, int threshold,
                                                      uint32_t* __restrict__ out,
                                                      unsigned long long* __restrict__ nsolid) {
  __shared__ uint32_t bits[kDfZWords];
  __shared__ int32_t before[kDfZWords];  // the highest set bit in the words below, or -1
  __shared__ int32_t after[kDfZWords];   // the lowest set bit in the words above, or kDfFar
  __shared__ uint32_t scount;
  const int i = threadIdx.x, lane = i & 63;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg, r1 = r0 + rows_per_wg < nrows ? r0 + rows_per_wg : nrows;
  const int64_t lo = r0 * nz, hi = r1 * nz, a0 = lo & ~(int64_t)7;
  const int ngroups = (int)((hi - a0 + 7) >> 3);
  if (i < kDfZWords) bits[i] = 0;
  if (i == 0) scount = 0;
  __syncthreads();
  for (int j = i; j < ngroups; j += kDfZThreads) {
    const int64_t p = a0 + 8 * (int64_t)j;
    uint32_t b = 0;
    for_cells8(L + p, (int)(ncell - p < 8 ? ncell - p : 8),
               [&](int k, int c) { b |= (uint32_t)(c >= threshold) << k; });
    ((unsigned char*)bits)[j] = (unsigned char)b;
  }
  __syncthreads();
  // wave 0: before[], wave 1: after[]; lane l owns the words 3l .. 3l + 2
  if (i < 128) {
    const int k0 = 3 * lane;
    const uint32_t w0 = bits[k0], w1 = bits[k0 + 1], w2 = bits[k0 + 2];
    if (i < 64) {
      const int h0 = w0 ? 32 * k0 + 31 - __clz((int)w0) : -1;
      const int h1 = w1 ? 32 * k0 + 63 - __clz((int)w1) : -1;
      const int h2 = w2 ? 32 * k0 + 95 - __clz((int)w2) : -1;
      int inc = max(h0, max(h1, h2));
      for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o, 64);
        if (lane >= o) inc = max(inc, u);
      }
      int ex = __shfl_up(inc, 1, 64);
      if (lane == 0) ex = -1;
      before[k0] = ex;
      before[k0 + 1] = max(ex, h0);
      before[k0 + 2] = max(ex, max(h0, h1));
    } else {
      const int l0 = w0 ? 32 * k0 + __ffs((int)w0) - 1 : kDfFar;
      const int l1 = w1 ? 32 * k0 + 32 + __ffs((int)w1) - 1 : kDfFar;
      const int l2 = w2 ? 32 * k0 + 64 + __ffs((int)w2) - 1 : kDfFar;
      int inc = min(l0, min(l1, l2));
      for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_down(inc, o, 64);
        if (lane + o < 64) inc = min(inc, u);
      }
      int ex = __shfl_down(inc, 1, 64);
      if (lane == 63) ex = kDfFar;
      after[k0 + 2] = ex;
      after[k0 + 1] = min(ex, l2);
      after[k0] = min(ex, min(l1, l2));
    }
  }
  __syncthreads();
  // four cells per lane and step, aligned to 4 cells: one 16-B store where all four are the span's
  const bool out_aligned = ((uintptr_t)out & 15) == 0;
  uint32_t c = 0;
  for (int64_t p4 = (lo & ~(int64_t)3) + 4 * (int64_t)i; p4 < hi; p4 += 4 * kDfZThreads) {
    const int64_t pf = p4 < lo ? lo : p4;
    const uint32_t rr = (uint32_t)(pf - lo) / (uint32_t)nz;
    int64_t a = lo + (int64_t)rr * nz, b = a + nz;  // the row of the current cell
    uint32_t d2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t p = p4 + k;
      d2[k] = kDfInf;
      if (p >= lo && p < hi) {
        if (p >= b) { a = b; b += nz; }
        const int pr = (int)(p - a0), ar = (int)(a - a0), br = (int)(b - a0);
        const int w = pr >> 5, bit = pr & 31;
        const uint32_t word = bits[w];
        const uint32_t mb = word & (0xffffffffu >> (31 - bit)), ma = word & (0xffffffffu << bit);
        const int pb = mb ? (w << 5) + 31 - __clz((int)mb) : before[w];
        const int pa = ma ? (w << 5) + __ffs((int)ma) - 1 : after[w];
        int d = kDfFar;
        if (pb >= ar) d = pr - pb;
        if (pa < br) d = min(d, pa - pr);
        if (d < kDfFar) d2[k] = (uint32_t)(d * d);
        c += d == 0;
      }
    }
    if (out_aligned && p4 >= lo && p4 + 4 <= hi) {
      *(uint4*)(out + p4) = make_uint4(d2[0], d2[1], d2[2], d2[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (p4 + k >= lo && p4 + k < hi) out[p4 + k] = d2[k];
    }
  }
  if (nsolid) {
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    if (lane == 0 && c) atomicAdd(&scount, c);
    __syncthreads();
    if (i == 0 && scount) atomicAdd(nsolid, (unsigned long long)scount);
  }
}

// One pass of the transform along an axis of n cells, in place.  Column c of ncols lies at
// f + (c / inner) * outer + (c % inner), its cells `stride` apart: along y, inner = zdim (c = x *
// zdim + z), outer = ydim * zdim, stride = zdim; along x, inner = ncols = ydim * zdim, stride =
// ydim * zdim.  Entry k of column c's stack is stk[k * ncols + c] = {g, site | start << 16}.
//
// The parabola of a finite site v is P_v(t) = (t - v)^2 + f(v) = t^2 - 2 v t + g_v with g_v = f(v) +
// v^2.  For v < q, P_q(t) < P_v(t) iff t > (g_q - g_v) / (2 (q - v)), so q is the better site
// from s = floor(that quotient) + 1 on, and v is at least as good before.  Sites come in ascending
// order: q pops every top entry that starts at or after s, then is pushed with start s -- unless
// s >= n, where it could only win past the column's end (it lies on or above the envelope over the
// whole column, so dropping it changes no value).  The bottom entry starts at 0.  Starts ascend
// strictly, so at most n entries exist, and site (< 2^11) and start (< 2^11) share one word.
//
// A pop must have the entry below the top before the walk can go on, and a load of it from the
// global stack is a full memory latency on the lane's critical path.  So the newest kDfWin entries
// of every lane are also kept in LDS, entry k in win[k % kDfWin][lane] (lane-adjacent: no bank
// conflict between lanes at equal depth): a push stores to both, a pop reads LDS when the entry
// is still there (k >= wlo: no later push has taken its place) and the global stack otherwise.
constexpr int kDfAxisThreads = 256, kDfAhead = 8, kDfWin = 16;
__global__ __launch_bounds__(kDfAxisThreads) void k_df_axis(int n, int64_t stride, uint32_t inner, int64_t outer,
                                                            uint32_t ncols, uint32_t* __restrict__ f,
                                                            uint2* __restrict__ stk) {
  __shared__ uint2 win[kDfWin][kDfAxisThreads];
  const uint32_t c = blockIdx.x * (uint32_t)kDfAxisThreads + threadIdx.x;
  if (c >= ncols) return;
  const uint32_t co = c / inner;
  uint32_t* const col = f + ((int64_t)co * outer + (int64_t)(c - co * inner));
  uint2* const S = stk + c;
  int k = -1;  // the top entry's index; the entry itself in tv, tg, ts (and in S[k * ncols])
  int wlo = 0;  // entries wlo .. k are in the LDS window
  int32_t tv = 0, tg = 0, ts = 0;
  for (int q0 = 0; q0 < n; q0 += kDfAhead) {
    uint32_t fv[kDfAhead];
#pragma unroll
    for (int j = 0; j < kDfAhead; ++j) fv[j] = q0 + j < n ? col[(int64_t)(q0 + j) * stride] : kDfInf;
#pragma unroll
    for (int j = 0; j < kDfAhead; ++j) {
      if (fv[j] != kDfInf) {
        const int32_t q = q0 + j, gq = (int32_t)fv[j] + q * q;
        int32_t s = 0;
        while (k >= 0) {
          const int32_t num = gq - tg, den = 2 * (q - tv);
          s = (num >= 0 ? num / den : -((den - 1 - num) / den)) + 1;
          if (s > ts) break;
          if (--k >= 0) {
            uint2 e;
            if (k >= wlo) {
              e = win[k & (kDfWin - 1)][threadIdx.x];
            } else {
              e = S[(int64_t)k * ncols];
              wlo = k + 1;  // (nothing below the top is in the window any more)
            }
            tg = (int32_t)e.x;
            tv = (int32_t)(e.y & 0xffffu);
            ts = (int32_t)(e.y >> 16);
          }
        }
        if (k < 0) s = 0;
        if (s < n) {
          ++k;
          tv = q;
          tg = gq;
          ts = s;
          const uint2 e = make_uint2((uint32_t)tg, (uint32_t)tv | (uint32_t)ts << 16);
          S[(int64_t)k * ncols] = e;
          win[k & (kDfWin - 1)][threadIdx.x] = e;
          wlo = wlo > k - (kDfWin - 1) ? wlo : k - (kDfWin - 1);
        }
      }
    }
  }
  if (k < 0) return;  // no finite site: the column stays infinite
  // the fill: entry k is current; k + 1 (whose start ends k's range) and k + 2 are read ahead, so
  // that a step into the next range does not wait for memory
  const int top = k;
  uint2 e0 = S[0], e1 = e0, e2 = e0;
  if (top > 0) e1 = S[ncols];
  if (top > 1) e2 = S[2 * (int64_t)ncols];
  int32_t next = top > 0 ? (int32_t)(e1.y >> 16) : n;  // the start of entry k + 1
  k = 0;
  for (int32_t t = 0; t < n; ++t) {
    while (t >= next) {
      ++k;
      e0 = e1;
      e1 = e2;
      next = k < top ? (int32_t)(e1.y >> 16) : n;
      if (k + 2 <= top) e2 = S[(int64_t)(k + 2) * ncols];
    }
    // (t - v)^2 + f(v) with f(v) = g_v - v^2 (exact modulo 2^32)
    const uint32_t cv = e0.y & 0xffffu, dt = (uint32_t)t - cv;
    col[(int64_t)t * stride] = dt * dt + (e0.x - cv * cv);
  }
}

__device__ inline bool df_finite3(const float v[3]) {
  return __builtin_isfinite(v[0]) & __builtin_isfinite(v[1]) & __builtin_isfinite(v[2]);
}

// One lane per segment a -> b: the ray origins = a, point = b of dmf_fuse_points, every cell it
// updates (the misses and the end cell alike); kDfInf when it has none.
constexpr int kDfClearThreads = 256;
__global__ __launch_bounds__(kDfClearThreads) void k_df_clear(Geom g, const uint32_t* __restrict__ dist2,
                                                              const float* __restrict__ a,
                                                              const float* __restrict__ b, int64_t n,
                                                              uint32_t* __restrict__ clear2) {
  const int64_t i = (int64_t)blockIdx.x * kDfClearThreads + threadIdx.x;
  if (i >= n) return;
  const float O[3] = {a[3 * i], a[3 * i + 1], a[3 * i + 2]};
  const float E[3] = {b[3 * i], b[3 * i + 1], b[3 * i + 2]};
  uint32_t best = kDfInf;
  Ray R = {};
  if (df_finite3(O) && df_finite3(E) && !dda_setup(g, O, E, endpoint_inside(g, E), R)) R.left = 0;
  for (Walk W(R); W.left > 0; W.step()) {
    const uint32_t d = dist2[((int64_t)W.c0 * g.n[1] + W.c1) * g.n[2] + W.c2];
    best = d < best ? d : best;
    if (--W.left == 0) break;
  }
  clear2[i] = best;
}

// The plain arguments first (no access to the volume: they are rejected without a device).
static int check_distance_args(const dmf_volume* v, const void* logodds, const void* dist2) {
  if (!v || !logodds || !dist2) return fail(DMF_ERR_INVALID, "null argument");
  return DMF_OK;
}
static int check_clearance_args(const dmf_volume* v, const void* dist2, const void* a, const void* b, int64_t n,
                                const void* clear2) {
  if (!v || !dist2 || !a || !b || !clear2) return fail(DMF_ERR_INVALID, "null argument");
  if (n < 0) return fail(DMF_ERR_INVALID, "negative segment count %lld", (long long)n);
  return DMF_OK;
}
static const char kDfGridLimit[] = "the distance field is limited to 2048 cells per axis";

static int distance_device(dmf_volume* v, const int16_t* d_logodds, int32_t threshold, uint32_t* d_dist2,
                           uint64_t* d_count) {
  const Geom g = v->geom();
  const int nx = g.n[0], ny = g.n[1], nz = g.n[2];
  const int64_t nrows = (int64_t)nx * ny, ncell = nrows * nz;
  void* stk = nullptr;
  if (nx > 1 || ny > 1) DMF_TRY(scratch(v, kScDfStack, sizeof(uint2) * (size_t)ncell, &stk));
  if (d_count) DMF_HIP(hipMemsetAsync(d_count, 0, sizeof(uint64_t), v->stream));
  const int rows_per_wg = kDfZCells / nz > 1 ? kDfZCells / nz : 1;
  hipLaunchKernelGGL(k_df_z, dim3((unsigned)((nrows + rows_per_wg - 1) / rows_per_wg)), dim3(kDfZThreads), 0, v->stream,
                     ncell, nz, rows_per_wg, nrows, d_logodds, threshold, d_dist2, (unsigned long long*)d_count);
  DMF_LAUNCH_CHECK();
  if (ny > 1) {
    const uint32_t ncols = (uint32_t)nx * (uint32_t)nz;
    hipLaunchKernelGGL(k_df_axis, dim3((ncols + kDfAxisThreads - 1) / kDfAxisThreads), dim3(kDfAxisThreads), 0,
                       v->stream, ny, (int64_t)nz, (uint32_t)nz, (int64_t)ny * nz, ncols, d_dist2, (uint2*)stk);
    DMF_LAUNCH_CHECK();
  }
  if (nx > 1) {
    const uint32_t ncols = (uint32_t)ny * (uint32_t)nz;
    hipLaunchKernelGGL(k_df_axis, dim3((ncols + kDfAxisThreads - 1) / kDfAxisThreads), dim3(kDfAxisThreads), 0,
                       v->stream, nx, (int64_t)ny * nz, ncols, (int64_t)0, ncols, d_dist2, (uint2*)stk);
    DMF_LAUNCH_CHECK();
  }
  return DMF_OK;
}

static int clearance_device(dmf_volume* v, const uint32_t* d_dist2, const float* d_a, const float* d_b, int64_t n,
                            uint32_t* d_clear2) {
  hipLaunchKernelGGL(k_df_clear, dim3((unsigned)((n + kDfClearThreads - 1) / kDfClearThreads)), dim3(kDfClearThreads),
                     0, v->stream, v->geom(), d_dist2, d_a, d_b, n, d_clear2);
  DMF_LAUNCH_CHECK();
  return DMF_OK;
}

}  // namespace dmf

using namespace dmf;

extern "C" {

int dmf_grid_distance_device(dmf_volume* v, const int16_t* d_logodds, int32_t threshold, uint32_t* d_dist2,
                             uint64_t* d_count) {
  DMF_API_BEGIN
  DMF_TRY(check_distance_args(v, d_logodds, d_dist2));
  DMF_TRY(require_grid_2048(v, kDfGridLimit));
  return distance_device(v, d_logodds, threshold, d_dist2, d_count);
  DMF_API_END
}

int dmf_grid_distance(dmf_volume* v, const int16_t* logodds, int32_t threshold, uint32_t* dist2, int64_t* n_solid) {
  DMF_API_BEGIN
  DMF_TRY(check_distance_args(v, logodds, dist2));
  DMF_TRY(require_grid_2048(v, kDfGridLimit));
  void *dl, *dd, *dc;
  uint64_t cnt = 0;
  DMF_TRY(upload_grid(v, logodds, &dl));
  DMF_TRY(scratch(v, kScDfDist, sizeof(uint32_t) * v->ncell, &dd));
  DMF_TRY(scratch(v, kScOut3, sizeof(uint64_t), &dc));
  DMF_TRY(distance_device(v, (const int16_t*)dl, threshold, (uint32_t*)dd, (uint64_t*)dc));
  DMF_HIP(hipMemcpyAsync(dist2, dd, sizeof(uint32_t) * v->ncell, hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipMemcpyAsync(&cnt, dc, sizeof(uint64_t), hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipStreamSynchronize(v->stream));
  if (n_solid) *n_solid = (int64_t)cnt;
  return DMF_OK;
  DMF_API_END
}

int dmf_grid_clearance_device(dmf_volume* v, const uint32_t* d_dist2, const float* d_a, const float* d_b, int64_t n,
                              uint32_t* d_clear2) {
  DMF_API_BEGIN
  DMF_TRY(check_clearance_args(v, d_dist2, d_a, d_b, n, d_clear2));
  if (n == 0) return DMF_OK;
  DMF_TRY(require_grid_2048(v, kDfGridLimit));
  return clearance_device(v, d_dist2, d_a, d_b, n, d_clear2);
  DMF_API_END
}

int dmf_grid_clearance(dmf_volume* v, const uint32_t* dist2, const float* a, const float* b, int64_t n,
                       uint32_t* clear2) {
  DMF_API_BEGIN
  DMF_TRY(check_clearance_args(v, dist2, a, b, n, clear2));
  if (n == 0) return DMF_OK;
  DMF_TRY(require_grid_2048(v, kDfGridLimit));
  void *dd, *da, *db, *dc;
  const size_t nb = sizeof(float) * 3 * (size_t)n;
  DMF_TRY(scratch(v, kScDfDist, sizeof(uint32_t) * v->ncell, &dd));
  DMF_TRY(scratch(v, kScHost1, nb, &da));
  DMF_TRY(scratch(v, kScHost2, nb, &db));
  DMF_TRY(scratch(v, kScOut0, sizeof(uint32_t) * (size_t)n, &dc));
  DMF_HIP(hipMemcpyAsync(dd, dist2, sizeof(uint32_t) * v->ncell, hipMemcpyHostToDevice, v->stream));
  DMF_HIP(hipMemcpyAsync(da, a, nb, hipMemcpyHostToDevice, v->stream));
  DMF_HIP(hipMemcpyAsync(db, b, nb, hipMemcpyHostToDevice, v->stream));
  DMF_TRY(clearance_device(v, (const uint32_t*)dd, (const float*)da, (const float*)db, n, (uint32_t*)dc));
  DMF_HIP(hipMemcpyAsync(clear2, dc, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipStreamSynchronize(v->stream));
  return DMF_OK;
  DMF_API_END
}

}  // extern "C"
