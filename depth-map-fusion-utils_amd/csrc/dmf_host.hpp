// dmf_host.hpp — host-side plumbing shared by the C-ABI translation units:
// status/error reporting, HIP error checks, the per-volume scratch arena and the
// pose-table upload.  No compute lives here.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <new>

#include "dmf_internal.hpp"

namespace dmf {

void set_error(const char* fmt, ...);
int fail(int status, const char* fmt, ...);

#define DMF_HIP(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return ::dmf::fail(DMF_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                         __FILE__, __LINE__);                                           \
  } while (0)

#define DMF_TRY(expr)            \
  do {                           \
    int s_ = (expr);             \
    if (s_ != DMF_OK) return s_; \
  } while (0)

#define DMF_LAUNCH_CHECK() DMF_HIP(hipGetLastError())

// Guard every C entry point: no C++ exception crosses the ABI.
#define DMF_API_BEGIN try {
#define DMF_API_END                                                        \
  }                                                                        \
  catch (const std::bad_alloc&) {                                          \
    return ::dmf::fail(DMF_ERR_NOMEM, "host allocation failed");           \
  }                                                                        \
  catch (...) {                                                            \
    return ::dmf::fail(DMF_ERR_INVALID, "unexpected C++ exception");       \
  }

// Make v's device current (HIP device state is per host thread).
int activate(const dmf_volume* v);
inline dmf_volume* v_mut(const dmf_volume* v) { return const_cast<dmf_volume*>(v); }
int require_constructed(const dmf_volume* v);
// ... and at most 2048 cells per axis (the fixed-point DDA's limit), else DMF_ERR_RANGE with `text`
int require_grid_2048(const dmf_volume* v, const char* text);

// Scratch arena: slot k is a device buffer grown on demand, reused across calls.
int scratch(dmf_volume* v, int k, size_t bytes, void** out);
// The fused grid's consumers, host forms: the caller's int16 grid into slot kScOut2 (on the stream).
int upload_grid(dmf_volume* v, const int16_t* logodds, void** d_grid);
// The brick pipeline's buffers (dmf_fuse.hip bk_buf_bytes states each one's size): every buffer
// exists once per staging slot of pipelined fusion; serial calls use slot 0.
enum BkBuf {
  kBufRays,                   // ray records, then the crossing paths
  kBufPairsA, kBufPairsB,     // pair records: the 16-byte half; the slab word (4 bytes) or the cell walk's uint2 (8)
  kBufBricks, kBufCtl,        // brick counts | offsets | part prefix | part order; phase F's queue control words
  kBufWgBase, kBufWgList,     // per-workgroup brick bases and touched-brick lists
  kBufPoseCnt, kBufPoseBase,  // per-pose brick counts and bases
  kBufBatch, kBufOvl,         // pose pair counts, then the batch table; pass A's hashed-histogram overflow list
  kBufStPoses, kBufStStats,   // requested on demand: a staged depth call's pose table, a staged call's pass-A statistics
  kBkBufCount, kBkPipeBufs = kBufStPoses  // [0, kBkPipeBufs): what every call uses (bk_scratch)
};
enum ScratchSlot {
  kScPoses = 0, kScHost0, kScHost1, kScHost2, kScOut0, kScOut1, kScOut2, kScOut3, kScTmp, kScSort0,
  kScSort1, kScSort2, kScSort3, kScCount, kScStats,
  kScOgP0, kScOgP1, kScOgFinal, kScOgOcc,  // OccupancyGrid reorganization (dmf_ogrid.hip)
  kScRevItems,  // reverseRayTraceFast's item-ordered (spatial order) result masks (dmf_trace.hip)
  kScRcFine, kScRcCoarse,  // the log-odds ray-cast's solid mask and its tile + brick levels (dmf_raycast.hip)
  // surface extraction (dmf_surface.hip): the solid, free and surface masks, the per-row counts
  // and their scan, the {surface, solid} counters, and the host forms' output staging
  kScSfSolid, kScSfFree, kScSfSurf, kScSfCounts, kScSfBases, kScSfTotals, kScSfHash, kScSfXyz, kScSfNrm,
  // the distance field (dmf_distance.hip): the y / x passes' envelope stacks, and the host forms' field
  kScDfStack, kScDfDist,
  // view gain (dmf_viewgain.hip): the solid and unknown masks, their tile + brick levels, and the
  // masks and gains of the calls that keep them in scratch
  kScVgSolid, kScVgUnknown, kScVgCoarse, kScVgSeen, kScVgGain,
  // the travel field (dmf_travel.hip): the traversable mask and its tile level, the two active-tile
  // lists with their "queued" bits, the counters and list lengths, and the host forms' field
  kScTrFine, kScTrCoarse, kScTrQueue, kScTrCtl, kScTrHops,
  // cloud nearest neighbour (dmf_cloud.hip): the control block, the cells' counts and offsets, the
  // cell-sorted records, the sorted variant's keys, and the host form's staging of both clouds,
  // both per-point outputs and the summaries
  kScClCtl, kScClCells, kScClRec, kScClKeys, kScClQuery, kScClRef, kScClDist, kScClIndex, kScClSums,
  // the tour (dmf_tour.hip): the control block, the four prefix arrays with the permutation check's
  // bits, and the host forms' map, path and info
  kScToCtl, kScToPre, kScToMap, kScToPath, kScToInfo,
  // candidate views (dmf_views.hip): the control block, the leaf keys with the point indices, the
  // segment-head flags with their scan, the leaves' first sorted positions, and the host forms'
  // staging of the cloud, the leaves, the poses and the counts (the chain's surface cloud lives in
  // kScSfXyz / kScSfNrm, its locations in kScVwOutXyz / kScVwOutNrm when the caller takes none)
  kScVwCtl, kScVwKeys, kScVwFlags, kScVwStart, kScVwInXyz, kScVwInNrm, kScVwOutXyz, kScVwOutNrm, kScVwOutPts,
  kScVwPoses, kScVwCount,
  // brick-owned fusion (dmf_fuse.hip): one block, buffer b of staging slot s at bk_key(b, s)
  kScBkFirst, kScBkEnd = kScBkFirst + 2 * kBkBufCount
};
inline int bk_key(int buf, int slot) { return kScBkFirst + slot * kBkBufCount + buf; }

// Striped statistics: kernels add into slot (block % kStatSlots) of a zeroed buffer
// of kStatSlots x kStatWidth counters (one hot address per counter serialises at the
// memory side); stats_end() sums the slots into the caller's counters.
// DMF_EXP_STATS is the one diagnostic build the sources keep: an instrument (extra counters
// 7..19 and s_memtime phase timers, read by bench.py and tools/exp_*.py; DESIGN.md §5.5-5.8
// rest on them), not an alternative implementation -- those live in the history.
#if defined(DMF_EXP_STATS)
constexpr int kStatSlots = 256, kStatWidth = 20;
#else
constexpr int kStatSlots = 256, kStatWidth = 8;
#endif
int stats_begin(dmf_volume* v, unsigned long long** striped);
// (on `stream`, the volume's stream by default; the sums are atomic: a pipelined call's
// pass-A statistics are summed on the staging stream while the previous call's are on the
// volume's)
int stats_end(dmf_volume* v, const unsigned long long* striped, uint64_t* d_user, int ncounters,
              uint32_t* fault = nullptr, hipStream_t stream = nullptr);
__device__ inline unsigned long long* stat_slot(unsigned long long* base) {
  return base ? base + kStatWidth * ((blockIdx.x + blockIdx.y * gridDim.x) & (kStatSlots - 1)) : nullptr;
}

// Upload P host poses (or take device poses) and build the PoseX table on device.
int pose_table(dmf_volume* v, const float* poses, int P, bool poses_on_device, PoseX** d_table);
// The same table from P device poses into d_out, on stream s (the staging stream of a
// pipelined fusion call).
int pose_table_into(const float* d_poses, int P, PoseX* d_out, hipStream_t s);

CamP cam_params(const dmf_camera* c);

// Fusion finalize over tiled counters, tiles [t0, t1) (dmf_fuse.hip); the tiled layout's
// x extent in 2-cell tile rows and tiles per row (a contiguous tile range of whole rows is
// an x slab of the grid).  finalize_tiles rejects clamp bounds outside int16 or inverted
// (check_finalize_params: DMF_ERR_INVALID, nothing launched); the merge calls the check
// itself before its collectives, which change the counters.
int check_finalize_params(const dmf_fuse_params* prm);
int finalize_tiles(dmf_volume* v, const int32_t* d_hits, const int32_t* d_misses, const dmf_fuse_params* prm,
                   int16_t* d_out, int64_t t0, int64_t t1, hipStream_t stream);
int tile_rows(const dmf_volume* v, int64_t* ntx, int64_t* tiles_per_row);
int check_camera(const dmf_camera* c);
// What every fusion call checks of the volume, the camera and the pose count P (dmf_fuse.hip
// check_fuse; the ray-cast of dmf_raycast.hip walks the same rays under the same limits).
int check_fuse_call(const dmf_volume* v, const dmf_camera* cam, int P);

// Lazily (re)build the float-accumulated enumeration list (reverseRayTrace / rayTraceVolume).
int ensure_enumeration(dmf_volume* v);
int ensure_brick_dist(dmf_volume* v);

// Device-wide helpers implemented with rocPRIM in dmf_core.hip.
int exclusive_scan_i64(dmf_volume* v, const int64_t* in, int64_t* out, size_t n);
int exclusive_scan_i32(dmf_volume* v, const int32_t* in, int32_t* out, size_t n);
int sort_pairs_u64(dmf_volume* v, uint64_t* keys, uint64_t* vals, size_t n, int end_bit);
int sort_pairs_u32(dmf_volume* v, uint32_t* keys, uint32_t* vals, size_t n, int end_bit);

// Order-preserving compaction of per-pose bitmasks (P x words) into concatenated
// lists: element e of pose p with bit set -> out[base[p] + rank] = value(e).
// value source: hash[e] (slot lists) or a callback kernel (enumeration lists).
int compact_masks(dmf_volume* v, const uint64_t* d_masks, int P, int64_t words, int64_t nelem,
                  int64_t* counts_h, uint64_t** d_out_lists, int64_t* total, int value_kind);
enum { kValueSlotHash = 0, kValueEnumCentroidHash = 1 };

// greedySetCover (Algorithms.hpp:38-86) over P device bitmasks of `words` uint64 (dmf_cover.hip);
// the selection order comes back on the host.  Scratch: kScTmp and kScCount.
int greedy_cover(dmf_volume* v, const uint64_t* d_masks, int P, int64_t words, int min_gain, int32_t* selected,
                 int32_t* nselected);
// Surface extraction in two steps (dmf_surface.hip), for callers that size a buffer by the count:
// surface_count leaves the masks, the row counts and their scan in the volume's scratch and writes
// d_count[2] = {surface cells, solid cells}; surface_emit, after it on the same grid, writes the
// first min(count, cap) entries of the given outputs; surface_count_host uploads a host grid, counts
// and reads the counts back (synchronises).
int surface_count(dmf_volume* v, const int16_t* d_logodds, int32_t occ, int32_t free_thr, uint64_t* d_count);
int surface_emit(dmf_volume* v, const int16_t* d_logodds, uint64_t* d_hash, float* d_xyz, float* d_nrm, int64_t cap);
int surface_count_host(dmf_volume* v, const int16_t* logodds, int32_t occ, int32_t free_thr, void** d_grid,
                       uint64_t cnt[2]);
// The log-odds ray-cast's argument checks (dmf_raycast.hip): the plain arguments without access to
// the volume, then check_fuse_call.
int check_raycast(const dmf_volume* v, const dmf_camera* cam, const void* logodds, const void* poses, int32_t P,
                  int32_t range_mm);

}  // namespace dmf
