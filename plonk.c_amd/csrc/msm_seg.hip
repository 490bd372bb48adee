// Segmented MSM (include/plonkhip.h, "Segmented MSM"): any list of consecutive segments of one flat point and
// scalar array, uniform (length m) or ragged (a device array of offsets), one word {x, y, infinite, status}
// per segment.
//
// For canonical inputs a segment's result is EXP[(sum s_i LOG_i) mod 102] (msm.hip's isomorphism E(F101) =
// Z/102; g1_mul takes the raw scalar byte and the group has order 102, so this holds for any s_i < 256).  A
// segment is therefore an integer sum over 4 bytes per point, and the call a segmented integer reduction.
// LOG is the conflict-free lookup of plk_g1log.h (stage_table, dlog, g1_word; shared with kzg_agg.hip): d = E[y] - k
// through an LDS table of 128 entries in 32 copies, d < 102 the log exactly when the encoding is canonical,
// d >= 256 otherwise; the 102 meaningful words of E reach the kernels as an argument.
//
// Two paths, a function of (total, m, nseg, ragged) alone (plk_msm_g1_segments_plan):
//   lane    uniform m <= 32: one lane per segment sums its m terms, looks EXP up and stores; one launch, no
//           workspace.  m a multiple of 16 and aligned arrays: 16-byte loads.
//   prefix  everything else.  It cuts the POINT range, not the segment list, so any mix of lengths is balanced:
//           1  every thread takes a chunk of 16 points, every block a tile of 256 chunks: the chunk's sum of
//              s LOG (mod 102) and its count of non-canonical points are scanned inside the tile; one word per
//              chunk (exclusive sum | exclusive count << 8, both within the tile) and two words per tile (sum
//              mod 102, count) are stored
//           2  one block turns the tile totals into exclusive tile prefixes in place (sum mod 102, the count
//              in a full 32-bit word: total < 2^32 keeps every difference exact)
//           3  one lane per segment: at most 32 points are summed from their bytes; a longer segment is
//              P(o_{g+1}) - P(o_g) with P(i) = tile prefix + chunk prefix + the up to 15 terms in front of i
//              inside its chunk, the count of bad points formed the same way; EXP, one 4-byte store
// Plain stores and launch boundaries only: no atomics, nothing to initialise, every word read was written by
// the same call, and every quantity is an integer, so the bytes do not depend on any order.
//
// A term of a non-canonical point is s (d & 0xFF): meaningless, but the same number in pass 1 and pass 3, so a
// bad point in front of a segment inside its first chunk cancels exactly in P(hi) - P(lo); the count decides.
#include <string.h>

#include <algorithm>
#include <vector>

#include "plk_device.h"
#include "plk_g1log.h"
#include "plk_hostcall.h"
#include "plk_internal.h"

namespace {

using plkg1log::TAB_C;
using plkg1log::TAB_E;
using plkg1log::dlog;
using plkg1log::g1_word;

constexpr uint32_t ORD = PLK_GROUP_ORDER;
constexpr int SEG_T = 256;                       // threads per block
constexpr int SEG_WAVES = SEG_T / PLK_WAVE;
constexpr uint32_t CHUNK = 16;                   // points per thread of pass 1
constexpr uint32_t TILE = SEG_T * CHUNK;         // points per block of pass 1
constexpr uint64_t LANE_MAX = 32;                // uniform m <= : the lane path
constexpr uint32_t DIRECT_MAX = 32;              // pass 3 sums a segment of at most this many points from its bytes
constexpr uint32_t LANE_BLOCKS = 2048;           // grid cap of the lane kernels (grid-stride loops)
constexpr uint64_t MAX_TOTAL = 1ull << 32, MAX_NSEG = 1ull << 30;

constexpr uint32_t ST_IRREGULAR = (uint32_t)PLK_MSM_SEG_IRREGULAR << 24 | 0xFFFFFFu;   // bytes FF FF FF 01
constexpr uint32_t ST_BAD = (uint32_t)PLK_MSM_SEG_BAD << 24 | 0xFFFFFFu;               // bytes FF FF FF 02

enum { PATH_LANE = 0, PATH_PREFIX = 1 };

// one point's term is at most 255 x 255 (a non-canonical point's d & 0xFF can be anything below 256)
constexpr uint32_t TERM_MAX = 255u * 255u;
static_assert((uint64_t)TERM_MAX * (CHUNK + DIRECT_MAX) + 4 * ORD < (1ull << 32), "a chunk's and a short segment's sums fit 32 bits");
static_assert((uint64_t)SEG_T * (ORD - 1) < (1u << 16) && TILE < (1u << 16), "a tile's scan packs (sum, count) into 16 + 16 bits");

struct SegTab { uint32_t w[ORD]; };              // E[y], y < 101, then E[256]

// one point's term and bad bit: sum += s (d & 0xFF) (<= TERM_MAX), bad += (d >= 256)
__device__ __forceinline__ void term(uint32_t k, uint32_t s, const uint32_t* tab, uint32_t lane4, uint32_t& sum, uint32_t& bad) {
  const uint32_t d = dlog(k, tab, lane4);
  sum += s * (d & 0xFFu);
  bad += d >= 256u ? 1u : 0u;
}

template <int J>
__device__ __forceinline__ void unit_term(const uint32_t (&w)[12], const uint32_t (&s)[4], const uint32_t* tab, uint32_t lane4,
                                          uint32_t& sum, uint32_t& bad) {
  term(g1_word<J>(w), (s[J >> 2] >> (8 * (J & 3))) & 0xFFu, tab, lane4, sum, bad);
}

// points [i0, i0 + cnt) byte-wise: sum grows by at most cnt TERM_MAX, bad by at most cnt
__device__ __forceinline__ void bytes_sum(const uint8_t* __restrict__ pts, const uint8_t* __restrict__ sc, uint64_t i0, uint32_t cnt,
                                          const uint32_t* tab, uint32_t lane4, uint32_t& sum, uint32_t& bad) {
  for (uint32_t j = 0; j < cnt; j++) {
    const uint64_t i = i0 + j;
    const uint32_t x = pts[3 * i], y = pts[3 * i + 1], f = pts[3 * i + 2];
    term(x << 8 | y << 16 | f << 24, sc[i], tab, lane4, sum, bad);
  }
}

// the 16 points from i0 (3 i0 and i0 16-byte aligned offsets of 16-byte aligned arrays) through four 16-byte loads
__device__ __forceinline__ void vec16_sum(const uint8_t* __restrict__ pts, const uint8_t* __restrict__ sc, uint64_t i0,
                                          const uint32_t* tab, uint32_t lane4, uint32_t& sum, uint32_t& bad) {
  const uint4* p4 = reinterpret_cast<const uint4*>(pts + 3 * i0);
  const uint4 a = p4[0], b = p4[1], c = p4[2], sv = *reinterpret_cast<const uint4*>(sc + i0);
  const uint32_t w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
  const uint32_t s[4] = {sv.x, sv.y, sv.z, sv.w};
  unit_term<0>(w, s, tab, lane4, sum, bad);   unit_term<1>(w, s, tab, lane4, sum, bad);
  unit_term<2>(w, s, tab, lane4, sum, bad);   unit_term<3>(w, s, tab, lane4, sum, bad);
  unit_term<4>(w, s, tab, lane4, sum, bad);   unit_term<5>(w, s, tab, lane4, sum, bad);
  unit_term<6>(w, s, tab, lane4, sum, bad);   unit_term<7>(w, s, tab, lane4, sum, bad);
  unit_term<8>(w, s, tab, lane4, sum, bad);   unit_term<9>(w, s, tab, lane4, sum, bad);
  unit_term<10>(w, s, tab, lane4, sum, bad);  unit_term<11>(w, s, tab, lane4, sum, bad);
  unit_term<12>(w, s, tab, lane4, sum, bad);  unit_term<13>(w, s, tab, lane4, sum, bad);
  unit_term<14>(w, s, tab, lane4, sum, bad);  unit_term<15>(w, s, tab, lane4, sum, bad);
}

// the segment's word: {x, y, infinite, 0} of EXP[sum mod 102], or FF FF FF and the status
__device__ __forceinline__ void store_word(uint8_t* __restrict__ out4, uint64_t g, uint32_t v, bool aligned) {
  uint8_t* o = out4 + 4 * g;
  if (aligned) {
    *reinterpret_cast<uint32_t*>(o) = v;
  } else {
    o[0] = (uint8_t)v;
    o[1] = (uint8_t)(v >> 8);
    o[2] = (uint8_t)(v >> 16);
    o[3] = (uint8_t)(v >> 24);
  }
}

// lane path: segment g = points [g m, (g + 1) m) in one lane, m <= LANE_MAX.  VEC (m a multiple of 16, both
// arrays 16-byte aligned): every segment is as aligned as the arrays and the lane takes 16-byte loads.
template <bool VEC>
__global__ __launch_bounds__(SEG_T) void seg_lane_kernel(SegTab t, const uint8_t* __restrict__ pts, const uint8_t* __restrict__ sc,
                                                        uint32_t m, uint64_t nseg, const uint32_t* __restrict__ expw,
                                                        uint8_t* __restrict__ out4, bool out_aligned) {
  __shared__ __attribute__((aligned(16))) uint32_t tab[TAB_E * TAB_C];
  plkg1log::stage_table<SEG_T>(t, tab);
  __syncthreads();
  const uint32_t lane4 = (threadIdx.x & (TAB_C - 1u)) << 2;
  for (uint64_t g = (uint64_t)blockIdx.x * SEG_T + threadIdx.x; g < nseg; g += (uint64_t)gridDim.x * SEG_T) {
    uint32_t sum = 0, bad = 0;   // sum <= 32 TERM_MAX
    if (VEC) {
      for (uint32_t j = 0; j < m; j += CHUNK) vec16_sum(pts, sc, g * m + j, tab, lane4, sum, bad);
    } else {
      bytes_sum(pts, sc, g * m, m, tab, lane4, sum, bad);
    }
    store_word(out4, g, bad ? ST_IRREGULAR : expw[sum % ORD], out_aligned);
  }
}

// Pass 1.  Chunk c = blockIdx.x SEG_T + threadIdx.x holds points [16 c, 16 c + 16) below total; there are
// nrec = total / 16 + 1 chunk records, so that P(total) has a record too (its chunk may be empty).  VEC: both
// arrays 16-byte aligned (a chunk cut by total still goes byte-wise).
//   rec[c]      = exclusive sum inside the tile mod 102 | exclusive bad count inside the tile (<= 4096) << 8
//   tile[2 b..] = {the tile's sum mod 102, the tile's bad count}
template <bool VEC>
__global__ __launch_bounds__(SEG_T) void seg_scan_kernel(SegTab t, const uint8_t* __restrict__ pts, const uint8_t* __restrict__ sc,
                                                        uint64_t total, uint64_t nrec, uint32_t* __restrict__ tile,
                                                        uint32_t* __restrict__ rec) {
  __shared__ __attribute__((aligned(16))) uint32_t tab[TAB_E * TAB_C];
  __shared__ uint32_t wtot[SEG_WAVES];
  plkg1log::stage_table<SEG_T>(t, tab);
  __syncthreads();
  const uint32_t lane4 = (threadIdx.x & (TAB_C - 1u)) << 2;
  const uint32_t wave = threadIdx.x / PLK_WAVE, lane = threadIdx.x & (PLK_WAVE - 1);
  const uint64_t c = (uint64_t)blockIdx.x * SEG_T + threadIdx.x, i0 = c * CHUNK;
  uint32_t sum = 0, bad = 0;   // sum <= 16 TERM_MAX, bad <= 16
  if (i0 < total) {
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(CHUNK, total - i0);
    if (VEC && cnt == CHUNK) vec16_sum(pts, sc, i0, tab, lane4, sum, bad);
    else bytes_sum(pts, sc, i0, cnt, tab, lane4, sum, bad);
  }
  // inclusive scan of (sum mod 102, bad) packed 16 + 16: <= 256 x 101 and <= 4096 over the tile
  const uint32_t own = (sum % ORD) | bad << 16;
  uint32_t v = own;
#pragma unroll
  for (int off = 1; off < PLK_WAVE; off <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)v, off, PLK_WAVE);
    if (lane >= (uint32_t)off) v += u;
  }
  if (lane == PLK_WAVE - 1) wtot[wave] = v;
  __syncthreads();
  uint32_t base = 0, all = 0;
#pragma unroll
  for (int k = 0; k < SEG_WAVES; k++) {
    if ((uint32_t)k < wave) base += wtot[k];
    all += wtot[k];
  }
  const uint32_t ex = base + v - own;
  if (c < nrec) rec[c] = ((ex & 0xFFFFu) % ORD) | (ex >> 16) << 8;
  if (threadIdx.x == 0) {
    tile[2 * (uint64_t)blockIdx.x] = (all & 0xFFFFu) % ORD;
    tile[2 * (uint64_t)blockIdx.x + 1] = all >> 16;
  }
}

// Pass 2: the tile totals become exclusive tile prefixes in place, one block.  Thread t owns tiles
// [t per, (t + 1) per): it sums them, the block scans the 256 thread sums, the thread rewrites its tiles.
// Sums stay reduced mod 102 (a thread's run sum < 102 after each step, the scan's <= 256 x 101); the bad
// counts are plain 32-bit sums, at most total < 2^32.
__global__ __launch_bounds__(SEG_T) void seg_tiles_kernel(uint32_t* __restrict__ tile, uint64_t ntiles) {
  __shared__ uint32_t ssum[SEG_T], sbad[SEG_T];
  const uint64_t per = (ntiles + SEG_T - 1) / SEG_T;
  const uint64_t lo = std::min<uint64_t>((uint64_t)threadIdx.x * per, ntiles), hi = std::min<uint64_t>(lo + per, ntiles);
  uint32_t s = 0, b = 0;
  for (uint64_t i = lo; i < hi; i++) {
    s = (s + tile[2 * i]) % ORD;
    b += tile[2 * i + 1];
  }
  ssum[threadIdx.x] = s;
  sbad[threadIdx.x] = b;
  __syncthreads();
  uint32_t ps = 0, pb = 0;
  for (uint32_t k = 0; k < threadIdx.x; k++) {   // <= 255 x 101
    ps += ssum[k];
    pb += sbad[k];
  }
  ps %= ORD;
  for (uint64_t i = lo; i < hi; i++) {
    const uint32_t ts = tile[2 * i], tb = tile[2 * i + 1];
    tile[2 * i] = ps;
    tile[2 * i + 1] = pb;
    ps = (ps + ts) % ORD;
    pb += tb;
  }
}

// P(i), i <= total: sum (mod 102 up to the caller: < 2 x 102 + 15 TERM_MAX) and bad count of points [0, i)
__device__ __forceinline__ void prefix_at(const uint8_t* __restrict__ pts, const uint8_t* __restrict__ sc, uint64_t i,
                                          const uint32_t* __restrict__ tile, const uint32_t* __restrict__ rec, const uint32_t* tab,
                                          uint32_t lane4, uint32_t& sum, uint32_t& bad) {
  const uint64_t c = i / CHUNK, b = i / TILE;
  const uint32_t r = rec[c];
  sum = tile[2 * b] + (r & 0xFFu);
  bad = tile[2 * b + 1] + (r >> 8);
  bytes_sum(pts, sc, c * CHUNK, (uint32_t)(i % CHUNK), tab, lane4, sum, bad);
}

// Pass 3: one lane per segment.  off == nullptr: o_g = g m.  Otherwise the offsets are read as min(o, total),
// so no value makes a lane read outside [0, total) of the arrays; a falling pair or an offset above total is
// PLK_MSM_SEG_BAD.
__global__ __launch_bounds__(SEG_T) void seg_finish_kernel(SegTab t, const uint8_t* __restrict__ pts, const uint8_t* __restrict__ sc,
                                                          uint64_t total, const uint32_t* __restrict__ off, uint64_t m,
                                                          uint64_t nseg, const uint32_t* __restrict__ tile,
                                                          const uint32_t* __restrict__ rec, const uint32_t* __restrict__ expw,
                                                          uint8_t* __restrict__ out4, bool out_aligned) {
  __shared__ __attribute__((aligned(16))) uint32_t tab[TAB_E * TAB_C];
  plkg1log::stage_table<SEG_T>(t, tab);
  __syncthreads();
  const uint32_t lane4 = (threadIdx.x & (TAB_C - 1u)) << 2;
  for (uint64_t g = (uint64_t)blockIdx.x * SEG_T + threadIdx.x; g < nseg; g += (uint64_t)gridDim.x * SEG_T) {
    uint64_t lo, hi;
    bool broken = false;
    if (off) {
      const uint64_t a = off[g], b = off[g + 1];
      broken = b < a || a > total || b > total;
      lo = std::min(a, total);
      hi = std::min(b, total);
    } else {
      lo = g * m;
      hi = lo + m;   // (m nseg == total: checked by the caller)
    }
    uint32_t v;
    if (broken) {
      v = ST_BAD;
    } else {
      uint32_t sum = 0, bad = 0;
      if (hi - lo <= DIRECT_MAX) {
        bytes_sum(pts, sc, lo, (uint32_t)(hi - lo), tab, lane4, sum, bad);   // <= 32 TERM_MAX
      } else {
        uint32_t s0, b0, s1, b1;
        prefix_at(pts, sc, lo, tile, rec, tab, lane4, s0, b0);
        prefix_at(pts, sc, hi, tile, rec, tab, lane4, s1, b1);
        sum = s1 % ORD + ORD - s0 % ORD;
        bad = b1 - b0;   // both exact counts below 2^32, b1 >= b0
      }
      v = bad ? ST_IRREGULAR : expw[sum % ORD];
    }
    store_word(out4, g, v, out_aligned);
  }
}

struct Plan {
  int path;
  uint64_t tile;       // points a block of the first launch covers
  int launches;
  uint64_t blocks;     // of the first launch
  uint64_t nrec, ntiles;
};

// arguments checked by the caller
Plan plan_of(uint64_t total, uint64_t m, uint64_t nseg, bool ragged) {
  Plan p{};
  if (!ragged && m <= LANE_MAX) {
    p.path = PATH_LANE;
    p.tile = SEG_T * m;
    p.launches = 1;
    p.blocks = std::min<uint64_t>((nseg + SEG_T - 1) / SEG_T, LANE_BLOCKS);
  } else {
    p.path = PATH_PREFIX;
    p.tile = TILE;
    p.launches = 3;
    p.nrec = total / CHUNK + 1;
    p.ntiles = (p.nrec + SEG_T - 1) / SEG_T;
    p.blocks = p.ntiles;
  }
  return p;
}

size_t workspace_of(const Plan& p) { return p.path == PATH_LANE ? 0 : (size_t)(8 * p.ntiles + 4 * p.nrec); }

// PLK_OK, or the code the launch returns for this shape
int check_shape(const char* fn, size_t total, size_t m, size_t nseg, bool ragged, bool quiet = false) {
  if (nseg == 0 || total == 0 || (!ragged && (m == 0 || total / m != nseg || total % m != 0))) {
    if (!quiet) plk_set_error("%s: nseg > 0 and total > 0 are required, and m > 0 with m nseg == total without offsets", fn);
    return PLK_ERR_ARG;
  }
  if ((uint64_t)total >= MAX_TOTAL || (uint64_t)nseg > MAX_NSEG) {
    if (!quiet) plk_set_error("%s: total = %zu must stay below 2^32 and nseg = %zu within 2^30", fn, total, nseg);
    return PLK_ERR_RANGE;
  }
  return PLK_OK;
}

struct HostStream {
  hipStream_t st = nullptr;
  ~HostStream() {
    if (st) (void)hipStreamDestroy(st);
  }
};

}  // namespace

extern "C" {

int plk_msm_g1_segments_plan(size_t total, size_t m, size_t nseg, int ragged, int64_t out[4]) {
  const char* fn = "plk_msm_g1_segments_plan";
  if (!out) {
    plk_set_error("%s: out is required", fn);
    return PLK_ERR_ARG;
  }
  const int rc = check_shape(fn, total, m, nseg, ragged != 0);
  if (rc) return rc;
  const Plan p = plan_of(total, m, nseg, ragged != 0);
  out[0] = p.path;
  out[1] = (int64_t)p.tile;
  out[2] = p.launches;
  out[3] = (int64_t)p.blocks;
  return PLK_OK;
}

size_t plk_msm_g1_segments_workspace(size_t total, size_t m, size_t nseg, int ragged) {
  if (check_shape("plk_msm_g1_segments_workspace", total, m, nseg, ragged != 0, true)) return 0;
  return workspace_of(plan_of(total, m, nseg, ragged != 0));
}

int plk_msm_g1_segments_dev(const uint8_t* d_points, const uint8_t* d_scalars, size_t total, const uint32_t* d_offsets, size_t m,
                            size_t nseg, uint8_t* d_out4, void* d_work, void* stream) {
  const char* fn = "plk_msm_g1_segments_dev";
  if (!d_points || !d_scalars || !d_out4) {
    plk_set_error("%s: d_points, d_scalars and d_out4 are required", fn);
    return PLK_ERR_ARG;
  }
  const bool ragged = d_offsets != nullptr;
  int rc = check_shape(fn, total, m, nseg, ragged);
  if (rc) return rc;
  if (ragged && (uintptr_t)d_offsets % 4) {
    plk_set_error("%s: d_offsets must be 4-byte aligned", fn);
    return PLK_ERR_ARG;
  }
  const Plan p = plan_of(total, m, nseg, ragged);
  if (p.launches > 1 && (!d_work || (uintptr_t)d_work % 4)) {
    plk_set_error("%s: d_work (plk_msm_g1_segments_workspace bytes, 4-byte aligned) is required for this shape", fn);
    return PLK_ERR_ARG;
  }
  if ((rc = plk_use_device())) return rc;
  SegTab t;
  plk_group_ytab_words(t.w);
  const uint32_t* expw = plk_msm_exp_words_dev();
  hipStream_t st = (hipStream_t)stream;
  const bool in_aligned = ((uintptr_t)d_points | (uintptr_t)d_scalars) % 16 == 0;
  const bool out_aligned = (uintptr_t)d_out4 % 4 == 0;
  if (p.path == PATH_LANE) {
    if (in_aligned && m % CHUNK == 0)
      hipLaunchKernelGGL(seg_lane_kernel<true>, dim3((uint32_t)p.blocks), dim3(SEG_T), 0, st, t, d_points, d_scalars, (uint32_t)m,
                         (uint64_t)nseg, expw, d_out4, out_aligned);
    else
      hipLaunchKernelGGL(seg_lane_kernel<false>, dim3((uint32_t)p.blocks), dim3(SEG_T), 0, st, t, d_points, d_scalars, (uint32_t)m,
                         (uint64_t)nseg, expw, d_out4, out_aligned);
    PLK_HIP(hipGetLastError());
    return PLK_OK;
  }
  uint32_t* tile = (uint32_t*)d_work;          // 2 ntiles words
  uint32_t* rec = tile + 2 * p.ntiles;         // nrec words
  if (in_aligned)
    hipLaunchKernelGGL(seg_scan_kernel<true>, dim3((uint32_t)p.ntiles), dim3(SEG_T), 0, st, t, d_points, d_scalars, (uint64_t)total,
                       p.nrec, tile, rec);
  else
    hipLaunchKernelGGL(seg_scan_kernel<false>, dim3((uint32_t)p.ntiles), dim3(SEG_T), 0, st, t, d_points, d_scalars, (uint64_t)total,
                       p.nrec, tile, rec);
  PLK_HIP(hipGetLastError());
  hipLaunchKernelGGL(seg_tiles_kernel, dim3(1), dim3(SEG_T), 0, st, tile, p.ntiles);
  PLK_HIP(hipGetLastError());
  hipLaunchKernelGGL(seg_finish_kernel, dim3((uint32_t)std::min<uint64_t>((nseg + SEG_T - 1) / SEG_T, LANE_BLOCKS)), dim3(SEG_T), 0,
                     st, t, d_points, d_scalars, (uint64_t)total, d_offsets, (uint64_t)m, (uint64_t)nseg, tile, rec, expw, d_out4,
                     out_aligned);
  PLK_HIP(hipGetLastError());
  return PLK_OK;
}

int plk_msm_g1_segments(const uint8_t* points, const uint8_t* scalars, size_t total, const uint32_t* offsets, size_t m, size_t nseg,
                        uint8_t* out3) {
  const char* fn = "plk_msm_g1_segments";
  if (!points || !scalars || !out3) {
    plk_set_error("%s: points, scalars and out3 are required", fn);
    return PLK_ERR_ARG;
  }
  const bool ragged = offsets != nullptr;
  int rc = check_shape(fn, total, m, nseg, ragged);
  if (rc) return rc;
  if (ragged) {
    for (size_t g = 0; g <= nseg; g++) {
      if (offsets[g] > total || (g && offsets[g] < offsets[g - 1])) {
        plk_set_error("%s: offsets[%zu] = %u falls or exceeds total = %zu", fn, g, offsets[g], total);
        return PLK_ERR_ARG;
      }
    }
  }
  if ((rc = plk_select_device())) return rc;
  constexpr size_t NREC = 64;   // raw folds in flight per read-back
  const size_t ws = plk_msm_g1_segments_workspace(total, m, nseg, ragged), ob = ragged ? 4 * (nseg + 1) : 0;
  PlkScratch D;   // every array on a 16-byte boundary: the kernels then take their 16-byte loads
  const size_t arrays = (plk_pad16(3 * total) + plk_pad16(total) + plk_pad16(ob) + plk_pad16(4 * nseg) + plk_pad16(ws) + 255) &
                        ~(size_t)255;   // the records behind them on a 256-byte boundary
  if ((rc = D.alloc(fn, arrays + NREC * sizeof(PlkMsmResult)))) return rc;
  uint8_t* dp = D.d;
  uint8_t* ds = dp + plk_pad16(3 * total);
  uint8_t* dof = ds + plk_pad16(total);
  uint8_t* dout = dof + plk_pad16(ob);
  uint8_t* dw = dout + plk_pad16(4 * nseg);
  PlkMsmResult* drec = (PlkMsmResult*)(D.d + arrays);
  PLK_HIP(hipMemcpy(dp, points, 3 * total, hipMemcpyHostToDevice));
  PLK_HIP(hipMemcpy(ds, scalars, total, hipMemcpyHostToDevice));
  if (ragged) PLK_HIP(hipMemcpy(dof, offsets, ob, hipMemcpyHostToDevice));
  if ((rc = plk_msm_g1_segments_dev(dp, ds, total, ragged ? (const uint32_t*)dof : nullptr, m, nseg, dout, ws ? dw : nullptr, nullptr)))
    return rc;
  std::vector<uint8_t> h(4 * nseg);
  PLK_HIP(hipMemcpy(h.data(), dout, 4 * nseg, hipMemcpyDeviceToHost));
  // irregular segments, exactly: the raw serial fold, NREC segments per read-back
  HostStream hs;
  std::vector<size_t> pend;
  std::vector<uint8_t> hr(32 * NREC);
  auto flush = [&]() -> int {
    if (pend.empty()) return PLK_OK;
    PLK_HIP(hipMemcpy2DAsync(hr.data(), 32, drec, sizeof(PlkMsmResult), 32, pend.size(), hipMemcpyDeviceToHost, hs.st));
    PLK_HIP(hipStreamSynchronize(hs.st));
    for (size_t k = 0; k < pend.size(); k++) memcpy(&h[4 * pend[k]], ((const PlkMsmResult*)(hr.data() + 32 * k))->g1, 3);
    pend.clear();
    return PLK_OK;
  };
  for (size_t g = 0; g < nseg; g++) {
    if (h[4 * g + 3] == 0) continue;
    if (h[4 * g + 3] != PLK_MSM_SEG_IRREGULAR) {
      plk_set_error("%s: segment %zu came back with status %u", fn, g, h[4 * g + 3]);
      return PLK_ERR_HIP;
    }
    if (!hs.st) PLK_HIP(hipStreamCreate(&hs.st));
    const size_t lo = ragged ? offsets[g] : g * m, hi = ragged ? offsets[g + 1] : lo + m;
    PLK_HIP(hipMemsetAsync(drec + pend.size(), 0, sizeof(PlkMsmResult), hs.st));
    if ((rc = plk_msm_serial_launch(dp + 3 * lo, ds + lo, hi - lo, drec + pend.size(), hs.st))) return rc;
    pend.push_back(g);
    if (pend.size() == NREC && (rc = flush())) return rc;
  }
  if ((rc = flush())) return rc;
  for (size_t g = 0; g < nseg; g++) memcpy(out3 + 3 * g, &h[4 * g], 3);
  return PLK_OK;
}

}  // extern "C"
