// KZG aggregate verification (include/plonkhip.h, "KZG aggregate verification"): n groups of m openings
// each, one verdict per group -- the random linear combination every KZG verifier forms, checked with two
// pairings per GROUP instead of two per opening.
//
// For canonical inputs the two accumulated points are integer sums of discrete logs (msm.hip's isomorphism
// E(F101) = Z/102), so the work is one streaming pass over 9 bytes per job
//     sL += r (LOG C + y (102 - lg) + z LOG W)       lg = LOG vk->g1; -y lg = y (102 - lg) mod 102
//     sW += r  LOG W
// and two pairings on EXP[sL mod 102], EXP[sW mod 102].  LOG is msm.hip's lookup d = E[y] - k (the log when the
// encoding is canonical, >= 256 otherwise) through an LDS table of 128 entries in 32 copies (copy = lane mod
// 32: ds_read_b32 banks are taken mod 32 within each 32-lane half, so the gathers are conflict free); the
// identity, E[256] there, is a select on the flag bit instead of a second table region.  The 102 meaningful
// words of E reach the kernel as an argument (capi.hip holds the host copy): no state, no upload.
//
// Three geometries, a function of (m, n) alone (plk_kzg_verify_agg_plan):
//   lane   m <= 32: one lane per group runs its m jobs byte-wise and the two pairings; one launch, no workspace
//   wave   m <= 2048: one wave per group, four groups per block in flight
//   block  otherwise: B = min(ceil(m / 16384), 1024) blocks per group, each a 16-aligned slice of the group
// wave and block write one (sL, sW, flags) record of 16 bytes per slice to d_work and a second launch finishes:
// one lane per group (B <= 8) or one wave per group sums the group's B records and runs the two pairings.
// Plain stores and a launch boundary: no atomics, nothing to initialise, every record read was written by the
// same call, and the sums are integers, so the result does not depend on any order.
//
// Groups that are valid but not canonical come out as PLK_KZG_AGG_UNDECIDED; the host form resolves them
// exactly: one lane per job materialises the raw L_i with G1Ops, msm.hip's exact raw fold runs over (L, r)
// and (W, r), and one lane runs the two pairings on the two folded points.
#include <algorithm>

#include "plk_device.h"
#include "plk_g1log.h"
#include "plk_hf17.h"
#include "plk_hostcall.h"
#include "plk_internal.h"
#include "plk_pairing.h"

namespace {

using namespace plkpair;
using plkg1log::TAB_C;
using plkg1log::TAB_E;
using plkg1log::dlog;
using plkg1log::g1_word;

constexpr uint32_t ORD = PLK_GROUP_ORDER;
constexpr int AGG_T = PAIR_T;                  // threads per block (stage_inverses strides by PAIR_T)
constexpr int AGG_WAVES = AGG_T / PLK_WAVE;
constexpr uint32_t F_INVALID = 1, F_IRREGULAR = 2;

constexpr uint64_t AGG_LANE_MAX = 32;          // m <= : one lane per group
constexpr uint64_t AGG_WAVE_MAX = 2048;        // m <= : one wave per group
constexpr uint64_t AGG_SLICE = 16384;          // jobs per block slice aimed at (256 threads x 4 steps of 16 jobs)
constexpr uint32_t AGG_MAX_SLICES = 1024;
constexpr uint32_t AGG_LANE_BLOCKS = 2048, AGG_STREAM_BLOCKS = 4096;
constexpr uint32_t AGG_FINISH_LANE_MAX = 8;    // slices per group a single lane still sums ...
constexpr uint64_t AGG_FINISH_WAVE_N = 4096;   // ... when there are more groups than this (else a wave per group: its
                                               // two pairings run side by side and the lanes are there to spare)
enum { PATH_LANE = 0, PATH_WAVE = 1, PATH_BLOCK = 2 };

// One job's terms stay below TERM_MAX for ANY nine bytes (a flagged group's sums are never used, but they must
// not leave 32 bits on the way): (255 + 255 x 101 + 255 x 255) x 255.
constexpr uint32_t TERM_MAX = (255u + 255u * 101u + 255u * 255u) * 255u;
static_assert((uint64_t)TERM_MAX * 16 < (1ull << 32), "a 16-job step fits 32 bits");

struct AggTab { uint32_t w[ORD]; };            // E[y], y < 101, then E[256]
struct AggIn { const uint8_t *c, *w, *z, *y, *r; };

__device__ __forceinline__ void job_term(uint32_t kc, uint32_t kw, uint32_t z, uint32_t y, uint32_t r, uint32_t nlg,
                                         const uint32_t* tab, uint32_t lane4, uint32_t& pl, uint32_t& pw, uint32_t& dor) {
  const uint32_t dc = dlog(kc, tab, lane4), dw = dlog(kw, tab, lane4);
  dor |= dc | dw;
  const uint32_t lw = dw & 0xFFu;
  pl += r * ((dc & 0xFFu) + y * nlg + z * lw);
  pw += r * lw;
}

// one job from its nine bytes, wherever they lie
__device__ __forceinline__ void job_bytes(const AggIn& in, uint64_t i, uint32_t nlg, const uint32_t* tab, uint32_t lane4,
                                          uint32_t& pl, uint32_t& pw, uint32_t& dor, uint32_t& flags) {
  const uint32_t cx = in.c[3 * i], cy = in.c[3 * i + 1], cf = in.c[3 * i + 2];
  const uint32_t wx = in.w[3 * i], wy = in.w[3 * i + 1], wf = in.w[3 * i + 2];
  const uint32_t z = in.z[i], y = in.y[i], r = in.r[i];
  if (cx >= GFP || cy >= GFP || cf > 1u || wx >= GFP || wy >= GFP || wf > 1u || z >= HFP || y >= HFP || r >= HFP)
    flags |= F_INVALID;
  job_term(cx << 8 | cy << 16 | cf << 24, wx << 8 | wy << 16 | wf << 24, z, y, r, nlg, tab, lane4, pl, pw, dor);
}

// non-zero when one of 16 points holds a coordinate >= 101 or a flag >= 2 (additions and masks only).  A byte
// b < 128 has b + a >= 0x80 exactly when b >= 0x80 - a, without a carry; a byte >= 128 keeps its own top bit.
// a = 0x1B for a coordinate, 0x7E for a flag; the roles x y f repeat every three words.
__device__ __forceinline__ uint32_t g1_invalid16(const uint32_t (&w)[12]) {
  uint32_t m = 0;
#pragma unroll
  for (int i = 0; i < 12; i += 3) {
    m |= ((w[i] & 0x7F7F7F7Fu) + 0x1B7E1B1Bu) | w[i];
    m |= ((w[i + 1] & 0x7F7F7F7Fu) + 0x1B1B7E1Bu) | w[i + 1];
    m |= ((w[i + 2] & 0x7F7F7F7Fu) + 0x7E1B1B7Eu) | w[i + 2];
  }
  return m & 0x80808080u;
}

__device__ __forceinline__ void words_of(const uint4& a, const uint4& b, const uint4& c, uint32_t (&w)[12]) {
  w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
  w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
  w[8] = c.x; w[9] = c.y; w[10] = c.z; w[11] = c.w;
}

template <int J>
__device__ __forceinline__ void unit_job(const uint32_t (&wc)[12], const uint32_t (&ww)[12], const uint32_t (&z)[4],
                                         const uint32_t (&y)[4], const uint32_t (&r)[4], uint32_t nlg, const uint32_t* tab,
                                         uint32_t lane4, uint32_t& pl, uint32_t& pw, uint32_t& dor) {
  job_term(g1_word<J>(wc), g1_word<J>(ww), hf17::byte_of(z, J), hf17::byte_of(y, J), hf17::byte_of(r, J), nlg, tab, lane4,
           pl, pw, dor);
}

// Jobs [j0, j0 + cnt) of the flat arrays, shared by the TEAM threads of which this one is number t: sl and sw
// come back reduced mod 102, flags with F_INVALID / F_IRREGULAR.  16 jobs per thread-step through nine 16-byte
// loads when the five bases are 16-byte aligned at j0 (then the cnt mod 16 tail, one job per thread);
// byte-wise otherwise, with the same result (vec_ok false: byte-wise whatever the bases).
template <int TEAM>
__device__ __forceinline__ void slice_sum(const AggIn& in, uint64_t j0, uint64_t cnt, uint32_t t, uint32_t nlg,
                                          const uint32_t* tab, uint32_t lane4, uint32_t& sl, uint32_t& sw, uint32_t& flags,
                                          bool vec_ok = true) {
  const uintptr_t bases = (uintptr_t)(in.c + 3 * j0) | (uintptr_t)(in.w + 3 * j0) | (uintptr_t)(in.z + j0) |
                          (uintptr_t)(in.y + j0) | (uintptr_t)(in.r + j0);
  uint32_t dor = 0, bad = 0;
  uint64_t done = 0;
  sl = sw = 0;
  if (vec_ok && bases % 16 == 0) {
    const uint4* c4 = reinterpret_cast<const uint4*>(in.c + 3 * j0);
    const uint4* w4 = reinterpret_cast<const uint4*>(in.w + 3 * j0);
    const uint4* z4 = reinterpret_cast<const uint4*>(in.z + j0);
    const uint4* y4 = reinterpret_cast<const uint4*>(in.y + j0);
    const uint4* r4 = reinterpret_cast<const uint4*>(in.r + j0);
    const uint64_t nu = cnt >> 4;
    for (uint64_t u = t; u < nu; u += TEAM) {
      const uint4 c0 = c4[3 * u], c1 = c4[3 * u + 1], c2 = c4[3 * u + 2];
      const uint4 w0 = w4[3 * u], w1 = w4[3 * u + 1], w2 = w4[3 * u + 2];
      const uint4 zv = z4[u], yv = y4[u], rv = r4[u];
      uint32_t wc[12], ww[12];
      words_of(c0, c1, c2, wc);
      words_of(w0, w1, w2, ww);
      const uint32_t z[4] = {zv.x, zv.y, zv.z, zv.w}, y[4] = {yv.x, yv.y, yv.z, yv.w}, r[4] = {rv.x, rv.y, rv.z, rv.w};
      bad |= g1_invalid16(wc) | g1_invalid16(ww);
      bad |= (hf17::top_bits4(z[0]) | hf17::top_bits4(z[1]) | hf17::top_bits4(z[2]) | hf17::top_bits4(z[3]) |
              hf17::top_bits4(y[0]) | hf17::top_bits4(y[1]) | hf17::top_bits4(y[2]) | hf17::top_bits4(y[3]) |
              hf17::top_bits4(r[0]) | hf17::top_bits4(r[1]) | hf17::top_bits4(r[2]) | hf17::top_bits4(r[3])) & 0x80808080u;
      uint32_t pl = 0, pw = 0;   // <= 16 TERM_MAX
      unit_job<0>(wc, ww, z, y, r, nlg, tab, lane4, pl, pw, dor);   unit_job<1>(wc, ww, z, y, r, nlg, tab, lane4, pl, pw, dor);
      unit_job<2>(wc, ww, z, y, r, nlg, tab, lane4, pl, pw, dor);   unit_job<3>(wc, ww, z, y, r, nlg, tab, lane4, pl, pw, dor);
      unit_job<4>(wc, ww, z, y, r, nlg, tab, lane4, pl, pw, dor);   unit_job<5>(wc, ww, z, y, r, nlg, tab, lane4, pl, pw, dor);
      unit_job<6>(wc, ww, z, y, r, nlg, tab, lane4, pl, pw, dor);   unit_job<7>(wc, ww, z, y, r, nlg, tab, lane4, pl, pw, dor);
      unit_job<8>(wc, ww, z, y, r, nlg, tab, lane4, pl, pw, dor);   unit_job<9>(wc, ww, z, y, r, nlg, tab, lane4, pl, pw, dor);
      unit_job<10>(wc, ww, z, y, r, nlg, tab, lane4, pl, pw, dor);  unit_job<11>(wc, ww, z, y, r, nlg, tab, lane4, pl, pw, dor);
      unit_job<12>(wc, ww, z, y, r, nlg, tab, lane4, pl, pw, dor);  unit_job<13>(wc, ww, z, y, r, nlg, tab, lane4, pl, pw, dor);
      unit_job<14>(wc, ww, z, y, r, nlg, tab, lane4, pl, pw, dor);  unit_job<15>(wc, ww, z, y, r, nlg, tab, lane4, pl, pw, dor);
      sl += pl % ORD;   // at most 2^30 / 16 / 64 = 2^20 steps a thread: the sums stay below 2^20 x 101 < 2^27
      sw += pw % ORD;
    }
    done = nu << 4;
  }
  for (uint64_t i = done + t; i < cnt; i += TEAM) {
    uint32_t pl = 0, pw = 0;
    job_bytes(in, j0 + i, nlg, tab, lane4, pl, pw, dor, flags);
    sl = (sl + pl) % ORD;
    sw = (sw + pw) % ORD;
  }
  sl %= ORD;
  sw %= ORD;
  if (bad) flags |= F_INVALID;
  if (dor >= 256u) flags |= F_IRREGULAR;
}

// the verdict byte of one group from its sums and flags: two pairings on EXP[sL], EXP[sW]
__device__ __forceinline__ uint32_t verdict(const G1Ops& G, const VkWords& vk, uint32_t vk_irregular, uint32_t sl, uint32_t sw,
                                            uint32_t flags, const uint32_t* expw) {
  const uint32_t a = expw[sl % ORD], b = expw[sw % ORD];   // {x, y, inf, 0}
  const Gt lhs = pairing(G, Pt{a & 0xFFu, (a >> 8) & 0xFFu, (a >> 16) & 0xFFu}, vk.h1x, vk.h1y);
  const Gt rhs = pairing(G, Pt{b & 0xFFu, (b >> 8) & 0xFFu, (b >> 16) & 0xFFu}, vk.hsx, vk.hsy);
  return (flags & F_INVALID) ? 2u
         : ((flags & F_IRREGULAR) || vk_irregular) ? (uint32_t)PLK_KZG_AGG_UNDECIDED
         : (lhs.a == rhs.a && lhs.b == rhs.b) ? 1u : 0u;
}

// the same byte computed by a whole wave (every lane holds the group's sums): lanes 0-31 run the left pairing and
// lanes 32-63 the right one, so the group waits for one pairing's dependent chain instead of two
__device__ __forceinline__ uint32_t verdict_wave(const G1Ops& G, const VkWords& vk, uint32_t vk_irregular, uint32_t sl,
                                                 uint32_t sw, uint32_t flags, const uint32_t* expw) {
  const bool right = (threadIdx.x & (PLK_WAVE - 1)) >= PLK_WAVE / 2;
  const uint32_t a = expw[(right ? sw : sl) % ORD];   // {x, y, inf, 0}
  const Gt e = pairing(G, Pt{a & 0xFFu, (a >> 8) & 0xFFu, (a >> 16) & 0xFFu}, right ? vk.hsx : vk.h1x, right ? vk.hsy : vk.h1y);
  const int both = (int)(e.a | e.b << 8);
  const bool eq = __builtin_amdgcn_readlane(both, 0) == __builtin_amdgcn_readlane(both, PLK_WAVE / 2);
  return (flags & F_INVALID) ? 2u : ((flags & F_IRREGULAR) || vk_irregular) ? (uint32_t)PLK_KZG_AGG_UNDECIDED : eq ? 1u : 0u;
}

// lane path: group g in one lane (m <= AGG_LANE_MAX), the pairings in the same lane.  A group size that is a
// multiple of 16 keeps every group as aligned as the arrays, and the lane takes the 16-byte loads (neighbouring
// lanes then read neighbouring 16-byte pieces); any other m runs byte-wise in every lane, so a wave never splits.
__global__ __launch_bounds__(AGG_T) void agg_lane_kernel(AggTab t, AggIn in, VkWords vk, uint32_t vk_irregular, uint32_t nlg,
                                                        uint32_t m, uint64_t n, const uint32_t* __restrict__ expw,
                                                        uint8_t* __restrict__ okb) {
  __shared__ __attribute__((aligned(16))) uint32_t tab[TAB_E * TAB_C];
  __shared__ uint32_t invl[GFP];
  plkg1log::stage_table<AGG_T>(t, tab);
  stage_inverses(invl);   // (ends with the barrier)
  const G1Ops G{invl};
  const uint32_t lane4 = (threadIdx.x & (TAB_C - 1u)) << 2;
  for (uint64_t g = (uint64_t)blockIdx.x * AGG_T + threadIdx.x; g < n; g += (uint64_t)gridDim.x * AGG_T) {
    uint32_t sl, sw, flags = 0;
    slice_sum<1>(in, g * m, m, 0u, nlg, tab, lane4, sl, sw, flags, m % 16 == 0);
    okb[g] = (uint8_t)verdict(G, vk, vk_irregular, sl, sw, flags, expw);
  }
}

// wave path (TEAM = 64, B = 1: the grid is blockIdx.x, four groups a block) and block path (TEAM = 256: slice
// blockIdx.x of B, groups blockIdx.y, blockIdx.y + gridDim.y, ...): record (g B + slice) of work = {sL, sW, flags, 0}
template <int TEAM>
__global__ __launch_bounds__(AGG_T) void agg_stream_kernel(AggTab t, AggIn in, uint32_t nlg, uint64_t m, uint64_t n, uint32_t B,
                                                          uint32_t* __restrict__ work) {
  __shared__ __attribute__((aligned(16))) uint32_t tab[TAB_E * TAB_C];
  __shared__ uint32_t part[AGG_WAVES][3];
  plkg1log::stage_table<AGG_T>(t, tab);
  __syncthreads();
  const uint32_t lane4 = (threadIdx.x & (TAB_C - 1u)) << 2;
  const uint32_t wave = threadIdx.x / PLK_WAVE, lane = threadIdx.x & (PLK_WAVE - 1);
  constexpr bool BLOCK = TEAM == AGG_T;
  const uint32_t slice = BLOCK ? blockIdx.x : 0u;
  const uint64_t gstep = BLOCK ? (uint64_t)gridDim.y : (uint64_t)gridDim.x * AGG_WAVES;
  const uint64_t per = ((m + B - 1) / B + 15) & ~15ull;   // a multiple of 16: every slice starts as aligned as the group
  const uint64_t lo = (uint64_t)slice * per < m ? (uint64_t)slice * per : m, hi = lo + per < m ? lo + per : m;
  for (uint64_t g = BLOCK ? (uint64_t)blockIdx.y : (uint64_t)blockIdx.x * AGG_WAVES + wave; g < n; g += gstep) {
    uint32_t sl, sw, flags = 0;
    slice_sum<TEAM>(in, g * m + lo, hi - lo, BLOCK ? threadIdx.x : lane, nlg, tab, lane4, sl, sw, flags);
    sl = plk_wave_sum(sl);   // <= 64 x 101
    sw = plk_wave_sum(sw);
    flags = (__ballot(flags & F_INVALID) ? F_INVALID : 0u) | (__ballot(flags & F_IRREGULAR) ? F_IRREGULAR : 0u);
    uint32_t* rec = work + ((uint64_t)g * B + slice) * 4;
    if (BLOCK) {
      if (lane == 0) {
        part[wave][0] = sl;
        part[wave][1] = sw;
        part[wave][2] = flags;
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        uint32_t a = 0, b = 0, f = 0;
#pragma unroll
        for (int k = 0; k < AGG_WAVES; k++) {
          a += part[k][0];
          b += part[k][1];
          f |= part[k][2];
        }
        rec[0] = a % ORD;
        rec[1] = b % ORD;
        rec[2] = f;
        rec[3] = 0;
      }
      __syncthreads();   // part is free for the block's next group
    } else if (lane == 0) {
      rec[0] = sl % ORD;
      rec[1] = sw % ORD;
      rec[2] = flags;
      rec[3] = 0;
    }
  }
}

// second launch: the group's B records summed by one lane (WAVE false) or by the lanes of one wave, then the pairings
template <bool WAVE>
__global__ __launch_bounds__(AGG_T) void agg_finish_kernel(VkWords vk, uint32_t vk_irregular, const uint32_t* __restrict__ work,
                                                          uint32_t B, uint64_t n, const uint32_t* __restrict__ expw,
                                                          uint8_t* __restrict__ okb) {
  __shared__ uint32_t invl[GFP];
  stage_inverses(invl);
  const G1Ops G{invl};
  if (WAVE) {
    const uint32_t wave = threadIdx.x / PLK_WAVE, lane = threadIdx.x & (PLK_WAVE - 1);
    for (uint64_t g = (uint64_t)blockIdx.x * AGG_WAVES + wave; g < n; g += (uint64_t)gridDim.x * AGG_WAVES) {
      uint32_t sl = 0, sw = 0, flags = 0;
      for (uint32_t b = lane; b < B; b += PLK_WAVE) {   // <= 16 records a lane: <= 16 x 101
        const uint32_t* rec = work + (g * B + b) * 4;
        sl += rec[0];
        sw += rec[1];
        flags |= rec[2];
      }
      sl = plk_wave_sum(sl);
      sw = plk_wave_sum(sw);
      flags = (__ballot(flags & F_INVALID) ? F_INVALID : 0u) | (__ballot(flags & F_IRREGULAR) ? F_IRREGULAR : 0u);
      const uint32_t v = verdict_wave(G, vk, vk_irregular, sl, sw, flags, expw);
      if (lane == 0) okb[g] = (uint8_t)v;
    }
  } else {
    for (uint64_t g = (uint64_t)blockIdx.x * AGG_T + threadIdx.x; g < n; g += (uint64_t)gridDim.x * AGG_T) {
      uint32_t sl = 0, sw = 0, flags = 0;
      for (uint32_t b = 0; b < B; b++) {
        const uint32_t* rec = work + (g * B + b) * 4;
        sl += rec[0];
        sw += rec[1];
        flags |= rec[2];
      }
      okb[g] = (uint8_t)verdict(G, vk, vk_irregular, sl, sw, flags, expw);
    }
  }
}

// host form, an undecided group: L_i = C_i - y_i G + z_i W_i with the raw formulas in the order the header
// fixes, one lane per job (the group's bytes are valid: an invalid group was decided as 2)
__global__ __launch_bounds__(AGG_T) void agg_raw_l_kernel(VkWords vk, AggIn in, uint64_t j0, uint64_t m,
                                                         uint8_t* __restrict__ l3) {
  __shared__ uint32_t invl[GFP];
  stage_inverses(invl);
  const G1Ops G{invl};
  const Pt g{vk.gx, vk.gy, vk.ginf};
  for (uint64_t i = (uint64_t)blockIdx.x * AGG_T + threadIdx.x; i < m; i += (uint64_t)gridDim.x * AGG_T) {
    bool ok = true;
    const Pt c = load_g1(in.c + 3 * (j0 + i), ok), w = load_g1(in.w + 3 * (j0 + i), ok);
    const uint32_t z = in.z[j0 + i] % 32u, y = in.y[j0 + i] % 32u;   // (< 17 here; G1Ops::mul takes k < 32)
    Pt l = G.add(c, G.negp(G.mul(g, y)));
    l = G.add(l, G.mul(w, z));
    l3[3 * i] = (uint8_t)l.x;
    l3[3 * i + 1] = (uint8_t)l.y;
    l3[3 * i + 2] = (uint8_t)l.inf;
  }
}

// host form, an undecided group: the two pairings on the two folded points (one block, one working lane)
__global__ __launch_bounds__(AGG_T) void agg_raw_finish_kernel(VkWords vk, const PlkMsmResult* __restrict__ rec,
                                                              uint8_t* __restrict__ okb) {
  __shared__ uint32_t invl[GFP];
  stage_inverses(invl);
  const G1Ops G{invl};
  if (threadIdx.x != 0) return;
  const Pt a{rec[0].g1[0], rec[0].g1[1], rec[0].g1[2]}, b{rec[1].g1[0], rec[1].g1[1], rec[1].g1[2]};
  const Gt lhs = pairing(G, a, vk.h1x, vk.h1y), rhs = pairing(G, b, vk.hsx, vk.hsy);
  *okb = (lhs.a == rhs.a && lhs.b == rhs.b) ? 1 : 0;
}

struct Plan {
  int path;
  uint32_t slices;    // B: records per group (0 on the lane path)
  uint32_t gx, gy;    // the first launch's grid
  int launches;
};

// (m, n) checked by the caller: m, n >= 1, m n <= 2^30
Plan plan_of(uint64_t m, uint64_t n) {
  Plan p{};
  if (m <= AGG_LANE_MAX) {
    p = Plan{PATH_LANE, 0u, (uint32_t)std::min<uint64_t>((n + AGG_T - 1) / AGG_T, AGG_LANE_BLOCKS), 1u, 1};
  } else if (m <= AGG_WAVE_MAX) {
    p = Plan{PATH_WAVE, 1u, (uint32_t)std::min<uint64_t>((n + AGG_WAVES - 1) / AGG_WAVES, AGG_STREAM_BLOCKS), 1u, 2};
  } else {
    const uint32_t B = (uint32_t)std::min<uint64_t>((m + AGG_SLICE - 1) / AGG_SLICE, AGG_MAX_SLICES);
    p = Plan{PATH_BLOCK, B, B, (uint32_t)std::min<uint64_t>(n, std::max<uint32_t>(AGG_STREAM_BLOCKS / B, 1u)), 2};
  }
  return p;
}

// PLK_OK, or the code the launch would return for this (m, n)
int check_shape(const char* fn, size_t m, size_t n, bool quiet = false) {
  if (m == 0 || n == 0) {
    if (!quiet) plk_set_error("%s: m > 0 and n > 0 are required", fn);
    return PLK_ERR_ARG;
  }
  if (m > PAIR_MAX_N || n > PAIR_MAX_N / m) {
    if (!quiet) plk_set_error("%s: m n = %zu x %zu exceeds 2^30 jobs per call", fn, m, n);
    return PLK_ERR_RANGE;
  }
  return PLK_OK;
}

// everything that comes before any device query
int check_call(const char* fn, const plk_kzg_vk_t* vk, size_t m, bool null_arg, size_t n, VkWords* w) {
  if (!vk || null_arg) {
    plk_set_error("%s: every pointer is required", fn);
    return PLK_ERR_ARG;
  }
  if (m == 0 || n == 0) return check_shape(fn, m, n);
  int rc = check_vk(fn, vk, w);
  return rc ? rc : check_shape(fn, m, n);
}

struct HostStream {
  hipStream_t st = nullptr;
  ~HostStream() {
    if (st) (void)hipStreamDestroy(st);
  }
};

}  // namespace

extern "C" {

int plk_kzg_verify_agg_plan(size_t m, size_t n, int64_t out[4]) {
  const char* fn = "plk_kzg_verify_agg_plan";
  if (!out) {
    plk_set_error("%s: out is required", fn);
    return PLK_ERR_ARG;
  }
  const int rc = check_shape(fn, m, n);
  if (rc) return rc;
  const Plan p = plan_of(m, n);
  out[0] = p.path;
  out[1] = p.slices;
  out[2] = (int64_t)p.gx * p.gy;
  out[3] = p.launches;
  return PLK_OK;
}

size_t plk_kzg_verify_agg_workspace(size_t m, size_t n) {
  if (check_shape("plk_kzg_verify_agg_workspace", m, n, true)) return 0;
  return (size_t)plan_of(m, n).slices * n * 16;
}

int plk_kzg_verify_agg_batch_dev(const plk_kzg_vk_t* vk, size_t m, const uint8_t* d_commits3, const uint8_t* d_zs,
                                 const uint8_t* d_ys, const uint8_t* d_proofs3, const uint8_t* d_rs, size_t n, uint8_t* d_ok,
                                 void* d_work, void* stream) {
  const char* fn = "plk_kzg_verify_agg_batch_dev";
  VkWords w;
  int rc = check_call(fn, vk, m, !d_commits3 || !d_zs || !d_ys || !d_proofs3 || !d_rs || !d_ok, n, &w);
  if (rc) return rc;
  const Plan p = plan_of(m, n);
  if (p.launches > 1 && (!d_work || (uintptr_t)d_work % 4)) {
    plk_set_error("%s: d_work (plk_kzg_verify_agg_workspace bytes, 4-byte aligned) is required for m = %zu", fn, m);
    return PLK_ERR_ARG;
  }
  if ((rc = plk_use_device())) return rc;
  AggTab t;
  plk_group_ytab_words(t.w);
  // lg = LOG vk->g1 by the kernel's own lookup; a key that is no canonical group element leaves every group undecided
  const uint32_t k = w.gx << 8 | w.gy << 16 | w.ginf << 24;
  const uint32_t d = (w.ginf ? t.w[ORD - 1] : t.w[w.gy]) - k;
  const uint32_t vk_irregular = d >= 256u ? 1u : 0u;
  const uint32_t nlg = vk_irregular ? 0u : (ORD - d) % ORD;
  const AggIn in{d_commits3, d_proofs3, d_zs, d_ys, d_rs};
  const uint32_t* expw = plk_msm_exp_words_dev();
  hipStream_t st = (hipStream_t)stream;
  uint32_t* work = (uint32_t*)d_work;
  if (p.path == PATH_LANE) {
    hipLaunchKernelGGL(agg_lane_kernel, dim3(p.gx), dim3(AGG_T), 0, st, t, in, w, vk_irregular, nlg, (uint32_t)m, (uint64_t)n,
                       expw, d_ok);
    PLK_HIP(hipGetLastError());
    return PLK_OK;
  }
  if (p.path == PATH_WAVE)
    hipLaunchKernelGGL(agg_stream_kernel<PLK_WAVE>, dim3(p.gx), dim3(AGG_T), 0, st, t, in, nlg, (uint64_t)m, (uint64_t)n, 1u,
                       work);
  else
    hipLaunchKernelGGL(agg_stream_kernel<AGG_T>, dim3(p.gx, p.gy), dim3(AGG_T), 0, st, t, in, nlg, (uint64_t)m, (uint64_t)n,
                       p.slices, work);
  PLK_HIP(hipGetLastError());
  if (p.slices <= AGG_FINISH_LANE_MAX && n > AGG_FINISH_WAVE_N)
    hipLaunchKernelGGL(agg_finish_kernel<false>, dim3((uint32_t)std::min<uint64_t>((n + AGG_T - 1) / AGG_T, AGG_LANE_BLOCKS)),
                       dim3(AGG_T), 0, st, w, vk_irregular, work, p.slices, (uint64_t)n, expw, d_ok);
  else
    hipLaunchKernelGGL(agg_finish_kernel<true>,
                       dim3((uint32_t)std::min<uint64_t>((n + AGG_WAVES - 1) / AGG_WAVES, AGG_LANE_BLOCKS)), dim3(AGG_T), 0, st,
                       w, vk_irregular, work, p.slices, (uint64_t)n, expw, d_ok);
  PLK_HIP(hipGetLastError());
  return PLK_OK;
}

int plk_kzg_verify_agg_batch(const plk_kzg_vk_t* vk, size_t m, const uint8_t* commits3, const uint8_t* zs, const uint8_t* ys,
                             const uint8_t* proofs3, const uint8_t* rs, size_t n, uint8_t* ok) {
  const char* fn = "plk_kzg_verify_agg_batch";
  VkWords w;
  int rc = check_call(fn, vk, m, !commits3 || !zs || !ys || !proofs3 || !rs || !ok, n, &w);
  if (rc || (rc = plk_select_device())) return rc;
  const size_t e = m * n, ws = plk_kzg_verify_agg_workspace(m, n);
  Staged D;   // every array on a 16-byte boundary: the streaming pass then takes its 16-byte loads
  if ((rc = D.alloc(fn, 2 * plk_pad16(3 * e) + 3 * plk_pad16(e) + plk_pad16(n) + ws))) return rc;
  uint8_t *c = D.add(commits3, 3 * e, 16), *p = D.add(proofs3, 3 * e, 16), *z = D.add(zs, e, 16), *y = D.add(ys, e, 16),
          *r = D.add(rs, e, 16), *o = D.add(nullptr, n, 16), *wk = D.add(nullptr, ws, 16);
  if ((rc = D.rc) || (rc = plk_kzg_verify_agg_batch_dev(vk, m, c, z, y, p, r, n, o, ws ? wk : nullptr, nullptr))) return rc;
  PLK_HIP(hipMemcpy(ok, o, n, hipMemcpyDeviceToHost));
  // undecided groups, exactly: raw L_i, the raw fold of (L, r) and of (W, r), two pairings
  PlkScratch R;
  HostStream hs;
  uint8_t* l3 = nullptr;
  PlkMsmResult* rec = nullptr;
  const AggIn in{c, p, z, y, r};
  for (size_t g = 0; g < n; g++) {
    if (ok[g] != PLK_KZG_AGG_UNDECIDED) continue;
    if (!R.d) {
      const size_t lb = (3 * m + 255) & ~(size_t)255;
      if ((rc = R.alloc(fn, lb + 2 * sizeof(PlkMsmResult)))) return rc;
      l3 = R.d;
      rec = (PlkMsmResult*)(R.d + lb);
      PLK_HIP(hipStreamCreate(&hs.st));
      PLK_HIP(hipMemsetAsync(rec, 0, 2 * sizeof(PlkMsmResult), hs.st));
    }
    const size_t j0 = g * m;
    hipLaunchKernelGGL(agg_raw_l_kernel, dim3((uint32_t)std::min<size_t>((m + AGG_T - 1) / AGG_T, AGG_LANE_BLOCKS)), dim3(AGG_T),
                       0, hs.st, w, in, (uint64_t)j0, (uint64_t)m, l3);
    PLK_HIP(hipGetLastError());
    if ((rc = plk_msm_serial_launch(l3, r + j0, m, rec, hs.st)) || (rc = plk_msm_serial_launch(p + 3 * j0, r + j0, m, rec + 1, hs.st)))
      return rc;
    hipLaunchKernelGGL(agg_raw_finish_kernel, dim3(1), dim3(AGG_T), 0, hs.st, w, rec, o + g);
    PLK_HIP(hipGetLastError());
  }
  if (R.d) {
    PLK_HIP(hipStreamSynchronize(hs.st));
    PLK_HIP(hipMemcpy(ok, o, n, hipMemcpyDeviceToHost));
  }
  return PLK_OK;
}

}  // extern "C"
