// KZG flat multi-point openings (include/plonkhip.h, "KZG flat multi-point openings"): very many GROUPS of short
// polynomials, each polynomial opened at its own set S_i of GF(17) points, two G1 elements W, W' a group, in one
// launch -- the producer at the scale of plk_kzg_verify_multi_batch_dev.  The layout is kzg_fold_flat.hip's:
// polynomial e is the bytes [o_e, o_{e+1}) of ONE flat coefficient array; group g owns polynomials, masks, weights
// and 17-byte ys rows [k g, k (g + 1)) and the one device byte us[g].
//
// The arithmetic is kzg_multi.hip's with one chunk and nothing to finish across blocks, in the other loop order:
//   h  = sum_i sum_{a in S_i} (w_i lambda_ia) Q_a(p_i),  lambda_ia = 1 / prod_{b in S_i, b != a} (a - b),
//        Q_a the single-point quotient (partial fractions of p_i div Z_i);            W  = [h]
//   F' = sum_i c_i p_i - c_T h,  c = plk_kzg_multi_coeffs of the group's masks;        W' = [Q_u(F')]
// Polynomials in the outer loop, the points of S_i in the inner one.  The total of the suffix scan at a IS p_i(a),
// so one scan gives the ys byte and the quotient's carry.  (w_i lambda_ia) q is summed exactly into sixteen h sums
// per thread and c_i p_i into sixteen F' sums in the same pass; each is reduced once.  u in T is no special case,
// because F' is formed explicitly and its remainder is simply dropped.  Nothing but the outputs reaches memory: no
// q_i, h or F'.  T = the union of the masks is read before the first polynomial is folded (group_of).
// Three paths, a function of m alone (plk_kzg_multi_flat_plan), each ONE launch with a grid-stride loop:
//   lane   m <= 32: one lane per group, both halves of sixteen coefficients in registers; the carry into the
//          lower half is the upper half's dot product (a^16 = 1).  The block holds the first 32 SRS logs in LDS.
//   wave   32 < m <= 1024: one wave per group, sixteen coefficients per lane, one hf17::wave_suffix per
//          (polynomial, point).  No LDS, no barrier.
//   block  1024 < m <= 4096: one block per group, kzgo::suffix_carry with one chunk per (polynomial, point).
// The wave and block paths are one kernel template.  Polynomials are taken one at a time, so no kernel depends on
// k.  Plain stores only: no workspace, no atomics, no record; every sum is an integer, so the bytes do not depend
// on any order.
#include <string.h>

#include <algorithm>
#include <vector>

#include "plk_device.h"
#include "plk_hf17.h"
#include "plk_hostcall.h"
#include "plk_internal.h"
#include "plk_kzg_host.h"
#include "plk_kzg_open.h"

namespace {

constexpr uint32_t HFP = hf17::P;
constexpr uint32_t ORD = PLK_GROUP_ORDER;
constexpr uint32_t NPTS = 17;                            // GF(17) points, the width of a ys row
constexpr uint32_t FULL_MASK = (1u << NPTS) - 1;
constexpr uint32_t LANE_MAX = 32;                        // m <= : the lane path
constexpr uint32_t WAVE_MAX = PLK_WAVE * kzgo::E;        // m <= : the wave path (1024)
constexpr uint32_t MULTI_BLOCKS = 2048;                  // grid cap of every path (grid-stride loops)
constexpr uint64_t MAX_TOTAL = 1ull << 32, MAX_NPOLY = 1ull << 30;
constexpr uint32_t G1_FLAGGED = 0xFFFFFFu;               // bytes FF FF FF
static_assert(PLK_KZG_FLAT_MAX == kzgo::CHUNK, "a polynomial is one chunk of the opening family");
static_assert(WAVE_MAX == 1024 && LANE_MAX == 2 * kzgo::E, "the paths' bounds as the header states them");
static_assert(PLK_KZG_MULTI_MAX <= kzgo::E && NPTS <= PLK_WAVE, "threads i < k store the commitments, threads a < 17 a ys row");
static_assert(PLK_KZG_MULTI_POINTS == NPTS - 1, "a set is at most sixteen of the seventeen points");
// an h sum before its one reduction: one term (w lambda) q per (polynomial, point of its set), both factors < 17
static_assert((uint32_t)PLK_KZG_MULTI_MAX * PLK_KZG_MULTI_POINTS * 16u * 16u < hf17::MOD17_BOUND, "sum (w lambda) q stays inside mod17's range");
// an F' sum before its one reduction: c_i < 17 on bytes <= 255, then (17 - c_T) h[j], both < 17
static_assert((uint32_t)PLK_KZG_MULTI_MAX * 16u * 255u + 16u * 16u < hf17::MOD17_BOUND, "sum c_i byte - c_T h stays inside mod17's range");
// a scan's input: the dot product of sixteen bytes with powers < 17
static_assert(16u * 255u * 16u < hf17::MOD17_BOUND, "a thread's aggregate stays inside mod17's range");
// a packed sum carries W's share in [15:0] and W''s in [31:16], each < 102, over 256 threads
static_assert(256u * 101u < (1u << 16), "the two halves of a packed sum do not meet");
static_assert(2ull * 16 * 255 * 101 < (1ull << 32), "the lane path's sums fit 32 bits");

enum { PATH_LANE = 0, PATH_WAVE = 1, PATH_BLOCK = 2 };

struct MultiArgs {
  const uint8_t* coeffs;
  uint64_t total;
  const uint32_t* off;      // k ngroups + 1 words, or nullptr: o_e = e m
  uint64_t ngroups;
  uint32_t m, k;
  uint32_t srs_bad;         // the SRS has no log form: every G1 output is flagged, ys stay exact
  const uint32_t* sets;     // k ngroups masks
  const uint8_t* weights;   // k ngroups
  const uint8_t* us;        // ngroups
  const uint8_t* logs;      // the SRS logs, zero padded (plk_kzg_host.h)
  const uint32_t* expw;     // the 102 EXP words {x, y, infinite, 0}
  uint8_t *ys, *proofs6;
  uint8_t* commits3;        // or nullptr
  uint8_t* status;
};

__host__ __device__ __forceinline__ bool mask_ok(uint32_t m) { return m != 0 && (m & ~FULL_MASK) == 0 && m != FULL_MASK; }

// Polynomial e: its first byte and length.  Offsets are read as min(o, total), so no value makes a caller of
// this read outside [0, total); false for a ragged polynomial that is empty, falls, has an offset above total
// or is longer than m.
__device__ __forceinline__ bool segment_of(const MultiArgs& A, uint64_t e, uint64_t& lo, uint32_t& len) {
  if (!A.off) {
    lo = e * A.m;   // (m k ngroups == total: checked by the caller)
    len = A.m;
    return true;
  }
  const uint64_t a = A.off[e], b = A.off[e + 1];
  const bool ok = a < b && b <= A.total && b - a <= A.m;
  lo = std::min(a, A.total);
  len = ok ? (uint32_t)(b - a) : 0u;
  return ok;
}

// Group g before any coefficient is read: false (PLK_KZG_FLAT_BAD) when one of its segments is broken, one of its
// masks is invalid or its u byte or one of its weight bytes is >= 17; L: the longest polynomial; T: the union of
// the masks.  Every thread of a wave or block that shares g reads the same bytes, so the answer is uniform there.
__device__ __forceinline__ bool group_of(const MultiArgs& A, uint64_t g, uint32_t& u, uint32_t& L, uint32_t& T) {
  const uint64_t e0 = g * A.k;
  const uint32_t ub = A.us[g];
  bool ok = ub < HFP;
  u = ok ? ub : 0u;
  L = A.off ? 0u : A.m;
  T = 0;
  for (uint32_t i = 0; i < A.k; i++) {
    const uint32_t mk = A.sets[e0 + i];
    ok = ok && A.weights[e0 + i] < HFP && mask_ok(mk);
    T |= mk;
    if (A.off) {
      uint64_t lo;
      uint32_t len;
      ok = segment_of(A, e0 + i, lo, len) && ok;
      L = max(L, len);
    }
  }
  return ok;
}

// prod_{b in mk} (x - b) mod 17 (x < 17; a product step <= 16 x 33)
__device__ __forceinline__ uint32_t vanish_at(uint32_t mk, uint32_t x) {
  uint32_t r = 1;
  for (; mk; mk &= mk - 1) r = hf17::mod17(r * (x + HFP - (uint32_t)__builtin_ctz(mk)));
  return r;
}
// w lambda_a mod 17 for the point a of the set mk
__device__ __forceinline__ uint32_t point_weight(uint32_t mk, uint32_t a, uint32_t w) {
  return hf17::mod17(w * hf17::inv_canon(vanish_at(mk & ~(1u << a), a)));
}

__device__ __forceinline__ void store_g1(uint8_t* out3, uint64_t e, uint32_t v) {
  out3[3 * e] = (uint8_t)v;
  out3[3 * e + 1] = (uint8_t)(v >> 8);
  out3[3 * e + 2] = (uint8_t)(v >> 16);
}
// polynomial e of a valid group: the commitment, exact for any coefficient byte (g1_mul takes the raw byte);
// sp: sum p_j log_j (any multiple of 102 on top)
__device__ __forceinline__ void store_commit(const MultiArgs& A, uint64_t e, uint32_t sp) {
  if (A.commits3) store_g1(A.commits3, e, A.srs_bad ? G1_FLAGGED : A.expw[sp % ORD]);
}
// group g's status and two proofs; sw, sq: sum h_j log_j and sum q_j log_j of F''s quotient
__device__ __forceinline__ void store_group(const MultiArgs& A, uint64_t g, bool ok, bool noncanon, uint32_t sw, uint32_t sq) {
  const uint32_t st = !ok ? (uint32_t)PLK_KZG_FLAT_BAD : (A.srs_bad || noncanon) ? (uint32_t)PLK_KZG_FLAT_IRREGULAR : 0u;
  A.status[g] = (uint8_t)st;
  store_g1(A.proofs6, 2 * g, st ? G1_FLAGGED : A.expw[sw % ORD]);
  store_g1(A.proofs6, 2 * g + 1, st ? G1_FLAGGED : A.expw[sq % ORD]);
}
// a PLK_KZG_FLAT_BAD group, shared by the nt threads t = 0 .. nt - 1 of its unit
__device__ __forceinline__ void store_group_bad(const MultiArgs& A, uint64_t g, uint32_t t, uint32_t nt) {
  const uint64_t e0 = g * A.k;
  for (uint32_t j = t; j < NPTS * A.k; j += nt) A.ys[NPTS * e0 + j] = 0xFF;
  if (A.commits3)
    for (uint32_t i = t; i < A.k; i += nt) store_g1(A.commits3, e0 + i, G1_FLAGGED);
  if (t == 0) store_group(A, g, false, false, 0, 0);
}

// acc[j] += w x byte j of nb: per-byte multiply-adds on genuine bytes (<= 16 x 255 a term)
__device__ __forceinline__ void weighted_add(const uint32_t (&nb)[4], uint32_t w, uint32_t (&acc)[kzgo::E]) {
#pragma unroll
  for (int j = 0; j < kzgo::E; j++) acc[j] += w * hf17::byte_of(nb, j);
}
// sixteen canonical bytes from their exact sums
__device__ __forceinline__ void reduce16(const uint32_t (&acc)[kzgo::E], uint32_t (&nb)[4]) {
  nb[0] = nb[1] = nb[2] = nb[3] = 0;
#pragma unroll
  for (int j = 0; j < kzgo::E; j++) nb[j >> 2] |= hf17::mod17(acc[j]) << (8 * (j & 3));
}
// F''s sixteen canonical bytes: facc[j] + (17 - c_T) h[j]
__device__ __forceinline__ void fprime16(const uint32_t (&facc)[kzgo::E], const uint32_t (&hb)[4], uint32_t ctn, uint32_t (&fb)[4]) {
  fb[0] = fb[1] = fb[2] = fb[3] = 0;
#pragma unroll
  for (int j = 0; j < kzgo::E; j++) fb[j >> 2] |= hf17::mod17(facc[j] + ctn * hf17::byte_of(hb, j)) << (8 * (j & 3));
}
// the puts of the h sums: a quotient byte < 17 (quotient16), a raw byte reduced first (shift16)
struct AddScaled {
  uint32_t (&acc)[kzgo::E];
  uint32_t lw;
  __device__ __forceinline__ void operator()(int j, uint32_t q) const { acc[j] += lw * q; }
};
struct AddScaledRaw {
  uint32_t (&acc)[kzgo::E];
  uint32_t lw;
  __device__ __forceinline__ void operator()(int j, uint32_t q) const { acc[j] += lw * hf17::mod17(q); }
};

// lane path: see the head of this file.  VEC (uniform, m a multiple of 16, coefficients 16-byte aligned):
// every polynomial is as aligned as the array.
template <bool VEC>
__global__ __launch_bounds__(kzgo::T) void multi_lane_kernel(MultiArgs A) {
  __shared__ __attribute__((aligned(16))) uint32_t slog[LANE_MAX / 4];   // the first 32 SRS logs, four to a word
  if (threadIdx.x < LANE_MAX / 4)
    slog[threadIdx.x] = A.srs_bad ? 0u : reinterpret_cast<const uint32_t*>(A.logs)[threadIdx.x];   // (>= 32 bytes, zero padded)
  __syncthreads();
  const bool commit = A.commits3 != nullptr;
  for (uint64_t g = (uint64_t)blockIdx.x * kzgo::T + threadIdx.x; g < A.ngroups; g += (uint64_t)gridDim.x * kzgo::T) {
    const uint64_t e0 = g * A.k;
    uint32_t u, L, T;
    if (!group_of(A, g, u, L, T)) {
      store_group_bad(A, g, 0, 1);
      continue;
    }
    uint32_t l[2][4];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const uint4 lv = *reinterpret_cast<const uint4*>(&slog[4 * h]);
      l[h][0] = lv.x; l[h][1] = lv.y; l[h][2] = lv.z; l[h][3] = lv.w;
    }
    const uint32_t ctn = hf17::neg(vanish_at(T, u));
    uint32_t hacc[2][kzgo::E], facc[2][kzgo::E];
#pragma unroll
    for (int j = 0; j < kzgo::E; j++) hacc[0][j] = hacc[1][j] = facc[0][j] = facc[1][j] = 0;
    bool noncanon = false;
    for (uint32_t i = 0; i < A.k; i++) {
      uint64_t lo;
      uint32_t len;
      (void)segment_of(A, e0 + i, lo, len);
      const uint8_t* p = A.coeffs + lo;
      const uint32_t mk = A.sets[e0 + i], w = A.weights[e0 + i];
      const bool two = len > kzgo::E;
      uint32_t nb[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
      for (int h = 0; h < 2; h++) {
        if (16u * h < len) {
          if (VEC) kzgo::load16_vec(p, 16u * h, nb[h]);
          else kzgo::load16_rolled(p, len, 16u * h, nb[h]);
        }
      }
      noncanon |= hf17::any_noncanonical(nb[0]) || hf17::any_noncanonical(nb[1]);
      const uint32_t ci = hf17::mod17(w * vanish_at(T & ~mk, u));
      weighted_add(nb[0], ci, facc[0]);
      if (two) weighted_add(nb[1], ci, facc[1]);
      if (commit) store_commit(A, e0 + i, kzgo::dot16(l[0], nb[0]) + kzgo::dot16(l[1], nb[1]));   // (<= 16 x 101 x 255 a half)
      uint8_t* row = A.ys + NPTS * (e0 + i);
      for (uint32_t a = 0; a < NPTS; a++)
        if (!((mk >> a) & 1u)) row[a] = 0xFF;
      for (uint32_t mm = mk; mm; mm &= mm - 1) {
        const uint32_t a = (uint32_t)__builtin_ctz(mm), lw = point_weight(mk, a, w);
        if (a != 0) {
          // the upper half has nothing above it; the carry into the lower half is the upper half's aggregate
          // (a^16 = 1), and both aggregates together are p_i(a)
          uint32_t pk[4];
          kzgo::packed_powers(a, pk);
          const uint32_t t1 = kzgo::dot16(nb[1], pk), t0 = kzgo::dot16(nb[0], pk);   // (<= 16 x 255 x 16 each)
          row[a] = (uint8_t)((t0 + t1) % HFP);
          if (two) kzgo::quotient16(nb[1], a, 0u, AddScaled{hacc[1], lw});
          kzgo::quotient16(nb[0], a, t1, AddScaled{hacc[0], lw});
        } else {
          row[0] = (uint8_t)((nb[0][0] & 0xFFu) % HFP);
          if (two) kzgo::shift16(nb[1], 0u, AddScaledRaw{hacc[1], lw});
          kzgo::shift16(nb[0], nb[1][0] & 0xFFu, AddScaledRaw{hacc[0], lw});
        }
      }
    }
    // h and F' from their sums, then F''s quotient at u from the top half down as a polynomial's above
    uint32_t hb[2][4], fb[2][4], o[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
    for (int h = 0; h < 2; h++) {
      reduce16(hacc[h], hb[h]);
      fprime16(facc[h], hb[h], ctn, fb[h]);
    }
    const bool two = L > kzgo::E;   // (else the upper halves are zero)
    if (u != 0) {
      uint32_t pk[4];
      kzgo::packed_powers(u, pk);
      if (two) kzgo::quotient16(fb[1], u, 0u, kzgo::PackInto{o[1]});
      kzgo::quotient16(fb[0], u, kzgo::dot16(fb[1], pk), kzgo::PackInto{o[0]});
    } else {
      if (two) kzgo::shift16(fb[1], 0u, kzgo::PackInto{o[1]});
      kzgo::shift16(fb[0], fb[1][0] & 0xFFu, kzgo::PackInto{o[0]});
    }
    store_group(A, g, true, noncanon, kzgo::dot16(l[0], hb[0]) + kzgo::dot16(l[1], hb[1]),
                kzgo::dot16(l[0], o[0]) + kzgo::dot16(l[1], o[1]));
  }
}

// The sixteen coefficients [base, base + 16) of a polynomial of len bytes at p, zero past len
__device__ __forceinline__ void load_run(const uint8_t* p, uint32_t len, uint32_t base, uint32_t (&nb)[4]) {
  if (kzgo::aligned16(p) && base + 16 <= len)
    kzgo::load16_vec(p, base, nb);
  else
    kzgo::load16_rolled(p, len, base, nb);
}

// wave (BLK false) and block (BLK true) paths: see the head of this file.  A unit -- a wave, a block -- owns one
// group, so group_of's answer, the masks and every branch on them are uniform over the unit; the block path's
// barriers all sit under such branches.
template <bool BLK>
__global__ __launch_bounds__(kzgo::T) void multi_wide_kernel(MultiArgs A) {
  __shared__ uint32_t ws[2][2 * kzgo::WAVES];                 // suffix_carry's words, alternating from scan to scan
  __shared__ uint32_t psum[PLK_KZG_MULTI_MAX][kzgo::WAVES];   // per polynomial and wave: the commitment share
  __shared__ uint32_t red[3][kzgo::WAVES];                    // per wave: the packed proof sums, a byte >= 17, F''s first byte
  const uint32_t wv = threadIdx.x / PLK_WAVE, lane = threadIdx.x & (PLK_WAVE - 1);
  const uint32_t t = BLK ? threadIdx.x : lane, nt = BLK ? (uint32_t)kzgo::T : (uint32_t)PLK_WAVE;   // the thread in its unit
  const uint32_t base = t * kzgo::E;
  const uint64_t first = BLK ? (uint64_t)blockIdx.x : (uint64_t)blockIdx.x * kzgo::WAVES + wv;
  const uint64_t stride = BLK ? (uint64_t)gridDim.x : (uint64_t)gridDim.x * kzgo::WAVES;
  uint32_t par = 0;
  for (uint64_t g = first; g < A.ngroups; g += stride) {
    const uint64_t e0 = g * A.k;
    uint32_t u, L, T;
    if (!group_of(A, g, u, L, T)) {   // (uniform)
      store_group_bad(A, g, t, nt);
      continue;
    }
    u = (uint32_t)__builtin_amdgcn_readfirstlane((int)u);   // (every thread read the same bytes)
    T = (uint32_t)__builtin_amdgcn_readfirstlane((int)T);
    const uint32_t ctn = hf17::neg(vanish_at(T, u));
    const uint4 lg = kzgo::Finish::logs(A.logs, A.srs_bad, base, L);
    const uint32_t l[4] = {lg.x, lg.y, lg.z, lg.w};
    uint32_t hacc[kzgo::E], facc[kzgo::E];
#pragma unroll
    for (int j = 0; j < kzgo::E; j++) hacc[j] = facc[j] = 0;
    bool noncanon = false;
    uint32_t mine = 0;   // wave path, lane i: polynomial i's commitment sum
    // the aggregates of the unit's later threads; on thread 0, run + tot is the whole sum
    const auto scan = [&](uint32_t tot) -> uint32_t {
      if (BLK) {
        bool unused = false;
        const uint32_t run = kzgo::suffix_carry(tot, nullptr, 0u, 1u, ws[par], unused);   // no other chunk
        par ^= 1u;   // (the next scan's words: a wave may arrive there while another still reads these)
        return run;
      }
      return hf17::wave_suffix(tot) - tot;
    };
    for (uint32_t i = 0; i < A.k; i++) {   // (uniform)
      const uint64_t e = e0 + i;
      uint64_t lo;
      uint32_t len, nb[4];
      (void)segment_of(A, e, lo, len);
      const uint8_t* p = A.coeffs + lo;
      const uint32_t mk = (uint32_t)__builtin_amdgcn_readfirstlane((int)A.sets[e]);
      const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)A.weights[e]);
      load_run(p, len, base, nb);
      noncanon |= hf17::any_noncanonical(nb);
      weighted_add(nb, hf17::mod17(w * vanish_at(T & ~mk, u)), facc);
      if (A.commits3) {
        const uint32_t s = plk_wave_sum(kzgo::dot16(l, nb) % ORD);   // (a share < 102: the sum <= 64 x 101)
        if (BLK) {
          if (lane == 0) psum[i][wv] = s;
        } else if (lane == i) {
          mine = s;
        }
      }
      uint8_t* row = A.ys + NPTS * e;
      if (t < NPTS && !((mk >> t) & 1u)) row[t] = 0xFF;
      for (uint32_t mm = mk; mm; mm &= mm - 1) {   // (uniform) the points of S_i
        const uint32_t a = (uint32_t)__builtin_ctz(mm), lw = point_weight(mk, a, w);
        if (a != 0) {
          uint32_t pk[4];
          kzgo::packed_powers(a, pk);
          const uint32_t tot = hf17::mod17(kzgo::dot16(nb, pk));   // (<= 16 x 255 x 16)
          const uint32_t run = scan(tot);
          if (t == 0) row[a] = (uint8_t)((run + tot) % HFP);
          kzgo::quotient16(nb, a, run, AddScaled{hacc, lw});
        } else {
          // q[j] = p[j + 1]: the thread's last quotient byte is the next thread's first coefficient
          if (t == 0) row[0] = (uint8_t)((nb[0] & 0xFFu) % HFP);
          kzgo::shift16(nb, base + 16 < len ? (uint32_t)p[base + 16] : 0u, AddScaledRaw{hacc, lw});
        }
      }
    }
    uint32_t hb[4], fb[4], o[4] = {0, 0, 0, 0};
    reduce16(hacc, hb);
    fprime16(facc, hb, ctn, fb);
    if (u != 0) {   // (uniform)
      uint32_t pk[4];
      kzgo::packed_powers(u, pk);
      const uint32_t tot = hf17::mod17(kzgo::dot16(fb, pk));   // (<= 16 x 16 x 16)
      kzgo::quotient16(fb, u, scan(tot), kzgo::PackInto{o});
    } else {
      // F' lives in registers only: the next thread's first byte comes by a shuffle, the next wave's through LDS
      uint32_t nxt = __shfl_down(fb[0] & 0xFFu, 1, PLK_WAVE);
      if (BLK) {
        if (lane == 0) red[2][wv] = fb[0] & 0xFFu;
        __syncthreads();
        if (lane == PLK_WAVE - 1) nxt = wv + 1 < kzgo::WAVES ? red[2][wv + 1] : 0u;
      } else if (lane == PLK_WAVE - 1) {
        nxt = 0;
      }
      kzgo::shift16(fb, nxt, kzgo::PackInto{o});
    }
    // [15:0] the share of W's sum, [31:16] of W''s
    const uint32_t s = plk_wave_sum(kzgo::dot16(l, hb) % ORD | (kzgo::dot16(l, o) % ORD) << 16);
    const bool anybad = __ballot(noncanon) != 0;
    if (!BLK) {
      if (lane < A.k) store_commit(A, e0 + lane, mine);
      if (lane == 0) store_group(A, g, true, anybad, s & 0xFFFFu, s >> 16);
    } else {
      if (lane == 0) {
        red[0][wv] = s;
        red[1][wv] = anybad ? 1u : 0u;
      }
      __syncthreads();   // psum and red are complete
      if (threadIdx.x < A.k) store_commit(A, e0 + threadIdx.x, psum[threadIdx.x][0] + psum[threadIdx.x][1] + psum[threadIdx.x][2] + psum[threadIdx.x][3]);
      if (threadIdx.x == 0) {
        const uint32_t sum = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        store_group(A, g, true, (red[1][0] | red[1][1] | red[1][2] | red[1][3]) != 0, sum & 0xFFFFu, sum >> 16);
      }
      __syncthreads();   // the next group writes psum and red only after these reads
    }
  }
}
static_assert(kzgo::WAVES == 4, "the block path adds four wave words");

struct Plan {
  int path;
  uint32_t per_block;   // groups a block takes per turn of its loop
  uint32_t blocks;
};

// arguments checked by the caller
Plan plan_of(uint64_t m, uint64_t ngroups) {
  Plan p{};
  p.path = m <= LANE_MAX ? PATH_LANE : m <= WAVE_MAX ? PATH_WAVE : PATH_BLOCK;
  p.per_block = p.path == PATH_LANE ? (uint32_t)kzgo::T : p.path == PATH_WAVE ? (uint32_t)kzgo::WAVES : 1u;
  p.blocks = (uint32_t)std::min<uint64_t>((ngroups + p.per_block - 1) / p.per_block, MULTI_BLOCKS);
  return p;
}

// PLK_OK, or the code every entry point returns for this shape (no handle, no device).  total: as the caller
// gave it, or m k ngroups for the plan of a uniform call
int check_shape(const char* fn, size_t m, size_t k, size_t ngroups, bool ragged, const size_t* total) {
  if (m == 0 || k == 0 || ngroups == 0 || (total && *total == 0)) {
    plk_set_error("%s: m > 0, k > 0, ngroups > 0 and total > 0 are required", fn);
    return PLK_ERR_ARG;
  }
  if (k > PLK_KZG_MULTI_MAX) {
    plk_set_error("%s: k = %zu exceeds PLK_KZG_MULTI_MAX = %d polynomials per group", fn, k, PLK_KZG_MULTI_MAX);
    return PLK_ERR_ARG;
  }
  if (m > PLK_KZG_FLAT_MAX) {
    plk_set_error("%s: m = %zu exceeds PLK_KZG_FLAT_MAX = %d coefficients per polynomial", fn, m, PLK_KZG_FLAT_MAX);
    return PLK_ERR_RANGE;
  }
  if ((uint64_t)ngroups > MAX_NPOLY / k) {   // (k ngroups > 2^30, without the product)
    plk_set_error("%s: k ngroups = %zu x %zu must stay within 2^30", fn, k, ngroups);
    return PLK_ERR_RANGE;
  }
  const uint64_t flat = (uint64_t)m * k * ngroups;   // (<= 2^12 x 2^30)
  if (total && !ragged && *total != flat) {
    plk_set_error("%s: m k ngroups == total is required without offsets (%zu x %zu x %zu != %zu)", fn, m, k, ngroups, *total);
    return PLK_ERR_ARG;
  }
  if ((total ? (uint64_t)*total : ragged ? 0ull : flat) >= MAX_TOTAL) {
    plk_set_error("%s: total = %llu must stay below 2^32", fn, (unsigned long long)(total ? *total : flat));
    return PLK_ERR_RANGE;
  }
  return PLK_OK;
}

// the checks of the two calls after the shape: pointers, the alignment of offsets and sets, the SRS bound on m as
// given, the device (no device query before the last)
int check_call(const char* fn, const plk_srs* s, bool null_ptr, const uint32_t* off, const uint32_t* sets, size_t m, bool commit) {
  if (!s || null_ptr) {
    plk_set_error("%s: the handle, the coefficient array, sets, weights, us and every required output are required", fn);
    return PLK_ERR_ARG;
  }
  if ((off && (uintptr_t)off % 4) || (sets && (uintptr_t)sets % 4)) {
    plk_set_error("%s: the offsets and the sets must be 4-byte aligned", fn);
    return PLK_ERR_ARG;
  }
  int rc;
  if (commit && (rc = plk_kzg_check_srs_len(s, m))) return rc;
  if ((rc = plk_kzg_check_srs_len(s, std::max<size_t>(m - 1, 1)))) return rc;
  return plk_kzg_check_device(fn, s);
}

// the one launch of a call, arguments checked
int launch_multi_flat(const plk_srs* s, const uint8_t* d_coeffs, size_t total, const uint32_t* d_off, size_t m, size_t k,
                      size_t ngroups, const uint32_t* d_sets, const uint8_t* d_weights, const uint8_t* d_us, uint8_t* d_ys,
                      uint8_t* d_proofs6, uint8_t* d_commits3, uint8_t* d_status, hipStream_t st) {
  MultiArgs A{};
  A.coeffs = d_coeffs;
  A.total = total;
  A.off = d_off;
  A.ngroups = ngroups;
  A.m = (uint32_t)m;
  A.k = (uint32_t)k;
  A.srs_bad = s->irregular ? 1u : 0u;
  A.sets = d_sets;
  A.weights = d_weights;
  A.us = d_us;
  A.logs = s->d_log;
  A.expw = s->exp_words;
  A.ys = d_ys;
  A.proofs6 = d_proofs6;
  A.commits3 = d_commits3;
  A.status = d_status;
  const Plan p = plan_of(m, ngroups);
  const dim3 grid(p.blocks), block(kzgo::T);
  if (p.path == PATH_LANE) {
    if (!d_off && m % kzgo::E == 0 && (uintptr_t)d_coeffs % 16 == 0)
      hipLaunchKernelGGL(multi_lane_kernel<true>, grid, block, 0, st, A);
    else
      hipLaunchKernelGGL(multi_lane_kernel<false>, grid, block, 0, st, A);
  } else if (p.path == PATH_WAVE) {
    hipLaunchKernelGGL(multi_wide_kernel<false>, grid, block, 0, st, A);
  } else {
    hipLaunchKernelGGL(multi_wide_kernel<true>, grid, block, 0, st, A);
  }
  PLK_HIP(hipGetLastError());
  return PLK_OK;
}

// the host form's own checks: every ragged polynomial non-empty, rising, inside total and within m; every mask
// valid; every u and every weight < 17
int check_host_lists(const char* fn, size_t total, const uint32_t* offsets, size_t m, size_t k, size_t ngroups,
                     const uint32_t* sets, const uint8_t* weights, const uint8_t* us) {
  const size_t npoly = k * ngroups;
  if (offsets) {
    for (size_t e = 0; e < npoly; e++) {
      const uint64_t a = offsets[e], b = offsets[e + 1];
      if (!(a < b && b <= total && b - a <= m)) {
        plk_set_error("%s: polynomial %zu = bytes [%u, %u) is empty, falls, leaves total = %zu or exceeds m = %zu", fn, e,
                      offsets[e], offsets[e + 1], total, m);
        return PLK_ERR_ARG;
      }
    }
  }
  for (size_t g = 0; g < ngroups; g++) {
    if (us[g] >= HFP) {
      plk_set_error("%s: group %zu: u = %u is not a GF(17) value", fn, g, (unsigned)us[g]);
      return PLK_ERR_ARG;
    }
  }
  for (size_t e = 0; e < npoly; e++) {
    if (!mask_ok(sets[e])) {
      plk_set_error("%s: polynomial %zu: the set 0x%x is not 1 .. %d points of GF(17)", fn, e, (unsigned)sets[e], PLK_KZG_MULTI_POINTS);
      return PLK_ERR_ARG;
    }
    if (weights[e] >= HFP) {
      plk_set_error("%s: polynomial %zu: weight = %u is not a GF(17) value", fn, e, (unsigned)weights[e]);
      return PLK_ERR_ARG;
    }
  }
  return PLK_OK;
}

// The host-buffer form: the arrays uploaded on 16-byte boundaries, the one launch, the read-back; every flagged
// group (a byte >= 17, every group of an irregular SRS) recomputed through plk_kzg_open_multi_batch /
// plk_kzg_commit_batch, RECOMP groups at a time.
int host_multi_flat(const char* fn, const plk_srs* s, const uint8_t* coeffs, size_t total, const uint32_t* offsets, size_t m,
                    size_t k, size_t ngroups, const uint32_t* sets, const uint8_t* weights, const uint8_t* us, uint8_t* ys,
                    uint8_t* proofs6, uint8_t* commits3) {
  const size_t npoly = k * ngroups;
  std::vector<uint8_t> status(ngroups, (uint8_t)PLK_KZG_FLAT_IRREGULAR);
  if (!s->irregular) {
    const size_t ob = offsets ? 4 * (npoly + 1) : 0;
    const size_t o_off = plk_pad16(total), o_set = o_off + plk_pad16(ob), o_w = o_set + plk_pad16(4 * npoly), o_us = o_w + plk_pad16(npoly),
                 o_ys = o_us + plk_pad16(ngroups), o_st = o_ys + plk_pad16(NPTS * npoly), o_pr = o_st + plk_pad16(ngroups),
                 o_cm = o_pr + plk_pad16(6 * ngroups), bytes = o_cm + plk_pad16(3 * npoly);
    PlkScratch D;
    int rc = D.alloc(fn, bytes);
    if (rc) return rc;
    PLK_HIP(hipMemcpyAsync(D.d, coeffs, total, hipMemcpyHostToDevice, s->st));
    if (offsets) PLK_HIP(hipMemcpyAsync(D.d + o_off, offsets, ob, hipMemcpyHostToDevice, s->st));
    PLK_HIP(hipMemcpyAsync(D.d + o_set, sets, 4 * npoly, hipMemcpyHostToDevice, s->st));
    PLK_HIP(hipMemcpyAsync(D.d + o_w, weights, npoly, hipMemcpyHostToDevice, s->st));
    PLK_HIP(hipMemcpyAsync(D.d + o_us, us, ngroups, hipMemcpyHostToDevice, s->st));
    if ((rc = launch_multi_flat(s, D.d, total, offsets ? (const uint32_t*)(D.d + o_off) : nullptr, m, k, ngroups,
                                (const uint32_t*)(D.d + o_set), D.d + o_w, D.d + o_us, D.d + o_ys, D.d + o_pr,
                                commits3 ? D.d + o_cm : nullptr, D.d + o_st, s->st)))
      return rc;
    PLK_HIP(hipMemcpyAsync(status.data(), D.d + o_st, ngroups, hipMemcpyDeviceToHost, s->st));
    PLK_HIP(hipMemcpyAsync(ys, D.d + o_ys, NPTS * npoly, hipMemcpyDeviceToHost, s->st));
    PLK_HIP(hipMemcpyAsync(proofs6, D.d + o_pr, 6 * ngroups, hipMemcpyDeviceToHost, s->st));
    if (commits3) PLK_HIP(hipMemcpyAsync(commits3, D.d + o_cm, 3 * npoly, hipMemcpyDeviceToHost, s->st));
    PLK_HIP(hipStreamSynchronize(s->st));
  }
  constexpr size_t RECOMP = 64;   // groups a batch (<= 960 polynomials)
  std::vector<size_t> idx;
  std::vector<const uint8_t*> pp;
  std::vector<size_t> ll;
  std::vector<int> start;
  std::vector<uint32_t> mm;
  std::vector<uint8_t> ww, uu, yy, g6, g3;
  auto flush = [&]() -> int {
    if (idx.empty()) return PLK_OK;
    const int n = (int)idx.size(), np = (int)pp.size();
    int rc;
    start.resize(n + 1);
    for (int r = 0; r <= n; r++) start[r] = r * (int)k;
    yy.resize(NPTS * (size_t)np);
    g6.resize(6 * (size_t)n);
    if ((rc = plk_kzg_open_multi_batch(s, pp.data(), ll.data(), mm.data(), ww.data(), start.data(), uu.data(), n, yy.data(), g6.data())))
      return rc;
    for (int r = 0; r < n; r++) {
      memcpy(ys + NPTS * k * idx[r], &yy[NPTS * k * (size_t)r], NPTS * k);
      memcpy(proofs6 + 6 * idx[r], &g6[6 * (size_t)r], 6);
    }
    // (a flagged group's commitments are exact unless the SRS is irregular)
    if (commits3 && s->irregular) {
      g3.resize(3 * (size_t)np);
      if ((rc = plk_kzg_commit_batch(s, pp.data(), ll.data(), np, g3.data()))) return rc;
      for (int r = 0; r < n; r++) memcpy(commits3 + 3 * k * idx[r], &g3[3 * k * (size_t)r], 3 * k);
    }
    idx.clear();
    pp.clear();
    ll.clear();
    mm.clear();
    ww.clear();
    uu.clear();
    return PLK_OK;
  };
  for (size_t g = 0; g < ngroups; g++) {
    if (status[g] == 0) continue;
    if (status[g] != PLK_KZG_FLAT_IRREGULAR) {
      plk_set_error("%s: group %zu came back with status %u", fn, g, (unsigned)status[g]);
      return PLK_ERR_HIP;
    }
    idx.push_back(g);
    uu.push_back(us[g]);
    for (size_t e = k * g; e < k * (g + 1); e++) {
      const size_t lo = offsets ? offsets[e] : e * m, len = offsets ? offsets[e + 1] - lo : m;
      pp.push_back(coeffs + lo);
      ll.push_back(len);
      mm.push_back(sets[e]);
      ww.push_back(weights[e]);
    }
    int rc;
    if (idx.size() == RECOMP && (rc = flush())) return rc;
  }
  return flush();
}

}  // namespace

extern "C" {

int plk_kzg_multi_flat_plan(size_t m, size_t k, size_t ngroups, int ragged, int64_t out[4]) {
  const char* fn = "plk_kzg_multi_flat_plan";
  if (!out) {
    plk_set_error("%s: out is required", fn);
    return PLK_ERR_ARG;
  }
  const int rc = check_shape(fn, m, k, ngroups, ragged != 0, nullptr);
  if (rc) return rc;
  const Plan p = plan_of(m, ngroups);
  out[0] = p.path;
  out[1] = p.per_block;
  out[2] = p.blocks;
  out[3] = 1;
  return PLK_OK;
}

int plk_kzg_open_multi_flat_dev(const plk_srs_t* s, const uint8_t* d_coeffs, size_t total, const uint32_t* d_offsets, size_t m,
                                size_t k, size_t ngroups, const uint32_t* d_sets, const uint8_t* d_weights, const uint8_t* d_us,
                                uint8_t* d_ys, uint8_t* d_proofs6, uint8_t* d_commits3, uint8_t* d_status, void* stream) {
  const char* fn = "plk_kzg_open_multi_flat_dev";
  int rc = check_shape(fn, m, k, ngroups, d_offsets != nullptr, &total);
  if (rc || (rc = check_call(fn, s, !d_coeffs || !d_sets || !d_weights || !d_us || !d_ys || !d_proofs6 || !d_status, d_offsets,
                             d_sets, m, d_commits3 != nullptr)))
    return rc;
  return launch_multi_flat(s, d_coeffs, total, d_offsets, m, k, ngroups, d_sets, d_weights, d_us, d_ys, d_proofs6, d_commits3,
                           d_status, (hipStream_t)stream);
}

int plk_kzg_open_multi_flat(const plk_srs_t* s, const uint8_t* coeffs, size_t total, const uint32_t* offsets, size_t m, size_t k,
                            size_t ngroups, const uint32_t* sets, const uint8_t* weights, const uint8_t* us, uint8_t* ys,
                            uint8_t* proofs6, uint8_t* commits3) {
  const char* fn = "plk_kzg_open_multi_flat";
  int rc = check_shape(fn, m, k, ngroups, offsets != nullptr, &total);
  if (rc) return rc;
  if (!s || !coeffs || !sets || !weights || !us || !ys || !proofs6) {
    plk_set_error("%s: the handle, coeffs, sets, weights, us, ys and proofs6 are required", fn);
    return PLK_ERR_ARG;
  }
  if ((rc = check_host_lists(fn, total, offsets, m, k, ngroups, sets, weights, us)) ||
      (rc = check_call(fn, s, false, nullptr, nullptr, m, commits3 != nullptr)))
    return rc;
  return host_multi_flat(fn, s, coeffs, total, offsets, m, k, ngroups, sets, weights, us, ys, proofs6, commits3);
}

}  // extern "C"
