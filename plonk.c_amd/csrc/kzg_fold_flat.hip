// KZG flat folded openings (include/plonkhip.h, "KZG flat folded openings"): very many GROUPS of short
// polynomials, each group opened at one point with one proof under per-polynomial weights, in one launch --
// the producer at the scale of plk_kzg_verify_fold_batch_dev.  Polynomial e is the bytes [o_e, o_{e+1}) of ONE
// flat coefficient array exactly as in kzg_flat.hip; group g owns polynomials, weights and ys [k g, k (g + 1))
// and the one device byte zs[g].
//
// The arithmetic is kzg.hip's kzg_fold_open_kernel with one chunk and nothing to finish across blocks, as
// kzg_flat.hip is to kzg_open_kernel: F[j] = sum_i w_i p_i[j] is summed exactly per coefficient (<= 16 x 16 x
// 255 = 65280, inside mod17's range), reduced once, and F's sixteen canonical bytes go through the unchanged
// pieces of plk_kzg_open.h.  F never reaches memory.  y_i and the commitment sum of polynomial i come from its
// own bytes while they are in registers.  Three paths, a function of m alone (plk_kzg_fold_flat_plan), each
// ONE launch with a grid-stride loop over the groups:
//   lane   m <= 32: one lane per group.  Polynomial by polynomial the lane adds the weighted bytes of both
//          halves of sixteen coefficients into 32 sums; then F's halves from the top down through quotient16,
//          the running top quotient byte handed from the upper half to the lower (z = 0 is no special case).
//          The block holds the first 32 SRS logs in LDS.
//   wave   32 < m <= 1024: one wave per group, sixteen coefficients per lane.  Per polynomial one load, the
//          weighted accumulate and ONE wave sum of (y share | commitment share << 16); then one wave_suffix and
//          one quotient for F.  Lanes i < k store y_i and commitment i.  No LDS, no barrier.
//   block  1024 < m <= 4096: one block per group: the wave path's sums as four wave words through LDS,
//          kzgo::suffix_carry with one chunk.
// Polynomials are taken one at a time (no tile of loads held in registers), so no kernel depends on k and none
// spills at k = 16.  Plain stores only: no workspace, no atomics, no record, every word read was written by the
// caller, and every sum is an integer, so the bytes do not depend on any order.
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
constexpr uint32_t LANE_MAX = 32;                        // m <= : the lane path
constexpr uint32_t WAVE_MAX = PLK_WAVE * kzgo::E;        // m <= : the wave path (1024)
constexpr uint32_t FOLD_BLOCKS = 2048;                   // grid cap of every path (grid-stride loops)
constexpr uint64_t MAX_TOTAL = 1ull << 32, MAX_NPOLY = 1ull << 30;
constexpr uint32_t G1_FLAGGED = 0xFFFFFFu;               // bytes FF FF FF
static_assert(PLK_KZG_FLAT_MAX == kzgo::CHUNK, "a polynomial is one chunk of the opening family");
static_assert(WAVE_MAX == 1024 && LANE_MAX == 2 * kzgo::E, "the paths' bounds as the header states them");
static_assert(PLK_KZG_FOLD_MAX <= kzgo::E, "lanes i < k of one wave store the group's ys and commitments");
// F's coefficient before its one reduction: k weights < 17 on bytes <= 255
static_assert((uint32_t)PLK_KZG_FOLD_MAX * 16u * 255u < hf17::MOD17_BOUND, "sum_i w_i byte stays inside mod17's range");
// a wave sum carries a polynomial's y share in [15:0] and its commitment share in [31:16]: 64 lanes of a value
// < 17 and of a value < 102 (the block path adds four such words: 256 lanes)
static_assert(256u * 16u < (1u << 16) && 256u * 101u < (1u << 16), "the two halves of a packed sum do not meet");
// the lane path adds two unreduced dot16s against logs (<= 32 x 255 x 101) and two against powers (<= 32 x 255 x 16)
static_assert(2ull * 16 * 255 * 101 < (1ull << 32), "the lane path's sums fit 32 bits");

enum { PATH_LANE = 0, PATH_WAVE = 1, PATH_BLOCK = 2 };

struct FoldArgs {
  const uint8_t* coeffs;
  uint64_t total;
  const uint32_t* off;      // k ngroups + 1 words, or nullptr: o_e = e m
  uint64_t ngroups;
  uint32_t m, k;
  uint32_t srs_bad;         // the SRS has no log form: every G1 output is flagged, ys stay exact
  const uint8_t* weights;   // k ngroups
  const uint8_t* zs;        // ngroups
  const uint8_t* logs;      // the SRS logs, zero padded (plk_kzg_host.h)
  const uint32_t* expw;     // the 102 EXP words {x, y, infinite, 0}
  uint8_t *ys, *proofs3;
  uint8_t* commits3;        // or nullptr
  uint8_t* status;
};

// Polynomial e: its first byte and length.  Offsets are read as min(o, total), so no value makes a caller of
// this read outside [0, total); false for a ragged polynomial that is empty, falls, has an offset above total
// or is longer than m.
__device__ __forceinline__ bool segment_of(const FoldArgs& A, uint64_t e, uint64_t& lo, uint32_t& len) {
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

// Group g before any coefficient is read: false (PLK_KZG_FLAT_BAD) when one of its segments is broken or its z
// byte or one of its weight bytes is >= 17; L: the longest polynomial.  Every thread of a wave or block that
// shares g reads the same bytes, so the answer is uniform there.
__device__ __forceinline__ bool group_of(const FoldArgs& A, uint64_t g, uint32_t& z, uint32_t& L) {
  const uint64_t e0 = g * A.k;
  const uint32_t zb = A.zs[g];
  bool ok = zb < HFP;
  z = ok ? zb : 0u;
  L = A.off ? 0u : A.m;
  for (uint32_t i = 0; i < A.k; i++) {
    ok = ok && A.weights[e0 + i] < HFP;
    if (A.off) {
      uint64_t lo;
      uint32_t len;
      ok = segment_of(A, e0 + i, lo, len) && ok;
      L = max(L, len);
    }
  }
  return ok;
}

__device__ __forceinline__ void store_g1(uint8_t* out3, uint64_t e, uint32_t v) {
  out3[3 * e] = (uint8_t)v;
  out3[3 * e + 1] = (uint8_t)(v >> 8);
  out3[3 * e + 2] = (uint8_t)(v >> 16);
}

// polynomial e of a valid group: y and the commitment, which is exact for any coefficient byte (g1_mul takes the
// raw byte); sp: sum p_j log_j (any multiple of 102 on top)
__device__ __forceinline__ void store_poly(const FoldArgs& A, uint64_t e, uint32_t y, uint32_t sp) {
  A.ys[e] = (uint8_t)y;
  if (A.commits3) store_g1(A.commits3, e, A.srs_bad ? G1_FLAGGED : A.expw[sp % ORD]);
}
// polynomial e of a PLK_KZG_FLAT_BAD group
__device__ __forceinline__ void store_poly_bad(const FoldArgs& A, uint64_t e) {
  A.ys[e] = 0xFF;
  if (A.commits3) store_g1(A.commits3, e, G1_FLAGGED);
}
// group g's status and proof; sq: sum q_j log_j of F's quotient
__device__ __forceinline__ void store_group(const FoldArgs& A, uint64_t g, bool ok, bool noncanon, uint32_t sq) {
  const uint32_t st = !ok ? (uint32_t)PLK_KZG_FLAT_BAD : (A.srs_bad || noncanon) ? (uint32_t)PLK_KZG_FLAT_IRREGULAR : 0u;
  A.status[g] = (uint8_t)st;
  store_g1(A.proofs3, g, st ? G1_FLAGGED : A.expw[sq % ORD]);
}

// acc[j] += w x byte j of nb: per-byte multiply-adds on genuine bytes (<= 16 x 255 a term)
__device__ __forceinline__ void weighted_add(const uint32_t (&nb)[4], uint32_t w, uint32_t (&acc)[kzgo::E]) {
#pragma unroll
  for (int j = 0; j < kzgo::E; j++) acc[j] += w * hf17::byte_of(nb, j);
}
// F's sixteen canonical bytes from their exact sums (each <= 65280)
__device__ __forceinline__ void reduce16(const uint32_t (&acc)[kzgo::E], uint32_t (&nb)[4]) {
  nb[0] = nb[1] = nb[2] = nb[3] = 0;
#pragma unroll
  for (int j = 0; j < kzgo::E; j++) nb[j >> 2] |= hf17::mod17(acc[j]) << (8 * (j & 3));
}

// lane path: see the head of this file.  VEC (uniform, m a multiple of 16, coefficients 16-byte aligned):
// every polynomial is as aligned as the array.
template <bool VEC>
__global__ __launch_bounds__(kzgo::T) void fold_lane_kernel(FoldArgs A) {
  __shared__ __attribute__((aligned(16))) uint32_t slog[LANE_MAX / 4];   // the first 32 SRS logs, four to a word
  if (threadIdx.x < LANE_MAX / 4)
    slog[threadIdx.x] = A.srs_bad ? 0u : reinterpret_cast<const uint32_t*>(A.logs)[threadIdx.x];   // (>= 32 bytes, zero padded)
  __syncthreads();
  const bool commit = A.commits3 != nullptr;
  for (uint64_t g = (uint64_t)blockIdx.x * kzgo::T + threadIdx.x; g < A.ngroups; g += (uint64_t)gridDim.x * kzgo::T) {
    const uint64_t e0 = g * A.k;
    uint32_t z, L;
    if (!group_of(A, g, z, L)) {
      for (uint32_t i = 0; i < A.k; i++) store_poly_bad(A, e0 + i);
      store_group(A, g, false, false, 0);
      continue;
    }
    uint32_t pk[4], l[2][4];
    kzgo::packed_powers(z, pk);
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const uint4 lv = *reinterpret_cast<const uint4*>(&slog[4 * h]);
      l[h][0] = lv.x; l[h][1] = lv.y; l[h][2] = lv.z; l[h][3] = lv.w;
    }
    uint32_t acc[2][kzgo::E];
#pragma unroll
    for (int j = 0; j < kzgo::E; j++) acc[0][j] = acc[1][j] = 0;
    bool noncanon = false;
    for (uint32_t i = 0; i < A.k; i++) {
      uint64_t lo;
      uint32_t len;
      (void)segment_of(A, e0 + i, lo, len);
      const uint8_t* p = A.coeffs + lo;
      const uint32_t w = A.weights[e0 + i];
      uint32_t yv = 0, sp = 0;
#pragma unroll
      for (int h = 0; h < 2; h++) {
        if (16u * h < len) {
          uint32_t nb[4];
          if (VEC) kzgo::load16_vec(p, 16u * h, nb);
          else kzgo::load16_rolled(p, len, 16u * h, nb);
          noncanon |= hf17::any_noncanonical(nb);
          weighted_add(nb, w, acc[h]);
          // z^16 = 1 needs z != 0; at z = 0 the powers are {1, 0, ..}, so the lower half alone gives p[0]
          if (h == 0 || z != 0) yv += kzgo::dot16(nb, pk);   // (<= 16 x 255 x 16 a half)
          if (commit) sp += kzgo::dot16(l[h], nb);           // (<= 16 x 101 x 255 a half)
        }
      }
      store_poly(A, e0 + i, yv % HFP, sp);
    }
    // F from the top half down: q[16 h + 15] = run, q[j] = F[j + 1] + z q[j + 1] below it; then the byte above
    // the next half, q[16 h - 1] = F[16 h] + z q[16 h]
    uint32_t run = 0, sq = 0;
#pragma unroll
    for (int h = 1; h >= 0; h--) {
      if (16u * h < L) {
        uint32_t nb[4], o[4] = {0, 0, 0, 0};
        reduce16(acc[h], nb);
        kzgo::quotient16(nb, z, run, kzgo::PackInto{o});
        sq += kzgo::dot16(l[h], o);
        run = (nb[0] & 0xFFu) + z * (o[0] & 0xFFu);
      }
    }
    store_group(A, g, true, noncanon, sq);
  }
}

// The sixteen coefficients [base, base + 16) of a polynomial of len bytes at p, zero past len
__device__ __forceinline__ void load_run(const uint8_t* p, uint32_t len, uint32_t base, uint32_t (&nb)[4]) {
  if (kzgo::aligned16(p) && base + 16 <= len)
    kzgo::load16_vec(p, base, nb);
  else
    kzgo::load16_rolled(p, len, base, nb);
}

// One polynomial of the wave and block paths: its run loaded, its weighted bytes added into acc, and the
// thread's share of its two sums packed for ONE reduction: [15:0] the share of p_i(z) (< 17), [31:16] the share
// of its commitment sum (< 102).
__device__ __forceinline__ uint32_t fold_poly(const FoldArgs& A, uint64_t e, uint32_t base, uint32_t z, const uint32_t (&pk)[4],
                                              const uint32_t (&l)[4], uint32_t (&acc)[kzgo::E], bool& noncanon) {
  uint64_t lo;
  uint32_t len, nb[4];
  (void)segment_of(A, e, lo, len);
  load_run(A.coeffs + lo, len, base, nb);
  noncanon |= hf17::any_noncanonical(nb);
  weighted_add(nb, A.weights[e], acc);
  uint32_t v = hf17::mod17(kzgo::dot16(nb, pk));   // (<= 16 x 255 x 16)
  if (z == 0 && base != 0) v = 0;                  // z^16 = 1 needs z != 0: p(0) = p[0], thread 0's
  if (A.commits3) v |= (kzgo::dot16(l, nb) % ORD) << 16;
  return v;
}

// The thread's sixteen quotient bytes o once it holds F's bytes nb and run = the aggregates of the threads
// after it (z != 0).  z = 0: the thread's last quotient byte is F[base + 16], folded here from the polynomials'
// own bytes (the next thread's first coefficient), as kzg_fold_open_kernel does.
__device__ __forceinline__ void fold_quotient(const FoldArgs& A, uint64_t e0, uint32_t base, const uint32_t (&nb)[4], uint32_t z,
                                              uint32_t run, uint32_t (&o)[4]) {
  o[0] = o[1] = o[2] = o[3] = 0;
  if (z != 0) {
    kzgo::quotient16(nb, z, run, kzgo::PackInto{o});
    return;
  }
  uint32_t sn = 0;   // (<= 65280)
  for (uint32_t i = 0; i < A.k; i++) {
    uint64_t lo;
    uint32_t len;
    (void)segment_of(A, e0 + i, lo, len);
    if (base + 16 < len) sn += (uint32_t)A.weights[e0 + i] * A.coeffs[lo + base + 16];
  }
  kzgo::shift16(nb, hf17::mod17(sn), kzgo::PackInto{o});
}

// wave path: see the head of this file.  Group g is wave-uniform, so every branch on it is.
__global__ __launch_bounds__(kzgo::T) void fold_wave_kernel(FoldArgs A) {
  const uint32_t lane = threadIdx.x & (PLK_WAVE - 1), base = lane * kzgo::E;
  for (uint64_t g = (uint64_t)blockIdx.x * kzgo::WAVES + threadIdx.x / PLK_WAVE; g < A.ngroups;
       g += (uint64_t)gridDim.x * kzgo::WAVES) {
    const uint64_t e0 = g * A.k;
    uint32_t z, L;
    const bool ok = group_of(A, g, z, L);
    if (!ok) {   // (uniform)
      if (lane < A.k) store_poly_bad(A, e0 + lane);
      if (lane == 0) store_group(A, g, false, false, 0);
      continue;
    }
    z = (uint32_t)__builtin_amdgcn_readfirstlane((int)z);   // (every lane read the same byte)
    uint32_t pk[4], acc[kzgo::E];
    kzgo::packed_powers(z, pk);
    const uint4 lg = kzgo::Finish::logs(A.logs, A.srs_bad, base, L);
    const uint32_t l[4] = {lg.x, lg.y, lg.z, lg.w};
#pragma unroll
    for (int j = 0; j < kzgo::E; j++) acc[j] = 0;
    bool noncanon = false;
    uint32_t mine = 0;   // lane i: polynomial i's packed sums
    for (uint32_t i = 0; i < A.k; i++) {   // (uniform)
      const uint32_t s = plk_wave_sum(fold_poly(A, e0 + i, base, z, pk, l, acc, noncanon));
      if (lane == i) mine = s;
    }
    noncanon = __ballot(noncanon) != 0;
    uint32_t nb[4], o[4];
    reduce16(acc, nb);
    const uint32_t tot = hf17::mod17(kzgo::dot16(nb, pk));   // (<= 16 x 16 x 16)
    const uint32_t run = hf17::wave_suffix(tot) - tot;       // the later lanes' aggregates (<= 63 x 16)
    fold_quotient(A, e0, base, nb, z, run, o);
    const uint32_t sq = plk_wave_sum(kzgo::dot16(l, o) % ORD);   // (the sum <= 64 x 101)
    if (lane < A.k) store_poly(A, e0 + lane, (mine & 0xFFFFu) % HFP, mine >> 16);
    if (lane == 0) store_group(A, g, true, noncanon, sq);
  }
}

// block path: see the head of this file.  Two barriers a group (suffix_carry's, which also orders psum, and the
// reduction's), so the LDS words of one group are read before the next one's are written.
__global__ __launch_bounds__(kzgo::T) void fold_block_kernel(FoldArgs A) {
  __shared__ uint32_t ws[2 * kzgo::WAVES];
  __shared__ uint32_t psum[PLK_KZG_FOLD_MAX][kzgo::WAVES];   // per polynomial and wave: the packed sums
  __shared__ uint32_t red[2][kzgo::WAVES];                   // per wave: sum q log, a byte >= 17
  const uint32_t base = threadIdx.x * kzgo::E, wv = threadIdx.x / PLK_WAVE, lane = threadIdx.x & (PLK_WAVE - 1);
  for (uint64_t g = blockIdx.x; g < A.ngroups; g += gridDim.x) {   // (uniform)
    const uint64_t e0 = g * A.k;
    uint32_t z, L;
    if (!group_of(A, g, z, L)) {   // (uniform)
      if (threadIdx.x < A.k) store_poly_bad(A, e0 + threadIdx.x);
      if (threadIdx.x == 0) store_group(A, g, false, false, 0);
      continue;
    }
    uint32_t pk[4], acc[kzgo::E];
    kzgo::packed_powers(z, pk);
    const uint4 lg = kzgo::Finish::logs(A.logs, A.srs_bad, base, L);
    const uint32_t l[4] = {lg.x, lg.y, lg.z, lg.w};
#pragma unroll
    for (int j = 0; j < kzgo::E; j++) acc[j] = 0;
    bool noncanon = false;
    for (uint32_t i = 0; i < A.k; i++) {   // (uniform)
      const uint32_t s = plk_wave_sum(fold_poly(A, e0 + i, base, z, pk, l, acc, noncanon));
      if (lane == 0) psum[i][wv] = s;
    }
    const uint32_t anybad = __ballot(noncanon) != 0 ? 1u : 0u;
    uint32_t nb[4], o[4];
    reduce16(acc, nb);
    const uint32_t tot = hf17::mod17(kzgo::dot16(nb, pk));   // (<= 16 x 16 x 16)
    bool unused = false;
    const uint32_t run = kzgo::suffix_carry(tot, nullptr, 0u, 1u, ws, unused);   // no other chunk: the block's exclusive suffix sum
    fold_quotient(A, e0, base, nb, z, run, o);
    const uint32_t sq = plk_wave_sum(kzgo::dot16(l, o) % ORD);
    // (psum is complete: suffix_carry held a barrier)
    if (threadIdx.x < A.k) {
      const uint32_t s = psum[threadIdx.x][0] + psum[threadIdx.x][1] + psum[threadIdx.x][2] + psum[threadIdx.x][3];
      store_poly(A, e0 + threadIdx.x, (s & 0xFFFFu) % HFP, s >> 16);
    }
    if (lane == 0) {
      red[0][wv] = sq;
      red[1][wv] = anybad;
    }
    __syncthreads();
    if (threadIdx.x == 0)
      store_group(A, g, true, (red[1][0] | red[1][1] | red[1][2] | red[1][3]) != 0, red[0][0] + red[0][1] + red[0][2] + red[0][3]);
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
  p.blocks = (uint32_t)std::min<uint64_t>((ngroups + p.per_block - 1) / p.per_block, FOLD_BLOCKS);
  return p;
}

// PLK_OK, or the code every entry point returns for this shape (no handle, no device).  total: as the caller
// gave it, or m k ngroups for the plan of a uniform call
int check_shape(const char* fn, size_t m, size_t k, size_t ngroups, bool ragged, const size_t* total) {
  if (m == 0 || k == 0 || ngroups == 0 || (total && *total == 0)) {
    plk_set_error("%s: m > 0, k > 0, ngroups > 0 and total > 0 are required", fn);
    return PLK_ERR_ARG;
  }
  if (k > PLK_KZG_FOLD_MAX) {
    plk_set_error("%s: k = %zu exceeds PLK_KZG_FOLD_MAX = %d polynomials per group", fn, k, PLK_KZG_FOLD_MAX);
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

// the checks of the two calls after the shape: pointers, the offsets' alignment, the SRS bound on m as given,
// the device (no device query before the last)
int check_call(const char* fn, const plk_srs* s, bool null_ptr, const uint32_t* off, size_t m, bool commit) {
  if (!s || null_ptr) {
    plk_set_error("%s: the handle, the coefficient array, weights, zs and every required output are required", fn);
    return PLK_ERR_ARG;
  }
  if (off && (uintptr_t)off % 4) {
    plk_set_error("%s: the offsets must be 4-byte aligned", fn);
    return PLK_ERR_ARG;
  }
  int rc;
  if (commit && (rc = plk_kzg_check_srs_len(s, m))) return rc;
  if ((rc = plk_kzg_check_srs_len(s, std::max<size_t>(m - 1, 1)))) return rc;
  return plk_kzg_check_device(fn, s);
}

// the one launch of a call, arguments checked
int launch_fold(const plk_srs* s, const uint8_t* d_coeffs, size_t total, const uint32_t* d_off, size_t m, size_t k, size_t ngroups,
                const uint8_t* d_weights, const uint8_t* d_zs, uint8_t* d_ys, uint8_t* d_proofs3, uint8_t* d_commits3,
                uint8_t* d_status, hipStream_t st) {
  FoldArgs A{};
  A.coeffs = d_coeffs;
  A.total = total;
  A.off = d_off;
  A.ngroups = ngroups;
  A.m = (uint32_t)m;
  A.k = (uint32_t)k;
  A.srs_bad = s->irregular ? 1u : 0u;
  A.weights = d_weights;
  A.zs = d_zs;
  A.logs = s->d_log;
  A.expw = s->exp_words;
  A.ys = d_ys;
  A.proofs3 = d_proofs3;
  A.commits3 = d_commits3;
  A.status = d_status;
  const Plan p = plan_of(m, ngroups);
  const dim3 grid(p.blocks), block(kzgo::T);
  if (p.path == PATH_LANE) {
    if (!d_off && m % kzgo::E == 0 && (uintptr_t)d_coeffs % 16 == 0)
      hipLaunchKernelGGL(fold_lane_kernel<true>, grid, block, 0, st, A);
    else
      hipLaunchKernelGGL(fold_lane_kernel<false>, grid, block, 0, st, A);
  } else if (p.path == PATH_WAVE) {
    hipLaunchKernelGGL(fold_wave_kernel, grid, block, 0, st, A);
  } else {
    hipLaunchKernelGGL(fold_block_kernel, grid, block, 0, st, A);
  }
  PLK_HIP(hipGetLastError());
  return PLK_OK;
}

// the host form's own checks: every ragged polynomial non-empty, rising, inside total and within m; every z and
// every weight < 17
int check_host_lists(const char* fn, size_t total, const uint32_t* offsets, size_t m, size_t k, size_t ngroups,
                     const uint8_t* weights, const uint8_t* zs) {
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
    if (zs[g] >= HFP) {
      plk_set_error("%s: group %zu: z = %u is not a GF(17) value", fn, g, (unsigned)zs[g]);
      return PLK_ERR_ARG;
    }
  }
  for (size_t e = 0; e < npoly; e++) {
    if (weights[e] >= HFP) {
      plk_set_error("%s: polynomial %zu: weight = %u is not a GF(17) value", fn, e, (unsigned)weights[e]);
      return PLK_ERR_ARG;
    }
  }
  return PLK_OK;
}

// The host-buffer form: the arrays uploaded on 16-byte boundaries, the one launch, the read-back; every flagged
// group (a byte >= 17, every group of an irregular SRS) recomputed through plk_kzg_open_fold_batch /
// plk_kzg_commit_batch, RECOMP groups at a time.
int host_fold(const char* fn, const plk_srs* s, const uint8_t* coeffs, size_t total, const uint32_t* offsets, size_t m, size_t k,
              size_t ngroups, const uint8_t* weights, const uint8_t* zs, uint8_t* ys, uint8_t* proofs3, uint8_t* commits3) {
  const size_t npoly = k * ngroups;
  std::vector<uint8_t> status(ngroups, (uint8_t)PLK_KZG_FLAT_IRREGULAR);
  if (!s->irregular) {
    const size_t ob = offsets ? 4 * (npoly + 1) : 0;
    const size_t o_off = plk_pad16(total), o_w = o_off + plk_pad16(ob), o_zs = o_w + plk_pad16(npoly), o_ys = o_zs + plk_pad16(ngroups),
                 o_st = o_ys + plk_pad16(npoly), o_pr = o_st + plk_pad16(ngroups), o_cm = o_pr + plk_pad16(3 * ngroups),
                 bytes = o_cm + plk_pad16(3 * npoly);
    PlkScratch D;
    int rc = D.alloc(fn, bytes);
    if (rc) return rc;
    PLK_HIP(hipMemcpyAsync(D.d, coeffs, total, hipMemcpyHostToDevice, s->st));
    if (offsets) PLK_HIP(hipMemcpyAsync(D.d + o_off, offsets, ob, hipMemcpyHostToDevice, s->st));
    PLK_HIP(hipMemcpyAsync(D.d + o_w, weights, npoly, hipMemcpyHostToDevice, s->st));
    PLK_HIP(hipMemcpyAsync(D.d + o_zs, zs, ngroups, hipMemcpyHostToDevice, s->st));
    if ((rc = launch_fold(s, D.d, total, offsets ? (const uint32_t*)(D.d + o_off) : nullptr, m, k, ngroups, D.d + o_w, D.d + o_zs,
                          D.d + o_ys, D.d + o_pr, commits3 ? D.d + o_cm : nullptr, D.d + o_st, s->st)))
      return rc;
    PLK_HIP(hipMemcpyAsync(status.data(), D.d + o_st, ngroups, hipMemcpyDeviceToHost, s->st));
    PLK_HIP(hipMemcpyAsync(ys, D.d + o_ys, npoly, hipMemcpyDeviceToHost, s->st));
    PLK_HIP(hipMemcpyAsync(proofs3, D.d + o_pr, 3 * ngroups, hipMemcpyDeviceToHost, s->st));
    if (commits3) PLK_HIP(hipMemcpyAsync(commits3, D.d + o_cm, 3 * npoly, hipMemcpyDeviceToHost, s->st));
    PLK_HIP(hipStreamSynchronize(s->st));
  }
  constexpr size_t RECOMP = 64;   // groups a batch (<= 1024 polynomials)
  std::vector<size_t> idx;
  std::vector<const uint8_t*> pp;
  std::vector<size_t> ll;
  std::vector<int> start;
  std::vector<uint8_t> ww, zz, yy, g3;
  auto flush = [&]() -> int {
    if (idx.empty()) return PLK_OK;
    const int n = (int)idx.size(), np = (int)pp.size();
    int rc;
    start.resize(n + 1);
    for (int r = 0; r <= n; r++) start[r] = r * (int)k;
    yy.resize(np);
    g3.resize(3 * (size_t)np);
    if ((rc = plk_kzg_open_fold_batch(s, pp.data(), ll.data(), ww.data(), start.data(), zz.data(), n, yy.data(), g3.data()))) return rc;
    for (int r = 0; r < n; r++) {
      memcpy(ys + k * idx[r], &yy[k * (size_t)r], k);
      memcpy(proofs3 + 3 * idx[r], &g3[3 * (size_t)r], 3);
    }
    // (a flagged group's commitments are exact unless the SRS is irregular)
    if (commits3 && s->irregular) {
      if ((rc = plk_kzg_commit_batch(s, pp.data(), ll.data(), np, g3.data()))) return rc;
      for (int r = 0; r < n; r++) memcpy(commits3 + 3 * k * idx[r], &g3[3 * k * (size_t)r], 3 * k);
    }
    idx.clear();
    pp.clear();
    ll.clear();
    ww.clear();
    zz.clear();
    return PLK_OK;
  };
  for (size_t g = 0; g < ngroups; g++) {
    if (status[g] == 0) continue;
    if (status[g] != PLK_KZG_FLAT_IRREGULAR) {
      plk_set_error("%s: group %zu came back with status %u", fn, g, (unsigned)status[g]);
      return PLK_ERR_HIP;
    }
    idx.push_back(g);
    zz.push_back(zs[g]);
    for (size_t e = k * g; e < k * (g + 1); e++) {
      const size_t lo = offsets ? offsets[e] : e * m, len = offsets ? offsets[e + 1] - lo : m;
      pp.push_back(coeffs + lo);
      ll.push_back(len);
      ww.push_back(weights[e]);
    }
    int rc;
    if (idx.size() == RECOMP && (rc = flush())) return rc;
  }
  return flush();
}

}  // namespace

extern "C" {

int plk_kzg_fold_flat_plan(size_t m, size_t k, size_t ngroups, int ragged, int64_t out[4]) {
  const char* fn = "plk_kzg_fold_flat_plan";
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

int plk_kzg_open_fold_flat_dev(const plk_srs_t* s, const uint8_t* d_coeffs, size_t total, const uint32_t* d_offsets, size_t m,
                               size_t k, size_t ngroups, const uint8_t* d_weights, const uint8_t* d_zs, uint8_t* d_ys,
                               uint8_t* d_proofs3, uint8_t* d_commits3, uint8_t* d_status, void* stream) {
  const char* fn = "plk_kzg_open_fold_flat_dev";
  int rc = check_shape(fn, m, k, ngroups, d_offsets != nullptr, &total);
  if (rc || (rc = check_call(fn, s, !d_coeffs || !d_weights || !d_zs || !d_ys || !d_proofs3 || !d_status, d_offsets, m,
                             d_commits3 != nullptr)))
    return rc;
  return launch_fold(s, d_coeffs, total, d_offsets, m, k, ngroups, d_weights, d_zs, d_ys, d_proofs3, d_commits3, d_status,
                     (hipStream_t)stream);
}

int plk_kzg_open_fold_flat(const plk_srs_t* s, const uint8_t* coeffs, size_t total, const uint32_t* offsets, size_t m, size_t k,
                           size_t ngroups, const uint8_t* weights, const uint8_t* zs, uint8_t* ys, uint8_t* proofs3,
                           uint8_t* commits3) {
  const char* fn = "plk_kzg_open_fold_flat";
  int rc = check_shape(fn, m, k, ngroups, offsets != nullptr, &total);
  if (rc) return rc;
  if (!s || !coeffs || !weights || !zs || !ys || !proofs3) {
    plk_set_error("%s: the handle, coeffs, weights, zs, ys and proofs3 are required", fn);
    return PLK_ERR_ARG;
  }
  if ((rc = check_host_lists(fn, total, offsets, m, k, ngroups, weights, zs)) ||
      (rc = check_call(fn, s, false, nullptr, m, commits3 != nullptr)))
    return rc;
  return host_fold(fn, s, coeffs, total, offsets, m, k, ngroups, weights, zs, ys, proofs3, commits3);
}

}  // extern "C"
