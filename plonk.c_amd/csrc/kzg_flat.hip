// KZG flat batches (include/plonkhip.h, "KZG flat batches"): very many SHORT polynomials committed and opened
// in one launch -- the producer at the scale of the flat verify calls.  Polynomial g is the bytes [o_g, o_{g+1})
// of ONE flat coefficient array (uniform: o_g = g m; ragged: a device array of offsets), opened at its own
// device byte z_g; commitments, ys, proofs and statuses leave in flat arrays, three bytes per G1, as
// plk_kzg_verify_batch_dev and plk_kzg_verify_agg_batch_dev read them.
//
// Every polynomial has at most PLK_KZG_FLAT_MAX = one kzgo::CHUNK of coefficients, so an opening is the
// single-chunk middle of kzg.hip's kzg_open_kernel with nothing to carry in from other blocks and nothing to
// finish across blocks.  Three paths, a function of m alone (plk_kzg_flat_plan), each ONE launch with a
// grid-stride loop over the polynomials:
//   lane   m <= 32: one lane per polynomial.  Plain synthetic division from the top coefficient down, sixteen
//          coefficients at a time (kzgo::quotient16 with the running top quotient byte handed from the upper
//          half to the lower: the lane's own recurrence, so z = 0 is no special case and no z^16 = 1 is
//          needed); the quotient and coefficient bytes dotted with the first 32 SRS logs, which the block holds
//          in LDS.  Uniform m a multiple of 16 with 16-byte aligned coefficients: 16-byte loads.
//   wave   32 < m <= 1024: one wave per polynomial, sixteen coefficients per lane: the lane's aggregate
//          sum_k p[base + k] z^k, hf17::wave_suffix, quotient16 (shift16 at z = 0), the dot with the lane's
//          sixteen logs, a wave sum.  No LDS, no barrier: a wave goes from polynomial to polynomial on its own.
//   block  1024 < m <= 4096: one block per polynomial, sixteen coefficients per thread: kzgo::suffix_carry with
//          one chunk, then a plain block reduction where kzg_open_kernel has the ticketed finish.
// Plain stores only: no workspace, no atomics, no record, every word read was written by the caller, and every
// sum is an integer, so the bytes do not depend on any order.
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
constexpr uint32_t FLAT_BLOCKS = 2048;                   // grid cap of every path (grid-stride loops)
constexpr uint64_t MAX_TOTAL = 1ull << 32, MAX_NPOLY = 1ull << 30;
constexpr uint32_t G1_FLAGGED = 0xFFFFFFu;               // bytes FF FF FF
static_assert(PLK_KZG_FLAT_MAX == kzgo::CHUNK, "a polynomial is one chunk of the opening family");
static_assert(WAVE_MAX == 1024 && LANE_MAX == 2 * kzgo::E, "the paths' bounds as the header states them");
// a polynomial's log sums before their one reduction mod 102: every lane's dot16 is reduced first on the wave
// and block paths (<= 256 x 101), the lane path adds two unreduced dot16s (<= 32 x 255 x 101)
static_assert(2ull * 16 * 255 * 101 < (1ull << 32), "the lane path's sums fit 32 bits");

enum { PATH_LANE = 0, PATH_WAVE = 1, PATH_BLOCK = 2 };

struct FlatArgs {
  const uint8_t* coeffs;
  uint64_t total;
  const uint32_t* off;      // npoly + 1 words, or nullptr: o_g = g m
  uint64_t npoly;
  uint32_t m;
  uint32_t srs_bad;         // the SRS has no log form: every G1 output is flagged, ys stay exact
  const uint8_t* zs;        // nullptr: commitments only
  const uint8_t* logs;      // the SRS logs, zero padded (plk_kzg_host.h)
  const uint32_t* expw;     // the 102 EXP words {x, y, infinite, 0}
  uint8_t *ys, *proofs3;    // (with zs)
  uint8_t* commits3;        // or nullptr
  uint8_t* status;
};

// Polynomial g: its first byte and length.  Offsets are read as min(o, total), so no value makes a caller of
// this read outside [0, total); false for a ragged polynomial that is empty, falls, has an offset above total
// or is longer than m (PLK_KZG_FLAT_BAD).
__device__ __forceinline__ bool segment_of(const FlatArgs& A, uint64_t g, uint64_t& lo, uint32_t& len) {
  if (!A.off) {
    lo = g * A.m;   // (m npoly == total: checked by the caller)
    len = A.m;
    return true;
  }
  const uint64_t a = A.off[g], b = A.off[g + 1];
  const bool ok = a < b && b <= A.total && b - a <= A.m;
  lo = std::min(a, A.total);
  len = ok ? (uint32_t)(b - a) : 0u;
  return ok;
}

__device__ __forceinline__ void store_g1(uint8_t* out3, uint64_t g, uint32_t v) {
  out3[3 * g] = (uint8_t)v;
  out3[3 * g + 1] = (uint8_t)(v >> 8);
  out3[3 * g + 2] = (uint8_t)(v >> 16);
}

// Everything polynomial g returns, by the one thread that holds its sums.  ok: segment_of's answer and z < 17;
// noncanon: a coefficient byte >= 17; y: p(z); sq, sp: sum q_j log_j and sum p_j log_j (any multiple of 102 on
// top).  The commitment is exact for any coefficient byte (g1_mul takes the raw byte); the proof is not.
__device__ __forceinline__ void store_poly(const FlatArgs& A, uint64_t g, bool ok, bool noncanon, uint32_t y, uint32_t sq,
                                           uint32_t sp) {
  const bool open = A.zs != nullptr;
  const uint32_t st = !ok ? (uint32_t)PLK_KZG_FLAT_BAD : (A.srs_bad || (open && noncanon)) ? (uint32_t)PLK_KZG_FLAT_IRREGULAR : 0u;
  A.status[g] = (uint8_t)st;
  if (open) {
    A.ys[g] = ok ? (uint8_t)y : (uint8_t)0xFF;
    store_g1(A.proofs3, g, st ? G1_FLAGGED : A.expw[sq % ORD]);
  }
  if (A.commits3) store_g1(A.commits3, g, (!ok || A.srs_bad) ? G1_FLAGGED : A.expw[sp % ORD]);
}

// The device z of polynomial g: false for a byte >= 17 (the host cannot see it), z = 0 then
__device__ __forceinline__ bool point_of(const FlatArgs& A, uint64_t g, uint32_t& z) {
  z = 0;
  if (!A.zs) return true;
  const uint32_t b = A.zs[g];
  if (b >= HFP) return false;
  z = b;
  return true;
}

// lane path: see the head of this file.  VEC (uniform, m a multiple of 16, coefficients 16-byte aligned):
// every polynomial is as aligned as the array.
template <bool VEC>
__global__ __launch_bounds__(kzgo::T) void flat_lane_kernel(FlatArgs A) {
  __shared__ __attribute__((aligned(16))) uint32_t slog[LANE_MAX / 4];   // the first 32 SRS logs, four to a word
  if (threadIdx.x < LANE_MAX / 4)
    slog[threadIdx.x] = A.srs_bad ? 0u : reinterpret_cast<const uint32_t*>(A.logs)[threadIdx.x];   // (>= 32 bytes, zero padded)
  __syncthreads();
  const bool open = A.zs != nullptr, commit = A.commits3 != nullptr;
  for (uint64_t g = (uint64_t)blockIdx.x * kzgo::T + threadIdx.x; g < A.npoly; g += (uint64_t)gridDim.x * kzgo::T) {
    uint64_t lo;
    uint32_t len, z;
    bool ok = segment_of(A, g, lo, len);
    ok = point_of(A, g, z) && ok;
    const uint8_t* p = A.coeffs + lo;
    uint32_t run = 0, sq = 0, sp = 0;   // run: the quotient byte above the half at hand, then p(z) (<= 255 + 16 x 16)
    bool noncanon = false;
    for (int h = ok ? (int)((len - 1) >> 4) : -1; h >= 0; h--) {
      uint32_t nb[4];
      if (VEC) kzgo::load16_vec(p, 16u * h, nb);
      else kzgo::load16_rolled(p, len, 16u * h, nb);
      noncanon |= hf17::any_noncanonical(nb);
      const uint4 lv = *reinterpret_cast<const uint4*>(&slog[4 * h]);
      const uint32_t l[4] = {lv.x, lv.y, lv.z, lv.w};
      if (commit) sp += kzgo::dot16(l, nb);   // (<= 16 x 101 x 255 a half)
      if (open) {
        // q[16 h + 15] = run, q[j] = p[j + 1] + z q[j + 1] below it; then the byte above the next half,
        // q[16 h - 1] = p[16 h] + z q[16 h] -- which after the last half is p[0] + z q[0] = p(z)
        uint32_t o[4] = {0, 0, 0, 0};
        kzgo::quotient16(nb, z, run, kzgo::PackInto{o});
        sq += kzgo::dot16(l, o);
        run = (nb[0] & 0xFFu) + z * (o[0] & 0xFFu);
      }
    }
    store_poly(A, g, ok, noncanon, run % HFP, sq, sp);
  }
}

// The sixteen coefficients [base, base + 16) of a polynomial of len bytes at p, zero past len
__device__ __forceinline__ void load_run(const uint8_t* p, uint32_t len, uint32_t base, uint32_t (&nb)[4]) {
  if (kzgo::aligned16(p) && base + 16 <= len)
    kzgo::load16_vec(p, base, nb);
  else
    kzgo::load16_rolled(p, len, base, nb);
}

// The thread's sixteen quotient bytes o once it holds its coefficients nb and run = the aggregates of the
// threads after it (z != 0): the pieces of plk_kzg_open.h as kzg.hip's open_quotient orders them
__device__ __forceinline__ void quotient_run(const uint8_t* p, uint32_t len, uint32_t base, const uint32_t (&nb)[4], uint32_t z,
                                             uint32_t run, uint32_t (&o)[4]) {
  o[0] = o[1] = o[2] = o[3] = 0;
  if (z != 0)
    kzgo::quotient16(nb, z, run, kzgo::PackInto{o});
  else   // the thread's last quotient byte is the next thread's first coefficient
    kzgo::shift16(nb, base + 16 < len ? p[base + 16] : 0u, kzgo::PackInto{o});
}

// wave path: see the head of this file.  Polynomial g is wave-uniform, so every branch on it is.
__global__ __launch_bounds__(kzgo::T) void flat_wave_kernel(FlatArgs A) {
  const uint32_t lane = threadIdx.x & (PLK_WAVE - 1), base = lane * kzgo::E;
  const bool open = A.zs != nullptr;
  for (uint64_t g = (uint64_t)blockIdx.x * kzgo::WAVES + threadIdx.x / PLK_WAVE; g < A.npoly;
       g += (uint64_t)gridDim.x * kzgo::WAVES) {
    uint64_t lo;
    uint32_t len, z;
    bool ok = segment_of(A, g, lo, len);
    ok = point_of(A, g, z) && ok;
    z = (uint32_t)__builtin_amdgcn_readfirstlane((int)z);   // (every lane read the same byte)
    uint32_t y = 0, sq = 0, sp = 0;
    bool noncanon = false;
    if (ok) {   // (uniform)
      const uint8_t* p = A.coeffs + lo;
      uint32_t nb[4];
      load_run(p, len, base, nb);
      const uint4 lg = kzgo::Finish::logs(A.logs, A.srs_bad, base, len);
      const uint32_t l[4] = {lg.x, lg.y, lg.z, lg.w};
      noncanon = __ballot(hf17::any_noncanonical(nb)) != 0;
      if (A.commits3) sp = plk_wave_sum(kzgo::dot16(l, nb) % ORD);   // (the sum <= 64 x 101)
      if (open) {
        uint32_t pk[4], o[4];
        kzgo::packed_powers(z, pk);
        const uint32_t tot = hf17::mod17(kzgo::dot16(nb, pk));   // (<= 16 x 255 x 16)
        const uint32_t run = hf17::wave_suffix(tot) - tot;       // the later lanes' aggregates (<= 63 x 16)
        quotient_run(p, len, base, nb, z, run, o);
        sq = plk_wave_sum(kzgo::dot16(l, o) % ORD);
        y = hf17::mod17((nb[0] & 0xFFu) + z * (o[0] & 0xFFu));   // (lane 0's: p[0] + z q[0])
      }
    }
    if (lane == 0) store_poly(A, g, ok, noncanon, y, sq, sp);
  }
}

// block path: see the head of this file.  Two barriers a polynomial (suffix_carry's, and the reduction's), so
// the LDS words of one polynomial are read before the next one's are written.
__global__ __launch_bounds__(kzgo::T) void flat_block_kernel(FlatArgs A) {
  __shared__ uint32_t ws[2 * kzgo::WAVES];
  __shared__ uint32_t red[3][kzgo::WAVES];   // per wave: sum q log, sum p log, a byte >= 17
  const uint32_t base = threadIdx.x * kzgo::E, wv = threadIdx.x / PLK_WAVE, lane = threadIdx.x & (PLK_WAVE - 1);
  const bool open = A.zs != nullptr;
  for (uint64_t g = blockIdx.x; g < A.npoly; g += gridDim.x) {   // (uniform)
    uint64_t lo;
    uint32_t len, z;
    bool ok = segment_of(A, g, lo, len);
    ok = point_of(A, g, z) && ok;
    if (!ok) {   // (uniform)
      if (threadIdx.x == 0) store_poly(A, g, false, false, 0, 0, 0);
      continue;
    }
    const uint8_t* p = A.coeffs + lo;
    uint32_t nb[4];
    load_run(p, len, base, nb);
    const uint4 lg = kzgo::Finish::logs(A.logs, A.srs_bad, base, len);
    const uint32_t l[4] = {lg.x, lg.y, lg.z, lg.w};
    const uint32_t anybad = __ballot(hf17::any_noncanonical(nb)) != 0 ? 1u : 0u;
    uint32_t y = 0, sq = 0, sp = 0;
    if (A.commits3) sp = plk_wave_sum(kzgo::dot16(l, nb) % ORD);
    if (open) {   // (uniform: suffix_carry holds a barrier)
      uint32_t pk[4], o[4];
      kzgo::packed_powers(z, pk);
      const uint32_t tot = hf17::mod17(kzgo::dot16(nb, pk));   // (<= 16 x 255 x 16)
      bool unused = false;
      const uint32_t run = kzgo::suffix_carry(tot, nullptr, 0u, 1u, ws, unused);   // no other chunk: the block's exclusive suffix sum
      quotient_run(p, len, base, nb, z, run, o);
      sq = plk_wave_sum(kzgo::dot16(l, o) % ORD);
      y = hf17::mod17((nb[0] & 0xFFu) + z * (o[0] & 0xFFu));   // (thread 0's: p[0] + z q[0])
    }
    if (lane == 0) {
      red[0][wv] = sq;
      red[1][wv] = sp;
      red[2][wv] = anybad;
    }
    __syncthreads();
    if (threadIdx.x == 0)
      store_poly(A, g, true, (red[2][0] | red[2][1] | red[2][2] | red[2][3]) != 0, y, red[0][0] + red[0][1] + red[0][2] + red[0][3],
                 red[1][0] + red[1][1] + red[1][2] + red[1][3]);
    if (!open) __syncthreads();   // (the second barrier that suffix_carry is with zs)
  }
}
static_assert(kzgo::WAVES == 4, "the block path adds four wave words");

struct Plan {
  int path;
  uint32_t per_block;   // polynomials a block takes per turn of its loop
  uint32_t blocks;
};

// arguments checked by the caller
Plan plan_of(uint64_t m, uint64_t npoly) {
  Plan p{};
  p.path = m <= LANE_MAX ? PATH_LANE : m <= WAVE_MAX ? PATH_WAVE : PATH_BLOCK;
  p.per_block = p.path == PATH_LANE ? (uint32_t)kzgo::T : p.path == PATH_WAVE ? (uint32_t)kzgo::WAVES : 1u;
  p.blocks = (uint32_t)std::min<uint64_t>((npoly + p.per_block - 1) / p.per_block, FLAT_BLOCKS);
  return p;
}

// PLK_OK, or the code every entry point returns for this shape (no handle, no device).  total: as the caller
// gave it, or m npoly for the plan of a uniform call
int check_shape(const char* fn, size_t m, size_t npoly, bool ragged, const size_t* total) {
  if (m == 0 || npoly == 0 || (total && *total == 0)) {
    plk_set_error("%s: m > 0, npoly > 0 and total > 0 are required", fn);
    return PLK_ERR_ARG;
  }
  if (m > PLK_KZG_FLAT_MAX) {
    plk_set_error("%s: m = %zu exceeds PLK_KZG_FLAT_MAX = %d coefficients per polynomial", fn, m, PLK_KZG_FLAT_MAX);
    return PLK_ERR_RANGE;
  }
  if ((uint64_t)npoly > MAX_NPOLY) {
    plk_set_error("%s: npoly = %zu must stay within 2^30", fn, npoly);
    return PLK_ERR_RANGE;
  }
  const uint64_t flat = (uint64_t)m * npoly;   // (<= 2^12 x 2^30)
  if (total && !ragged && *total != flat) {
    plk_set_error("%s: m npoly == total is required without offsets (%zu x %zu != %zu)", fn, m, npoly, *total);
    return PLK_ERR_ARG;
  }
  if ((total ? (uint64_t)*total : ragged ? 0ull : flat) >= MAX_TOTAL) {
    plk_set_error("%s: total = %llu must stay below 2^32", fn, (unsigned long long)(total ? *total : flat));
    return PLK_ERR_RANGE;
  }
  return PLK_OK;
}

// the checks of the four calls after the shape: pointers, the offsets' alignment, the SRS bound on m as given,
// the device (no device query before the last)
int check_call(const char* fn, const plk_srs* s, bool null_ptr, const uint32_t* off, size_t m, bool open, bool commit) {
  if (!s || null_ptr) {
    plk_set_error("%s: the handle, the coefficient array and every required output are required", fn);
    return PLK_ERR_ARG;
  }
  if (off && (uintptr_t)off % 4) {
    plk_set_error("%s: the offsets must be 4-byte aligned", fn);
    return PLK_ERR_ARG;
  }
  int rc;
  if (commit && (rc = plk_kzg_check_srs_len(s, m))) return rc;
  if (open && (rc = plk_kzg_check_srs_len(s, std::max<size_t>(m - 1, 1)))) return rc;
  return plk_kzg_check_device(fn, s);
}

// the one launch of a call, arguments checked
int launch_flat(const plk_srs* s, const uint8_t* d_coeffs, size_t total, const uint32_t* d_off, size_t m, size_t npoly,
                const uint8_t* d_zs, uint8_t* d_ys, uint8_t* d_proofs3, uint8_t* d_commits3, uint8_t* d_status, hipStream_t st) {
  FlatArgs A{};
  A.coeffs = d_coeffs;
  A.total = total;
  A.off = d_off;
  A.npoly = npoly;
  A.m = (uint32_t)m;
  A.srs_bad = s->irregular ? 1u : 0u;
  A.zs = d_zs;
  A.logs = s->d_log;
  A.expw = s->exp_words;
  A.ys = d_ys;
  A.proofs3 = d_proofs3;
  A.commits3 = d_commits3;
  A.status = d_status;
  const Plan p = plan_of(m, npoly);
  const dim3 grid(p.blocks), block(kzgo::T);
  if (p.path == PATH_LANE) {
    if (!d_off && m % kzgo::E == 0 && (uintptr_t)d_coeffs % 16 == 0)
      hipLaunchKernelGGL(flat_lane_kernel<true>, grid, block, 0, st, A);
    else
      hipLaunchKernelGGL(flat_lane_kernel<false>, grid, block, 0, st, A);
  } else if (p.path == PATH_WAVE) {
    hipLaunchKernelGGL(flat_wave_kernel, grid, block, 0, st, A);
  } else {
    hipLaunchKernelGGL(flat_block_kernel, grid, block, 0, st, A);
  }
  PLK_HIP(hipGetLastError());
  return PLK_OK;
}

// the host forms' own checks: every ragged polynomial non-empty, rising, inside total and within m; every z < 17
int check_host_lists(const char* fn, size_t total, const uint32_t* offsets, size_t m, size_t npoly, const uint8_t* zs) {
  if (offsets) {
    for (size_t g = 0; g < npoly; g++) {
      const uint64_t a = offsets[g], b = offsets[g + 1];
      if (!(a < b && b <= total && b - a <= m)) {
        plk_set_error("%s: polynomial %zu = bytes [%u, %u) is empty, falls, leaves total = %zu or exceeds m = %zu", fn, g,
                      offsets[g], offsets[g + 1], total, m);
        return PLK_ERR_ARG;
      }
    }
  }
  for (size_t g = 0; zs && g < npoly; g++) {
    if (zs[g] >= HFP) {
      plk_set_error("%s: polynomial %zu: z = %u is not a GF(17) value", fn, g, (unsigned)zs[g]);
      return PLK_ERR_ARG;
    }
  }
  return PLK_OK;
}

// The host-buffer forms: the arrays uploaded on 16-byte boundaries, the one launch, the read-back; every
// flagged polynomial (a byte >= 17 in an opening, every polynomial of an irregular SRS) recomputed through
// plk_kzg_open_batch / plk_kzg_commit_batch, RECOMP at a time.
int host_flat(const char* fn, const plk_srs* s, const uint8_t* coeffs, size_t total, const uint32_t* offsets, size_t m,
              size_t npoly, const uint8_t* zs, uint8_t* ys, uint8_t* proofs3, uint8_t* commits3) {
  const bool open = zs != nullptr;
  std::vector<uint8_t> status(npoly, (uint8_t)PLK_KZG_FLAT_IRREGULAR);
  if (!s->irregular) {
    const size_t ob = offsets ? 4 * (npoly + 1) : 0;
    const size_t o_off = plk_pad16(total), o_zs = o_off + plk_pad16(ob), o_ys = o_zs + plk_pad16(npoly), o_st = o_ys + plk_pad16(npoly),
                 o_pr = o_st + plk_pad16(npoly), o_cm = o_pr + plk_pad16(3 * npoly), bytes = o_cm + plk_pad16(3 * npoly);
    PlkScratch D;
    int rc = D.alloc(fn, bytes);
    if (rc) return rc;
    PLK_HIP(hipMemcpyAsync(D.d, coeffs, total, hipMemcpyHostToDevice, s->st));
    if (offsets) PLK_HIP(hipMemcpyAsync(D.d + o_off, offsets, ob, hipMemcpyHostToDevice, s->st));
    if (open) PLK_HIP(hipMemcpyAsync(D.d + o_zs, zs, npoly, hipMemcpyHostToDevice, s->st));
    if ((rc = launch_flat(s, D.d, total, offsets ? (const uint32_t*)(D.d + o_off) : nullptr, m, npoly, open ? D.d + o_zs : nullptr,
                          D.d + o_ys, D.d + o_pr, commits3 ? D.d + o_cm : nullptr, D.d + o_st, s->st)))
      return rc;
    PLK_HIP(hipMemcpyAsync(status.data(), D.d + o_st, npoly, hipMemcpyDeviceToHost, s->st));
    if (open) {
      PLK_HIP(hipMemcpyAsync(ys, D.d + o_ys, npoly, hipMemcpyDeviceToHost, s->st));
      PLK_HIP(hipMemcpyAsync(proofs3, D.d + o_pr, 3 * npoly, hipMemcpyDeviceToHost, s->st));
    }
    if (commits3) PLK_HIP(hipMemcpyAsync(commits3, D.d + o_cm, 3 * npoly, hipMemcpyDeviceToHost, s->st));
    PLK_HIP(hipStreamSynchronize(s->st));
  }
  constexpr size_t RECOMP = 1024;
  std::vector<size_t> idx;
  std::vector<const uint8_t*> pp;
  std::vector<size_t> ll;
  std::vector<uint8_t> zz, yy, g3;
  auto flush = [&]() -> int {
    if (idx.empty()) return PLK_OK;
    const int n = (int)idx.size();
    int rc;
    yy.resize(n);
    g3.resize(3 * (size_t)n);
    if (open) {
      if ((rc = plk_kzg_open_batch(s, pp.data(), ll.data(), zz.data(), n, yy.data(), g3.data()))) return rc;
      for (int k = 0; k < n; k++) {
        ys[idx[k]] = yy[k];
        memcpy(proofs3 + 3 * idx[k], &g3[3 * (size_t)k], 3);
      }
    }
    // (a flagged opening's commitment is exact unless the SRS is irregular)
    if (commits3 && (!open || s->irregular)) {
      if ((rc = plk_kzg_commit_batch(s, pp.data(), ll.data(), n, g3.data()))) return rc;
      for (int k = 0; k < n; k++) memcpy(commits3 + 3 * idx[k], &g3[3 * (size_t)k], 3);
    }
    idx.clear();
    pp.clear();
    ll.clear();
    zz.clear();
    return PLK_OK;
  };
  for (size_t g = 0; g < npoly; g++) {
    if (status[g] == 0) continue;
    if (status[g] != PLK_KZG_FLAT_IRREGULAR) {
      plk_set_error("%s: polynomial %zu came back with status %u", fn, g, (unsigned)status[g]);
      return PLK_ERR_HIP;
    }
    const size_t lo = offsets ? offsets[g] : g * m, len = offsets ? offsets[g + 1] - lo : m;
    idx.push_back(g);
    pp.push_back(coeffs + lo);
    ll.push_back(len);
    if (open) zz.push_back(zs[g]);
    int rc;
    if (idx.size() == RECOMP && (rc = flush())) return rc;
  }
  return flush();
}

}  // namespace

extern "C" {

int plk_kzg_flat_plan(size_t m, size_t npoly, int ragged, int64_t out[4]) {
  const char* fn = "plk_kzg_flat_plan";
  if (!out) {
    plk_set_error("%s: out is required", fn);
    return PLK_ERR_ARG;
  }
  const int rc = check_shape(fn, m, npoly, ragged != 0, nullptr);
  if (rc) return rc;
  const Plan p = plan_of(m, npoly);
  out[0] = p.path;
  out[1] = p.per_block;
  out[2] = p.blocks;
  out[3] = 1;
  return PLK_OK;
}

int plk_kzg_commit_flat_dev(const plk_srs_t* s, const uint8_t* d_coeffs, size_t total, const uint32_t* d_offsets, size_t m,
                            size_t npoly, uint8_t* d_commits3, uint8_t* d_status, void* stream) {
  const char* fn = "plk_kzg_commit_flat_dev";
  int rc = check_shape(fn, m, npoly, d_offsets != nullptr, &total);
  if (rc || (rc = check_call(fn, s, !d_coeffs || !d_commits3 || !d_status, d_offsets, m, false, true))) return rc;
  return launch_flat(s, d_coeffs, total, d_offsets, m, npoly, nullptr, nullptr, nullptr, d_commits3, d_status, (hipStream_t)stream);
}

int plk_kzg_open_flat_dev(const plk_srs_t* s, const uint8_t* d_coeffs, size_t total, const uint32_t* d_offsets, size_t m,
                          size_t npoly, const uint8_t* d_zs, uint8_t* d_ys, uint8_t* d_proofs3, uint8_t* d_commits3,
                          uint8_t* d_status, void* stream) {
  const char* fn = "plk_kzg_open_flat_dev";
  int rc = check_shape(fn, m, npoly, d_offsets != nullptr, &total);
  if (rc || (rc = check_call(fn, s, !d_coeffs || !d_zs || !d_ys || !d_proofs3 || !d_status, d_offsets, m, true, d_commits3 != nullptr)))
    return rc;
  return launch_flat(s, d_coeffs, total, d_offsets, m, npoly, d_zs, d_ys, d_proofs3, d_commits3, d_status, (hipStream_t)stream);
}

int plk_kzg_commit_flat(const plk_srs_t* s, const uint8_t* coeffs, size_t total, const uint32_t* offsets, size_t m, size_t npoly,
                        uint8_t* commits3) {
  const char* fn = "plk_kzg_commit_flat";
  int rc = check_shape(fn, m, npoly, offsets != nullptr, &total);
  if (rc) return rc;
  if (!s || !coeffs || !commits3) {
    plk_set_error("%s: the handle, coeffs and commits3 are required", fn);
    return PLK_ERR_ARG;
  }
  if ((rc = check_host_lists(fn, total, offsets, m, npoly, nullptr)) || (rc = check_call(fn, s, false, nullptr, m, false, true)))
    return rc;
  return host_flat(fn, s, coeffs, total, offsets, m, npoly, nullptr, nullptr, nullptr, commits3);
}

int plk_kzg_open_flat(const plk_srs_t* s, const uint8_t* coeffs, size_t total, const uint32_t* offsets, size_t m, size_t npoly,
                      const uint8_t* zs, uint8_t* ys, uint8_t* proofs3, uint8_t* commits3) {
  const char* fn = "plk_kzg_open_flat";
  int rc = check_shape(fn, m, npoly, offsets != nullptr, &total);
  if (rc) return rc;
  if (!s || !coeffs || !zs || !ys || !proofs3) {
    plk_set_error("%s: the handle, coeffs, zs, ys and proofs3 are required", fn);
    return PLK_ERR_ARG;
  }
  if ((rc = check_host_lists(fn, total, offsets, m, npoly, zs)) || (rc = check_call(fn, s, false, nullptr, m, true, commits3 != nullptr)))
    return rc;
  return host_flat(fn, s, coeffs, total, offsets, m, npoly, zs, ys, proofs3, commits3);
}

}  // extern "C"
