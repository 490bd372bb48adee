// KZG per-point openings (include/plonkhip.h, "KZG per-point openings"): one committed polynomial opened at a
// set S of GF(17) points with a separate proof per point -- the producer of the flat (z, y, proof) arrays the
// verify calls take on the device.
//
// Job e = (polynomial i, point a of S_i) is the single opening of kzg.hip: y = p_i(a), proof = [(p_i - y) / (x - a)].
// Listing the polynomial once per point there reads its bytes twice and the SRS logs once PER POINT.  Here a
// thread loads its sixteen coefficient bytes and its sixteen SRS logs once and forms the up to 17 single-point
// quotients from them in registers (plk_kzg_open.h: suffix_carry and quotient16 for a != 0, shift16 for a = 0),
// as kzg_multi.hip does -- but keeps them apart: each is dotted with the logs on its own, none is summed into
// an h.  The launches of a call, PLK_KZG_POINTS_LAUNCH_POLYS polynomials at a time:
//   points_agg_kernel     only when some polynomial exceeds one chunk; block (chunk >= 1, polynomial): one word
//                         per (point a != 0 of the set, chunk) = sum_j p[j] a^(j mod 16) mod 17 with the >= 17
//                         flag in bit 8, the polynomial's bytes loaded once for all its points
//   points_scan_kernel    after it; block (non-zero point, polynomial): the point's aggregate words turned in
//                         place into the carries, word c = sum of the aggregates of the chunks after c mod 17.
//                         With the aggregates as they are every opening block sums the later chunks' words once
//                         per point (chunks^2 / 2 words a point in all); with the carries it reads one word a
//                         point, asked for one point ahead.  Measured: nine polynomials of
//                         2^22 at 17 points 370 -> 338 us, one polynomial unchanged, a launch (2 us) dearer.
//   points_open_kernel    block (chunk, polynomial): per point of the set (a rolled loop, the point's constants
//                         uniform) the carry, the sixteen quotient bytes in four packed words, their dot product
//                         with the logs mod 102, the wave's sum into LDS; one barrier after the last point, then
//                         one thread per point adds the waves.  A polynomial of one chunk finishes here (EXP
//                         lookup, three bytes, status); otherwise the block writes one partial word per (job,
//                         chunk): the log sum mod 102, the bad flag in bit 8.  The chunk-0 block writes y and z.
//   points_finish_kernel  only when partials were written; one wave per job sums its nchunk partials, ORs the
//                         flags, looks EXP up and writes proof bytes and status.
// Plain stores and launch boundaries, as kzg_agg.hip: no atomics, no record to zero, every workspace word read
// was written by the same call, and the sums are integers, so the result does not depend on any order.
#include <string.h>

#include <algorithm>
#include <vector>

#include "plk_device.h"
#include "plk_hf17.h"
#include "plk_hostcall.h"
#include "plk_kzg_host.h"
#include "plk_kzg_open.h"

namespace {

constexpr uint32_t HFP = hf17::P;
constexpr uint32_t ORD = PLK_GROUP_ORDER;
constexpr int NPTS = 17;                              // GF(17) points
constexpr int POINTS_POLYS = PLK_KZG_POINTS_LAUNCH_POLYS;
constexpr uint32_t FULL_MASK = (1u << NPTS) - 1;
constexpr uint64_t POINTS_MAX_JOBS = 1ull << 30;
using hf17::any_noncanonical;
using hf17::mod17;
using kzgo::dot16;
using kzgo::packed_powers;

struct PointsPoly {
  const uint8_t* p;
  uint64_t len;
  uint32_t agg;    // first aggregate word: word (rank of a among the non-zero points) nchunk + c
  uint32_t part;   // first partial word: word (rank of a in the set) nchunk + c
  uint32_t job;    // the polynomial's first job in the call
  uint32_t mask;   // S_i
};
struct PointsBatch {
  PointsPoly p[POINTS_POLYS];
};
static_assert(sizeof(PointsBatch) <= 3072, "the batch travels as a kernel argument");

struct PointsOut {
  uint8_t *zs, *ys, *proofs3, *status;   // flat in job order (zs may be nullptr)
};

__device__ __forceinline__ uint32_t chunks_of(uint64_t len) { return (uint32_t)((len + kzgo::CHUNK - 1) / kzgo::CHUNK); }
// point number r of m, ascending (r < popcount(m))
__device__ __forceinline__ uint32_t point_of(uint32_t m, uint32_t r) {
  for (uint32_t k = 0; k < r; k++) m &= m - 1;
  return (uint32_t)__builtin_ctz(m);
}
__device__ __forceinline__ void points_load(const PointsPoly& P, uint64_t base, uint32_t (&w)[4]) {
  if (kzgo::aligned16(P.p) && base + 16 <= P.len)
    kzgo::load16_vec(P.p, base, w);
  else
    kzgo::load16_rolled(P.p, P.len, base, w);
}
// proof bytes and status of job e: EXP[lg], or FF FF FF under the flag
__device__ __forceinline__ void points_store(const PointsOut& out, uint32_t e, uint32_t lg, uint32_t flag,
                                             const uint32_t* __restrict__ exp_words) {
  const uint32_t g = flag ? 0xFFFFFFu : exp_words[lg];   // {x, y, inf, 0}
  out.proofs3[3 * (size_t)e] = (uint8_t)g;
  out.proofs3[3 * (size_t)e + 1] = (uint8_t)(g >> 8);
  out.proofs3[3 * (size_t)e + 2] = (uint8_t)(g >> 16);
  out.status[e] = (uint8_t)flag;
}

// Aggregates of chunk blockIdx.x + 1 of polynomial blockIdx.y (see the head of this file).
__global__ __launch_bounds__(kzgo::T) void points_agg_kernel(PointsBatch B, uint32_t* __restrict__ work) {
  __shared__ uint32_t psum[NPTS - 1][kzgo::WAVES];   // per wave: the sum mod 17
  __shared__ uint32_t pbad[kzgo::WAVES];
  const PointsPoly& P = B.p[blockIdx.y];
  const uint32_t c = blockIdx.x + 1, nchunk = chunks_of(P.len);
  if (c >= nchunk) return;
  const uint32_t lane = threadIdx.x & (PLK_WAVE - 1), wv = threadIdx.x / PLK_WAVE;
  const uint64_t base = (uint64_t)c * kzgo::CHUNK + (uint64_t)threadIdx.x * kzgo::E;
  uint32_t w[4];
  points_load(P, base, w);
  const uint32_t anybad = __ballot(any_noncanonical(w)) != 0 ? 1u : 0u;
  if (lane == 0) pbad[wv] = anybad;
  const uint32_t nz = P.mask >> 1;   // bit a - 1: the non-zero point a
  uint32_t r = 0;
  for (uint32_t m = nz; m; m &= m - 1, r++) {   // (uniform)
    const uint32_t a = (uint32_t)__builtin_ctz(m) + 1;
    uint32_t pk[4];
    packed_powers(a, pk);
    const uint32_t s = plk_wave_sum(dot16(w, pk));   // (<= 64 x 16 x 255 x 16)
    if (lane == 0) psum[r][wv] = s % HFP;
  }
  __syncthreads();
  if (threadIdx.x < r) {
    const uint32_t s = (psum[threadIdx.x][0] + psum[threadIdx.x][1] + psum[threadIdx.x][2] + psum[threadIdx.x][3]) % HFP;
    const uint32_t bad = (pbad[0] | pbad[1] | pbad[2] | pbad[3]) != 0 ? 1u : 0u;
    work[P.agg + threadIdx.x * nchunk + c] = s | bad << 8;
  }
}

// Row blockIdx.x (the non-zero points of the set, ascending) of polynomial blockIdx.y: aggregate words 1 ..
// nchunk - 1 turned in place into carries, word c = sum_{b > c} aggregate b mod 17 for c = 0 .. nchunk - 1 (the
// flag bits go: every chunk's block flags its own bytes, and a job's flag is the OR over its chunks).  Tiles of
// SCAN_TILE words from the top down, four consecutive words a thread; suffix_carry without chunks is the
// block's exclusive suffix sum, its one barrier the tile's.  tsum: thread 0 leaves the tile's total for the
// next tile's pass, read there after that pass's barrier (two slots: the tile after next writes this one again).
constexpr int SCAN_WORDS = 4, SCAN_TILE = kzgo::T * SCAN_WORDS;
__global__ __launch_bounds__(kzgo::T) void points_scan_kernel(PointsBatch B, uint32_t* __restrict__ work) {
  __shared__ uint32_t ws[2][2 * kzgo::WAVES];
  __shared__ uint32_t tsum[2];
  const PointsPoly& P = B.p[blockIdx.y];
  const uint32_t nchunk = chunks_of(P.len);
  if (nchunk <= 1 || blockIdx.x >= (uint32_t)__builtin_popcount(P.mask >> 1)) return;
  uint32_t* row = work + P.agg + blockIdx.x * nchunk;
  uint32_t above = 0, par = 0;   // the sum of the words above the tile, mod 17 (uniform)
  bool first = true, unused = false;
  for (uint32_t hi = nchunk; hi > 0;) {   // (uniform)
    const uint32_t lo = hi > SCAN_TILE ? hi - SCAN_TILE : 0u;
    const uint32_t i0 = lo + threadIdx.x * SCAN_WORDS;
    uint32_t v[SCAN_WORDS];
#pragma unroll
    for (int k = 0; k < SCAN_WORDS; k++) v[k] = i0 + k >= 1 && i0 + k < hi ? row[i0 + k] & 0xFFu : 0u;   // (word 0 was never written)
    const uint32_t tot = v[0] + v[1] + v[2] + v[3];   // (<= 4 x 16)
    uint32_t s = kzgo::suffix_carry(tot, nullptr, 0u, 1u, ws[par], unused);   // the later threads' words (<= 255 x 64)
    if (!first) above = (above + tsum[par ^ 1u]) % HFP;
    if (threadIdx.x == 0) tsum[par] = s + tot;   // the tile's total
    s += above;
#pragma unroll
    for (int k = SCAN_WORDS - 1; k >= 0; k--) {
      if (i0 + k < hi) row[i0 + k] = s % HFP;
      s += v[k];
    }
    first = false;
    par ^= 1u;
    hi = lo;
  }
}

// Block (chunk, polynomial) of the openings: see the head of this file.  srs_bad: the SRS has no log form
// (every job is then flagged; ys are still exact).
__global__ __launch_bounds__(kzgo::T) void points_open_kernel(PointsBatch B, const uint8_t* __restrict__ logs,
                                                            uint32_t* __restrict__ work, PointsOut out,
                                                            const uint32_t* __restrict__ exp_words, uint32_t srs_bad) {
  __shared__ uint32_t ws[2][2 * kzgo::WAVES];   // suffix_carry's words, alternating from point to point
  __shared__ uint32_t psum[NPTS][kzgo::WAVES];  // per (point, wave): the log sum
  __shared__ uint32_t ysum[NPTS][kzgo::WAVES];  // chunk 0, per (point, wave): the share of p(a)
  __shared__ uint32_t pbad[kzgo::WAVES];
  const PointsPoly& P = B.p[blockIdx.y];
  const uint32_t c = blockIdx.x, nchunk = chunks_of(P.len);
  if (c >= nchunk) return;
  const uint8_t* p = P.p;
  const uint64_t len = P.len, ql = len - 1;
  const uint32_t mask = P.mask;
  const uint64_t base = (uint64_t)c * kzgo::CHUNK + (uint64_t)threadIdx.x * kzgo::E;
  const uint32_t wv = threadIdx.x / PLK_WAVE, lane = threadIdx.x & (PLK_WAVE - 1);
  uint32_t nb[4];
  points_load(P, base, nb);
  const uint4 lg = kzgo::Finish::logs(logs, srs_bad, base, ql);
  const uint32_t l[4] = {lg.x, lg.y, lg.z, lg.w};
  bool bad = any_noncanonical(nb);
  // the carry into this chunk for non-zero point number rz (points_scan_kernel; < 17), asked for one point ahead
  const uint32_t tz = (uint32_t)__builtin_popcount(mask >> 1);
  const uint32_t* __restrict__ carries = work + P.agg + c;
  uint32_t next = nchunk > 1 && tz > 0 ? carries[0] : 0u;
  uint32_t par = 0, r = 0, rz = 0;
  for (uint32_t m = mask; m; m &= m - 1, r++) {   // (uniform) the points of S
    const uint32_t a = (uint32_t)__builtin_ctz(m);
    uint32_t o[4] = {0, 0, 0, 0};
    if (a != 0) {
      const uint32_t carry = next;
      if (nchunk > 1 && rz + 1 < tz) next = carries[(rz + 1) * nchunk];
      uint32_t pk[4];
      packed_powers(a, pk);
      const uint32_t t = dot16(nb, pk);   // (<= 16 x 255 x 16 = 65280, inside mod17's range)
      // (no chunks for suffix_carry to sum: the block's exclusive suffix sum, <= 255 x 16, and its barrier)
      const uint32_t run = kzgo::suffix_carry(mod17(t), nullptr, 0u, 1u, ws[par], bad) + carry;
      par ^= 1u;   // (the next point's words: a wave may arrive there while another still reads these)
      kzgo::quotient16(nb, a, run, kzgo::PackInto{o});
      if (c == 0) {   // (uniform) the wave's share of p(a): its own sums, and the later chunks' once (a^4096 = 1)
        const uint32_t s = plk_wave_sum(t);   // (<= 64 x 65280)
        if (lane == 0) ysum[r][wv] = s + (wv == 0 ? carry : 0u);
      }
      rz++;
    } else {
      // a = 0: q[j] = p[j + 1]; the thread's last quotient byte is the next thread's first coefficient
      kzgo::shift16(nb, base + 16 < len ? p[base + 16] : 0u, kzgo::PackInto{o});
    }
    const uint32_t s = plk_wave_sum(dot16(l, o) % ORD);   // (dot16 <= 16 x 101 x 255 < 2^19; the sum <= 64 x 101)
    if (lane == 0) psum[r][wv] = s;
  }
  const uint32_t anybad = __ballot(bad) != 0 ? 1u : 0u;
  if (lane == 0) pbad[wv] = anybad;
  __syncthreads();
  if (threadIdx.x >= r) return;   // one thread per point from here (r = |S| <= 17)
  const uint32_t e = P.job + threadIdx.x;
  const uint32_t s = (psum[threadIdx.x][0] + psum[threadIdx.x][1] + psum[threadIdx.x][2] + psum[threadIdx.x][3]) % ORD;
  const uint32_t flag = ((pbad[0] | pbad[1] | pbad[2] | pbad[3]) != 0 || srs_bad != 0) ? 1u : 0u;
  if (nchunk == 1)
    points_store(out, e, s, flag, exp_words);
  else
    work[P.part + threadIdx.x * nchunk + c] = s | flag << 8;
  if (c == 0) {
    const uint32_t a = point_of(mask, threadIdx.x);
    const uint32_t y = a == 0 ? p[0] % HFP
                              : (ysum[threadIdx.x][0] % HFP + ysum[threadIdx.x][1] % HFP + ysum[threadIdx.x][2] % HFP +
                                 ysum[threadIdx.x][3] % HFP) % HFP;
    out.ys[e] = (uint8_t)y;
    if (out.zs) out.zs[e] = (uint8_t)a;
  }
}

// Wave (4 blockIdx.x + wave) = the point's rank in the set of polynomial blockIdx.y: the job's nchunk partials.
__global__ __launch_bounds__(kzgo::T) void points_finish_kernel(PointsBatch B, const uint32_t* __restrict__ work,
                                                              PointsOut out, const uint32_t* __restrict__ exp_words) {
  const PointsPoly& P = B.p[blockIdx.y];
  const uint32_t nchunk = chunks_of(P.len);
  const uint32_t r = blockIdx.x * kzgo::WAVES + threadIdx.x / PLK_WAVE, lane = threadIdx.x & (PLK_WAVE - 1);
  if (nchunk <= 1 || r >= (uint32_t)__builtin_popcount(P.mask)) return;   // (the whole wave)
  uint32_t s = 0, f = 0;
  for (uint32_t b = lane; b < nchunk; b += PLK_WAVE) {   // (<= 8192 words a lane: <= 8192 x 101)
    const uint32_t v = work[P.part + r * nchunk + b];
    s += v & 0xFFu;
    f |= v >> 8;
  }
  s = plk_wave_sum(s);   // (< 2^26)
  const uint32_t flag = __ballot(f != 0) != 0 ? 1u : 0u;
  if (lane == 0) points_store(out, P.job + r, s % ORD, flag, exp_words);
}

bool mask_ok(uint32_t m) { return m != 0 && (m & ~FULL_MASK) == 0; }

// workspace words of one polynomial: aggregates per non-zero point, partials per point, none for one chunk
uint64_t poly_words(size_t len, uint32_t mask) {
  const uint64_t nchunk = plk_kzg_chunks_of(len);
  if (nchunk <= 1) return 0;
  return (uint64_t)(__builtin_popcount(mask >> 1) + __builtin_popcount(mask)) * nchunk;
}

// argument checks of both forms (no device is touched; the handle is read last, by the range checks).
// *jobs: J
int check_points(const char* fn, const plk_srs* s, const void* polys, const size_t* lens, const uint32_t* sets, int n,
                 bool null_out, uint64_t* jobs) {
  if (!s || !polys || !lens || !sets || n <= 0 || null_out) {
    plk_set_error("%s: handle, arrays, outputs and n > 0 are required", fn);
    return PLK_ERR_ARG;
  }
  uint64_t J = 0, words = 0;
  for (int i = 0; i < n; i++) {
    if (lens[i] == 0) {
      plk_set_error("%s: polynomial %d is empty", fn, i);
      return PLK_ERR_ARG;
    }
    if (!mask_ok(sets[i])) {
      plk_set_error("%s: polynomial %d: the set 0x%x is not 1 .. %d points of GF(17)", fn, i, (unsigned)sets[i], NPTS);
      return PLK_ERR_ARG;
    }
    J += (uint64_t)__builtin_popcount(sets[i]);
  }
  int rc;
  for (int i = 0; i < n; i++) {
    if ((rc = plk_kzg_check_record_len(fn, "polynomial", i, lens[i])) ||
        (rc = plk_kzg_check_srs_len(s, std::max<size_t>(lens[i] - 1, 1))))
      return rc;
    words += poly_words(lens[i], sets[i]);
  }
  if (J > POINTS_MAX_JOBS) {
    plk_set_error("%s: %llu jobs exceed 2^30 per call", fn, (unsigned long long)J);
    return PLK_ERR_RANGE;
  }
  if (words > 0xFFFFFFFFull) {
    plk_set_error("%s: the call's workspace exceeds 2^34 bytes", fn);
    return PLK_ERR_RANGE;
  }
  *jobs = J;
  return plk_kzg_check_device(fn, s);
}

// the launches of a call: POINTS_POLYS polynomials per launch of each kernel, consecutive on the stream
int launch_points(const plk_srs* s, const uint8_t* const* d_polys, const size_t* lens, const uint32_t* sets, int n,
                  const PointsOut& out, uint32_t* d_work, hipStream_t st) {
  const char* fn = "plk_kzg_open_points_batch_dev";
  for (int i = 0; i < n; i++) {
    if (!d_polys[i]) {
      plk_set_error("%s: polynomial %d is NULL", fn, i);
      return PLK_ERR_ARG;
    }
  }
  uint32_t word = 0, job = 0;
  for (int i0 = 0; i0 < n; i0 += POINTS_POLYS) {
    const int np = std::min(POINTS_POLYS, n - i0);
    PointsBatch B;
    memset(&B, 0, sizeof B);
    uint32_t maxc = 1, maxpts = 1, maxnz = 0;
    for (int j = 0; j < np; j++) {
      const int i = i0 + j;
      PointsPoly& P = B.p[j];
      const uint32_t nchunk = (uint32_t)plk_kzg_chunks_of(lens[i]);
      const uint32_t t = (uint32_t)__builtin_popcount(sets[i]), tz = (uint32_t)__builtin_popcount(sets[i] >> 1);
      P.p = d_polys[i];
      P.len = lens[i];
      P.mask = sets[i];
      P.job = job;
      P.agg = word;
      P.part = word + (nchunk > 1 ? tz * nchunk : 0u);
      word += (uint32_t)poly_words(lens[i], sets[i]);
      job += t;
      maxc = std::max(maxc, nchunk);
      if (nchunk > 1) {
        maxpts = std::max(maxpts, t);
        maxnz = std::max(maxnz, tz);
      }
    }
    if (maxc > 1) {
      if (!d_work || (uintptr_t)d_work % 4) {
        plk_set_error("%s: d_work (plk_kzg_points_workspace bytes, 4-byte aligned) is required for polynomials of more than %d coefficients",
                      fn, kzgo::CHUNK);
        return PLK_ERR_ARG;
      }
      if (maxnz > 0) {   // (sets of the point 0 alone have no aggregates)
        hipLaunchKernelGGL(points_agg_kernel, dim3(maxc - 1, np), dim3(kzgo::T), 0, st, B, d_work);
        hipLaunchKernelGGL(points_scan_kernel, dim3(maxnz, np), dim3(kzgo::T), 0, st, B, d_work);
      }
    }
    hipLaunchKernelGGL(points_open_kernel, dim3(maxc, np), dim3(kzgo::T), 0, st, B, s->d_log, d_work, out, s->exp_words,
                       s->irregular ? 1u : 0u);
    if (maxc > 1)
      hipLaunchKernelGGL(points_finish_kernel, dim3((maxpts + kzgo::WAVES - 1) / kzgo::WAVES, np), dim3(kzgo::T), 0, st, B,
                         d_work, out, s->exp_words);
    PLK_HIP(hipGetLastError());
  }
  return PLK_OK;
}

// polynomial i of the host form through plk_kzg_open_batch on its expanded jobs, as the header states the call
// (exact for every input byte and any SRS)
int compose_poly(const plk_srs* s, const uint8_t* poly, size_t len, uint32_t mask, uint8_t* ys, uint8_t* proofs3) {
  const uint8_t* pp[NPTS];
  size_t ll[NPTS];
  uint8_t zz[NPTS];
  int t = 0;
  for (uint32_t a = 0; a < NPTS; a++) {
    if (!((mask >> a) & 1u)) continue;
    pp[t] = poly;
    ll[t] = len;
    zz[t++] = (uint8_t)a;
  }
  return plk_kzg_open_batch(s, pp, ll, zz, t, ys, proofs3);
}

// the host-buffer form: one fused call over uploaded polynomials; a polynomial with a flagged job (a coefficient
// byte >= 17), and every polynomial of an irregular SRS, takes the composition
int host_points(const plk_srs* s, const uint8_t* const* polys, const size_t* lens, const uint32_t* sets, int n, size_t J,
                uint8_t* zs, uint8_t* ys, uint8_t* proofs3) {
  const char* fn = "plk_kzg_open_points_batch";
  size_t poly_bytes;
  const int null_at = plk_kzg_arena_bytes(polys, lens, n, &poly_bytes);
  if (null_at >= 0) {
    plk_set_error("%s: polynomial %d is NULL", fn, null_at);
    return PLK_ERR_ARG;
  }
  std::vector<uint8_t> status(J, 1);
  if (!s->irregular) {
    // the arena, then zs, ys, status (J each) and proofs (3 J), then the workspace
    const size_t o_out = plk_pad16(poly_bytes), o_work = plk_pad16(o_out + 6 * J), total = o_work + plk_kzg_points_workspace(lens, sets, n);
    PlkScratch S;
    int rc = S.alloc(fn, total);
    if (rc) return rc;
    const PointsOut out{S.d + o_out, S.d + o_out + J, S.d + o_out + 3 * J, S.d + o_out + 2 * J};
    std::vector<const uint8_t*> dp;
    if ((rc = plk_kzg_upload(S, polys, lens, n, s->st, dp)) ||
        (rc = launch_points(s, dp.data(), lens, sets, n, out, (uint32_t*)(S.d + o_work), s->st)))
      return rc;
    PLK_HIP(hipMemcpyAsync(ys, out.ys, J, hipMemcpyDeviceToHost, s->st));
    PLK_HIP(hipMemcpyAsync(status.data(), out.status, J, hipMemcpyDeviceToHost, s->st));
    PLK_HIP(hipMemcpyAsync(proofs3, out.proofs3, 3 * J, hipMemcpyDeviceToHost, s->st));
    PLK_HIP(hipStreamSynchronize(s->st));
  }
  size_t e = 0;
  for (int i = 0; i < n; i++) {
    const size_t t = (size_t)__builtin_popcount(sets[i]);
    if (status[e]) {   // (a polynomial's jobs are flagged together)
      const int rc = compose_poly(s, polys[i], lens[i], sets[i], ys + e, proofs3 + 3 * e);
      if (rc) return rc;
    }
    if (zs) {
      size_t k = e;
      for (uint32_t a = 0; a < NPTS; a++)
        if ((sets[i] >> a) & 1u) zs[k++] = (uint8_t)a;
    }
    e += t;
  }
  return PLK_OK;
}

}  // namespace

extern "C" {

size_t plk_kzg_points_count(const uint32_t* sets, int n) {
  if (!sets || n <= 0) return 0;
  uint64_t J = 0;
  for (int i = 0; i < n; i++) {
    if (!mask_ok(sets[i])) return 0;
    J += (uint64_t)__builtin_popcount(sets[i]);
  }
  return (size_t)J;
}

size_t plk_kzg_points_workspace(const size_t* lens, const uint32_t* sets, int n) {
  if (!lens || !sets || n <= 0) return 0;
  uint64_t words = 0;
  for (int i = 0; i < n; i++) {
    if (lens[i] == 0 || lens[i] > PLK_KZG_RECORD_MAX_LEN || !mask_ok(sets[i])) return 0;
    words += poly_words(lens[i], sets[i]);
  }
  return (size_t)((4 * words + 255) & ~255ull);
}

int plk_kzg_open_points_batch_dev(const plk_srs_t* s, const uint8_t* const* d_polys, const size_t* lens, const uint32_t* sets,
                                  int n, uint8_t* d_zs, uint8_t* d_ys, uint8_t* d_proofs3, uint8_t* d_status, void* d_work,
                                  void* stream) {
  uint64_t J = 0;
  int rc = check_points("plk_kzg_open_points_batch_dev", s, d_polys, lens, sets, n, !d_ys || !d_proofs3 || !d_status, &J);
  if (rc) return rc;
  return launch_points(s, d_polys, lens, sets, n, PointsOut{d_zs, d_ys, d_proofs3, d_status}, (uint32_t*)d_work,
                       (hipStream_t)stream);
}

int plk_kzg_open_points_batch(const plk_srs_t* s, const uint8_t* const* polys, const size_t* lens, const uint32_t* sets, int n,
                              uint8_t* zs, uint8_t* ys, uint8_t* proofs3) {
  uint64_t J = 0;
  int rc = check_points("plk_kzg_open_points_batch", s, polys, lens, sets, n, !ys || !proofs3, &J);
  if (rc) return rc;
  return host_points(s, polys, lens, sets, n, (size_t)J, zs, ys, proofs3);
}

}  // extern "C"
