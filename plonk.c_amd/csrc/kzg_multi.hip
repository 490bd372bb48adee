// KZG multi-point openings (include/plonkhip.h, "KZG multi-point openings"): k <= 15 polynomials, each
// opened at its own set S_i of GF(17) points, two G1 elements per group.
//
//   W  = [h],  h = sum_i w_i q_i,  q_i = p_i div Z_i,  Z_i = prod_{a in S_i} (x - a)
//   W' = the folded opening at u of (p_0 .. p_{k-1}, h) under (c_0 .. c_{k-1}, -c_T)
//
// Partial fractions turn every q_i into single-point quotients, q_i = sum_{a in S_i} lambda_ia (p_i - p_i(a)) / (x - a)
// with lambda_ia = 1 / prod_{b in S_i, b != a} (a - b), and division by x - a is linear in the numerator, so
//
//   h = sum_{a in T} (G_a - G_a(a)) / (x - a),   G_a = sum_{i : a in S_i} (w_i lambda_ia mod 17) p_i,   T = union S_i
//
// -- at most 17 single-point quotients per group however many (polynomial, point) pairs there are.  Each is
// what the opening kernel of kzg.hip forms, by the same device pieces (plk_kzg_open.h: suffix_carry and
// quotient16 for a != 0, shift16 for a = 0, then store16 and the finish; host side plk_kzg_host.h).
// The launches of a call, four whole groups at a time:
//   multi_agg_kernel   only when some polynomial exceeds one chunk; block (chunk >= 1, group): one word per
//                      (polynomial, point a != 0 of its set, chunk) = sum_j p[j] a^(j mod 16) mod 17 with the
//                      >= 17 flag in bit 8 (the polynomial's bytes loaded once for all its points), and one
//                      folded word per (group, point of T, chunk) = sum_i (w_i lambda_ia) agg_ia mod 17
//   multi_open_kernel  block (chunk, group): the polynomials' sixteen bytes per thread loaded once and
//                      transposed four polynomials to a word; per point of T (a rolled loop, the point's
//                      constants uniform) G_a's bytes by v_dot4_u32_u8, the carry, the sixteen quotient bytes
//                      in registers, added into h's sixteen sums; one mod17 per coefficient, the dot product
//                      with the SRS logs and the ticketed finish on record 2g; h stored once.  The chunk-0
//                      block writes every y_ia = p_i(a) (its own chunk's sum plus the aggregate words) and
//                      the 0xFF filler.  No q_i and no G_a ever reaches memory.
//   then the folded opening of kzg.hip, unchanged, on (p_0 .. p_{k-1}, h) with weights c, record 2g + 1, one
//   group per call of its launcher (its records are consecutive, ours alternate).
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
constexpr int NPTS = 17;                              // GF(17) points
constexpr int MULTI_GROUPS = 4;                       // whole groups per launch
constexpr int MULTI_POLYS = MULTI_GROUPS * PLK_KZG_MULTI_MAX;
constexpr uint32_t FULL_MASK = (1u << NPTS) - 1;
using hf17::any_noncanonical;
using hf17::mod17;
using kzgo::dot16;
using kzgo::packed_powers;

struct MultiPoly {
  const uint8_t* p;
  uint64_t len;
  uint32_t work;   // first word of the polynomial's aggregates: word (a - 1) nchunk + c, nchunk the group's
  uint32_t mask;   // S_i
};
struct MultiGroup {
  uint8_t* h;        // Lh bytes
  uint64_t lh;
  uint32_t first, k;
  uint32_t work;     // first word of the group's folded aggregates, indexed as a polynomial's
  uint32_t nchunk;   // chunks of the longest polynomial (>= those of Lh)
  uint32_t tmask;    // T
  uint32_t pad;
  uint32_t wpk[NPTS][4];   // per point a: w_i lambda_ia mod 17 of polynomial i in byte i & 3 of word i >> 2 (0: a not in S_i)
};
struct MultiBatch {
  MultiPoly p[MULTI_POLYS];
  MultiGroup g[MULTI_GROUPS];
};
static_assert(sizeof(MultiBatch) <= 3072, "the batch travels as a kernel argument");

// Coefficients [base, base + 16) of polynomials i0 .. i0 + NB - 1 of group G, zero past a polynomial's end
// and in the slots past k.  Decided per polynomial, so a ragged group keeps its long polynomials on the fast
// path: first every polynomial that is aligned and holds the whole run takes one vector load (predicated, all
// in flight together), then the few runs left -- a polynomial's last partial run, an unaligned polynomial --
// go byte by byte (kzgo::load16_rolled).  kzg.hip's fold_load decides once for the whole group instead; the
// two policies issue different loads for a ragged group, so each file keeps its own.
template <int NB>
__device__ __forceinline__ void multi_load(const MultiBatch& B, const MultiGroup& G, uint32_t i0, uint64_t base,
                                           uint32_t (&w)[NB][4]) {
#pragma unroll
  for (int u = 0; u < NB; u++) {
    w[u][0] = w[u][1] = w[u][2] = w[u][3] = 0;
    if (i0 + u < G.k) {   // (uniform)
      const MultiPoly& P = B.p[G.first + i0 + u];
      if (kzgo::aligned16(P.p) && base + 16 <= P.len) kzgo::load16_vec(P.p, base, w[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < NB; u++) {
    if (i0 + u < G.k) {   // (uniform)
      const MultiPoly& P = B.p[G.first + i0 + u];
      if (!(kzgo::aligned16(P.p) && base + 16 <= P.len) && base < P.len) kzgo::load16_rolled(P.p, P.len, base, w[u]);
    }
  }
}

__device__ __forceinline__ uint32_t point_weight(const MultiGroup& G, uint32_t a, uint32_t i) {
  return (G.wpk[a][i >> 2] >> (8 * (i & 3))) & 0xFFu;
}

// Aggregates of chunk blockIdx.x + 1 of group blockIdx.y (see the head of this file).
constexpr int AGG_NB = 4;
__global__ __launch_bounds__(kzgo::T) void multi_agg_kernel(MultiBatch B, uint32_t* __restrict__ work) {
  __shared__ uint32_t psum[PLK_KZG_MULTI_MAX][NPTS - 1][kzgo::WAVES];   // per wave: the sum mod 17
  __shared__ uint32_t pbad[PLK_KZG_MULTI_MAX][kzgo::WAVES];
  __shared__ uint32_t pfin[PLK_KZG_MULTI_MAX][NPTS - 1];
  const MultiGroup& G = B.g[blockIdx.y];
  const uint32_t c = blockIdx.x + 1;
  if (c >= G.nchunk) return;
  const uint32_t lane = threadIdx.x & (PLK_WAVE - 1), wv = threadIdx.x / PLK_WAVE;
  const uint64_t base = (uint64_t)c * kzgo::CHUNK + (uint64_t)threadIdx.x * kzgo::E;
  for (uint32_t i0 = 0; i0 < G.k; i0 += AGG_NB) {   // (uniform)
    uint32_t w[AGG_NB][4];
    multi_load<AGG_NB>(B, G, i0, base, w);
#pragma unroll
    for (int u = 0; u < AGG_NB; u++) {
      if (i0 + u < G.k) {   // (uniform)
        const uint32_t i = i0 + u;
        const uint32_t anybad = __ballot(any_noncanonical(w[u])) != 0 ? 1u : 0u;
        if (lane == 0) pbad[i][wv] = anybad;
        for (uint32_t m = B.p[G.first + i].mask >> 1; m; m &= m - 1) {   // (uniform) the non-zero points of S_i
          const uint32_t a = (uint32_t)__builtin_ctz(m) + 1;
          uint32_t pk[4];
          packed_powers(a, pk);
          const uint32_t s = plk_wave_sum(dot16(w[u], pk));   // (<= 64 x 16 x 255 x 16)
          if (lane == 0) psum[i][a - 1][wv] = s % HFP;
        }
      }
    }
  }
  __syncthreads();
  {
    const uint32_t i = threadIdx.x / (NPTS - 1), a = threadIdx.x % (NPTS - 1) + 1;
    if (i < G.k) {   // (kzgo::T >= 15 x 16)
      const MultiPoly& P = B.p[G.first + i];
      uint32_t s = 0;
      if ((P.mask >> a) & 1u) {
        s = (psum[i][a - 1][0] + psum[i][a - 1][1] + psum[i][a - 1][2] + psum[i][a - 1][3]) % HFP;
        const uint32_t anybad = (pbad[i][0] | pbad[i][1] | pbad[i][2] | pbad[i][3]) != 0 ? 1u : 0u;
        work[P.work + (a - 1) * G.nchunk + c] = s | anybad << 8;
      }
      pfin[i][a - 1] = s;
    }
  }
  __syncthreads();
  if (threadIdx.x < NPTS - 1) {
    const uint32_t a = threadIdx.x + 1;
    if ((G.tmask >> a) & 1u) {
      uint32_t fold = 0, badall = 0;
      for (uint32_t i = 0; i < G.k; i++) {
        fold += point_weight(G, a, i) * pfin[i][a - 1];   // (<= 15 x 16 x 16 in all)
        badall |= pbad[i][0] | pbad[i][1] | pbad[i][2] | pbad[i][3];
      }
      work[G.work + (a - 1) * G.nchunk + c] = fold % HFP | (badall != 0 ? 1u : 0u) << 8;
    }
  }
}

// Block (chunk, group) of a multi-point opening: see the head of this file.  NB = 4, 8, 12 or 16: the smallest
// that holds the launch's largest group.  srs_bad: the SRS has no log form (every record is then flagged; ys
// and h are still exact).  res: the launch's first W record (group y at res + 2 y).
template <int NB>
__global__ __launch_bounds__(kzgo::T) void multi_open_kernel(MultiBatch B, const uint8_t* __restrict__ logs,
                                                       const uint32_t* __restrict__ work, uint8_t* __restrict__ ys,
                                                       PlkMsmResult* res, const uint32_t* __restrict__ exp_words,
                                                       uint32_t srs_bad, uint32_t row0) {
  __shared__ kzgo::Finish fin;
  __shared__ uint32_t ws[2][2 * kzgo::WAVES];   // suffix_carry's words, alternating from point to point
  __shared__ uint32_t ysum[PLK_KZG_MULTI_MAX][NPTS][kzgo::WAVES];
  const MultiGroup& G = B.g[blockIdx.y];
  const uint32_t c = blockIdx.x;
  if (c >= G.nchunk) return;
  fin.stage(exp_words);
  const uint64_t base = (uint64_t)c * kzgo::CHUNK + (uint64_t)threadIdx.x * kzgo::E;
  const uint32_t wv = threadIdx.x / PLK_WAVE, lane = threadIdx.x & (PLK_WAVE - 1);
  bool bad = srs_bad != 0;
  // tr[q][j]: byte j of polynomials 4q .. 4q + 3, polynomial 4q + u in byte u
  uint32_t tr[NB / 4][kzgo::E];
  {
    uint32_t w[NB][4];
    multi_load<NB>(B, G, 0, base, w);
#pragma unroll
    for (int u = 0; u < NB; u++) bad |= u < (int)G.k && any_noncanonical(w[u]);
    if (c == 0) {   // (uniform) y_ia: this thread's share of p_i(a), a != 0 (a^16 = 1 needs a != 0)
      for (uint32_t a = 1; a < NPTS; a++) {
        if (!((G.tmask >> a) & 1u)) continue;
        uint32_t pk[4];
        packed_powers(a, pk);
#pragma unroll
        for (int u = 0; u < NB; u++) {
          if (u < (int)G.k && ((B.p[G.first + u].mask >> a) & 1u)) {   // (uniform)
            const MultiPoly& P = B.p[G.first + u];
            uint32_t v = dot16(w[u], pk);   // (<= 16 x 255 x 16)
            for (uint32_t b = 1 + threadIdx.x; b < G.nchunk; b += kzgo::T) v += work[P.work + (a - 1) * G.nchunk + b] & 0xFFu;
            const uint32_t s = plk_wave_sum(v);
            if (lane == 0) ysum[u][a][wv] = s;
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < NB / 4; q++)
#pragma unroll
      for (int m = 0; m < 4; m++)
#pragma unroll
        for (int j = 0; j < 4; j++)
          tr[q][4 * m + j] = kzgo::transpose4(w[4 * q][m], w[4 * q + 1][m], w[4 * q + 2][m], w[4 * q + 3][m], j);
  }
  uint32_t hacc[kzgo::E];   // sum over the points of T of the quotient bytes (<= 17 x 16)
#pragma unroll
  for (int j = 0; j < kzgo::E; j++) hacc[j] = 0;
  const auto add = [&hacc](int j, uint32_t q) { hacc[j] += q; };
  uint32_t par = 0;
  for (uint32_t m = G.tmask; m; m &= m - 1) {   // (uniform) the points of T
    const uint32_t a = (uint32_t)__builtin_ctz(m);
    // G_a's sixteen canonical bytes: sum_i weight x byte <= 15 x 16 x 255 = 61200, inside mod17's range
    uint32_t nb[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < kzgo::E; j++) {
      uint32_t t = 0;
#pragma unroll
      for (int q = 0; q < NB / 4; q++) t = __builtin_amdgcn_udot4(tr[q][j], G.wpk[a][q], t, false);
      nb[j >> 2] |= mod17(t) << (8 * (j & 3));
    }
    if (a != 0) {
      uint32_t pk[4];
      packed_powers(a, pk);
      const uint32_t tot = mod17(dot16(nb, pk));   // (<= 16 x 16 x 16)
      const uint32_t run = kzgo::suffix_carry(tot, work + G.work + (a - 1) * G.nchunk, c, G.nchunk, ws[par], bad);
      par ^= 1u;   // (the next point's words: a wave may arrive there while another still reads these)
      kzgo::quotient16(nb, a, run, add);
    } else {
      // a = 0: q[j] = G_0[j + 1]; the thread's last quotient byte is G_0[base + 16], folded from the
      // polynomials' bytes (the next thread's, or the next chunk's, first coefficient)
      uint32_t sn = 0;
      for (uint32_t i = 0; i < G.k; i++) {
        const MultiPoly& P = B.p[G.first + i];
        const uint32_t wt = point_weight(G, 0, i);
        if (wt != 0 && base + 16 < P.len) sn += wt * P.p[base + 16];
      }
      kzgo::shift16(nb, mod17(sn), add);   // (<= 61200)
    }
  }
  // h's sixteen canonical bytes, nothing past Lh (there the sums cancel mod 17 for canonical input)
  const uint64_t lh = G.lh;
  uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < kzgo::E; j++) o[j >> 2] |= (base + j < lh ? mod17(hacc[j]) : 0u) << (8 * (j & 3));   // (hacc <= 272)
  if (c == 0) {
    __syncthreads();   // (uniform) ysum is complete
    const uint32_t i = threadIdx.x / NPTS, a = threadIdx.x % NPTS;
    if (i < G.k) {   // (kzgo::T >= 15 x 17)
      const MultiPoly& P = B.p[G.first + i];
      uint32_t y = 0xFFu;
      if ((P.mask >> a) & 1u)
        y = a == 0 ? P.p[0] % HFP
                   : (ysum[i][a][0] % HFP + ysum[i][a][1] % HFP + ysum[i][a][2] % HFP + ysum[i][a][3] % HFP) % HFP;
      ys[(size_t)NPTS * (G.first + i) + a] = (uint8_t)y;
    }
  }
  if (base < lh) kzgo::store16(G.h, lh, base, kzgo::aligned16(G.h), o);
  fin.finish(kzgo::Finish::logs(logs, srs_bad, base, lh), o, bad, res + 2 * blockIdx.y, c, G.nchunk, row0 + blockIdx.y);
}

bool mask_ok(uint32_t m) { return m != 0 && (m & ~FULL_MASK) == 0 && m != FULL_MASK; }
uint32_t inv17(uint32_t a) {
  uint32_t r = 1;
  for (int i = 0; i < 15; i++) r = r * a % HFP;   // a^15
  return r;
}
// prod_{a in m} (u - a) mod 17
uint32_t vanish_at(uint32_t m, uint32_t u) {
  uint32_t r = 1;
  for (uint32_t a = 0; a < NPTS; a++)
    if ((m >> a) & 1u) r = r * ((u + HFP - a) % HFP) % HFP;
  return r;
}

// the lengths of group g: the longest polynomial and Lh = max_i max(len_i - t_i, 1)
struct GroupLens {
  uint64_t maxlen, lh;
};
GroupLens group_lens(const size_t* lens, const uint32_t* sets, const int* start, int g) {
  GroupLens L{0, 1};
  for (int i = start[g]; i < start[g + 1]; i++) {
    const uint64_t t = (uint64_t)__builtin_popcount(sets[i]);
    L.maxlen = std::max<uint64_t>(L.maxlen, lens[i]);
    if (lens[i] > t) L.lh = std::max<uint64_t>(L.lh, lens[i] - t);
  }
  return L;
}

// The workspace of group g, in bytes from the group's start (every part a multiple of 16):
//   [0, 32)   the ys of the folded opening (k + 1 bytes, not returned)
//   h         Lh bytes
//   agg       (k + 1) x 16 x nchunk words of multi_agg_kernel (none when the group is one chunk)
//   fold      the workspace of the folded opening of (p_0 .. p_{k-1}, h)
struct GroupWork {
  size_t o_h, o_agg, o_fold, total;
};
GroupWork group_work(const size_t* lens, const uint32_t* sets, const int* start, int g) {
  const GroupLens L = group_lens(lens, sets, start, g);
  const int k = start[g + 1] - start[g];
  const uint64_t nchunk = plk_kzg_chunks_of(L.maxlen);
  size_t fl[PLK_KZG_FOLD_MAX];
  for (int i = 0; i < k; i++) fl[i] = lens[start[g] + i];
  fl[k] = (size_t)L.lh;
  const int one[2] = {0, k + 1};
  GroupWork W;
  W.o_h = 32;
  W.o_agg = W.o_h + plk_pad16((size_t)L.lh) + 16;
  W.o_fold = W.o_agg + (nchunk > 1 ? (size_t)(k + 1) * (NPTS - 1) * nchunk * 4 : 0);
  W.total = W.o_fold + plk_kzg_fold_workspace(fl, one, 1);
  return W;
}

// argument checks of the opening (no device is touched; the handle is read last, by the range checks)
int check_multi(const char* fn, const plk_srs* s, const void* polys, const size_t* lens, const uint32_t* sets,
                const uint8_t* weights, const int* start, const uint8_t* us, int ngroups, bool null_out) {
  if (!s || !polys || !lens || !sets || !weights || !start || !us || ngroups <= 0 || null_out) {
    plk_set_error("%s: handle, arrays, outputs and ngroups > 0 are required", fn);
    return PLK_ERR_ARG;
  }
  if (!plk_kzg_layout_ok(start, ngroups, PLK_KZG_MULTI_MAX)) {
    plk_set_error("%s: start must rise strictly from 0 by at most %d polynomials a group", fn, PLK_KZG_MULTI_MAX);
    return PLK_ERR_ARG;
  }
  for (int g = 0; g < ngroups; g++) {
    if (us[g] >= HFP) {
      plk_set_error("%s: group %d: u = %u is not a GF(17) value", fn, g, (unsigned)us[g]);
      return PLK_ERR_ARG;
    }
    for (int i = start[g]; i < start[g + 1]; i++) {
      if (lens[i] == 0) {
        plk_set_error("%s: polynomial %d is empty", fn, i);
        return PLK_ERR_ARG;
      }
      if (!mask_ok(sets[i])) {
        plk_set_error("%s: polynomial %d: the set 0x%x is not 1 .. %d points of GF(17)", fn, i, (unsigned)sets[i],
                      PLK_KZG_MULTI_POINTS);
        return PLK_ERR_ARG;
      }
      if (weights[i] >= HFP) {
        plk_set_error("%s: polynomial %d: weight %u is not a GF(17) value", fn, i, (unsigned)weights[i]);
        return PLK_ERR_ARG;
      }
    }
  }
  int rc;
  for (int i = 0; i < start[ngroups]; i++)
    if ((rc = plk_kzg_check_record_len(fn, "polynomial", i, lens[i]))) return rc;
  for (int g = 0; g < ngroups; g++) {
    const GroupLens L = group_lens(lens, sets, start, g);
    const uint64_t need = std::max<uint64_t>(L.lh, std::max<uint64_t>(L.maxlen - 1, 1));   // (Lh <= the longest length)
    if ((rc = plk_kzg_check_srs_len(s, (size_t)need))) return rc;
  }
  return plk_kzg_check_device(fn, s);
}

// c[0 .. k) = w_i prod_{a in T \ S_i} (u - a), c[k] = -prod_{a in T} (u - a) (arguments checked by the caller)
void multi_coeffs(const uint32_t* sets, const uint8_t* weights, int k, uint32_t u, uint8_t* c) {
  uint32_t T = 0;
  for (int i = 0; i < k; i++) T |= sets[i];
  for (int i = 0; i < k; i++) c[i] = (uint8_t)(weights[i] * vanish_at(T & ~sets[i], u) % HFP);
  c[k] = (uint8_t)((HFP - vanish_at(T, u)) % HFP);
}

// the launches of a call: MULTI_GROUPS whole groups per launch of our kernels, consecutive on the stream,
// then the folded opening group by group
int launch_multi(const plk_srs* s, const uint8_t* const* d_polys, const size_t* lens, const uint32_t* sets,
                 const uint8_t* weights, const int* start, const uint8_t* us, int ngroups, uint8_t* d_ys,
                 PlkMsmResult* d_res, uint8_t* const* d_hs, uint8_t* d_work, hipStream_t st) {
  if (!d_work) {
    plk_set_error("plk_kzg_open_multi_batch_dev: d_work is required");
    return PLK_ERR_ARG;
  }
  for (int i = 0; i < start[ngroups]; i++) {
    if (!d_polys[i]) {
      plk_set_error("plk_kzg_open_multi_batch: polynomial %d is NULL", i);
      return PLK_ERR_ARG;
    }
  }
  std::vector<size_t> off(ngroups + 1, 0);
  for (int g = 0; g < ngroups; g++) off[g + 1] = off[g] + group_work(lens, sets, start, g).total;
  if (off[ngroups] / 4 > 0xFFFFFFFFull) {
    plk_set_error("plk_kzg_open_multi_batch: the call's workspace exceeds 2^34 bytes");
    return PLK_ERR_RANGE;
  }
  uint32_t* words = (uint32_t*)d_work;
  const uint32_t bad = s->irregular ? 1u : 0u;
  for (int g0 = 0; g0 < ngroups; g0 += MULTI_GROUPS) {
    const int ng = std::min(MULTI_GROUPS, ngroups - g0);
    MultiBatch B;
    memset(&B, 0, sizeof B);
    uint32_t maxc = 1, maxk = 1, np = 0;
    for (int j = 0; j < ng; j++) {
      const int g = g0 + j, k = start[g + 1] - start[g];
      const GroupLens L = group_lens(lens, sets, start, g);
      const GroupWork W = group_work(lens, sets, start, g);
      MultiGroup& G = B.g[j];
      G.h = d_hs && d_hs[g] ? d_hs[g] : d_work + off[g] + W.o_h;
      G.lh = L.lh;
      G.first = np;
      G.k = (uint32_t)k;
      G.nchunk = (uint32_t)plk_kzg_chunks_of(L.maxlen);
      const uint32_t agg0 = (uint32_t)((off[g] + W.o_agg) / 4), per = (NPTS - 1) * G.nchunk;
      G.work = agg0 + (uint32_t)k * per;
      for (int i = 0; i < k; i++, np++) {
        const int f = start[g] + i;
        MultiPoly& P = B.p[np];
        P.p = d_polys[f];
        P.len = lens[f];
        P.work = agg0 + (uint32_t)i * per;
        P.mask = sets[f];
        G.tmask |= sets[f];
        for (uint32_t a = 0; a < NPTS; a++) {
          if (!((sets[f] >> a) & 1u)) continue;
          uint32_t d = 1;   // prod_{b in S_i, b != a} (a - b)
          for (uint32_t b = 0; b < NPTS; b++)
            if (b != a && ((sets[f] >> b) & 1u)) d = d * ((a + HFP - b) % HFP) % HFP;
          G.wpk[a][i >> 2] |= (weights[f] * inv17(d) % HFP) << (8 * (i & 3));
        }
      }
      maxc = std::max(maxc, G.nchunk);
      maxk = std::max(maxk, G.k);
    }
    if (maxc > 1) hipLaunchKernelGGL(multi_agg_kernel, dim3(maxc - 1, ng), dim3(kzgo::T), 0, st, B, words);
    const auto open = maxk <= 4 ? multi_open_kernel<4> : maxk <= 8 ? multi_open_kernel<8> : maxk <= 12 ? multi_open_kernel<12> : multi_open_kernel<16>;
    hipLaunchKernelGGL(open, dim3(maxc, ng), dim3(kzgo::T), 0, st, B, s->d_log, words, d_ys + (size_t)NPTS * start[g0],
                       d_res + 2 * (size_t)g0, s->exp_words, bad, 2u * (uint32_t)g0);
    PLK_HIP(hipGetLastError());
  }
  for (int g = 0; g < ngroups; g++) {
    const int k = start[g + 1] - start[g];
    const GroupLens L = group_lens(lens, sets, start, g);
    const GroupWork W = group_work(lens, sets, start, g);
    const uint8_t* fp[PLK_KZG_FOLD_MAX];
    size_t fl[PLK_KZG_FOLD_MAX];
    uint8_t c[PLK_KZG_FOLD_MAX];
    for (int i = 0; i < k; i++) {
      fp[i] = d_polys[start[g] + i];
      fl[i] = lens[start[g] + i];
    }
    fp[k] = d_hs && d_hs[g] ? d_hs[g] : d_work + off[g] + W.o_h;
    fl[k] = (size_t)L.lh;
    multi_coeffs(sets + start[g], weights + start[g], k, us[g], c);
    const int one[2] = {0, k + 1};
    const int rc = plk_kzg_fold_launch(s, fp, fl, c, one, us + g, 1, d_work + off[g], d_res + 2 * (size_t)g + 1, nullptr,
                                       (uint32_t*)(d_work + off[g] + W.o_fold), st, 2u * (uint32_t)g + 1u);
    if (rc) return rc;
  }
  return PLK_OK;
}

// One group through the public host calls, as the header states the opening (exact for every input byte
// and any SRS).
int compose_group(const plk_srs* s, const uint8_t* const* polys, const size_t* lens, const uint32_t* sets,
                  const uint8_t* weights, int k, uint8_t u, uint8_t* ys, uint8_t* proofs6) {
  std::vector<std::vector<uint8_t>> den(k), quot(k), rem(k);
  std::vector<plk_divshort_job_t> jobs(k);
  std::vector<plk_lc_term_t> terms(k);
  std::vector<size_t> ql(k), rl(k);
  size_t lh = 1;
  int rc;
  for (int i = 0; i < k; i++) {
    uint8_t roots[NPTS];
    int t = 0;
    memset(ys + NPTS * i, 0xFF, NPTS);
    for (uint32_t a = 0; a < NPTS; a++) {
      if (!((sets[i] >> a) & 1u)) continue;
      roots[t++] = (uint8_t)a;
      if ((rc = plk_poly_eval(polys[i], lens[i], (uint8_t)a, ys + NPTS * i + a))) return rc;
    }
    den[i].resize(t + 1);
    if ((rc = plk_poly_from_roots(roots, t, den[i].data()))) return rc;
    const size_t dl = (size_t)t + 1, nq = lens[i] >= dl ? lens[i] - dl + 1 : 1;
    quot[i].assign(nq, 0);
    rem[i].assign(std::min(dl - 1, lens[i]), 0);
    jobs[i] = plk_divshort_job_t{polys[i], lens[i], den[i].data(), dl, quot[i].data(), rem[i].data()};
    terms[i] = plk_lc_term_t{quot[i].data(), nq, 0, 0, weights[i], 0, 0};
    lh = std::max(lh, nq);
  }
  if ((rc = plk_poly_divide_short_batch(jobs.data(), k, ql.data(), rl.data()))) return rc;
  std::vector<uint8_t> h(lh);
  const plk_lc_job_t lc{terms.data(), k, -1, h.data()};
  size_t hl = 0;
  if ((rc = plk_poly_lincomb(&lc, &hl))) return rc;
  const uint8_t* hp = h.data();
  if ((rc = plk_kzg_commit_batch(s, &hp, &hl, 1, proofs6))) return rc;
  const uint8_t* fp[PLK_KZG_FOLD_MAX];
  size_t fl[PLK_KZG_FOLD_MAX];
  uint8_t c[PLK_KZG_FOLD_MAX], fy[PLK_KZG_FOLD_MAX];
  for (int i = 0; i < k; i++) {
    fp[i] = polys[i];
    fl[i] = lens[i];
  }
  fp[k] = h.data();
  fl[k] = lh;
  multi_coeffs(sets, weights, k, u, c);
  const int one[2] = {0, k + 1};
  return plk_kzg_open_fold_batch(s, fp, fl, c, one, &u, 1, fy, proofs6 + 3);
}

// the host-buffer form: one fused call over uploaded polynomials; a group with a flagged record (a
// coefficient byte >= 17), and every group of an irregular SRS, takes the composition
int host_multi(const plk_srs* s, const uint8_t* const* polys, const size_t* lens, const uint32_t* sets,
               const uint8_t* weights, const int* start, const uint8_t* us, int ngroups, uint8_t* ys, uint8_t* proofs6) {
  const int np = start[ngroups];
  size_t poly_bytes;
  const int null_at = plk_kzg_arena_bytes(polys, lens, np, &poly_bytes);
  if (null_at >= 0) {
    plk_set_error("plk_kzg_open_multi_batch: polynomial %d is NULL", null_at);
    return PLK_ERR_ARG;
  }
  std::vector<uint32_t> irr(2 * (size_t)ngroups, 1u);
  if (!s->irregular) {
    const size_t o_res = plk_pad16(poly_bytes), o_ys = o_res + 2 * (size_t)ngroups * sizeof(PlkMsmResult),
                 o_work = plk_pad16(o_ys + (size_t)NPTS * np), total = o_work + plk_kzg_multi_workspace(lens, sets, start, ngroups);
    PlkScratch S;
    int rc = S.alloc("plk_kzg_open_multi_batch", total);
    if (rc) return rc;
    PlkMsmResult* d_res = (PlkMsmResult*)(S.d + o_res);
    PLK_HIP(hipMemsetAsync(d_res, 0, 2 * (size_t)ngroups * sizeof(PlkMsmResult), s->st));
    std::vector<const uint8_t*> dp;
    if ((rc = plk_kzg_upload(S, polys, lens, np, s->st, dp)) ||
        (rc = launch_multi(s, dp.data(), lens, sets, weights, start, us, ngroups, S.d + o_ys, d_res, nullptr, S.d + o_work,
                           s->st)))
      return rc;
    PLK_HIP(hipMemcpyAsync(ys, S.d + o_ys, (size_t)NPTS * np, hipMemcpyDeviceToHost, s->st));
    if ((rc = plk_kzg_read_records(d_res, 2 * (size_t)ngroups, s->st, irr.data(), proofs6))) return rc;
  }
  for (int g = 0; g < ngroups; g++) {
    if (!irr[2 * g] && !irr[2 * g + 1]) continue;
    const int a = start[g];
    const int rc = compose_group(s, polys + a, lens + a, sets + a, weights + a, start[g + 1] - a, us[g], ys + (size_t)NPTS * a,
                                 proofs6 + 6 * (size_t)g);
    if (rc) return rc;
  }
  return PLK_OK;
}

}  // namespace

extern "C" {

int plk_kzg_multi_coeffs(const uint32_t* sets, const uint8_t* weights, int k, uint8_t u, uint8_t* c) {
  const char* fn = "plk_kzg_multi_coeffs";
  if (!sets || !weights || !c || k < 1 || k > PLK_KZG_MULTI_MAX || u >= HFP) {
    plk_set_error("%s: arrays, k in 1 .. %d and u < 17 are required", fn, PLK_KZG_MULTI_MAX);
    return PLK_ERR_ARG;
  }
  for (int i = 0; i < k; i++) {
    if (!mask_ok(sets[i]) || weights[i] >= HFP) {
      plk_set_error("%s: entry %d: the set 0x%x or the weight %u is invalid", fn, i, (unsigned)sets[i], (unsigned)weights[i]);
      return PLK_ERR_ARG;
    }
  }
  multi_coeffs(sets, weights, k, u, c);
  return PLK_OK;
}

size_t plk_kzg_multi_workspace(const size_t* lens, const uint32_t* sets, const int* start, int ngroups) {
  if (!lens || !sets || !plk_kzg_layout_ok(start, ngroups, PLK_KZG_MULTI_MAX)) return 0;
  for (int i = 0; i < start[ngroups]; i++)
    if (lens[i] == 0 || lens[i] > PLK_KZG_RECORD_MAX_LEN || !mask_ok(sets[i])) return 0;
  size_t total = 0;
  for (int g = 0; g < ngroups; g++) total += group_work(lens, sets, start, g).total;
  return (total + 255) & ~(size_t)255;
}

int plk_kzg_open_multi_batch_dev(const plk_srs_t* s, const uint8_t* const* d_polys, const size_t* lens, const uint32_t* sets,
                                 const uint8_t* weights, const int* start, const uint8_t* us, int ngroups, uint8_t* d_ys,
                                 plk_msm_result_t* d_res, uint8_t* const* d_hs, void* d_work, void* stream) {
  int rc = check_multi("plk_kzg_open_multi_batch_dev", s, d_polys, lens, sets, weights, start, us, ngroups, !d_ys || !d_res);
  if (rc) return rc;
  return launch_multi(s, d_polys, lens, sets, weights, start, us, ngroups, d_ys, d_res, d_hs, (uint8_t*)d_work,
                      (hipStream_t)stream);
}

int plk_kzg_open_multi_batch(const plk_srs_t* s, const uint8_t* const* polys, const size_t* lens, const uint32_t* sets,
                             const uint8_t* weights, const int* start, const uint8_t* us, int ngroups, uint8_t* ys,
                             uint8_t* proofs6) {
  int rc = check_multi("plk_kzg_open_multi_batch", s, polys, lens, sets, weights, start, us, ngroups, !ys || !proofs6);
  if (rc) return rc;
  return host_multi(s, polys, lens, sets, weights, start, us, ngroups, ys, proofs6);
}

}  // extern "C"
