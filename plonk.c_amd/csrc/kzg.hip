// KZG commit and open over a resident SRS (include/plonkhip.h, "KZG over a resident SRS").
//
// plk_srs_t keeps an SRS on the device in both forms: the G1 bytes (3 B per point) and, when every
// encoding is a canonical group element, its discrete logs (1 B per point, msm.hip srs_log_kernel).
//
//   commit  job b = MSM over lens[b] points of the log SRS: one launch for a ragged batch
//                   (kzg_commit_kernel), the ticketed finish of plk_msm_finish.h per record.
//   open    job b: y = p(z), q = (p - y) / (x - z), proof = [q].  The division by x - z is the suffix
//                  sum q[j] = z^-(j+1) sum_{i>j} p[i] z^i, and z^16 = 1 in GF(17), so a 4096-coefficient
//                  chunk's weights z^(i mod 16) do not depend on the chunk: the carry into a chunk is
//                  the plain sum mod 17 of the later chunks' aggregates.  Two launches:
//                    kzg_agg_kernel   one word per chunk >= 1 (a wave each): sum p[i] z^(i mod 16) mod 17
//                                     (+ a flag bit when a coefficient byte is >= 17)
//                    kzg_open_kernel  block (chunk, job): carry = sum of the later aggregates, the
//                                     chunk's 4096 quotient bytes in registers, their dot product with
//                                     the SRS logs (v_dot4_u32_u8), optional quotient store, y from
//                                     chunk 0, then the ticketed finish on the job's record.
//                  A batch whose jobs all fit one chunk skips the aggregates launch.  The quotient
//                  never goes through HBM unless asked for: p is read twice (once when every job is
//                  one chunk), the logs once -- about 3 B per coefficient.
//   fold    group g: k <= 16 polynomials opened at one z with one proof under weights w: the opening
//                  of F = sum_i w_i p_i, with F formed in registers (kzg_fold_agg_kernel,
//                  kzg_fold_open_kernel; plonkhip.h, "KZG folded openings").  Every polynomial is
//                  read twice, the logs once, nothing else moves.
//   No block waits for another block: the carry comes from the previous launch, the only in-launch
//   cross-block words are the finish's tickets.
// The scan, the quotient bytes, the stores and the finish are the device pieces of plk_kzg_open.h, which
// kzg_multi.hip builds on too (here: open_quotient, the one middle of both opening kernels); the checks and the
// host-buffer forms' arena and read-back are plk_kzg_host.h.
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

constexpr int KZG_JOBS = 32;          // jobs per launch
constexpr uint32_t HFP = hf17::P;
using hf17::any_noncanonical;
using hf17::load16;
using hf17::mod17;
using kzgo::dot16;
using kzgo::packed_powers;

struct KzgJob {
  const uint8_t* p;
  uint8_t* q;        // quotient bytes wanted here (nullptr: not stored)
  uint64_t len;
  uint32_t work;     // first word of the job's chunk aggregates in the workspace
  uint32_t nchunk;
  uint32_t z;
  uint32_t vec;      // bit 0: p 16-byte aligned, bit 1: q 16-byte aligned
};
struct KzgBatch {
  KzgJob j[KZG_JOBS];
};

// kzgo::packed_powers' words from a written-out table of the sixteen powers.  Kept apart for the two
// kernels of the plain opening, whose whole call is 13-30 us: with the table their end-to-end medians fall
// on both sides of the previous code's, with packed_powers they read above it at seven of eight shapes
// (DESIGN section 17); the folded and multi-point kernels measure no slower with packed_powers and use it.
__device__ __forceinline__ void power_table_packed(uint32_t z, uint32_t (&pk)[4]) {
  uint32_t pw[16];
  pw[0] = 1;
#pragma unroll
  for (int k = 1; k < 16; k++) pw[k] = pw[k - 1] * z % HFP;
#pragma unroll
  for (int i = 0; i < 4; i++) pk[i] = pw[4 * i] | pw[4 * i + 1] << 8 | pw[4 * i + 2] << 16 | pw[4 * i + 3] << 24;
}

// Aggregates of job blockIdx.y: one wave per chunk (four 16-byte groups per lane, no LDS, no
// barrier), chunk 0 skipped -- its aggregate is never read.  One word per chunk:
// [7:0] sum_i p[i] z^(i mod 16) mod 17 over the chunk, bit 8 set when a byte is >= 17.
__global__ __launch_bounds__(kzgo::T) void kzg_agg_kernel(KzgBatch B, uint32_t* __restrict__ work) {
  const KzgJob& J = B.j[blockIdx.y];
  const uint32_t c = blockIdx.x * kzgo::WAVES + threadIdx.x / PLK_WAVE + 1;
  if (c >= J.nchunk) return;   // (the whole wave)
  uint32_t pk[4];
  power_table_packed(J.z, pk);
  const uint32_t lane = threadIdx.x & (PLK_WAVE - 1);
  constexpr int G = kzgo::CHUNK / (PLK_WAVE * kzgo::E);   // groups per lane
  uint32_t w[G][4];
#pragma unroll
  for (int i = 0; i < G; i++)
    load16(J.p, J.len, (uint64_t)c * kzgo::CHUNK + (uint64_t)(i * PLK_WAVE + lane) * kzgo::E, J.vec & 1u, w[i]);
  uint32_t acc = 0;
  bool bad = false;
#pragma unroll
  for (int i = 0; i < G; i++) {
    acc += dot16(w[i], pk);   // (<= 4 x 16 x 255 x 16)
    bad |= any_noncanonical(w[i]);
  }
  const uint32_t s = plk_wave_sum(acc % HFP);
  const uint64_t anybad = __ballot(bad);
  if (lane == 0) work[J.work + c] = s % HFP | (anybad != 0 ? 1u : 0u) << 8;
}

// The scan, the sixteen quotient bytes o and their optional store, once the thread holds its sixteen
// coefficient bytes nb (kzg_open_kernel: the polynomial's; kzg_fold_open_kernel: F's): the pieces of
// plk_kzg_open.h in order.  nxt(): coefficient base + 16, asked for only when z = 0.  Holds one barrier.
template <class Next>
__device__ __forceinline__ void open_quotient(const uint32_t (&nb)[4], const uint32_t (&pk)[4], uint32_t z, uint64_t base,
                                              uint64_t ql, uint8_t* q, bool qvec, const uint32_t* __restrict__ agg,
                                              uint32_t c, uint32_t nchunk, uint32_t* ws, bool& bad, uint32_t (&o)[4],
                                              Next nxt) {
  const uint32_t run = kzgo::suffix_carry(mod17(dot16(nb, pk)), agg, c, nchunk, ws, bad);   // (<= 16 x 255 x 16)
  o[0] = o[1] = o[2] = o[3] = 0;
  if (z != 0)
    kzgo::quotient16(nb, z, run, kzgo::PackInto{o});
  else
    kzgo::shift16(nb, nxt(), kzgo::PackInto{o});
  if (q) {
    kzgo::store16(q, ql, base, qvec, o);
    if (base == 0 && ql == 0) q[0] = 0;   // one coefficient: the quotient is {0}
  }
}

// Block (chunk, job) of an opening: see the head of this file.  srs_bad: the SRS has no log form
// (every record is then flagged; y and the quotient bytes are still exact).
__global__ __launch_bounds__(kzgo::T) void kzg_open_kernel(KzgBatch B, const uint8_t* __restrict__ logs,
                                                        const uint32_t* __restrict__ work, uint8_t* __restrict__ ys,
                                                        PlkMsmResult* res, const uint32_t* __restrict__ exp_words,
                                                        uint32_t srs_bad, uint32_t row0) {
  __shared__ kzgo::Finish fin;
  __shared__ uint32_t ws[2 * kzgo::WAVES];
  const KzgJob& J = B.j[blockIdx.y];
  const uint32_t c = blockIdx.x;
  if (c >= J.nchunk) return;
  fin.stage(exp_words);
  const uint8_t* p = J.p;
  const uint64_t len = J.len, ql = len - 1;
  const uint32_t z = J.z;
  uint32_t pk[4];
  power_table_packed(z, pk);
  // the thread's 16 consecutive coefficients [base, base + 16), base = 0 mod 16
  const uint64_t base = (uint64_t)c * kzgo::CHUNK + (uint64_t)threadIdx.x * kzgo::E;
  uint32_t nb[4];
  load16(p, len, base, J.vec & 1u, nb);
  const uint4 lg = kzgo::Finish::logs(logs, srs_bad, base, ql);
  bool bad = any_noncanonical(nb) || srs_bad;
  uint32_t o[4];
  // z = 0: the thread's last quotient byte is the next thread's first coefficient
  open_quotient(nb, pk, z, base, ql, J.q, (J.vec & 2u) != 0, work + J.work, c, J.nchunk, ws, bad, o,
                [&]() -> uint32_t { return base + 16 < len ? p[base + 16] : 0u; });
  if (base == 0) ys[blockIdx.y] = (uint8_t)(((nb[0] & 0xFFu) + z * (o[0] & 0xFFu)) % HFP);   // y = p[0] + z q[0]
  fin.finish(lg, o, bad, res + blockIdx.y, c, J.nchunk, row0 + blockIdx.y);
}

// Block (x, job) of a ragged batch of commitments: job b = MSM over its len points of the log SRS,
// one 16-point group per thread, any scalar byte (g1_mul takes the raw byte).
__global__ __launch_bounds__(kzgo::T) void kzg_commit_kernel(KzgBatch B, const uint8_t* __restrict__ logs,
                                                          PlkMsmResult* res, const uint32_t* __restrict__ exp_words,
                                                          uint32_t srs_bad, uint32_t row0) {
  __shared__ kzgo::Finish fin;
  const KzgJob& J = B.j[blockIdx.y];
  const uint32_t c = blockIdx.x;
  if (c >= J.nchunk) return;
  fin.stage(exp_words);
  const uint64_t base = (uint64_t)c * kzgo::CHUNK + (uint64_t)threadIdx.x * kzgo::E;
  uint32_t sc[4];
  load16(J.p, J.len, base, J.vec & 1u, sc);
  fin.finish(kzgo::Finish::logs(logs, srs_bad, base, J.len), sc, srs_bad != 0, res + blockIdx.y, c, J.nchunk,
             row0 + blockIdx.y);
}

// ---- folded openings: k polynomials at one point, one proof (plonkhip.h, "KZG folded openings") ----
// Group g = polynomials [first, first + k) of the launch with weights w: F[j] = sum_i w_i p_i[j] mod 17
// over L = the longest length, and the opening of (F, L, z) exactly as kzg_open_kernel computes it.
// F never exists in memory: a thread sums w_i x byte exactly (<= 16 x 16 x 255 = 65280, inside
// mod17's range), reduces once per coefficient and hands the 16 canonical bytes to the unchanged
// suffix scan.  Aggregates are linear in the bytes, so the folded aggregate of a chunk is
// sum_i w_i agg_i mod 17 for ANY coefficient bytes: quotient bytes are exact whatever the input.
constexpr int FOLD_POLYS = 32;   // polynomials per launch (>= PLK_KZG_FOLD_MAX: any group fits; at most as many groups)
static_assert(FOLD_POLYS >= PLK_KZG_FOLD_MAX, "a group is never split across launches");

struct FoldPoly {
  const uint8_t* p;
  uint64_t len;
  uint32_t work;     // first word of the polynomial's chunk aggregates (word c = chunk c, c >= 1)
  uint32_t nchunk;
};
struct FoldGroup {
  uint8_t* q;        // quotient bytes wanted here (nullptr: not stored)
  uint64_t len;      // L
  uint32_t first, k;
  uint32_t work;     // first word of the group's folded aggregates
  uint32_t nchunk;   // chunks of L
  uint32_t z;
  uint32_t vec;      // bit 1: q 16-byte aligned
  uint32_t wpk[PLK_KZG_FOLD_MAX / 4];   // the weights, four to a word (zero past k)
};
struct FoldBatch {
  FoldPoly p[FOLD_POLYS];
  FoldGroup g[FOLD_POLYS];
};

__device__ __forceinline__ uint32_t fold_weight(const FoldGroup& G, uint32_t i) { return (G.wpk[i >> 2] >> (8 * (i & 3))) & 0xFFu; }

// Coefficients [base, base + 16) of polynomials i0 .. i0 + NB - 1 of group G, zero past a polynomial's
// end.  Slots past k repeat the group's last polynomial (the callers give them weight zero and skip
// their sums), so that the common case -- all aligned and these sixteen coefficients inside each -- is
// NB vector loads in one basic block, in flight together; anything else (a base off a 16-byte
// boundary, a polynomial's last partial run, ragged lengths) goes byte by byte.
template <int NB>
__device__ __forceinline__ void fold_load(const FoldBatch& B, const FoldGroup& G, uint32_t i0, uint64_t base,
                                          uint32_t (&w)[NB][4]) {
  bool fast = true;
#pragma unroll
  for (int u = 0; u < NB; u++) {
    const FoldPoly& P = B.p[G.first + min(i0 + u, G.k - 1)];
    fast = fast && kzgo::aligned16(P.p) && base + 16 <= P.len;
  }
  if (fast) {
#pragma unroll
    for (int u = 0; u < NB; u++) kzgo::load16_vec(B.p[G.first + min(i0 + u, G.k - 1)].p, base, w[u]);
  } else {
#pragma unroll
    for (int u = 0; u < NB; u++) {
      const FoldPoly& P = B.p[G.first + min(i0 + u, G.k - 1)];
      kzgo::load16_rolled(P.p, P.len, base, w[u]);
    }
  }
}

// Aggregates of group blockIdx.y: one block per chunk c >= 1 of L, a 16-coefficient run per thread as
// in the opening, the group's polynomials NB at a time.  One word per (polynomial, chunk) as
// kzg_agg_kernel writes it, and one folded word per (group, chunk): sum_i w_i agg_i mod 17, bit 8 set
// when any polynomial of the group has a byte >= 17 in the chunk.
template <int NB>
__global__ __launch_bounds__(kzgo::T) void kzg_fold_agg_kernel(FoldBatch B, uint32_t* __restrict__ work) {
  __shared__ uint32_t psum[PLK_KZG_FOLD_MAX][kzgo::WAVES];   // per wave: the sum mod 17, bit 8 the flag
  const FoldGroup& G = B.g[blockIdx.y];
  const uint32_t c = blockIdx.x + 1;
  if (c >= G.nchunk) return;
  uint32_t pk[4];
  packed_powers(G.z, pk);
  const uint32_t lane = threadIdx.x & (PLK_WAVE - 1), wv = threadIdx.x / PLK_WAVE;
  const uint64_t base = (uint64_t)c * kzgo::CHUNK + (uint64_t)threadIdx.x * kzgo::E;
  for (uint32_t i0 = 0; i0 < G.k; i0 += NB) {   // (uniform)
    uint32_t w[NB][4];
    fold_load<NB>(B, G, i0, base, w);
#pragma unroll
    for (int u = 0; u < NB; u++) {
      if (i0 + u < G.k) {   // (uniform)
        const uint32_t s = plk_wave_sum(dot16(w[u], pk));   // (<= 64 x 16 x 255 x 16)
        const uint32_t anybad = __ballot(any_noncanonical(w[u])) != 0 ? 1u : 0u;
        if (lane == 0) psum[i0 + u][wv] = s % HFP | anybad << 8;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  uint32_t fold = 0, badall = 0;
  for (uint32_t i = 0; i < G.k; i++) {
    const FoldPoly& P = B.p[G.first + i];
    if (c >= P.nchunk) continue;   // (nothing of this polynomial in the chunk: its sums are zero)
    uint32_t t = 0;
#pragma unroll
    for (int v = 0; v < kzgo::WAVES; v++) t += psum[i][v];
    const uint32_t s = (t & 0xFFu) % HFP, anybad = (t >> 8) != 0 ? 1u : 0u;   // (sums < 4 x 17, flags above bit 8)
    work[P.work + c] = s | anybad << 8;
    fold += fold_weight(G, i) * s;   // (<= 16 x 16 x 16 in all)
    badall |= anybad;
  }
  work[G.work + c] = fold % HFP | badall << 8;
}

// Block (chunk, group) of a folded opening: kzg_open_kernel on F's bytes, which are formed in
// registers.  The group's polynomials are taken NB at a time (NB = 4, 8 or 16: the smallest that holds
// the launch's largest group, so a group's loads are all in flight together): their 16-byte loads
// issued together, the bytes of each coefficient position transposed into words of four polynomials
// and dotted with the four packed weights (v_dot4_u32_u8 on genuine bytes).  The chunk-0 block also
// writes every y_i: the polynomial's own chunk-0 sum plus its aggregate words (z^4096 = 1).
template <int NB>
__global__ __launch_bounds__(kzgo::T) void kzg_fold_open_kernel(FoldBatch B, const uint8_t* __restrict__ logs,
                                                             const uint32_t* __restrict__ work, uint8_t* __restrict__ ys,
                                                             PlkMsmResult* res, const uint32_t* __restrict__ exp_words,
                                                             uint32_t srs_bad, uint32_t row0) {
  __shared__ kzgo::Finish fin;
  __shared__ uint32_t ws[2 * kzgo::WAVES];
  __shared__ uint32_t ysum[PLK_KZG_FOLD_MAX][kzgo::WAVES];
  const FoldGroup& G = B.g[blockIdx.y];
  const uint32_t c = blockIdx.x;
  if (c >= G.nchunk) return;
  fin.stage(exp_words);
  const uint64_t ql = G.len - 1;
  const uint32_t z = G.z;
  uint32_t pk[4];
  packed_powers(z, pk);
  const uint64_t base = (uint64_t)c * kzgo::CHUNK + (uint64_t)threadIdx.x * kzgo::E;
  const int wv = (int)(threadIdx.x / PLK_WAVE);
  const uint32_t lane = threadIdx.x & (PLK_WAVE - 1);
  bool bad = srs_bad != 0;
  uint32_t acc[kzgo::E];   // sum_i w_i x byte of coefficient base + j, exact
#pragma unroll
  for (int j = 0; j < kzgo::E; j++) acc[j] = 0;
  for (uint32_t i0 = 0; i0 < G.k; i0 += NB) {   // (uniform; i0 + NB <= 16)
    uint32_t w[NB][4];
    fold_load<NB>(B, G, i0, base, w);
#pragma unroll
    for (int u = 0; u < NB; u++) bad |= i0 + u < G.k && any_noncanonical(w[u]);
#pragma unroll
    for (int q = 0; q < NB; q += 4) {
      const uint32_t wp = G.wpk[(i0 + q) >> 2];
#pragma unroll
      for (int m = 0; m < 4; m++) {
#pragma unroll
        for (int j = 0; j < 4; j++)
          acc[4 * m + j] = __builtin_amdgcn_udot4(kzgo::transpose4(w[q][m], w[q + 1][m], w[q + 2][m], w[q + 3][m], j), wp,
                                                  acc[4 * m + j], false);
      }
    }
    if (c == 0) {   // (uniform) y_i: this thread's share of p_i(z)
#pragma unroll
      for (int u = 0; u < NB; u++) {
        if (i0 + u < G.k) {
          const FoldPoly& P = B.p[G.first + i0 + u];
          uint32_t v = dot16(w[u], pk);   // (<= 16 x 255 x 16)
          if (z == 0) {
            v = threadIdx.x == 0 ? w[u][0] & 0xFFu : 0u;   // z^16 = 1 needs z != 0: p(0) = p[0]
          } else {
            for (uint32_t b = 1 + threadIdx.x; b < P.nchunk; b += kzgo::T) v += work[P.work + b] & 0xFFu;
          }
          const uint32_t s = plk_wave_sum(v);
          if (lane == 0) ysum[i0 + u][wv] = s;
        }
      }
    }
  }
  // F's sixteen canonical bytes
  uint32_t nb[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < kzgo::E; j++) nb[j >> 2] |= mod17(acc[j]) << (8 * (j & 3));   // (acc <= 65280)
  const uint4 lg = kzgo::Finish::logs(logs, srs_bad, base, ql);
  // z = 0: the thread's last quotient byte is F[base + 16], folded here from the polynomials' bytes (the
  // next thread's, or the next chunk's, first coefficient)
  uint32_t o[4];
  open_quotient(nb, pk, z, base, ql, G.q, (G.vec & 2u) != 0, work + G.work, c, G.nchunk, ws, bad, o, [&]() -> uint32_t {
    uint32_t sn = 0;
    for (uint32_t i = 0; i < G.k; i++) {
      const FoldPoly& P = B.p[G.first + i];
      if (base + 16 < P.len) sn += fold_weight(G, i) * P.p[base + 16];
    }
    return mod17(sn);   // (<= 65280)
  });
  // (ysum is complete: open_quotient held a barrier)
  if (c == 0 && threadIdx.x < G.k)
    ys[G.first + threadIdx.x] =
        (uint8_t)((ysum[threadIdx.x][0] % HFP + ysum[threadIdx.x][1] % HFP + ysum[threadIdx.x][2] % HFP + ysum[threadIdx.x][3] % HFP) % HFP);
  fin.finish(lg, o, bad, res + blockIdx.y, c, G.nchunk, row0 + blockIdx.y);
}

// argument checks shared by the four batch entry points (no device is touched)
int check_batch(const char* fn, const plk_srs* s, const void* polys, const size_t* lens, const uint8_t* zs, bool open,
                int n) {
  if (!s || !polys || !lens || n <= 0 || (open && !zs)) {
    plk_set_error("%s: handle, arrays and n > 0 are required", fn);
    return PLK_ERR_ARG;
  }
  for (int b = 0; b < n; b++) {
    if (lens[b] == 0) {
      plk_set_error("%s: job %d is an empty polynomial", fn, b);
      return PLK_ERR_ARG;
    }
    if (open && zs[b] >= HFP) {
      plk_set_error("%s: job %d: z = %u is not a GF(17) value", fn, b, (unsigned)zs[b]);
      return PLK_ERR_ARG;
    }
  }
  for (int b = 0; b < n; b++) {
    int rc = plk_kzg_check_record_len(fn, "job", b, lens[b]);
    if (rc || (rc = plk_kzg_check_srs_len(s, open ? std::max<size_t>(lens[b] - 1, 1) : lens[b]))) return rc;
  }
  return plk_kzg_check_device(fn, s);
}

// the launches of one batch: groups of up to KZG_JOBS jobs, consecutive on the stream
int launch_batch(const plk_srs* s, const uint8_t* const* d_polys, const size_t* lens, const uint8_t* zs, int n,
                 uint8_t* d_ys, PlkMsmResult* d_res, uint8_t* const* d_quots, uint32_t* d_work, hipStream_t st) {
  const bool open = zs != nullptr;
  uint64_t word = 0;
  for (int g0 = 0; g0 < n; g0 += KZG_JOBS) {
    const int nj = std::min(KZG_JOBS, n - g0);
    KzgBatch B;
    memset(&B, 0, sizeof B);
    uint32_t maxc = 1;
    for (int i = 0; i < nj; i++) {
      KzgJob& J = B.j[i];
      const int b = g0 + i;
      if (!d_polys[b]) {
        plk_set_error("plk_kzg: job %d has a NULL polynomial", b);
        return PLK_ERR_ARG;
      }
      J.p = d_polys[b];
      J.q = open && d_quots ? d_quots[b] : nullptr;
      J.len = lens[b];
      J.nchunk = (uint32_t)plk_kzg_chunks_of(lens[b]);
      J.work = (uint32_t)word;
      J.z = open ? zs[b] : 0;
      J.vec = ((uintptr_t)J.p % 16 == 0 ? 1u : 0u) | (J.q && (uintptr_t)J.q % 16 == 0 ? 2u : 0u);
      word += J.nchunk;
      maxc = std::max(maxc, J.nchunk);
    }
    const uint32_t bad = s->irregular ? 1u : 0u;
    if (open) {
      if (maxc > 1) {
        if (!d_work) {
          plk_set_error("plk_kzg_open_batch_dev: d_work is required for polynomials of more than %d coefficients",
                        kzgo::CHUNK);
          return PLK_ERR_ARG;
        }
        hipLaunchKernelGGL(kzg_agg_kernel, dim3((maxc - 1 + kzgo::WAVES - 1) / kzgo::WAVES, nj), dim3(kzgo::T), 0, st, B, d_work);
      }
      hipLaunchKernelGGL(kzg_open_kernel, dim3(maxc, nj), dim3(kzgo::T), 0, st, B, s->d_log, d_work, d_ys + g0, d_res + g0,
                         s->exp_words, bad, (uint32_t)g0);
    } else {
      hipLaunchKernelGGL(kzg_commit_kernel, dim3(maxc, nj), dim3(kzgo::T), 0, st, B, s->d_log, d_res + g0, s->exp_words, bad,
                         (uint32_t)g0);
    }
    PLK_HIP(hipGetLastError());
  }
  return PLK_OK;
}

// out3 = the reference's fold of sc[0, n) over the first n points of the G1 form (what plk_msm_g1
// computes): the dlog launch, then the raw serial fold when its record says irregular.
// d_sc: n scalars on the device; d_res: a zeroed record.
int msm_g1_form(const plk_srs* s, const uint8_t* d_sc, size_t n, PlkMsmResult* d_res, uint8_t out3[3]) {
  int rc = plk_msm_batch_launch(s->d_g1, 0, d_sc, 0, n, 1, d_res, s->st);
  if (rc) return rc;
  PlkMsmResult h;
  PLK_HIP(hipMemcpyAsync(&h, d_res, 32, hipMemcpyDeviceToHost, s->st));
  PLK_HIP(hipStreamSynchronize(s->st));
  if (h.irregular) {
    if ((rc = plk_msm_serial_launch(s->d_g1, d_sc, n, d_res, s->st))) return rc;
    PLK_HIP(hipMemcpyAsync(&h, d_res, 32, hipMemcpyDeviceToHost, s->st));
    PLK_HIP(hipStreamSynchronize(s->st));
  }
  memcpy(out3, h.g1, 3);
  return PLK_OK;
}

// the host-buffer forms: polynomials uploaded into one scratch arena, one batched call, and for
// every job its record flagged (a coefficient byte >= 17, or an SRS without log form) the
// composition of the public entry points with the commitment over the G1 form
int host_batch(const plk_srs* s, const uint8_t* const* polys, const size_t* lens, const uint8_t* zs, int n, uint8_t* ys,
               uint8_t* out3) {
  const bool open = zs != nullptr;
  size_t maxlen, poly_bytes;
  const int null_at = plk_kzg_arena_bytes(polys, lens, n, &poly_bytes, &maxlen);
  if (null_at >= 0) {
    plk_set_error("plk_kzg: job %d has a NULL polynomial", null_at);
    return PLK_ERR_ARG;
  }
  const size_t o_res = plk_pad16(poly_bytes), o_ys = o_res + (size_t)n * sizeof(PlkMsmResult), o_work = plk_pad16(o_ys + n),
               o_q = o_work + plk_kzg_workspace(lens, n), total = o_q + plk_pad16(maxlen) + 16;
  PlkScratch S;
  int rc = S.alloc("plk_kzg", total);
  if (rc) return rc;
  PlkMsmResult* d_res = (PlkMsmResult*)(S.d + o_res);
  PLK_HIP(hipMemsetAsync(d_res, 0, (size_t)n * sizeof(PlkMsmResult), s->st));
  std::vector<uint32_t> irr(n, 1u);
  if (!s->irregular) {
    std::vector<const uint8_t*> dp;
    if ((rc = plk_kzg_upload(S, polys, lens, n, s->st, dp)) ||
        (rc = launch_batch(s, dp.data(), lens, zs, n, S.d + o_ys, d_res, nullptr, (uint32_t*)(S.d + o_work), s->st)))
      return rc;
    if (open) PLK_HIP(hipMemcpyAsync(ys, S.d + o_ys, n, hipMemcpyDeviceToHost, s->st));
    if ((rc = plk_kzg_read_records(d_res, n, s->st, irr.data(), out3))) return rc;
  }
  std::vector<uint8_t> q, rem(1);
  uint8_t* d_q = S.d + o_q;
  for (int b = 0; b < n; b++) {
    if (!irr[b]) continue;
    // (the record may hold a set flag from the batched launch: start from a zeroed one)
    PLK_HIP(hipMemsetAsync(d_res + b, 0, sizeof(PlkMsmResult), s->st));
    const uint8_t* sc = polys[b];
    size_t sl = lens[b];
    if (open) {
      const uint8_t den[2] = {(uint8_t)((HFP - zs[b]) % HFP), 1};
      size_t qlen = 0, rl = 0;
      q.resize(std::max<size_t>(lens[b], 1));
      if ((rc = plk_poly_eval(polys[b], lens[b], zs[b], ys + b)) ||
          (rc = plk_poly_divide(polys[b], lens[b], den, 2, q.data(), &qlen, rem.data(), &rl)))
        return rc;
      sc = q.data();
      sl = qlen;
    }
    PLK_HIP(hipMemcpyAsync(d_q, sc, sl, hipMemcpyHostToDevice, s->st));
    if ((rc = msm_g1_form(s, d_q, sl, d_res + b, out3 + 3 * b))) return rc;
  }
  return PLK_OK;
}

// L of group g: the longest length
uint64_t fold_len(const size_t* lens, const int* start, int g) {
  size_t L = 0;
  for (int i = start[g]; i < start[g + 1]; i++) L = std::max(L, lens[i]);
  return L;
}

// argument checks of the folded opening (no device is touched; the handle is read last, by the
// range checks)
int check_fold(const char* fn, const plk_srs* s, const void* polys, const size_t* lens, const uint8_t* weights,
               const int* start, const uint8_t* zs, int ngroups, bool null_out) {
  if (!s || !polys || !lens || !weights || !start || !zs || ngroups <= 0 || null_out) {
    plk_set_error("%s: handle, arrays, outputs and ngroups > 0 are required", fn);
    return PLK_ERR_ARG;
  }
  if (!plk_kzg_layout_ok(start, ngroups, PLK_KZG_FOLD_MAX)) {
    plk_set_error("%s: start must rise strictly from 0 by at most %d polynomials a group", fn, PLK_KZG_FOLD_MAX);
    return PLK_ERR_ARG;
  }
  for (int g = 0; g < ngroups; g++) {
    if (zs[g] >= HFP) {
      plk_set_error("%s: group %d: z = %u is not a GF(17) value", fn, g, (unsigned)zs[g]);
      return PLK_ERR_ARG;
    }
    for (int i = start[g]; i < start[g + 1]; i++) {
      if (lens[i] == 0) {
        plk_set_error("%s: polynomial %d is empty", fn, i);
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
  for (int g = 0; g < ngroups; g++)
    if ((rc = plk_kzg_check_srs_len(s, std::max<size_t>(fold_len(lens, start, g) - 1, 1)))) return rc;
  return plk_kzg_check_device(fn, s);
}

}  // namespace

// the launches of a folded call (plk_kzg_host.h: kzg_multi.hip calls it too): as many whole groups as
// FOLD_POLYS polynomials allow per launch
int plk_kzg_fold_launch(const plk_srs* s, const uint8_t* const* d_polys, const size_t* lens, const uint8_t* weights,
                        const int* start, const uint8_t* zs, int ngroups, uint8_t* d_ys, PlkMsmResult* d_res,
                        uint8_t* const* d_quots, uint32_t* d_work, hipStream_t st, uint32_t row0) {
  uint64_t word = 0;
  int g = 0;
  while (g < ngroups) {
    FoldBatch B;
    memset(&B, 0, sizeof B);
    const int g0 = g, p0 = start[g];
    int np = 0;
    uint32_t maxc = 1, maxk = 1;
    for (; g < ngroups && np + (start[g + 1] - start[g]) <= FOLD_POLYS; g++) {
      FoldGroup& G = B.g[g - g0];
      G.q = d_quots ? d_quots[g] : nullptr;
      G.len = fold_len(lens, start, g);
      G.first = (uint32_t)np;
      G.k = (uint32_t)(start[g + 1] - start[g]);
      G.nchunk = (uint32_t)plk_kzg_chunks_of(G.len);
      G.z = zs[g];
      G.vec = G.q && (uintptr_t)G.q % 16 == 0 ? 2u : 0u;
      for (int i = start[g]; i < start[g + 1]; i++, np++) {
        if (!d_polys[i]) {
          plk_set_error("plk_kzg_open_fold: polynomial %d is NULL", i);
          return PLK_ERR_ARG;
        }
        FoldPoly& P = B.p[np];
        P.p = d_polys[i];
        P.len = lens[i];
        P.nchunk = (uint32_t)plk_kzg_chunks_of(lens[i]);
        P.work = (uint32_t)word;
        word += P.nchunk;
        G.wpk[(i - start[g]) >> 2] |= (uint32_t)weights[i] << (8 * ((i - start[g]) & 3));
      }
      G.work = (uint32_t)word;
      word += G.nchunk;
      maxc = std::max(maxc, G.nchunk);
      maxk = std::max(maxk, G.k);
    }
    const int ng = g - g0;
    if (maxc > 1) {
      if (!d_work) {
        plk_set_error("plk_kzg_open_fold_batch_dev: d_work is required for polynomials of more than %d coefficients",
                      kzgo::CHUNK);
        return PLK_ERR_ARG;
      }
      const auto agg = maxk <= 4 ? kzg_fold_agg_kernel<4> : maxk <= 8 ? kzg_fold_agg_kernel<8> : kzg_fold_agg_kernel<16>;
      hipLaunchKernelGGL(agg, dim3(maxc - 1, ng), dim3(kzgo::T), 0, st, B, d_work);
    }
    const auto open = maxk <= 4 ? kzg_fold_open_kernel<4> : maxk <= 8 ? kzg_fold_open_kernel<8> : kzg_fold_open_kernel<16>;
    hipLaunchKernelGGL(open, dim3(maxc, ng), dim3(kzgo::T), 0, st, B, s->d_log, d_work, d_ys + p0, d_res + g0, s->exp_words,
                       s->irregular ? 1u : 0u, row0 + (uint32_t)g0);
    PLK_HIP(hipGetLastError());
  }
  return PLK_OK;
}

namespace {

// the host-buffer form: one folded call over uploaded polynomials; a group whose record comes back
// flagged (a coefficient byte >= 17), and every group of an irregular SRS, takes the composition:
// y_i through plk_poly_eval, the quotient bytes of a one-group fused launch (exact for any input),
// trimmed, and their commitment over the resident G1 form
int host_fold(const plk_srs* s, const uint8_t* const* polys, const size_t* lens, const uint8_t* weights, const int* start,
              const uint8_t* zs, int ngroups, uint8_t* ys, uint8_t* out3) {
  const int np = start[ngroups];
  size_t maxlen, poly_bytes;
  const int null_at = plk_kzg_arena_bytes(polys, lens, np, &poly_bytes, &maxlen);
  if (null_at >= 0) {
    plk_set_error("plk_kzg_open_fold_batch: polynomial %d is NULL", null_at);
    return PLK_ERR_ARG;
  }
  // records: one per group and a spare for the one-group launches; ys: np and 16 spare
  const size_t o_res = plk_pad16(poly_bytes), o_ys = o_res + (size_t)(ngroups + 1) * sizeof(PlkMsmResult),
               o_work = plk_pad16(o_ys + np + PLK_KZG_FOLD_MAX), o_q = o_work + plk_kzg_fold_workspace(lens, start, ngroups),
               total = o_q + plk_pad16(maxlen) + 16;
  PlkScratch S;
  int rc = S.alloc("plk_kzg", total);
  if (rc) return rc;
  PlkMsmResult* d_res = (PlkMsmResult*)(S.d + o_res);
  uint32_t* d_work = (uint32_t*)(S.d + o_work);
  PLK_HIP(hipMemsetAsync(d_res, 0, (size_t)(ngroups + 1) * sizeof(PlkMsmResult), s->st));
  std::vector<const uint8_t*> dp;
  if ((rc = plk_kzg_upload(S, polys, lens, np, s->st, dp))) return rc;
  std::vector<uint32_t> irr(ngroups, 1u);
  if (!s->irregular) {
    if ((rc = plk_kzg_fold_launch(s, dp.data(), lens, weights, start, zs, ngroups, S.d + o_ys, d_res, nullptr, d_work, s->st,
                                  0)))
      return rc;
    PLK_HIP(hipMemcpyAsync(ys, S.d + o_ys, np, hipMemcpyDeviceToHost, s->st));
    if ((rc = plk_kzg_read_records(d_res, ngroups, s->st, irr.data(), out3))) return rc;
  }
  std::vector<uint8_t> q;
  uint8_t* d_q = S.d + o_q;
  PlkMsmResult* d_tmp = d_res + ngroups;
  for (int g = 0; g < ngroups; g++) {
    if (!irr[g]) continue;
    const int a = start[g], k = start[g + 1] - a;
    const int one[2] = {0, k};
    const size_t ql = std::max<size_t>(fold_len(lens, start, g) - 1, 1);
    uint8_t* const dq[1] = {d_q};
    PLK_HIP(hipMemsetAsync(d_tmp, 0, sizeof(PlkMsmResult), s->st));
    if ((rc = plk_kzg_fold_launch(s, dp.data() + a, lens + a, weights + a, one, zs + g, 1, S.d + o_ys + np, d_tmp, dq, d_work,
                                  s->st, (uint32_t)g)))
      return rc;
    q.resize(ql);
    PLK_HIP(hipMemcpyAsync(q.data(), d_q, ql, hipMemcpyDeviceToHost, s->st));
    PLK_HIP(hipStreamSynchronize(s->st));
    for (int i = a; i < a + k; i++)
      if ((rc = plk_poly_eval(polys[i], lens[i], zs[g], ys + i))) return rc;
    size_t sl = ql;
    while (sl > 1 && q[sl - 1] == 0) sl--;   // (the quotient as plk_poly_divide returns it)
    PLK_HIP(hipMemsetAsync(d_res + g, 0, sizeof(PlkMsmResult), s->st));
    if ((rc = msm_g1_form(s, d_q, sl, d_res + g, out3 + 3 * g))) return rc;
  }
  return PLK_OK;
}

}  // namespace

extern "C" {

int plk_srs_create(const uint8_t* g1s, size_t len, plk_srs_t** out) {
  if (!g1s || !len || !out) {
    plk_set_error("plk_srs_create: points, a length and out are required");
    return PLK_ERR_ARG;
  }
  int rc = plk_ctx_retain();
  if (rc) return rc;
  plk_srs* s = new plk_srs();
  s->dev = plk_cur_device();
  s->len = len;
  s->exp_words = plk_msm_exp_words_dev();
  const size_t lb = plk_pad16(len) + 16;
  rc = s->exp_words ? PLK_OK : PLK_ERR_HIP;
  if (!rc && (hipMalloc((void**)&s->d_g1, 3 * len + 16) != hipSuccess || hipMalloc((void**)&s->d_log, lb) != hipSuccess ||
              hipMalloc((void**)&s->d_flag, 16) != hipSuccess)) {
    plk_set_error("plk_srs_create: hipMalloc failed for %zu points", len);
    rc = PLK_ERR_NOMEM;
  }
  uint32_t flag = 0;
  if (!rc && (hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking) != hipSuccess ||
              hipMemsetAsync(s->d_log, 0, lb, s->st) != hipSuccess || hipMemsetAsync(s->d_flag, 0, 16, s->st) != hipSuccess ||
              hipMemcpyAsync(s->d_g1, g1s, 3 * len, hipMemcpyHostToDevice, s->st) != hipSuccess)) {
    plk_set_error("plk_srs_create: upload failed");
    rc = PLK_ERR_HIP;
  }
  if (!rc) rc = plk_srs_log_launch(s->d_g1, len, s->d_log, s->d_flag, s->st);
  if (!rc && (hipMemcpyAsync(&flag, s->d_flag, 4, hipMemcpyDeviceToHost, s->st) != hipSuccess ||
              hipStreamSynchronize(s->st) != hipSuccess)) {
    plk_set_error("plk_srs_create: the log conversion failed");
    rc = PLK_ERR_HIP;
  }
  if (rc) {
    plk_srs_destroy(s);
    return rc;
  }
  s->irregular = flag != 0;
  *out = s;
  return PLK_OK;
}

void plk_srs_destroy(plk_srs_t* s) {
  if (!s) return;
  const int prev = plk_cur_device();
  (void)hipSetDevice(s->dev);
  if (s->st) {
    (void)hipStreamSynchronize(s->st);
    (void)hipStreamDestroy(s->st);
  }
  (void)hipFree(s->d_g1);
  (void)hipFree(s->d_log);
  (void)hipFree(s->d_flag);
  (void)hipSetDevice(prev);
  delete s;
  plk_ctx_release();
}

size_t plk_srs_len(const plk_srs_t* s) { return s ? s->len : 0; }
int plk_srs_irregular(const plk_srs_t* s) { return s && s->irregular ? 1 : 0; }

size_t plk_kzg_workspace(const size_t* lens, int n) {
  if (!lens || n <= 0) return 0;
  uint64_t words = 0;
  for (int b = 0; b < n; b++) words += plk_kzg_chunks_of(lens[b]);
  return (size_t)((4 * words + 255) & ~255ull);
}

int plk_kzg_commit_batch_dev(const plk_srs_t* s, const uint8_t* const* d_polys, const size_t* lens, int n,
                             plk_msm_result_t* d_res, void* stream) {
  int rc = check_batch("plk_kzg_commit_batch_dev", s, d_polys, lens, nullptr, false, n);
  if (rc) return rc;
  if (!d_res) {
    plk_set_error("plk_kzg_commit_batch_dev: NULL d_res");
    return PLK_ERR_ARG;
  }
  return launch_batch(s, d_polys, lens, nullptr, n, nullptr, d_res, nullptr, nullptr, (hipStream_t)stream);
}

int plk_kzg_open_batch_dev(const plk_srs_t* s, const uint8_t* const* d_polys, const size_t* lens, const uint8_t* zs, int n,
                           uint8_t* d_ys, plk_msm_result_t* d_res, uint8_t* const* d_quots, void* d_work, void* stream) {
  int rc = check_batch("plk_kzg_open_batch_dev", s, d_polys, lens, zs, true, n);
  if (rc) return rc;
  if (!d_ys || !d_res) {
    plk_set_error("plk_kzg_open_batch_dev: NULL d_ys or d_res");
    return PLK_ERR_ARG;
  }
  return launch_batch(s, d_polys, lens, zs, n, d_ys, d_res, d_quots, (uint32_t*)d_work, (hipStream_t)stream);
}

int plk_kzg_commit_batch(const plk_srs_t* s, const uint8_t* const* polys, const size_t* lens, int n, uint8_t* out3) {
  int rc = check_batch("plk_kzg_commit_batch", s, polys, lens, nullptr, false, n);
  if (rc) return rc;
  if (!out3) {
    plk_set_error("plk_kzg_commit_batch: NULL out3");
    return PLK_ERR_ARG;
  }
  return host_batch(s, polys, lens, nullptr, n, nullptr, out3);
}

int plk_kzg_open_batch(const plk_srs_t* s, const uint8_t* const* polys, const size_t* lens, const uint8_t* zs, int n,
                       uint8_t* ys, uint8_t* proofs3) {
  int rc = check_batch("plk_kzg_open_batch", s, polys, lens, zs, true, n);
  if (rc) return rc;
  if (!ys || !proofs3) {
    plk_set_error("plk_kzg_open_batch: NULL ys or proofs3");
    return PLK_ERR_ARG;
  }
  return host_batch(s, polys, lens, zs, n, ys, proofs3);
}

size_t plk_kzg_fold_workspace(const size_t* lens, const int* start, int ngroups) {
  if (!lens || !plk_kzg_layout_ok(start, ngroups, PLK_KZG_FOLD_MAX)) return 0;
  uint64_t words = 0;
  for (int g = 0; g < ngroups; g++) {
    for (int i = start[g]; i < start[g + 1]; i++) words += plk_kzg_chunks_of(lens[i]);
    words += plk_kzg_chunks_of(fold_len(lens, start, g));
  }
  return (size_t)((4 * words + 255) & ~255ull);
}

int plk_kzg_open_fold_batch_dev(const plk_srs_t* s, const uint8_t* const* d_polys, const size_t* lens, const uint8_t* weights,
                                const int* start, const uint8_t* zs, int ngroups, uint8_t* d_ys, plk_msm_result_t* d_res,
                                uint8_t* const* d_quots, void* d_work, void* stream) {
  int rc = check_fold("plk_kzg_open_fold_batch_dev", s, d_polys, lens, weights, start, zs, ngroups, !d_ys || !d_res);
  if (rc) return rc;
  return plk_kzg_fold_launch(s, d_polys, lens, weights, start, zs, ngroups, d_ys, d_res, d_quots, (uint32_t*)d_work,
                             (hipStream_t)stream, 0);
}

int plk_kzg_open_fold_batch(const plk_srs_t* s, const uint8_t* const* polys, const size_t* lens, const uint8_t* weights,
                            const int* start, const uint8_t* zs, int ngroups, uint8_t* ys, uint8_t* proofs3) {
  int rc = check_fold("plk_kzg_open_fold_batch", s, polys, lens, weights, start, zs, ngroups, !ys || !proofs3);
  if (rc) return rc;
  return host_fold(s, polys, lens, weights, start, zs, ngroups, ys, proofs3);
}

}  // extern "C"
