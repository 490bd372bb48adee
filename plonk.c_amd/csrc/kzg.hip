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
#include <string.h>

#include <algorithm>
#include <vector>

#include "kzg_multi.h"
#include "plk_device.h"
#include "plk_hf17.h"
#include "plk_hostcall.h"
#include "plk_internal.h"
#include "plk_msm_finish.h"

namespace {

constexpr int KZG_T = 256, KZG_E = 16, KZG_CHUNK = KZG_T * KZG_E;
constexpr int KZG_JOBS = 32;          // jobs per launch
constexpr uint32_t HFP = hf17::P;
using hf17::any_noncanonical;
using hf17::byte_of;
using hf17::load16;
using hf17::mod17;
using hf17::wave_suffix;
constexpr uint64_t KZG_MAX_LEN = (8ull * 65535ull) * KZG_CHUNK;   // the finish's ticket field: blocks per record
static_assert(KZG_MAX_LEN == PLK_KZG_RECORD_MAX_LEN, "kzg_multi.h states the same bound");

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

// sum_k byte k of w x z^k over the 16 bytes (<= 16 x 255 x 16): the powers packed four to a word
// (uniform), four v_dot4_u32_u8 on genuine bytes
__device__ __forceinline__ uint32_t dot_powers(const uint32_t (&w)[4], const uint32_t (&pw)[16]) {
  uint32_t t = 0;
#pragma unroll
  for (int i = 0; i < 4; i++)
    t = __builtin_amdgcn_udot4(w[i], pw[4 * i] | pw[4 * i + 1] << 8 | pw[4 * i + 2] << 16 | pw[4 * i + 3] << 24, t, false);
  return t;
}
// Aggregates of job blockIdx.y: one wave per chunk (four 16-byte groups per lane, no LDS, no
// barrier), chunk 0 skipped -- its aggregate is never read.  One word per chunk:
// [7:0] sum_i p[i] z^(i mod 16) mod 17 over the chunk, bit 8 set when a byte is >= 17.
constexpr int KZG_AGG_WAVES = KZG_T / PLK_WAVE;   // chunks per block
__global__ __launch_bounds__(KZG_T) void kzg_agg_kernel(KzgBatch B, uint32_t* __restrict__ work) {
  const KzgJob& J = B.j[blockIdx.y];
  const uint32_t c = blockIdx.x * KZG_AGG_WAVES + threadIdx.x / PLK_WAVE + 1;
  if (c >= J.nchunk) return;   // (the whole wave)
  uint32_t pw[16];
  pw[0] = 1;
#pragma unroll
  for (int k = 1; k < 16; k++) pw[k] = pw[k - 1] * J.z % HFP;
  const uint32_t lane = threadIdx.x & (PLK_WAVE - 1);
  constexpr int G = KZG_CHUNK / (PLK_WAVE * KZG_E);   // groups per lane
  uint32_t w[G][4];
#pragma unroll
  for (int i = 0; i < G; i++)
    load16(J.p, J.len, (uint64_t)c * KZG_CHUNK + (uint64_t)(i * PLK_WAVE + lane) * KZG_E, J.vec & 1u, w[i]);
  uint32_t acc = 0;
  bool bad = false;
#pragma unroll
  for (int i = 0; i < G; i++) {
    acc += dot_powers(w[i], pw);   // (<= 4 x 16 x 255 x 16)
    bad |= any_noncanonical(w[i]);
  }
  const uint32_t s = plk_wave_sum(acc % HFP);
  const uint64_t anybad = __ballot(bad);
  if (lane == 0) work[J.work + c] = s % HFP | (anybad != 0 ? 1u : 0u) << 8;
}

// Block (chunk, job) of an opening: see the head of this file.  srs_bad: the SRS has no log form
// (every record is then flagged; y and the quotient bytes are still exact).
__global__ __launch_bounds__(KZG_T) void kzg_open_kernel(KzgBatch B, const uint8_t* __restrict__ logs,
                                                        const uint32_t* __restrict__ work, uint8_t* __restrict__ ys,
                                                        PlkMsmResult* res, const uint32_t* __restrict__ exp_words,
                                                        uint32_t srs_bad, uint32_t row0) {
  __shared__ uint32_t etab[PLK_GROUP_ORDER];
  __shared__ uint32_t wsum[KZG_T / PLK_WAVE];
  __shared__ uint32_t wbad[KZG_T / PLK_WAVE];
  __shared__ uint32_t ws[2][KZG_T / PLK_WAVE];
  const KzgJob& J = B.j[blockIdx.y];
  const uint32_t c = blockIdx.x;
  if (c >= J.nchunk) return;
  if (threadIdx.x < PLK_GROUP_ORDER) etab[threadIdx.x] = exp_words[threadIdx.x];
  const uint8_t* p = J.p;
  const uint64_t len = J.len, ql = len - 1;
  const uint32_t z = J.z;
  uint32_t pw[16];
  pw[0] = 1;
#pragma unroll
  for (int k = 1; k < 16; k++) pw[k] = pw[k - 1] * z % HFP;
  // the thread's 16 consecutive coefficients [base, base + 16), base = 0 mod 16
  const uint64_t base = (uint64_t)c * KZG_CHUNK + (uint64_t)threadIdx.x * KZG_E;
  uint32_t nb[4];
  load16(p, len, base, J.vec & 1u, nb);
  uint4 lg = make_uint4(0, 0, 0, 0);
  if (!srs_bad && base < ql) lg = *reinterpret_cast<const uint4*>(logs + base);   // (logs: zero padded to 16)
  bool bad = any_noncanonical(nb) || srs_bad;
  // the thread's aggregate sum_k p[base + k] z^k (base = 0 mod 16; coefficient 0 is not summed)
  uint32_t tot = dot_powers(nb, pw);
  if (base == 0) tot -= nb[0] & 0xFFu;   // (pw[0] = 1)
  tot = mod17(tot);                       // (<= 16 x 255 x 16)
  // carry: the aggregates of every later chunk (written by the previous launch)
  uint32_t cs = 0;
  for (uint32_t b = c + 1 + threadIdx.x; b < J.nchunk; b += KZG_T) {
    const uint32_t a = work[J.work + b];
    cs += a & 0xFFu;
    bad |= (a >> 8) != 0;
  }
  const uint32_t suf = wave_suffix(tot);        // this lane's coefficients and every later lane's
  const uint32_t cw = plk_wave_sum(cs % HFP);
  const int wv = (int)(threadIdx.x / PLK_WAVE);
  if ((threadIdx.x & (PLK_WAVE - 1)) == 0) {
    ws[0][wv] = suf;   // lane 0: the wave's total
    ws[1][wv] = cw;
  }
  __syncthreads();
  uint32_t run = suf - tot;   // the aggregates of the threads after this one, and the carry
#pragma unroll
  for (int u = 0; u < KZG_T / PLK_WAVE; u++) run += (u > wv ? ws[0][u] : 0u) + ws[1][u];
  // The quotient bytes, no bounds test: past the polynomial the loaded bytes are zero and the last
  // chunk has no carry, so q[j] comes out zero for j >= len - 1.
  uint32_t o[4] = {0, 0, 0, 0};
  if (z != 0) {
    // run = sum_{i >= base + 16} p[i] z^i and z^-(base + 16) = 1: the thread's top quotient byte is
    // run itself, the others follow the division's own recurrence q[j] = p[j + 1] + z q[j + 1]
    uint32_t qv = run % HFP;
    o[3] = qv << 24;
#pragma unroll
    for (int k = KZG_E - 2; k >= 0; k--) {
      qv = mod17(byte_of(nb, k + 1) + z * qv);   // (<= 255 + 16 x 16)
      o[k >> 2] |= qv << (8 * (k & 3));
    }
  } else {
    // z = 0: q[j] = p[j + 1], the loaded bytes one place down; the thread's last quotient byte is the
    // next thread's first coefficient
    const uint32_t nxt = base + 16 < len ? p[base + 16] : 0u;
    o[0] = nb[0] >> 8 | nb[1] << 24;
    o[1] = nb[1] >> 8 | nb[2] << 24;
    o[2] = nb[2] >> 8 | nb[3] << 24;
    o[3] = nb[3] >> 8 | nxt << 24;
  }
  if (base == 0) ys[blockIdx.y] = (uint8_t)(((nb[0] & 0xFFu) + z * (o[0] & 0xFFu)) % HFP);   // y = p[0] + z q[0]
  if (J.q) {
    if ((J.vec & 2u) && base + 16 <= ql) {
      *reinterpret_cast<uint4*>(J.q + base) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 16; k++)
        if (base + k < ql) J.q[base + k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
    }
    if (base == 0 && ql == 0) J.q[0] = 0;   // len 1: the quotient is {0}
  }
  uint32_t t = __builtin_amdgcn_udot4(lg.x, o[0], 0u, false);   // 16 x 101 x 255 < 2^19
  t = __builtin_amdgcn_udot4(lg.y, o[1], t, false);
  t = __builtin_amdgcn_udot4(lg.z, o[2], t, false);
  t = __builtin_amdgcn_udot4(lg.w, o[3], t, false);
  (void)msm_finish_xy<KZG_T>(t % PLK_GROUP_ORDER, bad, res + blockIdx.y, wsum, wbad, etab, c, J.nchunk,
                             row0 + blockIdx.y);
}

// Block (x, job) of a ragged batch of commitments: job b = MSM over its len points of the log SRS,
// one 16-point group per thread, any scalar byte (g1_mul takes the raw byte).
__global__ __launch_bounds__(KZG_T) void kzg_commit_kernel(KzgBatch B, const uint8_t* __restrict__ logs,
                                                          PlkMsmResult* res, const uint32_t* __restrict__ exp_words,
                                                          uint32_t srs_bad, uint32_t row0) {
  __shared__ uint32_t etab[PLK_GROUP_ORDER];
  __shared__ uint32_t wsum[KZG_T / PLK_WAVE];
  __shared__ uint32_t wbad[KZG_T / PLK_WAVE];
  const KzgJob& J = B.j[blockIdx.y];
  const uint32_t c = blockIdx.x;
  if (c >= J.nchunk) return;
  if (threadIdx.x < PLK_GROUP_ORDER) etab[threadIdx.x] = exp_words[threadIdx.x];
  const uint64_t base = (uint64_t)c * KZG_CHUNK + (uint64_t)threadIdx.x * KZG_E;
  uint32_t sc[4];
  load16(J.p, J.len, base, J.vec & 1u, sc);
  uint4 lg = make_uint4(0, 0, 0, 0);
  if (!srs_bad && base < J.len) lg = *reinterpret_cast<const uint4*>(logs + base);   // (logs: zero padded to 16)
  uint32_t t = __builtin_amdgcn_udot4(lg.x, sc[0], 0u, false);   // 16 x 101 x 255 < 2^19
  t = __builtin_amdgcn_udot4(lg.y, sc[1], t, false);
  t = __builtin_amdgcn_udot4(lg.z, sc[2], t, false);
  t = __builtin_amdgcn_udot4(lg.w, sc[3], t, false);
  (void)msm_finish_xy<KZG_T>(t % PLK_GROUP_ORDER, srs_bad != 0, res + blockIdx.y, wsum, wbad, etab, c, J.nchunk,
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

__device__ __forceinline__ bool aligned16(const uint8_t* p) { return ((uintptr_t)p & 15u) == 0; }
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
    fast = fast && aligned16(P.p) && base + 16 <= P.len;
  }
  if (fast) {
#pragma unroll
    for (int u = 0; u < NB; u++) {
      const uint4 v = *reinterpret_cast<const uint4*>(B.p[G.first + min(i0 + u, G.k - 1)].p + base);
      w[u][0] = v.x; w[u][1] = v.y; w[u][2] = v.z; w[u][3] = v.w;
    }
  } else {
    // byte-wise, as a rolled loop that shifts each byte in from the top (no indexed registers), which
    // keeps this rare path's code a fraction of the unrolled load16's
#pragma unroll
    for (int u = 0; u < NB; u++) {
      const FoldPoly& P = B.p[G.first + min(i0 + u, G.k - 1)];
      uint32_t x0 = 0, x1 = 0, x2 = 0, x3 = 0;
#pragma nounroll
      for (int k = 0; k < 16; k++) {
        const uint32_t b = base + k < P.len ? P.p[base + k] : 0u;
        x0 = x0 >> 8 | x1 << 24;
        x1 = x1 >> 8 | x2 << 24;
        x2 = x2 >> 8 | x3 << 24;
        x3 = x3 >> 8 | b << 24;
      }
      w[u][0] = x0; w[u][1] = x1; w[u][2] = x2; w[u][3] = x3;
    }
  }
}

// Aggregates of group blockIdx.y: one block per chunk c >= 1 of L, a 16-coefficient run per thread as
// in the opening, the group's polynomials NB at a time.  One word per (polynomial, chunk) as
// kzg_agg_kernel writes it, and one folded word per (group, chunk): sum_i w_i agg_i mod 17, bit 8 set
// when any polynomial of the group has a byte >= 17 in the chunk.
template <int NB>
__global__ __launch_bounds__(KZG_T) void kzg_fold_agg_kernel(FoldBatch B, uint32_t* __restrict__ work) {
  __shared__ uint32_t psum[PLK_KZG_FOLD_MAX][KZG_T / PLK_WAVE];   // per wave: the sum mod 17, bit 8 the flag
  const FoldGroup& G = B.g[blockIdx.y];
  const uint32_t c = blockIdx.x + 1;
  if (c >= G.nchunk) return;
  uint32_t pw[16];
  pw[0] = 1;
#pragma unroll
  for (int k = 1; k < 16; k++) pw[k] = pw[k - 1] * G.z % HFP;
  const uint32_t lane = threadIdx.x & (PLK_WAVE - 1), wv = threadIdx.x / PLK_WAVE;
  const uint64_t base = (uint64_t)c * KZG_CHUNK + (uint64_t)threadIdx.x * KZG_E;
  for (uint32_t i0 = 0; i0 < G.k; i0 += NB) {   // (uniform)
    uint32_t w[NB][4];
    fold_load<NB>(B, G, i0, base, w);
#pragma unroll
    for (int u = 0; u < NB; u++) {
      if (i0 + u < G.k) {   // (uniform)
        const uint32_t s = plk_wave_sum(dot_powers(w[u], pw));   // (<= 64 x 16 x 255 x 16)
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
    for (int v = 0; v < KZG_T / PLK_WAVE; v++) t += psum[i][v];
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
__global__ __launch_bounds__(KZG_T) void kzg_fold_open_kernel(FoldBatch B, const uint8_t* __restrict__ logs,
                                                             const uint32_t* __restrict__ work, uint8_t* __restrict__ ys,
                                                             PlkMsmResult* res, const uint32_t* __restrict__ exp_words,
                                                             uint32_t srs_bad, uint32_t row0) {
  __shared__ uint32_t etab[PLK_GROUP_ORDER];
  __shared__ uint32_t wsum[KZG_T / PLK_WAVE];
  __shared__ uint32_t wbad[KZG_T / PLK_WAVE];
  __shared__ uint32_t ws[2][KZG_T / PLK_WAVE];
  __shared__ uint32_t ysum[PLK_KZG_FOLD_MAX][KZG_T / PLK_WAVE];
  const FoldGroup& G = B.g[blockIdx.y];
  const uint32_t c = blockIdx.x;
  if (c >= G.nchunk) return;
  if (threadIdx.x < PLK_GROUP_ORDER) etab[threadIdx.x] = exp_words[threadIdx.x];
  const uint64_t len = G.len, ql = len - 1;
  const uint32_t z = G.z;
  uint32_t pw[16];
  pw[0] = 1;
#pragma unroll
  for (int k = 1; k < 16; k++) pw[k] = pw[k - 1] * z % HFP;
  const uint64_t base = (uint64_t)c * KZG_CHUNK + (uint64_t)threadIdx.x * KZG_E;
  const int wv = (int)(threadIdx.x / PLK_WAVE);
  const uint32_t lane = threadIdx.x & (PLK_WAVE - 1);
  bool bad = srs_bad != 0;
  uint32_t acc[KZG_E];   // sum_i w_i x byte of coefficient base + j, exact
#pragma unroll
  for (int j = 0; j < KZG_E; j++) acc[j] = 0;
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
        for (int j = 0; j < 4; j++) {
          // byte j of word m of four polynomials, polynomial q + u in byte u
          const uint32_t t = ((w[q][m] >> (8 * j)) & 0xFFu) | ((w[q + 1][m] >> (8 * j)) & 0xFFu) << 8 |
                             ((w[q + 2][m] >> (8 * j)) & 0xFFu) << 16 | ((w[q + 3][m] >> (8 * j)) & 0xFFu) << 24;
          acc[4 * m + j] = __builtin_amdgcn_udot4(t, wp, acc[4 * m + j], false);
        }
      }
    }
    if (c == 0) {   // (uniform) y_i: this thread's share of p_i(z)
#pragma unroll
      for (int u = 0; u < NB; u++) {
        if (i0 + u < G.k) {
          const FoldPoly& P = B.p[G.first + i0 + u];
          uint32_t v = dot_powers(w[u], pw);   // (<= 16 x 255 x 16)
          if (z == 0) {
            v = threadIdx.x == 0 ? w[u][0] & 0xFFu : 0u;   // z^16 = 1 needs z != 0: p(0) = p[0]
          } else {
            for (uint32_t b = 1 + threadIdx.x; b < P.nchunk; b += KZG_T) v += work[P.work + b] & 0xFFu;
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
  for (int j = 0; j < KZG_E; j++) nb[j >> 2] |= mod17(acc[j]) << (8 * (j & 3));   // (acc <= 65280)
  uint4 lg = make_uint4(0, 0, 0, 0);
  if (!srs_bad && base < ql) lg = *reinterpret_cast<const uint4*>(logs + base);   // (logs: zero padded to 16)
  // from here on kzg_open_kernel, on F
  uint32_t tot = dot_powers(nb, pw);
  if (base == 0) tot -= nb[0] & 0xFFu;
  tot = mod17(tot);
  uint32_t cs = 0;
  for (uint32_t b = c + 1 + threadIdx.x; b < G.nchunk; b += KZG_T) {
    const uint32_t a = work[G.work + b];
    cs += a & 0xFFu;
    bad |= (a >> 8) != 0;
  }
  const uint32_t suf = wave_suffix(tot);
  const uint32_t cw = plk_wave_sum(cs % HFP);
  if (lane == 0) {
    ws[0][wv] = suf;
    ws[1][wv] = cw;
  }
  __syncthreads();
  if (c == 0 && threadIdx.x < G.k)
    ys[G.first + threadIdx.x] =
        (uint8_t)((ysum[threadIdx.x][0] % HFP + ysum[threadIdx.x][1] % HFP + ysum[threadIdx.x][2] % HFP + ysum[threadIdx.x][3] % HFP) % HFP);
  uint32_t run = suf - tot;
#pragma unroll
  for (int u = 0; u < KZG_T / PLK_WAVE; u++) run += (u > wv ? ws[0][u] : 0u) + ws[1][u];
  uint32_t o[4] = {0, 0, 0, 0};
  if (z != 0) {
    uint32_t qv = run % HFP;
    o[3] = qv << 24;
#pragma unroll
    for (int k = KZG_E - 2; k >= 0; k--) {
      qv = mod17(byte_of(nb, k + 1) + z * qv);
      o[k >> 2] |= qv << (8 * (k & 3));
    }
  } else {
    // z = 0: q[j] = F[j + 1]; the thread's last quotient byte is F[base + 16], folded here from the
    // polynomials' bytes (the next thread's, or the next chunk's, first coefficient)
    uint32_t sn = 0;
    for (uint32_t i = 0; i < G.k; i++) {
      const FoldPoly& P = B.p[G.first + i];
      if (base + 16 < P.len) sn += fold_weight(G, i) * P.p[base + 16];
    }
    const uint32_t nxt = mod17(sn);   // (<= 65280)
    o[0] = nb[0] >> 8 | nb[1] << 24;
    o[1] = nb[1] >> 8 | nb[2] << 24;
    o[2] = nb[2] >> 8 | nb[3] << 24;
    o[3] = nb[3] >> 8 | nxt << 24;
  }
  if (G.q) {
    if ((G.vec & 2u) && base + 16 <= ql) {
      *reinterpret_cast<uint4*>(G.q + base) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 16; k++)
        if (base + k < ql) G.q[base + k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
    }
    if (base == 0 && ql == 0) G.q[0] = 0;   // L = 1: the quotient is {0}
  }
  uint32_t t = __builtin_amdgcn_udot4(lg.x, o[0], 0u, false);   // 16 x 101 x 255 < 2^19
  t = __builtin_amdgcn_udot4(lg.y, o[1], t, false);
  t = __builtin_amdgcn_udot4(lg.z, o[2], t, false);
  t = __builtin_amdgcn_udot4(lg.w, o[3], t, false);
  (void)msm_finish_xy<KZG_T>(t % PLK_GROUP_ORDER, bad, res + blockIdx.y, wsum, wbad, etab, c, G.nchunk,
                             row0 + blockIdx.y);
}

uint64_t chunks_of(uint64_t len) { return (len + KZG_CHUNK - 1) / KZG_CHUNK; }

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
    const size_t need = open ? std::max<size_t>(lens[b] - 1, 1) : lens[b];
    if (lens[b] > KZG_MAX_LEN) {
      plk_set_error("%s: job %d: %zu coefficients exceed the %llu one record's finish can count", fn, b, lens[b],
                    (unsigned long long)KZG_MAX_LEN);
      return PLK_ERR_RANGE;
    }
    if (need > s->len) {
      plk_set_error("Poynomial degree exceeds SRS size: POLY degree: %zu, SRS supports up to degree: %zu", need,
                    s->len);
      return PLK_ERR_RANGE;
    }
  }
  if (plk_cur_device() != s->dev) {
    plk_set_error("%s: the SRS lives on device %d but the calling thread's current device is %d", fn, s->dev,
                  plk_cur_device());
    return PLK_ERR_ARG;
  }
  return PLK_OK;
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
      J.nchunk = (uint32_t)chunks_of(lens[b]);
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
                        KZG_CHUNK);
          return PLK_ERR_ARG;
        }
        hipLaunchKernelGGL(kzg_agg_kernel, dim3((maxc - 1 + KZG_AGG_WAVES - 1) / KZG_AGG_WAVES, nj), dim3(KZG_T), 0, st, B, d_work);
      }
      hipLaunchKernelGGL(kzg_open_kernel, dim3(maxc, nj), dim3(KZG_T), 0, st, B, s->d_log, d_work, d_ys + g0, d_res + g0,
                         s->exp_words, bad, (uint32_t)g0);
    } else {
      hipLaunchKernelGGL(kzg_commit_kernel, dim3(maxc, nj), dim3(KZG_T), 0, st, B, s->d_log, d_res + g0, s->exp_words, bad,
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
  size_t maxlen = 0, poly_bytes = 0;
  for (int b = 0; b < n; b++) {
    if (!polys[b]) {
      plk_set_error("plk_kzg: job %d has a NULL polynomial", b);
      return PLK_ERR_ARG;
    }
    maxlen = std::max(maxlen, lens[b]);
    poly_bytes += plk_pad16(lens[b]);
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
    std::vector<const uint8_t*> dp(n);
    size_t off = 0;
    for (int b = 0; b < n; b++) {
      dp[b] = S.d + off;
      PLK_HIP(hipMemcpyAsync(S.d + off, polys[b], lens[b], hipMemcpyHostToDevice, s->st));
      off += plk_pad16(lens[b]);
    }
    if ((rc = launch_batch(s, dp.data(), lens, zs, n, S.d + o_ys, d_res, nullptr, (uint32_t*)(S.d + o_work), s->st)))
      return rc;
    std::vector<uint8_t> h(32 * (size_t)n);
    PLK_HIP(hipMemcpy2DAsync(h.data(), 32, d_res, sizeof(PlkMsmResult), 32, n, hipMemcpyDeviceToHost, s->st));
    if (open) PLK_HIP(hipMemcpyAsync(ys, S.d + o_ys, n, hipMemcpyDeviceToHost, s->st));
    PLK_HIP(hipStreamSynchronize(s->st));
    for (int b = 0; b < n; b++) {
      const PlkMsmResult* r = (const PlkMsmResult*)(h.data() + 32 * (size_t)b);
      irr[b] = r->irregular;
      memcpy(out3 + 3 * b, r->g1, 3);
    }
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

// the group layout of a folded call: start[0] = 0, strictly increasing, at most PLK_KZG_FOLD_MAX a group
bool fold_layout_ok(const int* start, int ngroups) {
  if (!start || ngroups <= 0 || start[0] != 0) return false;
  for (int g = 0; g < ngroups; g++) {
    const long long k = (long long)start[g + 1] - start[g];
    if (k < 1 || k > PLK_KZG_FOLD_MAX) return false;
  }
  return true;
}
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
  if (!fold_layout_ok(start, ngroups)) {
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
  for (int i = 0; i < start[ngroups]; i++) {
    if (lens[i] > KZG_MAX_LEN) {
      plk_set_error("%s: polynomial %d: %zu coefficients exceed the %llu one record's finish can count", fn, i, lens[i],
                    (unsigned long long)KZG_MAX_LEN);
      return PLK_ERR_RANGE;
    }
  }
  for (int g = 0; g < ngroups; g++) {
    const size_t need = std::max<size_t>(fold_len(lens, start, g) - 1, 1);
    if (need > s->len) {
      plk_set_error("Poynomial degree exceeds SRS size: POLY degree: %zu, SRS supports up to degree: %zu", need,
                    s->len);
      return PLK_ERR_RANGE;
    }
  }
  if (plk_cur_device() != s->dev) {
    plk_set_error("%s: the SRS lives on device %d but the calling thread's current device is %d", fn, s->dev,
                  plk_cur_device());
    return PLK_ERR_ARG;
  }
  return PLK_OK;
}

// the launches of a folded call: as many whole groups as FOLD_POLYS polynomials allow per launch,
// consecutive on the stream; row0: the record index of group 0 (the finish's shard spread)
int launch_fold(const plk_srs* s, const uint8_t* const* d_polys, const size_t* lens, const uint8_t* weights,
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
      G.nchunk = (uint32_t)chunks_of(G.len);
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
        P.nchunk = (uint32_t)chunks_of(lens[i]);
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
                      KZG_CHUNK);
        return PLK_ERR_ARG;
      }
      const auto agg = maxk <= 4 ? kzg_fold_agg_kernel<4> : maxk <= 8 ? kzg_fold_agg_kernel<8> : kzg_fold_agg_kernel<16>;
      hipLaunchKernelGGL(agg, dim3(maxc - 1, ng), dim3(KZG_T), 0, st, B, d_work);
    }
    const auto open = maxk <= 4 ? kzg_fold_open_kernel<4> : maxk <= 8 ? kzg_fold_open_kernel<8> : kzg_fold_open_kernel<16>;
    hipLaunchKernelGGL(open, dim3(maxc, ng), dim3(KZG_T), 0, st, B, s->d_log, d_work, d_ys + p0, d_res + g0, s->exp_words,
                       s->irregular ? 1u : 0u, row0 + (uint32_t)g0);
    PLK_HIP(hipGetLastError());
  }
  return PLK_OK;
}

// the host-buffer form: one folded call over uploaded polynomials; a group whose record comes back
// flagged (a coefficient byte >= 17), and every group of an irregular SRS, takes the composition:
// y_i through plk_poly_eval, the quotient bytes of a one-group fused launch (exact for any input),
// trimmed, and their commitment over the resident G1 form
int host_fold(const plk_srs* s, const uint8_t* const* polys, const size_t* lens, const uint8_t* weights, const int* start,
              const uint8_t* zs, int ngroups, uint8_t* ys, uint8_t* out3) {
  const int np = start[ngroups];
  size_t maxlen = 0, poly_bytes = 0;
  for (int i = 0; i < np; i++) {
    if (!polys[i]) {
      plk_set_error("plk_kzg_open_fold_batch: polynomial %d is NULL", i);
      return PLK_ERR_ARG;
    }
    maxlen = std::max(maxlen, lens[i]);
    poly_bytes += plk_pad16(lens[i]);
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
  std::vector<const uint8_t*> dp(np);
  size_t off = 0;
  for (int i = 0; i < np; i++) {
    dp[i] = S.d + off;
    PLK_HIP(hipMemcpyAsync(S.d + off, polys[i], lens[i], hipMemcpyHostToDevice, s->st));
    off += plk_pad16(lens[i]);
  }
  std::vector<uint32_t> irr(ngroups, 1u);
  if (!s->irregular) {
    if ((rc = launch_fold(s, dp.data(), lens, weights, start, zs, ngroups, S.d + o_ys, d_res, nullptr, d_work, s->st, 0)))
      return rc;
    std::vector<uint8_t> h(32 * (size_t)ngroups);
    PLK_HIP(hipMemcpy2DAsync(h.data(), 32, d_res, sizeof(PlkMsmResult), 32, ngroups, hipMemcpyDeviceToHost, s->st));
    PLK_HIP(hipMemcpyAsync(ys, S.d + o_ys, np, hipMemcpyDeviceToHost, s->st));
    PLK_HIP(hipStreamSynchronize(s->st));
    for (int g = 0; g < ngroups; g++) {
      const PlkMsmResult* r = (const PlkMsmResult*)(h.data() + 32 * (size_t)g);
      irr[g] = r->irregular;
      memcpy(out3 + 3 * g, r->g1, 3);
    }
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
    if ((rc = launch_fold(s, dp.data() + a, lens + a, weights + a, one, zs + g, 1, S.d + o_ys + np, d_tmp, dq, d_work, s->st,
                          (uint32_t)g)))
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

int plk_kzg_fold_launch(const plk_srs* s, const uint8_t* const* d_polys, const size_t* lens, const uint8_t* weights,
                        const int* start, const uint8_t* zs, int ngroups, uint8_t* d_ys, PlkMsmResult* d_res,
                        uint8_t* const* d_quots, uint32_t* d_work, hipStream_t st, uint32_t row0) {
  return launch_fold(s, d_polys, lens, weights, start, zs, ngroups, d_ys, d_res, d_quots, d_work, st, row0);
}

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
  for (int b = 0; b < n; b++) words += chunks_of(lens[b]);
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
  if (!lens || !fold_layout_ok(start, ngroups)) return 0;
  uint64_t words = 0;
  for (int g = 0; g < ngroups; g++) {
    for (int i = start[g]; i < start[g + 1]; i++) words += chunks_of(lens[i]);
    words += chunks_of(fold_len(lens, start, g));
  }
  return (size_t)((4 * words + 255) & ~255ull);
}

int plk_kzg_open_fold_batch_dev(const plk_srs_t* s, const uint8_t* const* d_polys, const size_t* lens, const uint8_t* weights,
                                const int* start, const uint8_t* zs, int ngroups, uint8_t* d_ys, plk_msm_result_t* d_res,
                                uint8_t* const* d_quots, void* d_work, void* stream) {
  int rc = check_fold("plk_kzg_open_fold_batch_dev", s, d_polys, lens, weights, start, zs, ngroups, !d_ys || !d_res);
  if (rc) return rc;
  return launch_fold(s, d_polys, lens, weights, start, zs, ngroups, d_ys, d_res, d_quots, (uint32_t*)d_work,
                     (hipStream_t)stream, 0);
}

int plk_kzg_open_fold_batch(const plk_srs_t* s, const uint8_t* const* polys, const size_t* lens, const uint8_t* weights,
                            const int* start, const uint8_t* zs, int ngroups, uint8_t* ys, uint8_t* proofs3) {
  int rc = check_fold("plk_kzg_open_fold_batch", s, polys, lens, weights, start, zs, ngroups, !ys || !proofs3);
  if (rc) return rc;
  return host_fold(s, polys, lens, weights, start, zs, ngroups, ys, proofs3);
}

}  // extern "C"
