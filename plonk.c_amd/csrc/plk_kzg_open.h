// Device pieces of the KZG opening family (kzg.hip: commit, open, fold; kzg_multi.hip: multi-point;
// kzg_points.hip: per-point).
// One definition of each: the opening kernels are these pieces around their own loads.
// Everything is __forceinline__, so a kernel's code does not depend on which file it sits in.
// (Not for msm.hip or the headers it includes: bench.py hashes those.)
//
// The geometry all of them share: a block of T threads owns a chunk of CHUNK coefficients, a thread the
// E = 16 consecutive ones at base = chunk x CHUNK + thread x E.  Division by x - a (a != 0) is the suffix
// sum q[j] = a^-(j+1) sum_{i>j} p[i] a^i, and a^16 = 1 in GF(17), so the weights a^(i mod 16) do not depend
// on the chunk: the carry into a chunk is the plain sum mod 17 of the later chunks' aggregate words
// ([7:0] the sum mod 17, bit 8 set when a coefficient byte was >= 17), written by the launch before.
#pragma once
#include "plk_device.h"
#include "plk_hf17.h"
#include "plk_msm_finish.h"

namespace kzgo {

constexpr int T = 256, E = 16, CHUNK = T * E, WAVES = T / PLK_WAVE;

// a^0 .. a^15 mod 17, four to a word (uniform)
__device__ __forceinline__ void packed_powers(uint32_t a, uint32_t (&pk)[4]) {
  uint32_t v = 1;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      w |= v << (8 * j);
      v = v * a % hf17::P;
    }
    pk[i] = w;
  }
}
// sum_j byte j of w x byte j of pk (<= 16 x 255 x 255 < 2^20): v_dot4_u32_u8 on genuine bytes
__device__ __forceinline__ uint32_t dot16(const uint32_t (&w)[4], const uint32_t (&pk)[4]) {
  uint32_t t = __builtin_amdgcn_udot4(w[0], pk[0], 0u, false);
  t = __builtin_amdgcn_udot4(w[1], pk[1], t, false);
  t = __builtin_amdgcn_udot4(w[2], pk[2], t, false);
  return __builtin_amdgcn_udot4(w[3], pk[3], t, false);
}

// bytes [base, base + 16) of p[0, len), zero past len, any alignment: a rolled loop that shifts each byte
// in from the top (no indexed registers), a fraction of the unrolled hf17::load16's code for a rare path
__device__ __forceinline__ void load16_rolled(const uint8_t* p, uint64_t len, uint64_t base, uint32_t (&w)[4]) {
  uint32_t x0 = 0, x1 = 0, x2 = 0, x3 = 0;
#pragma nounroll
  for (int k = 0; k < 16; k++) {
    const uint32_t b = base + k < len ? p[base + k] : 0u;
    x0 = x0 >> 8 | x1 << 24;
    x1 = x1 >> 8 | x2 << 24;
    x2 = x2 >> 8 | x3 << 24;
    x3 = x3 >> 8 | b << 24;
  }
  w[0] = x0; w[1] = x1; w[2] = x2; w[3] = x3;
}
// the aligned whole run as one vector load
__device__ __forceinline__ void load16_vec(const uint8_t* p, uint64_t base, uint32_t (&w)[4]) {
  const uint4 v = *reinterpret_cast<const uint4*>(p + base);
  w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
}
__device__ __forceinline__ bool aligned16(const uint8_t* p) { return ((uintptr_t)p & 15u) == 0; }

// byte j of the same word of four polynomials in one word, polynomial u in byte u
__device__ __forceinline__ uint32_t transpose4(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, int j) {
  return ((w0 >> (8 * j)) & 0xFFu) | ((w1 >> (8 * j)) & 0xFFu) << 8 | ((w2 >> (8 * j)) & 0xFFu) << 16 |
         ((w3 >> (8 * j)) & 0xFFu) << 24;
}

// The scan of one single-point quotient.  tot: the thread's aggregate sum_k p[base + k] a^k mod 17; agg: the
// polynomial's aggregate words, word b = chunk b; ws: 2 x WAVES LDS words nobody else touches until the
// block's next barrier.  Returns the aggregates of the threads after this one plus the carry from the
// chunks after c (unreduced), and sets bad when a later chunk carries the flag.  Holds exactly one
// __syncthreads, after the block's LDS writes and before its reads: kzg_fold_open_kernel relies on
// it to order its own ysum words too, so it must stay unconditional.
// Coefficient 0 needs no special case: thread 0's own tot leaves by suf - tot, and it reaches nobody else,
// because wave 0's total is read only by the waves before it.
__device__ __forceinline__ uint32_t suffix_carry(uint32_t tot, const uint32_t* __restrict__ agg, uint32_t c,
                                                 uint32_t nchunk, uint32_t* ws, bool& bad) {
  uint32_t cs = 0;
  for (uint32_t b = c + 1 + threadIdx.x; b < nchunk; b += T) {
    const uint32_t v = agg[b];
    cs += v & 0xFFu;
    bad |= (v >> 8) != 0;
  }
  const uint32_t suf = hf17::wave_suffix(tot);   // this lane's coefficients and every later lane's
  const uint32_t cw = plk_wave_sum(cs % hf17::P);
  const int wv = (int)(threadIdx.x / PLK_WAVE);
  if ((threadIdx.x & (PLK_WAVE - 1)) == 0) {
    ws[wv] = suf;   // lane 0: the wave's total
    ws[WAVES + wv] = cw;
  }
  __syncthreads();
  uint32_t run = suf - tot;
#pragma unroll
  for (int u = 0; u < WAVES; u++) run += (u > wv ? ws[u] : 0u) + ws[WAVES + u];
  return run;
}

// The thread's sixteen quotient bytes for a != 0, handed to put(k, byte) from k = 15 down.  nb: the thread's
// sixteen bytes; run: suffix_carry's result = sum_{i >= base + 16} p[i] a^i, and a^-(base + 16) = 1: the top
// quotient byte is run itself, the others follow the division's recurrence q[j] = p[j + 1] + a q[j + 1].
// No bounds test: past the polynomial the bytes are zero and the last chunk has no carry, so q[j] = 0 there.
template <class Put>
__device__ __forceinline__ void quotient16(const uint32_t (&nb)[4], uint32_t a, uint32_t run, Put put) {
  uint32_t qv = run % hf17::P;
  put(E - 1, qv);
#pragma unroll
  for (int k = E - 2; k >= 0; k--) {
    qv = hf17::mod17(hf17::byte_of(nb, k + 1) + a * qv);   // (<= 255 + 16 x 16)
    put(k, qv);
  }
}
// a = 0: q[j] = p[j + 1], the thread's bytes one place down; nxt: coefficient base + 16
template <class Put>
__device__ __forceinline__ void shift16(const uint32_t (&nb)[4], uint32_t nxt, Put put) {
#pragma unroll
  for (int k = 0; k < E - 1; k++) put(k, hf17::byte_of(nb, k + 1));
  put(E - 1, nxt);
}
// the put of a kernel that keeps the sixteen bytes packed in four words (zeroed by the caller)
struct PackInto {
  uint32_t (&o)[4];
  __device__ __forceinline__ void operator()(int k, uint32_t v) const { o[k >> 2] |= v << (8 * (k & 3)); }
};

// bytes [base, base + 16) of q[0, n) from four words: one vector store when q is 16-byte aligned (vec) and
// the whole run is inside, else the bytes below n
__device__ __forceinline__ void store16(uint8_t* q, uint64_t n, uint64_t base, bool vec, const uint32_t (&o)[4]) {
  if (vec && base + 16 <= n) {
    *reinterpret_cast<uint4*>(q + base) = make_uint4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 16; k++)
      if (base + k < n) q[base + k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
  }
}

// The end of every kernel of the family: the thread's sixteen scalar bytes against the SRS logs, the block's
// sum, the ticketed finish of plk_msm_finish.h on the record.  stage() early (any barrier before finish()
// orders it), logs() wherever the kernel wants the load in flight, finish() last.
struct Finish {
  uint32_t etab[PLK_GROUP_ORDER];
  uint32_t wsum[WAVES];
  uint32_t wbad[WAVES];
  __device__ __forceinline__ void stage(const uint32_t* __restrict__ exp_words) {
    if (threadIdx.x < PLK_GROUP_ORDER) etab[threadIdx.x] = exp_words[threadIdx.x];
  }
  // the sixteen logs at base, zero from n on and when the SRS has no log form (logs: zero padded to 16)
  static __device__ __forceinline__ uint4 logs(const uint8_t* __restrict__ d_log, uint32_t srs_bad, uint64_t base,
                                               uint64_t n) {
    uint4 lg = make_uint4(0, 0, 0, 0);
    if (!srs_bad && base < n) lg = *reinterpret_cast<const uint4*>(d_log + base);
    return lg;
  }
  // block x of the X that share record res; row: the record's index in the call (the finish's shard spread)
  __device__ __forceinline__ void finish(const uint4& lg, const uint32_t (&o)[4], bool bad, PlkMsmResult* res,
                                         uint32_t x, uint32_t X, uint32_t row) {
    const uint32_t l[4] = {lg.x, lg.y, lg.z, lg.w};
    const uint32_t t = dot16(l, o);   // 16 x 101 x 255 < 2^19
    (void)msm_finish_xy<T>(t % PLK_GROUP_ORDER, bad, res, wsum, wbad, etab, x, X, row);
  }
};

}  // namespace kzgo
