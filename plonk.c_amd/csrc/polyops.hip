// The polynomial and matrix ops around the hot path on gfx950:
//
//   poly_eval        src/poly.h:265-272   Horner over GF(17) on raw bytes
//   poly_divide      src/poly.h:124-177   long division num = quot * den + rem
//   matrix_mul       src/matrix.h:79-96   (interpolate_at_h, src/plonk.h:162-195)
//   matrix_inv       src/matrix.h:100-176 (plonk_new's Vandermonde inverse, src/plonk.h:105-113)
//
// Every op reproduces the reference's BYTE arithmetic, including non-canonical coefficient
// bytes (HF values >= 17): hf_add is a uint8 sum with one conditional subtract, hf_sub an int8
// difference with one conditional add, hf_mul (a * b) % 17 (src/hf.h:79-116).  The parallel
// paths hold on canonical inputs (or, for poly_eval, on inputs where no uint8 sum can wrap);
// the kernels detect the other inputs and run the reference's loop serially on the device.
#include "plk_device.h"
#include "plk_hf17.h"
#include "plk_internal.h"

#include <stdlib.h>
#include <string.h>

namespace {

constexpr uint32_t HP = hf17::P;
using hf17::add8;
using hf17::mul8;
using hf17::noncanonical4;
using hf17::pow16;
using hf17::sub8;
__constant__ uint8_t c_hinv17[17] = {0, 1, 9, 6, 13, 7, 3, 5, 15, 2, 12, 14, 10, 4, 11, 8, 16};

// block-wide sum of per-thread values (every thread calls; result valid in thread 0)
template <int NT>
__device__ __forceinline__ uint32_t block_sum(uint32_t v) {
  __shared__ uint32_t ws[NT / PLK_WAVE];
  v = plk_wave_sum(v);
  if ((threadIdx.x & (PLK_WAVE - 1)) == 0) ws[threadIdx.x / PLK_WAVE] = v;
  __syncthreads();
  uint32_t t = 0;
  if (threadIdx.x == 0)
#pragma unroll
    for (int w = 0; w < NT / PLK_WAVE; w++) t += ws[w];
  return t;
}

// ---------------------------------------------------------------------------------------
// poly_eval.  Horner: y = 0; for i = len-1 .. 0: y = hf_add(hf_mul(y, x), c_i).  hf_mul
// reduces mod 17, so only the residue of an intermediate y matters -- except that hf_add's
// uint8 sum can wrap (256 = 1 mod 17 changes the residue), which needs c_i >= 240.  With no
// such c_i at i >= 1, y_1 = S = sum_{i>=1} c_i x^(i-1) (mod 17), and the output is the exact
// byte hf_add((S x) % 17, c_0).  x^e = x^(e mod 16) for x != 0 (mod 17).  A job with a
// c_i >= 240 (i >= 1) is re-run by its last block with the reference's loop.
// ---------------------------------------------------------------------------------------
constexpr int EVAL_NT = 256;
struct EvalJobs {
  const uint8_t* p[PLK_EVAL_MAX_JOBS];
  uint64_t len[PLK_EVAL_MAX_JOBS];
  uint8_t x[PLK_EVAL_MAX_JOBS];
};

__global__ __launch_bounds__(EVAL_NT) void eval_batch_kernel(EvalJobs J, uint8_t* __restrict__ y,
                                                             unsigned long long* __restrict__ tick) {
  const int job = blockIdx.y;
  const uint8_t* p = J.p[job];
  const uint64_t len = J.len[job];
  const uint32_t xm = J.x[job] % HP;
  // pw[i mod 16] = x^(i - 1) for i >= 1 (x = 0: only i = 1 contributes)
  uint32_t pw[16];
  {
    uint32_t e = 1;   // x^0
#pragma unroll
    for (int t = 1; t <= 16; t++) {
      pw[t & 15] = xm == 0 ? (t == 1 ? 1u : 0u) : e;
      e = e * xm % HP;
    }
  }
  uint32_t acc = 0, bad = 0;
  const uint64_t chunks = (len + 15) >> 4;
  const bool vec = ((uintptr_t)p & 15) == 0;
  for (uint64_t c = (uint64_t)blockIdx.x * EVAL_NT + threadIdx.x; c < chunks; c += (uint64_t)gridDim.x * EVAL_NT) {
    const uint64_t i0 = c << 4;
    uint32_t w[4];
    if (vec && i0 + 16 <= len) {
      const uint4 v = *reinterpret_cast<const uint4*>(p + i0);
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
#pragma unroll
      for (int q = 0; q < 4; q++) w[q] = 0;
      for (int k = 0; k < 16; k++)
        if (i0 + k < len) w[k >> 2] |= (uint32_t)p[i0 + k] << (8 * (k & 3));
    }
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const uint32_t b = (w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
      const bool live = i0 + k > 0;           // c_0 is added exactly at the end
      acc += live ? b * pw[k] : 0u;           // (i0 + k) mod 16 = k; < 2^20 per chunk
      bad |= (live && b >= 240u) ? 1u : 0u;
    }
    acc %= HP;
  }
  const uint32_t s = block_sum<EVAL_NT>(acc % HP);
  const uint32_t anybad = __syncthreads_or(bad);
  if (threadIdx.x != 0) return;
  const unsigned long long add = (unsigned long long)(s % HP) | (1ull << 32) | ((unsigned long long)(anybad != 0) << 48);
  const unsigned long long old = atomicAdd(&tick[job * 16], add);
  if (((old >> 32) & 0xFFFFull) != gridDim.x - 1) return;
  const unsigned long long tot = old + add;
  atomicExch(&tick[job * 16], 0ull);
  uint32_t out = 0;
  if ((tot >> 48) == 0) {
    const uint32_t S = (uint32_t)(tot & 0xFFFFFFFFull) % HP;
    out = len ? add8(S * xm % HP, p[0]) : 0u;
  } else {   // the reference's loop, exactly
    const uint32_t xr = J.x[job];
    for (uint64_t i = len; i-- > 0;) out = add8(mul8(out, xr), p[i]);
  }
  y[job] = (uint8_t)out;
}

// ---------------------------------------------------------------------------------------
// poly_divide.  The reference's loop (for i = nl-1 .. dl-1: c = rem[i] * inv(lead);
// q[i-dl+1] = c; rem[i-j] -= c den[dl-1-j] for j < dl) on raw bytes, one thread: the general
// divisor and non-canonical inputs.
// ---------------------------------------------------------------------------------------
// The reference's loop (src/poly.h:124-177) on raw bytes, one thread.  den == nullptr: the
// binomial divisor lead x^(dl-1) + d0 given by its two bytes (the gated re-run behind the chain
// scans: no host-to-device copy of a mostly-zero divisor per call).
// The running remainder lives in the workspace (nl bytes); the caller's rem receives its first
// min(dl - 1, nl) bytes (the size plk_poly_divide_dev documents).
__device__ void serial_divide(const uint8_t* __restrict__ num, uint64_t nl, const uint8_t* __restrict__ den, uint64_t dl,
                              uint32_t d0, uint32_t lead, uint8_t* __restrict__ q, uint64_t qcap,
                              uint8_t* __restrict__ rem, uint64_t rl, uint8_t* __restrict__ run) {
  for (uint64_t i = 0; i < qcap; i++) q[i] = 0;
  for (uint64_t i = 0; i < nl; i++) run[i] = num[i];
  auto den_at = [&](uint64_t i) -> uint32_t { return den ? den[i] : (i == 0 ? d0 : (i == dl - 1 ? lead : 0u)); };
  const uint32_t inv = c_hinv17[den_at(dl - 1)];   // lead < 17 (host-checked)
  for (uint64_t i = nl; i-- > dl - 1;) {
    const uint32_t c = mul8(run[i], inv);
    q[i - (dl - 1)] = (uint8_t)c;
    // every j, zero divisor bytes included: hf_sub of raw bytes normalises as the reference does
    for (uint64_t j = 0; j < dl; j++) run[i - j] = (uint8_t)sub8(run[i - j], mul8(c, den_at(dl - 1 - j)));
  }
  for (uint64_t i = 0; i < rl; i++) rem[i] = run[i];
}

__device__ __forceinline__ uint32_t fin_block_max(uint32_t v, uint32_t* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_xor(v, off, PLK_WAVE));
  __syncthreads();
  if ((threadIdx.x & (PLK_WAVE - 1)) == 0) red[threadIdx.x / PLK_WAVE] = v;
  __syncthreads();
  uint32_t m = 0;
  for (int w = 0; w < (int)(blockDim.x / PLK_WAVE); w++) m = max(m, red[w]);
  return m;
}
// index + 1 of the last non-zero byte of p[0, len) (0: all zero), scanning back 16 KiB at a time
__device__ uint32_t fin_trim(const uint8_t* __restrict__ p, uint64_t len, uint32_t* red) {
  constexpr int64_t CH = 16384;
  for (int64_t end = (int64_t)len; end > 0; end -= CH) {
    const int64_t start = end > CH ? end - CH : 0;
    uint32_t last = 0;
    for (int64_t i = start + threadIdx.x; i < end; i += blockDim.x)
      if (p[i]) last = max(last, (uint32_t)(i + 1));
    last = fin_block_max(last, red);
    if (last) return last;
  }
  return 0;
}

// ONE launch after the division kernels: the reference's loop when it is needed (mode 1: always,
// the divisor copied to the device; mode 2: only when the chain scans flagged non-canonical
// numerator bytes, binomial divisor by its two bytes -- or, behind the Newton path, the divisor's
// device copy), then the trimmed lengths of q and rem
// (src/poly.h:158-170) -- three launches (serial re-run + two trims) folded into one.
__global__ __launch_bounds__(1024) void div_finish_kernel(const uint8_t* __restrict__ num, uint64_t nl,
                                                         const uint8_t* __restrict__ den, uint64_t dl, uint32_t d0,
                                                         uint32_t lead, uint8_t* __restrict__ q, uint64_t ql,
                                                         uint8_t* __restrict__ rem, uint64_t rl, int mode,
                                                         const uint32_t* __restrict__ gate, uint8_t* __restrict__ scratch,
                                                         uint32_t* __restrict__ lens) {
  __shared__ uint32_t red[16];
  const bool run = mode == 1 || (mode == 2 && *gate != 0);   // uniform
  if (run && threadIdx.x == 0) serial_divide(num, nl, den, dl, d0, lead, q, ql, rem, rl, scratch);
  __syncthreads();   // thread 0's global writes are visible to the block after the barrier
  const uint32_t lq = fin_trim(q, ql, red);
  const uint32_t lr = rl ? fin_trim(rem, rl, red) : 0u;
  if (threadIdx.x == 0) {
    lens[0] = lq;
    lens[1] = lr;
  }
}

// Divisor lead x^m + d0 (every other coefficient zero; m = dl - 1 >= 1), canonical bytes.  The
// loop gives q[k] = inv (num[k+m] - d0 q[k+m]) = v_k + A q[k+m] with A = -d0 inv, v_k = inv
// num[k+m]: m independent chains k = r, r + m, r + 2m, ...  and rem[t] = num[t] - d0 q[t]
// (t < m).  Short chains: one thread walks a chain from its top.
struct Binom {
  const uint8_t* num;
  uint64_t nl, m, lq;      // lq = nl - m quotient coefficients
  uint32_t inv, d0;
  uint8_t* q;
  uint8_t* rem;
  uint32_t* flag;          // set when some num byte is not canonical (serial path re-runs)
};

__global__ __launch_bounds__(256) void div_binom_short_kernel(Binom B) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= B.m) return;
  const uint32_t A = (HP - B.d0 * B.inv % HP) % HP;
  uint32_t prev = 0, bad = 0;
  if (r < B.lq) {
    const uint64_t cnt = (B.lq - 1 - r) / B.m + 1;
    for (uint64_t t = cnt; t-- > 0;) {
      const uint64_t k = r + t * B.m;
      const uint32_t b = B.num[k + B.m];
      bad |= b >= HP;
      prev = (b * B.inv + A * prev) % HP;
      B.q[k] = (uint8_t)prev;
    }
  }
  if (r < B.nl) {   // remainder coefficient r (r < m); prev = q[r], 0 when r has no quotient
    const uint32_t b = B.num[r];
    bad |= b >= HP;
    B.rem[r] = (uint8_t)((b + (HP - B.d0) * prev) % HP);
  }
  if (bad) atomicOr(B.flag, 1u);
}

// Long chains (m small, e.g. the linear divisors x - z of src/plonk.h:604-613): with A != 0,
// q_p = A^-p sum_{s >= p} A^s v_s along a chain (positions p; A^16 = 1), a suffix sum --
// two phases over blocks of SCAN_B positions: block aggregates, then each block reduces the
// aggregates after it and scans within itself.  A = 0 needs no scan (q = v).
constexpr int SCAN_T = 256, SCAN_E = 16, SCAN_B = SCAN_T * SCAN_E;

// chain r = blockIdx.y + y0, positions [blockIdx.x SCAN_B, +SCAN_B)
__global__ __launch_bounds__(SCAN_T) void div_binom_sums_kernel(Binom B, uint64_t y0, uint64_t nblk,
                                                                uint32_t* __restrict__ bsum) {
  const uint64_t r = y0 + blockIdx.y;
  const uint64_t len = (B.lq - 1 - r) / B.m + 1;   // chain length (r < min(m, lq): host)
  const uint32_t A = (HP - B.d0 * B.inv % HP) % HP;
  uint32_t pw[16];
  pow16(A, pw);
  const uint64_t p0 = (uint64_t)blockIdx.x * SCAN_B + (uint64_t)threadIdx.x * SCAN_E;
  uint32_t acc = 0, bad = 0;
#pragma unroll
  for (int e = 0; e < SCAN_E; e++) {
    const uint64_t p = p0 + e;
    if (p < len) {
      const uint32_t b = B.num[r + (p + 1) * B.m];
      bad |= b >= HP;
      acc += b * B.inv % HP * pw[p & 15];
    }
  }
  const uint32_t t = block_sum<SCAN_T>(acc % HP);
  if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(B.flag, 1u);
  if (threadIdx.x == 0) bsum[blockIdx.y * nblk + blockIdx.x] = t % HP;
}

__global__ __launch_bounds__(SCAN_T) void div_binom_apply_kernel(Binom B, uint64_t y0, uint64_t nblk,
                                                                 const uint32_t* __restrict__ bsum) {
  __shared__ uint32_t wtot[SCAN_T / PLK_WAVE];
  __shared__ uint32_t carry_s;
  const uint64_t r = y0 + blockIdx.y;
  const uint64_t len = (B.lq - 1 - r) / B.m + 1;
  const uint32_t A = (HP - B.d0 * B.inv % HP) % HP;
  uint32_t pw[16], ipw[16];
  pow16(A, pw);
  pow16(c_hinv17[A], ipw);
  // carry: aggregates of the blocks after this one
  if (threadIdx.x < PLK_WAVE) {
    uint32_t c = 0;
    for (uint64_t b = blockIdx.x + 1 + threadIdx.x; b < nblk; b += PLK_WAVE) c += bsum[blockIdx.y * nblk + b];
    c = plk_wave_sum(c % HP);
    if (threadIdx.x == 0) carry_s = c % HP;
  }
  const uint64_t p0 = (uint64_t)blockIdx.x * SCAN_B + (uint64_t)threadIdx.x * SCAN_E;
  uint32_t v[SCAN_E], tot = 0;
#pragma unroll
  for (int e = 0; e < SCAN_E; e++) {
    const uint64_t p = p0 + e;
    v[e] = p < len ? B.num[r + (p + 1) * B.m] * B.inv % HP : 0u;
    tot += A ? v[e] * pw[p & 15] : 0u;
  }
  tot %= HP;
  // exclusive suffix over threads: sum of the totals of threads after this one
  const int lane = threadIdx.x & (PLK_WAVE - 1), wave = threadIdx.x / PLK_WAVE;
  uint32_t suf = tot;
#pragma unroll
  for (int d = 1; d < PLK_WAVE; d <<= 1) {
    const uint32_t o = __shfl_down(suf, d, PLK_WAVE);
    if (lane + d < PLK_WAVE) suf += o;
  }
  if (lane == 0) wtot[wave] = suf % HP;
  __syncthreads();
  uint32_t after = (suf - tot) % HP + carry_s;   // this wave's threads after me, + later blocks
  for (int w = wave + 1; w < SCAN_T / PLK_WAVE; w++) after += wtot[w];
  after %= HP;
  uint32_t run = after;   // sum_{s > p} A^s v_s
  uint32_t q0 = 0;
#pragma unroll
  for (int e = SCAN_E - 1; e >= 0; e--) {
    const uint64_t p = p0 + e;
    if (p < len) {
      uint32_t qv;
      if (A) {
        run = (run + v[e] * pw[p & 15]) % HP;
        qv = run * ipw[p & 15] % HP;
      } else {
        qv = v[e];
      }
      B.q[r + p * B.m] = (uint8_t)qv;
      if (p == 0) q0 = qv;
    }
  }
  if (p0 == 0 && r < B.nl) {
    const uint32_t b = B.num[r];
    if (b >= HP) atomicOr(B.flag, 1u);
    B.rem[r] = (uint8_t)((b % HP + (HP - B.d0) * q0) % HP);
  }
}

// divisor of length 1 (m = 0): q = num * inv(lead) bytewise, no remainder coefficients
__global__ __launch_bounds__(256) void div_const_kernel(const uint8_t* __restrict__ num, uint64_t nl, uint32_t inv,
                                                        uint8_t* __restrict__ q) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nl; i += (uint64_t)gridDim.x * blockDim.x)
    q[i] = (uint8_t)mul8(num[i], inv);
}

// ---------------------------------------------------------------------------------------
// General divisors: Newton inverse over the exact products.  With m = dl - 1,
// k = nl - m, f = rev(den) (f[0] = lead), a = rev(num): g = f^-1 mod x^k, rev(q) = a g mod x^k,
// rem = num - q den mod x^m.  On canonical bytes that is the reference's loop (Euclidean
// division is unique); a numerator byte >= 17 sets the flag and div_finish_kernel re-runs the loop.
// The kernels below are the glue between the products: 16 bytes per thread at any address (num, q
// and rem are the caller's buffers), truncation and zero padding done here, not by memsets.
// ---------------------------------------------------------------------------------------
struct __attribute__((packed, aligned(1))) U4u {   // 16 bytes at any address (caller buffers)
  uint32_t x, y, z, w;
};
// per byte (17 - b) % 17, bytes < 17
__device__ __forceinline__ uint32_t neg4(uint32_t w) {
  uint32_t r = 0;
#pragma unroll
  for (int s = 0; s < 32; s += 8) {
    const uint32_t b = (w >> s) & 0xFFu;
    r |= (b ? HP - b : 0u) << s;
  }
  return r;
}
// per byte (a + 17 - b) % 17, b < 17 (a >= 17 gives some byte: the flagged re-run overwrites it)
__device__ __forceinline__ uint32_t sub4(uint32_t a, uint32_t b) {
  uint32_t r = 0;
#pragma unroll
  for (int s = 0; s < 32; s += 8) r |= ((((a >> s) & 0xFFu) + HP - ((b >> s) & 0xFFu)) % HP) << s;
  return r;
}

// dst[j] = src[n - 1 - j], j < n: 16 bytes per thread, reversed by byte permutes; check: a byte
// >= 17 sets the flag.  Job blockIdx.y (the numerator's top k bytes and the divisor in one launch).
struct RevJob {
  const uint8_t* src;
  uint8_t* dst;
  uint64_t n;
  int check;
};
struct RevJobs {
  RevJob j[2];
  uint32_t* flag;
};
__global__ __launch_bounds__(256) void div_reverse_kernel(RevJobs J) {
  const RevJob jb = J.j[blockIdx.y];
  const uint64_t chunks = (jb.n + 15) >> 4;
  uint32_t bad = 0;
  for (uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x; c < chunks; c += (uint64_t)gridDim.x * 256) {
    const uint64_t j0 = c << 4;
    if (j0 + 16 <= jb.n) {
      const U4u v = *reinterpret_cast<const U4u*>(jb.src + (jb.n - 16 - j0));
      bad |= noncanonical4(v.x) | noncanonical4(v.y) | noncanonical4(v.z) | noncanonical4(v.w);
      U4u o;
      o.x = __builtin_bswap32(v.w);
      o.y = __builtin_bswap32(v.z);
      o.z = __builtin_bswap32(v.y);
      o.w = __builtin_bswap32(v.x);
      *reinterpret_cast<U4u*>(jb.dst + j0) = o;
    } else {
      for (uint64_t j = j0; j < jb.n; j++) {
        const uint32_t b = jb.src[jb.n - 1 - j];
        bad |= b >= HP;
        jb.dst[j] = (uint8_t)b;
      }
    }
  }
  if (jb.check && bad) atomicOr(J.flag, 1u);
}

// g[0, B) = f^-1 mod x^B in one block, g and f in LDS (B <= INV_B0; f zero past fl).  Thread i
// owns acc_i = sum_{j >= 1} f[j] g[i - j] over the g known so far and g[i] = -inv(f[0]) acc_i.
// 64 coefficients at a time: their wave solves its triangle with lane broadcasts (no barrier),
// then every later thread adds the 64 new terms -- B / 64 barriers instead of B reductions.
constexpr int INV_B0 = 1024;
__global__ __launch_bounds__(INV_B0) void div_base_inverse_kernel(const uint8_t* __restrict__ f, uint32_t fl,
                                                                  uint32_t B, uint8_t* __restrict__ g) {
  __shared__ __attribute__((aligned(16))) uint8_t sf[INV_B0], sg[INV_B0];
  const uint32_t tid = threadIdx.x, lane = tid & (PLK_WAVE - 1);
  sf[tid] = tid < fl ? f[tid] : (uint8_t)0;
  sg[tid] = 0;
  __syncthreads();
  const uint32_t inv0 = c_hinv17[sf[0]], ninv = (HP - inv0) % HP;
  uint32_t acc = 0;
  for (uint32_t base = 0; base < B; base += PLK_WAVE) {
    if ((tid & ~(uint32_t)(PLK_WAVE - 1)) == base) {   // (wave-uniform)
      uint32_t gi = 0;
      for (uint32_t s = 0; s < PLK_WAVE; s++) {
        // final in lane s (acc < 17 + 63 * 256); s is uniform: a v_readlane, not an LDS permute
        const uint32_t mine = tid == 0 ? inv0 : ninv * acc % HP;
        const uint32_t gs = (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)s);
        if (lane == s) gi = gs;
        if (lane > s) acc += sf[lane - s] * gs;
      }
      sg[tid] = (uint8_t)gi;
    }
    __syncthreads();
    if (tid >= base + PLK_WAVE && tid < B) {
      const uint32_t* g4 = reinterpret_cast<const uint32_t*>(sg + base);   // (broadcast reads, 4 g per word)
      const uint8_t* fw = sf + (tid - base);
#pragma unroll 4
      for (uint32_t s = 0; s < PLK_WAVE; s += 4) {
        const uint32_t w = g4[s >> 2];
        acc += fw[-(int)s] * (w & 0xFFu) + fw[-(int)s - 1] * ((w >> 8) & 0xFFu) + fw[-(int)s - 2] * ((w >> 16) & 0xFFu) +
               fw[-(int)s - 3] * (w >> 24);
      }
      acc %= HP;
    }
  }
  if (tid < B) g[tid] = sg[tid];
}

// One Newton step t -> n2 = min(2t, k): with e = f g mod x^n2 = 1 + x^t e', the new upper half
// is g[t, n2) = (g[0, t) (-e'))[0, n2 - t).  This kernel forms E = -e' from the first product
// P = f[0, fl2) g[0, t) (pl bytes; zero past them): E[i] = -P[t + i], i < cnt; the second product
// writes g[t, ..) itself.
__global__ __launch_bounds__(256) void div_newton_neg_kernel(const uint8_t* __restrict__ P, uint64_t pl, uint64_t t,
                                                             uint8_t* __restrict__ E, uint64_t cnt) {
  const uint64_t chunks = (cnt + 15) >> 4;
  for (uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x; c < chunks; c += (uint64_t)gridDim.x * 256) {
    const uint64_t i0 = c << 4;
    if (i0 + 16 <= cnt && t + i0 + 16 <= pl) {
      const U4u v = *reinterpret_cast<const U4u*>(P + t + i0);
      U4u o;
      o.x = neg4(v.x);
      o.y = neg4(v.y);
      o.z = neg4(v.z);
      o.w = neg4(v.w);
      *reinterpret_cast<U4u*>(E + i0) = o;
    } else {
      for (uint64_t i = i0; i < cnt && i < i0 + 16; i++) {
        const uint32_t b = t + i < pl ? P[t + i] : 0u;
        E[i] = (uint8_t)(b ? HP - b : 0u);
      }
    }
  }
}

// rem[i] = num[i] - R[i] mod 17, i < m (R = q den's low bytes, workspace); checks num[0, m)
__global__ __launch_bounds__(256) void div_rem_sub_kernel(const uint8_t* __restrict__ num, const uint8_t* __restrict__ R,
                                                          uint64_t m, uint8_t* __restrict__ rem,
                                                          uint32_t* __restrict__ flag) {
  const uint64_t chunks = (m + 15) >> 4;
  uint32_t bad = 0;
  for (uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x; c < chunks; c += (uint64_t)gridDim.x * 256) {
    const uint64_t i0 = c << 4;
    if (i0 + 16 <= m) {
      const U4u a = *reinterpret_cast<const U4u*>(num + i0);
      const U4u r = *reinterpret_cast<const U4u*>(R + i0);
      bad |= noncanonical4(a.x) | noncanonical4(a.y) | noncanonical4(a.z) | noncanonical4(a.w);
      U4u o;
      o.x = sub4(a.x, r.x);
      o.y = sub4(a.y, r.y);
      o.z = sub4(a.z, r.z);
      o.w = sub4(a.w, r.w);
      *reinterpret_cast<U4u*>(rem + i0) = o;
    } else {
      for (uint64_t i = i0; i < m; i++) {
        const uint32_t a = num[i];
        bad |= a >= HP;
        rem[i] = (uint8_t)((a + HP - R[i]) % HP);
      }
    }
  }
  if (bad) atomicOr(flag, 1u);
}

// ---------------------------------------------------------------------------------------
// matrices (row-major bytes, src/matrix.h).  matrix_mul: sum = hf_add(sum, hf_mul(a, b)) per
// element (one thread each).  matrix_inv: Gauss-Jordan on [M | I] exactly as
// matrix_gauss_jordan (src/matrix.h:100-147) -- pivot search, swaps, normalisation and
// elimination in the reference's order, one workgroup (n is |H| <= 17 in GF(17)).
// ---------------------------------------------------------------------------------------
__global__ void matrix_mul_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint64_t m, uint64_t k,
                                  uint64_t n, uint8_t* __restrict__ out) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m * n; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = e / n, j = e % n;
    uint32_t s = 0;
    for (uint64_t t = 0; t < k; t++) s = add8(s, mul8(a[i * k + t], b[t * n + j]));
    out[e] = (uint8_t)s;
  }
}

// aug: n x 2n workspace (global); one block of 256 threads; columns in parallel per row op
__global__ __launch_bounds__(256) void matrix_inv_kernel(const uint8_t* __restrict__ mat, uint64_t n,
                                                         uint8_t* __restrict__ aug, uint8_t* __restrict__ out) {
  const uint64_t cols = 2 * n;
  for (uint64_t e = threadIdx.x; e < n * cols; e += blockDim.x) {
    const uint64_t i = e / cols, j = e % cols;
    aug[e] = j < n ? mat[i * n + j] : (j - n == i ? 1 : 0);
  }
  __syncthreads();
  __shared__ uint64_t s_i, s_lead;
  __shared__ int s_stop;
  uint64_t lead = 0;
  for (uint64_t r = 0; r < n; r++) {
    if (threadIdx.x == 0) {   // pivot search (src/matrix.h:108-118), serial as in the reference
      int stop = lead >= cols;
      uint64_t i = r;
      while (!stop && aug[i * cols + lead] == 0) {
        i++;
        if (i == n) {
          i = r;
          lead++;
          if (lead == cols) stop = 1;
        }
      }
      s_i = i;
      s_lead = lead;
      s_stop = stop;
    }
    __syncthreads();
    if (s_stop) break;
    lead = s_lead;
    const uint64_t i = s_i;
    if (i != r)
      for (uint64_t k = threadIdx.x; k < cols; k += blockDim.x) {
        const uint8_t t = aug[i * cols + k];
        aug[i * cols + k] = aug[r * cols + k];
        aug[r * cols + k] = t;
      }
    __syncthreads();
    const uint32_t div = aug[r * cols + lead];
    __syncthreads();
    if (div != 0)   // hf_div(value, div) = value * inv(div); div < 17 (host-checked bytes)
      for (uint64_t k = threadIdx.x; k < cols; k += blockDim.x)
        aug[r * cols + k] = (uint8_t)mul8(aug[r * cols + k], c_hinv17[div]);
    __syncthreads();
    // eliminate every other row (src/matrix.h:130-143): rows are independent given row r, so in
    // parallel; each row's multiplier is captured before its update
    __shared__ uint8_t mults[1024];
    for (uint64_t ii = threadIdx.x; ii < n; ii += blockDim.x) mults[ii] = aug[ii * cols + lead];
    __syncthreads();
    for (uint64_t e = threadIdx.x; e < n * cols; e += blockDim.x) {
      const uint64_t ii = e / cols, k = e % cols;
      if (ii == r) continue;
      aug[e] = (uint8_t)sub8(aug[e], mul8(aug[r * cols + k], mults[ii]));
    }
    __syncthreads();
    lead++;
  }
  __syncthreads();
  for (uint64_t e = threadIdx.x; e < n * n; e += blockDim.x) out[e] = aug[(e / n) * cols + n + e % n];
}

}  // namespace

// ------------------------------------------------------------------------------ launchers
int plk_poly_eval_batch_launch(const uint8_t* const* polys, const uint64_t* lens, const uint8_t* xs, int nj,
                               uint8_t* d_y, void* d_tick, hipStream_t st) {
  if (nj < 1 || nj > PLK_EVAL_MAX_JOBS) {
    plk_set_error("poly_eval batch: %d jobs (1..%d)", nj, PLK_EVAL_MAX_JOBS);
    return PLK_ERR_ARG;
  }
  EvalJobs J{};
  uint64_t mx = 0;
  for (int i = 0; i < nj; i++) {
    if (!polys[i] && lens[i]) {
      plk_set_error("poly_eval batch: job %d has a NULL polynomial", i);
      return PLK_ERR_ARG;
    }
    J.p[i] = polys[i];
    J.len[i] = lens[i];
    J.x[i] = xs[i];
    mx = lens[i] > mx ? lens[i] : mx;
  }
  // blocks per job: one per 64 KiB, at most 64 (the finish's ticket sums 16 bits)
  uint64_t nb = (mx + 65535) >> 16;
  nb = nb < 1 ? 1 : (nb > 64 ? 64 : nb);
  hipLaunchKernelGGL(eval_batch_kernel, dim3((unsigned)nb, nj), dim3(EVAL_NT), 0, st, J, d_y,
                     (unsigned long long*)d_tick);
  PLK_HIP(hipGetLastError());
  return PLK_OK;
}

static size_t divide_base_bytes(uint64_t nl, uint64_t dl) {
  // den copy + flag/length words + scan block aggregates (long chains)
  const uint64_t m = dl ? dl - 1 : 0;
  const uint64_t lq = nl >= dl ? nl - m : 0;
  const uint64_t chains = m < lq ? m : lq;
  const uint64_t len = chains ? (lq + m - 1) / (m ? m : 1) : 0;
  const uint64_t nblk = (len + SCAN_B - 1) / SCAN_B;
  return 256 + ((dl + 15) & ~15ull) + 4 * (chains * nblk + 16) + ((nl + 15) & ~15ull);   // + the serial remainder
}

// The Newton path's shapes and its buffers behind the base workspace (offsets from d_work, each
// a multiple of 256): g (the second product of a step writes g[t, ..) itself, t + n2 - 1 <= 2k
// bytes), the reversed operands, one product output, E, and the largest product's workspace.
struct NewtonPlan {
  // fl = min(dl, k) coefficients of f are ever read; B: the base inverse's size, k halved (rounding
  // up) until it is <= INV_B0, so that the doublings end at k with no short last step
  uint64_t m, k, fl, B;
  size_t o_g, o_ar, o_f, o_p, o_e, o_mw, total;
};
static uint64_t up256(uint64_t v) { return (v + 255) & ~255ull; }
static bool newton_shape(uint64_t nl, uint64_t dl) { return dl >= 3 && nl >= dl && nl <= (1ull << 31); }
static NewtonPlan newton_plan(uint64_t nl, uint64_t dl) {
  NewtonPlan p{};
  p.m = dl - 1;
  p.k = nl - p.m;
  p.fl = dl < p.k ? dl : p.k;
  for (p.B = p.k; p.B > (uint64_t)INV_B0;) p.B = (p.B + 1) / 2;
  const uint64_t kq = p.k < p.m ? p.k : p.m;
  uint64_t pout = 2 * p.k - 1, mw = plk_poly_mul_workspace_bytes(p.k, p.k);   // rev(q) = a g
  auto product = [&](uint64_t la, uint64_t lb, bool to_p) {
    if (to_p && la + lb - 1 > pout) pout = la + lb - 1;
    const uint64_t w = plk_poly_mul_workspace_bytes(la, lb);
    if (w > mw) mw = w;
  };
  product(kq, p.m, true);   // q den
  for (uint64_t t = p.B; t < p.k;) {
    const uint64_t n2 = 2 * t < p.k ? 2 * t : p.k;
    product(p.fl < n2 ? p.fl : n2, t, true);
    product(t, n2 - t, false);
    t = n2;
  }
  size_t o = up256(divide_base_bytes(nl, dl));
  p.o_g = o, o += up256(2 * p.k);
  p.o_ar = o, o += up256(p.k);
  p.o_f = o, o += up256(p.fl);
  p.o_p = o, o += up256(pout);
  p.o_e = o, o += up256((p.k + 1) / 2);
  p.o_mw = o, o += up256(mw);
  p.total = o;
  return p;
}

// covers the Newton buffers of every shape that could take that path, whatever
// PLK_OPT_DIVIDE_FAST_MIN is now
size_t plk_poly_divide_workspace_bytes(uint64_t nl, uint64_t dl) {
  return newton_shape(nl, dl) ? newton_plan(nl, dl).total : divide_base_bytes(nl, dl);
}

// The divisor's class, from one pass over its (host) bytes.  path: 0 trivial (nl < dl), 1 constant,
// 2 binomial scan, 3 the reference's loop on one thread, 4 Newton; a zero divisor or a lead byte
// >= 17: the error code negated (the message is set).
struct DivClass {
  int path;
  bool canonical_den, binom;   // every byte < 17; no non-zero byte between den[0] and the lead
};
static int divide_path(const uint8_t* den, uint64_t dl, uint64_t nl, bool any, bool canonical_den, bool binom) {
  if (!any) {
    plk_set_error("Division by zero polynomial in poly_divide");
    return -PLK_ERR_ARG;
  }
  const uint32_t lead = den[dl - 1];
  if (lead >= HP) {   // the reference indexes hf_inverses[17] out of bounds: undefined
    plk_set_error("poly_divide: divisor lead byte %u is not a GF(17) value (reference behaviour undefined)", lead);
    return -PLK_ERR_RANGE;
  }
  if (canonical_den && binom && lead != 0) return nl < dl ? 0 : (dl == 1 ? 1 : 2);
  if (nl < dl) return 0;
  const uint64_t fast = (uint64_t)plk_opt(PLK_OPT_DIVIDE_FAST_MIN);
  const uint64_t ql = nl - dl + 1;
  // (ql dl >= fast, without the product's overflow)
  if (fast && canonical_den && lead != 0 && newton_shape(nl, dl) && dl >= (fast + ql - 1) / ql) return 4;
  return 3;
}
static DivClass divide_classify(const uint8_t* den, uint64_t dl, uint64_t nl) {
  // (plain OR reductions, which the host compiler vectorises: a 2^20-byte divisor is scanned per call)
  uint8_t any = 0, big = 0, mid = 0;
  for (uint64_t i = 0; den && i < dl; i++) {
    any |= den[i];
    big |= (uint8_t)(den[i] >= HP);
  }
  for (uint64_t i = 1; den && i + 1 < dl; i++) mid |= den[i];
  DivClass c{0, !big, !mid};
  c.path = divide_path(den, dl, nl, any != 0, c.canonical_den, c.binom);
  return c;
}
int plk_poly_divide_classify(const uint8_t* den, uint64_t dl, uint64_t nl) { return divide_classify(den, dl, nl).path; }

static unsigned chunk_blocks(uint64_t bytes) {
  const uint64_t b = (((bytes + 15) >> 4) + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// The Newton path's launches (d_den: the divisor's device copy, enqueued before): 2 glue kernels,
// 3 launches per doubling step (two products and the negation), the two closing products with
// their reversal / subtraction.  div_finish_kernel follows (trims; the loop when flagged).
static int newton_divide(const uint8_t* d_num, uint64_t nl, const uint8_t* d_den, uint64_t dl, uint8_t* d_q,
                         uint8_t* d_rem, uint32_t* flag, uint8_t* w, hipStream_t st) {
  const NewtonPlan p = newton_plan(nl, dl);
  uint8_t *G = w + p.o_g, *AR = w + p.o_ar, *F = w + p.o_f, *P = w + p.o_p, *E = w + p.o_e;
  void* mw = w + p.o_mw;
  int rc;
  // a[0, k) = rev(num)[0, k) (checked), f[0, fl) = rev(den)[0, fl)
  RevJobs J{{{d_num + p.m, AR, p.k, 1}, {d_den + (dl - p.fl), F, p.fl, 0}}, flag};
  hipLaunchKernelGGL(div_reverse_kernel, dim3(chunk_blocks(p.k), 2), dim3(256), 0, st, J);
  PLK_HIP(hipGetLastError());
  hipLaunchKernelGGL(div_base_inverse_kernel, dim3(1), dim3(INV_B0), 0, st, F, (uint32_t)(p.fl < INV_B0 ? p.fl : INV_B0),
                     (uint32_t)p.B, G);
  PLK_HIP(hipGetLastError());
  for (uint64_t t = p.B; t < p.k;) {
    const uint64_t n2 = 2 * t < p.k ? 2 * t : p.k, fl2 = p.fl < n2 ? p.fl : n2;
    if ((rc = plk_poly_mul_launch(F, fl2, G, t, P, nullptr, mw, st))) return rc;
    hipLaunchKernelGGL(div_newton_neg_kernel, dim3(chunk_blocks(n2 - t)), dim3(256), 0, st, P, fl2 + t - 1, t, E, n2 - t);
    PLK_HIP(hipGetLastError());
    if ((rc = plk_poly_mul_launch(G, t, E, n2 - t, G + t, nullptr, mw, st))) return rc;
    t = n2;
  }
  // rev(q) = (a g)[0, k)
  if ((rc = plk_poly_mul_launch(AR, p.k, G, p.k, P, nullptr, mw, st))) return rc;
  RevJobs Q{{{P, d_q, p.k, 0}, {nullptr, nullptr, 0, 0}}, flag};
  hipLaunchKernelGGL(div_reverse_kernel, dim3(chunk_blocks(p.k), 1), dim3(256), 0, st, Q);
  PLK_HIP(hipGetLastError());
  // rem = num - (q[0, min(k, m)) den[0, m))[0, m)
  if ((rc = plk_poly_mul_launch(d_q, p.k < p.m ? p.k : p.m, d_den, p.m, P, nullptr, mw, st))) return rc;
  hipLaunchKernelGGL(div_rem_sub_kernel, dim3(chunk_blocks(p.m)), dim3(256), 0, st, d_num, P, p.m, d_rem, flag);
  PLK_HIP(hipGetLastError());
  return PLK_OK;
}

// Classifies the divisor on the host (den is a host array; the kernels get its bytes by value or
// in d_work), enqueues the division; d_lens[0] / d_lens[1] receive the index + 1 of the last
// non-zero quotient / remainder byte (0 if none) over the untrimmed lengths
// ql = nl >= dl ? nl - dl + 1 : 1 and rl = min(dl - 1, nl).
int plk_poly_divide_launch(const uint8_t* d_num, uint64_t nl, const uint8_t* den, uint64_t dl, uint8_t* d_q,
                           uint8_t* d_rem, uint32_t* d_lens, void* d_work, hipStream_t st) {
  const DivClass cls = divide_classify(den, dl, nl);
  const int path = cls.path;
  if (path < 0) return -path;
  const uint32_t lead = den[dl - 1];
  if (nl && !d_num) {
    plk_set_error("poly_divide: NULL numerator");
    return PLK_ERR_ARG;
  }
  const uint64_t m = dl - 1;
  const uint64_t ql = nl >= dl ? nl - dl + 1 : 1;
  const uint64_t rl = m < nl ? m : nl;
  uint8_t* w = (uint8_t*)d_work;
  uint32_t* flag = (uint32_t*)w;           // [0] non-canonical flag
  uint8_t* d_den = w + 256;
  uint32_t* bsum = (uint32_t*)(w + 256 + ((dl + 15) & ~15ull));
  uint8_t* scratch = w + divide_base_bytes(nl, dl) - ((nl + 15) & ~15ull);   // the base part's last nl bytes
  PLK_HIP(hipMemsetAsync(flag, 0, 16, st));
  const bool canonical_den = cls.canonical_den, binom = cls.binom;
  const uint32_t inv = [](uint32_t a) {
    static const uint8_t t[17] = {0, 1, 9, 6, 13, 7, 3, 5, 15, 2, 12, 14, 10, 4, 11, 8, 16};
    return (uint32_t)t[a];
  }(lead);
  const bool newton = path == 4;
  const bool serial = (!canonical_den || !binom || lead == 0) && !newton;
  if (newton) {
    PLK_HIP(hipMemcpyAsync(d_den, den, dl, hipMemcpyHostToDevice, st));
    const int rc = newton_divide(d_num, nl, d_den, dl, d_q, d_rem, flag, w, st);
    if (rc) return rc;
  } else if (!serial) {
    if (nl < dl) {
      // no loop step: q = {0}, rem = num[0 .. rl) -- parallel path still checks num's bytes
      PLK_HIP(hipMemsetAsync(d_q, 0, 1, st));
      if (rl) PLK_HIP(hipMemcpyAsync(d_rem, d_num, rl, hipMemcpyDeviceToDevice, st));
    } else if (m == 0) {
      const uint64_t b = (nl + 255) / 256;
      hipLaunchKernelGGL(div_const_kernel, dim3((unsigned)(b > 8192 ? 8192 : b)), dim3(256), 0, st, d_num, nl, inv, d_q);
      PLK_HIP(hipGetLastError());
    } else {
      Binom B{d_num, nl, m, nl - m, inv, den[0], d_q, d_rem, flag};
      const uint64_t lq = nl - m;
      const uint64_t chains = m < lq ? m : lq;
      const uint64_t len = (lq + m - 1) / m;   // longest chain
      if (len <= 4096) {
        const uint64_t b = (m + 255) / 256;
        hipLaunchKernelGGL(div_binom_short_kernel, dim3((unsigned)b), dim3(256), 0, st, B);
        PLK_HIP(hipGetLastError());
      } else {
        const uint64_t nblk = (len + SCAN_B - 1) / SCAN_B;
        for (uint64_t y0 = 0; y0 < chains; y0 += 65535) {
          const uint64_t ny = chains - y0 < 65535 ? chains - y0 : 65535;
          hipLaunchKernelGGL(div_binom_sums_kernel, dim3((unsigned)nblk, (unsigned)ny), dim3(SCAN_T), 0, st, B, y0,
                             nblk, bsum + y0 * nblk);
          PLK_HIP(hipGetLastError());
          hipLaunchKernelGGL(div_binom_apply_kernel, dim3((unsigned)nblk, (unsigned)ny), dim3(SCAN_T), 0, st, B,
                             y0, nblk, bsum + y0 * nblk);
          PLK_HIP(hipGetLastError());
        }
      }
    }
  }
  // a divisor outside the parallel forms, or (binomial path) non-canonical numerator bytes: the
  // reference's loop.  (m = 0 and nl < dl are exact for any bytes: hf_mul reduces, copies copy.)
  // (Newton path: gated the same way, the loop reading the divisor's device copy)
  const bool gated = !serial && nl >= dl && m > 0;
  if (serial) PLK_HIP(hipMemcpyAsync(d_den, den, dl, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(div_finish_kernel, dim3(1), dim3(1024), 0, st, d_num, nl, serial || newton ? d_den : nullptr, dl,
                     (uint32_t)den[0], lead, d_q, ql, d_rem, rl, serial ? 1 : (gated ? 2 : 0), flag, scratch, d_lens);
  PLK_HIP(hipGetLastError());
  return PLK_OK;
}

int plk_matrix_mul_launch(const uint8_t* d_a, uint64_t m, uint64_t k, const uint8_t* d_b, uint64_t n, uint8_t* d_out,
                          hipStream_t st) {
  const uint64_t e = m * n;
  if (!e) return PLK_OK;
  const uint64_t b = (e + 255) / 256;
  hipLaunchKernelGGL(matrix_mul_kernel, dim3((unsigned)(b > 4096 ? 4096 : b)), dim3(256), 0, st, d_a, d_b, m, k, n,
                     d_out);
  PLK_HIP(hipGetLastError());
  return PLK_OK;
}

int plk_matrix_inv_launch(const uint8_t* d_mat, uint64_t n, uint8_t* d_aug, uint8_t* d_out, hipStream_t st) {
  if (n > 1024) {
    plk_set_error("matrix_inv: n = %llu (max 1024)", (unsigned long long)n);
    return PLK_ERR_RANGE;
  }
  if (!n) return PLK_OK;
  hipLaunchKernelGGL(matrix_inv_kernel, dim3(1), dim3(256), 0, st, d_mat, n, d_aug, d_out);
  PLK_HIP(hipGetLastError());
  return PLK_OK;
}
