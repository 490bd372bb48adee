// GF(17) byte primitives shared by the device code of the polynomial, KZG and prover files.
// One definition of each: a feature file includes this header and defines none of them again.
// Everything is __forceinline__, so a kernel's code does not depend on which file it sits in.
// (Not for msm.hip or the headers it includes: bench.py hashes those.)
#pragma once
#include "plk_device.h"

namespace hf17 {

constexpr uint32_t P = 17;

// x mod 17 for x < 69632 by 24-bit multiplies (full rate; `% 17` on a u32 takes a quarter-rate
// multiply-high): 61681 = (2^20 + 1) / 17, so floor(x 61681 / 2^20) = floor(x / 17) for x < 2^20,
// and x 61681 < 2^32 (the static_asserts below walk every x < 69632).  Every call site's bound is noted.
constexpr uint32_t MOD17_BOUND = 69632;
constexpr uint32_t mod17_model(uint32_t x) { return x - 17u * ((x * 61681u) >> 20); }
constexpr bool mod17_exact(uint32_t lo, uint32_t hi) {
  for (uint32_t x = lo; x < hi; x++)
    if (mod17_model(x) != x % 17u || (uint64_t)x * 61681u >= (1ull << 32)) return false;
  return true;
}
static_assert(mod17_exact(0, MOD17_BOUND), "mod17 is exact and its product fits 32 bits for every x < 69632");
static_assert((uint64_t)MOD17_BOUND * 61681u >= (1ull << 32), "69632 is the first x whose product leaves 32 bits");
__device__ __forceinline__ uint32_t mod17(uint32_t x) { return x - 17u * (__umul24(x, 61681u) >> 20); }

__device__ __forceinline__ uint32_t neg(uint32_t a) { return a ? P - a : 0; }
// Two powers: pow reduces any b and takes any exponent; pow_canon (b < 17, e < 128; 0^0 = 1 as
// hf_pow) is the batched prover's fixed seven mod17 steps.  They compile differently, so both stay.
__device__ __forceinline__ uint32_t pow(uint32_t b, uint64_t e) {
  uint32_t r = 1;
  b %= P;
  while (e) {
    if (e & 1) r = r * b % P;
    b = b * b % P;
    e >>= 1;
  }
  return r;
}
__device__ __forceinline__ uint32_t pow_canon(uint32_t b, uint32_t e) {
  uint32_t r = 1;
  for (int k = 0; k < 7; k++) {
    if (e & 1u) r = mod17(r * b);
    b = mod17(b * b);
    e >>= 1;
  }
  return r;
}
// inv(0) = 0 (hf.h LUT)
__device__ __forceinline__ uint32_t inv(uint32_t a) { return pow(a, P - 2); }
__device__ __forceinline__ uint32_t inv_canon(uint32_t a) { return pow_canon(a, P - 2); }

// the reference's raw byte ops (src/hf.h:79-119): a uint8 sum with one conditional subtract, an
// int8 difference with one conditional add, (a * b) % 17 on whatever bytes come in
__device__ __forceinline__ uint32_t add8(uint32_t a, uint32_t b) {
  uint32_t s = (a + b) & 0xFFu;
  if (s >= P) s -= P;
  return s;
}
__device__ __forceinline__ uint32_t sub8(uint32_t a, uint32_t b) {
  int8_t d = (int8_t)((int)(int8_t)a - (int)(int8_t)b);
  if (d < 0) d = (int8_t)(d + (int)P);
  return (uint8_t)d;
}
// the same value from int temporaries: lincomb.hip's slow path compiles differently with sub8
// (and polyops.hip's serial loops with this one), so both forms stay
__device__ __forceinline__ uint32_t sub8_wide(uint32_t a, uint32_t b) {
  int d = (int)(int8_t)((int)(int8_t)a - (int)(int8_t)b);
  if (d < 0) d = (int)(int8_t)(d + (int)P);
  return (uint32_t)d & 0xFFu;
}
__device__ __forceinline__ uint32_t neg8(uint32_t a) { return a == 0 ? 0u : (P - a) & 0xFFu; }
__device__ __forceinline__ uint32_t mul8(uint32_t a, uint32_t b) { return a * b % P; }

// non-zero when some byte of w is >= 17 (additions and masks only: no products).  A byte b < 128
// has b + 0x6F >= 0x80 exactly when b >= 17, without a carry into the next byte; a byte >= 128
// keeps its own top bit.
__device__ __forceinline__ uint32_t top_bits4(uint32_t w) { return ((w & 0x7F7F7F7Fu) + 0x6F6F6F6Fu) | w; }
__device__ __forceinline__ uint32_t noncanonical4(uint32_t w) { return top_bits4(w) & 0x80808080u; }
// some byte of the four words is >= 17, four bytes at a time
__device__ __forceinline__ bool any_noncanonical(const uint32_t (&w)[4]) {
  uint32_t m = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) m |= top_bits4(w[i]);
  return (m & 0x80808080u) != 0;
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t (&w)[4], int k) { return (w[k >> 2] >> (8 * (k & 3))) & 0xFFu; }

// pw[j] = a^j mod 17, j < 16
__device__ __forceinline__ void pow16(uint32_t a, uint32_t (&pw)[16]) {
  pw[0] = 1;
#pragma unroll
  for (int j = 1; j < 16; j++) pw[j] = pw[j - 1] * a % P;
}

// inclusive suffix sum over the wave: lane l gets the sum over lanes l .. 63
__device__ __forceinline__ uint32_t wave_suffix(uint32_t x) {
  const int lane = (int)(threadIdx.x & (PLK_WAVE - 1));
#pragma unroll
  for (int d = 1; d < PLK_WAVE; d <<= 1) {
    const uint32_t v = __shfl_down(x, d, PLK_WAVE);
    if (lane + d < PLK_WAVE) x += v;
  }
  return x;
}

// bytes [i, i + 16) of p[0, len) as four words, zero past len; vec: p 16-byte aligned (i is)
__device__ __forceinline__ void load16(const uint8_t* p, uint64_t len, uint64_t i, bool vec, uint32_t (&w)[4]) {
  if (vec && i + 16 <= len) {
    const uint4 v = *reinterpret_cast<const uint4*>(p + i);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    return;
  }
  w[0] = w[1] = w[2] = w[3] = 0;
#pragma unroll
  for (int k = 0; k < 16; k++)
    if (i + k < len) w[k >> 2] |= (uint32_t)p[i + k] << (8 * (k & 3));
}

}  // namespace hf17
