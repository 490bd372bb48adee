// The raw G1 formulas, the pairing and the host scaffold shared by the verification files
// (pairing.hip: one lane per job; kzg_agg.hip: one verdict per group of jobs).  One definition of
// each: a feature file includes this header and defines none of them again.  Everything on the
// device side is __forceinline__, so a kernel's code does not depend on which file it sits in.
// (Not for msm.hip or the headers it includes: bench.py hashes those.)
//
// The raw G1 formulas are restated here after RawOps of msm.hip (which stays untouched); every
// select is branch-free so the lanes of a wave do not diverge on the encodings they hold.  The
// inverse table (inv(0) = 0, gf_inv is v^99) is indexed per lane, so it lives in LDS; each block
// computes it itself, one power per thread, which keeps the entry points free of any table upload.
#pragma once
#include "plk_hf17.h"
#include "plk_hostcall.h"
#include "plk_internal.h"

namespace plkpair {

constexpr uint32_t GFP = 101, HFP = hf17::P;
constexpr int PAIR_T = 256;
constexpr size_t PAIR_MAX_N = (size_t)1 << 30;

struct Pt { uint32_t x, y, inf; };
struct Gt { uint32_t a, b; };
struct VkWords { uint32_t gx, gy, ginf, h1x, h1y, hsx, hsy; };

// v mod 101 for v < 33554: 41529 = ceil(2^22 / 101), 101 * 41529 - 2^22 = 125 and 2^22 / 125 > 33554
__device__ __forceinline__ uint32_t red(uint32_t v) { return v - GFP * ((v * 41529u) >> 22); }
__device__ __forceinline__ uint32_t sub(uint32_t a, uint32_t b) { const uint32_t d = a + GFP - b; return d >= GFP ? d - GFP : d; }
__device__ __forceinline__ uint32_t neg(uint32_t a) { return a ? GFP - a : 0u; }

// the block's inverse table: thread v computes v^99
__device__ __forceinline__ void stage_inverses(uint32_t* invl) {
  for (uint32_t v = threadIdx.x; v < GFP; v += PAIR_T) {
    uint32_t r = 1, b = v;
#pragma unroll
    for (uint32_t e = GFP - 2; e; e >>= 1) {
      if (e & 1u) r = red(r * b);
      b = red(b * b);
    }
    invl[v] = r;
  }
  __syncthreads();
}

struct G1Ops {
  const uint32_t* inv;   // LDS
  // g1_double (src/g1.h:37-56); the formula runs for every lane (inv(0) = 0) and the identity is selected after
  __device__ __forceinline__ Pt dbl(Pt a) const {
    const uint32_t two_y = a.y + a.y;
    const uint32_t m = red(red(3u * a.x * a.x) * inv[two_y >= GFP ? two_y - GFP : two_y]);
    const uint32_t m2 = red(m * m);
    const uint32_t xr = red(m2 + 2u * GFP - 2u * a.x);
    const uint32_t yr = red(m * red(3u * a.x + GFP - m2) + GFP - a.y);
    const bool id = a.inf || a.y == 0;
    return Pt{id ? 0u : xr, id ? 0u : yr, id ? 1u : 0u};
  }
  // g1_add (src/g1.h:59-83)
  __device__ __forceinline__ Pt add(Pt a, Pt b) const {
    const uint32_t m = red((b.y + GFP - a.y) * inv[sub(b.x, a.x)]);
    const uint32_t xr = red(m * m + 2u * GFP - a.x - b.x);
    const uint32_t yr = red(m * sub(a.x, xr) + GFP - a.y);
    const Pt d = dbl(a);
    Pt r{xr, yr, 0};
    if (a.x == b.x) {
      const uint32_t s = a.y + b.y;
      const bool opposite = s == 0 || s == GFP;
      r = opposite ? Pt{0, 0, 1} : d;
    }
    if (b.inf) r = a;
    if (a.inf) r = b;
    return r;
  }
  // g1_neg (src/g1.h:85-89): a flagged point is returned as it is, coordinates included
  __device__ __forceinline__ Pt negp(Pt a) const { return Pt{a.x, a.inf ? a.y : neg(a.y), a.inf}; }
  // g1_mul (src/g1.h:91-103) for k < 32: a zero bit leaves the sum alone, so five fixed steps
  __device__ __forceinline__ Pt mul(Pt run, uint32_t k) const {
    Pt term{0, 0, 1};
#pragma unroll
    for (int i = 0; i < 5; i++) {
      const Pt t = add(term, run);
      if ((k >> i) & 1u) term = t;
      run = dbl(run);
    }
    return term;
  }
};

// gtp_mul (src/gt.h:23-28): (a + b u)(c + d u), u^2 = -2; 20402 = 2 * 101^2 keeps the difference positive
__device__ __forceinline__ Gt gt_mul(Gt f, Gt g) {
  return Gt{red(f.a * g.a + 20402u - 2u * f.b * g.b), red(f.a * g.b + f.b * g.a)};
}

// line(a, b) (src/pairing.h:19-29) evaluated at q as pairing_f does (src/pairing.h:41-44)
__device__ __forceinline__ Gt line_at(Pt a, Pt b, uint32_t qx, uint32_t qy) {
  const uint32_t m = sub(b.x, a.x), n = sub(b.y, a.y);
  const uint32_t c = red(m * a.y + GFP * GFP - n * a.x);
  return Gt{red(qx * n + c), red(qy * neg(m))};
}

__device__ __forceinline__ Gt pairing(const G1Ops& G, Pt p, uint32_t qx, uint32_t qy) {
  Gt f{1, 0};
  Pt d = p;
#pragma unroll
  for (int k = 0; k < 4; k++) {   // r = 2, 4, 8, 16
    f = gt_mul(gt_mul(f, f), line_at(d, G.dbl(G.negp(d)), qx, qy));
    d = G.dbl(d);
  }
  f = gt_mul(f, line_at(d, p, qx, qy));   // r = 17
  // f^600 = conj(f^5) f^95, 95 = 64 + 16 + 8 + 4 + 2 + 1
  const Gt f2 = gt_mul(f, f), f4 = gt_mul(f2, f2), f8 = gt_mul(f4, f4), f16 = gt_mul(f8, f8), f32 = gt_mul(f16, f16),
           f64 = gt_mul(f32, f32);
  const Gt f5 = gt_mul(f, f4);
  const Gt f95 = gt_mul(gt_mul(gt_mul(f5, f2), gt_mul(f8, f16)), f64);
  return gt_mul(Gt{f5.a, neg(f5.b)}, f95);
}

// a G1 from its three bytes (any alignment: byte loads, nothing read past the array); ok: valid encoding,
// and an invalid one is replaced by the identity so that no formula sees a value >= 101
__device__ __forceinline__ Pt load_g1(const uint8_t* p, bool& ok) {
  const uint32_t x = p[0], y = p[1], f = p[2];
  const bool v = x < GFP && y < GFP && f < 2u;
  ok = ok && v;
  return v ? Pt{x, y, f} : Pt{0, 0, 1};
}

// the checks that come before any device query
inline int check_n(const char* fn, bool null_arg, size_t n) {
  if (null_arg || n == 0) {
    plk_set_error("%s: every pointer and n > 0 are required", fn);
    return PLK_ERR_ARG;
  }
  return PLK_OK;
}
inline int check_range(const char* fn, size_t n) {
  if (n > PAIR_MAX_N) {
    plk_set_error("%s: n = %zu exceeds 2^30 jobs per call", fn, n);
    return PLK_ERR_RANGE;
  }
  return PLK_OK;
}
inline int check_vk(const char* fn, const plk_kzg_vk_t* vk, VkWords* w) {
  if (vk->g1[0] >= GFP || vk->g1[1] >= GFP || vk->g1[2] > 1 || vk->g2_1[0] >= GFP || vk->g2_1[1] >= GFP ||
      vk->g2_s[0] >= GFP || vk->g2_s[1] >= GFP) {
    plk_set_error("%s: the verification key holds an invalid encoding (coordinates < 101, flag 0 or 1)", fn);
    return PLK_ERR_ARG;
  }
  *w = VkWords{vk->g1[0], vk->g1[1], vk->g1[2], vk->g2_1[0], vk->g2_1[1], vk->g2_s[0], vk->g2_s[1]};
  return PLK_OK;
}

// The device arrays of one host form, one after another in the call's one allocation (alloc: the sum of
// their sizes; the masks go first, so their 4-byte alignment costs no padding).  add() appends an array at
// the next multiple of align, uploads it when it has a source and returns its device pointer; rc keeps the
// first failure -- a copy, or an array that would pass the allocation -- and is read once after the last add().
struct __attribute__((visibility("hidden"))) Staged {
  PlkScratch S;
  size_t cap = 0, off = 0;
  int rc = PLK_OK;
  int alloc(const char* fn, size_t bytes) {
    cap = bytes;
    return S.alloc(fn, bytes);
  }
  uint8_t* add(const void* src, size_t bytes, size_t align = 1) {
    off = (off + align - 1) / align * align;
    uint8_t* d = S.d + off;
    off += bytes;
    if (rc == PLK_OK && off > cap) {
      plk_set_error("%s:%d the staged arrays pass the %zu bytes allocated for them", __FILE__, __LINE__, cap);
      rc = PLK_ERR_ARG;
    }
    if (rc == PLK_OK && src && hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) {
      plk_set_error("%s:%d the upload of a staged array failed", __FILE__, __LINE__);
      rc = PLK_ERR_HIP;
    }
    return d;
  }
};

}  // namespace plkpair
