// Batched device products by short operands (include/plonkhip.h, "products by short operands"): the
// reference's poly_mul (src/poly.h:106-122) for min(la, lb) <= PLK_MUL_SHORT_MAX as a schoolbook
// convolution over packed bytes, whole runs of equal-shape products in one launch.  DESIGN section 16 has
// the geometry and the measurements.
//
//   Unit      A tile of MS_U = 1024 consecutive output coefficients of one product, computed by ONE wave:
//             a lane owns MS_E = 16 consecutive outputs.  A block is four waves, four units; the units of a
//             launch are numbered run by run, product by product, a product's tiles from the top down (so
//             the tile that settles the trimmed length runs first).  A wave finds its run by scanning the
//             launch's by-value prefix sums, then one division by the units per product.
//   Operands  s = the shorter operand (a when la == lb), ls coefficients, l = the longer one.  With
//             r[j] = s[ls - 1 - j] and the window win[p] = l[k0 - (ls - 1) + p] (zero outside l, and not
//             read there), output k0 + t is sum_j r[j] win[t + j]: a correlation.
//   Tables    Output t = 4 Q + m reads the window from the dword boundary 4 Q with r shifted up by m:
//             R_m[i] = r[i - m].  The wave stages the four shifted copies interleaved, rtab[g] = the words
//             {R_0, R_1, R_2, R_3}[4 g .. 4 g + 3], G4 entries (a multiple of 4, zero padded), and the window
//             as dwords.  Per table entry a lane issues 16 v_dot4_u32_u8 (4 window dwords x 4 shifts) against
//             one broadcast 16-byte table read; per four entries one 16-byte read slides its window.
//   Exactness Nothing is reduced on the way in: a term is at most 255 x 255 and a sum has at most 1040
//             terms, < 2^27, so the u32 accumulators hold conv(a, b) exactly for EVERY byte value, and one
//             % 17 per output gives conv(a mod 17, b mod 17) mod 17, which is what the reference's hf_mul /
//             hf_add fold produces.
//   Memory    Operands are read by aligned dwords joined by v_alignbyte, the dwords that straddle an
//             array's end by bytes: no byte outside [a, a + la) and [b, b + lb) is read.  The outputs leave
//             as aligned 16-byte stores cut on the boundaries of the OUTPUT ADDRESS (a lane joins its bytes
//             with the lane's below by one shuffle), the two ends of a tile by bytes: exactly la + lb - 1
//             bytes are written, whatever the pointers' alignment.
//   Barrier   One __syncthreads() between staging and use, executed by every wave of every block: a wave
//             past the launch's last unit skips its loads and stores, never the barrier.
//   d_nz      zeroed by one memset node in front of the launches; a unit reduces its lanes' candidates and
//             issues one atomicMax at the most, and only when a load shows the word smaller.
#include <string.h>

#include <algorithm>
#include <vector>

#include "plk_device.h"
#include "plk_hostcall.h"
#include "plk_internal.h"

namespace {

constexpr int MS_T = 256, MS_E = 16, MS_U = PLK_WAVE * MS_E, MS_WAVES = MS_T / PLK_WAVE;
constexpr int MS_RUNS = PLK_MUL_SHORT_LAUNCH_RUNS;
constexpr int MS_GMAX = (((PLK_MUL_SHORT_MAX + 3 + 3) / 4) + 3) & ~3;   // table entries: ceil((ls + 3) / 4), to a multiple of 4
constexpr int MS_WIN = MS_U / 4 + MS_GMAX;                               // window dwords
constexpr uint64_t MS_MAX_BLOCKS = 1ull << 23;                           // blocks per launch (2^31 threads)
constexpr uint64_t MS_MAX_PRODUCTS = 1ull << 24;                         // products per call
static_assert(PLK_WAVE == 64 && MS_E == 16, "a lane owns four dwords of outputs");
static_assert((uint64_t)255 * 255 * 4 * MS_GMAX < (1ull << 32), "raw bytes accumulate exactly");

struct MsRun {
  const uint8_t* a;
  const uint8_t* b;
  uint8_t* out;
  uint32_t* nz;     // the run's first word (nullptr: not wanted)
  uint64_t a_stride, b_stride, out_stride;
  uint32_t la, lb;
  uint32_t upp;     // units per product
  uint32_t start;   // the run's first unit in the launch
};
struct MsBatch {
  MsRun r[MS_RUNS];
  uint32_t nruns, total;   // total: units of the launch
};
static_assert(sizeof(MsRun) == 72, "launch structure layout");
static_assert(sizeof(MsBatch) <= 3072, "the launch structure travels by value: kernel arguments are 4 KiB at most");

// The four bytes at the 4-byte aligned address q as a word, those outside [lo, hi) zero and not read.
__device__ __forceinline__ uint32_t ms_word(int64_t q, int64_t lo, int64_t hi) {
  if (q >= lo && q + 4 <= hi) return *reinterpret_cast<const uint32_t*>((uintptr_t)q);
  uint32_t w = 0;
  if (q + 4 > lo && q < hi) {
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (q + k >= lo && q + k < hi) w |= (uint32_t) * reinterpret_cast<const uint8_t*>((uintptr_t)(q + k)) << (8 * k);
  }
  return w;
}

__global__ __launch_bounds__(MS_T) void mulshort_kernel(MsBatch B) {
  __shared__ __attribute__((aligned(16))) uint4 rtab[MS_WAVES][MS_GMAX];
  __shared__ __attribute__((aligned(16))) uint32_t win[MS_WAVES][MS_WIN];
  const uint32_t lane = threadIdx.x & (PLK_WAVE - 1);
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / PLK_WAVE));
  const uint32_t u = blockIdx.x * MS_WAVES + wave;
  const bool live = u < B.total;   // (wave-uniform)
  uint32_t G4 = 0, nv = 0, lout = 0, prod = 0;
  int64_t k0 = 0;
  uint32_t rn = 0;
  if (live) {
    while (rn + 1 < B.nruns && u >= B.r[rn + 1].start) rn++;
    rn = (uint32_t)__builtin_amdgcn_readfirstlane((int)rn);
    const MsRun& R = B.r[rn];
    const uint32_t local = u - R.start;
    prod = local / R.upp;
    const uint32_t tile = R.upp - 1 - (local - prod * R.upp);
    const bool a_short = R.la <= R.lb;
    const uint32_t ls = a_short ? R.la : R.lb, ll = a_short ? R.lb : R.la;
    const uint8_t* pa = R.a + (uint64_t)prod * R.a_stride;
    const uint8_t* pb = R.b + (uint64_t)prod * R.b_stride;
    const uint8_t* sp = a_short ? pa : pb;
    const int64_t L = (int64_t)(uintptr_t)(a_short ? pb : pa);   // address of l[0]
    lout = ls + ll - 1;
    k0 = (int64_t)tile * MS_U;
    nv = (uint32_t)min((int64_t)MS_U, (int64_t)lout - k0);   // outputs of this tile, >= 1
    G4 = (((ls + 3 + 3) >> 2) + 3) & ~3u;
    // the shifted tables: entry g from r[4 g - 3 .. 4 g + 3], r[j] = s[ls - 1 - j]
    for (uint32_t g = lane; g < G4; g += PLK_WAVE) {
      uint32_t t[7];
#pragma unroll
      for (int x = 0; x < 7; x++) {
        const int64_t j = (int64_t)4 * g - 3 + x;
        t[x] = j >= 0 && j < (int64_t)ls ? (uint32_t)sp[ls - 1 - (uint32_t)j] : 0u;
      }
      uint32_t w[4];
#pragma unroll
      for (int m = 0; m < 4; m++) w[m] = t[3 - m] | t[4 - m] << 8 | t[5 - m] << 16 | t[6 - m] << 24;
      rtab[wave][g] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    // the window: the dwords the lanes holding outputs read, [0, ceil16(nv) / 4 + G4)
    const uint32_t nd = ((nv + 15) >> 4) * 4 + G4;
    const int64_t X0 = L + k0 - (int64_t)(ls - 1);   // address of window byte 0 (may lie below l)
    const uint32_t m = (uint32_t)X0 & 3u;
    for (uint32_t d = lane; d < nd; d += PLK_WAVE) {
      const int64_t q = X0 - (int64_t)m + 4 * (int64_t)d;
      const uint32_t w0 = ms_word(q, L, L + (int64_t)ll);
      const uint32_t w1 = m ? ms_word(q + 4, L, L + (int64_t)ll) : 0u;
      win[wave][d] = __builtin_amdgcn_alignbyte(w1, w0, m);
    }
  }
  __syncthreads();   // every wave of the block, live or not
  if (!live) return;
  const MsRun& R = B.r[rn];
  uint32_t o[4] = {0, 0, 0, 0};
  if (lane * MS_E < nv) {
    uint32_t acc[MS_E];
#pragma unroll
    for (int e = 0; e < MS_E; e++) acc[e] = 0;
    const uint4* wv = reinterpret_cast<const uint4*>(&win[wave][0]) + lane;   // dwords 4 lane + ...
    uint4 c = wv[0];
    uint32_t W[8] = {c.x, c.y, c.z, c.w, 0, 0, 0, 0};
    for (uint32_t g0 = 0; g0 < G4; g0 += 4) {   // (uniform)
      c = wv[(g0 >> 2) + 1];
      W[4] = c.x; W[5] = c.y; W[6] = c.z; W[7] = c.w;
#pragma unroll
      for (int gg = 0; gg < 4; gg++) {
        const uint4 rr = rtab[wave][g0 + gg];
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const uint32_t x = W[q + gg];
          acc[4 * q + 0] = __builtin_amdgcn_udot4(x, rr.x, acc[4 * q + 0], false);
          acc[4 * q + 1] = __builtin_amdgcn_udot4(x, rr.y, acc[4 * q + 1], false);
          acc[4 * q + 2] = __builtin_amdgcn_udot4(x, rr.z, acc[4 * q + 2], false);
          acc[4 * q + 3] = __builtin_amdgcn_udot4(x, rr.w, acc[4 * q + 3], false);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; q++) W[q] = W[q + 4];
    }
#pragma unroll
    for (int e = 0; e < MS_E; e++) o[e >> 2] |= (acc[e] % 17u) << (8 * (e & 3));
  }
  // (outputs past la + lb - 1 read only window bytes above l: they are zero)
  // Stores: the tile's bytes [0, nv) go to dst; address group g = lane covers tile bytes [16 g - qo, 16 g -
  // qo + 16), qo = dst & 15: the last qo bytes of the lane below and the first 16 - qo of this lane.
  uint8_t* dst = R.out + (uint64_t)prod * R.out_stride + k0;
  const uint32_t qo = (uint32_t)((uintptr_t)dst & 15u);
  uint32_t cw[12];
  const int below = (int)((lane + PLK_WAVE - 1) & (PLK_WAVE - 1));   // (lane 0: lane 63, for the group past the tile)
#pragma unroll
  for (int x = 0; x < 4; x++) {
    cw[x] = (uint32_t)__shfl((int)o[x], below, PLK_WAVE);
    cw[4 + x] = o[x];
    cw[8 + x] = 0;
  }
  const uint32_t sb = 16u - qo, sw = sb >> 2, sr = sb & 3u;   // the group starts at byte sb of cw: 1 .. 16
  if (sw & 4u) {
#pragma unroll
    for (int x = 0; x < 8; x++) cw[x] = cw[x + 4];
  }
  if (sw & 2u) {
#pragma unroll
    for (int x = 0; x < 8; x++) cw[x] = cw[x + 2];
  }
  if (sw & 1u) {
#pragma unroll
    for (int x = 0; x < 8; x++) cw[x] = cw[x + 1];
  }
  uint32_t gw[4];
#pragma unroll
  for (int x = 0; x < 4; x++) gw[x] = __builtin_amdgcn_alignbyte(cw[x + 1], cw[x], sr);
  const int64_t tb0 = (int64_t)lane * 16 - (int64_t)qo;   // the group's first tile byte
  if (tb0 >= 0 && tb0 + 16 <= (int64_t)nv) {
    *reinterpret_cast<uint4*>(dst + tb0) = make_uint4(gw[0], gw[1], gw[2], gw[3]);
  } else if (tb0 < (int64_t)nv) {
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const int64_t tb = tb0 + k;
      if (tb >= 0 && tb < (int64_t)nv) dst[tb] = (uint8_t)(gw[k >> 2] >> (8 * (k & 3)));
    }
  }
  if (lane == 0 && qo && (int64_t)MS_U - (int64_t)qo < (int64_t)nv) {
    // the group past lane 63's: its first qo bytes are lane 63's last, which lane 0 holds in gw's first qo
    // bytes
#pragma unroll
    for (int k = 0; k < 15; k++) {
      const int64_t tb = (int64_t)MS_U - (int64_t)qo + k;
      if ((uint32_t)k < qo && tb < (int64_t)nv) dst[tb] = (uint8_t)(gw[k >> 2] >> (8 * (k & 3)));
    }
  }
  if (!R.nz) return;   // (uniform)
  uint32_t top = 0;     // index + 1 of the lane's last non-zero output
  {
    const uint32_t hiw = o[3] ? 3u : o[2] ? 2u : o[1] ? 1u : 0u;
    const uint32_t x = o[3] ? o[3] : o[2] ? o[2] : o[1] ? o[1] : o[0];
    if (x) top = (uint32_t)k0 + lane * MS_E + 4 * hiw + ((31 - __clz((int)x)) >> 3) + 1;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) top = max(top, (uint32_t)__shfl_xor((int)top, off, PLK_WAVE));
  if (lane == 0 && top) {
    uint32_t* word = R.nz + prod;
    if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < top) atomicMax(word, top);
  }
}

uint64_t units_of(uint64_t la, uint64_t lb) { return (la + lb - 1 + MS_U - 1) / MS_U; }

// the errors of one shape (no device is touched); count = 0 is the caller's to refuse
int check_shape(const char* fn, int r, uint64_t la, uint64_t lb, uint64_t count) {
  if (la == 0 || lb == 0 || count == 0) {
    plk_set_error("%s: run %d: la >= 1, lb >= 1 and count >= 1 are required", fn, r);
    return PLK_ERR_ARG;
  }
  if (std::min(la, lb) > PLK_MUL_SHORT_MAX) {
    plk_set_error("%s: run %d: both operands have more than %d coefficients", fn, r, PLK_MUL_SHORT_MAX);
    return PLK_ERR_RANGE;
  }
  if (std::max(la, lb) >= (1ull << 32) || la + lb - 1 >= (1ull << 32)) {
    plk_set_error("%s: run %d: a product of 2^32 coefficients or more", fn, r);
    return PLK_ERR_RANGE;
  }
  if (count > MS_MAX_PRODUCTS) {
    plk_set_error("%s: more than 2^24 products in one call", fn);
    return PLK_ERR_RANGE;
  }
  if ((count * units_of(la, lb) + MS_WAVES - 1) / MS_WAVES > MS_MAX_BLOCKS) {
    plk_set_error("%s: run %d: %llu products of %llu coefficients need more blocks than a grid holds", fn, r,
                  (unsigned long long)count, (unsigned long long)(la + lb - 1));
    return PLK_ERR_RANGE;
  }
  return PLK_OK;
}

int check_runs(const char* fn, const plk_mulshort_run_t* runs, int n) {
  if (!runs || n <= 0) {
    plk_set_error("%s: runs and n > 0 are required", fn);
    return PLK_ERR_ARG;
  }
  uint64_t products = 0;
  for (int r = 0; r < n; r++) {
    const plk_mulshort_run_t& S = runs[r];
    if (!S.a || !S.b || !S.out) {
      plk_set_error("%s: run %d: a, b and out are required", fn, r);
      return PLK_ERR_ARG;
    }
    const int rc = check_shape(fn, r, S.la, S.lb, S.count);
    if (rc) return rc;
    if (S.count > 1 && S.out_stride < S.la + S.lb - 1) {
      plk_set_error("%s: run %d: out_stride %zu is smaller than the %zu bytes of a product", fn, r, S.out_stride,
                    S.la + S.lb - 1);
      return PLK_ERR_ARG;
    }
    products += S.count;
    if (products > MS_MAX_PRODUCTS) {
      plk_set_error("%s: more than 2^24 products in one call", fn);
      return PLK_ERR_RANGE;
    }
  }
  return PLK_OK;
}

// the launches of a call: one memset node for the words, then MS_RUNS whole runs per launch (fewer when
// their blocks would not fit one grid), consecutive on the stream
int launch_runs(const plk_mulshort_run_t* runs, int n, uint32_t* d_nz, hipStream_t st) {
  if (d_nz) {
    uint64_t products = 0;
    for (int r = 0; r < n; r++) products += runs[r].count;
    PLK_HIP(hipMemsetAsync(d_nz, 0, (size_t)products * sizeof(uint32_t), st));
  }
  uint64_t first = 0;   // products in front of run r
  int r = 0;
  while (r < n) {
    MsBatch B;
    memset(&B, 0, sizeof B);
    uint64_t total = 0;
    int nr = 0;
    for (; r < n && nr < MS_RUNS; r++, nr++) {
      const plk_mulshort_run_t& S = runs[r];
      const uint64_t units = (uint64_t)S.count * units_of(S.la, S.lb);
      if (nr && (total + units + MS_WAVES - 1) / MS_WAVES > MS_MAX_BLOCKS) break;
      MsRun& D = B.r[nr];
      D.a = S.a;
      D.b = S.b;
      D.out = S.out;
      D.nz = d_nz ? d_nz + first : nullptr;
      D.a_stride = S.a_stride;
      D.b_stride = S.b_stride;
      D.out_stride = S.out_stride;
      D.la = (uint32_t)S.la;
      D.lb = (uint32_t)S.lb;
      D.upp = (uint32_t)units_of(S.la, S.lb);
      D.start = (uint32_t)total;
      total += units;
      first += S.count;
    }
    B.nruns = (uint32_t)nr;
    B.total = (uint32_t)total;
    hipLaunchKernelGGL(mulshort_kernel, dim3((uint32_t)((total + MS_WAVES - 1) / MS_WAVES)), dim3(MS_T), 0, st, B);
    PLK_HIP(hipGetLastError());
  }
  return PLK_OK;
}

}  // namespace

extern "C" {

int plk_poly_mul_short_plan(size_t la, size_t lb, size_t count, int64_t out[4]) {
  const char* fn = "plk_poly_mul_short_plan";
  if (!out) {
    plk_set_error("%s: out is required", fn);
    return PLK_ERR_ARG;
  }
  const int rc = check_shape(fn, 0, la, lb, count);
  if (rc) return rc;
  const uint64_t upp = units_of(la, lb);
  out[0] = MS_U;
  out[1] = (int64_t)upp;
  out[2] = MS_WAVES;
  out[3] = (int64_t)(((uint64_t)count * upp + MS_WAVES - 1) / MS_WAVES);
  return PLK_OK;
}

int plk_poly_mul_short_batch_dev(const plk_mulshort_run_t* runs, int n, uint32_t* d_nz, void* stream) {
  int rc = check_runs("plk_poly_mul_short_batch_dev", runs, n);
  if (rc || (rc = plk_use_device())) return rc;
  return launch_runs(runs, n, d_nz, (hipStream_t)stream);
}

int plk_poly_mul_short_batch(const plk_mulshort_run_t* runs, int n, size_t* out_lens) {
  const char* fn = "plk_poly_mul_short_batch";
  int rc = check_runs(fn, runs, n);
  if (rc) return rc;
  // one allocation: the words, then per run the bytes its operands span and its products packed tight
  std::vector<plk_mulshort_run_t> dr(runs, runs + n);
  std::vector<size_t> o_a((size_t)n), o_b((size_t)n), o_out((size_t)n), sa((size_t)n), sb((size_t)n);
  size_t products = 0;
  for (int r = 0; r < n; r++) products += runs[r].count;
  size_t total = plk_pad16(products * sizeof(uint32_t));
  for (int r = 0; r < n; r++) {
    const plk_mulshort_run_t& S = runs[r];
    size_t so = 0;
    if (!plk_span_of(S.la, S.a_stride, S.count, &sa[r]) || !plk_span_of(S.lb, S.b_stride, S.count, &sb[r]) ||
        !plk_span_of(S.la + S.lb - 1, S.la + S.lb - 1, S.count, &so)) {
      plk_set_error("%s: run %d: the strides overflow the address space", fn, r);
      return PLK_ERR_RANGE;
    }
    o_a[r] = total;
    total += plk_pad16(sa[r]);
    o_b[r] = total;
    total += plk_pad16(sb[r]);
    o_out[r] = total;
    total += plk_pad16(so);
  }
  if ((rc = plk_select_device())) return rc;
  PlkScratch S;
  if ((rc = S.alloc(fn, total))) return rc;
  for (int r = 0; r < n; r++) {
    PLK_HIP(hipMemcpy(S.d + o_a[r], runs[r].a, sa[r], hipMemcpyHostToDevice));
    PLK_HIP(hipMemcpy(S.d + o_b[r], runs[r].b, sb[r], hipMemcpyHostToDevice));
    dr[r].a = S.d + o_a[r];
    dr[r].b = S.d + o_b[r];
    dr[r].out = S.d + o_out[r];
    dr[r].out_stride = runs[r].la + runs[r].lb - 1;
  }
  if ((rc = launch_runs(dr.data(), n, (uint32_t*)S.d, nullptr))) return rc;
  for (int r = 0; r < n; r++) {   // the products alone: the bytes between them stay as they are
    const size_t lo = runs[r].la + runs[r].lb - 1;
    if (runs[r].count == 1)
      PLK_HIP(hipMemcpy(runs[r].out, S.d + o_out[r], lo, hipMemcpyDeviceToHost));
    else
      PLK_HIP(hipMemcpy2D(runs[r].out, runs[r].out_stride, S.d + o_out[r], lo, lo, runs[r].count, hipMemcpyDeviceToHost));
  }
  if (out_lens) {
    std::vector<uint32_t> nz(products);
    PLK_HIP(hipMemcpy(nz.data(), S.d, products * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < products; i++) out_lens[i] = nz[i] ? nz[i] : 1;
  }
  return PLK_OK;
}

}  // extern "C"
