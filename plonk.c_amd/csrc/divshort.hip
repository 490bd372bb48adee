// Batched device division by short divisors (include/plonkhip.h, "division by short divisors"): the
// reference's poly_divide loop (src/poly.h:124-177) for a divisor of degree t = dl - 1 in 1 .. 16 as one
// streaming scan over the numerator.  DESIGN section 15 has the algebra and the measurements.
//
//   Recurrence  Consume a[i] from the top down with a state R in GF(17)^t, the remainder of everything
//               above i:  c = inv R[t-1];  q[i] = c (kept for i < nl - t);  R <- low t coefficients of
//               (R x + a[i]) - c d.  A run of n coefficients acts as R -> R x^n mod d + (run mod d), so
//               runs compose by multiplication by x^n in GF(17)[x]/(d).  Nothing is ever inverted (d_0 = 0
//               makes x a zero divisor) and no period of x is assumed.
//   Buckets     The kernels are compiled for T = 2, 4, 8, 16 states.  A divisor of degree t < T runs as
//               D = d x^s, s = T - t, over the numerator a x^s: the quotient is the same, the remainder is
//               r x^s (read off from state entry s up).  In the shifted ("virtual") index v = i + s the
//               numerator reads as zero below s and above nl + s, and q[v] is coefficient v of the quotient.
//   Geometry    A thread owns DS_E = 32 consecutive virtual indices, a block of 256 threads a chunk of
//               DS_B = 8192; chunks are cut from virtual index 0 up, so every chunk is full (zeros above the
//               top) and every transfer element is x^(DS_E 2^k).  Thread 0 of a block holds the chunk's top.
//   Tables      Multiplication by x^n is a T x T byte matrix (row j = x^(n + j) mod D).  A block's prologue
//               squares the companion matrix in LDS, one entry per thread: log2 n squarings to reach x^n,
//               seven more for the eight levels of a 256-item scan.
//   Phases      aggregates (chunk mod D, T bytes per chunk, chunk 0 excepted), carries (one block per job
//               scans the job's chunk aggregates from the top, 256 at a time, and stores every chunk's
//               incoming state), apply (per-thread aggregates again, a Kogge-Stone scan over the block's
//               threads seeded with the chunk's carry, then each thread walks its bytes from its incoming
//               state, storing quotient bytes; the bottom chunk's last thread holds the remainder).  A group
//               of jobs that all fit one chunk runs the apply kernel alone.  No block waits for another.
//   Memory      A chunk's numerator bytes go through LDS: aligned 16-byte loads inside the array, byte loads
//               at its two ends; the quotient bytes return the same way.  Exactly a[0, nl) is read, exactly
//               the stated output bytes are written, whatever the pointers' alignment.
//   d_lens      zeroed by one memset node in front of the launches; blocks atomicMax the index + 1 of their
//               last non-zero quotient byte, the bottom block that of the remainder, and a block that loaded
//               a numerator byte >= 17 sets the status word.  Sums stay inside mod17's exact range for any
//               byte value, so such a job computes garbage inside its own buffers and nothing else.
#include <string.h>

#include <algorithm>
#include <vector>

#include "plk_device.h"
#include "plk_hf17.h"
#include "plk_hostcall.h"
#include "plk_internal.h"

namespace {

constexpr int DS_T = 256, DS_E = 32, DS_B = DS_T * DS_E;
constexpr int DS_E_LOG = 5, DS_B_LOG = 13;
constexpr int DS_LEVELS = 8;       // scan levels over DS_T items
constexpr int DS_JOBS = PLK_DIV_SHORT_LAUNCH_JOBS;
constexpr int DS_MAX_GRID = 1024;  // blocks per job of the aggregate and apply launches (chunks beyond: grid stride)
constexpr uint32_t HFP = hf17::P;
using hf17::mod17;
static_assert((1 << DS_E_LOG) == DS_E && (1 << DS_B_LOG) == DS_B && (1 << DS_LEVELS) == DS_T, "geometry");

struct DsJob {
  const uint8_t* num;
  uint8_t* quot;
  uint8_t* rem;
  uint32_t* lens;   // three words: quotient length, remainder length, status
  uint8_t* agg;     // nch x 16 bytes: chunk aggregates (written for chunks >= 1)
  uint8_t* carry;   // nch x 16 bytes: chunk c's incoming state (written for chunks < nch - 1)
  uint32_t nl, nch;
  uint8_t D[16];    // d x^s, coefficients 0 .. T - 1 (the lead only through inv)
  uint8_t s, t, inv, pad[5];
};
struct DsBatch {
  DsJob j[DS_JOBS];
};
static_assert(sizeof(DsJob) == 80, "launch structure layout");
static_assert(sizeof(DsBatch) <= 3072, "the launch structure travels by value: kernel arguments are 4 KiB at most");

template <int T>
struct Words {
  static constexpr int W = T < 4 ? 1 : T / 4;
};

template <int T>
__device__ __forceinline__ void ds_pack(const uint32_t (&v)[T], uint32_t (&w)[Words<T>::W]) {
#pragma unroll
  for (int i = 0; i < Words<T>::W; i++) w[i] = 0;
#pragma unroll
  for (int j = 0; j < T; j++) w[j >> 2] |= v[j] << (8 * (j & 3));
}
template <int T>
__device__ __forceinline__ void ds_unpack(const uint32_t (&w)[Words<T>::W], uint32_t (&v)[T]) {
#pragma unroll
  for (int j = 0; j < T; j++) v[j] = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
}

// v <- (u M + v) mod 17: u, v canonical, M a T x T byte matrix in LDS (every lane reads the same words)
template <int T>
__device__ __forceinline__ void ds_mulx(const uint8_t* M, const uint32_t (&u)[T], uint32_t (&v)[T]) {
  const uint32_t* Mw = reinterpret_cast<const uint32_t*>(M);
  uint32_t mw[T * T / 4];
#pragma unroll
  for (int i = 0; i < T * T / 4; i++) mw[i] = Mw[i];
#pragma unroll
  for (int m = 0; m < T; m++) {
    uint32_t acc = v[m];
#pragma unroll
    for (int j = 0; j < T; j++) {
      const int idx = j * T + m;
      acc += u[j] * ((mw[idx >> 2] >> (8 * (idx & 3))) & 0xFFu);
    }
    v[m] = mod17(acc);   // (acc <= 16 + 16 x 16 x 16)
  }
}

// tab[l] = the matrix of multiplication by x^(2^(first + l)) mod D, l < DS_LEVELS: the companion matrix
// (row j = x^(j + 1) mod D) squared first + DS_LEVELS - 1 times, entry (i, m) by thread i T + m.
template <int T>
__device__ void ds_build_tables(const DsJob& J, int first, uint8_t* tab, uint8_t* tmp) {
  constexpr int N = T * T;
  const int tid = threadIdx.x, i = tid / T, m = tid % T;
  if (tid < N) tmp[tid] = (uint8_t)(i < T - 1 ? (m == i + 1 ? 1u : 0u) : (HFP - (uint32_t)J.inv * J.D[m] % HFP) % HFP);
  __syncthreads();
  const uint8_t* src = tmp;
  for (int lvl = 1; lvl < first + DS_LEVELS; lvl++) {   // (uniform)
    uint8_t* dst = lvl >= first ? tab + (lvl - first) * N : tmp + (lvl & 1) * N;
    if (tid < N) {
      uint32_t acc = 0;
#pragma unroll
      for (int l = 0; l < T; l++) acc += (uint32_t)src[i * T + l] * (uint32_t)src[l * T + m];
      dst[tid] = (uint8_t)mod17(acc);
    }
    __syncthreads();
    src = dst;
  }
}

// Inclusive scan over the block's threads, thread 0 first: v_i <- v_0 x^(n i) + ... + v_i with tab[l] =
// x^(n 2^l).  On return sc[tid] holds the packed result of thread tid, visible to the block.
template <int T>
__device__ __forceinline__ void ds_block_scan(uint32_t (&v)[T], const uint8_t* tab, uint32_t* sc) {
  constexpr int W = Words<T>::W;
  const int tid = threadIdx.x;
  uint32_t w[W];
  ds_pack<T>(v, w);
#pragma unroll
  for (int i = 0; i < W; i++) sc[tid * W + i] = w[i];
  for (int lv = 0; lv < DS_LEVELS; lv++) {
    const int d = 1 << lv;
    __syncthreads();
    if (tid >= d) {
#pragma unroll
      for (int i = 0; i < W; i++) w[i] = sc[(tid - d) * W + i];
    }
    __syncthreads();
    if (tid >= d) {
      uint32_t u[T];
      ds_unpack<T>(w, u);
      ds_mulx<T>(tab + lv * T * T, u, v);
      ds_pack<T>(v, w);
#pragma unroll
      for (int i = 0; i < W; i++) sc[tid * W + i] = w[i];
    }
  }
  __syncthreads();
}

// The chunk's numerator bytes [ilo, ihi) into LDS at in[ioff + (i - ilo)], ioff = (num + ilo) & 15: the
// 16-byte groups of the ADDRESS that lie inside the range by one aligned load, the two ends by bytes.
__device__ __forceinline__ void ds_load_chunk(const uint8_t* num, int64_t ilo, int64_t ihi, uint32_t ioff, uint8_t* in) {
  if (ihi <= ilo) return;   // (uniform)
  const uint8_t* A = num + ilo - ioff;
  const uint32_t end = ioff + (uint32_t)(ihi - ilo), ng = (end + 15) >> 4;
  for (uint32_t g = threadIdx.x; g < ng; g += DS_T) {
    if (16 * g >= ioff && 16 * g + 16 <= end) {
      *reinterpret_cast<uint4*>(in + 16 * g) = *reinterpret_cast<const uint4*>(A + 16 * g);
    } else {
      for (uint32_t p = 16 * g; p < 16 * g + 16; p++)
        if (p >= ioff && p < end) in[p] = A[p];
    }
  }
}
__device__ __forceinline__ void ds_store_chunk(uint8_t* quot, int64_t qlo, int64_t qhi, uint32_t qoff, const uint8_t* out) {
  if (qhi <= qlo) return;   // (uniform)
  uint8_t* A = quot + qlo - qoff;
  const uint32_t end = qoff + (uint32_t)(qhi - qlo), ng = (end + 15) >> 4;
  for (uint32_t g = threadIdx.x; g < ng; g += DS_T) {
    if (16 * g >= qoff && 16 * g + 16 <= end) {
      *reinterpret_cast<uint4*>(A + 16 * g) = *reinterpret_cast<const uint4*>(out + 16 * g);
    } else {
      for (uint32_t p = 16 * g; p < 16 * g + 16; p++)
        if (p >= qoff && p < end) A[p] = out[p];
    }
  }
}

// A thread's DS_E steps of the recurrence from virtual index vtop down, S canonical on entry and on exit.
// Between the reductions an entry grows by at most 255 + 17 x 16 a step: < 9000 after 32, inside mod17's
// exact range for any numerator byte.
template <int T, bool OUT>
__device__ __forceinline__ void ds_walk(uint32_t (&S)[T], const uint32_t (&Dr)[T], uint32_t inv, const uint8_t* in,
                                        int64_t vtop, int64_t s, int64_t ilo, int64_t ihi, uint32_t ioff, uint8_t* out,
                                        int64_t qlo, int64_t qhi, uint32_t qoff, uint32_t& top, uint32_t& bad) {
#pragma unroll 8
  for (int e = 0; e < DS_E; e++) {
    const int64_t v = vtop - e, i = v - s;
    const uint32_t a = i >= ilo && i < ihi ? in[ioff + (uint32_t)(i - ilo)] : 0u;
    const uint32_t c = mod17(mod17(S[T - 1]) * inv);
    const uint32_t nc = HFP - c;
#pragma unroll
    for (int j = T - 1; j > 0; j--) S[j] = S[j - 1] + nc * Dr[j];
    S[0] = a + nc * Dr[0];
    if (OUT) {
      bad |= a >= HFP ? 1u : 0u;
      if (v >= qlo && v < qhi) {
        out[qoff + (uint32_t)(v - qlo)] = (uint8_t)c;
        if (c && !top) top = (uint32_t)v + 1;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < T; j++) S[j] = mod17(S[j]);
}

struct DsChunk {
  int64_t v0, ilo, ihi;
  uint32_t ioff;
};
__device__ __forceinline__ DsChunk ds_chunk(const DsJob& J, uint32_t k) {
  DsChunk c;
  c.v0 = (int64_t)k * DS_B;
  c.ilo = max(c.v0 - (int64_t)J.s, (int64_t)0);
  c.ihi = min(c.v0 + DS_B - (int64_t)J.s, (int64_t)J.nl);
  c.ioff = (uint32_t)((uintptr_t)(J.num + c.ilo) & 15u);
  return c;
}

// Phase 1, block (x, job): chunks x, x + gridDim.x, ... of the job, chunk 0 excepted: chunk mod D.
template <int T>
__global__ __launch_bounds__(DS_T) void divshort_agg_kernel(DsBatch B) {
  constexpr int W = Words<T>::W;
  __shared__ __attribute__((aligned(16))) uint8_t in[DS_B + 32];
  __shared__ __attribute__((aligned(16))) uint8_t tab[DS_LEVELS * T * T];
  __shared__ __attribute__((aligned(16))) uint8_t tmp[2 * T * T];
  __shared__ __attribute__((aligned(16))) uint32_t sc[DS_T * W];
  const DsJob& J = B.j[blockIdx.y];
  if (J.nch < 2 || blockIdx.x + 1 >= J.nch) return;   // (uniform)
  ds_build_tables<T>(J, DS_E_LOG, tab, tmp);
  uint32_t Dr[T];
#pragma unroll
  for (int j = 0; j < T; j++) Dr[j] = J.D[j];
  const int tid = threadIdx.x;
  for (uint32_t k = blockIdx.x + 1; k < J.nch; k += gridDim.x) {
    const DsChunk c = ds_chunk(J, k);
    ds_load_chunk(J.num, c.ilo, c.ihi, c.ioff, in);
    __syncthreads();
    uint32_t S[T], top = 0, bad = 0;
#pragma unroll
    for (int j = 0; j < T; j++) S[j] = 0;
    ds_walk<T, false>(S, Dr, J.inv, in, c.v0 + DS_B - 1 - (int64_t)tid * DS_E, J.s, c.ilo, c.ihi, c.ioff, nullptr, 0, 0, 0,
                      top, bad);
    ds_block_scan<T>(S, tab, sc);
    if (tid == DS_T - 1) {
      uint32_t w[4] = {0, 0, 0, 0}, ww[W];
      ds_pack<T>(S, ww);
#pragma unroll
      for (int i = 0; i < W; i++) w[i] = ww[i];
      *reinterpret_cast<uint4*>(J.agg + 16 * (size_t)k) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    __syncthreads();
  }
}

// Phase 2, one block per job: the incoming state of every chunk below the top one.  Item i is chunk
// nch - 1 - i; 256 items a round, the running state folded into the round's first item.
template <int T>
__global__ __launch_bounds__(DS_T) void divshort_carry_kernel(DsBatch B) {
  constexpr int W = Words<T>::W;
  __shared__ __attribute__((aligned(16))) uint8_t tab[DS_LEVELS * T * T];
  __shared__ __attribute__((aligned(16))) uint8_t tmp[2 * T * T];
  __shared__ __attribute__((aligned(16))) uint32_t sc[DS_T * W];
  const DsJob& J = B.j[blockIdx.x];
  if (J.nch < 2) return;   // (uniform)
  ds_build_tables<T>(J, DS_B_LOG, tab, tmp);
  const int tid = threadIdx.x;
  const uint32_t items = J.nch - 1;
  uint32_t run[T];
#pragma unroll
  for (int j = 0; j < T; j++) run[j] = 0;
  for (uint32_t i0 = 0; i0 < items; i0 += DS_T) {   // (uniform)
    const uint32_t i = i0 + tid;
    uint32_t v[T], w[W];
#pragma unroll
    for (int x = 0; x < W; x++) w[x] = 0;
    if (i < items) {
      const uint32_t* p = reinterpret_cast<const uint32_t*>(J.agg + 16 * (size_t)(J.nch - 1 - i));
#pragma unroll
      for (int x = 0; x < W; x++) w[x] = p[x];
    }
    ds_unpack<T>(w, v);
    if (tid == 0 && i0) ds_mulx<T>(tab, run, v);
    ds_block_scan<T>(v, tab, sc);
    if (i < items) {
      uint32_t o[4] = {0, 0, 0, 0};
      ds_pack<T>(v, w);
#pragma unroll
      for (int x = 0; x < W; x++) o[x] = w[x];
      *reinterpret_cast<uint4*>(J.carry + 16 * (size_t)(J.nch - 2 - i)) = make_uint4(o[0], o[1], o[2], o[3]);
    }
    if (tid == 0) {
#pragma unroll
      for (int x = 0; x < W; x++) w[x] = sc[(DS_T - 1) * W + x];
      ds_unpack<T>(w, run);
    }
    __syncthreads();
  }
}

// Phase 3, block (x, job): chunks x, x + gridDim.x, ...: quotient bytes, remainder, lengths, status.
template <int T>
__global__ __launch_bounds__(DS_T) void divshort_apply_kernel(DsBatch B) {
  constexpr int W = Words<T>::W;
  __shared__ __attribute__((aligned(16))) uint8_t in[DS_B + 32];
  __shared__ __attribute__((aligned(16))) uint8_t out[DS_B + 32];
  __shared__ __attribute__((aligned(16))) uint8_t tab[DS_LEVELS * T * T];
  __shared__ __attribute__((aligned(16))) uint8_t tmp[2 * T * T];
  __shared__ __attribute__((aligned(16))) uint32_t sc[DS_T * W];
  __shared__ uint32_t red[DS_T / PLK_WAVE];
  const DsJob& J = B.j[blockIdx.y];
  if (blockIdx.x >= J.nch) return;   // (uniform)
  ds_build_tables<T>(J, DS_E_LOG, tab, tmp);
  uint32_t Dr[T];
#pragma unroll
  for (int j = 0; j < T; j++) Dr[j] = J.D[j];
  const int tid = threadIdx.x;
  const int64_t ql = J.nl > J.t ? (int64_t)J.nl - J.t : 0;   // quotient coefficients the scan produces
  for (uint32_t k = blockIdx.x; k < J.nch; k += gridDim.x) {
    const DsChunk c = ds_chunk(J, k);
    const int64_t qlo = c.v0, qhi = min(c.v0 + DS_B, ql);
    const uint32_t qoff = (uint32_t)((uintptr_t)(J.quot + qlo) & 15u);
    ds_load_chunk(J.num, c.ilo, c.ihi, c.ioff, in);
    __syncthreads();
    const int64_t vtop = c.v0 + DS_B - 1 - (int64_t)tid * DS_E;
    uint32_t S[T], top = 0, bad = 0;
#pragma unroll
    for (int j = 0; j < T; j++) S[j] = 0;
    ds_walk<T, false>(S, Dr, J.inv, in, vtop, J.s, c.ilo, c.ihi, c.ioff, nullptr, 0, 0, 0, top, bad);
    uint32_t cin[T], w[W];
#pragma unroll
    for (int x = 0; x < W; x++) w[x] = 0;
    if (k + 1 < J.nch) {   // (uniform)
      const uint32_t* p = reinterpret_cast<const uint32_t*>(J.carry + 16 * (size_t)k);
#pragma unroll
      for (int x = 0; x < W; x++) w[x] = p[x];
    }
    ds_unpack<T>(w, cin);
    if (tid == 0) ds_mulx<T>(tab, cin, S);
    ds_block_scan<T>(S, tab, sc);
    if (tid) {
#pragma unroll
      for (int x = 0; x < W; x++) w[x] = sc[(tid - 1) * W + x];
    }
    ds_unpack<T>(w, S);   // (thread 0: w still holds the carry)
    ds_walk<T, true>(S, Dr, J.inv, in, vtop, J.s, c.ilo, c.ihi, c.ioff, out, qlo, qhi, qoff, top, bad);
    if (k == 0 && tid == DS_T - 1) {   // the state below virtual index 0: r x^s
      const int rl = (int)min((uint32_t)J.t, J.nl);
      uint32_t rtop = 0;
#pragma unroll
      for (int j = 0; j < T; j++) {
        const int r = j - (int)J.s;
        if (r >= 0 && r < rl) {
          J.rem[r] = (uint8_t)S[j];
          if (S[j]) rtop = (uint32_t)r + 1;
        }
      }
      if (rtop) atomicMax(J.lens + 1, rtop);
      if (ql == 0) J.quot[0] = 0;   // nl < dl: q = {0}
    }
    __syncthreads();
    ds_store_chunk(J.quot, qlo, qhi, qoff, out);
    // lengths and status: one atomic a block at the most, none when a load shows the word settled
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) top = max(top, (uint32_t)__shfl_xor(top, off, PLK_WAVE));
    if ((tid & (PLK_WAVE - 1)) == 0) red[tid / PLK_WAVE] = top;
    const int anybad = __syncthreads_or((int)bad);
    if (tid == 0) {
      uint32_t m = 0;
#pragma unroll
      for (int u = 0; u < DS_T / PLK_WAVE; u++) m = max(m, red[u]);
      if (m && __hip_atomic_load(J.lens, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < m) atomicMax(J.lens, m);
      if (anybad && __hip_atomic_load(J.lens + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) atomicMax(J.lens + 2, 1u);
    }
    __syncthreads();
  }
}

int bucket_of(size_t dl) { return dl <= 3 ? 2 : dl <= 5 ? 4 : dl <= 9 ? 8 : 16; }   // T >= t = dl - 1

uint64_t chunks_of(uint64_t nl, uint64_t dl) {
  const uint64_t s = (uint64_t)bucket_of(dl) - (dl - 1);
  return (nl + s + DS_B - 1) / DS_B;
}

// the argument errors of one job (no device is touched)
int check_job(const char* fn, const plk_divshort_job_t* job, int b) {
  if (!job->num || !job->den || !job->quot || !job->rem) {
    plk_set_error("%s: job %d: num, den, quot and rem are required", fn, b);
    return PLK_ERR_ARG;
  }
  if (job->nl == 0 || job->dl < 2) {
    plk_set_error("%s: job %d: nl >= 1 and dl >= 2 are required", fn, b);
    return PLK_ERR_ARG;
  }
  if (job->dl > PLK_DIV_SHORT_MAX) {
    plk_set_error("%s: job %d: a divisor of %zu coefficients (at most %d)", fn, b, job->dl, PLK_DIV_SHORT_MAX);
    return PLK_ERR_RANGE;
  }
  for (size_t i = 0; i < job->dl; i++)
    if (job->den[i] >= HFP) {
      plk_set_error("%s: job %d: divisor byte %zu is not a GF(17) value", fn, b, i);
      return PLK_ERR_ARG;
    }
  if (job->den[job->dl - 1] == 0) {
    plk_set_error("%s: job %d: the divisor's lead is zero", fn, b);
    return PLK_ERR_ARG;
  }
  if ((uint64_t)job->nl >= (1ull << 32)) {
    plk_set_error("%s: job %d: a numerator of 2^32 coefficients or more", fn, b);
    return PLK_ERR_RANGE;
  }
  return PLK_OK;
}

int check_jobs(const char* fn, const plk_divshort_job_t* jobs, int n) {
  if (!jobs || n <= 0) {
    plk_set_error("%s: jobs and n > 0 are required", fn);
    return PLK_ERR_ARG;
  }
  for (int b = 0; b < n; b++) {
    const int rc = check_job(fn, jobs + b, b);
    if (rc) return rc;
  }
  return PLK_OK;
}

size_t work_bytes(const plk_divshort_job_t* jobs, int n) {
  size_t total = 16;   // the base is rounded up to 16 bytes
  for (int b = 0; b < n; b++) total += 32 * (size_t)chunks_of(jobs[b].nl, jobs[b].dl);
  return total;
}

template <int T>
int launch_group(const DsBatch& B, int nj, uint32_t maxch, hipStream_t st) {
  const uint32_t gx = std::min<uint32_t>(maxch, DS_MAX_GRID);
  if (maxch > 1) {
    hipLaunchKernelGGL(divshort_agg_kernel<T>, dim3(std::min<uint32_t>(maxch - 1, DS_MAX_GRID), (uint32_t)nj), dim3(DS_T), 0,
                       st, B);
    PLK_HIP(hipGetLastError());
    hipLaunchKernelGGL(divshort_carry_kernel<T>, dim3((uint32_t)nj), dim3(DS_T), 0, st, B);
    PLK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(divshort_apply_kernel<T>, dim3(gx, (uint32_t)nj), dim3(DS_T), 0, st, B);
  PLK_HIP(hipGetLastError());
  return PLK_OK;
}

// The launches of a batch: one memset node for the 3 n words, then per state bucket the jobs of that
// bucket in call order, DS_JOBS to a group, each group one kernel (every job within one chunk) or three.
int launch_jobs(const plk_divshort_job_t* jobs, int n, uint32_t* d_lens, void* d_work, hipStream_t st) {
  PLK_HIP(hipMemsetAsync(d_lens, 0, (size_t)3 * n * sizeof(uint32_t), st));
  uint8_t* work = (uint8_t*)(((uintptr_t)d_work + 15) & ~(uintptr_t)15);
  std::vector<size_t> off((size_t)n);
  size_t total = 0;
  for (int b = 0; b < n; b++) {
    off[b] = total;
    total += 32 * (size_t)chunks_of(jobs[b].nl, jobs[b].dl);
  }
  uint32_t inv17[17] = {0};
  for (uint32_t a = 1; a < HFP; a++)
    for (uint32_t x = 1; x < HFP; x++)
      if (a * x % HFP == 1) inv17[a] = x;
  for (int T = 2; T <= 16; T *= 2) {
    int b = 0;
    while (b < n) {
      DsBatch B;
      memset(&B, 0, sizeof B);
      int nj = 0;
      uint32_t maxch = 0;
      for (; b < n && nj < DS_JOBS; b++) {
        const plk_divshort_job_t& S = jobs[b];
        if (bucket_of(S.dl) != T) continue;
        DsJob& J = B.j[nj++];
        J.num = S.num;
        J.quot = S.quot;
        J.rem = S.rem;
        J.lens = d_lens + 3 * (size_t)b;
        J.nl = (uint32_t)S.nl;
        J.nch = (uint32_t)chunks_of(S.nl, S.dl);
        J.agg = work + off[b];
        J.carry = J.agg + 16 * (size_t)J.nch;
        J.t = (uint8_t)(S.dl - 1);
        J.s = (uint8_t)(T - J.t);
        J.inv = (uint8_t)inv17[S.den[S.dl - 1]];
        for (int j = 0; j < T; j++) J.D[j] = j >= J.s ? S.den[j - J.s] : 0;
        maxch = std::max(maxch, J.nch);
      }
      if (!nj) break;
      int rc = T == 2 ? launch_group<2>(B, nj, maxch, st) : T == 4 ? launch_group<4>(B, nj, maxch, st)
               : T == 8 ? launch_group<8>(B, nj, maxch, st) : launch_group<16>(B, nj, maxch, st);
      if (rc) return rc;
    }
  }
  return PLK_OK;
}

size_t quot_bytes(const plk_divshort_job_t& j) { return j.nl >= j.dl ? j.nl - j.dl + 1 : 1; }
size_t rem_bytes(const plk_divshort_job_t& j) { return std::min(j.dl - 1, j.nl); }

}  // namespace

extern "C" {

size_t plk_poly_divide_short_workspace(const plk_divshort_job_t* jobs, int n) {
  if (!jobs || n <= 0) return 0;
  for (int b = 0; b < n; b++)
    if (jobs[b].nl == 0 || jobs[b].dl < 2 || jobs[b].dl > PLK_DIV_SHORT_MAX || (uint64_t)jobs[b].nl >= (1ull << 32)) return 0;
  return work_bytes(jobs, n);
}

int plk_poly_divide_short_plan(size_t nl, size_t dl, int out[4]) {
  const char* fn = "plk_poly_divide_short_plan";
  if (!out || nl == 0 || dl < 2) {
    plk_set_error("%s: out, nl >= 1 and dl >= 2 are required", fn);
    return PLK_ERR_ARG;
  }
  if (dl > PLK_DIV_SHORT_MAX || (uint64_t)nl >= (1ull << 32)) {
    plk_set_error("%s: dl <= %d and nl < 2^32 are required", fn, PLK_DIV_SHORT_MAX);
    return PLK_ERR_RANGE;
  }
  out[0] = chunks_of(nl, dl) > 1 ? 3 : 1;
  out[1] = DS_E;
  out[2] = DS_B;
  out[3] = DS_B - (bucket_of(dl) - (int)(dl - 1));
  return PLK_OK;
}

int plk_poly_divide_short_batch_dev(const plk_divshort_job_t* jobs, int n, uint32_t* d_lens, void* d_work, void* stream) {
  const char* fn = "plk_poly_divide_short_batch_dev";
  int rc = check_jobs(fn, jobs, n);
  if (rc) return rc;
  if (!d_lens || !d_work) {
    plk_set_error("%s: d_lens and d_work are required", fn);
    return PLK_ERR_ARG;
  }
  if ((rc = plk_use_device())) return rc;
  return launch_jobs(jobs, n, d_lens, d_work, (hipStream_t)stream);
}

int plk_poly_divide_short_batch(const plk_divshort_job_t* jobs, int n, size_t* quot_lens, size_t* rem_lens) {
  const char* fn = "plk_poly_divide_short_batch";
  int rc = check_jobs(fn, jobs, n);
  if (rc) return rc;
  if (!quot_lens || !rem_lens) {
    plk_set_error("%s: quot_lens and rem_lens are required", fn);
    return PLK_ERR_ARG;
  }
  if ((rc = plk_select_device())) return rc;
  // one allocation: the length words, every job's numerator, quotient and remainder in 16-byte aligned
  // slots, the workspace
  std::vector<plk_divshort_job_t> dj(jobs, jobs + n);
  std::vector<size_t> o_num((size_t)n), o_q((size_t)n), o_r((size_t)n);
  size_t total = plk_pad16((size_t)3 * n * sizeof(uint32_t));
  for (int b = 0; b < n; b++) {
    o_num[b] = total;
    total += plk_pad16(jobs[b].nl);
    o_q[b] = total;
    total += plk_pad16(quot_bytes(jobs[b]));
    o_r[b] = total;
    total += plk_pad16(rem_bytes(jobs[b]));
  }
  const size_t o_work = total;
  total += work_bytes(jobs, n);
  PlkScratch S;
  if ((rc = S.alloc(fn, total))) return rc;
  for (int b = 0; b < n; b++) {
    PLK_HIP(hipMemcpy(S.d + o_num[b], jobs[b].num, jobs[b].nl, hipMemcpyHostToDevice));
    dj[b].num = S.d + o_num[b];
    dj[b].quot = S.d + o_q[b];
    dj[b].rem = S.d + o_r[b];
  }
  if ((rc = launch_jobs(dj.data(), n, (uint32_t*)S.d, S.d + o_work, nullptr))) return rc;
  std::vector<uint32_t> lens((size_t)3 * n);
  PLK_HIP(hipMemcpy(lens.data(), S.d, lens.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  for (int b = 0; b < n; b++) {
    if (lens[3 * b + 2]) continue;
    PLK_HIP(hipMemcpy(jobs[b].quot, S.d + o_q[b], quot_bytes(jobs[b]), hipMemcpyDeviceToHost));
    PLK_HIP(hipMemcpy(jobs[b].rem, S.d + o_r[b], rem_bytes(jobs[b]), hipMemcpyDeviceToHost));
    quot_lens[b] = lens[3 * b] ? lens[3 * b] : 1;
    rem_lens[b] = lens[3 * b + 1] ? lens[3 * b + 1] : 1;
  }
  // a numerator holding a byte >= 17: the reference's loop on the raw bytes, as plk_poly_divide runs it
  for (int b = 0; b < n; b++) {
    if (!lens[3 * b + 2]) continue;
    if ((rc = plk_poly_divide(jobs[b].num, jobs[b].nl, jobs[b].den, jobs[b].dl, jobs[b].quot, quot_lens + b, jobs[b].rem,
                              rem_lens + b)))
      return rc;
  }
  return PLK_OK;
}

int plk_poly_from_roots(const uint8_t* roots, int t, uint8_t* out) {
  const char* fn = "plk_poly_from_roots";
  if (!roots || !out || t < 1) {
    plk_set_error("%s: roots, out and t >= 1 are required", fn);
    return PLK_ERR_ARG;
  }
  if (t > PLK_DIV_SHORT_MAX - 1) {
    plk_set_error("%s: at most %d roots", fn, PLK_DIV_SHORT_MAX - 1);
    return PLK_ERR_RANGE;
  }
  for (int i = 0; i < t; i++)
    if (roots[i] >= HFP) {
      plk_set_error("%s: root %d is not a GF(17) value", fn, i);
      return PLK_ERR_ARG;
    }
  uint8_t p[PLK_DIV_SHORT_MAX] = {1};
  for (int i = 0; i < t; i++) {   // p <- p (x - roots[i])
    const uint32_t m = (HFP - roots[i]) % HFP;
    p[i + 1] = 0;
    for (int j = i + 1; j > 0; j--) p[j] = (uint8_t)((p[j - 1] + m * p[j]) % HFP);
    p[0] = (uint8_t)(m * p[0] % HFP);
  }
  memcpy(out, p, (size_t)t + 1);
  return PLK_OK;
}

}  // extern "C"
