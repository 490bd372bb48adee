// Linear combinations of device polynomials (include/plonkhip.h, "poly linear combinations"):
// the reference's poly_add / poly_sub / poly_scale / poly_negate / poly_shift / poly_add_hf and the
// x -> twist x coefficient loop (src/poly.h:66-104, 179-216, 240-254, src/plonk.h:466-470) composed in
// ONE streaming pass: every term read once, the result written once, nothing in between.
//
//   Geometry  A lane owns 16 output bytes, a block 256 lanes.  The groups are cut on the 16-byte
//             boundaries of the OUTPUT ADDRESS (group g covers addresses [A + 16 g, A + 16 g + 16), A =
//             out rounded down to 16), so every group that lies inside the result is one aligned uint4
//             store whatever the base pointer; only the first and last group of a job may store bytes.
//             A term's bytes for a group sit at p + (j0 - shift): one uint4 load when that address is
//             16-byte aligned, two aligned loads joined by a byte funnel when it is not and both loads
//             lie inside the array, byte loads otherwise (the array's first and last groups).  No byte
//             outside [p, p + len) is read, none outside [out, out + L) written.
//   Fast path Per group, taken when every byte of every term that passes its bytes on unchanged (twist 0,
//             scale PLK_LC_RAW) is < 17.  Every operand of every hf_add / hf_sub / hf_neg is then
//             canonical (hf_mul reduces whatever it is given), so the whole fold is arithmetic mod 17:
//             out[j] = mod17(sum_i c_i[j] byte_i[j] + add_hf), c_i[j] <= 16 folding the scale, 17 - c for
//             sub xor neg and twist^(index mod 16).  The index of byte k of a group is k + (j0 - shift),
//             and j0 advances by 16 from group to group, so the sixteen weights of a (job, term) are the
//             same for every lane: the host packs them into four words of the launch structure.  The sum
//             is at most 16 x 16 x 255 + 16 = 65296, inside mod17's exact range; one reduction per
//             coefficient.
//   Slow path A group holding a raw byte >= 17 is redone byte by byte with the reference's uint8_t /
//             int8_t formulas in term order (the terms' bytes re-read: they are in cache).  Lanes
//             diverge only there.
//   d_nz      index + 1 of the last non-zero byte: the words are zeroed by one memset node in front of
//             the launches; a block reduces its lanes' candidates, and issues its device-scope atomicMax
//             only when it holds a non-zero byte, the first 64 result bytes ABOVE its chunk (recomputed by
//             one wave, a byte load per term) show none, AND a load of the word shows a smaller value.
//             For a dense polynomial only the top block reaches the word.  Blocks take the result's
//             chunks from the top down, so that block runs first.
#include <string.h>

#include <algorithm>
#include <vector>

#include "plk_device.h"
#include "plk_hf17.h"
#include "plk_hostcall.h"
#include "plk_internal.h"

namespace {

constexpr int LC_T = 256, LC_E = 16, LC_CHUNK = LC_T * LC_E;
constexpr int LC_JOBS = 24;    // jobs per launch
constexpr int LC_TERMS = 48;   // terms per launch (>= PLK_LC_MAX_TERMS: any job fits)
constexpr uint32_t HFP = hf17::P;
using hf17::add8;
using hf17::any_noncanonical;
using hf17::mod17;
using hf17::neg8;
using hf17::sub8_wide;
static_assert(LC_TERMS >= PLK_LC_MAX_TERMS, "a job is never split across launches");

constexpr uint32_t CFG_SUB = 1u << 16, CFG_NEG = 1u << 17, CFG_PASS = 1u << 18;

struct LcTerm {
  const uint8_t* p;
  uint32_t len, shift;
  uint32_t wq[4];   // fast path: the weight of byte k of a group, four to a word
  uint32_t cfg;     // [7:0] scale, [15:8] twist, CFG_SUB, CFG_NEG, CFG_PASS (bytes passed on unchanged)
  uint32_t pad;
};
struct LcJob {
  uint8_t* out;
  uint32_t* nz;      // nullptr: not wanted
  uint32_t len;      // L
  uint32_t nblk;     // blocks of the job
  uint16_t lead;     // out & 15: group g covers result indices [16 g - lead, 16 g - lead + 16)
  uint16_t inplace;  // out is a term's p: other blocks' results replace input bytes while the launch runs
  uint16_t first;    // first term in LcBatch::t
  uint8_t nterms;
  int8_t add_hf;
};
struct LcBatch {
  LcJob j[LC_JOBS];
  LcTerm t[LC_TERMS];
};
static_assert(sizeof(LcTerm) == 40 && sizeof(LcJob) == 32, "launch structure layout");
static_assert(sizeof(LcBatch) <= 3072, "the launch structure travels by value: kernel arguments are 4 KiB at most");

// Bytes [i0, i0 + 16) of p[0, len) as four words, zero outside the array (i0 may be negative).
__device__ __forceinline__ void lc_load16(const uint8_t* p, int64_t len, int64_t i0, uint32_t (&w)[4]) {
  if (i0 >= 0 && i0 + 16 <= len) {
    const uintptr_t a = (uintptr_t)(p + i0);
    const uint32_t m = (uint32_t)(a & 15u);
    if (m == 0) {
      const uint4 v = *reinterpret_cast<const uint4*>(p + i0);
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
      return;
    }
    if (i0 >= (int64_t)m && i0 - (int64_t)m + 32 <= len) {
      // two aligned loads inside the array, joined by a byte funnel (static register indices only)
      const uint4 lo = *reinterpret_cast<const uint4*>(p + i0 - m);
      const uint4 hi = *reinterpret_cast<const uint4*>(p + i0 - m + 16);
      const uint32_t s = m >> 2, r = 8u * (m & 3u);
      const uint32_t x0 = s == 0 ? lo.x : s == 1 ? lo.y : s == 2 ? lo.z : lo.w;
      const uint32_t x1 = s == 0 ? lo.y : s == 1 ? lo.z : s == 2 ? lo.w : hi.x;
      const uint32_t x2 = s == 0 ? lo.z : s == 1 ? lo.w : s == 2 ? hi.x : hi.y;
      const uint32_t x3 = s == 0 ? lo.w : s == 1 ? hi.x : s == 2 ? hi.y : hi.z;
      const uint32_t x4 = s == 0 ? hi.x : s == 1 ? hi.y : s == 2 ? hi.z : hi.w;
      w[0] = __funnelshift_r(x0, x1, r);
      w[1] = __funnelshift_r(x1, x2, r);
      w[2] = __funnelshift_r(x2, x3, r);
      w[3] = __funnelshift_r(x3, x4, r);
      return;
    }
  }
  uint32_t x0 = 0, x1 = 0, x2 = 0, x3 = 0;
  if (i0 + 16 > 0 && i0 < len) {
    // byte-wise, each byte shifted in from the top (a rolled loop: this is the arrays' edges only)
#pragma nounroll
    for (int k = 0; k < 16; k++) {
      const int64_t i = i0 + k;
      const uint32_t b = i >= 0 && i < len ? p[i] : 0u;
      x0 = x0 >> 8 | x1 << 24;
      x1 = x1 >> 8 | x2 << 24;
      x2 = x2 >> 8 | x3 << 24;
      x3 = x3 >> 8 | b << 24;
    }
  }
  w[0] = x0; w[1] = x1; w[2] = x2; w[3] = x3;
}

// result byte j by the reference's formulas in term order (the specification, literally)
__device__ __forceinline__ uint32_t lc_slow_byte(const LcBatch& B, const LcJob& J, int64_t j) {
  uint32_t acc = 0;
  for (uint32_t t = 0; t < J.nterms; t++) {
    const LcTerm& T = B.t[J.first + t];
    const int64_t i = j - (int64_t)T.shift;
    uint32_t v = 0;
    if (i >= 0 && i < (int64_t)T.len) {
      v = T.p[i];
      const uint32_t scale = T.cfg & 0xFFu, twist = (T.cfg >> 8) & 0xFFu;
      if (twist) {
        uint32_t pw = 1;
        for (uint32_t e = (uint32_t)i & 15u; e > 0; e--) pw = pw * twist % HFP;
        v = v * pw % HFP;
      }
      if (scale != PLK_LC_RAW) v = v * scale % HFP;
      if (T.cfg & CFG_NEG) v = neg8(v);
    }
    acc = t == 0 ? v : (T.cfg & CFG_SUB) ? sub8_wide(acc, v) : add8(acc, v);
  }
  if (j == 0 && J.add_hf >= 0) acc = add8(acc, (uint32_t)J.add_hf);
  return acc;
}

// Block (x, job): the job's chunks from the top down, one 16-byte group of the result per lane.
__global__ __launch_bounds__(LC_T) void lincomb_kernel(LcBatch B) {
  __shared__ uint32_t wmax[LC_T / PLK_WAVE];
  const LcJob& J = B.j[blockIdx.y];
  if (blockIdx.x >= J.nblk) return;
  const uint32_t c = J.nblk - 1 - blockIdx.x;
  const int64_t L = J.len;
  const int64_t j0 = ((int64_t)c * LC_T + threadIdx.x) * LC_E - (int64_t)J.lead;   // the group's first result index
  uint32_t top = 0;   // index + 1 of the lane's last non-zero byte
  if (j0 < L) {       // (j0 + 16 > 0 always: lead < 16)
    uint32_t acc[LC_E];
#pragma unroll
    for (int k = 0; k < LC_E; k++) acc[k] = 0;
    bool bad = false;
    for (uint32_t t = 0; t < J.nterms; t++) {   // (uniform)
      const LcTerm& T = B.t[J.first + t];
      uint32_t w[4];
      lc_load16(T.p, (int64_t)T.len, j0 - (int64_t)T.shift, w);
      if (T.cfg & CFG_PASS) bad |= any_noncanonical(w);
#pragma unroll
      for (int k = 0; k < LC_E; k++)
        acc[k] = __umul24((w[k >> 2] >> (8 * (k & 3))) & 0xFFu, (T.wq[k >> 2] >> (8 * (k & 3))) & 0xFFu) + acc[k];
    }
    if (j0 <= 0 && J.add_hf >= 0) {   // (result index 0: the first group only)
#pragma unroll
      for (int k = 0; k < LC_E; k++) acc[k] += j0 + k == 0 ? (uint32_t)J.add_hf : 0u;
    }
    uint32_t o[4] = {0, 0, 0, 0};
    if (!bad) {
#pragma unroll
      for (int k = 0; k < LC_E; k++) o[k >> 2] |= mod17(acc[k]) << (8 * (k & 3));   // (acc <= 65296)
    } else {
#pragma nounroll
      for (int k = 0; k < LC_E; k++) {
        const int64_t j = j0 + k;
        const uint32_t v = j >= 0 && j < L ? lc_slow_byte(B, J, j) : 0u;
        o[0] = o[0] >> 8 | o[1] << 24;
        o[1] = o[1] >> 8 | o[2] << 24;
        o[2] = o[2] >> 8 | o[3] << 24;
        o[3] = o[3] >> 8 | v << 24;
      }
    }
    if (j0 >= 0 && j0 + 16 <= L) {
      *reinterpret_cast<uint4*>(J.out + j0) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int k = 0; k < LC_E; k++) {
        const int64_t j = j0 + k;
        if (j >= 0 && j < L) J.out[j] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
      }
    }
    if (J.nz) {   // (bytes outside the result are zero: every term reads as zero there)
      const uint32_t hiw = o[3] ? 3u : o[2] ? 2u : o[1] ? 1u : 0u;
      const uint32_t x = o[3] ? o[3] : o[2] ? o[2] : o[1] ? o[1] : o[0];
      if (x) top = (uint32_t)(j0 + 4 * hiw + ((31 - __clz((int)x)) >> 3) + 1);
    }
  }
  if (!J.nz) return;   // (uniform)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) top = max(top, (uint32_t)__shfl_xor(top, off, PLK_WAVE));
  if ((threadIdx.x & (PLK_WAVE - 1)) == 0) wmax[threadIdx.x / PLK_WAVE] = top;
  __syncthreads();
  if (threadIdx.x >= PLK_WAVE) return;   // wave 0 decides
  uint32_t m = 0;
#pragma unroll
  for (int u = 0; u < LC_T / PLK_WAVE; u++) m = max(m, wmax[u]);
  if (m == 0) return;   // (uniform) nothing to report
  // A non-zero byte anywhere above this block's chunk puts the word's final value above m: nothing to
  // add.  The lanes look at the first 64 result bytes of the chunk above (one coalesced byte load per
  // term), each by the fast-path sum, which is exact for a position whose raw bytes are all < 17; a
  // lane that meets a raw byte >= 17, or the end of the result, claims nothing.  For a dense result
  // this keeps all but the top block away from the word.  (Not in place: the bytes above may already be
  // another block's results.)
  const int64_t j = ((int64_t)c + 1) * LC_CHUNK - (int64_t)J.lead + (int64_t)threadIdx.x;   // (j + lead = lane mod 16)
  bool above = false;
  if (!J.inplace && ((int64_t)c + 1) * LC_CHUNK - (int64_t)J.lead < L) {   // (uniform)
    const uint32_t k = threadIdx.x & 15u, q = k >> 2;
    bool known = j < L;
    uint32_t s = 0;
    // eight terms at a time, their byte loads unconditional (index clamped into the array, slots past
    // nterms repeat the last term) so that they are in flight together; what does not count is masked
    for (uint32_t t0 = 0; t0 < J.nterms; t0 += 8) {   // (uniform)
      uint32_t b[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const LcTerm& T = B.t[J.first + min(t0 + u, (uint32_t)J.nterms - 1)];
        const int64_t i = j - (int64_t)T.shift;
        b[u] = T.p[min(max(i, (int64_t)0), (int64_t)T.len - 1)];
      }
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const LcTerm& T = B.t[J.first + min(t0 + u, (uint32_t)J.nterms - 1)];
        const int64_t i = j - (int64_t)T.shift;
        const bool in = t0 + u < J.nterms && i >= 0 && i < (int64_t)T.len;
        if (in && (T.cfg & CFG_PASS) && b[u] >= HFP) known = false;
        const uint32_t wsel = q == 0 ? T.wq[0] : q == 1 ? T.wq[1] : q == 2 ? T.wq[2] : T.wq[3];
        s += in ? b[u] * ((wsel >> (8 * (k & 3))) & 0xFFu) : 0u;
      }
    }
    above = known && mod17(s) != 0;   // (s <= 16 x 16 x 255)
  }
  if (__ballot(above) != 0) return;
  if (threadIdx.x == 0 && __hip_atomic_load(J.nz, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < m) atomicMax(J.nz, m);
}

int64_t blocks_of(uint64_t lead, uint64_t L) { return (int64_t)((lead + L + LC_CHUNK - 1) / LC_CHUNK); }

// L of a job whose fields passed check_job, or 0 when len + shift does not fit a size_t
size_t job_len(const plk_lc_job_t* job) {
  size_t L = 0;
  for (int i = 0; i < job->nterms; i++) {
    const plk_lc_term_t& T = job->terms[i];
    if (T.len + T.shift < T.len) return 0;
    L = std::max(L, T.len + T.shift);
  }
  return L;
}

// the PLK_ERR_ARG conditions of one job (no device is touched)
int check_job(const char* fn, const plk_lc_job_t* job, int b, bool want_out) {
  if (!job->terms || (want_out && !job->out)) {
    plk_set_error("%s: job %d: terms and out are required", fn, b);
    return PLK_ERR_ARG;
  }
  if (job->nterms < 1 || job->nterms > PLK_LC_MAX_TERMS) {
    plk_set_error("%s: job %d: nterms = %d is outside 1 .. %d", fn, b, job->nterms, PLK_LC_MAX_TERMS);
    return PLK_ERR_ARG;
  }
  if (job->add_hf < -1 || job->add_hf > 16) {
    plk_set_error("%s: job %d: add_hf = %d is neither -1 nor a GF(17) value", fn, b, job->add_hf);
    return PLK_ERR_ARG;
  }
  for (int i = 0; i < job->nterms; i++) {
    const plk_lc_term_t& T = job->terms[i];
    if (!T.p || T.len == 0) {
      plk_set_error("%s: job %d term %d: a polynomial of at least one coefficient is required", fn, b, i);
      return PLK_ERR_ARG;
    }
    if (T.sub > 1 || T.neg > 1 || (T.scale > 16 && T.scale != PLK_LC_RAW) || T.twist > 16) {
      plk_set_error("%s: job %d term %d: sub, neg in 0 .. 1, scale in 0 .. 16 or PLK_LC_RAW, twist in 0 .. 16", fn, b, i);
      return PLK_ERR_ARG;
    }
    if (i == 0 && T.sub) {
      plk_set_error("%s: job %d: term 0 starts the accumulator and cannot be subtracted", fn, b);
      return PLK_ERR_ARG;
    }
  }
  return PLK_OK;
}

int check_jobs(const char* fn, const plk_lc_job_t* jobs, int n) {
  if (!jobs || n <= 0) {
    plk_set_error("%s: jobs and n > 0 are required", fn);
    return PLK_ERR_ARG;
  }
  for (int b = 0; b < n; b++) {
    const int rc = check_job(fn, jobs + b, b, true);
    if (rc) return rc;
  }
  for (int b = 0; b < n; b++) {
    const size_t L = job_len(jobs + b);
    if (L == 0 || (uint64_t)L >= (1ull << 32)) {
      plk_set_error("%s: job %d: a result of 2^32 coefficients or more", fn, b);
      return PLK_ERR_RANGE;
    }
  }
  return PLK_OK;
}

// the sixteen fast-path weights of a term for a result whose groups start at indices = -lead mod 16:
// byte k of a group is the term's coefficient k - lead - shift (mod 16)
void term_weights(const plk_lc_term_t& T, uint32_t lead, uint32_t wq[4]) {
  uint32_t c = T.scale == PLK_LC_RAW ? 1u : T.scale;
  if ((T.sub ^ T.neg) & 1u) c = (HFP - c) % HFP;
  uint32_t pw[16];
  pw[0] = 1;
  for (int e = 1; e < 16; e++) pw[e] = T.twist ? pw[e - 1] * T.twist % HFP : 1u;
  wq[0] = wq[1] = wq[2] = wq[3] = 0;
  for (uint32_t k = 0; k < 16; k++) {
    const uint32_t e = (k - lead - (uint32_t)(T.shift & 15u)) & 15u;
    wq[k >> 2] |= (c * pw[e] % HFP) << (8 * (k & 3));
  }
}

// the launches of a batch: as many whole jobs as LC_JOBS and LC_TERMS allow per launch, consecutive
// on the stream
int launch_jobs(const plk_lc_job_t* jobs, int n, uint32_t* d_nz, hipStream_t st) {
  if (d_nz) PLK_HIP(hipMemsetAsync(d_nz, 0, (size_t)n * sizeof(uint32_t), st));
  int b = 0;
  while (b < n) {
    LcBatch B;
    memset(&B, 0, sizeof B);
    int nj = 0, nt = 0;
    int64_t maxb = 1;
    for (; b < n && nj < LC_JOBS && nt + jobs[b].nterms <= LC_TERMS; b++, nj++) {
      const plk_lc_job_t& S = jobs[b];
      LcJob& J = B.j[nj];
      J.out = S.out;
      J.nz = d_nz ? d_nz + b : nullptr;
      J.len = (uint32_t)job_len(&S);
      J.lead = (uint16_t)((uintptr_t)S.out & 15u);
      J.nblk = (uint32_t)blocks_of(J.lead, J.len);
      J.first = (uint16_t)nt;
      J.nterms = (uint8_t)S.nterms;
      J.add_hf = (int8_t)S.add_hf;
      maxb = std::max<int64_t>(maxb, J.nblk);
      for (int i = 0; i < S.nterms; i++, nt++) {
        const plk_lc_term_t& T = S.terms[i];
        LcTerm& D = B.t[nt];
        D.p = T.p;
        if (T.p == S.out) J.inplace = 1;
        D.len = (uint32_t)T.len;
        D.shift = (uint32_t)T.shift;
        D.cfg = (uint32_t)T.scale | (uint32_t)T.twist << 8 | (T.sub ? CFG_SUB : 0u) | (T.neg ? CFG_NEG : 0u) |
                (T.twist == 0 && T.scale == PLK_LC_RAW ? CFG_PASS : 0u);
        term_weights(T, J.lead, D.wq);
      }
    }
    hipLaunchKernelGGL(lincomb_kernel, dim3((uint32_t)maxb, (uint32_t)nj), dim3(LC_T), 0, st, B);
    PLK_HIP(hipGetLastError());
  }
  return PLK_OK;
}

}  // namespace

extern "C" {

size_t plk_poly_lincomb_len(const plk_lc_job_t* job) {
  if (!job || check_job("plk_poly_lincomb_len", job, 0, false)) return 0;
  return job_len(job);
}

int plk_poly_lincomb_batch_dev(const plk_lc_job_t* jobs, int n, uint32_t* d_nz, void* stream) {
  int rc = check_jobs("plk_poly_lincomb_batch_dev", jobs, n);
  if (rc || (rc = plk_use_device())) return rc;
  return launch_jobs(jobs, n, d_nz, (hipStream_t)stream);
}

int plk_poly_lincomb(const plk_lc_job_t* job, size_t* out_len) {
  const char* fn = "plk_poly_lincomb";
  if (!job || !out_len) {
    plk_set_error("%s: job and out_len are required", fn);
    return PLK_ERR_ARG;
  }
  int rc = check_jobs(fn, job, 1);
  if (rc || (rc = plk_select_device())) return rc;
  // every term uploaded to its own 16-byte aligned slot, the result into one more (out may be a term's p)
  const size_t L = job_len(job);
  size_t total = 16;
  for (int i = 0; i < job->nterms; i++) total += plk_pad16(job->terms[i].len);
  const size_t o_out = total;
  total += plk_pad16(L);
  PlkScratch S;
  if ((rc = S.alloc(fn, total))) return rc;
  plk_lc_term_t terms[PLK_LC_MAX_TERMS];
  size_t off = 16;
  for (int i = 0; i < job->nterms; i++) {
    terms[i] = job->terms[i];
    terms[i].p = S.d + off;
    PLK_HIP(hipMemcpy(S.d + off, job->terms[i].p, terms[i].len, hipMemcpyHostToDevice));
    off += plk_pad16(terms[i].len);
  }
  plk_lc_job_t dj = *job;
  dj.terms = terms;
  dj.out = S.d + o_out;
  uint32_t nz = 0;
  if ((rc = launch_jobs(&dj, 1, (uint32_t*)S.d, nullptr))) return rc;
  PLK_HIP(hipMemcpy(job->out, S.d + o_out, L, hipMemcpyDeviceToHost));
  PLK_HIP(hipMemcpy(&nz, S.d, sizeof nz, hipMemcpyDeviceToHost));
  *out_len = nz ? nz : 1;
  return PLK_OK;
}

}  // extern "C"
