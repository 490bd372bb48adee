// Batched pairings and KZG opening verification (include/plonkhip.h, "Pairings and KZG verification").
//
// One lane per job, nothing shared between lanes but the block's table of GF(101) inverses: no
// workspace, no state, no atomics, no cross-lane or cross-block traffic.
//
//   pairing  the reference's pairing(p, q) (src/pairing.h:66-83).  pairing_f(17) unrolls to the fixed
//            schedule r = 2, 4, 8, 16, 17; the multiples it asks g1_mul for are 2^k p, which for every
//            valid encoding are k repeated g1_doubles, so one chain p, 2p, 4p, 8p, 16p serves the loop:
//              f <- f^2 * line(2^k p, g1_double(g1_neg(2^k p)))(q)     k = 0 .. 3
//              f <- f   * line(16 p, p)(q)
//            and the final power 600 = (101^2 - 1) / 17 is gtp_pow's >= 101 branch, conj(f^5) * f^95.
//            The formulas are applied blindly, as the reference applies them: no curve test, no subgroup
//            test, and line() reads x and y whatever the flag says.
//   verify   L = C - y G + z W built with the raw g1_mul / g1_neg / g1_add in the order the header
//            fixes, then pairing(L, [1]_2) == pairing(W, [s]_2), all in registers, one byte out
//            (opening_check: the one copy all three verification kernels call).
//   fold     the same check on C = the raw fold of g1_mul(C_i, w_i) over a job's k commitments and
//            y = sum_i w_i y_i: k uniform over the launch, so every lane runs the same k steps.
//   multi    the folded check on (C_0 .. C_{k-1}, W) with proof W' (plonkhip.h, "KZG multi-point openings"):
//            per polynomial the Lagrange value r_i(u) over its point mask and the weight c_i, in GF(17).
//
// The raw G1 formulas, the pairing, the inverse table and the host scaffold are plk_pairing.h's
// (shared with kzg_agg.hip).
#include <algorithm>

#include "plk_hf17.h"
#include "plk_hostcall.h"
#include "plk_internal.h"
#include "plk_pairing.h"

namespace {

using namespace plkpair;

constexpr uint32_t PAIR_MAX_BLOCKS = 2048;   // 8 blocks per CU; larger batches run the grid-stride loop

__global__ __launch_bounds__(PAIR_T) void pairing_kernel(const uint8_t* __restrict__ g1s, const uint8_t* __restrict__ g2s,
                                                        size_t n, uint8_t* __restrict__ out) {
  __shared__ uint32_t invl[GFP];
  stage_inverses(invl);
  const G1Ops G{invl};
  for (size_t i = (size_t)blockIdx.x * PAIR_T + threadIdx.x; i < n; i += (size_t)gridDim.x * PAIR_T) {
    bool ok = true;
    const Pt p = load_g1(g1s + 3 * i, ok);
    uint32_t qx = g2s[2 * i], qy = g2s[2 * i + 1];
    if (qx >= GFP || qy >= GFP) {
      ok = false;
      qx = qy = 0;
    }
    const Gt e = pairing(G, p, qx, qy);
    out[2 * i] = (uint8_t)(ok ? e.a : 0xFFu);
    out[2 * i + 1] = (uint8_t)(ok ? e.b : 0xFFu);
  }
}

// The opening check on (C, y, W, z), y and z < 17: L = C - y G + z W, then pairing(L, [1]_2) == pairing(W, [s]_2).
// 1 or 0; 2 when the job held an invalid byte (ok false).
__device__ __forceinline__ uint32_t opening_check(const G1Ops& G, const VkWords& vk, Pt c, uint32_t y, Pt w, uint32_t z,
                                                  bool ok) {
  const Pt g{vk.gx, vk.gy, vk.ginf};
  Pt l = G.add(c, G.negp(G.mul(g, y)));
  l = G.add(l, G.mul(w, z));
  const Gt lhs = pairing(G, l, vk.h1x, vk.h1y);
  const Gt rhs = pairing(G, w, vk.hsx, vk.hsy);
  return !ok ? 2u : (lhs.a == rhs.a && lhs.b == rhs.b) ? 1u : 0u;
}
// One entry of a folded check: C += g1_mul(C_i, w_i), y = hf_add(y, hf_mul(w_i, y_i)) (w_i, y_i < 17).
__device__ __forceinline__ void fold_entry(const G1Ops& G, Pt& c, uint32_t& y, Pt ci, uint32_t wi, uint32_t yi) {
  c = G.add(c, G.mul(ci, wi));
  y = (y + wi * yi % HFP) % HFP;
}

__global__ __launch_bounds__(PAIR_T) void kzg_verify_kernel(VkWords vk, const uint8_t* __restrict__ commits,
                                                           const uint8_t* __restrict__ zs, const uint8_t* __restrict__ ys,
                                                           const uint8_t* __restrict__ proofs, size_t n,
                                                           uint8_t* __restrict__ okb) {
  __shared__ uint32_t invl[GFP];
  stage_inverses(invl);
  const G1Ops G{invl};
  for (size_t i = (size_t)blockIdx.x * PAIR_T + threadIdx.x; i < n; i += (size_t)gridDim.x * PAIR_T) {
    bool ok = true;
    const Pt c = load_g1(commits + 3 * i, ok);
    const Pt w = load_g1(proofs + 3 * i, ok);
    uint32_t z = zs[i], y = ys[i];
    if (z >= HFP || y >= HFP) {
      ok = false;
      z = y = 0;
    }
    okb[i] = (uint8_t)opening_check(G, vk, c, y, w, z, ok);
  }
}

// Folded verification, job i: C = the fold of its k commitments under its k weights and y = the fold
// of its k values, built with the raw g1_mul / g1_add from the identity in entry order (as
// srs_eval_at_s folds), then the check of kzg_verify_kernel.  k is uniform over the launch, so the
// loop's trip count is the same in every lane.
__global__ __launch_bounds__(PAIR_T) void kzg_verify_fold_kernel(VkWords vk, uint32_t k, const uint8_t* __restrict__ commits,
                                                                const uint8_t* __restrict__ weights,
                                                                const uint8_t* __restrict__ ys, const uint8_t* __restrict__ zs,
                                                                const uint8_t* __restrict__ proofs, size_t n,
                                                                uint8_t* __restrict__ okb) {
  __shared__ uint32_t invl[GFP];
  stage_inverses(invl);
  const G1Ops G{invl};
  for (size_t i = (size_t)blockIdx.x * PAIR_T + threadIdx.x; i < n; i += (size_t)gridDim.x * PAIR_T) {
    bool ok = true;
    Pt c{0, 0, 1};
    uint32_t y = 0;
    for (uint32_t j = 0; j < k; j++) {
      const size_t e = i * k + j;
      const Pt ci = load_g1(commits + 3 * e, ok);
      uint32_t wi = weights[e], yi = ys[e];
      if (wi >= HFP || yi >= HFP) {
        ok = false;
        wi = yi = 0;
      }
      fold_entry(G, c, y, ci, wi, yi);
    }
    const Pt w = load_g1(proofs + 3 * i, ok);
    uint32_t z = zs[i];
    if (z >= HFP) {
      ok = false;
      z = 0;
    }
    okb[i] = (uint8_t)opening_check(G, vk, c, y, w, z, ok);
  }
}

// Multi-point verification (plonkhip.h, "KZG multi-point openings"), job i: per polynomial the Lagrange
// value r_j(u) from the claimed evaluations over its mask and the coefficient c_j, then the folded check on
// the k + 1 entries (C_0 .. C_{k-1}, W) with proof W'.  k is uniform over the launch; the masks are per lane.
constexpr uint32_t SET_BITS = 17, SET_FULL = (1u << SET_BITS) - 1;
// prod_{b in m} (x - b) mod 17 (x < 17)
__device__ __forceinline__ uint32_t vanish_at(uint32_t m, uint32_t x) {
  uint32_t r = 1;
  for (uint32_t b = 0; b < SET_BITS; b++)
    if ((m >> b) & 1u) r = hf17::mod17(r * (x + HFP - b));   // (<= 16 x 33)
  return r;
}
__device__ __forceinline__ uint32_t load_set(const uint32_t* sets, size_t e, bool& ok) {
  const uint32_t m = sets[e];
  const bool v = m != 0 && (m & ~SET_FULL) == 0 && m != SET_FULL;
  ok = ok && v;
  return v ? m : 1u;
}
__global__ __launch_bounds__(PAIR_T) void kzg_verify_multi_kernel(VkWords vk, uint32_t k, const uint8_t* __restrict__ commits,
                                                                 const uint32_t* __restrict__ sets,
                                                                 const uint8_t* __restrict__ weights,
                                                                 const uint8_t* __restrict__ ys, const uint8_t* __restrict__ us,
                                                                 const uint8_t* __restrict__ proofs, size_t n,
                                                                 uint8_t* __restrict__ okb) {
  __shared__ uint32_t invl[GFP];
  stage_inverses(invl);
  const G1Ops G{invl};
  for (size_t i = (size_t)blockIdx.x * PAIR_T + threadIdx.x; i < n; i += (size_t)gridDim.x * PAIR_T) {
    bool ok = true;
    uint32_t u = us[i];
    if (u >= HFP) {
      ok = false;
      u = 0;
    }
    uint32_t T = 0;
    for (uint32_t j = 0; j < k; j++) T |= load_set(sets, i * k + j, ok);
    Pt c{0, 0, 1};
    uint32_t y = 0;
    for (uint32_t j = 0; j < k; j++) {
      const size_t e = i * k + j;
      const Pt ci = load_g1(commits + 3 * e, ok);
      const uint32_t m = load_set(sets, e, ok);
      uint32_t wi = weights[e];
      if (wi >= HFP) {
        ok = false;
        wi = 0;
      }
      uint32_t r = 0;
      for (uint32_t a = 0; a < SET_BITS; a++) {
        if (!((m >> a) & 1u)) continue;
        uint32_t ya = ys[SET_BITS * e + a];
        if (ya >= HFP) {
          ok = false;
          ya = 0;
        }
        const uint32_t rest = m & ~(1u << a);
        const uint32_t l = hf17::mod17(vanish_at(rest, u) * hf17::inv_canon(vanish_at(rest, a)));   // the Lagrange basis at u
        r += hf17::mod17(ya * l);
      }
      fold_entry(G, c, y, ci, hf17::mod17(wi * vanish_at(T & ~m, u)), hf17::mod17(r));   // (r <= 16 x 16)
    }
    const Pt w = load_g1(proofs + 6 * i, ok);
    const Pt wp = load_g1(proofs + 6 * i + 3, ok);
    fold_entry(G, c, y, w, hf17::neg(vanish_at(T, u)), 0u);
    okb[i] = (uint8_t)opening_check(G, vk, c, y, wp, u, ok);
  }
}

uint32_t blocks_for(size_t n) { return (uint32_t)std::min<size_t>((n + PAIR_T - 1) / PAIR_T, PAIR_MAX_BLOCKS); }

// folded and multi-point verification: k in 1 .. kmax, then the pointers and n, the key, n k <= 2^30
int check_fold_verify(const char* fn, const plk_kzg_vk_t* vk, int k, bool null_arg, size_t n, VkWords* w,
                      int kmax = PLK_KZG_FOLD_MAX) {
  if (k < 1 || k > kmax) {
    plk_set_error("%s: k = %d is outside 1 .. %d", fn, k, kmax);
    return PLK_ERR_ARG;
  }
  int rc = check_n(fn, !vk || null_arg, n);
  if (rc || (rc = check_vk(fn, vk, w))) return rc;
  if (n > PAIR_MAX_N / (size_t)k) {
    plk_set_error("%s: n k = %zu x %d exceeds 2^30 entries per call", fn, n, k);
    return PLK_ERR_RANGE;
  }
  return PLK_OK;
}

}  // namespace

extern "C" {

int plk_pairing_batch_dev(const uint8_t* d_g1s, const uint8_t* d_g2s, size_t n, uint8_t* d_out_gt, void* stream) {
  const char* fn = "plk_pairing_batch_dev";
  int rc = check_n(fn, !d_g1s || !d_g2s || !d_out_gt, n);
  if (rc || (rc = check_range(fn, n)) || (rc = plk_use_device())) return rc;
  hipLaunchKernelGGL(pairing_kernel, dim3(blocks_for(n)), dim3(PAIR_T), 0, (hipStream_t)stream, d_g1s, d_g2s, n, d_out_gt);
  PLK_HIP(hipGetLastError());
  return PLK_OK;
}

int plk_kzg_verify_batch_dev(const plk_kzg_vk_t* vk, const uint8_t* d_commits3, const uint8_t* d_zs, const uint8_t* d_ys,
                             const uint8_t* d_proofs3, size_t n, uint8_t* d_ok, void* stream) {
  const char* fn = "plk_kzg_verify_batch_dev";
  VkWords w;
  int rc = check_n(fn, !vk || !d_commits3 || !d_zs || !d_ys || !d_proofs3 || !d_ok, n);
  if (rc || (rc = check_vk(fn, vk, &w)) || (rc = check_range(fn, n)) || (rc = plk_use_device())) return rc;
  hipLaunchKernelGGL(kzg_verify_kernel, dim3(blocks_for(n)), dim3(PAIR_T), 0, (hipStream_t)stream, w, d_commits3, d_zs, d_ys,
                     d_proofs3, n, d_ok);
  PLK_HIP(hipGetLastError());
  return PLK_OK;
}

int plk_pairing_batch(const uint8_t* g1s, const uint8_t* g2s, size_t n, uint8_t* out_gt) {
  const char* fn = "plk_pairing_batch";
  int rc = check_n(fn, !g1s || !g2s || !out_gt, n);
  if (rc || (rc = check_range(fn, n)) || (rc = plk_select_device())) return rc;
  Staged D;
  if ((rc = D.alloc(fn, 3 * n + 2 * n + 2 * n))) return rc;
  uint8_t *g1 = D.add(g1s, 3 * n), *g2 = D.add(g2s, 2 * n), *out = D.add(nullptr, 2 * n);
  if ((rc = D.rc) || (rc = plk_pairing_batch_dev(g1, g2, n, out, nullptr))) return rc;
  PLK_HIP(hipMemcpy(out_gt, out, 2 * n, hipMemcpyDeviceToHost));
  return PLK_OK;
}

int plk_kzg_verify_batch(const plk_kzg_vk_t* vk, const uint8_t* commits3, const uint8_t* zs, const uint8_t* ys,
                         const uint8_t* proofs3, size_t n, uint8_t* ok) {
  const char* fn = "plk_kzg_verify_batch";
  VkWords w;
  int rc = check_n(fn, !vk || !commits3 || !zs || !ys || !proofs3 || !ok, n);
  if (rc || (rc = check_vk(fn, vk, &w)) || (rc = check_range(fn, n)) || (rc = plk_select_device())) return rc;
  Staged D;
  if ((rc = D.alloc(fn, 3 * n + 3 * n + n + n + n))) return rc;
  uint8_t *c = D.add(commits3, 3 * n), *p = D.add(proofs3, 3 * n), *z = D.add(zs, n), *y = D.add(ys, n), *o = D.add(nullptr, n);
  if ((rc = D.rc) || (rc = plk_kzg_verify_batch_dev(vk, c, z, y, p, n, o, nullptr))) return rc;
  PLK_HIP(hipMemcpy(ok, o, n, hipMemcpyDeviceToHost));
  return PLK_OK;
}

int plk_kzg_verify_fold_batch_dev(const plk_kzg_vk_t* vk, int k, const uint8_t* d_commits3, const uint8_t* d_weights,
                                  const uint8_t* d_ys, const uint8_t* d_zs, const uint8_t* d_proofs3, size_t n, uint8_t* d_ok,
                                  void* stream) {
  const char* fn = "plk_kzg_verify_fold_batch_dev";
  VkWords w;
  int rc = check_fold_verify(fn, vk, k, !d_commits3 || !d_weights || !d_ys || !d_zs || !d_proofs3 || !d_ok, n, &w);
  if (rc || (rc = plk_use_device())) return rc;
  hipLaunchKernelGGL(kzg_verify_fold_kernel, dim3(blocks_for(n)), dim3(PAIR_T), 0, (hipStream_t)stream, w, (uint32_t)k,
                     d_commits3, d_weights, d_ys, d_zs, d_proofs3, n, d_ok);
  PLK_HIP(hipGetLastError());
  return PLK_OK;
}

int plk_kzg_verify_fold_batch(const plk_kzg_vk_t* vk, int k, const uint8_t* commits3, const uint8_t* weights,
                              const uint8_t* ys, const uint8_t* zs, const uint8_t* proofs3, size_t n, uint8_t* ok) {
  const char* fn = "plk_kzg_verify_fold_batch";
  VkWords w;
  int rc = check_fold_verify(fn, vk, k, !commits3 || !weights || !ys || !zs || !proofs3 || !ok, n, &w);
  if (rc || (rc = plk_select_device())) return rc;
  const size_t e = n * (size_t)k;   // entries
  Staged D;
  if ((rc = D.alloc(fn, 3 * e + e + e + 3 * n + n + n))) return rc;
  uint8_t *c = D.add(commits3, 3 * e), *wt = D.add(weights, e), *y = D.add(ys, e), *p = D.add(proofs3, 3 * n),
          *z = D.add(zs, n), *o = D.add(nullptr, n);
  if ((rc = D.rc) || (rc = plk_kzg_verify_fold_batch_dev(vk, k, c, wt, y, z, p, n, o, nullptr))) return rc;
  PLK_HIP(hipMemcpy(ok, o, n, hipMemcpyDeviceToHost));
  return PLK_OK;
}

int plk_kzg_verify_multi_batch_dev(const plk_kzg_vk_t* vk, int k, const uint8_t* d_commits3, const uint32_t* d_sets,
                                   const uint8_t* d_weights, const uint8_t* d_ys, const uint8_t* d_us, const uint8_t* d_proofs6,
                                   size_t n, uint8_t* d_ok, void* stream) {
  const char* fn = "plk_kzg_verify_multi_batch_dev";
  VkWords w;
  int rc = check_fold_verify(fn, vk, k, !d_commits3 || !d_sets || !d_weights || !d_ys || !d_us || !d_proofs6 || !d_ok, n, &w,
                             PLK_KZG_MULTI_MAX);
  if (rc) return rc;
  if ((uintptr_t)d_sets % 4) {
    plk_set_error("%s: d_sets must be 4-byte aligned", fn);
    return PLK_ERR_ARG;
  }
  if ((rc = plk_use_device())) return rc;
  hipLaunchKernelGGL(kzg_verify_multi_kernel, dim3(blocks_for(n)), dim3(PAIR_T), 0, (hipStream_t)stream, w, (uint32_t)k,
                     d_commits3, d_sets, d_weights, d_ys, d_us, d_proofs6, n, d_ok);
  PLK_HIP(hipGetLastError());
  return PLK_OK;
}

int plk_kzg_verify_multi_batch(const plk_kzg_vk_t* vk, int k, const uint8_t* commits3, const uint32_t* sets,
                               const uint8_t* weights, const uint8_t* ys, const uint8_t* us, const uint8_t* proofs6, size_t n,
                               uint8_t* ok) {
  const char* fn = "plk_kzg_verify_multi_batch";
  VkWords w;
  int rc = check_fold_verify(fn, vk, k, !commits3 || !sets || !weights || !ys || !us || !proofs6 || !ok, n, &w, PLK_KZG_MULTI_MAX);
  if (rc || (rc = plk_select_device())) return rc;
  const size_t e = n * (size_t)k;   // entries
  Staged D;
  if ((rc = D.alloc(fn, 4 * e + 3 * e + e + SET_BITS * e + 6 * n + n + n))) return rc;
  uint8_t *m = D.add(sets, 4 * e, 4), *c = D.add(commits3, 3 * e), *wt = D.add(weights, e), *y = D.add(ys, SET_BITS * e),
          *p = D.add(proofs6, 6 * n), *u = D.add(us, n), *o = D.add(nullptr, n);
  if ((rc = D.rc) || (rc = plk_kzg_verify_multi_batch_dev(vk, k, c, (const uint32_t*)m, wt, y, u, p, n, o, nullptr))) return rc;
  PLK_HIP(hipMemcpy(ok, o, n, hipMemcpyDeviceToHost));
  return PLK_OK;
}

}  // extern "C"
