// Batched small-circuit prover: many whole plonk_prove runs (src/plonk.h:223-656) in ONE launch.
//
// For n <= PLK_PROVE_BATCH_MAX_N gates no polynomial of a proof exceeds 4n + 6 <= 70 coefficients,
// so one wave holds a whole proof: its polynomials live in that wave's slice of LDS (bytes, one
// coefficient per lane, two per lane where a polynomial passes 64 coefficients: the t(x) numerator
// at n = 15, 16), products are schoolbook (lane j sums a[i] b[j - i]), the division by Z_H is the
// reference's long-division loop (src/poly.h:124-177) with the numerator in registers and one
// broadcast per step, the divisions by x - z and x - z omega are a Horner walk from the top per
// lane, and a commitment is sum coeff * log(SRS point) mod 102 by a wave reduction and one EXP
// lookup (the discrete-log MSM of msm.hip; a regular SRS only).  A block is four such waves; the
// prover's tables (h | k1_h | k2_h, h_pows_inv, Z_H, the SRS logs, the EXP words) are loaded into
// LDS once per block and a wave walks the batch with a grid stride.
//
// The reference's exits are decided here, in check_status's order (prove.hip), from the trimmed
// lengths and remainders: a wave that finds one writes the entry's status word and 34 zero bytes
// and goes on to its next entry.  No global scratch, no atomics, no wave waits for another (the
// one __syncthreads follows the table load, before any entry), and every loop's trip count is a
// function of n, Z_H's length and the batch alone.
#include <algorithm>

#include "plk_device.h"
#include "plk_hf17.h"
#include "plk_internal.h"

namespace {

constexpr uint32_t HFP = hf17::P;
using hf17::mod17;   // every call site's bound is noted
constexpr int PB_WAVES = 4;        // proofs in flight per block
constexpr int PB_T = PB_WAVES * PLK_WAVE;
constexpr int NMAX = PLK_PROVE_BATCH_MAX_N;
static_assert(NMAX == 16, "rows of 16: the (vector, row) passes split an index by >> 4 and & 15");
constexpr int PL = 72;             // bytes of a long polynomial: lanes 0..63 and 64..71 (4n + 6 <= 70)
constexpr int PS = 20;             // a_x b_x c_x z_x and their round-3 factors: at most n + 3 = 19
constexpr int PM = 36;             // products of two of those, w(x): at most 2n + 3 = 35
constexpr int NLOG = 2 * NMAX + 4; // SRS logs kept: min(srs_len, 2n + 3)

#define NEW_PHASE(lane) asm volatile("" : "+v"(lane))

// The lanes of a wave run in lockstep and its LDS operations complete in order; this keeps the
// compiler from moving one lane's LDS store past another lane's later load.
__device__ __forceinline__ void wsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct BlockTabs {
  uint32_t exp_words[PLK_GROUP_ORDER];   // {x, y, infinite, 0}
  uint8_t hinvm[NMAX * NMAX];            // h_pows_inv, row-major [r * n + c]
  uint8_t h3[3 * NMAX];                  // h | k1_h | k2_h
  uint8_t zh[NMAX + 4];
  uint8_t logs[NLOG];
};

struct WaveMem {
  uint8_t cir[14 * NMAX];        // the circuit bytes (prove_batch)
  uint8_t vals[11][NMAX];        // a b c q_o q_m q_l q_r q_c sigma1 sigma2 sigma3 over H
  uint8_t in[13][NMAX];          // f_a f_b f_c q_o q_m q_l q_r q_c s1 s2 s3 acc_x l_1_x, zero padded
  uint8_t ev[3][NMAX];           // s_sigma_k(omega^j)
  uint8_t ratio[NMAX];           // the grand product's factors
  uint8_t A[PS], B[PS], C[PS], Z[PS], ZW[PS];
  uint8_t A2[PS], B2[PS], C2[PS], A3[PS], B3[PS], C3[PS], Z1[PS];
  uint8_t AB[PM], T2a[PM], T2b[PM], T3a[PM], T3b[PM], P3[PM], W[PM], Q[PM];
  uint8_t TX[PL];
  uint8_t proof[36];
};
static_assert(sizeof(WaveMem) <= 5 * 1024, "at most 5 KiB of LDS per wave (32 waves per CU)");

enum { IN_FA, IN_FB, IN_FC, IN_QO, IN_QM, IN_QL, IN_QR, IN_QC, IN_S1, IN_S2, IN_S3, IN_ACC, IN_L1 };
enum { X_GATE = 1, X_COPY, X_SRS, X_ACC, X_REM_T, X_SLICE, X_REM_W1, X_REM_W2, X_INPUT };

__device__ __forceinline__ uint32_t exit_word(int kind, uint32_t gate = 0) {
  const uint32_t code = (kind == X_SRS || kind == X_SLICE) ? PLK_ERR_RANGE : PLK_ERR_ARG;
  return code | ((uint32_t)kind << 8) | (gate << 16);
}

// (a * b)[c] added into s for this lane's coefficient c (unreduced: at most min(la, lb) * 256 per call)
__device__ __forceinline__ void conv1(const uint8_t* a, int la, const uint8_t* b, int lb, int c, uint32_t& s) {
#pragma unroll 1
  for (int i = 0; i < la; i++) {
    const uint32_t j = (uint32_t)(c - i);
    const uint32_t bv = j < (uint32_t)lb ? b[j] : 0u;
    s += a[i] * bv;
  }
}
__device__ __forceinline__ void conv2(const uint8_t* a, int la, const uint8_t* b, int lb, int lane, uint32_t& s0,
                                      uint32_t& s1) {
#pragma unroll 1
  for (int i = 0; i < la; i++) {
    const uint32_t ai = a[i];
    const uint32_t j0 = (uint32_t)(lane - i), j1 = j0 + 64u;
    s0 += ai * (j0 < (uint32_t)lb ? b[j0] : 0u);
    s1 += ai * (j1 < (uint32_t)lb ? b[j1] : 0u);
  }
}
// out[0, PS or PM) = a * b, one coefficient per lane (la + lb - 1 <= 64); zero past the product
__device__ __forceinline__ void mul_store(const uint8_t* a, int la, const uint8_t* b, int lb, uint8_t* out, int cap,
                                          int lane) {
  uint32_t s = 0;
  conv1(a, la, b, lb, lane, s);   // <= 19 * 256
  if (lane < cap) out[lane] = (uint8_t)mod17(s);
}

// trimmed length (poly_new_internal, src/poly.h:20-38: at least 1) of the polynomial whose coefficient
// `lane` is v (0 in the lanes past its upper bound)
__device__ __forceinline__ uint32_t trimmed(uint32_t v) {
  const unsigned long long bal = __ballot(v != 0);
  return bal ? 64u - (uint32_t)__builtin_clzll(bal) : 1u;
}

// srs_eval_at_s (src/srs.h:53-68) over the log form: the point's 3 bytes as EXP word
__device__ __forceinline__ uint32_t commit(const BlockTabs& T, uint32_t coeff, int lane, int nlog) {
  const uint32_t lg = lane < nlog ? T.logs[lane] : 0u;
  const uint32_t s = plk_wave_sum(coeff * lg);   // <= 64 * 16 * 101
  return T.exp_words[s % PLK_GROUP_ORDER];
}
__device__ __forceinline__ void put_point(WaveMem& M, int slot, uint32_t w, int lane) {
  if (lane < 3) M.proof[3 * slot + lane] = (uint8_t)(w >> (8 * lane));
}

}  // namespace

// (8 waves per SIMD: at most 64 VGPRs)
__global__ __launch_bounds__(PB_T, 8) void prove_batch_kernel(PlkProveBatch a) {
  __shared__ BlockTabs T;
  __shared__ WaveMem WM[PB_WAVES];
  const int t = threadIdx.x, lane0 = t & 63, wv = t >> 6;
  const int n = (int)a.n, lz = (int)a.lz;
  // ---- the prover's tables, once per block
  for (int i = t; i < PLK_GROUP_ORDER; i += PB_T) T.exp_words[i] = a.exp_words[i];
  for (int i = t; i < NMAX * NMAX; i += PB_T) T.hinvm[i] = a.circuit && i < n * n ? (uint8_t)(a.hinv[i] % HFP) : 0;
  for (int i = t; i < 3 * NMAX; i += PB_T) T.h3[i] = a.circuit && i < 3 * n ? (uint8_t)(a.h3[i] % HFP) : 0;
  for (int i = t; i < NMAX + 4; i += PB_T) T.zh[i] = i < lz ? a.zh[i] : 0;
  const int nlog = (int)min(a.srs_len, (uint64_t)(2 * n + 3));
  for (int i = t; i < NLOG; i += PB_T) T.logs[i] = i < nlog ? a.srs_log[i] : 0;
  __syncthreads();
  WaveMem& M = WM[wv];
  // upper-bound lengths (prove.hip lens_for)
  const int la = max(lz + 1, n), lzx = max(lz + 2, n);
  const int lab = 2 * la - 1, l2b = la + lzx - 1, lnum = 3 * la + lzx - 3;
  const int ltx = lnum - lz + 1, part = n + 2;
  const int llo = min(part, ltx), lmid = ltx > part ? min(part, ltx - part) : 0, lhi = ltx > 2 * part ? ltx - 2 * part : 0;
  const int lr3 = lzx + n - 1;
  const int lw = max(max(part, max(lhi, 1)), max(max(n, lzx), max(lr3, la)));
  const int lwq = lw - 1, lwo = lzx - 1;
  const uint32_t invlead = hf17::inv_canon(T.zh[lz - 1]);
  const uint64_t srs_len = a.srs_len;

  for (uint32_t e = blockIdx.x * PB_WAVES + wv; e < a.batch; e += gridDim.x * PB_WAVES) {
    uint32_t st = 0;
    uint32_t accw = 1;
    // Register budget (64 VGPRs: all 32 wave slots of a CU): the lane index is made opaque per entry and
    // per phase (NEW_PHASE), so the per-lane LDS addresses derived from it are recomputed where they are
    // used instead of being kept live across the whole entry loop, and the convolution loops are not
    // unrolled; what a later phase needs of an earlier one it reloads from LDS.
    int lane = lane0;
    NEW_PHASE(lane);
    if (a.circuit) {
      // ---- stage A: constraints_satisfy, copy_constraints_to_roots, interpolations, grand product
      const uint8_t* cir = a.in + (uint64_t)e * 14u * (uint32_t)n;
      for (int i = lane; i < 14 * n; i += 64) {
        const uint32_t b = cir[i];
        M.cir[i] = (uint8_t)((i >= 5 * n && i < 11 * n) ? b : b % HFP);   // HF values reduced, copies raw
      }
      wsync();
      uint32_t bad = 0;
      if (lane < n) {
        const uint32_t qm = M.cir[lane], ql = M.cir[n + lane], qr = M.cir[2 * n + lane], qo = M.cir[3 * n + lane],
                       qc = M.cir[4 * n + lane];
        const uint32_t wa = M.cir[11 * n + lane], wb = M.cir[12 * n + lane], wc = M.cir[13 * n + lane];
        bad = mod17(ql * wa + qr * wb + qo * wc + qm * mod17(wa * wb) + qc);   // <= 4 * 256 + 16
        M.vals[0][lane] = (uint8_t)wa; M.vals[1][lane] = (uint8_t)wb; M.vals[2][lane] = (uint8_t)wc;
        M.vals[3][lane] = (uint8_t)qo; M.vals[4][lane] = (uint8_t)qm; M.vals[5][lane] = (uint8_t)ql;
        M.vals[6][lane] = (uint8_t)qr; M.vals[7][lane] = (uint8_t)qc;
      }
      const unsigned long long gbal = __ballot(bad != 0);
      uint32_t cbad = 0;
      if (lane < 3 * n) {
        const int k = lane / n, i = lane - k * n;
        const uint32_t type = M.cir[5 * n + 2 * lane], idx = M.cir[5 * n + 2 * lane + 1];
        uint8_t s = 0;
        if (type > 2 || idx == 0 || idx > (uint32_t)n) cbad = 1;
        else s = T.h3[type * n + (idx - 1)];
        M.vals[8 + k][i] = s;
      }
      const unsigned long long cbal = __ballot(cbad != 0);
      if (gbal) st = exit_word(X_GATE, (uint32_t)__builtin_ctzll(gbal));
      else if (cbal) st = exit_word(X_COPY);
      if (!st) {
        wsync();
        // interpolate_at_h (src/plonk.h:162-195): 11 vectors, one (vector, row) per lane and pass
        for (int it = lane; it < 11 * NMAX; it += 64) {
          const int v = it >> 4, r = it & 15;
          uint32_t s = 0;
          for (int c = 0; c < n; c++) s += T.hinvm[(r < n ? r : 0) * n + c] * M.vals[v][c];   // <= 16 * 256
          M.in[v][r] = r < n ? (uint8_t)mod17(s) : 0;
        }
        if (lane < NMAX) M.in[IN_L1][lane] = lane < n ? T.hinvm[lane * n] : 0;   // interpolate_at_h(e_0)
        wsync();
        // round 2's grand product (src/plonk.h:326-359)
        if (lane < 3 * NMAX) {
          const int k = lane >> 4, j = lane & 15;
          const uint32_t x = hf17::pow_canon(4, (uint32_t)j);
          uint32_t y = 0;
          for (int i = n - 1; i >= 0; i--) y = mod17(y * x + M.in[IN_S1 + k][i]);
          M.ev[k][j] = (uint8_t)y;
        }
        wsync();
        {
          const uint32_t be = a.chals[5 * (uint64_t)e + 1] % HFP, ga = a.chals[5 * (uint64_t)e + 2] % HFP;
          uint32_t r = 1;
          if (lane >= 1 && lane < n) {
            const int j = lane - 1;
            const uint32_t wa = M.vals[0][j], wb = M.vals[1][j], wc = M.vals[2][j], op = hf17::pow_canon(4, (uint32_t)j);
            const uint32_t den = mod17(mod17(mod17(wa + be * op + ga) * mod17(wb + be * mod17(2 * op) + ga)) *
                                      mod17(wc + be * mod17(3 * op) + ga));
            const uint32_t num = mod17(mod17(mod17(wa + be * M.ev[0][j] + ga) * mod17(wb + be * M.ev[1][j] + ga)) *
                                      mod17(wc + be * M.ev[2][j] + ga));
            r = mod17(den * hf17::inv_canon(num));
          }
          if (lane < NMAX) M.ratio[lane] = (uint8_t)r;
          wsync();
          uint32_t acc = 1;
          for (int i = 1; i < n; i++) acc = i <= lane ? mod17(acc * M.ratio[i]) : acc;
          wsync();
          if (lane < NMAX) M.ratio[lane] = lane < n ? (uint8_t)acc : 0;   // acc over H
          wsync();
          uint32_t s = 0;
          if (lane < NMAX)
            for (int c = 0; c < n; c++) s += T.hinvm[(lane < n ? lane : 0) * n + c] * M.ratio[c];
          const uint32_t ax = lane < n ? mod17(s) : 0;
          if (lane < NMAX) M.in[IN_ACC][lane] = (uint8_t)ax;
          // acc_x(omega^n) must be 1 (src/plonk.h:366-368)
          accw = mod17(plk_wave_sum(ax * hf17::pow_canon(hf17::pow_canon(4, (uint32_t)n), (uint32_t)lane & 15u)));   // <= 16 * 256
        }
      }
    } else {
      const uint8_t* pl = a.in + (uint64_t)e * 13u * (uint32_t)n;
      uint32_t big = 0;
      for (int it = lane; it < 13 * NMAX; it += 64) {
        const int v = it >> 4, r = it & 15;
        const uint32_t b = r < n ? pl[v * n + r] : 0;
        big |= b >= HFP;
        M.in[v][r] = (uint8_t)b;
      }
      if (__ballot(big != 0)) st = exit_word(X_INPUT);
    }
    if (!st) {
      wsync();
      const uint8_t* ch = a.chals + 5 * (uint64_t)e;
      const uint8_t* rd = a.rands + 9 * (uint64_t)e;
      const uint32_t al = ch[0] % HFP, be = ch[1] % HFP, ga = ch[2] % HFP, z = ch[3] % HFP, v = ch[4] % HFP;
      uint32_t b[9];
      for (int i = 0; i < 9; i++) b[i] = rd[i] % HFP;
      const uint32_t al2 = mod17(al * al), bk1 = mod17(be * 2), bk2 = mod17(be * 3);
      // ---- rounds 1-2: a_x = (b2 + b1 x) Z_H + f_a, ..., z_x = (b9 + b8 x + b7 x^2) Z_H + acc_x
      const uint32_t zh0 = lane < lz ? T.zh[lane] : 0, zh1 = lane >= 1 && lane - 1 < lz ? T.zh[lane - 1] : 0,
                     zh2 = lane >= 2 && lane - 2 < lz ? T.zh[lane - 2] : 0;
      const uint32_t inl = lane < n ? 1u : 0u;
      const int li = lane < NMAX ? lane : 0;
      const uint32_t ax = lane < la ? mod17(b[1] * zh0 + b[0] * zh1 + inl * M.in[IN_FA][li]) : 0;
      const uint32_t bx = lane < la ? mod17(b[3] * zh0 + b[2] * zh1 + inl * M.in[IN_FB][li]) : 0;
      const uint32_t cx = lane < la ? mod17(b[5] * zh0 + b[4] * zh1 + inl * M.in[IN_FC][li]) : 0;
      const uint32_t zx = lane < lzx ? mod17(b[8] * zh0 + b[7] * zh1 + b[6] * zh2 + inl * M.in[IN_ACC][li]) : 0;
      const uint32_t s1 = inl * M.in[IN_S1][li], s2 = inl * M.in[IN_S2][li], s3 = inl * M.in[IN_S3][li];
      const uint32_t c0 = lane == 0, c1 = lane == 1;
      if (lane < PS) {
        M.A[lane] = (uint8_t)ax; M.B[lane] = (uint8_t)bx; M.C[lane] = (uint8_t)cx; M.Z[lane] = (uint8_t)zx;
        // round 3's linear factors (src/plonk.h:409-489)
        M.A2[lane] = (uint8_t)mod17(al * mod17(ax + c0 * ga + c1 * be));
        M.B2[lane] = (uint8_t)mod17(bx + c0 * ga + c1 * bk1);
        M.C2[lane] = (uint8_t)mod17(cx + c0 * ga + c1 * bk2);
        M.A3[lane] = (uint8_t)mod17(al * mod17(ax + be * s1 + c0 * ga));
        M.B3[lane] = (uint8_t)mod17(bx + be * s2 + c0 * ga);
        M.C3[lane] = (uint8_t)mod17(cx + be * s3 + c0 * ga);
        M.ZW[lane] = (uint8_t)mod17(zx * hf17::pow_canon(4, (uint32_t)lane & 15u));   // z(omega x), OMEGA = 4
        M.Z1[lane] = (uint8_t)mod17(al2 * mod17(zx + c0 * 16u));
      }
      const uint32_t la_t = max(max(trimmed(ax), trimmed(bx)), trimmed(cx));
      if (la_t > srs_len) st = exit_word(X_SRS);
      else if (a.circuit && a.strict && accw != 1) st = exit_word(X_ACC);
      else if (trimmed(zx) > srs_len) st = exit_word(X_SRS);
      if (!st) {
        put_point(M, 0, commit(T, ax, lane, nlog), lane);
        put_point(M, 1, commit(T, bx, lane, nlog), lane);
        put_point(M, 2, commit(T, cx, lane, nlog), lane);
        put_point(M, 3, commit(T, zx, lane, nlog), lane);
        wsync();
        NEW_PHASE(lane);
        // ---- round 3: the t(x) numerator (src/plonk.h:386-503), products re-associated as in prove.hip
        mul_store(M.A, la, M.B, la, M.AB, PM, lane);
        mul_store(M.A2, la, M.B2, la, M.T2a, PM, lane);
        mul_store(M.C2, la, M.Z, lzx, M.T2b, PM, lane);
        mul_store(M.A3, la, M.B3, la, M.T3a, PM, lane);
        mul_store(M.C3, la, M.ZW, lzx, M.T3b, PM, lane);
        mul_store(M.Z, lzx, M.in[IN_S3], n, M.P3, PM, lane);
        wsync();
        uint32_t p0 = 0, p1 = 0, m0 = 0, m1 = 0;
        conv2(M.in[IN_QM], n, M.AB, lab, lane, p0, p1);          // (a b) q_m         <= 16 * 256 each
        conv2(M.in[IN_QL], n, M.A, la, lane, p0, p1);            // a q_l
        conv2(M.in[IN_QR], n, M.B, la, lane, p0, p1);            // b q_r
        conv2(M.in[IN_QO], n, M.C, la, lane, p0, p1);            // c q_o
        conv2(M.in[IN_L1], n, M.Z1, lzx, lane, p0, p1);          // alpha^2 (z - 1) l_1
        conv2(M.T2a, lab, M.T2b, l2b, lane, p0, p1);             // t_2               <= 35 * 256
        conv2(M.T3a, lab, M.T3b, l2b, lane, m0, m1);             // t_3               <= 35 * 256
        p0 += inl * M.in[IN_QC][li];                             // total <= 5 * 4096 + 8960 + 16 + 16 < 69632
        uint32_t r0 = mod17(p0 + hf17::neg(mod17(m0))), r1 = mod17(p1 + hf17::neg(mod17(m1)));
        if (lane + 64 >= lnum) r1 = 0;
        // ---- t(x) = numerator / Z_H: the reference's loop, one quotient coefficient per step
        uint32_t q0 = 0;   // (ltx <= 4n - 4 = 60 coefficients: one per lane)
#pragma unroll 1
        for (int k = ltx - 1; k >= 0; k--) {
          const int idx = k + lz - 1;
          const uint32_t top = (uint32_t)__shfl((int)(idx < 64 ? r0 : r1), idx & 63, 64);
          const uint32_t q = mod17(top * invlead);
          if (lane == k) q0 = q;
          const uint32_t d0 = (uint32_t)(lane - k), d1 = d0 + 64u;
          const uint32_t nq = hf17::neg(q);
          r0 = mod17(r0 + nq * (d0 < (uint32_t)lz ? T.zh[d0] : 0u));
          r1 = mod17(r1 + nq * (d1 < (uint32_t)lz ? T.zh[d1] : 0u));
        }
        const bool rem_t = __ballot((r0 | r1) != 0) != 0;   // what is left is the remainder (degree < lz - 1)
        M.TX[lane] = (uint8_t)q0;
        if (lane < PL - 64) M.TX[64 + lane] = 0;
        const uint32_t txlen = trimmed(q0);
        const uint32_t tlo = lane < llo ? q0 : 0;
        wsync();
        const uint32_t tmid = lane < lmid ? M.TX[part + lane] : 0, thi = lane < lhi ? M.TX[2 * part + lane] : 0;
        if (a.strict && rem_t) st = exit_word(X_REM_T);
        else if (txlen <= 2u * (uint32_t)part) st = exit_word(X_SLICE);
        else if (max(max(trimmed(tlo), trimmed(tmid)), trimmed(thi)) > srs_len) st = exit_word(X_SRS);
        if (!st) {
          put_point(M, 4, commit(T, tlo, lane, nlog), lane);
          put_point(M, 5, commit(T, tmid, lane, nlog), lane);
          put_point(M, 6, commit(T, thi, lane, nlog), lane);
          NEW_PHASE(lane);
          // ---- round 4: evaluations at z (src/plonk.h:527-574); evaluation is a ring homomorphism, so
          // r_z comes from r(x)'s terms (prove.hip scalars_r45)
          const uint32_t zp = hf17::pow_canon(z, (uint32_t)lane);   // z^lane, 0^0 = 1
          auto ev = [&](uint32_t coef) { return mod17(plk_wave_sum(coef * zp)); };   // <= 64 * 256
          const int ls = lane < PS ? lane : 0, li = lane < NMAX ? lane : 0;
          const uint32_t inl = lane < n ? 1u : 0u, c0 = lane == 0;
          const uint32_t ax = lane < la ? M.A[ls] : 0u, bx = lane < la ? M.B[ls] : 0u, cx = lane < la ? M.C[ls] : 0u,
                         zx = lane < lzx ? M.Z[ls] : 0u, zwx = lane < lzx ? M.ZW[ls] : 0u;
          const uint32_t s1 = inl * M.in[IN_S1][li], s2 = inl * M.in[IN_S2][li];
          const uint32_t p3 = lane < lr3 ? M.P3[lane < PM ? lane : 0] : 0;
          const uint32_t qm = inl * M.in[IN_QM][li], ql = inl * M.in[IN_QL][li], qr = inl * M.in[IN_QR][li],
                         qo = inl * M.in[IN_QO][li], l1 = inl * M.in[IN_L1][li];
          const uint32_t az = ev(ax), bz = ev(bx), cz = ev(cx), s1z = ev(s1), s2z = ev(s2), tz = ev(q0), zwz = ev(zwx),
                         l1z = ev(l1);
          const uint32_t abz = mod17(az * bz);
          const uint32_t x1 = mod17(az + be * z + ga), x2 = mod17(bz + mod17(be * 2) * z + ga),
                         x3 = mod17(cz + mod17(be * 3) * z + ga);
          const uint32_t r2 = mod17(mod17(mod17(x1 * x2) * x3) * al);
          const uint32_t r24 = mod17(r2 + mod17(l1z * al2));
          const uint32_t y1 = mod17(az + be * s1z + ga), y2 = mod17(bz + be * s2z + ga);
          const uint32_t r3b = mod17(mod17(mod17(y1 * y2) * al) * mod17(be * zwz));
          // r(x), coefficient `lane` (at most lr3 <= 34 coefficients)
          const uint32_t rx = mod17(abz * qm + az * ql + bz * qr + cz * qo + r24 * zx + r3b * p3);   // <= 6 * 256
          const uint32_t rz = ev(rx);
          // ---- round 5: w_z(x) and w_z_omega(x) (src/plonk.h:580-621)
          const uint32_t zn2 = hf17::pow_canon(z, (uint32_t)n + 2u), z2n4 = hf17::pow_canon(z, 2u * (uint32_t)n + 4u);
          const uint32_t v2 = mod17(v * v), v3 = mod17(v2 * v), v4 = mod17(v3 * v), v5 = mod17(v4 * v), v6 = mod17(v5 * v);
          const uint32_t w0 = mod17(hf17::neg(tz) + v * hf17::neg(rz) + v2 * hf17::neg(az) + v3 * hf17::neg(bz) + v4 * hf17::neg(cz) +
                                   v5 * hf17::neg(s1z) + v6 * hf17::neg(s2z));
          const uint32_t wx = mod17(tlo + zn2 * tmid + z2n4 * thi + v * rx + v2 * ax + v3 * bx + v4 * cx + v5 * s1 +
                                   v6 * s2 + c0 * w0);   // <= 9 * 256 + 32
          const uint32_t zz = mod17(zx + c0 * hf17::neg(zwz));
          if (lane < PM) { M.W[lane] = (uint8_t)wx; M.Q[lane] = (uint8_t)zz; }
          wsync();
          // quotient coefficient `lane` of the division by x - c: sum_{j > lane} p[j] c^(j - lane - 1)
          const uint32_t zo = mod17(z * 4);
          uint32_t wq = 0, wo = 0;
          for (int j = lw - 1; j >= 1; j--) wq = j > lane ? mod17(wq * z + M.W[j]) : wq;
          for (int j = lzx - 1; j >= 1; j--) wo = j > lane ? mod17(wo * zo + M.Q[j]) : wo;
          if (lane >= lwq) wq = 0;
          if (lane >= lwo) wo = 0;
          const uint32_t rem1 = ev(wx);                                        // w(z)
          const uint32_t rem2 = mod17(plk_wave_sum(zz * hf17::pow_canon(zo, (uint32_t)lane)));   // (z_x - z_omega_z)(z omega)
          if (a.strict && rem1) st = exit_word(X_REM_W1);
          else if (a.strict && rem2) st = exit_word(X_REM_W2);
          else if (max(trimmed(wq), trimmed(wo)) > srs_len) st = exit_word(X_SRS);
          if (!st) {
            put_point(M, 7, commit(T, wq, lane, nlog), lane);
            put_point(M, 8, commit(T, wo, lane, nlog), lane);
            if (lane == 0) {
              M.proof[27] = (uint8_t)az; M.proof[28] = (uint8_t)bz; M.proof[29] = (uint8_t)cz;
              M.proof[30] = (uint8_t)s1z; M.proof[31] = (uint8_t)s2z; M.proof[32] = (uint8_t)rz;
              M.proof[33] = (uint8_t)zwz;
            }
          }
        }
      }
    }
    wsync();
    if (lane < 34) a.proofs[34 * (uint64_t)e + lane] = st ? 0 : M.proof[lane];
    if (lane == 0) a.status[e] = st;
    wsync();
  }
}

int plk_prove_batch_launch(const PlkProveBatch* a, hipStream_t st) {
  if (a->n < 1 || a->n > PLK_PROVE_BATCH_MAX_N || a->lz < 2 || a->lz > a->n + 1 || a->batch == 0) {
    plk_set_error("prover not eligible for the fused batch kernel");
    return PLK_ERR_RANGE;
  }
  // 8 blocks of 4 waves per CU fill its 32 wave slots; the rest of the batch by the grid stride
  const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)a->batch + PB_WAVES - 1) / PB_WAVES, 2048);
  hipLaunchKernelGGL(prove_batch_kernel, dim3(blocks), dim3(PB_T), 0, st, *a);
  PLK_HIP(hipGetLastError());
  return PLK_OK;
}
