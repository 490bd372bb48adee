// The conflict-free discrete-log lookup of a G1 encoding, shared by the files that stream points outside
// msm.hip (kzg_agg.hip: the aggregate verification's sums; msm_seg.hip: the segmented MSM).  One definition of
// each: a feature file includes this header and defines none of them again.  Everything is __forceinline__,
// so a kernel's code does not depend on which file it sits in.
// (Not for msm.hip or the headers it includes: bench.py hashes those.)
//
// LOG is msm.hip's lookup d = E[y] - k (the log when the encoding is canonical, >= 256 otherwise) through an
// LDS table of 128 entries in 32 copies (copy = lane mod 32: ds_read_b32 banks are taken mod 32 within each
// 32-lane half, so the gathers are conflict free); the identity, E[256] there, is a select on the flag bit
// instead of a second table region.  The 102 meaningful words of E reach a kernel as an argument
// (plk_group_ytab_words, plk_hostcall.h): no state, no upload.
#pragma once
#include "plk_device.h"

namespace plkg1log {

constexpr int TAB_E = 128, TAB_C = 32;         // LDS table: entries x copies (16 KB)

// the block's lookup table (T threads; Tab: a struct whose w[102] holds E[y], y < 101, then E[256]): entry
// e < 101 is E[e]; the rest never match (a y byte that differs from the index)
template <int T, class Tab>
__device__ __forceinline__ void stage_table(const Tab& t, uint32_t* tab) {
  for (uint32_t i = threadIdx.x; i < TAB_E * TAB_C / 4; i += T) {
    const uint32_t e = i / (TAB_C / 4);
    const uint32_t v = e < (uint32_t)PLK_GF_P ? t.w[e] : ((e ^ 1u) << 16);
    reinterpret_cast<uint4*>(tab)[i] = make_uint4(v, v, v, v);
  }
}

// d = E[idx] - k for the encoded point k = x << 8 | y << 16 | flag << 24: the log (< 102) exactly when the
// encoding is canonical, >= 256 otherwise.  Any byte values are safe: the index is masked to the table.
// lane4 = (threadIdx.x & (TAB_C - 1)) << 2.
__device__ __forceinline__ uint32_t dlog(uint32_t k, const uint32_t* tab, uint32_t lane4) {
  const uint32_t idx = (k >> 16) & (TAB_E - 1u);
  const uint32_t e = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(tab) + ((idx << 7) | lane4));
  return (((k >> 24) & 1u) ? (1u << 24) : e) - k;
}

// Encoded point j (0..15) of 48 point bytes held in w[0..11] (the byte string shifted up by one byte)
template <int J>
__device__ __forceinline__ uint32_t g1_word(const uint32_t (&w)[12]) {
  constexpr int o = 3 * J, d = o >> 2, b = o & 3;
  constexpr int d1 = (b + 2 <= 3) ? d : d + 1;
  // v_perm_b32: selector bytes 0-3 pick from the 2nd operand, 4-7 from the 1st, 0x0C -> 0
  constexpr uint32_t sel = 0x0Cu | ((uint32_t)b << 8) | ((uint32_t)(b + 1) << 16) | ((uint32_t)(b + 2) << 24);
  return __builtin_amdgcn_perm(w[d1], w[d], sel);
}

}  // namespace plkg1log
