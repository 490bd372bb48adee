// Host pieces of the KZG opening family (kzg.hip, kzg_multi.hip, kzg_points.hip): the resident SRS, the chunk
// geometry, the argument checks the entry points share and the arena / read-back steps of the host-buffer forms.
// One definition of each: the three files include this header and define none of them again.
// (Not for msm.hip or the headers it includes: bench.py hashes those.)
#pragma once
#include <string.h>

#include <vector>

#include "plk_hostcall.h"
#include "plk_internal.h"
#include "plk_kzg_open.h"

struct plk_srs {
  int dev = 0;
  size_t len = 0;
  bool irregular = false;
  uint8_t* d_g1 = nullptr;    // 3 len bytes (+ 16)
  uint8_t* d_log = nullptr;   // len bytes, zero padded to a multiple of 16 (+ 16); unusable when irregular
  uint32_t* d_flag = nullptr;
  const uint32_t* exp_words = nullptr;
  hipStream_t st = nullptr;   // the host-buffer forms' stream
};

// the most coefficients one record's blocks can count (the finish's ticket field), a block taking one chunk
constexpr uint64_t PLK_KZG_RECORD_MAX_LEN = (8ull * 65535ull) * kzgo::CHUNK;
static inline uint64_t plk_kzg_chunks_of(uint64_t len) { return (len + kzgo::CHUNK - 1) / kzgo::CHUNK; }

// the group layout of a folded or multi-point call: start[0] = 0, strictly increasing, at most kmax a group
static inline bool plk_kzg_layout_ok(const int* start, int ngroups, int kmax) {
  if (!start || ngroups <= 0 || start[0] != 0) return false;
  for (int g = 0; g < ngroups; g++) {
    const long long k = (long long)start[g + 1] - start[g];
    if (k < 1 || k > kmax) return false;
  }
  return true;
}

// The three checks every entry point of the family makes after its own (no device is touched; the handle is
// read last): what: "job" or "polynomial", as the entry point counts its inputs.
static inline int plk_kzg_check_record_len(const char* fn, const char* what, int i, size_t len) {
  if (len <= PLK_KZG_RECORD_MAX_LEN) return PLK_OK;
  plk_set_error("%s: %s %d: %zu coefficients exceed the %llu one record's finish can count", fn, what, i, len,
                (unsigned long long)PLK_KZG_RECORD_MAX_LEN);
  return PLK_ERR_RANGE;
}
// need: the scalars the commitment takes (the reference's text and spelling)
static inline int plk_kzg_check_srs_len(const plk_srs* s, size_t need) {
  if (need <= s->len) return PLK_OK;
  plk_set_error("Poynomial degree exceeds SRS size: POLY degree: %zu, SRS supports up to degree: %zu", need, s->len);
  return PLK_ERR_RANGE;
}
static inline int plk_kzg_check_device(const char* fn, const plk_srs* s) {
  if (plk_cur_device() == s->dev) return PLK_OK;
  plk_set_error("%s: the SRS lives on device %d but the calling thread's current device is %d", fn, s->dev,
                plk_cur_device());
  return PLK_ERR_ARG;
}

// kzg.hip: the launches of plk_kzg_open_fold_batch_dev after its argument checks, as many whole groups as
// fit per launch, consecutive on the stream; group g's record at d_res + g; row0: the record index of
// group 0 (the finish's shard spread)
int plk_kzg_fold_launch(const plk_srs* s, const uint8_t* const* d_polys, const size_t* lens, const uint8_t* weights,
                        const int* start, const uint8_t* zs, int ngroups, uint8_t* d_ys, PlkMsmResult* d_res,
                        uint8_t* const* d_quots, uint32_t* d_work, hipStream_t st, uint32_t row0);

// The arena of a host-buffer form: polynomial i in a slot of plk_pad16(lens[i]) bytes from the start of the
// call's scratch.  The slots' bytes and, when asked for, the longest length; -1, or the index of the first
// NULL polynomial.
static inline int plk_kzg_arena_bytes(const uint8_t* const* polys, const size_t* lens, int n, size_t* bytes,
                                      size_t* maxlen = nullptr) {
  size_t b = 0, m = 0;
  for (int i = 0; i < n; i++) {
    if (!polys[i]) return i;
    if (lens[i] > m) m = lens[i];
    b += plk_pad16(lens[i]);
  }
  *bytes = b;
  if (maxlen) *maxlen = m;
  return -1;
}
// uploads the polynomials into their slots; dp: the device pointers
static inline int plk_kzg_upload(const PlkScratch& S, const uint8_t* const* polys, const size_t* lens, int n,
                                 hipStream_t st, std::vector<const uint8_t*>& dp) {
  dp.resize(n);
  size_t off = 0;
  for (int i = 0; i < n; i++) {
    dp[i] = S.d + off;
    PLK_HIP(hipMemcpyAsync(S.d + off, polys[i], lens[i], hipMemcpyHostToDevice, st));
    off += plk_pad16(lens[i]);
  }
  return PLK_OK;
}
// Waits for the stream, then irr[r] = the flag and out3 + 3 r = the G1 bytes of records [0, n) at d_res
// (the first 32 bytes of each record travel).
static inline int plk_kzg_read_records(const PlkMsmResult* d_res, size_t n, hipStream_t st, uint32_t* irr,
                                       uint8_t* out3) {
  std::vector<uint8_t> h(32 * n);
  PLK_HIP(hipMemcpy2DAsync(h.data(), 32, d_res, sizeof(PlkMsmResult), 32, n, hipMemcpyDeviceToHost, st));
  PLK_HIP(hipStreamSynchronize(st));
  for (size_t r = 0; r < n; r++) {
    const PlkMsmResult* rec = (const PlkMsmResult*)(h.data() + 32 * r);
    irr[r] = rec->irregular;
    memcpy(out3 + 3 * r, rec->g1, 3);
  }
  return PLK_OK;
}
