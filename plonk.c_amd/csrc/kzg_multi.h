// What kzg_multi.hip needs from kzg.hip: the resident SRS and the launcher of the folded opening.
#pragma once
#include "plk_internal.h"

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

// the finish's ticket field: the most coefficients one record's blocks can count (kzg.hip KZG_MAX_LEN)
constexpr uint64_t PLK_KZG_RECORD_MAX_LEN = (8ull * 65535ull) * 4096ull;

// kzg.hip launch_fold: the launches of plk_kzg_open_fold_batch_dev after its argument checks, group g's
// record at d_res + g; row0: the record index of group 0 (the finish's shard spread)
int plk_kzg_fold_launch(const plk_srs* s, const uint8_t* const* d_polys, const size_t* lens, const uint8_t* weights,
                        const int* start, const uint8_t* zs, int ngroups, uint8_t* d_ys, PlkMsmResult* d_res,
                        uint8_t* const* d_quots, uint32_t* d_work, hipStream_t st, uint32_t row0);
