// The scaffold of an entry point that comes as a host-buffer form and a _dev form: the device
// checks, the call's device scratch and the layout helpers of its one allocation.  One definition
// of each: a feature file includes this header and defines none of them again.
// (Not for msm.hip or the headers it includes: bench.py hashes those.)
#pragma once
#include "plk_internal.h"

// _dev form: the library initialised (PLK_ERR_NODEV without a GPU) and the calling thread on its device
// (PLK_ERR_ARG otherwise: the caller's pointers and stream belong to a device).  The retain is only
// that check -- the kernels read no library table, so nothing is held and it is released at once.
inline int plk_use_device(void) {
  const int rc = plk_ctx_retain();
  if (rc) return rc;
  plk_ctx_release();
  return PLK_OK;
}

// host forms: initialise if need be and make the library's primary device the calling thread's
// current one, as the other host-buffer entry points do
inline int plk_select_device(void) {
  int rc = plk_init(-1), dev = 0;
  if (rc) return rc;
  if (plk_devices(&dev, 1) < 1) {
    plk_set_error("libplonkhip was shut down during the call");
    return PLK_ERR_HIP;
  }
  PLK_HIP(hipSetDevice(dev));
  return PLK_OK;
}

// capi.hip: the 102 meaningful words of the MSM lookup table E (E[y] for y < 101, then E[256]) for a kernel
// outside msm.hip, which cannot see that file's __constant__ copy.  Valid once the library is initialised
// (after plk_use_device / plk_select_device returned PLK_OK); constant from then on.
void plk_group_ytab_words(uint32_t out[102]);

// device scratch of one host-buffer call, released on scope exit (hidden: its members are
// no part of the library's exports)
struct __attribute__((visibility("hidden"))) PlkScratch {
  uint8_t* d = nullptr;
  ~PlkScratch() {
    if (d) (void)hipFree(d);
  }
  int alloc(const char* fn, size_t bytes) {
    if (hipMalloc((void**)&d, bytes) != hipSuccess) {
      d = nullptr;
      plk_set_error("%s: hipMalloc(%zu) failed", fn, bytes);
      return PLK_ERR_NOMEM;
    }
    return PLK_OK;
  }
};

inline size_t plk_pad16(size_t n) { return (n + 15) & ~(size_t)15; }

// bytes from the first element's first byte to the last element's last in a strided run of count
// (>= 1) elements of len bytes; false when that overflows
inline bool plk_span_of(size_t len, size_t stride, size_t count, size_t* out) {
  size_t s = 0;
  if (__builtin_mul_overflow(count - 1, stride, &s) || __builtin_add_overflow(s, len, &s)) return false;
  *out = s;
  return true;
}
