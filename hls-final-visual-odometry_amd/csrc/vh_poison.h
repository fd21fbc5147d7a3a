// vh_poison.h -- the one poison rule (test aid).  VH_POISON=1 in the environment: every device and page-locked buffer the
// library allocates starts as 0xA5 bytes, so that a kernel or a download consuming memory nobody wrote gives the same
// wrong answer on every machine, instead of whatever the allocation's previous owner left there.  Every allocation site
// of csrc/ calls one of the two functions below (tests/test_poisoned_buffers.py keeps the list).  Unset: neither
// function does anything, and neither makes a HIP call.
#ifndef VH_POISON_H
#define VH_POISON_H

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

inline bool vh_poison_on() {
  static const bool on = [] { const char *e = getenv("VH_POISON"); return e && e[0] == '1'; }();  // (read once)
  return on;
}
// a fresh device range (blocking: the buffer's first user may be any stream)
inline hipError_t vh_poison_device(void *q, size_t bytes) {
  if (!vh_poison_on() || !q || !bytes) return hipSuccess;
  const hipError_t e = hipMemset(q, 0xA5, bytes);
  return e != hipSuccess ? e : hipDeviceSynchronize();
}
// fresh page-locked host memory (nothing to wait for: no kernel or copy knows the buffer yet)
inline void vh_poison_host(void *p, size_t bytes) {
  if (vh_poison_on() && p && bytes) memset(p, 0xA5, bytes);
}

#endif
