// Host-only helpers for the device workspaces of the raster units (polygonize.hip, sieve.hip): one walk over a list
// of arrays both sizes a workspace and binds it, and a clear or copy that fails is reported, not launched on top of.
#pragma once
#include "ffa_common.h"

inline long long ffa_ws_align_up(long long v) { return (v + 255) & ~255ll; }

template <typename T>
T* ffa_ws_at(void* ws, long long off) {
  return reinterpret_cast<T*>(static_cast<char*>(ws) + off);
}

// Bump allocator over a byte range, every array on a 256-byte boundary.  With a null base it only advances: the walk
// that binds the arrays of a workspace is the walk that sizes it (`off` after the last take).
struct ffa_carver {
  void* base;
  long long off = 0;
  template <typename T>
  void take(T*& p, long long count) {
    p = base ? ffa_ws_at<T>(base, off) : nullptr;
    off += ffa_ws_align_up(count * (long long)sizeof(T));
  }
};

// A failed clear would leave stale votes, counts or counters behind, a failed copy stale data under the kernels that
// follow: report it instead of launching on top of it.  `op` is the entry point, `what` names the array.
inline int ffa_zero_async(void* p, long long bytes, const char* op, const char* what, hipStream_t st) {
  const hipError_t e = hipMemsetAsync(p, 0, (size_t)bytes, st);
  if (e != hipSuccess) ffa_set_error("%s: clearing %s failed: %s", op, what, hipGetErrorString(e));
  return (int)e;
}

inline int ffa_copy_async(void* dst, const void* src, long long bytes, const char* op, const char* what, hipStream_t st) {
  const hipError_t e = hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, st);
  if (e != hipSuccess) ffa_set_error("%s: copying %s failed: %s", op, what, hipGetErrorString(e));
  return (int)e;
}

// return the first failure of a chain of such steps
#define FFA_TRY(expr)              \
  do {                             \
    const int ffa_rc_ = (expr);    \
    if (ffa_rc_ != 0) return ffa_rc_; \
  } while (0)
