// host_util.h — host-side glue that the entry points of libhcir state the same way: workspace carving, the
// dtype dispatch, the checks every loss makes of its dtype and temperature.
#pragma once
#include <stddef.h>

#include "../../include/hcir.h"

// Cuts one workspace allocation into 256-byte aligned pieces, in the order of the take() calls.  A null base sizes:
// every piece comes back null and `off` ends as the byte count the same calls need.
struct WsCarver {
  char* base;
  size_t off = 0;
  explicit WsCarver(void* b) : base(static_cast<char*>(b)) {}
  void* take(size_t bytes) {
    char* r = base ? base + off : nullptr;
    off += (bytes + 255) & ~size_t(255);
    return r;
  }
  template <typename T>
  T* take(size_t count) {
    return static_cast<T*>(take(count * sizeof(T)));
  }
};

// fn<T>(args...) with T the element type of `dtype`, which hcir_float_dtype_ok() has accepted
#define HCIR_DISPATCH_DTYPE(dtype, fn, ...)           \
  ((dtype) == HCIR_F32   ? fn<float>(__VA_ARGS__)     \
   : (dtype) == HCIR_F16 ? fn<_Float16>(__VA_ARGS__)  \
                         : fn<__bf16>(__VA_ARGS__))

static inline bool hcir_float_dtype_ok(int dtype) {
  return dtype == HCIR_F32 || dtype == HCIR_F16 || dtype == HCIR_BF16;
}
static inline size_t hcir_dtype_bytes(int dtype) { return dtype == HCIR_F32 ? 4 : 2; }
// 1 / T of a contrastive loss: any sign, not 0, not NaN
static inline bool hcir_inv_t_ok(float inv_t) { return inv_t == inv_t && inv_t != 0.f; }
