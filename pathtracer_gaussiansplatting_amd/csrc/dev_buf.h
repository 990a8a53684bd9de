// dev_buf.h — one owning device buffer, grown on demand: what the workspaces of the 3DGS forward pass
// (splat_workspace.h), densify (splat_densify.hip) and the loss (splat_loss.hip) are made of. A workspace that
// holds its buffers as DevBuf members frees them when it is deleted; there is no list to keep beside the struct.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>

namespace ptgs {

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;  // allocated

  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }

  // Keep a buffer of at least `need` bytes, or replace it by one of need + slack (the caller's growth policy). The
  // old buffer is freed before the new one is allocated: the peak is never both, and hipFree waits for the
  // work that still uses the old one. The contents are not kept.
  hipError_t ensure(size_t need, size_t slack) {
    if (bytes >= need) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    const hipError_t e = hipMalloc(&p, need + slack);
    if (e == hipSuccess) bytes = need + slack;
    return e;
  }

  template <typename T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

}  // namespace ptgs
