// ptmi_dbuf.h — DBuf: one device allocation, owned.  Freed when the owner goes (or by release()); moved, never copied.  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>

namespace ptmi {

struct DBuf {
  void* p = nullptr;
  size_t cap = 0;

  DBuf() = default;
  DBuf(DBuf&& o) noexcept : p(o.p), cap(o.cap) {
    o.p = nullptr;
    o.cap = 0;
  }
  DBuf& operator=(DBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      cap = o.cap;
      o.p = nullptr;
      o.cap = 0;
    }
    return *this;
  }
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  ~DBuf() { release(); }

  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    if (bytes == 0) return hipSuccess;
    size_t ask = bytes;
#ifdef PTMI_TEST_HOOKS  // the tests' own build of the library (_build.build_testhooks): pretend the board is smaller — through a hipMalloc that really fails
    if (const char* lim = getenv("PTMI_TEST_ALLOC_LIMIT"))
      if (bytes > strtoull(lim, nullptr, 10)) ask = (size_t)1 << 60;
#endif
    hipError_t e = hipMalloc(&p, ask);
    if (e == hipSuccess) cap = bytes;
    else {
      p = nullptr;
      (void)hipGetLastError();  // the failure is reported through the return value; do not leave it behind as the runtime's "last error"
    }
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};

}  // namespace ptmi
