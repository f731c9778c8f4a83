// ptmi_dbuf.h — DBuf: one device allocation, owned.  Freed when the owner goes (or by release()); moved, never copied.  StagedTable: a small table that every call
// rewrites, uploaded from a pinned host copy.  Host code only.
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
  // ensure() for a buffer that work already on `stream` may still use: where there is one and it has to be reallocated, the stream drains first.
  hipError_t ensure_idle(size_t bytes, hipStream_t stream) {
    if (p && bytes > cap)
      if (hipError_t e = hipStreamSynchronize(stream); e != hipSuccess) return e;
    return ensure(bytes);
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

// A table that kernels read and every call writes anew: the pinned host copy a call fills, the event that marks where the stream has read that copy — so the call stays
// asynchronous — and the device copy.  In two halves, so that everything that can fail for want of memory happens before the call enqueues anything.
struct StagedTable {
  void* host = nullptr;
  size_t host_cap = 0;
  hipEvent_t sent = nullptr;
  DBuf dev;

  StagedTable() = default;
  StagedTable(const StagedTable&) = delete;
  StagedTable& operator=(const StagedTable&) = delete;
  ~StagedTable() { release(); }

  // Room for `bytes` in both copies; *out: the host copy, free to be written (the last upload has read it).  Enqueues nothing.
  hipError_t stage(size_t bytes, hipStream_t stream, void** out) {
    hipError_t e = sent ? hipEventSynchronize(sent) : hipEventCreateWithFlags(&sent, hipEventDisableTiming);
    if (e == hipSuccess) e = dev.ensure_idle(bytes, stream);  // (an earlier call's kernel may still read the device copy)
    if (e == hipSuccess && bytes > host_cap) {
      if (host) (void)hipHostFree(host);
      host = nullptr, host_cap = 0;
      e = hipHostMalloc(&host, bytes, hipHostMallocDefault);
      if (e == hipSuccess) host_cap = bytes;
    }
    *out = host;
    return e;
  }
  // The upload of the first `bytes` of the host copy, on the stream.
  hipError_t send(size_t bytes, hipStream_t stream) {
    const hipError_t e = hipMemcpyAsync(dev.p, host, bytes, hipMemcpyHostToDevice, stream);
    return e == hipSuccess ? hipEventRecord(sent, stream) : e;
  }
  void release() {  // (with the stream drained)
    if (sent) (void)hipEventDestroy(sent);
    if (host) (void)hipHostFree(host);
    sent = nullptr, host = nullptr, host_cap = 0;
    dev.release();
  }
};

}  // namespace ptmi
