// Pool of the page-locked host buffers that carry results to the callers (kx_common.h: host_out_alloc / share / free /
// live_bytes forward to the process-wide instance, model_host.hip).  Plain C++17, no HIP header: the page-locked allocator is
// handed in, so the CPU suite drives the reference counts under the sanitizers (tests/cpp/host_pool_sanitize.cpp).
#pragma once
#include <cstddef>
#include <map>
#include <mutex>

namespace kx {

class HostPool {
  public:
    using AllocFn = void* (*)(size_t bytes);  // page-locked memory, or null when there is none to be had
    using FreeFn = void (*)(void* p);
    // max_idle: bytes of idle buffers the pool keeps; a buffer freed beyond that goes back to free_fn
    HostPool(AllocFn alloc_fn, FreeFn free_fn, size_t max_idle) : alloc_fn_(alloc_fn), free_fn_(free_fn), max_idle_(max_idle) {}
    ~HostPool();  // releases the idle buffers (whatever an owner still holds is the owner's)
    HostPool(const HostPool&) = delete;
    HostPool& operator=(const HostPool&) = delete;

    // An idle buffer of at most 2 * bytes + 1 MiB, else a new one of `bytes` rounded up to 1 MiB; plain malloc'd memory when
    // the page-locked allocation fails (throws kx::Error 3 when that fails too).
    void* alloc(size_t bytes);
    // n pointers into one alloc'd buffer handed to n owners: each is released with free(), the buffer goes back to the pool
    // with the last one (parts[0] may be the buffer's own address)
    void share(void* base, void* const* parts, int n);
    void free(void* p);  // (also plain malloc'd pointers)
    size_t live_bytes();  // capacity of the shared buffers that owners still hold a part of

  private:
    const AllocFn alloc_fn_;
    const FreeFn free_fn_;
    const size_t max_idle_;
    std::mutex mu_;
    std::map<void*, size_t> cap_;             // every live pinned buffer -> capacity
    std::multimap<size_t, void*> free_list_;  // idle ones by capacity
    std::map<void*, void*> alias_;            // pointer handed to an owner -> the shared buffer it lies in (share)
    std::map<void*, int> refs_;               // shared buffer -> owners still holding a part
    size_t idle_bytes_ = 0;
    size_t live_shared_ = 0;                  // capacity of the shared buffers in `refs_`
};

}  // namespace kx
