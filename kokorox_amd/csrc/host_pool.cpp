// The pooled result buffers (host_pool.h).  No HIP.
#include "host_pool.h"

#include <cstdlib>

#include "kx_error.h"

namespace kx {

HostPool::~HostPool() {
    for (auto& kv : free_list_) free_fn_(kv.second);
}

void* HostPool::alloc(size_t bytes) {
    {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = free_list_.lower_bound(bytes);
        if (it != free_list_.end() && it->first <= 2 * bytes + (1 << 20)) {
            void* p = it->second;
            idle_bytes_ -= it->first;
            free_list_.erase(it);
            return p;
        }
    }
    const size_t want = (bytes + (1 << 20) - 1) & ~((size_t(1) << 20) - 1);
    void* p = alloc_fn_(want);
    if (!p) {
        p = malloc(bytes);  // pageable memory still works with hipMemcpyAsync (staged by the runtime)
        if (!p) throw Error(3, "infer: out of host memory");
        return p;
    }
    std::lock_guard<std::mutex> lk(mu_);
    cap_[p] = want;
    return p;
}

void HostPool::share(void* base, void* const* parts, int n) {
    if (!base || n <= 0) return;
    std::lock_guard<std::mutex> lk(mu_);
    // one reference per DISTINCT pointer: two parts with the same address (a zero-byte part; cannot happen today, an utterance
    // has at least one frame) would share one key, and a count of n would then never come down to zero
    int distinct = 0;
    for (int i = 0; i < n; ++i) distinct += alias_.emplace(parts[i], base).second ? 1 : 0;
    refs_[base] = distinct;
    auto it = cap_.find(base);
    if (it != cap_.end()) live_shared_ += it->second;
}

size_t HostPool::live_bytes() {
    std::lock_guard<std::mutex> lk(mu_);
    return live_shared_;
}

void HostPool::free(void* p) {
    if (!p) return;
    size_t c = 0;
    {
        std::lock_guard<std::mutex> lk(mu_);
        auto al = alias_.find(p);
        if (al != alias_.end()) {  // one part of a shared batch buffer: the buffer itself goes when the last part has gone
            void* base = al->second;
            alias_.erase(al);
            auto rf = refs_.find(base);
            if (rf != refs_.end() && --rf->second > 0) return;
            if (rf != refs_.end()) refs_.erase(rf);
            p = base;
            auto cb = cap_.find(base);
            if (cb != cap_.end()) live_shared_ -= cb->second < live_shared_ ? cb->second : live_shared_;
        }
        auto it = cap_.find(p);
        if (it != cap_.end()) {
            c = it->second;
            if (idle_bytes_ + c <= max_idle_) {
                free_list_.emplace(c, p);
                idle_bytes_ += c;
                return;
            }
            cap_.erase(it);
        }
    }
    if (c) free_fn_(p);
    else ::free(p);
}

}  // namespace kx
