// Driver for the pool of the result buffers (kokorox_amd/csrc/host_pool.cpp), built by tests/test_host_sanitize_cpu.py with g++
// under ThreadSanitizer and under AddressSanitizer + UBSan with leak detection.  The page-locked allocator is replaced by a
// counting pair on malloc / free, so every buffer the pool gives back too early, twice or never is a sanitizer report or a
// failed count.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "host_pool.h"

static std::atomic<long> n_alloc{0}, n_free{0};
static void* counting_alloc(size_t bytes) {
    n_alloc += 1;
    return malloc(bytes);
}
static void* failing_alloc(size_t) {
    n_alloc += 1;
    return nullptr;
}
static void counting_free(void* p) {
    n_free += 1;
    free(p);
}

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

static constexpr size_t MiB = size_t(1) << 20;

static void reuse_rule() {
    n_alloc = n_free = 0;
    {
        kx::HostPool pool(counting_alloc, counting_free, 64 * MiB);
        void* p = pool.alloc(1000);
        memset(p, 1, MiB);  // (rounded up to 1 MiB)
        CHECK(n_alloc == 1);
        pool.free(p);
        CHECK(pool.alloc(1000) == p && n_alloc == 1);
        pool.free(p);
        // a buffer of 4 MiB serves requests down to (4 MiB - 1 MiB) / 2 and none below
        void* big = pool.alloc(4 * MiB);
        CHECK(big != p && n_alloc == 2);
        pool.free(big);
        const size_t least = (4 * MiB - MiB) / 2;
        CHECK(pool.alloc(least) == big && n_alloc == 2);
        pool.free(big);
        void* q = pool.alloc(least - 1);  // (the idle 1 MiB buffer is too small for it, the 4 MiB one too large)
        CHECK(q != big && q != p && n_alloc == 3);
        pool.free(q);
        CHECK(n_free == 0 && pool.live_bytes() == 0);
    }
    CHECK(n_alloc == 3 && n_free == 3);  // (the destructor releases the idle buffers)
}

static void shared_buffer_orders() {
    n_alloc = n_free = 0;
    kx::HostPool pool(counting_alloc, counting_free, 64 * MiB);
    const size_t cap = 3 * MiB;
    for (int first_is_base = 0; first_is_base < 2; ++first_is_base)
        for (int order = 0; order < 3; ++order) {
            char* base = static_cast<char*>(pool.alloc(cap));
            CHECK(n_alloc == 1);  // (every round re-uses the first buffer)
            void* parts[5] = {base + (first_is_base ? 0 : 16), base + 100, base + 100, base + 200, base + 300};  // n = 5, two equal
            pool.share(base, parts, 5);
            CHECK(pool.live_bytes() == cap);
            void* owners[4] = {parts[0], parts[1], parts[3], parts[4]};  // n - 1 owners
            static const int seq[3][4] = {{0, 1, 2, 3}, {3, 2, 1, 0}, {2, 0, 3, 1}};
            for (int i = 0; i < 4; ++i) {
                CHECK(pool.live_bytes() == cap);
                memset(base, i, cap);  // (still the owners': a buffer released early is a use after free once it is handed out again)
                pool.free(owners[seq[order][i]]);
            }
            CHECK(pool.live_bytes() == 0);
            CHECK(pool.alloc(cap) == base && n_alloc == 1);
            pool.free(base);
        }
    CHECK(n_free == 0);
}

static void two_shared_buffers_alternately() {
    n_alloc = n_free = 0;
    kx::HostPool pool(counting_alloc, counting_free, 64 * MiB);
    const size_t cap_a = 2 * MiB, cap_b = 5 * MiB;
    for (int round = 0; round < 2; ++round) {  // (the second round meets whatever alias the first one left behind)
        char* a = static_cast<char*>(pool.alloc(cap_a));
        char* b = static_cast<char*>(pool.alloc(cap_b));
        CHECK(n_alloc == 2);
        void* pa[3] = {a, a + 64, a + 128};
        void* pb[3] = {b + 8, b + 64, b + 128};
        pool.share(a, pa, 3);
        pool.share(b, pb, 3);
        CHECK(pool.live_bytes() == cap_a + cap_b);
        pool.free(pa[0]);
        pool.free(pb[0]);
        pool.free(pa[1]);
        pool.free(pb[1]);
        CHECK(pool.live_bytes() == cap_a + cap_b);
        pool.free(pa[2]);
        CHECK(pool.live_bytes() == cap_b);
        pool.free(pb[2]);
        CHECK(pool.live_bytes() == 0);
        // both are idle and plain again: handed out, and released as buffers, not as parts
        CHECK(pool.alloc(cap_a) == a && pool.alloc(cap_b) == b && n_alloc == 2);
        pool.free(a);
        pool.free(b);
        CHECK(pool.live_bytes() == 0 && n_free == 0);
    }
}

static void idle_cap() {
    n_alloc = n_free = 0;
    {
        kx::HostPool pool(counting_alloc, counting_free, MiB);
        void* p = pool.alloc(100);
        void* q = pool.alloc(100);
        CHECK(n_alloc == 2 && p != q);
        pool.free(p);
        CHECK(n_free == 0);
        pool.free(q);  // beyond the cap: back to the allocator, and forgotten
        CHECK(n_free == 1);
        CHECK(pool.alloc(100) == p && n_alloc == 2);
        void* r = pool.alloc(100);
        CHECK(n_alloc == 3);
        pool.free(r);
        pool.free(p);
        CHECK(n_free == 2);
    }
    CHECK(n_alloc == 3 && n_free == 3);
}

static void failing_allocator() {
    n_alloc = n_free = 0;
    {
        kx::HostPool pool(failing_alloc, counting_free, 64 * MiB);
        char* p = static_cast<char*>(pool.alloc(100));
        CHECK(p && n_alloc == 1);
        memset(p, 7, 100);  // (a plain malloc block of exactly the bytes asked for)
        void* parts[2] = {p, p + 50};
        pool.share(p, parts, 2);
        CHECK(pool.live_bytes() == 0);  // (not page-locked: nothing to account for)
        pool.free(p + 50);
        pool.free(p);  // released with free(): leak detection stays clean
        void* q = pool.alloc(100);
        CHECK(n_alloc == 2);
        pool.free(q);
    }
    CHECK(n_free == 0);
}

static uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static void threads() {
    n_alloc = n_free = 0;
    {
        kx::HostPool pool(counting_alloc, counting_free, 6 * MiB);  // (small: both the idle list and the allocator's free are taken)
        std::vector<std::thread> th;
        for (int t = 0; t < 8; ++t)
            th.emplace_back([&pool, t] {
                uint64_t s = 1000 + (uint64_t)t;
                std::vector<char*> held;  // buffers and parts of shared buffers: all released the same way
                for (int op = 0; op < 3000; ++op) {
                    const uint64_t r = splitmix(s);
                    const int kind = (int)(r % 4);
                    if (held.size() < 12 && kind == 0) {
                        char* p = static_cast<char*>(pool.alloc(1 + (size_t)((r >> 8) % (3 * MiB))));
                        p[0] = (char)t;
                        held.push_back(p);
                    } else if (held.size() < 12 && kind == 1) {
                        char* base = static_cast<char*>(pool.alloc(4096 + (size_t)((r >> 8) % (2 * MiB))));
                        const int n = 2 + (int)((r >> 40) % 3);
                        void* parts[5];
                        for (int i = 0; i < n; ++i) parts[i] = base + 1024 * i + ((r >> 50) & 1 ? 0 : 16);
                        parts[n] = parts[n - 1];  // (a part given twice counts once)
                        pool.share(base, parts, n + 1);
                        for (int i = 0; i < n; ++i) {
                            static_cast<char*>(parts[i])[0] = (char)t;
                            held.push_back(static_cast<char*>(parts[i]));
                        }
                    } else if (!held.empty()) {
                        const size_t i = (size_t)((r >> 8) % held.size());
                        held[i][0] = (char)(t + 1);  // (still ours until it is released)
                        pool.free(held[i]);
                        held[i] = held.back();
                        held.pop_back();
                    }
                    (void)pool.live_bytes();
                }
                for (char* p : held) pool.free(p);
            });
        for (auto& x : th) x.join();
        CHECK(pool.live_bytes() == 0);
    }
    CHECK(n_alloc > 0 && n_alloc == n_free);  // every allocator call is matched, the destructor's included
    printf("threads: %ld page-locked allocations, all released\n", n_alloc.load());
}

int main() {
    reuse_rule();
    shared_buffer_orders();
    two_shared_buffers_alternately();
    idle_cap();
    failing_allocator();
    threads();
    printf("host pool: all scenarios passed\n");
    return 0;
}
