// Driver for the host side of the weight container (kokorox_amd/csrc/kxw_file.cpp), built by tests/test_kxw_file_cpu.py with
// g++ -fsanitize=address,undefined.  A table needs no tensor data: the input is the header and table of a container, the
// container's size is an argument.
//   kxw_fuzz dump  <total> <table file>              the accepted table, one line per tensor: name ndim d0 d1 d2 d3 offset nbytes
//   kxw_fuzz check <total> <table file>...           per file one line: "accepted <n>" or "error <code> <message>"
//   kxw_fuzz fuzz  <total> <table file> <n> <seed>   n mutations; prints the accepted and rejected counts
//   kxw_fuzz read  <weight file>                     read_weight_file: "variant <v> bytes <n> fnv1a <hash>" or "error <code> <message>"
// Every table is handed over in a heap buffer of EXACTLY its length, so a read past the end is an ASan report; the only
// acceptable outcomes are an accepted table or kx::Error.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kxw_file.h"

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// header first (what Model::load_device_blob does with the first 64 bytes), then the table
static kx::TensorTable accept(const unsigned char* p, size_t n, size_t total) {
    (void)kx::kxw_header(p, n);
    return kx::kxw_table(p, n, total);
}

static int check(const char* path, size_t total) {
    const std::vector<unsigned char> v = kx::read_file(path, "table");
    unsigned char* m = (unsigned char*)malloc(v.size() ? v.size() : 1);
    if (!v.empty()) memcpy(m, v.data(), v.size());
    try {
        printf("accepted %zu\n", accept(m, v.size(), total).size());
    } catch (const kx::Error& e) {
        printf("error %d %s\n", e.code, e.what());
    }
    free(m);
    return 0;
}

static int fuzz(const std::vector<unsigned char>& orig, size_t total, long n_mut) {
    long ok = 0, rejected = 0;
    for (long it = -1; it < n_mut; ++it) {  // (-1: the table as it is)
        size_t n = orig.size();
        const int kind = it < 0 ? -1 : (int)(rnd() % 6);
        if (kind == 0 && n) n = (size_t)(rnd() % n);                          // truncate anywhere
        if (kind == 1 && n) n = n - 1 - (size_t)(rnd() % (n < 64 ? n : 64));  // truncate near the end
        unsigned char* m = (unsigned char*)malloc(n ? n : 1);
        if (n) memcpy(m, orig.data(), n);
        // positions are drawn with a bias towards the header and the first entries
        auto pos = [&]() -> size_t {
            if (!n) return 0;
            const uint64_t r = rnd();
            return (r & 1) ? (size_t)((r >> 1) % (n < 1024 ? n : 1024)) : (size_t)((r >> 1) % n);
        };
        if (n) {
            if (kind == 2)
                for (int k = 0, c = 1 + (int)(rnd() % 8); k < c; ++k) m[pos()] ^= (unsigned char)(1u << (rnd() % 8));  // bit flips
            if (kind == 3) {  // a run of 0xFF: huge offsets, sizes and dimensions
                size_t p = pos();
                for (size_t k = 0, c = 1 + (size_t)(rnd() % 12); k < c && p + k < n; ++k) m[p + k] = 0xFF;
            }
            if (kind == 4)
                for (int k = 0, c = 1 + (int)(rnd() % 4); k < c; ++k) m[pos()] = (unsigned char)rnd();  // random bytes
            if (kind == 5) {  // copy one region over another (valid-looking fields in the wrong place, names twice)
                const size_t a = pos(), b = pos(), len = (size_t)(rnd() % 256);
                for (size_t k = 0; k < len && a + k < n && b + k < n; ++k) m[b + k] = m[a + k];
            }
        }
        try {
            (void)accept(m, n, total);
            ++ok;
        } catch (const kx::Error& e) {
            if (e.code != 2) {
                printf("rejected with code %d: %s\n", e.code, e.what());
                return 1;
            }
            ++rejected;
        }
        free(m);
        if (it < 0 && ok != 1) {
            printf("the unmutated table was rejected\n");
            return 1;
        }
    }
    printf("%ld mutations + the original: %ld accepted, %ld rejected\n", n_mut, ok, rejected);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    try {
        if (mode == "read") {
            try {
                int variant = 99;
                const std::vector<unsigned char> b = kx::read_weight_file(argv[2], &variant);
                uint64_t h = 1469598103934665603ull;
                for (unsigned char c : b) h = (h ^ c) * 1099511628211ull;
                printf("variant %d bytes %zu fnv1a %016llx\n", variant, b.size(), (unsigned long long)h);
            } catch (const kx::Error& e) {
                printf("error %d %s\n", e.code, e.what());
            }
            return 0;
        }
        if (argc < 4) return 2;
        const size_t total = (size_t)strtoull(argv[2], nullptr, 10);
        if (mode == "check") {
            for (int i = 3; i < argc; ++i) check(argv[i], total);
            return 0;
        }
        const std::vector<unsigned char> orig = kx::read_file(argv[3], "table");
        if (mode == "dump") {
            for (const auto& kv : kx::kxw_table(orig.data(), orig.size(), total)) {
                const kx::TensorInfo& t = kv.second;
                printf("%s %d %d %d %d %d %zu %zu\n", kv.first.c_str(), t.ndim, t.dims[0], t.dims[1], t.dims[2], t.dims[3], t.offset, t.nbytes);
            }
            return 0;
        }
        if (mode == "fuzz" && argc >= 6) {
            rng_state = (uint64_t)atoll(argv[5]);
            return fuzz(orig, total, atol(argv[4]));
        }
    } catch (const kx::Error& e) {
        printf("error %d %s\n", e.code, e.what());
        return 1;
    }
    return 2;
}
