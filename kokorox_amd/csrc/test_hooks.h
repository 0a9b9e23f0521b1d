// The staging kit of the kernel hooks (test_hooks_*.hip, include/kokorox_hip_test.h): device buffers that free themselves, rows
// padded to 32 floats as the model pads them, NaN in what a kernel may not read, one sentinel in what it may not write, and 64 guard
// bytes of 0xA5 behind a buffer.  What the caller cannot see (row padding, guards) a hook checks itself: KX_ERR_STATE.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/kokorox_hip.h"
#include "../../include/kokorox_hip_test.h"
#include "model.h"
#include "check_device.h"
#include "api_guard.h"

namespace kx_test {
using kx::Error;
using kx::guarded_free;

struct DevMem {
    std::vector<void*> p;
    ~DevMem() {
        for (void* q : p) (void)hipFree(q);
    }
    template <class Tp>
    Tp* get(size_t n) {
        void* q = nullptr;
        KX_HIP(hipMalloc(&q, (n ? n : 1) * sizeof(Tp)));
        p.push_back(q);
        return static_cast<Tp*>(q);
    }
    template <class Tp>
    Tp* up(const Tp* h, size_t n) {
        Tp* d = get<Tp>(n);
        KX_HIP(hipMemcpy(d, h, n * sizeof(Tp), hipMemcpyHostToDevice));
        return d;
    }
};

constexpr float SENTINEL = -12345.5f;  // every output location a kernel must not write (integer buffers: 0xA5 bytes)
constexpr int GUARD_BYTES = 64;
constexpr int GUARD_BYTE = 0xA5;
const float POISON = std::nanf("");    // every input location a kernel must not read

inline int pad32(int x) { return (x + 31) & ~31; }

// lens[b] in 1 .. max for every utterance, or KX_ERR_INVALID
inline void check_lens(const int32_t* lens, int B, int max, const char* what) {
    for (int b = 0; b < B; ++b)
        if (lens[b] < 1 || lens[b] > max) throw Error(KX_ERR_INVALID, what);
}

// [B][C][len] -> [B][C][ld]: `fill` in the row padding and - own given - in every column at or past own[b] * own_mul + own_add of
// utterance b (what the caller has there is not copied)
inline std::vector<float> padded_rows(const float* src, int B, int C, int len, int ld, float fill, const int32_t* own = nullptr,
                                      int own_mul = 1, int own_add = 0) {
    std::vector<float> v((size_t)B * C * ld, fill);
    for (int b = 0; b < B; ++b) {
        const size_t n = own ? (size_t)own[b] * own_mul + own_add : (size_t)len;
        for (int c = 0; c < C; ++c) std::memcpy(&v[((size_t)b * C + c) * ld], src + ((size_t)b * C + c) * len, n * 4);
    }
    return v;
}

// [rows][ld] on the device -> [rows][len] on the host; `what` given, the padding of every row must still hold the sentinel
inline void unpad_rows(const float* d_src, size_t rows, int len, int ld, float* dst, const char* what) {
    std::vector<float> v(rows * ld);
    KX_HIP(hipMemcpy(v.data(), d_src, v.size() * 4, hipMemcpyDeviceToHost));
    for (size_t r = 0; r < rows; ++r) {
        std::memcpy(dst + r * len, &v[r * ld], (size_t)len * 4);
        for (int c = len; what && c < ld; ++c)
            if (v[r * ld + c] != SENTINEL) throw Error(KX_ERR_STATE, what);
    }
}

// n elements holding `byte` throughout, the guard behind them (tables and integer outputs)
template <class Tp>
Tp* guarded_bytes(DevMem& dm, size_t n, int byte) {
    unsigned char* d = dm.get<unsigned char>(n * sizeof(Tp) + GUARD_BYTES);
    KX_HIP(hipMemset(d, byte, n * sizeof(Tp)));
    KX_HIP(hipMemset(d + n * sizeof(Tp), GUARD_BYTE, GUARD_BYTES));
    return reinterpret_cast<Tp*>(d);
}
// a host image uploaded, the guard behind it (inputs too: a kernel that wrote behind one is caught as well)
inline float* guarded_upload(DevMem& dm, const std::vector<float>& v) {
    float* d = dm.get<float>(v.size() + GUARD_BYTES / 4);
    KX_HIP(hipMemcpy(d, v.data(), v.size() * 4, hipMemcpyHostToDevice));
    KX_HIP(hipMemset(d + v.size(), GUARD_BYTE, GUARD_BYTES));
    return d;
}
// n floats holding `fill`, the guard behind them
inline float* guarded_buffer(DevMem& dm, size_t n, float fill) { return guarded_upload(dm, std::vector<float>(n, fill)); }

inline void guard_untouched(const void* d_at, const char* what) {
    unsigned char tail[GUARD_BYTES];
    KX_HIP(hipMemcpy(tail, d_at, GUARD_BYTES, hipMemcpyDeviceToHost));
    for (unsigned char c : tail)
        if (c != GUARD_BYTE) throw Error(KX_ERR_STATE, what);
}
}  // namespace kx_test
