// The FLAC encoder of the output stage (gfx950): the 16-bit values of a request's final stream (request_stream.h: stage_final) as
// frames, their layout, and the body gathered at the front of its region.
#include "kx_common.h"
#include "request_stream.h"
#include "request_units.h"

namespace kx {

// ---- FLAC: lossless 16-bit frames, one workgroup a frame (include/kokorox_hip.h, "FLAC"; host_request.h: FlacRow) ---------------
// The samples are form 4's 16-bit v of the request's final stream, the one the packer of this plan would stage (request_stream.h:
// stage_final has the definition; this kernel keeps its own copy of it, the gain applied where it converts), then pcm16_sample with
// NaN -> 0.
//
// flac_frames_kernel: workgroup (f, r) encodes frame f of request r, n = min(4096, N - 4096 f) samples, into slot r's first + f of the
// scratch table and stores its size.  Lane t owns the 16 samples from 16 t: it keeps them and the four before them in registers, forms
// the residuals of the five fixed predictors by repeated differences (the binomial forms, |e| < 2^20 in int32) and folds them; a
// residual the rules do not count (i < o, i >= n) is 0.  The bit sums: sum of u >> k over the lane's 16, over four lanes with two
// __shfl_xor, one dword per (o, k, 64 samples) into LDS; then for P = 6 .. 0 a lane per (o, partition) takes the k in 0..14 with the
// fewest bits (the first minimum) and adds 4 + those bits to cost[o][P] with an LDS atomic -- integer addition: the order does not
// show -- while the pairs are summed into the other of two buffers for the next level (the staged samples are dead by then: their
// LDS is the second buffer).  Every sum fits a dword: at most 4092 residuals below 2^20 - 16.  Every lane reads the 35 costs and
// makes the one choice the header prescribes.  The code lengths are scanned (__shfl_up inside a wave, the four wave totals through
// LDS), and every lane ORs its codes into the zeroed bit buffer, MSB first: a Rice code is its stop bit and k bits at the position
// behind its zeros, at most two dwords.  The CRC-16 is NOT a serial walk: lane t takes the CRC of c = ceil(L / 256) bytes, the
// chunks aligned to the frame's end (zeros in front of a message do not change a CRC that starts at 0), multiplies it by
// x^(8 c (255 - t)) modulo the polynomial (square and multiply, 16-bit carry-less products) and the 256 products are XOR-ed: the
// CRC is linear.  The frame leaves as whole dwords, byte-swapped: the buffer is MSB first, memory little-endian.
constexpr int FLAC_THREADS = 256;
constexpr int FLAC_OWN = (int)FLAC_BLOCK / FLAC_THREADS;  // 16 samples a lane
constexpr int FLAC_WORDS = (int)FLAC_SLOT / 4;            // 2052 dwords a slot
constexpr int FLAC_KS = 15;                               // Rice parameters 0..14
static_assert(FLAC_OWN == 16 && FLAC_SLOT % 16 == 0 && FLAC_BLOCK == LEVEL_WINDOW, "16 samples a lane, aligned slots");

__device__ __forceinline__ void flac_put(uint32_t* __restrict__ buf, uint32_t pos, uint32_t value, int width) {
    const uint32_t off = pos & 31u;  // bits [off, off + width) of the 64-bit window of dwords pos / 32 and the next, counted from the MSB
    const unsigned long long x = (unsigned long long)value << (64u - off - (uint32_t)width);
    const uint32_t hi = (uint32_t)(x >> 32), lo = (uint32_t)x;
    if (hi) atomicOr(&buf[pos >> 5], hi);
    if (lo) atomicOr(&buf[(pos >> 5) + 1], lo);
}
// a b modulo x^16 + x^15 + x^2 + 1, the 16-bit remainders as dwords
__device__ __forceinline__ uint32_t flac_gf_mul(uint32_t a, uint32_t b) {
    uint32_t r = 0;
#pragma unroll
    for (int i = 15; i >= 0; --i) {
        r = ((r << 1) ^ ((r & 0x8000u) ? 0x8005u : 0u)) & 0xFFFFu;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}
// bytes of frame number f in the format's UTF-8-like coding: 1 below 2^7, n where it fits 5 n + 1 bits
__device__ __forceinline__ int flac_number_bytes(uint32_t f) {
    int n = 1;
    if (f >= 0x80u) {
        n = 2;
        while (n < 6 && (f >> (5 * n + 1))) ++n;
    }
    return n;
}

__global__ __launch_bounds__(FLAC_THREADS) void flac_frames_kernel(const float* __restrict__ audio, long audio_ld,
                                                                   const PackReq* __restrict__ reqs, const long* __restrict__ cum,
                                                                   const JoinRow* __restrict__ jrows, const float* __restrict__ y,
                                                                   const double* __restrict__ levels,
                                                                   const LimitRow* __restrict__ lrows, const float* __restrict__ lim,
                                                                   const FlacRow* __restrict__ frows, uint32_t* __restrict__ slots,
                                                                   int* __restrict__ flen) {
    __shared__ int vs[FLAC_BLOCK];                        // the staged floats, then v, then the sums of every other level
    __shared__ uint32_t sums[5 * FLAC_KS * 64];           // [o][k][64 samples], then every other level
    __shared__ uint32_t bitbuf[FLAC_WORDS];
    __shared__ uint32_t cost[5 * 7];                      // [o][P]: the bits of the partitions, their 4-bit parameters included
    __shared__ unsigned char ks[5 * 128];                 // [o][(1 << P) + j]: the parameter of partition j at order P
    __shared__ uint32_t wave_tot[FLAC_THREADS / 64];
    __shared__ uint32_t wave_crc[FLAC_THREADS / 64];
    const FlacRow fr = frows[blockIdx.y];
    if (fr.frames < 0 || (long)blockIdx.x >= fr.frames) return;  // (uniform: another form, or the grid covers the request with most frames)
    const PackReq rq = reqs[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long n0 = (long)blockIdx.x * FLAC_BLOCK;
    const long n1 = n0 + FLAC_BLOCK < fr.n_samples ? n0 + FLAC_BLOCK : fr.n_samples;
    const int n = (int)(n1 - n0);
    // the final stream's samples; every lane converts what it staged itself (sample i: lane (i - n0) mod 256)
    float* __restrict__ smp = reinterpret_cast<float*>(vs);
    const long lim_off = lrows ? lrows[blockIdx.y].off : -1;
    // (request_stream.h: stage_final, written out: staged through the helper this kernel's machine code is no longer the parent's --
    // profiles/request_units_codegen.txt, variant 1 -- and no timing was taken that would admit a changed kernel)
    bool scaled = false;
    if (lim_off >= 0) {  // (uniform) a limited request: scaled and limited already
        const float* __restrict__ src = lim + lim_off;
        for (long i = n0 + tid; i < n1; i += FLAC_THREADS) smp[i - n0] = src[i];
    } else if (rq.rate) {  // (uniform) a resampled request: one contiguous run
        const float* __restrict__ src = y + rq.y_off;
        for (long i = n0 + tid; i < n1; i += FLAC_THREADS) smp[i - n0] = src[i];
        scaled = levels != nullptr;
    } else {
        stage_rows<FLAC_THREADS>(smp, audio, audio_ld, cum, jrows, rq.first_row, rq.n_rows, n0, n1);
        scaled = levels != nullptr;
    }
    const double g = scaled ? levels[2 * blockIdx.y + 1] : 1.0;
    for (int i = tid; i < n; i += FLAC_THREADS) {
        float x = smp[i];
        if (scaled) x = (float)(g * (double)x);
        vs[i] = pcm16_sample(x, true);
    }
    for (int i = tid; i < FLAC_WORDS; i += FLAC_THREADS) bitbuf[i] = 0u;
    if (tid < 5 * 7) cost[tid] = 0u;
    __syncthreads();
    // the lane's samples and the four before them; w[4 + i] = v[16 t + i], 0 outside the frame
    const int base = FLAC_OWN * tid;
    int w[FLAC_OWN + 4];
#pragma unroll
    for (int i = 0; i < FLAC_OWN + 4; ++i) {
        const int idx = base - 4 + i;
        w[i] = idx >= 0 && idx < n ? vs[idx] : 0;
    }
    const int v0 = vs[0];
    int equal = 1;
#pragma unroll
    for (int i = 0; i < FLAC_OWN; ++i) equal &= (base + i >= n) | (w[4 + i] == v0);
    const int all_equal = __syncthreads_and(equal);  // (and the staged samples are in registers: vs is free)
    // the folded residuals u[o][i] of sample 16 t + i, by repeated differences
    uint32_t u[5][FLAC_OWN];
    {
        int d[FLAC_OWN + 4];
#pragma unroll
        for (int i = 0; i < FLAC_OWN + 4; ++i) d[i] = w[i];
#pragma unroll
        for (int o = 0; o < 5; ++o) {
#pragma unroll
            for (int i = 0; i < FLAC_OWN; ++i) {
                const int e = d[4 + i], idx = base + i;
                u[o][i] = idx >= o && idx < n ? ((uint32_t)e << 1) ^ (uint32_t)(e >> 31) : 0u;
            }
#pragma unroll
            for (int i = FLAC_OWN + 3; i >= 1; --i) d[i] -= d[i - 1];  // (entries below o + 1 are not used again)
        }
    }
    if (!all_equal) {  // (uniform)
#pragma unroll
        for (int o = 0; o < 5; ++o) {
#pragma unroll
            for (int k = 0; k < FLAC_KS; ++k) {
                uint32_t s = 0;
#pragma unroll
                for (int i = 0; i < FLAC_OWN; ++i) s += u[o][i] >> k;
                s += (uint32_t)__shfl_xor((int)s, 1);
                s += (uint32_t)__shfl_xor((int)s, 2);
                if ((tid & 3) == 0) sums[(o * FLAC_KS + k) * 64 + (tid >> 2)] = s;
            }
        }
        __syncthreads();
        uint32_t* src = sums;
        uint32_t* dst = reinterpret_cast<uint32_t*>(vs);
        for (int P = 6; P >= 0; --P) {
            const int parts = 1 << P;
            for (int t = tid; t < 5 * parts; t += FLAC_THREADS) {
                const int o = t >> P, j = t & (parts - 1);
                // (a short frame is judged at P = 0 alone, where the partition is the frame; its other costs are not read)
                const uint32_t count = (uint32_t)((n == (int)FLAC_BLOCK ? (int)FLAC_BLOCK >> P : n) - (j == 0 ? o : 0));
                uint32_t best = 0xFFFFFFFFu;
                int best_k = 0;
#pragma unroll
                for (int k = 0; k < FLAC_KS; ++k) {
                    const uint32_t c = src[((o * FLAC_KS + k) << P) + j] + (uint32_t)(k + 1) * count;
                    if (c < best) best = c, best_k = k;
                }
                ks[o * 128 + parts + j] = (unsigned char)best_k;
                atomicAdd(&cost[o * 7 + P], 4u + best);
            }
            if (P > 0) {
                const int half = parts >> 1;
                for (int t = tid; t < 5 * FLAC_KS * half; t += FLAC_THREADS) {
                    const int ok = t / half, j = t - ok * half;
                    dst[ok * half + j] = src[ok * parts + 2 * j] + src[ok * parts + 2 * j + 1];
                }
            }
            __syncthreads();
            uint32_t* const tmp = src;
            src = dst, dst = tmp;
        }
    }
    // the choice: the fewest bits, the smaller o, then the smaller P; VERBATIM from 16 n bits on
    int o_best = 0, P_best = 0;
    uint32_t bits_best = 0xFFFFFFFFu;
    if (!all_equal) {
        const int o_max = n - 1 < 4 ? n - 1 : 4, P_max = n == (int)FLAC_BLOCK ? 6 : 0;
        for (int o = 0; o <= o_max; ++o)
            for (int P = 0; P <= P_max; ++P) {
                const uint32_t b = 16u * (uint32_t)o + 6u + cost[o * 7 + P];
                if (b < bits_best) bits_best = b, o_best = o, P_best = P;
            }
    }
    const bool verbatim = !all_equal && bits_best >= 16u * (uint32_t)n;
    // the frame header: sync, block size and rate, one channel of 16 bits, the frame number, the short block's size, CRC-8
    const uint32_t fno = blockIdx.x;
    const int nb = flac_number_bytes(fno);
    const int head = 4 + nb + (n == (int)FLAC_BLOCK ? 0 : 2) + 1;
    const uint32_t hbits = 8u * (uint32_t)head;
    if (tid == 0) {
        unsigned char hb[16];
        const uint32_t rate_nibble = fr.rate == 1 ? 4u : (fr.rate == 2 ? 5u : (fr.rate == 3 ? 10u : 7u));
        hb[0] = 0xFF, hb[1] = 0xF8, hb[2] = (unsigned char)(((n == (int)FLAC_BLOCK ? 12u : 7u) << 4) | rate_nibble), hb[3] = 0x08;
        int at = 4;
        if (nb == 1) {
            hb[at++] = (unsigned char)fno;
        } else {
            hb[at++] = (unsigned char)(((0xFFu << (8 - nb)) & 0xFFu) | (fno >> (6 * (nb - 1))));
            for (int k = nb - 2; k >= 0; --k) hb[at++] = (unsigned char)(0x80u | ((fno >> (6 * k)) & 0x3Fu));
        }
        if (n != (int)FLAC_BLOCK) hb[at++] = (unsigned char)((n - 1) >> 8), hb[at++] = (unsigned char)((n - 1) & 255);
        uint32_t c = 0;
        for (int i = 0; i < at; ++i) {
            c ^= hb[i];
            for (int b = 0; b < 8; ++b) c = ((c << 1) ^ ((c & 0x80u) ? 0x07u : 0u)) & 0xFFu;
        }
        hb[at++] = (unsigned char)c;
        for (int i = 0; i < at; ++i) flac_put(bitbuf, 8u * (uint32_t)i, hb[i], 8);
    }
    uint32_t total_bits;
    if (all_equal) {  // (uniform)
        if (tid == 0) flac_put(bitbuf, hbits + 8u, (uint32_t)v0 & 0xFFFFu, 16);  // (the subframe's header byte is 0x00: CONSTANT)
        total_bits = hbits + 24u;
    } else if (verbatim) {  // (uniform)
        if (tid == 0) flac_put(bitbuf, hbits, 0x02u, 8);
#pragma unroll
        for (int i = 0; i < FLAC_OWN; ++i)
            if (base + i < n) flac_put(bitbuf, hbits + 8u + 16u * (uint32_t)(base + i), (uint32_t)w[4 + i] & 0xFFFFu, 16);
        total_bits = hbits + 8u + 16u * (uint32_t)n;
    } else {
        uint32_t ue[FLAC_OWN];
#pragma unroll
        for (int i = 0; i < FLAC_OWN; ++i) {
            ue[i] = u[0][i];
#pragma unroll
            for (int o = 1; o < 5; ++o)
                if (o == o_best) ue[i] = u[o][i];  // (uniform)
        }
        const int psz = (n == (int)FLAC_BLOCK ? (int)FLAC_BLOCK : n) >> P_best;  // (P_best = 0 in a short frame)
        const int j = base < n ? base / psz : 0;
        const int k = ks[o_best * 128 + (1 << P_best) + j];
        uint32_t len = 0;
#pragma unroll
        for (int i = 0; i < FLAC_OWN; ++i)
            if (base + i >= o_best && base + i < n) len += (ue[i] >> k) + 1u + (uint32_t)k;
        uint32_t incl = len;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int q = 0; q < FLAC_THREADS / 64; ++q) {
            before += q < wave ? wave_tot[q] : 0u;
            all += wave_tot[q];
        }
        const uint32_t body = hbits + 8u + 16u * (uint32_t)o_best + 6u;  // the first partition's parameter
        if (tid == 0) {
            flac_put(bitbuf, hbits, (uint32_t)(8 + o_best) << 1, 8);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < o_best) flac_put(bitbuf, hbits + 8u + 16u * (uint32_t)i, (uint32_t)w[4 + i] & 0xFFFFu, 16);
            flac_put(bitbuf, body - 6u, (uint32_t)P_best, 6);  // (coding method 00, then the partition order)
        }
        uint32_t pos = body + 4u * (uint32_t)(j + 1) + before + incl - len;
        if (base < n) {
            if (base % psz == 0) flac_put(bitbuf, pos - 4u, (uint32_t)k, 4);
#pragma unroll
            for (int i = 0; i < FLAC_OWN; ++i) {
                if (base + i >= o_best && base + i < n) {
                    const uint32_t q = ue[i] >> k;
                    flac_put(bitbuf, pos + q, (1u << k) | (ue[i] & ((1u << k) - 1u)), k + 1);
                    pos += q + 1u + (uint32_t)k;
                }
            }
        }
        total_bits = body + 4u * (1u << P_best) + all;
    }
    __syncthreads();
    // the CRC-16 of the L bytes so far, by linearity
    const int L = (int)((total_bits + 7u) >> 3), c = (L + FLAC_THREADS - 1) / FLAC_THREADS;
    uint32_t crc = 0;
    {
        const int lo = L - (FLAC_THREADS - tid) * c;
        for (int q = lo < 0 ? 0 : lo; q < lo + c; ++q) {
            crc ^= ((bitbuf[q >> 2] >> (24 - 8 * (q & 3))) & 0xFFu) << 8;
#pragma unroll
            for (int b = 0; b < 8; ++b) crc = ((crc << 1) ^ ((crc & 0x8000u) ? 0x8005u : 0u)) & 0xFFFFu;
        }
        uint32_t m = 1u;  // x^(8 c)
        for (int b = 0; b < 8 * c; ++b) m = ((m << 1) ^ ((m & 0x8000u) ? 0x8005u : 0u)) & 0xFFFFu;
        uint32_t shift = 1u;  // x^(8 c (255 - t))
        for (int e = FLAC_THREADS - 1 - tid; e > 0; e >>= 1) {
            if (e & 1) shift = flac_gf_mul(shift, m);
            m = flac_gf_mul(m, m);
        }
        crc = flac_gf_mul(crc, shift);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, o);
    if (lane == 0) wave_crc[wave] = crc;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int q = 1; q < FLAC_THREADS / 64; ++q) crc ^= wave_crc[q];
        flac_put(bitbuf, 8u * (uint32_t)L, crc, 16);
        flen[fr.slot + blockIdx.x] = L + 2;
    }
    __syncthreads();
    uint32_t* __restrict__ out = slots + (fr.slot + blockIdx.x) * FLAC_WORDS;
    for (int q = tid; q < (L + 2 + 3) / 4; q += FLAC_THREADS) out[q] = __builtin_bswap32(bitbuf[q]);
}

// flac_layout_kernel: one wave per request scans its frames' sizes into their offsets behind the first frame (__shfl_up, 64 frames a
// round), takes the smallest and the largest, and stores the padding's size with them and the body's true size into the lengths
// block; the size of a request of another form is its region's.
__global__ __launch_bounds__(64) void flac_layout_kernel(const FlacRow* __restrict__ frows, const int* __restrict__ flen,
                                                         long* __restrict__ foff, FlacInfo* __restrict__ finfo,
                                                         long long* __restrict__ lengths) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const FlacRow fr = frows[r];
    if (fr.frames < 0) {  // (the whole wave)
        if (lane == 0) lengths[r] = fr.out_bytes;
        return;
    }
    long carry = 0;
    int mn = 0x7FFFFFFF, mx = 0;
    for (long f0 = 0; f0 < fr.frames; f0 += 64) {
        const long f = f0 + lane;
        const int len = f < fr.frames ? flen[fr.slot + f] : 0;
        long incl = len;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        if (f < fr.frames) {
            foff[fr.slot + f] = carry + incl - len;
            mn = len < mn ? len : mn;
            mx = len > mx ? len : mx;
        }
        carry += __shfl(incl, 63);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if (lane != 0) return;
    const long p = (2 - carry) & 3;  // 46 + p + the frames' bytes is a multiple of 4
    finfo[r] = FlacInfo{46 + p, 46 + p + carry, fr.frames > 0 ? mn : 0, mx};
    lengths[r] = 46 + p + carry;
}

// flac_gather_kernel: the body at the front of its region.  A lane assembles ONE dword of it -- bytes 4 q .. 4 q + 3 -- and stores it
// whole: where the four bytes lie in one frame (found by bisection over the offsets) they are two dwords of its slot, funnel-shifted;
// a dword across a seam, or of the 46 + p bytes before the frames, is put together byte by byte, the header's bytes computed from
// the four numbers they depend on.  Nothing past the body's true size is written.
__device__ __forceinline__ uint32_t flac_head_byte(long q, const FlacRow& fr, const FlacInfo& fi) {
    const uint32_t hz = fr.rate == 1 ? 8000u : (fr.rate == 2 ? 16000u : (fr.rate == 3 ? 48000u : 24000u));
    if (q < 4) return q == 0 ? 0x66u : (q == 1 ? 0x4Cu : (q == 2 ? 0x61u : 0x43u));  // "fLaC"
    if (q < 8) return q == 7 ? 34u : 0u;                                               // STREAMINFO, not last, 34 bytes
    if (q < 12) return (q & 1) ? 0u : 0x10u;                                           // blocks of 4096, twice
    if (q < 15) return ((uint32_t)fi.min_frame >> (8 * (14 - q))) & 0xFFu;
    if (q < 18) return ((uint32_t)fi.max_frame >> (8 * (17 - q))) & 0xFFu;
    if (q < 26) {  // rate (20 bits), channels - 1 (3), bits - 1 (5), samples (36)
        const unsigned long long word = ((unsigned long long)hz << 44) | (15ull << 36) | (unsigned long long)fr.n_samples;
        return (uint32_t)(word >> (8 * (25 - q))) & 0xFFu;
    }
    if (q == 42) return 0x81u;  // PADDING, last
    if (q == 45) return (uint32_t)(fi.head - 46);
    return 0u;  // the MD5 ("not computed"), the upper bytes of the padding's size, the padding
}
__global__ __launch_bounds__(256) void flac_gather_kernel(const FlacRow* __restrict__ frows, const FlacInfo* __restrict__ finfo,
                                                          const uint32_t* __restrict__ slots, const int* __restrict__ flen,
                                                          const long* __restrict__ foff, char* __restrict__ out) {
    const FlacRow fr = frows[blockIdx.y];
    if (fr.frames < 0) return;  // (uniform) another form
    const FlacInfo fi = finfo[blockIdx.y];
    const long q0 = 4 * ((long)blockIdx.x * 256 + threadIdx.x);
    if (q0 >= fi.total) return;  // (the grid covers the largest region)
    // the frame of byte q >= head: the last one whose offset is at or before it
    auto frame_of = [&](long s) {
        long lo = 0, hi = fr.frames - 1;
        while (lo < hi) {
            const long mid = (lo + hi + 1) >> 1;
            if (foff[fr.slot + mid] <= s) lo = mid; else hi = mid - 1;
        }
        return lo;
    };
    uint32_t word = 0;
    bool done = false;
    if (q0 >= fi.head) {
        const long s = q0 - fi.head, f = frame_of(s), rel = s - foff[fr.slot + f];
        if (rel + 4 <= flen[fr.slot + f]) {
            const uint32_t* __restrict__ src = slots + (fr.slot + f) * FLAC_WORDS + (rel >> 2);
            const int sh = 8 * (int)(rel & 3);
            word = sh ? (src[0] >> sh) | (src[1] << (32 - sh)) : src[0];  // (src[1] holds byte rel + 4 - (rel & 3) .. : inside the frame's dwords)
            done = true;
        }
    }
    if (!done) {
        for (int t = 0; t < 4; ++t) {
            const long q = q0 + t;  // (below total: the body is a multiple of 4)
            uint32_t b;
            if (q < fi.head) {
                b = flac_head_byte(q, fr, fi);
            } else {
                const long s = q - fi.head, f = frame_of(s), rel = s - foff[fr.slot + f];
                b = (slots[(fr.slot + f) * FLAC_WORDS + (rel >> 2)] >> (8 * (int)(rel & 3))) & 0xFFu;
            }
            word |= b << (8 * t);
        }
    }
    *reinterpret_cast<uint32_t*>(out + fr.out_off + q0) = word;
}

// FLAC: the frames into their slots, the layout of every body, then the frames to their places; the samples are those the packer
// launched behind this stage would stage (the same join rows, gains and limit buffer)
void launch_flac_stage(const float* audio, long audio_ld, const OutputPlan& plan, const OutputTables& t, float* d_y, char* out,
                       hipStream_t s) {
    const unsigned R = (unsigned)plan.req.size();
    const bool gains = plan.limited || plan.levelled;
    if (plan.flac_max_frames > 0)
        launch_checked(flac_frames_kernel, dim3((unsigned)plan.flac_max_frames, R), dim3(FLAC_THREADS), s, audio, audio_ld, t.req, t.cum,
                       plan.joined || gains ? t.join : nullptr, d_y, gains ? plan_levels(plan, out) : nullptr, plan.limited ? t.limit : nullptr,
                       plan.limited ? t.lim : nullptr, t.frow, t.fslot, t.flen);
    launch_checked(flac_layout_kernel, dim3(R), dim3(64), s, t.frow, t.flen, t.foff, t.finfo, reinterpret_cast<long long*>(out + plan.flac_off));
    launch_checked(flac_gather_kernel, dim3((unsigned)((plan.flac_max_bytes / 4 + 255) / 256), R), dim3(256), s, t.frow, t.finfo, t.fslot, t.flen,
                   t.foff, out);
}

}  // namespace kx
