// The output stage of a call (gfx950): every request of the batch packed as the bytes a server sends -- the packer and its
// forms (samples, WAV, base64, G.711), the output-rate resampler before it, the levels between the two (a request's peak, its
// gain, the levelled packer) and the loudness beside them (the BS.1770 meter and its gain), the token timing marks behind the bodies and the edge durations the host's join plan needs.  host_request.h has the tables these kernels read and the planner that fills
// them (build_output_plan); launch_output_plan below is the one way they are launched, for the model and for the test hook.
#include "kx_common.h"
#include "adpcm_steps.h"
#include "kweight_coefs.h"
#include "limit_taps.h"
#include "resample_taps.h"
#include "truepeak_taps.h"

namespace kx {

// ---- output packing on device ------------------------------------------------------------------------
// f32 stereo = every sample written twice (koko.rs:1239-1246); PCM16 = (s.clamp(-1,1) * 32767) as i16,
// i.e. truncation toward zero (kokorox-websocket/src/lib.rs:701-704; a NaN: see pcm16_sample).
// `(s.clamp(-1.0, 1.0) * 32767.0) as i16`: the product rounded to f32, truncated toward zero.  nan_to_zero = Rust's meaning
// (clamp keeps a NaN and the cast turns it into 0: form 4); without it the fmaxf / fminf clamp drops the NaN and the sample
// becomes -32767, which is what form 2 has always given (left as it is).
__device__ __forceinline__ int pcm16_sample(float s, bool nan_to_zero) {
    if (nan_to_zero && s != s) return 0;
    const float c = fminf(fmaxf(s, -1.0f), 1.0f);
    return __float2int_rz(__fmul_rn(c, 32767.0f));
}

// ---- requests of several chunks, packed as the bytes a server sends ---------------------------------------------
// A request's region is a function of a VIRTUAL BYTE STREAM: the header of its form, then the sample bytes of its rows in
// order (the chunk loop of koko.rs:947-1191 appends the waveforms with no cross-fade).  Forms 0..2 are the bare samples above
// (the per-utterance entries kx_infer / kx_infer_packed / kx_infer_voices are single-row requests in those forms);
// 3 = `WavHeader::new(1, 24000, 32).write_header` + `to_le_bytes` of every sample (kokorox/src/utils/wav.rs:18-50,
// kokorox-openai/src/lib.rs:416-425: both size fields are the reference's 0xFFFFFFFF placeholders); 4 = standard base64 of a
// 16-bit WAV file (`encode_audio`, kokorox-websocket/src/lib.rs:696-736), whose output group g is stream bytes 3g .. 3g + 2.
//
// One lane writes one 16-byte unit of the output, aligned in the compact buffer (a region starts on a multiple of 4, so its
// first and last unit may be partial: those lanes store single dwords).  A workgroup first copies the window of the
// request's sample stream that its 256 units need into LDS, lanes along time, looking up the row of every sample in the
// batch's prefix table: the conversion then never sees a row boundary, and nothing at or past 600 * frames[b] of a row is
// ever read.  (44 + 1200 k) mod 3 = 2: every chunk boundary of form 4 falls inside a base64 group.
//
// A request with a rate code (PackReq::rate) was resampled as a whole by resample_requests_kernel below: its stream is then
// ONE run of n_samples floats at y + y_off, which the staging step copies instead of looking rows up; the forms apply to it
// exactly as to the model's samples, and the WAV headers carry the chosen rate.  Forms 8 / 9 are G.711 of form 4's 16-bit
// sample, one byte each.
constexpr int PACK_THREADS = 256;
constexpr int PACK_LDS = 4096 + 8;  // samples a workgroup's 4096 output bytes can need: 4096 (G.711), 2048 (PCM16), 1536 + 2 (base64)

__device__ __forceinline__ uint32_t wav_header_dword(int form, long S, int j, int rate_code) {
    const bool f32 = form == 3;
    const uint32_t hz = rate_code == 0 ? 24000u : (rate_code == 1 ? 8000u : (rate_code == 2 ? 16000u : 48000u));
    switch (j) {
        case 0: return 0x46464952u;                                   // "RIFF"
        case 1: return f32 ? 0xFFFFFFFFu : (uint32_t)(36 + 2 * S);   // file size - 8 (placeholder in the float form)
        case 2: return 0x45564157u;                                   // "WAVE"
        case 3: return 0x20746d66u;                                   // "fmt "
        case 4: return 16u;
        case 5: return (f32 ? 3u : 1u) | (1u << 16);                  // format tag (3 = IEEE float, 1 = PCM), 1 channel
        case 6: return hz;
        case 7: return f32 ? 4u * hz : 2u * hz;                       // bytes per second
        case 8: return f32 ? (4u | (32u << 16)) : (2u | (16u << 16));  // block align, bits per sample
        case 9: return 0x61746164u;                                   // "data"
        default: return f32 ? 0xFFFFFFFFu : (uint32_t)(2 * S);
    }
}
__device__ __forceinline__ uint32_t base64_char(uint32_t v) {
    return v < 26u ? 65u + v : (v < 52u ? 71u + v : (v < 62u ? v - 4u : (v == 62u ? 43u : 47u)));
}

// G.711 of a 16-bit sample, the 16-bit-input algorithms of CPython's audioop.lin2ulaw / lin2alaw (include/kokorox_hip.h)
__device__ __forceinline__ uint32_t g711_mulaw(int v) {
    int p = v >> 2;
    const uint32_t mask = p < 0 ? 0x7Fu : 0xFFu;
    p = p < 0 ? -p : p;
    p = (p > 8159 ? 8159 : p) + 33;
    int seg = 0;
    while (seg < 8 && p > (0x40 << seg) - 1) ++seg;  // first segment end 0x3F, 0x7F .. 0x1FFF that holds p
    if (seg == 8) return 0x7Fu ^ mask;
    return (uint32_t)((seg << 4) | ((p >> (seg + 1)) & 15)) ^ mask;
}
__device__ __forceinline__ uint32_t g711_alaw(int v) {
    const uint32_t mask = v >= 0 ? 0xD5u : 0x55u;
    const int p = (v >= 0 ? v : -v - 1) >> 3;
    int seg = 0;
    while (seg < 7 && p > (0x20 << seg) - 1) ++seg;  // (p <= 0xFFF: segment 7 holds whatever is left)
    return (uint32_t)((seg << 4) | ((p >> (seg < 2 ? 1 : seg)) & 15)) ^ mask;
}

// The staging step of the packer and of the resampler: samples [lo, hi) of a request's stream into dst[0 .. hi - lo), lanes
// along time.  Every lane finds the row of its first sample in the batch's prefix table (cum[row] <= g0 + i < cum[row + 1])
// and walks on from there.  Plain: the rows appended, sample o of row b is audio[b ld + o].  JOINED (include/kokorox_hip.h,
// "joins"; host_request.h: JoinRow): cum runs over keep + gap, and offset o of row b is its kept sample skip + o -- times its
// gain when o lies in one of the two fades, which never overlap -- while o < keep, and +0 in the pause behind it.  A fade is
// one float64 division, one float64 product and one rounding, computed here: it needs no storage.  Either way nothing at or
// past 600 * frames[b] of a row is read (skip + keep <= 600 frames[b]), and nothing of a cut region.
__device__ __forceinline__ float join_fade(float v, long i, int n) {
    return (float)((double)v * ((double)(2 * i + 1) / (double)(2 * n)));
}
template <bool JOINED, int THREADS>
__device__ __forceinline__ void stage_stream(float* __restrict__ dst, const float* __restrict__ audio, long audio_ld,
                                             const long* __restrict__ cum, const JoinRow* __restrict__ jrows, int first_row,
                                             int n_rows, long lo_i, long hi_i) {
    const long g0 = cum[first_row];
    const int row_end = first_row + n_rows;
    long i = lo_i + threadIdx.x;
    if (i < hi_i) {
        int lo = first_row, hi = row_end - 1;  // the row of the lane's first sample: cum[row] <= g0 + i < cum[row + 1]
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (cum[mid] <= g0 + i) lo = mid; else hi = mid - 1;
        }
        int row = lo;
        for (; i < hi_i; i += THREADS) {
            while (row + 1 < row_end && cum[row + 1] <= g0 + i) ++row;
            const long o = g0 + i - cum[row];
            if (!JOINED) {
                dst[i - lo_i] = audio[(long)row * audio_ld + o];
            } else {
                const JoinRow jr = jrows[row];
                float v = 0.0f;
                if (o < jr.keep) {
                    v = audio[(long)row * audio_ld + jr.skip + o];
                    if (o < jr.fade_head) v = join_fade(v, o, jr.fade_head);
                    else if (jr.keep - 1 - o < jr.fade_tail) v = join_fade(v, jr.keep - 1 - o, jr.fade_tail);
                }
                dst[i - lo_i] = v;
            }
        }
    }
}

// LEVELLED (include/kokorox_hip.h, "levels"): the staged sample z becomes f32(g * f64(z)) with the request's g from the levels
// block, which request_gain_kernel wrote before this launch; everything behind the barrier sees z' where it saw z.
// LIMITED (include/kokorox_hip.h, "limiter"): a limited request's stream is the run request_limit_kernel left at lim + its offset,
// copied as the resampled run is, with no further gain; a request beside it is staged and scaled as by the levelled form.
template <bool JOINED, bool LEVELLED = false, bool LIMITED = false>
__device__ __forceinline__ void pack_requests_body(const float* __restrict__ audio, long audio_ld,
                                                   const PackReq* __restrict__ reqs, const long* __restrict__ cum,
                                                   const JoinRow* __restrict__ jrows, const float* __restrict__ y,
                                                   char* __restrict__ out, const double* __restrict__ levels = nullptr,
                                                   const LimitRow* __restrict__ lrows = nullptr, const float* __restrict__ lim = nullptr) {
    __shared__ float smp[PACK_LDS];
    const PackReq rq = reqs[blockIdx.y];
    if (rq.form == FORM_ADPCM_WAV) return;  // (uniform: adpcm_blocks_kernel writes that region)
    const long mis = rq.out_off & 15;  // the region starts `mis` bytes into its first 16-byte unit
    const long blk_lo = (long)blockIdx.x * (PACK_THREADS * 16) - mis;
    if (blk_lo >= rq.out_bytes) return;  // (uniform: the grid covers the largest region of the batch)
    const long p_lo = blk_lo < 0 ? 0 : blk_lo;
    const long p_hi = blk_lo + PACK_THREADS * 16 < rq.out_bytes ? blk_lo + PACK_THREADS * 16 : rq.out_bytes;
    const long S = rq.n_samples;
    // samples of the request's stream that output bytes [p_lo, p_hi) depend on
    long s_lo, s_hi;
    if (rq.form == 0) {
        s_lo = p_lo >> 2, s_hi = p_hi >> 2;
    } else if (rq.form == 1) {
        s_lo = p_lo >> 3, s_hi = (p_hi + 7) >> 3;
    } else if (rq.form == 2) {
        s_lo = p_lo >> 1, s_hi = p_hi >> 1;
    } else if (rq.form == 3) {
        s_lo = (p_lo < 44 ? 0 : p_lo - 44) >> 2, s_hi = (p_hi < 44 ? 0 : p_hi - 44) >> 2;
    } else if (rq.form == 4) {
        const long k_lo = (p_lo >> 2) * 3, k_hi = (p_hi >> 2) * 3;  // stream bytes of its groups
        s_lo = (k_lo < 44 ? 0 : k_lo - 44) >> 1, s_hi = (k_hi < 44 ? 0 : k_hi - 43) >> 1;
    } else if (rq.form == FORM_WAV16) {  // (the last dword of an odd S holds one sample and two zero bytes: s_hi is cut to S below)
        s_lo = (p_lo < 44 ? 0 : p_lo - 44) >> 1, s_hi = (p_hi < 44 ? 0 : p_hi - 44) >> 1;
    } else {
        s_lo = p_lo, s_hi = p_hi;
    }
    s_hi = s_hi > S ? S : s_hi;
    long lim_off = -1;
    if (LIMITED) lim_off = lrows[blockIdx.y].off;
    if (LIMITED && lim_off >= 0) {  // (uniform) a limited request: one contiguous run, scaled and limited already
        const float* __restrict__ src = lim + lim_off;
        for (long i = s_lo + threadIdx.x; i < s_hi; i += PACK_THREADS) smp[i - s_lo] = src[i];
    } else if (rq.rate) {  // (uniform) a resampled request: one contiguous run
        const float* __restrict__ src = y + rq.y_off;
        if (LEVELLED) {
            const double g = levels[2 * blockIdx.y + 1];
            for (long i = s_lo + threadIdx.x; i < s_hi; i += PACK_THREADS) smp[i - s_lo] = (float)(g * (double)src[i]);
        } else {
            for (long i = s_lo + threadIdx.x; i < s_hi; i += PACK_THREADS) smp[i - s_lo] = src[i];
        }
    } else {
        stage_stream<JOINED, PACK_THREADS>(smp, audio, audio_ld, cum, jrows, rq.first_row, rq.n_rows, s_lo, s_hi);
        if (LEVELLED) {  // (every lane scales the samples it staged itself: sample i belongs to lane (i - s_lo) mod PACK_THREADS)
            const double g = levels[2 * blockIdx.y + 1];
            for (long i = s_lo + threadIdx.x; i < s_hi; i += PACK_THREADS) smp[i - s_lo] = (float)(g * (double)smp[i - s_lo]);
        }
    }
    __syncthreads();
    const long u_lo = blk_lo + (long)threadIdx.x * 16;  // the lane's unit, as a byte offset in the region (may start before it)
    if (u_lo >= rq.out_bytes) return;
    auto sample = [&](long i) { return smp[i - s_lo]; };
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long p = u_lo + 4 * j;
        uint32_t v = 0;
        if (p >= 0 && p < rq.out_bytes) {
            if (rq.form == 0) {
                v = __float_as_uint(sample(p >> 2));
            } else if (rq.form == 1) {
                v = __float_as_uint(sample(p >> 3));
            } else if (rq.form == 2) {
                v = ((uint32_t)pcm16_sample(sample(p >> 1), false) & 0xFFFFu) | ((uint32_t)pcm16_sample(sample((p >> 1) + 1), false) << 16);
            } else if (rq.form == 3) {
                v = p < 44 ? wav_header_dword(3, S, (int)(p >> 2), rq.rate) : __float_as_uint(sample((p - 44) >> 2));
            } else if (rq.form == FORM_WAV16) {  // form 4's file as bytes: its header, then sample pairs from byte 44, zeros behind sample S - 1
                if (p < 44) {
                    v = wav_header_dword(4, S, (int)(p >> 2), rq.rate);
                } else {
                    const long i = (p - 44) >> 1;
                    v = (uint32_t)pcm16_sample(sample(i), true) & 0xFFFFu;
                    if (i + 1 < S) v |= (uint32_t)pcm16_sample(sample(i + 1), true) << 16;
                }
            } else if (rq.form >= 8) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {  // (a region of G.711 bytes is a multiple of 4 long: p + 3 is inside it)
                    const int pcm = pcm16_sample(sample(p + t), true);
                    v |= (rq.form == 8 ? g711_mulaw(pcm) : g711_alaw(pcm)) << (8 * t);
                }
            } else {
                const long k = (p >> 2) * 3, L = 44 + 2 * S;  // group p / 4 = stream bytes k .. k + 2 of L
                uint32_t b[3];
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const long kk = k + t;
                    if (kk >= L) {
                        b[t] = 0;
                    } else if (kk < 44) {
                        b[t] = (wav_header_dword(4, S, (int)(kk >> 2), rq.rate) >> (8 * (int)(kk & 3))) & 255u;
                    } else {
                        const long d = kk - 44;
                        b[t] = ((uint32_t)pcm16_sample(sample(d >> 1), true) >> (8 * (int)(d & 1))) & 255u;
                    }
                }
                const long n = L - k;  // bytes of this group: 3, or 2 / 1 in the last one ('=' padding)
                const uint32_t c0 = base64_char(b[0] >> 2), c1 = base64_char(((b[0] & 3u) << 4) | (b[1] >> 4));
                const uint32_t c2 = n < 2 ? 61u : base64_char(((b[1] & 15u) << 2) | (b[2] >> 6));
                const uint32_t c3 = n < 3 ? 61u : base64_char(b[2] & 63u);
                v = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
            }
        }
        w[j] = v;
    }
    char* o = out + rq.out_off + u_lo;  // 16-byte aligned: out_off + u_lo = 16 * (unit index) - mis + out_off
    if (u_lo >= 0 && u_lo + 16 <= rq.out_bytes) {
        *reinterpret_cast<uint4*>(o) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long p = u_lo + 4 * j;
            if (p >= 0 && p < rq.out_bytes) *reinterpret_cast<uint32_t*>(o + 4 * j) = w[j];
        }
    }
}
// (three kernels, not one with flags: the plain and the joined form keep their names, their arguments and their registers)
__global__ __launch_bounds__(PACK_THREADS) void pack_requests_kernel(const float* __restrict__ audio, long audio_ld,
                                                                     const PackReq* __restrict__ reqs,
                                                                     const long* __restrict__ cum,
                                                                     const float* __restrict__ y, char* __restrict__ out) {
    pack_requests_body<false>(audio, audio_ld, reqs, cum, nullptr, y, out);
}
__global__ __launch_bounds__(PACK_THREADS) void pack_requests_joined_kernel(const float* __restrict__ audio, long audio_ld,
                                                                            const PackReq* __restrict__ reqs,
                                                                            const long* __restrict__ cum,
                                                                            const JoinRow* __restrict__ jrows,
                                                                            const float* __restrict__ y, char* __restrict__ out) {
    pack_requests_body<true>(audio, audio_ld, reqs, cum, jrows, y, out);
}
// (always the joined staging: the plan fills a JoinRow for every row, {0, 600 frames[b], 0, 0, 0} where nothing shapes it)
__global__ __launch_bounds__(PACK_THREADS) void pack_requests_levelled_kernel(const float* __restrict__ audio, long audio_ld,
                                                                              const PackReq* __restrict__ reqs,
                                                                              const long* __restrict__ cum,
                                                                              const JoinRow* __restrict__ jrows,
                                                                              const float* __restrict__ y, char* __restrict__ out,
                                                                              const double* __restrict__ levels) {
    pack_requests_body<true, true>(audio, audio_ld, reqs, cum, jrows, y, out, levels);
}
// (the limited form: the levelled one, with the limited requests read from the limit buffer)
__global__ __launch_bounds__(PACK_THREADS) void pack_requests_limited_kernel(const float* __restrict__ audio, long audio_ld,
                                                                             const PackReq* __restrict__ reqs,
                                                                             const long* __restrict__ cum,
                                                                             const JoinRow* __restrict__ jrows,
                                                                             const float* __restrict__ y, char* __restrict__ out,
                                                                             const double* __restrict__ levels,
                                                                             const LimitRow* __restrict__ lrows,
                                                                             const float* __restrict__ lim) {
    pack_requests_body<true, true, true>(audio, audio_ld, reqs, cum, jrows, y, out, levels, lrows, lim);
}

// ---- levels: a request's peak, its gain, and the product in the packer's staging step (include/kokorox_hip.h, "levels") ------
// The stream z of request r is what the packer stages: the run at y + y_off with a rate code, the rows through stage_stream
// (joined or plain as the plan says) at 24 000 Hz.  p = the largest |z[n]| over the samples that are no NaN, +inf included, 0 when
// there is none.  For non-NaN floats the unsigned order of bits(|v|) is the order of |v|, so the maximum is taken on dwords: it
// does not depend on the order, and 0 is both the empty maximum and +0.
//
// request_peak_kernel: a workgroup reduces one window of LEVEL_WINDOW samples -- every lane over its samples, the wave with
// __shfl_xor, the four waves through LDS with one barrier -- and stores ONE dword into the partials table [R][windows].  No atomic,
// nothing to zero between calls: request_gain_kernel reads exactly the ceil(N_r / LEVEL_WINDOW) entries this launch wrote.
constexpr int PEAK_THREADS = 256;
__device__ __forceinline__ uint32_t peak_take(uint32_t m, float v) {
    const uint32_t b = __float_as_uint(v) & 0x7FFFFFFFu;
    return b <= 0x7F800000u && b > m ? b : m;  // (a NaN is above +inf in this order: skipped)
}
__global__ __launch_bounds__(PEAK_THREADS) void request_peak_kernel(const float* __restrict__ audio, long audio_ld,
                                                                     const PackReq* __restrict__ reqs, const long* __restrict__ cum,
                                                                     const JoinRow* __restrict__ jrows, const float* __restrict__ y,
                                                                     uint32_t* __restrict__ partials, long windows) {
    __shared__ float xs[LEVEL_WINDOW];
    __shared__ uint32_t wave_max[PEAK_THREADS / 64];
    const PackReq rq = reqs[blockIdx.y];
    const long n0 = (long)blockIdx.x * LEVEL_WINDOW;
    if (n0 >= rq.n_samples) return;  // (uniform: the grid covers the longest request)
    const long n1 = n0 + LEVEL_WINDOW < rq.n_samples ? n0 + LEVEL_WINDOW : rq.n_samples;
    uint32_t m = 0;
    if (rq.rate) {  // (uniform) one contiguous run: 16-byte loads where the window starts on a 16-byte address
        const float* __restrict__ src = y + rq.y_off;
        long tail = n0;
        if ((reinterpret_cast<uintptr_t>(src + n0) & 15) == 0) {
            tail = n0 + ((n1 - n0) & ~3L);
            for (long i = n0 + 4 * (long)threadIdx.x; i < tail; i += 4 * PEAK_THREADS) {
                const float4 v = *reinterpret_cast<const float4*>(src + i);
                m = peak_take(peak_take(peak_take(peak_take(m, v.x), v.y), v.z), v.w);
            }
        }
        for (long i = tail + threadIdx.x; i < n1; i += PEAK_THREADS) m = peak_take(m, src[i]);
    } else {  // the rows, cut and faded as the packer will see them; every lane reads back the samples it staged itself
        if (jrows) stage_stream<true, PEAK_THREADS>(xs, audio, audio_ld, cum, jrows, rq.first_row, rq.n_rows, n0, n1);
        else stage_stream<false, PEAK_THREADS>(xs, audio, audio_ld, cum, jrows, rq.first_row, rq.n_rows, n0, n1);
        for (long i = n0 + threadIdx.x; i < n1; i += PEAK_THREADS) m = peak_take(m, xs[i - n0]);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t v = (uint32_t)__shfl_xor((int)m, o);
        m = v > m ? v : m;
    }
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < PEAK_THREADS / 64; ++w) m = wave_max[w] > m ? wave_max[w] : m;
        partials[(long)blockIdx.y * windows + blockIdx.x] = m;
    }
}
// request_gain_kernel: one wave per request reduces its partials (the windows past its end were never written and are not read),
// computes g in float64 as the header defines it and stores {f64(p), g} into the levels block of the packed buffer.  A spec with
// PEAK_TRUE: the maximum runs over the true-peak partials as well (request_truepeak_kernel wrote that request's row of them), so p
// is tp from here on; the second table is not read for any other request.
__global__ __launch_bounds__(64) void request_gain_kernel(const PackReq* __restrict__ reqs, const LevelSpec* __restrict__ specs,
                                                          const uint32_t* __restrict__ partials,
                                                          const uint32_t* __restrict__ tpartials, long windows,
                                                          double* __restrict__ levels) {
    const int r = blockIdx.x;
    const LevelSpec ls = specs[r];
    const bool true_peak = (ls.mode & PEAK_TRUE) != 0;  // (the whole wave)
    const long n = (reqs[r].n_samples + LEVEL_WINDOW - 1) / LEVEL_WINDOW;
    uint32_t m = 0;
    for (long w = threadIdx.x; w < n; w += 64) {
        const uint32_t v = partials[(long)r * windows + w];
        m = v > m ? v : m;
        if (true_peak) {
            const uint32_t u = tpartials[(long)r * windows + w];
            m = u > m ? u : m;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t v = (uint32_t)__shfl_xor((int)m, o);
        m = v > m ? v : m;
    }
    if (threadIdx.x != 0) return;
    const uint32_t mode = ls.mode & ~PEAK_TRUE;
    const double p = (double)__uint_as_float(m), peak = (double)ls.peak;
    const bool usable = m > 0u && m < 0x7F800000u;
    double g = (double)ls.gain;
    if (mode == LEVEL_NORMALIZE) g = usable ? peak / p : 1.0;
    else if (mode == LEVEL_CEILING && usable && g * p > peak) g = peak / p;
    levels[2 * r] = p;
    levels[2 * r + 1] = g;
}

// ---- true peak: the largest value of the stream four times oversampled (include/kokorox_hip.h, "levels": PEAK_TRUE) ------------
// For phi = 1..3, u_phi[n] = f32(sum over j = n - 11 .. n + 12 ascending of f64(t_phi[n - j + 12]) x[j]), x the stream with zeros
// outside [0, N) and where z is not finite; tp = max(p, max |u_phi[n]|).  A float32 x float32 product is exact in float64, so the
// fused and the unfused form give the same bits and a host loop in the same order reproduces every u (voices.py: true_peak).
//
// request_truepeak_kernel: workgroup (w, r) owns the samples [4096 w, min(4096 (w + 1), N)) of request r -- the windows of the peak
// pass -- and stages them with a halo of 11 before and 12 behind into LDS, +0 for every index outside the stream: nothing outside
// the request's own run of y is read, nothing at or past 600 * frames[b] of a row.  The 72 taps sit beside them as float64.  Lane
// t takes the samples t + 256 k, eight of them at a time: 24 float64 chains in registers, the tap index running downwards as j
// runs upwards; a step reads three taps (one address for the wave: a broadcast) and eight inputs (consecutive dwords across the
// lanes) for 24 multiply-adds.  The three phases of a sample are independent chains, each in its ascending order.  The maximum is
// taken on dwords as in the peak pass, and ONE dword per workgroup goes into the second partials table: the gain kernels join it
// with the first.  A request whose governing spec lacks the flag returns at once; its row of the table is neither written nor read.
constexpr int TP_THREADS = 256;
constexpr int TP_BEFORE = TRUEPEAK_NTAPS / 2 - 1, TP_BEHIND = TRUEPEAK_NTAPS / 2;  // j = n - 11 .. n + 12
constexpr int TP_LDS = (int)LEVEL_WINDOW + TP_BEFORE + TP_BEHIND;                    // 4119 floats
constexpr int TP_GROUP = 8;                                                          // samples of a lane in flight
static_assert(LEVEL_WINDOW % (TP_THREADS * TP_GROUP) == 0 && KX_TRUEPEAK_PHASES == 3 && KX_TRUEPEAK_NTAPS == 24, "whole groups, [3][24] taps");
__device__ const uint32_t truepeak_tap_bits[TRUEPEAK_PHASES * TRUEPEAK_NTAPS] = {KX_TRUEPEAK_TAPS_1, KX_TRUEPEAK_TAPS_2, KX_TRUEPEAK_TAPS_3};
// The 24-tap interpolation of TP_GROUP samples of a lane, TP_THREADS apart: sample k reads xp[TP_THREADS k + 0 .. 23], its inputs
// j = n - 11 .. n + 12 ascending, and ts holds the 72 taps as float64.  request_truepeak_kernel and request_limit_kernel share it.
__device__ __forceinline__ void truepeak_chains(const float* __restrict__ xp, const double* __restrict__ ts,
                                                double (&acc)[TRUEPEAK_PHASES][TP_GROUP]) {
#pragma unroll
    for (int f = 0; f < TRUEPEAK_PHASES; ++f)
#pragma unroll
        for (int k = 0; k < TP_GROUP; ++k) acc[f][k] = 0.0;
#pragma unroll 4
    for (int jj = 0; jj < TRUEPEAK_NTAPS; ++jj) {  // j = n - 11 + jj ascending: tap n - j + 12 = 23 - jj
        const double t1 = ts[TRUEPEAK_NTAPS - 1 - jj], t2 = ts[2 * TRUEPEAK_NTAPS - 1 - jj], t3 = ts[3 * TRUEPEAK_NTAPS - 1 - jj];
#pragma unroll
        for (int k = 0; k < TP_GROUP; ++k) {
            const double x = (double)xp[TP_THREADS * k + jj];
            acc[0][k] += t1 * x;
            acc[1][k] += t2 * x;
            acc[2][k] += t3 * x;
        }
    }
}

__global__ __launch_bounds__(TP_THREADS) void request_truepeak_kernel(const float* __restrict__ audio, long audio_ld,
                                                                       const PackReq* __restrict__ reqs, const long* __restrict__ cum,
                                                                       const JoinRow* __restrict__ jrows, const float* __restrict__ y,
                                                                       const LevelSpec* __restrict__ levels,
                                                                       const LoudSpec* __restrict__ louds,
                                                                       uint32_t* __restrict__ tpartials, long windows) {
    __shared__ float xs[TP_LDS];
    __shared__ double ts[TRUEPEAK_PHASES * TRUEPEAK_NTAPS];
    __shared__ uint32_t wave_max[TP_THREADS / 64];
    // the governing spec: the loudness spec of a metered request (LOUD_NONE has the flag's bit set: asked first), else the level spec
    const uint32_t lmode = louds ? louds[blockIdx.y].mode : LOUD_NONE;
    const uint32_t mode = lmode != LOUD_NONE ? lmode : levels[blockIdx.y].mode;
    if ((mode & PEAK_TRUE) == 0) return;  // (uniform) a request beside the flagged ones
    const PackReq rq = reqs[blockIdx.y];
    const long N = rq.n_samples;
    const long n0 = (long)blockIdx.x * LEVEL_WINDOW;
    if (n0 >= N) return;  // (uniform: the grid covers the longest request)
    const long n1 = n0 + LEVEL_WINDOW < N ? n0 + LEVEL_WINDOW : N;
    // the window: local index i is sample n0 - 11 + i of the stream, i < T; [s_lo, s_hi) of them are inside it, zeros around
    const long w_lo = n0 - TP_BEFORE, T = n1 - n0 + TP_BEFORE + TP_BEHIND;
    const long s_lo = w_lo < 0 ? 0 : w_lo, s_hi = n1 + TP_BEHIND < N ? n1 + TP_BEHIND : N;
    const long front = s_lo - w_lo, back = s_hi - w_lo;  // front <= 11; T - back <= 12
    for (long i = threadIdx.x; i < front; i += TP_THREADS) xs[i] = 0.0f;
    for (long i = back + threadIdx.x; i < T; i += TP_THREADS) xs[i] = 0.0f;
    float* __restrict__ dst = xs + front;
    auto finite = [](float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; };
    if (rq.rate) {  // (uniform) one contiguous run
        const float* __restrict__ src = y + rq.y_off;
        for (long i = s_lo + threadIdx.x; i < s_hi; i += TP_THREADS) {
            const float v = src[i];
            dst[i - s_lo] = finite(v) ? v : 0.0f;
        }
    } else {  // the rows, cut and faded as the packer will see them; every lane checks the samples it staged itself
        if (jrows) stage_stream<true, TP_THREADS>(dst, audio, audio_ld, cum, jrows, rq.first_row, rq.n_rows, s_lo, s_hi);
        else stage_stream<false, TP_THREADS>(dst, audio, audio_ld, cum, jrows, rq.first_row, rq.n_rows, s_lo, s_hi);
        for (long i = s_lo + threadIdx.x; i < s_hi; i += TP_THREADS)
            if (!finite(dst[i - s_lo])) dst[i - s_lo] = 0.0f;
    }
    if (threadIdx.x < TRUEPEAK_PHASES * TRUEPEAK_NTAPS) ts[threadIdx.x] = (double)__uint_as_float(truepeak_tap_bits[threadIdx.x]);
    __syncthreads();
    const int count = (int)(n1 - n0);
    uint32_t m = 0;
    // (a group past the window's end is skipped by the whole wave; inside the last group a lane past the end computes on LDS
    // that nobody staged, inside xs, and its values are dropped)
    for (int base = 0; base < (int)LEVEL_WINDOW; base += TP_THREADS * TP_GROUP) {
        if (base + (int)(threadIdx.x & ~63u) >= count) break;
        const float* __restrict__ xp = xs + base + threadIdx.x;  // sample n0 + base + t + 256 k reads xp[256 k + 0 .. 23]
        double acc[TRUEPEAK_PHASES][TP_GROUP];
        truepeak_chains(xp, ts, acc);
#pragma unroll
        for (int k = 0; k < TP_GROUP; ++k) {
            if (base + (int)threadIdx.x + TP_THREADS * k < count) {
#pragma unroll
                for (int f = 0; f < TRUEPEAK_PHASES; ++f) m = peak_take(m, (float)acc[f][k]);
            }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t v = (uint32_t)__shfl_xor((int)m, o);
        m = v > m ? v : m;
    }
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < TP_THREADS / 64; ++w) m = wave_max[w] > m ? wave_max[w] : m;
        tpartials[(long)blockIdx.y * windows + blockIdx.x] = m;
    }
}

// ---- loudness: BS.1770 K-weighting, hop energies, gating and the gain (include/kokorox_hip.h, "loudness") ---------------------
// The stream z is the one the peak pass reads; x[n] = f64(z[n]) where z[n] is finite, else 0.  The K-weighting is two biquads in
// direct form I (kweight_coefs.h), so beside the input the recurrence carries s = (v[n-1], v[n-2], w[n-1], w[n-2]), and with the
// input switched off one step is s <- A s with a 4x4 matrix A.
//
// request_loudness_kernel: workgroup (k, r) owns hop k of request r (loud_hop samples, 100 ms) and stores its energy e[k], the sum
// of w[n]^2, as ONE double into the table [R][max_hops].  It stages the hop and the loud_warmup samples before it (zeros before the
// stream's start) into LDS and runs the recurrence over those T samples from zero state as a scan: lane t takes the `run` samples
// from t * run (run is odd: lanes are run dwords apart, on distinct banks), first from zero state, which leaves q_t; the true end
// states follow from s_(t+1) = A^run s_t + q_t, one __shfl_up ladder per wave with the host's powers A^(run o) and one exchange of
// the four wave states through LDS; then every lane runs its samples again from its true start state and sums w^2 over those of
// the hop.  The sum over the lanes is a __shfl_xor tree and a fixed walk over the four waves.  Every boundary is a function of the
// request's own sample index, so e[k] does not depend on the batch; no atomic, nothing to zero between calls.
constexpr int LOUD_LDS = 8192 + 4800;  // loud_warmup + loud_hop at 48 000 Hz, the largest
static_assert(loud_warmup(0) + loud_hop(0) <= LOUD_LDS && loud_warmup(1) + loud_hop(1) <= LOUD_LDS && loud_warmup(2) + loud_hop(2) <= LOUD_LDS &&
                  loud_warmup(3) + loud_hop(3) == LOUD_LDS && LOUD_THREADS == 256,
              "the staged window fits, four waves");
static_assert((long)LOUD_THREADS * loud_run(0) >= loud_warmup(0) + loud_hop(0) && (long)LOUD_THREADS * loud_run(1) >= loud_warmup(1) + loud_hop(1) &&
                  (long)LOUD_THREADS * loud_run(2) >= loud_warmup(2) + loud_hop(2) && (long)LOUD_THREADS * loud_run(3) >= loud_warmup(3) + loud_hop(3),
              "the lanes' runs cover the window");
__device__ const unsigned long long kweight_bits[4][10] = {{KX_KWEIGHT_COEFS_24000}, {KX_KWEIGHT_COEFS_8000}, {KX_KWEIGHT_COEFS_16000}, {KX_KWEIGHT_COEFS_48000}};

struct KwState {
    double v1, v2, w1, w2;
};
// s += P t, P row-major 4x4
__device__ __forceinline__ void kw_apply(KwState& s, const double* __restrict__ P, const KwState& t) {
    s.v1 += P[0] * t.v1 + P[1] * t.v2 + P[2] * t.w1 + P[3] * t.w2;
    s.v2 += P[4] * t.v1 + P[5] * t.v2 + P[6] * t.w1 + P[7] * t.w2;
    s.w1 += P[8] * t.v1 + P[9] * t.v2 + P[10] * t.w1 + P[11] * t.w2;
    s.w2 += P[12] * t.v1 + P[13] * t.v2 + P[14] * t.w1 + P[15] * t.w2;
}
// samples [lo, hi) of the staged window through the cascade, from state s (the two inputs before lo are read from the window);
// returns the sum of w^2 over the samples at or past `from`
__device__ __forceinline__ double kw_run(const float* __restrict__ xs, long lo, long hi, long from, const double* __restrict__ k, KwState& s) {
    double x1 = lo >= 1 ? (double)xs[lo - 1] : 0.0, x2 = lo >= 2 ? (double)xs[lo - 2] : 0.0, acc = 0.0;
    for (long n = lo; n < hi; ++n) {
        const double x = (double)xs[n];
        const double v = k[0] * x + k[1] * x1 + k[2] * x2 - k[3] * s.v1 - k[4] * s.v2;
        const double w = k[5] * v + k[6] * s.v1 + k[7] * s.v2 - k[8] * s.w1 - k[9] * s.w2;
        x2 = x1, x1 = x;
        s.v2 = s.v1, s.v1 = v;
        s.w2 = s.w1, s.w1 = w;
        if (n >= from) acc += w * w;
    }
    return acc;
}
__global__ __launch_bounds__(LOUD_THREADS) void request_loudness_kernel(const float* __restrict__ audio, long audio_ld,
                                                                         const PackReq* __restrict__ reqs, const long* __restrict__ cum,
                                                                         const JoinRow* __restrict__ jrows, const float* __restrict__ y,
                                                                         const LoudSpec* __restrict__ specs,
                                                                         const double* __restrict__ powers, double* __restrict__ hops,
                                                                         long max_hops) {
    __shared__ float xs[LOUD_LDS];
    __shared__ double wave_state[LOUD_THREADS / 64][4];
    __shared__ double wave_sum[LOUD_THREADS / 64];
    if (specs[blockIdx.y].mode == LOUD_NONE) return;  // (uniform) a request beside the metered ones
    const PackReq rq = reqs[blockIdx.y];
    const long hop = loud_hop(rq.rate), W = loud_warmup(rq.rate), T = W + hop;
    const int run = loud_run(rq.rate);
    const long h0 = (long)blockIdx.x * hop;
    if (h0 + hop > rq.n_samples) return;  // (uniform: the grid covers the request with most hops; a partial hop is ignored)
    // the window: local index i is sample h0 - W + i of the stream; the first `zeros` of them lie before its start
    const long zeros = h0 < W ? W - h0 : 0, s_lo = h0 - W + zeros, s_hi = h0 + hop;
    for (long i = threadIdx.x; i < zeros; i += LOUD_THREADS) xs[i] = 0.0f;
    float* __restrict__ dst = xs + zeros;
    auto finite = [](float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; };
    if (rq.rate) {  // (uniform) one contiguous run
        const float* __restrict__ src = y + rq.y_off;
        for (long i = s_lo + threadIdx.x; i < s_hi; i += LOUD_THREADS) {
            const float v = src[i];
            dst[i - s_lo] = finite(v) ? v : 0.0f;
        }
    } else {  // the rows, cut and faded as the packer will see them; every lane checks the samples it staged itself
        if (jrows) stage_stream<true, LOUD_THREADS>(dst, audio, audio_ld, cum, jrows, rq.first_row, rq.n_rows, s_lo, s_hi);
        else stage_stream<false, LOUD_THREADS>(dst, audio, audio_ld, cum, jrows, rq.first_row, rq.n_rows, s_lo, s_hi);
        for (long i = s_lo + threadIdx.x; i < s_hi; i += LOUD_THREADS)
            if (!finite(dst[i - s_lo])) dst[i - s_lo] = 0.0f;
    }
    __syncthreads();
    double k[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) k[i] = __longlong_as_double((long long)kweight_bits[rq.rate][i]);
    const double* __restrict__ P = powers + (long)rq.rate * LOUD_POWERS * 16;  // P + 16 o = A^(run o)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long lo = (long)threadIdx.x * run < T ? (long)threadIdx.x * run : T, hi = lo + run < T ? lo + run : T;
    // first pass, from zero state: q of the lane, then the inclusive scan inside the wave
    KwState incl{0.0, 0.0, 0.0, 0.0};
    (void)kw_run(xs, lo, hi, T, k, incl);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const KwState up{__shfl_up(incl.v1, o), __shfl_up(incl.v2, o), __shfl_up(incl.w1, o), __shfl_up(incl.w2, o)};
        if (lane >= o) kw_apply(incl, P + 16 * o, up);
    }
    if (lane == 63) {
        wave_state[wave][0] = incl.v1, wave_state[wave][1] = incl.v2, wave_state[wave][2] = incl.w1, wave_state[wave][3] = incl.w2;
    }
    // the lane's start state inside its wave: the end state of the lane before it
    KwState start{__shfl_up(incl.v1, 1), __shfl_up(incl.v2, 1), __shfl_up(incl.w1, 1), __shfl_up(incl.w2, 1)};
    if (lane == 0) start = KwState{0.0, 0.0, 0.0, 0.0};
    __syncthreads();
    // the state the wave starts from: c_0 = 0, c_(w+1) = A^(64 run) c_w + the end state of wave w alone; it reaches the lane through A^(run lane)
    KwState carry{0.0, 0.0, 0.0, 0.0};
    for (int w = 0; w < wave; ++w) {
        KwState next{wave_state[w][0], wave_state[w][1], wave_state[w][2], wave_state[w][3]};
        kw_apply(next, P + 16 * 64, carry);
        carry = next;
    }
    kw_apply(start, P + 16 * lane, carry);
    // second pass, from the true state: the energy of the hop's samples
    double acc = kw_run(xs, lo, hi, W, k, start);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) wave_sum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < LOUD_THREADS / 64; ++w) acc += wave_sum[w];
        hops[(long)blockIdx.y * max_hops + blockIdx.x] = acc;
    }
}
// request_loudness_gain_kernel: one wave per metered request.  It reduces the peak partials as request_gain_kernel does (with
// PEAK_TRUE in its spec over both tables, so that p is tp), forms the 400 ms block means z_j from the hop energies, applies the two
// gates in the energy domain, every lane over j = lane, lane + 64, ..
// and the wave with a __shfl_xor tree (a fixed order: the same bits run to run), and stores {f64(p), g} into the request's slot of the
// levels block and {I, f64(n_g)} into the loudness block behind it.
__device__ __forceinline__ void loud_gate(const double* __restrict__ e, long J, double scale, double floor_, double& sum, int& count) {
    double s = 0.0;
    int c = 0;
    for (long j = threadIdx.x; j < J; j += 64) {
        const double z = (e[j] + e[j + 1] + e[j + 2] + e[j + 3]) / scale;
        if (z > LOUD_ABS_GATE && z > floor_) s += z, c += 1;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o), c += __shfl_xor(c, o);
    sum = s, count = c;
}
__global__ __launch_bounds__(64) void request_loudness_gain_kernel(const PackReq* __restrict__ reqs, const LoudSpec* __restrict__ specs,
                                                                   const uint32_t* __restrict__ partials,
                                                                   const uint32_t* __restrict__ tpartials, long windows,
                                                                   const double* __restrict__ hops, long max_hops,
                                                                   double* __restrict__ levels, double* __restrict__ loud) {
    const int r = blockIdx.x;
    const LoudSpec ls = specs[r];
    if (ls.mode == LOUD_NONE) return;  // (the whole wave: its slot is request_gain_kernel's)
    const bool true_peak = (ls.mode & PEAK_TRUE) != 0;  // (the whole wave, and behind LOUD_NONE, which has the bit set)
    const long n = (reqs[r].n_samples + LEVEL_WINDOW - 1) / LEVEL_WINDOW;
    uint32_t m = 0;
    for (long w = threadIdx.x; w < n; w += 64) {
        const uint32_t v = partials[(long)r * windows + w];
        m = v > m ? v : m;
        if (true_peak) {
            const uint32_t u = tpartials[(long)r * windows + w];
            m = u > m ? u : m;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t v = (uint32_t)__shfl_xor((int)m, o);
        m = v > m ? v : m;
    }
    const long hop = loud_hop(reqs[r].rate), J = reqs[r].n_samples / hop - 3;  // (J < 1: no block, nothing of the table is read)
    const double* __restrict__ e = hops + (long)r * max_hops;
    const double scale = 4.0 * (double)hop;
    double s1, s2 = 0.0;
    int c1, c2 = 0;
    loud_gate(e, J, scale, 0.0, s1, c1);
    if (c1 > 0) loud_gate(e, J, scale, 0.1 * (s1 / (double)c1), s2, c2);
    if (threadIdx.x != 0) return;
    const double I = c2 > 0 ? -0.691 + 10.0 * log10(s2 / (double)c2) : __longlong_as_double(0x7FF8000000000000LL);
    const double p = (double)__uint_as_float(m), peak = (double)ls.peak;
    const bool usable = m > 0u && m < 0x7F800000u;
    double g = 1.0;
    if ((ls.mode & ~PEAK_TRUE) == LOUD_NORMALIZE) {
        if (c2 > 0) g = pow(10.0, ((double)ls.target_lufs - I) / 20.0);
        if (usable && g * p > peak) g = peak / p;
    }
    levels[2 * r] = p;
    levels[2 * r + 1] = g;
    loud[2 * r] = I;
    loud[2 * r + 1] = (double)c2;
}

// ---- output sample rates: a request's whole stream through a polyphase FIR, before the packer -----------------------------
// For rate code c the ratio is L / M ((1, 3), (2, 3), (2, 1)), C = 24 max(L, M), N = 2 C + 1 taps h (resample_taps.h), and
//     y[n] = f32( sum over j ascending, 0 <= j < S, 0 <= n M - j L + C < N, of f64(h[n M - j L + C]) * f64(x[j]) )
// with a float64 accumulator from +0, one addition per term and one round-to-nearest-even conversion at the end: a product
// of two float32 values is exact in float64, so a fused multiply-add and a multiply and an add give the same bits, and a
// host loop in the same order reproduces y bit for bit (kokorox_amd/voices.py: resample_stream).  x is the request's stream
// as the packer defines it: a chunk boundary is invisible, and nothing at or past 600 * frames[b] of a row is read.
//
// A workgroup owns RS_WINDOW consecutive outputs of one request, lane t the outputs n0 + t + 256 k.  It stages the inputs
// those outputs touch into LDS with the packer's row lookup, and the taps as float64; every lane then runs its chains out
// of LDS.  Neighbouring lanes read inputs 3 (8 kHz), 1 or 2 (16 kHz) and 0 or 1 (48 kHz) dwords apart: conflict-free, at
// most two-way, and pairwise broadcast; the taps are one address per phase.
constexpr int RS_THREADS = 256;
constexpr int RS_WINDOW = 1024;
constexpr int RS_MAX_TAPS = KX_RESAMPLE_NTAPS_8000;
// inputs of a window: floor(((n0 + 1023) M + C) / L) - ceil((n0 M - C) / L) + 1 <= (1023 M + 2 C) / L + 1 = 3214 at 8 kHz
constexpr int RS_LDS = 3 * (RS_WINDOW - 1) + (RS_MAX_TAPS - 1) + 1 + 2;
static_assert(KX_RESAMPLE_NTAPS_16000 <= RS_MAX_TAPS && KX_RESAMPLE_NTAPS_48000 <= RS_MAX_TAPS, "the 8 kHz table is the longest");
__device__ const uint32_t resample_tap_bits[3][RS_MAX_TAPS] = {{KX_RESAMPLE_TAPS_8000}, {KX_RESAMPLE_TAPS_16000}, {KX_RESAMPLE_TAPS_48000}};

template <bool JOINED>
__device__ __forceinline__ void resample_requests_body(const float* __restrict__ audio, long audio_ld,
                                                       const PackReq* __restrict__ reqs, const long* __restrict__ cum,
                                                       const JoinRow* __restrict__ jrows, float* __restrict__ y) {
    __shared__ float xs[RS_LDS];
    __shared__ double hs[RS_MAX_TAPS];
    const PackReq rq = reqs[blockIdx.y];
    if (rq.rate == 0) return;  // (uniform) a request at 24 kHz: the packer reads the model's slab
    const long n0 = (long)blockIdx.x * RS_WINDOW;
    if (n0 >= rq.n_samples) return;  // (uniform: the grid covers the longest resampled request)
    const long n1 = n0 + RS_WINDOW < rq.n_samples ? n0 + RS_WINDOW : rq.n_samples;
    const int L = rq.rate == 1 ? 1 : 2, M = rq.rate == 3 ? 1 : 3, C = rq.rate == 3 ? 48 : 72, N = 2 * C + 1;
    const long S = rq.src_samples;
    // inputs some output of [n0, n1) touches: ceil((n0 M - C) / L) .. floor(((n1 - 1) M + C) / L), inside the stream
    const long a_lo = n0 * M - C;
    const long j_lo = a_lo <= 0 ? 0 : (a_lo + L - 1) / L;
    long j_hi = ((n1 - 1) * M + C) / L + 1;
    j_hi = j_hi > S ? S : j_hi;
    for (int t = threadIdx.x; t < N; t += RS_THREADS) hs[t] = (double)__uint_as_float(resample_tap_bits[rq.rate - 1][t]);
    stage_stream<JOINED, RS_THREADS>(xs, audio, audio_ld, cum, jrows, rq.first_row, rq.n_rows, j_lo, j_hi);
    __syncthreads();
    float* __restrict__ dst = y + rq.y_off;
    for (long n = n0 + threadIdx.x; n < n1; n += RS_THREADS) {
        const long a = n * M - C;
        const long jl = a <= 0 ? 0 : (a + L - 1) / L;  // >= j_lo, as n >= n0
        long jh = (n * M + C) / L;                      // < j_hi, as n < n1
        jh = jh > S - 1 ? S - 1 : jh;
        int idx = (int)(n * M - jl * L) + C;            // <= 2 C, as jl L >= n M - C; stays >= 0 down to j = jh
        const float* xp = xs + (jl - j_lo);
        double acc = 0.0;
        for (long j = jl; j <= jh; ++j, idx -= L) acc += hs[idx] * (double)*xp++;
        dst[n] = (float)acc;
    }
}
__global__ __launch_bounds__(RS_THREADS) void resample_requests_kernel(const float* __restrict__ audio, long audio_ld,
                                                                        const PackReq* __restrict__ reqs,
                                                                        const long* __restrict__ cum, float* __restrict__ y) {
    resample_requests_body<false>(audio, audio_ld, reqs, cum, nullptr, y);
}
__global__ __launch_bounds__(RS_THREADS) void resample_requests_joined_kernel(const float* __restrict__ audio, long audio_ld,
                                                                               const PackReq* __restrict__ reqs,
                                                                               const long* __restrict__ cum,
                                                                               const JoinRow* __restrict__ jrows,
                                                                               float* __restrict__ y) {
    resample_requests_body<true>(audio, audio_ld, reqs, cum, jrows, y);
}

// ---- pieces: a request resampled in several calls (include/kokorox_hip.h, "pieces"; host_request.h: PieceRow, PieceCarry) --------
// The resampler of a plan with pieces, for every request of it.  A piece's source is tail_in ++ its joined rows: samples
// [A' - n_tail_in, A') and [A', A) of the whole request's stream x, and it writes the outputs [E', E) of the whole request's y to
// y + y_off.  Every index below is one of the whole request's, so the taps an output meets, their order (j ascending over the terms
// that exist: no sample before x[0], none at or past A), the float64 accumulator from +0 and the one rounding are those of
// resample_requests_body on the whole stream: the same bits.  A request run whole is the piece [0, N) of [0, S) without a tail.
// The window is staged as there, the carried tail first and the rows behind it through the row lookup, plain or JOINED as the plan
// says; PIECE_TAIL guarantees that no output of [E', E) reads before A' - n_tail_in, and an index that did would read +0, never
// outside the tail buffer.
template <bool JOINED>
__device__ __forceinline__ void resample_pieces_body(const float* __restrict__ audio, long audio_ld,
                                                                      const PackReq* __restrict__ reqs,
                                                                      const PieceRow* __restrict__ pieces,
                                                                      const long* __restrict__ cum,
                                                                      const JoinRow* __restrict__ jrows,
                                                                      const float* __restrict__ tails, float* __restrict__ y) {
    __shared__ float xs[RS_LDS];
    __shared__ double hs[RS_MAX_TAPS];
    const PackReq rq = reqs[blockIdx.y];
    if (rq.rate == 0) return;  // (uniform) a request at 24 kHz: the packer reads the model's slab
    const PieceRow pr = pieces[blockIdx.y];
    const long n0 = pr.emit_lo + (long)blockIdx.x * RS_WINDOW;
    if (n0 >= pr.emit_hi) return;  // (uniform: the grid covers the request with most outputs in this call)
    const long n1 = n0 + RS_WINDOW < pr.emit_hi ? n0 + RS_WINDOW : pr.emit_hi;
    const int L = rq.rate == 1 ? 1 : 2, M = rq.rate == 3 ? 1 : 3, C = rq.rate == 3 ? 48 : 72, N = 2 * C + 1;
    const long S = pr.src_end;  // the stream so far: a term at or past it does not exist (no final output has one)
    const long a_lo = n0 * M - C;
    const long j_lo = a_lo <= 0 ? 0 : (a_lo + L - 1) / L;
    long j_hi = ((n1 - 1) * M + C) / L + 1;
    j_hi = j_hi > S ? S : j_hi;
    for (int t = threadIdx.x; t < N; t += RS_THREADS) hs[t] = (double)__uint_as_float(resample_tap_bits[rq.rate - 1][t]);
    // the carried tail: x[base .. A'), then the piece's own rows: x[A' .. A)
    const long base = pr.src_before - pr.n_tail_in;
    const long t_hi = j_hi < pr.src_before ? j_hi : pr.src_before;
    for (long j = j_lo + threadIdx.x; j < t_hi; j += RS_THREADS) xs[j - j_lo] = j >= base ? tails[pr.tail_in + (j - base)] : 0.0f;
    const long r_lo = j_lo > pr.src_before ? j_lo : pr.src_before;
    if (r_lo < j_hi)
        stage_stream<JOINED, RS_THREADS>(xs + (r_lo - j_lo), audio, audio_ld, cum, jrows, rq.first_row, rq.n_rows, r_lo - pr.src_before,
                                         j_hi - pr.src_before);
    __syncthreads();
    float* __restrict__ dst = y + rq.y_off;
    for (long n = n0 + threadIdx.x; n < n1; n += RS_THREADS) {
        const long a = n * M - C;
        const long jl = a <= 0 ? 0 : (a + L - 1) / L;  // >= j_lo, as n >= n0
        long jh = (n * M + C) / L;                      // < j_hi, as n < n1
        jh = jh > S - 1 ? S - 1 : jh;
        int idx = (int)(n * M - jl * L) + C;
        const float* xp = xs + (jl - j_lo);
        double acc = 0.0;
        for (long j = jl; j <= jh; ++j, idx -= L) acc += hs[idx] * (double)*xp++;
        dst[n - pr.emit_lo] = (float)acc;
    }
}
__global__ __launch_bounds__(RS_THREADS) void resample_pieces_kernel(const float* __restrict__ audio, long audio_ld,
                                                                      const PackReq* __restrict__ reqs,
                                                                      const PieceRow* __restrict__ pieces,
                                                                      const long* __restrict__ cum, const float* __restrict__ tails,
                                                                      float* __restrict__ y) {
    resample_pieces_body<false>(audio, audio_ld, reqs, pieces, cum, nullptr, tails, y);
}
__global__ __launch_bounds__(RS_THREADS) void resample_pieces_joined_kernel(const float* __restrict__ audio, long audio_ld,
                                                                             const PackReq* __restrict__ reqs,
                                                                             const PieceRow* __restrict__ pieces,
                                                                             const long* __restrict__ cum,
                                                                             const JoinRow* __restrict__ jrows,
                                                                             const float* __restrict__ tails, float* __restrict__ y) {
    resample_pieces_body<true>(audio, audio_ld, reqs, pieces, cum, jrows, tails, y);
}
// The carry a piece leaves, one workgroup of PIECE_TAIL lanes per request: lane t stores sample t of the new tail, the last
// n_tail_out samples of tail_in ++ joined rows -- the last of the piece's own kept samples, staged through the joined row lookup, and
// in front of them, where the piece kept fewer than n_tail_out, the last of the old tail -- and +0 behind them; lane 0 the record's
// head.  A request run whole gets the all-zero record.
__global__ __launch_bounds__(PIECE_TAIL) void piece_carry_kernel(const float* __restrict__ audio, long audio_ld,
                                                                  const PackReq* __restrict__ reqs,
                                                                  const PieceRow* __restrict__ pieces, const long* __restrict__ cum,
                                                                  const JoinRow* __restrict__ jrows,
                                                                  const float* __restrict__ tails, char* __restrict__ out) {
    __shared__ float xs[PIECE_TAIL];
    const PackReq rq = reqs[blockIdx.x];
    const PieceRow pr = pieces[blockIdx.x];
    PieceCarry* __restrict__ c = reinterpret_cast<PieceCarry*>(out + pr.carry_off);
    const bool piece = pr.flags != PIECE_WHOLE;
    const int t = threadIdx.x;
    const long own = pr.src_end - pr.src_before;                       // the piece's joined samples
    const int n_out = piece ? pr.n_tail_out : 0;
    const int from_rows = own < (long)n_out ? (int)own : n_out;        // (uniform)
    const int from_tail = n_out - from_rows;                           // <= n_tail_in: A' >= n_out - own
    if (from_rows > 0) stage_stream<true, PIECE_TAIL>(xs, audio, audio_ld, cum, jrows, rq.first_row, rq.n_rows, own - from_rows, own);
    __syncthreads();
    float v = 0.0f;
    if (t < from_tail) v = pr.n_tail_in - from_tail + t >= 0 ? tails[pr.tail_in + pr.n_tail_in - from_tail + t] : 0.0f;
    else if (t < n_out) v = xs[t - from_tail];
    c->tail[t] = v;
    if (t == 0) {
        c->magic = piece ? PIECE_MAGIC : 0u;
        c->format_word = piece ? pr.word : 0u;
        c->src_samples = piece ? pr.src_end : 0;
        c->out_samples = piece ? pr.emit_hi : 0;
        c->n_tail = n_out;
        c->reserved = piece ? pr.chunks_end : 0;
    }
}

// ---- limiter: a look-ahead gain that keeps every sample at or below the request's peak (include/kokorox_hip.h, "limiter") ------
// The stream z is the one the peak pass reads and g its drive from the levels block (the gain kernels ran before: a limited request's
// derived spec carries the drive cap).  z1[n] = f32(g f64(z[n])); a[n] = |z1[n]|, with PEAK_TRUE the largest of it and the three
// interpolated values either side, non-finite values as 0; c[n] = 1 where a[n] <= peak, else f32(f64(peak) / f64(a[n])), and 1 outside
// the stream; m[j] = min of c over [j - W, j + W]; s[n] = sum over j = n - W .. n + W ascending of f64(h[j - n + W]) f64(m[j]), a float64
// accumulator from +0 (1.0 where every m of the sum is 1.0f); z2[n] = f32(s[n] f64(z1[n])), clamped to +-peak.
//
// request_limit_kernel: workgroup (w, r) owns the samples [4096 w, min(4096 (w + 1), N)) of request r, the windows of the peak pass.
// It stages z with a halo of 2 W (+ 12 with the flag) either side into LDS, +0 for every index outside the stream -- nothing outside
// the request's own run of y is read, nothing at or past 600 * frames[b] of a row -- scales it, keeps the 16 raw z1 of every lane in
// registers and zeroes what is not finite.  With the flag the shared 24-tap chains give e[n] = max over phi of |u_phi[n]| for the
// span and one more sample in front.  c goes into the second buffer; a workgroup none of whose c is below 1 stores z1 clamped and
// leaves.  The sliding minimum is log2 doubling passes that ping-pong between the two buffers (the staged samples are dead by then)
// and one last pass that joins two power-of-two windows.  The FIR: wave v owns samples [1024 v, 1024 v + 1024) in two rounds of
// 512, lane t the samples t + 64 k: eight float64 chains in registers, the weight read a broadcast, the eight m consecutive dwords
// across the lanes.  A round whose whole span of m is 1.0f skips the sum (the per-sample exception, taken by the whole wave: the sum
// itself rounds to 1.0f and leaves z1 as it is, so which samples take it does not show).  z2 goes to lim + the request's offset,
// and ONE dword per workgroup, the smallest f32(s) in the order of positive floats, into the partials table [R][windows].
constexpr int LIM_THREADS = 256;
constexpr int LIM_MAX_W = (LIMIT_MAX_TAPS - 1) / 2;                           // 240, at 48 000 Hz
constexpr int LIM_CS = (int)LEVEL_WINDOW + 4 * LIM_MAX_W + 8;                 // c over the window and 2 W either side (+ 1 for e)
constexpr int LIM_XS = 3 * TP_THREADS * TP_GROUP + TRUEPEAK_NTAPS;            // the chains' groups of 2048 may run past the staged span
constexpr int LIM_PER_LANE = (LIM_CS + LIM_THREADS - 1) / LIM_THREADS;        // 20 entries of the span a lane
constexpr int LIM_OWN = (int)LEVEL_WINDOW / LIM_THREADS;                      // 16 samples a lane
static_assert(LIM_XS >= LIM_CS + 2 * TRUEPEAK_NTAPS && (int)LEVEL_WINDOW + 4 * LIM_MAX_W + 1 <= 3 * TP_THREADS * TP_GROUP && LIM_THREADS == TP_THREADS &&
                  LEVEL_WINDOW == 4 * 1024 && LIM_OWN == 2 * 8 && KX_LIMIT_MAX_NTAPS == LIMIT_MAX_TAPS,
              "the staged span fits both buffers; four waves of two rounds of 512");
__device__ const uint32_t limit_tap_bits[4][LIMIT_MAX_TAPS] = {{KX_LIMIT_TAPS_24000}, {KX_LIMIT_TAPS_8000}, {KX_LIMIT_TAPS_16000}, {KX_LIMIT_TAPS_48000}};

__global__ __launch_bounds__(LIM_THREADS) void request_limit_kernel(const float* __restrict__ audio, long audio_ld,
                                                                     const PackReq* __restrict__ reqs, const long* __restrict__ cum,
                                                                     const JoinRow* __restrict__ jrows, const float* __restrict__ y,
                                                                     const LimitRow* __restrict__ lrows, const double* __restrict__ levels,
                                                                     float* __restrict__ lim, uint32_t* __restrict__ lpartials,
                                                                     long windows) {
    __shared__ float xs[LIM_XS];
    __shared__ float cs[LIM_CS];
    __shared__ double hs[LIMIT_MAX_TAPS];
    __shared__ double ts[TRUEPEAK_PHASES * TRUEPEAK_NTAPS];
    __shared__ uint32_t wave_min[LIM_THREADS / 64];
    const LimitRow lr = lrows[blockIdx.y];
    if (lr.off < 0) return;  // (uniform) a request beside the limited ones
    const PackReq rq = reqs[blockIdx.y];
    const long N = rq.n_samples;
    const long n0 = (long)blockIdx.x * LEVEL_WINDOW;
    if (n0 >= N) return;  // (uniform: the grid covers the longest request)
    const long n1 = n0 + LEVEL_WINDOW < N ? n0 + LEVEL_WINDOW : N;
    const int cnt = (int)(n1 - n0);
    const bool flagged = (lr.mode & PEAK_TRUE) != 0;  // (uniform)
    const int W = limit_window(rq.rate), L = 2 * W + 1, XO = flagged ? TRUEPEAK_NTAPS / 2 : 0;
    const float peak = lr.peak;
    const double g = levels[2 * blockIdx.y + 1];
    // the staged span: local index i of xs is sample n0 - 2 W - XO + i of the stream, i < T0; [s_lo, s_hi) of them are inside it
    const int Ta = cnt + 4 * W, T0 = Ta + 2 * XO;
    const long w_lo = n0 - 2 * W - XO;
    const long s_lo = w_lo < 0 ? 0 : w_lo, s_hi = w_lo + T0 < N ? w_lo + T0 : N;
    const int front = (int)(s_lo - w_lo), back = (int)(s_hi - w_lo);
    for (int i = threadIdx.x; i < front; i += LIM_THREADS) xs[i] = 0.0f;
    for (int i = back + threadIdx.x; i < T0; i += LIM_THREADS) xs[i] = 0.0f;
    float* __restrict__ dst = xs + front;
    if (rq.rate) {  // (uniform) one contiguous run
        const float* __restrict__ src = y + rq.y_off;
        for (long i = s_lo + threadIdx.x; i < s_hi; i += LIM_THREADS) dst[i - s_lo] = (float)(g * (double)src[i]);
    } else {  // the rows, cut and faded as the packer would see them; every lane scales the samples it staged itself
        if (jrows) stage_stream<true, LIM_THREADS>(dst, audio, audio_ld, cum, jrows, rq.first_row, rq.n_rows, s_lo, s_hi);
        else stage_stream<false, LIM_THREADS>(dst, audio, audio_ld, cum, jrows, rq.first_row, rq.n_rows, s_lo, s_hi);
        for (long i = s_lo + threadIdx.x; i < s_hi; i += LIM_THREADS) dst[i - s_lo] = (float)(g * (double)dst[i - s_lo]);
    }
    for (int i = threadIdx.x; i < L; i += LIM_THREADS) hs[i] = (double)__uint_as_float(limit_tap_bits[rq.rate][i]);
    if (threadIdx.x < TRUEPEAK_PHASES * TRUEPEAK_NTAPS) ts[threadIdx.x] = (double)__uint_as_float(truepeak_tap_bits[threadIdx.x]);
    __syncthreads();
    // the lane's own samples, raw (a NaN or an inf of z1 is needed again at the end): sample q = 1024 wave + 512 round + lane + 64 k
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float own[LIM_OWN];
#pragma unroll
    for (int e = 0; e < LIM_OWN; ++e) {
        const int q = 1024 * wave + 512 * (e >> 3) + lane + 64 * (e & 7);
        own[e] = q < cnt ? xs[2 * W + XO + q] : 0.0f;
    }
    __syncthreads();
    auto finite = [](float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; };
    for (int i = front + threadIdx.x; i < back; i += LIM_THREADS)
        if (!finite(xs[i])) xs[i] = 0.0f;
    __syncthreads();
    // c[k], k < Ta, of sample n0 - 2 W + k: its x is xs[k + XO]
    float cv[LIM_PER_LANE];
    if (flagged) {
        // e[q] of sample n0 - 2 W - 1 + q, q <= Ta, into cs: u of that sample reads xs[q + 0 .. 23]
        for (int base = 0; base < Ta + 1; base += TP_THREADS * TP_GROUP) {
            if (base + (int)(threadIdx.x & ~63u) >= Ta + 1) break;
            double acc[TRUEPEAK_PHASES][TP_GROUP];
            truepeak_chains(xs + base + threadIdx.x, ts, acc);
#pragma unroll
            for (int k = 0; k < TP_GROUP; ++k) {
                const int q = base + (int)threadIdx.x + TP_THREADS * k;
                if (q < Ta + 1) {
                    const long n = n0 - 2 * W - 1 + q;
                    float e = fmaxf(fmaxf(fabsf((float)acc[0][k]), fabsf((float)acc[1][k])), fabsf((float)acc[2][k]));
                    if (n < 0 || n >= N) e = 0.0f;  // (u is defined inside the stream; u[-1] = 0)
                    cs[q] = e;
                }
            }
        }
        __syncthreads();
    }
    int below = 0;
#pragma unroll
    for (int e = 0; e < LIM_PER_LANE; ++e) {
        const int k = (int)threadIdx.x + LIM_THREADS * e;
        float c = 1.0f;
        if (k < Ta) {
            const long n = n0 - 2 * W + k;
            float a = fabsf(xs[k + XO]);
            if (flagged) a = fmaxf(fmaxf(a, cs[k]), cs[k + 1]);
            if (n >= 0 && n < N && !(a <= peak)) c = (float)((double)peak / (double)a);
        }
        cv[e] = c;
        below |= c < 1.0f;
    }
    const int any_below = __syncthreads_or(below);  // (and every lane has read the e it needs)
    float* __restrict__ out = lim + lr.off + n0;
    uint32_t rmin = 0x3F800000u;
    if (any_below) {  // (uniform)
#pragma unroll
        for (int e = 0; e < LIM_PER_LANE; ++e) {
            const int k = (int)threadIdx.x + LIM_THREADS * e;
            if (k < Ta) cs[k] = cv[e];
        }
        __syncthreads();
        // the sliding minimum over L = 2 W + 1: M_d[i] = min c[i .. i + d), d doubling up to the largest power of two p <= L, between the
        // two buffers; then m[i] = min(M_p[i], M_p[i + L - p]), i < Tm.  An entry whose window would pass Ta is never needed.
        float* src = cs;
        float* alt = xs;
        int d = 1;
        for (; 2 * d <= L; d *= 2) {
            for (int i = threadIdx.x; i < Ta; i += LIM_THREADS) alt[i] = i + d < Ta ? fminf(src[i], src[i + d]) : src[i];
            __syncthreads();
            float* t = src;
            src = alt, alt = t;
        }
        const int Tm = cnt + 2 * W;  // m[i] of sample n0 - W + i
        for (int i = threadIdx.x; i < Tm; i += LIM_THREADS) alt[i] = fminf(src[i], src[i + L - d]);
        __syncthreads();
        const float* ms = alt;
        // the FIR: s of sample q reads ms[q + 0 .. 2 W]
#pragma unroll
        for (int round = 0; round < 2; ++round) {
            const int qb = 1024 * wave + 512 * round;
            if (qb >= cnt) break;  // (the wave)
            const int q_end = (qb + 512 < cnt ? qb + 512 : cnt) + 2 * W;
            int ones = 1;
            for (int j = qb + lane; j < q_end; j += 64) ones &= ms[j] == 1.0f;
            double acc[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] = 1.0;
            if (!__all(ones)) {  // (the wave)
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[k] = 0.0;
                const float* mp = ms + qb + lane;
#pragma unroll 4
                for (int i = 0; i < L; ++i) {
                    const double h = hs[i];
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc[k] += h * (double)mp[64 * k + i];
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int q = qb + lane + 64 * k;
                if (q < cnt) {
                    const uint32_t sb = __float_as_uint((float)acc[k]);
                    rmin = sb < rmin ? sb : rmin;
                    float z2 = (float)(acc[k] * (double)own[8 * round + k]);
                    if (fabsf(z2) > peak) z2 = copysignf(peak, z2);
                    out[q] = z2;
                }
            }
        }
    } else {  // nothing of the span is above the peak: s = 1 throughout
#pragma unroll
        for (int e = 0; e < LIM_OWN; ++e) {
            const int q = 1024 * wave + 512 * (e >> 3) + lane + 64 * (e & 7);
            if (q < cnt) {
                float z2 = own[e];
                if (fabsf(z2) > peak) z2 = copysignf(peak, z2);
                out[q] = z2;
            }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t v = (uint32_t)__shfl_xor((int)rmin, o);
        rmin = v < rmin ? v : rmin;
    }
    if (lane == 0) wave_min[wave] = rmin;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < LIM_THREADS / 64; ++w) rmin = wave_min[w] < rmin ? wave_min[w] : rmin;
        lpartials[(long)blockIdx.y * windows + blockIdx.x] = rmin;
    }
}
// request_limit_report_kernel: one wave per limited request reduces its partials (the windows past its end were never written and
// are not read) and stores {f64(p), g, I, n_g, r} into the limits block: p and g from the levels block, I and n_g from the loudness
// block in mode 1 and a quiet NaN and 0 in mode 0, r = f64(min f32(s)), 1.0 for a request nothing limited.
__global__ __launch_bounds__(64) void request_limit_report_kernel(const PackReq* __restrict__ reqs, const LimitRow* __restrict__ lrows,
                                                                  const uint32_t* __restrict__ lpartials, long windows,
                                                                  const double* __restrict__ levels, const double* __restrict__ loud,
                                                                  double* __restrict__ limits) {
    const int r = blockIdx.x;
    const LimitRow lr = lrows[r];
    if (lr.off < 0) return;  // (the whole wave)
    const long n = (reqs[r].n_samples + LEVEL_WINDOW - 1) / LEVEL_WINDOW;
    uint32_t m = 0x3F800000u;
    for (long w = threadIdx.x; w < n; w += 64) {
        const uint32_t v = lpartials[(long)r * windows + w];
        m = v < m ? v : m;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t v = (uint32_t)__shfl_xor((int)m, o);
        m = v < m ? v : m;
    }
    if (threadIdx.x != 0) return;
    const bool metered = (lr.mode & ~PEAK_TRUE) == LIMIT_LOUDNESS;
    limits[5 * r] = levels[2 * r];
    limits[5 * r + 1] = levels[2 * r + 1];
    limits[5 * r + 2] = metered ? loud[2 * r] : __longlong_as_double(0x7FF8000000000000LL);
    limits[5 * r + 3] = metered ? loud[2 * r + 1] : 0.0;
    limits[5 * r + 4] = (double)__uint_as_float(m);
}

// ---- FLAC: lossless 16-bit frames, one workgroup a frame (include/kokorox_hip.h, "FLAC"; host_request.h: FlacRow) ---------------
// The samples are form 4's 16-bit v of the stream the packer of this plan would stage: the limit buffer's run of a limited request,
// the resampled run or the rows (joined where the plan is), times g where the plan is levelled, then pcm16_sample with NaN -> 0.
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
    // the samples, as the packer of this plan stages them; every lane converts what it staged itself (sample i: lane (i - n0) mod 256)
    float* __restrict__ smp = reinterpret_cast<float*>(vs);
    const long lim_off = lrows ? lrows[blockIdx.y].off : -1;
    bool scaled = false;
    if (lim_off >= 0) {  // (uniform) a limited request: scaled and limited already
        const float* __restrict__ src = lim + lim_off;
        for (long i = n0 + tid; i < n1; i += FLAC_THREADS) smp[i - n0] = src[i];
    } else if (rq.rate) {  // (uniform) a resampled request: one contiguous run
        const float* __restrict__ src = y + rq.y_off;
        for (long i = n0 + tid; i < n1; i += FLAC_THREADS) smp[i - n0] = src[i];
        scaled = levels != nullptr;
    } else {
        if (jrows) stage_stream<true, FLAC_THREADS>(smp, audio, audio_ld, cum, jrows, rq.first_row, rq.n_rows, n0, n1);
        else stage_stream<false, FLAC_THREADS>(smp, audio, audio_ld, cum, jrows, rq.first_row, rq.n_rows, n0, n1);
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

// ---- IMA ADPCM in a WAV file: one lane a block (include/kokorox_hip.h, "IMA ADPCM"; host_request.h: FORM_ADPCM_WAV) --------------
// The samples are form 4's 16-bit v of the stream the packer of this plan would stage, exactly as the FLAC encoder takes them.  A
// body is 60 header bytes and F blocks of A bytes, so every block's place follows from the plan: no layout pass, no gather.
//
// adpcm_blocks_kernel: workgroup (k, r) encodes blocks G k .. G k + G - 1 of request r, G = 8192 / A of them (32, 16, 8), whose
// samples are ONE run of at most G P of the stream.  All 256 lanes stage that run along time, a tile of 4096 floats at a time through
// the packers' staging functions, and every lane converts the samples it staged itself and stores them as 16-bit values into the LDS
// row of their block; the samples behind N repeat v[N - 1].  Then lane g < G runs the recurrence of block g out of its row and keeps
// eight codes in a register per dword it stores into the code rows (the float tile, dead by then); at last all lanes move the group's
// 8192 bytes (and the header, in group 0) to global memory as aligned 16-byte units, single dwords at a region's ragged ends as in
// the packer.  No lane walks global memory with a block-sized stride.
// LDS strides: a row is P samples = P / 2 dwords, no whole number (252.5, 508.5, 1020.5), so lanes g and g + 2 would sit 505 dwords
// = 57 banks apart and the 32 lanes of the 8 kHz form fold onto the 64 banks twice.  The rows are therefore padded to (P + 1) / 2 =
// 253, 509, 1021 dwords, all odd: lane g reads dword g S + t / 2, and g S mod 64 takes every value once -- no two of up to 64
// lanes on one bank.  The code rows are A / 4 + 1 = 65, 129, 257 dwords for the same reason (A / 4 alone is a multiple of 64: every
// lane on bank 0).  The step table is in LDS too: the lookup step = STEP[index] is on the recurrence's critical path.
constexpr int ADPCM_THREADS = 256;
constexpr int ADPCM_TILE = 4096;                                   // floats staged at a time; the code rows afterwards
constexpr int ADPCM_ROW_WORDS = 8 * ((2 * 1024 - 7 + 1) / 2);      // G S at its largest: 8 x 1021 dwords (32 x 253 = 8096, 16 x 509 = 8144)
static_assert(ADPCM_GROUP_BYTES / 256 * (256 / 4 + 1) <= ADPCM_TILE && 32 * 253 <= ADPCM_ROW_WORDS && 16 * 509 <= ADPCM_ROW_WORDS &&
                  ADPCM_GROUP_BYTES / 256 <= 64 && ADPCM_HEADER == 60,
              "the code rows fit the tile, the sample rows their buffer, one wave holds a group's lanes");
__device__ const int adpcm_step_table[KX_ADPCM_NSTEPS] = {KX_ADPCM_STEPS};

__device__ __forceinline__ uint32_t adpcm_header_dword(int j, long N, long F, int A, int P, int rate_code) {
    const uint32_t hz = rate_code == 0 ? 24000u : (rate_code == 1 ? 8000u : (rate_code == 2 ? 16000u : 48000u));
    switch (j) {
        case 0: return 0x46464952u;                        // "RIFF"
        case 1: return (uint32_t)(52 + (long)A * F);       // file size - 8
        case 2: return 0x45564157u;                        // "WAVE"
        case 3: return 0x20746d66u;                        // "fmt "
        case 4: return 20u;
        case 5: return 0x0011u | (1u << 16);               // WAVE_FORMAT_IMA_ADPCM, 1 channel
        case 6: return hz;
        case 7: return hz * (uint32_t)A / (uint32_t)P;     // bytes per second
        case 8: return (uint32_t)A | (4u << 16);           // block align, bits per sample
        case 9: return 2u | ((uint32_t)P << 16);           // cbSize, wSamplesPerBlock
        case 10: return 0x74636166u;                       // "fact"
        case 11: return 4u;
        case 12: return (uint32_t)N;
        case 13: return 0x61746164u;                       // "data"
        default: return (uint32_t)((long)A * F);
    }
}

template <int A>
__device__ __forceinline__ void adpcm_group(const float* __restrict__ audio, long audio_ld, const PackReq& rq, int r,
                                            const long* __restrict__ cum, const JoinRow* __restrict__ jrows,
                                            const float* __restrict__ y, const double* __restrict__ levels,
                                            const LimitRow* __restrict__ lrows, const float* __restrict__ lim, char* __restrict__ out,
                                            float* ftile, uint32_t* rows, const int* steps) {
    constexpr int P = 1 + 2 * (A - 4), G = (int)ADPCM_GROUP_BYTES / A, S = (P + 1) / 2, CW = A / 4 + 1;
    static_assert(S % 2 == 1 && CW % 2 == 1 && G * S <= ADPCM_ROW_WORDS && G * CW <= ADPCM_TILE, "odd strides, rows inside their buffers");
    const int tid = threadIdx.x;
    const long N = rq.n_samples, F = (N + P - 1) / P;
    const long b0 = (long)blockIdx.x * G;
    if (b0 >= F && blockIdx.x > 0) return;  // (uniform: the grid covers the request with most blocks; group 0 has the header)
    const int nb = (int)(F - b0 < G ? F - b0 : G);  // blocks of this group; 0 in the only group of an empty request
    const long n0 = b0 * P, n1 = n0 + (long)nb * P < N ? n0 + (long)nb * P : N;
    short* rows16 = reinterpret_cast<short*>(rows);
    // the samples, as the packer of this plan stages them; every lane converts what it staged itself (sample i: lane (i - t0) mod 256)
    const long lim_off = lrows ? lrows[r].off : -1;
    const bool scaled = lim_off < 0 && levels != nullptr;
    const double g = scaled ? levels[2 * r + 1] : 1.0;
    for (long t0 = n0; t0 < n1; t0 += ADPCM_TILE) {
        const long t1 = t0 + ADPCM_TILE < n1 ? t0 + ADPCM_TILE : n1;
        if (lim_off >= 0) {  // (uniform) a limited request: scaled and limited already
            const float* __restrict__ src = lim + lim_off;
            for (long i = t0 + tid; i < t1; i += ADPCM_THREADS) ftile[i - t0] = src[i];
        } else if (rq.rate) {  // (uniform) a resampled request: one contiguous run
            const float* __restrict__ src = y + rq.y_off;
            for (long i = t0 + tid; i < t1; i += ADPCM_THREADS) ftile[i - t0] = src[i];
        } else if (jrows) {
            stage_stream<true, ADPCM_THREADS>(ftile, audio, audio_ld, cum, jrows, rq.first_row, rq.n_rows, t0, t1);
        } else {
            stage_stream<false, ADPCM_THREADS>(ftile, audio, audio_ld, cum, jrows, rq.first_row, rq.n_rows, t0, t1);
        }
        for (long i = t0 + tid; i < t1; i += ADPCM_THREADS) {
            float x = ftile[i - t0];
            if (scaled) x = (float)(g * (double)x);
            const int rel = (int)(i - n0), blk = rel / P;
            rows16[blk * (2 * S) + (rel - blk * P)] = (short)pcm16_sample(x, true);
        }
    }
    __syncthreads();
    const int have = (int)(n1 - n0);  // samples of the group that exist; the rest of its last block repeats v[N - 1]
    if (have < nb * P) {
        const int at = have - 1, ab = at / P;
        const short last = rows16[ab * (2 * S) + (at - ab * P)];
        for (int rel = have + tid; rel < nb * P; rel += ADPCM_THREADS) {
            const int blk = rel / P;
            rows16[blk * (2 * S) + (rel - blk * P)] = last;
        }
        __syncthreads();
    }
    uint32_t* codes = reinterpret_cast<uint32_t*>(ftile);  // (every lane's staged floats are converted: the tile is free)
    if (tid < nb) {
        const short* row = rows16 + tid * (2 * S);
        int pred = row[0];
        int d0 = 0;  // the largest of the block's first differences (a block holds at least 505 samples)
#pragma unroll
        for (int j = 0; j < KX_ADPCM_START_DIFFS; ++j) {
            const int d = abs((int)row[j + 1] - (int)row[j]);
            d0 = d > d0 ? d : d0;
        }
        int lo = 0, hi = KX_ADPCM_NSTEPS - 1;  // the smallest index whose step reaches d0; 88 when none does
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (steps[mid] >= d0) hi = mid; else lo = mid + 1;
        }
        int index = lo, step = steps[lo];
        uint32_t* crow = codes + tid * CW;
        crow[0] = ((uint32_t)pred & 0xFFFFu) | ((uint32_t)index << 16);
        for (int w = 0; w < (A - 4) / 4; ++w) {
            uint32_t acc = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                int d = (int)row[1 + 8 * w + j] - pred;
                uint32_t code = d < 0 ? 8u : 0u;
                d = d < 0 ? -d : d;
                int vp = step >> 3, h = step;
                if (d >= h) code |= 4u, d -= h, vp += h;
                h = step >> 1;
                if (d >= h) code |= 2u, d -= h, vp += h;
                h = step >> 2;
                if (d >= h) code |= 1u, vp += h;
                pred = (code & 8u) ? pred - vp : pred + vp;
                pred = pred < -32768 ? -32768 : (pred > 32767 ? 32767 : pred);
                index += (code & 4u) ? 2 * (int)(code & 3u) + 2 : -1;  // -1, -1, -1, -1, 2, 4, 6, 8 by the low three bits
                index = index < 0 ? 0 : (index > KX_ADPCM_NSTEPS - 1 ? KX_ADPCM_NSTEPS - 1 : index);
                step = steps[index];
                acc |= code << (4 * j);
            }
            crow[1 + w] = acc;
        }
    }
    __syncthreads();
    // bytes [lo_b, hi_b) of the region: the group's blocks, and the header in front of block 0; one aligned 16-byte unit a lane
    const long lo_b = blockIdx.x == 0 ? 0 : ADPCM_HEADER + (long)A * b0, hi_b = ADPCM_HEADER + (long)A * (b0 + nb);
    for (long a = ((rq.out_off + lo_b) & ~15L) + 16L * tid; a < rq.out_off + hi_b; a += 16L * ADPCM_THREADS) {
        uint32_t w[4];
        bool in[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long p = a + 4 * j - rq.out_off;
            in[j] = p >= lo_b && p < hi_b;
            w[j] = 0;
            if (in[j]) {
                if (p < ADPCM_HEADER) {
                    w[j] = adpcm_header_dword((int)(p >> 2), N, F, A, P, rq.rate);
                } else {
                    const int q = (int)(((p - ADPCM_HEADER) >> 2) - b0 * (A / 4));
                    w[j] = codes[(q / (A / 4)) * CW + (q % (A / 4))];
                }
            }
        }
        char* o = out + a;  // 16-byte aligned
        if (in[0] && in[1] && in[2] && in[3]) {
            *reinterpret_cast<uint4*>(o) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (in[j]) *reinterpret_cast<uint32_t*>(o + 4 * j) = w[j];
        }
    }
}

__global__ __launch_bounds__(ADPCM_THREADS) void adpcm_blocks_kernel(const float* __restrict__ audio, long audio_ld,
                                                                     const PackReq* __restrict__ reqs, const long* __restrict__ cum,
                                                                     const JoinRow* __restrict__ jrows, const float* __restrict__ y,
                                                                     const double* __restrict__ levels,
                                                                     const LimitRow* __restrict__ lrows, const float* __restrict__ lim,
                                                                     char* __restrict__ out) {
    __shared__ float ftile[ADPCM_TILE];
    __shared__ uint32_t rows[ADPCM_ROW_WORDS];
    __shared__ int steps[KX_ADPCM_NSTEPS];
    const PackReq rq = reqs[blockIdx.y];
    if (rq.form != FORM_ADPCM_WAV) return;  // (uniform: another form)
    if (threadIdx.x < KX_ADPCM_NSTEPS) steps[threadIdx.x] = adpcm_step_table[threadIdx.x];  // (read behind the first barrier)
    if (rq.rate == 1)
        adpcm_group<256>(audio, audio_ld, rq, (int)blockIdx.y, cum, jrows, y, levels, lrows, lim, out, ftile, rows, steps);
    else if (rq.rate == 3)
        adpcm_group<1024>(audio, audio_ld, rq, (int)blockIdx.y, cum, jrows, y, levels, lrows, lim, out, ftile, rows, steps);
    else
        adpcm_group<512>(audio, audio_ld, rq, (int)blockIdx.y, cum, jrows, y, levels, lrows, lim, out, ftile, rows, steps);
}

// The bodies of a plan: its request table, prefixes and (a joined or levelled plan) join rows copied into `t`, the resampler when
// some request carries a rate code, then the packer.  d_y: plan.y_floats floats (may be null when that is 0); out: 16-byte aligned,
// plan.total_bytes long.  The joined form of the two kernels runs only when the plan says so (OutputPlan::joined).  A measured
// plan (OutputPlan::measured): between the resampler and the packer the peak pass and the gain kernel, which stores every
// request's {p, g} at out + plan.levels_off; the levelled packer runs only when some spec is not the plain one.  A plan with
// loudness (OutputPlan::loud): the meter behind the peak pass, its gain kernel behind request_gain_kernel, {I, n_g} of every
// metered request at out + plan.loud_off; a plan without loudness launches neither.  A plan with a true peak (OutputPlan::true_peak):
// request_truepeak_kernel behind the resampler and before the gain kernels; a plan without the flag does not launch it.  A plan with
// a limited request (OutputPlan::limited): request_limit_kernel and its report behind the gain kernels, the limited streams into
// t.lim, {f64(p), g, I, n_g, r} at out + plan.limits_off, and the limited packer; a plan without one launches none of the three.  A
// plan with a FLAC request (OutputPlan::has_flac): flac_frames_kernel, flac_layout_kernel and flac_gather_kernel behind the limiter,
// every region's true size at out + plan.flac_off; a plan without one launches none of them and copies plan.req as it always did.
// A plan with an ADPCM request (OutputPlan::adpcm_groups > 0): adpcm_blocks_kernel at the same place, which needs no table of its own.
void launch_pack_plan(const float* audio, long audio_ld, const OutputPlan& plan, const OutputTables& t, float* d_y, void* out,
                      hipStream_t s) {
    if (plan.max_units <= 0 && !plan.measured && !plan.has_flac() && plan.adpcm_groups <= 0 && !plan.has_pieces()) return;
    const size_t R = plan.req.size(), B = plan.join.size();
    KX_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0 && R <= 65535, "pack: unaligned output or too many requests");
    // (a plan with FLAC: the packer's table has those requests emptied; every other kernel reads the fields the two tables share)
    KX_HIP(hipMemcpyAsync(t.req, plan.has_flac() ? plan.pack_req.data() : plan.req.data(), R * sizeof(PackReq), hipMemcpyHostToDevice, s));
    if (plan.has_flac()) {
        KX_REQUIRE(t.frow && t.finfo && plan.flac.size() == R && plan.pack_req.size() == R && (plan.flac_off & 7) == 0 &&
                       plan.flac_off >= plan.blocks_end() && plan.flac_max_frames <= 0x7FFFFFFF &&
                       (plan.flac_slots == 0 || (t.fslot && t.flen && t.foff && (reinterpret_cast<uintptr_t>(t.fslot) & 15) == 0)),
                   "flac: bad launch argument");
        KX_HIP(hipMemcpyAsync(t.frow, plan.flac.data(), R * sizeof(FlacRow), hipMemcpyHostToDevice, s));
    }
    KX_HIP(hipMemcpyAsync(t.cum, plan.cum.data(), (B + 1) * sizeof(long), hipMemcpyHostToDevice, s));
    if (plan.joined || plan.levelled || plan.has_pieces())
        KX_HIP(hipMemcpyAsync(t.join, plan.join.data(), B * sizeof(JoinRow), hipMemcpyHostToDevice, s));
    if (plan.has_pieces()) {  // (the table of the two piece kernels and the carried tails; both always stage through the join table)
        KX_REQUIRE(t.piece && t.join && (t.piece_tail || plan.tail_in.empty()) && plan.piece.size() == R && (plan.carry_off & 7) == 0 &&
                       plan.carry_off >= plan.report_end() && plan.tail_in.size() <= R * (size_t)PIECE_TAIL,
                   "pieces: bad launch argument");
        KX_HIP(hipMemcpyAsync(t.piece, plan.piece.data(), R * sizeof(PieceRow), hipMemcpyHostToDevice, s));
        if (!plan.tail_in.empty())
            KX_HIP(hipMemcpyAsync(t.piece_tail, plan.tail_in.data(), plan.tail_in.size() * sizeof(float), hipMemcpyHostToDevice, s));
    }
    if (plan.measured) {
        KX_REQUIRE(t.level && t.peak && plan.level.size() == R && (plan.levels_off & 7) == 0, "levels: bad launch argument");
        KX_HIP(hipMemcpyAsync(t.level, plan.level.data(), R * sizeof(LevelSpec), hipMemcpyHostToDevice, s));
    }
    const bool loud = !plan.loud.empty();
    if (loud) {
        KX_REQUIRE(t.loud && t.loud_pow && (t.hops || plan.max_hops == 0) && plan.loud.size() == R && plan.loud_off == plan.levels_off + 16 * (long)R,
                   "loudness: bad launch argument");
        KX_HIP(hipMemcpyAsync(t.loud, plan.loud.data(), R * sizeof(LoudSpec), hipMemcpyHostToDevice, s));
        KX_HIP(hipMemcpyAsync(t.loud_pow, loud_powers(), (size_t)4 * LOUD_POWERS * 16 * sizeof(double), hipMemcpyHostToDevice, s));
    }
    if (plan.limited) {
        KX_REQUIRE(t.limit && t.lpart && (t.lim || plan.lim_floats == 0) && loud && plan.limit.size() == R &&
                       plan.limits_off == plan.loud_off + 16 * (long)R,
                   "limiter: bad launch argument");
        KX_HIP(hipMemcpyAsync(t.limit, plan.limit.data(), R * sizeof(LimitRow), hipMemcpyHostToDevice, s));
    }
    if (plan.y_floats > 0) {
        KX_REQUIRE(d_y != nullptr, "pack: no buffer for the resampled streams");
        const dim3 grid((unsigned)((plan.max_resampled + RS_WINDOW - 1) / RS_WINDOW), (unsigned)R);
        if (plan.has_pieces() && plan.joined)  // (every request of the plan, the ones run whole included: the same bits)
            hipLaunchKernelGGL(resample_pieces_joined_kernel, grid, dim3(RS_THREADS), 0, s, audio, audio_ld, t.req, t.piece, t.cum, t.join,
                               t.piece_tail, d_y);
        else if (plan.has_pieces())
            hipLaunchKernelGGL(resample_pieces_kernel, grid, dim3(RS_THREADS), 0, s, audio, audio_ld, t.req, t.piece, t.cum, t.piece_tail,
                               d_y);
        else if (plan.joined)
            hipLaunchKernelGGL(resample_requests_joined_kernel, grid, dim3(RS_THREADS), 0, s, audio, audio_ld, t.req, t.cum, t.join, d_y);
        else
            hipLaunchKernelGGL(resample_requests_kernel, grid, dim3(RS_THREADS), 0, s, audio, audio_ld, t.req, t.cum, d_y);
        KX_HIP(hipGetLastError());
    }
    // the carries of a plan with pieces, into their block behind everything else: they depend on the rows and the old tails alone
    if (plan.has_pieces()) {
        hipLaunchKernelGGL(piece_carry_kernel, dim3((unsigned)R), dim3(PIECE_TAIL), 0, s, audio, audio_ld, t.req, t.piece, t.cum, t.join,
                           t.piece_tail, static_cast<char*>(out));
        KX_HIP(hipGetLastError());
    }
    double* levels = plan.measured ? reinterpret_cast<double*>(static_cast<char*>(out) + plan.levels_off) : nullptr;
    const uint32_t* tpeak = plan.true_peak ? t.tpeak : nullptr;  // (read for a flagged request only)
    if (plan.measured) {
        if (plan.peak_windows > 0) {
            hipLaunchKernelGGL(request_peak_kernel, dim3((unsigned)plan.peak_windows, (unsigned)R), dim3(PEAK_THREADS), 0, s, audio, audio_ld,
                               t.req, t.cum, plan.joined ? t.join : nullptr, d_y, t.peak, plan.peak_windows);
            KX_HIP(hipGetLastError());
        }
        if (loud && plan.max_hops > 0) {
            hipLaunchKernelGGL(request_loudness_kernel, dim3((unsigned)plan.max_hops, (unsigned)R), dim3(LOUD_THREADS), 0, s, audio, audio_ld,
                               t.req, t.cum, plan.joined ? t.join : nullptr, d_y, t.loud, t.loud_pow, t.hops, plan.max_hops);
            KX_HIP(hipGetLastError());
        }
        // the true peak of the flagged requests into the second table, [R][peak_windows] as the first: the gain kernels join the two
        if (plan.true_peak && plan.peak_windows > 0) {
            KX_REQUIRE(t.tpeak != nullptr, "levels: no table for the true peak");
            hipLaunchKernelGGL(request_truepeak_kernel, dim3((unsigned)plan.peak_windows, (unsigned)R), dim3(TP_THREADS), 0, s, audio,
                               audio_ld, t.req, t.cum, plan.joined ? t.join : nullptr, d_y, t.level, loud ? t.loud : nullptr, t.tpeak,
                               plan.peak_windows);
            KX_HIP(hipGetLastError());
        }
        // (a metered request's {p, g} slot is the loudness gain kernel's: request_gain_kernel, which runs only when some request is
        // not metered, leaves the plain spec's {p, 1} there and the later kernel of the same stream stores the request's own)
        if (!plan.loud_all) {
            hipLaunchKernelGGL(request_gain_kernel, dim3((unsigned)R), dim3(64), 0, s, t.req, t.level, t.peak, tpeak, plan.peak_windows, levels);
            KX_HIP(hipGetLastError());
        }
        if (loud) {
            hipLaunchKernelGGL(request_loudness_gain_kernel, dim3((unsigned)R), dim3(64), 0, s, t.req, t.loud, t.peak, tpeak, plan.peak_windows,
                               t.hops, plan.max_hops, levels, reinterpret_cast<double*>(static_cast<char*>(out) + plan.loud_off));
            KX_HIP(hipGetLastError());
        }
        // the limiter, behind the gains it is driven by: every limited request's z2 into the limit buffer, then its five values
        if (plan.limited) {
            if (plan.peak_windows > 0) {
                hipLaunchKernelGGL(request_limit_kernel, dim3((unsigned)plan.peak_windows, (unsigned)R), dim3(LIM_THREADS), 0, s, audio,
                                   audio_ld, t.req, t.cum, plan.joined ? t.join : nullptr, d_y, t.limit, levels, t.lim, t.lpart,
                                   plan.peak_windows);
                KX_HIP(hipGetLastError());
            }
            hipLaunchKernelGGL(request_limit_report_kernel, dim3((unsigned)R), dim3(64), 0, s, t.req, t.limit, t.lpart, plan.peak_windows,
                               levels, reinterpret_cast<double*>(static_cast<char*>(out) + plan.loud_off),
                               reinterpret_cast<double*>(static_cast<char*>(out) + plan.limits_off));
            KX_HIP(hipGetLastError());
        }
    }
    // FLAC: the frames into their slots, the layout of every body, then the frames to their places; the samples are those the packer
    // launched below would stage (the same join rows, gains and limit buffer)
    if (plan.has_flac()) {
        const bool gains = plan.limited || plan.levelled;
        if (plan.flac_max_frames > 0) {
            hipLaunchKernelGGL(flac_frames_kernel, dim3((unsigned)plan.flac_max_frames, (unsigned)R), dim3(FLAC_THREADS), 0, s, audio, audio_ld,
                               t.req, t.cum, plan.joined || gains ? t.join : nullptr, d_y, gains ? levels : nullptr,
                               plan.limited ? t.limit : nullptr, plan.limited ? t.lim : nullptr, t.frow, t.fslot, t.flen);
            KX_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(flac_layout_kernel, dim3((unsigned)R), dim3(64), 0, s, t.frow, t.flen, t.foff, t.finfo,
                           reinterpret_cast<long long*>(static_cast<char*>(out) + plan.flac_off));
        KX_HIP(hipGetLastError());
        hipLaunchKernelGGL(flac_gather_kernel, dim3((unsigned)((plan.flac_max_bytes / 4 + 255) / 256), (unsigned)R), dim3(256), 0, s, t.frow,
                           t.finfo, t.fslot, t.flen, t.foff, static_cast<char*>(out));
        KX_HIP(hipGetLastError());
    }
    // ADPCM: every block of every form-17 request straight to its place, from the samples the packer launched below would stage
    if (plan.adpcm_groups > 0) {
        const bool gains = plan.limited || plan.levelled;
        KX_REQUIRE(plan.adpcm_groups <= 0x7FFFFFFF, "adpcm: too many blocks");
        hipLaunchKernelGGL(adpcm_blocks_kernel, dim3((unsigned)plan.adpcm_groups, (unsigned)R), dim3(ADPCM_THREADS), 0, s, audio, audio_ld,
                           t.req, t.cum, plan.joined || gains ? t.join : nullptr, d_y, gains ? levels : nullptr,
                           plan.limited ? t.limit : nullptr, plan.limited ? t.lim : nullptr, static_cast<char*>(out));
        KX_HIP(hipGetLastError());
    }
    if (plan.max_units <= 0) return;  // (a measured plan of empty requests: its levels are written, there is no body)
    const dim3 grid((unsigned)((plan.max_units + PACK_THREADS - 1) / PACK_THREADS), (unsigned)R);
    if (plan.limited)
        hipLaunchKernelGGL(pack_requests_limited_kernel, grid, dim3(PACK_THREADS), 0, s, audio, audio_ld, t.req, t.cum, t.join, d_y,
                           static_cast<char*>(out), levels, t.limit, t.lim);
    else if (plan.levelled)
        hipLaunchKernelGGL(pack_requests_levelled_kernel, grid, dim3(PACK_THREADS), 0, s, audio, audio_ld, t.req, t.cum, t.join, d_y,
                           static_cast<char*>(out), levels);
    else if (plan.joined)
        hipLaunchKernelGGL(pack_requests_joined_kernel, grid, dim3(PACK_THREADS), 0, s, audio, audio_ld, t.req, t.cum, t.join, d_y,
                           static_cast<char*>(out));
    else
        hipLaunchKernelGGL(pack_requests_kernel, grid, dim3(PACK_THREADS), 0, s, audio, audio_ld, t.req, t.cum, d_y,
                           static_cast<char*>(out));
    KX_HIP(hipGetLastError());
}

// ---- token timing marks (include/kokorox_hip.h has the definition; host_request.h: MarkRow, build_output_plan) ----------------
// One workgroup of 512 per row: lane t holds the duration of token t (0 at and beyond lens[b]: the front half leaves those
// entries of `dur` unwritten, they are never loaded), an exclusive scan in 64 bits, and lane t stores base + K x scan[t] as one
// 8-byte value, coalesced along t; the lane of the last token stores entry T, the row's end, as well.  The scan is one
// __shfl_up ladder inside each wave64 and ONE exchange of the eight wave totals through LDS (one barrier).
// JOINED (a batch with a joined request): the value is (src_base + clamp(600 x scan - skip, 0, keep)) L / M, written as x K / 600
// -- every term is a multiple of 24 and K of 200, so the division is exact; a plain row (skip 0, keep 600 x its frames) gives
// base + K x scan as before.
constexpr int MARK_THREADS = 512;
template <bool JOINED>
__device__ __forceinline__ void token_marks_body(const int* __restrict__ dur, const int* __restrict__ lens,
                                                 const MarkRow* __restrict__ rows, long long* __restrict__ marks) {
    __shared__ long long wave_total[MARK_THREADS / 64];
    const int b = blockIdx.x, t = threadIdx.x;
    const MarkRow mr = rows[b];
    if (mr.first < 0) return;  // (the whole workgroup: its request wants no marks)
    const int T = min(lens[b], MARK_THREADS);
    const long long d = t < T ? (long long)dur[(long)b * 512 + t] : 0;
    const int lane = t & 63, wave = t >> 6;
    long long incl = d;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    long long before = 0;
#pragma unroll
    for (int w = 0; w < MARK_THREADS / 64; ++w) before += w < wave ? wave_total[w] : 0;
    incl += before;
    auto mark = [&](long long scan) -> long long {
        if (!JOINED) return mr.base + mr.K * scan;
        long long u = 600 * scan - mr.skip;
        u = u < 0 ? 0 : (u > mr.keep ? mr.keep : u);
        return (mr.src_base + u) * mr.K / 600;
    };
    if (t < T) {
        marks[mr.first + t] = mark(incl - d);
        if (t == T - 1) marks[mr.first + T] = mark(incl);
    }
}
__global__ __launch_bounds__(MARK_THREADS) void token_marks_kernel(const int* __restrict__ dur, const int* __restrict__ lens,
                                                                   const MarkRow* __restrict__ rows,
                                                                   long long* __restrict__ marks) {
    token_marks_body<false>(dur, lens, rows, marks);
}
__global__ __launch_bounds__(MARK_THREADS) void token_marks_joined_kernel(const int* __restrict__ dur, const int* __restrict__ lens,
                                                                          const MarkRow* __restrict__ rows,
                                                                          long long* __restrict__ marks) {
    token_marks_body<true>(dur, lens, rows, marks);
}
// The marks of a plan (n_marks > 0): its mark rows copied into `t`, then one launch.  dur [B][512], lens [B]: device; marks: the
// marks block (8-byte aligned), n_marks values long.  A joined plan: the rows' skip / keep / src_base matter.
void launch_token_marks(const int* dur, const int* lens, const OutputPlan& plan, const OutputTables& t, void* marks, hipStream_t s) {
    const size_t B = plan.mark.size();
    KX_REQUIRE(dur && lens && t.mark && marks && B >= 1 && (reinterpret_cast<uintptr_t>(marks) & 7) == 0, "marks: bad launch argument");
    KX_HIP(hipMemcpyAsync(t.mark, plan.mark.data(), B * sizeof(MarkRow), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(plan.joined ? token_marks_joined_kernel : token_marks_kernel, dim3((unsigned)B), dim3(MARK_THREADS), 0, s, dur,
                       lens, t.mark, static_cast<long long*>(marks));
    KX_HIP(hipGetLastError());
}

// The output stage of a call whose plan is built, for the model and for the test hook alike: the bodies into d_packed, and the
// marks of the requests that want them in their block behind the bodies (8-aligned), and behind those the levels of a measured
// plan (and behind those the loudness of a plan that has it), so one copy to the host brings them all (the limits of a plan
// with a limited request are the last block).  The order is resampler, peak, loudness, true peak, gain, limiter, packer, marks.
void launch_output_plan(const float* audio, long audio_ld, const int* dur, const int* lens, const OutputPlan& plan,
                        const OutputTables& t, float* d_y, void* d_packed, hipStream_t s) {
    launch_pack_plan(audio, audio_ld, plan, t, d_y, d_packed, s);
    if (plan.n_marks > 0) launch_token_marks(dur, lens, plan, t, static_cast<char*>(d_packed) + plan.marks_off, s);
}

// ---- joins: the used durations of every row's first and last token, for the host's join plan ---------------------------------
// edges[b] = {dur[b][0], dur[b][lens[b] - 1]}: eight bytes per row behind the duration head, copied to the host beside the
// frame counts before the forward's one host wait.
__global__ void edge_durations_kernel(const int* __restrict__ dur, const int* __restrict__ lens, int2* __restrict__ edges, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int T = min(max(lens[b], 1), 512);
    edges[b] = make_int2(dur[(long)b * 512], dur[(long)b * 512 + T - 1]);
}
void launch_edge_durations(const int* dur, const int* lens, int* edges, int B, hipStream_t s) {
    KX_REQUIRE(dur && lens && edges && B >= 1 && (reinterpret_cast<uintptr_t>(edges) & 7) == 0, "join: bad launch argument");
    hipLaunchKernelGGL(edge_durations_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, dur, lens,
                       reinterpret_cast<int2*>(edges), B);
    KX_HIP(hipGetLastError());
}

}  // namespace kx
