// The packer of the output stage (gfx950): every request of the batch as the bytes a server sends, in its form -- samples, WAV,
// base64, G.711 -- from the request's final stream (request_stream.h: stage_final).  host_request.h has the tables it reads.
#include "kx_common.h"
#include "request_stream.h"
#include "request_units.h"

namespace kx {

// ---- requests of several chunks, packed as the bytes a server sends ---------------------------------------------
// A request's region is a function of a VIRTUAL BYTE STREAM: the header of its form, then the sample bytes of its rows in
// order (the chunk loop of koko.rs:947-1191 appends the waveforms with no cross-fade).  Forms 0..2 are the bare samples (request_stream.h)
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
// A request with a rate code (PackReq::rate) was resampled as a whole by resample_requests_kernel (request_resample.hip): its stream is then
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
    stage_final<PACK_THREADS, JOINED ? 1 : 0, LEVELLED>(smp, audio, audio_ld, cum, jrows, y, lim, lim_off, levels, blockIdx.y, rq.rate,
                                                        rq.y_off, rq.first_row, rq.n_rows, s_lo, s_hi);
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

// The packer of a plan, the form its flags name: limited, else levelled, else joined, else plain.
void launch_pack_stage(const float* audio, long audio_ld, const OutputPlan& plan, const OutputTables& t, float* d_y, char* out,
                       hipStream_t s) {
    if (plan.max_units <= 0) return;  // (a measured plan of empty requests: its levels are written, there is no body)
    const dim3 grid((unsigned)((plan.max_units + PACK_THREADS - 1) / PACK_THREADS), (unsigned)plan.req.size()), block(PACK_THREADS);
    double* levels = plan_levels(plan, out);
    if (plan.limited) launch_checked(pack_requests_limited_kernel, grid, block, s, audio, audio_ld, t.req, t.cum, t.join, d_y, out, levels, t.limit, t.lim);
    else if (plan.levelled) launch_checked(pack_requests_levelled_kernel, grid, block, s, audio, audio_ld, t.req, t.cum, t.join, d_y, out, levels);
    else if (plan.joined) launch_checked(pack_requests_joined_kernel, grid, block, s, audio, audio_ld, t.req, t.cum, t.join, d_y, out);
    else launch_checked(pack_requests_kernel, grid, block, s, audio, audio_ld, t.req, t.cum, d_y, out);
}

}  // namespace kx
