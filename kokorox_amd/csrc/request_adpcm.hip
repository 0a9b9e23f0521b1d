// The IMA ADPCM encoder of the output stage (gfx950): the 16-bit values of a request's final stream (request_stream.h:
// stage_final) as a WAV file of 4-bit blocks, every block straight to its place in the region.
#include "kx_common.h"
#include "adpcm_steps.h"
#include "request_stream.h"
#include "request_units.h"

namespace kx {

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
    // the final stream's samples; every lane converts what it staged itself (sample i: lane (i - t0) mod 256)
    const long lim_off = lrows ? lrows[r].off : -1;
    const bool scaled = lim_off < 0 && levels != nullptr;  // (the gain rule of stage_final, needed before the first tile)
    const double g = scaled ? levels[2 * r + 1] : 1.0;
    for (long t0 = n0; t0 < n1; t0 += ADPCM_TILE) {
        const long t1 = t0 + ADPCM_TILE < n1 ? t0 + ADPCM_TILE : n1;
        stage_final<ADPCM_THREADS, -1, false>(ftile, audio, audio_ld, cum, jrows, y, lim, lim_off, levels, (unsigned)r, rq.rate, rq.y_off,
                                              rq.first_row, rq.n_rows, t0, t1);
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

// ADPCM: every block of every form-17 request straight to its place, from the samples the packer launched behind this stage would
// stage; it needs no table of its own
void launch_adpcm_stage(const float* audio, long audio_ld, const OutputPlan& plan, const OutputTables& t, float* d_y, char* out,
                        hipStream_t s) {
    const bool gains = plan.limited || plan.levelled;
    KX_REQUIRE(plan.adpcm_groups <= 0x7FFFFFFF, "adpcm: too many blocks");
    launch_checked(adpcm_blocks_kernel, dim3((unsigned)plan.adpcm_groups, (unsigned)plan.req.size()), dim3(ADPCM_THREADS), s, audio, audio_ld, t.req,
                   t.cum, plan.joined || gains ? t.join : nullptr, d_y, gains ? plan_levels(plan, out) : nullptr, plan.limited ? t.limit : nullptr,
                   plan.limited ? t.lim : nullptr, out);
}

}  // namespace kx
