// A request's stream on the device (gfx950): what sample i of request r is at each stage of the output stage -- the rows the
// model wrote, plain or joined (stage_stream, stage_rows), the run the resampler left at y + y_off, the gain of the levels block and
// the run the limiter left (stage_final) -- and its 16-bit value (pcm16_sample).  Every request_*.hip unit stages through these.
#pragma once
#include "kx_common.h"

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
// The rows of request rq, joined where the plan handed the kernel its join rows and plain where it passed none: the run-time form of
// the choice, for the kernels that are not compiled once per form.
template <int THREADS>
__device__ __forceinline__ void stage_rows(float* __restrict__ dst, const float* __restrict__ audio, long audio_ld,
                                           const long* __restrict__ cum, const JoinRow* __restrict__ jrows, int first_row, int n_rows,
                                           long lo_i, long hi_i) {
    if (jrows) stage_stream<true, THREADS>(dst, audio, audio_ld, cum, jrows, first_row, n_rows, lo_i, hi_i);
    else stage_stream<false, THREADS>(dst, audio, audio_ld, cum, jrows, first_row, n_rows, lo_i, hi_i);
}

// The FINAL stream of request r, the one whose 16-bit values and bytes leave: samples [lo, hi) of it into dst[0 .. hi - lo), lanes
// along time.  It is the limited run at lim + lim_off where the limiter ran on the request (lim_off >= 0: scaled and limited
// already), else the resampled run at y + y_off where the request has a rate code, else its rows -- and, unless limited, every
// sample z becomes f32(g * f64(z)) with g = levels[2 r + 1] in a levelled plan (include/kokorox_hip.h, "levels", "limiter").
// ROWS: 0 = plain, 1 = joined, -1 = as jrows says (stage_rows).  SCALE: the plan is levelled and the product is formed here, in
// the copy of a run and in place behind the row lookup (every lane scales the samples it staged itself: sample i belongs to lane
// (i - lo) mod THREADS, so no barrier lies between).  Without SCALE the samples are staged as they are and the caller, which knows
// at run time only whether the plan is levelled, forms the product where it converts them: it owes the product where the request is
// not limited and the plan has gains (lim_off < 0 && levels != nullptr), a rule the encoders state themselves because they need g
// before the first tile.  A caller without a limiter passes lim_off = -1; levels is read with SCALE alone.  The request's fields
// come as scalars, not as the record: a reference into the caller's copy of it changes how the caller itself is compiled.
template <int THREADS, int ROWS, bool SCALE>
__device__ __forceinline__ void stage_final(float* __restrict__ dst, const float* __restrict__ audio, long audio_ld,
                                            const long* __restrict__ cum, const JoinRow* __restrict__ jrows, const float* __restrict__ y,
                                            const float* __restrict__ lim, long lim_off, const double* __restrict__ levels, unsigned r,
                                            int rate, long y_off, int first_row, int n_rows, long lo_i, long hi_i) {
    if (lim_off >= 0) {  // (uniform) a limited request: one contiguous run, scaled and limited already
        const float* __restrict__ src = lim + lim_off;
        for (long i = lo_i + threadIdx.x; i < hi_i; i += THREADS) dst[i - lo_i] = src[i];
    } else if (rate) {  // (uniform) a resampled request: one contiguous run
        const float* __restrict__ src = y + y_off;
        if (SCALE) {
            const double g = levels[2 * r + 1];
            for (long i = lo_i + threadIdx.x; i < hi_i; i += THREADS) dst[i - lo_i] = (float)(g * (double)src[i]);
        } else {
            for (long i = lo_i + threadIdx.x; i < hi_i; i += THREADS) dst[i - lo_i] = src[i];
        }
    } else {
        if (ROWS < 0) stage_rows<THREADS>(dst, audio, audio_ld, cum, jrows, first_row, n_rows, lo_i, hi_i);
        else stage_stream<ROWS != 0, THREADS>(dst, audio, audio_ld, cum, jrows, first_row, n_rows, lo_i, hi_i);
        if (SCALE) {
            const double g = levels[2 * r + 1];
            for (long i = lo_i + threadIdx.x; i < hi_i; i += THREADS) dst[i - lo_i] = (float)(g * (double)dst[i - lo_i]);
        }
    }
}

}  // namespace kx
