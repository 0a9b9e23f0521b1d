// The look-ahead limiter of the output stage (gfx950) and its report: a limited request's stream, driven by the gain the levels
// unit left, into the limit buffer that the packer and the encoders read in place of the rows (request_stream.h: stage_final).
#include "kx_common.h"
#include "limit_taps.h"
#include "request_stream.h"
#include "request_truepeak.h"
#include "request_units.h"

namespace kx {

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
        stage_rows<LIM_THREADS>(dst, audio, audio_ld, cum, jrows, rq.first_row, rq.n_rows, s_lo, s_hi);
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

// The limiter of a plan with a limited request, behind the gains it is driven by: every limited request's z2 into the limit buffer,
// then its five values.
void launch_limit_stage(const float* audio, long audio_ld, const OutputPlan& plan, const OutputTables& t, float* d_y, char* out,
                        hipStream_t s) {
    const unsigned R = (unsigned)plan.req.size();
    double* levels = plan_levels(plan, out);
    if (plan.peak_windows > 0)
        launch_checked(request_limit_kernel, dim3((unsigned)plan.peak_windows, R), dim3(LIM_THREADS), s, audio, audio_ld, t.req, t.cum,
                       plan.joined ? t.join : nullptr, d_y, t.limit, levels, t.lim, t.lpart, plan.peak_windows);
    launch_checked(request_limit_report_kernel, dim3(R), dim3(64), s, t.req, t.limit, t.lpart, plan.peak_windows, levels,
                   reinterpret_cast<double*>(out + plan.loud_off), reinterpret_cast<double*>(out + plan.limits_off));
}

}  // namespace kx
