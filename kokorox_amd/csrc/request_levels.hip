// What the output stage measures of a request's stream (gfx950): its sample peak and true peak, its BS.1770 loudness, and the gain
// either of them leads to, into the levels and loudness blocks of the packed buffer.  The packer and the limiter apply the gain.
#include "kx_common.h"
#include "kweight_coefs.h"
#include "request_stream.h"
#include "request_truepeak.h"
#include "request_units.h"

namespace kx {

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
        stage_rows<PEAK_THREADS>(xs, audio, audio_ld, cum, jrows, rq.first_row, rq.n_rows, n0, n1);
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
        stage_rows<TP_THREADS>(dst, audio, audio_ld, cum, jrows, rq.first_row, rq.n_rows, s_lo, s_hi);
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
        stage_rows<LOUD_THREADS>(dst, audio, audio_ld, cum, jrows, rq.first_row, rq.n_rows, s_lo, s_hi);
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

// The measurements of a measured plan, behind the resampler: peak pass, meter, true peak, then the two gain kernels.
void launch_measure_stage(const float* audio, long audio_ld, const OutputPlan& plan, const OutputTables& t, float* d_y, char* out,
                          hipStream_t s) {
    const unsigned R = (unsigned)plan.req.size();
    const bool loud = !plan.loud.empty();
    const JoinRow* jrows = plan.joined ? t.join : nullptr;
    double* levels = plan_levels(plan, out);
    const uint32_t* tpeak = plan.true_peak ? t.tpeak : nullptr;  // (read for a flagged request only)
    if (plan.peak_windows > 0)
        launch_checked(request_peak_kernel, dim3((unsigned)plan.peak_windows, R), dim3(PEAK_THREADS), s, audio, audio_ld, t.req, t.cum, jrows, d_y,
                       t.peak, plan.peak_windows);
    if (loud && plan.max_hops > 0)
        launch_checked(request_loudness_kernel, dim3((unsigned)plan.max_hops, R), dim3(LOUD_THREADS), s, audio, audio_ld, t.req, t.cum, jrows, d_y,
                       t.loud, t.loud_pow, t.hops, plan.max_hops);
    // the true peak of the flagged requests into the second table, [R][peak_windows] as the first: the gain kernels join the two
    if (plan.true_peak && plan.peak_windows > 0) {
        KX_REQUIRE(t.tpeak != nullptr, "levels: no table for the true peak");
        launch_checked(request_truepeak_kernel, dim3((unsigned)plan.peak_windows, R), dim3(TP_THREADS), s, audio, audio_ld, t.req, t.cum, jrows, d_y,
                       t.level, loud ? t.loud : nullptr, t.tpeak, plan.peak_windows);
    }
    // (a metered request's {p, g} slot is the loudness gain kernel's: request_gain_kernel, which runs only when some request is
    // not metered, leaves the plain spec's {p, 1} there and the later kernel of the same stream stores the request's own)
    if (!plan.loud_all) launch_checked(request_gain_kernel, dim3(R), dim3(64), s, t.req, t.level, t.peak, tpeak, plan.peak_windows, levels);
    if (loud)
        launch_checked(request_loudness_gain_kernel, dim3(R), dim3(64), s, t.req, t.loud, t.peak, tpeak, plan.peak_windows, t.hops, plan.max_hops,
                       levels, reinterpret_cast<double*>(out + plan.loud_off));
}

}  // namespace kx
