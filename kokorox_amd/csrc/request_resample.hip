// The output-rate resampler of the output stage (gfx950): a request's rows through a polyphase FIR into the run at y + y_off that
// every later stage reads, whole or piece by piece, and the carry a piece leaves for the next call.
#include "kx_common.h"
#include "resample_taps.h"
#include "request_stream.h"
#include "request_units.h"

namespace kx {

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

// The chains that the whole-stream and the piece form share, so that their bits are the same by construction (the four lines of
// the window's bounds stay written out in both bodies: as a function of their own they changed the whole-stream kernels' code and
// cost the joined one two registers: profiles/request_units_codegen.txt, variant 2).
// the lane's outputs n0 + t + 256 k of [n0, n1), from the window xs = x[j_lo ..] and the taps hs; output n goes to dst[n - out0]
__device__ __forceinline__ void resample_outputs(long n0, long n1, long S, int L, int M, int C, const float* xs, const double* hs,
                                                 long j_lo, float* dst, long out0) {
    for (long n = n0 + threadIdx.x; n < n1; n += RS_THREADS) {
        const long a = n * M - C;
        const long jl = a <= 0 ? 0 : (a + L - 1) / L;  // >= j_lo, as n >= n0
        long jh = (n * M + C) / L;                      // < j_hi, as n < n1
        jh = jh > S - 1 ? S - 1 : jh;
        int idx = (int)(n * M - jl * L) + C;            // <= 2 C, as jl L >= n M - C; stays >= 0 down to j = jh
        const float* xp = xs + (jl - j_lo);
        double acc = 0.0;
        for (long j = jl; j <= jh; ++j, idx -= L) acc += hs[idx] * (double)*xp++;
        dst[n - out0] = (float)acc;
    }
}

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
    resample_outputs(n0, n1, S, L, M, C, xs, hs, j_lo, y + rq.y_off, 0);
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
// resample_requests_body on the whole stream -- both run resample_outputs: the same bits.  A request run whole is the piece [0, N) of [0, S) without a tail.
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
    resample_outputs(n0, n1, S, L, M, C, xs, hs, j_lo, y + rq.y_off, pr.emit_lo);
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

// The resampler of a plan some request of which carries a rate code -- the piece form for every request of a plan with pieces, the
// ones run whole included: the same bits -- and the carries of a plan with pieces, into their block behind everything else: they
// depend on the rows and the old tails alone.
void launch_resample_stage(const float* audio, long audio_ld, const OutputPlan& plan, const OutputTables& t, float* d_y, char* out,
                           hipStream_t s) {
    const unsigned R = (unsigned)plan.req.size();
    if (plan.y_floats > 0) {
        KX_REQUIRE(d_y != nullptr, "pack: no buffer for the resampled streams");
        const dim3 grid((unsigned)((plan.max_resampled + RS_WINDOW - 1) / RS_WINDOW), R), block(RS_THREADS);
        if (plan.has_pieces() && plan.joined)
            launch_checked(resample_pieces_joined_kernel, grid, block, s, audio, audio_ld, t.req, t.piece, t.cum, t.join, t.piece_tail, d_y);
        else if (plan.has_pieces()) launch_checked(resample_pieces_kernel, grid, block, s, audio, audio_ld, t.req, t.piece, t.cum, t.piece_tail, d_y);
        else if (plan.joined) launch_checked(resample_requests_joined_kernel, grid, block, s, audio, audio_ld, t.req, t.cum, t.join, d_y);
        else launch_checked(resample_requests_kernel, grid, block, s, audio, audio_ld, t.req, t.cum, d_y);
    }
    if (plan.has_pieces())
        launch_checked(piece_carry_kernel, dim3(R), dim3(PIECE_TAIL), s, audio, audio_ld, t.req, t.piece, t.cum, t.join, t.piece_tail, out);
}

}  // namespace kx
