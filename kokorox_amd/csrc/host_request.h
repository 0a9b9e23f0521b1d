// What a call is refused for before it touches the device, and where its output bytes go: the argument checks of the two
// inference entries (Model::infer_host_once, Model::infer_device) and the layout of the compact output.  Plain C++17, no HIP
// header: built with g++ and the sanitizers by the CPU suite (tests/cpp/host_request_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "kx_error.h"

namespace kx {

// A request's join spec: the layout of kx_join (include/kokorox_hip.h, "joins"; api.hip asserts the two agree).
struct JoinSpec {
    uint32_t flags;    // JOIN_TRIM_* bits, every other bit zero
    int32_t keep_ms;   // 0..1000
    int32_t pause_ms;  // 0..5000
    int32_t fade_ms;   // 0..12
};
constexpr uint32_t JOIN_TRIM_HEAD = 1u, JOIN_TRIM_TAIL = 2u, JOIN_TRIM_INNER = 4u;
inline bool join_spec_ok(const JoinSpec& j) {
    return (j.flags & ~7u) == 0 && j.keep_ms >= 0 && j.keep_ms <= 1000 && j.pause_ms >= 0 && j.pause_ms <= 5000 && j.fade_ms >= 0 &&
           j.fade_ms <= 12;
}
inline bool join_spec_plain(const JoinSpec& j) { return j.flags == 0 && j.keep_ms == 0 && j.pause_ms == 0 && j.fade_ms == 0; }

// A request's level spec: the layout of kx_level (include/kokorox_hip.h, "levels"; api.hip asserts the two agree).
struct LevelSpec {
    uint32_t mode;  // LEVEL_GAIN, LEVEL_NORMALIZE or LEVEL_CEILING
    float gain;     // 0..64; exactly 1 in mode 1
    float peak;     // +0 in mode 0; 2^-15..1 in modes 1 and 2
};
constexpr uint32_t LEVEL_GAIN = 0u, LEVEL_NORMALIZE = 1u, LEVEL_CEILING = 2u;
inline uint32_t level_float_bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}
// (every comparison is written so that a NaN fails it)
inline bool level_spec_ok(const LevelSpec& l) {
    if (l.mode > LEVEL_CEILING || !(l.gain >= 0.0f && l.gain <= 64.0f)) return false;
    if (l.mode == LEVEL_GAIN) return level_float_bits(l.peak) == 0u;  // +0.0f and nothing else
    return (l.mode != LEVEL_NORMALIZE || l.gain == 1.0f) && l.peak >= 0x1p-15f && l.peak <= 1.0f;
}
inline bool level_spec_plain(const LevelSpec& l) { return l.mode == LEVEL_GAIN && l.gain == 1.0f && level_float_bits(l.peak) == 0u; }
// samples of a request's stream (at its output rate) that one workgroup of the peak pass reduces (request_kernels.hip)
constexpr long LEVEL_WINDOW = 4096;

// A request's loudness spec: the layout of kx_loudness (include/kokorox_hip.h, "loudness"; api.hip asserts the two agree).
struct LoudSpec {
    uint32_t mode;      // LOUD_MEASURE or LOUD_NORMALIZE (LOUD_NONE: inside a plan only, a request beside loudness ones that has none)
    float target_lufs;  // +0 in mode 0; -70..0 in mode 1
    float peak;         // +0 in mode 0; 2^-15..1 in mode 1
};
constexpr uint32_t LOUD_MEASURE = 0u, LOUD_NORMALIZE = 1u, LOUD_NONE = 0xFFFFFFFFu;
// (every comparison is written so that a NaN fails it)
inline bool loud_spec_ok(const LoudSpec& l) {
    if (l.mode == LOUD_MEASURE) return level_float_bits(l.target_lufs) == 0u && level_float_bits(l.peak) == 0u;
    return l.mode == LOUD_NORMALIZE && l.target_lufs >= -70.0f && l.target_lufs <= 0.0f && l.peak >= 0x1p-15f && l.peak <= 1.0f;
}
// The meter's grid at rate code c (request_kernels.hip: request_loudness_kernel): a hop of 100 ms, the warm-up a workgroup runs from
// zero state before its hop (the tail of sum |h| of the K-weighting beyond it is below 1e-15), and the odd number of samples one of
// its LOUD_THREADS lanes runs: LOUD_THREADS * loud_run(c) >= loud_warmup(c) + loud_hop(c).
constexpr int LOUD_THREADS = 256;
constexpr int LOUD_POWERS = 65;  // A^(run k), k = 0..64, of a rate's 4x4 transition matrix: 16 doubles each, row-major
constexpr double LOUD_ABS_GATE = 1.1724653045822981e-07;  // 10^((-70 + 0.691) / 10)
constexpr long loud_rate_hz(int c) { return c == 1 ? 8000 : (c == 2 ? 16000 : (c == 3 ? 48000 : 24000)); }
constexpr long loud_hop(int c) { return loud_rate_hz(c) / 10; }
constexpr long loud_warmup(int c) { return c == 1 ? 1536 : (c == 2 ? 3072 : (c == 3 ? 8192 : 4096)); }
constexpr int loud_run(int c) { return (int)((loud_warmup(c) + loud_hop(c) + LOUD_THREADS - 1) / LOUD_THREADS) | 1; }
// the ten K-weighting coefficients of rate code 0..3 (kweight_coefs.h: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2)
const double* loud_coefs(int rate_code);  // throws KX_ERR_INVALID outside 0..3
// [4][LOUD_POWERS][16]: the powers of every rate's transition matrix over the state (v[n-1], v[n-2], w[n-1], w[n-2]) of the cascade
const double* loud_powers();

// What a call asks of the output stage (a view: the arrays are the caller's): how its rows group into requests, and each
// request's format word, wish for token marks, join spec, level spec and loudness spec.  build_output_plan and output_bounds take it.
struct RequestLayout {
    const int32_t* chunks_per_request;  // [R] rows of each request; null: every row a request of its own, and R = B
    int R;
    const int32_t* formats;             // [n_format] format words (check_format_word), n_format = 1 (shared) or R
    int n_format;
    const uint8_t* marks;               // [R] request r wants token marks when marks[r] != 0; null: none does
    const JoinSpec* joins;              // [n_join] with n_join = 1 (shared) or R; null: the rows are appended as they are
    int n_join;
    const LevelSpec* levels;            // [n_level] with n_level = 1 (shared) or R; null: nothing is measured or scaled
    int n_level;
    const LoudSpec* loudness;           // [n_loudness] with n_loudness = 1 (shared) or R; null: no request is metered (a spec of mode
    int n_loudness;                     // LOUD_NONE: that request is not)
};

// general host entry behind kx_infer / kx_infer_voices / kx_infer_packed / kx_infer_requests (Model::infer_host_ex)
struct HostCall {
    const float* styles = nullptr;       // host [B][256], or
    const int32_t* voice_ids = nullptr;  // host [B][max_mix] into the device voice table
    const float* weights = nullptr;      // host [B][max_mix]
    int max_mix = 0;
    const uint64_t* utt_seeds = nullptr;
    int format = 0;                      // 0 f32 mono, 1 f32 stereo, 2 pcm16 mono: every row a region of its own in that form
    // per-utterance kinds (the dispatcher's mixed batches); null = the batch-wide fields above
    const int32_t* kinds = nullptr;      // host [B]: 0 = row of `styles`, 1 = single voice (copy), 2 = mix
    // requests of several chunks (kx_infer_requests, the dispatcher): rows are chunks, request r owns chunks_per_request[r]
    // consecutive rows and comes out as ONE region (header of its form, then its rows' samples with nothing between them);
    // out_bytes / out_samples of the call then have n_requests entries and `format` is not used
    const int32_t* chunks_per_request = nullptr;  // host [n_requests], every entry >= 1, sum = B
    int n_requests = 0;
    const int32_t* req_formats = nullptr;         // host [n_req_formats], format words (form | rate code << 8: check_format_word)
    int n_req_formats = 0;                        // 1 (shared) or n_requests
    const uint32_t* utt_index = nullptr;          // host [B] beside utt_seeds: row b draws (utt_seeds[b], utt_index[b])
    // token timing marks (include/kokorox_hip.h, "token marks"): request r wants them when req_marks[r] != 0; null = none
    const uint8_t* req_marks = nullptr;           // host [n_requests]
    // joins (include/kokorox_hip.h, "joins"): request r is shaped by req_joins[n_req_joins == 1 ? 0 : r]; null = none
    bool join_call = false;                       // the entry that takes joins: req_joins must then be there (check_join_call)
    const JoinSpec* req_joins = nullptr;          // host [n_req_joins]
    int n_req_joins = 0;                          // 1 (shared) or n_requests
    // levels (include/kokorox_hip.h, "levels"): request r is measured and scaled by req_levels[n_req_levels == 1 ? 0 : r]; null = none
    bool level_call = false;                      // the entry that takes levels: req_levels must then be there (check_level_call)
    const LevelSpec* req_levels = nullptr;        // host [n_req_levels]
    int n_req_levels = 0;                         // 1 (shared) or n_requests
    // loudness (include/kokorox_hip.h, "loudness"): request r is metered and scaled by req_loudness[n_req_loudness == 1 ? 0 : r]; null = none
    bool loud_call = false;                       // the entry that takes loudness: req_loudness must then be there (check_loudness_call)
    const LoudSpec* req_loudness = nullptr;       // host [n_req_loudness]
    int n_req_loudness = 0;                       // 1 (shared) or n_requests

    bool grouped() const { return chunks_per_request != nullptr; }
    bool by_voice() const { return voice_ids != nullptr; }
    int kind_of(int b) const { return kinds ? kinds[b] : (by_voice() ? (max_mix == 1 ? 1 : 2) : 0); }
    // what the call asks of the output stage: a call without chunks_per_request is B single-row requests sharing `format`
    RequestLayout layout(int B) const {
        if (!grouped()) return RequestLayout{nullptr, B, &format, 1, nullptr, nullptr, 0, nullptr, 0};
        return RequestLayout{chunks_per_request, n_requests, req_formats, n_req_formats, req_marks, req_joins, n_req_joins, req_levels,
                             n_req_levels, req_loudness, n_req_loudness};
    }
};

// ---- the refusals, side by side.  The two entries word some of them differently (a row longer than the stride, for one):
// each keeps its own text; callers and tests match on them. ----------------------------------------------------------------
// Everything Model::infer_host_once refuses before its first device call, in its order of precedence; *out is cleared once
// the output arguments are known to be there.
void check_host_call(const int64_t* ids, int64_t t_stride, const int32_t* lens, int B, const float* speeds, const HostCall& hc,
                     void** out, const int64_t* out_bytes, const int64_t* out_samples, int n_vocab, int n_voices,
                     bool have_voice_table);
// The entries that return token marks (HostCall::req_marks set): their two extra output arguments, checked after everything
// above; *out_marks is cleared.  throws KX_ERR_INVALID: "infer: null marks argument"
void check_marks_call(const HostCall& hc, int64_t** out_marks, int64_t* out_n_marks);
// The entry that takes joins (HostCall::join_call; req_joins / n_req_joins as the caller gave them, a null pointer included),
// checked after check_host_call.  throws KX_ERR_INVALID: "infer: null join argument", "infer: bad join count" (not 1 or R),
// "infer: bad join" (a stray flag bit or a field outside its range).  Its marks arguments may both be null (no marks); exactly
// one null is check_marks_call's refusal.
void check_join_call(const HostCall& hc);
// The entry that takes levels (HostCall::level_call), checked after everything above.  throws KX_ERR_INVALID: "infer: null level
// argument", "infer: bad level count" (not 1 or R), "infer: bad level" (level_spec_ok fails).
void check_level_call(const HostCall& hc);
// The entry that takes loudness (HostCall::loud_call), checked after everything above.  throws KX_ERR_INVALID: "infer: null loudness
// argument", "infer: bad loudness count" (not 1 or R), "infer: bad loudness" (loud_spec_ok fails).
void check_loudness_call(const HostCall& hc);
// Everything Model::infer_device refuses before hipSetDevice; returns the longest token count.
int check_device_call(const void* d_ids, int64_t t_stride, const int32_t* lens_host, int B, const void* d_styles,
                      const float* speeds_host, int n_speed);

// ---- the format word of the request entries (include/kokorox_hip.h, KX_PACK_*) -------------------------------------------
// bits 0..7 = the form (0..4, 8 = G.711 mu-law, 9 = G.711 A-law), bits 8..11 = the rate code (0 = 24 000 Hz, 1 = 8000,
// 2 = 16 000, 3 = 48 000), every other bit zero.
inline int format_form(int word) { return word & 0xFF; }
inline int format_rate(int word) { return (word >> 8) & 15; }
// throws KX_ERR_INVALID: "infer: unknown output format" (forms 5..7 and above 9, stray bits, negative words), then
// "infer: unknown output sample rate" (rate codes 4..15)
void check_format_word(int word);

// The FIR of rate code 1..3 (resample_taps.h, generated by tools/gen_resample_taps.py): output n of a stream x[0..S) is
// f32(sum over j ascending of f64(taps[n M - j L + C]) * f64(x[j])), S L / M outputs in all.
struct ResampleFilter {
    int L, M, C, n_taps;
    const float* taps;
};
const ResampleFilter& resample_filter(int rate_code);  // throws KX_ERR_INVALID outside 1..3
long resampled_samples(int rate_code, long n_samples);  // n_samples L / M (exact for whole frames); code 0: n_samples

// ---- the output stage of a call: every request packed as the bytes a server sends (request_kernels.hip) ----------------------
// A request is n_rows consecutive rows of the audio slab; its output is a function of a virtual byte stream: the header of
// its form (if any), then the sample bytes of its rows in order with nothing between them.  Forms 0..2 are the bare samples
// (f32, f32 written twice, PCM16: request_kernels.hip, pcm16_sample), 3 = 44-byte float WAV header + f32 bit copies, 4 = base64
// of a 16-bit WAV file, 8 / 9 = G.711 bytes (include/kokorox_hip.h, KX_PACK_*).  With a rate code the stream is first resampled as a whole (resample_requests_kernel) into a buffer of
// plan.y_floats floats, and the packer reads the request as ONE row of that buffer.
struct PackReq {
    int first_row, n_rows, form, rate;  // form = bits 0..7 of the word; rate = its rate code
    long out_off;      // byte offset of the request's region in the compact output (a multiple of 4)
    long out_bytes;    // size of the region (a multiple of 4 in every form)
    long n_samples;    // samples of the region, at the output rate: the samples of its stream * L / M
    long src_samples;  // samples of its stream at 24 000 Hz: 600 * the sum of its rows' frames when nothing joins them
    long y_off;        // rate code != 0: floats before the request's resampled stream in the intermediate buffer
};
// Joins: a kept segment of each row, then a run of zeros (include/kokorox_hip.h, "joins").  Row b of a request contributes
// x[skip .. skip + keep) of its 600 frames[b] valid samples, the first fade_head and the last fade_tail of them faded, then gap
// zeros.  The staging step of the joined packer and resampler reads this table beside the prefix table, which runs over
// keep + gap (OutputPlan::cum), so PackReq's sizes follow the joined stream S'.  A row nothing shapes: {0, 600 frames[b], 0, 0, 0}.
struct JoinRow {
    long skip, keep, gap;      // samples at 24 000 Hz, multiples of 24
    int fade_head, fade_tail;  // 24 fade_ms where that edge is trimmed, else 0
};
// Token timing marks behind the bodies (request_kernels.hip: token_marks_kernel; include/kokorox_hip.h has the definition):
// per chunk its tokens + 1 int64 sample offsets at the request's output rate.  They live in a block of their own in the packed
// buffer, at total_bytes rounded up to 8, the requests that want them back to back in request order, so body and marks leave
// the device in one copy.  One MarkRow per ROW of the batch; the packer's and the resampler's table (PackReq) does not know
// about marks.
struct MarkRow {
    long first;  // index (in int64 values) of the row's first mark in the marks block; -1: its request wants none
    long base;   // the row's first mark: the samples of the request's earlier rows (their pauses included) x L / M
    long K;      // output samples per frame: 600 L / M of the request's rate (600, 200, 400, 1200)
    // what the joined form of the kernel clamps with (the row's JoinRow), at 24 000 Hz
    long src_base = 0;  // samples of the request's stream before the row: base = src_base x L / M
    long skip = 0, keep = 0;
};
inline long frame_samples(int rate_code) { return rate_code == 1 ? 200 : (rate_code == 2 ? 400 : (rate_code == 3 ? 1200 : 600)); }

// Everything the output stage of one call is launched with (kx_common.h: launch_output_plan), from build_output_plan.
struct OutputPlan {
    std::vector<PackReq> req;  // [R]
    std::vector<long> cum;     // [B + 1] samples (keep + gap) of the rows before row b, over the whole batch
    long total_bytes = 0;
    long max_units = 0;      // 16-byte units of the largest region (the packer's grid)
    long y_floats = 0;       // floats of the intermediate buffer: the resampled streams back to back (0: nothing to resample)
    long max_resampled = 0;  // most output samples of one resampled request (the resampler's grid)
    std::vector<JoinRow> join;  // [B]
    bool joined = false;        // some request's spec is not all zeros: the joined form of the kernels is launched
    std::vector<MarkRow> mark;  // [B]; empty when the token counts were not given
    std::vector<long> count;    // [R] marks of request r: the sum over its rows of lens + 1, or 0 when it wants none
    std::vector<long> first;    // [R] index of request r's first mark in the block
    long marks_off = 0;         // byte offset of the block in the packed buffer (a multiple of 8, >= total_bytes)
    long n_marks = 0;           // int64 values of the block
    // Levels (include/kokorox_hip.h, "levels"; request_kernels.hip: request_peak_kernel, request_gain_kernel): a third block
    // behind the marks, [R]{double p, double g}, so body, marks and levels still leave the device in one copy.
    std::vector<LevelSpec> level;  // [R]; empty when the layout has no levels
    bool measured = false;         // levels were given: every request's peak is taken and its {p, g} stored
    bool levelled = false;         // some spec is not the plain one: the levelled packer runs
    long levels_off = 0;           // byte offset of the block (a multiple of 8, >= marks_off + 8 n_marks); 0 when not measured
    long peak_windows = 0;         // LEVEL_WINDOW-sample windows of the longest request: the peak pass's grid and table stride
    long peak_dwords() const { return measured ? (long)req.size() * peak_windows : 0; }  // the partials table [R][peak_windows]
    // Loudness (include/kokorox_hip.h, "loudness"; request_kernels.hip: request_loudness_kernel, request_loudness_gain_kernel): a
    // fourth block behind the levels, [R]{double I, double n_g}.  A plan with loudness is measured: the metered requests' {p, g} come
    // from the loudness gain kernel, the others' from request_gain_kernel (the plain spec where the layout gave no levels).
    std::vector<LoudSpec> loud;    // [R], LOUD_NONE where a request is not metered; empty when the layout has no loudness
    bool loud_all = false;         // every request is metered: request_gain_kernel has no slot to write
    long loud_off = 0;             // byte offset of the block: levels_off + 16 R; 0 without loudness
    long max_hops = 0;             // whole hops of the metered request that has most: the meter's grid and the stride of its table
    long hop_doubles() const { return (long)loud.size() * max_hops; }  // the hop energies [R][max_hops]
    // bytes of body + marks (+ levels (+ loudness)): what one copy brings to the host
    long end_bytes() const {
        return !loud.empty() ? loud_off + 16 * (long)req.size() : (measured ? levels_off + 16 * (long)req.size() : marks_off + 8 * n_marks);
    }
};
// `form` = a format word, n_samples at 24 000 Hz.  throws KX_ERR_INVALID: unknown word, 16-bit WAV past 4 GiB
long pack_request_bytes(int form, long n_samples);
// The plan of a call whose frame counts are known.  frames [B]; lens [B] tokens per row (may be null when the layout has
// neither marks nor joins); edges [B][2] = the used durations of each row's first and last token, in frames (may be null when
// it has no joins).  A layout without joins is the plain case of the same walk (JoinRow above), and so is a spec of all zeros:
// plan.joined stays false and the plain kernels run.
void build_output_plan(const int* frames, const int* lens, const int* edges, int B, const RequestLayout& layout, OutputPlan& plan);

// What a call of B rows needs before its forward has run, for n_samples samples (at 24 000 Hz) in all -- with joins the pauses
// come on top, 24 pause_ms (rows_r - 1) per request; trimming only shrinks.  packed_bytes: R requests, every one in the widest
// of the layout's words (48 000 Hz doubles the samples; the per-request header and the base64 padding do not scale with the
// samples); with marks (lens [B] then required) 8 + 8 x the sum over the rows of lens + 1 more: the alignment gap and a block
// in which every request wants them.  y_floats: the intermediate buffer of the resampled streams, 0 when no word carries a
// rate code.  With levels 8 + 16 R bytes more (the alignment gap and the block), and peak_dwords: the partials table of the peak
// pass, R rows of the windows the longest request can have.  With loudness 16 R bytes more (and the levels' share when the layout
// has none), and hop_doubles: the hop energies, R rows of the hops all the samples can make (a hop is 100 ms at every rate).
struct OutputBounds {
    size_t packed_bytes, y_floats, peak_dwords, hop_doubles;
};
OutputBounds output_bounds(const RequestLayout& layout, int B, size_t n_samples, const int32_t* lens);

}  // namespace kx
