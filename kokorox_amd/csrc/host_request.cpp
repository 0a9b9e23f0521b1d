// The argument checks of the two inference entries and the layout of their compact output (host_request.h).  No HIP.
#include "host_request.h"

#include <cstring>

#include "adpcm_steps.h"
#include "kweight_coefs.h"
#include "limit_taps.h"
#include "resample_taps.h"
#include "truepeak_taps.h"

namespace kx {

// ---- the format word and the resampler's tables ------------------------------------------------------------------------------
void check_format_word(int word) {
    const int form = format_form(word);
    KX_REQUIRE(word >= 0 && (word & ~0xFFF) == 0 && (form <= 4 || form == 8 || form == 9 || form == FORM_FLAC || form == FORM_ADPCM_WAV || form == FORM_WAV16),
               "infer: unknown output format");
    KX_REQUIRE(format_rate(word) <= 3, "infer: unknown output sample rate");
}

namespace {
// (the tables are committed as bit patterns: what the library computes with is what the generator rounded)
const uint32_t kBits8000[KX_RESAMPLE_NTAPS_8000] = {KX_RESAMPLE_TAPS_8000};
const uint32_t kBits16000[KX_RESAMPLE_NTAPS_16000] = {KX_RESAMPLE_TAPS_16000};
const uint32_t kBits48000[KX_RESAMPLE_NTAPS_48000] = {KX_RESAMPLE_TAPS_48000};
struct FilterTables {
    float taps[3][KX_RESAMPLE_NTAPS_8000];
    ResampleFilter f[3];
    FilterTables() {
        static_assert(sizeof(float) == 4 && KX_RESAMPLE_NTAPS_16000 <= KX_RESAMPLE_NTAPS_8000 && KX_RESAMPLE_NTAPS_48000 <= KX_RESAMPLE_NTAPS_8000,
                      "float32 bit patterns, the 8000 Hz table the longest");
        std::memcpy(taps[0], kBits8000, sizeof kBits8000);
        std::memcpy(taps[1], kBits16000, sizeof kBits16000);
        std::memcpy(taps[2], kBits48000, sizeof kBits48000);
        f[0] = ResampleFilter{1, 3, 72, KX_RESAMPLE_NTAPS_8000, taps[0]};
        f[1] = ResampleFilter{2, 3, 72, KX_RESAMPLE_NTAPS_16000, taps[1]};
        f[2] = ResampleFilter{2, 1, 48, KX_RESAMPLE_NTAPS_48000, taps[2]};
    }
};
}  // namespace

const ResampleFilter& resample_filter(int rate_code) {
    KX_REQUIRE(rate_code >= 1 && rate_code <= 3, "infer: unknown output sample rate");
    static const FilterTables tables;
    return tables.f[rate_code - 1];
}

long resampled_samples(int rate_code, long n_samples) {
    if (rate_code == 0) return n_samples;
    const ResampleFilter& f = resample_filter(rate_code);
    return n_samples * f.L / f.M;
}

// ---- pieces (include/kokorox_hip.h, "pieces") ---------------------------------------------------------------------------------------
static_assert(PIECE_TAIL >= piece_tail_need(1, 3, KX_RESAMPLE_NTAPS_8000) && PIECE_TAIL >= piece_tail_need(2, 3, KX_RESAMPLE_NTAPS_16000) &&
                  PIECE_TAIL >= piece_tail_need(2, 1, KX_RESAMPLE_NTAPS_48000),
              "a carry holds every source sample an output still to come reads");

static_assert(KX_RESAMPLE_NTAPS_8000 == 2 * 72 + 1 && KX_RESAMPLE_NTAPS_16000 == 2 * 72 + 1 && KX_RESAMPLE_NTAPS_48000 == 2 * 48 + 1,
              "piece_emitted has the three filters' C written out");

void check_piece_call(const HostCall& hc) {
    if (!hc.piece_call) return;  // (an entry without pieces; the dispatcher's pieces were checked when they were submitted)
    KX_REQUIRE(hc.piece_flags && hc.carry_out, "infer: null piece argument");
    KX_REQUIRE(hc.grouped(), "infer: pieces are for requests (chunks_per_request)");
    const char* refusal = piece_refusal(hc.layout(0));
    KX_REQUIRE(!refusal, refusal);
}

// ---- the true-peak meter's table (include/kokorox_hip.h, "levels") ---------------------------------------------------------------
const float* truepeak_taps() {
    static_assert(KX_TRUEPEAK_PHASES == TRUEPEAK_PHASES && KX_TRUEPEAK_NTAPS == TRUEPEAK_NTAPS, "the committed table is [3][24]");
    static const uint32_t kBits[TRUEPEAK_PHASES * TRUEPEAK_NTAPS] = {KX_TRUEPEAK_TAPS_1, KX_TRUEPEAK_TAPS_2, KX_TRUEPEAK_TAPS_3};
    static const struct Table {
        float taps[TRUEPEAK_PHASES * TRUEPEAK_NTAPS];
        Table() { std::memcpy(taps, kBits, sizeof taps); }
    } table;
    return table.taps;
}

// ---- the limiter's weights (include/kokorox_hip.h, "limiter") ---------------------------------------------------------------------
const float* limit_taps(int rate_code) {
    KX_REQUIRE(rate_code >= 0 && rate_code <= 3, "infer: unknown output sample rate");
    static_assert(KX_LIMIT_MAX_NTAPS == LIMIT_MAX_TAPS && KX_LIMIT_NTAPS_48000 == LIMIT_MAX_TAPS && KX_LIMIT_W_24000 == limit_window(0) &&
                      KX_LIMIT_W_8000 == limit_window(1) && KX_LIMIT_W_16000 == limit_window(2) && KX_LIMIT_W_48000 == limit_window(3),
                  "the committed tables are those of W = fs / 200");
    // (committed as bit patterns, rate codes 0..3: what the library computes with is what the generator rounded)
    static const uint32_t kBits24000[KX_LIMIT_NTAPS_24000] = {KX_LIMIT_TAPS_24000};
    static const uint32_t kBits8000[KX_LIMIT_NTAPS_8000] = {KX_LIMIT_TAPS_8000};
    static const uint32_t kBits16000[KX_LIMIT_NTAPS_16000] = {KX_LIMIT_TAPS_16000};
    static const uint32_t kBits48000[KX_LIMIT_NTAPS_48000] = {KX_LIMIT_TAPS_48000};
    static const struct Table {
        float taps[4][LIMIT_MAX_TAPS];
        Table() {
            std::memset(taps, 0, sizeof taps);
            std::memcpy(taps[0], kBits24000, sizeof kBits24000);
            std::memcpy(taps[1], kBits8000, sizeof kBits8000);
            std::memcpy(taps[2], kBits16000, sizeof kBits16000);
            std::memcpy(taps[3], kBits48000, sizeof kBits48000);
        }
    } table;
    return table.taps[rate_code];
}

// ---- refusals of the host entry (Model::infer_host_once) ---------------------------------------------------------------------
void check_host_call(const int64_t* ids, int64_t t_stride, const int32_t* lens, int B, const float* speeds, const HostCall& hc,
                     void** out, const int64_t* out_bytes, const int64_t* out_samples, int n_vocab, int n_voices,
                     bool have_voice_table) {
    KX_REQUIRE(out && out_bytes && out_samples, "infer: null output argument");
    *out = nullptr;
    KX_REQUIRE(B >= 1, "infer: empty batch");
    KX_REQUIRE(ids && lens && speeds, "infer: null argument");
    const bool grouped = hc.grouped();  // (then `format` is not used)
    KX_REQUIRE(grouped || (hc.format >= 0 && hc.format <= 2), "infer: unknown output format");
    if (grouped) {
        const int R = hc.n_requests;
        KX_REQUIRE(R >= 1 && hc.req_formats && (hc.n_req_formats == 1 || hc.n_req_formats == R), "infer: requests need 1 or R output formats");
        long rows = 0;
        for (int r = 0; r < R; ++r) {
            KX_REQUIRE(hc.chunks_per_request[r] >= 1, "infer: chunks_per_request entries must be >= 1 and add up to the batch");
            rows += hc.chunks_per_request[r];
        }
        KX_REQUIRE(rows == B, "infer: chunks_per_request entries must be >= 1 and add up to the batch");
        for (int i = 0; i < hc.n_req_formats; ++i) check_format_word(hc.req_formats[i]);
    }
    KX_REQUIRE(!hc.utt_index || hc.utt_seeds, "infer: utterance indices go with per-row seeds");
    const bool by_voice = hc.by_voice();
    KX_REQUIRE(by_voice || hc.styles, "infer: styles or voice ids are required");
    KX_REQUIRE(!hc.kinds || (by_voice && hc.styles), "infer: per-utterance kinds need both styles and voice ids");
    if (by_voice) {
        KX_REQUIRE(have_voice_table && hc.weights && hc.max_mix >= 1 && hc.max_mix <= 16, "infer: voice table not set or bad mix");
    }
    for (int b = 0; b < B; ++b) {
        KX_REQUIRE(lens[b] >= 1 && lens[b] <= 512 && lens[b] <= t_stride, "infer: token count must be 1..512");
        for (int t = 0; t < lens[b]; ++t) {
            const int64_t id = ids[b * t_stride + t];
            KX_REQUIRE(id >= 0 && id < n_vocab, "infer: token id outside 0..177");
        }
        const int kind = hc.kind_of(b);
        KX_REQUIRE(kind >= 0 && kind <= 2, "infer: unknown kind / output format");
        if (kind != 0) {
            KX_REQUIRE(lens[b] >= 2, "infer: voice rows need the two 0 pads (row = tokens - 2)");
            bool any = false;
            for (int k = 0; k < hc.max_mix; ++k) {
                const int v = hc.voice_ids[(size_t)b * hc.max_mix + k];
                KX_REQUIRE(v < n_voices, "infer: voice id outside the table");
                any = any || v >= 0;
            }
            KX_REQUIRE(any && (kind != 1 || hc.voice_ids[(size_t)b * hc.max_mix] >= 0), "infer: no voice given");
        }
    }
}

void check_marks_call(const HostCall& hc, int64_t** out_marks, int64_t* out_n_marks) {
    KX_REQUIRE(out_marks && out_n_marks, "infer: null marks argument");
    *out_marks = nullptr;
    KX_REQUIRE(hc.grouped(), "infer: marks are for requests (chunks_per_request)");
}

namespace {
// (the three texts of a list are written out whole below: callers and tests match on them)
template <class Spec>
void check_list(const HostCall& hc, const SpecList<Spec>& list, bool (*ok)(const Spec&), const char* null_list, const char* bad_count,
                const char* bad_spec) {
    KX_REQUIRE(list.specs, null_list);
    KX_REQUIRE(hc.grouped() && (list.n == 1 || list.n == hc.n_requests), bad_count);
    for (int i = 0; i < list.n; ++i) KX_REQUIRE(ok(list.specs[i]), bad_spec);
}
}  // namespace

void check_spec_list(const HostCall& hc, const SpecList<JoinSpec>& list) {
    check_list(hc, list, join_spec_ok, "infer: null join argument", "infer: bad join count", "infer: bad join");
}
void check_spec_list(const HostCall& hc, const SpecList<LevelSpec>& list) {
    check_list(hc, list, level_spec_ok, "infer: null level argument", "infer: bad level count", "infer: bad level");
}
void check_spec_list(const HostCall& hc, const SpecList<LoudSpec>& list) {
    check_list(hc, list, loud_spec_ok, "infer: null loudness argument", "infer: bad loudness count", "infer: bad loudness");
}
void check_spec_list(const HostCall& hc, const SpecList<LimitSpec>& list) {
    check_list(hc, list, limit_spec_ok, "infer: null limit argument", "infer: bad limit count", "infer: bad limit");
}

void check_prosody_call(const HostCall& hc, const int32_t* lens, int B, int64_t t_stride, float** out_report, int64_t* out_n_report) {
    KX_REQUIRE((out_report != nullptr) == (out_n_report != nullptr), "infer: null report argument");
    if (out_report) *out_report = nullptr;
    KX_REQUIRE(!hc.req_reports || (hc.grouped() && out_report), "infer: reports are for requests (chunks_per_request)");
    KX_REQUIRE(prosody_ok(hc.prosody, lens, B, t_stride), "infer: bad prosody");
}

void check_fit_call(const HostCall& hc, const int32_t* lens, int B, int64_t t_stride, FitPlan& plan) {
    if (!hc.fit_call) {  // (an entry without spans: nothing to check, nothing planned)
        plan.prefix.clear();
        plan.flat.clear();
        return;
    }
    const bool ok = fit_ok(hc.fit_spans, hc.n_fit_spans, hc.chunks_per_request, hc.n_requests, lens, B,
                           hc.prosody ? hc.prosody->frames : nullptr, t_stride, plan);
    if (!ok) {
        plan.prefix.clear();
        plan.flat.clear();
    }
    KX_REQUIRE(ok, "infer: bad fit");
}

// ---- the meter's tables (include/kokorox_hip.h, "loudness") ---------------------------------------------------------------------
namespace {
// (committed as bit patterns, rate codes 0..3: what the library computes with is what the generator rounded)
const uint64_t kKweightBits[4][10] = {{KX_KWEIGHT_COEFS_24000}, {KX_KWEIGHT_COEFS_8000}, {KX_KWEIGHT_COEFS_16000}, {KX_KWEIGHT_COEFS_48000}};
struct LoudTables {
    double coefs[4][10];
    double powers[4][LOUD_POWERS][16];
    LoudTables() {
        static_assert(sizeof(double) == 8, "float64 bit patterns");
        std::memcpy(coefs, kKweightBits, sizeof coefs);
        for (int c = 0; c < 4; ++c) {
            // one step of the cascade with no input, over s = (v1, v2, w1, w2): v = -a1 v1 - a2 v2, w = c0 v + c1 v1 + c2 v2 - d1 w1 - d2 w2
            const double* k = coefs[c];
            const double a1 = k[3], a2 = k[4], c0 = k[5], c1 = k[6], c2 = k[7], d1 = k[8], d2 = k[9];
            // (the high-pass has a pole pair at radius 0.995 .. 0.97: entries of A^n reach a few hundred, and some 3000 products
            // in float64 would leave 1e-10 in them, which the scan would carry into every hop; the products run in long double --
            // 64 bits of mantissa where the host has them -- and each power is rounded to float64 once)
            typedef long double wide;
            const wide A[16] = {-(wide)a1, -(wide)a2, 0, 0, 1, 0, 0, 0, (wide)c1 - (wide)c0 * a1, (wide)c2 - (wide)c0 * a2, -(wide)d1, -(wide)d2, 0, 0, 1, 0};
            auto mul = [](const wide* x, const wide* y, wide* z) {  // z = x y
                for (int i = 0; i < 4; ++i)
                    for (int j = 0; j < 4; ++j) {
                        wide acc = 0;
                        for (int t = 0; t < 4; ++t) acc += x[4 * i + t] * y[4 * t + j];
                        z[4 * i + j] = acc;
                    }
            };
            wide step[16], cur[16], next[16];  // A^run, and its powers
            for (int i = 0; i < 16; ++i) step[i] = cur[i] = (i % 5 == 0) ? 1 : 0;
            for (int n = 0; n < loud_run(c); ++n) {
                mul(A, step, next);
                std::memcpy(step, next, sizeof step);
            }
            for (int p = 0; p < LOUD_POWERS; ++p) {
                for (int i = 0; i < 16; ++i) powers[c][p][i] = (double)cur[i];
                mul(step, cur, next);
                std::memcpy(cur, next, sizeof cur);
            }
        }
    }
};
const LoudTables& loud_tables() {
    static const LoudTables t;
    return t;
}
}  // namespace

const double* loud_coefs(int rate_code) {
    KX_REQUIRE(rate_code >= 0 && rate_code <= 3, "infer: unknown output sample rate");
    return loud_tables().coefs[rate_code];
}
const double* loud_powers() { return &loud_tables().powers[0][0][0]; }

// ---- refusals of the device entry (Model::infer_device) ----------------------------------------------------------------------
int check_device_call(const void* d_ids, int64_t t_stride, const int32_t* lens_host, int B, const void* d_styles,
                      const float* speeds_host, int n_speed) {
    KX_REQUIRE(B >= 1 && B <= 4096, "infer: batch must be 1..4096 (empty input is an error)");
    KX_REQUIRE(d_ids && lens_host && d_styles && speeds_host, "infer: null argument");
    KX_REQUIRE(n_speed == 1 || n_speed == B, "infer: n_speed must be 1 or B");
    int Tmax = 0;
    for (int b = 0; b < B; ++b) {
        KX_REQUIRE(lens_host[b] >= 1 && lens_host[b] <= 512, "infer: token count must be 1..512");
        KX_REQUIRE((int64_t)lens_host[b] <= t_stride, "infer: lens[b] exceeds the row stride");
        if (lens_host[b] > Tmax) Tmax = lens_host[b];
    }
    for (int i = 0; i < n_speed; ++i) KX_REQUIRE(speeds_host[i] > 0.f, "infer: speed must be > 0");
    return Tmax;
}

// ---- layout of the compact output ----------------------------------------------------------------------------------------------
OutputBounds output_bounds(const RequestLayout& lay, int B, size_t n_samples, const int32_t* lens) {
    if (lay.joins && lay.chunks_per_request)
        for (int r = 0; r < lay.R; ++r) {
            // (a piece that is not the last keeps the pause behind its final chunk)
            const int pauses = lay.chunks_per_request[r] - (lay.piece_flags && !(lay.piece_flags[r] & PIECE_LAST) ? 0 : 1);
            if (pauses > 0) n_samples += (size_t)24 * (size_t)lay.joins[lay.n_join == 1 ? 0 : r].pause_ms * (size_t)pauses;
        }
    // bytes per sample: 8 (stereo), 4 (f32, float WAV), 3 >= 8 / 3 (base64 of 16 bits), 2 (PCM16), 1 (G.711), twice that at 48 000 Hz
    // (the lower rates are counted as 24 000 Hz); per request: the 44-byte header, or its 60 base64 characters and the last
    // group's padding -- what a one-frame request needs beyond its samples.  Resampled floats per sample: every request at the
    // batch's highest ratio, 2 at 48 000 Hz, below 1 otherwise
    size_t per_sample = 0, y_per_sample = 0;
    bool flac = false, adpcm = false;
    for (int i = 0; i < lay.n_format; ++i) {
        const int f = format_form(lay.formats[i]), c = format_rate(lay.formats[i]);
        flac = flac || f == FORM_FLAC;
        adpcm = adpcm || f == FORM_ADPCM_WAV;
        // (ADPCM: A bytes for P = 2 A - 7 samples, below 1 byte a sample from A = 256 on; its last block is counted below)
        size_t w = f == 1 ? 8 : (f == 2 || f == FORM_FLAC || f == FORM_WAV16 ? 2 : (f == 4 ? 3 : (f >= 8 ? 1 : 4)));
        if (c == 3) w *= 2;
        const size_t y = c == 0 ? 0 : (c == 3 ? 2 : 1);
        per_sample = w > per_sample ? w : per_sample;
        y_per_sample = y > y_per_sample ? y : y_per_sample;
    }
    OutputBounds bound{n_samples * per_sample + (size_t)lay.R * 64 + 16, n_samples * y_per_sample, 0, 0, 0, 0, 0, 0};
    // (an ADPCM body beyond its samples: 60 header bytes and a last block padded to its full size, at most 1024 bytes)
    if (adpcm) bound.packed_bytes += (size_t)lay.R * (size_t)(ADPCM_HEADER + ADPCM_MAX_BLOCK);
    if (flac) {  // (a FLAC body beyond its samples: 52 <= 64 bytes a request, counted above, and 16 a frame; the lengths block)
        bound.flac_slots = n_samples * (y_per_sample > 1 ? y_per_sample : 1) / (size_t)FLAC_BLOCK + (size_t)lay.R;
        bound.packed_bytes += 16 * bound.flac_slots + 8 + 8 * (size_t)lay.R;
    }
    // (a layout whose limit specs are all LIMIT_NONE has no limiter: its bounds are those of the layout without them)
    bool limited = false;
    for (int i = 0; lay.limits && i < lay.n_limit; ++i) limited = limited || lay.limits[i].mode != LIMIT_NONE;
    if (lay.marks) {
        KX_REQUIRE(lens, "infer: marks need the token counts");
        bound.packed_bytes += 8;
        for (int b = 0; b < B; ++b) bound.packed_bytes += 8 * ((size_t)lens[b] + 1);
    }
    if (lay.loudness || limited) {  // (a hop is 2400 samples at 24 000 Hz, whatever the output rate)
        bound.packed_bytes += 16 * (size_t)lay.R;
        bound.hop_doubles = (size_t)lay.R * (n_samples / 2400 + 1);
    }
    if (lay.levels || lay.loudness || limited) {  // (no request is longer than all the samples at the batch's highest ratio)
        bound.packed_bytes += 8 + 16 * (size_t)lay.R;
        const size_t longest = n_samples * (y_per_sample > 1 ? y_per_sample : 1);
        bound.peak_dwords = (size_t)lay.R * ((longest + (size_t)LEVEL_WINDOW - 1) / (size_t)LEVEL_WINDOW + 1);
        // the second table, when some request's governing spec asks for the true peak (a metered request's level spec is the plain one)
        bool flagged = false;
        for (int i = 0; lay.levels && i < lay.n_level; ++i) flagged = flagged || (lay.levels[i].mode & PEAK_TRUE) != 0;
        for (int i = 0; lay.loudness && i < lay.n_loudness; ++i)
            flagged = flagged || (lay.loudness[i].mode != LOUD_NONE && (lay.loudness[i].mode & PEAK_TRUE) != 0);
        for (int i = 0; limited && i < lay.n_limit; ++i)
            flagged = flagged || (lay.limits[i].mode != LIMIT_NONE && (lay.limits[i].mode & PEAK_TRUE) != 0);
        if (flagged) bound.truepeak_dwords = bound.peak_dwords;
        if (limited) {  // (the fifth block; every request limited, at the batch's highest ratio)
            bound.packed_bytes += 40 * (size_t)lay.R;
            bound.lim_floats = longest;
            bound.limit_dwords = bound.peak_dwords;
        }
    }
    if (lay.piece_flags) {
        // (a piece also emits what the pieces before it held back: fewer than C / M + 4 <= 52 outputs, 8 bytes each at the most;
        // then the alignment gap and the carry block)
        bound.packed_bytes += (size_t)lay.R * 512;
        if (y_per_sample > 0) bound.y_floats += (size_t)lay.R * 64;
        bound.packed_bytes += 8 + (size_t)lay.R * sizeof(PieceCarry);
    }
    if (lay.reports) {  // (the alignment gap and a block in which every request wants the report)
        KX_REQUIRE(lens, "infer: reports need the token counts");
        bound.packed_bytes += 8;
        for (int b = 0; b < B; ++b) bound.packed_bytes += 16 * (size_t)lens[b];
    }
    return bound;
}

long pack_request_bytes(int form, long n_samples) {
    check_format_word(form);
    const long n = resampled_samples(format_rate(form), n_samples);  // samples at the output rate
    switch (format_form(form)) {
        case 0: return 4 * n;
        case 1: return 8 * n;
        case 2: return 2 * n;
        case 3: return 44 + 4 * n;
        case 4:
            KX_REQUIRE(36 + 2 * n <= 0xFFFFFFFFL, "pack: a 16-bit WAV file cannot hold that many samples (size field of 32 bits)");
            return 4 * ((44 + 2 * n + 2) / 3);
        case FORM_FLAC: return flac_bound(n);  // (the region; the body's true size is the device's to say)
        case FORM_ADPCM_WAV: {
            // (both size fields of 32 bits: the RIFF size 52 + A F, and N itself in the fact chunk, which is the first to overflow)
            const long A = adpcm_block_bytes(format_rate(form));
            KX_REQUIRE(n <= 0xFFFFFFFFL && 52 + A * adpcm_blocks(n, A) <= 0xFFFFFFFFL,
                       "pack: an ADPCM WAV file cannot hold that many samples (size field of 32 bits)");
            return ADPCM_HEADER + A * adpcm_blocks(n, A);
        }
        case FORM_WAV16:
            KX_REQUIRE(36 + 2 * n <= 0xFFFFFFFFL, "pack: a 16-bit WAV file cannot hold that many samples (size field of 32 bits)");
            return (44 + 2 * n + 3) & ~3L;
        default: return n;  // 8, 9: one G.711 byte per sample
    }
}

long adpcm_block_bytes(int rate_code) {
    static const long bytes[4] = {KX_ADPCM_BLOCK_BYTES};
    KX_REQUIRE(rate_code >= 0 && rate_code <= 3, "infer: unknown output sample rate");
    return bytes[rate_code];
}
const int* adpcm_steps() {
    static const int steps[KX_ADPCM_NSTEPS] = {KX_ADPCM_STEPS};
    return steps;
}

long flac_bound(long n_samples) { return (49 + 16 * flac_frames(n_samples) + 2 * n_samples + 3) & ~3L; }

long close_flac_gaps(char* host, const OutputPlan& plan, const int64_t* lengths, int64_t* out_bytes) {
    KX_REQUIRE(out_bytes && (!plan.has_flac() || (host && lengths)), "flac: bad argument");
    long at = 0;
    for (size_t r = 0; r < plan.req.size(); ++r) {
        const PackReq& q = plan.req[r];
        long len = q.out_bytes;
        if (plan.has_flac()) {
            len = lengths[r];
            const bool flac = plan.flac[r].frames >= 0;
            KX_REQUIRE(len >= 0 && (len & 3) == 0 && len <= q.out_bytes && (flac || len == q.out_bytes), "flac: bad length");
            if (at != q.out_off && len > 0) std::memmove(host + at, host + q.out_off, (size_t)len);
        }
        out_bytes[r] = len;
        at += len;
    }
    return at;
}

long report_rows(const RequestLayout& lay, const int32_t* lens, int B, std::vector<long>& rep_first, std::vector<long>* rep_count) {
    KX_REQUIRE(lay.reports && lens && B >= 1 && lay.R >= 1, "plan: bad argument");
    rep_first.assign((size_t)B, -1);
    if (rep_count) rep_count->assign((size_t)lay.R, 0);
    long tokens = 0;
    int row = 0;
    for (int r = 0; r < lay.R; ++r) {
        const int n = lay.chunks_per_request ? lay.chunks_per_request[r] : 1;
        KX_REQUIRE(n >= 1 && n <= B - row, "infer: chunks_per_request entries must be >= 1 and add up to the batch");
        for (int b = row; b < row + n && lay.reports[r]; ++b) {
            KX_REQUIRE(lens[b] >= 1 && lens[b] <= 512, "infer: token count must be 1..512");
            rep_first[(size_t)b] = tokens;
            tokens += lens[b];
            if (rep_count) (*rep_count)[(size_t)r] += lens[b];
        }
        row += n;
    }
    return tokens;
}

void build_output_plan(const int* frames, const int* lens, const int* edges, int B, const RequestLayout& lay, OutputPlan& plan) {
    const int R = lay.R;
    KX_REQUIRE(frames && lay.formats && B >= 1 && R >= 1 && (lay.n_format == 1 || lay.n_format == R) &&
                   (!lay.joins || (edges && (lay.n_join == 1 || lay.n_join == R))) && (lens || (!lay.marks && !lay.joins && !lay.reports)) &&
                   (!lay.levels || lay.n_level == 1 || lay.n_level == R) && (!lay.loudness || lay.n_loudness == 1 || lay.n_loudness == R) &&
                   (!lay.limits || lay.n_limit == 1 || lay.n_limit == R),
               "plan: bad argument");
    auto rows_of = [&](int r) { return lay.chunks_per_request ? lay.chunks_per_request[r] : 1; };
    // (a request run in pieces: its head rules only in its first piece, its tail rules only in its last; PIECE_WHOLE where none is given)
    const char* refusal = piece_refusal(lay);
    KX_REQUIRE(!refusal, refusal);
    auto flags_of = [&](int r) { return lay.piece_flags ? lay.piece_flags[r] : PIECE_WHOLE; };
    // the rows: what each contributes to its request's stream, and the prefix over it.  (A pass of its own: the refusals of the
    // rows speak before those of the request table below, whichever request they are in, and callers match on the text.)
    const JoinSpec as_it_is{};
    plan.join.assign((size_t)B, JoinRow{});
    plan.joined = false;
    plan.cum.assign((size_t)B + 1, 0);
    int row = 0;
    for (int r = 0; r < R; ++r) {
        const int n = rows_of(r);
        KX_REQUIRE(n >= 1 && n <= B - row, "infer: chunks_per_request entries must be >= 1 and add up to the batch");
        const JoinSpec& js = lay.joins ? lay.joins[lay.n_join == 1 ? 0 : r] : as_it_is;
        KX_REQUIRE(join_spec_ok(js), "infer: bad join");
        plan.joined = plan.joined || !join_spec_plain(js);
        const long k = 24L * js.keep_ms, fade = 24L * js.fade_ms;
        for (int b = row; b < row + n; ++b) {
            KX_REQUIRE(frames[b] >= 0 && (!lay.joins || (edges[2 * b] >= 0 && edges[2 * b + 1] >= 0)), "pack: negative frame count");
            const bool first = b == row && (flags_of(r) & PIECE_FIRST) != 0, last = b == row + n - 1 && (flags_of(r) & PIECE_LAST) != 0;
            const bool long_enough = js.flags != 0 && lens[b] >= 3;  // (shorter rows are pads only)
            const bool head = long_enough && (js.flags & (first ? JOIN_TRIM_HEAD : JOIN_TRIM_INNER)) != 0;
            const bool tail = long_enough && (js.flags & (last ? JOIN_TRIM_TAIL : JOIN_TRIM_INNER)) != 0;
            JoinRow& j = plan.join[(size_t)b];
            const long lead = head ? 600L * edges[2 * b] - k : 0, trail = tail ? 600L * edges[2 * b + 1] - k : 0;
            j.skip = lead > 0 ? lead : 0;
            const long cut = trail > 0 ? trail : 0;
            j.keep = 600L * frames[b] - j.skip - cut;
            j.gap = last ? 0 : 24L * js.pause_ms;
            j.fade_head = head ? (int)fade : 0;
            j.fade_tail = tail ? (int)fade : 0;
            // (the middle tokens of a trimmed row have at least one frame each: 600 samples, more than the two fades' 576)
            KX_REQUIRE(j.keep >= 0 && j.keep >= (long)j.fade_head + j.fade_tail, "join: a row's edge durations exceed its frames");
            plan.cum[(size_t)b + 1] = plan.cum[(size_t)b] + j.keep + j.gap;
        }
        row += n;
    }
    KX_REQUIRE(row == B, "infer: chunks_per_request entries must be >= 1 and add up to the batch");
    // the requests: the table of the packer and the resampler over that prefix, and the rows' marks behind the bodies
    plan.req.assign((size_t)R, PackReq{});
    plan.total_bytes = plan.max_units = plan.y_floats = plan.max_resampled = plan.adpcm_groups = 0;
    plan.mark.assign(lens ? (size_t)B : 0, MarkRow{-1, 0, 0});
    plan.count.assign((size_t)R, 0);
    plan.first.assign((size_t)R, 0);
    plan.n_marks = 0;
    // (a layout whose flags are all PIECE_WHOLE has no piece: its plan is that of the layout without them)
    bool pieces = false;
    for (int r = 0; r < R; ++r) pieces = pieces || flags_of(r) != PIECE_WHOLE;
    plan.piece.assign(pieces ? (size_t)R : 0, PieceRow{});
    plan.tail_in.clear();
    plan.carry_off = 0;
    row = 0;
    for (int r = 0; r < R; ++r) {
        const int n = rows_of(r);
        PackReq& q = plan.req[(size_t)r];
        q.first_row = row;
        q.n_rows = n;
        const int word = lay.formats[lay.n_format == 1 ? 0 : r];
        check_format_word(word);
        q.form = format_form(word);
        q.rate = format_rate(word);
        q.src_samples = plan.cum[(size_t)(row + n)] - plan.cum[(size_t)row];
        q.n_samples = resampled_samples(q.rate, q.src_samples);
        const bool piece = flags_of(r) != PIECE_WHOLE;
        long src_before = 0;  // A_{k-1}: the marks of a later piece start from it
        if (pieces) {
            PieceRow& pr = plan.piece[(size_t)r];
            pr = PieceRow{0, q.n_samples, 0, q.src_samples, 0, 0, 0, 0, flags_of(r), (uint32_t)word, n, 0};
            if (piece) {
                if (!(pr.flags & PIECE_FIRST)) {
                    const PieceCarry& c = lay.carry_in[r];
                    pr.src_before = src_before = (long)c.src_samples;
                    pr.emit_lo = (long)c.out_samples;
                    pr.n_tail_in = c.n_tail;
                    pr.chunks_end = c.reserved + n;
                    pr.tail_in = (long)plan.tail_in.size();
                    plan.tail_in.insert(plan.tail_in.end(), c.tail, c.tail + c.n_tail);
                }
                pr.src_end = pr.src_before + q.src_samples;
                pr.emit_hi = piece_emitted(q.rate, pr.src_end, (pr.flags & PIECE_LAST) != 0);
                pr.n_tail_out = q.rate == 0 ? 0 : (int)(pr.src_end < PIECE_TAIL ? pr.src_end : PIECE_TAIL);
                KX_REQUIRE(pr.emit_hi >= pr.emit_lo, "infer: bad piece carry");
                q.n_samples = pr.emit_hi - pr.emit_lo;
            }
        }
        q.y_off = 0;
        if (q.rate) {
            q.y_off = plan.y_floats;
            plan.y_floats += q.n_samples;
            plan.max_resampled = q.n_samples > plan.max_resampled ? q.n_samples : plan.max_resampled;
        }
        q.out_off = plan.total_bytes;
        q.out_bytes = pack_request_bytes(word, q.src_samples);
        if (piece) {  // (its samples in the form, behind the header only in a first piece: a later piece of a float WAV is bare floats)
            const bool bare = q.form == 3 && !(flags_of(r) & PIECE_FIRST);
            if (bare) q.form = 0;
            q.out_bytes = (q.form == 3 ? 44 : 0) + (q.form == 1 ? 8 : (q.form == 2 ? 2 : (q.form >= 8 ? 1 : 4))) * q.n_samples;
        }
        plan.total_bytes += q.out_bytes;
        // (the packer writes no FLAC region and no ADPCM region)
        const long units = q.form == FORM_FLAC || q.form == FORM_ADPCM_WAV ? 0 : ((q.out_off & 15) + q.out_bytes + 15) / 16;
        if (q.form == FORM_ADPCM_WAV) {  // (the workgroup of block 0 writes the header: one group even where there is no block)
            const long A = adpcm_block_bytes(q.rate), per_group = ADPCM_GROUP_BYTES / A;
            const long groups = (adpcm_blocks(q.n_samples, A) + per_group - 1) / per_group;
            const long wanted = groups > 1 ? groups : 1;
            plan.adpcm_groups = wanted > plan.adpcm_groups ? wanted : plan.adpcm_groups;
        }
        plan.max_units = units > plan.max_units ? units : plan.max_units;
        plan.first[(size_t)r] = plan.n_marks;
        if (lens) {
            const long K = frame_samples(q.rate);
            for (int b = row; b < row + n; ++b) {
                KX_REQUIRE(lens[b] >= 1 && lens[b] <= 512, "infer: token count must be 1..512");
                MarkRow& m = plan.mark[(size_t)b];
                m.K = K;
                m.src_base = src_before + plan.cum[(size_t)b] - plan.cum[(size_t)row];
                m.base = m.src_base * K / 600;  // (exact: cum counts multiples of 24 samples)
                m.skip = plan.join[(size_t)b].skip;
                m.keep = plan.join[(size_t)b].keep;
                if (lay.marks && lay.marks[r]) {
                    m.first = plan.n_marks;
                    plan.n_marks += lens[b] + 1;
                }
            }
        }
        plan.count[(size_t)r] = plan.n_marks - plan.first[(size_t)r];
        row += n;
    }
    plan.marks_off = (plan.total_bytes + 7) & ~7L;
    // the levels: every request's spec, the block behind the marks and the grid of the peak pass
    // (a layout whose limit specs are all LIMIT_NONE has no limiter: its plan is that of the layout without them)
    plan.limit_spec.clear();
    plan.limit.clear();
    plan.limited = false;
    plan.lim_floats = plan.limits_off = 0;
    for (int r = 0; lay.limits && r < R; ++r) {
        const LimitSpec& ms = lay.limits[lay.n_limit == 1 ? 0 : r];
        KX_REQUIRE(ms.mode == LIMIT_NONE || limit_spec_ok(ms), "infer: bad limit");
        plan.limited = plan.limited || ms.mode != LIMIT_NONE;
    }
    plan.level.clear();
    plan.measured = lay.levels != nullptr || lay.loudness != nullptr || plan.limited;
    plan.levelled = plan.true_peak = false;
    plan.levels_off = plan.peak_windows = 0;
    const LevelSpec plain_level{LEVEL_GAIN, 1.0f, 0.0f};
    if (plan.measured) {
        plan.level.resize((size_t)R);
        long longest = 0;
        for (int r = 0; r < R; ++r) {
            const LevelSpec& ls = lay.levels ? lay.levels[lay.n_level == 1 ? 0 : r] : plain_level;
            KX_REQUIRE(level_spec_ok(ls), "infer: bad level");
            plan.level[(size_t)r] = ls;
            plan.levelled = plan.levelled || !level_spec_plain(ls);
            plan.true_peak = plan.true_peak || (ls.mode & PEAK_TRUE) != 0;
            longest = plan.req[(size_t)r].n_samples > longest ? plan.req[(size_t)r].n_samples : longest;
        }
        plan.levels_off = (plan.marks_off + 8 * plan.n_marks + 7) & ~7L;
        plan.peak_windows = (longest + LEVEL_WINDOW - 1) / LEVEL_WINDOW;
    }
    // the loudness: every request's spec, the block behind the levels and the grid of the meter.  A metered request's {p, g} are the
    // loudness gain kernel's: its level spec is the plain one.
    plan.loud.clear();
    plan.loud_all = false;
    plan.loud_off = plan.max_hops = 0;
    // A limited request is driven through the same two kernels: its derived spec is the ceiling rule 12 dB up (4 peak is exact),
    // LEVEL_CEILING with its gain in mode 0 and LOUD_NORMALIZE with its target in mode 1, the flag carried over.
    const LoudSpec no_loud{LOUD_NONE, 0.0f, 0.0f};
    if (plan.limited) {
        plan.limit_spec.resize((size_t)R);
        plan.limit.resize((size_t)R);
        plan.levelled = true;  // (the limited packer stages through the join table and scales the requests beside the limited ones)
    }
    if (lay.loudness || plan.limited) {
        plan.loud.resize((size_t)R);
        plan.loud_all = true;
        for (int r = 0; r < R; ++r) {
            LoudSpec ls = lay.loudness ? lay.loudness[lay.n_loudness == 1 ? 0 : r] : no_loud;
            KX_REQUIRE(ls.mode == LOUD_NONE || loud_spec_ok(ls), "infer: bad loudness");
            if (plan.limited) {
                const LimitSpec& ms = lay.limits[lay.n_limit == 1 ? 0 : r];
                plan.limit_spec[(size_t)r] = ms;
                plan.limit[(size_t)r] = LimitRow{-1, 0.0f, LIMIT_NONE};
                if (ms.mode != LIMIT_NONE) {
                    KX_REQUIRE(ls.mode == LOUD_NONE && level_spec_plain(plan.level[(size_t)r]), "plan: a request has a level, a loudness or a limit, not two of them");
                    const uint32_t flag = ms.mode & PEAK_TRUE;
                    if ((ms.mode & ~PEAK_TRUE) == LIMIT_LOUDNESS) {
                        ls = LoudSpec{LOUD_NORMALIZE | flag, ms.target_lufs, LIMIT_DRIVE_CAP * ms.peak};
                    } else {
                        plan.level[(size_t)r] = LevelSpec{LEVEL_CEILING | flag, ms.gain, LIMIT_DRIVE_CAP * ms.peak};
                        plan.true_peak = plan.true_peak || flag != 0;
                    }
                    plan.limit[(size_t)r] = LimitRow{plan.lim_floats, ms.peak, ms.mode};
                    plan.lim_floats += plan.req[(size_t)r].n_samples;
                }
            }
            plan.loud[(size_t)r] = ls;
            if (ls.mode == LOUD_NONE) {
                plan.loud_all = false;
                continue;
            }
            KX_REQUIRE(level_spec_plain(plan.level[(size_t)r]), "plan: a request has a level or a loudness, not both");
            plan.levelled = plan.levelled || (ls.mode & ~PEAK_TRUE) == LOUD_NORMALIZE;
            plan.true_peak = plan.true_peak || (ls.mode & PEAK_TRUE) != 0;
            const long hops = plan.req[(size_t)r].n_samples / loud_hop(plan.req[(size_t)r].rate);
            plan.max_hops = hops > plan.max_hops ? hops : plan.max_hops;
        }
        plan.loud_off = plan.levels_off + 16L * R;
        if (plan.limited) plan.limits_off = plan.loud_off + 16L * R;
    }
    // FLAC: the packer's table without those requests, the encoder's table, the slots and the lengths block behind everything else
    plan.pack_req.clear();
    plan.flac.clear();
    plan.flac_slots = plan.flac_max_frames = plan.flac_max_bytes = plan.flac_off = 0;
    bool flac = false;
    for (int r = 0; r < R; ++r) flac = flac || plan.req[(size_t)r].form == FORM_FLAC;
    if (flac) {
        plan.pack_req = plan.req;
        plan.flac.resize((size_t)R);
        for (int r = 0; r < R; ++r) {
            const PackReq& q = plan.req[(size_t)r];
            FlacRow& f = plan.flac[(size_t)r];
            f = FlacRow{q.out_off, q.out_bytes, q.n_samples, -1, plan.flac_slots, q.rate};
            if (q.form != FORM_FLAC) continue;
            plan.pack_req[(size_t)r].out_off = plan.pack_req[(size_t)r].out_bytes = 0;
            f.frames = flac_frames(q.n_samples);
            plan.flac_slots += f.frames;
            plan.flac_max_frames = f.frames > plan.flac_max_frames ? f.frames : plan.flac_max_frames;
            plan.flac_max_bytes = q.out_bytes > plan.flac_max_bytes ? q.out_bytes : plan.flac_max_bytes;
        }
        plan.flac_off = (plan.blocks_end() + 7) & ~7L;
    }
    // the prosody report: the tokens of the requests that want it, behind everything else
    plan.rep_first.clear();
    plan.rep_count.clear();
    plan.report_off = plan.n_report = 0;
    if (lay.reports) {
        plan.n_report = report_rows(lay, lens, B, plan.rep_first, &plan.rep_count);
        if (plan.n_report > 0) plan.report_off = (plan.fixed_end() + 7) & ~7L;
    }
    // the carries of a plan with pieces: one record per request, behind everything else
    if (pieces) {
        plan.carry_off = (plan.report_end() + 7) & ~7L;
        for (int r = 0; r < R; ++r) plan.piece[(size_t)r].carry_off = plan.carry_off + (long)sizeof(PieceCarry) * r;
    }
}

}  // namespace kx

