// Stand-alone check of the request plan with format WORDS (form | rate code << 8): region sizes and offsets for every form x
// rate, the packed bound of one-frame requests, the intermediate buffer of the resampled streams, the filter table's shape and
// the refusals with their messages.  Built with g++ -fsanitize=address,undefined together with kokorox_amd/csrc/host_request.cpp
// (tests/test_resample_cpu.py); every expected value is written out here on its own.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "host_request.h"

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

static const int FORMS[7] = {0, 1, 2, 3, 4, 8, 9};
static const int RATE_L[4] = {1, 1, 2, 2}, RATE_M[4] = {1, 3, 3, 1}, RATE_TAPS[4] = {0, 145, 145, 97};

static long out_samples(int rate, long S) { return S * RATE_L[rate] / RATE_M[rate]; }
static long region_bytes(int form, long n) {  // n = samples at the output rate
    switch (form) {
        case 0: return 4 * n;
        case 1: return 8 * n;
        case 2: return 2 * n;
        case 3: return 44 + 4 * n;
        case 4: return 4 * ((44 + 2 * n + 2) / 3);
        default: return n;  // 8, 9
    }
}

static bool refused(const std::function<void()>& call, const char* message) {
    try {
        call();
    } catch (const kx::Error& e) {
        return e.code == 1 && strcmp(e.what(), message) == 0;
    }
    return false;
}

static void filters() {
    for (int c = 1; c <= 3; ++c) {
        const kx::ResampleFilter& f = kx::resample_filter(c);
        const int Q = f.L > f.M ? f.L : f.M;
        CHECK(f.L == RATE_L[c] && f.M == RATE_M[c] && f.C == 24 * Q && f.n_taps == 2 * f.C + 1 && f.n_taps == RATE_TAPS[c]);
        double sum = 0;
        for (int i = 0; i < f.n_taps; ++i) {
            CHECK(f.taps[i] == f.taps[f.n_taps - 1 - i]);
            sum += f.taps[i];
        }
        CHECK(sum > f.L - 1e-5 && sum < f.L + 1e-5 && f.taps[f.C] > 0.3f);
        CHECK(kx::resampled_samples(c, 600) == 600 * f.L / f.M);
    }
    CHECK(kx::resampled_samples(0, 600) == 600);
    CHECK(refused([] { (void)kx::resample_filter(0); }, "infer: unknown output sample rate"));
    CHECK(refused([] { (void)kx::resample_filter(4); }, "infer: unknown output sample rate"));
    printf("filters: 145 145 97 taps\n");
}

// the bound of the bodies, written out: the widest word's bytes per sample (twice at 48 000 Hz), 64 per request, 16
static size_t body_bound(const std::vector<int>& words, int R, size_t n_samples) {
    size_t per_sample = 0;
    for (int word : words) {
        const int f = word & 255;
        const size_t w = (f == 1 ? 8 : (f == 2 ? 2 : (f == 4 ? 3 : (f >= 8 ? 1 : 4)))) * (size_t)((word >> 8) == 3 ? 2 : 1);
        per_sample = w > per_sample ? w : per_sample;
    }
    return n_samples * per_sample + (size_t)R * 64 + 16;
}

// one request per entry of `chunks` over rows of `frames` frames, request r in words[r]
static void check_plan(const std::vector<int>& frames, const std::vector<int>& chunks, const std::vector<int>& words) {
    const int B = (int)frames.size(), R = (int)chunks.size();
    kx::OutputPlan plan;
    plan.y_floats = 77;  // (stale contents must not survive)
    plan.max_resampled = 77;
    const kx::RequestLayout lay{chunks.data(), R, words.data(), (int)words.size(), nullptr, nullptr, 0};
    kx::build_output_plan(frames.data(), nullptr, nullptr, B, lay, plan);
    CHECK(plan.req.size() == (size_t)R);
    long off = 0, units = 0, y = 0, widest = 0, S_all = 0;
    int row = 0;
    for (int r = 0; r < R; ++r) {
        const kx::PackReq& q = plan.req[(size_t)r];
        const int word = words[words.size() == 1 ? 0 : (size_t)r], form = word & 255, rate = word >> 8;
        long S = 0;
        for (int i = 0; i < chunks[(size_t)r]; ++i) S += 600L * frames[(size_t)(row + i)];
        const long n = out_samples(rate, S);
        CHECK(q.first_row == row && q.n_rows == chunks[(size_t)r] && q.form == form && q.rate == rate);
        CHECK(q.src_samples == S && q.n_samples == n && n * RATE_M[rate] == S * RATE_L[rate]);
        CHECK(q.out_off == off && q.out_bytes == region_bytes(form, n) && q.out_bytes % 4 == 0);
        CHECK(q.out_bytes == kx::pack_request_bytes(word, S));
        if (rate) {
            CHECK(q.y_off == y);
            y += n;
            widest = n > widest ? n : widest;
        }
        const long u = ((off & 15) + q.out_bytes + 15) / 16;
        units = u > units ? u : units;
        off += q.out_bytes;
        row += chunks[(size_t)r];
        S_all += S;
    }
    CHECK(plan.total_bytes == off && plan.max_units == units && plan.y_floats == y && plan.max_resampled == widest);
    // what is sized before the frame counts are known holds the plan: the packed buffer and the resampled streams
    kx::HostCall hc;
    hc.chunks_per_request = chunks.data();
    hc.n_requests = R;
    hc.req_formats = words.data();
    hc.n_req_formats = (int)words.size();
    const kx::OutputBounds bound = kx::output_bounds(lay, B, (size_t)S_all, nullptr);
    const kx::OutputBounds same = kx::output_bounds(hc.layout(B), B, (size_t)S_all, nullptr);
    CHECK(same.packed_bytes == bound.packed_bytes && same.y_floats == bound.y_floats);
    CHECK(bound.packed_bytes == body_bound(words, R, (size_t)S_all) && (size_t)plan.total_bytes <= bound.packed_bytes);
    CHECK((size_t)plan.y_floats <= bound.y_floats);
}

static void plans() {
    int n = 0;
    // every form x rate, one request of 1, 2 and 3 frames (all three base64 paddings at the other rates)
    for (int rate = 0; rate < 4; ++rate)
        for (int form : FORMS)
            for (int fr = 1; fr <= 3; ++fr, ++n) {
                check_plan({fr}, {1}, {form | rate << 8});
                check_plan({fr, 1, fr}, {2, 1}, {form | rate << 8});
            }
    // the sizes themselves, written out: 600 samples -> 200 / 400 / 1200
    CHECK(kx::pack_request_bytes(8 | 0x100, 600) == 200 && kx::pack_request_bytes(9 | 0x200, 600) == 400);
    CHECK(kx::pack_request_bytes(2 | 0x300, 600) == 2400 && kx::pack_request_bytes(3 | 0x100, 1200) == 44 + 1600);
    CHECK(kx::pack_request_bytes(4 | 0x100, 600) == 4 * ((44 + 400 + 2) / 3) && (44 + 400) % 3 == 0);      // no '='
    CHECK(kx::pack_request_bytes(4 | 0x100, 1200) == 4 * ((44 + 800 + 2) / 3) && (44 + 800) % 3 == 1);     // "=="
    CHECK(kx::pack_request_bytes(4 | 0x100, 1800) == 4 * ((44 + 1200 + 2) / 3) && (44 + 1200) % 3 == 2);   // "="
    CHECK(kx::pack_request_bytes(8, 600) == 600 && kx::pack_request_bytes(0, 600) == 2400);
    // a batch that mixes rates and forms, rate 0 among them: the streams of the resampled requests lie back to back
    check_plan({1, 2, 3, 5, 1, 1}, {2, 1, 3}, {4 | 0x100, 0, 8 | 0x300});
    check_plan({1, 2, 3, 5, 1, 1}, {1, 1, 1, 1, 1, 1}, {0, 2 | 0x200, 3, 9 | 0x100, 1 | 0x300, 4});
    {
        const int frames[3] = {1, 2, 3}, words[3] = {4, 3, 2};
        kx::OutputPlan plan;
        const kx::RequestLayout lay{nullptr, 3, words, 3, nullptr, nullptr, 0};
        kx::build_output_plan(frames, nullptr, nullptr, 3, lay, plan);
        CHECK(plan.y_floats == 0 && plan.max_resampled == 0);  // nothing to resample: the resampler is not launched
        CHECK(kx::output_bounds(lay, 3, 3600, nullptr).y_floats == 0);
    }
    printf("plans: %d (rate, form, frames) triples\n", n);
}

static void bounds() {
    int n = 0;
    // one frame per request is where a per-sample estimate falls short
    for (int R = 1; R <= 64; R += 9)
        for (int rate = 0; rate < 4; ++rate)
            for (int form : FORMS) {
                check_plan(std::vector<int>((size_t)R, 1), std::vector<int>((size_t)R, 1), {form | rate << 8});
                ++n;
            }
    // form 4: the size field counts OUTPUT samples
    const long first_bad_out = (0xFFFFFFFFL - 36) / 2 + 1;  // output samples a 16-bit WAV file cannot hold
    CHECK(refused([&] { (void)kx::pack_request_bytes(4 | 0x300, first_bad_out / 2 + 600); },
                  "pack: a 16-bit WAV file cannot hold that many samples (size field of 32 bits)"));
    CHECK(kx::pack_request_bytes(4 | 0x300, 600 * ((first_bad_out / 2) / 600)) > 0);
    CHECK(kx::pack_request_bytes(4 | 0x100, first_bad_out + 600) > 0);  // a third of them at 8 kHz: fits
    printf("bounds: %d one-frame batches\n", n);
}

static void refusals() {
    const char* FORMAT = "infer: unknown output format";
    const char* RATE = "infer: unknown output sample rate";
    int n = 0;
    const int one = 1, frames = 1;
    kx::OutputPlan plan;
    auto all_refuse = [&](int word, const char* message) {
        CHECK(refused([&] { kx::check_format_word(word); }, message));
        CHECK(refused([&] { (void)kx::pack_request_bytes(word, 600); }, message));
        CHECK(refused([&] { kx::build_output_plan(&frames, nullptr, nullptr, 1, {&one, 1, &word, 1, nullptr, nullptr, 0}, plan); }, message));
        ++n;
    };
    for (int code = 4; code <= 15; ++code)
        for (int form : FORMS) all_refuse(form | code << 8, RATE);
    for (int rate = 0; rate < 4; ++rate)
        for (int form : {5, 6, 7, 10, 11, 16, 128, 255}) all_refuse(form | rate << 8, FORMAT);
    for (int word : {0x1000, 0x1100, 0x10000 | 8, 0x40000000, -1, -256, (int)0x80000100}) all_refuse(word, FORMAT);
    all_refuse(0x405, FORMAT);  // both wrong: the form speaks first
    for (int rate = 0; rate < 4; ++rate)
        for (int form : FORMS) kx::check_format_word(form | rate << 8);
    printf("refusals: %d words\n", n);
}

int main() {
    filters();
    plans();
    bounds();
    refusals();
    return 0;
}
