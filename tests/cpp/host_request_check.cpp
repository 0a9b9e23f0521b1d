// Driver for the argument checks and the output layout of the inference entries (kokorox_amd/csrc/host_request.cpp), built by
// tests/test_host_request_cpu.py with g++ -fsanitize=address,undefined.  No device, nothing loaded into python.
//   host_request_check refusals   one line per case: "<entry>.<case>\t<code>\t<message>" or "<entry>.<case>\taccepted"
//   host_request_check layout     the per-utterance calls' plans, request plans and the packed buffer's bound, checked here against
//                                 sums written out independently; prints what it covered, exits 1 at the first difference
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "host_request.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

static void report(const char* name, const std::function<void()>& call) {
    try {
        call();
        printf("%s\taccepted\n", name);
    } catch (const kx::Error& e) {
        printf("%s\t%d\t%s\n", name, e.code, e.what());
    }
}

// ---- a sound call of the host entry, and one change per case ---------------------------------------------------------------
struct HostArgs {
    static constexpr int N_VOCAB = 178, N_VOICES = 4;
    int B = 3;
    int64_t t_stride = 8;
    std::vector<int64_t> ids;
    std::vector<int32_t> lens{3, 8, 2};
    std::vector<float> speeds{1.f};
    std::vector<float> styles = std::vector<float>(3 * 256, 0.f);
    std::vector<int32_t> voice_ids, kinds, cpr, req_formats;
    std::vector<float> weights;
    std::vector<uint64_t> seeds{1, 2, 3};
    std::vector<uint32_t> index{0, 1, 2};
    kx::HostCall hc;
    bool have_table = true;
    void* result = reinterpret_cast<void*>(0x10);  // (must come back cleared)
    void** out = &result;
    std::vector<int64_t> bytes = std::vector<int64_t>(3), samples = std::vector<int64_t>(3);
    const int64_t* ids_p;
    const int32_t* lens_p;
    const float* speeds_p;
    int64_t *bytes_p, *samples_p;
    HostArgs() : ids(3 * 8, 1) {
        for (int b = 0; b < 3; ++b) ids[(size_t)b * 8] = ids[(size_t)b * 8 + (size_t)lens[(size_t)b] - 1] = 0;  // the two pads
        hc.styles = styles.data();
        ids_p = ids.data();
        lens_p = lens.data();
        speeds_p = speeds.data();
        bytes_p = bytes.data();
        samples_p = samples.data();
    }
    void voices(int max_mix, std::vector<int32_t> v) {  // by voice id instead of by style row
        voice_ids = std::move(v);
        weights.assign(voice_ids.size(), 1.f);
        hc.styles = nullptr;
        hc.voice_ids = voice_ids.data();
        hc.weights = weights.data();
        hc.max_mix = max_mix;
    }
    void grouped(std::vector<int32_t> chunks, std::vector<int32_t> forms) {
        cpr = std::move(chunks);
        req_formats = std::move(forms);
        hc.chunks_per_request = cpr.data();
        hc.n_requests = (int)cpr.size();
        hc.req_formats = req_formats.data();
        hc.n_req_formats = (int)req_formats.size();
    }
    void check() {
        kx::check_host_call(ids_p, t_stride, lens_p, B, speeds_p, hc, out, bytes_p, samples_p, N_VOCAB, N_VOICES, have_table);
        CHECK(result == nullptr);
    }
};

static void host_case(const char* name, const std::function<void(HostArgs&)>& change) {
    HostArgs a;
    change(a);
    report((std::string("host.") + name).c_str(), [&] { a.check(); });
    if (a.out && a.bytes_p && a.samples_p) CHECK(a.result == nullptr);  // (cleared whatever is refused after the output arguments)
}

struct DeviceArgs {
    int B = 3, n_speed = 1;
    int64_t t_stride = 8;
    std::vector<int32_t> lens{3, 8, 2};
    std::vector<float> speeds{1.f, 1.5f, 0.5f};
    int64_t ids[1] = {0};
    float styles[1] = {0.f};
    const void* d_ids = ids;  // (device pointers to the entry: only looked at for null)
    const void* d_styles = styles;
};

static void device_case(const char* name, const std::function<void(DeviceArgs&)>& change, int want_tmax = 0) {
    DeviceArgs a;
    change(a);
    report((std::string("device.") + name).c_str(), [&] {
        const int tmax = kx::check_device_call(a.d_ids, a.t_stride, a.lens.data(), a.B, a.d_styles, a.speeds.data(), a.n_speed);
        CHECK(tmax == want_tmax);
    });
}

static void refusals() {
    using A = HostArgs;
    host_case("null_out", [](A& a) { a.out = nullptr; });
    host_case("null_out_bytes", [](A& a) { a.bytes_p = nullptr; });
    host_case("null_out_samples", [](A& a) { a.samples_p = nullptr; });
    host_case("B_0", [](A& a) { a.B = 0; });
    host_case("null_ids", [](A& a) { a.ids_p = nullptr; });
    host_case("null_lens", [](A& a) { a.lens_p = nullptr; });
    host_case("null_speeds", [](A& a) { a.speeds_p = nullptr; });
    host_case("format_3_ungrouped", [](A& a) { a.hc.format = 3; });
    host_case("utt_index_without_seeds", [](A& a) { a.hc.utt_index = a.index.data(); });
    host_case("neither_styles_nor_voices", [](A& a) { a.hc.styles = nullptr; });
    host_case("kinds_with_styles_only", [](A& a) { a.kinds = {0, 0, 0}; a.hc.kinds = a.kinds.data(); });
    host_case("kinds_with_voices_only", [](A& a) { a.voices(1, {0, 1, 2}); a.kinds = {1, 1, 1}; a.hc.kinds = a.kinds.data(); });
    host_case("voices_without_table", [](A& a) { a.voices(1, {0, 1, 2}); a.have_table = false; });
    host_case("voices_without_weights", [](A& a) { a.voices(1, {0, 1, 2}); a.hc.weights = nullptr; });
    host_case("max_mix_0", [](A& a) { a.voices(0, {0, 1, 2}); });
    host_case("max_mix_17", [](A& a) { a.voices(17, std::vector<int32_t>(3 * 17, 0)); });
    host_case("lens_0", [](A& a) { a.lens[1] = 0; });
    host_case("lens_513", [](A& a) { a.t_stride = 600; a.ids.assign(3 * 600, 0); a.ids_p = a.ids.data(); a.lens[1] = 513; });
    host_case("lens_above_stride", [](A& a) { a.t_stride = 7; });
    host_case("id_minus_1", [](A& a) { a.ids[8 + 3] = -1; });
    host_case("id_n_vocab", [](A& a) { a.ids[2 * 8 + 1] = A::N_VOCAB; });
    host_case("kind_3", [](A& a) { a.voices(1, {0, 1, 2}); a.hc.styles = a.styles.data(); a.kinds = {0, 3, 1}; a.hc.kinds = a.kinds.data(); });
    host_case("voice_row_of_one_token", [](A& a) { a.voices(1, {0, 1, 2}); a.lens[2] = 1; });
    host_case("voice_id_n_voices", [](A& a) { a.voices(2, {0, 1, 2, A::N_VOICES, 3, -1}); });
    host_case("all_voice_ids_negative", [](A& a) { a.voices(2, {0, 1, -1, -1, 3, -1}); });
    host_case("kind_1_negative_first_id", [](A& a) {
        a.voices(2, {0, 1, -1, 2, 3, -1});
        a.hc.styles = a.styles.data();
        a.kinds = {2, 1, 1};
        a.hc.kinds = a.kinds.data();
    });
    // the (chunks_per_request, format) pairs of test_model_refuses_bad_groupings_and_formats, B = 3 rows
    host_case("grouped_1_2_format_5", [](A& a) { a.grouped({1, 2}, {5}); });
    host_case("grouped_1_2_formats_0_5", [](A& a) { a.grouped({1, 2}, {0, 5}); });
    host_case("grouped_1_2_format_minus_1", [](A& a) { a.grouped({1, 2}, {-1}); });
    host_case("grouped_1_0_2", [](A& a) { a.grouped({1, 0, 2}, {0}); });
    host_case("grouped_1_1", [](A& a) { a.grouped({1, 1}, {0}); });
    host_case("grouped_2_2", [](A& a) { a.grouped({2, 2}, {0}); });
    host_case("grouped_3_1", [](A& a) { a.grouped({3, 1}, {0}); });
    host_case("grouped_1_2_formats_0_1_2", [](A& a) { a.grouped({1, 2}, {0, 1, 2}); });
    // accepted: one call of each kind
    host_case("ok_style_rows", [](A&) {});
    host_case("ok_style_rows_seeds_and_index", [](A& a) { a.hc.utt_seeds = a.seeds.data(); a.hc.utt_index = a.index.data(); a.hc.format = 2; });
    host_case("ok_single_voice", [](A& a) { a.voices(1, {0, 3, 2}); });
    host_case("ok_mix", [](A& a) { a.voices(2, {0, 1, -1, 2, 3, -1}); });
    host_case("ok_per_utterance_kinds", [](A& a) {
        a.voices(2, {-1, -1, 1, -1, 3, 2});  // (row 0 is a style row: its voice ids are not looked at)
        a.hc.styles = a.styles.data();
        a.kinds = {0, 1, 2};
        a.hc.kinds = a.kinds.data();
    });
    host_case("ok_ungrouped_each_form", [](A& a) {
        for (int form = 0; form <= 2; ++form) {
            a.hc.format = form;
            a.result = reinterpret_cast<void*>(0x10);
            a.check();
        }
    });
    host_case("ok_grouped_shared_format", [](A& a) { a.grouped({1, 2}, {4}); a.hc.format = 9; /* (not used then) */ });
    host_case("ok_grouped_formats_per_request", [](A& a) { a.grouped({2, 1}, {3, 4}); });

    using D = DeviceArgs;
    device_case("B_0", [](D& a) { a.B = 0; });
    device_case("B_4097", [](D& a) { a.B = 4097; a.lens.assign(4097, 2); });
    device_case("null_ids", [](D& a) { a.d_ids = nullptr; });
    device_case("null_styles", [](D& a) { a.d_styles = nullptr; });
    device_case("n_speed_2_of_3", [](D& a) { a.n_speed = 2; });
    device_case("lens_0", [](D& a) { a.lens[0] = 0; });
    device_case("lens_513", [](D& a) { a.t_stride = 600; a.lens[2] = 513; });
    device_case("lens_above_stride", [](D& a) { a.t_stride = 7; });
    device_case("speed_0", [](D& a) { a.speeds[0] = 0.f; });
    device_case("speed_negative", [](D& a) { a.n_speed = 3; a.speeds[2] = -1.f; });
    device_case("ok_one_speed", [](D&) {}, 8);
    device_case("ok_speed_per_row", [](D& a) { a.n_speed = 3; a.lens = {3, 2, 5}; }, 5);
    device_case("ok_B_4096", [](D& a) { a.B = 4096; a.lens.assign(4096, 2); a.lens[4095] = 7; }, 7);
}

// ---- layout ---------------------------------------------------------------------------------------------------------------------
static long form_bytes(int form, long n) {  // include/kokorox_hip.h, KX_PACK_*
    switch (form) {
        case 0: return 4 * n;
        case 1: return 8 * n;
        case 2: return 2 * n;
        case 3: return 44 + 4 * n;
        default: return 4 * ((44 + 2 * n + 2) / 3);  // base64 of a 44-byte header and 16-bit samples
    }
}

// the bound of the bodies, written out: the widest word's bytes per sample (forms 0..4 at 24 000 Hz here), 64 per request, 16
static size_t body_bound(const int* words, int n_words, int R, size_t n_samples) {
    size_t per_sample = 0;
    for (int i = 0; i < n_words; ++i) {
        const size_t w = words[i] == 1 ? 8 : (words[i] == 2 ? 2 : (words[i] == 4 ? 3 : 4));
        per_sample = w > per_sample ? w : per_sample;
    }
    return n_samples * per_sample + (size_t)R * 64 + 16;
}

static void utterance_layout() {
    // what kx_infer / kx_infer_packed / kx_infer_voices ask of the plan builder: null chunks, one shared form 0..2, R = B
    const int B = 5;
    const int frames[B] = {1, 7, 422, 1, 3};
    static const int width[3] = {4, 8, 2};
    const int mixed[B] = {0, 1, 2, 2, 1};  // (as a grouped call of single-row requests: the dispatcher's mixed batches)
    const int ones[B] = {1, 1, 1, 1, 1};
    for (int c = 0; c < 4; ++c) {
        kx::OutputPlan plan;
        plan.total_bytes = 77;  // (stale contents must not survive)
        plan.max_units = 77;
        plan.req.resize(9);
        plan.cum.assign(3, 5);
        const int form = c < 3 ? c : 0;
        kx::HostCall hc;
        hc.format = form;
        if (c == 3) {
            hc.chunks_per_request = ones;
            hc.n_requests = B;
            hc.req_formats = mixed;
            hc.n_req_formats = B;
        }
        const kx::RequestLayout lay = hc.layout(B);
        CHECK(lay.R == B && lay.n_format == (c < 3 ? 1 : B) && !lay.marks && !lay.joins);
        kx::build_output_plan(frames, nullptr, nullptr, B, lay, plan);
        CHECK(plan.req.size() == (size_t)B && plan.cum.size() == (size_t)B + 1);
        long sum = 0, n = 0;
        for (int b = 0; b < B; ++b) {
            const int w = width[c < 3 ? c : mixed[b]];
            const kx::PackReq& q = plan.req[(size_t)b];
            CHECK(q.first_row == b && q.n_rows == 1 && q.form == (c < 3 ? c : mixed[b]) && q.rate == 0);
            CHECK(q.n_samples == 600L * frames[b]);
            CHECK(q.out_bytes == 600L * frames[b] * w);
            CHECK(q.out_off == sum);
            sum += q.out_bytes;
            n += 600L * frames[b];
        }
        CHECK(plan.total_bytes == sum && plan.y_floats == 0);
        // before the forward the packed buffer is sized by the requests' bound over the call's words, and holds the plan:
        // for these frames, and for B rows of one frame each
        const int* words = c < 3 ? &form : mixed;
        const int n_words = c < 3 ? 1 : B;
        CHECK(kx::output_bounds(lay, B, 1000, nullptr).packed_bytes == body_bound(words, n_words, B, 1000));
        CHECK(kx::output_bounds(lay, B, (size_t)n, nullptr).packed_bytes == body_bound(words, n_words, B, (size_t)n));
        CHECK(kx::output_bounds(lay, B, (size_t)n, nullptr).packed_bytes >= (size_t)plan.total_bytes);
        kx::build_output_plan(ones, nullptr, nullptr, B, lay, plan);
        CHECK(plan.total_bytes == (c < 3 ? 600L * B * width[c] : 600L * (4 + 8 + 2 + 2 + 8)));
        CHECK(kx::output_bounds(lay, B, (size_t)600 * B, nullptr).packed_bytes >= (size_t)plan.total_bytes);
        CHECK(kx::output_bounds(lay, B, 1000, nullptr).y_floats == 0);  // (24 kHz: nothing to resample)
    }
    printf("utterance layout: 4 assignments of forms over %d utterances\n", B);
}

static void check_plan(const std::vector<int>& frames, const std::vector<int>& chunks, const std::vector<int>& forms) {
    const int B = (int)frames.size(), R = (int)chunks.size();
    kx::OutputPlan plan;
    plan.total_bytes = 99;  // (stale contents must not survive)
    plan.max_units = 99;
    plan.req.resize(11);
    kx::build_output_plan(frames.data(), nullptr, nullptr, B, {chunks.data(), R, forms.data(), (int)forms.size(), nullptr, nullptr, 0}, plan);
    CHECK(plan.cum.size() == (size_t)B + 1 && plan.cum[0] == 0);
    for (int b = 0; b < B; ++b) CHECK(plan.cum[(size_t)b + 1] == plan.cum[(size_t)b] + 600L * frames[(size_t)b]);
    CHECK(plan.req.size() == (size_t)R);
    long off = 0, units = 0;
    int row = 0;
    for (int r = 0; r < R; ++r) {
        const kx::PackReq& q = plan.req[(size_t)r];
        long fr = 0;
        for (int i = 0; i < chunks[(size_t)r]; ++i) fr += frames[(size_t)(row + i)];
        const int form = forms[forms.size() == 1 ? 0 : (size_t)r];
        CHECK(q.first_row == row && q.n_rows == chunks[(size_t)r] && q.form == form && q.rate == 0);
        CHECK(q.n_samples == 600 * fr);
        CHECK(q.out_bytes == kx::pack_request_bytes(form, q.n_samples));
        CHECK(q.out_bytes == form_bytes(form, q.n_samples) && q.out_bytes % 4 == 0);
        CHECK(q.out_off == off);
        const long u = ((off & 15) + q.out_bytes + 15) / 16;
        units = u > units ? u : units;
        off += q.out_bytes;
        row += chunks[(size_t)r];
    }
    CHECK(row == B && plan.total_bytes == off && plan.max_units == units);
    // the grouped call's packed buffer, sized before the frame counts are known, holds the plan
    kx::HostCall hc;
    hc.chunks_per_request = chunks.data();
    hc.n_requests = R;
    hc.req_formats = forms.data();
    hc.n_req_formats = (int)forms.size();
    const size_t bound = body_bound(forms.data(), (int)forms.size(), R, (size_t)plan.cum[(size_t)B]);
    CHECK(kx::output_bounds(hc.layout(B), B, (size_t)plan.cum[(size_t)B], nullptr).packed_bytes == bound);
    CHECK((size_t)plan.total_bytes <= bound);
}

static void request_plans() {
    const std::vector<int> frames{1, 7, 422, 1, 3, 50};
    static const int mixed[6] = {4, 0, 3, 1, 2, 4};
    int n = 0;
    for (int cuts = 0; cuts < 32; ++cuts) {  // every composition of the 6 rows: a cut or none behind each of the first five
        std::vector<int> chunks{1};
        for (int i = 0; i < 5; ++i) {
            if (cuts >> i & 1) chunks.push_back(1);
            else chunks.back() += 1;
        }
        for (int form = 0; form < 5; ++form, ++n) check_plan(frames, chunks, {form});
        check_plan(frames, chunks, std::vector<int>(mixed, mixed + chunks.size()));
        ++n;
    }
    // null chunks: every row a request of its own
    kx::OutputPlan plan;
    const int forms[6] = {4, 0, 3, 1, 2, 4};
    kx::build_output_plan(frames.data(), nullptr, nullptr, 6, {nullptr, 6, forms, 6, nullptr, nullptr, 0}, plan);
    for (int r = 0; r < 6; ++r) CHECK(plan.req[(size_t)r].first_row == r && plan.req[(size_t)r].n_rows == 1 && plan.req[(size_t)r].n_samples == 600L * frames[(size_t)r]);
    printf("request plans: %d (composition, forms) pairs over 6 rows\n", n);
}

static bool refused(const std::function<void()>& call, const char* needle) {
    try {
        call();
    } catch (const kx::Error& e) {
        return e.code == 1 && strstr(e.what(), needle) != nullptr;
    }
    return false;
}

static void bounds() {
    // one frame per request is where a per-sample estimate falls short: header and base64 padding do not scale
    for (int R = 1; R <= 64; ++R)
        for (int form = 0; form < 5; ++form) check_plan(std::vector<int>((size_t)R, 1), std::vector<int>((size_t)R, 1), {form});
    // form 4: the 16-bit WAV file's size field has 32 bits
    const long first_bad = (0xFFFFFFFFL - 36) / 2 + 1;
    CHECK(36 + 2 * first_bad > 0xFFFFFFFFL && 36 + 2 * (first_bad - 1) <= 0xFFFFFFFFL);
    CHECK(refused([&] { (void)kx::pack_request_bytes(4, first_bad); }, "16-bit WAV"));
    CHECK(kx::pack_request_bytes(4, first_bad - 1) == form_bytes(4, first_bad - 1));
    CHECK(refused([&] { (void)kx::pack_request_bytes(5, 600); }, "unknown output format"));
    // ... in rows: the first request of whole frames past it, and the same request one row shorter
    const int last_ok = (int)((first_bad - 1) / 600);  // frames
    const int form4 = 4, two = 2, one = 1;
    const int fr[2] = {last_ok, 1};
    kx::OutputPlan plan;
    CHECK(refused([&] { kx::build_output_plan(fr, nullptr, nullptr, 2, {&two, 1, &form4, 1, nullptr, nullptr, 0}, plan); }, "16-bit WAV"));
    kx::build_output_plan(fr, nullptr, nullptr, 1, {&one, 1, &form4, 1, nullptr, nullptr, 0}, plan);
    CHECK(plan.req[0].n_samples == 600L * last_ok && plan.total_bytes == form_bytes(4, 600L * last_ok));
    printf("bounds: 64 x 5 one-frame batches; form 4 refused from %ld samples\n", first_bad);
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "refusals") {
        refusals();
    } else if (mode == "layout") {
        utterance_layout();
        request_plans();
        bounds();
    } else {
        fprintf(stderr, "usage: host_request_check refusals | layout\n");
        return 2;
    }
    return 0;
}
