// CPU driver of the loudness layout (kokorox_amd/csrc/host_request.cpp: build_output_plan with loudness, output_bounds,
// check_spec_list, the meter's tables) and of the dispatcher's loudness submit: built with g++ -fsanitize=address,undefined
// together with host_request.cpp by tests/test_loudness_cpu.py and run as a child process.
//
//   loudness_plan_check plans < cases   every case of the input: "name B R", frames [B], chunks_per_request [R], words [R],
//                                       n_loud (1 or R), specs [n_loud][3] (mode, the bits of target_lufs, the bits of peak;
//                                       mode 4294967295 = that request is not metered), printed as
//       case <name>
//       req <r> <out_off> <out_bytes> <n_samples> <mode> <target bits> <peak bits> <level mode>
//       sizes <total_bytes> <marks_off> <levels_off> <loud_off> <end_bytes> <measured> <levelled> <loud_all> <max_hops> <hop_doubles> <peak_windows>
//       bounds <packed bytes> <hop doubles> <peak dwords> <packed bytes of the same layout without loudness>
//     (it judges one thing itself, in every case: the same layout without loudness gives today's plan, byte for byte in every
//     field, with none of the new ones set -- also when the plan object held a loudness plan before)
//   loudness_plan_check refusals        one line per refusal: <name> TAB <code> TAB <message>, or <name> TAB accepted
//   loudness_plan_check dispatcher      the same for kx::dispatch::Core::submit_request_loudness on a stub model
//   loudness_plan_check tables          the meter's grid and its transition powers, checked against a direct evaluation
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "dispatcher_core.h"
#include "host_request.h"

namespace {

#define REQUIRE_SAME(cond)                                                      \
    do {                                                                        \
        if (!(cond)) {                                                          \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);            \
            exit(1);                                                            \
        }                                                                       \
    } while (0)

float from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}

template <class T>
bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(T)));
}

// `b` was built from the layout of `a` without its loudness: every field the plan had before loudness is equal, no new one is set
void without_loudness_is_todays_plan(const kx::OutputPlan& a, const kx::OutputPlan& b, bool levels) {
    REQUIRE_SAME(a.req.size() == b.req.size() && same_bytes(a.cum, b.cum) && same_bytes(a.count, b.count) && same_bytes(a.first, b.first));
    for (size_t r = 0; r < a.req.size(); ++r) REQUIRE_SAME(!memcmp(&a.req[r], &b.req[r], sizeof(kx::PackReq)));
    REQUIRE_SAME(a.join.size() == b.join.size() && a.mark.size() == b.mark.size());
    REQUIRE_SAME(a.total_bytes == b.total_bytes && a.max_units == b.max_units && a.y_floats == b.y_floats && a.joined == b.joined);
    REQUIRE_SAME(a.max_resampled == b.max_resampled && a.marks_off == b.marks_off && a.n_marks == b.n_marks);
    REQUIRE_SAME(b.loud.empty() && !b.loud_all && b.loud_off == 0 && b.max_hops == 0 && b.hop_doubles() == 0);
    REQUIRE_SAME(b.measured == levels && b.level.size() == (levels ? a.req.size() : 0));
    if (!levels) REQUIRE_SAME(!b.levelled && b.levels_off == 0 && b.peak_windows == 0 && b.end_bytes() == b.marks_off + 8 * b.n_marks);
    else REQUIRE_SAME(b.levels_off == a.levels_off && b.peak_windows == a.peak_windows && b.end_bytes() == b.levels_off + 16 * (long)a.req.size());
}

bool read_longs(std::vector<long>& v, size_t n) {
    v.assign(n, 0);
    for (size_t i = 0; i < n; ++i)
        if (scanf("%ld", &v[i]) != 1) return false;
    return true;
}

bool run_case() {
    char name[64];
    int B, R, n_loud;
    if (scanf("%63s %d %d", name, &B, &R) != 3) return false;
    std::vector<long> fr, cp, wd, sp;
    if (!read_longs(fr, (size_t)B) || !read_longs(cp, (size_t)R) || !read_longs(wd, (size_t)R) || scanf("%d", &n_loud) != 1 ||
        !read_longs(sp, (size_t)3 * n_loud))
        return false;
    std::vector<int> frames(fr.begin(), fr.end()), cpr(cp.begin(), cp.end()), words(wd.begin(), wd.end());
    std::vector<kx::LoudSpec> loud((size_t)n_loud);
    for (int i = 0; i < n_loud; ++i)
        loud[(size_t)i] = kx::LoudSpec{(uint32_t)sp[(size_t)3 * i], from_bits((uint32_t)sp[(size_t)3 * i + 1]), from_bits((uint32_t)sp[(size_t)3 * i + 2])};
    // (nine fields, as the drivers written before loudness give them: the two new members are zero)
    const kx::RequestLayout parent{cpr.data(), R, words.data(), R, nullptr, nullptr, 0, nullptr, 0};
    REQUIRE_SAME(parent.loudness == nullptr && parent.n_loudness == 0);
    kx::RequestLayout lay = parent;
    lay.loudness = loud.data();
    lay.n_loudness = n_loud;
    kx::OutputPlan plan, old;
    kx::build_output_plan(frames.data(), nullptr, nullptr, B, lay, plan);
    kx::build_output_plan(frames.data(), nullptr, nullptr, B, parent, old);
    without_loudness_is_todays_plan(plan, old, false);
    kx::OutputPlan again = plan;  // ... and a plan object that is used again for a call without loudness forgets it
    kx::build_output_plan(frames.data(), nullptr, nullptr, B, parent, again);
    without_loudness_is_todays_plan(plan, again, false);
    // ... and beside levels: the metered requests keep the plain level spec, the layout without loudness is today's levelled plan
    std::vector<kx::LevelSpec> levels((size_t)R, kx::LevelSpec{0u, 1.0f, 0.0f});
    for (int r = 0; r < R; ++r)
        if (loud[(size_t)(n_loud == 1 ? 0 : r)].mode == kx::LOUD_NONE) levels[(size_t)r] = kx::LevelSpec{1u, 1.0f, 0.5f};
    kx::RequestLayout with_levels = parent, both = lay;
    with_levels.levels = both.levels = levels.data();
    with_levels.n_level = both.n_level = R;
    kx::OutputPlan pl, pb;
    kx::build_output_plan(frames.data(), nullptr, nullptr, B, with_levels, pl);
    kx::build_output_plan(frames.data(), nullptr, nullptr, B, both, pb);
    without_loudness_is_todays_plan(pb, pl, true);
    REQUIRE_SAME(pb.loud_off == plan.loud_off && pb.max_hops == plan.max_hops && pb.end_bytes() == plan.end_bytes());
    printf("case %s\n", name);
    REQUIRE_SAME(plan.loud.size() == (size_t)R && plan.level.size() == (size_t)R && plan.measured);
    for (int r = 0; r < R; ++r) {
        const kx::PackReq& q = plan.req[(size_t)r];
        const kx::LoudSpec& l = plan.loud[(size_t)r];
        REQUIRE_SAME(kx::level_spec_plain(plan.level[(size_t)r]));
        printf("req %d %ld %ld %ld %u %u %u %u\n", r, q.out_off, q.out_bytes, q.n_samples, l.mode, kx::level_float_bits(l.target_lufs),
               kx::level_float_bits(l.peak), pb.level[(size_t)r].mode);
    }
    printf("sizes %ld %ld %ld %ld %ld %d %d %d %ld %ld %ld\n", plan.total_bytes, plan.marks_off, plan.levels_off, plan.loud_off, plan.end_bytes(),
           plan.measured ? 1 : 0, plan.levelled ? 1 : 0, plan.loud_all ? 1 : 0, plan.max_hops, plan.hop_doubles(), plan.peak_windows);
    long frames_all = 0;
    for (int b = 0; b < B; ++b) frames_all += frames[(size_t)b];
    const size_t n_samples = (size_t)600 * (size_t)frames_all;
    const kx::OutputBounds without = kx::output_bounds(parent, B, n_samples, nullptr);
    REQUIRE_SAME(without.peak_dwords == 0 && without.hop_doubles == 0);
    const kx::OutputBounds bound = kx::output_bounds(lay, B, n_samples, nullptr);
    const kx::OutputBounds bound_l = kx::output_bounds(with_levels, B, n_samples, nullptr), bound_b = kx::output_bounds(both, B, n_samples, nullptr);
    REQUIRE_SAME(bound_l.hop_doubles == 0 && bound_b.packed_bytes == bound_l.packed_bytes + 16 * (size_t)R && bound_b.hop_doubles == bound.hop_doubles);
    printf("bounds %zu %zu %zu %zu\n", bound.packed_bytes, bound.hop_doubles, bound.peak_dwords, without.packed_bytes);
    return true;
}

void refusal(const char* name, const kx::LoudSpec* specs, int n) {
    const int cpr[3] = {1, 2, 1}, words[1] = {0};
    kx::HostCall hc;
    hc.chunks_per_request = cpr;
    hc.n_requests = 3;
    hc.req_formats = words;
    hc.n_req_formats = 1;
    hc.loudness.call = true;
    hc.loudness.specs = specs;
    hc.loudness.n = n;
    try {
        kx::check_spec_list(hc, hc.loudness);
        printf("%s\taccepted\n", name);
    } catch (const kx::Error& e) {
        printf("%s\t%d\t%s\n", name, e.code, e.what());
    }
}

// A model that runs nothing: every request of a batch gets a body that spells the specs it arrived with.
struct StubBackend {
    struct Handle {};
    struct Out {};
    static int forward(Handle*, std::vector<kx::dispatch::Request*>& batch, Out&) {
        for (kx::dispatch::Request* r : batch) r->rc = KX_OK;
        return KX_OK;
    }
    static void distribute(std::vector<kx::dispatch::Request*>& batch, Out&) {
        for (kx::dispatch::Request* r : batch) {
            uint32_t* p = static_cast<uint32_t*>(malloc(8 * sizeof(uint32_t)));
            p[0] = r->loudness.mode, p[1] = kx::level_float_bits(r->loudness.target_lufs), p[2] = kx::level_float_bits(r->loudness.peak);
            p[3] = r->metered ? 1u : 0u, p[4] = r->levelled ? 1u : 0u, p[5] = r->joined() ? 1u : 0u, p[6] = r->join.pause_ms, p[7] = 0;
            r->out = p;
            r->out_bytes = 32;
            r->out_samples = 0;
            r->marks = nullptr;
            r->n_marks = 0;
            r->loud_out[0] = 0.25, r->loud_out[1] = 3.0, r->loud_out[2] = -23.5, r->loud_out[3] = 7.0;
        }
    }
    static int n_voices(Handle*) { return 0; }
    static int n_vocab(Handle*) { return 178; }
    static void free_out(void* p) { free(p); }
};

void dispatcher_case(kx::dispatch::Core<StubBackend>& core, const char* name, const kx_join* join, const kx_loudness* loudness, bool want_out) {
    const int64_t ids[5] = {0, 5, 0, 0, 0};
    const int32_t chunk_tokens[2] = {3, 2};
    std::vector<float> styles(2 * KX_STYLE_DIM, 0.f);
    void* out = nullptr;
    int64_t nb = 0, ns = 0;
    double v[4] = {-1.0, -1.0, -1.0, -1.0};
    char err[256] = "";
    const int rc = core.submit_request_loudness(ids, chunk_tokens, 2, styles.data(), nullptr, nullptr, 0, 1.f, 1, 0, &out, &nb, &ns, nullptr,
                                                nullptr, join, loudness, want_out ? v : nullptr, err, sizeof err);
    if (rc != KX_OK) {
        printf("%s\t%d\t%s\n", name, rc, err);
        return;
    }
    const uint32_t* p = static_cast<const uint32_t*>(out);
    printf("%s\taccepted\t%u %#x %#x metered=%u levelled=%u joined=%u pause=%u out=%g %g %g %g\n", name, p[0], p[1], p[2], p[3], p[4], p[5], p[6],
           v[0], v[1], v[2], v[3]);
    free(out);
}

// the transition powers against the recurrence itself: the state after run * k steps with no input, from each unit state
void tables() {
    static_assert(kx::loud_hop(0) == 2400 && kx::loud_hop(1) == 800 && kx::loud_hop(2) == 1600 && kx::loud_hop(3) == 4800, "a hop is 100 ms");
    for (int c = 0; c < 4; ++c) {
        const int run = kx::loud_run(c);
        REQUIRE_SAME(run % 2 == 1 && (long)kx::LOUD_THREADS * run >= kx::loud_warmup(c) + kx::loud_hop(c));
        REQUIRE_SAME((long)kx::LOUD_THREADS * (run - 2) < kx::loud_warmup(c) + kx::loud_hop(c));
        const double* k = kx::loud_coefs(c);
        const double* P = kx::loud_powers() + (size_t)c * kx::LOUD_POWERS * 16;
        // (the recurrence in long double: where that is wider than float64 the only error left is the one rounding of each entry,
        // half an ulp of a value below 1024, 1.2e-13; the bound leaves room for a host whose long double is float64)
        long double worst = 0, largest = 0;
        for (int unit = 0; unit < 4; ++unit) {
            long double s[4] = {0, 0, 0, 0};
            s[unit] = 1;
            for (int p = 0; p < kx::LOUD_POWERS; ++p) {
                for (int i = 0; i < 4; ++i) {
                    const long double d = std::fabs((long double)P[16 * p + 4 * i + unit] - s[i]), a = std::fabs(s[i]);
                    worst = d > worst ? d : worst;
                    largest = a > largest ? a : largest;
                }
                for (int n = 0; n < run; ++n) {  // one step with x = 0
                    const long double v = -(long double)k[3] * s[0] - (long double)k[4] * s[1];
                    const long double w = (long double)k[5] * v + (long double)k[6] * s[0] + (long double)k[7] * s[1] - (long double)k[8] * s[2] -
                                          (long double)k[9] * s[3];
                    s[1] = s[0], s[0] = v, s[3] = s[2], s[2] = w;
                }
            }
        }
        printf("rate %d run %d warmup %ld hop %ld powers_dev %.3Le largest %.3Le\n", c, run, kx::loud_warmup(c), kx::loud_hop(c), worst, largest);
        REQUIRE_SAME(largest < 1024 && worst < (sizeof(long double) > sizeof(double) ? 2e-13L : 1e-9L));
    }
    try {
        kx::loud_coefs(4);
        REQUIRE_SAME(false);
    } catch (const kx::Error&) {
    }
}

}  // namespace

int main(int argc, char** argv) {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    if (argc == 2 && !strcmp(argv[1], "plans")) {
        int n = 0;
        while (run_case()) ++n;
        printf("done %d\n", n);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "refusals")) {
        const kx::LoudSpec ok[3] = {{0u, 0.0f, 0.0f}, {1u, -23.0f, 1.0f}, {1u, -70.0f, 0x1p-15f}};
        refusal("null_loudness", nullptr, 1);
        refusal("n_loudness_0", ok, 0);
        refusal("n_loudness_2_of_3", ok, 2);
        refusal("n_loudness_minus_1", ok, -1);
        const struct {
            const char* name;
            kx::LoudSpec l;
        } bad[] = {{"mode_2", {2u, -23.0f, 1.0f}},         {"mode_stray_bit", {0x80000001u, -23.0f, 1.0f}}, {"mode_none", {kx::LOUD_NONE, 0.0f, 0.0f}},
                   {"target_plus_1", {1u, 1.0f, 1.0f}},    {"target_minus_71", {1u, -71.0f, 1.0f}},         {"peak_2", {1u, -23.0f, 2.0f}},
                   {"peak_small", {1u, -23.0f, 0x1p-16f}}, {"peak_0", {1u, -23.0f, 0.0f}},                  {"mode0_target_set", {0u, -23.0f, 0.0f}},
                   {"mode0_peak_set", {0u, 0.0f, 0.5f}},   {"mode0_target_minus_0", {0u, -0.0f, 0.0f}},     {"target_nan", {1u, nan, 1.0f}},
                   {"peak_nan", {1u, -23.0f, nan}},        {"mode0_target_nan", {0u, nan, 0.0f}}};
        for (const auto& b : bad) {
            refusal(b.name, &b.l, 1);
            REQUIRE_SAME(!kx::loud_spec_ok(b.l));
        }
        const kx::LoudSpec bad_last[3] = {{0u, 0.0f, 0.0f}, {1u, -23.0f, 1.0f}, {1u, -23.0f, 2.0f}};
        refusal("third_of_three_bad", bad_last, 3);
        refusal("ok_shared", ok + 1, 1);
        refusal("ok_per_request", ok, 3);
        const kx::LoudSpec edge[2] = {{1u, 0.0f, 1.0f}, {1u, -0.0f, 0x1p-15f}};
        for (const kx::LoudSpec& l : edge) REQUIRE_SAME(kx::loud_spec_ok(l));
        REQUIRE_SAME(sizeof(kx::LoudSpec) == 12);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "dispatcher")) {
        StubBackend::Handle h;
        StubBackend::Handle* hs[1] = {&h};
        kx::dispatch::Core<StubBackend> core(hs, 1, 8, 0);
        const kx_join join = {5u, 10, 85, 1}, bad_join = {8u, 0, 0, 0};
        const kx_loudness meter = {0u, 0.0f, 0.0f}, norm = {1u, -23.0f, 0.5f};
        const kx_loudness mode2 = {2u, -23.0f, 1.0f}, target1 = {1u, 1.0f, 1.0f}, peak2 = {1u, -23.0f, 2.0f}, meter_target = {0u, -23.0f, 0.0f},
                          target_nan = {1u, nan, 1.0f}, none = {0xFFFFFFFFu, 0.0f, 0.0f}, stray = {0x00010001u, -23.0f, 1.0f},
                          target71 = {1u, -71.0f, 1.0f}, peak_nan = {1u, -23.0f, nan};
        dispatcher_case(core, "null_loudness", &join, nullptr, true);
        dispatcher_case(core, "mode_2", nullptr, &mode2, true);
        dispatcher_case(core, "target_plus_1", nullptr, &target1, true);
        dispatcher_case(core, "peak_2", nullptr, &peak2, true);
        dispatcher_case(core, "mode0_target_set", nullptr, &meter_target, true);
        dispatcher_case(core, "target_nan", nullptr, &target_nan, true);
        dispatcher_case(core, "mode_none", nullptr, &none, true);
        dispatcher_case(core, "mode_stray_bit", nullptr, &stray, true);
        dispatcher_case(core, "target_minus_71", nullptr, &target71, true);
        dispatcher_case(core, "peak_nan", nullptr, &peak_nan, true);
        dispatcher_case(core, "bad_join", &bad_join, &norm, true);
        dispatcher_case(core, "ok_no_join", nullptr, &norm, true);
        dispatcher_case(core, "ok_join", &join, &norm, true);
        dispatcher_case(core, "ok_meter_no_out", nullptr, &meter, false);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "tables")) {
        tables();
        return 0;
    }
    fprintf(stderr, "usage: loudness_plan_check plans|refusals|dispatcher|tables\n");
    return 2;
}
