// CPU driver of the limiter in the host layout (kokorox_amd/csrc/host_request.cpp: limit_spec_ok, limit_taps, check_spec_list,
// build_output_plan, output_bounds) and of the dispatcher's submit: built with g++ -fsanitize=address,undefined together with
// host_request.cpp by tests/test_limit_cpu.py and run as a child process.
//
//   limit_plan_check specs             every low-byte mode 0..255, alone and with the flag, with the fields of each valid mode: one line
//                                      "<mode> <ok>" per mode that is accepted (bit i of ok: field set i passed)
//   limit_plan_check plans < cases     every case of the input: "name B R", frames [B], chunks_per_request [R], words [R], level specs
//                                      [R][3], loudness specs [R][3], limit specs [R][4] (mode, the bits of the floats; a loudness or
//                                      limit mode 4294967295 = the request has none), printed as
//       case <name>
//       sizes <limited> <lim_floats> <limit_dwords> <peak_windows> <measured> <levelled> <true_peak> <levels_off> <loud_off> <limits_off> <end_bytes> <max_hops>
//       row <r> <off> <peak bits> <mode> <level mode> <gain bits> <peak bits> <loudness mode> <target bits> <peak bits>
//       bounds <packed bytes> <lim floats> <limit dwords> <peak dwords> <hop doubles> <truepeak dwords>
//     (it judges two things itself, in every case: the layout with every limit spec taken out -- as a null pointer and as specs of
//     mode LIMIT_NONE -- gives the plan of the layout that never had them, field for field, also when the plan object held a limited
//     plan before; and output_bounds covers what the plan needs)
//   limit_plan_check refusals          one line per case: <name> TAB <code> TAB <message>, or <name> TAB accepted
//   limit_plan_check dispatcher        the same for kx::dispatch::Core's submit on a stub model
//   limit_plan_check taps              W and the 2 W + 1 weights as float32 bit patterns, one rate code 0..3 per line
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// two plans of layouts without a limited request: every field
void same_plan(const kx::OutputPlan& a, const kx::OutputPlan& b) {
    REQUIRE_SAME(a.req.size() == b.req.size() && same_bytes(a.cum, b.cum) && same_bytes(a.count, b.count) && same_bytes(a.first, b.first));
    for (size_t r = 0; r < a.req.size(); ++r) REQUIRE_SAME(!memcmp(&a.req[r], &b.req[r], sizeof(kx::PackReq)));
    REQUIRE_SAME(a.join.size() == b.join.size() && a.mark.size() == b.mark.size());
    REQUIRE_SAME(a.total_bytes == b.total_bytes && a.max_units == b.max_units && a.y_floats == b.y_floats && a.joined == b.joined);
    REQUIRE_SAME(a.max_resampled == b.max_resampled && a.marks_off == b.marks_off && a.n_marks == b.n_marks);
    REQUIRE_SAME(a.measured == b.measured && a.levelled == b.levelled && a.levels_off == b.levels_off && a.peak_windows == b.peak_windows);
    REQUIRE_SAME(a.true_peak == b.true_peak && a.truepeak_dwords() == b.truepeak_dwords() && a.peak_dwords() == b.peak_dwords());
    REQUIRE_SAME(a.loud_all == b.loud_all && a.loud_off == b.loud_off && a.max_hops == b.max_hops && a.hop_doubles() == b.hop_doubles());
    REQUIRE_SAME(a.end_bytes() == b.end_bytes() && a.level.size() == b.level.size() && a.loud.size() == b.loud.size());
    for (size_t r = 0; r < a.level.size(); ++r) REQUIRE_SAME(!memcmp(&a.level[r], &b.level[r], sizeof(kx::LevelSpec)));
    for (size_t r = 0; r < a.loud.size(); ++r) REQUIRE_SAME(!memcmp(&a.loud[r], &b.loud[r], sizeof(kx::LoudSpec)));
    REQUIRE_SAME(!a.limited && !b.limited && a.limit.empty() && b.limit.empty() && a.limit_spec.empty() && b.limit_spec.empty());
    REQUIRE_SAME(a.lim_floats == 0 && b.lim_floats == 0 && a.limits_off == 0 && b.limits_off == 0 && a.limit_dwords() == 0 && b.limit_dwords() == 0);
}

bool read_longs(std::vector<long>& v, size_t n) {
    v.assign(n, 0);
    for (size_t i = 0; i < n; ++i)
        if (scanf("%ld", &v[i]) != 1) return false;
    return true;
}

bool run_case() {
    char name[64];
    int B, R;
    if (scanf("%63s %d %d", name, &B, &R) != 3) return false;
    std::vector<long> fr, cp, wd, lv, ld, lm;
    if (!read_longs(fr, (size_t)B) || !read_longs(cp, (size_t)R) || !read_longs(wd, (size_t)R) || !read_longs(lv, (size_t)3 * R) ||
        !read_longs(ld, (size_t)3 * R) || !read_longs(lm, (size_t)4 * R))
        return false;
    std::vector<int> frames(fr.begin(), fr.end()), cpr(cp.begin(), cp.end()), words(wd.begin(), wd.end());
    std::vector<kx::LevelSpec> level((size_t)R);
    std::vector<kx::LoudSpec> loud((size_t)R);
    std::vector<kx::LimitSpec> limit((size_t)R), none((size_t)R, kx::LimitSpec{kx::LIMIT_NONE, 1.0f, 0.0f, 1.0f});
    bool any_loud = false, any_level = false, any_limit = false;
    for (int r = 0; r < R; ++r) {
        const size_t i = (size_t)3 * r, j = (size_t)4 * r;
        level[(size_t)r] = kx::LevelSpec{(uint32_t)lv[i], from_bits((uint32_t)lv[i + 1]), from_bits((uint32_t)lv[i + 2])};
        loud[(size_t)r] = kx::LoudSpec{(uint32_t)ld[i], from_bits((uint32_t)ld[i + 1]), from_bits((uint32_t)ld[i + 2])};
        limit[(size_t)r] = kx::LimitSpec{(uint32_t)lm[j], from_bits((uint32_t)lm[j + 1]), from_bits((uint32_t)lm[j + 2]), from_bits((uint32_t)lm[j + 3])};
        any_level = any_level || !kx::level_spec_plain(level[(size_t)r]);
        any_loud = any_loud || loud[(size_t)r].mode != kx::LOUD_NONE;
        any_limit = any_limit || limit[(size_t)r].mode != kx::LIMIT_NONE;
    }
    // (a batch carries only the kinds of spec some request of it has, as the dispatcher builds it)
    const kx::RequestLayout lay0{cpr.data(), R, words.data(), R, nullptr, nullptr, 0, any_level ? level.data() : nullptr, any_level ? R : 0,
                                 any_loud ? loud.data() : nullptr, any_loud ? R : 0, nullptr, 0};
    kx::RequestLayout lay = lay0, lay_none = lay0;
    lay.limits = limit.data(), lay.n_limit = R;
    lay_none.limits = none.data(), lay_none.n_limit = R;
    kx::OutputPlan plan, old, unlimited;
    kx::build_output_plan(frames.data(), nullptr, nullptr, B, lay, plan);
    kx::build_output_plan(frames.data(), nullptr, nullptr, B, lay0, old);
    kx::build_output_plan(frames.data(), nullptr, nullptr, B, lay_none, unlimited);
    same_plan(old, unlimited);
    kx::OutputPlan again = plan;  // ... and a plan object that is used again for a call without limits forgets them
    kx::build_output_plan(frames.data(), nullptr, nullptr, B, lay0, again);
    same_plan(old, again);
    REQUIRE_SAME(plan.limited == any_limit);
    if (!any_limit) same_plan(old, plan);
    printf("case %s\n", name);
    printf("sizes %d %ld %ld %ld %d %d %d %ld %ld %ld %ld %ld\n", plan.limited ? 1 : 0, plan.lim_floats, plan.limit_dwords(), plan.peak_windows,
           plan.measured ? 1 : 0, plan.levelled ? 1 : 0, plan.true_peak ? 1 : 0, plan.levels_off, plan.loud_off, plan.limits_off, plan.end_bytes(),
           plan.max_hops);
    for (int r = 0; plan.limited && r < R; ++r) {
        const kx::LimitRow& q = plan.limit[(size_t)r];
        const kx::LevelSpec& l = plan.level[(size_t)r];
        const kx::LoudSpec& d = plan.loud[(size_t)r];
        REQUIRE_SAME(!memcmp(&plan.limit_spec[(size_t)r], &limit[(size_t)r], sizeof(kx::LimitSpec)));
        printf("row %d %ld %u %u %u %u %u %u %u %u\n", r, q.off, kx::level_float_bits(q.peak), q.mode, l.mode, kx::level_float_bits(l.gain),
               kx::level_float_bits(l.peak), d.mode, kx::level_float_bits(d.target_lufs), kx::level_float_bits(d.peak));
    }
    long frames_all = 0;
    for (int b = 0; b < B; ++b) frames_all += frames[(size_t)b];
    const size_t n_samples = (size_t)600 * (size_t)frames_all;
    const kx::OutputBounds bound = kx::output_bounds(lay, B, n_samples, nullptr), bound0 = kx::output_bounds(lay0, B, n_samples, nullptr),
                           bound_none = kx::output_bounds(lay_none, B, n_samples, nullptr);
    REQUIRE_SAME(!memcmp(&bound0, &bound_none, sizeof bound0) && bound0.lim_floats == 0 && bound0.limit_dwords == 0);
    REQUIRE_SAME(bound.packed_bytes >= (size_t)plan.end_bytes() && bound.lim_floats >= (size_t)plan.lim_floats &&
                 bound.limit_dwords >= (size_t)plan.limit_dwords() && bound.peak_dwords >= (size_t)plan.peak_dwords() &&
                 bound.hop_doubles >= (size_t)plan.hop_doubles() && bound.truepeak_dwords >= (size_t)plan.truepeak_dwords() &&
                 bound.y_floats >= (size_t)plan.y_floats);
    REQUIRE_SAME(any_limit || !memcmp(&bound, &bound0, sizeof bound));
    printf("bounds %zu %zu %zu %zu %zu %zu\n", bound.packed_bytes, bound.lim_floats, bound.limit_dwords, bound.peak_dwords, bound.hop_doubles,
           bound.truepeak_dwords);
    return true;
}

void refusal(const char* name, const kx::LimitSpec* limit, int n_limit, int R = 1, const kx::LevelSpec* level = nullptr,
             const kx::LoudSpec* loud = nullptr) {
    const int cpr[2] = {1, 1}, words[1] = {0};
    kx::HostCall hc;
    hc.chunks_per_request = cpr;
    hc.n_requests = R;
    hc.req_formats = words;
    hc.n_req_formats = 1;
    hc.limits.call = true;
    hc.limits.specs = limit;
    hc.limits.n = n_limit;
    hc.levels.specs = level;
    hc.levels.n = level ? 1 : 0;
    hc.loudness.specs = loud;
    hc.loudness.n = loud ? 1 : 0;
    try {
        kx::check_spec_list(hc, hc.limits);
        // ... and the planner itself, which checks every spec once more and that a request has one kind of spec
        const int frames[2] = {3, 3};
        const kx::RequestLayout lay = hc.layout(R);
        kx::OutputPlan plan;
        kx::build_output_plan(frames, nullptr, nullptr, R, lay, plan);
        printf("%s\taccepted\n", name);
    } catch (const kx::Error& e) {
        printf("%s\t%d\t%s\n", name, e.code, e.what());
    }
}

// A model that runs nothing: every request of a batch gets a body that spells the spec it arrived with.
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
            p[0] = r->limit.mode, p[1] = kx::level_float_bits(r->limit.gain), p[2] = kx::level_float_bits(r->limit.target_lufs);
            p[3] = kx::level_float_bits(r->limit.peak), p[4] = r->limited ? 1u : 0u, p[5] = r->levelled ? 1u : 0u, p[6] = r->metered ? 1u : 0u;
            p[7] = r->join.pause_ms;
            for (int i = 0; i < 5; ++i) r->limit_out[i] = 10.0 + i;
            r->out = p;
            r->out_bytes = 32;
            r->out_samples = 0;
            r->marks = nullptr;
            r->n_marks = 0;
        }
    }
    static int n_voices(Handle*) { return 0; }
    static int n_vocab(Handle*) { return 178; }
    static void free_out(void* p) { free(p); }
};

void dispatcher_case(kx::dispatch::Core<StubBackend>& core, const char* name, const kx_limit* limit, const kx_join* join = nullptr) {
    const int64_t ids[5] = {0, 5, 0, 0, 0};
    const int32_t chunk_tokens[2] = {3, 2};
    std::vector<float> styles(2 * KX_STYLE_DIM, 0.f);
    void* out = nullptr;
    int64_t nb = 0, ns = 0;
    double five[5] = {0, 0, 0, 0, 0};
    char err[256] = "";
    const int rc = core.submit_request_limited(ids, chunk_tokens, 2, styles.data(), nullptr, nullptr, 0, 1.f, 1, 0, &out, &nb, &ns, nullptr, nullptr,
                                               join, limit, five, err, sizeof err);
    if (rc != KX_OK) {
        printf("%s\t%d\t%s\n", name, rc, err);
        return;
    }
    const uint32_t* p = static_cast<const uint32_t*>(out);
    printf("%s\taccepted\tlimit %#x %#x %#x %#x limited=%u levelled=%u metered=%u pause=%u out %g %g %g %g %g\n", name, p[0], p[1], p[2], p[3], p[4],
           p[5], p[6], p[7], five[0], five[1], five[2], five[3], five[4]);
    free(out);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "specs")) {
        static_assert((kx::LIMIT_NONE & kx::PEAK_TRUE) != 0 && sizeof(kx::LimitSpec) == 16 && sizeof(kx::LimitRow) == 16, "the sentinel has the flag's bit set");
        for (uint32_t flag = 0; flag <= kx::PEAK_TRUE; flag += kx::PEAK_TRUE)
            for (uint32_t low = 0; low < 256; ++low) {
                const uint32_t mode = low | flag;
                const kx::LimitSpec lm[2] = {{mode, 2.0f, 0.0f, 0.5f}, {mode, 1.0f, -16.0f, 0.5f}};
                int ok = 0;
                for (int i = 0; i < 2; ++i) ok |= kx::limit_spec_ok(lm[i]) ? 1 << i : 0;
                if (ok) printf("%#x %d\n", mode, ok);
            }
        // the edges of every range, and -0.0 where +0.0 is asked for
        REQUIRE_SAME(kx::limit_spec_ok({0u, 0.0f, 0.0f, 0x1p-15f}) && kx::limit_spec_ok({0u, 64.0f, 0.0f, 1.0f}) && kx::limit_spec_ok({1u, 1.0f, -70.0f, 1.0f}) &&
                     kx::limit_spec_ok({1u, 1.0f, 0.0f, 0x1p-15f}) && kx::limit_spec_ok({1u, 1.0f, -0.0f, 0.5f}));
        REQUIRE_SAME(!kx::limit_spec_ok({0u, 1.0f, -0.0f, 0.5f}) && !kx::limit_spec_ok({0u, 1.0f, 0.0f, 0x1p-16f}) && !kx::limit_spec_ok({0u, 64.5f, 0.0f, 0.5f}) &&
                     !kx::limit_spec_ok({0u, -0.5f, 0.0f, 0.5f}) && !kx::limit_spec_ok({1u, 1.0f, -70.5f, 0.5f}) && !kx::limit_spec_ok({1u, 1.0f, 0.5f, 0.5f}) &&
                     !kx::limit_spec_ok({1u, 0.5f, -16.0f, 0.5f}) && !kx::limit_spec_ok({0u, 1.0f, 0.0f, 1.5f}) && !kx::limit_spec_ok({kx::LIMIT_NONE, 1.0f, 0.0f, 1.0f}));
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "plans")) {
        int n = 0;
        while (run_case()) ++n;
        printf("done %d\n", n);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "refusals")) {
        const float nan = from_bits(0x7FC00000u);
        const kx::LimitSpec ok{0u, 2.0f, 0.0f, 0.5f}, ok1{0x101u, 1.0f, -16.0f, 1.0f};
        refusal("null", nullptr, 1);
        refusal("count_0", &ok, 0);
        refusal("count_3", &ok, 3, 2);
        refusal("shared_ok", &ok, 1, 2);
        refusal("loud_tp_ok", &ok1, 1);
        const struct {
            const char* name;
            kx::LimitSpec l;
        } bad[] = {{"mode_2", {2u, 1.0f, 0.0f, 0.5f}},        {"mode_0x200", {0x200u, 1.0f, 0.0f, 0.5f}}, {"mode_0x80000000", {0x80000000u, 1.0f, 0.0f, 0.5f}},
                   {"mode_none", {kx::LIMIT_NONE, 1.0f, 0.0f, 1.0f}}, {"gain_65", {0u, 65.0f, 0.0f, 0.5f}},       {"gain_nan", {0u, nan, 0.0f, 0.5f}},
                   {"target_in_mode_0", {0u, 1.0f, -16.0f, 0.5f}}, {"peak_2", {0u, 1.0f, 0.0f, 2.0f}},         {"peak_0", {0u, 1.0f, 0.0f, 0.0f}},
                   {"peak_nan", {0x100u, 1.0f, 0.0f, nan}},     {"gain_in_mode_1", {1u, 2.0f, -16.0f, 0.5f}}, {"target_1", {1u, 1.0f, 1.0f, 0.5f}},
                   {"target_nan", {0x101u, 1.0f, nan, 0.5f}}};
        for (const auto& c : bad) refusal(c.name, &c.l, 1);
        // one kind of spec per request
        const kx::LevelSpec ceiling{kx::LEVEL_CEILING, 2.0f, 0.5f}, plain{kx::LEVEL_GAIN, 1.0f, 0.0f};
        const kx::LoudSpec meter{kx::LOUD_MEASURE, 0.0f, 0.0f}, not_metered{kx::LOUD_NONE, 0.0f, 0.0f};
        refusal("with_a_level", &ok, 1, 1, &ceiling, nullptr);
        refusal("with_the_plain_level_ok", &ok, 1, 1, &plain, nullptr);
        refusal("with_a_loudness", &ok, 1, 1, nullptr, &meter);
        refusal("beside_unmetered_ok", &ok, 1, 1, nullptr, &not_metered);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "dispatcher")) {
        StubBackend::Handle h;
        StubBackend::Handle* hs[1] = {&h};
        kx::dispatch::Core<StubBackend> core(hs, 1, 8, 0);
        const kx_limit gain = {KX_LIMIT_GAIN, 2.0f, 0.0f, 0.5f}, loud_tp = {KX_LIMIT_LOUDNESS | KX_PEAK_TRUE, 1.0f, -16.0f, 0.5f},
                       m2 = {2u, 1.0f, 0.0f, 0.5f}, m200 = {0x200u, 1.0f, 0.0f, 0.5f}, peak2 = {0u, 1.0f, 0.0f, 2.0f}, none = {0xFFFFFFFFu, 1.0f, 0.0f, 1.0f};
        const kx_join pause = {0u, 0, 85, 0}, bad_join = {8u, 0, 0, 0};
        dispatcher_case(core, "gain", &gain);
        dispatcher_case(core, "loudness_tp_joined", &loud_tp, &pause);
        dispatcher_case(core, "null", nullptr);
        dispatcher_case(core, "mode_2", &m2);
        dispatcher_case(core, "mode_0x200", &m200);
        dispatcher_case(core, "peak_2", &peak2);
        dispatcher_case(core, "none", &none);
        dispatcher_case(core, "bad_join", &gain, &bad_join);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "taps")) {
        for (int c = 0; c < 4; ++c) {
            const float* t = kx::limit_taps(c);
            printf("%d", kx::limit_window(c));
            for (int i = 0; i < 2 * kx::limit_window(c) + 1; ++i) printf(" %08x", kx::level_float_bits(t[i]));
            printf("\n");
        }
        return 0;
    }
    fprintf(stderr, "usage: limit_plan_check specs|plans|refusals|dispatcher|taps\n");
    return 2;
}
