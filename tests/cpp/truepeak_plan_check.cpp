// CPU driver of the true-peak flag in the host layout (kokorox_amd/csrc/host_request.cpp: level_spec_ok and loud_spec_ok with
// PEAK_TRUE, build_output_plan, output_bounds, the two argument checks, the interpolator's table) and of the dispatcher's two
// submits: built with g++ -fsanitize=address,undefined together with host_request.cpp by tests/test_truepeak_cpu.py and run as a
// child process.
//
//   truepeak_plan_check specs             every low-byte mode 0..255 of both spec kinds, alone and with the flag, with the fields of
//                                         each valid mode: one line "<kind> <mode> <ok>" per mode that is accepted
//   truepeak_plan_check plans < cases     every case of the input: "name B R", frames [B], chunks_per_request [R], words [R],
//                                         level specs [R][3] and loudness specs [R][3] (mode, the bits of the two floats; a loudness
//                                         mode 4294967295 = not metered), printed as
//       case <name>
//       sizes <true_peak> <truepeak_dwords> <peak_dwords> <peak_windows> <measured> <levelled> <levels_off> <loud_off> <end_bytes>
//       bounds <packed bytes> <peak dwords> <truepeak dwords> <hop doubles>
//     (it judges one thing itself, in every case: the same layout with the flag taken out of every spec gives the same plan in every
//     field but true_peak, the second table's size and the modes themselves -- also when the plan object held a flagged plan before)
//   truepeak_plan_check refusals          one line per case: <name> TAB <code> TAB <message>, or <name> TAB accepted
//   truepeak_plan_check dispatcher        the same for kx::dispatch::Core's two submits on a stub model
//   truepeak_plan_check taps              the 72 taps as float32 bit patterns, one phase per line
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

// `b` was built from the layout of `a` with the flag taken out of every spec
void without_the_flag_is_todays_plan(const kx::OutputPlan& a, const kx::OutputPlan& b) {
    REQUIRE_SAME(a.req.size() == b.req.size() && same_bytes(a.cum, b.cum) && same_bytes(a.count, b.count) && same_bytes(a.first, b.first));
    for (size_t r = 0; r < a.req.size(); ++r) REQUIRE_SAME(!memcmp(&a.req[r], &b.req[r], sizeof(kx::PackReq)));
    REQUIRE_SAME(a.join.size() == b.join.size() && a.mark.size() == b.mark.size());
    REQUIRE_SAME(a.total_bytes == b.total_bytes && a.max_units == b.max_units && a.y_floats == b.y_floats && a.joined == b.joined);
    REQUIRE_SAME(a.max_resampled == b.max_resampled && a.marks_off == b.marks_off && a.n_marks == b.n_marks);
    REQUIRE_SAME(a.measured == b.measured && a.levels_off == b.levels_off && a.peak_windows == b.peak_windows && a.peak_dwords() == b.peak_dwords());
    REQUIRE_SAME(a.loud.size() == b.loud.size() && a.level.size() == b.level.size() && a.loud_all == b.loud_all && a.loud_off == b.loud_off);
    REQUIRE_SAME(a.max_hops == b.max_hops && a.hop_doubles() == b.hop_doubles() && a.end_bytes() == b.end_bytes());
    REQUIRE_SAME(!b.true_peak && b.truepeak_dwords() == 0);
    bool levelled = false;  // (a flagged spec is never the plain one: the levelled packer runs for it, with g as the low byte gives it)
    for (size_t r = 0; r < a.level.size(); ++r) {
        REQUIRE_SAME((a.level[r].mode & ~kx::PEAK_TRUE) == b.level[r].mode && (b.level[r].mode & kx::PEAK_TRUE) == 0);
        REQUIRE_SAME(kx::level_float_bits(a.level[r].gain) == kx::level_float_bits(b.level[r].gain) &&
                     kx::level_float_bits(a.level[r].peak) == kx::level_float_bits(b.level[r].peak));
        levelled = levelled || !kx::level_spec_plain(a.level[r]);
    }
    for (size_t r = 0; r < a.loud.size(); ++r) {
        if (a.loud[r].mode == kx::LOUD_NONE) {
            REQUIRE_SAME(b.loud[r].mode == kx::LOUD_NONE);
            continue;
        }
        REQUIRE_SAME((a.loud[r].mode & ~kx::PEAK_TRUE) == b.loud[r].mode);
        levelled = levelled || b.loud[r].mode == kx::LOUD_NORMALIZE;
    }
    REQUIRE_SAME(a.levelled == levelled && (!b.levelled || a.levelled));
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
    std::vector<long> fr, cp, wd, lv, ld;
    if (!read_longs(fr, (size_t)B) || !read_longs(cp, (size_t)R) || !read_longs(wd, (size_t)R) || !read_longs(lv, (size_t)3 * R) ||
        !read_longs(ld, (size_t)3 * R))
        return false;
    std::vector<int> frames(fr.begin(), fr.end()), cpr(cp.begin(), cp.end()), words(wd.begin(), wd.end());
    std::vector<kx::LevelSpec> level((size_t)R), level0((size_t)R);
    std::vector<kx::LoudSpec> loud((size_t)R), loud0((size_t)R);
    bool any_loud = false, flagged = false;
    for (int r = 0; r < R; ++r) {
        const size_t i = (size_t)3 * r;
        level[(size_t)r] = level0[(size_t)r] = kx::LevelSpec{(uint32_t)lv[i], from_bits((uint32_t)lv[i + 1]), from_bits((uint32_t)lv[i + 2])};
        loud[(size_t)r] = loud0[(size_t)r] = kx::LoudSpec{(uint32_t)ld[i], from_bits((uint32_t)ld[i + 1]), from_bits((uint32_t)ld[i + 2])};
        level0[(size_t)r].mode &= ~kx::PEAK_TRUE;
        const bool metered = loud[(size_t)r].mode != kx::LOUD_NONE;
        if (metered) loud0[(size_t)r].mode &= ~kx::PEAK_TRUE;
        any_loud = any_loud || metered;
        flagged = flagged || (((metered ? loud[(size_t)r].mode : level[(size_t)r].mode) & kx::PEAK_TRUE) != 0);
    }
    // (a batch without a metered request carries no loudness at all, as the dispatcher builds it)
    kx::RequestLayout lay{cpr.data(), R, words.data(), R, nullptr, nullptr, 0, level.data(), R, any_loud ? loud.data() : nullptr, any_loud ? R : 0};
    kx::RequestLayout lay0 = lay;
    lay0.levels = level0.data();
    if (any_loud) lay0.loudness = loud0.data();
    kx::OutputPlan plan, old;
    kx::build_output_plan(frames.data(), nullptr, nullptr, B, lay, plan);
    kx::build_output_plan(frames.data(), nullptr, nullptr, B, lay0, old);
    without_the_flag_is_todays_plan(plan, old);
    kx::OutputPlan again = plan;  // ... and a plan object that is used again for a call without the flag forgets it
    kx::build_output_plan(frames.data(), nullptr, nullptr, B, lay0, again);
    without_the_flag_is_todays_plan(plan, again);
    REQUIRE_SAME(plan.true_peak == flagged && plan.truepeak_dwords() == (flagged ? plan.peak_dwords() : 0));
    printf("case %s\n", name);
    printf("sizes %d %ld %ld %ld %d %d %ld %ld %ld\n", plan.true_peak ? 1 : 0, plan.truepeak_dwords(), plan.peak_dwords(), plan.peak_windows,
           plan.measured ? 1 : 0, plan.levelled ? 1 : 0, plan.levels_off, plan.loud_off, plan.end_bytes());
    long frames_all = 0;
    for (int b = 0; b < B; ++b) frames_all += frames[(size_t)b];
    const size_t n_samples = (size_t)600 * (size_t)frames_all;
    const kx::OutputBounds bound = kx::output_bounds(lay, B, n_samples, nullptr), bound0 = kx::output_bounds(lay0, B, n_samples, nullptr);
    REQUIRE_SAME(bound0.truepeak_dwords == 0 && bound0.packed_bytes == bound.packed_bytes && bound0.y_floats == bound.y_floats &&
                 bound0.peak_dwords == bound.peak_dwords && bound0.hop_doubles == bound.hop_doubles);
    REQUIRE_SAME(bound.truepeak_dwords == (flagged ? bound.peak_dwords : 0) && bound.truepeak_dwords >= (size_t)plan.truepeak_dwords() &&
                 bound.peak_dwords >= (size_t)plan.peak_dwords());
    printf("bounds %zu %zu %zu %zu\n", bound.packed_bytes, bound.peak_dwords, bound.truepeak_dwords, bound.hop_doubles);
    return true;
}

void refusal(const char* name, const kx::LevelSpec* level, const kx::LoudSpec* loud) {
    const int cpr[1] = {1}, words[1] = {0};
    kx::HostCall hc;
    hc.chunks_per_request = cpr;
    hc.n_requests = 1;
    hc.req_formats = words;
    hc.n_req_formats = 1;
    hc.levels.call = level != nullptr;
    hc.levels.specs = level;
    hc.levels.n = level ? 1 : 0;
    hc.loudness.call = loud != nullptr;
    hc.loudness.specs = loud;
    hc.loudness.n = loud ? 1 : 0;
    try {
        if (level) kx::check_spec_list(hc, hc.levels);
        if (loud) kx::check_spec_list(hc, hc.loudness);
        // ... and the planner itself, which checks every spec once more
        const int frames[1] = {3};
        const kx::RequestLayout lay = hc.layout(1);
        kx::OutputPlan plan;
        kx::build_output_plan(frames, nullptr, nullptr, 1, lay, plan);
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
            p[0] = r->level.mode, p[1] = kx::level_float_bits(r->level.gain), p[2] = kx::level_float_bits(r->level.peak);
            p[3] = r->loudness.mode, p[4] = kx::level_float_bits(r->loudness.target_lufs), p[5] = kx::level_float_bits(r->loudness.peak);
            p[6] = r->levelled ? 1u : 0u, p[7] = r->metered ? 1u : 0u;
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

void dispatcher_case(kx::dispatch::Core<StubBackend>& core, const char* name, const kx_level* level, const kx_loudness* loudness) {
    const int64_t ids[5] = {0, 5, 0, 0, 0};
    const int32_t chunk_tokens[2] = {3, 2};
    std::vector<float> styles(2 * KX_STYLE_DIM, 0.f);
    void* out = nullptr;
    int64_t nb = 0, ns = 0;
    char err[256] = "";
    const int rc = level ? core.submit_request_levelled(ids, chunk_tokens, 2, styles.data(), nullptr, nullptr, 0, 1.f, 1, 0, &out, &nb, &ns, nullptr,
                                                        nullptr, nullptr, level, nullptr, err, sizeof err)
                         : core.submit_request_loudness(ids, chunk_tokens, 2, styles.data(), nullptr, nullptr, 0, 1.f, 1, 0, &out, &nb, &ns, nullptr,
                                                        nullptr, nullptr, loudness, nullptr, err, sizeof err);
    if (rc != KX_OK) {
        printf("%s\t%d\t%s\n", name, rc, err);
        return;
    }
    const uint32_t* p = static_cast<const uint32_t*>(out);
    printf("%s\taccepted\tlevel %#x %#x %#x loudness %#x %#x %#x levelled=%u metered=%u\n", name, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]);
    free(out);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "specs")) {
        static_assert(kx::PEAK_TRUE == 0x100u && (kx::LOUD_NONE & kx::PEAK_TRUE) != 0, "the flag is bit 8, and the sentinel has it set");
        for (uint32_t flag = 0; flag <= kx::PEAK_TRUE; flag += kx::PEAK_TRUE)
            for (uint32_t low = 0; low < 256; ++low) {
                const uint32_t mode = low | flag;
                // the fields of each of the valid modes in turn: a mode is accepted when some set of them passes
                const kx::LevelSpec lv[3] = {{mode, 2.0f, 0.0f}, {mode, 1.0f, 0.5f}, {mode, 2.0f, 0.5f}};
                const kx::LoudSpec ld[2] = {{mode, 0.0f, 0.0f}, {mode, -23.0f, 0.5f}};
                int lv_ok = 0, ld_ok = 0;
                for (int i = 0; i < 3; ++i) lv_ok |= kx::level_spec_ok(lv[i]) ? 1 << i : 0;
                for (int i = 0; i < 2; ++i) ld_ok |= kx::loud_spec_ok(ld[i]) ? 1 << i : 0;
                if (lv_ok) printf("level %#x %d\n", mode, lv_ok);
                if (ld_ok) printf("loudness %#x %d\n", mode, ld_ok);
            }
        // a flagged spec is not the plain one, and the rules on the fields follow the low byte
        REQUIRE_SAME(!kx::level_spec_plain(kx::LevelSpec{kx::PEAK_TRUE, 1.0f, 0.0f}) && kx::level_spec_plain(kx::LevelSpec{0u, 1.0f, 0.0f}));
        REQUIRE_SAME(!kx::level_spec_ok(kx::LevelSpec{1u | kx::PEAK_TRUE, 2.0f, 0.5f}) && !kx::level_spec_ok(kx::LevelSpec{kx::PEAK_TRUE, 1.0f, 0.5f}) &&
                     !kx::level_spec_ok(kx::LevelSpec{2u | kx::PEAK_TRUE, 1.0f, 2.0f}) && !kx::loud_spec_ok(kx::LoudSpec{kx::PEAK_TRUE, -23.0f, 0.0f}) &&
                     !kx::loud_spec_ok(kx::LoudSpec{1u | kx::PEAK_TRUE, 1.0f, 1.0f}));
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "plans")) {
        int n = 0;
        while (run_case()) ++n;
        printf("done %d\n", n);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "refusals")) {
        const struct {
            const char* name;
            kx::LevelSpec l;
        } levels[] = {{"level_0x200", {0x200u, 1.0f, 0.0f}},          {"level_0x301", {0x101u | 0x200u, 1.0f, 0.5f}}, {"level_0x103", {0x103u, 1.0f, 0.5f}},
                      {"level_0x80000000", {0x80000000u, 1.0f, 0.0f}}, {"level_0x80000001", {0x80000001u, 1.0f, 0.5f}}, {"level_0x00010001", {0x00010001u, 1.0f, 0.5f}},
                      {"level_3", {3u, 1.0f, 0.5f}},                  {"level_none", {0xFFFFFFFFu, 1.0f, 0.0f}},      {"level_0x100_ok", {0x100u, 2.0f, 0.0f}},
                      {"level_0x101_ok", {0x101u, 1.0f, 0.5f}},       {"level_0x102_ok", {0x102u, 2.0f, 0.5f}}};
        for (const auto& c : levels) refusal(c.name, &c.l, nullptr);
        const struct {
            const char* name;
            kx::LoudSpec l;
        } louds[] = {{"loudness_0x200", {0x200u, 0.0f, 0.0f}},          {"loudness_0x301", {0x101u | 0x200u, -23.0f, 0.5f}}, {"loudness_0x103", {0x103u, -23.0f, 0.5f}},
                     {"loudness_0x102", {0x102u, -23.0f, 0.5f}},        {"loudness_none", {kx::LOUD_NONE, 0.0f, 0.0f}},     {"loudness_0x80000001", {0x80000001u, -23.0f, 1.0f}},
                     {"loudness_0x00010001", {0x00010001u, -23.0f, 1.0f}}, {"loudness_2", {2u, -23.0f, 1.0f}},             {"loudness_0x100_ok", {0x100u, 0.0f, 0.0f}},
                     {"loudness_0x101_ok", {0x101u, -23.0f, 0.5f}}};
        for (const auto& c : louds) refusal(c.name, nullptr, &c.l);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "dispatcher")) {
        StubBackend::Handle h;
        StubBackend::Handle* hs[1] = {&h};
        kx::dispatch::Core<StubBackend> core(hs, 1, 8, 0);
        const kx_level norm_tp = {KX_LEVEL_NORMALIZE | KX_PEAK_TRUE, 1.0f, 0.5f}, gain_tp = {KX_PEAK_TRUE, 2.0f, 0.0f}, lv200 = {0x200u, 1.0f, 0.0f},
                       lv103 = {0x103u, 1.0f, 0.5f}, lv301 = {0x301u, 1.0f, 0.5f}, lv_norm_gain2 = {0x101u, 2.0f, 0.5f};
        const kx_loudness meter_tp = {KX_LOUDNESS_MEASURE | KX_PEAK_TRUE, 0.0f, 0.0f}, loud_tp = {KX_LOUDNESS_NORMALIZE | KX_PEAK_TRUE, -23.0f, 0.5f},
                          ld200 = {0x200u, 0.0f, 0.0f}, ld102 = {0x102u, -23.0f, 0.5f}, ld103 = {0x103u, -23.0f, 0.5f}, none = {0xFFFFFFFFu, 0.0f, 0.0f};
        dispatcher_case(core, "level_norm_tp", &norm_tp, nullptr);
        dispatcher_case(core, "level_gain_tp", &gain_tp, nullptr);
        dispatcher_case(core, "level_0x200", &lv200, nullptr);
        dispatcher_case(core, "level_0x103", &lv103, nullptr);
        dispatcher_case(core, "level_0x301", &lv301, nullptr);
        dispatcher_case(core, "level_0x101_gain_2", &lv_norm_gain2, nullptr);
        dispatcher_case(core, "loudness_meter_tp", nullptr, &meter_tp);
        dispatcher_case(core, "loudness_norm_tp", nullptr, &loud_tp);
        dispatcher_case(core, "loudness_0x200", nullptr, &ld200);
        dispatcher_case(core, "loudness_0x102", nullptr, &ld102);
        dispatcher_case(core, "loudness_0x103", nullptr, &ld103);
        dispatcher_case(core, "loudness_none", nullptr, &none);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "taps")) {
        const float* t = kx::truepeak_taps();
        for (int f = 0; f < kx::TRUEPEAK_PHASES; ++f) {
            for (int m = 0; m < kx::TRUEPEAK_NTAPS; ++m) printf("%s%08x", m ? " " : "", kx::level_float_bits(t[f * kx::TRUEPEAK_NTAPS + m]));
            printf("\n");
        }
        return 0;
    }
    fprintf(stderr, "usage: truepeak_plan_check specs|plans|refusals|dispatcher|taps\n");
    return 2;
}
