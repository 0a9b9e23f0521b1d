// CPU driver of the levels layout (kokorox_amd/csrc/host_request.cpp: build_output_plan with levels, output_bounds,
// check_spec_list) and of the dispatcher's levelled submit: built with g++ -fsanitize=address,undefined together with
// host_request.cpp by tests/test_levels_cpu.py and run as a child process.  It prints what the unit under test lays out, and the
// test compares that with its own arithmetic.
//
//   level_plan_check plans < cases     every case of the input, one after the other (see run_case), printed as
//       case <name>
//       req <r> <out_off> <out_bytes> <n_samples> <n_marks> <mode> <gain bits> <peak bits>
//       sizes <total_bytes> <marks_off> <n_marks> <levels_off> <end_bytes> <measured> <levelled> <peak_windows> <peak_dwords>
//       bounds <packed bytes> <resampled floats> <peak dwords> <packed bytes of the same layout without levels>
//     (one thing it does judge, in every case: the same layout without levels gives a plan that equals this one in every field
//     the parent had, has none of the new ones set, and ends where the marks end)
//   level_plan_check refusals          one line per refusal: <name> TAB <code> TAB <message>, or <name> TAB accepted
//   level_plan_check dispatcher        the same for kx::dispatch::Core::submit_request_levelled on a stub model, which records
//                                      the specs every request reached its batch with
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

template <class T>
bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {  // (vectors of long)
    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(T)));
}

float from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}

// `a` was built from a layout with levels, `b` from the same layout without: every field the plan had before levels is equal.
void without_levels_is_the_parents_plan(const kx::OutputPlan& a, const kx::OutputPlan& b, int B, int R) {
    REQUIRE_SAME(a.req.size() == (size_t)R && b.req.size() == (size_t)R && a.cum.size() == (size_t)B + 1);
    for (int r = 0; r < R; ++r) {
        const kx::PackReq &p = a.req[(size_t)r], &q = b.req[(size_t)r];
        REQUIRE_SAME(p.first_row == q.first_row && p.n_rows == q.n_rows && p.form == q.form && p.rate == q.rate);
        REQUIRE_SAME(p.out_off == q.out_off && p.out_bytes == q.out_bytes && p.n_samples == q.n_samples);
        REQUIRE_SAME(p.src_samples == q.src_samples && p.y_off == q.y_off);
    }
    REQUIRE_SAME(a.join.size() == b.join.size() && a.mark.size() == b.mark.size());
    for (size_t i = 0; i < a.join.size(); ++i) {
        const kx::JoinRow &j = a.join[i], &k = b.join[i];
        REQUIRE_SAME(k.skip == j.skip && k.keep == j.keep && k.gap == j.gap && k.fade_head == j.fade_head && k.fade_tail == j.fade_tail);
    }
    for (size_t i = 0; i < a.mark.size(); ++i) {
        const kx::MarkRow &m = a.mark[i], &n = b.mark[i];
        REQUIRE_SAME(m.first == n.first && m.base == n.base && m.K == n.K && m.src_base == n.src_base && m.skip == n.skip && m.keep == n.keep);
    }
    REQUIRE_SAME(same_bytes(a.cum, b.cum) && same_bytes(a.count, b.count) && same_bytes(a.first, b.first));
    REQUIRE_SAME(a.total_bytes == b.total_bytes && a.max_units == b.max_units && a.y_floats == b.y_floats && a.joined == b.joined);
    REQUIRE_SAME(a.max_resampled == b.max_resampled && a.marks_off == b.marks_off && a.n_marks == b.n_marks);
    REQUIRE_SAME(!b.measured && !b.levelled && b.level.empty() && b.levels_off == 0 && b.peak_windows == 0 && b.peak_dwords() == 0);
    REQUIRE_SAME(b.end_bytes() == b.marks_off + 8 * b.n_marks);
}

bool read_ints(std::vector<int>& v, size_t n) {
    v.assign(n, 0);
    for (size_t i = 0; i < n; ++i)
        if (scanf("%d", &v[i]) != 1) return false;
    return true;
}

// A case: "name B R", then lens [B], the durations of every row (lens[b] values each), chunks_per_request [R], words [R],
// has_joins, joins [R][4] (flags keep_ms pause_ms fade_ms), want [R], n_level (1 or R), levels [n_level][3] (mode, the bits
// of gain, the bits of peak).
bool run_case() {
    char name[64];
    int B, R, has_joins, n_level;
    if (scanf("%63s %d %d", name, &B, &R) != 3) return false;
    std::vector<int> lens, cpr, words, jv, want, lv;
    if (!read_ints(lens, (size_t)B)) return false;
    std::vector<int> frames((size_t)B, 0), edges((size_t)2 * B, 0);
    for (int b = 0; b < B; ++b) {
        std::vector<int> d;
        if (!read_ints(d, (size_t)lens[(size_t)b])) return false;
        for (int v : d) frames[(size_t)b] += v;
        edges[(size_t)2 * b] = d.front();
        edges[(size_t)2 * b + 1] = d.back();
    }
    if (!read_ints(cpr, (size_t)R) || !read_ints(words, (size_t)R) || scanf("%d", &has_joins) != 1 || !read_ints(jv, (size_t)4 * R) ||
        !read_ints(want, (size_t)R) || scanf("%d", &n_level) != 1 || !read_ints(lv, (size_t)3 * n_level))
        return false;
    std::vector<kx::JoinSpec> joins((size_t)R);
    std::vector<uint8_t> want8((size_t)R);
    for (int r = 0; r < R; ++r) {
        joins[(size_t)r] = kx::JoinSpec{(uint32_t)jv[(size_t)4 * r], jv[(size_t)4 * r + 1], jv[(size_t)4 * r + 2], jv[(size_t)4 * r + 3]};
        want8[(size_t)r] = (uint8_t)want[(size_t)r];
    }
    std::vector<kx::LevelSpec> levels((size_t)n_level);
    for (int i = 0; i < n_level; ++i)
        levels[(size_t)i] = kx::LevelSpec{(uint32_t)lv[(size_t)3 * i], from_bits((uint32_t)lv[(size_t)3 * i + 1]), from_bits((uint32_t)lv[(size_t)3 * i + 2])};
    // (seven fields, as the drivers written before levels give them: the two new members are zero)
    const kx::RequestLayout parent{cpr.data(), R, words.data(), R, want8.data(), has_joins ? joins.data() : nullptr, has_joins ? R : 0};
    REQUIRE_SAME(parent.levels == nullptr && parent.n_level == 0);
    kx::RequestLayout lay = parent;
    lay.levels = levels.data();
    lay.n_level = n_level;
    kx::OutputPlan plan, old;
    kx::build_output_plan(frames.data(), lens.data(), edges.data(), B, lay, plan);
    kx::build_output_plan(frames.data(), lens.data(), edges.data(), B, parent, old);
    without_levels_is_the_parents_plan(plan, old, B, R);
    // ... and a plan object that is used again for a call without levels forgets them
    kx::build_output_plan(frames.data(), lens.data(), edges.data(), B, parent, plan);
    without_levels_is_the_parents_plan(old, plan, B, R);
    kx::build_output_plan(frames.data(), lens.data(), edges.data(), B, lay, plan);
    printf("case %s\n", name);
    REQUIRE_SAME(plan.level.size() == (size_t)R);
    for (int r = 0; r < R; ++r) {
        const kx::PackReq& q = plan.req[(size_t)r];
        const kx::LevelSpec& l = plan.level[(size_t)r];
        printf("req %d %ld %ld %ld %ld %u %u %u\n", r, q.out_off, q.out_bytes, q.n_samples, plan.count[(size_t)r], l.mode,
               kx::level_float_bits(l.gain), kx::level_float_bits(l.peak));
    }
    printf("sizes %ld %ld %ld %ld %ld %d %d %ld %ld\n", plan.total_bytes, plan.marks_off, plan.n_marks, plan.levels_off, plan.end_bytes(),
           plan.measured ? 1 : 0, plan.levelled ? 1 : 0, plan.peak_windows, plan.peak_dwords());
    long frames_all = 0;
    for (int b = 0; b < B; ++b) frames_all += frames[(size_t)b];
    kx::HostCall hc;
    hc.chunks_per_request = cpr.data();
    hc.n_requests = R;
    hc.req_formats = words.data();
    hc.n_req_formats = R;
    hc.req_marks = want8.data();
    if (has_joins) {
        hc.joins.specs = joins.data();
        hc.joins.n = R;
    }
    const size_t n_samples = (size_t)600 * (size_t)frames_all;
    const kx::OutputBounds without = kx::output_bounds(hc.layout(B), B, n_samples, lens.data());
    REQUIRE_SAME(without.peak_dwords == 0);
    hc.levels.specs = levels.data();
    hc.levels.n = n_level;
    const kx::OutputBounds bound = kx::output_bounds(hc.layout(B), B, n_samples, lens.data());
    printf("bounds %zu %zu %zu %zu\n", bound.packed_bytes, bound.y_floats, bound.peak_dwords, without.packed_bytes);
    return true;
}

void refusal(const char* name, const kx::LevelSpec* levels, int n_level) {
    const int cpr[3] = {1, 2, 1}, words[1] = {0};
    kx::HostCall hc;
    hc.chunks_per_request = cpr;
    hc.n_requests = 3;
    hc.req_formats = words;
    hc.n_req_formats = 1;
    hc.levels.call = true;
    hc.levels.specs = levels;
    hc.levels.n = n_level;
    try {
        kx::check_spec_list(hc, hc.levels);
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
            p[3] = r->levelled ? 1u : 0u, p[4] = r->joined() ? 1u : 0u, p[5] = r->join.pause_ms, p[6] = r->want_marks ? 1u : 0u, p[7] = 0;
            r->out = p;
            r->out_bytes = 32;
            r->out_samples = 0;
            r->marks = nullptr;
            r->n_marks = 0;
            r->level_out[0] = 0.25;
            r->level_out[1] = 3.0;
        }
    }
    static int n_voices(Handle*) { return 0; }
    static int n_vocab(Handle*) { return 178; }
    static void free_out(void* p) { free(p); }
};

void dispatcher_case(kx::dispatch::Core<StubBackend>& core, const char* name, const kx_join* join, const kx_level* level, bool want_out) {
    const int64_t ids[5] = {0, 5, 0, 0, 0};
    const int32_t chunk_tokens[2] = {3, 2};
    std::vector<float> styles(2 * KX_STYLE_DIM, 0.f);
    void* out = nullptr;
    int64_t nb = 0, ns = 0;
    double lv[2] = {-1.0, -1.0};
    char err[256] = "";
    const int rc = core.submit_request_levelled(ids, chunk_tokens, 2, styles.data(), nullptr, nullptr, 0, 1.f, 1, 0, &out, &nb, &ns, nullptr,
                                                nullptr, join, level, want_out ? lv : nullptr, err, sizeof err);
    if (rc != KX_OK) {
        printf("%s\t%d\t%s\n", name, rc, err);
        return;
    }
    const uint32_t* p = static_cast<const uint32_t*>(out);
    printf("%s\taccepted\t%u %#x %#x levelled=%u joined=%u pause=%u out=%g %g\n", name, p[0], p[1], p[2], p[3], p[4], p[5], lv[0], lv[1]);
    free(out);
}

}  // namespace

int main(int argc, char** argv) {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    if (argc == 2 && !strcmp(argv[1], "plans")) {
        int n = 0;
        while (run_case()) ++n;
        printf("done %d\n", n);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "refusals")) {
        const kx::LevelSpec ok[3] = {{0u, 1.0f, 0.0f}, {1u, 1.0f, 0.5f}, {2u, 64.0f, 0x1p-15f}};
        refusal("null_levels", nullptr, 1);
        refusal("n_level_0", ok, 0);
        refusal("n_level_2_of_3", ok, 2);
        refusal("n_level_minus_1", ok, -1);
        const struct {
            const char* name;
            kx::LevelSpec l;
        } bad[] = {{"mode_3", {3u, 1.0f, 0.0f}},          {"mode_high_bit", {0x80000000u, 1.0f, 0.0f}}, {"gain_negative", {0u, -0.5f, 0.0f}},
                   {"gain_65", {0u, 65.0f, 0.0f}},        {"gain_nan", {0u, nan, 0.0f}},                 {"gain_inf", {2u, inf, 0.5f}},
                   {"mode0_peak_set", {0u, 1.0f, 0.5f}},  {"mode0_peak_minus_0", {0u, 1.0f, -0.0f}},    {"mode0_peak_nan", {0u, 1.0f, nan}},
                   {"mode1_gain_2", {1u, 2.0f, 0.5f}},    {"mode1_peak_0", {1u, 1.0f, 0.0f}},           {"mode1_peak_small", {1u, 1.0f, 0x1p-16f}},
                   {"mode1_peak_above_1", {1u, 1.0f, 1.0000001f}}, {"mode1_peak_nan", {1u, 1.0f, nan}}, {"mode2_peak_0", {2u, 1.0f, 0.0f}},
                   {"mode2_peak_2", {2u, 1.0f, 2.0f}},    {"mode2_peak_nan", {2u, 1.0f, nan}},          {"mode2_gain_nan", {2u, nan, 0.5f}},
                   {"mode2_peak_negative", {2u, 1.0f, -0.5f}}};
        for (const auto& b : bad) {
            refusal(b.name, &b.l, 1);
            REQUIRE_SAME(!kx::level_spec_ok(b.l));
        }
        const kx::LevelSpec bad_last[3] = {{0u, 1.0f, 0.0f}, {0u, 1.0f, 0.0f}, {1u, 1.0f, 2.0f}};
        refusal("third_of_three_bad", bad_last, 3);
        refusal("ok_shared", ok + 1, 1);
        refusal("ok_per_request", ok, 3);
        const kx::LevelSpec edge[4] = {{0u, 0.0f, 0.0f}, {0u, 64.0f, 0.0f}, {1u, 1.0f, 1.0f}, {2u, 0.0f, 0x1p-15f}};
        for (const kx::LevelSpec& l : edge) REQUIRE_SAME(kx::level_spec_ok(l) && !kx::level_spec_plain(l));
        REQUIRE_SAME(kx::level_spec_plain(ok[0]) && kx::level_spec_ok(ok[0]) && sizeof(kx::LevelSpec) == 12);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "dispatcher")) {
        StubBackend::Handle h;
        StubBackend::Handle* hs[1] = {&h};
        kx::dispatch::Core<StubBackend> core(hs, 1, 8, 0);
        const kx_join join = {5u, 10, 85, 1}, bad_join = {8u, 0, 0, 0};
        const kx_level plain = {0u, 1.0f, 0.0f}, norm = {1u, 1.0f, 0.5f}, ceil = {2u, 4.0f, 0.75f};
        const kx_level mode3 = {3u, 1.0f, 0.0f}, gain_nan = {0u, nan, 0.0f}, peak_big = {1u, 1.0f, 2.0f}, norm_gain = {1u, 2.0f, 0.5f},
                       minus_zero = {0u, 1.0f, -0.0f};
        dispatcher_case(core, "null_level", &join, nullptr, true);
        dispatcher_case(core, "mode_3", nullptr, &mode3, true);
        dispatcher_case(core, "gain_nan", nullptr, &gain_nan, true);
        dispatcher_case(core, "peak_2", nullptr, &peak_big, true);
        dispatcher_case(core, "mode1_gain_2", nullptr, &norm_gain, true);
        dispatcher_case(core, "mode0_peak_minus_0", nullptr, &minus_zero, true);
        dispatcher_case(core, "bad_join", &bad_join, &norm, true);
        dispatcher_case(core, "ok_no_join", nullptr, &norm, true);
        dispatcher_case(core, "ok_join", &join, &ceil, true);
        dispatcher_case(core, "ok_plain_no_out", nullptr, &plain, false);
        // a request through the older entry beside them: no spec, not measured
        {
            const int64_t ids[3] = {0, 5, 0};
            const int32_t chunk_tokens[1] = {3};
            std::vector<float> styles(KX_STYLE_DIM, 0.f);
            void* out = nullptr;
            int64_t nb = 0, ns = 0;
            char err[256] = "";
            const int rc = core.submit_request_joined(ids, chunk_tokens, 1, styles.data(), nullptr, nullptr, 0, 1.f, 1, 0, &out, &nb, &ns, nullptr,
                                                      nullptr, &join, err, sizeof err);
            REQUIRE_SAME(rc == KX_OK);
            const uint32_t* p = static_cast<const uint32_t*>(out);
            printf("old_entry\taccepted\t%u %#x %#x levelled=%u joined=%u pause=%u\n", p[0], p[1], p[2], p[3], p[4], p[5]);
            free(out);
        }
        return 0;
    }
    fprintf(stderr, "usage: level_plan_check plans|refusals|dispatcher\n");
    return 2;
}
