// CPU driver of FLAC in the host layout (kokorox_amd/csrc/host_request.cpp: check_format_word, flac_bound, build_output_plan,
// output_bounds, close_flac_gaps): built with g++ -fsanitize=address,undefined together with host_request.cpp by
// tests/test_flac_cpu.py and run as a child process.
//
//   flac_plan_check bounds < numbers   one line "<N> <flac_bound(N)> <frames>" per sample count of the input
//   flac_plan_check plans < cases      every case of the input: "name B R", frames [B], lens [B], chunks_per_request [R], words [R],
//                                      want [R] (marks), kind [R] (0 nothing, 1 a level, 2 a loudness, 3 a limit), printed as
//       case <name>
//       req <r> <form> <rate> <out_off> <out_bytes> <n_samples> <pack out_off> <pack out_bytes> <flac frames> <flac slot>
//       sizes <total_bytes> <max_units> <marks_off> <n_marks> <levels_off> <loud_off> <limits_off> <flac_off> <end_bytes> <flac_slots> <flac_max_frames> <flac_max_bytes>
//       bounds <packed bytes> <flac slots>
//     (it judges three things itself, in every case: the same layout with every form 12 taken for form 2 has no FLAC field set and
//     its packer reads plan.req, also when the plan object held a FLAC plan before; the FLAC rows repeat the request table; and
//     output_bounds covers what the plan needs)
//   flac_plan_check refusals           one line per case: <name> TAB <code> TAB <message>, or <name> TAB accepted
//   flac_plan_check gaps < cases       every case "name R", then per request "form out_bytes length": a plan made by hand, every
//                                      region filled with its own pattern and 0xEE behind its length; prints
//       case <name> total <sum> bytes <out_bytes ..>        after close_flac_gaps, the bodies checked byte for byte, or
//       case <name> refused <message>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host_request.h"

namespace {

#define REQUIRE_SAME(cond)                                                      \
    do {                                                                        \
        if (!(cond)) {                                                          \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);            \
            exit(1);                                                            \
        }                                                                       \
    } while (0)

bool read_longs(std::vector<long>& v, size_t n) {
    v.assign(n, 0);
    for (size_t i = 0; i < n; ++i)
        if (scanf("%ld", &v[i]) != 1) return false;
    return true;
}

void no_flac(const kx::OutputPlan& p) {
    REQUIRE_SAME(!p.has_flac() && p.pack_req.empty() && p.flac.empty() && p.flac_slots == 0 && p.flac_max_frames == 0);
    REQUIRE_SAME(p.flac_max_bytes == 0 && p.flac_off == 0 && p.end_bytes() == p.blocks_end());
}

bool run_plan_case() {
    char name[64];
    int B, R;
    if (scanf("%63s %d %d", name, &B, &R) != 3) return false;
    std::vector<long> fr, ln, cp, wd, wt, kd;
    if (!read_longs(fr, (size_t)B) || !read_longs(ln, (size_t)B) || !read_longs(cp, (size_t)R) || !read_longs(wd, (size_t)R) ||
        !read_longs(wt, (size_t)R) || !read_longs(kd, (size_t)R))
        return false;
    std::vector<int> frames(fr.begin(), fr.end()), lens(ln.begin(), ln.end()), cpr(cp.begin(), cp.end()), words(wd.begin(), wd.end());
    std::vector<uint8_t> want(wt.begin(), wt.end());
    std::vector<kx::LevelSpec> level((size_t)R, kx::LevelSpec{kx::LEVEL_GAIN, 1.0f, 0.0f});
    std::vector<kx::LoudSpec> loud((size_t)R, kx::LoudSpec{kx::LOUD_NONE, 0.0f, 0.0f});
    std::vector<kx::LimitSpec> limit((size_t)R, kx::LimitSpec{kx::LIMIT_NONE, 1.0f, 0.0f, 1.0f});
    bool any_level = false, any_loud = false, any_limit = false, any_want = false, any_flac = false;
    for (int r = 0; r < R; ++r) {
        if (kd[(size_t)r] == 1) level[(size_t)r] = kx::LevelSpec{kx::LEVEL_NORMALIZE, 1.0f, 0.5f}, any_level = true;
        if (kd[(size_t)r] == 2) loud[(size_t)r] = kx::LoudSpec{kx::LOUD_NORMALIZE, -16.0f, 0.5f}, any_loud = true;
        if (kd[(size_t)r] == 3) limit[(size_t)r] = kx::LimitSpec{kx::LIMIT_GAIN | kx::PEAK_TRUE, 2.0f, 0.0f, 0.5f}, any_limit = true;
        any_want = any_want || want[(size_t)r];
        any_flac = any_flac || kx::format_form(words[(size_t)r]) == kx::FORM_FLAC;
    }
    // (a batch carries only the kinds of spec some request of it has, as the dispatcher builds it)
    const kx::RequestLayout lay{cpr.data(), R, words.data(), R, any_want ? want.data() : nullptr, nullptr, 0, any_level ? level.data() : nullptr,
                                any_level ? R : 0, any_loud ? loud.data() : nullptr, any_loud ? R : 0, any_limit ? limit.data() : nullptr,
                                any_limit ? R : 0};
    std::vector<int> as_pcm = words;
    for (int& w : as_pcm)
        if (kx::format_form(w) == kx::FORM_FLAC) w = (w & ~0xFF) | 2;
    kx::RequestLayout lay_pcm = lay;
    lay_pcm.formats = as_pcm.data();
    kx::OutputPlan plan, pcm;
    kx::build_output_plan(frames.data(), lens.data(), nullptr, B, lay, plan);
    kx::build_output_plan(frames.data(), lens.data(), nullptr, B, lay_pcm, pcm);
    no_flac(pcm);
    kx::OutputPlan again = plan;  // ... and a plan object that is used again for a call without the form forgets it
    kx::build_output_plan(frames.data(), lens.data(), nullptr, B, lay_pcm, again);
    no_flac(again);
    REQUIRE_SAME(again.total_bytes == pcm.total_bytes && again.max_units == pcm.max_units && again.end_bytes() == pcm.end_bytes());
    REQUIRE_SAME(plan.has_flac() == any_flac);
    if (!any_flac) no_flac(plan);
    printf("case %s\n", name);
    long slots = 0;
    for (int r = 0; r < R; ++r) {
        const kx::PackReq& q = plan.req[(size_t)r];
        const kx::PackReq& k = plan.has_flac() ? plan.pack_req[(size_t)r] : q;
        long f_frames = -1, f_slot = 0;
        if (plan.has_flac()) {
            const kx::FlacRow& f = plan.flac[(size_t)r];
            REQUIRE_SAME(f.out_off == q.out_off && f.out_bytes == q.out_bytes && f.n_samples == q.n_samples && f.rate == q.rate && f.slot == slots);
            REQUIRE_SAME((f.frames >= 0) == (q.form == kx::FORM_FLAC) && k.first_row == q.first_row && k.n_rows == q.n_rows && k.form == q.form &&
                         k.rate == q.rate && k.n_samples == q.n_samples && k.src_samples == q.src_samples && k.y_off == q.y_off);
            if (f.frames >= 0) {
                REQUIRE_SAME(f.frames == kx::flac_frames(q.n_samples) && q.out_bytes == kx::flac_bound(q.n_samples) && k.out_bytes == 0 && k.out_off == 0);
                slots += f.frames;
            } else {
                REQUIRE_SAME(k.out_off == q.out_off && k.out_bytes == q.out_bytes);
            }
            f_frames = f.frames, f_slot = f.slot;
        }
        printf("req %d %d %d %ld %ld %ld %ld %ld %ld %ld\n", r, q.form, q.rate, q.out_off, q.out_bytes, q.n_samples, k.out_off, k.out_bytes, f_frames,
               f_slot);
    }
    REQUIRE_SAME(slots == plan.flac_slots);
    printf("sizes %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld\n", plan.total_bytes, plan.max_units, plan.marks_off, plan.n_marks,
           plan.levels_off, plan.loud_off, plan.limits_off, plan.flac_off, plan.end_bytes(), plan.flac_slots, plan.flac_max_frames,
           plan.flac_max_bytes);
    long samples = 0;
    for (int b = 0; b < B; ++b) samples += 600L * frames[(size_t)b];
    const kx::OutputBounds bound = kx::output_bounds(lay, B, (size_t)samples, lens.data());
    const kx::OutputBounds bound_pcm = kx::output_bounds(lay_pcm, B, (size_t)samples, lens.data());
    REQUIRE_SAME((long)bound.packed_bytes >= plan.end_bytes() && (long)bound.flac_slots >= plan.flac_slots && bound_pcm.flac_slots == 0);
    REQUIRE_SAME((bound.flac_slots > 0) == any_flac && bound.y_floats == bound_pcm.y_floats && bound.peak_dwords == bound_pcm.peak_dwords &&
                 bound.hop_doubles == bound_pcm.hop_doubles && bound.lim_floats == bound_pcm.lim_floats);
    printf("bounds %zu %zu\n", bound.packed_bytes, bound.flac_slots);
    return true;
}

void refusal(const char* name, int word) {
    try {
        kx::check_format_word(word);
        printf("%s\taccepted\n", name);
    } catch (const kx::Error& e) {
        printf("%s\t%d\t%s\n", name, e.code, e.what());
    }
}

void refusals() {
    char name[64];
    for (int form : {5, 6, 7, 10, 11, 13, 14, 15, 16, 128, 255}) {
        snprintf(name, sizeof name, "form_%d", form);
        refusal(name, form);
    }
    for (int rate = 0; rate < 6; ++rate) {
        snprintf(name, sizeof name, "flac_rate_%d", rate);
        refusal(name, kx::FORM_FLAC | (rate << 8));
    }
    refusal("flac_stray_bit", kx::FORM_FLAC | 0x1000);
    refusal("flac_negative", (int)(0x80000000u | kx::FORM_FLAC));
    // the entries that take the forms 0..2 keep refusing it: a call without chunks_per_request
    const int64_t ids[3] = {0, 5, 0};
    const int32_t lens[1] = {3};
    const float speeds[1] = {1.0f};
    std::vector<float> styles(256, 0.0f);
    void* out = nullptr;
    int64_t bytes[1], samples[1];
    for (int format : {2, kx::FORM_FLAC, kx::FORM_FLAC | 0x100}) {
        kx::HostCall hc;
        hc.styles = styles.data();
        hc.format = format;
        snprintf(name, sizeof name, "per_utterance_format_%d", format);
        try {
            kx::check_host_call(ids, 3, lens, 1, speeds, hc, &out, bytes, samples, 178, 0, false);
            printf("%s\taccepted\n", name);
        } catch (const kx::Error& e) {
            printf("%s\t%d\t%s\n", name, e.code, e.what());
        }
    }
    // the request entry takes it
    const int32_t cpr[1] = {1}, words[1] = {kx::FORM_FLAC | 0x300};
    kx::HostCall hc;
    hc.styles = styles.data();
    hc.chunks_per_request = cpr, hc.n_requests = 1, hc.req_formats = words, hc.n_req_formats = 1;
    try {
        kx::check_host_call(ids, 3, lens, 1, speeds, hc, &out, bytes, samples, 178, 0, false);
        printf("request_format_flac_48000\taccepted\n");
    } catch (const kx::Error& e) {
        printf("request_format_flac_48000\t%d\t%s\n", e.code, e.what());
    }
}

bool run_gap_case() {
    char name[64];
    int R;
    if (scanf("%63s %d", name, &R) != 2) return false;
    std::vector<long> v;
    if (!read_longs(v, (size_t)3 * R)) return false;
    kx::OutputPlan plan;
    plan.req.assign((size_t)R, kx::PackReq{});
    bool any = false;
    long total = 0;
    for (int r = 0; r < R; ++r) {
        kx::PackReq& q = plan.req[(size_t)r];
        q.form = (int)v[(size_t)3 * r], q.out_off = total, q.out_bytes = v[(size_t)3 * r + 1];
        total += q.out_bytes;
        any = any || q.form == kx::FORM_FLAC;
    }
    plan.total_bytes = total;
    if (any) {
        plan.pack_req = plan.req;
        plan.flac.resize((size_t)R);
        for (int r = 0; r < R; ++r)
            plan.flac[(size_t)r] = kx::FlacRow{plan.req[(size_t)r].out_off, plan.req[(size_t)r].out_bytes, 0, plan.req[(size_t)r].form == kx::FORM_FLAC ? 1 : -1, 0, 0};
    }
    // (a heap buffer of exactly the bodies: a move past either end is the sanitizer's to report)
    std::vector<char> host((size_t)(total > 0 ? total : 1), (char)0xEE);
    std::vector<int64_t> lengths((size_t)R), out_bytes((size_t)R, -7);
    for (int r = 0; r < R; ++r) {
        lengths[(size_t)r] = v[(size_t)3 * r + 2];
        const long n = lengths[(size_t)r] < plan.req[(size_t)r].out_bytes ? lengths[(size_t)r] : plan.req[(size_t)r].out_bytes;
        for (long i = 0; i < n; ++i) host[(size_t)(plan.req[(size_t)r].out_off + i)] = (char)(16 * (r + 1) + i % 13);
    }
    try {
        const long sum = kx::close_flac_gaps(host.data(), plan, lengths.data(), out_bytes.data());
        long at = 0;
        for (int r = 0; r < R; ++r) {
            REQUIRE_SAME(out_bytes[(size_t)r] == (any ? lengths[(size_t)r] : plan.req[(size_t)r].out_bytes) && at % 4 == 0);
            for (long i = 0; i < out_bytes[(size_t)r]; ++i) REQUIRE_SAME(host[(size_t)(at + i)] == (char)(16 * (r + 1) + i % 13));
            at += out_bytes[(size_t)r];
        }
        REQUIRE_SAME(at == sum);
        printf("case %s total %ld bytes", name, sum);
        for (int r = 0; r < R; ++r) printf(" %ld", (long)out_bytes[(size_t)r]);
        printf("\n");
    } catch (const kx::Error& e) {
        printf("case %s refused %s\n", name, e.what());
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "bounds") {
        long n;
        while (scanf("%ld", &n) == 1) printf("%ld %ld %ld\n", n, kx::flac_bound(n), kx::flac_frames(n));
    } else if (mode == "plans") {
        while (run_plan_case()) {
        }
    } else if (mode == "refusals") {
        refusals();
    } else if (mode == "gaps") {
        while (run_gap_case()) {
        }
    } else {
        fprintf(stderr, "usage: flac_plan_check bounds|plans|refusals|gaps\n");
        return 2;
    }
    return 0;
}
