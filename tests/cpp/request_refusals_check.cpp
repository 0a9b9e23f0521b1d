// CPU driver that records what the request options are refused for, word for word, and which refusal wins when two arguments are
// wrong at once: the checks of the host entry (kokorox_amd/csrc/host_request.cpp) and every submit_request* of kx::dispatch::Core on
// a stub model.  Built with g++ -fsanitize=address,undefined together with host_request.cpp by tests/test_request_refusals_cpu.py
// and run as a child process.  The inputs are the smallest: R = 2 requests over three rows of three tokens.
//
//   request_refusals_check host         one line per case: <name> TAB <code> TAB <message>, or <name> TAB accepted
//   request_refusals_check dispatcher   <entry> TAB <fault>[+<fault>] TAB <code> TAB <message>, or ... TAB accepted
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dispatcher_core.h"
#include "host_request.h"

namespace {

float from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}
const float NaN = from_bits(0x7FC00000u);

// ---- the host entry -----------------------------------------------------------------------------------------------------------
// What a call hands over beside its HostCall: the output arguments the checks look at.
struct HostOut {
    void* body = nullptr;
    int64_t bytes[2], samples[2], n_marks[2], n_report[2];
    int64_t* marks_p = nullptr;
    float* report_p = nullptr;
    void** out = &body;
    int64_t** out_marks = &marks_p;
    int64_t* out_n_marks = n_marks;
    float** out_report = &report_p;
    int64_t* out_n_report = n_report;
};

const int64_t kIds[9] = {0, 5, 0, 0, 6, 0, 0, 7, 0};
const int32_t kLens[3] = {3, 3, 3}, kChunks[2] = {2, 1}, kWords[1] = {0};
const float kSpeed[3] = {1.f, 1.f, 1.f};
const uint8_t kWant[2] = {1, 1};
std::vector<float> g_styles(3 * 256, 0.f);

kx::HostCall grouped_call() {
    kx::HostCall hc;
    hc.styles = g_styles.data();
    hc.chunks_per_request = kChunks;
    hc.n_requests = 2;
    hc.req_formats = kWords;
    hc.n_req_formats = 1;
    return hc;
}

// the lists as the entries that take them set them
void set_joins(kx::HostCall& hc, const kx::JoinSpec* p, int n) { hc.joins.call = true, hc.joins.specs = p, hc.joins.n = n; }
void set_levels(kx::HostCall& hc, const kx::LevelSpec* p, int n) { hc.levels.call = true, hc.levels.specs = p, hc.levels.n = n; }
void set_loudness(kx::HostCall& hc, const kx::LoudSpec* p, int n) { hc.loudness.call = true, hc.loudness.specs = p, hc.loudness.n = n; }
void set_limits(kx::HostCall& hc, const kx::LimitSpec* p, int n) { hc.limits.call = true, hc.limits.specs = p, hc.limits.n = n; }

// The checks of Model::infer_host_once, in its order (tests/test_request_refusals_cpu.py holds the source to that order).
void host_checks(const kx::HostCall& hc, HostOut& o) {
    kx::check_host_call(kIds, 3, kLens, 3, kSpeed, hc, o.out, o.bytes, o.samples, 178, 0, false);
    if (hc.joins.call) kx::check_spec_list(hc, hc.joins);
    if (hc.req_marks) kx::check_marks_call(hc, o.out_marks, o.out_n_marks);
    if (hc.levels.call) kx::check_spec_list(hc, hc.levels);
    if (hc.loudness.call) kx::check_spec_list(hc, hc.loudness);
    if (hc.limits.call) kx::check_spec_list(hc, hc.limits);
    if (hc.prosody_call) kx::check_prosody_call(hc, kLens, 3, 3, o.out_report, o.out_n_report);
}

void host_case(const std::string& name, const kx::HostCall& hc, HostOut& o) {
    try {
        host_checks(hc, o);
        printf("%s\taccepted\n", name.c_str());
    } catch (const kx::Error& e) {
        printf("%s\t%d\t%s\n", name.c_str(), e.code, e.what());
    }
}

// null, the two bad counts, a good shared list, a good list of R, every bad spec alone, and a bad spec behind a good one
template <class Spec, class Set>
void list_cases(const char* noun, Set set, const Spec& good, const std::vector<std::pair<const char*, Spec>>& bad) {
    auto run = [&](const std::string& what, const Spec* p, int n) {
        kx::HostCall hc = grouped_call();
        set(hc, p, n);
        HostOut o;
        host_case(std::string(noun) + "." + what, hc, o);
    };
    const Spec two[2] = {good, good}, three[3] = {bad[0].second, good, good};
    run("null", nullptr, 1);
    run("count_0", &good, 0);
    run("count_3_and_bad", three, 3);
    run("shared_ok", &good, 1);
    run("per_request_ok", two, 2);
    for (const auto& b : bad) run(b.first, &b.second, 1);
    const Spec second[2] = {good, bad[0].second};
    run("second_bad", second, 2);
}

const kx::JoinSpec kJoin{kx::JOIN_TRIM_HEAD, 10, 85, 5};
const kx::LevelSpec kLevel{kx::LEVEL_CEILING, 2.0f, 0.5f};
const kx::LoudSpec kLoud{kx::LOUD_NORMALIZE, -16.0f, 0.5f};
const kx::LimitSpec kLimit{kx::LIMIT_GAIN, 2.0f, 0.0f, 0.5f};

void host_mode() {
    list_cases<kx::JoinSpec>("join", set_joins, kJoin,
                             {{"flags_8", {8u, 0, 0, 0}}, {"keep_-1", {0u, -1, 0, 0}}, {"keep_1001", {0u, 1001, 0, 0}}, {"pause_-1", {0u, 0, -1, 0}},
                              {"pause_5001", {0u, 0, 5001, 0}}, {"fade_-1", {0u, 0, 0, -1}}, {"fade_13", {0u, 0, 0, 13}}});
    list_cases<kx::LevelSpec>("level", set_levels, kLevel,
                              {{"mode_3", {3u, 1.0f, 0.5f}}, {"mode_0x200", {0x200u, 1.0f, 0.0f}}, {"gain_-0.5", {0u, -0.5f, 0.0f}}, {"gain_65", {0u, 65.0f, 0.0f}},
                               {"gain_nan", {0u, NaN, 0.0f}}, {"peak_in_mode_0", {0u, 1.0f, 0.5f}}, {"gain_in_mode_1", {1u, 2.0f, 0.5f}},
                               {"peak_0", {2u, 1.0f, 0.0f}}, {"peak_2", {2u, 1.0f, 2.0f}}, {"peak_nan", {0x102u, 1.0f, NaN}}});
    list_cases<kx::LoudSpec>("loudness", set_loudness, kLoud,
                             {{"mode_2", {2u, 0.0f, 0.0f}}, {"mode_none", {kx::LOUD_NONE, 0.0f, 0.0f}}, {"target_in_mode_0", {0u, -16.0f, 0.0f}},
                              {"peak_in_mode_0", {0u, 0.0f, 0.5f}}, {"target_-71", {1u, -71.0f, 0.5f}}, {"target_1", {1u, 1.0f, 0.5f}},
                              {"target_nan", {0x101u, NaN, 0.5f}}, {"peak_0", {1u, -16.0f, 0.0f}}, {"peak_2", {1u, -16.0f, 2.0f}}, {"peak_nan", {1u, -16.0f, NaN}}});
    list_cases<kx::LimitSpec>("limit", set_limits, kLimit,
                              {{"mode_2", {2u, 1.0f, 0.0f, 0.5f}}, {"mode_none", {kx::LIMIT_NONE, 1.0f, 0.0f, 1.0f}}, {"gain_-0.5", {0u, -0.5f, 0.0f, 0.5f}},
                               {"gain_65", {0u, 65.0f, 0.0f, 0.5f}}, {"gain_nan", {0u, NaN, 0.0f, 0.5f}}, {"target_in_mode_0", {0u, 1.0f, -16.0f, 0.5f}},
                               {"gain_in_mode_1", {1u, 2.0f, -16.0f, 0.5f}}, {"target_1", {1u, 1.0f, 1.0f, 0.5f}}, {"target_nan", {0x101u, 1.0f, NaN, 0.5f}},
                               {"peak_0", {0u, 1.0f, 0.0f, 0.0f}}, {"peak_2", {0u, 1.0f, 0.0f, 2.0f}}, {"peak_nan", {0x100u, 1.0f, 0.0f, NaN}}});
    {  // marks
        kx::HostCall hc = grouped_call();
        hc.req_marks = kWant;
        HostOut ok, no_marks, no_count;
        no_marks.out_marks = nullptr;
        no_count.out_n_marks = nullptr;
        host_case("marks.ok", hc, ok);
        host_case("marks.null_marks", hc, no_marks);
        host_case("marks.null_count", hc, no_count);
        kx::HostCall rows;  // (a call of rows, no requests)
        rows.styles = g_styles.data();
        rows.req_marks = kWant;
        HostOut o;
        host_case("marks.not_grouped", rows, o);
    }
    {  // prosody: the report pair, the report of a call of rows, every field of the spec
        kx::HostCall hc = grouped_call();
        hc.prosody_call = true;
        hc.req_reports = kWant;
        HostOut ok, no_report, no_count, neither;
        no_report.out_report = nullptr;
        no_count.out_n_report = nullptr;
        neither.out_report = nullptr, neither.out_n_report = nullptr;
        host_case("prosody.null_spec_ok", hc, ok);
        host_case("prosody.null_report", hc, no_report);
        host_case("prosody.null_count", hc, no_count);
        host_case("prosody.reports_without_the_pair", hc, neither);
        hc.req_reports = nullptr;
        host_case("prosody.no_report_ok", hc, neither);
        kx::HostCall rows;
        rows.styles = g_styles.data();
        rows.prosody_call = true;
        rows.req_reports = kWant;
        HostOut o;
        host_case("prosody.reports_not_grouped", rows, o);
        const struct {
            const char* name;
            float rate;
            int32_t frames;
            float pitch, energy;
        } bad[] = {{"rate_0.2", 0.2f, 0, 1.f, 1.f},  {"rate_5", 5.f, 0, 1.f, 1.f},   {"rate_nan", NaN, 0, 1.f, 1.f},    {"frames_-1", 1.f, -1, 1.f, 1.f},
                   {"frames_51", 1.f, 51, 1.f, 1.f}, {"pitch_0.2", 1.f, 0, 0.2f, 1.f}, {"pitch_5", 1.f, 0, 5.f, 1.f},     {"pitch_nan", 1.f, 0, NaN, 1.f},
                   {"energy_-1", 1.f, 0, 1.f, -1.f}, {"energy_5", 1.f, 0, 1.f, 5.f},   {"energy_nan", 1.f, 0, 1.f, NaN}, {"all_edges_ok", 4.f, 50, 0.25f, 0.f}};
        for (const auto& c : bad) {  // (the last token of the last row: the walk reaches it)
            std::vector<float> rate(9, 1.f), pitch(9, 1.f), energy(9, 1.f);
            std::vector<int32_t> frames(9, 0);
            rate[8] = c.rate, frames[8] = c.frames, pitch[8] = c.pitch, energy[8] = c.energy;
            const kx::ProsodySpec ps{rate.data(), frames.data(), pitch.data(), energy.data()};
            hc.prosody = &ps;
            HostOut p;
            host_case(std::string("prosody.") + c.name, hc, p);
            if (!strcmp(c.name, "rate_5")) {  // ... and the report pair is looked at before the spec
                HostOut half;
                half.out_n_report = nullptr;
                host_case("prosody.null_count_and_rate_5", hc, half);
            }
        }
    }
    // two wrong at once: the one that infer_host_once checks first is reported
    const char* names[7] = {"output", "join", "marks", "level", "loudness", "limit", "prosody"};
    for (int i = 0; i < 7; ++i)
        for (int j = i + 1; j < 7; ++j) {
            kx::HostCall hc = grouped_call();
            HostOut o;
            for (int k : {i, j}) {
                if (k == 0) o.out = nullptr;
                if (k == 1) set_joins(hc, nullptr, 1);
                if (k == 2) hc.req_marks = kWant, o.out_marks = nullptr;
                if (k == 3) set_levels(hc, nullptr, 1);
                if (k == 4) set_loudness(hc, nullptr, 1);
                if (k == 5) set_limits(hc, nullptr, 1);
                if (k == 6) hc.prosody_call = true, o.out_n_report = nullptr;
            }
            host_case(std::string("both.") + names[i] + "+" + names[j], hc, o);
        }
}

// ---- the dispatcher's submits ---------------------------------------------------------------------------------------------------
struct StubBackend {  // a model that runs nothing
    struct Handle {};
    struct Out {};
    static int forward(Handle*, std::vector<kx::dispatch::Request*>& batch, Out&) {
        for (kx::dispatch::Request* r : batch) r->rc = KX_OK;
        return KX_OK;
    }
    static void distribute(std::vector<kx::dispatch::Request*>& batch, Out&) {
        for (kx::dispatch::Request* r : batch) {
            r->out = malloc(8);
            r->out_bytes = 8;
        }
    }
    static int n_voices(Handle*) { return 0; }
    static int n_vocab(Handle*) { return 178; }
    static void free_out(void* p) { free(p); }
};
using Core = kx::dispatch::Core<StubBackend>;

enum Fault { BAD_JOIN, NULL_JOIN, BAD_SPEC, NULL_SPEC, REPORT_HALF, MARKS_HALF, MARKS_NULL, NULL_OUT, CHUNKS, TOKENS, BAD_PROSODY, N_FAULTS };
const char* kFault[N_FAULTS] = {"bad_join", "null_join", "bad_spec", "null_spec", "report_half", "marks_half", "marks_null", "null_out",
                                "chunks",   "tokens",    "bad_prosody"};
enum Entry { PLAIN, MARKS, JOINED, LEVELLED, LOUDNESS, LIMITED, PROSODY, N_ENTRIES };
const char* kEntry[N_ENTRIES] = {"request", "marks", "joined", "levelled", "loudness", "limited", "prosody"};

void submit_case(Core& core, Entry e, unsigned faults) {
    auto has = [&](Fault f) { return (faults >> f & 1u) != 0; };
    int32_t chunk_tokens[3] = {has(TOKENS) ? 0 : 3, 3, 3};
    const int n_chunks = has(CHUNKS) ? 0 : 3;
    void* body = nullptr;
    int64_t nb = 0, ns = 0, n_marks = 0, n_report = 0;
    int64_t* marks = nullptr;
    float* report = nullptr;
    void** out = has(NULL_OUT) ? nullptr : &body;
    int64_t** out_marks = has(MARKS_NULL) ? nullptr : &marks;
    int64_t* out_n_marks = has(MARKS_NULL) || has(MARKS_HALF) ? nullptr : &n_marks;
    const kx_join good_join = {KX_JOIN_TRIM_HEAD, 10, 85, 5}, bad_join = {8u, 0, 0, 0};
    const kx_join* join = has(NULL_JOIN) ? nullptr : (has(BAD_JOIN) ? &bad_join : &good_join);
    const kx_level level = {KX_LEVEL_CEILING, has(BAD_SPEC) ? 65.0f : 2.0f, 0.5f};
    const kx_loudness loud = {KX_LOUDNESS_NORMALIZE, has(BAD_SPEC) ? 1.0f : -16.0f, 0.5f};
    const kx_limit limit = {KX_LIMIT_GAIN, 2.0f, 0.0f, has(BAD_SPEC) ? 2.0f : 0.5f};
    std::vector<float> rate(9, 1.f);
    if (has(BAD_PROSODY)) rate[8] = 5.f;
    const kx_prosody pros = {rate.data(), nullptr, nullptr, nullptr};
    double five[5];
    char err[256] = "";
    int rc = -1;
    const float* st = g_styles.data();
#define COMMON kIds, chunk_tokens, n_chunks, st, nullptr, nullptr, 0, 1.f, 1, 0, out, &nb, &ns
    switch (e) {
        case PLAIN: rc = core.submit_request(COMMON, err, sizeof err); break;
        case MARKS: rc = core.submit_request_marks(COMMON, out_marks, out_n_marks, err, sizeof err); break;
        case JOINED: rc = core.submit_request_joined(COMMON, out_marks, out_n_marks, join, err, sizeof err); break;
        case LEVELLED: rc = core.submit_request_levelled(COMMON, out_marks, out_n_marks, join, has(NULL_SPEC) ? nullptr : &level, five, err, sizeof err); break;
        case LOUDNESS: rc = core.submit_request_loudness(COMMON, out_marks, out_n_marks, join, has(NULL_SPEC) ? nullptr : &loud, five, err, sizeof err); break;
        case LIMITED: rc = core.submit_request_limited(COMMON, out_marks, out_n_marks, join, has(NULL_SPEC) ? nullptr : &limit, five, err, sizeof err); break;
        case PROSODY:
            rc = core.submit_request_prosody(COMMON, out_marks, out_n_marks, join, has(NULL_SPEC) ? nullptr : &pros, &report,
                                             has(REPORT_HALF) ? nullptr : &n_report, err, sizeof err);
            break;
        default: break;
    }
#undef COMMON
    std::string what;
    for (int f = 0; f < N_FAULTS; ++f)
        if (has((Fault)f)) what += (what.empty() ? "" : "+") + std::string(kFault[f]);
    if (rc == KX_OK) {
        printf("%s\t%s\taccepted\n", kEntry[e], what.empty() ? "none" : what.c_str());
        free(body);
    } else {
        printf("%s\t%s\t%d\t%s\n", kEntry[e], what.c_str(), rc, err);
    }
}

void dispatcher_mode() {
    StubBackend::Handle h;
    StubBackend::Handle* hs[1] = {&h};
    Core core(hs, 1, 8, 0);
    // what each entry can be given wrong (the prosody entry's NULL_SPEC is the neutral prosody: accepted)
    const std::vector<Fault> faults[N_ENTRIES] = {
        {NULL_OUT, CHUNKS, TOKENS},
        {MARKS_HALF, MARKS_NULL, NULL_OUT, CHUNKS, TOKENS},
        {BAD_JOIN, NULL_JOIN, MARKS_HALF, MARKS_NULL, NULL_OUT, CHUNKS, TOKENS},
        {BAD_JOIN, NULL_JOIN, BAD_SPEC, NULL_SPEC, MARKS_HALF, MARKS_NULL, NULL_OUT, CHUNKS, TOKENS},
        {BAD_JOIN, NULL_JOIN, BAD_SPEC, NULL_SPEC, MARKS_HALF, MARKS_NULL, NULL_OUT, CHUNKS, TOKENS},
        {BAD_JOIN, NULL_JOIN, BAD_SPEC, NULL_SPEC, MARKS_HALF, MARKS_NULL, NULL_OUT, CHUNKS, TOKENS},
        {BAD_JOIN, NULL_JOIN, NULL_SPEC, REPORT_HALF, MARKS_HALF, MARKS_NULL, NULL_OUT, CHUNKS, TOKENS, BAD_PROSODY}};
    auto exclusive = [](Fault a, Fault b) {  // two states of one argument
        return (a == BAD_JOIN && b == NULL_JOIN) || (a == BAD_SPEC && b == NULL_SPEC) || (a == MARKS_HALF && b == MARKS_NULL) ||
               (a == NULL_SPEC && b == BAD_PROSODY);
    };
    for (int e = 0; e < N_ENTRIES; ++e) {
        submit_case(core, (Entry)e, 0u);
        for (Fault a : faults[e]) submit_case(core, (Entry)e, 1u << a);
        for (size_t i = 0; i < faults[e].size(); ++i)
            for (size_t j = i + 1; j < faults[e].size(); ++j)
                if (!exclusive(faults[e][i], faults[e][j])) submit_case(core, (Entry)e, 1u << faults[e][i] | 1u << faults[e][j]);
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "host")) {
        host_mode();
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "dispatcher")) {
        dispatcher_mode();
        return 0;
    }
    fprintf(stderr, "usage: request_refusals_check host|dispatcher\n");
    return 2;
}
