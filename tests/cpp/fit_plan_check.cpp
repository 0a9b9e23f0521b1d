// Driver of tests/test_fit_cpu.py: fit_ok / check_fit_call of kokorox_amd/csrc/host_request.{h,cpp} (include/kokorox_hip.h, "fit")
// on layouts read from a file, every refusal by name, and the call record of a call without spans.  Plain C++17, no HIP: built with
// g++ -fsanitize=address,undefined and run as a child process.
//   fit_plan_check plans <file>   the file: n, then per case "B R S stride", lens [B], cpr [R], held [B * stride], spans [4 S]
//                                 -> per case "case i: <1|0> | prefix ... | begin end frames ..." (refused: the lists are empty)
//   fit_plan_check refusals       -> "<name>\t<code>\t<text>" or "<name>\taccepted"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "host_request.h"

namespace {
void fail(const char* what) {
    fprintf(stderr, "fit_plan_check: %s\n", what);
    exit(1);
}

bool same_layout(const kx::RequestLayout& a, const kx::RequestLayout& b) {
    return a.chunks_per_request == b.chunks_per_request && a.R == b.R && a.formats == b.formats && a.n_format == b.n_format &&
           a.marks == b.marks && a.joins == b.joins && a.n_join == b.n_join && a.levels == b.levels && a.n_level == b.n_level &&
           a.loudness == b.loudness && a.n_loudness == b.n_loudness && a.limits == b.limits && a.n_limit == b.n_limit &&
           a.reports == b.reports;
}

void plans(const char* path) {
    std::ifstream in(path);
    int n = 0;
    in >> n;
    for (int c = 0; c < n; ++c) {
        int B, R, S, stride;
        in >> B >> R >> S >> stride;
        std::vector<int32_t> lens(B), cpr(R), held((size_t)B * stride);
        std::vector<kx::FitSpan> spans(S);
        for (auto& v : lens) in >> v;
        for (auto& v : cpr) in >> v;
        for (auto& v : held) in >> v;
        for (auto& s : spans) in >> s.request >> s.begin >> s.end >> s.frames;
        if (!in) fail("short case file");
        kx::FitPlan plan;
        const bool ok = kx::fit_ok(spans.data(), S, cpr.data(), R, lens.data(), B, held.data(), stride, plan);
        // the entry's check says the same, with the text of the header
        const int32_t fmt = 0;
        kx::HostCall hc;
        hc.chunks_per_request = cpr.data();
        hc.n_requests = R;
        hc.req_formats = &fmt;
        hc.n_req_formats = 1;
        const kx::ProsodySpec ps{nullptr, held.data(), nullptr, nullptr};
        hc.prosody = &ps;
        const kx::RequestLayout before = hc.layout(B);
        hc.fit_call = true;
        hc.fit_spans = spans.data();
        hc.n_fit_spans = S;
        kx::FitPlan again;
        bool threw = false;
        try {
            kx::check_fit_call(hc, lens.data(), B, stride, again);
        } catch (const kx::Error& e) {
            threw = true;
            if (std::string(e.what()) != "infer: bad fit" || e.code != 1) fail("check_fit_call: another refusal than \"infer: bad fit\"");
        }
        if (threw == ok) fail("check_fit_call and fit_ok disagree");
        if (ok && (again.prefix != plan.prefix || again.flat.size() != plan.flat.size())) fail("check_fit_call made another plan");
        // the spans are no part of what the output stage is asked: the layout is the parent's, field for field
        if (!same_layout(before, hc.layout(B))) fail("a call with spans has another output layout");
        // the same arrays back to back (the dispatcher's request) give the same answer
        std::vector<int32_t> flat_held;
        for (int b = 0; b < B; ++b) flat_held.insert(flat_held.end(), held.begin() + (size_t)b * stride, held.begin() + (size_t)b * stride + lens[b]);
        kx::FitPlan third;
        if (kx::fit_ok(spans.data(), S, cpr.data(), R, lens.data(), B, flat_held.data(), 0, third, true) != ok) fail("held_flat disagrees");
        printf("case %d: %d |", c, ok ? 1 : 0);
        if (ok)
            for (int32_t v : plan.prefix) printf(" %d", v);
        printf(" |");
        if (ok)
            for (const kx::FitFlat& f : plan.flat) {
                if (f.pad != 0) fail("a flat span's padding is not zero");
                printf(" %d %d %d", f.begin, f.end, f.frames);
            }
        printf("\n");
    }
    // a call without spans: nothing to check, nothing planned, and its record is the parent's
    kx::FitPlan plan;
    plan.prefix.assign(3, 7);
    if (!kx::fit_ok(nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, plan) || !plan.prefix.empty() || !plan.flat.empty()) fail("n_spans == 0 is not the empty plan");
    kx::HostCall fitted;
    const kx::RequestLayout plain = fitted.layout(4);
    fitted.fit_call = true;
    if (!same_layout(plain, fitted.layout(4))) fail("the record of a call without spans changed");
    const int32_t one = 5;
    kx::check_fit_call(fitted, &one, 1, 5, plan);
    printf("plans: %d layouts\n", n);
}

void refusals() {
    // two requests: rows of 4 and 3 tokens, then one row of 5; token 2 of row 0 is held at 6 frames
    const int32_t lens[3] = {4, 3, 5}, cpr[2] = {2, 1};
    int32_t held[3 * 5] = {0};
    held[2] = 6;
    auto say = [&](const char* name, const kx::FitSpan* spans, int n) {
        const int32_t fmt = 0;
        kx::HostCall hc;
        hc.chunks_per_request = cpr;
        hc.n_requests = 2;
        hc.req_formats = &fmt;
        hc.n_req_formats = 1;
        const kx::ProsodySpec ps{nullptr, held, nullptr, nullptr};
        hc.prosody = &ps;
        hc.fit_call = true;
        hc.fit_spans = spans;
        hc.n_fit_spans = n;
        kx::FitPlan plan;
        try {
            kx::check_fit_call(hc, lens, 3, 5, plan);
            printf("%s\taccepted\n", name);
        } catch (const kx::Error& e) {
            if (!plan.prefix.empty() || !plan.flat.empty()) fail("a refused call left a plan behind");
            printf("%s\t%d\t%s\n", name, e.code, e.what());
        }
    };
    auto one = [&](const char* name, kx::FitSpan s) { say(name, &s, 1); };
    one("ok", {0, 0, 7, 6 + 6});
    one("ok_at_50n", {0, 0, 7, 6 + 300});
    one("ok_second_request", {1, 1, 5, 9});
    one("request_negative", {-1, 0, 2, 4});
    one("request_past_R", {2, 0, 2, 4});
    one("begin_negative", {0, -1, 2, 4});
    one("begin_equals_end", {0, 3, 3, 4});
    one("begin_after_end", {0, 4, 3, 4});
    one("end_past_tokens", {0, 0, 8, 20});
    one("end_past_tokens_second", {1, 0, 6, 20});
    one("no_free_token", {0, 2, 3, 6});
    one("below_n", {0, 0, 7, 6 + 5});
    one("above_50n", {0, 0, 7, 6 + 301});
    one("below_held", {0, 0, 7, 3});
    const kx::FitSpan sorted[2] = {{0, 0, 2, 4}, {0, 3, 7, 8}}, swapped[2] = {{0, 3, 7, 8}, {0, 0, 2, 4}},
                      overlap[2] = {{0, 0, 4, 6 + 3}, {0, 3, 7, 8}}, by_request[2] = {{1, 0, 2, 4}, {0, 0, 2, 4}},
                      touching[2] = {{0, 0, 3, 6 + 2}, {0, 3, 7, 8}};
    say("two_sorted", sorted, 2);
    say("two_touching", touching, 2);
    say("unsorted", swapped, 2);
    say("overlapping", overlap, 2);
    say("unsorted_by_request", by_request, 2);
    say("null_spans", nullptr, 1);
    say("negative_count", sorted, -1);
    say("no_spans", nullptr, 0);
}
}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "plans" && argc > 2) {
        plans(argv[2]);
        return 0;
    }
    if (mode == "refusals") {
        refusals();
        return 0;
    }
    fprintf(stderr, "usage: fit_plan_check plans <case file> | refusals\n");
    return 2;
}
