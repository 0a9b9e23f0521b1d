// CPU checker of the token-marks layout (kokorox_amd/csrc/host_request.cpp: build_output_plan, output_bounds, check_marks_call):
// built with g++ -fsanitize=address,undefined together with host_request.cpp by tests/test_token_marks_cpu.py and run as a child
// process.  Every expectation is written out here on its own (plain sums over the rows), not taken from the unit under test.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "host_request.h"

namespace {

int g_checks = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        ++g_checks;                                                          \
        if (!(cond)) {                                                       \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

const int kLens[6] = {3, 12, 5, 7, 1, 512};
const int kFrames[6] = {4, 30, 5, 9, 1, 600};  // (any frame counts: the plan takes them as given)
const long kK[4] = {600, 200, 400, 1200};      // rate codes 0..3

// one grouping, one assignment of words and want flags: the plan against sums written out here
void check_plan(const std::vector<int>& cpr, const std::vector<int>& words, const std::vector<uint8_t>* want) {
    const int R = (int)cpr.size();
    kx::OutputPlan plan;
    kx::build_output_plan(kFrames, kLens, nullptr, 6, {cpr.data(), R, words.data(), (int)words.size(), want ? want->data() : nullptr, nullptr, 0}, plan);
    const kx::OutputPlan& mp = plan;
    CHECK((int)mp.mark.size() == 6 && (int)mp.count.size() == R && (int)mp.first.size() == R);
    CHECK(mp.marks_off % 8 == 0 && mp.marks_off >= plan.total_bytes && mp.marks_off < plan.total_bytes + 8);
    long next = 0;
    int row = 0;
    for (int r = 0; r < R; ++r) {
        const int word = words[words.size() == 1 ? 0 : (size_t)r];
        const long K = kK[(word >> 8) & 15];
        const bool wanted = want && (*want)[(size_t)r];
        long frames_before = 0, n = 0;
        CHECK(mp.first[(size_t)r] == next);
        for (int b = row; b < row + cpr[(size_t)r]; ++b) {
            const kx::MarkRow& m = mp.mark[(size_t)b];
            CHECK(m.K == K);
            CHECK(m.base == K * frames_before);
            CHECK(m.first == (wanted ? next + n : -1));
            frames_before += kFrames[b];
            n += kLens[b] + 1;
        }
        CHECK(mp.count[(size_t)r] == (wanted ? n : 0));
        // the last mark of the request (base of a row after the last + nothing) is its sample count
        CHECK(K * frames_before == plan.req[(size_t)r].n_samples);
        next += wanted ? n : 0;
        row += cpr[(size_t)r];
    }
    CHECK(mp.n_marks == next);
    CHECK(mp.end_bytes() == mp.marks_off + 8 * next);
}

void plans() {
    const std::vector<std::vector<int>> groupings = {{1, 1, 1, 1, 1, 1}, {2, 1, 3}, {6}};
    int n = 0;
    for (const auto& cpr : groupings) {
        const size_t R = cpr.size();
        for (int rate = 0; rate < 4; ++rate)
            for (int form : {0, 1, 2, 3, 4, 8, 9}) {  // (odd body sizes: G.711 and the 44-byte header move the block's start)
                std::vector<int> shared = {form | (rate << 8)};
                std::vector<uint8_t> all(R, 1), none(R, 0), some(R, 0);
                for (size_t r = 0; r < R; r += 2) some[r] = 1;
                check_plan(cpr, shared, &all);
                check_plan(cpr, shared, &none);
                check_plan(cpr, shared, &some);
                check_plan(cpr, shared, nullptr);
                n += 4;
            }
        // the four rates and mixed forms in one batch, the odd requests wanted
        std::vector<int> mixed;
        std::vector<uint8_t> odd;
        const int forms[6] = {8, 3, 2, 4, 9, 1};
        for (size_t r = 0; r < R; ++r) {
            mixed.push_back(forms[r % 6] | (int)((r + 1) % 4) << 8);
            odd.push_back(r % 2 ? 1 : 0);
        }
        if (R == 1) odd[0] = 1;
        check_plan(cpr, mixed, &odd);
        n += 1;
    }
    printf("mark plans: %d (grouping, words, want) cases over 6 rows\n", n);
}

// the bound of the bodies alone, written out: the word's bytes per sample (twice at 48 000 Hz), 64 per request, 16
size_t body_bound(int word, int R, size_t n_samples) {
    const int f = word & 255;
    const size_t w = (f == 1 ? 8 : (f == 2 ? 2 : (f == 4 ? 3 : (f >= 8 ? 1 : 4)))) * (size_t)((word >> 8) == 3 ? 2 : 1);
    return n_samples * w + (size_t)R * 64 + 16;
}

void bounds() {
    // without marks: exactly today's value; with marks: 8 + 8 x sum(lens + 1) more, and enough for one frame per token
    int n = 0;
    for (int R = 1; R <= 6; ++R) {
        std::vector<int> cpr((size_t)R, 1), lens((size_t)R), frames((size_t)R);
        std::vector<uint8_t> want((size_t)R, 1);
        long tokens = 0;
        for (int r = 0; r < R; ++r) {
            lens[(size_t)r] = r == 0 ? 1 : (r == 1 ? 512 : 3 * r);
            frames[(size_t)r] = lens[(size_t)r];  // one frame per token
            tokens += lens[(size_t)r];
        }
        for (int rate = 0; rate < 4; ++rate)
            for (int form : {0, 1, 2, 3, 4, 8, 9}) {
                const int word = form | (rate << 8);
                kx::HostCall hc;
                hc.chunks_per_request = cpr.data();
                hc.n_requests = R;
                hc.req_formats = &word;
                hc.n_req_formats = 1;
                const size_t n_samples = 600 * (size_t)tokens;
                const size_t plain = kx::output_bounds(hc.layout(R), R, n_samples, nullptr).packed_bytes;
                CHECK(plain == body_bound(word, R, n_samples));
                CHECK(kx::output_bounds(hc.layout(R), R, n_samples, lens.data()).packed_bytes == plain);  // (lens alone asks for nothing)
                hc.req_marks = want.data();
                const size_t with = kx::output_bounds(hc.layout(R), R, n_samples, lens.data()).packed_bytes;
                CHECK(with == plain + 8 + 8 * (size_t)(tokens + R));
                kx::OutputPlan mp;
                kx::build_output_plan(frames.data(), lens.data(), nullptr, R, hc.layout(R), mp);
                CHECK(mp.n_marks == tokens + R);
                CHECK((size_t)mp.end_bytes() <= with);
                ++n;
            }
    }
    // the ungrouped entries do not know marks: their bound does not move
    kx::HostCall hc;
    hc.format = 1;
    const int stereo = 1, three[3] = {1, 1, 1};
    CHECK(kx::output_bounds(hc.layout(3), 3, 1800, nullptr).packed_bytes == body_bound(stereo, 3, 1800));
    CHECK(kx::output_bounds(hc.layout(3), 3, 1800, three).packed_bytes == kx::output_bounds(hc.layout(3), 3, 1800, nullptr).packed_bytes);
    printf("bounds: %d batches of one frame per token\n", n);
}

void refusals() {
    const int cpr[2] = {1, 2};
    const int word = 0;
    const uint8_t want[2] = {1, 1};
    kx::HostCall hc;
    hc.chunks_per_request = cpr;
    hc.n_requests = 2;
    hc.req_formats = &word;
    hc.n_req_formats = 1;
    hc.req_marks = want;
    int64_t* marks = reinterpret_cast<int64_t*>(&hc);  // (any non-null value: the check clears it)
    int64_t n[2] = {7, 7};
    auto text = [&](int64_t** a, int64_t* b, const kx::HostCall& c) -> std::string {
        try {
            kx::check_marks_call(c, a, b);
        } catch (const kx::Error& e) {
            return std::to_string(e.code) + "\t" + e.what();
        }
        return "accepted";
    };
    printf("null_out_marks\t%s\n", text(nullptr, n, hc).c_str());
    printf("null_out_n_marks\t%s\n", text(&marks, nullptr, hc).c_str());
    kx::HostCall flat = hc;
    flat.chunks_per_request = nullptr;
    printf("marks_without_requests\t%s\n", text(&marks, n, flat).c_str());
    marks = reinterpret_cast<int64_t*>(&hc);
    printf("ok\t%s\n", text(&marks, n, hc).c_str());
    CHECK(marks == nullptr);
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "plans") {
        plans();
        bounds();
        printf("checks: %d\n", g_checks);
        return 0;
    }
    if (mode == "refusals") {
        refusals();
        return 0;
    }
    fprintf(stderr, "usage: marks_plan_check plans|refusals\n");
    return 2;
}
