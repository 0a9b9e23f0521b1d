// CPU checker of the prosody rules and of the report block's layout (kokorox_amd/csrc/host_request.{h,cpp}: prosody_ok,
// check_prosody_call, report_rows, build_output_plan, output_bounds): built with g++ -fsanitize=address,undefined together with
// host_request.cpp by tests/test_prosody_cpu.py and run as a child process.  The layouts come from the test (a file of cases) and go
// back as numbers, which the test compares with a numpy layout of its own; what must hold between two plans is checked here.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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

// ---- the validity rule: every edge of every range, just outside it, and NaN -------------------------------------------------------
bool ok_one(const float* rate, const int32_t* frames, const float* pitch, const float* energy) {
    const kx::ProsodySpec p{rate, frames, pitch, energy};
    const int32_t one = 1;
    return kx::prosody_ok(&p, &one, 1, 1);
}

void rule() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float below = std::nextafterf(0.25f, 0.0f), above = std::nextafterf(4.0f, 8.0f);
    int n = 0;
    // rate and pitch: 0.25 .. 4
    for (int which = 0; which < 2; ++which) {
        for (float v : {0.25f, 1.0f, 4.0f, std::nextafterf(0.25f, 1.0f), std::nextafterf(4.0f, 0.0f)}) {
            CHECK(ok_one(which == 0 ? &v : nullptr, nullptr, which == 1 ? &v : nullptr, nullptr));
            ++n;
        }
        for (float v : {below, above, 0.0f, -1.0f, nan, inf, -inf}) {
            CHECK(!ok_one(which == 0 ? &v : nullptr, nullptr, which == 1 ? &v : nullptr, nullptr));
            ++n;
        }
    }
    // energy: 0 .. 4 (a negative zero is zero)
    for (float v : {0.0f, -0.0f, 1.0f, 4.0f, std::numeric_limits<float>::denorm_min()}) {
        CHECK(ok_one(nullptr, nullptr, nullptr, &v));
        ++n;
    }
    for (float v : {-std::numeric_limits<float>::denorm_min(), above, nan, inf, -inf}) {
        CHECK(!ok_one(nullptr, nullptr, nullptr, &v));
        ++n;
    }
    // frames: 0 .. 50
    for (int32_t v : {0, 1, 49, 50}) {
        CHECK(ok_one(nullptr, &v, nullptr, nullptr));
        ++n;
    }
    for (int32_t v : {-1, 51, std::numeric_limits<int32_t>::min(), std::numeric_limits<int32_t>::max()}) {
        CHECK(!ok_one(nullptr, &v, nullptr, nullptr));
        ++n;
    }
    // null spec, null arrays; only t < lens[b] is read (the NaN behind a row's end and in the stride's slack is not looked at)
    CHECK(kx::prosody_ok(nullptr, nullptr, 0, 0));
    CHECK(ok_one(nullptr, nullptr, nullptr, nullptr));
    const int32_t lens[2] = {2, 1};
    const float two_rows[6] = {1.0f, 2.0f, nan, 0.5f, nan, nan};
    const kx::ProsodySpec p{two_rows, nullptr, two_rows, nullptr};
    CHECK(kx::prosody_ok(&p, lens, 2, 3));
    const int32_t longer[2] = {2, 2};
    CHECK(!kx::prosody_ok(&p, longer, 2, 3));
    CHECK(kx::prosody_value_ok(1.0f, 0, 1.0f, 1.0f) && !kx::prosody_value_ok(1.0f, 0, 1.0f, nan));
    printf("rule: %d single values\n", n);
}

// ---- the report block of a layout ----------------------------------------------------------------------------------------------
std::vector<long> read_longs(FILE* f, long n) {
    std::vector<long> v((size_t)n);
    for (long i = 0; i < n; ++i)
        if (fscanf(f, "%ld", &v[(size_t)i]) != 1) {
            fprintf(stderr, "bad case file\n");
            exit(2);
        }
    return v;
}

bool same_req(const kx::PackReq& a, const kx::PackReq& b) {
    return a.first_row == b.first_row && a.n_rows == b.n_rows && a.form == b.form && a.rate == b.rate && a.out_off == b.out_off &&
           a.out_bytes == b.out_bytes && a.n_samples == b.n_samples && a.src_samples == b.src_samples && a.y_off == b.y_off;
}

// every field the parent's plan has, one by one (the report's own fields are looked at by the caller)
void check_same_plan(const kx::OutputPlan& a, const kx::OutputPlan& b) {
    CHECK(a.req.size() == b.req.size());
    for (size_t r = 0; r < a.req.size(); ++r) CHECK(same_req(a.req[r], b.req[r]));
    CHECK(a.cum == b.cum && a.total_bytes == b.total_bytes && a.max_units == b.max_units && a.y_floats == b.y_floats &&
          a.max_resampled == b.max_resampled && a.joined == b.joined && a.count == b.count && a.first == b.first &&
          a.marks_off == b.marks_off && a.n_marks == b.n_marks);
    CHECK(a.join.size() == b.join.size() && a.mark.size() == b.mark.size());
    for (size_t i = 0; i < a.join.size(); ++i)
        CHECK(a.join[i].skip == b.join[i].skip && a.join[i].keep == b.join[i].keep && a.join[i].gap == b.join[i].gap &&
              a.join[i].fade_head == b.join[i].fade_head && a.join[i].fade_tail == b.join[i].fade_tail);
    for (size_t i = 0; i < a.mark.size(); ++i)
        CHECK(a.mark[i].first == b.mark[i].first && a.mark[i].base == b.mark[i].base && a.mark[i].K == b.mark[i].K &&
              a.mark[i].src_base == b.mark[i].src_base && a.mark[i].skip == b.mark[i].skip && a.mark[i].keep == b.mark[i].keep);
    CHECK(a.level.size() == b.level.size() && a.measured == b.measured && a.levelled == b.levelled && a.levels_off == b.levels_off &&
          a.peak_windows == b.peak_windows && a.true_peak == b.true_peak && a.loud.size() == b.loud.size() && a.loud_all == b.loud_all &&
          a.loud_off == b.loud_off && a.max_hops == b.max_hops && a.limit_spec.size() == b.limit_spec.size() && a.limit.size() == b.limit.size() &&
          a.limited == b.limited && a.lim_floats == b.lim_floats && a.limits_off == b.limits_off);
    CHECK(a.pack_req.size() == b.pack_req.size() && a.flac.size() == b.flac.size() && a.flac_slots == b.flac_slots &&
          a.flac_max_frames == b.flac_max_frames && a.flac_max_bytes == b.flac_max_bytes && a.flac_off == b.flac_off);
    for (size_t r = 0; r < a.pack_req.size(); ++r) CHECK(same_req(a.pack_req[r], b.pack_req[r]));
    CHECK(a.blocks_end() == b.blocks_end() && a.fixed_end() == b.fixed_end());
}

// case file: n, then per case "B R", lens [B], frames [B], chunks [R], words [R], marks [R], reports [R]
void plans(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(2);
    }
    const long n = read_longs(f, 1)[0];
    for (long c = 0; c < n; ++c) {
        const std::vector<long> br = read_longs(f, 2);
        const int B = (int)br[0], R = (int)br[1];
        const std::vector<long> lens_l = read_longs(f, B), frames_l = read_longs(f, B), cpr_l = read_longs(f, R), words_l = read_longs(f, R),
                                marks_l = read_longs(f, R), reports_l = read_longs(f, R);
        const std::vector<int> lens(lens_l.begin(), lens_l.end()), frames(frames_l.begin(), frames_l.end()), cpr(cpr_l.begin(), cpr_l.end()),
            words(words_l.begin(), words_l.end());
        const std::vector<uint8_t> marks(marks_l.begin(), marks_l.end()), reports(reports_l.begin(), reports_l.end()), none((size_t)R, 0);
        kx::RequestLayout lay{cpr.data(), R, words.data(), R, marks.data(), nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0};
        kx::OutputPlan parent, with, without;
        kx::build_output_plan(frames.data(), lens.data(), nullptr, B, lay, parent);  // (reports == null: the layout the parent knew)
        lay.reports = reports.data();
        kx::build_output_plan(frames.data(), lens.data(), nullptr, B, lay, with);
        lay.reports = none.data();
        kx::build_output_plan(frames.data(), lens.data(), nullptr, B, lay, without);
        // a plan without a report is the parent's plan field for field, whether nobody could ask or nobody did
        check_same_plan(parent, with);
        check_same_plan(parent, without);
        CHECK(parent.rep_first.empty() && parent.rep_count.empty() && parent.report_off == 0 && parent.n_report == 0 && !parent.has_report());
        CHECK(without.report_off == 0 && without.n_report == 0 && !without.has_report() && without.end_bytes() == parent.end_bytes());
        CHECK(parent.end_bytes() == parent.fixed_end());
        for (long v : without.rep_first) CHECK(v == -1);
        // the bound of the packed buffer covers the block, and moves by exactly the block's share
        const size_t n_samples = (size_t)600 * (size_t)(with.cum[(size_t)B] / 600 + 1);
        lay.reports = nullptr;
        const size_t bound_parent = kx::output_bounds(lay, B, n_samples, lens.data()).packed_bytes;
        lay.reports = reports.data();
        const size_t bound_with = kx::output_bounds(lay, B, n_samples, lens.data()).packed_bytes;
        long tokens = 0;
        for (int b = 0; b < B; ++b) tokens += lens[(size_t)b];
        CHECK(bound_with == bound_parent + 8 + 16 * (size_t)tokens);
        CHECK((size_t)with.end_bytes() <= bound_with);
        std::vector<long> first_again;
        CHECK(kx::report_rows(lay, lens.data(), B, first_again, nullptr) == with.n_report && first_again == with.rep_first);
        printf("case %ld: %ld %ld %ld %ld %ld %ld %ld |", c, with.total_bytes, with.marks_off, with.n_marks, with.fixed_end(), with.report_off,
               with.n_report, with.end_bytes());
        for (long v : with.rep_first) printf(" %ld", v);
        printf(" |");
        for (long v : with.rep_count) printf(" %ld", v);
        printf("\n");
    }
    fclose(f);
    printf("plans: %ld layouts\n", n);
}

void refusals() {
    const int cpr[2] = {1, 2};
    const int word = 0;
    const uint8_t want[2] = {1, 0};
    const int32_t lens[3] = {2, 3, 1};
    const float good[9] = {1, 1, 9, 0.25f, 4, 1, 1, 9, 9};  // (the 9s sit behind the rows' ends: never read)
    const float bad[9] = {1, 1, 1, 0.25f, 4, 5, 1, 1, 1};
    kx::HostCall hc;
    hc.chunks_per_request = cpr;
    hc.n_requests = 2;
    hc.req_formats = &word;
    hc.n_req_formats = 1;
    hc.prosody_call = true;
    hc.req_reports = want;
    float* rep = reinterpret_cast<float*>(&hc);  // (any non-null value: the check clears it)
    int64_t n[2] = {7, 7};
    auto text = [&](const kx::HostCall& c, float** a, int64_t* b) -> std::string {
        try {
            kx::check_prosody_call(c, lens, 3, 3, a, b);
        } catch (const kx::Error& e) {
            return std::to_string(e.code) + "\t" + e.what();
        }
        return "accepted";
    };
    printf("null_out_report\t%s\n", text(hc, nullptr, n).c_str());
    printf("null_out_n_report\t%s\n", text(hc, &rep, nullptr).c_str());
    kx::HostCall flat = hc;
    flat.chunks_per_request = nullptr;
    printf("report_without_requests\t%s\n", text(flat, &rep, n).c_str());
    const kx::ProsodySpec ps_good{good, nullptr, good, nullptr}, ps_bad{nullptr, nullptr, nullptr, bad};
    hc.prosody = &ps_bad;
    printf("bad_value\t%s\n", text(hc, &rep, n).c_str());
    hc.prosody = &ps_good;
    rep = reinterpret_cast<float*>(&hc);
    printf("ok\t%s\n", text(hc, &rep, n).c_str());
    CHECK(rep == nullptr);
    kx::HostCall quiet = hc;  // (no report asked for: both null is fine)
    quiet.req_reports = nullptr;
    printf("no_report\t%s\n", text(quiet, nullptr, nullptr).c_str());
    quiet.prosody = nullptr;
    printf("null_prosody\t%s\n", text(quiet, nullptr, nullptr).c_str());
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "rule") {
        rule();
        printf("checks: %d\n", g_checks);
        return 0;
    }
    if (mode == "plans" && argc > 2) {
        plans(argv[2]);
        printf("checks: %d\n", g_checks);
        return 0;
    }
    if (mode == "refusals") {
        refusals();
        return 0;
    }
    fprintf(stderr, "usage: prosody_plan_check rule | plans <case file> | refusals\n");
    return 2;
}
