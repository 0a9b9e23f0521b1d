// CPU driver of the join layout (kokorox_amd/csrc/host_request.cpp: build_output_plan with joins and marks,
// output_bounds, check_spec_list): built with g++ -fsanitize=address,undefined
// together with host_request.cpp by tests/test_joins_cpu.py and run as a child process.  It judges nothing itself: it prints
// what the unit under test lays out, and the test compares that with the hand-derived answers of tests/golden/joins.json and
// with the numpy definition (kokorox_amd/voices.py).
//
//   join_plan_check plans < cases      every case of the input, one after the other (see read_case), printed as
//       case <name>
//       row <b> <skip> <keep> <gap> <fade_head> <fade_tail>
//       req <r> <out_off> <out_bytes> <n_samples> <src_samples> <n_marks>
//       marks <r> <values ...>          (from the rows of the mark plan, with token_marks_joined_kernel's arithmetic)
//       sizes <total_bytes> <end_bytes> <y_floats> <bound of the packed bytes> <bound of the resampled floats> <joined>
//     (one thing it does judge, in every case: the same rows, grouping, words and want flags with no specs at all and with
//     all-zero specs give equal plans, field for field, and both select the plain kernels)
//   join_plan_check refusals           one line per refusal: <name> TAB <code> TAB <message>, or <name> TAB accepted
//   join_plan_check dispatcher         the same for kx::dispatch::Core::submit_request_joined on a stub model, which records
//                                      the spec every request reached its batch with
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

template <class T>
bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {  // (vectors of long)
    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(T)));
}

// A layout with null joins and the same layout with all-zero specs: equal request tables, prefixes, rows, marks and counts,
// and the plain kernels for both.
void plain_specs_equal_no_specs(const std::vector<int>& frames, const std::vector<int>& lens, const std::vector<int>& edges,
                                const kx::RequestLayout& lay) {
    const int B = (int)frames.size();
    const std::vector<kx::JoinSpec> zeros((size_t)lay.R, kx::JoinSpec{0u, 0, 0, 0});
    kx::RequestLayout none = lay, zero = lay;
    none.joins = nullptr, none.n_join = 0;
    zero.joins = zeros.data(), zero.n_join = lay.R;
    kx::OutputPlan a, b;
    kx::build_output_plan(frames.data(), lens.data(), nullptr, B, none, a);
    kx::build_output_plan(frames.data(), lens.data(), edges.data(), B, zero, b);
    REQUIRE_SAME(!a.joined && !b.joined);
    REQUIRE_SAME(a.req.size() == (size_t)lay.R && a.cum.size() == (size_t)B + 1 && a.mark.size() == (size_t)B);
    for (int r = 0; r < lay.R; ++r) {
        const kx::PackReq &p = a.req[(size_t)r], &q = b.req[(size_t)r];
        REQUIRE_SAME(p.first_row == q.first_row && p.n_rows == q.n_rows && p.form == q.form && p.rate == q.rate);
        REQUIRE_SAME(p.out_off == q.out_off && p.out_bytes == q.out_bytes && p.n_samples == q.n_samples);
        REQUIRE_SAME(p.src_samples == q.src_samples && p.y_off == q.y_off);
    }
    for (int i = 0; i < B; ++i) {
        const kx::JoinRow &j = a.join[(size_t)i], &k = b.join[(size_t)i];
        REQUIRE_SAME(j.skip == 0 && j.keep == 600L * frames[(size_t)i] && j.gap == 0 && j.fade_head == 0 && j.fade_tail == 0);
        REQUIRE_SAME(k.skip == j.skip && k.keep == j.keep && k.gap == j.gap && k.fade_head == j.fade_head && k.fade_tail == j.fade_tail);
        const kx::MarkRow &m = a.mark[(size_t)i], &n = b.mark[(size_t)i];
        REQUIRE_SAME(m.first == n.first && m.base == n.base && m.K == n.K && m.src_base == n.src_base && m.skip == n.skip && m.keep == n.keep);
    }
    REQUIRE_SAME(same_bytes(a.cum, b.cum) && same_bytes(a.count, b.count) && same_bytes(a.first, b.first));
    REQUIRE_SAME(a.total_bytes == b.total_bytes && a.max_units == b.max_units && a.y_floats == b.y_floats);
    REQUIRE_SAME(a.max_resampled == b.max_resampled && a.marks_off == b.marks_off && a.n_marks == b.n_marks);
}

bool read_ints(std::vector<int>& v, size_t n) {
    v.assign(n, 0);
    for (size_t i = 0; i < n; ++i)
        if (scanf("%d", &v[i]) != 1) return false;
    return true;
}

// A case: "name B R", then lens [B], the durations of every row (lens[b] values each), chunks_per_request [R], words [R],
// joins [R][4] (flags keep_ms pause_ms fade_ms), want [R].
bool run_case() {
    char name[64];
    int B, R;
    if (scanf("%63s %d %d", name, &B, &R) != 3) return false;
    std::vector<int> lens, cpr, words, jv, want;
    if (!read_ints(lens, (size_t)B)) return false;
    std::vector<std::vector<int>> dur((size_t)B);
    std::vector<int> frames((size_t)B, 0), edges((size_t)2 * B, 0);
    for (int b = 0; b < B; ++b) {
        if (!read_ints(dur[(size_t)b], (size_t)lens[(size_t)b])) return false;
        for (int d : dur[(size_t)b]) frames[(size_t)b] += d;
        edges[(size_t)2 * b] = dur[(size_t)b].front();
        edges[(size_t)2 * b + 1] = dur[(size_t)b].back();
    }
    if (!read_ints(cpr, (size_t)R) || !read_ints(words, (size_t)R) || !read_ints(jv, (size_t)4 * R) || !read_ints(want, (size_t)R)) return false;
    std::vector<kx::JoinSpec> joins((size_t)R);
    std::vector<uint8_t> want8((size_t)R);
    for (int r = 0; r < R; ++r) {
        joins[(size_t)r] = kx::JoinSpec{(uint32_t)jv[(size_t)4 * r], jv[(size_t)4 * r + 1], jv[(size_t)4 * r + 2], jv[(size_t)4 * r + 3]};
        want8[(size_t)r] = (uint8_t)want[(size_t)r];
    }
    const kx::RequestLayout lay{cpr.data(), R, words.data(), R, want8.data(), joins.data(), R};
    kx::OutputPlan plan;
    kx::build_output_plan(frames.data(), lens.data(), edges.data(), B, lay, plan);
    const kx::OutputPlan &jp = plan, &mp = plan;
    plain_specs_equal_no_specs(frames, lens, edges, lay);
    printf("case %s\n", name);
    for (int b = 0; b < B; ++b) {
        const kx::JoinRow& j = jp.join[(size_t)b];
        printf("row %d %ld %ld %ld %d %d\n", b, j.skip, j.keep, j.gap, j.fade_head, j.fade_tail);
    }
    long frames_all = 0;
    for (int b = 0; b < B; ++b) frames_all += frames[(size_t)b];
    for (int r = 0; r < R; ++r) {
        const kx::PackReq& q = plan.req[(size_t)r];
        printf("req %d %ld %ld %ld %ld %ld\n", r, q.out_off, q.out_bytes, q.n_samples, q.src_samples, mp.count[(size_t)r]);
        if (!mp.count[(size_t)r]) continue;
        printf("marks %d", r);
        for (int b = q.first_row; b < q.first_row + q.n_rows; ++b) {
            const kx::MarkRow& m = mp.mark[(size_t)b];
            long scan = 0;
            for (int t = 0; t <= lens[(size_t)b]; ++t) {  // (the kernel's value from the row's fields, in 64 bits)
                long u = 600 * scan - m.skip;
                u = u < 0 ? 0 : (u > m.keep ? m.keep : u);
                printf(" %ld", (m.src_base + u) * m.K / 600);
                if (t < lens[(size_t)b]) scan += dur[(size_t)b][(size_t)t];
            }
        }
        printf("\n");
    }
    kx::HostCall hc;
    hc.chunks_per_request = cpr.data();
    hc.n_requests = R;
    hc.req_formats = words.data();
    hc.n_req_formats = R;
    hc.req_marks = want8.data();
    hc.joins.specs = joins.data();
    hc.joins.n = R;
    const size_t n_samples = (size_t)600 * (size_t)frames_all;
    const kx::OutputBounds bound = kx::output_bounds(hc.layout(B), B, n_samples, lens.data());
    printf("sizes %ld %ld %ld %zu %zu %d\n", plan.total_bytes, mp.end_bytes(), plan.y_floats, bound.packed_bytes, bound.y_floats,
           jp.joined ? 1 : 0);
    return true;
}

void refusal(const char* name, const kx::JoinSpec* joins, int n_join, bool marks, bool one_mark_null) {
    const int cpr[3] = {1, 2, 1}, words[1] = {0};
    const uint8_t want[3] = {1, 1, 1};
    kx::HostCall hc;
    hc.chunks_per_request = cpr;
    hc.n_requests = 3;
    hc.req_formats = words;
    hc.n_req_formats = 1;
    hc.joins.call = true;
    hc.joins.specs = joins;
    hc.joins.n = n_join;
    int64_t* mk = nullptr;
    int64_t n_mk[3] = {0, 0, 0};
    try {
        kx::check_spec_list(hc, hc.joins);
        if (marks) {  // (the entry sets req_marks when either marks argument is there)
            hc.req_marks = want;
            kx::check_marks_call(hc, one_mark_null ? nullptr : &mk, n_mk);
        }
        printf("%s\taccepted\n", name);
    } catch (const kx::Error& e) {
        printf("%s\t%d\t%s\n", name, e.code, e.what());
    }
}

// A model that runs nothing: every request of a batch gets a body that spells the join spec it arrived with.
struct StubBackend {
    struct Handle {};
    struct Out {};
    static int forward(Handle*, std::vector<kx::dispatch::Request*>& batch, Out&) {
        for (kx::dispatch::Request* r : batch) r->rc = KX_OK;
        return KX_OK;
    }
    static void distribute(std::vector<kx::dispatch::Request*>& batch, Out&) {
        for (kx::dispatch::Request* r : batch) {
            int32_t* p = static_cast<int32_t*>(malloc(6 * sizeof(int32_t) + 8));
            p[0] = (int32_t)r->join.flags, p[1] = r->join.keep_ms, p[2] = r->join.pause_ms, p[3] = r->join.fade_ms;
            p[4] = r->joined() ? 1 : 0, p[5] = r->want_marks ? 1 : 0;
            r->out = p;
            r->out_bytes = 24;
            r->out_samples = 0;
            r->marks = r->want_marks ? reinterpret_cast<int64_t*>(p + 6) : nullptr;
            r->n_marks = r->want_marks ? 1 : 0;
            if (r->marks) r->marks[0] = 7;
        }
    }
    static int n_voices(Handle*) { return 0; }
    static int n_vocab(Handle*) { return 178; }
    static void free_out(void* p) { free(p); }
};

void dispatcher_case(kx::dispatch::Core<StubBackend>& core, const char* name, const kx_join* join, bool out_marks, bool out_n_marks) {
    const int64_t ids[5] = {0, 5, 0, 0, 0};
    const int32_t chunk_tokens[2] = {3, 2};
    std::vector<float> styles(2 * KX_STYLE_DIM, 0.f);
    void* out = nullptr;
    int64_t nb = 0, ns = 0, n_mk = 0;
    int64_t* mk = nullptr;
    char err[256] = "";
    const int rc = core.submit_request_joined(ids, chunk_tokens, 2, styles.data(), nullptr, nullptr, 0, 1.f, 1, 0, &out, &nb, &ns,
                                              out_marks ? &mk : nullptr, out_n_marks ? &n_mk : nullptr, join, err, sizeof err);
    if (rc != KX_OK) {
        printf("%s\t%d\t%s\n", name, rc, err);
        return;
    }
    const int32_t* p = static_cast<const int32_t*>(out);
    printf("%s\taccepted\t%d %d %d %d joined=%d marks=%d n_marks=%ld\n", name, p[0], p[1], p[2], p[3], p[4], p[5], (long)n_mk);
    free(out);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "plans")) {
        int n = 0;
        while (run_case()) ++n;
        printf("done %d\n", n);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "refusals")) {
        const kx::JoinSpec ok[3] = {{5u, 10, 85, 1}, {0u, 0, 0, 0}, {7u, 1000, 5000, 12}};
        refusal("null_joins", nullptr, 1, false, false);
        refusal("n_join_0", ok, 0, false, false);
        refusal("n_join_2_of_3", ok, 2, false, false);
        const kx::JoinSpec bit8[1] = {{8u, 0, 0, 0}}, keep_neg[1] = {{1u, -1, 0, 0}}, keep_big[1] = {{1u, 1001, 0, 0}},
                           pause_neg[1] = {{0u, 0, -1, 0}}, pause_big[1] = {{0u, 0, 5001, 0}}, fade_neg[1] = {{1u, 0, 0, -1}},
                           fade_big[1] = {{1u, 0, 0, 13}};
        refusal("flag_bit_8", bit8, 1, false, false);
        refusal("keep_minus_1", keep_neg, 1, false, false);
        refusal("keep_1001", keep_big, 1, false, false);
        refusal("pause_minus_1", pause_neg, 1, false, false);
        refusal("pause_5001", pause_big, 1, false, false);
        refusal("fade_minus_1", fade_neg, 1, false, false);
        refusal("fade_13", fade_big, 1, false, false);
        const kx::JoinSpec bad_last[3] = {{0u, 0, 0, 0}, {0u, 0, 0, 0}, {0u, 0, 0, 13}};
        refusal("third_of_three_bad", bad_last, 3, false, false);
        refusal("one_marks_pointer_null", ok, 3, true, true);
        refusal("ok_shared", ok, 1, false, false);
        refusal("ok_per_request_with_marks", ok, 3, true, false);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "dispatcher")) {
        StubBackend::Handle h;
        StubBackend::Handle* hs[1] = {&h};
        kx::dispatch::Core<StubBackend> core(hs, 1, 8, 0);
        const kx_join ok = {5u, 10, 85, 1}, plain = {0u, 0, 0, 0}, most = {7u, 1000, 5000, 12};
        const kx_join bit8 = {8u, 0, 0, 0}, keep_neg = {1u, -1, 0, 0}, keep_big = {1u, 1001, 0, 0}, pause_neg = {0u, 0, -1, 0},
                      pause_big = {0u, 0, 5001, 0}, fade_neg = {1u, 0, 0, -1}, fade_big = {1u, 0, 0, 13};
        dispatcher_case(core, "null_join", nullptr, false, false);
        dispatcher_case(core, "flag_bit_8", &bit8, false, false);
        dispatcher_case(core, "keep_minus_1", &keep_neg, false, false);
        dispatcher_case(core, "keep_1001", &keep_big, false, false);
        dispatcher_case(core, "pause_minus_1", &pause_neg, false, false);
        dispatcher_case(core, "pause_5001", &pause_big, false, false);
        dispatcher_case(core, "fade_minus_1", &fade_neg, false, false);
        dispatcher_case(core, "fade_13", &fade_big, false, false);
        dispatcher_case(core, "only_out_marks", &ok, true, false);
        dispatcher_case(core, "only_out_n_marks", &ok, false, true);
        dispatcher_case(core, "ok_no_marks", &ok, false, false);
        dispatcher_case(core, "ok_marks", &most, true, true);
        dispatcher_case(core, "ok_plain_spec", &plain, true, true);
        return 0;
    }
    fprintf(stderr, "usage: join_plan_check plans|refusals|dispatcher\n");
    return 2;
}
