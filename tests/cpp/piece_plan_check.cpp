// CPU driver of the piece layout (kokorox_amd/csrc/host_request.cpp: build_output_plan with pieces, output_bounds,
// check_piece_call; host_request.h: piece_refusal, piece_emitted): built with g++ -fsanitize=address,undefined together with
// host_request.cpp by tests/test_pieces_cpu.py and run as a child process.  It prints what the unit under test lays out, and the
// test compares that with the numpy definition (kokorox_amd/voices.py: piece_ranges, piece_lengths, joined_marks).
//
//   piece_plan_check plans < cases      every case of the input, one after the other (see run_case), printed as
//       case <name>
//       req <r> <out_off> <out_bytes> <n_samples> <src_samples> <form> <rate> <y_off> <n_marks>
//       piece <r> <emit_lo> <emit_hi> <src_before> <src_end> <n_tail_in> <n_tail_out> <carry_off> <chunks_end> <flags>
//       marks <r> <values ...>          (from the rows of the mark plan, with token_marks_joined_kernel's arithmetic)
//       sizes <total_bytes> <end_bytes> <y_floats> <carry_off> <tail floats> <bound of the packed bytes> <bound of the resampled floats>
//     (one thing it judges itself, in every case: the same rows, grouping, words, joins and want flags with no flags at all and
//     with every flag word PIECE_WHOLE give equal plans, field for field, and neither has a piece table)
//   piece_plan_check refusals           one line per refusal: <name> TAB <code> TAB <message>, or <name> TAB accepted
//   piece_plan_check dispatcher         the same for kx::dispatch::Core::submit_request_piece on a stub model, which hands back
//                                       the flags, the chunk base and the carry every piece reached its batch with
//   piece_plan_check tail               for every rate and every residue of A modulo 4 M (A a multiple of 24 up to 24 x 4 M x 8):
//                                       tail <rate> <worst A - (first source index an output still to come reads)> <KX_PIECE_TAIL>
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
bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(T)));
}

// A layout without flags (what every entry but the piece entry builds, and what build_output_plan built before it knew pieces) and
// the same layout with every flag word PIECE_WHOLE: equal plans, field for field.
void whole_flags_equal_no_flags(const std::vector<int>& frames, const std::vector<int>& lens, const std::vector<int>& edges,
                                const kx::RequestLayout& lay) {
    const int B = (int)frames.size();
    const std::vector<uint32_t> whole((size_t)lay.R, kx::PIECE_WHOLE);
    kx::RequestLayout none = lay, all = lay;
    none.piece_flags = nullptr, none.carry_in = nullptr;
    all.piece_flags = whole.data(), all.carry_in = nullptr;
    kx::OutputPlan a, b;
    kx::build_output_plan(frames.data(), lens.data(), edges.data(), B, none, a);
    kx::build_output_plan(frames.data(), lens.data(), edges.data(), B, all, b);
    REQUIRE_SAME(!a.has_pieces() && !b.has_pieces() && a.carry_off == 0 && b.carry_off == 0 && a.tail_in.empty() && b.tail_in.empty());
    REQUIRE_SAME(a.req.size() == (size_t)lay.R && b.req.size() == (size_t)lay.R);
    for (int r = 0; r < lay.R; ++r) {
        const kx::PackReq &p = a.req[(size_t)r], &q = b.req[(size_t)r];
        REQUIRE_SAME(p.first_row == q.first_row && p.n_rows == q.n_rows && p.form == q.form && p.rate == q.rate);
        REQUIRE_SAME(p.out_off == q.out_off && p.out_bytes == q.out_bytes && p.n_samples == q.n_samples);
        REQUIRE_SAME(p.src_samples == q.src_samples && p.y_off == q.y_off);
        // (and the sizes are those of the whole request, as pack_request_bytes and resampled_samples give them)
        REQUIRE_SAME(p.n_samples == kx::resampled_samples(p.rate, p.src_samples));
        REQUIRE_SAME(p.out_bytes == kx::pack_request_bytes(lay.formats[lay.n_format == 1 ? 0 : r], p.src_samples));
    }
    for (int i = 0; i < B; ++i) {
        const kx::JoinRow &j = a.join[(size_t)i], &k = b.join[(size_t)i];
        REQUIRE_SAME(k.skip == j.skip && k.keep == j.keep && k.gap == j.gap && k.fade_head == j.fade_head && k.fade_tail == j.fade_tail);
        const kx::MarkRow &m = a.mark[(size_t)i], &n = b.mark[(size_t)i];
        REQUIRE_SAME(m.first == n.first && m.base == n.base && m.K == n.K && m.src_base == n.src_base && m.skip == n.skip && m.keep == n.keep);
    }
    REQUIRE_SAME(same_bytes(a.cum, b.cum) && same_bytes(a.count, b.count) && same_bytes(a.first, b.first));
    REQUIRE_SAME(a.total_bytes == b.total_bytes && a.max_units == b.max_units && a.y_floats == b.y_floats && a.joined == b.joined);
    REQUIRE_SAME(a.max_resampled == b.max_resampled && a.marks_off == b.marks_off && a.n_marks == b.n_marks);
    REQUIRE_SAME(a.measured == b.measured && a.levelled == b.levelled && a.levels_off == b.levels_off && a.peak_windows == b.peak_windows);
    REQUIRE_SAME(a.end_bytes() == b.end_bytes() && a.end_bytes() == a.report_end() && a.blocks_end() == b.blocks_end());
    const kx::OutputBounds x = kx::output_bounds(none, B, 600, lens.data()), y = kx::output_bounds(all, B, 600, lens.data());
    REQUIRE_SAME(y.packed_bytes >= x.packed_bytes && y.y_floats >= x.y_floats);
}

bool read_ints(std::vector<int>& v, size_t n) {
    v.assign(n, 0);
    for (size_t i = 0; i < n; ++i)
        if (scanf("%d", &v[i]) != 1) return false;
    return true;
}

// the carry a piece that ended at `src` joined samples and `chunks` chunks left, its tail a ramp
kx::PieceCarry carry_of(int word, long src, int chunks) {
    kx::PieceCarry c{};
    const int rate = kx::format_rate(word);
    c.magic = kx::PIECE_MAGIC;
    c.format_word = (uint32_t)word;
    c.src_samples = src;
    c.out_samples = kx::piece_emitted(rate, src, false);
    c.n_tail = rate == 0 ? 0 : (int32_t)(src < kx::PIECE_TAIL ? src : kx::PIECE_TAIL);
    c.reserved = chunks;
    for (int i = 0; i < c.n_tail; ++i) c.tail[i] = 0.5f + (float)i;
    return c;
}

// A case: "name B R", then lens [B], the durations of every row (lens[b] values each), chunks_per_request [R], words [R],
// joins [R][4], want [R], gain-levels on/off (one int), flags [R], and for every request the pair (source samples before,
// chunks before) its carry is built from (read, and ignored, for a first piece too).
bool run_case() {
    char name[64];
    int B, R;
    if (scanf("%63s %d %d", name, &B, &R) != 3) return false;
    std::vector<int> lens, cpr, words, jv, want, levelled, flags, before;
    if (!read_ints(lens, (size_t)B)) return false;
    std::vector<std::vector<int>> dur((size_t)B);
    std::vector<int> frames((size_t)B, 0), edges((size_t)2 * B, 0);
    for (int b = 0; b < B; ++b) {
        if (!read_ints(dur[(size_t)b], (size_t)lens[(size_t)b])) return false;
        for (int d : dur[(size_t)b]) frames[(size_t)b] += d;
        edges[(size_t)2 * b] = dur[(size_t)b].front();
        edges[(size_t)2 * b + 1] = dur[(size_t)b].back();
    }
    if (!read_ints(cpr, (size_t)R) || !read_ints(words, (size_t)R) || !read_ints(jv, (size_t)4 * R) || !read_ints(want, (size_t)R) ||
        !read_ints(levelled, 1) || !read_ints(flags, (size_t)R) || !read_ints(before, (size_t)2 * R))
        return false;
    std::vector<kx::JoinSpec> joins((size_t)R);
    std::vector<uint8_t> want8((size_t)R);
    std::vector<uint32_t> pf((size_t)R);
    std::vector<kx::PieceCarry> carries((size_t)R);
    const std::vector<kx::LevelSpec> levels((size_t)R, kx::LevelSpec{kx::LEVEL_GAIN, 0.5f, 0.0f});
    for (int r = 0; r < R; ++r) {
        joins[(size_t)r] = kx::JoinSpec{(uint32_t)jv[(size_t)4 * r], jv[(size_t)4 * r + 1], jv[(size_t)4 * r + 2], jv[(size_t)4 * r + 3]};
        want8[(size_t)r] = (uint8_t)want[(size_t)r];
        pf[(size_t)r] = (uint32_t)flags[(size_t)r];
        carries[(size_t)r] = carry_of(words[(size_t)r], before[(size_t)2 * r], before[(size_t)2 * r + 1]);
    }
    kx::RequestLayout lay{cpr.data(), R, words.data(), R, want8.data(), joins.data(), R};
    if (levelled[0]) lay.levels = levels.data(), lay.n_level = R;
    whole_flags_equal_no_flags(frames, lens, edges, lay);
    lay.piece_flags = pf.data();
    lay.carry_in = carries.data();
    kx::OutputPlan plan;
    kx::build_output_plan(frames.data(), lens.data(), edges.data(), B, lay, plan);
    printf("case %s\n", name);
    long frames_all = 0, tails = 0;
    for (int b = 0; b < B; ++b) frames_all += frames[(size_t)b];
    for (int r = 0; r < R; ++r) {
        const kx::PackReq& q = plan.req[(size_t)r];
        printf("req %d %ld %ld %ld %ld %d %d %ld %ld\n", r, q.out_off, q.out_bytes, q.n_samples, q.src_samples, q.form, q.rate, q.y_off,
               plan.count[(size_t)r]);
        if (plan.has_pieces()) {
            const kx::PieceRow& p = plan.piece[(size_t)r];
            printf("piece %d %ld %ld %ld %ld %d %d %ld %d %u\n", r, p.emit_lo, p.emit_hi, p.src_before, p.src_end, p.n_tail_in, p.n_tail_out,
                   p.carry_off, p.chunks_end, p.flags);
            // (a carried tail lies in the plan's buffer where the row says, as the carry had it)
            REQUIRE_SAME((p.n_tail_in == 0 || p.tail_in == tails) && p.tail_in + p.n_tail_in <= (long)plan.tail_in.size());
            for (int i = 0; i < p.n_tail_in; ++i) REQUIRE_SAME(plan.tail_in[(size_t)(p.tail_in + i)] == carries[(size_t)r].tail[i]);
            tails += p.n_tail_in;
        }
        if (!plan.count[(size_t)r]) continue;
        printf("marks %d", r);
        for (int b = q.first_row; b < q.first_row + q.n_rows; ++b) {
            const kx::MarkRow& m = plan.mark[(size_t)b];
            long scan = 0;
            for (int t = 0; t <= lens[(size_t)b]; ++t) {
                long u = 600 * scan - m.skip;
                u = u < 0 ? 0 : (u > m.keep ? m.keep : u);
                printf(" %ld", (m.src_base + u) * m.K / 600);
                REQUIRE_SAME(plan.joined || (m.src_base + u) * m.K / 600 == m.base + m.K * scan);  // (the plain kernel's form of the same value)
                if (t < lens[(size_t)b]) scan += dur[(size_t)b][(size_t)t];
            }
        }
        printf("\n");
    }
    REQUIRE_SAME((long)plan.tail_in.size() == tails);
    const kx::OutputBounds bound = kx::output_bounds(lay, B, (size_t)600 * (size_t)frames_all, lens.data());
    printf("sizes %ld %ld %ld %ld %zu %zu %zu\n", plan.total_bytes, plan.end_bytes(), plan.y_floats, plan.carry_off, plan.tail_in.size(),
           bound.packed_bytes, bound.y_floats);
    return true;
}

// One request of two rows, 3 frames each, as a piece with these flags, word, level, loudness, limit and carry.
void refusal(const char* name, bool through_entry, const uint32_t* flags, int word, const kx::LevelSpec* level, const kx::LoudSpec* loud,
             const kx::LimitSpec* limit, const kx::PieceCarry* carry, bool carry_out = true) {
    const int cpr[1] = {2}, words[1] = {word}, frames[2] = {3, 3}, lens[2] = {1, 1};
    kx::PieceCarry out{};
    try {
        if (through_entry) {
            kx::HostCall hc;
            hc.chunks_per_request = cpr, hc.n_requests = 1, hc.req_formats = words, hc.n_req_formats = 1;
            if (level) hc.levels = {true, level, 1};
            if (loud) hc.loudness = {true, loud, 1};
            if (limit) hc.limits = {true, limit, 1};
            hc.piece_call = true, hc.piece_flags = flags, hc.carry_in = carry, hc.carry_out = carry_out ? &out : nullptr;
            kx::check_piece_call(hc);
        } else {
            kx::RequestLayout lay{cpr, 1, words, 1, nullptr, nullptr, 0, level, level ? 1 : 0, loud, loud ? 1 : 0, limit, limit ? 1 : 0};
            lay.piece_flags = flags, lay.carry_in = carry;
            kx::OutputPlan plan;
            kx::build_output_plan(frames, lens, nullptr, 2, lay, plan);
        }
        printf("%s\taccepted\n", name);
    } catch (const kx::Error& e) {
        printf("%s\t%d\t%s\n", name, e.code, e.what());
    }
}

// A model that runs nothing: every piece gets a body that spells the flags, the chunk base and the carry it arrived with, and
// leaves a carry that counts its chunks.
struct StubBackend {
    struct Handle {};
    struct Out {};
    static int forward(Handle*, std::vector<kx::dispatch::Request*>& batch, Out&) {
        for (kx::dispatch::Request* r : batch) r->rc = KX_OK;
        return KX_OK;
    }
    static void distribute(std::vector<kx::dispatch::Request*>& batch, Out&) {
        for (kx::dispatch::Request* r : batch) {
            int64_t* p = static_cast<int64_t*>(malloc(6 * sizeof(int64_t)));
            p[0] = r->piece_flags, p[1] = r->chunk_base(), p[2] = r->carry_in.src_samples, p[3] = r->carry_in.magic, p[4] = r->levelled ? 1 : 0;
            p[5] = r->piece() ? 1 : 0;
            r->out = p;
            r->out_bytes = 48;
            r->out_samples = 0;
            r->carry_out = kx::PieceCarry{};
            r->carry_out.magic = kx::PIECE_MAGIC;
            r->carry_out.reserved = r->chunk_base() + r->rows();
        }
    }
    static int n_voices(Handle*) { return 0; }
    static int n_vocab(Handle*) { return 178; }
    static void free_out(void* p) { free(p); }
};

void dispatcher_case(kx::dispatch::Core<StubBackend>& core, const char* name, uint32_t flags, int word, const kx_level* level,
                     const kx::PieceCarry* carry, bool carry_out = true) {
    const int64_t ids[5] = {0, 5, 0, 0, 0};
    const int32_t chunk_tokens[2] = {3, 2};
    std::vector<float> styles(2 * KX_STYLE_DIM, 0.f);
    void* out = nullptr;
    int64_t nb = 0, ns = 0;
    double lv[2] = {0, 0};
    kx_piece_carry next;
    memset(&next, 0xEE, sizeof next);
    char err[256] = "";
    const int rc = core.submit_request_piece(ids, chunk_tokens, 2, styles.data(), nullptr, nullptr, 0, 1.f, 1, word, &out, &nb, &ns, nullptr,
                                             nullptr, nullptr, level, level ? lv : nullptr, flags, reinterpret_cast<const kx_piece_carry*>(carry),
                                             carry_out ? &next : nullptr, err, sizeof err);
    if (rc != KX_OK) {
        printf("%s\t%d\t%s\n", name, rc, err);
        return;
    }
    const int64_t* p = static_cast<const int64_t*>(out);
    printf("%s\taccepted\tflags=%ld base=%ld src=%ld magic=%ld levelled=%ld piece=%ld next_chunks=%d\n", name, (long)p[0], (long)p[1], (long)p[2],
           (long)p[3], (long)p[4], (long)p[5], next.reserved);
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
        const uint32_t first[1] = {1u}, middle[1] = {0u}, last[1] = {2u}, whole[1] = {3u}, four[1] = {4u};
        const kx::LevelSpec gain{kx::LEVEL_GAIN, 0.5f, 0.0f}, norm{kx::LEVEL_NORMALIZE, 1.0f, 0.5f}, ceil{kx::LEVEL_CEILING, 2.0f, 0.5f},
            gain_tp{kx::LEVEL_GAIN | kx::PEAK_TRUE, 0.5f, 0.0f};
        const kx::LoudSpec meter{kx::LOUD_MEASURE, 0.0f, 0.0f}, no_loud{kx::LOUD_NONE, 0.0f, 0.0f};
        const kx::LimitSpec lim{kx::LIMIT_GAIN, 1.0f, 0.0f, 0.5f}, no_lim{kx::LIMIT_NONE, 1.0f, 0.0f, 1.0f};
        const kx::PieceCarry good = carry_of(0x108, 2400, 2);
        for (int entry = 0; entry < 2; ++entry) {
            const std::string who = entry ? "entry_" : "plan_";
            auto run = [&](const char* name, const uint32_t* flags, int word, const kx::LevelSpec* lv, const kx::LoudSpec* ld,
                           const kx::LimitSpec* lm, const kx::PieceCarry* c) { refusal((who + name).c_str(), entry != 0, flags, word, lv, ld, lm, c); };
            run("level_normalize", first, 0x108, &norm, nullptr, nullptr, nullptr);
            run("level_ceiling", first, 0x108, &ceil, nullptr, nullptr, nullptr);
            run("level_true_peak", first, 0x108, &gain_tp, nullptr, nullptr, nullptr);
            run("loudness", first, 0x108, nullptr, &meter, nullptr, nullptr);
            run("limiter", first, 0x108, nullptr, nullptr, &lim, nullptr);
            run("form_4", first, 0x104, nullptr, nullptr, nullptr, nullptr);
            run("form_12", first, 0x10C, nullptr, nullptr, nullptr, nullptr);
            run("form_17", first, 0x111, nullptr, nullptr, nullptr, nullptr);
            run("form_18", last, 0x012, nullptr, nullptr, nullptr, &good);
            run("flags_0_without_carry", middle, 0x108, nullptr, nullptr, nullptr, nullptr);
            run("flags_4", four, 0x108, nullptr, nullptr, nullptr, &good);
            kx::PieceCarry c = good;
            c.magic ^= 1u;
            run("carry_magic", middle, 0x108, nullptr, nullptr, nullptr, &c);
            c = good, c.format_word = 0x208;
            run("carry_other_word", middle, 0x108, nullptr, nullptr, nullptr, &c);
            c = good, c.n_tail = kx::PIECE_TAIL + 1;
            run("carry_n_tail_257", last, 0x108, nullptr, nullptr, nullptr, &c);
            c = good, c.n_tail = -1;
            run("carry_n_tail_minus_1", last, 0x108, nullptr, nullptr, nullptr, &c);
            c = good, c.n_tail = 255;
            run("carry_n_tail_short", last, 0x108, nullptr, nullptr, nullptr, &c);
            c = good, c.out_samples += 4;
            run("carry_out_samples", middle, 0x108, nullptr, nullptr, nullptr, &c);
            c = good, c.src_samples = -24;
            run("carry_src_negative", middle, 0x108, nullptr, nullptr, nullptr, &c);
            c = good, c.src_samples = 2401;
            run("carry_src_odd", middle, 0x108, nullptr, nullptr, nullptr, &c);
            c = good, c.reserved = 0;
            run("carry_no_chunks", middle, 0x108, nullptr, nullptr, nullptr, &c);
            // what is accepted: every allowed form, a gain, the sentinels of a batch, a whole request with anything
            run("ok_first_mulaw_gain", first, 0x108, &gain, &no_loud, &no_lim, nullptr);
            run("ok_middle", middle, 0x108, &gain, nullptr, nullptr, &good);
            run("ok_last", last, 0x108, nullptr, nullptr, nullptr, &good);
            run("ok_first_ignores_a_bad_carry", first, 0x108, nullptr, nullptr, nullptr, &c);
            run("ok_whole_normalize_flac", whole, 0x10C, &norm, nullptr, nullptr, nullptr);
            run("ok_whole_loudness", whole, 0x104, nullptr, &meter, nullptr, nullptr);
            const int forms[6] = {0, 1, 2, 3, 8, 9};
            for (int f : forms)
                for (int rate = 0; rate < 4; ++rate) {
                    const kx::PieceCarry cf = carry_of(f | rate << 8, 2400, 1);
                    run(("ok_form_" + std::to_string(f) + "_rate_" + std::to_string(rate)).c_str(), middle, f | rate << 8, nullptr, nullptr, nullptr, &cf);
                }
        }
        refusal("entry_null_flags", true, nullptr, 0x108, nullptr, nullptr, nullptr, nullptr);
        refusal("entry_null_carry_out", true, first, 0x108, nullptr, nullptr, nullptr, nullptr, false);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "dispatcher")) {
        StubBackend::Handle h;
        StubBackend::Handle* hs[1] = {&h};
        kx::dispatch::Core<StubBackend> core(hs, 1, 8, 0);
        const kx_level gain = {KX_LEVEL_GAIN, 0.5f, 0.0f}, norm = {KX_LEVEL_NORMALIZE, 1.0f, 0.5f}, bad = {7u, 1.0f, 0.0f};
        const kx::PieceCarry good = carry_of(0x108, 2400, 3);
        kx::PieceCarry c = good;
        dispatcher_case(core, "ok_first", 1u, 0x108, nullptr, nullptr);
        dispatcher_case(core, "ok_first_ignores_carry", 1u, 0x108, &gain, &good);
        dispatcher_case(core, "ok_middle", 0u, 0x108, &gain, &good);
        dispatcher_case(core, "ok_last", 2u, 0x108, nullptr, &good);
        dispatcher_case(core, "ok_whole", 3u, 0x10C, &norm, nullptr);
        dispatcher_case(core, "null_carry_out", 1u, 0x108, nullptr, nullptr, false);
        dispatcher_case(core, "flags_4", 4u, 0x108, nullptr, &good);
        dispatcher_case(core, "middle_without_carry", 0u, 0x108, nullptr, nullptr);
        dispatcher_case(core, "level_normalize", 1u, 0x108, &norm, nullptr);
        dispatcher_case(core, "bad_level", 1u, 0x108, &bad, nullptr);
        dispatcher_case(core, "form_12", 1u, 0x10C, nullptr, nullptr);
        dispatcher_case(core, "form_4", 2u, 0x004, nullptr, &good);
        c.magic = 0;
        dispatcher_case(core, "carry_magic", 2u, 0x108, nullptr, &c);
        c = good, c.format_word = 0x109;
        dispatcher_case(core, "carry_other_word", 2u, 0x108, nullptr, &c);
        c = good, c.n_tail = 300;
        dispatcher_case(core, "carry_n_tail", 2u, 0x108, nullptr, &c);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "tail")) {
        // After a piece that is not the last, outputs n >= E are still to come; the first source index output E reads is
        // ceil((E M - C) / L), clamped to 0.  Every residue of A modulo 4 M, over eight periods, A a multiple of 24 or not.
        for (int rate = 1; rate <= 3; ++rate) {
            const kx::ResampleFilter& f = kx::resample_filter(rate);
            long worst = 0;
            for (long A = 0; A <= 8L * 4 * f.M * 24 + 4096; ++A) {
                const long q = A * f.L - 1 - f.C;
                const long F = q < 0 ? 0 : q / f.M + 1, E = F & ~3L;
                if (A % 24 == 0 && (A * f.L) % f.M == 0) REQUIRE_SAME(E == kx::piece_emitted(rate, A, false) || F > A * f.L / f.M);
                const long a = E * f.M - f.C;
                const long first = a <= 0 ? 0 : (a + f.L - 1) / f.L;
                const long reach = A - first;
                worst = reach > worst ? reach : worst;
                REQUIRE_SAME(first >= A - kx::PIECE_TAIL);
                REQUIRE_SAME(reach <= kx::piece_tail_need(f.L, f.M, f.n_taps));
            }
            printf("tail %d %ld %d %d\n", rate, worst, kx::piece_tail_need(f.L, f.M, f.n_taps), kx::PIECE_TAIL);
        }
        return 0;
    }
    fprintf(stderr, "usage: piece_plan_check plans|refusals|dispatcher|tail\n");
    return 2;
}
