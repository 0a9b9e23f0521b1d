// Sanitizer build of the dispatcher's host logic (kokorox_amd/csrc/dispatcher_core.h) for requests of several chunks, against a
// stub model that understands rows.  Built and run by tests/test_request_sanitize_cpu.py with g++ -fsanitize=thread and
// -fsanitize=address,undefined.  (tests/cpp/host_sanitize.cpp covers the single-utterance submits and the C ABI's guard.)
//
// The reference runs the chunks of a text one after the other through its one `Mutex<Session>` (kokorox/src/tts/koko.rs:947-1191);
// here a request of n chunks is n rows of ONE batched forward.  Checked: every request is answered once with its own bytes, no
// batch exceeds max_batch ROWS, no request is split over forwards (the stub stamps every row with the forward it ran in), a
// max_batch-chunk request behind a stream of small ones completes, an INVALID batch is replayed request by request with all
// chunks, a model that fails twice hands whole requests to the healthy one, bad chunk counts are refused at submit, and the
// dispatcher can be destroyed while multi-chunk requests are queued.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "dispatcher_core.h"

using kx::dispatch::Request;

namespace {

struct StubModel {
    std::mutex mu;
    std::atomic<long> forwards{0};
    std::atomic<long> max_rows{0};
    bool dead = false;  // every forward fails with DEVICE
    int sleep_us = 300;
    int id = 0;
};
struct StubHandle {
    std::unique_ptr<StubModel> m;
};

constexpr float POISON_SPEED = 13.0f;  // passes the submit-time checks, fails any batch it is in
constexpr size_t ROW_BYTES = 24;       // per chunk: 16 bytes of content hash + 8 bytes naming the forward it ran in

uint32_t mix(uint32_t h, uint32_t v) { return (h ^ v) * 16777619u; }

// the content part of chunk c of a request: depends on its ids, the request's seed, the chunk index (its noise stream), the
// voice (the style row of THAT chunk for kind 0) and the format
void chunk_hash(const Request& r, int c, unsigned char* out16) {
    uint32_t h = 2166136261u;
    size_t at = 0;
    for (int k = 0; k < c; ++k) at += (size_t)r.chunk_len(k);
    for (int t = 0; t < r.chunk_len(c); ++t) h = mix(h, (uint32_t)r.ids[at + (size_t)t]);
    h = mix(h, (uint32_t)r.seed);
    h = mix(h, (uint32_t)c + 101u);
    h = mix(h, (uint32_t)r.kind * 31u + (uint32_t)r.format);
    if (r.kind == 0) h = mix(h, (uint32_t)(r.style[(size_t)c * KX_STYLE_DIM] * 1024.f));
    for (int k = 0; k < r.n_mix; ++k) h = mix(h, (uint32_t)r.voice_ids[k] + 7u);
    for (int i = 0; i < 16; ++i) out16[i] = (unsigned char)((h >> ((i & 3) * 8)) + (unsigned)i);
}

struct StubBackend {
    using Handle = StubHandle;
    struct Out {
        std::vector<std::vector<unsigned char>> parts;  // one region per REQUEST
    };
    static int n_voices(StubHandle*) { return 54; }
    static int n_vocab(StubHandle*) { return 178; }
    static void free_out(void* p) { free(p); }
    static int forward(StubHandle* h, std::vector<Request*>& batch, Out& o) {
        StubModel& M = *h->m;
        std::unique_lock<std::mutex> lk(M.mu, std::try_to_lock);
        if (!lk.owns_lock()) {
            for (Request* r : batch) {
                r->rc = KX_ERR_STATE;
                r->err = "stub: two forwards on one model at once";
            }
            return KX_ERR_STATE;
        }
        const uint64_t stamp = ((uint64_t)M.id << 48) | (uint64_t)(++M.forwards);
        long rows = 0;
        for (Request* r : batch) rows += r->rows();
        long seen = M.max_rows.load();
        while (rows > seen && !M.max_rows.compare_exchange_weak(seen, rows)) {
        }
        if (M.sleep_us) std::this_thread::sleep_for(std::chrono::microseconds(M.sleep_us));
        int rc = KX_OK;
        std::string err;
        if (M.dead) {
            rc = KX_ERR_DEVICE;
            err = "stub: device failure";
        } else {
            for (Request* r : batch)
                if (r->speed == POISON_SPEED) {
                    rc = KX_ERR_INVALID;
                    err = "stub: poison request";
                }
        }
        o.parts.clear();
        for (Request* r : batch) {
            r->rc = rc;
            r->err = err;
            if (rc != KX_OK) continue;
            o.parts.emplace_back((size_t)r->rows() * ROW_BYTES);
            for (int c = 0; c < r->rows(); ++c) {
                unsigned char* p = o.parts.back().data() + (size_t)c * ROW_BYTES;
                chunk_hash(*r, c, p);
                memcpy(p + 16, &stamp, 8);
            }
        }
        return rc;
    }
    static void distribute(std::vector<Request*>& batch, Out& o) {
        for (size_t i = 0; i < batch.size(); ++i) {  // ONE pointer per request, for its whole region
            Request* r = batch[i];
            const std::vector<unsigned char>& e = o.parts[i];
            r->out = malloc(e.size());
            memcpy(r->out, e.data(), e.size());
            r->out_bytes = (int64_t)e.size();
            r->out_samples = (int64_t)r->rows() * 600;
        }
    }
};

using Core = kx::dispatch::Core<StubBackend>;

int failures = 0;
#define CHECK(cond, ...)                                         \
    do {                                                         \
        if (!(cond)) {                                           \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                        \
            fprintf(stderr, "\n");                               \
            ++failures;                                          \
        }                                                        \
    } while (0)

struct Totals {
    std::atomic<long> ok{0}, invalid{0}, device{0}, state{0}, wrong{0}, split{0}, rows{0};
};

std::atomic<uint64_t> next_seed{1};

// One request of n_chunks chunks (n_chunks = 1: through submit_ex half of the time); compares the bytes chunk by chunk and
// that every chunk ran in the same forward.
int one_request(Core& core, unsigned& rng, int n_chunks, bool poison, Totals& tot) {
    auto rnd = [&] { return rng = rng * 1664525u + 1013904223u, rng >> 8; };
    Request ref;
    std::vector<int32_t> lens((size_t)n_chunks);
    for (int c = 0; c < n_chunks; ++c) {
        lens[(size_t)c] = 2 + (int32_t)(rnd() % 20);
        for (int t = 0; t < lens[(size_t)c]; ++t) ref.ids.push_back((int64_t)(rnd() % 178));
    }
    ref.seed = next_seed++;
    ref.kind = (int)(rnd() % 3);
    const bool single = n_chunks == 1 && (rnd() & 1);
    ref.format = (int)(rnd() % (single ? 3 : 5));
    if (!single) ref.chunk_lens = lens;
    const float speed = poison ? POISON_SPEED : 1.0f;
    std::vector<float> styles((size_t)n_chunks * KX_STYLE_DIM);
    for (int c = 0; c < n_chunks; ++c)
        for (int k = 0; k < KX_STYLE_DIM; ++k) styles[(size_t)c * KX_STYLE_DIM + (size_t)k] = 0.25f * (float)(c + 1);
    int32_t vids[3] = {(int32_t)(rnd() % 54), -1, (int32_t)(rnd() % 54)};
    float w[3] = {0.4f, 0.f, 0.5f};
    const int32_t* vp = nullptr;
    const float* wp = nullptr;
    int n_mix = 0;
    if (ref.kind == 0) {
        ref.style = styles;
    } else if (ref.kind == 1) {
        ref.n_mix = n_mix = 1;
        ref.voice_ids[0] = vids[0];
        vp = vids;
    } else {
        ref.n_mix = n_mix = 3;
        for (int k = 0; k < 3; ++k) ref.voice_ids[k] = vids[k];
        vp = vids;
        wp = w;
    }
    char err[256] = {0};
    void* out = nullptr;
    int64_t nb = 0, ns = 0;
    int rc;
    if (single)
        rc = core.submit_ex(ref.ids.data(), lens[0], ref.kind == 0 ? styles.data() : nullptr, vp, wp, n_mix, speed, ref.seed, ref.format, &out,
                            &nb, &ns, err, sizeof err);
    else
        rc = core.submit_request(ref.ids.data(), lens.data(), n_chunks, ref.kind == 0 ? styles.data() : nullptr, vp, wp, n_mix, speed,
                                 ref.seed, ref.format, &out, &nb, &ns, err, sizeof err);
    if (rc == KX_OK) {
        bool good = nb == (int64_t)((size_t)n_chunks * ROW_BYTES) && ns == (int64_t)n_chunks * 600 && !poison;
        if (good) {
            const unsigned char* p = static_cast<const unsigned char*>(out);
            for (int c = 0; c < n_chunks; ++c) {
                unsigned char e[16];
                chunk_hash(ref, c, e);
                if (memcmp(e, p + (size_t)c * ROW_BYTES, 16) != 0) good = false;
                if (memcmp(p + 16, p + (size_t)c * ROW_BYTES + 16, 8) != 0) ++tot.split;  // a chunk ran in another forward
            }
        }
        if (!good) ++tot.wrong;
        free(out);
        ++tot.ok;
        tot.rows += n_chunks;
    } else if (rc == KX_ERR_INVALID) {
        ++tot.invalid;
        if (!poison || !strstr(err, "poison")) ++tot.wrong;
    } else if (rc == KX_ERR_DEVICE) {
        ++tot.device;
    } else if (rc == KX_ERR_STATE) {
        ++tot.state;
    } else {
        ++tot.wrong;
    }
    return rc;
}

std::vector<StubHandle> make_models(int n) {
    std::vector<StubHandle> hs((size_t)n);
    for (int i = 0; i < n; ++i) {
        hs[(size_t)i].m.reset(new StubModel);
        hs[(size_t)i].m->id = i + 1;
    }
    return hs;
}

void scenario_mixed_load() {
    // 64 clients, every other request a single row, the others 2 .. max_batch chunks, one request in 23 poisoned
    constexpr int MAXB = 12, CLIENTS = 64, PER = 24;
    std::vector<StubHandle> hs = make_models(3);
    StubHandle* ptr[3] = {&hs[0], &hs[1], &hs[2]};
    Totals tot;
    long poisoned = 0;
    for (int k = 0; k < CLIENTS * PER; ++k) poisoned += k % 23 == 0;
    {
        Core core(ptr, 3, MAXB, 500);
        std::vector<std::thread> th;
        for (int c = 0; c < CLIENTS; ++c)
            th.emplace_back([&, c] {
                unsigned rng = 4321u + (unsigned)c * 977u;
                for (int i = 0; i < PER; ++i) {
                    const int n = (i & 1) ? 1 : 2 + (int)((rng >> 9) % (MAXB - 1));
                    one_request(core, rng, n, (c * PER + i) % 23 == 0, tot);
                }
            });
        for (auto& t : th) t.join();
        std::lock_guard<std::mutex> lk(core.mu);
        CHECK(core.n_requests >= CLIENTS * PER, "n_requests %ld counts requests", (long)core.n_requests);
        CHECK(core.max_seen_batch > 1 && core.max_seen_batch <= MAXB, "max_batch_seen %ld rows (limit %d)", (long)core.max_seen_batch, MAXB);
        CHECK(core.n_replayed > 0, "no batch was replayed request by request");
        CHECK(core.queued_rows == 0 && core.queue.empty(), "queued rows %ld after the load", core.queued_rows);
    }
    long max_rows = 0;
    for (auto& h : hs) max_rows = h.m->max_rows > max_rows ? h.m->max_rows.load() : max_rows;
    CHECK(max_rows > 1 && max_rows <= MAXB, "a forward ran %ld rows (limit %d)", max_rows, MAXB);
    CHECK(tot.wrong == 0 && tot.split == 0, "%ld wrong results, %ld split requests", tot.wrong.load(), tot.split.load());
    CHECK(tot.invalid == poisoned && tot.ok == CLIENTS * PER - poisoned, "%ld INVALID for %ld poison requests, %ld ok", tot.invalid.load(), poisoned,
          tot.ok.load());
    CHECK(tot.device == 0 && tot.state == 0, "device %ld state %ld", tot.device.load(), tot.state.load());
}

void scenario_large_request_does_not_starve() {
    // one model, small requests arrive without pause from 16 clients; a request of max_batch chunks joins the queue and must be
    // served: a worker always takes the head of the queue, whatever its share
    constexpr int MAXB = 8;
    std::vector<StubHandle> hs = make_models(1);
    StubHandle* ptr[1] = {&hs[0]};
    Totals tot, big;
    std::atomic<bool> done{false};
    {
        Core core(ptr, 1, MAXB, 100);
        std::vector<std::thread> th;
        for (int c = 0; c < 16; ++c)
            th.emplace_back([&, c] {
                unsigned rng = 11u + (unsigned)c * 131u;
                while (!done) one_request(core, rng, 1 + (int)(rng >> 12) % 2, false, tot);
            });
        std::this_thread::sleep_for(std::chrono::milliseconds(5));
        unsigned rng = 999u;
        for (int i = 0; i < 3; ++i) one_request(core, rng, MAXB, false, big);
        done = true;
        for (auto& t : th) t.join();
    }
    CHECK(big.ok == 3 && big.wrong == 0 && big.split == 0, "large requests: ok %ld wrong %ld split %ld", big.ok.load(), big.wrong.load(), big.split.load());
    CHECK(tot.ok > 0 && tot.wrong == 0 && tot.split == 0, "small requests: ok %ld wrong %ld", tot.ok.load(), tot.wrong.load());
    CHECK(hs[0].m->max_rows <= MAXB, "a forward ran %ld rows", hs[0].m->max_rows.load());
}

void scenario_invalid_replay_isolates_the_bad_request() {
    // 12 multi-chunk requests wait together in front of one model; exactly one is poisoned: the batch fails as a whole, is
    // replayed request by request with all chunks, and only the poisoned one reports INVALID
    std::vector<StubHandle> hs = make_models(1);
    hs[0].m->sleep_us = 2000;
    StubHandle* ptr[1] = {&hs[0]};
    Totals tot;
    long replayed;
    {
        Core core(ptr, 1, 64, 20000);
        std::vector<std::thread> th;
        for (int c = 0; c < 12; ++c)
            th.emplace_back([&, c] {
                unsigned rng = 71u + (unsigned)c * 17u;
                one_request(core, rng, 2 + c % 4, c == 5, tot);
            });
        for (auto& t : th) t.join();
        std::lock_guard<std::mutex> lk(core.mu);
        replayed = (long)core.n_replayed;
    }
    CHECK(tot.invalid == 1 && tot.ok == 11 && tot.wrong == 0 && tot.split == 0, "invalid %ld ok %ld wrong %ld split %ld", tot.invalid.load(),
          tot.ok.load(), tot.wrong.load(), tot.split.load());
    CHECK(replayed >= 2, "replayed %ld requests", replayed);
}

void scenario_failed_model_requeues_whole_requests() {
    std::vector<StubHandle> hs = make_models(2);
    hs[0].m->dead = true;
    StubHandle* ptr[2] = {&hs[0], &hs[1]};
    Totals tot;
    {
        Core core(ptr, 2, 8, 300);
        std::vector<std::thread> th;
        for (int c = 0; c < 32; ++c)
            th.emplace_back([&, c] {
                unsigned rng = 555u + (unsigned)c * 29u;
                for (int i = 0; i < 10; ++i) one_request(core, rng, 1 + (int)((rng >> 10) % 8), false, tot);
            });
        for (auto& t : th) t.join();
        std::lock_guard<std::mutex> lk(core.mu);
        CHECK(core.failed[0] == 1 && core.failed[1] == 0, "health %d %d", core.failed[0], core.failed[1]);
        CHECK(core.n_model_failures == 1 && core.n_requeued > 0 && core.n_retried == 1, "failures %ld requeued %ld retried %ld",
              (long)core.n_model_failures, (long)core.n_requeued, (long)core.n_retried);
        CHECK(core.queued_rows == 0, "queued rows %ld", core.queued_rows);
    }
    CHECK(hs[0].m->forwards == 2, "%ld forwards on the failed model (its one batch, tried twice)", hs[0].m->forwards.load());
    CHECK(tot.ok == 320 && tot.wrong == 0 && tot.split == 0 && tot.device == 0, "ok %ld wrong %ld split %ld device %ld", tot.ok.load(), tot.wrong.load(),
          tot.split.load(), tot.device.load());
    CHECK(hs[1].m->max_rows <= 8, "a forward ran %ld rows", hs[1].m->max_rows.load());
}

void scenario_refused_at_submit() {
    std::vector<StubHandle> hs = make_models(1);
    StubHandle* ptr[1] = {&hs[0]};
    Core core(ptr, 1, 4, 100);
    std::vector<int64_t> ids = {0, 5, 0, 0, 6, 7, 0, 0, 8, 0, 0, 9, 0, 0, 3, 0};
    int32_t lens5[5] = {3, 4, 3, 3, 3};
    std::vector<float> styles(5 * KX_STYLE_DIM, 0.5f);
    char err[256];
    void* out = nullptr;
    int64_t nb = 0, ns = 0;
    auto sub = [&](const int32_t* lens, int n, const float* st, const int32_t* v, const float* w, int n_mix, float speed, int fmt) {
        return core.submit_request(ids.data(), lens, n, st, v, w, n_mix, speed, 1, fmt, &out, &nb, &ns, err, sizeof err);
    };
    int32_t v1[1] = {3}, vbad[1] = {54};
    CHECK(sub(lens5, 0, styles.data(), nullptr, nullptr, 0, 1.f, 0) == KX_ERR_INVALID && strstr(err, "1..4 chunks"), "0 chunks: %s", err);
    CHECK(sub(lens5, 5, styles.data(), nullptr, nullptr, 0, 1.f, 0) == KX_ERR_INVALID && strstr(err, "1..4 chunks"), "max_batch + 1 chunks: %s", err);
    CHECK(sub(lens5, 4, styles.data(), nullptr, nullptr, 0, 1.f, 5) == KX_ERR_INVALID, "format 5");
    CHECK(sub(lens5, 4, styles.data(), nullptr, nullptr, 0, 1.f, -1) == KX_ERR_INVALID, "format -1");
    CHECK(sub(lens5, 4, styles.data(), nullptr, nullptr, 0, 0.f, 0) == KX_ERR_INVALID, "speed 0");
    CHECK(sub(lens5, 4, styles.data(), v1, nullptr, 1, 1.f, 0) == KX_ERR_INVALID, "rows and voices");
    CHECK(sub(lens5, 4, nullptr, nullptr, nullptr, 0, 1.f, 0) == KX_ERR_INVALID, "neither rows nor voices");
    CHECK(sub(lens5, 4, nullptr, vbad, nullptr, 1, 1.f, 0) == KX_ERR_INVALID && strstr(err, "voice id 54"), "voice id: %s", err);
    CHECK(sub(lens5, 4, nullptr, v1, nullptr, 2, 1.f, 0) == KX_ERR_INVALID, "two ids without weights");
    int32_t zero_len[2] = {3, 0}, one_len[2] = {3, 1}, long_len[2] = {3, 513};
    CHECK(sub(zero_len, 2, styles.data(), nullptr, nullptr, 0, 1.f, 0) == KX_ERR_INVALID && strstr(err, "chunk 1"), "empty chunk: %s", err);
    CHECK(sub(one_len, 2, nullptr, v1, nullptr, 1, 1.f, 0) == KX_ERR_INVALID, "a voice on a one-token chunk");
    CHECK(sub(long_len, 2, styles.data(), nullptr, nullptr, 0, 1.f, 0) == KX_ERR_INVALID, "513 tokens");
    std::vector<int64_t> keep = ids;
    ids[5] = 178;  // in the second chunk
    CHECK(sub(lens5, 2, styles.data(), nullptr, nullptr, 0, 1.f, 0) == KX_ERR_INVALID && strstr(err, "0..177"), "token id: %s", err);
    ids = keep;
    CHECK(core.submit_request(ids.data(), lens5, 4, styles.data(), nullptr, nullptr, 0, 1.f, 1, 4, nullptr, &nb, &ns, err, sizeof err) == KX_ERR_INVALID,
          "null out");
    CHECK(sub(lens5, 4, nullptr, v1, nullptr, 1, 1.f, 4) == KX_OK && nb == 4 * (int64_t)ROW_BYTES && ns == 2400, "a valid request: %s", err);
    free(out);
    std::lock_guard<std::mutex> lk(core.mu);
    CHECK(core.n_requests == 1 && core.max_seen_batch == 4, "refused requests reached a batch: %ld requests, %ld rows", (long)core.n_requests,
          (long)core.max_seen_batch);
}

void scenario_destroy_while_queued() {
    for (int round = 0; round < 4; ++round) {
        std::vector<StubHandle> hs = make_models(1);
        hs[0].m->sleep_us = 1500;
        StubHandle* ptr[1] = {&hs[0]};
        Totals tot;
        Core* core = new Core(ptr, 1, 6, 0);
        std::vector<std::thread> th;
        for (int c = 0; c < 48; ++c)
            th.emplace_back([&, c] {
                unsigned rng = 5u + (unsigned)c * 31u + (unsigned)round;
                one_request(*core, rng, 1 + c % 6, false, tot);
            });
        for (;;) {  // until every client is inside submit() or already back from it
            const long back = tot.ok + tot.invalid + tot.device + tot.state;
            std::unique_lock<std::mutex> lk(core->mu);
            if (core->inside + back >= 48) break;
            lk.unlock();
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
        delete core;  // = kx_dispatcher_destroy: what is queued is still served, whole
        for (auto& t : th) t.join();
        CHECK(tot.ok + tot.state == 48 && tot.wrong == 0 && tot.split == 0, "round %d: ok %ld state %ld wrong %ld split %ld", round, tot.ok.load(),
              tot.state.load(), tot.wrong.load(), tot.split.load());
        CHECK(hs[0].m->max_rows <= 6, "a forward ran %ld rows", hs[0].m->max_rows.load());
    }
}

}  // namespace

int main() {
    scenario_refused_at_submit();
    scenario_mixed_load();
    scenario_large_request_does_not_starve();
    scenario_invalid_replay_isolates_the_bad_request();
    scenario_failed_model_requeues_whole_requests();
    scenario_destroy_while_queued();
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("request scenarios passed\n");
    return 0;
}
