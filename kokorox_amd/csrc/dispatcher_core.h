// Request dispatcher, host logic only (queue, workers, shares, validation, error policy); HIP-free.  dispatcher.hip
// instantiates it on kx::Model, the CPU suite's sanitizer build on a stub backend (tests/cpp/host_sanitize.cpp, built with
// g++ -fsanitize=thread and -fsanitize=address).
//
// The reference serves every request through one `Mutex<Session>` (kokorox/src/onn/ort_koko.rs:78; callers
// kokorox-openai/src/lib.rs:370-439, kokorox-websocket/src/lib.rs:657-668): N clients = N sequential runs.
// Here any number of OS threads call submit*(); worker threads of each model (= each GPU) take requests off ONE shared
// queue and run them as one batched forward:
//   * a worker whose model is free and that finds work waits at most `max_wait_us` after the oldest request's arrival for
//     company (unless the queue already holds a full batch for every free model), then takes its SHARE of the queue:
//     ceil(queued rows / free models), at most `max_batch` rows.  32 requests waiting in front of 8 idle GPUs become 8 batches of 4, not one batch
//     of 32 on one GPU beside seven idle ones; a single worker that frees up while the others are busy takes up to a
//     whole batch (the reference's config 5: kokorox-openai, 32 clients over 8 GPUs).
//   * a request names its voice either as the 256-float style row (what `mix_styles` returns, koko.rs:1255-1306) or as
//     (voice id, weight) pairs into the device voice table, single voice or mix, and its output form (f32 mono / f32
//     stereo, koko.rs:1239-1246 / PCM16, kokorox-websocket/src/lib.rs:696-736; a request of chunks also the two bodies the
//     servers send, float WAV and base64 of a 16-bit WAV file, G.711 bytes, and any of them at 8, 16 or 48 kHz); requests of
//     every kind, form and rate share one batch.
//   * a request is 1 .. max_batch CHUNKS (the chunk loop of koko.rs:947-1191 as one submit): its chunks are consecutive rows
//     of one forward and its result is one region.  Batches are sized in ROWS; a request is never split over batches or
//     models, and a worker always takes the request at the head of the queue, so a request of max_batch chunks cannot starve
//     behind a stream of small ones.  Replay, retry and re-queue move whole requests.
//   * every request carries its own noise seed, applied per utterance, so a request's bytes are identical whether it
//     ran alone or inside any batch on any of the models.
//   * a request is checked COMPLETELY when it is submitted (token ids, token count, speed, format, voice ids against the
//     smallest voice table of the models, mix size): a bad request is refused there and never reaches a batch, so one
//     client cannot make other clients' batch fail.
//   * if a batch still fails as a whole: an INVALID-class failure is re-run request by request and only the requests that
//     fail alone report it; a DEVICE-class failure (HIP error) is retried ONCE as a batch — never B times on a GPU that may
//     be faulted.  If it fails again the MODEL is marked failed (round 5): its workers stop taking requests, it no longer
//     counts as a free model, and the batch goes back to the head of the queue for the healthy models; a sticky fault on
//     one GPU of eight therefore costs its clients one retry, not a share of all traffic failing twice for ever.  Only when
//     no healthy model is left do requests report the failure (what is queued then, and every later submit).
//     kx_dispatcher_health / kx_dispatcher_failures show the state.
//   * a finished request wakes ITS client only (one condition variable per request, signalled under the queue's mutex):
//     with one shared condition variable every batch woke every waiting client of every model.
//
//   * two worker threads per model alternate, so that the host side of a finished batch (handing every client its bytes,
//     waking it) runs beside the NEXT batch's forward; a worker takes requests only when its model's GPU phase is free,
//     so what arrives during a forward accumulates into the next batch.
//
// Backend contract:
//   using Handle = ...;  using Out = ...;                                 one Handle per model; Out = a finished batch's packed result
//   static int forward(Handle*, std::vector<dispatch::Request*>&, Out&);  the batched forward: fills rc / err of EVERY request
//                                                                         (and Out on success), returns the batch's status
//   static void distribute(std::vector<dispatch::Request*>&, Out&);       gives every request its out / out_bytes / out_samples
//                                                                         (and marks / n_marks where want_marks is set);
//                                                                         Request::join shapes a request's seams;
//                                                                         Request::level sets its level, and a request
//                                                                         with `levelled` set gets level_out = {f64(p), g}
//   static int n_voices(Handle*);                                         rows of the model's voice table (0 = none)
//   static int n_vocab(Handle*);                                          rows of its embedding tables (token ids are 0 .. n_vocab - 1)
//   static void free_out(void*);                                          releases a request's `out` (what distribute handed out)
#pragma once
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/kokorox_hip.h"
#include "host_request.h"

namespace kx {
namespace dispatch {

constexpr int MAX_MIX = 16;

struct Request {
    std::vector<int64_t> ids;  // the chunks' ids back to back
    // tokens of each chunk; empty = ONE chunk of ids.size() tokens (the single-utterance submits)
    std::vector<int32_t> chunk_lens;
    int rows() const { return chunk_lens.empty() ? 1 : (int)chunk_lens.size(); }
    int chunk_len(int c) const { return chunk_lens.empty() ? (int)ids.size() : (int)chunk_lens[(size_t)c]; }
    int kind = 0;  // 0 = style rows, 1 = single voice, 2 = mix
    std::vector<float> style;  // kind 0: rows() x 256 floats, one row per chunk
    int32_t voice_ids[MAX_MIX];
    float weights[MAX_MIX];
    int n_mix = 0;
    int format = 0;
    float speed = 1.f;
    uint64_t seed = 0;
    kx_join join = {0, 0, 0, 0};  // how its seams are shaped (submit_request_joined); all zeros = the chunks appended
    bool joined() const { return join.flags || join.keep_ms || join.pause_ms || join.fade_ms; }
    kx_level level = {KX_LEVEL_GAIN, 1.0f, 0.0f};  // its level spec (submit_request_levelled); the plain spec = the samples as they are
    bool levelled = false;    // it came through the levelled entry: it is measured, whatever its spec
    kx_loudness loudness = {KX_LOUDNESS_MEASURE, 0.0f, 0.0f};  // its loudness spec (submit_request_loudness)
    bool metered = false;     // it came through the loudness entry: its loudness is measured, whatever its spec
    double loud_out[4] = {0.0, 1.0, 0.0, 0.0};  // metered: f64(p), g, I and n_g of the request, as the GPU computed them
    kx_limit limit = {KX_LIMIT_GAIN, 1.0f, 0.0f, 1.0f};  // its limit spec (submit_request_limited)
    bool limited = false;     // it came through the limiter's entry: its body is driven and limited by `limit`
    double limit_out[5] = {0.0, 1.0, 0.0, 0.0, 1.0};  // limited: f64(p), g, I, n_g and r of the request, as the GPU computed them
    bool want_marks = false;  // the token marks of the request beside its body (submit_request_marks); a batch may mix both kinds
    // a piece of a request (submit_request_piece; include/kokorox_hip.h, "pieces"): its flags, the carry it came with and the one it
    // leaves.  PIECE_WHOLE = a request run whole, as through every other entry; a batch may mix both kinds
    uint32_t piece_flags = PIECE_WHOLE;
    PieceCarry carry_in = {}, carry_out = {};
    bool piece() const { return piece_flags != PIECE_WHOLE; }
    // the index of its first chunk in the whole request: the rows of a later piece draw the noise they draw in the request run whole
    int chunk_base() const { return piece() && !(piece_flags & PIECE_FIRST) ? carry_in.reserved : 0; }
    // its prosody (submit_request_prosody): per token, the chunks back to back as `ids`; an empty vector = that array was not given
    std::vector<float> p_rate, p_pitch, p_energy;
    std::vector<int32_t> p_frames;
    bool want_report = false;  // the prosody report of the request beside its body; a batch may mix both kinds
    // its fit spans (submit_request_fitted): `request` 0, positions over its chunks back to back; empty = none.  A batch may mix both
    // kinds.  fit_out [fit.size()]: what the GPU chose for each span
    std::vector<FitSpan> fit;
    std::vector<FitResult> fit_out;
    // result
    void* out = nullptr;
    int64_t out_bytes = 0, out_samples = 0;
    int64_t* marks = nullptr;  // want_marks: into the allocation of `out`, 8-byte aligned behind the body; released with `out`
    int64_t n_marks = 0;
    float* report = nullptr;   // want_report: into the allocation of `out`, 8-byte aligned behind body and marks; released with `out`
    int64_t n_report = 0;      // tokens of it (four float32 values each)
    double level_out[2] = {0.0, 1.0};  // levelled: f64(p) and g of the request, as the GPU computed them
    int rc = -1;
    std::string err;
    bool done = false;
    std::condition_variable cv;  // signalled (under the core's mutex) when `done` is set: wakes this request's client only
    std::chrono::steady_clock::time_point t_submit;
};

// the public spec structs as their kx:: twins (host_request.h)
inline JoinSpec to_spec(const kx_join& j) { return JoinSpec{j.flags, j.keep_ms, j.pause_ms, j.fade_ms}; }
inline LevelSpec to_spec(const kx_level& l) { return LevelSpec{l.mode, l.gain, l.peak}; }
inline LoudSpec to_spec(const kx_loudness& l) { return LoudSpec{l.mode, l.target_lufs, l.peak}; }
inline LimitSpec to_spec(const kx_limit& l) { return LimitSpec{l.mode, l.gain, l.target_lufs, l.peak}; }
// a spec a submit refuses: one that is out of range, or a null one where the entry is the one that takes it
template <class Pub, class Spec>
bool spec_bad(const Pub* p, bool needed, bool (*ok)(const Spec&)) {
    return p ? !ok(to_spec(*p)) : needed;
}

// What a submit_request* entry takes beyond the arguments they all have (Core::submit_request_any).  A null spec: the request has
// no such option -- unless the entry is the one named for it (need_*), which refuses a null spec as it refuses a bad one.
struct RequestOptions {
    bool want_marks = false;  // the token marks of the request, through the pair
    int64_t** out_marks = nullptr;
    int64_t* out_n_marks = nullptr;
    const kx_join* join = nullptr;
    const kx_level* level = nullptr;
    const kx_loudness* loudness = nullptr;
    const kx_limit* limit = nullptr;
    double *out_level = nullptr, *out_loudness = nullptr, *out_limit = nullptr;  // [2], [4], [5]: each may be null
    const kx_prosody* prosody = nullptr;  // (the prosody entry: never null, a request without arrays has the neutral one)
    float** out_report = nullptr;  // the report pair: both or neither
    int64_t* out_n_report = nullptr;
    const kx_fit_span* spans = nullptr;  // the fit entry: the request's spans (n_spans == 0: none) and where their results go (may be null)
    int n_spans = 0;
    kx_fit_result* out_fit = nullptr;
    // the piece entry: the flag word, the carry before (null with KX_PIECE_FIRST) and where the carry goes
    bool need_piece = false;
    uint32_t piece_flags = PIECE_WHOLE;
    const kx_piece_carry* carry_in = nullptr;
    kx_piece_carry* carry_out = nullptr;
    bool need_join = false, need_level = false, need_loudness = false, need_limit = false;
    // the entries behind the marks entry: either argument of the pair asks for marks, and then both must be there
    void set_marks(int64_t** marks, int64_t* n_marks) {
        want_marks = marks || n_marks;
        out_marks = marks;
        out_n_marks = n_marks;
    }
};

template <class Backend>
struct Core {
    using Handle = typename Backend::Handle;
    std::vector<Handle*> models;
    int max_batch = 64;
    int max_wait_us = 2000;
    std::mutex mu;
    std::condition_variable cv_work, cv_quiet;
    std::deque<Request*> queue;
    long queued_rows = 0;  // rows (chunks) of the requests in `queue`: what shares and batch sizes are counted in
    bool stop = false;
    static constexpr int WORKERS_PER_MODEL = 2;
    std::vector<char> busy;  // per model: a forward is running (its GPU phase); 0 = a worker may start the next batch
    std::vector<char> failed;  // per model: a batch failed with DEVICE twice in a row: the model takes no more work
    int64_t n_model_failures = 0, n_requeued = 0;
    int inside = 0;  // client threads inside submit() (shutdown waits for them before the object goes away)
    std::vector<std::thread> workers;
    int64_t n_requests = 0, n_batches = 0, max_seen_batch = 0, n_replayed = 0, n_retried = 0;
    std::vector<int64_t> per_model_batches;

    Core(Handle** ms, int n, int max_b, int wait_us) : models(ms, ms + n), max_batch(max_b), max_wait_us(wait_us) {
        per_model_batches.assign((size_t)n, 0);
        busy.assign((size_t)n, 0);
        failed.assign((size_t)n, 0);
        for (int i = 0; i < n * WORKERS_PER_MODEL; ++i) workers.emplace_back([this, i] { worker(i); });
    }
    Core(const Core&) = delete;
    Core& operator=(const Core&) = delete;

    // Queued requests are still served; submit() calls that arrive from now on are refused; returns when the workers have
    // drained the queue and every client thread has left submit().
    void shutdown() {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
        }
        cv_work.notify_all();
        for (std::thread& t : workers)
            if (t.joinable()) t.join();
        std::unique_lock<std::mutex> lk(mu);
        cv_quiet.wait(lk, [&] { return inside == 0; });
    }
    ~Core() { shutdown(); }

    // Two workers per model alternate: while one hands a finished batch's results to its clients (host work: copies, wake-ups),
    // the other already runs the next batch's forward.  `busy[m]` is the model's GPU phase: a worker takes requests off the
    // queue only when its model is free, so requests that arrive during a forward accumulate into the next batch.
    void worker(int wi) {
        const size_t m = (size_t)wi / WORKERS_PER_MODEL;
        Handle* h = models[m];
        for (;;) {
            std::vector<Request*> batch;
            bool more;
            {
                std::unique_lock<std::mutex> lk(mu);
                for (;;) {
                    // (after `stop` the queue is still drained: a worker leaves only when nothing is waiting)
                    cv_work.wait(lk, [&] { return failed[m] || (stop && queue.empty()) || (!queue.empty() && !busy[m]); });
                    if (failed[m]) return;  // (its sibling marked the model failed: nothing more runs on it)
                    if (queue.empty()) return;
                    // work is here and this model is free: give others a short chance to join, unless every free model
                    // already has a full batch waiting
                    bool go = true;
                    while (!stop && !failed[m] && !queue.empty() && !busy[m] && queued_rows < (long)max_batch * free_models()) {
                        const auto deadline = queue.front()->t_submit + std::chrono::microseconds(max_wait_us);
                        const auto now = std::chrono::steady_clock::now();
                        if (now >= deadline) break;
#if defined(__SANITIZE_THREAD__)
                        // gcc 11's ThreadSanitizer does not intercept pthread_cond_clockwait (what a steady-clock wait becomes)
                        // and then reports the mutex as locked twice; a system-clock wait goes through pthread_cond_timedwait
                        cv_work.wait_until(lk, std::chrono::system_clock::now() + (deadline - now));
#else
                        cv_work.wait_until(lk, deadline);
#endif
                    }
                    if (failed[m]) return;
                    if (queue.empty() || busy[m]) go = false;  // (the sibling worker, or another model's, was quicker)
                    if (go) break;
                }
                // this model's share of what is waiting (the other free models' workers wake up on the same notify)
                const long fm = free_models();
                long take = (queued_rows + fm - 1) / fm;
                take = take > max_batch ? max_batch : take;
                // whole requests, in order, while they fit the share; the head of the queue always goes (it has at most
                // max_batch rows: submit checks that), so a large request cannot starve behind small ones
                long rows = 0;
                while (!queue.empty() && (batch.empty() || rows + queue.front()->rows() <= take)) {
                    rows += queue.front()->rows();
                    batch.push_back(queue.front());
                    queue.pop_front();
                }
                queued_rows -= rows;
                busy[m] = true;
                n_batches += 1;
                per_model_batches[m] += 1;
                n_requests += (int64_t)batch.size();
                if ((int64_t)rows > max_seen_batch) max_seen_batch = (int64_t)rows;
                more = !queue.empty();
            }
            if (more) cv_work.notify_all();  // (what is left is for the other free models)
            typename Backend::Out out;
            int rc = forward_retrying(h, batch, out);
            const bool replay = rc == KX_ERR_INVALID && batch.size() > 1;
            if (replay) {
                // per-request isolation (a request with all its chunks): only the requests that fail alone report the failure
                for (Request* r : batch) {
                    std::vector<Request*> one{r};
                    typename Backend::Out o1;
                    if (forward_retrying(h, one, o1) == KX_OK) Backend::distribute(one, o1);
                }
            }
            bool model_failed = false, requeued = false;
            {
                std::lock_guard<std::mutex> lk(mu);
                busy[m] = false;  // the model's GPU phase is over: its other worker may start the next batch
                if (replay) n_replayed += (int64_t)batch.size();
                if (rc == KX_ERR_DEVICE) {
                    // failed, retried, failed again: the model is out.  Its batch goes back to the HEAD of the queue (in order)
                    // for the healthy models; with none left, it and everything queued report the failure.
                    model_failed = true;
                    if (!failed[m]) n_model_failures += 1;
                    failed[m] = 1;
                    if (healthy_models() > 0) {
                        for (auto it = batch.rbegin(); it != batch.rend(); ++it) {
                            queue.push_front(*it);
                            queued_rows += (*it)->rows();
                        }
                        n_requeued += (int64_t)batch.size();
                        requeued = true;
                    } else {
                        for (Request* r : queue) {
                            r->rc = KX_ERR_DEVICE;
                            r->err = "dispatcher: no healthy model is left (" + batch[0]->err + ")";
                            finish(r);
                        }
                        queue.clear();
                        queued_rows = 0;
                    }
                }
            }
            cv_work.notify_all();
            if (rc == KX_OK) Backend::distribute(batch, out);  // host work, beside the next batch's forward
            if (!requeued) {
                std::lock_guard<std::mutex> lk(mu);
                for (Request* r : batch) finish(r);
            }
            if (model_failed) return;
        }
    }

    // (under mu) the request is complete: wake its client.  Signalled while the mutex is held: the client cannot leave submit()
    // -- and destroy the request with its condition variable -- before this thread has let go of the mutex.
    void finish(Request* r) {
        r->done = true;
        r->cv.notify_one();
    }

    long healthy_models() const {  // (under mu)
        long n = 0;
        for (char f : failed) n += f ? 0 : 1;
        return n;
    }
    long free_models() const {  // (under mu) at least 1: the caller's own model is free when this is asked
        long n = 0;
        for (size_t i = 0; i < busy.size(); ++i) n += (busy[i] || failed[i]) ? 0 : 1;
        return n > 0 ? n : 1;
    }

    // One forward; a DEVICE-class failure gets one more try as the same batch; a second failure marks the model failed (worker).
    int forward_retrying(Handle* h, std::vector<Request*>& batch, typename Backend::Out& out) {
        int rc = Backend::forward(h, batch, out);
        if (rc != KX_ERR_DEVICE) return rc;
        rc = Backend::forward(h, batch, out);
        std::lock_guard<std::mutex> lk(mu);
        n_retried += 1;
        return rc;
    }

    // common tail of the submit calls: queue the request, wait for its result
    int submit(Request& r, void** out, int64_t* out_bytes, int64_t* out_samples, char* err, size_t err_len) {
        r.t_submit = std::chrono::steady_clock::now();
        {
            std::unique_lock<std::mutex> lk(mu);
            if (stop) {
                if (err && err_len) snprintf(err, err_len, "dispatcher is shutting down");
                return KX_ERR_STATE;
            }
            if (healthy_models() == 0) {
                if (err && err_len) snprintf(err, err_len, "dispatcher: no healthy model is left (kx_dispatcher_health)");
                return KX_ERR_DEVICE;
            }
            ++inside;
            queue.push_back(&r);
            queued_rows += r.rows();
            cv_work.notify_all();
            r.cv.wait(lk, [&] { return r.done; });
            if (--inside == 0) cv_quiet.notify_all();
        }
        if (r.rc != KX_OK) {
            if (err && err_len) snprintf(err, err_len, "%s", r.err.c_str());
            if (r.out) Backend::free_out(r.out);  // (never set on a failed request today; were it ever, it is not malloc'd memory)
            return r.rc;
        }
        *out = r.out;
        if (out_bytes) *out_bytes = r.out_bytes;
        if (out_samples) *out_samples = r.out_samples;
        return KX_OK;
    }

    // rows of the SMALLEST embedding table among the models: token ids must be valid on whichever model takes the request
    int vocab_everywhere() {
        int n = -1;
        for (Handle* h : models) {
            const int v = Backend::n_vocab(h);
            n = (n < 0 || v < n) ? v : n;
        }
        return n < 0 ? 0 : n;
    }

    // format_word: `format` is the word of the request entries (include/kokorox_hip.h: a form 0..4, 8, 9, 12, 17 or 18 in bits 0..7, a
    // rate code 0..3 in bits 8..11, nothing else); otherwise one of the three forms 0..2 of the single-utterance submits
    bool check_common(const int64_t* ids, int n_tokens, float speed, int format, const char* who, char* err,
                      size_t err_len, bool format_word = false) {
        const int form = format_word ? (format & 0xFF) : format;
        const bool form_ok = format_word ? (format >= 0 && (format & ~0xFFF) == 0 && (form <= KX_PACK_WAV16_BASE64 || form == KX_PACK_MULAW || form == KX_PACK_ALAW || form == KX_PACK_FLAC ||
                                                         form == KX_PACK_ADPCM_WAV || form == KX_PACK_WAV16))
                                         : (format >= 0 && format <= KX_PACK_PCM16_MONO);
        if (!ids || n_tokens < 1 || n_tokens > KX_MAX_TOKENS || !(speed > 0.f) || !form_ok) {
            if (err && err_len)
                snprintf(err, err_len, "%s: bad argument (1..512 tokens, speed > 0, format %s)", who, format_word ? "0..4, 8, 9, 12, 17, 18 | rate code << 8" : "0..2");
            return false;
        }
        if (format_word && ((format >> 8) & 15) > 3) {
            if (err && err_len) snprintf(err, err_len, "%s: unknown output sample rate (rate codes 0..3)", who);
            return false;
        }
        const int nv = vocab_everywhere();  // (from the models' embedding tables: vocab.rs:5-20 has 178 rows, a checkpoint may differ)
        for (int t = 0; t < n_tokens; ++t)
            if (ids[t] < 0 || ids[t] >= nv) {
                if (err && err_len) snprintf(err, err_len, "%s: token id outside 0..%d", who, nv - 1);
                return false;
            }
        return true;
    }

    // rows of the SMALLEST voice table among the models (a request may land on any of them)
    int voices_everywhere() {
        int n = -1;
        for (Handle* h : models) {
            const int v = Backend::n_voices(h);
            n = (n < 0 || v < n) ? v : n;
        }
        return n < 0 ? 0 : n;
    }

    // The voice of a request named into the device voice table, for both submit forms: `voice_ids[n_mix]` with weights = null and
    // n_mix = 1 (a single voice: row copy) or with `weights[n_mix]` (a mix; ids < 0 are skipped parts, koko.rs:1283).  min_tokens
    // = the shortest chunk: the row of a voice is tokens - 2, so the two 0 pads must be there.  Fills r.kind / n_mix / voice_ids /
    // weights; the ids are checked against the voice tables NOW: inside a batch a bad id would fail every request it was batched with.
    bool set_voices(Request& r, const int32_t* voice_ids, const float* weights, int n_mix, int min_tokens, const char* who, char* err,
                    size_t err_len) {
        if (!voice_ids || n_mix < 1 || n_mix > MAX_MIX || min_tokens < 2 || (!weights && n_mix != 1)) {
            if (err && err_len)
                snprintf(err, err_len, "%s: voices need 1..16 ids (one id when weights is null: a single voice) and the two 0 pads "
                                       "among the tokens", who);
            return false;
        }
        const int nv = voices_everywhere();
        bool any = false;
        for (int k = 0; k < n_mix; ++k) {
            if (voice_ids[k] >= nv) {
                if (err && err_len)
                    snprintf(err, err_len, "%s: voice id %d outside the table of %d voices%s", who, (int)voice_ids[k], nv,
                             nv ? "" : " (kx_set_voice_table was not called on every model)");
                return false;
            }
            any = any || voice_ids[k] >= 0;
        }
        if (!any || (!weights && voice_ids[0] < 0)) {
            if (err && err_len) snprintf(err, err_len, "%s: no voice given", who);
            return false;
        }
        r.kind = weights ? 2 : 1;
        r.n_mix = n_mix;
        for (int k = 0; k < n_mix; ++k) {
            r.voice_ids[k] = voice_ids[k];
            r.weights[k] = weights ? weights[k] : 0.f;
        }
        return true;
    }

    int submit_row(const int64_t* ids, int n_tokens, const float* style, float speed, uint64_t seed, float** out,
                   int64_t* out_len, char* err, size_t err_len) {
        if (!style || !out || !out_len) {
            if (err && err_len) snprintf(err, err_len, "dispatcher_submit: bad argument (1..512 tokens, speed > 0)");
            return KX_ERR_INVALID;
        }
        if (!check_common(ids, n_tokens, speed, 0, "dispatcher_submit", err, err_len)) return KX_ERR_INVALID;
        Request r;
        r.ids.assign(ids, ids + n_tokens);
        r.style.assign(style, style + KX_STYLE_DIM);
        r.speed = speed;
        r.seed = seed;
        void* p = nullptr;
        const int rc = submit(r, &p, nullptr, out_len, err, err_len);
        if (rc == KX_OK) *out = static_cast<float*>(p);
        return rc;
    }

    int submit_ex(const int64_t* ids, int n_tokens, const float* style, const int32_t* voice_ids, const float* weights,
                  int n_mix, float speed, uint64_t seed, int format, void** out, int64_t* out_bytes, int64_t* out_samples,
                  char* err, size_t err_len) {
        if (!out || !out_bytes || !out_samples) {
            if (err && err_len) snprintf(err, err_len, "dispatcher_submit_ex: null output argument");
            return KX_ERR_INVALID;
        }
        if (!check_common(ids, n_tokens, speed, format, "dispatcher_submit_ex", err, err_len)) return KX_ERR_INVALID;
        Request r;
        if (style) {
            if (voice_ids) {
                if (err && err_len) snprintf(err, err_len, "dispatcher_submit_ex: give the style row OR voice ids, not both");
                return KX_ERR_INVALID;
            }
            r.kind = 0;
            r.style.assign(style, style + KX_STYLE_DIM);
        } else if (!set_voices(r, voice_ids, weights, n_mix, n_tokens, "dispatcher_submit_ex", err, err_len)) {
            return KX_ERR_INVALID;
        }
        r.ids.assign(ids, ids + n_tokens);
        r.format = format;
        r.speed = speed;
        r.seed = seed;
        return submit(r, out, out_bytes, out_samples, err, err_len);
    }

    // A request of n_chunks chunks: ids = the chunks back to back (chunk c has chunk_tokens[c] ids incl. its two 0 pads);
    // styles = n_chunks rows of 256 floats, or null with ONE voice spec for the whole request as in submit_ex (the row of the
    // voice is chunk_tokens[c] - 2 per chunk, koko.rs:1166); format = a format word.  Every chunk is checked with submit_ex's rules.
    int submit_request(const int64_t* ids, const int32_t* chunk_tokens, int n_chunks, const float* styles,
                       const int32_t* voice_ids, const float* weights, int n_mix, float speed, uint64_t seed, int format,
                       void** out, int64_t* out_bytes, int64_t* out_samples, char* err, size_t err_len) {
        return submit_request_any(ids, chunk_tokens, n_chunks, styles, voice_ids, weights, n_mix, speed, seed, format, out, out_bytes,
                                  out_samples, RequestOptions{}, err, err_len);
    }
    // ... and with the request's token marks: *out_marks points into the allocation of *out
    int submit_request_marks(const int64_t* ids, const int32_t* chunk_tokens, int n_chunks, const float* styles,
                             const int32_t* voice_ids, const float* weights, int n_mix, float speed, uint64_t seed, int format,
                             void** out, int64_t* out_bytes, int64_t* out_samples, int64_t** out_marks, int64_t* out_n_marks,
                             char* err, size_t err_len) {
        RequestOptions o;
        o.set_marks(out_marks, out_n_marks);
        o.want_marks = true;
        return submit_request_any(ids, chunk_tokens, n_chunks, styles, voice_ids, weights, n_mix, speed, seed, format, out, out_bytes,
                                  out_samples, o, err, err_len);
    }
    // ... and with its join spec; both marks arguments null = no marks
    int submit_request_joined(const int64_t* ids, const int32_t* chunk_tokens, int n_chunks, const float* styles,
                              const int32_t* voice_ids, const float* weights, int n_mix, float speed, uint64_t seed, int format,
                              void** out, int64_t* out_bytes, int64_t* out_samples, int64_t** out_marks, int64_t* out_n_marks,
                              const kx_join* join, char* err, size_t err_len) {
        RequestOptions o;
        o.set_marks(out_marks, out_n_marks);
        o.join = join, o.need_join = true;
        return submit_request_any(ids, chunk_tokens, n_chunks, styles, voice_ids, weights, n_mix, speed, seed, format, out, out_bytes,
                                  out_samples, o, err, err_len);
    }
    // ... and with its level spec; `join` may be null here (no join), out_level may be null
    int submit_request_levelled(const int64_t* ids, const int32_t* chunk_tokens, int n_chunks, const float* styles,
                                const int32_t* voice_ids, const float* weights, int n_mix, float speed, uint64_t seed, int format,
                                void** out, int64_t* out_bytes, int64_t* out_samples, int64_t** out_marks, int64_t* out_n_marks,
                                const kx_join* join, const kx_level* level, double* out_level, char* err, size_t err_len) {
        RequestOptions o;
        o.set_marks(out_marks, out_n_marks);
        o.join = join;
        o.level = level, o.out_level = out_level, o.need_level = true;
        return submit_request_any(ids, chunk_tokens, n_chunks, styles, voice_ids, weights, n_mix, speed, seed, format, out, out_bytes,
                                  out_samples, o, err, err_len);
    }
    // ... and with its loudness spec; `join` may be null here (no join), out_loudness may be null
    int submit_request_loudness(const int64_t* ids, const int32_t* chunk_tokens, int n_chunks, const float* styles,
                                const int32_t* voice_ids, const float* weights, int n_mix, float speed, uint64_t seed, int format,
                                void** out, int64_t* out_bytes, int64_t* out_samples, int64_t** out_marks, int64_t* out_n_marks,
                                const kx_join* join, const kx_loudness* loudness, double* out_loudness, char* err, size_t err_len) {
        RequestOptions o;
        o.set_marks(out_marks, out_n_marks);
        o.join = join;
        o.loudness = loudness, o.out_loudness = out_loudness, o.need_loudness = true;
        return submit_request_any(ids, chunk_tokens, n_chunks, styles, voice_ids, weights, n_mix, speed, seed, format, out, out_bytes,
                                  out_samples, o, err, err_len);
    }
    // ... and with its limit spec; `join` may be null here (no join), out_limit may be null
    int submit_request_limited(const int64_t* ids, const int32_t* chunk_tokens, int n_chunks, const float* styles,
                               const int32_t* voice_ids, const float* weights, int n_mix, float speed, uint64_t seed, int format,
                               void** out, int64_t* out_bytes, int64_t* out_samples, int64_t** out_marks, int64_t* out_n_marks,
                               const kx_join* join, const kx_limit* limit, double* out_limit, char* err, size_t err_len) {
        RequestOptions o;
        o.set_marks(out_marks, out_n_marks);
        o.join = join;
        o.limit = limit, o.out_limit = out_limit, o.need_limit = true;
        return submit_request_any(ids, chunk_tokens, n_chunks, styles, voice_ids, weights, n_mix, speed, seed, format, out, out_bytes,
                                  out_samples, o, err, err_len);
    }
    // ... and with its prosody (include/kokorox_hip.h, "prosody") and the report; `join` and `prosody` may be null here
    int submit_request_prosody(const int64_t* ids, const int32_t* chunk_tokens, int n_chunks, const float* styles,
                               const int32_t* voice_ids, const float* weights, int n_mix, float speed, uint64_t seed, int format,
                               void** out, int64_t* out_bytes, int64_t* out_samples, int64_t** out_marks, int64_t* out_n_marks,
                               const kx_join* join, const kx_prosody* prosody, float** out_report, int64_t* out_n_report, char* err,
                               size_t err_len) {
        const kx_prosody neutral = {nullptr, nullptr, nullptr, nullptr};
        RequestOptions o;
        o.set_marks(out_marks, out_n_marks);
        o.join = join;
        o.prosody = prosody ? prosody : &neutral;
        o.out_report = out_report, o.out_n_report = out_n_report;
        return submit_request_any(ids, chunk_tokens, n_chunks, styles, voice_ids, weights, n_mix, speed, seed, format, out, out_bytes,
                                  out_samples, o, err, err_len);
    }
    // ... and with its fit spans (include/kokorox_hip.h, "fit") and their results
    int submit_request_fitted(const int64_t* ids, const int32_t* chunk_tokens, int n_chunks, const float* styles,
                              const int32_t* voice_ids, const float* weights, int n_mix, float speed, uint64_t seed, int format,
                              void** out, int64_t* out_bytes, int64_t* out_samples, int64_t** out_marks, int64_t* out_n_marks,
                              const kx_join* join, const kx_prosody* prosody, float** out_report, int64_t* out_n_report,
                              const kx_fit_span* spans, int n_spans, kx_fit_result* out_fit, char* err, size_t err_len) {
        const kx_prosody neutral = {nullptr, nullptr, nullptr, nullptr};
        RequestOptions o;
        o.set_marks(out_marks, out_n_marks);
        o.join = join;
        o.prosody = prosody ? prosody : &neutral;
        o.out_report = out_report, o.out_n_report = out_n_report;
        o.spans = spans, o.n_spans = n_spans, o.out_fit = out_fit;
        return submit_request_any(ids, chunk_tokens, n_chunks, styles, voice_ids, weights, n_mix, speed, seed, format, out, out_bytes,
                                  out_samples, o, err, err_len);
    }
    // ... and as a piece of a request (include/kokorox_hip.h, "pieces"); `join` and `level` may be null here, out_level may be null
    int submit_request_piece(const int64_t* ids, const int32_t* chunk_tokens, int n_chunks, const float* styles,
                             const int32_t* voice_ids, const float* weights, int n_mix, float speed, uint64_t seed, int format,
                             void** out, int64_t* out_bytes, int64_t* out_samples, int64_t** out_marks, int64_t* out_n_marks,
                             const kx_join* join, const kx_level* level, double* out_level, uint32_t piece_flags,
                             const kx_piece_carry* carry_in, kx_piece_carry* carry_out, char* err, size_t err_len) {
        RequestOptions o;
        o.set_marks(out_marks, out_n_marks);
        o.join = join;
        o.level = level, o.out_level = out_level;
        o.need_piece = true, o.piece_flags = piece_flags, o.carry_in = carry_in, o.carry_out = carry_out;
        return submit_request_any(ids, chunk_tokens, n_chunks, styles, voice_ids, weights, n_mix, speed, seed, format, out, out_bytes,
                                  out_samples, o, err, err_len);
    }
    // The submits above are this one.  The request's options are looked at first, a bad join before a bad level, loudness or limit,
    // then the report pair; the arguments every submit has come after them.
    int submit_request_any(const int64_t* ids, const int32_t* chunk_tokens, int n_chunks, const float* styles,
                           const int32_t* voice_ids, const float* weights, int n_mix, float speed, uint64_t seed, int format,
                           void** out, int64_t* out_bytes, int64_t* out_samples, const RequestOptions& o, char* err, size_t err_len) {
        const char* who = "dispatcher_submit_request";
        // (these texts are written out whole: callers and tests match on them)
        const char* bad = spec_bad(o.join, o.need_join, join_spec_ok)               ? "dispatcher_submit_request: bad join"
                          : spec_bad(o.level, o.need_level, level_spec_ok)          ? "dispatcher_submit_request: bad level"
                          : spec_bad(o.loudness, o.need_loudness, loud_spec_ok)     ? "dispatcher_submit_request: bad loudness"
                          : spec_bad(o.limit, o.need_limit, limit_spec_ok)          ? "dispatcher_submit_request: bad limit"
                          : (o.out_report != nullptr) != (o.out_n_report != nullptr) ? "dispatcher_submit_request: null report argument"
                                                                                     : nullptr;
        auto refuse = [&](const char* fmt, auto... args) {
            if (err && err_len) snprintf(err, err_len, fmt, args...);
            return (int)KX_ERR_INVALID;
        };
        if (bad) return refuse("%s", bad);
        if (o.need_piece) {  // (the model's refusals of a piece, under the dispatcher's name: "infer: ..." becomes "dispatcher_submit_request: ...")
            static_assert(sizeof(kx_piece_carry) == sizeof(PieceCarry), "the layout of host_request.h");
            if (!o.carry_out) return refuse("%s: null piece argument", who);
            const LevelSpec ls = o.level ? to_spec(*o.level) : LevelSpec{LEVEL_GAIN, 1.0f, 0.0f};
            RequestLayout lay{};
            lay.R = 1, lay.formats = &format, lay.n_format = 1;
            lay.levels = &ls, lay.n_level = 1;
            lay.piece_flags = &o.piece_flags;
            lay.carry_in = reinterpret_cast<const PieceCarry*>(o.carry_in);
            if (const char* why = piece_refusal(lay)) return refuse("%s: %s", who, strncmp(why, "infer: ", 7) == 0 ? why + 7 : why);
        }
        if (!out || !out_bytes || !out_samples) return refuse("%s: null output argument", who);
        if (o.want_marks && (!o.out_marks || !o.out_n_marks)) return refuse("%s: null marks argument", who);
        if (!ids || !chunk_tokens || n_chunks < 1 || n_chunks > max_batch) return refuse("%s: a request has 1..%d chunks (max_batch)", who, max_batch);
        if ((styles != nullptr) == (voice_ids != nullptr)) return refuse("%s: give the style rows OR voice ids, not both", who);
        size_t total = 0;
        int min_tokens = KX_MAX_TOKENS;
        for (int c = 0; c < n_chunks; ++c) {
            // (the count first: check_common reads chunk_tokens[c] ids)
            if (chunk_tokens[c] < (voice_ids ? 2 : 1) || chunk_tokens[c] > KX_MAX_TOKENS)
                return refuse("%s: chunk %d: 1..512 tokens (with a voice: at least the two 0 pads)", who, c);
            if (!check_common(ids + total, chunk_tokens[c], speed, format, who, err, err_len, true)) return KX_ERR_INVALID;
            total += (size_t)chunk_tokens[c];
            min_tokens = chunk_tokens[c] < min_tokens ? chunk_tokens[c] : min_tokens;
        }
        Request r;
        if (const kx_prosody* p = o.prosody) {  // (the arrays run over the chunks back to back: one row of `total` tokens as far as the rule goes)
            const ProsodySpec ps{p->rate, p->frames, p->pitch, p->energy};
            const int32_t all = (int32_t)total;
            if (!prosody_ok(&ps, &all, 1, (int64_t)total)) return refuse("%s: bad prosody", who);
            if (p->rate) r.p_rate.assign(p->rate, p->rate + total);
            if (p->frames) r.p_frames.assign(p->frames, p->frames + total);
            if (p->pitch) r.p_pitch.assign(p->pitch, p->pitch + total);
            if (p->energy) r.p_energy.assign(p->energy, p->energy + total);
            r.want_report = o.out_report != nullptr;
        }
        if (o.n_spans != 0) {  // (`request` must be 0: the request is the only one of its call as far as the rule goes)
            static_assert(sizeof(kx_fit_span) == sizeof(FitSpan) && sizeof(kx_fit_result) == sizeof(FitResult), "the layouts of host_request.h");
            FitPlan plan;
            const int32_t one = n_chunks;
            if (!fit_ok(reinterpret_cast<const FitSpan*>(o.spans), o.n_spans, &one, 1, chunk_tokens, n_chunks,
                        o.prosody ? o.prosody->frames : nullptr, 0, plan, true))
                return refuse("%s: bad fit", who);
            r.fit.assign(reinterpret_cast<const FitSpan*>(o.spans), reinterpret_cast<const FitSpan*>(o.spans) + o.n_spans);
        }
        if (styles) {
            r.kind = 0;
            r.style.assign(styles, styles + (size_t)n_chunks * KX_STYLE_DIM);
        } else if (!set_voices(r, voice_ids, weights, n_mix, min_tokens, who, err, err_len)) {
            return KX_ERR_INVALID;
        }
        r.ids.assign(ids, ids + total);
        r.chunk_lens.assign(chunk_tokens, chunk_tokens + n_chunks);
        r.format = format;
        r.speed = speed;
        r.seed = seed;
        r.want_marks = o.want_marks;
        if (o.join) r.join = *o.join;
        if (o.level) {
            r.level = *o.level;
            r.levelled = true;
        }
        if (o.loudness) {
            r.loudness = *o.loudness;
            r.metered = true;
        }
        if (o.limit) {
            r.limit = *o.limit;
            r.limited = true;
        }
        if (o.need_piece) {
            r.piece_flags = o.piece_flags;
            if (r.piece() && !(r.piece_flags & PIECE_FIRST)) r.carry_in = *reinterpret_cast<const PieceCarry*>(o.carry_in);
        }
        const int rc = submit(r, out, out_bytes, out_samples, err, err_len);
        if (rc != KX_OK) return rc;
        if (o.need_piece) memcpy(o.carry_out, &r.carry_out, sizeof(PieceCarry));
        if (o.limit && o.out_limit)
            for (int i = 0; i < 5; ++i) o.out_limit[i] = r.limit_out[i];
        if (o.loudness && o.out_loudness)
            for (int i = 0; i < 4; ++i) o.out_loudness[i] = r.loud_out[i];
        if (o.want_marks) {
            *o.out_marks = r.marks;
            *o.out_n_marks = r.n_marks;
        }
        if (o.out_fit && !r.fit.empty() && r.fit_out.size() == r.fit.size()) memcpy(o.out_fit, r.fit_out.data(), r.fit.size() * sizeof(FitResult));
        if (r.want_report) {
            *o.out_report = r.report;
            *o.out_n_report = r.n_report;
        }
        if (o.level && o.out_level) {
            o.out_level[0] = r.level_out[0];
            o.out_level[1] = r.level_out[1];
        }
        return KX_OK;
    }
};

}  // namespace dispatch
}  // namespace kx
