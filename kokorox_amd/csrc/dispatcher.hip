// Request dispatcher: the C entry points and the kx::Model backend of the host logic in dispatcher_core.h (queue, workers,
// shares, submit-time validation, error policy — HIP-free there so that the CPU suite can run it under the thread and
// address sanitizers against a stub model).
//
// The reference serves every request through one `Mutex<Session>` (kokorox/src/onn/ort_koko.rs:78; callers
// kokorox-openai/src/lib.rs:370-439, kokorox-websocket/src/lib.rs:657-668): N clients = N sequential runs.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dispatcher_core.h"
#include "kx_handle.h"

namespace {

using kx::dispatch::Request;
using kx::dispatch::to_spec;

// One batched forward on a model: requests of every kind / format in one HostCall (per-row kinds and keys, per-request formats).
struct ModelBackend {
    using Handle = kx_model;
    struct Out {
        void* buf = nullptr;  // the packed batch in one pooled page-locked buffer (requests back to back); per REQUEST:
        std::vector<int64_t> bytes, samples;
        // the token marks of the requests that want them: one block in the same buffer, behind the bodies (null: nobody asked)
        int64_t* marks = nullptr;
        std::vector<int64_t> n_marks;
        std::vector<double> levels;  // [R][2] = {f64(p), g} when some request of the batch came through the levelled entry, else empty
        std::vector<double> loud;    // [R][4] = {f64(p), g, I, n_g} when some request came through the loudness entry, else empty
        std::vector<double> limits;  // [R][5] = {f64(p), g, I, n_g, r} when some request came through the limiter's entry, else empty
        std::vector<kx::PieceCarry> carries;  // [R] the carries the pieces of the batch leave, when it has one, else empty
        // the prosody report of the requests that want it: the last block of the same buffer (null: nobody asked)
        float* report = nullptr;
        std::vector<int64_t> n_report;
    };
    static int n_voices(kx_model* h) { return h->m->n_voices(); }
    static int n_vocab(kx_model* h) { return h->m->n_vocab(); }
    static void free_out(void* p) { kx::host_out_free(p); }
    // Rows are chunks: a request of n chunks is n consecutive rows, each with the request's seed as its noise key and its chunk
    // index as the utterance of that key's stream, and comes out of the forward as ONE region (HostCall::chunks_per_request).
    static int forward(kx_model* h, std::vector<Request*>& batch, Out& o) {
        const int R = (int)batch.size();
        int B = 0;
        size_t stride = 0;
        int mm = 1;
        bool any_voice = false, any_marks = false, any_join = false, any_level = false, any_loud = false, any_limit = false;
        bool any_piece = false;
        bool any_rate = false, any_frames = false, any_pitch = false, any_energy = false, any_report = false;
        for (Request* r : batch) {
            any_rate = any_rate || !r->p_rate.empty();
            any_frames = any_frames || !r->p_frames.empty();
            any_pitch = any_pitch || !r->p_pitch.empty();
            any_energy = any_energy || !r->p_energy.empty();
            any_report = any_report || r->want_report;
            any_piece = any_piece || r->piece();
            any_limit = any_limit || r->limited;
            any_loud = any_loud || r->metered;
            any_marks = any_marks || r->want_marks;
            any_join = any_join || r->joined();
            any_level = any_level || r->levelled;
            B += r->rows();
            for (int c = 0; c < r->rows(); ++c) stride = (size_t)r->chunk_len(c) > stride ? (size_t)r->chunk_len(c) : stride;
            mm = r->n_mix > mm ? r->n_mix : mm;
            any_voice = any_voice || r->kind != 0;
        }
        std::vector<int64_t> ids((size_t)B * stride, 0);
        std::vector<int32_t> lens(B), kinds(B), chunks(R), formats(R), vids((size_t)B * mm, -1);
        std::vector<float> styles((size_t)B * KX_STYLE_DIM, 0.f), speeds(B), weights((size_t)B * mm, 0.f);
        std::vector<uint64_t> seeds(B);
        std::vector<uint32_t> uidx(B);
        std::vector<uint8_t> want(R), want_report(R);
        // (a request without prosody beside one that has it: the neutral values, which leave its bits alone)
        std::vector<float> p_rate(any_rate ? (size_t)B * stride : 0, 1.0f), p_pitch(any_pitch ? (size_t)B * stride : 0, 1.0f),
            p_energy(any_energy ? (size_t)B * stride : 0, 1.0f);
        std::vector<int32_t> p_frames(any_frames ? (size_t)B * stride : 0, 0);
        std::vector<kx::JoinSpec> joins(R);  // (a plain request beside a joined one: the all-zero spec, the plain bytes)
        std::vector<kx::LevelSpec> levels(R);  // (a request without levels beside a levelled one: the plain spec, z' = z)
        std::vector<kx::LoudSpec> louds(R);  // (a request without loudness beside a metered one: LOUD_NONE, the meter passes it by)
        // (a request run whole beside a piece: PIECE_WHOLE, planned and launched as ever)
        std::vector<uint32_t> piece_flags(any_piece ? (size_t)R : 0, kx::PIECE_WHOLE);
        std::vector<kx::PieceCarry> carry_in(any_piece ? (size_t)R : 0);
        std::vector<kx::LimitSpec> limits(R);  // (a request without a limiter beside a limited one: LIMIT_NONE, the limiter passes it by)
        // the fit spans of the batch: every request's own, renumbered to its index in the batch (sorted by (request, begin) as the
        // requests' own lists are); a request without spans adds none, and its tokens get zeros in the fitted counts
        std::vector<kx::FitSpan> spans;
        for (int q = 0; q < R; ++q)
            for (const kx::FitSpan& f : batch[(size_t)q]->fit) spans.push_back(kx::FitSpan{q, f.begin, f.end, f.frames});
        std::vector<kx::FitResult> fit_out(spans.size());
        int b = 0;
        for (int q = 0; q < R; ++q) {
            const Request& r = *batch[(size_t)q];
            limits[q] = r.limited ? to_spec(r.limit) : kx::LimitSpec{kx::LIMIT_NONE, 1.0f, 0.0f, 1.0f};
            chunks[q] = r.rows();
            formats[q] = r.format;
            want[q] = r.want_marks ? 1 : 0;
            want_report[q] = r.want_report ? 1 : 0;
            joins[q] = to_spec(r.join);
            levels[q] = to_spec(r.level);
            louds[q] = r.metered ? to_spec(r.loudness) : kx::LoudSpec{kx::LOUD_NONE, 0.0f, 0.0f};
            if (r.piece()) {
                piece_flags[(size_t)q] = r.piece_flags;
                carry_in[(size_t)q] = r.carry_in;
            }
            size_t at = 0;
            for (int c = 0; c < r.rows(); ++c, ++b) {
                lens[b] = (int32_t)r.chunk_len(c);
                memcpy(&ids[(size_t)b * stride], r.ids.data() + at, (size_t)lens[b] * 8);
                if (!r.p_rate.empty()) memcpy(&p_rate[(size_t)b * stride], r.p_rate.data() + at, (size_t)lens[b] * 4);
                if (!r.p_frames.empty()) memcpy(&p_frames[(size_t)b * stride], r.p_frames.data() + at, (size_t)lens[b] * 4);
                if (!r.p_pitch.empty()) memcpy(&p_pitch[(size_t)b * stride], r.p_pitch.data() + at, (size_t)lens[b] * 4);
                if (!r.p_energy.empty()) memcpy(&p_energy[(size_t)b * stride], r.p_energy.data() + at, (size_t)lens[b] * 4);
                at += (size_t)lens[b];
                kinds[b] = r.kind;
                if (r.kind == 0) memcpy(&styles[(size_t)b * KX_STYLE_DIM], r.style.data() + (size_t)c * KX_STYLE_DIM, KX_STYLE_DIM * 4);
                for (int k = 0; k < r.n_mix; ++k) {
                    vids[(size_t)b * mm + k] = r.voice_ids[k];
                    weights[(size_t)b * mm + k] = r.weights[k];
                }
                speeds[b] = r.speed;
                seeds[b] = r.seed;
                uidx[b] = (uint32_t)(r.chunk_base() + c);  // (a later piece's rows: numbered as in the request run whole)
            }
        }
        o.buf = nullptr;
        o.bytes.assign(R, 0);
        o.samples.assign(R, 0);
        o.marks = nullptr;
        o.n_marks.assign(R, 0);
        o.report = nullptr;
        o.n_report.assign(R, 0);
        o.levels.assign(any_level ? (size_t)2 * R : 0, 0.0);
        o.loud.assign(any_loud ? (size_t)4 * R : 0, 0.0);
        o.limits.assign(any_limit ? (size_t)5 * R : 0, 0.0);
        o.carries.assign(any_piece ? (size_t)R : 0, kx::PieceCarry{});
        int rc = KX_ERR_DEVICE;
        std::string err;
        {
            kx::Model& M = *h->m;
            std::lock_guard<std::mutex> lk(M.mu);
            try {
                kx::Model::HostCall hc;
                hc.utt_seeds = seeds.data();
                // every batch is a call of R requests, the single-utterance traffic of submit / submit_ex included: its rows
                // carry utterance index 0, which source_sample_kernel reads exactly as it reads a null utt_index (utterance 0
                // of the key's stream), so their noise, and with it their audio, is what a call without indices gives
                hc.utt_index = uidx.data();
                hc.chunks_per_request = chunks.data();
                hc.n_requests = R;
                hc.req_formats = formats.data();
                hc.n_req_formats = R;
                if (any_marks) hc.req_marks = want.data();
                // (the lists go without their `call` flag: every request was checked when it was submitted)
                if (any_join) hc.joins = {false, joins.data(), R};
                if (any_level) hc.levels = {false, levels.data(), R};
                if (any_loud) hc.loudness = {false, louds.data(), R};
                if (any_limit) hc.limits = {false, limits.data(), R};
                if (any_piece) hc.piece_flags = piece_flags.data(), hc.carry_in = carry_in.data(), hc.carry_out = o.carries.data();
                const kx::ProsodySpec ps{any_rate ? p_rate.data() : nullptr, any_frames ? p_frames.data() : nullptr,
                                         any_pitch ? p_pitch.data() : nullptr, any_energy ? p_energy.data() : nullptr};
                if (any_rate || any_frames || any_pitch || any_energy || any_report) {
                    hc.prosody_call = true;
                    hc.prosody = &ps;
                    if (any_report) hc.req_reports = want_report.data();
                }
                if (!spans.empty()) {
                    hc.fit_call = true;
                    hc.fit_spans = spans.data();
                    hc.n_fit_spans = (int)spans.size();
                }
                if (any_voice) {
                    hc.voice_ids = vids.data();
                    hc.weights = weights.data();
                    hc.max_mix = mm;
                    hc.styles = styles.data();  // (rows of the kind-0 requests; zeros elsewhere)
                    hc.kinds = kinds.data();
                } else {
                    hc.styles = styles.data();
                }
                kx::Model::HostResults res{&o.buf, o.bytes.data(), o.samples.data()};
                res.out_marks = &o.marks, res.out_n_marks = o.n_marks.data();
                if (any_level) res.out_levels = o.levels.data();
                if (any_loud) res.out_loudness = o.loud.data();
                if (any_limit) res.out_limits = o.limits.data();
                if (any_report) res.out_report = &o.report, res.out_n_report = o.n_report.data();
                if (!spans.empty()) res.out_fit = fit_out.data();
                M.infer_host_ex(ids.data(), (int64_t)stride, lens.data(), B, speeds.data(), B, 0, 0, hc, res);
                rc = KX_OK;
                size_t at = 0;  // (the results come back in the order the spans went in)
                for (Request* r : batch) {
                    r->fit_out.assign(fit_out.begin() + (long)at, fit_out.begin() + (long)(at + r->fit.size()));
                    at += r->fit.size();
                }
            } catch (const kx::Error& e) {
                rc = e.code;
                err = e.what();
            } catch (const std::exception& e) {
                err = e.what();
            }
        }
        for (Request* r : batch) {
            r->rc = rc;
            r->err = err;
        }
        return rc;
    }
    // Every request gets ONE pointer INTO the batch's page-locked buffer, for its whole region (no per-request malloc + copy of a
    // megabyte each: that was ~5 ms per batch of host time); the buffer goes back to the pool when the last of them has been
    // freed (kx_free_audio / kx_free_packed -> host_out_free).  The owners counted here and by the copy-out path below are
    // requests, not rows.
    static void distribute(std::vector<Request*>& batch, Out& o) {
        const int B = (int)batch.size();
        std::vector<void*> parts((size_t)B);
        std::vector<int64_t*> marks((size_t)B, nullptr);  // a request's marks go with its body: one owner, one pointer to release
        std::vector<float*> reports((size_t)B, nullptr);  // ... and so does its prosody report
        int64_t off = 0, moff = 0, roff = 0;
        for (int b = 0; b < B; ++b) {
            parts[(size_t)b] = static_cast<char*>(o.buf) + off;
            off += o.bytes[(size_t)b];
            if (o.report && o.n_report[(size_t)b] > 0) reports[(size_t)b] = o.report + 4 * roff;
            roff += o.n_report[(size_t)b];
            if (o.marks && o.n_marks[(size_t)b] > 0) marks[(size_t)b] = o.marks + moff;
            moff += o.n_marks[(size_t)b];
        }
        // A client that keeps (caches, leaks) one result keeps its whole batch's buffer page-locked.  Beyond KX_PINNED_LIVE_CAP_MB
        // (default 4096) of such buffers still held, a batch's results are copied out into plain allocations instead -- the ~5 ms of
        // host time per batch the sharing saves are the price of clients that do not give results back -- and the buffer returns
        // to the pool at once.
        static const long cap_mb = getenv("KX_PINNED_LIVE_CAP_MB") ? atol(getenv("KX_PINNED_LIVE_CAP_MB")) : 4096;
        if (kx::host_out_live_bytes() + (size_t)off > (size_t)(cap_mb > 0 ? cap_mb : 0) * (size_t(1) << 20)) {
            std::vector<void*> copies;
            copies.reserve((size_t)B);
            bool ok = true;
            std::vector<int64_t*> mcopies((size_t)B, nullptr);
            std::vector<float*> rcopies((size_t)B, nullptr);
            for (int b = 0; b < B && ok; ++b) {
                // body, marks and report in ONE plain allocation, each 8-aligned behind the one before: still one pointer to release
                const size_t body = (size_t)o.bytes[(size_t)b], mbytes = marks[(size_t)b] ? (size_t)o.n_marks[(size_t)b] * 8 : 0;
                const size_t rbytes = reports[(size_t)b] ? (size_t)o.n_report[(size_t)b] * 16 : 0;
                const size_t mat = (body + 7) & ~size_t(7);
                void* q = malloc(mbytes || rbytes ? mat + mbytes + rbytes : (body > 0 ? body : 1));
                ok = q != nullptr;
                if (ok) {
                    memcpy(q, parts[(size_t)b], body);
                    if (rbytes) {
                        rcopies[(size_t)b] = reinterpret_cast<float*>(static_cast<char*>(q) + mat + mbytes);
                        memcpy(rcopies[(size_t)b], reports[(size_t)b], rbytes);
                    }
                    if (mbytes) {
                        mcopies[(size_t)b] = reinterpret_cast<int64_t*>(static_cast<char*>(q) + mat);
                        memcpy(mcopies[(size_t)b], marks[(size_t)b], mbytes);
                    }
                    copies.push_back(q);
                }
            }
            if (ok) {
                parts = copies;
                marks = mcopies;
                reports = rcopies;
                kx::host_out_free(o.buf);
            } else {  // (out of pageable memory: share after all)
                for (void* q : copies) free(q);
                kx::host_out_share(o.buf, parts.data(), B);
            }
        } else {
            kx::host_out_share(o.buf, parts.data(), B);
        }
        for (int b = 0; b < B; ++b) {
            Request* r = batch[(size_t)b];
            r->out = parts[(size_t)b];
            r->out_bytes = o.bytes[(size_t)b];
            r->out_samples = o.samples[(size_t)b];
            r->marks = r->want_marks ? marks[(size_t)b] : nullptr;
            r->n_marks = r->want_marks ? o.n_marks[(size_t)b] : 0;
            r->report = r->want_report ? reports[(size_t)b] : nullptr;
            r->n_report = r->want_report ? o.n_report[(size_t)b] : 0;
            if (r->levelled && !o.levels.empty()) {
                r->level_out[0] = o.levels[(size_t)2 * b];
                r->level_out[1] = o.levels[(size_t)2 * b + 1];
            }
            if (r->piece() && !o.carries.empty()) r->carry_out = o.carries[(size_t)b];
            if (r->limited && !o.limits.empty())
                for (int i = 0; i < 5; ++i) r->limit_out[i] = o.limits[(size_t)5 * b + i];
            if (r->metered && !o.loud.empty())
                for (int i = 0; i < 4; ++i) r->loud_out[i] = o.loud[(size_t)4 * b + i];
        }
        o.buf = nullptr;
        o.marks = nullptr;
        o.report = nullptr;
    }
};

}  // namespace

struct kx_dispatcher : kx::dispatch::Core<ModelBackend> {
    kx_dispatcher(kx_model** ms, int n, int max_b, int wait_us) : kx::dispatch::Core<ModelBackend>(ms, n, max_b, wait_us) {}
};

// what every submit entry answers to a null dispatcher
static int no_dispatcher(const char* who, char* err, size_t err_len) {
    if (err && err_len) snprintf(err, err_len, "%s: null dispatcher", who);
    return KX_ERR_INVALID;
}

extern "C" {

kx_dispatcher* kx_dispatcher_create(kx_model** models, int n_models, int max_batch, int max_wait_us, char* err,
                                    size_t err_len) {
    if (!models || n_models < 1 || max_batch < 1 || max_batch > 4096 || max_wait_us < 0) {
        if (err && err_len) snprintf(err, err_len, "dispatcher: bad argument");
        return nullptr;
    }
    for (int i = 0; i < n_models; ++i)
        if (!models[i] || !models[i]->m) {
            if (err && err_len) snprintf(err, err_len, "dispatcher: null model");
            return nullptr;
        }
    try {
        return new kx_dispatcher(models, n_models, max_batch, max_wait_us);
    } catch (const std::exception& e) {
        if (err && err_len) snprintf(err, err_len, "dispatcher: %s", e.what());
        return nullptr;
    }
}

kx_dispatcher* kx_dispatcher_create_warm(kx_model** models, int n_models, int max_batch, int max_wait_us, int warm_tokens,
                                         int warm_frames_per_token, char* err, size_t err_len) {
    if (!models || n_models < 1 || max_batch < 1 || max_batch > 4096) {
        if (err && err_len) snprintf(err, err_len, "dispatcher: bad argument");
        return nullptr;
    }
    // one discarded forward of the largest shape the deployment expects on every model, the models side by side: arenas,
    // page-locked result buffers and tile tables exist before the first request (kx_warmup says why)
    std::vector<std::string> werr((size_t)n_models);
    std::vector<std::thread> th;
    for (int i = 0; i < n_models; ++i)
        th.emplace_back([&, i] {
            if (!models[i] || !models[i]->m) {
                werr[(size_t)i] = "null model";
                return;
            }
            kx::Model& M = *models[i]->m;
            std::lock_guard<std::mutex> lk(M.mu);
            try {
                M.warmup(max_batch, warm_tokens, warm_frames_per_token);
            } catch (const std::exception& e) {
                werr[(size_t)i] = e.what();
            }
        });
    for (std::thread& t : th) t.join();
    for (int i = 0; i < n_models; ++i)
        if (!werr[(size_t)i].empty()) {
            if (err && err_len) snprintf(err, err_len, "dispatcher: warm-up of model %d failed: %s", i, werr[(size_t)i].c_str());
            return nullptr;
        }
    return kx_dispatcher_create(models, n_models, max_batch, max_wait_us, err, err_len);
}

int kx_dispatcher_submit(kx_dispatcher* d, const int64_t* ids, int n_tokens, const float* style, float speed,
                         uint64_t seed, float** out, int64_t* out_len, char* err, size_t err_len) {
    if (!d) return no_dispatcher("dispatcher_submit", err, err_len);
    return d->submit_row(ids, n_tokens, style, speed, seed, out, out_len, err, err_len);
}

int kx_dispatcher_submit_ex(kx_dispatcher* d, const int64_t* ids, int n_tokens, const float* style,
                            const int32_t* voice_ids, const float* weights, int n_mix, float speed, uint64_t seed,
                            int format, void** out, int64_t* out_bytes, int64_t* out_samples, char* err, size_t err_len) {
    if (!d) return no_dispatcher("dispatcher_submit_ex", err, err_len);
    return d->submit_ex(ids, n_tokens, style, voice_ids, weights, n_mix, speed, seed, format, out, out_bytes, out_samples, err,
                        err_len);
}

int kx_dispatcher_submit_request(kx_dispatcher* d, const int64_t* ids, const int32_t* chunk_tokens, int n_chunks,
                                 const float* styles, const int32_t* voice_ids, const float* weights, int n_mix,
                                 float speed, uint64_t seed, int format, void** out, int64_t* out_bytes,
                                 int64_t* out_samples, char* err, size_t err_len) {
    if (!d) return no_dispatcher("dispatcher_submit_request", err, err_len);
    return d->submit_request(ids, chunk_tokens, n_chunks, styles, voice_ids, weights, n_mix, speed, seed, format, out, out_bytes,
                             out_samples, err, err_len);
}

int kx_dispatcher_submit_request_marks(kx_dispatcher* d, const int64_t* ids, const int32_t* chunk_tokens, int n_chunks,
                                       const float* styles, const int32_t* voice_ids, const float* weights, int n_mix,
                                       float speed, uint64_t seed, int format, void** out, int64_t* out_bytes,
                                       int64_t* out_samples, int64_t** out_marks, int64_t* out_n_marks, char* err,
                                       size_t err_len) {
    if (!d) return no_dispatcher("dispatcher_submit_request", err, err_len);
    return d->submit_request_marks(ids, chunk_tokens, n_chunks, styles, voice_ids, weights, n_mix, speed, seed, format, out,
                                   out_bytes, out_samples, out_marks, out_n_marks, err, err_len);
}

int kx_dispatcher_submit_request_joined(kx_dispatcher* d, const int64_t* ids, const int32_t* chunk_tokens, int n_chunks,
                                        const float* styles, const int32_t* voice_ids, const float* weights, int n_mix,
                                        float speed, uint64_t seed, int format, void** out, int64_t* out_bytes,
                                        int64_t* out_samples, int64_t** out_marks, int64_t* out_n_marks, const kx_join* join,
                                        char* err, size_t err_len) {
    if (!d) return no_dispatcher("dispatcher_submit_request", err, err_len);
    return d->submit_request_joined(ids, chunk_tokens, n_chunks, styles, voice_ids, weights, n_mix, speed, seed, format, out,
                                    out_bytes, out_samples, out_marks, out_n_marks, join, err, err_len);
}

int kx_dispatcher_submit_request_levelled(kx_dispatcher* d, const int64_t* ids, const int32_t* chunk_tokens, int n_chunks,
                                          const float* styles, const int32_t* voice_ids, const float* weights, int n_mix,
                                          float speed, uint64_t seed, int format, void** out, int64_t* out_bytes,
                                          int64_t* out_samples, int64_t** out_marks, int64_t* out_n_marks, const kx_join* join,
                                          const kx_level* level, double* out_level, char* err, size_t err_len) {
    if (!d) return no_dispatcher("dispatcher_submit_request", err, err_len);
    return d->submit_request_levelled(ids, chunk_tokens, n_chunks, styles, voice_ids, weights, n_mix, speed, seed, format, out,
                                      out_bytes, out_samples, out_marks, out_n_marks, join, level, out_level, err, err_len);
}

int kx_dispatcher_submit_request_prosody(kx_dispatcher* d, const int64_t* ids, const int32_t* chunk_tokens, int n_chunks,
                                         const float* styles, const int32_t* voice_ids, const float* weights, int n_mix,
                                         float speed, uint64_t seed, int format, void** out, int64_t* out_bytes,
                                         int64_t* out_samples, int64_t** out_marks, int64_t* out_n_marks, const kx_join* join,
                                         const kx_prosody* prosody, float** out_report, int64_t* out_n_report, char* err,
                                         size_t err_len) {
    if (!d) return no_dispatcher("dispatcher_submit_request", err, err_len);
    return d->submit_request_prosody(ids, chunk_tokens, n_chunks, styles, voice_ids, weights, n_mix, speed, seed, format, out,
                                     out_bytes, out_samples, out_marks, out_n_marks, join, prosody, out_report, out_n_report, err,
                                     err_len);
}

int kx_dispatcher_submit_request_fitted(kx_dispatcher* d, const int64_t* ids, const int32_t* chunk_tokens, int n_chunks,
                                        const float* styles, const int32_t* voice_ids, const float* weights, int n_mix,
                                        float speed, uint64_t seed, int format, void** out, int64_t* out_bytes,
                                        int64_t* out_samples, int64_t** out_marks, int64_t* out_n_marks, const kx_join* join,
                                        const kx_prosody* prosody, float** out_report, int64_t* out_n_report,
                                        const kx_fit_span* spans, int n_spans, kx_fit_result* out_fit, char* err, size_t err_len) {
    if (!d) {
        if (err && err_len) snprintf(err, err_len, "dispatcher_submit_request: null dispatcher");
        return KX_ERR_INVALID;
    }
    return d->submit_request_fitted(ids, chunk_tokens, n_chunks, styles, voice_ids, weights, n_mix, speed, seed, format, out,
                                    out_bytes, out_samples, out_marks, out_n_marks, join, prosody, out_report, out_n_report, spans,
                                    n_spans, out_fit, err, err_len);
}

int kx_dispatcher_submit_request_limited(kx_dispatcher* d, const int64_t* ids, const int32_t* chunk_tokens, int n_chunks,
                                         const float* styles, const int32_t* voice_ids, const float* weights, int n_mix,
                                         float speed, uint64_t seed, int format, void** out, int64_t* out_bytes,
                                         int64_t* out_samples, int64_t** out_marks, int64_t* out_n_marks, const kx_join* join,
                                         const kx_limit* limit, double* out_limit, char* err, size_t err_len) {
    if (!d) return no_dispatcher("dispatcher_submit_request", err, err_len);
    return d->submit_request_limited(ids, chunk_tokens, n_chunks, styles, voice_ids, weights, n_mix, speed, seed, format, out,
                                     out_bytes, out_samples, out_marks, out_n_marks, join, limit, out_limit, err, err_len);
}

int kx_dispatcher_submit_request_piece(kx_dispatcher* d, const int64_t* ids, const int32_t* chunk_tokens, int n_chunks,
                                       const float* styles, const int32_t* voice_ids, const float* weights, int n_mix, float speed,
                                       uint64_t seed, int format, void** out, int64_t* out_bytes, int64_t* out_samples,
                                       int64_t** out_marks, int64_t* out_n_marks, const kx_join* join, const kx_level* level,
                                       double* out_level, uint32_t piece_flags, const kx_piece_carry* carry_in,
                                       kx_piece_carry* carry_out, char* err, size_t err_len) {
    if (!d) return no_dispatcher("dispatcher_submit_request", err, err_len);
    return d->submit_request_piece(ids, chunk_tokens, n_chunks, styles, voice_ids, weights, n_mix, speed, seed, format, out, out_bytes,
                                   out_samples, out_marks, out_n_marks, join, level, out_level, piece_flags, carry_in, carry_out, err,
                                   err_len);
}

int kx_dispatcher_submit_request_loudness(kx_dispatcher* d, const int64_t* ids, const int32_t* chunk_tokens, int n_chunks,
                                          const float* styles, const int32_t* voice_ids, const float* weights, int n_mix,
                                          float speed, uint64_t seed, int format, void** out, int64_t* out_bytes,
                                          int64_t* out_samples, int64_t** out_marks, int64_t* out_n_marks, const kx_join* join,
                                          const kx_loudness* loudness, double* out_loudness, char* err, size_t err_len) {
    if (!d) return no_dispatcher("dispatcher_submit_request", err, err_len);
    return d->submit_request_loudness(ids, chunk_tokens, n_chunks, styles, voice_ids, weights, n_mix, speed, seed, format, out,
                                      out_bytes, out_samples, out_marks, out_n_marks, join, loudness, out_loudness, err, err_len);
}

int kx_dispatcher_stats(kx_dispatcher* d, int64_t* n_requests, int64_t* n_batches, int64_t* max_batch_seen) {
    if (!d) return KX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(d->mu);
    if (n_requests) *n_requests = d->n_requests;
    if (n_batches) *n_batches = d->n_batches;
    if (max_batch_seen) *max_batch_seen = d->max_seen_batch;
    return KX_OK;
}

int kx_dispatcher_failures(kx_dispatcher* d, int64_t* n_replayed, int64_t* n_retried) {
    if (!d) return KX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(d->mu);
    if (n_replayed) *n_replayed = d->n_replayed;
    if (n_retried) *n_retried = d->n_retried;
    return KX_OK;
}

int kx_dispatcher_health(kx_dispatcher* d, int32_t* healthy, int n_models, int64_t* n_model_failures, int64_t* n_requeued) {
    if (!d || n_models < 0 || (n_models > 0 && !healthy)) return KX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(d->mu);
    for (int i = 0; i < n_models && i < (int)d->failed.size(); ++i) healthy[i] = d->failed[(size_t)i] ? 0 : 1;
    if (n_model_failures) *n_model_failures = d->n_model_failures;
    if (n_requeued) *n_requeued = d->n_requeued;
    return KX_OK;
}

int kx_dispatcher_model_batches(kx_dispatcher* d, int64_t* per_model, int n_models) {
    if (!d || !per_model || n_models < 0) return KX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(d->mu);
    for (int i = 0; i < n_models && i < (int)d->per_model_batches.size(); ++i) per_model[i] = d->per_model_batches[i];
    return KX_OK;
}

void kx_dispatcher_destroy(kx_dispatcher* d) {
    if (!d) return;
    d->shutdown();  // serves what is queued, refuses new submits, waits for every client thread to leave
    delete d;
}

}  // extern "C"
