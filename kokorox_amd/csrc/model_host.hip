// The host side of a call: staging of a batch's inputs, the forward, the packed result in a pooled page-locked buffer.
// What a call is refused for and where its bytes go is decided without HIP (host_request.cpp, host_pool.cpp).
#include "model.h"

#include <cstdlib>
#include <cstring>

#include "host_pool.h"

namespace kx {

void Model::warmup(int B, int n_tokens, int frames_per_token) {
    KX_REQUIRE(B >= 1 && B <= 4096 && n_tokens >= 2 && n_tokens <= 512 && frames_per_token >= 1 && frames_per_token <= 50,
               "warmup: 1..4096 utterances of 2..512 tokens at 1..50 frames per token");
    // (the caller's pinned pattern, if any, is put back afterwards)
    std::vector<int32_t> saved((size_t)n_pinned_);
    if (n_pinned_) {
        KX_HIP(hipSetDevice(device));
        KX_HIP(hipStreamSynchronize(stream_));
        KX_HIP(hipMemcpy(saved.data(), d_pinned_, saved.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    const int32_t fpt = frames_per_token;
    set_pinned(&fpt, 1);
    struct Restore {
        Model& m;
        std::vector<int32_t>& s;
        ~Restore() {
            try {
                m.set_pinned(s.empty() ? nullptr : s.data(), (int)s.size());
            } catch (...) {
            }
        }
    } restore{*this, saved};
    std::vector<int64_t> ids((size_t)B * n_tokens, 1);
    for (int b = 0; b < B; ++b) ids[(size_t)b * n_tokens] = ids[(size_t)b * n_tokens + n_tokens - 1] = 0;  // the two pads
    std::vector<int32_t> lens((size_t)B, n_tokens);
    std::vector<float> styles((size_t)B * 256, 0.f);
    const float speed = 1.f;
    HostCall hc;
    hc.styles = styles.data();
    void* out = nullptr;
    std::vector<int64_t> bytes((size_t)B), samples((size_t)B);
    infer_host_ex(ids.data(), n_tokens, lens.data(), B, &speed, 1, 0, 1u /* noise off */, hc, HostResults{&out, bytes.data(), samples.data()});
    host_out_free(out);
}

// page-locked scratch for the small per-call host arrays (grown when a larger batch arrives; the stream is idle then: a
// call's copies out of it are followed by that call's synchronisations)
int* Model::stage_ints(size_t n) {
    if (n > h_stage_cap_) {
        KX_HIP(hipStreamSynchronize(stream_));
        if (h_stage_) KX_HIP(hipHostFree(h_stage_));
        h_stage_ = nullptr;
        h_stage_cap_ = 0;
        const size_t want = n < 1024 ? 1024 : 2 * n;
        KX_HIP(hipHostMalloc((void**)&h_stage_, want * sizeof(int), hipHostMallocDefault));
        h_stage_cap_ = want;
    }
    return h_stage_;
}

// kx_infer_device: d_ids / d_styles were written by the caller, typically on the legacy null stream (torch's default);
// the model's stream is non-blocking, so that order is made explicit here (an event on the null stream, no host wait).
void Model::order_after_null_stream() {
    KX_HIP(hipSetDevice(device));
    KX_HIP(hipEventRecord(ev_null_, nullptr));
    KX_HIP(hipStreamWaitEvent(stream_, ev_null_, 0));
}

// ... and on the way out: the model's streams are non-blocking, so work the caller queues on the legacy null stream AFTER
// kx_infer_device returns (torch's default stream reading d_audio, or overwriting d_ids / d_styles for the next request) would
// race with the back half that is still queued.  The null stream waits, on the GPU, for the end of this forward: a caller on
// the null stream is ordered as it was when the model's stream was a blocking one; no host stall.  (Callers on other streams
// must use kx_sync: the header says so.)
void Model::order_null_stream_after() {
    if (!ev_done_) KX_HIP(hipEventCreateWithFlags(&ev_done_, hipEventDisableTiming));
    KX_HIP(hipEventRecord(ev_done_, main_stream_));
    KX_HIP(hipStreamWaitEvent(nullptr, ev_done_, 0));
}

void Model::set_voice_table(const float* table, int n_voices) {
    KX_REQUIRE(table && n_voices >= 1 && n_voices <= 4096, "voice table: 1..4096 voices of [511][256] floats");
    KX_HIP(hipSetDevice(device));
    KX_HIP(hipStreamSynchronize(stream_));
    if (d_voices_) {
        for (auto it = owned_.begin(); it != owned_.end(); ++it)
            if (*it == d_voices_) {
                owned_.erase(it);
                break;
            }
        KX_HIP(hipFree(d_voices_));
        d_voices_ = nullptr;
    }
    const size_t n = (size_t)n_voices * 511 * 256;
    d_voices_ = dev_alloc(n);
    KX_HIP(hipMemcpy(d_voices_, table, n * sizeof(float), hipMemcpyHostToDevice));
    n_voices_.store(n_voices, std::memory_order_release);
}

void Model::infer_host(const int64_t* ids, int64_t t_stride, const int32_t* lens, int B, const float* styles,
                       const float* speeds, int n_speed, uint64_t seed, uint32_t flags, float** out,
                       int64_t* out_lens, const uint64_t* utt_seeds) {
    KX_REQUIRE(out && out_lens, "infer: null output argument");
    HostCall hc;
    hc.styles = styles;
    hc.utt_seeds = utt_seeds;
    KX_REQUIRE(styles, "infer: null argument");
    void* p = nullptr;
    *out = nullptr;
    std::vector<int64_t> bytes(B > 0 ? B : 1);
    infer_host_ex(ids, t_stride, lens, B, speeds, n_speed, seed, flags, hc, HostResults{&p, bytes.data(), out_lens});
    *out = static_cast<float*>(p);
}

// A hand-off time-out of the resident-weights recurrence invalidates the call it happened in, not the request: the host entry
// points run the call once more, now on the streaming recurrence (same bits), and the caller sees a result, not an error.
void Model::infer_host_ex(const int64_t* ids, int64_t t_stride, const int32_t* lens, int B, const float* speeds,
                          int n_speed, uint64_t seed, uint32_t flags, const HostCall& hc, const HostResults& res) {
    try {
        infer_host_once(ids, t_stride, lens, B, speeds, n_speed, seed, flags, hc, res);
    } catch (const LstmTimeout&) {
        n_rerun_ += 1;
        infer_host_once(ids, t_stride, lens, B, speeds, n_speed, seed, flags, hc, res);
    }
    note_clean_forward();
}

void Model::infer_host_once(const int64_t* ids, int64_t t_stride, const int32_t* lens, int B, const float* speeds,
                            int n_speed, uint64_t seed, uint32_t flags, const HostCall& hc, const HostResults& res) {
    check_host_call(ids, t_stride, lens, B, speeds, hc, res.out, res.out_bytes, res.out_samples, n_vocab_, n_voices_, d_voices_ != nullptr);
    if (hc.joins.call) check_spec_list(hc, hc.joins);
    if (hc.req_marks) check_marks_call(hc, res.out_marks, res.out_n_marks);
    if (hc.levels.call) check_spec_list(hc, hc.levels);
    if (hc.loudness.call) check_spec_list(hc, hc.loudness);
    if (hc.limits.call) check_spec_list(hc, hc.limits);
    if (hc.prosody_call) check_prosody_call(hc, lens, B, t_stride, res.out_report, res.out_n_report);
    check_piece_call(hc);  // (nothing to check unless the call came through the entry that takes pieces)
    check_fit_call(hc, lens, B, t_stride, fit_plan_);  // (the empty plan unless the call came through the entry that takes spans)
    const int n_spans = (int)fit_plan_.flat.size();
    KX_REQUIRE(n_spans == 0 || n_pinned_ == 0, "infer: fit with pinned durations");
    const bool by_voice = hc.by_voice();
    // one way to lay the output out and pack it: a call without chunks_per_request is R = B single-row requests in hc.format
    const RequestLayout layout = hc.layout(B);
    const int R = layout.R;
    const bool joins = layout.joins != nullptr;
    const bool marks = layout.marks != nullptr;  // (with chunks_per_request then: check_marks_call)
    // (a call whose flags are all PIECE_WHOLE has no piece: it is planned and launched as the call without them)
    bool pieces = false;
    for (int r = 0; layout.piece_flags && r < R; ++r) pieces = pieces || layout.piece_flags[r] != PIECE_WHOLE;
    // (a call with a limited request is metered and measured: the limiter's drive comes from the two gain kernels)
    bool limited = false;
    for (int i = 0; layout.limits && i < layout.n_limit; ++i) limited = limited || layout.limits[i].mode != LIMIT_NONE;
    const bool loud = layout.loudness != nullptr || limited;
    const bool levels = layout.levels != nullptr || loud;  // (a call with loudness is measured: its peak pass, its levels block)
    // prosody: the arrays the call gave go up with the ids; the rows of the report are known from the token counts alone
    const ProsodySpec no_prosody{nullptr, nullptr, nullptr, nullptr};
    const ProsodySpec& ps = hc.prosody ? *hc.prosody : no_prosody;
    const long n_report = layout.reports ? report_rows(layout, lens, B, h_rep_first_, nullptr) : 0;
    ProsodyDev pd;
    pd.stride = (long)t_stride;
    pd.dur_stride = n_spans > 0 ? 512 : (long)t_stride;  // (a call with spans: the duration kernel reads rate and the fitted counts [B][512])
    pd.n_spans = n_spans;
    if (n_spans > 0 && ps.rate) {
        h_fit_rate_.assign((size_t)B * 512, 1.0f);
        for (int b = 0; b < B; ++b) memcpy(&h_fit_rate_[(size_t)b * 512], ps.rate + (size_t)b * t_stride, (size_t)lens[b] * 4);
    }
    KX_HIP(hipSetDevice(device));
    // I/O staging lives in its own arena: ids, styles, frames, noise keys, voice picks, audio, packed audio
    int64_t* d_ids;
    float* d_styles;
    int* d_fr;
    uint64_t* d_seeds;
    uint32_t* d_uidx;
    OutputTables tables{};
    size_t peak_cap = 0;   // dwords of tables.peak
    size_t hop_cap = 0;    // doubles of tables.hops
    size_t tpeak_cap = 0;  // dwords of tables.tpeak
    size_t lpart_cap = 0;  // dwords of tables.lpart
    size_t lim_cap = 0;    // floats of tables.lim
    size_t slot_cap = 0;   // frames of tables.fslot, tables.flen and tables.foff
    float* d_y = nullptr;  // the resampled streams of the requests with a rate code, back to back
    int *d_vid, *d_rows, *d_kinds;
    float* d_w;
    void* d_packed;
    const int mm = by_voice ? hc.max_mix : 1;
    auto planIO = [&](Arena& A, size_t audio_floats) {
        d_ids = static_cast<int64_t*>(A.alloc((size_t)B * t_stride * 8));
        d_seeds = static_cast<uint64_t*>(A.alloc((size_t)B * 8));
        d_uidx = static_cast<uint32_t*>(A.alloc((size_t)B * 4));
        d_styles = A.f((size_t)B * 256);
        d_fr = A.i(B);
        d_vid = A.i((size_t)B * mm);
        d_rows = A.i(B);
        d_kinds = A.i(B);
        d_w = A.f((size_t)B * mm);
        tables.req = static_cast<PackReq*>(A.alloc((size_t)R * sizeof(PackReq)));
        tables.cum = static_cast<long*>(A.alloc(((size_t)B + 1) * 8));
        const OutputBounds bound = output_bounds(layout, B, audio_floats, lens);
        d_y = A.f(bound.y_floats);  // (0 floats when no word carries a rate code)
        if (joins || levels || pieces) tables.join = static_cast<JoinRow*>(A.alloc((size_t)B * sizeof(JoinRow)));
        if (pieces) {  // (the table of the piece kernels and room for every request's carried tail)
            tables.piece = static_cast<PieceRow*>(A.alloc((size_t)R * sizeof(PieceRow)));
            tables.piece_tail = A.f((size_t)R * PIECE_TAIL);
        }
        if (levels) {  // (the partials of the peak pass are sized here, before the forward: nothing new on a warm model)
            tables.level = static_cast<LevelSpec*>(A.alloc((size_t)R * sizeof(LevelSpec)));
            tables.peak = static_cast<uint32_t*>(A.alloc(bound.peak_dwords * sizeof(uint32_t)));
            peak_cap = bound.peak_dwords;
            if (bound.truepeak_dwords > 0) tables.tpeak = static_cast<uint32_t*>(A.alloc(bound.truepeak_dwords * sizeof(uint32_t)));
            tpeak_cap = bound.truepeak_dwords;
        }
        if (loud) {  // (the hop energies of the meter and its transition powers: sized before the forward as well)
            tables.loud = static_cast<LoudSpec*>(A.alloc((size_t)R * sizeof(LoudSpec)));
            tables.hops = static_cast<double*>(A.alloc(bound.hop_doubles * sizeof(double)));
            tables.loud_pow = static_cast<double*>(A.alloc((size_t)4 * LOUD_POWERS * 16 * sizeof(double)));
            hop_cap = bound.hop_doubles;
        }
        if (limited) {  // (the limited streams and the partials of r: sized before the forward as well)
            tables.limit = static_cast<LimitRow*>(A.alloc((size_t)R * sizeof(LimitRow)));
            tables.lpart = static_cast<uint32_t*>(A.alloc(bound.limit_dwords * sizeof(uint32_t)));
            tables.lim = A.f(bound.lim_floats);
            lpart_cap = bound.limit_dwords;
            lim_cap = bound.lim_floats;
        }
        if (marks) tables.mark = static_cast<MarkRow*>(A.alloc((size_t)B * sizeof(MarkRow)));
        if (bound.flac_slots > 0) {  // (some word has form 12: the encoder's tables and its frame slots, sized before the forward as well)
            tables.frow = static_cast<FlacRow*>(A.alloc((size_t)R * sizeof(FlacRow)));
            tables.finfo = static_cast<FlacInfo*>(A.alloc((size_t)R * sizeof(FlacInfo)));
            tables.fslot = static_cast<uint32_t*>(A.alloc(bound.flac_slots * (size_t)FLAC_SLOT));
            tables.flen = A.i(bound.flac_slots);
            tables.foff = static_cast<long*>(A.alloc(bound.flac_slots * sizeof(long)));
            slot_cap = bound.flac_slots;
        }
        const size_t per_token = (size_t)B * t_stride;  // (laid out as the ids)
        pd.rate = ps.rate ? A.f(n_spans > 0 ? (size_t)B * 512 : per_token) : nullptr;
        if (n_spans > 0) {
            pd.fit_prefix = A.i((size_t)B + 1);
            pd.fit_spans = static_cast<FitFlat*>(A.alloc((size_t)n_spans * sizeof(FitFlat)));
            pd.fit_w = A.f((size_t)B * 512);
            pd.fit_fitted = A.i((size_t)B * 512);
            pd.fit_results = static_cast<FitResult*>(A.alloc((size_t)n_spans * sizeof(FitResult)));
        }
        pd.frames = ps.frames ? A.i(per_token) : nullptr;
        pd.pitch = ps.pitch ? A.f(per_token) : nullptr;
        pd.energy = ps.energy ? A.f(per_token) : nullptr;
        pd.rep_first = n_report > 0 ? static_cast<long*>(A.alloc((size_t)B * sizeof(long))) : nullptr;
        pd.report = n_report > 0 ? A.f((size_t)4 * n_report) : nullptr;
        d_packed = A.alloc(bound.packed_bytes);  // compact output: the requests back to back, then the marks
        return A.f(audio_floats);
    };
    // worst case length is 50 frames per token; start from a typical 8 and retry once if short
    int Tmax = 0;
    for (int b = 0; b < B; ++b) Tmax = lens[b] > Tmax ? lens[b] : Tmax;
    int64_t ld = (int64_t)600 * Tmax * 8;
    for (int attempt = 0; attempt < 2; ++attempt) {
        float* d_audio = plan_arena(arenaIO_, false, [&](Arena& A) { return planIO(A, (size_t)B * ld); });
        KX_HIP(hipMemcpyAsync(d_ids, ids, (size_t)B * t_stride * 8, hipMemcpyHostToDevice, stream_));
        if (hc.styles)  // (explicit rows first: the mix kernel then fills the rows of the utterances that name voices)
            KX_HIP(hipMemcpyAsync(d_styles, hc.styles, (size_t)B * 256 * 4, hipMemcpyHostToDevice, stream_));
        if (by_voice) {
            std::vector<int> rows(B);
            for (int b = 0; b < B; ++b) rows[b] = lens[b] >= 2 ? lens[b] - 2 : 0;  // tokens before the 0 padding (koko.rs:1161-1166)
            KX_HIP(hipMemcpyAsync(d_vid, hc.voice_ids, (size_t)B * mm * 4, hipMemcpyHostToDevice, stream_));
            KX_HIP(hipMemcpyAsync(d_w, hc.weights, (size_t)B * mm * 4, hipMemcpyHostToDevice, stream_));
            int* st = stage_ints((size_t)2 * B);  // page-locked: rows | kinds, copied on the model's own stream
            memcpy(st, rows.data(), (size_t)B * 4);
            KX_HIP(hipMemcpyAsync(d_rows, st, (size_t)B * 4, hipMemcpyHostToDevice, stream_));
            if (hc.kinds) {
                memcpy(st + B, hc.kinds, (size_t)B * 4);
                KX_HIP(hipMemcpyAsync(d_kinds, st + B, (size_t)B * 4, hipMemcpyHostToDevice, stream_));
            }
            launch_style_mix(d_voices_, n_voices_, d_vid, d_w, mm, d_rows, hc.kinds ? d_kinds : nullptr, d_styles, B, stream_);
        }
        // (the per-row noise keys are this call's: the call state keeps pointing at them, into arenaIO_, until the next call
        // resets it, and nothing may read them in between)
        if (hc.utt_seeds) KX_HIP(hipMemcpyAsync(d_seeds, hc.utt_seeds, (size_t)B * 8, hipMemcpyHostToDevice, stream_));
        if (hc.utt_index) KX_HIP(hipMemcpyAsync(d_uidx, hc.utt_index, (size_t)B * 4, hipMemcpyHostToDevice, stream_));
        {
            const size_t per_token = (size_t)B * t_stride * 4;  // bytes of each array
            if (ps.rate && n_spans > 0)
                KX_HIP(hipMemcpyAsync(const_cast<float*>(pd.rate), h_fit_rate_.data(), (size_t)B * 512 * 4, hipMemcpyHostToDevice, stream_));
            else if (ps.rate)
                KX_HIP(hipMemcpyAsync(const_cast<float*>(pd.rate), ps.rate, per_token, hipMemcpyHostToDevice, stream_));
            if (n_spans > 0) {
                KX_HIP(hipMemcpyAsync(const_cast<int*>(pd.fit_prefix), fit_plan_.prefix.data(), ((size_t)B + 1) * 4, hipMemcpyHostToDevice, stream_));
                KX_HIP(hipMemcpyAsync(const_cast<FitFlat*>(pd.fit_spans), fit_plan_.flat.data(), (size_t)n_spans * sizeof(FitFlat),
                                      hipMemcpyHostToDevice, stream_));
            }
            if (ps.frames) KX_HIP(hipMemcpyAsync(const_cast<int*>(pd.frames), ps.frames, per_token, hipMemcpyHostToDevice, stream_));
            if (ps.pitch) KX_HIP(hipMemcpyAsync(const_cast<float*>(pd.pitch), ps.pitch, per_token, hipMemcpyHostToDevice, stream_));
            if (ps.energy) KX_HIP(hipMemcpyAsync(const_cast<float*>(pd.energy), ps.energy, per_token, hipMemcpyHostToDevice, stream_));
            if (pd.rep_first)
                KX_HIP(hipMemcpyAsync(const_cast<long*>(pd.rep_first), h_rep_first_.data(), (size_t)B * sizeof(long), hipMemcpyHostToDevice, stream_));
        }
        Restore<ProsodyDev> prosody(pros_, pd);  // (front_half and back_half read it; the plain call finds it empty)
        int64_t need_ld = 0;
        Restore<bool> edges(want_edges_, joins);  // (the forward brings every row's two edge durations back with its frame counts)
        try {
            infer_device(d_ids, t_stride, lens, B, d_styles, speeds, n_speed, seed, flags, d_audio, ld, d_fr, &need_ld,
                         hc.utt_seeds ? d_seeds : nullptr, hc.utt_index ? d_uidx : nullptr);
        } catch (const Error& e) {
            if (attempt == 0 && need_ld > ld) {
                ld = need_ld;
                continue;
            }
            throw;
        }
        // frame counts are known (the forward's one host sync): the plan of the output stage, then ONE launch packs every
        // request of the batch back to back on the GPU, whatever its form (one before it, the resampler, when a request asks
        // for another rate; one behind it, the token marks, when a request wants them), then ONE asynchronous copy of bodies
        // and marks into a page-locked host buffer.  (All-zero join specs: the plain kernels, the plain bytes.)  A call with
        // levels: the peak pass and the gain kernel sit between resampler and packer, and {p, g} of every request come back
        // behind the marks in the same copy.
        OutputPlan& plan = output_plan_;
        build_output_plan(call_.hF.data(), lens, joins ? h_edge_.data() : nullptr, B, layout, plan);
        for (int r = 0; r < R; ++r) {
            res.out_samples[r] = plan.req[(size_t)r].n_samples;
            res.out_bytes[r] = plan.req[(size_t)r].out_bytes;
            if (marks) res.out_n_marks[r] = plan.count[(size_t)r];
            if (res.out_n_report) res.out_n_report[r] = layout.reports ? plan.rep_count[(size_t)r] : 0;
        }
        KX_REQUIRE(plan.n_report == n_report, "prosody: the report's rows changed under the call");
        KX_REQUIRE((size_t)plan.peak_dwords() <= peak_cap, "levels: the peak table is too small");
        KX_REQUIRE((size_t)plan.hop_doubles() <= hop_cap, "loudness: the hop table is too small");
        KX_REQUIRE((size_t)plan.truepeak_dwords() <= tpeak_cap, "levels: the true-peak table is too small");
        KX_REQUIRE((size_t)plan.limit_dwords() <= lpart_cap && (size_t)plan.lim_floats <= lim_cap, "limiter: the limit buffer is too small");
        KX_REQUIRE((size_t)plan.flac_slots <= slot_cap, "flac: the frame table is too small");
        launch_output_plan(d_audio, ld, call_.d_dur, call_.dT, plan, tables, d_y, d_packed, stream_);
        const int64_t marks_off = plan.marks_off, n_marks = plan.n_marks;
        // (the report was staged by the back half, 16-byte aligned; its block is 8-aligned: one more copy on the device, then the one to the host)
        if (plan.has_report())
            KX_HIP(hipMemcpyAsync(static_cast<char*>(d_packed) + plan.report_off, pd.report, (size_t)16 * plan.n_report, hipMemcpyDeviceToDevice, stream_));
        const int64_t total =
            n_marks > 0 || plan.measured || plan.has_flac() || plan.has_report() || plan.has_pieces() ? plan.end_bytes() : plan.total_bytes;
        char* host = static_cast<char*>(host_out_alloc((size_t)(total > 0 ? total : 1)));
        hipError_t e = hipMemcpyAsync(host, d_packed, (size_t)total, hipMemcpyDeviceToHost, stream_);
        if (e == hipSuccess) e = hipStreamSynchronize(stream_);
        if (e != hipSuccess) {
            host_out_free(host);
            throw Error(3, std::string("infer: D2H copy failed: ") + hipGetErrorString(e));
        }
        // the sticky device error word once more: kernels of the back half (the frame-axis LSTM) can raise it after the
        // forward's mid-way check, and the audio of THIS call would be garbage -- it must fail here, not in the next call
        try {
            check_dev_err();
        } catch (...) {
            host_out_free(host);
            throw;
        }
        // (FLAC bodies are as long as their samples make them: the device's lengths, then the regions moved together; the blocks
        // behind the bodies stay where the plan put them)
        if (plan.has_flac()) {
            try {
                close_flac_gaps(host, plan, reinterpret_cast<const int64_t*>(host + plan.flac_off), res.out_bytes);
            } catch (...) {
                host_out_free(host);
                throw;
            }
        }
        if (hc.out_durations) {  // (the used durations, [B][512] on the device and alive until the next call, as the caller's ids are laid out)
            std::vector<int> h_dur((size_t)B * 512);
            e = hipMemcpy(h_dur.data(), call_.d_dur, h_dur.size() * sizeof(int), hipMemcpyDeviceToHost);
            if (e != hipSuccess) {
                host_out_free(host);
                throw Error(3, std::string("infer: D2H copy failed: ") + hipGetErrorString(e));
            }
            for (int b = 0; b < B; ++b) memcpy(hc.out_durations + (size_t)b * t_stride, &h_dur[(size_t)b * 512], (size_t)lens[b] * sizeof(int));
        }
        if (res.out_fit && n_spans > 0) memcpy(res.out_fit, h_fit_results_.data(), (size_t)n_spans * sizeof(FitResult));
        *res.out = host;
        if (res.out_report) *res.out_report = plan.has_report() ? reinterpret_cast<float*>(host + plan.report_off) : nullptr;
        if (marks) *res.out_marks = n_marks > 0 ? reinterpret_cast<int64_t*>(host + marks_off) : nullptr;
        if (hc.carry_out) {  // (a call without a piece: every request was run whole, and its record is all zeros)
            if (plan.has_pieces()) memcpy(hc.carry_out, host + plan.carry_off, (size_t)R * sizeof(PieceCarry));
            else memset(hc.carry_out, 0, (size_t)R * sizeof(PieceCarry));
        }
        if (plan.measured && res.out_levels) memcpy(res.out_levels, host + plan.levels_off, (size_t)R * 16);
        if (plan.limited && res.out_limits)
            for (int r = 0; r < R; ++r)
                if (plan.limit[(size_t)r].off >= 0) memcpy(res.out_limits + 5 * r, host + plan.limits_off + 40 * (size_t)r, 40);
        if (!plan.loud.empty() && res.out_loudness)
            for (int r = 0; r < R; ++r) {  // {f64(p), g} of the levels block, {I, n_g} of the loudness block
                memcpy(res.out_loudness + 4 * r, host + plan.levels_off + 16 * (size_t)r, 16);
                memcpy(res.out_loudness + 4 * r + 2, host + plan.loud_off + 16 * (size_t)r, 16);
            }
        return;
    }
}

// ---- pooled page-locked host buffers for the results (host_pool.cpp): the process-wide pool on hipHostMalloc ---------------
namespace {
void* pinned_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess || !p) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}
void pinned_free(void* p) { (void)hipHostFree(p); }
HostPool& host_pool() {
    static HostPool* p = new HostPool(pinned_alloc, pinned_free, size_t(1) << 30);  // (leaked on purpose: buffers may outlive static destruction order)
    return *p;
}
}  // namespace

void* host_out_alloc(size_t bytes) { return host_pool().alloc(bytes); }
void host_out_share(void* base, void* const* parts, int n) { host_pool().share(base, parts, n); }
size_t host_out_live_bytes() { return host_pool().live_bytes(); }
void host_out_free(void* p) { host_pool().free(p); }

}  // namespace kx
