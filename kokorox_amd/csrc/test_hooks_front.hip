// Kernel hooks of tests/ (include/kokorox_hip_test.h), the token-axis kernels of Model::front_half: the BiLSTM (dense and ragged) with
// its two process-wide switches, ALBERT's attention, the duration head and alignment, the embeddings, the style projections and the
// row fills and copies.
#include "test_hooks.h"

using namespace kx_test;

namespace {
// What both LSTM hooks set up: the weights as Model::make_lstm packs them, the input GEMM of x (channel-major [B][n_in][x_ld]) on the
// f32 kernel with a time-major store, which is what these tests pin, and the two-CU recurrence's exchange buffer and sticky error
// word as Model holds them.  p = w_ih, w_hh, b_ih, b_hh, then the reverse direction's four.
struct LstmSetup {
    float* gx;    // [B][L][2048] input products (poison_gx: NaN wherever the GEMM does not store)
    float* whhT;
    unsigned long long* xchg;
    unsigned* errw;
};
LstmSetup lstm_setup(DevMem& dm, const float* const (&p)[8], int n_in, const float* dx, int x_ld, const kx::LenMap& lm, int B, int L,
                     bool poison_gx) {
    const kx::DevAlloc alloc = [&dm](size_t bytes) -> void* { return dm.get<unsigned char>(bytes); };
    const kx::PackSrc src{{dm.up(p[0], (size_t)1024 * n_in), dm.up(p[4], (size_t)1024 * n_in), nullptr}, {1024, 1024, 0}};
    const kx::ConvW ih = kx::pack_conv(src, n_in, 1, nullptr, alloc);
    float* bias = dm.get<float>(2048);
    kx::launch_vec_add(dm.up(p[2], 1024), dm.up(p[3], 1024), bias, 1024, nullptr);
    kx::launch_vec_add(dm.up(p[6], 1024), dm.up(p[7], 1024), bias + 1024, 1024, nullptr);
    LstmSetup s{};
    s.whhT = dm.get<float>(2 * 256 * 1024);
    kx::launch_transpose_whh(dm.up(p[1], 1024 * 256), s.whhT, nullptr);
    kx::launch_transpose_whh(dm.up(p[5], 1024 * 256), s.whhT + 256 * 1024, nullptr);
    s.gx = dm.get<float>((size_t)B * L * 2048);
    if (poison_gx) KX_HIP(hipMemset(s.gx, 0xFF, (size_t)B * L * 2048 * 4));
    kx::ConvArgs a{};
    a.x = dx;
    a.x_bs = (long)n_in * x_ld;
    a.x_ld = x_ld;
    a.Cin = n_in;
    a.in_len = lm;
    a.out_len = lm;
    a.n_chunks = ih.n_chunks;
    a.w = ih.w;
    a.bias = bias;
    a.K = 1; a.dil = 1; a.stride = 1; a.pad = 0;
    a.Cout = ih.rows;
    a.y = s.gx;
    a.y_bs = (long)L * 2048;
    a.y_ld = 2048;
    a.out_mul = 1.f; a.out_div = 1.f;
    a.store = kx::ST_TMAJOR;
    a.up_cout = 1;
    kx::launch_conv1d(a, ih.BM, B, L, nullptr);
    s.xchg = dm.get<unsigned long long>(kx::lstm_exchange_bytes(B) / sizeof(unsigned long long));
    KX_HIP(hipMemset(s.xchg, 0, kx::lstm_exchange_bytes(B)));
    s.errw = dm.get<unsigned>(1);
    KX_HIP(hipMemset(s.errw, 0, sizeof(unsigned)));
    return s;
}
// after a launch of the recurrence: wait for it, and fail if its error word is set
void lstm_finish(const LstmSetup& s, const char* timed_out) {
    KX_HIP(hipDeviceSynchronize());
    unsigned herr = 0;
    KX_HIP(hipMemcpy(&herr, s.errw, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (herr) throw Error(KX_ERR_DEVICE, timed_out);
}
}  // namespace

extern "C" {

int kx_test_lstm_fault(int nth) {
    // fault injection is a process-wide switch: it arms only when the environment says this is a test process
    const char* e = getenv("KX_TEST_HOOKS");
    if (!e || strcmp(e, "1") != 0) return KX_ERR_STATE;
    kx::lstm_set_test_fault(nth);
    return KX_OK;
}

int kx_test_lstm_parts(int n) {
    kx::lstm_set_parts(n);
    return KX_OK;
}

int kx_test_lstm(int device_id, const float* x, int B, int L, int n_in, const float* w_ih, const float* w_hh,
                 const float* b_ih, const float* b_hh, const float* w_ih_r, const float* w_hh_r, const float* b_ih_r,
                 const float* b_hh_r, float* y, char* err, size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(x && y && B > 0 && L > 0 && n_in > 0, "test_lstm: bad argument");
        KX_HIP(hipSetDevice(device_id));
        DevMem dm;
        std::vector<float> xc((size_t)B * n_in * L);  // [B,L,n_in] -> channel-major [B][n_in][L], dense rows
        for (int b = 0; b < B; ++b)
            for (int t = 0; t < L; ++t)
                for (int c = 0; c < n_in; ++c) xc[((size_t)b * n_in + c) * L + t] = x[((size_t)b * L + t) * n_in + c];
        const std::vector<int> lens(B, L);
        const kx::LenMap lm{dm.up(lens.data(), B), 1, 0};
        const float* const wts[8] = {w_ih, w_hh, b_ih, b_hh, w_ih_r, w_hh_r, b_ih_r, b_hh_r};
        const LstmSetup s = lstm_setup(dm, wts, n_in, dm.up(xc.data(), xc.size()), L, lm, B, L, false);
        float* dy = dm.get<float>((size_t)B * 512 * L);
        kx::launch_lstm(s.gx, (long)L * 2048, 2048, s.whhT, dy, (long)512 * L, L, lm, B, s.xchg, s.errw, nullptr);
        lstm_finish(s, "test_lstm: the two-CU recurrence timed out waiting for its partner");
        std::vector<float> yc((size_t)B * 512 * L);
        KX_HIP(hipMemcpy(yc.data(), dy, yc.size() * 4, hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b)
            for (int c = 0; c < 512; ++c)
                for (int t = 0; t < L; ++t) y[((size_t)b * L + t) * 512 + c] = yc[((size_t)b * 512 + c) * L + t];
    });
}

int kx_test_lstm_ragged(int device_id, const float* x, const int32_t* lens, int B, int L, int n_in, const float* w_ih,
                        const float* w_hh, const float* b_ih, const float* b_hh, const float* w_ih_r, const float* w_hh_r,
                        const float* b_ih_r, const float* b_hh_r, int inplace, int repeat, uint32_t epoch0, float* y, char* err,
                        size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(x && lens && y && B > 0 && L > 0 && n_in > 0 && repeat >= 1 && repeat <= 16 && epoch0 <= 0xffffu, "test_lstm_ragged: bad argument");
        KX_REQUIRE(!inplace || n_in == 640, "test_lstm_ragged: the in-place form is the duration encoder's: 640 input rows");
        check_lens(lens, B, L, "test_lstm_ragged: lens out of range");
        KX_HIP(hipSetDevice(device_id));
        DevMem dm;
        const int ld = pad32(L);
        // [B,L,n_in] -> channel-major [B][n_in][ld]; the row padding and every column >= lens[b] are NaN
        std::vector<float> xc((size_t)B * n_in * ld, POISON);
        for (int b = 0; b < B; ++b)
            for (int t = 0; t < lens[b]; ++t)
                for (int c = 0; c < n_in; ++c) xc[((size_t)b * n_in + c) * ld + t] = x[((size_t)b * L + t) * n_in + c];
        float* dx = dm.up(xc.data(), xc.size());
        const kx::LenMap lm{dm.up(lens, B), 1, 0};
        // the input GEMM as in kx_test_lstm, on the ragged lengths; gx starts as NaN throughout, so a recurrence that reads a row past an
        // utterance's length poisons its output
        const float* const wts[8] = {w_ih, w_hh, b_ih, b_hh, w_ih_r, w_hh_r, b_ih_r, b_hh_r};
        const LstmSetup s = lstm_setup(dm, wts, n_in, dx, ld, lm, B, L, true);
        KX_HIP(hipDeviceSynchronize());  // (in place, the rows it read are blanked next)
        // the output: 512 padded rows per utterance, of a tensor of its own or (in place, as Model::lstm is called for the duration
        // encoder) rows 0..511 of the 640-row input, whose other 128 rows must come back as they were
        const long y_bs = inplace ? (long)640 * ld : (long)512 * ld;
        float* dy = inplace ? dx : dm.get<float>((size_t)B * 512 * ld);
        const std::vector<float> blank((size_t)512 * ld, SENTINEL);
        unsigned epoch_state = epoch0;  // (the exchange buffer's own launch counter, as Model keeps one per buffer)
        std::vector<float> got((size_t)B * 512 * ld), first;
        for (int r = 0; r < repeat; ++r) {
            // (hipMemcpy on the null stream: behind the GEMM that read these rows, and behind the previous launch)
            for (int b = 0; b < B; ++b) KX_HIP(hipMemcpy(dy + b * y_bs, blank.data(), blank.size() * 4, hipMemcpyHostToDevice));
            kx::launch_lstm(s.gx, (long)L * 2048, 2048, s.whhT, dy, y_bs, ld, lm, B, s.xchg, s.errw, nullptr, &epoch_state);
            lstm_finish(s, "test_lstm_ragged: the two-CU recurrence timed out waiting for its partner");
            for (int b = 0; b < B; ++b)
                KX_HIP(hipMemcpy(&got[(size_t)b * 512 * ld], dy + b * y_bs, (size_t)512 * ld * 4, hipMemcpyDeviceToHost));
            if (r == 0)
                first = got;
            else if (std::memcmp(first.data(), got.data(), got.size() * 4) != 0)
                throw Error(KX_ERR_STATE, "test_lstm_ragged: two launches on one exchange buffer differ");
        }
        if (inplace) {
            std::vector<float> tail((size_t)128 * ld);
            for (int b = 0; b < B; ++b) {
                KX_HIP(hipMemcpy(tail.data(), dx + b * y_bs + (long)512 * ld, tail.size() * 4, hipMemcpyDeviceToHost));
                if (std::memcmp(tail.data(), &xc[((size_t)b * 640 + 512) * ld], tail.size() * 4) != 0)
                    throw Error(KX_ERR_STATE, "test_lstm_ragged: the recurrence wrote into rows 512..639 of its input");
            }
        }
        // (columns >= lens[b] go back to the caller as they are: the sentinel, if the kernel left them alone)
        for (int b = 0; b < B; ++b)
            for (int c = 0; c < 512; ++c) {
                const float* row = &got[((size_t)b * 512 + c) * ld];
                for (int t = 0; t < L; ++t) y[((size_t)b * L + t) * 512 + c] = row[t];
                for (int t = L; t < ld; ++t)
                    if (row[t] != SENTINEL) throw Error(KX_ERR_STATE, "test_lstm_ragged: the kernel wrote into the row padding");
            }
    });
}

int kx_test_attention(int device_id, const float* qkv, const int32_t* lens, int B, int T, float* ctx, char* err,
                      size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(qkv && lens && ctx && B > 0 && T > 0 && T <= 512, "test_attention: bad argument");
        check_lens(lens, B, T, "test_attention: lens out of range");
        KX_HIP(hipSetDevice(device_id));
        DevMem dm;
        const int ld = pad32(T);  // rows padded as in the model (128-byte lines); the padding holds NaNs: the kernel must not use it
        const std::vector<float> q = padded_rows(qkv, B, 2304, T, ld, POISON);
        const float* d_q = dm.up(q.data(), q.size());
        const int* d_len = dm.up(lens, B);
        float* d_ctx = dm.get<float>((size_t)B * 768 * ld);
        KX_HIP(hipMemset(d_ctx, 0, (size_t)B * 768 * ld * 4));
        kx::launch_attention(d_q, (long)2304 * ld, ld, d_ctx, (long)768 * ld, ld, d_len, B, T, nullptr);
        KX_HIP(hipDeviceSynchronize());
        unpad_rows(d_ctx, (size_t)B * 768, T, ld, ctx, nullptr);
    });
}

// the fit in front of the duration head (kx_test_fit_durations): the spans as the caller gave them and where w, the fitted counts
// and the results go
struct FitHook {
    const int32_t* chunks_per_request;
    int R;
    const kx_fit_span* spans;
    int n_spans;
    float* w;                // [B][512]
    int32_t* fitted;         // [B][512]
    kx_fit_result* results;  // [n_spans]
};
// the duration head and the gather; rate / fixed [B][T], both null: launch_duration (kx_test_alignment), else launch_prosody_duration;
// fit given: the two fit kernels first, and launch_prosody_duration on what they wrote
static int alignment_hook(int device_id, const float* logits, int B, int T, const int32_t* lens, const float* speeds, int n_speed,
                          const int32_t* pinned, int n_pinned, const float* rate, const int32_t* fixed, const float* src, int C, int idx_ld,
                          int32_t* dur, int32_t* frames, int32_t* idx, float* gathered, int Fcap, uint32_t* overflow, char* err,
                          size_t err_len, const FitHook* fit = nullptr) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(logits && lens && speeds && src && dur && frames && idx && gathered && overflow && B > 0 && T > 0 && T <= 512 && C > 0 &&
                       idx_ld >= 1 && idx_ld <= 50 * 512 && Fcap >= 1 && (n_speed == 1 || n_speed == B) && n_pinned >= 0 && n_pinned <= 512 &&
                       (n_pinned == 0 || pinned),
                   "test_alignment: bad argument");
        check_lens(lens, B, T, "test_alignment: lens out of range");
        for (int i = 0; i < n_speed; ++i) KX_REQUIRE(speeds[i] > 0.f, "test_alignment: speed must be > 0");
        for (int i = 0; i < n_pinned; ++i) KX_REQUIRE(pinned[i] >= 1 && pinned[i] <= 50, "test_alignment: pinned durations must be in 1..50");
        KX_HIP(hipSetDevice(device_id));
        DevMem dm;
        const int Tp = pad32(T);
        // logits and src on the model's padded rows: the padding and every column >= lens[b] are NaN
        const std::vector<float> lg = padded_rows(logits, B, 50, T, Tp, POISON, lens), sp = padded_rows(src, B, C, T, Tp, POISON, lens);
        const float* d_lg = dm.up(lg.data(), lg.size());
        const float* d_src = dm.up(sp.data(), sp.size());
        const int* d_len = dm.up(lens, B);
        const float* d_speed = dm.up(speeds, n_speed);
        const int* d_pin = n_pinned ? dm.up(pinned, n_pinned) : nullptr;
        // integer outputs start as 0xA5 bytes; the guard stands behind idx
        int* d_dur = dm.get<int>((size_t)B * 512);
        int* d_frames = dm.get<int>(B);
        int* d_idx = guarded_bytes<int>(dm, (size_t)B * idx_ld, 0xA5);
        unsigned* d_over = dm.get<unsigned>(1);
        KX_HIP(hipMemset(d_dur, 0xA5, (size_t)B * 512 * 4));
        KX_HIP(hipMemset(d_frames, 0xA5, (size_t)B * 4));
        KX_HIP(hipMemset(d_over, 0, sizeof(unsigned)));
        float* d_w = nullptr;
        int* d_fitted = nullptr;
        kx::FitResult* d_res = nullptr;
        if (fit) {
            KX_REQUIRE(fit->spans && fit->n_spans >= 1 && fit->w && fit->fitted && fit->results && n_pinned == 0, "test_fit_durations: bad argument");
            // (rate as the duration kernel then reads it, [B][512]; fixed as the caller laid it out; poison past lens[b] in both)
            std::vector<float> hr((size_t)B * 512, POISON);
            std::vector<int32_t> hf((size_t)B * T, (int32_t)0xA5A5A5A5u);
            for (int b = 0; b < B; ++b)
                for (int t = 0; t < lens[b]; ++t) {
                    const size_t i = (size_t)b * T + t;
                    KX_REQUIRE(kx::prosody_value_ok(rate ? rate[i] : 1.0f, fixed ? fixed[i] : 0, 1.0f, 1.0f), "test_fit_durations: bad prosody");
                    if (rate) hr[(size_t)b * 512 + t] = rate[i];
                    if (fixed) hf[i] = fixed[i];
                }
            kx::FitPlan plan;
            KX_REQUIRE(kx::fit_ok(reinterpret_cast<const kx::FitSpan*>(fit->spans), fit->n_spans, fit->chunks_per_request, fit->R, lens, B, fixed, T, plan),
                       "test_fit_durations: bad fit");
            const float* d_rate = rate ? dm.up(hr.data(), hr.size()) : nullptr;
            const int* d_fixed = fixed ? dm.up(hf.data(), hf.size()) : nullptr;
            const int* d_prefix = dm.up(plan.prefix.data(), plan.prefix.size());
            const kx::FitFlat* d_spans = dm.up(plan.flat.data(), plan.flat.size());
            // outputs start as the sentinel / 0xA5 bytes, a guard behind each
            d_w = guarded_buffer(dm, (size_t)B * 512, SENTINEL);
            d_fitted = guarded_bytes<int>(dm, (size_t)B * 512, 0xA5);
            d_res = guarded_bytes<kx::FitResult>(dm, (size_t)fit->n_spans, 0xA5);
            kx::launch_fit_weights(d_lg, (long)50 * Tp, Tp, d_speed, n_speed, d_len, d_rate, 512, d_fixed, T, d_w, d_fitted, B, nullptr);
            kx::launch_fit_spans(d_prefix, B, d_spans, fit->n_spans, d_w, d_fitted, d_res, nullptr);
            kx::launch_prosody_duration(d_lg, (long)50 * Tp, Tp, d_speed, n_speed, d_len, d_pin, n_pinned, d_rate, d_fitted, 512, d_dur, d_frames,
                                        d_idx, idx_ld, d_over, B, nullptr);
        } else if (rate || fixed) {
            // (entries at or past lens[b] go up as NaN / 0xA5 bytes: the kernel must not use them)
            std::vector<float> hr((size_t)B * T, POISON);
            std::vector<int32_t> hf((size_t)B * T, (int32_t)0xA5A5A5A5u);
            for (int b = 0; b < B; ++b)
                for (int t = 0; t < lens[b]; ++t) {
                    const size_t i = (size_t)b * T + t;
                    KX_REQUIRE(kx::prosody_value_ok(rate ? rate[i] : 1.0f, fixed ? fixed[i] : 0, 1.0f, 1.0f), "test_prosody_durations: bad prosody");
                    if (rate) hr[i] = rate[i];
                    if (fixed) hf[i] = fixed[i];
                }
            kx::launch_prosody_duration(d_lg, (long)50 * Tp, Tp, d_speed, n_speed, d_len, d_pin, n_pinned, rate ? dm.up(hr.data(), hr.size()) : nullptr,
                                        fixed ? dm.up(hf.data(), hf.size()) : nullptr, T, d_dur, d_frames, d_idx, idx_ld, d_over, B, nullptr);
        } else {
            kx::launch_duration(d_lg, (long)50 * Tp, Tp, d_speed, n_speed, d_len, d_pin, n_pinned, d_dur, d_frames, d_idx, idx_ld, d_over, B, nullptr);
        }
        KX_HIP(hipDeviceSynchronize());
        KX_HIP(hipMemcpy(dur, d_dur, (size_t)B * 512 * 4, hipMemcpyDeviceToHost));
        KX_HIP(hipMemcpy(frames, d_frames, (size_t)B * 4, hipMemcpyDeviceToHost));
        KX_HIP(hipMemcpy(idx, d_idx, (size_t)B * idx_ld * 4, hipMemcpyDeviceToHost));
        KX_HIP(hipMemcpy(overflow, d_over, sizeof(unsigned), hipMemcpyDeviceToHost));
        guard_untouched(d_idx + (size_t)B * idx_ld, "test_alignment: the duration kernel wrote past idx");
        if (fit) {
            KX_HIP(hipMemcpy(fit->w, d_w, (size_t)B * 512 * 4, hipMemcpyDeviceToHost));
            KX_HIP(hipMemcpy(fit->fitted, d_fitted, (size_t)B * 512 * 4, hipMemcpyDeviceToHost));
            KX_HIP(hipMemcpy(fit->results, d_res, (size_t)fit->n_spans * sizeof(kx::FitResult), hipMemcpyDeviceToHost));
            guard_untouched(d_w + (size_t)B * 512, "test_fit_durations: a fit kernel wrote past w");
            guard_untouched(d_fitted + (size_t)B * 512, "test_fit_durations: a fit kernel wrote past the fitted counts");
            guard_untouched(d_res + fit->n_spans, "test_fit_durations: the fit kernel wrote past its results");
        }
        // the gather reads idx[b][0 .. frames[b]): nothing is launched on a frame count or an index outside its row
        int Fmax = 0;
        for (int b = 0; b < B; ++b) {
            if (frames[b] < 0 || frames[b] > idx_ld) throw Error(KX_ERR_STATE, "test_alignment: a frame count outside 0..idx_ld");
            for (int f = 0; f < frames[b]; ++f)
                if (idx[(size_t)b * idx_ld + f] < 0 || idx[(size_t)b * idx_ld + f] >= lens[b])
                    throw Error(KX_ERR_STATE, "test_alignment: an alignment index outside its utterance");
            Fmax = frames[b] > Fmax ? frames[b] : Fmax;
        }
        KX_REQUIRE(Fmax <= Fcap, "test_alignment: Fcap is too small");
        const int Fp = pad32(Fcap);
        const size_t n_g = (size_t)B * C * Fp;
        float* d_g = guarded_buffer(dm, n_g, SENTINEL);
        if (Fmax > 0) kx::launch_gather_cols(d_src, (long)C * Tp, Tp, d_g, (long)C * Fp, Fp, C, d_idx, idx_ld, d_frames, B, Fmax, nullptr);
        KX_HIP(hipDeviceSynchronize());
        unpad_rows(d_g, (size_t)B * C, Fcap, Fp, gathered, "test_alignment: the gather wrote into the row padding");
        guard_untouched(d_g + n_g, "test_alignment: the gather wrote past its tensor");
    });
}

int kx_test_alignment(int device_id, const float* logits, int B, int T, const int32_t* lens, const float* speeds, int n_speed,
                      const int32_t* pinned, int n_pinned, const float* src, int C, int idx_ld, int32_t* dur, int32_t* frames,
                      int32_t* idx, float* gathered, int Fcap, uint32_t* overflow, char* err, size_t err_len) {
    return alignment_hook(device_id, logits, B, T, lens, speeds, n_speed, pinned, n_pinned, nullptr, nullptr, src, C, idx_ld, dur, frames, idx,
                          gathered, Fcap, overflow, err, err_len);
}

int kx_test_prosody_durations(int device_id, const float* logits, int B, int T, const int32_t* lens, const float* speeds, int n_speed,
                              const int32_t* pinned, int n_pinned, const float* rate, const int32_t* fixed, const float* src, int C,
                              int idx_ld, int32_t* dur, int32_t* frames, int32_t* idx, float* gathered, int Fcap, uint32_t* overflow,
                              char* err, size_t err_len) {
    if (!rate && !fixed) return guarded_free(err, err_len, [] { throw Error(KX_ERR_INVALID, "test_prosody_durations: a rate or a frame count per token"); });
    return alignment_hook(device_id, logits, B, T, lens, speeds, n_speed, pinned, n_pinned, rate, fixed, src, C, idx_ld, dur, frames, idx,
                          gathered, Fcap, overflow, err, err_len);
}

int kx_test_fit_durations(int device_id, const float* logits, int B, int T, const int32_t* lens, const float* speeds, int n_speed,
                          const float* rate, const int32_t* fixed, const int32_t* chunks_per_request, int R, const kx_fit_span* spans,
                          int n_spans, const float* src, int C, int idx_ld, int32_t* dur, int32_t* frames, int32_t* idx, float* gathered,
                          int Fcap, uint32_t* overflow, float* w, int32_t* fitted, kx_fit_result* results, char* err, size_t err_len) {
    const FitHook fit{chunks_per_request, R, spans, n_spans, w, fitted, results};
    return alignment_hook(device_id, logits, B, T, lens, speeds, n_speed, nullptr, 0, rate, fixed, src, C, idx_ld, dur, frames, idx, gathered,
                          Fcap, overflow, err, err_len, &fit);
}

int kx_test_prosody_curves(int device_id, const float* curves, const int32_t* frames, int B, int Fcap, const int32_t* lens, int T,
                           const int32_t* idx, int idx_ld, const int32_t* dur, const float* pitch, const float* energy, float* shaped,
                           float* report, char* err, size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(curves && frames && lens && idx && dur && shaped && B > 0 && Fcap >= 1 && T > 0 && T <= 512 && idx_ld >= Fcap &&
                       idx_ld <= 50 * 512 && (pitch || energy || report),
                   "test_prosody_curves: bad argument");
        check_lens(lens, B, T, "test_prosody_curves: lens out of range");
        // what the kernel indexes with is checked here: frames inside the row, every index a token of its utterance, durations that
        // add up to the frames
        long n_tokens = 0;
        std::vector<long> first((size_t)B);
        std::vector<int32_t> dur512((size_t)B * 512, (int32_t)0xA5A5A5A5u);
        std::vector<float> hp((size_t)B * T, POISON), he((size_t)B * T, POISON);
        for (int b = 0; b < B; ++b) {
            KX_REQUIRE(frames[b] >= 1 && frames[b] <= Fcap, "test_prosody_curves: frames out of range");
            long sum = 0;
            for (int t = 0; t < lens[b]; ++t) {
                const size_t i = (size_t)b * T + t;
                KX_REQUIRE(dur[i] >= 0, "test_prosody_curves: negative duration");
                KX_REQUIRE(kx::prosody_value_ok(1.0f, 0, pitch ? pitch[i] : 1.0f, energy ? energy[i] : 1.0f), "test_prosody_curves: bad prosody");
                sum += dur[i];
                dur512[(size_t)b * 512 + t] = dur[i];
                if (pitch) hp[i] = pitch[i];
                if (energy) he[i] = energy[i];
            }
            KX_REQUIRE(sum == frames[b], "test_prosody_curves: durations do not add up to the frames");
            for (int f = 0; f < frames[b]; ++f)
                KX_REQUIRE(idx[(size_t)b * idx_ld + f] >= 0 && idx[(size_t)b * idx_ld + f] < lens[b], "test_prosody_curves: an alignment index outside its utterance");
            first[(size_t)b] = n_tokens;
            n_tokens += lens[b];
        }
        KX_HIP(hipSetDevice(device_id));
        DevMem dm;
        // the curves on the model's padded rows, as the caller gave them (its poison past 2 frames[b] comes back with `shaped`); the
        // row padding holds the sentinel and the guard stands behind the tensor
        const int n2 = 2 * Fcap, ld = pad32(n2);
        const std::vector<float> rows = padded_rows(curves, B, 2, n2, ld, SENTINEL);
        float* d_curves = guarded_upload(dm, rows);
        float* d_report = report ? guarded_buffer(dm, (size_t)4 * n_tokens, SENTINEL) : nullptr;
        kx::launch_prosody_curves(d_curves, (long)2 * ld, ld, dm.up(frames, B), dm.up(lens, B), dm.up(dur512.data(), dur512.size()),
                                  dm.up(idx, (size_t)B * idx_ld), idx_ld, pitch ? dm.up(hp.data(), hp.size()) : nullptr,
                                  energy ? dm.up(he.data(), he.size()) : nullptr, T, report ? dm.up(first.data(), first.size()) : nullptr, d_report, B,
                                  nullptr);
        KX_HIP(hipDeviceSynchronize());
        unpad_rows(d_curves, (size_t)B * 2, n2, ld, shaped, "test_prosody_curves: the kernel wrote into the row padding");
        guard_untouched(d_curves + rows.size(), "test_prosody_curves: the kernel wrote past the curves");
        if (report) {
            KX_HIP(hipMemcpy(report, d_report, (size_t)16 * n_tokens, hipMemcpyDeviceToHost));
            guard_untouched(d_report + (size_t)4 * n_tokens, "test_prosody_curves: the kernel wrote past the report");
        }
    });
}

int kx_test_embed(int device_id, const int64_t* ids, int B, int ids_stride, int T, const int32_t* lens, const float* text_table,
                  const float* word, const float* type0, const float* pos, int n_vocab, float* out_text, float* out_albert,
                  uint32_t* bad, char* err, size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(ids && lens && text_table && word && type0 && pos && out_text && out_albert && bad && B > 0 && T > 0 && T <= 512 &&
                       ids_stride >= T && n_vocab > 0,
                   "test_embed: bad argument");
        check_lens(lens, B, T, "test_embed: lens out of range");
        KX_HIP(hipSetDevice(device_id));
        DevMem dm;
        const int ld = pad32(T);
        const int64_t* d_ids = dm.up(ids, (size_t)B * ids_stride);
        const int* d_len = dm.up(lens, B);
        const float* d_tab = dm.up(text_table, (size_t)n_vocab * 512);
        const float* d_word = dm.up(word, (size_t)n_vocab * 128);
        const float* d_type = dm.up(type0, 128);
        const float* d_pos = dm.up(pos, (size_t)T * 128);
        const std::vector<float> blank((size_t)B * 512 * ld, SENTINEL);
        float* d_text = dm.up(blank.data(), (size_t)B * 512 * ld);
        float* d_alb = dm.up(blank.data(), (size_t)B * 128 * ld);
        // one sticky word for both kernels, as in the model
        unsigned* d_bad = dm.get<unsigned>(1);
        KX_HIP(hipMemset(d_bad, 0, sizeof(unsigned)));
        kx::launch_embed(d_ids, ids_stride, d_tab, 512, d_text, (long)512 * ld, ld, d_len, B, T, n_vocab, d_bad, nullptr);
        kx::launch_albert_embed(d_ids, ids_stride, d_word, d_type, d_pos, d_alb, (long)128 * ld, ld, d_len, B, T, n_vocab, d_bad, nullptr);
        KX_HIP(hipDeviceSynchronize());
        KX_HIP(hipMemcpy(bad, d_bad, sizeof(unsigned), hipMemcpyDeviceToHost));
        unpad_rows(d_text, (size_t)B * 512, T, ld, out_text, "test_embed: embed_kernel wrote into the row padding");
        unpad_rows(d_alb, (size_t)B * 128, T, ld, out_albert, "test_embed: albert_embed_kernel wrote into the row padding");
    });
}

int kx_test_style_fc(int device_id, const float* styles, int B, const float* w, const float* bias, const int32_t* n_out,
                     const int32_t* style_off, int n_desc, float* out, char* err, size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(styles && w && bias && n_out && style_off && out && B > 0 && n_desc > 0, "test_style_fc: bad argument");
        KX_HIP(hipSetDevice(device_id));
        DevMem dm;
        // the descriptors as Model::add_fc packs them: outputs back to back in one row per utterance, every weight tensor an
        // allocation of its own (a blob's tensors start on 256-byte boundaries: the kernel reads the rows as float4)
        std::vector<kx::FcDesc> desc((size_t)n_desc);
        long total = 0;
        for (int i = 0; i < n_desc; ++i) {
            KX_REQUIRE(n_out[i] > 0 && (style_off[i] == 0 || style_off[i] == 128), "test_style_fc: bad descriptor");
            kx::FcDesc& d = desc[(size_t)i];
            d.w = dm.up(w + (size_t)total * 128, (size_t)n_out[i] * 128);
            d.b = dm.up(bias + total, (size_t)n_out[i]);
            d.n_out = n_out[i];
            d.style_off = style_off[i];
            d.out_off = total;
            total += n_out[i];
        }
        const kx::FcDesc* d_desc = dm.up(desc.data(), desc.size());
        const float* d_styles = dm.up(styles, (size_t)B * 256);
        const size_t n = (size_t)B * total;
        float* d_out = guarded_buffer(dm, n, SENTINEL);
        kx::launch_style_fc(d_desc, n_desc, d_styles, d_out, total, B, nullptr);
        KX_HIP(hipDeviceSynchronize());
        KX_HIP(hipMemcpy(out, d_out, n * 4, hipMemcpyDeviceToHost));
        guard_untouched(d_out + n, "test_style_fc: the kernel wrote past the last utterance's row");
    });
}

int kx_test_rows(int device_id, const float* styles, const int32_t* lens, int B, int T, float* fill_out, const float* src, int rows,
                 int Ls, int Ld, int mul, int add, float* copy_out, char* err, size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(styles && lens && fill_out && src && copy_out && B > 0 && T > 0 && rows > 0 && Ls > 0 && Ld > 0, "test_rows: bad argument");
        for (int b = 0; b < B; ++b) {
            const long m = (long)lens[b] * mul + add;
            KX_REQUIRE(lens[b] >= 1 && lens[b] <= T && m >= 0 && m <= Ls && m <= Ld, "test_rows: lens out of range");
        }
        KX_HIP(hipSetDevice(device_id));
        DevMem dm;
        const int* d_len = dm.up(lens, B);
        const float* d_styles = dm.up(styles, (size_t)B * 256);
        // the style rows of the duration encoder's input: rows 512..639 of a 640-row tensor = the second half of the style row
        const int ld = pad32(T);
        const std::vector<float> blank((size_t)B * 640 * ld, SENTINEL);
        float* d_fill = dm.up(blank.data(), blank.size());
        kx::launch_fill_style_rows(d_fill, (long)640 * ld, ld, 512, d_styles, 128, d_len, B, T, nullptr);
        // a copy between tensors of different row strides over a mapped length (lens[b] mul + add columns of every row)
        const int sld = pad32(Ls), dld = pad32(Ld) + 32;
        const std::vector<float> sp = padded_rows(src, B, rows, Ls, sld, POISON);
        const float* d_src = dm.up(sp.data(), sp.size());
        const size_t n = (size_t)B * rows * dld;
        float* d_copy = guarded_buffer(dm, n, SENTINEL);
        kx::launch_copy_rows(d_src, (long)rows * sld, sld, d_copy, (long)rows * dld, dld, rows, kx::LenMap{d_len, mul, add}, B, Ld, nullptr);
        KX_HIP(hipDeviceSynchronize());
        unpad_rows(d_fill, (size_t)B * 640, T, ld, fill_out, "test_rows: fill_style_rows_kernel wrote into the row padding");
        unpad_rows(d_copy, (size_t)B * rows, Ld, dld, copy_out, "test_rows: copy_rows_kernel wrote into the row padding");
        guard_untouched(d_copy + n, "test_rows: copy_rows_kernel wrote past its tensor");
    });
}

}  // extern "C"
