// extern "C" surface of libkokorox_hip.so (include/kokorox_hip.h).  Nothing throws across it.
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>
#include <thread>
#include <chrono>
#include <mutex>

#include "../../include/kokorox_hip.h"
#include "model.h"

using kx::Error;
using kx::Model;

#include "kx_handle.h"

#include "check_device.h"
#include "api_guard.h"  // the exception fence + the per-thread last-error text (HIP-free: sanitizer-tested on the CPU)
using kx::guarded;
using kx::guarded_free;
using kx::set_err;

extern "C" {

const char* kx_version(void) { return "kokorox-hip 0.4 (gfx950; conv modes: f16f8 split MFMA with 8-bit cross terms [default], f16x3 split MFMA, f32 MFMA, f16 / bf16 reduced precision [opt-in])"; }

int kx_init(int device_id, char* err, size_t err_len) {
    return guarded_free(err, err_len, [&] { check_device(device_id); });
}

kx_model* kx_create(const char* weights_path, int device_id, char* err, size_t err_len) {
    kx_model* h = nullptr;
    int rc = guarded_free(err, err_len, [&] {
        check_device(device_id);
        std::unique_ptr<Model> m(new Model(device_id));
        m->load_file(weights_path);
        h = new kx_model{std::move(m)};
    });
    return rc == KX_OK ? h : nullptr;
}

int kx_import_onnx(const char* onnx_path, const char* out_path, char* err, size_t err_len) {
    return guarded_free(err, err_len, [&] {
        KX_REQUIRE(onnx_path && *onnx_path && out_path && *out_path, "kx_import_onnx: two paths");
        const std::vector<unsigned char> in = kx::read_file(onnx_path, "weight file");
        const std::vector<unsigned char> blob = kx::import_onnx_bytes(in.data(), in.size());
        kx::write_file_atomic(out_path, blob.data(), blob.size());
    });
}

int kx_resample_filter(int format_word, int32_t* L, int32_t* M, int32_t* n_taps, float* taps, int cap) {
    return guarded_free(nullptr, 0, [&] {
        kx::check_format_word(format_word);
        const int code = kx::format_rate(format_word);
        if (code == 0) {  // 24 000 Hz: the samples as they are
            if (L) *L = 1;
            if (M) *M = 1;
            if (n_taps) *n_taps = 0;
            return;
        }
        const kx::ResampleFilter& f = kx::resample_filter(code);
        if (L) *L = f.L;
        if (M) *M = f.M;
        if (n_taps) *n_taps = f.n_taps;
        if (taps) {
            KX_REQUIRE(cap >= f.n_taps, "resample_filter: cap is smaller than the number of taps");
            std::memcpy(taps, f.taps, (size_t)f.n_taps * sizeof(float));
        }
    });
}

int kx_limit_filter(int format_word, int32_t* W, float* taps, int cap) {
    return guarded_free(nullptr, 0, [&] {
        kx::check_format_word(format_word);
        const int c = kx::format_rate(format_word), n = 2 * kx::limit_window(c) + 1;
        KX_REQUIRE(W && taps && cap >= n, "limit_filter: null argument or too small a buffer");
        *W = kx::limit_window(c);
        std::memcpy(taps, kx::limit_taps(c), (size_t)n * sizeof(float));
    });
}

int kx_loudness_filter(int format_word, double* out10) {
    return guarded_free(nullptr, 0, [&] {
        kx::check_format_word(format_word);
        KX_REQUIRE(out10, "loudness_filter: null argument");
        std::memcpy(out10, kx::loud_coefs(kx::format_rate(format_word)), 10 * sizeof(double));
    });
}

int kx_truepeak_filter(float* taps, int cap) {
    return guarded_free(nullptr, 0, [&] {
        KX_REQUIRE(taps, "truepeak_filter: null argument");
        KX_REQUIRE(cap >= kx::TRUEPEAK_PHASES * kx::TRUEPEAK_NTAPS, "truepeak_filter: cap is smaller than the 72 taps");
        std::memcpy(taps, kx::truepeak_taps(), (size_t)kx::TRUEPEAK_PHASES * kx::TRUEPEAK_NTAPS * sizeof(float));
    });
}

int kx_adpcm_block(int format_word, int32_t* block_bytes, int32_t* samples_per_block) {
    return guarded_free(nullptr, 0, [&] {
        const long A = kx::adpcm_block_bytes(kx::format_rate(format_word));
        if (block_bytes) *block_bytes = (int32_t)A;
        if (samples_per_block) *samples_per_block = (int32_t)kx::adpcm_block_samples(A);
    });
}

kx_model* kx_create_from_device_blob(const void* d_blob, size_t n_bytes, int device_id, char* err, size_t err_len) {
    kx_model* h = nullptr;
    int rc = guarded_free(err, err_len, [&] {
        check_device(device_id);
        std::unique_ptr<Model> m(new Model(device_id));
        m->load_device_blob(d_blob, n_bytes);
        h = new kx_model{std::move(m)};
    });
    return rc == KX_OK ? h : nullptr;
}

static std::mutex g_replica_times_mu;
static double g_replica_times[3] = {0, 0, 0};

int kx_replicas_times(double* out3) {
    if (!out3) return KX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(g_replica_times_mu);
    for (int i = 0; i < 3; ++i) out3[i] = g_replica_times[i];
    return KX_OK;
}

kx_model* kx_create_partition(const char* weights_path, int device_id, int part, int n_parts, char* err, size_t err_len) {
    kx_model* h = nullptr;
    int rc = guarded_free(err, err_len, [&] {
        check_device(device_id);
        std::unique_ptr<Model> m(new Model(device_id, part, n_parts));
        m->load_file(weights_path);
        h = new kx_model{std::move(m)};
    });
    return rc == KX_OK ? h : nullptr;
}

int kx_create_replicas(const char* weights_path, const int* device_ids, int n, kx_model** out_models, char* err,
                       size_t err_len) {
    if (out_models)
        for (int i = 0; i < n; ++i) out_models[i] = nullptr;
    std::vector<void*> blobs;       // per replica: its device blob until a model has adopted it
    std::vector<int> blob_dev;
    std::vector<hipStream_t> streams;
    std::vector<kx_model*> made;
    using clk = std::chrono::steady_clock;
    const clk::time_point t0 = clk::now();
    auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
    double t_ms[3] = {0, 0, 0};  // file read (+ conversion) done, fan-out done, models built
    int rc = guarded_free(err, err_len, [&] {
        KX_REQUIRE(device_ids && out_models && n >= 1 && n <= 64, "create_replicas: 1..64 device ids and an output array");
        for (int i = 0; i < n; ++i) check_device(device_ids[i]);
        int variant = -2;
        const std::vector<unsigned char> host = kx::read_weight_file(weights_path, &variant);  // the ONE file read
        const size_t nb = host.size();
        (void)kx::kxw_table(host.data(), nb, nb);  // refused here, before n copies of it are made (every model checks its own again)
        t_ms[0] = ms_since(t0);
        blobs.assign(n, nullptr);
        blob_dev.assign(device_ids, device_ids + n);
        streams.assign(n, nullptr);
        // replica 0: host -> device over PCIe, once
        KX_HIP(hipSetDevice(device_ids[0]));
        KX_HIP(hipMalloc(&blobs[0], nb));
        KX_HIP(hipMemcpy(blobs[0], host.data(), nb, hipMemcpyHostToDevice));
        // every other replica: device -> device from replica 0, all copies in flight together (xGMI is
        // point-to-point: each destination has its own link to the source, so they do not share bandwidth)
        for (int i = 1; i < n; ++i) {
            KX_HIP(hipSetDevice(device_ids[i]));
            if (device_ids[i] != device_ids[0]) {
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, device_ids[i], device_ids[0]) == hipSuccess && can) {
                    hipError_t pe = hipDeviceEnablePeerAccess(device_ids[0], 0);
                    if (pe != hipSuccess) (void)hipGetLastError();  // already enabled, or staged copies: both fine
                }
            }
            KX_HIP(hipMalloc(&blobs[i], nb));
            KX_HIP(hipStreamCreateWithFlags(&streams[i], hipStreamNonBlocking));
            KX_HIP(hipMemcpyPeerAsync(blobs[i], device_ids[i], blobs[0], device_ids[0], nb, streams[i]));
        }
        for (int i = 1; i < n; ++i) {
            KX_HIP(hipSetDevice(device_ids[i]));
            KX_HIP(hipStreamSynchronize(streams[i]));
        }
        t_ms[1] = ms_since(t0);
        // A device id that is given k times gets k CU-partitioned models (each confined to 1 / k of the CUs: they run side by
        // side without competing for a CU -- Model::Model); KX_REPLICA_PARTITION=0: whole-device models that take turns.
        static const bool partition = !(getenv("KX_REPLICA_PARTITION") && atoi(getenv("KX_REPLICA_PARTITION")) == 0);
        std::vector<int> part(n, 0), parts(n, 1);
        if (partition)
            for (int i = 0; i < n; ++i) {
                int k = 0, j = 0;
                for (int q = 0; q < n; ++q) {
                    if (device_ids[q] != device_ids[i]) continue;
                    if (q < i) ++j;
                    ++k;
                }
                KX_REQUIRE(k <= 8, "create_replicas: at most 8 models per device");
                part[i] = j;
                parts[i] = k;
            }
        // the models are built side by side, one host thread each (weight repacking on the model's own GPU and stream)
        made.assign(n, nullptr);
        std::vector<std::string> build_err(n);
        std::vector<int> build_rc(n, KX_OK);
        std::vector<std::thread> th;
        for (int i = 0; i < n; ++i)
            th.emplace_back([&, i] {
                void* b = blobs[i];
                try {
                    std::unique_ptr<Model> m(new Model(device_ids[i], part[i], parts[i]));
                    blobs[i] = nullptr;  // the model owns it from here on (freed by its destructor, also on a failed build)
                    m->adopt_blob_guard(b);
                    if (getenv("KX_TEST_HOOKS") && getenv("KX_TEST_FAIL_REPLICA") && atoi(getenv("KX_TEST_FAIL_REPLICA")) == i)
                        throw Error(KX_ERR_IO, "create_replicas: injected failure of replica " + std::to_string(i) + " (KX_TEST_FAIL_REPLICA)");
                    m->load_device_blob(b, nb, /*adopt=*/true);
                    m->set_source_variant(variant);
                    made[i] = new kx_model{std::move(m)};
                } catch (const Error& e) {
                    build_rc[i] = e.code;
                    build_err[i] = e.what();
                } catch (const std::exception& e) {
                    build_rc[i] = KX_ERR_DEVICE;
                    build_err[i] = e.what();
                }
            });
        for (std::thread& t : th) t.join();
        t_ms[2] = ms_since(t0);
        for (int i = 0; i < n; ++i)
            if (build_rc[i] != KX_OK) throw Error(build_rc[i], "create_replicas: replica " + std::to_string(i) + ": " + build_err[i]);
    });
    {
        std::lock_guard<std::mutex> lk(g_replica_times_mu);
        for (int i = 0; i < 3; ++i) g_replica_times[i] = t_ms[i];
    }
    for (size_t i = 0; i < streams.size(); ++i)
        if (streams[i]) {
            (void)hipSetDevice(blob_dev[i]);
            (void)hipStreamDestroy(streams[i]);
        }
    for (size_t i = 0; i < blobs.size(); ++i)
        if (blobs[i]) {
            (void)hipSetDevice(blob_dev[i]);
            (void)hipFree(blobs[i]);
        }
    if (rc != KX_OK) {
        for (kx_model* h : made)
            if (h) kx_destroy(h);
        return rc;
    }
    for (int i = 0; i < n; ++i) out_models[i] = made[i];
    return KX_OK;
}

void kx_destroy(kx_model* m) {
    if (!m) return;
    try {
        delete m;
    } catch (...) {
    }
}

// The message is copied under the model's mutex into storage owned by the CALLING thread: another thread failing on
// the same model afterwards cannot change or free what this pointer refers to.
const char* kx_last_error(const kx_model* m) {
    if (!m || !m->m) return "null model";
    return kx::last_error_of(m);  // (the calling thread's own last failure on this model)
}

int kx_last_error_copy(const kx_model* m, char* buf, size_t buf_len) {
    if (!buf || !buf_len) return KX_ERR_INVALID;
    if (!m || !m->m) {
        set_err(buf, buf_len, "null model");
        return KX_ERR_INVALID;
    }
    set_err(buf, buf_len, kx::last_error_of(m));
    return KX_OK;
}

int kx_infer(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B, const float* styles,
             const float* speeds, int n_speed, uint64_t seed, uint32_t flags, float** out, int64_t* out_lens) {
    return guarded(m, [&](Model& M) { M.infer_host(ids, t_stride, lens, B, styles, speeds, n_speed, seed, flags, out, out_lens); });
}

static_assert(sizeof(kx_prosody) == sizeof(kx::ProsodySpec) && offsetof(kx_prosody, rate) == offsetof(kx::ProsodySpec, rate) &&
                  offsetof(kx_prosody, frames) == offsetof(kx::ProsodySpec, frames) && offsetof(kx_prosody, pitch) == offsetof(kx::ProsodySpec, pitch) &&
                  offsetof(kx_prosody, energy) == offsetof(kx::ProsodySpec, energy) && KX_PROSODY_MAX_FRAMES == kx::PROSODY_MAX_FRAMES,
              "kx_prosody is the layout of kx::ProsodySpec");

int kx_infer_prosody(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B, const float* styles,
                     const float* speeds, int n_speed, uint64_t seed, uint32_t flags, float** out, int64_t* out_lens,
                     const kx_prosody* prosody, int32_t* out_durations) {
    return guarded(m, [&](Model& M) {
        KX_REQUIRE(out && out_lens, "infer: null output argument");
        *out = nullptr;
        KX_REQUIRE(styles, "infer: null argument");
        Model::HostCall hc;
        hc.styles = styles;
        hc.prosody_call = true;
        hc.prosody = reinterpret_cast<const kx::ProsodySpec*>(prosody);
        hc.out_durations = out_durations;
        void* p = nullptr;
        std::vector<int64_t> bytes(B > 0 ? B : 1);
        M.infer_host_ex(ids, t_stride, lens, B, speeds, n_speed, seed, flags, hc, Model::HostResults{&p, bytes.data(), out_lens});
        *out = static_cast<float*>(p);
    });
}

void kx_free_audio(float* p) { kx::host_out_free(p); }
void kx_free_packed(void* p) { kx::host_out_free(p); }

int kx_set_voice_table(kx_model* m, const float* table, int n_voices) {
    return guarded(m, [&](Model& M) { M.set_voice_table(table, n_voices); });
}

int kx_infer_voices(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B,
                    const int32_t* voice_ids, const float* weights, int max_mix, const float* speeds, int n_speed,
                    uint64_t seed, uint32_t flags, int format, void** out, int64_t* out_bytes, int64_t* out_samples) {
    return guarded(m, [&](Model& M) {
        KX_REQUIRE(voice_ids && weights, "infer_voices: null argument");
        Model::HostCall hc;
        hc.voice_ids = voice_ids;
        hc.weights = weights;
        hc.max_mix = max_mix;
        hc.format = format;
        M.infer_host_ex(ids, t_stride, lens, B, speeds, n_speed, seed, flags, hc, Model::HostResults{out, out_bytes, out_samples});
    });
}

int kx_infer_packed(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B, const float* styles,
                    const float* speeds, int n_speed, uint64_t seed, uint32_t flags, int format, void** out,
                    int64_t* out_bytes, int64_t* out_samples) {
    return guarded(m, [&](Model& M) {
        KX_REQUIRE(styles, "infer_packed: null argument");
        Model::HostCall hc;
        hc.styles = styles;
        hc.format = format;
        M.infer_host_ex(ids, t_stride, lens, B, speeds, n_speed, seed, flags, hc, Model::HostResults{out, out_bytes, out_samples});
    });
}

static_assert(sizeof(kx_join) == sizeof(kx::JoinSpec) && offsetof(kx_join, flags) == offsetof(kx::JoinSpec, flags) &&
                  offsetof(kx_join, keep_ms) == offsetof(kx::JoinSpec, keep_ms) && offsetof(kx_join, pause_ms) == offsetof(kx::JoinSpec, pause_ms) &&
                  offsetof(kx_join, fade_ms) == offsetof(kx::JoinSpec, fade_ms) && KX_JOIN_TRIM_HEAD == kx::JOIN_TRIM_HEAD &&
                  KX_JOIN_TRIM_TAIL == kx::JOIN_TRIM_TAIL && KX_JOIN_TRIM_INNER == kx::JOIN_TRIM_INNER,
              "kx_join is the layout of kx::JoinSpec");

static_assert(sizeof(kx_level) == 12 && sizeof(kx_level) == sizeof(kx::LevelSpec) && offsetof(kx_level, mode) == offsetof(kx::LevelSpec, mode) &&
                  offsetof(kx_level, gain) == offsetof(kx::LevelSpec, gain) && offsetof(kx_level, peak) == offsetof(kx::LevelSpec, peak) &&
                  KX_LEVEL_GAIN == kx::LEVEL_GAIN && KX_LEVEL_NORMALIZE == kx::LEVEL_NORMALIZE && KX_LEVEL_CEILING == kx::LEVEL_CEILING && KX_PEAK_TRUE == kx::PEAK_TRUE,
              "kx_level is the layout of kx::LevelSpec");

static_assert(sizeof(kx_loudness) == 12 && sizeof(kx_loudness) == sizeof(kx::LoudSpec) && offsetof(kx_loudness, mode) == offsetof(kx::LoudSpec, mode) &&
                  offsetof(kx_loudness, target_lufs) == offsetof(kx::LoudSpec, target_lufs) && offsetof(kx_loudness, peak) == offsetof(kx::LoudSpec, peak) &&
                  KX_LOUDNESS_MEASURE == kx::LOUD_MEASURE && KX_LOUDNESS_NORMALIZE == kx::LOUD_NORMALIZE,
              "kx_loudness is the layout of kx::LoudSpec");

static_assert(sizeof(kx_limit) == 16 && sizeof(kx_limit) == sizeof(kx::LimitSpec) && offsetof(kx_limit, mode) == offsetof(kx::LimitSpec, mode) &&
                  offsetof(kx_limit, gain) == offsetof(kx::LimitSpec, gain) && offsetof(kx_limit, target_lufs) == offsetof(kx::LimitSpec, target_lufs) &&
                  offsetof(kx_limit, peak) == offsetof(kx::LimitSpec, peak) && KX_LIMIT_GAIN == kx::LIMIT_GAIN && KX_LIMIT_LOUDNESS == kx::LIMIT_LOUDNESS &&
                  KX_LIMIT_MAX_TAPS == kx::LIMIT_MAX_TAPS,
              "kx_limit is the layout of kx::LimitSpec");

// The seven kx_infer_requests* entries are one call.  What they all take, in the order of their C signatures ...
struct RequestArgs {
    kx_model* m;
    const int64_t* ids; int64_t t_stride; const int32_t* lens; int B;
    const int32_t* chunks_per_request; int R;
    const float* styles; const int32_t* voice_ids; const float* weights; int max_mix;
    const float* speeds; int n_speed;
    uint64_t seed; uint32_t flags;
    const int32_t* formats; int n_format;
    void** out; int64_t* out_bytes; int64_t* out_samples;
};
// ... and what each takes beyond that: an entry sets the fields it has, by name.
struct RequestExtras {
    int64_t** out_marks = nullptr;  // the marks pair: either of the two asks for marks
    int64_t* out_n_marks = nullptr;
    const kx_join* joins = nullptr;
    int n_join = 0;
    bool marks_entry = false;  // kx_infer_requests_marks: the pair must be there
    bool join_entry = false;   // kx_infer_requests_joined: `joins` must be there; elsewhere see infer_requests
    // the spec list of the levelled, the loudness or the limiter's entry (a null list is refused with the call's other arguments:
    // check_spec_list) and the array its values come back in
    kx::SpecList<kx::LevelSpec> levels;
    kx::SpecList<kx::LoudSpec> loudness;
    kx::SpecList<kx::LimitSpec> limits;
    double* out_values = nullptr;
    bool prosody_entry = false;  // kx_infer_requests_prosody: a null `prosody` is the neutral one; the report pair is both there or
    const kx_prosody* prosody = nullptr;  // both null (check_prosody_call)
    float** out_report = nullptr;
    int64_t* out_n_report = nullptr;
    bool fit_entry = false;  // kx_infer_requests_fitted: the spans (n_spans == 0: none) and where their results go (may be null)
    const kx_fit_span* spans = nullptr;
    int n_spans = 0;
    kx_fit_result* out_fit = nullptr;
    bool piece_entry = false;  // kx_infer_requests_pieces: the flags and the carry-out must be there (check_piece_call)
    const uint32_t* piece_flags = nullptr;
    const kx_piece_carry* carry_in = nullptr;
    kx_piece_carry* carry_out = nullptr;
};

static int infer_requests(const RequestArgs& a, const RequestExtras& x) {
    return guarded(a.m, [&](Model& M) {
        KX_REQUIRE(a.chunks_per_request && a.formats && a.R >= 1, "infer_requests: null argument");
        KX_REQUIRE((a.styles != nullptr) != (a.voice_ids != nullptr), "infer_requests: give the style rows OR voice ids, not both");
        KX_REQUIRE(a.styles || a.weights, "infer_requests: null argument");
        Model::HostCall hc;
        hc.styles = a.styles;
        hc.voice_ids = a.voice_ids;
        hc.weights = a.weights;
        hc.max_mix = a.voice_ids ? a.max_mix : 0;
        hc.chunks_per_request = a.chunks_per_request;
        hc.n_requests = a.R;
        hc.req_formats = a.formats;
        hc.n_req_formats = a.n_format;
        std::vector<uint8_t> want;
        if (x.marks_entry || x.out_marks || x.out_n_marks) {  // (every request of the call)
            want.assign((size_t)a.R, 1);
            hc.req_marks = want.data();
        }
        // (joins == NULL with n_join == 0: no joins; anything else goes through the join entry's checks)
        if (x.join_entry || x.joins || x.n_join != 0) hc.joins = {true, reinterpret_cast<const kx::JoinSpec*>(x.joins), x.n_join};
        hc.levels = x.levels;
        hc.loudness = x.loudness;
        hc.limits = x.limits;
        Model::HostResults res{a.out, a.out_bytes, a.out_samples};
        res.out_marks = x.out_marks;
        res.out_n_marks = x.out_n_marks;
        res.out_levels = x.levels.call ? x.out_values : nullptr;
        res.out_loudness = x.loudness.call ? x.out_values : nullptr;
        res.out_limits = x.limits.call ? x.out_values : nullptr;
        std::vector<uint8_t> want_report;
        if (x.prosody_entry) {
            hc.prosody_call = true;
            hc.prosody = reinterpret_cast<const kx::ProsodySpec*>(x.prosody);
            if (x.out_report && x.out_n_report) {  // (every request of the call)
                want_report.assign((size_t)a.R, 1);
                hc.req_reports = want_report.data();
            }
            res.out_report = x.out_report;
            res.out_n_report = x.out_n_report;
        }
        if (x.fit_entry) {
            hc.fit_call = true;
            hc.fit_spans = reinterpret_cast<const kx::FitSpan*>(x.spans);
            hc.n_fit_spans = x.n_spans;
            res.out_fit = reinterpret_cast<kx::FitResult*>(x.out_fit);
        }
        if (x.piece_entry) {
            hc.piece_call = true;
            hc.piece_flags = x.piece_flags;
            hc.carry_in = reinterpret_cast<const kx::PieceCarry*>(x.carry_in);
            hc.carry_out = reinterpret_cast<kx::PieceCarry*>(x.carry_out);
        }
        M.infer_host_ex(a.ids, a.t_stride, a.lens, a.B, a.speeds, a.n_speed, a.seed, a.flags, hc, res);
    });
}

int kx_infer_requests(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B,
                      const int32_t* chunks_per_request, int R, const float* styles, const int32_t* voice_ids,
                      const float* weights, int max_mix, const float* speeds, int n_speed, uint64_t seed, uint32_t flags,
                      const int32_t* formats, int n_format, void** out, int64_t* out_bytes, int64_t* out_samples) {
    return infer_requests({m, ids, t_stride, lens, B, chunks_per_request, R, styles, voice_ids, weights, max_mix, speeds, n_speed, seed,
                           flags, formats, n_format, out, out_bytes, out_samples},
                          RequestExtras{});
}

int kx_infer_requests_marks(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B,
                            const int32_t* chunks_per_request, int R, const float* styles, const int32_t* voice_ids,
                            const float* weights, int max_mix, const float* speeds, int n_speed, uint64_t seed, uint32_t flags,
                            const int32_t* formats, int n_format, void** out, int64_t* out_bytes, int64_t* out_samples,
                            int64_t** out_marks, int64_t* out_n_marks) {
    RequestExtras x{out_marks, out_n_marks};
    x.marks_entry = true;
    return infer_requests({m, ids, t_stride, lens, B, chunks_per_request, R, styles, voice_ids, weights, max_mix, speeds, n_speed, seed,
                           flags, formats, n_format, out, out_bytes, out_samples},
                          x);
}

int kx_infer_requests_joined(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B,
                             const int32_t* chunks_per_request, int R, const float* styles, const int32_t* voice_ids,
                             const float* weights, int max_mix, const float* speeds, int n_speed, uint64_t seed, uint32_t flags,
                             const int32_t* formats, int n_format, void** out, int64_t* out_bytes, int64_t* out_samples,
                             int64_t** out_marks, int64_t* out_n_marks, const kx_join* joins, int n_join) {
    RequestExtras x{out_marks, out_n_marks, joins, n_join};
    x.join_entry = true;
    return infer_requests({m, ids, t_stride, lens, B, chunks_per_request, R, styles, voice_ids, weights, max_mix, speeds, n_speed, seed,
                           flags, formats, n_format, out, out_bytes, out_samples},
                          x);
}

int kx_infer_requests_prosody(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B,
                              const int32_t* chunks_per_request, int R, const float* styles, const int32_t* voice_ids,
                              const float* weights, int max_mix, const float* speeds, int n_speed, uint64_t seed, uint32_t flags,
                              const int32_t* formats, int n_format, void** out, int64_t* out_bytes, int64_t* out_samples,
                              int64_t** out_marks, int64_t* out_n_marks, const kx_join* joins, int n_join, const kx_prosody* prosody,
                              float** out_report, int64_t* out_n_report) {
    RequestExtras x{out_marks, out_n_marks, joins, n_join};
    x.prosody_entry = true;
    x.prosody = prosody;
    x.out_report = out_report, x.out_n_report = out_n_report;
    return infer_requests({m, ids, t_stride, lens, B, chunks_per_request, R, styles, voice_ids, weights, max_mix, speeds, n_speed, seed,
                           flags, formats, n_format, out, out_bytes, out_samples},
                          x);
}

static_assert(sizeof(kx_fit_span) == 16 && sizeof(kx_fit_span) == sizeof(kx::FitSpan) && offsetof(kx_fit_span, request) == offsetof(kx::FitSpan, request) &&
                  offsetof(kx_fit_span, begin) == offsetof(kx::FitSpan, begin) && offsetof(kx_fit_span, end) == offsetof(kx::FitSpan, end) &&
                  offsetof(kx_fit_span, frames) == offsetof(kx::FitSpan, frames),
              "kx_fit_span is the layout of kx::FitSpan");
static_assert(sizeof(kx_fit_result) == 16 && sizeof(kx_fit_result) == sizeof(kx::FitResult) &&
                  offsetof(kx_fit_result, lambda) == offsetof(kx::FitResult, lambda) && offsetof(kx_fit_result, n_free) == offsetof(kx::FitResult, n_free) &&
                  offsetof(kx_fit_result, held_frames) == offsetof(kx::FitResult, held_frames) &&
                  offsetof(kx_fit_result, excess) == offsetof(kx::FitResult, excess),
              "kx_fit_result is the layout of kx::FitResult");

int kx_infer_requests_fitted(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B,
                             const int32_t* chunks_per_request, int R, const float* styles, const int32_t* voice_ids,
                             const float* weights, int max_mix, const float* speeds, int n_speed, uint64_t seed, uint32_t flags,
                             const int32_t* formats, int n_format, void** out, int64_t* out_bytes, int64_t* out_samples,
                             int64_t** out_marks, int64_t* out_n_marks, const kx_join* joins, int n_join, const kx_prosody* prosody,
                             float** out_report, int64_t* out_n_report, const kx_fit_span* spans, int n_spans, kx_fit_result* out_fit) {
    RequestExtras x{out_marks, out_n_marks, joins, n_join};
    x.prosody_entry = true;
    x.prosody = prosody;
    x.out_report = out_report, x.out_n_report = out_n_report;
    x.fit_entry = true;
    x.spans = spans, x.n_spans = n_spans, x.out_fit = out_fit;
    return infer_requests({m, ids, t_stride, lens, B, chunks_per_request, R, styles, voice_ids, weights, max_mix, speeds, n_speed, seed,
                           flags, formats, n_format, out, out_bytes, out_samples},
                          x);
}

int kx_infer_requests_levelled(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B,
                               const int32_t* chunks_per_request, int R, const float* styles, const int32_t* voice_ids,
                               const float* weights, int max_mix, const float* speeds, int n_speed, uint64_t seed, uint32_t flags,
                               const int32_t* formats, int n_format, void** out, int64_t* out_bytes, int64_t* out_samples,
                               int64_t** out_marks, int64_t* out_n_marks, const kx_join* joins, int n_join, const kx_level* levels,
                               int n_level, double* out_levels) {
    RequestExtras x{out_marks, out_n_marks, joins, n_join};
    x.levels = {true, reinterpret_cast<const kx::LevelSpec*>(levels), n_level};
    x.out_values = out_levels;
    return infer_requests({m, ids, t_stride, lens, B, chunks_per_request, R, styles, voice_ids, weights, max_mix, speeds, n_speed, seed,
                           flags, formats, n_format, out, out_bytes, out_samples},
                          x);
}

static_assert(sizeof(kx_piece_carry) == 1056 && sizeof(kx_piece_carry) == sizeof(kx::PieceCarry) &&
                  offsetof(kx_piece_carry, magic) == offsetof(kx::PieceCarry, magic) &&
                  offsetof(kx_piece_carry, format_word) == offsetof(kx::PieceCarry, format_word) &&
                  offsetof(kx_piece_carry, src_samples) == offsetof(kx::PieceCarry, src_samples) &&
                  offsetof(kx_piece_carry, out_samples) == offsetof(kx::PieceCarry, out_samples) &&
                  offsetof(kx_piece_carry, n_tail) == offsetof(kx::PieceCarry, n_tail) && offsetof(kx_piece_carry, tail) == offsetof(kx::PieceCarry, tail) &&
                  KX_PIECE_FIRST == kx::PIECE_FIRST && KX_PIECE_LAST == kx::PIECE_LAST && KX_PIECE_TAIL == kx::PIECE_TAIL &&
                  KX_PIECE_MAGIC == kx::PIECE_MAGIC,
              "kx_piece_carry is the layout of kx::PieceCarry");

int kx_infer_requests_pieces(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B,
                             const int32_t* chunks_per_request, int R, const float* styles, const int32_t* voice_ids,
                             const float* weights, int max_mix, const float* speeds, int n_speed, uint64_t seed, uint32_t flags,
                             const int32_t* formats, int n_format, void** out, int64_t* out_bytes, int64_t* out_samples,
                             int64_t** out_marks, int64_t* out_n_marks, const kx_join* joins, int n_join, const kx_level* levels,
                             int n_level, double* out_levels, const uint32_t* piece_flags, const kx_piece_carry* carry_in,
                             kx_piece_carry* carry_out) {
    RequestExtras x{out_marks, out_n_marks, joins, n_join};
    // (levels == NULL with n_level == 0: no levels; anything else goes through the levelled entry's checks)
    if (levels || n_level != 0) x.levels = {true, reinterpret_cast<const kx::LevelSpec*>(levels), n_level};
    x.out_values = out_levels;
    x.piece_entry = true;
    x.piece_flags = piece_flags, x.carry_in = carry_in, x.carry_out = carry_out;
    return infer_requests({m, ids, t_stride, lens, B, chunks_per_request, R, styles, voice_ids, weights, max_mix, speeds, n_speed, seed,
                           flags, formats, n_format, out, out_bytes, out_samples},
                          x);
}

int kx_infer_requests_loudness(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B,
                               const int32_t* chunks_per_request, int R, const float* styles, const int32_t* voice_ids,
                               const float* weights, int max_mix, const float* speeds, int n_speed, uint64_t seed, uint32_t flags,
                               const int32_t* formats, int n_format, void** out, int64_t* out_bytes, int64_t* out_samples,
                               int64_t** out_marks, int64_t* out_n_marks, const kx_join* joins, int n_join,
                               const kx_loudness* loudness, int n_loudness, double* out_loudness) {
    RequestExtras x{out_marks, out_n_marks, joins, n_join};
    x.loudness = {true, reinterpret_cast<const kx::LoudSpec*>(loudness), n_loudness};
    x.out_values = out_loudness;
    return infer_requests({m, ids, t_stride, lens, B, chunks_per_request, R, styles, voice_ids, weights, max_mix, speeds, n_speed, seed,
                           flags, formats, n_format, out, out_bytes, out_samples},
                          x);
}

int kx_infer_requests_limited(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B,
                              const int32_t* chunks_per_request, int R, const float* styles, const int32_t* voice_ids,
                              const float* weights, int max_mix, const float* speeds, int n_speed, uint64_t seed, uint32_t flags,
                              const int32_t* formats, int n_format, void** out, int64_t* out_bytes, int64_t* out_samples,
                              int64_t** out_marks, int64_t* out_n_marks, const kx_join* joins, int n_join, const kx_limit* limits,
                              int n_limit, double* out_limits) {
    RequestExtras x{out_marks, out_n_marks, joins, n_join};
    x.limits = {true, reinterpret_cast<const kx::LimitSpec*>(limits), n_limit};
    x.out_values = out_limits;
    return infer_requests({m, ids, t_stride, lens, B, chunks_per_request, R, styles, voice_ids, weights, max_mix, speeds, n_speed, seed,
                           flags, formats, n_format, out, out_bytes, out_samples},
                          x);
}

int kx_infer_device(kx_model* m, const int64_t* d_ids, int64_t t_stride, const int32_t* lens_host, int B,
                    const float* d_styles, const float* speeds_host, int n_speed, uint64_t seed, uint32_t flags,
                    float* d_audio, int64_t audio_ld, int32_t* d_frames, int64_t* need_ld) {
    return guarded(m, [&](Model& M) {
        M.order_after_null_stream();  // (the caller's device inputs: typically written on the legacy null stream)
        try {
            M.infer_device(d_ids, t_stride, lens_host, B, d_styles, speeds_host, n_speed, seed, flags, d_audio, audio_ld,
                           d_frames, need_ld);
        } catch (const kx::LstmTimeout&) {
            // a token-axis recurrence timed out (seen at the forward's one host wait): the inputs are still where the caller put
            // them, so the call is simply made again, now on the streaming recurrence (same bits).  A time-out of the frame-axis
            // recurrence shows only at kx_sync, which then fails with KX_ERR_DEVICE: that call cannot be repeated from here.
            M.note_rerun();
            M.infer_device(d_ids, t_stride, lens_host, B, d_styles, speeds_host, n_speed, seed, flags, d_audio, audio_ld,
                           d_frames, need_ld);
        }
        M.order_null_stream_after();  // (the caller's later null-stream work waits, on the GPU, for the forward's end)
    });
}

int kx_sync(kx_model* m) {
    return guarded(m, [&](Model& M) {
        M.sync();
        M.note_clean_forward();
    });
}

int kx_model_info(kx_model* m, int64_t* out8) {
    return guarded(m, [&](Model& M) {
        KX_REQUIRE(out8, "model_info: null argument");
        M.info(out8);
    });
}

int kx_model_status(kx_model* m, int64_t* out4) {
    return guarded(m, [&](Model& M) {
        KX_REQUIRE(out4, "model_status: null argument");
        M.status(out4);
    });
}

int kx_set_pinned_durations(kx_model* m, const int32_t* pattern, int n) {
    return guarded(m, [&](Model& M) { M.set_pinned(pattern, n); });
}

int kx_warmup(kx_model* m, int B, int n_tokens, int frames_per_token) {
    return guarded(m, [&](Model& M) { M.warmup(B, n_tokens, frames_per_token); });
}

int kx_call_times(kx_model* m, double* out4) {
    return guarded(m, [&](Model& M) {
        KX_REQUIRE(out4, "call_times: null argument");
        M.call_times(out4);
    });
}

int kx_arena_bytes(kx_model* m, int64_t* out3) {
    if (!out3) return KX_ERR_INVALID;
    return guarded(m, [&](Model& M) { M.arena_bytes(out3); });
}

int kx_set_conv_mode(kx_model* m, int mode) {
    return guarded(m, [&](Model& M) {
        KX_REQUIRE(mode == kx::CONV_F32 || mode == kx::CONV_F16X3 || mode == kx::CONV_F16 || mode == kx::CONV_BF16 || mode == kx::CONV_F16F8,
                   "conv mode must be 0 (f32 MFMA), 1 (f16x3 split MFMA), 4 (f16, reduced precision), 5 (bf16, reduced precision) or 6 (f16f8: 8-bit cross terms)");
        M.set_conv_mode(mode);
    });
}

int kx_get_conv_mode(kx_model* m) { return (m && m->m) ? m->m->conv_mode : -1; }

int kx_set_stft_variant(kx_model* m, int variant) {
    return guarded(m, [&](Model& M) {
        KX_REQUIRE(variant == kx::STFT_ONNX || variant == kx::STFT_TORCH,
                   "stft variant must be 0 (ONNX export: conv-based pair) or 1 (torch.stft / torch.istft)");
        M.sync();
        M.stft_variant = variant;
    });
}

int kx_get_stft_variant(kx_model* m) { return (m && m->m) ? m->m->stft_variant : -1; }

int kx_set_lanes(kx_model* m, int n_lanes) {
    return guarded(m, [&](Model& M) {
        KX_REQUIRE(n_lanes >= 0 && n_lanes <= 4, "lanes must be 0 (by batch size) or 1..4");
        M.sync();
        M.set_lanes(n_lanes);
    });
}

int kx_set_utterance_base(kx_model* m, uint64_t utt_base) {
    return guarded(m, [&](Model& M) { M.utt_base = utt_base; });
}

int kx_profile_enable(kx_model* m, int on) {
    return guarded(m, [&](Model& M) { M.profile_enable(on != 0); });
}

int kx_profile_read(kx_model* m, int64_t* launches, double* total_ms, double* total_flops) {
    return guarded(m, [&](Model& M) {
        KX_REQUIRE(launches && total_ms && total_flops, "profile_read: null argument");
        M.profile_read(launches, total_ms, total_flops);
    });
}

int kx_profile_detail(kx_model* m, double* out, int64_t cap_rows, int64_t* n_rows) {
    return guarded(m, [&](Model& M) {
        KX_REQUIRE(n_rows, "profile_detail: null argument");
        *n_rows = (int64_t)M.prof_detail.size();
        if (!out) return;
        int64_t n = *n_rows < cap_rows ? *n_rows : cap_rows;
        for (int64_t i = 0; i < n; ++i) {
            const auto& r = M.prof_detail[i];
            double* o = out + i * 10;
            o[0] = r.rows; o[1] = r.Cin; o[2] = r.K; o[3] = r.dil; o[4] = r.stride; o[5] = r.store;
            o[6] = r.cols; o[7] = r.flops; o[8] = r.ms; o[9] = r.bytes;
        }
    });
}

int kx_profile_aux(kx_model* m, int64_t* stats_launches, double* stats_bytes) {
    return guarded(m, [&](Model& M) {
        KX_REQUIRE(stats_launches && stats_bytes, "profile_aux: null argument");
        M.profile_aux(stats_launches, stats_bytes);
    });
}

int kx_diag_enable(kx_model* m, int on) {
    return guarded(m, [&](Model& M) { M.diag_enable(on != 0); });
}

int kx_diag_count(kx_model* m, int64_t* n) {
    return guarded(m, [&](Model& M) {
        KX_REQUIRE(n, "diag_count: null argument");
        *n = (int64_t)M.diag_collect().size();
    });
}

int kx_diag_get(kx_model* m, int64_t i, char* name, size_t name_len, double* vals7) {
    return guarded(m, [&](Model& M) {
        KX_REQUIRE(name && name_len && vals7, "diag_get: null argument");
        const auto& d = M.diag_collect();
        KX_REQUIRE(i >= 0 && i < (int64_t)d.size(), "diag_get: index out of range");
        set_err(name, name_len, d[i].name);
        vals7[0] = d[i].rows; vals7[1] = d[i].Cin; vals7[2] = d[i].K; vals7[3] = d[i].act_shift;
        vals7[4] = d[i].absmax; vals7[5] = d[i].rms; vals7[6] = d[i].count;
    });
}

int kx_set_act_prescale(kx_model* m, const char* conv_name, int log2_scale) {
    return guarded(m, [&](Model& M) {
        KX_REQUIRE(conv_name, "set_act_prescale: null argument");
        M.set_act_shift(conv_name, log2_scale);
    });
}

int kx_debug_tap(kx_model* m, const char* name, int b, float* out, int64_t out_cap, int32_t* C, int32_t* L) {
    return guarded(m, [&](Model& M) {
        KX_REQUIRE(name && C && L, "debug_tap: null argument");
        const kx::Tap* t = M.find_tap(name);
        if (!t) throw Error(KX_ERR_STATE, std::string("no such tap (was KX_FLAG_TAPS set?): ") + name);
        KX_REQUIRE(b >= 0 && b < t->B, "debug_tap: utterance index out of range");
        *C = t->C;
        *L = t->L[b];
        if (!out) return;
        KX_REQUIRE(out_cap >= (int64_t)t->C * t->L[b], "debug_tap: output buffer too small");
        for (int c = 0; c < t->C; ++c)
            memcpy(out + (size_t)c * t->L[b], t->data.data() + ((size_t)b * t->C + c) * t->ld, (size_t)t->L[b] * 4);
    });
}

}  // extern "C"
