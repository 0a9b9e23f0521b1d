// Host-side model object behind the C ABI (include/kokorox_hip.h).
#pragma once
#include <atomic>
#include <chrono>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "kx_common.h"
#include "kxw_file.h"

namespace kx {

struct ConvW {
    const float* w = nullptr;     // packed [co_tile][chunk][k][8][BM]
    const float* bias = nullptr;  // [Cout] or null
    int rows = 0, Cin = 0, K = 0, BM = 0, n_chunks = 0;
    int up_s = 0, up_cout = 0;  // polyphase transposed conv
    const void* w16 = nullptr;  // split-f16 image (conv_f16x3.hip)
    const void* w16b = nullptr; // bf16 form of it (built when KOKOROX_CONV=bf16 / kx_set_conv_mode(5) is first selected)
    const void* w8x = nullptr;  // 8-bit cross image of it (f16f8 mode: KOKOROX_CONV=f16f8 / kx_set_conv_mode(6); the S16 form's shapes only)
    int n_chunks16 = 0;
    float unscale = 1.f;        // 2^-ws
    std::string name;           // registry key (diagnostics, kx_set_act_prescale)
    int act_shift = 0;          // f16x3: the transformed input is multiplied by 2^act_shift before the hi/lo split
};

struct LstmW {
    ConvW ih;                     // rows 2048 = [fwd i f g o | rev i f g o], bias = b_ih + b_hh
    const float* whhT = nullptr;  // [2][256][1024]
};

// bump allocator over one device allocation; `measure` mode only counts
struct Arena {
    char* base = nullptr;
    size_t cap = 0, off = 0;
    bool measure = false;
    void* alloc(size_t bytes) {
        const size_t a = (off + 255) & ~size_t(255);
        off = a + bytes;
        if (measure) return nullptr;
        if (off > cap) throw Error(3, "arena overflow (internal sizing bug)");
        return base + a;
    }
    float* f(size_t n) { return static_cast<float*>(alloc(n * sizeof(float))); }
    int* i(size_t n) { return static_cast<int*>(alloc(n * sizeof(int))); }
};

struct Tap {
    std::vector<float> data;  // [B][C][ld]
    int B = 0, C = 0, ld = 0;
    std::vector<int> L;
};

// activation view: [B][C][ld], utterance b valid for len.lens[b]*len.mul+len.add columns
struct T {
    float* p = nullptr;
    long bs = 0;
    int ld = 0;
    int C = 0;
    LenMap len{nullptr, 1, 0};
    int Lmax = 0;
    // C rows of ld floats per utterance; bs: floats from one utterance to the next where that is not C * ld
    static T of(float* p, int C, int ld, LenMap len, int Lmax, long bs = -1) {
        T t;
        t.p = p; t.bs = bs >= 0 ? bs : (long)C * ld; t.ld = ld; t.C = C; t.len = len; t.Lmax = Lmax;
        return t;
    }
    T rows(int r0, int n) const {
        T t = *this;
        t.p = p + (long)r0 * ld;
        t.C = n;
        return t;
    }
};

struct ConvOpts {
    const float* nmean = nullptr;
    const float* nscale = nullptr;
    const float* nshift = nullptr;
    int act = ACT_NONE;
    float slope = 0.f;
    const float* alpha = nullptr;
    int dil = 1, stride = 1, pad = 0, in_up2 = 0;
    const T* resid = nullptr;
    int accum = 0;
    float out_mul = 1.f, out_div = 1.f;
    int epi = EPI_NONE;
    int store = ST_NORMAL;
    int up_pad = 0, up_off = 0, up_reflect = 0;
    LenMap up_len{nullptr, 1, 0};  // ST_UPSCATTER: un-shifted output length
    float2* stat_part = nullptr;   // fuse InstanceNorm partial sums of the output into the epilogue
};

// ---- conv launch assembly (conv_call.hip): the weight images of a layer and the arguments of a launch, built in one place for
// Model and for the kernel hooks of tests/ -------------------------------------------------------------------------------------
using DevAlloc = std::function<void*(size_t bytes)>;  // device memory that lives as long as the weights (Model: owned_)
// a complete ConvW (f32 pack, weight shift, split-f16 image; no bias) from canonical device weights: one to three
// row-concatenated [rows_i][Cin][K] sources, or a ConvTranspose1d weight [Cin][Cout][2 stride] as a polyphase two-tap GEMM
ConvW pack_conv(const PackSrc& src, int Cin, int K, hipStream_t s, const DevAlloc& alloc);
ConvW pack_convT(const float* w, int Cin, int Cout, int stride, hipStream_t s, const DevAlloc& alloc);
// the bf16 image (128-row tiles) / the 8-bit cross image (conv16_f8_layer shapes of plain convs), where the layer qualifies
// and does not have it yet
void add_bf16_image(ConvW& c, hipStream_t s, const DevAlloc& alloc);
void add_f8_image(ConvW& c, hipStream_t s, const DevAlloc& alloc);

struct ConvCtx {  // what a conv launch takes from its caller beyond layer, tensors and options
    int mode = CONV_F16F8;   // ConvMode
    bool p1_region = false;  // inside the part of the forward whose direct-A convs may run reduced precision (CONV_F16 / CONV_BF16)
    int B = 0;
    int cus = 0;             // ConvLaunch::cus
    int n_bs = 0;            // row stride of the AdaIN parameter planes
    // the test hooks' overrides
    int force = 0;           // ConvForce bits (ConvArgs::ws_force)
    int image = 0;           // ConvLaunch::image (the model: 1 while the back half is issued)
    int epi_stream = -1;     // ConvArgs::epi_stream; -1 = by the size of the output
    bool offer_merge = true; // merged columns wherever the length maps allow them
    bool flat = true;        // false: a ragged batch on the dense grid (the plan's flat tile list is not taken)
    bool stats = false;      // statistics are wanted and the slots come later, sized from the plan (the model: ConvOpts::stat_part)
};

// Plan and kernel arguments of one launch.  Three things need a resource of the caller's, who is told by the plan: the
// pre-split image (plan.pre), the flat tile table (plan.flat_bn) and, under ConvCtx::stats, the statistics slots
// (plan.stat_cols); the setters fill in what depends on them.
struct ConvCall {
    ConvPlan plan;
    ConvArgs a;
    int B;
    size_t image_bytes() const { return conv16_pre_image_bytes(a.Cin, a.x_ld); }  // per utterance
    void set_image(const void* img, long img_bs) {  // (written by launch_split_image(a, ..))
        a.x16 = img;
        a.x16_bs = img_bs;
        a.x16_ld = a.x_ld;
    }
    // the flat tile list runs over these columns per utterance: flat_len() + flat_extra()
    const LenMap& flat_len() const { return a.store == ST_UPSCATTER ? a.in_len : a.out_len; }
    int flat_extra() const { return a.store == ST_UPSCATTER ? 1 : 0; }
    void set_flat(const int* tile_prefix, int tiles_host) {  // launch_tile_prefix's table and conv_tile_count of the same lengths
        a.tile_prefix = tile_prefix;
        a.flat_ny = (a.Cout + 127) / 128;
        a.flat_B = B;
        a.flat_tiles_host = tiles_host;
        a.flat_bn_host = plan.flat_bn;
    }
    void set_stats(float2* part) {  // [B][rows][plan.stat_tiles]
        a.stat_part = part;
        a.stat_tiles = plan.stat_tiles;
    }
};
ConvCall conv_call(const ConvW& w, const T& in, const T& out, const ConvOpts& o, const ConvCtx& ctx);
// column tiles of `bn` columns over a batch whose host lengths are h_lens (tile_prefix[B] as the host counts it)
int conv_tile_count(const int* h_lens, int B, const LenMap& lm, int extra, int bn);

// (KX_ERR_DEVICE class) a part of a resident-weights LSTM recurrence timed out waiting for its partner: the call is invalid,
// the model has switched to the streaming recurrence; host entry points re-run the call once
struct LstmTimeout : Error {
    explicit LstmTimeout(const std::string& m) : Error(3, m) {}
};

// sets a variable for a scope and puts its earlier value back on every way out
template <class V>
struct Restore {
    V& ref;
    V saved;
    Restore(V& r, V now) : ref(r), saved(r) { ref = now; }
    ~Restore() { ref = saved; }
    Restore(const Restore&) = delete;
};

class Model {
  public:
    Model(int device, int part = 0, int n_parts = 1);  // n_parts > 1: confined to CUs [part, part + 1) x CUs / n_parts
    ~Model();
    void load_file(const char* path);
    void load_device_blob(const void* d_blob, size_t n, bool adopt = false);
    // take ownership of a hipMalloc'd blob BEFORE parsing it, so that it is freed with the model even when the
    // build throws (kx_create_replicas)
    void adopt_blob_guard(void* d_blob) { blob_ = static_cast<char*>(d_blob); }

    void infer_device(const int64_t* d_ids, int64_t t_stride, const int32_t* lens_host, int B,
                      const float* d_styles, const float* speeds_host, int n_speed, uint64_t seed, uint32_t flags,
                      float* d_audio, int64_t audio_ld, int32_t* d_frames, int64_t* need_ld,
                      // device [B] each, valid for this call only: the host entries' per-row noise keys and stream indices
                      const uint64_t* d_utt_seeds = nullptr, const uint32_t* d_utt_index = nullptr);
    void infer_host(const int64_t* ids, int64_t t_stride, const int32_t* lens, int B, const float* styles,
                    const float* speeds, int n_speed, uint64_t seed, uint32_t flags, float** out,
                    int64_t* out_lens, const uint64_t* utt_seeds = nullptr);
    using HostCall = kx::HostCall;  // (host_request.h)
    using HostResults = kx::HostResults;
    void infer_host_ex(const int64_t* ids, int64_t t_stride, const int32_t* lens, int B, const float* speeds,
                       int n_speed, uint64_t seed, uint32_t flags, const HostCall& hc, const HostResults& res);
    // [0] recurrence in use: 0 = resident weights (two / four workgroups), 1 = the streaming fall-back; [1] hand-off time-outs so
    // far; [2] clean forwards left until the resident forms return (0 when they are in use); [3] calls re-run transparently
    void status(int64_t out[4]) const;
    // kx_infer_device + kx_sync: the forward finished cleanly (counts towards the resident forms' return)
    void note_clean_forward();
    void note_rerun() { n_rerun_ += 1; }
    static constexpr int LSTM_REARM_AFTER = 64;
    void set_voice_table(const float* table, int n_voices);
    int n_voices() const { return n_voices_.load(std::memory_order_acquire); }  // (read by the dispatcher without the mutex)
    int n_vocab() const { return n_vocab_; }                                    // (fixed once the model is built)
    void sync();
    void order_after_null_stream();
    void order_null_stream_after();
    void set_pinned(const int32_t* pattern, int n);
    // one forward of B utterances x n_tokens with every duration pinned to frames_per_token, output discarded: sizes the arenas,
    // the pooled page-locked buffer and the flat tile tables for that shape before the first real request
    void warmup(int B, int n_tokens, int frames_per_token);
    void arena_bytes(int64_t out[3]) const { out[0] = (int64_t)arenaT_.cap; out[1] = (int64_t)arenaF_.cap; out[2] = (int64_t)arenaIO_.cap; }
    // host-side milestones of the last infer_device call, ms from its entry: front half queued, front half done on the GPU (the
    // one host wait), back half planned, back half queued (= the call's return)
    void call_times(double out[4]) const { for (int i = 0; i < 4; ++i) out[i] = call_.ms[i]; }
    void profile_enable(bool on);
    void profile_read(int64_t* launches, double* ms, double* flops);
    struct ProfRec { int rows, Cin, K, dil, stride, store; double cols, flops; float ms; double bytes; };
    void profile_aux(int64_t* stats_launches, double* stats_bytes);  // unfused InstanceNorm statistics passes since the last read
    std::vector<ProfRec> prof_detail;  // filled by profile_read (one record per timed launch)
    // real-weights diagnostics: with diag on, every conv launch also measures its input (after the AdaIN affine)
    struct DiagRec { std::string name; int rows, Cin, K, act_shift; double absmax, rms, count; };
    void diag_enable(bool on);
    const std::vector<DiagRec>& diag_collect();  // syncs, converts the device slots of the last call(s)
    void set_act_shift(const std::string& conv_name, int shift);
    int get_act_shift(const std::string& conv_name) const;
    const Tap* find_tap(const std::string& name) const;

    int cu_partition(int* n_parts) const { *n_parts = n_parts_; return part_; }
    // [0] source variant (read_weight_file; -2 = built from a device blob: unknown), [1] 1 = the arithmetic is the reference's for
    // this file (fp32 / fp16 source or container), 0 = de-quantised weights run f32-class (NOT ORT's integer arithmetic),
    // [2] conv mode, [3] vocabulary rows, [4] voices in the device table, [5] CU partition, [6] partitions, [7] CUs of the model
    void info(int64_t out[8]) const;
    void set_source_variant(int v) { source_variant_ = v; }
    std::mutex mu;
    uint64_t utt_base = 0;
    void set_lanes(int n) { lanes_cfg_ = n < 0 ? 0 : (n > N_LANES ? N_LANES : n); }
    void set_conv_mode(int mode);  // (modes 5 / 6 build the bf16 / 8-bit cross weight images on first use)
    int conv_mode = CONV_F16F8;  // (default since round 5; KOKOROX_CONV=f16x3 / kx_set_conv_mode(1): three f16 MFMAs per product everywhere)
    int stft_variant = STFT_ONNX;  // the ONNX export's conv-based STFT pair (what the reference runs)
    int device;

  private:
    void build();  // pack weights, style-fc descriptors (table_ and blob_ are in place)
    const float* wt(const std::string& name) const;
    const TensorInfo& info(const std::string& name) const;
    bool has(const std::string& name) const { return table_.count(name) != 0; }
    float* dev_alloc(size_t floats);
    DevAlloc owned_alloc();  // hipMalloc'd, freed with the model
    ConvW make_conv(const std::string& name, bool bias = true);
    ConvW make_conv_cat(const std::vector<std::string>& names);
    ConvW make_convT(const std::string& name, int stride);
    LstmW make_lstm(const std::string& name);
    void add_fc(const std::string& key, const std::string& fc_name, int style_off);
    long fc_off(const std::string& key) const;

    void conv(const ConvW& w, const T& in, const T& out, const ConvOpts& o);
    void prof_begin(const ConvW& w, const T& in, const T& out, const ConvOpts& o);  // profile mode: the bracket around a timed launch
    void prof_end();
    void stats(const T& x, const std::string& fc_key);
    void adain_resblk(const std::string& name, const T& x, const T& out, bool upsample, float* ws_a, float* ws_b,
                      float* ws_c);
    void adain_resblock1(const std::string& name, int k, const T& x, const T& xj, const T& t1, const T& out,
                         int accum, float out_div, float2* part_t1, float2* part_xj, hipEvent_t wait_before_last = nullptr);
    void lstm(const LstmW& w, const T& in, const T& out, float* gx);
    void tap(const char* name, const T& t);
    void ensure_arena(Arena& a, size_t bytes);

    // Lanes of the back half: chains that do not depend on each other (the harmonic-source / noise path, the three
    // resblocks of a generator stage) are issued on streams of their own and meet through events, so that the HBM-bound
    // phases of one chain (epilogues, statistics passes, k = 3 convs) run under the matrix work of another.  Lane 0 is the
    // main stream.  Every lane has its own InstanceNorm parameter set (stats() writes it, the next conv reads it).
    static constexpr int N_LANES = 4;
    struct Lane {
        hipStream_t stream = nullptr;
        float *nmean = nullptr, *nscale = nullptr, *nshift = nullptr;
    };
    Lane lanes_[N_LANES];
    int lanes_cfg_ = 0;  // 0 = by batch size (4 up to 32 utterances, else 1), 1..4 = fixed (KX_LANES, kx_set_lanes)
    std::vector<hipEvent_t> lane_ev_;
    hipEvent_t record_here();               // a pooled event recorded on the current stream (null in the sizing pass)
    void wait_here(hipEvent_t e);           // the current stream waits for it
    struct LaneScope;                       // issue on lane k until the scope ends (model_forward.hip)
    struct DeviceTurn;                      // one forward at a time per GPU across models (model_forward.hip)
    void sync_lanes();

    int part_ = 0, n_parts_ = 1, cu_count_ = 0;  // cu_count_ = 0: the whole device
    int source_variant_ = -2;
    std::vector<uint32_t> cu_mask_;
    void new_stream(hipStream_t* s);
    hipStream_t stream_ = nullptr;
    // side stream for the TextEncoder branch, which does not depend on the ALBERT / duration branch
    hipStream_t stream2_ = nullptr;
    hipEvent_t ev_fork_ = nullptr, ev_join_ = nullptr;
    char* blob_ = nullptr;
    size_t blob_bytes_ = 0;
    TensorTable table_;
    std::vector<void*> owned_;
    std::map<std::string, ConvW> convs_;
    std::map<std::string, LstmW> lstms_;
    std::vector<FcDesc> fc_host_;
    std::map<std::string, long> fc_off_;
    FcDesc* fc_dev_ = nullptr;
    long gb_total_ = 0;
    int n_vocab_ = 178;  // rows of the two embedding tables (vocab.rs:5-20)

    Arena arenaT_, arenaF_, arenaIO_;
    float* d_voices_ = nullptr;  // [n_voices_][511][256]
    std::atomic<int> n_voices_{0};
    int* d_pinned_ = nullptr;
    int n_pinned_ = 0;

    // ---- per-call state: value-initialised when a forward starts (start_call), read until the next one does -----------
    struct PartInfo { const float2* part; int tiles, cols_per_tile, C; };
    // a flat tile list (ConvArgs::tile_prefix), one per (length map, tile width, stream)
    struct PrefixKey { const int* lens; int mul, add, bn; hipStream_t stream; const int* dev; };
    struct CallState {
        int B = 0, Tmax = 0, Fmax = 0;
        std::vector<int> hT, hF;           // host copies of the token / frame counts
        int *dT = nullptr, *dF = nullptr;  // the device's
        const int* d_dur = nullptr;        // [B][512] frames per token as the forward used them (token-axis arena: alive until the next call)
        bool taps_on = false;
        bool dry = false;        // sizing pass: allocate (count) but launch nothing
        bool p1_region = false;  // inside the part of the forward whose direct-A convs may run reduced precision
        std::map<const float*, PartInfo> parts;  // output tensor -> fused statistics partials of its producer
        std::vector<PrefixKey> prefix_keys;      // the flat tile lists belong to one call's lengths
        size_t prefix_used = 0;
        size_t lane_ev_used = 0;
        int n_lanes = 1;
        const uint64_t* d_utt_seeds = nullptr;  // per-utterance noise keys (infer_device's argument)
        const uint32_t* d_utt_index = nullptr;  // beside them: the utterance index of each row's stream (chunk c of a dispatched request)
        Arena* stats_arena = nullptr;  // where stats() keeps the raw sums of tensors it had to read (frame-axis arena)
        Arena* img_arena = nullptr;    // where conv() puts pre-split input images; non-null only while the back half is issued
        std::chrono::steady_clock::time_point t_enter;
        double ms[4] = {0, 0, 0, 0};   // call_times()
        void mark(int i) { ms[i] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_enter).count(); }
    };
    CallState call_;
    // the three steps of infer_device (model_forward.hip)
    void start_call(std::chrono::steady_clock::time_point t_enter, const int32_t* lens_host, int B, int Tmax, uint32_t flags,
                    const uint64_t* d_utt_seeds, const uint32_t* d_utt_index);
    struct Front {  // what the back half reads of the front half
        T dcat, t_en;
        const int* idx; int idx_ld, Tp;
        uint64_t seed; int noise_off;
        float* d_audio; int64_t audio_ld;
    };
    Front front_half(const int64_t* d_ids, int64_t t_stride, const int32_t* lens_host, const float* d_styles,
                     const float* speeds_host, int n_speed, uint64_t seed, uint32_t flags, float* d_audio, int64_t audio_ld,
                     int32_t* d_frames, int64_t* need_ld);
    void back_half(const Front& f, Arena& A);
    // host lengths behind a length map of the running call, and their sum in columns (+ extra per utterance)
    const std::vector<int>& host_lens(const LenMap& lm) const { return lm.lens == call_.dT ? call_.hT : call_.hF; }
    double host_cols(const LenMap& lm, int extra = 0) const {
        double cols = 0;
        for (int b = 0; b < call_.B; ++b) cols += (double)host_lens(lm)[b] * lm.mul + lm.add + extra;
        return cols;
    }
    // Sizes an arena by running `plan` on it in measure mode (dry: as a sizing pass of the launch sequence, nothing is
    // launched), grows it, then runs `plan` for real and returns what that returns.
    template <class Plan>
    auto plan_arena(Arena& A, bool dry, Plan&& plan) {
        {
            Restore<bool> measure(A.measure, true), dry_pass(call_.dry, dry);
            A.off = 0;
            plan(A);
        }
        ensure_arena(A, A.off);
        A.off = 0;
        return plan(A);
    }
    // two-CU LSTM: exchange buffers (one for the main stream, one for the TextEncoder branch that runs beside it) and the
    // sticky device error word (bit 1: a half never saw its partner) checked at every host synchronisation
    unsigned long long* d_xchg_[2] = {nullptr, nullptr};
    size_t xchg_cap_ = 0;
    unsigned xchg_epoch_[2] = {0, 0};  // launches on each exchange buffer since it was last cleared (16-bit tag epoch)
    bool lstm_pair_ok_ = true;         // false after a hand-off time-out: the streaming recurrence until lstm_rearm_in_ forwards were clean
    int lstm_rearm_in_ = 0;
    int64_t n_lstm_timeouts_ = 0, n_rerun_ = 0;
    void infer_host_once(const int64_t* ids, int64_t t_stride, const int32_t* lens, int B, const float* speeds, int n_speed,
                         uint64_t seed, uint32_t flags, const HostCall& hc, const HostResults& res);
    // The running host call's prosody on the device (include/kokorox_hip.h, "prosody"): infer_host_once sets it around its forward,
    // front_half and back_half read it.  All null: a plain call, which launches what it always launched.
    struct ProsodyDev {
        const float* rate = nullptr;    // [B][stride] each, as the ids
        const int* frames = nullptr;
        const float* pitch = nullptr;
        const float* energy = nullptr;
        long stride = 0;
        const long* rep_first = nullptr;  // [B] first token of row b in `report`, -1: none (null with report)
        float* report = nullptr;          // [tokens][4], staged in the I/O arena and copied behind the packed blocks
        // a call with fit spans (include/kokorox_hip.h, "fit"): then `rate` is [B][512] (dur_stride), `frames` stays [B][stride]
        long dur_stride = 0;                  // stride of `rate`, and of `frames` as the duration kernel reads it
        int n_spans = 0;
        const int* fit_prefix = nullptr;      // [B + 1] running sum of lens
        const FitFlat* fit_spans = nullptr;   // [n_spans] in that flat token space
        float* fit_w = nullptr;               // [B][512] weights
        int* fit_fitted = nullptr;            // [B][512] fixed counts of the call: the caller's, then the fitted ones
        FitResult* fit_results = nullptr;     // [n_spans]
        bool durations() const { return rate || frames || n_spans > 0; }
        bool curves() const { return pitch || energy || report; }
    };
    ProsodyDev pros_;
    std::vector<long> h_rep_first_;  // host side of ProsodyDev::rep_first (outlives the asynchronous copy)
    FitPlan fit_plan_;                    // host side of the running call's fit (outlives the asynchronous copies)
    std::vector<float> h_fit_rate_;       // the call's rate laid out [B][512]
    std::vector<FitResult> h_fit_results_;  // what front_half brings back in front of its host wait
    // host staging that asynchronous copies read / write: outlives the calling frame
    OutputPlan output_plan_;           // the tables of the running call's output stage: requests, prefixes, joins, marks, levels
    bool want_edges_ = false;          // the running host call has joins: front_half brings the rows' edge durations back
    std::vector<int> h_edge_;          // [B][2] used durations of every row's first and last token (valid when want_edges_)
    unsigned h_bad_id_ = 0;
    unsigned h_dur_over_ = 0;
    unsigned* d_dev_err_ = nullptr;
    unsigned* h_words_ = nullptr;    // page-locked: [0] the device error word as read back
    int* h_stage_ = nullptr;         // page-locked scratch of the small per-call host arrays (stage_ints)
    size_t h_stage_cap_ = 0;
    int* stage_ints(size_t n);
    hipEvent_t ev_null_ = nullptr;   // orders kx_infer_device's inputs after the caller's null-stream work
    hipEvent_t ev_done_ = nullptr;   // ... and the caller's later null-stream work after the forward (order_null_stream_after)
    hipStream_t main_stream_ = nullptr;
    void check_dev_err();
    unsigned* d_bad_id_ = nullptr;  // sticky word: first out-of-table token id seen by the embedding kernels
    unsigned* d_dur_over_ = nullptr;  // sticky word: first utterance whose durations did not fit its row of the alignment (duration_kernel)
    float* gb_ = nullptr;  // [B][gb_total_]
    float *nmean_ = nullptr, *nscale_ = nullptr, *nshift_ = nullptr;
    int n_bs_ = 0;
    std::map<std::string, Tap> taps_;

    int* d_prefix_ = nullptr;  // device block of the flat tile lists (CallState::prefix_keys)
    size_t prefix_cap_ = 0;
    const int* tile_prefix_for(const LenMap& lm, int extra, int bn, int* total);

    bool diag_on_ = false;
    std::vector<DiagRec> diag_recs_;
    float* d_diag_ = nullptr;  // [diag_cap_][3]
    size_t diag_cap_ = 0, diag_used_ = 0;
    bool prof_on_ = false;
    std::vector<hipEvent_t> ev_;
    size_t ev_used_ = 0;
    double prof_flops_ = 0.0;
    std::vector<ProfRec> prof_recs_;
    int64_t prof_launches_ = 0;
    int64_t prof_stats_launches_ = 0;
    double prof_stats_bytes_ = 0.0;
};

}  // namespace kx
