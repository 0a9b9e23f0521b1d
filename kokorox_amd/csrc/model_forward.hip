// The forward of the MI355X Kokoro-82M model: the launch sequence that replaces `sess.run`
// (kokorox/src/onn/ort_koko.rs:79), its lanes and the per-call tables.  The graph is the published Kokoro-82M (SURVEY.md
// Appendix A.2); stage comments name the upstream module.
#include "model.h"

#include <chrono>
#include <cstdlib>

namespace kx {

static constexpr float RSQRT2 = 0.70710678118654752f;
// row strides are multiples of 32 floats: every 32-column half-wave store of the conv epilogue is one whole
// 128-byte line (arenas are 256-byte aligned)
static inline int up4(int x) { return (x + 31) & ~31; }

// CUs of the launches this thread is issuing: the device's, or the model's share of them (CU-partitioned models)
static thread_local int tl_cu_override = 0;
int cu_count_override() { return tl_cu_override; }
struct CuScope {
    int saved;
    explicit CuScope(int n) : saved(tl_cu_override) { tl_cu_override = n; }
    ~CuScope() { tl_cu_override = saved; }
};

// ---- lanes (model.h) ---------------------------------------------------------------------------
hipEvent_t Model::record_here() {
    if (call_.dry) return nullptr;
    if (call_.lane_ev_used == lane_ev_.size()) {
        hipEvent_t e;
        KX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        lane_ev_.push_back(e);
    }
    hipEvent_t e = lane_ev_[call_.lane_ev_used++];
    KX_HIP(hipEventRecord(e, stream_));
    return e;
}

void Model::wait_here(hipEvent_t e) {
    if (call_.dry || !e) return;
    KX_HIP(hipStreamWaitEvent(stream_, e, 0));
}

void Model::sync_lanes() {
    for (int i = 1; i < N_LANES; ++i)
        if (lanes_[i].stream) (void)hipStreamSynchronize(lanes_[i].stream);
}

// Everything issued inside the scope goes to lane k (its stream, its InstanceNorm parameter set), which first waits for
// what the issuing stream has queued so far.  Leaving the scope joins nothing: chains meet through record_here / wait_here.
struct Model::LaneScope {
    Model& m;
    hipStream_t s0;
    float *a0, *b0, *c0;
    LaneScope(Model& mm, int k) : m(mm), s0(mm.stream_), a0(mm.nmean_), b0(mm.nscale_), c0(mm.nshift_) {
        const Lane& L = m.lanes_[k < m.call_.n_lanes ? k : 0];
        if (L.stream == m.stream_) return;
        hipEvent_t e = m.record_here();
        m.stream_ = L.stream;
        m.nmean_ = L.nmean;
        m.nscale_ = L.nscale;
        m.nshift_ = L.nshift;
        m.wait_here(e);
    }
    ~LaneScope() {
        m.stream_ = s0;
        m.nmean_ = a0;
        m.nscale_ = b0;
        m.nshift_ = c0;
    }
};

void Model::conv(const ConvW& w, const T& in, const T& out, const ConvOpts& o) {
    // Plan and kernel arguments (conv_call.hip): also in the dry run, which plans the pre-split input images like every other
    // buffer of the back half
    ConvCtx ctx;
    ctx.mode = conv_mode;
    ctx.p1_region = call_.p1_region;
    ctx.B = call_.B;
    ctx.cus = call_.dry ? 0 : conv16_cu_count();  // (the dry run needs the image only, which does not depend on it)
    ctx.n_bs = n_bs_;
    ctx.image = call_.img_arena ? 1 : 0;
    ConvCall call = conv_call(w, in, out, o, ctx);
    const ConvPlan& plan = call.plan;
    const long x16_bs = plan.pre ? (long)call.image_bytes() : 0;
    void* x16 = plan.pre ? call_.img_arena->alloc((size_t)call_.B * x16_bs) : nullptr;
    if (call_.dry) return;
    if (diag_on_ && diag_used_ < diag_cap_) {
        float* slot = d_diag_ + 3 * diag_used_++;
        launch_diag_stats(in.p, in.bs, in.ld, w.Cin, in.len, call_.B, in.Lmax, o.nmean, o.nscale, o.nshift, n_bs_, slot, stream_);
        diag_recs_.push_back(DiagRec{w.name, w.rows, w.Cin, w.K, w.act_shift, 0.0, 0.0, 0.0});
    }
    call_.parts.erase(out.p);  // whatever statistics were known for this tensor are stale now
    if (plan.stat_cols) call_.parts[out.p] = PartInfo{o.stat_part, plan.stat_tiles, plan.stat_cols, w.rows};
    // ragged batch: the direct-A kernels take a flat list of the live tiles instead of a (longest length) x B grid
    if (plan.flat_bn) {
        int total = 0;
        const int* prefix = tile_prefix_for(call.flat_len(), call.flat_extra(), plan.flat_bn, &total);
        call.set_flat(prefix, total);
        if (total <= 0) return;  // (nothing to compute)
    }
    if (x16) {
        // (outside the timed interval of the profile mode: that one is the conv kernel's own duration, which the rocprofv3
        // summary of the same kernel name must reproduce; the pass shows up under its own name there and in ms_per_step)
        launch_split_image(call.a, call_.B, in.Lmax, x16, x16_bs, stream_);
        call.set_image(x16, x16_bs);
    }
    // timed: the dominant kernel family, every 128-row conv / GEMM launch (direct-A, direct-A GEMM, LDS-DMA forms; f32 mode:
    // conv1d_mfma_kernel<128,128,2,2>)
    const bool timed = prof_on_ && w.BM == 128;
    if (timed) prof_begin(w, in, out, o);
    launch_conv(plan, call.a, call_.B, stream_);
    if (timed) prof_end();
}

// The device prefix table of (length map, extra columns, tile width) for the running call: built once per call and key by a
// one-thread kernel on the current stream, from the same device lengths the kernels read; *total = its last entry, counted
// on the host from the host copies of those lengths (the grid size).
const int* Model::tile_prefix_for(const LenMap& lm, int extra, int bn, int* total) {
    KX_REQUIRE(lm.lens == call_.dT || lm.lens == call_.dF, "internal: tile prefix of an unknown length array");
    *total = conv_tile_count(host_lens(lm).data(), call_.B, lm, extra, bn);
    for (const PrefixKey& k : call_.prefix_keys)
        if (k.lens == lm.lens && k.mul == lm.mul && k.add == lm.add + extra && k.bn == bn && k.stream == stream_) return k.dev;
    const size_t need = (size_t)(call_.B + 1);
    if (call_.prefix_used + need > prefix_cap_) {  // (grown like the arenas; tables of this call that are in use stay where they are)
        const size_t want = std::max<size_t>(prefix_cap_ * 2, (size_t)64 * need);
        int* p = nullptr;
        KX_HIP(hipMalloc((void**)&p, want * sizeof(int)));
        owned_.push_back(p);  // (the old block stays alive until the model goes: launches of this call may still read it)
        d_prefix_ = p;
        prefix_cap_ = want;
        call_.prefix_used = 0;
    }
    int* dev = d_prefix_ + call_.prefix_used;
    call_.prefix_used += need;
    launch_tile_prefix(lm, extra, bn, call_.B, dev, stream_);
    // (keyed by stream too: a table built on one lane's stream is ordered before that lane's launches only)
    call_.prefix_keys.push_back(PrefixKey{lm.lens, lm.mul, lm.add + extra, bn, stream_, dev});
    return dev;
}

void Model::stats(const T& x, const std::string& fc_key) {
    // a tensor whose sums are not known yet gets a small cache for them (planned in the dry run like everything else)
    float2* raw = call_.stats_arena ? reinterpret_cast<float2*>(call_.stats_arena->alloc((size_t)call_.B * x.C * 2 * sizeof(float2))) : nullptr;
    if (call_.dry) return;
    auto it = call_.parts.find(x.p);
    if (it != call_.parts.end() && it->second.C == x.C) {
        const PartInfo& pi = it->second;
        launch_stats_finalize(pi.part, pi.tiles, pi.cols_per_tile, x.C, x.len, call_.B, gb_ + fc_off(fc_key), gb_total_,
                              nmean_, nscale_, nshift_, n_bs_, stream_);
        return;
    }
    if (prof_on_) {  // (the PMC tooling checks FETCH_SIZE of this kernel against these bytes: it reads x exactly once)
        prof_stats_bytes_ += 4.0 * x.C * host_cols(x.len);
        prof_stats_launches_ += 1;
    }
    launch_in_stats(x.p, x.bs, x.ld, x.C, x.len, call_.B, gb_ + fc_off(fc_key), gb_total_, nmean_, nscale_, nshift_, n_bs_,
                    raw, stream_);
    // (two "tiles": the high and the low part of the f64 sums, both read back whatever the length)
    if (raw) call_.parts[x.p] = PartInfo{raw, 2, STAT_RAW_TILES, x.C};
}

void Model::tap(const char* name, const T& t) {
    if (!call_.taps_on || call_.dry) return;
    KX_HIP(hipStreamSynchronize(stream_));
    Tap tp;
    tp.B = call_.B;
    tp.C = t.C;
    tp.ld = t.ld;
    tp.data.resize((size_t)call_.B * t.C * t.ld);
    for (int b = 0; b < call_.B; ++b) {
        tp.L.push_back(host_lens(t.len)[b] * t.len.mul + t.len.add);
        KX_HIP(hipMemcpy(tp.data.data() + (size_t)b * t.C * t.ld, t.p + (long)b * t.bs, (size_t)t.C * t.ld * 4,
                         hipMemcpyDeviceToHost));
    }
    taps_[name] = std::move(tp);
}

void Model::lstm(const LstmW& w, const T& in, const T& out, float* gx) {
    if (call_.dry) return;
    const T g = T::of(gx, 2048, 2048, in.len, in.Lmax, (long)in.Lmax * 2048);
    ConvOpts o;
    o.store = ST_TMAJOR;
    conv(w.ih, in, g, o);
    // (after a timed-out hand-off the model stays on the one-CU kernel: see check_dev_err)
    const int xb = stream_ == main_stream_ ? 0 : 1;
    launch_lstm(gx, g.bs, 2048, w.whhT, out.p, out.bs, out.ld, in.len, call_.B, lstm_pair_ok_ ? d_xchg_[xb] : nullptr,
                d_dev_err_, stream_, &xchg_epoch_[xb]);
}

// AdainResBlk1d (istftnet.py): out = (conv2(act(norm2(conv1(pool(act(norm1(x))))))) + shortcut(x)) / sqrt(2)
void Model::adain_resblk(const std::string& name, const T& x, const T& out, bool upsample, float* ws_a, float* ws_b,
                         float* ws_c) {
    const ConvW& c1 = convs_.at(name + ".conv1");
    const ConvW& c2 = convs_.at(name + ".conv2");
    T t1 = out;
    t1.p = ws_a;
    t1.bs = (long)out.C * out.ld;
    // the 1x1 shortcut depends on x only: it is issued first, on a side lane, and joins before conv2 reads it
    T sc = out;
    const T* res = &x;
    hipEvent_t ev_sc = nullptr;
    if (convs_.count(name + ".conv1x1")) {
        sc.p = ws_b;
        sc.bs = (long)out.C * out.ld;
        ConvOpts osc;
        osc.in_up2 = upsample ? 1 : 0;
        {
            LaneScope side(*this, 2);
            conv(convs_.at(name + ".conv1x1"), x, sc, osc);
            ev_sc = record_here();
        }
        res = &sc;
    } else {
        KX_REQUIRE(!upsample && x.C == out.C, "internal: identity shortcut needs equal shapes");
    }
    // InstanceNorm partial sums of t1 (normalised by norm2 below) and of the block's output (normalised by the next block's
    // norm1 when that block reads exactly this tensor) leave the conv epilogues, as in the generator: no separate pass
    auto part_for = [&](const T& t) -> float2* {
        const size_t n = (size_t)call_.B * t.C * (t.Lmax / 64 + 4);
        return call_.stats_arena ? static_cast<float2*>(call_.stats_arena->alloc(n * sizeof(float2))) : nullptr;
    };
    float2* part_t1 = part_for(t1);
    float2* part_out = part_for(out);
    stats(x, name + ".norm1");
    if (!upsample) {
        ConvOpts o;
        o.nmean = nmean_; o.nscale = nscale_; o.nshift = nshift_;
        o.act = ACT_LEAKY; o.slope = 0.2f; o.pad = 1;
        o.stat_part = part_t1;
        conv(c1, x, t1, o);
    } else {
        T p = out;
        p.p = ws_c;
        p.C = x.C;
        p.bs = (long)x.C * out.ld;
        if (!call_.dry)
            launch_pool_up2(x.p, x.bs, x.ld, x.C, nmean_, nscale_, nshift_, n_bs_, 0.2f, wt(name + ".pool.weight"),
                            wt(name + ".pool.bias"), p.p, p.bs, p.ld, x.len, call_.B, x.Lmax, stream_);
        ConvOpts o;
        o.pad = 1;
        o.stat_part = part_t1;
        conv(c1, p, t1, o);
    }
    stats(t1, name + ".norm2");
    ConvOpts o;
    o.nmean = nmean_; o.nscale = nscale_; o.nshift = nshift_;
    o.act = ACT_LEAKY; o.slope = 0.2f; o.pad = 1;
    o.resid = res;
    o.out_mul = RSQRT2;
    o.stat_part = part_out;
    wait_here(ev_sc);  // (the shortcut ran beside conv1)
    conv(c2, t1, out, o);
}

// AdaINResBlock1 with Snake1D (istftnet.py).  x is read-only; xj/t1 are scratch of x's shape;
// the third iteration lands in `out` (optionally accumulated and divided: mean over kernels).
void Model::adain_resblock1(const std::string& name, int k, const T& x, const T& xj, const T& t1, const T& out,
                            int accum, float out_div, float2* part_t1, float2* part_xj, hipEvent_t wait_before_last) {
    static const int dils[3] = {1, 3, 5};
    for (int i = 0; i < 3; ++i) {
        const std::string s = std::to_string(i);
        const T& cur = (i == 0) ? x : xj;
        const T& dst = (i == 2) ? out : xj;
        stats(cur, name + ".adain1." + s);
        ConvOpts o1;
        o1.nmean = nmean_; o1.nscale = nscale_; o1.nshift = nshift_;
        o1.act = ACT_SNAKE;
        o1.alpha = call_.dry ? nullptr : wt(name + ".alpha1." + s);
        o1.dil = dils[i];
        o1.pad = (k * dils[i] - dils[i]) / 2;
        o1.stat_part = part_t1;  // t1 is normalised by adain2 next
        conv(convs_.at(name + ".convs1." + s), cur, t1, o1);
        stats(t1, name + ".adain2." + s);
        ConvOpts o2;
        o2.nmean = nmean_; o2.nscale = nscale_; o2.nshift = nshift_;
        o2.act = ACT_SNAKE;
        o2.alpha = call_.dry ? nullptr : wt(name + ".alpha2." + s);
        o2.pad = (k - 1) / 2;
        o2.resid = &cur;
        if (i == 2) {
            o2.accum = accum;
            o2.out_div = out_div;
            wait_here(wait_before_last);  // (the running sum this conv adds to is written by another lane)
        } else {
            o2.stat_part = part_xj;  // xj is normalised by the next iteration's adain1
        }
        conv(convs_.at(name + ".convs2." + s), t1, dst, o2);
    }
}

// ---- one forward at a time per GPU, across the models that live on it -------------------------------------------------
// Models are meant to be one per GPU, but nothing stops a process from holding several on one device (kx_create_replicas with
// repeated ids, tests).  Their streams are non-blocking, so their kernels would run side by side - and the two-CU recurrence
// does not survive that: its 1024-thread, 134 KB-LDS workgroups need a whole CU free at once, the other model's 256-thread conv
// workgroups refill every slot that frees, and a recurrence's second half can starve until the first half's bounded poll gives
// up (measured: a 1 - 2 s stall, KX_ERR_DEVICE, fall-back to the one-CU kernel; profiles/r04_serve_models_per_gpu.txt).  So the
// forwards of the models of one device take turns: a forward's first launch waits (on the GPU, by an event) for the end of
// the previous forward of ANOTHER model on that device, and the host side queues one forward at a time per device.  With one
// model per device this is one uncontended mutex and one event record per forward.
namespace {
struct DeviceGate {
    std::mutex mu;
    hipEvent_t last = nullptr;   // end of the most recent forward queued on this device
    const void* owner = nullptr; // the model that queued it
};
DeviceGate& device_gate(int dev) {
    static DeviceGate g[KX_MAX_DEVICES];
    if (dev < 0 || dev >= KX_MAX_DEVICES) throw Error(1, "device id outside 0.." + std::to_string(KX_MAX_DEVICES - 1));  // (the Model constructor refuses such ids)
    return g[dev];
}
// KX_DEVICE_TURN=0: the models of one device run their forwards side by side (tests; see kx_model_status for what then happens
// to a starved recurrence)
bool device_turn_on() {
    static const bool on = !(getenv("KX_DEVICE_TURN") && atoi(getenv("KX_DEVICE_TURN")) == 0);
    return on;
}
}  // namespace

struct Model::DeviceTurn {
    Model& m;
    DeviceGate& g;
    std::unique_lock<std::mutex> lk;
    const bool on;
    // (CU-partitioned models never compete for a CU: they do not take turns)
    explicit DeviceTurn(Model& mm) : m(mm), g(device_gate(mm.device)), lk(g.mu, std::defer_lock), on(device_turn_on() && mm.n_parts_ == 1) {
        if (!on) return;
        lk.lock();
        if (g.last && g.owner != &m) KX_HIP(hipStreamWaitEvent(m.main_stream_, g.last, 0));
    }
    ~DeviceTurn() {  // (also on a failed forward: whatever it queued is what the next model has to wait for)
        if (!on) return;
        if (!g.last && hipEventCreateWithFlags(&g.last, hipEventDisableTiming) != hipSuccess) g.last = nullptr;
        if (g.last && hipEventRecord(g.last, m.main_stream_) == hipSuccess) g.owner = &m;
        else g.owner = nullptr;
    }
};

// ---- step 1: the per-call state starts afresh; the exchange buffers of the two-CU LSTM grow like the arenas -----------------
void Model::start_call(std::chrono::steady_clock::time_point t_enter, const int32_t* lens_host, int B, int Tmax, uint32_t flags,
                       const uint64_t* d_utt_seeds, const uint32_t* d_utt_index) {
    // (the three vectors keep their capacity from call to call: no host allocation in a steady stream of calls)
    std::vector<int> hT = std::move(call_.hT), hF = std::move(call_.hF);
    std::vector<PrefixKey> keys = std::move(call_.prefix_keys);
    keys.clear();
    call_ = CallState{};
    call_.hT = std::move(hT);
    call_.hF = std::move(hF);
    call_.prefix_keys = std::move(keys);
    call_.t_enter = t_enter;
    call_.B = B;
    call_.Tmax = Tmax;
    call_.taps_on = (flags & 2u) != 0;
    call_.d_utt_seeds = d_utt_seeds;
    call_.d_utt_index = d_utt_index;
    taps_.clear();
    // Measured (profiles/r03_lanes_dephase.txt): side-by-side chains take 15 % off the batch-1 step (small grids leave CUs
    // idle: 14.1 -> 11.9 ms), 14 % at batch 4, 6 % at batch 16; at batch 64 every launch fills the chip and they change
    // nothing (125.1 vs 125.1 ms) while the per-launch event timings of the profile mode would overlap.  So: lanes for
    // small batches only.
    // (with the per-launch event timing on, one lane: intervals recorded on overlapping streams would be summed side by side)
    call_.n_lanes = prof_on_ ? 1 : (lanes_cfg_ ? lanes_cfg_ : (B <= 32 ? N_LANES : 1));
    call_.hT.assign(lens_host, lens_host + B);
    call_.hF.assign(B, 0);
    n_bs_ = 1104;
    if (lstm_exchange_bytes(B) > xchg_cap_) {
        KX_HIP(hipStreamSynchronize(stream_));
        for (auto*& p : d_xchg_) {
            if (p) KX_HIP(hipFree(p));
            p = nullptr;
            KX_HIP(hipMalloc((void**)&p, lstm_exchange_bytes(B)));
            KX_HIP(hipMemsetAsync(p, 0, lstm_exchange_bytes(B), stream_));  // (stream-ordered before the first recurrence)
        }
        xchg_cap_ = lstm_exchange_bytes(B);
        xchg_epoch_[0] = xchg_epoch_[1] = 0;
    }
}

// ---- step 2, the front half: everything on the token axis, up to the one host round trip ---------------------------------
Model::Front Model::front_half(const int64_t* d_ids, int64_t t_stride, const int32_t* lens_host, const float* d_styles,
                               const float* speeds_host, int n_speed, uint64_t seed, uint32_t flags, float* d_audio,
                               int64_t audio_ld, int32_t* d_frames, int64_t* need_ld) {
    const int B = call_.B, Tmax = call_.Tmax;
    const int Tp = up4(Tmax);
    const int idx_ld = Tmax * 50;
    float *emb, *h, *qkv, *ctx, *av, *ff, *dcat, *gxT, *gxT2, *xl, *logits, *te0, *te1, *t_en, *d_speeds;
    int *dur, *idx, *d_edge = nullptr;
    plan_arena(arenaT_, false, [&](Arena& A) {
        call_.dT = A.i(B);
        call_.dF = A.i(B);
        if (want_edges_) d_edge = A.i((size_t)2 * B);  // (a call with joins: every row's two edge durations)
        d_bad_id_ = reinterpret_cast<unsigned*>(A.i(1));
        d_dur_over_ = reinterpret_cast<unsigned*>(A.i(1));
        d_speeds = A.f(B);
        dur = A.i((size_t)B * 512);
        call_.d_dur = dur;
        idx = A.i((size_t)B * idx_ld);
        gb_ = A.f((size_t)B * gb_total_);
        nmean_ = A.f((size_t)B * n_bs_);
        nscale_ = A.f((size_t)B * n_bs_);
        nshift_ = A.f((size_t)B * n_bs_);
        lanes_[0].nmean = nmean_;
        lanes_[0].nscale = nscale_;
        lanes_[0].nshift = nshift_;
        for (int i = 1; i < N_LANES; ++i) {
            lanes_[i].nmean = A.f((size_t)B * n_bs_);
            lanes_[i].nscale = A.f((size_t)B * n_bs_);
            lanes_[i].nshift = A.f((size_t)B * n_bs_);
        }
        const size_t bt = (size_t)B * Tp;
        emb = A.f(bt * 128);
        h = A.f(bt * 768);
        qkv = A.f(bt * 2304);
        ctx = A.f(bt * 768);
        av = A.f(bt * 768);
        ff = A.f(bt * 2048);
        dcat = A.f(bt * 640);
        gxT = A.f(bt * 2048);
        gxT2 = A.f(bt * 2048);  // LSTM input products of the TextEncoder branch (side stream)
        xl = A.f(bt * 512);
        logits = A.f(bt * 50);
        te0 = A.f(bt * 512);
        te1 = A.f(bt * 512);
        t_en = A.f(bt * 512);
    });

    KX_HIP(hipMemcpyAsync(call_.dT, lens_host, B * sizeof(int), hipMemcpyHostToDevice, stream_));
    KX_HIP(hipMemsetAsync(d_bad_id_, 0, sizeof(unsigned), stream_));
    KX_HIP(hipMemsetAsync(d_dur_over_, 0, sizeof(unsigned), stream_));
    KX_HIP(hipMemcpyAsync(d_speeds, speeds_host, n_speed * sizeof(float), hipMemcpyHostToDevice, stream_));
    const LenMap LT{call_.dT, 1, 0};
    auto TT = [&](float* p, int C) { return T::of(p, C, Tp, LT, Tmax); };
    launch_style_fc(fc_dev_, (int)fc_host_.size(), d_styles, gb_, gb_total_, B, stream_);

    // --- TextEncoder (embedding, 3 x conv k5 + LayerNorm + LeakyReLU, biLSTM) ---
    // Independent of the ALBERT / duration branch below: it runs on the side stream beside it (at small batch
    // neither branch fills the chip: the recurrences use one CU per utterance and direction).
    KX_HIP(hipEventRecord(ev_fork_, stream_));
    KX_HIP(hipStreamWaitEvent(stream2_, ev_fork_, 0));
    T t_ten = TT(t_en, 512);
    {
    Restore<hipStream_t> on_side(stream_, stream2_);  // every launch helper issues on stream_: the side stream, for this block
    T t_te0 = TT(te0, 512), t_te1 = TT(te1, 512);
    launch_embed(d_ids, t_stride, wt("text_encoder.embedding.weight"), 512, te0, t_te0.bs, Tp, call_.dT, B, Tmax, n_vocab_,
                 d_bad_id_, stream_);
    T* cur = &t_te0;
    T* nxt = &t_te1;
    for (int i = 0; i < 3; ++i) {
        ConvOpts o;
        o.pad = 2;
        conv(convs_.at("text_encoder.cnn." + std::to_string(i)), *cur, *nxt, o);
        const std::string ln = "text_encoder.cnn." + std::to_string(i) + ".1.";
        launch_layernorm_ch(nxt->p, nxt->p, nxt->bs, Tp, 512, LT, B, Tmax, 1e-5f, LN_AFFINE, wt(ln + "gamma"),
                            wt(ln + "beta"), 0, 0.2f, stream_);
        std::swap(cur, nxt);
    }
    tap("text_enc.cnn", *cur);
    lstm(lstms_.at("text_encoder.lstm"), *cur, t_ten, gxT2);
    tap("text_enc.out", t_ten);
    KX_HIP(hipEventRecord(ev_join_, stream_));
    }

    // --- PL-BERT (ALBERT, 12 passes over one shared layer) ---
    const std::string E = "bert.embeddings.";
    const std::string AL = "bert.encoder.albert_layer_groups.0.albert_layers.0.";
    T t_emb = TT(emb, 128), t_h = TT(h, 768), t_qkv = TT(qkv, 2304), t_ctx = TT(ctx, 768), t_a = TT(av, 768),
      t_f = TT(ff, 2048);
    launch_albert_embed(d_ids, t_stride, wt(E + "word_embeddings.weight"), wt(E + "token_type_embeddings.weight"),
                        wt(E + "position_embeddings.weight"), emb, t_emb.bs, Tp, call_.dT, B, Tmax, n_vocab_, d_bad_id_, stream_);
    launch_layernorm_ch(emb, emb, t_emb.bs, Tp, 128, LT, B, Tmax, 1e-12f, LN_AFFINE, wt(E + "LayerNorm.weight"),
                        wt(E + "LayerNorm.bias"), 0, 0.f, stream_);
    tap("bert.emb", t_emb);
    conv(convs_.at("bert.map"), t_emb, t_h, ConvOpts{});
    for (int l = 0; l < 12; ++l) {
        conv(convs_.at("bert.qkv"), t_h, t_qkv, ConvOpts{});
        launch_attention(qkv, t_qkv.bs, Tp, ctx, t_ctx.bs, Tp, call_.dT, B, Tmax, stream_);
        ConvOpts od;
        od.resid = &t_h;
        conv(convs_.at("bert.dense"), t_ctx, t_a, od);
        launch_layernorm_ch(av, av, t_a.bs, Tp, 768, LT, B, Tmax, 1e-12f, LN_AFFINE,
                            wt(AL + "attention.LayerNorm.weight"), wt(AL + "attention.LayerNorm.bias"), 0, 0.f, stream_);
        ConvOpts of;
        of.epi = EPI_GELU_NEW;
        conv(convs_.at("bert.ffn"), t_a, t_f, of);
        ConvOpts oo;
        oo.resid = &t_a;
        conv(convs_.at("bert.ffn_out"), t_f, t_h, oo);
        launch_layernorm_ch(h, h, t_h.bs, Tp, 768, LT, B, Tmax, 1e-12f, LN_AFFINE,
                            wt(AL + "full_layer_layer_norm.weight"), wt(AL + "full_layer_layer_norm.bias"), 0, 0.f,
                            stream_);
        if (l == 0) tap("bert.layer0", t_h);
    }
    tap("bert.out", t_h);

    // --- bert_encoder + DurationEncoder (3 x biLSTM + AdaLayerNorm) + duration head ---
    T t_dcat = TT(dcat, 640);
    T t_d512 = t_dcat.rows(0, 512);
    conv(convs_.at("bert_encoder"), t_h, t_d512, ConvOpts{});
    tap("d_en", t_d512);
    launch_fill_style_rows(dcat, t_dcat.bs, Tp, 512, d_styles, 128, call_.dT, B, Tmax, stream_);
    for (int i = 0; i < 3; ++i) {
        lstm(lstms_.at("predictor.text_encoder.lstms." + std::to_string(2 * i)), t_dcat, t_d512, gxT);
        const float* g = gb_ + fc_off("dur_enc." + std::to_string(i));
        launch_layernorm_ch(dcat, dcat, t_dcat.bs, Tp, 512, LT, B, Tmax, 1e-5f, LN_ADA, g, g + 512, (int)gb_total_, 0.f,
                            stream_);
        tap(("dur_enc." + std::to_string(i)).c_str(), t_dcat);
    }
    T t_xl = TT(xl, 512), t_logits = TT(logits, 50);
    lstm(lstms_.at("predictor.lstm"), t_dcat, t_xl, gxT);
    tap("dur.lstm", t_xl);
    conv(convs_.at("duration_proj"), t_xl, t_logits, ConvOpts{});
    if (pros_.n_spans > 0) {
        // a call with fit spans: every token's weight, then one workgroup a span finds the span's lambda and writes the fitted counts
        // beside the caller's fixed ones; the duration kernel takes them as its fixed array and everything downstream follows
        launch_fit_weights(logits, t_logits.bs, Tp, d_speeds, n_speed, call_.dT, pros_.rate, pros_.dur_stride, pros_.frames, pros_.stride,
                           pros_.fit_w, pros_.fit_fitted, B, stream_);
        launch_fit_spans(pros_.fit_prefix, B, pros_.fit_spans, pros_.n_spans, pros_.fit_w, pros_.fit_fitted, pros_.fit_results, stream_);
        launch_prosody_duration(logits, t_logits.bs, Tp, d_speeds, n_speed, call_.dT, d_pinned_, n_pinned_, pros_.rate, pros_.fit_fitted,
                                pros_.dur_stride, dur, call_.dF, idx, idx_ld, d_dur_over_, B, stream_);
        h_fit_results_.assign((size_t)pros_.n_spans, FitResult{});
        KX_HIP(hipMemcpyAsync(h_fit_results_.data(), pros_.fit_results, (size_t)pros_.n_spans * sizeof(FitResult), hipMemcpyDeviceToHost,
                              stream_));
        tap("pred.dur.weights", T::of(pros_.fit_w, 1, 512, LT, Tmax));
        tap("pred.dur.fitted", T::of(reinterpret_cast<float*>(pros_.fit_fitted), 1, 512, LT, Tmax));  // (int32 bits)
    } else if (pros_.durations())  // (a call with a per-token rate or fixed frame counts: the restated kernel; the plain call keeps its own)
        launch_prosody_duration(logits, t_logits.bs, Tp, d_speeds, n_speed, call_.dT, d_pinned_, n_pinned_, pros_.rate, pros_.frames,
                                pros_.dur_stride, dur, call_.dF, idx, idx_ld, d_dur_over_, B, stream_);
    else
        launch_duration(logits, t_logits.bs, Tp, d_speeds, n_speed, call_.dT, d_pinned_, n_pinned_, dur, call_.dF, idx, idx_ld, d_dur_over_,
                        B, stream_);
    KX_HIP(hipMemcpyAsync(call_.hF.data(), call_.dF, B * sizeof(int), hipMemcpyDeviceToHost, stream_));
    if (want_edges_) {
        // a call with joins sizes its regions from the used durations of every row's two pad tokens as well: a gather of
        // eight bytes per row and one more copy in front of the same host wait
        h_edge_.assign((size_t)2 * B, 0);
        launch_edge_durations(dur, call_.dT, d_edge, B, stream_);
        KX_HIP(hipMemcpyAsync(h_edge_.data(), d_edge, (size_t)2 * B * sizeof(int), hipMemcpyDeviceToHost, stream_));
    }
    h_bad_id_ = 0;
    KX_HIP(hipMemcpyAsync(&h_bad_id_, d_bad_id_, sizeof(unsigned), hipMemcpyDeviceToHost, stream_));
    h_dur_over_ = 0;
    KX_HIP(hipMemcpyAsync(&h_dur_over_, d_dur_over_, sizeof(unsigned), hipMemcpyDeviceToHost, stream_));

    // ===== the one host round trip: predicted frame counts size everything downstream =========
    KX_HIP(hipStreamWaitEvent(stream_, ev_join_, 0));  // the TextEncoder branch joins here
    call_.mark(0);  // host time to queue the front half
    KX_HIP(hipStreamSynchronize(stream_));
    call_.mark(1);  // ... until the GPU has finished it (the forward's one host wait)
    check_dev_err();
    if (h_bad_id_) {  // a device-side id outside the embedding tables (clamped for the gather, never read out of bounds)
        const unsigned w = h_bad_id_ - 1;
        throw Error(1, "infer: token id outside 0.." + std::to_string(n_vocab_ - 1) + " (utterance " + std::to_string(w >> 16) +
                           ", position " + std::to_string(w & 0xffffu) + ")");
    }
    if (h_dur_over_) {  // an utterance slowed down beyond its row of the alignment (cut at idx_ld on the device, never written past it)
        throw Error(1, "infer: speed too low for utterance " + std::to_string(h_dur_over_ - 1) + ": its durations add up to more than " +
                           std::to_string(idx_ld) + " frames (50 per token of the call's longest utterance)");
    }
    int Fmax = 0;
    for (int b = 0; b < B; ++b) Fmax = call_.hF[b] > Fmax ? call_.hF[b] : Fmax;
    call_.Fmax = Fmax;
    if (need_ld) *need_ld = (int64_t)600 * Fmax;
    if (d_frames) KX_HIP(hipMemcpyAsync(d_frames, call_.dF, B * sizeof(int), hipMemcpyDeviceToDevice, stream_));
    if (audio_ld < (int64_t)600 * Fmax || !d_audio)
        throw Error(1, "infer: audio buffer too small, need ld >= " + std::to_string((long long)600 * Fmax));

    Front f;
    f.dcat = t_dcat;
    f.t_en = t_ten;
    f.idx = idx;
    f.idx_ld = idx_ld;
    f.Tp = Tp;
    f.seed = seed;
    f.noise_off = (flags & 1u) ? 1 : 0;
    f.d_audio = d_audio;
    f.audio_ld = audio_ld;
    return f;
}

// ---- step 3, the back half: the frame axis.  Issued twice with the same allocation sequence: a sizing pass (call_.dry, the
// arena measures), then for real ----------------------------------------------------------------------------------------------
void Model::back_half(const Front& f, Arena& A) {
    const int B = call_.B, Fmax = call_.Fmax;
    const int F1p = up4(Fmax), F2p = up4(2 * Fmax), F20p = up4(20 * Fmax), F120p = up4(120 * Fmax + 1);
    const LenMap LF1{call_.dF, 1, 0}, LF2{call_.dF, 2, 0}, LF20{call_.dF, 20, 0}, LF120{call_.dF, 120, 0}, LF121{call_.dF, 120, 1};
    auto mk = [&](int C, int ld, LenMap len, int Lmax) { return T::of(A.f((size_t)B * C * ld), C, ld, len, Lmax); };
    // (pre-split images exist only while the back half is being issued)
    Restore<Arena*> stats_here(call_.stats_arena, &A), img_here(call_.img_arena, &A);
    auto F1 = [&](int C) { return mk(C, F1p, LF1, Fmax); };
    auto F2 = [&](int C) { return mk(C, F2p, LF2, 2 * Fmax); };
    auto F20 = [&](int C) { return mk(C, F20p, LF20, 20 * Fmax); };
    auto F121 = [&](int C) { return mk(C, F120p, LF121, 120 * Fmax + 1); };
    // --- alignment expand + shared biLSTM + F0 / N predictors (ProsodyPredictor.F0Ntrain) ---
    T en = F1(640);
    if (!call_.dry) launch_gather_cols(f.dcat.p, f.dcat.bs, f.Tp, en.p, en.bs, en.ld, 640, f.idx, f.idx_ld, call_.dF, B, Fmax, stream_);
    float* gxF = A.f((size_t)B * Fmax * 2048);
    T xsh = F1(512);
    lstm(lstms_.at("predictor.shared"), en, xsh, gxF);
    tap("pred.shared", xsh);
    T curves = F2(2);  // row 0 = F0 curve, row 1 = N curve, length 2F
    // The F0 and the N branch read xsh and are independent: N goes to lane 1, F0 stays here.  The raw InstanceNorm sums
    // of xsh are computed once, before the fork (stats() caches them per tensor).
    stats(xsh, "predictor.F0.0.norm1");
    hipEvent_t ev_n = nullptr;
    for (int br = 1; br >= 0; --br) {
        const std::string P = std::string("predictor.") + (br == 0 ? "F0" : "N");
        LaneScope on_lane(*this, br);
        T y0 = F1(512);
        adain_resblk(P + ".0", xsh, y0, false, A.f((size_t)B * 512 * F1p), nullptr, nullptr);
        T y1 = F2(256);
        float* wa = A.f((size_t)B * 256 * F2p);
        float* wb = A.f((size_t)B * 256 * F2p);
        float* wc = A.f((size_t)B * 512 * F2p);
        adain_resblk(P + ".1", y0, y1, true, wa, wb, wc);
        T y2 = F2(256);
        adain_resblk(P + ".2", y1, y2, false, A.f((size_t)B * 256 * F2p), nullptr, nullptr);
        conv(convs_.at(P + "_proj"), y2, curves.rows(br, 1), ConvOpts{});
        if (br == 1) ev_n = record_here();
    }
    wait_here(ev_n);
    tap("pred.F0.raw", curves.rows(0, 1));
    tap("pred.N.raw", curves.rows(1, 1));
    // prosody: the per-token pitch / energy ratios shape the two curves here, before anything reads them (the source below, F0_conv
    // and N_conv of the decoder), and the report is taken of what they then hold
    if (pros_.curves() && !call_.dry)
        launch_prosody_curves(curves.p, curves.bs, curves.ld, call_.dF, call_.dT, call_.d_dur, f.idx, f.idx_ld, pros_.pitch, pros_.energy,
                              pros_.stride, pros_.rep_first, pros_.report, B, stream_);
    tap("pred.F0", curves.rows(0, 1));
    tap("pred.N", curves.rows(1, 1));
    // --- Generator, source side: harmonic source -> STFT -> noise_convs / noise_res of both stages.  It depends on the
    // F0 curve only, so it runs on a lane of its own beside the decoder and the first generator stage.
    const std::string G = "decoder.generator.";
    T ns[2];
    hipEvent_t ev_ns[2] = {nullptr, nullptr};
    size_t part_n[2];
    call_.p1_region = true;  // (from here on: generator and decoder convs)
    {
        LaneScope on_lane(*this, 3);
        const long hs_ld = (long)600 * Fmax;
        float* har_src = A.f((size_t)B * hs_ld);
        float* phase = A.f((size_t)B * 9 * 2 * Fmax);
        if (!call_.dry)
            launch_source(curves.p, curves.bs, call_.dF, B, Fmax, wt(G + "m_source.l_linear.weight"),
                          wt(G + "m_source.l_linear.bias"), f.seed, utt_base, call_.d_utt_seeds, call_.d_utt_index, f.noise_off, phase, har_src, hs_ld, stream_);
        if (call_.taps_on && !call_.dry) tap("gen.har_source", T::of(har_src, 1, (int)hs_ld, LenMap{call_.dF, 600, 0}, 600 * Fmax, hs_ld));
        T har = F121(22);
        if (!call_.dry) launch_stft(har_src, hs_ld, har.p, har.bs, har.ld, call_.dF, B, Fmax, stft_variant, stream_);
        tap("gen.har", har);
        for (int st = 0; st < 2; ++st) {
            const int ch = st == 0 ? 256 : 128;
            auto S = [&](int C) { return st == 0 ? F20(C) : F121(C); };
            ns[st] = S(ch);
            T t1 = S(ch);
            part_n[st] = (size_t)B * ch * ((st == 0 ? 20 * Fmax : 120 * Fmax + 1) / 64 + 4);  // >= tiles * WN
            float2* part_t1 = static_cast<float2*>(A.alloc(part_n[st] * sizeof(float2)));
            float2* part_xj = static_cast<float2*>(A.alloc(part_n[st] * sizeof(float2)));
            {
                ConvOpts o;
                if (st == 0) { o.stride = 6; o.pad = 3; }
                o.stat_part = part_xj;
                conv(convs_.at(G + "noise_convs." + std::to_string(st)), har, ns[st], o);
            }
            adain_resblock1(G + "noise_res." + std::to_string(st), st == 0 ? 7 : 11, ns[st], ns[st], t1, ns[st], 0, 1.f,
                            part_t1, part_xj);
            tap(("gen.x_source." + std::to_string(st)).c_str(), ns[st]);
            ev_ns[st] = record_here();
        }
    }
    // --- Decoder (istftnet.py Decoder.forward) ---
    T xcat0 = F1(514);
    if (!call_.dry)
        launch_gather_cols(f.t_en.p, f.t_en.bs, f.Tp, xcat0.p, xcat0.bs, xcat0.ld, 512, f.idx, f.idx_ld, call_.dF, B, Fmax, stream_);
    {
        ConvOpts o;
        o.stride = 2;
        o.pad = 1;
        conv(convs_.at("decoder.F0_conv"), curves.rows(0, 1), xcat0.rows(512, 1), o);
        conv(convs_.at("decoder.N_conv"), curves.rows(1, 1), xcat0.rows(513, 1), o);
    }
    T catA = F1(1090), catB = F1(1090);
    float* wa = A.f((size_t)B * 1024 * F1p);
    float* wb = A.f((size_t)B * 1024 * F1p);
    adain_resblk("decoder.encode", xcat0, catA.rows(0, 1024), false, wa, wb, nullptr);
    tap("dec.encode", catA.rows(0, 1024));
    conv(convs_.at("decoder.asr_res"), xcat0.rows(0, 512), catA.rows(1024, 64), ConvOpts{});
    if (!call_.dry) {
        launch_copy_rows(xcat0.rows(512, 2).p, xcat0.bs, xcat0.ld, catA.rows(1088, 2).p, catA.bs, catA.ld, 2, LF1, B,
                         Fmax, stream_);
        launch_copy_rows(catA.rows(1024, 66).p, catA.bs, catA.ld, catB.rows(1024, 66).p, catB.bs, catB.ld, 66, LF1,
                         B, Fmax, stream_);
    }
    T* ci = &catA;
    T* co = &catB;
    for (int i = 0; i < 3; ++i) {
        adain_resblk("decoder.decode." + std::to_string(i), *ci, co->rows(0, 1024), false, wa, wb, nullptr);
        tap(("dec.decode." + std::to_string(i)).c_str(), co->rows(0, 1024));
        std::swap(ci, co);
    }
    T g0 = F2(512);
    {
        float* ua = A.f((size_t)B * 512 * F2p);
        float* ub = A.f((size_t)B * 512 * F2p);
        float* uc = A.f((size_t)B * 1090 * F2p);
        adain_resblk("decoder.decode.3", *ci, g0, true, ua, ub, uc);
    }
    tap("dec.decode.3", g0);
    // --- Generator: 2 up-sampling stages -> iSTFT head (the harmonic source / noise path was issued above) ---
    T x = g0;
    for (int st = 0; st < 2; ++st) {
        const int ch = st == 0 ? 256 : 128;
        auto S = [&](int C) { return st == 0 ? F20(C) : F121(C); };
        T xu = S(ch), xs = S(ch);
        wait_here(ev_ns[st]);
        {
            ConvOpts o;  // x = ups(leaky_relu(x, 0.1)) (+ reflection pad on the last stage) + x_source
            o.act = ACT_LEAKY; o.slope = 0.1f; o.pad = 1;
            o.store = ST_UPSCATTER;
            o.up_pad = st == 0 ? 5 : 3;
            o.up_off = st == 0 ? 0 : 1;
            o.up_reflect = st == 0 ? 0 : 1;
            o.up_len = st == 0 ? LF20 : LF120;
            o.resid = &ns[st];
            conv(convs_.at(G + "ups." + std::to_string(st)), x, xu, o);
        }
        tap(("gen.ups." + std::to_string(st)).c_str(), xu);
        // The three resblocks (k = 3, 7, 11) read xu and are averaged: three independent chains, each on a lane of its
        // own with its own scratch; only the last conv of a chain touches the shared running sum xs, in the fixed
        // order k = 3, 7, 11 (events), so the result does not depend on how the chains interleave.  The raw
        // InstanceNorm sums of xu are computed once, here, before the chains fork (stats() caches them per tensor).
        static const int ks[3] = {3, 7, 11};
        const std::string RB = G + "resblocks.";
        stats(xu, RB + std::to_string(st * 3 + 2) + ".adain1.0");
        hipEvent_t ev_r = nullptr;
        for (int j = 0; j < 3; ++j) {
            T xj = S(ch), t1 = S(ch);
            float2* p_t1 = static_cast<float2*>(A.alloc(part_n[st] * sizeof(float2)));
            float2* p_xj = static_cast<float2*>(A.alloc(part_n[st] * sizeof(float2)));
            LaneScope on_lane(*this, j == 2 ? 0 : j + 1);  // (the longest chain stays on the main stream)
            adain_resblock1(RB + std::to_string(st * 3 + j), ks[j], xu, xj, t1, xs, j > 0 ? 1 : 0, j == 2 ? 3.0f : 1.0f,
                            p_t1, p_xj, ev_r);
            if (j < 2) ev_r = record_here();
        }
        tap(("gen.stage." + std::to_string(st)).c_str(), xs);
        x = xs;
    }
    T cp = F121(22);
    {
        ConvOpts o;
        o.act = ACT_LEAKY; o.slope = 0.01f; o.pad = 3;
        conv(convs_.at(G + "conv_post"), x, cp, o);
    }
    call_.p1_region = false;
    tap("gen.conv_post", cp);
    float* spec = A.f((size_t)B * 22 * F120p);
    if (!call_.dry) launch_istft_head(cp.p, cp.bs, cp.ld, spec, f.d_audio, f.audio_ld, call_.dF, B, Fmax, stft_variant, stream_);
    if (call_.taps_on && !call_.dry) tap("audio", T::of(f.d_audio, 1, (int)f.audio_ld, LenMap{call_.dF, 600, 0}, 600 * Fmax, f.audio_ld));
}

void Model::infer_device(const int64_t* d_ids, int64_t t_stride, const int32_t* lens_host, int B,
                         const float* d_styles, const float* speeds_host, int n_speed, uint64_t seed, uint32_t flags,
                         float* d_audio, int64_t audio_ld, int32_t* d_frames, int64_t* need_ld, const uint64_t* d_utt_seeds,
                         const uint32_t* d_utt_index) {
    const int Tmax = check_device_call(d_ids, t_stride, lens_host, B, d_styles, speeds_host, n_speed);
    KX_HIP(hipSetDevice(device));
    CuScope cu_scope(cu_count_);  // (grid heuristics of the launchers: this model's CUs)
    const auto t_enter = std::chrono::steady_clock::now();
    DeviceTurn turn(*this);  // (until this call has queued its last launch)
    start_call(t_enter, lens_host, B, Tmax, flags, d_utt_seeds, d_utt_index);
    const Front f = front_half(d_ids, t_stride, lens_host, d_styles, speeds_host, n_speed, seed, flags, d_audio, audio_ld, d_frames,
                               need_ld);
    plan_arena(arenaF_, true, [&](Arena& A) {
        if (call_.dry) return back_half(f, A);
        call_.mark(2);  // ... until the back half is planned (dry run of the launch sequence)
        try {
            back_half(f, A);
        } catch (...) {
            sync_lanes();  // (nothing of this call may still be running on a side lane when the arenas are handed out again)
            throw;
        }
    });
    call_.mark(3);  // ... until the back half is queued (the call returns; the GPU is still running it)
}

}  // namespace kx
