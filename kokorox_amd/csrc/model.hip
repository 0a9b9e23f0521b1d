// Host side of the MI355X Kokoro-82M model: streams and their tear-down, the weight registry + repacking, arenas, settings,
// profile and diagnostics.  The launch sequence is model_forward.hip, the host entries of a call model_host.hip.
#include "model.h"

#include <cstdlib>
#include <cstring>

namespace kx {

Model::Model(int dev, int part, int n_parts) : device(dev), part_(part), n_parts_(n_parts) {
    if (const char* e = getenv("KOKOROX_CONV"))
        conv_mode = (strcmp(e, "f32") == 0) ? CONV_F32 : (strcmp(e, "f16") == 0 ? CONV_F16 : (strcmp(e, "bf16") == 0 ? CONV_BF16 : (strcmp(e, "f16f8") == 0 ? CONV_F16F8 : CONV_F16X3)));
    if (const char* e = getenv("KOKOROX_STFT")) stft_variant = (strcmp(e, "torch") == 0) ? STFT_TORCH : STFT_ONNX;
    // (per-device state of the library -- the per-device turn of the forwards, dynamic-LDS attribute limits, CU counts -- is
    // kept in tables of KX_MAX_DEVICES entries: an id beyond them is refused here, never aliased onto another device's entry)
    if (dev < 0 || dev >= KX_MAX_DEVICES) throw Error(1, "device id outside 0.." + std::to_string(KX_MAX_DEVICES - 1));
    KX_HIP(hipSetDevice(device));
    // Non-blocking: the model's streams never synchronise with the legacy null stream, so nothing one model does can stall
    // another model on the same GPU (two models per GPU in the server, kx_create_replicas with repeated ids).  Everything
    // on the forward's path is issued on stream_ or ordered to it by events; kx_infer_device orders its device inputs
    // after the caller's null-stream work explicitly (infer_device_after_null).
    // A CU-partitioned model (kx_create_partition; kx_create_replicas with a device id given k times): every stream of the model
    // is confined to its share of the CUs -- bits [part, part + 1) x CUs / n_parts of the queue's CU mask, which the driver deals
    // over the XCCs (probed: either half of the bits is 128 CUs on all 8 XCCs) -- so k models run their forwards side by side
    // on one GPU without ever competing for a CU: a recurrence's workgroups, which need a whole CU each, cannot starve behind
    // another model's conv workgroups (profiles/r04_serve_models_per_gpu.txt), and the under-filled phases of one forward (the
    // token-axis front half, the recurrences) run beside the other's convs.  (Such streams synchronise with the legacy null
    // stream -- the extension has no flags argument; nothing on the forward's path touches that stream.)
    KX_REQUIRE(n_parts >= 1 && n_parts <= 8 && part >= 0 && part < n_parts, "model: partition must be 0 .. n_parts - 1 of 1 .. 8");
    if (n_parts > 1) {
        hipDeviceProp_t prop;
        KX_HIP(hipGetDeviceProperties(&prop, device));
        const int cus = prop.multiProcessorCount;
        const int lo = (int)((long)cus * part / n_parts), hi = (int)((long)cus * (part + 1) / n_parts);
        KX_REQUIRE(hi - lo >= 16, "model: a partition needs at least 16 CUs");
        cu_mask_.assign((size_t)(cus + 31) / 32, 0u);
        for (int i = lo; i < hi; ++i) cu_mask_[(size_t)i >> 5] |= 1u << (i & 31);
        cu_count_ = hi - lo;
    }
    new_stream(&stream_);
    main_stream_ = stream_;
    KX_HIP(hipMalloc((void**)&d_dev_err_, sizeof(unsigned)));
    KX_HIP(hipMemsetAsync(d_dev_err_, 0, sizeof(unsigned), stream_));
    KX_HIP(hipHostMalloc((void**)&h_words_, 8 * sizeof(unsigned), hipHostMallocDefault));
    memset(h_words_, 0, 8 * sizeof(unsigned));
    KX_HIP(hipEventCreateWithFlags(&ev_null_, hipEventDisableTiming));
    KX_HIP(hipStreamSynchronize(stream_));
    new_stream(&stream2_);
    lanes_[0].stream = stream_;
    for (int i = 1; i < N_LANES; ++i) new_stream(&lanes_[i].stream);
    if (const char* e = getenv("KX_LANES")) set_lanes(atoi(e));
    KX_HIP(hipEventCreateWithFlags(&ev_fork_, hipEventDisableTiming));
    KX_HIP(hipEventCreateWithFlags(&ev_join_, hipEventDisableTiming));
    init_dft_tables();
}

// (CU-masked streams are created and retired one at a time, process-wide: kx_create_replicas builds its models on one thread each,
// and the runtime of this image has shown one stall in masked-stream teardown already -- see ~Model)
static std::mutex& masked_stream_mutex() {
    static std::mutex m;
    return m;
}

void Model::new_stream(hipStream_t* s) {
    if (cu_mask_.empty()) {
        KX_HIP(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
        return;
    }
    std::lock_guard<std::mutex> lk(masked_stream_mutex());
    KX_HIP(hipExtStreamCreateWithCUMask(s, (uint32_t)cu_mask_.size(), cu_mask_.data()));
}

Model::~Model() {
    const bool tr = getenv("KX_TRACE_DTOR") != nullptr;
    // CU-masked streams: with the ROCm 7.2 runtime of this image (not with the one torch bundles) hipStreamDestroy of the SECOND
    // masked stream of a device hung for good although every stream had been synchronised on its own; behind one
    // hipDeviceSynchronize it returns at once (probed: tools/_dbg in git history, profiles/r05_experiments_not_kept.txt item 9).
    // KX_MASKED_DESTROY=0 leaves the masked streams to the runtime's own teardown instead (also probed: clean exit).
    // One stall of the C++ replicas demo in 20 runs of the suite was seen AFTER that fix (the stage was not recorded; the demo and
    // this destructor now report theirs): masked streams are retired one model at a time under a process-wide lock.
    const int md = getenv("KX_MASKED_DESTROY") ? atoi(getenv("KX_MASKED_DESTROY")) : 2;
    const bool masked = !cu_mask_.empty();
    auto T = [&](const char* what) { if (tr) { fprintf(stderr, "dtor: %s\n", what); fflush(stderr); } };
    (void)hipSetDevice(device);
    std::unique_lock<std::mutex> masked_lk;
    if (masked) masked_lk = std::unique_lock<std::mutex>(masked_stream_mutex());
    T("device sync");
    if (masked && md == 2) (void)hipDeviceSynchronize();
    auto destroy = [&](hipStream_t st) { if (!masked || md >= 1) (void)hipStreamDestroy(st); };
    T("sync main");
    if (stream_) (void)hipStreamSynchronize(stream_);
    T("sync side");
    if (stream2_) (void)hipStreamSynchronize(stream2_);
    for (int i = 1; i < N_LANES; ++i)
        if (lanes_[i].stream) {
            T("sync lane");
            (void)hipStreamSynchronize(lanes_[i].stream);
            T("destroy lane");
            destroy(lanes_[i].stream);
        }
    T("lanes gone");
    for (hipEvent_t e : lane_ev_) (void)hipEventDestroy(e);
    for (void* p : owned_) (void)hipFree(p);
    if (d_dev_err_) (void)hipFree(d_dev_err_);
    if (h_words_) (void)hipHostFree(h_words_);
    if (h_stage_) (void)hipHostFree(h_stage_);
    if (ev_null_) (void)hipEventDestroy(ev_null_);
    if (ev_done_) (void)hipEventDestroy(ev_done_);
    for (auto* p : d_xchg_)
        if (p) (void)hipFree(p);
    for (Arena* a : {&arenaT_, &arenaF_, &arenaIO_})
        if (a->base) (void)hipFree(a->base);
    if (blob_) (void)hipFree(blob_);
    for (hipEvent_t e : ev_) (void)hipEventDestroy(e);
    if (ev_fork_) (void)hipEventDestroy(ev_fork_);
    if (ev_join_) (void)hipEventDestroy(ev_join_);
    T("destroy side");
    if (stream2_) destroy(stream2_);
    T("destroy main");
    if (stream_) destroy(stream_);
    T("done");
}

// ---- weight container: read and checked on the host (kxw_file.cpp); here it reaches the device --------------------------
// (in both loaders the table is accepted before the blob is allocated and before build() launches anything)
void Model::load_file(const char* path) {
    const std::vector<unsigned char> host = read_weight_file(path, &source_variant_);
    const size_t n = host.size();
    table_ = kxw_table(host.data(), n, n);
    KX_HIP(hipSetDevice(device));
    KX_HIP(hipMalloc((void**)&blob_, n));
    blob_bytes_ = n;
    KX_HIP(hipMemcpy(blob_, host.data(), n, hipMemcpyHostToDevice));
    build();
}

void Model::load_device_blob(const void* d_blob, size_t n, bool adopt) {
    KX_REQUIRE(d_blob && n >= KXW_HEADER_BYTES, "kx_create_from_device_blob: empty blob");
    KX_HIP(hipSetDevice(device));
    unsigned char h64[KXW_HEADER_BYTES];
    KX_HIP(hipMemcpy(h64, d_blob, sizeof h64, hipMemcpyDeviceToHost));
    const KxwHeader h = kxw_header(h64, sizeof h64);
    if (h.total_bytes != n) throw Error(2, "weight blob: size does not match header");
    std::vector<unsigned char> hdr(h.table_bytes);  // (not beyond the blob: kxw_header)
    KX_HIP(hipMemcpy(hdr.data(), d_blob, hdr.size(), hipMemcpyDeviceToHost));
    table_ = kxw_table(hdr.data(), hdr.size(), n);
    blob_bytes_ = n;
    if (adopt) {  // the caller hands over a hipMalloc'd blob on this device (kx_create_replicas): no second copy
        blob_ = static_cast<char*>(const_cast<void*>(d_blob));
    } else {
        KX_HIP(hipMalloc((void**)&blob_, n));
        KX_HIP(hipMemcpy(blob_, d_blob, n, hipMemcpyDeviceToDevice));
        KX_HIP(hipStreamSynchronize(nullptr));  // (a device-to-device hipMemcpy may return before it has run)
    }
    build();
}

const TensorInfo& Model::info(const std::string& name) const {
    auto it = table_.find(name);
    if (it == table_.end()) throw Error(2, "weight blob: missing tensor " + name);
    return it->second;
}
const float* Model::wt(const std::string& name) const {
    return reinterpret_cast<const float*>(blob_ + info(name).offset);
}
float* Model::dev_alloc(size_t floats) {
    void* p = nullptr;
    KX_HIP(hipMalloc(&p, floats * sizeof(float)));
    owned_.push_back(p);
    return static_cast<float*>(p);
}

DevAlloc Model::owned_alloc() {
    return [this](size_t bytes) -> void* { return dev_alloc((bytes + 3) / 4); };
}

// The layers' weight images come from the shared packers (conv_call.hip); what is left here is finding the tensors and the bias.
// A layer the packers refuse (non-finite weights, or weights beyond the split's range: KX_ERR_INVALID there) is a load error
// like any other of the container: KX_ERR_IO, "weight blob: ...", naming the tensor.
template <class F>
static ConvW packed_or_load_error(const std::string& tensors, F&& pack) {
    try {
        return pack();
    } catch (const Error& e) {
        if (e.code != 1) throw;
        throw Error(2, "weight blob: bad weights " + tensors + ": " + e.what());
    }
}

ConvW Model::make_conv(const std::string& name, bool bias) {
    const TensorInfo& ti = info(name + ".weight");
    const PackSrc src{{wt(name + ".weight"), nullptr, nullptr}, {ti.dims[0], 0, 0}};
    ConvW c = packed_or_load_error(name + ".weight", [&] { return pack_conv(src, ti.dims[1], ti.ndim >= 3 ? ti.dims[2] : 1, stream_, owned_alloc()); });
    c.bias = (bias && has(name + ".bias")) ? wt(name + ".bias") : nullptr;
    return c;
}

ConvW Model::make_conv_cat(const std::vector<std::string>& names) {
    KX_REQUIRE(names.size() <= 3 && !names.empty(), "make_conv_cat");
    PackSrc src{{nullptr, nullptr, nullptr}, {0, 0, 0}};
    int Cin = 0, K = 1;
    std::string tensors;
    for (size_t i = 0; i < names.size(); ++i) {
        const TensorInfo& ti = info(names[i] + ".weight");
        tensors += (i ? ", " : "") + names[i] + ".weight";
        src.p[i] = wt(names[i] + ".weight");
        src.rows[i] = ti.dims[0];
        Cin = ti.dims[1];
        K = ti.ndim >= 3 ? ti.dims[2] : 1;
    }
    ConvW c = packed_or_load_error(tensors, [&] { return pack_conv(src, Cin, K, stream_, owned_alloc()); });
    float* bias = dev_alloc(c.rows);
    int r0 = 0;
    for (size_t i = 0; i < names.size(); ++i) {
        KX_HIP(hipMemcpyAsync(bias + r0, wt(names[i] + ".bias"), (size_t)src.rows[i] * 4, hipMemcpyDeviceToDevice,
                              stream_));
        r0 += src.rows[i];
    }
    c.bias = bias;
    return c;
}

ConvW Model::make_convT(const std::string& name, int stride) {
    const TensorInfo& ti = info(name + ".weight");  // [Cin][Cout][k]
    KX_REQUIRE(ti.dims[2] == 2 * stride, "transposed conv: only k == 2*stride is supported");
    ConvW c = packed_or_load_error(name + ".weight", [&] { return pack_convT(wt(name + ".weight"), ti.dims[0], ti.dims[1], stride, stream_, owned_alloc()); });
    c.bias = wt(name + ".bias");
    return c;
}

LstmW Model::make_lstm(const std::string& name) {
    LstmW l;
    const TensorInfo& ti = info(name + ".weight_ih_l0");
    const PackSrc src{{wt(name + ".weight_ih_l0"), wt(name + ".weight_ih_l0_reverse"), nullptr}, {1024, 1024, 0}};
    l.ih = packed_or_load_error(name + ".weight_ih_l0, " + name + ".weight_ih_l0_reverse", [&] { return pack_conv(src, ti.dims[1], 1, stream_, owned_alloc()); });
    float* bias = dev_alloc(2048);
    launch_vec_add(wt(name + ".bias_ih_l0"), wt(name + ".bias_hh_l0"), bias, 1024, stream_);
    launch_vec_add(wt(name + ".bias_ih_l0_reverse"), wt(name + ".bias_hh_l0_reverse"), bias + 1024, 1024, stream_);
    l.ih.bias = bias;
    float* wh = dev_alloc(2 * 256 * 1024);
    launch_transpose_whh(wt(name + ".weight_hh_l0"), wh, stream_);
    launch_transpose_whh(wt(name + ".weight_hh_l0_reverse"), wh + 256 * 1024, stream_);
    l.whhT = wh;
    return l;
}

void Model::add_fc(const std::string& key, const std::string& fc_name, int style_off) {
    const TensorInfo& ti = info(fc_name + ".weight");
    KX_REQUIRE(ti.dims[1] == 128, "style fc: expected 128 inputs");
    FcDesc d;
    d.w = wt(fc_name + ".weight");
    d.b = wt(fc_name + ".bias");
    d.n_out = ti.dims[0];
    d.style_off = style_off;
    d.out_off = gb_total_;
    fc_off_[key] = gb_total_;
    gb_total_ += d.n_out;
    fc_host_.push_back(d);
}
long Model::fc_off(const std::string& key) const {
    auto it = fc_off_.find(key);
    if (it == fc_off_.end()) throw Error(4, "internal: unknown style fc " + key);
    return it->second;
}

void Model::build() {
    {
        const TensorInfo& we = info("bert.embeddings.word_embeddings.weight");
        const TensorInfo& te = info("text_encoder.embedding.weight");
        n_vocab_ = we.dims[0] < te.dims[0] ? we.dims[0] : te.dims[0];  // ids index both tables (178 rows each)
        KX_REQUIRE(n_vocab_ >= 1, "weight blob: empty embedding table");
    }
    const std::string L = "bert.encoder.albert_layer_groups.0.albert_layers.0.";
    convs_["bert.map"] = make_conv("bert.encoder.embedding_hidden_mapping_in");
    convs_["bert.qkv"] = make_conv_cat({L + "attention.query", L + "attention.key", L + "attention.value"});
    convs_["bert.dense"] = make_conv(L + "attention.dense");
    convs_["bert.ffn"] = make_conv(L + "ffn");
    convs_["bert.ffn_out"] = make_conv(L + "ffn_output");
    convs_["bert_encoder"] = make_conv("bert_encoder");
    for (int i = 0; i < 3; ++i) {
        const std::string n = "predictor.text_encoder.lstms." + std::to_string(2 * i);
        lstms_[n] = make_lstm(n);
        add_fc("dur_enc." + std::to_string(i), "predictor.text_encoder.lstms." + std::to_string(2 * i + 1) + ".fc", 128);
    }
    lstms_["predictor.lstm"] = make_lstm("predictor.lstm");
    lstms_["predictor.shared"] = make_lstm("predictor.shared");
    lstms_["text_encoder.lstm"] = make_lstm("text_encoder.lstm");
    convs_["duration_proj"] = make_conv("predictor.duration_proj.linear_layer");
    auto reg_resblk = [&](const std::string& n, int style_off) {
        convs_[n + ".conv1"] = make_conv(n + ".conv1");
        convs_[n + ".conv2"] = make_conv(n + ".conv2");
        if (has(n + ".conv1x1.weight")) convs_[n + ".conv1x1"] = make_conv(n + ".conv1x1", false);
        add_fc(n + ".norm1", n + ".norm1.fc", style_off);
        add_fc(n + ".norm2", n + ".norm2.fc", style_off);
    };
    for (const char* br : {"F0", "N"}) {
        for (int i = 0; i < 3; ++i) reg_resblk(std::string("predictor.") + br + "." + std::to_string(i), 128);
        convs_[std::string("predictor.") + br + "_proj"] = make_conv(std::string("predictor.") + br + "_proj");
    }
    for (int i = 0; i < 3; ++i)
        convs_["text_encoder.cnn." + std::to_string(i)] = make_conv("text_encoder.cnn." + std::to_string(i) + ".0");
    reg_resblk("decoder.encode", 0);
    for (int i = 0; i < 4; ++i) reg_resblk("decoder.decode." + std::to_string(i), 0);
    convs_["decoder.F0_conv"] = make_conv("decoder.F0_conv");
    convs_["decoder.N_conv"] = make_conv("decoder.N_conv");
    convs_["decoder.asr_res"] = make_conv("decoder.asr_res.0");
    const std::string G = "decoder.generator.";
    auto reg_resblock1 = [&](const std::string& n) {
        for (int i = 0; i < 3; ++i) {
            const std::string s = std::to_string(i);
            convs_[n + ".convs1." + s] = make_conv(n + ".convs1." + s);
            convs_[n + ".convs2." + s] = make_conv(n + ".convs2." + s);
            add_fc(n + ".adain1." + s, n + ".adain1." + s + ".fc", 0);
            add_fc(n + ".adain2." + s, n + ".adain2." + s + ".fc", 0);
        }
    };
    for (int i = 0; i < 2; ++i) {
        convs_[G + "noise_convs." + std::to_string(i)] = make_conv(G + "noise_convs." + std::to_string(i));
        reg_resblock1(G + "noise_res." + std::to_string(i));
    }
    convs_[G + "ups.0"] = make_convT(G + "ups.0", 10);
    convs_[G + "ups.1"] = make_convT(G + "ups.1", 6);
    for (int i = 0; i < 6; ++i) reg_resblock1(G + "resblocks." + std::to_string(i));
    convs_[G + "conv_post"] = make_conv(G + "conv_post");

    for (auto& kv : convs_) kv.second.name = kv.first;
    if (conv_mode == CONV_BF16 || conv_mode == CONV_F16F8) set_conv_mode(conv_mode);  // (KOKOROX_CONV=bf16 / f16f8: the images exist from the start)
    for (auto& kv : lstms_) kv.second.ih.name = kv.first + ".ih";
    KX_HIP(hipMalloc((void**)&fc_dev_, fc_host_.size() * sizeof(FcDesc)));
    owned_.push_back(fc_dev_);
    KX_HIP(hipMemcpyAsync(fc_dev_, fc_host_.data(), fc_host_.size() * sizeof(FcDesc), hipMemcpyHostToDevice, stream_));
    KX_HIP(hipStreamSynchronize(stream_));
}

// ---- helpers ------------------------------------------------------------------------------------
void Model::ensure_arena(Arena& a, size_t bytes) {
    if (bytes <= a.cap) return;
    KX_HIP(hipStreamSynchronize(stream_));
    if (a.base) KX_HIP(hipFree(a.base));
    a.base = nullptr;
    a.cap = 0;
    // half again as much as asked for: a serving process meets its largest (batch x length) shape step by step, and every
    // regrowth is a stream sync + hipFree + hipMalloc of gigabytes (seen as a 1.3 s latency outlier in a 25 s soak with 12 %
    // slack); the card has 288 GB
    const size_t want = bytes + bytes / 2 + (1 << 20);
    KX_HIP(hipMalloc((void**)&a.base, want));
    a.cap = want;
}

// profile mode: FLOPs and algorithmic HBM bytes of a launch, and the first of the two events around it
void Model::prof_begin(const ConvW& w, const T& in, const T& out, const ConvOpts& o) {
    const LenMap& lm = (o.store == ST_UPSCATTER) ? in.len : out.len;
    const double cols = host_cols(lm, o.store == ST_UPSCATTER ? 1 : 0);
    prof_flops_ += 2.0 * w.rows * w.Cin * w.K * cols;
    prof_launches_ += 1;
    // algorithmic HBM bytes of the launch: the input tensor once, the residual and the running
    // sum where the epilogue reads them, the output once, the split-f16 weights once
    const double in_cols = host_cols(in.len);
    const double out_rows = (o.store == ST_UPSCATTER) ? (double)(w.up_cout ? w.up_cout : 1) : (double)w.rows;
    const double out_cols = (o.store == ST_UPSCATTER) ? cols * w.up_s : cols;
    const double out_elems = out_rows * out_cols;
    const double bytes = 4.0 * ((double)w.Cin * in_cols + out_elems * (1.0 + (o.resid ? 1.0 : 0.0) + (o.accum ? 1.0 : 0.0)) +
                                (double)w.rows * w.Cin * w.K);
    prof_recs_.push_back(ProfRec{w.rows, w.Cin, w.K, o.dil, o.stride, o.store, cols, 2.0 * w.rows * w.Cin * w.K * cols, 0.f, bytes});
    if (ev_used_ + 2 > ev_.size()) {
        for (int i = 0; i < 64; ++i) {
            hipEvent_t e;
            KX_HIP(hipEventCreate(&e));
            ev_.push_back(e);
        }
    }
    KX_HIP(hipEventRecord(ev_[ev_used_], stream_));
}

void Model::prof_end() {
    KX_HIP(hipEventRecord(ev_[ev_used_ + 1], stream_));
    ev_used_ += 2;
}

const Tap* Model::find_tap(const std::string& name) const {
    auto it = taps_.find(name);
    return it == taps_.end() ? nullptr : &it->second;
}

void Model::sync() {
    KX_HIP(hipSetDevice(device));
    KX_HIP(hipStreamSynchronize(stream_));
    check_dev_err();
}

// (the stream is idle) raise what a kernel recorded in the sticky device error word, and clear it
void Model::check_dev_err() {
    // (through the model's own stream into page-locked memory: a null-stream copy here would wait for, and hold up, every
    // other model's blocking work on this GPU)
    KX_HIP(hipMemcpyAsync(&h_words_[0], d_dev_err_, sizeof(unsigned), hipMemcpyDeviceToHost, main_stream_));
    KX_HIP(hipStreamSynchronize(main_stream_));
    const unsigned e = h_words_[0];
    if (!e) return;
    KX_HIP(hipMemsetAsync(d_dev_err_, 0, sizeof(unsigned), main_stream_));
    KX_HIP(hipStreamSynchronize(main_stream_));
    // A part of a resident-weights recurrence never saw its partner (starved behind other work on the GPU): what this call
    // computed is garbage.  The model switches to the streaming recurrence -- same bits, no partner to wait for -- and goes back
    // to the resident forms after LSTM_REARM_AFTER clean forwards; the host entry points re-run the call once (infer_host_ex).
    lstm_pair_ok_ = false;
    lstm_rearm_in_ = LSTM_REARM_AFTER;
    n_lstm_timeouts_ += 1;
    throw LstmTimeout("device error word " + std::to_string(e) +
                      ": a part of the resident-weights LSTM recurrence never saw its partner; this call's result is invalid; the "
                      "model runs the streaming recurrence (same bits) for the next " + std::to_string(LSTM_REARM_AFTER) + " forwards");
}

void Model::set_conv_mode(int mode) {
    sync();
    if (mode == CONV_BF16 || mode == CONV_F16F8) {
        // the bf16 / 8-bit cross forms of the weight images of the layers that take them, once (bf16: 160 MB more)
        KX_HIP(hipSetDevice(device));
        const DevAlloc alloc = owned_alloc();
        for (auto& kv : convs_) {
            if (mode == CONV_BF16) add_bf16_image(kv.second, stream_, alloc);
            else add_f8_image(kv.second, stream_, alloc);
        }
        KX_HIP(hipStreamSynchronize(stream_));
    }
    conv_mode = mode;
}

void Model::info(int64_t out[8]) const {
    out[0] = source_variant_;
    out[1] = (source_variant_ == 3 || source_variant_ == 4) ? 0 : 1;
    out[2] = conv_mode;
    out[3] = n_vocab_;
    out[4] = n_voices_.load(std::memory_order_acquire);
    out[5] = part_;
    out[6] = n_parts_;
    int cus = cu_count_;
    if (cus == 0) {
        hipDeviceProp_t prop;
        cus = hipGetDeviceProperties(&prop, device) == hipSuccess ? prop.multiProcessorCount : 0;
    }
    out[7] = cus;
}

void Model::status(int64_t out[4]) const {
    out[0] = lstm_pair_ok_ ? 0 : 1;
    out[1] = n_lstm_timeouts_;
    out[2] = lstm_pair_ok_ ? 0 : lstm_rearm_in_;
    out[3] = n_rerun_;
}

// a forward has finished cleanly: count down to the resident-weights recurrence's return
void Model::note_clean_forward() {
    if (!lstm_pair_ok_ && lstm_rearm_in_ > 0 && --lstm_rearm_in_ == 0) lstm_pair_ok_ = true;
}

void Model::set_pinned(const int32_t* pattern, int n) {
    KX_HIP(hipSetDevice(device));
    KX_HIP(hipStreamSynchronize(stream_));
    n_pinned_ = 0;
    if (n <= 0) return;
    KX_REQUIRE(pattern && n <= 512, "pinned durations: 1..512 entries");
    for (int i = 0; i < n; ++i) KX_REQUIRE(pattern[i] >= 1 && pattern[i] <= 50, "pinned durations must be in 1..50");
    if (!d_pinned_) {
        KX_HIP(hipMalloc((void**)&d_pinned_, 512 * sizeof(int)));
        owned_.push_back(d_pinned_);
    }
    KX_HIP(hipMemcpy(d_pinned_, pattern, n * sizeof(int), hipMemcpyHostToDevice));
    n_pinned_ = n;
}

void Model::diag_enable(bool on) {
    sync();
    diag_on_ = on;
    diag_recs_.clear();
    diag_used_ = 0;
    if (on && !d_diag_) {
        diag_cap_ = 1024;
        d_diag_ = dev_alloc(3 * diag_cap_);
    }
    if (on) {
        KX_HIP(hipMemsetAsync(d_diag_, 0, 3 * diag_cap_ * sizeof(float), stream_));
        KX_HIP(hipStreamSynchronize(stream_));
    }
}

const std::vector<Model::DiagRec>& Model::diag_collect() {
    sync();
    std::vector<float> h(3 * diag_used_);
    if (diag_used_) KX_HIP(hipMemcpy(h.data(), d_diag_, h.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < diag_recs_.size() && i < diag_used_; ++i) {
        diag_recs_[i].absmax = h[3 * i];
        diag_recs_[i].count = (double)h[3 * i + 2];  // (one add of the utterance's length per channel and utterance)
        diag_recs_[i].rms = diag_recs_[i].count > 0 ? std::sqrt((double)h[3 * i + 1] / diag_recs_[i].count) : 0.0;
    }
    return diag_recs_;
}

void Model::set_act_shift(const std::string& conv_name, int shift) {
    KX_REQUIRE(shift >= -24 && shift <= 24, "activation pre-scale: shift must be in -24..24");
    sync();
    auto it = convs_.find(conv_name);
    if (it != convs_.end()) {
        it->second.act_shift = shift;
        return;
    }
    const std::string suf = ".ih";
    if (conv_name.size() > suf.size() && conv_name.compare(conv_name.size() - suf.size(), suf.size(), suf) == 0) {
        auto il = lstms_.find(conv_name.substr(0, conv_name.size() - suf.size()));
        if (il != lstms_.end()) {
            il->second.ih.act_shift = shift;
            return;
        }
    }
    throw Error(4, "no such conv layer: " + conv_name);
}

int Model::get_act_shift(const std::string& conv_name) const {
    auto it = convs_.find(conv_name);
    if (it == convs_.end()) throw Error(4, "no such conv layer: " + conv_name);
    return it->second.act_shift;
}

void Model::profile_enable(bool on) {
    sync();
    prof_on_ = on;
    prof_recs_.clear();
    ev_used_ = 0;
    prof_flops_ = 0;
    prof_launches_ = 0;
    prof_stats_bytes_ = 0;
    prof_stats_launches_ = 0;
}

void Model::profile_aux(int64_t* stats_launches, double* stats_bytes) {
    if (!prof_on_) throw Error(4, "profiling is not enabled");
    *stats_launches = prof_stats_launches_;
    *stats_bytes = prof_stats_bytes_;
    prof_stats_launches_ = 0;
    prof_stats_bytes_ = 0;
}

void Model::profile_read(int64_t* launches, double* ms, double* flops) {
    if (!prof_on_) throw Error(4, "profiling is not enabled");
    sync();
    double total = 0;
    for (size_t i = 0; i + 1 < ev_used_; i += 2) {
        float t = 0;
        KX_HIP(hipEventElapsedTime(&t, ev_[i], ev_[i + 1]));
        total += t;
        if (i / 2 < prof_recs_.size()) prof_recs_[i / 2].ms = t;
    }
    prof_detail.swap(prof_recs_);
    prof_recs_.clear();
    *launches = prof_launches_;
    *ms = total;
    *flops = prof_flops_;
    ev_used_ = 0;
    prof_flops_ = 0;
    prof_launches_ = 0;
}

}  // namespace kx
