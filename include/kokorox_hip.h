/*
 * kokorox_hip.h — C ABI of libkokorox_hip.so: the MI355X-native replacement for the one
 * hot path of byteowlz/kokorox, the Kokoro-82M forward pass that the reference runs as
 * `ort::Session::run()` inside `OrtKoko::infer`.
 *
 * Every entry point names the reference interface it replaces (paths relative to the
 * reference checkout).  Plain pointers and sizes only; no C++/torch types; nothing
 * throws or unwinds across this boundary: every call returns a status and the text of
 * the last failure is available from kx_last_error().
 *
 * Threading: a kx_model may be shared by any number of OS threads.  Calls on one model
 * are serialised on an internal mutex, which is exactly what the reference's
 * `Mutex<Session>` does (kokorox/src/onn/ort_koko.rs:14,78).  Use one model per GPU.
 */
#ifndef KOKOROX_HIP_H
#define KOKOROX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KX_OK 0
#define KX_ERR_INVALID 1   /* bad argument (empty batch, id out of range, T > 512 ...)   */
#define KX_ERR_IO 2        /* weight file missing / malformed                             */
#define KX_ERR_DEVICE 3    /* HIP runtime failure, no gfx950 device                       */
#define KX_ERR_STATE 4     /* unknown tap name, profiling not enabled ...                 */

#define KX_STYLE_DIM 256       /* ort_koko.rs:44 "1,256"; koko.rs:1255-1306 builds the row */
#define KX_SAMPLES_PER_FRAME 600
#define KX_SAMPLE_RATE 24000
#define KX_MAX_TOKENS 512      /* model position table; koko.rs:783 chunks to <=500 + 2 pads */

/* kx_infer flags */
#define KX_FLAG_NOISE_OFF 1u   /* zero the SineGen additive noise (timing experiments only) */
#define KX_FLAG_TAPS 2u        /* keep named intermediates for kx_debug_tap (tests)          */

typedef struct kx_model kx_model;

/* Replaces `init_ort(dylib_path)` (kokorox/src/onn/mod.rs:19-49): one-off runtime
 * initialisation.  Checks that `device_id` exists and is a gfx950 part.
 * err/err_len: optional buffer for a message when the return value is not KX_OK. */
int kx_init(int device_id, char* err, size_t err_len);

/* Replaces `OrtKoko::new(model_path)` → `OrtBase::load_model` → `commit_from_file`
 * (kokorox/src/onn/ort_koko.rs:31-35, ort_base.rs:14-39; call site kokorox/src/tts/koko.rs:570-573).
 * `weights_path` is what the reference passes there: the Hugging Face `onnx/model.onnx` (path built at
 * kokorox/src/utils/hf_cache.rs:128-158; its fp16 / int8 / 4-bit siblings of hf_cache.rs:135-144 load as well, their
 * weights de-quantised to f32).  The library reads the ONNX initialisers itself (csrc/onnx_import.cpp: no protobuf
 * package, no ONNX Runtime), places them by the rules of kokorox_amd/importer.py, uploads them and repacks the
 * contraction weights for the MFMA kernels.  A file that starts with the magic "KXHIPW01" is taken as the library's own
 * pre-converted container (kokorox_amd/weights.py) instead; `<path>.kxw` beside an .onnx is used when it is at least as
 * new as the .onnx, and written when the environment has KOKOROX_KXW_CACHE=1.
 * Returns NULL on failure with the reason in err (KX_ERR_IO class: missing / truncated / external-data files, tensors
 * of the model that could not be found — the message lists initialisers that were not placed). */
kx_model* kx_create(const char* weights_path, int device_id, char* err, size_t err_len);

/* Host only (no GPU is touched): `model.onnx` → the KXHIPW01 container kx_create would build from it in memory, written
 * to out_path — for a deployment that wants to convert once (the bytes equal `python -m kokorox_amd.importer`'s).
 * No reference counterpart: ONNX Runtime parses the file on every start (ort_base.rs:27-33). */
int kx_import_onnx(const char* onnx_path, const char* out_path, char* err, size_t err_len);

/* Same, from a weight blob that is ALREADY resident in this GPU's memory, e.g. after the
 * one-time RCCL broadcast over xGMI.  The blob is borrowed for the
 * duration of the call only (the library keeps its own repacked copy and copies the
 * small tensors it needs). */
kx_model* kx_create_from_device_blob(const void* d_blob, size_t n_bytes, int device_id,
                                     char* err, size_t err_len);

/* One model per GPU for the server (the reference's server is ONE process, kokorox-openai/src/lib.rs:
 * 370-439): reads the weight file ONCE (`.onnx` or container, as kx_create), uploads it to device_ids[0] over PCIe and fans it out to the other
 * devices with concurrent device-to-device copies (hipMemcpyPeerAsync, one xGMI link per destination), then builds
 * every model from its resident blob, the models side by side (one host thread each).  out_models[n] receives the handles,
 * ready for kx_dispatcher_create.  A device id that is given k times (k <= 8) gets k CU-PARTITIONED models, each confined to
 * 1 / k of the device's CUs (kx_create_partition): they run their forwards side by side on the one GPU and never compete for a
 * CU (KX_REPLICA_PARTITION=0: whole-device models that take turns instead).  On failure nothing is leaked and every entry of
 * out_models is NULL.
 * (A multi-PROCESS launch — one rank per GPU, as bench.py under torch.distributed — uses an RCCL broadcast of the
 * blob and kx_create_from_device_blob instead: kokorox_amd/dist.py.) */
int kx_create_replicas(const char* weights_path, const int* device_ids, int n, kx_model** out_models, char* err,
                       size_t err_len);
/* Milestones of the process's last kx_create_replicas call, ms from its entry: out3[0] weight file read (and, for an .onnx,
 * converted), [1] blob resident on every device (PCIe upload + the fan-out copies), [2] every model built. */
int kx_replicas_times(double* out3);

/* A model confined to CUs [part, part + 1) x CUs / n_parts of the device (n_parts 1 .. 8; n_parts = 1 is kx_create): every
 * stream of the model carries that CU mask (hipExtStreamCreateWithCUMask; the driver deals the bits over the XCCs, so a
 * partition keeps its share of every XCC's L2).  Models with disjoint partitions run concurrently on one GPU with no
 * contention for CUs -- two forwards in flight per GPU behind one dispatcher -- and give the bits of a whole-device model.
 * No reference counterpart (one Mutex<Session> per process, ort_koko.rs:78). */
kx_model* kx_create_partition(const char* weights_path, int device_id, int part, int n_parts, char* err, size_t err_len);

/* Replaces `Drop for OrtKoko` / TTSKoko::cleanup (kokorox/src/tts/koko.rs:1338-1375). */
void kx_destroy(kx_model* m);

/* Text of the CALLING THREAD's last failed call on this model ("" if its last call succeeded or it never failed):
 * several threads may share one model (calls are serialised inside), and neither another thread's success nor its
 * failure touches what this thread reads.  The pointer stays valid until the calling thread's next call on any model.
 * kx_last_error_copy writes the same text into a caller buffer (always NUL-terminated). */
const char* kx_last_error(const kx_model* m);
int kx_last_error_copy(const kx_model* m, char* buf, size_t buf_len);

/* Replaces `OrtKoko::infer(tokens, styles, speed)` (kokorox/src/onn/ort_koko.rs:37-91;
 * caller kokorox/src/tts/koko.rs:1177).
 *   ids      [B, t_stride] int64, row b holds lens[b] token ids already wrapped with the
 *            0 pad at both ends (koko.rs:1169-1173); ids must be in 0..177 (vocab.rs:5-20)
 *   lens     [B] tokens per utterance incl. the two pads, 1..512 (3..512 for real text).  The reference is
 *            batch-1 (koko.rs:1175); B>1 gives the same result as B separate calls.
 *   styles   [B,256] float32 voice-style rows (mix_styles, koko.rs:1255-1306)
 *   speeds   [n_speed] float32, n_speed = 1 (shared, ort_koko.rs:67-68) or B; each > 0.  A speed so low that an
 *            utterance's durations add up to more than 50 frames per token of the call's longest utterance is
 *            KX_ERR_INVALID, "infer: speed too low for utterance b: ..." (speeds >= 1 never are)
 *   seed     Philox key of the harmonic-source noise; utterance b of the call draws the
 *            stream (seed, utt_base + b)
 *   out      *out = a library-owned (pooled, page-locked) float32 buffer holding the B waveforms back to back;
 *            out_lens[b] = samples of utterance b (600 * predicted frames).  Free with
 *            kx_free_audio.  The reference likewise returns an owned copy
 *            (ort_koko.rs:85 `data.to_vec()`).
 * Empty input (B = 0 or a len < 1) is an error, not a panic as in ort_koko.rs:56,61. */
int kx_infer(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B,
             const float* styles, const float* speeds, int n_speed, uint64_t seed,
             uint32_t flags, float** out, int64_t* out_lens);

void kx_free_audio(float* p);

/* Device-resident form of the same call for batch serving and for bench.py: every
 * pointer is GPU memory of this model's device, nothing crosses PCIe, nothing is
 * allocated per call after the first call of a given shape.
 *   d_audio      [B, audio_ld] float32, written for samples < 600*frames[b]
 *   d_frames     [B] int32 predicted frame counts
 * Returns KX_ERR_INVALID if audio_ld is smaller than the longest waveform (the needed
 * length is then in *need_ld), or if a token id in d_ids lies outside 0..177: device-side ids are range-checked by
 * the embedding kernels (clamped for the gather, so nothing is read out of bounds) and reported at the call's one
 * host synchronisation point.  The call returns after the work has been queued on the
 * model's stream and its frame counts are known; kx_sync waits for completion.
 * Streams: the model's streams are NON-BLOCKING (they do not synchronise with the legacy null stream).  The call orders
 * itself against the NULL stream on both sides, on the GPU, without a host stall: its reads of d_ids / d_styles wait for what
 * the caller had queued on the null stream before the call, and null-stream work queued AFTER the call returns (torch's default
 * stream reading d_audio / d_frames, or writing the next request into d_ids / d_styles) waits for the end of this forward.
 * A caller that produces the inputs or consumes the outputs on any OTHER stream (a torch side stream, a per-thread default
 * stream) is not ordered at all: it must finish its writes before the call and call kx_sync before touching d_audio,
 * d_frames, d_ids or d_styles again. */
int kx_infer_device(kx_model* m, const int64_t* d_ids, int64_t t_stride, const int32_t* lens_host,
                    int B, const float* d_styles, const float* speeds_host, int n_speed,
                    uint64_t seed, uint32_t flags, float* d_audio, int64_t audio_ld,
                    int32_t* d_frames, int64_t* need_ld);

int kx_sync(kx_model* m);

/* What was loaded and how it runs.  out8[0]: the weight file's kind -- 0 the library's KXHIPW01 container, 1 fp32 ONNX
 * (onnx/model.onnx, hf_cache.rs:10), 2 fp16 / bf16 ONNX (model_fp16: widened to f32), 3 an 8-bit quantised ONNX variant
 * (model_quantized / model_uint8 / model_q8f16 / model_uint8f16), 4 a 4-bit one (model_q4 / model_q4f16), -1 a cached
 * conversion, -2 built from a device blob (kind unknown).  out8[1]: 1 = the model computes what the reference computes for
 * this file; 0 for kinds 3 and 4: ONNX Runtime runs those as DynamicQuantizeLinear -> MatMulInteger / ConvInteger /
 * MatMulNBits, i.e. it quantises the ACTIVATIONS at run time, while this library de-quantises the WEIGHTS at load and then
 * runs f32-class arithmetic -- closer to the fp32 model than the reference's own output for that file, and therefore not
 * within 1e-4 of it (a notice is printed at load; hf_cache.rs:135-144, ort_base.rs:27-33).  out8[2]: conv mode
 * (kx_get_conv_mode); [3] rows of the embedding tables; [4] voices in the device table; [5] / [6] CU partition and number of
 * partitions (kx_create_partition; 0 / 1 = the whole device); [7] CUs the model launches on. */
int kx_model_info(kx_model* m, int64_t* out8);

/* What the model's LSTM recurrences are running on, and whether anything went wrong (SURVEY 8b "Threading"; the reference has
 * nothing to report: one Mutex<Session>, ort_koko.rs:78).  out4[0]: 0 = the resident-weights forms (two / four workgroups per
 * utterance and direction, which hand h over between CUs), 1 = the streaming fall-back (one workgroup, no hand-off); out4[1]:
 * hand-off time-outs so far (a part of a recurrence starved behind other work on the GPU for ~0.1 s); out4[2]: clean forwards
 * left until the resident forms return (64 after a time-out, 0 in normal operation); out4[3]: calls that were re-run
 * transparently after a time-out.  Both forms give the SAME BITS, so the switch never changes a result; it costs time
 * (~6 us against 1.6 - 2.5 us per recurrence step).  All zeros in a healthy deployment. */
int kx_model_status(kx_model* m, int64_t* out4);

/* Benchmark control (SURVEY.md §8d "duration pinning"): when set, the predicted duration
 * of token t is replaced by pattern[t % n] for every utterance (the duration head still
 * runs).  n = 0 clears it. */
int kx_set_pinned_durations(kx_model* m, const int32_t* pattern, int n);

/* For servers: one discarded forward of B utterances x n_tokens (incl. the two pads) with every duration pinned to
 * frames_per_token, so that the model's arenas, its page-locked result buffer and its tile tables already have the largest
 * (batch x length) shape the deployment expects when the first request arrives.  Without it the arenas grow on demand - a
 * stream sync + hipFree + hipMalloc of gigabytes, measured as a 1.3 s latency outlier the first time a larger batch shape
 * arrives.  No reference counterpart (ONNX Runtime allocates per run).  A pinned pattern set before stays in force. */
int kx_warmup(kx_model* m, int B, int n_tokens, int frames_per_token);
/* Host-side milestones of the last kx_infer_device / kx_infer* call on this model, in ms from the call's entry:
 * out4[0] front half queued, [1] front half finished on the GPU (the forward's one host wait: the predicted frame counts size
 * everything downstream), [2] back half planned, [3] back half queued (kx_infer_device returns here, the GPU still running). */
int kx_call_times(kx_model* m, double* out4);

/* Capacities in bytes of the three device arenas (token axis, frame axis, I/O): they change only when a larger shape arrives. */
int kx_arena_bytes(kx_model* m, int64_t* out3);

/* Contraction arithmetic of the conv/linear kernel: 0 = f32 MFMA (v_mfma_f32_32x32x2_f32, exact f32
 * products), 1 = f16x3 split MFMA (three v_mfma_f32_32x32x16_f16 per K-step on hi/lo halves, ~22
 * significant bits per product, f32 accumulation; env KOKOROX_CONV=f16x3).  Env KOKOROX_CONV=f32 selects 0 at create.
 * 6 = f16f8, the DEFAULT since round 5 (env KOKOROX_CONV=f16f8): mode 1, except that the snake convs of the generator (3, 7 and 11
 * taps: 85 % of the forward's multiply-adds) carry the two cross terms of the split product, a_lo b_hi + a_hi b_lo, on the 8-bit
 * scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4 on e4m3 images of the four operands) and a_hi b_hi on v_mfma_f32_16x16x32_f16:
 * two MFMA-equivalents per product instead of three, ~17 significant bits per product instead of 22 (measured 1e-5 relative per
 * conv output; the waveform moves by < 1e-5 against mode 1), inside the 1e-4 parity band by the same protocol as modes 0 and 1
 * (tests/test_gpu_forward.py::test_ragged_batch_matches_oracle) and far above the bf16 that BASELINE configs[2] names.  Their
 * snake activation v + sin^2(alpha v) / alpha takes sin^2 from the hardware cosine there, 0.5 - 0.5 v_cos_f32(alpha v / pi): at most
 * 3e-6 absolute in sin^2 for |alpha v| <= 40 and less towards alpha v = 0, so the activation error sin^2-error / alpha is at most
 * 6e-6 (3e-6 rms) at alpha = 0.01 and below 1e-6 from alpha = 0.2 up: the mode's 1e-5 per conv output holds, measured, for every
 * alpha from 0.01 to 20 at O(1) activations.  Argument domain: none that matters.  The ISA documents +-256 turns for the
 * instruction (|alpha v| = 804), but on gfx950 it reduces any finite argument: the sin^2 error grows smoothly as 7e-8 |alpha v|
 * (the float32 product alpha v / pi in front of it) through that edge and far beyond -- 6e-5 at 800, 7e-4 at 9000 -- which in the
 * activation is 7e-8 |v| whatever alpha, and a conv at |alpha v| up to 8800 keeps the error it has at O(1) arguments
 * (tests/test_gpu_snake_range.py; tools/probes/sin_accuracy.hip).  The 8-bit weight images are built at create
 * (or at the first selection of the mode).
 * 4 = reduced precision, opt-in (env KOKOROX_CONV=f16): the decoder / generator convs of the direct-A kernel issue ONE
 * f16 MFMA per product (weights and activations rounded to f16, f32 accumulation) -- the library's counterpart of the
 * reference's `model_fp16` / quantised variants run at their own precision (kokorox/src/utils/hf_cache.rs:135-144) and
 * of BASELINE configs[2] "bf16"; duration head, F0 / N predictor, harmonic source and STFT pair stay f32-class.  Never
 * the default: the waveform leaves the 1e-4 parity band (measured bound in tests/test_gpu_forward.py).
 * 5 = the same on bf16 (env KOKOROX_CONV=bf16; v_mfma_f32_32x32x16_bf16, a bf16 weight image built at the first selection):
 * the dtype BASELINE configs[2] names; 8 significant bits instead of 11, so its error is ~8x that of mode 4 (same test). */
int kx_set_conv_mode(kx_model* m, int mode);
int kx_get_conv_mode(kx_model* m);

/* Which STFT / inverse-STFT pair the generator uses (n_fft 20, hop 5 on both):
 *   0 = the conv-based pair of the ONNX export (upstream custom_stft.py: magnitude sqrt(re^2+im^2+1e-14), phase
 *       atan2 with (im == 0 && re < 0) -> +pi, inverse = cos/sin * window / n_fft transposed convolutions summed as
 *       real - imag, without one-sided doubling or window-envelope division).  Default: `model.onnx` is what the
 *       reference runs (kokorox/src/utils/hf_cache.rs:8-10, ort_koko.rs:79).
 *   1 = torch.stft / torch.istft semantics (the PyTorch checkpoint's own path).
 * Both are restated from the public upstream sources from memory: which of the two the
 * shipped graph contains is the first thing to confirm when a real model.onnx is reachable.  Env KOKOROX_STFT=torch
 * selects 1 at create. */
int kx_set_stft_variant(kx_model* m, int variant);
int kx_get_stft_variant(kx_model* m);

/* Streams ("lanes") of the back half: 1 = every launch on the model's one stream; 4 = the harmonic-source / noise path
 * and the three resblock chains of each generator stage are issued on streams of their own and meet through events;
 * 0 (default) = 4 for batches of up to 32 utterances, where launches leave CUs idle (batch 1: 14.1 -> 11.9 ms), else 1.
 * Also side by side in that mode: the F0 and N predictor branches, and the 1x1 shortcut conv of every AdainResBlk1d.
 * Results are bit-identical for every value: only the last conv of a chain touches the shared running sum, in a fixed
 * order.  Env KX_LANES at create. */
int kx_set_lanes(kx_model* m, int n_lanes);

/* First utterance index used for the noise stream of the next calls (default 0). */
int kx_set_utterance_base(kx_model* m, uint64_t utt_base);

/* Per-kernel-class HIP-event timing on the model's stream (bench.py roofline leg).
 * While enabled every launch of the dominant kernel family -- the 128-row conv / GEMM kernels: conv1d_f16x3_da_kernel,
 * conv1d_f16x3_dag_kernel and conv1d_f16x3_kernel<128,..> (conv1d_mfma_kernel<128,128,2,2> in f32 mode) -- is
 * bracketed by events on the stream it is issued on.
 * kx_profile_read drains them: launches, summed milliseconds and summed algorithmic
 * FLOPs (2*Cout*Cin*k*columns per launch) since the last read. */
int kx_profile_enable(kx_model* m, int on);
int kx_profile_read(kx_model* m, int64_t* launches, double* total_ms, double* total_flops);
/* Per-launch records of the last kx_profile_read: out[i*10 + 0..9] = GEMM rows, Cin, taps, dilation,
 * stride, store form, summed columns, FLOPs, milliseconds, algorithmic HBM bytes (input once + residual /
 * running sum where read + output once + weights once).  out = NULL returns the count only. */
int kx_profile_detail(kx_model* m, double* out, int64_t cap_rows, int64_t* n_rows);
/* Unfused InstanceNorm statistics passes (in_stats_kernel) since the last call: launches and the bytes they must read
 * (each reads its tensor exactly once) - the known byte count the PMC tooling checks FETCH_SIZE against. */
int kx_profile_aux(kx_model* m, int64_t* stats_launches, double* stats_bytes);

/* ---- real-weights readiness (tools/real_weights_report.py) -------------------------------------------------
 * The f16x3 contraction carries every f32 operand as two f16 halves.  That is f32-class for O(1) activations; an input
 * whose magnitude is far below 1e-3 loses its low half to the f16 subnormal quantum, one above 65504 is clamped.
 * kx_diag_enable(1) makes every conv launch of the following kx_infer* calls also measure its input after the AdaIN
 * affine (absmax, rms); kx_diag_count / kx_diag_get read the records (vals7 = GEMM rows, Cin, taps, current
 * pre-scale exponent, absmax, rms, elements).  kx_set_act_prescale(name, e) multiplies that layer's transformed input
 * by 2^e before the split and divides the accumulators by it in the epilogue - exact, so results are unchanged
 * wherever the split was already lossless.  Layer names are the weight names without ".weight" (LSTM input
 * projections: "<lstm>.ih"). */
int kx_diag_enable(kx_model* m, int on);
int kx_diag_count(kx_model* m, int64_t* n);
int kx_diag_get(kx_model* m, int64_t i, char* name, size_t name_len, double* vals7);
int kx_set_act_prescale(kx_model* m, const char* conv_name, int log2_scale);

/* ---- voice table on device + output packing -----------------------------
 * kx_set_voice_table uploads the table that `TTSKoko::load_voices` builds (kokorox/src/tts/koko.rs:1308-1334;
 * layout [n_voices][511][1][256] f32, row 510 zero, kokorox/src/utils/hf_cache.rs:284-309) once; requests then
 * carry (voice id, weight) pairs instead of 256 floats.  The mix is `mix_styles` (koko.rs:1255-1306) on the
 * GPU, bit for bit: max_mix = 1 copies row `lens[b] - 2` of the voice; otherwise the row is
 * sum_k row_k * (weights[k] * 0.1), in order, un-normalised; entries with voice id < 0 are skipped. */
int kx_set_voice_table(kx_model* m, const float* table, int n_voices);

/* Output forms of the reference (kx_infer_packed, kx_infer_voices and kx_dispatcher_submit_ex take these three):
 * 0 = f32 mono (ort_koko.rs:80-87), 1 = f32 stereo with every sample written twice (koko.rs:1239-1246), 2 = 16-bit PCM
 * `(s.clamp(-1,1) * 32767) as i16` (kokorox-websocket/src/lib.rs:701-704).
 * Packed on the GPU, so only the packed bytes cross PCIe. */
#define KX_PACK_F32_MONO 0
#define KX_PACK_F32_STEREO 1
#define KX_PACK_PCM16_MONO 2
/* The bodies the reference's servers send, mono, at 24 000 Hz unless the format word says otherwise (kx_infer_requests and
 * kx_dispatcher_submit_request only):
 * 3 = the HTTP body (kokorox-openai/src/lib.rs:416-425): the 44 bytes of `WavHeader::new(1, 24000, 32).write_header`
 *     (kokorox/src/utils/wav.rs:18-50: IEEE float, both size fields the reference's 0xFFFFFFFF placeholders) followed by the
 *     samples as f32 little-endian bit copies (a NaN keeps its payload); 44 + 4 S bytes.
 * 4 = the WebSocket chunk (`encode_audio`, kokorox-websocket/src/lib.rs:696-736): standard-alphabet base64 with `=` padding,
 *     no line breaks, no NUL, of a 16-bit WAV file: 44-byte header with its true sizes (36 + 2 S and 2 S), then
 *     `(s.clamp(-1.0, 1.0) * 32767.0) as i16` per sample with Rust's meaning (NaN -> 0, +-inf -> +-32767, the product rounded
 *     to f32 and truncated toward zero); 4 * ceil((44 + 2 S) / 3) characters, always ending in exactly one `=`, as S is a
 *     multiple of 600.  A request of more than 0xFFFFFFFF - 36 data bytes is refused with KX_ERR_INVALID.
 * (Form 2, as it has been since it was added, clamps with fmax / fmin, which drop a NaN: a NaN sample becomes -32767 there.) */
#define KX_PACK_WAV_F32 3
#define KX_PACK_WAV16_BASE64 4
/* Raw G.711, one byte per sample, no header (kx_infer_requests and kx_dispatcher_submit_request only): the 16-bit-input
 * algorithms that CPython's audioop.lin2ulaw / lin2alaw (width 2) implement, applied to form 4's 16-bit sample v (NaN -> 0).
 * 8 = mu-law: p = v >> 2 (arithmetic); p < 0: p = -p, mask 0x7F, else mask 0xFF; p = min(p, 8159) + 33; seg = the first index
 *     with p <= {0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF}; none: byte = 0x7F ^ mask; else
 *     byte = ((seg << 4) | ((p >> (seg + 1)) & 15)) ^ mask.
 * 9 = A-law: v >= 0: mask 0xD5, m = v, else mask 0x55, m = -v - 1; p = m >> 3; seg = the first index with
 *     p <= {0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF}; mantissa = (p >> 1) & 15 for seg 0 and 1, (p >> seg) & 15 above;
 *     byte = ((seg << 4) | mantissa) ^ mask.
 * Forms 5, 6 and 7 do not exist and are refused ("infer: unknown output format"). */
#define KX_PACK_MULAW 8
#define KX_PACK_ALAW 9
/* FLAC (kx_infer_requests and its siblings, kx_dispatcher_submit_request* only): a lossless body of form 4's 16-bit samples v
 * (NaN -> 0, +-inf -> +-32767) of the request's stream at its output rate, N of them -- after the join, the resampler and the levels
 * or the limiter; out_samples[r] and the marks are what they are for any other form.  RFC 9639 gives the meaning of every field;
 * the choices it leaves open are fixed here, so the body is a function of v and the rate, and the numpy definition
 * (kokorox_amd/voices.py: flac_body) and the GPU agree on every byte.  All fields MSB first.  F = ceil(N / 4096).
 *   Body: "fLaC"; a STREAMINFO block, not last: min = max block size 4096, min and max frame size the true ones over the F frames (0
 *     and 0 when F = 0), the output rate, 1 channel, 16 bits, N samples, the MD5 all zeros ("not computed"); a PADDING block, last,
 *     of p = (2 - the bytes of all frames) mod 4 zero bytes; frames f = 0 .. F - 1 of n = min(4096, N - 4096 f) samples.  The body is a
 *     multiple of 4 bytes, as every region of every form.
 *   Frame header: FF F8 (fixed block size); block-size nibble 1100 for n = 4096, else 0111 and n - 1 as 16 bits behind the frame
 *     number; rate nibble 0100 / 0101 / 0111 / 1010 for 8000 / 16 000 / 24 000 / 48 000 Hz; 08 (one channel, 16 bits); f in the
 *     format's UTF-8-like coding; CRC-8 (polynomial 0x07, from 0).  One subframe, zero bits to the byte boundary, CRC-16 (polynomial
 *     0x8005, from 0, not reflected) over the whole frame.  No wasted bits.
 *   Subframe: CONSTANT when all n samples are equal.  Else FIXED: for o = 0 .. min(4, n - 1) the residuals e_o[i], i >= o, in int32
 *     by the binomial forms (e_1 = v[i] - v[i-1], .., e_4 = v[i] - 4 v[i-1] + 6 v[i-2] - 4 v[i-3] + v[i-4]), folded as
 *     u = (e << 1) ^ (e >> 31); partition order P = 0 .. 6 when n = 4096, else 0; coding method 00 (4-bit parameters), never the
 *     escape; a partition's Rice parameter is the k in 0 .. 14 with the fewest bits, sum (u >> k) + (k + 1) count, the smaller k on a
 *     tie; bits(o, P) = 16 o + 6 + the sum over the partitions of 4 + their bits, the first partition holding (n >> P) - o
 *     residuals; the (o, P) with the fewest bits is taken, the smaller o on a tie, then the smaller P.  VERBATIM when that reaches or
 *     exceeds 16 n bits.
 *   A frame is at most 16 + 2 n bytes and a body at most 42 + 7 + the sum of those, rounded up to 4: the bound.  This is the one form
 *     whose size follows from the samples: out_bytes[r] is the body's true size, and the R bodies lie back to back by those sizes
 *     like all others (the copy from the device carries the bound; the host closes the gaps).
 * Not offered: LPC subframes, stereo, other block sizes, an MD5 signature, seek tables.  Forms 10 and 11 do not exist and are
 * refused like 5, 6 and 7. */
#define KX_PACK_FLAC 12
#define KX_FLAC_BLOCK 4096
/* IMA ADPCM in a WAV file (kx_infer_requests and its siblings, kx_dispatcher_submit_request* only): 4 bits per sample, the body a
 * telephone, an IVR or a small device decodes (WAVE_FORMAT_IMA_ADPCM, tag 0x0011, which is the form's number), a quarter of the
 * 16-bit size.  v[0..N) are form 4's 16-bit samples (NaN -> 0, +-inf -> +-32767, truncation toward zero) of the request's stream at
 * its output rate -- after the join, the resampler and the levels or the limiter; out_samples[r] and the marks are what they are
 * for any other form.  Every choice is fixed here, so the body is a function of v and the rate, and the numpy definition
 * (kokorox_amd/voices.py: adpcm_wav_body) and the GPU agree on every byte.  All fields little-endian.
 *   Block size by rate: A = 256 bytes at 8000 Hz, 512 at 16 000 and 24 000 Hz, 1024 at 48 000 Hz; a block holds P = 1 + 2 (A - 4)
 *     samples (505, 1017, 2041).  F = ceil(N / P) blocks; the samples past N in the last block repeat v[N - 1].
 *   Header, 60 bytes: "RIFF", 52 + A F, "WAVE"; "fmt ", 20: tag 0x0011, 1 channel, the rate, floor(rate A / P) bytes per second,
 *     block align A, 4 bits per sample, cbSize 2, wSamplesPerBlock P; "fact", 4: N; "data", A F.  The body is 60 + A F bytes, a
 *     multiple of 4 as every region.  A body whose N (the fact chunk) or RIFF size would pass 0xFFFFFFFF is refused with
 *     KX_ERR_INVALID, as form 4's is.
 *   Block: int16 predictor = the block's first sample; uint8 index i0; uint8 0; then A - 4 bytes of two codes each, the earlier
 *     sample in the LOW nibble.
 *   Start index: i0 = the smallest i with STEP[i] >= max over t = 0..7 of |v[t + 1] - v[t]|, the block's own (padded) samples
 *     counted from its first, 88 when there is none.  (Eight differences, not the first alone: a block that begins near an extremum
 *     of the waveform would otherwise start with far too small a step; DESIGN.md section 7 has the measurements.)
 *     A block is thereby a function of its own samples: all blocks of all requests are encoded at once, and a body is the same
 *     bytes whatever it was batched with.
 *   Per sample s (the standard IMA / DVI step, the algorithm of CPython's audioop.lin2adpcm), with the 89 steps STEP = 7, 8, 9, ..
 *     29794, 32767 (kokorox_amd/csrc/adpcm_steps.h) and the index steps -1, -1, -1, -1, 2, 4, 6, 8: d = s - pred; the code's bit 8
 *     is set when d < 0, and d = |d|; vp = step >> 3; three compare-subtract rounds at step, step >> 1 and step >> 2 set bits
 *     4, 2 and 1, each subtracting the compared value from d and adding it to vp; pred -= vp or += vp by the sign, clamped to
 *     [-32768, 32767]; index += the index step of the code's low three bits, clamped to [0, 88]; step = STEP[index].
 * Not offered: stereo, other block sizes, raw DVI4 without a container, G.726.  Forms 13..16 do not exist and are refused. */
#define KX_PACK_ADPCM_WAV 17
#define KX_ADPCM_MAX_BLOCK 1024
/* The plain 16-bit WAV file, as bytes: what form 4 encodes as base64 -- the 44-byte header with its true sizes, then the 16-bit
 * samples with form 4's meaning; 44 + 2 N bytes, padded with zero bytes to a multiple of 4 as every region is (out_bytes[r]
 * counts the padding; the header's sizes do not).  Refused where form 4 is (a RIFF size past 0xFFFFFFFF).  Requests only. */
#define KX_PACK_WAV16 18
/* The block of form 17 at the rate of `format_word` (only bits 8..11 are read): *block_bytes = A, *samples_per_block = P (either
 * may be NULL).  Host only, touches no GPU; KX_ERR_INVALID for a rate code above 3. */
int kx_adpcm_block(int format_word, int32_t* block_bytes, int32_t* samples_per_block);

/* The `format` / `formats[]` value of kx_infer_requests and kx_dispatcher_submit_request is a WORD: bits 0..7 = the form above
 * (0..4, 8, 9, 12, 17, 18), bits 8..11 = the output sample rate, every other bit zero (else "infer: unknown output format").  Rate code 0 =
 * 24 000 Hz, the model's own rate: the bytes of the plain forms, unchanged.  Codes 4..15 are refused with KX_ERR_INVALID,
 * "infer: unknown output sample rate".  Every form combines with every rate.  (kx_infer, kx_infer_packed, kx_infer_voices,
 * kx_dispatcher_submit and kx_dispatcher_submit_ex keep taking the forms 0..2 and nothing else.)
 *
 * With a rate code the request's stream x[0..S) -- its chunks' samples appended, S a multiple of 600 -- is resampled on the GPU
 * as a whole before its form is applied (a chunk boundary is invisible to the filter); out_samples[r] then counts samples at
 * the OUTPUT rate, S L / M, the WAV headers of forms 3 and 4 carry that rate and its byte rate (rate x 4, rate x 2), and form
 * 4's text ends in zero, one or two `=` ((44 + 2 S L / M) mod 3 takes all three values; its 4 GiB refusal counts output samples).
 *
 *   code   rate     (L, M)   Q = max(L, M)   C = 24 Q   N = 2 C + 1 taps
 *    1     8000     (1, 3)        3             72          145
 *    2    16000     (2, 3)        3             72          145
 *    3    48000     (2, 1)        2             48           97
 *
 * Taps: h[i] = sinc((i - C) / Q) * kaiser_N(i; beta = 10.0) in float64 (sinc(t) = sin(pi t) / (pi t)), scaled so that their sum
 * is L, rounded once to float32 (committed as bit patterns: kx_resample_filter hands them out).  With x[j] = 0 outside the stream,
 *     y[n] = f32( sum_j f64(h[n M - j L + C]) * f64(x[j]) ),   n in [0, S L / M),
 * over every j in [0, S) with 0 <= n M - j L + C < N, in ASCENDING j, the accumulator a float64 that starts at +0, one addition
 * per term, then one round-to-nearest-even conversion to f32.  A product of two float32 values is exact in float64, so a fused
 * multiply-add and a separate multiply and add give the same bits: a host loop in that order reproduces the GPU bit for bit
 * (subnormal and infinite inputs aside).  Pass band to 0.85 of the smaller Nyquist frequency within 2e-5, -6 dB at it, below
 * -99 dB from 1.15 of it. */
#define KX_PACK_RATE_24000 0x000
#define KX_PACK_RATE_8000 0x100
#define KX_PACK_RATE_16000 0x200
#define KX_PACK_RATE_48000 0x300
#define KX_RESAMPLE_MAX_TAPS 145
/* The filter of a format word's rate code, from the library's one table; host only, touches no GPU.  Any of L, M, n_taps, taps
 * may be NULL; taps receives n_taps floats (cap = its capacity in floats, KX_RESAMPLE_MAX_TAPS always suffices).  Rate code 0
 * gives L = M = 1 and no taps.  An unknown word is refused as by kx_infer_requests. */
int kx_resample_filter(int format_word, int32_t* L, int32_t* M, int32_t* n_taps, float* taps, int cap);

/* kx_infer with device-side style lookup/mix and packed output.  *out = library-owned bytes of the B utterances back
 * to back (kx_free_packed); out_bytes[b] / out_samples[b] per utterance. */
int kx_infer_voices(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B,
                    const int32_t* voice_ids, const float* weights, int max_mix, const float* speeds, int n_speed,
                    uint64_t seed, uint32_t flags, int format, void** out, int64_t* out_bytes, int64_t* out_samples);
/* kx_infer (explicit style rows) with packed output. */
int kx_infer_packed(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B, const float* styles,
                    const float* speeds, int n_speed, uint64_t seed, uint32_t flags, int format, void** out,
                    int64_t* out_bytes, int64_t* out_samples);
void kx_free_packed(void* p);

/* The chunk loop of `TTSKoko::tts_raw_audio` (kokorox/src/tts/koko.rs:947-1191: a text is split into chunks of at most 500
 * tokens, run one after the other, the waveforms appended with no cross-fade) as ONE forward with the bodies packed on the
 * GPU.  Rows are chunks; request r owns chunks_per_request[r] consecutive rows (every entry >= 1, their sum = B, otherwise
 * KX_ERR_INVALID).  The voice is per row: `styles` [B,256], or NULL with `voice_ids` / `weights` [B,max_mix] as
 * kx_infer_voices (the row of a voice is lens[b] - 2 of each chunk, koko.rs:1166).  Row b draws the noise stream
 * (seed, utterance base + b) exactly as kx_infer.  `formats` [n_format], n_format = 1 (shared) or R: format words (a KX_PACK_*
 * form, optionally | KX_PACK_RATE_*).
 * *out = one pooled page-locked buffer (kx_free_packed) holding the R requests back to back: request r is the header of its
 * form, if any, then its chunks' samples in order with nothing between chunks; out_bytes[r], out_samples[r] (= 600 x the sum
 * of its chunks' frames, x L / M with a rate code) per request.  Forms 0..2 at rate code 0 give the bytes of kx_infer_packed. */
int kx_infer_requests(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B,
                      const int32_t* chunks_per_request, int R, const float* styles, const int32_t* voice_ids,
                      const float* weights, int max_mix, const float* speeds, int n_speed, uint64_t seed, uint32_t flags,
                      const int32_t* formats, int n_format, void** out, int64_t* out_bytes, int64_t* out_samples);

/* ---- token marks: where each input token sits in a request's stream -------------------------------------------------------
 * The duration head decides how many 600-sample frames every token occupies; the marks give that as sample offsets in the
 * request's own stream, at the request's own output rate, across its chunks.
 *   Request r has chunks c = 0 .. n-1; chunk c has T_c tokens, its two 0 pads included.  d_c[t] are the durations the forward
 *   USED, in frames: after kx_set_pinned_durations if a pattern is set, after the division by the speed and the clamp to >= 1.
 *   The request's format word has the rate (L, M); K = 600 L / M (600 at 24 000 Hz, 200 at 8000, 400 at 16 000, 1200 at
 *   48 000).  F_c = sum over t of d_c[t].  The marks of request r are, chunk after chunk, T_c + 1 int64 values per chunk:
 *       m_c[t] = K * ( sum over c' < c of F_c'  +  sum over t' < t of d_c[t'] ),   t = 0 .. T_c
 * Token t of chunk c occupies the output samples [m_c[t], m_c[t+1]) of the request's stream.  m_0[0] = 0;
 * m_c[T_c] = m_{c+1}[0] (the chunk boundary is stored twice on purpose: every chunk indexes on its own); the last value equals
 * out_samples[r]; request r has sum over c of (T_c + 1) marks.
 * Marks count SAMPLES of the stream, not bytes, and do not depend on the form: a stereo pair counts once, a WAV header and
 * base64 are not counted.  The resampler's filter is symmetric about its tap C (kx_resample_filter), so output sample n sits
 * at time n / rate with no delay: that is why scaling a 24 000 Hz offset by L / M is exact.
 *
 * kx_infer_requests with marks for every request.  *out, out_bytes, out_samples: exactly those of kx_infer_requests (same
 * bytes, sizes, layout).  *out_marks points INTO the buffer of *out (8-byte aligned, behind the bodies) and holds the marks of
 * the R requests back to back, out_n_marks[r] values for request r; it is never freed on its own and stays valid until *out is
 * released with kx_free_packed.  A null out_marks or out_n_marks: KX_ERR_INVALID "infer: null marks argument"; everything
 * kx_infer_requests refuses is refused here the same way with the same text. */
int kx_infer_requests_marks(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B,
                            const int32_t* chunks_per_request, int R, const float* styles, const int32_t* voice_ids,
                            const float* weights, int max_mix, const float* speeds, int n_speed, uint64_t seed, uint32_t flags,
                            const int32_t* formats, int n_format, void** out, int64_t* out_bytes, int64_t* out_samples,
                            int64_t** out_marks, int64_t* out_n_marks);

/* ---- joins: shaping the seams of a request on the GPU ------------------------------------------------------------------------
 * Every chunk carries a 0 pad token at both ends and the duration head gives each pad some frames: a request of several chunks
 * has a lead-in, a tail and inner silences whose lengths the model chose.  A join spec trims those pad spans, puts a pause of
 * the caller's choice between consecutive chunks and fades the trimmed edges, before the request is resampled and packed.
 * Everything is defined at 24 000 Hz, before resampling: 1 ms is 24 samples.
 *
 * Chunk c (row b) has T tokens, used durations d[0..T) (the ones the marks use: after pinning, after the speed, after the
 * clamp), F = sum of d, valid samples x[0..600 F).
 *   Which edges are trimmed.  The head edge of a row is SELECTED if the row has T >= 3 and either (it is the request's first
 *   row and HEAD is set) or (it is not the first row and INNER is set); the tail edge symmetrically, with TAIL and INNER.  Rows
 *   with T < 3 are never trimmed: their one or two tokens are both pads, a lead span and a tail span would overlap.
 *   Per row, with k = 24 keep_ms:  skip = max(0, 600 d[0] - k) if the head is selected, else 0;
 *   cut = max(0, 600 d[T-1] - k) if the tail is selected, else 0;  keep = 600 F - skip - cut (>= 600: the middle tokens have
 *   d >= 1);  gap = 24 pause_ms for every row but the request's last, else 0.
 *   Fades, with n = 24 fade_ms (2 n <= 576 < 600: the two never overlap).  If the head is selected and n > 0, sample i < n of
 *   the kept segment is f32(f64(x) * (f64(2 i + 1) / f64(2 n))); if the tail is selected and n > 0, sample keep - 1 - i, i < n,
 *   gets the same expression: one float64 division, one float64 product, one round-to-nearest-even conversion.  A NaN stays a
 *   NaN.
 *   The request's stream: for each chunk in order, x[skip .. skip + keep) with its fades, then gap zeros (+0.0f).  Its length
 *   is S' = sum of (keep + gap); every term is a multiple of 24, so S' L / M is exact at all four rates.  The stream is then
 *   resampled as a whole -- the zeros and the cuts are invisible to the filter, exactly as chunk boundaries are -- and packed
 *   in its form exactly as a plain request: the WAV headers, the `=` count, out_samples[r] = S' L / M and the 4 GiB refusal of
 *   form 4 all follow S'.
 *   Marks of a joined request.  With P_c = sum over c' < c of (keep_c' + gap_c') and u = 600 x sum over t' < t of d_c[t']:
 *       m_c[t] = (P_c + clamp(u - skip_c, 0, keep_c)) L / M,   t = 0 .. T_c
 *   A cut part of a pad collapses onto the edge; m_c[T_c] <= m_{c+1}[0], the difference is the pause and belongs to no token;
 *   the last value equals out_samples[r]; all values are multiples of 24 before scaling, so they are exact integers.
 *   A spec of all zeros gives the bytes and marks of kx_infer_requests_marks. */
#define KX_JOIN_TRIM_HEAD  1u  /* the request's lead-in: the first pad of its first chunk            */
#define KX_JOIN_TRIM_TAIL  2u  /* the request's tail: the last pad of its last chunk                 */
#define KX_JOIN_TRIM_INNER 4u  /* at every boundary between two chunks: the last pad of the earlier
                                  chunk and the first pad of the later one                           */
typedef struct kx_join {
    uint32_t flags;     /* the three bits above, every other bit zero            */
    int32_t  keep_ms;   /* 0..1000: of a trimmed pad span at most this much stays */
    int32_t  pause_ms;  /* 0..5000: zeros inserted between consecutive chunks     */
    int32_t  fade_ms;   /* 0..12: linear fade at every trimmed edge               */
} kx_join;
/* kx_infer_requests_marks with a join spec per request: joins [n_join], n_join = 1 (shared) or R.  out_marks / out_n_marks may
 * BOTH be NULL (no marks); exactly one NULL: "infer: null marks argument".  Refused with KX_ERR_INVALID before any device work:
 * a null `joins` ("infer: null join argument"), n_join not 1 or R ("infer: bad join count"), a stray flag bit or a field outside
 * its range ("infer: bad join"); everything kx_infer_requests refuses is refused the same way with the same text. */
int kx_infer_requests_joined(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B,
                             const int32_t* chunks_per_request, int R, const float* styles, const int32_t* voice_ids,
                             const float* weights, int max_mix, const float* speeds, int n_speed, uint64_t seed, uint32_t flags,
                             const int32_t* formats, int n_format, void** out, int64_t* out_bytes, int64_t* out_samples,
                             int64_t** out_marks, int64_t* out_n_marks, const kx_join* joins, int n_join);

/* ---- levels: gain, peak normalisation and ceiling of a request on the GPU ----------------------------------------------------
 * The 16-bit forms (2, 4, and through them 8 and 9) clamp to +-1 without a word, the resampler's steep filter overshoots (a
 * stream inside +-1 at 24 000 Hz need not stay inside it at the output rate) and a voice mix is un-normalised.  A level spec
 * sets the level of a request's body where the body is made, behind the join and behind the resampler.
 *   The stream.  Request r's stream z[0..N) is what form 0 in its format word would hold, N = out_samples[r]: after the join,
 *   after the resampler, at the request's output rate.  Levels are measured and applied on that stream, the packer's input, so
 *   a ceiling holds for the samples the body actually carries.
 *   The peak.  p = the maximum of |z[n]| over all n for which z[n] is not a NaN, as a float32; p = 0 when there is no such n.
 *   +inf counts.  p is "usable" when 0 < p < +inf.
 *   The gain.  g is a float64.  Mode 0: g = f64(gain).  Mode 1: g = f64(peak) / f64(p) if p is usable, else 1.0.  Mode 2:
 *   g = f64(gain); if p is usable and g * f64(p) > f64(peak) (one float64 product), then g = f64(peak) / f64(p).
 *   The samples.  z'[n] = f32(g * f64(z[n])): one float64 product and one round-to-nearest-even conversion.  A NaN stays a
 *   NaN.  The form (f32, stereo, PCM16, WAV, base64, G.711) is then applied to z' exactly as it is applied to z without
 *   levels.  Marks, out_samples, headers and sizes do not change.
 *   Valid specs.  mode is 0, 1 or 2; 0 <= gain <= 64, and gain is exactly 1.0f in mode 1; peak is +0.0f in mode 0 and
 *   2^-15 <= peak <= 1 in modes 1 and 2; a NaN fails every one of these.  The plain spec is {0, 1.0f, 0.0f}: z' = z.
 *   A property.  f32((f64(peak) / f64(p)) * f64(p)) == peak exactly: the quotient is within 2^-53 relative of peak / p, the
 *   product within 2^-52 relative of the float32 value peak, far inside the half-ulp 2^-25 that rounds back onto it; rounding
 *   is monotone, so no |z'[n]| exceeds it.  A request that mode 1 or mode 2 normalises therefore has a largest |sample| of
 *   exactly `peak`, and with peak <= 1 the clamp of the 16-bit forms never engages.
 *   True peak.  KX_PEAK_TRUE (0x100) OR-ed into kx_level.mode or kx_loudness.mode replaces p by the true peak tp, in the gain
 *   rules and in slot 0 of out_levels / out_loudness: a body whose samples stay inside `peak` can still overshoot it between
 *   the samples, in the next resampler, codec or DAC (EBU R128 pairs -23 LUFS with -1 dBTP).  The valid modes are exactly
 *   {0, 1, 2} and {0, 1, 2} | 0x100 for levels, {0, 1} and {0, 1} | 0x100 for loudness; the rules on gain, peak and target_lufs
 *   follow the low byte; every other bit is refused as before.
 *     Oversampling.  Four times at every output rate (the factor libebur128 uses below 96 kHz), 12 input samples either side:
 *     U = 4, C = 48, N = 97, w[i] = sinc((i - 48) / 4) * kaiser_97(i; beta = 8) in float64; for phi = 1, 2, 3 and m = 0..23,
 *     t_phi[m] = w[4 m + phi] / (sum over m of w[4 m + phi]) in float64, rounded once to float32: 72 taps, every phase with DC
 *     gain 1 (kx_truepeak_filter hands them out).  Phase 0 is the identity (sinc(k) = delta) and is not computed: the samples
 *     themselves stand for it.
 *     The input.  x[j] = f64(z[j]) if z[j] is finite and 0 <= j < N, else 0.0 -- z the stream defined above.
 *     Interpolated values.  For n in [0, N) and phi in 1..3, u_phi[n] = f32(sum over j = n - 11 .. n + 12, ascending, of
 *     f64(t_phi[n - j + 12]) * x[j]): a float64 accumulator from +0, one addition per term, one round-to-nearest-even
 *     conversion.  A float32 x float32 product is exact in float64, so fused and unfused forms agree and a host loop in the same
 *     order equals the GPU bit for bit.
 *     The result.  tp = max(p, max over n and phi of |u_phi[n]|) as a float32: tp >= p always.  tp is "usable" when
 *     0 < tp < +inf; a u that overflows to +-inf makes it unusable, as +inf does for p.
 *     The gain and the property.  The gain rules stand with tp in place of p.  The property becomes an inequality: with
 *     g = f64(peak) / f64(tp) no |z'[n]| exceeds `peak` (monotone rounding, p <= tp), so the 16-bit and G.711 forms still cannot
 *     clip.  The true peak of z' equals `peak` only up to the rounding of the interpolation (z' is rounded to float32 before it
 *     would be interpolated again), not exactly.
 *     The filter.  A phase's response is within 8.1e-5 of the ideal fractional delay up to half the Nyquist frequency and
 *     within 1.35e-3 (0.012 dB) up to 0.8 of it.  A 4800-sample fs/4 sine of amplitude 0.5 at phase 0 / 45 / 60 / 67.5 degrees
 *     reads -6.021 / -5.914 / -5.954 / -5.847 dBTP, inside the -6.0 +0.2 / -0.4 window of EBU Tech 3341 cases 15..18 (what lies
 *     above -6.02 is the Gibbs transient at the burst's edges, not filter error). */
#define KX_LEVEL_GAIN      0u  /* multiply by `gain`                                                   */
#define KX_LEVEL_NORMALIZE 1u  /* scale so that the body's largest |sample| is `peak`                  */
#define KX_LEVEL_CEILING   2u  /* multiply by `gain`, but never let the largest |sample| exceed `peak` */
#define KX_PEAK_TRUE   0x100u  /* OR-ed into a kx_level or kx_loudness mode: `peak` bounds the true peak, p is tp */
typedef struct kx_level { uint32_t mode; float gain; float peak; } kx_level;   /* 12 bytes */
/* The 72 taps of the true-peak interpolator as [3][24] float32, phase 1 first.  Host only; KX_ERR_INVALID for a null `taps` or
 * cap < 72. */
int kx_truepeak_filter(float* taps, int cap);
/* kx_infer_requests_joined with a level spec per request: levels [n_level], n_level = 1 (shared) or R.  `joins` may be NULL
 * with n_join == 0 here (no joins); otherwise the join rules and refusals of kx_infer_requests_joined apply.  out_levels may be
 * NULL; when given it receives [R][2] doubles, f64(p) and g of request r as the GPU computed them.  Through this entry every
 * request is measured, a plain spec included: a plain spec with out_levels is a peak meter.  Body, marks and levels leave the
 * device in one copy.  Refused with KX_ERR_INVALID before any device work, after everything kx_infer_requests_joined refuses
 * (with its texts): a null `levels` ("infer: null level argument"), n_level not 1 or R ("infer: bad level count"), an invalid
 * spec ("infer: bad level"). */
int kx_infer_requests_levelled(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B,
                               const int32_t* chunks_per_request, int R, const float* styles, const int32_t* voice_ids,
                               const float* weights, int max_mix, const float* speeds, int n_speed, uint64_t seed, uint32_t flags,
                               const int32_t* formats, int n_format, void** out, int64_t* out_bytes, int64_t* out_samples,
                               int64_t** out_marks, int64_t* out_n_marks, const kx_join* joins, int n_join, const kx_level* levels,
                               int n_level, double* out_levels);

/* ---- loudness: ITU-R BS.1770 metering and LUFS normalisation of a request on the GPU -------------------------------------------
 * Two bodies with the same peak can differ by many LU.  A loudness spec measures the integrated loudness of a request's body
 * where the body is made, and scales it to a target.
 *   The stream.  z[0..N) is exactly the stream "levels" defines: what form 0 of the request's format word would hold, after the
 *   join and after the resampler, at the output rate fs in {24000, 8000, 16000, 48000}.  The peak p keeps its meaning of "levels".
 *   The input.  x[n] = f64(z[n]) if z[n] is finite, else 0.0: a NaN or an infinity does not poison the recurrence.
 *   K-weighting.  Two biquads, shelf first, then high-pass, direct form I, float64, zero initial state:
 *       v[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 v[n-1] - a2 v[n-2],   w[n] likewise from v with the high-pass's coefficients.
 *   With K = tan(pi f0 / fs) -- shelf: f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, Vh = 10^(G/20),
 *   Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2, b = [(Vh + Vb K/Q + K^2)/a0, 2 (K^2 - Vh)/a0, (Vh - Vb K/Q + K^2)/a0],
 *   a1 = 2 (K^2 - 1)/a0, a2 = (1 - K/Q + K^2)/a0; high-pass: f0 = 38.13547087602444, Q = 0.5003270373238773, b = [1, -2, 1], a1
 *   and a2 as for the shelf with this K and Q.  At 48 000 Hz these are the standard's published coefficients.  The four rates'
 *   coefficients are committed once as float64 bit patterns (kx_loudness_filter hands them out).
 *   Blocks.  hop = fs / 10 samples.  e[k] = the sum of w[n]^2 over hop k, k < H = floor(N / hop); a trailing partial hop is
 *   ignored.  Block j covers hops j..j+3: z_j = (e[j] + e[j+1] + e[j+2] + e[j+3]) / (4 hop), j < J = H - 3.
 *   Gating, in the energy domain.  A block passes the absolute gate when z_j > 10^((-70 + 0.691) / 10); m1 = the mean of z_j over
 *   those blocks; a block passes the relative gate when it passes the absolute gate and z_j > 0.1 m1; n_g = the number of blocks
 *   that pass both, m2 their mean.  I = -0.691 + 10 log10(m2) LUFS (mono: channel weight 1).  I is undefined when J < 1 or
 *   n_g = 0, and then reported as a quiet NaN.
 *   The gain.  Mode 0 (a meter): g = 1.  Mode 1: g = 10^((f64(target_lufs) - I) / 20) if I is defined, else 1.0; then, if p is
 *   usable and g * f64(p) > f64(peak), g = f64(peak) / f64(p) -- the ceiling rule of KX_LEVEL_CEILING, so the 16-bit and G.711
 *   forms cannot clip.
 *   The samples.  z'[n] = f32(g * f64(z[n])), then the form, as in "levels".  Marks, sizes and headers do not change.
 *   Valid specs.  Mode 0: target_lufs and peak are +0.0f.  Mode 1: -70 <= target_lufs <= 0 and 2^-15 <= peak <= 1; a NaN fails.
 *   Either mode may carry KX_PEAK_TRUE ("levels", True peak): p is then tp, in the ceiling and in out_loudness.
 *   The GPU's e[k] agree with a sequential float64 evaluation to about 1e-14 relative; I, g and e[k] of a request do not depend on
 *   what it was batched with. */
#define KX_LOUDNESS_MEASURE   0u  /* measure only: g = 1                                                        */
#define KX_LOUDNESS_NORMALIZE 1u  /* scale to `target_lufs`, but never let the largest |sample| exceed `peak`   */
typedef struct kx_loudness { uint32_t mode; float target_lufs; float peak; } kx_loudness;   /* 12 bytes */
/* The ten K-weighting coefficients of a format word's rate: shelf b0 b1 b2 a1 a2, then high-pass b0 b1 b2 a1 a2.  Host only;
 * KX_ERR_INVALID for an unknown word, as kx_resample_filter. */
int kx_loudness_filter(int format_word, double* out10);
/* kx_infer_requests_joined with a loudness spec per request: loudness [n_loudness], n_loudness = 1 (shared) or R.  `joins` may
 * be NULL with n_join == 0 (no joins).  out_loudness may be NULL; when given it receives [R][4] doubles: f64(p), g, I and n_g of
 * request r as the GPU computed them.  Body, marks, levels and loudness leave the device in one copy.  Refused with
 * KX_ERR_INVALID before any device work, after everything kx_infer_requests_joined refuses: a null `loudness`
 * ("infer: null loudness argument"), n_loudness not 1 or R ("infer: bad loudness count"), an invalid spec ("infer: bad loudness"). */
int kx_infer_requests_loudness(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B,
                               const int32_t* chunks_per_request, int R, const float* styles, const int32_t* voice_ids,
                               const float* weights, int max_mix, const float* speeds, int n_speed, uint64_t seed, uint32_t flags,
                               const int32_t* formats, int n_format, void** out, int64_t* out_bytes, int64_t* out_samples,
                               int64_t** out_marks, int64_t* out_n_marks, const kx_join* joins, int n_join,
                               const kx_loudness* loudness, int n_loudness, double* out_loudness);

/* ---- limiter: a look-ahead peak limiter for a request's body on the GPU, sample peak or true peak ------------------------------------
 * Every other scaling here is one gain per request: where a loudness target meets its ceiling the whole body is pulled down, and
 * speech, with a crest factor of 15-20 dB, meets it routinely.  A limit spec drives the body to the level asked for and turns down
 * only the neighbourhood of the samples that would pass `peak`.
 *   The stream.  z[0..N) at the output rate fs is exactly the stream of "levels": after the join, after the resampler.  p, tp, I and
 *   n_g keep their meanings of "levels" and "loudness"; with KX_PEAK_TRUE in the mode p is tp.
 *   The static gain g, float64.  Mode 0: g = f64(gain).  Mode 1: g = 10^((f64(target_lufs) - I) / 20) if I is defined, else 1.0.
 *   Drive cap: if p is usable and g * f64(p) > 4 f64(peak) (one product; 4 peak is exact), g = 4 f64(peak) / f64(p) -- the ceiling
 *   rule of KX_LEVEL_CEILING with the ceiling 12 dB up: at most 12.04 dB ever goes into the limiter.  z1[n] = f32(g * f64(z[n])).
 *   Window and weights.  W = fs / 200 samples: 40, 80, 120, 240 at 8, 16, 24, 48 kHz; 5 ms spans a pitch period down to 100 Hz, so
 *   the gain does not ride single pitch pulses.  h_W[i], i = 0..2W, is (1 - cos(2 pi (i + 1) / (2 W + 2))) divided by its float64
 *   sum and rounded once to float32; the four tables are committed as bit patterns (kx_limit_filter hands them out).
 *   Envelope, float32.  a[n] = |z1[n]| if z1[n] is finite, else 0.  With KX_PEAK_TRUE: a[n] = max(|z1[n]|, |u_phi[n-1]|, |u_phi[n]|)
 *   over phi = 1..3, u the interpolator of "True peak" applied to z1 -- same taps, same order, non-finite values and values outside
 *   the stream taken as 0 -- and u_phi[-1] = 0.
 *   Required gain.  c[n] = 1.0f if a[n] <= peak, else f32(f64(peak) / f64(a[n])); c[k] = 1.0f for k outside [0, N).
 *   Sliding minimum.  m[j] = the smallest c[k], k in [j - W, j + W], for every j in [-W, N + W): float32, order-free.  An m outside
 *   the stream still sees the c inside it; without that the gain would rise towards the ends and the bound below would break.
 *   Smoothing.  s[n] = the sum over j = n - W .. n + W, ascending, of f64(h_W[j - n + W]) * f64(m[j]): a float64 accumulator from
 *   +0, one addition per term.  A float32 x float32 product is exact in float64, so fused and unfused forms agree and a host loop
 *   in this order gives the GPU's bits.  Per sample: if every m[j] of the sum is 1.0f, s[n] = 1.0 exactly and the sum is not taken.
 *   Output.  z2[n] = f32(s[n] * f64(z1[n])); then, if |z2[n]| > peak, z2[n] = copysign(peak, z2[n]).  A NaN stays a NaN, +-inf
 *   becomes +-peak.  The form is applied to z2 exactly as to z; marks, sizes and headers do not change.
 *   Sample ceiling.  For j in [n - W, n + W], n lies in j's window, so m[j] <= c[n]; a weighted mean of these stays within rounding
 *   of c[n], and the final clamp makes |z2[n]| <= peak unconditional.  With KX_PEAK_TRUE the true peak of z2 is bounded only
 *   approximately, because the gain acts at the sample rate: on voiced, noise and click streams driven to the cap's full 12 dB it
 *   stayed within 6e-7 of peak at all four rates, where the sample-only limiter leaves 0.5 to 20 per cent; the tests hold it to
 *   peak (1 + 1e-4).  The loudness of a limited body
 *   is at or below the target: I is the input's loudness, it is not measured again.
 *   Valid specs.  Low byte 0 (KX_LIMIT_GAIN): 0 <= gain <= 64 and target_lufs is +0.0f.  Low byte 1 (KX_LIMIT_LOUDNESS): gain is
 *   exactly 1.0f and -70 <= target_lufs <= 0.  Both: 2^-15 <= peak <= 1.  KX_PEAK_TRUE may be OR-ed in; every other bit is refused
 *   and a NaN fails every rule.  There is no plain limit spec: a request without a limiter takes the older entries, or sits beside
 *   limited ones in a dispatcher batch.
 *   Report.  Five doubles per request: f64(p), g, I, n_g (a quiet NaN and 0 in mode 0) and r = f64(the smallest f32(s[n])), 1.0 for
 *   a request nothing limited.  Bytes, marks and the five values of a request do not depend on what it was batched with. */
#define KX_LIMIT_GAIN     0u  /* drive by `gain`, limit at `peak`                                            */
#define KX_LIMIT_LOUDNESS 1u  /* drive to `target_lufs` (BS.1770, as KX_LOUDNESS_NORMALIZE), limit at `peak` */
#define KX_LIMIT_MAX_TAPS 481 /* 2 W + 1 at 48 000 Hz                                                        */
typedef struct kx_limit { uint32_t mode; float gain; float target_lufs; float peak; } kx_limit;   /* 16 bytes */
/* W and the 2 W + 1 weights h_W of a format word's rate into taps[cap], cap >= 2 W + 1 (KX_LIMIT_MAX_TAPS always does).  Host only;
 * KX_ERR_INVALID for an unknown word, as kx_resample_filter. */
int kx_limit_filter(int format_word, int32_t* W, float* taps, int cap);
/* kx_infer_requests_joined with a limit spec per request: limits [n_limit], n_limit = 1 (shared) or R.  `joins` may be NULL with
 * n_join == 0 (no joins).  out_limits may be NULL; when given it receives [R][5] doubles, the report above.  Body, marks and all
 * blocks leave the device in one copy.  Refused with KX_ERR_INVALID before any device work, after everything
 * kx_infer_requests_joined refuses: a null `limits` ("infer: null limit argument"), n_limit not 1 or R ("infer: bad limit count"),
 * an invalid spec ("infer: bad limit"). */
int kx_infer_requests_limited(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B,
                              const int32_t* chunks_per_request, int R, const float* styles, const int32_t* voice_ids,
                              const float* weights, int max_mix, const float* speeds, int n_speed, uint64_t seed, uint32_t flags,
                              const int32_t* formats, int n_format, void** out, int64_t* out_bytes, int64_t* out_samples,
                              int64_t** out_marks, int64_t* out_n_marks, const kx_join* joins, int n_join, const kx_limit* limits,
                              int n_limit, double* out_limits);

/* ---- prosody: per-token rate, fixed durations, pitch and energy of a call, and what the model chose -----------------------------
 * The input side of a call beyond ids, style and one speed per row.  Every array of a kx_prosody that is not NULL is
 * [B, t_stride], laid out as `ids`; only t < lens[b] is read.  A NULL array is neutral; a kx_prosody of four NULLs, or a NULL
 * kx_prosody*, gives the call without prosody bit for bit.
 *   Valid values.  0.25 <= rate <= 4, 0 <= frames <= 50, 0.25 <= pitch <= 4, 0 <= energy <= 4; a NaN fails every rule.  Checked on
 *   the host before any device work: KX_ERR_INVALID "infer: bad prosody" (dispatcher: "dispatcher_submit_request: bad prosody").
 *   Durations.  Token t of row b: (1) s = the float32 sum of the 50 sigmoids, as without prosody; (2) s = s / speed_b; (3) with
 *   `rate`, s = s / rate[t], one float32 division (x / 1.0f is x: neutral spans keep their bits); (4) rintf, at least 1, and the
 *   guard of the row's end, as without prosody; (5) the model's pinned pattern, if set (kx_set_pinned_durations); (6) with `frames`
 *   and frames[t] >= 1, d = frames[t]: it replaces whatever came before.  A row longer than its alignment is cut and refused as
 *   without prosody ("infer: speed too low ...").  Marks and joins are defined on these USED durations, so they follow.
 *   Curves.  The model's F0 and N curves live on 2 F_b steps per row (F_b frames); step j belongs to token tau(j) = the token of
 *   frame j >> 1.  With a per-token ratio rho (pitch or energy) and cl(i) = min(max(i, 0), 2 F_b - 1):
 *       r[j] = (sum over k = -2 .. 2, ascending, of f64(w_k) * f64(rho[tau(cl(j + k))])) / 9.0,   w = (1, 2, 3, 2, 1),
 *   a float64 accumulator from +0, one addition per term, one division.  Five equal ratios of 1 give exactly 1.0; the 5-step
 *   triangle (62.5 ms wide) keeps a ratio step between two tokens from becoming a pitch jump.
 *   F0: if !(F0[j] > 10.0f) (unvoiced for the source, or NaN) F0'[j] = F0[j]; otherwise v = f32(f64(F0[j]) * r[j]) and
 *   F0'[j] = v > 10.0f ? v : the float above 10 (bits 0x41200001): the model's voiced / unvoiced decision never flips.
 *   N: N'[j] = f32(f64(N[j]) * e[j]) for every j; a NaN stays.  Both readers of the curves, the harmonic source and the decoder,
 *   take the shaped values.  Under KX_FLAG_TAPS, "pred.F0.raw" / "pred.N.raw" hold the curves before and "pred.F0" / "pred.N" after.
 *   The API takes ratios, not semitones: exp2 in float64 is not the same bits on every libm.  float32(2 ^ (p / 12)) is the
 *   caller's to compute (Python: voices.semitones).
 *   Report.  Four float32 values per token of a request, chunk after chunk: [0] the mean of F0'[j] over the token's steps
 *   j in [2 start, 2 (start + d)) with F0'[j] > 10 -- a float64 sum in ascending j, divided by the count, rounded once; +0.0f when
 *   none is voiced (or d = 0); [1] that count; [2] f32(the float64 sum of N'[j] over all its steps, ascending, / (2 d)), +0.0f
 *   when d = 0; [3] d.  It is the last block of the packed buffer, 8-aligned behind every other block, 16 x the request's tokens
 *   bytes, present only when asked for, and leaves the device in the one copy.  To aim at a pitch in Hz: measure with neutral
 *   ratios, then set pitch = target / measured.
 *   Not offered: prosody together with the levelled, loudness and limited entries; semitone or Hz inputs; per-frame curves;
 *   silence inside a chunk (a join's pause does that between chunks); SSML parsing. */
#define KX_PROSODY_MAX_FRAMES 50
typedef struct kx_prosody {
    const float*   rate;    /* per token; durations are divided by it, like `speed`   */
    const int32_t* frames;  /* per token; 0 = as predicted, 1..50 = exactly that many */
    const float*   pitch;   /* per token; ratio applied to the F0 curve (1 = as is)   */
    const float*   energy;  /* per token; ratio applied to the N curve  (1 = as is)   */
} kx_prosody;
/* kx_infer with a kx_prosody (may be NULL) and the used durations: out_durations [B, t_stride] int32, entries t < lens[b] written,
 * may be NULL. */
int kx_infer_prosody(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B, const float* styles,
                     const float* speeds, int n_speed, uint64_t seed, uint32_t flags, float** out, int64_t* out_lens,
                     const kx_prosody* prosody, int32_t* out_durations);
/* kx_infer_requests_joined with a kx_prosody (may be NULL) for the call's rows and the report.  `joins` may be NULL with
 * n_join == 0 (no joins).  out_report and out_n_report are both NULL (no report) or both set, else "infer: null report argument":
 * *out_report points INTO *out as *out_marks does (never freed on its own), the requests' tokens back to back, and
 * out_n_report[r] = the tokens of request r (the sum of its chunks' lens). */
int kx_infer_requests_prosody(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B,
                              const int32_t* chunks_per_request, int R, const float* styles, const int32_t* voice_ids,
                              const float* weights, int max_mix, const float* speeds, int n_speed, uint64_t seed, uint32_t flags,
                              const int32_t* formats, int n_format, void** out, int64_t* out_bytes, int64_t* out_samples,
                              int64_t** out_marks, int64_t* out_n_marks, const kx_join* joins, int n_join, const kx_prosody* prosody,
                              float** out_report, int64_t* out_n_report);

/* ---- fit: spans of a request's tokens made to last exactly so many frames ----------------------------------------------------
 * The `duration` attribute of SSML's <prosody>: "this sentence takes exactly 2.4 s".  A frame is 600 samples at 24 000 Hz, 25 ms
 * (Python: voices.fit_frames(seconds)).  A call carries n_spans spans, sorted by (request, begin) and disjoint; tokens
 * [begin, end) of request `request` -- positions count the request's tokens with its chunks laid end to end, the two pad tokens of
 * every chunk included -- get durations that add up to exactly `frames`.  A span may cross chunk boundaries; one span over all
 * tokens fits the whole request.  For each span the GPU finds the one rate that does it (numpy twin: voices.fit_durations):
 *   Weights.  Token t of row b has the float32 value s after steps (1) to (3) of "prosody" above (the sum of 50 sigmoids, / speed_b,
 *   / rate[t] when given), before rintf.  w = s where 2^-20 <= s <= 2^20; below that 2^-20, above it 2^20, and a NaN gives 1.0f.
 *   Held tokens.  A token whose prosody frames[t] >= 1 is held: it keeps that count and is no part of the fit.  Phi = the sum of
 *   the held counts inside the span, n = its free tokens, G = frames - Phi = what the free tokens must add up to.
 *   The fit.  For a float32 lambda > 0: d_t(lambda) = min(max(rintf(f32(w_t * lambda)), 1), 50) (one float32 multiply; an infinite
 *   product gives 50) and F(lambda) = the sum of d_t(lambda) over the free tokens.  F is non-decreasing in lambda read as its bit
 *   pattern.  Bisection over the patterns u in 0x00800000 .. 0x7F7FFFFF: while lo < hi, mid = lo + (hi - lo) / 2; F(mid) >= G ?
 *   hi = mid : lo = mid + 1 (31 steps at most).  lambda = the float of lo, lambda- = the float of lo - 1, E = F(lambda) - G >= 0
 *   the excess.  Between adjacent floats no d_t moves by more than 1 (DESIGN.md section 7 "Fit"), so at least E tokens have
 *   d_t(lambda) = d_t(lambda-) + 1: the steppers.  Of them, the E with the highest token position keep d_t(lambda-); every other
 *   free token gets d_t(lambda).  At lo = 0x00800000, E is 0.  The sum is G exactly.
 *   The fitted counts are fixed frame counts as in step (6) of "prosody": marks, joins and the prosody report follow them.
 *   A fit at the natural total need not reproduce the un-fitted durations token for token: every d_t of the span goes through one
 *   common lambda and the tie rule, and lambda = 1 is only one of the patterns the bisection may end on.
 *   The fit counts the model's frames.  A join that trims pads afterwards shortens the body as it always does: fit, then join.
 *   Refusals, on the host before any device work, KX_ERR_INVALID "infer: bad fit" (dispatcher: "dispatcher_submit_request: bad
 *   fit"): spans unsorted or overlapping; `request` outside 0..R-1; begin >= end or end past the request's tokens; n = 0; G < n or
 *   G > 50 n; a null span array with n_spans != 0.  A model with a pinned duration pattern (kx_set_pinned_durations) refuses a call
 *   that has spans: "infer: fit with pinned durations".  n_spans == 0 is the prosody call bit for bit.  Alignment rows hold 50
 *   frames per token of the longest row; a fitted token has at most 50, so a span adds no overflow path.
 *   Under KX_FLAG_TAPS, "pred.dur.weights" holds w [B,1,512] and "pred.dur.fitted" the fixed counts the duration kernel took (int32
 *   bits in the float32 tap): the caller's, the fitted ones, 0 for a token nothing fixes.
 *   Not offered: fit together with the levelled, loudness and limited entries; targets in samples or at the output rate; fitting the
 *   stream after a join's trims; silence inside a chunk; SSML parsing. */
typedef struct kx_fit_span {
    int32_t request;  /* 0 .. R-1 */
    int32_t begin;    /* first token of the span, counted over the request's chunks laid end to end */
    int32_t end;      /* one past its last token */
    int32_t frames;   /* what its durations add up to: 25 ms each */
} kx_fit_span;
typedef struct kx_fit_result {
    float   lambda;       /* the factor the GPU chose for the span's weights; 1 / lambda is speed-like */
    int32_t n_free;       /* n: tokens the fit set */
    int32_t held_frames;  /* Phi */
    int32_t excess;       /* E */
} kx_fit_result;
/* kx_infer_requests_prosody with spans; out_fit [n_spans] may be NULL.  `joins`, `prosody` and the report pair as there. */
int kx_infer_requests_fitted(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B,
                             const int32_t* chunks_per_request, int R, const float* styles, const int32_t* voice_ids,
                             const float* weights, int max_mix, const float* speeds, int n_speed, uint64_t seed, uint32_t flags,
                             const int32_t* formats, int n_format, void** out, int64_t* out_bytes, int64_t* out_samples,
                             int64_t** out_marks, int64_t* out_n_marks, const kx_join* joins, int n_join, const kx_prosody* prosody,
                             float** out_report, int64_t* out_n_report, const kx_fit_span* spans, int n_spans, kx_fit_result* out_fit);

/* ---- pieces: a request delivered in several calls whose payloads join byte for byte ---------------------------------------------
 * A request's body is complete only when all its chunks have been through the forward.  A *piece* is a run of consecutive chunks
 * of a request, submitted as one request of a call, with a flag word and a carry record; the caller sends the chunks it has, gets
 * the bytes that are final, and hands the carry it got back to the next piece.  The invariant:
 *
 *     the payloads of a request's pieces, laid end to end, ARE the body of the same request run whole -- every byte -- and
 *     their marks are its marks.
 *
 * KX_PIECE_FIRST marks the first piece of a request, KX_PIECE_LAST the last; a request run whole is the single piece with both
 * flags, and is planned and launched exactly as through kx_infer_requests_levelled (its carry-out is all zeros).
 *
 * Let x[0..A) be the whole request's stream at 24 000 Hz after the join, y[0..N) that stream at the output rate after the
 * resampler and the gain, A_k the joined source samples of pieces 0..k, and (L, M, C) the rate's filter of 2 C + 1 taps
 * (kx_resample_filter).  Output n is *final* once its window lies inside the data, n M + C <= A_k L - 1:
 *     F_k = clamp(floor((A_k L - 1 - C) / M) + 1, 0, N)      final outputs after piece k
 *     E_k = 4 floor(F_k / 4)                                  emitted after piece k (every region stays a multiple of 4 bytes)
 * with E_k = A_k at rate code 0 and E_k = N for the last piece.  Piece k's payload is the bytes of samples [E_{k-1}, E_k) in the
 * request's form, behind the form's header in the FIRST piece only; out_samples is E_k - E_{k-1}.  It may be 0, and a piece of 0
 * bytes is a good result.  The accumulation of every output is the whole request's: float64 from +0, j ascending over the terms
 * that exist (no source sample before x[0] and none at or past A), one rounding -- the same bits.
 *
 * Joins: a piece's rows get the join rows they have in the whole request.  Head rules apply only under KX_PIECE_FIRST, tail rules
 * only under KX_PIECE_LAST; a piece that is not last keeps the pause behind its final chunk; every boundary between pieces is an
 * inner boundary.  Marks are the whole request's ("joins"), positions in the whole body's sample stream, their base from the carry.
 *
 * A piece may ask for forms 0, 1, 2, 3, 8 and 9, any rate, any join spec, marks, and a level of mode KX_LEVEL_GAIN (a product per
 * sample; the p it reports is the piece's).  What needs the whole body before the first byte is refused with KX_ERR_INVALID before
 * any device work, "infer: a piece cannot carry <noun>": `a measured level` (modes NORMALIZE and CEILING, KX_PEAK_TRUE), `loudness`,
 * `a limiter`, `a sized form` (4, 12, 17 and 18: their headers hold sizes).  Prosody and fit spans are per call.  Out of scope:
 * ADPCM and FLAC pieces (block and frame alignment need a larger hold-back, STREAMINFO holds totals), a streaming limiter or
 * loudness, MP3, text segmentation.
 *
 * The carry is a POD the caller owns, one per request in and one out.  `tail` holds the last n_tail = min(KX_PIECE_TAIL, A_k)
 * samples of the joined 24 000 Hz stream so far (n_tail = 0 at rate code 0) and zeros behind them: every source sample an output
 * not yet emitted reads -- at most (2 C + 3 M) / L = 153 of them, at 8000 Hz.  The GPU writes the carry-out into a block of its own
 * behind every other block of the packed buffer, so body, marks and carry leave the device in one copy.  A FIRST piece ignores its
 * carry-in.  Any other piece is refused with "infer: bad piece carry" when its carry has another magic, a format word other than
 * the piece's, or fields that do not belong together (n_tail, out_samples = E of src_samples, src_samples a multiple of 24).  The
 * model keeps no state between calls and the dispatcher none between submissions. */
#define KX_PIECE_FIRST 1u
#define KX_PIECE_LAST  2u
#define KX_PIECE_TAIL  256
#define KX_PIECE_MAGIC 0x4350584Bu
typedef struct kx_piece_carry {
    uint32_t magic;        /* KX_PIECE_MAGIC */
    uint32_t format_word;  /* the request's format word */
    int64_t src_samples;   /* A_k */
    int64_t out_samples;   /* E_k */
    int32_t n_tail;
    int32_t reserved;      /* chunks of the pieces so far (the dispatcher numbers a later piece's rows from it) */
    float tail[KX_PIECE_TAIL];
} kx_piece_carry;   /* 1056 bytes */
/* kx_infer_requests_levelled with pieces: piece_flags [R], carry_in [R] (entry r is read unless request r has KX_PIECE_FIRST; may
 * be NULL when none is read), carry_out [R].  `levels` may be NULL with n_level == 0 here (no levels), `joins` with n_join == 0.
 * Refused after everything kx_infer_requests_levelled refuses: a null piece_flags or carry_out ("infer: null piece argument"), a
 * flag word with a bit beyond the two ("infer: bad piece flags"; 0 is a piece that is neither the first nor the last), and the refusals above. */
int kx_infer_requests_pieces(kx_model* m, const int64_t* ids, int64_t t_stride, const int32_t* lens, int B,
                             const int32_t* chunks_per_request, int R, const float* styles, const int32_t* voice_ids,
                             const float* weights, int max_mix, const float* speeds, int n_speed, uint64_t seed, uint32_t flags,
                             const int32_t* formats, int n_format, void** out, int64_t* out_bytes, int64_t* out_samples,
                             int64_t** out_marks, int64_t* out_n_marks, const kx_join* joins, int n_join, const kx_level* levels,
                             int n_level, double* out_levels, const uint32_t* piece_flags, const kx_piece_carry* carry_in,
                             kx_piece_carry* carry_out);

/* ---- request dispatcher ----------------------------------------------------
 * Replaces the reference's one-request-at-a-time `Mutex<Session>` (kokorox/src/onn/ort_koko.rs:78; callers
 * kokorox-openai/src/lib.rs:370-439, kokorox-websocket/src/lib.rs:657-668).  Any number of threads submit
 * single utterances; two workers per model (= per GPU; one runs a forward while the other hands the previous batch's results
 * to its clients) coalesce whatever is queued — up to max_batch, waiting at most max_wait_us after the first arrival — into
 * one batched forward.  A request's waveform depends only on (ids, style, speed, seed), not on what it was batched with, nor
 * on which model ran it, nor on which LSTM recurrence that model was running (kx_model_status: both forms give the same bits).
 * A request is checked completely when it is submitted (token ids against the models' embedding tables, token count, speed,
 * format, voice ids against the smallest voice table among the models, mix size) and refused there with KX_ERR_INVALID: a bad
 * request never reaches a batch.  If a batch still fails as a whole, an INVALID-class failure is re-run request by request
 * (only the requests that fail alone report it); a DEVICE-class failure is retried once as a batch, and if it fails again
 * that MODEL is marked failed: it takes no more work and its batch goes back to the head of the queue for the healthy models
 * (kx_dispatcher_health).  Requests report KX_ERR_DEVICE only when no healthy model is left.
 * Results (*out of the submit calls) are NOT malloc'd memory: they point into a page-locked buffer shared by the requests of
 * one batch, which returns to the library's pool when the last of them has been released.  Release them with kx_free_audio /
 * kx_free_packed and with nothing else (free() corrupts the heap); a result that is kept alive keeps its batch's buffer alive. */
typedef struct kx_dispatcher kx_dispatcher;
kx_dispatcher* kx_dispatcher_create(kx_model** models, int n_models, int max_batch, int max_wait_us, char* err,
                                    size_t err_len);
/* The same, after one discarded forward of max_batch utterances x warm_tokens tokens at warm_frames_per_token frames per token
 * on every model (kx_warmup, the models side by side): what a server should call, so that no request ever pays for an arena
 * growing (a stream sync + hipFree + hipMalloc of gigabytes: a 1.3 s outlier in the round-4 soak). */
kx_dispatcher* kx_dispatcher_create_warm(kx_model** models, int n_models, int max_batch, int max_wait_us, int warm_tokens,
                                         int warm_frames_per_token, char* err, size_t err_len);
/* Blocking; thread-safe.  ids = n_tokens ids incl. the two 0 pads; style = 256 floats.  *out: release with kx_free_audio
 * only (see above).  Equals kx_infer(B = 1, same seed, utterance base 0) bit for bit. */
int kx_dispatcher_submit(kx_dispatcher* d, const int64_t* ids, int n_tokens, const float* style, float speed,
                         uint64_t seed, float** out, int64_t* out_len, char* err, size_t err_len);
/* The request as the reference's servers make it (kokorox-openai/src/lib.rs:370-439, kokorox-websocket/src/lib.rs:
 * 657-736): the voice is EITHER the 256-float style row (`style`, voice_ids = NULL) OR names into the device voice
 * table every model of the dispatcher holds (kx_set_voice_table): `voice_ids[n_mix]` with `weights` = NULL and
 * n_mix = 1 for a single voice (row copy), or with `weights[n_mix]` for a mix "a.4+b.5" (sum_k row_k * (w_k * 0.1),
 * koko.rs:1255-1306; ids < 0 are skipped); `format` is a KX_PACK_* output form.  *out = the packed bytes (release with
 * kx_free_audio / kx_free_packed only); requests of every kind and format share batches, and a request's bytes equal those of
 * kx_infer_voices / kx_infer_packed (B = 1, same seed, utterance base 0) whatever it was batched with.
 * Errors are per request: when a batch fails as a whole its requests are re-run one by one. */
int kx_dispatcher_submit_ex(kx_dispatcher* d, const int64_t* ids, int n_tokens, const float* style,
                            const int32_t* voice_ids, const float* weights, int n_mix, float speed, uint64_t seed,
                            int format, void** out, int64_t* out_bytes, int64_t* out_samples, char* err, size_t err_len);
/* A request of 1 .. max_batch chunks (the chunk loop of koko.rs:947-1191 as one submit): `ids` holds the chunks back to back,
 * chunk c has chunk_tokens[c] ids incl. its own two 0 pads; `styles` = n_chunks rows of 256 floats, or NULL with ONE voice
 * spec for the request as in kx_dispatcher_submit_ex (the row of the voice is chunk_tokens[c] - 2 per chunk); `format` is a
 * format word (a KX_PACK_* form, optionally | KX_PACK_RATE_*).  Checked completely at submit with the rules of kx_dispatcher_submit_ex per chunk.  The chunks run as
 * rows of ONE batched forward (a request is never split over batches or models; batches are sized in rows), chunk c draws
 * the noise stream (seed, c), and *out is the request's one region: header of the form, if any, then the chunks' samples in
 * order.  The bytes equal kx_infer_requests (R = 1, same seed, utterance base 0) whatever the request was batched with and
 * on whichever model.  Release *out with kx_free_packed / kx_free_audio only. */
int kx_dispatcher_submit_request(kx_dispatcher* d, const int64_t* ids, const int32_t* chunk_tokens, int n_chunks,
                                 const float* styles, const int32_t* voice_ids, const float* weights, int n_mix,
                                 float speed, uint64_t seed, int format, void** out, int64_t* out_bytes,
                                 int64_t* out_samples, char* err, size_t err_len);
/* kx_dispatcher_submit_request with the request's token marks (see "token marks" above): *out_marks points INTO the allocation
 * of *out, 8-byte aligned behind the body, *out_n_marks values = the sum over the chunks of chunk_tokens[c] + 1; it is never
 * freed on its own and lives until *out is released (kx_free_packed / kx_free_audio).  Body and marks equal those of
 * kx_infer_requests_marks (R = 1, same seed, utterance base 0) whatever the request was batched with -- requests with and
 * without marks share batches -- on whichever model and recurrence form.  A null out_marks or out_n_marks: KX_ERR_INVALID
 * "dispatcher_submit_request: null marks argument"; every other refusal as kx_dispatcher_submit_request. */
int kx_dispatcher_submit_request_marks(kx_dispatcher* d, const int64_t* ids, const int32_t* chunk_tokens, int n_chunks,
                                       const float* styles, const int32_t* voice_ids, const float* weights, int n_mix,
                                       float speed, uint64_t seed, int format, void** out, int64_t* out_bytes,
                                       int64_t* out_samples, int64_t** out_marks, int64_t* out_n_marks, char* err,
                                       size_t err_len);
/* kx_dispatcher_submit_request_marks with the request's join spec (see "joins" above; one request, one spec).  out_marks and
 * out_n_marks are both NULL (no marks) or both set, else "dispatcher_submit_request: null marks argument"; a null `join`, a
 * stray flag bit or a field outside its range: "dispatcher_submit_request: bad join".  Joined and plain requests, with and
 * without marks, share batches; body and marks equal those of kx_infer_requests_joined (R = 1, same seed, utterance base 0)
 * whatever the request was batched with. */
int kx_dispatcher_submit_request_joined(kx_dispatcher* d, const int64_t* ids, const int32_t* chunk_tokens, int n_chunks,
                                        const float* styles, const int32_t* voice_ids, const float* weights, int n_mix,
                                        float speed, uint64_t seed, int format, void** out, int64_t* out_bytes,
                                        int64_t* out_samples, int64_t** out_marks, int64_t* out_n_marks, const kx_join* join,
                                        char* err, size_t err_len);
/* kx_dispatcher_submit_request_joined with the request's level spec (see "levels" above); `join` may be NULL here (no join).
 * out_level may be NULL; when given it receives two doubles, f64(p) and g of the request.  A null or invalid `level`:
 * "dispatcher_submit_request: bad level"; every other refusal as kx_dispatcher_submit_request_joined.  Levelled, joined and
 * plain requests, with and without marks, share batches; body, marks and levels equal those of kx_infer_requests_levelled
 * (R = 1, same seed, utterance base 0) whatever the request was batched with. */
int kx_dispatcher_submit_request_levelled(kx_dispatcher* d, const int64_t* ids, const int32_t* chunk_tokens, int n_chunks,
                                          const float* styles, const int32_t* voice_ids, const float* weights, int n_mix,
                                          float speed, uint64_t seed, int format, void** out, int64_t* out_bytes,
                                          int64_t* out_samples, int64_t** out_marks, int64_t* out_n_marks, const kx_join* join,
                                          const kx_level* level, double* out_level, char* err, size_t err_len);
/* kx_dispatcher_submit_request_levelled as a piece of a request (see "pieces" above): piece_flags = KX_PIECE_FIRST and / or
 * KX_PIECE_LAST, carry_in the record the piece before left (NULL with KX_PIECE_FIRST), carry_out where this one's goes.  `join` and
 * `level` may both be NULL here.  The rows of a later piece draw the noise they draw in the request run whole (the carry counts the
 * chunks so far).  Refusals as kx_infer_requests_pieces names them, under "dispatcher_submit_request: " ("... a piece cannot carry a
 * sized form", "... bad piece carry", "... bad piece flags", "... null piece argument").  Pieces of different requests, and pieces
 * beside whole requests of every kind, share batches; payload, marks and carry equal those of kx_infer_requests_pieces whatever
 * the piece was batched with. */
int kx_dispatcher_submit_request_piece(kx_dispatcher* d, const int64_t* ids, const int32_t* chunk_tokens, int n_chunks,
                                       const float* styles, const int32_t* voice_ids, const float* weights, int n_mix, float speed,
                                       uint64_t seed, int format, void** out, int64_t* out_bytes, int64_t* out_samples,
                                       int64_t** out_marks, int64_t* out_n_marks, const kx_join* join, const kx_level* level,
                                       double* out_level, uint32_t piece_flags, const kx_piece_carry* carry_in,
                                       kx_piece_carry* carry_out, char* err, size_t err_len);
/* kx_dispatcher_submit_request_joined with the request's loudness spec (see "loudness" above); `join` may be NULL here (no
 * join).  out_loudness may be NULL; when given it receives four doubles, f64(p), g, I and n_g of the request.  A null or invalid
 * `loudness`: "dispatcher_submit_request: bad loudness"; every other refusal as kx_dispatcher_submit_request_joined.  Loudness,
 * levelled, joined and plain requests share batches; body, marks and the four values equal those of kx_infer_requests_loudness
 * (R = 1, same seed, utterance base 0) bit for bit, whatever the request was batched with. */
int kx_dispatcher_submit_request_loudness(kx_dispatcher* d, const int64_t* ids, const int32_t* chunk_tokens, int n_chunks,
                                          const float* styles, const int32_t* voice_ids, const float* weights, int n_mix,
                                          float speed, uint64_t seed, int format, void** out, int64_t* out_bytes,
                                          int64_t* out_samples, int64_t** out_marks, int64_t* out_n_marks, const kx_join* join,
                                          const kx_loudness* loudness, double* out_loudness, char* err, size_t err_len);
/* kx_dispatcher_submit_request_joined with the request's limit spec (see "limiter" above); `join` may be NULL here (no join).
 * out_limit may be NULL; when given it receives five doubles, f64(p), g, I, n_g and r of the request.  A null or invalid `limit`:
 * "dispatcher_submit_request: bad limit"; every other refusal as kx_dispatcher_submit_request_joined.  Limited, loudness, levelled,
 * joined and plain requests share batches; body, marks and the five values equal those of kx_infer_requests_limited (R = 1, same
 * seed, utterance base 0) bit for bit, whatever the request was batched with. */
int kx_dispatcher_submit_request_limited(kx_dispatcher* d, const int64_t* ids, const int32_t* chunk_tokens, int n_chunks,
                                         const float* styles, const int32_t* voice_ids, const float* weights, int n_mix,
                                         float speed, uint64_t seed, int format, void** out, int64_t* out_bytes,
                                         int64_t* out_samples, int64_t** out_marks, int64_t* out_n_marks, const kx_join* join,
                                         const kx_limit* limit, double* out_limit, char* err, size_t err_len);
/* kx_dispatcher_submit_request_joined with the request's prosody (see "prosody" above) and its report; `join` may be NULL here
 * (no join).  The arrays of `prosody` that are not NULL hold the chunks' values back to back, as `ids` does; a NULL `prosody` is
 * the neutral one.  out_report and out_n_report are both NULL (no report) or both set, else
 * "dispatcher_submit_request: null report argument"; *out_report points INTO the allocation of *out, as *out_marks does, and
 * *out_n_report = the request's tokens.  A value outside its range: "dispatcher_submit_request: bad prosody".  Prosody and plain requests share batches; a request's bytes,
 * marks and report equal those of kx_infer_requests_prosody (R = 1, same seed, utterance base 0) whatever it was batched with. */
int kx_dispatcher_submit_request_prosody(kx_dispatcher* d, const int64_t* ids, const int32_t* chunk_tokens, int n_chunks,
                                         const float* styles, const int32_t* voice_ids, const float* weights, int n_mix,
                                         float speed, uint64_t seed, int format, void** out, int64_t* out_bytes,
                                         int64_t* out_samples, int64_t** out_marks, int64_t* out_n_marks, const kx_join* join,
                                         const kx_prosody* prosody, float** out_report, int64_t* out_n_report, char* err,
                                         size_t err_len);
/* kx_dispatcher_submit_request_prosody with the request's fit spans (see "fit" above): `request` of every span must be 0, positions
 * count the request's tokens, chunks back to back; out_fit [n_spans] may be NULL.  A refusal of "fit":
 * "dispatcher_submit_request: bad fit".  Fitted and plain requests share batches; a request's bytes, marks, report and fit results
 * equal those of kx_infer_requests_fitted (R = 1, same seed, utterance base 0) whatever it was batched with. */
int kx_dispatcher_submit_request_fitted(kx_dispatcher* d, const int64_t* ids, const int32_t* chunk_tokens, int n_chunks,
                                        const float* styles, const int32_t* voice_ids, const float* weights, int n_mix,
                                        float speed, uint64_t seed, int format, void** out, int64_t* out_bytes,
                                        int64_t* out_samples, int64_t** out_marks, int64_t* out_n_marks, const kx_join* join,
                                        const kx_prosody* prosody, float** out_report, int64_t* out_n_report,
                                        const kx_fit_span* spans, int n_spans, kx_fit_result* out_fit, char* err, size_t err_len);
/* n_requests counts requests, max_batch_seen the largest batch in ROWS (a request of n chunks is n rows). */
int kx_dispatcher_stats(kx_dispatcher* d, int64_t* n_requests, int64_t* n_batches, int64_t* max_batch_seen);
/* batches each model (worker) has run so far: per_model[n_models] */
int kx_dispatcher_model_batches(kx_dispatcher* d, int64_t* per_model, int n_models);
/* What went wrong so far: requests that were re-run one by one after their batch failed with an INVALID-class error, and
 * batches that were run a second time after a DEVICE-class failure.  Both stay 0 in a healthy deployment. */
int kx_dispatcher_failures(kx_dispatcher* d, int64_t* n_replayed, int64_t* n_retried);
/* Per-model health: healthy[i] = 1 while model i takes work, 0 once a batch failed on it with KX_ERR_DEVICE twice in a row (it
 * is then out for the dispatcher's lifetime: destroy the dispatcher and the model to recover the GPU); *n_model_failures =
 * models marked failed so far, *n_requeued = requests that went back to the queue for another model (either may be NULL). */
int kx_dispatcher_health(kx_dispatcher* d, int32_t* healthy, int n_models, int64_t* n_model_failures, int64_t* n_requeued);
void kx_dispatcher_destroy(kx_dispatcher* d);  /* waits for queued requests; models stay alive */

/* ---- debugging ---------------------------------------------------------------------
 * (the stand-alone kernel hooks of tests/ are NOT part of this library: include/kokorox_hip_test.h, libkokorox_hip_test.so) */

/* Named intermediate of the last kx_infer*(…, KX_FLAG_TAPS): utterance b's [C, L] slab
 * is copied to out (row-major, rows = channels).  Query with out = NULL to get C and L. */
int kx_debug_tap(kx_model* m, const char* name, int b, float* out, int64_t out_cap,
                 int32_t* C, int32_t* L);

const char* kx_version(void);

#ifdef __cplusplus
}
#endif
#endif /* KOKOROX_HIP_H */
