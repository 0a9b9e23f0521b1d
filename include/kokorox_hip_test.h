/* Test hooks of libkokorox_hip (tests/ only): stand-alone runs of single kernels on host arrays and two process-wide test
 * switches.  They live in a library of their own, libkokorox_hip_test.so (kokorox_amd/csrc/test_hooks_*.hip, one unit per job: conv
 * launches, the token-axis front half, the back half's other kernels, the output stage), which links against libkokorox_hip.so; the
 * production library exports none of them. */
#ifndef KOKOROX_HIP_TEST_H
#define KOKOROX_HIP_TEST_H
#include "kokorox_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* One conv launch as the model assembles it (conv_call.hip: the model's packers, plan and kernel arguments), on host arrays.
 * Fields that are left 0 / NULL are off; out_mul and out_div must be set (1 = off).  Every ragged call (lens given): the hook writes
 * NaN into every input and residual column at or past an utterance's own length; what the caller has there is not uploaded.  A
 * STRICT call -- one with stride != 1, a length map, up_off or view -- also gets -12345.5 back in every output column the utterance
 * does not own (other calls: 0, or the running sum), and has 64 guard bytes behind x, y, resid and the partial-sum table checked
 * (KX_ERR_STATE).  Contradictory fields are KX_ERR_INVALID before any launch. */
typedef struct kx_test_conv_args {
    uint32_t struct_size;   /* sizeof(kx_test_conv_args): any other value is KX_ERR_INVALID, before the device is looked at */
    int32_t device_id;
    const float* x;         /* [B,Cin,L] */
    const float* w;         /* [Cout,Cin,k]; up_stride > 0: [Cin,Cout,k] */
    const float* bias;      /* [Cout] or NULL */
    const float* alpha;     /* [Cin], act = 2 */
    const float* norm;      /* [3,B,Cin] (mean, scale, shift): the fused AdaIN affine on the input, or NULL */
    const float* resid;     /* [B,Cout,Lout + up_off], added in the store, or NULL */
    const int32_t* lens;    /* [B]: a RAGGED batch, utterance b is lens[b] columns long (columns past its output length stay as they
                             * were, its statistics cover its own columns only); with a length map, lens[b] units.  NULL = all L */
    float* y;               /* [B,Cout,Lout + up_off], tmajor: [B,Lout,Cout].  Lout = ((in_up2 ? 2 L : L) + 2 pad - dil (k-1) - 1) /
                             * stride + 1, up_stride = s > 0: (L-1) s - 2 pad + k.  Read as the running sum when accumulate != 0 */
    int64_t y_floats;       /* floats the caller allocated for y: fewer than the stored shape is KX_ERR_INVALID */
    float* stats_out;       /* [B,Cout,2] or NULL: the fused InstanceNorm partial sums (sum, sum of squares of each stored row; a
                             * ragged row: the slots of its own output columns) */
    const float* norm_gb;   /* [B,2 Cout] (gamma | beta), with norm_out: the conv's own partial sums go through launch_stats_finalize */
    float* norm_out;        /* ... and come back as the next conv's [3,B,Cout] (mean, scale, shift) planes */
    int64_t* plan_out;      /* [17] or NULL: the kx::ConvPlan that was launched, fields as in kx_test_conv_plan */
    int32_t B, Cin, L, Cout, k;
    int32_t stride;         /* >= 1, plain convs; a strided conv is refused a merged, in_up2 or time-major launch */
    int32_t pad, dil;
    int32_t up_stride;      /* s > 0: the polyphase transposed conv of the generator's upsamplers (needs k = 2 s, pad = (k - s) / 2,
                             * dil = 1, stride = 1); ragged only with a length map */
    int32_t act;            /* on the input: 0 none, 1 leaky(slope), 2 snake(alpha) */
    float slope;
    int32_t accumulate;     /* y = (conv + bias + resid [+ y]) * out_mul / out_div */
    float out_mul, out_div;
    int32_t mode;           /* as in kx_set_conv_mode, plus 2 = f16x3 on the LDS-DMA kernel forms only (conv_f16x3.hip: what the
                             * direct-A kernels are compared with bit for bit) and 3 = f16x3 through the direct-A kernel whatever the
                             * grid; + 0x100 (modes 1 and 3) = the input staged through a pre-split image (conv_f16x3_pre.hip) whatever
                             * the row count; + 0x200 = f16f8 (the layer carries the 8-bit cross image of its weights); + 0x400 = the
                             * direct-A conv's 256-column tile with the 4 x 1 wave layout too; + 0x800 = no 16x16x32 form */
    int32_t pad_ld;         /* rows padded to a multiple of 32 floats as the model lays them out: input and residual padding is NaN,
                             * the output padding [Lout + up_off, y_ld) holds a sentinel that must survive (KX_ERR_STATE) */
    int32_t flat;           /* the flat list of live tiles the model hands the direct-A kernels on a batch of more than one utterance */
    int32_t in_up2;         /* the conv reads x[p >> 1]: x stands for 2 L columns, lens[] are stored lengths */
    int32_t epi;            /* kx::ConvEpi: 1 = gelu_new */
    int32_t merged;         /* offer the plan ConvLaunch::merge_T = L, as the model does for every conv whose input and output share
                             * one plain length array; the plan decides */
    int32_t tmajor;         /* ST_TMAJOR; with pad_ld its rows of Cout values end in a checked margin */
    int32_t prec1;          /* 1 / 2 = one f16 / bf16 MFMA per product, 2 on the bf16 weight image of Model::set_conv_mode */
    int32_t act_shift;      /* x_prescale = 2^act_shift, w_unscale its inverse, as kx_set_act_prescale sets them */
    int32_t epi_stream;     /* ConvArgs::epi_stream */
    int32_t len_mul_in, len_add_in, len_mul_out, len_add_out;
                            /* len_mul_in > 0: lens[b] are UNITS (the model's frames); utterance b stores lens[b] len_mul_in +
                             * len_add_in input columns (<= L) and owns lens[b] len_mul_out + len_add_out output columns, and in.len,
                             * out.len and up_len are those LenMaps over one device array, as in Model::back_half.  The output count
                             * must be the conv's own on the input count.  len_mul_in = 0 keeps {lens, 1, 0} in and {lens, 1 or 2,
                             * Lout - L} out (stride 1, plain convs only) */
    int32_t up_off;         /* with up_stride: the output starts at column 1 of y and column 0 is its reflection
                             * (ReflectionPad1d((1, 0)), the last upsampler) */
    int32_t view;           /* x and resid each sit 3 rows below the top of a tensor 8 rows taller than they are, y likewise, and the
                             * batch strides are those of the taller tensors; the foreign input and residual rows hold NaN, the
                             * foreign output rows the sentinel, and a changed one is KX_ERR_STATE */
} kx_test_conv_args;

int kx_test_conv(const kx_test_conv_args* args, char* err, size_t err_len);

/* Stand-alone channel layer norm (launch_layernorm_ch) of x [B,C,T] over C, on rows padded to 32 floats (input padding NaN, output
 * padding checked): mode 0 plain, 1 affine (g, be [C]), 2 adaptive ((1 + g) xhat + be, g, be [B,C]); leaky != 0: leaky ReLU on the
 * result.  y [B,C,T]: columns >= lens[b] come back as -12345.5 (never written). */
int kx_test_layernorm(int device_id, const float* x, int B, int C, int T, const int32_t* lens, float eps, int mode, const float* g,
                      const float* be, float leaky, float* y, char* err, size_t err_len);

/* Stand-alone InstanceNorm statistics of x [B,C,L] (padded rows, NaN padding), gb [B,2 C] (gamma | beta) -> out [3,3,B,C]:
 * (mean, scale = (1 + gamma) rstd, shift = beta) from launch_in_stats alone, from launch_in_stats that also leaves its raw sums, and
 * from those raw sums through launch_stats_finalize. */
int kx_test_instance_norm(int device_id, const float* x, int B, int C, int L, const int32_t* lens, const float* gb, float* out,
                          char* err, size_t err_len);

/* The launch plan of one conv (kokorox_amd/csrc/conv_plan.hip: kernel form, tile, statistics slots, flat tile list, pre-split
 * input), computed on the host without a device.  in[25] = the fields of kx::ConvLaunch in declaration order (mode, prec1, f8, BM,
 * rows, n_chunks16, K, dil, stride, pad, act, in_up2, store, accum, epi, norm, stats, image, merge_T, x_bs, x_ld, B, cols, cus,
 * force), out[17] = those of kx::ConvPlan (form, bm, act, kt, wm, wn, vt, pf, p1, bf, bn, cols, merged, pre, stat_cols,
 * stat_tiles, flat_bn). */
int kx_test_conv_plan(const int64_t* in, int n_in, int64_t* out, int n_out, char* err, size_t err_len);

/* Stand-alone bidirectional LSTM (hidden 256): x [B,L,n_in] -> y [B,L,512]. */
int kx_test_lstm(int device_id, const float* x, int B, int L, int n_in, const float* w_ih,
                 const float* w_hh, const float* b_ih, const float* b_hh, const float* w_ih_r,
                 const float* w_hh_r, const float* b_ih_r, const float* b_hh_r, float* y,
                 char* err, size_t err_len);

/* Stand-alone ALBERT self-attention (12 heads x 64): qkv [B][2304][T] (rows Q | K | V, head-major, time
 * contiguous) with per-utterance valid lengths -> ctx [B][768][T]; columns >= lens[b] are left untouched. */
int kx_test_attention(int device_id, const float* qkv, const int32_t* lens, int B, int T, float* ctx,
                      char* err, size_t err_len);

/* Stand-alone harmonic source: f0 [B, 2F] -> har_source [B, 600F] (bit-exact phase). */
int kx_test_source(int device_id, const float* f0, int B, int F2, const float* lin_w,
                   float lin_b, uint64_t seed, uint64_t utt_base, int noise_off, float* out,
                   char* err, size_t err_len);

/* The output stage of a call alone (include/kokorox_hip.h: the KX_PACK_* forms and rates, "token marks", "joins"): the packer,
 * the resampler and the marks kernel through build_output_plan and launch_output_plan, the planner and the launcher the model
 * runs, host arrays in, host bytes out.  audio [B, audio_ld] with row b valid for 600 frames[b] samples (whatever lies beyond
 * must not reach the result), or NULL for the marks alone (no audio is read, out may be NULL with out_cap 0).  The frame counts
 * are either given (frames [B]; dur and lens NULL, and then neither marks nor joins) or derived on the host from dur [B][512]
 * frames per token with row b valid for lens[b] entries (frames NULL): frames[b] = the sum of the row's valid durations, its
 * edge durations dur[b][0] and dur[b][lens[b] - 1].  Request r = chunks_per_request[r] consecutive rows (NULL: every row a
 * request of its own, R = B) in the format word formats[r] (a KX_PACK_* form, optionally | KX_PACK_RATE_*; [R]), shaped by
 * joins[r] ([R], NULL = rows appended as they are), with marks when want[r] != 0 ([R], NULL = none).  out receives the R bodies
 * back to back (out_cap bytes available), out_bytes[r] / out_samples[r] their sizes, out_marks the wanted requests' marks back
 * to back (marks_cap values available), out_n_marks[r] their counts (0 where not wanted). */
int kx_test_output_plan(int device_id, const float* audio, int B, int64_t audio_ld, const int32_t* frames, const int32_t* dur,
                        const int32_t* lens, const int32_t* chunks_per_request, int R, const int32_t* formats, const kx_join* joins,
                        const uint8_t* want, void* out, int64_t out_cap, int64_t* out_bytes, int64_t* out_samples,
                        int64_t* out_marks, int64_t marks_cap, int64_t* out_n_marks, char* err, size_t err_len);

/* kx_test_output_plan with levels (include/kokorox_hip.h, "levels"): levels [R] (one spec per request; needs audio), out_levels
 * [R][2] doubles = f64(p) and g of every request as request_gain_kernel stored them.  The order is resampler, peak, gain, packer,
 * marks, through launch_output_plan.  levels = NULL (then out_levels = NULL too) is kx_test_output_plan, which calls this. */
int kx_test_output_plan_levelled(int device_id, const float* audio, int B, int64_t audio_ld, const int32_t* frames, const int32_t* dur,
                                 const int32_t* lens, const int32_t* chunks_per_request, int R, const int32_t* formats,
                                 const kx_join* joins, const uint8_t* want, void* out, int64_t out_cap, int64_t* out_bytes,
                                 int64_t* out_samples, int64_t* out_marks, int64_t marks_cap, int64_t* out_n_marks,
                                 const kx_level* levels, double* out_levels, char* err, size_t err_len);

/* kx_test_output_plan_levelled with loudness (include/kokorox_hip.h, "loudness"): loudness [R] (one spec per request; needs audio;
 * mode 0xFFFFFFFF = that request is not metered, as a plain or levelled request beside metered ones in a batch -- a metered request's
 * level spec must be the plain one), out_loudness [R][4] doubles = f64(p), g, I and n_g of every request (I and n_g of a request
 * that is not metered are not written), out_hops [R][hops_cap] doubles whose first out_n_hops[r] entries in row r are the hop
 * energies e[k] request_loudness_kernel stored.  `levels` may be NULL here (then out_levels too).  The order is resampler, peak,
 * loudness, gain, packer, marks, through the same build_output_plan and launch_output_plan.  loudness = NULL (then the three
 * outputs NULL and hops_cap 0) is kx_test_output_plan_levelled, which calls this. */
int kx_test_output_plan_loudness(int device_id, const float* audio, int B, int64_t audio_ld, const int32_t* frames, const int32_t* dur,
                                 const int32_t* lens, const int32_t* chunks_per_request, int R, const int32_t* formats,
                                 const kx_join* joins, const uint8_t* want, void* out, int64_t out_cap, int64_t* out_bytes,
                                 int64_t* out_samples, int64_t* out_marks, int64_t marks_cap, int64_t* out_n_marks,
                                 const kx_level* levels, double* out_levels, const kx_loudness* loudness, double* out_loudness,
                                 double* out_hops, int64_t hops_cap, int64_t* out_n_hops, char* err, size_t err_len);

/* kx_test_output_plan_loudness with limits (include/kokorox_hip.h, "limiter"): limits [R] (one spec per request; needs audio; a spec
 * of mode 0xFFFFFFFF: that request has none, as a request beside limited ones in a dispatcher batch; a limited request's level spec
 * must be the plain one and its loudness spec, if loudness is given, of mode 0xFFFFFFFF), out_limits [R][5] doubles = f64(p), g, I,
 * n_g and r of every limited request (the rows of the others are left as they were).  `levels` and `loudness` may be NULL here
 * (then their outputs too).  The order is resampler, peak, loudness, true peak, gain, limiter, packer, marks, through the same
 * build_output_plan and launch_output_plan.  limits = NULL (then out_limits too): kx_test_output_plan_loudness. */
int kx_test_output_plan_limited(int device_id, const float* audio, int B, int64_t audio_ld, const int32_t* frames, const int32_t* dur,
                                const int32_t* lens, const int32_t* chunks_per_request, int R, const int32_t* formats,
                                const kx_join* joins, const uint8_t* want, void* out, int64_t out_cap, int64_t* out_bytes,
                                int64_t* out_samples, int64_t* out_marks, int64_t marks_cap, int64_t* out_n_marks,
                                const kx_level* levels, double* out_levels, const kx_loudness* loudness, double* out_loudness,
                                double* out_hops, int64_t hops_cap, int64_t* out_n_hops, const kx_limit* limits, double* out_limits,
                                char* err, size_t err_len);

/* The same with FLAC requests (form 12; include/kokorox_hip.h, "FLAC"): the limited hook, and out_lengths [R] = the lengths block as
 * the device wrote it, the true size of every region (may be NULL).  `out` needs room for every FLAC region at its bound,
 * 52 + 16 ceil(N / 4096) + 2 N bytes; on return the R bodies lie back to back by their true sizes, as kx_infer_requests hands them
 * out, out_bytes holds those sizes, and the bytes of `out` behind the last body are zero.  The encoder's frame slots, its two
 * per-frame tables and every byte of a region behind its body are poisoned before the launch and have a guard behind them; the hook
 * fails with KX_ERR_STATE where a guard or the slack of a region is not as it was filled.  Every pointer of the limited hook may be
 * NULL as there (limits = NULL: no request is limited); a batch without form 12 is kx_test_output_plan_limited, which calls this. */
int kx_test_output_plan_flac(int device_id, const float* audio, int B, int64_t audio_ld, const int32_t* frames, const int32_t* dur,
                             const int32_t* lens, const int32_t* chunks_per_request, int R, const int32_t* formats,
                             const kx_join* joins, const uint8_t* want, void* out, int64_t out_cap, int64_t* out_bytes,
                             int64_t* out_samples, int64_t* out_marks, int64_t marks_cap, int64_t* out_n_marks,
                             const kx_level* levels, double* out_levels, const kx_loudness* loudness, double* out_loudness,
                             double* out_hops, int64_t hops_cap, int64_t* out_n_hops, const kx_limit* limits, double* out_limits,
                             int64_t* out_lengths, char* err, size_t err_len);

/* The same with pieces (include/kokorox_hip.h, "pieces"): the levelled hook, `loudness` / out_loudness [R][4] as in the loudness hook
 * (may both be NULL; the hop energies are not handed out) for a metered request run whole beside the pieces, and piece_flags [R],
 * carry_in [R] (may be NULL when every piece has KX_PIECE_FIRST), carry_out [R] as kx_infer_requests_pieces takes them, host arrays
 * in and out, through build_output_plan and launch_output_plan.  The carry block sits behind a guard of its own and has one behind
 * it, as have the carried tails; the hook fails with KX_ERR_STATE where one is not as it was filled.  Needs audio. */
int kx_test_output_plan_pieces(int device_id, const float* audio, int B, int64_t audio_ld, const int32_t* frames, const int32_t* dur,
                               const int32_t* lens, const int32_t* chunks_per_request, int R, const int32_t* formats,
                               const kx_join* joins, const uint8_t* want, void* out, int64_t out_cap, int64_t* out_bytes,
                               int64_t* out_samples, int64_t* out_marks, int64_t marks_cap, int64_t* out_n_marks,
                               const kx_level* levels, double* out_levels, const kx_loudness* loudness, double* out_loudness,
                               const uint32_t* piece_flags, const kx_piece_carry* carry_in, kx_piece_carry* carry_out, char* err,
                               size_t err_len);

/* The token-axis kernels of Model::front_half, alone.  Common to these hooks: rows padded to a multiple of 32 floats as in the
 * model, NaN in every input column a kernel must not read, -12345.5 (0xA5 bytes in integer buffers) in every output location it
 * must not write; what the caller cannot see (row padding, guard regions behind a buffer) the hook checks itself after the launch
 * and fails with KX_ERR_STATE. */

/* kx_test_lstm on a RAGGED batch: x [B,L,n_in] with utterance b valid for lens[b] steps (the rest is never uploaded: NaN) -> y
 * [B,L,512], where columns >= lens[b] come back as -12345.5.  The input products start as NaN before the input GEMM (the f32
 * launch of kx_test_lstm, on the ragged lengths), so a recurrence that reads a step past an utterance's length poisons its output.
 * inplace = 1 (n_in = 640): the output is rows 0..511 of the 640-row input tensor itself, as Model::lstm is called for the duration
 * encoder; rows 512..639 must come back as they were.  repeat = n (1..16): n launches on ONE exchange buffer whose launch counter
 * starts at epoch0 (0..0xffff; 0xfffd with repeat = 4 crosses the 16-bit wrap and the clearing that goes with it), the output reset
 * between them; the last result is returned, and two launches that differ in a bit are KX_ERR_STATE.  kx_test_lstm_parts selects
 * the form. */
int kx_test_lstm_ragged(int device_id, const float* x, const int32_t* lens, int B, int L, int n_in, const float* w_ih,
                        const float* w_hh, const float* b_ih, const float* b_hh, const float* w_ih_r, const float* w_hh_r,
                        const float* b_ih_r, const float* b_hh_r, int inplace, int repeat, uint32_t epoch0, float* y, char* err,
                        size_t err_len);

/* Duration head and alignment: launch_duration on logits [B,50,T] (row b valid for lens[b] tokens), speeds [n_speed] (1 or B),
 * pinned [n_pinned] (0 = none; each 1..50) with rows of idx_ld frames (the model: 50 T), then launch_gather_cols of src [B,C,T]
 * over Fmax = max(frames).  Out: dur [B,512] (0xA5 bytes past lens[b]), frames [B], idx [B,idx_ld] (0xA5 bytes past frames[b]),
 * gathered [B,C,Fcap] (-12345.5 in columns >= frames[b]; Fcap >= Fmax), overflow = the sticky word of duration_kernel (0, or
 * b + 1 of the first row whose durations did not fit idx_ld).  A frame count or an index outside its row is KX_ERR_STATE, and the
 * gather is then not launched. */
int kx_test_alignment(int device_id, const float* logits, int B, int T, const int32_t* lens, const float* speeds, int n_speed,
                      const int32_t* pinned, int n_pinned, const float* src, int C, int idx_ld, int32_t* dur, int32_t* frames,
                      int32_t* idx, float* gathered, int Fcap, uint32_t* overflow, char* err, size_t err_len);

/* kx_test_alignment on launch_prosody_duration (include/kokorox_hip.h, "prosody"): rate [B,T] and fixed [B,T] per token (either may
 * be NULL, not both; entries at or past lens[b] are not read: they go up as NaN / 0xA5 bytes).  Everything else as kx_test_alignment. */
int kx_test_prosody_durations(int device_id, const float* logits, int B, int T, const int32_t* lens, const float* speeds, int n_speed,
                              const int32_t* pinned, int n_pinned, const float* rate, const int32_t* fixed, const float* src, int C,
                              int idx_ld, int32_t* dur, int32_t* frames, int32_t* idx, float* gathered, int Fcap, uint32_t* overflow,
                              char* err, size_t err_len);

/* kx_test_prosody_durations with the fit in front of it (include/kokorox_hip.h, "fit"): launch_fit_weights, launch_fit_spans, then
 * launch_prosody_duration on the fitted counts.  rate and fixed may both be NULL here; there is no pinned pattern.  spans [n_spans]
 * (n_spans >= 1) over the R requests of chunks_per_request (NULL: every row a request), checked by fit_ok ("test_fit_durations: bad
 * fit").  Out, beside kx_test_alignment's: w [B,512] and fitted [B,512] whole as the kernels left them (0 at and past lens[b]), and
 * results [n_spans].  The three start as sentinel / 0xA5 bytes with a guard behind each, checked here: KX_ERR_STATE. */
int kx_test_fit_durations(int device_id, const float* logits, int B, int T, const int32_t* lens, const float* speeds, int n_speed,
                          const float* rate, const int32_t* fixed, const int32_t* chunks_per_request, int R, const kx_fit_span* spans,
                          int n_spans, const float* src, int C, int idx_ld, int32_t* dur, int32_t* frames, int32_t* idx, float* gathered,
                          int Fcap, uint32_t* overflow, float* w, int32_t* fitted, kx_fit_result* results, char* err, size_t err_len);

/* launch_prosody_curves on curves [B,2,2 Fcap] (row 0 = F0, row 1 = N; row b valid for 2 frames[b] steps, 1 <= frames[b] <= Fcap),
 * idx [B,idx_ld] (entries f < frames[b] in 0 .. lens[b] - 1), dur [B,T] (sum over t < lens[b] = frames[b]) and the per-token ratios
 * pitch / energy [B,T] (either may be NULL).  Out: shaped [B,2,2 Fcap], the whole rows as the kernel left them (what the caller had
 * past 2 frames[b] must come back), and, when report is not NULL, report [sum of lens,4], the rows' tokens back to back.  The row
 * padding and the guards behind both buffers are checked here: KX_ERR_STATE. */
int kx_test_prosody_curves(int device_id, const float* curves, const int32_t* frames, int B, int Fcap, const int32_t* lens, int T,
                           const int32_t* idx, int idx_ld, const int32_t* dur, const float* pitch, const float* energy, float* shaped,
                           float* report, char* err, size_t err_len);

/* Both embedding kernels on one id buffer ids [B,ids_stride] (ids_stride >= T; row b valid for lens[b] ids): launch_embed with
 * text_table [n_vocab,512] -> out_text [B,512,T], launch_albert_embed with word [n_vocab,128], type0 [128], pos [T,128] ->
 * out_albert [B,128,T]; columns >= lens[b] come back as -12345.5.  bad = the sticky word the two share, as in the model (0, or
 * (b << 16 | t) + 1 of the first id outside 0..n_vocab-1). */
int kx_test_embed(int device_id, const int64_t* ids, int B, int ids_stride, int T, const int32_t* lens, const float* text_table,
                  const float* word, const float* type0, const float* pos, int n_vocab, float* out_text, float* out_albert,
                  uint32_t* bad, char* err, size_t err_len);

/* The style projections of a call in one launch (launch_style_fc): n_desc descriptors, descriptor i with n_out[i] outputs from
 * half style_off[i] (0 or 128) of styles [B,256]; w = their [n_out[i],128] weights back to back, bias likewise; out
 * [B, sum n_out], descriptor i at the offset Model::add_fc gives it (the sum of the n_out before it). */
int kx_test_style_fc(int device_id, const float* styles, int B, const float* w, const float* bias, const int32_t* n_out,
                     const int32_t* style_off, int n_desc, float* out, char* err, size_t err_len);

/* Row fills and copies.  launch_fill_style_rows as the duration encoder's input is built: rows 512..639 of fill_out [B,640,T] =
 * styles[b][128 + k] over lens[b] columns, everything else -12345.5.  launch_copy_rows of src [B,rows,Ls] into copy_out
 * [B,rows,Ld] (another row stride) over lens[b] mul + add columns of every row, the rest -12345.5. */
int kx_test_rows(int device_id, const float* styles, const int32_t* lens, int B, int T, float* fill_out, const float* src, int rows,
                 int Ls, int Ld, int mul, int add, float* copy_out, char* err, size_t err_len);

/* The back half's kernels that are no conv.  Conventions of the four hooks: every row on the device is padded as the model pads
 * it, every input location a kernel must not read holds NaN (the hook writes them: what the caller has there is not uploaded),
 * every output location it must not write holds -12345.5 and goes back to the caller as it is, and 64 guard bytes stand behind
 * every buffer; a write into row padding or guard is KX_ERR_STATE.  Arguments the model could not produce are KX_ERR_INVALID
 * before anything is launched: frames[b] / lens[b] outside 1 .. the row size, B > 64, Fmax > 64 (source: > 2048), C > 1024,
 * L > 4096.
 *
 * kx_test_source_ragged: source_phase_kernel + source_sample_kernel on f0 [B, 2 Fmax], utterance b valid for 2 frames[b] steps, ->
 * out [B, 600 Fmax], valid for 600 frames[b] samples.  utt_seeds / utt_index [B]: the per-utterance noise keys of the dispatcher;
 * utt_seeds NULL: (seed, utt_base + b); utt_index NULL beside utt_seeds: utterance 0 of every seed. */
int kx_test_source_ragged(int device_id, const float* f0, const int32_t* frames, int B, int Fmax, const float* lin_w, float lin_b,
                          uint64_t seed, uint64_t utt_base, const uint64_t* utt_seeds, const uint32_t* utt_index, int noise_off,
                          float* out, char* err, size_t err_len);

/* stft_kernel: hs [B, hs_ld] (600 Fmax <= hs_ld <= 600 Fmax + 4096), utterance b valid for 600 frames[b] samples, variant 0 / 1
 * (kx_set_stft_variant) -> har [B, 22, 120 Fmax + 1] (11 magnitude rows, 11 phase rows), valid for 120 frames[b] + 1 columns. */
int kx_test_stft(int device_id, const float* hs, int B, int hs_ld, const int32_t* frames, int Fmax, int variant, float* har, char* err,
                 size_t err_len);

/* istft_spec_kernel + istft_ola_kernel: cp [B, 22, 120 Fmax + 1] (11 rows of log-magnitudes, 11 of phase logits), utterance b
 * valid for 120 frames[b] + 1 columns -> spec [B, 22, 120 Fmax + 1] (11 real rows, 11 imaginary rows: what the first kernel
 * stored) and audio [B, 600 Fmax], valid for 600 frames[b] samples. */
int kx_test_istft_head(int device_id, const float* cp, int B, const int32_t* frames, int Fmax, int variant, float* spec, float* audio,
                       char* err, size_t err_len);

/* pool_up2_kernel: x [B, C, L], utterance b valid for lens[b] columns; norm [3, B, C] = the mean, scale and shift planes, which
 * the hook lays out with n_bs > C slots per utterance (the unused ones NaN); w [C, 3], bias [C] -> y [B, C, 2 L], valid for
 * 2 lens[b] columns, on rows of another stride than x's. */
int kx_test_pool_up2(int device_id, const float* x, int B, int C, int L, const int32_t* lens, const float* norm, int n_bs, const float* w,
                     const float* bias, float slope, float* y, char* err, size_t err_len);

/* The weight images of one layer, byte for byte, from the model's own packers (conv_call.hip: pack_conv or pack_convT, then
 * add_bf16_image and add_f8_image) and nothing else.  n_src = 1..3 float32 sources src[i] [src_rows[i]][Cin][K], row-concatenated
 * as kx::PackSrc takes them; or, with up_stride = s > 0, one transposed-conv weight src[0] [Cin][src_rows[0] = Cout][K = 2 s].
 * Out: meta[9] = BM, rows, n_chunks, n_chunks16, K of the kx::ConvW, then the byte lengths of its images w (f32), w16 (split f16),
 * w16b (bf16) and w8x (e4m3 cross operands), 0 for an image the layer does not get; *unscale = ConvW::unscale; images[4] = host
 * buffers of cap[4] bytes that receive those images.  Every image is allocated with 64 guard bytes behind it and pre-filled with
 * the byte 0xC3, so an entry its packer never writes shows; a changed guard is KX_ERR_STATE.  Sizes no layer has are
 * KX_ERR_INVALID before any launch: rows (all sources; s Cout) outside 1..4096, Cin outside 1..2048, K outside 1..24.  A layer the
 * packers refuse (non-finite weights, or max|w| 2^ws beyond f16) is their KX_ERR_INVALID and message. */
int kx_test_weight_images(int device_id, const float* const* src, const int32_t* src_rows, int n_src, int Cin, int K, int up_stride,
                          int64_t* meta, float* unscale, void* const* images, const int64_t* cap, char* err, size_t err_len);

/* Fault injection for the two-CU LSTM recurrence (process-wide, test only): nth > 0 makes the nth following launch of
 * the pair kernel, and every later one, lose the second half of each pair and poll with a short limit, so the call it
 * belongs to must fail with KX_ERR_DEVICE (the bounded wait's error path) and the model must fall back to the one-CU
 * kernel; 0 switches it off.  nth = 6 hits the frame-axis LSTM of a forward, after the mid-way error check.
 * Arms only in a process whose environment has KX_TEST_HOOKS=1 (KX_ERR_STATE otherwise). */
int kx_test_lstm_fault(int nth);

/* Workgroups per (utterance, direction) of the LSTM recurrence (process-wide, test only): 2 or 4 = that resident-weights form
 * whatever the batch, 1 = the streaming fall-back (one workgroup), 0 = by batch size (four while 8 B workgroups fit the CUs).
 * All three give the same bits. */
int kx_test_lstm_parts(int n);

#ifdef __cplusplus
}
#endif
#endif /* KOKOROX_HIP_TEST_H */
