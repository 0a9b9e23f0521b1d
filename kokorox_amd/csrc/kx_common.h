// Internal declarations shared by the kokorox_hip translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include <atomic>
#include <mutex>

#include "host_request.h"
#include "kx_error.h"

namespace kx {

constexpr int KX_MAX_DEVICES = 64;

// hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE attribute of a kernel, and a process may hold one model per GPU,
// each driven from a host thread of its own (kx_create_replicas, the dispatcher's workers): one of these per launcher
// (function-local static), raised per device only as far as a launch needs, race-free.
struct DynLdsLimit {
    std::atomic<size_t> limit[KX_MAX_DEVICES];
    std::mutex mu;
    DynLdsLimit() {
        for (auto& l : limit) l.store(64 * 1024);  // what a kernel may use without the attribute
    }
    void ensure(const void* kern, size_t lds) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= KX_MAX_DEVICES) throw Error(3, "dynamic LDS limit: bad current device");
        if (lds <= limit[dev].load(std::memory_order_acquire)) return;
        std::lock_guard<std::mutex> lk(mu);
        if (lds <= limit[dev].load(std::memory_order_relaxed)) return;
        const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) throw Error(3, std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString(e));
        limit[dev].store(lds, std::memory_order_release);
    }
};

#define KX_HIP(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            throw kx::Error(3, std::string(#expr) + ": " + hipGetErrorString(e_) + " (" +  \
                                   __FILE__ + ":" + std::to_string(__LINE__) + ")");       \
    } while (0)

// Valid length of utterance b for a tensor = lens[b] * mul + add (lens = tokens or frames).
struct LenMap {
    const int* lens;
    int mul, add;
};

// ---- conv1d as implicit GEMM on the f32 MFMA (conv_mfma.hip) -------------------------
constexpr int CONV_CK = 8;  // input channels per K-chunk

enum ConvAct { ACT_NONE = 0, ACT_LEAKY = 1, ACT_SNAKE = 2 };
enum ConvStore { ST_NORMAL = 0, ST_TMAJOR = 1, ST_UPSCATTER = 2 };
enum ConvEpi { EPI_NONE = 0, EPI_GELU_NEW = 1 };

struct ConvArgs {
    // input [B][Cin][x_ld]
    const float* x;
    long x_bs;
    int x_ld;
    int Cin;
    LenMap in_len;   // valid (virtual, after in_up2) input length
    LenMap out_len;  // valid output length (ST_UPSCATTER: un-shifted upsampled length)
    // packed weights [co_tile][chunk][k][8][BM] and bias [Cout]
    const float* w;
    const float* bias;
    // optional per (b, ci) affine (x - mean) * scale + shift, each [B][n_bs]
    const float* nmean;
    const float* nscale;
    const float* nshift;
    int n_bs;
    int act;
    float slope;
    const float* alpha;  // snake, [Cin]
    int K, dil, stride, pad;
    int in_up2;  // read x[p >> 1] (nearest x2 upsample of the input)
    int Cout;    // GEMM rows (ST_UPSCATTER: up_s * up_cout)
    int n_chunks;
    // output [B][Cout][y_ld] (ST_TMAJOR: [B][L][y_ld])
    float* y;
    long y_bs;
    int y_ld;
    const float* resid;
    long r_bs;
    int r_ld;
    int accum;
    float out_mul;
    float out_div;
    int epi;
    int store;
    int up_s, up_pad, up_off, up_reflect, up_cout;
    // f16x3 path (conv_f16x3.hip): split-f16 weight image, 16-channel chunks, 2^-ws to undo the weight scale
    const void* w16;
    const void* w16b;  // the bf16 form of the same image (prec1 == 2 launches of the direct-A kernel swap it in), or null
    const void* w8x;   // f16f8 mode (CONV_F16F8): the 8-bit image of the weights' cross-term operands (launch_pack_conv8x), or null
    int epi_stream;    // the direct-A kernels' interior stores and residual loads non-temporal (the output tensor is far beyond L2 + MALL)
    int n_chunks16;
    float w_unscale;
    float x_prescale;  // f16x3: power of two applied to the transformed input before the hi/lo split (w_unscale carries
                       // its inverse); 1 unless a layer's activations are so small that their low halves would be lost
    // k = 1 GEMMs over a short axis: columns of all B utterances form one merged space of B * merge_T
    // columns (utterance = col / merge_T); 0 = off.  Requires K = 1, stride 1, pad 0, no norm, no in_up2.
    int merge_T;
    int merge_B;
    float2* stat_part;  // optional [B][Cout][stat_tiles] partial (sum, sum of squares) of the stored values
    int stat_tiles;
    int xcd_swizzle;               // XCD-aware tile order of the f16x3 kernels: always 1 (conv_call.hip)
    int ws_force;                  // test hook: 1 = the LDS-DMA kernel forms only (no direct-A kernel), 2 = the direct-A kernel whatever the grid
    unsigned long long* stamps;  // retired diagnostic, never set (null); its run-time tests are open work: DESIGN.md section 3
    int prec1;  // direct-A conv: the reduced-precision forms, opt-in: 1 = one f16 MFMA per product (KOKOROX_CONV=f16), 2 = one bf16
                // MFMA per product on a bf16 weight image (KOKOROX_CONV=bf16)
    int dephase_cycles, dephase_mode;  // retired diagnostic, never set (0)
    int dbg;  // retired timing ablations, never set (0)
    // Flat tile list of a ragged batch (direct-A kernels): tile_prefix[b] = column tiles of the utterances before b (so
    // tile_prefix[B] = all of them); the grid is then ONE dimension of tile_prefix[B] * flat_ny workgroups, none of them
    // dead, and the XCD-aware order runs over the whole list.  null = the (max_cols / BN) x row tiles x B grid with
    // early-exit workgroups.  (The dense grid deals each XCD the same eighth of EVERY utterance's slab, so on a ragged
    // batch the XCDs that hold the slabs' tails run empty and the launch takes as long as if every utterance had the
    // longest length: profiles/r04_ragged_attribution.txt.)
    const int* tile_prefix;
    int flat_ny;     // row tiles (the fastest index of the list)
    int flat_B;
    int flat_tiles_host, flat_bn_host;  // host side only: tile_prefix[B] as the host counted it, and the tile width it assumed
    // Pre-split input image (direct-A convs whose window is staged by many row tiles; conv_f16x3_pre.hip): the input after
    // its AdaIN affine, activation, pre-scale and f16 hi / lo split, per utterance [chunk of 16 channels][hi|lo][octet][x16_ld
    // columns][8 halves] = the kernels' LDS image; x16_bs bytes per utterance.  null = the kernel transforms a.x itself.
    const void* x16;
    long x16_bs;
    int x16_ld;
};

// ---- the launch plan of a conv (conv_plan.hip): kernel form, tile, statistics slots, flat tile list, input staging ----------
enum ConvMode { CONV_F32 = 0, CONV_F16X3 = 1, CONV_F16X3_LDS = 2, CONV_F16X3_DA = 3, CONV_F16 = 4, CONV_BF16 = 5, CONV_F16F8 = 6 };  // (2, 3: test hook only: f16x3 kept on the LDS-DMA kernel forms of conv_f16x3.hip / forced through conv_f16x3_da.hip)
enum ConvForm {
    FORM_F32 = 0,  // conv1d_mfma_kernel<bm, ..> (conv_mfma.hip: the f32 mode)
    FORM_LDS,      // conv1d_f16x3_kernel<bm, bn, wm, wn, act, vt == 1 ? 3 : vt, pf, vt> (conv_f16x3.hip: weights by LDS-DMA; vt > 1: k = 1 GEMMs)
    FORM_DAG,      // conv1d_f16x3_dag_kernel<act> (conv_f16x3_dag.hip: k = 1 GEMMs, 128 x 128 tiles)
    FORM_DAGN,     // conv1d_f16x3_dagn_kernel<act> (the same on small grids: 128 x 32 tiles)
    FORM_DA,       // conv1d_f16x3_da_kernel<act, kt, bn / 32, p1, .., bf>, 4 x 1 waves (conv_f16x3_da.hip; p1: conv_f16x3_da_p1.hip)
    FORM_DA_W2,    // its 2 x 2-wave forms of the 256-column tile (conv_f16x3_da_w2.hip)
    FORM_DA_S16,   // its 16x16x32 forms: 11 / 7 taps, 192 / 128 columns (conv_f16x3_da_s16.hip)
    FORM_DA_F8,    // their f16f8 forms: 11 / 7 / 3 taps (conv_f16x3_da_f8.hip)
    FORM_DA_PRE,   // its forms that stage a pre-split input image (conv_f16x3_da_pre.hip)
    FORM_DAPN,     // the narrow pre-split form for small grids: 32 rows x 128 columns, no staging (conv_f16x3_dapn.hip)
};
// ConvArgs::ws_force, the test hooks' overrides (0 in the model): the low two bits hold 1 = the LDS-DMA forms only or 2 = the
// direct-A forms whatever the grid; FORCE_DA_4X1 = the 4 x 1 wave layout on the 256-column tile too, FORCE_NO_S16 = no 16x16x32 form
enum ConvForce { FORCE_LDS = 1, FORCE_DA = 2, FORCE_DA_4X1 = 4, FORCE_NO_S16 = 8 };

struct ConvLaunch {  // what the plan of a conv launch depends on
    int mode;          // ConvMode: CONV_F32, CONV_F16X3, CONV_F16, CONV_BF16 or CONV_F16F8
    int prec1;         // ConvArgs::prec1 (1: one f16 MFMA per product; 2: one bf16 MFMA, on the layer's bf16 image)
    int f8;            // the launch carries the layer's 8-bit cross image (ConvArgs::w8x)
    int BM, rows, n_chunks16, K, dil, stride, pad, act, in_up2, store, accum, epi;
    int norm;          // AdaIN affine on the input
    int stats;         // InstanceNorm partial sums of the output requested
    int image;         // pre-split input image: 0 = none can be made, 1 = by the layer's shape, 2 = wherever the layer has that form
    int merge_T;       // > 0: input and output share one plain length array and this longest length (the columns may be merged)
    long x_bs;         // input floats per utterance
    int x_ld;
    int B, cols;       // batch; columns of the launch (the longest output; ST_UPSCATTER: the longest input + 1)
    int cus;           // CUs of the device, or of the model's CU partition
    int force;         // ConvArgs::ws_force
};
struct ConvPlan {
    int form;                           // ConvForm
    int bm, act, kt, wm, wn, vt, pf, p1, bf;  // the form's template parameters (kt: the direct-A forms' compile-time taps, 0 = run time)
    int bn;                             // tile width: columns per workgroup
    int cols;                           // columns of the launch (merged: B x merge_T)
    int merged;                         // one merged column space for the batch (ConvArgs::merge_T, merge_B)
    int pre;                            // the input is written as a pre-split image first (ConvArgs::x16)
    int stat_cols, stat_tiles;          // fused InstanceNorm partial sums: slot width, slots per row (0: not fused)
    int flat_bn;                        // tile width of the flat tile list of a ragged batch (= bn), 0 = the form takes none
};
ConvPlan conv_plan(const ConvLaunch& c);
bool conv16_f8_layer(int BM, int rows, int K, int n_chunks16);  // layers that get an 8-bit cross image in f16f8 mode (dilation 1)
// carries the plan out: one launch, a conv1d_mfma / conv1d_f16x3 / direct-A kernel (conv_f16x3.hip)
void launch_conv(const ConvPlan& p, const ConvArgs& a, int B, hipStream_t s);
int conv16_cu_count();  // CUs of the current device, or of the launching model's CU partition (conv_f16x3.hip)
int cu_count_override(); // model_forward.hip: the CU partition of the model that is launching on this thread (0 = none)

// pre-split images (conv_f16x3_pre.hip)
size_t conv16_pre_image_bytes(int Cin, int x_ld);  // per utterance
// writes the image of a.x (a's norm parameters, activation, slope, pre-scale) for B utterances of at most Lmax columns
void launch_split_image(const ConvArgs& a, int B, int Lmax, void* img, long img_bs, hipStream_t s);

// tile_prefix of a LenMap for `bn`-column tiles (+ `extra` columns per utterance: the polyphase convs' L + 1), on the device
void launch_tile_prefix(LenMap len, int extra, int bn, int B, int* out, hipStream_t s);

inline int conv_pick_bm(int rows) { return rows >= 128 ? 128 : (rows > 32 ? 64 : 32); }

void launch_conv1d(const ConvArgs& a, int BM, int B, int max_cols, hipStream_t s);

// weight repack: canonical layouts -> [co_tile][chunk][k][8][BM]
struct PackSrc {
    const float* p[3];  // up to three row-concatenated sources, each [rows_i][Cin][K]
    int rows[3];
};
void launch_pack_conv(const PackSrc& src, float* dst, int Cout, int Cin, int K, int BM, hipStream_t s);
// ConvTranspose1d weight [Cin][Cout][k], k == 2*s  ->  polyphase GEMM rows (p, co), 2 taps
void launch_pack_convT(const float* w, float* dst, int Cin, int Cout, int s, int BM, hipStream_t s_);
size_t packed_conv_floats(int rows, int Cin, int K, int BM);

// f16x3 split path: the launchers of the plan's forms (launch_conv calls them)
// direct-A conv units, one entry each: conv_f16x3_da.hip (FORM_DA, f16x3), _p1.hip (FORM_DA, reduced precision), _w2.hip,
// _s16.hip, _f8.hip, _pre.hip
void launch_conv16_da(const ConvPlan& p, const ConvArgs& a, int B, hipStream_t s);
void launch_conv16_da_p1(const ConvPlan& p, const ConvArgs& a, int B, hipStream_t s);
void launch_conv16_da_w2(const ConvPlan& p, const ConvArgs& a, int B, hipStream_t s);
void launch_conv16_da_s16(const ConvPlan& p, const ConvArgs& a, int B, hipStream_t s);
void launch_conv16_da_f8(const ConvPlan& p, const ConvArgs& a, int B, hipStream_t s);
void launch_conv16_da_pre(const ConvPlan& p, const ConvArgs& a, int B, hipStream_t s);
// the narrow pre-split form (conv_f16x3_dapn.hip): 32 rows x 128 columns per workgroup, B fragments straight from the image
void launch_conv1d_f16x3_dapn(const ConvArgs& a, int B, int max_cols, hipStream_t s);
// k = 1 GEMMs (incl. the merged token-axis form) in the direct-A form (conv_f16x3_dag.hip): FORM_DAG / FORM_DAGN
void launch_conv1d_f16x3_dag(const ConvPlan& p, const ConvArgs& a, int B, hipStream_t s);
size_t packed_conv16_halves(int rows, int Cin, int K, int BM);
float device_absmax(const float* p, long n, hipStream_t s);
int pick_weight_shift(float absmax);
void launch_pack_conv16(const PackSrc& src, void* dst, int Cout, int Cin, int K, int BM, float wscale, hipStream_t s);
void launch_pack_convT16(const float* w, void* dst, int Cin, int Cout, int sd, int BM, float wscale, hipStream_t s);
// a split-f16 weight image (hi + lo = the f32 weight to 22 bits) -> the same layout with bf16(hi + lo) in the hi slots (CONV_BF16)
void launch_image_to_bf16(const void* w16, void* dst, size_t n_halves, hipStream_t s);
// f16f8 mode: the cross terms a_lo b_hi + a_hi b_lo of the split product on v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 x e4m3, twice the
// f16 rate), a_hi b_hi stays on the f16 MFMA.  The weights' side of the cross terms, from a split-f16 image of 128-row tiles:
// [row tile][chunk16][tap group of 4][k-group g = octet + 2 (tap pair)][slot 0 | 1][128 rows][16 B] (a lane's 32-byte operand is
// its row's two slots: taps 4 m + 2 (g >> 1) and + 1; taps >= K are zero; a load instruction reads one slot of 16 consecutive
// rows = 256 contiguous bytes), a slot = four dwords [e4m3(2^7 lo(2d)), e4m3(2^7 lo(2d+1)), e4m3(2^-4 hi(2d)),
// e4m3(2^-4 hi(2d+1))] of the octet's channel pairs d -- byte for byte the partner of the activation image's 8-bit plane
// (split_pair_f8, conv_f16x3_common.h); the products of a slot carry 2^7 (undone by the instruction's block scale).
size_t packed_conv8x_bytes(int rows, int Cin, int K);
void launch_pack_conv8x(const void* w16, void* dst, int rows, int Cin, int K, hipStream_t s);

// ---- everything else (kernels_misc.hip) ----------------------------------------------
void launch_vec_add(const float* a, const float* b, float* out, int n, hipStream_t s);
void launch_transpose_whh(const float* whh, float* out, hipStream_t s);  // [1024 rows][256 k] -> [64][1024][4 k]

void launch_albert_embed(const int64_t* ids, long ids_stride, const float* word, const float* type0,
                         const float* pos, float* out, long bs, int ld, const int* lens, int B, int Tmax,
                         int n_vocab, unsigned* bad_id, hipStream_t s);
void launch_embed(const int64_t* ids, long ids_stride, const float* table, int C, float* out, long bs, int ld,
                  const int* lens, int B, int Tmax, int n_vocab, unsigned* bad_id, hipStream_t s);

enum LnMode { LN_PLAIN = 0, LN_AFFINE = 1, LN_ADA = 2 };
// channel layer-norm over C rows of [B][C][ld], in place allowed. ADA: g/be are [B][g_bs], (1+g)*xhat+be
void launch_layernorm_ch(const float* x, float* y, long bs, int ld, int C, LenMap len, int B, int Lmax,
                         float eps, int mode, const float* g, const float* be, int g_bs, float leaky,
                         hipStream_t s);

void launch_attention(const float* qkv, long bs, int ld, float* ctx, long cbs, int cld, const int* lens, int B,
                      int Tmax, hipStream_t s);

struct FcDesc {
    const float* w;  // [n_out][128]
    const float* b;  // [n_out]
    int n_out;
    int style_off;  // 0 or 128 within the 256-float style row
    long out_off;   // into the gamma/beta arena, per utterance
};
void launch_style_fc(const FcDesc* d_desc, int n_desc, const float* styles, float* out, long out_bs, int B,
                     hipStream_t s);

// instance-norm statistics of [B][C][ld] rows -> mean, scale = rstd*(1+gamma), shift = beta
// finalize fused statistics: partials [B][C][tiles] -> mean, scale, shift (same outputs as launch_in_stats)
// cols_per_tile = STAT_RAW_TILES: the tiles are the high and low parts of launch_in_stats' raw_out, summed whatever the length
constexpr int STAT_RAW_TILES = 0;
void launch_stats_finalize(const float2* part, int tiles, int cols_per_tile, int C, LenMap len, int B, const float* gb,
                           long gb_bs, float* mean, float* scale, float* shift, int n_bs, hipStream_t s);
void launch_in_stats(const float* x, long bs, int ld, int C, LenMap len, int B, const float* gb, long gb_bs,
                     float* mean, float* scale, float* shift, int n_bs, float2* raw_out, hipStream_t s);

// diagnostics (real-weights report): absmax and sum of squares of a conv's input after its AdaIN affine
// (out[0] = absmax bits as uint, out[1] = sum of squares, out[2] = element count)
void launch_diag_stats(const float* x, long bs, int ld, int C, LenMap len, int B, int Lmax, const float* nmean,
                       const float* nscale, const float* nshift, int n_bs, float* out3, hipStream_t s);

void launch_style_mix(const float* table, int n_voices, const int* voice_ids, const float* weights, int max_mix,
                      const int* rows, const int* kinds, float* styles, int B, hipStream_t s);

// ---- the output stage of a call (request_launch.hip and the request_*.hip units it launches; host_request.h: OutputPlan, build_output_plan) ----------------------
// Device memory for a plan's tables, which the launchers copy the plan into: req [R], cum [B + 1], join [B] (used by a joined
// or levelled plan only), mark [B] (used when a request wants marks only); a measured plan (OutputPlan::measured) also level [R]
// and peak, the partials table of the peak pass (plan.peak_dwords() dwords: scratch, nothing in it outlives a call)
struct OutputTables {
    PackReq* req;
    long* cum;
    JoinRow* join;
    MarkRow* mark;
    LevelSpec* level;
    uint32_t* peak;
    // a plan with loudness (OutputPlan::loud): loud [R], hops = the hop energies [R][plan.max_hops] (plan.hop_doubles() doubles:
    // scratch like peak) and loud_pow = the meter's transition powers, 4 * LOUD_POWERS * 16 doubles (host_request.h: loud_powers)
    LoudSpec* loud;
    double* hops;
    double* loud_pow;
    // a plan with a true peak (OutputPlan::true_peak): the second partials table, plan.truepeak_dwords() dwords, scratch like peak
    uint32_t* tpeak;
    // a plan with a limited request (OutputPlan::limited): limit [R], lpart = the partials of r, plan.limit_dwords() dwords, and lim =
    // the limited streams back to back, plan.lim_floats floats; both scratch like peak
    LimitRow* limit;
    uint32_t* lpart;
    float* lim;
    // a plan with FLAC (OutputPlan::has_flac): frow [R], finfo [R], and scratch sized by plan.flac_slots: fslot = the encoded frames,
    // FLAC_SLOT bytes each (16-byte aligned), flen = their sizes and foff = their offsets behind the request's first frame
    FlacRow* frow;
    FlacInfo* finfo;
    uint32_t* fslot;
    int* flen;
    long* foff;
    // a plan with pieces (OutputPlan::has_pieces): piece [R], and piece_tail = the carried tails back to back, at most R * PIECE_TAIL
    // floats; `join` is then used whatever the plan's other flags say
    PieceRow* piece;
    float* piece_tail;
};
// Everything between "the plan is built" and "copy to the host", for the model and for the test hook: the resampler when
// plan.y_floats > 0 (d_y: that many floats, null when 0), the packer into d_packed (16-byte aligned, plan.total_bytes long), and
// when plan.n_marks > 0 the token marks at d_packed + plan.marks_off.  audio [B][audio_ld]; dur [B][512] as duration_kernel
// wrote it and lens [B], both on the device.  The joined form of the kernels runs only when plan.joined.  A measured plan: the peak
// pass and the gain kernel between resampler and packer, {p, g} of every request at d_packed + plan.levels_off (8-aligned; d_packed
// is then plan.end_bytes() long), and the levelled packer when plan.levelled.  A plan with loudness: request_loudness_kernel behind
// the peak pass and request_loudness_gain_kernel behind the gain kernel, {I, n_g} of every metered request at d_packed + plan.loud_off.
// A plan with a FLAC request (OutputPlan::has_flac): the three FLAC kernels behind the limiter, the body at the front of its region
// and the true size of every region at d_packed + plan.flac_off; host_request.h: close_flac_gaps moves the regions together.
// A plan with an ADPCM request (OutputPlan::adpcm_groups > 0): adpcm_blocks_kernel at the same place writes those regions, header and
// blocks, where the plan put them; the packer leaves them alone.
// A plan with pieces (OutputPlan::has_pieces): resample_pieces_kernel in the resampler's place, for every request of the plan, and
// piece_carry_kernel behind it, every request's carry record at d_packed + plan.carry_off (8-aligned; d_packed is then
// plan.end_bytes() long).  The gain, the packer and the marks run on the emitted range as they run on a whole request.
void launch_output_plan(const float* audio, long audio_ld, const int* dur, const int* lens, const OutputPlan& plan,
                        const OutputTables& t, float* d_y, void* d_packed, hipStream_t s);
// its two halves: the bodies, and the marks (n_marks > 0) into a block of their own, 8-byte aligned
void launch_pack_plan(const float* audio, long audio_ld, const OutputPlan& plan, const OutputTables& t, float* d_y, void* out,
                      hipStream_t s);
void launch_token_marks(const int* dur, const int* lens, const OutputPlan& plan, const OutputTables& t, void* marks, hipStream_t s);
// edges [B][2] = {dur[b][0], dur[b][lens[b] - 1]} (8-byte aligned): what the host's join plan needs beside the frame counts
void launch_edge_durations(const int* dur, const int* lens, int* edges, int B, hipStream_t s);
// Host output buffers of the kx_infer* calls: page-locked and pooled (one asynchronous D2H copy at PCIe rate instead
// of per-utterance pageable copies); host_out_free also accepts plain malloc'd pointers (dispatcher results).
void* host_out_alloc(size_t bytes);
void host_out_free(void* p);
// n pointers into one host_out_alloc'd buffer handed to n owners: each is released with host_out_free, the buffer goes back
// to the pool with the last one (parts[0] may be the buffer's own address)
void host_out_share(void* base, void* const* parts, int n);
// page-locked bytes of shared batch buffers that owners still hold a part of (what the dispatcher caps: a client that keeps one
// result keeps its whole batch's buffer pinned)
size_t host_out_live_bytes();
void launch_fill_style_rows(float* dst, long bs, int ld, int row0, const float* styles, int style_off,
                            const int* lens, int B, int Tmax, hipStream_t s);
void launch_copy_rows(const float* src, long sbs, int sld, float* dst, long dbs, int dld, int rows, LenMap len,
                      int B, int Lmax, hipStream_t s);

// xchg / err_word: exchange buffer (lstm_exchange_bytes(B), any contents) and sticky error word of the two-CU form;
// null = the one-CU streaming kernel
void launch_lstm(const float* gx, long gx_bs, int gx_ld, const float* whhT, float* y, long y_bs, int y_ld,
                 LenMap len, int B, unsigned long long* xchg, unsigned* err_word, hipStream_t s,
                 unsigned* epoch_state = nullptr);  // epoch_state: the buffer's own launch counter (see launch_lstm)
size_t lstm_exchange_bytes(int B);
void lstm_set_parts(int n);       // test hook: 2 / 4 workgroups per (utterance, direction) whatever the batch, 0 = by batch size
void lstm_set_test_fault(int on);  // test hook: the two-CU kernel's partner never shows up (bounded-poll error path)

void launch_duration(const float* logits, long bs, int ld, const float* speeds, int n_speed, const int* lens,
                     const int* pinned, int n_pinned, int* dur, int* frames, int* idx, int idx_ld, unsigned* overflow, int B,
                     hipStream_t s);  // overflow: sticky word, first row cut at idx_ld frames as b + 1 (see duration_kernel)
// Prosody (include/kokorox_hip.h, "prosody"; kernels_misc.hip).  launch_duration with a call's per-token rate / fixed frame
// counts ([B][p_stride] on the device, either may be null, not both): only for a call that gives one.
void launch_prosody_duration(const float* logits, long bs, int ld, const float* speeds, int n_speed, const int* lens,
                             const int* pinned, int n_pinned, const float* rate, const int* fixed, long p_stride, int* dur,
                             int* frames, int* idx, int idx_ld, unsigned* overflow, int B, hipStream_t s);
// The two curves ([B][2][ld]: F0, N; 2 frames[b] steps each) shaped in place by the per-token pitch / energy ratios ([B][p_stride],
// either may be null), and, where rep_first[b] >= 0, the report of row b's tokens at report + 4 (rep_first[b] + t) (16-byte aligned).
void launch_prosody_curves(float* curves, long bs, int ld, const int* frames, const int* lens, const int* dur, const int* idx,
                           int idx_ld, const float* pitch, const float* energy, long p_stride, const long* rep_first, float* report,
                           int B, hipStream_t s);
// Fit (include/kokorox_hip.h, "fit"; kernels_misc.hip).  launch_fit_weights: w [B][512] = every token's duration before rintf,
// clamped, and fitted [B][512] = the caller's fixed counts (fixed [B][f_stride], may be null) or 0; rate [B][r_stride] may be null.
// launch_fit_spans: prefix [B + 1] = the running sum of lens, spans [n_spans] in that flat token space (fit_ok made them); the free
// tokens of every span get their fitted count in `fitted`, and results [n_spans] what the fit chose.  launch_prosody_duration then
// takes `fitted` as its fixed array, stride 512.
void launch_fit_weights(const float* logits, long bs, int ld, const float* speeds, int n_speed, const int* lens, const float* rate,
                        long r_stride, const int* fixed, long f_stride, float* w, int* fitted, int B, hipStream_t s);
void launch_fit_spans(const int* prefix, int B, const FitFlat* spans, int n_spans, const float* w, int* fitted, FitResult* results,
                      hipStream_t s);
void launch_gather_cols(const float* src, long sbs, int sld, float* dst, long dbs, int dld, int C,
                        const int* idx, int idx_ld, const int* frames, int B, int Fmax, hipStream_t s);

// AdainResBlk1d "pool": leaky(norm(x)) -> depth-wise ConvTranspose1d(k3,s2,p1,op1)
void launch_pool_up2(const float* x, long xbs, int xld, int C, const float* mean, const float* scale,
                     const float* shift, int n_bs, float slope, const float* w, const float* bias, float* y,
                     long ybs, int yld, LenMap in_len, int B, int Lmax_in, hipStream_t s);

void launch_source(const float* f0, long f0_bs, const int* frames, int B, int Fmax, const float* lin_w,
                   const float* lin_b, uint64_t seed, uint64_t utt_base, const uint64_t* utt_seeds,
                   const uint32_t* utt_index,  // beside utt_seeds: row b draws (utt_seeds[b], utt_index[b]); null = utterance 0
                   int noise_off, float* phase_ws,
                   float* har, long har_bs, hipStream_t s);
enum StftVariant { STFT_ONNX = 0, STFT_TORCH = 1 };  // (kernels_misc.hip: the two STFT / iSTFT pairs)
void launch_stft(const float* har_src, long hs_bs, float* har, long bs, int ld, const int* frames, int B,
                 int Fmax, int variant, hipStream_t s);
void launch_istft_head(const float* cp, long bs, int ld, float* spec_ws, float* audio, long audio_ld,
                       const int* frames, int B, int Fmax, int variant, hipStream_t s);
void init_dft_tables();

}  // namespace kx
