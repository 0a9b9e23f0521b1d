// Conv launch assembly, host code only: the weight images of a layer (ConvW) and the plan and kernel arguments of one launch
// (ConvCall), built here once for Model (model.hip) and for the kernel hooks of tests/ (test_hooks.hip), so that the tests
// launch what the model launches.  The callers keep what needs a resource of theirs: device memory for the images, the
// pre-split input image, the flat tile table and the statistics slots (model.h: ConvCall).
#include <cmath>
#include <cstdlib>
#include <string>

#include "model.h"

namespace kx {

// ---- weight images ---------------------------------------------------------------------------------------------------------

static void pack_sizes(ConvW& c) {
    c.BM = conv_pick_bm(c.rows);
    c.n_chunks = (c.Cin + CONV_CK - 1) / CONV_CK;
    c.n_chunks16 = (c.Cin + 15) / 16;
}

// What the pack path carries: a layer whose weights are all finite and whose largest, times the layer's power of two, fits f16.
// The shift is clamped at -8 (pick_weight_shift), so max|w| 2^ws > 65504 only from 2^24 (65504 / 65536) upwards, where hi would
// be an infinity and lo = inf - inf a NaN.  Anything else is refused here, at load time, with KX_ERR_INVALID.
static float max_absmax(float a, float b) { return std::isnan(a) || std::isnan(b) ? std::nanf("") : std::fmax(a, b); }

// the weight shift of the split-f16 image: 2^ws scales the largest weight to f16's upper range, c.unscale undoes it
static float weight_scale(ConvW& c, float absmax) {
    if (!std::isfinite(absmax)) throw Error(1, "conv weights: non-finite weight (a NaN or an infinity) in the layer");
    const int ws = pick_weight_shift(absmax);
    if (std::ldexp(absmax, ws) > 65504.f)
        throw Error(1, "conv weights: max|w| = " + std::to_string(absmax) + " is beyond the split's range (max|w| 2^" + std::to_string(ws) +
                           " must fit f16: at most 65504)");
    c.unscale = std::ldexp(1.0f, -ws);
    return std::ldexp(1.0f, ws);
}

ConvW pack_conv(const PackSrc& src, int Cin, int K, hipStream_t s, const DevAlloc& alloc) {
    ConvW c;
    c.rows = src.rows[0] + src.rows[1] + src.rows[2];
    c.Cin = Cin;
    c.K = K;
    pack_sizes(c);
    float amax = 0.f;
    for (int i = 0; i < 3; ++i)
        if (src.p[i]) amax = max_absmax(amax, device_absmax(src.p[i], (long)src.rows[i] * Cin * K, s));
    const float scale = weight_scale(c, amax);  // (throws before anything is allocated for a layer it refuses)
    float* p = static_cast<float*>(alloc(packed_conv_floats(c.rows, Cin, K, c.BM) * sizeof(float)));
    launch_pack_conv(src, p, c.rows, Cin, K, c.BM, s);
    c.w = p;
    void* p16 = alloc(packed_conv16_halves(c.rows, Cin, K, c.BM) * 2);
    launch_pack_conv16(src, p16, c.rows, Cin, K, c.BM, scale, s);
    c.w16 = p16;
    return c;
}

ConvW pack_convT(const float* w, int Cin, int Cout, int stride, hipStream_t s, const DevAlloc& alloc) {
    ConvW c;
    c.Cin = Cin;
    c.up_cout = Cout;
    c.up_s = stride;
    c.rows = stride * Cout;
    c.K = 2;
    pack_sizes(c);
    const float scale = weight_scale(c, device_absmax(w, (long)Cin * Cout * 2 * stride, s));
    float* p = static_cast<float*>(alloc(packed_conv_floats(c.rows, Cin, 2, c.BM) * sizeof(float)));
    launch_pack_convT(w, p, Cin, Cout, stride, c.BM, s);
    c.w = p;
    void* p16 = alloc(packed_conv16_halves(c.rows, Cin, 2, c.BM) * 2);
    launch_pack_convT16(w, p16, Cin, Cout, stride, c.BM, scale, s);
    c.w16 = p16;
    return c;
}

// bf16(hi + lo) from the split-f16 image, for the direct-A kernels' 128-row tiles
void add_bf16_image(ConvW& c, hipStream_t s, const DevAlloc& alloc) {
    if (c.w16b || !c.w16 || c.BM != 128) return;
    const size_t nh = packed_conv16_halves(c.rows, c.Cin, c.K, c.BM);
    void* p = alloc(nh * 2);
    launch_image_to_bf16(c.w16, p, nh, s);
    c.w16b = p;
}

// the layers the f16f8 kernels take (7- and 11-tap convs, and the 3-tap ones of at most 256 rows: the generator's snake
// resblocks -- the activation is a property of the call, not of the weights, so a few leaky 3-tap convs of the predictor get an
// image they never use)
void add_f8_image(ConvW& c, hipStream_t s, const DevAlloc& alloc) {
    if (c.w8x || !c.w16 || c.up_s || !conv16_f8_layer(c.BM, c.rows, c.K, c.n_chunks16)) return;
    void* p = alloc(packed_conv8x_bytes(c.rows, c.Cin, c.K));
    launch_pack_conv8x(c.w16, p, c.rows, c.Cin, c.K, s);
    c.w8x = p;
}

// ---- one launch ------------------------------------------------------------------------------------------------------------

int conv_tile_count(const int* h_lens, int B, const LenMap& lm, int extra, int bn) {
    int total = 0;
    for (int b = 0; b < B; ++b) {
        const int cols = h_lens[b] * lm.mul + lm.add + extra;
        total += cols > 0 ? (cols + bn - 1) / bn : 0;
    }
    return total;
}

ConvCall conv_call(const ConvW& w, const T& in, const T& out, const ConvOpts& o, const ConvCtx& ctx) {
    KX_REQUIRE(in.C == w.Cin, "internal: conv Cin mismatch");
    // reduced-precision mode (opt-in): the decoder and generator convs that take the direct-A kernel run one f16 MFMA
    // per product; everything upstream of the F0 / N curves (duration head, prosody predictor) and every kernel that is
    // not the direct-A conv (harmonic source, STFT pair, k = 1 GEMMs, conv_post) stays f32-class (hard part 3)
    const int prec1 = (ctx.mode == CONV_F16 && ctx.p1_region) ? 1 : ((ctx.mode == CONV_BF16 && ctx.p1_region && w.w16b) ? 2 : 0);
    // f16f8 mode (the default): the layers that carry an 8-bit cross image run two MFMA-equivalents per product instead of three
    const void* w8x = ctx.mode == CONV_F16F8 ? w.w8x : nullptr;
    const bool upscatter = o.store == ST_UPSCATTER;
    ConvCall call{};
    call.B = ctx.B;

    ConvLaunch c{};
    c.mode = ctx.mode;
    c.prec1 = prec1;
    c.f8 = w8x != nullptr;
    c.BM = w.BM;
    c.rows = w.rows;
    c.n_chunks16 = w.n_chunks16;
    c.K = w.K;
    c.dil = o.dil;
    c.stride = o.stride;
    c.pad = o.pad;
    c.act = o.act;
    c.in_up2 = o.in_up2;
    c.store = o.store;
    c.accum = o.accum;
    c.epi = o.epi;
    c.norm = o.nmean != nullptr;
    c.stats = o.stat_part != nullptr || ctx.stats;
    c.image = ctx.image;
    const bool plain_lens = in.len.mul == 1 && in.len.add == 0 && out.len.lens == in.len.lens && out.len.mul == 1 && out.len.add == 0;
    c.merge_T = ctx.offer_merge && plain_lens ? in.Lmax : 0;
    c.x_bs = in.bs;
    c.x_ld = in.ld;
    c.B = ctx.B;
    c.cols = upscatter ? in.Lmax + 1 : out.Lmax;
    c.cus = ctx.cus;
    c.force = ctx.force;
    ConvPlan& plan = call.plan;
    plan = conv_plan(c);
    if (!ctx.flat) plan.flat_bn = 0;

    ConvArgs& a = call.a;
    a.x = in.p;
    a.x_bs = in.bs;
    a.x_ld = in.ld;
    a.Cin = w.Cin;
    a.in_len = in.len;
    if (o.in_up2) {
        a.in_len.mul *= 2;
        a.in_len.add *= 2;
    }
    a.out_len = upscatter ? o.up_len : out.len;
    a.w = w.w;
    a.bias = w.bias;
    a.nmean = o.nmean;
    a.nscale = o.nscale;
    a.nshift = o.nshift;
    a.n_bs = ctx.n_bs;
    a.act = o.act;
    a.slope = o.slope;
    a.alpha = o.alpha;
    a.K = w.K;
    a.dil = o.dil;
    a.stride = o.stride;
    a.pad = o.pad;
    a.in_up2 = o.in_up2;
    a.Cout = w.rows;
    a.n_chunks = w.n_chunks;
    a.y = out.p;
    a.y_bs = out.bs;
    a.y_ld = out.ld;
    if (o.resid) {
        a.resid = o.resid->p;
        a.r_bs = o.resid->bs;
        a.r_ld = o.resid->ld;
    }
    a.accum = o.accum;
    a.out_mul = o.out_mul;
    a.out_div = o.out_div;
    a.epi = o.epi;
    a.store = o.store;
    a.up_s = w.up_s;
    a.up_pad = o.up_pad;
    a.up_off = o.up_off;
    a.up_reflect = o.up_reflect;
    a.up_cout = w.up_cout ? w.up_cout : 1;
    a.prec1 = prec1;
    a.w16 = w.w16;
    a.w16b = w.w16b;
    a.w8x = w8x;
    a.n_chunks16 = w.n_chunks16;
    a.ws_force = ctx.force;
    // outputs that no cache can hold until the next layer reads them (> 512 MB: L2 is 32 MB, MALL 256 MB) are streamed by the direct-A
    // kernels' interior stores (non-temporal stores and residual loads); smaller ones (small batches, the token axis, the decoder)
    // stay cacheable
    constexpr double EPI_STREAM_BYTES = 512.0 * 1048576.0;
    a.epi_stream = ctx.epi_stream >= 0 ? ctx.epi_stream
                                       : plan.form != FORM_F32 && (double)ctx.B * w.rows * out.ld * 4.0 > EPI_STREAM_BYTES;
    a.xcd_swizzle = 1;
    a.x_prescale = std::ldexp(1.0f, w.act_shift);
    a.w_unscale = std::ldexp(w.unscale, -w.act_shift);  // (exact: both are powers of two)
    if (plan.merged) {  // k = 1 GEMM on a short axis: one merged column space for the whole batch
        a.merge_T = in.Lmax;
        a.merge_B = ctx.B;
    }
    if (plan.stat_cols && o.stat_part) call.set_stats(o.stat_part);  // InstanceNorm partial sums in the epilogue
    return call;
}

}  // namespace kx
