// Stand-alone kernel hooks for tests/ (include/kokorox_hip_test.h): libkokorox_hip_test.so, a library of its own that links
// against libkokorox_hip.so -- the production library exports none of them.  The conv hooks take their weight images, launch
// plan and kernel arguments from conv_call.hip, the code Model runs; what is theirs is the buffers, the tensor views over them
// and the checks around the launch.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/kokorox_hip.h"
#include "../../include/kokorox_hip_test.h"
#include "model.h"

using kx::Error;
using kx::Model;

#include "kx_handle.h"

#include "check_device.h"
#include "api_guard.h"
using kx::guarded;
using kx::guarded_free;
using kx::set_err;

namespace {
struct DevMem {
    std::vector<void*> p;
    ~DevMem() {
        for (void* q : p) (void)hipFree(q);
    }
    template <class Tp>
    Tp* get(size_t n) {
        void* q = nullptr;
        KX_HIP(hipMalloc(&q, (n ? n : 1) * sizeof(Tp)));
        p.push_back(q);
        return static_cast<Tp*>(q);
    }
    template <class Tp>
    Tp* up(const Tp* h, size_t n) {
        Tp* d = get<Tp>(n);
        KX_HIP(hipMemcpy(d, h, n * sizeof(Tp), hipMemcpyHostToDevice));
        return d;
    }
};
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

// ---- stand-alone kernel hooks for tests/ ------------------------------------------------------

namespace {
struct ConvTestExtra {  // epilogue forms beyond bias: residual, accumulate into y, scale / divide, fused statistics
    const float* resid = nullptr;
    int accum = 0;
    float out_mul = 1.f, out_div = 1.f;
    float* stats_out = nullptr;  // [B][Cout][2] = sum, sum of squares over the stored row
    const int32_t* lens = nullptr;  // [B] valid input columns per utterance (ragged batch); null = all L
    int pad_ld = 0;              // rows padded to a multiple of 32 floats as in the model (x padding = NaN, y padding checked)
    int flat = 0;                // ragged batches: the flat tile list the model gives the direct-A kernels (ConvArgs::tile_prefix)
    int up_off = 0, up_reflect = 0;  // transposed: the output starts at column up_off of y (and column 0 = reflection of column 1)
    // the launch options a forward sets beyond that (kx_test_conv1d_opts)
    int in_up2 = 0;              // the conv reads x[p >> 1]: L stored columns stand for 2 L
    int epi = kx::EPI_NONE;
    int merged = 0;              // input and output share one plain length array: conv_call offers the plan merged columns (ConvLaunch::merge_T)
    int tmajor = 0;              // ST_TMAJOR: y is [B][Lout][Cout]
    int prec1 = 0;               // 1 / 2: one f16 / bf16 MFMA per product (the hook runs CONV_F16 / CONV_BF16 inside the reduced-precision region; 2: on add_bf16_image's image)
    int act_shift = 0;           // x_prescale = 2^act_shift, w_unscale carries its inverse
    int epi_stream = 0;
    const float* norm_gb = nullptr;  // [B][2 Cout] (gamma | beta): finalize the conv's own partial sums into ...
    float* norm_out = nullptr;       // ... [3][B][Cout] = mean, scale, shift (launch_stats_finalize)
    int64_t* plan_out = nullptr;     // [17] the ConvPlan that was launched, fields as kx_test_conv_plan returns them
    // the generator's length maps (opts[8 ..] of kx_test_conv1d_opts).  len_mul_in > 0: lens[] are units (the model's frames), utterance
    // b stores lens[b] * len_mul_in + len_add_in input columns and owns lens[b] * len_mul_out + len_add_out output columns
    int len_mul_in = 0, len_add_in = 0, len_mul_out = 0, len_add_out = 0;
    int view = 0;    // x, resid and y are row slices of taller tensors: VIEW_TOP foreign rows above them, VIEW_ROWS - VIEW_TOP below
    int strict = 0;  // a call that uses one of these fields: unowned output columns hold the sentinel, guard bytes behind the buffers
};
constexpr int VIEW_ROWS = 8, VIEW_TOP = 3, GUARD = 16;  // (GUARD floats = 64 bytes)
const float GUARD_VALUE = 7.25e9f;
}  // namespace

// a ConvPlan as the 17 integers kx_test_conv_plan and kx_test_conv1d_opts return
static void plan_fields(const kx::ConvPlan& p, int64_t* out) {
    const int v[] = {p.form, p.bm, p.act, p.kt, p.wm, p.wn, p.vt, p.pf, p.p1, p.bf, p.bn, p.cols, p.merged, p.pre, p.stat_cols,
                     p.stat_tiles, p.flat_bn};
    for (int i = 0; i < 17; ++i) out[i] = v[i];
}

static int test_conv1d_impl(int device_id, const float* x, int B, int Cin, int L, const float* w, const float* bias, int Cout,
                            int k, int stride, int pad, int dil, int transposed, int act, float slope, const float* alpha,
                            const float* norm, float* y, int Lout, int mode, const ConvTestExtra& ex, char* err,
                            size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(x && w && y && B > 0 && Cin > 0 && Cout > 0 && L > 0 && Lout > 0 && k > 0, "test_conv1d: bad argument");
        KX_HIP(hipSetDevice(device_id));
        DevMem dm;
        std::vector<int> lens(B, 1);
        // bit 8 of the mode: stage the input through a pre-split image (conv_f16x3_pre.hip), whatever the layer's row count
        const bool pre = (mode & 0x100) != 0;
        // bit 9: f16f8 -- the layer gets the 8-bit cross image of its weights (the S16 form's shapes then run the f16f8 kernel)
        const bool f8 = (mode & 0x200) != 0;
        // bits 10, 11: the 4 x 1 wave layout on the direct-A conv's 256-column tile too; no 16x16x32 form (ConvForce)
        const int force_bits = (mode & 0x400 ? kx::FORCE_DA_4X1 : 0) | (mode & 0x800 ? kx::FORCE_NO_S16 : 0);
        mode &= 0xff;
        KX_REQUIRE(mode >= kx::CONV_F32 && mode <= kx::CONV_F16X3_DA, "test_conv1d: mode must be 0, 1, 2 or 3");
        KX_REQUIRE(!pre || mode == kx::CONV_F16X3 || mode == kx::CONV_F16X3_DA, "test_conv1d: pre-split images exist for the direct-A kernels only");
        // row strides: the caller's dense rows, or (pad_ld) the model's: a multiple of 32 floats, input padding poisoned
        const int Ly = Lout + ex.up_off;  // columns of y (Lout: the conv's own output length)
        KX_REQUIRE(ex.up_off == 0 || (transposed && ex.up_off == 1), "test_conv1d: an output offset comes with transposed convs");
        KX_REQUIRE(stride >= 1 && (transposed || stride == 1 || (!ex.merged && !ex.in_up2 && !ex.tmajor)),
                   "test_conv1d: a strided conv takes no merged, in_up2 or time-major launch");
        KX_REQUIRE(!ex.view || !ex.tmajor, "test_conv1d: row-slice views of channel-major tensors only");
        // (time-major stores: a row of y is one column's Cout values; padded, it ends in a 32-float margin)
        const int yr = ex.tmajor ? Lout : Cout, yc = ex.tmajor ? Cout : Ly;  // rows per utterance and columns of y as stored
        const int x_ld = ex.pad_ld ? (L + 31) & ~31 : L;
        const int y_ld = ex.tmajor ? (ex.pad_ld ? ((Cout + 31) & ~31) + 32 : Cout) : (ex.pad_ld ? (Ly + 31) & ~31 : Ly);
        const int Lv = ex.in_up2 ? 2 * L : L;  // the input length the conv sees
        const bool want_stats = ex.stats_out != nullptr || ex.norm_out != nullptr;
        KX_REQUIRE(!ex.tmajor || (!transposed && !ex.resid && !ex.accum && !want_stats), "test_conv1d: time-major stores are plain stores");
        KX_REQUIRE(!ex.in_up2 || !transposed, "test_conv1d: in_up2 with plain convs only");
        KX_REQUIRE(!ex.merged || (!transposed && Lout == L), "test_conv1d: merged columns need input and output of one length");
        KX_REQUIRE((ex.norm_out != nullptr) == (ex.norm_gb != nullptr), "test_conv1d: norm planes come with gamma / beta");
        KX_REQUIRE(ex.act_shift >= -24 && ex.act_shift <= 24 && ex.prec1 >= 0 && ex.prec1 <= 2, "test_conv1d: bad act_shift / prec1");
        KX_REQUIRE(!transposed || (k == 2 * stride && pad == (k - stride) / 2 && dil == 1), "test_conv1d: transposed needs k=2s, pad=(k-s)/2");
        KX_REQUIRE(act != kx::ACT_SNAKE || alpha, "test_conv1d: snake needs alpha");
        const float poison = std::nanf(""), sentinel = -12345.5f;
        // per utterance: the input columns it stores and the output columns it owns (without the offset column)
        const int up = ex.in_up2 ? 2 : 1;
        const bool units = ex.len_mul_in > 0;
        std::vector<int> lin(B, L), lout(B, Lout);
        KX_REQUIRE(ex.len_mul_in >= 0 && (units || (!ex.len_add_in && !ex.len_mul_out && !ex.len_add_out)), "test_conv1d: bad length map");
        KX_REQUIRE(!units || (ex.lens && !ex.in_up2 && !ex.merged), "test_conv1d: length maps need lens, and no in_up2 or merged launch");
        if (ex.lens) {  // ragged batch
            KX_REQUIRE(units || (!transposed && stride == 1), "test_conv1d: ragged strided and transposed convs state their length maps");
            for (int b = 0; b < B; ++b) {
                if (units) {  // utterance b: lens[b] units; the output map must agree with the conv's own formula on the input count
                    KX_REQUIRE(ex.lens[b] >= 1 && ex.lens[b] <= L, "test_conv1d: lens out of range");
                    lin[b] = ex.lens[b] * ex.len_mul_in + ex.len_add_in;
                    lout[b] = ex.lens[b] * ex.len_mul_out + ex.len_add_out;
                    KX_REQUIRE(lin[b] >= 1 && lin[b] <= L, "test_conv1d: an utterance's input columns overrun L");
                    const int want = transposed ? stride * lin[b] : (lin[b] + 2 * pad - dil * (k - 1) - 1) / stride + 1;
                    KX_REQUIRE(lin[b] + 2 * pad - dil * (k - 1) - 1 >= 0 || transposed, "test_conv1d: lens out of range");
                    KX_REQUIRE(lout[b] == want && lout[b] >= 1 && lout[b] <= Lout, "test_conv1d: the output length map contradicts the conv's own output count");
                } else {  // utterance b is lens[b] columns long (stride-1 convs: the output shrinks by Lv - Lout)
                    KX_REQUIRE(ex.lens[b] >= 1 && ex.lens[b] <= L && up * ex.lens[b] + (Lout - Lv) >= 1, "test_conv1d: lens out of range");
                    lin[b] = ex.lens[b];
                    lout[b] = up * ex.lens[b] + (Lout - Lv);
                }
                lens[b] = ex.lens[b];
            }
        } else if (ex.merged)
            lens.assign(B, L);
        // A [B][C][len] host tensor as the launch sees it: rows of ld floats (view: VIEW_TOP foreign rows above each utterance's C rows,
        // VIEW_ROWS in all), with `fill` in the foreign rows, in [len, ld) and - own given - in the columns at or past own[b]; src null
        // = zeros.  GUARD floats follow.
        const int vrows = ex.view ? VIEW_ROWS : 0, vtop = ex.view ? VIEW_TOP : 0;
        auto stage = [&](const float* src, int C, int len, int ld, float fill, const int* own, int own_add) {
            std::vector<float> v((size_t)B * (C + vrows) * ld + GUARD, fill);
            for (int b = 0; b < B; ++b)
                for (int r = 0; r < C; ++r) {
                    float* d = &v[((size_t)b * (C + vrows) + vtop + r) * ld];
                    const int n = own ? std::min(len, own[b] + own_add) : len;
                    if (src)
                        std::memcpy(d, src + ((size_t)b * C + r) * len, (size_t)n * 4);
                    else
                        std::fill(d, d + n, 0.f);
                }
            std::fill(v.end() - GUARD, v.end(), GUARD_VALUE);
            return v;
        };
        auto guard_ok = [&](const float* d_end) {  // the GUARD floats behind a device buffer
            float g[GUARD];
            KX_HIP(hipMemcpy(g, d_end, sizeof g, hipMemcpyDeviceToHost));
            for (float f : g)
                if (f != GUARD_VALUE) return false;
            return true;
        };
        const kx::DevAlloc alloc = [&dm](size_t bytes) -> void* { return dm.get<unsigned char>(bytes); };

        // the layer: its weight images from the model's packers (conv_call.hip), bias and pre-scale as Model keeps them
        const float* dw = dm.up(w, (size_t)Cout * Cin * k);
        kx::ConvW cw = transposed ? kx::pack_convT(dw, Cin, Cout, stride, nullptr, alloc)
                                  : kx::pack_conv(kx::PackSrc{{dw, nullptr, nullptr}, {Cout, 0, 0}}, Cin, k, nullptr, alloc);
        cw.bias = bias ? dm.up(bias, (size_t)Cout) : nullptr;
        cw.act_shift = ex.act_shift;
        const int rows = cw.rows;
        if (f8 && mode != kx::CONV_F32) {
            kx::add_f8_image(cw, nullptr, alloc);
            KX_REQUIRE(cw.w8x, "test_conv1d: f16f8 images exist for the 128-row tiles of plain 3-, 7- and 11-tap convs");
        }
        if (ex.prec1 == 2 && mode != kx::CONV_F32) {
            kx::add_bf16_image(cw, nullptr, alloc);
            KX_REQUIRE(cw.w16b, "test_conv1d: bf16 images exist for 128-row tiles");
        }

        // the input and output views: dense = every utterance L columns ({lens, 0, L}), ragged = its own length.  A ragged call
        // poisons what an utterance does not own: NaN in its input and residual columns at or past its length, whatever the caller has
        // there; a strict one also starts its unowned output columns from the sentinel
        kx::T in, out, res;
        const std::vector<float> xp = stage(x, Cin, L, x_ld, poison, ex.lens ? lin.data() : nullptr, 0);
        const size_t x_n = xp.size() - GUARD;
        float* dx = dm.up(xp.data(), xp.size());
        in.p = dx + (size_t)vtop * x_ld;
        in.bs = (long)(Cin + vrows) * x_ld;
        in.ld = x_ld;
        in.C = Cin;
        in.Lmax = L;
        // (the merged kernels read the length array itself: a merged launch always carries real lengths)
        const bool ragged = ex.lens != nullptr || ex.merged;
        int* d_one = dm.up(lens.data(), B);
        // (the stored columns: in_up2 doubles them in the launch)
        in.len = units ? kx::LenMap{d_one, ex.len_mul_in, ex.len_add_in} : (ragged ? kx::LenMap{d_one, 1, 0} : kx::LenMap{d_one, 0, L});
        // y holds the running sum (accumulate) or zeros; the row padding holds a sentinel nobody may touch
        const std::vector<float> y0 = stage(ex.accum ? y : nullptr, yr, yc, y_ld, sentinel, ex.strict && ex.lens ? lout.data() : nullptr, ex.up_off);
        const size_t y_n = y0.size() - GUARD;
        float* dy = dm.up(y0.data(), y0.size());
        out.p = dy + (size_t)vtop * y_ld;
        out.bs = (long)(yr + vrows) * y_ld;
        out.ld = y_ld;
        out.C = rows;
        out.Lmax = Lout;
        const kx::LenMap own_len = units ? kx::LenMap{d_one, ex.len_mul_out, ex.len_add_out}
                                         : (ragged ? kx::LenMap{d_one, up, Lout - Lv} : kx::LenMap{d_one, 0, Lout});
        out.len = own_len;
        out.len.add += ex.up_off;  // (the stored columns of y; an up-scattering launch masks with o.up_len)

        kx::ConvOpts o;
        if (transposed) {  // the polyphase two-tap GEMM, scattered to the up-sampled axis
            o.pad = 1;
            o.store = kx::ST_UPSCATTER;
            o.up_pad = pad;
            o.up_off = ex.up_off;
            o.up_reflect = ex.up_reflect;
            o.up_len = own_len;
        } else {
            o.stride = stride;
            o.pad = pad;
            o.dil = dil;
            o.store = ex.tmajor ? kx::ST_TMAJOR : kx::ST_NORMAL;
        }
        if (norm) {
            const float* dn = dm.up(norm, (size_t)3 * B * Cin);
            o.nmean = dn;
            o.nscale = dn + (size_t)B * Cin;
            o.nshift = dn + (size_t)2 * B * Cin;
        }
        o.act = act;
        o.slope = slope;
        o.alpha = alpha ? dm.up(alpha, (size_t)Cin) : nullptr;
        o.in_up2 = ex.in_up2;
        o.epi = ex.epi;
        o.out_mul = ex.out_mul;
        o.out_div = ex.out_div;
        o.accum = ex.accum;
        float* d_res = nullptr;
        size_t r_n = 0;
        if (ex.resid) {
            // (laid out as y is: its own Ly columns, NaN behind them and past an utterance's own output)
            const std::vector<float> rp = stage(ex.resid, Cout, Ly, y_ld, poison, ex.lens ? lout.data() : nullptr, ex.up_off);
            r_n = rp.size() - GUARD;
            d_res = dm.up(rp.data(), rp.size());
            res.p = d_res + (size_t)vtop * y_ld;
            res.bs = (long)(Cout + vrows) * y_ld;
            res.ld = y_ld;
            o.resid = &res;
        }

        // the launch as the model assembles it: the hook's modes 2 and 3 are f16x3 with an override, prec1 is the f16 / bf16
        // mode inside its region
        kx::ConvCtx ctx;
        ctx.mode = mode == kx::CONV_F32 ? kx::CONV_F32
                                        : (ex.prec1 == 1 ? kx::CONV_F16 : (ex.prec1 == 2 ? kx::CONV_BF16 : (f8 ? kx::CONV_F16F8 : kx::CONV_F16X3)));
        ctx.p1_region = true;
        ctx.B = B;
        ctx.cus = mode == kx::CONV_F32 ? 0 : kx::conv16_cu_count();
        ctx.n_bs = norm ? Cin : 0;
        ctx.force = (mode == kx::CONV_F16X3_LDS ? kx::FORCE_LDS : (mode == kx::CONV_F16X3_DA ? kx::FORCE_DA : 0)) | force_bits;
        ctx.image = pre ? 2 : 0;
        ctx.epi_stream = ex.epi_stream;
        ctx.offer_merge = ex.merged != 0;
        ctx.flat = ex.flat != 0;
        ctx.stats = want_stats;
        kx::ConvCall call = kx::conv_call(cw, in, out, o, ctx);
        const kx::ConvPlan& plan = call.plan;
        const kx::ConvArgs& a = call.a;
        if (ex.plan_out) plan_fields(plan, ex.plan_out);
        float2* d_part = nullptr;
        size_t part_n = 0;
        if (want_stats) {
            KX_REQUIRE(!transposed && !ex.accum && plan.stat_cols > 0, "test_conv1d: fused statistics come with plain, non-accumulating stores");
            part_n = (size_t)B * rows * plan.stat_tiles;
            std::vector<float> p0(2 * part_n + GUARD, 0.f);
            std::fill(p0.end() - GUARD, p0.end(), GUARD_VALUE);
            d_part = reinterpret_cast<float2*>(dm.up(p0.data(), p0.size()));
            call.set_stats(d_part);
        }
        if (plan.flat_bn) {
            int* d_pre = dm.get<int>((size_t)B + 1);
            kx::launch_tile_prefix(call.flat_len(), call.flat_extra(), plan.flat_bn, B, d_pre, nullptr);
            call.set_flat(d_pre, kx::conv_tile_count(lens.data(), B, call.flat_len(), call.flat_extra(), plan.flat_bn));
        }
        if (pre) {
            KX_REQUIRE(plan.pre, "test_conv1d: this layer has no pre-split form");
            const long img_bs = (long)call.image_bytes();
            unsigned char* img = dm.get<unsigned char>((size_t)B * img_bs);
            KX_HIP(hipMemset(img, 0xff, (size_t)B * img_bs));  // (NaN halves wherever the pass does not write)
            kx::launch_split_image(a, B, L, img, img_bs, nullptr);
            call.set_image(img, img_bs);
        }
        kx::launch_conv(plan, a, B, nullptr);
        KX_HIP(hipDeviceSynchronize());
        {
            std::vector<float> yp(y_n);
            KX_HIP(hipMemcpy(yp.data(), dy, y_n * 4, hipMemcpyDeviceToHost));
            for (int b = 0; b < B; ++b)
                for (int r = 0; r < yr + vrows; ++r) {
                    const float* row = &yp[((size_t)b * (yr + vrows) + r) * y_ld];
                    const bool foreign = r < vtop || r >= vtop + yr;
                    if (!foreign) std::memcpy(y + ((size_t)b * yr + (r - vtop)) * yc, row, (size_t)yc * 4);
                    for (int c = foreign ? 0 : yc; c < y_ld; ++c)
                        if (row[c] != sentinel)
                            throw Error(KX_ERR_STATE, foreign ? "test_conv1d: the kernel wrote into a foreign row of the output tensor"
                                                              : "test_conv1d: the kernel wrote into the row padding");
                }
        }
        if (ex.strict) {
            const bool ok = guard_ok(dx + x_n) && guard_ok(dy + y_n) && (!d_res || guard_ok(d_res + r_n)) &&
                            (!d_part || guard_ok(reinterpret_cast<const float*>(d_part) + 2 * part_n));
            if (!ok) throw Error(KX_ERR_STATE, "test_conv1d: the guard bytes behind a buffer changed");
        }
        if (ex.norm_out) {  // the model's route from the partial sums to the next conv's AdaIN planes (Model::stats)
            const float* d_gb = dm.up(ex.norm_gb, (size_t)B * 2 * rows);
            float* d_pl = dm.get<float>((size_t)3 * B * rows);
            kx::launch_stats_finalize(d_part, a.stat_tiles, plan.stat_cols, rows, a.out_len, B, d_gb, 2L * rows, d_pl, d_pl + (size_t)B * rows,
                                      d_pl + (size_t)2 * B * rows, rows, nullptr);
            KX_HIP(hipDeviceSynchronize());
            KX_HIP(hipMemcpy(ex.norm_out, d_pl, (size_t)3 * B * rows * 4, hipMemcpyDeviceToHost));
        }
        if (ex.stats_out) {
            std::vector<float2> part((size_t)B * rows * a.stat_tiles);
            KX_HIP(hipMemcpy(part.data(), d_part, part.size() * sizeof(float2), hipMemcpyDeviceToHost));
            for (size_t br = 0; br < (size_t)B * rows; ++br) {
                // (the tiles of the row's own output columns: a ragged row's later slots are never written)
                const int used = (lout[br / rows] + plan.stat_cols - 1) / plan.stat_cols;
                double sm = 0.0, sq = 0.0;
                for (int t = 0; t < used && t < a.stat_tiles; ++t) {
                    sm += part[br * a.stat_tiles + t].x;
                    sq += part[br * a.stat_tiles + t].y;
                }
                ex.stats_out[2 * br] = (float)sm;
                ex.stats_out[2 * br + 1] = (float)sq;
            }
        }
    });
}

int kx_test_conv1d(int device_id, const float* x, int B, int Cin, int L, const float* w, const float* bias, int Cout,
                   int k, int stride, int pad, int dil, int transposed, int act, float slope, const float* alpha,
                   const float* norm, float* y, int Lout, int mode, char* err, size_t err_len) {
    return test_conv1d_impl(device_id, x, B, Cin, L, w, bias, Cout, k, stride, pad, dil, transposed, act, slope, alpha, norm,
                            y, Lout, mode, ConvTestExtra{}, err, err_len);
}

int kx_test_conv_transpose(int device_id, const float* x, int B, int Cin, int L, const float* w, const float* bias, int Cout,
                           int stride, int act, float slope, const float* resid, int up_off, float* y, int mode, char* err,
                           size_t err_len) {
    ConvTestExtra ex;
    ex.resid = resid;
    ex.up_off = up_off ? 1 : 0;
    ex.up_reflect = up_off ? 1 : 0;
    const int k = 2 * stride, pad = (k - stride) / 2;
    const int Lout = (L - 1) * stride - 2 * pad + k;
    return test_conv1d_impl(device_id, x, B, Cin, L, w, bias, Cout, k, stride, pad, 1, 1, act, slope, nullptr, nullptr, y, Lout, mode, ex,
                            err, err_len);
}

int kx_test_conv1d_epilogue(int device_id, const float* x, int B, int Cin, int L, const float* w, const float* bias,
                            int Cout, int k, int pad, int dil, const float* resid, int accumulate, float out_mul,
                            float out_div, float* y, float* stats_out, int mode, char* err, size_t err_len) {
    ConvTestExtra ex;
    ex.resid = resid;
    ex.accum = accumulate;
    ex.out_mul = out_mul;
    ex.out_div = out_div;
    ex.stats_out = stats_out;
    const int Lout = L + 2 * pad - dil * (k - 1);
    return test_conv1d_impl(device_id, x, B, Cin, L, w, bias, Cout, k, 1, pad, dil, 0, 0, 0.f, nullptr, nullptr, y, Lout, mode,
                            ex, err, err_len);
}

int kx_test_conv1d_full(int device_id, const float* x, int B, int Cin, int L, const int32_t* lens, int pad_ld, const float* w,
                        const float* bias, int Cout, int k, int pad, int dil, int act, float slope, const float* alpha,
                        const float* norm, const float* resid, int accumulate, float out_mul, float out_div, float* y,
                        float* stats_out, int mode, char* err, size_t err_len) {
    ConvTestExtra ex;
    ex.resid = resid;
    ex.accum = accumulate;
    ex.out_mul = out_mul;
    ex.out_div = out_div;
    ex.stats_out = stats_out;
    ex.lens = lens;
    ex.pad_ld = pad_ld & 1;
    ex.flat = (pad_ld >> 1) & 1;
    const int Lout = L + 2 * pad - dil * (k - 1);
    return test_conv1d_impl(device_id, x, B, Cin, L, w, bias, Cout, k, 1, pad, dil, 0, act, slope, alpha, norm, y, Lout, mode, ex,
                            err, err_len);
}

int kx_test_conv1d_opts(int device_id, const float* x, int B, int Cin, int L, const int32_t* lens, int pad_ld, const float* w,
                        const float* bias, int Cout, int k, int pad, int dil, int act, float slope, const float* alpha,
                        const float* norm, const float* resid, int accumulate, float out_mul, float out_div, float* y,
                        float* stats_out, int mode, const int32_t* opts, int n_opts, const float* norm_gb, float* norm_out,
                        int64_t* plan_out, char* err, size_t err_len) {
    ConvTestExtra ex;
    if (!opts || (n_opts != 8 && n_opts != 15) || !plan_out || opts[7] < 0)
        return guarded_free(err, err_len, [] { throw Error(KX_ERR_INVALID, "test_conv1d_opts: 8 or 15 options in, 17 plan fields out"); });
    ex.resid = resid;
    ex.accum = accumulate;
    ex.out_mul = out_mul;
    ex.out_div = out_div;
    ex.stats_out = stats_out;
    ex.lens = lens;
    ex.pad_ld = pad_ld & 1;
    ex.flat = (pad_ld >> 1) & 1;
    ex.in_up2 = opts[0] != 0;
    ex.epi = opts[1];
    ex.merged = opts[2] != 0;
    ex.tmajor = opts[3] != 0;
    ex.prec1 = opts[4];
    ex.act_shift = opts[5];
    ex.epi_stream = opts[6] != 0;
    ex.norm_gb = norm_gb;
    ex.norm_out = norm_out;
    ex.plan_out = plan_out;
    int stride = 1;
    if (n_opts == 15) {
        stride = opts[8];
        ex.len_mul_in = opts[9];
        ex.len_add_in = opts[10];
        ex.len_mul_out = opts[11];
        ex.len_add_out = opts[12];
        ex.up_off = ex.up_reflect = opts[13] != 0;
        ex.view = opts[14] != 0;
        ex.strict = stride != 1 || ex.len_mul_in || ex.len_add_in || ex.len_mul_out || ex.len_add_out || ex.up_off || ex.view;
        if (stride < 1 || (stride > 1 && opts[7]))
            return guarded_free(err, err_len, [] { throw Error(KX_ERR_INVALID, "test_conv1d_opts: stride >= 1, with plain convs only"); });
    }
    if (const int s = opts[7]) {  // a polyphase transposed conv (kx_test_conv_transpose: k = 2 s, pad = s / 2, w [Cin,Cout,k]) with these options
        const int pd = (k - s) / 2;
        return test_conv1d_impl(device_id, x, B, Cin, L, w, bias, Cout, k, s, pd, 1, 1, act, slope, alpha, norm, y, (L - 1) * s - 2 * pd + k,
                                mode, ex, err, err_len);
    }
    const int Lout = ((ex.in_up2 ? 2 * L : L) + 2 * pad - dil * (k - 1) - 1) / stride + 1;
    return test_conv1d_impl(device_id, x, B, Cin, L, w, bias, Cout, k, stride, pad, dil, 0, act, slope, alpha, norm, y, Lout, mode, ex,
                            err, err_len);
}

int kx_test_layernorm(int device_id, const float* x, int B, int C, int T, const int32_t* lens, float eps, int mode, const float* g,
                      const float* be, float leaky, float* y, char* err, size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(x && y && lens && B > 0 && C > 0 && T > 0 && mode >= kx::LN_PLAIN && mode <= kx::LN_ADA, "test_layernorm: bad argument");
        KX_REQUIRE(mode == kx::LN_PLAIN || (g && be), "test_layernorm: the affine forms need gamma and beta");
        for (int b = 0; b < B; ++b) KX_REQUIRE(lens[b] >= 1 && lens[b] <= T, "test_layernorm: lens out of range");
        KX_HIP(hipSetDevice(device_id));
        DevMem dm;
        const int ld = (T + 31) & ~31;  // rows padded as in the model; the input padding is NaN, the output holds a sentinel throughout
        const float sentinel = -12345.5f;
        std::vector<float> xp((size_t)B * C * ld, std::nanf(""));
        for (size_t r = 0; r < (size_t)B * C; ++r) std::memcpy(&xp[r * ld], x + r * T, (size_t)T * 4);
        const float* dx = dm.up(xp.data(), xp.size());
        std::vector<float> yp((size_t)B * C * ld, sentinel);
        float* dy = dm.up(yp.data(), yp.size());
        const int* d_len = dm.up(lens, B);
        const size_t ng = mode == kx::LN_ADA ? (size_t)B * C : (size_t)C;
        const float* dg = mode == kx::LN_PLAIN ? nullptr : dm.up(g, ng);
        const float* db = mode == kx::LN_PLAIN ? nullptr : dm.up(be, ng);
        kx::launch_layernorm_ch(dx, dy, (long)C * ld, ld, C, kx::LenMap{d_len, 1, 0}, B, T, eps, mode, dg, db, C, leaky, nullptr);
        KX_HIP(hipDeviceSynchronize());
        KX_HIP(hipMemcpy(yp.data(), dy, yp.size() * 4, hipMemcpyDeviceToHost));
        for (size_t r = 0; r < (size_t)B * C; ++r) {
            std::memcpy(y + r * T, &yp[r * ld], (size_t)T * 4);  // (columns past lens[b] come back as the sentinel: the caller checks them)
            for (int c = T; c < ld; ++c)
                if (yp[r * ld + c] != sentinel) throw Error(KX_ERR_STATE, "test_layernorm: the kernel wrote into the row padding");
        }
    });
}

int kx_test_instance_norm(int device_id, const float* x, int B, int C, int L, const int32_t* lens, const float* gb, float* out,
                          char* err, size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(x && lens && gb && out && B > 0 && C > 0 && L > 0, "test_instance_norm: bad argument");
        for (int b = 0; b < B; ++b) KX_REQUIRE(lens[b] >= 1 && lens[b] <= L, "test_instance_norm: lens out of range");
        KX_HIP(hipSetDevice(device_id));
        DevMem dm;
        const int ld = (L + 31) & ~31;
        std::vector<float> xp((size_t)B * C * ld, std::nanf(""));
        for (size_t r = 0; r < (size_t)B * C; ++r) std::memcpy(&xp[r * ld], x + r * L, (size_t)L * 4);
        const float* dx = dm.up(xp.data(), xp.size());
        const int* d_len = dm.up(lens, B);
        const float* d_gb = dm.up(gb, (size_t)B * 2 * C);
        const size_t n = (size_t)B * C;
        float* pl = dm.get<float>(9 * n);
        float2* raw = dm.get<float2>(2 * n);
        const kx::LenMap lm{d_len, 1, 0};
        // out[0]: the pass alone; out[1]: the pass that also leaves its raw sums (Model::stats, first AdaIN of a tensor); out[2]: those
        // raw sums finalized (its later AdaINs)
        kx::launch_in_stats(dx, (long)C * ld, ld, C, lm, B, d_gb, 2L * C, pl, pl + n, pl + 2 * n, C, nullptr, nullptr);
        kx::launch_in_stats(dx, (long)C * ld, ld, C, lm, B, d_gb, 2L * C, pl + 3 * n, pl + 4 * n, pl + 5 * n, C, raw, nullptr);
        kx::launch_stats_finalize(raw, 2, kx::STAT_RAW_TILES, C, lm, B, d_gb, 2L * C, pl + 6 * n, pl + 7 * n, pl + 8 * n, C, nullptr);
        KX_HIP(hipDeviceSynchronize());
        KX_HIP(hipMemcpy(out, pl, 9 * n * 4, hipMemcpyDeviceToHost));
    });
}

int kx_test_conv_plan(const int64_t* in, int n_in, int64_t* out, int n_out, char* err, size_t err_len) {
    return guarded_free(err, err_len, [&] {
        KX_REQUIRE(in && out && n_in == 25 && n_out == 17, "test_conv_plan: 25 launch fields in, 17 plan fields out");
        kx::ConvLaunch c{};
        int* f[] = {&c.mode, &c.prec1, &c.f8, &c.BM, &c.rows, &c.n_chunks16, &c.K, &c.dil, &c.stride, &c.pad, &c.act, &c.in_up2,
                    &c.store, &c.accum, &c.epi, &c.norm, &c.stats, &c.image, &c.merge_T};
        for (int i = 0; i < 19; ++i) *f[i] = (int)in[i];
        c.x_bs = (long)in[19];
        c.x_ld = (int)in[20];
        c.B = (int)in[21];
        c.cols = (int)in[22];
        c.cus = (int)in[23];
        c.force = (int)in[24];
        plan_fields(kx::conv_plan(c), out);
    });
}

int kx_test_lstm(int device_id, const float* x, int B, int L, int n_in, const float* w_ih, const float* w_hh,
                 const float* b_ih, const float* b_hh, const float* w_ih_r, const float* w_hh_r, const float* b_ih_r,
                 const float* b_hh_r, float* y, char* err, size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(x && y && B > 0 && L > 0 && n_in > 0, "test_lstm: bad argument");
        KX_HIP(hipSetDevice(device_id));
        DevMem dm;
        std::vector<float> xc((size_t)B * n_in * L);  // [B,L,n_in] -> channel-major [B][n_in][L]
        for (int b = 0; b < B; ++b)
            for (int t = 0; t < L; ++t)
                for (int c = 0; c < n_in; ++c) xc[((size_t)b * n_in + c) * L + t] = x[((size_t)b * L + t) * n_in + c];
        std::vector<int> lens(B, L);
        int* d_len = dm.up(lens.data(), B);
        // the input GEMM's weights as Model::make_lstm packs them; launched here on the f32 kernel, which is what this test pins
        const kx::DevAlloc alloc = [&dm](size_t bytes) -> void* { return dm.get<unsigned char>(bytes); };
        const kx::PackSrc src{{dm.up(w_ih, (size_t)1024 * n_in), dm.up(w_ih_r, (size_t)1024 * n_in), nullptr}, {1024, 1024, 0}};
        const kx::ConvW ih = kx::pack_conv(src, n_in, 1, nullptr, alloc);
        float* bias = dm.get<float>(2048);
        kx::launch_vec_add(dm.up(b_ih, 1024), dm.up(b_hh, 1024), bias, 1024, nullptr);
        kx::launch_vec_add(dm.up(b_ih_r, 1024), dm.up(b_hh_r, 1024), bias + 1024, 1024, nullptr);
        float* whhT = dm.get<float>(2 * 256 * 1024);
        kx::launch_transpose_whh(dm.up(w_hh, 1024 * 256), whhT, nullptr);
        kx::launch_transpose_whh(dm.up(w_hh_r, 1024 * 256), whhT + 256 * 1024, nullptr);
        float* gx = dm.get<float>((size_t)B * L * 2048);
        kx::ConvArgs a{};
        a.x = dm.up(xc.data(), xc.size());
        a.x_bs = (long)n_in * L;
        a.x_ld = L;
        a.Cin = n_in;
        a.in_len = kx::LenMap{d_len, 1, 0};
        a.out_len = a.in_len;
        a.n_chunks = ih.n_chunks;
        a.w = ih.w;
        a.bias = bias;
        a.K = 1; a.dil = 1; a.stride = 1; a.pad = 0;
        a.Cout = ih.rows;
        a.y = gx;
        a.y_bs = (long)L * 2048;
        a.y_ld = 2048;
        a.out_mul = 1.f; a.out_div = 1.f;
        a.store = kx::ST_TMAJOR;
        a.up_cout = 1;
        kx::launch_conv1d(a, ih.BM, B, L, nullptr);
        float* dy = dm.get<float>((size_t)B * 512 * L);
        // (the hook runs the product's two-CU recurrence: exchange buffer + sticky error word as Model holds them)
        unsigned long long* xchg = dm.get<unsigned long long>(kx::lstm_exchange_bytes(B) / sizeof(unsigned long long));
        KX_HIP(hipMemset(xchg, 0, kx::lstm_exchange_bytes(B)));
        unsigned* errw = dm.get<unsigned>(1);
        KX_HIP(hipMemset(errw, 0, sizeof(unsigned)));
        kx::launch_lstm(gx, (long)L * 2048, 2048, whhT, dy, (long)512 * L, L, kx::LenMap{d_len, 1, 0}, B, xchg, errw, nullptr);
        KX_HIP(hipDeviceSynchronize());
        unsigned herr = 0;
        KX_HIP(hipMemcpy(&herr, errw, sizeof(unsigned), hipMemcpyDeviceToHost));
        if (herr) throw Error(KX_ERR_DEVICE, "test_lstm: the two-CU recurrence timed out waiting for its partner");
        KX_HIP(hipDeviceSynchronize());
        std::vector<float> yc((size_t)B * 512 * L);
        KX_HIP(hipMemcpy(yc.data(), dy, yc.size() * 4, hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b)
            for (int c = 0; c < 512; ++c)
                for (int t = 0; t < L; ++t) y[((size_t)b * L + t) * 512 + c] = yc[((size_t)b * 512 + c) * L + t];
    });
}

int kx_test_attention(int device_id, const float* qkv, const int32_t* lens, int B, int T, float* ctx, char* err,
                      size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(qkv && lens && ctx && B > 0 && T > 0 && T <= 512, "test_attention: bad argument");
        for (int b = 0; b < B; ++b) KX_REQUIRE(lens[b] >= 1 && lens[b] <= T, "test_attention: lens out of range");
        KX_HIP(hipSetDevice(device_id));
        DevMem dm;
        const int ld = (T + 31) & ~31;  // rows padded as in the model (128-byte lines)
        std::vector<float> q((size_t)B * 2304 * ld, std::nanf(""));  // padding holds NaNs: the kernel must not use it
        for (int b = 0; b < B; ++b)
            for (int c = 0; c < 2304; ++c)
                std::memcpy(&q[((size_t)b * 2304 + c) * ld], &qkv[((size_t)b * 2304 + c) * T], (size_t)T * 4);
        const float* d_q = dm.up(q.data(), q.size());
        const int* d_len = dm.up(lens, B);
        float* d_ctx = dm.get<float>((size_t)B * 768 * ld);
        KX_HIP(hipMemset(d_ctx, 0, (size_t)B * 768 * ld * 4));
        kx::launch_attention(d_q, (long)2304 * ld, ld, d_ctx, (long)768 * ld, ld, d_len, B, T, nullptr);
        KX_HIP(hipDeviceSynchronize());
        std::vector<float> c((size_t)B * 768 * ld);
        KX_HIP(hipMemcpy(c.data(), d_ctx, c.size() * 4, hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b)
            for (int r = 0; r < 768; ++r)
                std::memcpy(&ctx[((size_t)b * 768 + r) * T], &c[((size_t)b * 768 + r) * ld], (size_t)T * 4);
    });
}

int kx_test_source(int device_id, const float* f0, int B, int F2, const float* lin_w, float lin_b, uint64_t seed,
                   uint64_t utt_base, int noise_off, float* out, char* err, size_t err_len) {
    // every row its full length: the ragged hook with frames[b] = F2 / 2 (nothing of `out` is left as the sentinel)
    if (!(B > 0 && B <= 64 && F2 > 0 && (F2 % 2) == 0))
        return guarded_free(err, err_len, [] { throw Error(KX_ERR_INVALID, "test_source: bad argument"); });
    const std::vector<int32_t> fr((size_t)B, F2 / 2);
    return kx_test_source_ragged(device_id, f0, fr.data(), B, F2 / 2, lin_w, lin_b, seed, utt_base, nullptr, nullptr, noise_off, out, err,
                                 err_len);
}

int kx_test_output_plan(int device_id, const float* audio, int B, int64_t audio_ld, const int32_t* frames_in, const int32_t* dur,
                        const int32_t* lens, const int32_t* chunks_per_request, int R, const int32_t* formats, const kx_join* joins,
                        const uint8_t* want, void* out, int64_t out_cap, int64_t* out_bytes, int64_t* out_samples,
                        int64_t* out_marks, int64_t marks_cap, int64_t* out_n_marks, char* err, size_t err_len) {
    return kx_test_output_plan_levelled(device_id, audio, B, audio_ld, frames_in, dur, lens, chunks_per_request, R, formats, joins, want,
                                        out, out_cap, out_bytes, out_samples, out_marks, marks_cap, out_n_marks, nullptr, nullptr, err,
                                        err_len);
}

int kx_test_output_plan_levelled(int device_id, const float* audio, int B, int64_t audio_ld, const int32_t* frames_in,
                                 const int32_t* dur, const int32_t* lens, const int32_t* chunks_per_request, int R,
                                 const int32_t* formats, const kx_join* joins, const uint8_t* want, void* out, int64_t out_cap,
                                 int64_t* out_bytes, int64_t* out_samples, int64_t* out_marks, int64_t marks_cap,
                                 int64_t* out_n_marks, const kx_level* levels, double* out_levels, char* err, size_t err_len) {
    return kx_test_output_plan_loudness(device_id, audio, B, audio_ld, frames_in, dur, lens, chunks_per_request, R, formats, joins, want,
                                        out, out_cap, out_bytes, out_samples, out_marks, marks_cap, out_n_marks, levels, out_levels,
                                        nullptr, nullptr, nullptr, 0, nullptr, err, err_len);
}

int kx_test_output_plan_loudness(int device_id, const float* audio, int B, int64_t audio_ld, const int32_t* frames_in,
                                 const int32_t* dur, const int32_t* lens, const int32_t* chunks_per_request, int R,
                                 const int32_t* formats, const kx_join* joins, const uint8_t* want, void* out, int64_t out_cap,
                                 int64_t* out_bytes, int64_t* out_samples, int64_t* out_marks, int64_t marks_cap,
                                 int64_t* out_n_marks, const kx_level* levels, double* out_levels, const kx_loudness* loudness,
                                 double* out_loudness, double* out_hops, int64_t hops_cap, int64_t* out_n_hops, char* err,
                                 size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(formats && out_bytes && out_samples && out_n_marks && B > 0 && R > 0 && (frames_in ? !dur : dur && lens) &&
                       ((!want && !joins) || dur) && (audio ? out != nullptr : out_cap == 0 && dur) && (levels ? audio && out_levels : !out_levels) &&
                       (loudness ? audio && out_loudness && out_hops && out_n_hops && hops_cap >= 0 : !out_loudness && !out_hops && !out_n_hops),
                   "test_output_plan: bad argument");
        // what the forward would have brought back: the rows' frame counts and the durations of their two edge tokens
        std::vector<int> frames((size_t)B, 0), edges((size_t)2 * B, 0);
        for (int b = 0; b < B; ++b) {
            long f = frames_in ? frames_in[b] : 0;
            if (dur) {
                KX_REQUIRE(lens[b] >= 1 && lens[b] <= 512, "test_output_plan: lens out of range");
                for (int t = 0; t < lens[b]; ++t) {
                    KX_REQUIRE(dur[(size_t)b * 512 + t] >= 0, "test_output_plan: negative duration");
                    f += dur[(size_t)b * 512 + t];
                }
                edges[(size_t)2 * b] = dur[(size_t)b * 512];
                edges[(size_t)2 * b + 1] = dur[(size_t)b * 512 + lens[b] - 1];
            }
            KX_REQUIRE(f >= 0 && f <= 0x7FFFFFFF / 600 && (!audio || 600L * f <= audio_ld), "test_output_plan: a row is shorter than its frames");
            frames[(size_t)b] = (int)f;
        }
        static_assert(sizeof(kx_join) == sizeof(kx::JoinSpec), "kx_join is JoinSpec");
        const kx::JoinSpec* specs = reinterpret_cast<const kx::JoinSpec*>(joins);
        for (int r = 0; joins && r < R; ++r) KX_REQUIRE(kx::join_spec_ok(specs[r]), "infer: bad join");
        static_assert(sizeof(kx_level) == sizeof(kx::LevelSpec), "kx_level is LevelSpec");
        const kx::LevelSpec* lspecs = reinterpret_cast<const kx::LevelSpec*>(levels);
        for (int r = 0; levels && r < R; ++r) KX_REQUIRE(kx::level_spec_ok(lspecs[r]), "infer: bad level");
        // (a loudness spec of mode 0xFFFFFFFF: that request is not metered, as a plain request beside metered ones in a batch)
        static_assert(sizeof(kx_loudness) == sizeof(kx::LoudSpec), "kx_loudness is LoudSpec");
        const kx::LoudSpec* dspecs = reinterpret_cast<const kx::LoudSpec*>(loudness);
        for (int r = 0; loudness && r < R; ++r)
            KX_REQUIRE(dspecs[r].mode == kx::LOUD_NONE || kx::loud_spec_ok(dspecs[r]), "infer: bad loudness");
        // the planner and the launcher of Model::infer_host_once
        const kx::RequestLayout layout{chunks_per_request, R, formats, R, want, specs, R, lspecs, levels ? R : 0, dspecs, loudness ? R : 0};
        kx::OutputPlan plan;
        kx::build_output_plan(frames.data(), lens, joins ? edges.data() : nullptr, B, layout, plan);
        for (int r = 0; r < R; ++r) {
            out_bytes[r] = plan.req[(size_t)r].out_bytes;
            out_samples[r] = plan.req[(size_t)r].n_samples;
            out_n_marks[r] = plan.count[(size_t)r];
            if (loudness) {
                const bool on = dspecs[r].mode != kx::LOUD_NONE;
                out_n_hops[r] = on ? plan.req[(size_t)r].n_samples / kx::loud_hop(plan.req[(size_t)r].rate) : 0;
            }
        }
        KX_REQUIRE(!loudness || plan.max_hops <= hops_cap, "test_output_plan: hops_cap is too small");
        KX_REQUIRE(plan.n_marks <= marks_cap && (plan.n_marks == 0 || out_marks), "test_output_plan: marks_cap is too small");
        KX_REQUIRE(!audio || plan.total_bytes <= out_cap, "test_output_plan: out_cap is too small");
        if (!audio && plan.n_marks == 0) return;
        KX_HIP(hipSetDevice(device_id));
        DevMem dm;
        // the partials of the peak pass: poisoned with a large finite value (an entry the launch did not write must not be read),
        // 64 bytes of sentinel behind them
        const size_t n_peak = (size_t)plan.peak_dwords();
        uint32_t* d_peak = plan.measured ? dm.get<uint32_t>(n_peak + 16) : nullptr;
        if (d_peak) {
            KX_HIP(hipMemset(d_peak, 0x7F, n_peak * 4));
            KX_HIP(hipMemset(d_peak + n_peak, 0xA5, 64));
        }
        // the true-peak partials: poisoned and guarded like the first table
        const size_t n_tpeak = (size_t)plan.truepeak_dwords();
        uint32_t* d_tpeak = plan.true_peak ? dm.get<uint32_t>(n_tpeak + 16) : nullptr;
        if (d_tpeak) {
            KX_HIP(hipMemset(d_tpeak, 0x7F, n_tpeak * 4));
            KX_HIP(hipMemset(d_tpeak + n_tpeak, 0xA5, 64));
        }
        // the hop energies of the meter: poisoned with NaNs (an entry the launch did not write must not be read), a sentinel behind them
        const size_t n_hop = (size_t)plan.hop_doubles();
        double* d_hops = loudness ? dm.get<double>(n_hop + 8) : nullptr;
        if (d_hops) {
            KX_HIP(hipMemset(d_hops, 0xFF, n_hop * 8));
            KX_HIP(hipMemset(d_hops + n_hop, 0xA5, 64));
        }
        const kx::OutputTables tables{dm.get<kx::PackReq>((size_t)R), dm.get<long>((size_t)B + 1), dm.get<kx::JoinRow>((size_t)B),
                                      dm.get<kx::MarkRow>((size_t)B), plan.measured ? dm.get<kx::LevelSpec>((size_t)R) : nullptr, d_peak,
                                      loudness ? dm.get<kx::LoudSpec>((size_t)R) : nullptr, d_hops,
                                      loudness ? dm.get<double>((size_t)4 * kx::LOUD_POWERS * 16) : nullptr, d_tpeak};
        const int* d_dur = dur ? dm.up(dur, (size_t)B * 512) : nullptr;
        const int* d_len = dur ? dm.up(lens, (size_t)B) : nullptr;
        // sentinels: 64 bytes after the last region, after the resampled streams, after the last mark and after the levels, which
        // the kernels must leave alone.  The marks block is moved 64 bytes back for the first of them, the levels block 64 more
        // for the third (the kernels are handed the addresses, still 8-aligned; the offsets themselves are nothing they see).
        // (the loudness block stays right behind the levels: the two count as one here)
        const long body = audio ? plan.total_bytes : 0, n_mk = plan.n_marks * 8, n_lv = plan.measured ? (loudness ? 32L : 16L) * R : 0;
        if (audio) plan.marks_off += 64;
        if (plan.measured) plan.levels_off += 128;
        if (loudness) plan.loud_off = plan.levels_off + 16L * R;
        const long mk_off = audio ? plan.marks_off : 0, lv_off = plan.measured ? plan.levels_off : mk_off + n_mk;
        const long d_out_bytes = plan.measured ? lv_off + n_lv + 64 : mk_off + n_mk + 64;
        char* d_out = dm.get<char>((size_t)d_out_bytes);
        KX_HIP(hipMemset(d_out, 0xA5, (size_t)d_out_bytes));
        float* d_y = audio && plan.y_floats > 0 ? dm.get<float>((size_t)plan.y_floats + 16) : nullptr;
        if (d_y) KX_HIP(hipMemset(d_y + plan.y_floats, 0xA5, 64));
        if (audio) {
            const float* d_audio = dm.up(audio, (size_t)B * (size_t)audio_ld);
            kx::launch_output_plan(d_audio, (long)audio_ld, d_dur, d_len, plan, tables, d_y, d_out, nullptr);
        } else {  // (the marks alone: no audio is read, no body written)
            kx::launch_token_marks(d_dur, d_len, plan, tables, d_out, nullptr);
        }
        KX_HIP(hipDeviceSynchronize());
        std::vector<unsigned char> tail(64);
        auto untouched = [&](const void* d_at, const char* what) {
            KX_HIP(hipMemcpy(tail.data(), d_at, 64, hipMemcpyDeviceToHost));
            for (unsigned char c : tail) KX_REQUIRE(c == 0xA5, what);
        };
        if (audio) {
            KX_HIP(hipMemcpy(out, d_out, (size_t)body, hipMemcpyDeviceToHost));
            untouched(d_out + body, "test_output_plan: the kernel wrote past the last region");
            if (d_y) untouched(d_y + plan.y_floats, "test_output_plan: the resampler wrote past the last stream");
        }
        if (plan.measured) {
            std::vector<double> lv((size_t)n_lv / 8);
            KX_HIP(hipMemcpy(lv.data(), d_out + lv_off, (size_t)n_lv, hipMemcpyDeviceToHost));
            if (out_levels) std::memcpy(out_levels, lv.data(), (size_t)R * 16);
            if (loudness) {
                for (int r = 0; r < R; ++r) {  // {f64(p), g} of the levels block, {I, n_g} of the loudness block
                    std::memcpy(out_loudness + 4 * r, &lv[(size_t)2 * r], 16);
                    std::memcpy(out_loudness + 4 * r + 2, &lv[(size_t)2 * R + 2 * r], 16);
                }
                // [R][hops_cap]: the first out_n_hops[r] entries of row r are the e[k] the meter stored
                for (int r = 0; r < R; ++r)
                    if (out_n_hops[r] > 0)
                        KX_HIP(hipMemcpy(out_hops + (size_t)r * hops_cap, d_hops + (size_t)r * plan.max_hops, (size_t)out_n_hops[r] * 8,
                                         hipMemcpyDeviceToHost));
                untouched(d_hops + n_hop, "test_output_plan: the meter wrote past its table");
            }
            untouched(d_out + lv_off - 64, "test_output_plan: a kernel wrote in front of the levels");
            untouched(d_out + lv_off + n_lv, "test_output_plan: the kernel wrote past the last level");
            untouched(d_peak + n_peak, "test_output_plan: the peak pass wrote past its table");
            if (d_tpeak) untouched(d_tpeak + n_tpeak, "test_output_plan: the true-peak pass wrote past its table");
        }
        if (plan.n_marks == 0) return;
        KX_HIP(hipMemcpy(out_marks, d_out + mk_off, (size_t)n_mk, hipMemcpyDeviceToHost));
        untouched(d_out + mk_off + n_mk, "test_output_plan: the kernel wrote past the last mark");
    });
}

// ---- the token-axis kernels of Model::front_half ---------------------------------------------------------------------------------
namespace {
constexpr float FRONT_SENTINEL = -12345.5f;
inline int pad32(int x) { return (x + 31) & ~31; }
// [rows][len] -> [rows][ld], the padding filled
void padded_rows(const float* src, size_t rows, int len, int ld, float fill, std::vector<float>& v) {
    v.assign(rows * ld, fill);
    for (size_t r = 0; r < rows; ++r) std::memcpy(&v[r * ld], src + r * len, (size_t)len * 4);
}
// [rows][ld] on the device -> [rows][len] on the host; the padding of every row must still hold the sentinel
void unpad_rows(const float* d_src, size_t rows, int len, int ld, float* dst, const char* what) {
    std::vector<float> v(rows * ld);
    KX_HIP(hipMemcpy(v.data(), d_src, v.size() * 4, hipMemcpyDeviceToHost));
    for (size_t r = 0; r < rows; ++r) {
        std::memcpy(dst + r * len, &v[r * ld], (size_t)len * 4);
        for (int c = len; c < ld; ++c)
            if (v[r * ld + c] != FRONT_SENTINEL) throw Error(KX_ERR_STATE, what);
    }
}
// 64 bytes of 0xA5 behind a buffer, as in kx_test_output_plan
void guard_untouched(const void* d_at, const char* what) {
    unsigned char tail[64];
    KX_HIP(hipMemcpy(tail, d_at, 64, hipMemcpyDeviceToHost));
    for (unsigned char c : tail)
        if (c != 0xA5) throw Error(KX_ERR_STATE, what);
}
}  // namespace

int kx_test_lstm_ragged(int device_id, const float* x, const int32_t* lens, int B, int L, int n_in, const float* w_ih,
                        const float* w_hh, const float* b_ih, const float* b_hh, const float* w_ih_r, const float* w_hh_r,
                        const float* b_ih_r, const float* b_hh_r, int inplace, int repeat, uint32_t epoch0, float* y, char* err,
                        size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(x && lens && y && B > 0 && L > 0 && n_in > 0 && repeat >= 1 && repeat <= 16 && epoch0 <= 0xffffu, "test_lstm_ragged: bad argument");
        KX_REQUIRE(!inplace || n_in == 640, "test_lstm_ragged: the in-place form is the duration encoder's: 640 input rows");
        for (int b = 0; b < B; ++b) KX_REQUIRE(lens[b] >= 1 && lens[b] <= L, "test_lstm_ragged: lens out of range");
        KX_HIP(hipSetDevice(device_id));
        DevMem dm;
        const int ld = pad32(L);
        const float poison = std::nanf("");
        // [B,L,n_in] -> channel-major [B][n_in][ld]; the row padding and every column >= lens[b] are NaN
        std::vector<float> xc((size_t)B * n_in * ld, poison);
        for (int b = 0; b < B; ++b)
            for (int t = 0; t < lens[b]; ++t)
                for (int c = 0; c < n_in; ++c) xc[((size_t)b * n_in + c) * ld + t] = x[((size_t)b * L + t) * n_in + c];
        float* dx = dm.up(xc.data(), xc.size());
        int* d_len = dm.up(lens, B);
        const kx::LenMap lm{d_len, 1, 0};
        // the input GEMM as in kx_test_lstm (f32 kernel, time-major store), on the ragged lengths; gx starts as NaN throughout, so a
        // recurrence that reads a row past an utterance's length poisons its output
        const kx::DevAlloc alloc = [&dm](size_t bytes) -> void* { return dm.get<unsigned char>(bytes); };
        const kx::PackSrc src{{dm.up(w_ih, (size_t)1024 * n_in), dm.up(w_ih_r, (size_t)1024 * n_in), nullptr}, {1024, 1024, 0}};
        const kx::ConvW ih = kx::pack_conv(src, n_in, 1, nullptr, alloc);
        float* bias = dm.get<float>(2048);
        kx::launch_vec_add(dm.up(b_ih, 1024), dm.up(b_hh, 1024), bias, 1024, nullptr);
        kx::launch_vec_add(dm.up(b_ih_r, 1024), dm.up(b_hh_r, 1024), bias + 1024, 1024, nullptr);
        float* whhT = dm.get<float>(2 * 256 * 1024);
        kx::launch_transpose_whh(dm.up(w_hh, 1024 * 256), whhT, nullptr);
        kx::launch_transpose_whh(dm.up(w_hh_r, 1024 * 256), whhT + 256 * 1024, nullptr);
        float* gx = dm.get<float>((size_t)B * L * 2048);
        KX_HIP(hipMemset(gx, 0xFF, (size_t)B * L * 2048 * 4));
        kx::ConvArgs a{};
        a.x = dx;
        a.x_bs = (long)n_in * ld;
        a.x_ld = ld;
        a.Cin = n_in;
        a.in_len = lm;
        a.out_len = lm;
        a.n_chunks = ih.n_chunks;
        a.w = ih.w;
        a.bias = bias;
        a.K = 1; a.dil = 1; a.stride = 1; a.pad = 0;
        a.Cout = ih.rows;
        a.y = gx;
        a.y_bs = (long)L * 2048;
        a.y_ld = 2048;
        a.out_mul = 1.f; a.out_div = 1.f;
        a.store = kx::ST_TMAJOR;
        a.up_cout = 1;
        kx::launch_conv1d(a, ih.BM, B, L, nullptr);
        KX_HIP(hipDeviceSynchronize());  // (in place, the rows it read are blanked next)
        // the output: 512 padded rows per utterance, of a tensor of its own or (in place, as Model::lstm is called for the duration
        // encoder) rows 0..511 of the 640-row input, whose other 128 rows must come back as they were
        const long y_bs = inplace ? (long)640 * ld : (long)512 * ld;
        float* dy = inplace ? dx : dm.get<float>((size_t)B * 512 * ld);
        const std::vector<float> blank((size_t)512 * ld, FRONT_SENTINEL);
        unsigned long long* xchg = dm.get<unsigned long long>(kx::lstm_exchange_bytes(B) / sizeof(unsigned long long));
        KX_HIP(hipMemset(xchg, 0, kx::lstm_exchange_bytes(B)));
        unsigned* errw = dm.get<unsigned>(1);
        KX_HIP(hipMemset(errw, 0, sizeof(unsigned)));
        unsigned epoch_state = epoch0;  // (the exchange buffer's own launch counter, as Model keeps one per buffer)
        std::vector<float> got((size_t)B * 512 * ld), first;
        for (int r = 0; r < repeat; ++r) {
            // (hipMemcpy on the null stream: behind the GEMM that read these rows, and behind the previous launch)
            for (int b = 0; b < B; ++b) KX_HIP(hipMemcpy(dy + b * y_bs, blank.data(), blank.size() * 4, hipMemcpyHostToDevice));
            kx::launch_lstm(gx, (long)L * 2048, 2048, whhT, dy, y_bs, ld, lm, B, xchg, errw, nullptr, &epoch_state);
            KX_HIP(hipDeviceSynchronize());
            unsigned herr = 0;
            KX_HIP(hipMemcpy(&herr, errw, sizeof(unsigned), hipMemcpyDeviceToHost));
            if (herr) throw Error(KX_ERR_DEVICE, "test_lstm_ragged: the two-CU recurrence timed out waiting for its partner");
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
                    if (row[t] != FRONT_SENTINEL) throw Error(KX_ERR_STATE, "test_lstm_ragged: the kernel wrote into the row padding");
            }
    });
}

int kx_test_alignment(int device_id, const float* logits, int B, int T, const int32_t* lens, const float* speeds, int n_speed,
                      const int32_t* pinned, int n_pinned, const float* src, int C, int idx_ld, int32_t* dur, int32_t* frames,
                      int32_t* idx, float* gathered, int Fcap, uint32_t* overflow, char* err, size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(logits && lens && speeds && src && dur && frames && idx && gathered && overflow && B > 0 && T > 0 && T <= 512 && C > 0 &&
                       idx_ld >= 1 && idx_ld <= 50 * 512 && Fcap >= 1 && (n_speed == 1 || n_speed == B) && n_pinned >= 0 && n_pinned <= 512 &&
                       (n_pinned == 0 || pinned),
                   "test_alignment: bad argument");
        for (int b = 0; b < B; ++b) KX_REQUIRE(lens[b] >= 1 && lens[b] <= T, "test_alignment: lens out of range");
        for (int i = 0; i < n_speed; ++i) KX_REQUIRE(speeds[i] > 0.f, "test_alignment: speed must be > 0");
        for (int i = 0; i < n_pinned; ++i) KX_REQUIRE(pinned[i] >= 1 && pinned[i] <= 50, "test_alignment: pinned durations must be in 1..50");
        KX_HIP(hipSetDevice(device_id));
        DevMem dm;
        const int Tp = pad32(T);
        const float poison = std::nanf("");
        // logits and src on the model's padded rows: the padding and every column >= lens[b] are NaN
        auto ragged = [&](const float* p, int rows) {
            std::vector<float> v((size_t)B * rows * Tp, poison);
            for (int b = 0; b < B; ++b)
                for (int r = 0; r < rows; ++r)
                    std::memcpy(&v[((size_t)b * rows + r) * Tp], p + ((size_t)b * rows + r) * T, (size_t)lens[b] * 4);
            return v;
        };
        const std::vector<float> lg = ragged(logits, 50), sp = ragged(src, C);
        const float* d_lg = dm.up(lg.data(), lg.size());
        const float* d_src = dm.up(sp.data(), sp.size());
        const int* d_len = dm.up(lens, B);
        const float* d_speed = dm.up(speeds, n_speed);
        const int* d_pin = n_pinned ? dm.up(pinned, n_pinned) : nullptr;
        // integer outputs start as 0xA5 bytes; 64 more of them stand guard behind idx
        int* d_dur = dm.get<int>((size_t)B * 512);
        int* d_frames = dm.get<int>(B);
        int* d_idx = dm.get<int>((size_t)B * idx_ld + 16);
        unsigned* d_over = dm.get<unsigned>(1);
        KX_HIP(hipMemset(d_dur, 0xA5, (size_t)B * 512 * 4));
        KX_HIP(hipMemset(d_frames, 0xA5, (size_t)B * 4));
        KX_HIP(hipMemset(d_idx, 0xA5, ((size_t)B * idx_ld + 16) * 4));
        KX_HIP(hipMemset(d_over, 0, sizeof(unsigned)));
        kx::launch_duration(d_lg, (long)50 * Tp, Tp, d_speed, n_speed, d_len, d_pin, n_pinned, d_dur, d_frames, d_idx, idx_ld, d_over, B, nullptr);
        KX_HIP(hipDeviceSynchronize());
        KX_HIP(hipMemcpy(dur, d_dur, (size_t)B * 512 * 4, hipMemcpyDeviceToHost));
        KX_HIP(hipMemcpy(frames, d_frames, (size_t)B * 4, hipMemcpyDeviceToHost));
        KX_HIP(hipMemcpy(idx, d_idx, (size_t)B * idx_ld * 4, hipMemcpyDeviceToHost));
        KX_HIP(hipMemcpy(overflow, d_over, sizeof(unsigned), hipMemcpyDeviceToHost));
        guard_untouched(d_idx + (size_t)B * idx_ld, "test_alignment: the duration kernel wrote past idx");
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
        float* d_g = dm.get<float>(n_g + 16);
        {
            const std::vector<float> blank(n_g, FRONT_SENTINEL);
            KX_HIP(hipMemcpy(d_g, blank.data(), n_g * 4, hipMemcpyHostToDevice));
            KX_HIP(hipMemset(d_g + n_g, 0xA5, 64));
        }
        if (Fmax > 0) kx::launch_gather_cols(d_src, (long)C * Tp, Tp, d_g, (long)C * Fp, Fp, C, d_idx, idx_ld, d_frames, B, Fmax, nullptr);
        KX_HIP(hipDeviceSynchronize());
        unpad_rows(d_g, (size_t)B * C, Fcap, Fp, gathered, "test_alignment: the gather wrote into the row padding");
        guard_untouched(d_g + n_g, "test_alignment: the gather wrote past its tensor");
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
        for (int b = 0; b < B; ++b) KX_REQUIRE(lens[b] >= 1 && lens[b] <= T, "test_embed: lens out of range");
        KX_HIP(hipSetDevice(device_id));
        DevMem dm;
        const int ld = pad32(T);
        const int64_t* d_ids = dm.up(ids, (size_t)B * ids_stride);
        const int* d_len = dm.up(lens, B);
        const float* d_tab = dm.up(text_table, (size_t)n_vocab * 512);
        const float* d_word = dm.up(word, (size_t)n_vocab * 128);
        const float* d_type = dm.up(type0, 128);
        const float* d_pos = dm.up(pos, (size_t)T * 128);
        const std::vector<float> blank((size_t)B * 512 * ld, FRONT_SENTINEL);
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
        float* d_out = dm.get<float>(n + 16);
        const std::vector<float> blank(n, FRONT_SENTINEL);
        KX_HIP(hipMemcpy(d_out, blank.data(), n * 4, hipMemcpyHostToDevice));
        KX_HIP(hipMemset(d_out + n, 0xA5, 64));
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
        const std::vector<float> blank((size_t)B * 640 * ld, FRONT_SENTINEL);
        float* d_fill = dm.up(blank.data(), blank.size());
        kx::launch_fill_style_rows(d_fill, (long)640 * ld, ld, 512, d_styles, 128, d_len, B, T, nullptr);
        // a copy between tensors of different row strides over a mapped length (lens[b] mul + add columns of every row)
        const int sld = pad32(Ls), dld = pad32(Ld) + 32;
        std::vector<float> sp;
        padded_rows(src, (size_t)B * rows, Ls, sld, std::nanf(""), sp);
        const float* d_src = dm.up(sp.data(), sp.size());
        const size_t n = (size_t)B * rows * dld;
        float* d_copy = dm.get<float>(n + 16);
        {
            const std::vector<float> blank2(n, FRONT_SENTINEL);
            KX_HIP(hipMemcpy(d_copy, blank2.data(), n * 4, hipMemcpyHostToDevice));
            KX_HIP(hipMemset(d_copy + n, 0xA5, 64));
        }
        kx::launch_copy_rows(d_src, (long)rows * sld, sld, d_copy, (long)rows * dld, dld, rows, kx::LenMap{d_len, mul, add}, B, Ld, nullptr);
        KX_HIP(hipDeviceSynchronize());
        unpad_rows(d_fill, (size_t)B * 640, T, ld, fill_out, "test_rows: fill_style_rows_kernel wrote into the row padding");
        unpad_rows(d_copy, (size_t)B * rows, Ld, dld, copy_out, "test_rows: copy_rows_kernel wrote into the row padding");
        guard_untouched(d_copy + n, "test_rows: copy_rows_kernel wrote past its tensor");
    });
}

// ---- the back half's kernels that are no conv: harmonic source, the STFT pair, the up-sampling pool ---------------------------------
namespace {
constexpr int HEAD_MAX_B = 64;        // utterances per hook call
constexpr int HEAD_MAX_F = 64;        // frames per utterance for the STFT hooks (38 400 samples, 7 681 STFT frames)
constexpr int SOURCE_MAX_F = 2048;    // frames per utterance for the source hook (four chunks of its phase kernel)
// a device buffer of n floats holding `fill`, 64 bytes of 0xA5 behind it
float* guarded_buffer(DevMem& dm, size_t n, float fill) {
    float* d = dm.get<float>(n + 16);
    const std::vector<float> blank(n, fill);
    KX_HIP(hipMemcpy(d, blank.data(), n * 4, hipMemcpyHostToDevice));
    KX_HIP(hipMemset(d + n, 0xA5, 64));
    return d;
}
// a host image uploaded behind which 64 bytes of 0xA5 stand (inputs: a kernel that wrote into one would be caught as well)
float* guarded_upload(DevMem& dm, const std::vector<float>& v) {
    float* d = dm.get<float>(v.size() + 16);
    KX_HIP(hipMemcpy(d, v.data(), v.size() * 4, hipMemcpyHostToDevice));
    KX_HIP(hipMemset(d + v.size(), 0xA5, 64));
    return d;
}
void check_frames(const int32_t* frames, int B, int Fmax, const char* what) {
    for (int b = 0; b < B; ++b)
        if (frames[b] < 1 || frames[b] > Fmax) throw Error(KX_ERR_INVALID, what);
}
}  // namespace

int kx_test_source_ragged(int device_id, const float* f0, const int32_t* frames, int B, int Fmax, const float* lin_w, float lin_b,
                          uint64_t seed, uint64_t utt_base, const uint64_t* utt_seeds, const uint32_t* utt_index, int noise_off,
                          float* out, char* err, size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(f0 && frames && lin_w && out && B > 0 && B <= HEAD_MAX_B && Fmax > 0 && Fmax <= SOURCE_MAX_F && (utt_seeds || !utt_index),
                   "test_source_ragged: bad argument");
        check_frames(frames, B, Fmax, "test_source_ragged: frames out of range");
        KX_HIP(hipSetDevice(device_id));
        kx::init_dft_tables();
        DevMem dm;
        // f0 on padded rows: NaN in the padding and in every step >= 2 frames[b]
        const int L2 = 2 * Fmax, f0_ld = pad32(L2);
        std::vector<float> fp((size_t)B * f0_ld, std::nanf(""));
        for (int b = 0; b < B; ++b) std::memcpy(&fp[(size_t)b * f0_ld], f0 + (size_t)b * L2, (size_t)2 * frames[b] * 4);
        const float* d_f0 = guarded_upload(dm, fp);
        const int* d_fr = dm.up(frames, B);
        const float* d_w = dm.up(lin_w, 9);
        const float* d_b = dm.up(&lin_b, 1);
        const uint64_t* d_seeds = utt_seeds ? dm.up(utt_seeds, B) : nullptr;
        const uint32_t* d_index = utt_index ? dm.up(utt_index, B) : nullptr;
        // the phase workspace [B][9][2 Fmax] as the model sizes it, and the output on rows longer than 600 Fmax
        const size_t n_ph = (size_t)B * 9 * L2;
        float* phase = guarded_buffer(dm, n_ph, std::nanf(""));
        const int Ls = 600 * Fmax, har_ld = pad32(Ls) + 32;
        const size_t n_har = (size_t)B * har_ld;
        float* har = guarded_buffer(dm, n_har, FRONT_SENTINEL);
        kx::launch_source(d_f0, f0_ld, d_fr, B, Fmax, d_w, d_b, seed, utt_base, d_seeds, d_index, noise_off, phase, har, har_ld, nullptr);
        KX_HIP(hipDeviceSynchronize());
        // (samples >= 600 frames[b] go back as they are: the sentinel, if the kernel left them alone)
        unpad_rows(har, (size_t)B, Ls, har_ld, out, "test_source_ragged: source_sample_kernel wrote into the row padding");
        guard_untouched(har + n_har, "test_source_ragged: source_sample_kernel wrote past its tensor");
        guard_untouched(phase + n_ph, "test_source_ragged: source_phase_kernel wrote past its workspace");
        guard_untouched(d_f0 + fp.size(), "test_source_ragged: a kernel wrote behind f0");
    });
}

int kx_test_stft(int device_id, const float* hs, int B, int hs_ld, const int32_t* frames, int Fmax, int variant, float* har, char* err,
                 size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(hs && frames && har && B > 0 && B <= HEAD_MAX_B && Fmax > 0 && Fmax <= HEAD_MAX_F && hs_ld >= 600 * Fmax &&
                       hs_ld <= 600 * Fmax + 4096 && (variant == kx::STFT_ONNX || variant == kx::STFT_TORCH),
                   "test_stft: bad argument");
        check_frames(frames, B, Fmax, "test_stft: frames out of range");
        KX_HIP(hipSetDevice(device_id));
        kx::init_dft_tables();
        DevMem dm;
        // the source rows as the caller strides them: NaN from sample 600 frames[b] on
        std::vector<float> hp((size_t)B * hs_ld, std::nanf(""));
        for (int b = 0; b < B; ++b) std::memcpy(&hp[(size_t)b * hs_ld], hs + (size_t)b * hs_ld, (size_t)600 * frames[b] * 4);
        const float* d_hs = guarded_upload(dm, hp);
        const int* d_fr = dm.up(frames, B);
        const int nfmax = 120 * Fmax + 1, ld = pad32(nfmax);
        const size_t n = (size_t)B * 22 * ld;
        float* d_har = guarded_buffer(dm, n, FRONT_SENTINEL);
        kx::launch_stft(d_hs, hs_ld, d_har, (long)22 * ld, ld, d_fr, B, Fmax, variant, nullptr);
        KX_HIP(hipDeviceSynchronize());
        unpad_rows(d_har, (size_t)B * 22, nfmax, ld, har, "test_stft: stft_kernel wrote into the row padding");
        guard_untouched(d_har + n, "test_stft: stft_kernel wrote past its tensor");
        guard_untouched(d_hs + hp.size(), "test_stft: stft_kernel wrote behind its input");
    });
}

int kx_test_istft_head(int device_id, const float* cp, int B, const int32_t* frames, int Fmax, int variant, float* spec, float* audio,
                       char* err, size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(cp && frames && spec && audio && B > 0 && B <= HEAD_MAX_B && Fmax > 0 && Fmax <= HEAD_MAX_F &&
                       (variant == kx::STFT_ONNX || variant == kx::STFT_TORCH),
                   "test_istft_head: bad argument");
        check_frames(frames, B, Fmax, "test_istft_head: frames out of range");
        KX_HIP(hipSetDevice(device_id));
        kx::init_dft_tables();
        DevMem dm;
        // conv_post's output on the model's padded rows: NaN in the padding and from frame 120 frames[b] + 1 on
        const int nfmax = 120 * Fmax + 1, ld = pad32(nfmax);
        const size_t n = (size_t)B * 22 * ld;
        std::vector<float> cpp(n, std::nanf(""));
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < 22; ++k)
                std::memcpy(&cpp[((size_t)b * 22 + k) * ld], cp + ((size_t)b * 22 + k) * nfmax, (size_t)(120 * frames[b] + 1) * 4);
        const float* d_cp = guarded_upload(dm, cpp);
        const int* d_fr = dm.up(frames, B);
        float* d_spec = guarded_buffer(dm, n, FRONT_SENTINEL);
        const int Ls = 600 * Fmax, audio_ld = pad32(Ls) + 32;
        const size_t n_a = (size_t)B * audio_ld;
        float* d_audio = guarded_buffer(dm, n_a, FRONT_SENTINEL);
        kx::launch_istft_head(d_cp, (long)22 * ld, ld, d_spec, d_audio, audio_ld, d_fr, B, Fmax, variant, nullptr);
        KX_HIP(hipDeviceSynchronize());
        unpad_rows(d_spec, (size_t)B * 22, nfmax, ld, spec, "test_istft_head: istft_spec_kernel wrote into the row padding");
        unpad_rows(d_audio, (size_t)B, Ls, audio_ld, audio, "test_istft_head: istft_ola_kernel wrote into the row padding");
        guard_untouched(d_spec + n, "test_istft_head: istft_spec_kernel wrote past its tensor");
        guard_untouched(d_audio + n_a, "test_istft_head: istft_ola_kernel wrote past its tensor");
        guard_untouched(d_cp + n, "test_istft_head: a kernel wrote behind its input");
    });
}

int kx_test_pool_up2(int device_id, const float* x, int B, int C, int L, const int32_t* lens, const float* norm, int n_bs, const float* w,
                     const float* bias, float slope, float* y, char* err, size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(x && lens && norm && w && bias && y && B > 0 && B <= HEAD_MAX_B && C > 0 && C <= 1024 && L > 0 && L <= 4096 && n_bs > C &&
                       n_bs <= 2048,
                   "test_pool_up2: bad argument");
        for (int b = 0; b < B; ++b) KX_REQUIRE(lens[b] >= 1 && lens[b] <= L, "test_pool_up2: lens out of range");
        KX_HIP(hipSetDevice(device_id));
        DevMem dm;
        const float poison = std::nanf("");
        // x on the model's padded rows: NaN in the padding and in every column >= lens[b]
        const int x_ld = pad32(L);
        std::vector<float> xp((size_t)B * C * x_ld, poison);
        for (int b = 0; b < B; ++b)
            for (int c = 0; c < C; ++c)
                std::memcpy(&xp[((size_t)b * C + c) * x_ld], x + ((size_t)b * C + c) * L, (size_t)lens[b] * 4);
        const float* d_x = guarded_upload(dm, xp);
        // the (mean, scale, shift) planes [3][B][n_bs]: an utterance's C values at the front of its n_bs slots, the others NaN
        std::vector<float> pl((size_t)3 * B * n_bs, poison);
        for (int p = 0; p < 3; ++p)
            for (int b = 0; b < B; ++b) std::memcpy(&pl[((size_t)p * B + b) * n_bs], norm + ((size_t)p * B + b) * C, (size_t)C * 4);
        const float* d_pl = dm.up(pl.data(), pl.size());
        const float* d_w = dm.up(w, (size_t)C * 3);
        const float* d_bias = dm.up(bias, (size_t)C);
        const int* d_len = dm.up(lens, B);
        // y on rows of another stride than x's
        const int y_ld = pad32(2 * L) + 32;
        const size_t n = (size_t)B * C * y_ld;
        float* d_y = guarded_buffer(dm, n, FRONT_SENTINEL);
        kx::launch_pool_up2(d_x, (long)C * x_ld, x_ld, C, d_pl, d_pl + (size_t)B * n_bs, d_pl + (size_t)2 * B * n_bs, n_bs, slope, d_w, d_bias,
                            d_y, (long)C * y_ld, y_ld, kx::LenMap{d_len, 1, 0}, B, L, nullptr);
        KX_HIP(hipDeviceSynchronize());
        unpad_rows(d_y, (size_t)B * C, 2 * L, y_ld, y, "test_pool_up2: pool_up2_kernel wrote into the row padding");
        guard_untouched(d_y + n, "test_pool_up2: pool_up2_kernel wrote past its tensor");
        guard_untouched(d_x + xp.size(), "test_pool_up2: pool_up2_kernel wrote behind its input");
    });
}

// ---- a layer's weight images, byte for byte ---------------------------------------------------------------------------------------
int kx_test_weight_images(int device_id, const float* const* src, const int32_t* src_rows, int n_src, int Cin, int K, int up_stride,
                          int64_t* meta, float* unscale, void* const* images, const int64_t* cap, char* err, size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(src && src_rows && meta && unscale && images && cap && n_src >= 1 && n_src <= 3 && up_stride >= 0,
                   "test_weight_images: bad argument");
        KX_REQUIRE(up_stride == 0 || (n_src == 1 && K == 2 * up_stride), "test_weight_images: a transposed weight is one source of 2 s taps");
        // sizes no layer has are refused before anything is launched (a transposed weight's GEMM has stride x Cout rows)
        long rows = 0;
        for (int i = 0; i < n_src; ++i) {
            KX_REQUIRE(src[i] && src_rows[i] >= 1 && src_rows[i] <= 4096, "test_weight_images: rows out of range");
            rows += src_rows[i];
        }
        if (up_stride) rows *= up_stride;
        KX_REQUIRE(rows <= 4096 && Cin >= 1 && Cin <= 2048 && K >= 1 && K <= 24, "test_weight_images: size out of range");
        KX_HIP(hipSetDevice(device_id));
        DevMem dm;
        // every image behind a guard, and filled with a pattern no packer writes into a padding slot (a padding slot is +0)
        struct Img { unsigned char* p; size_t bytes; };
        std::vector<Img> imgs;
        const kx::DevAlloc alloc = [&](size_t bytes) -> void* {
            unsigned char* p = dm.get<unsigned char>(bytes + 64);
            KX_HIP(hipMemset(p, 0xC3, bytes));
            KX_HIP(hipMemset(p + bytes, 0xA5, 64));
            imgs.push_back({p, bytes});
            return p;
        };
        kx::ConvW cw;
        std::vector<const float*> d_src;
        std::vector<size_t> n_srcf;
        if (up_stride) {
            n_srcf.push_back((size_t)Cin * src_rows[0] * K);
            d_src.push_back(guarded_upload(dm, std::vector<float>(src[0], src[0] + n_srcf[0])));
            cw = kx::pack_convT(d_src[0], Cin, src_rows[0], up_stride, nullptr, alloc);
        } else {
            kx::PackSrc ps{{nullptr, nullptr, nullptr}, {0, 0, 0}};
            for (int i = 0; i < n_src; ++i) {
                n_srcf.push_back((size_t)src_rows[i] * Cin * K);
                d_src.push_back(guarded_upload(dm, std::vector<float>(src[i], src[i] + n_srcf[i])));
                ps.p[i] = d_src[i];
                ps.rows[i] = src_rows[i];
            }
            cw = kx::pack_conv(ps, Cin, K, nullptr, alloc);
        }
        kx::add_bf16_image(cw, nullptr, alloc);
        kx::add_f8_image(cw, nullptr, alloc);
        KX_HIP(hipDeviceSynchronize());
        for (const Img& im : imgs) guard_untouched(im.p + im.bytes, "test_weight_images: a packer wrote past its image");
        for (size_t i = 0; i < d_src.size(); ++i) guard_untouched(d_src[i] + n_srcf[i], "test_weight_images: a packer wrote behind a source");
        const int64_t m5[5] = {cw.BM, cw.rows, cw.n_chunks, cw.n_chunks16, cw.K};
        for (int i = 0; i < 5; ++i) meta[i] = m5[i];
        *unscale = cw.unscale;
        const void* which[4] = {cw.w, cw.w16, cw.w16b, cw.w8x};
        for (int k = 0; k < 4; ++k) {
            meta[5 + k] = 0;
            if (!which[k]) continue;  // (an image the layer does not get: length 0)
            const Img* im = nullptr;
            for (const Img& c : imgs)
                if (c.p == which[k]) im = &c;
            KX_REQUIRE(im, "test_weight_images: an image that did not come from the allocator");
            KX_REQUIRE(images[k] && cap[k] >= (int64_t)im->bytes, "test_weight_images: image buffer too small");
            KX_HIP(hipMemcpy(images[k], im->p, im->bytes, hipMemcpyDeviceToHost));
            meta[5 + k] = (int64_t)im->bytes;
        }
    });
}

}  // extern "C"
