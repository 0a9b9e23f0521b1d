// Kernel hooks of tests/ (include/kokorox_hip_test.h), conv launches: the conv hook, the launch plan, a layer's weight images and the
// norm kernels that feed convs.  The conv hook takes its weight images, launch plan and kernel arguments from conv_call.hip, the code
// Model runs; what is its own is the buffers, the tensor views over them and the checks around the launch.
#include "test_hooks.h"

using namespace kx_test;

namespace {
constexpr int VIEW_ROWS = 8, VIEW_TOP = 3;  // a row-slice view: VIEW_TOP foreign rows above the tensor's own, VIEW_ROWS - VIEW_TOP below

// a ConvPlan as the 17 integers kx_test_conv_plan and kx_test_conv return
void plan_fields(const kx::ConvPlan& p, int64_t* out) {
    const int v[] = {p.form, p.bm, p.act, p.kt, p.wm, p.wn, p.vt, p.pf, p.p1, p.bf, p.bn, p.cols, p.merged, p.pre, p.stat_cols,
                     p.stat_tiles, p.flat_bn};
    for (int i = 0; i < 17; ++i) out[i] = v[i];
}
}  // namespace

extern "C" {

int kx_test_conv(const kx_test_conv_args* args, char* err, size_t err_len) {
    return guarded_free(err, err_len, [&] {
        KX_REQUIRE(args && args->struct_size == sizeof(kx_test_conv_args), "test_conv: struct_size is not sizeof(kx_test_conv_args)");
        const kx_test_conv_args& ex = *args;
        check_device(ex.device_id);
        const float *x = ex.x, *w = ex.w;
        float* y = ex.y;
        const int B = ex.B, Cin = ex.Cin, L = ex.L, Cout = ex.Cout, k = ex.k, pad = ex.pad, dil = ex.dil, act = ex.act;
        KX_REQUIRE(ex.up_stride >= 0 && ex.stride >= 1 && (ex.stride == 1 || !ex.up_stride), "test_conv1d_opts: stride >= 1, with plain convs only");
        // a polyphase transposed conv is a GEMM whose stride is the up-sampling factor
        const bool transposed = ex.up_stride > 0;
        const int stride = transposed ? ex.up_stride : ex.stride;
        const int Lv = ex.in_up2 ? 2 * L : L;  // the input length the conv sees
        const int span = Lv + 2 * pad - dil * (k - 1) - 1;
        const int Lout = transposed ? (L - 1) * stride - 2 * pad + k : (span >= 0 ? span / stride + 1 : 0);
        KX_REQUIRE(x && w && y && B > 0 && Cin > 0 && Cout > 0 && L > 0 && Lout > 0 && k > 0, "test_conv1d: bad argument");
        // the strict checks: unowned output columns start from the sentinel, guard bytes behind the buffers are checked
        const bool strict = ex.stride != 1 || ex.len_mul_in || ex.len_add_in || ex.len_mul_out || ex.len_add_out || ex.up_off || ex.view;
        KX_HIP(hipSetDevice(ex.device_id));
        DevMem dm;
        std::vector<int> lens(B, 1);
        int mode = ex.mode;
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
        const int up_off = ex.up_off ? 1 : 0;
        const int Ly = Lout + up_off;  // columns of y (Lout: the conv's own output length)
        KX_REQUIRE(up_off == 0 || transposed, "test_conv1d: an output offset comes with transposed convs");
        KX_REQUIRE(transposed || stride == 1 || (!ex.merged && !ex.in_up2 && !ex.tmajor),
                   "test_conv1d: a strided conv takes no merged, in_up2 or time-major launch");
        KX_REQUIRE(!ex.view || !ex.tmajor, "test_conv1d: row-slice views of channel-major tensors only");
        // (time-major stores: a row of y is one column's Cout values; padded, it ends in a 32-float margin)
        const int yr = ex.tmajor ? Lout : Cout, yc = ex.tmajor ? Cout : Ly;  // rows per utterance and columns of y as stored
        const int x_ld = ex.pad_ld ? pad32(L) : L;
        const int y_ld = ex.tmajor ? (ex.pad_ld ? pad32(Cout) + 32 : Cout) : (ex.pad_ld ? pad32(Ly) : Ly);
        const bool want_stats = ex.stats_out != nullptr || ex.norm_out != nullptr;
        KX_REQUIRE(!ex.tmajor || (!transposed && !ex.resid && !ex.accumulate && !want_stats), "test_conv1d: time-major stores are plain stores");
        KX_REQUIRE(!ex.in_up2 || !transposed, "test_conv1d: in_up2 with plain convs only");
        KX_REQUIRE(!ex.merged || (!transposed && Lout == L), "test_conv1d: merged columns need input and output of one length");
        KX_REQUIRE((ex.norm_out != nullptr) == (ex.norm_gb != nullptr), "test_conv1d: norm planes come with gamma / beta");
        KX_REQUIRE(ex.act_shift >= -24 && ex.act_shift <= 24 && ex.prec1 >= 0 && ex.prec1 <= 2, "test_conv1d: bad act_shift / prec1");
        KX_REQUIRE(!transposed || (k == 2 * stride && pad == (k - stride) / 2 && dil == 1), "test_conv1d: transposed needs k=2s, pad=(k-s)/2");
        KX_REQUIRE(act != kx::ACT_SNAKE || ex.alpha, "test_conv1d: snake needs alpha");
        // per utterance: the input columns it stores and the output columns it owns (without the offset column)
        const int up = ex.in_up2 ? 2 : 1;
        const bool units = ex.len_mul_in > 0;
        std::vector<int> lin(B, L), lout(B, Lout);
        KX_REQUIRE(ex.len_mul_in >= 0 && (units || (!ex.len_add_in && !ex.len_mul_out && !ex.len_add_out)), "test_conv1d: bad length map");
        KX_REQUIRE(!units || (ex.lens && !ex.in_up2 && !ex.merged), "test_conv1d: length maps need lens, and no in_up2 or merged launch");
        if (ex.lens) {  // ragged batch
            KX_REQUIRE(units || (!transposed && stride == 1), "test_conv1d: ragged strided and transposed convs state their length maps");
            check_lens(ex.lens, B, L, "test_conv1d: lens out of range");
            for (int b = 0; b < B; ++b) {
                if (units) {  // utterance b: lens[b] units; the output map must agree with the conv's own formula on the input count
                    lin[b] = ex.lens[b] * ex.len_mul_in + ex.len_add_in;
                    lout[b] = ex.lens[b] * ex.len_mul_out + ex.len_add_out;
                    KX_REQUIRE(lin[b] >= 1 && lin[b] <= L, "test_conv1d: an utterance's input columns overrun L");
                    const int want = transposed ? stride * lin[b] : (lin[b] + 2 * pad - dil * (k - 1) - 1) / stride + 1;
                    KX_REQUIRE(lin[b] + 2 * pad - dil * (k - 1) - 1 >= 0 || transposed, "test_conv1d: lens out of range");
                    KX_REQUIRE(lout[b] == want && lout[b] >= 1 && lout[b] <= Lout, "test_conv1d: the output length map contradicts the conv's own output count");
                } else {  // utterance b is lens[b] columns long (stride-1 convs: the output shrinks by Lv - Lout)
                    KX_REQUIRE(up * ex.lens[b] + (Lout - Lv) >= 1, "test_conv1d: lens out of range");
                    lin[b] = ex.lens[b];
                    lout[b] = up * ex.lens[b] + (Lout - Lv);
                }
                lens[b] = ex.lens[b];
            }
        } else if (ex.merged)
            lens.assign(B, L);
        KX_REQUIRE(ex.y_floats >= (int64_t)B * yr * yc, "test_conv: y is too small for the stored shape");
        // A [B][C][len] host tensor as the launch sees it: rows of ld floats (view: VIEW_TOP foreign rows above each utterance's C rows,
        // VIEW_ROWS in all), with `fill` in the foreign rows, in [len, ld) and - own given - in the columns at or past own[b]; src null
        // = zeros.  Uploaded with the guard behind it.
        const int vrows = ex.view ? VIEW_ROWS : 0, vtop = ex.view ? VIEW_TOP : 0;
        auto stage = [&](const float* src, int C, int len, int ld, float fill, const int* own, int own_add, size_t& n) {
            std::vector<float> v((size_t)B * (C + vrows) * ld, fill);
            for (int b = 0; b < B; ++b)
                for (int r = 0; r < C; ++r) {
                    float* d = &v[((size_t)b * (C + vrows) + vtop + r) * ld];
                    const int m = own ? std::min(len, own[b] + own_add) : len;
                    if (src)
                        std::memcpy(d, src + ((size_t)b * C + r) * len, (size_t)m * 4);
                    else
                        std::fill(d, d + m, 0.f);
                }
            n = v.size();
            return guarded_upload(dm, v);
        };
        const kx::DevAlloc alloc = [&dm](size_t bytes) -> void* { return dm.get<unsigned char>(bytes); };

        // the layer: its weight images from the model's packers (conv_call.hip), bias and pre-scale as Model keeps them
        const float* dw = dm.up(w, (size_t)Cout * Cin * k);
        kx::ConvW cw = transposed ? kx::pack_convT(dw, Cin, Cout, stride, nullptr, alloc)
                                  : kx::pack_conv(kx::PackSrc{{dw, nullptr, nullptr}, {Cout, 0, 0}}, Cin, k, nullptr, alloc);
        cw.bias = ex.bias ? dm.up(ex.bias, (size_t)Cout) : nullptr;
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
        size_t x_n = 0, y_n = 0, r_n = 0;
        float* dx = stage(x, Cin, L, x_ld, POISON, ex.lens ? lin.data() : nullptr, 0, x_n);
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
        float* dy = stage(ex.accumulate ? y : nullptr, yr, yc, y_ld, SENTINEL, strict && ex.lens ? lout.data() : nullptr, up_off, y_n);
        out.p = dy + (size_t)vtop * y_ld;
        out.bs = (long)(yr + vrows) * y_ld;
        out.ld = y_ld;
        out.C = rows;
        out.Lmax = Lout;
        const kx::LenMap own_len = units ? kx::LenMap{d_one, ex.len_mul_out, ex.len_add_out}
                                         : (ragged ? kx::LenMap{d_one, up, Lout - Lv} : kx::LenMap{d_one, 0, Lout});
        out.len = own_len;
        out.len.add += up_off;  // (the stored columns of y; an up-scattering launch masks with o.up_len)

        kx::ConvOpts o;
        if (transposed) {  // the polyphase two-tap GEMM, scattered to the up-sampled axis
            o.pad = 1;
            o.store = kx::ST_UPSCATTER;
            o.up_pad = pad;
            o.up_off = up_off;
            o.up_reflect = up_off;
            o.up_len = own_len;
        } else {
            o.stride = stride;
            o.pad = pad;
            o.dil = dil;
            o.store = ex.tmajor ? kx::ST_TMAJOR : kx::ST_NORMAL;
        }
        if (ex.norm) {
            const float* dn = dm.up(ex.norm, (size_t)3 * B * Cin);
            o.nmean = dn;
            o.nscale = dn + (size_t)B * Cin;
            o.nshift = dn + (size_t)2 * B * Cin;
        }
        o.act = act;
        o.slope = ex.slope;
        o.alpha = ex.alpha ? dm.up(ex.alpha, (size_t)Cin) : nullptr;
        o.in_up2 = ex.in_up2 != 0;
        o.epi = ex.epi;
        o.out_mul = ex.out_mul;
        o.out_div = ex.out_div;
        o.accum = ex.accumulate;
        float* d_res = nullptr;
        if (ex.resid) {
            // (laid out as y is: its own Ly columns, NaN behind them and past an utterance's own output)
            d_res = stage(ex.resid, Cout, Ly, y_ld, POISON, ex.lens ? lout.data() : nullptr, up_off, r_n);
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
        ctx.n_bs = ex.norm ? Cin : 0;
        ctx.force = (mode == kx::CONV_F16X3_LDS ? kx::FORCE_LDS : (mode == kx::CONV_F16X3_DA ? kx::FORCE_DA : 0)) | force_bits;
        ctx.image = pre ? 2 : 0;
        ctx.epi_stream = ex.epi_stream != 0;
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
            KX_REQUIRE(!transposed && !ex.accumulate && plan.stat_cols > 0, "test_conv1d: fused statistics come with plain, non-accumulating stores");
            part_n = (size_t)B * rows * plan.stat_tiles;
            d_part = reinterpret_cast<float2*>(guarded_buffer(dm, 2 * part_n, 0.f));
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
                        if (row[c] != SENTINEL)
                            throw Error(KX_ERR_STATE, foreign ? "test_conv1d: the kernel wrote into a foreign row of the output tensor"
                                                              : "test_conv1d: the kernel wrote into the row padding");
                }
        }
        if (strict) {
            const char* what = "test_conv1d: the guard bytes behind a buffer changed";
            guard_untouched(dx + x_n, what);
            guard_untouched(dy + y_n, what);
            if (d_res) guard_untouched(d_res + r_n, what);
            if (d_part) guard_untouched(reinterpret_cast<const float*>(d_part) + 2 * part_n, what);
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

int kx_test_layernorm(int device_id, const float* x, int B, int C, int T, const int32_t* lens, float eps, int mode, const float* g,
                      const float* be, float leaky, float* y, char* err, size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(x && y && lens && B > 0 && C > 0 && T > 0 && mode >= kx::LN_PLAIN && mode <= kx::LN_ADA, "test_layernorm: bad argument");
        KX_REQUIRE(mode == kx::LN_PLAIN || (g && be), "test_layernorm: the affine forms need gamma and beta");
        check_lens(lens, B, T, "test_layernorm: lens out of range");
        KX_HIP(hipSetDevice(device_id));
        DevMem dm;
        const int ld = pad32(T);  // rows padded as in the model; the input padding is NaN, the output holds the sentinel throughout
        const std::vector<float> xp = padded_rows(x, B, C, T, ld, POISON), blank(xp.size(), SENTINEL);
        const float* dx = dm.up(xp.data(), xp.size());
        float* dy = dm.up(blank.data(), blank.size());
        const int* d_len = dm.up(lens, B);
        const size_t ng = mode == kx::LN_ADA ? (size_t)B * C : (size_t)C;
        const float* dg = mode == kx::LN_PLAIN ? nullptr : dm.up(g, ng);
        const float* db = mode == kx::LN_PLAIN ? nullptr : dm.up(be, ng);
        kx::launch_layernorm_ch(dx, dy, (long)C * ld, ld, C, kx::LenMap{d_len, 1, 0}, B, T, eps, mode, dg, db, C, leaky, nullptr);
        KX_HIP(hipDeviceSynchronize());
        // (columns past lens[b] come back as the sentinel: the caller checks them)
        unpad_rows(dy, (size_t)B * C, T, ld, y, "test_layernorm: the kernel wrote into the row padding");
    });
}

int kx_test_instance_norm(int device_id, const float* x, int B, int C, int L, const int32_t* lens, const float* gb, float* out,
                          char* err, size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(x && lens && gb && out && B > 0 && C > 0 && L > 0, "test_instance_norm: bad argument");
        check_lens(lens, B, L, "test_instance_norm: lens out of range");
        KX_HIP(hipSetDevice(device_id));
        DevMem dm;
        const int ld = pad32(L);
        const std::vector<float> xp = padded_rows(x, B, C, L, ld, POISON);
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
            imgs.push_back({guarded_bytes<unsigned char>(dm, bytes, 0xC3), bytes});
            return imgs.back().p;
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
