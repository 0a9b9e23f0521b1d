// The f16f8 forms of the direct-A conv's 16x16x32 loop (conv1d_f16x3_da_kernel<.., S16 = true, .., F8 = true>: a_hi b_hi on the f16
// MFMA, the two cross terms of a product on v_mfma_scale_f32_16x16x128_f8f6f4), compiled beside the others: the layers that carry
// an 8-bit cross image (ConvArgs::w8x, KOKOROX_CONV=f16f8, the default mode) and whose tap count is 3 mod 4 (11, 7 and 3).
#define KX_DA_UNIT
#include "conv_f16x3_da.hip"

namespace kx {

void launch_conv16_da_f8(const ConvPlan& p, const ConvArgs& a, int B, hipStream_t s) {
    KX_REQUIRE(p.form == FORM_DA_F8 && a.w8x != nullptr && (p.kt == 11 || p.kt == 7 || p.kt == 3) && a.K == p.kt && (a.K - 1) * a.dil <= 64 &&
                   a.act == ACT_SNAKE && !a.prec1 && a.n_chunks16 >= 2 && (a.n_chunks16 & 1) == 0,
               "conv1d f16x3 da f8: launch not eligible");
    KX_REQUIRE(p.bn == 192 || p.bn == 128, "conv1d f16x3 da f8: tile of 192 or 128 columns");
    KX_REQUIRE((long)a.Cin * a.x_ld * 4 < (1L << 32), "conv1d f16x3 da f8: input tensor of one utterance beyond 4 GiB");
    if (p.kt == 11) {
        if (p.bn == 192) launch_da_inst<ACT_SNAKE, 11, 6, false, false, true, false, false, true>(a, B, p.cols, s);
        else launch_da_inst<ACT_SNAKE, 11, 4, false, false, true, false, false, true>(a, B, p.cols, s);
    } else if (p.kt == 7) {
        if (p.bn == 192) launch_da_inst<ACT_SNAKE, 7, 6, false, false, true, false, false, true>(a, B, p.cols, s);
        else launch_da_inst<ACT_SNAKE, 7, 4, false, false, true, false, false, true>(a, B, p.cols, s);
    } else {
        if (p.bn == 192) launch_da_inst<ACT_SNAKE, 3, 6, false, false, true, false, false, true>(a, B, p.cols, s);
        else launch_da_inst<ACT_SNAKE, 3, 4, false, false, true, false, false, true>(a, B, p.cols, s);
    }
}

}  // namespace kx
