// The 16x16x32 forms of the direct-A conv (conv1d_f16x3_da_kernel<.., S16 = true>: 11-tap snake convs and the un-dilated 7-tap
// ones, 192- and 128-column tiles), compiled beside the others.
#define KX_DA_UNIT
#include "conv_f16x3_da.hip"

namespace kx {

void launch_conv16_da_s16(const ConvPlan& p, const ConvArgs& a, int B, hipStream_t s) {
    KX_REQUIRE(p.form == FORM_DA_S16 && (p.kt == 11 || p.kt == 7) && a.K == p.kt && a.act == ACT_SNAKE && (a.K - 1) * a.dil <= 64 &&
                   !a.prec1 && a.n_chunks16 >= 2 && (a.n_chunks16 & 1) == 0,
               "conv1d f16x3 da s16: launch not eligible");
    KX_REQUIRE(p.bn == 192 || p.bn == 128, "conv1d f16x3 da s16: tile of 192 or 128 columns");
    if (p.kt == 11) {
        if (p.bn == 192) launch_da_inst<ACT_SNAKE, 11, 6, false, false, true>(a, B, p.cols, s);
        else launch_da_inst<ACT_SNAKE, 11, 4, false, false, true>(a, B, p.cols, s);
    } else {
        if (p.bn == 192) launch_da_inst<ACT_SNAKE, 7, 6, false, false, true>(a, B, p.cols, s);
        else launch_da_inst<ACT_SNAKE, 7, 4, false, false, true>(a, B, p.cols, s);
    }
}

}  // namespace kx
