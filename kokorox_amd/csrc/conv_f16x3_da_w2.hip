// The 2 x 2-wave forms of the direct-A conv's unrolled main loop on the 256-column tile (conv1d_f16x3_da_kernel<.., W2 = true>),
// compiled beside the others.  Results are bit-identical to the 4 x 1 forms they replace.
#define KX_DA_UNIT
#include "conv_f16x3_da.hip"

namespace kx {

void launch_conv16_da_w2(const ConvPlan& p, const ConvArgs& a, int B, hipStream_t s) {
    KX_REQUIRE(p.form == FORM_DA_W2 && p.bn == 256 && a.K == p.kt && (a.K - 1) * a.dil <= 64 && !a.prec1 &&
                   ((p.act == ACT_SNAKE && (p.kt == 3 || p.kt == 7 || p.kt == 11)) || (p.act == ACT_LEAKY && p.kt == 3)),
               "conv1d f16x3 da w2: launch not eligible");
#ifdef KX_DA_AUDIT
    launch_da_inst<ACT_SNAKE, 11, 8, false, true>(a, B, p.cols, s);
    return;
#endif
    if (p.act == ACT_LEAKY) launch_da_inst<ACT_LEAKY, 3, 8, false, true>(a, B, p.cols, s);
    else if (p.kt == 11) launch_da_inst<ACT_SNAKE, 11, 8, false, true>(a, B, p.cols, s);
    else if (p.kt == 7) launch_da_inst<ACT_SNAKE, 7, 8, false, true>(a, B, p.cols, s);
    else launch_da_inst<ACT_SNAKE, 3, 8, false, true>(a, B, p.cols, s);
}

}  // namespace kx
