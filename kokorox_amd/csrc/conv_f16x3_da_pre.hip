// The pre-split-image forms of the direct-A conv kernel (see conv_f16x3_da.hip, "PRE"): a translation unit of their own, compiled
// beside the others.  The input is a pre-split image (a.x16); which layers get one is decided from the layer's shape alone
// (conv_plan.hip), never from the batch.
#define KX_DA_UNIT
#include "conv_f16x3_da.hip"

namespace kx {

void launch_conv16_da_pre(const ConvPlan& p, const ConvArgs& a, int B, hipStream_t s) {
    KX_REQUIRE(p.form == FORM_DA_PRE && a.x16 != nullptr && a.x16_ld > 0 && !a.in_up2 && !a.prec1 && (p.kt == 0 || (a.K == 3 && p.kt == 3)),
               "conv1d f16x3 da pre: launch not eligible");
    KX_REQUIRE(p.bn == 256 || p.bn == 128, "conv1d f16x3 da pre: tile of 256 or 128 columns");
    // the chunk term of the image offsets is a 32-bit scalar: n_chunks x four planes x x16_ld x 16 B per utterance
    KX_REQUIRE((long)a.n_chunks16 * 64 * a.x16_ld < (1L << 31), "conv1d f16x3 da pre: image of one utterance beyond 2 GiB");
    // the unrolled 3-tap forms (2 x 2 waves on the 256-column tile), else run-time taps
    if (p.bn == 256) {
        if (p.kt == 3) launch_da_inst<ACT_NONE, 3, 8, false, true, false, true>(a, B, p.cols, s);
        else launch_da_inst<ACT_NONE, 0, 8, false, false, false, true>(a, B, p.cols, s);
    } else {
        if (p.kt == 3) launch_da_inst<ACT_NONE, 3, 4, false, false, false, true>(a, B, p.cols, s);
        else launch_da_inst<ACT_NONE, 0, 4, false, false, false, true>(a, B, p.cols, s);
    }
}

}  // namespace kx
