// The reduced-precision instantiations of the direct-A conv kernel (one f16 MFMA per product: KOKOROX_CONV=f16; one bf16 MFMA on
// the layer's bf16 weight image: KOKOROX_CONV=bf16), compiled as a translation unit of their own beside conv_f16x3_da.hip.
#define KX_DA_UNIT
#include "conv_f16x3_da.hip"

namespace kx {

// FORM_DA with p1: the 4 x 1 layout (the W2 instantiations of this mode measured 78.2 against 78.4 ms per step -- it is bound by the
// transform's vector work, not by the operand reads -- and are not built)
void launch_conv16_da_p1(const ConvPlan& p, const ConvArgs& a, int B, hipStream_t s) {
    KX_REQUIRE(p.form == FORM_DA && p.p1 && a.prec1 == (p.bf ? 2 : 1), "conv1d f16x3 da p1: not a reduced-precision form");
    if (p.bf) {  // bf16 operands: the bf16 form of the weight image
        KX_REQUIRE(a.w16b != nullptr, "conv1d f16x3 da p1: no bf16 weight image");
        ConvArgs b16 = a;
        b16.w16 = a.w16b;
        launch_da_4x1_bn<true, true>(p, b16, B, s);
        return;
    }
    launch_da_4x1_bn<true, false>(p, a, B, s);
}

}  // namespace kx
