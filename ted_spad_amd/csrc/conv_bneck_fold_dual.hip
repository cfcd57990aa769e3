// The downsample (two-source) form of the layer1 tail that also emits the next block's conv1, layer1.0 -> layer1.1.conv1 on four-frame clips:
//     y  = relu( bn3(conv3(relu(bn2(conv2(h))))) + bn_d(conv_d(x2)) )     (what conv_bneck_tail_kernel<T, DUAL> stores, bit for bit)
//     h' = relu( bn1'(conv1'(y)) )
// Kernel body, LDS map and launch checks are in conv_bneck_fold.h (the DUAL form); this file instantiates that form only.
#include "conv_bneck_fold.h"

using namespace tedspad;

extern "C" int32_t tedspad_bneck_tail_fold2_fwd(const tedspad_conv_desc *d2, const void *x, const void *w2_packed, const float *scale2, const float *shift2,
                                                const void *w3p, const float *scale3, const float *shift3, const void *x2, int32_t ldx2, const float *scale_d,
                                                void *y, int32_t ldy, int32_t relu, const void *w1p, const float *scale1, const float *shift1, void *h_next,
                                                int32_t ldh, void *stream) {
    return fold_launch<true>("tedspad_bneck_tail_fold2_fwd", d2, x, w2_packed, scale2, shift2, w3p, scale3, shift3, x2, ldx2, scale_d, y, ldy, relu, w1p, scale1,
                             shift1, h_next, ldh, stream);
}
