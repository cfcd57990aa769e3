// The plain (residual) form of the layer1 tail that also emits the next block's conv1: kernel body, LDS map and launch checks are in conv_bneck_fold.h,
// shared with the downsample form of conv_bneck_fold_dual.hip. This file instantiates the plain form only (tests/test_l1_fold_host.py compiles it alone).
#include "conv_bneck_fold.h"

using namespace tedspad;

extern "C" int32_t tedspad_bneck_tail_fold_fwd(const tedspad_conv_desc *d2, const void *x, const void *w2_packed, const float *scale2, const float *shift2,
                                               const void *w3p, const float *scale3, const float *shift3, const void *residual, int32_t ldres, void *y,
                                               int32_t ldy, int32_t relu, const void *w1p, const float *scale1, const float *shift1, void *h_next,
                                               int32_t ldh, void *stream) {
    return fold_launch<false>("tedspad_bneck_tail_fold_fwd", d2, x, w2_packed, scale2, shift2, w3p, scale3, shift3, residual, ldres, nullptr, y, ldy, relu, w1p,
                              scale1, shift1, h_next, ldh, stream);
}
