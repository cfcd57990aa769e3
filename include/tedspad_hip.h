/*
 * tedspad_hip.h -- C ABI of libtedspad_hip.so, the MI355X (gfx950) kernels behind the
 * TeD-SPAD video-encoder hot path (I3D clip feature extraction, UNet anonymizer, losses).
 *
 * The reference has NO native layer: every op below is reached there through a stock
 * torch.nn module (cuDNN).  Each entry point cites the reference call it replaces.
 * Conventions:
 *   - plain pointers + sizes, no torch types; all pointers are DEVICE pointers unless
 *     the name says host; `stream` is a hipStream_t passed as void*.
 *   - every function returns 0 on success, a negative TEDSPAD_E* code otherwise and
 *     never throws; tedspad_last_error() gives the message (thread-local).
 *   - no hidden allocation, no synchronisation: launches are asynchronous on `stream`
 *     and are hipGraph-capturable.
 *   - activations are channels-last (N,T,H,W,C) 16-bit (f16 or bf16, see `dtype`),
 *     accumulation and the BN/residual/ReLU epilogue are fp32.
 */
#ifndef TEDSPAD_HIP_H
#define TEDSPAD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TEDSPAD_ABI_VERSION 5   /* 5: tedspad_count_saturated added (round 6); 2: the BatchNorm entries take `zdtype` / `groups` / `dbias`, multi-job refresh entries (round 2); 3: tedspad_conv_extras.nosat / .nchunk_src, the fp32-clip stem entry (round 4); 4: tedspad_bneck_l1_* removed, tedspad_frames_crop_resize_tp added (round 5) */

enum { TEDSPAD_F16 = 0, TEDSPAD_BF16 = 1, TEDSPAD_F32 = 2 /* only where an argument says so (the BatchNorm `zdtype`) */ };
enum { TEDSPAD_OK = 0, TEDSPAD_EINVAL = -1, TEDSPAD_ELAUNCH = -2, TEDSPAD_EUNSUPPORTED = -3 };

/* Geometry of one convolution in channels-last form.  2-D convs (UNet) use t = kt = 1. */
typedef struct tedspad_conv_desc {
    int32_t n, t, h, w;          /* input pixels                                              */
    int32_t cin;                 /* channels read per pixel, multiple of 8                    */
    int32_t ldx;                 /* elements between consecutive input pixels (>= cin)        */
    int32_t cout;                /* output channels written, multiple of 8                    */
    int32_t ldy;                 /* elements between consecutive output pixels (concat slices) */
    int32_t ldres;               /* same for the residual tensor; ignored if residual == NULL */
    int32_t kt, kh, kw;          /* kernel                                                    */
    int32_t st, sh, sw;          /* stride                                                    */
    int32_t pt, ph, pw;          /* FRONT zero padding (TF-SAME is asymmetric: i3d.py:82-106) */
    int32_t to, ho, wo;          /* output pixels                                             */
    int32_t relu;                /* 1: ReLU after scale/shift(+residual)                      */
    int32_t dtype;               /* TEDSPAD_F16 | TEDSPAD_BF16                                */
    int32_t tile_cfg;            /* 0: built-in heuristic; 1..tedspad_conv_num_tile_cfgs(): forced
                                    (the host autotuner's analogue of cudnn.benchmark, train_anonymizer.py:28) */
} tedspad_conv_desc;

typedef struct tedspad_pool_desc {
    int32_t n, t, h, w, c;       /* input, c multiple of 8                                    */
    int32_t ldx, ldy;            /* pixel strides (elements)                                  */
    int32_t kt, kh, kw, st, sh, sw, pt, ph, pw;
    int32_t to, ho, wo;
    int32_t pad_zero;            /* 1: padded taps contribute 0 (MaxPool3dSamePadding, i3d.py:41-45) */
    int32_t dtype;
} tedspad_pool_desc;

int32_t     tedspad_abi_version(void);
const char *tedspad_last_error(void);

/* ---- packing helpers (HOST side, pure CPU) ------------------------------------------------ */

/* K = kt*kh*kw*cin rounded up to the kernel's K tile; rows of the packed weight matrix. */
int32_t tedspad_conv_kpad(const tedspad_conv_desc *d);
int32_t tedspad_conv_cout_pad(const tedspad_conv_desc *d);
/* Number of tile configurations of the conv kernel (valid tile_cfg values are 1..this). */
int32_t tedspad_conv_num_tile_cfgs(void);
/* Number of int32 pairs in the K-chunk table (= kpad / 8). */
int32_t tedspad_conv_ktab_entries(const tedspad_conv_desc *d);
/* Fills host_out[2*entries]: {element offset of the tap+channel chunk, packed (dt,dh,dw,valid)}. */
int32_t tedspad_conv_build_ktab(const tedspad_conv_desc *d, int32_t *host_out);

/* ---- device launchers --------------------------------------------------------------------- */

/*
 * y[n,to,ho,wo,co] = act( scale[co] * sum_{dt,dh,dw,ci} x[n, to*st-pt+dt, ..., ci] * w[co][(dt,dh,dw,ci)]
 *                         + shift[co] (+ residual[n,to,ho,wo,co]) )
 * Replaces nn.Conv3d/Conv2d + BatchNorm(eval) + ReLU (+ residual add):
 *   Unit3D.forward            aux_code/models/i3d.py:89-120
 *   Bottleneck.forward        aux_code/models/large_i3d.py:61-84
 *   I3Res50 stem              aux_code/models/large_i3d.py:229-231
 *   DoubleConv / OutConv      aux_code/models/unet_parts.py:8-25,71-77
 * w_packed: [cout_pad][kpad] 16-bit, K ordered (dt,dh,dw,ci), zero padded.
 * ktab: device copy of tedspad_conv_build_ktab.  scale/shift: fp32 [cout_pad].
 * act: relu if d->relu; `sigmoid` != 0 applies a logistic instead (UNet output, unet_model.py:37).
 */
int32_t tedspad_conv_fwd(const tedspad_conv_desc *d, const void *x, const void *w_packed,
                         const int32_t *ktab, const float *scale, const float *shift,
                         const void *residual, void *y, int32_t sigmoid, void *stream);

/* Optional epilogue extras used by the training path (all-zero / NULL = plain tedspad_conv_fwd):
 *   mask   : 16-bit tensor shaped like the output; out = mask > 0 ? out : 0. Fuses the ReLU backward
 *            into the data-gradient conv that produces d(input) (the input IS the ReLU output).
 *   stats  : fp32 [2][stats_ld], pre-zeroed; receives per-channel sum and sum of squares of
 *            scale*conv+shift over all output pixels (BatchNorm batch statistics, train mode:
 *            train_anonymizer.py:73,139) via one atomic per channel per workgroup.
 *   out_strided: output pixel (n,to,ho,wo) is written at (n, to*ost+oot, ho*osh+ooh, wo*osw+oow) of a
 *            (tf,hf,wf) tensor: lets the stride-s data gradient run as s^d dense sub-convolutions
 *            (one per output parity class) that interleave their results in place. */
typedef struct tedspad_conv_extras {
    const void *mask;
    float      *stats;
    float      *y32;     /* optional fp32 output (pixel stride ldy32); `y` may then be NULL. Train-mode BatchNorm keeps
                            the pre-normalisation conv output in fp32: rounding it to 16 bits before subtracting the
                            batch mean flips ReLU branches (DESIGN.md "training precision"). */
    int32_t     ldmask, stats_ld, ldy32;
    int32_t     out_strided, ost, osh, osw, oot, ooh, oow, tf, hf, wf;
    int32_t     fold_hw, fold_c, fold_ldy;  /* fold_hw > 0 (tile_cfg 25 / 26 only, plain epilogue): the conv's output channels hold cout / fold_c output FRAMES of
                                fold_c channels: channel n of output row m = sample*fold_hw + px (fold_hw = to*ho*wo) is stored as channel n % fold_c of row
                                (sample * (cout / fold_c) + n / fold_c) * fold_hw + px with row stride fold_ldy (d->ldy is not used); scale / shift are fold_c long; fold_c a multiple of 128 (an epilogue pass of the kernel). Lets a 3x1x1 'same' conv on a
                                2-frame tensor (layer3 / layer4 of I3Res50 after maxpool2) run as ONE GEMM with K = 2*cin over both frames -- out[0] =
                                [W1 W2].[x0;x1], out[1] = [W0 W1].[x0;x1] -- instead of K = 3*cin with a third of the products on zero padding */
    int32_t     stats_rows;  /* 0: one set of statistics over all output rows. > 0 (>= 256): output rows [g*stats_rows, (g+1)*stats_rows) are
                                statistics GROUP g and accumulate into stats + g*2*stats_ld -- the three clips of a training step run through the
                                network as ONE batch while their BatchNorms keep separate batch statistics (train_anonymizer.py:169-175) */
    int32_t     nosat;       /* 1: f16 results are NOT clamped to +-65504 (the training path: an overflow stays inf / NaN, as under the reference's fp16
                                autocast, train_anonymizer.py:78, so that a loss scale's non-finite check sees it). 0: saturate (inference) */
    int32_t     nchunk_src;  /* > 0 (= cin / 64, <= 8; tile_cfg 32 / 33 only, kt = 1): the input is a GATHERED CONCATENATION -- the 64-channel chunk k of every
                                input pixel is read from chunk_src[k] (pointer to that chunk's first channel at pixel 0, 16-byte aligned) with pixel stride
                                chunk_ld[k]; bit k of chunk_up: that source is a (n, h/2, w/2) tensor read through a nearest x2 upsample (pixel (h, w) <-
                                (h >> 1, w >> 1); h, w even). `x` / d->ldx are not read. This is `torch.cat([F.interpolate(x, scale_factor=2, mode='nearest'),
                                *skips], dim=1)` of the default anonymizer's decoder blocks (arch='unet++', aux_code/model_loaders.py:17-30; smp
                                decoders/unetplusplus/decoder.py DecoderBlock.forward) without the upsampled tensor or the concat buffer ever being written */
    int32_t     chunk_up;
    int32_t     chunk_ld[8];
    const void *chunk_src[8];
} tedspad_conv_extras;

int32_t tedspad_conv_fwd_ex(const tedspad_conv_desc *d, const void *x, const void *w_packed,
                            const int32_t *ktab, const float *scale, const float *shift,
                            const void *residual, void *y, int32_t sigmoid,
                            const tedspad_conv_extras *ex, void *stream);

/* Bottleneck tail + temporal max-pool in one launch: y = MaxPool3d((2,1,1), stride (2,1,1)) of
 * ReLU(conv1x1x1(x)*scale + shift + residual) -- `bn3 / += residual / relu` of the last layer1 block followed by
 * `maxpool2` (large_i3d.py:77-84,139,235). `d` describes the convolution (1x1x1, stride 1, cin 64 or 128, to/ho/wo = its
 * own output extent); y is (n, t/2, h, w) with pixel stride d->ldy. Persistent kernel of tile_cfg 19: the un-pooled
 * tensor is never written. */
int32_t tedspad_conv_pool_t2_fwd(const tedspad_conv_desc *d, const void *x, const void *w_packed, const float *scale,
                                 const float *shift, const void *residual, void *y, void *stream);

/* First bottleneck of a stage whose two branches are both 1x1x1 stride-1 convs with cin = 64 (layer1.0 of I3Res50):
 * y = ReLU((conv(x, w)*scale + shift) + (conv(x2, w2)*scale2 + shift2)) -- `bn3(conv3(out))`, `downsample(x)`, `+=`, `relu`
 * of large_i3d.py:77-84 in one persistent launch (tile_cfg 19's kernel with two sources): the downsample tensor is never
 * written. `d` describes the first conv (cin = 64; d->relu applies to the sum); x2 has the same pixel grid, pixel stride
 * ldx2, 64 channels; both weight matrices are packed [cout_pad][64]. Each branch is accumulated and scaled in fp32. */
int32_t tedspad_conv_pw_dual_fwd(const tedspad_conv_desc *d, const void *x, const void *w_packed, const float *scale,
                                 const float *shift, const void *x2, int32_t ldx2, const void *w2_packed,
                                 const float *scale2, const float *shift2, void *y, void *stream);

/* First bottleneck of layer2/3/4 (large_i3d.py:77-84 with a STRIDED downsample branch) as one GEMM on the ping-pong kernel:
 * y = act([W3*s3 | Wd*sd] . [x ; x2 sampled with stride (sh2, sw2)] + shift). `d` describes the first conv (1x1x1, stride 1,
 * cin % 64 == 0, cout % 256 == 0); x2 is (n, t, h2, w2) with cin2 % 64 == 0 channels and pixel stride ldx2; w_packed is the
 * [cout_pad][cin + cin2] matrix with the BatchNorm scales already folded into the rows (scale = ones, shift = b3 + bd). */
int32_t tedspad_conv_p8_dual_fwd(const tedspad_conv_desc *d, const void *x, const void *x2, int32_t cin2, int32_t ldx2, int32_t h2, int32_t w2,
                                 int32_t sh2, int32_t sw2, const void *w_packed, const float *scale, const float *shift, void *y,
                                 void *stream);

/* Tail of a layer1 bottleneck in one launch (csrc/conv_bneck.hip; aux_code/models/large_i3d.py:49-54,69-84):
 *     y = act( bn3(conv3(relu(bn2(conv2(x))))) + residual )                         (plain block)
 *     y = act( bn3(conv3(relu(bn2(conv2(x))))) + bn_d(conv_d(x2)) )                 (first block: downsample branch, stride 1)
 * conv2 = `d2`: a stride-1 'same' 1 x kh x kw convolution with 64 input and 64 output channels (weights `w2_packed` in the
 * tedspad_conv_fwd layout, BatchNorm folded to scale2 / shift2); conv3 / conv_d are 1x1x1 with 64 input channels and cout3 (a multiple of
 * 64, <= 512) output channels. `w3p` is [cout3][KB * 64] 16-bit (KB = 2 with the second source): columns
 * ((a*2 + s)*2 + h)*8 + j = conv3 weight of input channel 32 a + 16 s + 8 (j >> 2) + 4 h + (j & 3) (the k order in which an MFMA
 * accumulator tile is consumed as the next MFMA's operand), columns 64 + c = conv_d weight of input channel c. scale3 / scale_d are the two
 * BatchNorm scales, shift3 the sum of the shifts. The 64-channel tensor between conv2 and conv3 is never written.
 * Residual and result rows go through wave-private LDS images, so that every global access moves whole 128-byte lines (variant bits 0 / 1, which
 * selected that form until ABI 3, are ignored).
 * variant bit 2 (plain block only, t even): MaxPool3d((2,1,1), stride (2,1,1)) of the block's output fused (large_i3d.py:139):
 * y[n][t/2][h][w][ldy] = max over the frame pair; a workgroup runs conv2 for the same 256 pixels of both frames and stores once. */
int32_t tedspad_bneck_tail_fwd(const tedspad_conv_desc *d2, const void *x, const void *w2_packed, const float *scale2, const float *shift2,
                               const void *w3p, const float *scale3, const float *shift3, int32_t cout3, const void *residual, int32_t ldres,
                               const void *x2, int32_t ldx2, const float *scale_d, void *y, int32_t ldy, int32_t relu, int32_t variant, void *stream);

/* The plain block's tail above AND the next block's conv1 in one launch (csrc/conv_bneck_fold.hip) -- replaces, for two consecutive layer1
 * bottlenecks on four-frame clips, the tail of the first `Bottleneck.forward` and the head of the second (aux_code/models/large_i3d.py:61-84:
 * lines 69-84 of block i, then lines 61-68 of block i + 1):
 *     y      = act( bn3(conv3(relu(bn2(conv2(x))))) + residual )        bit-identical to tedspad_bneck_tail_fwd's
 *     h_next = relu( bn1'(conv1'(y)) )                                  conv1' 3x1x1, stride 1, pads (1,0,0), 256 -> 64
 * so that `y` is not read a third time only to make the 64-channel h_next. d2 as above with t == 4, a 1 x 3 x 3 kernel and pads (0,1,1),
 * any h and w: a workgroup owns an 8 x 8 pixel patch (partial at the right / bottom edge) across the four frames of a clip, one frame per wave, and the temporal
 * neighbours of a pixel are read from the sibling waves' LDS row images. cout3 is 256; w3p as above (64 columns).
 * `w1p` is [4][3][64][64] 16-bit: tile (g, dt) = conv1' weights of output channels 0..63 (rows) against input channels 64 g .. 64 g + 63 at
 * temporal tap dt; the columns of the dt = 1 tiles are in the accumulator k order of w3p, those of dt = 0 and 2 in natural order.
 * scale1 / shift1: bn1' folded, 64 floats each. h_next is (n,4,h,w,ldh). */
int32_t tedspad_bneck_tail_fold_fwd(const tedspad_conv_desc *d2, const void *x, const void *w2_packed, const float *scale2, const float *shift2,
                                    const void *w3p, const float *scale3, const float *shift3, const void *residual, int32_t ldres, void *y,
                                    int32_t ldy, int32_t relu, const void *w1p, const float *scale1, const float *shift1, void *h_next, int32_t ldh,
                                    void *stream);

/* The same for a block WITH the downsample branch, layer1.0 -> layer1.1's conv1 (csrc/conv_bneck_fold_dual.hip; large_i3d.py:49-54 in place of the residual):
 *     y      = act( bn3(conv3(relu(bn2(conv2(x))))) + bn_d(conv_d(x2)) )     bit-identical to tedspad_bneck_tail_fwd's two-source form
 *     h_next = relu( bn1'(conv1'(y)) )
 * x2 is (n,4,h,w,ldx2) with 64 channels, w3p is the two-source image of tedspad_bneck_tail_fwd ([256][128]: conv3 columns in accumulator k order, then the
 * downsample columns in natural order), shift3 holds b3 + bd and scale_d the downsample BatchNorm's scale (256 floats). Everything else as above. */
int32_t tedspad_bneck_tail_fold2_fwd(const tedspad_conv_desc *d2, const void *x, const void *w2_packed, const float *scale2, const float *shift2,
                                     const void *w3p, const float *scale3, const float *shift3, const void *x2, int32_t ldx2, const float *scale_d, void *y,
                                     int32_t ldy, int32_t relu, const void *w1p, const float *scale1, const float *shift1, void *h_next, int32_t ldh,
                                     void *stream);

/* WHOLE bottleneck of a plain I3Res50 layer3 block (csrc/conv_bneck_frame.hip) -- replaces the `Bottleneck.forward` of
 * aux_code/models/large_i3d.py:61-84 for blocks without `downsample` on 14 x 14 frames (cin = 1024, cmid = 256):
 *     y = act( bn3(conv3( relu(bn2(conv2( relu(bn1(conv1(x))) ))) )) + x )
 * conv1 1x1x1 (steps1 = cin / 32) or 3x1x1 'same' on TWO-frame clips in its folded form (steps1 = 2 * cin / 32, t == 2: output frame f =
 * Wa . x[frame 0] + Wb . x[frame 1] with (Wa, Wb) = (W[:,:,1], W[:,:,2]) for f = 0 and (W[:,:,0], W[:,:,1]) for f = 1); conv2 1x3x3 stride 1 pad 1;
 * conv3 1x1x1. One workgroup owns a whole frame; both cmid-channel tensors stay in LDS. x / y: (n, t, h, w, cin) 16-bit channels-last with pixel
 * strides ldx / ldy (y must not alias x).
 * Weights are streams of 16 KB SLOT IMAGES, one per 32-deep K step and 256 output channels: for a matrix Wm[rows][K], row block rb, K step ks
 *     img[wc 0..3][j 0..3][lane 0..63][kk 0..7] = Wm[256 rb + 64 wc + r(j, lane & 15)][32 ks + 8 (lane >> 4) + kk]
 * (lane-linear v_mfma_f32_16x16x32 fragments) with r(j, i) = 16 (i >> 2) + 4 j + (i & 3) for conv1 / conv2 (a lane ends with 16 consecutive channels of a pixel:
 * the LDS rows of the mid tensors) and r(j, i) = 4 i + j for conv3 (weights as the B operand: consecutive lanes end with consecutive channels, so residual
 * loads and stores are fully coalesced).
 *   w1_even / w1_odd: steps1 images of conv1 for even / odd frames (the same buffer twice for the 1x1x1 form), K = ci (folded form: frame * cin + ci);
 *   w23: 72 images of conv2 (K = (dh*3 + dw) * cmid + ci), 4 x 8 images of conv3 (row block = 256 output channels, K = ci) and 2 padding images (the ring
 *        fetches two steps past the end).
 * scale / shift: the three folded BatchNorms (cmid, cmid, cin floats, 16-byte aligned). ldy must equal ldx; relu must be non-zero (large_i3d.py:84). */
int32_t tedspad_bneck_frame_fwd(const void *x, int32_t ldx, void *y, int32_t ldy, int32_t n, int32_t t, int32_t h, int32_t w, int32_t cin, int32_t cmid,
                                const void *w1_even, const void *w1_odd, int32_t steps1, const void *w23, const float *scale1, const float *shift1,
                                const float *scale2, const float *shift2, const float *scale3, const float *shift3, int32_t relu, int32_t dtype,
                                void *stream);
int32_t tedspad_bneck_frame_lds_bytes(void);   /* dynamic LDS of the kernel above (one workgroup per CU) */

/* Measurement aid (bench.py `roofline.peak_at_clock`): `workgroups` x 256 threads run 4 x iters v_mfma_f32_32x32x16_f16 per wave; workgroup b writes
 * out[2b] = elapsed shader cycles (s_memtime) and out[2b+1] = elapsed 100 MHz ticks (s_memrealtime): the sustained clock under matrix load is
 * 100 MHz x out[2b] / out[2b+1]. out: 2 x workgroups uint64. */
int32_t tedspad_clock_probe(int32_t iters, int32_t workgroups, void *out, void *stream);

/* Deterministic mode for the training kernels (the reference has no such switch: torch's convolution backward is non-deterministic too unless
 * torch.use_deterministic_algorithms is set). on != 0: the workgroups of a launch pass through their float-atomic sections -- BatchNorm batch statistics in
 * the conv epilogues (tedspad_conv_fwd_ex with `stats`), the channel sums of tedspad_bn_bwd_reduce, the weight-gradient flush of tedspad_conv_wgrad -- one at a
 * time, in blockIdx order (csrc/det_gate.h): bit-identical sums from run to run, at the price of serialising those sections. The caller must keep such
 * launches of one kernel family off concurrent streams, use fixed tile configurations, and form a conv bias gradient with tedspad_bn_bwd_reduce instead of
 * tedspad_bn_bwd_apply's fused one (ted_spad_amd.engine.set_deterministic does all of it). Synchronises the device. tedspad_deterministic_giveups: how many
 * workgroups stopped waiting for their turn since the mode was set (0 unless something is wrong; results are then not reproducible, nothing hangs). */
int32_t tedspad_set_deterministic(int32_t on);
int32_t tedspad_deterministic_giveups(void);

/* Persistent Cin = 3 stem (csrc/conv_stem_pt.hip): conv1 5x7x7 / stride 2 / pad (2,3,3) + bn1 + ReLU of large_i3d.py:133-137,229-231
 * with the temporal half of maxpool1 (MaxPool3d((2,3,3), 2), large_i3d.py:138,232) fused: y[n][to/2][ho][wo][64] =
 * max over the output frame pair (to, to+1) of act(conv * scale + shift); the spatial 3x3 / 2 half of the pool is a
 * tedspad_maxpool_fwd with kt = 1 on y.
 * tedspad_clip_to_tp lays the fp32 (n, c <= 3, t, h, w) clip (W even) out as x_tp[n][tp][h][b][w/2][24] 16-bit: the 48-byte record of
 * pixel (h, 2*wq + b) for output-frame pair tp holds value dt*3 + ci = x[n][ci][4*tp - pad_t + dt][h][2*wq + b], dt = 0..7, zeros
 * outside the clip (stride_t = 2). Output frame 2*tp reads the 32 bytes at offset 0 of a record, frame 2*tp + 1 those at offset 12.
 * w_img (tedspad_stem_pt_wimg_bytes() bytes): [tap = dh*7 + dw][co 0..63][half][8] 16-bit, value v = dt*3 + ci (zero for v >= kt*3)
 * of half v / 8, the two halves of a row stored swapped when (co >> 4) & 1 (the kernel's conflict-free LDS image, copied linearly).
 * t_pairs = output frame pairs (floor(To / 2)); ho = ceil(h / 2), wo = w / 2; nwg = persistent workgroups (0: 256);
 * variant bit 1: 8 waves per workgroup, the output channels split between the two waves of a SIMD (same results); bits 8-10:
 * timing ablations (wrong results, see the kernel). */
int32_t tedspad_clip_to_tp(const float *x, void *x_tp, int32_t n, int32_t c, int32_t t, int32_t h, int32_t w, int64_t sn, int64_t sc,
                           int64_t st, int64_t sh, int64_t sw, int32_t pad_t, int32_t stride_t, int32_t t_pairs, int32_t dtype, void *stream);
int32_t tedspad_stem_pt_wimg_bytes(void);
int32_t tedspad_stem_pt_fwd(const void *x_tp, const void *w_img, const float *scale, const float *shift, void *y, int32_t n, int32_t t_pairs,
                            int32_t h, int32_t w, int32_t ho, int32_t wo, int32_t ldy, int32_t relu, int32_t nwg,
                            int32_t variant, int32_t dtype, void *stream);
/* The same stem with the WHOLE maxpool1 fused (MaxPool3d((2,3,3), stride 2, no padding), large_i3d.py:138,232): ReLU always;
 * y[n][t_pairs][hp][wp][ldy], hp = (ceil(h/2) - 3) / 2 + 1, wp = (w/2 - 3) / 2 + 1. Workgroups walk column strips of 8 x 16 patches top
 * to bottom, pool each patch over columns in registers and over rows through LDS (the rows a window shares with the patch above are
 * carried); the pooled column a patch shares with its right neighbour is joined by a second small launch from `side`
 * (tedspad_stem_pt_side_bytes() bytes of scratch, 16-byte aligned). The 112 x 112 stem tensor never reaches HBM. */
/* variant bit 2 (with the 8 waves of bit 1): the same taps on v_mfma_f32_16x16x32 -- one MFMA sums a PAIR of taps (K = 32); the chip holds a ~12 % higher
 * clock on that shape under load. w_img then is the tap-pair image (tedspad_stem_pt_wimg16_bytes() bytes): [pair 0..24][co][chunk q][8] 16-bit with chunk
 * q = 2 * (tap of the pair) + (8-value half of its 16 values dt*3 + ci), chunk q of row co stored at chunk q ^ (2 * ((co >> 3) & 1)); pairs in the order
 * phase 0 (dh even): ((dh, 1), (dh, 2)), ((dh, 3), (dh, 4)), ((dh, 5), (dh, 6)) for dh = 0, 2, 4, 6, then ((0, 0), (2, 0)), ((4, 0), (6, 0)); phase 1 (dh odd)
 * likewise for dh = 1, 3, 5, then ((1, 0), (3, 0)), ((5, 0), zeros). Sums the 49 taps in another order than the 32x32x16 form (fp32: one f16 step apart). */
int32_t tedspad_stem_pt_wimg16_bytes(void);
int64_t tedspad_stem_pt_side_bytes(int32_t n, int32_t t_pairs, int32_t h, int32_t w);
int32_t tedspad_stem_pt_pool_fwd(const void *x_tp, const void *w_img, const float *scale, const float *shift, void *y, void *side, int32_t n,
                                 int32_t t_pairs, int32_t h, int32_t w, int32_t hp, int32_t wp, int32_t ldy, int32_t nwg, int32_t variant,
                                 int32_t dtype, void *stream);
/* The pool-fused 16x16x32 stem WITHOUT the layout pass: x is the fp32 (n, c, t, h, w) clip batch exactly as the reference hands it to
 * `I3Res50.extract_features` / `forward` (large_i3d.py:229-232,251-254; produced by dali_extraction.py:38-50 / st_feature_extraction.py:18-26), element
 * strides sn, sc, st, sh, sw = 1, rows 16-byte aligned (w % 4 == 0, x and every stride multiples of 4 elements). The persistent workgroups build their halo
 * images from it themselves (register-staged 16-byte loads requested a whole patch ahead, converted to the 16-bit dtype on the way into LDS): the 9.6 MB
 * per clip of tedspad_clip_to_tp records are never written or read. Same arithmetic, same results as tedspad_clip_to_tp + tedspad_stem_pt_pool_fwd(variant 6).
 * w_img16: the tap-pair image; variant bit 3: the loader waves deal their tasks per LANE (every load behind per-lane plane guards and address arithmetic) instead
 * of one (frame, half) per WAVE with scalar guards and buffer loads -- same results, kept for A/B and as the fallback for row strides past the buffer loads' range
 * (TEDSPAD_STEM_UNIFORM=0 sets the bit for every call); bits 8..10 timing ablations only. */
int32_t tedspad_stem_pt_pool_clip_fwd(const float *x, int32_t n, int32_t c, int32_t t, int32_t h, int32_t w, int64_t sn, int64_t sc, int64_t st, int64_t sh,
                                      int64_t sw, int32_t pad_t, int32_t stride_t, int32_t t_pairs, const void *w_img16, const float *scale,
                                      const float *shift, void *y, void *side, int32_t hp, int32_t wp, int32_t ldy, int32_t nwg, int32_t variant,
                                      int32_t dtype, void *stream);

/* The block that ends the default anonymizer's decoder (arch = 'unet++', aux_code/model_loaders.py:17-30; smp 0.3.3 UnetPlusPlusDecoder blocks['x_0_3'] =
 * DecoderBlock(64, 0, 32) followed by SegmentationHead(32, 3, kernel_size 3)) in ONE launch, at full resolution:
 *     y = conv3x3(relu(bn(conv3x3(relu(bn(conv3x3(interpolate(x, 2, 'nearest'))))))) ) + bias         64 -> 32 -> 32 -> 3
 * x: (n, h/2, w/2, 64) channels-last 16-bit, pixel stride ldx; y: (n, 3, h, w) fp32 NCHW (the model's output as the extraction loops consume it,
 * dali_extraction.py:169-173); both 32-channel tensors stay in LDS. w_img: tedspad_unetpp_tail_wimg_bytes() bytes, the three weight tensors in the kernel's
 * LDS image: [hc 2][tap 9][co 32][32 ci] | [tap 9][co 32][32 ci] | [tap 9][co 16 (3 used)][32 ci] 16-bit, the four 16-byte pieces of a 64-byte row stored at
 * piece ^ ((co >> 1) & 3) (unetpp.py packs it); scale / shift: the folded BatchNorms (32 values each), bias3: 3 values. */
int32_t tedspad_unetpp_tail_wimg_bytes(void);
int32_t tedspad_unetpp_tail_fwd(const void *x, int32_t ldx, float *y, int32_t n, int32_t h, int32_t w, const void *w_img, const float *scale1,
                                const float *shift1, const float *scale2, const float *shift2, const float *bias3, int32_t dtype, void *stream);

/* Weight gradient: dw[co][k] += sum over output pixels of dy[m][co] * x[m @ tap(k)][ci(k)], fp32, in the
 * packed [cout_pad][kpad] layout of the forward weights (k ordered (dt,dh,dw,ci)). `dw` must be
 * zeroed by the caller (hipMemsetAsync on the same stream); accumulation uses float atomics.
 * `d` is the FORWARD descriptor of the convolution (d->ldy = pixel stride of dy). Replaces the
 * autograd of nn.Conv3d/Conv2d in loss.backward(): train_anonymizer.py:122,190-191. */
int32_t tedspad_conv_wgrad(const tedspad_conv_desc *d, const void *x, const void *dy, const int32_t *ktab,
                           float *dw, void *stream);

/* nn.MaxPool3d / MaxPool3dSamePadding / nn.MaxPool2d: large_i3d.py:138-139, i3d.py:13-45, unet_parts.py:34 */
int32_t tedspad_maxpool_fwd(const tedspad_pool_desc *d, const void *x, void *y, void *stream);
/* Same, also recording the window-local index of the FIRST maximum of every output element
 * (uint8, laid out (n,to,ho,wo,c) contiguous) for tedspad_maxpool_bwd. This is the TRAINING forward: like torch's
 * max_pool3d it hands non-finite values on -- +-inf is not clamped to the largest finite value, a NaN in a window gives NaN
 * (index: the last NaN of the window, as torch) -- so that an overflow reaches the loss scale's non-finite check
 * (tedspad_conv_extras.nosat); tedspad_maxpool_fwd keeps the saturating inference semantics. pad_zero = 1 together with
 * `idx` is used by no training path and is not covered by the op-level tests. */
int32_t tedspad_maxpool_fwd_idx(const tedspad_pool_desc *d, const void *x, void *y, uint8_t *idx, void *stream);

/* AdaptiveAvgPool3d(1) / AvgPool3d([2,7,7]) over `spatial` pixels: large_i3d.py:146,262; i3d.py:293,340.
 * x: (n, spatial, c) 16-bit with pixel stride ldx -> y fp32 (n, c). */
int32_t tedspad_global_avgpool_fwd(const void *x, float *y, int32_t n, int32_t spatial, int32_t c,
                                   int32_t ldx, int32_t dtype, void *stream);

/* nn.AvgPool3d(kernel_size=[kt,kh,kw], stride=(1,1,1)) of InceptionI3d.extract_features (aux_code/models/i3d.py:293-295,336-340) on a
 * Mixed_5c map larger than the kernel: x (n,t,h,w,c) 16-bit channels-last, pixel stride ldx -> y fp32 (n,c,t-kt+1,h-kh+1,w-kw+1). */
int32_t tedspad_avgpool3d_s1_fwd(const void *x, float *y, int32_t n, int32_t t, int32_t h, int32_t w, int32_t c, int32_t ldx, int32_t kt,
                                 int32_t kh, int32_t kw, int32_t dtype, void *stream);

/* fp32 NCTHW clip (as ft.extract_features takes it: large_i3d.py:249) -> 16-bit NTHWC with the
 * channel dim zero-padded to cpad (4: stem pixel-pair form; 8: UNet).  x strides in elements. */
int32_t tedspad_clip_to_channels_last(const float *x, void *y, int32_t n, int32_t c, int32_t t,
                                      int32_t h, int32_t w, int64_t sn, int64_t sc, int64_t st_,
                                      int64_t sh, int64_t sw, int32_t cpad, int32_t dtype, void *stream);

/* 16-bit NTHWC (pixel stride ldx, first c channels) -> fp32 NCTHW contiguous (module boundary out). */
int32_t tedspad_channels_last_to_nchw(const void *x, float *y, int32_t n, int32_t c, int32_t t,
                                      int32_t h, int32_t w, int32_t ldx, int32_t dtype, void *stream);

/* y[b,n] = act( scale[n] * sum_k x[b,k] * w[n,k] + shift[n] ), all fp32 (scale/shift may be NULL).
 * Replaces nn.Linear (+ BatchNorm1d eval + ReLU): I3Res50.fc large_i3d.py:147,245; mlp.fc1/bn1/fc2/bn2
 * aux_code/model_loaders.py:242-253. */
int32_t tedspad_linear_fwd(const float *x, const float *w, const float *scale, const float *shift, float *y,
                           int32_t B, int32_t K, int32_t N, int32_t relu, void *stream);

/* y[b,:] = x[b,:] / max(||x[b,:]||_2, eps): nn.functional.normalize(p=2, dim=1), model_loaders.py:253. */
int32_t tedspad_l2_normalize_rows(const float *x, float *y, int32_t B, int32_t N, float eps, void *stream);

/* nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True) + F.pad to the skip size
 * (unet_parts.py:50,56-62), written straight into its channel slice of the concat buffer (:67).
 * x: (n,h,w,c) pixel stride ldx -> y: (n,ho,wo,c) pixel stride ldy; rows/cols outside
 * [pad_top, pad_top+2h) x [pad_left, pad_left+2w) are zero-filled. */
int32_t tedspad_upsample_bilinear2x_fwd(const void *x, void *y, int32_t n, int32_t h, int32_t w, int32_t c,
                                        int32_t ldx, int32_t ldy, int32_t ho, int32_t wo, int32_t pad_top,
                                        int32_t pad_left, int32_t dtype, void *stream);

/* ---- losses of the anonymizer training step: value AND input gradients in one launch ---------- */

/* NTXentLoss(device, N, temperature, use_cosine)(zis, zjs)  -- aux_code/nt_xent_original.py:49-70.
 * zis, zjs: fp32 (N, C); loss: fp32[1]; dzis/dzjs: fp32 (N, C) = dloss/dz (both or neither NULL).
 * 2N <= 64, even C <= 256 (reference call sites: N = 12, C = 128, T = 0.1, dot similarity). */
int32_t tedspad_ntxent_fwd_bwd(const float *zis, const float *zjs, float *loss, float *dzis, float *dzjs,
                               int32_t N, int32_t C, float temperature, int32_t use_cosine, void *stream);

/* nn.TripletMarginLoss(margin, p=2, eps=1e-6), mean reduction -- train_anonymizer.py:349-350,115.
 * a,p,n: fp32 (B, C); row_ws: fp32[B] workspace; da/dp/dn may all be NULL (value only). */
int32_t tedspad_triplet_fwd_bwd(const float *a, const float *p, const float *n, float *loss, float *row_ws,
                                float *da, float *dp, float *dn, int32_t B, int32_t C, float margin, float eps,
                                void *stream);

/* nn.CrossEntropyLoss() (mean) -- train_anonymizer.py:347,107. logits fp32 (B, C), labels int64 (B). */
int32_t tedspad_cross_entropy_fwd_bwd(const float *logits, const int64_t *labels, float *loss, float *row_ws,
                                      float *dlogits, int32_t B, int32_t C, void *stream);

/* Privacy classifier head (privacy_training/train_privacy.py:49-55): nn.Linear(K, N) + nn.BCEWithLogitsLoss() (mean) and their
 * backward in ONE launch -- replaces head.linear, the loss and the three GEMVs of the fc backward (torch: F.linear,
 * F.binary_cross_entropy_with_logits, then addmm / mm / sum in autograd). All fp32, deterministic (no float atomics).
 * f (B, K), W (N, K), bias (N) or NULL, y (B, N) float targets (0/1 or fractional) -> logits (B, N) (NULL: not written),
 * loss fp32[1] = mean over B*N (unscaled). df (B, K), dW (N, K), db (N): all or none; each = gradient x grad_scale.
 * W == NULL: logits mode -- f holds the (B, N) logits (K == N, bias / dW / db NULL), df = d(loss)/d(logits) x grad_scale.
 * B <= 128, N <= 64; with W: K % 4 == 0, f / W / df / dW 16-byte aligned. */
int32_t tedspad_bce_head_fwd_bwd(const float *f, const float *W, const float *bias, const float *y, float *logits, float *loss,
                                 float *df, float *dW, float *db, int32_t B, int32_t K, int32_t N, float grad_scale,
                                 void *stream);

/* ---- training path: train-mode BatchNorm around the conv kernels, backward of the pooling / resize ops ----
 * Reference: autograd of the torch.nn modules of aux_code/models/{large_i3d,unet_parts}.py under
 * fa_model.train() / ft_model.train() (anonymization_training/train_anonymizer.py:73-75,137-139). */

/* tedspad_bn_finalize + tedspad_scale_shift_act as ONE launch: y = act((z - mean) * gamma * invstd + beta (+ res)) with mean / invstd from the
 * batch sums `stats` ([2][stats_ld]: sum, sum of squares over `count` values per channel); writes mean / invstd (C floats each, kept for the
 * backward pass) and updates running_mean / running_var in place (momentum, unbiased variance; NULL: not tracked). z: (pixels, Cz)
 * with Cz >= C channels per pixel (channels >= C come out as 0, whatever z and `res` hold there); zdtype TEDSPAD_F32, or `dtype` (16-bit conv output, ldz % 8 == 0 -- what
 * the reference's autocast region holds in front of its BatchNorms, train_anonymizer.py:78,151; the batch sums come from the conv's fp32
 * accumulators either way). nn.BatchNorm{2,3}d in train() mode. */
int32_t tedspad_bn_train_apply(const void *z, int32_t zdtype, const float *stats, int32_t stats_ld, int64_t count, const float *gamma, const float *beta,
                               float eps, float momentum, float *running_mean, float *running_var, float *mean, float *invstd, int32_t C,
                               const void *res, void *y, int64_t pixels, int32_t Cz, int32_t ldz, int32_t ldres, int32_t ldy, int32_t relu,
                               int32_t groups, int32_t dtype, void *stream);
/* groups (here and in the two backward entries below): the tensors hold `groups` consecutive blocks of `pixels` rows, each normalised with its OWN
 * statistics (stats / sums: [groups][2][ld], mean / invstd: [groups][Cz]); the running statistics take the groups' momentum updates in order. */

/* From the per-channel sum / sum-of-squares the conv epilogue accumulated (tedspad_conv_extras.stats) over
 * `count` pixels: batch mean / biased variance -> scale = gamma*invstd, shift = beta - mean*scale; updates
 * running_mean / running_var in place (momentum, unbiased variance) when they are not NULL. */
int32_t tedspad_bn_finalize(const float *stats, int32_t stats_ld, int64_t count, const float *gamma, const float *beta,
                            float eps, float momentum, float *running_mean, float *running_var, float *scale,
                            float *shift, float *mean, float *invstd, int32_t C, void *stream);

/* y = act(z*scale[c] + shift[c] (+ res)); z fp32 (pixel stride ldz), res / y 16-bit channels-last. */
int32_t tedspad_scale_shift_act(const float *z, const float *scale, const float *shift, const void *res, void *y,
                                int64_t pixels, int32_t C, int32_t ldz, int32_t ldres, int32_t ldy, int32_t relu,
                                int32_t dtype, void *stream);

/* sums[0][c] += sum_px g, sums[1][c] += sum_px g*xhat  with g = dy*(y>0 if relu), xhat = (z-mean)*invstd
 * (second row skipped when z == NULL: plain per-channel sum = bias gradient). `sums` pre-zeroed.
 * relu with y == NULL (units without a residual input): the mask is recomputed as z*s + b > 0 with the forward pass's own s = gamma*invstd,
 * b = beta - mean*s (gamma / beta: C floats) -- the 16-bit output is not re-read (2 of the 8 bytes per element this pass moves). */
int32_t tedspad_bn_bwd_reduce(const void *dy, const void *y, const void *z, int32_t zdtype, const float *mean, const float *invstd,
                              const float *gamma, const float *beta, float *sums, int32_t sums_ld, int64_t pixels, int32_t C, int32_t lddy, int32_t ldy,
                              int32_t ldz, int32_t relu, int32_t groups, int32_t dtype, void *stream);

/* dz = gamma*invstd*(g - sums[0]/M - xhat*sums[1]/M); optionally dres = g (gradient of a fused residual input); y == NULL with relu as above.
 * dbias ([dbias_slots][C] floats, pre-zeroed, may be NULL): the rows together += sum over pixels of dz -- the gradient of the bias of the conv
 * in front of the BatchNorm (nn.Conv2d(bias=True) + BatchNorm2d in unet_parts.py DoubleConv), gathered here instead of by another pass over dz;
 * workgroup b adds into row b % dbias_slots (several rows: thousands of atomics on one address serialise), the caller sums the rows.
 * C <= 3520 (the kernel keeps 16 bytes of folded terms per channel in LDS). */
int32_t tedspad_bn_bwd_apply(const void *dy, const void *y, const void *z, int32_t zdtype, const float *mean, const float *invstd,
                             const float *gamma, const float *beta, const float *sums, int32_t sums_ld, void *dz, void *dres,
                             float *dbias, int32_t dbias_slots, int64_t pixels, int32_t C, int32_t lddy, int32_t ldy, int32_t ldz, int32_t lddz,
                             int32_t lddres, int32_t relu, int32_t groups, int32_t dtype, void *stream);

/* dx[i] = (add ? add[i] : 0) + sum over pooling windows o containing i of dy[o]*[argmax(o) == i]; `d` = forward
 * desc, idx from tedspad_maxpool_fwd_idx (first maximum wins, as torch). relu_mask != 0 additionally zeroes dx
 * where x <= 0 (x is a ReLU output: folds that ReLU's backward in). */
int32_t tedspad_maxpool_bwd(const tedspad_pool_desc *d, const void *x, const uint8_t *idx, const void *dy, int32_t lddy,
                            const void *add, int32_t ldadd, void *dx, int32_t lddx, int32_t relu_mask, void *stream);

/* dx[n,p,c] = dfeat[n,c] / spatial, zeroed where mask <= 0 (mask may be NULL). */
int32_t tedspad_global_avgpool_bwd(const float *dfeat, const void *mask, int32_t ldmask, void *dx, int32_t n,
                                   int32_t spatial, int32_t c, int32_t lddx, int32_t dtype, void *stream);

/* F.interpolate(scale_factor=2, mode="nearest") of the UNet++ decoder blocks (segmentation_models_pytorch 0.3.3,
 * decoders/unetplusplus/decoder.py, DecoderBlock.forward; the anonymizer of model_loaders.py:17-30), written straight into its channel
 * slice of the block's concat buffer: y[n][2h+a][2w+b][0..c) = x[n][h][w][0..c), 16-bit elements, pixel strides ldx / ldy.
 * tedspad_copy_channels copies a channel slice (npix pixels x c channels) between two channels-last buffers: the dense skip pathway
 * concatenates some tensors into two different blocks' inputs (torch.cat in UnetPlusPlusDecoder.forward). */
int32_t tedspad_upsample_nearest2x_fwd(const void *x, void *y, int32_t n, int32_t h, int32_t w, int32_t c, int32_t ldx, int32_t ldy,
                                       void *stream);
int32_t tedspad_copy_channels(const void *x, void *y, int64_t npix, int32_t c, int32_t ldx, int32_t ldy, void *stream);
/* Their backward passes (the autograd of F.interpolate(nearest) and of a tensor with several consumers; the train-mode anonymizer,
 * train_anonymizer.py:73-123): dx[n][h][w] (+)= the fp32 sum of the 2 x 2 block of dy; y[:, 0..c) += x[:, 0..c). */
int32_t tedspad_upsample_nearest2x_bwd(const void *dy, void *dx, int32_t n, int32_t h, int32_t w, int32_t c, int32_t ldy, int32_t ldx,
                                       int32_t accumulate, int32_t dtype, void *stream);
int32_t tedspad_add_channels(const void *x, void *y, int64_t npix, int32_t c, int32_t ldx, int32_t ldy, int32_t dtype, void *stream);

/* Backward of tedspad_upsample_bilinear2x_fwd: dy is the (n,ho,wo,c) slice the forward wrote, dx is (n,h,w,c). */
int32_t tedspad_upsample_bilinear2x_bwd(const void *dy, void *dx, int32_t n, int32_t h, int32_t w, int32_t c,
                                        int32_t lddy, int32_t lddx, int32_t ho, int32_t wo, int32_t pad_top,
                                        int32_t pad_left, int32_t dtype, void *stream);

/* fp32 (n,c,thw) gradient -> 16-bit (n,thw,8) channels-last; if y_sigmoid != NULL multiplies by y*(1-y)
 * (backward of the UNet's sigmoid output, unet_model.py:37). */
int32_t tedspad_nchw_grad_to_channels_last(const float *dy, const float *y_sigmoid, void *out, int32_t n, int32_t c,
                                           int64_t thw, int32_t dtype, void *stream);

/* 16-bit (n,t,h,w,ldx) first c channels -> fp32 tensor with arbitrary element strides (gradient w.r.t. a clip view). */
int32_t tedspad_channels_last_to_nchw_strided(const void *x, float *y, int32_t n, int32_t c, int32_t t, int32_t h,
                                              int32_t w, int32_t ldx, int64_t sn, int64_t sc, int64_t st_, int64_t sh,
                                              int64_t sw, int32_t dtype, void *stream);

/* ---- fp32 head ops of the training step (B x C matrices with tiny B): mlp / fc of wrapper_i3d ---- */
/* nn.BatchNorm1d in train mode (+ ReLU): model_loaders.py:252-253 under ft_model.train(). */
int32_t tedspad_bn1d_train_fwd(const float *x, const float *gamma, const float *beta, float eps, float momentum,
                               float *running_mean, float *running_var, float *y, float *mean, float *invstd,
                               int32_t B, int32_t C, int32_t relu, void *stream);
int32_t tedspad_bn1d_train_bwd(const float *dy, const float *x, const float *y, const float *mean, const float *invstd,
                               const float *gamma, float *dx, float *dgamma, float *dbeta, int32_t B, int32_t C,
                               int32_t relu, void *stream);
/* backward of tedspad_l2_normalize_rows (x = its INPUT). */
int32_t tedspad_l2_normalize_rows_bwd(const float *x, const float *dy, float *dx, int32_t B, int32_t N, float eps,
                                      void *stream);
/* out = a * b * scale (dropout mask application: I3Res50.drop, large_i3d.py:148,242). */
int32_t tedspad_mul_f32(const float *a, const float *b, float *out, int64_t n, float scale, void *stream);

/* Device-side weight packing: fp32 (co, ci, kt, kh, kw) parameter -> the 16-bit [rows_pad][kpad] matrix of
 * tedspad_conv_fwd. mode 0: forward matrix (rows = co; K ordered (dt,dh,dw,c) over the kernel-form channels
 * cink / width taps kwk; pair_shift >= 0 selects the stem's pixel-pair form, -1 plain zero-padded channels).
 * mode 1: data-gradient matrix of one parity class (rows = kernel-form input channels, K ordered (et,eh,ew,co));
 * dgrad_geo = host int32[9] {Et,Eh,Ew, ct,ch,cw, st,sh,sw}: tap = c + s*(E-1-e) per dim. `scale` (per co, may be
 * NULL) is multiplied in (folded eval-mode BatchNorm). */
int32_t tedspad_pack_conv_weights(const float *w, const float *scale, void *out, int32_t co, int32_t ci, int32_t kt,
                                  int32_t kh, int32_t kw, int32_t cink, int32_t kwk, int32_t pair_shift, int32_t mode,
                                  int32_t rows, int32_t rows_pad, int32_t kpad, const int32_t *dgrad_geo, int32_t dtype,
                                  void *stream);

/* ---- multi-job weight refresh (csrc/pack.hip) -------------------------------------------------------------------
 * After an optimizer step every 16-bit weight image of the updated network is stale: the reference simply reads its fp32
 * parameters again (nn.Conv3d / FrozenBN in large_i3d.py:8-38, 61-84; train_anonymizer.py:123,193 `optimizer.step()`), here the
 * images and the folded BatchNorm vectors are rewritten IN PLACE by ONE launch per kind, from a job table that stays on the
 * device (every address in it is static). `jobs`: HOST array (the library validates it and fills block0 / nblocks);
 * `table_dev`: njobs * sizeof(job) device bytes; upload != 0 copies jobs -> table_dev on `stream` first (needed once, and again
 * only when a job changed). */
typedef struct tedspad_pack_job {           /* one tedspad_pack_conv_weights call */
    const float *w, *scale;
    void *out;
    int32_t co, ci, kt, kh, kw, cink, kwk, pair_shift, mode, rows, rows_pad, kpad;
    int32_t geo[9];                         /* mode 1 (data gradient): {Et,Eh,Ew, ct,ch,cw, st,sh,sw} */
    int32_t dtype;
    int32_t block0, nblocks;                /* filled by the library */
} tedspad_pack_job;
int32_t tedspad_pack_multi(tedspad_pack_job *jobs, int32_t njobs, void *table_dev, int32_t upload, void *stream);

typedef struct tedspad_fold_job {           /* one tedspad_bn_fold call, written zero-padded to n (and n2) floats */
    const float *gamma, *beta, *mean, *var, *conv_bias;   /* gamma NULL: no BatchNorm -- scale = 1, shift = conv_bias (or 0) */
    float *scale, *shift;                   /* n floats each (either may be NULL) */
    float *scale2, *shift2;                 /* optional second copy, n2 floats each */
    double eps;
    int32_t C, n, n2, reserved;
} tedspad_fold_job;
int32_t tedspad_fold_multi(tedspad_fold_job *jobs, int32_t njobs, void *table_dev, int32_t upload, void *stream);

/* packed fp32 weight-gradient accumulators of tedspad_conv_wgrad ([co_pad][kpad], K ordered (dt,dh,dw,c) over cink channels) ->
 * the parameters' gradients in the reference layout (co, ci, kt, kh, kw): grad = (accumulate ? grad : 0) + dw * row_scale[co]. */
typedef struct tedspad_wgrad_unpack_job {
    const float *dw;
    float *grad;
    const float *row_scale;                 /* per output channel, may be NULL */
    int32_t co, ci, kt, kh, kw, cink, kpad, accumulate;
    int32_t block0, nblocks;                /* filled by the library */
} tedspad_wgrad_unpack_job;
int32_t tedspad_wgrad_unpack_multi(tedspad_wgrad_unpack_job *jobs, int32_t njobs, void *table_dev, int32_t upload, void *stream);

/* Eval-mode BatchNorm folded to y = x*scale + shift (fp64 inside, rounded once): scale = gamma/sqrt(var+eps),
 * shift = beta - mean*scale (+ conv_bias*scale). FrozenBN / .eval() semantics (large_i3d.py:8-38, i3d.py:113-116). */
int32_t tedspad_bn_fold(const float *gamma, const float *beta, const float *mean, const float *var, const float *conv_bias,
                        double eps, int32_t C, float *scale, float *shift, void *stream);

/* ---- the steps either side of the encoder ---------------------------------------- */
/* Antialiased bilinear resize weights of one axis, as torch builds them for F.interpolate(mode='bilinear',
 * antialias=True, align_corners=False) -- the call behind torchvision F.resize(antialias=True) on a float tensor
 * (feature_extraction/dali_extraction.py:49). Host functions: `table` receives out_size entries of
 * (2 + taps) 32-bit words {first input index, tap count, float weights[taps]}; copy it to the device. */
int32_t tedspad_resize_aa_taps(int32_t in_size, int32_t out_size);
int32_t tedspad_resize_aa_table(int32_t in_size, int32_t out_size, int32_t *table);

/* DALIDataloader.val_augmentations (dali_extraction.py:38-50) for one crop box: frames (T,H,W,C) interleaved,
 * uint8 or float (in_is_float) -> value / divisor (255) -> crop [y0,y0+ch) x [x0,x0+cw) -> antialiased bilinear
 * resize to (oh,ow) with the two device tables above (for ch->oh and cw->ow) -> optional horizontal flip (ten-crop)
 * -> fp32 out[t*so_t + c*so_c + y*so_h + x*so_w] (element strides: (T,C,h,w) as the reference returns it, or
 * straight into a (C,T,h,w) clip of the encoder's batch). T * oh < 2^31 (one workgroup per frame and output row). */
int32_t tedspad_frames_crop_resize(const void *frames, int32_t in_is_float, int32_t T, int32_t H, int32_t W, int32_t C,
                                   int32_t y0, int32_t x0, int32_t ch, int32_t cw, int32_t oh, int32_t ow,
                                   const int32_t *ytab, const int32_t *xtab, float divisor, int32_t flip, float *out,
                                   int64_t so_t, int64_t so_c, int64_t so_h, int64_t so_w, void *stream);

/* The same frames -> /divisor -> crop -> antialiased resize (-> flip), written as the INPUT RECORDS of the persistent stem (tedspad_clip_to_tp's layout,
 * X[n][tp][oh][b][ow/2][24] 16-bit) instead of an fp32 clip: the step between the decoder's frames and I3Res50's conv1 (dali_extraction.py:38-50 ->
 * large_i3d.py:229) without the 9.6 MB per clip of fp32 in between. Clip n of n_clips takes source frames first + n*clip_step + f*frame_step,
 * f = 0 .. t_clip-1 (HybridValPipe: sequence_length 16, stride fix_skip = 2, step 32; dali_extraction.py:62-73); frames outside [0, T) are zero frames
 * (pad_sequences). pad_t / stride_t / t_pairs: the stem's temporal geometry as in tedspad_clip_to_tp. Every value is the fp32 value
 * tedspad_frames_crop_resize computes, rounded to `dtype` as tedspad_clip_to_tp rounds it: records bit-identical to crop_resize + clip_to_tp. */
int32_t tedspad_frames_crop_resize_tp(const void *frames, int32_t in_is_float, int32_t T, int32_t H, int32_t W, int32_t C, int32_t n_clips,
                                      int32_t first, int32_t clip_step, int32_t frame_step, int32_t t_clip, int32_t y0, int32_t x0, int32_t ch,
                                      int32_t cw, int32_t oh, int32_t ow, const int32_t *ytab, const int32_t *xtab, float divisor, int32_t flip,
                                      void *records, int32_t pad_t, int32_t stride_t, int32_t t_pairs, int32_t dtype, void *stream);

/* torchvision's ten_crop of size (ch, cw) in place of the single crop box: the records X[10 * n_clips][tp][oh][b][ow/2][24] of all ten crops of every clip,
 * clip time i / crop k at index 10 * i + k, k in torchvision's order (tl, tr, bl, br, centre, then the same five of the horizontally flipped frame). Replaces the
 * ten tedspad_frames_crop_resize_tp calls over the boxes (0,0) (0,W-cw) (H-ch,0) (H-ch,W-cw) (yc,xc) without flip and (0,W-cw) (0,0) (H-ch,W-cw) (H-ch,0)
 * (yc,W-cw-xc) with flip, each writing every tenth clip, bit for bit: per output row the vertical pass runs once per row origin (three, not ten), the horizontal
 * pass once per distinct box, and a flipped crop is the store of its box's values right to left. (yc, xc): the centre crop's origin, torchvision's center_crop
 * rule (half to even). The other arguments as tedspad_frames_crop_resize_tp; (3 * n_clips * oh + 8) * (t_pairs + 1) < 2^31; LDS: 48 * ow + 16 * W * C + 1024
 * bytes of the CU's 160 KB (four full-width row buffers: 101.5 KB for a 1080 x 1920 source at 224 columns). */
int32_t tedspad_frames_ten_crop_tp(const void *frames, int32_t in_is_float, int32_t T, int32_t H, int32_t W, int32_t C, int32_t n_clips,
                                   int32_t first, int32_t clip_step, int32_t frame_step, int32_t t_clip, int32_t ch, int32_t cw, int32_t yc,
                                   int32_t xc, int32_t oh, int32_t ow, const int32_t *ytab, const int32_t *xtab, float divisor, void *records,
                                   int32_t pad_t, int32_t stride_t, int32_t t_pairs, int32_t dtype, void *stream);

/* `shanghai_frames_dataset.augmentation` (feature_extraction/shanghai_dl.py:27-40): uint8 frames (T,H,W,C) -> crop box -> Pillow's
 * two-pass BILINEAR resize with its 8-bit intermediate image (what torchvision's resize does for a PIL image) -> to_tensor (/255)
 * -> fp32 out[t*so_t + c*so_c + y*so_h + x*so_w]. ytab / xtab: device tables of (2 + taps) int32 per output index
 * {first input index, count, coefficients with 22 fractional bits}, built by the host as libImaging/Resample.c does
 * (ted_spad_amd/preprocess.pil_table). Bit-exact with Pillow (tests/test_hip_feed.py). */
int32_t tedspad_frames_crop_resize_pil(const void *frames, int32_t T, int32_t H, int32_t W, int32_t C, int32_t y0, int32_t x0, int32_t ch,
                                       int32_t cw, int32_t oh, int32_t ow, const int32_t *ytab, int32_t ytaps, const int32_t *xtab,
                                       int32_t xtaps, float *out, int64_t so_t, int64_t so_c, int64_t so_h, int64_t so_w, void *stream);

/* Decoded frames -> the ANONYMIZER's input activation (the extraction scripts run fa on every frame: dali_extraction.py:169-173, st_feature_extraction.py:24-26).
 * The clip sampling of tedspad_frames_crop_resize_tp (clip i, frame f = source frame first + i*clip_step + f*frame_step; an index >= T is a zero frame, stored
 * as zeros), each frame / divisor -> crop -> antialiased resize (-> flip) as tedspad_frames_crop_resize, written as output frame i*t_clip + f of the 16-bit
 * channels-last activation tedspad_clip_to_channels_last builds from the fp32 frames: cpad = 4 -> (frames, oh, ow/2, 8) pixel pairs {c0 c1 c2 0 | c0 c1 c2 0}
 * (ow even), cpad = 8 -> (frames, oh, ow, 8), channels >= C zero. `act` 16-byte aligned, n_clips * t_clip * oh < 2^31. Bit-identical to
 * tedspad_frames_crop_resize followed by tedspad_clip_to_channels_last; no fp32 frame is written. */
int32_t tedspad_frames_crop_resize_act(const void *frames, int32_t in_is_float, int32_t T, int32_t H, int32_t W, int32_t C, int32_t n_clips,
                                       int32_t first, int32_t clip_step, int32_t frame_step, int32_t t_clip, int32_t y0, int32_t x0, int32_t ch,
                                       int32_t cw, int32_t oh, int32_t ow, const int32_t *ytab, const int32_t *xtab, float divisor, int32_t flip,
                                       void *act, int32_t cpad, int32_t dtype, void *stream);

/* The same sampling and output with the arithmetic of tedspad_frames_crop_resize_pil (uint8 frames, Pillow's two-pass fixed-point resample, / 255):
 * bit-identical to tedspad_frames_crop_resize_pil followed by tedspad_clip_to_channels_last. */
int32_t tedspad_frames_crop_resize_pil_act(const void *frames, int32_t T, int32_t H, int32_t W, int32_t C, int32_t n_clips, int32_t first,
                                           int32_t clip_step, int32_t frame_step, int32_t t_clip, int32_t y0, int32_t x0, int32_t ch, int32_t cw,
                                           int32_t oh, int32_t ow, const int32_t *ytab, int32_t ytaps, const int32_t *xtab, int32_t xtaps,
                                           void *act, int32_t cpad, int32_t dtype, void *stream);

/* The training loaders' per-frame augmentation (aux_code/ucf101_dl.py: contrastive_train_dataloader.augmentation :596-630 / weak_augmentation :632-642,
 * single_train_dataloader.augmentation :149-183) for a whole batch in ONE launch: uint8 (H,W,3) frame -> resized_crop (Pillow crop, zero-filled right of and
 * below the frame, + two-pass BILINEAR resize, as tedspad_frames_crop_resize_pil) -> contrast / hue / saturation / brightness / contrast / grayscale + gamma
 * (Pillow's 8-bit ImageEnhance / HSV / point arithmetic) -> hflip -> to_tensor (/255) -> two erased boxes -> fp32
 * out[dst + c*so_c + y*so_h + x*so_w]. One record per OUTPUT frame, so frames of different videos (sizes), per-clip and per-frame parameters share the launch.
 * `blob_host`: HOST bytes {nrec records | int32 Pillow tables | 256-byte gamma tables}, copied to `blob_dev` (blob_bytes device bytes, 8-byte aligned) on
 * `stream` before the launch (the one upload); the records' table offsets are int32-word offsets from tables_off, rows of (2 + taps) words
 * {first index, count, 22-bit coefficients} (ted_spad_amd/preprocess.pil_table) for crop height -> oh and crop width -> ow. Every record, every table
 * row it names and the extent of its output frame inside out_elems are checked on the host before anything is launched. One workgroup per record holds
 * the resized frame in LDS: 3*oh*ow bytes must fit (TEDSPAD_EUNSUPPORTED above 224 x 224). Bit-exact with Pillow (tests/test_hip_augment.py). */
enum {
    TEDSPAD_AUG_CONTRAST_FIRST = 1,     /* adjust_contrast before hue (:606) */
    TEDSPAD_AUG_HUE = 2,
    TEDSPAD_AUG_SATURATION = 4,
    TEDSPAD_AUG_BRIGHTNESS = 8,
    TEDSPAD_AUG_CONTRAST_LATE = 16,     /* adjust_contrast after brightness (:614) */
    TEDSPAD_AUG_GRAY = 32,
    TEDSPAD_AUG_GAMMA = 64,             /* only together with TEDSPAD_AUG_GRAY (:616-619) */
    TEDSPAD_AUG_HFLIP = 128,
    TEDSPAD_AUG_REVERSE = 256           /* read the source channels in reverse order (single_train_dataloader :124) */
};
typedef struct tedspad_augment_record {
    const uint8_t *src;                 /* the (H, W, 3) uint8 source frame */
    int64_t dst;                        /* element offset of the output frame in `out` */
    int32_t H, W;
    int32_t top, left, ch, cw;          /* crop box; top + ch > H and left + cw > W are allowed (zero fill), negative origins are not */
    int32_t ytab, xtab, ytaps, xtaps;   /* the two tables: word offsets and taps per row */
    int32_t flags;                      /* TEDSPAD_AUG_* */
    int32_t gamma_lut;                  /* index of the 256-byte table adjust_gamma's point() uses */
    float contrast, saturation, brightness;     /* Image.blend factors */
    int32_t hue_off;                    /* uint8(hue_factor * 255), 0..255: added to H modulo 256 */
    int32_t erase[8];                   /* two boxes {i (row), j (column), h, w}; h <= 0 or w <= 0: none. Clipped at the borders like a slice */
} tedspad_augment_record;
int32_t tedspad_clip_augment(const void *blob_host, void *blob_dev, int64_t blob_bytes, int32_t nrec, int64_t tables_off, int64_t table_words,
                             int64_t luts_off, int32_t nluts, float *out, int64_t out_elems, int32_t oh, int32_t ow, int64_t so_c, int64_t so_h,
                             int64_t so_w, void *stream);

/* The validation loaders' frames (aux_code/ucf101_dl.py: single_val_dataloader.augmentation :297-320, contrastive_val_dataloader.augmentation :873-896) for a
 * whole batch in ONE launch: uint8 (H,W,3) frame -> center_crop (torchvision zero-pads where the crop is larger than the frame, so the box origin may be
 * NEGATIVE and every source coordinate outside [0,H) x [0,W) is zero) -> Pillow's two-pass BILINEAR resize as in tedspad_clip_augment -> hflip -> / 255.
 * The blob is {nrec records | int32 Pillow tables}, laid out, uploaded and checked like tedspad_clip_augment's; a table's windows must not move backwards from
 * one output row to the next. A workgroup owns `band` output rows of three planes: it resamples every temporary row the band's vertical taps reach ONCE into
 * LDS (bytes), then runs the vertical pass out of LDS, so no frame-sized buffer limits oh x ow. The caller picks `band` (1 .. tedspad_val_clips_band_max());
 * over the worst record and band the temporary rows (3 planes x ow bytes each), plus in the activation form the band's 16-bit output rows, must fit
 * tedspad_val_clips_lds_bytes(): otherwise TEDSPAD_EUNSUPPORTED and nothing is launched (ted_spad_amd/val_clips.band_height picks the largest that fits).
 *   tedspad_val_clips      fp32 out[dst + c*so_c + y*so_h + x*so_w], the three planes of a workgroup are the colours of one record.
 *   tedspad_val_clips_act  the anonymizer's input for the pseudo-images the training / validation loops feed it: the nrec = B*n records are n per
 *                          batch item; with p = c*n + k (colour c of record k of item b) image b*n + p/3 of the 16-bit channels-last activation
 *                          (nrec, oh, ow*cpad/8) x 16 bytes holds plane p in channel p%3, the other channels zero (cpad 4: pixel pairs, even ow; cpad 8),
 *                          bit-identical to tedspad_clip_to_channels_last of the permuted fp32 batch. `dst` must be 0.
 * Flags: TEDSPAD_AUG_HFLIP and TEDSPAD_AUG_REVERSE only. Bit-exact with Pillow (tests/test_hip_val_clips.py). */
typedef struct tedspad_val_record {
    const uint8_t *src;                 /* the (H, W, 3) uint8 source frame */
    int64_t dst;                        /* fp32 form: element offset of the output frame in `out` */
    int32_t H, W;
    int32_t top, left, ch, cw;          /* crop box in frame coordinates; it may leave the frame on every side (zero fill) but must intersect it */
    int32_t ytab, xtab, ytaps, xtaps;   /* the two tables (crop height -> oh, crop width -> ow): word offsets and taps per row */
    int32_t flags;                      /* TEDSPAD_AUG_HFLIP | TEDSPAD_AUG_REVERSE */
    int32_t reserved;                   /* 0 */
} tedspad_val_record;
int32_t tedspad_val_clips_lds_bytes(void);
int32_t tedspad_val_clips_band_max(void);
int32_t tedspad_val_clips(const void *blob_host, void *blob_dev, int64_t blob_bytes, int32_t nrec, int64_t tables_off, int64_t table_words, float *out,
                          int64_t out_elems, int32_t oh, int32_t ow, int32_t band, int64_t so_c, int64_t so_h, int64_t so_w, void *stream);
int32_t tedspad_val_clips_act(const void *blob_host, void *blob_dev, int64_t blob_bytes, int32_t nrec, int64_t tables_off, int64_t table_words, void *act,
                              int64_t act_bytes, int32_t n, int32_t oh, int32_t ow, int32_t band, int32_t cpad, int32_t dtype, void *stream);

/* The VISPR loaders' per-image augmentation (aux_code/vispr_dl.py: vispr_dataset.augmentation :71-129, vispr_ssl_dataset.augmentation :186-251) for a whole
 * ragged batch in ONE launch: contiguous uint8 (3,H,W) image (torchvision.io.read_image's layout) -> resized_crop (crop, zero-filled right of and below the
 * image, + ATen's antialiased bilinear resize on fp32: width pass, height pass, one rounding half to even) -> contrast / hue / saturation / brightness /
 * contrast / grayscale + gamma (torchvision's TENSOR path: fp32 _blend and RGB->HSV->RGB truncated to a byte after every op) -> hflip -> one erased box ->
 * / 255 -> fp32 out[dst + c*so_c + y*so_h + x*so_w]. One record per OUTPUT image; two records may name the same source (the two SSL views). The blob is laid
 * out as in tedspad_clip_augment, with tedspad_image_record records, tables of (2 + taps) words {first index, count, fp32 weights}
 * (tedspad_resize_aa_table) and 256-byte gamma tables the caller builds. `scratch` holds the fp32 width-pass intermediate: record i owns the
 * 3 * min(ch, H - top) * ow floats at `tmp`, slices must not overlap. Everything is checked on the host before the launch. Limits: 3*oh*ow bytes must fit the
 * LDS (224 x 224), sources up to 16384 x 16384, crop boxes up to 4096 x 4096; beyond them TEDSPAD_EUNSUPPORTED, nothing is clamped. The resize equals torch's
 * bit for bit at dyadic scales and elsewhere except where torch's own fp32 value lies at a rounding tie; the colour chain is bit-exact
 * (tests/test_hip_vispr_augment.py). Flags: TEDSPAD_AUG_* above, without TEDSPAD_AUG_REVERSE. */
typedef struct tedspad_image_record {
    const uint8_t *src;                 /* the (3, H, W) uint8 source image */
    int64_t dst;                        /* element offset of the output image in `out` */
    int64_t tmp;                        /* element offset of this record's width-pass intermediate in `scratch` */
    int32_t H, W;
    int32_t top, left, ch, cw;          /* crop box; top + ch > H and left + cw > W are allowed (zero fill), negative origins are not */
    int32_t ytab, xtab, ytaps, xtaps;   /* the two tables: word offsets and taps per row */
    int32_t flags;                      /* TEDSPAD_AUG_* */
    int32_t gamma_lut;                  /* index of the 256-byte table of adjust_gamma */
    float contrast, contrast_1m;        /* _blend's ratio and (1.0 - ratio), the latter formed in double and then rounded, as Python does */
    float saturation, saturation_1m;
    float brightness, brightness_1m;
    float hue;                          /* hue_factor in [-0.5, 0.5] */
    int32_t erase[4];                   /* one box {i (row), j (column), h, w}; h <= 0 or w <= 0: none. Clipped at the borders like a slice */
    int32_t reserved;
} tedspad_image_record;
int32_t tedspad_image_augment(const void *blob_host, void *blob_dev, int64_t blob_bytes, int32_t nrec, int64_t tables_off, int64_t table_words,
                              int64_t luts_off, int32_t nluts, float *scratch, int64_t scratch_elems, float *out, int64_t out_elems, int32_t oh,
                              int32_t ow, int64_t so_c, int64_t so_h, int64_t so_w, void *stream);

/* MGFN feature feed(anomaly_detection_mgfn/datasets/dataset.py:65-100): feat (T, ncrops, F) fp32.
 * length > 0 (train): out (ncrops, length, F+1) = process_feat (utils/utils.py:34-42: means over the
 * numpy.linspace(0,T,length+1,dtype=int) segments, a single row where a segment is empty) + L2 magnitude channel.
 * length == 0 (test_mode): out (T, ncrops, F+1) = the rows + magnitude channel. */
int32_t tedspad_segment_pool_mag(const float *feat, int32_t T, int32_t ncrops, int32_t F, int32_t length, float *out,
                                 void *stream);

/* f16 head-room made observable (large_i3d.py:78-79 runs in fp32 / autocast fp16, where an overflow is an inf; the inference stores here SATURATE at
 * +-65504 instead, silently): counts, in a channels-last 16-bit tensor of `rows` pixels x `c` channels (pixel stride ldx), the elements AT the largest finite
 * value of the type (f16: what a clamped store writes; bf16: never) into out2[0] and the non-finite ones into out2[1] (both ADDED to). */
int32_t tedspad_count_saturated(const void *x, int64_t rows, int32_t c, int32_t ldx, int32_t dtype, uint32_t *out2, void *stream);

/* ---- MGFN inference (anomaly_detection_mgfn/models/mgfn.py, utils/utils.py:101-180, model.eval()), all fp32 (csrc/mgfn.hip) ----
 * Token-major (token, channel) rows over a ragged batch of crop sequences. bounds: int32 (M, 2) = first / one-past-last token of each
 * token's sequence; seq_off: int32 (nseq + 1) sequence starts. Deterministic, and every result of a sequence depends on that sequence
 * alone (bit-identical in any batch). */
/* stats (M, 2) = per-token mean and 1 / (std + eps) (torch_ln == 0: MGFN LayerNorm) or 1 / sqrt(var + eps) (torch_ln != 0: nn.LayerNorm),
 * biased variance over C channels. C, ldx % 4 == 0. */
int32_t tedspad_mgfn_ln_stats(const float *x, int32_t ldx, int32_t M, int32_t C, float eps, int32_t torch_ln, float *stats, void *stream);
/* y[m, n] = sum_{t, c} A[m, t, c] w[n, t * cin + c] + bias[n] (NULL: 0), then exact GELU (gelu != 0), then + res[m, n] (NULL: none).
 * A[m, t, c] = x[m + t - taps / 2, c], zero outside m's sequence (a Conv1d(k = taps, padding = taps / 2) over time); with stats
 * (taps == 1 only): (x[m, c] - mean[m]) * rs[m]. f32-input MFMA. N % 64 == 0, cin % 16 == 0, x / w 16-byte aligned, y != x. */
int32_t tedspad_mgfn_gemm(const float *x, int32_t ldx, const int32_t *bounds, int32_t taps, int32_t cin, const float *stats, const float *w,
                          const float *bias, int32_t gelu, const float *res, int32_t ldres, float *y, int32_t ldy, int32_t M, int32_t N,
                          void *stream);
/* GLANCE attention: qkv rows = q | k | v, each heads x 64 channels (head-blocked, 'b (h d) n'); out[m, h * 64 + d] =
 * softmax_j((q_m / 8) . k_j) v_j over m's sequence. tmax >= the longest sequence; heads and (tmax + 31) / 32 at most 65535 (as
 * tedspad_mgfn_attention_bwd). */
int32_t tedspad_mgfn_attention(const float *qkv, int32_t ldqkv, const int32_t *seq_off, int32_t nseq, int32_t tmax, int32_t heads, float *out,
                               int32_t ldo, void *stream);
/* FOCUS rel_pos: out[m, c] = b[c % heads] + sum_t w[c % heads, t] v[m + t - 2, c] (5 taps, zero outside the sequence; head-interleaved
 * channels). C, ldv, ldo % 4 == 0, ldv, ldo >= C, out != v. */
int32_t tedspad_mgfn_relpos(const float *v, int32_t ldv, const int32_t *bounds, int32_t M, int32_t C, int32_t heads, const float *w,
                            const float *b, float *out, int32_t ldo, void *stream);
/* h = nn.LayerNorm(C)(x) (written when h != NULL, (M, C)), logit = h . fc_w + fc_b, score = sigmoid(logit), mag = ||h||_2, each (M).
 * C, ldx % 4 == 0, ldx >= C. */
int32_t tedspad_mgfn_head(const float *x, int32_t ldx, int32_t M, int32_t C, const float *ln_w, const float *ln_b, const float *fc_w, float fc_b,
                          float eps, float *h, float *logit, float *score, float *mag, void *stream);
/* Crop means: video v owns segments seg_off[v] .. seg_off[v+1] (T_v of them) and tokens ncrops * seg_off[v] + c * T_v + t;
 * a_out[seg_off[v] + t] = mean_c a[...] (and the same for b when b != NULL). tmax >= max T_v. */
int32_t tedspad_mgfn_crop_mean(const float *a, float *a_out, const float *b, float *b_out, const int32_t *seg_off, int32_t nvid, int32_t tmax,
                               int32_t ncrops, void *stream);

/* ---- MGFN training (anomaly_detection_mgfn/train.py:79-106, models/mgfn.py:18-86 under model.train()), all fp32 (csrc/mgfn_train.hip) ----
 * Same layout as the inference entries. No float atomics: every reduction over tokens sums fixed chunks of 128 tokens in order into a
 * workspace and then the chunks in order, so two runs give the same bits. Data gradients are tedspad_mgfn_gemm products on transposed,
 * flipped-tap weights; weight gradients are tedspad_mgfn_transpose + tedspad_mgfn_wgrad. */
/* floats of workspace `ws` that any entry below needs for M tokens and C channels */
int64_t tedspad_mgfn_train_ws_floats(int32_t M, int32_t C);
/* Ordered column reductions over the tokens, out = scale * sum_m (...):
 * mode 0: out0[c] = sum a[m, c];
 * mode 1: out0 = sum a, out1 = sum a * xh, xh = (x[m, c] - st[2m]) * st[2m + 1] (row statistics of tedspad_mgfn_ln_stats: LayerNorm db, dg);
 * mode 2: the same with column statistics xh = (x[m, c] - st[c]) * st[C + c] (BatchNorm dbeta, dgamma);
 * mode 3: out0 = sum (a[m, c] - st[c])^2 (st NULL: mode 0); mode 4: out0 = sum st[m] * a[m, c], out1[c] = sum st[m] (fc dweight, dbias). */
int32_t tedspad_mgfn_col_reduce(const float *a, int32_t lda, const float *x, int32_t ldx, const float *st, int32_t mode, int32_t M, int32_t C,
                                float scale, float *ws, float *out0, float *out1, void *stream);
/* y[m, c] = (x[m, c] - stats[2m]) * stats[2m + 1] * g[c] + b[c]: either LayerNorm, materialised (stats of tedspad_mgfn_ln_stats). */
int32_t tedspad_mgfn_ln_apply(const float *x, int32_t ldx, const float *stats, const float *g, const float *b, int32_t M, int32_t C, float *y,
                              int32_t ldy, void *stream);
/* dx of tedspad_mgfn_ln_apply for dy = d/dy (torch_ln == 0: MGFN's (x - mean) / (std + eps), eps as given to ln_stats; else nn.LayerNorm),
 * plus add[m, c] when add != NULL (the residual branch's gradient). dg / db: tedspad_mgfn_col_reduce mode 1. */
int32_t tedspad_mgfn_ln_bwd(const float *dy, int32_t lddy, const float *x, int32_t ldx, const float *stats, const float *g, int32_t torch_ln,
                            float eps, const float *add, int32_t ldadd, float *dx, int32_t lddx, int32_t M, int32_t C, void *stream);
/* nn.BatchNorm1d in train mode over all M tokens: stat (2C) = batch mean | 1 / sqrt(biased var + eps); y = (x - mean) invstd gamma + beta;
 * running_mean / running_var (NULL: none) updated with `momentum`, running_var from the unbiased variance. */
int32_t tedspad_mgfn_bn_train_fwd(const float *x, int32_t ldx, int32_t M, int32_t C, const float *gamma, const float *beta, float eps,
                                  float momentum, float *ws, float *stat, float *running_mean, float *running_var, float *y, int32_t ldy,
                                  void *stream);
/* its backward: dgamma, dbeta (C) and dx = gamma invstd (dy - dbeta / M - xh dgamma / M) + add (NULL: none). */
int32_t tedspad_mgfn_bn_train_bwd(const float *dy, int32_t lddy, const float *x, int32_t ldx, const float *stat, const float *gamma, int32_t M,
                                  int32_t C, float *ws, float *dgamma, float *dbeta, const float *add, int32_t ldadd, float *dx, int32_t lddx,
                                  void *stream);
/* Exact-erf GELU over n contiguous floats (n % 4 == 0) and its backward on the kept pre-activation x. */
int32_t tedspad_mgfn_gelu(const float *x, float *y, int64_t n, void *stream);
int32_t tedspad_mgfn_gelu_bwd(const float *x, const float *dy, float *dx, int64_t n, void *stream);
/* out[(t * C + c) * ldo + m] = x[m + t - taps / 2, c], zero outside m's sequence and for M <= m < ldo: the transposed k-tap window matrix.
 * With ldo % 16 == 0 this image and the transposed dy (N, ldo) are the operands of tedspad_mgfn_wgrad. */
int32_t tedspad_mgfn_transpose(const float *x, int32_t ldx, const int32_t *bounds, int32_t taps, int32_t M, int32_t C, float *out, int32_t ldo,
                               void *stream);
/* Weight gradient dwt (rows, N) = at (rows, ldk) . dyt (N, ldk)^T over the token axis (both from tedspad_mgfn_transpose, ldk % 16 == 0,
 * N % 64 == 0) on the f32 MFMA: the token axis is cut into slices whose number depends on the shapes only, one wave per 64 x 64 tile and
 * slice, the slices' partial results go to ws (tedspad_mgfn_wgrad_ws_floats floats; 0: one slice, ws unused) and are added in order. */
int64_t tedspad_mgfn_wgrad_ws_floats(int32_t ldk, int32_t rows, int32_t N);
int32_t tedspad_mgfn_wgrad(const float *at, const float *dyt, int32_t ldk, int32_t rows, int32_t N, float *ws, float *dwt, void *stream);
/* Backward of tedspad_mgfn_attention: o its output, d_o the gradient of o; dqkv rows = dq | dk | dv. lse (M, heads, 2) is scratch (the rows'
 * log-sum-exp and dO . O). P is recomputed per 32-query / 32-key block. */
int32_t tedspad_mgfn_attention_bwd(const float *qkv, int32_t ldqkv, const float *o, int32_t ldo, const float *d_o, int32_t lddo,
                                   const int32_t *seq_off, int32_t nseq, int32_t tmax, int32_t heads, float *lse, float *dqkv, int32_t lddqkv,
                                   void *stream);
/* Backward of tedspad_mgfn_relpos: dv[m, c] = sum_t w[c % heads, t] dout[m - t + 2, c]; dw (heads, 5), db (heads). */
int32_t tedspad_mgfn_relpos_bwd(const float *dout, int32_t lddo, const float *v, int32_t ldv, const int32_t *bounds, int32_t M, int32_t C,
                                int32_t heads, const float *w, float *ws, float *dv, int32_t lddv, float *dw, float *db, void *stream);
/* fc -> sigmoid backward: dz[m] = dscore[m] score[m] (1 - score[m]); dh[m, :] += dz[m] fc_w (dh (M, C) in place). The to_logits LayerNorm's
 * backward is tedspad_mgfn_ln_bwd / col_reduce on dh; fc's gradients are col_reduce mode 4 on h with st = dz. */
int32_t tedspad_mgfn_head_bwd(const float *score, const float *dscore, const float *fc_w, int32_t M, int32_t C, float *dh, float *dz, void *stream);
/* MSNSD's training branch and the whole cost, forward and gradient. Videos 0 .. n-1 normal, n .. 2n-1 abnormal, each ncrops x T tokens of C
 * channels (h, the to_logits output); crop_scores / crop_mags (2n, T) from tedspad_mgfn_crop_mean; masks (2, n, T) = select_idx (abnormal),
 * select_idx_normal; labels (2n). Out: idx (2n, k) the k largest masked magnitudes, descending, ties to the lowest index; vid_score (2n)
 * the mean crop-mean score of those; l1 / dl1 (2, ncrops n, k): L1 norms of the selected rows (abnormal, normal; row crop n + video) and
 * the cost's gradient on them; losses (8) = cost, smooth, sparse, cls, con, con_n, con_a, total; dcs (2n, T), dvid (2n) gradients on the
 * crop-mean and video scores; dscore (M) and dh (M, C) the gradients on the per-token score and on h (zero off the selected rows). */
int32_t tedspad_mgfn_msnsd(const float *h, const float *crop_scores, const float *crop_mags, const float *masks, const float *labels, int32_t n,
                           int32_t ncrops, int32_t T, int32_t C, int32_t k, int32_t *idx, float *vid_score, float *l1, float *losses, float *dl1,
                           float *dcs, float *dvid, float *dscore, float *dh, void *stream);

/* ---- validation of the action classifier, pictures of the anonymizer (csrc/action_eval.hip) -- all fp32, deterministic, no float atomics ---- */

/* One validation batch behind the ft forward -- train_anonymizer.py:259,272,282-283 / train_anonymized_action.py:156,169,179-180:
 * probs (B, C) = nn.functional.softmax(logits, dim=1) (max-subtracted), row_loss (B) = cross entropy per row, loss fp32[1] = their mean
 * (nn.CrossEntropyLoss(), reduced in a fixed order), pred int32 (B) = np.flip(np.argsort(probs, axis=1), axis=1)[:, 0] with ties resolved
 * as kind='stable' does: among exactly equal maxima the HIGHEST index (the reference's default sort kind leaves ties unspecified).
 * labels: int64 (B) on the device; labels_host: the same values in host memory, range-checked before the launch, or NULL when the
 * labels exist on the device only (a label outside [0, C) then gives a NaN row loss and reads nothing). One launch.
 * 1 <= B <= 1024, 2 <= C <= 1024; anything else is TEDSPAD_EINVAL and nothing is launched. */
int32_t tedspad_softmax_ce_eval(const float *logits, const int64_t *labels, const int64_t *labels_host, float *probs, float *row_loss,
                                float *loss, int32_t *pred, int32_t B, int32_t C, void *stream);

/* pred_dict[name].append(predictions[entry]) -- train_anonymizer.py:285-290 / train_anonymized_action.py:182-189, kept as running sums:
 * sums[vid[b], :] += probs[b, :] and counts[vid[b]] += 1 for b = 0 .. B-1 IN ROW ORDER (two rows of a batch may name one video; the result
 * does not depend on scheduling). sums fp32 (V, C), counts int32 (V). vid: int32 (B) on the device; vid_host: the same values in host
 * memory -- an index outside [0, V) is TEDSPAD_EINVAL before anything is launched. One launch. */
int32_t tedspad_vote_accumulate(const float *probs, const int32_t *vid, const int32_t *vid_host, float *sums, int32_t *counts, int32_t B,
                                int32_t C, int32_t V, void *stream);

/* predictions[entry] = np.mean(pred_dict[key], axis=0); c_pred = np.flip(np.argsort(predictions, axis=1), axis=1)[:, 0];
 * c_pred == ground_truth -- train_anonymizer.py:475-487,491-504 / train_anonymized_action.py:352-364,368-381.
 * mean (V, C) = sums / counts (IEEE division), pred_v int32 (V) with the tie rule above, correct uint8 (V) = (pred_v == labels_v), labels_v
 * int64 (V). A video with counts == 0 was never seen: mean row 0, pred_v = -1, correct = 0. */
int32_t tedspad_vote_finalize(const float *sums, const int32_t *counts, const int64_t *labels_v, float *mean, int32_t *pred_v,
                              uint8_t *correct, int32_t V, int32_t C, void *stream);

/* torchvision.utils.save_image(x, padding=pad, nrow=nrow) up to the file -- train_anonymizer.py:313-314. x: NCHW fp32 (N, 3, H, W), N >= 2;
 * out: uint8 (Hg, Wg, 3). xmaps = min(nrow, N), ymaps = ceil(N / xmaps), Hg = ymaps (H + pad) + pad, Wg = xmaps (W + pad) + pad; image k
 * starts at row (k / xmaps)(H + pad) + pad, column (k % xmaps)(W + pad) + pad; everything else is 0; each value is
 * uint8(clamp(x * 255 + 0.5, 0, 255)), the multiply and the add rounded separately (torch's mul(255).add_(0.5)).
 * tedspad_image_grid_dims (HOST side, pure CPU) gives Hg and Wg and makes the same argument checks. */
int32_t tedspad_image_grid_dims(int32_t N, int32_t H, int32_t W, int32_t nrow, int32_t pad, int32_t *hg, int32_t *wg);
int32_t tedspad_image_grid_u8(const float *x, uint8_t *out, int32_t N, int32_t H, int32_t W, int32_t nrow, int32_t pad, void *stream);

/* save_video -- visualization/visualize_anonymization.py:52-59, after the colour flip of :108.
 * tedspad_minmax_f32: out2 = {min, max} of n fp32 values (ws: fp32[tedspad_minmax_ws_floats()] workspace; two launches).
 * tedspad_video_frames_u8: x (T, 3, H, W) fp32, minmax fp32[2] on the device -> out uint8 (T, H, W, 3) with the channel order reversed,
 * uint8(trunc(((x - min) / (max - min)) * 255)): IEEE subtract, divide, multiply in that order, as numpy's fp32 does. max == min is 0 / 0 in
 * the reference (undefined); here it writes zeros. */
int32_t tedspad_minmax_ws_floats(void);
int32_t tedspad_minmax_f32(const float *x, int64_t n, float *ws, float *out2, void *stream);
int32_t tedspad_video_frames_u8(const float *x, const float *minmax, uint8_t *out, int32_t T, int32_t H, int32_t W, void *stream);

/* ---- nn.L1Loss() and its gradient: fa_pretraining/train_reconstruction.py:46-47,77 (`criterion(output, inputs)`, `loss.backward()`) ----
 * Both forms: *loss = mean |y - x| (0-d fp32), every reduction in a fixed order without atomics (bit-identical from run to run); two launches (the terms and
 * per-workgroup partials, then the mean). ws: fp32[tedspad_l1_ws_floats()] workspace. The gradient magnitude is g = grad_scale / (float)numel, one fp32
 * division on the host; an element's gradient is +g, -g, exactly 0 where y == x (torch.sign) and NaN where the difference is NaN.
 * A lane of the first launch adds ceil(items / (blocks * tedspad_l1_block_threads())) items in sequence, blocks = min(ceil(items / threads),
 * tedspad_l1_max_blocks()); everything after that is a binary tree (items: pixel records of 3 terms each in the train form, elements in the flat form).
 *
 * tedspad_l1_loss_grad_cl (train form): y = the head's 16-bit channels-last output, n * hw pixel records of 8 channels `ld` elements apart (ld >= 8), channels
 * 0-2 valid; x = the fp32 (n,3,hw) target. dl = the 16-bit (n,hw,8) gradient records ConvLayer.wgrad / dgrad read: channels 0-2 = sign(float(y) - x) * g with g
 * rounded once to the storage type (round to nearest even), channels 3-7 = 0, one 16-byte store each (dl 16-byte aligned). y32 (may be NULL): the fp32 (n,3,hw)
 * copy of y. numel = n * 3 * hw.
 * tedspad_l1_loss_flat: y, x contiguous fp32 of numel elements in any (common) layout; dy (may be NULL) = sign(y - x) * g in fp32. (c, hw) only choose the ORDER of
 * the sum: c = 1, hw = numel adds in index order; for (n,c,hw) arrays, c and hw make an item of the c values of one pixel -- with c = 3 the partition and order
 * of the train form, whose loss this then equals bit for bit on the same values. numel must be a multiple of c * hw. */
int32_t tedspad_l1_block_threads(void);
int32_t tedspad_l1_max_blocks(void);
int32_t tedspad_l1_ws_floats(void);
int32_t tedspad_l1_loss_grad_cl(const void *y, int32_t ld, const float *x, void *dl, float *y32, float *ws, float *loss, int32_t n, int64_t hw,
                                float grad_scale, int32_t dtype, void *stream);
int32_t tedspad_l1_loss_flat(const float *y, const float *x, float *dy, float *ws, float *loss, int64_t numel, int32_t c, int64_t hw, float grad_scale,
                             void *stream);

/* ---- the optimizer tail of a training step: GradScaler's non-finite check and unscale, torch.optim.Adam / AdamW / SGD, GradScaler.update ----
 * (action_training/train_action.py:79-81 `scaler.scale(loss).backward(); scaler.step(optimizer); scaler.update()`, :251-259 the optimizer choice.)
 * A whole network is updated by at most three launches whose count and host work do not depend on the number of tensors:
 *   tedspad_optim_check   reads every gradient of the table once, writes nothing to them, stores 1 to state[0] if any value is not finite (racing writers store
 *                         the same constant: no atomics). Left out when the step runs without a loss scale.
 *   tedspad_optim_update  one launch for adam / adamw / sgd. Does nothing at all when state[0] is set. Multiplies each gradient by 1 / *scale (scale NULL: by 1) and
 *                         applies torch's single-tensor arithmetic in fp32 (no amsgrad, no maximize, dampening 0, no nesterov), t = state[1] + 1:
 *                           adam   g += wd p (wd != 0); m += (1 - b1)(g - m); v = b2 v + (1 - b2) g g; p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 *                           adamw  p -= lr wd p, then adam with wd = 0
 *                           sgd    g += wd p; buf = mu buf + g (buf starts as zeros, so the first applied step leaves buf = g); p -= lr buf; mu = 0 keeps no buffer (m NULL)
 *   tedspad_optim_finish  one tiny launch (a kernel of its own: folded into the update it would need an arrival counter across workgroups), no host synchronisation:
 *                         out[0] = found_inf as 0 / 1, out[1] = the scale the gradients of this step carried (1 without scale_state); state[1] += !found_inf and the
 *                         bias corrections of the next step; GradScaler.update() on scale_state when growth_interval > 0 (found_inf: scale *= backoff, tracker = 0;
 *                         else ++tracker and at growth_interval scale *= growth, tracker = 0), growth_interval <= 0 leaves the scale alone (a static scale); state[0] = 0.
 * table: nchunks records ON THE DEVICE, each one contiguous run of at most tedspad_optim_chunk_elems() elements of ONE tensor; a workgroup reads its record into
 * scalar registers. p, m, v 16-byte aligned take 16-byte accesses; g may sit at any 4-byte phase (16-byte loads where it is 16-byte aligned, dwords where not;
 * the check walks g alone and aligns itself on it: head, 16-byte body, tail). An element's result does not depend on the path that handled it.
 * state: 8 int32 words on the device {found_inf, t (applied steps), fp32 bits of 1 - b1^(t+1), fp32 bits of sqrt(1 - b2^(t+1)), double b1^(t+1), double b2^(t+1)}
 * (the caller initialises them; adam / adamw only read words 2-3). scale_state: {fp32 scale, int32 growth tracker}. mode: 0 adam, 1 adamw, 2 sgd. */
typedef struct tedspad_optim_chunk {
    float *p;
    const float *g;
    float *m, *v;
    int64_t n, reserved;
} tedspad_optim_chunk;
int32_t tedspad_optim_chunk_elems(void);
int32_t tedspad_optim_check(const tedspad_optim_chunk *table, int32_t nchunks, int32_t *state, void *stream);
int32_t tedspad_optim_update(const tedspad_optim_chunk *table, int32_t nchunks, int32_t mode, const int32_t *state, const float *scale, float lr, double beta1,
                             double beta2, float eps, float weight_decay, float momentum, void *stream);
int32_t tedspad_optim_finish(int32_t *state, float *scale_state, double beta1, double beta2, float growth, float backoff, int32_t growth_interval, float *out,
                             void *stream);

/* ---- the attention core of I3Res50's NonLocalBlock, inference (csrc/nonlocal.hip) ----
 * Replaces large_i3d.py:112-119 (`view` x 3, `bmm(theta^T, phi)`, `* dim_inner**-.5`, `softmax(dim=-1)`, `bmm(g, p^T)`, `view`) with one launch
 * that never writes the q x k score matrix. Channels-last 16-bit rows: theta (n, q, d) with row stride ld_theta, phi and g (n, k, d) with their
 * own row strides (two channel slices of one wider buffer: pass each slice's first channel and the buffer's row stride), out (n, q, d):
 *   out[b, i, :] = sum_j softmax_j(scale * theta[b, i, :] . phi[b, j, :]) * g[b, j, :]
 * fp32 logits and accumulation, the running maximum subtracted (online softmax over key tiles); the probabilities are rounded to the storage type
 * for the second product, the row sum is taken of the unrounded ones. q, k >= 1 are arbitrary; every result depends on its own batch item alone
 * (bit-identical in any batch). d must be 256 or 512 (anything else: TEDSPAD_EINVAL); ld % 8 == 0, 16-byte aligned pointers, out aliases no input. */
int32_t tedspad_nl_attention_fwd(const void *theta, int32_t ld_theta, const void *phi, int32_t ld_phi, const void *g, int32_t ld_g, void *out, int32_t ld_out,
                                 int32_t n, int32_t q, int32_t k, int32_t d, float scale, int32_t dtype, void *stream);

/* ---- the same with a tape, and its backward (csrc/nonlocal.hip) ----
 * tedspad_nl_attention_fwd_lse is tedspad_nl_attention_fwd (the same kernel, `out` bit-identical) with one more output: lse (n, q) fp32,
 *   lse[b, i] = ln sum_j exp(scale * theta[b, i, :] . phi[b, j, :])        (the running maximum included)
 * tedspad_nl_attention_bwd takes theta, phi, g, the forward's out `t`, the upstream gradient `dt` (n, q, d) and lse, and writes
 *   P = exp(scale theta phi^T - lse)     recomputed, never written
 *   dg = P^T dt        D_i = sum_c dt[i, c] t[i, c]        dS = P o (dt g^T - D)        dtheta = scale dS phi        dphi = scale dS^T theta
 * as 16-bit rows with their own strides (dphi | dg may be the two channel halves of one buffer, as phi | g may be). P and dS are rounded to the storage
 * type for the second products, every sum is fp32, every output is rounded once. All of these conversions are the training path's: none clamps, so a
 * dS or a result past the f16 range, and a non-finite dt or lse, reach the gradients as inf / NaN (for a loss scale's non-finite check to find).
 * f16 and small values: gfx950's matrix cores flush f16 SUBNORMAL operands, so a P below 2^-14 = 6.1e-5 (a key more than 9.7 below the row's
 * log-sum-exp; with 392 equally weighted keys every P is 2.6e-3) and a dS below it contribute nothing to dg / dtheta / dphi: the error of a term is
 * u * P only above that floor. Pass dt SCALED (the autograd bridge multiplies by 256, a loss scale does the same) so that dS stays normal; bf16 has
 * fp32's range and no such floor. Three launches (D, one workgroup per 32 keys for
 * dphi and dg, one per 32 queries for dtheta), no atomics: every result depends on its own batch item alone and is bit-identical from run to run and in
 * any batch. `workspace` holds D: tedspad_nl_attention_bwd_workspace (HOST side, pure CPU) gives its size in bytes. Shapes, alignment and the error for
 * d other than 256 / 512 as in the forward; no output aliases another argument. */
int32_t tedspad_nl_attention_fwd_lse(const void *theta, int32_t ld_theta, const void *phi, int32_t ld_phi, const void *g, int32_t ld_g, void *out,
                                     int32_t ld_out, float *lse, int32_t n, int32_t q, int32_t k, int32_t d, float scale, int32_t dtype, void *stream);
int32_t tedspad_nl_attention_bwd_workspace(int32_t n, int32_t q, int64_t *bytes);
int32_t tedspad_nl_attention_bwd(const void *theta, int32_t ld_theta, const void *phi, int32_t ld_phi, const void *g, int32_t ld_g, const void *t, int32_t ld_t,
                                 const void *dt, int32_t ld_dt, const float *lse, void *dtheta, int32_t ld_dtheta, void *dphi, int32_t ld_dphi, void *dg,
                                 int32_t ld_dg, void *workspace, int32_t n, int32_t q, int32_t k, int32_t d, float scale, int32_t dtype, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TEDSPAD_HIP_H */
