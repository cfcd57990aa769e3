// Validation of the action classifier and the pictures of the anonymizer for gfx950: what the reference's scripts do BETWEEN epochs
// (anonymization_training/train_anonymizer.py:216-315,459-509, action_training/train_anonymized_action.py:115-200,335-386,
// visualization/visualize_anonymization.py:52-62,104-111). All fp32, deterministic (no float atomics, every reduction in a fixed order).
//
//  * softmax_ce_eval : softmax(dim=1), per-row cross entropy, its mean and the top-1 class of a (B, C) logit matrix in ONE launch:
//                      a single workgroup, one wave per row (round-robin), then wave 0 reduces the row losses in a fixed order.
//  * vote_accumulate : adds each clip's probability row into its video's sum, in row order (one thread per class walks the rows).
//  * vote_finalize   : per-video mean probabilities, top-1 class and correctness (one wave per video).
//  * image_grid_u8   : torchvision.utils.save_image's grid (make_grid + mul(255).add_(0.5).clamp_(0, 255) -> uint8 HWC).
//  * minmax_f32 / video_frames_u8 : save_video's whole-video min-max normalisation, channel flip and uint8 HWC frames.
#include "common.h"

namespace tedspad {
namespace {

__device__ __forceinline__ float wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wmax(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = __builtin_fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wmin(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = __builtin_fminf(v, __shfl_xor(v, o, 64));
    return v;
}

// Top-1 of a row held as per-lane (value, index) candidates. Among exactly equal maxima the HIGHEST index wins: what
// np.flip(np.argsort(p, kind='stable'), axis=1)[:, 0] gives (the reference's default sort kind leaves ties unspecified).
__device__ __forceinline__ int wargmax_last(float v, int idx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (ov > v || (ov == v && oi > idx)) { v = ov; idx = oi; }
    }
    return idx;
}
// one wave: the top-1 class of row[0..C) under the rule above (lane-strided scan, later index replaces an equal value)
__device__ __forceinline__ int row_argmax_last(const float *row, int C, int lane) {
    float best = -INFINITY;
    int bi = -1;
    for (int c = lane; c < C; c += 64) {
        const float v = row[c];
        if (v >= best) { best = v; bi = c; }
    }
    return wargmax_last(best, bi);
}

constexpr int SCE_MAX_B = 1024, SCE_MAX_C = 1024, SCE_THREADS = 1024;

// single workgroup of 16 waves; wave w owns rows w, w + 16, ...
__global__ __launch_bounds__(SCE_THREADS) void softmax_ce_eval_kernel(const float *logits, const long *labels, float *probs, float *row_loss,
                                                                       float *loss, int *pred, int B, int C) {
    __shared__ float rl[SCE_MAX_B];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int row = wave; row < B; row += SCE_THREADS / 64) {
        const float *z = logits + (size_t)row * C;
        float mx = -INFINITY;
        for (int c = lane; c < C; c += 64) mx = __builtin_fmaxf(mx, z[c]);
        mx = wmax(mx);                                           // max-subtracted: |logit| ~ 80 neither overflows nor turns into NaN
        const int top = row_argmax_last(z, C, lane);             // softmax is monotonic: the top logit is the top probability
        float rest = 0.f;                                        // the denominator WITHOUT the top class's exp(0) = 1: a confident row keeps its small terms
        for (int c = lane; c < C; c += 64) rest += c == top ? 0.f : expf(z[c] - mx);
        rest = wsum(rest);
        const float den = 1.f + rest;
        for (int c = lane; c < C; c += 64) probs[(size_t)row * C + c] = __fdiv_rn(expf(z[c] - mx), den);   // nn.functional.softmax(output, dim=1) (:272)
        const long lab = labels[row];
        // -log_softmax[label] = log1p(rest) + (max - z[label]): 0 + log1p(rest) where the label is the top class. A label outside [0, C)
        // (the host checks its copy before the launch; a device-only label cannot be) reads nothing and gives NaN.
        const float l = (lab >= 0 && lab < C) ? log1pf(rest) + (mx - z[lab]) : __builtin_nanf("");
        if (lane == 0) {
            row_loss[row] = l;
            rl[row] = l;
            pred[row] = top;
        }
    }
    __syncthreads();
    if (wave == 0) {                                             // nn.CrossEntropyLoss(): mean over B, lane-strided then the butterfly -- a fixed order
        float s = 0.f;
        for (int i = lane; i < B; i += 64) s += rl[i];
        s = wsum(s);
        if (lane == 0) loss[0] = s / (float)B;
    }
}

// thread c walks the B rows in order: sums[vid[b], c] += probs[b, c]; the thread of class 0 also counts the rows. Two rows of one batch that
// name the same video are added one after the other by the same thread, so the result does not depend on scheduling.
__global__ __launch_bounds__(256) void vote_accumulate_kernel(const float *probs, const int *vid, float *sums, int *counts, int B, int C, int V) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    int cur = -1, n = 0;                                         // a run of rows of one video stays in registers: the same additions in the same order
    float acc = 0.f;
    for (int b = 0; b < B; ++b) {
        const int v = vid[b];
        if (v < 0 || v >= V) continue;                           // (checked on the host before the launch; never written out of bounds)
        if (v != cur) {
            if (cur >= 0) {
                sums[(size_t)cur * C + c] = acc;
                if (c == 0) counts[cur] += n;
            }
            cur = v; n = 0;
            acc = sums[(size_t)v * C + c];
        }
        acc = __fadd_rn(acc, probs[(size_t)b * C + c]);
        ++n;
    }
    if (cur >= 0) {
        sums[(size_t)cur * C + c] = acc;
        if (c == 0) counts[cur] += n;
    }
}

// one wave per video: mean = sums / counts (np.mean(pred_dict[key], axis=0)), top-1 of the mean, correct = (top-1 == label)
__global__ __launch_bounds__(256) void vote_finalize_kernel(const float *sums, const int *counts, const long *labels, float *mean, int *pred,
                                                             uint8_t *correct, int V, int C) {
    const int v = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (v >= V) return;
    const int n = counts[v];
    float *m = mean + (size_t)v * C;
    if (n <= 0) {                                                // a video no clip named: not seen
        for (int c = lane; c < C; c += 64) m[c] = 0.f;
        if (lane == 0) { pred[v] = -1; correct[v] = 0; }
        return;
    }
    const float fn = (float)n;
    float best = -INFINITY;
    int bi = -1;
    for (int c = lane; c < C; c += 64) {
        const float q = __fdiv_rn(sums[(size_t)v * C + c], fn);
        m[c] = q;
        if (q >= best) { best = q; bi = c; }
    }
    const int top = wargmax_last(best, bi);
    if (lane == 0) {
        pred[v] = top;
        correct[v] = (long)top == labels[v] ? 1 : 0;
    }
}

// one thread per grid pixel (3 channels)
__global__ __launch_bounds__(256) void image_grid_kernel(const float *x, uint8_t *out, int N, int H, int W, int xmaps, int pad, int Hg, int Wg) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= Hg * Wg) return;
    const int gy = p / Wg, gx = p % Wg;
    const int cy = gy / (H + pad), cx = gx / (W + pad);          // cell; its image starts `pad` below / right of the cell's corner
    const int iy = gy - cy * (H + pad) - pad, ix = gx - cx * (W + pad) - pad;
    const int k = cy * xmaps + cx;
    const bool in = iy >= 0 && ix >= 0 && iy < H && ix < W && cx < xmaps && k < N;     // (the last row / column of padding falls in cell ymaps / xmaps)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        uint8_t q = 0;
        if (in) {
            const float v = x[(((size_t)k * 3 + c) * H + iy) * W + ix];
            const float s = __fadd_rn(__fmul_rn(v, 255.f), 0.5f);                      // grid.mul(255).add_(0.5): two roundings, no FMA
            q = (uint8_t)__builtin_fminf(__builtin_fmaxf(s, 0.f), 255.f);              // .clamp_(0, 255).to(torch.uint8)  (NaN -> 0)
        }
        out[(size_t)p * 3 + c] = q;
    }
}

constexpr int MM_BLOCKS = 256;

// stage 1: block partials into ws[2 * block]; stage 2 (nblocks == 1 over the partials): out2 = {min, max}
__global__ __launch_bounds__(256) void minmax_kernel(const float *x, long n, float *dst, int pairs_in) {
    __shared__ float smn[4], smx[4];
    float mn = INFINITY, mx = -INFINITY;
    if (pairs_in) {                                              // x = (n, 2) partial {min, max} pairs
        for (long i = threadIdx.x; i < n; i += 256) {
            mn = __builtin_fminf(mn, x[2 * i]);
            mx = __builtin_fmaxf(mx, x[2 * i + 1]);
        }
    } else {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
            const float v = x[i];
            mn = __builtin_fminf(mn, v);
            mx = __builtin_fmaxf(mx, v);
        }
    }
    mn = wmin(mn); mx = wmax(mx);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { smn[wave] = mn; smx[wave] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        dst[2 * blockIdx.x] = __builtin_fminf(__builtin_fminf(smn[0], smn[1]), __builtin_fminf(smn[2], smn[3]));
        dst[2 * blockIdx.x + 1] = __builtin_fmaxf(__builtin_fmaxf(smx[0], smx[1]), __builtin_fmaxf(smx[2], smx[3]));
    }
}

// one thread per output pixel: out[t, y, x, k] = uint8(trunc((v - min) / (max - min) * 255)), v = in[t, 2 - k, y, x] (torch.flip(dims=[1]), :108)
__global__ __launch_bounds__(256) void video_frames_kernel(const float *x, const float *mm, uint8_t *out, long npix, int HW) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const float mn = mm[0], mx = mm[1];
    const float range = __fsub_rn(mx, mn);
    const long t = p / HW, r = p % HW;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        uint8_t q = 0;
        if (mx > mn) {                                           // max == min is 0 / 0 in the reference (undefined): zeros here
            const float v = x[(t * 3 + (2 - k)) * HW + r];
            const float u = __fmul_rn(__fdiv_rn(__fsub_rn(v, mn), range), 255.f);      // IEEE subtract, divide, multiply: numpy's fp32 (:57-59)
            q = (uint8_t)__builtin_fminf(__builtin_fmaxf(u, 0.f), 255.f);              // in [0, 255] by construction; astype(np.uint8) truncates
        }
        out[p * 3 + k] = q;
    }
}

}  // namespace
}  // namespace tedspad

using namespace tedspad;

extern "C" int32_t tedspad_softmax_ce_eval(const float *logits, const int64_t *labels, const int64_t *labels_host, float *probs, float *row_loss,
                                           float *loss, int32_t *pred, int32_t B, int32_t C, void *stream) {
    TS_REQUIRE(logits && labels && probs && row_loss && loss && pred, "tedspad_softmax_ce_eval: null argument");
    TS_REQUIRE(B >= 1 && B <= SCE_MAX_B && C >= 2 && C <= SCE_MAX_C, "tedspad_softmax_ce_eval: supports 1 <= B <= 1024, 2 <= C <= 1024 (got B=%d C=%d)", B, C);
    if (labels_host)
        for (int i = 0; i < B; ++i)
            TS_REQUIRE(labels_host[i] >= 0 && labels_host[i] < C, "tedspad_softmax_ce_eval: label %lld of row %d outside [0, %d)", (long long)labels_host[i], i, C);
    hipLaunchKernelGGL(softmax_ce_eval_kernel, dim3(1), dim3(SCE_THREADS), 0, (hipStream_t)stream, logits, (const long *)labels, probs, row_loss, loss, pred, B, C);
    return check_launch("tedspad_softmax_ce_eval");
}

extern "C" int32_t tedspad_vote_accumulate(const float *probs, const int32_t *vid, const int32_t *vid_host, float *sums, int32_t *counts, int32_t B,
                                           int32_t C, int32_t V, void *stream) {
    TS_REQUIRE(probs && vid && vid_host && sums && counts, "tedspad_vote_accumulate: null argument");
    TS_REQUIRE(B >= 1 && B <= SCE_MAX_B && C >= 2 && C <= SCE_MAX_C && V >= 1, "tedspad_vote_accumulate: supports 1 <= B <= 1024, 2 <= C <= 1024, V >= 1 (got B=%d C=%d V=%d)", B, C, V);
    for (int i = 0; i < B; ++i)
        TS_REQUIRE(vid_host[i] >= 0 && vid_host[i] < V, "tedspad_vote_accumulate: video index %d of row %d outside [0, %d)", vid_host[i], i, V);
    hipLaunchKernelGGL(vote_accumulate_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, probs, vid, sums, counts, B, C, V);
    return check_launch("tedspad_vote_accumulate");
}

extern "C" int32_t tedspad_vote_finalize(const float *sums, const int32_t *counts, const int64_t *labels_v, float *mean, int32_t *pred_v,
                                         uint8_t *correct, int32_t V, int32_t C, void *stream) {
    TS_REQUIRE(sums && counts && labels_v && mean && pred_v && correct, "tedspad_vote_finalize: null argument");
    TS_REQUIRE(V >= 1 && V <= (1 << 24) && C >= 2 && C <= SCE_MAX_C, "tedspad_vote_finalize: supports 1 <= V <= 2^24, 2 <= C <= 1024 (got V=%d C=%d)", V, C);
    hipLaunchKernelGGL(vote_finalize_kernel, dim3((V + 3) / 4), dim3(256), 0, (hipStream_t)stream, sums, counts, (const long *)labels_v, mean, pred_v, correct, V, C);
    return check_launch("tedspad_vote_finalize");
}

extern "C" int32_t tedspad_image_grid_dims(int32_t N, int32_t H, int32_t W, int32_t nrow, int32_t pad, int32_t *hg, int32_t *wg) {
    TS_REQUIRE(hg && wg, "tedspad_image_grid_dims: null argument");
    TS_REQUIRE(N >= 2 && H >= 1 && W >= 1 && nrow >= 1 && pad >= 0, "tedspad_image_grid: needs N >= 2, H, W, nrow >= 1, padding >= 0 (got N=%d H=%d W=%d nrow=%d padding=%d)", N, H, W, nrow, pad);
    const int64_t xmaps = nrow < N ? nrow : N, ymaps = (N + xmaps - 1) / xmaps;
    const int64_t Hg = ymaps * ((int64_t)H + pad) + pad, Wg = xmaps * ((int64_t)W + pad) + pad;
    TS_REQUIRE(Hg * Wg * 3 < ((int64_t)1 << 31) && (int64_t)N * 3 * H * W < ((int64_t)1 << 31), "tedspad_image_grid: the grid (%lld x %lld) is too large", (long long)Hg, (long long)Wg);
    *hg = (int32_t)Hg;
    *wg = (int32_t)Wg;
    return TEDSPAD_OK;
}

extern "C" int32_t tedspad_image_grid_u8(const float *x, uint8_t *out, int32_t N, int32_t H, int32_t W, int32_t nrow, int32_t pad, void *stream) {
    TS_REQUIRE(x && out, "tedspad_image_grid_u8: null argument");
    int32_t Hg = 0, Wg = 0;
    const int32_t rc = tedspad_image_grid_dims(N, H, W, nrow, pad, &Hg, &Wg);
    if (rc != TEDSPAD_OK) return rc;
    const int xmaps = nrow < N ? nrow : N;
    hipLaunchKernelGGL(image_grid_kernel, dim3((Hg * Wg + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, out, N, H, W, xmaps, pad, Hg, Wg);
    return check_launch("tedspad_image_grid_u8");
}

extern "C" int32_t tedspad_minmax_ws_floats(void) { return 2 * MM_BLOCKS; }

extern "C" int32_t tedspad_minmax_f32(const float *x, int64_t n, float *ws, float *out2, void *stream) {
    TS_REQUIRE(x && ws && out2 && n >= 1, "tedspad_minmax_f32: bad arguments");
    const int64_t want = (n + 255) / 256;
    const int blocks = (int)(want < MM_BLOCKS ? want : MM_BLOCKS);
    hipLaunchKernelGGL(minmax_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, (long)n, ws, 0);
    hipLaunchKernelGGL(minmax_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float *)ws, (long)blocks, out2, 1);
    return check_launch("tedspad_minmax_f32");
}

extern "C" int32_t tedspad_video_frames_u8(const float *x, const float *minmax, uint8_t *out, int32_t T, int32_t H, int32_t W, void *stream) {
    TS_REQUIRE(x && minmax && out && T >= 1 && H >= 1 && W >= 1, "tedspad_video_frames_u8: bad arguments");
    TS_REQUIRE((int64_t)H * W < ((int64_t)1 << 31) && (int64_t)T * H * W < ((int64_t)1 << 38), "tedspad_video_frames_u8: the video is too large");
    const int64_t npix = (int64_t)T * H * W;
    TS_REQUIRE((npix + 255) / 256 < ((int64_t)1 << 31), "tedspad_video_frames_u8: the video is too large");
    hipLaunchKernelGGL(video_frames_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, minmax, out, (long)npix, H * W);
    return check_launch("tedspad_video_frames_u8");
}
