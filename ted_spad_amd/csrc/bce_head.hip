// Fused multi-label head of the privacy classifier for gfx950: Linear(K -> N) + BCEWithLogitsLoss (mean) + every gradient, ONE launch
// (privacy_training/train_privacy.py:52-55: `criterion = nn.BCEWithLogitsLoss()` on the 7-way fc of a ResNet-50, params_privacy.py:9).
// Eager torch runs it as fc GEMV + loss kernel(s) + the three GEMVs of the fc backward.
//
//  z[b,n]   = sum_k f[b,k] W[n,k] + bias[n]
//  loss     = mean_{b,n} max(z,0) - z y + log1p(exp(-|z|))          (torch's numerically stable form)
//  g[b,n]   = (sigmoid(z) - y) / (B N)
//  df[b,k]  = s sum_n g[b,n] W[n,k]   dW[n,k] = s sum_b g[b,n] f[b,k]   db[n] = s sum_b g[b,n]      (s = grad_scale)
//
// The gradients need every logit, i.e. the whole K reduction, before they can start. Rather than a grid-wide barrier, every workgroup
// recomputes the B x N logits (a few hundred thousand FMAs, f and W come from L2) and then writes its own 256-column slice of df / dW;
// workgroup 0 also writes the logits, the loss and db. All sums run in a fixed order (per-lane strided partial sums, one xor-shuffle
// tree, then loops in index order): no float atomics, the result is the same on every run and in every workgroup.
//
// Logits mode (W == NULL): `f` already holds the (B, N) logits -- nn.BCEWithLogitsLoss on its own; df is then d(loss)/d(logits) x s.
#include "common.h"

namespace tedspad {
namespace {

constexpr int BCE_MAX_B = 128;
constexpr int BCE_MAX_N = 64;
constexpr int BCE_THREADS = 1024;
constexpr int BCE_COLS = 256;        // K columns per workgroup in the gradient phase (one float4 per lane)

__device__ __forceinline__ float bce_wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(BCE_THREADS) void bce_head_kernel(const float *f, const float *W, const float *bias, const float *y,
                                                                 float *logits, float *loss, float *df, float *dW, float *db,
                                                                 int B, int K, int N, float gscale) {
    __shared__ float zs[BCE_MAX_B * BCE_MAX_N];      // logits, then g = (sigmoid(z) - y) / (B N)
    __shared__ float red[BCE_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = BCE_THREADS / 64;
    const int BN = B * N;
    const bool first = blockIdx.x == 0;
    // ---- logits -----------------------------------------------------------------------------------------------------------------
    if (W) {
        for (int p = wave; p < BN; p += nwaves) {
            const int b = p / N, n = p - b * N;
            const float *pf = f + (size_t)b * K, *pw = W + (size_t)n * K;
            float acc = 0.f;
            for (int k = lane * 4; k < K; k += 256) {
                const f32x4 a = *reinterpret_cast<const f32x4 *>(pf + k), c = *reinterpret_cast<const f32x4 *>(pw + k);
                acc += a[0] * c[0] + a[1] * c[1] + a[2] * c[2] + a[3] * c[3];
            }
            acc = bce_wsum(acc);
            if (lane == 0) zs[p] = acc + (bias ? bias[n] : 0.f);
        }
    } else {
        for (int p = tid; p < BN; p += BCE_THREADS) zs[p] = f[p];
    }
    __syncthreads();
    // ---- element losses and logit gradients ------------------------------------------------------------------------------------
    const float inv = 1.f / (float)BN;
    float part = 0.f;
    for (int p = tid; p < BN; p += BCE_THREADS) {
        const float z = zs[p], t = y[p];
        const float e = expf(-fabsf(z));                               // in (0, 1]: no overflow for any z
        part += fmaxf(z, 0.f) - z * t + log1pf(e);
        const float sig = z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        if (first && logits) logits[p] = z;
        zs[p] = (sig - t) * inv;
    }
    part = bce_wsum(part);
    if (lane == 0) red[wave] = part;
    __syncthreads();
    if (first && tid == 0) {
        float s = 0.f;
        for (int w = 0; w < nwaves; ++w) s += red[w];
        loss[0] = s * inv;
    }
    if (!df) return;
    const float *g = zs;
    if (!W) {                                                          // logits mode: d(loss)/d(logits)
        for (int p = tid; p < BN; p += BCE_THREADS) df[p] = g[p] * gscale;
        return;
    }
    if (first && tid < N) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += g[b * N + tid];
        db[tid] = s * gscale;
    }
    // ---- this workgroup's columns of df (rows 0..B-1) and dW (rows B..B+N-1) ---------------------------------------------------
    const int k = blockIdx.x * BCE_COLS + lane * 4;
    if (k >= K) return;
    for (int r = wave; r < B + N; r += nwaves) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (r < B) {
            for (int n = 0; n < N; ++n) acc += g[r * N + n] * *reinterpret_cast<const f32x4 *>(W + (size_t)n * K + k);
            *reinterpret_cast<f32x4 *>(df + (size_t)r * K + k) = acc * gscale;
        } else {
            const int n = r - B;
            for (int b = 0; b < B; ++b) acc += g[b * N + n] * *reinterpret_cast<const f32x4 *>(f + (size_t)b * K + k);
            *reinterpret_cast<f32x4 *>(dW + (size_t)n * K + k) = acc * gscale;
        }
    }
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace tedspad

using namespace tedspad;

extern "C" int32_t tedspad_bce_head_fwd_bwd(const float *f, const float *W, const float *bias, const float *y, float *logits, float *loss,
                                            float *df, float *dW, float *db, int32_t B, int32_t K, int32_t N, float grad_scale,
                                            void *stream) {
    TS_REQUIRE(f && y && loss && B > 0 && N > 0 && K > 0, "tedspad_bce_head_fwd_bwd: bad arguments");
    TS_REQUIRE(B <= BCE_MAX_B && N <= BCE_MAX_N, "tedspad_bce_head_fwd_bwd: supports B <= %d and N <= %d (got B=%d, N=%d)", BCE_MAX_B,
               BCE_MAX_N, B, N);
    int grid = 1;
    if (W) {
        TS_REQUIRE(K % 4 == 0 && aligned16(f) && aligned16(W), "tedspad_bce_head_fwd_bwd: needs K %% 4 == 0 and 16-byte aligned f / W (K=%d)", K);
        TS_REQUIRE((!df && !dW && !db) || (df && dW && db), "tedspad_bce_head_fwd_bwd: pass df, dW and db, or none of them");
        TS_REQUIRE(!df || (aligned16(df) && aligned16(dW)), "tedspad_bce_head_fwd_bwd: df / dW must be 16-byte aligned");
        if (df) grid = (K + BCE_COLS - 1) / BCE_COLS;
    } else {
        TS_REQUIRE(!bias && !dW && !db && K == N, "tedspad_bce_head_fwd_bwd: logits mode (W == NULL) takes f = logits (B, N), K == N, no bias / dW / db");
    }
    hipLaunchKernelGGL(bce_head_kernel, dim3(grid), dim3(BCE_THREADS), 0, (hipStream_t)stream, f, W, bias, y, logits, loss, df, dW, db, B, K,
                       N, grad_scale);
    return check_launch("tedspad_bce_head_fwd_bwd");
}
