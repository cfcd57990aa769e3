// MGFN training for gfx950, all fp32: what one iteration of anomaly_detection_mgfn/train.py:79-106 needs beyond the forward kernels of
// mgfn.hip (same layout: token-major rows over a ragged batch, `bounds` / `seq_off`).
//
//   col_reduce       ordered column reductions over the tokens: bias gradients, LayerNorm / BatchNorm parameter gradients, BatchNorm sums,
//                    fc gradients. Pass 1: every MT_CHUNK-token chunk sums its tokens in order into a workspace; pass 2 adds the chunks in order
//   ln_apply / ln_bwd  (x - mean) rs g + b materialised (train mode cannot fold g / b into the GEMM: they need gradients), and its dx
//   bn_train_fwd/bwd BatchNorm1d over all tokens with batch statistics, running-statistics update, dx / dgamma / dbeta
//   gelu / gelu_bwd  exact-erf GELU on the kept pre-activation
//   transpose, wgrad the (taps * C, M) image of the k-tap window matrix and of dy; dW^T = A^T dy over the token axis on the f32 MFMA, split
//                    over fixed token slices into a workspace, the slices added in order
//   attention_bwd    GLANCE: dq per 32-query block, dk / dv per 32-key block, P recomputed from q, k and the row log-sum-exp; MFMA for
//                    every product
//   relpos_bwd       FOCUS rel_pos: dv (5-tap correlation with the flipped filter), d(weight), d(bias)
//   head_bwd         fc -> sigmoid backward into the to_logits LayerNorm output's gradient
//   msnsd            MSNSD's training branch (models/mgfn.py:18-86) + the cost of train.py:47-75, 8-20, 96-100 and its gradient
//
// No float atomics anywhere: every sum runs in an order fixed by the shapes, so two runs give the same bits.
#include "common.h"

namespace tedspad {
namespace {

constexpr int MT_CHUNK = 128;          // tokens per first-pass chunk of an ordered reduction
constexpr int MT_THREADS = 256;

__device__ __forceinline__ float wsum64(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

#define MT_ROW(e, hf) (((e) & 3) + 8 * ((e) >> 2) + 4 * (hf))          // row of MFMA accumulator register e

inline bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }
inline int nchunks_of(int M) { return (M + MT_CHUNK - 1) / MT_CHUNK; }

// ---- ordered column reductions --------------------------------------------------------------------------------------------------------
enum { CR_SUM = 0, CR_LN = 1, CR_BN = 2, CR_SQ = 3, CR_ROW = 4 };

__global__ void col_partial_kernel(const float *a, int lda, const float *x, int ldx, const float *st, int mode, int M, int C, float *ws) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, chunk = blockIdx.y;
    if (c >= C) return;
    const int m0 = chunk * MT_CHUNK, m1 = min(M, m0 + MT_CHUNK);
    float s0 = 0.f, s1 = 0.f;
    const float cm = (mode == CR_BN || mode == CR_SQ) ? st[c] : 0.f, ci = mode == CR_BN ? st[C + c] : 1.f;
    for (int m = m0; m < m1; ++m) {
        const float av = a[(size_t)m * lda + c];
        if (mode == CR_SUM) {
            s0 += av;
        } else if (mode == CR_LN) {
            s0 += av;
            s1 += av * ((x[(size_t)m * ldx + c] - st[2 * m]) * st[2 * m + 1]);
        } else if (mode == CR_BN) {
            s0 += av;
            s1 += av * ((x[(size_t)m * ldx + c] - cm) * ci);
        } else if (mode == CR_SQ) {
            const float d = av - cm;
            s0 += d * d;
        } else {
            s0 += st[m] * av;
            s1 += st[m];
        }
    }
    ws[((size_t)chunk * 2) * C + c] = s0;
    ws[((size_t)chunk * 2 + 1) * C + c] = s1;
}

__global__ void col_final_kernel(const float *ws, int nchunks, int C, float scale, float *out0, float *out1) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float s0 = 0.f, s1 = 0.f;
    for (int k = 0; k < nchunks; ++k) {
        s0 += ws[((size_t)k * 2) * C + c];
        s1 += ws[((size_t)k * 2 + 1) * C + c];
    }
    if (out0) out0[c] = s0 * scale;
    if (out1) out1[c] = s1 * scale;
}

void col_reduce(const float *a, int lda, const float *x, int ldx, const float *st, int mode, int M, int C, float scale, float *ws, float *out0,
                float *out1, hipStream_t s) {
    const int bt = C >= MT_THREADS ? MT_THREADS : 64, nb = (C + bt - 1) / bt, nch = nchunks_of(M);
    hipLaunchKernelGGL(col_partial_kernel, dim3(nb, nch), dim3(bt), 0, s, a, lda, x, ldx, st, mode, M, C, ws);
    hipLaunchKernelGGL(col_final_kernel, dim3(nb), dim3(bt), 0, s, ws, nch, C, scale, out0, out1);
}

// ---- LayerNorm (both flavours: the row statistics of tedspad_mgfn_ln_stats say which) ---------------------------------------------------
__global__ void ln_apply_kernel(const float *x, int ldx, const float *stats, const float *g, const float *b, int M, int C, float *y, int ldy) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c4 = C / 4;
    if (idx >= (long long)M * c4) return;
    const int m = (int)(idx / c4), c = (int)(idx - (long long)m * c4) * 4;
    const f32x4 v = (*reinterpret_cast<const f32x4 *>(x + (size_t)m * ldx + c) - stats[2 * m]) * stats[2 * m + 1] *
                        *reinterpret_cast<const f32x4 *>(g + c) + *reinterpret_cast<const f32x4 *>(b + c);
    *reinterpret_cast<f32x4 *>(y + (size_t)m * ldy + c) = v;
}

// y = xh g + b, xh = (x - mean) rs, rs = 1 / (std + eps) (MGFN, utils.py:108-111) or 1 / sqrt(var + eps) (nn.LayerNorm). With dxh = dy g,
// s1 = mean_c dxh, s2 = mean_c dxh xh:  dx = rs (dxh - s1) - xh s2 / D, D = d(denominator)/d(std-like) = std (MGFN) or sqrt(var + eps).
__global__ __launch_bounds__(MT_THREADS) void ln_bwd_kernel(const float *dy, int lddy, const float *x, int ldx, const float *stats,
                                                            const float *g, int torch_ln, float eps, const float *add, int ldadd, float *dx,
                                                            int lddx, int M, int C) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * (MT_THREADS / 64) + (threadIdx.x >> 6);
    if (m >= M) return;
    const float mean = stats[2 * m], rs = stats[2 * m + 1];
    const float *xr = x + (size_t)m * ldx, *dr = dy + (size_t)m * lddy;
    float s1 = 0.f, s2 = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        const f32x4 xh = (*reinterpret_cast<const f32x4 *>(xr + c) - mean) * rs;
        const f32x4 d = *reinterpret_cast<const f32x4 *>(dr + c) * *reinterpret_cast<const f32x4 *>(g + c);
        s1 += (d[0] + d[1]) + (d[2] + d[3]);
        s2 += (d[0] * xh[0] + d[1] * xh[1]) + (d[2] * xh[2] + d[3] * xh[3]);
    }
    s1 = wsum64(s1) / (float)C;
    s2 = wsum64(s2) / (float)C;
    const float k2 = s2 * (torch_ln ? rs : 1.f / (1.f / rs - eps));
    for (int c = lane * 4; c < C; c += 256) {
        const f32x4 xh = (*reinterpret_cast<const f32x4 *>(xr + c) - mean) * rs;
        const f32x4 d = *reinterpret_cast<const f32x4 *>(dr + c) * *reinterpret_cast<const f32x4 *>(g + c);
        f32x4 v = (d - s1) * rs - xh * k2;
        if (add) v += *reinterpret_cast<const f32x4 *>(add + (size_t)m * ldadd + c);
        *reinterpret_cast<f32x4 *>(dx + (size_t)m * lddx + c) = v;
    }
}

// ---- BatchNorm1d over all tokens, train mode -------------------------------------------------------------------------------------------
// stat = mean (C) | var on entry, invstd on exit (C)
__global__ void bn_finish_kernel(float *stat, int M, int C, float eps, float momentum, float *rmean, float *rvar) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float mean = stat[c], var = stat[C + c];
    stat[C + c] = 1.f / sqrtf(var + eps);
    if (rmean) {
        rmean[c] = (1.f - momentum) * rmean[c] + momentum * mean;
        rvar[c] = (1.f - momentum) * rvar[c] + momentum * (M > 1 ? var * ((float)M / (float)(M - 1)) : var);   // unbiased, as nn.BatchNorm1d
    }
}

__global__ void bn_apply_kernel(const float *x, int ldx, const float *stat, const float *gamma, const float *beta, int M, int C, float *y,
                                int ldy) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c4 = C / 4;
    if (idx >= (long long)M * c4) return;
    const int m = (int)(idx / c4), c = (int)(idx - (long long)m * c4) * 4;
    const f32x4 v = (*reinterpret_cast<const f32x4 *>(x + (size_t)m * ldx + c) - *reinterpret_cast<const f32x4 *>(stat + c)) *
                        *reinterpret_cast<const f32x4 *>(stat + C + c) * *reinterpret_cast<const f32x4 *>(gamma + c) +
                    *reinterpret_cast<const f32x4 *>(beta + c);
    *reinterpret_cast<f32x4 *>(y + (size_t)m * ldy + c) = v;
}

// dx = gamma invstd (dy - dbeta / M - xh dgamma / M) [+ add]
__global__ void bn_bwd_apply_kernel(const float *dy, int lddy, const float *x, int ldx, const float *stat, const float *gamma,
                                    const float *dgamma, const float *dbeta, const float *add, int ldadd, int M, int C, float *dx, int lddx) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c4 = C / 4;
    if (idx >= (long long)M * c4) return;
    const int m = (int)(idx / c4), c = (int)(idx - (long long)m * c4) * 4;
    const f32x4 is = *reinterpret_cast<const f32x4 *>(stat + C + c);
    const f32x4 xh = (*reinterpret_cast<const f32x4 *>(x + (size_t)m * ldx + c) - *reinterpret_cast<const f32x4 *>(stat + c)) * is;
    const float inv = 1.f / (float)M;
    f32x4 v = *reinterpret_cast<const f32x4 *>(gamma + c) * is *
              (*reinterpret_cast<const f32x4 *>(dy + (size_t)m * lddy + c) - *reinterpret_cast<const f32x4 *>(dbeta + c) * inv -
               xh * *reinterpret_cast<const f32x4 *>(dgamma + c) * inv);
    if (add) v += *reinterpret_cast<const f32x4 *>(add + (size_t)m * ldadd + c);
    *reinterpret_cast<f32x4 *>(dx + (size_t)m * lddx + c) = v;
}

// ---- exact-erf GELU (nn.GELU(), Q-M5) --------------------------------------------------------------------------------------------------
__global__ void gelu_kernel(const float *x, float *y, long long n4) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const f32x4 v = reinterpret_cast<const f32x4 *>(x)[i];
    f32x4 o;
#pragma unroll
    for (int u = 0; u < 4; ++u) o[u] = 0.5f * v[u] * (1.f + erff(v[u] * 0.70710678118654752440f));
    reinterpret_cast<f32x4 *>(y)[i] = o;
}

__global__ void gelu_bwd_kernel(const float *x, const float *dy, float *dx, long long n4) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const f32x4 v = reinterpret_cast<const f32x4 *>(x)[i], d = reinterpret_cast<const f32x4 *>(dy)[i];
    f32x4 o;
#pragma unroll
    for (int u = 0; u < 4; ++u)   // d/dx [x Phi(x)] = Phi(x) + x phi(x)
        o[u] = d[u] * (0.5f * (1.f + erff(v[u] * 0.70710678118654752440f)) + v[u] * 0.39894228040143267794f * expf(-0.5f * v[u] * v[u]));
    reinterpret_cast<f32x4 *>(dx)[i] = o;
}

// ---- transposed k-tap window: out[(t C + c) ldo + m] = x[m + t - taps / 2, c], zero outside m's sequence and for M <= m < ldo --------------
__global__ __launch_bounds__(256) void transpose_kernel(const float *x, int ldx, const int *bounds, int taps, int M, int C, float *out, int ldo) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;            // 32 x 8
    const int m0 = blockIdx.x * 32, c0 = blockIdx.y * 32, t = blockIdx.z, sh = t - (taps >> 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = m0 + ty + 8 * r, c = c0 + tx;
        float v = 0.f;
        if (m < M && c < C) {
            const int src = m + sh;
            const int lo = bounds ? bounds[2 * m] : m, hi = bounds ? bounds[2 * m + 1] : m + 1;
            if (src >= lo && src < hi) v = x[(size_t)src * ldx + c];
        }
        tile[ty + 8 * r][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int c = c0 + ty + 8 * r, m = m0 + tx;
        if (c < C && m < ldo) out[((size_t)t * C + c) * ldo + m] = tile[tx][ty + 8 * r];
    }
}

// ---- weight gradient: dW^T (rows, N) = A^T (rows, K) . dy^T (N, K)^T with the token axis as K, on the f32 MFMA -------------------------------
// One wave per (64 x 64 output tile, K slice): operands as gemm_kernel (mgfn.hip) takes them, lane (i, h) loads 8 consecutive K values of
// its row per 16-wide chunk. The slices (a count fixed by the shapes alone) go to a workspace and are added in order by wgrad_reduce_kernel.
__global__ __launch_bounds__(64) void wgrad_kernel(const float *at, const float *dyt, int ldk, int rows, int N, int kslice, float *out) {
    const int lane = threadIdx.x, i = lane & 31, hf = lane >> 5;
    const int n0 = blockIdx.x * 64, r0 = blockIdx.y * 64, k0 = blockIdx.z * kslice, k1 = min(ldk, k0 + kslice);
    const float *arow[2], *brow[2];
    bool aok[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int row = r0 + 32 * r + i;
        aok[r] = row < rows;
        arow[r] = at + (size_t)(aok[r] ? row : rows - 1) * ldk + 8 * hf;
        brow[r] = dyt + (size_t)(n0 + 32 * r + i) * ldk + 8 * hf;
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[r][c][e] = 0.f;
    for (int k = k0; k < k1; k += 16) {
        f32x4 a[2][2], b[2][2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            a[r][0] = *reinterpret_cast<const f32x4 *>(arow[r] + k);
            a[r][1] = *reinterpret_cast<const f32x4 *>(arow[r] + k + 4);
            if (!aok[r]) {
                a[r][0] = f32x4{0.f, 0.f, 0.f, 0.f};
                a[r][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            b[r][0] = *reinterpret_cast<const f32x4 *>(brow[r] + k);
            b[r][1] = *reinterpret_cast<const f32x4 *>(brow[r] + k + 4);
        }
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c)
                    acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r][s >> 2][s & 3], b[c][s >> 2][s & 3], acc[r][c], 0, 0, 0);
    }
    float *o = out + (size_t)blockIdx.z * rows * N;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = r0 + 32 * r + MT_ROW(e, hf);
                if (row < rows) o[(size_t)row * N + n0 + 32 * c + i] = acc[r][c][e];
            }
}

__global__ void wgrad_reduce_kernel(const float *ws, int nslices, long long n4, float *out) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n4) return;
    f32x4 s = reinterpret_cast<const f32x4 *>(ws)[e];
    for (int k = 1; k < nslices; ++k) s += reinterpret_cast<const f32x4 *>(ws)[(size_t)k * n4 + e];
    reinterpret_cast<f32x4 *>(out)[e] = s;
}

// K slice of a weight gradient: enough slices for ~2048 waves, at least 128 tokens each; a function of the shapes only
inline int wgrad_kslice(int ldk, int rows, int N) {
    const long long tiles = (long long)((rows + 63) / 64) * (N / 64);
    long long want = (2048 + tiles - 1) / tiles;
    const long long most = (ldk + 127) / 128;
    if (want > most) want = most;
    if (want < 1) want = 1;
    const int ks = (int)(((ldk + want - 1) / want + 15) / 16 * 16);
    return ks;
}

// ---- GLANCE attention backward ----------------------------------------------------------------------------------------------------------
// Operand layouts as attention_kernel (mgfn.hip): an MFMA result has its column on the lane and its rows in the 16 registers,
// row(e) = (e & 3) + 8 (e >> 2) + 4 (lane >> 5). With S = (q / 8) K^T, P = softmax(S), O = P V, D_i = dO_i . O_i:
//   dP = dO V^T, dS = P (dP - D), dq = dS K / 8, dk = dS^T q / 8, dv = P^T dO.
constexpr int AT_D = 64;

// One wave per (sequence, 32 queries, head): dq, and the rows' log-sum-exp L and D into lse (token, head, 2) for the key-block kernel.
__global__ __launch_bounds__(64) void attn_bwd_q_kernel(const float *qkv, int ldqkv, const float *o, int ldo, const float *dO, int lddo,
                                                        const int *seq_off, int heads, float *dqkv, int lddqkv, float *lse) {
    __shared__ float Pl[32][33];
    __shared__ float Dl[32];
    const int lane = threadIdx.x, i = lane & 31, hf = lane >> 5;
    const int seq = blockIdx.x, head = blockIdx.z;
    const int base = seq_off[seq], T = seq_off[seq + 1] - base;
    const int q0 = blockIdx.y * 32;
    if (q0 >= T) return;
    const int inner = heads * AT_D;
    const float *Q = qkv + (size_t)base * ldqkv + head * AT_D;
    const float *Kp = Q + inner, *Vp = Q + 2 * inner;
    const int qi = min(q0 + i, T - 1);                        // rows past the end compute a copy of the last row; never stored
    float q[32], dor[32];
    {
        const float *orow = o + (size_t)(base + qi) * ldo + head * AT_D + 32 * hf;
        const float *drow = dO + (size_t)(base + qi) * lddo + head * AT_D + 32 * hf;
        float part = 0.f;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const f32x4 t = *reinterpret_cast<const f32x4 *>(Q + (size_t)qi * ldqkv + 32 * hf + 4 * v) * 0.125f;
            const f32x4 d = *reinterpret_cast<const f32x4 *>(drow + 4 * v), ov = *reinterpret_cast<const f32x4 *>(orow + 4 * v);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                q[4 * v + u] = t[u];
                dor[4 * v + u] = d[u];
                part += d[u] * ov[u];
            }
        }
        part += __shfl_xor(part, 32, 64);
        if (hf == 0) Dl[i] = part;
    }
    __syncthreads();
    float Drow[16], mrow[16], lrow[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        Drow[e] = Dl[MT_ROW(e, hf)];
        mrow[e] = -INFINITY;
        lrow[e] = 0.f;
    }
    auto scores = [&](int kj, f32x16 &s) {
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const f32x4 kk = *reinterpret_cast<const f32x4 *>(Kp + (size_t)kj * ldqkv + 32 * hf + 4 * v);
#pragma unroll
            for (int u = 0; u < 4; ++u) s = __builtin_amdgcn_mfma_f32_32x32x2f32(q[4 * v + u], kk[u], s, 0, 0, 0);
        }
    };
    for (int kb = 0; kb < T; kb += 32) {                      // pass 1: the rows' max and sum
        const bool kval = kb + i < T;
        f32x16 s;
        scores(kval ? kb + i : T - 1, s);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float sv = kval ? s[e] : -INFINITY;
            float mx = sv;
#pragma unroll
            for (int w = 16; w > 0; w >>= 1) mx = fmaxf(mx, __shfl_xor(mx, w, 64));
            const float mnew = fmaxf(mrow[e], mx);
            float ps = expf(sv - mnew);
#pragma unroll
            for (int w = 16; w > 0; w >>= 1) ps += __shfl_xor(ps, w, 64);
            lrow[e] = lrow[e] * expf(mrow[e] - mnew) + ps;
            mrow[e] = mnew;
        }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) mrow[e] += logf(lrow[e]);    // L = log sum exp
    f32x16 dq0, dq1;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        dq0[e] = 0.f;
        dq1[e] = 0.f;
    }
    for (int kb = 0; kb < T; kb += 32) {                      // pass 2: dS and dq += dS K
        const bool kval = kb + i < T;
        const int kj = kval ? kb + i : T - 1;
        f32x16 s, dp;
        scores(kj, s);
#pragma unroll
        for (int e = 0; e < 16; ++e) dp[e] = 0.f;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const f32x4 vv = *reinterpret_cast<const f32x4 *>(Vp + (size_t)kj * ldqkv + 32 * hf + 4 * v);
#pragma unroll
            for (int u = 0; u < 4; ++u) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(dor[4 * v + u], vv[u], dp, 0, 0, 0);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float p = kval ? expf(s[e] - mrow[e]) : 0.f;
            Pl[MT_ROW(e, hf)][i] = p * (dp[e] - Drow[e]);
        }
        __syncthreads();
#pragma unroll
        for (int st = 0; st < 16; ++st) {
            const int key = kb + 16 * hf + st;
            const bool vk = key < T;
            const float *kr = Kp + (size_t)(vk ? key : T - 1) * ldqkv;
            const float pa = Pl[i][16 * hf + st];
            const float k0 = vk ? kr[i] : 0.f, k1 = vk ? kr[32 + i] : 0.f;
            dq0 = __builtin_amdgcn_mfma_f32_32x32x2f32(pa, k0, dq0, 0, 0, 0);
            dq1 = __builtin_amdgcn_mfma_f32_32x32x2f32(pa, k1, dq1, 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int r = q0 + MT_ROW(e, hf);
        if (r >= T) continue;
        float *drow = dqkv + (size_t)(base + r) * lddqkv + head * AT_D;
        drow[i] = dq0[e] * 0.125f;
        drow[32 + i] = dq1[e] * 0.125f;
        if (i == 0) {
            float *l = lse + ((size_t)(base + r) * heads + head) * 2;
            l[0] = mrow[e];
            l[1] = Drow[e];
        }
    }
}

// One wave per (sequence, 32 keys, head): dk and dv, over all query blocks in order. S^T = K (q / 8)^T has the query on the lane.
__global__ __launch_bounds__(64) void attn_bwd_kv_kernel(const float *qkv, int ldqkv, const float *dO, int lddo, const int *seq_off, int heads,
                                                         const float *lse, float *dqkv, int lddqkv) {
    __shared__ float PT[32][33];
    __shared__ float ST[32][33];
    const int lane = threadIdx.x, i = lane & 31, hf = lane >> 5;
    const int seq = blockIdx.x, head = blockIdx.z;
    const int base = seq_off[seq], T = seq_off[seq + 1] - base;
    const int k0b = blockIdx.y * 32;
    if (k0b >= T) return;
    const int inner = heads * AT_D;
    const float *Q = qkv + (size_t)base * ldqkv + head * AT_D;
    const float *Kp = Q + inner, *Vp = Q + 2 * inner;
    const float *dOp = dO + (size_t)base * lddo + head * AT_D;
    const int kj = min(k0b + i, T - 1);
    float kreg[32], vreg[32];
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(Kp + (size_t)kj * ldqkv + 32 * hf + 4 * v);
        const f32x4 b = *reinterpret_cast<const f32x4 *>(Vp + (size_t)kj * ldqkv + 32 * hf + 4 * v);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            kreg[4 * v + u] = a[u];
            vreg[4 * v + u] = b[u];
        }
    }
    f32x16 dk0, dk1, dv0, dv1;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        dk0[e] = 0.f;
        dk1[e] = 0.f;
        dv0[e] = 0.f;
        dv1[e] = 0.f;
    }
    for (int qb = 0; qb < T; qb += 32) {
        const bool qval = qb + i < T;
        const int qi = qval ? qb + i : T - 1;
        f32x16 sT, dpT;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            sT[e] = 0.f;
            dpT[e] = 0.f;
        }
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const f32x4 qq = *reinterpret_cast<const f32x4 *>(Q + (size_t)qi * ldqkv + 32 * hf + 4 * v) * 0.125f;
            const f32x4 dd = *reinterpret_cast<const f32x4 *>(dOp + (size_t)qi * lddo + 32 * hf + 4 * v);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                sT = __builtin_amdgcn_mfma_f32_32x32x2f32(kreg[4 * v + u], qq[u], sT, 0, 0, 0);
                dpT = __builtin_amdgcn_mfma_f32_32x32x2f32(vreg[4 * v + u], dd[u], dpT, 0, 0, 0);
            }
        }
        const float *l = lse + ((size_t)(base + qi) * heads + head) * 2;
        const float L = l[0], D = l[1];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int r = MT_ROW(e, hf);
            const float p = (qval && k0b + r < T) ? expf(sT[e] - L) : 0.f;
            PT[r][i] = p;
            ST[r][i] = p * (dpT[e] - D);
        }
        __syncthreads();
#pragma unroll
        for (int st = 0; st < 16; ++st) {
            const int qq = qb + 16 * hf + st;
            const bool vq = qq < T;
            const float *dr = dOp + (size_t)(vq ? qq : T - 1) * lddo;
            const float *qr = Q + (size_t)(vq ? qq : T - 1) * ldqkv;
            const float pa = PT[i][16 * hf + st], sa = ST[i][16 * hf + st];
            const float d0 = vq ? dr[i] : 0.f, d1 = vq ? dr[32 + i] : 0.f, c0 = vq ? qr[i] : 0.f, c1 = vq ? qr[32 + i] : 0.f;
            dv0 = __builtin_amdgcn_mfma_f32_32x32x2f32(pa, d0, dv0, 0, 0, 0);
            dv1 = __builtin_amdgcn_mfma_f32_32x32x2f32(pa, d1, dv1, 0, 0, 0);
            dk0 = __builtin_amdgcn_mfma_f32_32x32x2f32(sa, c0, dk0, 0, 0, 0);
            dk1 = __builtin_amdgcn_mfma_f32_32x32x2f32(sa, c1, dk1, 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int r = k0b + MT_ROW(e, hf);
        if (r >= T) continue;
        float *drow = dqkv + (size_t)(base + r) * lddqkv + head * AT_D;
        drow[inner + i] = dk0[e] * 0.125f;
        drow[inner + 32 + i] = dk1[e] * 0.125f;
        drow[2 * inner + i] = dv0[e];
        drow[2 * inner + 32 + i] = dv1[e];
    }
}

// ---- FOCUS rel_pos backward ------------------------------------------------------------------------------------------------------------
// out[m, c] = b[c % heads] + sum_t w[c % heads, t] v[m + t - 2, c]  =>  dv[m, c] = sum_t w[c % heads, t] dout[m - t + 2, c]
__global__ void relpos_bwd_dv_kernel(const float *dout, int lddo, const int *bounds, int M, int C, int heads, const float *w, float *dv,
                                     int lddv) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c4 = C / 4;
    if (idx >= (long long)M * c4) return;
    const int m = (int)(idx / c4), c = (int)(idx - (long long)m * c4) * 4;
    const int lo = bounds[2 * m], hi = bounds[2 * m + 1];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        const int src = m - t + 2;
        if (src < lo || src >= hi) continue;
        const f32x4 d = *reinterpret_cast<const f32x4 *>(dout + (size_t)src * lddo + c);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] += w[((c + u) % heads) * 5 + t] * d[u];
    }
    *reinterpret_cast<f32x4 *>(dv + (size_t)m * lddv + c) = acc;
}

// ws[(chunk * 6 + j) * C + c]: j < 5: sum_m dout[m, c] v[m + j - 2, c]; j == 5: sum_m dout[m, c], over the chunk's tokens in order
__global__ void relpos_bwd_partial_kernel(const float *dout, int lddo, const float *v, int ldv, const int *bounds, int M, int C, float *ws) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, chunk = blockIdx.y;
    if (c >= C) return;
    const int m0 = chunk * MT_CHUNK, m1 = min(M, m0 + MT_CHUNK);
    float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int m = m0; m < m1; ++m) {
        const float d = dout[(size_t)m * lddo + c];
        const int lo = bounds[2 * m], hi = bounds[2 * m + 1];
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const int src = m + t - 2;
            if (src >= lo && src < hi) s[t] += d * v[(size_t)src * ldv + c];
        }
        s[5] += d;
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) ws[((size_t)chunk * 6 + j) * C + c] = s[j];
}

// one block per (head, j): thread t adds entries t, t + 256, ... of the (chunk, channel of the head) list in order, then a fixed tree
__global__ __launch_bounds__(256) void relpos_bwd_final_kernel(const float *ws, int nchunks, int C, int heads, float *dw, float *db) {
    __shared__ float sm[256];
    const int h = blockIdx.x / 6, j = blockIdx.x - 6 * h, per = C / heads, total = nchunks * per;
    float s = 0.f;
    for (int e = threadIdx.x; e < total; e += 256) {
        const int k = e / per, c = h + (e - k * per) * heads;
        s += ws[((size_t)k * 6 + j) * C + c];
    }
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (j < 5)
            dw[h * 5 + j] = sm[0];
        else
            db[h] = sm[0];
    }
}

// ---- head backward: score = sigmoid(h . fw + fb); dh += dz fw with dz = dscore s (1 - s) ---------------------------------------------------
__global__ __launch_bounds__(MT_THREADS) void head_bwd_kernel(const float *score, const float *dscore, const float *fw, int M, int C, float *dh,
                                                              float *dz) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * (MT_THREADS / 64) + (threadIdx.x >> 6);
    if (m >= M) return;
    const float s = score[m], z = dscore[m] * s * (1.f - s);
    for (int c = lane * 4; c < C; c += 256) {
        f32x4 *p = reinterpret_cast<f32x4 *>(dh + (size_t)m * C + c);
        *p = *p + *reinterpret_cast<const f32x4 *>(fw + c) * z;
    }
    if (lane == 0) dz[m] = z;
}

// ---- MSNSD (training branch) and the cost -------------------------------------------------------------------------------------------------
// Videos 0 .. n-1 are normal, n .. 2n-1 abnormal (train.py:85); token of (video, crop, segment) = (video ncrops + crop) T + segment.
// masks (2, n, T): [0] = select_idx (abnormal), [1] = select_idx_normal (models/mgfn.py:43-44, 65-66).
constexpr int MS_MAXK = 8;

// one thread per video: the k largest masked crop-mean magnitudes, descending, ties to the lowest index; the mean of their crop-mean scores
__global__ void msnsd_select_kernel(const float *crop_mags, const float *crop_scores, const float *masks, int n, int T, int k, int *idx,
                                    float *vid_score) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= 2 * n) return;
    const float *mg = crop_mags + (size_t)v * T;
    const float *mk = v < n ? masks + ((size_t)n + v) * T : masks + (size_t)(v - n) * T;
    float ssum = 0.f;
    for (int j = 0; j < k; ++j) {
        int best = -1;
        float bv = 0.f;
        for (int t = 0; t < T; ++t) {
            bool taken = false;
            for (int u = 0; u < j; ++u) taken |= idx[v * k + u] == t;          // this thread's own earlier picks
            if (taken) continue;
            const float val = mg[t] * mk[t];
            if (best < 0 || val > bv) {
                best = t;
                bv = val;
            }
        }
        idx[v * k + j] = best;
        ssum += crop_scores[(size_t)v * T + best];
    }
    vid_score[v] = ssum / (float)k;
}

// one wave per (video, crop, j): l1[half][(crop n + video') k + j] = sum_c |h[token, c]|   (train.py:67-73: torch.norm(p = 1, dim = 2))
__global__ __launch_bounds__(MT_THREADS) void msnsd_l1_kernel(const float *h, const int *idx, int n, int ncrops, int T, int C, int k, float *l1) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * (MT_THREADS / 64) + (threadIdx.x >> 6);
    if (w >= 2 * n * ncrops * k) return;
    const int j = w % k, crop = (w / k) % ncrops, v = w / (k * ncrops);
    const float *row = h + ((size_t)(v * ncrops + crop) * T + idx[v * k + j]) * C;
    float s = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        const f32x4 x = *reinterpret_cast<const f32x4 *>(row + c);
        s += (fabsf(x[0]) + fabsf(x[1])) + (fabsf(x[2]) + fabsf(x[3]));
    }
    s = wsum64(s);
    const int half = v < n ? 1 : 0, vv = v < n ? v : v - n;                 // half 0: abnormal, 1: normal
    if (lane == 0) l1[((size_t)half * n * ncrops + crop * n + vv) * k + j] = s;
}

__device__ float block_sum(float v, float *sm) {       // fixed tree over 256 threads
    __syncthreads();
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    return sm[0];
}

// One block. losses: cost, smooth, sparse, cls, con, con_n, con_a, total. dl1 (2, R, k), dcs (2n, T): d cost / d (L1 norm, crop-mean score).
__global__ __launch_bounds__(256) void msnsd_cost_kernel(const float *vid_score, const float *labels, const float *l1, const float *crop_scores,
                                                         const int *idx, int n, int ncrops, int T, int k, float *losses, float *dl1, float *dcs,
                                                         float *dvid) {
    __shared__ float sm[256];
    const int tid = threadIdx.x, R = n * ncrops, sep = R / 2, L = n * T;
    const float *A = l1, *N = l1 + (size_t)R * k;
    float *dA = dl1, *dN = dl1 + (size_t)R * k;
    // BCELoss (train.py:66): logs clamped at -100; gradient (s - y) / max(s (1 - s), 1e-12) / count, as torch's backward
    float acc = 0.f;
    for (int v = tid; v < 2 * n; v += 256) {
        const float s = vid_score[v], y = labels[v];
        acc -= y * fmaxf(logf(s), -100.f) + (1.f - y) * fmaxf(log1pf(-s), -100.f);
        dvid[v] = (s - y) / fmaxf(s * (1.f - s), 1e-12f) / (float)(2 * n);
    }
    const float loss_cls = block_sum(acc, sm) / (float)(2 * n);
    // ContrastiveLoss (train.py:28-32), margin 200, F.pairwise_distance: ||o1 - o2 + 1e-6||_2 over k
    acc = 0.f;
    for (int r = tid; r < R; r += 256) {                                    // abnormal vs normal, label 1, weight 0.001 * 0.001
        float d2 = 0.f;
        for (int j = 0; j < k; ++j) {
            const float df = A[r * k + j] - N[r * k + j] + 1e-6f;
            d2 += df * df;
        }
        const float d = sqrtf(d2), hinge = fmaxf(200.f - d, 0.f);
        acc += hinge * hinge;
        const float gd = d > 0.f ? -2.f * hinge / (float)R * 1e-6f / d : 0.f;
        for (int j = 0; j < k; ++j) {
            const float df = A[r * k + j] - N[r * k + j] + 1e-6f;
            dA[r * k + j] = gd * df;
            dN[r * k + j] = -gd * df;
        }
    }
    const float loss_con = block_sum(acc, sm) / (float)R;
    float con2[2];
#pragma unroll
    for (int which = 0; which < 2; ++which) {                                // second half vs first half, label 0, weight 0.001
        const float *X = which ? A : N;
        float *dX = which ? dA : dN;
        acc = 0.f;
        for (int r = tid; r < sep; r += 256) {
            float d2 = 0.f;
            for (int j = 0; j < k; ++j) {
                const float df = X[(sep + r) * k + j] - X[r * k + j] + 1e-6f;
                d2 += df * df;
                const float gdf = 2.f * df / (float)sep * 1e-3f;
                dX[(sep + r) * k + j] += gdf;
                dX[r * k + j] -= gdf;
            }
            acc += d2;
        }
        con2[which] = block_sum(acc, sm) / (float)sep;
    }
    const float loss_con_n = con2[0], loss_con_a = con2[1];
    // sparsity and smooth on the flattened abnormal crop-mean scores (train.py:8-20, 88-98)
    const float *a = crop_scores + (size_t)n * T;
    acc = 0.f;
    for (int t = tid; t < L; t += 256) acc += a[t] * a[t];
    const float nrm = sqrtf(block_sum(acc, sm));
    acc = 0.f;
    for (int t = tid; t + 1 < L; t += 256) acc += (a[t + 1] - a[t]) * (a[t + 1] - a[t]);
    const float loss_smooth = 8e-4f * block_sum(acc, sm), loss_sparse = 8e-3f * nrm;
    for (int e = tid; e < 2 * n * T; e += 256) {
        const int v = e / T, t = e - v * T;
        float g = 0.f;
        for (int j = 0; j < k; ++j)
            if (idx[v * k + j] == t) g += dvid[v] / (float)k;
        if (v >= n) {
            const int p = e - n * T;
            if (nrm > 0.f) g += 8e-3f * a[p] / nrm;
            float ds = 0.f;
            if (p >= 1) ds += a[p] - a[p - 1];
            if (p + 1 < L) ds -= a[p + 1] - a[p];
            g += 8e-4f * 2.f * ds;
        }
        dcs[e] = g;
    }
    if (tid == 0) {
        const float total = loss_cls + (0.001f * loss_con + loss_con_a + loss_con_n) * 0.001f;
        losses[0] = total + loss_smooth + loss_sparse;
        losses[1] = loss_smooth;
        losses[2] = loss_sparse;
        losses[3] = loss_cls;
        losses[4] = loss_con;
        losses[5] = loss_con_n;
        losses[6] = loss_con_a;
        losses[7] = total;
    }
}

// one wave per token: dscore = dcs / ncrops; dh row = dl1 sign(h) on a selected segment, else 0
__global__ __launch_bounds__(MT_THREADS) void msnsd_scatter_kernel(const float *h, const int *idx, const float *dl1, const float *dcs, int n,
                                                                   int ncrops, int T, int C, int k, float *dscore, float *dh) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * (MT_THREADS / 64) + (threadIdx.x >> 6);
    if (m >= 2 * n * ncrops * T) return;
    const int t = m % T, crop = (m / T) % ncrops, v = m / (T * ncrops);
    int j = -1;
    for (int u = 0; u < k; ++u)
        if (idx[v * k + u] == t) j = u;
    const int half = v < n ? 1 : 0, vv = v < n ? v : v - n;
    const float coef = j >= 0 ? dl1[((size_t)half * n * ncrops + crop * n + vv) * k + j] : 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        if (j >= 0) {
            const f32x4 x = *reinterpret_cast<const f32x4 *>(h + (size_t)m * C + c);
#pragma unroll
            for (int u = 0; u < 4; ++u) o[u] = x[u] > 0.f ? coef : (x[u] < 0.f ? -coef : 0.f);
        }
        *reinterpret_cast<f32x4 *>(dh + (size_t)m * C + c) = o;
    }
    if (lane == 0) dscore[m] = dcs[v * T + t] / (float)ncrops;
}

}  // namespace
}  // namespace tedspad

using namespace tedspad;

extern "C" int64_t tedspad_mgfn_train_ws_floats(int32_t M, int32_t C) { return (int64_t)nchunks_of(M > 0 ? M : 1) * 6 * (C > 0 ? C : 1); }

extern "C" int32_t tedspad_mgfn_col_reduce(const float *a, int32_t lda, const float *x, int32_t ldx, const float *st, int32_t mode, int32_t M,
                                           int32_t C, float scale, float *ws, float *out0, float *out1, void *stream) {
    TS_REQUIRE(a && ws && out0 && M > 0 && C > 0 && lda >= C && mode >= CR_SUM && mode <= CR_ROW, "tedspad_mgfn_col_reduce: bad arguments");
    TS_REQUIRE((mode != CR_LN && mode != CR_BN) || (x && ldx >= C && st && out1), "tedspad_mgfn_col_reduce: modes 1 and 2 need x, st and out1");
    TS_REQUIRE(mode != CR_ROW || st, "tedspad_mgfn_col_reduce: mode 4 needs the row factors");
    TS_REQUIRE(nchunks_of(M) <= 65535, "tedspad_mgfn_col_reduce: too many tokens (M=%d)", M);
    col_reduce(a, lda, x, ldx, mode == CR_SQ && !st ? nullptr : st, mode == CR_SQ && !st ? CR_SUM : mode, M, C, scale, ws, out0, out1,
               (hipStream_t)stream);
    return check_launch("tedspad_mgfn_col_reduce");
}

extern "C" int32_t tedspad_mgfn_ln_apply(const float *x, int32_t ldx, const float *stats, const float *g, const float *b, int32_t M, int32_t C,
                                         float *y, int32_t ldy, void *stream) {
    TS_REQUIRE(x && stats && g && b && y && M > 0 && C > 0 && C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ldx >= C && ldy >= C && al16(x) &&
                   al16(y) && al16(g) && al16(b),
               "tedspad_mgfn_ln_apply: bad arguments (C, ldx, ldy %% 4 == 0, 16-byte aligned)");
    const long long n = (long long)M * (C / 4);
    hipLaunchKernelGGL(ln_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, stats, g, b, M, C, y, ldy);
    return check_launch("tedspad_mgfn_ln_apply");
}

extern "C" int32_t tedspad_mgfn_ln_bwd(const float *dy, int32_t lddy, const float *x, int32_t ldx, const float *stats, const float *g,
                                       int32_t torch_ln, float eps, const float *add, int32_t ldadd, float *dx, int32_t lddx, int32_t M,
                                       int32_t C, void *stream) {
    TS_REQUIRE(dy && x && stats && g && dx && M > 0 && C > 0 && C % 4 == 0 && lddy % 4 == 0 && ldx % 4 == 0 && lddx % 4 == 0 && lddy >= C &&
                   ldx >= C && lddx >= C && al16(dy) && al16(x) && al16(dx) && al16(g) && (!add || (al16(add) && ldadd % 4 == 0 && ldadd >= C)),
               "tedspad_mgfn_ln_bwd: bad arguments (C and strides %% 4 == 0, 16-byte aligned)");
    const int per = MT_THREADS / 64;
    hipLaunchKernelGGL(ln_bwd_kernel, dim3((M + per - 1) / per), dim3(MT_THREADS), 0, (hipStream_t)stream, dy, lddy, x, ldx, stats, g, torch_ln,
                       eps, add, ldadd, dx, lddx, M, C);
    return check_launch("tedspad_mgfn_ln_bwd");
}

extern "C" int32_t tedspad_mgfn_bn_train_fwd(const float *x, int32_t ldx, int32_t M, int32_t C, const float *gamma, const float *beta, float eps,
                                             float momentum, float *ws, float *stat, float *running_mean, float *running_var, float *y,
                                             int32_t ldy, void *stream) {
    TS_REQUIRE(x && gamma && beta && ws && stat && y && M > 0 && C > 0 && C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ldx >= C && ldy >= C &&
                   al16(x) && al16(y) && al16(gamma) && al16(beta) && al16(stat) && (!running_mean == !running_var) && nchunks_of(M) <= 65535,
               "tedspad_mgfn_bn_train_fwd: bad arguments (C, ldx, ldy %% 4 == 0, 16-byte aligned)");
    hipStream_t s = (hipStream_t)stream;
    col_reduce(x, ldx, nullptr, 0, nullptr, CR_SUM, M, C, 1.f / (float)M, ws, stat, nullptr, s);               // mean
    col_reduce(x, ldx, nullptr, 0, stat, CR_SQ, M, C, 1.f / (float)M, ws, stat + C, nullptr, s);                // biased variance
    const int bt = C >= 256 ? 256 : 64;
    hipLaunchKernelGGL(bn_finish_kernel, dim3((C + bt - 1) / bt), dim3(bt), 0, s, stat, M, C, eps, momentum, running_mean, running_var);
    const long long n = (long long)M * (C / 4);
    hipLaunchKernelGGL(bn_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, ldx, stat, gamma, beta, M, C, y, ldy);
    return check_launch("tedspad_mgfn_bn_train_fwd");
}

extern "C" int32_t tedspad_mgfn_bn_train_bwd(const float *dy, int32_t lddy, const float *x, int32_t ldx, const float *stat, const float *gamma,
                                             int32_t M, int32_t C, float *ws, float *dgamma, float *dbeta, const float *add, int32_t ldadd,
                                             float *dx, int32_t lddx, void *stream) {
    TS_REQUIRE(dy && x && stat && gamma && ws && dgamma && dbeta && dx && M > 0 && C > 0 && C % 4 == 0 && lddy % 4 == 0 && ldx % 4 == 0 &&
                   lddx % 4 == 0 && lddy >= C && ldx >= C && lddx >= C && al16(dy) && al16(x) && al16(dx) && al16(stat) && al16(gamma) &&
                   al16(dgamma) && al16(dbeta) && (!add || (al16(add) && ldadd % 4 == 0 && ldadd >= C)) && nchunks_of(M) <= 65535,
               "tedspad_mgfn_bn_train_bwd: bad arguments (C and strides %% 4 == 0, 16-byte aligned)");
    hipStream_t s = (hipStream_t)stream;
    col_reduce(dy, lddy, x, ldx, stat, CR_BN, M, C, 1.f, ws, dbeta, dgamma, s);
    const long long n = (long long)M * (C / 4);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dy, lddy, x, ldx, stat, gamma, dgamma, dbeta, add,
                       ldadd, M, C, dx, lddx);
    return check_launch("tedspad_mgfn_bn_train_bwd");
}

extern "C" int32_t tedspad_mgfn_gelu(const float *x, float *y, int64_t n, void *stream) {
    TS_REQUIRE(x && y && n > 0 && n % 4 == 0 && al16(x) && al16(y), "tedspad_mgfn_gelu: bad arguments (n %% 4 == 0, 16-byte aligned)");
    hipLaunchKernelGGL(gelu_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, (long long)(n / 4));
    return check_launch("tedspad_mgfn_gelu");
}

extern "C" int32_t tedspad_mgfn_gelu_bwd(const float *x, const float *dy, float *dx, int64_t n, void *stream) {
    TS_REQUIRE(x && dy && dx && n > 0 && n % 4 == 0 && al16(x) && al16(dy) && al16(dx),
               "tedspad_mgfn_gelu_bwd: bad arguments (n %% 4 == 0, 16-byte aligned)");
    hipLaunchKernelGGL(gelu_bwd_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, dy, dx, (long long)(n / 4));
    return check_launch("tedspad_mgfn_gelu_bwd");
}

extern "C" int32_t tedspad_mgfn_transpose(const float *x, int32_t ldx, const int32_t *bounds, int32_t taps, int32_t M, int32_t C, float *out,
                                          int32_t ldo, void *stream) {
    TS_REQUIRE(x && out && M > 0 && C > 0 && ldx >= C && ldo >= M && taps >= 1 && taps % 2 == 1 && taps <= 65535 && (taps == 1 || bounds) &&
                   (C + 31) / 32 <= 65535,
               "tedspad_mgfn_transpose: bad arguments");
    hipLaunchKernelGGL(transpose_kernel, dim3((ldo + 31) / 32, (C + 31) / 32, taps), dim3(256), 0, (hipStream_t)stream, x, ldx, bounds, taps, M, C,
                       out, ldo);
    return check_launch("tedspad_mgfn_transpose");
}

extern "C" int64_t tedspad_mgfn_wgrad_ws_floats(int32_t ldk, int32_t rows, int32_t N) {
    if (ldk <= 0 || rows <= 0 || N <= 0) return 0;
    const int ks = wgrad_kslice(ldk, rows, N), ns = (ldk + ks - 1) / ks;
    return ns > 1 ? (int64_t)ns * rows * N : 0;
}

extern "C" int32_t tedspad_mgfn_wgrad(const float *at, const float *dyt, int32_t ldk, int32_t rows, int32_t N, float *ws, float *dwt,
                                      void *stream) {
    TS_REQUIRE(at && dyt && dwt && ldk > 0 && rows > 0 && N > 0 && ldk % 16 == 0 && N % 64 == 0 && al16(at) && al16(dyt) && al16(dwt),
               "tedspad_mgfn_wgrad: bad arguments (ldk %% 16 == 0, N %% 64 == 0, 16-byte aligned; ldk=%d rows=%d N=%d)", ldk, rows, N);
    const int ks = wgrad_kslice(ldk, rows, N), ns = (ldk + ks - 1) / ks;
    TS_REQUIRE(ns == 1 || (ws && al16(ws)), "tedspad_mgfn_wgrad: needs the workspace of tedspad_mgfn_wgrad_ws_floats");
    TS_REQUIRE((rows + 63) / 64 <= 65535 && ns <= 65535, "tedspad_mgfn_wgrad: too many rows (%d)", rows);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(wgrad_kernel, dim3(N / 64, (rows + 63) / 64, ns), dim3(64), 0, s, at, dyt, ldk, rows, N, ks, ns > 1 ? ws : dwt);
    if (ns > 1) {
        const long long n4 = (long long)rows * N / 4;
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, ws, ns, n4, dwt);
    }
    return check_launch("tedspad_mgfn_wgrad");
}

extern "C" int32_t tedspad_mgfn_attention_bwd(const float *qkv, int32_t ldqkv, const float *o, int32_t ldo, const float *d_o, int32_t lddo,
                                              const int32_t *seq_off, int32_t nseq, int32_t tmax, int32_t heads, float *lse, float *dqkv,
                                              int32_t lddqkv, void *stream) {
    TS_REQUIRE(qkv && o && d_o && seq_off && lse && dqkv && nseq > 0 && tmax > 0 && heads > 0 && heads <= 65535 && (tmax + 31) / 32 <= 65535,
               "tedspad_mgfn_attention_bwd: bad arguments");
    TS_REQUIRE(ldqkv % 4 == 0 && ldqkv >= 3 * heads * AT_D && lddqkv >= 3 * heads * AT_D && ldo % 4 == 0 && lddo % 4 == 0 &&
                   ldo >= heads * AT_D && lddo >= heads * AT_D && al16(qkv) && al16(o) && al16(d_o),
               "tedspad_mgfn_attention_bwd: rows must hold q | k | v (3 x heads x %d) and o (heads x %d), 16-byte aligned", AT_D, AT_D);
    const dim3 grid(nseq, (tmax + 31) / 32, heads);
    hipLaunchKernelGGL(attn_bwd_q_kernel, grid, dim3(64), 0, (hipStream_t)stream, qkv, ldqkv, o, ldo, d_o, lddo, seq_off, heads, dqkv, lddqkv, lse);
    hipLaunchKernelGGL(attn_bwd_kv_kernel, grid, dim3(64), 0, (hipStream_t)stream, qkv, ldqkv, d_o, lddo, seq_off, heads, lse, dqkv, lddqkv);
    return check_launch("tedspad_mgfn_attention_bwd");
}

extern "C" int32_t tedspad_mgfn_relpos_bwd(const float *dout, int32_t lddo, const float *v, int32_t ldv, const int32_t *bounds, int32_t M,
                                           int32_t C, int32_t heads, const float *w, float *ws, float *dv, int32_t lddv, float *dw, float *db,
                                           void *stream) {
    TS_REQUIRE(dout && v && bounds && w && ws && dv && dw && db && M > 0 && heads > 0 && C > 0 && C % 4 == 0 && C % heads == 0 && lddo % 4 == 0 &&
                   lddv % 4 == 0 && lddo >= C && ldv >= C && lddv >= C && al16(dout) && al16(dv) && dv != dout && nchunks_of(M) <= 65535,
               "tedspad_mgfn_relpos_bwd: bad arguments (C, lddo, lddv %% 4 == 0, 16-byte aligned, not in place)");
    hipStream_t s = (hipStream_t)stream;
    const long long n = (long long)M * (C / 4);
    hipLaunchKernelGGL(relpos_bwd_dv_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dout, lddo, bounds, M, C, heads, w, dv, lddv);
    const int bt = C >= 256 ? 256 : 64, nch = nchunks_of(M);
    hipLaunchKernelGGL(relpos_bwd_partial_kernel, dim3((C + bt - 1) / bt, nch), dim3(bt), 0, s, dout, lddo, v, ldv, bounds, M, C, ws);
    hipLaunchKernelGGL(relpos_bwd_final_kernel, dim3(heads * 6), dim3(256), 0, s, ws, nch, C, heads, dw, db);
    return check_launch("tedspad_mgfn_relpos_bwd");
}

extern "C" int32_t tedspad_mgfn_head_bwd(const float *score, const float *dscore, const float *fc_w, int32_t M, int32_t C, float *dh, float *dz,
                                         void *stream) {
    TS_REQUIRE(score && dscore && fc_w && dh && dz && M > 0 && C > 0 && C % 4 == 0 && al16(fc_w) && al16(dh),
               "tedspad_mgfn_head_bwd: bad arguments (C %% 4 == 0, 16-byte aligned)");
    const int per = MT_THREADS / 64;
    hipLaunchKernelGGL(head_bwd_kernel, dim3((M + per - 1) / per), dim3(MT_THREADS), 0, (hipStream_t)stream, score, dscore, fc_w, M, C, dh, dz);
    return check_launch("tedspad_mgfn_head_bwd");
}

extern "C" int32_t tedspad_mgfn_msnsd(const float *h, const float *crop_scores, const float *crop_mags, const float *masks, const float *labels,
                                      int32_t n, int32_t ncrops, int32_t T, int32_t C, int32_t k, int32_t *idx, float *vid_score, float *l1,
                                      float *losses, float *dl1, float *dcs, float *dvid, float *dscore, float *dh, void *stream) {
    TS_REQUIRE(h && crop_scores && crop_mags && masks && labels && idx && vid_score && l1 && losses && dl1 && dcs && dvid && dscore && dh,
               "tedspad_mgfn_msnsd: null argument");
    TS_REQUIRE(n >= 2 && ncrops >= 1 && (n * ncrops) % 2 == 0 && k >= 1 && k <= MS_MAXK && T >= k && C > 0 && C % 4 == 0 && al16(h) && al16(dh) &&
                   (long long)2 * n * ncrops * T < (1ll << 31),
               "tedspad_mgfn_msnsd: needs n >= 2, n * ncrops even, 1 <= k <= %d, T >= k, C %% 4 == 0 (n=%d ncrops=%d T=%d k=%d C=%d)", MS_MAXK,
               n, ncrops, T, k, C);
    hipStream_t s = (hipStream_t)stream;
    const int per = MT_THREADS / 64;
    hipLaunchKernelGGL(msnsd_select_kernel, dim3((2 * n + 63) / 64), dim3(64), 0, s, crop_mags, crop_scores, masks, n, T, k, idx, vid_score);
    const int nw = 2 * n * ncrops * k;
    hipLaunchKernelGGL(msnsd_l1_kernel, dim3((nw + per - 1) / per), dim3(MT_THREADS), 0, s, h, idx, n, ncrops, T, C, k, l1);
    hipLaunchKernelGGL(msnsd_cost_kernel, dim3(1), dim3(256), 0, s, vid_score, labels, l1, crop_scores, idx, n, ncrops, T, k, losses, dl1, dcs,
                       dvid);
    const int M = 2 * n * ncrops * T;
    hipLaunchKernelGGL(msnsd_scatter_kernel, dim3((M + per - 1) / per), dim3(MT_THREADS), 0, s, h, idx, dl1, dcs, n, ncrops, T, C, k, dscore, dh);
    return check_launch("tedspad_mgfn_msnsd");
}
