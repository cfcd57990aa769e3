// MGFN inference for gfx950, all fp32 (anomaly_detection_mgfn/models/mgfn.py, utils/utils.py:101-180 under model.eval()).
//
// Layout: token-major (token, channel) rows over a RAGGED batch. Crop sequences are concatenated; `bounds[2m], bounds[2m+1]` are the
// first and one-past-last token of token m's sequence, `seq_off` (nseq + 1) the same per sequence. Temporal taps never cross a sequence
// end (the reference's zero padding) and attention never mixes sequences.
//
//   mgfn_ln_stats   per-token mean and 1/(std + eps) (MGFN LayerNorm, Q-M1) or 1/sqrt(var + eps) (nn.LayerNorm)
//   mgfn_gemm       Y = A W^T + bias [-> exact GELU] [+ residual] on the f32-input MFMA (32x32x2f32). A is x itself (1x1 conv), its
//                   k-tap window (k = 3 temporal conv, K = taps * cin) or its per-token normalised rows (LayerNorm prologue; the
//                   LayerNorm's g / b are folded into W / bias on the host)
//   mgfn_attention  GLANCE softmax attention per (sequence, head, 32 queries), d = 64, online softmax, MFMA for QK^T and PV
//   mgfn_relpos     FOCUS rel_pos: depthwise 5-tap temporal conv, channel ch uses the filter of head ch % heads (Q-M2)
//   mgfn_head       nn.LayerNorm -> fc -> sigmoid, plus the L2 norm of the LayerNorm output (MSNSD's magnitude)
//   mgfn_crop_mean  mean over the crops of one video, per segment
//
// Every output element is summed in a fixed order that depends only on its own sequence: no float atomics, no split that depends on the
// batch, so a video's results are bit-identical alone or inside any ragged batch.
#include "common.h"

namespace tedspad {
namespace {

__device__ __forceinline__ float wsum64(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- per-token LayerNorm statistics (one wave per token) ----------------------------------------------------------------------------
constexpr int LN_THREADS = 256;

__global__ __launch_bounds__(LN_THREADS) void ln_stats_kernel(const float *x, int ldx, int M, int C, float eps, int torch_ln, float *stats) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * (LN_THREADS / 64) + (threadIdx.x >> 6);
    if (m >= M) return;
    const float *row = x + (size_t)m * ldx;
    float s = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(row + c);
        s += (v[0] + v[1]) + (v[2] + v[3]);
    }
    const float mean = wsum64(s) / (float)C;
    float q = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(row + c) - mean;
        q += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
    const float var = wsum64(q) / (float)C;               // biased, as torch.var(unbiased=False) and nn.LayerNorm
    if (lane == 0) {
        stats[2 * m] = mean;
        stats[2 * m + 1] = torch_ln ? 1.f / sqrtf(var + eps) : 1.f / (sqrtf(var) + eps);
    }
}

// ---- ragged-token GEMM on the f32 MFMA -----------------------------------------------------------------------------------------------
// Workgroup: 4 waves stacked along M, each a 64 x 64 output tile (2 x 2 MFMA tiles of 32 x 32). Operands go straight from global memory
// to VGPRs: lane (i, h) of a 32-row block loads 8 consecutive K values of its row (two float4) per 16-wide K chunk and feeds element s to
// k-step s, so k-step s sums k = kc + s (half 0) and kc + 8 + s (half 1) -- a bijection over the chunk, the same for A and W. The next
// chunk's operands are loaded before the current chunk's 32 MFMAs.
constexpr int GM_WAVES = 4;
constexpr int GM_WM = 64, GM_WN = 64, GM_KC = 16;

struct GemmArgs {
    const float *x;
    const int *bounds;
    const float *stats;
    const float *w;
    const float *bias;
    const float *res;
    float *y;
    int ldx, taps, cin, K, ldres, ldy, M, N, gelu;
};

template <bool LN>
__global__ __launch_bounds__(64 * GM_WAVES) void gemm_kernel(GemmArgs g) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 31, hf = lane >> 5;
    const int n0 = blockIdx.x * GM_WN;
    const int m0 = (blockIdx.y * GM_WAVES + wave) * GM_WM;
    if (m0 >= g.M) return;
    int row[2], lo[2], hi[2];
    float mu[2] = {0.f, 0.f}, rs[2] = {1.f, 1.f};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        row[r] = m0 + 32 * r + i;
        const bool ok = row[r] < g.M;
        const int rr = ok ? row[r] : g.M - 1;
        lo[r] = ok ? (g.bounds ? g.bounds[2 * rr] : rr) : 1;     // a row past M has an empty window: it loads zeros
        hi[r] = ok ? (g.bounds ? g.bounds[2 * rr + 1] : rr + 1) : 0;
        if (LN) {
            mu[r] = g.stats[2 * rr];
            rs[r] = g.stats[2 * rr + 1];
        }
    }
    const float *wrow[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) wrow[c] = g.w + (size_t)(n0 + 32 * c + i) * g.K + 8 * hf;
    const int half_taps = g.taps >> 1, chunks_per_tap = g.cin / GM_KC, nchunks = g.taps * chunks_per_tap;

    auto load = [&](int kk, f32x4(&a)[2][2], f32x4(&b)[2][2]) {
        const int t = kk / chunks_per_tap, c = (kk - t * chunks_per_tap) * GM_KC + 8 * hf;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int src = row[r] + t - half_taps;
            if (src >= lo[r] && src < hi[r]) {
                const float *p = g.x + (size_t)src * g.ldx + c;
                a[r][0] = *reinterpret_cast<const f32x4 *>(p);
                a[r][1] = *reinterpret_cast<const f32x4 *>(p + 4);
                if (LN) {
                    a[r][0] = (a[r][0] - mu[r]) * rs[r];
                    a[r][1] = (a[r][1] - mu[r]) * rs[r];
                }
            } else {
                a[r][0] = f32x4{0.f, 0.f, 0.f, 0.f};
                a[r][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        const int kw = kk * GM_KC;
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            b[cc][0] = *reinterpret_cast<const f32x4 *>(wrow[cc] + kw);
            b[cc][1] = *reinterpret_cast<const f32x4 *>(wrow[cc] + kw + 4);
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[r][c][e] = 0.f;
    f32x4 a[2][2], b[2][2], an[2][2], bn[2][2];
    load(0, a, b);
    for (int kk = 0; kk < nchunks; ++kk) {
        if (kk + 1 < nchunks) load(kk + 1, an, bn);
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c)
                    acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r][s >> 2][s & 3], b[c][s >> 2][s & 3], acc[r][c], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                a[r][q] = an[r][q];
                b[r][q] = bn[r][q];
            }
    }
    // ---- epilogue: C/D map col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5) ----
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int col = n0 + 32 * c + i;
        const float bv = g.bias ? g.bias[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + 32 * r + (e & 3) + 8 * (e >> 2) + 4 * hf;
                if (m >= g.M) continue;
                float v = acc[r][c][e] + bv;
                if (g.gelu) v = 0.5f * v * (1.f + erff(v * 0.70710678118654752440f));   // nn.GELU(): exact erf form (Q-M5)
                if (g.res) v += g.res[(size_t)m * g.ldres + col];
                g.y[(size_t)m * g.ldy + col] = v;
            }
    }
}

// ---- GLANCE attention: one wave per (32 queries, sequence, head) --------------------------------------------------------------------
// S = (q / 8) K^T over a 32-key block: A = Q (lane (i, h) holds q[i][32h + s] for k-step s), B = K^T (lane (j, h) holds k[j][32h + s]).
// S comes out with the key on the lane and the query rows in registers; the running max / sum of every row are kept in that layout, which
// is also the layout of the output accumulator, so the rescale needs no lane movement. P goes through LDS once to become the A operand
// of P V (k-step s of half h is key 16h + s).
constexpr int AT_D = 64;

__global__ __launch_bounds__(64) void attention_kernel(const float *qkv, int ldqkv, const int *seq_off, int heads, float *out, int ldo) {
    __shared__ float P[32][33];
    const int lane = threadIdx.x, i = lane & 31, hf = lane >> 5;
    const int seq = blockIdx.x, head = blockIdx.z;           // sequences on x: no 65535 limit on their number
    const int base = seq_off[seq], T = seq_off[seq + 1] - base;
    const int q0 = blockIdx.y * 32;
    if (q0 >= T) return;
    const int inner = heads * AT_D;
    const float *Q = qkv + (size_t)base * ldqkv + head * AT_D;
    const float *Kp = Q + inner, *Vp = Q + 2 * inner;

    float q[32];
    {
        const int qi = min(q0 + i, T - 1);                       // query rows past the end compute a copy of the last row; never stored
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const f32x4 t = *reinterpret_cast<const f32x4 *>(Q + (size_t)qi * ldqkv + 32 * hf + 4 * v) * 0.125f;   // q * dim_head^-0.5 (exact)
            q[4 * v] = t[0];
            q[4 * v + 1] = t[1];
            q[4 * v + 2] = t[2];
            q[4 * v + 3] = t[3];
        }
    }
    f32x16 o0, o1;
    float mrow[16], lrow[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        o0[e] = 0.f;
        o1[e] = 0.f;
        mrow[e] = -INFINITY;
        lrow[e] = 0.f;
    }
    for (int kb = 0; kb < T; kb += 32) {
        const bool kval = kb + i < T;
        const int kj = kval ? kb + i : T - 1;
        f32x16 s;
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const f32x4 kk = *reinterpret_cast<const f32x4 *>(Kp + (size_t)kj * ldqkv + 32 * hf + 4 * v);
#pragma unroll
            for (int u = 0; u < 4; ++u) s = __builtin_amdgcn_mfma_f32_32x32x2f32(q[4 * v + u], kk[u], s, 0, 0, 0);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float sv = kval ? s[e] : -INFINITY;
            float mx = sv;
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
            const float mnew = fmaxf(mrow[e], mx);                // finite: key kb is always valid
            const float alpha = expf(mrow[e] - mnew);
            const float p = expf(sv - mnew);
            float ps = p;
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) ps += __shfl_xor(ps, o, 64);
            lrow[e] = lrow[e] * alpha + ps;
            mrow[e] = mnew;
            o0[e] *= alpha;
            o1[e] *= alpha;
            P[(e & 3) + 8 * (e >> 2) + 4 * hf][i] = p;
        }
        __syncthreads();
#pragma unroll
        for (int st = 0; st < 16; ++st) {
            const int key = kb + 16 * hf + st;
            const bool vv = key < T;
            const float *vr = Vp + (size_t)(vv ? key : T - 1) * ldqkv;
            const float pa = P[i][16 * hf + st];
            const float v0 = vv ? vr[i] : 0.f, v1 = vv ? vr[32 + i] : 0.f;
            o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(pa, v0, o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(pa, v1, o1, 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int qi = q0 + (e & 3) + 8 * (e >> 2) + 4 * hf;
        if (qi >= T) continue;
        float *orow = out + (size_t)(base + qi) * ldo + head * AT_D;
        orow[i] = o0[e] / lrow[e];
        orow[32 + i] = o1[e] / lrow[e];
    }
}

// ---- FOCUS rel_pos: depthwise 5-tap temporal conv with interleaved heads (one thread per 4 channels of a token) -----------------------
__global__ void relpos_kernel(const float *v, int ldv, const int *bounds, int M, int C, int heads, const float *w, const float *b, float *out,
                              int ldo) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c4 = C / 4;
    if (idx >= (long long)M * c4) return;
    const int m = (int)(idx / c4), c = (int)(idx - (long long)m * c4) * 4;
    const int lo = bounds[2 * m], hi = bounds[2 * m + 1];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 5; ++t) {                            // Conv1d is a correlation: tap t reads token m + t - 2
        const int src = m + t - 2;
        if (src < lo || src >= hi) continue;
        const f32x4 x = *reinterpret_cast<const f32x4 *>(v + (size_t)src * ldv + c);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] += w[((c + u) % heads) * 5 + t] * x[u];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] += b[(c + u) % heads];
    *reinterpret_cast<f32x4 *>(out + (size_t)m * ldo + c) = acc;
}

// ---- head: nn.LayerNorm(C) -> fc(C -> 1) -> sigmoid, and ||LayerNorm output||_2 (one wave per token) ---------------------------------
__global__ __launch_bounds__(LN_THREADS) void head_kernel(const float *x, int ldx, int M, int C, const float *lw, const float *lb,
                                                          const float *fw, float fb, float eps, float *h, float *logit, float *score,
                                                          float *mag) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * (LN_THREADS / 64) + (threadIdx.x >> 6);
    if (m >= M) return;
    const float *row = x + (size_t)m * ldx;
    float s = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(row + c);
        s += (v[0] + v[1]) + (v[2] + v[3]);
    }
    const float mean = wsum64(s) / (float)C;
    float q = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(row + c) - mean;
        q += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
    const float rs = 1.f / sqrtf(wsum64(q) / (float)C + eps);
    float z = 0.f, n2 = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        const f32x4 v = (*reinterpret_cast<const f32x4 *>(row + c) - mean) * rs * *reinterpret_cast<const f32x4 *>(lw + c) +
                        *reinterpret_cast<const f32x4 *>(lb + c);
        if (h) *reinterpret_cast<f32x4 *>(h + (size_t)m * C + c) = v;
        const f32x4 wv = *reinterpret_cast<const f32x4 *>(fw + c);
        z += (v[0] * wv[0] + v[1] * wv[1]) + (v[2] * wv[2] + v[3] * wv[3]);
        n2 += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
    z = wsum64(z) + fb;
    n2 = wsum64(n2);
    if (lane == 0) {
        logit[m] = z;
        score[m] = 1.f / (1.f + expf(-z));
        mag[m] = sqrtf(n2);
    }
}

// ---- crop mean: out[seg_off[v] + t] = mean_c in[ncrops seg_off[v] + c T_v + t] -------------------------------------------------------
__global__ void crop_mean_kernel(const float *a, float *a_out, const float *b, float *b_out, const int *seg_off, int ncrops) {
    const int v = blockIdx.x, t = blockIdx.y * blockDim.x + threadIdx.x;
    const int s0 = seg_off[v], T = seg_off[v + 1] - s0;
    if (t >= T) return;
    const size_t base = (size_t)ncrops * s0 + t;
    float sa = 0.f, sb = 0.f;
    for (int c = 0; c < ncrops; ++c) {
        sa += a[base + (size_t)c * T];
        if (b) sb += b[base + (size_t)c * T];
    }
    a_out[s0 + t] = sa / (float)ncrops;
    if (b) b_out[s0 + t] = sb / (float)ncrops;
}

inline bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace tedspad

using namespace tedspad;

extern "C" int32_t tedspad_mgfn_ln_stats(const float *x, int32_t ldx, int32_t M, int32_t C, float eps, int32_t torch_ln, float *stats,
                                         void *stream) {
    TS_REQUIRE(x && stats && M > 0 && C > 0 && C % 4 == 0 && ldx % 4 == 0 && ldx >= C && al16(x),
               "tedspad_mgfn_ln_stats: bad arguments (M=%d C=%d ldx=%d; C, ldx %% 4 == 0, x 16-byte aligned)", M, C, ldx);
    const int per = LN_THREADS / 64;
    hipLaunchKernelGGL(ln_stats_kernel, dim3((M + per - 1) / per), dim3(LN_THREADS), 0, (hipStream_t)stream, x, ldx, M, C, eps, torch_ln,
                       stats);
    return check_launch("tedspad_mgfn_ln_stats");
}

extern "C" int32_t tedspad_mgfn_gemm(const float *x, int32_t ldx, const int32_t *bounds, int32_t taps, int32_t cin, const float *stats,
                                     const float *w, const float *bias, int32_t gelu, const float *res, int32_t ldres, float *y, int32_t ldy,
                                     int32_t M, int32_t N, void *stream) {
    TS_REQUIRE(x && w && y && M > 0 && N > 0 && cin > 0 && taps >= 1 && taps % 2 == 1, "tedspad_mgfn_gemm: bad arguments");
    TS_REQUIRE(N % GM_WN == 0 && cin % GM_KC == 0, "tedspad_mgfn_gemm: needs N %% %d == 0 and cin %% %d == 0 (N=%d cin=%d)", GM_WN, GM_KC, N,
               cin);
    TS_REQUIRE(ldx % 4 == 0 && ldx >= cin && ldy >= N && al16(x) && al16(w), "tedspad_mgfn_gemm: x / w need 16-byte aligned rows");
    TS_REQUIRE(taps == 1 || bounds, "tedspad_mgfn_gemm: a temporal conv (taps > 1) needs the sequence bounds");
    TS_REQUIRE(!stats || taps == 1, "tedspad_mgfn_gemm: the LayerNorm prologue is for 1x1 convs only");
    TS_REQUIRE(!res || ldres >= N, "tedspad_mgfn_gemm: bad residual stride");
    TS_REQUIRE(y != x, "tedspad_mgfn_gemm: y must not alias x (other workgroups still read it)");
    GemmArgs g{x, bounds, stats, w, bias, res, y, ldx, taps, cin, taps * cin, ldres, ldy, M, N, gelu};
    const dim3 grid(N / GM_WN, (M + GM_WAVES * GM_WM - 1) / (GM_WAVES * GM_WM));
    TS_REQUIRE(grid.y <= 65535, "tedspad_mgfn_gemm: at most %d tokens per launch (M=%d)", 65535 * GM_WAVES * GM_WM, M);
    if (stats)
        hipLaunchKernelGGL(gemm_kernel<true>, grid, dim3(64 * GM_WAVES), 0, (hipStream_t)stream, g);
    else
        hipLaunchKernelGGL(gemm_kernel<false>, grid, dim3(64 * GM_WAVES), 0, (hipStream_t)stream, g);
    return check_launch("tedspad_mgfn_gemm");
}

extern "C" int32_t tedspad_mgfn_attention(const float *qkv, int32_t ldqkv, const int32_t *seq_off, int32_t nseq, int32_t tmax, int32_t heads,
                                          float *out, int32_t ldo, void *stream) {
    TS_REQUIRE(qkv && seq_off && out && nseq > 0 && tmax > 0 && heads > 0 && heads <= 65535 && (tmax + 31) / 32 <= 65535,
               "tedspad_mgfn_attention: bad arguments (heads and tmax / 32 at most 65535: the grid's y and z)");
    TS_REQUIRE(ldqkv % 4 == 0 && ldqkv >= 3 * heads * AT_D && ldo >= heads * AT_D && al16(qkv),
               "tedspad_mgfn_attention: qkv rows must hold q | k | v (3 x heads x %d), 16-byte aligned", AT_D);
    hipLaunchKernelGGL(attention_kernel, dim3(nseq, (tmax + 31) / 32, heads), dim3(64), 0, (hipStream_t)stream, qkv, ldqkv, seq_off, heads,
                       out, ldo);
    return check_launch("tedspad_mgfn_attention");
}

extern "C" int32_t tedspad_mgfn_relpos(const float *v, int32_t ldv, const int32_t *bounds, int32_t M, int32_t C, int32_t heads, const float *w,
                                       const float *b, float *out, int32_t ldo, void *stream) {
    TS_REQUIRE(v && bounds && w && b && out && M > 0 && heads > 0 && C > 0 && C % 4 == 0 && ldv % 4 == 0 && ldo % 4 == 0 && ldv >= C &&
                   ldo >= C && al16(v) && al16(out) && v != out,
               "tedspad_mgfn_relpos: bad arguments (C, ldv, ldo %% 4 == 0, ldv, ldo >= C, 16-byte aligned, not in place)");
    const long long n = (long long)M * (C / 4);
    hipLaunchKernelGGL(relpos_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, v, ldv, bounds, M, C, heads, w, b,
                       out, ldo);
    return check_launch("tedspad_mgfn_relpos");
}

extern "C" int32_t tedspad_mgfn_head(const float *x, int32_t ldx, int32_t M, int32_t C, const float *ln_w, const float *ln_b, const float *fc_w,
                                     float fc_b, float eps, float *h, float *logit, float *score, float *mag, void *stream) {
    TS_REQUIRE(x && ln_w && ln_b && fc_w && logit && score && mag && M > 0 && C > 0 && C % 4 == 0 && ldx % 4 == 0 && ldx >= C && al16(x) &&
                   al16(ln_w) && al16(ln_b) && al16(fc_w) && (!h || al16(h)),
               "tedspad_mgfn_head: bad arguments (C, ldx %% 4 == 0, ldx >= C, 16-byte aligned)");
    const int per = LN_THREADS / 64;
    hipLaunchKernelGGL(head_kernel, dim3((M + per - 1) / per), dim3(LN_THREADS), 0, (hipStream_t)stream, x, ldx, M, C, ln_w, ln_b, fc_w, fc_b,
                       eps, h, logit, score, mag);
    return check_launch("tedspad_mgfn_head");
}

extern "C" int32_t tedspad_mgfn_crop_mean(const float *a, float *a_out, const float *b, float *b_out, const int32_t *seg_off, int32_t nvid,
                                          int32_t tmax, int32_t ncrops, void *stream) {
    TS_REQUIRE(a && a_out && seg_off && nvid > 0 && tmax > 0 && ncrops > 0 && (!b || b_out), "tedspad_mgfn_crop_mean: bad arguments");
    hipLaunchKernelGGL(crop_mean_kernel, dim3(nvid, (tmax + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, a_out, b, b_out, seg_off, ncrops);
    return check_launch("tedspad_mgfn_crop_mean");
}
