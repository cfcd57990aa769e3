// The attention core of I3Res50's NonLocalBlock (large_i3d.py:112-119) for gfx950, inference:
//
//   T[q, :] = sum_j softmax_j(scale * theta[q, :] . phi[j, :]) * g[j, :]        per batch item, q queries x k keys x d channels
//
// fused: the q x k score matrix is never written. A workgroup of four waves owns 32 queries of one item and walks the keys in tiles of 64
// with a running max / sum (online softmax). Per tile:
//   S    wave w takes the tile's keys 16w .. 16w+15 against all 32 queries over the full d: S^T = phi . theta^T on the 16x16x32 MFMA (keys are the
//        rows, so a lane ends with four keys of ONE query and the row statistics need no LDS beyond the four waves' maxima). phi rows go from
//        global memory straight into the A operand; theta (32 x d) is resident in LDS.
//   P    exp2 of the scaled logits minus the running max, rounded to the storage type into a [32 queries][64 keys] LDS image; every wave keeps the
//        sum of ITS keys' (unrounded) p and the four are added at the end.
//   PV   wave w owns channels w d/4 .. (w+1) d/4 of the output (d is split across the waves: a 32-row fp32 accumulator over all of d = 512
//        would be 256 registers): O^T[c][q] += g^T[c][key] P^T[key][q] on the 32x32x16 MFMA. g is channels-last, the MFMA sums over keys: the wave
//        stages its [32 keys][d/4] slice, one half of the tile after the other, in a private LDS region and reads it back key-major with
//        ds_read_b64_tr_b16. Sixteen-key steps that lie wholly past k are skipped (their P is zero).
// The output leaves through the same private region, so that it is stored as whole 16-byte pieces of contiguous rows. LDS (40 KB at d = 256, 72 KB at
// d = 512) and registers (<= 256) leave room for two workgroups per CU: with k = 98 keys a workgroup lives for two tiles, and its prologue
// (theta -> LDS) and epilogue run under the other's MFMAs.
// Keys past k are clamped for the loads, get logit -inf (p = 0) and a zero g row; query rows past q compute a copy of the last row and are
// not stored. No row of another batch item is ever addressed.
#include <math.h>

#include "common.h"

namespace tedspad {
namespace {

struct NlArgs {
    const uint16_t *theta, *phi, *g;
    uint16_t *out;
    int ldt, ldp, ldg, ldo;
    int q, k, qtiles;
    float c2;          // scale * log2(e): the softmax runs in base 2
};

constexpr int NL_QT = 32;          // queries per workgroup
constexpr int NL_KT = 64;          // keys per tile (16 per wave in the S phase)
constexpr int NL_PST = NL_KT * 2 + 16;   // bytes per row of the P image

template <int D>
struct NlGeo {
    static constexpr int CW = D / 4;             // channels of the output a wave owns
    static constexpr int QST = D * 2 + 16;       // bytes per row of the theta image
    static constexpr int VST = CW * 2 + 16;      // bytes per row of a wave's g image
    static constexpr int Q_BYTES = NL_QT * QST, V_BYTES = (NL_KT / 2) * VST, P_BYTES = NL_QT * NL_PST, M_BYTES = 4 * NL_QT * 4;
    static constexpr int LDS = Q_BYTES + 4 * V_BYTES + P_BYTES + M_BYTES;
};

typedef short short4v __attribute__((ext_vector_type(4)));

template <typename T, int D>
__global__ __launch_bounds__(256, 2) void nl_attention_kernel(const NlArgs a) {
    using G = NlGeo<D>;
    constexpr int CW = G::CW, NCB = CW / 32, KS = D / 32, NV = CW / 8, NVH = NV / 2;     // NV: 16-byte chunks per row of the wave's g slice; NVH: chunks per lane per 32 keys
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned char *Qs = smem, *Vs = smem + G::Q_BYTES + wave * G::V_BYTES, *Ps = smem + G::Q_BYTES + 4 * G::V_BYTES;
    float *Ms = reinterpret_cast<float *>(Ps + G::P_BYTES);
    const int item = blockIdx.x / a.qtiles, q0 = (blockIdx.x - item * a.qtiles) * NL_QT;
    const uint16_t *theta = a.theta + (size_t)item * a.q * a.ldt;
    const uint16_t *phi = a.phi + (size_t)item * a.k * a.ldp;
    const uint16_t *gv = a.g + (size_t)item * a.k * a.ldg + wave * CW;

    for (int idx = tid; idx < NL_QT * (D / 8); idx += 256) {              // theta tile -> LDS
        const int row = idx / (D / 8), ch = idx - row * (D / 8);
        const int qi = min(q0 + row, a.q - 1);
        *reinterpret_cast<uint4 *>(Qs + row * G::QST + ch * 16) = *reinterpret_cast<const uint4 *>(theta + (size_t)qi * a.ldt + ch * 8);
    }

    const int kq = lane & 15, kg = lane >> 4;              // S phase: operand row / column, k group
    const int r = lane & 31, h = lane >> 5;                // PV phase: query column, k half
    const int vrow = lane / NV, vch = lane - vrow * NV;    // g staging: this lane's chunk of the first 64 / NV rows
    uint4 kf[KS], vf[NVH];
    auto load_k = [&](int kb) {
        const uint16_t *row = phi + (size_t)min(kb + 16 * wave + kq, a.k - 1) * a.ldp + 8 * kg;
#pragma unroll
        for (int s = 0; s < KS; ++s) kf[s] = *reinterpret_cast<const uint4 *>(row + 32 * s);
    };
    auto load_v = [&](int kb) {
#pragma unroll
        for (int i = 0; i < NVH; ++i) {
            const int key = kb + i * (64 / NV) + vrow;
            const uint4 v = *reinterpret_cast<const uint4 *>(gv + (size_t)min(key, a.k - 1) * a.ldg + vch * 8);
            vf[i] = key < a.k ? v : make_uint4(0, 0, 0, 0);
        }
    };
    auto store_v = [&]() {
        asm volatile("" ::: "memory");         // after the reads of the half before it (LDS operations of a wave complete in order)
#pragma unroll
        for (int i = 0; i < NVH; ++i) *reinterpret_cast<uint4 *>(Vs + (i * (64 / NV) + vrow) * G::VST + vch * 16) = vf[i];
    };
    auto tr = [&](const unsigned char *p) -> uint2 {
        return __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v *)(p)));
    };

    f32x16 oacc[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int e = 0; e < 16; ++e) oacc[cb][e] = 0.f;
    float mrow[2] = {-INFINITY, -INFINITY}, lrow[2] = {0.f, 0.f};

    load_k(0);
    __syncthreads();
    for (int kb = 0; kb < a.k; kb += NL_KT) {
        load_v(kb);
        // ---- S^T = phi . theta^T: lane (kq, kg) ends with keys 4 kg + e of query 16 qh + kq ----
        f32x4 sa[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        if (kb + 16 * wave < a.k) {              // a wave whose sixteen keys all lie past k has nothing to multiply
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const uint4 b0 = *reinterpret_cast<const uint4 *>(Qs + kq * G::QST + (32 * s + 8 * kg) * 2);
                const uint4 b1 = *reinterpret_cast<const uint4 *>(Qs + (16 + kq) * G::QST + (32 * s + 8 * kg) * 2);
                sa[0] = T::mfma16(kf[s], b0, sa[0]);
                sa[1] = T::mfma16(kf[s], b1, sa[1]);
            }
        }
        store_v();
        const bool second = kb + NL_KT / 2 < a.k;
        if (second) load_v(kb + NL_KT / 2);
        if (kb + NL_KT < a.k) load_k(kb + NL_KT);
        float sv[2][4];
#pragma unroll
        for (int qh = 0; qh < 2; ++qh) {
            float mx = -INFINITY;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sv[qh][e] = kb + 16 * wave + 4 * kg + e < a.k ? sa[qh][e] * a.c2 : -INFINITY;
                mx = fmaxf(mx, sv[qh][e]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            if (kg == 0) Ms[wave * NL_QT + 16 * qh + kq] = mx;
        }
        __syncthreads();
        // ---- running max / sum, P ----
        float alpha[2];
#pragma unroll
        for (int qh = 0; qh < 2; ++qh) {
            const int qc = 16 * qh + kq;
            const float mx = fmaxf(fmaxf(Ms[qc], Ms[NL_QT + qc]), fmaxf(Ms[2 * NL_QT + qc], Ms[3 * NL_QT + qc]));    // finite: the tile's first key is valid
            const float mnew = fmaxf(mrow[qh], mx);
            alpha[qh] = __builtin_amdgcn_exp2f(mrow[qh] - mnew);
            mrow[qh] = mnew;
            float p[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) p[e] = __builtin_amdgcn_exp2f(sv[qh][e] - mnew);
            lrow[qh] = lrow[qh] * alpha[qh] + ((p[0] + p[1]) + (p[2] + p[3]));
            const uint32_t lo = (uint32_t)T::from_f32(p[0]) | ((uint32_t)T::from_f32(p[1]) << 16);
            const uint32_t hi = (uint32_t)T::from_f32(p[2]) | ((uint32_t)T::from_f32(p[3]) << 16);
            *reinterpret_cast<uint2 *>(Ps + qc * NL_PST + (16 * wave + 4 * kg) * 2) = make_uint2(lo, hi);
        }
        {
            const float ao = (kg & 1) ? alpha[1] : alpha[0];       // the PV column r = 16 (kg & 1) + kq: this lane holds that query's factor
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                for (int e = 0; e < 16; ++e) oacc[cb][e] *= ao;
        }
        __syncthreads();
        // ---- O^T += g^T . P^T: lane (r, h) ends with channels 32 cb + (e & 3) + 8 (e >> 2) + 4 h of query r ----
        auto pv = [&](int s) {
            const uint4 pb = *reinterpret_cast<const uint4 *>(Ps + r * NL_PST + (16 * s + 8 * h) * 2);
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                // transposing read: lane 16 kg + 4 tq + tp supplies key row 16 (s & 1) + 8 h + 4 rd + tq of the staged half, channels
                // 32 cb + 16 (kg & 1) + 4 tp ..; it receives channel 32 cb + r of the four rows
                const unsigned char *vb = Vs + (16 * (s & 1) + 8 * h + ((lane >> 2) & 3)) * G::VST + (32 * cb + 16 * (kg & 1) + 4 * (lane & 3)) * 2;
                const uint2 v0 = tr(vb), v1 = tr(vb + 4 * G::VST);
                oacc[cb] = T::mfma(make_uint4(v0.x, v0.y, v1.x, v1.y), pb, oacc[cb]);
            }
        };
        pv(0);
        if (kb + 16 < a.k) pv(1);
        if (second) {
            store_v();
            pv(2);
            if (kb + 48 < a.k) pv(3);
        }
    }
    // ---- row sums over the lane groups and the waves, then the store ----
#pragma unroll
    for (int qh = 0; qh < 2; ++qh) {
        float l = lrow[qh];
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        if (kg == 0) Ms[wave * NL_QT + 16 * qh + kq] = l;
    }
    __syncthreads();
    const float lsum = (Ms[r] + Ms[NL_QT + r]) + (Ms[2 * NL_QT + r] + Ms[3 * NL_QT + r]);
    asm volatile("" ::: "memory");
    // the wave's [32 queries][d/4] block through its private region: a lane holds four channels of one query, the store wants whole rows
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const uint32_t lo = (uint32_t)T::from_f32(oacc[cb][4 * gq] / lsum) | ((uint32_t)T::from_f32(oacc[cb][4 * gq + 1] / lsum) << 16);
            const uint32_t hi = (uint32_t)T::from_f32(oacc[cb][4 * gq + 2] / lsum) | ((uint32_t)T::from_f32(oacc[cb][4 * gq + 3] / lsum) << 16);
            *reinterpret_cast<uint2 *>(Vs + r * G::VST + (32 * cb + 8 * gq + 4 * h) * 2) = make_uint2(lo, hi);
        }
    asm volatile("" ::: "memory");
    uint16_t *obase = a.out + (size_t)item * a.q * a.ldo + wave * CW + vch * 8;
#pragma unroll
    for (int i = 0; i < NVH; ++i) {
        const int row = i * (64 / NV) + vrow;
        const uint4 v = *reinterpret_cast<const uint4 *>(Vs + row * G::VST + vch * 16);
        if (q0 + row < a.q) *reinterpret_cast<uint4 *>(obase + (size_t)(q0 + row) * a.ldo) = v;
    }
}

inline bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

template <typename T, int D>
int32_t nl_launch(const NlArgs &a, int n, hipStream_t s) {
    return launch_lds<nl_attention_kernel<T, D>>("tedspad_nl_attention_fwd", dim3((unsigned)(n * a.qtiles)), dim3(256), NlGeo<D>::LDS, s, a);
}

}  // namespace
}  // namespace tedspad

using namespace tedspad;

extern "C" int32_t tedspad_nl_attention_fwd(const void *theta, int32_t ld_theta, const void *phi, int32_t ld_phi, const void *g, int32_t ld_g, void *out,
                                            int32_t ld_out, int32_t n, int32_t q, int32_t k, int32_t d, float scale, int32_t dtype, void *stream) {
    TS_REQUIRE(theta && phi && g && out && n > 0 && q > 0 && k > 0, "tedspad_nl_attention_fwd: bad arguments (n=%d q=%d k=%d)", n, q, k);
    TS_REQUIRE(dtype == TEDSPAD_F16 || dtype == TEDSPAD_BF16, "tedspad_nl_attention_fwd: f16 / bf16 storage only (dtype=%d)", dtype);
    TS_REQUIRE(d == 256 || d == 512, "tedspad_nl_attention_fwd: no kernel for d = %d (the non-local blocks of I3Res50 have d = 256 and d = 512)", d);
    TS_REQUIRE(ld_theta >= d && ld_phi >= d && ld_g >= d && ld_out >= d && ld_theta % 8 == 0 && ld_phi % 8 == 0 && ld_g % 8 == 0 && ld_out % 8 == 0 &&
                   al16(theta) && al16(phi) && al16(g) && al16(out),
               "tedspad_nl_attention_fwd: rows must hold d channels, 16-byte aligned (ld %d %d %d %d)", ld_theta, ld_phi, ld_g, ld_out);
    TS_REQUIRE(out != theta && out != phi && out != g, "tedspad_nl_attention_fwd: out must not alias an input (other workgroups still read it)");
    const int qtiles = (q + NL_QT - 1) / NL_QT;
    TS_REQUIRE((int64_t)n * qtiles < (1ll << 31) && (int64_t)q * ld_theta < (1ll << 31) && (int64_t)k * ld_phi < (1ll << 31) && (int64_t)k * ld_g < (1ll << 31) &&
                   (int64_t)q * ld_out < (1ll << 31) && isfinite(scale),
               "tedspad_nl_attention_fwd: too large (n=%d q=%d k=%d) or a non-finite scale", n, q, k);
    const NlArgs a{(const uint16_t *)theta, (const uint16_t *)phi, (const uint16_t *)g, (uint16_t *)out, ld_theta, ld_phi, ld_g, ld_out, q, k, qtiles,
                   scale * 1.44269504088896340736f};
    if (d == 256) TS_WITH_T(dtype, return nl_launch<T, 256>(a, n, (hipStream_t)stream));
    TS_WITH_T(dtype, return nl_launch<T, 512>(a, n, (hipStream_t)stream));
    return TEDSPAD_OK;
}
