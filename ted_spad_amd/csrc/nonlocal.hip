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
// The LSE instantiation also writes the log-sum-exp of every query's logits: the tape of the backward kernels in the second half of this file.
#include <math.h>

#include "common.h"

namespace tedspad {
namespace {

struct NlArgs {
    const uint16_t *theta, *phi, *g;
    uint16_t *out;
    float *lse;        // (n, q) log-sum-exp of the scaled logits for the backward, written by the LSE instantiation only
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

template <typename T, int D, bool LSE>
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
    if constexpr (LSE) {                   // ln sum_j exp(scale s_j) = (m + log2 l) ln 2: the running max is the same in every wave
        if (wave == 0 && kg == 0) {
#pragma unroll
            for (int qh = 0; qh < 2; ++qh) {
                const int qc = 16 * qh + kq;
                const float l = (Ms[qc] + Ms[NL_QT + qc]) + (Ms[2 * NL_QT + qc] + Ms[3 * NL_QT + qc]);
                if (q0 + qc < a.q) a.lse[(size_t)item * a.q + q0 + qc] = (mrow[qh] + __builtin_amdgcn_logf(l)) * 0.69314718055994530942f;
            }
        }
    }
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
int32_t nl_launch(const char *who, const NlArgs &a, int n, hipStream_t s) {
    if (a.lse) return launch_lds<nl_attention_kernel<T, D, true>>(who, dim3((unsigned)(n * a.qtiles)), dim3(256), NlGeo<D>::LDS, s, a);
    return launch_lds<nl_attention_kernel<T, D, false>>(who, dim3((unsigned)(n * a.qtiles)), dim3(256), NlGeo<D>::LDS, s, a);
}

int32_t nl_forward(const char *who, const void *theta, int32_t ld_theta, const void *phi, int32_t ld_phi, const void *g, int32_t ld_g, void *out, int32_t ld_out,
                   float *lse, int32_t n, int32_t q, int32_t k, int32_t d, float scale, int32_t dtype, void *stream) {
    TS_REQUIRE(theta && phi && g && out && n > 0 && q > 0 && k > 0, "%s: bad arguments (n=%d q=%d k=%d)", who, n, q, k);
    TS_REQUIRE(dtype == TEDSPAD_F16 || dtype == TEDSPAD_BF16, "%s: f16 / bf16 storage only (dtype=%d)", who, dtype);
    TS_REQUIRE(d == 256 || d == 512, "%s: no kernel for d = %d (the non-local blocks of I3Res50 have d = 256 and d = 512)", who, d);
    TS_REQUIRE(ld_theta >= d && ld_phi >= d && ld_g >= d && ld_out >= d && ld_theta % 8 == 0 && ld_phi % 8 == 0 && ld_g % 8 == 0 && ld_out % 8 == 0 &&
                   al16(theta) && al16(phi) && al16(g) && al16(out),
               "%s: rows must hold d channels, 16-byte aligned (ld %d %d %d %d)", who, ld_theta, ld_phi, ld_g, ld_out);
    TS_REQUIRE(out != theta && out != phi && out != g, "%s: out must not alias an input (other workgroups still read it)", who);
    const int qtiles = (q + NL_QT - 1) / NL_QT;
    TS_REQUIRE((int64_t)n * qtiles < (1ll << 31) && (int64_t)q * ld_theta < (1ll << 31) && (int64_t)k * ld_phi < (1ll << 31) && (int64_t)k * ld_g < (1ll << 31) &&
                   (int64_t)q * ld_out < (1ll << 31) && isfinite(scale),
               "%s: too large (n=%d q=%d k=%d) or a non-finite scale", who, n, q, k);
    const NlArgs a{(const uint16_t *)theta, (const uint16_t *)phi, (const uint16_t *)g, (uint16_t *)out, lse, ld_theta, ld_phi, ld_g, ld_out, q, k, qtiles,
                   scale * 1.44269504088896340736f};
    if (d == 256) TS_WITH_T(dtype, return nl_launch<T, 256>(who, a, n, (hipStream_t)stream));
    TS_WITH_T(dtype, return nl_launch<T, 512>(who, a, n, (hipStream_t)stream));
    return TEDSPAD_OK;
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------------
// With S = scale theta phi^T, P = softmax_j(S) (recomputed as exp(S - lse)), T = P g and the upstream gradient dT:
//   dg = P^T dT,  dP = dT g^T,  D_i = sum_c dT[i,c] T[i,c],  dS = P o (dP - D),  dtheta = scale dS phi,  dphi = scale dS^T theta.
// Three launches, no atomics, fixed summation order (bit-identical from run to run and in any batch):
//   nl_dsum_kernel   D, one wave per 16 query rows, into the caller's workspace.
//   nl_bwd_kernel<KEYS = true>    one workgroup per (item, 32 keys) walks the queries in steps of 32 and keeps dphi and dg of its keys in fp32.
//   nl_bwd_kernel<KEYS = false>   one workgroup per (item, 32 queries) walks the keys in steps of 32 and keeps dtheta of its queries in fp32.
// Both are one template: a workgroup owns 32 RESIDENT rows (their two operands channel-contiguous in LDS) and walks the other side. Per step:
//   A   wave (wh, rh) takes walked rows 16 wh.. against resident rows 16 rh.. over all of d on the 16x16x32 MFMA: S and dP, the walked operands straight
//       from global memory (rows are channel-contiguous, which is what this product sums over). A lane ends with four walked rows of one resident row,
//       so dS (and P) go to LDS TRANSPOSED -- [resident row][walked row], 8 bytes per lane -- rounded to the storage type.
//   B   out^T[c][r] += W^T[c][w] M^T[w][r]: the sum runs over the walked rows, so the walked operand is staged [channel][walked row] in LDS (the transposition
//       is done by the staging stores); wave w owns channels w d/4 ... of every output. A lane ends with four channels of one resident row.
// Rows past the end: loads are clamped, P and dS are zero there, the transposed image holds zeros, resident rows past the end are not stored.
struct NlBwdArgs {
    const uint16_t *r1, *r2, *w1, *w2;     // resident / walked operands: (phi, g | theta, dT) for KEYS, (theta, dT | phi, g) otherwise
    uint16_t *o0, *o1;                     // KEYS: dphi, dg; otherwise dtheta
    const float *lse, *dsum;
    int ldr1, ldr2, ldw1, ldw2, ldo0, ldo1;
    int nr, nw, q, tiles;
    float c2, scale;
};

constexpr int NB_RT = 32;               // resident rows per workgroup = walked rows per step
constexpr int NB_TST = NB_RT * 2 + 16;  // bytes per row of the transposed images

template <int D, bool KEYS>
struct NlBwdGeo {
    static constexpr int NOUT = KEYS ? 2 : 1;
    static constexpr int RST = D * 2 + 16;
    static constexpr int R_BYTES = NB_RT * RST, W_BYTES = D * NB_TST, M_BYTES = NB_RT * NB_TST;
    static constexpr int LDS = 2 * R_BYTES + NOUT * (W_BYTES + M_BYTES);
};

// D_i = dT[i, :] . T[i, :] as the DIAGONAL of a 16 x 16 product on the same MFMA, in the same order of steps, as the dP = dT g^T of the kernels below: where a T row
// equals a g row bit for bit (one key; a one-hot softmax) dP - D is then exactly zero, which no other order of summation would give.
template <typename T>
__global__ __launch_bounds__(256) void nl_dsum_kernel(const uint16_t *t, int ldt, const uint16_t *dt, int lddt, float *dsum, long rows, int d) {
    const int lane = threadIdx.x & 63, kq = lane & 15, kg = lane >> 4;
    const long row0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    if (row0 >= rows) return;
    const long row = row0 + kq < rows ? row0 + kq : rows - 1;
    const uint16_t *pa = dt + (size_t)row * lddt + 8 * kg, *pb = t + (size_t)row * ldt + 8 * kg;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < d; c += 32) acc = T::mfma16(*reinterpret_cast<const uint4 *>(pa + c), *reinterpret_cast<const uint4 *>(pb + c), acc);
    if (kg == (kq >> 2) && row0 + kq < rows) dsum[row0 + kq] = acc[kq & 3];      // element (row 4 kg + e, column kq) with 4 kg + e == kq
}

template <typename T, int D, bool KEYS>
__global__ __launch_bounds__(256, (KEYS && D == 512) ? 1 : 2) void nl_bwd_kernel(const NlBwdArgs a) {
    using G = NlBwdGeo<D, KEYS>;
    constexpr int NOUT = G::NOUT, KS = D / 32, CW = D / 4, NCT = CW / 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned char *R1 = smem, *R2 = smem + G::R_BYTES, *Wt = smem + 2 * G::R_BYTES, *Mt = Wt + NOUT * G::W_BYTES;
    const int item = blockIdx.x / a.tiles, r0 = (blockIdx.x - item * a.tiles) * NB_RT;
    const uint16_t *r1 = a.r1 + (size_t)item * a.nr * a.ldr1, *r2 = a.r2 + (size_t)item * a.nr * a.ldr2;
    const uint16_t *w1 = a.w1 + (size_t)item * a.nw * a.ldw1, *w2 = a.w2 + (size_t)item * a.nw * a.ldw2;
    const float *lse = a.lse + (size_t)item * a.q, *dsum = a.dsum + (size_t)item * a.q;

    for (int idx = tid; idx < NB_RT * (D / 8); idx += 256) {              // the resident rows -> LDS
        const int row = idx / (D / 8), ch = idx - row * (D / 8);
        const int ri = min(r0 + row, a.nr - 1);
        *reinterpret_cast<uint4 *>(R1 + row * G::RST + ch * 16) = *reinterpret_cast<const uint4 *>(r1 + (size_t)ri * a.ldr1 + ch * 8);
        *reinterpret_cast<uint4 *>(R2 + row * G::RST + ch * 16) = *reinterpret_cast<const uint4 *>(r2 + (size_t)ri * a.ldr2 + ch * 8);
    }

    const int kq = lane & 15, kg = lane >> 4;
    const int wh = wave & 1, rh = wave >> 1;
    const int rres = r0 + 16 * rh + kq;                // phase A: this lane's resident row
    f32x4 acc[NOUT][NCT][2];
#pragma unroll
    for (int o = 0; o < NOUT; ++o)
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int h = 0; h < 2; ++h) acc[o][ct][h] = f32x4{0.f, 0.f, 0.f, 0.f};
    float lse_r = 0.f, d_r = 0.f;
    if (!KEYS) {                                       // the resident rows are the queries: one lse / D per lane for the whole walk
        lse_r = lse[min(rres, a.q - 1)] * 1.44269504088896340736f;
        d_r = dsum[min(rres, a.q - 1)];
    }
    __syncthreads();

    for (int w0 = 0; w0 < a.nw; w0 += NB_RT) {
        // ---- the walked rows, transposed: lane (wp, ch) takes rows 2 wp, 2 wp + 1 x 8 channels and stores eight row pairs ----
        for (int idx = tid; idx < (NB_RT / 2) * (D / 8); idx += 256) {
            const int wp = idx & 15, ch = idx >> 4;
            const int wa = w0 + 2 * wp, wb = wa + 1;
#pragma unroll
            for (int o = 0; o < NOUT; ++o) {
                const uint16_t *src = o == 0 ? w1 : w2;
                const int ld = o == 0 ? a.ldw1 : a.ldw2;
                uint4 va = *reinterpret_cast<const uint4 *>(src + (size_t)min(wa, a.nw - 1) * ld + ch * 8);
                uint4 vb = *reinterpret_cast<const uint4 *>(src + (size_t)min(wb, a.nw - 1) * ld + ch * 8);
                if (wa >= a.nw) va = make_uint4(0, 0, 0, 0);
                if (wb >= a.nw) vb = make_uint4(0, 0, 0, 0);
                const uint32_t xa[4] = {va.x, va.y, va.z, va.w}, xb[4] = {vb.x, vb.y, vb.z, vb.w};
                unsigned char *dst = Wt + o * G::W_BYTES + (8 * ch) * NB_TST + 4 * wp;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    *reinterpret_cast<uint32_t *>(dst + (2 * e) * NB_TST) = (xa[e] & 0xffffu) | (xb[e] << 16);
                    *reinterpret_cast<uint32_t *>(dst + (2 * e + 1) * NB_TST) = (xa[e] >> 16) | (xb[e] & 0xffff0000u);
                }
            }
        }
        // ---- A: S and dP of walked rows 16 wh.. x resident rows 16 rh..; lane (kq, kg) ends with walked rows 4 kg + e of resident row kq ----
        f32x4 sa = {0.f, 0.f, 0.f, 0.f}, da = {0.f, 0.f, 0.f, 0.f};
        const bool live = w0 + 16 * wh < a.nw && r0 + 16 * rh < a.nr;       // wave-uniform
        if (live) {
            const uint16_t *wa1 = w1 + (size_t)min(w0 + 16 * wh + kq, a.nw - 1) * a.ldw1 + 8 * kg;
            const uint16_t *wa2 = w2 + (size_t)min(w0 + 16 * wh + kq, a.nw - 1) * a.ldw2 + 8 * kg;
            const unsigned char *rb1 = R1 + (16 * rh + kq) * G::RST + 16 * kg, *rb2 = R2 + (16 * rh + kq) * G::RST + 16 * kg;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const uint4 a1 = *reinterpret_cast<const uint4 *>(wa1 + 32 * s), a2 = *reinterpret_cast<const uint4 *>(wa2 + 32 * s);
                sa = T::mfma16(a1, *reinterpret_cast<const uint4 *>(rb1 + 64 * s), sa);
                da = T::mfma16(a2, *reinterpret_cast<const uint4 *>(rb2 + 64 * s), da);
            }
        }
        float pv[4], dv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int wrow = w0 + 16 * wh + 4 * kg + e;
            float l2 = lse_r, dd = d_r;
            if (KEYS) {                                // the walked rows are the queries
                l2 = lse[min(wrow, a.q - 1)] * 1.44269504088896340736f;
                dd = dsum[min(wrow, a.q - 1)];
            }
            const bool valid = live && wrow < a.nw && rres < a.nr;
            pv[e] = valid ? __builtin_amdgcn_exp2f(sa[e] * a.c2 - l2) : 0.f;
            dv[e] = valid ? pv[e] * (da[e] - dd) : 0.f;
        }
        {
            unsigned char *m = Mt + (16 * rh + kq) * NB_TST + (16 * wh + 4 * kg) * 2;
            // training-path conversion (no +-65504 clamp): a dS past the f16 range, or a non-finite dT / lse, must reach the gradients as inf / NaN, where
            // the loss scale's non-finite check finds it -- clamped, dtheta and dphi would come out finite and wrong
            auto pk = [](float lo, float hi) { return (uint32_t)T::from_f32_lim(lo, INFINITY) | ((uint32_t)T::from_f32_lim(hi, INFINITY) << 16); };
            *reinterpret_cast<uint2 *>(m) = make_uint2(pk(dv[0], dv[1]), pk(dv[2], dv[3]));
            if (KEYS) *reinterpret_cast<uint2 *>(m + G::M_BYTES) = make_uint2(pk(pv[0], pv[1]), pk(pv[2], pv[3]));
        }
        __syncthreads();
        // ---- B: out^T[c][r] += W^T[c][w] M^T[w][r]; lane (kq, kg) ends with channels 16 ct + 4 kg + e of resident row 16 h + kq ----
#pragma unroll
        for (int o = 0; o < NOUT; ++o) {
            const unsigned char *mo = Mt + o * G::M_BYTES + kq * NB_TST + 16 * kg;
            const uint4 b0 = *reinterpret_cast<const uint4 *>(mo), b1 = *reinterpret_cast<const uint4 *>(mo + 16 * NB_TST);
            const unsigned char *wo = Wt + o * G::W_BYTES + (wave * CW + kq) * NB_TST + 16 * kg;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const uint4 av = *reinterpret_cast<const uint4 *>(wo + 16 * ct * NB_TST);
                acc[o][ct][0] = T::mfma16(av, b0, acc[o][ct][0]);
                acc[o][ct][1] = T::mfma16(av, b1, acc[o][ct][1]);
            }
        }
        __syncthreads();
    }
    // ---- each result rounded once; an overflow stays visible as inf, as in every training kernel ----
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
        uint16_t *out = (o == 0 ? a.o0 : a.o1) + (size_t)item * a.nr * (o == 0 ? a.ldo0 : a.ldo1) + wave * CW + 4 * kg;
        const int ld = o == 0 ? a.ldo0 : a.ldo1;
        const float f = o == 0 ? a.scale : 1.f;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = r0 + 16 * h + kq;
            if (row < a.nr) {
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    const f32x4 v = acc[o][ct][h];
                    const uint32_t lo = (uint32_t)T::from_f32_lim(v[0] * f, INFINITY) | ((uint32_t)T::from_f32_lim(v[1] * f, INFINITY) << 16);
                    const uint32_t hi = (uint32_t)T::from_f32_lim(v[2] * f, INFINITY) | ((uint32_t)T::from_f32_lim(v[3] * f, INFINITY) << 16);
                    *reinterpret_cast<uint2 *>(out + (size_t)row * ld + 16 * ct) = make_uint2(lo, hi);
                }
            }
        }
    }
}

template <typename T, int D>
int32_t nl_bwd_launch(const NlBwdArgs &keys, const NlBwdArgs &queries, const uint16_t *t, int ldt, const uint16_t *dt, int lddt, float *dsum, int n, int q,
                      hipStream_t s) {
    const char *who = "tedspad_nl_attention_bwd";
    const long rows = (long)n * q;
    hipLaunchKernelGGL(nl_dsum_kernel<T>, dim3((unsigned)((rows + 63) / 64)), dim3(256), 0, s, t, ldt, dt, lddt, dsum, rows, D);
    int32_t rc = check_launch(who);
    if (rc != TEDSPAD_OK) return rc;
    rc = launch_lds<nl_bwd_kernel<T, D, true>>(who, dim3((unsigned)(n * keys.tiles)), dim3(256), NlBwdGeo<D, true>::LDS, s, keys);
    if (rc != TEDSPAD_OK) return rc;
    return launch_lds<nl_bwd_kernel<T, D, false>>(who, dim3((unsigned)(n * queries.tiles)), dim3(256), NlBwdGeo<D, false>::LDS, s, queries);
}

}  // namespace
}  // namespace tedspad

using namespace tedspad;

extern "C" int32_t tedspad_nl_attention_fwd(const void *theta, int32_t ld_theta, const void *phi, int32_t ld_phi, const void *g, int32_t ld_g, void *out,
                                            int32_t ld_out, int32_t n, int32_t q, int32_t k, int32_t d, float scale, int32_t dtype, void *stream) {
    return nl_forward("tedspad_nl_attention_fwd", theta, ld_theta, phi, ld_phi, g, ld_g, out, ld_out, nullptr, n, q, k, d, scale, dtype, stream);
}

extern "C" int32_t tedspad_nl_attention_fwd_lse(const void *theta, int32_t ld_theta, const void *phi, int32_t ld_phi, const void *g, int32_t ld_g, void *out,
                                                int32_t ld_out, float *lse, int32_t n, int32_t q, int32_t k, int32_t d, float scale, int32_t dtype,
                                                void *stream) {
    TS_REQUIRE(lse && ((uintptr_t)lse & 3) == 0, "tedspad_nl_attention_fwd_lse: lse must be an fp32 (n, q) buffer");
    return nl_forward("tedspad_nl_attention_fwd_lse", theta, ld_theta, phi, ld_phi, g, ld_g, out, ld_out, lse, n, q, k, d, scale, dtype, stream);
}

extern "C" int32_t tedspad_nl_attention_bwd_workspace(int32_t n, int32_t q, int64_t *bytes) {
    TS_REQUIRE(bytes && n > 0 && q > 0, "tedspad_nl_attention_bwd_workspace: bad arguments (n=%d q=%d)", n, q);
    *bytes = (int64_t)n * q * (int64_t)sizeof(float);      // D, one fp32 per query row
    return TEDSPAD_OK;
}

extern "C" int32_t tedspad_nl_attention_bwd(const void *theta, int32_t ld_theta, const void *phi, int32_t ld_phi, const void *g, int32_t ld_g, const void *t,
                                            int32_t ld_t, const void *dt, int32_t ld_dt, const float *lse, void *dtheta, int32_t ld_dtheta, void *dphi,
                                            int32_t ld_dphi, void *dg, int32_t ld_dg, void *workspace, int32_t n, int32_t q, int32_t k, int32_t d, float scale,
                                            int32_t dtype, void *stream) {
    const char *who = "tedspad_nl_attention_bwd";
    TS_REQUIRE(theta && phi && g && t && dt && lse && dtheta && dphi && dg && workspace && n > 0 && q > 0 && k > 0, "%s: bad arguments (n=%d q=%d k=%d)", who, n,
               q, k);
    TS_REQUIRE(dtype == TEDSPAD_F16 || dtype == TEDSPAD_BF16, "%s: f16 / bf16 storage only (dtype=%d)", who, dtype);
    TS_REQUIRE(d == 256 || d == 512, "%s: no kernel for d = %d (the non-local blocks of I3Res50 have d = 256 and d = 512)", who, d);
    const int32_t lds[8] = {ld_theta, ld_phi, ld_g, ld_t, ld_dt, ld_dtheta, ld_dphi, ld_dg};
    const void *ptrs[8] = {theta, phi, g, t, dt, dtheta, dphi, dg};
    const int32_t rows[8] = {q, k, k, q, q, q, k, k};
    for (int i = 0; i < 8; ++i)
        TS_REQUIRE(lds[i] >= d && lds[i] % 8 == 0 && al16(ptrs[i]) && (int64_t)rows[i] * lds[i] < (1ll << 31),
                   "%s: rows must hold d channels, 16-byte aligned, an item below 2^31 elements (argument %d: ld %d)", who, i, lds[i]);
    TS_REQUIRE(((uintptr_t)lse & 3) == 0 && ((uintptr_t)workspace & 3) == 0, "%s: lse and the workspace are fp32 buffers", who);
    for (int o = 5; o < 8; ++o)
        for (int i = 0; i < 8; ++i) TS_REQUIRE(i == o || ptrs[o] != ptrs[i], "%s: an output must not alias another argument (%d, %d)", who, o, i);
    const int ktiles = (k + NB_RT - 1) / NB_RT, qtiles = (q + NB_RT - 1) / NB_RT;
    TS_REQUIRE((int64_t)n * qtiles < (1ll << 31) && (int64_t)n * ktiles < (1ll << 31) && (int64_t)n * q < (1ll << 33) && isfinite(scale), "%s: too large (n=%d q=%d k=%d) or a non-finite scale", who, n,
               q, k);
    const float c2 = scale * 1.44269504088896340736f;
    float *dsum = (float *)workspace;
    const uint16_t *th = (const uint16_t *)theta, *ph = (const uint16_t *)phi, *gg = (const uint16_t *)g, *tt = (const uint16_t *)t, *dd = (const uint16_t *)dt;
    const NlBwdArgs keys{ph, gg, th, dd, (uint16_t *)dphi, (uint16_t *)dg, lse, dsum, ld_phi, ld_g, ld_theta, ld_dt, ld_dphi, ld_dg, k, q, q, ktiles, c2, scale};
    const NlBwdArgs queries{th, dd, ph, gg, (uint16_t *)dtheta, nullptr, lse, dsum, ld_theta, ld_dt, ld_phi, ld_g, ld_dtheta, 0, q, k, q, qtiles, c2, scale};
    if (d == 256) TS_WITH_T(dtype, return (nl_bwd_launch<T, 256>(keys, queries, tt, ld_t, dd, ld_dt, dsum, n, q, (hipStream_t)stream)));
    TS_WITH_T(dtype, return (nl_bwd_launch<T, 512>(keys, queries, tt, ld_t, dd, ld_dt, dsum, n, q, (hipStream_t)stream)));
    return TEDSPAD_OK;
}
