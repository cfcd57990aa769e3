// The optimizer tail of a training step for gfx950: what `scaler.step(optimizer); scaler.update()` does in action_training/train_action.py:80-81 (and
// train_anonymized_action.py:87-88) for the optimizers the scripts choose from (train_action.py:251-259: Adam, AdamW, SGD), on a whole network at once.
//
//  * optim_check_kernel  : GradScaler's non-finite check. Reads every gradient of the chunk table once, writes nothing to them; a thread that saw an inf / NaN stores
//                          1 to state[0] (every racing writer stores the same constant: no atomics, no float atomics).
//  * optim_update_kernel : unscale (g * 1/scale, the scale read from the device; scales are powers of two, so this is exact) + the update of torch's single-tensor
//                          implementations (torch/optim/adam.py _single_tensor_adam, adamw.py, sgd.py _single_tensor_sgd; no amsgrad, no maximize, dampening 0, no
//                          nesterov) in fp32. One launch for all three. It returns at once when state[0] is set: parameters and state keep their bits.
//  * optim_finish_kernel : one thread. t += !found_inf, the next step's bias corrections, GradScaler.update(), found_inf = 0, and the two values the caller hands
//                          out (found_inf, the scale this step's gradients carried). A kernel of its own: folded into the update it would have to know that every
//                          workgroup has read state[0] -- an arrival counter across workgroups -- for the price of one ~2 us launch.
//
// The work list is a device-resident table of chunk records (tedspad_optim_chunk): one contiguous run of at most OPT_CHUNK elements of ONE tensor. A workgroup walks
// chunks blockIdx.x, + gridDim.x, ...; the record index is wave-uniform, so the record arrives by scalar loads and every branch on it is a scalar branch. Launch
// count and host work do not depend on the number of tensors.
//
// Memory: a pure stream, 28 B per element for Adam (p, g, m, v in; p, m, v out). Parameters and the state flats are 16-byte aligned per tensor (optim.py lays the
// state out so); gradient slots of grad_reduce.GradBucketReducer sit at any 4-byte phase. A full chunk issues all of its 16 loads per lane (4 x {p, g, m, v}) before
// the first use; g is loaded 16 bytes wide where its slot is 16-byte aligned and as four dwords where it is not (the same lines, four times the load instructions).
// A short chunk (a tensor's last one) takes a plain loop of vectors and then n % 4 single elements. A tensor whose p / m / v is not 16-byte aligned is walked
// element by element. Every path calls update_elem, written with explicitly rounded operations (no contraction the compiler could choose differently per path):
// an element's result does not depend on the path that handled it.
#include "common.h"

namespace tedspad {
namespace {

constexpr int OPT_THREADS = 256, OPT_VEC_PER_LANE = 4, OPT_CHUNK = OPT_THREADS * 4 * OPT_VEC_PER_LANE;      // 4096 elements
static_assert(sizeof(tedspad_optim_chunk) == 48, "optim.py builds the records as 6 x int64");

enum { OPT_ADAM = 0, OPT_ADAMW = 1, OPT_SGD = 2, OPT_SGD_PLAIN = 3 };      // SGD_PLAIN: momentum 0, no buffer

// Pointers read from the chunk table are generic to the compiler (flat loads); every one of them is global memory, and saying so gets global_load / global_store.
typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) f32x4 gf32x4;
typedef __attribute__((address_space(1))) uint32_t gu32;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) u32x4 gu32x4;
__device__ __forceinline__ gf32 *as_global(const float *p) { return reinterpret_cast<gf32 *>(reinterpret_cast<uintptr_t>(p)); }
__device__ __forceinline__ f32x4 ld4(const gf32 *p, int i) { return reinterpret_cast<const gf32x4 *>(p)[i]; }
__device__ __forceinline__ void st4(gf32 *p, int i, f32x4 v) { reinterpret_cast<gf32x4 *>(p)[i] = v; }
__device__ __forceinline__ f32x4 ld4_dwords(const gf32 *p, int i) { return f32x4{p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]}; }

struct OptHyper {
    float inv_scale, lr, wd, decay, omb1, beta2, omb2, eps, step_size, bc2_sqrt, mu;
};

template <int MODE>
__device__ __forceinline__ void update_elem(float &p, float g, float &m, float &v, const OptHyper &h) {
    g = __fmul_rn(g, h.inv_scale);
    if (MODE == OPT_ADAMW) p = __fmaf_rn(p, h.decay, p);                                    // adamw.py: param.mul_(1 - lr * weight_decay)
    else if (h.wd != 0.f) g = __fmaf_rn(h.wd, p, g);                                        // grad.add(param, alpha=weight_decay)
    if (MODE == OPT_SGD || MODE == OPT_SGD_PLAIN) {
        if (MODE == OPT_SGD) {
            m = __fmaf_rn(h.mu, m, g);                                                      // buf.mul_(momentum).add_(grad); zeros at the start: buf = grad
            g = m;
        }
        p = __fmaf_rn(-h.lr, g, p);
    } else {
        m = __fmaf_rn(h.omb1, __fsub_rn(g, m), m);                                          // exp_avg.lerp_(grad, 1 - beta1)
        v = __fmaf_rn(__fmul_rn(h.omb2, g), g, __fmul_rn(h.beta2, v));                      // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), h.bc2_sqrt), h.eps);         // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
        p = __fmaf_rn(-h.step_size, __fdiv_rn(m, denom), p);                                // param.addcdiv_(exp_avg, denom, value=-step_size)
    }
}

template <int MODE>
__device__ __forceinline__ void update_vec(f32x4 &p, const f32x4 &g, f32x4 &m, f32x4 &v, const OptHyper &h) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float pe = p[j], me = m[j], ve = v[j];
        update_elem<MODE>(pe, g[j], me, ve, h);
        p[j] = pe;
        m[j] = me;
        v[j] = ve;
    }
}

template <int MODE>
__device__ __forceinline__ void update_one(gf32 *p, const gf32 *g, gf32 *m, gf32 *v, int i, const OptHyper &h) {
    constexpr bool HAS_M = MODE != OPT_SGD_PLAIN, HAS_V = MODE == OPT_ADAM || MODE == OPT_ADAMW;
    float pe = p[i], me = 0.f, ve = 0.f;
    if (HAS_M) me = m[i];
    if (HAS_V) ve = v[i];
    update_elem<MODE>(pe, g[i], me, ve, h);
    p[i] = pe;
    if (HAS_M) m[i] = me;
    if (HAS_V) v[i] = ve;
}

// a full chunk: every lane owns OPT_VEC_PER_LANE vectors, all loads issued before the first use
template <int MODE, bool G_ALIGNED>
__device__ __forceinline__ void update_full_chunk(gf32 *p, const gf32 *g, gf32 *m, gf32 *v, const OptHyper &h) {
    constexpr bool HAS_M = MODE != OPT_SGD_PLAIN, HAS_V = MODE == OPT_ADAM || MODE == OPT_ADAMW;
    f32x4 P[OPT_VEC_PER_LANE], G[OPT_VEC_PER_LANE], M[OPT_VEC_PER_LANE], V[OPT_VEC_PER_LANE];
#pragma unroll
    for (int k = 0; k < OPT_VEC_PER_LANE; ++k) {
        const int i = threadIdx.x + k * OPT_THREADS;
        P[k] = ld4(p, i);
        G[k] = G_ALIGNED ? ld4(g, i) : ld4_dwords(g, i);
        M[k] = HAS_M ? ld4(m, i) : f32x4{0.f, 0.f, 0.f, 0.f};
        V[k] = HAS_V ? ld4(v, i) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int k = 0; k < OPT_VEC_PER_LANE; ++k) {
        const int i = threadIdx.x + k * OPT_THREADS;
        update_vec<MODE>(P[k], G[k], M[k], V[k], h);
        st4(p, i, P[k]);
        if (HAS_M) st4(m, i, M[k]);
        if (HAS_V) st4(v, i, V[k]);
    }
}

template <int MODE>
__global__ __launch_bounds__(OPT_THREADS) void optim_update_kernel(const tedspad_optim_chunk *__restrict__ table, int nchunks, const int32_t *__restrict__ state,
                                                                   const float *__restrict__ scale, float lr, float wd, float omb1, float beta2, float omb2,
                                                                   float eps, float mu) {
    constexpr bool HAS_M = MODE != OPT_SGD_PLAIN, HAS_V = MODE == OPT_ADAM || MODE == OPT_ADAMW;
    if (state[0] != 0) return;                                   // found_inf: the step is skipped, nothing is written
    OptHyper h;
    h.inv_scale = scale ? __fdiv_rn(1.f, scale[0]) : 1.f;
    h.lr = lr; h.wd = wd; h.decay = -__fmul_rn(lr, wd); h.omb1 = omb1; h.beta2 = beta2; h.omb2 = omb2; h.eps = eps; h.mu = mu;
    h.step_size = __fdiv_rn(lr, __builtin_bit_cast(float, state[2]));                      // lr / (1 - beta1^t)
    h.bc2_sqrt = __builtin_bit_cast(float, state[3]);                                       // sqrt(1 - beta2^t)
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const tedspad_optim_chunk rec = table[c];               // wave-uniform: scalar loads
        gf32 *p = as_global(rec.p), *m = as_global(rec.m), *v = as_global(rec.v);
        const gf32 *g = as_global(rec.g);
        const int n = (int)rec.n;
        uintptr_t a = (uintptr_t)p;
        if (HAS_M) a |= (uintptr_t)m;
        if (HAS_V) a |= (uintptr_t)v;
        if ((a & 15) != 0) {                                     // a tensor that is not 16-byte aligned: element by element
            for (int i = threadIdx.x; i < n; i += OPT_THREADS) update_one<MODE>(p, g, m, v, i, h);
            continue;
        }
        const bool g_aligned = ((uintptr_t)g & 15) == 0;
        if (n == OPT_CHUNK) {
            if (g_aligned) update_full_chunk<MODE, true>(p, g, m, v, h);
            else update_full_chunk<MODE, false>(p, g, m, v, h);
            continue;
        }
        const int nv = n >> 2;                                   // a tensor's last chunk: whole vectors, then the n % 4 elements behind them
        for (int i = threadIdx.x; i < nv; i += OPT_THREADS) {
            f32x4 P = ld4(p, i), M = {0.f, 0.f, 0.f, 0.f}, V = M;
            const f32x4 G = g_aligned ? ld4(g, i) : ld4_dwords(g, i);
            if (HAS_M) M = ld4(m, i);
            if (HAS_V) V = ld4(v, i);
            update_vec<MODE>(P, G, M, V, h);
            st4(p, i, P);
            if (HAS_M) st4(m, i, M);
            if (HAS_V) st4(v, i, V);
        }
        if ((int)threadIdx.x < (n & 3)) update_one<MODE>(p, g, m, v, 4 * nv + threadIdx.x, h);
    }
}

__device__ __forceinline__ uint32_t non_finite(uint32_t bits) { return (bits & 0x7f800000u) == 0x7f800000u ? 1u : 0u; }

__global__ __launch_bounds__(OPT_THREADS) void optim_check_kernel(const tedspad_optim_chunk *__restrict__ table, int nchunks, int32_t *state) {
    uint32_t bad = 0;
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const gu32 *g = reinterpret_cast<const gu32 *>(reinterpret_cast<uintptr_t>(table[c].g));
        const int n = (int)table[c].n;
        int head = (int)((4 - (((uintptr_t)g >> 2) & 3)) & 3);  // elements in front of the first 16-byte boundary
        head = head < n ? head : n;
        const int nv = (n - head) >> 2, tail = n - head - 4 * nv;
        const gu32x4 *gv = reinterpret_cast<const gu32x4 *>(g + head);
#pragma unroll 4
        for (int i = threadIdx.x; i < nv; i += OPT_THREADS) {
            const u32x4 q = gv[i];
            bad |= non_finite(q.x) | non_finite(q.y) | non_finite(q.z) | non_finite(q.w);
        }
        if ((int)threadIdx.x < head) bad |= non_finite(g[threadIdx.x]);
        if ((int)threadIdx.x < tail) bad |= non_finite(g[head + 4 * nv + threadIdx.x]);
    }
    if (bad) state[0] = 1;
}

__global__ void optim_finish_kernel(int32_t *state, float *scale_state, double beta1, double beta2, float growth, float backoff, int growth_interval, float *out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int found = state[0];
    const float scale = scale_state ? scale_state[0] : 1.f;
    out[0] = found ? 1.f : 0.f;
    out[1] = scale;
    if (!found) {
        double *pw = reinterpret_cast<double *>(state + 4);      // beta^(t+1) of the step just applied -> of the next one
        const double b1 = pw[0] * beta1, b2 = pw[1] * beta2;
        pw[0] = b1;
        pw[1] = b2;
        state[1] += 1;
        state[2] = __builtin_bit_cast(int32_t, (float)(1.0 - b1));
        state[3] = __builtin_bit_cast(int32_t, (float)__dsqrt_rn(1.0 - b2));
    }
    if (scale_state && growth_interval > 0) {                   // torch.amp.GradScaler.update (_amp_update_scale_)
        int tracker = __builtin_bit_cast(int32_t, scale_state[1]);
        float s = scale;
        if (found) {
            s = __fmul_rn(s, backoff);
            tracker = 0;
        } else if (++tracker == growth_interval) {
            const float grown = __fmul_rn(s, growth);
            if (grown < __builtin_inff()) s = grown;
            tracker = 0;
        }
        scale_state[0] = s;
        scale_state[1] = __builtin_bit_cast(float, tracker);
    }
    state[0] = 0;
}

}  // namespace
}  // namespace tedspad

using namespace tedspad;

extern "C" int32_t tedspad_optim_chunk_elems(void) { return OPT_CHUNK; }

extern "C" int32_t tedspad_optim_check(const tedspad_optim_chunk *table, int32_t nchunks, int32_t *state, void *stream) {
    TS_REQUIRE(table && state, "tedspad_optim_check: null argument");
    TS_REQUIRE(nchunks > 0, "tedspad_optim_check: needs nchunks > 0 (got %d)", nchunks);
    hipLaunchKernelGGL(optim_check_kernel, dim3(grid_for((long)nchunks * OPT_THREADS)), dim3(OPT_THREADS), 0, (hipStream_t)stream, table, nchunks, state);
    return check_launch("tedspad_optim_check");
}

extern "C" int32_t tedspad_optim_update(const tedspad_optim_chunk *table, int32_t nchunks, int32_t mode, const int32_t *state, const float *scale, float lr,
                                        double beta1, double beta2, float eps, float weight_decay, float momentum, void *stream) {
    TS_REQUIRE(table && state, "tedspad_optim_update: null argument (only scale may be NULL)");
    TS_REQUIRE(nchunks > 0, "tedspad_optim_update: needs nchunks > 0 (got %d)", nchunks);
    TS_REQUIRE(mode == OPT_ADAM || mode == OPT_ADAMW || mode == OPT_SGD, "tedspad_optim_update: mode must be 0 (adam), 1 (adamw) or 2 (sgd), got %d", mode);
    TS_REQUIRE((uintptr_t)state % 8 == 0, "tedspad_optim_update: state must be 8-byte aligned");
    if (mode == OPT_SGD && momentum == 0.f) mode = OPT_SGD_PLAIN;
    const dim3 grid(grid_for((long)nchunks * OPT_THREADS)), block(OPT_THREADS);
    hipStream_t s = (hipStream_t)stream;
    const float omb1 = (float)(1.0 - beta1), b2 = (float)beta2, omb2 = (float)(1.0 - beta2);
#define TS_OPT_LAUNCH(M) hipLaunchKernelGGL(optim_update_kernel<M>, grid, block, 0, s, table, nchunks, state, scale, lr, weight_decay, omb1, b2, omb2, eps, momentum)
    switch (mode) {
        case OPT_ADAM: TS_OPT_LAUNCH(OPT_ADAM); break;
        case OPT_ADAMW: TS_OPT_LAUNCH(OPT_ADAMW); break;
        case OPT_SGD: TS_OPT_LAUNCH(OPT_SGD); break;
        default: TS_OPT_LAUNCH(OPT_SGD_PLAIN); break;
    }
#undef TS_OPT_LAUNCH
    return check_launch("tedspad_optim_update");
}

extern "C" int32_t tedspad_optim_finish(int32_t *state, float *scale_state, double beta1, double beta2, float growth, float backoff, int32_t growth_interval,
                                        float *out, void *stream) {
    TS_REQUIRE(state && out, "tedspad_optim_finish: null argument (only scale_state may be NULL)");
    TS_REQUIRE((uintptr_t)state % 8 == 0, "tedspad_optim_finish: state must be 8-byte aligned");
    hipLaunchKernelGGL(optim_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, scale_state, beta1, beta2, growth, backoff, (int)growth_interval, out);
    return check_launch("tedspad_optim_finish");
}
