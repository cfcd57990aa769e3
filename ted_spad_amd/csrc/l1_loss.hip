// nn.L1Loss (mean reduction) and its gradient for gfx950: the loss of fa_pretraining/train_reconstruction.py:46,77 (`criterion(output, inputs)`).
//
//  * l1_cl_kernel   : the TRAIN form. y is the segmentation head's 16-bit channels-last output (8-channel pixel records, first 3 valid, any ld), x the fp32 NCHW
//                     batch that is both the network's input and the target. One thread per pixel record: |float(y) - x| into the loss partial, the gradient
//                     record sign(float(y) - x) * g (g rounded once to the storage type; exactly 0 at a tie, NaN where the difference is NaN; channels 3-7 zero)
//                     as ONE 16-byte store in the (n,1,h,w,8) layout ConvLayer.wgrad / dgrad read, and optionally the fp32 NCHW copy of y.
//  * l1_flat_kernel : the same for two contiguous fp32 arrays of any layout (evaluation, losses.L1Loss); the fp32 gradient is optional. Told that the arrays are
//                     (n,c,hw) it adds in the train form's order: `evaluate` and `step` report the same bits for the same values.
//  * l1_finish_kernel: the per-workgroup partials -> the mean.
//
// Reductions are in a fixed order and use no atomics (the result is bit-identical from run to run, nothing here goes through det_gate.h): every lane adds its
// grid-strided terms in index order, a butterfly (__shfl_xor) over the 64 lanes, a 2-level tree over the 4 waves of the workgroup, one partial per workgroup in
// ws[blockIdx.x]; the finishing launch (one workgroup of L1_MAX_BLOCKS threads, one partial each, missing ones are 0) is the same tree over 16 waves. All terms
// are >= 0, so the relative error of the sum is at most (L + log2(P)) * 2^-24 with L = the additions a lane makes in sequence and P = L1_THREADS * L1_MAX_BLOCKS.
#include "common.h"

namespace tedspad {
namespace {

constexpr int L1_THREADS = 256, L1_MAX_BLOCKS = 1024;
static_assert(L1_MAX_BLOCKS == 1024 && L1_THREADS == 256, "the trees below are written for 4 and 16 waves");

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// every thread calls it; thread 0 returns the sum over the workgroup's NW waves (NW a power of two <= 64), combined as a tree
template <int NW>
__device__ __forceinline__ float block_sum(float v, float *sm) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = wave_sum(v);
    if (lane == 0) sm[wave] = v;
    __syncthreads();
    float t = 0.f;
    if (wave == 0) {
        t = lane < NW ? sm[lane] : 0.f;
#pragma unroll
        for (int o = NW / 2; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    }
    return t;
}

// sign(d) * g as torch.sign gives it: 0 at d == 0, NaN for a NaN difference
__device__ __forceinline__ float signed_g(float d, float g) { return d > 0.f ? g : (d < 0.f ? -g : (d == 0.f ? 0.f : d)); }
// the same on the storage type's bits, gb = g rounded once (the clamp of from_f32_lim would turn a NaN into -inf)
template <typename T>
__device__ __forceinline__ uint32_t signed_g16(float d, uint32_t gb) {
    constexpr uint32_t nan = T::kDtype == TEDSPAD_F16 ? 0x7e00u : 0x7fc0u;
    return d > 0.f ? gb : (d < 0.f ? (gb | 0x8000u) : (d == 0.f ? 0u : nan));
}

template <typename T>
__global__ __launch_bounds__(L1_THREADS) void l1_cl_kernel(const uint16_t *y, int ld, int wide, const float *x, uint16_t *dl, float *y32, float *ws, long hw,
                                                           long npix, float g) {
    __shared__ float sm[L1_THREADS / 64];
    float acc = 0.f;
    const uint32_t gb = T::from_f32_lim(g, __builtin_inff());
    for (long p = (long)blockIdx.x * L1_THREADS + threadIdx.x; p < npix; p += (long)gridDim.x * L1_THREADS) {
        const uint16_t *rec = y + p * ld;
        uint16_t q[3];
        if (wide) {                                            // records 8-byte aligned: channels 0-3 in one load
            const uint2 v = *reinterpret_cast<const uint2 *>(rec);
            q[0] = (uint16_t)(v.x & 0xffffu); q[1] = (uint16_t)(v.x >> 16); q[2] = (uint16_t)(v.y & 0xffffu);
        } else {
            q[0] = rec[0]; q[1] = rec[1]; q[2] = rec[2];
        }
        const long o = (p / hw) * 3 * hw + p % hw;              // (n, 0, pixel) of the NCHW arrays
        uint32_t v[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float yf = T::to_f32(q[ch]);
            const float d = __fsub_rn(yf, x[o + ch * hw]);
            acc = __fadd_rn(acc, __builtin_fabsf(d));
            v[ch] = signed_g16<T>(d, gb);
            if (y32) y32[o + ch * hw] = yf;
        }
        *reinterpret_cast<uint4 *>(dl + p * 8) = make_uint4(v[0] | (v[1] << 16), v[2], 0u, 0u);          // channels 3-7: zero
    }
    const float t = block_sum<L1_THREADS / 64>(acc, sm);
    if (threadIdx.x == 0) ws[blockIdx.x] = t;
}

// item p = the c elements (p / hw) * c * hw + p % hw + ch * hw: c = 1 is the plain index order, c = 3 walks an (n,3,hw) array pixel by pixel -- the partition and the
// order of l1_cl_kernel, so that both forms give the same bits on the same values
__global__ __launch_bounds__(L1_THREADS) void l1_flat_kernel(const float *y, const float *x, float *dy, float *ws, long items, int c, long hw, float g) {
    __shared__ float sm[L1_THREADS / 64];
    float acc = 0.f;
    for (long p = (long)blockIdx.x * L1_THREADS + threadIdx.x; p < items; p += (long)gridDim.x * L1_THREADS) {
        const long o = (p / hw) * c * hw + p % hw;
        for (int ch = 0; ch < c; ++ch) {
            const long i = o + ch * hw;
            const float d = __fsub_rn(y[i], x[i]);
            acc = __fadd_rn(acc, __builtin_fabsf(d));
            if (dy) dy[i] = signed_g(d, g);
        }
    }
    const float t = block_sum<L1_THREADS / 64>(acc, sm);
    if (threadIdx.x == 0) ws[blockIdx.x] = t;
}

__global__ __launch_bounds__(L1_MAX_BLOCKS) void l1_finish_kernel(const float *ws, int blocks, float numel, float *loss) {
    __shared__ float sm[L1_MAX_BLOCKS / 64];
    const float t = block_sum<L1_MAX_BLOCKS / 64>((int)threadIdx.x < blocks ? ws[threadIdx.x] : 0.f, sm);
    if (threadIdx.x == 0) *loss = __fdiv_rn(t, numel);
}

inline int l1_blocks(int64_t items) {
    const int64_t want = (items + L1_THREADS - 1) / L1_THREADS;
    return (int)(want < L1_MAX_BLOCKS ? want : L1_MAX_BLOCKS);
}

}  // namespace
}  // namespace tedspad

using namespace tedspad;

extern "C" int32_t tedspad_l1_block_threads(void) { return L1_THREADS; }
extern "C" int32_t tedspad_l1_max_blocks(void) { return L1_MAX_BLOCKS; }
extern "C" int32_t tedspad_l1_ws_floats(void) { return L1_MAX_BLOCKS; }

extern "C" int32_t tedspad_l1_loss_grad_cl(const void *y, int32_t ld, const float *x, void *dl, float *y32, float *ws, float *loss, int32_t n, int64_t hw,
                                           float grad_scale, int32_t dtype, void *stream) {
    TS_REQUIRE(y && x && dl && ws && loss, "tedspad_l1_loss_grad_cl: null argument (only y32 may be NULL)");
    TS_REQUIRE(n > 0 && hw > 0 && (int64_t)n * hw < ((int64_t)1 << 40), "tedspad_l1_loss_grad_cl: needs numel = n * 3 * hw > 0 (got n=%d hw=%lld)", n, (long long)hw);
    TS_REQUIRE(ld >= 8, "tedspad_l1_loss_grad_cl: y holds 8-channel pixel records, ld >= 8 (got %d)", ld);
    TS_REQUIRE(dtype == TEDSPAD_F16 || dtype == TEDSPAD_BF16, "tedspad_l1_loss_grad_cl: dtype must be TEDSPAD_F16 or TEDSPAD_BF16 (got %d)", dtype);
    TS_REQUIRE((uintptr_t)dl % 16 == 0 && (uintptr_t)y % 2 == 0, "tedspad_l1_loss_grad_cl: the gradient records must be 16-byte aligned");
    const int64_t npix = (int64_t)n * hw;
    const float numel = (float)(npix * 3), g = grad_scale / numel;
    const int blocks = l1_blocks(npix), wide = (uintptr_t)y % 8 == 0 && ld % 4 == 0;
    hipStream_t s = (hipStream_t)stream;
    TS_LAUNCH_T(dtype, l1_cl_kernel<T>, dim3(blocks), dim3(L1_THREADS), 0, s, (const uint16_t *)y, ld, wide, x, (uint16_t *)dl, y32, ws, (long)hw, (long)npix, g);
    hipLaunchKernelGGL(l1_finish_kernel, dim3(1), dim3(L1_MAX_BLOCKS), 0, s, (const float *)ws, blocks, numel, loss);
    return check_launch("tedspad_l1_loss_grad_cl");
}

extern "C" int32_t tedspad_l1_loss_flat(const float *y, const float *x, float *dy, float *ws, float *loss, int64_t numel, int32_t c, int64_t hw, float grad_scale,
                                        void *stream) {
    TS_REQUIRE(y && x && ws && loss, "tedspad_l1_loss_flat: null argument (only dy may be NULL)");
    TS_REQUIRE(numel > 0 && numel < ((int64_t)1 << 42), "tedspad_l1_loss_flat: needs numel > 0 (got %lld)", (long long)numel);
    TS_REQUIRE(c >= 1 && hw >= 1 && numel % ((int64_t)c * hw) == 0, "tedspad_l1_loss_flat: numel = %lld is not a multiple of c * hw = %d * %lld (c = 1, hw = numel: plain order)",
               (long long)numel, c, (long long)hw);
    const float nf = (float)numel, g = grad_scale / nf;
    const int64_t items = numel / c;
    const int blocks = l1_blocks(items);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(l1_flat_kernel, dim3(blocks), dim3(L1_THREADS), 0, s, y, x, dy, ws, (long)items, c, (long)hw, g);
    hipLaunchKernelGGL(l1_finish_kernel, dim3(1), dim3(L1_MAX_BLOCKS), 0, s, (const float *)ws, blocks, nf, loss);
    return check_launch("tedspad_l1_loss_flat");
}
