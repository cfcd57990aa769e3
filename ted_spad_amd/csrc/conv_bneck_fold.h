// Bottleneck tail of a layer1 block that ALSO emits the next block's conv1, for four-frame clips on gfx950:
//     y  = relu( bn3(conv3(relu(bn2(conv2(x))))) + residual )             (what conv_bneck_tail_kernel computes, bit for bit)
//     h' = relu( bn1'(conv1'(y)) )                                        (the next block's 3 x 1 x 1 conv, pads (1,0,0), 256 -> 64)
// in ONE launch (aux_code/models/large_i3d.py:61-84). Unfused, the 256-channel `y` is written by the tail, read as the next block's residual, and read a third
// time by the temporal-conv launch only to make the 64-channel h'; here that third read never happens.
//
// Tile: behind maxpool1 a 16-frame clip has T = 4 frames and a workgroup has 4 waves, so a workgroup owns an 8 x 8 pixel patch across all four frames of a
// clip and wave w takes frame w (a 64 co x 64 px register tile, as in the flat tile of conv_bneck.hip). The temporal neighbours t - 1, t + 1 of every pixel
// then sit in the sibling waves w - 1, w + 1. Frames need not be whole patches (layer1 is 55 x 55 at 224 x 224 clips: 7 x 7 patches, the last row and
// column 7 wide): a partial patch computes all 64 positions, reads zeros for the residual rows outside the frame and does not store those rows;
// both convolutions after conv2 are pointwise in space, so a position outside the frame never reaches one inside.
// Stage A: conv2 on the patch's 10 x 10 halo per frame (4 x 100 positions of 128 bytes, out-of-frame positions zero-filled); tap order, k order and MFMA
// shape are those of conv_bneck_tail_kernel, so `y` is bit-identical. The [64][64] weight tile of a tap streams through a THREE-slot ring (the four halos
// take 51.2 KB; a fourth slot would pass the 80 KB that let two workgroups share a CU), so a stage is in flight for one tap, not two.
// Stage B: per 64-channel output group as in conv_bneck_tail_kernel (conv3 weights streamed per group), up to the packed result.
// The fold: a group's packed result is already the MFMA B operand of the dt = 0 tap (the weight columns of that tap are stored in the accumulator k order,
// as w3p's are). The same group also passes through the wave-private row image on its way out; after a barrier wave w reads the images of waves w - 1 and
// w + 1 as B fragments (16-byte chunks of 8 channels per pixel row, natural k order) and accumulates W1[dt] . y[w + dt] into one 64 x 64 fp32 tile over the
// four groups. Waves 0 and 3 skip the tap that falls on temporal padding. h' leaves through the row image as whole 128-byte rows.
//
// Two forms share this body (one source file each, so that each is compiled and inspected alone):
//   plain (conv_bneck_fold.hip):     ... + residual, the wave's image receives the group's 64 residual channels of its 64 pixels before the results
//   DUAL (conv_bneck_fold_dual.hip): ... + bn_d(conv_d(x2)), the downsample branch of layer1.0 (large_i3d.py:49-54) in place of the residual:
//       y = relu( bn3(conv3(.)) + bn_d(conv_d(x2)) ), bit for bit what conv_bneck_tail_kernel<T, DUAL> stores.
//     The wave's image receives its frame's 64 px x 64 ch of x2 instead -- the SAME 8 KB for each of the four groups: the results of a group leave through
//     the image, so the rows are fetched again per group (three re-reads of 32 KB per workgroup, L2 hits) rather than held in 32 more registers. The x2
//     fragments are read from the image in natural k order (w3p's columns 64..127 are natural). bn3 and bn_d scale differently, so conv3 and conv_d keep
//     separate accumulators; a 32-channel tile is walked one pixel half at a time (a3 + ad = 32 registers, as the plain form's a3[2]) and the two weight
//     fragments are read twice from LDS.
#pragma once
#include "conv_common.h"
#include <type_traits>

namespace tedspad {
namespace {

__device__ uint4 g_fold_zero16b[8];       // a 128-byte line of zeros: halo positions and residual rows outside the frame

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int FD_WSTAGE = 64 * BK * 2;           // one [64][64] 16-bit weight tile
constexpr int FD_HALO = 4 * 100 * 128;           // four frames' 10 x 10 halos
constexpr int FD_WS = 3;                         // conv2 weight ring slots
// stage B's LDS map (plain 66 KB, DUAL 75 KB; stage A's halo + ring take 74 KB)
template <bool DUAL>
struct FoldMap {
    static constexpr int W3 = 0;                                      // conv3 weight tile of the group (DUAL: the downsample tile behind it)
    static constexpr int W1 = W3 + (DUAL ? 2 : 1) * FD_WSTAGE;        // the next conv1's three tap tiles of the group
    static constexpr int NBN = DUAL ? 3 : 2;                          // scale3, shift3 (, scale_d): [NBN][256] fp32
    static constexpr int BNV = W1 + 3 * FD_WSTAGE;
    static constexpr int IMG = BNV + NBN * 256 * 4;                   // one [64 px][64 ch] row image per wave
    static constexpr int A_END = FD_HALO + FD_WS * FD_WSTAGE, B_END = IMG + 4 * 8192;
    static constexpr int BN = A_END > B_END ? A_END : B_END;          // behind both stages: scale2, shift2, scale1', shift1': [4][64] fp32
    static constexpr int LDS = BN + 4 * 64 * 4;
    static_assert(LDS <= 80 * 1024, "two workgroups per CU");
};
static_assert(FoldMap<false>::BN == FD_HALO + FD_WS * FD_WSTAGE && FoldMap<true>::BN == 76800, "stage B ends below the BatchNorm vectors");

__device__ __forceinline__ void gstore16(void *dst, u32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" ::"v"(dst), "v"(v) : "memory");   // (see conv_bneck.hip)
}

// scale / shift (+ residual pair) + lower clamp + saturation of two neighbouring channels -> one packed pair (conv_bneck.hip's tail_pair)
template <typename T, bool RES>
__device__ __forceinline__ unsigned fold_pair(float a0, float a1, float s0, float s1, float b0, float b1, unsigned res, float lo) {
    if constexpr (T::kDtype == TEDSPAD_F16) {
        unsigned pk;
        if (RES) {
            float t0, t1;
            asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel_hi:[1,0,0]" : "=v"(t0) : "v"(res), "v"(b0));
            asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(t1) : "v"(res), "v"(b1));
            b0 = t0;
            b1 = t1;
        }
        const float v0 = __builtin_amdgcn_fmed3f(__builtin_fmaf(a0, s0, b0), lo, 65504.f);
        const float v1 = __builtin_amdgcn_fmed3f(__builtin_fmaf(a1, s1, b1), lo, 65504.f);
        asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(pk) : "v"(v0), "v"(v1));
        return pk;
    } else {
        float o0 = __builtin_fmaf(a0, s0, b0), o1 = __builtin_fmaf(a1, s1, b1);
        if (RES) {
            o0 += T::to_f32((uint16_t)(res & 0xffffu));
            o1 += T::to_f32((uint16_t)(res >> 16));
        }
        return (unsigned)T::from_f32(__builtin_fmaxf(o0, lo)) | ((unsigned)T::from_f32(__builtin_fmaxf(o1, lo)) << 16);
    }
}

struct FoldKP {
    const uint16_t *x;          // conv2 input (n,4,h,w,64+), pixel stride ldx
    const uint16_t *w2;         // conv2 weights, packed [64][9 * 64] (K = (dh, dw, ci))
    const float *scale2, *shift2;
    const uint16_t *w3p;        // [256][64]: conv3 weights, columns in accumulator k order; DUAL: [256][128], columns 64..127 = downsample weights (natural order)
    const float *scale3, *shift3;
    const uint16_t *res;        // plain: residual (n,4,h,w,256)
    const uint16_t *w1p;        // [4 groups][3 taps][64 co][64 k]: the next conv1; the dt = 0 tap's columns in accumulator k order, the others natural
    const float *scale1, *shift1;
    uint16_t *y, *hn;
    int H, W, PW, PPC;          // frame, patches per row, patches per clip
    int Kpad, ldx, ldres, ldy, ldh, relu;
};
struct FoldDualKP : FoldKP {    // DUAL: res / ldres unused; shift3 holds b3 + bd
    const uint16_t *x2;         // the downsample branch's source (n,4,h,w,64+), pixel stride ldx2
    const float *scaled;
    int ldx2;
};
template <bool DUAL>
using FoldArgs = std::conditional_t<DUAL, FoldDualKP, FoldKP>;

template <typename T, bool DUAL>
__global__ __launch_bounds__(256, 2) void conv_bneck_fold_kernel(const FoldArgs<DUAL> p) {
    constexpr int NT = 256;
    constexpr int FD_W3 = FoldMap<DUAL>::W3, FD_W1 = FoldMap<DUAL>::W1, FD_BNV = FoldMap<DUAL>::BNV, FD_IMG = FoldMap<DUAL>::IMG, FD_BN = FoldMap<DUAL>::BN;
    constexpr int NWT = DUAL ? 5 : 4;                                // weight tiles per group: conv3 (, downsample), three conv1' taps
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int clip = tile / p.PPC, pr = tile - clip * p.PPC;
    const int prow = pr / p.PW;
    const int py0 = prow * 8, px0 = (pr - prow * p.PW) * 8;          // the patch's first pixel in its frame
    const int HW = p.H * p.W;
    const long clip0 = (long)clip * 4 * HW;                          // first pixel of the clip
    const unsigned lds0 = (unsigned)(uintptr_t)(lptr_t)dsm;
    const uint16_t *zero = reinterpret_cast<const uint16_t *>(g_fold_zero16b);
    const int l31 = lane & 31, lh = lane >> 5;
    const int swz = (l31 >> 1) & 7;

    // ================================ stage A: conv2 on the four 10 x 10 halos ================================
    const int rsub = wave * 8 + (lane >> 3);
    const int kc = (lane & 7) ^ ((4 * (wave & 1) + (lane >> 4)) & 7);
    const uint16_t *wsrc = p.w2 + (size_t)rsub * p.Kpad + kc * 8;
    auto issue_w = [&](int kt, int slot) {
        const unsigned dst = lds0 + FD_HALO + slot * FD_WSTAGE + wave * 8 * (BK * 2);
        lds_dma16(wsrc + kt * BK, dst);
        lds_dma16(wsrc + (size_t)32 * p.Kpad + kt * BK, dst + 32 * (BK * 2));
    };
    // BatchNorm vectors of bn2 and of the next block's bn1 -> LDS behind everything else (read after stage A / after stage B)
    float *bnsm = reinterpret_cast<float *>(dsm + FD_BN);
    f32x4 bnreg = {0.f, 0.f, 0.f, 0.f};
    if (tid < 64) bnreg = reinterpret_cast<const f32x4 *>(tid < 16 ? p.scale2 : tid < 32 ? p.shift2 : tid < 48 ? p.scale1 : p.shift1)[tid & 15];
    issue_w(0, 0);
    // halo slot s = 16-byte chunk (s & 7) of position s >> 3; position = frame * 100 + hy * 10 + hx <-> pixel (py0 - 1 + hy, px0 - 1 + hx) of that frame
    for (int i = 0; i < (FD_HALO / 16 + NT - 1) / NT; ++i) {
        if (i * NT + wave * 64 >= FD_HALO / 16) break;                // wave-uniform
        const int s = i * NT + tid;
        const int pos = s >> 3, cs = s & 7;
        const int f = (pos * 656) >> 16;                              // pos / 100 (pos < 400)
        const int r = pos - f * 100;
        const int hy = (r * 205) >> 11;                               // r / 10 (r < 100)
        const int hx = r - hy * 10;
        const int yy = py0 - 1 + hy, xx = px0 - 1 + hx;
        const bool ok = (unsigned)yy < (unsigned)p.H && (unsigned)xx < (unsigned)p.W;
        const uint16_t *src = ok ? p.x + (clip0 + (long)f * HW + yy * p.W + xx) * p.ldx + ((cs ^ ((pos >> 1) & 7)) << 3) : zero;
        lds_dma16(src, lds0 + (i * NT + wave * 64) * 16);
    }
    issue_w(1, 1);
    // a lane's two pixels (b = 0, 1): pixel b * 32 + l31 of the wave's frame = (row b * 4 + (l31 >> 3), column l31 & 7) of the patch
    int pbase[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) pbase[b] = wave * 100 + (b * 4 + (l31 >> 3)) * 10 + (l31 & 7);
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    if (tid < 64) *reinterpret_cast<f32x4 *>(bnsm + tid * 4) = bnreg;
    wait_vmcnt<0>();                                     // halo + weight stages 0, 1 of this wave have landed
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    // The fragments of tap kt + 1 are requested during tap kt with asm ds_read_b128 and waited for with counted lgkmcnt, as in conv_bneck.hip's stage A. With
    // three ring slots: stage kt + 1 has landed when tap kt starts (wait + barrier), stage kt + 2 is issued behind the first MFMAs of tap kt into the slot of
    // stage kt - 1, whose fragments every wave consumed during tap kt - 1.
    u32x4 fa[4][2], fw[4][2];
    auto tap_pos = [&](int delta, unsigned (&xo)[2], unsigned (&xs)[2]) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int pos = pbase[b] + delta;
            xo[b] = (unsigned)pos * 128u;
            xs[b] = (unsigned)(pos >> 1) & 7u;
        }
    };
    auto read_frags = [&](int ks, int slot, const unsigned (&xo)[2], const unsigned (&xs)[2]) {
        const unsigned c = (unsigned)((ks << 1) | lh);
        const unsigned wt = lds0 + FD_HALO + slot * FD_WSTAGE + l31 * (BK * 2) + ((c ^ swz) << 4);
#pragma unroll
        for (int b = 0; b < 2; ++b) asm volatile("ds_read_b128 %0, %1" : "=v"(fa[ks][b]) : "v"(lds0 + xo[b] + ((c ^ xs[b]) << 4)));
        asm volatile("ds_read_b128 %0, %1" : "=v"(fw[ks][0]) : "v"(wt));
        asm volatile("ds_read_b128 %0, %1 offset:4096" : "=v"(fw[ks][1]) : "v"(wt));
    };
    static_assert(32 * BK * 2 == 4096, "second weight fragment: 32 rows further");
    unsigned xoff[2], xswz[2];
    tap_pos(0, xoff, xswz);
    asm volatile("; FD_COUNTED_LGKM_BEGIN" ::: "memory");      // (markers for the structure check of tests/test_l1_fold_host.py)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) read_frags(ks, 0, xoff, xswz);
    auto tap = [&](auto ktc) {
        constexpr int kt = decltype(ktc)::value;
        constexpr bool more = kt + 1 < 9;
        if constexpr (more) tap_pos(((kt + 1) / 3) * 10 + (kt + 1) % 3, xoff, xswz);
        if constexpr (kt >= 1 && more) {
            wait_vmcnt<0>();                             // stage kt + 1 landed
            __builtin_amdgcn_s_barrier();                // ... of every wave; nobody reads the slot of stage kt - 1 any more
            asm volatile("" ::: "memory");
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            u32x4 x0 = fa[ks][0], x1 = fa[ks][1], w0 = fw[ks][0], w1 = fw[ks][1];
            if (more || ks == 0) asm volatile("s_waitcnt lgkmcnt(12)" : "+v"(x0), "+v"(x1), "+v"(w0), "+v"(w1));
            else if (ks == 1) asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(x0), "+v"(x1), "+v"(w0), "+v"(w1));
            else if (ks == 2) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(x0), "+v"(x1), "+v"(w0), "+v"(w1));
            else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(x0), "+v"(x1), "+v"(w0), "+v"(w1));
            acc[0][0] = T::mfma(__builtin_bit_cast(uint4, w0), __builtin_bit_cast(uint4, x0), acc[0][0]);
            acc[0][1] = T::mfma(__builtin_bit_cast(uint4, w0), __builtin_bit_cast(uint4, x1), acc[0][1]);
            acc[1][0] = T::mfma(__builtin_bit_cast(uint4, w1), __builtin_bit_cast(uint4, x0), acc[1][0]);
            acc[1][1] = T::mfma(__builtin_bit_cast(uint4, w1), __builtin_bit_cast(uint4, x1), acc[1][1]);
            if constexpr (more) read_frags(ks, (kt + 1) % FD_WS, xoff, xswz);
            if constexpr (kt + 2 < 9) {
                if (ks == 0) issue_w(kt + 2, (kt + 2) % FD_WS);
            }
        }
    };
    using std::integral_constant;
    tap(integral_constant<int, 0>{}); tap(integral_constant<int, 1>{}); tap(integral_constant<int, 2>{});
    tap(integral_constant<int, 3>{}); tap(integral_constant<int, 4>{}); tap(integral_constant<int, 5>{});
    tap(integral_constant<int, 6>{}); tap(integral_constant<int, 7>{}); tap(integral_constant<int, 8>{});
    asm volatile("; FD_COUNTED_LGKM_END" ::: "memory");
    __syncthreads();         // every wave is done with the halos and the weight ring: stage B's images land there

    // ---- stage B's loads: per group the conv3 tile (DUAL: and the downsample tile), the next conv1's three tap tiles and the wave's residual rows (DUAL: its x2 rows)
    auto load_wt = [&](int g) {
        for (int i = wave; i < NWT * 8; i += 4) {          // 8 wave-instructions (8 rows x 128 B) per tile: tile 0 = conv3 (, 1 = downsample), the last three = conv1 taps
            const int tl = i >> 3, sub = i & 7;
            const int row = sub * 8 + (lane >> 3);
            const int ch = (lane & 7) ^ ((row >> 1) & 7);
            const uint16_t *src;
            if constexpr (DUAL) src = tl < 2 ? p.w3p + (size_t)(g * 64 + row) * 128 + tl * 64 + ch * 8 : p.w1p + (size_t)((g * 3 + tl - 2) * 64 + row) * 64 + ch * 8;
            else src = tl == 0 ? p.w3p + (size_t)(g * 64 + row) * 64 + ch * 8 : p.w1p + (size_t)((g * 3 + tl - 1) * 64 + row) * 64 + ch * 8;
            lds_dma16(src, lds0 + FD_W3 + tl * FD_WSTAGE + sub * 1024);
        }
    };
    static_assert(FD_W1 == FD_W3 + (NWT - 3) * FD_WSTAGE, "the tiles of a group are consecutive");
    float *bnv = reinterpret_cast<float *>(dsm + FD_BNV);
    unsigned char *wbuf = dsm + FD_IMG + wave * 8192;
    const unsigned wbuf_lds = lds0 + FD_IMG + wave * 8192;
    // row-layout role of this lane in instruction k: patch row k, column lane >> 3 (image row k * 8 + rrow), physical chunk lane & 7
    const int rrow = lane >> 3, rch = lane & 7;
    const int c0 = rch ^ (rrow >> 1);
    const long pix0 = clip0 + (long)wave * HW + (long)py0 * p.W + px0 + rrow;      // this lane's pixel of patch row 0 in the wave's frame
    const int rows_ok = min(8, p.H - py0);              // a partial patch at the frame's bottom / right edge: rows / columns inside the frame
    const bool col_ok = px0 + rrow < p.W;
    // Outside the frame: a lane whose column is outside reads the zero line in every row (base and row step chosen once per lane) and stores nothing; a row
    // outside does so for the whole wave (uniform). Every wave issues 8 loads per group and rows_ok stores: the counted wait below leaves 8 stores in flight
    // on whole patches and drains on the bottom-edge ones. (A shared scratch line for the skipped stores, as conv_bneck.hip's ragged last tile uses, is
    // written by a quarter of all workgroups at 55 x 55 and serialises them on one memory channel.)
    const int lstep = col_ok ? p.W : 0;
    // DUAL: the same eight row instructions fetch the wave's 64 px x 64 ch of x2 -- the same rows for every group (the group's results leave through the
    // image in between); the first fetch comes from HBM, the three after it are meant to hit L2, so they carry no nt hint.
    auto issue_res = [&](int g) {
        int opq = 0, ls = lstep;              // opaque: hipcc must not carry this call's row addresses across the group loop
        asm volatile("" : "+v"(opq), "+v"(ls));
        if constexpr (DUAL) {
            const uint16_t *base = col_ok ? p.x2 + (size_t)(pix0 + opq) * p.ldx2 : zero + opq;
#pragma unroll
            for (int k = 0; k < 8; ++k) lds_dma16((k < rows_ok ? base + (size_t)(k * ls) * p.ldx2 : zero) + ((c0 ^ ((k & 1) << 2)) << 3), wbuf_lds + k * 1024);
        } else {
            const uint16_t *base = col_ok ? p.res + (size_t)(pix0 + opq) * p.ldres + 64 * g : zero + opq;
#pragma unroll
            for (int k = 0; k < 8; ++k) lds_dma16_nt((k < rows_ok ? base + (size_t)(k * ls) * p.ldres : zero) + ((c0 ^ ((k & 1) << 2)) << 3), wbuf_lds + k * 1024);
        }
    };
    auto store_rows = [&](uint16_t *dstbase, int ld, const uint4 (&rowv)[8]) {
        int opq = 0;
        asm volatile("" : "+v"(opq));
        uint16_t *base = dstbase + (size_t)(pix0 + opq) * ld;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k >= rows_ok) break;               // wave-uniform
            uint16_t *dst = base + (size_t)(k * p.W) * ld + ((rch ^ (((k * 8 + rrow) >> 1) & 7)) << 3);
            if (col_ok) gstore16(dst, u32x4{rowv[k].x, rowv[k].y, rowv[k].z, rowv[k].w});
        }
    };
    load_wt(0);
    if constexpr (DUAL) {
        if (wave < 3) lds_dma16((wave == 0 ? p.scale3 : wave == 1 ? p.shift3 : p.scaled) + lane * 4, lds0 + FD_BNV + wave * 1024);
    } else {
        if (wave < 2) lds_dma16((wave == 0 ? p.scale3 : p.shift3) + lane * 4, lds0 + FD_BNV + wave * 1024);
    }
    issue_res(0);

    // ---- relu(bn2(.)) of the conv2 tile, packed to 16 bits: fragment (a*2 + s) = rows 16 s .. 16 s + 15 of channel half a ----------------------
    uint4 y2[4][2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        asm volatile("" ::: "memory");          // one channel half at a time (conv_bneck.hip)
        float sc[16], sf[16];
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            const int c = a * 32 + 8 * rq + 4 * lh;
            const f32x4 vs = *reinterpret_cast<const f32x4 *>(bnsm + c), vf = *reinterpret_cast<const f32x4 *>(bnsm + 64 + c);
#pragma unroll
            for (int i = 0; i < 4; ++i) { sc[4 * rq + i] = vs[i]; sf[4 * rq + i] = vf[i]; }
        }
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = __builtin_fmaxf(acc[a][b][8 * s + j] * sc[8 * s + j] + sf[8 * s + j], 0.f);
                y2[a * 2 + s][b] = pack8<T>(v);
            }
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int s = 0; s < 2; ++s) asm volatile("" : "+v"(y2[a * 2 + s][b].x), "+v"(y2[a * 2 + s][b].y), "+v"(y2[a * 2 + s][b].z), "+v"(y2[a * 2 + s][b].w));
    }

    // ================================ stage B: conv3 + residual on the register tile, and the fold ================================
    const float lo = p.relu ? 0.f : (T::kDtype == TEDSPAD_F16 ? -65504.f : -3.3e38f);
    f32x16 hacc[2][2];          // the next conv1's tile: 64 co x 64 px of this wave's frame
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) hacc[a][b][r] = 0.f;
    // packed pairs in the accumulator layout -> the store layout -> the wave's image -> whole rows
    auto to_image = [&](unsigned (&d)[2][2][4][2]) {
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
#pragma unroll
                for (int q = 0; q < 4; q += 2)
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        auto sw = __builtin_amdgcn_permlane32_swap(d[tt][b][q][h], d[tt][b][q + 1][h], false, false);
                        d[tt][b][q][h] = sw[0];
                        d[tt][b][q + 1][h] = sw[1];
                    }
#pragma unroll
                for (int qq = 0; qq < 2; ++qq) {
                    const unsigned c8 = (unsigned)(4 * tt + 2 * qq + lh);
                    *reinterpret_cast<uint4 *>(wbuf + (b * 32 + l31) * 128 + ((c8 ^ swz) << 4)) =
                        make_uint4(d[tt][b][2 * qq][0], d[tt][b][2 * qq][1], d[tt][b][2 * qq + 1][0], d[tt][b][2 * qq + 1][1]);
                }
            }
    };
    auto read_rows = [&](uint4 (&rowv)[8]) {
#pragma unroll
        for (int k = 0; k < 8; ++k) rowv[k] = *reinterpret_cast<const uint4 *>(wbuf + k * 1024 + lane * 16);
    };
    const unsigned char *W3t = dsm + FD_W3 + l31 * (BK * 2);
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {
        // this group's weight tiles and residual rows landed; the previous group's 8 stores (issued after them) stay in flight
        if (g && rows_ok == 8) wait_vmcnt<8>(); else wait_vmcnt<0>();
        __syncthreads();           // ... of every wave
        unsigned d[2][2][4][2];    // [32-channel tile][pixel half][q][h]: packed results in the accumulator layout
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            if constexpr (DUAL) {
                // conv3 and the downsample conv of the tile, one pixel half at a time: two accumulators (bn3 and bn_d scale differently), the x2 fragments of
                // the half from the wave's image (natural k order; to_image below overwrites it only after both tiles)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    __builtin_amdgcn_sched_barrier(0);      // keep the halves' live ranges apart: hoisted fragment and BatchNorm loads of the next half spill
                    f32x16 a3, ad;
#pragma unroll
                    for (int r = 0; r < 16; ++r) { a3[r] = 0.f; ad[r] = 0.f; }
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) {
                        const unsigned c = (unsigned)((ks << 1) | lh);
                        const uint4 f3 = *reinterpret_cast<const uint4 *>(W3t + tt * 32 * (BK * 2) + ((c ^ swz) << 4));
                        const uint4 fd = *reinterpret_cast<const uint4 *>(W3t + FD_WSTAGE + tt * 32 * (BK * 2) + ((c ^ swz) << 4));
                        const uint4 fx = *reinterpret_cast<const uint4 *>(wbuf + (b * 32 + l31) * 128 + ((c ^ swz) << 4));
                        a3 = T::mfma(f3, y2[ks][b], a3);
                        ad = T::mfma(fd, fx, ad);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    // lane (l31, lh) holds channels 64 g + 32 tt + 8 q + 4 lh + {0..3}, q = 0..3
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int c = 64 * g + 32 * tt + 8 * q + 4 * lh;
                        const f32x4 s3 = *reinterpret_cast<const f32x4 *>(bnv + c), b3 = *reinterpret_cast<const f32x4 *>(bnv + 256 + c);
                        const f32x4 sd = *reinterpret_cast<const f32x4 *>(bnv + 512 + c);
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int r = 4 * q + 2 * h;
                            d[tt][b][q][h] = tail_pair_dual<T>(a3[r], a3[r + 1], s3[2 * h], s3[2 * h + 1], b3[2 * h], b3[2 * h + 1], ad[r], ad[r + 1], sd[2 * h],
                                                               sd[2 * h + 1], p.relu);
                        }
                    }
                }
            } else {
                f32x16 a3[2];
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int r = 0; r < 16; ++r) a3[b][r] = 0.f;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const unsigned c = (unsigned)((ks << 1) | lh);
                    const uint4 f3 = *reinterpret_cast<const uint4 *>(W3t + tt * 32 * (BK * 2) + ((c ^ swz) << 4));
#pragma unroll
                    for (int b = 0; b < 2; ++b) a3[b] = T::mfma(f3, y2[ks][b], a3[b]);
                }
                // lane (l31, lh) holds channels 64 g + 32 tt + 8 q + 4 lh + {0..3}, q = 0..3
                f32x4 s3[4], b3[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = 64 * g + 32 * tt + 8 * q + 4 * lh;
                    s3[q] = *reinterpret_cast<const f32x4 *>(bnv + c);
                    b3[q] = *reinterpret_cast<const f32x4 *>(bnv + 256 + c);
                }
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    unsigned rs[4][2];
                    // residual chunks in the STORE layout (lane: channels 16 qq + 8 lh .. + 7 of the tile), swapped back into the accumulator layout
#pragma unroll
                    for (int qq = 0; qq < 2; ++qq) {
                        const unsigned c8 = (unsigned)(4 * tt + 2 * qq + lh);
                        const uint4 L = *reinterpret_cast<const uint4 *>(wbuf + (b * 32 + l31) * 128 + ((c8 ^ swz) << 4));
                        auto s0 = __builtin_amdgcn_permlane32_swap(L.x, L.z, false, false);
                        auto s1 = __builtin_amdgcn_permlane32_swap(L.y, L.w, false, false);
                        rs[2 * qq][0] = s0[0]; rs[2 * qq + 1][0] = s0[1];
                        rs[2 * qq][1] = s1[0]; rs[2 * qq + 1][1] = s1[1];
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int r = 4 * q + 2 * h;
                            d[tt][b][q][h] = fold_pair<T, true>(a3[b][r], a3[b][r + 1], s3[q][2 * h], s3[q][2 * h + 1], b3[q][2 * h], b3[q][2 * h + 1], rs[q][h], lo);
                        }
                }
            }
            // the dt = 0 tap: registers 8 s .. 8 s + 7 of the packed tile are the B fragment of k-step 2 tt + s of this group (no lane movement)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const unsigned c = (unsigned)(((2 * tt + s) << 1) | lh);
                const unsigned char *W1t = dsm + FD_W1 + FD_WSTAGE + l31 * (BK * 2) + ((c ^ swz) << 4);
                const uint4 w0 = *reinterpret_cast<const uint4 *>(W1t), w1 = *reinterpret_cast<const uint4 *>(W1t + 32 * (BK * 2));
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const uint4 fb = make_uint4(d[tt][b][2 * s][0], d[tt][b][2 * s][1], d[tt][b][2 * s + 1][0], d[tt][b][2 * s + 1][1]);
                    hacc[0][b] = T::mfma(w0, fb, hacc[0][b]);
                    hacc[1][b] = T::mfma(w1, fb, hacc[1][b]);
                }
            }
        }
        // ---- results -> the wave's image (every residual read above is complete: its data was consumed) -> whole rows ------------
        to_image(d);
        __syncthreads();           // every wave's image of this group is complete
        // ---- the dt = -1 / +1 taps: frames w - 1, w + 1 of the same pixels, from the sibling waves' images (natural k order) ----------
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const int nb = wave + 2 * side - 1;
            if (nb < 0 || nb > 3) continue;                 // temporal padding: nothing is multiplied (wave-uniform)
            const unsigned char *img = dsm + FD_IMG + nb * 8192 + l31 * 128;
            const unsigned char *W1t = dsm + FD_W1 + 2 * side * FD_WSTAGE + l31 * (BK * 2);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const unsigned c = (unsigned)((ks << 1) | lh);
                const uint4 w0 = *reinterpret_cast<const uint4 *>(W1t + ((c ^ swz) << 4)), w1 = *reinterpret_cast<const uint4 *>(W1t + 32 * (BK * 2) + ((c ^ swz) << 4));
                const uint4 f0 = *reinterpret_cast<const uint4 *>(img + ((c ^ swz) << 4)), f1 = *reinterpret_cast<const uint4 *>(img + 32 * 128 + ((c ^ swz) << 4));
                hacc[0][0] = T::mfma(w0, f0, hacc[0][0]);
                hacc[0][1] = T::mfma(w0, f1, hacc[0][1]);
                hacc[1][0] = T::mfma(w1, f0, hacc[1][0]);
                hacc[1][1] = T::mfma(w1, f1, hacc[1][1]);
            }
        }
        asm volatile("" ::: "memory");          // (the rows are read behind the neighbour taps: their 32 registers are not live beside those fragments)
        uint4 rowv[8];
        read_rows(rowv);
        __syncthreads();           // every wave has read its own and its neighbours' images and the group's weight tiles: the next group's may land
        if (g + 1 < 4) {
            load_wt(g + 1);
            issue_res(g + 1);
        }
        store_rows(p.y + 64 * g, p.ldy, rowv);
    }

    // ---- h' = relu(bn1'(.)) of the fold's tile -> the wave's image -> whole 128-byte rows -----------------------------------------------
    {
        unsigned d[2][2][4][2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            f32x4 s1[4], b1[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = 32 * a + 8 * q + 4 * lh;
                s1[q] = *reinterpret_cast<const f32x4 *>(bnsm + 128 + c);
                b1[q] = *reinterpret_cast<const f32x4 *>(bnsm + 192 + c);
            }
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int r = 4 * q + 2 * h;
                        d[a][b][q][h] = fold_pair<T, false>(hacc[a][b][r], hacc[a][b][r + 1], s1[q][2 * h], s1[q][2 * h + 1], b1[q][2 * h], b1[q][2 * h + 1], 0u, 0.f);
                    }
        }
        uint4 rowv[8];
        to_image(d);
        read_rows(rowv);
        store_rows(p.hn, p.ldh, rowv);
    }
}

// The checks and the launch behind both C entries. `src2`, `ld2`: the residual (256+ channels per pixel) of the plain form, x2 (64+) of DUAL; `scaled`: DUAL only.
template <bool DUAL>
inline int32_t fold_launch(const char *who, const tedspad_conv_desc *d2, const void *x, const void *w2_packed, const float *scale2, const float *shift2,
                           const void *w3p, const float *scale3, const float *shift3, const void *src2, int32_t ld2, const float *scaled, void *y, int32_t ldy,
                           int32_t relu, const void *w1p, const float *scale1, const float *shift1, void *h_next, int32_t ldh, void *stream) {
    TS_REQUIRE(d2 && x && w2_packed && scale2 && shift2 && w3p && scale3 && shift3 && src2 && y && w1p && scale1 && shift1 && h_next && (scaled || !DUAL),
               "%s: null pointer", who);
    TS_REQUIRE(d2->cin == 64 && d2->cout == 64 && d2->kt == 1 && d2->kh == 3 && d2->kw == 3 && d2->st == 1 && d2->sh == 1 && d2->sw == 1 && d2->pt == 0 &&
                   d2->ph == 1 && d2->pw == 1 && d2->to == d2->t && d2->ho == d2->h && d2->wo == d2->w,
               "%s: conv2 must be the stride-1 'same' 1 x 3 x 3 conv with 64 -> 64 channels", who);
    TS_REQUIRE(d2->n > 0 && d2->t == 4 && d2->h > 0 && d2->w > 0, "%s: four-frame clips only (t == 4)", who);
    TS_REQUIRE(d2->ldx >= 64 && d2->ldx % 8 == 0 && ldy >= 256 && ldy % 8 == 0 && ld2 >= (DUAL ? 64 : 256) && ld2 % 8 == 0 && ldh >= 64 && ldh % 8 == 0,
               "%s: bad leading dimension", who);
    TS_REQUIRE(((uintptr_t)x | (uintptr_t)w2_packed | (uintptr_t)w3p | (uintptr_t)y | (uintptr_t)src2 | (uintptr_t)w1p | (uintptr_t)h_next | (uintptr_t)scale3 |
                (uintptr_t)shift3 | (uintptr_t)scale2 | (uintptr_t)shift2 | (uintptr_t)scale1 | (uintptr_t)shift1 | (uintptr_t)scaled) % 16 == 0,
               "%s: pointers must be 16-byte aligned", who);
    TS_REQUIRE(d2->dtype == TEDSPAD_F16 || d2->dtype == TEDSPAD_BF16, "%s: bad dtype", who);
    const long M = (long)d2->n * 4 * d2->h * d2->w;
    int ldmax = d2->ldx > ldy ? d2->ldx : ldy;
    if (ld2 > ldmax) ldmax = ld2;
    if (ldh > ldmax) ldmax = ldh;
    TS_REQUIRE(M * ldmax < (1L << 31), "%s: tensor too large for 32-bit offsets; split the batch", who);
    FoldArgs<DUAL> p;
    p.x = (const uint16_t *)x; p.w2 = (const uint16_t *)w2_packed; p.scale2 = scale2; p.shift2 = shift2;
    p.w3p = (const uint16_t *)w3p; p.scale3 = scale3; p.shift3 = shift3;
    if constexpr (DUAL) {
        p.res = nullptr; p.ldres = 0;
        p.x2 = (const uint16_t *)src2; p.ldx2 = ld2; p.scaled = scaled;
    } else {
        p.res = (const uint16_t *)src2; p.ldres = ld2;
    }
    p.w1p = (const uint16_t *)w1p; p.scale1 = scale1; p.shift1 = shift1; p.y = (uint16_t *)y; p.hn = (uint16_t *)h_next;
    p.H = d2->h; p.W = d2->w; p.PW = (d2->w + 7) / 8; p.PPC = ((d2->h + 7) / 8) * p.PW;
    p.Kpad = tedspad_conv_kpad(d2); p.ldx = d2->ldx; p.ldy = ldy; p.ldh = ldh; p.relu = relu;
    TS_REQUIRE(p.Kpad == 9 * 64, "%s: unexpected K padding of the conv2 weights", who);
    const long tiles = (long)d2->n * p.PPC;
    TS_REQUIRE(tiles < (1L << 31), "%s: too many patches", who);
    TS_WITH_T(d2->dtype, return launch_lds<conv_bneck_fold_kernel<T, DUAL>>(who, dim3((unsigned)tiles), dim3(256), FoldMap<DUAL>::LDS, (hipStream_t)stream, p));
}

}  // namespace
}  // namespace tedspad
