// The two HBM-bound steps either side of the encoder, for gfx950:
//   * frames -> /255 -> crop box -> antialiased bilinear resize (-> optional horizontal flip) -> fp32 clip
//     (DALIDataloader.val_augmentations, feature_extraction/dali_extraction.py:38-50)
//   * (T, ncrops, F) features -> 32-segment mean pooling + L2 magnitude channel
//     (process_feat, anomaly_detection_mgfn/utils/utils.py:34-42; Dataset.__getitem__, datasets/dataset.py:65-100)
// Both are pure bandwidth work: every global access below is a run of consecutive bytes / floats across the
// lanes of a wave, intermediates live in LDS, and grids are one workgroup per output row (>> 256 workgroups).
#include <math.h>

#include "common.h"

namespace tedspad {
namespace {

// ------------------------------------------------------------------------------------------------------------
// antialiased separable bilinear resize, weights as torch builds them for F.interpolate(mode='bilinear',
// antialias=True, align_corners=False) -- which is what torchvision's F.resize(antialias=True) calls on a
// float tensor (dali_extraction.py:49). Table entry of output index i: {xmin, xsize, w[0..taps)}.
// ------------------------------------------------------------------------------------------------------------
inline int aa_taps(int in, int out) {
    const float scale = (float)in / (float)out;
    const float support = scale >= 1.f ? scale : 1.f;
    return (int)ceilf(support) * 2 + 1;
}

inline void aa_table(int in, int out, int32_t *tab) {
    const int taps = aa_taps(in, out);
    const float scale = (float)in / (float)out;
    const float support = scale >= 1.f ? scale : 1.f;
    const float invscale = scale >= 1.f ? 1.f / scale : 1.f;
    for (int i = 0; i < out; i++) {
        int32_t *e = tab + (size_t)i * (2 + taps);
        float *w = (float *)(e + 2);
        const float center = scale * ((float)i + 0.5f);
        long lo = (long)(center - support + 0.5f);
        long hi = (long)(center + support + 0.5f);
        if (lo < 0) lo = 0;
        if (hi > in) hi = in;
        int n = (int)(hi - lo);
        if (n > taps) n = taps;
        float total = 0.f;
        for (int j = 0; j < taps; j++) w[j] = 0.f;
        for (int j = 0; j < n; j++) {
            float x = ((float)(j + lo) - center + 0.5f) * invscale;
            x = fabsf(x);
            w[j] = x < 1.f ? 1.f - x : 0.f;
            total += w[j];
        }
        if (total != 0.f)
            for (int j = 0; j < n; j++) w[j] /= total;
        e[0] = (int32_t)lo;
        e[1] = n;
    }
}

struct ResizeKP {
    const void *in;
    float *out;
    const int32_t *ytab, *xtab;
    int T, H, W, C;          // frames are (T, H, W, C) with C interleaved (DALI / decoder layout)
    int y0, x0, ch, cw;      // crop box
    int oh, ow, ytaps, xtaps;
    int flip;
    float div;               // 255: applied as a true division per sample, like `video / 255.`
    long so_t, so_c, so_h, so_w;
};

// bytes a[0..3] as one dword (byte k in bits 8k..): aligned 4-byte loads (one, or two joined by v_alignbyte_b32 when `a` is not 4-byte aligned) where they stay
// inside the buffer, single bytes at its very end. `a & 3` is wave-uniform for the callers below (uniform row pointer + 4 * lane group).
__device__ __forceinline__ unsigned load_u8x4(const uint8_t *a, const uint8_t *end) {
    const unsigned sh = (unsigned)((uintptr_t)a & 3u);
    if (a + 8 <= end) {
        const unsigned *ap = reinterpret_cast<const unsigned *>(a - sh);
        const unsigned w0 = ap[0];
        if (sh == 0) return w0;
        return __builtin_amdgcn_alignbyte(ap[1], w0, sh);
    }
    unsigned w = 0;
    for (int k = 0; k < 4; ++k)
        if (a + k < end) w |= (unsigned)a[k] << (8 * k);
    return w;
}

// byte / divisor of the kernels that load four bytes at a time (crop_resize_tp_kernel, crop_resize_act_kernel): for 255 without the division or a table --
// b * fl(1/255) corrected by one residual step is the correctly rounded quotient for every byte value (checked exhaustively in exact arithmetic; tests compare
// with the dividing kernel bit for bit) -- else from the workgroup's 256-entry table lut[b] = (float)b / div.
__device__ __forceinline__ float u8_px(unsigned bt, bool div255, const float *lut) {
    if (div255) {
        const float xb = (float)bt, r = 1.0f / 255.0f;
        const float q0 = xb * r;
        return __builtin_fmaf(__builtin_fmaf(-q0, 255.0f, xb), r, q0);
    }
    return lut[bt];
}

template <typename In> __device__ __forceinline__ float load_px(const In *p, float div);
template <> __device__ __forceinline__ float load_px<uint8_t>(const uint8_t *p, float div) { return (float)(*p) / div; }
template <> __device__ __forceinline__ float load_px<float>(const float *p, float div) { return *p / div; }

// The two passes, shared by the fp32-clip kernel and the stem-record kernel below (one source expression per value: the two kernels give the same bits).
// Pass 1 (vertical): every lane owns interleaved (x, c) elements of the cropped input row span, consecutive lanes = consecutive bytes, and reduces the
// <= ytaps input rows of this output row into LDS. Pass 2 (horizontal): a lane owns an output pixel and reads its taps from LDS.
template <typename In>
__device__ __forceinline__ void aa_vpass(const In *base, long rstride, const int32_t *ye, int span, float div, float *row) {
    const int yn = ye[1];
    const float *wy = (const float *)(ye + 2);
    for (int e = threadIdx.x; e < span; e += 256) {
        float acc = 0.f;
        for (int j = 0; j < yn; j++) acc += wy[j] * load_px<In>(base + j * rstride + e, div);
        row[e] = acc;
    }
}
__device__ __forceinline__ float aa_hpass(const float *row, const int32_t *xe, int C, int c) {
    const int xmin = xe[0], xn = xe[1];
    const float *wx = (const float *)(xe + 2);
    float acc = 0.f;
    for (int j = 0; j < xn; j++) acc += wx[j] * row[(xmin + j) * C + c];
    return acc;
}

// One workgroup per (frame, output row).
template <typename In>
__global__ __launch_bounds__(256) void crop_resize_aa_kernel(const ResizeKP p) {
    extern __shared__ float row[];      // cw * C
    const int t = blockIdx.x / p.oh, oy = blockIdx.x % p.oh;
    const int32_t *ye = p.ytab + (size_t)oy * (2 + p.ytaps);
    const In *base = (const In *)p.in + (((long)t * p.H + p.y0 + ye[0]) * p.W + p.x0) * p.C;
    aa_vpass<In>(base, (long)p.W * p.C, ye, p.cw * p.C, p.div, row);
    __syncthreads();
    for (int ox = threadIdx.x; ox < p.ow; ox += 256) {
        const int32_t *xe = p.xtab + (size_t)ox * (2 + p.xtaps);
        const int oxw = p.flip ? p.ow - 1 - ox : ox;
        for (int c = 0; c < p.C; c++) p.out[t * p.so_t + c * p.so_c + oy * p.so_h + oxw * p.so_w] = aa_hpass(row, xe, p.C, c);
    }
}

// The same resize written as the persistent stem's input records (csrc/conv_stem_pt.hip, tedspad_clip_to_tp's layout): X[n][tp][oh][b][ow/2][24] 16-bit, the
// record of pixel (oy, 2*wq + b) for output-frame pair tp holding value dt*3 + c = clip[n][c][4*tp - pt + dt][oy][2*wq + b], dt = 0..7 (temporal stride 2),
// zero outside the clip. Clip n = source frames first + n*clip_step + f*frame_step, f = 0 .. t_clip - 1 (dali_extraction.py:62-73: sequence_length 16,
// stride 2, step 32), frames past the end of the video are zero frames (pad_sequences). The fp32 clip (9.6 MB at 16 x 224 x 224) is never written.
// A workgroup owns one output row of one QUAD of frames 4*qd - pt .. 4*qd - pt + 3 of one clip: those four frames are the first half (dt 0..3, 24 bytes) of
// pair qd's records AND the second half (dt 4..7) of pair qd - 1's, so every frame is resized once, into one LDS tile of half records (5.3 KB at 224
// columns), which leaves twice as 8-byte pieces; the sibling quad's workgroup (the next blockIdx) fills the other halves of the same lines right behind it.
// One load -> sync -> resize -> sync -> store chain per workgroup, ~24 KB of LDS: six workgroups per CU. (One workgroup per (clip, row) with all four pairs'
// records in a 43 KB tile: two per CU, 9.0 ms per 375 clips; one per (clip, row, pair), every frame resized twice: 3.5 ms; byte loads instead of 4-byte
// loads cost 3.6 ms of an earlier 6.6: scripts/crop_tp_probe.py.)
struct ResizeTpKP {
    ResizeKP r;
    uint16_t *rec;
    int n_clips, first, clip_step, frame_step, t_clip, pt, stt, tp_n;
    const uint8_t *in_end;      // one past the last byte of the frame buffer (the 4-byte loads of the uint8 path stay inside it)
};

template <typename In, typename T>
__global__ __launch_bounds__(256) void crop_resize_tp_kernel(const ResizeTpKP q) {
    constexpr int FG = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_tp[];
    const ResizeKP &p = q.r;
    const int wq_n = p.ow >> 1;
    uint2 *tile = reinterpret_cast<uint2 *>(lds_tp);                 // [plane b][wq][3 x 8 B]: half records (4 frames x 3 channels)
    const int tile8 = 2 * wq_n * 3;
    const int span = p.cw * p.C;
    float *rows = reinterpret_cast<float *>(lds_tp + (size_t)tile8 * 8);        // [FG][span]
    float *lut = rows + FG * span;                                   // [256] (uint8 input, divisor != 255)
    int32_t *xt = reinterpret_cast<int32_t *>(lut + 256);            // this launch's column table [ow][2 + xtaps]: read 4 x 3 times per output pixel below
    const int nq = q.tp_n + 1;
    const int qd = blockIdx.x % nq, rowid = blockIdx.x / nq;
    const int n = rowid / p.oh, oy = rowid % p.oh;
    const int f0 = 4 * qd - q.pt;                                    // first clip frame of the quad
    const bool div255 = p.div == 255.0f;
    for (int i = threadIdx.x; i < tile8; i += 256) tile[i] = make_uint2(0u, 0u);               // frames outside the clip, channels >= C
    if (sizeof(In) == 1 && !div255) lut[threadIdx.x] = (float)threadIdx.x / p.div;
    for (int i = threadIdx.x; i < p.ow * (2 + p.xtaps); i += 256) xt[i] = p.xtab[i];
    const int32_t *ye = p.ytab + (size_t)oy * (2 + p.ytaps);
    const int yn = ye[1];
    const float *wy = (const float *)(ye + 2);
    const long rstride = (long)p.W * p.C;
    uint16_t *t16 = reinterpret_cast<uint16_t *>(lds_tp);
    const In *base[FG];
    bool live[FG];
#pragma unroll
    for (int ff = 0; ff < FG; ++ff) {
        const long fr = (long)q.first + (long)n * q.clip_step + (long)(f0 + ff) * q.frame_step;
        live[ff] = f0 + ff >= 0 && f0 + ff < q.t_clip && fr >= 0 && fr < p.T;    // else a zero frame: its slots stay zero (uniform)
        base[ff] = (const In *)p.in + (((live[ff] ? fr : 0) * p.H + p.y0 + ye[0]) * p.W + p.x0) * p.C;
    }
    if constexpr (sizeof(In) == 1) {
        if (!div255) __syncthreads();                                // the value table (uniform branch)
        // four consecutive bytes per lane and load (byte loads: 64 bytes per wave instruction)
        for (int g = threadIdx.x; 4 * g < span; g += 256) {
            float acc[FG][4];
#pragma unroll
            for (int ff = 0; ff < FG; ++ff)
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[ff][k] = 0.f;
            for (int j = 0; j < yn; j++) {
                unsigned w4[FG];
#pragma unroll
                for (int ff = 0; ff < FG; ++ff) w4[ff] = live[ff] ? load_u8x4(reinterpret_cast<const uint8_t *>(base[ff]) + j * rstride + 4 * g, q.in_end) : 0u;
#pragma unroll
                for (int ff = 0; ff < FG; ++ff)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        acc[ff][k] += wy[j] * u8_px((w4[ff] >> (8 * k)) & 255u, div255, lut);
                    }
            }
#pragma unroll
            for (int ff = 0; ff < FG; ++ff)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (4 * g + k < span) rows[ff * span + 4 * g + k] = acc[ff][k];
        }
    } else {
        for (int e = threadIdx.x; e < span; e += 256) {
            float acc[FG];
#pragma unroll
            for (int ff = 0; ff < FG; ++ff) acc[ff] = 0.f;
            for (int j = 0; j < yn; j++) {
#pragma unroll
                for (int ff = 0; ff < FG; ++ff) acc[ff] += wy[j] * (live[ff] ? load_px<In>(base[ff] + j * rstride + e, p.div) : 0.f);
            }
#pragma unroll
            for (int ff = 0; ff < FG; ++ff) rows[ff * span + e] = acc[ff];
        }
    }
    __syncthreads();                                                 // rows, the zeroed tile and the column table are complete
    for (int ox = threadIdx.x; ox < p.ow; ox += 256) {
        const int32_t *xe = xt + ox * (2 + p.xtaps);
        const int xmin = xe[0], xn = xe[1];
        const float *wx = reinterpret_cast<const float *>(xe + 2);
        const int oxw = p.flip ? p.ow - 1 - ox : ox;
        // aa_hpass for the FG frames x 3 channels at once: a tap's weight is read once; every sum still runs over its taps in ascending order
        float acc[FG][3];
#pragma unroll
        for (int ff = 0; ff < FG; ++ff)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[ff][c] = 0.f;
        for (int j = 0; j < xn; j++) {
            const float wj = wx[j];
            const float *r = rows + (xmin + j) * p.C;
#pragma unroll
            for (int ff = 0; ff < FG; ++ff)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (c < p.C) acc[ff][c] += wj * r[ff * span + c];
        }
        uint16_t *rec = t16 + ((size_t)((oxw & 1) * wq_n + (oxw >> 1))) * 12;
#pragma unroll
        for (int ff = 0; ff < FG; ++ff) {
            if (!live[ff]) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) rec[ff * 3 + c] = c < p.C ? T::from_f32(acc[ff][c]) : (uint16_t)0;
        }
    }
    __syncthreads();
    // half records -> pair qd (first halves) and pair qd - 1 (second halves); both planes of a row are one contiguous run of records
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int tp = qd - half;
        if (tp < 0 || tp >= q.tp_n) continue;                        // uniform
        uint2 *dst = reinterpret_cast<uint2 *>(q.rec) + ((((long)n * q.tp_n + tp) * p.oh + oy) * 2 * (long)wq_n) * 6 + half * 3;
        for (int i = threadIdx.x; i < tile8; i += 256) {
            const int rc = i / 3, pc = i - rc * 3;
            dst[(long)rc * 6 + pc] = tile[i];
        }
    }
}

// torchvision's ten_crop in front of the same resize (preprocess.ten_crop_boxes: tl, tr, bl, br, centre of the frame, then the same five of the horizontally
// flipped frame), all ten crops' records X[10*n + crop] in one launch. The ten boxes have three row origins (0, yc, H - ch), and a crop of the flipped frame is
// the mirror image of a crop of the unflipped one: crop 5 (flipped tl) = crop 1 (tr) written right to left, 6 = mirror of 0, 7 = of 3, 8 = of 2, and crop 9 is the
// mirror of the box at column W - cw - xc -- which is crop 4's box only when W - cw is even (center_crop rounds half to even: xc = 14 of 27 puts the flipped
// frame's centre crop at column 13).
// A workgroup owns one output row of one quad of frames (as crop_resize_tp_kernel) of one ROW ORIGIN: the vertical pass runs once over the columns its boxes
// cover (the full width for the corner origins), the horizontal pass once per distinct column origin (two for the corners; one for the centre, two when W - cw is
// odd) into one LDS tile of half records each, and every tile leaves up to twice per record half: in record order, and for a flipped crop in reversed record
// order (pixel ox of the mirror = pixel ow - 1 - ox: the other plane, pair ow/2 - 1 - wq). Same helpers and source expressions as crop_resize_tp_kernel: every
// record has the bits of the ten launches it replaces.
// Block order: the quads of one (row, row origin) write the two halves of the same records, and the hardware deals consecutive blocks round-robin over the 8
// XCDs, each with an L2 of its own, so in hardware order the two halves of a cache line leave two L2s as two partial writes. The kernel numbers its work so that
// the tp_n + 1 quads of a row are blocks b, b + 8, ... : one XCD (as observed; a placement the result does not depend on), whose L2 joins the halves. That alone
// took the launch from 3.10 ms to 1.37 ms at 370 clips of 224 x 224; the column table read from global memory instead of a copy in LDS
// (27 KB, six workgroups per CU, instead of 33 KB, four) gave 1.24 ms.
struct TenCropKP {
    ResizeTpKP q;               // q.r.y0, q.r.x0 and q.r.flip are not used
    int yc, xc;                 // the centre crop's origin (preprocess.center_crop_box)
    int nblk;                   // (clip time, output row, row origin, quad) items; the grid is rounded up to a multiple of 8 * (tp_n + 1)
};

template <typename In, typename T>
__global__ __launch_bounds__(256) void ten_crop_tp_kernel(const TenCropKP kp) {
    constexpr int FG = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_tc[];
    const ResizeTpKP &q = kp.q;
    const ResizeKP &p = q.r;
    const int wq_n = p.ow >> 1;
    const int tile8 = 2 * wq_n * 3;
    uint2 *tile = reinterpret_cast<uint2 *>(lds_tc);                 // [column origin a, b][plane][wq][3 x 8 B]
    const int rbuf = p.W * p.C;                                      // a frame's row buffer: the full width
    float *rows = reinterpret_cast<float *>(lds_tc + (size_t)2 * tile8 * 8);    // [FG][rbuf]
    float *lut = rows + FG * rbuf;                                   // [256] (uint8 input, divisor != 255)
    const int32_t *xt = p.xtab;
    const int nq = q.tp_n + 1;
    const int slot = blockIdx.x >> 3;                                // blocks b, b + 8, ... in turn: the quads of one row, then the next row of this residue
    const int bid = ((slot / nq) * 8 + (blockIdx.x & 7)) * nq + slot % nq;
    if (bid >= kp.nblk) return;                                      // the grid's rounding (uniform)
    const int qd = bid % nq;
    const int grp = (bid / nq) % 3, rowid = bid / (3 * nq);          // row origin: 0 top, 1 centre, 2 bottom
    const int n = rowid / p.oh, oy = rowid % p.oh;
    const int f0 = 4 * qd - q.pt;
    const bool div255 = p.div == 255.0f;
    const int y0 = grp == 0 ? 0 : grp == 1 ? kp.yc : p.H - p.ch;
    const int xa = grp == 1 ? kp.xc : 0, xb = p.W - p.cw - xa;       // column origins: of the direct crop, and of the box whose mirror is the flipped frame's crop
    const int x_lo = xa < xb ? xa : xb;
    const int ncol = xa == xb ? 1 : 2;
    const int span = ((xa < xb ? xb : xa) + p.cw - x_lo) * p.C;      // <= rbuf
    for (int i = threadIdx.x; i < ncol * tile8; i += 256) tile[i] = make_uint2(0u, 0u);
    if (sizeof(In) == 1 && !div255) lut[threadIdx.x] = (float)threadIdx.x / p.div;
    const int32_t *ye = p.ytab + (size_t)oy * (2 + p.ytaps);
    const int yn = ye[1];
    const float *wy = (const float *)(ye + 2);
    const long rstride = (long)p.W * p.C;
    const In *base[FG];
    bool live[FG];
#pragma unroll
    for (int ff = 0; ff < FG; ++ff) {
        const long fr = (long)q.first + (long)n * q.clip_step + (long)(f0 + ff) * q.frame_step;
        live[ff] = f0 + ff >= 0 && f0 + ff < q.t_clip && fr >= 0 && fr < p.T;
        base[ff] = (const In *)p.in + (((live[ff] ? fr : 0) * p.H + y0 + ye[0]) * p.W + x_lo) * p.C;
    }
    if constexpr (sizeof(In) == 1) {
        if (!div255) __syncthreads();
        for (int g = threadIdx.x; 4 * g < span; g += 256) {
            float acc[FG][4];
#pragma unroll
            for (int ff = 0; ff < FG; ++ff)
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[ff][k] = 0.f;
            for (int j = 0; j < yn; j++) {
                unsigned w4[FG];
#pragma unroll
                for (int ff = 0; ff < FG; ++ff) w4[ff] = live[ff] ? load_u8x4(reinterpret_cast<const uint8_t *>(base[ff]) + j * rstride + 4 * g, q.in_end) : 0u;
#pragma unroll
                for (int ff = 0; ff < FG; ++ff)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        acc[ff][k] += wy[j] * u8_px((w4[ff] >> (8 * k)) & 255u, div255, lut);
                    }
            }
#pragma unroll
            for (int ff = 0; ff < FG; ++ff)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (4 * g + k < span) rows[ff * rbuf + 4 * g + k] = acc[ff][k];
        }
    } else {
        for (int e = threadIdx.x; e < span; e += 256) {
            float acc[FG];
#pragma unroll
            for (int ff = 0; ff < FG; ++ff) acc[ff] = 0.f;
            for (int j = 0; j < yn; j++) {
#pragma unroll
                for (int ff = 0; ff < FG; ++ff) acc[ff] += wy[j] * (live[ff] ? load_px<In>(base[ff] + j * rstride + e, p.div) : 0.f);
            }
#pragma unroll
            for (int ff = 0; ff < FG; ++ff) rows[ff * rbuf + e] = acc[ff];
        }
    }
    __syncthreads();
    for (int it = threadIdx.x; it < ncol * p.ow; it += 256) {        // (column origin, output pixel)
        const int col = it >= p.ow, ox = it - col * p.ow;
        const int32_t *xe = xt + ox * (2 + p.xtaps);
        const int xmin = xe[0], xn = xe[1];
        const float *wx = reinterpret_cast<const float *>(xe + 2);
        const float *rw = rows + ((col ? xb : xa) - x_lo + xmin) * p.C;
        float acc[FG][3];
#pragma unroll
        for (int ff = 0; ff < FG; ++ff)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[ff][c] = 0.f;
        for (int j = 0; j < xn; j++) {
            const float wj = wx[j];
            const float *r = rw + j * p.C;
#pragma unroll
            for (int ff = 0; ff < FG; ++ff)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (c < p.C) acc[ff][c] += wj * r[ff * rbuf + c];
        }
        uint16_t *rec = reinterpret_cast<uint16_t *>(tile + col * tile8) + ((size_t)((ox & 1) * wq_n + (ox >> 1))) * 12;
#pragma unroll
        for (int ff = 0; ff < FG; ++ff) {
            if (!live[ff]) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) rec[ff * 3 + c] = c < p.C ? T::from_f32(acc[ff][c]) : (uint16_t)0;
        }
    }
    __syncthreads();
    // crops of this row origin: ka from origin a, ka + 1 from origin b (corners), 5 + ka = the mirror of origin b, 5 + ka + 1 = the mirror of origin a (corners)
    const int ka = grp == 0 ? 0 : grp == 1 ? 4 : 2;
    const uint2 *ta = tile, *tb = tile + (ncol - 1) * tile8;
    const int nrec = 2 * wq_n;
    const bool corner = grp != 1;
    const long clip8 = (long)q.tp_n * p.oh * nrec * 6;               // a clip's records in 8-byte pieces
    uint2 *dst[2];                                                   // this row of crop 0, pair qd (first halves) and pair qd - 1 (second halves)
    bool on[2];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int tp = qd - half;
        on[half] = tp >= 0 && tp < q.tp_n;                           // uniform
        dst[half] = reinterpret_cast<uint2 *>(q.rec) + (long)n * 10 * clip8 + (((long)(on[half] ? tp : 0) * p.oh + oy) * (long)nrec) * 6 + half * 3;
    }
    // a piece is read once per tile and order and leaves for both pairs: four loads from LDS in flight, then up to eight stores
    for (int i = threadIdx.x; i < tile8; i += 256) {
        const int rc = i / 3, pc = i - rc * 3, mi = (nrec - 1 - rc) * 3 + pc;
        const uint2 va = ta[i], vbm = tb[mi];
        uint2 vb = va, vam = vbm;
        if (corner) {
            vb = tb[i];
            vam = ta[mi];
        }
        const long o = (long)rc * 6 + pc;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if (!on[half]) continue;
            uint2 *d = dst[half] + o;
            d[ka * clip8] = va;
            d[(5 + ka) * clip8] = vbm;
            if (corner) {
                d[(ka + 1) * clip8] = vb;
                d[(6 + ka) * clip8] = vam;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------
// uint8 frames -> crop box -> Pillow's two-pass BILINEAR resize (8-bit intermediate image) -> /255 -> fp32:
// `shanghai_frames_dataset.augmentation` (feature_extraction/shanghai_dl.py:27-40: to_pil_image, center_crop, resize(antialias),
// to_tensor). Pillow (libImaging/Resample.c, 8 bits per channel) resamples HORIZONTALLY first, rounds that image to uint8, then
// vertically, with fixed-point coefficients of 22 fractional bits: out = clip8((2^21 + sum px * kk) >> 22). The integer tables
// {first index, count, kk[0..taps)} are built on the host exactly as precompute_coeffs / normalize_coeffs_8bpc do (preprocess.py).
// One workgroup per (frame, output row): a thread owns output pixels (x, c) and runs the horizontal pass of the <= ytaps
// temporary rows it needs itself (every input row feeds ~2 output rows: 2x redundant integer MACs on a memory-bound op).
// ------------------------------------------------------------------------------------------------------------
struct ResizeU8KP {
    const uint8_t *in;
    float *out;
    const int32_t *ytab, *xtab;
    int T, H, W, C, y0, x0, oh, ow, ytaps, xtaps;
    long so_t, so_c, so_h, so_w;
};

__device__ __forceinline__ int clip8_fixed(int v) {
    v >>= 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ __launch_bounds__(256) void crop_resize_pil_kernel(const ResizeU8KP p) {
    const int t = blockIdx.x / p.oh, oy = blockIdx.x % p.oh;
    const int32_t *ye = p.ytab + (size_t)oy * (2 + p.ytaps);
    const int ymin = ye[0], yn = ye[1];
    const uint8_t *base = p.in + (((long)t * p.H + p.y0 + ymin) * p.W + p.x0) * p.C;
    const long rstride = (long)p.W * p.C;
    for (int e = threadIdx.x; e < p.ow * p.C; e += 256) {
        const int ox = e / p.C, c = e - ox * p.C;
        const int32_t *xe = p.xtab + (size_t)ox * (2 + p.xtaps);
        const int xmin = xe[0], xn = xe[1];
        int acc = 1 << 21;
        for (int j = 0; j < yn; j++) {
            const uint8_t *r = base + j * rstride + (long)xmin * p.C + c;
            int hs = 1 << 21;
            for (int i = 0; i < xn; i++) hs += (int)r[(long)i * p.C] * xe[2 + i];
            acc += clip8_fixed(hs) * ye[2 + j];                  // the horizontal pass's uint8 pixel of temporary row ymin + j
        }
        p.out[t * p.so_t + c * p.so_c + oy * p.so_h + ox * p.so_w] = (float)clip8_fixed(acc) / 255.f;   // to_tensor: uint8 -> float / 255
    }
}

// ------------------------------------------------------------------------------------------------------------
// Decoded frames -> the ANONYMIZER's input activation (dali_extraction.py:169-173, st_feature_extraction.py:24-26: every frame of every clip goes through fa
// as an RGB image): HybridValPipe's clip sampling as in crop_resize_tp_kernel, each frame / divisor -> crop -> resize (-> flip), written as the 16-bit
// channels-last rows tedspad_clip_to_channels_last gives the first conv of UnetPlusPlus (cpad 4: pixel pairs {c0 c1 c2 0 | c0 c1 c2 0}) or UNet (cpad 8:
// {c0 c1 c2 0 0 0 0 0}); the fp32 frame batch between the two is never written. One workgroup per (output frame, output row): vertical pass into an fp32 LDS
// row (aa_vpass, or for uint8 frames crop_resize_tp_kernel's four-bytes-per-load form of it on the same u8_px), horizontal pass (aa_hpass) rounded into a 16-bit
// LDS row, which leaves as 16-byte pieces on consecutive lanes. A source frame outside [0, T) is a zero frame: its rows are stored as zeros.
// ------------------------------------------------------------------------------------------------------------
struct ActOutKP {
    uint4 *act;                 // (frames, oh, ow * cpad / 8) 16-byte pieces
    int first, clip_step, frame_step, t_clip, cpad;
};

// the source frame of output frame fo, or -1 for a zero frame
__device__ __forceinline__ long act_src_frame(const ActOutKP &a, int fo, int T) {
    const long fr = (long)a.first + (long)(fo / a.t_clip) * a.clip_step + (long)(fo % a.t_clip) * a.frame_step;
    return fr >= 0 && fr < T ? fr : -1;
}

// row `orow` (= frame * oh + y) of the activation: `n16` 16-byte pieces from the LDS row, or zeros
__device__ __forceinline__ void act_store_row(const ActOutKP &a, long orow, int n16, const unsigned char *tile) {
    uint4 *dst = a.act + orow * n16;
    for (int i = threadIdx.x; i < n16; i += 256) dst[i] = tile ? reinterpret_cast<const uint4 *>(tile)[i] : make_uint4(0u, 0u, 0u, 0u);
}

template <typename In, typename T>
__global__ __launch_bounds__(256) void crop_resize_act_kernel(const ResizeKP p, const ActOutKP a, const uint8_t *in_end) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_act[];
    const int n16 = p.ow * a.cpad / 8;
    const int fo = blockIdx.x / p.oh, oy = blockIdx.x % p.oh;
    const long fr = act_src_frame(a, fo, p.T);
    if (fr < 0) {                                                    // uniform
        act_store_row(a, blockIdx.x, n16, nullptr);
        return;
    }
    const int span = p.cw * p.C;
    float *row = reinterpret_cast<float *>(lds_act + (size_t)n16 * 16);     // [span]
    float *lut = row + span;                                                // [256] (uint8 input, divisor != 255)
    const int32_t *ye = p.ytab + (size_t)oy * (2 + p.ytaps);
    const long rstride = (long)p.W * p.C;
    const In *base = (const In *)p.in + ((fr * p.H + p.y0 + ye[0]) * p.W + p.x0) * p.C;
    if constexpr (sizeof(In) == 1) {
        const bool div255 = p.div == 255.0f;
        const int yn = ye[1];
        const float *wy = (const float *)(ye + 2);
        if (!div255) {                                               // uniform
            lut[threadIdx.x] = (float)threadIdx.x / p.div;
            __syncthreads();
        }
        for (int g = threadIdx.x; 4 * g < span; g += 256) {          // four consecutive bytes per lane and load, as crop_resize_tp_kernel
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < yn; j++) {
                const unsigned w4 = load_u8x4(reinterpret_cast<const uint8_t *>(base) + j * rstride + 4 * g, in_end);
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] += wy[j] * u8_px((w4 >> (8 * k)) & 255u, div255, lut);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * g + k < span) row[4 * g + k] = acc[k];
        }
    } else {
        aa_vpass<In>(base, rstride, ye, span, p.div, row);
    }
    __syncthreads();
    for (int ox = threadIdx.x; ox < p.ow; ox += 256) {
        const int32_t *xe = p.xtab + (size_t)ox * (2 + p.xtaps);
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (c < p.C) v[c] = aa_hpass(row, xe, p.C, c);
        act_put_pixel<T>(lds_act, a.cpad, p.flip ? p.ow - 1 - ox : ox, v);
    }
    __syncthreads();
    act_store_row(a, blockIdx.x, n16, lds_act);
}

// The same for Pillow's resample (crop_resize_pil_kernel's arithmetic: a lane owns an output pixel and runs the horizontal pass of its temporary rows itself).
template <typename T>
__global__ __launch_bounds__(256) void crop_resize_pil_act_kernel(const ResizeU8KP p, const ActOutKP a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_act[];
    const int n16 = p.ow * a.cpad / 8;
    const int fo = blockIdx.x / p.oh, oy = blockIdx.x % p.oh;
    const long fr = act_src_frame(a, fo, p.T);
    if (fr < 0) {                                                    // uniform
        act_store_row(a, blockIdx.x, n16, nullptr);
        return;
    }
    const int32_t *ye = p.ytab + (size_t)oy * (2 + p.ytaps);
    const int ymin = ye[0], yn = ye[1];
    const uint8_t *base = p.in + ((fr * p.H + p.y0 + ymin) * p.W + p.x0) * p.C;
    const long rstride = (long)p.W * p.C;
    for (int ox = threadIdx.x; ox < p.ow; ox += 256) {
        const int32_t *xe = p.xtab + (size_t)ox * (2 + p.xtaps);
        const int xmin = xe[0], xn = xe[1];
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c >= p.C) continue;
            int acc = 1 << 21;
            for (int j = 0; j < yn; j++) {
                const uint8_t *r = base + j * rstride + (long)xmin * p.C + c;
                int hs = 1 << 21;
                for (int i = 0; i < xn; i++) hs += (int)r[(long)i * p.C] * xe[2 + i];
                acc += clip8_fixed(hs) * ye[2 + j];
            }
            v[c] = (float)clip8_fixed(acc) / 255.f;
        }
        act_put_pixel<T>(lds_act, a.cpad, ox, v);
    }
    __syncthreads();
    act_store_row(a, blockIdx.x, n16, lds_act);
}

// ------------------------------------------------------------------------------------------------------------
// process_feat + magnitude. One workgroup per (crop, segment); lanes stride over F (consecutive floats).
// length > 0 : out (ncrops, length, F+1): row s = mean of feature rows r[s]..r[s+1]-1 (or row r[s] if empty),
//              r = linspace(0, T, length+1) truncated to int exactly as numpy does it in float64.
// length == 0: test-mode layout out (T, ncrops, F+1): the rows themselves + magnitude.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void segment_pool_mag_kernel(const float *feat, float *out, int T, int ncrops, int F, int length) {
    __shared__ float red[256];
    const int seg = blockIdx.x, crop = blockIdx.y;
    int r0, r1;
    if (length > 0) {
        const double step = (double)T / (double)length;          // numpy.linspace: start + arange * step, last = stop
        r0 = (int)((double)seg * step);
        r1 = seg + 1 == length ? T : (int)((double)(seg + 1) * step);
    } else {
        r0 = seg;
        r1 = seg + 1;
    }
    float *o = length > 0 ? out + ((size_t)crop * length + seg) * (F + 1) : out + ((size_t)seg * ncrops + crop) * (F + 1);
    float ss = 0.f;
    for (int f = threadIdx.x; f < F; f += 256) {
        float v;
        if (r1 > r0) {
            float acc = 0.f;
            for (int r = r0; r < r1; r++) acc += feat[((size_t)r * ncrops + crop) * F + f];
            v = acc / (float)(r1 - r0);
        } else {
            v = feat[((size_t)r0 * ncrops + crop) * F + f];
        }
        o[f] = v;
        ss += v * v;
    }
    red[threadIdx.x] = ss;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) o[F] = sqrtf(red[0]);
}

}  // namespace
}  // namespace tedspad

using namespace tedspad;

extern "C" int32_t tedspad_resize_aa_taps(int32_t in_size, int32_t out_size) {
    if (in_size <= 0 || out_size <= 0) return 0;
    return aa_taps(in_size, out_size);
}

extern "C" int32_t tedspad_resize_aa_table(int32_t in_size, int32_t out_size, int32_t *table) {
    TS_REQUIRE(in_size > 0 && out_size > 0 && table, "tedspad_resize_aa_table: bad arguments");
    aa_table(in_size, out_size, table);
    return TEDSPAD_OK;
}

extern "C" int32_t tedspad_frames_crop_resize(const void *frames, int32_t in_is_float, int32_t T, int32_t H, int32_t W, int32_t C,
                                              int32_t y0, int32_t x0, int32_t ch, int32_t cw, int32_t oh, int32_t ow,
                                              const int32_t *ytab, const int32_t *xtab, float divisor, int32_t flip, float *out,
                                              int64_t so_t, int64_t so_c, int64_t so_h, int64_t so_w, void *stream) {
    TS_REQUIRE(frames && out && ytab && xtab, "tedspad_frames_crop_resize: null pointer");
    TS_REQUIRE(T > 0 && H > 0 && W > 0 && C > 0 && C <= 4 && oh > 0 && ow > 0, "tedspad_frames_crop_resize: bad sizes");
    TS_REQUIRE(y0 >= 0 && x0 >= 0 && ch > 0 && cw > 0 && y0 + ch <= H && x0 + cw <= W,
               "tedspad_frames_crop_resize: crop box (%d,%d,%d,%d) outside the %dx%d frame", y0, x0, ch, cw, H, W);
    TS_REQUIRE(divisor != 0.f, "tedspad_frames_crop_resize: divisor must be non-zero");
    const size_t lds = (size_t)cw * C * sizeof(float);
    TS_REQUIRE(lds <= 64 * 1024, "tedspad_frames_crop_resize: crop width %d x %d channels exceeds the 64 KB LDS row buffer", cw, C);
    ResizeKP p;
    p.in = frames; p.out = out; p.ytab = ytab; p.xtab = xtab;
    p.T = T; p.H = H; p.W = W; p.C = C; p.y0 = y0; p.x0 = x0; p.ch = ch; p.cw = cw; p.oh = oh; p.ow = ow;
    p.ytaps = aa_taps(ch, oh); p.xtaps = aa_taps(cw, ow); p.flip = flip; p.div = divisor;
    p.so_t = so_t; p.so_c = so_c; p.so_h = so_h; p.so_w = so_w;
    hipStream_t s = (hipStream_t)stream;
    const dim3 g((unsigned)((long)T * oh));
    if (in_is_float) hipLaunchKernelGGL(crop_resize_aa_kernel<float>, g, dim3(256), lds, s, p);
    else hipLaunchKernelGGL(crop_resize_aa_kernel<uint8_t>, g, dim3(256), lds, s, p);
    return check_launch("tedspad_frames_crop_resize");
}

extern "C" int32_t tedspad_frames_crop_resize_tp(const void *frames, int32_t in_is_float, int32_t T, int32_t H, int32_t W, int32_t C, int32_t n_clips,
                                                 int32_t first, int32_t clip_step, int32_t frame_step, int32_t t_clip, int32_t y0, int32_t x0, int32_t ch,
                                                 int32_t cw, int32_t oh, int32_t ow, const int32_t *ytab, const int32_t *xtab, float divisor, int32_t flip,
                                                 void *records, int32_t pad_t, int32_t stride_t, int32_t t_pairs, int32_t dtype, void *stream) {
    TS_REQUIRE(frames && records && ytab && xtab, "tedspad_frames_crop_resize_tp: null pointer");
    TS_REQUIRE(T > 0 && H > 0 && W > 0 && C > 0 && C <= 3 && oh > 0 && ow > 0 && ow % 2 == 0, "tedspad_frames_crop_resize_tp: bad sizes (<= 3 channels, even output width)");
    TS_REQUIRE(n_clips > 0 && t_clip > 0 && frame_step > 0 && clip_step >= 0, "tedspad_frames_crop_resize_tp: bad clip sampling");
    TS_REQUIRE(y0 >= 0 && x0 >= 0 && ch > 0 && cw > 0 && y0 + ch <= H && x0 + cw <= W,
               "tedspad_frames_crop_resize_tp: crop box (%d,%d,%d,%d) outside the %dx%d frame", y0, x0, ch, cw, H, W);
    TS_REQUIRE(divisor != 0.f, "tedspad_frames_crop_resize_tp: divisor must be non-zero");
    TS_REQUIRE(stride_t == 2 && pad_t >= 0 && t_pairs > 0, "tedspad_frames_crop_resize_tp: temporal stride 2 (tedspad_clip_to_tp's record layout)");
    TS_REQUIRE(dtype == TEDSPAD_F16 || dtype == TEDSPAD_BF16, "tedspad_frames_crop_resize_tp: bad dtype");
    TS_REQUIRE((uintptr_t)records % 16 == 0 && (long)n_clips * oh * (t_pairs + 1) < (1L << 31), "tedspad_frames_crop_resize_tp: records must be 16-byte aligned; too many rows");
    const size_t lds = (size_t)ow * 24 + (size_t)4 * cw * C * sizeof(float) + 1024 + (size_t)ow * (2 + aa_taps(cw, ow)) * 4;      // a row of half records + four frames' row buffers + the value table + the column table
    TS_REQUIRE(lds <= 160 * 1024, "tedspad_frames_crop_resize_tp: %d columns of records + four %d x %d row buffers exceed the CU's 160 KB of LDS", ow, cw, C);
    ResizeTpKP q;
    ResizeKP &p = q.r;
    p.in = frames; p.out = nullptr; p.ytab = ytab; p.xtab = xtab;
    p.T = T; p.H = H; p.W = W; p.C = C; p.y0 = y0; p.x0 = x0; p.ch = ch; p.cw = cw; p.oh = oh; p.ow = ow;
    p.ytaps = aa_taps(ch, oh); p.xtaps = aa_taps(cw, ow); p.flip = flip; p.div = divisor;
    p.so_t = p.so_c = p.so_h = p.so_w = 0;
    q.rec = (uint16_t *)records; q.n_clips = n_clips; q.first = first; q.clip_step = clip_step; q.frame_step = frame_step; q.t_clip = t_clip;
    q.pt = pad_t; q.stt = stride_t; q.tp_n = t_pairs;
    q.in_end = (const uint8_t *)frames + (size_t)T * H * W * C * (in_is_float ? 4 : 1);
    hipStream_t s = (hipStream_t)stream;
    const dim3 g((unsigned)((long)n_clips * oh * (t_pairs + 1)));
    const char *who = "tedspad_frames_crop_resize_tp";      // (wide source frames (HD) need more than the default 64 KB of dynamic LDS)
    if (in_is_float) TS_WITH_T(dtype, return launch_lds<crop_resize_tp_kernel<float, T>>(who, g, dim3(256), lds, s, q));
    TS_WITH_T(dtype, return launch_lds<crop_resize_tp_kernel<uint8_t, T>>(who, g, dim3(256), lds, s, q));
}

extern "C" int32_t tedspad_frames_ten_crop_tp(const void *frames, int32_t in_is_float, int32_t T, int32_t H, int32_t W, int32_t C, int32_t n_clips,
                                              int32_t first, int32_t clip_step, int32_t frame_step, int32_t t_clip, int32_t ch, int32_t cw, int32_t yc,
                                              int32_t xc, int32_t oh, int32_t ow, const int32_t *ytab, const int32_t *xtab, float divisor, void *records,
                                              int32_t pad_t, int32_t stride_t, int32_t t_pairs, int32_t dtype, void *stream) {
    TS_REQUIRE(frames && records && ytab && xtab, "tedspad_frames_ten_crop_tp: null pointer");
    TS_REQUIRE(T > 0 && H > 0 && W > 0 && C > 0 && C <= 3 && oh > 0 && ow > 0 && ow % 2 == 0, "tedspad_frames_ten_crop_tp: bad sizes (<= 3 channels, even output width)");
    TS_REQUIRE(n_clips > 0 && t_clip > 0 && frame_step > 0 && clip_step >= 0, "tedspad_frames_ten_crop_tp: bad clip sampling");
    TS_REQUIRE(ch > 0 && cw > 0 && ch <= H && cw <= W, "tedspad_frames_ten_crop_tp: crop %dx%d larger than the %dx%d frame", ch, cw, H, W);
    TS_REQUIRE(yc >= 0 && xc >= 0 && yc + ch <= H && xc + cw <= W,
               "tedspad_frames_ten_crop_tp: centre crop box (%d,%d,%d,%d) outside the %dx%d frame", yc, xc, ch, cw, H, W);
    TS_REQUIRE(divisor != 0.f, "tedspad_frames_ten_crop_tp: divisor must be non-zero");
    TS_REQUIRE(stride_t == 2 && pad_t >= 0 && t_pairs > 0, "tedspad_frames_ten_crop_tp: temporal stride 2 (tedspad_clip_to_tp's record layout)");
    TS_REQUIRE(dtype == TEDSPAD_F16 || dtype == TEDSPAD_BF16, "tedspad_frames_ten_crop_tp: bad dtype");
    const long nblk = 3L * n_clips * oh * (t_pairs + 1), per = 8L * (t_pairs + 1);      // (clip time, output row, row origin, frame quad)
    TS_REQUIRE((uintptr_t)records % 16 == 0 && nblk + per < (1L << 31), "tedspad_frames_ten_crop_tp: records must be 16-byte aligned; too many rows");
    // two rows of half records (one per column origin) + four frames' full-width row buffers + the value table
    const size_t lds = (size_t)ow * 48 + (size_t)4 * W * C * sizeof(float) + 1024;
    TS_REQUIRE(lds <= 160 * 1024, "tedspad_frames_ten_crop_tp: %d columns of records + four %d x %d row buffers exceed the CU's 160 KB of LDS", ow, W, C);
    TenCropKP kp;
    ResizeTpKP &q = kp.q;
    ResizeKP &p = q.r;
    p.in = frames; p.out = nullptr; p.ytab = ytab; p.xtab = xtab;
    p.T = T; p.H = H; p.W = W; p.C = C; p.y0 = 0; p.x0 = 0; p.ch = ch; p.cw = cw; p.oh = oh; p.ow = ow;
    p.ytaps = aa_taps(ch, oh); p.xtaps = aa_taps(cw, ow); p.flip = 0; p.div = divisor;
    p.so_t = p.so_c = p.so_h = p.so_w = 0;
    q.rec = (uint16_t *)records; q.n_clips = n_clips; q.first = first; q.clip_step = clip_step; q.frame_step = frame_step; q.t_clip = t_clip;
    q.pt = pad_t; q.stt = stride_t; q.tp_n = t_pairs;
    q.in_end = (const uint8_t *)frames + (size_t)T * H * W * C * (in_is_float ? 4 : 1);
    kp.yc = yc; kp.xc = xc;
    hipStream_t s = (hipStream_t)stream;
    kp.nblk = (int)nblk;
    const dim3 g((unsigned)((nblk + per - 1) / per * per));          // whole rounds of 8 x (t_pairs + 1) blocks: the kernel's block order
    const char *who = "tedspad_frames_ten_crop_tp";
    if (in_is_float) TS_WITH_T(dtype, return launch_lds<ten_crop_tp_kernel<float, T>>(who, g, dim3(256), lds, s, kp));
    TS_WITH_T(dtype, return launch_lds<ten_crop_tp_kernel<uint8_t, T>>(who, g, dim3(256), lds, s, kp));
}

// the checks the two activation entries share; fills the output description
static int32_t act_out_args(const char *who, int32_t T, int32_t H, int32_t W, int32_t C, int32_t n_clips, int32_t first, int32_t clip_step, int32_t frame_step,
                            int32_t t_clip, int32_t y0, int32_t x0, int32_t ch, int32_t cw, int32_t oh, int32_t ow, void *act, int32_t cpad, int32_t dtype, ActOutKP *a) {
    TS_REQUIRE(T > 0 && H > 0 && W > 0 && C > 0 && C <= 3 && oh > 0 && ow > 0, "%s: bad sizes (<= 3 channels)", who);
    TS_REQUIRE(n_clips > 0 && t_clip > 0 && frame_step > 0 && clip_step >= 0 && first >= 0, "%s: bad clip sampling", who);
    TS_REQUIRE(y0 >= 0 && x0 >= 0 && ch > 0 && cw > 0 && y0 + ch <= H && x0 + cw <= W, "%s: crop box (%d,%d,%d,%d) outside the %dx%d frame", who, y0, x0, ch, cw, H, W);
    TS_REQUIRE(cpad == 4 || cpad == 8, "%s: cpad must be 4 (pixel pairs) or 8", who);
    TS_REQUIRE(cpad == 8 || ow % 2 == 0, "%s: cpad=4 packs pixel pairs, the output width %d must be even", who, ow);
    TS_REQUIRE(dtype == TEDSPAD_F16 || dtype == TEDSPAD_BF16, "%s: bad dtype", who);
    TS_REQUIRE((uintptr_t)act % 16 == 0, "%s: the activation must be 16-byte aligned", who);
    TS_REQUIRE((long)n_clips * t_clip * oh < (1L << 31), "%s: %d clips x %d frames x %d rows do not fit one launch", who, n_clips, t_clip, oh);
    a->act = (uint4 *)act; a->first = first; a->clip_step = clip_step; a->frame_step = frame_step; a->t_clip = t_clip; a->cpad = cpad;
    return TEDSPAD_OK;
}

extern "C" int32_t tedspad_frames_crop_resize_act(const void *frames, int32_t in_is_float, int32_t T, int32_t H, int32_t W, int32_t C, int32_t n_clips,
                                                  int32_t first, int32_t clip_step, int32_t frame_step, int32_t t_clip, int32_t y0, int32_t x0, int32_t ch,
                                                  int32_t cw, int32_t oh, int32_t ow, const int32_t *ytab, const int32_t *xtab, float divisor, int32_t flip,
                                                  void *act, int32_t cpad, int32_t dtype, void *stream) {
    const char *who = "tedspad_frames_crop_resize_act";
    TS_REQUIRE(frames && act && ytab && xtab, "tedspad_frames_crop_resize_act: null pointer");
    TS_REQUIRE(divisor != 0.f, "tedspad_frames_crop_resize_act: divisor must be non-zero");
    ActOutKP a;
    const int32_t rc = act_out_args(who, T, H, W, C, n_clips, first, clip_step, frame_step, t_clip, y0, x0, ch, cw, oh, ow, act, cpad, dtype, &a);
    if (rc != TEDSPAD_OK) return rc;
    const size_t lds = (size_t)ow * cpad * 2 + (size_t)cw * C * sizeof(float) + 1024;       // the 16-bit output row + the fp32 row buffer + the value table
    TS_REQUIRE(lds <= 160 * 1024, "tedspad_frames_crop_resize_act: %d output columns + a %d x %d row buffer exceed the CU's 160 KB of LDS", ow, cw, C);
    ResizeKP p;
    p.in = frames; p.out = nullptr; p.ytab = ytab; p.xtab = xtab;
    p.T = T; p.H = H; p.W = W; p.C = C; p.y0 = y0; p.x0 = x0; p.ch = ch; p.cw = cw; p.oh = oh; p.ow = ow;
    p.ytaps = aa_taps(ch, oh); p.xtaps = aa_taps(cw, ow); p.flip = flip; p.div = divisor;
    p.so_t = p.so_c = p.so_h = p.so_w = 0;
    const uint8_t *in_end = (const uint8_t *)frames + (size_t)T * H * W * C * (in_is_float ? 4 : 1);
    hipStream_t s = (hipStream_t)stream;
    const dim3 g((unsigned)((long)n_clips * t_clip * oh));
    if (in_is_float) TS_WITH_T(dtype, return launch_lds<crop_resize_act_kernel<float, T>>(who, g, dim3(256), lds, s, p, a, in_end));
    TS_WITH_T(dtype, return launch_lds<crop_resize_act_kernel<uint8_t, T>>(who, g, dim3(256), lds, s, p, a, in_end));
}

extern "C" int32_t tedspad_frames_crop_resize_pil_act(const void *frames, int32_t T, int32_t H, int32_t W, int32_t C, int32_t n_clips, int32_t first,
                                                      int32_t clip_step, int32_t frame_step, int32_t t_clip, int32_t y0, int32_t x0, int32_t ch, int32_t cw,
                                                      int32_t oh, int32_t ow, const int32_t *ytab, int32_t ytaps, const int32_t *xtab, int32_t xtaps,
                                                      void *act, int32_t cpad, int32_t dtype, void *stream) {
    const char *who = "tedspad_frames_crop_resize_pil_act";
    TS_REQUIRE(frames && act && ytab && xtab && ytaps > 0 && xtaps > 0, "tedspad_frames_crop_resize_pil_act: bad arguments");
    ActOutKP a;
    const int32_t rc = act_out_args(who, T, H, W, C, n_clips, first, clip_step, frame_step, t_clip, y0, x0, ch, cw, oh, ow, act, cpad, dtype, &a);
    if (rc != TEDSPAD_OK) return rc;
    const size_t lds = (size_t)ow * cpad * 2;
    TS_REQUIRE(lds <= 160 * 1024, "tedspad_frames_crop_resize_pil_act: %d output columns exceed the CU's 160 KB of LDS", ow);
    ResizeU8KP p;
    p.in = (const uint8_t *)frames; p.out = nullptr; p.ytab = ytab; p.xtab = xtab;
    p.T = T; p.H = H; p.W = W; p.C = C; p.y0 = y0; p.x0 = x0; p.oh = oh; p.ow = ow; p.ytaps = ytaps; p.xtaps = xtaps;
    p.so_t = p.so_c = p.so_h = p.so_w = 0;
    const dim3 g((unsigned)((long)n_clips * t_clip * oh));
    TS_WITH_T(dtype, return launch_lds<crop_resize_pil_act_kernel<T>>(who, g, dim3(256), lds, (hipStream_t)stream, p, a));
}

extern "C" int32_t tedspad_segment_pool_mag(const float *feat, int32_t T, int32_t ncrops, int32_t F, int32_t length, float *out,
                                            void *stream) {
    TS_REQUIRE(feat && out && T > 0 && ncrops > 0 && F > 0 && length >= 0, "tedspad_segment_pool_mag: bad arguments");
    const dim3 g((unsigned)(length > 0 ? length : T), (unsigned)ncrops);
    hipLaunchKernelGGL(segment_pool_mag_kernel, g, dim3(256), 0, (hipStream_t)stream, feat, out, T, ncrops, F, length);
    return check_launch("tedspad_segment_pool_mag");
}

extern "C" int32_t tedspad_frames_crop_resize_pil(const void *frames, int32_t t, int32_t h, int32_t w, int32_t c, int32_t y0, int32_t x0, int32_t ch,
                                                  int32_t cw, int32_t oh, int32_t ow, const int32_t *ytab, int32_t ytaps, const int32_t *xtab,
                                                  int32_t xtaps, float *out, int64_t so_t, int64_t so_c, int64_t so_h, int64_t so_w, void *stream) {
    TS_REQUIRE(frames && ytab && xtab && out && t > 0 && h > 0 && w > 0 && c > 0 && c <= 4 && oh > 0 && ow > 0 && ytaps > 0 && xtaps > 0,
               "tedspad_frames_crop_resize_pil: bad arguments");
    TS_REQUIRE(y0 >= 0 && x0 >= 0 && ch > 0 && cw > 0 && y0 + ch <= h && x0 + cw <= w, "tedspad_frames_crop_resize_pil: crop box outside the frame");
    TS_REQUIRE((long)t * oh < (1L << 31), "tedspad_frames_crop_resize_pil: too many rows");
    ResizeU8KP p;
    p.in = (const uint8_t *)frames; p.out = out; p.ytab = ytab; p.xtab = xtab;
    p.T = t; p.H = h; p.W = w; p.C = c; p.y0 = y0; p.x0 = x0; p.oh = oh; p.ow = ow; p.ytaps = ytaps; p.xtaps = xtaps;
    p.so_t = so_t; p.so_c = so_c; p.so_h = so_h; p.so_w = so_w;
    hipLaunchKernelGGL(crop_resize_pil_kernel, dim3((unsigned)((long)t * oh)), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch("tedspad_frames_crop_resize_pil");
}
