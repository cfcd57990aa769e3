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

// the source frames, the crop box and the resize: what every antialiased kernel reads
struct ResizeSrc {
    const void *in;
    const int32_t *ytab, *xtab;
    int T, H, W, C;          // frames are (T, H, W, C) with C interleaved (DALI / decoder layout)
    int y0, x0, ch, cw;      // crop box
    int oh, ow, ytaps, xtaps;
    int flip;
    float div;               // 255: applied as a true division per sample, like `video / 255.`
};

// + the strided fp32 output of crop_resize_aa_kernel
struct ResizeKP : ResizeSrc {
    float *out;
    long so_t, so_c, so_h, so_w;
};

// Clip sampling (HybridValPipe, dali_extraction.py:62-73: sequence_length 16, stride 2, step 32): frame f of clip n is source frame
// first + n*clip_step + f*frame_step; frames past the end of the video are zero frames (pad_sequences), and so is every f outside [0, t_clip).
struct ClipKP {
    int first, clip_step, frame_step, t_clip;
};

// the one rule of the record and activation kernels: the source frame of frame f of clip n, or -1 for a zero frame
__device__ __forceinline__ long src_frame(const ClipKP &s, int n, int f, int T) {
    const long fr = (long)s.first + (long)n * s.clip_step + (long)f * s.frame_step;
    // one mask, no short circuit: a caller's `>= 0` then folds back into these four tests (with && it does not, and the record kernels' uint8 form loses 1.5 %)
    const bool in = (f >= 0) & (f < s.t_clip) & (fr >= 0) & (fr < T);
    return in ? fr : -1;
}

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

// byte / divisor of the kernels that load four bytes at a time (aa_vpass_frames: the record and activation kernels): for 255 without the division or a table --
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

// The two passes of the fp32-clip kernel, the form every other kernel is tested against bit for bit. The record and activation kernels below run the same sums
// for several frames at once through aa_vpass_frames and aa_hpass_rec: one source expression per value, so that they give the same bits among themselves.
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

// The FG frames of a record kernel's workgroup, frames f0 .. f0 + FG - 1 of clip n: live[ff] false for a zero frame (uniform), base[ff] its row y at column x.
template <int FG, typename In>
__device__ __forceinline__ void clip_frames(const ResizeSrc &p, const ClipKP &s, int n, int f0, int y, int x, const In *(&base)[FG], bool (&live)[FG]) {
#pragma unroll
    for (int ff = 0; ff < FG; ++ff) {
        const long fr = src_frame(s, n, f0 + ff, p.T);
        live[ff] = fr >= 0;
        base[ff] = (const In *)p.in + (((live[ff] ? fr : 0) * p.H + y) * p.W + x) * p.C;
    }
}

// Pass 1 of the record and activation kernels: FG frames at once (live[ff] false: a zero frame, its row is zeros) into the LDS rows rows[ff * pitch + e],
// e < span, of the input row span that starts at base[ff]. Every sum is aa_vpass's, rows in ascending order. Float frames: its expression on load_px. uint8
// frames: four consecutive bytes per lane and load (byte loads: 64 bytes per wave instruction) through u8_px, whose value table `lut` is filled here first
// when the divisor is not 255: one barrier, on a wave-uniform branch that the whole workgroup reaches. (Fill and barrier stay in one branch: split over
// caller and pass, the activation kernel's row weights arrive through vector loads instead of scalar ones and its launch took 0.9 % longer.)
template <int FG, typename In>
__device__ __forceinline__ void aa_vpass_frames(const In *const (&base)[FG], const bool (&live)[FG], long rstride, const int32_t *ye, int span, float div,
                                                const uint8_t *in_end, float *lut, float *rows, int pitch) {
    const int yn = ye[1];
    const float *wy = (const float *)(ye + 2);
    if constexpr (sizeof(In) == 1) {
        const bool div255 = div == 255.0f;
        if (!div255) {                                               // uniform
            lut[threadIdx.x] = (float)threadIdx.x / div;
            __syncthreads();
        }
        for (int g = threadIdx.x; 4 * g < span; g += 256) {
            float acc[FG][4];
#pragma unroll
            for (int ff = 0; ff < FG; ++ff)
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[ff][k] = 0.f;
            for (int j = 0; j < yn; j++) {
                unsigned w4[FG];
#pragma unroll
                for (int ff = 0; ff < FG; ++ff) w4[ff] = live[ff] ? load_u8x4(reinterpret_cast<const uint8_t *>(base[ff]) + j * rstride + 4 * g, in_end) : 0u;
#pragma unroll
                for (int ff = 0; ff < FG; ++ff)
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[ff][k] += wy[j] * u8_px((w4[ff] >> (8 * k)) & 255u, div255, lut);
            }
#pragma unroll
            for (int ff = 0; ff < FG; ++ff)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (4 * g + k < span) rows[ff * pitch + 4 * g + k] = acc[ff][k];
        }
    } else {
        for (int e = threadIdx.x; e < span; e += 256) {
            float acc[FG];
#pragma unroll
            for (int ff = 0; ff < FG; ++ff) acc[ff] = 0.f;
            for (int j = 0; j < yn; j++) {
#pragma unroll
                for (int ff = 0; ff < FG; ++ff) acc[ff] += wy[j] * (live[ff] ? load_px<In>(base[ff] + j * rstride + e, div) : 0.f);
            }
#pragma unroll
            for (int ff = 0; ff < FG; ++ff) rows[ff * pitch + e] = acc[ff];
        }
    }
}

// Pass 2 of the record kernels: aa_hpass for the FG frames x 3 channels of one output pixel at once -- a tap's weight is read once; every sum still runs over
// its taps in ascending order -- rounded into the pixel's half record `rec` (FG x 3 values; channels >= C are zero, a zero frame's slots keep the tile's zeros).
// `row`: column 0 of the crop box in frame 0's LDS row; `xe`: the pixel's table entry, in LDS or global memory as the caller keeps it.
template <int FG, typename T>
__device__ __forceinline__ void aa_hpass_rec(const float *row, int pitch, const int32_t *xe, int C, const bool (&live)[FG], uint16_t *rec) {
    const int xmin = xe[0], xn = xe[1];
    const float *wx = reinterpret_cast<const float *>(xe + 2);
    float acc[FG][3];
#pragma unroll
    for (int ff = 0; ff < FG; ++ff)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[ff][c] = 0.f;
    for (int j = 0; j < xn; j++) {
        const float wj = wx[j];
        const float *r = row + (xmin + j) * C;
#pragma unroll
        for (int ff = 0; ff < FG; ++ff)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (c < C) acc[ff][c] += wj * r[ff * pitch + c];
    }
#pragma unroll
    for (int ff = 0; ff < FG; ++ff) {
        if (!live[ff]) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) rec[ff * 3 + c] = c < C ? T::from_f32(acc[ff][c]) : (uint16_t)0;
    }
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
    ResizeSrc r;
    ClipKP s;
    uint16_t *rec;
    int pt, tp_n;               // the stem's temporal padding and this clip length's frame pairs (temporal stride 2: the entry checks it)
    const uint8_t *in_end;      // one past the last byte of the frame buffer (the 4-byte loads of the uint8 path stay inside it)
};

template <typename In, typename T>
__global__ __launch_bounds__(256) void crop_resize_tp_kernel(const ResizeTpKP q) {
    constexpr int FG = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_tp[];
    const ResizeSrc &p = q.r;
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
    for (int i = threadIdx.x; i < tile8; i += 256) tile[i] = make_uint2(0u, 0u);               // frames outside the clip, channels >= C
    for (int i = threadIdx.x; i < p.ow * (2 + p.xtaps); i += 256) xt[i] = p.xtab[i];
    const int32_t *ye = p.ytab + (size_t)oy * (2 + p.ytaps);
    uint16_t *t16 = reinterpret_cast<uint16_t *>(lds_tp);
    const In *base[FG];
    bool live[FG];                                                   // false: a zero frame, its slots stay zero
    clip_frames<FG, In>(p, q.s, n, f0, p.y0 + ye[0], p.x0, base, live);
    aa_vpass_frames<FG, In>(base, live, (long)p.W * p.C, ye, span, p.div, q.in_end, lut, rows, span);
    __syncthreads();                                                 // rows, the zeroed tile and the column table are complete
    for (int ox = threadIdx.x; ox < p.ow; ox += 256) {
        const int oxw = p.flip ? p.ow - 1 - ox : ox;
        aa_hpass_rec<FG, T>(rows, span, xt + ox * (2 + p.xtaps), p.C, live, t16 + ((size_t)((oxw & 1) * wq_n + (oxw >> 1))) * 12);
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
// order (pixel ox of the mirror = pixel ow - 1 - ox: the other plane, pair ow/2 - 1 - wq). The passes and the frame rule are crop_resize_tp_kernel's own
// (aa_vpass_frames, aa_hpass_rec, src_frame; only the LDS row pitch differs): every record has the bits of the ten launches it replaces.
// Block order: the quads of one (row, row origin) write the two halves of the same records, and the hardware deals consecutive blocks round-robin over the 8
// XCDs, each with an L2 of its own, so in hardware order the two halves of a cache line leave two L2s as two partial writes. The kernel numbers its work so that
// the tp_n + 1 quads of a row are blocks b, b + 8, ... : one XCD (as observed; a placement the result does not depend on), whose L2 joins the halves. That alone
// took the launch from 3.10 ms to 1.37 ms at 370 clips of 224 x 224; the column table read from global memory instead of a copy in LDS
// (27 KB, six workgroups per CU, instead of 33 KB, four) gave 1.24 ms.
struct TenCropKP {
    ResizeTpKP q;               // q.r's box is the centre crop's (preprocess.center_crop_box); the kernel has no use for q.r.flip
    int nblk;                   // (clip time, output row, row origin, quad) items; the grid is rounded up to a multiple of 8 * (tp_n + 1)
};

template <typename In, typename T>
__global__ __launch_bounds__(256) void ten_crop_tp_kernel(const TenCropKP kp) {
    constexpr int FG = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_tc[];
    const ResizeTpKP &q = kp.q;
    const ResizeSrc &p = q.r;
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
    const int y0 = grp == 0 ? 0 : grp == 1 ? p.y0 : p.H - p.ch;
    const int xa = grp == 1 ? p.x0 : 0, xb = p.W - p.cw - xa;        // column origins: of the direct crop, and of the box whose mirror is the flipped frame's crop
    const int x_lo = xa < xb ? xa : xb;
    const int ncol = xa == xb ? 1 : 2;
    const int span = ((xa < xb ? xb : xa) + p.cw - x_lo) * p.C;      // <= rbuf
    for (int i = threadIdx.x; i < ncol * tile8; i += 256) tile[i] = make_uint2(0u, 0u);
    const int32_t *ye = p.ytab + (size_t)oy * (2 + p.ytaps);
    const In *base[FG];
    bool live[FG];
    clip_frames<FG, In>(p, q.s, n, f0, y0 + ye[0], x_lo, base, live);
    aa_vpass_frames<FG, In>(base, live, (long)p.W * p.C, ye, span, p.div, q.in_end, lut, rows, rbuf);
    __syncthreads();
    for (int it = threadIdx.x; it < ncol * p.ow; it += 256) {        // (column origin, output pixel)
        const int col = it >= p.ow, ox = it - col * p.ow;
        aa_hpass_rec<FG, T>(rows + ((col ? xb : xa) - x_lo) * p.C, rbuf, xt + ox * (2 + p.xtaps), p.C, live,
                            reinterpret_cast<uint16_t *>(tile + col * tile8) + ((size_t)((ox & 1) * wq_n + (ox >> 1))) * 12);
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
struct ResizeU8Src {
    const uint8_t *in;
    const int32_t *ytab, *xtab;
    int T, H, W, C, y0, x0, oh, ow, ytaps, xtaps;
};

// + the strided fp32 output of crop_resize_pil_kernel
struct ResizeU8KP : ResizeU8Src {
    float *out;
    long so_t, so_c, so_h, so_w;
};

__device__ __forceinline__ int clip8_fixed(int v) {
    v >>= 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// Both 8-bit passes of one output pixel (x, c) of the output row with table entry `ye`, for the two Pillow kernels. `px`: channel c of the crop box's column 0
// in the row's first input row (ye[0]); `xe`: the table entry of x.
__device__ __forceinline__ float pil_px(const uint8_t *px, long rstride, int C, const int32_t *ye, const int32_t *xe) {
    const int yn = ye[1], xmin = xe[0], xn = xe[1];
    int acc = 1 << 21;
    for (int j = 0; j < yn; j++) {
        const uint8_t *r = px + j * rstride + (long)xmin * C;
        int hs = 1 << 21;
        for (int i = 0; i < xn; i++) hs += (int)r[(long)i * C] * xe[2 + i];
        acc += clip8_fixed(hs) * ye[2 + j];                      // the horizontal pass's uint8 pixel of temporary row ye[0] + j
    }
    return (float)clip8_fixed(acc) / 255.f;                      // to_tensor: uint8 -> float / 255
}

__global__ __launch_bounds__(256) void crop_resize_pil_kernel(const ResizeU8KP p) {
    const int t = blockIdx.x / p.oh, oy = blockIdx.x % p.oh;
    const int32_t *ye = p.ytab + (size_t)oy * (2 + p.ytaps);
    const uint8_t *base = p.in + (((long)t * p.H + p.y0 + ye[0]) * p.W + p.x0) * p.C;
    for (int e = threadIdx.x; e < p.ow * p.C; e += 256) {
        const int ox = e / p.C, c = e - ox * p.C;
        p.out[t * p.so_t + c * p.so_c + oy * p.so_h + ox * p.so_w] = pil_px(base + c, (long)p.W * p.C, p.C, ye, p.xtab + (size_t)ox * (2 + p.xtaps));
    }
}

// ------------------------------------------------------------------------------------------------------------
// Decoded frames -> the ANONYMIZER's input activation (dali_extraction.py:169-173, st_feature_extraction.py:24-26: every frame of every clip goes through fa
// as an RGB image): HybridValPipe's clip sampling as in crop_resize_tp_kernel, each frame / divisor -> crop -> resize (-> flip), written as the 16-bit
// channels-last rows tedspad_clip_to_channels_last gives the first conv of UnetPlusPlus (cpad 4: pixel pairs {c0 c1 c2 0 | c0 c1 c2 0}) or UNet (cpad 8:
// {c0 c1 c2 0 0 0 0 0}); the fp32 frame batch between the two is never written. One workgroup per (output frame, output row): vertical pass into an fp32 LDS
// row (aa_vpass_frames, the record kernels' vertical pass, at one frame), horizontal pass (aa_hpass) rounded into a 16-bit
// LDS row, which leaves as 16-byte pieces on consecutive lanes. A source frame outside [0, T) is a zero frame (src_frame): its rows are stored as zeros.
// ------------------------------------------------------------------------------------------------------------
struct ActOutKP {
    uint4 *act;                 // (frames, oh, ow * cpad / 8) 16-byte pieces
    ClipKP s;                   // output frame fo is frame fo % t_clip of clip fo / t_clip
    int cpad;
};

// row `orow` (= frame * oh + y) of the activation: `n16` 16-byte pieces from the LDS row, or zeros
__device__ __forceinline__ void act_store_row(const ActOutKP &a, long orow, int n16, const unsigned char *tile) {
    uint4 *dst = a.act + orow * n16;
    for (int i = threadIdx.x; i < n16; i += 256) dst[i] = tile ? reinterpret_cast<const uint4 *>(tile)[i] : make_uint4(0u, 0u, 0u, 0u);
}

template <typename In, typename T>
__global__ __launch_bounds__(256) void crop_resize_act_kernel(const ResizeSrc p, const ActOutKP a, const uint8_t *in_end) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_act[];
    const int n16 = p.ow * a.cpad / 8;
    const int fo = blockIdx.x / p.oh, oy = blockIdx.x % p.oh;
    const long fr = src_frame(a.s, fo / a.s.t_clip, fo % a.s.t_clip, p.T);
    if (fr < 0) {                                                    // uniform
        act_store_row(a, blockIdx.x, n16, nullptr);
        return;
    }
    const int span = p.cw * p.C;
    float *row = reinterpret_cast<float *>(lds_act + (size_t)n16 * 16);     // [span]
    float *lut = row + span;                                                // [256] (uint8 input, divisor != 255)
    const int32_t *ye = p.ytab + (size_t)oy * (2 + p.ytaps);
    const In *const base[1] = {(const In *)p.in + ((fr * p.H + p.y0 + ye[0]) * p.W + p.x0) * p.C};
    const bool live[1] = {true};
    aa_vpass_frames<1, In>(base, live, (long)p.W * p.C, ye, span, p.div, in_end, lut, row, span);
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

// The same for Pillow's resample (crop_resize_pil_kernel's pil_px: a lane owns an output pixel and runs the horizontal pass of its temporary rows itself).
template <typename T>
__global__ __launch_bounds__(256) void crop_resize_pil_act_kernel(const ResizeU8Src p, const ActOutKP a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_act[];
    const int n16 = p.ow * a.cpad / 8;
    const int fo = blockIdx.x / p.oh, oy = blockIdx.x % p.oh;
    const long fr = src_frame(a.s, fo / a.s.t_clip, fo % a.s.t_clip, p.T);
    if (fr < 0) {                                                    // uniform
        act_store_row(a, blockIdx.x, n16, nullptr);
        return;
    }
    const int32_t *ye = p.ytab + (size_t)oy * (2 + p.ytaps);
    const uint8_t *base = p.in + ((fr * p.H + p.y0 + ye[0]) * p.W + p.x0) * p.C;
    for (int ox = threadIdx.x; ox < p.ow; ox += 256) {
        const int32_t *xe = p.xtab + (size_t)ox * (2 + p.xtaps);
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (c < p.C) v[c] = pil_px(base + c, (long)p.W * p.C, p.C, ye, xe);
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

// The checks every frame entry shares: sizes, clip sampling, box inside the frame. Where entries differ the difference is an argument: `cmax`, the channels the
// output takes (4 in the fp32 forms, 3 in records and activations); `s`, null in the fp32 forms, which take every frame; `first_ge0`, which only the
// activation entries ask for (the record kernels give zero frames in front of the video).
static int32_t crop_args(const char *who, int32_t T, int32_t H, int32_t W, int32_t C, int32_t cmax, int32_t n_clips, const ClipKP *s, bool first_ge0, int32_t y0,
                         int32_t x0, int32_t ch, int32_t cw, int32_t oh, int32_t ow) {
    TS_REQUIRE(T > 0 && H > 0 && W > 0 && C > 0 && C <= cmax && oh > 0 && ow > 0, "%s: bad sizes (<= %d channels)", who, cmax);
    TS_REQUIRE(!s || (n_clips > 0 && s->t_clip > 0 && s->frame_step > 0 && s->clip_step >= 0 && (s->first >= 0 || !first_ge0)), "%s: bad clip sampling", who);
    TS_REQUIRE(y0 >= 0 && x0 >= 0 && ch > 0 && cw > 0 && y0 + ch <= H && x0 + cw <= W, "%s: crop box (%d,%d,%d,%d) outside the %dx%d frame", who, y0, x0, ch, cw, H, W);
    return TEDSPAD_OK;
}

// + what the four antialiased entries share; fills the source and geometry part of their kernel parameters
static int32_t aa_args(const char *who, const void *frames, const void *dst, const int32_t *ytab, const int32_t *xtab, int32_t T, int32_t H, int32_t W, int32_t C,
                       int32_t cmax, int32_t n_clips, const ClipKP *s, bool first_ge0, int32_t y0, int32_t x0, int32_t ch, int32_t cw, int32_t oh, int32_t ow,
                       float divisor, int32_t flip, ResizeSrc *p) {
    TS_REQUIRE(frames && dst && ytab && xtab, "%s: null pointer", who);
    const int32_t rc = crop_args(who, T, H, W, C, cmax, n_clips, s, first_ge0, y0, x0, ch, cw, oh, ow);
    if (rc != TEDSPAD_OK) return rc;
    TS_REQUIRE(divisor != 0.f, "%s: divisor must be non-zero", who);
    p->in = frames; p->ytab = ytab; p->xtab = xtab;
    p->T = T; p->H = H; p->W = W; p->C = C; p->y0 = y0; p->x0 = x0; p->ch = ch; p->cw = cw; p->oh = oh; p->ow = ow;
    p->ytaps = aa_taps(ch, oh); p->xtaps = aa_taps(cw, ow); p->flip = flip; p->div = divisor;
    return TEDSPAD_OK;
}

// + what the two Pillow entries share (their tables come with their tap counts: preprocess.pil_table)
static int32_t pil_args(const char *who, const void *frames, const void *dst, const int32_t *ytab, int32_t ytaps, const int32_t *xtab, int32_t xtaps, int32_t T,
                        int32_t H, int32_t W, int32_t C, int32_t cmax, int32_t n_clips, const ClipKP *s, int32_t y0, int32_t x0, int32_t ch, int32_t cw, int32_t oh,
                        int32_t ow, ResizeU8Src *p) {
    TS_REQUIRE(frames && dst && ytab && xtab && ytaps > 0 && xtaps > 0, "%s: bad arguments", who);
    const int32_t rc = crop_args(who, T, H, W, C, cmax, n_clips, s, true, y0, x0, ch, cw, oh, ow);
    if (rc != TEDSPAD_OK) return rc;
    p->in = (const uint8_t *)frames; p->ytab = ytab; p->xtab = xtab;
    p->T = T; p->H = H; p->W = W; p->C = C; p->y0 = y0; p->x0 = x0; p->oh = oh; p->ow = ow; p->ytaps = ytaps; p->xtaps = xtaps;
    return TEDSPAD_OK;
}

// what the two record entries add: pixel pairs, the stem's temporal geometry, the storage type, alignment, and `blocks` workgroups numbered in 32 bits
static int32_t rec_args(const char *who, int32_t in_is_float, void *records, int32_t pad_t, int32_t stride_t, int32_t t_pairs, int32_t dtype, long blocks,
                        ResizeTpKP *q) {
    const ResizeSrc &p = q->r;
    TS_REQUIRE(p.ow % 2 == 0, "%s: a record line holds pixel pairs, the output width %d must be even", who, p.ow);
    TS_REQUIRE(stride_t == 2 && pad_t >= 0 && t_pairs > 0, "%s: temporal stride 2 (tedspad_clip_to_tp's record layout)", who);
    TS_REQUIRE(dtype == TEDSPAD_F16 || dtype == TEDSPAD_BF16, "%s: bad dtype", who);
    TS_REQUIRE((uintptr_t)records % 16 == 0 && blocks < (1L << 31), "%s: records must be 16-byte aligned; too many rows", who);
    q->rec = (uint16_t *)records; q->pt = pad_t; q->tp_n = t_pairs;
    q->in_end = (const uint8_t *)p.in + (size_t)p.T * p.H * p.W * p.C * (in_is_float ? 4 : 1);
    return TEDSPAD_OK;
}

extern "C" int32_t tedspad_frames_crop_resize(const void *frames, int32_t in_is_float, int32_t T, int32_t H, int32_t W, int32_t C,
                                              int32_t y0, int32_t x0, int32_t ch, int32_t cw, int32_t oh, int32_t ow,
                                              const int32_t *ytab, const int32_t *xtab, float divisor, int32_t flip, float *out,
                                              int64_t so_t, int64_t so_c, int64_t so_h, int64_t so_w, void *stream) {
    const char *who = "tedspad_frames_crop_resize";
    ResizeKP p;
    const int32_t rc = aa_args(who, frames, out, ytab, xtab, T, H, W, C, 4, 0, nullptr, false, y0, x0, ch, cw, oh, ow, divisor, flip, &p);
    if (rc != TEDSPAD_OK) return rc;
    TS_REQUIRE((long)T * oh < (1L << 31), "tedspad_frames_crop_resize: %d frames x %d rows do not fit one launch", T, oh);
    const size_t lds = (size_t)cw * C * sizeof(float);
    TS_REQUIRE(lds <= 64 * 1024, "tedspad_frames_crop_resize: crop width %d x %d channels exceeds the 64 KB LDS row buffer", cw, C);
    p.out = out; p.so_t = so_t; p.so_c = so_c; p.so_h = so_h; p.so_w = so_w;
    hipStream_t s = (hipStream_t)stream;
    const dim3 g((unsigned)((long)T * oh));
    if (in_is_float) hipLaunchKernelGGL(crop_resize_aa_kernel<float>, g, dim3(256), lds, s, p);
    else hipLaunchKernelGGL(crop_resize_aa_kernel<uint8_t>, g, dim3(256), lds, s, p);
    return check_launch(who);
}

extern "C" int32_t tedspad_frames_crop_resize_tp(const void *frames, int32_t in_is_float, int32_t T, int32_t H, int32_t W, int32_t C, int32_t n_clips,
                                                 int32_t first, int32_t clip_step, int32_t frame_step, int32_t t_clip, int32_t y0, int32_t x0, int32_t ch,
                                                 int32_t cw, int32_t oh, int32_t ow, const int32_t *ytab, const int32_t *xtab, float divisor, int32_t flip,
                                                 void *records, int32_t pad_t, int32_t stride_t, int32_t t_pairs, int32_t dtype, void *stream) {
    const char *who = "tedspad_frames_crop_resize_tp";
    ResizeTpKP q;
    q.s = {first, clip_step, frame_step, t_clip};
    int32_t rc = aa_args(who, frames, records, ytab, xtab, T, H, W, C, 3, n_clips, &q.s, false, y0, x0, ch, cw, oh, ow, divisor, flip, &q.r);
    if (rc == TEDSPAD_OK) rc = rec_args(who, in_is_float, records, pad_t, stride_t, t_pairs, dtype, (long)n_clips * oh * (t_pairs + 1), &q);
    if (rc != TEDSPAD_OK) return rc;
    const size_t lds = (size_t)ow * 24 + (size_t)4 * cw * C * sizeof(float) + 1024 + (size_t)ow * (2 + aa_taps(cw, ow)) * 4;      // a row of half records + four frames' row buffers + the value table + the column table
    TS_REQUIRE(lds <= 160 * 1024, "tedspad_frames_crop_resize_tp: %d columns of records + four %d x %d row buffers exceed the CU's 160 KB of LDS", ow, cw, C);
    hipStream_t s = (hipStream_t)stream;
    const dim3 g((unsigned)((long)n_clips * oh * (t_pairs + 1)));
    // (wide source frames (HD) need more than the default 64 KB of dynamic LDS: launch_lds)
    if (in_is_float) TS_WITH_T(dtype, return launch_lds<crop_resize_tp_kernel<float, T>>(who, g, dim3(256), lds, s, q));
    TS_WITH_T(dtype, return launch_lds<crop_resize_tp_kernel<uint8_t, T>>(who, g, dim3(256), lds, s, q));
}

extern "C" int32_t tedspad_frames_ten_crop_tp(const void *frames, int32_t in_is_float, int32_t T, int32_t H, int32_t W, int32_t C, int32_t n_clips,
                                              int32_t first, int32_t clip_step, int32_t frame_step, int32_t t_clip, int32_t ch, int32_t cw, int32_t yc,
                                              int32_t xc, int32_t oh, int32_t ow, const int32_t *ytab, const int32_t *xtab, float divisor, void *records,
                                              int32_t pad_t, int32_t stride_t, int32_t t_pairs, int32_t dtype, void *stream) {
    const char *who = "tedspad_frames_ten_crop_tp";
    TS_REQUIRE(ch > 0 && cw > 0 && ch <= H && cw <= W, "tedspad_frames_ten_crop_tp: crop %dx%d larger than the %dx%d frame", ch, cw, H, W);
    TenCropKP kp;
    ResizeTpKP &q = kp.q;
    q.s = {first, clip_step, frame_step, t_clip};
    const long nblk = 3L * n_clips * oh * (t_pairs + 1), per = 8L * (t_pairs + 1);      // (clip time, output row, row origin, frame quad)
    // the box of the shared checks and of the kernel parameters is the centre crop's; the corner boxes are inside the frame when the crop is no larger than it
    int32_t rc = aa_args(who, frames, records, ytab, xtab, T, H, W, C, 3, n_clips, &q.s, false, yc, xc, ch, cw, oh, ow, divisor, 0, &q.r);
    if (rc == TEDSPAD_OK) rc = rec_args(who, in_is_float, records, pad_t, stride_t, t_pairs, dtype, nblk + per, &q);
    if (rc != TEDSPAD_OK) return rc;
    // two rows of half records (one per column origin) + four frames' full-width row buffers + the value table
    const size_t lds = (size_t)ow * 48 + (size_t)4 * W * C * sizeof(float) + 1024;
    TS_REQUIRE(lds <= 160 * 1024, "tedspad_frames_ten_crop_tp: %d columns of records + four %d x %d row buffers exceed the CU's 160 KB of LDS", ow, W, C);
    hipStream_t s = (hipStream_t)stream;
    kp.nblk = (int)nblk;
    const dim3 g((unsigned)((nblk + per - 1) / per * per));          // whole rounds of 8 x (t_pairs + 1) blocks: the kernel's block order
    if (in_is_float) TS_WITH_T(dtype, return launch_lds<ten_crop_tp_kernel<float, T>>(who, g, dim3(256), lds, s, kp));
    TS_WITH_T(dtype, return launch_lds<ten_crop_tp_kernel<uint8_t, T>>(who, g, dim3(256), lds, s, kp));
}

// what the two activation entries add; fills the rest of the output description (a->s is the entry's)
static int32_t act_out_args(const char *who, int32_t n_clips, int32_t oh, int32_t ow, void *act, int32_t cpad, int32_t dtype, ActOutKP *a) {
    TS_REQUIRE(cpad == 4 || cpad == 8, "%s: cpad must be 4 (pixel pairs) or 8", who);
    TS_REQUIRE(cpad == 8 || ow % 2 == 0, "%s: cpad=4 packs pixel pairs, the output width %d must be even", who, ow);
    TS_REQUIRE(dtype == TEDSPAD_F16 || dtype == TEDSPAD_BF16, "%s: bad dtype", who);
    TS_REQUIRE((uintptr_t)act % 16 == 0, "%s: the activation must be 16-byte aligned", who);
    TS_REQUIRE((long)n_clips * a->s.t_clip * oh < (1L << 31), "%s: %d clips x %d frames x %d rows do not fit one launch", who, n_clips, a->s.t_clip, oh);
    a->act = (uint4 *)act; a->cpad = cpad;
    return TEDSPAD_OK;
}

extern "C" int32_t tedspad_frames_crop_resize_act(const void *frames, int32_t in_is_float, int32_t T, int32_t H, int32_t W, int32_t C, int32_t n_clips,
                                                  int32_t first, int32_t clip_step, int32_t frame_step, int32_t t_clip, int32_t y0, int32_t x0, int32_t ch,
                                                  int32_t cw, int32_t oh, int32_t ow, const int32_t *ytab, const int32_t *xtab, float divisor, int32_t flip,
                                                  void *act, int32_t cpad, int32_t dtype, void *stream) {
    const char *who = "tedspad_frames_crop_resize_act";
    ResizeSrc p;
    ActOutKP a;
    a.s = {first, clip_step, frame_step, t_clip};
    int32_t rc = aa_args(who, frames, act, ytab, xtab, T, H, W, C, 3, n_clips, &a.s, true, y0, x0, ch, cw, oh, ow, divisor, flip, &p);
    if (rc == TEDSPAD_OK) rc = act_out_args(who, n_clips, oh, ow, act, cpad, dtype, &a);
    if (rc != TEDSPAD_OK) return rc;
    const size_t lds = (size_t)ow * cpad * 2 + (size_t)cw * C * sizeof(float) + 1024;       // the 16-bit output row + the fp32 row buffer + the value table
    TS_REQUIRE(lds <= 160 * 1024, "tedspad_frames_crop_resize_act: %d output columns + a %d x %d row buffer exceed the CU's 160 KB of LDS", ow, cw, C);
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
    ResizeU8Src p;
    ActOutKP a;
    a.s = {first, clip_step, frame_step, t_clip};
    int32_t rc = pil_args(who, frames, act, ytab, ytaps, xtab, xtaps, T, H, W, C, 3, n_clips, &a.s, y0, x0, ch, cw, oh, ow, &p);
    if (rc == TEDSPAD_OK) rc = act_out_args(who, n_clips, oh, ow, act, cpad, dtype, &a);
    if (rc != TEDSPAD_OK) return rc;
    const size_t lds = (size_t)ow * cpad * 2;
    TS_REQUIRE(lds <= 160 * 1024, "tedspad_frames_crop_resize_pil_act: %d output columns exceed the CU's 160 KB of LDS", ow);
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
    const char *who = "tedspad_frames_crop_resize_pil";
    ResizeU8KP p;
    const int32_t rc = pil_args(who, frames, out, ytab, ytaps, xtab, xtaps, t, h, w, c, 4, 0, nullptr, y0, x0, ch, cw, oh, ow, &p);
    if (rc != TEDSPAD_OK) return rc;
    TS_REQUIRE((long)t * oh < (1L << 31), "tedspad_frames_crop_resize_pil: too many rows");
    p.out = out; p.so_t = so_t; p.so_c = so_c; p.so_h = so_h; p.so_w = so_w;
    hipLaunchKernelGGL(crop_resize_pil_kernel, dim3((unsigned)((long)t * oh)), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch(who);
}
