// The training loaders' frame augmentation on the device, for gfx950 (aux_code/ucf101_dl.py: contrastive_train_dataloader.augmentation :596-630,
// weak_augmentation :632-642, single_train_dataloader.augmentation :149-183). The reference turns every frame into a PIL image, so the whole chain is 8-bit
// integer / fixed-point / single-rounding fp32 arithmetic and this kernel gives Pillow's bytes:
//   resized_crop  Image.crop (zeros right of / below the frame) + Image.resize(BILINEAR): libImaging/Resample.c, horizontal pass rounded to uint8, then the
//                 vertical pass, 22-bit coefficients, clip8((2^21 + sum px * kk) >> 22)                       (the arithmetic of feed.hip's crop_resize_pil_kernel)
//   contrast / saturation / brightness   ImageEnhance: Image.blend(degenerate, image, factor), libImaging/Blend.c: (float)d + a * (float)(p - d), one multiply
//                 and one add, truncated (clamped first when a is outside [0, 1]); degenerate = mean luma (int(mean + 0.5)) / luma / 0
//   hue           RGB -> HSV -> h += offset (mod 256) -> RGB, libImaging/Convert.c rgb2hsv_row / hsv2rgb
//   grayscale     L = (R*19595 + G*38470 + B*7471 + 0x8000) >> 16 in all three channels; adjust_gamma = a 256-entry point() table (built on the host)
//   hflip, to_tensor (byte / 255.f), erase (zero boxes, after the flip)
// One workgroup of 1024 threads per output frame; the resized uint8 frame lives in LDS as three planes (150 528 B at 224 x 224, 37 632 B at 112 x 112), the
// colour chain runs on it in place, and the planes leave as coalesced fp32 rows. Contrast needs the mean luma of the whole frame: an integer sum through one LDS
// counter (order-independent, hence deterministic).
//
// build.py compiles with -ffp-contract=fast; a fused multiply-add changes Pillow's bytes (929 of the 65 536 (degenerate, pixel) pairs at factor 1.1). The
// pragma below stops the front end from contracting, but under that flag the gfx950 back end still fuses a multiply with the add behind it (v_fma_f32 in the
// blend, seen in the ISA and as wrong bytes), so every product that feeds an addition goes through aug_mul, which hides it from the combiner.
#pragma clang fp contract(off)
#include <math.h>

#include "common.h"

namespace tedspad {
namespace {

constexpr int AUG_THREADS = 1024;
constexpr size_t AUG_LDS_MAX = 3 * 224 * 224;       // the frame planes: 150 528 of the CU's 163 840 bytes
constexpr int AUG_LDS_HEAD = 16;                    // the two luma sums in front of them

struct AugKP {
    const tedspad_augment_record *rec;
    const int32_t *tables;
    const uint8_t *luts;
    float *out;
    int oh, ow;
    long so_c, so_h, so_w;
};

__device__ __forceinline__ int aug_clip8_fixed(int v) {
    v >>= 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__device__ __forceinline__ int aug_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ __forceinline__ int aug_luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// one IEEE multiply whose result no later addition can be fused with
__device__ __forceinline__ float aug_mul(float a, float b) {
    float m = a * b;
    asm volatile("" : "+v"(m));
    return m;
}

// libImaging/Blend.c for one byte: d = the degenerate image's byte, p = the image's
__device__ __forceinline__ int aug_blend(int d, int p, float a, bool inside) {
    const float t = (float)d + aug_mul(a, (float)(p - d));
    if (inside) return (int)t & 255;
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

// libImaging/Convert.c rgb2hsv_row -> h + off (mod 256) -> hsv2rgb
__device__ __forceinline__ void aug_hue(int &r, int &g, int &b, int off) {
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    int uh = 0, us = 0;
    const int v = maxc;
    if (maxc != minc) {
        const float cr = (float)(maxc - minc);
        const float s = cr / (float)maxc;
        const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
        float h;
        if (r == maxc) h = bc - gc;
        else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
        else h = (float)(4.0 + (double)gc - (double)rc);
        double hd = (double)h / 6.0 + 1.0;          // in (0.8, 1.9): fmod(hd, 1.0) is hd or hd - 1, both exact
        if (hd >= 1.0) hd -= 1.0;
        h = (float)hd;
        uh = aug_clip8((int)((double)h * 255.0));
        us = aug_clip8((int)((double)s * 255.0));
    }
    uh = (uh + off) & 255;
    if (us == 0) {
        r = g = b = v;
        return;
    }
    const float h6 = (float)uh * 6.0f / 255.0f;
    const int i = (int)floorf(h6);
    const float f = h6 - (float)i;
    const float fs = (float)us / 255.0f;
    const float fv = (float)v;
    // (the outer products too: roundf subtracts its argument's integer part, which would otherwise be fused with the product)
    const int p = aug_clip8((int)roundf(aug_mul(fv, 1.0f - fs)));
    const int q = aug_clip8((int)roundf(aug_mul(fv, 1.0f - aug_mul(fs, f))));
    const int t = aug_clip8((int)roundf(aug_mul(fv, 1.0f - aug_mul(fs, 1.0f - f))));
    switch (i % 6) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
    }
}

// int(mean + 0.5) of n luma bytes with sum s, in integers
__device__ __forceinline__ int aug_mean(unsigned s, int n) { return (int)((2ul * s + (unsigned long)n) / (2ul * (unsigned long)n)); }

__global__ __launch_bounds__(AUG_THREADS) void clip_augment_kernel(const AugKP p) {
    // all of the LDS is dynamic (launch.h raises the dynamic limit to the CU's 160 KB: static LDS beside it would not fit the attribute)
    extern __shared__ __attribute__((aligned(16))) uint8_t aug_lds[];
    unsigned *lsum = reinterpret_cast<unsigned *>(aug_lds);               // the two luma sums
    uint8_t *aug_px = aug_lds + AUG_LDS_HEAD;                             // [3][oh][ow]
    const tedspad_augment_record &R = p.rec[blockIdx.x];
    const int oh = p.oh, ow = p.ow, npix = oh * ow;
    const int tid = threadIdx.x;
    const int flags = R.flags;
    if (tid < 2) lsum[tid] = 0u;

    // 1. crop + Pillow resample: thread = one (pixel, channel) of the output, interleaved so that a wave reads consecutive source bytes. Like
    // crop_resize_pil_kernel every thread runs the horizontal pass of the temporary rows it needs itself.
    {
        const int32_t *ytab = p.tables + R.ytab, *xtab = p.tables + R.xtab;
        const int H = R.H, W = R.W, top = R.top, left = R.left;
        const bool rev = flags & TEDSPAD_AUG_REVERSE;
        for (int e = tid; e < npix * 3; e += AUG_THREADS) {
            const int pix = e / 3, c = e - pix * 3;
            const int oy = pix / ow, ox = pix - oy * ow;
            const int32_t *ye = ytab + (long)oy * (2 + R.ytaps), *xe = xtab + (long)ox * (2 + R.xtaps);
            const int ymin = ye[0], yn = ye[1], xmin = xe[0], xn = xe[1];
            const int sc = rev ? 2 - c : c;
            int acc = 1 << 21;
            for (int j = 0; j < yn; j++) {
                const int sy = top + ymin + j;
                int hs = 1 << 21;
                if (sy < H) {                       // rows below the frame are zeros
                    const uint8_t *row = R.src + ((long)sy * W) * 3 + sc;
                    for (int i = 0; i < xn; i++) {
                        const int sx = left + xmin + i;
                        if (sx < W) hs += (int)row[(long)sx * 3] * xe[2 + i];
                    }
                }
                acc += aug_clip8_fixed(hs) * ye[2 + j];
            }
            aug_px[c * npix + pix] = (uint8_t)aug_clip8_fixed(acc);
        }
    }
    __syncthreads();

    uint8_t *pr = aug_px, *pg = aug_px + npix, *pb = aug_px + 2 * npix;
    const int colour = TEDSPAD_AUG_CONTRAST_FIRST | TEDSPAD_AUG_HUE | TEDSPAD_AUG_SATURATION | TEDSPAD_AUG_BRIGHTNESS | TEDSPAD_AUG_CONTRAST_LATE |
                       TEDSPAD_AUG_GRAY;
    if (flags & colour) {                           // (uniform)
        const float ac = R.contrast, as = R.saturation, ab = R.brightness;
        const bool ic = ac >= 0.f && ac <= 1.f, is = as >= 0.f && as <= 1.f, ib = ab >= 0.f && ab <= 1.f;
        const uint8_t *lut = p.luts + (long)R.gamma_lut * 256;
        // 2a. mean luma for a contrast in first position
        int mean0 = 0;
        if (flags & TEDSPAD_AUG_CONTRAST_FIRST) {
            unsigned s = 0;
            for (int i = tid; i < npix; i += AUG_THREADS) s += (unsigned)aug_luma(pr[i], pg[i], pb[i]);
            atomicAdd(&lsum[0], s);
            __syncthreads();
            mean0 = aug_mean(lsum[0], npix);
        }
        // 2b. contrast, hue, saturation, brightness; then grayscale + gamma unless a late contrast has to see the whole frame first
        const bool late = flags & TEDSPAD_AUG_CONTRAST_LATE;
        unsigned s1 = 0;
        for (int i = tid; i < npix; i += AUG_THREADS) {
            int r = pr[i], g = pg[i], b = pb[i];
            if (flags & TEDSPAD_AUG_CONTRAST_FIRST) {
                r = aug_blend(mean0, r, ac, ic);
                g = aug_blend(mean0, g, ac, ic);
                b = aug_blend(mean0, b, ac, ic);
            }
            if (flags & TEDSPAD_AUG_HUE) aug_hue(r, g, b, R.hue_off);
            if (flags & TEDSPAD_AUG_SATURATION) {
                const int l = aug_luma(r, g, b);
                r = aug_blend(l, r, as, is);
                g = aug_blend(l, g, as, is);
                b = aug_blend(l, b, as, is);
            }
            if (flags & TEDSPAD_AUG_BRIGHTNESS) {
                r = aug_blend(0, r, ab, ib);
                g = aug_blend(0, g, ab, ib);
                b = aug_blend(0, b, ab, ib);
            }
            if (late) {
                s1 += (unsigned)aug_luma(r, g, b);
            } else if (flags & TEDSPAD_AUG_GRAY) {
                int l = aug_luma(r, g, b);
                if (flags & TEDSPAD_AUG_GAMMA) l = lut[l];
                r = g = b = l;
            }
            pr[i] = (uint8_t)r;
            pg[i] = (uint8_t)g;
            pb[i] = (uint8_t)b;
        }
        // 2c. the late contrast and what follows it (a thread meets the pixels it wrote itself)
        if (late) {
            atomicAdd(&lsum[1], s1);
            __syncthreads();
            const int mean1 = aug_mean(lsum[1], npix);
            for (int i = tid; i < npix; i += AUG_THREADS) {
                int r = aug_blend(mean1, pr[i], ac, ic), g = aug_blend(mean1, pg[i], ac, ic), b = aug_blend(mean1, pb[i], ac, ic);
                if (flags & TEDSPAD_AUG_GRAY) {
                    int l = aug_luma(r, g, b);
                    if (flags & TEDSPAD_AUG_GAMMA) l = lut[l];
                    r = g = b = l;
                }
                pr[i] = (uint8_t)r;
                pg[i] = (uint8_t)g;
                pb[i] = (uint8_t)b;
            }
        }
        __syncthreads();
    }

    // 3. hflip, to_tensor, erase: consecutive lanes write consecutive floats of an output row
    const bool flip = flags & TEDSPAD_AUG_HFLIP;
    const int e0i = R.erase[0], e0j = R.erase[1], e0h = R.erase[2], e0w = R.erase[3];
    const int e1i = R.erase[4], e1j = R.erase[5], e1h = R.erase[6], e1w = R.erase[7];
    float *out = p.out + R.dst;
    for (int e = tid; e < npix * 3; e += AUG_THREADS) {
        const int c = e / npix, pix = e - c * npix;
        const int oy = pix / ow, ox = pix - oy * ow;
        int v = aug_px[c * npix + oy * ow + (flip ? ow - 1 - ox : ox)];
        if (oy >= e0i && oy - e0i < e0h && ox >= e0j && ox - e0j < e0w) v = 0;
        if (oy >= e1i && oy - e1i < e1h && ox >= e1j && ox - e1j < e1w) v = 0;
        out[c * p.so_c + oy * p.so_h + ox * p.so_w] = (float)v / 255.f;
    }
}

// a table of `n` rows of (2 + taps) words for an input of `in` samples: every row's window inside the input
bool aug_table_ok(const int32_t *tables, long words, long off, int taps, int n, int in) {
    if (off < 0 || taps < 1 || off + (long)n * (2 + taps) > words) return false;
    for (int i = 0; i < n; i++) {
        const int32_t *e = tables + off + (long)i * (2 + taps);
        if (e[0] < 0 || e[1] < 0 || e[1] > taps || (long)e[0] + e[1] > in) return false;
    }
    return true;
}

}  // namespace
}  // namespace tedspad

using namespace tedspad;

extern "C" int32_t tedspad_clip_augment(const void *blob_host, void *blob_dev, int64_t blob_bytes, int32_t nrec, int64_t tables_off, int64_t table_words,
                                        int64_t luts_off, int32_t nluts, float *out, int64_t out_elems, int32_t oh, int32_t ow, int64_t so_c, int64_t so_h,
                                        int64_t so_w, void *stream) {
    const char *who = "tedspad_clip_augment";
    static_assert(sizeof(tedspad_augment_record) == 112, "tedspad_augment_record layout (ted_spad_amd/augment.py RECORD)");
    TS_REQUIRE(blob_host && blob_dev && out, "%s: null pointer", who);
    TS_REQUIRE((uintptr_t)blob_dev % 8 == 0 && (uintptr_t)blob_host % 8 == 0, "%s: the record table must be 8-byte aligned", who);
    TS_REQUIRE(nrec > 0 && oh > 0 && ow > 0 && oh < 32768 && ow < 32768, "%s: bad sizes", who);
    if ((size_t)3 * oh * ow > AUG_LDS_MAX) {
        set_error("%s: a %d x %d frame (%ld bytes) does not fit the %ld bytes of LDS a workgroup holds it in", who, oh, ow, 3L * oh * ow, (long)AUG_LDS_MAX);
        return TEDSPAD_EUNSUPPORTED;
    }
    TS_REQUIRE(nluts >= 0 && table_words >= 0 && tables_off == (int64_t)nrec * (int64_t)sizeof(tedspad_augment_record) &&
                   luts_off == tables_off + table_words * 4 && blob_bytes == luts_off + (int64_t)nluts * 256,
               "%s: the blob must be {records, tables, gamma tables} back to back", who);
    TS_REQUIRE(so_c >= 0 && so_h >= 0 && so_w >= 0 && out_elems > 0, "%s: negative output stride", who);
    const int64_t extent = 2 * so_c + (int64_t)(oh - 1) * so_h + (int64_t)(ow - 1) * so_w;
    const tedspad_augment_record *rec = (const tedspad_augment_record *)blob_host;
    const int32_t *tables = (const int32_t *)((const char *)blob_host + tables_off);
    const int known = TEDSPAD_AUG_REVERSE * 2 - 1;
    for (int i = 0; i < nrec; i++) {
        const tedspad_augment_record &r = rec[i];
        TS_REQUIRE(r.src && r.H > 0 && r.W > 0, "%s: record %d: no source frame", who, i);
        TS_REQUIRE(r.top >= 0 && r.left >= 0 && r.ch > 0 && r.cw > 0 && r.top < r.H && r.left < r.W && r.ch < (1 << 20) && r.cw < (1 << 20),
                   "%s: record %d: crop box (top %d, left %d, %d x %d) must start inside the %d x %d frame", who, i, r.top, r.left, r.ch, r.cw, r.H, r.W);
        TS_REQUIRE(aug_table_ok(tables, table_words, r.ytab, r.ytaps, oh, r.ch) && aug_table_ok(tables, table_words, r.xtab, r.xtaps, ow, r.cw),
                   "%s: record %d: a resample table lies outside the blob or reaches outside the %d x %d crop", who, i, r.ch, r.cw);
        TS_REQUIRE((r.flags & ~known) == 0 && (!(r.flags & TEDSPAD_AUG_GAMMA) || ((r.flags & TEDSPAD_AUG_GRAY) && r.gamma_lut >= 0 && r.gamma_lut < nluts)),
                   "%s: record %d: bad flags 0x%x / gamma table %d of %d", who, i, r.flags, r.gamma_lut, nluts);
        TS_REQUIRE((r.flags & TEDSPAD_AUG_GAMMA) || r.gamma_lut == 0, "%s: record %d: gamma table index without the gamma op", who, i);
        TS_REQUIRE(r.hue_off >= 0 && r.hue_off <= 255, "%s: record %d: hue offset %d outside 0..255", who, i, r.hue_off);
        TS_REQUIRE(r.contrast == r.contrast && r.saturation == r.saturation && r.brightness == r.brightness, "%s: record %d: NaN factor", who, i);
        TS_REQUIRE(r.dst >= 0 && r.dst + extent < out_elems, "%s: record %d: output frame at %ld leaves the %ld elements of out", who, i, (long)r.dst,
                   (long)out_elems);
    }
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(blob_dev, blob_host, (size_t)blob_bytes, hipMemcpyHostToDevice, s) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: uploading the record table failed", who);
        return TEDSPAD_ELAUNCH;
    }
    AugKP p;
    p.rec = (const tedspad_augment_record *)blob_dev;
    p.tables = (const int32_t *)((const char *)blob_dev + tables_off);
    p.luts = (const uint8_t *)blob_dev + luts_off;
    p.out = out;
    p.oh = oh; p.ow = ow; p.so_c = so_c; p.so_h = so_h; p.so_w = so_w;
    return launch_lds<clip_augment_kernel>(who, dim3((unsigned)nrec), dim3(AUG_THREADS), AUG_LDS_HEAD + (size_t)3 * oh * ow, s, p);
}
