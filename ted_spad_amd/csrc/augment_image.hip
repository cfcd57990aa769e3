// The VISPR loaders' image augmentation on the device, for gfx950 (aux_code/vispr_dl.py: vispr_dataset.augmentation :71-129, vispr_ssl_dataset.augmentation
// :186-251). `read_image` gives the reference a uint8 TENSOR, so every trans.functional call takes torchvision's tensor path (0.15.2 _functional_tensor.py),
// which is fp32 arithmetic truncated to a byte after every op -- not Pillow's fixed point, hence not augment.hip's kernel:
//   resized_crop  crop (zeros right of / below the image) + ATen's _upsample_bilinear2d_aa on fp32 (align_corners=False): width pass into an fp32
//                 intermediate, then the height pass, triangle weights normalised in fp32 (feed.hip's aa_table, built on the host), ONE rounding at the end:
//                 round half to even, cast to a byte
//   _blend        (f * a + (1 - f) * b).clamp(0, 255) truncated; every product and the sum round on their own in eager torch; f and (1 - f) arrive as
//                 fp32 (1 - f is formed in double on the host, as Python does)
//   contrast      _blend(img, mean(float(gray(img))), f), the mean = an integer sum below 2^24 (order-independent) / the pixel count, one IEEE division
//   hue           byte / 255 -> _rgb2hsv -> (h + f) % 1.0 -> _hsv2rgb -> * (256 - 1e-3) truncated
//   saturation    _blend(img, gray(img), f);   brightness: _blend(img, 0, f);   gray: (0.2989 r + 0.587 g + 0.114 b) truncated
//   gamma         a 256-entry table the host builds with torch's own CPU pow;   hflip;   one erase box (zeros, after the flip);   byte / 255
// One workgroup of 1024 threads per output image; the resized uint8 image lives in LDS as three planes (150 528 B at 224 x 224), the colour chain runs on it
// in place, and the planes leave as coalesced fp32 rows. The width-pass intermediate ([3][rows of the crop][ow] fp32, 3 MB for 1100 rows at 224 columns) does
// not fit beside the planes: it lives in a scratch buffer the wrapper allocates (one slice per record, written and read back by the same workgroup, so it
// stays in L2), and a __syncthreads() separates the passes.
//
// As in augment.hip: build.py compiles with -ffp-contract=fast and the gfx950 back end fuses a multiply with the add behind it, which changes bytes of every
// op of the colour chain, so every product that feeds an addition or subtraction there goes through img_mul. The two resize passes are left to the compiler:
// torch's own kernel is compiled for several vector ISAs, with and without FMA, so its last bit is not defined either.
#pragma clang fp contract(off)
#include <math.h>

#include "common.h"

namespace tedspad {
namespace {

constexpr int IMG_THREADS = 1024;
constexpr size_t IMG_LDS_MAX = 3 * 224 * 224;       // the image planes: 150 528 of the CU's 163 840 bytes
constexpr int IMG_LDS_HEAD = 16;                    // the two gray sums in front of them
constexpr int IMG_MAX_SIDE = 16384;                 // source height / width
constexpr int IMG_MAX_CROP = 4096;                  // crop height / width: the intermediate of one record stays below 3 * 4096 * 224 floats

struct ImgKP {
    const tedspad_image_record *rec;
    const int32_t *tables;
    const uint8_t *luts;
    float *scratch;
    float *out;
    int oh, ow;
    long so_c, so_h, so_w;
};

// one IEEE multiply whose result no later addition can be fused with
__device__ __forceinline__ float img_mul(float a, float b) {
    float m = a * b;
    asm volatile("" : "+v"(m));
    return m;
}

__device__ __forceinline__ float img_clamp(float v, float hi) { return fminf(fmaxf(v, 0.f), hi); }

// (0.2989 * r + 0.587 * g + 0.114 * b).to(uint8)
__device__ __forceinline__ int img_gray(int r, int g, int b) {
    return (int)((img_mul(0.2989f, (float)r) + img_mul(0.587f, (float)g)) + img_mul(0.114f, (float)b));
}

// _blend for one byte: (f * a + (1 - f) * b).clamp(0, 255).to(uint8)
__device__ __forceinline__ int img_blend(int a, float b, float f, float f1m) { return (int)img_clamp(img_mul(f, (float)a) + img_mul(f1m, b), 255.f); }

// adjust_hue for one pixel: convert_image_dtype -> _rgb2hsv -> (h + f) % 1.0 -> _hsv2rgb -> convert_image_dtype
__device__ __forceinline__ void img_hue(int &ri, int &gi, int &bi, float hf) {
    const float r = (float)ri / 255.f, g = (float)gi / 255.f, b = (float)bi / 255.f;
    const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
    const bool eqc = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eqc ? 1.f : maxc);
    const float crd = eqc ? 1.f : cr;
    const float rc = (maxc - r) / crd, gc = (maxc - g) / crd, bc = (maxc - b) / crd;
    float h;
    if (maxc == r) h = bc - gc;
    else if (maxc == g) h = (2.0f + rc) - bc;
    else h = (4.0f + gc) - rc;
    h = h / 6.0f + 1.0f;                    // in [0.83, 1.84): fmod(h, 1.0) is h or h - 1, both exact
    if (h >= 1.0f) h -= 1.0f;
    // (h + f) % 1.0 as torch.remainder: fmod (exact), then + 1.0 (rounded) for a negative remainder
    h = h + hf;
    h = h - truncf(h);
    if (h < 0.f) h += 1.0f;
    const float v = maxc;
    const float h6 = img_mul(h, 6.0f);
    const float fl = floorf(h6);
    const float f = h6 - fl;
    const float p = img_clamp(img_mul(v, 1.0f - s), 1.f);
    const float q = img_clamp(img_mul(v, 1.0f - img_mul(s, f)), 1.f);
    const float t = img_clamp(img_mul(v, 1.0f - img_mul(s, 1.0f - f)), 1.f);
    float ro, go, bo;
    switch ((int)fl % 6) {
    case 0: ro = v; go = t; bo = p; break;
    case 1: ro = q; go = v; bo = p; break;
    case 2: ro = p; go = v; bo = t; break;
    case 3: ro = p; go = q; bo = v; break;
    case 4: ro = t; go = p; bo = v; break;
    default: ro = v; go = p; bo = q; break;
    }
    const float k = (float)(255 + 1.0 - 1e-3);
    ri = (int)img_mul(ro, k);
    gi = (int)img_mul(go, k);
    bi = (int)img_mul(bo, k);
}

__global__ __launch_bounds__(IMG_THREADS) void image_augment_kernel(const ImgKP p) {
    // all of the LDS is dynamic (launch.h raises the dynamic limit to the CU's 160 KB: static LDS beside it would not fit the attribute)
    extern __shared__ __attribute__((aligned(16))) uint8_t img_lds[];
    unsigned *lsum = reinterpret_cast<unsigned *>(img_lds);               // the two gray sums
    uint8_t *img_px = img_lds + IMG_LDS_HEAD;                             // [3][oh][ow]
    const tedspad_image_record &R = p.rec[blockIdx.x];
    const int oh = p.oh, ow = p.ow, npix = oh * ow;
    const int tid = threadIdx.x;
    const int flags = R.flags;
    if (tid < 2) lsum[tid] = 0u;

    // 1. crop + ATen's antialiased bilinear resize. Rows of the crop below the image are zeros and are neither computed nor stored.
    {
        const int32_t *ytab = p.tables + R.ytab, *xtab = p.tables + R.xtab;
        const int H = R.H, W = R.W, top = R.top, left = R.left;
        const int rows = min(R.ch, H - top);
        float *tmp = p.scratch + R.tmp;                                   // [3][rows][ow]
        // 1a. width pass: consecutive lanes = consecutive output columns of one source row
        for (int e = tid; e < 3 * rows * ow; e += IMG_THREADS) {
            const int rr = e / ow, ox = e - rr * ow;
            const int c = rr / rows, r = rr - c * rows;
            const int32_t *xe = xtab + (long)ox * (2 + R.xtaps);
            const int xmin = xe[0], xn = xe[1];
            const float *wx = reinterpret_cast<const float *>(xe + 2);
            const uint8_t *row = R.src + ((long)c * H + top + r) * W + left + xmin;
            const int live = min(xn, W - left - xmin);                    // columns right of the image are zeros
            float acc = 0.f;
            for (int i = 0; i < live; i++) acc += wx[i] * (float)row[i];
            tmp[e] = acc;
        }
        __syncthreads();
        // 1b. height pass, one rounding (half to even), the byte into LDS
        for (int e = tid; e < npix * 3; e += IMG_THREADS) {
            const int c = e / npix, pix = e - c * npix;
            const int oy = pix / ow, ox = pix - oy * ow;
            const int32_t *ye = ytab + (long)oy * (2 + R.ytaps);
            const int ymin = ye[0];
            const float *wy = reinterpret_cast<const float *>(ye + 2);
            const int live = min(ye[1], rows - ymin);
            const float *col = tmp + ((long)c * rows + ymin) * ow + ox;
            float acc = 0.f;
            for (int j = 0; j < live; j++) acc += wy[j] * col[(long)j * ow];
            img_px[e] = (uint8_t)(int)img_clamp(rintf(acc), 255.f);
        }
    }
    __syncthreads();

    uint8_t *pr = img_px, *pg = img_px + npix, *pb = img_px + 2 * npix;
    const int colour = TEDSPAD_AUG_CONTRAST_FIRST | TEDSPAD_AUG_HUE | TEDSPAD_AUG_SATURATION | TEDSPAD_AUG_BRIGHTNESS | TEDSPAD_AUG_CONTRAST_LATE |
                       TEDSPAD_AUG_GRAY;
    if (flags & colour) {                           // (uniform)
        const float ac = R.contrast, ac1 = R.contrast_1m, as = R.saturation, as1 = R.saturation_1m, ab = R.brightness, ab1 = R.brightness_1m;
        const uint8_t *lut = p.luts + (long)R.gamma_lut * 256;
        // 2a. mean gray for a contrast in first position
        float mean0 = 0.f;
        if (flags & TEDSPAD_AUG_CONTRAST_FIRST) {
            unsigned s = 0;
            for (int i = tid; i < npix; i += IMG_THREADS) s += (unsigned)img_gray(pr[i], pg[i], pb[i]);
            atomicAdd(&lsum[0], s);
            __syncthreads();
            mean0 = (float)lsum[0] / (float)npix;
        }
        // 2b. contrast, hue, saturation, brightness; then grayscale + gamma unless a late contrast has to see the whole image first
        const bool late = flags & TEDSPAD_AUG_CONTRAST_LATE;
        unsigned s1 = 0;
        for (int i = tid; i < npix; i += IMG_THREADS) {
            int r = pr[i], g = pg[i], b = pb[i];
            if (flags & TEDSPAD_AUG_CONTRAST_FIRST) {
                r = img_blend(r, mean0, ac, ac1);
                g = img_blend(g, mean0, ac, ac1);
                b = img_blend(b, mean0, ac, ac1);
            }
            if (flags & TEDSPAD_AUG_HUE) img_hue(r, g, b, R.hue);
            if (flags & TEDSPAD_AUG_SATURATION) {
                const float l = (float)img_gray(r, g, b);
                r = img_blend(r, l, as, as1);
                g = img_blend(g, l, as, as1);
                b = img_blend(b, l, as, as1);
            }
            if (flags & TEDSPAD_AUG_BRIGHTNESS) {
                r = img_blend(r, 0.f, ab, ab1);
                g = img_blend(g, 0.f, ab, ab1);
                b = img_blend(b, 0.f, ab, ab1);
            }
            if (late) {
                s1 += (unsigned)img_gray(r, g, b);
            } else if (flags & TEDSPAD_AUG_GRAY) {
                int l = img_gray(r, g, b);
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
            const float mean1 = (float)lsum[1] / (float)npix;
            for (int i = tid; i < npix; i += IMG_THREADS) {
                int r = img_blend(pr[i], mean1, ac, ac1), g = img_blend(pg[i], mean1, ac, ac1), b = img_blend(pb[i], mean1, ac, ac1);
                if (flags & TEDSPAD_AUG_GRAY) {
                    int l = img_gray(r, g, b);
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

    // 3. hflip, erase, / 255: consecutive lanes write consecutive floats of an output row
    const bool flip = flags & TEDSPAD_AUG_HFLIP;
    const int ei = R.erase[0], ej = R.erase[1], eh = R.erase[2], ew = R.erase[3];
    float *out = p.out + R.dst;
    for (int e = tid; e < npix * 3; e += IMG_THREADS) {
        const int c = e / npix, pix = e - c * npix;
        const int oy = pix / ow, ox = pix - oy * ow;
        int v = img_px[c * npix + oy * ow + (flip ? ow - 1 - ox : ox)];
        if (oy >= ei && oy - ei < eh && ox >= ej && ox - ej < ew) v = 0;
        out[c * p.so_c + oy * p.so_h + ox * p.so_w] = (float)v / 255.f;
    }
}

// a table of `n` rows of (2 + taps) words for an input of `in` samples: every row's window inside the input
bool img_table_ok(const int32_t *tables, long words, long off, int taps, int n, int in) {
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

extern "C" int32_t tedspad_image_augment(const void *blob_host, void *blob_dev, int64_t blob_bytes, int32_t nrec, int64_t tables_off, int64_t table_words,
                                         int64_t luts_off, int32_t nluts, float *scratch, int64_t scratch_elems, float *out, int64_t out_elems, int32_t oh,
                                         int32_t ow, int64_t so_c, int64_t so_h, int64_t so_w, void *stream) {
    const char *who = "tedspad_image_augment";
    static_assert(sizeof(tedspad_image_record) == 120, "tedspad_image_record layout (ted_spad_amd/vispr_augment.py RECORD)");
    TS_REQUIRE(blob_host && blob_dev && out && scratch, "%s: null pointer", who);
    TS_REQUIRE((uintptr_t)blob_dev % 8 == 0 && (uintptr_t)blob_host % 8 == 0, "%s: the record table must be 8-byte aligned", who);
    TS_REQUIRE(nrec > 0 && oh > 0 && ow > 0 && oh < 32768 && ow < 32768, "%s: bad sizes", who);
    if ((size_t)3 * oh * ow > IMG_LDS_MAX) {
        set_error("%s: a %d x %d image (%ld bytes) does not fit the %ld bytes of LDS a workgroup holds it in", who, oh, ow, 3L * oh * ow, (long)IMG_LDS_MAX);
        return TEDSPAD_EUNSUPPORTED;
    }
    TS_REQUIRE(nluts >= 0 && table_words >= 0 && tables_off == (int64_t)nrec * (int64_t)sizeof(tedspad_image_record) &&
                   luts_off == tables_off + table_words * 4 && blob_bytes == luts_off + (int64_t)nluts * 256,
               "%s: the blob must be {records, tables, gamma tables} back to back", who);
    TS_REQUIRE(so_c >= 0 && so_h >= 0 && so_w >= 0 && out_elems > 0 && scratch_elems > 0, "%s: negative output stride", who);
    const int64_t extent = 2 * so_c + (int64_t)(oh - 1) * so_h + (int64_t)(ow - 1) * so_w;
    const tedspad_image_record *rec = (const tedspad_image_record *)blob_host;
    const int32_t *tables = (const int32_t *)((const char *)blob_host + tables_off);
    const int known = TEDSPAD_AUG_HFLIP * 2 - 1;
    for (int i = 0; i < nrec; i++) {
        const tedspad_image_record &r = rec[i];
        TS_REQUIRE(r.src && r.H > 0 && r.W > 0, "%s: record %d: no source image", who, i);
        if (r.H > IMG_MAX_SIDE || r.W > IMG_MAX_SIDE || r.ch > IMG_MAX_CROP || r.cw > IMG_MAX_CROP) {
            set_error("%s: record %d: a %d x %d crop of a %d x %d image is beyond the limit: sources up to %d x %d, crop boxes up to %d x %d", who, i, r.ch,
                      r.cw, r.H, r.W, IMG_MAX_SIDE, IMG_MAX_SIDE, IMG_MAX_CROP, IMG_MAX_CROP);
            return TEDSPAD_EUNSUPPORTED;
        }
        TS_REQUIRE(r.top >= 0 && r.left >= 0 && r.ch > 0 && r.cw > 0 && r.top < r.H && r.left < r.W,
                   "%s: record %d: crop box (top %d, left %d, %d x %d) must start inside the %d x %d image", who, i, r.top, r.left, r.ch, r.cw, r.H, r.W);
        TS_REQUIRE(img_table_ok(tables, table_words, r.ytab, r.ytaps, oh, r.ch) && img_table_ok(tables, table_words, r.xtab, r.xtaps, ow, r.cw),
                   "%s: record %d: a resample table lies outside the blob or reaches outside the %d x %d crop", who, i, r.ch, r.cw);
        TS_REQUIRE((r.flags & ~known) == 0 && (!(r.flags & TEDSPAD_AUG_GAMMA) || ((r.flags & TEDSPAD_AUG_GRAY) && r.gamma_lut >= 0 && r.gamma_lut < nluts)),
                   "%s: record %d: bad flags 0x%x / gamma table %d of %d", who, i, r.flags, r.gamma_lut, nluts);
        TS_REQUIRE((r.flags & TEDSPAD_AUG_GAMMA) || r.gamma_lut == 0, "%s: record %d: gamma table index without the gamma op", who, i);
        TS_REQUIRE(!((r.flags & TEDSPAD_AUG_CONTRAST_FIRST) && (r.flags & TEDSPAD_AUG_CONTRAST_LATE)), "%s: record %d: contrast in both positions", who, i);
        TS_REQUIRE(r.hue >= -0.5f && r.hue <= 0.5f, "%s: record %d: hue factor %g outside [-0.5, 0.5]", who, i, (double)r.hue);
        TS_REQUIRE(r.contrast == r.contrast && r.saturation == r.saturation && r.brightness == r.brightness && r.contrast_1m == r.contrast_1m &&
                       r.saturation_1m == r.saturation_1m && r.brightness_1m == r.brightness_1m, "%s: record %d: NaN factor", who, i);
        const int64_t rows = r.ch < r.H - r.top ? r.ch : r.H - r.top;
        TS_REQUIRE(r.tmp >= 0 && r.tmp + 3 * rows * ow <= scratch_elems, "%s: record %d: the width-pass intermediate at %ld leaves the %ld elements of scratch",
                   who, i, (long)r.tmp, (long)scratch_elems);
        for (int k = 0; k < i; k++) {            // two workgroups must not share a slice
            const int64_t krows = rec[k].ch < rec[k].H - rec[k].top ? rec[k].ch : rec[k].H - rec[k].top;
            TS_REQUIRE(r.tmp + 3 * rows * ow <= rec[k].tmp || rec[k].tmp + 3 * krows * ow <= r.tmp, "%s: records %d and %d share scratch", who, k, i);
        }
        TS_REQUIRE(r.dst >= 0 && r.dst + extent < out_elems, "%s: record %d: output image at %ld leaves the %ld elements of out", who, i, (long)r.dst,
                   (long)out_elems);
    }
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(blob_dev, blob_host, (size_t)blob_bytes, hipMemcpyHostToDevice, s) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: uploading the record table failed", who);
        return TEDSPAD_ELAUNCH;
    }
    ImgKP p;
    p.rec = (const tedspad_image_record *)blob_dev;
    p.tables = (const int32_t *)((const char *)blob_dev + tables_off);
    p.luts = (const uint8_t *)blob_dev + luts_off;
    p.scratch = scratch;
    p.out = out;
    p.oh = oh; p.ow = ow; p.so_c = so_c; p.so_h = so_h; p.so_w = so_w;
    return launch_lds<image_augment_kernel>(who, dim3((unsigned)nrec), dim3(IMG_THREADS), IMG_LDS_HEAD + (size_t)3 * oh * ow, s, p);
}
