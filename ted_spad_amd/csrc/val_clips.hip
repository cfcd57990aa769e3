// The validation loaders' frames on the device, for gfx950 (aux_code/ucf101_dl.py: single_val_dataloader.augmentation :297-320, contrastive_val_dataloader
// .augmentation :873-896): center_crop -> resize -> hflip -> to_tensor on 8-bit PIL images, so the arithmetic is augment.hip's resized_crop step
//   Image.resize(BILINEAR): libImaging/Resample.c, horizontal pass rounded to uint8, then the vertical pass, 22-bit coefficients, clip8((2^21 + sum px * kk) >> 22)
// with one difference in the crop: torchvision's center_crop zero-pads a frame that is smaller than the crop, so the box may start at a negative coordinate and
// a source pixel outside the frame on ANY side is zero.
// A workgroup owns a band of output rows of three planes. It runs the horizontal pass once for every temporary row the band's vertical taps reach and keeps the
// bytes in LDS ([plane][row][ow]); after a barrier the vertical pass reads them back, consecutive lanes on consecutive bytes. Nothing frame-sized is held, so
// the output size is bounded only by one output row's taps (VAL_LDS_BUDGET). Two epilogues:
//   fp32  the planes are the three colours of one record (horizontal pass: lane = (pixel, colour), consecutive source bytes); lanes write consecutive floats.
//   act   the anonymizer's input for the PSEUDO-images the training / validation loops build ((B,3,n,H,W).reshape(-1,3,H,W)): plane p = c*n + k of
//         batch item b is channel p % 3 of image b*n + p/3, so the three planes are three (record, colour) pairs. Pixels are packed like feed.hip's activation
//         rows (act_put_pixel) into an LDS image of the band, which leaves as 16-byte pieces on consecutive lanes -- the band's rows are contiguous in HBM.
#include "common.h"

namespace tedspad {
namespace {

constexpr int VAL_THREADS = 256;
constexpr int VAL_LDS_BUDGET = 32 * 1024;           // per workgroup: five of them share a CU's 160 KB
constexpr int VAL_BAND_MAX = 16;                    // output rows per workgroup at most: small frames still spread over the CUs

struct ValKP {
    const tedspad_val_record *rec;
    const int32_t *tables;
    void *out;
    int oh, ow, band, nbands, trows;                // trows: the temporary rows a plane owns in LDS (the worst band of the worst record)
    int n, cpad;                                    // act form
    long so_c, so_h, so_w;                          // fp32 form
};

// one plane of a band: a record's frame, its tables and the temporary rows [lo, lo + rows) the band's vertical windows cover (the windows never move
// backwards: the entry checks it, so the first and the last output row bound them)
struct ValPlane {
    const uint8_t *src;
    const int32_t *ytab, *xtab;
    int ytaps, xtaps, H, W, top, left, lo, rows;
    bool flip, rev;
};

__device__ __forceinline__ int val_clip8_fixed(int v) {
    v >>= 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__device__ __forceinline__ ValPlane val_plane(const ValKP &p, const tedspad_val_record &R, int oy0, int oy1) {
    ValPlane P;
    P.src = R.src;
    P.ytab = p.tables + R.ytab;
    P.xtab = p.tables + R.xtab;
    P.ytaps = R.ytaps; P.xtaps = R.xtaps; P.H = R.H; P.W = R.W; P.top = R.top; P.left = R.left;
    const int32_t *first = P.ytab + (long)oy0 * (2 + R.ytaps), *last = P.ytab + (long)(oy1 - 1) * (2 + R.ytaps);
    P.lo = first[0];
    P.rows = last[0] + last[1] - first[0];
    P.flip = R.flags & TEDSPAD_AUG_HFLIP;
    P.rev = R.flags & TEDSPAD_AUG_REVERSE;
    return P;
}

// Horizontal pass of the plane's temporary rows into LDS bytes. NC == 3: the three colours of the record go to three LDS planes `pstride` apart, lane =
// (row, pixel, colour) with the colour fastest, so that a wave reads consecutive source bytes; NC == 1: output colour `c` alone, lane = (row, pixel).
template <int NC>
__device__ __forceinline__ void val_hpass(const ValPlane &P, int c, uint8_t *tmp, int pstride, int ow) {
    const int total = P.rows * ow * NC;
    for (int e = threadIdx.x; e < total; e += VAL_THREADS) {
        int q = e;
        if (NC == 3) {
            q = e / 3;
            c = e - q * 3;
        }
        const int r = q / ow, ox = q - r * ow;
        const int sy = P.top + P.lo + r;
        int hs = 1 << 21;
        if (sy >= 0 && sy < P.H) {                  // rows above and below the frame are zeros
            const int32_t *xe = P.xtab + (long)ox * (2 + P.xtaps);
            const int xmin = xe[0], xn = xe[1];
            const uint8_t *row = P.src + ((long)sy * P.W) * 3 + (P.rev ? 2 - c : c);
            for (int i = 0; i < xn; i++) {
                const int sx = P.left + xmin + i;
                if (sx >= 0 && sx < P.W) hs += (int)row[(long)sx * 3] * xe[2 + i];
            }
        }
        tmp[(NC == 3 ? c * pstride : 0) + r * ow + ox] = (uint8_t)val_clip8_fixed(hs);
    }
}

// vertical pass of output pixel (oy, ox) out of the plane's LDS rows, after the flip
__device__ __forceinline__ int val_vpass(const ValPlane &P, const uint8_t *tmp, int ow, int oy, int ox) {
    const int32_t *ye = P.ytab + (long)oy * (2 + P.ytaps);
    const int yn = ye[1];
    const uint8_t *col = tmp + (ye[0] - P.lo) * ow + (P.flip ? ow - 1 - ox : ox);
    int acc = 1 << 21;
    for (int j = 0; j < yn; j++) acc += (int)col[j * ow] * ye[2 + j];
    return val_clip8_fixed(acc);
}

template <bool ACT, typename T>
__global__ __launch_bounds__(VAL_THREADS) void val_clips_kernel(const ValKP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char val_lds[];
    const int ow = p.ow, tid = threadIdx.x;
    const int band = blockIdx.x % p.nbands, unit = blockIdx.x / p.nbands;
    const int oy0 = band * p.band, oy1 = min(p.oh, oy0 + p.band), nr = oy1 - oy0;
    const int pstride = p.trows * ow;
    if constexpr (!ACT) {
        uint8_t *tmp = val_lds;                                       // [3][trows][ow]
        const tedspad_val_record &R = p.rec[unit];
        const ValPlane P = val_plane(p, R, oy0, oy1);
        val_hpass<3>(P, 0, tmp, pstride, ow);
        __syncthreads();
        float *out = (float *)p.out + R.dst;
        const int npix = nr * ow;
        for (int e = tid; e < 3 * npix; e += VAL_THREADS) {           // consecutive lanes write consecutive floats of an output row
            const int c = e / npix, q = e - c * npix;
            const int oyl = q / ow, ox = q - oyl * ow;
            out[c * p.so_c + (oy0 + oyl) * p.so_h + ox * p.so_w] = (float)val_vpass(P, tmp + c * pstride, ow, oy0 + oyl, ox) / 255.f;
        }
    } else {
        const int n16 = ow * p.cpad / 8;                              // 16-byte pieces per activation row
        unsigned char *stage = val_lds;                               // [band][n16] pieces
        uint8_t *tmp = val_lds + (size_t)p.band * n16 * 16;           // [3][trows][ow]
        const int b = unit / p.n, m = unit - b * p.n;                 // pseudo-image m of batch item b: planes 3m, 3m + 1, 3m + 2
        ValPlane P[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int pl = 3 * m + j;
            const int c = pl / p.n, k = pl - c * p.n;
            P[j] = val_plane(p, p.rec[(long)b * p.n + k], oy0, oy1);
            val_hpass<1>(P[j], c, tmp + j * pstride, pstride, ow);
        }
        __syncthreads();
        for (int q = tid; q < nr * ow; q += VAL_THREADS) {
            const int oyl = q / ow, ox = q - oyl * ow;
            float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 3; ++j) v[j] = (float)val_vpass(P[j], tmp + j * pstride, ow, oy0 + oyl, ox) / 255.f;
            act_put_pixel<T>(stage + (size_t)oyl * n16 * 16, p.cpad, ox, v);
        }
        __syncthreads();
        uint4 *dst = (uint4 *)p.out + ((long)unit * p.oh + oy0) * n16;        // image b * n + m = unit; the band's rows follow one another
        for (int i = tid; i < nr * n16; i += VAL_THREADS) dst[i] = reinterpret_cast<const uint4 *>(stage)[i];
    }
}

// a table of `n` rows of (2 + taps) words for an input of `in` samples: every window inside the input, no window before the one of the row above
bool val_table_ok(const int32_t *tables, long words, long off, int taps, int n, int in) {
    if (off < 0 || taps < 1 || off + (long)n * (2 + taps) > words) return false;
    int lo = 0, hi = 0;
    for (int i = 0; i < n; i++) {
        const int32_t *e = tables + off + (long)i * (2 + taps);
        if (e[0] < 0 || e[1] < 0 || e[1] > taps || (long)e[0] + e[1] > in) return false;
        if (e[0] < lo || e[0] + e[1] < hi) return false;
        lo = e[0];
        hi = e[0] + e[1];
    }
    return true;
}

// What the two entries share: the blob, every record but its destination, and the LDS the band needs (`stage_row` bytes of packed output per band row on top
// of the temporary rows). Fills the kernel parameters that describe the blob and the bands.
int32_t val_check(const char *who, const void *blob_host, void *blob_dev, int64_t blob_bytes, int32_t nrec, int64_t tables_off, int64_t table_words,
                  const void *out, int32_t oh, int32_t ow, int32_t band, long stage_row, ValKP *p, size_t *lds) {
    static_assert(sizeof(tedspad_val_record) == 64, "tedspad_val_record layout (ted_spad_amd/val_clips.py RECORD)");
    TS_REQUIRE(blob_host && blob_dev && out, "%s: null pointer", who);
    TS_REQUIRE((uintptr_t)blob_dev % 8 == 0 && (uintptr_t)blob_host % 8 == 0, "%s: the record table must be 8-byte aligned", who);
    TS_REQUIRE(nrec > 0 && oh > 0 && ow > 0 && oh < 32768 && ow < 32768, "%s: bad sizes", who);
    TS_REQUIRE(band >= 1 && band <= VAL_BAND_MAX, "%s: %d output rows per workgroup; 1 .. %d", who, band, VAL_BAND_MAX);
    TS_REQUIRE(table_words >= 0 && tables_off == (int64_t)nrec * (int64_t)sizeof(tedspad_val_record) && blob_bytes == tables_off + table_words * 4,
               "%s: the blob must be {records, tables} back to back", who);
    const tedspad_val_record *rec = (const tedspad_val_record *)blob_host;
    const int32_t *tables = (const int32_t *)((const char *)blob_host + tables_off);
    const int nbands = (oh + band - 1) / band;
    TS_REQUIRE((long)nrec * nbands < (1L << 31), "%s: %d records x %d bands do not fit one launch", who, nrec, nbands);
    int trows = 1;
    for (int i = 0; i < nrec; i++) {
        const tedspad_val_record &r = rec[i];
        TS_REQUIRE(r.src && r.H > 0 && r.W > 0, "%s: record %d: no source frame", who, i);
        TS_REQUIRE(r.ch > 0 && r.cw > 0 && r.ch < (1 << 20) && r.cw < (1 << 20), "%s: record %d: empty crop box %d x %d", who, i, r.ch, r.cw);
        TS_REQUIRE(r.top > -(1 << 20) && r.left > -(1 << 20) && r.top < r.H && r.left < r.W && r.top + r.ch > 0 && r.left + r.cw > 0,
                   "%s: record %d: crop box (top %d, left %d, %d x %d) does not intersect the %d x %d frame", who, i, r.top, r.left, r.ch, r.cw, r.H, r.W);
        TS_REQUIRE(val_table_ok(tables, table_words, r.ytab, r.ytaps, oh, r.ch) && val_table_ok(tables, table_words, r.xtab, r.xtaps, ow, r.cw),
                   "%s: record %d: a resample table lies outside the blob, reaches outside the %d x %d crop or moves backwards", who, i, r.ch, r.cw);
        TS_REQUIRE((r.flags & ~(TEDSPAD_AUG_HFLIP | TEDSPAD_AUG_REVERSE)) == 0 && r.reserved == 0, "%s: record %d: bad flags 0x%x", who, i, r.flags);
        const int32_t *ytab = tables + r.ytab;
        for (int oy0 = 0; oy0 < oh; oy0 += band) {
            const int32_t *first = ytab + (long)oy0 * (2 + r.ytaps), *last = ytab + (long)((oy0 + band < oh ? oy0 + band : oh) - 1) * (2 + r.ytaps);
            const int rows = last[0] + last[1] - first[0];
            if (rows > trows) trows = rows;
        }
    }
    const long need = (long)band * stage_row + 3L * trows * ow;
    if (need > VAL_LDS_BUDGET) {
        set_error("%s: a band of %d output rows of width %d reaches %d temporary rows: %ld bytes of LDS, the budget is %d", who, band, ow, trows, need,
                  VAL_LDS_BUDGET);
        return TEDSPAD_EUNSUPPORTED;
    }
    p->rec = (const tedspad_val_record *)blob_dev;
    p->tables = (const int32_t *)((const char *)blob_dev + tables_off);
    p->oh = oh; p->ow = ow; p->band = band; p->nbands = nbands; p->trows = trows;
    p->n = 0; p->cpad = 0; p->so_c = p->so_h = p->so_w = 0;
    *lds = (size_t)((need + 15) / 16 * 16);
    return TEDSPAD_OK;
}

int32_t val_upload(const char *who, const void *blob_host, void *blob_dev, int64_t blob_bytes, hipStream_t s) {
    if (hipMemcpyAsync(blob_dev, blob_host, (size_t)blob_bytes, hipMemcpyHostToDevice, s) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: uploading the record table failed", who);
        return TEDSPAD_ELAUNCH;
    }
    return TEDSPAD_OK;
}

}  // namespace
}  // namespace tedspad

using namespace tedspad;

extern "C" int32_t tedspad_val_clips_lds_bytes(void) { return VAL_LDS_BUDGET; }

extern "C" int32_t tedspad_val_clips_band_max(void) { return VAL_BAND_MAX; }

extern "C" int32_t tedspad_val_clips(const void *blob_host, void *blob_dev, int64_t blob_bytes, int32_t nrec, int64_t tables_off, int64_t table_words, float *out,
                                     int64_t out_elems, int32_t oh, int32_t ow, int32_t band, int64_t so_c, int64_t so_h, int64_t so_w, void *stream) {
    const char *who = "tedspad_val_clips";
    ValKP p;
    size_t lds;
    int32_t rc = val_check(who, blob_host, blob_dev, blob_bytes, nrec, tables_off, table_words, out, oh, ow, band, 0, &p, &lds);
    if (rc != TEDSPAD_OK) return rc;
    TS_REQUIRE(so_c >= 0 && so_h >= 0 && so_w >= 0 && out_elems > 0, "%s: negative output stride", who);
    const int64_t extent = 2 * so_c + (int64_t)(oh - 1) * so_h + (int64_t)(ow - 1) * so_w;
    const tedspad_val_record *rec = (const tedspad_val_record *)blob_host;
    for (int i = 0; i < nrec; i++)
        TS_REQUIRE(rec[i].dst >= 0 && rec[i].dst + extent < out_elems, "%s: record %d: output frame at %ld leaves the %ld elements of out", who, i,
                   (long)rec[i].dst, (long)out_elems);
    hipStream_t s = (hipStream_t)stream;
    rc = val_upload(who, blob_host, blob_dev, blob_bytes, s);
    if (rc != TEDSPAD_OK) return rc;
    p.out = out;
    p.so_c = so_c; p.so_h = so_h; p.so_w = so_w;
    return launch_lds<val_clips_kernel<false, F16>>(who, dim3((unsigned)((long)nrec * p.nbands)), dim3(VAL_THREADS), lds, s, p);
}

extern "C" int32_t tedspad_val_clips_act(const void *blob_host, void *blob_dev, int64_t blob_bytes, int32_t nrec, int64_t tables_off, int64_t table_words, void *act,
                                         int64_t act_bytes, int32_t n, int32_t oh, int32_t ow, int32_t band, int32_t cpad, int32_t dtype, void *stream) {
    const char *who = "tedspad_val_clips_act";
    TS_REQUIRE(cpad == 4 || cpad == 8, "%s: cpad must be 4 (pixel pairs) or 8", who);
    TS_REQUIRE(cpad == 8 || ow % 2 == 0, "%s: cpad=4 packs pixel pairs, the output width %d must be even", who, ow);
    TS_REQUIRE(dtype == TEDSPAD_F16 || dtype == TEDSPAD_BF16, "%s: bad dtype", who);
    TS_REQUIRE((uintptr_t)act % 16 == 0, "%s: the activation must be 16-byte aligned", who);
    ValKP p;
    size_t lds;
    int32_t rc = val_check(who, blob_host, blob_dev, blob_bytes, nrec, tables_off, table_words, act, oh, ow, band, (long)ow * cpad * 2, &p, &lds);
    if (rc != TEDSPAD_OK) return rc;
    TS_REQUIRE(n > 0 && nrec % n == 0, "%s: %d records are not whole batch items of %d frames (every item needs the same number)", who, nrec, n);
    TS_REQUIRE(act_bytes >= (int64_t)nrec * oh * ow * cpad * 2, "%s: %d images of %d x %d x %d leave the %ld bytes of the activation", who, nrec, oh, ow, cpad,
               (long)act_bytes);
    const tedspad_val_record *rec = (const tedspad_val_record *)blob_host;
    for (int i = 0; i < nrec; i++) TS_REQUIRE(rec[i].dst == 0, "%s: record %d: the activation form takes no destination offset", who, i);
    hipStream_t s = (hipStream_t)stream;
    rc = val_upload(who, blob_host, blob_dev, blob_bytes, s);
    if (rc != TEDSPAD_OK) return rc;
    p.out = act;
    p.n = n; p.cpad = cpad;
    const dim3 g((unsigned)((long)nrec * p.nbands));
    TS_WITH_T(dtype, return launch_lds<val_clips_kernel<true, T>>(who, g, dim3(VAL_THREADS), lds, s, p));
}
