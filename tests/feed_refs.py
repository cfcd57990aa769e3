"""float64 references and case tables of the frame-feed kernels (csrc/feed.hip: tedspad_frames_crop_resize, _tp, tedspad_frames_ten_crop_tp, _act, _pil, _pil_act),
restated from the contract in include/tedspad_hip.h and the reference's semantics (dali_extraction.py:38-73, shanghai_dl.py:27-40); nothing follows a kernel's code
path. CPU only: tests/test_feed_refs.py checks the tables' conditions and that they are telling, tests/test_hip_feed_exact.py (-m gpu) compares the kernels with them
through `verdict`, the one comparison both files make.

Two kinds of element. EXACT: uint8 / integer-valued frames, divisor 256 and weights that are multiples of 2^-g (identity, x2, x4, the interior of 2:1 and 4:1): every
product and partial sum is a multiple of 2^-(8 + gy + gx) below 1, exact in fp32 in any order, so the fp32 output equals the reference and a 16-bit output equals its
one rounding, ties to even included. (Identity at divisor 255: weights {1, 0}, the output is fl32(b / 255) itself.) BOUNDED: all terms are non-negative, so the fp32
result g obeys |g - ref| <= k * 2^-24 * ref, k = ytaps + xtaps + 4 (a rounding per product and per add of each pass, the division, one of slack); a 16-bit output
lies between the roundings of the two ends, with no tolerance of its own. Both are one interval test per element: lo <= got <= hi, lo = hi for an exact element.

Everything returned is a float64 torch tensor unless it says otherwise."""
import zlib
from dataclasses import dataclass

import numpy as np
import torch

import kernel_refs as K

D = torch.float64
EPS = 2.0 ** -24
SENTINEL16 = 12288.0                       # the exact files' fill of a 16-bit buffer; no value here exceeds 255 / 200
WRONG = ("trunc16", "drop_last_tap", "flip_shift", "box_x0_zero", "no_zero_front", "t_clip_16", "chan_swap", "centre_half_up")
ENTRIES = ("fp32", "rec", "ten", "act4", "act8")
STEM_KT, STEM_PAD_T = 5, 2                 # I3Res50's conv1: 5 frames, temporal stride 2, pad 2 (large_i3d.py:133)


# ---- the resize weights: torch's rule (aten UpSampleKernel, _compute_indices_min_size_weights_aa with the bilinear filter) in fp32 ------------------------------
def aa_taps(n_in, n_out):
    f = np.float32
    scale = f(n_in) / f(n_out)
    return int(np.ceil(max(scale, f(1)))) * 2 + 1


def aa_table(n_in, n_out):
    """(first[out] int, count[out] int, w[out, taps] float32): the header's table {first input index, tap count, float weights}."""
    f = np.float32
    scale = f(n_in) / f(n_out)
    support = scale if scale >= f(1) else f(1)
    invscale = f(1) / scale if scale >= f(1) else f(1)
    taps = aa_taps(n_in, n_out)
    first, count, w = np.zeros(n_out, np.int64), np.zeros(n_out, np.int64), np.zeros((n_out, taps), f)
    for i in range(n_out):
        center = f(scale * f(f(i) + f(0.5)))
        lo = max(int(f(f(center - support) + f(0.5))), 0)                  # int(): towards zero, as the cast to int64
        hi = min(int(f(f(center + support) + f(0.5))), n_in)
        n = min(hi - lo, taps)
        total = f(0)
        for j in range(n):
            x = abs(f(f(f(f(j + lo) - center) + f(0.5)) * invscale))
            w[i, j] = f(1) - x if x < f(1) else f(0)
            total = f(total + w[i, j])
        if total != 0:
            w[i, :n] = w[i, :n] / total
        first[i], count[i] = lo, n
    return first, count, w


def aa_weights(n_in, n_out, wrong=None):
    """The dense (out, in) weight matrix, the fp32 weights as float64."""
    first, count, w = aa_table(n_in, n_out)
    dense = torch.zeros((n_out, n_in), dtype=D)
    for i in range(n_out):
        n = int(count[i])
        if wrong == "drop_last_tap":
            n -= 1
        dense[i, first[i]:first[i] + n] = torch.from_numpy(w[i, :n].astype(np.float64))
    return dense


def dyadic_bits(w, limit=12):
    """The smallest g with every weight a multiple of 2^-g, or None if there is none up to `limit`."""
    for g in range(limit + 1):
        s = w * 2.0 ** g
        if bool((s == s.round()).all()):
            return g
    return None


# ---- clip sampling -------------------------------------------------------------------------------------------------------------------------------------------
def frame_pairs(t_clip):
    """The stem's output-frame pairs of a clip of t_clip frames (conv 5 / stride 2 / pad 2, then the temporal pool's pairs)."""
    return ((t_clip + 2 * STEM_PAD_T - STEM_KT) // 2 + 1) // 2


def frame_of(n, f, first, clip_step, frame_step, t_clip, T, wrong=None):
    """Source frame of frame f of clip n, None for a zero frame: f outside the clip, a source index in front of the video or past its end."""
    if not 0 <= f < (16 if wrong == "t_clip_16" else t_clip):
        return None
    fr = first + n * clip_step + f * frame_step
    if fr >= T:
        return None
    if fr < 0:
        return fr % T if wrong == "no_zero_front" else None
    return fr


# ---- the resample --------------------------------------------------------------------------------------------------------------------------------------------
def resample64(frames, box, out_hw, divisor, flip, wrong=None):
    """frames: (T,H,W,C) numpy, uint8 or integer-valued float32. fl32(px / divisor) -- the one fp32 division is the reference's input -- then Wy @ v @ Wx^T in
    float64, then the flip. Returns (T, C, oh, ow)."""
    y0, x0, ch, cw = box
    if wrong == "box_x0_zero":
        x0 = 0
    v = (frames[:, y0:y0 + ch, x0:x0 + cw].astype(np.float32) / np.float32(divisor)).astype(np.float64)
    v = torch.from_numpy(v).permute(0, 3, 1, 2)
    wy, wx = aa_weights(ch, out_hw[0], wrong), aa_weights(cw, out_hw[1], wrong)
    out = torch.einsum("yh,tchw,xw->tcyx", wy, v, wx)
    if flip:
        out = out.flip(-1)
        if wrong == "flip_shift":
            out = out.roll(1, -1)                                           # pixel ox from ow - ox instead of ow - 1 - ox
    if wrong == "chan_swap" and out.shape[1] > 1:
        out = out.flip(1)
    return out


def bound_k(box, out_hw):
    return aa_taps(box[2], out_hw[0]) + aa_taps(box[3], out_hw[1]) + 4


def pil_resample(frames, box, out_hw):
    """Pillow itself on the cropped array (mode "L" for one channel), then / 255 as to_tensor: (T, C, oh, ow)."""
    from PIL import Image
    y0, x0, ch, cw = box
    out = []
    for fr in frames:
        crop = np.ascontiguousarray(fr[y0:y0 + ch, x0:x0 + cw])
        img = Image.fromarray(crop[..., 0]) if crop.shape[2] == 1 else Image.fromarray(crop)
        arr = np.array(img.resize((out_hw[1], out_hw[0]), Image.BILINEAR), copy=True).reshape(out_hw[0], out_hw[1], -1)
        out.append((arr.astype(np.float32) / np.float32(255)).astype(np.float64))
    return torch.from_numpy(np.stack(out)).permute(0, 3, 1, 2).contiguous()


# ---- the 16-bit rounding ---------------------------------------------------------------------------------------------------------------------------------------
def round16(t64, dtype, wrong=None):
    """float64 -> fp32 -> 16 bits, each to nearest even: K.round_once without its exactness check (monotone, which is all the containment test needs: an fp32
    value inside [lo, hi] rounds to a 16-bit value inside [round16(lo), round16(hi)])."""
    f = t64.to(torch.float32)
    if wrong == "trunc16":
        keep = 16 if dtype == "bf16" else 13
        f = (f.view(torch.int32) & ~((1 << keep) - 1)).view(torch.float32)
    return f.to(K.TDT[dtype]).to(D)


def is_tie(v, dtype):
    """True where the fp32-exact value lies exactly half way between two neighbours of the storage type."""
    r = round16(v, dtype)
    other = 2.0 * v - r
    return (r != v) & (round16(other, dtype) == other)


# ---- layouts, from the header's text -----------------------------------------------------------------------------------------------------------------------------
def records64(x, samp, wrong=None):
    """x: (T, C, oh, ow) resampled source frames -> X[n][tp][oh][b][ow/2][24]: value dt*3 + c of the record of pixel (y, 2*wq + b) = channel c of frame
    4*tp - pad_t + dt of clip n, zero for a zero frame and for c >= C."""
    n_clips, first, clip_step, frame_step, t_clip = samp
    T, C, oh, ow = x.shape
    tp_n = frame_pairs(t_clip)
    out = torch.zeros((n_clips, tp_n, oh, 2, ow // 2, 24), dtype=D)
    for n in range(n_clips):
        for tp in range(tp_n):
            for dt in range(8):
                s = frame_of(n, 4 * tp - STEM_PAD_T + dt, first, clip_step, frame_step, t_clip, T, wrong)
                if s is None:
                    continue
                for c in range(C):
                    for b in range(2):
                        out[n, tp, :, b, :, dt * 3 + c] = x[s, c, :, b::2]
    return out


def ten_crop_boxes64(H, W, ch, cw, wrong=None):
    """torchvision's ten_crop as (y0, x0, flip) in the unflipped frame's coordinates: tl, tr, bl, br, centre (center_crop: round half to even), then the same five
    of the horizontally flipped frame -- box (y, x) of the flipped frame is the mirror image of box (y, W - cw - x)."""
    if wrong == "centre_half_up":
        yc, xc = int(np.floor((H - ch) / 2.0 + 0.5)), int(np.floor((W - cw) / 2.0 + 0.5))
    else:
        yc, xc = int(round((H - ch) / 2.0)), int(round((W - cw) / 2.0))
    five = [(0, 0), (0, W - cw), (H - ch, 0), (H - ch, W - cw), (yc, xc)]
    return [(y, x, False) for y, x in five] + [(y, W - cw - x, True) for y, x in five]


def ten_crop64(per_box, samp, wrong=None):
    """per_box: the ten resampled (T, C, oh, ow) -> records of clip time i / crop k at index 10 * i + k."""
    recs = [records64(x, samp, wrong) for x in per_box]
    return torch.stack(recs, dim=1).reshape((10 * samp[0],) + tuple(recs[0].shape[1:]))


def act64(x, samp, cpad, wrong=None):
    """x: (T, C, oh, ow) -> output frame i * t_clip + f = frame f of clip i as channels-last rows (frames, 1, oh, ow, cpad), channels >= C zero; shaped as the
    library's buffer: cpad 4 -> pixel pairs (frames, 1, oh, ow / 2, 8), cpad 8 -> (frames, 1, oh, ow, 8)."""
    n_clips, first, clip_step, frame_step, t_clip = samp
    T, C, oh, ow = x.shape
    tc = 16 if wrong == "t_clip_16" else t_clip
    out = torch.zeros((n_clips * t_clip, oh, ow, cpad), dtype=D)
    for fo in range(n_clips * t_clip):
        s = frame_of(fo // tc, fo % tc, first, clip_step, frame_step, t_clip, T, wrong)
        if s is not None:
            out[fo, :, :, :C] = x[s].permute(1, 2, 0)
    return out.reshape(n_clips * t_clip, 1, oh, ow // 2 if cpad == 4 else ow, 8)


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------------------------
_FRAMES = {}


@dataclass(frozen=True)
class Case:
    name: str
    thwc: tuple                      # source frames (T, H, W, C)
    box: tuple                       # (y0, x0, ch, cw) of the single-box entries; the ten-crop entry takes (ch, cw)
    out: tuple                       # (oh, ow)
    samp: tuple                      # (n_clips, first, clip_step, frame_step, t_clip); the activation entries, which refuse first < 0, take |first|
    divisor: float = 256.0
    flip: bool = False
    kind: str = "exact"              # "exact": lo = hi = ref; "ring": exact on the interior, bounded on the first and last output row and column; "bounded"
    fill: str = "rand"               # "rand", or "bytes": every frame's crop box holds every byte value
    shift: int = 0                   # the uint8 frames begin `shift` bytes into their buffer (buf[s:s+n].view(T,H,W,C)), which ends with them
    entries: tuple = ENTRIES
    needs: tuple = ()                # the properties (PROPERTIES) this case is in the table for

    @property
    def C(self):
        return self.thwc[3]

    def samp_of(self, entry):
        n, first, cs, fs, tc = self.samp
        return (n, abs(first) if entry.startswith("act") else first, cs, fs, tc)

    def frames(self):
        """(T,H,W,C) uint8 numpy, seeded by the name; built once."""
        if self.name not in _FRAMES:
            _FRAMES[self.name] = self._frames()
        return _FRAMES[self.name]

    def _frames(self):
        T, H, W, C = self.thwc
        if self.fill == "bytes":
            y0, x0, ch, cw = self.box
            fr = np.zeros(self.thwc, np.uint8)
            n = ch * cw * C
            for t in range(T):
                fr[t, y0:y0 + ch, x0:x0 + cw] = ((np.arange(n) * 37 + 5 * t) % 256).reshape(ch, cw, C)
            return fr
        return np.random.default_rng(zlib.crc32(self.name.encode())).integers(0, 256, self.thwc, dtype=np.uint8)


def _tail(s):
    # 5 x 9 x 11 x 3 = 1485 bytes (1 past a dword); the box is the bottom-right corner: with first + 4 * frame_step = T - 1 the last frame is sampled
    return Case("tail_s%d" % s, (5, 9, 11, 3), (3, 3, 6, 8), (12, 16), (2, -4, 3, 2, 6), shift=s,
                needs=("buf_shift_%d" % s, "buf_end", "buf_bytes_mod4", "first_lt0", "up2"))


CASES = [
    Case("ident255", (20, 12, 24, 3), (2, 3, 8, 16), (8, 16), (2, -3, 8, 1, 16), divisor=255.0, fill="bytes",
         needs=("identity255_all_bytes", "x0c_mod4_1", "first_lt0", "overlap", "t_clip_16", "frame_step_1", "C3")),
    Case("up2_wide", (10, 14, 140, 3), (1, 6, 12, 130), (24, 260), (2, -2, 6, 1, 8), flip=True,
         needs=("ow_gt_256", "up2", "flip_exact", "x0c_mod4_2", "t_clip_8", "first_lt0", "overlap", "ties")),
    Case("up4", (23, 17, 21, 1), (3, 7, 12, 12), (48, 48), (4, 0, 9, 3, 6),
         needs=("up4", "C1", "t_clip_6", "frame_step_3", "buf_bytes_mod4", "ten_two_centres", "clip_past_end")),
    Case("down2", (40, 40, 70, 2), (5, 3, 32, 64), (16, 32), (4, -4, 20, 3, 16), kind="ring",
         needs=("down2", "C2", "clip_past_end", "frame_step_3", "first_lt0", "t_clip_16")),
    Case("down4", (9, 32, 64, 3), (0, 0, 32, 64), (8, 16), (2, -1, 5, 1, 8), kind="ring",
         needs=("down4", "ten_crop_is_frame", "t_clip_8", "overlap")),
    Case("corners", (7, 20, 32, 3), (7, 13, 8, 12), (16, 24), (2, 1, 4, 1, 6), flip=True,
         needs=("ten_corners_disjoint", "x0c_mod4_3", "up2", "t_clip_6", "overlap", "flip_exact")),
    _tail(0), _tail(1), _tail(2), _tail(3),
    Case("c4_up2", (3, 10, 13, 4), (1, 2, 8, 10), (16, 20), (1, 0, 1, 1, 6), entries=("fp32",), flip=True, needs=("C4_fp32",)),
    Case("c4_b", (3, 33, 47, 4), (2, 3, 29, 41), (16, 24), (1, 0, 1, 1, 6), divisor=255.0, kind="bounded", entries=("fp32",), needs=("C4_fp32",)),
    Case("b5", (12, 33, 47, 2), (1, 5, 29, 41), (16, 24), (2, 1, 5, 1, 8), divisor=255.0, kind="bounded",
         needs=("taps_5", "div_255", "C2", "off_centre")),
    Case("b7", (9, 44, 64, 3), (2, 9, 37, 53), (16, 24), (2, -2, 3, 1, 6), divisor=255.0, flip=True, kind="bounded",
         needs=("taps_7", "div_255", "off_centre", "first_lt0", "ten_two_centres")),
    Case("b9", (14, 60, 75, 1), (6, 1, 50, 70), (13, 18), (3, 0, 7, 3, 6), divisor=200.0, kind="bounded",
         needs=("taps_9", "div_200", "C1", "off_centre", "ten_two_centres", "clip_past_end")),
    Case("b_up", (10, 30, 40, 3), (4, 5, 23, 31), (40, 52), (2, -1, 4, 1, 8), divisor=200.0, kind="bounded",
         needs=("bounded_up", "div_200", "off_centre", "first_lt0", "ten_two_centres")),
]


def _samp_live(c):
    n, first, cs, fs, tc = c.samp
    return [[frame_of(i, f, first, cs, fs, tc, c.thwc[0]) for f in range(tc)] for i in range(n)]


def _x0c(c, m):
    return (c.box[1] * c.C) % 4 == m and (c.thwc[2] * c.C) % 4 == 0 and c.shift == 0          # every row of the box starts m bytes past a dword


def _ratio(c, num, den):
    return c.box[2] * num == c.out[0] * den and c.box[3] * num == c.out[1] * den


def _taps(c, n):
    return c.kind == "bounded" and aa_taps(c.box[2], c.out[0]) == n and aa_taps(c.box[3], c.out[1]) == n


def _bytes(c):
    return int(np.prod(c.thwc))


# what the table must hold; each predicate is checked on the cases that claim it, and every property needs a case
PROPERTIES = {
    "identity255_all_bytes": lambda c: c.divisor == 255.0 and c.kind == "exact" and _ratio(c, 1, 1) and c.fill == "bytes" and all(
        len(np.unique(f[c.box[0]:c.box[0] + c.box[2], c.box[1]:c.box[1] + c.box[3]])) == 256 for f in c.frames()),
    "ow_gt_256": lambda c: c.out[1] >= 260 and c.kind == "exact",
    "up2": lambda c: c.kind == "exact" and _ratio(c, 2, 1) and c.divisor == 256.0,
    "up4": lambda c: c.kind == "exact" and _ratio(c, 4, 1) and c.divisor == 256.0,
    "down2": lambda c: c.kind == "ring" and _ratio(c, 1, 2) and c.divisor == 256.0,
    "down4": lambda c: c.kind == "ring" and _ratio(c, 1, 4) and c.divisor == 256.0,
    "flip_exact": lambda c: c.flip and c.kind == "exact",
    "ties": lambda c: c.kind == "exact" and _ratio(c, 2, 1),
    "x0c_mod4_1": lambda c: _x0c(c, 1), "x0c_mod4_2": lambda c: _x0c(c, 2), "x0c_mod4_3": lambda c: _x0c(c, 3),
    "C1": lambda c: c.C == 1 and c.entries == ENTRIES, "C2": lambda c: c.C == 2 and c.entries == ENTRIES, "C3": lambda c: c.C == 3 and c.entries == ENTRIES,
    "C4_fp32": lambda c: c.C == 4 and c.entries == ("fp32",),
    "first_lt0": lambda c: c.samp[1] < 0 and any(s is not None for s in _samp_live(c)[0]) and _samp_live(c)[0][0] is None,
    "t_clip_16": lambda c: c.samp[4] == 16, "t_clip_8": lambda c: c.samp[4] == 8, "t_clip_6": lambda c: c.samp[4] == 6,
    "overlap": lambda c: c.samp[0] > 1 and c.samp[2] < c.samp[4] * c.samp[3],
    "clip_past_end": lambda c: all(s is None for s in _samp_live(c)[-1]) and c.samp[1] + (c.samp[0] - 1) * c.samp[2] >= c.thwc[0],
    "frame_step_1": lambda c: c.samp[3] == 1, "frame_step_3": lambda c: c.samp[3] == 3,
    "buf_shift_0": lambda c: c.shift == 0 and _bytes(c) % 4 != 0, "buf_shift_1": lambda c: c.shift == 1, "buf_shift_2": lambda c: c.shift == 2,
    "buf_shift_3": lambda c: c.shift == 3,
    "buf_end": lambda c: c.box[0] + c.box[2] == c.thwc[1] and c.box[1] + c.box[3] == c.thwc[2] and c.thwc[0] - 1 in _samp_live(c)[0],
    "buf_bytes_mod4": lambda c: _bytes(c) % 4 != 0,
    "ten_two_centres": lambda c: (c.thwc[2] - c.box[3]) % 2 == 1 and "ten" in c.entries,
    "ten_crop_is_frame": lambda c: c.box[2:] == c.thwc[1:3] and "ten" in c.entries,
    "ten_corners_disjoint": lambda c: 2 * c.box[2] <= c.thwc[1] and 2 * c.box[3] <= c.thwc[2] and "ten" in c.entries,
    "taps_5": lambda c: _taps(c, 5), "taps_7": lambda c: _taps(c, 7), "taps_9": lambda c: _taps(c, 9),
    "bounded_up": lambda c: c.kind == "bounded" and c.out[0] > c.box[2] and c.out[1] > c.box[3],
    "div_255": lambda c: c.kind == "bounded" and c.divisor == 255.0, "div_200": lambda c: c.kind == "bounded" and c.divisor == 200.0,
    "off_centre": lambda c: c.kind == "bounded" and (c.box[0], c.box[1]) != (int(round((c.thwc[1] - c.box[2]) / 2.0)), int(round((c.thwc[2] - c.box[3]) / 2.0))),
}


def case(name):
    return next(c for c in CASES if c.name == name)


# ---- the interval of every element, per entry --------------------------------------------------------------------------------------------------------------------
def _ends(c, box, flip, wrong=None):
    """(ref, lo, hi) of one box, each (T, C, oh, ow): lo = hi = ref on exact elements, ref * (1 -+ k * 2^-24) on bounded ones."""
    ref = resample64(c.frames(), box, c.out, c.divisor, flip, wrong)
    if c.kind == "exact":
        return ref, ref, ref
    k = bound_k(box, c.out)
    lo, hi = ref * (1.0 - k * EPS), ref * (1.0 + k * EPS)
    if c.kind == "ring":
        inner = torch.zeros(ref.shape[2:], dtype=torch.bool)
        inner[1:-1, 1:-1] = True
        lo, hi = torch.where(inner, ref, lo), torch.where(inner, ref, hi)
    return ref, lo, hi


_CACHE = {}


def ends(c, entry, wrong=None):
    """(ref, lo, hi) in the entry's output layout, unrounded float64; computed once per (case, entry) and shared."""
    key = (c.name, entry, wrong)
    if key not in _CACHE:
        samp = c.samp_of(entry)
        if entry == "ten":
            boxes = ten_crop_boxes64(c.thwc[1], c.thwc[2], c.box[2], c.box[3], wrong)
            per = [_ends(c, (y, x, c.box[2], c.box[3]), fl, wrong) for y, x, fl in boxes]
            _CACHE[key] = tuple(ten_crop64([p[i] for p in per], samp, wrong) for i in range(3))
        else:
            e = _ends(c, c.box, c.flip, wrong)
            if entry == "fp32":
                _CACHE[key] = e
            elif entry == "rec":
                _CACHE[key] = tuple(records64(x, samp, wrong) for x in e)
            else:
                _CACHE[key] = tuple(act64(x, samp, int(entry[3]), wrong) for x in e)
    return _CACHE[key]


def interval(c, entry, dtype=None):
    """(lo, hi) as the kernel's output type holds them: fp32 entry -> the float64 ends themselves; 16-bit -> each end rounded once."""
    _, lo, hi = ends(c, entry)
    if entry == "fp32":
        return lo, hi
    if c.kind == "exact":
        r = K.round_once(lo, dtype)                                         # the exactness check included
        return r, r
    return round16(lo, dtype), round16(hi, dtype)


def produce(c, entry, dtype=None, wrong=None):
    """What a kernel with the given mistake would return: the (wrong) reference rounded to the output type."""
    ref = ends(c, entry, None if wrong == "trunc16" else wrong)[0]
    if entry == "fp32":
        return ref.to(torch.float32).to(D)
    return round16(ref, dtype, wrong)


def verdict(c, entry, dtype, got):
    """'' if every element of `got` (float64) lies in its interval, else the count of offenders and the first one. THE comparison of both test files."""
    lo, hi = interval(c, entry, dtype)
    assert got.shape == lo.shape, (got.shape, lo.shape)
    bad = ~((got >= lo) & (got <= hi))                                      # a NaN is an offender
    if not bool(bad.any()):
        return ""
    idx = tuple(int(i) for i in bad.nonzero()[0])
    return "%s %s %s: %d of %d outside; first at %s: got %r, interval [%r, %r]" % (c.name, entry, dtype, int(bad.sum()), bad.numel(), idx, float(got[idx]),
                                                                                  float(lo[idx]), float(hi[idx]))


def worst_units(c, entry, got):
    """The worst |got - ref| / (ref * 2^-24) over the bounded elements of an fp32 output, beside the case's k (0 if there is no bounded element)."""
    ref, lo, hi = ends(c, entry)
    m = (lo != hi) & (ref > 0)
    if not bool(m.any()):
        return 0.0
    return float(((got - ref).abs()[m] / (ref[m] * EPS)).max())


# ---- the Pillow forms ------------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class PilCase:
    name: str
    thwc: tuple
    box: tuple
    out: tuple
    samp: tuple                      # first >= 0: the Pillow activation entry refuses frames in front of the video

    def frames(self):
        """Random bytes; frame 1 is a smooth ramp (the fixed-point ties)."""
        T, H, W, C = self.thwc
        fr = np.random.default_rng(zlib.crc32(self.name.encode())).integers(0, 256, self.thwc, dtype=np.uint8)
        fr[1] = (np.add.outer(np.arange(H), np.arange(W))[..., None] * (np.arange(C) + 1)) % 256
        return fr


PIL_CASES = [
    PilCase("pil_wide", (9, 30, 140, 3), (3, 5, 20, 131), (24, 264), (2, 1, 4, 1, 6)),        # off-centre, non-square, 264 columns, overlapping clips
    PilCase("pil_c1", (14, 50, 70, 1), (6, 1, 41, 57), (16, 24), (3, 0, 7, 3, 8)),            # one channel, 7 taps, frame_step 3, the last clip wholly past the end
    PilCase("pil_sq", (20, 21, 33, 3), (2, 9, 19, 23), (32, 48), (2, 2, 8, 1, 16)),           # up-sampling, t_clip 16, 99-byte rows: every alignment
]

_PIL = {}


def pil_ref(c, cpad=None):
    """Pillow's result: (T, C, oh, ow), or with `cpad` the activation of the case's sampling."""
    if c.name not in _PIL:
        _PIL[c.name] = pil_resample(c.frames(), c.box, c.out)
    return _PIL[c.name] if cpad is None else act64(_PIL[c.name], c.samp, cpad)
