"""GPU: tedspad_val_clips / tedspad_val_clips_act (csrc/val_clips.hip, ted_spad_amd/val_clips.py) against Pillow itself (tests/val_clips_ref.py), the
activation form against `engine.clip_to_act` of the permuted fp32 batch, and `ActionValidator.evaluate_frames` against `evaluate`. Everything is
BIT-equal (torch.equal): the reference chain runs on 8-bit PIL images and the activation is a re-layout, so there is no tolerance in this file."""
import json
import os
import types

import numpy as np
import pytest
import torch

import augment_ref
import val_clips_ref
from conftest import GOLDEN_DIR
from ted_spad_amd import _lib
from ted_spad_amd import engine as E
from ted_spad_amd import val_clips as V
from ted_spad_amd._lib import TedSpadHipError
from ted_spad_amd.synth import synth_state_dict
from ted_spad_amd.train_step import AnonymizerTrainStep

pytestmark = pytest.mark.gpu

R = V.frame_record
SIZES = [(24, 34), (34, 24), (7, 9)]


def random_video(t, h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(t, h, w, 3)).astype(np.uint8)


@pytest.fixture(scope="module")
def small_videos():
    return [random_video(2, h, w, 3 + i) for i, (h, w) in enumerate(SIZES)]


def check(videos, records, reso):
    """one launch == Pillow, record by record; returns the device result"""
    got = V.val_clips([torch.from_numpy(v).cuda() for v in videos], records, reso)
    ref = val_clips_ref.apply_val_records(videos, records, reso)
    assert got.shape == ref.shape and got.dtype == torch.float32
    got = got.cpu()
    for b in range(ref.shape[0]):
        for k in range(ref.shape[1]):
            assert torch.equal(got[b, k], ref[b, k]), "record (%d, %d): %r, %d values differ" % (b, k, records[b][k], int((got[b, k] != ref[b, k]).sum()))
    return got


def boxes_of_every_kind():
    """(video, box): padded above / below and left / right (the single loader's swapped crops), padded on all four sides, inside, the whole frame"""
    p = types.SimpleNamespace(no_ar_distortion=False)
    out = []
    for v, (h, w) in enumerate(SIZES):
        out += [(v, V.val_box(p, h, w, 0.8, "single")), (v, V.val_box(p, h, w, 0.8, "contrastive")), (v, (0, 0, h, w)),
                (v, (-3, -2, h + 7, w + 6)), (v, (h // 3, w // 4, h // 2, w // 2)), (v, (-2, w // 2, h + 2, w))]
    assert out[0][1] == (-1, 8, 27, 19) and out[6][1] == (8, -1, 19, 27)
    return out


@pytest.mark.parametrize("reso", [(1, 2), (28, 28), (35, 35)], ids=["1x2", "28", "35"])
def test_boxes_scales_and_flags(small_videos, reso):
    """every kind of box on the three frame sizes (7 x 9 -> 28: upscaling), hflip and reverse on and off, in one launch"""
    recs = [R(k % 2, box, video=v, hflip=f, reverse=r) for k, (v, box) in enumerate(boxes_of_every_kind()) for f in (False, True) for r in (False, True)]
    got = check(small_videos, [recs], reso)
    if reso[1] > 2:
        assert not torch.equal(got[0, 0], got[0, 1]) and not torch.equal(got[0, 0], got[0, 2])          # the flags change the picture
        assert torch.equal(got[0, 0].flip(0), got[0, 1]) and torch.equal(got[0, 0].flip(2), got[0, 2])


def test_one_frame_at_280(small_videos):
    """cropping_factor 1: int(224 / 0.8) = 280, more than a workgroup could hold as a frame"""
    check(small_videos, [[R(1, (-1, 8, 27, 19), reverse=True)]], (280, 280))


@pytest.mark.parametrize("ow", [28, 64])
def test_hard_downscale(ow):
    """200 rows -> 7: 59 vertical taps a row; at 64 columns the LDS budget, not the cap, sets the band"""
    video = augment_ref.synthetic_video(1, 200, 9, 4)
    recs = [[R(0, (0, 0, 200, 9)), R(0, (-5, -1, 210, 11), hflip=True), R(0, (40, 2, 150, 5), reverse=True)]]
    band = V.band_height(recs, (7, ow))
    assert (band < 7) == (ow == 64)
    check([video], recs, (7, ow))


def test_heights_around_one_band(small_videos):
    cap = _lib.lib().tedspad_val_clips_band_max()
    for oh in (1, cap, cap + 1, 2 * cap + 3):
        recs = [[R(0, (-1, 8, 27, 19)), R(1, (0, 0, 24, 34), hflip=True)]]
        assert V.band_height(recs, (oh, 28)) == min(cap, oh)
        check(small_videos, recs, (oh, 28))


def test_ragged_batch_into_a_strided_out():
    """three videos of different sizes in one launch, the single loader's records, `out` a strided view: nothing outside the frames is touched"""
    p = types.SimpleNamespace(num_frames=16, fix_skip=2, reso_h=28, reso_w=28, num_modes=5, no_ar_distortion=False, temporal_loss=None,
                              temporal_align=False, temporal_distance=None)
    videos = [augment_ref.synthetic_video(40, 24, 34, 11), augment_ref.synthetic_video(64, 34, 24, 12), augment_ref.synthetic_video(20, 7, 9, 13)]
    records = []
    for v, video in enumerate(videos):
        _, clip = V.sample_val_single(p, *video.shape[:3], mode=v + 1, hflip=v % 2)
        records.append([dict(r, video=v) for r in clip])
    assert len({r["box"] for row in records for r in row}) == 3 and records[0][0]["box"][0] < 0 and records[1][0]["box"][1] < 0
    base = torch.full((3, 18, 3, 30, 33), -7.0, dtype=torch.float32, device="cuda")
    out = base[:, 1:17, :, 1:29, 2:30]
    ret = V.val_clips([torch.from_numpy(v).cuda() for v in videos], records, (28, 28), out=out)
    assert ret is out
    assert torch.equal(out.cpu(), val_clips_ref.apply_val_records(videos, records, (28, 28)))
    mask = torch.ones_like(base, dtype=torch.bool)
    mask[:, 1:17, :, 1:29, 2:30] = False
    assert bool((base[mask] == -7.0).all())


# ---- the activation form ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def act_videos():
    return [torch.from_numpy(random_video(48, 24, 34, 21)).cuda(), torch.from_numpy(random_video(48, 34, 24, 22)).cuda()]


def act_records(n):
    """B = 2: item 0 from the 24 x 34 video, item 1 from the 34 x 24 one, flipped; the boxes change from frame to frame, so the three planes of a
    workgroup have different temporary rows"""
    b0 = [(-1, 8, 27, 19), (0, 0, 24, 34), (-3, -2, 31, 40), (6, 9, 11, 13)]
    b1 = [(8, -1, 19, 27), (0, 0, 34, 24), (2, 3, 30, 20)]
    return [[R(k, b0[k % 4], video=0, reverse=True) for k in range(n)], [R(n - 1 - k, b1[k % 3], video=1, reverse=k % 2 == 0, hflip=True) for k in range(n)]]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("cpad", [4, 8])
@pytest.mark.parametrize("n", [4, 16, 48])
def test_act_equals_clip_to_act_of_the_fed_batch(act_videos, n, cpad, dtype):
    records = act_records(n)
    reso = (28, 28) if n != 16 else (35, 36)
    x = V.val_clips(act_videos, records, reso)                                          # pinned to Pillow above
    want = E.clip_to_act(AnonymizerTrainStep._feed(x)[0].unsqueeze(2), cpad, dtype)
    out = None
    if n == 4:
        out = torch.full(tuple(want.buf.shape), 3.0, dtype=want.buf.dtype, device="cuda")
    got = V.val_clips_act(act_videos, records, reso, cpad, dtype, out=out)
    assert out is None or got.buf is out
    assert (got.c, got.coff, got.cpad) == (want.c, want.coff, want.cpad) and got.buf.shape == want.buf.shape and got.buf.dtype == want.buf.dtype
    assert torch.equal(got.buf.view(torch.int16), want.buf.view(torch.int16))
    assert bool((got.buf.view(torch.int16)[..., 3] == 0).all())                         # the padded channel
    if cpad == 8:
        assert bool((got.buf.view(torch.int16)[..., 3:] == 0).all())


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["single_landscape", "single_portrait", "contrastive_trip", "temporal_distance", "no_ar_distortion", "factor_1",
                                  "factor_1p2", "hflip", "short_20", "clamped_19"])
def test_fixture_clips(name):
    """the clips the reference's loaders returned (tests/golden/make_val_clip_golden.py); twice gives the same bits"""
    with open(os.path.join(GOLDEN_DIR, "val_clip_golden_meta.json")) as f:
        meta = json.load(f)
    case = [c for c in meta["cases"] if c["name"] == name][0]
    clips = torch.from_numpy(np.load(os.path.join(GOLDEN_DIR, "val_clip_golden.npz"))[name + "_clips"])
    params = types.SimpleNamespace(**case["params"])
    t, h, w, _ = case["video"]
    cf = case["cropping_factor"]
    if case["loader"] == "contrastive":
        records = V.sample_val_contrastive(np.random.RandomState(case["seed"]), params, t, h, w, case["mode"], case["hflip"], cf)[1]
    else:
        records = [V.sample_val_single(params, t, h, w, case["mode"], case["hflip"], cf)[1]]
    video = torch.from_numpy(augment_ref.synthetic_video(*case["video"])).cuda()
    reso = V.val_reso(params, cf)
    got = V.val_clips([video], records, reso)
    again = V.val_clips([video], records, reso)
    assert torch.equal(got.cpu(), clips.to(torch.float32).div(255))
    assert torch.equal(got, again)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_entries_refuse_bad_records_and_write_nothing():
    L = _lib.lib()
    video = torch.from_numpy(random_video(4, 24, 34, 0)).cuda()
    records = [[R(k, (-1, 8, 27, 19), hflip=True) for k in range(4)]]
    oh = ow = 28
    out = torch.full((1, 4, 3, oh, ow), -7.0, device="cuda")
    act = torch.full((4, 1, oh, ow // 2, 8), -7.0, dtype=torch.float16, device="cuda")
    blob0, nrec, toff, words = V._build_table("test", [video], records, (oh, ow), lambda b, k: k * 3 * oh * ow)
    dev = torch.empty(blob0.nbytes, dtype=torch.uint8, device="cuda")

    def f32(blob, band=4, reso=(oh, ow), elems=None):
        return L.tedspad_val_clips(blob.ctypes.data, dev.data_ptr(), blob.nbytes, nrec, toff, words, out.data_ptr(), out.numel() if elems is None else elems,
                                   reso[0], reso[1], band, oh * ow, ow, 1, None)

    def a16(blob, n=4, cpad=4, reso=(oh, ow), nbytes=None, dtype=0, band=4):
        return L.tedspad_val_clips_act(blob.ctypes.data, dev.data_ptr(), blob.nbytes, nrec, toff, words, act.data_ptr(),
                                       act.numel() * 2 if nbytes is None else nbytes, n, reso[0], reso[1], band, cpad, dtype, None)

    def poked(**kw):
        blob = blob0.copy()
        rec = blob[:toff].view(V.RECORD)
        for k, v in kw.items():
            rec[2][k] = v
        return blob

    H, W = 24, 34
    bad = [poked(src=0), poked(ch=0), poked(cw=-3), poked(top=H), poked(top=-27), poked(left=W), poked(left=-19),          # no frame; empty; disjoint
           poked(ytab=words), poked(xtab=-1), poked(ytaps=1), poked(ch=20), poked(cw=18),                                   # tables outside the blob / crop
           poked(flags=1), poked(flags=V.HFLIP | 512), poked(reserved=1)]                                                  # unknown flags
    for i, blob in enumerate(bad):
        assert f32(blob) == -1, i
        assert b"record 2" in L.tedspad_last_error(), i
        assert a16(blob) == -1, i
        assert b"record 2" in L.tedspad_last_error(), i
    assert f32(poked(dst=out.numel())) == -1 and f32(poked(dst=-1)) == -1 and f32(blob0, elems=out.numel() - 1) == -1     # a destination outside out
    assert f32(blob0, band=0) == -1 and f32(blob0, band=L.tedspad_val_clips_band_max() + 1) == -1
    zero_dst = blob0.copy()
    zero_dst[:toff].view(V.RECORD)["dst"] = 0
    assert a16(blob0) == -1 and b"destination" in L.tedspad_last_error()                 # the activation form places the images itself
    assert a16(zero_dst, n=3) == -1 and b"batch items" in L.tedspad_last_error()         # items with differing n cannot be 4 records
    assert a16(zero_dst, nbytes=act.numel() * 2 - 16) == -1                              # a destination outside out
    assert a16(zero_dst, cpad=6) == -1 and a16(zero_dst, dtype=2) == -1
    odd, _, otoff, owords = V._build_table("test", [video], records, (oh, 27), lambda b, k: 0)
    assert L.tedspad_val_clips_act(odd.ctypes.data, dev.data_ptr(), odd.nbytes, nrec, otoff, owords, act.data_ptr(), act.numel() * 2, 4, oh, 27, 4, 4, 0,
                                   None) == -1 and b"even" in L.tedspad_last_error()     # odd width with pixel pairs
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((act == -7.0).all())
    # and the same blobs, unpoked, run
    assert f32(blob0) == 0 and a16(zero_dst) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, V.val_clips([video], records, (oh, ow)))
    assert torch.equal(act.view(torch.int16), V.val_clips_act([video], records, (oh, ow), 4, "f16").buf.view(torch.int16))


def test_launchers_refuse_bad_arguments():
    video = torch.from_numpy(random_video(2, 24, 34, 0)).cuda()
    ok = [[R(0, (-1, 8, 27, 19)), R(1, (0, 0, 24, 34))]]
    out = torch.full((1, 2, 3, 28, 28), -7.0, device="cuda")
    with pytest.raises(ValueError):
        V.val_clips([video], [[R(0, (0, 0, 24, 34))], ok[0]], (28, 28))                 # batch items with differing n
    with pytest.raises(ValueError):
        V.val_clips_act([video], [[R(0, (0, 0, 24, 34))], ok[0]], (28, 28), 4, "f16")
    with pytest.raises(ValueError):
        V.val_clips([video], [[R(0, (0, 0, 0, 34)), R(1, (0, 0, 24, 34))]], (28, 28), out=out)          # empty box
    with pytest.raises(ValueError):
        V.val_clips([video], [[R(2, (0, 0, 24, 34)), R(1, (0, 0, 24, 34))]], (28, 28), out=out)         # frame outside the video
    with pytest.raises(ValueError):
        V.val_clips([video], [[R(0, (0, 0, 24, 34), contrast=1.1), R(1, (0, 0, 24, 34))]], (28, 28), out=out)
    with pytest.raises(ValueError):
        V.val_clips([video.float()], ok, (28, 28), out=out)
    with pytest.raises(ValueError):
        V.val_clips([video], ok, (28, 28), out=out[..., :27])
    with pytest.raises(ValueError):
        V.val_clips_act([video], ok, (28, 27), 4, "f16")                                # odd width with pixel pairs
    with pytest.raises(ValueError):
        V.val_clips_act([video], ok, (28, 28), 4, "f16", out=torch.zeros((2, 1, 28, 14, 8), device="cuda"))          # fp32 out
    with pytest.raises(TedSpadHipError, match="no CPU path"):
        V.val_clips([video.cpu()], ok, (28, 28), out=out)
    with pytest.raises(TedSpadHipError, match="does not intersect"):
        V.val_clips([video], [[R(0, (24, 0, 5, 5)), R(1, (0, 0, 24, 34))]], (28, 28), out=out)          # a box below the frame
    with pytest.raises(TedSpadHipError, match="does not intersect"):
        V.val_clips([video], [[R(0, (0, -9, 5, 9)), R(1, (0, 0, 24, 34))]], (28, 28), out=out)          # a box left of it
    tall = torch.zeros((1, 4000, 8, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(TedSpadHipError, match="LDS"):
        V.val_clips([tall], [[R(0, (0, 0, 4000, 8))]], (1, 8))                          # one output row's taps exceed the budget: refused, not clamped
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    V.val_clips([video], ok, (28, 28), out=out)                                         # and the good call still runs
    assert bool((out != -7.0).all())
    V.val_clips_act([video], ok, (28, 27), 8, "f16")                                    # cpad 8 takes an odd width


# ---- ActionValidator.evaluate_frames ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets():
    from ted_spad_amd.model_loaders import load_fa_model, load_ft_model
    fa = load_fa_model(arch="unet")
    ft = load_ft_model("largei3d", num_classes=102)
    fa.load_state_dict(synth_state_dict(fa.state_dict(), 0))
    ft.load_state_dict(synth_state_dict(ft.state_dict(), 0))
    fa, ft = fa.cuda().eval(), ft.cuda().eval()
    p = types.SimpleNamespace(num_frames=16, fix_skip=2, reso_h=64, reso_w=64, num_modes=5, no_ar_distortion=False, temporal_loss="trip",
                              temporal_align=False, temporal_distance=None)
    videos = [augment_ref.synthetic_video(64, 80, 100, 31), augment_ref.synthetic_video(64, 96, 72, 32)]      # 64 frames: any third start fits
    records = []
    for v, video in enumerate(videos):
        _, clips = V.sample_val_contrastive(np.random.RandomState(v), p, *video.shape[:3], mode=1 + v)
        records.append([dict(r, video=v) for clip in clips for r in clip])
    assert len(records[0]) == len(records[1]) == 48
    return fa, ft, [torch.from_numpy(v).cuda() for v in videos], records


PATHS = ["/data/ucf/mode0/v_Walk_g01_c01.avi", "/data/ucf/mode0/v_Run_g02_c03.avi"]


@pytest.mark.parametrize("with_fa", [True, False], ids=["fa", "raw"])
def test_evaluate_frames_equals_evaluate(nets, with_fa):
    from ted_spad_amd.action_eval import ActionValidator
    fa, ft, videos, records = nets
    a, b = ActionValidator(ft, fa if with_fa else None), ActionValidator(ft, fa if with_fa else None)
    labels = [7, 55]
    x = V.val_clips(videos, records, (64, 64))
    ra = a.evaluate(x, labels, PATHS)
    rb = b.evaluate_frames(videos, records, labels, PATHS, (64, 64))
    assert ra["logits"].shape == (2, 102) and bool(torch.isfinite(ra["logits"]).all())
    for k in ("logits", "probs", "loss", "pred"):
        assert torch.equal(ra[k], rb[k]), k
    pa, pb = a.end_pass(), b.end_pass()
    assert pa == pb and pb["num_videos"] == 2
    assert torch.equal(a.counts, b.counts) and a.counts.tolist() == [1, 1]
    if with_fa:
        raw = ActionValidator(ft, None).evaluate(x, labels, PATHS)
        assert not torch.equal(raw["logits"], rb["logits"])                             # the anonymizer is in the path
