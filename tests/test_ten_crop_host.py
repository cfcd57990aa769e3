"""CPU: the host side of ten-crop extraction from decoded frames -- the C-ABI entry is declared on both sides, and the refusals that need no GPU:
preprocess.ten_crop_records' (the same exception types as crop_resize_records') and the `crops` parameter of the two extraction drivers."""
import os
import re

import pytest
import torch

from conftest import ROOT


def test_entry_is_declared_in_the_header_and_the_symbol_table():
    from ted_spad_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tedspad_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint32_t\s+tedspad_frames_ten_crop_tp\s*\(", hdr)
    assert "tedspad_frames_ten_crop_tp" in _lib.SYMBOLS
    # the single-crop entry's arguments with (ch, cw, yc, xc) for (y0, x0, ch, cw) and no flip
    one, ten = _lib.SYMBOLS["tedspad_frames_crop_resize_tp"], _lib.SYMBOLS["tedspad_frames_ten_crop_tp"]
    assert ten[0] is one[0] and len(ten[1]) == len(one[1]) - 1
    assert hasattr(_lib.lib(), "tedspad_frames_ten_crop_tp")
    assert _lib.lib().tedspad_abi_version() == 5


class _Stem:
    """The fields of engine.StemPT the record entries read (I3Res50's stem: 5 frames, stride 2, padding 2)."""
    torch_dtype, dtype_code, pad_t, stride_t = torch.float16, 0, 2, 2

    def frame_pairs(self, t_clip):
        return 4


def _raised(fn):
    try:
        fn()
    except Exception as e:      # noqa: BLE001 -- the type is what the test compares
        return type(e)
    return None


def test_ten_crop_records_refuses_what_crop_resize_records_refuses(monkeypatch):
    """A CPU tensor; then, with the device check out of the way (the entries refuse these before anything is launched, so host memory is never touched): a crop
    larger than the frame, an odd output width, an `out` of the wrong shape or dtype."""
    from ted_spad_amd import preprocess
    from ted_spad_amd._lib import TedSpadHipError
    stem, v = _Stem(), torch.zeros((20, 32, 32, 3), dtype=torch.uint8)
    one = lambda box, out_hw, **kw: preprocess.crop_resize_records(v, box, out_hw, stem, 1, **kw)              # noqa: E731
    ten = lambda crop, out_hw, **kw: preprocess.ten_crop_records(v, crop, out_hw, stem, 1, **kw)               # noqa: E731
    assert _raised(lambda: ten((24, 24), (16, 16))) is _raised(lambda: one((4, 4, 24, 24), (16, 16))) is TedSpadHipError      # no CPU path
    monkeypatch.setattr(preprocess, "require_cuda", lambda t, what: None)
    monkeypatch.setattr(preprocess, "_stream_ptr", lambda: None)                  # the null stream: no device to ask for the current one
    assert _raised(lambda: ten((40, 32), (16, 16))) is _raised(lambda: one((0, 0, 40, 32), (16, 16))) is TedSpadHipError      # taller than the frame
    assert _raised(lambda: ten((32, 33), (16, 16))) is _raised(lambda: one((0, 0, 32, 33), (16, 16))) is TedSpadHipError      # wider than the frame
    assert _raised(lambda: ten((32, 32), (16, 15))) is _raised(lambda: one((0, 0, 32, 32), (16, 15))) is TedSpadHipError      # records hold pixel pairs
    wrong_dtype = torch.zeros((10, 4, 16, 2, 8, 24))
    wrong_shape = torch.zeros((1, 4, 16, 2, 8, 24), dtype=torch.float16)          # one crop's records
    assert _raised(lambda: ten((32, 32), (16, 16), out=wrong_dtype)) is ValueError
    assert _raised(lambda: one((0, 0, 32, 32), (16, 16), out=wrong_dtype[:1])) is ValueError
    assert _raised(lambda: ten((32, 32), (16, 16), out=wrong_shape)) is ValueError
    assert _raised(lambda: one((0, 0, 32, 32), (16, 16), out=wrong_shape[:, :3])) is ValueError


class _FaStub:
    compute_dtype, ACT_CPAD = "f16", 4

    def forward_act(self, a):
        raise AssertionError("not reached")


def test_extraction_drivers_refuse_other_crop_counts():
    from ted_spad_amd import extraction
    frames = torch.zeros((32, 24, 32, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="crops"):
        extraction.extract_video_features_uint8(object(), frames, out_hw=(16, 16), crops=3)
    with pytest.raises(ValueError, match="crops"):
        extraction.extract_anonymized_video_features_uint8(object(), _FaStub(), frames, out_hw=(16, 16), crops=3)
    with pytest.raises(ValueError, match="flip"):
        extraction.extract_anonymized_video_features_uint8(object(), _FaStub(), frames, out_hw=(16, 16), crops=10, resample="pil")
