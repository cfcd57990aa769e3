"""CPU: the host side of extraction.extract_anonymized_video_features_uint8 -- how many clips the two extraction scripts cut from a video, which crop box
they take, and the refusals that need no GPU."""
import math

import pytest
import torch

LENGTHS = (1, 15, 16, 31, 32, 33, 64, 100)


def _hybrid_val_pipe_count(total_frames, sequence_length=16, stride=2, step=32):
    """fn.readers.video(sequence_length, stride, step, pad_sequences=True) (dali_extraction.py:62-73): a sequence starts at every `step`-th frame of the file,
    and with pad_sequences the starts whose sequence runs past the end are kept (padded with zero frames) instead of dropped."""
    return len([s for s in range(0, total_frames, step)])


def _read_video_clips(total_frames, num_frames=16, skip=2):
    """shanghai_dl.py:48-80 without the decoder and without the `repeat` tail: (fix_skip, [[1-based frame positions of a clip], ...])."""
    fix_skip = 1 if total_frames < skip * num_frames else skip
    full_frame_pos, frame_pos = [], []
    count = 0
    while True:
        count += 1
        ret = count <= total_frames                          # cap.read()
        if not ret:
            break
        if count % fix_skip == 0:
            frame_pos.append(count)
            if count % (num_frames * fix_skip) == 0:
                full_frame_pos.append(frame_pos)
                frame_pos = []
    return fix_skip, full_frame_pos


@pytest.mark.parametrize("t", LENGTHS)
def test_default_clip_count_aa_is_hybrid_val_pipes(t):
    from ted_spad_amd import extraction
    assert extraction.anonymized_video_clips(t, "aa") == _hybrid_val_pipe_count(t) == math.ceil(t / 32)
    assert extraction.anonymized_video_clips(t, "aa", first=0, clip_step=8, frame_step=1, t_clip=16) == _hybrid_val_pipe_count(t, 16, 1, 8)


@pytest.mark.parametrize("t", LENGTHS)
def test_default_clip_count_pil_is_read_videos(t):
    """Called as the docstring says (first = fix_skip - 1, clip_step = 16 * fix_skip), the count and every frame index are read_video's."""
    from ted_spad_amd import extraction
    fix_skip, clips = _read_video_clips(t)
    n = extraction.anonymized_video_clips(t, "pil", first=fix_skip - 1, clip_step=16 * fix_skip, frame_step=fix_skip, t_clip=16)
    assert n == len(clips)
    for i, pos in enumerate(clips):
        assert [fix_skip - 1 + i * 16 * fix_skip + f * fix_skip for f in range(16)] == [p - 1 for p in pos]       # 0-based source frames
    # whole clips only, for any start: one more frame than the last clip needs changes nothing, one fewer drops it
    for first in (0, 1, 5):
        m = extraction.anonymized_video_clips(t, "pil", first=first)
        assert m == len([i for i in range(t) if first + i * 32 + 15 * 2 < t])


def test_clip_count_rejects_bad_sampling():
    from ted_spad_amd import extraction
    with pytest.raises(ValueError):
        extraction.anonymized_video_clips(64, "bicubic")
    with pytest.raises(ValueError):
        extraction.anonymized_video_clips(64, "aa", clip_step=0)


def test_crop_boxes_of_both_resamplers():
    from ted_spad_amd import extraction, preprocess
    # val_augmentations (dali_extraction.py:38-50): int(h * f) x int(w * f), or the square of the shorter side; center_crop's rounding
    assert extraction.anonymized_video_box(240, 320) == (24, 32, 192, 256)
    assert extraction.anonymized_video_box(240, 320, no_ar_distortion=True) == (24, 64, 192, 192)
    assert extraction.anonymized_video_box(241, 321, cropping_factor=0.8) == preprocess.center_crop_box(241, 321, 192, 256)
    assert extraction.anonymized_video_box(120, 160, cropping_factor=1.0) == (0, 0, 120, 160)
    # shanghai_dl.py:27-35: a square from the HEIGHT; with no_ar_distortion min(image.shape) is the channel count
    assert extraction.anonymized_video_box(480, 856, 3, resample="pil") == (48, 236, 384, 384)
    assert extraction.anonymized_video_box(480, 856, 3, no_ar_distortion=True, resample="pil") == (239, 427, 2, 2)
    assert extraction.anonymized_video_box(97, 131, 3, resample="pil") == preprocess.center_crop_box(97, 131, 77, 77)
    with pytest.raises(ValueError):
        extraction.anonymized_video_box(300, 200, 3, resample="pil")          # the height's square is wider than the frame
    with pytest.raises(ValueError):
        extraction.anonymized_video_box(240, 320, resample="nearest")


class _FaStub:
    compute_dtype, ACT_CPAD = "f16", 4

    def forward_act(self, a):
        raise AssertionError("not reached")


def test_cpu_tensors_are_refused():
    from ted_spad_amd import extraction, preprocess
    from ted_spad_amd._lib import TedSpadHipError
    frames = torch.zeros((32, 24, 32, 3), dtype=torch.uint8)
    with pytest.raises(TedSpadHipError):
        extraction.extract_anonymized_video_features_uint8(object(), _FaStub(), frames, out_hw=(16, 16))
    with pytest.raises(TedSpadHipError):
        preprocess.crop_resize_act(frames, (0, 0, 24, 32), (16, 16), 1)
    with pytest.raises(TypeError):
        extraction.extract_anonymized_video_features_uint8(object(), object(), frames, out_hw=(16, 16))    # an anonymizer without forward_act
