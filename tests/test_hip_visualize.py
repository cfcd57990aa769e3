"""-m gpu: the pictures of the anonymizer on MI355X (ted_spad_amd/visualize.py, csrc/action_eval.hip) -- the save_image grid and the
save_video frames, each exactly equal to an fp32 numpy restatement of the layout and arithmetic the header documents."""
import numpy as np
import pytest
import torch

from ted_spad_amd.synth import synth_state_dict, synth_tensor

pytestmark = pytest.mark.gpu


def _grid_ref(x, nrow, pad):
    """make_grid + mul(255).add_(0.5).clamp_(0, 255).to(uint8) in numpy fp32: two separately rounded operations, HWC."""
    n, _, h, w = x.shape
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    grid = np.zeros((ymaps * (h + pad) + pad, xmaps * (w + pad) + pad, 3), dtype=np.uint8)
    for k in range(n):
        r0, c0 = (k // xmaps) * (h + pad) + pad, (k % xmaps) * (w + pad) + pad
        v = x[k].transpose(1, 2, 0) * np.float32(255)
        v = v + np.float32(0.5)
        assert v.dtype == np.float32
        grid[r0:r0 + h, c0:c0 + w] = np.clip(v, 0, 255).astype(np.uint8)
    return grid


def _grid_values(n, h, w):
    """[-0.5, 1.5] noise with exact k / 255 and (k + 0.5) / 255 points (the rounding boundaries of x * 255 + 0.5) written over its start."""
    x = synth_tensor(0, "grid_%d_%d_%d" % (n, h, w), (n, 3, h, w), -0.5, 1.5).numpy().copy()
    k = np.arange(256, dtype=np.float32)
    pts = np.concatenate([k / np.float32(255), (k + np.float32(0.5)) / np.float32(255), np.float32([0.0, 1.0, -0.5, 1.5, -1e-3, 1.002])])
    flat = x.reshape(-1)
    m = min(len(pts), flat.size // 2)
    flat[:m] = pts[:m]
    flat[-m:] = pts[-m:]
    return x


@pytest.mark.parametrize("n,h,w,nrow", [(2, 5, 7, 1), (3, 5, 7, 2), (4, 64, 64, 2), (32, 16, 16, 16)])
def test_image_grid_exact(n, h, w, nrow):
    from ted_spad_amd.visualize import image_grid_u8
    x = _grid_values(n, h, w)
    for pad in (5, 0):
        got = image_grid_u8(torch.from_numpy(x).cuda(), nrow=nrow, padding=pad)
        ref = _grid_ref(x, nrow, pad)
        assert got.dtype == torch.uint8 and tuple(got.shape) == ref.shape
        assert np.array_equal(got.cpu().numpy(), ref)
        if (n, nrow) == (3, 2):
            assert not bool(got[h + pad:, w + pad:].any())           # the last cell is blank


def test_anonymization_grid_is_inputs_over_outputs():
    from ted_spad_amd._lib import TedSpadHipError
    from ted_spad_amd.visualize import anonymization_grid, image_grid_u8
    a, b = _grid_values(4, 16, 16), _grid_values(4, 16, 16)[::-1].copy()
    got = anonymization_grid(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    assert np.array_equal(got.cpu().numpy(), _grid_ref(np.concatenate([a, b]), 4, 5))
    assert tuple(got.shape) == (2 * 21 + 5, 4 * 21 + 5, 3)
    with pytest.raises(TedSpadHipError):
        image_grid_u8(torch.from_numpy(a[:1]).cuda())                # N = 1: outside the supported range


def _frames_ref(x):
    t = x.transpose(0, 2, 3, 1)[..., ::-1]                           # permute(0, 2, 3, 1) of the channel-flipped tensor
    t = (t - t.min()) / (t.max() - t.min())
    assert t.dtype == np.float32
    return (t * 255).astype(np.uint8)


@pytest.mark.parametrize("t,h,w", [(1, 3, 5), (3, 5, 7), (17, 64, 64)])
def test_video_frames_exact(t, h, w):
    from ted_spad_amd.visualize import video_frames_u8
    x = synth_tensor(0, "frames_%d_%d_%d" % (t, h, w), (t, 3, h, w), -1.3, 2.1).numpy()
    got = video_frames_u8(torch.from_numpy(x).cuda())
    ref = _frames_ref(x)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (t, h, w, 3)
    assert ref.max() == 255 and ref.min() == 0
    assert np.array_equal(got.cpu().numpy(), ref)
    const = video_frames_u8(torch.full((t, 3, h, w), 0.37, device="cuda"))
    assert not bool(const.any())                                     # max == min: zeros (0 / 0 in the reference)


def test_anonymized_video_frames_is_the_kernel_on_the_eval_forward():
    from ted_spad_amd.model_loaders import load_fa_model
    from ted_spad_amd.visualize import anonymized_video_frames, video_frames_u8
    fa = load_fa_model(arch="unet")
    fa.load_state_dict(synth_state_dict(fa.state_dict(), 0))
    fa = fa.cuda().train()
    frames = synth_tensor(0, "anon_frames", (5, 3, 64, 64)).cuda()
    got = anonymized_video_frames(fa, frames)
    assert not fa.training
    with torch.no_grad():
        out = fa.eval()(frames)
    assert tuple(got.shape) == (5, 64, 64, 3) and torch.equal(got, video_frames_u8(out))
    assert np.array_equal(got.cpu().numpy(), _frames_ref(out.cpu().numpy()))


def test_save_png_round_trip(tmp_path):
    from ted_spad_amd.visualize import image_grid_u8, save_png
    grid = image_grid_u8(torch.from_numpy(_grid_values(2, 5, 7)).cuda(), nrow=2, padding=5)
    path = str(tmp_path / "grid.png")
    try:
        from PIL import Image
    except ImportError:
        with pytest.raises(RuntimeError, match="Pillow"):            # no Pillow: a clear error, nothing written
            save_png(grid, path)
        return
    save_png(grid, path)
    assert np.array_equal(np.asarray(Image.open(path)), grid.cpu().numpy())
    with pytest.raises(ValueError):
        save_png(grid.float(), path)
