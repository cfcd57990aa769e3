"""Pictures of what the anonymizer does, on MI355X.

    anonymization_grid(inputs, outputs, padding=5)   the per-epoch grid of `val_visualization_fa_vispr` (anonymization_training/
                                                     train_anonymizer.py:305-315): save_image(cat([inputs, outputs]), padding=5, nrow=B)
    anonymized_video_frames(fa_model, frames)        the frames `anonymize_videos` writes (visualization/visualize_anonymization.py:
                                                     104-111 and save_video, :52-59)
    save_png(array, path)                            the file, through Pillow

Both return uint8 HWC tensors on the device, bit-equal to the fp32 arithmetic of torch (grid) and numpy (video). torchvision is not part of
this build: the grid layout is pinned to its published make_grid (DESIGN.md "Validation, pictures, checkpoints").
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .engine import _stream_ptr, require_cuda


def image_grid_u8(images, nrow: int = 8, padding: int = 2):
    """(N, 3, H, W) fp32 cuda, N >= 2 -> uint8 (Hg, Wg, 3): torchvision's save_image defaults otherwise (pad_value 0, no normalize)."""
    require_cuda(images, "image_grid_u8")
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError("image_grid_u8: images must be (N, 3, H, W), got %s" % (tuple(images.shape),))
    x = images.contiguous().float()
    n, _, h, w = x.shape
    hg, wg = C.c_int32(0), C.c_int32(0)
    _lib.check(_lib.lib().tedspad_image_grid_dims(n, h, w, int(nrow), int(padding), C.byref(hg), C.byref(wg)), "tedspad_image_grid_dims")
    out = torch.empty(hg.value, wg.value, 3, dtype=torch.uint8, device=x.device)
    _lib.check(_lib.lib().tedspad_image_grid_u8(x.data_ptr(), out.data_ptr(), n, h, w, int(nrow), int(padding), _stream_ptr()), "tedspad_image_grid_u8")
    return out


def anonymization_grid(inputs, outputs, padding: int = 5):
    """Row of inputs over the row of their anonymised versions: cat([inputs, outputs]) with nrow = B (train_anonymizer.py:313-314)."""
    if inputs.shape != outputs.shape:
        raise ValueError("anonymization_grid: inputs %s and outputs %s differ in shape" % (tuple(inputs.shape), tuple(outputs.shape)))
    return image_grid_u8(torch.cat([inputs, outputs], dim=0), nrow=int(inputs.shape[0]), padding=padding)


def video_frames_u8(video):
    """(T, 3, H, W) fp32 cuda -> uint8 (T, H, W, 3), channels reversed, normalised by the min and max of the WHOLE video:
    ((x - min) / (max - min) * 255).astype(uint8) in fp32 (save_video after torch.flip(dims=[1])). A constant video (0 / 0 in the
    reference) gives zeros."""
    require_cuda(video, "video_frames_u8")
    if video.dim() != 4 or video.shape[1] != 3:
        raise ValueError("video_frames_u8: video must be (T, 3, H, W), got %s" % (tuple(video.shape),))
    x = video.contiguous().float()
    t, _, h, w = x.shape
    lib = _lib.lib()
    ws = torch.empty(lib.tedspad_minmax_ws_floats(), dtype=torch.float32, device=x.device)
    mm = torch.empty(2, dtype=torch.float32, device=x.device)
    _lib.check(lib.tedspad_minmax_f32(x.data_ptr(), x.numel(), ws.data_ptr(), mm.data_ptr(), _stream_ptr()), "tedspad_minmax_f32")
    out = torch.empty(t, h, w, 3, dtype=torch.uint8, device=x.device)
    _lib.check(lib.tedspad_video_frames_u8(x.data_ptr(), mm.data_ptr(), out.data_ptr(), t, h, w, _stream_ptr()), "tedspad_video_frames_u8")
    return out


def anonymized_video_frames(fa_model, frames):
    """frames (T, 3, H, W) fp32 cuda in [0, 1] -> the uint8 (T, H, W, 3) frames of the anonymised video (visualize_anonymization.py:104-111)."""
    require_cuda(frames, "anonymized_video_frames")
    fa_model.eval()                                                   # :47
    with torch.no_grad():
        out = fa_model(frames)                                        # :105
    return video_frames_u8(out)                                       # :108 (flip) + :54-59


def save_png(array, path):
    """Writes a uint8 (H, W, 3) tensor / array as a PNG (what save_image's last step does, through Pillow as there)."""
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("save_png needs Pillow (PIL), which does not import here: %s. The uint8 array itself is complete -- "
                           "write it with any image library." % e)
    if isinstance(array, torch.Tensor):
        array = array.cpu().numpy()
    if array.dtype.name != "uint8" or array.ndim != 3 or array.shape[2] != 3:
        raise ValueError("save_png: expected uint8 (H, W, 3), got %s %s" % (array.dtype, array.shape))
    Image.fromarray(array).save(path, format="PNG")
