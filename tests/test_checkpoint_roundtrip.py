"""CPU (the factory builds its modules without a GPU): ted_spad_amd/checkpoint.py writes the reference scripts' checkpoint layouts
(anonymization_training/train_anonymizer.py:519-550, action_training/train_anonymized_action.py:396-414) and the model factory reads
them back strictly."""
import pytest
import torch
import torch.nn as nn

from ted_spad_amd.checkpoint import save_action_checkpoint, save_anonymizer_checkpoint
from ted_spad_amd.model_loaders import load_fa_model, load_fb_model, load_ft_model
from ted_spad_amd.synth import synth_state_dict
from ted_spad_amd.train_step import fused_adam


@pytest.fixture(scope="module")
def models():
    fa = load_fa_model(arch="unet")
    ft = load_ft_model("largei3d", num_classes=102)
    fb = load_fb_model(arch="r50", ssl=True)                         # train_anonymizer.py:338
    fa.load_state_dict(synth_state_dict(fa.state_dict(), 3))
    ft.load_state_dict(synth_state_dict(ft.state_dict(), 3))
    fb.load_state_dict(synth_state_dict(fb.state_dict(), 3))
    return fa, fb, ft


def _same(model, loaded):
    a, b = model.state_dict(), loaded.state_dict()
    assert list(a.keys()) == list(b.keys())
    for k in a:
        assert torch.equal(a[k], b[k]), k


class _DataParallelNames(nn.Module):
    """State-dict keys as nn.DataParallel gives them ('module.' in front), without needing a device."""

    def __init__(self, module):
        super().__init__()
        self.module = module


def _load_all(path):
    return (load_fa_model(saved_model_file=path, arch="unet"), load_fb_model(arch="r50", saved_model_file=path, ssl=True),
            load_ft_model("largei3d", saved_model_file=path, num_classes=102))


@pytest.mark.parametrize("with_optimizers", [False, True])
def test_anonymizer_checkpoint_round_trip(models, tmp_path, with_optimizers):
    fa, fb, ft = models
    path = str(tmp_path / "model_temp.pth")
    opts = tuple(fused_adam(m, 1e-5) for m in (fa, fb, ft)) if with_optimizers else None
    save_anonymizer_checkpoint(path, 6, fa, fb, ft, optimizers=opts)
    saved = torch.load(path, map_location="cpu")
    keys = {"epoch", "fa_model_state_dict", "fb_model_state_dict", "ft_model_state_dict"}
    assert set(saved) == (keys | {"optimizer_fa", "optimizer_fb", "optimizer_ft"} if with_optimizers else keys)
    assert saved["epoch"] == 7                                       # 'epoch': epoch + 1
    if with_optimizers:
        assert all(saved["optimizer_" + n]["param_groups"][0]["lr"] == 1e-5 for n in ("fa", "fb", "ft"))
    for model, loaded in zip((fa, fb, ft), _load_all(path)):
        _same(model, loaded)


def test_data_parallel_prefixed_checkpoint_still_loads(models, tmp_path):
    fa, fb, ft = models
    path = str(tmp_path / "model_dp.pth")
    save_anonymizer_checkpoint(path, 0, _DataParallelNames(fa), _DataParallelNames(fb), ft)
    saved = torch.load(path, map_location="cpu")
    assert all(k.startswith("module.") for n in ("fa", "fb") for k in saved["%s_model_state_dict" % n])
    _same(fa, load_fa_model(saved_model_file=path, arch="unet"))
    _same(fb, load_fb_model(arch="r50", saved_model_file=path, ssl=True))


def test_action_checkpoint_round_trip(models, tmp_path):
    _, _, ft = models
    path = str(tmp_path / "model_temp.pth")
    opt = fused_adam(ft, 1e-5)
    save_action_checkpoint(path, 11, ft, opt, 256.0)
    saved = torch.load(path, map_location="cpu")
    assert set(saved) == {"epoch", "amp_scaler", "ft_model_state_dict", "optimizer"}
    assert saved["epoch"] == 12 and saved["amp_scaler"] == {"scale": 256.0}
    assert len(saved["optimizer"]["param_groups"][0]["params"]) == len(list(ft.parameters()))
    _same(ft, load_ft_model("largei3d", saved_model_file=path, num_classes=102))
