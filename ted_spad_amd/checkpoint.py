"""Checkpoints with the reference scripts' own dict keys, so that its loaders (and model_loaders.load_*_model here) read them back.

    save_anonymizer_checkpoint(path, epoch, fa, fb, ft, optimizers=None)   anonymization_training/train_anonymizer.py:511-550
    save_action_checkpoint(path, epoch, ft, optimizer, loss_scale)         action_training/train_anonymized_action.py:388-414
    save_reconstruction_checkpoint(path, epoch, lr_counter, fa, optimizer) fa_pretraining/train_reconstruction.py:179-196

`epoch` is stored as `epoch + 1`, as the scripts do. The action script stores its `GradScaler` object under 'amp_scaler'; this build has a
static loss scale and no GradScaler, so the key holds the plain dict {'scale': loss_scale} (a file torch.load reads with weights_only=True).
"""
from __future__ import annotations

import torch


def save_anonymizer_checkpoint(path, epoch, fa, fb, ft, optimizers=None):
    """optimizers: None (`model_temp.pth` / best-accuracy files, :519-536) or (optimizer_fa, optimizer_fb, optimizer_ft) (every third
    epoch, :541-550)."""
    states = {
        "epoch": epoch + 1,
        "fa_model_state_dict": fa.state_dict(),
        "fb_model_state_dict": fb.state_dict(),
        "ft_model_state_dict": ft.state_dict(),
    }
    if optimizers is not None:
        opt_fa, opt_fb, opt_ft = optimizers
        states["optimizer_fa"] = opt_fa.state_dict()
        states["optimizer_fb"] = opt_fb.state_dict()
        states["optimizer_ft"] = opt_ft.state_dict()
    torch.save(states, path)
    return states


def save_reconstruction_checkpoint(path, epoch, lr_counter, fa, optimizer):
    """`model_temp.pth` / the best-validation file of fa_pretraining/train_reconstruction.py:179-196: what `load_fa_model(saved_model_file=...)`
    (and train_anonymizer.py through it) starts from."""
    states = {
        "epoch": epoch + 1,
        "lr_counter": lr_counter,
        "fa_model_state_dict": fa.state_dict(),
        "optimizer": optimizer.state_dict(),
    }
    torch.save(states, path)
    return states


def save_action_checkpoint(path, epoch, ft, optimizer, loss_scale):
    states = {
        "epoch": epoch + 1,
        "amp_scaler": {"scale": float(loss_scale)},
        "ft_model_state_dict": ft.state_dict(),
        "optimizer": optimizer.state_dict(),
    }
    torch.save(states, path)
    return states
