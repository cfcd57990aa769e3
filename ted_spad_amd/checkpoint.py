"""Checkpoints with the reference scripts' own dict keys, so that its loaders (and model_loaders.load_*_model here) read them back.

    save_anonymizer_checkpoint(path, epoch, fa, fb, ft, optimizers=None)   anonymization_training/train_anonymizer.py:511-550
    save_action_checkpoint(path, epoch, ft, optimizer, loss_scale)         action_training/train_anonymized_action.py:388-414
    save_reconstruction_checkpoint(path, epoch, lr_counter, fa, optimizer) fa_pretraining/train_reconstruction.py:179-196

`epoch` is stored as `epoch + 1`, as the scripts do. The action script stores its `GradScaler` object under 'amp_scaler'; here the key holds a plain
dict (a file torch.load reads with weights_only=True): {'scale': loss_scale} for the drivers with a static loss scale, the `state_dict()` of the
optim.DynamicLossScale (GradScaler.state_dict()'s keys) for ActionTrainStep (`scaler=`).
"""
from __future__ import annotations

import torch


def save_anonymizer_checkpoint(path, epoch, fa, fb, ft, optimizers=None):
    """optimizers: None (`model_temp.pth` / best-accuracy files, :519-536) or (optimizer_fa, optimizer_fb, optimizer_ft) (every third
    epoch, :541-550). fb None (AnonymizerTrainStep without a privacy branch, whose `opt_fb` is None too): the file has no fb keys."""
    states = {"epoch": epoch + 1, "fa_model_state_dict": fa.state_dict()}
    if fb is not None:
        states["fb_model_state_dict"] = fb.state_dict()
    states["ft_model_state_dict"] = ft.state_dict()
    if optimizers is not None:
        opt_fa, opt_fb, opt_ft = optimizers
        states["optimizer_fa"] = opt_fa.state_dict()
        if opt_fb is not None:
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


def save_action_checkpoint(path, epoch, ft, optimizer, loss_scale, scaler=None):
    """scaler: an optim.DynamicLossScale (ActionTrainStep.scaler): 'amp_scaler' then holds its `state_dict()` -- the keys of GradScaler.state_dict(), what
    `GradScaler.load_state_dict` takes -- and `loss_scale` is not looked at. Without it the file is what it always was. `optimizer` may be a torch.optim
    optimizer or an optim.FusedOptimizer: both write torch's state_dict layout."""
    states = {
        "epoch": epoch + 1,
        "amp_scaler": {"scale": float(loss_scale)} if scaler is None else scaler.state_dict(),
        "ft_model_state_dict": ft.state_dict(),
        "optimizer": optimizer.state_dict(),
    }
    torch.save(states, path)
    return states
