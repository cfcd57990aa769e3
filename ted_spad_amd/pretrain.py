"""The first stage of TeD-SPAD on MI355X: pre-training the unet++ anonymizer fa to reproduce its input (fa_pretraining/train_reconstruction.py).

    ReconstructionTrainStep(fa).step(images)        one `train_epoch` batch (:35-49): fa.train(), forward, nn.L1Loss(output, inputs), backward, Adam
    ReconstructionTrainStep.evaluate(images)        one `validation_epoch` batch (:62-78): fa.eval() forward under no_grad + the loss
    ReconstructionSchedule()                        the epoch logic of `train_classifier` (:138-168): warm-up, drop on a rising loss, validation epochs
    auto_loss_scale(numel, dtype)                   the loss scale of a batch shape (below)

The data side is vispr_augment.sample_vispr / center_record / augment_images unchanged (reconstruction_dl.py:78-137 makes the draws and calls of
vispr_dl.py:71-129 in the same order); the picture `validation_epoch` saves (:85-86) is visualize.anonymization_grid; the checkpoint is
checkpoint.save_reconstruction_checkpoint.

The step keeps both ends of the network in 16 bits: UNetPPTrainer.forward(nchw=False) returns the head's channels-last output, ONE kernel
(tedspad_l1_loss_grad_cl) reads it and the fp32 batch and writes the loss and the gradient records the head's wgrad / dgrad consume
(UNetPPTrainer.backward(dl=...)).

Loss scale. The L1 gradient has ONE magnitude, g = loss_scale / numel, at every element. At the script's batch (32 x 3 x 224 x 224 = 4 816 896 elements) the
project's usual scale of 256 gives g = 5.3e-5, below the smallest normal f16 (6.1e-5): gfx950's matrix cores flush subnormal f16 operands (train_step.py), the
head's wgrad and dgrad would read zeros and the step would train nothing without reporting a skip. So the scale follows the batch shape: `auto_loss_scale`
returns the power of two that puts g into the binade [2^-k, 2^(1-k)), k = GRAD_BINADE[dtype]. A power of two that is divided out again in fp32 changes no
mathematics, only which values are representable. DESIGN.md "Reconstruction pre-training" has the measurements behind k.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from .grad_reduce import GradBucketReducer
from .losses import l1_flat, l1_train
from .train_nets import UNetPPTrainer
from .train_step import StepDriver, fused_adam

# fa_pretraining/parameters.py:10-25
DEFAULT_PARAMS = SimpleNamespace(batch_size=32, num_workers=4, learning_rate=1e-3, num_epochs=100, warmup_array=list(np.linspace(0.01, 1, 5) + 1e-9), warmup=5,
                                 scheduled_drop=5, lr_patience=0, hflip=[0], cropping_fac1=[0.8], reso_h=224, reso_w=224)
# train_reconstruction.py:132
VAL_EPOCHS = [1, 3, 5, 10, 12, 15, 20, 25, 30, 35, 40, 45] + [50 + x for x in range(100)]

# g = loss_scale / numel lies in [2^-k, 2^(1-k)). k = 10 by the measurement of scripts/pretrain_scale_probe.py: the candidates 4, 6, 8, 10
# differ in the fourth digit of the gradient error only, 10 is the lowest; 2^-10 is 16 x the smallest normal f16.
GRAD_BINADE = {"f16": 10, "bf16": 10}


def auto_loss_scale(numel: int, dtype: str = "f16") -> float:
    """The power of two S with 2^-k <= S / numel < 2^(1-k), k = GRAD_BINADE[dtype] (pure host arithmetic on integers)."""
    if dtype not in GRAD_BINADE:
        raise ValueError("auto_loss_scale: dtype must be one of %s, got %r" % (sorted(GRAD_BINADE), dtype))
    numel = int(numel)
    if numel < 1:
        raise ValueError("auto_loss_scale: numel must be >= 1, got %d" % numel)
    e = (numel - 1).bit_length()                # 2^(e-1) < numel <= 2^e
    return float(2.0 ** (e - GRAD_BINADE[dtype]))


class ReconstructionSchedule:
    """Learning rate and validation epochs of `train_classifier` (train_reconstruction.py:138-168), one call per statement group:

        for epoch in range(1, params.num_epochs + 1):
            lr = sched.lr_for_epoch(epoch)              # :144-145   -> step.set_lr(lr)
            ... train the epoch ...
            sched.after_train_epoch(train_loss)         # :154-165
            if sched.should_validate(epoch): ...        # :168

    As in the script: the warm-up reads `warmup_array[epoch]` from epoch 1 (element 0 is never used) and, since `lr_flag` is never set, overrides
    an earlier drop while `epoch < warmup`; with `lr_patience = 0` the first epoch whose loss exceeds the best so far divides the lr by `scheduled_drop`
    (and `lr_counter` is back at 0 when the checkpoint stores it)."""

    def __init__(self, params=DEFAULT_PARAMS):
        self.params = params
        self.lr = params.learning_rate                                # :108
        self.lr_flag, self.lr_counter = 0, 0                          # :138-139
        self.train_loss_best = 10000                                  # :140

    def lr_for_epoch(self, epoch: int) -> float:
        p = self.params
        if epoch < p.warmup and self.lr_flag == 0:                    # :144
            self.lr = p.warmup_array[epoch] * p.learning_rate         # :145
        return self.lr

    def after_train_epoch(self, train_loss: float) -> float:
        p = self.params
        if train_loss > self.train_loss_best:                         # :154
            self.lr_counter += 1
        if self.lr_counter > p.lr_patience:                           # :156
            self.lr_counter = 0
            self.lr = self.lr / p.scheduled_drop                      # :158
        if train_loss < self.train_loss_best:                         # :164
            self.train_loss_best = train_loss
        return self.lr

    @staticmethod
    def should_validate(epoch: int) -> bool:
        return epoch in VAL_EPOCHS                                    # :168


class ReconstructionTrainStep(StepDriver):
    check_at_scale_1 = True                     # an automatic scale is 1 for some shapes: the non-finite check runs all the same

    def __init__(self, fa_model, learning_rate: float = 1e-3, loss_scale=None, group=None):
        """fa_model: unetpp.UnetPlusPlus (cuda) -- `load_fa_model(arch='unet++')`, train_reconstruction.py:105. learning_rate: parameters.py:12 (the
        script rewrites it every epoch: `set_lr`). loss_scale: None = `auto_loss_scale` of each batch's shape; a number is used as given."""
        from .unetpp import UnetPlusPlus
        if not isinstance(fa_model, UnetPlusPlus):
            raise TypeError("ReconstructionTrainStep trains the unet++ anonymizer (unetpp.UnetPlusPlus, what train_reconstruction.py:105 builds); got %s"
                            % type(fa_model).__name__)
        self.fixed_scale = None if loss_scale is None else float(loss_scale)
        super().__init__(self.fixed_scale if self.fixed_scale is not None else 1.0)
        self.fa, self.group = fa_model, group
        self.fa_tr = UNetPPTrainer(fa_model)
        self._off_path = self.fa_tr.off_path_params()                 # encoder.layer4 (never run): no gradient
        self.opt = fused_adam(fa_model, learning_rate)                # :123; `set_lr` is :28-29
        self.red = GradBucketReducer(self.fa_tr.grad_buckets(), group, all_params=list(fa_model.parameters()))

    def scale_for(self, images) -> float:
        return self.fixed_scale if self.fixed_scale is not None else auto_loss_scale(images.numel(), self.fa.compute_dtype)

    def step(self, images):
        """images (B,3,H,W) fp32 cuda in [0,1], H and W multiples of 16: input and target. Returns dict(loss=float, skipped=DeviceFlag)."""
        self.fa.train()                                               # :35
        self._begin(images.device, (self.opt,))                       # :43
        self.red.prepare(exclude=self._off_path)
        self.loss_scale = self.scale_for(images)
        y, tape = self.fa_tr.forward(images, nchw=False)              # :45
        loss, dl, _ = l1_train(y, images, self.loss_scale)            # :46 and the first node of :47
        self._post(dict(loss=loss))                                   # :49
        self.fa_tr.backward(tape, dl=dl, on_bucket_done=self.red.bucket_ready)        # :47
        v, skipped = self._end(self.fa_tr, self.red, self.opt, self.fa)                # :48
        return dict(loss=v["loss"], skipped=skipped)

    def evaluate(self, images):
        """One `validation_epoch` batch (:62,75-77): fa.eval() forward under no_grad and the loss. Returns (output (B,3,H,W) fp32 -- exactly
        `fa.eval()(images)` --, loss 0-d fp32 tensor on the device: the flat form of the L1 kernel on those two tensors)."""
        self.fa.eval()                                                # :62
        with torch.no_grad():
            out = self.fa(images)                                     # :76
        return out, l1_flat(out, images)                              # :77
