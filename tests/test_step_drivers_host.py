"""The step drivers' class layout (host) and the read-back invariant of StepDriver's begin helper (-m gpu): train_step.StepDriver owns the state and
the step skeleton; AnonymizerTrainStep, ActionTrainStep, privacy.PrivacyTrainStep, pretrain.ReconstructionTrainStep and mgfn.MGFNTrainStep only add to it."""
import inspect

import pytest
import torch


def _driver_classes():
    from ted_spad_amd import mgfn, pretrain, privacy, train_step
    found = []
    for mod in (train_step, privacy, pretrain, mgfn):
        found += [c for _, c in inspect.getmembers(mod, inspect.isclass) if c.__module__ == mod.__name__]
    return found


def test_action_train_step_is_a_step_driver_and_no_anonymizer_step():
    from ted_spad_amd.train_step import ActionTrainStep, AnonymizerTrainStep, StepDriver
    assert issubclass(ActionTrainStep, StepDriver) and issubclass(AnonymizerTrainStep, StepDriver)
    assert not issubclass(ActionTrainStep, AnonymizerTrainStep)
    for phase in ("step_fa", "step_ft", "step_action"):
        assert not hasattr(ActionTrainStep, phase), phase
        assert hasattr(AnonymizerTrainStep, phase), phase
    assert callable(AnonymizerTrainStep._feed) and ActionTrainStep._feed is AnonymizerTrainStep._feed


def test_set_lr_and_unscale_live_in_step_driver_only():
    from ted_spad_amd.train_step import StepDriver
    classes = _driver_classes()
    names = {c.__name__ for c in classes}
    assert {"StepDriver", "AnonymizerTrainStep", "ActionTrainStep", "PrivacyTrainStep", "ReconstructionTrainStep", "MGFNTrainStep"} <= names
    for c in classes:
        if c is not StepDriver:
            assert "set_lr" not in c.__dict__ and "_unscale" not in c.__dict__, c.__name__
    assert "set_lr" in StepDriver.__dict__ and "_unscale" in StepDriver.__dict__


@pytest.mark.gpu
@pytest.mark.parametrize("lazy", [False, True])
def test_begin_drops_what_a_raised_step_left_posted(lazy):
    """A step that raised between `_post` and `_collect` leaves nothing behind: after `_begin` only what the new step posts comes back."""
    from ted_spad_amd.train_step import StepDriver

    class Bare(StepDriver):
        pass

    d = Bare()
    d.lazy_losses = lazy
    d._post(dict(stale_a=torch.tensor(1.5, device="cuda"), stale_b=torch.tensor(2.5, device="cuda")))      # ... and the step raises here
    assert len(d._posted) == 1
    d._begin()
    assert d._posted == [] and d._pin_used == 0
    d._post(dict(fresh=torch.tensor(0.375, device="cuda")))
    got = d._collect()
    assert list(got) == ["fresh"]
    if lazy:
        assert torch.is_tensor(got["fresh"]) and got["fresh"].dim() == 0 and got["fresh"].is_cuda and float(got["fresh"]) == 0.375
    else:
        assert isinstance(got["fresh"], float) and got["fresh"] == 0.375
    assert d._posted == [] and d._pin_used == 0
