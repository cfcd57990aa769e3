"""CPU: ActionSchedule against sequences derived by hand from action_training/train_action.py:268-326,414 (the loop's learning-rate logic)."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

from ted_spad_amd.train_step import DEFAULT_ACTION_PARAMS, ActionSchedule

LR0 = 1e-4


def _params(**kw):
    return SimpleNamespace(**{**vars(DEFAULT_ACTION_PARAMS), **kw})


def _run(sched, losses, epochs):
    """lr of every epoch; `losses` is a function epoch -> train loss or a list (the loss of epoch e is losses[e - 1])"""
    lrs, stops = [], []
    for e in epochs:
        lrs.append(float(sched.lr_for_epoch(e)))
        stops.append(sched.end_epoch(losses(e) if callable(losses) else losses[e - 1]))
    return lrs, stops


def test_cosine_is_the_default_and_never_stops():
    p = DEFAULT_ACTION_PARAMS
    assert p.lr_scheduler == "cosine" and p.learning_rate == LR0 and len(p.cosine_lr_array) == p.num_epochs == 100
    s = ActionSchedule(p)
    assert list(s.epochs()) == list(range(1, 101))
    lrs, stops = _run(s, lambda e: 3.0 / e, s.epochs())
    assert np.allclose(lrs[:5], np.linspace(0.01, 1, 5) * LR0, rtol=1e-15)            # :300-301, params_action.py:40
    assert lrs[5] == LR0                                                              # (cos 0 + 1) / 2
    assert lrs[99] == pytest.approx((math.cos(math.pi / 0.99) + 1) / 2 * LR0, rel=1e-12)
    assert lrs == [c * LR0 for c in p.cosine_lr_array]
    assert not any(stops) and not s.should_stop
    # a tiny base rate would meet the stop rule's numbers; under cosine the rule is not applied (:414)
    s = ActionSchedule(_params(learning_rate=1e-14))
    assert not any(_run(s, lambda e: 1.0, range(1, 30))[1])


def test_patience_based_without_warmup_halves_every_second_epoch():
    # scheduler_epoch grows every epoch (no positive loss is < best_score = 0); the drop fires when it EQUALS lr_patience and resets it
    s = ActionSchedule(_params(lr_scheduler="patience_based", warmup=0, lr_patience=2, lr_reduce_factor=2))
    lrs, _ = _run(s, lambda e: 0.5 + 1.0 / e, range(1, 9))
    assert lrs == [LR0, LR0, LR0 / 2, LR0 / 2, LR0 / 4, LR0 / 4, LR0 / 8, LR0 / 8]


def test_patience_based_behind_the_default_warmup_never_drops():
    p = _params(lr_scheduler="patience_based")
    s = ActionSchedule(p)
    lrs, stops = _run(s, lambda e: 2.0, range(1, 41))
    assert lrs[:10] == [w * LR0 for w in p.warmup_array] and np.allclose(lrs[:10], (np.linspace(0.01, 1, 10) + 1e-9) * LR0, rtol=1e-15)
    # from epoch 11 no branch assigns the rate (the counter stands at 10 when `== lr_patience` is first tested, and only grows): the last warm-up value persists
    assert lrs[10:] == [p.warmup_array[-1] * LR0] * 30 and lrs[10] == pytest.approx(LR0 * (1 + 1e-9), rel=1e-15) and lrs[10] != LR0
    assert s.scheduler_epoch == 40 and s.scheduler_step == 1 and not any(stops)


def test_loss_based_follows_the_last_loss_and_never_raises_the_rate():
    s = ActionSchedule(_params(lr_scheduler="loss_based", warmup=0))
    lrs, _ = _run(s, [1000, 0.7, 0.3, 0.05, 2.0, 2.0], range(1, 7))
    assert lrs[0] == LR0                                                              # train_loss starts at 1000 (:271)
    assert lrs[1:] == [LR0, LR0 / 2, LR0 / 10, LR0 / 20, LR0 / 20]                    # a loss of 2.0 matches no band: the rate stays
    # the warm-up branch comes first: while it lasts the loss is not looked at
    s = ActionSchedule(_params(lr_scheduler="loss_based"))
    lrs, _ = _run(s, lambda e: 0.05, range(1, 13))
    assert lrs[:10] == [w * LR0 for w in s.params.warmup_array] and lrs[10:] == [LR0 / 20] * 2


def test_stop_rule_fires_at_the_first_epoch_past_ten_with_a_rate_below_1e_12():
    # lr0 / 2^k < 1e-12 from k = 27 (1e-4 / 2^27 = 7.5e-13); lr_patience = 1, no warm-up: the counter is back at 1 at the end of
    # every epoch (reset by the drop, then incremented by :326), so the rate halves at every epoch from 2 on: k = e - 1, k = 27 at epoch 28
    s = ActionSchedule(_params(lr_scheduler="patience_based", warmup=0, lr_patience=1, lr_reduce_factor=2))
    lrs, stops = _run(s, lambda e: 1.0, range(1, 61))
    first = stops.index(True) + 1
    assert first == 28 and lrs[first - 1] == LR0 / 2 ** 27 < 1e-12 <= lrs[first - 2]
    # a rate that is below the limit from the start stops only once the epoch exceeds 10
    s = ActionSchedule(_params(lr_scheduler="loss_based", warmup=0, learning_rate=1e-13), start_epoch=3)
    _, stops = _run(s, lambda e: 5.0, s.epochs())
    assert list(s.epochs())[0] == 3 and stops.index(True) == 11 - 3 and all(stops[8:])
