"""Validating the action classifier on MI355X: what the reference's scripts run between epochs to decide which checkpoint is kept.

    ActionValidator(ft, fa).evaluate(inputs_video, labels, vid_paths)   one batch of `val_epoch_video` (anonymization_training/
                                                                        train_anonymizer.py:227-272) / `val_epoch`
                                                                        (action_training/train_anonymized_action.py:126-169; with
                                                                        fa_model=None, train_action.py:119-152)
    ActionValidator.evaluate_frames(videos, records, labels, paths, reso)   the same batch from decoded uint8 frames (val_clips.py): with an
                                                                        anonymizer one launch writes its 16-bit input, no fp32 batch
    ActionValidator.end_pass()                                          the end of one (mode, cropping_fac) pass: the two numbers
                                                                        `val_epoch*` returns and the "Running Avg Accuracy" line
                                                                        (train_anonymizer.py:281-301,475-488)
    ActionValidator.result()                                            the epoch's numbers (train_anonymizer.py:490-509)

Behind the ft forward a batch costs two launches (tedspad_softmax_ce_eval: softmax, cross entropy, its mean and the top-1 class;
tedspad_vote_accumulate: the per-video probability sums) and no host synchronisation; the reference's `pred_dict` of per-clip numpy rows
becomes a (V, C) sum and a count per video on the device, finalised once per pass (tedspad_vote_finalize). Ties between exactly equal
probabilities go to the highest class index (numpy's stable argsort, flipped); the reference's default sort kind leaves them unspecified.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .engine import _stream_ptr, require_cuda
from .train_step import DEFAULT_PARAMS, AnonymizerTrainStep


def _host_i64(labels):
    """labels as the loader delivers them (list / numpy / CPU tensor) -> contiguous int64 numpy; None for a device tensor."""
    if isinstance(labels, torch.Tensor):
        if labels.is_cuda:
            return None
        labels = labels.numpy()
    return np.ascontiguousarray(np.asarray(labels).reshape(-1), dtype=np.int64)


def softmax_ce_eval(logits, labels):
    """logits (B, C) fp32 cuda; labels (B): host values (range-checked before the launch) or an int64 cuda tensor (not checkable without
    a synchronisation: an out-of-range label gives a NaN loss). -> probs (B, C), row_loss (B), loss (1), pred (B) int32."""
    require_cuda(logits, "softmax_ce_eval")
    if logits.dim() != 2:
        raise ValueError("softmax_ce_eval: logits must be (B, C), got %s" % (tuple(logits.shape),))
    lg = logits.contiguous().float()
    b, c = lg.shape
    host = _host_i64(labels)
    lab = labels.contiguous().long() if host is None else torch.from_numpy(host).to(lg.device, non_blocking=True)
    if lab.numel() != b:
        raise ValueError("softmax_ce_eval: %d labels for %d rows" % (lab.numel(), b))
    probs = torch.empty_like(lg)
    row_loss = torch.empty(b, dtype=torch.float32, device=lg.device)
    loss = torch.empty(1, dtype=torch.float32, device=lg.device)
    pred = torch.empty(b, dtype=torch.int32, device=lg.device)
    softmax_ce_eval_into(lg, lab, host, probs, row_loss, loss, pred)
    return probs, row_loss, loss, pred


def softmax_ce_eval_into(lg, lab, host, probs, row_loss, loss, pred, B=None, Cn=None):
    """The raw call on caller-owned buffers (B / Cn override the logits' shape: the argument checks are the library's)."""
    b, c = (lg.shape[0] if B is None else B), (lg.shape[1] if Cn is None else Cn)
    _lib.check(_lib.lib().tedspad_softmax_ce_eval(lg.data_ptr(), lab.data_ptr(), None if host is None else host.ctypes.data, probs.data_ptr(),
                                                  row_loss.data_ptr(), loss.data_ptr(), pred.data_ptr(), b, c, _stream_ptr()), "tedspad_softmax_ce_eval")


def vote_accumulate(probs, vid, sums, counts):
    """sums[vid[b]] += probs[b], counts[vid[b]] += 1 in row order. vid: host int32 values (list / numpy); checked against sums' rows first."""
    require_cuda(probs, "vote_accumulate")
    host = np.ascontiguousarray(np.asarray(vid).reshape(-1), dtype=np.int32)
    b, c = probs.shape
    if host.size != b or sums.shape[1] != c or counts.numel() != sums.shape[0] or not probs.is_contiguous():
        raise ValueError("vote_accumulate: probs %s, %d indices, sums %s, counts %s" % (tuple(probs.shape), host.size, tuple(sums.shape), tuple(counts.shape)))
    dev = torch.from_numpy(host).to(probs.device, non_blocking=True)
    _lib.check(_lib.lib().tedspad_vote_accumulate(probs.data_ptr(), dev.data_ptr(), host.ctypes.data, sums.data_ptr(), counts.data_ptr(), b, c,
                                                  sums.shape[0], _stream_ptr()), "tedspad_vote_accumulate")


def vote_finalize(sums, counts, labels_v):
    """-> mean (V, C) fp32, pred_v (V) int32 (-1: never seen), correct (V) uint8."""
    require_cuda(sums, "vote_finalize")
    v, c = sums.shape
    if counts.numel() != v or labels_v.numel() != v or labels_v.dtype != torch.int64:
        raise ValueError("vote_finalize: sums %s, counts %s, labels %s %s" % (tuple(sums.shape), tuple(counts.shape), tuple(labels_v.shape), labels_v.dtype))
    mean = torch.empty_like(sums)
    pred = torch.empty(v, dtype=torch.int32, device=sums.device)
    correct = torch.empty(v, dtype=torch.uint8, device=sums.device)
    _lib.check(_lib.lib().tedspad_vote_finalize(sums.data_ptr(), counts.data_ptr(), labels_v.data_ptr(), mean.data_ptr(), pred.data_ptr(),
                                                correct.data_ptr(), v, c, _stream_ptr()), "tedspad_vote_finalize")
    return mean, pred, correct


class ActionValidator:
    def __init__(self, ft_model, fa_model=None, params=DEFAULT_PARAMS, temporal_loss: bool = False):
        """ft_model: the action classifier (returns (logits, feature)); fa_model: the anonymizer in front, or None for the raw
        train_action.py path. temporal_loss=False is `val_epoch_video` (its triplet lines are commented out: train_anonymizer.py:261-268);
        True adds params.temporal_loss_weight x triplet(feat1, feat2, feat3) as train_anonymized_action.py:158-165 does."""
        self.ft, self.fa, self.params, self.temporal_loss = ft_model, fa_model, params, bool(temporal_loss)
        self.reset()

    def reset(self):
        """Forget everything accumulated: a new `pred_dict, label_dict = {}, {}` (train_anonymizer.py:459)."""
        self._index, self._names, self._labels = {}, [], []          # video key -> row; keys in first-seen order; first label seen per key
        self._sums = self._counts = None                              # (cap, C) fp32, (cap) int32 on the device; cap doubles
        self._rows = []                                               # (probs, [row per clip]) per batch, for pred_dict
        self._pass_loss, self._pass_pred, self._pass_lab = [], [], []
        self.val_losses = []                                          # one mean per closed pass (:473)

    # ---- the device buffers ---------------------------------------------------------------------------------------------------------
    def _reserve(self, need, c, device):
        if self._sums is None:
            cap = 64
            while cap < need:
                cap *= 2
            self._sums = torch.zeros(cap, c, dtype=torch.float32, device=device)
            self._counts = torch.zeros(cap, dtype=torch.int32, device=device)
            return
        if self._sums.shape[1] != c:
            raise ValueError("ActionValidator: %d classes after %d; reset() between models" % (c, self._sums.shape[1]))
        cap = self._sums.shape[0]
        if need <= cap:
            return
        while cap < need:
            cap *= 2
        sums, counts = torch.zeros(cap, c, dtype=torch.float32, device=device), torch.zeros(cap, dtype=torch.int32, device=device)
        sums[:self._sums.shape[0]].copy_(self._sums)
        counts[:self._counts.shape[0]].copy_(self._counts)
        self._sums, self._counts = sums, counts

    @property
    def counts(self):
        """Clips seen per video so far, in `names` order (device int32)."""
        return self._counts[:len(self._names)] if self._counts is not None else torch.zeros(0, dtype=torch.int32)

    # ---- one batch ------------------------------------------------------------------------------------------------------------------
    def evaluate(self, inputs_video, labels, vid_paths):
        """inputs_video: (B, T, 3, H, W) fp32 cuda as the loader delivers it (T = num_frames, or 3 x num_frames for the triplet loaders);
        labels: (B) class indices (list / numpy / tensor); vid_paths: B paths. Returns dict(logits, probs, loss, pred) of device tensors."""
        require_cuda(inputs_video, "ActionValidator.evaluate")
        vid_paths = list(vid_paths)
        if len(vid_paths) != inputs_video.shape[0]:
            raise ValueError("ActionValidator.evaluate: %d paths for a batch of %d" % (len(vid_paths), inputs_video.shape[0]))
        self.ft.eval()                                                # :220-221
        with torch.no_grad():
            if self.fa is not None:
                self.fa.eval()
                frames, shape = AnonymizerTrainStep._feed(inputs_video)   # :232,240-242 (Q2)
                clip = self.fa(frames).reshape(shape)                 # :243
            else:
                clip = inputs_video.permute(0, 2, 1, 3, 4)            # train_action.py:120
        return self._evaluate_clip(clip, labels, vid_paths)

    def evaluate_frames(self, videos, records, labels, vid_paths, reso):
        """The same batch from DECODED FRAMES: videos / records / reso as `val_clips.val_clips` takes them (records[b]: the 16 or 3 x 16 frame records
        of sample b, `val_clips.sample_val_*`). With an anonymizer ONE launch (val_clips.val_clips_act) writes the 16-bit activation of the pseudo-images
        its first conv reads (Q2) and `fa.forward_act` starts there: the fp32 batch and `_feed`'s permuted copy are never written, and the logits are those
        of `evaluate(val_clips.val_clips(videos, records, reso), ...)` bit for bit. Without one the fp32 batch is written and `evaluate` runs on it."""
        from . import val_clips
        if self.fa is None:
            return self.evaluate(val_clips.val_clips(videos, records, reso), labels, vid_paths)
        if not hasattr(self.fa, "forward_act"):
            raise TypeError("ActionValidator.evaluate_frames: fa_model %s has no forward_act (UnetPlusPlus and UNet start from the 16-bit activation)"
                            % type(self.fa).__name__)
        vid_paths = list(vid_paths)
        if len(vid_paths) != len(records):
            raise ValueError("ActionValidator.evaluate_frames: %d paths for a batch of %d" % (len(vid_paths), len(records)))
        self.ft.eval()
        self.fa.eval()
        with torch.no_grad():
            act = val_clips.val_clips_act(videos, records, reso, self.fa.ACT_CPAD, self.fa.compute_dtype)
            b, t = len(records), len(records[0])
            clip = self.fa.forward_act(act).reshape(b, 3, t, int(reso[0]), int(reso[1]))      # :243 (the Q2 reshape back)
        return self._evaluate_clip(clip, labels, vid_paths)

    def _evaluate_clip(self, clip, labels, vid_paths):
        """clip (B, 3, T, H, W) as ft sees it -> the heads, the losses and the votes (:246-294)."""
        p = self.params
        with torch.no_grad():
            t = clip.shape[2]
            if t == 3 * p.num_frames:
                clips = torch.split(clip, [p.num_frames] * 3, dim=2)  # :246
            elif t == p.num_frames and not self.temporal_loss:
                clips = (clip,)                                       # :250
            else:
                raise ValueError("ActionValidator.evaluate: %d frames per sample; expected %s%d" % (
                    t, "" if self.temporal_loss else "%d or " % p.num_frames, 3 * p.num_frames))
            logits, feat1 = self.ft(clips[0])                         # :251
            probs, _, loss, pred = softmax_ce_eval(logits, labels)    # :259,272
            loss = loss[0]
            if self.temporal_loss:                                    # train_anonymized_action.py:158-165
                feat2, feat3 = self.ft(clips[1])[1], self.ft(clips[2])[1]
                a, pp, n = (f.contiguous().float() for f in (feat1, feat2, feat3))
                trip = torch.empty(1, dtype=torch.float32, device=a.device)
                ws = torch.empty(a.shape[0], dtype=torch.float32, device=a.device)
                _lib.check(_lib.lib().tedspad_triplet_fwd_bwd(a.data_ptr(), pp.data_ptr(), n.data_ptr(), trip.data_ptr(), ws.data_ptr(), None, None, None,
                                                              a.shape[0], a.shape[1], C.c_float(float(p.triplet_loss_margin)), C.c_float(1e-6),
                                                              _stream_ptr()), "tedspad_triplet_fwd_bwd")
                loss = torch.add(loss, trip[0], alpha=float(p.temporal_loss_weight))
        # the video each clip votes for: path.split('/')[-1] (:286), rows in first-seen order, the first label seen is the video's (:292-294)
        host_lab = _host_i64(labels)
        if host_lab is None:
            host_lab = labels.cpu().numpy().astype(np.int64)          # (device labels: the one read-back the caller chose)
        vid = []
        for path, lab in zip(vid_paths, host_lab):
            key = str(str(path).split("/")[-1])
            row = self._index.get(key)
            if row is None:
                row = self._index[key] = len(self._names)
                self._names.append(key)
                self._labels.append(int(lab))
            vid.append(row)
        self._reserve(len(self._names), probs.shape[1], probs.device)
        vote_accumulate(probs, vid, self._sums, self._counts)
        self._rows.append((probs, vid))
        self._pass_loss.append(loss)
        self._pass_pred.append(pred)
        self._pass_lab.append(host_lab)
        return dict(logits=logits, probs=probs, loss=loss, pred=pred)

    # ---- per pass / per epoch -------------------------------------------------------------------------------------------------------
    def _finalize(self):
        v = len(self._names)
        if v == 0:
            raise RuntimeError("ActionValidator: no batch has been evaluated")
        labels_v = torch.tensor(self._labels, dtype=torch.int64).to(self._sums.device)
        mean, pred, correct = vote_finalize(self._sums[:v], self._counts[:v], labels_v)
        return mean, pred.cpu().numpy(), correct.cpu().numpy()

    def end_pass(self):
        """Closes one (mode, cropping_fac) pass. Returns dict(accuracy: clip-level top-1 of the pass (:296-297), loss: np.mean of its batch
        losses (:301), running_accuracy / correct_count / num_videos: per-video top-1 over everything seen so far (:475-488))."""
        if not self._pass_loss:
            raise RuntimeError("ActionValidator.end_pass: the pass has no batch")
        losses = torch.stack(self._pass_loss).cpu().numpy()           # the pass's one read-back (the reference: loss.item() per batch, :270)
        c_pred = torch.cat(self._pass_pred).cpu().numpy()
        truth = np.concatenate(self._pass_lab)
        accuracy = float(np.sum(c_pred == truth)) / len(c_pred)
        loss = float(np.mean([float(x) for x in losses]))
        self.val_losses.append(loss)
        self._pass_loss, self._pass_pred, self._pass_lab = [], [], []
        _, _, correct = self._finalize()
        n = int(correct.sum())
        return dict(accuracy=accuracy, loss=loss, running_accuracy=float(n) / len(correct), correct_count=n, num_videos=len(correct))

    def result(self):
        """The epoch's numbers (:490-509) over every closed pass."""
        if self._pass_loss:
            raise RuntimeError("ActionValidator.result: a pass is open; call end_pass() first")
        mean, pred, correct = self._finalize()
        n = int(correct.sum())
        pred_dict = {k: [] for k in self._names}
        for probs, vid in self._rows:
            rows = probs.cpu().numpy()
            for r, v in zip(rows, vid):
                pred_dict[self._names[v]].append(r)
        return dict(accuracy=float(n) / len(correct), correct_count=n, num_videos=len(correct), val_loss=float(np.mean(self.val_losses)),
                    names=list(self._names), mean_probs=mean, predictions=pred, labels=np.asarray(self._labels, dtype=np.int64),
                    pred_dict=pred_dict, label_dict=dict(zip(self._names, self._labels)))
