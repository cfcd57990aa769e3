"""-m gpu: MGFN inference on MI355X (csrc/mgfn.hip, ted_spad_amd.mgfn, ted_spad_amd.anomaly). Every entry point against fp64 torch on the
same inputs (rel-L2 <= 1e-5) over ragged batches; the model against the reference's recorded outputs (tests/golden/mgfn_golden.npz) within
10x the reference's own fp32-vs-fp64 error; batch independence bit for bit; test()'s AUCs exactly; the extraction -> feed -> score chain;
checkpoint loading."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN_DIR, rel_l2
from kernel_refs import mgfn_attention_torch, mgfn_conv_seq as _conv_seq, mgfn_relpos_torch, mgfn_seqs as _seqs
from ted_spad_amd import _lib
from ted_spad_amd.engine import _stream_ptr
from ted_spad_amd.synth import synth_mgfn_state_dict, synth_tensor

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 31, 32, 33, 257, 1500]
BOUND = 1e-5


def _meta():
    with open(os.path.join(GOLDEN_DIR, "mgfn_golden_meta.json")) as f:
        return json.load(f)


def _golden():
    return dict(np.load(os.path.join(GOLDEN_DIR, "mgfn_golden.npz")))


def _ragged(lengths):
    L = torch.tensor(lengths, dtype=torch.int64)
    off = torch.zeros(len(L) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(L, 0)
    st = off[:-1].repeat_interleave(L)
    bounds = torch.stack([st, st + L.repeat_interleave(L)], 1).to(torch.int32).cuda()
    return off.tolist(), bounds, off.to(torch.int32).cuda()


def _check(name, got, ref):
    e = rel_l2(got.detach().cpu().double().numpy(), ref.detach().cpu().numpy())
    print("%-28s rel-L2 %.2e" % (name, e))
    assert e <= BOUND, (name, e)


@pytest.mark.parametrize("mode", ["to_tokens_k3x2049", "scc_k3", "ln_gelu_res", "plain_res"])
def test_gemm_vs_fp64(mode):
    off, bounds, _ = _ragged(LENGTHS)
    M = off[-1]
    taps, cin, N, gelu, ln, res = {"to_tokens_k3x2049": (3, 2064, 64, 0, 0, 0), "scc_k3": (3, 128, 128, 0, 0, 1),
                                   "ln_gelu_res": (1, 1024, 4096, 1, 1, 1), "plain_res": (1, 4096, 1024, 0, 0, 1)}[mode]
    x = synth_tensor(1, "g_x" + mode, (M, cin), -2, 2)
    if mode.startswith("to_tokens"):
        x[:, 2049:] = 0                                            # F + 1 = 2049 channels padded to 2064, the pad is zero
    w = synth_tensor(1, "g_w" + mode, (N, taps, cin), -1, 1) / (taps * cin) ** 0.5
    if mode.startswith("to_tokens"):
        w[:, :, 2049:] = 0
    b = synth_tensor(1, "g_b" + mode, (N,), -0.1, 0.1)
    r = synth_tensor(1, "g_r" + mode, (M, N), -1, 1) if res else None
    xc, wc, bc = x.cuda(), w.cuda().contiguous(), b.cuda()
    rc = r.cuda() if res else None
    stats = None
    if ln:
        stats = torch.empty((M, 2), device="cuda")
        _lib.check(_lib.lib().tedspad_mgfn_ln_stats(xc.data_ptr(), cin, M, cin, 1e-5, 0, stats.data_ptr(), _stream_ptr()))
    y = torch.empty((M, N), device="cuda")
    _lib.check(_lib.lib().tedspad_mgfn_gemm(xc.data_ptr(), cin, bounds.data_ptr(), taps, cin, stats.data_ptr() if ln else None, wc.data_ptr(),
                                            bc.data_ptr(), gelu, rc.data_ptr() if res else None, N, y.data_ptr(), N, M, N, _stream_ptr()))
    xd, wd, bd = x.double(), w.double(), b.double()
    if ln:                                                          # MGFN LayerNorm without g / b (folded into w on the host): / (std + eps)
        mu = xd.mean(1, keepdim=True)
        xd = (xd - mu) / (((xd - mu) ** 2).mean(1, keepdim=True).sqrt() + 1e-5)
    ref = torch.cat([_conv_seq(s, wd, bd, taps) for s in _seqs(xd, off)])
    if gelu:
        ref = F.gelu(ref)
    if res:
        ref = ref + r.double()
    _check("gemm " + mode, y, ref)


@pytest.mark.parametrize("heads", [1, 2, 16])
def test_attention_vs_fp64(heads):
    lengths = LENGTHS
    off, _, off_d = _ragged(lengths)
    M, inner = off[-1], 64 * heads
    qkv = synth_tensor(2, "att%d" % heads, (M, 3 * inner), -2, 2)
    out = torch.empty((M, inner), device="cuda")
    qc = qkv.cuda()
    _lib.check(_lib.lib().tedspad_mgfn_attention(qc.data_ptr(), 3 * inner, off_d.data_ptr(), len(lengths), max(lengths), heads, out.data_ptr(),
                                                 inner, _stream_ptr()))
    _check("attention heads=%d" % heads, out, mgfn_attention_torch(qkv, off, heads, torch.float64))


@pytest.mark.parametrize("heads", [1, 16])
def test_relpos_vs_fp64(heads):
    off, bounds, _ = _ragged(LENGTHS)
    M, C = off[-1], 64 * heads
    v = synth_tensor(3, "rp_v%d" % heads, (M, C), -1, 1)
    w = synth_tensor(3, "rp_w%d" % heads, (heads, 5), -1, 1)
    b = synth_tensor(3, "rp_b%d" % heads, (heads,), -0.1, 0.1)
    out = torch.empty((M, C), device="cuda")
    vc, wc, bc = v.cuda(), w.cuda(), b.cuda()
    _lib.check(_lib.lib().tedspad_mgfn_relpos(vc.data_ptr(), C, bounds.data_ptr(), M, C, heads, wc.data_ptr(), bc.data_ptr(), out.data_ptr(), C,
                                              _stream_ptr()))
    ref = mgfn_relpos_torch(v, w, b, off, heads, torch.float64)
    _check("relpos heads=%d" % heads, out, ref)


def test_ln_stats_head_crop_mean_vs_fp64():
    lengths = LENGTHS
    nc = 10
    seq_len = [T for T in lengths for _ in range(nc)]
    M, C = sum(seq_len), 1024
    x = synth_tensor(4, "head_x", (M, C), -3, 5)
    lw, lb = synth_tensor(4, "head_lw", (C,), 0.5, 1.5), synth_tensor(4, "head_lb", (C,), -0.1, 0.1)
    fw = synth_tensor(4, "head_fw", (C,), -0.05, 0.05)
    xc = x.cuda()
    L, st = _lib.lib(), _stream_ptr()
    for torch_ln in (0, 1):
        s = torch.empty((M, 2), device="cuda")
        _lib.check(L.tedspad_mgfn_ln_stats(xc.data_ptr(), C, M, C, 1e-5, torch_ln, s.data_ptr(), st))
        xd = x.double()
        mu, var = xd.mean(1), xd.var(1, unbiased=False)
        rs = 1 / (var + 1e-5).sqrt() if torch_ln else 1 / (var.sqrt() + 1e-5)
        _check("ln_stats mean torch_ln=%d" % torch_ln, s[:, 0], mu)
        _check("ln_stats rs torch_ln=%d" % torch_ln, s[:, 1], rs)
    h, lg, sc, mg = torch.empty((M, C), device="cuda"), *(torch.empty(M, device="cuda") for _ in range(3))
    lwc, lbc, fwc = lw.cuda(), lb.cuda(), fw.cuda()                                       # kept alive across the launch
    _lib.check(L.tedspad_mgfn_head(xc.data_ptr(), C, M, C, lwc.data_ptr(), lbc.data_ptr(), fwc.data_ptr(), 0.05, 1e-5,
                                   h.data_ptr(), lg.data_ptr(), sc.data_ptr(), mg.data_ptr(), st))
    hd = F.layer_norm(x.double(), (C,), lw.double(), lb.double(), 1e-5)
    zd = hd @ fw.double() + 0.05
    _check("head h", h, hd)
    _check("head logits", lg, zd)
    _check("head scores", sc, torch.sigmoid(zd))
    _check("head mags", mg, hd.norm(dim=1))
    seg = torch.zeros(len(lengths) + 1, dtype=torch.int32)
    seg[1:] = torch.cumsum(torch.tensor(lengths), 0)
    nseg = int(seg[-1])
    a_out, b_out = torch.empty(nseg, device="cuda"), torch.empty(nseg, device="cuda")
    seg_c = seg.cuda()
    _lib.check(L.tedspad_mgfn_crop_mean(sc.data_ptr(), a_out.data_ptr(), mg.data_ptr(), b_out.data_ptr(), seg_c.data_ptr(), len(lengths),
                                        max(lengths), nc, st))
    ra, rb, o = [], [], 0
    for T in lengths:
        ra.append(sc[o:o + nc * T].double().view(nc, T).mean(0))
        rb.append(mg[o:o + nc * T].double().view(nc, T).mean(0))
        o += nc * T
    _check("crop_mean scores", a_out, torch.cat(ra))
    _check("crop_mean mags", b_out, torch.cat(rb))


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def _model(cfg, seed):
    from ted_spad_amd.mgfn import MGFN
    m = MGFN(feature_size=cfg["feature_size"], depths=tuple(cfg["depths"]), mgfn_types=tuple(cfg["types"])).eval()
    m.load_state_dict(synth_mgfn_state_dict(m.state_dict(), seed))
    return m.cuda()


def _video(meta, name, T, F):
    return synth_tensor(meta["seed"], name, (1, meta["ncrops"], T, F + 1), 0.0, 2.0).cuda()


@pytest.mark.parametrize("config", ["a", "b", "c"])
def test_model_vs_golden(config):
    meta, gold = _meta(), _golden()
    E = meta["errors"]
    cfg = meta["configs"][config]
    m = _model(cfg, meta["seed"])
    for case, cm in meta["cases"].items():
        if cm["config"] != config:
            continue
        T = cm["T"]
        video = _video(meta, cm["video"], T, cm["F"])
        r = m.infer([video[0].permute(1, 0, 2)], keep_h=True)
        g = lambda k: gold["%s/%s" % (case, k)]  # noqa: E731
        e_s = float((r["crop_scores"].cpu().double() - torch.from_numpy(g("crop_scores"))).abs().max())
        e_l = float((r["logits"].cpu().double().view(10, T) - torch.from_numpy(g("logits"))).abs().max())
        e_m = rel_l2(r["mags"].cpu().view(10, T).numpy(), g("mags"))
        print("%s scores %.2e (bound %.2e)  logits %.2e (bound %.2e)  mags %.2e (bound %.2e)" % (
            case, e_s, 10 * E["scores_max_abs"], e_l, 10 * E["logits_max_abs"], e_m, 10 * E["mags_rel_l2"]))
        assert e_s <= 10 * E["scores_max_abs"] and e_l <= 10 * E["logits_max_abs"] and e_m <= 10 * E["mags_rel_l2"], case
        sa, sn, fa, fn, scores = m(video)
        assert (sa is sn) and (fa is fn) and tuple(scores.shape) == (1, T, 1) and tuple(fa.shape) == (10, 3, 1024)
        # forward's own top-3 choice: its features are the to_logits rows of exactly the fixture's indices, in its order (forward and
        # infer are bit-identical, test_batch_independence_config_a), and its score is the mean of those segments' scores
        gi = torch.from_numpy(g("idx")).cuda()
        assert torch.equal(fa, r["h"].view(10, T, -1)[:, gi]), (case, g("idx"))
        assert torch.equal(sa, torch.mean(torch.gather(scores, 1, gi.view(1, 3, 1)), dim=1))
        e_sa = abs(float(sa[0, 0]) - float(g("score_abnormal")))
        e_f = rel_l2(fa.cpu().numpy(), g("feat"))
        print("%s score_abnormal %.2e  features rel-L2 %.2e (bound %.2e)" % (case, e_sa, e_f, 10 * E["h_rel_l2"]))
        assert e_sa <= 10 * E["scores_max_abs"] and e_f <= 10 * E["h_rel_l2"]
        if T == 3:
            e_h = rel_l2(r["h"].cpu().view(10, 3, -1).numpy(), g("h"))
            print("%s h rel-L2 %.2e" % (case, e_h))
            assert e_h <= 10 * E["h_rel_l2"]


def test_batch_independence_config_a():
    meta = _meta()
    cfg = meta["configs"]["a"]
    m = _model(cfg, meta["seed"])
    vids = [_video(meta, cm["video"], cm["T"], cm["F"]) for cm in meta["cases"].values() if cm["config"] == "a"]
    feats = [v[0].permute(1, 0, 2) for v in vids]
    batch = m.score(feats)
    for v, f, s in zip(vids, feats, batch):
        alone = m.score([f])[0]
        fwd = m(v)[4].view(-1)
        assert torch.equal(alone, s) and torch.equal(fwd, s)
    # and in another order, with other videos around
    again = m.score(feats[::-1] + feats[:1])
    for s, t in zip(batch[::-1], again):
        assert torch.equal(s, t)


def test_evaluate_matches_test_py_aucs():
    from ted_spad_amd.anomaly import evaluate
    meta, gold = _meta(), _golden()
    cfg = meta["configs"]["a"]
    m = _model(cfg, meta["seed"])
    feats = [_video(meta, n, T, cfg["feature_size"])[0].permute(1, 0, 2) for n, T in zip(meta["eval"]["videos"], meta["eval"]["Ts"])]
    rec_auc, pr_auc = evaluate(m, feats, gold["eval/gt"])
    print("rec_auc %r pr_auc %r (reference %r %r)" % (rec_auc, pr_auc, meta["eval"]["rec_auc"], meta["eval"]["pr_auc"]))
    assert rec_auc == meta["eval"]["rec_auc"] and pr_auc == meta["eval"]["pr_auc"]


def test_extraction_feed_score_chain(tmp_path):
    from ted_spad_amd import extraction, mgfn_feed
    from ted_spad_amd.model_loaders import load_ft_model
    from ted_spad_amd.synth import synth_clips, synth_state_dict
    from ted_spad_amd.mgfn import MGFN
    ft = load_ft_model("largei3d", num_classes=102)
    ft.load_state_dict(synth_state_dict(ft.state_dict(), 0), strict=True)
    ft = ft.cuda().eval()
    T, nc = 4, 10
    clips = synth_clips(5, T * nc, (3, 16, 112, 112)).cuda()
    feats = extraction.extract_clip_features(ft, clips).view(T, nc, -1)                 # stays on the device
    m = MGFN().eval()
    m.load_state_dict(synth_mgfn_state_dict(m.state_dict(), 0))
    m = m.cuda()
    s_dev = m.score([mgfn_feed.getitem(feats, test_mode=True)])[0]
    path = extraction.save_features_batched(str(tmp_path), [("vid0.mp4", feats)])[0]
    host = np.array(np.load(path), dtype=np.float32)                                      # dataset.py:54-55
    s_npy = m.score([mgfn_feed.getitem(torch.from_numpy(host).cuda(), test_mode=True)])[0]
    assert s_dev.shape == (T,) and torch.equal(s_dev, s_npy)


def test_checkpoints_and_modes():
    from ted_spad_amd.mgfn import MGFN
    meta = _meta()
    m = MGFN().eval()
    sd = synth_mgfn_state_dict(m.state_dict(), 0)
    m.load_state_dict({k.replace("module.", ""): v for k, v in {"module." + k: v for k, v in sd.items()}.items()})   # test.py:64
    m = m.cuda()
    cm = meta["cases"]["a_T7"]
    f = _video(meta, cm["video"], cm["T"], cm["F"])[0].permute(1, 0, 2)
    s0 = m.score([f])[0].clone()
    bad = dict(sd)
    bad.pop("fc.bias")
    with pytest.raises(RuntimeError):
        MGFN().load_state_dict(bad)
    extra = dict(sd)
    extra["fc.extra"] = torch.zeros(1)
    with pytest.raises(RuntimeError):
        MGFN().load_state_dict(extra)
    with torch.no_grad():
        m.fc.bias.add_(0.5)                                                               # in place: the packed weights are rebuilt
    s1 = m.score([f])[0]
    assert (s1 > s0).all()
    with torch.no_grad():
        m.fc.bias.sub_(0.5)
    m.train()
    with pytest.raises(NotImplementedError):
        m(f.permute(1, 0, 2).unsqueeze(0))
    with pytest.raises(NotImplementedError):
        m.score([f])
