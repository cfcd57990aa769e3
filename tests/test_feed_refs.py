"""CPU: the references and case tables of tests/feed_refs.py on their own, before anything from the GPU is compared with them (tests/test_hip_feed_exact.py):
the conditions under which the exact comparison is exact, the cap on the bounded comparison's slack, the coverage of the case table, and that the table is
telling -- every `wrong=` variant of the reference fails, on at least one case, the very comparison the GPU test makes (feed_refs.verdict).

Measured on the table (per exact case, f16 / bf16): really rounded 17 .. 99 % / 78 .. 100 %; exact ties 17 .. 22 % / 5 .. 16 % on the x2 and x4 rows. The 2:1 and
4:1 interiors hold few bf16 ties (2.3 % and 0.1 %) and fl32(b / 255) none at all, so the ties floor is asserted on the up-sampling rows, the rounding floor on every
exact row. The two ends of a bounded element differ in at most 0.6 % of a case's elements (cap: 2 %)."""
import numpy as np
import pytest
import torch

import feed_refs as R
import kernel_refs as K

D = torch.float64
EXACT = [c for c in R.CASES if c.kind in ("exact", "ring")]
BOUNDED = [c for c in R.CASES if c.kind in ("ring", "bounded")]


def _ids(cases):
    return [c.name for c in cases]


def test_aa_weights_follow_torch():
    """The fp32 restatement of torch's rule against the dense matrix read off torch's own antialiased interpolate (2e-6: torch normalises in another order), and
    the dyadic / non-dyadic size pairs the exact rows rely on."""
    from oracle import preprocess_ref
    for n_in, n_out in [(864, 224), (100, 224), (53, 24), (70, 18), (5, 3), (3, 5), (130, 260), (64, 32)]:
        w = R.aa_weights(n_in, n_out)
        ref = preprocess_ref.resize_matrix(n_in, n_out).to(D)
        assert float((w - ref).abs().max()) < 2e-6, (n_in, n_out)
        assert int((w != 0).sum(1).max()) <= R.aa_taps(n_in, n_out)
    for n_in, n_out in [(8, 8), (8, 16), (13, 26), (12, 48)]:
        assert R.dyadic_bits(R.aa_weights(n_in, n_out)) is not None, (n_in, n_out)
    for n_in, n_out in [(16, 8), (32, 8)]:
        w = R.aa_weights(n_in, n_out)
        assert R.dyadic_bits(w[1:-1]) is not None and R.dyadic_bits(w[:1]) is None and R.dyadic_bits(w[-1:]) is None, (n_in, n_out)
    assert R.dyadic_bits(R.aa_weights(9, 27)) is None
    assert torch.equal(R.aa_weights(8, 8), torch.eye(8, dtype=D))


def test_frame_rule():
    assert R.frame_of(0, 0, -3, 8, 1, 16, 20) is None and R.frame_of(0, 3, -3, 8, 1, 16, 20) == 0            # zero frames in front of the video
    assert R.frame_of(1, 15, -3, 8, 1, 16, 20) is None and R.frame_of(1, 14, -3, 8, 1, 16, 20) == 19          # and past its end
    assert R.frame_of(0, 6, 0, 9, 3, 6, 40) is None and R.frame_of(0, -1, 0, 9, 3, 6, 40) is None             # outside the clip
    assert R.frame_of(0, 6, 0, 9, 3, 6, 40, wrong="t_clip_16") == 18 and R.frame_of(0, 0, -3, 8, 1, 16, 20, wrong="no_zero_front") == 17
    assert [R.frame_pairs(t) for t in (16, 8, 6)] == [4, 2, 1]


def test_layouts_against_independent_restatements():
    """records64 against the padded-clip slicing of test_clip_to_frame_pair_layout, act64 against a permute, ten_crop_boxes64 against known boxes."""
    x = torch.arange(11 * 2 * 3 * 4, dtype=D).reshape(11, 2, 3, 4) + 1.0
    samp = (2, -1, 5, 2, 8)
    got = R.records64(x, samp)
    clips = torch.zeros(2, 3, 2 + 8 + 6, 3, 4, dtype=D)                     # (n, c, pad + t_clip + pad, h, w)
    for n in range(2):
        for f in range(8):
            s = -1 + 5 * n + 2 * f
            if 0 <= s < 11:
                clips[n, :2, 2 + f] = x[s]
    ref = torch.stack([clips[:, :, 4 * tp:4 * tp + 8] for tp in range(2)], dim=1)                # (n, tp, c, dt, h, w)
    ref = ref.permute(0, 1, 4, 5, 3, 2).reshape(2, 2, 3, 2, 2, 24).permute(0, 1, 2, 4, 3, 5)
    assert torch.equal(got, ref) and bool((got[0, 0, ..., :9] == 0).all()) and bool((got != 0).any())
    for cpad in (4, 8):
        act = R.act64(x, samp, cpad).reshape(16, 3, 4, cpad)
        assert torch.equal(act[8 + 1, ..., :2], x[-1 + 5 + 2].permute(1, 2, 0)) and not bool(act[..., 2:].any()) and not bool(act[0].any())
    b = R.ten_crop_boxes64(97, 131, 77, 104)
    assert b[4] == (10, 14, False) and b[9] == (10, 13, True) and b[1] == (0, 27, False) and b[5] == (0, 27, True) and b[6] == (0, 0, True)
    assert R.ten_crop_boxes64(97, 131, 77, 104, wrong="centre_half_up")[4] == (10, 14, False)               # 13.5 -> 14 either way
    assert R.ten_crop_boxes64(17, 21, 12, 12)[4] == (2, 4, False) and R.ten_crop_boxes64(17, 21, 12, 12, wrong="centre_half_up")[4] == (3, 5, False)


def test_pil_resample_is_the_oracles_chain():
    from oracle import preprocess_ref
    fr = np.random.default_rng(3).integers(0, 256, (1, 97, 131, 3), dtype=np.uint8)
    side = int(97 * 0.8)
    box = (int(round((97 - side) / 2.0)), int(round((131 - side) / 2.0)), side, side)
    assert torch.equal(R.pil_resample(fr, box, (32, 40))[0].to(torch.float32), preprocess_ref.shanghai_augmentation(fr[0], reso_h=32, reso_w=40))


def test_the_table_covers_every_property_and_needs_every_case():
    for c in R.CASES:
        assert c.needs, c.name
        for p in c.needs:
            assert R.PROPERTIES[p](c), (c.name, p)
        T, H, W, C = c.thwc
        assert T <= 40 and H <= 64 and W <= 140 and c.out[0] <= 48 and c.out[1] <= 264, c.name
        assert c.box[0] + c.box[2] <= H and c.box[1] + c.box[3] <= W and c.out[1] % 2 == 0
    missing = set(R.PROPERTIES) - {p for c in R.CASES for p in c.needs}
    assert not missing, "not covered by any case: %s" % sorted(missing)
    assert len({c.name for c in R.CASES}) == len(R.CASES)
    for c in R.PIL_CASES:
        assert c.samp[1] >= 0 and c.box[0] + c.box[2] <= c.thwc[1] and c.box[1] + c.box[3] <= c.thwc[2]
    assert any(c.out[1] >= 260 for c in R.PIL_CASES) and {c.thwc[3] for c in R.PIL_CASES} == {1, 3}
    assert any(c.box[2] != c.box[3] for c in R.PIL_CASES)


@pytest.mark.parametrize("c", EXACT, ids=_ids(EXACT))
def test_exact_rows_are_exact_and_round(c):
    """Every weight used is dyadic, every value on the grid fp32 holds in any order, and the 16-bit rounding really happens: >= 10 % of the exact elements are
    rounded per storage type, and on the up-sampling rows >= 5 % are exact ties."""
    oh, ow = c.out
    wy, wx = R.aa_weights(c.box[2], oh), R.aa_weights(c.box[3], ow)
    ref, lo, hi = R.ends(c, "fp32")
    if c.kind == "ring":
        wy, wx = wy[1:-1], wx[1:-1]
        assert bool((lo != hi)[..., 0, :].any()) and bool((lo != hi)[..., :, -1].any())                   # the ring is bounded, not dropped
    gy, gx = R.dyadic_bits(wy), R.dyadic_bits(wx)
    assert gy is not None and gx is not None, (gy, gx)
    exact = (lo == hi)
    vals = ref[exact]
    if c.divisor == 256.0:
        assert 8 + gy + gx <= 24
        assert K.exact_in_fp32(vals * 2.0 ** (8 + gy + gx))                 # multiples of 2^-(8+gy+gx) below 1
    else:
        assert gy == 0 and gx == 0                                          # weights {1, 0}: the value is fl32(b / 255) itself
        want = (c.frames()[:, c.box[0]:c.box[0] + c.box[2], c.box[1]:c.box[1] + c.box[3]].astype(np.float32) / np.float32(255)).astype(np.float64)
        assert torch.equal(ref, torch.from_numpy(want).permute(0, 3, 1, 2))
    assert torch.equal(vals.to(torch.float32).to(D), vals)
    for dt in ("f16", "bf16"):
        rounded = float((K.round_once(vals, dt) != vals).double().mean())
        ties = float(R.is_tie(vals, dt).double().mean())
        print("%s %s: rounded %.3f, ties %.3f of %d exact elements (gy %d, gx %d)" % (c.name, dt, rounded, ties, vals.numel(), gy, gx))
        assert rounded >= 0.10, (dt, rounded)
        if c.out[0] > c.box[2]:
            assert ties >= 0.05, (dt, ties)


@pytest.mark.parametrize("c", BOUNDED, ids=_ids(BOUNDED))
def test_bounded_rows_leave_little_slack(c):
    """The two ends of the containment test differ in at most 2 % of the case's elements, per storage type; k is the taps' count + 4."""
    ref, lo, hi = R.ends(c, "fp32")
    assert R.bound_k(c.box, c.out) == R.aa_taps(c.box[2], c.out[0]) + R.aa_taps(c.box[3], c.out[1]) + 4
    assert 10 <= R.bound_k(c.box, c.out) <= 22 and bool((lo <= ref).all()) and bool((ref <= hi).all()) and float(ref.min()) >= 0.0
    for dt in ("f16", "bf16"):
        share = float((R.round16(lo, dt) != R.round16(hi, dt)).double().mean())
        print("%s %s: ends differ in %.4f" % (c.name, dt, share))
        assert share <= 0.02, (dt, share)


def _runs(c):
    return [(e, dt) for e in c.entries for dt in ((None,) if e == "fp32" else ("f16", "bf16"))]


@pytest.mark.parametrize("c", R.CASES, ids=_ids(R.CASES))
def test_the_reference_passes_its_own_comparison(c):
    for e, dt in _runs(c):
        assert R.verdict(c, e, dt, R.produce(c, e, dt)) == ""


# where each mistake must show: the comparison kind and the entries that can see it
_SEES = {"trunc16": ("rec", "ten", "act4", "act8"), "drop_last_tap": R.ENTRIES, "flip_shift": ("fp32", "rec", "act4", "act8"), "box_x0_zero": ("fp32", "rec", "act4", "act8"),
         "no_zero_front": ("rec", "ten"), "t_clip_16": ("rec", "ten", "act4", "act8"), "chan_swap": R.ENTRIES, "centre_half_up": ("ten",)}


@pytest.mark.parametrize("wrong", R.WRONG)
def test_every_wrong_variant_fails_the_gpu_tests_comparison(wrong):
    """On an exact case (inequality) and, where the mistake is in the arithmetic, on a bounded one (the bound, the containment) as well; for every entry that can
    see the mistake and for both storage types."""
    caught = {}
    for c in R.CASES:
        for e, dt in _runs(c):
            if e in _SEES[wrong] and R.verdict(c, e, dt, R.produce(c, e, dt, wrong)):
                caught.setdefault((e, dt), []).append(c.name)
    print(wrong, {k: len(v) for k, v in caught.items()})
    for e in _SEES[wrong]:
        for dt in ((None,) if e == "fp32" else ("f16", "bf16")):
            names = caught.get((e, dt), [])
            assert names, (wrong, e, dt)
            assert any(R.case(n).kind == "exact" for n in names), (wrong, e, dt)
            if wrong in ("trunc16", "drop_last_tap", "chan_swap", "box_x0_zero"):
                assert any(R.case(n).kind == "bounded" for n in names), (wrong, e, dt)
