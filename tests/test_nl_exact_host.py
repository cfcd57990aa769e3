"""CPU: the winners / decoys construction of tests/nl_exact.py is what tests/test_hip_nl_exact.py takes it for -- at every shape of the sweep the closed form
IS the float64 reference, nothing rounds on the way into or through the kernels, and no case is degenerate (every key carries a gradient, every decoy
placement occurs). Without these the GPU sweep could pass on inputs that exercise nothing."""
import pytest
import torch

import nl_exact as X
import nl_grad_ref

CASES = [(q, k, d) for d in X.WIDTHS for (q, k) in X.SHAPES]


def test_the_shape_lists():
    assert len(set(X.SHAPES)) == 24 and set(X.HOST_TAPE_SHAPES) <= set(X.SHAPES) and set(X.STRIDE_SHAPES) <= set(X.SHAPES) and len(X.HOST_TAPE_SHAPES) == 6
    ks, qs = {k for _, k in X.SHAPES}, {q for q, _ in X.SHAPES}
    for mult in (16, 32, 48, 64, 96, 128):                       # k on a multiple of the 16-key step and one beside it
        assert mult in ks and (mult - 1 in ks or mult + 1 in ks), mult
    assert {191, 193, 256} <= ks
    assert {31, 33, 63, 65, 95, 97, 129} <= qs                   # q one off a multiple of 32


def test_hadamard_rows_are_orthogonal():
    for d in X.WIDTHS:
        h = X.hadamard_of(d)
        assert torch.equal(h @ h.t(), d * torch.eye(d, dtype=torch.float64)) and bool((h.abs() == 1).all())
        c, _ = X.case(129, 256, d)
        gram = torch.einsum("nkd,njd->nkj", c["phi"], c["phi"])
        assert torch.equal(gram, (d * torch.eye(256, dtype=torch.float64)).expand(X.N_ITEMS, -1, -1))
        assert not torch.equal(c["phi"][0], c["phi"][1])


@pytest.mark.parametrize("q,k,d", CASES)
def test_closed_form_is_the_float64_reference(q, k, d):
    c, e = X.case(q, k, d)
    ref = nl_grad_ref.attention_grads(c["theta"], c["phi"], c["g"], c["dt"], c["scale"])
    for key in ("t", "lse", "p", "dtheta", "dphi", "dg"):
        tol = 1e-12 * max(1.0, float(ref[key].abs().max()))
        assert float((e[key] - ref[key]).abs().max()) <= tol, key
    assert float(ref["p"][~c["win"]].max() if bool((~c["win"]).any()) else 0.0) < 1e-50         # the largest probability off the winners
    logits = torch.einsum("nqd,nkd->nqk", c["theta"], c["phi"]) * c["scale"]
    assert torch.equal(logits, 256.0 * c["win"].double() + 128.0 * c["dec"].double())
    assert torch.equal(c["win"].sum(dim=2), c["m"]) and not bool((c["win"] & c["dec"]).any())
    assert not torch.equal(c["win"][0], c["win"][1]) or k == 1                                    # the items have different sets


@pytest.mark.parametrize("q,k,d", CASES)
def test_nothing_rounds(q, k, d):
    c, e = X.case(q, k, d)
    for dtype, tdt in X.STORAGE.items():
        for key, v in (("theta", c["theta"]), ("phi", c["phi"]), ("g", c["g"]), ("dt", c["dt"]), ("p", e["p"]), ("ds", e["ds"]), ("t", e["t"])):
            assert torch.equal(v.float().to(tdt).double(), v), (key, dtype)
    assert torch.equal(e["t"], e["t"].round()) and torch.equal(e["dp"], e["dp"].round()) and float(e["dp"].abs().max()) <= 64
    # every sum a kernel forms, in units of its grid, with every term taken at its absolute value: below 2^24 no order of summation rounds in fp32
    a = lambda t: t.abs()
    grids = {
        "theta . phi (unit 8)": a(c["theta"]).sum(dim=2) / 8.0,
        "P g, over all keys at p = 1 as a tile without a winner accumulates them (unit 32)": a(c["g"]).sum(dim=1) / 32.0,
        "sum of p (unit 1)": torch.tensor(float(k)),
        "dT . g (unit 32)": torch.einsum("nqd,nkd->nqk", a(c["dt"]), a(c["g"])) / 32.0,
        "dT . T (unit 1)": (a(c["dt"]) * a(e["t"])).sum(dim=2),
        "P^T dT (unit 1/32)": torch.einsum("nqk,nqd->nkd", e["p"], a(c["dt"])) * 32.0,
        "dS phi (unit 1/32)": torch.einsum("nqk,nkd->nqd", a(e["ds"]), a(c["phi"])) * 32.0,
        "dS^T theta (unit 1/4)": torch.einsum("nqk,nqd->nkd", a(e["ds"]), a(c["theta"])) * 4.0,
    }
    for what, v in grids.items():
        assert float(v.max()) < 2.0 ** 24, what
    for what, v, unit in (("dS", e["ds"], 1 / 32.0), ("dphi / scale", e["dphi"] / c["scale"], 0.25), ("dtheta / scale", e["dtheta"] / c["scale"], 1 / 32.0),
                          ("dg", e["dg"], 1 / 32.0)):
        assert torch.equal((v / unit).round() * unit, v), what
    for key in ("t", "dtheta", "dphi", "dg", "ds", "lse"):
        assert float(e[key].abs().max()) < 65504.0, key
        assert torch.equal(e[key].float().double(), e[key]) or key == "lse"


@pytest.mark.parametrize("q,k,d", CASES)
def test_no_case_is_degenerate(q, k, d):
    c, e = X.case(q, k, d)
    one = c["m"] == 1
    assert float(e["dtheta"][one].abs().max()) == 0.0                      # one winner: dP - D vanishes, by design
    if k > 1:
        rows = e["dtheta"][~one].abs().amax(dim=1) > 0                      # a row with several winners is zero only where their g agree in dT's channel
        assert bool(rows.float().mean() > 0.75) if rows.numel() >= 16 else bool(rows.any())
        assert float(e["dphi"].abs().max()) > 0.0
    assert bool((e["t"].abs().amax(dim=2) > 0).all()) and bool(c["win"][:, :, k - 1].any())
    if q >= k:
        assert bool(c["win"].any(dim=1).all()), "a key in no winner set"
        assert bool((e["dg"].abs().amax(dim=2) > 0).all())
        if k > 1:                                                         # with one key dphi is zero analytically
            assert bool((e["dphi"].abs().amax(dim=2) > 0).all())


def test_every_decoy_placement_occurs():
    seen = {}
    for d in X.WIDTHS:
        for q, k in X.SHAPES:
            c, _ = X.case(q, k, d)
            for key, v in X.placements(c).items():
                seen.setdefault(key, []).extend([(q, k)] * int(v.sum()))
            if k > 64 and d == 256:                                       # and, per shape with more than one key tile, a query with a tile that holds none of its keys
                tiles = [(c["win"] | c["dec"])[:, :, t0:t0 + 64].any(dim=2) for t0 in range(0, k, 64)]
                assert any(bool((~t).any()) for t in tiles), (q, k)
    for key in ("earlier", "later", "other_wave"):
        print("%s: %d queries at %d shapes" % (key, len(seen[key]), len(set(seen[key]))))
        assert len(set(seen[key])) >= 3, key
    wraps = sum(int((c["win"][:, :, 0] & c["win"][:, :, k - 1] & (c["m"] < k)).sum()) for (q, k) in X.SHAPES for c in [X.case(q, k, 256)[0]])
    assert wraps > 50                                                      # windows that run past k - 1 onto key 0
