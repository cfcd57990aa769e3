"""-m gpu: the entry points that split a batch into chunks of whole samples under the kernels' 32-bit offsets (engine.sample_chunks), on the chunk loops
that only a tensor past 2^31 elements reaches otherwise: PackedConv.call_pool_t2 / call_dual / gather, nl_attention (with and without lse) and
nl_attention_bwd. (PackedConv.__call__, dgrad and wgrad: tests/test_hip_train_ops.py::test_batch_chunking_matches_single_launch.)

Each case runs once under the real limit and once with engine.MAX_ELEMS lowered to two samples + 1, so that its three samples go as 2 + 1, and demands
torch.equal on every output: the kernels treat samples independently, and csrc/nonlocal.hip sums in a fixed order without atomics. The tuner is off. No
tile is pinned: call_pool_t2 and call_dual have one kernel each, and the built-in choice for gathered sources depends on the frame width and the kernel
size only (csrc/conv_igemm.hip), not on the batch. Inputs from ted_spad_amd.synth, rounded to f16."""
import pytest
import torch

from ted_spad_amd.synth import synth_tensor

pytestmark = pytest.mark.gpu
H = torch.float16
N = 3


def act(name, dims, c, lo=-1.0, hi=1.0):
    """A seeded f16 channels-last Act (N, *dims, c) on the GPU."""
    from ted_spad_amd import engine as E
    return E.Act(synth_tensor(17, name, (N,) + tuple(dims) + (c,), lo, hi).to(H).cuda(), c)


def conv(name, cout, cin, k):
    from ted_spad_amd import engine as E
    w = synth_tensor(17, name + "w", (cout, cin) + k, -1, 1) * (1.0 / (cin * k[0] * k[1] * k[2])) ** 0.5
    return E.PackedConv(w, synth_tensor(17, name + "s", (cout,), 0.5, 1.5), synth_tensor(17, name + "b", (cout,), -0.5, 0.5), dtype="f16", device="cuda")


@pytest.fixture
def both(monkeypatch):
    """both(run, per_sample) -> (outputs under the real limit, outputs with MAX_ELEMS = 2 * per_sample + 1); `run` returns a tuple of tensors. Checks on
    the way that the entry point itself went through one launch the first time and through samples 0-1, then 2, the second time."""
    from ted_spad_amd import engine as E
    monkeypatch.setattr(E, "AUTOTUNE", False)
    seen, real = [], E.sample_chunks
    monkeypatch.setattr(E, "sample_chunks", lambda *a: seen.append(list(real(*a))) or seen[-1])

    def go(run, per_sample):
        one = [t.clone() for t in run()]
        assert seen and all(s == [(0, N)] for s in seen), seen
        del seen[:]
        monkeypatch.setattr(E, "MAX_ELEMS", 2 * per_sample + 1)
        many = run()
        torch.cuda.synchronize()
        assert seen and all(s == [(0, 2), (2, N)] for s in seen), seen
        assert all(bool(torch.isfinite(t.float()).all()) for t in one)
        return one, many
    return go


def same(one, many):
    assert len(one) == len(many)
    for i, (a, b) in enumerate(zip(one, many)):
        assert a.shape == b.shape and torch.equal(a, b), "output %d differs between one launch and 2 + 1 samples" % i


def test_call_pool_t2(both):
    pc = conv("pt2", 64, 64, (1, 1, 1))
    x, res = act("pt2x", (2, 4, 4), 64), act("pt2r", (2, 4, 4), 64)
    one, many = both(lambda: (pc.call_pool_t2(x, residual=res, relu=True).buf,), 2 * 4 * 4 * 64)
    assert tuple(one[0].shape) == (N, 1, 4, 4, 64)
    same(one, many)


def test_call_dual(both):
    pc, other = conv("du1", 64, 64, (1, 1, 1)), conv("du2", 64, 64, (1, 1, 1))
    x, x2 = act("dux", (1, 4, 4), 64), act("dux2", (1, 4, 4), 64)
    same(*both(lambda: (pc.call_dual(x, other, x2, relu=True).buf,), 4 * 4 * 64))


def test_gather(both):
    """A 1x3x3 'same' conv over [upsampled half-size source | full-size source], 64 channels each."""
    pc = conv("ga", 64, 128, (1, 3, 3))
    srcs = [(act("gaup", (1, 4, 4), 64), True), (act("gafull", (1, 8, 8), 64), False)]
    one, many = both(lambda: (pc.gather(srcs, pads=(0, 1, 1)).buf,), 8 * 8 * 64)
    assert tuple(one[0].shape) == (N, 1, 8, 8, 64)
    same(one, many)


D = 256


def nl_inputs():
    """theta (N, 2, 3, 3, 256); phi and g the two channel halves of one (N, 2, 1, 2, 512) buffer, as i3res50.nonlocal_forward passes them."""
    pg = act("nlpg", (2, 1, 2), 2 * D)
    return act("nlth", (2, 3, 3), D), pg.slice(0, D), pg.slice(D, D)


@pytest.mark.parametrize("with_lse", [False, True])
def test_nl_attention(both, with_lse):
    from ted_spad_amd import engine as E
    theta, phi, g = nl_inputs()

    def run():
        if not with_lse:
            return (E.nl_attention(theta, phi, g, D ** -0.5).buf,)
        t, lse = E.nl_attention_lse(theta, phi, g, D ** -0.5)
        return t.buf, lse
    same(*both(run, 2 * 3 * 3 * D))


def test_nl_attention_bwd(both):
    from ted_spad_amd import engine as E, train_engine as TE
    theta, phi, g = nl_inputs()
    t, lse = E.nl_attention_lse(theta, phi, g, D ** -0.5)
    dt = E.Act((synth_tensor(17, "nldt", (N, 2, 3, 3, D), -1, 1) * TE.GRAD_SCALE).to(H).cuda(), D)      # scaled, as the training path hands it over
    same(*both(lambda: tuple(a.buf for a in E.nl_attention_bwd(theta, phi, g, t, lse, dt, D ** -0.5)), 2 * 3 * 3 * D))
