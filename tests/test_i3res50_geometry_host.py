"""CPU: the geometry table of tests/i3res50_geometry.py -- it reaches every launch form of I3Res50._trunk, its size rules are the oracle's, the
matched-rounding oracle leaves room under the feature gate at every entry, and the oracle raises on what the reference cannot take."""
import pytest
import torch

import i3res50_geometry as G


def test_every_branch_is_reached_by_a_table_entry():
    """A condition, not a measurement: a launch form that no run of the GPU file's table reaches fails here."""
    reached = {}
    for name, use_nl, input_form in G.RUNS:
        for label in G.expected_sequence(G.GEOMETRIES[name], use_nl, input_form):
            reached.setdefault(G.form(label), (name, use_nl, input_form))
    assert set(reached) == set(G.BRANCHES), (sorted(set(G.BRANCHES) - set(reached)), sorted(set(reached) - set(G.BRANCHES)))


@pytest.mark.parametrize("name", list(G.GEOMETRIES))
def test_entry_reaches_what_the_table_says(name):
    seq = G.expected_sequence(G.GEOMETRIES[name])
    assert len(seq) == len(set(seq))
    missing = [label for label in G.REACHES[name] if label not in seq]
    assert not missing, (missing, seq)


def test_sequence_of_a_production_clip_spelled_out():
    """16 x 216^2 takes 16 x 224^2's forms (I3Res50._stem / _bottleneck read at t = 4 -> 2 and 53 / 27 / 14 / 7 pixel frames), written out by hand."""
    blocks = lambda li, forms: ["layer%d.%d:%s" % (li, i, f) for i, fs in enumerate(forms) for f in fs]
    want = (["stem:conv_pool_clip"] +
            blocks(1, [["conv1", "tail_dual+fold2"], ["tail+fold"], ["tail+pool_t2"]]) +
            blocks(2, [["conv1_tpair", "conv2", "dual_p8"], ["conv1", "tail"], ["conv1_tpair", "tail"], ["conv1", "tail"]]) +
            blocks(3, [["conv1_tpair", "conv2", "dual_p8"]] + [["frame"]] * 5) +
            blocks(4, [["conv1", "conv2", "dual_p8"], ["conv1_tpair", "conv2", "conv3"], ["conv1", "conv2", "conv3"]]) + ["avgpool"])
    assert G.expected_sequence(G.GEOMETRIES["f14_t2"]) == want
    assert G.expected_sequence((2, 16, 224, 224)) == want and G.expected_sequence((1, 16, 112, 112))[:6] == want[:6]


def test_prefix_and_input_form_sequences():
    g = G.GEOMETRIES["t8"]
    full = G.expected_sequence(g)
    assert G.expected_sequence(g, layers=1) == full[:full.index("layer2.0:conv1")] + ["avgpool"]            # the pool is fused: no maxpool2 launch
    assert G.expected_sequence(G.GEOMETRIES["t12"], layers=1)[-3:] == ["layer1.2:conv2", "layer1.2:conv3+pool_t2", "avgpool"]
    assert G.expected_sequence(g, input_form="records")[:2] == ["stem:conv_pool", "layer1.0:conv1"]
    assert G.expected_sequence(g, input_form="offset4")[:2] == ["stem:layout", "stem:conv_pool"]
    assert G.expected_sequence(g, input_form="tslice") == full
    assert G.expected_sequence(g, input_form="wstride")[:2] == ["stem:pair", "maxpool1"]
    assert G.expected_sequence(g, input_form="wstride")[2:] == full[1:]
    taps = G.expected_sequence(g, input_form="taps")
    assert taps[:7] == ["stem:pair", "maxpool1", "layer1.0:conv1", "layer1.0:conv2", "layer1.0:down", "layer1.0:conv3", "layer1.1:conv1"]
    assert taps.count("maxpool2") == 1 and taps[-1] == "layer4.2:conv3" and len(taps) == 2 + 1 + 3 * 16 + 4
    nl = G.expected_sequence(g, use_nl=True)
    assert [l for l in nl if l not in full] == ["%s:nl_%s" % (b, f) for b in G.nl_ref.NL_BLOCKS for f in ("theta", "pool", "phi_g", "attention", "out")]


@pytest.mark.parametrize("name", list(G.GEOMETRIES))
def test_stage_dims_are_the_oracles(name):
    geometry = G.GEOMETRIES[name]
    taps = G.oracle(name)
    dims = G.stage_dims(geometry)
    assert list(dims) == list(G.STAGES)
    for stage, d in dims.items():
        assert tuple(taps[stage].shape[2:]) == d and taps[stage].shape[0] == geometry[0], (stage, tuple(taps[stage].shape), d)
    assert tuple(taps["feature"].shape) == (geometry[0], 2048, 1, 1, 1)
    assert tuple(G.stage_ref(taps, "layer1").shape[2:]) == (dims["layer2"][0],) + dims["layer1"][1:]


@pytest.mark.parametrize("name", list(G.GEOMETRIES))
def test_matched_rounding_leaves_room_under_the_gate(name):
    """The f16 matched-rounding oracle's feature is within 1e-3 rel-L2 (the project's feature gate) of the fp32 oracle's, per clip: a device that rounds
    where that oracle does can meet the gate at this geometry."""
    ref, m = G.oracle(name), G.oracle(name, torch.float16)
    print("%s: matched-rounding f16 vs fp32 oracle, rel-L2: %s  feature %.3e (worst clip %.3e)" % (
        name, "  ".join("%s %.2e" % (s, G.rel_l2(m[s], ref[s])) for s in G.STAGES), G.rel_l2(m["feature"], ref["feature"]),
        G.worst_position(m["feature"], ref["feature"])))
    assert G.worst_position(m["feature"], ref["feature"]) < 1e-3


@pytest.mark.parametrize("name", list(G.REFUSED))
def test_oracle_raises_on_what_the_reference_cannot_take(name):
    geometry, use_nl, _ = G.REFUSED[name]
    with pytest.raises(RuntimeError):
        G.oracle_on(G.clip(geometry), None, use_nl)
    if use_nl:
        G.oracle_on(G.clip(geometry), None, False)            # the plain network takes it
        dims = G.stage_dims(geometry)
        assert dims["layer2"][1:] == (2, 2) and dims["layer3"][1:] == (1, 1)


@pytest.mark.parametrize("name", G.NL_ENTRIES)
def test_matched_rounding_leaves_room_under_the_gate_with_nonlocal_blocks(name):
    ref, m = G.oracle(name, None, True), G.oracle(name, torch.float16, True)
    print("%s use_nl: matched-rounding f16 vs fp32 oracle, rel-L2: %s  feature (worst clip) %.3e" % (
        name, "  ".join("%s %.2e" % (s, G.rel_l2(m[s], ref[s])) for s in G.STAGES), G.worst_position(m["feature"], ref["feature"])))
    assert G.worst_position(m["feature"], ref["feature"]) < 1e-3
    assert G.rel_l2(ref["layer2"], G.oracle(name)["layer2"]) > 1e-2            # the blocks do change the maps


@pytest.fixture(scope="module")
def host_nets():
    from ted_spad_amd.i3res50 import I3Res50
    return {use_nl: I3Res50(num_classes=4, use_nl=use_nl) for use_nl in (False, True)}


def frames_behind_maxpool1(T):
    return ((T + 2 * 2 - 5) // 2 + 1) // 2


@pytest.mark.parametrize("name", list(G.REFUSED))
def test_geometry_check_refuses_what_the_oracle_raises_on(name, host_nets):
    (n, T, H, W), use_nl, what = G.REFUSED[name]
    with pytest.raises(ValueError, match=what):
        host_nets[use_nl]._check_geometry(frames_behind_maxpool1(T), H, W, (n, 3, T, H, W))


def test_geometry_check_takes_the_table_and_the_smallest_clips(host_nets):
    for name, (n, T, H, W) in G.GEOMETRIES.items():
        for use_nl in (False, True):
            host_nets[use_nl]._check_geometry(frames_behind_maxpool1(T), H, W, (n, 3, T, H, W))
    host_nets[False]._check_geometry(frames_behind_maxpool1(7), 5, 6, (1, 3, 7, 5, 6))           # the smallest clip the reference takes
    G.oracle_on(G.clip((1, 7, 5, 6)))
    host_nets[True]._check_geometry(frames_behind_maxpool1(7), 21, 22, (1, 3, 7, 21, 22))        # layer3 frames 2 x 2
    G.oracle_on(G.clip((1, 7, 21, 22)), None, True)
    with pytest.raises(ValueError, match="at least 5 x 5"):
        host_nets[False]._check_geometry(2, 40, 4, (1, 3, 8, 40, 4))
