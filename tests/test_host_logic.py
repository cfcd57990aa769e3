"""CPU: the C-ABI library loads and exports every symbol include/tedspad_hip.h declares (no
compute calls), the host-side packing logic, the loader's checkpoint fallbacks, and that the
product refuses CPU tensors instead of falling back."""
import ctypes
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_l2
from ted_spad_amd import _lib, engine as E
from ted_spad_amd.synth import synth_state_dict, synth_tensor


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "tedspad_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(tedspad_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), "libtedspad_hip.so lacks %s" % name
    assert declared == set(_lib.SYMBOLS), (declared ^ set(_lib.SYMBOLS))
    assert _lib.lib().tedspad_abi_version() == _lib.ABI_VERSION == 5


# kernels that are allowed to keep private memory, with the reason; everything else in the library must have NO VGPR spill and NO scratch
KNOWN_SCRATCH = {
    # private arrays by design (a rolling window / an 8 x 8 transpose tile), HBM-bound kernels outside the conv stack. (The fused bottleneck tails, white-listed
    # here for three rounds, are spill-free since round 5: their BatchNorm vectors are requested one channel block at a time, csrc/conv_bneck.hip.)
    "maxpool_k3s1_kernel": "rolling column maxima in a private array",
    "to_channels_last_w8_kernel": "8 x 8 transpose tile in a private array",
}


def test_no_kernel_spills_registers():
    """Every code object of libtedspad_hip.so (llvm-readelf --notes): .vgpr_spill_count == 0 and .private_segment_fixed_size == 0 for every kernel but the
    documented exceptions above -- a spill inside a loop that carries asm-issued LDS-DMA costs a vmcnt(0) drain per reload (round-2 review item 2)."""
    import glob
    import shutil
    import subprocess
    import tempfile
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("ROCm LLVM tools not installed")
    tmp = tempfile.mkdtemp()
    try:
        so = os.path.join(tmp, "lib.so")
        shutil.copy(_lib.LIB_PATH, so)
        subprocess.run([objdump, "--offloading", so], cwd=tmp, check=True, capture_output=True)
        cos = glob.glob(os.path.join(tmp, "lib.so.*gfx950*"))
        assert cos, "no gfx950 code objects extracted"
        seen, bad = 0, []
        for co in cos:
            notes = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
            for k in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
                seen += 1
                name = re.search(r"\.name:\s+(\S+)", k).group(1)
                spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", k).group(1))
                scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", k).group(1))
                if (spill or scratch) and not any(tag in name for tag in KNOWN_SCRATCH):
                    bad.append((name, spill, scratch))
        assert seen > 150, "parsed only %d kernels" % seen
        assert not bad, "kernels with VGPR spills / scratch: %s" % bad
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_tail_stage_a_keeps_its_counted_lds_waits():
    """csrc/conv_bneck.hip's stage A requests its MFMA fragments one tap ahead with asm ds_read_b128 and waits with COUNTED s_waitcnt lgkmcnt(12) (hipcc's own
    bookkeeping drained every request at the loop header). Compiles the file to assembly and checks, between the markers the kernel emits, that every
    instantiation still has the requests, the counted waits, and no full drain (lgkmcnt(0)) in front of the MFMAs of the pipelined taps."""
    import subprocess
    import tempfile
    from ted_spad_amd import build as B
    if not os.path.exists(B.HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "conv_bneck.s")
        flags = [f for f in B.FLAGS if f != "-fPIC"]
        subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "conv_bneck.hip"), "-o", out], check=True, capture_output=True)
        text = open(out).read()
    regions = re.findall(r"; BT_COUNTED_LGKM_BEGIN(.*?); BT_COUNTED_LGKM_END", text, flags=re.S)
    assert len(regions) >= 8, "expected the marked region in every instantiation of the 64-channel tail (plain, two-source, pooled x 2 frames; f16 + bf16), found %d" % len(regions)
    for r in regions:
        assert r.count("ds_read_b128") >= 16 * 4 and r.count("s_waitcnt lgkmcnt(12)") >= 4 * 3 + 1
        loop = re.search(r"=>This Inner Loop Header.*?s_cbranch_scc\d \.LBB", r, flags=re.S)      # the steady-state taps
        assert loop and loop.group(0).count("v_mfma") == 16 and "lgkmcnt(0)" not in loop.group(0)
        # hipcc believes an asm request's destination is written when the statement ends: it must not spill or copy such a register inside the region
        # (the bytes land later); the fragments stay put because they are live from the request to the MFMA
        frag = set()
        for a, b in re.findall(r"ds_read_b128 v\[(\d+):(\d+)\]", r):
            frag.update(range(int(a), int(b) + 1))
        moved = []
        for l in r.splitlines():
            code = l.split(";")[0]
            if re.match(r"\s*(scratch_store|v_accvgpr_write|v_mov_b32)", code):
                ops = code.split(None, 1)[1].split(",")
                srcs = re.findall(r"\bv(\d+)\b", ",".join(ops[1:]))          # everything after the first operand (destination / 'off')
                if any(int(v) in frag for v in srcs):
                    moved.append(code.strip())
        assert not moved, "fragment registers spilled / copied inside the counted-wait region: %s" % moved[:4]


C_SCALARS = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}
HEADER_STRUCTS = {"tedspad_conv_desc": _lib.ConvDesc, "tedspad_conv_extras": _lib.ConvExtras, "tedspad_pool_desc": _lib.PoolDesc,
                  "tedspad_pack_job": _lib.PackJob, "tedspad_fold_job": _lib.FoldJob, "tedspad_wgrad_unpack_job": _lib.WgradUnpackJob}


def _header_code():
    """include/tedspad_hip.h without comments and preprocessor lines"""
    hdr = open(os.path.join(ROOT, "include", "tedspad_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", " ", hdr)
    return re.sub(r"^\s*#[^\n]*", " ", hdr, flags=re.M)


def _c_kind(decl, what):
    """'ptr' for any pointer, else the scalar type's name: `decl` is a C type with or without a parameter name. An unknown type raises."""
    if "*" in decl:
        return "ptr"
    words = [t for t in re.findall(r"[A-Za-z_][A-Za-z0-9_]*", decl) if t != "const"]
    assert words and words[0] in C_SCALARS and len(words) <= 2, "%s: a C type this test does not know: %r" % (what, decl.strip())
    return words[0]


def _ctypes_kind(t):
    """the same classes for a ctypes type of the table"""
    if t in (ctypes.c_void_p, ctypes.c_char_p) or isinstance(t, type(ctypes.POINTER(ctypes.c_int32))):
        return "ptr"
    for name, ct in C_SCALARS.items():
        if t is ct:
            return name
    raise AssertionError("a ctypes type this test does not know: %r" % (t,))


def _header_prototypes():
    """name -> (kind of the return type, [kind of each parameter]) for every function include/tedspad_hip.h declares"""
    code = re.sub(r"\{[^{}]*\}", " ", _header_code())        # struct and enum bodies (the extern "C" braces hold no pair without a nested one)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ \t\n\*]*?)\b(tedspad_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", code):
        assert name not in protos, "%s is declared twice" % name
        params = [p for p in params.split(",")] if params.strip() != "void" else []
        protos[name] = (_c_kind(ret + " x", name + " (return type)"), [_c_kind(p, "%s argument %d" % (name, i)) for i, p in enumerate(params)])
    return protos


def test_ctypes_table_mirrors_the_header_argument_by_argument():
    """Every prototype of include/tedspad_hip.h against _lib.SYMBOLS: the return type and every parameter, as pointer / int32_t / int64_t / float / double
    (an int64_t stride bound as c_int32 works at test sizes and truncates at the workload's). A type the parser does not know fails. Then the field types
    of the six structs that cross the ABI, arrays included. No GPU."""
    protos = _header_prototypes()
    declared = set(re.findall(r"\b(tedspad_[a-z0-9_]+)\s*\(", _header_code()))
    assert len(protos) >= 100 and set(protos) == declared == set(_lib.SYMBOLS), set(protos) ^ declared ^ set(_lib.SYMBOLS)
    bad = []
    for name, (ret, args) in sorted(protos.items()):
        res, argtypes = _lib.SYMBOLS[name]
        if _ctypes_kind(res) != ret:
            bad.append("%s: returns %s in the header, %s in the table" % (name, ret, _ctypes_kind(res)))
        if len(argtypes) != len(args):
            bad.append("%s: %d parameters in the header, %d in the table" % (name, len(args), len(argtypes)))
            continue
        for i, (h, t) in enumerate(zip(args, argtypes)):
            if _ctypes_kind(t) != h:
                bad.append("%s argument %d: %s in the header, %s in the table" % (name, i, h, _ctypes_kind(t)))
    assert not bad, "\n".join(bad)
    for ptr_to, struct in ((_lib.ConvDesc, "tedspad_conv_desc"), (_lib.ConvExtras, "tedspad_conv_extras"), (_lib.PoolDesc, "tedspad_pool_desc")):
        users = [n for n, (_, a) in _lib.SYMBOLS.items() if ctypes.POINTER(ptr_to) in a]
        assert users and all(re.search(r"\b%s\s*\([^()]*\b%s\s*\*" % (n, struct), _header_code()) for n in users), (struct, users)
    code = _header_code()
    for cname, cls in HEADER_STRUCTS.items():
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), code, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            if not decl.strip():
                continue
            base = _c_kind(decl.split(",")[0], cname)                  # "const float *w, *scale, *out": every piece carries its own '*'
            for piece in decl.split(","):
                dim = re.search(r"\[(\d+)\]", piece)
                fields.append(("ptr" if "*" in piece else base, int(dim.group(1)) if dim else 0))
        mine = []
        for _, t in cls._fields_:
            n = getattr(t, "_length_", 0) if issubclass(t, ctypes.Array) else 0
            mine.append((_ctypes_kind(t._type_ if n else t), n))
        assert fields == mine, (cname, [i for i, (a, b) in enumerate(zip(fields, mine)) if a != b], len(fields), len(mine))


def test_header_parser_sees_a_wrong_binding():
    """The comparison above is not vacuous: the kinds it derives tell an int64_t from an int32_t, a float from a double, and refuse an unknown type."""
    assert _c_kind("int64_t sn", "t") == "int64_t" != _ctypes_kind(ctypes.c_int32) and _c_kind("const float *x", "t") == "ptr" == _ctypes_kind(ctypes.POINTER(_lib.ConvDesc))
    assert _c_kind("double eps", "t") != _ctypes_kind(ctypes.c_float) and _c_kind("const char *", "t") == _ctypes_kind(ctypes.c_char_p)
    for unknown in ("uint8_t flag", "size_t n", "unsigned long n", "tedspad_conv_desc d"):
        with pytest.raises(AssertionError):
            _c_kind(unknown, "t")
    with pytest.raises(AssertionError):
        _ctypes_kind(ctypes.c_uint8)
    protos = _header_prototypes()
    assert protos["tedspad_clip_to_channels_last"][1][7:12] == ["int64_t"] * 5 and protos["tedspad_bn_fold"][1][5] == "double"
    assert protos["tedspad_last_error"] == ("ptr", []) and protos["tedspad_stem_pt_side_bytes"] == ("int64_t", ["int32_t"] * 4)


def test_job_structs_mirror_the_header():
    """The multi-job launches take arrays of plain C structs (include/tedspad_hip.h: tedspad_pack_job / _fold_job / _wgrad_unpack_job); the ctypes
    mirrors must have the sizes csrc/pack.hip static_asserts and the header's field order -- and so must the descriptors every conv and pool launch takes
    (tedspad_conv_desc / _conv_extras / _pool_desc). No GPU: a null job list is refused by the host check."""
    assert (ctypes.sizeof(_lib.PackJob), ctypes.sizeof(_lib.FoldJob), ctypes.sizeof(_lib.WgradUnpackJob)) == (120, 96, 64)
    hdr = open(os.path.join(ROOT, "include", "tedspad_hip.h")).read()
    for cls, cname in ((_lib.PackJob, "tedspad_pack_job"), (_lib.FoldJob, "tedspad_fold_job"), (_lib.WgradUnpackJob, "tedspad_wgrad_unpack_job"),
                       (_lib.ConvDesc, "tedspad_conv_desc"), (_lib.ConvExtras, "tedspad_conv_extras"), (_lib.PoolDesc, "tedspad_pool_desc")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            for piece in decl.split(","):               # "const float *w", " *scale", "int32_t geo[9]", " nblocks"
                ids = re.findall(r"[A-Za-z_][A-Za-z0-9_]*", re.sub(r"\[\d+\]", "", piece))
                if ids:
                    names.append(ids[-1])
        assert names == [f[0] for f in cls._fields_], (cname, names, [f[0] for f in cls._fields_])
    L = _lib.lib()
    assert L.tedspad_pack_multi(None, 0, None, 0, None) != 0 and b"tedspad_pack_multi" in L.tedspad_last_error()


def test_ktab_and_padding_helpers():
    d = _lib.ConvDesc(n=1, t=4, h=6, w=5, cin=16, ldx=24, cout=40, ldy=40, ldres=0, kt=3, kh=3, kw=3, st=1, sh=1, sw=1,
                      pt=1, ph=1, pw=1, to=4, ho=6, wo=5, relu=1, dtype=0, tile_cfg=0)
    L = _lib.lib()
    assert L.tedspad_conv_kpad(d) == 448 and L.tedspad_conv_cout_pad(d) == 128 and L.tedspad_conv_ktab_entries(d) == 56
    buf = (ctypes.c_int32 * 112)()
    assert L.tedspad_conv_build_ktab(d, buf) == 0
    tab = np.array(buf).reshape(56, 2)
    for e in range(54):
        tap, c8 = divmod(e, 2)
        dt, dh, dw = tap // 9, (tap // 3) % 3, tap % 3
        assert tab[e, 0] == ((dt * 6 + dh) * 5 + dw) * 24 + c8 * 8
        assert tab[e, 1] == dt | ((8 + dh) << 8) | ((16 + dw) << 16)
    assert (tab[54:, 1] == (31 | 31 << 8 | 31 << 16)).all()      # K padding -> zero page
    bad = _lib.ConvDesc(n=1, t=1, h=1, w=1, cin=12, ldx=12, cout=8, ldy=8, kt=1, kh=1, kw=1, st=1, sh=1, sw=1, to=1, ho=1, wo=1)
    assert L.tedspad_conv_kpad(bad) < 0                           # cin not a multiple of 8
    assert L.tedspad_conv_fwd(ctypes.byref(bad), None, None, None, None, None, None, None, 0, None) < 0
    assert b"descriptor" in L.tedspad_last_error()


@pytest.mark.parametrize("k,pw", [((5, 7, 7), 3), ((7, 7, 7), 2)])
def test_stem_pair_rewrite_is_the_same_convolution(k, pw):
    """PackedConv(pair_w=...) turns the Cin=3 stride-2 stem into an 8-channel conv over pixel pairs."""
    from oracle.conv_ref import conv_cl
    w = synth_tensor(0, "w", (16, 3) + k, -1, 1)
    x = synth_tensor(0, "x", (1, 3, 6, 12, 12))
    pc = E.PackedConv(w, torch.ones(16), torch.zeros(16), stride=(2, 2, 2), dtype="f16", device="cpu", pair_w=pw)
    kt, kh, kw2 = pc.k
    w2 = pc.w[:16, :kt * kh * kw2 * 8].float().reshape(16, kt, kh, kw2, 8).permute(0, 4, 1, 2, 3)   # back to (co, ci, kt, kh, kw)
    xp = torch.zeros(1, 6, 12, 6, 8)
    xp.view(1, 6, 12, 6, 2, 4)[..., :3] = x.permute(0, 2, 3, 4, 1).reshape(1, 6, 12, 6, 2, 3)
    pf = (k[0] // 2, 3, pw) if pw == 3 else (2, 2, 2)
    pb = (k[0] // 2, 3, 3) if pw == 3 else (3, 3, 3)
    ref = conv_cl(x.permute(0, 2, 3, 4, 1), w.half().float(), torch.ones(16), torch.zeros(16), (2, 2, 2), pf, pb, relu=False)
    got = conv_cl(xp, w2, torch.ones(16), torch.zeros(16), (2, 2, 1), (pf[0], pf[1], pc.pair_pw),
                  (pb[0], pb[1], kw2 - 1 - pc.pair_pw), relu=False)
    assert got.shape == ref.shape and rel_l2(got, ref) < 1e-6


def test_fold_bn_matches_torch_batchnorm_eval():
    bn = torch.nn.BatchNorm3d(8, eps=1e-3).eval()
    sd = synth_state_dict(bn.state_dict(), 3)
    bn.load_state_dict(sd)
    x = synth_tensor(3, "x", (2, 8, 2, 3, 3), -2, 2)
    s, b = E.fold_bn(sd["weight"], sd["bias"], sd["running_mean"], sd["running_var"], 1e-3)
    assert torch.allclose(bn(x), x * s.view(1, -1, 1, 1, 1) + b.view(1, -1, 1, 1, 1), atol=1e-6)


def test_same_pads_rule():
    assert E.same_pads(224, 7, 2) == (2, 3) and E.same_pads(16, 7, 2) == (2, 3)
    assert E.same_pads(112, 3, 2) == (0, 1) and E.same_pads(7, 2, 2) == (0, 1) and E.same_pads(28, 3, 1) == (1, 1)


def test_loader_signatures_and_checkpoint_fallbacks(tmp_path, capsys):
    from ted_spad_amd import model_loaders as ml
    assert ml.load_ft_model() is None                      # default arch 'r3d' matches no branch (model_loaders.py:65-67)
    assert "invalid for ft_model" in capsys.readouterr().out
    assert ml.load_fa_model(arch="nope") is None
    upp = ml.load_fa_model()                               # default arch 'unet++' (model_loaders.py:17): smp's UnetPlusPlus, restated
    assert "freshly initialized" in capsys.readouterr().out
    keys = list(upp.state_dict())
    assert len(keys) == 206 and sum(p.numel() for p in upp.parameters()) == 13898787
    for k, shape in (("encoder.conv1.weight", (64, 3, 7, 7)), ("encoder.layer2.0.downsample.0.weight", (128, 64, 1, 1)),
                     ("encoder.layer4.1.bn2.running_var", (512,)),                      # ResNetEncoder keeps layer4 at depth 4
                     ("decoder.blocks.x_0_0.conv1.0.weight", (256, 384, 3, 3)), ("decoder.blocks.x_1_1.conv1.0.weight", (64, 192, 3, 3)),
                     ("decoder.blocks.x_2_2.conv2.1.num_batches_tracked", ()), ("decoder.blocks.x_0_1.conv1.0.weight", (128, 384, 3, 3)),
                     ("decoder.blocks.x_1_2.conv1.0.weight", (64, 192, 3, 3)), ("decoder.blocks.x_0_2.conv1.0.weight", (64, 320, 3, 3)),
                     ("decoder.blocks.x_0_3.conv1.0.weight", (32, 64, 3, 3)), ("segmentation_head.0.weight", (3, 32, 3, 3)),
                     ("segmentation_head.0.bias", (3,))):
        assert tuple(upp.state_dict()[k].shape) == shape, k
    assert not any(k.startswith("encoder.fc") or "attention" in k for k in keys)
    pu = str(tmp_path / "upp.pth")                         # DataParallel-style 'module.' checkpoint (model_loaders.py:38-46)
    torch.save({"fa_model_state_dict": {"module." + k: v for k, v in upp.state_dict().items()}}, pu)
    assert ml.load_fa_model(saved_model_file=pu) is not None and "loaded from" in capsys.readouterr().out
    ft = ml.load_ft_model("largei3d", num_classes=102)
    sd = synth_state_dict(ft.state_dict(), 5)
    # (1) plain checkpoint dict, as train_anonymizer.py:519-550 writes it
    p1 = str(tmp_path / "a.pth")
    torch.save({"epoch": 3, "ft_model_state_dict": sd, "fa_model_state_dict": ml.load_fa_model(arch="unet").state_dict()}, p1)
    m1 = ml.load_ft_model("largei3d", saved_model_file=p1, num_classes=102)
    assert torch.equal(m1.state_dict()["i3d.layer3.2.conv2.weight"], sd["i3d.layer3.2.conv2.weight"])
    # (2) FrozenBN-style keys: `scale` instead of `weight`, no num_batches_tracked (model_loaders.py:76-82)
    frozen = OrderedDict()
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            continue
        is_bn = k.rsplit(".", 1)[0] + ".running_mean" in sd
        frozen[k.replace(".weight", ".scale") if (is_bn and k.endswith(".weight")) else k] = v
    p2 = str(tmp_path / "b.pth")
    torch.save({"ft_model_state_dict": frozen}, p2)
    m2 = ml.load_ft_model("largei3d", saved_model_file=p2, num_classes=102)
    assert torch.equal(m2.state_dict()["i3d.bn1.weight"], sd["i3d.bn1.weight"])
    # (3) bare I3Res50 dict -> ft_model.i3d.load_state_dict (model_loaders.py:84)
    p3 = str(tmp_path / "c.pth")
    torch.save({"ft_model_state_dict": OrderedDict((k[4:], v) for k, v in sd.items() if k.startswith("i3d."))}, p3)
    m3 = ml.load_ft_model("largei3d", saved_model_file=p3, num_classes=102)
    assert torch.equal(m3.state_dict()["i3d.fc.weight"], sd["i3d.fc.weight"])
    # (4) fa: DataParallel 'module.' prefix (model_loaders.py:41-46)
    fa_sd = synth_state_dict(ml.load_fa_model(arch="unet").state_dict(), 5)
    p4 = str(tmp_path / "d.pth")
    torch.save({"fa_model_state_dict": OrderedDict(("module." + k, v) for k, v in fa_sd.items())}, p4)
    fa = ml.load_fa_model(saved_model_file=p4, arch="unet")
    assert torch.equal(fa.state_dict()["up1.conv.double_conv.0.weight"], fa_sd["up1.conv.double_conv.0.weight"])
    # the i3d logits are registered first and can be replaced
    inc = ml.load_ft_model("i3d", num_classes=400)
    assert list(inc.state_dict())[0] == "logits.conv3d.weight"
    inc.replace_logits(102)
    assert inc.state_dict()["logits.conv3d.weight"].shape == (102, 1024, 1, 1, 1)


def test_no_cpu_fallback():
    from ted_spad_amd import model_loaders as ml
    ft = ml.load_ft_model("largei3d", num_classes=102).eval()
    with pytest.raises(_lib.TedSpadHipError):
        ft.i3d.extract_features(torch.zeros(1, 3, 16, 32, 32))
    fa = ml.load_fa_model(arch="unet").eval()
    with pytest.raises(_lib.TedSpadHipError):
        fa(torch.zeros(1, 3, 32, 32))
    from ted_spad_amd.losses import NTXentLoss
    with pytest.raises(_lib.TedSpadHipError):
        NTXentLoss("cpu", 4, 0.1, False)(torch.zeros(4, 8), torch.zeros(4, 8))
    for holder in (ft.i3d.conv1, ft.i3d.bn1, ft.mlp.fc1):
        with pytest.raises(RuntimeError):
            holder(torch.zeros(1))
    # the decoded-frames entries (round 5): frames / records on the CPU are refused, not converted by some host path
    from ted_spad_amd import extraction, preprocess
    with pytest.raises(_lib.TedSpadHipError):
        extraction.extract_video_features_uint8(ft, torch.zeros((32, 24, 32, 3), dtype=torch.uint8), out_hw=(16, 16))
    with pytest.raises(_lib.TedSpadHipError):
        preprocess.crop_resize_records(torch.zeros((32, 24, 32, 3), dtype=torch.uint8), (0, 0, 24, 32), (16, 16), None, 1)
    with pytest.raises(_lib.TedSpadHipError):
        ft.i3d.extract_features_records(torch.zeros((1, 4, 16, 2, 8, 24), dtype=torch.float16))


def test_resize_aa_table_matches_torch_antialias_weights():
    """Host builder of the antialiased-resize weights (tedspad_resize_aa_table, no GPU involved) against the dense
    resize matrix read off torch.nn.functional.interpolate(antialias=True) itself -- the call behind
    torchvision F.resize in dali_extraction.py:49. Tolerance: 2e-6 absolute on weights in [0,1] (fp32 rounding)."""
    from oracle import preprocess_ref
    from ted_spad_amd import preprocess
    for n_in, n_out in [(864, 224), (576, 224), (224, 224), (100, 224), (1080, 7), (5, 3), (3, 5)]:
        tab = preprocess.aa_table_host(n_in, n_out)
        dense = np.zeros((n_out, n_in), np.float32)
        for i in range(n_out):
            lo, cnt = int(tab[i, 0]), int(tab[i, 1])
            assert 0 <= lo and lo + cnt <= n_in and cnt <= tab.shape[1] - 2
            dense[i, lo:lo + cnt] = tab[i, 2:2 + cnt].view(np.float32)
        ref = preprocess_ref.resize_matrix(n_in, n_out).numpy()
        assert np.abs(dense - ref).max() < 2e-6, (n_in, n_out, np.abs(dense - ref).max())
        assert np.allclose(dense.sum(1), 1.0, atol=1e-5)


def test_crop_boxes():
    from ted_spad_amd import preprocess
    assert preprocess.center_crop_box(1080, 1920, 864, 1536) == (108, 192, 864, 1536)
    assert preprocess.center_crop_box(241, 321, 192, 256) == (24, 32, 192, 256)       # 24.5 -> 24, 32.5 -> 32: half to even
    boxes = preprocess.ten_crop_boxes(256, 340, 224, 224)
    assert len(boxes) == 10 and boxes[0] == (0, 0, 224, 224, False) and boxes[4][:2] == (16, 58)
    assert boxes[5] == (0, 116, 224, 224, True) and boxes[6] == (0, 0, 224, 224, True)  # flipped tl = right edge of the frame
    with pytest.raises(ValueError):
        preprocess.center_crop_box(100, 100, 120, 50)


def test_save_features_batched(tmp_path):
    from ted_spad_amd.extraction import save_features_batched
    a, b = synth_tensor(0, "fa", (5, 16)), synth_tensor(0, "fb", (3, 10, 8))
    paths = save_features_batched(str(tmp_path), [("/x/y/Abuse001_x264.mp4", a), ("Normal_7.avi", b)])
    assert [os.path.basename(p) for p in paths] == ["Abuse001_x264.npy", "Normal_7.npy"]
    la, lb = np.load(paths[0]), np.load(paths[1])
    assert la.dtype == np.float64 and la.shape == (5, 16) and np.array_equal(la, a.numpy().astype(np.float64))
    assert lb.shape == (3, 10, 8) and np.array_equal(lb, b.numpy().astype(np.float64))


def test_fb_model_has_torchvision_resnet50_keys():
    """fb = nn.Sequential(resnet50(fc=Identity), MLP) (model_loaders.py:124-153): key names / counts of
    torchvision.models.resnet50 so `fb_model_state_dict` checkpoints load strict=True (incl. the 'module.' fallback)."""
    from ted_spad_amd.model_loaders import load_fb_model
    fb = load_fb_model(arch="r50", ssl=True)
    sd = fb.state_dict()
    assert len(sd) == 322 and sum(p.numel() for p in fb.parameters()) == 23508032 + 2048 * 2048 + 2048 + 2048 * 128 + 128
    for k, shape in {"0.conv1.weight": (64, 3, 7, 7), "0.bn1.running_var": (64,), "0.layer1.0.conv1.weight": (64, 64, 1, 1),
                     "0.layer1.0.downsample.0.weight": (256, 64, 1, 1), "0.layer2.0.conv2.weight": (128, 128, 3, 3),
                     "0.layer4.2.bn3.num_batches_tracked": (), "1.fc1.bias": (2048,), "1.fc2.weight": (128, 2048)}.items():
        assert tuple(sd[k].shape) == shape, k
    assert not any(k.startswith("0.fc") for k in sd)                      # fc = nn.Identity()
    pred = load_fb_model(arch="r50", ssl=False, num_pa=7)
    assert tuple(pred.state_dict()["fc.weight"].shape) == (7, 2048) and len(pred.state_dict()) == 320


def test_kinetics_pretrained_classifiers_load_strictly_then_get_the_new_head(tmp_path, monkeypatch):
    """model_loaders.py:171-196: with `pretrained` the network is built with Kinetics' 400 classes, the checkpoint loaded strict=True (InceptionI3d:
    `rgb_imagenet.pt` into the model, I3Res50: `i3d_r50_kinetics.pth` into `.i3d`), then the head replaced for `num_classes`; without it the network
    is built for `num_classes` directly. The checkpoints here are written by the test (the real ones are downloads)."""
    import contextlib, io
    from ted_spad_amd import model_loaders as ML
    from ted_spad_amd.inception_i3d import InceptionI3d
    from ted_spad_amd.synth import synth_state_dict
    with contextlib.redirect_stdout(io.StringIO()):
        big = ML.wrapper_i3d(num_classes=400)
        inc = InceptionI3d(num_classes=400, dropout_keep_prob=0.5)
    sd_big, sd_inc = synth_state_dict(big.i3d.state_dict(), 3), synth_state_dict(inc.state_dict(), 4)
    torch.save(sd_big, tmp_path / "i3d_r50_kinetics.pth")
    torch.save(sd_inc, tmp_path / "rgb_imagenet.pt")
    monkeypatch.setattr(ML, "SAVED_MODELS_DIR", str(tmp_path))
    with contextlib.redirect_stdout(io.StringIO()):
        m = ML.build_largei3d_classifier(num_classes=102, pretrained=True)
        m400 = ML.build_largei3d_classifier(num_classes=400, pretrained=True)
        i = ML.build_i3d_classifier(num_classes=102, pretrained=True)
        fresh = ML.build_largei3d_classifier(num_classes=7, pretrained=False)
    assert tuple(m.i3d.fc.weight.shape) == (102, 2048) and tuple(m400.i3d.fc.weight.shape) == (400, 2048) and tuple(fresh.i3d.fc.weight.shape) == (7, 2048)
    for k, v in m.i3d.state_dict().items():
        if not k.startswith("fc."):
            assert torch.equal(v, sd_big[k]), k
    assert torch.equal(m400.i3d.fc.weight, sd_big["fc.weight"])              # 400 classes: the checkpoint's own head stays
    assert i.logits.conv3d.weight.shape[0] == 102
    got = i.state_dict()
    for k, v in sd_inc.items():
        if not k.startswith("logits."):
            assert torch.equal(got[k], v), k
    monkeypatch.setattr(ML, "SAVED_MODELS_DIR", str(tmp_path / "nowhere"))
    with pytest.raises(FileNotFoundError):
        ML.build_largei3d_classifier(num_classes=102, pretrained=True)


def test_device_flag_reads_its_tensor_once_and_on_demand():
    """`skipped` of a training-step result (train_step.DeviceFlag): the truth value of a 0-d tensor, read when somebody looks (bool / == / repr / hash), once."""
    from ted_spad_amd.train_step import DeviceFlag
    for v, want in ((0.0, False), (1.0, True), (3.0, True)):
        f = DeviceFlag(torch.tensor(v))
        assert f._v is None                       # nothing read yet
        assert bool(f) is want and f == want and (f != (not want)) and repr(f) == "DeviceFlag(%s)" % want and hash(f) == hash(want)
        assert f._t is None                       # the tensor is dropped after the first read
    d = {"skipped": DeviceFlag(torch.tensor(0.0))}
    assert not d["skipped"] and (True if not d["skipped"] else False)


def test_sample_chunks_and_act_sample_range(monkeypatch):
    """engine.sample_chunks: ranges of whole samples under the limit the caller reads from the module when it calls, the whole batch as (0, n) alone, a
    loud failure for a single sample that does not fit; Act.samples: the same channel view of samples [n0, n1), the Act itself for the whole batch."""
    per = 100
    assert list(E.sample_chunks(6, [per], 3 * per + 1)) == [(0, 3), (3, 6)]
    assert list(E.sample_chunks(5, [per, 7], 2 * per + 1)) == [(0, 2), (2, 4), (4, 5)]
    for n in (1, 4):
        assert list(E.sample_chunks(n, [per], E.MAX_ELEMS)) == [(0, n)]
    assert list(E.sample_chunks(6, [per], 1 << 20, [10], 2 * 10 + 1)) == [(0, 2), (2, 4), (4, 6)]     # a second (sizes, limit) pair: the weight gradient's pixel count
    with pytest.raises(_lib.TedSpadHipError, match="single sample"):
        list(E.sample_chunks(2, [1 << 31], E.MAX_ELEMS))
    monkeypatch.setattr(E, "MAX_ELEMS", 3 * per + 1)              # lowered after import, as the GPU tests do: read at call time
    assert list(E.sample_chunks(6, [per], E.MAX_ELEMS)) == [(0, 3), (3, 6)]
    with pytest.raises(_lib.TedSpadHipError, match="single sample"):
        list(E.sample_chunks(2, [3 * per + 1], E.MAX_ELEMS))
    a = E.Act(torch.zeros((5, 2, 3, 4, 32), dtype=torch.float16), 8, 16)
    assert a.samples(0, 5) is a
    for n0, n1 in ((0, 2), (2, 4), (4, 5)):
        s = a.samples(n0, n1)
        assert (s.c, s.coff, s.ld, s.cpad) == (a.c, a.coff, a.ld, a.cpad) and s.dims == (n1 - n0, 2, 3, 4)
        assert s.ptr == a.ptr + n0 * 2 * 3 * 4 * 32 * 2
    assert E.Act(a.buf, 8, 0, 4).samples(1, 3).cpad == 4
    assert E.dtype_code(a.buf) == _lib.F16 and E.dtype_code(a.buf.bfloat16()) == _lib.BF16
