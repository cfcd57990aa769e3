"""No GPU: structure of csrc/conv_bneck_fold_dual.hip's stage A in the compiled assembly (the body it shares with conv_bneck_fold.hip, csrc/conv_bneck_fold.h),
and the host-side weight image of engine.BneckTailFoldDual."""
import os
import re

import pytest
import torch


def test_dual_fold_stage_a_keeps_its_counted_lds_waits():
    """test_l1_fold_host.py::test_fold_stage_a_keeps_its_counted_lds_waits pointed at the downsample form's source file: the file instantiates the DUAL form
    only (the marked region once per storage type), and stage A is the plain fold's: nine unrolled taps' requests, their 144 MFMAs, the counted waits, a full
    drain only on the last tap, and no copy or spill of a fragment register."""
    import subprocess
    import tempfile
    from ted_spad_amd import build as B
    if not os.path.exists(B.HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "conv_bneck_fold_dual.s")
        flags = [f for f in B.FLAGS if f != "-fPIC"]
        subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "conv_bneck_fold_dual.hip"), "-o", out], check=True, capture_output=True)
        text = open(out).read()
    regions = re.findall(r"; FD_COUNTED_LGKM_BEGIN(.*?); FD_COUNTED_LGKM_END", text, flags=re.S)
    assert len(regions) == 2, "expected the marked region once per storage type, found %d" % len(regions)
    for r in regions:
        assert r.count("ds_read_b128") == 9 * 16 and 8 * 16 < r.count("v_mfma") <= 9 * 16      # (the last tap's MFMAs may sink below the end marker)
        assert r.count("s_waitcnt lgkmcnt(12)") == 8 * 4 + 1 and r.count("s_waitcnt lgkmcnt(0)") == 1
        assert r.count("s_barrier") == 7 and r.count("global_load_lds_dwordx4") == 7 * 2
        frag = set()
        for a, b in re.findall(r"ds_read_b128 v\[(\d+):(\d+)\]", r):
            frag.update(range(int(a), int(b) + 1))
        moved = []
        for l in r.splitlines():
            code = l.split(";")[0]
            if re.match(r"\s*(scratch_store|v_accvgpr_write|v_mov_b32)", code):
                ops = code.split(None, 1)[1].split(",")
                srcs = re.findall(r"\bv(\d+)\b", ",".join(ops[1:]))
                if any(int(v) in frag for v in srcs):
                    moved.append(code.strip())
        assert not moved, "fragment registers spilled / copied inside the counted-wait region: %s" % moved[:4]
    # the budgets of the kernel's metadata: no scratch, no spill, at most 256 registers (two workgroups per CU with the 78 KB of LDS the launch asks for)
    for k in re.split(r"\n\s+- \.agpr_count", text)[1:]:
        if "conv_bneck_fold_kernel" not in k:
            continue
        g = lambda f: int(re.search(r"\.%s:\s+(\d+)" % f, k).group(1))
        assert g("vgpr_count") <= 256 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0 and g("private_segment_fixed_size") == 0


def test_dual_fold_weight_image_layout():
    """w1p[g][dt][co][k] as BneckTailFold's: the dt = 1 tile's columns in the accumulator k order of BneckTail.PERM, the others natural (include/tedspad_hip.h);
    the class takes the two-source tail only, BneckTailFold the plain one only."""
    from ted_spad_amd import engine as E
    w1 = torch.arange(64 * 256 * 3, dtype=torch.float32).reshape(64, 256, 3, 1, 1) % 2039      # exact in f16
    tail = type("T", (), {})()
    tail.cmid, tail.cout3, tail.dual = 64, 256, True
    tail.conv2 = type("C", (), {"device": torch.device("cpu"), "torch_dtype": torch.float16, "k": (1, 3, 3)})()
    assert E.BneckTailFoldDual.supported(tail, w1) and not E.BneckTailFold.supported(tail, w1)
    assert not issubclass(E.BneckTailFoldDual, E.BneckTailFold)
    img = E.BneckTailFoldDual(tail, None, w1).w1p.float()
    assert tuple(img.shape) == (4, 3, 64, 64)
    for g in range(4):
        for dt in range(3):
            cols = [64 * g + (E.BneckTail.PERM[k] if dt == 1 else k) for k in range(64)]
            assert torch.equal(img[g, dt], w1[:, cols, dt, 0, 0])
    tail.dual = False
    assert not E.BneckTailFoldDual.supported(tail, w1)
    tail.dual = True
    for shape in ((64, 256, 1, 1, 1), (128, 256, 3, 1, 1), (64, 128, 3, 1, 1)):
        assert not E.BneckTailFoldDual.supported(tail, torch.zeros(shape))
