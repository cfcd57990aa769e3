"""No GPU: structure of csrc/conv_bneck_fold.hip's stage A in the compiled assembly, and the host-side weight image of engine.BneckTailFold."""
import os
import re

import pytest
import torch


def test_fold_stage_a_keeps_its_counted_lds_waits():
    """Stage A of the folded tail requests its MFMA fragments one tap ahead with asm ds_read_b128 and waits with counted s_waitcnt lgkmcnt, like
    conv_bneck.hip's (test_host_logic.py::test_tail_stage_a_keeps_its_counted_lds_waits). Between the kernel's markers every instantiation must have the
    requests of nine unrolled taps, their 144 MFMAs, the counted waits, a full drain only on the last tap, and no copy or spill of a fragment register
    (hipcc believes an asm request's destination is written when the statement ends; the bytes land later)."""
    import subprocess
    import tempfile
    from ted_spad_amd import build as B
    if not os.path.exists(B.HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "conv_bneck_fold.s")
        flags = [f for f in B.FLAGS if f != "-fPIC"]
        subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "conv_bneck_fold.hip"), "-o", out], check=True, capture_output=True)
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


def test_fold_weight_image_layout():
    """w1p[g][dt][co][k]: the dt = 1 tile's columns in the accumulator k order of BneckTail.PERM, the others natural (include/tedspad_hip.h)."""
    from ted_spad_amd import engine as E
    w1 = torch.arange(64 * 256 * 3, dtype=torch.float32).reshape(64, 256, 3, 1, 1) % 2039      # exact in f16
    tail = type("T", (), {})()
    tail.cmid, tail.cout3, tail.dual = 64, 256, False
    tail.conv2 = type("C", (), {"device": torch.device("cpu"), "torch_dtype": torch.float16, "k": (1, 3, 3)})()
    assert E.BneckTailFold.supported(tail, w1)
    img = E.BneckTailFold(tail, None, w1).w1p.float()
    assert tuple(img.shape) == (4, 3, 64, 64)
    for g in range(4):
        for dt in range(3):
            cols = [64 * g + (E.BneckTail.PERM[k] if dt == 1 else k) for k in range(64)]
            assert torch.equal(img[g, dt], w1[:, cols, dt, 0, 0])
