"""No GPU: the budgets of the fp32-clip stem's two loader-wave instantiations (csrc/conv_stem_pt.hip: the wave-uniform task deal and the per-lane one) in the compiled
assembly's kernel metadata, the shape of the uniform deal's loads, and the LDS image both are launched with."""
import os
import re

import pytest


@pytest.fixture(scope="module")
def stem_asm():
    import subprocess
    import tempfile
    from ted_spad_amd import build as B
    if not os.path.exists(B.HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "conv_stem_pt.s")
        flags = [f for f in B.FLAGS if f != "-fPIC"]
        subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "conv_stem_pt.hip"), "-o", out], check=True, capture_output=True)
        return open(out).read()


# conv_stem_pt_kernel<T, 8, true, 16, true, 8, UNI>: the mangled template arguments after the storage type
LOADER_FORMS = {"uniform": "Li8ELb1ELi16ELb1ELi8ELb1E", "per-lane": "Li8ELb1ELi16ELb1ELi8ELb0E"}


def test_loader_instantiations_keep_their_budgets(stem_asm):
    """Both deals, both storage types: at most 128 registers (16 waves of 64 on a CU's 512 per SIMD lane), nothing spilled, no scratch, no static LDS beside the
    launch's dynamic image."""
    seen = {k: 0 for k in LOADER_FORMS}
    for k in re.split(r"\n\s+- \.agpr_count", stem_asm)[1:]:
        name = re.search(r"\.name:\s+(\S+)", k).group(1)
        g = lambda f: int(re.search(r"\.%s:\s+(\d+)" % f, k).group(1))
        for form, tag in LOADER_FORMS.items():
            if "conv_stem_pt_kernel" in name and tag in name:
                seen[form] += 1
                assert g("vgpr_count") <= 128, (form, name, g("vgpr_count"))
                assert g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0 and g("private_segment_fixed_size") == 0, (form, name)
                assert g("group_segment_fixed_size") == 0 and g("max_flat_workgroup_size") == 1024, (form, name)
    assert seen == {"uniform": 2, "per-lane": 2}, seen


def test_uniform_loader_issues_plain_buffer_loads(stem_asm):
    """The uniform deal's kernels fetch the clip with buffer loads whose descriptors are scalar (no waterfall loop: no v_readfirstlane feeds a descriptor);
    every issue point holds eight loads per region."""
    starts = [(m.start(), m.group(1)) for m in re.finditer(r"\n(_Z\S*conv_stem_pt_kernel\S*):", stem_asm)]
    found = 0
    for i, (pos, name) in enumerate(starts):
        if LOADER_FORMS["uniform"] not in name:
            continue
        found += 1
        body = stem_asm[pos:starts[i + 1][0] if i + 1 < len(starts) else stem_asm.index(".amdgpu_metadata")]
        loads = re.findall(r"buffer_load_dwordx4 v\[\d+:\d+\], v\d+, s\[\d+:\d+\], 0 offen", body)
        assert loads and len(loads) % 8 == 0 and len(loads) == body.count("buffer_load_dwordx4"), (name, len(loads))
        assert "v_readfirstlane_b32" not in body[body.index("buffer_load_dwordx4"):body.rindex("buffer_load_dwordx4")], name
    assert found == 2


def test_stem_lds_image_is_160_kb():
    """Halo regions (27 + 24 wave-instructions of 1 KB) + the tap-pair weight image + the column-pooled rows [8][9][64] 16-bit = the CU's 160 KB."""
    from ted_spad_amd import _lib
    assert (27 + 24) * 1024 + _lib.lib().tedspad_stem_pt_wimg16_bytes() + 8 * 9 * 128 == 160 * 1024
