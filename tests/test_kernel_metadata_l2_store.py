"""Code-object metadata of the SIFT keyframe store's count kernels (lcm_l2_store.hip; hipcc cross-compiles gfx950 without a
GPU): exactly the kernels the file's header names, none with scratch memory, spills or LDS, k_l2_count_store<1> within 128
VGPRs (4 waves per SIMD) and k_l2_count_store<2> within 168 (3 waves per SIMD): the budgets of k_l2_count, whose body
they share."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-loop-closing_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")
EXPECTED = ("k_l2_count_storeILi1E", "k_l2_count_storeILi2E")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_l2_store_kernels_use_no_scratch_no_lds_and_fit_their_budget(tmp_path):
    out = tmp_path / "lcm_l2_store.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-x", "hip",
                           os.path.join(CSRC, "lcm_l2_store.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    ks = {}
    for block in re.split(r"\n  - \.a", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        ks[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1)) for k in FIELDS}
    for want in EXPECTED:
        assert sum(want in n for n in ks) == 1, (want, sorted(ks))
    assert len(ks) == len(EXPECTED), sorted(ks)
    for name, m in ks.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= (168 if "ILi2E" in name else 128), (name, m)
    # the matrix-core instruction of the shared body, and the verdict's double multiply left uncontracted
    assert "v_mfma_i32_32x32x32_i8" in text and "v_mul_f64" in text


def test_the_count_body_exists_once():
    """k_l2_count and k_l2_count_store call one device function: neither file holds a tile loop of its own."""
    for f in ("lcm_l2_count.hip", "lcm_l2_store.hip"):
        src = open(os.path.join(CSRC, f)).read()
        assert "l2_count_item<QT>(" in src and "__builtin_amdgcn_mfma" not in src and "l2_ratio_pass(D1" not in src, f
    assert open(os.path.join(CSRC, "lcm_l2_count_device.h")).read().count("__builtin_amdgcn_mfma_i32_32x32x32_i8(") == 1
