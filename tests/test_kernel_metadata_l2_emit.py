"""Code-object metadata of the device-side ratio test, compaction and keypoint gather (lcm_l2_emit.hip; hipcc cross-compiles
gfx950 without a GPU): exactly the kernels the file's header names, none with scratch memory or spills, each within 128
VGPRs, and no more LDS than the header states (16 bytes: the four waves' counts; none in k_l2_emit_offsets)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-loop-closing_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")
LDS = {"15k_l2_emit_countE": 16, "17k_l2_emit_offsetsE": 0, "9k_l2_emitE": 16}      # mangled name fragment -> bytes


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_l2_emit_kernels_use_no_scratch_and_fit_their_budget(tmp_path):
    out = tmp_path / "lcm_l2_emit.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-x", "hip",
                           os.path.join(CSRC, "lcm_l2_emit.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    ks = {}
    for block in re.split(r"\n  - \.a", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        ks[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1)) for k in FIELDS}
    for want in LDS:
        assert sum(want in n for n in ks) == 1, (want, sorted(ks))
    assert len(ks) == len(LDS), sorted(ks)
    for name, m in ks.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 128, (name, m)
        assert m["group_segment_fixed_size"] <= next(v for k, v in LDS.items() if k in name), (name, m)


def test_the_header_names_the_kernels_and_the_verdict_exists_once():
    src = open(os.path.join(CSRC, "lcm_l2_emit.hip")).read()
    head = src[: src.index("#include")]
    defined = re.findall(r"__global__[^\n]*\bvoid\s+(\w+)\s*\(", src)
    assert sorted(defined) == ["k_l2_emit", "k_l2_emit_count", "k_l2_emit_offsets"]
    for k in defined:
        assert re.search(rf"^// {k}\s", head, flags=re.M), k
    # one verdict: the shared header's, called from one place; no root or comparison of this file's own
    assert src.count("l2_ratio_pass(") == 1 and "sqrt(" not in src
    assert open(os.path.join(CSRC, "lcm_l2_count_device.h")).read().count("bool l2_ratio_pass(") == 1
