"""Code-object metadata of the ratio-test score kernel (lcm_ratio.hip; hipcc cross-compiles gfx950 without a GPU): every
workgroup shape of k_ratio_rowlane uses no scratch memory, spills nothing and stays within 96 VGPRs (5 waves per SIMD)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-loop-closing_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_ratio_kernel_uses_no_scratch_and_fits_96_vgprs(tmp_path):
    out = tmp_path / "lcm_ratio.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-x", "hip",
                           os.path.join(CSRC, "lcm_ratio.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    ks = {}
    for block in re.split(r"\n  - \.a", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        ks[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1)) for k in FIELDS}
    # 64 / 128 / 192 / 256 threads of 8 rows per lane
    assert sum("k_ratio_rowlane" in n for n in ks) == 4, sorted(ks)
    for name, m in ks.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 96, (name, m)
        assert m["group_segment_fixed_size"] <= 1024, (name, m)
