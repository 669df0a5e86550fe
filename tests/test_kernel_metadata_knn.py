"""Code-object metadata of the k = 2 pair-mode kernels (lcm_knn.hip; hipcc cross-compiles gfx950 without a GPU): no
scratch memory, no spills, at most 128 VGPRs (4 waves per SIMD at the least) and 64 KB of LDS."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-loop-closing_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_knn_kernels_use_no_scratch_and_fit_their_budget(tmp_path):
    out = tmp_path / "lcm_knn.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-x", "hip",
                           os.path.join(CSRC, "lcm_knn.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    ks = {}
    for block in re.split(r"\n  - \.a", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        ks[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1)) for k in FIELDS}
    # the score kernel in its latency shape (2 rows per lane) and its throughput shapes (8 rows per lane), and the fold
    assert sum("k_knn2_rowlane" in n for n in ks) >= 2 and any("k_fold_pair_keys2" in n for n in ks), sorted(ks)
    for name, m in ks.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 128, (name, m)
        assert m["group_segment_fixed_size"] <= 65536, (name, m)
