"""Code-object metadata of the SIFT / L2 pair-mode kernels (lcm_l2.hip; hipcc cross-compiles gfx950 without a GPU): no
scratch memory, no spills, at most 64 KB of LDS, and the VGPR budget the file's header claims: at most 128 (4 waves per
SIMD) for every kernel but the score kernel's two-tiles-per-wave shape, which gets 168 (3 waves per SIMD)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-loop-closing_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")
EXPECTED = ("k_l2_pack", "k_l2_scoreILi1E", "k_l2_scoreILi2E", "k_l2_fold", "k_l2_rescan")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_l2_kernels_use_no_scratch_and_fit_their_budget(tmp_path):
    out = tmp_path / "lcm_l2.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-x", "hip",
                           os.path.join(CSRC, "lcm_l2.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
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
        assert m["vgpr_count"] <= (168 if "k_l2_scoreILi2E" in name else 128), (name, m)
        assert m["group_segment_fixed_size"] <= 65536, (name, m)
        if "k_l2_pack" not in name:
            assert m["group_segment_fixed_size"] == 0, (name, m)
