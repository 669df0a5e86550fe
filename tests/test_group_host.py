"""The group's sharding arithmetic without a device (csrc/lcm_group_host.h): eligible frames, a shard's share, the record
layout of a search, the shard geometry, the rank-major query slot and the three host merges, as a stand-alone program under
ASan + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-loop-closing_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_sharding_arithmetic_runs_clean_under_sanitizers(tmp_path):
    """tests/cpp/group_host_check.cpp enumerates every (query position, stored position) pair by brute force — owner =
    stored position mod W, a shard's order = (query, stored) ascending — and checks against it: eligible_count, shard_share,
    the layout with 32-bit and size_t offsets (merged offsets, per-shard offsets, shard_base, total), shard_geometry,
    q_frame_of through a rank-major buffer, the host merge, the online interleave and the candidate merge.  W = 1, 2, 3, 5, 8;
    N = 0, 1, W - 1, W, W + 1, 57; gaps 0, 1, 3, 30; id steps 1 and 3 (some shards own nothing in several of these: asserted);
    empty candidate lists, one list holding everything, equal current ids across shards.  The 2^32 boundary: 92682 frames =
    4 294 930 221 pairs accepted, 92683 refused with the library's message (and accepted with size_t offsets).  Built as plain
    C++ (no HIP runtime is linked) with ASan + UBSan (no recovery) and run on the CPU: exit status 0 and no report."""
    exe = tmp_path / "group_host_check"
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "group_host_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "all held" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr)
