"""csrc/lcm_sift_host.h and csrc/lcm_sift_device.h as a stand-alone program (tests/cpp/sift_host_check.cpp) under ASan + UBSan, on the
CPU: the extrema search and the refinement compiled from the device's own text replay planted stacks of tests/siftcases.py and must
equal tests/siftref.py bit for bit, candidates, reasons and records.  Nothing loaded into Python runs under a sanitizer."""
import os
import struct
import subprocess

import numpy as np
import pytest

import siftcases as S
import siftref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-loop-closing_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
HIP_INCLUDE = "/opt/rocm/include"          # lcm_sift_device.h includes hip_runtime.h: as plain C++ its markers expand to nothing


def pack_params(p):
    return struct.pack("<4d8i", p.contrast_threshold, p.edge_threshold, p.sigma, p.init_sigma, p.n_octave_layers, p.upsample, p.n_octaves,
                       p.border, p.max_steps, 0, 0, 0)


def replay_case(d, p, octave):
    """One case of the replay file: the parameters, the stack as octave `octave`, its candidates, their reasons, the records."""
    stack = [None] * octave + [d]
    cand = R.extrema([np.zeros((p.n_octave_layers + 2, 1, 1), np.float32)] * octave + [d], p)
    kp, why = R.refine(stack, cand, p)
    why = np.where(why == R.LEFT_LAYERS, R.LEFT, why).astype(np.int32)
    assert len(kp) == int(np.sum(why == R.OK)) and kp.dtype.itemsize == 32
    return (pack_params(p) + struct.pack("<4i", d.shape[2], d.shape[1], octave, len(cand)) + d.tobytes() + cand.tobytes() + why.tobytes() +
            struct.pack("<i", len(kp)) + kp.tobytes()), why


def write_replay(path):
    p = R.params()
    cases, seen = [], np.zeros(8, np.int64)
    walks, cand, why = S.refine_walks(p)
    S.assert_walks_cover(walks, cand, why, p)
    planted, sites = S.refine_planted(64, 24, p)
    S.assert_planted(planted, sites, p)
    for d, q, octave in ((walks, p, 0), (walks, R.params(max_steps=2, upsample=0), 3), (planted, p, 1), (planted, R.params(edge_threshold=1.0), 0),
                         (S.smooth_noise_stack(50, 37, R.params(n_octave_layers=5, border=2), seed=2), R.params(n_octave_layers=5, border=2), 2),
                         (S.extrema_plateau(23, 17, p)[0], p, 0), (S.extrema_values(70, 41, p)[0], p, 0)):
        blob, why = replay_case(d, q, octave)
        cases.append(blob)
        seen += np.bincount(why, minlength=8)
    assert all(seen[r] > 0 for r in (R.OK, R.ZERO_PIVOT, R.LEFT, R.NOT_CONVERGED, R.LOW_CONTRAST, R.EDGE)), seen
    img = np.zeros((9, 16), np.uint8)
    img[:, :13] = S.ramp_image(13, 9)
    big = R.upsample2(img[:, :13].astype(np.float32))
    with open(path, "wb") as f:
        f.write(struct.pack("<2i", 0x53494654, len(cases)) + b"".join(cases))
        f.write(struct.pack("<3i", 13, 9, 16) + img.tobytes() + big.astype(np.float32).tobytes())


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs clang++")
def test_host_compiled_arithmetic_equals_the_restatement_under_sanitizers(tmp_path):
    """Built as plain C++ (no HIP runtime is linked) with ASan + UBSan (no recovery) and run on the CPU: exit status 0, no report."""
    exe, replay = tmp_path / "sift_host_check", tmp_path / "sift_replay.bin"
    write_replay(replay)
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", HIP_INCLUDE, "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "sift_host_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), str(replay)], capture_output=True, text=True)
    assert r.returncode == 0 and "all held" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr)
    assert r.stdout.count("case ") == 7
