"""Times the SIFT keypoint detector on the device (lcm_sift_space_build, lcm_sift_extrema, lcm_sift_detect; lcm_sift.hip), in one
process and one run.

Images: seeded noise, smoothed by a 3 x 3 box (tests/siftcases.py's noise_image), at 640 x 480 and 1920 x 1080; the defaults (the
first octave is the image enlarged 2x).

  build    lcm_sift_space_build: kernel_ms (every launch of the pyramid between the call's two events) and wall time (the upload of
           the image and the wait included); the bytes the stage has to move (the image once; per blur one layer read and two
           written; per next octave one layer read at a quarter and one written), the rate they give over kernel_ms and its share
           of the 8.0 TB/s of HBM; the sum of the layers' sizes beside it.
  extrema  lcm_sift_extrema: the count, scan and emit launches; bytes = the DoG layers once + the candidates.
  detect   lcm_sift_detect: extrema + refinement + compaction; wall time includes the two counts read back and the records' download.
  numpy    tests/siftref.py's detect on the same image, once (CPU); the records compared with the device's.

With --stats-csv the per-kernel table of a separate `rocprofv3 --kernel-trace --stats` run of this tool (--profile-run: warm-up and
--calls calls, nothing timed, no numpy) is added: kernel time per stage.

Warm-up calls, then --calls timed calls; median (min - max).

    python tools/sift_time.py          # writes profiles/sift_time.txt and prints it
"""
import argparse
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as entry  # noqa: E402
from epi_time import mmm  # noqa: E402

HBM_PEAK = 8.0e12
SIZES = ((640, 480), (1920, 1080))


def kernel_table(path):
    """kernel name -> (calls, total ns, average ns) of the k_sift_* and k_block_scan rows of a rocprofv3 kernel_stats.csv"""
    out = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            short = name.split("(")[0].split("::")[-1]
            if short.startswith("k_sift_") or short == "k_block_scan":
                out.append((short, int(row["Calls"]), float(row["TotalDurationNs"]), float(row["AverageNs"])))
    return sorted(out, key=lambda r: -r[2])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--stats-csv", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sift_time.txt"))
    args = ap.parse_args()

    import numpy as np
    import siftcases as S
    import siftref as R
    pkg = entry.load_package()
    p = R.params()
    lines = [f"sift_time: seeded smoothed noise, the defaults (3 layers an octave, first octave enlarged 2x), {args.calls} timed calls after "
             f"{args.warmup} warm-up calls; median (min - max); HBM peak taken as {HBM_PEAK / 1e12:.1f} TB/s"]
    with pkg.Matcher() as m:
        for w, h in SIZES:
            img = S.noise_image(w, h, seed=w)
            with m.sift_space(w, h) as space:
                info = space.info()
                room = int(info.candidate_capacity)                    # the callers' buffers, made once: the calls are timed, not numpy's zeros
                cand_out, kp_out = np.zeros(room, pkg.capi.SIFT_CANDIDATE_DTYPE), np.zeros(room, pkg.capi.SIFT_KEYPOINT_DTYPE)
                kernel = {"build": [], "extrema": [], "detect": []}
                wall = {"build": [], "extrema": [], "detect": []}
                moved = {}
                for k in range(args.warmup + args.calls):
                    for stage, call in (("build", lambda: space.build(img)), ("extrema", lambda: space.extrema(room, cand_out)),
                                        ("detect", lambda: space.detect(room, kp_out))):
                        t0 = time.perf_counter()
                        res = call()
                        t1 = time.perf_counter()
                        li = m.launch_info()
                        if k >= args.warmup:
                            kernel[stage].append(li.kernel_ms); wall[stage].append((t1 - t0) * 1e3)
                        moved[stage] = (li.algo_bytes, li.launches, li.workgroups)
                    kp, n_cand = res
                if args.profile_run:
                    continue
                pl = space.info().plan
                layer_bytes = 4 * (pl.space_floats - pl.base_w * pl.base_h)
                lines.append(f"{w} x {h}: {pl.n_octaves} octaves from {pl.base_w} x {pl.base_h}, {n_cand} candidates, {len(kp)} keypoints; the layers "
                             f"hold {layer_bytes / 1e6:.1f} MB ({pl.n_gauss} Gaussian + {pl.n_dog} DoG an octave), the space {info.device_bytes / 1e6:.1f} MB")
                for stage in ("build", "extrema", "detect"):
                    b, launches, groups = moved[stage]
                    med = sorted(kernel[stage])[len(kernel[stage]) // 2]
                    lines.append(f"  {stage:8s} kernel_ms {mmm(kernel[stage])}  wall_ms {mmm(wall[stage])}  {launches} launches, {groups} workgroups, "
                                 f"{b / 1e6:.1f} MB to move = {b / 1e9 / (med / 1e3):.0f} GB/s = {100.0 * b / (med / 1e3) / HBM_PEAK:.1f} % of HBM peak")
                t0 = time.perf_counter()
                want, cand, _ = R.detect(img, p)
                t1 = time.perf_counter()
                same = want.tobytes() == np.ascontiguousarray(kp).tobytes()
                lines.append(f"  numpy    tests/siftref.py detect, once: {(t1 - t0) * 1e3:.0f} ms on the CPU; its {len(want)} records "
                             f"{'equal' if same else 'DIFFER FROM'} the device's bit for bit")
    if args.profile_run:
        print("profile run done")
        return
    if args.stats_csv:
        lines.append(f"kernel time per stage, from a separate rocprofv3 --kernel-trace --stats run of the same calls ({args.warmup + args.calls} of "
                     f"each per size, both sizes together; k_block_scan serves both compactions): name, launches, total ms, average us")
        for name, calls, total, avg in kernel_table(args.stats_csv):
            lines.append(f"  {name:16s} {calls:6d} {total / 1e6:10.3f} {avg / 1e3:10.2f}")
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
