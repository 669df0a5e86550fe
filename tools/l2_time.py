"""Times the pair mode on SIFT rows (128 uint8, L2; lcm_l2.hip): one 4000 x 4000 lcm_match_features_ratio_l2 call (the
reference's cv::SIFT::create(4000) frame size) and one lcm_match_pairs_ratio_l2 call over 64 frames x 4000 rows, all pairs
with curr - past >= 32 (528 pairs, 8.4 G distances).  Per case: warm-up calls, then the median, minimum and maximum of
lcm_last_launch_info().kernel_ms (device events around the score kernel) and of the call's wall time, and distances/s from
the median kernel time.  Each case runs in both work-item shapes (LCM_TUNE_L2_CHUNK = 128: one query tile per wave, 256:
two) and in the shape the library picks on its own.

    python tools/l2_time.py            # prints one JSON line
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as entry  # noqa: E402


def measure(call, info, warmup, calls):
    for _ in range(warmup):
        call()
    kernel, wall = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        kernel.append(info().kernel_ms)
    med = statistics.median(kernel)
    return {"kernel_ms_median": med, "kernel_ms_min": min(kernel), "kernel_ms_max": max(kernel),
            "wall_ms_median": statistics.median(wall), "wall_ms_min": min(wall), "workgroups": info().workgroups,
            "distances": info().distances, "distances_per_s": info().distances / (med * 1e-3) if med > 0 else 0.0}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ratio", type=float, default=0.7)
    ap.add_argument("--rows", type=int, default=4000)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--gap", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--batch-calls", type=int, default=3)
    args = ap.parse_args()

    import numpy as np
    pkg = entry.load_package()
    rng = np.random.default_rng(31)
    frames = [rng.integers(0, 256, (args.rows, 128), dtype=np.uint8) for _ in range(args.frames)]
    for f in range(1, args.frames):                      # half of every frame's rows are near copies of the previous frame's
        n = args.rows // 2
        frames[f][:n] = np.clip(frames[f - 1][:n].astype(np.int16) + rng.integers(-20, 21, (n, 128)), 0, 255).astype(np.uint8)
    pairs = [(c, p) for c in range(args.frames) for p in range(args.frames) if c - p >= args.gap]
    out = {"library": pkg.capi.LIB_PATH, "rows": args.rows, "frames": args.frames, "pairs": len(pairs), "ratio": args.ratio}
    with pkg.Matcher() as m:
        single = lambda: m.match_features_ratio_l2(frames[1], frames[0], args.ratio)
        batch = lambda: m.match_pairs_ratio_l2(frames, pairs, args.ratio)
        out["matches_single"] = int(len(single()))
        for chunk in ("auto", "128", "256"):
            if chunk == "auto":
                os.environ.pop("LCM_TUNE_L2_CHUNK", None)
            else:
                os.environ["LCM_TUNE_L2_CHUNK"] = chunk
            out[f"pair_{args.rows}x{args.rows}_chunk_{chunk}"] = measure(single, m.launch_info, args.warmup, args.calls)
            out[f"batch_{len(pairs)}_pairs_chunk_{chunk}"] = measure(batch, m.launch_info, 1, args.batch_calls)
        os.environ.pop("LCM_TUNE_L2_CHUNK", None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
