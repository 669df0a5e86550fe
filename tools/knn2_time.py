"""Times the pair mode's score kernel for k = 1 (match_features / match_stored_batch) or k = 2 (match_features_ratio /
match_stored_batch_ratio) on the same inputs: one 2000 x 2000 call (latency shape) and one batch of 17 pairs of 2000-row
stored frames (68 M distances, throughput shape).  Per case: 3 warm-up calls, then the median, minimum and maximum of
lcm_last_launch_info().kernel_ms (device events around the score kernel) and of the call's wall time over 20 calls.

The k = 2 surcharge is the ratio between a run of this library with --k 2 and a run of the PARENT commit's library with
--k 1 (build it separately and select it with LCM_LIB_PATH); run the two alternately on an otherwise idle card:

    LCM_LIB_PATH=/path/to/parent/liblcm_hip.so python tools/knn2_time.py --k 1
    python tools/knn2_time.py --k 2
"""
import argparse
import ctypes
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
    return {"kernel_ms_median": statistics.median(kernel), "kernel_ms_min": min(kernel), "kernel_ms_max": max(kernel),
            "wall_ms_median": statistics.median(wall), "wall_ms_min": min(wall), "workgroups": info().workgroups,
            "distances": info().distances}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, choices=(1, 2), required=True)
    ap.add_argument("--ratio", type=float, default=0.75)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    pkg = entry.load_package()
    if args.k == 1:
        # a library built from the parent commit has no k = 2 entry points: bind only what it exports
        exported = ctypes.CDLL(pkg.capi.LIB_PATH)
        for name in [n for n in pkg.capi._SIGNATURES if not hasattr(exported, n)]:
            del pkg.capi._SIGNATURES[name]
    fs = pkg.synth.make_frames(8, 2000, seed=31, dup_frac=0.5)
    q, t = fs.frame(5), fs.frame(1)
    distinct = [(5, 1), (1, 5), (6, 2), (2, 6)]
    pairs = [distinct[i % 4] for i in range(17)]
    with pkg.Matcher() as m:
        for f in range(fs.n_frames):
            m.append(int(fs.ids[f]), fs.frame(f))
        if args.k == 1:
            single, batch = (lambda: m.match_features(q, t)), (lambda: m.match_stored_batch(pairs))
        else:
            single, batch = (lambda: m.match_features_ratio(q, t, args.ratio)), (lambda: m.match_stored_batch_ratio(pairs, args.ratio))
        out = {"k": args.k, "label": args.label, "library": pkg.capi.LIB_PATH, "calls": args.calls, "warmup": args.warmup,
               "pair_2000x2000": measure(single, m.launch_info, args.warmup, args.calls),
               "batch_17x2000x2000": measure(batch, m.launch_info, args.warmup, args.calls)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
