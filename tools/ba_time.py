"""Times the alternating bundle adjustment on the device (lcm_ba_optimize; lcm_ba.hip), in one process and one run.

Scenes: --cams cameras on a ring of radius 4 looking at a cloud of --points points in [-1, 1]^3 (numpy default_rng(47)), every
point seen by --per-point consecutive cameras, pixels with 0.5 px of noise, poses and points moved off the truth (0.004 rad,
0.02 units).  The observation list is shuffled.  Two sizes: the reference's scale and a large one.

  optimize   lcm_ba_optimize per size, outer_iters = inner_iters = 5: kernel_ms (all 2 + 4 x 5 launches between the call's two
             events) and wall time (staging, the host's two counting sorts and the download included), under the default
             min_update and with every iteration forced (min_update = 0); one camera phase, one point phase and one mean error
             beside it.
  numpy      at the first size: tests/baref.py's optimize (route A), the same run on the host, once.

Warm-up calls, then --calls timed calls; median (min - max).

    python tools/ba_time.py           # writes profiles/ba_time.txt and prints it
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as entry  # noqa: E402
from epi_time import mmm  # noqa: E402

K = (1000.0, 1000.0, 640.0, 360.0)


def scene(np, rng, n_cams, n_points, per_point):
    """(R, t, X, cam, pt, uv): the poses and points moved off the truth, the shuffled observation list."""
    import pgoref as G
    a = 2 * np.pi * (np.arange(n_cams) + 0.3 * rng.random(n_cams)) / n_cams
    C = np.stack([4 * np.cos(a), 4 * np.sin(a), 0.4 * rng.standard_normal(n_cams)], 1)
    z = -C / np.linalg.norm(C, axis=1, keepdims=True)
    x = np.cross(np.array([0.0, 0.0, 1.0]), z)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    Rt = np.stack([x, np.cross(z, x), z], 1)
    tt = -np.einsum("nij,nj->ni", Rt, C)
    Xt = rng.uniform(-1.0, 1.0, (n_points, 3))
    k = min(per_point, n_cams)
    cam = ((rng.integers(0, n_cams, n_points)[:, None] + np.arange(k)[None, :]) % n_cams).reshape(-1)
    pt = np.repeat(np.arange(n_points), k)
    order = rng.permutation(len(cam))
    cam, pt = cam[order], pt[order]
    Xc = np.einsum("nij,nj->ni", Rt[cam], Xt[pt]) + tt[cam]
    uv = np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], 1) + rng.uniform(-0.5, 0.5, (len(cam), 2))
    R = G.mm(G.exp(0.004 * rng.standard_normal((n_cams, 3))), Rt)
    return R, tt + 0.02 * rng.standard_normal((n_cams, 3)), Xt + 0.02 * rng.standard_normal((n_points, 3)), cam, pt, uv


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cams", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--points", type=int, nargs="+", default=[50000, 1000000])
    ap.add_argument("--per-point", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ba_time.txt"))
    args = ap.parse_args()

    import numpy as np
    import baref as B
    pkg = entry.load_package()
    c = pkg.capi
    rng = np.random.default_rng(47)
    lines = [f"ba_time: ring scenes, {args.per_point} observations a point, outer_iters = inner_iters = 5, {args.calls} timed calls after "
             f"{args.warmup} warm-up calls"]
    with pkg.Matcher() as m:
        for size, (n_cams, n_points) in enumerate(zip(args.cams, args.points)):
            R, t, X, cam, pt, uv = scene(np, rng, n_cams, n_points, args.per_point)
            poses, points, obs = c.pgo_poses(R, t), c.ba_points(X), c.ba_obs(cam, pt, uv)
            for label, over in (("default min_update", {}), ("min_update = 0", dict(min_update=0.0))):
                p = c.default_ba_params(fx=K[0], fy=K[1], cx=K[2], cy=K[3], **over)
                kernel, wall, cams, pts, err = [], [], [], [], []
                for k in range(args.warmup + args.calls):
                    t0 = time.perf_counter()
                    out = m.ba_optimize(poses, points, obs, p)
                    w = (time.perf_counter() - t0) * 1e3
                    i = m.launch_info()
                    m.ba_refine_cameras(poses, points, obs, p)
                    c_ms = m.launch_info().kernel_ms
                    m.ba_refine_points(poses, points, obs, p)
                    p_ms = m.launch_info().kernel_ms
                    m.ba_error(poses, points, obs, p)
                    e_ms = m.launch_info().kernel_ms
                    if k >= args.warmup:
                        kernel.append(i.kernel_ms), wall.append(w), cams.append(c_ms), pts.append(p_ms), err.append(e_ms)
                info = out[4]
                assert i.launches == 22 and i.pairs == len(obs)
                lines.append(f"optimize {n_cams:5d} cameras, {n_points:8d} points, {len(obs):8d} observations, {label}: kernel_ms {mmm(kernel)} | "
                             f"wall_ms {mmm(wall)} | one camera phase {mmm(cams)} | one point phase {mmm(pts)} | one mean error {mmm(err)} | "
                             f"mean error {info.mean_error[0]:.4g} -> {info.mean_error[5]:.4g} px | cameras per status {list(info.cameras)}, "
                             f"points {list(info.points)}")
            if size == 0:
                t0 = time.perf_counter()
                want, _, _, means = B.optimize(B.Map(K, R, t, X, cam, pt, uv), "a", min_update=0.0)
                lines.append(f"numpy    {n_cams:5d} cameras, {n_points:8d} points, min_update = 0: tests/baref.py optimize, once: "
                             f"{(time.perf_counter() - t0) * 1e3:.0f} ms of wall time | mean error {means[0]:.4g} -> {means[-1]:.4g} px | largest "
                             f"difference to the device's points {np.abs(c.ba_xyz(out[1]) - want.X).max():.3g}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
