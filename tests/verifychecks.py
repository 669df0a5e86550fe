"""Comparisons shared by the GPU tests of the loop verification (tests/test_gpu_epi.py, test_gpu_pose.py,
test_gpu_verify_limits.py): the RANSAC's closure on the device's own hypotheses and the pose stage's comparison with poseref,
field by field and bit for bit."""
import numpy as np

import epiref as R
import epiref as E_
import poseref as P


def as_bytes(a):
    return np.ascontiguousarray(a).tobytes()


def check_closure(res, mask, pts, offs, hyps, pairs, threshold=1.0):
    """n_inliers, best_iter, E and every mask byte of the pairs against the numpy closure over the device's hypotheses."""
    for p in pairs:
        lo, hi = int(offs[p]), int(offs[p + 1])
        _, E = hyps[p]
        n_in, best, m = R.closure(E, pts[lo:hi], threshold)
        r = res[p]
        assert (r["n_points"], r["n_inliers"], r["best_iter"]) == (hi - lo, n_in, best), (p, r, n_in, best)
        assert r["status"] == (1 if hi - lo < 8 else 0)
        np.testing.assert_array_equal(mask[lo:hi], m, err_msg=str(p))
        assert int(mask[lo:hi].sum()) == r["n_inliers"]
        assert as_bytes(r["E"]) == as_bytes(E[best])


def check_against_reference(res, mask, pts, offs, E, mask_in, max_depth, k=E_.K):
    """Every field of every record and every mask byte against poseref."""
    want, want_mask = P.recover_pairs(E, pts, offs, mask_in, max_depth, k)
    for p, w in enumerate(want):
        r = res[p]
        got = (list(r["counts"]), r["choice"], r["n_good"], r["n_used"], r["status"])
        assert got == (list(w["counts"]), w["choice"], w["n_good"], w["n_used"], w["status"]), (p, got, w)
        assert as_bytes(r["R"]) == as_bytes(w["R"]) and as_bytes(r["t"]) == as_bytes(w["t"]), (p, r["R"] - w["R"], r["t"] - w["t"])
    np.testing.assert_array_equal(mask, want_mask)
