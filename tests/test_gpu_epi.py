"""The essential-matrix RANSAC on the device (include/lcm.h lcm_epi_*; lcm_epi.hip, lcm_epi.cpp, lcm_l2_db.cpp) against
tests/epiref.py.  Needs a real MI355X.

The sampler and the scoring are compared exactly: integers there, and the header's arithmetic (double, every product and sum
rounded on its own) is numpy's.  The solver differs from the reference's (elimination + Jacobi against two SVDs) and is held
to the tolerances of DESIGN 9h.  The loop is closed on the device's OWN hypotheses: they are read back through
lcm_epi_hypotheses and scored in numpy, and count, winning hypothesis and every mask byte must equal what the calls report."""
import ctypes as C

import numpy as np
import pytest

import epicases as S
import epiref as R
from verifychecks import check_closure

pytestmark = pytest.mark.gpu

# the worst deviation of epiref's float64 solver (numpy SVD) over the 256 hypotheses of the noise-free scene,
# seed 0, pair 0, times the margin of 16 for the device's different elimination order.
#   singular values: max |s - (1, 1, 0)| = 1.554e-15 over all 256 hypotheses
#   truth:           max Frobenius distance to the true E (both at norm sqrt 2, up to sign) = 5.224e-4 over the 23 hypotheses
#                    whose eight samples are all planted inliers (the coordinates are rounded to float32)
SV_TOL = 16 * 1.554e-15
TRUTH_TOL = 16 * 5.224e-4
FILL = 0xA7


def params(pkg, **over):
    return pkg.capi.default_epi_params(R.FX, R.FY, R.CX, R.CY, **over)


def as_bytes(a):
    return np.ascontiguousarray(a).tobytes()


# ---- 1. the sampler, exact -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (8, 9, 63, 64, 65, 257))
def test_sampler_parity(pkg, matcher, n):
    pts = np.ascontiguousarray(S.scene("s1025")[0][:n])
    for iters in (64, 128):
        for seed in (0, 0xFFFFFFFF):
            for pair in (0, 70000):
                got, E = matcher.epi_hypotheses(pts, pair, params(pkg, iters=iters, seed=seed))
                assert got.shape == (iters, 8) and E.shape == (iters, 9)
                np.testing.assert_array_equal(got, R.samples(seed, pair, iters, n), err_msg=str((n, iters, seed, pair)))


def test_fewer_than_eight_points_have_no_hypotheses(pkg, matcher):
    for n in (0, 1, 7):
        s, E = matcher.epi_hypotheses(S.scene("s1025")[0][:n], 3, params(pkg, iters=64))
        assert (s == -1).all() and (E == 0).all()


# ---- 2. the scoring, exact -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 63, 64, 65, 1025))
def test_scoring_parity(pkg, matcher, n):
    # the integer-coordinate cases under K = (1, 1, 0, 0), with the all-zero matrix
    E_int, pts_int = S.integer_cases()
    unit = pkg.capi.default_epi_params(*S.K_UNIT)
    models = np.stack([E_int, np.zeros(9), -E_int, 2.0 * E_int])
    got = matcher.epi_score_models(pts_int[:n], models, unit)
    same = int((pts_int[:n, 1] == pts_int[:n, 3]).sum())
    np.testing.assert_array_equal(got, [same, 0, same, same])
    np.testing.assert_array_equal(got, R.counts(models, pts_int[:n], 1.0, S.K_UNIT))
    # 130 matrices over a scene's points, K = (700, 700, 320, 240), at 1 px and at 0.25 px
    pts = S.scene("s1025")[0][:n]
    models = np.concatenate([S.model_set(np.random.default_rng(n))[:129], np.zeros((1, 9))])       # 130: the call pads to 192
    for thr in (1.0, 0.25):
        got = matcher.epi_score_models(pts, models, params(pkg, threshold=thr))
        want = R.counts(models, pts, thr)
        np.testing.assert_array_equal(got, want)
        assert got[-1] == 0                                                                      # the all-zero matrix
    if n >= 64:
        assert len(set(want.tolist())) > 10 and want.max() > 0.6 * n                             # the counts do spread


@pytest.fixture(scope="module")
def verified(pkg, matcher):
    """The seven-pair call of test 4 (seed 0), once: results, mask, and the device's own hypotheses of every pair."""
    pts, offs, scenes = S.verify_call()
    ep = params(pkg)
    res, mask = matcher.epi_verify_pairs(pts, offs, ep)
    hyp = [matcher.epi_hypotheses(pts[int(offs[p]):int(offs[p + 1])], p, ep) for p in range(len(scenes))]
    return pts, offs, scenes, res.copy(), mask.copy(), hyp


def test_closure_on_the_devices_own_hypotheses(verified):
    pts, offs, scenes, res, mask, hyp = verified
    check_closure(res, mask, pts, offs, hyp, range(len(scenes)))
    eight = [nm for nm, _ in scenes].index("eight")
    cnt = R.counts(hyp[eight][1], pts[int(offs[eight]):int(offs[eight + 1])])
    assert (cnt == 8).all() and res[eight]["best_iter"] == 0 and res[eight]["n_inliers"] == 8      # first of equals


# ---- 3. the solver, with a tolerance ---------------------------------------------------------------------------------------
def test_solver_properties(pkg, matcher):
    pts, planted = S.scene(S.SOLVER_SCENE[0])
    s, E = matcher.epi_hypotheses(pts, 0, params(pkg, iters=S.SOLVER_ITERS))
    assert np.isfinite(E).all()
    zero = (E == 0).all(axis=1)
    assert zero.sum() < len(E) // 4
    assert R.singular_deviation(E[~zero]).max() <= SV_TOL                    # every non-zero E is on the manifold
    good = planted[s].all(axis=1)                                            # all eight samples planted inliers
    assert good.sum() >= 10 and not zero[good].any()
    assert R.truth_distance(E[good]).max() <= TRUTH_TOL


# ---- 4. end to end on host points -------------------------------------------------------------------------------------------
def test_verify_pairs_end_to_end(pkg, matcher, verified):
    pts, offs, scenes, res, mask, _ = verified
    ep = params(pkg)
    loop = {}
    for p, (name, planted) in enumerate(scenes):
        lo, hi = int(offs[p]), int(offs[p + 1])
        r = res[p]
        assert r["n_points"] == hi - lo
        loop[name] = pkg.capi.epi_loop_test(r, ep)
        if hi - lo < 8:
            assert r["status"] == pkg.capi.EPI_TOO_FEW and r["n_inliers"] == 0 and not r["E"].any() and not mask[lo:hi].any()
            continue
        assert r["status"] == pkg.capi.EPI_OK
        assert r["n_inliers"] >= planted.sum() and mask[lo:hi][planted].all(), (name, r["n_inliers"], planted.sum())
        assert R.singular_deviation(r["E"][None])[0] <= SV_TOL
    assert loop == {"s400_280": True, "out400": False, "empty": False, "seven": False, "eight": False, "s65": False, "s1025": True}
    assert res[1]["n_inliers"] <= 200
    # 230 of 400 (0.575): more than min_inliers, refused on the ratio alone
    p230, planted = S.scene(S.RATIO_SCENE[0])
    r230, m230 = matcher.epi_verify_pairs(p230, [0, 400], ep)
    assert r230[0]["n_inliers"] >= 230 and m230[planted].all()
    assert r230[0]["n_inliers"] > ep.min_inliers and r230[0]["n_inliers"] / 400 <= ep.min_ratio and not pkg.capi.epi_loop_test(r230[0], ep)
    # the same call again; the same pairs in two calls at the same positions: no dependence on time or neighbours
    res2, mask2 = matcher.epi_verify_pairs(pts, offs, ep)
    assert as_bytes(res2) == as_bytes(res) and as_bytes(mask2) == as_bytes(mask)
    ra, ma = matcher.epi_verify_pairs(pts[: int(offs[4])], offs[:5], ep)
    tail = np.concatenate([np.zeros(4, np.uintp), offs[4:] - offs[4]])
    rb, mb = matcher.epi_verify_pairs(pts[int(offs[4]):], tail, ep)
    assert as_bytes(ra) == as_bytes(res[:4]) and as_bytes(ma) == as_bytes(mask[: int(offs[4])])
    assert as_bytes(rb[4:]) == as_bytes(res[4:]) and as_bytes(mb) == as_bytes(mask[int(offs[4]):])
    assert (rb[:4]["status"] == pkg.capi.EPI_TOO_FEW).all() and not rb[:4]["n_points"].any()
    # another seed: other hypotheses, the same verdicts
    ep2 = params(pkg, seed=S.SEEDS[1])
    res3, mask3 = matcher.epi_verify_pairs(pts, offs, ep2)
    assert [pkg.capi.epi_loop_test(r, ep2) for r in res3] == [loop[nm] for nm, _ in scenes]
    assert as_bytes(res3) != as_bytes(res)
    for p, (name, planted) in enumerate(scenes):
        if len(planted) >= 8:
            assert res3[p]["n_inliers"] >= planted.sum() and mask3[int(offs[p]):int(offs[p + 1])][planted].all()
    # mask == NULL is allowed; the launch record is the three kernels'
    res4, none = matcher.epi_verify_pairs(pts, offs, ep, want_mask=False)
    assert none is None and as_bytes(res4) == as_bytes(res)
    info = matcher.launch_info()
    assert info.launches == 3 and info.pairs == len(scenes) and info.kernel_ms > 0 and info.route == 0


def test_refusals_with_a_handle_write_nothing(pkg, matcher):
    lib = pkg.load_library()
    pts = np.zeros((16, 4), np.float32)
    offs = np.array([0, 16], np.uintp)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    bad = [pkg.capi.default_epi_params(), params(pkg, iters=100), params(pkg, iters=0), params(pkg, threshold=float("nan")),
           pkg.capi.default_epi_params(700.0, -1.0, 320.0, 240.0)]
    for ep in bad + [None]:
        epp = None if ep is None else C.byref(ep)
        res, mask, smp, E, cnt = (np.full(k, FILL, np.uint8) for k in (88, 16, 65536 * 8 * 4 // 64, 4608, 256))
        assert lib.lcm_epi_verify_pairs(matcher._h, vp(pts), vp(offs), 1, epp, vp(res), vp(mask)) == -1
        assert lib.lcm_epi_hypotheses(matcher._h, vp(pts), 16, 0, epp, vp(smp), vp(E)) == -1
        assert lib.lcm_epi_score_models(matcher._h, vp(pts), 16, vp(np.zeros((64, 9))), 64, epp, vp(cnt)) == -1
        for a in (res, mask, smp, E, cnt):
            assert (a == FILL).all()
    ok = params(pkg, iters=64)
    res, mask = np.full(88, FILL, np.uint8), np.full(16, FILL, np.uint8)
    assert lib.lcm_epi_verify_pairs(matcher._h, vp(pts), None, 1, C.byref(ok), vp(res), vp(mask)) == -1            # NULL offsets
    assert lib.lcm_epi_verify_pairs(matcher._h, None, vp(offs), 1, C.byref(ok), vp(res), vp(mask)) == -1           # NULL points
    assert lib.lcm_epi_verify_pairs(matcher._h, vp(pts), vp(offs), 1, C.byref(ok), None, vp(mask)) == -1           # NULL results
    assert lib.lcm_epi_verify_pairs(matcher._h, vp(pts), vp(np.array([0, 65536], np.uintp)), 1, C.byref(ok), vp(res), vp(mask)) == -4
    assert lib.lcm_epi_verify_pairs(matcher._h, vp(pts), vp(np.array([16, 0], np.uintp)), 1, C.byref(ok), vp(res), vp(mask)) == -1
    assert lib.lcm_epi_score_models(matcher._h, vp(pts), 16, vp(np.zeros((64, 9))), 0, C.byref(ok), vp(mask)) == -1
    assert (res == FILL).all() and (mask == FILL).all()


# ---- 5. the store's forms -------------------------------------------------------------------------------------------------
CURR = 4
PASTS = ((500, 420), (520, 330), (300, 100), (400, 310))          # (rows, rows shared with the current frame)


@pytest.fixture(scope="module")
def loop_store(pkg):
    """A matcher of its own with four past frames and a current one (slot 4).  A past frame shares rows (exact copies: the only
    survivors of the ratio test among uniformly random rows) with the current one; the shared rows' keypoints are the two sides
    of a scene's correspondences, 400 true and 120 planted false ones over the current frame's 520 rows."""
    rng = np.random.default_rng(77)
    pts, planted = R.make_scene(400, 120, 21)
    curr = rng.integers(0, 256, (520, 128), dtype=np.uint8)
    frames, kps, shared = [], [], []
    for rows, n_shared in PASTS:
        f = rng.integers(0, 256, (rows, 128), dtype=np.uint8)
        kp = rng.uniform(0.0, 480.0, (rows, 2)).astype(np.float32)
        qi = np.sort(rng.choice(520, n_shared, replace=False))
        ti = rng.choice(rows, n_shared, replace=False)
        f[ti], kp[ti] = curr[qi], pts[qi, 2:]
        frames.append(f), kps.append(kp), shared.append((qi, ti))
    frames.append(curr), kps.append(np.ascontiguousarray(pts[:, :2]))
    m = pkg.Matcher()
    for k, (f, kp) in enumerate(zip(frames, kps)):
        assert m.l2_db_append_kp(f, kp) == k
    yield m, frames, kps, shared, planted
    m.close()


def test_store_verify_pairs(pkg, loop_store):
    m, frames, kps, shared, planted = loop_store
    ep = params(pkg)
    pairs = [(CURR, 0), (CURR, 2), (CURR, 1), (CURR, 3)]
    rng = np.random.default_rng(3)
    hq, ht = rng.integers(0, 256, (70, 32), dtype=np.uint8), rng.integers(0, 256, (90, 32), dtype=np.uint8)
    ham = m.match_pair(hq, ht)
    out0, pts0, offs0 = m.l2_db_match_points(pairs, 0.7)
    info0 = m.launch_info()
    for k, (_, past) in enumerate(pairs):                        # the survivors are the shared rows, with the scene's points
        lo, hi = int(offs0[k]), int(offs0[k + 1])
        qi, ti = shared[past]
        np.testing.assert_array_equal(out0[lo:hi]["query_idx"], qi)
        np.testing.assert_array_equal(out0[lo:hi]["train_idx"], ti)
    res, out, pts, mask, offs = m.epi_db_verify_pairs(pairs, 0.7, ep)
    info = m.launch_info()
    np.testing.assert_array_equal(offs, offs0)
    assert as_bytes(out) == as_bytes(out0) and as_bytes(pts) == as_bytes(pts0)
    want_res, want_mask = m.epi_verify_pairs(pts0, offs0, ep)          # same positions, same seed, the returned points
    assert as_bytes(res) == as_bytes(want_res) and as_bytes(mask) == as_bytes(want_mask)
    for k, (_, past) in enumerate(pairs):
        true = planted[shared[past][0]]
        assert res[k]["n_inliers"] >= true.sum() and mask[int(offs[k]):int(offs[k + 1])][true].all()
        assert pkg.capi.epi_loop_test(res[k], ep) == (past != 2)
    # the launch record: the _points form's, plus the three kernels
    assert (info.workgroups, info.pairs, info.route, info.distances) == (info0.workgroups, info0.pairs, info0.route, info0.distances)
    assert info.launches == info0.launches + 3 and info.kernel_ms > 0 and info.aux_kernel_ms > 0
    # `cap` one too small: as lcm_l2_db_match_points, and nothing is written
    total = int(offs[-1])
    bufs = dict(out=np.full(total, FILL, np.uint8).repeat(16).view(pkg.capi.DMATCH_DTYPE),
                pts=np.full((total, 16), FILL, np.uint8).view(np.float32),
                results=np.full(len(pairs) * 88, FILL, np.uint8).view(pkg.capi.EPI_RESULT_DTYPE),
                mask=np.full(total, FILL, np.uint8))
    with pytest.raises(pkg.LcmError) as e:
        m.epi_db_verify_pairs(pairs, 0.7, ep, cap=total - 1, **bufs)
    assert e.value.code == -4 and int(m.last_offsets[len(pairs)]) == total
    for a in bufs.values():
        assert (a.view(np.uint8) == FILL).all()
    # bad parameters are refused before the store is touched
    with pytest.raises(pkg.LcmError) as e:
        m.epi_db_verify_pairs(pairs, 0.7, params(pkg, iters=96), **bufs)
    assert e.value.code == -1
    for a in bufs.values():
        assert (a.view(np.uint8) == FILL).all()
    # the calls around it return what they returned
    out1, pts1, offs1 = m.l2_db_match_points(pairs, 0.7)
    assert as_bytes(out1) == as_bytes(out0) and as_bytes(pts1) == as_bytes(pts0) and as_bytes(offs1) == as_bytes(offs0)
    info1 = m.launch_info()
    assert info1.launches == info0.launches
    ham1 = m.match_pair(hq, ht)
    assert as_bytes(ham1[0]) == as_bytes(ham[0]) and as_bytes(ham1[1]) == as_bytes(ham[1])


def test_store_detect_loops(pkg, loop_store):
    m, frames, kps, shared, planted = loop_store
    ep = params(pkg)
    cands0, np0, out0, pts0, offs0 = m.l2_db_detect_loops_points(CURR, 1)
    info0 = m.launch_info()
    assert [int(c) for c in cands0["matched_frame_id"]] == [0, 1, 3]           # 100 shared rows are below the gate of 300
    cands, npairs, res, out, pts, mask, offs = m.epi_db_detect_loops(CURR, 1, ep)
    info = m.launch_info()
    assert as_bytes(cands) == as_bytes(cands0) and npairs == np0
    assert as_bytes(out) == as_bytes(out0) and as_bytes(pts) == as_bytes(pts0) and as_bytes(offs) == as_bytes(offs0)
    want_res, want_mask = m.epi_verify_pairs(pts0, offs0, ep)
    assert as_bytes(res) == as_bytes(want_res) and as_bytes(mask) == as_bytes(want_mask)
    assert all(pkg.capi.epi_loop_test(r, ep) for r in res) and (res["status"] == 0).all()
    assert info.launches == info0.launches + 3 and info.aux_kernel_ms > 0
    assert (info.workgroups, info.pairs, info.route) == (info0.workgroups, info0.pairs, info0.route)
    # the host-query form: the current frame's rows and points standing for position 4
    m.l2_db_truncate(CURR)
    try:
        c2, _, r2, o2, p2, m2, f2 = m.epi_db_detect_loops(CURR, 1, ep, query=frames[CURR], query_pts=kps[CURR])
        assert as_bytes(c2) == as_bytes(cands) and as_bytes(r2) == as_bytes(res) and as_bytes(m2) == as_bytes(mask)
        assert as_bytes(o2) == as_bytes(out) and as_bytes(p2) == as_bytes(pts) and as_bytes(f2) == as_bytes(offs)
        # no candidate: nothing to verify, nothing launched for it
        c3, _, r3, o3, p3, m3, f3 = m.epi_db_detect_loops(CURR, 1, ep, query=frames[CURR][:250], query_pts=kps[CURR][:250])
        assert len(c3) == 0 and len(r3) == 0 and len(o3) == 0 and len(m3) == 0 and f3.tolist() == [0]
    finally:
        assert m.l2_db_append_kp(frames[CURR], kps[CURR]) == CURR
    again = m.l2_db_detect_loops_points(CURR, 1)
    assert as_bytes(again[0]) == as_bytes(cands0) and as_bytes(again[2]) == as_bytes(out0) and as_bytes(again[3]) == as_bytes(pts0)


# ---- 6. slicing -----------------------------------------------------------------------------------------------------------
def test_seventy_thousand_pairs_make_two_slices(pkg, matcher):
    """70 000 pairs of 8 to 12 records, 64 hypotheses each: more pairs than gridDim.y holds, so every launch is sliced.  Every
    pair's n_inliers and every mask byte are checked against numpy under the pair's reported E (count == mask sum == the
    rule's verdicts); 500 pairs spread over both slices get the full closure over their hypotheses read back."""
    P = 70000
    rng = np.random.default_rng(11)
    lens = rng.integers(8, 13, P)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uintp)
    total = int(offs[-1])
    pts, _ = R.make_scene(total - total // 5, total // 5, 12)
    ep = params(pkg, iters=64)
    res, mask = matcher.epi_verify_pairs(pts, offs, ep)
    info = matcher.launch_info()
    assert info.launches == 6 and info.pairs == P
    np.testing.assert_array_equal(res["n_points"], lens)
    assert (res["status"] == 0).all() and (res["best_iter"] >= 0).all() and (res["best_iter"] < 64).all()
    pair_of = np.repeat(np.arange(P), lens)
    a, b, c, d = R.normalise(pts)
    want = R.inliers_each(res["E"][pair_of], a, b, c, d, R.threshold2()).astype(np.uint8)
    np.testing.assert_array_equal(mask, want)
    np.testing.assert_array_equal(res["n_inliers"], np.add.reduceat(want.astype(np.int64), offs[:-1].astype(np.int64)))
    assert (res["n_inliers"] >= 8).mean() > 0.25 and (res["n_inliers"][-100:] >= 8).any()
    sample = np.unique(np.concatenate([[0, 1, 65534, 65535, 65536, P - 1], rng.choice(P, 494, replace=False)]))
    hyps = {int(p): matcher.epi_hypotheses(pts[int(offs[p]):int(offs[p + 1])], int(p), ep) for p in sample}
    check_closure(res, mask, pts, offs, hyps, [int(p) for p in sample])
