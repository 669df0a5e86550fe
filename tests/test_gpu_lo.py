"""The RANSAC's local optimisation on the device (include/lcm.h lcm_lo_*; lcm_lo.hip, lcm_lo.cpp, lcm_l2_db.cpp) against
tests/loref.py.  Needs a real MI355X.

The selection is integers and compared exactly.  One refit round is compared through the seam: the selected set and the status
are exact (the inlier rule is numpy's arithmetic and the models are the same bytes), the refitted matrix is held to 16 x
loref's own error.  The full optimisation is closed on the device's OWN output: the count and every mask byte are epiref's
rule applied to the returned E, the RANSAC's part is lcm_epi_verify_pairs's bytes, and the seeds are recomputed from counts
read back through the RANSAC's seams.  The value of the step is asserted on the noisy pairs whose reference verdict it turns."""
import ctypes as C

import numpy as np
import pytest

import epiref as R
import locases as S
import loref as L
import poseref as P

pytestmark = pytest.mark.gpu

# loref's own error: the worst disagreement of its two float64 routes (eigh of the moment matrix against the SVD of the rows)
# over every model of the one-round cases below, measured on the CPU (tests/test_lo_ref_host.py asserts it):
# 5.037e-10, at the nine-record case under multiplier 1.  Times the project's margin of 16 for the device's Jacobi.
OWN_ERROR = 5.1e-10
E_TOL = 16 * OWN_ERROR
SV_TOL = 16 * 1.554e-15                     # tests/test_gpu_epi.py's: the projection is the solver's
FILL = 0xA7


def params(pkg, **over):
    return pkg.capi.default_epi_params(R.FX, R.FY, R.CX, R.CY, **over)


def as_bytes(a):
    return np.ascontiguousarray(a).tobytes()


# ---- 1. the selection, exact ------------------------------------------------------------------------------------------------
def count_patterns(iters):
    rng = np.random.default_rng(iters)
    last = np.zeros(iters, np.int32)
    last[-1] = 7
    return {"equal": np.full(iters, 5, np.int32), "ascending": np.arange(iters, dtype=np.int32),
            "descending": (65535 - np.arange(iters)).astype(np.int32), "ties": rng.integers(0, 6, iters).astype(np.int32),
            "last": last}


@pytest.mark.parametrize("iters", (64, 128, 1024, 65536))
def test_selection_parity(matcher, iters):
    for name, cnt in count_patterns(iters).items():
        got = matcher.lo_select(cnt)
        np.testing.assert_array_equal(got, L.select(cnt), err_msg=name)
    assert matcher.lo_select(np.full(iters, 5, np.int32)).tolist() == list(range(64))               # the lowest hypotheses first
    assert matcher.lo_select(count_patterns(iters)["last"])[0] == iters - 1


# ---- 2. one round: the selected set exact, the matrix within tolerance --------------------------------------------------------
@pytest.mark.parametrize("n_models", S.REFIT_MODELS)
@pytest.mark.parametrize("n", sorted(S.REFIT_CASES))
def test_one_round_parity(pkg, matcher, n, n_models):
    pts = S.refit_points(n)
    models = S.refit_models()[:n_models]
    for mult in S.REFIT_MULTS:
        want_E, want_n, want_status, _ = S.refit_reference(n, mult)
        E, n_sel, status = matcher.lo_refit_models(pts, models, mult, params(pkg))
        np.testing.assert_array_equal(n_sel, want_n[:n_models], err_msg=str((n, mult)))
        np.testing.assert_array_equal(status, want_status[:n_models], err_msg=str((n, mult)))
        ok = status == L.OK
        assert not E[~ok].any()
        if ok.any():
            dist = L.sign_aligned_distance(E[ok], want_E[:n_models][ok])
            dev = R.singular_deviation(E[ok])
            print(f"n {n} models {n_models} mult {mult}: worst distance {dist.max():.3e} (limit {E_TOL:.3e}), singular values {dev.max():.3e}")
            assert dist.max() <= E_TOL, (n, mult, dist.max())
            assert dev.max() <= SV_TOL, (n, mult, dev.max())
        # 3. the moments are summed in a fixed order: the same call returns the same bytes
        E2, n2, s2 = matcher.lo_refit_models(pts, models, mult, params(pkg))
        assert as_bytes(E2) == as_bytes(E) and as_bytes(n2) == as_bytes(n_sel) and as_bytes(s2) == as_bytes(status)
    if n_models >= 63:
        assert status[62] == L.TOO_FEW and n_sel[62] == 0                                           # the all-zero model


def test_one_round_too_few_and_degenerate(pkg, matcher):
    ep = params(pkg)
    models = S.refit_models()
    seven = S.scene("seven")[0]
    E, n_sel, status = matcher.lo_refit_models(seven, models, 3.0, ep)
    assert (status == L.TOO_FEW).all() and (n_sel <= 7).all() and n_sel[0] == 7 and not E.any()
    E, n_sel, status = matcher.lo_refit_models(seven[:0], models[:1], 1.0, ep)
    assert status.tolist() == [L.TOO_FEW] and n_sel.tolist() == [0] and not E.any()
    same = S.scene(S.DEGENERATE)[0]
    a, b, c, d = R.normalise(same)
    fits = R.skew(np.array([a[0] - c[0], b[0] - d[0], 0.0])).reshape(9)                              # the record satisfies it
    E, n_sel, status = matcher.lo_refit_models(same, np.stack([fits, models[1], np.zeros(9)]), 1.0, ep)
    want = [L.refit(e, a, b, c, d, L.scaled_threshold(), 1.0) for e in (fits, models[1], np.zeros(9))]
    assert status.tolist() == [w[2] for w in want] and n_sel.tolist() == [w[1] for w in want]
    assert (status[0], n_sel[0], status[2], n_sel[2]) == (L.DEGENERATE, 40, L.TOO_FEW, 0) and not E.any()


# ---- 4. closure on the device's own output ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def optimised(pkg, matcher):
    """The fourteen-pair call at both sampler seeds, once: the RANSAC's records, the optimised ones, and per pair the 64 seeds
    recomputed in numpy from the device's own hypotheses' counts."""
    pts, offs = S.call()
    out = {}
    for seed in S.SEEDS:
        ep = params(pkg, seed=seed)
        res0, mask0 = matcher.epi_verify_pairs(pts, offs, ep)
        res, info, mask = matcher.lo_verify_pairs(pts, offs, ep)
        launch = matcher.launch_info()
        res2, info2, mask2 = matcher.lo_verify_pairs(pts, offs, ep)
        assert as_bytes(res2) == as_bytes(res) and as_bytes(info2) == as_bytes(info) and as_bytes(mask2) == as_bytes(mask)
        seeds = []
        for p in range(len(S.CALL)):
            pp = pts[int(offs[p]):int(offs[p + 1])]
            if len(pp) < 8:
                seeds.append(None)
                continue
            _, E = matcher.epi_hypotheses(pp, p, ep)
            seeds.append(L.select(matcher.epi_score_models(pp, E, ep)))
        out[seed] = (res0.copy(), mask0.copy(), res.copy(), info.copy(), mask.copy(), seeds, launch)
    return pts, offs, out


@pytest.mark.parametrize("seed", S.SEEDS)
def test_closure_on_the_devices_own_output(pkg, optimised, seed):
    pts, offs, out = optimised
    res0, mask0, res, info, mask, seeds, launch = out[seed]
    assert launch.launches == 5 and launch.pairs == len(S.CALL) and launch.kernel_ms > 0
    improved = 0
    for p, name in enumerate(S.CALL):
        lo, hi = int(offs[p]), int(offs[p + 1])
        n = hi - lo
        r, r0, i = res[p], res0[p], info[p]
        a, b, c, d = R.normalise(pts[lo:hi])
        want = (R.inliers(r["E"].reshape(1, 9), a, b, c, d, R.threshold2())[0] if n else np.zeros(0, bool)).astype(np.uint8)
        np.testing.assert_array_equal(mask[lo:hi], want, err_msg=name)
        assert r["n_inliers"] == int(want.sum()) and r["n_points"] == n and r["status"] == r0["status"] == (1 if n < 8 else 0)
        assert i["n_inliers_ransac"] == r0["n_inliers"] and r["n_inliers"] >= r0["n_inliers"]
        assert i["seed_iter"] == r["best_iter"]
        assert i["status"] == (L.TOO_FEW if n < 8 else L.DEGENERATE if name == S.DEGENERATE else L.OK), (name, i)
        if i["round"] == -1:
            assert as_bytes(r) == as_bytes(r0) and as_bytes(mask[lo:hi]) == as_bytes(mask0[lo:hi]), name
        else:
            improved += 1
            assert 0 <= i["round"] < 4 and r["n_inliers"] > r0["n_inliers"] and r["best_iter"] in seeds[p].tolist(), (name, i)
            assert R.singular_deviation(r["E"])[0] <= SV_TOL
        if seeds[p] is not None:
            assert seeds[p][0] == r0["best_iter"]
        if n < 8 or name == S.DEGENERATE:
            assert i["round"] == -1 and not r["E"].any() and r["n_inliers"] == 0
        print(f"seed {seed} {name}: RANSAC {r0['n_inliers']} -> {r['n_inliers']} round {i['round']} seed_iter {i['seed_iter']}")
    for nm, *_ in S.NOISY:                                             # where the restatement gains clearly, the device gains
        p = S.CALL.index(nm)
        r_ref, o_ref = S.reference(nm, seed, p)
        if o_ref["n_inliers"] - r_ref >= 10:
            assert info[p]["round"] >= 0 and res[p]["n_inliers"] - res0[p]["n_inliers"] >= 5, (nm, r_ref, o_ref["n_inliers"], res[p])
    assert improved >= 4
    for nm in ("s400_280", "eight", "s65"):                            # every record already an inlier or none to gain: kept
        assert info[S.CALL.index(nm)]["round"] == -1
    assert res[S.CALL.index("out400")]["n_inliers"] < 30


# ---- 5. the value -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.VALUE)
def test_the_optimisation_turns_the_verdict(pkg, matcher, name):
    pts = S.scene(name)[0]
    n = len(pts)
    offs = np.array([0, n], np.uintp)
    ep = params(pkg)
    r_ref, o_ref = S.reference(name)
    assert not R.loop_test(r_ref, n) and R.loop_test(o_ref["n_inliers"], n)                          # the pre-condition
    res0, mask0 = matcher.epi_verify_pairs(pts, offs, ep)
    res, info, mask = matcher.lo_verify_pairs(pts, offs, ep)
    d0, d1 = R.truth_distance(res0[0]["E"])[0], R.truth_distance(res[0]["E"])[0]
    pose0, _ = matcher.pose_recover_pairs(pts, offs, res0["E"], ep, None, mask0)
    pose1, _ = matcher.pose_recover_pairs(pts, offs, res["E"], ep, None, mask)
    e0 = P.motion_error(pose0[0]["R"].reshape(3, 3), pose0[0]["t"], R.R_TRUE, R.T_TRUE)
    e1 = P.motion_error(pose1[0]["R"].reshape(3, 3), pose1[0]["t"], R.R_TRUE, R.T_TRUE)
    print(f"{name}: inliers {res0[0]['n_inliers']} -> {res[0]['n_inliers']} of {n} (reference {r_ref} -> {o_ref['n_inliers']}), "
          f"|E - E_true| {d0:.4f} -> {d1:.4f}, motion error R {e0[0]:.2e} -> {e1[0]:.2e}, t {e0[1]:.2e} -> {e1[1]:.2e}")
    assert not pkg.capi.epi_loop_test(res0[0], ep) and pkg.capi.epi_loop_test(res[0], ep)
    assert info[0]["round"] >= 0 and info[0]["n_inliers_ransac"] == res0[0]["n_inliers"]
    assert d1 < d0
    assert pose1[0]["status"] == 0 and e1[0] < e0[0] and e1[1] < e0[1]


# ---- 6. the store's forms -----------------------------------------------------------------------------------------------------
CURR = 4
PASTS = ((500, 420), (520, 330), (300, 100), (400, 310))          # (rows, rows shared with the current frame)
SIGMA = 0.3


@pytest.fixture(scope="module")
def noisy_store(pkg):
    """tests/test_gpu_pose.py's loop_store with 0.3 px of Gaussian noise on the keypoints of the true correspondences: four
    past frames and a current one (slot 4) of 300 to 520 rows; a past frame shares rows with the current one, whose keypoints
    are the two sides of the correspondences (400 true, 120 planted false) of a two-view scene."""
    rng = np.random.default_rng(78)
    pts, planted = R.make_scene(400, 120, 22)
    p = pts.astype(np.float64)
    p[planted] += np.random.default_rng(1022).normal(0.0, SIGMA, (400, 4))
    pts = p.astype(np.float32)
    curr = rng.integers(0, 256, (520, 128), dtype=np.uint8)
    frames, kps = [], []
    for rows, n_shared in PASTS:
        f = rng.integers(0, 256, (rows, 128), dtype=np.uint8)
        kp = rng.uniform(0.0, 480.0, (rows, 2)).astype(np.float32)
        qi = np.sort(rng.choice(520, n_shared, replace=False))
        ti = rng.choice(rows, n_shared, replace=False)
        f[ti], kp[ti] = curr[qi], pts[qi, 2:]
        frames.append(f), kps.append(kp)
    frames.append(curr), kps.append(np.ascontiguousarray(pts[:, :2]))
    m = pkg.Matcher()
    for k, (f, kp) in enumerate(zip(frames, kps)):
        assert m.l2_db_append_kp(f, kp) == k
    yield m, frames, kps
    m.close()


def test_store_verify_pairs(pkg, noisy_store):
    m, frames, kps = noisy_store
    ep = params(pkg)
    pairs = [(CURR, 0), (CURR, 2), (CURR, 1), (CURR, 3)]
    out0, pts0, offs0 = m.l2_db_match_points(pairs, 0.7)
    _, _, *_rest = pose = m.pose_db_verify_pairs(pairs, 0.7, ep)
    info_pose = m.launch_info()
    res, info, pres, out, pts, mask, pmask, offs = m.lo_db_verify_pairs(pairs, 0.7, ep)
    launch = m.launch_info()
    # everything before the RANSAC, byte for byte; the composition of the three host-list calls after it
    assert as_bytes(offs) == as_bytes(offs0) and as_bytes(out) == as_bytes(out0) and as_bytes(pts) == as_bytes(pts0)
    want_res, want_info, want_mask = m.lo_verify_pairs(pts0, offs0, ep)
    assert as_bytes(res) == as_bytes(want_res) and as_bytes(info) == as_bytes(want_info) and as_bytes(mask) == as_bytes(want_mask)
    want_pose, want_pmask = m.pose_recover_pairs(pts0, offs0, res["E"], ep, None, mask)
    assert as_bytes(pres) == as_bytes(want_pose) and as_bytes(pmask) == as_bytes(want_pmask)
    assert (info["n_inliers_ransac"] == pose[0]["n_inliers"]).all() and (res["n_inliers"] >= pose[0]["n_inliers"]).all()
    assert (info["round"] >= 0).any()
    # the launch record: the pose form's, plus the two kernels
    assert launch.launches == info_pose.launches + 2 and launch.aux_kernel_ms > 0 and launch.kernel_ms > 0
    assert (launch.workgroups, launch.pairs, launch.route) == (info_pose.workgroups, info_pose.pairs, info_pose.route)
    # other rounds reach the kernel through the store's form too
    lp1 = pkg.capi.default_lo_params(mult=(1.0,))
    res1, info1, *_x = m.lo_db_verify_pairs(pairs, 0.7, ep, lp1)
    want1, want_info1, _ = m.lo_verify_pairs(pts0, offs0, ep, lp1)
    assert as_bytes(res1) == as_bytes(want1) and as_bytes(info1) == as_bytes(want_info1) and (info1["round"] <= 0).all()
    # `cap` one too small: as lcm_pose_db_verify_pairs, and nothing new is written either
    total = int(offs[-1])
    bufs = dict(out=np.full(total, FILL, np.uint8).repeat(16).view(pkg.capi.DMATCH_DTYPE),
                pts=np.full((total, 16), FILL, np.uint8).view(np.float32),
                results=np.full(len(pairs) * 88, FILL, np.uint8).view(pkg.capi.EPI_RESULT_DTYPE),
                info=np.full(len(pairs) * 16, FILL, np.uint8).view(pkg.capi.LO_INFO_DTYPE),
                mask=np.full(total, FILL, np.uint8),
                pose_results=np.full(len(pairs) * 128, FILL, np.uint8).view(pkg.capi.POSE_RESULT_DTYPE),
                pose_mask=np.full(total, FILL, np.uint8))
    with pytest.raises(pkg.LcmError) as e:
        m.lo_db_verify_pairs(pairs, 0.7, ep, cap=total - 1, **bufs)
    assert e.value.code == -4 and int(m.last_offsets[len(pairs)]) == total
    for a in bufs.values():
        assert (a.view(np.uint8) == FILL).all()
    bad_lp = pkg.capi.default_lo_params()
    bad_lp.mult[0] = 0.5
    for bad in (dict(ep=params(pkg, iters=96)), dict(ep=ep, lp=bad_lp), dict(ep=ep, lp=pkg.capi.default_lo_params(rounds=9)),
                dict(ep=ep, pp=pkg.capi.default_pose_params(max_depth=0.0))):
        with pytest.raises(pkg.LcmError) as e:
            m.lo_db_verify_pairs(pairs, 0.7, **bad, **bufs)
        assert e.value.code == -1
        for a in bufs.values():
            assert (a.view(np.uint8) == FILL).all()
    # no pair: nothing to do; the pose form around it returns what it returned
    r_none, i_none, *_x = m.lo_db_verify_pairs([(CURR, CURR)][:0], 0.7, ep)
    assert len(r_none) == 0 and len(i_none) == 0
    again = m.pose_db_verify_pairs(pairs, 0.7, ep)
    assert as_bytes(again[0]) == as_bytes(pose[0]) and as_bytes(again[1]) == as_bytes(pose[1]) and as_bytes(again[4]) == as_bytes(pose[4])


def test_store_detect_loops(pkg, noisy_store):
    m, frames, kps = noisy_store
    ep = params(pkg)
    c0, np0, res0, pres0, out0, pts0, mask0, pmask0, offs0, best0 = m.pose_db_detect_loops(CURR, 1, ep)
    assert [int(c) for c in c0["matched_frame_id"]] == [0, 1, 3]               # 100 shared rows are below the gate of 300
    cands, npairs, res, info, pres, out, pts, mask, pmask, offs, best = m.lo_db_detect_loops(CURR, 1, ep)
    assert as_bytes(cands) == as_bytes(c0) and npairs == np0
    assert as_bytes(out) == as_bytes(out0) and as_bytes(pts) == as_bytes(pts0) and as_bytes(offs) == as_bytes(offs0)
    # the verify call on its candidates, plus lcm_pose_best on the host
    pairs = [(CURR, int(c)) for c in cands["matched_frame_id"]]
    v_res, v_info, v_pres, v_out, v_pts, v_mask, v_pmask, v_offs = m.lo_db_verify_pairs(pairs, 0.7, ep)
    assert as_bytes(res) == as_bytes(v_res) and as_bytes(info) == as_bytes(v_info) and as_bytes(pres) == as_bytes(v_pres)
    assert as_bytes(mask) == as_bytes(v_mask) and as_bytes(pmask) == as_bytes(v_pmask) and as_bytes(offs) == as_bytes(v_offs)
    assert best == pkg.capi.pose_best(res, pres, ep)
    assert (info["n_inliers_ransac"] == res0["n_inliers"]).all()
    before = [pkg.capi.pose_loop_test(r, q, ep) for r, q in zip(res0, pres0)]
    after = [pkg.capi.pose_loop_test(r, q, ep) for r, q in zip(res, pres)]
    print(f"inliers {res0['n_inliers'].tolist()} -> {res['n_inliers'].tolist()} of {res['n_points'].tolist()}; verdicts {before} -> {after}; "
          f"best {best0} -> {best}")
    assert before != after and all(x or not y for x, y in zip(after, before))  # at least one verdict turns, none is lost
    assert best >= 0 and best == int(np.argmax(np.where(after, res["n_inliers"], -1)))
    # floor_inliers reaches lcm_pose_best
    *_x, b = m.lo_db_detect_loops(CURR, 1, ep, floor_inliers=int(res["n_inliers"].max()))
    assert b == -1
    # `cap` too small and too few candidate slots: refused, as the pose form
    total = int(offs[-1])
    with pytest.raises(pkg.LcmError) as e:
        m.lo_db_detect_loops(CURR, 1, ep, cap=total - 1)
    assert e.value.code == -4 and int(m.last_offsets[3]) == total
    with pytest.raises(pkg.LcmError) as e:
        m.lo_db_detect_loops(CURR, 1, ep, cand_cap=2)
    assert e.value.code == -4
    # the host-query form: the current frame's rows and points standing for position 4
    m.l2_db_truncate(CURR)
    try:
        got = m.lo_db_detect_loops(CURR, 1, ep, query=frames[CURR], query_pts=kps[CURR])
        for x, y in zip(got[:10], (cands, npairs, res, info, pres, out, pts, mask, pmask, offs)):
            assert as_bytes(np.asarray(x)) == as_bytes(np.asarray(y))
        assert got[10] == best
        none = m.lo_db_detect_loops(CURR, 1, ep, query=frames[CURR][:250], query_pts=kps[CURR][:250])
        assert len(none[0]) == 0 and len(none[3]) == 0 and none[9].tolist() == [0] and none[10] == -1
    finally:
        assert m.l2_db_append_kp(frames[CURR], kps[CURR]) == CURR


# ---- 7. edges ---------------------------------------------------------------------------------------------------------------
def test_seventy_thousand_pairs_make_two_slices(pkg, matcher):
    """70 000 pairs of 8 records, 64 hypotheses each (every hypothesis a seed): more pairs than gridDim.y holds, so every
    launch is sliced.  Every pair's count and every mask byte are the rule's verdict under the pair's reported E, the RANSAC's
    part is lcm_epi_verify_pairs's, and an unimproved pair keeps its record."""
    n_pairs = 70000
    offs = (8 * np.arange(n_pairs + 1)).astype(np.uintp)
    total = int(offs[-1])
    pts, _ = R.make_scene(total - total // 5, total // 5, 12)
    ep = params(pkg, iters=64)
    res0, mask0 = matcher.epi_verify_pairs(pts, offs, ep)
    res, info, mask = matcher.lo_verify_pairs(pts, offs, ep)
    launch = matcher.launch_info()
    assert launch.launches == 10 and launch.pairs == n_pairs
    pair_of = np.repeat(np.arange(n_pairs), 8)
    a, b, c, d = R.normalise(pts)
    want = R.inliers_each(res["E"][pair_of], a, b, c, d, R.threshold2()).astype(np.uint8)
    np.testing.assert_array_equal(mask, want)
    np.testing.assert_array_equal(res["n_inliers"], want.reshape(-1, 8).sum(axis=1))
    np.testing.assert_array_equal(info["n_inliers_ransac"], res0["n_inliers"])
    np.testing.assert_array_equal(info["seed_iter"], res["best_iter"])
    assert (info["status"] == L.OK).all() and (res["status"] == 0).all() and (res["n_points"] == 8).all()
    kept = info["round"] == -1
    assert as_bytes(res[kept]) == as_bytes(res0[kept]) and (res["n_inliers"][~kept] > res0["n_inliers"][~kept]).all()
    assert as_bytes(mask.reshape(-1, 8)[kept]) == as_bytes(mask0.reshape(-1, 8)[kept])
    assert (info["round"][~kept] < 4).all() and (res["best_iter"] >= 0).all() and (res["best_iter"] < 64).all()
    # eight records leave the eight-point solver nothing to gain where they all fit: most pairs keep their record
    print(f"kept {int(kept.sum())} of {n_pairs}, improved {int((~kept).sum())}; in the second slice kept {int(kept[65535:].sum())}")
    assert kept[:65535].any() and kept[65535:].any() and (res["n_inliers"][65535:] >= 8).any()


def test_rounds_and_multipliers_reach_the_kernel(pkg, matcher):
    pts = S.scene("n400_s3")[0]
    offs = np.array([0, len(pts)], np.uintp)
    ep = params(pkg)
    res0, _ = matcher.epi_verify_pairs(pts, offs, ep)
    seen = {}
    for key, lp in (("default", None), ("one", pkg.capi.default_lo_params(mult=(3.0,))), ("eight", pkg.capi.default_lo_params(mult=(3.0, 3.0, 2.0, 2.0, 1.5, 1.5, 1.0, 1.0))),
                    ("tight", pkg.capi.default_lo_params(mult=(1.0, 1.0, 1.0, 1.0))), ("explicit", pkg.capi.default_lo_params())):
        res, info, mask = matcher.lo_verify_pairs(pts, offs, ep, lp)
        a, b, c, d = R.normalise(pts)
        assert int(R.inliers(res[0]["E"].reshape(1, 9), a, b, c, d, R.threshold2()).sum()) == res[0]["n_inliers"] == int(mask.sum())
        assert res[0]["n_inliers"] >= res0[0]["n_inliers"] and info[0]["round"] < (lp.rounds if lp else 4)
        seen[key] = (as_bytes(res), as_bytes(info))
        print(f"{key}: {res0[0]['n_inliers']} -> {res[0]['n_inliers']} round {info[0]['round']}")
    assert seen["default"] == seen["explicit"]                         # NULL is the defaults
    assert seen["tight"] != seen["default"] and seen["one"] != seen["default"]


def test_refusals_with_a_handle_write_nothing(pkg, matcher):
    lib = pkg.load_library()
    pts = np.zeros((16, 4), np.float32)
    offs = np.array([0, 16], np.uintp)
    E = np.zeros((64, 9))
    counts = np.zeros(64, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    ok = params(pkg, iters=64)
    h = matcher._h
    res, info, mask = np.full(88, FILL, np.uint8), np.full(16, FILL, np.uint8), np.full(16, FILL, np.uint8)
    seeds, Eo, n_sel, status = np.full(256, FILL, np.uint8), np.full(64 * 72, FILL, np.uint8), np.full(256, FILL, np.uint8), np.full(256, FILL, np.uint8)
    verify = lambda ep, lp, o=offs, p=pts, r=res, i=info: lib.lcm_lo_verify_pairs(     # noqa: E731
        h, None if p is None else vp(p), None if o is None else vp(o), 1, None if ep is None else C.byref(ep),
        None if lp is None else C.byref(lp), None if r is None else vp(r), None if i is None else vp(i), vp(mask))
    for ep in (None, pkg.capi.default_epi_params(), params(pkg, iters=96), params(pkg, threshold=-1.0)):
        assert verify(ep, None) == -1
    for over in (dict(rounds=0), dict(rounds=9), dict(seeds=32)):
        lp = pkg.capi.default_lo_params()
        for k, v in over.items():
            setattr(lp, k, v)
        assert verify(ok, lp) == -1
    for bad in (0.999, float("nan"), float("inf"), -2.0):
        lp = pkg.capi.default_lo_params()
        lp.mult[3] = bad
        assert verify(ok, lp) == -1
        assert lib.lcm_lo_refit_models(h, vp(pts), 16, vp(E), 64, C.c_double(bad), C.byref(ok), vp(Eo), vp(n_sel), vp(status)) == -1
    assert verify(ok, None, o=None) == -1 and verify(ok, None, p=None) == -1 and verify(ok, None, r=None) == -1 and verify(ok, None, i=None) == -1
    assert verify(ok, None, o=np.array([0, 65536], np.uintp)) == -4 and verify(ok, None, o=np.array([16, 0], np.uintp)) == -1
    for n_models in (0, 65, -1):
        assert lib.lcm_lo_refit_models(h, vp(pts), 16, vp(E), n_models, C.c_double(1.0), C.byref(ok), vp(Eo), vp(n_sel), vp(status)) == -1
    assert lib.lcm_lo_refit_models(h, vp(pts), 65536, vp(E), 64, C.c_double(1.0), C.byref(ok), vp(Eo), vp(n_sel), vp(status)) == -4
    assert lib.lcm_lo_refit_models(h, vp(pts), 16, None, 64, C.c_double(1.0), C.byref(ok), vp(Eo), vp(n_sel), vp(status)) == -1
    assert lib.lcm_lo_refit_models(h, vp(pts), 16, vp(E), 64, C.c_double(1.0), None, vp(Eo), vp(n_sel), vp(status)) == -1
    for iters in (0, 63, 100, 65536 + 64):
        assert lib.lcm_lo_select(h, vp(np.zeros(max(iters, 1), np.int32)), iters, vp(seeds)) == -1
    assert lib.lcm_lo_select(h, None, 64, vp(seeds)) == -1 and lib.lcm_lo_select(h, vp(counts), 64, None) == -1
    big = counts.copy()
    big[5] = 65536
    assert lib.lcm_lo_select(h, vp(big), 64, vp(seeds)) == -1
    big[5] = -1
    assert lib.lcm_lo_select(h, vp(big), 64, vp(seeds)) == -1
    for a in (res, info, mask, seeds, Eo, n_sel, status):
        assert (a == FILL).all()
    assert lib.lcm_lo_verify_pairs(h, None, vp(np.zeros(1, np.uintp)), 0, C.byref(ok), None, None, None, None) == 0     # no pair: nothing to do
