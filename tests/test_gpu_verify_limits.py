"""The loop verification on the device (lcm_epi_*, lcm_lo_*, lcm_pose_* and the store's forms; lcm_epi.hip, lcm_lo.hip,
lcm_pose.hip, lcm_verify.cpp) at its record limit and at its tile seams, on tests/verifylimitcases.py's inputs.  Needs a real
MI355X.

include/lcm.h: a pair holds up to 65 535 records, `iters` goes up to 65 536.  The pairs here end one below, on and one above
k_epi_score's 512-record chunk (511, 512, 513), one and two of k_lo_refine's 2 016-record tiles (2015, 2016, 2017, 4032, 4033)
and on the limit (65535).  Everything but the refitted matrix is compared exactly, as in tests/test_gpu_epi.py, test_gpu_lo.py
and test_gpu_pose.py.  The refitted matrix of one optimisation round is held to the tolerance of tests/test_gpu_lo.py, 16 x
loref's own error: the worst own error over all one-round cases stays the nine-record case's 5.037e-10, the lengths here
measure 1.757e-11 (511 - 513), 1.623e-11 (2015 - 2017), 4.332e-13 (4032 / 4033) and 2.992e-13 (65535) on the CPU
(tests/test_verify_limit_cases_host.py asserts them)."""
import numpy as np
import pytest

import epicases as EC
import epiref as R
import locases as LC
import loref as L
import posecases as PC
import poseref as P
import verifylimitcases as V
from verifychecks import as_bytes, check_against_reference, check_closure

pytestmark = pytest.mark.gpu

OWN_ERROR = 5.1e-10                         # tests/test_gpu_lo.py's: the old worst case stays the worst (module docstring)
E_TOL = 16 * OWN_ERROR
SV_TOL = 16 * 1.554e-15                     # tests/test_gpu_epi.py's
BIG_PAIRS = ("big", "big2017", "big513", "big4033")


def params(pkg, **over):
    return pkg.capi.default_epi_params(R.FX, R.FY, R.CX, R.CY, **over)


def pair(pts, offs, p):
    return pts[int(offs[p]):int(offs[p + 1])]


# ---- 1. the scoring, exact --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", V.LENS)
def test_scoring_parity_at_every_length(pkg, matcher, n):
    pts = V.big_prefix(n)
    models = np.concatenate([EC.model_set(np.random.default_rng(n))[:129], np.zeros((1, 9))])
    for thr in (1.0, 0.25):
        got = matcher.epi_score_models(pts, models, params(pkg, threshold=thr))
        want = R.counts(models, pts, thr)
        np.testing.assert_array_equal(got, want, err_msg=str((n, thr)))
        assert got[-1] == 0 and len(set(want.tolist())) > 10 and want.max() > (0.6 * n if thr == 1.0 else 8)
    # exactly the planted rows below the pair's end are inliers, under E, -E and 2 E; none under the zero matrix
    E, hot_pts, hot = V.one_hot()
    models = np.stack([E, np.zeros(9), -E, 2.0 * E])
    got = matcher.epi_score_models(hot_pts[:n], models, pkg.capi.default_epi_params(*EC.K_UNIT))
    same = int((hot < n).sum())
    assert same == sum(h < n for h in V.HOT_ROWS) >= 1
    np.testing.assert_array_equal(got, [same, 0, same, same])


def test_scoring_a_full_pair(pkg, matcher):
    got = matcher.epi_score_models(V.full(), np.stack([R.E_TRUE, -R.E_TRUE, np.zeros(9)]), params(pkg))
    assert got.tolist() == [V.LIMIT, V.LIMIT, 0]


# ---- 2. the sampler at the limit, exact --------------------------------------------------------------------------------------
def test_sampler_at_the_limit(pkg, matcher):
    for position in (0, 70000):
        s, E = matcher.epi_hypotheses(V.full(), position, params(pkg, iters=V.ITERS))
        np.testing.assert_array_equal(s, R.samples(0, position, V.ITERS, V.LIMIT), err_msg=str(position))
        assert (s > 32767).any() and (s > V.LIMIT - V.EPI_CHUNK).any() and np.isfinite(E).all()


# ---- 3. the RANSAC and the optimisation over the mixed call ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(pkg, matcher):
    """mixed_call() at both sampler seeds with 64 hypotheses, once: the RANSAC's records, the optimised ones, the launch
    records, and per pair the device's own hypotheses, their counts and the 64 seeds recomputed from those in numpy."""
    pts, offs = V.mixed_call()
    out = {}
    for seed in LC.SEEDS:
        ep = params(pkg, iters=V.ITERS, seed=seed)
        res0, mask0 = matcher.epi_verify_pairs(pts, offs, ep)
        launch0 = matcher.launch_info()
        res, info, mask = matcher.lo_verify_pairs(pts, offs, ep)
        launch = matcher.launch_info()
        hyps, counts = [], []
        for p in range(len(V.MIXED)):
            pp = pair(pts, offs, p)
            hyps.append(matcher.epi_hypotheses(pp, p, ep))
            counts.append(matcher.epi_score_models(pp, hyps[p][1], ep) if len(pp) >= 8 else None)
        out[seed] = dict(ep=ep, res0=res0.copy(), mask0=mask0.copy(), res=res.copy(), info=info.copy(), mask=mask.copy(), hyps=hyps,
                         counts=counts, launches=(launch0.launches, launch0.pairs, launch.launches, launch.pairs),
                         ms=(launch0.kernel_ms, launch.kernel_ms, launch.aux_kernel_ms))
    return pts, offs, out


@pytest.mark.parametrize("seed", LC.SEEDS)
def test_ransac_over_the_mixed_call(pkg, matcher, mixed, seed):
    pts, offs, out = mixed
    o = out[seed]
    res0, mask0, hyps, ep = o["res0"], o["mask0"], o["hyps"], o["ep"]
    assert o["launches"][:2] == (3, len(V.MIXED))
    check_closure(res0, mask0, pts, offs, hyps, range(len(V.MIXED)))
    for p, name in enumerate(V.MIXED):
        print(f"seed {seed} {name}: {res0[p]['n_inliers']} of {res0[p]['n_points']} at hypothesis {res0[p]['best_iter']}")
    # the full pair: the count's top byte is all ones; where the device's own hypothesis 0 holds every record, the key is
    # 0xFFFFFFFF and the record says exactly that
    f = V.MIXED.index("full")
    assert res0[f]["n_inliers"] >= 65280
    n_in, best, _ = R.closure(hyps[f][1], pair(pts, offs, f))
    if (n_in, best) == (V.LIMIT, 0):
        assert (res0[f]["n_inliers"], res0[f]["best_iter"]) == (V.LIMIT, 0) and pair(mask0, offs, f).all()
        assert as_bytes(res0[f]["E"]) == as_bytes(hyps[f][1][0])
    assert (o["counts"][f] == R.counts(hyps[f][1], pair(pts, offs, f))).all()
    # the short pairs keep their records inside the long pairs' grid
    for name in ("empty", "seven"):
        p = V.MIXED.index(name)
        r = res0[p]
        assert (r["status"], r["n_inliers"], r["best_iter"], r["n_points"]) == (pkg.capi.EPI_TOO_FEW, 0, 0, len(pair(pts, offs, p)))
        assert not r["E"].any() and not pair(mask0, offs, p).any()
    e = V.MIXED.index("eight")
    assert (res0[e]["status"], res0[e]["n_inliers"], res0[e]["best_iter"]) == (pkg.capi.EPI_OK, 8, 0) and pair(mask0, offs, e).all()
    assert (o["counts"][e] == 8).all()
    for name in BIG_PAIRS:
        p = V.MIXED.index(name)
        np.testing.assert_array_equal(o["counts"][p], R.counts(hyps[p][1], pair(pts, offs, p)), err_msg=name)
    if seed != LC.SEEDS[0]:
        return
    # mask == NULL: the same result bytes; the same call again: the same bytes
    res1, none = matcher.epi_verify_pairs(pts, offs, ep, want_mask=False)
    assert none is None and as_bytes(res1) == as_bytes(res0)
    info = matcher.launch_info()
    assert info.launches == 3 and info.pairs == len(V.MIXED) and info.kernel_ms > 0
    # the same 4 033 records at positions 0 and 7 of another call: position 7 gives the mixed call's bytes, position 0 differs
    # through its sampler's seed alone (its closure is on the hypotheses of position 0)
    last = len(V.MIXED) - 1
    p4033 = V.big_prefix(4033)
    offs2 = np.array([0] + [4033] * last + [8066], np.uintp)
    pts2 = np.ascontiguousarray(np.concatenate([p4033, p4033]))
    res2, mask2 = matcher.epi_verify_pairs(pts2, offs2, ep)
    assert as_bytes(res2[last]) == as_bytes(res0[last]) and as_bytes(mask2[4033:]) == as_bytes(pair(mask0, offs, last))
    h0 = matcher.epi_hypotheses(p4033, 0, ep)
    check_closure(res2, mask2, pts2, offs2, {0: h0, last: hyps[last]}, (0, last))
    assert as_bytes(h0[0]) != as_bytes(hyps[last][0]) and as_bytes(res2[0]["E"]) != as_bytes(res2[last]["E"])
    assert (res2[1:last]["status"] == pkg.capi.EPI_TOO_FEW).all() and not res2[1:last]["n_points"].any()


def test_ransac_counts_on_both_sides_of_15_bits(pkg, matcher):
    """One wave of 64 hypotheses whose keys have the top bit set (some 60 000 inliers) beside keys that have it clear."""
    pts = V.most()
    offs = np.array([0, V.LIMIT], np.uintp)
    ep = params(pkg, iters=V.ITERS)
    res, mask = matcher.epi_verify_pairs(pts, offs, ep)
    info = matcher.launch_info()
    assert info.launches == 3 and info.pairs == 1
    hyps = matcher.epi_hypotheses(pts, 0, ep)
    check_closure(res, mask, pts, offs, [hyps], (0,))
    cnt = matcher.epi_score_models(pts, hyps[1], ep)
    np.testing.assert_array_equal(cnt, R.counts(hyps[1], pts))
    assert (cnt >= 32768).sum() >= 16 and (cnt < 32768).sum() >= 16 and res[0]["n_inliers"] == cnt.max() >= 60000
    res1, info1, mask1 = matcher.lo_verify_pairs(pts, offs, ep)
    lo_closure(pkg, "most", pts, res1[0], res[0], info1[0], mask1, mask, L.select(cnt))
    print(f"most: {res[0]['n_inliers']} at hypothesis {res[0]['best_iter']} -> {res1[0]['n_inliers']} round {info1[0]['round']}")


def lo_closure(pkg, name, pp, r, r0, i, m, m0, seeds, rounds=4):
    """What tests/test_gpu_lo.py's test_closure_on_the_devices_own_output asserts of one pair."""
    n = len(pp)
    a, b, c, d = R.normalise(pp)
    want = (R.inliers(r["E"].reshape(1, 9), a, b, c, d, R.threshold2())[0] if n else np.zeros(0, bool)).astype(np.uint8)
    np.testing.assert_array_equal(m, want, err_msg=name)
    assert r["n_inliers"] == int(want.sum()) and r["n_points"] == n and r["status"] == r0["status"] == (1 if n < 8 else 0)
    assert i["n_inliers_ransac"] == r0["n_inliers"] and r["n_inliers"] >= r0["n_inliers"]
    assert i["seed_iter"] == r["best_iter"]
    assert i["status"] == (L.TOO_FEW if n < 8 else L.OK), (name, i)
    if i["round"] == -1:
        assert as_bytes(r) == as_bytes(r0) and as_bytes(m) == as_bytes(m0), name
    else:
        assert 0 <= i["round"] < rounds and r["n_inliers"] > r0["n_inliers"] and r["best_iter"] in seeds.tolist(), (name, i)
        assert R.singular_deviation(r["E"])[0] <= SV_TOL
    if seeds is not None:
        assert seeds[0] == r0["best_iter"]
    if n < 8:
        assert i["round"] == -1 and not r["E"].any() and r["n_inliers"] == 0


@pytest.mark.parametrize("seed", LC.SEEDS)
def test_optimisation_over_the_mixed_call(pkg, matcher, mixed, seed):
    pts, offs, out = mixed
    o = out[seed]
    res0, mask0, res, info, mask = o["res0"], o["mask0"], o["res"], o["info"], o["mask"]
    assert o["launches"][2:] == (5, len(V.MIXED))
    print(f"seed {seed}: kernel_ms of the RANSAC call {o['ms'][0]:.3f}, of the optimised call {o['ms'][1]:.3f} (aux_kernel_ms {o['ms'][2]:.3f})")
    for p, name in enumerate(V.MIXED):
        seeds = None if o["counts"][p] is None else L.select(o["counts"][p])
        lo_closure(pkg, name, pair(pts, offs, p), res[p], res0[p], info[p], pair(mask, offs, p), pair(mask0, offs, p), seeds)
        print(f"seed {seed} {name}: RANSAC {res0[p]['n_inliers']} -> {res[p]['n_inliers']} of {res[p]['n_points']} round {info[p]['round']} "
              f"seed_iter {info[p]['seed_iter']}")
    # every record already an inlier, or none to gain: kept
    for name in ("full", "eight"):
        assert info[V.MIXED.index(name)]["round"] == -1
    # where the restatement over the device's OWN hypotheses gains clearly, the device gains
    gains = 0
    for name in BIG_PAIRS:
        p = V.MIXED.index(name)
        ref = L.optimise(pair(pts, offs, p), o["hyps"][p][1], o["counts"][p])
        assert ref["n_inliers_ransac"] == res0[p]["n_inliers"]
        print(f"seed {seed} {name}: loref over the device's hypotheses {ref['n_inliers_ransac']} -> {ref['n_inliers']} round {ref['round']}")
        if ref["n_inliers"] - ref["n_inliers_ransac"] >= 10:
            gains += 1
            assert info[p]["round"] >= 0 and res[p]["n_inliers"] - res0[p]["n_inliers"] >= 5, (name, ref["n_inliers"], res[p])
    assert gains >= 2
    if seed == LC.SEEDS[0]:
        res2, info2, mask2 = matcher.lo_verify_pairs(pts, offs, o["ep"])
        assert as_bytes(res2) == as_bytes(res) and as_bytes(info2) == as_bytes(info) and as_bytes(mask2) == as_bytes(mask)
        res3, info3, none = matcher.lo_verify_pairs(pts, offs, o["ep"], want_mask=False)
        assert none is None and as_bytes(res3) == as_bytes(res) and as_bytes(info3) == as_bytes(info)


def test_one_and_eight_rounds_across_two_tile_seams(pkg, matcher):
    pts = V.big_prefix(4033)
    offs = np.array([0, 4033], np.uintp)
    ep = params(pkg, iters=V.ITERS)
    res0, mask0 = matcher.epi_verify_pairs(pts, offs, ep)
    seeds = L.select(matcher.epi_score_models(pts, matcher.epi_hypotheses(pts, 0, ep)[1], ep))
    for lp in (pkg.capi.default_lo_params(mult=(3.0,)), pkg.capi.default_lo_params(mult=(3.0, 3.0, 2.0, 2.0, 1.5, 1.5, 1.0, 1.0))):
        res, info, mask = matcher.lo_verify_pairs(pts, offs, ep, lp)
        launch = matcher.launch_info()
        assert launch.launches == 5 and launch.pairs == 1
        lo_closure(pkg, f"rounds {lp.rounds}", pts, res[0], res0[0], info[0], mask, mask0, seeds, lp.rounds)
        print(f"rounds {lp.rounds}: {res0[0]['n_inliers']} -> {res[0]['n_inliers']} round {info[0]['round']}")
        assert info[0]["round"] >= 0


# ---- 4. iters = 65536 ------------------------------------------------------------------------------------------------------
def test_the_largest_number_of_hypotheses(pkg, matcher):
    iters = 65536
    ep = params(pkg, iters=iters)
    p16 = np.ascontiguousarray(EC.scene("s1025")[0][:16])
    eight = EC.scene("eight")[0]
    pts = np.ascontiguousarray(np.concatenate([p16, eight]))
    offs = np.array([0, 16, 24], np.uintp)
    hyps = [matcher.epi_hypotheses(p16, 0, ep), matcher.epi_hypotheses(eight, 1, ep)]
    np.testing.assert_array_equal(hyps[0][0], R.samples(0, 0, iters, 16))
    assert np.isfinite(hyps[0][1]).all() and np.isfinite(hyps[1][1]).all()
    assert (np.sort(hyps[1][0], axis=1) == np.arange(8)).all()
    res0, mask0 = matcher.epi_verify_pairs(pts, offs, ep)
    launch = matcher.launch_info()
    assert launch.launches == 3 and launch.pairs == 2 and launch.workgroups == 2 * 256
    check_closure(res0, mask0, pts, offs, hyps, (0, 1))
    cnt = [matcher.epi_score_models(pair(pts, offs, p), hyps[p][1], ep) for p in range(2)]
    for p in range(2):
        np.testing.assert_array_equal(cnt[p], R.counts(hyps[p][1], pair(pts, offs, p)))
    assert (cnt[1] == 8).all() and (res0[1]["n_inliers"], res0[1]["best_iter"]) == (8, 0)           # first of 65 536 equals
    res, info, mask = matcher.lo_verify_pairs(pts, offs, ep)
    launch = matcher.launch_info()
    assert launch.launches == 5 and launch.pairs == 2
    for p in range(2):
        seeds = L.select(cnt[p])
        np.testing.assert_array_equal(matcher.lo_select(cnt[p]), seeds)
        lo_closure(pkg, str(p), pair(pts, offs, p), res[p], res0[p], info[p], pair(mask, offs, p), pair(mask0, offs, p), seeds)
        print(f"pair {p}: {res0[p]['n_inliers']} -> {res[p]['n_inliers']} round {info[p]['round']} seed_iter {info[p]['seed_iter']}, "
              f"last seed {seeds[-1]}")


# ---- 5. one optimisation round through the seam ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_models", LC.REFIT_MODELS)
@pytest.mark.parametrize("n", V.LENS)
def test_one_round_at_every_length(pkg, matcher, n, n_models):
    pts = V.big_prefix(n)
    models = LC.refit_models()[:n_models]
    for mult in LC.REFIT_MULTS:
        want_E, want_n, want_status, _ = V.refit_reference(n, mult)
        E, n_sel, status = matcher.lo_refit_models(pts, models, mult, params(pkg))
        np.testing.assert_array_equal(n_sel, want_n[:n_models], err_msg=str((n, mult)))
        np.testing.assert_array_equal(status, want_status[:n_models], err_msg=str((n, mult)))
        ok = status == L.OK
        assert ok.any() and not E[~ok].any()
        dist = L.sign_aligned_distance(E[ok], want_E[:n_models][ok])
        dev = R.singular_deviation(E[ok])
        print(f"n {n} models {n_models} mult {mult}: worst distance {dist.max():.3e} (limit {E_TOL:.3e}), singular values {dev.max():.3e}, "
              f"selected up to {n_sel.max()}")
        assert dist.max() <= E_TOL, (n, mult, dist.max())
        assert dev.max() <= SV_TOL, (n, mult, dev.max())
        E2, n2, s2 = matcher.lo_refit_models(pts, models, mult, params(pkg))
        assert as_bytes(E2) == as_bytes(E) and as_bytes(n2) == as_bytes(n_sel) and as_bytes(s2) == as_bytes(status)
    if n_models >= 63:
        assert status[62] == L.TOO_FEW and n_sel[62] == 0                                           # the all-zero model


# ---- 6. the pose, exact -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_kind", PC.MASKS)
@pytest.mark.parametrize("max_depth", PC.MAX_DEPTHS)
def test_pose_parity_at_the_tile_seams_and_the_limit(pkg, matcher, mask_kind, max_depth):
    """One call of four pairs: the prefixes of the 65 535-record scene, each under the true matrix."""
    parts = [V.pose_prefix(n)[0] for n in V.POSE_LENS]
    E = V.pose_scene()[2]
    offs = np.concatenate([[0], np.cumsum(V.POSE_LENS)]).astype(np.uintp)
    pts = np.ascontiguousarray(np.concatenate(parts))
    mask_in = None if mask_kind == "null" else np.concatenate([PC.mask_of(mask_kind, n) for n in V.POSE_LENS])
    Es = np.tile(E, (len(parts), 1))
    res, mask = matcher.pose_recover_pairs(pts, offs, Es, params(pkg), pkg.capi.default_pose_params(max_depth=max_depth), mask_in)
    info = matcher.launch_info()
    assert info.launches == 1 and info.pairs == len(parts) and info.workgroups == len(parts) and info.kernel_ms > 0
    check_against_reference(res, mask, pts, offs, Es, mask_in, max_depth)
    np.testing.assert_array_equal(res["n_good"], [int(pair(mask, offs, p).sum()) for p in range(len(parts))])
    if mask_kind == "zeros":
        assert not res["n_used"].any() and (res["choice"] == 0).all()
    elif mask_kind in ("null", "ones"):
        assert res["n_used"].tolist() == list(V.POSE_LENS)
        if max_depth == P.MAX_DEPTH:                     # the near points: about 80 %, more than 15 bits at the limit
            assert (res["n_good"] > 0.7 * np.array(V.POSE_LENS)).all() and res[-1]["n_good"] > 32767


def test_pose_over_the_mixed_call(pkg, matcher, mixed):
    pts, offs, out = mixed
    o = out[LC.SEEDS[0]]
    res, mask = matcher.pose_recover_pairs(pts, offs, o["res0"]["E"], o["ep"], None, o["mask0"])
    info = matcher.launch_info()
    assert info.launches == 1 and info.pairs == len(V.MIXED)
    check_against_reference(res, mask, pts, offs, o["res0"]["E"], o["mask0"], P.MAX_DEPTH)
    for name in ("empty", "seven"):
        p = V.MIXED.index(name)
        r = res[p]
        assert (r["status"], r["choice"], r["n_used"], r["n_good"]) == (pkg.capi.POSE_NO_MODEL, -1, 0, 0)
        assert not r["R"].any() and not r["t"].any() and not r["counts"].any() and not pair(mask, offs, p).any()
    f = V.MIXED.index("full")
    assert res[f]["status"] == pkg.capi.POSE_OK and res[f]["n_used"] == o["res0"][f]["n_inliers"] and res[f]["n_good"] > 65000
    # the optimised matrices and masks go the same way
    res, mask = matcher.pose_recover_pairs(pts, offs, o["res"]["E"], o["ep"], None, o["mask"])
    check_against_reference(res, mask, pts, offs, o["res"]["E"], o["mask"], P.MAX_DEPTH)
    np.testing.assert_array_equal(res["n_used"], o["res"]["n_inliers"])


# ---- 7. the store's forms across a tile ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def limit_store(pkg):
    frames, kps, shared, scene = V.store_frames()
    m = pkg.Matcher()
    for k, (f, kp) in enumerate(zip(frames, kps)):
        assert m.l2_db_append_kp(f, kp) == k
    yield m
    m.close()


def test_store_forms_across_a_tile(pkg, limit_store):
    m = limit_store
    ep = params(pkg)
    pairs = [tuple(p) for p in V.STORE_PAIRS]
    out0, pts0, offs0 = m.l2_db_match_points(pairs, 0.7)
    n0 = m.launch_info().launches
    assert offs0.tolist() == [0, 2050, 2350]
    for k in range(2):
        qi, ti, rec = V.store_points(k)
        np.testing.assert_array_equal(pair(out0, offs0, k)["query_idx"], qi)
        np.testing.assert_array_equal(pair(out0, offs0, k)["train_idx"], ti)
        assert as_bytes(pair(pts0, offs0, k)) == as_bytes(rec)
    # the RANSAC's form and the pose form against their host-list calls
    e_res, e_out, e_pts, e_mask, e_offs = m.epi_db_verify_pairs(pairs, 0.7, ep)
    n_epi = m.launch_info().launches
    want_res, want_mask = m.epi_verify_pairs(pts0, offs0, ep)
    assert m.launch_info().launches == 3 and m.launch_info().pairs == 2
    assert as_bytes(e_res) == as_bytes(want_res) and as_bytes(e_mask) == as_bytes(want_mask)
    assert as_bytes(e_out) == as_bytes(out0) and as_bytes(e_pts) == as_bytes(pts0) and as_bytes(e_offs) == as_bytes(offs0)
    p_res, p_pres, p_out, p_pts, p_mask, p_pmask, p_offs = m.pose_db_verify_pairs(pairs, 0.7, ep)
    n_pose = m.launch_info().launches
    want_pose, want_pmask = m.pose_recover_pairs(pts0, offs0, e_res["E"], ep, None, e_mask)
    assert as_bytes(p_res) == as_bytes(e_res) and as_bytes(p_mask) == as_bytes(e_mask) and as_bytes(p_offs) == as_bytes(offs0)
    assert as_bytes(p_pres) == as_bytes(want_pose) and as_bytes(p_pmask) == as_bytes(want_pmask)
    check_against_reference(p_pres, p_pmask, pts0, offs0, e_res["E"], e_mask, P.MAX_DEPTH)
    # the optimised form: byte for byte the composition of the three host-list calls on the returned points
    res, info, pres, out, pts, mask, pmask, offs = m.lo_db_verify_pairs(pairs, 0.7, ep)
    n_lo = m.launch_info().launches
    assert as_bytes(offs) == as_bytes(offs0) and as_bytes(out) == as_bytes(out0) and as_bytes(pts) == as_bytes(pts0)
    want_res, want_info, want_mask = m.lo_verify_pairs(pts0, offs0, ep)
    assert m.launch_info().launches == 5 and m.launch_info().pairs == 2
    assert as_bytes(res) == as_bytes(want_res) and as_bytes(info) == as_bytes(want_info) and as_bytes(mask) == as_bytes(want_mask)
    want_pose, want_pmask = m.pose_recover_pairs(pts0, offs0, res["E"], ep, None, mask)
    assert as_bytes(pres) == as_bytes(want_pose) and as_bytes(pmask) == as_bytes(want_pmask)
    assert (n_epi, n_pose, n_lo) == (n0 + 3, n0 + 4, n0 + 6)
    for k in range(2):
        seeds = L.select(m.epi_score_models(pair(pts0, offs0, k), m.epi_hypotheses(pair(pts0, offs0, k), k, ep)[1], ep))
        lo_closure(pkg, str(k), pair(pts0, offs0, k), res[k], e_res[k], info[k], pair(mask, offs0, k), pair(e_mask, offs0, k), seeds)
        print(f"pair {pairs[k]}: {e_res[k]['n_inliers']} -> {res[k]['n_inliers']} of {res[k]['n_points']} round {info[k]['round']}")
    assert info[0]["round"] >= 0 and res[0]["n_inliers"] > 0.7 * 2050
    # the keyframe's own search finds both frames and returns the same records and the same best loop
    cands, npairs, d_res, d_info, d_pres, d_out, d_pts, d_mask, d_pmask, d_offs, best = m.lo_db_detect_loops(2, 1, ep)
    assert [int(c) for c in cands["matched_frame_id"]] == [0, 1] and npairs == 2
    assert as_bytes(d_res) == as_bytes(res) and as_bytes(d_info) == as_bytes(info) and as_bytes(d_pres) == as_bytes(pres)
    assert as_bytes(d_out) == as_bytes(out) and as_bytes(d_pts) == as_bytes(pts) and as_bytes(d_offs) == as_bytes(offs)
    assert as_bytes(d_mask) == as_bytes(mask) and as_bytes(d_pmask) == as_bytes(pmask)
    assert best == pkg.capi.pose_best(res, pres, ep) == 0
