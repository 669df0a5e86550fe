"""The relative-pose recovery on the device (include/lcm.h lcm_pose_*; lcm_pose.hip, lcm_pose.cpp, lcm_l2_db.cpp) against
tests/poseref.py.  Needs a real MI355X.

Everything is compared exactly: the model is +, -, x, / and square roots in double with every product and sum rounded on its
own, which is numpy's arithmetic.  The loop is also closed on the device's OWN candidates: they are read back
through lcm_pose_candidates and scored in numpy, and counts, choice and every mask byte must equal what the calls report."""
import ctypes as C

import numpy as np
import pytest

import epicases as ES
import epiref as E_
import posecases as S
import poseref as P
from verifychecks import check_against_reference

pytestmark = pytest.mark.gpu

FILL = 0xA7


def params(pkg, **over):
    return pkg.capi.default_epi_params(E_.FX, E_.FY, E_.CX, E_.CY, **over)


def as_bytes(a):
    return np.ascontiguousarray(a).tobytes()


def check_closure(matcher, res, mask, pts, offs, E, mask_in, max_depth, pairs, k=E_.K):
    """Counts, choice, n_good, R, t and the mask of `pairs` against numpy's scoring of the DEVICE's four candidates."""
    E = np.asarray(E).reshape(-1, 9)
    R4, t4, status = matcher.pose_candidates(E[list(pairs)])
    for j, p in enumerate(pairs):
        lo, hi = int(offs[p]), int(offs[p + 1])
        r = res[p]
        assert r["status"] == status[j]
        if status[j] == P.NO_MODEL:
            assert r["choice"] == -1 and not r["counts"].any() and not mask[lo:hi].any() and not r["R"].any() and not r["t"].any()
            continue
        counts, choice, n_used, m = P.score(R4[j], t4[j], pts[lo:hi], None if mask_in is None else mask_in[lo:hi], max_depth, k)
        assert (list(r["counts"]), r["choice"], r["n_used"], r["n_good"]) == (list(counts), choice, n_used, int(counts[choice])), (p, r, counts)
        np.testing.assert_array_equal(mask[lo:hi], m, err_msg=str(p))
        assert as_bytes(r["R"]) == as_bytes(R4[j, choice]) and as_bytes(r["t"]) == as_bytes(t4[j, choice])


# ---- 1. the decomposition, exact -------------------------------------------------------------------------------------------
def model_set():
    """6 integer cases, 130 random essential matrices, the zero matrix, a NaN matrix: 138."""
    return np.concatenate([[E for E, _, _ in S.integer_cases()], S.random_essentials(130, 17), [np.zeros(9)], [[np.nan] + [0.0] * 8]])


@pytest.mark.parametrize("n_models", (1, 63, 64, 65, 138))
def test_decomposition_parity(matcher, n_models):
    E = model_set()[-n_models:] if n_models < 138 else model_set()
    R4, t4, status = matcher.pose_candidates(E)
    wR, wt, ws = P.candidates(E)
    np.testing.assert_array_equal(status, ws)
    assert as_bytes(R4) == as_bytes(wR), np.abs(R4 - wR).max()
    assert as_bytes(t4) == as_bytes(wt), np.abs(t4 - wt).max()
    assert (status[-2:] == P.NO_MODEL).all() if n_models >= 2 else status[0] == P.NO_MODEL


def test_decomposition_of_the_integer_cases_is_the_planted_motion(matcher):
    cases = S.integer_cases()
    R4, t4, status = matcher.pose_candidates(np.stack([E for E, _, _ in cases]))
    assert (status == P.OK).all()
    for m, (_, R, t) in enumerate(cases):
        hits = [k for k in range(4) if (R4[m, k].reshape(3, 3) == R).all() and (t4[m, k] == t).all()]
        assert len(hits) == 1, (m, R4[m], t4[m])
    assert len(matcher.pose_candidates(np.zeros((0, 9)))[2]) == 0


# ---- 2. the depth test and the selection, exact ------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_kind", S.MASKS)
@pytest.mark.parametrize("max_depth", S.MAX_DEPTHS)
def test_cheirality_parity(pkg, matcher, mask_kind, max_depth):
    """One call of eight pairs: the prefixes of the parity scene, each under the true matrix."""
    pts1025, _, E, *_ = S.scene("p1025")
    parts = [pts1025[:n] for n in S.PARITY_SIZES]
    offs = np.concatenate([[0], np.cumsum(S.PARITY_SIZES)]).astype(np.uintp)
    pts = np.ascontiguousarray(np.concatenate(parts))
    mask_in = None if mask_kind == "null" else np.concatenate([S.mask_of(mask_kind, n) for n in S.PARITY_SIZES])
    Es = np.tile(E, (len(parts), 1))
    pp = pkg.capi.default_pose_params(max_depth=max_depth)
    res, mask = matcher.pose_recover_pairs(pts, offs, Es, params(pkg), pp, mask_in)
    check_against_reference(res, mask, pts, offs, Es, mask_in, max_depth)
    check_closure(matcher, res, mask, pts, offs, Es, mask_in, max_depth, range(len(parts)))
    np.testing.assert_array_equal(res["n_good"], [int(mask[int(offs[p]):int(offs[p + 1])].sum()) for p in range(len(parts))])
    if mask_kind == "zeros":
        assert not res["n_used"].any() and (res["choice"] == 0).all() and (res["status"] == P.OK).all()
    info = matcher.launch_info()
    assert info.launches == 1 and info.pairs == len(parts) and info.workgroups == len(parts) and info.kernel_ms > 0 and info.route == 0


def test_tie_at_identical_rays_and_default_params(pkg, matcher):
    Ez = P.essential(np.eye(3), [0.0, 0.0, 1.0])
    unit = pkg.capi.default_epi_params(*S.K_UNIT)
    res, mask = matcher.pose_recover_pairs(np.zeros((1, 4), np.float32), [0, 1], Ez, unit)             # pp == NULL: the defaults
    r = res[0]
    assert (r["choice"], r["n_used"], r["n_good"], r["status"]) == (0, 1, 0, 0) and not r["counts"].any() and mask.tolist() == [0]
    assert (r["R"].reshape(3, 3) == np.eye(3)).all() and r["t"].tolist() == [0.0, 0.0, 1.0]
    pts, kind, E, *_ = S.scene("general")
    a, _ = matcher.pose_recover_pairs(pts, [0, len(pts)], E, params(pkg))
    b, _ = matcher.pose_recover_pairs(pts, [0, len(pts)], E, params(pkg), pkg.capi.default_pose_params())
    assert as_bytes(a) == as_bytes(b)
    none = matcher.pose_recover_pairs(pts, [0, len(pts)], E, params(pkg), want_mask=False)
    assert none[1] is None and as_bytes(none[0]) == as_bytes(a)


# ---- 3. planted scenes ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted_call(pkg, matcher):
    """The four motions under E and -E, with the planted mask: one call of eight pairs."""
    names = ("forward", "sideways", "general", "twisted")
    parts, Es, masks = [], [], []
    for nm in names:
        pts, kind, E, *_ = S.scene(nm)
        for sign in (1.0, -1.0):
            parts.append(pts), Es.append(sign * E), masks.append(S.planted_mask(kind))
    offs = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uintp)
    pts, Es, mask_in = np.ascontiguousarray(np.concatenate(parts)), np.stack(Es), np.concatenate(masks)
    res, mask = matcher.pose_recover_pairs(pts, offs, Es, params(pkg), None, mask_in)
    return names, pts, offs, Es, mask_in, res.copy(), mask.copy()


def test_planted_scenes_recover_the_planted_motion(pkg, matcher, planted_call):
    names, pts, offs, Es, mask_in, res, mask = planted_call
    check_against_reference(res, mask, pts, offs, Es, mask_in, P.MAX_DEPTH)
    check_closure(matcher, res, mask, pts, offs, Es, mask_in, P.MAX_DEPTH, range(len(res)))
    for j, nm in enumerate(names):
        _, kind, _, R, t = S.scene(nm)
        plus, minus = res[2 * j], res[2 * j + 1]
        dR, dt = P.motion_error(plus["R"], plus["t"], R, t)
        assert dR <= S.TRUTH_TOL and dt <= S.TRUTH_TOL, (nm, dR, dt)                      # the true matrix went in: rounding only
        lo, mid, hi = int(offs[2 * j]), int(offs[2 * j + 1]), int(offs[2 * j + 2])
        np.testing.assert_array_equal(mask[lo:mid], (kind == 0).astype(np.uint8))      # the near points, not the far ones, no outlier
        assert plus["n_good"] == (kind == 0).sum() and plus["n_used"] == (kind != 2).sum()
        # E negated: Ra and Rb change places, nothing else does
        assert as_bytes(minus["R"]) == as_bytes(plus["R"]) and as_bytes(minus["t"]) == as_bytes(plus["t"])
        assert as_bytes(mask[mid:hi]) == as_bytes(mask[lo:mid]) and (minus["n_used"], minus["n_good"]) == (plus["n_used"], plus["n_good"])
        assert minus["choice"] == plus["choice"] ^ 1 and list(minus["counts"]) == [int(plus["counts"][h ^ 1]) for h in range(4)]
        assert pkg.capi.pose_loop_test(dict(n_points=len(kind), n_inliers=int((kind != 2).sum()), best_iter=0, status=0), plus, params(pkg))


def test_determinism_over_calls_and_positions(pkg, matcher, planted_call):
    names, pts, offs, Es, mask_in, res, mask = planted_call
    res2, mask2 = matcher.pose_recover_pairs(pts, offs, Es, params(pkg), None, mask_in)
    assert as_bytes(res2) == as_bytes(res) and as_bytes(mask2) == as_bytes(mask)
    order = [5, 0, 7, 2, 2, 6]                                               # other positions, other neighbours, one pair twice
    parts = [pts[int(offs[p]):int(offs[p + 1])] for p in order]
    offs3 = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uintp)
    m3 = np.concatenate([mask_in[int(offs[p]):int(offs[p + 1])] for p in order])
    res3, mask3 = matcher.pose_recover_pairs(np.concatenate(parts), offs3, Es[order], params(pkg), None, m3)
    for j, p in enumerate(order):
        assert as_bytes(res3[j]) == as_bytes(res[p])
        assert as_bytes(mask3[int(offs3[j]):int(offs3[j + 1])]) == as_bytes(mask[int(offs[p]):int(offs[p + 1])])


# ---- 4. after the RANSAC ---------------------------------------------------------------------------------------------------
def test_pose_after_the_ransac_and_no_model(pkg, matcher):
    """lcm_epi_verify_pairs' own E and mask go in: the eight-point E of a scene gives a pose with most inliers in front;
    LCM_EPI_TOO_FEW and an all-zero E give LCM_POSE_NO_MODEL with zero records and an all-zero mask."""
    pts, offs, scenes = ES.verify_call()
    ep = params(pkg)
    eres, emask = matcher.epi_verify_pairs(pts, offs, ep)
    res, mask = matcher.pose_recover_pairs(pts, offs, eres["E"], ep, None, emask)
    check_against_reference(res, mask, pts, offs, eres["E"], emask, P.MAX_DEPTH)
    check_closure(matcher, res, mask, pts, offs, eres["E"], emask, P.MAX_DEPTH, range(len(scenes)))
    for p, (name, planted) in enumerate(scenes):
        lo, hi = int(offs[p]), int(offs[p + 1])
        r = res[p]
        if eres[p]["status"] == pkg.capi.EPI_TOO_FEW:
            assert (r["status"], r["choice"], r["n_used"], r["n_good"]) == (pkg.capi.POSE_NO_MODEL, -1, 0, 0)
            assert not r["R"].any() and not r["t"].any() and not r["counts"].any() and not mask[lo:hi].any()
            assert not pkg.capi.pose_loop_test(eres[p], r, ep)
            continue
        assert r["status"] == pkg.capi.POSE_OK and r["n_used"] == eres[p]["n_inliers"] and r["n_good"] == mask[lo:hi].sum()
        assert not mask[lo:hi][emask[lo:hi] == 0].any()                      # only the RANSAC's inliers take part
    verdicts = {name: pkg.capi.pose_loop_test(eres[p], res[p], ep) for p, (name, _) in enumerate(scenes)}
    assert verdicts == {"s400_280": True, "out400": False, "empty": False, "seven": False, "eight": False, "s65": False, "s1025": True}
    assert res[0]["n_good"] > 100 and res[6]["n_good"] > 100
    # a pair whose E is all zero (no hypothesis had an inlier): 400 records, no model
    out, planted = ES.scene("out400")
    r0, m0 = matcher.pose_recover_pairs(out, [0, 400], np.zeros(9), ep)
    assert (r0[0]["status"], r0[0]["choice"], r0[0]["n_used"]) == (1, -1, 0) and not m0.any() and len(m0) == 400
    assert as_bytes(r0[0]) == as_bytes(np.array([(np.zeros(9), np.zeros(3), np.zeros(4), 0, 0, -1, 1)], pkg.capi.POSE_RESULT_DTYPE)[0])


def test_refusals_with_a_handle_write_nothing(pkg, matcher):
    lib = pkg.load_library()
    pts = np.zeros((16, 4), np.float32)
    offs = np.array([0, 16], np.uintp)
    E = np.zeros((1, 9))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    ok = params(pkg)
    h = matcher._h
    res, mask = np.full(128, FILL, np.uint8), np.full(16, FILL, np.uint8)
    for ep in (None, pkg.capi.default_epi_params(), pkg.capi.default_epi_params(700.0, -1.0, 320.0, 240.0)):
        epp = None if ep is None else C.byref(ep)
        assert lib.lcm_pose_recover_pairs(h, vp(pts), vp(offs), 1, vp(E), None, epp, None, vp(res), vp(mask)) == -1
    for md in (0.0, -50.0, float("nan")):
        pp = pkg.capi.default_pose_params(max_depth=md)
        assert lib.lcm_pose_recover_pairs(h, vp(pts), vp(offs), 1, vp(E), None, C.byref(ok), C.byref(pp), vp(res), vp(mask)) == -1
    assert lib.lcm_pose_recover_pairs(h, vp(pts), None, 1, vp(E), None, C.byref(ok), None, vp(res), vp(mask)) == -1            # NULL offsets
    assert lib.lcm_pose_recover_pairs(h, None, vp(offs), 1, vp(E), None, C.byref(ok), None, vp(res), vp(mask)) == -1           # NULL points
    assert lib.lcm_pose_recover_pairs(h, vp(pts), vp(offs), 1, None, None, C.byref(ok), None, vp(res), vp(mask)) == -1         # NULL matrices
    assert lib.lcm_pose_recover_pairs(h, vp(pts), vp(offs), 1, vp(E), None, C.byref(ok), None, None, vp(mask)) == -1           # NULL results
    assert lib.lcm_pose_recover_pairs(h, vp(pts), vp(np.array([0, 65536], np.uintp)), 1, vp(E), None, C.byref(ok), None, vp(res), vp(mask)) == -4
    assert lib.lcm_pose_recover_pairs(h, vp(pts), vp(np.array([16, 0], np.uintp)), 1, vp(E), None, C.byref(ok), None, vp(res), vp(mask)) == -1
    R4, t4, st = np.full(36 * 8, FILL, np.uint8), np.full(12 * 8, FILL, np.uint8), np.full(4, FILL, np.uint8)
    assert lib.lcm_pose_candidates(h, None, 1, vp(R4), vp(t4), vp(st)) == -1
    assert lib.lcm_pose_candidates(h, vp(E), -1, vp(R4), vp(t4), vp(st)) == -1
    assert lib.lcm_pose_candidates(h, vp(E), 1, vp(R4), None, vp(st)) == -1
    for a in (res, mask, R4, t4, st):
        assert (a == FILL).all()
    assert lib.lcm_pose_recover_pairs(h, None, vp(np.zeros(1, np.uintp)), 0, None, None, C.byref(ok), None, None, None) == 0     # no pair: nothing to do


# ---- 5. the store's forms -------------------------------------------------------------------------------------------------
CURR = 4
PASTS = ((500, 420), (520, 330), (300, 100), (400, 310))          # (rows, rows shared with the current frame)


@pytest.fixture(scope="module")
def loop_store(pkg):
    """A matcher of its own with four past frames and a current one (slot 4).  A past frame shares rows (exact copies: the only
    survivors of the ratio test among uniformly random rows) with the current one; the shared rows' keypoints are the two sides
    of a scene's correspondences under the `general` motion, 400 true and 120 planted false ones over the current frame's 520
    rows."""
    rng = np.random.default_rng(78)
    R, t = S.MOTIONS["general"]
    pts, kind = P.make_scene(R, t, 400, 0, 120, 22)
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
    yield m, frames, kps, shared, kind == 0
    m.close()


def test_store_verify_pairs(pkg, loop_store):
    m, frames, kps, shared, planted = loop_store
    ep = params(pkg)
    pairs = [(CURR, 0), (CURR, 2), (CURR, 1), (CURR, 3)]
    res0, out0, pts0, mask0, offs0 = m.epi_db_verify_pairs(pairs, 0.7, ep)
    info0 = m.launch_info()
    res, pres, out, pts, mask, pmask, offs = m.pose_db_verify_pairs(pairs, 0.7, ep)
    info = m.launch_info()
    # everything the RANSAC's form returns, byte for byte
    assert as_bytes(offs) == as_bytes(offs0) and as_bytes(out) == as_bytes(out0) and as_bytes(pts) == as_bytes(pts0)
    assert as_bytes(res) == as_bytes(res0) and as_bytes(mask) == as_bytes(mask0)
    # the pose: lcm_pose_recover_pairs on the returned points, E and mask; poseref on the same
    want, want_mask = m.pose_recover_pairs(pts0, offs0, res0["E"], ep, None, mask0)
    assert as_bytes(pres) == as_bytes(want) and as_bytes(pmask) == as_bytes(want_mask)
    check_against_reference(pres, pmask, pts0, offs0, res0["E"], mask0, P.MAX_DEPTH)
    for k, (_, past) in enumerate(pairs):
        true = planted[shared[past][0]]
        assert pres[k]["status"] == 0 and pres[k]["n_used"] == res[k]["n_inliers"] and pres[k]["n_good"] == pmask[int(offs[k]):int(offs[k + 1])].sum()
        assert pkg.capi.pose_loop_test(res[k], pres[k], ep) == (past != 2), (past, res[k]["n_inliers"], pres[k]["n_good"], true.sum())
    # the launch record: the RANSAC form's, plus one kernel
    assert (info.workgroups, info.pairs, info.route, info.distances) == (info0.workgroups, info0.pairs, info0.route, info0.distances)
    assert info.launches == info0.launches + 1 and info.kernel_ms > 0 and info.aux_kernel_ms > 0
    # another far limit reaches the kernel
    pp = pkg.capi.default_pose_params(max_depth=12.0)
    _, pres12, *_rest, pmask12, _ = m.pose_db_verify_pairs(pairs, 0.7, ep, pp)
    check_against_reference(pres12, pmask12, pts0, offs0, res0["E"], mask0, 12.0)
    assert (pres12["n_good"] < pres["n_good"]).all()
    # `cap` one too small: as lcm_epi_db_verify_pairs, and nothing new is written either
    total = int(offs[-1])
    bufs = dict(out=np.full(total, FILL, np.uint8).repeat(16).view(pkg.capi.DMATCH_DTYPE),
                pts=np.full((total, 16), FILL, np.uint8).view(np.float32),
                results=np.full(len(pairs) * 88, FILL, np.uint8).view(pkg.capi.EPI_RESULT_DTYPE),
                mask=np.full(total, FILL, np.uint8),
                pose_results=np.full(len(pairs) * 128, FILL, np.uint8).view(pkg.capi.POSE_RESULT_DTYPE),
                pose_mask=np.full(total, FILL, np.uint8))
    with pytest.raises(pkg.LcmError) as e:
        m.pose_db_verify_pairs(pairs, 0.7, ep, cap=total - 1, **bufs)
    assert e.value.code == -4 and int(m.last_offsets[len(pairs)]) == total
    for a in bufs.values():
        assert (a.view(np.uint8) == FILL).all()
    for bad in (dict(ep=params(pkg, iters=96)), dict(ep=ep, pp=pkg.capi.default_pose_params(max_depth=0.0))):
        with pytest.raises(pkg.LcmError) as e:
            m.pose_db_verify_pairs(pairs, 0.7, **bad, **bufs)
        assert e.value.code == -1
        for a in bufs.values():
            assert (a.view(np.uint8) == FILL).all()
    # no pair: nothing to do; the calls around it return what they returned
    _, pe, *_x = m.pose_db_verify_pairs([(CURR, CURR)][:0], 0.7, ep)
    assert len(pe) == 0
    again = m.epi_db_verify_pairs(pairs, 0.7, ep)
    assert as_bytes(again[0]) == as_bytes(res0) and as_bytes(again[3]) == as_bytes(mask0) and m.launch_info().launches == info0.launches


def python_walk(res, pres, ep, pp_limit=100, floor=-1):
    """src/main.cpp:1403-1418 over the returned records."""
    return P.best_loop([(int(r["n_inliers"]), int(r["n_points"]), int(q["n_good"]), int(q["status"])) for r, q in zip(res, pres)], floor,
                       min_inliers=ep.min_inliers, min_ratio=ep.min_ratio, min_pose_inliers=pp_limit)


def test_store_detect_loops_and_the_best_loop(pkg, loop_store):
    m, frames, kps, shared, planted = loop_store
    ep = params(pkg)
    cands0, np0, res0, out0, pts0, mask0, offs0 = m.epi_db_detect_loops(CURR, 1, ep)
    info0 = m.launch_info()
    assert [int(c) for c in cands0["matched_frame_id"]] == [0, 1, 3]           # 100 shared rows are below the gate of 300
    cands, npairs, res, pres, out, pts, mask, pmask, offs, best = m.pose_db_detect_loops(CURR, 1, ep)
    info = m.launch_info()
    assert as_bytes(cands) == as_bytes(cands0) and npairs == np0 and as_bytes(res) == as_bytes(res0) and as_bytes(mask) == as_bytes(mask0)
    assert as_bytes(out) == as_bytes(out0) and as_bytes(pts) == as_bytes(pts0) and as_bytes(offs) == as_bytes(offs0)
    want, want_mask = m.pose_recover_pairs(pts0, offs0, res0["E"], ep, None, mask0)
    assert as_bytes(pres) == as_bytes(want) and as_bytes(pmask) == as_bytes(want_mask)
    check_against_reference(pres, pmask, pts0, offs0, res0["E"], mask0, P.MAX_DEPTH)
    assert info.launches == info0.launches + 1 and info.aux_kernel_ms > 0
    assert (info.workgroups, info.pairs, info.route) == (info0.workgroups, info0.pairs, info0.route)
    # the best loop against a Python walk of :1403-1418, and against lcm_pose_best
    assert all(pkg.capi.pose_loop_test(r, q, ep) for r, q in zip(res, pres))
    assert best == python_walk(res, pres, ep) == pkg.capi.pose_best(res, pres, ep) == int(np.argmax(res["n_inliers"]))
    top = int(res["n_inliers"].max())
    for floor in (top - 1, top, 0):
        *_, b = m.pose_db_detect_loops(CURR, 1, ep, None, floor)
        assert b == python_walk(res, pres, ep, 100, floor) == (-1 if floor >= top else best)
    strict = pkg.capi.default_pose_params(min_pose_inliers=int(pres[best]["n_good"]))      # the winner fails the pose test: the next one
    *_, b = m.pose_db_detect_loops(CURR, 1, ep, strict)
    assert b == python_walk(res, pres, ep, strict.min_pose_inliers) and b != best
    # the candidates do not fit: refused first, nothing new written
    with pytest.raises(pkg.LcmError) as e:
        m.pose_db_detect_loops(CURR, 1, ep, cand_cap=2)
    assert e.value.code == -4
    total = int(offs[-1])
    with pytest.raises(pkg.LcmError) as e:
        m.pose_db_detect_loops(CURR, 1, ep, cap=total - 1)
    assert e.value.code == -4 and int(m.last_offsets[3]) == total
    # the host-query form: the current frame's rows and points standing for position 4
    m.l2_db_truncate(CURR)
    try:
        c2, _, r2, q2, o2, p2, m2, pm2, f2, b2 = m.pose_db_detect_loops(CURR, 1, ep, query=frames[CURR], query_pts=kps[CURR])
        assert as_bytes(c2) == as_bytes(cands) and as_bytes(r2) == as_bytes(res) and as_bytes(m2) == as_bytes(mask)
        assert as_bytes(q2) == as_bytes(pres) and as_bytes(pm2) == as_bytes(pmask) and b2 == best
        assert as_bytes(o2) == as_bytes(out) and as_bytes(p2) == as_bytes(pts) and as_bytes(f2) == as_bytes(offs)
        # no candidate: nothing to recover, nothing launched for it, no best loop
        c3, _, r3, q3, o3, p3, m3, pm3, f3, b3 = m.pose_db_detect_loops(CURR, 1, ep, query=frames[CURR][:250], query_pts=kps[CURR][:250])
        assert len(c3) == 0 and len(q3) == 0 and len(pm3) == 0 and f3.tolist() == [0] and b3 == -1
    finally:
        assert m.l2_db_append_kp(frames[CURR], kps[CURR]) == CURR
    again = m.epi_db_detect_loops(CURR, 1, ep)
    assert as_bytes(again[2]) == as_bytes(res0) and as_bytes(again[5]) == as_bytes(mask0) and m.launch_info().launches == info0.launches


# ---- 6. slicing -----------------------------------------------------------------------------------------------------------
def test_seventy_thousand_pairs_make_two_slices(pkg, matcher):
    """70 000 pairs of 8 to 12 records, pair p under its own matrix: more pairs than gridDim.y holds, so the launch is sliced.
    Every pair's counts, choice, R, t and every mask byte are checked against numpy under the pair's own E."""
    pts, offs, E = S.many_pairs()
    n_pairs = len(offs) - 1
    res, mask = matcher.pose_recover_pairs(pts, offs, E, params(pkg))
    info = matcher.launch_info()
    assert info.launches == 2 and info.pairs == n_pairs
    lens = np.diff(offs.astype(np.int64))
    starts = offs[:-1].astype(np.int64)
    pair_of = np.repeat(np.arange(n_pairs), lens)
    ok, ra, rb, t = P.decompose(E)
    assert ok.all() and (res["status"] == 0).all()
    a, b, c, d = E_.normalise(pts)
    verdict = []
    for h in range(4):
        r = (rb if h & 1 else ra)[pair_of]
        tt = (-t if h & 2 else t)[pair_of]
        verdict.append(P.in_front([r[:, i] for i in range(9)], [tt[:, i] for i in range(3)], a, b, c, d))
    verdict = np.stack(verdict)
    counts = np.stack([np.add.reduceat(v.astype(np.int64), starts) for v in verdict], axis=1)
    choice = np.argmax(counts, axis=1)
    np.testing.assert_array_equal(res["counts"], counts)
    np.testing.assert_array_equal(res["choice"], choice)
    np.testing.assert_array_equal(res["n_used"], lens)
    np.testing.assert_array_equal(res["n_good"], counts[np.arange(n_pairs), choice])
    np.testing.assert_array_equal(mask, verdict[choice[pair_of], np.arange(len(pair_of))].astype(np.uint8))
    R = np.where((choice & 1)[:, None] == 1, rb, ra)
    T = np.where((choice & 2)[:, None] == 2, -t, t)
    assert as_bytes(res["R"]) == as_bytes(R) and as_bytes(res["t"]) == as_bytes(T)
    assert len(set(choice.tolist())) == 4 and (res["n_good"][-100:] > 0).any() and (res["n_good"][65536:] >= 6).any()
