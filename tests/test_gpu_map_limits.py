"""The map building on the device (include/lcm.h, lcm_map_*) ON its thresholds, at its documented limits and across its block
seams, on tests/maplimitcases.py's inputs (tests/test_map_limit_cases_host.py runs their assertions without a device).

A. Verdicts.  Every record with a point obeys mapref.status_of_fields on the DEVICE's own lcm_map_tri (no guard band, no record
left out); one parameter moved onto an accepted record's own rel, max(err1, err2) or cos_parallax keeps it accepted and the
neighbouring double rejects it, in lcm_map_triangulate_pairs and through lcm_map_add_keyframe; the keyframe gates at the device's
own median, n_good and n_good / n through lcm_map_add_keyframe and lcm_map_db_track.
B. Sizes.  Pairs of 65 535 / 65 536 / 65 537 records, LCM_MAP_MAX_PAIRS pairs in one launch, medians over a plateau of 66 000 equal
values and over 262 145 records, merges of 256, 257 and 1026 blocks, the map's point count up to 2^31 - 1, the chained calls at
65 535 matches.  Fields within MARGIN x the constants the host file measures on mapref alone (mapcases.OWN_*, and
maplimitcases.BIG_OWN_* / MANY_OWN_* where the new records' own rounding is larger); everything else exact."""
import ctypes as C

import numpy as np
import pytest

import l2emitcases as E
import mapcases as S
import maplimitcases as L
import mapref as M
import test_gpu_map as T
import verifylimitcases as V
from test_gpu_map import as_bytes, dmatches, epi_params, map_params, run_pairs

pytestmark = pytest.mark.gpu
FILL = T.FILL
K = S.K
track_store = T.track_store
OWN = dict(x=S.OWN_X_REL, d=S.OWN_DEPTH_REL, c=S.OWN_COS, e=S.OWN_ERR)
BIG_OWN = dict(x=L.BIG_OWN_X_REL, d=L.BIG_OWN_DEPTH_REL, c=L.BIG_OWN_COS, e=L.BIG_OWN_ERR)
MANY_OWN = dict(x=S.OWN_X_REL, d=S.OWN_DEPTH_REL, c=L.MANY_OWN_COS, e=L.MANY_OWN_ERR)


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def check_rule(tri, status, baseline, cosine, pp=None):
    """A1: every record whose device status is >= REJ_DEPTH has the status map_record's five lines give on its own fields."""
    has = status >= M.REJ_DEPTH
    rule = M.status_of_fields(tri, baseline, cosine, pp)
    assert np.array_equal(status[has], rule[has]), np.flatnonzero(has & (status != rule))[:8]
    assert not as_bytes(tri[~has]).strip(b"\0")


def check_fields(name, tri, want, own):
    """The device's lcm_map_tri against mapref's within MARGIN x the reference's own rounding; 1e9 where mapref has it."""
    scale = np.maximum(1.0, np.abs(want["X"]).max(1))
    dev = dict(x=float((np.abs(tri["X"] - want["X"]).max(1) / scale).max()),
               d=max(float((np.abs(tri[f] - want[f]) / np.maximum(1.0, np.abs(want[f]))).max()) for f in ("depth1", "depth2")),
               c=float(np.abs(tri["cos_parallax"] - want["cos_parallax"]).max()),
               e=max(float(np.abs(tri[f] - want[f]).max()) for f in ("err1", "err2")))
    print(name, len(tri), {k: f"{v:.1e}" for k, v in dev.items()})
    for f in ("err1", "err2"):
        assert np.array_equal(tri[f] == M.BEHIND, want[f] == M.BEHIND)
    for k in dev:
        assert dev[k] <= S.MARGIN * own[k], (name, k, dev[k], own[k])


# ---- A1. the rule on the device's own fields ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.pair_cases()))
def test_every_status_is_the_rule_on_the_devices_own_fields(pkg, matcher, name):
    case = S.pair_cases()[name]
    (tri, status, info), _ = run_pairs(pkg, matcher, [case], mask=None if case.mask is None else "own")
    want = case.records(cosine=float(info[0]["cos_min"])) if len(case.pts) else None
    if want is not None:
        check_rule(tri, status, float(info[0]["baseline"]), float(info[0]["cos_min"]), case.pp)
        for s in (M.NOT_INLIER, M.NO_POINT):
            assert np.array_equal(status == s, want.status == s)
        assert info[0]["counts"].tolist() == np.bincount(status, minlength=8).tolist()


# ---- A2. derived parameter sets -------------------------------------------------------------------------------------------------
def library_cosine(pkg, matcher):
    """deg -> the LIBRARY's info.cos_min, from a one-record call; remembered per deg."""
    case, seen = S.pair_cases()["n1"], {}

    def cos_of(deg):
        if deg not in seen:
            one = S.Pair("c", case.R1, case.t1, case.R2, case.t2, case.pts, None, dict(min_parallax_deg=deg))
            seen[deg] = float(run_pairs(pkg, matcher, [one], mask=None)[0][2][0]["cos_min"])
        return seen[deg]
    return cos_of


def parameter_sets(pkg, matcher, tri, status, info, pp):
    """[(edge, k, parameters, the status record k must get)]: the depth and reprojection edges, and min_parallax_deg on the records the
    library's own cosine hits exactly (at least three: maplimitcases.cosine_edges asserts it)."""
    base, cosine = float(info["baseline"]), float(info["cos_min"])
    out = []
    for d in L.derived_sets(tri, status, base, cosine, pp):
        out += [(d.edge, d.k, d.at, M.ACCEPTED), (d.edge, d.k, d.off, d.off_status)]
    for k, (at, off) in L.cosine_edges(library_cosine(pkg, matcher), tri, status).items():
        out += [("min_parallax_deg", k, dict(pp or {}, min_parallax_deg=at), M.ACCEPTED), ("min_parallax_deg", k, dict(pp or {}, min_parallax_deg=off), M.REJ_PARALLAX)]
    return out


@pytest.mark.parametrize("name", ["mixed", "wide"])
def test_a_parameter_on_a_records_own_value_and_on_the_neighbouring_double(pkg, matcher, name):
    case = S.pair_cases()[name]
    own = None if case.mask is None else "own"
    (tri0, status0, info0), _ = run_pairs(pkg, matcher, [case], mask=own)
    sets = parameter_sets(pkg, matcher, tri0, status0, info0[0], case.pp)
    assert {"min_depth", "max_depth", "max_reproj", "min_parallax_deg"} == {e for e, _, _, _ in sets} and len({k // 64 for _, k, _, _ in sets}) >= 2
    turned = 0
    for edge, k, pp, want in sets:
        moved = S.Pair(name, case.R1, case.t1, case.R2, case.t2, case.pts, case.mask, pp)
        (tri, status, info), _ = run_pairs(pkg, matcher, [moved], mask=own)
        assert as_bytes(tri) == as_bytes(tri0)                                  # the limits do not enter the arithmetic
        check_rule(tri, status, float(info[0]["baseline"]), float(info[0]["cos_min"]), pp)
        assert status[k] == want, (k, pp, status[k], want)
        assert info[0]["counts"].tolist() == np.bincount(status, minlength=8).tolist()
        assert np.array_equal(status <= M.NO_POINT, status0 <= M.NO_POINT)
        if edge == "min_parallax_deg":
            c = float(tri0["cos_parallax"][k])
            assert float(info[0]["cos_min"]) == (c if want == M.ACCEPTED else float(np.nextafter(c, -np.inf)))
        turned += want != M.ACCEPTED
    assert turned == len(sets) // 2 >= 12 + L.MIN_COSINE_HITS


@pytest.fixture(scope="module")
def first_keyframe(pkg, matcher):
    """Frame 1 of the trajectory added to a map in which every third keypoint of frame 0 has a point already, with the defaults;
    the records' lcm_map_tri from the public calls on the same lists (the pose stage's mask, the report's pose)."""
    c = pkg.capi
    tr = S.Trajectory()
    m, p = tr.matches(0, 1)
    mp, ep, lp = map_params(pkg), epi_params(pkg), c.default_lo_params()
    pose0 = c.pgo_poses(np.eye(3)[None], np.zeros((1, 3)))
    t1 = np.full(tr.n_points, -1, np.int32)
    t1[::3] = np.arange(len(t1[::3]))
    n_points = len(t1[::3])
    g1, g2 = t1.copy(), np.full(tr.n_points, -1, np.int32)
    rep, points, obs, status = matcher.map_add_keyframe(dmatches(pkg, m), p, 0, pose0, g1, 1, g2, n_points, mp, ep, lp=lp)
    assert rep.verdict == M.KEYFRAME and rep.n_new > 50 and rep.n_merged > 50
    res, _, mask = matcher.lo_verify_pairs(p, [0, len(p)], ep, lp)
    pres, pmask = matcher.pose_recover_pairs(p, [0, len(p)], res["E"], ep, mask_in=mask)
    pose1 = c.pgo_poses(np.array(rep.R).reshape(1, 3, 3), np.array(rep.t).reshape(1, 3))
    tri, st, info = matcher.map_triangulate_pairs(p, [0, len(p)], pose0, pose1, mp, pmask)
    return dict(tr=tr, m=m, p=p, mp=mp, ep=ep, lp=lp, pose0=pose0, pose1=pose1, t1=t1, n_points=n_points, rep=rep, points=points, obs=obs,
                status=status, tables=(g1, g2), tri=tri, tri_status=st, info=info[0], pres=pres[0], pmask=pmask)


def keyframe_statuses(f, tri_status):
    """What the merge makes of a triangulation's statuses: accepted -> NEW without a point in table_last, else MERGED."""
    acc = tri_status == M.ACCEPTED
    fresh = acc & (f["t1"][f["m"][:, 0]] == -1)
    return np.where(fresh, M.NEW, np.where(acc, M.MERGED, tri_status)).astype(np.uint8)


def test_the_derived_sets_through_add_keyframe(pkg, matcher, first_keyframe):
    f = first_keyframe
    assert np.array_equal(f["status"], keyframe_statuses(f, f["tri_status"]))                      # the composition names the report's records
    base, cosine = float(f["info"]["baseline"]), float(f["info"]["cos_min"])
    assert base == f["rep"].baseline
    sets = parameter_sets(pkg, matcher, f["tri"], f["tri_status"], f["info"], None)
    assert len(sets) >= 2 * (12 + L.MIN_COSINE_HITS)
    by_k = {}
    for edge, k, pp, want in sets:
        g1, g2 = f["t1"].copy(), np.full(len(f["t1"]), -1, np.int32)
        rep, points, obs, status = matcher.map_add_keyframe(dmatches(pkg, f["m"]), f["p"], 0, f["pose0"], g1, 1, g2, f["n_points"], map_params(pkg, **pp),
                                                            f["ep"], lp=f["lp"])
        assert rep.verdict == M.KEYFRAME and bytes(rep)[:112] == bytes(f["rep"])[:112]               # pose, median, baseline: not the limits' business
        has = f["tri_status"] >= M.REJ_DEPTH
        cos_now = cosine if edge != "min_parallax_deg" else library_cosine(pkg, matcher)(pp["min_parallax_deg"])
        rule = np.where(has, M.status_of_fields(f["tri"], base, cos_now, pp), f["tri_status"]).astype(np.uint8)
        want_status = keyframe_statuses(f, rule)
        assert np.array_equal(status, want_status) and status[k] == (want if want != M.ACCEPTED else f["status"][k]), (k, pp)
        counts = np.bincount(want_status, minlength=8)
        assert list(rep.counts) == counts.tolist() and (rep.n_new, rep.n_merged) == (counts[M.NEW], counts[M.MERGED]) and counts[M.ACCEPTED] == 0
        assert len(points) == rep.n_new and len(obs) == 2 * rep.n_new + rep.n_merged
        by_k.setdefault((k, edge), []).append((want, rep))
    for (k, edge), ((w_at, at), (w_off, off)) in by_k.items():                                          # the record that turns takes its count with it
        kind = int(f["status"][k])
        assert w_at == M.ACCEPTED and w_off != M.ACCEPTED and kind in (M.NEW, M.MERGED)
        assert at.counts[kind] - off.counts[kind] >= 1 and off.counts[w_off] - at.counts[w_off] == at.counts[kind] - off.counts[kind]
        assert (at.n_new - off.n_new, at.n_merged - off.n_merged) == ((at.counts[kind] - off.counts[kind], 0) if kind == M.NEW else (0, at.counts[kind] - off.counts[kind]))


# ---- A3. the gates on the device's own numbers ------------------------------------------------------------------------------------
def gates(median, n_good, n):
    """[(parameters at the threshold: a keyframe, parameters one step beyond, the verdict there)]"""
    ratio = n_good / n
    return [(dict(min_displacement=median), dict(min_displacement=float(np.nextafter(median, np.inf))), M.LITTLE_MOTION),
            (dict(max_displacement=median), dict(max_displacement=float(np.nextafter(median, -np.inf))), M.MUCH_MOTION),
            (dict(min_tracked=n), dict(min_tracked=n + 1), M.FEW_MATCHES),
            (dict(min_pose_inliers=n_good), dict(min_pose_inliers=n_good + 1), M.NO_POSE),
            (dict(min_inliers=n_good), dict(min_inliers=n_good + 1), M.FEW_INLIERS),
            (dict(min_inlier_ratio=ratio), dict(min_inlier_ratio=float(np.nextafter(ratio, np.inf))), M.FEW_INLIERS)]


def reference_verdict(n, median, n_good, pp):
    v = M.motion_verdict(n, median, pp)
    return v if v != M.KEYFRAME else M.pose_verdict(n, True, n_good, pp)


def raw_add_keyframe(pkg, matcher, f, matches, pts, mp, lp):
    """lcm_map_add_keyframe over pre-filled buffers: (rc, report, table_last, table_new, points, obs, status)."""
    n = len(pts)
    t1, t2 = f["t1"].copy(), np.full(len(f["t1"]), -1, np.int32)
    points, obs, status = np.full(24 * n, FILL, np.uint8), np.full(48 * n, FILL, np.uint8), np.full(n, FILL, np.uint8)
    rep = pkg.capi.MapKeyframeReport()
    rc = pkg.load_library().lcm_map_add_keyframe(matcher._h, vp(matches), vp(pts), n, 0, vp(f["pose0"]), vp(t1), len(t1), 1, vp(t2), len(t2), f["n_points"],
                                                 C.byref(mp), C.byref(f["ep"]), None if lp is None else C.byref(lp), None, vp(points), n, vp(obs), 2 * n,
                                                 vp(status), C.byref(rep))
    return rc, rep, t1, t2, points, obs, status


def test_the_gates_at_the_devices_own_numbers_through_add_keyframe(pkg, matcher, first_keyframe):
    f = first_keyframe
    dm, p, rep0 = dmatches(pkg, f["m"]), f["p"], f["rep"]
    n, n_good, median = rep0.n_matches, rep0.n_inliers, rep0.median
    assert n == len(p) and median == M.median(p) and n_good == int(f["pres"]["n_good"]) and 50 <= n_good < n
    for at, off, verdict in gates(median, n_good, n):
        assert reference_verdict(n, median, n_good, at) == M.KEYFRAME and reference_verdict(n, median, n_good, off) == verdict
        rc, rep, t1, t2, points, obs, status = raw_add_keyframe(pkg, matcher, f, dm, p, map_params(pkg, **at), f["lp"])
        assert rc == 0 and rep.verdict == M.KEYFRAME and bytes(rep) == bytes(rep0), at
        assert np.array_equal(t1, f["tables"][0]) and np.array_equal(t2, f["tables"][1]) and as_bytes(status) == as_bytes(f["status"])
        assert as_bytes(points[:24 * rep.n_new]) == as_bytes(f["points"]) and as_bytes(obs[:24 * (2 * rep.n_new + rep.n_merged)]) == as_bytes(f["obs"])
        assert (points[24 * rep.n_new:] == FILL).all() and (obs[24 * (2 * rep.n_new + rep.n_merged):] == FILL).all()
        before = bytes(matcher.launch_info())
        rc, rep, t1, t2, points, obs, status = raw_add_keyframe(pkg, matcher, f, dm, p, map_params(pkg, **off), f["lp"])
        assert rc == 0 and rep.verdict == verdict, (off, rep.verdict)
        assert (rep.n_new, rep.n_merged, rep.n_matches) == (0, 0, n) and not any(rep.R) and not any(rep.t) and not any(rep.counts)
        assert np.array_equal(t1, f["t1"]) and (t2 == -1).all() and all((x == FILL).all() for x in (points, obs, status))
        assert rep.median == (0.0 if verdict == M.FEW_MATCHES else median) and rep.n_inliers == (n_good if verdict == M.FEW_INLIERS else 0)
        if verdict == M.FEW_MATCHES:
            assert bytes(matcher.launch_info()) == before                          # decided from the count: nothing was launched


def test_eight_records_are_not_refused_for_their_number(pkg, matcher, first_keyframe):
    """min_tracked = 0 and min_displacement = 0 let a list of 7 and of 8 records through to the pose gate (max_displacement out of
    the way too), every inlier gate at 0:
    7 records are LCM_MAP_NO_POSE (n < 8); 8 records get what mapref.pose_verdict says on the pose stage's public output."""
    f = first_keyframe
    over = dict(min_tracked=0, min_displacement=0.0, max_displacement=1e9, min_pose_inliers=0, min_inliers=0, min_inlier_ratio=0.0)
    mp = map_params(pkg, **over)
    good = np.flatnonzero(f["pmask"] != 0)[:8]                                      # eight inliers of the full list's pose
    dm, p = dmatches(pkg, f["m"][good]), np.ascontiguousarray(f["p"][good])
    rc, rep, t1, t2, points, obs, status = raw_add_keyframe(pkg, matcher, f, dm[:7], p[:7], mp, f["lp"])
    assert rc == 0 and rep.verdict == M.NO_POSE and rep.n_inliers == 0 and np.array_equal(t1, f["t1"]) and (t2 == -1).all()
    assert all((x == FILL).all() for x in (points, obs, status)) and rep.median == M.median(p[:7])
    res, _, mask = matcher.lo_verify_pairs(p, [0, 8], f["ep"], f["lp"])
    pres, pmask = matcher.pose_recover_pairs(p, [0, 8], res["E"], f["ep"], mask_in=mask)
    ok, n_good = int(pres[0]["status"]) == pkg.capi.POSE_OK, int(pres[0]["n_good"])
    want = M.pose_verdict(8, ok, n_good, over)
    rc, rep, t1, t2, points, obs, status = raw_add_keyframe(pkg, matcher, f, dm, p, mp, f["lp"])
    print("eight records: pose ok", ok, "n_good", n_good, "verdict", rep.verdict)
    assert rc == 0 and rep.verdict == want and (want == M.KEYFRAME) == ok and rep.n_inliers == (n_good if ok else 0)
    if ok:
        assert not (status == FILL).any() and (status[pmask == 0] == M.NOT_INLIER).all() and rep.n_new + rep.n_merged == (status >= M.MERGED).sum()


def test_the_gates_at_the_devices_own_numbers_through_db_track(pkg, track_store):
    c = pkg.capi
    m, frames, kps = track_store
    ep = epi_params(pkg)
    pose0 = c.pgo_poses(np.eye(3)[None], np.zeros((1, 3)))
    t1 = np.full(300, -1, np.int32)
    t1[5::7] = np.arange(len(t1[5::7]))
    n_points = len(t1[5::7])

    def track(**over):
        g1, g2 = t1.copy(), np.full(300, -1, np.int32)
        lists, rep, points, obs, status = m.map_db_track(0, 2, 0.75, 0, pose0, g1, 1, g2, n_points, map_params(pkg, **over), ep)
        return rep, (as_bytes(points), as_bytes(obs), as_bytes(status), as_bytes(g1), as_bytes(g2)), g1, g2, status

    rep0, bytes0, _, g2, _ = track()
    n, n_good, median = rep0.n_matches, rep0.n_inliers, rep0.median
    assert rep0.verdict == M.KEYFRAME and n >= 270 and 50 <= n_good < n and not (g2 == -1).all()
    for at, off, verdict in gates(median, n_good, n):
        rep, got, _, _, _ = track(**at)
        assert rep.verdict == M.KEYFRAME and bytes(rep) == bytes(rep0) and got == bytes0, at
        rep, got, g1, g2, status = track(**off)
        assert rep.verdict == verdict == reference_verdict(n, median, n_good, off), (off, rep.verdict)
        assert (rep.n_new, rep.n_merged, rep.n_matches) == (0, 0, n) and not any(rep.R) and not any(rep.counts)
        assert np.array_equal(g1, t1) and (g2 == -1).all() and not status.any() and got[0] == b"" and got[1] == b""
        assert rep.median == (0.0 if verdict == M.FEW_MATCHES else median) and rep.n_inliers == (n_good if verdict == M.FEW_INLIERS else 0)


# ---- B1. triangulation at its sizes -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_runs(pkg, matcher):
    return {}


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", L.BIG_LENS)
def test_one_pair_of_65535_to_65537_records(pkg, matcher, n, masked):
    pair, want_tri, want_status = L.big_pair(n, masked)
    (tri, status, info), offs = run_pairs(pkg, matcher, [pair], mask="own" if masked else None)
    li = matcher.launch_info()
    assert len(tri) == n and li.launches == 1 and li.pairs == n and li.workgroups == -(-n // L.BLOCK) == (257 if n == 65537 else 256)
    base, cosine = float(info[0]["baseline"]), float(info[0]["cos_min"])
    assert base == float(pair.plan().baseline) and abs(cosine - M.cos_min(1.0)) <= 2.3e-16
    check_rule(tri, status, base, cosine)
    for s in (M.NOT_INLIER, M.NO_POINT):
        assert np.array_equal(status == s, want_status == s)
    assert status[-1] == M.ACCEPTED and info[0]["counts"].tolist() == np.bincount(status, minlength=8).tolist() and (info[0]["counts"][1:6] > 0).all()
    check_fields(pair.name, tri, want_tri, BIG_OWN)
    # the restatement's statuses, wherever its own record is the guard's distance clear of every threshold: all but a handful
    clear = S.clear_of_thresholds(L.big_source()[1], pair.plan(cosine), None)[:n]
    print("records within the guard of a threshold:", int((~clear).sum()), "status differs on", int((status != want_status).sum()))
    assert np.array_equal(status[clear], want_status[clear]) and (~clear).sum() < 200


def test_4096_pairs_in_one_launch(pkg, matcher):
    mp = L.many_pairs()
    c = pkg.capi
    p1, p2 = c.pgo_poses(mp.R1, mp.t1), c.pgo_poses(mp.R2, mp.t2)
    tri, status, info = matcher.map_triangulate_pairs(mp.pts, mp.offsets, p1, p2, map_params(pkg), mp.mask)
    li = matcher.launch_info()
    assert li.launches == 1 and li.pairs == int(mp.offsets[-1]) and li.workgroups == 2 * L.MAX_PAIRS       # grid x = ceil(300 / 256)
    assert np.array_equal(status, mp.status), np.flatnonzero(status != mp.status)[:8]
    assert np.array_equal(info["counts"], mp.counts) and np.array_equal(info["baseline"], mp.baseline)
    base = np.repeat(info["baseline"], np.diff(mp.offsets.astype(np.int64)))
    check_rule(tri, status, base, float(info[0]["cos_min"]))
    check_fields("4096 pairs", tri, mp.tri, MANY_OWN)
    tri2, status2, info2 = matcher.map_triangulate_pairs(mp.pts, mp.offsets, p1, p2, map_params(pkg), mp.mask)
    assert as_bytes(tri) == as_bytes(tri2) and as_bytes(status) == as_bytes(status2) and as_bytes(info) == as_bytes(info2)
    # the same offsets through the median
    got = matcher.map_median_displacement(mp.pts, mp.offsets)
    offs = mp.offsets.astype(np.int64)
    want = np.array([np.sort(M.displacements(mp.pts[offs[p]:offs[p + 1]]))[(offs[p + 1] - offs[p]) // 2] if offs[p + 1] > offs[p] else 0.0 for p in range(L.MAX_PAIRS)])
    assert as_bytes(got) == as_bytes(want) and (got > 0).sum() > 1000
    li = matcher.launch_info()
    assert li.launches == 1 and li.workgroups == L.MAX_PAIRS and li.pairs == int(mp.offsets[-1])


# ---- B2. the median -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plateau_inside", "plateau_above", "uniform262145"])
def test_median_over_a_plateau_and_over_262145_records(matcher, name):
    pts, want = L.uniform_pair() if name == "uniform262145" else L.plateau_pair(name == "plateau_above")
    got = matcher.map_median_displacement(pts, [0, len(pts)])
    assert as_bytes(got) == as_bytes(np.array([np.sort(M.displacements(pts))[len(pts) // 2]])) and got[0] == want
    assert as_bytes(matcher.map_median_displacement(pts, [0, len(pts)])) == as_bytes(got)


# ---- B3. the merge ------------------------------------------------------------------------------------------------------------
def run_merge(pkg, matcher, c, **caps):
    g1, g2 = c.table1.copy(), c.table2.copy()
    points, obs, out, n_new, n_merged = matcher.map_merge(dmatches(pkg, c.matches), c.pts, c.tri, c.status, 4, 5, g1, g2, c.n_points, **caps)
    return points, obs, out, g1, g2, n_new, n_merged


@pytest.mark.parametrize("name", ["dense65535", "dense65537", "dense262401", "seam262401", "blocks262401", "top65537"])
def test_merge_at_256_257_and_1026_blocks(pkg, matcher, name):
    c = L.merge_cases()[name]
    want, n = c.want, len(c.matches)
    points, obs, out, g1, g2, n_new, n_merged = run_merge(pkg, matcher, c)
    li = matcher.launch_info()
    assert li.launches == 4 and li.pairs == n and li.workgroups == -(-n // L.BLOCK)
    fresh = want[2] == M.NEW
    assert (n_new, n_merged) == (int(fresh.sum()), int((want[2] == M.MERGED).sum()))
    assert np.array_equal(out, want[2]), np.flatnonzero(out != want[2])[:8]
    assert as_bytes(points) == as_bytes(c.tri["X"][fresh]) == as_bytes(want[0])                    # byte-equal to the records' X
    assert as_bytes(obs) == as_bytes(L.obs_array(want[1], pkg.capi.BA_OBS_DTYPE))
    assert np.array_equal(g1, want[3]) and np.array_equal(g2, want[4])
    scan = L.merge_scan_of(name)                                                  # the second witness
    assert as_bytes(points) == as_bytes(scan[0]) and as_bytes(obs) == as_bytes(L.obs_array(scan[1], pkg.capi.BA_OBS_DTYPE))
    assert np.array_equal(out, scan[2]) and np.array_equal(g1, scan[3]) and np.array_equal(g2, scan[4])
    for train, last in L.last_writer(c):                                          # the last in list order wins
        assert g2[train] == g1[c.matches[last, 0]]
    if name == "top65537":
        assert c.n_points + n == L.INT_MAX and obs["point"].max() == g1.max() == c.n_points + n_new - 1 <= L.INT_MAX - 1
        carried = np.flatnonzero(c.table1 >= c.n_points - 3)
        assert len(carried) >= 4 and np.array_equal(g1[carried], c.table1[carried]) and ((g2 >= c.n_points - 3) & (g2 < c.n_points)).sum() >= 2
    if name == "seam262401":
        assert np.flatnonzero(out >= M.MERGED).tolist() == list(L.SEAM_RECORDS) and (n_new, n_merged) == (6, 6)
    again = run_merge(pkg, matcher, c)
    assert all(as_bytes(x) == as_bytes(y) for x, y in zip(again[:5], (points, obs, out, g1, g2))) and matcher.launch_info().launches == 4


def test_merge_refusals_at_the_point_limit_and_one_short_at_262401(pkg, matcher):
    lib, h = pkg.load_library(), matcher._h
    a, b = C.c_int32(-7), C.c_int32(-7)

    def call(c, n_pts, cap_points, cap_obs, bufs):
        g1, g2 = c.table1.copy(), c.table2.copy()
        dm = dmatches(pkg, c.matches)
        rc = lib.lcm_map_merge(h, vp(dm), vp(c.pts), vp(c.tri), vp(c.status), len(dm), 4, 5, vp(g1), len(g1), vp(g2), len(g2), n_pts, vp(bufs[0]), cap_points,
                               vp(bufs[1]), cap_obs, vp(bufs[2]), C.byref(a), C.byref(b))
        return rc, g1, g2

    # n_points + n = 2^31: refused, nothing written, nothing counted
    top = L.merge_cases()["top65537"]
    n = len(top.matches)
    bufs = [np.full(24 * n, FILL, np.uint8), np.full(48 * n, FILL, np.uint8), np.full(n, FILL, np.uint8)]
    rc, g1, g2 = call(top, top.n_points + 1, n, 2 * n, bufs)
    assert rc == -4 and (a.value, b.value) == (-7, -7) and np.array_equal(g1, top.table1) and np.array_equal(g2, top.table2)
    assert all((x == FILL).all() for x in bufs)
    # one short on either buffer at 1026 blocks: the counts are reported, nothing else
    c = L.merge_cases()["dense262401"]
    n = len(c.matches)
    n_new, n_merged = int((c.want[2] == M.NEW).sum()), int((c.want[2] == M.MERGED).sum())
    n_obs = 2 * n_new + n_merged
    bufs = [np.full(24 * n_new, FILL, np.uint8), np.full(24 * n_obs, FILL, np.uint8), np.full(n, FILL, np.uint8)]
    for caps in ((n_new - 1, n_obs), (n_new, n_obs - 1)):
        rc, g1, g2 = call(c, c.n_points, *caps, bufs)
        assert rc == -4 and (a.value, b.value) == (n_new, n_merged) and np.array_equal(g1, c.table1) and np.array_equal(g2, c.table2)
        assert all((x == FILL).all() for x in bufs)
        a.value = b.value = -7
    rc, g1, g2 = call(c, c.n_points, n_new, n_obs, bufs)                            # a following good call: a fresh one's bytes
    assert rc == 0 and as_bytes(bufs[0]) == as_bytes(c.want[0]) and as_bytes(bufs[1]) == as_bytes(L.obs_array(c.want[1], pkg.capi.BA_OBS_DTYPE))
    assert np.array_equal(bufs[2], c.want[2]) and np.array_equal(g1, c.want[3]) and np.array_equal(g2, c.want[4])


# ---- B4. the chained calls at 65 535 matches ----------------------------------------------------------------------------------
def test_add_keyframe_at_65535_matches_is_the_composition_of_the_public_calls(pkg, matcher):
    c = pkg.capi
    tr = L.trajectory()
    m, p = tr.matches(0, 1)
    n = len(p)
    assert n == L.MAX_MATCHES == tr.n_points
    mp, ep, lp = map_params(pkg), epi_params(pkg), c.default_lo_params()
    pose0 = c.pgo_poses(np.eye(3)[None], np.zeros((1, 3)))
    t1 = np.full(n, -1, np.int32)
    t1[2::5] = np.arange(len(t1[2::5]))
    n_points = len(t1[2::5])
    dm = dmatches(pkg, m)
    g1, g2 = t1.copy(), np.full(n, -1, np.int32)
    rep, points, obs, status = matcher.map_add_keyframe(dm, p, 0, pose0, g1, 1, g2, n_points, mp, ep, lp=lp)
    assert rep.verdict == M.KEYFRAME and rep.n_matches == n and rep.median == M.median(p) and 50 < rep.median < 65
    # the public calls on the same lists
    res, _, mask = matcher.lo_verify_pairs(p, [0, n], ep, lp)
    pres, pmask = matcher.pose_recover_pairs(p, [0, n], res["E"], ep, mask_in=mask)
    assert int(pres[0]["status"]) == c.POSE_OK and rep.n_inliers == int(pres[0]["n_good"]) == int((pmask != 0).sum()) > 50000
    Rn, tn = M.new_pose(pres[0]["R"], pres[0]["t"], pose0["R"][0], pose0["t"][0])
    assert as_bytes(Rn) == as_bytes(np.array(rep.R)) and as_bytes(tn) == as_bytes(np.array(rep.t))
    pose1 = c.pgo_poses(Rn[None], tn[None])
    tri, st, info = matcher.map_triangulate_pairs(p, [0, n], pose0, pose1, mp, pmask)
    check_rule(tri, st, float(info[0]["baseline"]), float(info[0]["cos_min"]))
    assert float(info[0]["baseline"]) == rep.baseline and np.array_equal(st == M.NOT_INLIER, pmask == 0)
    h1, h2 = t1.copy(), np.full(n, -1, np.int32)
    points2, obs2, status2, n_new, n_merged = matcher.map_merge(dm, p, tri, st, 0, 1, h1, h2, n_points)
    assert (rep.n_new, rep.n_merged) == (n_new, n_merged) and n_new > 30000 and n_merged > 8000
    assert as_bytes(points) == as_bytes(points2) and as_bytes(obs) == as_bytes(obs2) and as_bytes(status) == as_bytes(status2)
    assert np.array_equal(g1, h1) and np.array_equal(g2, h2)
    counts = np.bincount(status2, minlength=8)
    assert list(rep.counts) == counts.tolist() and counts[M.ACCEPTED] == 0 and counts[M.NOT_INLIER] >= 2900
    # ... and the Python loop fed with the pose stage's public output, as the six-keyframe replay is
    pose = (True, int(pres[0]["n_good"]), pres[0]["R"], pres[0]["t"], pmask)
    want = M.add_keyframe(K, m, p, 0, pose0["R"][0], pose0["t"][0], t1, 1, np.full(n, -1, np.int32), n_points, pose, float(info[0]["cos_min"]))
    assert want["verdict"] == M.KEYFRAME and want["median"] == rep.median and want["n_inliers"] == rep.n_inliers
    assert as_bytes(want["R"]) == as_bytes(np.array(rep.R)) and float(want["plan"].baseline) == rep.baseline
    clear = S.clear_of_thresholds(want["records"], want["plan"], None)
    print("add_keyframe at 65535: n_new", rep.n_new, "n_merged", rep.n_merged, "records within the guard", int((~clear).sum()))
    assert (~clear).sum() < 200 and np.array_equal(st[clear], want["records"].status[clear])
    acc = (st == M.ACCEPTED) & (want["records"].status == M.ACCEPTED)                # the map's points: the same scene's accepted records
    scale = np.maximum(1.0, np.abs(want["records"].X[acc]).max(1))
    assert acc.sum() > 50000 and (np.abs(tri["X"][acc] - want["records"].X[acc]).max(1) / scale).max() <= S.MARGIN * L.BIG_OWN_X_REL
    if np.array_equal(st, want["records"].status):                                # no record on the other side of a threshold: the whole map
        assert np.array_equal(status, want["status"]) and np.array_equal(g1, want["table_last"]) and np.array_equal(g2, want["table_new"])
        assert as_bytes(obs) == as_bytes(L.obs_array(want["obs"], c.BA_OBS_DTYPE)) and list(rep.counts) == want["counts"].tolist()
    # 65 536 matches: refused over pre-filled buffers
    f = dict(t1=np.full(n + 1, -1, np.int32), pose0=pose0, n_points=0, ep=ep)
    more_m = np.concatenate([m, [[n, 0]]]).astype(np.int32)
    more_p = np.ascontiguousarray(np.concatenate([p, p[:1]]))
    rc, rep2, r1, r2, pb, ob, sb = raw_add_keyframe(pkg, matcher, f, dmatches(pkg, more_m), more_p, mp, lp)
    assert rc == -4 and (r1 == -1).all() and (r2 == -1).all() and all((x == FILL).all() for x in (pb, ob, sb)) and not bytes(rep2).strip(b"\0")


def test_db_track_over_the_65535_row_frames_is_the_composition(pkg):
    """lcm_map_db_track on the stored pair (C, P) of l2emitcases.py, whose point records are verifylimitcases.big() bit for bit,
    against lcm_pose_db_verify_pairs and lcm_map_add_keyframe on the returned lists.  Override: min_inlier_ratio = 0.0 (the best of
    the 64 hypotheses holds 14 867 of the 65 535 records, below the default 0.3); the composition claim does not depend on it.
    The scene's camera is epiref's."""
    import epiref as R
    c = pkg.capi
    s = E.copy_store()
    n = E.N
    ep = c.default_epi_params(R.FX, R.FY, R.CX, R.CY, iters=V.ITERS)
    mp = c.default_map_params(fx=R.FX, fy=R.FY, cx=R.CX, cy=R.CY, min_inlier_ratio=0.0)
    pose0 = c.pgo_poses(np.eye(3)[None], np.zeros((1, 3)))
    t1 = np.full(n, -1, np.int32)
    t1[1::4] = np.arange(len(t1[1::4]))
    n_points = len(t1[1::4])
    m = pkg.Matcher()
    try:
        assert m.l2_db_append_kp(s.frames[E.SLOT_P], s.kps[E.SLOT_P]) == 0 and m.l2_db_append_kp(s.frames[E.SLOT_C], s.kps[E.SLOT_C]) == 1
        g1, g2 = t1.copy(), np.full(n, -1, np.int32)
        lists, rep, points, obs, status = m.map_db_track(1, 0, 0.7, 0, pose0, g1, 1, g2, n_points, mp, ep)
        res, pres, out, pts, mask, pmask, offs = m.pose_db_verify_pairs([(1, 0)], 0.7, ep)
        for got, want in ((lists["results"], res), (lists["pose_results"], pres), (lists["out"], out), (lists["pts"], pts), (lists["mask"], mask),
                          (lists["pose_mask"], pmask), (lists["offsets"], offs)):
            assert as_bytes(got) == as_bytes(want)
        assert int(offs[1]) == n and as_bytes(pts) == as_bytes(V.big()[0]) and np.array_equal(out["train_idx"], s.perm)
        h1, h2 = t1.copy(), np.full(n, -1, np.int32)
        rep2, points2, obs2, status2 = m.map_add_keyframe(out, pts, 0, pose0, h1, 1, h2, n_points, mp, ep)
        assert bytes(rep) == bytes(rep2) and as_bytes(points) == as_bytes(points2) and as_bytes(obs) == as_bytes(obs2) and as_bytes(status) == as_bytes(status2)
        assert np.array_equal(g1, h1) and np.array_equal(g2, h2)
        print("db_track at 65535 rows: verdict", rep.verdict, "median", rep.median, "n_inliers", rep.n_inliers, "new", rep.n_new, "merged", rep.n_merged)
        assert rep.verdict == M.KEYFRAME and rep.n_matches == n and rep.median == M.median(pts) and rep.n_inliers == int(pres[0]["n_good"])
        assert rep.n_new > 0 and rep.n_merged > 0 and rep.n_new + rep.n_merged == (status >= M.MERGED).sum() and (g2 != -1).any()
        assert list(rep.counts) == np.bincount(status, minlength=8).tolist()
    finally:
        m.close()
