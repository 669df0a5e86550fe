"""The map building before the loop on the device (include/lcm.h, lcm_map_*) against tests/mapref.py over tests/mapcases.py:
statuses and per-pair counts exactly (no record is left out: test_map_ref_host.py shows every record clear of every threshold), the
lcm_map_tri fields within MARGIN x the restatement's own rounding and all zero where stated; the median bit for bit numpy's; the
merge's points byte-equal to the records' X and its observations, tables, statuses and counts exact; lcm_map_add_keyframe on a
planted six-keyframe trajectory replayed against the Python loop, every verdict provoked once with the map's bytes unchanged, the
resulting map accepted by lcm_ba_error; lcm_map_db_track byte for byte the composition of lcm_pose_db_verify_pairs and
lcm_map_add_keyframe; two identical calls give identical bytes; refusals leave the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

import mapcases as S
import mapref as M

pytestmark = pytest.mark.gpu
FILL = 0xA7
K = S.K


def as_bytes(a):
    return np.ascontiguousarray(a).tobytes()


def map_params(pkg, **over):
    return pkg.capi.default_map_params(fx=K[0], fy=K[1], cx=K[2], cy=K[3], **over)


def poses_of(pkg, pairs):
    c = pkg.capi
    return (c.pgo_poses(np.stack([p.R1 for p in pairs]), np.stack([p.t1 for p in pairs])),
            c.pgo_poses(np.stack([p.R2 for p in pairs]), np.stack([p.t2 for p in pairs])))


def run_pairs(pkg, m, pairs, mask="own"):
    pts, offs, own = S.pack(pairs)
    p1, p2 = poses_of(pkg, pairs)
    assert all(p.pp == pairs[0].pp for p in pairs)
    return m.map_triangulate_pairs(pts, offs, p1, p2, map_params(pkg, **pairs[0].pp), None if mask is None else own), offs


def check_records(tri, status, info, case):
    """One pair's device records against the restatement under the LIBRARY's cos_min: statuses and counts exact, the fields
    within MARGIN x OWN_* (relative where the constant is), exactly zero without a point."""
    want = case.records(cosine=float(info["cos_min"]))
    assert abs(float(info["cos_min"]) - M.cos_min(M.params(case.pp)["min_parallax_deg"])) <= 2.3e-16        # an ulp of a value below 1
    assert float(info["baseline"]) == float(case.plan().baseline)
    assert np.array_equal(status, want.status), (case.name, np.flatnonzero(status != want.status)[:8])
    assert info["counts"].tolist() == want.counts().tolist() and info["counts"][6:].tolist() == [0, 0]
    none = ~want.has
    assert not as_bytes(tri[none]).strip(b"\0")
    scale = np.maximum(1.0, np.abs(want.X).max(1)) if len(want.X) else np.zeros(0)
    dev = dict(x=0.0, d=0.0, c=0.0, e=0.0)
    if len(tri):
        dev["x"] = float((np.abs(tri["X"] - want.X).max(1) / scale).max())
        dev["d"] = max(float((np.abs(tri[f] - getattr(want, f)) / np.maximum(1.0, np.abs(getattr(want, f)))).max()) for f in ("depth1", "depth2"))
        dev["c"] = float(np.abs(tri["cos_parallax"] - want.cos_parallax).max())
        dev["e"] = max(float(np.abs(tri[f] - getattr(want, f)).max()) for f in ("err1", "err2"))
        for f in ("err1", "err2"):
            assert np.array_equal(tri[f] == M.BEHIND, getattr(want, f) == M.BEHIND)
    print(case.name, len(tri), {k: f"{v:.1e}" for k, v in dev.items()})
    assert dev["x"] <= S.MARGIN * S.OWN_X_REL and dev["d"] <= S.MARGIN * S.OWN_DEPTH_REL, (case.name, dev)
    assert dev["c"] <= S.MARGIN * S.OWN_COS and dev["e"] <= S.MARGIN * S.OWN_ERR, (case.name, dev)


# ---- 1. triangulation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [f"n{n}" for n in S.SIZES] + ["mixed", "no_mask", "all_masked", "same_centre", "wide"] + [f"only{s}" for s in range(1, 6)])
def test_one_pair(pkg, matcher, name):
    case = S.pair_cases()[name]
    (tri, status, info), offs = run_pairs(pkg, matcher, [case], mask=None if case.mask is None else "own")
    assert len(tri) == len(case.pts) == int(offs[1]) and len(info) == 1
    check_records(tri, status, info[0], case)
    li = matcher.launch_info()
    assert li.pairs == len(case.pts) and li.launches == (1 if len(case.pts) else 0) and (li.kernel_ms > 0 or not len(case.pts))
    if name == "same_centre":
        assert float(info[0]["baseline"]) == 0.0 and (status == M.REJ_DEPTH).all() and not tri["depth1"].any() and (tri["err1"] == M.BEHIND).all()
    if name == "mixed":
        assert (info[0]["counts"][:6] > 0).all()                                  # every status occurs


def test_many_pairs_in_one_launch_with_empty_pairs_between(pkg, matcher):
    pairs = [p for p in S.many_pairs() if not p.pp] + [p for p in S.many_pairs() if not p.pp][:2]
    assert sum(len(p.pts) == 0 for p in pairs) >= 3 and len(pairs) >= 9
    (tri, status, info), offs = run_pairs(pkg, matcher, pairs)
    assert matcher.launch_info().launches == 1 and matcher.launch_info().pairs == int(offs[-1])
    for k, p in enumerate(pairs):
        lo, hi = int(offs[k]), int(offs[k + 1])
        check_records(tri[lo:hi], status[lo:hi], info[k], p)
    # the same call gives the same bytes; mask = NULL makes every record take part
    (tri2, status2, info2), _ = run_pairs(pkg, matcher, pairs)
    assert as_bytes(tri) == as_bytes(tri2) and as_bytes(status) == as_bytes(status2) and as_bytes(info) == as_bytes(info2)
    (tri3, status3, info3), _ = run_pairs(pkg, matcher, pairs, mask=None)
    assert not (status3 == M.NOT_INLIER).any() and info3["counts"][:, 0].sum() == 0
    keep = np.concatenate([np.ones(len(p.pts), bool) if p.mask is None else p.mask != 0 for p in pairs])
    assert as_bytes(tri3[keep]) == as_bytes(tri[keep]) and np.array_equal(status3[keep], status[keep])


def test_triangulation_refusals_leave_the_outputs_untouched(pkg, matcher):
    lib, h = pkg.load_library(), matcher._h
    case = S.pair_cases()["n65"]
    pts, offs, mask = S.pack([case])
    p1, p2 = poses_of(pkg, [case])
    mp = map_params(pkg)
    tri, status, info = np.full(65 * 64, FILL, np.uint8), np.full(65, FILL, np.uint8), np.full(48, FILL, np.uint8)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)          # noqa: E731

    def call(pts=pts, offs=offs, n=1, p1=p1, p2=p2, mp=mp, tri=tri, status=status, info=info):
        return lib.lcm_map_triangulate_pairs(h, vp(pts), vp(offs), n, vp(mask), vp(p1), vp(p2), None if mp is None else C.byref(mp), vp(tri), vp(status), vp(info))

    skew = p2.copy()
    skew["R"][0, 4] = 0.5
    for bad in (dict(mp=None), dict(mp=pkg.capi.default_map_params()), dict(pts=None), dict(offs=None), dict(p1=None), dict(p2=skew), dict(tri=None),
                dict(status=None), dict(info=None), dict(n=-1), dict(offs=np.array([0, 65, 64], np.uintp), n=2), dict(offs=np.array([1, 65], np.uintp))):
        assert call(**bad) == -1, bad
    assert call(n=4097) == -4 and call(offs=np.array([0, (1 << 24) + 1], np.uintp)) == -4
    med = np.full(8, FILL, np.uint8)
    assert lib.lcm_map_median_displacement(h, None, vp(offs), 1, vp(med)) == -1 and lib.lcm_map_median_displacement(h, vp(pts), vp(offs), 1, None) == -1
    assert lib.lcm_map_median_displacement(h, vp(pts), vp(offs), 4097, vp(med)) == -4
    for a in (tri, status, info, med):
        assert (a == FILL).all()
    assert call() == 0 and not (status == FILL).all()
    assert lib.lcm_map_triangulate_pairs(h, None, vp(np.zeros(1, np.uintp)), 0, None, None, None, C.byref(mp), None, None, None) == 0        # no pair


# ---- 2. the median ------------------------------------------------------------------------------------------------------------
def test_median_is_bit_for_bit_numpys(matcher):
    rng = np.random.default_rng(7)
    pairs = [rng.uniform(0, 1280, (n, 4)).astype(np.float32) for n in (0, 1, 2, 3, 64, 65)]
    same = np.tile(np.array([[10.0, 20.0, 13.0, 24.0]], np.float32), (100, 1))                         # all values equal: 5.0
    ties = np.zeros((9, 4), np.float32)
    ties[:, 2] = [1, 2, 3, 3, 3, 3, 3, 8, 9]                                                            # ties around the middle
    even = np.zeros((8, 4), np.float32)
    even[:, 3] = [7, 1, 5, 5, 2, 5, 9, 0.5]
    tiny = np.zeros((5, 4), np.float32)
    tiny[:, 2] = [0.0, 1e-30, 1e-38, 1e-45, 2e-45]                                                      # zeros and denormal differences
    pairs += [same, ties, even, tiny]
    pairs += [rng.uniform(0, 640, (int(n), 4)).astype(np.float32) for n in rng.integers(0, 700, 300)]   # 300 pairs of mixed sizes
    pairs[20][:, :] = pairs[20][:1, :]
    offs = np.concatenate([[0], np.cumsum([len(p) for p in pairs])]).astype(np.uintp)
    got = matcher.map_median_displacement(np.concatenate(pairs), offs)
    want = np.array([np.sort(M.displacements(p))[len(p) // 2] if len(p) else 0.0 for p in pairs])
    assert as_bytes(got) == as_bytes(want)
    assert got[6] == 5.0 and got[7] == 3.0 and got[8] == 5.0 and got[0] == 0.0
    li = matcher.launch_info()
    assert li.launches == 1 and li.pairs == int(offs[-1]) and li.kernel_ms > 0
    assert as_bytes(matcher.map_median_displacement(np.concatenate(pairs), offs)) == as_bytes(got)


def test_median_of_one_pair_of_65535_records(matcher):
    rng = np.random.default_rng(8)
    pts = rng.uniform(0, 2000, (65535, 4)).astype(np.float32)
    pts[1000:30000, 2:] = pts[1000:30000, :2] + np.float32(3.0)                  # 29 000 equal values below the middle
    got = matcher.map_median_displacement(pts, [0, 65535])
    assert as_bytes(got) == as_bytes(np.array([np.sort(M.displacements(pts))[65535 // 2]]))


# ---- 3. the merge -------------------------------------------------------------------------------------------------------------
def dmatches(pkg, m):
    dm = np.zeros(len(m), pkg.capi.DMATCH_DTYPE)
    if len(m):
        dm["query_idx"], dm["train_idx"] = m[:, 0], m[:, 1]
    return dm


def check_merge(pkg, matcher, lists, kf1=4, kf2=5):
    m, pts, tri, status, t1, t2, n_points = lists
    want = M.merge_sequential(m, pts, tri, status, kf1, kf2, t1, t2, n_points)
    g1, g2 = t1.copy(), t2.copy()
    points, obs, out, n_new, n_merged = matcher.map_merge(dmatches(pkg, m), pts, tri, status, kf1, kf2, g1, g2, n_points)
    fresh = want[2] == M.NEW
    assert (n_new, n_merged) == (int(fresh.sum()), int((want[2] == M.MERGED).sum()))
    assert as_bytes(points) == as_bytes(tri["X"][fresh]) == as_bytes(want[0])                          # byte-equal to the records' X
    assert [(int(o["cam"]), int(o["point"]), float(o["u"]), float(o["v"])) for o in obs] == want[1]
    assert np.array_equal(out, want[2]) and np.array_equal(g1, want[3]) and np.array_equal(g2, want[4])
    return points, obs, out, g1, g2, n_new, n_merged


@pytest.mark.parametrize("n,kp1,kp2,seed,n_points,accepted,existing", [
    (400, 500, 450, 1, 50, 0.6, 0.4),       # tables with existing points; records 3 and 300 share a train_idx across blocks
    (300, 300, 300, 3, 0, 0.7, 0.0),        # an empty map: all new
    (257, 257, 40, 6, 9, 1.0, 1.0),         # every record accepted, every query keypoint has a point: all merged
    (256, 300, 300, 7, 5, 0.0, 0.5),        # no accepted record
    (64, 64, 10, 2, 7, 0.8, 0.3), (65, 80, 80, 9, 3, 0.5, 0.5), (1, 5, 5, 4, 3, 1.0, 0.0)])
def test_merge_against_the_sequential_loop(pkg, matcher, n, kp1, kp2, seed, n_points, accepted, existing):
    shared = ((3, 300), (10, 40)) if n == 400 else (((10, 40),) if n >= 64 and accepted > 0 else ())     # (10, 40): inside one wave
    lists = S.merge_lists(n, kp1, kp2, seed, accepted=accepted, existing=existing, shared=shared, n_points=n_points)
    if accepted == 0.0:
        lists[3][lists[3] == M.ACCEPTED] = M.REJ_REPROJ
    points, obs, out, g1, g2, n_new, n_merged = check_merge(pkg, matcher, lists)
    m, status = lists[0], lists[3]
    for a, b in shared:
        last = int(np.flatnonzero((status == M.ACCEPTED) & (m[:, 1] == m[b, 1]))[-1])
        assert m[a, 1] == m[b, 1] and last >= b and g2[m[b, 1]] == g1[m[last, 0]]                        # the last in list order wins
    if existing == 1.0 and accepted == 1.0:
        assert n_new == 0 and n_merged == n
    if n_points == 0:
        assert n_merged == 0 and n_new == int((status == M.ACCEPTED).sum())
    if accepted == 0.0:
        assert (n_new, n_merged) == (0, 0) and np.array_equal(g1, lists[4]) and np.array_equal(g2, lists[5]) and np.array_equal(out, status)
    li = matcher.launch_info()
    assert li.pairs == n and li.launches == 4 and li.kernel_ms > 0
    again = check_merge(pkg, matcher, lists)
    assert all(as_bytes(x) == as_bytes(y) for x, y in zip(again[:5], (points, obs, out, g1, g2)))


def test_merge_capacity_and_refusals(pkg, matcher):
    lib, h = pkg.load_library(), matcher._h
    m, pts, tri, status, t1, t2, n_points = S.merge_lists(400, 500, 450, 1)
    dm = dmatches(pkg, m)
    want = M.merge_sequential(m, pts, tri, status, 4, 5, t1, t2, n_points)
    n_new, n_merged = int((want[2] == M.NEW).sum()), int((want[2] == M.MERGED).sum())
    n_obs = 2 * n_new + n_merged
    bufs = [np.full(24 * n_new, FILL, np.uint8), np.full(24 * n_obs, FILL, np.uint8), np.full(400, FILL, np.uint8)]
    a, b = C.c_int32(-7), C.c_int32(-7)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)                                 # noqa: E731

    def call(cap_points, cap_obs, matches=dm, tab1=None, n_pts=n_points):
        g1, g2 = (t1 if tab1 is None else tab1).copy(), t2.copy()
        rc = lib.lcm_map_merge(h, vp(matches), vp(pts), vp(tri), vp(status), 400, 4, 5, vp(g1), 500, vp(g2), 450, n_pts, vp(bufs[0]), cap_points,
                               vp(bufs[1]), cap_obs, vp(bufs[2]), C.byref(a), C.byref(b))
        return rc, g1, g2

    for caps in ((n_new - 1, n_obs), (n_new, n_obs - 1)):                       # one short on either buffer
        rc, g1, g2 = call(*caps)
        assert rc == -4 and (a.value, b.value) == (n_new, n_merged) and np.array_equal(g1, t1) and np.array_equal(g2, t2)
        assert all((x == FILL).all() for x in bufs)
        a.value = b.value = -7
    twice = dm.copy()
    twice["query_idx"][7] = twice["query_idx"][200]
    wrong = t1.copy()
    wrong[11] = n_points
    for kw in (dict(matches=twice), dict(tab1=wrong), dict(n_pts=-1)):
        rc, g1, g2 = call(n_new, n_obs, **kw)
        assert rc == -1 and (a.value, b.value) == (-7, -7) and all((x == FILL).all() for x in bufs), kw
    rc, g1, g2 = call(n_new, n_obs)
    assert rc == 0 and as_bytes(bufs[0]) == as_bytes(want[0]) and np.array_equal(bufs[2], want[2]) and np.array_equal(g1, want[3]) and np.array_equal(g2, want[4])


# ---- 4. lcm_map_add_keyframe --------------------------------------------------------------------------------------------------
def epi_params(pkg):
    return pkg.capi.default_epi_params(fx=K[0], fy=K[1], cx=K[2], cy=K[3])


def library_cos_min(pkg, matcher, deg=1.0):
    case = S.pair_cases()["n1"]
    (_, _, info), _ = run_pairs(pkg, matcher, [S.Pair("c", case.R1, case.t1, case.R2, case.t2, case.pts, None, dict(min_parallax_deg=deg))], mask=None)
    return float(info[0]["cos_min"])


@pytest.fixture(scope="module")
def replay(pkg, matcher):
    """The trajectory through the library, keyframe by keyframe, beside the Python loop fed with the pose stage's own public
    outputs (lcm_lo_verify_pairs and lcm_pose_recover_pairs on the same lists, tested against their restatements elsewhere).  The
    local optimisation is on: the minimal-sample matrix alone leaves a pose error that five keyframes would add up."""
    c = pkg.capi
    tr = S.Trajectory()
    mp, ep, lp = map_params(pkg), epi_params(pkg), c.default_lo_params()
    cosine = library_cos_min(pkg, matcher)
    poses = [c.pgo_poses(np.eye(3)[None], np.zeros((1, 3)))]
    tables = [np.full(tr.n_points, -1, np.int32)]
    py_tables = [tables[0].copy()]
    points, obs, py_points, py_obs, reports, steps = [], [], [], [], [], []
    for f in range(1, tr.n_frames):
        m, p = tr.matches(f - 1, f)
        n_before = sum(len(x) for x in points)
        t_new = np.full(tr.n_points, -1, np.int32)
        rep, new_points, new_obs, status = matcher.map_add_keyframe(dmatches(pkg, m), p, f - 1, poses[-1], tables[-1], f, t_new, n_before, mp, ep, lp=lp)
        launches = matcher.launch_info().launches
        res, _, mask = matcher.lo_verify_pairs(p, [0, len(p)], ep, lp)
        pres, pmask = matcher.pose_recover_pairs(p, [0, len(p)], res["E"], ep, mask_in=mask)
        pose = (int(pres[0]["status"]) == c.POSE_OK, int(pres[0]["n_good"]), pres[0]["R"], pres[0]["t"], pmask)
        want = M.add_keyframe(K, m, p, f - 1, poses[-1]["R"][0], poses[-1]["t"][0], py_tables[-1], f, np.full(tr.n_points, -1, np.int32), n_before,
                              pose, cosine)
        steps.append(dict(rep=rep, want=want, status=status, new_points=new_points, new_obs=new_obs, launches=launches, matches=m, pts=p))
        assert rep.verdict == want["verdict"] == M.KEYFRAME, (f, rep.verdict, want["verdict"])
        poses.append(c.pgo_poses(np.array(rep.R).reshape(1, 3, 3), np.array(rep.t).reshape(1, 3)))
        py_tables[-1] = want["table_last"]
        tables.append(t_new), py_tables.append(want["table_new"])
        points.append(new_points), obs.append(new_obs), py_points.append(want["points"]), py_obs.extend(want["obs"])
        reports.append(rep)
    return dict(tr=tr, poses=np.concatenate(poses), tables=tables, py_tables=py_tables, points=np.concatenate(points), obs=np.concatenate(obs),
                py_points=np.concatenate(py_points), py_obs=py_obs, steps=steps, mp=mp, ep=ep, lp=lp)


def test_trajectory_replayed_against_the_python_loop(pkg, replay):
    tr = replay["tr"]
    for f, s in enumerate(replay["steps"], 1):
        rep, want = s["rep"], s["want"]
        assert rep.n_matches == tr.n_points and rep.median == want["median"] and rep.n_inliers == want["n_inliers"] >= 200
        assert as_bytes(np.array(rep.R)) == as_bytes(want["R"]) and as_bytes(np.array(rep.t)) == as_bytes(want["t"])
        assert float(rep.baseline) == float(want["plan"].baseline) and abs(rep.baseline - 1.0) < 1e-9                # |t| = 1
        assert np.array_equal(s["status"], want["status"]) and list(rep.counts) == want["counts"].tolist()
        assert rep.counts[M.ACCEPTED] == 0 and rep.n_new == rep.counts[M.NEW] and rep.n_merged == rep.counts[M.MERGED]
        assert rep.n_new > 0 and (f == 1) == (rep.n_merged == 0) and rep.counts[M.NOT_INLIER] >= 20                  # the planted wrong matches
        x = np.stack([s["new_points"]["x"], s["new_points"]["y"], s["new_points"]["z"]], 1)
        scale = np.maximum(1.0, np.abs(want["points"]).max(1))
        assert (np.abs(x - want["points"]).max(1) / scale).max() <= S.MARGIN * S.OWN_X_REL
        assert s["launches"] >= 1 + 3 + 2 + 1 + 1 + 4                                             # median, RANSAC, optimisation, pose, triangulation, merge
    assert [(int(o["cam"]), int(o["point"]), float(o["u"]), float(o["v"])) for o in replay["obs"]] == replay["py_obs"]
    for a, b in zip(replay["tables"], replay["py_tables"]):
        assert np.array_equal(a, b)
    assert len(replay["points"]) == len(replay["py_points"]) > tr.n_points // 2
    # the recovered poses are the planted ones (equal chords of length 1, pose 0 the identity)
    for f in range(tr.n_frames):
        assert np.abs(replay["poses"]["R"][f].reshape(3, 3) - tr.R[f]).max() < 2e-2 and np.abs(replay["poses"]["t"][f] - tr.t[f]).max() < 1e-1


def test_the_map_is_accepted_by_the_bundle_adjustment(pkg, matcher, replay):
    c = pkg.capi
    bp = c.default_ba_params(fx=K[0], fy=K[1], cx=K[2], cy=K[3])
    mean, each = matcher.ba_error(replay["poses"], replay["points"], replay["obs"], bp, per_observation=True)
    print("mean reprojection error of the built map", mean, "over", len(each), "observations")
    assert mean < replay["mp"].max_reproj and len(each) == len(replay["obs"]) and np.isfinite(each).all()
    assert replay["obs"]["point"].max() == len(replay["points"]) - 1 and replay["obs"]["cam"].max() == replay["tr"].n_frames - 1


def test_each_verdict_once_with_the_maps_bytes_unchanged(pkg, matcher, replay):
    c = pkg.capi
    tr, ep, lp0 = replay["tr"], replay["ep"], replay["lp"]
    m, p = tr.matches(0, 1)
    dm = dmatches(pkg, m)
    pose0 = replay["poses"][:1]
    still = p.copy()
    still[:, 2:] = still[:, :2] + np.float32(2.0)
    jump = p.copy()
    jump[:, 2] += np.float32(400.0)
    cases = ((M.FEW_MATCHES, dict(), dm[:99], p[:99]), (M.LITTLE_MOTION, dict(), dm, still), (M.MUCH_MOTION, dict(), dm, jump),
             (M.NO_POSE, dict(min_pose_inliers=100000), dm, p), (M.NO_POSE, dict(min_tracked=0, min_displacement=0.0), dm[:7], p[:7]),
             (M.FEW_INLIERS, dict(min_inliers=100000), dm, p), (M.FEW_INLIERS, dict(min_inlier_ratio=0.999), dm, p))
    for verdict, over, matches, pts in cases:
        t1, t2 = np.full(tr.n_points, -1, np.int32), np.full(tr.n_points, -1, np.int32)
        t1[::3] = 0
        keep1, keep2 = t1.copy(), t2.copy()
        points, obs, status = np.full(24 * len(pts), FILL, np.uint8), np.full(48 * len(pts), FILL, np.uint8), np.full(len(pts), FILL, np.uint8)
        rep = c.MapKeyframeReport()
        mp = map_params(pkg, **over)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)                             # noqa: E731
        rc = pkg.load_library().lcm_map_add_keyframe(matcher._h, vp(matches), vp(pts), len(pts), 0, vp(pose0), vp(t1), len(t1), 1, vp(t2), len(t2), 1,
                                                     C.byref(mp), C.byref(ep), None, None, vp(points), len(pts), vp(obs), 2 * len(pts), vp(status),
                                                     C.byref(rep))
        assert rc == 0 and rep.verdict == verdict, (verdict, over, rep.verdict)
        assert (rep.n_new, rep.n_merged, rep.n_matches) == (0, 0, len(pts)) and not any(rep.R) and not any(rep.counts)
        assert np.array_equal(t1, keep1) and np.array_equal(t2, keep2) and all((x == FILL).all() for x in (points, obs, status))
        assert rep.median == (0.0 if verdict == M.FEW_MATCHES else M.median(pts))
        assert (rep.n_inliers > 0) == (verdict == M.FEW_INLIERS)
    # the same frame with the defaults is a keyframe, twice with the same bytes; with the local optimisation in between as well
    outs = []
    for lp in (None, None, lp0):
        t1, t2 = np.full(tr.n_points, -1, np.int32), np.full(tr.n_points, -1, np.int32)
        rep, points, obs, status = matcher.map_add_keyframe(dm, p, 0, pose0, t1, 1, t2, 0, replay["mp"], ep, lp=lp)
        assert rep.verdict == M.KEYFRAME and rep.n_new > 200
        outs.append((bytes(rep), as_bytes(points), as_bytes(obs), as_bytes(status), as_bytes(t1), as_bytes(t2)))
    assert outs[0] == outs[1] and outs[2][0] == bytes(replay["steps"][0]["rep"]) and outs[2][1] == as_bytes(replay["steps"][0]["new_points"])
    # too little room: LCM_ERR_CAPACITY, the needed counts in the report, nothing else written
    need = replay["steps"][0]["rep"]
    for caps in ((need.n_new - 1, 2 * need.n_new), (need.n_new, 2 * need.n_new + need.n_merged - 1)):
        t1, t2 = np.full(tr.n_points, -1, np.int32), np.full(tr.n_points, -1, np.int32)
        with pytest.raises(pkg.LcmError) as e:
            matcher.map_add_keyframe(dm, p, 0, pose0, t1, 1, t2, 0, replay["mp"], ep, lp=lp0, cap_points=caps[0], cap_obs=caps[1])
        assert e.value.code == -4 and (t1 == -1).all() and (t2 == -1).all()


# ---- 5. lcm_map_db_track ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def track_store(pkg):
    """A store of its own: slot 0 holds 300 rows (the trajectory's keyframe 0), slot 1 64 rows and slot 2 300 rows of keyframe 1.
    A later slot shares rows (exact copies: the only survivors of the ratio test among uniformly random rows) with slot 0; the
    shared rows' keypoints are the two views of one world point, a tenth of them of different points (false matches)."""
    rng = np.random.default_rng(91)
    tr = S.Trajectory(seed=6)
    desc0 = rng.integers(0, 256, (300, 128), dtype=np.uint8)
    kp0 = np.ascontiguousarray(tr.kp[0][:300])
    world = np.argsort(tr.kp_of[0])[:300]                                       # keypoint k of frame 0 shows world point world[k]
    frames, kps = [desc0], [kp0]
    for rows, n_shared in ((64, 60), (300, 280)):
        f = rng.integers(0, 256, (rows, 128), dtype=np.uint8)
        kp = rng.uniform(0.0, 700.0, (rows, 2)).astype(np.float32)
        qi = np.sort(rng.choice(300, n_shared, replace=False))
        ti = rng.choice(rows, n_shared, replace=False)
        shown = world[qi].copy()
        wrong = rng.choice(n_shared, n_shared // 10, replace=False)
        shown[wrong] = rng.integers(0, tr.n_points, len(wrong))
        f[ti], kp[ti] = desc0[qi], tr.kp[1][tr.kp_of[1][shown]]
        frames.append(f), kps.append(kp)
    m = pkg.Matcher()
    for k, (f, kp) in enumerate(zip(frames, kps)):
        assert m.l2_db_append_kp(f, kp) == k
    yield m, frames, kps
    m.close()


@pytest.mark.parametrize("curr,rows,over", [(1, 64, dict(min_tracked=40, min_inliers=30)), (2, 300, dict()), (1, 64, dict())])
def test_db_track_is_the_composition_byte_for_byte(pkg, track_store, curr, rows, over):
    c = pkg.capi
    m, frames, kps = track_store
    mp, ep = map_params(pkg, **over), epi_params(pkg)
    pose0 = c.pgo_poses(np.eye(3)[None], np.zeros((1, 3)))
    assert m.l2_db_rows(0) == 300 and m.l2_db_rows(curr) == rows
    t1, t2 = np.full(300, -1, np.int32), np.full(rows, -1, np.int32)
    t1[5::7] = np.arange(len(t1[5::7]))
    n_points = len(t1[5::7])
    g1, g2 = t1.copy(), t2.copy()
    lists, rep, points, obs, status = m.map_db_track(0, curr, 0.75, 0, pose0, g1, 1, g2, n_points, mp, ep)
    # the lists, points and masks of the verify call, unchanged
    res, pres, out, pts, mask, pmask, offs = m.pose_db_verify_pairs([(0, curr)], 0.75, ep)
    for got, want in ((lists["results"], res), (lists["pose_results"], pres), (lists["out"], out), (lists["pts"], pts), (lists["mask"], mask),
                      (lists["pose_mask"], pmask), (lists["offsets"], offs)):
        assert as_bytes(got) == as_bytes(want)
    assert int(offs[1]) == len(out) >= (56 if rows == 64 else 270)
    assert np.array_equal(pts[:, :2], kps[0][out["query_idx"]]) and np.array_equal(pts[:, 2:], kps[curr][out["train_idx"]])
    # ... plus what lcm_map_add_keyframe returns on those lists
    h1, h2 = t1.copy(), t2.copy()
    rep2, points2, obs2, status2 = m.map_add_keyframe(out, pts, 0, pose0, h1, 1, h2, n_points, mp, ep)
    assert bytes(rep) == bytes(rep2) and as_bytes(points) == as_bytes(points2) and as_bytes(obs) == as_bytes(obs2) and as_bytes(status) == as_bytes(status2)
    assert np.array_equal(g1, h1) and np.array_equal(g2, h2)
    if over or rows == 300:
        assert rep.verdict == M.KEYFRAME and rep.n_new > 0 and rep.n_merged > 0 and rep.n_new + rep.n_merged == (status >= M.MERGED).sum()
        assert not np.array_equal(g2, t2)
    else:
        assert rep.verdict == M.FEW_MATCHES and np.array_equal(g1, t1) and np.array_equal(g2, t2) and len(points) == 0 and len(obs) == 0
    again = m.map_db_track(0, curr, 0.75, 0, pose0, t1.copy(), 1, t2.copy(), n_points, mp, ep)
    assert bytes(again[1]) == bytes(rep) and as_bytes(again[2]) == as_bytes(points) and as_bytes(again[3]) == as_bytes(obs)


def test_db_track_refusals(pkg, track_store):
    c = pkg.capi
    m, frames, kps = track_store
    mp, ep = map_params(pkg), epi_params(pkg)
    pose0 = c.pgo_poses(np.eye(3)[None], np.zeros((1, 3)))
    t1, t2 = np.full(300, -1, np.int32), np.full(300, -1, np.int32)
    for kw in (dict(last_slot=0, curr_slot=3), dict(last_slot=-1, curr_slot=2)):
        with pytest.raises(pkg.LcmError) as e:
            m.map_db_track(kw["last_slot"], kw["curr_slot"], 0.75, 0, pose0, t1, 1, t2, 0, mp, ep)
        assert e.value.code == -1
    wrong = t1.copy()
    wrong[4] = 9
    with pytest.raises(pkg.LcmError) as e:
        m.map_db_track(0, 2, 0.75, 0, pose0, wrong, 1, t2, 9, mp, ep)
    assert e.value.code == -1
    with pytest.raises(pkg.LcmError) as e:
        m.map_db_track(0, 2, 0.75, 0, pose0, t1, 1, t2, 0, mp, ep, cap=10)                 # the lists do not fit: nothing of the map either
    assert e.value.code == -4 and (t1 == -1).all() and (t2 == -1).all()
