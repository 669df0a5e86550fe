"""Deterministic inputs for the map building (include/lcm.h, lcm_map_*) ON its thresholds, at its size limits and across its
block seams, like verifylimitcases.py for the verification.  Shared by tests/test_map_limit_cases_host.py (CPU) and
tests/test_gpu_map_limits.py (GPU).  Every expectation comes from tests/mapref.py and numpy alone, and every generator asserts
what it planted.

DERIVED PARAMETER SETS: mapcases.py keeps every record clear of every threshold; here one parameter is moved ONTO a record's own
field (rel = depth1 / baseline, max(err1, err2), cos_parallax), read from a lcm_map_tri array (the device's on the GPU, mapref's
in the host file), and onto the neighbouring double.  mapref.status_of_fields says what every record's status then is.
BIG PAIRS: 65 535, 65 536 and 65 537 records (grid x = 256, 256, 257): the two-frame trajectory of 65 535 points with planted
records of the statuses it lacks, and two more accepted records.  THE 4096-PAIR CALL: LCM_MAP_MAX_PAIRS pairs of 0 .. 5 records,
300 at both ends, eight pose pairs laid out so that a pair index taken modulo 256 or 1024 finds other poses.
THE MEDIAN: a plateau of 66 000 equal displacements (more than 2^16 values in one bin through all eight passes).
THE MERGE: 65 535, 65 537 and 262 401 records (256, 257 and 1026 blocks: the block scan's second 1024-entry chunk), dense, only
the seams, and with whole blocks empty; train keypoints shared across blocks and chunks; the map's point count up to 2^31 - 1."""
import functools
from collections import namedtuple

import numpy as np

import mapcases as S
import mapref as M

K = S.K
BLOCK = 256                       # MAP_THREADS: records per workgroup of every map kernel
MAX_PAIRS = 4096                  # LCM_MAP_MAX_PAIRS
MAX_MATCHES = 65535               # EPI_MAX_POINTS: lcm_map_add_keyframe's longest list
INT_MAX = (1 << 31) - 1


def ro(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


# ---- A. derived parameter sets -----------------------------------------------------------------------------------------------
WANTED = (0, 64, 128, 192, 256)  # one position per wave of the first block, and the first record of the second


def pick_accepted(status, wanted=WANTED, allowed=None):
    """The accepted record nearest to every wanted position (the earlier one of two equally near), without repeats.  allowed:
    bool [n], a further condition on the records."""
    ok = np.asarray(status) == M.ACCEPTED
    if allowed is not None:
        ok = ok & np.asarray(allowed)
    have = np.flatnonzero(ok)
    assert len(have) >= len(wanted), f"{len(have)} accepted records for {len(wanted)} positions"
    out = []
    for w in wanted:
        rest = have[~np.isin(have, out)]
        out.append(int(rest[np.argmin(np.abs(rest - w), axis=0)]))
    assert len(set(out)) == len(wanted)
    if max(wanted) >= 64:
        assert len({k // 64 for k in out}) >= 2, "the records must lie in different waves"
    return out


def larger_error(tri):
    """1 where err1 > err2, 2 where err2 > err1, 0 where equal."""
    t = np.asarray(tri)
    return np.where(t["err1"] > t["err2"], 1, np.where(t["err2"] > t["err1"], 2, 0))


def reproj_records(tri, status):
    """(k1, k2): an accepted record whose larger error is err1 and one whose larger error is err2; both kinds must exist."""
    acc, which = np.asarray(status) == M.ACCEPTED, larger_error(tri)
    one, two = np.flatnonzero(acc & (which == 1)), np.flatnonzero(acc & (which == 2))
    assert len(one) and len(two), f"{len(one)} accepted records with err1 larger, {len(two)} with err2 larger"
    return int(one[len(one) // 2]), int(two[len(two) // 2])


Derived = namedtuple("Derived", "edge k at off off_status")
EDGES = ("min_depth", "max_depth", "max_reproj")


def derive(tri, status, baseline, cosine, pp, k, edge, source=None):
    """One parameter moved onto record k's own value (`at`: k stays accepted) and onto the neighbouring double (`off`: k gets
    off_status).  source: the record the value is read from (the host test passes a neighbour and must see this fail)."""
    t = np.asarray(tri)
    j = k if source is None else source
    assert status[k] == M.ACCEPTED and M.status_of_fields(t[k:k + 1], baseline, cosine, pp)[0] == M.ACCEPTED, f"record {k} is not accepted"
    if edge == "min_depth":
        v = float(M.rel_depth(t[j:j + 1], baseline)[0])
        at, off, want = v, float(np.nextafter(v, np.inf)), M.REJ_DEPTH
    elif edge == "max_depth":
        v = float(M.rel_depth(t[j:j + 1], baseline)[0])
        at, off, want = v, float(np.nextafter(v, -np.inf)), M.REJ_DEPTH
    else:
        assert edge == "max_reproj"
        v = float(max(t["err1"][j], t["err2"][j]))
        at, off, want = v, float(np.nextafter(v, -np.inf)), M.REJ_REPROJ
    p_at, p_off = dict(pp or {}, **{edge: at}), dict(pp or {}, **{edge: off})
    got_at = M.status_of_fields(t[k:k + 1], baseline, cosine, p_at)[0]
    got_off = M.status_of_fields(t[k:k + 1], baseline, cosine, p_off)[0]
    assert got_at == M.ACCEPTED and got_off == want, f"{edge} from record {j}: record {k} is {got_at} on the value and {got_off} beside it"
    return Derived(edge, k, p_at, p_off, want)


def derived_sets(tri, status, baseline, cosine, pp=None, wanted=WANTED):
    """Every derived set of one pair: the depth edges on the accepted records nearest to `wanted`, max_reproj on the first and
    the last of them and on one record of each kind (err1 larger, err2 larger)."""
    ks = pick_accepted(status, wanted)
    out = [derive(tri, status, baseline, cosine, pp, k, e) for e in ("min_depth", "max_depth") for k in ks]
    k1, k2 = reproj_records(tri, status)
    assert larger_error(tri)[k1] == 1 and larger_error(tri)[k2] == 2
    out += [derive(tri, status, baseline, cosine, pp, k, "max_reproj") for k in dict.fromkeys([k1, k2, ks[0], ks[-1]])]
    return out


def ulps(x, k):
    """The double k steps away from x (k of either sign), by its bit pattern; x > 0."""
    b = np.array([x], np.float64).view(np.int64)
    return float((b + np.int64(k)).view(np.float64)[0])


def cosine_edge(cos_of, c, span=4000):
    """(deg_at, deg_off) for an accepted record's cos_parallax c under the cosine function cos_of(deg) -> double: deg_at with
    cos_of(deg_at) == c bit for bit, and the nearest deg above it whose cosine is the next double below c; None where no double
    within `span` steps of degrees(acos(c)) hits c.  cos_of is not increasing in deg: a bisection over the steps, its result
    checked."""
    d0 = float(np.degrees(np.arccos(c)))
    lo, hi = -span, span                                     # the smallest step whose cosine is <= c
    if not (cos_of(ulps(d0, lo)) > c >= cos_of(ulps(d0, hi))):
        return None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if cos_of(ulps(d0, mid)) <= c else (mid, hi)
    if cos_of(ulps(d0, hi)) != c:
        return None
    at = hi
    lo, hi = at, span                                        # the smallest step whose cosine is < c
    if not cos_of(ulps(d0, hi)) < c:
        return None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if cos_of(ulps(d0, mid)) < c else (mid, hi)
    if cos_of(ulps(d0, hi)) != float(np.nextafter(c, -np.inf)) or cos_of(ulps(d0, hi - 1)) != c:
        return None
    return ulps(d0, at), ulps(d0, hi)


MIN_COSINE_HITS = 3


def cosine_edges(cos_of, tri, status, wanted=WANTED):
    """{k: (deg_at, deg_off)} over the accepted records nearest to `wanted`; at least MIN_COSINE_HITS of them must be hit."""
    t = np.asarray(tri)
    out = {}
    for k in pick_accepted(status, wanted):
        e = cosine_edge(cos_of, float(t["cos_parallax"][k]))
        if e is not None:
            out[k] = e
    assert len(out) >= MIN_COSINE_HITS, f"an exact cosine for {len(out)} of {len(wanted)} records"
    return out


# ---- B1. the big pairs -------------------------------------------------------------------------------------------------------
BIG_LENS = (65535, 65536, 65537)
# mapref's own float64 rounding against np.longdouble on big_source()'s 65 537 records, rounded up from what
# test_map_limit_cases_host.py::test_own_rounding_on_the_new_pairs measures.  The 3000 wrong matches are records no case of
# mapcases.py holds (rays that meet a hundredth of a baseline in front of a camera, reprojection errors of tens of thousands of
# pixels), and three of mapcases' constants do not bound them; the depth's does and is kept.
BIG_OWN_X_REL = 2e-11             # measured 1.4e-11 (mapcases.OWN_X_REL: 5e-12)
BIG_OWN_DEPTH_REL = S.OWN_DEPTH_REL   # measured 3.0e-12
BIG_OWN_COS = 1e-12               # measured 5.7e-13 (mapcases.OWN_COS: 5e-13)
BIG_OWN_ERR = 5e-9                # measured 2.5e-9 px, on an error of 82 306 px (mapcases.OWN_ERR: 1e-10)
# three planted kinds (no point, depth, parallax) in turn, on both sides of the first and the last block seam
PLANT_AT = (1, 2, 3, 62, 63, 64, 253, 254, 255, 256, 257, 258, 65277, 65278, 65279, 65280, 65281, 65282)


@functools.lru_cache(maxsize=None)
def trajectory():
    return S.Trajectory(n_frames=2, n_points=MAX_MATCHES, wrong=3000)


@functools.lru_cache(maxsize=None)
def big_source(keep_last=True):
    """(Pair of 65 537 records without a mask, its mapref Records, the mask of the masked form).  Records 0 .. 65 534 are the
    trajectory's matches of frames 0 and 1 (3000 of them wrong), with records of mapcases.candidates under the same two poses
    (no point, depth, parallax: BUILD's distances clear of every threshold) planted on PLANT_AT and on 600 random positions;
    records 65 534, 65 535 and 65 536 are accepted ones, so every length of BIG_LENS ends in an accepted record and the last
    record of 65 537 is alone in its workgroup.  keep_last = False leaves record 65 536 to chance (the host test)."""
    tr = trajectory()
    _, pts = tr.matches(0, 1)
    pts = pts.copy()
    pool = S.Pair("pool", tr.R[0], tr.t[0], tr.R[1], tr.t[1], S.candidates(tr.R[0], tr.t[0], tr.R[1], tr.t[1], 41))
    rec = pool.records()
    ok = S.clear_of_thresholds(rec, pool.plan(), None, S.BUILD)
    rng = np.random.default_rng(42)
    spots = np.concatenate([np.array(PLANT_AT), rng.choice(np.setdiff1d(np.arange(300, 65000), PLANT_AT), 600, replace=False)])
    kinds = [np.flatnonzero(ok & (rec.status == s)) for s in (M.NO_POINT, M.REJ_DEPTH, M.REJ_PARALLAX)]
    assert all(len(k) >= 3 for k in kinds), [len(k) for k in kinds]
    for i, at in enumerate(spots):
        have = kinds[i % 3]
        pts[at] = pool.pts[have[(i // 3) % len(have)]]
    own = S.Pair("traj", tr.R[0], tr.t[0], tr.R[1], tr.t[1], pts).records()
    good = np.flatnonzero((own.status == M.ACCEPTED) & S.clear_of_thresholds(own, pool.plan(), None, S.BUILD))
    good = good[~np.isin(good, spots)]
    assert len(good) > 50000
    tail = pts[good[[100, 20000, 40000]]]
    pts[MAX_MATCHES - 1] = tail[0]
    pts = np.concatenate([pts, tail[1:]])
    if not keep_last:
        pts[-1] = pool.pts[kinds[1][0]]
    pair = S.Pair("big", tr.R[0], tr.t[0], tr.R[1], tr.t[1], pts)
    r = pair.records()
    for n in BIG_LENS:
        assert r.status[n - 1] == M.ACCEPTED, f"the last record of {n} is {r.status[n - 1]}, not accepted"
    counts = r.counts()
    assert (counts[1:6] >= 100).all() and counts[0] == 0, counts
    for s in (M.NO_POINT, M.REJ_DEPTH, M.REJ_PARALLAX):          # the planted kinds on both sides of the first and the last block seam
        for lo, hi in ((0, 256), (256, 512), (65024, 65280), (65280, 65535)):
            assert (r.status[lo:hi] == s).any(), (s, lo)
    # no record that takes part is near the one threshold status_of_fields does not restate: |w| against 1e-9
    assert not S.near(np.abs(r.w), M.MIN_W, S.GUARD_W).any()
    mask = (np.random.default_rng(43).random(len(pts)) > 0.1).astype(np.uint8)
    mask[[MAX_MATCHES - 1, MAX_MATCHES, MAX_MATCHES + 1]] = 1
    mask[[0, 255, 256]] = (0, 1, 0)
    ro(pair.pts, mask)
    return pair, r, mask


def big_pair(n, masked):
    """(Pair of n records, expected lcm_map_tri, expected statuses by mapref) as a prefix of big_source()."""
    assert n in BIG_LENS
    pair, r, mask = big_source()
    tri, status = r.tri()[:n].copy(), r.status[:n].copy()
    if masked:
        off = mask[:n] == 0
        tri[off] = np.zeros(1, M.TRI_DTYPE)
        status[off] = M.NOT_INLIER
    return S.Pair(f"big{n}", pair.R1, pair.t1, pair.R2, pair.t2, pair.pts[:n], mask[:n] if masked else None), tri, status


# ---- B1. LCM_MAP_MAX_PAIRS pairs in one call ---------------------------------------------------------------------------------
N_POSES = 8
# The same measurement over the records of many_pairs() (every status as often as the others, which weights the far side points
# and the points at infinity more than mapcases' cases do): X and the depths stay within mapcases' constants, these two do not.
# BUILD's distances (1e-6 and 1e-3) stay above twice 1000 x MARGIN x these, so the statuses still compare exactly.
MANY_OWN_COS = 2e-12              # measured 1.2e-12 (mapcases.OWN_COS: 5e-13)
MANY_OWN_ERR = 5e-10              # measured 2.9e-10 px (mapcases.OWN_ERR: 1e-10)


def pose_of(p):
    """The pose pair of pair p: differs between p and p +- 1, p +- 256 and p +- 1024."""
    return (p + p // 256 + p // 1024) % N_POSES


ManyPairs = namedtuple("ManyPairs", "pts offsets mask R1 t1 R2 t2 tri status counts baseline group")


@functools.lru_cache(maxsize=None)
def pose_pools():
    pools = []
    for g in range(N_POSES):
        R1, t1, R2, t2 = S.two_cameras(50 + g, (12, 24, 18, 16)[g % 4])
        pool = S.Pair(f"pose{g}", R1, t1, R2, t2, S.candidates(R1, t1, R2, t2, 60 + g))
        rec = pool.records()
        keep = np.flatnonzero(S.clear_of_thresholds(rec, pool.plan(), None, S.BUILD))
        assert all((rec.status[keep] == s).sum() >= 3 for s in range(1, 6)), (g, np.bincount(rec.status[keep], minlength=6))
        pools.append(pool.take(keep))
    return pools


def many_pairs(layout=pose_of, n_pairs=MAX_PAIRS, seed=70):
    """The 4096-pair call: sizes 0 .. 5 (half of the pairs empty), 300 records in pairs 0 and 4095, a zero mask byte on a
    seventh of the records.  The reference is computed once per pose pair over that pose pair's concatenated records and
    scattered back; counts per pair."""
    for p in range(n_pairs):
        for d in (1, 256, 1024):
            for q in (p - d, p + d):
                assert not 0 <= q < n_pairs or layout(p) != layout(q), f"pairs {p} and {q} share pose pair {layout(p)}"
    assert len({layout(p) for p in range(n_pairs)}) >= 8
    pools = pose_pools()
    rng = np.random.default_rng(seed)
    sizes = rng.choice([0, 0, 0, 0, 0, 1, 2, 3, 4, 5], n_pairs)
    sizes[0] = sizes[n_pairs - 1] = 300
    sizes[[1, 255, 256, 1023, 1024]] = (0, 5, 5, 4, 5)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    total = int(offsets[-1])
    group = np.repeat(np.array([layout(p) for p in range(n_pairs)]), sizes)
    pts, mask = np.zeros((total, 4), np.float32), (rng.random(total) > 1 / 7).astype(np.uint8)
    tri, status = np.zeros(total, M.TRI_DTYPE), np.zeros(total, np.uint8)
    baseline = np.zeros(N_POSES)
    for g, pool in enumerate(pools):
        at = np.flatnonzero(group == g)
        kind = rng.integers(1, 6, len(at))                   # every status as often as the others
        by = [np.flatnonzero(pool.records().status == s) for s in range(6)]
        pts[at] = pool.pts[[by[s][rng.integers(0, len(by[s]))] for s in kind]]
        r = M.triangulate(pool.plan(), pts[at], mask[at])
        tri[at], status[at], baseline[g] = r.tri(), r.status, float(pool.plan().baseline)
    pair_of = np.repeat(np.arange(n_pairs), sizes)
    counts = np.zeros((n_pairs, 8), np.int64)
    np.add.at(counts, (pair_of, status), 1)
    assert (sizes == 0).sum() > n_pairs // 3 and total < 20000 and (counts[:, :6].sum(0) > 100).all(), counts.sum(0)
    assert len({pools[g].R2.tobytes() for g in range(N_POSES)}) == N_POSES
    ps = [pools[layout(p)] for p in range(n_pairs)]
    R1, t1, R2, t2 = (np.stack([getattr(q, f) for q in ps]) for f in ("R1", "t1", "R2", "t2"))
    return ManyPairs(pts, offsets, mask, R1, t1, R2, t2, tri, status, counts, np.array([baseline[layout(p)] for p in range(n_pairs)]), group)


# ---- B2. the median ----------------------------------------------------------------------------------------------------------
PLATEAU, PLATEAU_VALUE = 66000, 5.0


def plateau_pair(above, plateau=PLATEAU, seed=80):
    """float32 [n, 4] in which `plateau` records share the displacement 5.0 exactly (integer pixels, a 3 : 4 : 5 triangle).
    above = False: 70 000 records, 2000 smaller and 2000 larger values: element n / 2 lies inside the plateau, whose 66 000 values
    (more than 2^16) sit in ONE bin of every one of the eight passes.  above = True: the element n / 2 of 70 000 records cannot
    leave a plateau of 66 000 (it covers 66 000 consecutive ranks of 70 000), so this variant has 132 001 records: the plateau at
    the bottom and 66 001 larger values; element n / 2 = 66 000 is the smallest value above the plateau, the rank wanted is
    above 2^16 from the first pass to the last, and the larger values share their upper three bytes with the plateau."""
    rng = np.random.default_rng(seed)
    n_low, n_high = (0, plateau + 1) if above else (2000, 2000)
    n = plateau + n_low + n_high
    q = np.stack([rng.integers(0, 1200, n), rng.integers(0, 4, n)], 1).astype(np.float32)       # small y: q + d stays exact in float
    d = np.zeros((n, 2), np.float32)
    d[:] = (3.0, 4.0)
    d[:, 0] *= rng.choice([-1.0, 1.0], n).astype(np.float32)
    order = rng.permutation(n)
    low, high = order[:n_low], order[n_low:n_low + n_high]
    d[low, 1] = rng.uniform(0.0, 3.9, n_low).astype(np.float32)
    d[high, 1] = (4.0 + rng.integers(1, 1000, n_high) * 2.0 ** -20).astype(np.float32)
    pts = np.ascontiguousarray(np.concatenate([q, q + d], 1), np.float32)
    disp = M.displacements(pts)
    want = float(np.sort(disp)[n // 2])
    flat = int((disp == PLATEAU_VALUE).sum())
    assert flat == plateau > 1 << 16, f"{flat} records on the plateau: no bin holds more than 2^16 values"
    assert (disp < PLATEAU_VALUE).sum() == n_low and (disp > PLATEAU_VALUE).sum() == n_high
    if above:
        assert n // 2 == plateau > 1 << 16 and want == disp[disp > PLATEAU_VALUE].min() > PLATEAU_VALUE
        assert (disp.view(np.uint64) >> np.uint64(40) == np.float64(PLATEAU_VALUE).view(np.uint64) >> np.uint64(40)).all()
    else:
        assert want == PLATEAU_VALUE and n_low < n // 2 < n_low + plateau
    return pts, want


def uniform_pair(n=262145, seed=81):
    pts = np.random.default_rng(seed).uniform(0, 2000, (n, 4)).astype(np.float32)
    return pts, float(np.sort(M.displacements(pts))[n // 2])


# ---- B3. the merge -----------------------------------------------------------------------------------------------------------
BIG_N = 262401                                               # 1026 blocks: block 1024 opens the scan's second chunk
SEAM_RECORDS = (0, 63, 64, 255, 256, 257, 65535, 65536, 262143, 262144, 262399, 262400)
FULL_BLOCKS = (0, 1023, 1024, 1025)
BLOCKS_SHARED = ((5, 262300), (262143, 262144))           # first and last chunk; adjacent blocks on both sides of the chunk seam
SHARED = {65535: ((5, 65500), (255, 256), (1000, 30000, 60000)), 65537: ((5, 65500), (255, 256), (1000, 30000, 60000)),
          BIG_N: ((5, 262300), (255, 256), (1000, 70000, 200000))}
N_KP2 = 70000
MergeCase = namedtuple("MergeCase", "name matches pts tri status table1 table2 n_points shared want")


def merge_case(n, variant="dense", n_points=50000, seed=90, drop_shared=None, flip=None, reference=True):
    """The lists of one merge of n records (query_idx unique, n_kp1 = n + 1000, n_kp2 = 70 000: every train keypoint is named by
    several records at n = 262 401) and merge_sequential's outputs.
    dense: about 60 % accepted, about 40 % of the query keypoints with a point; SHARED[n]'s records accepted, each group on one
    train keypoint.  seam (n = 262 401): ONLY SEAM_RECORDS are accepted, in turn new and merged, so both kinds occur on each
    side of record 262 144; (255, 256) and (63, 262 400) share a train keypoint.  blocks (n = 262 401): accepted records only in
    blocks FULL_BLOCKS; (5, 262 300) and (262 143, 262 144) share.
    drop_shared: a group of SHARED left out; flip: a record whose status is changed afterwards (the host test: both must fail)."""
    rng = np.random.default_rng(seed + n % 1000)
    n_kp1 = n + 1000
    m = np.stack([rng.permutation(n_kp1)[:n], rng.integers(0, N_KP2, n)], 1).astype(np.int32)
    other = rng.integers(0, 5, n).astype(np.uint8)
    table1 = np.where(rng.random(n_kp1) < 0.4, rng.integers(0, max(n_points, 1), n_kp1), -1).astype(np.int32)
    if variant == "dense":
        status = np.where(rng.random(n) < 0.6, M.ACCEPTED, other).astype(np.uint8)
        status[n - 1] = M.ACCEPTED                            # at 65 537 and 262 401 the last record is alone in its block
        shared = SHARED[n]
    elif variant == "seam":
        assert n == BIG_N
        status = other
        status[list(SEAM_RECORDS)] = M.ACCEPTED
        for i, k in enumerate(SEAM_RECORDS):
            table1[m[k, 0]] = -1 if i % 2 == 0 else (7 * i) % n_points
        shared = ((255, 256), (63, 262400))
    else:
        assert variant == "blocks" and n == BIG_N
        inside = np.isin(np.arange(n) // BLOCK, FULL_BLOCKS)
        status = np.where(inside & (rng.random(n) < 0.6), M.ACCEPTED, other).astype(np.uint8)
        status[n - 1] = M.ACCEPTED                            # block 1025 holds this one record
        shared = BLOCKS_SHARED
    shared = tuple(g for g in shared if g != drop_shared)
    for g in shared:
        m[list(g[1:]), 1] = m[g[0], 1]
        if variant != "seam":
            status[list(g)] = M.ACCEPTED
    if flip is not None:
        status[flip] = M.REJ_REPROJ if status[flip] == M.ACCEPTED else M.ACCEPTED
    if n_points > INT_MAX - 2 * n:                           # the map's last points are named by the table: carried over unchanged
        table1[m[np.flatnonzero(status == M.ACCEPTED)[:4], 0]] = (n_points - 1, n_points - 2, n_points - 1, n_points - 3)
    table2 = np.full(N_KP2, -1, np.int32)
    pts = rng.uniform(0, 1280, (n, 4)).astype(np.float32)
    tri = np.zeros(n, M.TRI_DTYPE)
    tri["X"] = rng.standard_normal((n, 3))
    tri["X"][0] = [-0.0, np.pi, 1e-310]                       # bytes, not values, are moved
    # ---- what was planted
    acc = status == M.ACCEPTED
    fresh = acc & (table1[m[:, 0]] == -1)
    for g in SHARED[n] if variant == "dense" else (((255, 256), (63, 262400)) if variant == "seam" else BLOCKS_SHARED):
        assert acc[list(g)].all(), f"a record of {g} is not accepted"
        assert len(set(m[list(g), 1].tolist())) == 1, f"the records {g} do not share a train keypoint"
    if variant == "dense":
        assert 0.55 < acc.mean() < 0.65 and 0.3 < (acc & ~fresh).sum() / acc.sum() < 0.5
        assert (np.bincount(m[acc, 1], minlength=N_KP2) > 1).sum() > (1000 if n == BIG_N else 100)
    if variant == "seam":
        assert np.flatnonzero(acc).tolist() == list(SEAM_RECORDS), "the accepted records are not exactly the seam records"
        for side in (np.arange(n) < 262144, np.arange(n) >= 262144):
            assert (fresh & side).any() and (acc & ~fresh & side).any()
    if variant == "blocks":
        blocks = np.unique(np.flatnonzero(acc) // BLOCK)
        assert blocks.tolist() == list(FULL_BLOCKS), blocks
        assert (fresh & (np.arange(n) >= 262144)).any() and (acc & ~fresh & (np.arange(n) >= 262144)).any()
    assert flip == n - 1 or acc[n - 1], "the last record is not accepted"
    assert len(np.unique(m[:, 0])) == n and -(-n // BLOCK) == {65535: 256, 65537: 257, BIG_N: 1026}[n]
    want = M.merge_sequential(m, pts, tri, status, 4, 5, table1, table2, n_points) if reference else None
    if want is not None and n_points > INT_MAX - 2 * n:
        assert ((want[4] >= n_points - 3) & (want[4] < n_points)).sum() >= 2 and want[3].max() == n_points + int((want[2] == M.NEW).sum()) - 1 <= INT_MAX - 1
    ro(m, pts, tri, status, table1, table2)
    return MergeCase(f"{variant}{n}", m, pts, tri, status, table1, table2, n_points, shared, want)


@functools.lru_cache(maxsize=None)
def merge_cases():
    """Every merge case by name, each with its sequential reference, computed once."""
    out = [merge_case(65535), merge_case(65537), merge_case(BIG_N), merge_case(BIG_N, "seam"), merge_case(BIG_N, "blocks")]
    out.append(merge_case(65537, n_points=INT_MAX - 65537)._replace(name="top65537"))
    return {c.name: c for c in out}


@functools.lru_cache(maxsize=None)
def merge_scan_of(name):
    """The second witness of a case, computed once."""
    c = merge_cases()[name]
    return M.merge_scan(c.matches, c.pts, c.tri, c.status, 4, 5, c.table1, c.table2, c.n_points)


def last_writer(case):
    """Per shared group: (train keypoint, the accepted record that names it last in list order)."""
    acc = case.status == M.ACCEPTED
    return [(int(case.matches[g[0], 1]), int(np.flatnonzero(acc & (case.matches[:, 1] == case.matches[g[0], 1]))[-1])) for g in case.shared]


def obs_array(obs, dtype):
    """merge_sequential's observation tuples as records of the library's dtype."""
    return np.array(obs, dtype=dtype) if len(obs) else np.zeros(0, dtype)
