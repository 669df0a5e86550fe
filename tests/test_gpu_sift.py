"""The SIFT keypoint detector on the device (lcm_sift_*: lcm_sift.cpp, lcm_sift.hip) against tests/siftref.py, bit for bit: every
Gaussian and DoG layer of every octave, the candidates of planted DoG stacks in their order, every field of the refined records, and
both one-call forms end to end.  The shapes are chosen for where a tile, a fold or a compaction can break.  Needs a real MI355X."""
import numpy as np
import pytest

import siftcases as S
import siftref as R

pytestmark = pytest.mark.gpu

TILE = 32           # the blur kernel's output tile (csrc/lcm_sift_device.h, SIFT_TILE)
BLOCK = 256         # pixels per block of the extrema search; the scan carries after 1024 blocks
POISON = np.float32(-7.25e8)


def sp_of(pkg, p):
    return pkg.capi.default_sift_params(**vars(p))


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_space_equals(space, img, p, what):
    pl, G, D = R.build(np.ascontiguousarray(img), p)
    info = space.info()
    assert (info.w, info.h, info.plan.n_octaves, info.plan.n_gauss, info.plan.n_dog) == (img.shape[1], img.shape[0], pl.n_octaves, pl.n_gauss, pl.n_dog)
    for o in range(pl.n_octaves):
        for i in range(pl.n_gauss):
            got = space.read(0, o, i)
            assert same(got, G[o][i]), (what, "G", o, i, int(np.sum(got != G[o][i])), np.argwhere(got != G[o][i])[:4].tolist())
        for l in range(pl.n_dog):
            got = space.read(1, o, l)
            assert same(got, D[o][l]), (what, "D", o, l, int(np.sum(got != D[o][l])), np.argwhere(got != D[o][l])[:4].tolist())
    return pl


# the issue's sizes, one size on each side of the tile edge (31 / 32 / 33 as the base, 16 / 17 enlarged to 32 / 34), and layers 2, 5
# and 1 (radius 45: the blur's dynamic LDS above 64 KiB)
SCALE_SPACE = [(w, h, up, {}) for (w, h) in ((17, 13), (64, 64), (65, 63), (129, 97), (200, 37), (37, 200)) for up in (0, 1)] + \
    [(31, 33, 0, {}), (32, 32, 0, {}), (33, 31, 0, {}), (16, 17, 1, {}), (65, 63, 1, {"n_octave_layers": 2}), (129, 97, 0, {"n_octave_layers": 5}),
     (64, 40, 1, {"n_octave_layers": 1})]


@pytest.mark.parametrize("w,h,up,over", SCALE_SPACE, ids=lambda v: str(v).replace(" ", ""))
def test_scale_space_equals_the_restatement(pkg, matcher, w, h, up, over):
    p = R.params(upsample=up, **over)
    img = S.ramp_image(w, h, seed=w + h)
    with matcher.sift_space(w, h, sp_of(pkg, p)) as space:
        space.build(img)
        assert_space_equals(space, img, p, (w, h, up, over))


def test_a_row_stride_above_the_width(pkg, matcher):
    p = R.params()
    wide = S.ramp_image(80, 63, seed=5)
    img = wide[:, :65]                                       # 65 x 63 with a stride of 80 bytes
    assert img.strides == (80, 1)
    with matcher.sift_space(65, 63, sp_of(pkg, p)) as space:
        space.build(img)
        assert_space_equals(space, img, p, "stride")


def test_a_reused_space_equals_a_fresh_one(pkg, matcher):
    p = R.params()
    big, small = S.ramp_image(129, 97, seed=1), S.ramp_image(65, 63, seed=2)
    with matcher.sift_space(129, 97, sp_of(pkg, p)) as space:
        space.build(big)
        pl = assert_space_equals(space, big, p, "first")
        for o in range(pl.n_octaves):                        # poison every layer through the write door
            for kind, layers in ((0, pl.n_gauss), (1, pl.n_dog)):
                for i in range(layers):
                    space.write(kind, o, i, np.full((pl.height[o], pl.width[o]), POISON, np.float32))
        assert (space.read(1, pl.n_octaves - 1, 0) == POISON).all()
        space.build(small)
        assert_space_equals(space, small, p, "rebuilt")
        with pytest.raises(pkg.LcmError) as e:
            space.build(S.ramp_image(130, 97))
        assert e.value.code == -4
        assert_space_equals(space, small, p, "after a refusal")


def planted_space(matcher, pkg, p, w, h, octave=0):
    """A space whose octave `octave` is w x h and whose every DoG layer is zero: a zero image, no enlargement."""
    q = R.params(**{**vars(p), "upsample": 0})
    space = matcher.sift_space(w << octave, h << octave, sp_of(pkg, q))
    space.build(np.zeros((h << octave, w << octave), np.uint8))
    pl = space.info().plan
    assert (pl.width[octave], pl.height[octave]) == (w, h)
    return space, q


def plant(space, d, octave=0):
    for l in range(d.shape[0]):
        space.write(1, octave, l, d[l])


EXTREMA = [("values", S.extrema_values, 70, 41, {}), ("border", S.extrema_border, 70, 41, {}), ("seams", S.extrema_seams, 70, 41, {}),
           ("seams, wide rows", S.extrema_seams, 300, 17, {}), ("values, 2 layers, border 3", S.extrema_values, 70, 41, {"n_octave_layers": 2, "border": 3}),
           ("seams, 5 layers, border 1", S.extrema_seams, 67, 35, {"n_octave_layers": 5, "border": 1}), ("plateau", S.extrema_plateau, 40, 30, {})]


@pytest.mark.parametrize("name,make,w,h,over", EXTREMA, ids=[e[0] for e in EXTREMA])
def test_extrema_of_planted_stacks(pkg, matcher, name, make, w, h, over):
    p = R.params(**over)
    d, want = make(w, h, p)
    space, q = planted_space(matcher, pkg, p, w, h)
    with space:
        plant(space, d)
        got = space.extrema()
        assert same(got, want), (name, len(got), len(want))
        assert same(space.extrema(), want)                   # the same bytes again
        with pytest.raises(pkg.LcmError) as e:
            space.extrema(cap=len(want) - 1)
        assert e.value.code == -4


def test_extrema_in_a_higher_octave_and_across_the_scans_carry(pkg, matcher):
    """A plateau of 300 x 300 as octave 1 of a 600 x 600 space: 3 x 290 x 290 candidates in 1055 blocks of octave 1 behind the 4219
    of octave 0, so the counts cross the scan's carry (1024 blocks) more than once."""
    p = R.params()
    d, want = S.extrema_plateau(300, 300, p)
    want = want.copy()
    want["octave"] = 1
    assert 3 * 300 * 300 > 1024 * BLOCK
    space, q = planted_space(matcher, pkg, p, 300, 300, octave=1)
    with space:
        plant(space, d, octave=1)
        got = space.extrema()
        assert same(got, want), (len(got), len(want))


def assert_detect_equals(pkg, space, D, p, octave=0, what=None):
    stack = [np.zeros((p.n_octave_layers + 2, 1, 1), np.float32)] * octave + [D]
    cand = R.extrema(stack, p)
    want, why = R.refine(stack, cand, p)
    got, n_cand = space.detect()
    assert n_cand == len(cand), (what, n_cand, len(cand))
    assert same(got, want), (what, len(got), len(want))
    return cand, why


def test_refinement_of_walking_candidates(pkg, matcher):
    """Kept after one step and after exactly max_steps steps, not converged, out of the border, off the layers, low contrast, an edge."""
    p = R.params()
    d, cand, why = S.refine_walks(p)
    S.assert_walks_cover(d, cand, why, p)
    space, q = planted_space(matcher, pkg, p, d.shape[2], d.shape[1])
    with space:
        plant(space, d)
        assert_detect_equals(pkg, space, d, q, what="defaults")
    for over in ({"max_steps": 2}, {"max_steps": 1}, {"contrast_threshold": 0.12, "edge_threshold": 3.0}):
        q = R.params(**over)
        space, q = planted_space(matcher, pkg, q, d.shape[2], d.shape[1])
        with space:
            plant(space, d)
            c2, w2 = assert_detect_equals(pkg, space, d, q, what=over)
            assert np.sum(w2 == R.OK) >= 1 and np.sum(w2 != R.OK) >= 1


def test_refinement_of_planted_neighbourhoods(pkg, matcher):
    """A zero pivot, det == 0 with a regular H, the edge test at equality (edge_threshold 1) and just above it (1.01)."""
    p = R.params()
    d, sites = S.refine_planted(64, 24, p)
    S.assert_planted(d, sites, p)
    for over in ({}, {"edge_threshold": 1.0}, {"edge_threshold": 1.01}):
        space, q = planted_space(matcher, pkg, R.params(**over), 64, 24)
        with space:
            plant(space, d)
            assert_detect_equals(pkg, space, d, q, what=over)
    # the same stack as octave 2: x, y and size scale with the octave
    space, q = planted_space(matcher, pkg, p, 64, 24, octave=2)
    with space:
        plant(space, d, octave=2)
        assert_detect_equals(pkg, space, d, q, octave=2, what="octave 2")


@pytest.fixture(scope="module")
def scenes():
    """image name -> (image, the restatement's records, its candidates), computed once"""
    p = R.params()
    out = {}
    for name, img in (("blobs", S.blob_image()), ("noise", S.noise_image())):
        kp, cand, _ = R.detect(img, p)
        out[name] = (img, kp, cand)
    assert len(out["blobs"][1]) == len(S.BLOBS) and len(out["noise"][1]) > 100
    return out


@pytest.mark.parametrize("name", ["blobs", "noise"])
def test_end_to_end(pkg, matcher, scenes, name):
    img, want, cand = scenes[name]
    p = R.params()
    n = len(want)
    with matcher.sift_space(160, 120, sp_of(pkg, p)) as space:
        space.build(img)
        got, n_cand = space.detect()
        assert n_cand == len(cand) and same(got, want), (len(got), n)
        assert same(space.extrema(), cand)
        again, _ = space.detect()
        assert same(again, want)                             # the same bytes on a second call
        room = np.zeros(n, pkg.capi.SIFT_KEYPOINT_DTYPE)
        room.view(np.uint8)[:] = 0xA7
        before = room.tobytes()
        with pytest.raises(pkg.LcmError) as e:
            space.detect(cap=n - 1, out=room)
        assert e.value.code == -4 and f"{n} keypoints" in str(e.value) and room.tobytes() == before     # the count, and nothing written
        fits, _ = space.detect(cap=n, out=room)
        assert same(np.ascontiguousarray(fits), want)
    one = matcher.sift_detect_image(img)
    assert same(np.ascontiguousarray(one), want)
    assert same(np.ascontiguousarray(matcher.sift_detect_image(img)), want)
    with pytest.raises(pkg.LcmError) as e:
        matcher.sift_detect_image(img, cap=n - 1)
    assert e.value.code == -4
    # the cached space follows the parameters and the size
    q = R.params(n_octave_layers=2, upsample=0)
    small = img[:97, :129]
    assert same(np.ascontiguousarray(matcher.sift_detect_image(small, sp_of(pkg, q))), R.detect(np.ascontiguousarray(small), q)[0])
    assert same(np.ascontiguousarray(matcher.sift_detect_image(img)), want)


def test_interleaved_with_a_store_search(pkg, scenes):
    """Detection and a search of the SIFT keyframe store alternate on one handle: neither changes the other's result."""
    img, want, _ = scenes["noise"]
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, (n, 128)).astype(np.uint8) for n in (300, 257, 64)]
    m = pkg.Matcher()
    try:
        for f in frames:
            m.l2_db_append(f)
        pairs = [(1, 0), (2, 0), (2, 1)]
        first = m.l2_db_score_pairs(pairs, 0.75)
        with m.sift_space(160, 120) as space:
            space.build(img)
            a, _ = space.detect()
            mid = m.l2_db_score_pairs(pairs, 0.75)
            b, _ = space.detect()
            one = m.sift_detect_image(img)
            last = m.l2_db_score_pairs(pairs, 0.75)
        assert same(a, want) and same(b, want) and same(np.ascontiguousarray(one), want)
        assert same(first, mid) and same(first, last)
    finally:
        m.close()
