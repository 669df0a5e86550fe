"""Deterministic inputs of the SIFT keypoint detector's tests: images (blobs, seeded noise, a ramp) and planted difference-of-Gaussians
stacks for the extrema search and for the refinement.  Every generator asserts, through the numpy restatement (siftref.py), that
what it meant to plant is there; the tests hold the device to the restatement on the same inputs."""
import numpy as np

import siftref as R

F = np.float32


# ---- images
def ramp_image(w, h, seed=0):
    """Every pixel different from its neighbours, the full uint8 range: shows a wrong fold, stride or tile at once."""
    rng = np.random.default_rng(1000 + seed)
    y, x = np.mgrid[0:h, 0:w]
    img = ((x * 7 + y * 13 + (x * y) % 11) % 256).astype(np.uint8)
    img[rng.integers(0, h, 8), rng.integers(0, w, 8)] = 255
    return img


def noise_image(w=160, h=120, seed=7):
    """Seeded noise, smoothed once by a 3 x 3 box so that extrema survive the contrast test."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h + 2, w + 2)).astype(np.float64)
    s = sum(a[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) / 9.0
    return np.clip(np.rint((s - 128.0) * 2.5 + 128.0), 0, 255).astype(np.uint8)


BLOBS = ((40, 36, 3.0, 90.0), (110, 40, 4.5, -80.0), (60, 88, 6.0, 100.0), (125, 90, 3.5, 85.0))     # x, y, sigma, amplitude


def blob_image(w=160, h=120, blobs=BLOBS):
    """Isotropic Gaussian blobs, bright and dark, on mid gray."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.full((h, w), 128.0)
    for bx, by, s, amp in blobs:
        a += amp * np.exp(-((x - bx) ** 2 + (y - by) ** 2) / (2.0 * s * s))
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


# ---- planted stacks for the extrema search: (stack (n + 2, h, w) float32, the candidates expected, in order)
def _expect(cands):
    out = np.zeros(len(cands), R.CAND_DTYPE)
    for i, c in enumerate(sorted(cands)):
        out[i] = c
    return out


def extrema_values(w, h, p):
    """The value conditions, far from each other: |v| == T is none and the next float above is one; a tie with one neighbour and
    with all 26; a negative extremum; a positive value below a larger neighbour is none."""
    n, b, T = p.n_octave_layers, p.border, R.threshold(p)
    d = np.zeros((n + 2, h, w), F)
    up = np.nextafter(T, F(np.inf))
    assert w >= 2 * b + 26 and h >= 2 * b + 5 and T >= 1
    r, want = b + 2, []
    d[1, r, b + 1] = T                                       # |v| == T: none
    d[1, r, b + 5] = up; want.append((0, 1, r, b + 5))       # the next float above
    d[1, r, b + 9] = -up; want.append((0, 1, r, b + 9))      # a negative extremum
    d[1, r, b + 13] = 9.0; d[1, r, b + 14] = 9.0             # a tie with one neighbour: both are candidates
    want += [(0, 1, r, b + 13), (0, 1, r, b + 14)]
    d[n, r, b + 18] = 5.0; d[n + 1, r, b + 18] = 6.0         # a larger neighbour in the layer above: none (and layer n + 1 never reports)
    d[0, r, b + 22] = 50.0                                   # layer 0 never reports
    d[n + 1, r, b + 24] = -50.0
    got = R.extrema([d], p)
    assert got.tolist() == _expect(want).tolist()
    return d, _expect(want)


def extrema_plateau(w, h, p, v=3.0):
    """Every value equal (a tie with all 26): every pixel inside the border is a candidate, on every layer 1 .. n; the count crosses
    the blocks' seams and, when large enough, the scan's carry."""
    n, b = p.n_octave_layers, p.border
    d = np.full((n + 2, h, w), v, F)
    want = [(0, l, r, c) for l in range(1, n + 1) for r in range(b, h - b) for c in range(b, w - b)]
    got = R.extrema([d], p)
    assert len(got) == len(want) == n * (w - 2 * b) * (h - 2 * b) and got.tolist() == _expect(want).tolist()
    return d, got


def extrema_border(w, h, p):
    """Single spikes on both sides of the border in x and in y: border - 1 / border and cols - border - 1 / cols - border."""
    n, b = p.n_octave_layers, p.border
    d = np.zeros((n + 2, h, w), F)
    assert w >= 2 * b + 4 and h >= 2 * b + 4
    mid_r, mid_c, want = h // 2, w // 2, []
    for c, inside in ((b - 1, False), (b, True), (w - b - 1, True), (w - b, False)):
        d[1, mid_r, c] = 40.0
        if inside:
            want.append((0, 1, mid_r, c))
    for r, inside in ((b - 1, False), (b, True), (h - b - 1, True), (h - b, False)):
        d[n, r, mid_c] = -40.0
        if inside:
            want.append((0, n, r, mid_c))
    got = R.extrema([d], p)
    assert got.tolist() == _expect(want).tolist()
    return d, got


def extrema_seams(w, h, p, block=256, tile=32):
    """Spikes on the last and the first pixel of every block of the search's linear order (layer, row, col) that lie inside the
    border, and on both sides of every multiple of the tile in x and y."""
    n, b = p.n_octave_layers, p.border
    d = np.zeros((n + 2, h, w), F)
    sites = set()
    for i in range(block - 1, n * h * w, block):
        for k in (i, i + 1):
            if k < n * h * w:
                l, rem = divmod(k, h * w)
                sites.add((l + 1, rem // w, rem % w))
    for e in range(tile, max(w, h), tile):
        for k in (e - 1, e):
            if k < w:
                sites.add((1, h // 2, k))
            if k < h:
                sites.add((n, k, w // 2))
    want = []
    for l, r, c in sorted(sites):
        if d[max(l - 1, 0):l + 2, max(r - 1, 0):r + 2, max(c - 1, 0):c + 2].any():
            continue                                         # keep spikes apart, so that each is an extremum on its own
        d[l, r, c] = 25.0 + l
        if b <= r < h - b and b <= c < w - b:
            want.append((0, l, r, c))
    got = R.extrema([d], p)
    assert got.tolist() == _expect(want).tolist() and len(want) >= 4
    return d, got


# ---- planted stacks for the refinement
def smooth_noise_stack(w, h, p, seed=3, amp=60.0):
    """A seeded smooth random field: its extrema converge at once, walk, leave the border or the layers, fail the contrast or the
    edge test.  The tests take the candidates from the device's own search."""
    n = p.n_octave_layers
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n + 4, h + 2, w + 2))
    s = sum(a[dl:dl + n + 2, dy:dy + h, dx:dx + w] for dl in range(3) for dy in range(3) for dx in range(3)) / 27.0
    return (s * amp).astype(F)


def plant(d, layer, row, col, cube):
    """cube[dl + 1][dy + 1][dx + 1] around (layer, row, col)."""
    d[layer - 1:layer + 2, row - 1:row + 2, col - 1:col + 2] = np.asarray(cube, F)


def refine_planted(w, h, p):
    """Hand-made neighbourhoods on a zero stack, 8 pixels apart: a plateau (a zero pivot), det == 0 with a regular H (the edge test's
    first clause), an isotropic peak (tr^2 == 4 det exactly: the edge test at equality when edge_threshold is 1), an ordinary peak
    a little off centre (kept).  Returns (stack, {name: (layer, row, col)})."""
    n, b = p.n_octave_layers, p.border
    assert w >= b + 40 and h >= 2 * b + 6 and n >= 1
    d = np.zeros((n + 2, h, w), F)
    r, sites = b + 3, {}
    v = 50.0
    plant(d, 1, r, b + 3, np.full((3, 3, 3), v)); sites["plateau"] = (1, r, b + 3)
    cube = np.full((3, 3, 3), v - 8.0)
    cube[1, 1, 1] = v; cube[1, 1, 0] = cube[1, 1, 2] = v - 4.0; cube[1, 0, 1] = cube[1, 2, 1] = v; cube[0, 1, 1] = cube[2, 1, 1] = v - 4.0
    cube[2, 2, 1], cube[2, 0, 1], cube[0, 2, 1], cube[0, 0, 1] = v - 2.0, v - 6.0, v - 6.0, v - 2.0
    plant(d, 1, r, b + 11, cube); sites["det0"] = (1, r, b + 11)
    cube = np.full((3, 3, 3), v - 12.0)
    cube[1, 1, 1] = v; cube[1, 1, 0] = cube[1, 1, 2] = cube[1, 0, 1] = cube[1, 2, 1] = cube[0, 1, 1] = cube[2, 1, 1] = v - 6.0
    plant(d, 1, r, b + 19, cube); sites["isotropic"] = (1, r, b + 19)
    cube = np.full((3, 3, 3), v - 14.0)
    cube[1, 1, 1] = v; cube[1, 1, 0], cube[1, 1, 2] = v - 7.0, v - 5.0; cube[1, 0, 1], cube[1, 2, 1] = v - 6.0, v - 8.0
    cube[0, 1, 1], cube[2, 1, 1] = v - 6.0, v - 7.0
    plant(d, 1, r, b + 27, cube); sites["peak"] = (1, r, b + 27)
    return d, sites


def reason_at(cand, why, site, octave=0):
    layer, row, col = site
    k = np.nonzero((cand["octave"] == octave) & (cand["layer"] == layer) & (cand["row"] == row) & (cand["col"] == col))[0]
    assert len(k) == 1, site
    return int(why[k[0]])


def steps_needed(D, cand, p, most=8):
    """Per candidate: the step at which its walk ends (converged, left, rejected by the solve), or most + 1."""
    out = np.full(len(cand), most + 1, np.int32)
    for k in range(most, 0, -1):
        q = R.params(**{**vars(p), "max_steps": k})
        _, why = R.refine(D, cand, q)
        out[why != R.NOT_CONVERGED] = k
    return out


def refine_walks(p, w=96, h=64, seed=6):
    """The smooth stack whose extrema, under the defaults, meet every fate but a zero pivot: kept after one step and after exactly
    max_steps steps, not converged, out of the border, off the layers, low contrast, an edge.  (stack, candidates, reasons)."""
    d = smooth_noise_stack(w, h, p, seed=seed)
    cand = R.extrema([d], p)
    _, why = R.refine([d], cand, p)
    return d, cand, why


def assert_walks_cover(d, cand, why, p):
    counts = np.bincount(why, minlength=8)
    for reason in (R.OK, R.LEFT, R.LEFT_LAYERS, R.NOT_CONVERGED, R.LOW_CONTRAST, R.EDGE):
        assert counts[reason] >= 1, (reason, counts)
    _, one = R.refine([d], cand, R.params(**{**vars(p), "max_steps": 1}))
    _, before = R.refine([d], cand, R.params(**{**vars(p), "max_steps": p.max_steps - 1}))
    assert np.sum(one == R.OK) >= 1                                             # converges in 1 step
    assert np.sum((why == R.OK) & (before == R.NOT_CONVERGED)) >= 1            # converges in exactly max_steps steps
    return counts


def assert_planted(d, sites, p):
    """What refine_planted means, under p (the defaults) and under edge_threshold 1 and 1.01."""
    cand = R.extrema([d], p)
    _, why = R.refine([d], cand, p)
    got = {k: reason_at(cand, why, v) for k, v in sites.items()}
    assert got == {"plateau": R.ZERO_PIVOT, "det0": R.EDGE, "isotropic": R.OK, "peak": R.OK}, got
    l, r, c = sites["isotropic"]
    v2 = d[l, r, c] * F(2.0)
    dxx, dyy = ((d[l, r, c + 1] + d[l, r, c - 1]) - v2) * R.SECOND_SCALE, ((d[l, r + 1, c] + d[l, r - 1, c]) - v2) * R.SECOND_SCALE
    tr, det = dxx + dyy, dxx * dyy
    assert (tr * tr) * F(1.0) == ((F(1.0) + F(1.0)) * (F(1.0) + F(1.0))) * det and det > 0          # equality, exactly
    _, at1 = R.refine([d], cand, R.params(**{**vars(p), "edge_threshold": 1.0}))
    _, above = R.refine([d], cand, R.params(**{**vars(p), "edge_threshold": 1.01}))
    assert reason_at(cand, at1, sites["isotropic"]) == R.EDGE and reason_at(cand, above, sites["isotropic"]) == R.OK
    l, r, c = sites["det0"]
    assert d[l, r + 1, c] == d[l, r, c] == d[l, r - 1, c]                       # dyy == 0 and dxy == 0: det == 0 with a regular H
    return cand, why
