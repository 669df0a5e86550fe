"""Numpy restatement of the SIFT keypoint detector's definition (include/lcm.h, lcm_sift_*; csrc/lcm_sift_host.h and
csrc/lcm_sift_device.h): the plan and its taps in double, then the base image, the blur, the difference-of-Gaussians layers, the
26-neighbour extrema and the sub-pixel refinement in float32, every product and every sum rounded on its own and summed in the
stated order.  The definition is modelled on OpenCV's detector; parity with cv::SIFT is unpinned (no OpenCV to compare with), so
this file, not OpenCV, is what the device is held to bit for bit.  The refinement is vectorised over the candidates of an octave."""
import math
from types import SimpleNamespace

import numpy as np

F = np.float32
DEFAULTS = dict(contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6, init_sigma=0.5, n_octave_layers=3, upsample=1, n_octaves=0,
                border=5, max_steps=5)
MAX_SIDE, MAX_OCTAVES, MAX_LAYERS, MAX_RADIUS = 4096, 16, 8, 48
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("response", "<f4"), ("xi", "<f4"), ("octave", "<i2"), ("layer", "<i2"),
                     ("col", "<i4"), ("row", "<i4")])
CAND_DTYPE = np.dtype([("octave", "<i4"), ("layer", "<i4"), ("row", "<i4"), ("col", "<i4")])
# why the refinement dropped a candidate
OK, ZERO_PIVOT, TOO_FAR, LEFT, NOT_CONVERGED, LOW_CONTRAST, EDGE = range(7)
LEFT_LAYERS = 7                                            # LEFT, told apart here: the walk left layers 1 .. n (the device says LEFT for both)
IMG_SCALE = F(1.0) / F(255.0)
DERIV_SCALE, SECOND_SCALE, CROSS_SCALE = IMG_SCALE * F(0.5), IMG_SCALE, IMG_SCALE * F(0.25)
X_LIMIT = F(715827882.0)                                   # INT_MAX / 3, rounded to float
LN2 = F(0.693147182)
EXP_COEF = [F(1.0 / math.factorial(k)) for k in range(9)]  # the size's 2^f = exp(f ln 2), Taylor to the 8th power, Horner in float


def params(**over):
    p = dict(DEFAULTS)
    for k, v in over.items():
        if k not in p:
            raise TypeError(k)
        p[k] = v
    return SimpleNamespace(**p)


def params_problem(p):
    for k in ("contrast_threshold", "edge_threshold", "sigma", "init_sigma"):
        v = getattr(p, k)
        if not (math.isfinite(v) and v > 0):
            return k
    if not 1 <= p.n_octave_layers <= MAX_LAYERS:
        return "n_octave_layers"
    if p.border < 1 or p.max_steps < 1 or p.n_octaves < 0 or p.n_octaves > MAX_OCTAVES or p.upsample not in (0, 1):
        return "border, max_steps, n_octaves or upsample"
    return None


def cv_round(x):
    return int(np.rint(x))                                 # half to even, as cvRound


def radius(sig):
    return (cv_round(8.0 * sig + 1.0) | 1) // 2


def taps(sig):
    r = radius(sig)
    t = [math.exp(-float(x * x) / (2.0 * sig * sig)) for x in range(-r, r + 1)]
    s = 0.0
    for v in t:
        s += v
    return np.array([v / s for v in t], np.float64).astype(F)


def plan(w, h, p):
    """None where the definition refuses; else the octave count, the sizes, the sigmas, the radii and the taps."""
    if params_problem(p) or not (1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE):
        return None
    bw, bh = (2 * w, 2 * h) if p.upsample else (w, h)
    n_oct = p.n_octaves if p.n_octaves > 0 else cv_round(math.log2(min(bw, bh)) - 2.0) + (1 if p.upsample else 0)
    if n_oct < 1 or n_oct > MAX_OCTAVES or (min(bw, bh) >> (n_oct - 1)) < 1:
        return None
    n = p.n_octave_layers
    k = math.pow(2.0, 1.0 / n)
    sig = [p.sigma]
    for i in range(1, n + 3):
        prev = p.sigma * math.pow(k, float(i - 1))
        total = prev * k
        sig.append(math.sqrt(total * total - prev * prev))
    a = 2.0 * p.init_sigma if p.upsample else p.init_sigma
    first = math.sqrt(max(p.sigma * p.sigma - a * a, 0.01))
    rad = [0] + [radius(s) for s in sig[1:]]
    if max(rad + [radius(first)]) > MAX_RADIUS:
        return None
    return SimpleNamespace(n_octaves=n_oct, n_gauss=n + 3, n_dog=n + 2, base_w=bw, base_h=bh, width=[bw >> o for o in range(n_oct)],
                           height=[bh >> o for o in range(n_oct)], sig=sig, first_sigma=first, radius=rad, first_radius=radius(first),
                           taps=[None] + [taps(s) for s in sig[1:]], first_taps=taps(first))


def fold(i, n):
    """Reflect-101: the index i of a line of n pixels, folded with period 2 (n - 1) until it is inside."""
    if n == 1:
        return np.zeros_like(np.asarray(i))
    q = np.mod(np.asarray(i), 2 * (n - 1))
    return np.where(q < n, q, 2 * (n - 1) - q)


def upsample2(a):
    h, w = a.shape

    def line(n):
        d = np.arange(2 * n)
        k, even = d // 2, d % 2 == 0
        return (np.where(even, np.maximum(k - 1, 0), k), np.where(even, k, np.minimum(k + 1, n - 1)),
                np.where(even, F(0.25), F(0.75)).astype(F), np.where(even, F(0.75), F(0.25)).astype(F))

    x0, x1, wx0, wx1 = line(w)
    y0, y1, wy0, wy1 = line(h)
    rows = wx0[None, :] * a[:, x0] + wx1[None, :] * a[:, x1]
    return wy0[:, None] * rows[y0, :] + wy1[:, None] * rows[y1, :]


def base_image(img, p):
    a = np.ascontiguousarray(img, np.uint8).astype(F)
    return upsample2(a) if p.upsample else a


def blur(src, t):
    r, (h, w) = len(t) // 2, src.shape
    xi = fold(np.arange(-r, w + r), w)
    tmp = t[0] * src[:, xi[0:w]]
    for j in range(1, 2 * r + 1):
        tmp = tmp + t[j] * src[:, xi[j:j + w]]
    yi = fold(np.arange(-r, h + r), h)
    dst = t[0] * tmp[yi[0:h], :]
    for j in range(1, 2 * r + 1):
        dst = dst + t[j] * tmp[yi[j:j + h], :]
    assert dst.dtype == F
    return dst


def build(img, p, pl=None):
    """(plan, G, D): G[o] is (n + 3, h_o, w_o), D[o] is (n + 2, h_o, w_o), float32."""
    h, w = img.shape
    pl = pl or plan(w, h, p)
    n = p.n_octave_layers
    G, D = [], []
    for o in range(pl.n_octaves):
        g = [blur(base_image(img, p), pl.first_taps) if o == 0 else np.ascontiguousarray(G[o - 1][n][::2, ::2][:pl.height[o], :pl.width[o]])]
        for i in range(1, n + 3):
            g.append(blur(g[i - 1], pl.taps[i]))
        G.append(np.stack(g))
        D.append(G[o][1:] - G[o][:-1])
        assert G[o].shape == (n + 3, pl.height[o], pl.width[o]) and D[o].dtype == F
    return pl, G, D


def threshold(p):
    return F(math.floor(0.5 * p.contrast_threshold / p.n_octave_layers * 255.0))


def extrema(D, p):
    """Candidates {octave, layer, row, col} in ascending order."""
    T, n, b, out = threshold(p), p.n_octave_layers, p.border, []
    for o, d in enumerate(D):
        h, w = d.shape[1:]
        if h <= 2 * b or w <= 2 * b:
            continue
        for l in range(1, n + 1):
            c = d[l, b:h - b, b:w - b]
            nb = [d[l + dl, b + dy:h - b + dy, b + dx:w - b + dx] for dl in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                  if (dl, dy, dx) != (0, 0, 0)]
            mx, mn = np.maximum.reduce(nb), np.minimum.reduce(nb)
            rows, cols = np.nonzero((np.abs(c) > T) & (((c > 0) & (c >= mx)) | ((c < 0) & (c <= mn))))
            out += [(o, l, r + b, x + b) for r, x in zip(rows, cols)]
    return np.array(out, CAND_DTYPE) if out else np.zeros(0, CAND_DTYPE)


def solve3(A, b):
    """A x = b by Gaussian elimination with partial pivoting (largest |.|, first of equals), float32; (x, a pivot was zero)."""
    A, b = A.copy(), b.copy()
    idx, zero = np.arange(len(b)), np.zeros(len(b), bool)
    with np.errstate(all="ignore"):
        for k in range(3):
            p = k + np.argmax(np.abs(A[:, k:, k]), axis=1)
            zero |= A[idx, p, k] == 0
            Ak, Ap, bk, bp = A[idx, k, :].copy(), A[idx, p, :].copy(), b[idx, k].copy(), b[idx, p].copy()
            A[idx, k, :], A[idx, p, :], b[idx, k], b[idx, p] = Ap, Ak, bp, bk
            for i in range(k + 1, 3):
                f = A[:, i, k] / A[:, k, k]
                for j in range(k + 1, 3):
                    A[:, i, j] = A[:, i, j] - f * A[:, k, j]
                b[:, i] = b[:, i] - f * b[:, k]
        x2 = b[:, 2] / A[:, 2, 2]
        x1 = (b[:, 1] - A[:, 1, 2] * x2) / A[:, 1, 1]
        x0 = ((b[:, 0] - A[:, 0, 1] * x1) - A[:, 0, 2] * x2) / A[:, 0, 0]
    assert x0.dtype == F
    return np.stack([x0, x1, x2], axis=1), zero


def pow2_frac(e):
    """2^e for the size, float32: k = rint(e), f = e - k, the Taylor polynomial of exp(f ln 2) by Horner, times 2^k."""
    k = np.rint(e)
    x = (e - k) * LN2
    acc = np.full_like(x, EXP_COEF[8])
    for c in EXP_COEF[7::-1]:
        acc = c + x * acc
    return acc * np.ldexp(F(1.0), k.astype(np.int32)).astype(F)


def refine_octave(d, o, layer, row, col, p):
    """The refinement of the candidates (layer, row, col) of ONE octave over its DoG stack d (n + 2, h, w): (records, reasons)."""
    n, b, (h, w) = p.n_octave_layers, p.border, d.shape[1:]
    N = len(layer)
    l, r, c = (np.array(v, np.int64) for v in (layer, row, col))
    reason = np.full(N, NOT_CONVERGED, np.int32)
    live = np.ones(N, bool)                                  # still walking
    done = np.zeros(N, bool)
    X = np.zeros((N, 3), F)
    dD = np.zeros((N, 3), F)
    H2 = np.zeros((N, 3), F)                                 # dxx, dyy, dxy at the last position
    with np.errstate(all="ignore"):
        for _ in range(p.max_steps):
            a = np.nonzero(live)[0]
            if len(a) == 0:
                break
            la, ra, ca = l[a], r[a], c[a]
            at = lambda dl, dy, dx: d[la + dl, ra + dy, ca + dx]                # noqa: E731
            g = np.stack([(at(0, 0, 1) - at(0, 0, -1)) * DERIV_SCALE, (at(0, 1, 0) - at(0, -1, 0)) * DERIV_SCALE,
                          (at(1, 0, 0) - at(-1, 0, 0)) * DERIV_SCALE], axis=1)
            v2 = at(0, 0, 0) * F(2.0)
            dxx = ((at(0, 0, 1) + at(0, 0, -1)) - v2) * SECOND_SCALE
            dyy = ((at(0, 1, 0) + at(0, -1, 0)) - v2) * SECOND_SCALE
            dss = ((at(1, 0, 0) + at(-1, 0, 0)) - v2) * SECOND_SCALE
            dxy = (((at(0, 1, 1) - at(0, 1, -1)) - at(0, -1, 1)) + at(0, -1, -1)) * CROSS_SCALE
            dxs = (((at(1, 0, 1) - at(1, 0, -1)) - at(-1, 0, 1)) + at(-1, 0, -1)) * CROSS_SCALE
            dys = (((at(1, 1, 0) - at(1, -1, 0)) - at(-1, 1, 0)) + at(-1, -1, 0)) * CROSS_SCALE
            A = np.stack([np.stack([dxx, dxy, dxs], 1), np.stack([dxy, dyy, dys], 1), np.stack([dxs, dys, dss], 1)], 1)
            sol, zero = solve3(A, g)
            x = -sol
            X[a], dD[a], H2[a] = x, g, np.stack([dxx, dyy, dxy], 1)
            ax = np.abs(x)
            conv = ~zero & (ax[:, 0] < F(0.5)) & (ax[:, 1] < F(0.5)) & (ax[:, 2] < F(0.5))
            far = ~zero & ~conv & ~((ax[:, 0] <= X_LIMIT) & (ax[:, 1] <= X_LIMIT) & (ax[:, 2] <= X_LIMIT))
            move = ~zero & ~conv & ~far
            reason[a[zero]] = ZERO_PIVOT
            reason[a[far]] = TOO_FAR
            done[a[conv]] = True
            live[a[zero | far | conv]] = False
            m = a[move]
            step = np.rint(x[move]).astype(np.int64)
            c[m] += step[:, 0]; r[m] += step[:, 1]; l[m] += step[:, 2]
            off = (l[m] < 1) | (l[m] > n)
            out = off | (c[m] < b) | (c[m] >= w - b) | (r[m] < b) | (r[m] >= h - b)
            reason[m[out]] = np.where(off[out], LEFT_LAYERS, LEFT)
            live[m[out]] = False
        k = np.nonzero(done)[0]
        t = (dD[k, 0] * X[k, 0] + dD[k, 1] * X[k, 1]) + dD[k, 2] * X[k, 2]
        contr = d[l[k], r[k], c[k]] * IMG_SCALE + t * F(0.5)
        low = np.abs(contr) * F(n) < F(p.contrast_threshold)
        dxx, dyy, dxy = H2[k, 0], H2[k, 1], H2[k, 2]
        tr, det = dxx + dyy, dxx * dyy - dxy * dxy
        et = F(p.edge_threshold)
        edge = ~low & ((det <= 0) | ((tr * tr) * et >= ((et + F(1.0)) * (et + F(1.0))) * det))
        reason[k] = np.where(low, LOW_CONTRAST, np.where(edge, EDGE, OK))
        keep = ~low & ~edge
        k, contr = k[keep], contr[keep]
        scale = F(2.0 ** o) * (F(0.5) if p.upsample else F(1.0))
        rec = np.zeros(len(k), KP_DTYPE)
        rec["x"] = (c[k].astype(F) + X[k, 0]) * scale
        rec["y"] = (r[k].astype(F) + X[k, 1]) * scale
        rec["size"] = (F(p.sigma) * pow2_frac((l[k].astype(F) + X[k, 2]) / F(n))) * (scale * F(2.0))
        rec["response"], rec["xi"] = np.abs(contr), X[k, 2]
        rec["octave"], rec["layer"], rec["col"], rec["row"] = o, l[k], c[k], r[k]
    return rec, reason


def refine(D, cand, p):
    """Survivors in candidate order, and every candidate's reason."""
    recs, reasons = [], np.zeros(len(cand), np.int32)
    for o in sorted(set(cand["octave"].tolist())):
        sel = np.nonzero(cand["octave"] == o)[0]
        rec, why = refine_octave(D[o], o, cand["layer"][sel], cand["row"][sel], cand["col"][sel], p)
        recs.append(rec)
        reasons[sel] = why
    return (np.concatenate(recs) if recs else np.zeros(0, KP_DTYPE)), reasons


def detect(img, p):
    pl, G, D = build(np.asarray(img), p)
    cand = extrema(D, p)
    kp, why = refine(D, cand, p)
    return kp, cand, why
