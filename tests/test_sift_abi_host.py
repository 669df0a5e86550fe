"""The SIFT keypoint detector's C surface without a device (include/lcm.h, lcm_sift_*): declarations, exports and ctypes entries, the
records' layouts (also by the C compiler), the defaults, every refusal that needs no device (each writing nothing), LCM_ERR_NO_DEVICE
from the calls that would make a space, and lcm_sift_plan == siftref.plan: counts, sizes, sigmas and radii exact, taps bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import siftref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("lcm_sift_params_default", "lcm_sift_plan", "lcm_sift_plan_read", "lcm_sift_space_create", "lcm_sift_space_destroy",
         "lcm_sift_space_build", "lcm_sift_space_info", "lcm_sift_space_read", "lcm_sift_space_write", "lcm_sift_extrema", "lcm_sift_detect",
         "lcm_sift_detect_image")
FILL = 0xA7
INVALID, NO_DEVICE, CAPACITY = -1, -2, -4


def header():
    txt = open(os.path.join(ROOT, "include", "lcm.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def no_device(lib):
    return lib.lcm_device_count() == 0


def test_every_call_is_declared_exported_and_bound(pkg):
    declared = set(re.findall(r"LCM_API\s+[\w\s\*]+?\b(lcm_sift_\w+)\s*\(", header()))
    assert declared - {"lcm_sift_pack_f32"} == set(CALLS)       # the descriptor rows' packing is the matcher's (lcm_l2_*)
    lib = C.CDLL(pkg.capi.LIB_PATH)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in pkg.capi._SIGNATURES, name
    assert callable(pkg.Matcher.sift_space) and callable(pkg.Matcher.sift_detect_image)
    for name in ("build", "info", "read", "write", "extrema", "detect", "close"):
        assert callable(getattr(pkg.capi.SiftSpace, name)), name
    raw = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "lcm.h")).read().replace("\n *", " "))
    for words in ("parity with cv::SIFT is unpinned", "every product and every sum rounded on its own", "the first of equals", "half to even",
                  "folded with period 2 (n - 1)", "no atomic cursor", "invalidates nothing else", "All device memory is allocated here, once",
                  "cv::undistort, the orientation histogram", "(2 x, 2 y)"):
        assert words in raw, words


def test_record_layouts(pkg):
    c = pkg.capi
    assert (C.sizeof(c.SiftParams), C.sizeof(c.SiftPlanInfo), c.SIFT_KEYPOINT_DTYPE.itemsize, c.SIFT_CANDIDATE_DTYPE.itemsize) == (64, 320, 32, 16)
    assert [getattr(c.SiftParams, f).offset for f in ("contrast_threshold", "edge_threshold", "sigma", "init_sigma", "n_octave_layers", "upsample",
                                                      "n_octaves", "border", "max_steps", "reserved")] == [0, 8, 16, 24, 32, 36, 40, 44, 48, 52]
    assert [c.SIFT_KEYPOINT_DTYPE.fields[f][1] for f in ("x", "y", "size", "response", "xi", "octave", "layer", "col", "row")] == \
        [0, 4, 8, 12, 16, 20, 22, 24, 28]
    assert c.SIFT_KEYPOINT_DTYPE == R.KP_DTYPE and c.SIFT_CANDIDATE_DTYPE == R.CAND_DTYPE
    assert [getattr(c.SiftPlanInfo, f).offset for f in ("n_octaves", "width", "height", "radius", "first_sigma", "sig", "space_floats")] == \
        [0, 32, 96, 160, 208, 216, 312]
    assert (c.SIFT_MAX_SIDE, c.SIFT_MAX_OCTAVES, c.SIFT_MAX_RADIUS, c.SIFT_MAX_CANDIDATES) == (R.MAX_SIDE, R.MAX_OCTAVES, R.MAX_RADIUS, 1 << 20)
    assert (c.SIFT_GAUSSIAN, c.SIFT_DOG) == (0, 1)


def test_the_c_compiler_agrees_on_the_layouts(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "lcm.h"\n'
                   "_Static_assert(sizeof(lcm_sift_params) == 64 && sizeof(lcm_sift_plan_info) == 320 && sizeof(lcm_sift_keypoint) == 32 && "
                   "sizeof(lcm_sift_candidate) == 16 && sizeof(lcm_sift_space_info_t) == 352, \"sizes\");\n"
                   "_Static_assert(offsetof(lcm_sift_keypoint, xi) == 16 && offsetof(lcm_sift_keypoint, octave) == 20 && "
                   "offsetof(lcm_sift_keypoint, layer) == 22 && offsetof(lcm_sift_keypoint, col) == 24 && offsetof(lcm_sift_keypoint, row) == 28, \"keypoint\");\n"
                   "_Static_assert(offsetof(lcm_sift_params, n_octave_layers) == 32 && offsetof(lcm_sift_params, max_steps) == 48 && "
                   "offsetof(lcm_sift_plan_info, radius) == 160 && offsetof(lcm_sift_plan_info, space_floats) == 312 && "
                   "offsetof(lcm_sift_space_info_t, plan) == 32, \"records\");\n"
                   "_Static_assert(LCM_SIFT_GAUSSIAN == 0 && LCM_SIFT_DOG == 1 && LCM_SIFT_MAX_SIDE == 4096 && LCM_SIFT_MAX_OCTAVES == 16 && "
                   "LCM_SIFT_MAX_RADIUS == 48 && LCM_SIFT_MAX_CANDIDATES == 1048576, \"constants\");\n"
                   "int main(void) { return 0; }\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_defaults(pkg):
    p = pkg.capi.SiftParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    pkg.load_library().lcm_sift_params_default(C.byref(p))
    assert all(getattr(p, k) == v for k, v in R.DEFAULTS.items()) and len(R.DEFAULTS) == 9 and list(p.reserved) == [0, 0, 0]
    pkg.load_library().lcm_sift_params_default(None)                           # no-op
    q = pkg.capi.default_sift_params(n_octave_layers=5, upsample=0)
    assert (q.n_octave_layers, q.upsample, q.sigma) == (5, 0, 1.6)
    with pytest.raises(TypeError):
        pkg.capi.default_sift_params(octaves=3)


SIZES = ((17, 13), (64, 64), (65, 63), (129, 97), (200, 37), (37, 200), (160, 120), (640, 480), (1920, 1080), (4096, 4096), (4, 4))
OVERS = ({}, {"upsample": 0}, {"n_octave_layers": 2}, {"n_octave_layers": 5}, {"n_octave_layers": 1}, {"n_octave_layers": 8, "upsample": 0},
         {"n_octaves": 3}, {"sigma": 1.2, "init_sigma": 0.8})


def test_the_plan_equals_the_restatement(pkg):
    """Counts, sizes, sigmas and radii exact; taps bit for bit (the host's exp and numpy's are the same libm here; a tap may differ
    by one float ulp where they are not, and the test says which)."""
    c = pkg.capi
    differing = []
    for w, h in SIZES:
        for over in OVERS:
            want, sp = R.plan(w, h, R.params(**over)), c.default_sift_params(**over)
            if want is None:
                with pytest.raises(pkg.LcmError):
                    c.sift_plan(w, h, sp)
                continue
            got = c.sift_plan(w, h, sp)
            n_oct, n_g = want.n_octaves, want.n_gauss
            assert (got.n_octaves, got.n_gauss, got.n_dog, got.base_w, got.base_h) == (n_oct, n_g, want.n_dog, want.base_w, want.base_h)
            assert list(got.width[:n_oct]) == want.width and list(got.height[:n_oct]) == want.height and not any(got.width[n_oct:])
            assert list(got.radius[:n_g]) == want.radius and got.first_radius == want.first_radius and got.max_radius == max(want.radius + [want.first_radius])
            assert list(got.sig[:n_g]) == want.sig and got.first_sigma == want.first_sigma
            assert got.space_floats == want.base_w * want.base_h + (2 * (n_g - 3) + 5) * sum(a * b for a, b in zip(want.width, want.height))
            for layer in [-1] + list(range(1, n_g)):
                t, ref = c.sift_plan_taps(w, h, layer, sp), want.first_taps if layer == -1 else want.taps[layer]
                assert len(t) == len(ref)
                if t.tobytes() != ref.tobytes():
                    ulps = np.abs(t.view(np.int32) - ref.view(np.int32))
                    assert ulps.max() <= 1, (w, h, over, layer)
                    differing.append((w, h, over, layer, np.nonzero(ulps)[0].tolist()))
    print("taps that differ by one float ulp:", differing or "none")


def test_refusals_that_need_no_device_write_nothing(pkg):
    c, lib = pkg.capi, pkg.load_library()
    sp = c.default_sift_params()
    fake = C.c_void_p(0x10)                                  # a handle that is never dereferenced: the host checks come first
    out = c.SiftPlanInfo()
    C.memset(C.byref(out), FILL, C.sizeof(out))
    taps, n = np.full(128, FILL, np.uint8).view(np.float32), C.c_int(-7)
    space = C.c_void_p(0x55)
    img = np.zeros((64, 64), np.uint8)
    kp, cnt = np.full(64 * 32, FILL, np.uint8), C.c_size_t(77)
    bad = [dict(sigma=0.0), dict(sigma=float("nan")), dict(contrast_threshold=-0.04), dict(edge_threshold=float("inf")), dict(init_sigma=0.0),
           dict(n_octave_layers=0), dict(n_octave_layers=9), dict(border=0), dict(max_steps=0), dict(n_octaves=17), dict(n_octaves=-1), dict(upsample=2)]
    for over in bad:
        q = c.default_sift_params(**over)
        assert lib.lcm_sift_plan(64, 64, C.byref(q), C.byref(out)) == INVALID, over
        assert lib.lcm_sift_plan_read(64, 64, C.byref(q), 1, taps.ctypes.data, 32, C.byref(n)) == INVALID, over
        assert lib.lcm_sift_space_create(fake, 64, 64, C.byref(q), C.byref(space)) == INVALID and not space.value, over
        space.value = 0x55
        assert lib.lcm_sift_detect_image(fake, img.ctypes.data, 64, 64, 64, C.byref(q), kp.ctypes.data, 64, C.byref(cnt)) == INVALID, over
    for w, h, code in ((0, 64, INVALID), (64, -1, INVALID), (4097, 64, CAPACITY), (64, 4097, CAPACITY)):
        assert lib.lcm_sift_plan(w, h, C.byref(sp), C.byref(out)) == code, (w, h)
        assert lib.lcm_sift_space_create(fake, w, h, C.byref(sp), C.byref(space)) == code and not space.value, (w, h)
        space.value = 0x55
    no_up = c.default_sift_params(upsample=0)
    assert lib.lcm_sift_plan(5, 5, C.byref(no_up), C.byref(out)) == INVALID                 # no octave
    assert lib.lcm_sift_plan(8, 8, C.byref(c.default_sift_params(n_octaves=6)), C.byref(out)) == INVALID
    assert lib.lcm_sift_plan(64, 64, C.byref(c.default_sift_params(n_octave_layers=1, sigma=2.0)), C.byref(out)) == CAPACITY       # radius 56
    assert lib.lcm_sift_plan(64, 64, C.byref(sp), None) == INVALID
    assert lib.lcm_sift_plan_read(64, 64, C.byref(sp), 0, taps.ctypes.data, 32, C.byref(n)) == INVALID          # layer 0 is not blurred from a layer
    assert lib.lcm_sift_plan_read(64, 64, C.byref(sp), 6, taps.ctypes.data, 32, C.byref(n)) == INVALID
    assert lib.lcm_sift_plan_read(64, 64, C.byref(sp), 1, None, 32, C.byref(n)) == INVALID and n.value == -7
    assert lib.lcm_sift_plan_read(64, 64, C.byref(sp), 5, taps.ctypes.data, 26, C.byref(n)) == CAPACITY and n.value == 27
    assert bytes(out) == bytes([FILL]) * C.sizeof(out) and (taps.view(np.uint8) == FILL).all()
    # a NULL handle, a NULL space, NULL buffers
    assert lib.lcm_sift_space_create(None, 64, 64, C.byref(sp), C.byref(space)) == INVALID and not space.value
    assert lib.lcm_sift_space_create(fake, 64, 64, C.byref(sp), None) == INVALID
    assert lib.lcm_sift_detect_image(None, img.ctypes.data, 64, 64, 64, None, kp.ctypes.data, 64, C.byref(cnt)) == INVALID
    assert lib.lcm_sift_detect_image(fake, None, 64, 64, 64, None, kp.ctypes.data, 64, C.byref(cnt)) == INVALID
    assert lib.lcm_sift_detect_image(fake, img.ctypes.data, 64, 64, 63, None, kp.ctypes.data, 64, C.byref(cnt)) == INVALID      # stride < w
    assert lib.lcm_sift_detect_image(fake, img.ctypes.data, 64, 64, 64, None, None, 64, C.byref(cnt)) == INVALID
    assert lib.lcm_sift_detect_image(fake, img.ctypes.data, 64, 64, 64, None, kp.ctypes.data, 64, None) == INVALID
    info = c.SiftSpaceInfo()
    assert lib.lcm_sift_space_build(None, img.ctypes.data, 64, 64, 64) == INVALID
    assert lib.lcm_sift_space_info(None, C.byref(info)) == INVALID
    assert lib.lcm_sift_space_read(None, 0, 0, 0, kp.ctypes.data) == INVALID and lib.lcm_sift_space_write(None, 1, 0, 0, kp.ctypes.data) == INVALID
    assert lib.lcm_sift_extrema(None, kp.ctypes.data, 4, C.byref(cnt)) == INVALID
    assert lib.lcm_sift_detect(None, kp.ctypes.data, 4, C.byref(cnt), None) == INVALID
    lib.lcm_sift_space_destroy(None)                         # no-op
    assert lib.lcm_last_error() != b""
    assert (kp == FILL).all() and cnt.value == 77


def test_no_device_no_space(pkg):
    """Without a device the calls that would make a space say LCM_ERR_NO_DEVICE, after the host checks and before the handle is
    looked at; with one, the same calls are exercised by tests/test_gpu_sift.py."""
    c, lib = pkg.capi, pkg.load_library()
    if not no_device(lib):
        return                                               # with a device the refusal cannot arise
    fake, space = C.c_void_p(0x10), C.c_void_p(0x55)
    img, kp, cnt = np.zeros((64, 64), np.uint8), np.full(64 * 32, FILL, np.uint8), C.c_size_t(77)
    assert lib.lcm_sift_space_create(fake, 64, 64, None, C.byref(space)) == NO_DEVICE and not space.value
    assert b"no CPU fallback" in lib.lcm_last_error()
    assert lib.lcm_sift_detect_image(fake, img.ctypes.data, 64, 64, 64, None, kp.ctypes.data, 64, C.byref(cnt)) == NO_DEVICE
    assert (kp == FILL).all() and cnt.value == 77
