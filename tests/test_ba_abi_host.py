"""The bundle adjustment's C surface without a device (include/lcm.h, lcm_ba_*): declarations, exports and ctypes entries, the
records' layouts (also by the C compiler), the defaults, the three host-only calls (lcm_ba_params_default, lcm_ba_compact,
lcm_ba_add_loop_observations) against tests/baref.py and a walk of src/main.cpp:1633-1659 and :1496-1513, the refusals that need no
handle, and the pure host functions (csrc/lcm_ba_host.h) with the host-compiled arithmetic (csrc/lcm_ba_device.h) as a
stand-alone program under ASan + UBSan.  Nothing loaded into Python runs under a sanitizer."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bacases as S
import baref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-loop-closing_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
HIP_INCLUDE = "/opt/rocm/include"          # lcm_ba_device.h includes hip_runtime.h: as plain C++ its markers expand to nothing
CALLS = ("lcm_ba_params_default", "lcm_ba_error", "lcm_ba_refine_cameras", "lcm_ba_refine_points", "lcm_ba_step_cameras", "lcm_ba_step_points",
         "lcm_ba_optimize", "lcm_ba_outliers", "lcm_ba_compact", "lcm_ba_add_loop_observations", "lcm_ba_refine_map")
FILL = 0xA7


def header():
    txt = open(os.path.join(ROOT, "include", "lcm.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_every_call_is_declared_exported_and_bound(pkg):
    declared = set(re.findall(r"LCM_API\s+[\w\s\*]+?\b(lcm_ba_\w+)\s*\(", header()))
    assert declared == set(CALLS)
    lib = C.CDLL(pkg.capi.LIB_PATH)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in pkg.capi._SIGNATURES, name
    for name in ("ba_error", "ba_refine_cameras", "ba_refine_points", "ba_step_cameras", "ba_step_points", "ba_optimize", "ba_outliers",
                 "ba_refine_map"):
        assert callable(getattr(pkg.Matcher, name)), name
    raw = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "lcm.h")).read().replace("\n *", " "))
    for words in ("There is no test on z", "absolute, not scaled by the trace", "come back byte for byte", "depends neither on min_update nor on inner_iters",
                  "does not enter the maximum", "decided from the counts before any buffer is read"):
        assert words in raw, words


def test_record_layouts(pkg):
    c = pkg.capi
    assert (C.sizeof(c.BaParams), C.sizeof(c.BaInfo), C.sizeof(c.BaMapReport)) == (112, 184, 56)
    assert (c.BA_POINT_DTYPE.itemsize, c.BA_OBS_DTYPE.itemsize, c.BA_ELEM_INFO_DTYPE.itemsize) == (24, 24, 24)
    p = c.BaParams
    assert [getattr(p, f).offset for f in ("fx", "fy", "cx", "cy", "eps", "damping", "min_update", "outlier_px", "min_spread", "spread_factor",
                                           "outer_iters", "inner_iters", "min_cam_obs", "min_point_obs", "reserved")] == \
        [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 84, 88, 92, 96]
    assert [getattr(c.BaInfo, f).offset for f in ("mean_error", "outer_iters", "cameras", "points", "reserved")] == [0, 136, 140, 160, 180]
    assert [getattr(c.BaMapReport, f).offset for f in ("error_before", "error_after", "error_filtered", "error_final", "threshold", "n_outliers",
                                                       "n_points", "n_obs", "reserved")] == [0, 8, 16, 24, 32, 40, 44, 48, 52]
    assert [c.BA_POINT_DTYPE.fields[f][1] for f in ("x", "y", "z")] == [0, 8, 16]
    assert [c.BA_OBS_DTYPE.fields[f][1] for f in ("cam", "point", "u", "v")] == [0, 4, 8, 16]
    assert [c.BA_ELEM_INFO_DTYPE.fields[f][1] for f in ("last_update", "cost", "iterations", "status")] == [0, 8, 16, 20]
    assert (c.BA_CONVERGED, c.BA_MAX_ITERS, c.BA_SOLVE_FAILED, c.BA_HALF_TURN, c.BA_SKIPPED) == (0, 1, 2, 3, 4)
    assert (c.BA_CONVERGED, c.BA_MAX_ITERS, c.BA_SOLVE_FAILED, c.BA_HALF_TURN) == (c.PGO_CONVERGED, c.PGO_MAX_ITERS, c.PGO_SOLVE_FAILED, c.PGO_HALF_TURN)
    assert (c.BA_MAX_CAMERAS, c.BA_MAX_POINTS, c.BA_MAX_OBS) == (4096, 1 << 24, 1 << 24)


def test_the_c_compiler_agrees_on_the_layouts(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "lcm.h"\n'
                   "_Static_assert(sizeof(lcm_ba_point) == 24 && sizeof(lcm_ba_obs) == 24 && sizeof(lcm_ba_elem_info) == 24 && "
                   "sizeof(lcm_ba_params) == 112 && sizeof(lcm_ba_info) == 184 && sizeof(lcm_ba_map_report) == 56 && sizeof(lcm_pgo_pose) == 96, \"sizes\");\n"
                   "_Static_assert(offsetof(lcm_ba_obs, point) == 4 && offsetof(lcm_ba_obs, u) == 8 && offsetof(lcm_ba_obs, v) == 16 && "
                   "offsetof(lcm_ba_elem_info, cost) == 8 && offsetof(lcm_ba_elem_info, iterations) == 16 && offsetof(lcm_ba_elem_info, status) == 20, \"records\");\n"
                   "_Static_assert(offsetof(lcm_ba_params, eps) == 32 && offsetof(lcm_ba_params, outlier_px) == 56 && offsetof(lcm_ba_params, outer_iters) == 80 && "
                   "offsetof(lcm_ba_params, min_point_obs) == 92 && offsetof(lcm_ba_params, reserved) == 96, \"params\");\n"
                   "_Static_assert(offsetof(lcm_ba_info, outer_iters) == 136 && offsetof(lcm_ba_info, cameras) == 140 && offsetof(lcm_ba_info, points) == 160 && "
                   "offsetof(lcm_ba_map_report, threshold) == 32 && offsetof(lcm_ba_map_report, n_outliers) == 40 && offsetof(lcm_ba_map_report, n_obs) == 48, \"info\");\n"
                   "_Static_assert(LCM_BA_CONVERGED == 0 && LCM_BA_MAX_ITERS == 1 && LCM_BA_SOLVE_FAILED == 2 && LCM_BA_HALF_TURN == 3 && LCM_BA_SKIPPED == 4 && "
                   "LCM_BA_MAX_CAMERAS == 4096 && LCM_BA_MAX_POINTS == 16777216 && LCM_BA_MAX_OBS == 16777216, \"constants\");\n"
                   "int main(void) { return 0; }\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_defaults(pkg):
    p = pkg.capi.BaParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    pkg.load_library().lcm_ba_params_default(C.byref(p))
    assert (p.fx, p.fy, p.cx, p.cy, p.eps, p.damping, p.min_update, p.outlier_px, p.min_spread, p.spread_factor) == \
        (0.0, 0.0, 0.0, 0.0, 1e-6, 1e-3, 1e-6, 5.0, 10.0, 5.0)
    assert (p.outer_iters, p.inner_iters, p.min_cam_obs, p.min_point_obs, list(p.reserved)) == (5, 5, 10, 2, [0] * 4)
    pkg.load_library().lcm_ba_params_default(None)                             # no-op
    q = pkg.capi.default_ba_params(fx=500.0, inner_iters=3)
    assert (q.fx, q.inner_iters, q.eps) == (500.0, 3, 1e-6)
    with pytest.raises(TypeError):
        pkg.capi.default_ba_params(iterations=1)
    d = B.DEFAULTS
    assert all(getattr(p, k) == v for k, v in d.items())


def test_compact_walks_the_reference_lines(pkg):
    c = pkg.capi
    m, _ = S.planted(6, 30, 41, per_point=3, shuffle=True)
    points, obs = c.ba_points(m.X), c.ba_obs(m.cam, m.pt, m.uv)
    flags = (np.arange(30) % 4 == 1).astype(np.uint8)
    flags[7] = 200                                                              # any non-zero byte flags
    kx, ko, table = c.ba_compact(points, obs, flags)
    old_to_new, pts, kept = [-1] * 30, [], []                                   # :1633-1652
    for i in range(30):
        if not flags[i]:
            old_to_new[i] = len(pts)
            pts.append(points[i])
    for o in obs:
        if old_to_new[o["point"]] != -1:
            kept.append((o["cam"], old_to_new[o["point"]], o["u"], o["v"]))
    assert table.tolist() == old_to_new and kx.tobytes() == np.array(pts).tobytes() and [tuple(o) for o in ko] == kept
    want, wt = B.compact(m, flags)
    assert np.array_equal(table, wt) and np.array_equal(c.ba_xyz(kx), want.X) and np.array_equal(ko["point"], want.pt)
    # too little room: the counts, LCM_ERR_CAPACITY, nothing else written; bad arguments
    lib = pkg.load_library()
    bufs = [np.full(24 * len(kx), FILL, np.uint8), np.full(24 * len(ko), FILL, np.uint8), np.full(4 * 30, FILL, np.uint8)]
    a, b = C.c_int32(-1), C.c_int32(-1)

    def call(cap_points, cap_obs, the_obs=obs, n_points=30, na=a, nb=b):
        return lib.lcm_ba_compact(points.ctypes.data, n_points, the_obs.ctypes.data, len(the_obs), flags.ctypes.data, bufs[0].ctypes.data, cap_points,
                                  bufs[1].ctypes.data, cap_obs, bufs[2].ctypes.data, None if na is None else C.byref(na),
                                  None if nb is None else C.byref(nb))

    for caps in ((len(kx) - 1, len(ko)), (len(kx), len(ko) - 1)):
        assert call(*caps) == -4 and (a.value, b.value) == (len(kx), len(ko)) and all((x == FILL).all() for x in bufs)
    a.value = b.value = -1
    wrong = obs.copy()
    wrong["point"][3] = 30
    assert call(30, len(obs), the_obs=wrong) == -1 and call(30, len(obs), na=None) == -1 and call(-1, len(obs)) == -1
    assert (a.value, b.value) == (-1, -1) and all((x == FILL).all() for x in bufs)
    assert call(len(kx), len(ko)) == 0 and bufs[0].tobytes() == kx.tobytes() and bufs[1].tobytes() == ko.tobytes()
    everything = c.ba_compact(points, obs, np.ones(30, np.uint8))
    assert len(everything[0]) == 0 and len(everything[1]) == 0 and (everything[2] == -1).all()


def test_add_loop_observations_walks_the_reference_lines(pkg):
    c = pkg.capi
    matches, mask, past, curr, kp, n_points = S.loop_lists()
    dm = np.zeros(len(matches), c.DMATCH_DTYPE)
    dm["query_idx"], dm["train_idx"] = matches[:, 0], matches[:, 1]
    obs0 = c.ba_obs([0, 1], [3, 4], [[1.0, 2.0], [3.0, 4.0]])
    table = curr.copy()
    obs, added = c.ba_add_loop_observations(dm, mask, past, table, kp, 9, n_points, obs0)
    new, want_table = B.add_loop_observations(matches, mask, past, curr, kp, 9)            # :1496-1513
    assert added == len(new) > 5 and np.array_equal(table, want_table) and obs[:2].tobytes() == obs0.tobytes()
    assert [(int(o["cam"]), int(o["point"]), float(o["u"]), float(o["v"])) for o in obs[2:]] == new
    # too little room: the count, LCM_ERR_CAPACITY, nothing else written; bad lists
    lib = pkg.load_library()
    buf = np.full(24 * (2 + added), FILL, np.uint8)
    n = C.c_int32(-1)

    def call(cap, the_matches=dm, the_past=past, n_past=len(past), n_curr=len(curr), points=n_points, tab=None, count=n):
        tab = curr.copy() if tab is None else tab
        rc = lib.lcm_ba_add_loop_observations(the_matches.ctypes.data, mask.ctypes.data, len(the_matches), the_past.ctypes.data, n_past,
                                              tab.ctypes.data, kp.ctypes.data, n_curr, 9, points, buf.ctypes.data, 2, cap,
                                              None if count is None else C.byref(count))
        return rc, np.array_equal(tab, curr)

    assert call(2 + added - 1) == (-4, True) and n.value == added and (buf == FILL).all()
    n.value = -1
    hit = int(np.flatnonzero(mask)[0])
    for bad in (dict(the_matches=_with(dm, hit, "query_idx", len(curr))), dict(the_matches=_with(dm, hit, "train_idx", -1)),
                dict(n_past=int(dm["train_idx"][mask != 0].max())), dict(points=int(past[dm["train_idx"][mask != 0]].max())), dict(the_past=_at(past, int(dm["train_idx"][hit]), -2)),
                dict(count=None), dict(cap=1)):
        cap = bad.pop("cap", 2 + added)
        assert call(cap, **bad) == (-1, True) and n.value == -1 and (buf == FILL).all(), bad
    final = curr.copy()
    assert call(2 + added, tab=final)[0] == 0 and n.value == added and np.array_equal(final, want_table)
    assert buf[48:].tobytes() == obs[2:].tobytes() and (buf[:48] == FILL).all()


def _with(records, index, field, value):
    out = records.copy()
    out[field][index] = value
    return out


def _at(array, index, value):
    out = array.copy()
    out[index] = value
    return out


def test_a_null_handle_is_refused_and_nothing_is_written(pkg):
    c = pkg.capi
    lib = pkg.load_library()
    m, _ = S.planted(3, 8, 1, per_point=2)
    poses, points, obs = c.pgo_poses(m.R, m.t), c.ba_points(m.X), c.ba_obs(m.cam, m.pt, m.uv)
    p = c.default_ba_params(fx=1000.0, fy=1000.0)
    bufs = [np.full(4096, FILL, np.uint8) for _ in range(6)]
    b = [x.ctypes.data for x in bufs]
    head = (None, poses.ctypes.data, None, 3, points.ctypes.data, 8, obs.ctypes.data, len(obs), C.byref(p))
    assert lib.lcm_ba_error(*head, C.cast(b[0], C.POINTER(C.c_double)), b[1]) == -1
    assert lib.lcm_ba_refine_cameras(*head, b[0], b[1]) == -1 and lib.lcm_ba_refine_points(*head, b[0], b[1]) == -1
    assert lib.lcm_ba_step_cameras(*head, *b) == -1 and lib.lcm_ba_step_points(*head, *b) == -1
    assert lib.lcm_ba_optimize(*head, b[0], b[1], b[2], b[3], C.cast(b[4], C.POINTER(c.BaInfo))) == -1
    assert lib.lcm_ba_outliers(*head, b[0], b[1], C.cast(b[2], C.POINTER(C.c_double)), C.cast(b[3], C.POINTER(C.c_int32))) == -1
    assert lib.lcm_ba_refine_map(*head, 0, b[0], b[1], b[2], b[3], C.cast(b[4], C.POINTER(c.BaMapReport))) == -1
    assert all((x == FILL).all() for x in bufs) and lib.lcm_last_error() != b""


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs clang++")
def test_host_functions_run_clean_under_sanitizers(tmp_path):
    """csrc/lcm_ba_host.h holds every pure host function of the feature and csrc/lcm_ba_device.h its arithmetic;
    tests/cpp/ba_host_check.cpp is their stand-alone program.  Built as plain C++ (no HIP runtime is linked) with ASan + UBSan (no
    recovery) and run on the CPU: exit status 0 and no report."""
    exe = tmp_path / "ba_host_check"
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", HIP_INCLUDE, "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "ba_host_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "all held" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr)
