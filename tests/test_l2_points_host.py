"""The C surface of the store's loop correspondences without a device (include/lcm.h: lcm_l2_db_append_kp, lcm_l2_db_read_kp,
lcm_l2_db_match_points, lcm_l2_db_detect_loops_points): every call is declared, exported and bound, lcm_point_pair has the
documented 16 bytes, and a NULL handle is refused with a status code before anything is written."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("lcm_l2_db_append_kp", "lcm_l2_db_read_kp", "lcm_l2_db_match_points", "lcm_l2_db_detect_loops_points")
METHODS = ("l2_db_append_kp", "l2_db_read_kp", "l2_db_match_points", "l2_db_detect_loops_points")


def header():
    txt = open(os.path.join(ROOT, "include", "lcm.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_every_points_call_is_declared_exported_and_bound(pkg):
    h = header()
    lib = C.CDLL(pkg.capi.LIB_PATH)
    for name in CALLS:
        assert len(re.findall(rf"LCM_API\s+extern\s+int\s+{name}\s*\(", h)) == 1, name
        assert hasattr(lib, name), name
        assert pkg.capi._SIGNATURES[name][0] is C.c_int, name
    for name in METHODS:
        assert callable(getattr(pkg.Matcher, name)), name
    # argument counts of the bindings = the declarations'
    for name in CALLS:
        args = re.search(rf"{name}\s*\((.*?)\)\s*;", h, flags=re.S).group(1)
        assert len(pkg.capi._SIGNATURES[name][1]) == args.count(",") + 1, name


def test_point_pair_is_16_bytes(pkg):
    P = pkg.capi.PointPair
    assert C.sizeof(P) == 16
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("qx", 0), ("qy", 4), ("tx", 8), ("ty", 12)]
    assert all(t is C.c_float for _, t in P._fields_)
    body = re.search(r"typedef struct lcm_point_pair \{(.*?)\} lcm_point_pair;", header(), flags=re.S).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "float qx, qy, tx, ty;"


def test_null_handle_is_refused(pkg):
    lib, E = pkg.load_library(), pkg.capi
    buf = (C.c_uint8 * 256)()
    pts = (C.c_float * 8)()
    n, z, z2, off = C.c_int32(7), C.c_size_t(7), C.c_size_t(7), (C.c_size_t * 4)(7, 7, 7, 7)
    pair = (C.c_int32 * 2)(0, 0)
    assert lib.lcm_l2_db_append_kp(None, buf, pts, 1, C.byref(n)) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_read_kp(None, 0, pts, 1) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_match_points(None, pair, 1, 0.7, buf, pts, 1, off) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_detect_loops_points(None, 0, buf, pts, 1, None, 3, None, buf, 1, C.byref(z), C.byref(z2), buf, pts, 1,
                                             off) == E.ERR_INVALID_ARG
    assert n.value == 7 and z.value == 7 and z2.value == 7 and list(off) == [7] * 4      # nothing is written for a NULL handle
    assert not any(buf) and not any(pts)
    assert b"" != lib.lcm_last_error()
