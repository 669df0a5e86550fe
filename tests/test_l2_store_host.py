"""The SIFT keyframe store's C surface without a device (include/lcm.h, lcm_l2_db_*): every call is declared, exported and
bound, refuses a NULL handle with a status code, and lcm_l2_db_info has the documented 40 bytes."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("lcm_l2_db_append", "lcm_l2_db_size", "lcm_l2_db_rows", "lcm_l2_db_read", "lcm_l2_db_truncate", "lcm_l2_db_clear",
         "lcm_l2_db_info_read", "lcm_l2_db_score_pairs", "lcm_l2_db_match_pairs_ratio", "lcm_l2_db_loop_search",
         "lcm_l2_db_detect_loops")
METHODS = ("l2_db_append", "l2_db_size", "l2_db_rows", "l2_db_read", "l2_db_truncate", "l2_db_clear", "l2_db_info",
           "l2_db_score_pairs", "l2_db_match_pairs_ratio", "l2_db_loop_search", "l2_db_detect_loops")


def header():
    txt = open(os.path.join(ROOT, "include", "lcm.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_every_store_call_is_declared_exported_and_bound(pkg):
    declared = set(re.findall(r"LCM_API\s+int\s+(lcm_l2_db_\w+)\s*\(", header()))
    assert declared == set(CALLS)
    lib = C.CDLL(pkg.capi.LIB_PATH)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in pkg.capi._SIGNATURES, name
        assert pkg.capi._SIGNATURES[name][0] is C.c_int
    for name in METHODS:
        assert callable(getattr(pkg.Matcher, name)), name


def test_info_struct_is_40_bytes(pkg, tmp_path):
    I = pkg.capi.L2DbInfo
    assert C.sizeof(I) == 40
    assert [(n, getattr(I, n).offset) for n, _ in I._fields_] == [("frames", 0), ("reserved_", 4), ("tiles_used", 8),
                                                                   ("tiles_reserved", 16), ("device_bytes", 24), ("table_bytes", 32)]
    body = re.search(r"typedef struct lcm_l2_db_info \{(.*?)\} lcm_l2_db_info;", header(), flags=re.S).group(1)
    assert re.findall(r"(\w+)\s+(\w+);", body) == [("int32_t", "frames"), ("int32_t", "reserved_"), ("uint64_t", "tiles_used"),
                                                    ("uint64_t", "tiles_reserved"), ("uint64_t", "device_bytes"),
                                                    ("uint64_t", "table_bytes")]


def test_null_handle_is_refused(pkg):
    lib, E = pkg.load_library(), pkg.capi
    buf = (C.c_uint8 * 256)()
    n, z, z2 = C.c_int32(7), C.c_size_t(7), C.c_size_t(7)
    info = E.L2DbInfo()
    pair = (C.c_int32 * 2)(0, 0)
    assert lib.lcm_l2_db_append(None, buf, 1, C.byref(n)) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_size(None) == 0
    assert lib.lcm_l2_db_rows(None, 0, C.byref(n)) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_read(None, 0, buf, 1) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_truncate(None, 0) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_clear(None) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_info_read(None, C.byref(info)) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_score_pairs(None, pair, 1, 0.7, buf) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_match_pairs_ratio(None, pair, 1, 0.7, buf, 1, C.byref(z)) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_loop_search(None, None, 3, None, buf, 1, C.byref(z), C.byref(z2)) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_detect_loops(None, 0, buf, 1, None, 3, None, buf, 1, C.byref(z), C.byref(z2)) == E.ERR_INVALID_ARG
    assert n.value == 7 and z.value == 7 and z2.value == 7              # nothing is written for a NULL handle
    assert b"" != lib.lcm_last_error()
