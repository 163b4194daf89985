"""The argument checks of the archive readers with and without the knob "unzip_legacy" (uz_check, fz_check, cz_check; tests/unlegacy/
unzip_legacy_plan_host.cpp): off, methods 1 .. 6 are refused with the text of before; on, they are known, and the text for the others lists all."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from _common import ROOT

E_INVALID, W_METHOD = -1, 1
OLD = b"unknown method (0 Store, 8 Deflate, 9 Deflate64, 12 BZip2, 14 LZMA)"
NEW = b"unknown method (0 Store, 1 Shrink, 2 .. 5 Reduce, 6 Implode, 8 Deflate, 9 Deflate64, 12 BZip2, 14 LZMA)"
DT = np.dtype([("in_off", "<u8"), ("n_in", "<u8"), ("out_off", "<u8"), ("cap", "<u8"), ("method", "<u2"), ("flags", "u1"), ("check", "u1"), ("pad", "<u4")])


@pytest.fixture(scope="module")
def plan():
    d = os.path.join(ROOT, "tests", "unlegacy")
    src, p = os.path.join(d, "unzip_legacy_plan_host.cpp"), os.path.join(d, "libunzip_legacy_plan_host.so")
    hdrs = [os.path.join(ROOT, "zip-ada_amd", "csrc", h) for h in ("zada_unzip_plan.h", "zada_rezip_plan.h", "zada_find_plan.h")]
    if not os.path.exists(p) or os.path.getmtime(p) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", p, src], check=True)
    L = ctypes.CDLL(p)
    vp, i32, u64, ip = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.POINTER(ctypes.c_int)
    L.ulp_check.argtypes = [vp, i32, u64, u64, i32, i32, i32, ip, ip]
    L.ulp_check_default.argtypes = [vp, i32, u64, u64, i32, i32, ip, ip]
    L.ulp_find_check.argtypes = [vp, i32, u64, i32, i32, ip, ip]
    L.ulp_comp_check.argtypes = [vp, vp, i32, u64, u64, i32, i32, ip, ip, ip]
    L.ulp_why_text.restype = ctypes.c_char_p
    L.ulp_why_text_default.restype = ctypes.c_char_p
    return L


def _rows(methods):
    t = np.zeros(len(methods), dtype=DT)
    for k, m in enumerate(methods):
        t[k] = (10 * k, 10, 100 * k, 100, m, 6 if m == 6 else 0, 0, 0)
    return t


def _check(L, t, legacy):
    bad, why = ctypes.c_int(-9), ctypes.c_int(-9)
    if legacy is None:
        rc = L.ulp_check_default(t.ctypes.data, len(t), 1000, 10000, 1, 0, ctypes.byref(bad), ctypes.byref(why))
    else:
        rc = L.ulp_check(t.ctypes.data, len(t), 1000, 10000, 1, 0, legacy, ctypes.byref(bad), ctypes.byref(why))
    return rc, bad.value, why.value


def test_knob_off_refuses_with_the_text_of_before(plan):
    assert plan.ulp_why_text(W_METHOD, 0) == OLD and plan.ulp_why_text_default(W_METHOD) == OLD
    for legacy in (None, 0):
        for m in (1, 2, 3, 4, 5, 6, 7, 10, 13):
            assert _check(plan, _rows([0, 8, m, 14]), legacy) == (E_INVALID, 2, W_METHOD), (legacy, m)
        assert _check(plan, _rows([0, 8, 9, 12, 14]), legacy) == (0, -1, 0)


def test_knob_on_knows_methods_1_to_6(plan):
    assert plan.ulp_why_text(W_METHOD, 1) == NEW
    assert _check(plan, _rows([0, 1, 2, 3, 4, 5, 6, 8, 9, 12, 14]), 1) == (0, -1, 0)
    for m in (7, 10, 13, 11, 15, 99):
        assert _check(plan, _rows([1, 6, m]), 1) == (E_INVALID, 2, W_METHOD), m
    # the other rules hold for a legacy row as for any other: its data beyond the archive
    t = _rows([1])
    t[0]["n_in"] = 2000
    assert _check(plan, t, 1) == (E_INVALID, 0, 3)


def test_find_and_comp_checks_pass_the_knob_on_and_rezip_does_not(plan):
    t = _rows([0, 1, 6])
    bad, why, side = ctypes.c_int(-9), ctypes.c_int(-9), ctypes.c_int(-9)
    assert plan.ulp_find_check(t.ctypes.data, 3, 1000, 0, 0, ctypes.byref(bad), ctypes.byref(why)) == E_INVALID and (bad.value, why.value) == (1, W_METHOD)
    assert plan.ulp_find_check(t.ctypes.data, 3, 1000, 0, 1, ctypes.byref(bad), ctypes.byref(why)) == 0
    b = _rows([0, 8, 5])
    args = (t.ctypes.data, b.ctypes.data, 3, 1000, 1000, 0)
    assert plan.ulp_comp_check(*args, 0, ctypes.byref(bad), ctypes.byref(side), ctypes.byref(why)) == E_INVALID and (bad.value, side.value, why.value) == (1, 1, W_METHOD)
    assert plan.ulp_comp_check(*args, 1, ctypes.byref(bad), ctypes.byref(side), ctypes.byref(why)) == 0
    assert [plan.ulp_rezip_knows(m) for m in (0, 1, 6, 8, 14)] == [1, 0, 0, 1, 1]
