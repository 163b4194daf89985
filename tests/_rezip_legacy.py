"""tests/_rezip.py's model of ReZip (tools/rezip_lib.adb) extended by what the knobs "zip_legacy" and "unzip_legacy" add: the approaches shrink and
reduce_4 with their size limits, the formats of Shrink, Reduce and Implode in a format set, and the flag word of a kept Implode stream; and the
loader of tests/zip_legacy/libzip_legacy_plan_host.so."""
import ctypes
import os
import subprocess

import _rezip
from _rezip import ALL_FORMATS, DEFLATE_OR_STORE, FAST_DECOMPRESSION, FORMAT_BIT, NOT_TRIED, APPROACHES, M32, put, try_all_approaches   # noqa: F401

ROOT = _rezip.ROOT
_DIR = os.path.join(ROOT, "tests", "zip_legacy")
SRC = os.path.join(_DIR, "zip_legacy_plan_host.cpp")
_HDRS = [os.path.join(ROOT, "zip-ada_amd", "csrc", h) for h in ("zada_rezip_plan.h", "zada_unzip_plan.h", "zada_zip_plan.h", "zada_legacy_plan.h")] + [os.path.join(ROOT, "include", "zada.h")]

METHOD = (0, 35, 34, 1, 5, 10, 11, 14, 13, 12, 18, 17)          # Approach_to_Method, :238-249, as Compression_Method'Pos: shrink => Shrink_1, reduce_4 => Reduce_4
SHRINK, REDUCE_4 = 3, 4
SHRINK_MAX, REDUCE_4_MAX = 6000, 9000
DEFAULT, LEGACY, TWELVE = 0x0FE7, 0x0018, 0x0FFF


def method_format(m):
    """Method_to_Format of a single method, as a zip type: Shrink 1, Reduce_1 .. _4 2 .. 5 (zip.ads)"""
    return m if 1 <= m <= 5 else _rezip.method_format(m)


def format_choice(formats, zt):
    """format_choice (fmt) of a set given as the C mask.  The mask names store, deflate, deflate_64, bzip2 and lzma; of the reference's three sets
    (rezip_lib.ads:46-54) only all_formats holds shrink, reduce_1 .. _4 and implode, so these are in the set exactly when the mask is all formats."""
    return bool((formats >> FORMAT_BIT[zt]) & 1) if zt in FORMAT_BIT else formats == ALL_FORMATS


def consider_a_priori(approaches, formats):
    """:1072-1089 over all twelve internal approaches"""
    c = [False] * 12
    for a in range(12):
        if a == 0:
            c[a] = True                                        # when original
        elif not (approaches >> a) & 1:
            c[a] = False
        elif METHOD[a] >= 34:                                  # Multi_Method
            c[a] = formats == ALL_FORMATS
        else:                                                  # Single_Method
            c[a] = format_choice(formats, method_format(METHOD[a]))
    return c


def consider_entry(consider, usize):
    """:819-832: the limits of shrink and reduce_4 on one entry"""
    c = list(consider)
    c[SHRINK] = c[SHRINK] and usize <= SHRINK_MAX
    c[REDUCE_4] = c[REDUCE_4] and usize <= REDUCE_4_MAX
    return c


def kept_flag(method, flags, kept, eos):
    """the flag word: :1002-1007, and -- the departure -- bits 1 and 2 of a kept Implode stream stay"""
    f = (flags & 0xFFF5) | (2 if eos else 0)
    if kept and method == 6:
        f |= flags & 6
    return f


def rezip_archive(entries, base=0, comment=b""):
    """_rezip.rezip_archive for entries that also carry method (the source's) and kept (the winner is original).  The base model writes
    (flags and 0xFFF5), with bit 1 set again where `eos` says so; the mask leaves bit 2 alone, so a kept Implode entry's word is the base model's with
    bit 1 set again where the source had it."""
    return _rezip.rezip_archive([dict(e, eos=bool(kept_flag(e["method"], e["flags"], e["kept"], e["eos"]) & 2)) for e in entries], base, comment)


def build_plan():
    p = os.path.join(_DIR, "libzip_legacy_plan_host.so")
    if not os.path.exists(p) or os.path.getmtime(p) < max(os.path.getmtime(x) for x in [SRC] + _HDRS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", p, SRC], check=True)
    return p


def load_plan():
    L = ctypes.CDLL(build_plan())
    u64, u32, vp, i32, ip = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)
    for f in (L.zlp_slot, L.zlp_footprint):
        f.restype, f.argtypes = u64, [u64]
    L.zlp_entry_max.restype = u64
    L.zlp_too_large.argtypes = [vp, i32]
    L.zlp_groups.argtypes = [vp, i32, i32, u64, u64, vp, i32]
    L.zlp_considered.restype, L.zlp_considered.argtypes = u32, [u32, u32, i32]
    L.zlp_considered_default.restype, L.zlp_considered_default.argtypes = u32, [u32, u32]
    L.zlp_methods.argtypes = [u32, i32, i32, u64, vp]
    L.zlp_methods_default.argtypes = [u32, i32, i32, vp]
    L.zlp_considered_entry.restype, L.zlp_considered_entry.argtypes = u32, [u32, u64]
    L.zlp_original_allowed.argtypes = [u32, i32]
    L.zlp_choose.argtypes = [vp, i32]
    L.zlp_rz_check.argtypes = [vp, i32, u64, i32, ip, ip]
    L.zlp_rz_check_default.argtypes = [vp, i32, u64, ip, ip]
    L.zlp_rz_why_text.restype, L.zlp_rz_why_text.argtypes = ctypes.c_char_p, [i32, i32]
    L.zlp_rz_why_text_default.restype, L.zlp_rz_why_text_default.argtypes = ctypes.c_char_p, [i32]
    L.zlp_rz_archive.restype = u64
    L.zlp_rz_archive.argtypes = [vp, i32, vp, vp, vp, vp, u64, ctypes.c_char_p, u32, vp, u64, ctypes.POINTER(u64)]
    return L
