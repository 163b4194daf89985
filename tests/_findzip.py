"""Find_Zip (tools/find_zip.adb) restated literally from the Ada text, for the tests of the plan (test_find_plan.py) and of the device tool
(test_gpu_findzip.py); the closed form as a second opinion; and the loader of tests/find/libfind_plan_host.so."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DIR = os.path.join(ROOT, "tests", "find")
SRC = os.path.join(_DIR, "find_plan_host.cpp")
_HDRS = [os.path.join(ROOT, "zip-ada_amd", "csrc", h) for h in ("zada_find_plan.h", "zada_unzip_plan.h")] + [os.path.join(ROOT, "include", "zada.h")]

MAX = 2 ** 10                                              # max : constant := 2**10
IGNORE_CASE = 1


def build_plan():
    p = os.path.join(_DIR, "libfind_plan_host.so")
    if not os.path.exists(p) or os.path.getmtime(p) < max(os.path.getmtime(x) for x in [SRC] + _HDRS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", p, SRC], check=True)
    return p


def load_plan():
    L = ctypes.CDLL(build_plan())
    u64, u64p, vp, i32, i32p, u32 = ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_uint32
    L.fp_upper_table.restype = ctypes.POINTER(ctypes.c_uint8 * 256)
    L.fp_lower_table.restype = ctypes.POINTER(ctypes.c_uint8 * 256)
    L.fp_check_len.argtypes = [u64]
    L.fp_upper4.restype = u32
    L.fp_upper4.argtypes = [u32]
    L.fp_upper16.argtypes = [vp]
    L.fp_eq_mask4.restype = u32
    L.fp_eq_mask4.argtypes = [u32, u32]
    L.fp_piece_log.restype = u32
    L.fp_piece_count.restype = u64
    L.fp_piece_count.argtypes = [u64]
    L.fp_needle.argtypes = [ctypes.c_char_p, u64, u32, vp, vp]
    L.fp_model.argtypes = [ctypes.c_char_p, u64, u32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, u64, u32, u64p, u64p]
    L.fp_check.argtypes = [vp, i32, u64, i32, i32p, i32p]
    L.fp_groups.argtypes = [vp, i32, u64, vp, i32]
    return L


# ---- Ada.Characters.Handling on Latin-1 ----
def to_upper_char(c):
    """To_Upper of one Character (its 'Pos): the lower-case letters of Latin-1 -- a .. z, 16#E0# .. 16#F6#, 16#F8# .. 16#FE# -- lose 32."""
    return c - 0x20 if 0x61 <= c <= 0x7A or 0xE0 <= c <= 0xF6 or 0xF8 <= c <= 0xFE else c


def to_lower_char(c):
    """To_Lower: A .. Z, 16#C0# .. 16#D6#, 16#D8# .. 16#DE# gain 32."""
    return c + 0x20 if 0x41 <= c <= 0x5A or 0xC0 <= c <= 0xD6 or 0xD8 <= c <= 0xDE else c


def to_upper(s):
    return bytes(to_upper_char(c) for c in s)


def to_lower(s):
    return bytes(to_lower_char(c) for c in s)


def prepare_search_string(s, ignore_case=True):
    """Prepare_Search_String (find_zip.adb:186-199) -> (str (1 .. stl), l).  stl > str'Length raises Constraint_Error; l := str (stl) with stl = 0 is
    an index check that fails: Constraint_Error as well."""
    s = bytes(s)
    if ignore_case:
        s = to_upper(s)
    stl = len(s)
    if stl > MAX:
        raise ValueError("Constraint_Error: the string is longer than max")
    if stl == 0:
        raise ValueError("Constraint_Error: str (0)")
    return s, s[stl - 1]


def search_1_file(item, s, ignore_case=True):
    """Search_1_file_using_output_stream's Write (find_zip.adb:55-85) on the whole entry, statement by statement; str is 1-based in the Ada text, so
    str (j) is s [j - 1].  -> (occ, 0-based offset of the byte at which occ first rose, or len (item))"""
    s, l = prepare_search_string(s, ignore_case)
    stl = len(s)
    occ = 0
    siz = MAX
    buf = [0x20] * siz                                     # buf : array (Buffer_range) of Character := (others => ' ');
    bup = 0
    first = len(item)
    for sei in range(len(item)):                           # for sei in Item'Range loop
        c = item[sei]
        if ignore_case:
            c = to_upper_char(c)
        if c == l:                                         # last character do match, search further...
            i = bup
            j = stl
            while True:                                    # match : loop
                i = (i - 1) % siz                          # this loops modulo max
                j = j - 1
                if j == 0:                                 # we survived the whole search string
                    occ += 1
                    if first == len(item):
                        first = sei
                    break
                if s[j - 1] != buf[i]:                     # exit match when str (j) /= buf (i);
                    break
        buf[bup] = c
        bup = (bup + 1) % siz
    return occ, first


def closed_form(item, s, ignore_case=True):
    """The second opinion: the occurrences, overlapping ones included, of the prepared string in (stl - 1) spaces ++ the entry, by bytes.find."""
    s, _ = prepare_search_string(s, ignore_case)
    x = b" " * (len(s) - 1) + (to_upper(item) if ignore_case else bytes(item))
    occ, first, at = 0, len(item), x.find(s)
    while at >= 0:
        occ += 1
        if first == len(item):
            first = at                                     # (the occurrence's last byte: at + stl - 1, less the stl - 1 spaces)
        at = x.find(s, at + 1)
    return occ, first


def search_in_entry_name(file_name, s, ignore_case=True):
    """Search_in_entry_name (find_zip.adb:150-159): Index (un, str (1 .. stl)) > 0"""
    s, _ = prepare_search_string(s, ignore_case)
    un = bytes(file_name)
    if ignore_case:
        un = to_upper(un)
    return un.find(s) >= 0                                 # Ada.Strings.Fixed.Index, Forward, no mapping


def find_zip(entries, s, ignore_case=True):
    """Find_Zip on an archive given as a list of (raw name, bytes) in directory order -> (in_contents [(name as traversed, occ, first)], in_names,
    the output lines).  Zip.Traverse walks the dictionary names: '\\' turned into '/', ascending, case-sensitive (zip.adb:152-166, 216-219)."""
    d = sorted((nm.replace(b"\\", b"/"), data) for nm, data in entries)
    contents, names, lines = [], [], []
    for name, data in d:                                   # Search_all_files (z)
        occ, first = search_1_file(data, s, ignore_case)
        if occ > 0:
            contents.append((name, occ, first))
            lines.append("%5d" % occ + " in [" + to_lower(name).decode("latin-1") + "]'s contents")       # Put (occ, 5); Put_Line (...)
    for name, _ in d:                                      # Search_all_file_names (z)
        if search_in_entry_name(name, s, ignore_case):
            names.append(name)
            lines.append(" Found in [" + to_lower(name).decode("latin-1") + "]'s entry name")
    return contents, names, lines


# ---- the cases the CPU model (test_find_plan.py) and the kernel (test_gpu_findzip.py) are both held to ----
PIECE = 16384
STRING_LENGTHS = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1023, 1024)
TEXT_LENGTHS = (0, 1, 15, 16, 17, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE + 3)
_cases = {}


def grid_cases():
    """[(entry, string)]: every text length against every string length.  The string ends in z, which every eighth byte of the text is; it is
    planted so that it ends at the entry's byte stl - 1 (it begins at the first byte), at the first byte (only its last character fits), at the last
    byte, at PIECE - 1, at PIECE, at PIECE + stl - 2 (it begins in the piece before) and at 2 PIECE + 1 (stl = 1024: across two boundaries).  For
    three of the text lengths also a string whose head is spaces against an entry that begins with z: it matches in front of the first byte."""
    if "grid" not in _cases:
        import random
        rng = random.Random(9)
        out = []
        for n in TEXT_LENGTHS:
            for stl in STRING_LENGTHS:
                s = bytes(rng.choice(b"abcxy ") for _ in range(stl - 1)) + b"z"
                x = bytearray(rng.choice(b"abcxy  z") for _ in range(n))
                for end in (stl - 1, 0, n - 1, PIECE - 1, PIECE, PIECE + stl - 2, 2 * PIECE + 1):      # (end: the occurrence's last byte)
                    if 0 <= end < n:
                        lo = max(0, end + 1 - stl)
                        x[lo:end + 1] = s[stl - (end + 1 - lo):]
                out.append((bytes(x), s))
                if n in (1, 17, PIECE + 1):
                    out.append((b"z" + bytes(x[1:]), b" " * (stl - 1) + b"z"))
        _cases["grid"] = out
    return _cases["grid"]


def named_cases():
    """[(entry, string, ignore_case)]: virtual spaces, overlaps, dense candidates, case, and 1024 bytes across two piece boundaries."""
    if "named" not in _cases:
        import random
        rng = random.Random(10)
        a = b"a" * (2 * PIECE + 3)
        mixed = b"Hello W\xf6rld, hello w\xf6rld, HELLO W\xd6RLD \xf7\xd7 \xff\xdf"
        x = bytearray(b"." * (2 * PIECE + 700))
        s = bytes(rng.choice(b"abc") for _ in range(1024))
        x[2 * PIECE - 500:2 * PIECE + 524] = s
        _cases["named"] = [
            (b"ab" + b"q" * 40, b"  ab", True), (b"     ", b" " * 1024, True), (b"x    ", b" " * 1024, True),
            (a, b"aaa", True), (a, b"b" + b"a" * 40, True), (b" " * (2 * PIECE + 3), b" ", True),
            (mixed, b"hello w\xf6rld", True), (mixed, b"hello w\xf6rld", False), (mixed, b"HELLO W\xd6RLD", False),
            (b"\xd7\xf7\xdf\xff" * 9, b"\xf7", True), (b"\xd7\xf7\xdf\xff" * 9, b"\xd7", True), (b"\xd7\xf7\xdf\xff" * 9, b"\xdf\xff", True),
            (b"\xd7\xf7\xdf\xff" * 9, b"\xff", True), (b"\xd7\xf7\xdf\xff" * 9, b"\xdf", True), (bytes(x), s, True)]
    return _cases["named"]


_want = {}


def reference(x, s, ignore_case=True):
    """search_1_file, computed once per case."""
    key = (x, s, ignore_case)
    if key not in _want:
        _want[key] = search_1_file(x, s, ignore_case)
    return _want[key]
