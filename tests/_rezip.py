"""ReZip's approach loop and header writing (tools/rezip_lib.adb) and Comp_Zip (tools/comp_zip_prc.adb) restated literally from the Ada text, for the
tests of the plan (test_rezip_plan.py) and of the device tools (test_gpu_rezip.py, test_gpu_rezip_device.py); and the loader of
tests/rezip/librezip_plan_host.so."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DIR = os.path.join(ROOT, "tests", "rezip")
SRC = os.path.join(_DIR, "rezip_plan_host.cpp")
_HDRS = [os.path.join(ROOT, "zip-ada_amd", "csrc", h) for h in ("zada_rezip_plan.h", "zada_unzip_plan.h", "zada_zip_plan.h")] + [os.path.join(ROOT, "include", "zada.h")]

OK, DIFFERENT, SHORTER, LONGER, MISSING, DAMAGED = range(6)
ABSENT = 0x80


def build_plan():
    p = os.path.join(_DIR, "librezip_plan_host.so")
    if not os.path.exists(p) or os.path.getmtime(p) < max(os.path.getmtime(x) for x in [SRC] + _HDRS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", p, SRC], check=True)
    return p


def load_plan():
    L = ctypes.CDLL(build_plan())
    u64, u64p, vp, i32, i32p = ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)
    L.rp_verdict.argtypes = [u64, u64, u64, u64p, u64p]
    L.rp_check.argtypes = [vp, vp, i32, u64, u64, i32, i32p, i32p, i32p]
    L.rp_why_text.restype = ctypes.c_char_p
    L.rp_why_text.argtypes = [i32]
    L.rp_slot.restype = u64
    L.rp_slot.argtypes = [vp, vp]
    L.rp_groups.argtypes = [vp, vp, i32, u64, vp, i32]
    L.rp_piece_count.restype = u64
    L.rp_piece_count.argtypes = [u64]
    L.rp_piece_log.restype = ctypes.c_uint32
    u32 = ctypes.c_uint32
    L.rp_considered.restype = u32
    L.rp_considered.argtypes = [u32, u32]
    L.rp_choose.argtypes = [vp, i32]
    L.rp_methods.argtypes = [u32, i32, i32, vp]
    L.rp_rz_check.argtypes = [vp, i32, u64, u64, u64, u64, i32p, i32p]
    L.rp_rz_why_text.restype = ctypes.c_char_p
    L.rp_rz_why_text.argtypes = [i32]
    L.rp_rz_bound.restype = u64
    L.rp_rz_bound.argtypes = [i32, vp, u64]
    L.rp_rz_groups.argtypes = [vp, i32, u64, vp, i32]
    L.rp_rz_archive.restype = u64
    L.rp_rz_archive.argtypes = [vp, i32, vp, vp, vp, u64, ctypes.c_char_p, u32, vp, u64, vp, u64p]
    return L


def compare_1_file(f1, f2):
    """Compare_1_file's loop behind "File found, now the comparison" (comp_zip_prc.adb:102-143), statement by statement, on two byte strings.
    -> (verdict, position or 0, bytes that go to total_bytes or 0)"""
    p = 1
    i1 = i2 = 0                                            # the streams' read positions
    while not i1 == len(f1):                               # while not End_Of_File (f (1)) loop
        if i2 == len(f2):                                  # if End_Of_File (f (2)) then
            return SHORTER, p, 0                           # "Shorter in [2] at position" p; size_failures + 1
        c1, c2 = f1[i1], f2[i2]                            # Character'Read, one of each stream
        i1 += 1
        i2 += 1
        if c1 != c2:
            return DIFFERENT, p, 0                         # "Difference at position" p; compare_failures + 1
        p += 1
    if not i2 == len(f2):                                  # if not End_Of_File (f (2)) then
        return LONGER, 0, 0                                # "Longer in [2]"; size_failures + 1
    return OK, 0, p - 1                                    # "OK -" p - 1 "bytes compared"; total_bytes + (p - 1)


def comp_zip(z1, z2):
    """Comp_Zip_Prc on two archives given as lists of (raw name, bytes) in directory order -> dict of the counters and the per-entry verdicts
    [(raw name as traversed, verdict, position)].  Zip.Traverse walks archive 1 in the order of the dictionary names: '\\' turned into '/',
    case-sensitive (zip.adb:152-166, 216-219); Open looks the traversed name up in archive 2 the same way."""
    norm = lambda nm: nm.replace(b"\\", b"/")
    d1 = sorted((norm(nm), data) for nm, data in z1)
    d2 = {norm(nm): data for nm, data in z2}
    c = dict(total_1=0, total_2=0, common=0, size_failures=0, compare_failures=0, missing_1_in_2=0, just_a_directory=0, missing_2_in_1=0, total_bytes=0)
    entries = []
    for name, data in d1:
        c["total_1"] += 1                                  # Open (f (1), ...) succeeded
        if name not in d2:                                 # Zip.Entry_name_not_found for i = 2
            if name[-1:] in (b"/", b"\\"):
                c["just_a_directory"] += 1
            c["missing_1_in_2"] += 1
            entries.append((name, MISSING, 0))
            continue
        v, pos, nbytes = compare_1_file(data, d2[name])
        if v in (SHORTER, LONGER):
            c["size_failures"] += 1
        elif v == DIFFERENT:
            c["compare_failures"] += 1
        else:
            c["total_bytes"] += nbytes
        entries.append((name, v, pos))
    c["total_2"] = len(z2)
    c["common"] = c["total_1"] - c["missing_1_in_2"]
    c["missing_2_in_1"] = c["total_2"] - c["common"]
    c["total_differences"] = c["size_failures"] + c["compare_failures"] + c["missing_1_in_2"] + c["missing_2_in_1"]
    return c, entries


# ---- ReZip (tools/rezip_lib.adb) ----
APPROACHES = ("original", "presel_2", "presel_1", "shrink", "reduce_4", "deflate_3", "deflate_r", "bzip2_3", "bzip2_2", "bzip2_1", "lzma_3", "lzma_2")
METHOD = (0, 35, 34, 0, 0, 10, 11, 14, 13, 12, 18, 17)          # Approach_to_Method, :238-249, as Compression_Method'Pos
ALL_FORMATS, DEFLATE_OR_STORE, FAST_DECOMPRESSION = 0x1F, 0x03, 0x17
FORMAT_BIT = {0: 0, 8: 1, 9: 2, 12: 3, 14: 4}
NOT_TRIED = 0xFFFFFFFFFFFFFFFF
M32 = 0xFFFFFFFF


def method_format(m):
    """Method_to_Format of a single method, as a zip type"""
    return 0 if m == 0 else 8 if m <= 11 else 12 if m <= 14 else 14


def consider_a_priori(approaches, formats):
    """:1072-1089 over the built approaches: original True; Single_Method: format_choice (Method_to_Format (meth)); Multi_Method: format_choice =
    all_formats"""
    c = [False] * 12
    for a in range(12):
        if a == 0:
            c[a] = True
        elif a in (3, 4) or not (approaches >> a) & 1:
            c[a] = False
        elif METHOD[a] >= 34:
            c[a] = formats == ALL_FORMATS
        else:
            c[a] = bool((formats >> FORMAT_BIT[method_format(METHOD[a])]) & 1)
    return c


def try_all_approaches(consider, size, original_format_allowed):
    """The loop Try_all_approaches, :835-889, statement by statement: size [a] is e.info (a).size of a considered approach.  -> choice"""
    choice = 0
    for a in range(len(consider)):
        if consider[a]:
            if size[a] < size[choice]:
                choice = a                                     # "Hurra, we found a smaller size than previous choice!"
            if choice == 0 and not original_format_allowed:    # choice = original and not format_choice (mth): mth is original's format
                choice = a
    return choice


def put(v, n):
    return int(v).to_bytes(n, "little")


def rezip_archive(entries, base=0, comment=b""):
    """The archive as Process_one (:1000-1032) and Repack_contents (:1184-1260) write it.  entries: dicts with name (bytes), version, flags, time, crc,
    usize -- the source's local header and directory -- and the winner's csize, zip_type, eos, payload (bytes, or None: only its length csize counts
    and it is left out of the bytes).  -> (local headers and payloads, central directory with end records and comment, [offsets], archive length)"""
    out, cd, offs = bytearray(), bytearray(), []
    needs_64 = False
    pos = 0
    for e in entries:
        flag = (e["flags"] & 0xFFF5) | (2 if e["eos"] else 0)
        off = base + pos
        z64 = e["csize"] >= M32 or e["usize"] >= M32 or off >= M32          # Needs_Local_Zip_64_Header_Extension
        h = b"PK\x03\x04" + put(e["version"], 2) + put(flag, 2) + put(e["zip_type"], 2) + put(e["time"], 4) + put(e["crc"], 4)
        h += (b"\xff" * 8 if z64 else put(e["csize"], 4) + put(e["usize"], 4)) + put(len(e["name"]), 2) + put(20 if z64 else 0, 2) + e["name"]
        if z64:
            h += put(1, 2) + put(16, 2) + put(e["usize"], 8) + put(e["csize"], 8)
        offs.append(off)
        if e.get("payload") is not None:
            out += h + e["payload"]
        else:
            out += h
        pos += len(h) + e["csize"]
        c = b"PK\x01\x02" + put(20, 2) + put(e["version"], 2) + put(flag, 2) + put(e["zip_type"], 2) + put(e["time"], 4) + put(e["crc"], 4)
        c += put(M32 if z64 else e["csize"], 4) + put(M32 if z64 else e["usize"], 4) + put(len(e["name"]), 2) + put(28 if z64 else 0, 2)
        c += put(0, 2) + put(0, 2) + put(0, 2) + put(0, 4) + put(M32 if z64 else off, 4) + e["name"]
        if z64:
            c += put(1, 2) + put(24, 2) + put(e["usize"], 8) + put(e["csize"], 8) + put(off, 8)
            needs_64 = True
        cd += c
    cd_off, n = base + pos, len(entries)
    tail = bytes(cd)
    if needs_64:
        tail += b"PK\x06\x06" + put(44, 8) + put(0x2D, 2) + put(0x2D, 2) + put(0, 4) + put(0, 4) + put(n, 8) + put(n, 8) + put(len(cd), 8) + put(cd_off, 8)
        tail += b"PK\x06\x07" + put(0, 4) + put(cd_off + len(cd), 8) + put(1, 4)
        tail += b"PK\x05\x06" + put(0, 2) + put(0, 2) + put(0xFFFF, 2) + put(0xFFFF, 2) + put(M32, 4) + put(M32, 4)
    else:
        tail += b"PK\x05\x06" + put(0, 2) + put(0, 2) + put(n, 2) + put(n, 2) + put(len(cd), 4) + put(cd_off, 4)
    tail += put(len(comment), 2) + comment
    return bytes(out), tail, offs, pos + len(tail)
