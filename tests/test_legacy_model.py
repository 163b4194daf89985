"""The CPU models of Shrink_1 and Reduce_1 .. _4 (tests/legacy/): the encoders as the reference states them against the closed forms the GPU kernels
use, the decoders written from APPNOTE 5.1 / 5.2, and the censuses that say which branches the shared inputs reach.  No GPU."""
import ctypes
import os
import shutil
import struct
import subprocess
import zlib

import pytest

import _legacy as L

SHOULD_NOT_HAPPEN = ("add_under_freed", "alloc_with_child", "unreachable", "full_nonliteral")


def _shrink_inputs():
    """The named inputs, the edge sizes, and every other input a GPU test hands the device under Shrink_1."""
    d = dict(L.shrink_inputs())
    for n in L.edge_sizes():
        d["edge_%d" % n] = L.edge_input(n)
    known = set(d.values())
    d.update(("gpu_%d" % i, x) for i, x in enumerate(L.gpu_test_inputs(1)) if x not in known)
    return d


def _reduce_inputs(factor):
    """The named inputs, every edge size, and every other input a GPU test hands the device under this factor."""
    d = dict(L.reduce_inputs())
    for n in L.edge_sizes():
        d["edge_%d" % n] = L.edge_input(n)
    known = set(d.values())
    d.update(("gpu_%d" % i, x) for i, x in enumerate(L.gpu_test_inputs(factor + 1)) if x not in known)
    return d


def test_shrink_stated_equals_closed_and_decodes():
    for name, data in _shrink_inputs().items():
        s, cs = L.shrink(data)
        s2, cs2 = L.shrink(data, stated=True)
        assert s == s2 and cs == cs2, name
        assert L.unshrink(s, len(data)) == data, name
        for k in SHOULD_NOT_HAPPEN:                        # with any of these the closed form of the partial clear would be wrong for that input
            assert cs2[k] == 0, (name, k, cs2[k])


def test_shrink_census_of_the_shared_inputs():
    c = {k: L.shrink(v, stated=True) for k, v in L.shrink_inputs().items()}
    assert len(c["abcd_48k"][0]) == 14248 and c["abcd_48k"][1]["clears"] == 1 and c["abcd_48k"][1]["rises"] == 4
    assert len(c["abcd_128k"][0]) == 37328 and c["abcd_128k"][1]["clears"] == 4 and c["sym16_96k"][1]["clears"] == 6
    assert len(c["random_16k"][0]) == 24317 and c["random_16k"][1]["clears"] == 2      # not shorter than its 16 384 bytes: rc 1 on the device
    for k in ("abcd_48k", "abcd_128k", "sym16_96k"):
        assert c[k][1]["clears"] >= 1 and c[k][1]["rises"] == 4 and c[k][1]["dup_adds"] >= 1, (k, c[k][1])
    # the pair added behind a clear was in the table already at (almost) every clear: the later copy is a leaf that nothing finds
    assert c["abcd_128k"][1]["dup_adds"] == 4 and c["sym16_96k"][1]["dup_adds"] == 6
    assert L.shrink(b"")[0] == b"" and len(L.shrink(b"x")[0]) == 2


def test_reduce_stated_equals_closed_and_decodes():
    seen = dict.fromkeys(L.REDUCE_CENSUS, 0)
    per = {}
    for factor in (1, 2, 3, 4):
        for name, data in _reduce_inputs(factor).items():
            a = L.reduce(data, factor)
            b = L.reduce(data, factor, stated=True)
            assert a[0] == b[0] and a[1] == b[1] and (a[2] == b[2]).all() and a[4] == b[4], (name, factor)
            assert L.followers_in_use(a[2], a[3]) == L.followers_in_use(b[2], b[3]), (name, factor)
            assert L.unreduce(a[0], factor, len(data)) == data, (name, factor)
            per[name, factor] = b[4]
            for k, v in b[4].items():
                seen[k] += v
    assert all(seen["slen%d" % k] > 0 for k in (0, 2, 4, 8, 16, 32)), seen           # every Slen somewhere in the set
    assert per["words_24k", 1]["lit144"] >= 100 and all(per["words_24k", f]["expanded"] > 0 for f in (1, 2, 3)) and per["words_24k", 4]["two_byte"] > 0
    assert per["runs_A_90", 3]["two_byte"] > 0 and per["runs_A_90", 4]["two_byte"] > 0
    assert all(per["far_repeats", f]["expanded"] > 0 for f in (1, 2, 3))
    assert all(len(L.reduce(L.reduce_inputs()["big_400k"], f)[1]) > 1 << 18 for f in (1, 4))      # the raw stream passes the model's 256 KiB cache
    assert len(L.reduce(b"", 4)[0]) == 192                                             # 256 empty follower sets


def test_seeded_small_inputs():
    cs = (ctypes.c_uint64 * len(L.SHRINK_CENSUS))()
    assert L.shrink_lib().shrink_selftest(1, 3000, cs) == 0
    cr = (ctypes.c_uint64 * len(L.REDUCE_CENSUS))()
    assert L.reduce_lib().reduce_selftest(1, 2000, cr) == 0
    assert cr[0] > 0 and cr[1] > 0 and cr[2] > 0


def test_models_under_sanitizers(tmp_path):
    """The two models with a main of their own under AddressSanitizer and UndefinedBehaviorSanitizer, over seeded inputs and every input of the tests above -- the GPU tests' inputs at full size among them."""
    exe = str(tmp_path / "legacy_check")
    r = subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(L.DIR, "legacy_check_main.c")],
                       capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr + r.stdout and "cannot find" in r.stderr + r.stdout:
        pytest.skip("no sanitizer runtime for gcc on this machine")
    assert r.returncode == 0, r.stderr[-2000:]
    # every input of the CPU tests above, under the methods it is used with: one file per input, grouped by the set of methods
    uses = {}
    for data in _shrink_inputs().values():
        uses.setdefault(data, set()).add(1)
    for factor in (1, 2, 3, 4):
        for data in _reduce_inputs(factor).values():
            uses.setdefault(data, set()).add(factor + 1)
    args = []
    for methods in sorted({frozenset(m) for m in uses.values()}, key=sorted):
        args.append("-m" + "".join(str(m) for m in sorted(methods)))
        for data, m in uses.items():
            if m == methods:
                args.append(str(tmp_path / ("in_%d.bin" % len(args))))
                with open(args[-1], "wb") as f:
                    f.write(data)
    r = subprocess.run([exe, "50"] + args, capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])


def _one_entry_zip(name, payload, method, crc, usize):
    nm = name.encode()
    local = struct.pack("<IHHHHHIIIHH", 0x04034B50, 10, 0, method, 0, 0x21, crc, len(payload), usize, len(nm), 0) + nm
    central = struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, 20, 10, 0, method, 0, 0x21, crc, len(payload), usize, len(nm), 0, 0, 0, 0, 0, 0) + nm
    end = struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, 1, 1, len(central), len(local) + len(payload), 0)
    return local + payload + central + end


@pytest.mark.skipif(shutil.which("unzip") is None, reason="no unzip on this machine")
def test_unzip_reads_the_shrink_streams(tmp_path):
    for name, data in L.shrink_inputs().items():
        s = L.shrink(data)[0]
        p = tmp_path / (name + ".zip")
        p.write_bytes(_one_entry_zip(name, s, 1, zlib.crc32(data), len(data)))
        r = subprocess.run(["unzip", "-p", str(p)], capture_output=True)
        assert r.returncode == 0 and r.stdout == data, (name, r.stderr[-300:])
