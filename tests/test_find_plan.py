"""The host plan and the lane arithmetic of Find_Zip on the device (zip-ada_amd/csrc/zada_find_plan.h: the Latin-1 tables, the length check, the
SWAR helpers, the string as the kernel takes it, the groups, and the CPU model of k_fz_search built from the same helpers the kernel uses) through
tests/find/find_plan_host.cpp, against the literal restatement of the Ada loop in tests/_findzip.py; the same lists once more through a program of
its own built with -fsanitize=address,undefined.  No GPU, and nothing is loaded into this interpreter with a sanitizer."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import _findzip

PIECE = _findzip.PIECE
ALPHABET = b" aA\xe0\xc0\xff\xf7"
DT = np.dtype([("in_off", "<u8"), ("n_in", "<u8"), ("out_off", "<u8"), ("cap", "<u8"), ("method", "<u2"), ("flags", "u1"), ("check", "u1"), ("pad", "<u4")])


@pytest.fixture(scope="module")
def plan():
    return _findzip.load_plan()


def model(plan, entry, text, ignore_case=True, phase=0, front=None, behind=None):
    """The model's (occurrences, first) for the entry at `phase`; by default the bytes in front of it are the string itself (upper-cased or not, as
    it would have to be to count) behind exclamation marks, and the bytes behind it the string's last character."""
    if front is None:
        front = (b"!" * 2048 + bytes(text))[-2048:]
    if behind is None:
        behind = bytes(text[-1:] or b"!") * 2048
    occ, first = ctypes.c_uint64(77), ctypes.c_uint64(77)
    rc = plan.fp_model(bytes(entry), len(entry), phase, front, behind, bytes(text), len(text), 1 if ignore_case else 0, ctypes.byref(occ), ctypes.byref(first))
    assert rc == 0, "the model loaded a word that holds no byte of the entry" if rc == 1 else rc
    return occ.value, first.value


def test_tables_for_all_256_bytes(plan):
    up, lo = bytes(plan.fp_upper_table().contents), bytes(plan.fp_lower_table().contents)
    for c in range(256):
        lower_letter = 0x61 <= c <= 0x7A or 0xE0 <= c <= 0xF6 or 0xF8 <= c <= 0xFE
        upper_letter = 0x41 <= c <= 0x5A or 0xC0 <= c <= 0xD6 or 0xD8 <= c <= 0xDE
        assert up[c] == (c - 0x20 if lower_letter else c) == _findzip.to_upper_char(c), c
        assert lo[c] == (c + 0x20 if upper_letter else c) == _findzip.to_lower_char(c), c
    for c in (0xDF, 0xF7, 0xFF, 0xD7):
        assert up[c] == c
    assert up[0xE0] == 0xC0 and up[0xFE] == 0xDE and lo[0xD7] == 0xD7 and lo[0xDE] == 0xFE
    # Python's own Latin-1 agrees wherever the upper-case form stays inside Latin-1 (0xB5, 0xDF and 0xFF leave it)
    for c in range(256):
        u = bytes([c]).decode("latin-1").upper()
        if len(u) == 1 and ord(u) < 256:
            assert up[c] == ord(u), c


def test_swar_helpers_in_every_byte_lane(plan):
    """All 256 values in every byte lane of a dword, in the company of random neighbours: upper-casing four bytes at once, sixteen at once, and
    the mask of the bytes equal to a character."""
    rng = random.Random(5)
    for lane in range(4):
        for c in range(256):
            for _ in range(3):
                b = [rng.randrange(256) for _ in range(4)]
                b[lane] = c
                x = int.from_bytes(bytes(b), "little")
                assert plan.fp_upper4(x).to_bytes(4, "little") == _findzip.to_upper(bytes(b)), (lane, c, b)
                for ch in (c, b[(lane + 1) & 3], rng.randrange(256), _findzip.to_upper_char(c)):
                    want = sum(0x80 << (8 * i) for i in range(4) if b[i] == ch)
                    assert plan.fp_eq_mask4(x, ch) == want, (b, ch)
    for _ in range(200):
        raw = bytes(rng.randrange(256) for _ in range(16))
        w = (ctypes.c_uint32 * 4).from_buffer_copy(raw)
        plan.fp_upper16(w)
        assert bytes(w) == _findzip.to_upper(raw)


def test_length_check_and_the_string_as_the_kernel_takes_it(plan):
    assert [plan.fp_check_len(n) for n in (0, 1, 1024, 1025)] == [-1, 0, 0, -1]
    buf, out = ctypes.create_string_buffer(1024), (ctypes.c_uint32 * 7)()
    assert plan.fp_needle(b"", 0, 1, buf, out) == -1 and plan.fp_needle(b"x" * 1025, 1025, 1, buf, out) == -1
    for text, fold in ((b"a", 1), (b"ab", 1), (b"\xe0bc", 1), (b"abcd", 0), (b"xyz\xff\xf7q", 1), (b"abcdefg", 1), (b"abcdefgh", 0), (b"q" * 1024, 1)):
        assert plan.fp_needle(text, len(text), fold, buf, out) == 0
        want = _findzip.to_upper(text) if fold else text
        assert buf.raw == bytes(1024 - len(text)) + want
        tail = (bytes(4) + want)[-4:]
        assert out[0] == len(text) and out[1] == int.from_bytes(tail, "little") and out[4] == fold
        assert out[2] == (0xFFFFFFFF << (8 * max(0, 4 - len(text)))) & 0xFFFFFFFF and out[3] == want[-1] * 0x01010101
        front = (bytes(8) + want)[-8:-4]
        assert out[5] == int.from_bytes(front, "little") and out[6] == int.from_bytes(bytes(0xFF if b else 0 for b in (bytes(8) + b"\1" * len(text))[-8:-4]), "little")
    for text in (b"", b"x" * 1025):
        with pytest.raises(ValueError, match="Constraint_Error"):
            _findzip.prepare_search_string(text)


def listed_cases():
    """(entry, string, ignore_case, phase): the lists the GPU tests run too (tests/_findzip.py), each at some phase of its 16-byte word."""
    for k, (x, s) in enumerate(_findzip.grid_cases()):
        yield x, s, True, (len(x) + 3 * len(s) + k) % 16
    for k, (x, s, fold) in enumerate(_findzip.named_cases()):
        yield x, s, fold, (5 * k + 1) % 16


def random_cases(count=400):
    rng = random.Random(21)
    for _ in range(count):
        stl = rng.choice((1, 2, 3, 4, 5, 6, 17, rng.randrange(1, 40)))
        s = bytes(rng.choice(ALPHABET) for _ in range(stl))
        if rng.random() < 0.3:
            s = b" " * rng.randrange(1, 4) + s
        x = bytearray(rng.choice(ALPHABET) for _ in range(rng.choice((0, 1, 5, 33, 300, 3000))))
        for _ in range(rng.randrange(0, 4)):
            if len(x):
                at = rng.randrange(len(x))
                x[at:at + len(s)] = s
                del x[3000:]
        yield bytes(x), s, rng.random() < 0.8, rng.randrange(16)


def test_the_model_of_the_kernel_against_the_literal_loop(plan):
    seen = 0
    for x, s, fold, phase in list(listed_cases()) + list(random_cases()):
        want = _findzip.search_1_file(x, s, fold)
        assert want == _findzip.closed_form(x, s, fold), (len(x), s[:20], fold)
        assert model(plan, x, s, fold, phase) == want, (len(x), s[:20], fold, phase)
        seen += want[0] > 0
    assert seen > 150


def test_bytes_around_the_entry_do_not_count(plan):
    """Non-space bytes where the virtual spaces are expected, the string's own head where a real match would need it, the string's tail behind."""
    assert model(plan, b"ab", b"  ab", front=b"#" * 2048) == (1, 1)
    assert model(plan, b"cd", b"abcd", front=b"#" * 2046 + b"ab") == (0, 2)
    assert model(plan, b"ab", b"abcd", behind=b"cd" * 1024) == (0, 2)
    assert model(plan, b" ab", b"  ab", phase=9, front=b"#" * 2048) == (1, 2)
    assert model(plan, b"q ab", b"  ab", phase=9, front=b" " * 2048) == (0, 4)


def test_checks_and_groups(plan):
    rows = np.zeros(5, dtype=DT)
    rows["n_in"], rows["cap"], rows["method"] = 10, (100, 300, 1 << 20, 50, 70), 8
    bad, why = ctypes.c_int(9), ctypes.c_int(9)
    assert plan.fp_check(rows.ctypes.data, 5, 10, 0, ctypes.byref(bad), ctypes.byref(why)) == 0 and bad.value == -1
    rows["in_off"][3] = 1
    assert plan.fp_check(rows.ctypes.data, 5, 10, 0, ctypes.byref(bad), ctypes.byref(why)) == -1 and (bad.value, why.value) == (3, 3)
    rows["in_off"][3] = 0
    rows["flags"][1] = 1
    assert plan.fp_check(rows.ctypes.data, 5, 10, 0, ctypes.byref(bad), ctypes.byref(why)) == -1 and (bad.value, why.value) == (1, 5)
    assert plan.fp_check(rows.ctypes.data, 5, 10, 1, ctypes.byref(bad), ctypes.byref(why)) == 0
    rows["out_off"] = 1 << 50                                # ignored
    assert plan.fp_check(rows.ctypes.data, 5, 10, 1, ctypes.byref(bad), ctypes.byref(why)) == 0
    rows["cap"][4] = 1 << 40
    assert plan.fp_check(rows.ctypes.data, 5, 10, 1, ctypes.byref(bad), ctypes.byref(why)) == -4 and bad.value == 4
    rows["cap"][4] = 70
    ends = (ctypes.c_int * 8)()
    n = plan.fp_groups(rows.ctypes.data, 5, 1024, ends, 8)                 # slots of 256, 512, 1 MiB, 256, 256: the large one runs alone
    assert list(ends[:n]) == [2, 3, 5]
    assert plan.fp_piece_log() == 14 and [plan.fp_piece_count(v) for v in (0, 1, PIECE, PIECE + 1)] == [0, 1, 1, 2]


def test_the_same_lists_under_the_sanitizers(plan, tmp_path):
    """A program of its own (its own main, -fsanitize=address,undefined), run as a child process on the tables, the SWAR helpers and the cases of
    the tests above: it ends clean and prints what the restatements give."""
    exe = str(tmp_path / "find_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DFIND_PLAN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", exe, _findzip.SRC],
                   check=True)
    lines = ["T"]
    want = [bytes(_findzip.to_upper_char(c) for c in range(256)).hex() + " " + bytes(_findzip.to_lower_char(c) for c in range(256)).hex()]
    rng = random.Random(2)
    for _ in range(300):
        b = bytes(rng.choice(b"a\xe0\xf7\xff z{`\x7f\xde") if rng.random() < 0.6 else rng.randrange(256) for _ in range(4))
        c = rng.choice(b)
        lines.append("U %08x %02x" % (int.from_bytes(b, "little"), c))
        want.append("%08x %08x" % (int.from_bytes(_findzip.to_upper(b), "little"), sum(0x80 << (8 * i) for i in range(4) if b[i] == c)))
    for x, s, fold, phase in list(listed_cases()) + list(random_cases(150)):
        lines.append("S %d %d %s %s" % (fold, phase, s.hex(), x.hex() or "-"))
        want.append("%d %d" % _findzip.search_1_file(x, s, fold))
    lines.append("S 1 0 - 6162")
    want.append("refused")
    lines.append("S 1 0 %s 6162" % (b"x" * 1025).hex())
    want.append("refused")
    src = tmp_path / "cases.txt"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert got[-1] == "plan ok" and got[:-1] == want
