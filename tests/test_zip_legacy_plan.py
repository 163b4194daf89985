"""The host plans of zada_zip_device_ex and zada_rezip_device with and without the knobs "zip_legacy" and "unzip_legacy" (zada_zip_plan.h,
zada_rezip_plan.h through tests/zip_legacy/zip_legacy_plan_host.cpp): off, every answer is the one of before; on, Shrink_1 and Reduce_1 .. _4 are
methods of the writer with their own groups, shrink and reduce_4 approaches of ReZip with their size limits, sources of methods 1 .. 6 are known, and a
kept Implode stream keeps its two flag bits.  The model is tests/_rezip_legacy.py (tools/rezip_lib.adb:819-832, 1002-1007, 1072-1089)."""
import ctypes
import random

import numpy as np
import pytest

import _rezip
import _rezip_legacy as RL

E_INVALID, E_TOO_LARGE = -1, -4
G_BATCH, G_SINGLE = 0, 1
ZIP_DT = np.dtype([("d_data", "<u8"), ("n", "<u8"), ("name", "<u8"), ("name_len", "<u4"), ("time", "<u4"), ("flags", "<u4"), ("pad", "<u4")])
RZ_DT = np.dtype([("in_off", "<u8"), ("n_in", "<u8"), ("usize", "<u8"), ("crc", "<u4"), ("time", "<u4"), ("method", "<u2"), ("flags", "<u2"), ("version", "<u2"),
                  ("pad", "<u2"), ("name_len", "<u4"), ("pad2", "<u4"), ("name", "<u8")])
NT = RL.NOT_TRIED
RZ_W_METHOD = 2


@pytest.fixture(scope="module")
def plan():
    return RL.load_plan()


def test_knobs_off_every_answer_is_the_one_of_before(plan):
    base = _rezip.load_plan()
    for m in range(-1, 38):
        want = 1 if m == 0 or 6 <= m <= 35 else 0
        assert plan.zlp_method_ok(m, 0) == want and plan.zlp_method_ok_default(m) == want, m
    for approaches in (0x0FFF, 0x0FE7, 0x0018, 0x0019, 0x27, 0):
        for formats in (RL.ALL_FORMATS, RL.DEFLATE_OR_STORE, RL.FAST_DECOMPRESSION, 0x1E, 0):
            want = base.rp_considered(approaches, formats)
            assert plan.zlp_considered(approaches, formats, 0) == want and plan.zlp_considered_default(approaches, formats) == want
            assert not want & RL.LEGACY
    assert plan.zlp_considered(0x0FFF, RL.ALL_FORMATS, 0) == 0x0FE7
    out, out0 = (ctypes.c_int * 12)(), (ctypes.c_int * 12)()
    for considered in (0x0FE7, 0x27, 0x0C07, 1):
        for usize in (0, 6001, 1 << 20):
            k = plan.zlp_methods(considered, 15, 9, usize, out)
            assert list(out[:k]) == list(out0[:plan.zlp_methods_default(considered, 15, 9, out0)]) == list(out0[:base.rp_methods(considered, 15, 9, out0)])
    # sources of methods 1 .. 6: refused with the text of before
    old = b"unknown source method (0 Store, 8 Deflate, 9 Deflate64, 12 BZip2, 14 LZMA)"
    assert plan.zlp_rz_why_text(RZ_W_METHOD, 0) == old == plan.zlp_rz_why_text_default(RZ_W_METHOD)
    for m in (1, 2, 5, 6, 7):
        t, keep = rz_table([(b"a", 0, 5, 5, 0, 0), (b"b", 5, 5, 9, m, 0)])
        bad, why = ctypes.c_int(-9), ctypes.c_int(-9)
        assert plan.zlp_rz_check(t.ctypes.data, 2, 100, 0, ctypes.byref(bad), ctypes.byref(why)) == E_INVALID and (bad.value, why.value) == (1, RZ_W_METHOD)
        assert plan.zlp_rz_check_default(t.ctypes.data, 2, 100, ctypes.byref(bad), ctypes.byref(why)) == E_INVALID and (bad.value, why.value) == (1, RZ_W_METHOD)
    # the flag word without `kept`: the reference's mask, whatever the source
    assert plan.zlp_flag(6, 6, 6, 0, 0) == 4 and plan.zlp_flag(14, 0x080A, 14, 1, 0) == 0x0802


def test_methods_and_zip_types(plan):
    assert [plan.zlp_method_ok(m, 1) for m in (-1, 0, 1, 2, 3, 4, 5, 6, 35, 36)] == [0, 1, 1, 1, 1, 1, 1, 1, 1, 0]
    assert [plan.zlp_zip_type(m) for m in (0, 1, 2, 3, 4, 5, 6, 11, 12, 14, 15, 33)] == [0, 1, 2, 3, 4, 5, 8, 8, 12, 12, 14, 14]
    assert [plan.zlp_slot(n) for n in (0, 1, 63, 64, 65, 6000)] == [64, 64, 64, 64, 128, 6016]
    t = zip_table([5, (1 << 30) - 65537, (1 << 30) - 65536, 1 << 31])
    assert plan.zlp_too_large(t.ctypes.data, 2) == -1 and plan.zlp_too_large(t.ctypes.data, 4) == 2


def zip_table(sizes):
    t = np.zeros(len(sizes), dtype=ZIP_DT)
    t["n"] = sizes
    t["d_data"] = 4096
    return t


def groups_of(plan, sizes, method, limit, work_limit):
    t = zip_table(sizes)
    out = (ctypes.c_int * (3 * (len(sizes) + 1)))()
    k = plan.zlp_groups(t.ctypes.data, len(sizes), method, limit, work_limit, out, len(sizes) + 1)
    return [tuple(out[3 * j:3 * j + 3]) for j in range(k)]


def test_groups_hold_their_three_bounds(plan):
    """Random size lists under Shrink_1 and Reduce_4, with the default knobs, with reduce_group_mib = 1 and with batch_mib = 1: every entry once and
    in order; a group of one, or an entry above ZW_ENTRY_MAX, is single; a group's slots stay within the limit and below 2 ** 32, a Reduce group's work
    arrays within theirs; and no group could have taken the next entry too (the groups are as large as the rules allow)."""
    r = random.Random(31)
    emax = plan.zlp_entry_max()
    seen = dict(single=0, batch=0, work_cut=0, slot_cut=0, big=0)
    for trial in range(60):
        sizes = [r.choice((0, 1, 63, 64, 65, 6000, 9000, 70000, 300000, emax, emax + 1, 6 << 20)) if r.random() < 0.5 else r.randint(0, 200000) for _ in range(r.randint(1, 80))]
        for method in (1, 5):
            for limit, work in ((512 << 20, 4096 << 20), (512 << 20, 1 << 20), (1 << 20, 4096 << 20), (8 << 30, 4096 << 20)):
                gs = groups_of(plan, sizes, method, limit, work)
                assert [g[0] for g in gs] == [0] + [g[1] for g in gs[:-1]] and gs[-1][1] == len(sizes) and all(g[1] > g[0] for g in gs)
                lim = min(limit, 1 << 30)
                for j, (g0, g1, kind) in enumerate(gs):
                    slots = sum(2 * plan.zlp_slot(n) for n in sizes[g0:g1])
                    wk = sum(plan.zlp_footprint(n) for n in sizes[g0:g1]) if method != 1 else 0
                    assert kind == (G_SINGLE if g1 - g0 == 1 else G_BATCH)
                    if g1 - g0 > 1:
                        assert slots <= lim and slots < 1 << 32 and wk <= work and max(sizes[g0:g1]) <= emax
                        seen["batch"] += 1
                    else:
                        seen["single"] += 1
                        seen["big"] += sizes[g0] > emax
                    if g1 < len(sizes) and sizes[g1] <= emax and max(sizes[g0:g1]) <= emax:      # why the next entry was not taken
                        s2, w2 = slots + 2 * plan.zlp_slot(sizes[g1]), wk + (plan.zlp_footprint(sizes[g1]) if method != 1 else 0)
                        assert s2 > lim or w2 > work
                        seen["slot_cut"] += s2 > lim
                        seen["work_cut"] += w2 > work
    assert all(seen.values()), seen
    assert groups_of(plan, [], 1, 1 << 20, 1 << 20) == []


def test_considered_is_the_models(plan):
    for approaches in (RL.TWELVE, RL.DEFAULT, RL.LEGACY, 0x0008, 0x0010, 0x0C18, 0):
        for formats in (RL.ALL_FORMATS, RL.DEFLATE_OR_STORE, RL.FAST_DECOMPRESSION):
            want = sum(1 << a for a, c in enumerate(RL.consider_a_priori(approaches, formats)) if c)
            assert plan.zlp_considered(approaches, formats, 1) == want, (approaches, formats)
    assert plan.zlp_considered(RL.TWELVE, RL.ALL_FORMATS, 1) == RL.TWELVE
    assert plan.zlp_considered(RL.TWELVE, RL.DEFLATE_OR_STORE, 1) == 1 | 1 << 5 | 1 << 6
    assert plan.zlp_considered(RL.TWELVE, RL.FAST_DECOMPRESSION, 1) == 1 | 1 << 5 | 1 << 6 | 1 << 10 | 1 << 11


def test_methods_per_entry_at_the_size_limits(plan):
    out = (ctypes.c_int * 12)()
    for usize, shrink, reduce in ((5999, 1, 1), (6000, 1, 1), (6001, 0, 1), (8999, 0, 1), (9000, 0, 1), (9001, 0, 0), (0, 1, 1)):
        for approaches in (RL.TWELVE, RL.LEGACY | 1, 0x0009, 0x0011):
            consider = RL.consider_entry(RL.consider_a_priori(approaches, RL.ALL_FORMATS), usize)
            assert (consider[RL.SHRINK], consider[RL.REDUCE_4]) == (bool(shrink and approaches & 8), bool(reduce and approaches & 16))
            want = sorted({15 if a == 1 else 9 if a == 2 else RL.METHOD[a] for a in range(1, 12) if consider[a]})
            considered = plan.zlp_considered(approaches, RL.ALL_FORMATS, 1)
            k = plan.zlp_methods(considered, 15, 9, usize, out)
            assert list(out[:k]) == want, (usize, approaches)
            assert plan.zlp_considered_entry(considered, usize) == sum(1 << a for a, c in enumerate(consider) if c)


def choose(plan, size, allowed):
    return plan.zlp_choose((ctypes.c_uint64 * 12)(*size), 1 if allowed else 0)


def test_choice_with_a_legacy_original(plan):
    for m in (1, 2, 3, 4, 5, 6):
        assert plan.zlp_original_allowed(RL.ALL_FORMATS, m) == 1
        assert plan.zlp_original_allowed(RL.DEFLATE_OR_STORE, m) == 0 and plan.zlp_original_allowed(RL.FAST_DECOMPRESSION, m) == 0
        assert RL.format_choice(RL.ALL_FORMATS, m) and not RL.format_choice(RL.DEFLATE_OR_STORE, m)
    for zt in (0, 8, 9, 12, 14):
        for formats in (RL.ALL_FORMATS, RL.DEFLATE_OR_STORE, RL.FAST_DECOMPRESSION):
            assert plan.zlp_original_allowed(formats, zt) == int(RL.format_choice(formats, zt))
    for formats in (RL.ALL_FORMATS, RL.DEFLATE_OR_STORE):
        allowed = RL.format_choice(formats, 1)
        for usize in (100, 7000, 20000):
            consider = RL.consider_entry(RL.consider_a_priori(RL.TWELVE, formats), usize)
            for orig, other in ((50, 50), (50, 90), (90, 50)):
                size = [other + a if consider[a] else NT for a in range(12)]
                size[0] = orig
                got = choose(plan, size, allowed)
                assert got == RL.try_all_approaches(consider, [0 if x == NT else x for x in size], allowed)
                if not allowed:
                    assert got != 0                            # forced out, even at a larger size (:880-886)
    # a Shrink stream that wins, and one that ties with original
    size = [NT] * 12
    size[0], size[3], size[4], size[5] = 100, 80, 80, 81
    assert choose(plan, size, True) == 3
    size[0] = 80
    assert choose(plan, size, True) == 0


def test_flag_word(plan):
    cases = [(6, 6, 6, 0, 1, 6),           # an Implode original that is kept: bits 1 and 2 stay (the departure)
             (6, 6, 8, 0, 0, 4),           # ... beaten by Deflate: the reference's mask
             (14, 2, 14, 1, 1, 2),         # LZMA with EOS, kept
             (14, 2, 14, 1, 0, 2),
             (14, 0x000A, 8, 0, 0, 0),
             (1, 0, 1, 0, 1, 0),           # Shrink: no flag bits of its own
             (1, 0x0808, 1, 0, 1, 0x0800),
             (8, 6, 8, 0, 1, 4),           # a kept Deflate stream: the mask (only method 6 keeps bit 1)
             (6, 2, 6, 0, 1, 2), (6, 4, 6, 0, 1, 4), (6, 0x080E, 6, 0, 1, 0x0806)]
    for method, flags, zt, eos, kept, want in cases:
        assert plan.zlp_flag(method, flags, zt, eos, kept) == want == RL.kept_flag(method, flags, kept, eos), (method, flags, kept)


def rz_table(rows):
    tab = np.zeros(len(rows), dtype=RZ_DT)
    blob = np.frombuffer(b"".join(r[0] for r in rows) + b"\0", dtype=np.uint8)
    at = 0
    for k, (nm, in_off, n_in, usize, method, flags) in enumerate(rows):
        tab[k] = (in_off, n_in, usize, 0x1234 + k, 0x5A210000 + k, method, flags, 10 + k % 11, 0, len(nm), 0, blob.ctypes.data + at)
        at += len(nm)
    return tab, blob


def test_sources_of_methods_1_to_6_are_known(plan):
    new = b"unknown method (0 Store, 1 Shrink, 2 .. 5 Reduce, 6 Implode, 8 Deflate, 9 Deflate64, 12 BZip2, 14 LZMA)"
    assert plan.zlp_rz_why_text(RZ_W_METHOD, 1) == new
    bad, why = ctypes.c_int(-9), ctypes.c_int(-9)
    t, keep = rz_table([(b"n%d" % m, 5 * k, 5, 9, m, 6 if m == 6 else 0) for k, m in enumerate((0, 1, 2, 3, 4, 5, 6, 8, 9, 12, 14))])
    assert plan.zlp_rz_check(t.ctypes.data, len(t), 100, 1, ctypes.byref(bad), ctypes.byref(why)) == 0
    for m in (7, 10, 13, 99):
        t, keep = rz_table([(b"a", 0, 5, 5, 1, 0), (b"b", 5, 5, 9, m, 0)])
        assert plan.zlp_rz_check(t.ctypes.data, 2, 100, 1, ctypes.byref(bad), ctypes.byref(why)) == E_INVALID and (bad.value, why.value) == (1, RZ_W_METHOD)
    t, keep = rz_table([(b"a", 0, 5, 5, 1, 1)])              # the other rules hold for a legacy row: encrypted
    assert plan.zlp_rz_check(t.ctypes.data, 1, 100, 1, ctypes.byref(bad), ctypes.byref(why)) == E_INVALID and why.value == 3


def test_archives_with_legacy_winners_and_kept_implode(plan):
    """Random directories: sources of every method, winners of zip types 1 and 5 among the others, Implode entries kept and beaten, dropped names,
    comments, a base: the plan's header bytes equal the model's."""
    r = random.Random(77)
    seen = dict(kept_implode=0, beaten_implode=0, shrink=0, reduce=0, eos=0)
    for trial in range(40):
        rows, winners, model = [], [], []
        for k in range(r.randint(1, 30)):
            method = r.choice((0, 1, 2, 5, 6, 6, 8, 9, 12, 14))
            flags = r.choice((0, 2, 4, 6, 8, 0x0806, 0x080E)) if method in (6, 14) else r.choice((0, 8, 0x0800))
            nm = (b"d%d/" % k) if r.random() < 0.1 else b"e%03d_%d.bin" % (k, r.randint(0, 999))
            usize, n_in = r.randint(0, 70000), r.randint(0, 70000)
            kept = r.random() < 0.5
            zt = method if kept else r.choice((0, 1, 5, 8, 12, 14))
            eos = (method == 14 and bool(flags & 2)) if kept else zt == 14
            csize = n_in if kept else r.randint(0, usize)
            rows.append((nm, 0, n_in, usize, method, flags))
            winners.append((csize, zt, eos, kept))
            if nm[-1:] != b"/":
                seen["kept_implode"] += kept and method == 6 and flags & 2 == 2
                seen["beaten_implode"] += (not kept) and method == 6 and flags & 2 == 2
                seen["shrink"] += zt == 1
                seen["reduce"] += zt == 5
                seen["eos"] += eos
        tab, keep = rz_table(rows)
        comment, base = r.choice((b"", b"a comment")), r.choice((0, 12345))
        for k, ((nm, _, n_in, usize, method, flags), (csize, zt, eos, kept)) in enumerate(zip(rows, winners)):
            if nm[-1:] != b"/":
                model.append(dict(name=nm, version=int(tab["version"][k]), flags=flags, time=int(tab["time"][k]), crc=int(tab["crc"][k]), usize=usize, method=method,
                                  csize=csize, zip_type=zt, eos=eos, kept=kept, payload=None))
        locals_, tail, offs, alen = RL.rezip_archive(model, base, comment)
        cs = np.array([w[0] for w in winners], dtype=np.uint64)
        zts = np.array([w[1] for w in winners], dtype=np.uint16)
        eo = np.array([w[2] for w in winners], dtype=np.uint8)
        kp = np.array([w[3] for w in winners], dtype=np.uint8)
        out = np.zeros(len(locals_) + len(tail) + 64, dtype=np.uint8)
        got_len = ctypes.c_uint64(0)
        k = plan.zlp_rz_archive(tab.ctypes.data, len(tab), cs.ctypes.data, zts.ctypes.data, eo.ctypes.data, kp.ctypes.data, base, comment, len(comment), out.ctypes.data,
                                len(out), ctypes.byref(got_len))
        assert out[:k].tobytes() == locals_ + tail and got_len.value == alen
    assert all(seen.values()), seen
