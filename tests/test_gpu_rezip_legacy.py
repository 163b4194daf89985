"""zada_rezip_device with the knobs "zip_legacy" (the approaches shrink and reduce_4) and "unzip_legacy" (source entries of methods 1 .. 6).  The
reference is never the code under test: the sizes of the two approaches come from the CPU models of Shrink_1 and Reduce_4 (tests/legacy/), the
choice from the approach loop and the archive bytes from the header model restated from the Ada text (tests/_rezip_legacy.py), the plaintexts of
PKZIP's own streams from the digests recorded with them (tests/golden/many_formats_legacy.json)."""
import hashlib
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import _legacy as L
import _rezip_legacy as RL
import _unlegacy as U
from _common import product
from _zip_legacy import knobs, model_stream
from test_gpu_rezip_device import Call, host_streams

pytestmark = pytest.mark.gpu
E_INVALID = -1
NT = RL.NOT_TRIED
LIMITS = (5999, 6000, 6001, 8999, 9000, 9001)
COMMENT = b"legacy sources"
# the entries the two approaches win under a mask of original and that approach alone (picked on the CPU with the models: a stored entry of text
# with matches in it, within the approach's size limit; the models' streams are 1 888 and 2 969 bytes)
SHRINK_WINS, REDUCE_4_WINS = b"st6000.txt", b"st9000.txt"


def plain_golden():
    row, payload = U.fixtures()[0]
    return U.host_decode(row["format"], row["flags"], payload, row["size"])[1]


_src = {}


def source(enc):
    """-> (archive bytes, {name without the directory entry: plaintext}).  PKZIP's seven streams (Reduce_1 .. _4, Shrink, Implode twice with flags 6),
    entries ZipCreate writes under Shrink_1 and Reduce_4, stored and Deflate entries on both sides of the two size limits, an empty entry and a
    directory entry; a comment."""
    if not _src:
        za = product()
        zc = za.ZipCreate(enc, 0)
        want = {}
        gold = plain_golden()
        for row, payload in U.fixtures():
            zc.add_compressed(row["file"], payload, int(row["crc32"], 16), row["size"], row["format"], flag_bits=row["flags"])
            want[row["file"]] = gold
        for nm, m, d in (("own_shrink.txt", 1, L.edge_input(20000, seed=5)), ("own_reduce4.txt", 5, L.edge_input(7000, seed=6)), ("own_shrink_small.txt", 1, L.edge_input(3000, seed=7))):
            zt, s = host_streams(enc, m, [d])[0]
            assert zt == zada_type(m)
            zc.add_compressed(nm, s, zlib.crc32(d), len(d), zt)
            want[nm] = d
        zc.add_compressed("dir/", b"", 0, 0, 0)
        for n in LIMITS:
            d = L.edge_input(n, seed=20)
            zc.add_compressed("st%d.txt" % n, d, zlib.crc32(d), n, 0)
            want["st%d.txt" % n] = d
            d = L.edge_input(n, seed=21)
            zt, s = host_streams(enc, 8, [d])[0]
            zc.add_compressed("df%d.txt" % n, s, zlib.crc32(d), n, zt)
            want["df%d.txt" % n] = d
        zc.add_compressed("empty", b"", 0, 0, 0)
        want["empty"] = b""
        arc = bytearray(zc.finish())
        arc[-2:] = len(COMMENT).to_bytes(2, "little")
        _src["a"] = (bytes(arc + COMMENT), want)
    return _src["a"]


def zada_type(m):
    return m if m <= 5 else 8


def run(enc, cap=None, approaches=RL.TWELVE, formats=RL.ALL_FORMATS, zip_legacy=1, unzip_legacy=1, arc=None, a_out=3):
    arc = source(enc)[0] if arc is None else arc
    c = Call(enc, arc, a_out)
    cap = enc.rezip_bound(c.tab, len(COMMENT)) if cap is None else cap
    with knobs(enc, zip_legacy=zip_legacy, unzip_legacy=unzip_legacy):
        rc, alen, res, sizes, buf, said = c.run(cap, approaches=approaches, formats=formats, comment=COMMENT)
    return c, rc, alen, res, sizes, buf, said


def check_against_model(enc, c, alen, res, sizes, buf, approaches, formats, arc=None):
    """The sizes of shrink and reduce_4 are the CPU models' (or not tried); every other approach is tried exactly where the model considers it; the
    choice is the approach loop's on the sizes the call reports; the archive is the header model's around the payloads that lie in it; a winner that
    is original is the source's stream, one of zip type 1 / 5 the CPU model's.  -> [(name, approach, zip type)] of the kept entries"""
    za = product()
    arc, want = (source(enc)[0] if arc is None else arc), source(enc)[1]
    order = za.zip_load_order(za.ZipInfo.load(arc))
    consider0 = RL.consider_a_priori(approaches, formats)
    rows, out = [], []
    for k, (key, e) in enumerate(order):
        row = [int(x) for x in sizes[k]]
        if key[-1:] == b"/":
            assert int(res["flags"][k]) & 1 and row == [NT] * 12
            continue
        d = want[key.decode()]
        consider = RL.consider_entry(consider0, e.usize)
        assert [x != NT for x in row] == consider, (key, row)
        assert row[0] == e.csize
        for a, m in ((RL.SHRINK, 1), (RL.REDUCE_4, 5)):
            if consider[a]:
                mrc, s, _ = model_stream(d, m)
                assert row[a] == (len(d) if mrc else len(s)), (key, a)
        choice = RL.try_all_approaches(consider, [0 if x == NT else x for x in row], RL.format_choice(formats, e.method))
        zt, csize, off = int(res["zip_type"][k]), int(res["csize"][k]), int(res["offset"][k])
        assert (int(res["rc"][k]), int(res["approach"][k]), csize, int(res["crc"][k])) == (0, choice, row[choice], e.crc), (key, row)
        payload = buf[off + 30 + len(key):off + 30 + len(key) + csize]
        if choice == 0:
            assert zt == e.method and payload == arc[e.data_offset:e.data_offset + e.csize], key
        elif choice in (RL.SHRINK, RL.REDUCE_4):
            mrc, s, _ = model_stream(d, 1 if choice == RL.SHRINK else 5)
            assert (zt, payload) == ((0, d) if mrc else (1 if choice == RL.SHRINK else 5, s)), key
        rows.append(dict(name=key, version=e.local_version, flags=e.local_flags, time=e.local_time, crc=e.crc, usize=e.usize, method=e.method, kept=choice == 0,
                         csize=csize, zip_type=zt, eos=(e.method == 14 and bool(e.local_flags & 2)) if choice == 0 else zt == 14, payload=payload))
        out.append((key, choice, zt))
    body, tail, offs, total = RL.rezip_archive(rows, 0, COMMENT)
    assert alen == total and buf[:alen] == body + tail
    return out


def extracts_to_the_inputs(enc, archive):
    import torch
    za = product()
    t = torch.from_numpy(np.frombuffer(archive, dtype=np.uint8).copy()).cuda()
    got = za.UnZip(enc, bzip2=True, lzma=True, legacy=True).extract_device(za.ZipInfo.load_device(t))
    assert {nm: bytes(v.cpu().numpy()) for nm, v in got.items()} == source(enc)[1]
    return t


def test_knobs(encoder):
    """Each knob alone leaves the other's refusal as it is today; both together: the call succeeds."""
    c, rc, _, _, _, buf, said = run(encoder, unzip_legacy=0)
    first = [k for k, (key, e) in enumerate(product().zip_load_order(product().ZipInfo.load(source(encoder)[0]))) if 1 <= e.method <= 6][0]
    assert rc == E_INVALID and said == "zada_rezip_device: entry %d: unknown source method (0 Store, 8 Deflate, 9 Deflate64, 12 BZip2, 14 LZMA)" % first
    for bit, text in ((3, "shrink (Shrink_1)"), (4, "reduce_4 (Reduce_4)")):
        c, rc, _, _, _, buf, said = run(encoder, approaches=RL.DEFAULT | 1 << bit, zip_legacy=0)
        assert rc == E_INVALID and said == "zada_rezip_device: approach %s is not taken by the device writer" % text
    c, rc, _, _, _, buf, said = run(encoder, approaches=1 | RL.LEGACY, zip_legacy=0, unzip_legacy=0)
    assert rc == E_INVALID and "is not taken by the device writer" in said
    c, rc, alen, res, sizes, buf, said = run(encoder, approaches=1 | RL.LEGACY)
    assert rc == 0 and alen > 0, said


@pytest.fixture(scope="module")
def twelve(encoder):
    c, rc, alen, res, sizes, buf, said = run(encoder)
    assert rc == 0, said
    return c, alen, res, sizes, buf


def test_all_twelve_approaches(encoder, twelve):
    c, alen, res, sizes, buf = twelve
    out = check_against_model(encoder, c, alen, res, sizes, buf, RL.TWELVE, RL.ALL_FORMATS)
    names = [key for key, _, _ in out]
    col = {key: [int(x) for x in sizes[k]] for k, (key, _) in enumerate(product().zip_load_order(product().ZipInfo.load(source(encoder)[0])))}
    for n in LIMITS:
        for pre in ("st", "df"):
            row = col[("%s%d.txt" % (pre, n)).encode()]
            assert (row[3] != NT, row[4] != NT) == (n <= 6000, n <= 9000), (pre, n)
    for key in names:
        if key.startswith(b"many_formats"):
            assert col[key][3] == col[key][4] == NT                   # 81 682 bytes: beyond both limits
    extracts_to_the_inputs(encoder, buf[:alen])


def test_exact_capacity(encoder, twelve):
    c, alen, res, sizes, buf = twelve
    c2, rc, alen2, _, _, buf2, said = run(encoder, cap=alen)
    assert rc == 0 and alen2 == alen and buf2 == buf[:alen], said
    c2, rc, _, _, _, _, said = run(encoder, cap=alen - 1)
    assert rc == E_INVALID and said == "zada_rezip_device: archive buffer too small"


@pytest.mark.parametrize("approach", (RL.SHRINK, RL.REDUCE_4))
def test_original_or_one_legacy_approach(encoder, approach):
    """Mask original | shrink, and original | reduce_4: the stored entries within the limit are won by the approach, with zip type 1 / 5"""
    c, rc, alen, res, sizes, buf, said = run(encoder, approaches=1 | 1 << approach)
    assert rc == 0, said
    out = check_against_model(encoder, c, alen, res, sizes, buf, 1 | 1 << approach, RL.ALL_FORMATS)
    won = {key: zt for key, a, zt in out if a == approach}
    assert won.get(SHRINK_WINS if approach == RL.SHRINK else REDUCE_4_WINS) == (1 if approach == RL.SHRINK else 5), won
    limit = 6000 if approach == RL.SHRINK else 9000
    assert all(a == 0 for key, a, zt in out if len(source(encoder)[1][key.decode()]) > limit)
    extracts_to_the_inputs(encoder, buf[:alen])


def test_original_only_keeps_every_legacy_stream(encoder, tmp_path):
    """approaches = original: the legacy sources are kept, the Implode entries with flag bits 1 and 2 in both headers (the departure from the
    reference's mask); the result extracts to the recorded digests, compares equal to the source but for the directory entry, and Info-ZIP's unzip
    accepts every entry it has a decoder for (it is built without one for Reduce)."""
    za = product()
    c, rc, alen, res, sizes, buf, said = run(encoder, approaches=1)
    assert rc == 0, said
    out = check_against_model(encoder, c, alen, res, sizes, buf, 1, RL.ALL_FORMATS)
    assert all(a == 0 for _, a, _ in out)
    result = buf[:alen]
    info = za.ZipInfo.load(result)
    by_name = {e.name: e for e in info.entries}
    for row, payload in U.fixtures():
        e = by_name[row["file"]]
        assert e.method == row["format"] and result[e.data_offset:e.data_offset + e.csize] == payload
        if row["format"] == 6:
            assert row["flags"] == 6 and e.flags & 6 == 6 and e.local_flags & 6 == 6
    t = extracts_to_the_inputs(encoder, result)
    got = za.UnZip(encoder, legacy=True).extract_device(za.ZipInfo.load_device(t), what=[row["file"] for row, _ in U.fixtures()])
    for row, _ in U.fixtures():
        d = bytes(got[row["file"]].cpu().numpy())
        assert "%08x" % zlib.crc32(d) == row["crc32"] and hashlib.sha256(d).hexdigest() == row["sha256"] and len(d) == row["size"]
    import torch
    ts = torch.from_numpy(np.frombuffer(source(encoder)[0], dtype=np.uint8).copy()).cuda()
    r = za.CompZip(encoder, legacy=True).compare_device(za.ZipInfo.load_device(ts), za.ZipInfo.load_device(t))
    assert (r.size_failures, r.compare_failures, r.damaged, r.missing_1_in_2, r.just_a_directory, r.missing_2_in_1) == (0, 0, 0, 1, 1, 0)
    if shutil.which("unzip"):
        p = os.path.join(str(tmp_path), "kept.zip")
        with open(p, "wb") as f:
            f.write(result)
        u = subprocess.run(["unzip", "-t", p], capture_output=True, timeout=60)
        lines = u.stdout.decode("latin-1").splitlines()
        ok = {ln.split()[1] for ln in lines if ln.strip().startswith("testing:") and ln.rstrip().endswith("OK")}
        reduce_names = {e.name for e in info.entries if 2 <= e.method <= 5}
        assert ok >= {e.name for e in info.entries} - reduce_names, u.stdout[-600:]
        skipped = {ln.split()[1] for ln in lines if ln.strip().startswith("skipping:")}
        assert (u.returncode, skipped) in ((0, set()), (81, reduce_names)), (u.returncode, u.stdout[-600:])      # (81: entries skipped for their method)


def test_deflate_or_store_forces_every_legacy_original_out(encoder):
    c, rc, alen, res, sizes, buf, said = run(encoder, formats=RL.DEFLATE_OR_STORE)
    assert rc == 0, said
    out = check_against_model(encoder, c, alen, res, sizes, buf, RL.TWELVE, RL.DEFLATE_OR_STORE)
    assert all(zt in (0, 8) for _, _, zt in out)
    assert all(int(row[3]) == NT and int(row[4]) == NT for row in sizes)
    src = {e.name.encode(): e for e in product().ZipInfo.load(source(encoder)[0]).entries}
    forced = [key for key, a, _ in out if 1 <= src[key].method <= 6]
    assert len(forced) == 10 and all(a != 0 for key, a, _ in out if key in forced)
    extracts_to_the_inputs(encoder, buf[:alen])


def test_python(encoder, twelve):
    import torch
    za = product()
    arc, want = source(encoder)
    t = torch.from_numpy(np.frombuffer(arc, dtype=np.uint8).copy()).cuda()
    rz = za.ReZip(encoder, legacy=True)
    out, rep = rz.rezip_device(za.ZipInfo.load_device(t), report=True)          # approaches=None: all twelve
    _, alen, _, _, buf = twelve
    assert bytes(out.cpu().numpy()) == buf[:alen]
    assert set(rep["totals"]) == set(za.RZ_APPROACHES) and any("shrink" in row and "reduce_4" in row for _, row, _ in rep["entries"])
    assert sum(v["count"] for v in rep["totals"].values()) == len(want)
    out2, rep2 = rz.rezip_device(za.ZipInfo.load_device(t), approaches=("original", "shrink", "reduce_4"), report=True)
    assert rep2["totals"]["shrink"]["count"] >= 1 and rep2["totals"]["reduce_4"]["count"] >= 1 and rep2["totals"]["shrink"]["saved"] > 0
    assert all(set(row) <= {"original", "shrink", "reduce_4"} for _, row, _ in rep2["entries"])
    assert rz.rezip(arc, approaches=("original", "shrink", "reduce_4")) == bytes(out2.cpu().numpy())
    # the knobs were set around the calls only: without the keyword, today's refusals
    with pytest.raises(za.UnsupportedMethod):
        za.ReZip(encoder).rezip_device(za.ZipInfo.load_device(t))
    zc = za.ZipCreate(encoder, 0)
    zc.add_stream("a.txt", L.edge_input(3000))
    plain = zc.finish()
    with pytest.raises(za.ZadaError, match=r"approach shrink \(Shrink_1\) is not taken by the device writer"):
        za.ReZip(encoder).rezip(plain, approaches=("original", "shrink"))
    with pytest.raises(za.ZadaError, match=r"approach reduce_4 \(Reduce_4\) is not taken by the device writer"):
        za.ReZip(encoder).rezip(plain, approaches=0x0FE7 | 0x10)
    assert za.ReZip(encoder).rezip(plain, approaches=None) == za.ReZip(encoder).rezip(plain, approaches=0x0FE7)
