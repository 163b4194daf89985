"""Deflate_3's lazy window descriptors (knob "descr_lazy", zip-ada_amd/csrc/zada_huff.hip: k_piece_masks / k_cut_scan_lazy) against the full
path ("descr_lazy" 0: every window's descriptor) and against the oracle: the same stream, CRC, blocks, cuts and distances, with the
counters of last_timing showing that the lazy path did run -- and did not for Deflate_2 / Deflate_1, which have no test point at step
level 3 only."""
import numpy as np
import pytest

from _common import edge_inputs, oracle_deflate, oracle_tokens, silesia_mix

pytestmark = pytest.mark.gpu

ONE_FLUSH_4096 = 396610          # bytes of the text class that Deflate_3 and Deflate_2 parse into 65 536 + 4 096 atoms (found with the oracle)
_cache = {}


def _inputs():
    if "in" not in _cache:
        e = edge_inputs()
        d = {name: e[name] for name in ("mix_1m_off", "text_rand_text", "copies_1500k", "fixedlike_mix")}   # (copies_1500k: the null-slice input)
        for m in (1, 8, 16, 0x1F):
            d["mix3m_%02x" % m] = silesia_mix(3 << 20, class_mask=m)
        d["flush_plus_4096"] = silesia_mix(1 << 20, class_mask=1)[:ONE_FLUSH_4096]
        _cache["in"] = d
    return _cache["in"]


NAMES = ("mix_1m_off", "text_rand_text", "copies_1500k", "fixedlike_mix", "mix3m_01", "mix3m_08", "mix3m_10", "mix3m_1f", "flush_plus_4096")


def _oracle(name, method):
    key = (name, method)
    if key not in _cache:
        blocks, cuts, sim = [], [], []
        rc, ref, crc = oracle_deflate(_inputs()[name], method, blocks, cuts, sim)
        _cache[key] = (rc, ref, crc, blocks, cuts, sim)
    return _cache[key]


def _counters(enc):
    t = dict(enc.last_timing())
    return int(t["#descr_l3_points"]), int(t["#descr_excluded"]), int(t["#descr_late"])


def _run(enc, d, method, lazy):
    enc.set_knob("descr_lazy", lazy)
    try:
        out, crc = enc.deflate(d, method)
        cnt = _counters(enc)
        blocks = [tuple(int(x) for x in r) for r in enc.last_blocks()]
        trace = [tuple(int(x) for x in r) for r in enc.last_trace()]
        return out, crc, cnt, blocks, trace
    finally:
        enc.set_knob("descr_lazy", 1)


@pytest.mark.parametrize("name", NAMES)
def test_lazy_descriptors_equal_the_full_path_and_the_oracle(encoder, name):
    d = _inputs()[name]
    if name == "flush_plus_4096":
        assert len(oracle_tokens(d, 10)) == 65536 + 4096
    for method in (10, 9, 8):
        rc, ref, crc, oblocks, ocuts, osim = _oracle(name, method)
        assert rc == 0
        got = {lazy: _run(encoder, d, method, lazy) for lazy in (1, 0)}
        for lazy in (1, 0):
            out, crc2, cnt, blocks, trace = got[lazy]
            assert out == ref and crc2 == crc, (name, method, lazy)
            assert blocks == oblocks, (name, method, lazy)
            dist = {a: b for a, b, _ in trace}
            assert len(osim) > 0 and all(dist.get(w) == dd for w, dd, _, _ in osim), (name, method, lazy)
            assert sorted(set(w for w, _, _, _ in osim)) == sorted(dist), (name, method, lazy)
            assert [(a, c) for a, _, c in trace if c] == ocuts, (name, method, lazy)
        assert got[1][3] == got[0][3] and got[1][4] == got[0][4], (name, method)
        l3, excluded, late = got[1][2]
        print(name, method, "l3 points %d excluded %d late %d" % (l3, excluded, late))
        assert got[0][2] == (0, 0, 0), (name, method)                          # the full path counts nothing
        if method == 10:
            # every level-3-only test point (slot k of its flush with k % 4 /= 0; the oracle lists a slot once per level it tests there) is
            # either decided by the bound or gets its descriptor inside the scan
            points = set(w for w, _, _, _ in osim if (w % 65536) // 750 % 4)
            assert l3 == len(points) and excluded + late == l3, (name, l3, excluded, late)
            if name in ("mix_1m_off", "mix3m_01", "flush_plus_4096"):
                assert excluded > 0, name                                         # text: the bound decides
            # the empty windows of the null slice (slots 1 and 2 of every even flush) are always built in the scan
            empty = sum(1 for w in points if (w // 65536) % 2 == 0 and (w % 65536) // 750 in (1, 2))
            assert late >= empty, (name, late, empty)
            if name == "copies_1500k":
                assert empty > 0 and late > 0, name
            if name == "text_rand_text":
                assert late > empty, (name, late, empty)                          # text against random bytes: a bound of 205 000 or more leads to a descriptor
        else:
            assert (l3, excluded, late) == (0, 0, 0), (name, method)


def test_lazy_descriptors_in_a_batch(encoder):
    """Two entries through one launch sequence (zada_deflate_batch: the flush table, one flush grid per entry): streams and CRCs against the
    oracle, blocks and trace of the batch the same with the lazy path and without."""
    text = silesia_mix(1 << 20, class_mask=1)
    datas = [text[:700000], edge_inputs()["copies_1500k"][:900000]]
    got = {}
    for lazy in (1, 0):
        encoder.set_knob("descr_lazy", lazy)
        try:
            res = encoder.deflate_batch(datas, 10)
            cnt = _counters(encoder)
            got[lazy] = (res, cnt, [tuple(int(x) for x in r) for r in encoder.last_blocks()], [tuple(int(x) for x in r) for r in encoder.last_trace()])
        finally:
            encoder.set_knob("descr_lazy", 1)
        for d, (rc2, out, crc2) in zip(datas, res):
            rc, ref, crc = oracle_deflate(d, 10)
            assert rc == rc2 == 0 and out == ref and crc2 == crc, (lazy, len(d))
    assert got[1][2] == got[0][2] and got[1][3] == got[0][3] and len(got[1][3]) > 0
    l3, excluded, late = got[1][1]
    print("batch: l3 points %d excluded %d late %d" % (l3, excluded, late))
    assert got[0][1] == (0, 0, 0) and excluded > 0 and late > 0 and excluded + late == l3


def test_counters_cover_every_span_of_a_call(encoder):
    """A stream taken span after span ("span_mib" 1 on 3 MiB): the same bytes, and the counters of last_timing count the whole call, not its last span."""
    name = "mix3m_1f"
    d = _inputs()[name]
    rc, ref, crc, _, _, osim = _oracle(name, 10)
    points = set(w for w, _, _, _ in osim if (w % 65536) // 750 % 4)
    encoder.set_knob("span_mib", 1)
    try:
        out, crc2 = encoder.deflate(d, 10)
        l3, excluded, late = _counters(encoder)
    finally:
        encoder.set_knob("span_mib", 2048)
    assert rc == 0 and out == ref and crc2 == crc
    assert l3 == len(points) and excluded + late == l3 and excluded > 0, (l3, excluded, late, len(points))
