"""CPU tests of the Deflate_R model (tests/rich/rich_model.c): the literal restatement of LZ77_by_Rich and the per-sector
closed form the GPU implements give the same tokens, and the streams built from them decode."""
import zlib

import numpy as np
import pytest

import _rich
from _common import edge_inputs, silesia_mix

# A case where the unwritten ring bytes decide a token: near the end of the stream, in the ring's first lap, a comparison
# reads past the loaded bytes (found by a seeded search over short inputs of four symbols).
FILL_CASE = b"a\x00a\x00\xff\xffaaaabab\x00\x00\x00\x00\x00\x00a\x00abbb\x00bbbb\xffb\x00a\xffb\x00\x00"


def rich_cases():
    """Rich-specific inputs: sector edges, the first Delete_Data, short final sectors, degenerate and few-symbol data."""
    rs = np.random.RandomState(11)
    cases = {}
    for k in range(1, 6):
        for d in range(-3, 4):
            cases["sector_%d%+d" % (k, d)] = silesia_mix(8192 * k + d, class_mask=1, offset=k * 65536)
    for n in (32768, 40960 - 3, 40960 - 1, 40960, 40960 + 1, 40960 + 3):
        cases["delete_%d" % n] = silesia_mix(n)
    for tail in (1, 2, 3):
        cases["final_%d" % tail] = silesia_mix(3 * 8192 + tail, class_mask=2)
    cases["zeros_70000"] = bytes(70000)
    cases["ab_41000"] = b"ab" * 20500
    cases["two_symbol_50000"] = bytes(rs.randint(0, 2, 50000).astype(np.uint8))
    cases["mix_v2_300000"] = silesia_mix(300000, version=2)
    cases["fill_case"] = FILL_CASE
    return cases


def all_cases():
    c = dict(edge_inputs())
    c.update(rich_cases())
    return c


@pytest.fixture(scope="module")
def cases():
    return all_cases()


def test_restatement_equals_closed_form(cases):
    for name, d in cases.items():
        a, _ = _rich.restate(d)
        b, _ = _rich.closed(d)
        assert len(a) == len(b) and (a == b).all(), name


def test_streams_decode(cases):
    for name, d in cases.items():
        rc, s = _rich.deflate_r(d)
        if rc == 0:
            assert zlib.decompress(s, -15) == d, name
        else:
            assert rc == 1, name                      # Compression_inefficient: the caller Stores the entry


def test_token_invariants(cases):
    for name, d in cases.items():
        t = _rich.tokens(d)
        pos, lens, dist, is_m = _rich.token_spans(t)
        assert int(lens.sum()) == len(d), name
        assert ((lens[is_m] >= 3) & (lens[is_m] <= 258)).all(), name
        assert ((dist[is_m] >= 1) & (dist[is_m] <= 32767)).all(), name
        assert (pos[is_m] // 8192 == (pos[is_m] + lens[is_m] - 1) // 8192).all(), name          # no token spans a sector's end
        assert (dist[is_m] <= pos[is_m]).all(), name
        raw = np.frombuffer(d, dtype=np.uint8)
        assert (t[~is_m] == raw[pos[~is_m]]).all(), name


def test_search_cap_is_reached_on_two_symbol_data():
    d = rich_cases()["two_symbol_50000"]
    _, ca = _rich.restate(d)
    _, cb = _rich.closed(d)
    assert ca > 0 and cb > 0


def test_unwritten_bytes_convention_is_observable():
    """Fill 0 and fill 0xFF give different tokens on FILL_CASE; both streams are valid Deflate."""
    a, _ = _rich.closed(FILL_CASE, 0)
    b, _ = _rich.closed(FILL_CASE, 0xFF)
    assert len(a) != len(b) or (a != b).any()
    for fill, t in ((0, a), (0xFF, b)):
        ra, _ = _rich.restate(FILL_CASE, fill)
        assert len(ra) == len(t) and (ra == t).all(), fill
        rc, s = _rich.deflate_r(FILL_CASE, t)
        assert rc == 0 and zlib.decompress(s, -15) == FILL_CASE
