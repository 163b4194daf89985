"""Trained_Compression without a GPU: the premise on the reference's own data files (the stub and the stream of trainer & data have at least `skip`
bytes in common, liblzma decodes stub [: skip] + message, training pays), and the decoder's fork -- zip-ada_amd/csrc/zada_unlzma_logic.h compiled for
the CPU with one lane (tests/trained/trained_host.cpp): a decoder stopped at a symbol boundary and started again from the state it left, on fresh
buffers, gives what one uninterrupted decoder gives (bytes, input count, verdict), and what liblzma gives; the same checker once more as a program
of its own under AddressSanitizer + UBSan."""
import subprocess

import numpy as np
import pytest

import _trained
from _common import silesia_mix
from _lzmah import oracle_lzma_encode
from _trained import E_DATA, FORK_MARGIN, MARGIN, liblzma_verdict, model_decode, tc_stream

END_MARKER = 1


@pytest.fixture(scope="module")
def cases():
    return _trained.fixture_cases()


def test_premise_on_the_fixtures(cases):
    assert len(cases) == 8
    for label, trainer, data, stub, skip, whole in cases:
        assert skip == len(stub) - MARGIN > 0, label
        common = _trained.common_prefix(stub, whole)
        assert common >= skip, (label, common, skip)
        glued = stub[:skip] + whole[skip:]
        assert glued == whole
        assert liblzma_verdict(glued, len(trainer) + len(data)) == ("accepted", trainer + data, len(glued)), label
        trained = len(whole) - skip
        untrained = len(oracle_lzma_encode(data, 3, 3, 0, 2, end_marker=True, dictionary_size=_trained.DICT)[0])
        print("%-28s stub %6d common %6d trained %6d untrained %6d" % (label, len(stub), common, trained, untrained))
        assert trained < untrained, label


def _same(stream, cap, **stop):
    """The forked decoder against the uninterrupted one -> (the record, the fork)."""
    whole, _ = model_decode(stream, cap)
    forked, fork = model_decode(stream, cap, **stop)
    assert forked == whole, (stop, forked[0], whole[0], forked[2:], whole[2:])
    return whole, fork


def test_fork_on_the_fixtures(cases):
    for label, trainer, data, stub, skip, whole in cases:
        cap = len(trainer) + len(data)
        rec, fork = _same(whole, cap, in_limit=skip)
        assert rec[:3] == (0, trainer + data, len(whole)) and rec[6] == END_MARKER, label
        assert fork is not None and 0 <= skip - fork[0] < FORK_MARGIN and 0 < fork[1] <= len(trainer), (label, fork, skip)
        assert liblzma_verdict(whole, cap) == ("accepted", rec[1], rec[2]), label
        # one byte less of room, and a message cut short: the same refusal either way
        short, _ = _same(whole, cap - 1, in_limit=skip)
        assert short[0] == E_DATA and short[3] == "output beyond cap", label
        cut, _ = _same(whole[:-7], cap, in_limit=skip)
        assert cut[0] == E_DATA and cut[3] == "input exhausted before the end of the stream", label


def test_every_boundary_of_a_small_stream():
    data = bytes(silesia_mix(3000, class_mask=1))
    stream = tc_stream(data)
    whole, _ = model_decode(stream, len(data))
    assert whole[:3] == (0, data, len(stream))
    # by symbols: every boundary there is, the one in front of the marker included; beyond the last one the decoder never stops
    forks = []
    k = 0
    while True:
        _, fork = _same(stream, len(data), symbols=k)
        if fork is None:
            break
        forks.append(fork)
        k += 1
    assert forks[0] == (10, 0) and forks[-1][1] == len(data) and len(forks) > 500       # (header and the range coder's five bytes; in front of the marker)
    assert all(a[0] <= b[0] and a[1] < b[1] for a, b in zip(forks, forks[1:]))
    # by input bytes: every limit, and the boundary taken is the first from which fewer than 64 bytes remain
    for limit in range(0, len(stream) + 2 * FORK_MARGIN):
        _, fork = _same(stream, len(data), in_limit=limit)
        want = next((f for f in forks if f[0] + FORK_MARGIN > limit), None) if limit >= 10 else None
        assert fork == want, (limit, fork, want)
    # no symbol takes 64 bytes: the boundary taken never lies beyond the limit
    assert max(b[0] - a[0] for a, b in zip(forks, forks[1:])) < FORK_MARGIN


def test_damaged_messages_fork_and_liblzma():
    dmg = _trained.damaged_messages()
    assert len(dmg) == 2000
    accepted, refused, skipped = 0, 0, 0
    for k, (head, msg, cap, kind) in enumerate(dmg):
        stream = head + msg
        rec, fork = _same(stream, cap, in_limit=len(head))
        assert fork is not None and fork[0] <= len(head), k
        v = liblzma_verdict(stream, cap)
        if v[0] == "accepted":
            accepted += 1
            assert (rec[0], rec[1], rec[2]) == (0, v[1], v[2]), (k, kind, rec[3])
        else:
            refused += 1
            assert rec[0] == E_DATA and rec[1:3] == (b"", 0), (k, kind, v[0], rec[3:])
    print("damaged messages: %d accepted by liblzma, %d refused, %d left out of the comparison" % (accepted, refused, skipped))
    assert skipped == 0 and refused > 1500 and accepted + refused == 2000


def test_streams_without_a_boundary():
    """A stub part below ten bytes holds no symbol boundary (the header and the range coder's five bytes reach beyond it): no fork, as
    zada_trained_open_decoder has it; an empty text is a stream of its own."""
    empty = tc_stream(b"")
    rec, _ = model_decode(empty, 0)
    assert rec[:3] == (0, b"", len(empty)) and rec[6] == END_MARKER
    data = bytes(silesia_mix(300, class_mask=1))
    stream = tc_stream(data)
    for limit in range(0, 10):
        _, fork = _same(stream, len(data), in_limit=limit)
        assert fork is None
    assert _same(stream, len(data), in_limit=10)[1] == (10, 0)
    for n in (0, 3, 5, 9):
        rec, _ = _same(stream[:n], len(data), in_limit=n)
        assert rec[0] == E_DATA and rec[3] == "input exhausted before the end of the stream"
    bad = bytes([225]) + stream[1:]
    assert _same(bad, len(data), in_limit=40)[0][3] == "incorrect LZMA properties"


def test_checker_under_the_sanitizers(cases, tmp_path):
    """tests/trained/trained_host.cpp as a program with its own main, built with -fsanitize=address,undefined, over the fixture streams (every 997th
    limit and symbol), a small stream at every boundary, and a damaged one: a child process, nothing sanitized is loaded into python."""
    prog = _trained.build_check()
    small = bytes(silesia_mix(1200, class_mask=1))
    jobs = [(label, whole, len(trainer) + len(data), 997) for label, trainer, data, stub, skip, whole in cases]
    jobs.append(("small", tc_stream(small), len(small), 1))
    hurt = bytearray(tc_stream(small))
    hurt[len(hurt) // 2] ^= 0x40
    jobs.append(("damaged", bytes(hurt), len(small), 1))
    jobs.append(("short", tc_stream(small), len(small) - 1, 7))
    for k, (label, stream, cap, step) in enumerate(jobs):
        f = tmp_path / ("s%d.bin" % k)
        f.write_bytes(stream)
        r = subprocess.run([prog, str(f), str(cap), str(step)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "trained_check ok" in r.stdout, (label, r.stdout[-500:], r.stderr[-3000:])
        if label not in ("damaged", "short"):
            assert " rc 0 out_len %d " % cap in r.stdout, (label, r.stdout)
