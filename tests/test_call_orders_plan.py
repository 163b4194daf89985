"""The plan of the call-order tests (tests/_orders.py, tests/test_gpu_call_orders.py), checked without a GPU: the sequence holds every ordered pair,
the segments lose none, every public entry point -- of the Python classes by introspection, of the C ABI by include/zada.h -- has a node or a
reason to have none, and every node's expected result is computable from the CPU references alone (building the list is this test's work, so the
models run on the nodes' shapes before any GPU does)."""
import inspect
import os
import re

import _orders
from _common import ROOT, product

CLASSES = ("Encoder", "ZipCreate", "UnZip", "ReZip", "CompZip", "FindZip", "TrainedCompression")


def test_the_sequence_holds_every_ordered_pair_once():
    for k in (1, 2, 3, 7, len(_orders.COVERS)):
        seq = _orders.sequence(k)
        assert len(seq) == k * k + 1 and seq[0] == seq[-1] == 0
        pairs = list(zip(seq, seq[1:]))
        assert len(set(pairs)) == len(pairs) == k * k and set(pairs) == {(a, b) for a in range(k) for b in range(k)}


def test_the_segments_lose_no_pair():
    for k, size in ((1, 150), (3, 4), (7, 10), (len(_orders.COVERS), _orders.SEGMENT)):
        seq = _orders.sequence(k)
        segs = _orders.segments(seq, size)
        assert all(2 <= len(s) <= size for s in segs)
        assert all(a[-1] == b[0] for a, b in zip(segs, segs[1:]))
        pairs = [p for s in segs for p in zip(s, s[1:])]
        assert pairs == list(zip(seq, seq[1:]))


def _python_surface():
    za = product()
    out = set()
    for cls in CLASSES:
        for name, member in vars(getattr(za, cls)).items():
            if not name.startswith("_") and (inspect.isfunction(member) or isinstance(member, (staticmethod, classmethod))):
                out.add("%s.%s" % (cls, name))
    return out


def _c_surface():
    with open(os.path.join(ROOT, "include", "zada.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return set(re.findall(r"\b(zada_[a-z0-9_]+)\s*\(", text))


def test_every_entry_point_has_a_node_or_a_reason():
    """A new public method or a new zada_* function fails here until a node of tests/_orders.py reaches it (COVERS) or EXEMPT says why none does."""
    surface = _python_surface() | _c_surface()
    assert len(_python_surface()) > 100 and len(_c_surface()) > 90
    covered = {p for reached in _orders.COVERS.values() for p in reached}
    assert all(reached for reached in _orders.COVERS.values())
    missing = sorted(surface - covered - set(_orders.EXEMPT))
    assert not missing, "entry points without a node in tests/_orders.py and without a reason in EXEMPT: %s" % ", ".join(missing)
    stale = sorted((covered | set(_orders.EXEMPT)) - surface)
    assert not stale, "COVERS / EXEMPT name what is no entry point (any more): %s" % ", ".join(stale)
    both = sorted(covered & set(_orders.EXEMPT))
    assert not both, "both covered and exempt: %s" % ", ".join(both)


HOOKS = {"Encoder.lz77_tokens", "zada_lz77_tokens", "Encoder.lzma_match_sets", "zada_lzma_match_sets", "zada_bz2_run", "zada_bz2_fetch", "zada_test_llhc",
         "zada_test_radix_sort", "zada_test_scan"}
NOTHING_LAUNCHED = ("getter", "launches nothing", "a dtype", "a bound", "ends the context", "makes the context", "frees a handle")


def test_only_what_launches_nothing_is_exempt():
    """Every reason is one line.  The test and stage hooks are exempt as hooks and the range calls for their shapes (their stages' tests run both on
    contexts of their own); every other exempt entry point is of a kind that launches no kernel: getters, knobs, bounds, dtypes, host arithmetic,
    handles and contexts made or freed."""
    ranges = {n for n in _python_surface() | _c_surface() if "range_" in n}
    for name, why in _orders.EXEMPT.items():
        assert why and "\n" not in why, name
        if name in _orders.EXEMPT_THOUGH_LAUNCHING:
            assert name in HOOKS | ranges, name
        else:
            assert any(k in why for k in NOTHING_LAUNCHED), (name, why)
    assert HOOKS | ranges == _orders.EXEMPT_THOUGH_LAUNCHING


def test_every_expected_result_is_computable_here():
    nodes = _orders.nodes()
    assert [n[0] for n in nodes] == list(_orders.COVERS) and len({n[0] for n in nodes}) == len(nodes)
    for name, run, want in nodes:
        assert callable(run) and want is not None, name
        assert _orders.differs(want, want) is None, name
    # differs names the place two results part at
    assert _orders.differs((1, [b"ab", {"k": (2, b"x")}]), (1, [b"ab", {"k": (2, b"y")}])) == "item 1 of 2: item 1 of 2: 'k': item 1 of 2: 1 bytes, 1 expected, first difference at byte 0"
