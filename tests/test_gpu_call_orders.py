"""Every ordered pair of entry points on one context.

tests/conftest.py hands the GPU suite one session-wide Encoder whose state objects are made on first use and only grow, and every family's own test
file runs after hundreds of larger calls.  Here the nodes of tests/_orders.py -- one small call per kind of entry point, refused and stopped calls
among them, each with the result its CPU reference gives -- run

  * after one another so that every ordered pair (A, B), (A, A) included, is a pair of neighbours once, cut into segments of about 150 calls, each
    on a context made for it: a call that books too little, reads what the call before left behind, or trusts a flag or a record that call set,
    differs from its reference in the segment that holds the pair;
  * each alone on a context that has booked nothing;
  * on two contexts alive at once, one walking the list upwards and one downwards in turn: state that lives in the process, not in the context.

One context (two in the last test) is open at a time, closed in `finally`, as in test_gpu_fresh_context.py."""
import pytest

import _orders
from _common import product
from test_gpu_fresh_context import _differs

pytestmark = pytest.mark.gpu

K = len(_orders.COVERS)
SEGMENTS = _orders.segments(_orders.sequence(K))


@pytest.fixture(scope="module")
def nodes():
    return _orders.nodes()


def _check(node, enc, before):
    name, run, want = node
    got = run(enc)
    assert _differs(got, want) is None, "%s differs in %s (%s); the call before was %s" % (name, _differs(got, want), _orders.differs(got, want), before)
    return name


@pytest.mark.parametrize("which", range(len(SEGMENTS)))
def test_every_ordered_pair(nodes, which):
    enc = product().Encoder(0)
    try:
        before = "nothing"
        for i in SEGMENTS[which]:
            before = _check(nodes[i], enc, before)
    finally:
        enc.close()


def test_each_node_alone_on_a_fresh_context(nodes):
    for node in nodes:
        enc = product().Encoder(0)
        try:
            _check(node, enc, "nothing")
        finally:
            enc.close()


def test_two_contexts_alive_at_once(nodes):
    """X walks the list upwards, Y downwards, call by call in turn: what a call of one context leaves in the process (function-local statics, once
    flags, kernel attributes guarded per context) is met by the other context's next call."""
    x = y = None
    try:
        x, y = product().Encoder(0), product().Encoder(0)
        bx = by = "nothing"
        for up, down in zip(nodes, reversed(nodes)):
            bx = _check(up, x, "%s on this context, %s on the other" % (bx, by))
            by = _check(down, y, "%s on this context, %s on the other" % (by, bx))
    finally:
        for enc in (x, y):
            if enc is not None:
                enc.close()
