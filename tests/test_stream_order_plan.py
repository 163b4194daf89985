"""The plan of the stream-order tests (tests/_streams.py, tests/test_gpu_stream_order.py), checked without a GPU.

It keeps part (a) of test_gpu_stream_order.py honest when a method is added: every public method of the package's classes whose code takes a
data_ptr () -- found by inspect and ast, so a docstring that mentions the word does not count -- must be a key of _streams.TENSOR_METHODS, every case
the table names must have a runner, and each of these methods must synchronise torch's current stream before the first call it hands such a pointer
to (`self.enc.*` or a `*_raw` method).  A `self.enc.*` call that takes no pointer -- a bound, a dtype, the keys of a password -- launches nothing
and may stand in front of the synchronisation; whatever is between the synchronisation and the call runs on settled memory.

The checks themselves are checked on scratch copies of the source: a commented-out synchronize () line and a method missing from the table fail."""
import ast
import inspect
import textwrap

import pytest

import _streams as S
from _common import product


def _classes():
    za = product()
    return [(name, obj) for name, obj in vars(za).items() if inspect.isclass(obj) and obj.__module__ == za.__name__ and not name.startswith("_")]


def _is_data_ptr(node):
    return isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "data_ptr"


def _takes_pointer(fn_node):
    return any(_is_data_ptr(n) for n in ast.walk(fn_node))


def pointer_methods(source=None):
    """{"Class.method": its ast.FunctionDef} for the public methods whose code calls .data_ptr ().  source: the package's text instead of the
    imported package (the scratch copies below)."""
    out = {}
    if source is not None:
        for cls in ast.parse(source).body:
            if isinstance(cls, ast.ClassDef) and not cls.name.startswith("_"):
                for fn in cls.body:
                    if isinstance(fn, ast.FunctionDef) and not fn.name.startswith("_") and _takes_pointer(fn):
                        out["%s.%s" % (cls.name, fn.name)] = fn
        return out
    for cname, cls in _classes():
        for name, member in vars(cls).items():
            fn = member.__func__ if isinstance(member, (staticmethod, classmethod)) else member
            if name.startswith("_") or not inspect.isfunction(fn):
                continue
            node = ast.parse(textwrap.dedent(inspect.getsource(fn))).body[0]
            if _takes_pointer(node):
                out["%s.%s" % (cname, name)] = node
    return out


def _is_sync(node):
    """torch.cuda.current_stream (...).synchronize ()"""
    if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "synchronize"):
        return False
    inner = node.func.value
    return isinstance(inner, ast.Call) and isinstance(inner.func, ast.Attribute) and inner.func.attr == "current_stream"


def _hands_pointer_on(node):
    """a call of self.enc.* or of a *_raw method with a .data_ptr () among its arguments"""
    if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)):
        return False
    f = node.func
    to_enc = isinstance(f.value, ast.Attribute) and f.value.attr == "enc" and isinstance(f.value.value, ast.Name) and f.value.value.id == "self"
    if not (to_enc or f.attr.endswith("_raw")):
        return False
    return any(_is_data_ptr(n) for a in list(node.args) + [k.value for k in node.keywords] for n in ast.walk(a))


def unsynchronised(fn_node):
    """None, or why the method does not synchronise torch's current stream before the first call it hands a pointer to."""
    calls = sorted((n.lineno, n.col_offset) for n in ast.walk(fn_node) if _hands_pointer_on(n))
    syncs = sorted((n.lineno, n.col_offset) for n in ast.walk(fn_node) if _is_sync(n))
    if not calls:
        return "no self.enc.* / *_raw call takes its pointers"
    if not syncs:
        return "no torch.cuda.current_stream (...).synchronize ()"
    if syncs[0] >= calls[0]:
        return "the first synchronize () stands behind the first call that takes a pointer"
    return None


def test_every_pointer_taking_method_is_in_the_table():
    found = pointer_methods()
    assert len(found) >= 8, sorted(found)
    missing = sorted(set(found) - set(S.TENSOR_METHODS))
    assert not missing, "methods that take a data_ptr () and have no case in tests/_streams.py::TENSOR_METHODS: %s" % ", ".join(missing)
    za = product()
    for name in S.TENSOR_METHODS:
        cls, meth = name.split(".")
        assert callable(getattr(getattr(za, cls), meth)), name
    stale = sorted(set(S.TENSOR_METHODS) - set(found) - {"ZipInfo.load_device"})        # (load_device takes no pointer: torch operations)
    assert not stale, "TENSOR_METHODS names methods that take no data_ptr () (any more): %s" % ", ".join(stale)


def test_every_case_of_the_table_has_a_runner():
    import test_gpu_stream_order as G
    cases = S.tensor_cases()
    assert all(S.TENSOR_METHODS.values()) and len(cases) == len(set(cases))
    assert set(cases) == set(G.RUNNERS), sorted(set(cases) ^ set(G.RUNNERS))
    params = [m for m in G.test_tensor_methods_wait_for_the_current_stream.pytestmark if m.name == "parametrize"]
    assert len(params) == 1 and list(params[0].args[1]) == cases, "the GPU test iterates over the table"


def test_every_pointer_taking_method_synchronises_first():
    for name, node in pointer_methods().items():
        assert unsynchronised(node) is None, "%s: %s" % (name, unsynchronised(node))


def _package_source():
    return inspect.getsource(product())


def test_a_commented_out_synchronize_is_seen():
    """each of the package's synchronize () lines in turn, commented out in a scratch copy of the source: the check above names that method"""
    src = _package_source().split("\n")
    lines = [i for i, ln in enumerate(src) if ln.strip().startswith("torch.cuda.current_stream(") and ln.strip().endswith(".synchronize()")]
    assert len(lines) == 8, lines
    for i in lines:
        scratch = list(src)
        scratch[i] = scratch[i].replace("torch.cuda", "pass  # torch.cuda", 1)
        bad = {name for name, node in pointer_methods("\n".join(scratch)).items() if unsynchronised(node) is not None}
        assert len(bad) == 1, (i + 1, bad)
    assert not [name for name, node in pointer_methods("\n".join(src)).items() if unsynchronised(node) is not None]


def test_a_method_missing_from_the_table_is_seen(monkeypatch):
    """... and so is a method taken out of the table, or a new method that takes a pointer"""
    for name in pointer_methods():
        table = {k: v for k, v in S.TENSOR_METHODS.items() if k != name}
        monkeypatch.setattr(S, "TENSOR_METHODS", table)
        with pytest.raises(AssertionError, match=name.replace(".", r"\.")):
            test_every_pointer_taking_method_is_in_the_table()
        monkeypatch.undo()
    added = _package_source() + "\n\nclass Later:\n    def send_device(self, t):\n        return self.enc.crc32_device(t.data_ptr(), t.numel())\n"
    found = pointer_methods(added)
    assert "Later.send_device" in found and unsynchronised(found["Later.send_device"]) is not None
    assert set(found) - {"Later.send_device"} == set(pointer_methods())


def test_the_delay_is_sized_from_the_measurement():
    """at least ten times the measured host gap, at most 250 ms per case; the calibrated figure is the one the constant asks for"""
    assert 10 * S.HOST_GAP_MS <= S.DELAY_MS <= S.MAX_DELAY_MS == 250.0
    assert abs(S.CALIBRATED_MS - S.DELAY_MS) <= 0.05 * S.DELAY_MS
