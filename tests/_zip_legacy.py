"""What the GPU tests of the knobs "zip_legacy" / "unzip_legacy" share (test_gpu_zip_device_legacy.py, test_gpu_rezip_legacy.py): the knobs set for
a block and put back, and the CPU models' verdict per (data, method), computed once."""
import contextlib

import _legacy as L

NAMES = {1: "Shrink_1", 2: "Reduce_1", 3: "Reduce_2", 4: "Reduce_3", 5: "Reduce_4"}
DEFAULTS = dict(zip_legacy=0, unzip_legacy=0, batch_mib=512, reduce_group_mib=4096)


@contextlib.contextmanager
def knobs(enc, **kw):
    """knobs set for the block and put back to their defaults behind it, whatever happens (the encoder is the session's)"""
    for k, v in kw.items():
        enc.set_knob(k, v)
    try:
        yield
    finally:
        for k in kw:
            enc.set_knob(k, DEFAULTS[k])


_models = {}


def model_stream(d, method):
    """(rc, stream, running CRC register) of the CPU model's closed form for method 1 (Shrink_1) or 2 .. 5 (Reduce_1 .. _4); rc 1: not shorter than d"""
    if (d, method) not in _models:
        _models[(d, method)] = L.model_result(d, method)
    return _models[(d, method)]
