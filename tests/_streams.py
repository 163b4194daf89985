"""What the stream-order tests share (test_gpu_stream_order.py, test_stream_order_plan.py): a producer that is provably still pending when the call
under test is entered, the table of the tensor-taking methods with the cases that run each of them behind such a producer, and the stale inputs.

The contract under test (include/zada.h, "Context = device + stream + workspace"): work queued on the legacy default stream before a call is ordered
before the call's accesses; work on any other stream is the caller's to finish, which the tensor-taking Python methods do for torch's current stream
by synchronising it just before their one C call; every call returns with its work complete.

pending_fill (dst, src_dev, stream) queues, on `stream`:  delay -> gate event -> dst.copy_ (src_dev) -> done event.  `dst` holds a stale content A,
the copy writes B.  The gate is recorded behind the delay and in front of the copy, so `not gate.query ()` on the host proves that no byte of B has
been written yet; a test asserts that immediately before it enters the method under test, and a gate that has fired FAILS the test (fired ()
below says so, with the advice to lengthen DELAY_MS): it neither skips nor passes."""
import math
import time

import numpy as np

# Length of the producer's delay.  Measured on one MI355X with other tenants on the machine, three rounds over every case of part (a):
#   host gap, end of pending_fill -> the synchronize () in front of the C call (in between: the gate's assertion, the method's checks, its table,
#   the bound and the output tensor): 0.04 .. 0.19 ms warm; the slowest to prepare are the writers' and ReZip's tables (write_device 0.06 .. 0.15 ms,
#   rezip_device 0.08 .. 0.11 ms); the largest figure of all, a first call in a process, 0.67 ms (TrainedCompression.encode_device; write_device 0.37 ms);
#   calibrated delay (torch.cuda._sleep, 2.40 million cycles per ms, two timing events around it on the stream): 59.97 .. 60.00 ms for DELAY_MS = 60.
# The delay is to be at least ten times the gap (host jitter on a shared machine) -- it is ninety times the largest -- and at most 250 ms per case
# (the file stays within seconds: 56 cases in 7.5 s).
HOST_GAP_MS = 0.67          # the largest gap measured
CALIBRATED_MS = 60.0        # what DELAY_MS took on the device
DELAY_MS = 60.0
MAX_DELAY_MS = 250.0
FALLBACK_BYTES = 64 << 20   # the tensor of the fallback delay: a chain of in-place elementwise operations on it

_cal = {}
last_fill_end = [0.0]       # time.perf_counter () at the end of the last pending_fill: what the host gap is measured from


def _timed(stream, queue):
    """milliseconds `queue ()` takes on `stream`, by two timing events"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        a.record(stream)
        queue()
        b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def calibrate():
    """Once per process: ("sleep", cycles per ms) for torch.cuda._sleep, or ("chain", operations per ms, the tensor) where _sleep is missing or
    calibrates to nothing.  The probes grow from well under a millisecond, so no probe runs for long whatever a cycle is."""
    import torch
    if "kind" in _cal:
        return _cal
    st = torch.cuda.current_stream()
    sleep = getattr(torch.cuda, "_sleep", None)
    if sleep is not None:
        cycles = 100000
        sleep(cycles)                                        # (first launch: the kernel is loaded)
        torch.cuda.synchronize()
        while cycles <= 10 ** 10:
            ms = _timed(st, lambda: sleep(cycles))
            if ms >= 5.0:
                _cal.update(kind="sleep", per_ms=cycles / ms)
                return _cal
            cycles *= 4 if ms < 1.0 else max(2, int(6.0 / ms) + 1)
    buf = torch.zeros(FALLBACK_BYTES // 4, dtype=torch.float32, device="cuda")
    buf.add_(1.0)
    torch.cuda.synchronize()
    ops = 64
    ms = _timed(st, lambda: [buf.add_(1.0) for _ in range(ops)])
    _cal.update(kind="chain", per_ms=ops / max(ms, 1e-3), buf=buf)
    return _cal


def queue_delay(ms=None):
    """The delay on torch's current stream."""
    import torch
    ms = min(DELAY_MS if ms is None else ms, MAX_DELAY_MS)
    c = calibrate()
    if c["kind"] == "sleep":
        torch.cuda._sleep(int(c["per_ms"] * ms))
    else:
        for _ in range(int(math.ceil(c["per_ms"] * ms))):
            c["buf"].add_(1.0)


def measured_delay_ms():
    """What the delay of DELAY_MS takes on the device, by two timing events (the calibration's check, and the figure of the summary)."""
    import torch
    calibrate()
    return _timed(torch.cuda.current_stream(), queue_delay)


def pending_fill(dst, src_dev, stream):
    """On `stream`: delay -> gate event -> dst.copy_ (src_dev, non_blocking=True) -> done event.  -> (gate, done).  dst and src_dev are settled
    device tensors of one shape (the caller's set-up has synchronised); the calibration, which synchronises, has run before the first fill."""
    import torch
    calibrate()
    gate, done = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(stream):
        queue_delay()
        gate.record(stream)
        dst.copy_(src_dev, non_blocking=True)
        done.record(stream)
    last_fill_end[0] = time.perf_counter()
    return gate, done


def fired(what):
    return ("%s: the producer's gate had fired before the method under test was entered -- the case proves nothing; lengthen DELAY_MS in "
            "tests/_streams.py (%.0f ms now, at most %.0f)" % (what, DELAY_MS, MAX_DELAY_MS))


def pending_tensor(stale, fresh, stream, a_in=0):
    """A device tensor of a_in + len (stale) bytes that holds `stale` at offset a_in now and `fresh` once the pending fill on `stream` has run.
    -> (tensor, gate, done).  The set-up -- both host-to-device copies -- is settled before the fill is queued."""
    import torch
    assert len(stale) == len(fresh), "A and B are of one length"
    n = len(stale)
    h = np.full((2, max(a_in + n, 1)), 0x3C, dtype=np.uint8)
    h[0, a_in:a_in + n] = np.frombuffer(bytes(stale), dtype=np.uint8)
    h[1, a_in:a_in + n] = np.frombuffer(bytes(fresh), dtype=np.uint8)
    with torch.cuda.stream(stream):                          # (allocated on the stream that will use it)
        dst = torch.empty(h.shape[1], dtype=torch.uint8, device="cuda")
    dst.copy_(torch.from_numpy(h[0]))
    src = torch.from_numpy(h[1]).cuda()
    torch.cuda.synchronize()
    gate, done = pending_fill(dst, src, stream)
    return dst, gate, done


def pending_entries(stale, fresh, stream):
    """One pending arena for a list of entries: -> ([tensor per entry: views of the arena, one behind the other, so at every alignment], gate, done)."""
    assert [len(a) for a in stale] == [len(b) for b in fresh]
    arena, gate, done = pending_tensor(b"".join(stale), b"".join(fresh), stream)
    views, at = [], 0
    for b in fresh:
        views.append(arena[at:at + len(b)])
        at += len(b)
    return views, gate, done


# ---- the tensor-taking methods and the cases of test_gpu_stream_order.py (a) that run each behind a pending producer ----------------------------
# "Class.method" -> the names of its cases.  tests/test_stream_order_plan.py holds that every public method of the package whose code takes a
# data_ptr () is a key here, that every case named here has a runner in test_gpu_stream_order.py, and that each of these methods synchronises
# torch's current stream before the call it hands the pointers to.  (ZipInfo.load_device takes no pointer: it goes through torch operations, which
# run on the current stream; it is here because its tensor is read.)
TENSOR_METHODS = {
    "ZipCreate.write_device": ("write_device(Store)", "write_device(Deflate_Fixed)", "write_device(Deflate_1)"),
    "ZipCreate.write_device_ex": ("write_device_ex(BZip2_1)", "write_device_ex(LZMA_1)", "write_device_ex(Deflate_1, password)", "write_device_ex(Shrink_1, legacy)"),
    "ZipInfo.load_device": ("load_device + extract_device(Store, Deflate)", "load_device + extract_device(BZip2, LZMA)"),
    "UnZip.extract_device": ("extract_device(Store, Deflate)", "extract_device(Store, Deflate, test_only)", "extract_device(BZip2, LZMA)",
                             "extract_device(BZip2, LZMA, test_only)"),
    "CompZip.compare_device": ("compare_device(second archive pending)",),
    "ReZip.rezip_device": ("rezip_device(deflate_3, bzip2_1)",),
    "FindZip.find_device": ("find_device(needle)",),
    "TrainedCompression.encode_device": ("trained encode_device + decode_device",),
    "TrainedCompression.decode_device": ("trained encode_device + decode_device",),
}


def tensor_cases():
    """the case names, each once, in the table's order"""
    out = []
    for cases in TENSOR_METHODS.values():
        out += [c for c in cases if c not in out]
    return out


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------------
def entry_lists(count=8):
    """(A, B): two lists of `count` entries of 0 .. 5 000 bytes, pairwise of one length and different wherever there is a byte: one empty, one of one
    byte, one that crosses 4 096 bytes; text and mixed content (silesia_mix) and the legacy tests' edge_input, whose matches and 144s Shrink and
    Reduce need."""
    from _common import silesia_mix
    from _legacy import edge_input
    lens = (3000, 0, 4500, 1, 777, 2048, 4097, 1500)[:count]
    text, mix = silesia_mix(40000, class_mask=1), silesia_mix(40000)
    A, B = [], []
    for k, n in enumerate(lens):
        if k % 3 == 2:
            a, b = edge_input(n, seed=50 + k), edge_input(n, seed=70 + k)
        else:
            src = text if k % 3 == 0 else mix
            a, b = src[1000 * k:1000 * k + n], src[20000 + 1000 * k:20000 + 1000 * k + n]
        if n == 1:
            a, b = b"a", b"b"
        assert len(a) == len(b) == n and (n == 0 or a != b)
        A.append(a)
        B.append(b)
    return A, B


def stale_stream(encode, target_len, cap, seed=1, avoid=None):
    """A valid stream of `encode` of exactly target_len bytes, made from exactly cap bytes of data (the readers of the oldest formats end a stream
    by its promised size): the stale content A of a decoder's input, where B is a stream of target_len bytes that holds cap bytes.  The data are
    cap - r bytes of a short repeated phrase and r random bytes; the stream's length grows by about a byte per random byte, so r is found by
    bisection and a short walk; a length that one phrase steps over is met by the next."""
    for p in range(0, 64):
        rnd = np.random.default_rng(1000 * seed + p).integers(0, 256, max(cap, 1), dtype=np.uint8).tobytes()
        phrase = (b"stale content %d, " % p) + bytes(range(65, 65 + p % 26))
        filler = phrase * (cap // len(phrase) + 1)
        data = lambda r: filler[:cap - r] + rnd[:r]
        size = lambda r: len(encode(data(r)))
        lo, hi = 0, cap
        if size(lo) > target_len or size(hi) < target_len:
            continue
        while hi - lo > 1:                                   # (nearly monotone: the walk below mends what the bisection misses)
            mid = (lo + hi) // 2
            if size(mid) < target_len:
                lo = mid
            else:
                hi = mid
        for r in range(max(0, lo - 24), min(cap, hi + 24) + 1):
            s = encode(data(r))
            if len(s) == target_len and s != avoid:
                return s
    raise AssertionError("no stale stream of %d bytes that holds %d bytes of data" % (target_len, cap))


def padded_archives(make, entries_a, entries_b):
    """Two archives of one length: make (entries, comment) -> bytes; the shorter one gets an archive comment that makes up the difference."""
    a, b = make(entries_a, b""), make(entries_b, b"")
    if len(a) < len(b):
        a = make(entries_a, b"." * (len(b) - len(a)))
    elif len(b) < len(a):
        b = make(entries_b, b"." * (len(a) - len(b)))
    assert len(a) == len(b) and a != b
    return a, b


def zipfile_archive(entries, methods, comment=b""):
    """zipfile's archive of [(name, bytes)] with one compress_type per entry (fixed date: the same bytes every time)."""
    import io
    import zipfile
    bio = io.BytesIO()
    with zipfile.ZipFile(bio, "w") as zf:
        for (nm, d), m in zip(entries, methods):
            zf.writestr(zipfile.ZipInfo(nm, (2024, 5, 6, 7, 8, 10)), d, compress_type=m)
        zf.comment = comment
    return bio.getvalue()
