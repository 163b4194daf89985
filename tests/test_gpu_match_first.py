"""k_match settles the first candidate of every search in its all-lanes fetch (knob "match_first"): the tokens and the
stream are the oracle's with the knob on and off, at every budget, for every method (their nice_match / chain rows differ: lz_config), on
inputs built to reach each branch of the new step -- searches that end in the fetch, compares that run past its bound, chain-length
limits (positions the fetch leaves alone), hash collisions at the head of a chain, ends of entries (la < 258, nice_match > la), segment
boundaries.  The counters #match_first_seen / #match_first_done (last_timing) say that the branch meant was taken."""
import numpy as np
import pytest

from _common import METHODS, edge_inputs, few_symbol_inputs, oracle_deflate, oracle_tokens, product, silesia_mix

gpu = pytest.mark.gpu
BUDGETS = (1, 2, 6, 0)
MAX_DIST = 32506
_cache = {}


def hash5(s):
    """hashL_of(v, 5) of zada_lz.hip: the 16-bit hash of five bytes the last level's chains are made of."""
    x = int.from_bytes(s[:4], "little")
    return ((x * 2654435761 + s[4] * 0x9E3779B1) & 0xFFFFFFFF) >> 16


def colliding_pair():
    """Two five-byte strings with the same hash that differ in the bytes the walker's filter reads (3 and 4), of bytes no text holds."""
    rs = np.random.RandomState(17)
    seen = {}
    for _ in range(100000):
        s = bytes(rs.randint(128, 256, 5).astype(np.uint8))
        o = seen.setdefault(hash5(s), s)
        if o[3:] != s[3:] and o[:4] != s[:4]:
            return o, s
    raise AssertionError("no collision found")


def near_copies(block=12288, copies=1):
    """Random bytes and copies of them, each with every 37th byte of the one before changed: every five-byte string of a copy has one earlier
    occurrence within the window, `block` bytes back, and matches are at most 36 bytes long.  (The copy of a block of 48 KiB would lie beyond
    MAX_DIST = 32 506, and no chain would be walked at all: the blocks are 12 KiB, which also keeps strangers with the same 16-bit hash rare.)"""
    rs = np.random.RandomState(23)
    parts = [rs.randint(0, 256, block).astype(np.uint8)]
    for k in range(copies):
        c = parts[-1].copy()
        c[5 + k::37] ^= 0x55
        parts.append(c)
    return np.concatenate(parts).tobytes()


def collisions_first():
    """200 KiB of text in which, time and again, a string A.. comes back after a string B.. with hash5(A) == hash5(B): B is the nearest
    member of the chain of the second A, and no match.  The tails behind A are 1 .. 30 bytes, on both sides of the fetch's compare bound."""
    a, b = colliding_pair()
    assert hash5(a) == hash5(b) and a != b
    rs = np.random.RandomState(29)
    text = silesia_mix(1 << 20, class_mask=1)
    out, off = bytearray(), 0
    while len(out) < 200 << 10:
        tail = bytes(rs.randint(128, 256, 1 + len(out) % 30).astype(np.uint8))
        for piece in (a + tail, b + bytes(rs.randint(128, 256, 7).astype(np.uint8)), a + tail):
            ln = int(rs.randint(50, 300))
            out += text[off:off + ln] + piece
            off = (off + ln) % (len(text) - 400)
    return bytes(out[:200 << 10])


def inputs():
    if not _cache:
        c = {}
        c["mix_1m"] = silesia_mix(1 << 20, offset=5 * 65536 + 12345)
        for bit in range(5):
            c["class_%d" % (1 << bit)] = silesia_mix(300 << 10, class_mask=1 << bit)
        c["near_copies"] = near_copies()
        nc = near_copies(copies=5)                    # 72 KiB: copies across the segment boundaries
        c["near_copies_32k5"] = nc[:32768 + 5]
        c["near_copies_64k3"] = nc[:65536 - 3]
        c["zeros"] = bytes(300 << 10)
        c["period_7"] = (b"abcdefg" * (300 << 10))[:300 << 10]
        e = edge_inputs()
        for per in (32505, 32506, 32507):
            c["period_%d" % per] = e["period_%d" % per]
        f = few_symbol_inputs()
        c["sym2"] = f["sym2_4m"][:512 << 10]
        c["sym4"] = f["sym4_4m"][:512 << 10]
        c["collisions"] = collisions_first()
        _cache.update(c)
    return _cache


ORDINARY = ("mix_1m", "class_1", "class_2", "class_4", "class_8", "class_16")
ENDING = ("near_copies", "near_copies_32k5", "near_copies_64k3")
LONG = ("zeros", "period_7", "period_32505", "period_32506", "period_32507")
LIMITS = ("sym2", "sym4")
CASES = [(n, m) for n in ORDINARY + ENDING + LONG + ("collisions",) for m in METHODS] + [(n, m) for n in LIMITS for m in (8, 9, 10)]


def gpu_deflate(enc, d, method):
    za = product()
    try:
        out, crc = enc.deflate(d, method)
        return 0, out, crc
    except za.CompressionInefficient:
        return 1, b"", None


def all_knobs(enc, d, method):
    """Tokens and stream == the oracle's for every budget with the knob off and on; the counters of every run with the knob on."""
    want = oracle_tokens(d, method)
    rc, ref, crc = oracle_deflate(d, method)
    counters = []
    try:
        for mf in (0, 1):
            enc.set_knob("match_first", mf)
            for budget in BUDGETS:
                enc.set_knob("budget", budget)
                got = enc.lz77_tokens(d, method)
                assert len(got) == len(want) and (got == want).all(), (mf, budget)
                t = dict(enc.last_timing())
                rc2, out, crc2 = gpu_deflate(enc, d, method)
                assert rc2 == rc and (rc != 0 or (out == ref and crc2 == crc)), (mf, budget)
                seen, done = int(t["#match_first_seen"]), int(t["#match_first_done"])
                if mf:
                    counters.append((seen, done))
                else:
                    assert (seen, done) == (0, 0)
    finally:
        enc.set_knob("match_first", 1)
        enc.set_knob("budget", -1)
    # what the fetch does with a first candidate does not depend on the budget
    assert len(set(counters)) == 1, counters
    return counters[0]


@gpu
@pytest.mark.parametrize("name,method", CASES)
def test_streams_and_tokens_with_first_candidate_in_fetch(encoder, name, method):
    d = inputs()[name]
    seen, done = all_knobs(encoder, d, method)
    print(name, method, "seen", seen, "done", done, "of", len(d))
    assert 0 <= done <= seen <= len(d)
    if method == 7:                                   # Deflate_0: literals only, no match finder
        assert seen == 0
    elif name in ORDINARY:
        assert 0 < done <= seen
    elif name == "near_copies":
        # one true candidate per chain: a search whose compare ends within the bound ends with it, unless a stranger with the same 16-bit hash
        # lies in the window too (at most 24 576 earlier positions over 65 536 buckets; test_near_copies_model has the share: 2 941 of 4 810)
        assert seen > 3000 and 2 * done >= seen
    elif name in LONG:
        # every true candidate's compare runs far beyond the bound: those positions stay on the walker's path (zeros, period 7: all of them).  What the
        # fetch does settle in the random blocks are strangers with the same 16-bit hash in front of the true candidate, and the search goes on to that one
        # (period 32 507: the true candidates lie beyond MAX_DIST, so a stranger stepped over ends its search; but few chains are walked at all -- a
        # four-byte match within the window is needed first, which only the 2 000 bytes of text in each period are likely to have)
        if name != "period_32507":
            assert 10 * done <= seen
        else:
            # the issue expects "done far below seen" here too; it cannot hold: with every true candidate out of the window, whatever is settled
            # is a stranger or a short repeat inside the text, and nothing follows it.  Few are settled, some but not all of them end there.
            # Here the model is the kernel's equal (no candidate at MAX_DIST itself, no heavy bucket, nice_match 258 out of reach for methods 9, 10).
            assert seen < len(d) // 10 and 0 < done < seen
            if method >= 9:
                assert (seen, done) == fetch_model(d)[:2]
    elif name == "collisions":
        # (that strangers are stepped over: test_collisions_input_reaches_the_branch, and the tokens above)
        assert 0 < done < seen


def fetch_model(d):
    """A few lines of Python in place of the kernel's new step (no segments, no chain-length limits): for every position with a four-byte match
    and a chain head within MAX_DIST - 1, the nearest earlier position with the same five-byte hash; compare bounded at 16 bytes; the search is
    over when the chain has no further member within the window.  Returns (settled, finished, settled ones that fail the filter at bytes 3, 4)."""
    last, prev = {}, [0] * len(d)
    for p in range(len(d) - 4):
        h = hash5(d[p:p + 5])
        prev[p] = last.get(h, -1)
        last[h] = p
    four = {}
    seen = done = stepped = 0
    for p in range(len(d) - 260):
        q4 = four.get(d[p:p + 4], -1)
        four[d[p:p + 4]] = p
        c = prev[p]
        if q4 < 0 or p - q4 > MAX_DIST - 1 or c < 0 or p - c > MAX_DIST - 1:
            continue
        ln = 0
        while ln < 17 and d[c + ln] == d[p + ln]:
            ln += 1
        if ln >= 16:
            continue                                  # the compare does not end within two turns
        seen += 1
        stepped += d[c + 3:c + 5] != d[p + 3:p + 5]
        c2 = prev[c]
        done += c2 < 0 or p - c2 > MAX_DIST - 1
    return seen, done, stepped


def test_near_copies_model():
    """The share asserted for near_copies on the GPU, from the model (no GPU needed)."""
    seen, done, _ = fetch_model(near_copies())
    assert seen > 3000 and 2 * done >= seen, (seen, done)


def test_collisions_input_reaches_the_branch():
    """The collisions input does what it was built for (no GPU needed): hundreds of searches whose first candidate is a stranger with the same
    hash that fails the filter and is stepped over, with the true occurrence behind it -- the tokens the GPU test compares depend on that step."""
    d = collisions_first()
    a, b = colliding_pair()
    spots = 0
    for p in range(len(d) - 5):
        if d[p:p + 5] == a:
            q = d.rfind(b, 0, p)
            r = d.rfind(a, 0, p)
            spots += 0 <= r < q and p - r <= MAX_DIST - 1 and hash5(d[q:q + 5]) == hash5(a) and d[q + 3:q + 5] != a[3:5]
    seen, done, stepped = fetch_model(d)
    assert spots >= 300 and stepped >= spots, (spots, seen, done, stepped)


@gpu
def test_ends_of_entries_in_a_batch(encoder):
    """Entries of 1 .. 600 bytes, entries that end 1 .. 260 bytes behind the start of a long match (la < 258 and nice_match > la in the fetch),
    and entries of more than one segment, through the batch entry point: every stream the oracle's, knob off and on, at every budget."""
    text = silesia_mix(1 << 20, class_mask=1)
    base = text[5000:5700]
    datas = [text[k * 611:k * 611 + k] for k in range(1, 601)]
    datas += [base + base[:j] for j in range(1, 261)]
    datas += [text[:32768], text[100:100 + 40000], text[:32768 + 300] + text[32768:32768 + 200], text[:65536 + 7]]
    try:
        for method in (6, 8, 9, 10):
            refs = [oracle_deflate(d, method) for d in datas]
            for mf in (0, 1):
                encoder.set_knob("match_first", mf)
                for budget in BUDGETS:
                    encoder.set_knob("budget", budget)
                    res = encoder.deflate_batch(datas, method)
                    t = dict(encoder.last_timing())
                    assert mf == 0 or 0 < t["#match_first_done"] <= t["#match_first_seen"]
                    for i, ((rc, ref, crc), (rc2, out, crc2)) in enumerate(zip(refs, res)):
                        assert rc == rc2 and crc == crc2 and (rc != 0 or out == ref), (method, mf, budget, i, len(datas[i]))
    finally:
        encoder.set_knob("match_first", 1)
        encoder.set_knob("budget", -1)


@gpu
def test_inner_budget_with_first_candidate_in_fetch(encoder):
    """Knob hygiene: the `inner` bit has moved inside the queue record; "inner_budget" 1 and 2 still change no byte."""
    d = inputs()["mix_1m"]
    rc, ref, crc = oracle_deflate(d, 10)
    want = oracle_tokens(d, 10)
    try:
        encoder.set_knob("match_first", 1)
        for inner in (1, 2):
            encoder.set_knob("inner_budget", inner)
            for budget in (6, -1):
                encoder.set_knob("budget", budget)
                got = encoder.lz77_tokens(d, 10)
                assert len(got) == len(want) and (got == want).all(), (inner, budget)
                rc2, out, crc2 = gpu_deflate(encoder, d, 10)
                assert rc == rc2 == 0 and out == ref and crc == crc2, (inner, budget)
    finally:
        encoder.set_knob("inner_budget", 0)
        encoder.set_knob("budget", -1)
