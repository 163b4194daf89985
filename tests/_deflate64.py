"""A Deflate64 (Zip method 9) writer with dynamic blocks, for the tests of the parallel Inflate on that format: nothing else here writes one, and
the fixed-block writer of test_inflate_model.py makes streams whose every block the finder cannot see.  Greedy matches (one candidate per four-byte
key, window 65 536, lengths up to 65 538), Huffman lengths by heapq with the frequencies halved until the limit holds, every block sent with
HLIT = 29, HDIST = 31, HCLEN = 15 and plain code lengths (no 16 / 17 / 18).  Also the inputs and the damaged cases the CPU and GPU tests share."""
import heapq

import numpy as np

WINDOW, MAX_LEN = 65536, 65538
_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227]
_LEXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5]
_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
_cache = {}


def _dist_base(c):
    return c + 1 if c < 4 else 1 + ((2 + (c & 1)) << ((c >> 1) - 1))


def length_code(ln):
    """-> (symbol, extra value, extra bits): 258 is code 284's last value here, 285 has base 3 and 16 extra bits"""
    if ln <= 258:
        c = max(i for i in range(28) if _LBASE[i] <= ln)
        return 257 + c, ln - _LBASE[c], _LEXTRA[c]
    return 285, ln - 3, 16


def dist_code(d):
    c = d - 1 if d <= 4 else max(c for c in range(4, 32) if _dist_base(c) <= d)
    return c, d - _dist_base(c), 0 if c < 4 else (c >> 1) - 1


_LCODE = [None] * 3 + [length_code(n) for n in range(3, 259)]


def tokenize(data):
    """The greedy matcher: ints (literals) and (length, distance) pairs."""
    n, p, out, last = len(data), 0, [], {}
    while p < n:
        key = data[p:p + 4]
        c = last.get(key, -1)
        ln = 0
        if len(key) == 4 and c >= 0 and p - c <= WINDOW:
            ln, top = 4, min(MAX_LEN, n - p)
            while ln + 64 <= top and data[p + ln:p + ln + 64] == data[c + ln:c + ln + 64]:
                ln += 64
            while ln < top and data[p + ln] == data[c + ln]:
                ln += 1
        last[key] = p                                  # (token starts only: the positions inside a match are not candidates)
        if ln:
            out.append((ln, p - c))
            p += ln
        else:
            out.append(data[p])
            p += 1
    return out


def expand(tokens, out=None):
    out = bytearray() if out is None else out
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            ln, d = t
            assert 3 <= ln <= MAX_LEN and 1 <= d <= min(WINDOW, len(out)), t
            if d >= ln:
                out += out[len(out) - d:len(out) - d + ln]
            else:
                piece = bytes(out[-d:])
                out += (piece * (ln // d + 1))[:ln]
    return out


def huffman_lengths(freq, limit):
    """Code lengths of a complete prefix code over the symbols with a count; a dummy count on the first symbols when fewer than two have one."""
    freq = list(freq)
    for s in range(len(freq)):
        if sum(1 for f in freq if f) >= 2:
            break
        if not freq[s]:
            freq[s] = 1
    while True:
        heap = [(f, s, (s,)) for s, f in enumerate(freq) if f]
        heapq.heapify(heap)
        lens = [0] * len(freq)
        while len(heap) > 1:
            fa, sa, a = heapq.heappop(heap)
            fb, sb, b = heapq.heappop(heap)
            for s in a + b:
                lens[s] += 1
            heapq.heappush(heap, (fa + fb, min(sa, sb), a + b))
        if max(lens) <= limit:
            return lens
        freq = [(f + 1) // 2 if f else 0 for f in freq]


def canonical(lens):
    """symbol -> code as its bits in the order they are sent (most significant first), as an int to put least significant first"""
    code, codes = 0, [0] * len(lens)
    for ln in range(1, max(lens) + 1):
        for s, l in enumerate(lens):
            if l == ln:
                codes[s] = int(format(code, "0%db" % ln)[::-1], 2)
                code += 1
        code <<= 1
    return codes


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, k):
        self.acc |= v << self.n
        self.n += k

    def done(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def deflate64_blocks(blocks, info=None):
    """blocks: token lists, one dynamic block each, the last one final -> the stream.  info (a dict) gets block_bits: the bit every block starts at,
    and the stream's length in bits behind them; block_out: the output position every block starts at, and the whole length behind them."""
    w = _Bits()
    bits, outs, made = [], [], 0
    for bi, tokens in enumerate(blocks):
        bits.append(w.n)
        outs.append(made)
        lf, df = [0] * 286, [0] * 32
        lf[256] = 1
        for t in tokens:
            if isinstance(t, int):
                lf[t] += 1
            else:
                lf[(_LCODE[t[0]] if t[0] <= 258 else length_code(t[0]))[0]] += 1
                df[dist_code(t[1])[0]] += 1
        ll, dl = huffman_lengths(lf, 15), huffman_lengths(df, 15)
        cf = [0] * 19
        for l in ll + dl:
            cf[l] += 1
        cl = huffman_lengths(cf, 7)
        lc, dc, cc = canonical(ll), canonical(dl), canonical(cl)
        # the block in an accumulator of its own, appended at once (the whole stream's shifted per code would be quadratic)
        b = _Bits()
        b.put(1 if bi == len(blocks) - 1 else 0, 1)
        b.put(2, 2)
        b.put(29, 5)
        b.put(31, 5)
        b.put(15, 4)
        for s in _CL_ORDER:
            b.put(cl[s], 3)
        for l in ll + dl:
            b.put(cc[l], cl[l])
        for t in tokens:
            if isinstance(t, int):
                b.put(lc[t], ll[t])
                made += 1
            else:
                s, ev, eb = _LCODE[t[0]] if t[0] <= 258 else length_code(t[0])
                b.put(lc[s], ll[s])
                b.put(ev, eb)
                c, ev, eb = dist_code(t[1])
                b.put(dc[c], dl[c])
                b.put(ev, eb)
                made += t[0]
        b.put(lc[256], ll[256])
        w.put(b.acc, b.n)
    if info is not None:
        info["block_bits"], info["block_out"] = bits + [w.n], outs + [made]
    return w.done()


def deflate64(data, per_block, info=None):
    """data -> a Deflate64 stream with a new dynamic block every per_block tokens"""
    t = tokenize(data)
    return deflate64_blocks([t[i:i + per_block] for i in range(0, max(len(t), 1), per_block)], info)


def token_stats(tokens):
    """-> (matches beyond 32 768, matches longer than 258, matches with distance code 30 or 31)"""
    m = [t for t in tokens if not isinstance(t, int)]
    return sum(1 for t in m if t[1] > 32768), sum(1 for t in m if t[0] > 258), sum(1 for t in m if dist_code(t[1])[0] >= 30)


PER_BLOCK = {"period_49152": 3000, "period_65000": 1500}


def _periodic(seed, letters, rnd):
    r = np.random.RandomState(seed)
    return (bytes(r.randint(97, 113, letters).astype(np.uint8)) + bytes(r.randint(0, 256, rnd).astype(np.uint8))) * 8


def streams():
    """name -> (data, Deflate64 stream, token list, info of deflate64_blocks).
      period_49152: 40 000 bytes of a 16-letter alphabet and 9 152 random bytes, eight times: distances beyond Deflate's window in every later chunk.
      period_65000: 5 000 such letters and 60 000 random bytes, eight times: single tokens of about 60 000 bytes from 65 000 back.
      far_first / near_first: by token lists; block 3 begins at output 65 536 with marker offset 65 535 and a maximal token that runs from markers
        into its own chunk (far), or with offset 0 and a run of 65 538 copies of one marker (near)."""
    if "s" not in _cache:
        d = {}
        for name, data in (("period_49152", _periodic(5, 40000, 9152)), ("period_65000", _periodic(7, 5000, 60000))):
            t, info = tokenize(data), {}
            s = deflate64_blocks([t[i:i + PER_BLOCK[name]] for i in range(0, len(t), PER_BLOCK[name])], info)
            d[name] = (data, s, t, info)
        r = np.random.RandomState(11)
        lits = lambda n: [int(x) for x in r.randint(0, 256, n)]
        b12 = [lits(30000), lits(35536)]
        for name, b3 in (("far_first", [(3, 65536), (65538, 65536), (9, 49153), (65538, 1), (300, 65536)]),
                         ("near_first", [(65538, 1), (3, 65536), (258, 32769), (259, 32768)])):
            blocks = b12 + [b3, [(1000, 65536)] + lits(5000), [(4000, 40000)] + lits(3000)]
            info = {}
            s = deflate64_blocks(blocks, info)
            t = [x for b in blocks for x in b]
            d[name] = (bytes(expand(t)), s, t, info)
        _cache["s"] = d
    return _cache["s"]


def gpu_damaged_picks():
    """The 60 damaged cases of near_first the GPU test runs: every eighth or so, all four kinds -> (index into damaged_cases, stream, cap)"""
    mine = [(k, c) for k, c in enumerate(damaged_cases()) if c[0] == "near_first"]
    assert len(mine) == 500
    picked = [mine[8 * i + i % 4] for i in range(60)]
    assert {k % 4 for k, _ in picked} == {0, 1, 2, 3}
    return [(k, c[1], c[2]) for k, c in picked]


def damaged_cases():
    """The four kinds of damage of _inflate.damaged_corpus on the four streams: 2 000 (name, stream, cap), deterministic.  Kind 0: a bit among the
    first 200 bytes; 1, 2: a bit anywhere; 3: cut short."""
    if "d" not in _cache:
        bases = [(k, v[1], len(v[0])) for k, v in streams().items()]
        rng = np.random.default_rng(1)
        cases = []
        for k in range(2000):
            name, s, cap = bases[(k // 4) % 4]
            kind = k % 4
            if kind == 3:
                cases.append((name, s[:int(rng.integers(0, len(s)))], cap))
                continue
            pos = int(rng.integers(0, min(len(s), 200))) if kind == 0 else int(rng.integers(0, len(s)))
            b = bytearray(s)
            b[pos] ^= 1 << int(rng.integers(0, 8))
            cases.append((name, bytes(b), cap))
        _cache["d"] = cases
    return _cache["d"]
