"""Deterministic inputs for the direct tests of the three device-only building blocks (tests/test_primitives_model.py on the CPU,
tests/test_gpu_primitives.py through the hooks of zip-ada_amd/csrc/zada_testhooks.hip): the LLHC frequency vectors and their lengths from
the oracle, the key sets of the radix sort, the inputs of the scan; and the reader of dynamic block headers behind the census of blocks
in which a length limit binds."""
import ctypes
import heapq

import numpy as np

from _common import hostcheck, oracle, oracle_deflate, oracle_tokens

# (n, max_bits): the six instantiations in use (k_window_descr / k_block_analyze: 288 and 32 symbols at 15 bits, 19 at 7; the BZip2
# entropy search: up to 258 symbols at 15, 16 and 17 bits) and BZip2's smallest alphabets
BZ_SHAPES = [(258, 15), (258, 16), (258, 17)] + [(k, 17) for k in range(3, 9)]
SHAPES = [(288, 15), (32, 15), (19, 7)] + BZ_SHAPES
PER_SHAPE = {288: 2400, 258: 2400, 32: 2000, 19: 2000}        # vectors per shape, filled up with the random kinds (smallest alphabets: 1 200)
SUM_LIMIT = 1 << 27                                              # the hook and the set: counts add up to less


def chunk_items(ns):
    """CH of llhc_wave: list items one lane merges."""
    return (((2 * ns - 1 + 63) >> 6) + 1) & ~1


def boundary_ns(n):
    """Every ns <= n next to an internal boundary of llhc_wave: 2 | 3, 16 | 17 (route), 64 | 65 and 128 | 129 (ballot chunks), where CH changes,
    286, 288 and the full alphabet."""
    s = {2, 3, 16, 17, 64, 65, 128, 129, 286, 288, n - 1, n}
    for ns in range(3, 289):
        if chunk_items(ns) != chunk_items(ns - 1):
            s.update((ns - 1, ns))
    return sorted(x for x in s if 2 <= x <= n)


def _place(w, n, where, rs):
    """The weights w, in their order, on n symbols: at the first, the last or the middle positions, or spread at random."""
    w = np.asarray(w, dtype=np.int64)
    k = len(w)
    assert k <= n
    f = np.zeros(n, dtype=np.int64)
    if where == "first":
        f[:k] = w
    elif where == "last":
        f[n - k:] = w
    elif where == "mid":
        f[(n - k) // 2:(n - k) // 2 + k] = w
    else:
        f[np.sort(rs.choice(n, k, replace=False))] = w
    return f


def peel_two_order(m, from_right=False):
    """Distinct weights 1 .. m in an order on which every partition of the reference's Quick_sort (pivot a (m / 2), Hoare) splits off exactly
    two elements: the two smallest at the left end (or the two largest at the right end), as long as more than four are left.  The pivot is
    the second smallest, a (0) the smallest: the scans meet after one swap, at 2; the rest is the same order for m - 2."""
    if m < 5:
        return list(range(1, m + 1))
    r = [x + (0 if from_right else 2) for x in peel_two_order(m - 2, from_right)]
    a = [0] * m
    if not from_right:
        a[0], a[m // 2] = 1, 2
        a[1] = r[m // 2 - 2]
        for k in range(2, m):
            if k != m // 2:
                a[k] = r[k - 2]
    else:
        a[m - 1], a[m // 2] = m, m - 1
        a[m - 2] = r[m // 2]
        for k in range(m - 2):
            if k != m // 2:
                a[k] = r[k]
    return a


def quicksort_splits(w):
    """The sizes (m, i) of every partition the reference's Quick_sort (huffman-encoding-length_limited_coding.adb:196-223) makes on w."""
    a, out = list(w), []

    def qs(lo, m):
        if m < 2:
            return
        p = a[lo + m // 2]
        i, j = 0, m - 1
        while True:
            while a[lo + i] < p:
                i += 1
            while p < a[lo + j]:
                j -= 1
            if i >= j:
                break
            a[lo + i], a[lo + j] = a[lo + j], a[lo + i]
            i += 1
            j -= 1
        out.append((m, i))
        qs(lo, i)
        qs(lo + i, m - i)
    qs(0, len(a))
    return out


def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def _median_mid(ns, rs):
    """Distinct weights with the median at ns / 2 and everything else at random: the first partition splits in the middle after many swaps."""
    w = rs.permutation(ns) + 1
    med = (ns // 2) + 1
    i = int(np.where(w == med)[0][0])
    w[i], w[ns // 2] = w[ns // 2], w[i]
    return w


def _random_kind(kind, n, rs):
    """The seven random kinds of tests/test_hostlogic.py::test_llhc_lane_serial_equals_oracle."""
    while True:
        if kind == 0: f = rs.randint(0, 4, n)
        elif kind == 1: f = rs.randint(0, 50, n)
        elif kind == 2: f = (rs.pareto(1.0, n) * 10).astype(np.int64)
        elif kind == 3: f = rs.randint(0, 2, n) * rs.randint(1, 100000, n)
        elif kind == 4: f = np.where(rs.rand(n) < 0.1, rs.randint(1, 5, n), 0)
        elif kind == 5: f = (2 ** rs.randint(0, 17, n)) * (rs.rand(n) < 0.5)
        else: f = rs.randint(1, 3, n)
        f = np.minimum(f, 1 << 24).astype(np.int64)
        if int(f.sum()) < SUM_LIMIT:
            return f


def _families(n, mb, rs):
    """family name -> list of count vectors for the shape (n, mb)."""
    fam = {}
    bz = (n, mb) in BZ_SHAPES
    bnd = boundary_ns(n)
    wheres = ("first", "last", "mid", "spread")

    t = [np.zeros(n, dtype=np.int64)]
    for ns in (1, 2, 3):
        for where in ("first", "last", "mid"):
            for w in ([1] * ns, [5, 1, 3][:ns], [1, 1 << 20, 7][:ns]):
                t.append(_place(w, n, where, rs))
    fam["tiny"] = t

    s = []
    for ns in bnd:
        for k in range(4):
            w = (rs.randint(1, 5, ns), rs.randint(1, 50, ns), rs.randint(1, 100000, ns), (rs.pareto(1.0, ns) * 10).astype(np.int64) % 100000 + 1)[k]
            s.append(_place(w, n, wheres[(k + ns) % 4], rs))
    fam["straddle"] = s

    fam["all_equal"] = [_place([c] * ns, n, where, rs) for ns in bnd for c, where in ((1, "first"), (1000, "spread"), (3, "last"))]

    tw = []
    for ns in bnd:
        a, b = int(rs.randint(1, 10)), int(rs.randint(10, 1000))
        h = ns // 2
        tw += [_place([a] * h + [b] * (ns - h), n, "spread", rs), _place([b] * h + [a] * (ns - h), n, "spread", rs),
               _place([a, b] * h + [a] * (ns - 2 * h), n, "spread", rs), _place(np.where(rs.rand(ns) < 0.5, a, b), n, "spread", rs),
               _place(np.where(rs.rand(ns) < 0.1, a, b), n, "spread", rs)]
    fam["two_weights"] = tw

    o = []
    for ns in bnd:
        if ns < 3:
            continue
        for step, dup in ((1, 1), (3, 2)):                            # distinct; every weight twice
            up = (np.arange(ns) // dup) * step + 1
            pipe = np.concatenate((up[::2], up[1::2][::-1]))
            o += [_place(up, n, "spread", rs), _place(up[::-1], n, "spread", rs), _place(pipe, n, "spread", rs), _place(pipe[::-1], n, "spread", rs)]
        o.append(_place(_median_mid(ns, rs), n, "spread", rs))
    fam["orders"] = o

    p = []
    for m in sorted(set(range(min(17, n), min(64, n) + 1)) | {n}):
        for fr in (False, True):
            w = np.array(peel_two_order(m, fr))
            p.append(_place(w, n, "first" if m & 1 else "last", rs))
            p.append(_place(w * 3 + 1, n, "spread", rs))
    fam["peel_two"] = p

    g = []
    for k in sorted({min(n, mb + 2), min(n, mb + 3), min(n, mb + 8), min(n, 38)}):
        f = _fib(k)
        g += [_place(f, n, "first", rs), _place(f[::-1], n, "last", rs), _place(rs.permutation(f), n, "spread", rs)]
        if k < n and sum(f) + 3 * f[-1] < SUM_LIMIT:
            g.append(_place(list(f) + [f[-1]] * min(n - k, 3), n, "spread", rs))
    for k in sorted({min(n, mb + 2), min(n, mb + 3), min(n, 26)}):
        f = [1 << i for i in range(k)]
        g += [_place(f, n, "first", rs), _place(f[::-1], n, "last", rs), _place(rs.permutation(f), n, "spread", rs)]
    fam["fib_pow2"] = g

    fam["giant"] = [_place([1] * j + [1 << 26] + [1] * (ns - 1 - j), n, where, rs) for ns in bnd for j, where in ((0, "first"), (ns // 2, "spread"), (ns - 1, "last"))]

    fam["full"] = [rs.randint(1, hi, n).astype(np.int64) for hi in (2, 3, 10, 1000, 100000) for _ in range(4)]

    if bz:
        # the counts as the BZip2 entropy search hands them over, after Avoid_Zeros (bzip2-encoding.adb:436-460): no zero; up to 100 zeros
        # are raised to 1, with more of them every count is doubled and the zeros become 1
        az = []
        for it in range(60):
            v = (rs.geometric(0.5 ** (1 + it % 6), n) - 1).astype(np.int64) * int(rs.randint(1, 2000))
            if it % 3 == 0:
                v[rs.rand(n) < 0.7] = 0
            v = np.minimum(v, 1800000 // n)
            zeroes = int((v == 0).sum())
            az.append(np.maximum(v, 1) if zeroes <= 100 else np.where(v == 0, 1, 2 * v))
        az.append(np.full(n, 2 * (900000 // n), dtype=np.int64))     # a block of 900 000 spread evenly, doubled
        one = np.ones(n, dtype=np.int64); one[0] = 2 * 899000        # ... and all but all of it on one symbol
        az.append(one)
        fam["avoid_zeros"] = az

    want = PER_SHAPE.get(n, 1200)
    have = sum(len(v) for v in fam.values())
    per = max((want - have + 6) // 7, 40)
    for kind in range(7):
        fam["random_%d" % kind] = [_random_kind(kind, n, rs) for _ in range(per)]
    return fam


FAMILIES = ("tiny", "straddle", "all_equal", "two_weights", "orders", "peel_two", "fib_pow2", "giant", "full") + tuple("random_%d" % k for k in range(7))
_cache = {}


def llhc_vectors():
    """(n, max_bits) -> (freq uint32 [count, n], family name per vector).  The families take turns, so that neighbouring vectors -- the
    four waves of a workgroup -- come from different ones."""
    if "v" not in _cache:
        out = {}
        for si, (n, mb) in enumerate(SHAPES):
            fam = _families(n, mb, np.random.RandomState(100 + si))
            rows = sorted((i, k, name) for k, name in enumerate(fam) for i in range(len(fam[name])))
            f = np.stack([fam[name][i] for i, _, name in rows])
            assert f.min() >= 0 and int(f.sum(axis=1).max()) < SUM_LIMIT and int((f > 0).sum(axis=1).max()) <= (1 << mb)
            out[(n, mb)] = (np.ascontiguousarray(f, dtype=np.uint32), [name for _, _, name in rows])
        _cache["v"] = out
    return _cache["v"]


def oracle_lengths(freq, mb):
    """zo_llhc over every row of freq: (lengths uint8 [count, n], return codes)."""
    O = oracle()
    count, n = freq.shape
    out = np.zeros((count, n), dtype=np.uint8)
    rcs = np.zeros(count, dtype=np.int64)
    f64 = freq.astype(np.uint64)
    a = np.zeros(n, dtype=np.int32)
    for v in range(count):
        rcs[v] = O.zo_llhc(f64[v].ctypes.data, n, mb, a.ctypes.data)
        out[v] = a
    return out, rcs


def llhc_expected():
    """(n, max_bits) -> the oracle's lengths for llhc_vectors (), computed once."""
    if "e" not in _cache:
        exp = {}
        for shape, (f, _) in llhc_vectors().items():
            bl, rcs = oracle_lengths(f, shape[1])
            assert (rcs == 0).all(), shape
            exp[shape] = bl
        _cache["e"] = exp
    return _cache["e"]


def hostcheck_lengths(freq, mb, which):
    """hc_llhc_pm (the wave form's math: closed-form partition, lists level by level) or hc_llhc (llhc_serial) over every row."""
    H = hostcheck()
    fn = getattr(H, which)
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    fn.restype = None
    count, n = freq.shape
    out = np.zeros((count, n), dtype=np.uint8)
    for v in range(count):
        fn(freq[v].ctypes.data, n, mb, out[v].ctypes.data)
    return out


# ---- radix sort ----
SORT_NS = (1, 2, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193)
SORT_BIG = 1000003
SORT_RANGES = ((0, 1), (0, 9), (0, 10), (0, 11), (0, 17), (0, 18), (8, 30), (0, 32), (23, 32), (5, 5))
SORT_BIG_RANGES = ((0, 11), (0, 17), (8, 30))                 # what the product sorts by: BZip2 group lists, hash-2 / hash-3 keys, hash-4 buckets
SORT_KEYSETS = ("random", "all_equal", "tile_digit", "two_digits", "sorted", "reversed", "stability")
SORT_TILE = 4096


def sort_keys(kind, n, begin, end, seed=0):
    """uint32 keys of the named set for the bit range [begin, end).  Outside the sorted bits every set but all_equal carries bits that differ
    from key to key: the full key has to travel."""
    rs = np.random.RandomState(1000 + seed)
    nb = end - begin
    mask = (1 << nb) - 1
    outside = ~np.uint32(mask << begin) if nb < 32 else np.uint32(0)
    i = np.arange(n, dtype=np.uint64)
    noise = (rs.randint(0, 1 << 32, n, dtype=np.uint64)).astype(np.uint32) & outside

    def with_bits(b):
        return ((np.asarray(b, dtype=np.uint64) & mask) << begin).astype(np.uint32) | noise
    if kind == "random":
        return rs.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    if kind == "all_equal":
        return np.full(n, 0xDEADBEEF, dtype=np.uint32)
    if kind == "tile_digit":                                                           # a whole tile of one digit, in every pass
        return with_bits(((i // SORT_TILE + 1) * 0x9E3779B1) >> 7)
    if kind == "two_digits":
        a, b = int(rs.randint(0, 1 << 32, dtype=np.uint64)) & mask, int(rs.randint(0, 1 << 32, dtype=np.uint64)) & mask
        return with_bits(np.where(i & 1, a, b))
    if kind in ("sorted", "reversed"):
        b = np.sort(rs.randint(0, 1 << 32, n, dtype=np.uint64) & mask)
        return with_bits(b if kind == "sorted" else b[::-1])
    if kind == "stability":                                                            # equal in the sorted bits (three values of them), distinct outside
        idx = (i * 2654435761 % (1 << 32)).astype(np.uint32) & outside
        return ((((i % 3) * 0x5555555) & mask) << begin).astype(np.uint32) | idx
    raise KeyError(kind)


def sort_values(n, value_bytes):
    """Values that name their index: uint32 [n] or uint32 [n, 4]."""
    i = np.arange(n, dtype=np.uint32)
    if value_bytes == 4:
        return i
    return np.ascontiguousarray(np.stack((i, ~i, i * np.uint32(7), np.full(n, 0xC0FFEE, dtype=np.uint32)), axis=1))


def sort_expected(keys, begin, end):
    """numpy's stable order by the bits [begin, end)."""
    d = (keys.astype(np.uint64) >> begin) & ((1 << (end - begin)) - 1)
    return np.argsort(d, kind="stable")


# ---- scan ----
SCAN_NS = (1, 2, 1023, 1024, 1025, 1048575, 1048576, 1048577, 3000000)
SCAN_INPUTS = ("ones", "below_16", "last")


def scan_input(kind, n):
    if kind == "ones":
        return np.ones(n, dtype=np.uint32)
    if kind == "below_16":
        return np.random.RandomState(n & 0xFFFF).randint(0, 16, n).astype(np.uint32)
    a = np.zeros(n, dtype=np.uint32)
    a[-1] = 0xFFFFFFF0
    return a


def scan_expected(a):
    c = np.cumsum(a.astype(np.uint64))
    return np.concatenate(([0], c[:-1])).astype(np.uint32), int(c[-1]) & 0xFFFFFFFF


# ---- the hooks ----
def _lib(enc):
    L = enc.lib
    vp, i32, u32, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64
    L.zada_test_llhc.argtypes = [vp, i32, i32, u32, i32, vp, vp]
    L.zada_test_radix_sort.argtypes = [vp, u64, i32, ctypes.c_uint, ctypes.c_uint, i32, vp, vp, vp, vp]
    L.zada_test_scan.argtypes = [vp, u64, i32, vp, vp, vp]
    L.zada_last_error.restype = ctypes.c_char_p
    L.zada_last_error.argtypes = [vp]
    return L


def _check(L, enc, rc, what):
    if rc != 0:
        raise RuntimeError("%s rc=%d: %s" % (what, rc, (L.zada_last_error(enc.ctx) or b"").decode()))


def gpu_llhc(enc, freq, mb, waves_per_group):
    L = _lib(enc)
    count, n = freq.shape
    bl = np.full((count, n), 0xEE, dtype=np.uint8)
    _check(L, enc, L.zada_test_llhc(enc.ctx, mb, n, count, waves_per_group, freq.ctypes.data, bl.ctypes.data), "zada_test_llhc")
    return bl


def gpu_sort(enc, keys, vals, begin, end, in_place):
    L = _lib(enc)
    ko, vo = np.full_like(keys, 0xEEEEEEEE), np.full_like(vals, 0xEEEEEEEE)
    vb = vals.dtype.itemsize * (vals.shape[1] if vals.ndim == 2 else 1)
    _check(L, enc, L.zada_test_radix_sort(enc.ctx, len(keys), vb, begin, end, int(in_place), keys.ctypes.data, vals.ctypes.data, ko.ctypes.data, vo.ctypes.data),
           "zada_test_radix_sort")
    return ko, vo


def gpu_scan(enc, a, in_place):
    L = _lib(enc)
    out = np.full_like(a, 0xEEEEEEEE)
    total = ctypes.c_uint32(0xEEEEEEEE)
    _check(L, enc, L.zada_test_scan(enc.ctx, len(a), int(in_place), a.ctypes.data, out.ctypes.data, ctypes.byref(total)), "zada_test_scan")
    return out, total.value


# ---- census: blocks of the oracle's Deflate streams in which a length limit binds ----
_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def read_dynamic_header(stream, bit):
    """The code lengths a dynamic block's header (RFC 1951, 3.2.7) declares, read from `bit` on (behind BFINAL and BTYPE): lengths of the
    literal/length code [288], of the distance code [32], of the code length code [19], how often the header uses every code length symbol
    [19], and the bit behind the header."""
    pos = [bit]

    def bits(k):
        v = 0
        for i in range(k):
            v |= ((stream[pos[0] >> 3] >> (pos[0] & 7)) & 1) << i
            pos[0] += 1
        return v
    hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
    cl = [0] * 19
    for k in range(hclen):
        cl[_CL_ORDER[k]] = bits(3)
    # canonical codes of the code length code (3.2.2), looked up by (length, code read most significant bit first)
    code, table = 0, {}
    for ln in range(1, 8):
        for s in range(19):
            if cl[s] == ln:
                table[(ln, code)] = s
                code += 1
        code <<= 1
    lens, used = [], [0] * 19
    while len(lens) < hlit + hdist:
        c, ln = 0, 0
        while (ln, c) not in table or ln == 0:
            c = (c << 1) | bits(1)
            ln += 1
            assert ln <= 7, "not a code length code"
        s = table[(ln, c)]
        used[s] += 1
        if s < 16: lens.append(s)
        elif s == 16: lens += [lens[-1]] * (3 + bits(2))
        elif s == 17: lens += [0] * (3 + bits(3))
        else: lens += [0] * (11 + bits(7))
    assert len(lens) == hlit + hdist
    return lens[:hlit] + [0] * (288 - hlit), lens[hlit:] + [0] * (32 - hdist), cl, used, pos[0]


def huffman_depth(counts):
    """The longest code of a Huffman code without a limit over the non-zero counts -- the flattest of the optimal ones (ties go to the
    shallower subtree), so that "longer than the limit" does not hang on a choice among equals."""
    h = [(int(c), 0) for c in counts if c > 0]
    if len(h) < 2:
        return len(h)
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1))
    return h[0][1]


def limit_binds(counts, lengths, max_bits):
    return max(lengths) == max_bits and huffman_depth(counts) > max_bits


def dynamic_blocks(data, method):
    """The dynamic blocks of the oracle's stream for (data, method): for each the counts and the declared lengths of its three code sets,
    [(first atom, {"litlen" | "dist" | "clen": (counts, lengths)})].  The counts are the ones Length_Limited_Coding was given: the block's
    atoms, through Tweak_for_better_RLE for the second descriptor, the distance counts patched (zip-compress-deflate.adb:340-365); the header
    is found from the bit position of the block's decision and the end-of-block code in force.  Every set is checked against the oracle's
    procedure on the way: counts and header belong together."""
    H, O = hostcheck(), oracle()
    blocks, bitpos = [], []
    rc, stream, _ = oracle_deflate(data, method, blocks=blocks, bitpos=bitpos)
    if rc != 0:
        return []
    assert len(blocks) == len(bitpos)
    tok = oracle_tokens(data, method).astype(np.int64)
    is_m = (tok & 0x80000000) != 0
    H.hc_len_symbol.restype = H.hc_dist_symbol.restype = ctypes.c_int
    lsym = np.array([0, 0, 0] + [H.hc_len_symbol(L) for L in range(3, 259)])
    dsym = np.array([0] + [H.hc_dist_symbol(D) for D in range(1, 32769)])
    ll_sym = np.where(is_m, lsym[np.where(is_m, (tok >> 16) & 0x1FF, 0)], tok & 0xFF)
    d_sym = dsym[np.where(is_m, tok & 0xFFFF, 0)]
    out = []
    eob = None                                              # length of the end-of-block code a new block has to write first
    for (first, count, choice, _), (_, pos) in zip(blocks, bitpos):
        if choice in (2, 3):
            hdr = pos + (eob or 0) + 3
            assert (stream[(hdr - 2) >> 3] >> ((hdr - 2) & 7)) & 1 == 0 and (stream[(hdr - 1) >> 3] >> ((hdr - 1) & 7)) & 1 == 1, "BTYPE is not 2"
            ll, dl, cl, used, _ = read_dynamic_header(stream, hdr)
            st = np.bincount(ll_sym[first:first + count], minlength=288).astype(np.uint32)
            st[256] = 1
            sd = np.bincount(d_sym[first:first + count][is_m[first:first + count]], minlength=32).astype(np.uint32)
            if choice == 3:
                H.hc_tweak(st.ctypes.data_as(ctypes.c_void_p), 288)
                H.hc_tweak(sd.ctypes.data_as(ctypes.c_void_p), 32)
            H.hc_patch_dist(sd.ctypes.data_as(ctypes.c_void_p))
            sets = {"litlen": (st, ll, 15), "dist": (sd, dl, 15), "clen": (np.array(used, dtype=np.uint32), cl, 7)}
            for name, (cnt, lens, mb) in sets.items():
                a = np.zeros(len(cnt), dtype=np.int32)
                c64 = cnt.astype(np.uint64)
                assert O.zo_llhc(c64.ctypes.data, len(cnt), mb, a.ctypes.data) == 0
                assert a.tolist() == list(lens), "block at atom %d: the %s counts do not give the header's lengths" % (first, name)
            out.append((first, {k: (v[0], v[1]) for k, v in sets.items()}))
            eob = ll[256]
        elif choice == 1:
            eob = 7
        elif choice == 0:
            eob = None
    return out


CENSUS_SETS = (("litlen", 15), ("dist", 15), ("clen", 7))


def census(cases, methods=(8, 9, 10)):
    """name -> method -> (dynamic blocks, {code set: blocks in which its limit binds})."""
    res = {}
    for name, d in cases.items():
        res[name] = {}
        for m in methods:
            bl = dynamic_blocks(d, m)
            res[name][m] = (len(bl), {s: sum(limit_binds(b[s][0], b[s][1], mb) for _, b in bl) for s, mb in CENSUS_SETS})
    return res
