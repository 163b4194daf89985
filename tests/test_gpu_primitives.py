"""The three device-only building blocks on chosen inputs, through the test hooks of the C ABI (zip-ada_amd/csrc/zada_testhooks.hip):
llhc_wave <max_bits> against the oracle's Length_Limited_Coding, radix_sort_pairs against numpy's stable order, exclusive_scan_u32 against
cumsum.  The streams of the other GPU tests reach this code only at the shapes their data happens to produce; a wrong permutation on a tie
or an offset wrong by one at a boundary gives a different but valid stream, which no round trip sees."""
import numpy as np
import pytest

import _primitives as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("waves_per_group", [1, 4])
@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "n%d_b%d" % s)
def test_llhc_wave_equals_oracle(encoder, shape, waves_per_group):
    """Every vector of the set (tests/_primitives.py: more than 20 000 over the twelve shapes; tests/test_primitives_model.py holds what the
    set contains): the lengths of llhc_wave equal zo_llhc's.  With four waves per workgroup the neighbours in a workgroup come from
    different families; between 1 and 4 the vectors swap between counts read from LDS and from global memory."""
    f, names = P.llhc_vectors()[shape]
    want = P.llhc_expected()[shape]
    got = P.gpu_llhc(encoder, f, shape[1], waves_per_group)
    bad = np.where((got != want).any(axis=1))[0]
    assert len(bad) == 0, "%d of %d vectors differ; first: #%d (%s) freq=%s got=%s want=%s" % (
        len(bad), len(f), bad[0], names[bad[0]], f[bad[0]].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist())


def _sort_cases(encoder, n, ranges):
    for begin, end in ranges:
        for si, kind in enumerate(P.SORT_KEYSETS):
            keys = P.sort_keys(kind, n, begin, end, seed=si)
            p = P.sort_expected(keys, begin, end)
            for vb in (4, 16):
                vals = P.sort_values(n, vb)
                for in_place in (False, True):
                    ko, vo = P.gpu_sort(encoder, keys, vals, begin, end, in_place)       # (out of place: the hook fails if the inputs changed)
                    what = (n, begin, end, kind, vb, in_place)
                    assert np.array_equal(ko, keys[p]), what
                    assert np.array_equal(vo, vals[p]), what


@pytest.mark.parametrize("n", P.SORT_NS)
def test_radix_sort_equals_stable_argsort(encoder, n):
    """Keys (all 32 bits of them) and values come out in numpy's stable order by the bits [begin, end): around the tile of 4 096, digit
    widths 1 to 9 over one to four passes (odd pass counts in place go through the alternate buffer), no bits at all (the copy), values of 4
    and 16 bytes, in place and not; key sets with a whole tile of one digit, ties in the sorted bits told apart by the other bits and by
    values that name their index."""
    _sort_cases(encoder, n, P.SORT_RANGES)


@pytest.mark.parametrize("bits", P.SORT_BIG_RANGES, ids=lambda r: "%d_%d" % r)
def test_radix_sort_at_a_million(encoder, bits):
    """245 tiles, the scan over [digit][tile] beyond one scan block: the three bit ranges the product sorts by."""
    _sort_cases(encoder, P.SORT_BIG, (bits,))


@pytest.mark.parametrize("n", P.SCAN_NS)
def test_exclusive_scan_equals_cumsum(encoder, n):
    """Blocks of 1 024 and, from 1 048 577 on, more than 1 024 of them (the pass over the block sums then loops with a carry); in place and
    not; the total as well.  The last input wraps around 2 ** 32 nowhere but puts everything behind the last place."""
    for kind in P.SCAN_INPUTS:
        a = P.scan_input(kind, n)
        want, total = P.scan_expected(a)
        for in_place in (False, True):
            out, tot = P.gpu_scan(encoder, a, in_place)
            assert np.array_equal(out, want), (n, kind, in_place, int(np.argmax(out != want)))
            assert tot == total, (n, kind, in_place, tot, total)
