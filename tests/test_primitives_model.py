"""CPU side of the direct tests of the device-only building blocks: the LLHC vector set of tests/_primitives.py through the oracle, through
the math of the wave form (tests/hostcheck: hc_llhc_pm -- closed-form partition, package before leaf on ties, lists level by level) and
through llhc_serial; and the census of blocks in which a length limit binds, over the Deflate streams the GPU suite compares."""
import numpy as np

import _primitives as P
from _common import edge_inputs


def test_vector_set_is_what_the_gpu_test_promises():
    """At least 20 000 vectors; every family at every shape it applies to; only what the reference accepts (llhc_vectors asserts the sums
    and the numbers of used symbols); neighbours of four from different families; the families do what their names say."""
    vec = P.llhc_vectors()
    assert set(vec) == set(P.SHAPES)
    assert sum(len(f) for f, _ in vec.values()) >= 20000
    for shape, (f, names) in vec.items():
        want = set(P.FAMILIES) | ({"avoid_zeros"} if shape in P.BZ_SHAPES else set())
        assert set(names) == want, (shape, want ^ set(names))
        for g in range(0, len(names) - 3, 4):
            assert len(set(names[g:g + 4])) == 4, (shape, g, names[g:g + 4])
        n = shape[0]
        ns_seen = set((f[[x in ("straddle", "all_equal") for x in names]] > 0).sum(axis=1).tolist())
        assert set(P.boundary_ns(n)) <= ns_seen, shape
        if shape in P.BZ_SHAPES:
            assert (f[[x == "avoid_zeros" for x in names]] > 0).all()
    # ns where the merge chunk changes: 64 | 65, 128 | 129, 192 | 193, 256 | 257
    assert [ns for ns in range(3, 289) if P.chunk_items(ns) != P.chunk_items(ns - 1)] == [65, 129, 193, 257]
    for m in list(range(5, 65)) + [258, 288]:               # (258 and 288: the vectors with m = n, the longest chains of small sub-arrays)
        for fr in (False, True):
            w = P.peel_two_order(m, fr)
            assert sorted(w) == list(range(1, m + 1))
            big = [(mm, i) for mm, i in P.quicksort_splits(w) if mm > 4]
            assert [mm for mm, _ in big] == list(range(m, 4, -2)) and all(i == (mm - 2 if fr else 2) for mm, i in big), (m, fr)


def test_wave_math_equals_oracle_equals_serial():
    """For every vector: hc_llhc_pm == zo_llhc == hc_llhc (the last one up to its 15 bits), and zo_llhc accepts it.  This is the check
    zada_llhc_wave.h names."""
    exp = P.llhc_expected()                                     # (asserts rc = 0 for every vector)
    for shape, (f, names) in P.llhc_vectors().items():
        for which in ("hc_llhc_pm", "hc_llhc") if shape[1] <= 15 else ("hc_llhc_pm",):      # (llhc_serial's tables are laid out for 15 bits)
            got = P.hostcheck_lengths(f, shape[1], which)
            bad = np.where((got != exp[shape]).any(axis=1))[0]
            assert len(bad) == 0, (which, shape, int(bad[0]), names[bad[0]], f[bad[0]].tolist())
        used = f > 0
        assert ((exp[shape] > 0) == used).all() and exp[shape].max() <= shape[1]
        # a complete code wherever two symbols or more are used
        k = (np.where(used, 2.0 ** -exp[shape].astype(np.float64), 0.0)).sum(axis=1)
        assert (k[used.sum(axis=1) >= 2] == 1.0).all(), shape
    # the limit binds in the set, by one level, by two and by many
    f, names = P.llhc_vectors()[(288, 15)]
    depth = [P.huffman_depth(f[v]) for v in range(len(names)) if names[v] == "fib_pow2"]
    assert {17, 18}.issubset(depth) and max(depth) >= 23


def test_census_of_blocks_in_which_a_limit_binds(capsys):
    """Over the Deflate streams the GPU suite compares byte for byte (edge_inputs (), methods 8 to 10): the dynamic blocks of the ORACLE's
    stream, their headers read back, and for each of the three code sets the blocks in which Length_Limited_Coding's limit binds -- the
    longest code has max_bits and a Huffman code without a limit would be longer.  Printed; the table is DESIGN.md's ("Length-limited
    Huffman").  Asserted: the reader and the counts belong together (dynamic_blocks checks every code set of every block against zo_llhc),
    the table in DESIGN.md is this one, and in skew_litlen and skew_dist the limit binds on the literal / length code and on the distance
    code: through them a bound 15-bit code of either kind is part of every stream comparison of the GPU suite."""
    res = P.census(edge_inputs())
    tot = {s: 0 for s, _ in P.CENSUS_SETS}
    nblk = 0
    lines = []
    for name in sorted(res):
        for m, (nb, c) in sorted(res[name].items()):
            nblk += nb
            for s in tot:
                tot[s] += c[s]
            if any(c.values()):
                lines.append("%-18s %6d %8d %8d %8d %8d" % (name, m, nb, c["litlen"], c["dist"], c["clen"]))
    lines.append("%-18s %6s %8d %8d %8d %8d" % ("all %d inputs" % len(res), "8-10", nblk, tot["litlen"], tot["dist"], tot["clen"]))
    with capsys.disabled():
        print("\n%-18s %6s %8s %8s %8s %8s" % ("input", "method", "dynamic", "litlen15", "dist15", "clen7"))
        print("\n".join(lines))
    assert nblk >= 200
    # the two inputs built for it (tests/_common.py, _skewed_like): the limit binds for the code set each was made for, with every method
    for m in (8, 9, 10):
        assert res["skew_litlen"][m][1]["litlen"] > 0, (m, res["skew_litlen"][m])
        assert res["skew_dist"][m][1]["dist"] > 0, (m, res["skew_dist"][m])
    import os
    from _common import ROOT
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for ln in lines:
        assert "  " + ln + "\n" in design, "DESIGN.md's census is not the one the suite's inputs give:\n" + ln
