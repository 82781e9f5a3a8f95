"""The kernels of canvas_wavelets (csrc/wavelets.hip) one by one, through the probe entries (canvas_wavelets_*_probe: the product's kernels with the launch sets the call uses),
against the plain restatements of tests/wavelets_ref.py on the node families of tests/wavelets_cases.py: prefix sums and medians bit for bit against integer arithmetic, the
closed form against its own error bound, the level decisions against the first arg-max of the sequential recurrences, chains and subtrees bit for bit against the recurrences,
and the inputs of the thresholds against the oracle."""
import functools
import math
import time

import numpy as np
import pytest

import oracle_lib as O
import wavelets_cases as WC
import wavelets_ref as R
from gpu_common import get_canvas, to_dev, wavelets_coverage as _coverage

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _ref(name, n, seed=0):
    """(inner products, coefficient, first arg-max) of a family node by the sequential recurrences; computed once per node"""
    ipi, mean = R.inner_products(WC.to_x(WC.family(name, n, seed)).tolist())
    ind = R.first_argmax(ipi)
    return ipi, ipi[ind - 1] / max(0.5, mean / 200.0), ind


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ------------------------------------------------------------------------------------------------------------------------------------ prefix sums
def test_prefix_sums_bit_for_bit_at_the_tile_edges():
    """k_wv_prefix_tiles / k_wv_prefix_apply over tiles of 1 024 bins: chromosome lengths on and around the tile, chromosomes of 1 and 2 bins between them, and three long ones.
    A tile with number j inside its chromosome adds up the j tiles in front of it, 1 024 per round of the carry loop (`for b0 = 0; b0 < j; b0 += 1024`): the second round, in
    which a tile's term takes the carry of the first, begins at j = 1 025.  1 024 x 1 024 + 1 bins are 1 025 tiles, the last of them j = 1 024: one full round, not yet a
    second.  1 025 x 1 024 + 1 bins (last tile j = 1 025, one bin in it) and 1 026 x 1 024 bins (last tile j = 1 025, full, the chromosome ending on the tile's edge) reach it."""
    cv = get_canvas()
    rng = np.random.RandomState(41)
    lengths = [1, 2, 1023, 1, 1024, 2, 1025, 1, 2048, 2, 2049, 1, 1024 * 1024 + 1, 2, 1025 * 1024 + 1, 1, 1026 * 1024, 2]
    assert [(n + 1023) // 1024 - 1 for n in lengths[12::2]] == [1024, 1025, 1025]              # the number j of each long chromosome's last tile
    per = []
    for n in lengths:
        big = n > 100_000                               # (the sums of the long chromosomes must stay below 2^61: small values with a few of the largest)
        k = rng.randint(0, 1000 if big else WC.KMAX + 1, n).astype(np.int64)
        k[rng.randint(0, n, max(1, n // 300 if not big else 5))] = WC.KMAX
        k[rng.randint(0, n, max(1, n // 300))] = 0
        per.append(k)
    per[2][-1] = WC.KMAX; per[4][0] = WC.KMAX; per[6][1024] = WC.KMAX
    for i in (12, 14, 16):                              # the largest value in the first tile, at both sides of the edge of tile 1 024 and in the last bin (the last but one bin 0)
        per[i][3] = WC.KMAX; per[i][1024 * 1024 - 1] = WC.KMAX; per[i][1024 * 1024] = WC.KMAX; per[i][-2] = 0; per[i][-1] = WC.KMAX
    k = np.concatenate(per)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    p1, p2, bad = cv.wavelets_prefix_probe(WC.to_x(k), off)
    e1, e2 = R.prefix_sums(k, off)
    assert bad.tolist() == [0, 0]
    assert (p1 == e1).all(), np.flatnonzero(p1 != e1)[:5]
    assert (p2 == e2).all(), np.flatnonzero(p2 != e2)[:5]
    assert int(e2.max()) < 2 ** 61 and max(int(e1[off[i + 1] - 1]) * lengths[i] for i in (12, 14, 16)) < 2 ** 61


@pytest.mark.parametrize("value,want", [(1.234, [1, 0]), (-3.5, [1, 0]), (20_000_000.00, [1, 0]), (float("nan"), [1, 1]), (float("inf"), [1, 1]), (-0.0, [0, 0]), (19_999_999.99, [0, 0])])
def test_bad_words_of_single_values(value, want):
    cv = get_canvas()
    x = WC.to_x(WC.family("poisson", 2500)); x[1300] = value
    _, _, bad = cv.wavelets_prefix_probe(x, [0, 1000, 2500])
    assert [int(bool(b)) for b in bad] == want


def test_sums_that_pass_2_61_set_the_first_bad_word_and_the_call_takes_the_chains():
    cv = get_canvas()
    flat = np.full(70_000, 19_999_999.99)
    p1, _, bad = cv.wavelets_prefix_probe(flat, [0, 70_000])
    assert bad[0] != 0 and bad[1] == 0
    assert (p1 == WC.KMAX * np.arange(1, 70_001, dtype=np.int64)).all()          # (the first sums themselves are still exact)
    # canvas_wavelets on such a coverage: every long node through the chains, the oracle's breakpoints.  (On the exactly flat chromosome every node splits off its last bin:
    # 70 000 levels, a minute for the oracle and for the device alike — the same 70 000 bins with noise in the last digits and one step pass 2^61 just the same.)
    rng = np.random.RandomState(3)
    k = WC.KMAX - rng.poisson(100, 70_000).astype(np.int64) * 100
    k[20_000:30_000] //= 2
    x = WC.to_x(k)
    assert int(R.prefix_sums(k, [0, len(k)])[1][-1]) > 2 ** 61
    bad = cv.wavelets_prefix_probe(x, [0, 70_000])[2]
    assert bad[0] != 0 and bad[1] == 0
    exp = O.wavelets_genome([x], window=1000)
    got = cv.wavelets(to_dev(x, cv.device), np.array([0, 70_000], np.int64), window=1000)
    assert got[0].tolist() == exp[0].tolist() and len(exp[0]) == 3
    assert cv.wavelets_decisions()[3] == 0


@pytest.mark.parametrize("value", [-3.5, 20_000_000.00])
def test_the_call_on_values_outside_the_integers_is_the_oracle_s(value):
    """a negative value or one at 2e7 sets bad[0]; canvas_wavelets then takes the chains (its finiteness check passes): whatever the oracle computes for them"""
    cv = get_canvas()
    x = WC.to_x(WC.family("step", 3000)); x[1700] = value
    exp = O.wavelets_genome([x], window=100)
    got = cv.wavelets(to_dev(x, cv.device), np.array([0, 3000], np.int64), window=100)
    assert got[0].tolist() == exp[0].tolist()
    assert cv.wavelets_decisions()[3] == 0


# ------------------------------------------------------------------------------------------------------------------------------------ the bound
BOUND_LENGTHS = (9, 65, 66, 2048, 2049, 2050, 4097, 6000)


def test_the_bound_covers_the_recurrences_for_every_element_of_every_node():
    """|ref[m]| 100 and |T[m]| differ by at most B[m] for every m of every node: all families at lengths around the chunk of 2 048 elements, nodes at a chromosome's first bin and
    behind other nodes (the sums in front of the node enter), in three chromosomes, and one node behind 1.2 M bins of large values (P2 close to 2^60).
    Measured on the MI355X: the largest ratio is 0.18 (headspike, n = 65); the CPU model of tests/test_wavelets_ref.py, which takes exact square roots, gives 0.094."""
    cv = get_canvas()
    per = [[], [], []]; nodes = []; names = []
    i = 0
    for name in WC.FAMILIES:
        for n in BOUND_LENGTHS:
            c = i % 3; i += 1
            nodes.append((c, sum(len(a) for a in per[c]), n)); names.append((name, n, 0))
            per[c].append(WC.family(name, n))
    tail = WC.family("poisson", 3000, 1)
    per.append([np.full(1_200_000, 1_500_000, np.int64), tail])
    nodes.append((3, 1_200_000, 3000)); names.append(("poisson", 3000, 1))
    chrom = [np.concatenate(p) for p in per]
    off = np.concatenate([[0], np.cumsum([len(a) for a in chrom])]).astype(np.int64)
    k = np.concatenate(chrom)
    p2 = R.prefix_sums(k, off)[1]
    assert 2 ** 59 < int(p2[-1]) < 2 ** 60
    arr = np.array([(off[c] + s, n, c) for c, s, n in nodes], np.int32)
    assert (arr[:, 0] > off[arr[:, 2]]).sum() > 50 and (arr[:, 0] == off[arr[:, 2]]).sum() == 3
    T, B = cv.wavelets_bound_probe(WC.to_x(k), off, arr)
    worst = (0.0, None)
    for (name, n, seed), t, b in zip(names, T, B):
        ipi = np.abs(np.array(_ref(name, n, seed)[0])) * 100.0
        d = np.abs(ipi - np.abs(t))
        assert len(t) == n - 1 and np.isfinite(t).all() and (b >= 0).all()
        assert (d[b == 0] == 0).all(), (name, n)
        ratio = float(np.max(d[b > 0] / b[b > 0])) if (b > 0).any() else 0.0
        print(f"{name} n={n}: max |ref - T| / B = {ratio:.3g}")
        worst = max(worst, (ratio, (name, n)))
        assert (d <= b).all(), (name, n, ratio)
    print("largest |ref - T| / B on the device:", worst)


# ------------------------------------------------------------------------------------------------------------------------------------ level decisions
LEVEL_LENGTHS = (65, 66, 2048, 2049, 2050, 4097, 4098)          # n - 1 = 64, 65, 2047, 2048, 2049, 4096, 4097
KEEP_KINDS = ("half", "just_below", "double", "nan")


@functools.lru_cache(maxsize=None)
def _level_case():
    """coverage, offsets, nodes (start, len, chromosome, level), per node (family, n, seed, keep kind), keepAbove per chromosome.  The family nodes and one node of
    256 x 2 048 + 2 bins (257 chunks) have a chromosome each, whose keepAbove is set relative to the node's coefficient; ~2 900 short nodes fill further chromosomes,
    50 to each with gaps between them, so that the list has more than 2 048 chunks."""
    chroms, nodes, info, keep = [], [], [], []
    j = 0
    for name in WC.FAMILIES:
        for n in LEVEL_LENGTHS:
            kind = KEEP_KINDS[j % 4] if name in WC.NON_TIE else "nan"; j += 1
            lead = (j % 3) * 5                                   # bins in front of the node inside its chromosome
            chroms.append(np.concatenate([WC.family("poisson", lead, 7) if lead else np.zeros(0, np.int64), WC.family(name, n), np.zeros(3, np.int64)]))
            nodes.append((len(chroms) - 1, lead, n, j % 3)); info.append((name, n, 0, kind))
    big = 256 * 2048 + 2
    chroms.append(WC.family("step", big)); nodes.append((len(chroms) - 1, 0, big, 0)); info.append(("step", big, 0, "double"))
    for f in range(58):
        parts = []
        at = 0
        for q in range(50):
            seed = (f * 50 + q) % 37
            name = ("poisson", "step")[q % 2]; n = 65 + (q % 3 == 0)
            parts.append(np.zeros(q % 4, np.int64)); at += q % 4
            nodes.append((len(chroms), at, n, q % 5)); info.append((name, n, seed, "nan"))
            parts.append(WC.family(name, n, seed)); at += n
        chroms.append(np.concatenate(parts + [np.zeros(8, np.int64)]))
    off = np.concatenate([[0], np.cumsum([len(a) for a in chroms])]).astype(np.int64)
    keep = np.full(len(chroms), -1.0)
    for (c, s, n, lv), (name, nn, seed, kind) in zip(nodes, info):
        cabs = abs(_ref(name, nn, seed)[1])
        if kind != "nan":
            keep[c] = {"half": 0.5 * cabs, "just_below": cabs * (1 - 1e-12), "double": 2 * cabs}[kind]
    arr = np.array([(off[c] + s, n, c, lv) for c, s, n, lv in nodes], np.int32)
    return WC.to_x(np.concatenate(chroms)), off, arr, info, keep


@pytest.mark.parametrize("wv_long", [8, 64, 256])
def test_one_level_decides_what_has_one_arg_max_and_places_the_children(wv_long):
    """The arg-max of a zeroed node (status 1) is no kernel output: the probe reconstructs it from the children the kernel appended (canvas_hip.h).  So every decided node's ind is
    first compared with the first arg-max of the recurrences, an independent value, and only then are the expected children derived from that arg-max (ref_ind, not the probe's)."""
    cv = get_canvas()
    x, off, nodes, info, keep = _level_case()
    assert len(nodes) > 2900 and int(((nodes[:, 1] - 1 + 2047) // 2048).sum()) > 2048
    out = cv.wavelets_level_probe(x, off, nodes, keep, wv_long=wv_long)
    assert out["overflow"] == 0
    want_next, want_roots = set(), set()
    for (s, n, c, lv), (name, nn, seed, kind), status, ind in zip(nodes.tolist(), info, out["status"].tolist(), out["ind"].tolist()):
        if WC.is_tie(name, nn):
            assert status == 0, (name, nn)
            continue
        if name in WC.NON_TIE:
            assert status != 0, (name, nn, seed)                  # what has one clear arg-max is decided
        if status == 0:
            continue
        _, coef, ref_ind = _ref(name, nn, seed)
        assert ind == ref_ind, (name, nn, seed, ind, ref_ind)
        if kind in ("half", "just_below", "nan"):
            assert status == 2, (name, nn, kind)                  # |coefficient| > keepAbove (or no threshold): never zeroed
        elif kind == "double":
            assert status == 1, (name, nn, kind)
        b, e, cb = s + ref_ind - 1, s + n - 1, int(off[c])
        for cs, ce in ((s, b), (b + 1, e)):
            if (cs == s and b - s >= 1) or (cs == b + 1 and e - b >= 2):
                ln = ce - cs + 1
                if ln > wv_long:
                    want_next.add((cs, ln, c, lv + 1))
                else:
                    want_roots.add((cs, ln, c, lv + 1, cs - cb + 1, cb))
    got_next = [tuple(r) for r in out["next"].tolist()]; got_roots = [tuple(r) for r in out["roots"].tolist()]
    assert len(set(got_next)) == len(got_next) and set(got_next) == want_next
    assert len(set(got_roots)) == len(got_roots) and set(got_roots) == want_roots
    counts = np.zeros(len(x), np.int32)
    np.add.at(counts, off[nodes[:, 2]] + nodes[:, 3], 1)
    assert (out["counts"] == counts).all()


def test_level_probe_refuses_what_it_cannot_hold():
    from canvas_amd import CanvasError
    cv = get_canvas()
    x = WC.to_x(WC.family("poisson", 400))
    ok = cv.wavelets_level_probe(x, [0, 400], np.array([[0, 100, 0, 0]], np.int32), [-1.0], wv_long=64)
    assert ok["status"].tolist() == [2] and ok["ind"][0] == _first(x[:100])
    for nodes, wv_long in (([[0, 1, 0, 0]], 64), ([[350, 100, 0, 0]], 64), ([[0, 100, 0, 0], [50, 100, 0, 0]], 64), ([[0, 100, 1, 0]], 64), ([[0, 100, 0, 0]], 7), ([[0, 100, 0, 0]], 257),
                           ([[0, 100, 0, 400]], 64)):
        with pytest.raises(CanvasError):
            cv.wavelets_level_probe(x, [0, 400], np.array(nodes, np.int32), [-1.0], wv_long=wv_long)
    many = np.array([[2 * i, 2, 0, 0] for i in range(200)], np.int32)          # the shortest nodes there are, back to back: more than 400 bins can hold at wv_long = 8
    with pytest.raises(CanvasError):
        cv.wavelets_level_probe(x, [0, 400], many, [-1.0], wv_long=8)
    out = cv.wavelets_level_probe(x, [0, 400], many[:30], [-1.0], wv_long=8)
    assert out["overflow"] == 0 and len(out["next"]) == 0 and len(out["roots"]) == 0 and int(out["counts"].sum()) == 30 and (out["ind"][out["status"] > 0] == 1).all()


def _first(x):
    return R.coefficient(x)[1]


# ------------------------------------------------------------------------------------------------------------------------------------ chains
CHAIN_LENGTHS = (9, 57, 58, 59, 113, 114, 115, 170, 171, 1002, 64, 65, 66, 129, 130)      # n - 2 = 7, 55, 56, 57, 111, 112, 113, 168, 169, 1 000 and n - 1 = 63, 64, 65, 128, 129


@functools.lru_cache(maxsize=None)
def _chain_case():
    parts, nodes, info = [], [], []
    at = 0
    for name in WC.FAMILIES:
        for n in CHAIN_LENGTHS:
            parts.append(WC.family(name, n)); nodes.append((at, n)); info.append((name, n)); at += n
    return WC.to_x(np.concatenate(parts)), np.array(nodes, np.int32), info


def _expect_chain(x, nodes, lim=None):
    coef, ind = [], []
    for i, (s, n) in enumerate(nodes.tolist()):
        c, k = R.coefficient(x[s:s + n], None if lim is None else int(lim[i]))
        coef.append(c); ind.append(k)
    return np.array(coef), np.array(ind, np.int32)


@pytest.mark.parametrize("fast", [False, True])
def test_chains_reproduce_the_recurrences_bit_for_bit(fast):
    """k_wv_coeff, k_wv_chain_long, k_wv_chunks and k_wv_reduce at the edges of the chunk of 56 steps and of the 64 lanes.  With the shortcut division no node may be
    flagged on data of this kind (flagged nodes on the MI355X: 0)."""
    cv = get_canvas()
    x, nodes, info = _chain_case()
    coef, ind, flag = cv.wavelets_chain_probe(x, nodes, fast=fast)
    ecoef = np.array([_ref(name, n)[1] for name, n in info]); eind = np.array([_ref(name, n)[2] for name, n in info], np.int32)
    print("flagged nodes:", [info[i] for i in np.flatnonzero(flag)])
    assert (flag == 0).all()
    assert (ind == eind).all(), [info[i] for i in np.flatnonzero(ind != eind)]
    assert (_bits(coef) == _bits(ecoef)).all(), [info[i] for i in np.flatnonzero(_bits(coef) != _bits(ecoef))]


@pytest.mark.parametrize("which", ["1", "55", "56", "57", "n-2", "n+5", "ind-1"])
def test_chains_that_stop_at_a_known_arg_max(which):
    """lim: the arg-max is the first one over m <= lim and the coefficient is computed from it; with lim = ind - 1 of the whole node the coefficient's bits are the whole node's"""
    cv = get_canvas()
    x, nodes, info = _chain_case()
    n = nodes[:, 1]
    full_ind = np.array([_ref(name, nn)[2] for name, nn in info], np.int32)
    lim = {"n-2": n - 2, "n+5": n + 5, "ind-1": full_ind - 1}.get(which)
    if lim is None:
        lim = np.full(len(n), int(which), np.int32)
    lim = lim.astype(np.int32)
    ecoef, eind = _expect_chain(x, nodes, lim)
    if which in ("n-2", "n+5", "ind-1"):
        assert (eind == full_ind).all() and (_bits(ecoef) == _bits(np.array([_ref(name, nn)[1] for name, nn in info]))).all()
    for fast in (True, False):
        coef, ind, flag = cv.wavelets_chain_probe(x, nodes, lim=lim, fast=fast, own_slices=fast)
        assert (flag == 0).all() and (ind == eind).all() and (_bits(coef) == _bits(ecoef)).all(), (which, fast)


def test_chains_of_overlapping_nodes_in_slices_of_their_own_and_many_nodes_in_one_call():
    from canvas_amd import CanvasError
    cv = get_canvas()
    x, nodes, _ = _chain_case()
    pick = nodes[[i for i in range(len(nodes)) if nodes[i, 1] >= 57][::3]]
    both = np.concatenate([pick, np.stack([pick[:, 0], pick[:, 1] // 2], 1), np.stack([pick[:, 0] + 3, pick[:, 1] - 5], 1)]).astype(np.int32)
    ecoef, eind = _expect_chain(x, both)
    for fast in (True, False):
        coef, ind, flag = cv.wavelets_chain_probe(x, both, fast=fast, own_slices=True)
        assert (flag == 0).all() and (ind == eind).all() and (_bits(coef) == _bits(ecoef)).all()
    with pytest.raises(CanvasError):
        cv.wavelets_chain_probe(x, both, own_slices=False)       # would share operands
    for bad in ([[0, 1]], [[len(x) - 5, 6]], [[-1, 5]]):
        with pytest.raises(CanvasError):
            cv.wavelets_chain_probe(x, np.array(bad, np.int32))
    # ~200 nodes of mixed lengths: the chunk -> node search over many bases
    rng = np.random.RandomState(9)
    y = WC.to_x(WC.family("step", 30_000, 3))
    lens = rng.choice([2, 3, 5, 56, 57, 58, 113, 200, 400], 200)
    starts = np.cumsum(np.concatenate([[0], lens[:-1] + rng.randint(0, 9, 199)]))
    mixed = np.stack([starts, lens], 1).astype(np.int32)
    assert mixed[-1].sum() <= len(y)
    ecoef, eind = _expect_chain(y, mixed)
    coef, ind, flag = cv.wavelets_chain_probe(y, mixed, fast=True)
    assert (flag == 0).all() and (ind == eind).all() and (_bits(coef) == _bits(ecoef)).all()


# ------------------------------------------------------------------------------------------------------------------------------------ subtrees
SUBTREE_LENGTHS = (2, 3, 4, 8, 63, 64, 65, 255, 256)
SUBTREE_KEEP = (40.0, -1.0)


@functools.lru_cache(maxsize=None)
def _subtree_case():
    """two chromosomes (keepAbove 40 and -1), each starting with a root at its first bin; every root with the counts and candidates of its subtree by the recursion"""
    per = [[], []]; roots = []
    j = 0
    for name in WC.FAMILIES + ("decreasing",):
        for n in SUBTREE_LENGTHS:
            c = j % 2; j += 1
            x = WC.decreasing_x(n) if name == "decreasing" else WC.to_x(WC.family(name, n))
            gap = np.zeros(j % 4 if per[c] else 0)
            s1 = sum(len(a) for a in per[c]) + len(gap) + 1
            per[c] += [gap, x]
            roots.append((c, s1, n, j % 3, R.subtree(x, j % 3, SUBTREE_KEEP[c], s1)))
    chrom = [np.concatenate(p) for p in per]
    off = np.array([0, len(chrom[0]), len(chrom[0]) + len(chrom[1])], np.int64)
    return np.concatenate(chrom), off, roots


@pytest.mark.parametrize("use_table", [True, False])
@pytest.mark.parametrize("wv_long", [8, 64, 256])
def test_subtrees_are_the_recursion_bit_for_bit(wv_long, use_table):
    cv = get_canvas()
    x, off, roots = _subtree_case()
    sel = [r for r in roots if r[2] <= wv_long]
    assert {r[2] for r in sel} == {n for n in SUBTREE_LENGTHS if n <= wv_long}
    arr = np.array([(off[c] + s1 - 1, n, c, lv, s1, off[c]) for c, s1, n, lv, _ in sel], np.int32)
    counts = np.zeros(len(x), np.int32); want = []
    for c, s1, n, lv, (cnt, cands) in sel:
        for level, k in cnt.items():
            counts[off[c] + level] += k
        want += [(c, level, s, b, e, float(coef).hex()) for level, s, b, e, coef in cands]
    assert len(set(want)) == len(want) and 0 < sum(1 for w in want if w[0] == 0) < int(counts[:off[1]].sum())
    out = cv.wavelets_subtree_probe(x, off, arr, SUBTREE_KEEP, cap_cand=len(x) + 16, wv_long=wv_long, use_table=use_table)
    got = [tuple(r) + (float(v).hex(),) for r, v in zip(out["cand"].tolist(), out["coef"].tolist())]
    assert out["overflow"] == 0 and out["ncand"] == len(want)
    assert (out["counts"] == counts).all()
    assert sorted(got) == sorted(want)
    # a candidate list that is too short: the overflow word, exactly `capacity` entries, each one of the expected
    cap = len(want) // 2
    out = cv.wavelets_subtree_probe(x, off, arr, SUBTREE_KEEP, cap_cand=cap, wv_long=wv_long, use_table=use_table)
    got = [tuple(r) + (float(v).hex(),) for r, v in zip(out["cand"].tolist(), out["coef"].tolist())]
    assert out["overflow"] != 0 and out["ncand"] == len(want) and len(got) == cap and len(set(got)) == cap and set(got) <= set(want)
    assert (out["counts"] == counts).all()


def test_subtree_probe_refuses_bad_roots():
    from canvas_amd import CanvasError
    cv = get_canvas()
    x = WC.to_x(WC.family("poisson", 300))
    for roots, wv_long in (([[0, 65, 0, 0, 1, 0]], 64), ([[0, 1, 0, 0, 1, 0]], 64), ([[290, 20, 0, 0, 291, 0]], 64), ([[10, 20, 0, 0, 10, 0]], 64), ([[10, 20, 0, 0, 11, 1]], 64),
                           ([[0, 20, 0, 0, 1, 0], [19, 5, 0, 0, 20, 0]], 64), ([[0, 8, 0, 0, 1, 0]], 7), ([[0, 8, 0, 295, 1, 0]], 64)):
        with pytest.raises(CanvasError):
            cv.wavelets_subtree_probe(x, [0, 300], np.array(roots, np.int32), [-1.0], cap_cand=100, wv_long=wv_long)


# ------------------------------------------------------------------------------------------------------------------------------------ medians of many stretches
def _median_stretches():
    rng = np.random.RandomState(17)
    fixed = [0, 1, 2, 3, 4095, 4096, 4097, 8193]
    lens = []
    for i in range(1024):
        if i < 4 * len(fixed):
            lens.append(fixed[i % len(fixed)] + (i >= 3 * len(fixed) and fixed[i % len(fixed)] > 3))      # (the fixed lengths with every kind of values, and their even / odd neighbours)
        elif i % 9 == 4 or i >= 1015:
            lens.append(0)                                  # empty stretches between the others, and last
        else:
            lens.append(int(rng.randint(1, 2500)))
    parts = []
    for i, n in enumerate(lens):
        kind = i % 6
        h = n // 2
        if kind == 0:        # the two middle elements of an even stretch in different digits of pass 0 (bits 20..30)
            k = np.concatenate([rng.randint(0, 1 << 20, h), (3 << 20) + rng.randint(0, 1 << 20, n - h)])
        elif kind == 1:      # ... of pass 1 (bits 9..19), the upper digit shared
            k = (5 << 20) + np.concatenate([rng.randint(0, 1 << 9, h), (7 << 9) + rng.randint(0, 1 << 9, n - h)])
        elif kind == 2:      # ... of pass 2: the elements differ in the low 9 bits only
            k = (1907 << 20) + (77 << 9) + rng.randint(0, 1 << 9, n)
        elif kind == 3:
            k = np.full(n, [0, 12_345, WC.KMAX][i % 3])
        elif kind == 4:      # the whole range, the largest integer among them
            k = rng.randint(0, WC.KMAX + 1, n); k[:1] = WC.KMAX
        else:
            k = rng.poisson(100, n) * 100
        k = np.asarray(k, np.int64)
        rng.shuffle(k)
        parts.append(k)
    return lens, parts


def test_medians_of_1024_stretches_bit_for_bit_on_both_paths():
    cv = get_canvas()
    lens, parts = _median_stretches()
    assert len(lens) == 1024 and lens[-1] == 0 and {0, 1, 2, 3, 4095, 4096, 4097, 8193} <= set(lens)
    k = np.concatenate(parts)
    assert int(k.max()) == WC.KMAX
    start = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    want = np.array([R.stretch_median(p) for p in parts])
    for i in (0, 1, 2):      # the constructions do what they say: the middle pair of the first even stretch of each kind differs in that pass's digit only
        p = np.sort(next(q for j, q in enumerate(parts) if j % 6 == i and len(q) % 2 == 0 and len(q) > 2)); lo, hi = int(p[len(p) // 2 - 1]), int(p[len(p) // 2])
        assert [(lo >> 20) != (hi >> 20), (lo >> 9) != (hi >> 9), True][i] and (i == 0 or (lo >> 20) == (hi >> 20)) and (i < 2 or (lo >> 9) == (hi >> 9))
    med, wg, bad = cv.wavelets_median_probe(WC.to_x(k), start, lens, per_workgroup=True)
    assert bad.tolist() == [0, 0]
    assert (_bits(med) == _bits(want)).all(), np.flatnonzero(_bits(med) != _bits(want))[:8]
    assert (_bits(wg) == _bits(want)).all(), np.flatnonzero(_bits(wg) != _bits(want))[:8]
    from canvas_amd import CanvasError
    with pytest.raises(CanvasError):
        cv.wavelets_median_probe(WC.to_x(k), np.zeros(1025, np.int64), np.ones(1025, np.int64))
    with pytest.raises(CanvasError):
        cv.wavelets_median_probe(WC.to_x(k), [len(k) - 3], [4])


# ------------------------------------------------------------------------------------------------------------------------------------ the inputs of a call
@functools.lru_cache(maxsize=None)
def _input_cases():
    """(chromosomes, window, whether the tree is slow, the oracle's coverage variability and factor-of-three values), computed once"""
    rng = np.random.RandomState(77)
    zeros = _coverage(rng, 30_000); zeros[5000:21000] = 0.0
    cases = [([_coverage(rng, 120_000, wave=0.05), _coverage(rng, 7_001), _coverage(rng, 200)], w) for w in (5000, 12000, 999)]
    cases += [([zeros, _coverage(rng, 9_000)], w) for w in (5000, 12000, 999)]
    cases += [([_coverage(rng, 160)], w) for w in (5000, 12000, 999)]
    rng = np.random.RandomState(5)
    x = np.zeros(1200); x[800:] = rng.poisson(40, 400)
    cases.append(([x], 100))                                # the NaN threshold
    # (a long stretch of equal values — the 16 000 zeros of the second coverage, an event of _coverage that zeroes a quarter of a chromosome — is one exact tie: its tree has
    # thousands of levels and costs the call 5 to 20 s.  The genome-wide statistics do not depend on the tree: such a coverage is marked slow, and the test runs it with the
    # default min_size once, and otherwise with min_size above its chromosomes — no roots, no tree.)
    def flat_run(a):
        edges = np.flatnonzero(np.diff(a) != 0)
        return int(np.diff(np.concatenate([[-1], edges, [len(a) - 1]])).max())
    return [(per, w, max(flat_run(a) for a in per) > 2000, O.coverage_variability(w, per), O.factor_of_three(per)) for per, w in cases]


def _same(a, b):
    a = np.atleast_1d(np.asarray(a, np.float64)); b = np.atleast_1d(np.asarray(b, np.float64))
    return a.shape == b.shape and bool(((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("switch", [None, "CANVAS_WV_F3_HOST", "CANVAS_WV_VAR_HOST", "CANVAS_WV_MEDIAN_PER_WG"])
def test_the_inputs_of_the_thresholds_are_the_oracle_s(monkeypatch, switch):
    """cv, the factor-of-three values and the chromosome medians as canvas_wavelets held them (canvas_wavelets_inputs), against the oracle and numpy directly: a threshold that is
    off in its last digits hardly ever moves a breakpoint.  Once per path that computes them: the device (default), the host threads, the per-workgroup medians; the call
    reports which path it took (paths), so a switch that did not reach the library fails here.  A coverage whose tree is slow (_input_cases) has its chromosomes as roots —
    median, sigma and keepAbove compared — in one call, under the default switches at window 999; its other calls compare cv and the factor-of-three values."""
    cv = get_canvas()
    if switch:
        monkeypatch.setenv(switch, "1")
    lower, upper, mad_factor = 0.05, 80.0, 5.0
    roots = slow_roots = 0
    for per, window, slow, ocv, of3 in _input_cases():
        min_size = 200_000 if slow and not (switch is None and window == 999) else 10
        off = np.concatenate([[0], np.cumsum([len(a) for a in per])]).astype(np.int64)
        t0 = time.perf_counter()
        cv.wavelets(to_dev(np.concatenate(per), cv.device), off, window=window, min_size=min_size)      # (its breakpoints: tests/test_wavelets_gpu.py)
        print(f"{[len(a) for a in per]} window {window} min_size {min_size}: {time.perf_counter() - t0:.2f} s")
        inp = cv.wavelets_inputs(len(per))
        has_cv = sum(len(a) for a in per) >= 10 * window
        want = dict(f3_device=switch != "CANVAS_WV_F3_HOST", var_device=has_cv and switch != "CANVAS_WV_VAR_HOST", median_device=has_cv and switch != "CANVAS_WV_VAR_HOST",
                    median_from_integers=has_cv and switch not in ("CANVAS_WV_VAR_HOST", "CANVAS_WV_MEDIAN_PER_WG"))
        assert inp["paths"] == want, ("the hook did not reach the library", switch, inp["paths"], want)
        assert inp["has_cv"] == (ocv is not None)
        if ocv is not None:
            assert _same(inp["cv"], ocv), (inp["cv"], ocv)
        assert _same(inp["f3"], of3), (inp["f3"], of3)
        for c, a in enumerate(per):
            assert inp["is_root"][c] == (len(a) > min_size)
            if not inp["is_root"][c]:
                assert inp["median"][c] == 0.0
                continue
            roots += 1; slow_roots += slow
            median = float(np.median(a))
            assert _same(inp["median"][c], median)
            threshold = mad_factor * (median * ocv if ocv is not None else float(np.median(np.abs(a - median))))
            if threshold < lower:
                threshold = lower
            if threshold > upper:
                threshold = upper
            assert _same(inp["sigma"][c], threshold), (c, inp["sigma"][c], threshold)
            keep = 2 * threshold * math.sqrt(2 * math.log(float(len(a))))
            assert inp["keep_above"][c] == -1.0 if math.isnan(threshold) else 0.99 * keep < inp["keep_above"][c] <= keep
    assert roots >= 10 and slow_roots == (2 if switch is None else 0)
