"""The restatements behind the direct tests of the Wavelets kernels (tests/wavelets_ref.py, tests/wavelets_cases.py), checked on the CPU against each other: the hand-derived
rounding-error bound of DESIGN.md (Wavelets, *The bound*) holds for the sequential recurrences on every family, it decides what has one arg-max and leaves exact ties alone,
and the depth-first subtree is the level-by-level tree of the other restatement (tests/test_oracle_independent.py).  No GPU, no oracle."""
import numpy as np
import pytest

import wavelets_cases as WC
import wavelets_ref as R

SIZES = (9, 65, 2049, 6000)


@pytest.fixture(scope="module")
def model():
    """(family, n) -> (ratio of the bound, decision of the closed form, first arg-max of the recurrences), computed once"""
    out = {}
    for name in WC.FAMILIES:
        for n in SIZES:
            k = WC.family(name, n)
            ipi, _ = R.inner_products(WC.to_x(k).tolist())
            T, B = R.closed_form(k)
            out[name, n] = (R.bound_ratio(ipi, T, B), R.decided(T, B), R.first_argmax(ipi))
    return out


@pytest.mark.parametrize("name", WC.FAMILIES)
def test_the_bound_holds_for_the_recurrences(model, name):
    for n in SIZES:
        ratio = model[name, n][0]
        print(f"{name} n={n}: max |ref - T| / B = {ratio:.3g}")
        assert ratio <= 1.0, (name, n, ratio)


def test_the_largest_ratio_is_far_from_one(model):
    """B[m] adds up the magnitude of every rounding of the recurrences at its full half unit in the last place, all with one sign: real roundings are neither all at the limit
    nor of one sign, so the ratio stays well below 1.  The slips such a derivation is prone to — a unit in the last place taken for half of one or the other way round, a term
    counted once that enters twice — are factors of two: a ratio above 0.5 on any family says that the margin a correct bound has is gone, before the bound itself is broken."""
    worst = max((v[0], key) for key, v in model.items())
    print("largest ratio", worst)
    assert worst[0] <= 0.5, worst


@pytest.mark.parametrize("name", WC.NON_TIE)
def test_non_tie_families_are_decided_and_at_the_reference_arg_max(model, name):
    for n in SIZES:
        _, dec, ind = model[name, n]
        assert dec is not None and dec == ind, (name, n, dec, ind)


@pytest.mark.parametrize("name", WC.TIE_ANY_N + WC.TIE_ODD_N)
def test_tie_families_are_not_decided(model, name):
    for n in SIZES:
        if WC.is_tie(name, n):
            assert model[name, n][1] is None, (name, n)


def test_a_zero_bound_means_equality():
    T, B = R.closed_form(WC.family("zero", 65))
    assert all(b == 0.0 for b in B) and all(t == 0.0 for t in T)
    ipi, _ = R.inner_products([0.0] * 65)
    assert R.bound_ratio(ipi, T, B) == 0.0
    assert R.bound_ratio([1e-300] + ipi[1:], T, B) == float("inf")


def test_subtree_is_the_tree_of_the_other_restatement():
    from test_oracle_independent import py_haar_tree
    rng = np.random.RandomState(808)
    vectors = [WC.to_x(WC.family("poisson", 40)), WC.to_x(WC.family("step", 63)), WC.to_x(WC.family("flat", 17)), WC.to_x(WC.family("ramp", 33)), WC.decreasing_x(24),
               np.round(rng.normal(100, 10, 97), 2), np.array([3.0, 1.0]), np.array([1.0, 5.0, 2.0])]
    for x in vectors:
        tree = py_haar_tree([float(v) for v in x])
        counts, cands = R.subtree(x, 0, -1.0)
        assert counts == {j: len(level) for j, level in enumerate(tree)}
        want = sorted((j, start, split, end, coef) for j, level in enumerate(tree) for _, coef, start, split, end in level)
        assert sorted(cands) == want
        # a threshold keeps exactly the coefficients above it, a start level and a start position shift the labels
        keep = float(np.median([abs(c[4]) for c in cands]))
        counts2, cands2 = R.subtree(x, 5, keep, s1=11)
        assert counts2 == {j + 5: c for j, c in counts.items()}
        assert sorted(cands2) == sorted((lv + 5, s + 10, b + 10, e + 10, c) for lv, s, b, e, c in cands if abs(c) > keep)


def test_decreasing_family_splits_off_one_bin_per_node():
    for n in (8, 64, 256):
        counts, _ = R.subtree(WC.decreasing_x(n), 0, -1.0)
        assert counts == {lv: 1 for lv in range(n - 1)}


def test_prefix_sums_and_medians():
    k = np.array([5, 0, WC.KMAX, 7, 1, 2], np.int64)
    p1, p2 = R.prefix_sums(k, [0, 3, 3, 6])
    assert p1.tolist() == [5, 5, 5 + WC.KMAX, 7, 8, 10] and p2.tolist() == [5, 10, 15 + WC.KMAX, 7, 15, 25]
    assert R.stretch_median(k[:0]) == 0.0 and R.stretch_median(k[:1]) == 0.05 and R.stretch_median(k[3:]) == 0.02
    assert R.stretch_median(np.array([1, 2], np.int64)) == (0.01 + 0.02) / 2
    assert R.stretch_median(k) == float(np.median(k / 100.0))
