"""The two CPU restatements of Tools/FlagUniqueKmers (tests/kmer_ref.py) against each other and against hand-checked cases: what the GPU tests compare with is itself
checked here, without a GPU."""
import numpy as np
import pytest

import kmer_cases as KC
import kmer_ref as R


@pytest.mark.parametrize("case", KC.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(case):
    name, contigs, expected = case
    a, _ = R.unique_flags_checker(contigs)
    b = R.unique_flags_numpy(contigs)
    assert len(a) == len(b) == len(expected)
    for fa, fb, fe in zip(a, b, expected):
        assert fa.tolist() == fe.tolist(), name
        assert fb.tolist() == fe.tolist(), name


def test_tail_includes_l_minus_35():
    """rule 2 is >=: position L - 35, whose 35-mer fits, is lower case"""
    seq = KC.rand_seq(np.random.RandomState(1), 80)
    for fn in (lambda c: R.unique_flags_checker(c)[0], R.unique_flags_numpy):
        f = fn([seq])[0]
        assert f[:45].all() and not f[45:].any()
    assert R.apply_case(seq.lower(), R.unique_flags_numpy([seq])[0]) == seq[:45] + seq[45:].lower()


def test_key_is_canonical_and_order_preserving():
    rng = np.random.RandomState(2)
    for _ in range(50):
        k = KC.rand_seq(rng, 35)
        key = R.KmerChecker.GetKeyForKmer(k.decode())
        assert key == R.KmerChecker.GetKeyForKmer(R.revcomp(k).decode()) and len(key) == 9
        assert k != R.revcomp(k)                       # 35 is odd
        num = lambda s: int("".join(str(b"ACGT".index(ch)) for ch in s), 4)
        packed = lambda v: sum(ord(ch) << (8 * (8 - i) - 2 if i < 8 else 0) for i, ch in enumerate(v))      # eight 8-bit characters, then a 6-bit one
        assert packed(key) == min(num(k), num(R.revcomp(k)))
    assert R.KmerChecker.GetKeyForKmer("A" * 34 + "N") is None


@pytest.mark.parametrize("seed", range(12))
def test_restatements_agree_on_low_complexity_genomes(seed):
    contigs = KC.low_complexity_genome(seed)
    a, _ = R.unique_flags_checker(contigs)
    b = R.unique_flags_numpy(contigs)
    for fa, fb in zip(a, b):
        assert fa.tolist() == fb.tolist()


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_dictionary_cap_does_not_change_the_answer(seed):
    """rule 5: the 400 M-entry passes bound memory only"""
    contigs = KC.low_complexity_genome(100 + seed, ncontigs=6, max_len=900) + [KC.rand_seq(np.random.RandomState(seed), 400)]      # more than 100 distinct keys
    full, p_full = R.unique_flags_checker(contigs)
    assert p_full == 1
    for cap in (7, 100):
        capped, passes = R.unique_flags_checker(contigs, cap)
        assert passes > 1
        for fa, fb in zip(full, capped):
            assert fa.tolist() == fb.tolist(), cap


def test_planted_genome_exercises_both_outcomes():
    """the ~20 Mb GPU case: between 5 % and 60 % of its positions are non-unique"""
    G = KC.planted_genome()
    flags = R.unique_flags_numpy(G)
    total = sum(len(g) for g in G)
    non_unique = total - sum(int(f.sum()) for f in flags)
    assert 0.05 < non_unique / total < 0.60, non_unique / total
    # the planted material is there: tail positions of every contig, Ns, and copies across contigs
    assert all(not f[-35:].any() for f in flags)
    assert any((g == ord("N")).any() for g in G)


def test_pack_mask_and_render():
    f = np.zeros(70, bool); f[[0, 63, 64, 69]] = True
    w = R.pack_mask(f)
    assert w.tolist() == [(1 << 63) | 1, 1 | (1 << 5)]
    assert R.pack_mask(np.zeros(0, bool)).size == 0
    out = R.render_fasta(["c1", "e"], [b"acgtN-*x", b""], [np.array([1, 0, 1, 0, 1, 1, 1, 1], bool), np.zeros(0, bool)])
    assert out == b">c1\nAcGtN-*X\n>e\n\n"
