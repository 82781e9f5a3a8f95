"""Canvas.flag_unique_kmers / Canvas.fasta_case_from_mask (canvas_amd/csrc/kmer.hip) against the CPU restatements of Tools/FlagUniqueKmers (tests/kmer_ref.py).
Every comparison is bit equality of whole masks."""
import numpy as np
import pytest

import kmer_cases as KC
import kmer_ref as R
from gpu_common import get_canvas, to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cv():
    return get_canvas()


def _upload(cv, contigs):
    import torch
    arrs = [np.frombuffer(bytes(c), np.uint8) if not isinstance(c, np.ndarray) else c for c in contigs]
    bases = [to_dev(a, cv.device) if len(a) else torch.zeros(0, dtype=torch.uint8, device=cv.device) for a in arrs]
    return arrs, bases, np.array([len(a) for a in arrs], np.int64)


def gpu_masks(cv, contigs, max_table_bytes=0, keep=None):
    arrs, bases, lens = _upload(cv, contigs)
    masks, stats = cv.flag_unique_kmers(bases, lens, max_table_bytes=max_table_bytes)
    if keep is not None:
        keep.update(arrs=arrs, bases=bases, lens=lens)
    return [m.cpu().numpy().view(np.uint64) for m in masks], stats


def expect_masks(flags):
    return [R.pack_mask(f) for f in flags]


def assert_same(got, exp, what=""):
    assert len(got) == len(exp)
    for c, (g, e) in enumerate(zip(got, exp)):
        assert g.shape == e.shape and (g == e).all(), (what, c, int((g != e).sum()) if g.shape == e.shape else "shape")


def check_stats(stats, contigs, flags):
    assert stats["positions"] == sum(len(c) for c in contigs)
    assert stats["unique"] == sum(int(f.sum()) for f in flags)
    assert stats["unique"] <= stats["keyed"] <= stats["positions"]


@pytest.mark.parametrize("case", KC.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(cv, case):
    name, contigs, expected = case
    got, stats = gpu_masks(cv, contigs)
    assert_same(got, expect_masks(expected), name)
    check_stats(stats, contigs, expected)


@pytest.mark.parametrize("seed", range(6))
def test_low_complexity_genomes_against_the_line_by_line_restatement(cv, seed):
    contigs = KC.low_complexity_genome(seed)
    flags, _ = R.unique_flags_checker(contigs)
    got, stats = gpu_masks(cv, contigs)
    assert_same(got, expect_masks(flags), seed)
    check_stats(stats, contigs, flags)


@pytest.fixture(scope="module")
def planted():
    G = KC.planted_genome()
    return G, R.unique_flags_numpy(G)


def test_planted_genome(cv, planted):
    """~20 Mb, seven contigs, copies on both strands (within and across contigs, some in contig tails), tandem repeats, homopolymers, N runs; the same call
    repeated gives the same masks (thread order does not matter), and the bases are not modified"""
    G, flags = planted
    keep = {}
    got, stats = gpu_masks(cv, G, keep=keep)
    exp = expect_masks(flags)
    assert_same(got, exp, "planted")
    check_stats(stats, G, flags)
    assert stats["passes"] == 1 and stats["longest_probe"] >= 1 and stats["table_bytes"] == 8 * stats["table_slots"]
    for a, b in zip(keep["arrs"], keep["bases"]):
        assert (b.cpu().numpy() == a).all()
    again, stats2 = cv.flag_unique_kmers(keep["bases"], keep["lens"])
    assert_same([m.cpu().numpy().view(np.uint64) for m in again], exp, "planted, repeated")
    assert stats2["unique"] == stats["unique"] and stats2["keyed"] == stats["keyed"]


def test_small_table_takes_many_passes_and_gives_the_same_masks(cv, planted):
    G, flags = planted
    _, one = gpu_masks(cv, G)
    budget = one["table_bytes"] // 9
    got, stats = gpu_masks(cv, G, max_table_bytes=budget)
    assert stats["passes"] >= 8, stats
    assert stats["table_bytes"] <= budget
    assert_same(got, expect_masks(flags), "planted, small table")
    check_stats(stats, G, flags)
    # a given mask tensor list is filled in place
    arrs, bases, lens = _upload(cv, G)
    import torch
    mine = [torch.full(((int(L) + 63) // 64,), -1, dtype=torch.int64, device=cv.device) for L in lens]
    out, _ = cv.flag_unique_kmers(bases, lens, masks=mine, max_table_bytes=budget * 2)
    assert all(a is b for a, b in zip(out, mine))
    assert_same([m.cpu().numpy().view(np.uint64) for m in mine], expect_masks(flags), "planted, given masks")


def test_budget_below_one_class_is_an_error(cv, planted):
    from canvas_amd import CanvasError
    G, _ = planted
    with pytest.raises(CanvasError, match="largest key class"):
        gpu_masks(cv, G[-1:], max_table_bytes=4096)


def test_two_letter_genome(cv):
    G = KC.two_letter_genome()
    flags = R.unique_flags_numpy(G)
    assert 0 < sum(int(f.sum()) for f in flags) < sum(len(g) for g in G) - 70
    for budget in (0, 3 << 20):
        got, stats = gpu_masks(cv, G, max_table_bytes=budget)
        assert_same(got, expect_masks(flags), ("two letters", budget))
        check_stats(stats, G, flags)
    assert stats["passes"] > 1


def test_period36_tiling(cv):
    """36 distinct 35-mers, each tens of thousands of times: nothing is unique, and a class holds many equal keys"""
    G = KC.period36_genome()
    flags = R.unique_flags_numpy(G)
    assert not any(f.any() for f in flags)
    got, stats = gpu_masks(cv, G)
    assert_same(got, expect_masks(flags), "period 36")
    assert stats["unique"] == 0 and stats["keyed"] == sum(len(g) - 35 for g in G)


def test_many_contigs(cv):
    """thousands of contigs, empty ones, ones shorter than 36, all-'n' ones and ones that repeat another contig"""
    G = KC.many_contig_genome(3000)
    lens = [len(g) for g in G]
    assert lens.count(0) > 10 and sum(0 < n < 36 for n in lens) > 10
    flags = R.unique_flags_numpy(G)
    got, stats = gpu_masks(cv, G)
    assert_same(got, expect_masks(flags), "3000 contigs")
    check_stats(stats, G, flags)
    got, stats = gpu_masks(cv, G, max_table_bytes=stats["table_bytes"] // 5)
    assert stats["passes"] >= 4
    assert_same(got, expect_masks(flags), "3000 contigs, small table")


def test_no_contigs_and_nothing_keyed(cv):
    masks, stats = cv.flag_unique_kmers([], [])
    assert masks == [] and stats["positions"] == 0 and stats["passes"] == 0
    got, stats = gpu_masks(cv, [b"ACGT" * 8, b"", b"N" * 200])
    assert [g.tolist() for g in got] == [[0], [], [0, 0, 0, 0]] and stats["keyed"] == 0 and stats["unique"] == 0


def test_case_from_mask_is_the_inverse_of_mask_from_fasta(cv):
    import torch
    rng = np.random.RandomState(5)
    for L in (1, 15, 16, 17, 64, 1000, 100_003):
        alphabet = np.frombuffer(b"ACGTNacgtnRr-*0@[`{\x00\xc1\xe1", np.uint8)
        b = alphabet[rng.randint(0, len(alphabet), L)]
        bits = rng.rand(L) < 0.5
        m = R.pack_mask(bits)
        d_b = to_dev(np.concatenate([b, np.zeros((-L) % 16, np.uint8)]), cv.device)
        d_m = to_dev(m.view(np.int64), cv.device)
        cv.fasta_case_from_mask(d_b, L, d_m)
        out = d_b.cpu().numpy()[:L]
        assert out.tobytes() == R.apply_case(b, bits)
        letters = ((b | 0x20) >= ord("a")) & ((b | 0x20) <= ord("z")) & (b < 0x80)
        assert (out[~letters] == b[~letters]).all()                        # non-letters pass through untouched
        back = cv.mask_from_fasta(d_b, L).cpu().numpy().view(np.uint64)
        want = R.pack_mask(bits & letters)                                 # char.IsUpper is false for a non-letter
        assert (back == want).all(), L
    # on letters alone the round trip is the identity
    L = 4099
    b = np.frombuffer(b"ACGTacgtNn", np.uint8)[rng.randint(0, 10, L)]
    bits = rng.rand(L) < 0.3
    d_b = to_dev(np.concatenate([b, np.zeros((-L) % 16, np.uint8)]), cv.device)
    cv.fasta_case_from_mask(d_b, L, to_dev(R.pack_mask(bits).view(np.int64), cv.device))
    assert (cv.mask_from_fasta(d_b, L).cpu().numpy().view(np.uint64) == R.pack_mask(bits)).all()
    assert torch.equal(d_b[L:], torch.zeros_like(d_b[L:]))
