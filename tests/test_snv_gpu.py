"""Canvas.snv_count (canvas_amd/csrc/snv.hip) against the sequential restatement of SNVReviewer.ProcessBamFile (tests/snv_ref.py): directed records, a seeded
random soak split into chunks, and malformed records.  Counts are integers: every comparison is exact and covers every site."""
import numpy as np
import pytest

import snv_ref as R
import snv_cases as SC
from gpu_common import get_canvas, to_dev

pytestmark = pytest.mark.gpu
V = R.Variant


@pytest.fixture(scope="module")
def cv():
    return get_canvas()


def _sites_dev(cv, variants):
    import torch
    from canvas_amd.lib import snv_allele_codes
    pos = to_dev(np.array([v.pos for v in variants], np.int32), cv.device) if variants else torch.zeros(0, dtype=torch.int32, device=cv.device)
    ref = to_dev(snv_allele_codes([v.ref for v in variants]), cv.device) if variants else torch.zeros(0, dtype=torch.uint8, device=cv.device)
    alt = to_dev(snv_allele_codes([v.alt for v in variants]), cv.device) if variants else torch.zeros(0, dtype=torch.uint8, device=cv.device)
    return pos, ref, alt


def gpu_pileup(cv, reads, variants, min_mapq=0, cuts=(), ref_id=0, pad=SC.PAD, min_base_q=20):
    """the reads in chunks [0, cuts[0]), [cuts[0], cuts[1]), ...; -> (ref counts, alt counts, summed info)"""
    import torch
    pos, ref, alt = _sites_dev(cv, variants)
    rc = ac = None
    info = np.zeros(5, np.int64)
    bounds = [0] + list(cuts) + [len(reads)]
    for a, b in zip(bounds[:-1], bounds[1:]):
        buf, offs, nbytes = SC.chunk_of(reads[a:b], pad)
        d_buf = to_dev(buf, cv.device) if len(buf) else torch.zeros(1, dtype=torch.uint8, device=cv.device)
        d_off = to_dev(offs, cv.device) if len(offs) else torch.zeros(0, dtype=torch.int64, device=cv.device)
        rc, ac, i5 = cv.snv_count(d_buf, d_off, ref_id, pos, ref, alt, rc, ac, min_mapq=min_mapq, min_base_q=min_base_q, nbytes=nbytes)
        info += i5
    n = len(variants)
    return rc.cpu().numpy()[:n].tolist(), ac.cpu().numpy()[:n].tolist(), info


def check(cv, reads, variants, min_mapq=0, cuts=(), what=""):
    exp = R.pileup(reads, 0, variants, min_mapq)
    rc, ac, info = gpu_pileup(cv, reads, variants, min_mapq, cuts)
    assert (rc, ac) == (list(exp[0]), list(exp[1])), what
    assert info[0] == len(reads) and info[4] == 0, (what, info)
    return info


def _read(pos, cigar, seq, **kw):
    d = dict(ref=0, pos=pos, cigar=cigar, seq=seq, flag=0, mapq=30, qual=[30] * len(seq))
    d.update(kw)
    return d


def test_filters(cv):
    site = [V("c", 11, "A", "C")]
    flags = [0, 0x100, 0x4, 0x400, 0x200, 0x800, 0x10, 0x1, 0x100 | 0x4, 0x400 | 0x200, 0x100 | 0x400 | 0x4, 0x800 | 0x200 | 0x10, 0x41, 0x81, 0x904, 0xFFFF]
    for f in flags:
        info = check(cv, [_read(10, [(4, "M")], "ACGT", flag=f)], site, what="flag %x" % f)
        assert info[1] == (0 if f & 0x504 else 1), f
    check(cv, [_read(10, [(4, "M")], "ACGT", flag=f) for f in flags], site, what="all flags")
    for q, m in ((5, 5), (6, 5), (0, 0), (1, 0), (255, 254), (255, 255), (30, 29)):
        check(cv, [_read(10, [(4, "M")], "ACGT", mapq=q)], site, min_mapq=m, what="mapq %d min %d" % (q, m))


def test_cigar_operations_in_every_place(cv):
    sites = [V("c", p, "A", "C") for p in range(5, 60)]
    for op in "MIDNSHP=X":
        for place in range(3):
            cig = [(5, "M"), (6, "M"), (7, "M")]
            cig[place] = (3, op)
            need = sum(k for k, o in cig if o in "MIS=X")
            check(cv, [_read(10, cig, ("ACCAAC" * 5)[:need])], sites, what="%s at %d" % (op, place))
    info = check(cv, [_read(10, [(3, "H"), (5, "M")], "AAAAA"), _read(10, [(5, "M"), (2, "N"), (5, "M")], "AAAAAAAAAA"), _read(10, [(5, "M")], "AAAAA")], sites)
    assert info[2] == 3 and info[3] == 2                        # walked 3, two of them ended at an unsupported operation


def test_site_placement(cv):
    # sites on the base before the read, its first and last base, the base behind it; on a deleted base; inside an insertion's reference gap
    r = _read(20, [(2, "S"), (4, "M"), (3, "I"), (2, "M"), (3, "D"), (4, "M")], "GGACGTTTTCAACGT")
    sites = [V("c", p, b, "A") for p in range(18, 36) for b in "ACGT"]
    check(cv, [r], sites)
    for p in (20, 21, 24, 25, 26, 27, 28, 29, 30, 33, 34):      # one site at a time: 0-based 19 (before) .. 33 (behind)
        check(cv, [r], [V("c", p, "A", "C")], what="site %d" % p)


def test_qualities_alleles_duplicates(cv):
    for q in (0, 19, 20, 21, 254, 255):
        check(cv, [_read(10, [(3, "M")], "ACA", qual=[30, q, 30])], [V("c", 12, "C", "T"), V("c", 12, "C", "C")], what="qual %d" % q)
    sites = [V("c", 11, x, y) for x, y in (("A", "A"), ("a", "A"), ("A", "a"), (".", "A"), ("A", "."), ("N", "A"), ("=", "A"), ("R", "M"), ("A", "C"), ("A", "C"))]
    for base in "ACGTN=RM":
        check(cv, [_read(10, [(2, "M")], base + "A")], sites, what="base " + base)
    rc, ac, _ = gpu_pileup(cv, [_read(10, [(2, "M")], "AA")], sites)
    assert rc == [1, 0, 1, 0, 1, 0, 0, 0, 1, 1] and ac == [1, 1, 0, 1, 0, 1, 1, 0, 0, 0]        # written out: exact characters, duplicates each


def test_thousand_base_rule(cv):
    long_read = _read(100, [(1500, "M")], "A" * 1500)
    for off in (999, 1000, 1001):
        check(cv, [long_read], [V("c", 101 + off, "A", "C")], what="offset %d" % off)
    rc, ac, _ = gpu_pileup(cv, [long_read], [V("c", 1100, "A", "C")])
    assert rc == [1]
    rc, ac, _ = gpu_pileup(cv, [long_read], [V("c", 1101, "A", "C")])
    assert rc == [0]
    check(cv, [long_read], [V("c", 1100, "A", "C"), V("c", 1101, "A", "C"), V("c", 1599, "A", "C"), V("c", 1600, "A", "C"), V("c", 1601, "A", "C")])
    check(cv, [long_read], [V("c", 100, "A", "C"), V("c", 1500, "A", "C")])
    check(cv, [_read(100, [(700, "M"), (600, "D"), (800, "M")], "A" * 1500)], [V("c", 900, "A", "C"), V("c", 1500, "A", "C"), V("c", 2200, "A", "C"), V("c", 2201, "A", "C")])


def test_edges_of_the_lists(cv):
    reads = [_read(p, [(10, "M")], "ACGTACGTAC") for p in (5, 50, 500, 5000)]
    check(cv, reads, [V("c", 8, "T", "A"), V("c", 55, "A", "C")])          # reads behind the last site
    check(cv, reads, [])                                                     # zero sites
    rc, ac, info = gpu_pileup(cv, [], [V("c", 8, "T", "A")])                 # zero records
    assert rc == [0] and ac == [0] and info.tolist() == [0] * 5
    other = [dict(r, ref=1) for r in reads]
    rc, ac, info = gpu_pileup(cv, other, [V("c", 8, "T", "A")])              # another reference's records add nothing
    assert rc == [0] and info[0] == 4 and info[1] == 0


@pytest.mark.parametrize("seed", range(6))
def test_random_soak(cv, seed):
    """reads of 35-300 bases plus a long-read class, random CIGARs, depth up to a few hundred; site densities from one per 10 kb to every base; 1, 2 and many chunks"""
    rng = np.random.RandomState(20261016 + seed)
    nconf = 0
    for every in (10000, 1000, 100, 10, 1):
        for depth_cfg in range(8):
            span = int(rng.choice([400, 3000, 40000]))
            n = int(rng.choice([50, 400, 1500]))
            if every >= 1000:
                span = max(span, 40000)
            reads = SC.random_reads(rng, n, span, long_frac=float(rng.choice([0, 0.05])), exotic=0.08)
            sites = SC.random_sites(rng, span + 400, every)
            mq = int(rng.choice([0, 5]))
            exp = R.pileup(reads, 0, sites, mq)
            for cuts in ((), (int(rng.randint(0, n + 1)),), tuple(sorted(rng.randint(0, n + 1, 7).tolist()))):
                rc, ac, info = gpu_pileup(cv, reads, sites, mq, cuts, pad=0)
                assert rc == list(exp[0]) and ac == list(exp[1]), (seed, every, depth_cfg, cuts)
                assert info[0] == n and info[4] == 0
            nconf += 1
    assert nconf == 40


def test_contended_site(cv):
    """several hundred reads over the same few sites: the atomics on one word"""
    rng = np.random.RandomState(7)
    reads = sorted((_read(int(rng.randint(0, 60)), [(100, "M")], "".join(rng.choice(list("ACGT"), 100))) for _ in range(3000)), key=lambda r: r["pos"])
    sites = [V("c", p, "A", "C") for p in (70, 70, 71, 99)]
    info = check(cv, reads, sites, cuts=(1000, 1001, 2500))
    assert info[2] == 3000


def test_malformed_records(cv):
    """every bad record sits inside a padded allocation, so that a kernel WITHOUT the check would read wrong bytes, not fault; the good records around it must count as if it
    were absent and info must report it"""
    sites = [V("c", p, "A", "C") for p in range(1, 400)]
    good = lambda p: _read(p, [(20, "M")], "ACCA" * 5)
    cases = {
        "l_seq shorter than the CIGAR consumes": _read(30, [(20, "M")], "ACCA" * 5, l_seq=6, tail=bytes(12)),
        "CIGAR count past block_size": _read(30, [(20, "M")], "ACCA" * 5, n_cigar=4000),
        "name length past block_size": _read(30, [(20, "M")], "ACCA" * 5, l_read_name=255, block_size=60),
        "negative l_seq": _read(30, [(20, "M")], "ACCA" * 5, l_seq=-5),
        "block_size below the fixed fields": _read(30, [(20, "M")], "ACCA" * 5, block_size=8),
    }
    for what, bad in cases.items():
        reads = [good(10), good(25), bad, good(31), good(45)]
        exp = R.pileup([r for r in reads if r is not bad], 0, sites)
        rc, ac, info = gpu_pileup(cv, reads, sites)
        assert (rc, ac) == (list(exp[0]), list(exp[1])), what
        assert info[0] == 5 and info[4] == 1, (what, info)
    # a record offset whose record would end past nbytes: the last record is announced, but nbytes stops in the middle of it (the bytes are there: padding)
    import torch
    reads = [good(10), good(25), good(31)]
    buf, offs, nbytes = SC.chunk_of(reads, SC.PAD)
    pos, ref, alt = _sites_dev(cv, sites)
    for short in (1, 20, len(R.encode_record(reads[2])) - 1):
        rc, ac, info = cv.snv_count(to_dev(buf, cv.device), to_dev(offs, cv.device), 0, pos, ref, alt, nbytes=nbytes - short)
        exp = R.pileup(reads[:2], 0, sites)
        assert rc.cpu().numpy()[:len(sites)].tolist() == list(exp[0]) and ac.cpu().numpy()[:len(sites)].tolist() == list(exp[1]), short
        assert info[0] == 3 and info[4] == 1
    bad_offs = np.array([0, nbytes + 5, 1 << 40, -1], np.int64)                # offsets outside the chunk
    rc, ac, info = cv.snv_count(to_dev(buf, cv.device), to_dev(bad_offs, cv.device), 0, pos, ref, alt, nbytes=nbytes)
    exp = R.pileup(reads[:1], 0, sites)
    assert rc.cpu().numpy()[:len(sites)].tolist() == list(exp[0]) and info[4] == 3
