"""CPU checks of the CanvasSNV restatement (tests/snv_ref.py) against the reference's own known answers and hand-computed pileups, one per rule of the pileup;
the executable's argument conventions that need no device; the new ABI symbols."""
import json
import os
import subprocess

import pytest

import snv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "canvas_amd", "bin", "CanvasSNV")
V = R.Variant


def _read(pos, cigar, seq, **kw):
    d = dict(ref=0, pos=pos, cigar=cigar, seq=seq, flag=0, mapq=30, qual=[30] * len(seq))
    d.update(kw)
    return d


def test_b_allele_frequency_reference_cases():
    """the six InlineData rows of CanvasTest/TestCanvasSNV.cs"""
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "snv_baf_cases.json")))
    assert len(cases) == 6
    for c in cases:
        assert R.b_allele_frequency(c["ref"], c["alt"], c["ref_count"], c["alt_count"]) == c["expected"], c


def test_b_allele_frequency_dot_and_invalid():
    assert R.b_allele_frequency(".", "A", 1, 1) is None and R.b_allele_frequency("A", ".", 1, 1) is None
    assert R.b_allele_frequency("a", "c", 1, 3) == 0.25
    with pytest.raises(ValueError):
        R.b_allele_frequency("A", "N", 1, 1)


def test_g15_text():
    assert [R.format_g15(v) for v in (1 / 3, 2 / 3, 1 / 7, 0.5, 1.0, 0.0)] == ["0.333333333333333", "0.666666666666667", "0.142857142857143", "0.5", "1", "0"]
    assert R.format_g15(1 / 3000000) == "3.33333333333333E-07" and R.format_g15(0.00001) == "1E-05" and R.format_g15(0.0001) == "0.0001"


# ---- one hand-computed pileup per numbered rule
def test_rule1_read_filters():
    site = [V("c", 11, "A", "C")]                       # 0-based 10: base index 0 of a read at 10
    def one(**kw):
        return R.pileup([_read(10, [(4, "M")], "ACGT", **kw)], 0, site, kw.pop("min_mapq_", 0))
    assert one() == ([1], [0])
    for flag in (0x100, 0x4, 0x400, 0x100 | 0x10, 0x404):
        assert one(flag=flag) == ([0], [0]), flag
    for flag in (0x200, 0x800, 0x10, 0x1 | 0x40):       # failed QC, supplementary, reverse strand, paired: counted
        assert one(flag=flag) == ([1], [0]), flag
    assert R.pileup([_read(10, [(4, "M")], "ACGT", mapq=5)], 0, site, 5) == ([0], [0])       # mapq <= min_mapq
    assert R.pileup([_read(10, [(4, "M")], "ACGT", mapq=6)], 0, site, 5) == ([1], [0])
    assert R.pileup([_read(10, [(4, "M")], "ACGT", mapq=0)], 0, site, 0) == ([0], [0])
    # both mates where they overlap
    assert R.pileup([_read(10, [(4, "M")], "ACGT", flag=0x41), _read(10, [(4, "M")], "CCGT", flag=0x81)], 0, site) == ([1], [1])


def test_rule2_scan_pointer_and_1000_bases():
    long_read = lambda: _read(100, [(1500, "M")], "A" * 1500)
    # the first site at or behind the read decides: offsets 999 / 1000 / 1001 from the read's start are 1-based positions 1100 / 1101 / 1102
    assert R.pileup([long_read()], 0, [V("c", 1100, "A", "C")]) == ([1], [0])
    assert R.pileup([long_read()], 0, [V("c", 1101, "A", "C")]) == ([0], [0])      # pos + 1000 < 1101: lost, although the read covers it
    assert R.pileup([long_read()], 0, [V("c", 1102, "A", "C")]) == ([0], [0])
    assert R.pileup([long_read()], 0, [V("c", 1100, "A", "C"), V("c", 1101, "A", "C")]) == ([1, 1], [0, 0])      # a near site keeps the far one
    assert R.pileup([long_read()], 0, [V("c", 100, "A", "C"), V("c", 1500, "A", "C")]) == ([0, 1], [0, 0])       # pos1 == pos: in reach, not on the read
    # no site at or behind the read: nothing, and the loop ends
    assert R.pileup([_read(100, [(4, "M")], "AAAA"), _read(101, [(4, "M")], "AAAA")], 0, [V("c", 50, "A", "C")]) == ([0], [0])
    assert R.pileup([_read(100, [(4, "M")], "AAAA")], 0, []) == ([], [])


def test_rule3_cigar_walk():
    sites = [V("c", p, "A", "C") for p in range(11, 31)]       # 0-based 10..29
    rc, ac = R.pileup([_read(10, [(2, "S"), (3, "M"), (2, "I"), (2, "M"), (3, "D"), (2, "M")], "GGACAGGCAAC")], 0, sites)
    #                 bases: SS=GG | M: A C A -> 10,11,12 | I: GG | M: C A -> 13,14 | D 15,16,17 | M: A C -> 18,19
    assert rc[:10] == [1, 0, 1, 0, 1, 0, 0, 0, 1, 0] and ac[:10] == [0, 1, 0, 1, 0, 0, 0, 0, 0, 1] and sum(rc[10:]) + sum(ac[10:]) == 0
    for op in "NHP=X":
        rc, ac = R.pileup([_read(10, [(3, "M"), (2, op), (3, "M")], "AAAAAAAA")], 0, sites)
        assert rc[:3] == [1, 1, 1] and sum(rc[3:]) == 0, op              # what was counted before the operation stays, nothing after it
        rc, ac = R.pileup([_read(10, [(2, op), (3, "M")], "AAAAA")], 0, sites)
        assert sum(rc) == 0, op                                            # e.g. a leading hard clip: nothing


def test_rule4_qualities_and_alleles():
    r = lambda q: _read(10, [(3, "M")], "ACA", qual=[30, q, 30])
    site = [V("c", 12, "C", "C")]
    assert R.pileup([r(19)], 0, site) == ([0], [0])
    assert R.pileup([r(20)], 0, site) == ([1], [1])                        # both counters when REF == ALT
    assert R.pileup([r(255)], 0, site) == ([1], [1])                       # 0xFF "missing" counts
    assert R.pileup([r(30)], 0, [V("c", 12, "c", "."), V("c", 12, "C", "G"), V("c", 12, "N", "C")]) == ([0, 1, 0], [0, 0, 1])      # chars compared exactly; duplicates each count


def test_rule5_sites_before_inside_after_the_read():
    sites = [V("c", p, "A", "C") for p in (10, 11, 14, 15)]                # 0-based 9 (before), 10 (first), 13 (last), 14 (behind)
    assert R.pileup([_read(10, [(4, "M")], "ACCA")], 0, sites) == ([0, 1, 1, 0], [0, 0, 0, 0])


def test_rule6_order_is_trusted_scan_pointer_never_goes_back():
    """the sequential form is what the restatement states: a read that lies before its predecessor does not get the sites the pointer has passed"""
    sites = [V("c", 11, "A", "C"), V("c", 101, "A", "C")]
    assert R.pileup([_read(100, [(1, "M")], "A"), _read(10, [(1, "M")], "A")], 0, sites) == ([0, 1], [0, 0])


def test_is_variant_site_and_texts():
    vs = [V("c", 5, "A", "T"), V("c", 6, "A", "T"), V("c", 7, "T", "A"), V("c", 8, ".", "A")]
    t, b = R.result_texts(vs, [0, 2, 1, 1], [0, 0, 2, 1], False)
    assert t == "#Chromosome\tPosition\tRef\tAlt\tCountRef\tCountAlt\nc\t6\tA\tT\t2\t0\nc\t7\tT\tA\t1\t2\nc\t8\t.\tA\t1\t1\n"
    assert b == "Chromosome,Position,BAF\nc,6,1\nc,7,0.666666666666667\n"
    t, b = R.result_texts(vs, [0, 2, 1, 1], [0, 0, 2, 1], True)
    assert t.count("\n") == 3 and "c\t6" not in t


def test_bam_round_trip(tmp_path):
    reads = [_read(5, [(2, "S"), (3, "M")], "ACGTN", name="x1", qual=[1, 2, 3, 4, 255]), _read(7, [(4, "M")], "GGCC", flag=0x10, mapq=7)]
    p = str(tmp_path / "a.bam")
    R.write_bam(p, [("c", 100)], reads, cut=17)
    refs, back = R.read_bam(p)
    assert refs == [("c", 100)]
    for a, b in zip(reads, back):
        assert all(b[k] == a[k] for k in ("pos", "cigar", "seq", "qual", "flag", "mapq")), (a, b)


def test_load_variants(tmp_path):
    p = str(tmp_path / "v.vcf")
    hdr = "##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\tS2\n"
    rows = ["b\t1\t.\tA\tC\t.\tPASS\t.\tGT\t0/1\t0/1", "c\t5\t.\tA\tC\t.\tPASS\t.\tGT:GQX\t0/1:40\t1/1:10", "c\t6\t.\tA\tC,G\t.\tPASS\t.\tGT\t0/1\t0/1",
            "c\t7\t.\tAT\tC\t.\tPASS\t.\tGT\t0/1\t0/1", "c\t8\t.\tA\tC\t.\tLowGQX\t.\tGT\t0/1\t0/1", "c\t9\t.\tA\tC\t.\tPASS\t.\tGT:FT\t0/1:q\t0/1:PASS",
            "c\t10\t.\tA\tC\t.\tPASS\t.\tGQX\t50\t50", "c\t11\t.\tA\tC\t.\tPASS\t.\tGT:GQX\t0|1:.\t0/0:50", "c\t12\t.\tA\tC\t.\tPASS\t.\tGT:GQX\t1|0:29.5\t1|1",
            "d\t1\t.\tA\tC\t.\tPASS\t.\tGT\t0/1\t0/1", "c\t13\t.\tA\tC\t.\tPASS\t.\tGT\t0/1\t0/1"]
    open(p, "w").write(hdr + "\n".join(rows) + "\n")
    pos = lambda **kw: [v.pos for v in R.load_variants(p, "c", **kw)]
    assert pos(sample_name="S1") == [5, 11, 12]                             # germline: het or hom alt of S1; stops at "d"
    assert pos(sample_name="S1", is_somatic=True) == [5]                    # GQX "." and 29.5 fail
    assert pos(sample_name="S2") == [5, 9, 12] and pos(sample_name="S2", is_somatic=True) == [9]
    with pytest.raises(ValueError):
        pos()
    with pytest.raises(ValueError):
        pos(sample_name="S3")
    q = str(tmp_path / "db.vcf")
    open(q, "w").write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\nc\t5\trs1\tA\tC\t.\t.\t.\nc\t6\trs2\tA\tCT\t.\t.\t.\n")
    assert [v.pos for v in R.load_variants(q, "c", is_dbsnp=True)] == [5]


# ---- the executable's conventions that need no device
def _run(*args):
    return subprocess.run([EXE] + list(args), capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def built():
    from canvas_amd import build
    build.build()
    assert os.path.exists(EXE)


def test_tool_usage_and_missing_files(built, tmp_path):
    for args in ([], ["-h"], ["-c", "chr1"], ["-o", "x"], ["-c", "chr1", "-o", "x", "--bogus"]):
        r = _run(*args)
        assert r.returncode == 0 and "Usage: CanvasSNV.exe" in r.stdout, args
    r = _run("-c", "c", "-o", str(tmp_path / "o"), "-v", str(tmp_path / "no.vcf"), "-b", str(tmp_path / "no.bam"))
    assert r.returncode == 1 and "no.vcf does not exist! Exiting." in r.stdout
    open(tmp_path / "v.vcf", "w").write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
    r = _run("-c", "c", "-o", str(tmp_path / "o"), "-v", str(tmp_path / "v.vcf"), "-b", str(tmp_path / "no.bam"))
    assert r.returncode == 1 and "no.bam does not exist! Exiting." in r.stdout


def test_tool_refusals_before_the_device(built, tmp_path):
    bam = str(tmp_path / "a.bam")
    R.write_bam(bam, [("c", 1000)], [_read(5, [(4, "M")], "ACGT")])
    one = str(tmp_path / "one.vcf"); two = str(tmp_path / "two.vcf")
    open(one, "w").write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\nc\t6\t.\tA\tC\t.\tPASS\t.\tGT\t0/1\n")
    open(two, "w").write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\tS2\nc\t6\t.\tA\tC\t.\tPASS\t.\tGT\t0/1\t0/1\n")
    out = str(tmp_path / "o.gz")
    r = _run("-c", "nochr", "-v", one, "-b", bam, "-o", out)
    assert r.returncode not in (0, 1) and "does not match bam file" in r.stderr
    r = _run("-c", "c", "-v", two, "-b", bam, "-o", out)
    assert r.returncode != 0 and ">1 samples" in r.stderr
    r = _run("-c", "c", "-v", two, "-b", bam, "-o", out, "-n", "S9")
    assert r.returncode != 0 and "corresponding to sample S9" in r.stderr
    for mode in ("histogram", "RegionHistogram"):
        r = _run("-c", mode, "-v", one, "-b", bam, "-o", out)
        assert r.returncode == 1 and "not supported" in r.stderr
    os.remove(bam + ".bai")
    r = _run("-c", "c", "-v", one, "-b", bam, "-o", out)
    assert r.returncode != 0 and "index not found" in r.stderr
    assert not os.path.exists(out)


def test_abi_lists_the_new_entry_points(built):
    import ctypes
    from canvas_amd.lib import ABI_SYMBOLS
    lib = ctypes.CDLL(os.path.join(ROOT, "canvas_amd", "libcanvas_hip.so"))
    hdr = open(os.path.join(ROOT, "include", "canvas_hip.h")).read()
    for name in ("canvas_snv_count", "canvas_memcpy_h2d_async"):
        assert name in ABI_SYMBOLS and hasattr(lib, name) and name + "(" in hdr
    assert lib.canvas_snv_count(None, None, 0, None, 0, 0, 0, 20, None, None, None, 0, None, None, None) == -1      # no context: CANVAS_ERR_INVALID
