"""The drop-in CanvasSNV executable (canvas_amd/bin/CanvasSNV) against the restatement (tests/snv_ref.py): both output files byte for byte (the counts file after
gunzip), on synthetic BAM + VCF pairs, on the reference's own aligner output (tests/golden/ref_data/single-end.bam), and in the chain
CanvasSNV per chromosome -> concatenation -> CanvasPartition -m Wavelets -v."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import snv_ref as R
import snv_cases as SC
from gpu_common import get_canvas

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "canvas_amd", "bin", "CanvasSNV")
PARTITION = os.path.join(ROOT, "canvas_amd", "bin", "CanvasPartition")
GOLDEN_BAM = os.path.join(ROOT, "tests", "golden", "ref_data", "single-end.bam")
VCF_HEAD = "##fileformat=VCFv4.1\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"


def _run(args, env=None, exe=EXE):
    e = dict(os.environ, CANVAS_TOOL_THREADS="16")
    e.update(env or {})
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=e)


def _outputs(out):
    return gzip.open(out, "rt").read(), open(str(out) + ".baf").read()


def _check(tmp_path, vcf, bam, chrom, extra=(), env=None, **ref_kw):
    get_canvas()
    out = tmp_path / ("out_%s.txt.gz" % chrom)
    for f in (out, str(out) + ".baf"):
        if os.path.exists(f):
            os.remove(f)
    r = _run(["-c", chrom, "-v", vcf, "-b", bam, "-o", out] + list(extra), env)
    assert r.returncode == 0, r.stdout + r.stderr
    exp = R.run(str(vcf), str(bam), chrom, **ref_kw)
    got = _outputs(out)
    assert got[0] == exp[0] and got[1] == exp[1]
    return exp


def _genome(seed, n_per_ref=4000, span=30000):
    rng = np.random.RandomState(seed)
    refs = [("chrA", span + 5000), ("chrB", span + 5000), ("chrC", span + 5000)]
    reads = []
    for i in (0, 1):                                            # chrC has no reads
        reads += SC.random_reads(rng, n_per_ref, span, long_frac=0.02, exotic=0.05, ref=i)
    reads += [dict(ref=-1, pos=-1, flag=4, mapq=0, cigar=[], seq="ACGT", qual=[30] * 4, name="u%d" % i) for i in range(5)]
    return rng, refs, reads


def _write_vcf(path, rng, chroms, span, every, samples=("S1",), genotypes=True, gz=False):
    lines = [VCF_HEAD.rstrip("\n"), "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO" + ("\tFORMAT\t" + "\t".join(samples) if genotypes else "")]
    al = "ACGT"
    for c in chroms:
        pos = np.sort(rng.randint(1, span, span // every))
        for p in pos:
            ref = al[rng.randint(4)]; alt = al[rng.randint(4)]
            t = rng.rand()
            if t < 0.05:
                alt = alt + "," + al[rng.randint(4)]
            elif t < 0.1:
                ref = ref + "T"
            elif t < 0.12:
                alt = "."
            elif t < 0.14:
                ref = ref.lower()
            row = [c, str(int(p)), ".", ref, alt, "50", "PASS" if rng.rand() < 0.9 else "LowGQX", "."]
            if genotypes:
                fmt = "GT:GQX:FT" if rng.rand() < 0.5 else ("GT:GQX" if rng.rand() < 0.7 else ("GT" if rng.rand() < 0.8 else "GQX"))
                row.append(fmt)
                for _ in samples:
                    v = {"GT": ["0/1", "1/0", "0|1", "1|0", "1/1", "1|1", "0/0", "./.", "1/2"][rng.randint(9)], "GQX": [".", "12", "29.9", "30", "45", "99"][rng.randint(6)],
                         "FT": "PASS" if rng.rand() < 0.85 else "LowDP"}
                    row.append(":".join(v[k] for k in fmt.split(":")))
            lines.append("\t".join(row))
    text = "\n".join(lines) + "\n"
    if gz:
        with gzip.open(path, "wt") as f:
            f.write(text)
    else:
        open(path, "w").write(text)


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    d = tmp_path_factory.mktemp("snv")
    rng, refs, reads = _genome(20261016)
    bam = str(d / "S.bam")
    R.write_bam(bam, refs, reads)
    one = str(d / "one.vcf"); two = str(d / "two.vcf.gz"); db = str(d / "dbsnp.vcf")
    _write_vcf(one, rng, ["chrA", "chrB", "chrC"], 33000, 12)
    _write_vcf(two, rng, ["chrA", "chrB", "chrC"], 33000, 12, samples=("S1", "S2"), gz=True)
    _write_vcf(db, rng, ["chrA", "chrB", "chrC"], 33000, 12, genotypes=False)
    return dict(bam=bam, one=one, two=two, db=db)


def test_germline_plain_vcf(synthetic, tmp_path):
    for chrom in ("chrA", "chrB", "chrC"):
        exp = _check(tmp_path, synthetic["one"], synthetic["bam"], chrom)
        assert (exp[0].count("\n") > 100) == (chrom != "chrC")                 # real work on the chromosomes that have reads; chrC: header lines only


def test_many_chunks_give_the_same_files(synthetic, tmp_path):
    _check(tmp_path, synthetic["one"], synthetic["bam"], "chrB", env={"CANVAS_SNV_CHUNK_BYTES": "65536"})


def test_bgzf_forms_give_the_same_files(synthetic, tmp_path):
    """BGZF blocks with a subfield in front of BC and an empty block in the middle of the file (records span blocks in both): the files of the plainly written BAM"""
    get_canvas()
    other = str(tmp_path / "other_form.bam")
    R.reblock_bam(synthetic["bam"], other)
    got = []
    for tag, bam in (("plain", synthetic["bam"]), ("other", other)):
        out = tmp_path / (tag + ".txt.gz")
        r = _run(["-c", "chrB", "-v", synthetic["one"], "-b", bam, "-o", out])
        assert r.returncode == 0, r.stdout + r.stderr
        got.append((open(out, "rb").read(), open(str(out) + ".baf", "rb").read()))
    assert got[1] == got[0] and got[0][1].count(b"\n") > 100


def test_somatic_dbsnp_sample_name_and_mapq(synthetic, tmp_path):
    _check(tmp_path, synthetic["one"], synthetic["bam"], "chrA", ["-s"], is_somatic=True)
    _check(tmp_path, synthetic["db"], synthetic["bam"], "chrA", ["-i"], is_dbsnp=True)
    _check(tmp_path, synthetic["one"], synthetic["bam"], "chrA", ["-i"], is_dbsnp=True)
    _check(tmp_path, synthetic["two"], synthetic["bam"], "chrB", ["-n", "S2"], sample_name="S2")
    _check(tmp_path, synthetic["two"], synthetic["bam"], "chrB", ["--sampleName=S1", "--isSomatic"], sample_name="S1", is_somatic=True)
    _check(tmp_path, synthetic["one"], synthetic["bam"], "chrB", ["-q", "5"], min_mapq=5)
    _check(tmp_path, synthetic["one"], synthetic["bam"], "chrB", ["-q", "29", "-s"], min_mapq=29, is_somatic=True)


def test_reference_aligner_output(tmp_path):
    """tests/golden/ref_data/single-end.bam: the VCF is derived from the restatement's own reading of the file — sites where reads disagree, sites without coverage,
    sites on soft-clipped and deleted bases"""
    refs, reads = R.read_bam(GOLDEN_BAM)
    assert reads
    for ref_id, (chrom, length) in enumerate(refs):
        mine = [r for r in reads if r["ref"] == ref_id]
        if not mine:
            continue
        pos = set()
        for r in mine:
            p = r["pos"]
            span = sum(k for k, o in r["cigar"] if o in "MD=XN")
            pos.update(range(max(1, p - 2), p + span + 4))                    # every base of the read (deleted and skipped ones included) and a margin without coverage
        pos.update(range(1, min(length, 50)))
        pos = sorted(x for x in pos if 1 <= x <= length)
        al = "ACGT"
        vcf = str(tmp_path / ("derived_%d.vcf" % ref_id))
        with open(vcf, "w") as f:
            f.write(VCF_HEAD + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n")
            for i, p in enumerate(pos):
                for k in range(2):                                            # two allele pairs per position: whatever the reads carry matches somewhere
                    f.write("%s\t%d\t.\t%s\t%s\t.\tPASS\t.\tGT\t0/1\n" % (chrom, p, al[(i + k) % 4], al[(i + k + 1 + (i // 4) % 3) % 4]))
        exp = _check(tmp_path, vcf, GOLDEN_BAM, chrom)
        assert exp[0].count("\n") > 1, "the fixture's reads reach no site"


def test_baf_in_the_e_minus_05_decade(tmp_path):
    """1 reference read against 19 999 variant reads at one site: BAF = 1 / 20000 = 5E-05, where .NET's double.ToString() is already scientific (0.0001 is not);
    plus sites at 1 / 10001 and 2 / 20001 (both still in the E-05 decade) and one at exactly 0.0001"""
    rd = lambda p, seq: dict(ref=0, pos=p, flag=0, mapq=30, cigar=[(len(seq), "M")], seq=seq, qual=[30] * len(seq), name="d")
    # columns (0-based 100..103): site A: 1 A / 19999 T, site B: 1 A / 10000 T, site C: 2 A / 19999 T, site D: 1 A / 9999 T
    reads = [rd(100, "AAAA"), rd(100, "GGAG")]
    reads += [rd(100, "TTTT") for _ in range(9999)] + [rd(100, "TTTG") for _ in range(1)] + [rd(100, "TGTG") for _ in range(9999)] + [rd(100, "GGGG")]
    bam = str(tmp_path / "deep.bam"); vcf = str(tmp_path / "deep.vcf")
    R.write_bam(bam, [("chrD", 1000)], reads, cut=60000)
    open(vcf, "w").write(VCF_HEAD + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n" + "".join("chrD\t%d\t.\tA\tT\t.\tPASS\t.\tGT\t0/1\n" % p for p in (101, 102, 103, 104)))
    exp = _check(tmp_path, vcf, bam, "chrD")
    lines = exp[1].splitlines()
    assert lines[1] == "chrD,101,5E-05" and lines[2] == "chrD,102,9.99900009999E-05" and lines[3] == "chrD,103,9.99950002499875E-05" and lines[4] == "chrD,104,0.0001"


def test_refusals(synthetic, tmp_path):
    get_canvas()
    out = tmp_path / "o.gz"
    uns = str(tmp_path / "unsorted.vcf")
    open(uns, "w").write(VCF_HEAD + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\nchrA\t500\t.\tA\tC\t.\tPASS\t.\tGT\t0/1\nchrA\t400\t.\tA\tC\t.\tPASS\t.\tGT\t0/1\n")
    r = _run(["-c", "chrA", "-v", uns, "-b", synthetic["bam"], "-o", out])
    assert r.returncode == 1 and "chrA:400" in r.stderr and not os.path.exists(out)
    bam = str(tmp_path / "unsorted.bam")
    rd = lambda p, n: dict(ref=0, pos=p, flag=0, mapq=30, cigar=[(4, "M")], seq="ACGT", qual=[30] * 4, name=n)
    R.write_bam(bam, [("chrA", 10000)], [rd(100, "first"), rd(300, "second"), rd(200, "offender")])
    r = _run(["-c", "chrA", "-v", synthetic["one"], "-b", bam, "-o", out])
    assert r.returncode == 1 and "offender" in r.stderr and "chrA:201" in r.stderr
    r = _run(["-c", "histogram", "-v", synthetic["one"], "-b", synthetic["bam"], "-o", out])
    assert r.returncode == 1 and "not supported" in r.stderr
    r = _run(["-c", "RegionHistogram", "-v", tmp_path, "-b", tmp_path / "no_such_folder", "-o", out])          # the reference's arguments in these modes: folders, no BAM
    assert r.returncode == 1 and "not supported" in r.stderr and "does not exist" not in r.stdout
    # a truncated BAM: the host's framing refuses it
    raw = open(synthetic["bam"], "rb").read()
    for cut in (len(raw) // 2, len(raw) // 3 + 7):
        tb = str(tmp_path / ("trunc%d.bam" % cut))
        open(tb, "wb").write(raw[:cut]); open(tb + ".bai", "wb").write(open(synthetic["bam"] + ".bai", "rb").read())
        r = _run(["-c", "chrA", "-v", synthetic["one"], "-b", tb, "-o", out])
        assert r.returncode == 1 and ("truncated" in r.stderr or "BGZF" in r.stderr), r.stderr
    # a letter GetBAlleleFrequency does not know: the reference's ArgumentException
    nv = str(tmp_path / "n.vcf")
    open(nv, "w").write(VCF_HEAD + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n" + "".join("chrA\t%d\t.\tN\tA\t.\t.\t.\n" % p for p in range(1000, 1400)))
    r = _run(["-c", "chrA", "-v", nv, "-b", synthetic["bam"], "-o", out, "-i"])
    assert r.returncode not in (0, 1) and "Invalid single nucleotide allele: N" in r.stderr


def test_chain_into_canvas_partition(synthetic, tmp_path):
    """per chromosome CanvasSNV -> concatenated as CanvasRunner.ConcatenateCanvasSNVResults does -> CanvasPartition -m Wavelets -v: segments, and the same file as
    with a .vaf written by the restatement"""
    get_canvas()
    chroms = ["chrA", "chrB", "chrC"]
    parts, ref_parts = [], []
    for c in chroms:
        out = tmp_path / ("VF_%s.txt.gz" % c)
        r = _run(["-c", c, "-v", synthetic["one"], "-b", synthetic["bam"], "-o", out])
        assert r.returncode == 0, r.stderr
        parts.append(gzip.open(out, "rt").read())
        ref_parts.append(R.run(synthetic["one"], synthetic["bam"], c)[0])

    def concat(texts, path):
        with gzip.open(path, "wt") as w:
            header = False
            for t in texts:
                for line in t.splitlines():
                    if line.startswith("#"):
                        if header:
                            continue
                        header = True
                    w.write(line + "\n")
    vaf = str(tmp_path / "VFResults.txt.gz"); vaf_ref = str(tmp_path / "VFResults_ref.txt.gz")
    concat(parts, vaf); concat(ref_parts, vaf_ref)
    assert gzip.open(vaf, "rt").read() == gzip.open(vaf_ref, "rt").read()
    rng = np.random.RandomState(3)
    cleaned = str(tmp_path / "S.cleaned")
    with gzip.open(cleaned, "wt") as f:
        for c in chroms:
            level = 100.0
            for b in range(700):
                if b in (200, 450):
                    level = 160.0 if level == 100.0 else 100.0
                f.write("%s\t%d\t%d\t%.2f\t%d\n" % (c, b * 50, b * 50 + 50, level + rng.randn() * 3, 40 + b % 20))
    ref_dir = tmp_path / "WholeGenomeFasta"; ref_dir.mkdir()
    outs = []
    for v in (vaf, vaf_ref):
        o = str(tmp_path / ("S.partitioned_%d" % len(outs)))
        r = _run(["-i", cleaned, "-o", o, "-r", ref_dir, "-m", "Wavelets"] + (["-v", v] if v else []), exe=PARTITION)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(gzip.open(o, "rt").read().splitlines())
    assert outs[0] == outs[1] and len(outs[0]) == 2100
    assert len({ln.split("\t")[4] for ln in outs[0]}) >= 3                     # segments were derived: at least one per chromosome
