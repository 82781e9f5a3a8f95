"""The CanvasDiploidCaller executable end to end on the GPU: the VCF (plain text and BGZF, compared after decompression) and <stem>.CoverageAndVariantFrequency.txt byte
for byte against the Python restatement of the readers, the caller and the writers (tests/diploid_ref.py: files_from_text), with and without a ploidy VCF and a -s file."""
import gzip
import json
import os
import subprocess

import pytest

import diploid_cases as DC
import diploid_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from canvas_amd import build
    build.build()
    return [e for e in build.build_more_tools() if os.path.basename(e) == "CanvasDiploidCaller"][0]


def version():
    import ctypes
    from canvas_amd.lib import load_library
    lib = load_library(); lib.canvas_version.restype = ctypes.c_char_p
    return lib.canvas_version().decode()


def write_inputs(tmp, part, vaf, contigs, ploidy, gz):
    ref = tmp / "ref"; ref.mkdir()
    (ref / "GenomeSize.xml").write_text('<sequenceSizes genomeName="test">\n' + "".join(
        '\t<chromosome fileName="genome.fa" contigName="%s" totalBases="%d" isCircular="false" md5="x" ploidy="2" knownBases="%d" type="Chromosome" />\n' % (n, l, l) for n, l in contigs) + "</sequenceSizes>\n")
    p = tmp / ("s.partitioned" + (".gz" if gz else "")); v = tmp / "s.vaf"
    (gzip.open(p, "wt") if gz else open(p, "w")).write("".join(x + "\n" for x in part))
    v.write_text("".join(x + "\n" for x in vaf))
    pl = None
    if ploidy is not None:
        pl = tmp / "ploidy.vcf"
        rows = ["##fileformat=VCFv4.1", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1"]
        rows += ["%s\t%d\t.\tN\t<CNV>\t.\tPASS\tEND=%d\tCN\t%s" % (c, s, e, "." if k == 2 else k) for c, iv in ploidy.items() for s, e, k in iv]
        pl.write_text("".join(r + "\n" for r in rows))
    return ref, p, v, pl


@pytest.mark.parametrize("seed,gz,with_ploidy", [(1, False, False), (2, True, True)])
def test_files_equal_the_restatement(exe, tmp_path, seed, gz, with_ploidy):
    part, vaf, contigs, ploidy = DC.file_case(seed, with_ploidy)
    ref, p, v, pl = write_inputs(tmp_path, part, vaf, contigs, ploidy, gz)
    out = tmp_path / ("CNV.vcf.gz" if gz else "calls.vcf")
    b = (-4.5, 4.25, -6.0, -1.5) if with_ploidy else R.LOGISTIC_GERMLINE
    args = [exe, "-i", str(p), "-v", str(v), "-o", str(out), "-r", str(ref), "-n", "NA12878"]
    if with_ploidy:
        s = tmp_path / "q.json"; s.write_text(json.dumps({"LogisticGermlineIntercept": str(b[0]), "LogisticGermlineLogBinCount": b[1], "LogisticGermlineModelDistance": "%r" % b[2],
                                                          "LogisticGermlineDistanceRatio": b[3], "LogisticIntercept": "1"}))
        args += ["-p", str(pl), "-s", str(s), "-d"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    want_vcf, want_cov = R.files_from_text(part, vaf, contigs, version(), str(ref), "NA12878", ploidy, b)
    raw = open(out, "rb").read()
    if gz:
        assert raw[:4] == b"\x1f\x8b\x08\x04" and raw[12:14] == b"BC" and raw.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
        got_vcf = gzip.decompress(raw).decode()
    else:
        got_vcf = raw.decode()
    assert got_vcf.split("\n") == want_vcf.split("\n")
    cov = tmp_path / ("CNV.CoverageAndVariantFrequency.txt" if gz else "calls.vcf.CoverageAndVariantFrequency.txt")
    assert open(cov).read().split("\n") == want_cov.split("\n")
    records = [l for l in got_vcf.split("\n") if l and l[0] != "#"]
    assert len(records) > 20 and [l.split("\t")[0] for l in records] == sorted([l.split("\t")[0] for l in records], key=[c for c, _ in contigs].index)
    kinds = {l.split("\t")[2].split(":")[1] for l in records}
    assert {"GAIN", "LOSS", "REF"} <= kinds and any("L10kb" in l for l in records) and "##OverallPloidy=" in got_vcf


def test_empty_partitioned_writes_the_header_only(exe, tmp_path):
    part, vaf, contigs, _ = DC.file_case(3)
    ref, p, v, _ = write_inputs(tmp_path, [], vaf, contigs, None, False)
    out = tmp_path / "e.vcf"
    r = subprocess.run([exe, "-i", str(p), "-v", str(v), "-o", str(out), "-r", str(ref)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "No segments loaded" in r.stdout
    assert open(out).read() == R.files_from_text([], vaf, contigs, version(), str(ref))[0] and "##OverallPloidy" not in open(out).read()


def test_unsorted_or_unknown_input_exits_1(exe, tmp_path):
    part, vaf, contigs, _ = DC.file_case(4)
    ref, p, v, _ = write_inputs(tmp_path, part, vaf, contigs, None, False)
    run = lambda: subprocess.run([exe, "-i", str(p), "-v", str(v), "-o", str(tmp_path / "o.vcf"), "-r", str(ref)], capture_output=True, text=True, timeout=120)
    rows = [x for x in vaf if x.startswith("chrA")]
    v.write_text("".join(x + "\n" for x in rows[:10] + [rows[3]] + rows[10:]))
    r = run(); assert r.returncode == 1 and "not sorted" in r.stderr and rows[3].split("\t")[1] in r.stderr
    v.write_text("".join(x + "\n" for x in vaf + [rows[0]]))
    r = run(); assert r.returncode == 1 and "chrA comes back" in r.stderr
    v.write_text("".join(x + "\n" for x in vaf))
    p.write_text("".join(x + "\n" for x in part + [part[0]]))
    r = run(); assert r.returncode == 1 and "comes back" in r.stderr
    p.write_text("".join(x + "\n" for x in part + ["chrNowhere\t0\t1000\t100.00\t0"]))
    r = run(); assert r.returncode == 1 and "unknown chromosome 'chrNowhere'" in r.stderr
