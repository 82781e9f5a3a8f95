"""CANVAS_TOOL_DEVICE_FRAME=1: CanvasSNV, CanvasBin -c and CanvasBin -m Fragment inflate their BAM AND frame its records on the device (canvas_bgzf_inflate,
canvas_bam_frame).  Every output file, stdout, every stderr line that is no timing line, and the exit code must be what the same executable gives without the
variable; the timing line tells which way a run went.  BAMs of a few thousand records in chunks of 64 KiB (records and BGZF blocks straddle chunks, chr1 ends in the
middle of a chunk), written by the helpers of tests/test_tools_device_inflate_gpu.py: sorted; going backwards inside the chromosome; holding a record of
block_size 20; truncated inside a record; holding a record larger than a chunk."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import fragment_ref as F
import hits_ref as H
import snv_cases as SC
import snv_ref as R
import test_tools_device_inflate_gpu as TI

pytestmark = pytest.mark.gpu
BIN, SNV, REFS = TI.BIN, TI.SNV, TI.REFS
INPUTS = ["sorted", "backwards", "block_size_20", "truncated", "large_record"]


@pytest.fixture(scope="module", autouse=True)
def built():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from canvas_amd import build
    build.build()


def variant(reads, kind, passing=None):
    """`reads` (sorted by reference and position) with one thing changed; -> (reads, chromosome to ask for).  passing: the flag of the read that goes backwards (one
    that CanvasBin's read filters keep: a read they drop is not compared with anything)"""
    reads = [dict(r) for r in reads]
    mid = len([r for r in reads if r["ref"] == 0]) * 2 // 3
    if kind == "backwards":
        reads[mid]["pos"] = max(reads[mid - 40]["pos"] - 3, 0)
        assert reads[mid]["pos"] < reads[mid - 1]["pos"]
        if passing is not None:
            reads[mid]["flag"] = reads[mid - 1]["flag"] = passing
    elif kind == "block_size_20":
        reads[mid]["block_size"] = 20
    elif kind == "truncated":                                   # the last record of the file says it is longer than the file
        reads[-1]["block_size"] = len(H.encode_record(reads[-1])) - 4 + 50
        return reads, "chr2"
    elif kind == "large_record":                                # 100 000 bytes behind the qualities: longer than a chunk, shorter than the buffers
        reads[mid]["tail"] = bytes(100000)
    return reads, "chr1"


def run(exe, args, outputs, device, chunk_var):
    env = dict(os.environ, CANVAS_TOOL_TIMING="1", CANVAS_TOOL_THREADS="16")
    env[chunk_var] = "65536"
    for v in ("CANVAS_TOOL_DEVICE_INFLATE", "CANVAS_TOOL_DEVICE_FRAME"):
        env.pop(v, None)
    if device:
        env["CANVAS_TOOL_DEVICE_FRAME"] = "1"
    for f in outputs:
        if os.path.exists(f):
            os.remove(f)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300, env=env)
    timing = [ln for ln in r.stderr.splitlines() if ln.startswith(("[snv]", "[bam]", "[frag]"))]
    messages = [ln for ln in r.stderr.splitlines() if not ln.startswith(("[", "{"))]
    files = [open(f, "rb").read() if os.path.exists(f) else None for f in outputs]
    files = [gzip.decompress(f) if f is not None and f[:2] == b"\x1f\x8b" else f for f in files]
    return r.returncode, r.stdout, messages, files, timing


def both(exe, args, outputs, chunk_var):
    host = run(exe, args, outputs, False, chunk_var)
    dev = run(exe, args, outputs, True, chunk_var)
    assert dev[:4] == host[:4], (dev[:3], host[:3])
    assert (host[4] and dev[4]) or host[0] != 0, (host[2], dev[2])      # (CanvasSNV prints no timing line for a file it refuses)
    assert all('"device_frame": 0, "frame_kernel_ms": ' in ln and '"device_inflate": 0' in ln and ln.endswith("}") for ln in host[4]), host[4]
    assert all('"device_frame": 1, "frame_kernel_ms": ' in ln and '"device_inflate": 1' in ln and ln.endswith("}") for ln in dev[4]), dev[4]
    return host, dev


@pytest.fixture(scope="module")
def hits_reads():
    rng = np.random.RandomState(20261021)
    reads = []
    for ri, (name, ln) in enumerate(REFS):
        for i, p in enumerate(np.sort(rng.randint(0, ln - 40, 3000))):
            flag = 0x1 | 0x40 | (0x2 if rng.rand() < 0.9 else 0) | (0x10 if rng.rand() < 0.3 else 0)
            reads.append(dict(ref=ri, pos=int(p), flag=flag, cigar=[(36, "M")], seq="A" * 36, tlen=int(rng.choice([-300, 0, 180, 333])), name="r%d" % i))
    return reads


@pytest.fixture(scope="module")
def kmer_fa(tmp_path_factory):
    rng = np.random.RandomState(4)
    fa = str(tmp_path_factory.mktemp("frame_fa") / "kmer.fa")
    with open(fa, "wb") as f:
        for name, ln in REFS:
            f.write(b">" + name.encode() + b"\n" + rng.choice(np.frombuffer(b"ACGTacgtn", np.uint8), ln).tobytes() + b"\n")
    return fa


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("mode", ["3", "5"])
def test_canvasbin_observed_alignments(hits_reads, kmer_fa, tmp_path, mode, kind):
    reads, chrom = variant(hits_reads, kind, passing=0x43)
    bam = str(tmp_path / "S.bam")
    TI.write_bam(bam, reads, H.write_bam)
    out = str(tmp_path / "chr.dat")
    host, dev = both(BIN, ["-b", bam, "-r", kmer_fa, "-c", chrom, "-o", out, "-d", "100", "-m", mode, "-p"], [out], "CANVAS_BIN_CHUNK_BYTES")
    handed_back = kind in ("block_size_20", "truncated") or (kind == "backwards" and mode == "5")
    assert all(('"host_path": %d' % handed_back) in ln for ln in dev[4] + host[4]), (dev[4], host[4])
    if kind in ("sorted", "large_record"):
        assert host[0] == 0 and "Kept" in dev[1] and all('"chunks": 1,' not in ln for ln in dev[4])


@pytest.fixture(scope="module")
def fragment_inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("frame_frag")
    rng = np.random.RandomState(5)
    fa = str(d / "genome.fa")
    with open(fa, "w") as f:
        for n, L in REFS:
            f.write(">%s\n" % n + rng.choice(np.frombuffer(b"ACGTn", np.uint8), L, p=[0.27, 0.2, 0.2, 0.27, 0.06]).tobytes().decode() + "\n")
    bed = str(d / "bins.bed")
    with open(bed, "w") as f:
        for n, L in REFS:
            for k, a in enumerate(range(500, L - 900, 450)):
                f.write("%s\t%d\t%d\t%d\n" % (n, a, a + 400, 40 + k % 20))
    reads = []
    for ri, (n, L) in enumerate(REFS):
        for k in range(2000):
            pos = int(rng.randint(0, L - 700))
            tlen = int(rng.choice([0, 150, 300, 450]))
            mpos = pos + max(0, tlen - 36)
            reads.append(F.rd(pos, "q%d_%d" % (ri, k), 0x63, int(rng.choice([2, 30, 60])), mpos, tlen, ref=ri))
            reads.append(F.rd(mpos, "q%d_%d" % (ri, k), 0x93, 30, pos, -tlen, ref=ri))
    reads.sort(key=lambda r: (r["ref"], r["pos"]))
    return fa, bed, reads


@pytest.mark.parametrize("kind", INPUTS)
def test_canvasbin_fragment(fragment_inputs, tmp_path, kind):
    fa, bed, base = fragment_inputs
    reads, chrom = variant(base, kind)
    bam = str(tmp_path / "pairs.bam")
    TI.write_bam(bam, reads, H.write_bam)
    out = str(tmp_path / "out.binned")
    host, dev = both(BIN, ["-b", bam, "-r", fa, "-n", bed, "-o", out, "-m", "Fragment", "-p"], [out], "CANVAS_BIN_CHUNK_BYTES")
    if kind in ("sorted", "large_record"):
        assert host[0] == 0 and len(dev[4]) == 2 and all('"host_path": 0' in ln for ln in dev[4])


@pytest.fixture(scope="module")
def snv_inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("frame_snv")
    rng = np.random.RandomState(20261022)
    reads = []
    for i in range(len(REFS)):
        reads += SC.random_reads(rng, 3000, 25000, long_frac=0.02, exotic=0.05, ref=i)
    vcf = str(d / "sites.vcf")
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.1\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\n")
        for c, _ in REFS:
            for p in np.sort(rng.randint(1, 25000, 2000)):
                a, b = rng.choice(list("ACGT"), 2, replace=False)
                f.write("%s\t%d\t.\t%s\t%s\t50\tPASS\t.\tGT\t0/1\n" % (c, p, a, b))
    return reads, vcf


@pytest.mark.parametrize("kind", INPUTS)
def test_canvassnv(snv_inputs, tmp_path, kind):
    base, vcf = snv_inputs
    reads, chrom = variant(base, kind)
    bam = str(tmp_path / "S.bam")
    TI.write_bam(bam, reads, R.write_bam)
    out = str(tmp_path / "chr.txt.gz")
    host, dev = both(SNV, ["-c", chrom, "-v", vcf, "-b", bam, "-o", out], [out, out + ".baf"], "CANVAS_SNV_CHUNK_BYTES")
    words = {"backwards": "is not sorted by position: read '", "block_size_20": "malformed alignment record (block_size 20)", "truncated": "the file ends inside an alignment record"}
    if kind in words:
        assert host[0] != 0 and any(words[kind] in m for m in dev[2]), dev[2]
    else:
        assert host[0] == 0 and host[3][0].count(b"\n") > 100
