"""CANVAS_TOOL_DEVICE_INFLATE=1: CanvasSNV, CanvasBin -c and CanvasBin -m Fragment read their BAM through canvas_bgzf_inflate instead of the host's zlib.  Every
output file, stdout, every stderr line that is no timing line, and the exit code must be what the same executable gives without the variable; the timing line tells
which way a run went.  The BAMs: a few thousand records, BGZF blocks written alternately at levels 0 and 6, an empty block (ISIZE 0) in the middle, chunks of 64 KiB,
so that records and blocks straddle chunks.  Damaged files (one corrupted deflate byte, a wrong ISIZE, a block of ISIZE 65536 without deflate data as a chunk of its own) must be refused in the same words."""
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import deflate_cases as D
import fragment_ref as F
import hits_ref as H
import snv_cases as SC
import snv_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "canvas_amd", "bin", "CanvasBin")
SNV = os.path.join(ROOT, "canvas_amd", "bin", "CanvasSNV")
REFS = [("chr1", 40_000), ("chr2", 30_000)]


@pytest.fixture(scope="module", autouse=True)
def built():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from canvas_amd import build
    build.build()


def write_bam(path, reads, writer):
    """`writer` (hits_ref.write_bam / snv_ref.write_bam) with blocks alternately stored (level 0) and deflated (level 6), then snv_ref.reblock_bam: an empty block in the
    middle and a subfield in front of BC"""
    count = [0]
    saved = R.bgzf_block

    def block(data):
        count[0] += 1
        co = zlib.compressobj(0 if count[0] % 2 else 6, zlib.DEFLATED, -15)
        c = co.compress(bytes(data)) + co.flush()
        return struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(c) + 25) + c + struct.pack("<II", zlib.crc32(bytes(data)) & 0xFFFFFFFF, len(data))
    R.bgzf_block = block
    try:
        writer(path + ".plain", REFS, reads)
    finally:
        R.bgzf_block = saved
    R.reblock_bam(path + ".plain", path)
    assert count[0] > 100 and R.bgzf_read_all(path + ".plain") == R.zlib_stream(open(path, "rb").read())


def damaged(bam, kind, tmp_path):
    """one block in the second half of chr1's records, refused by zlib either way"""
    raw = bytearray(open(bam, "rb").read())
    blocks = []
    at = 0
    while at < len(raw):
        xlen, = struct.unpack_from("<H", raw, at + 10)
        size = struct.unpack_from("<H", raw, at + 12 + xlen - 2)[0] + 1          # (reblock_bam puts BC last)
        blocks.append((at, 12 + xlen, size))
        at += size
    if kind == "no_deflate_data":      # chr1's first block (block 0 holds the header) gives way to one of ISIZE 65536 without a byte of data: with 64 KiB chunks a chunk of its own
        at, head, size = blocks[1]
        empty = bytearray(raw[at:at + head]) + struct.pack("<II", 0, 65536)
        struct.pack_into("<H", empty, head - 2, len(empty) - 1)
        raw[at:at + size] = empty
        blocks = []
    for at, head, size in blocks[len(blocks) // 4:]:
        isize, = struct.unpack_from("<I", raw, at + size - 4)
        if isize < 2000 or size - head - 8 > isize:                              # a deflated block (a stored one is longer than what it holds)
            continue
        if kind == "isize":
            struct.pack_into("<I", raw, at + size - 4, isize + 1)
        else:
            for k in range(at + head + 20, at + size - 8):
                raw[k] ^= 0x55
                if not D.zlib_verdict(bytes(raw[at + head:at + size - 8]), isize)[0]:
                    break
                raw[k] ^= 0x55
        assert not D.zlib_verdict(bytes(raw[at + head:at + size - 8]), struct.unpack_from("<I", raw, at + size - 4)[0])[0]
        break
    else:
        assert kind == "no_deflate_data", "no deflated block found"
    bad = str(tmp_path / ("%s_%s" % (kind, os.path.basename(bam))))
    open(bad, "wb").write(raw)
    open(bad + ".bai", "wb").write(open(bam + ".bai", "rb").read())
    return bad


def run(exe, args, outputs, device, chunk_var):
    env = dict(os.environ, CANVAS_TOOL_TIMING="1", CANVAS_TOOL_THREADS="16")
    env[chunk_var] = "65536"
    env.pop("CANVAS_TOOL_DEVICE_INFLATE", None)
    if device:
        env["CANVAS_TOOL_DEVICE_INFLATE"] = "1"
    for f in outputs:
        if os.path.exists(f):
            os.remove(f)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300, env=env)
    timing = [ln for ln in r.stderr.splitlines() if ln.startswith(("[snv]", "[bam]", "[frag]"))]
    messages = [ln for ln in r.stderr.splitlines() if not ln.startswith(("[", "{"))]
    files = [open(f, "rb").read() if os.path.exists(f) else None for f in outputs]
    files = [gzip.decompress(f) if f is not None and f[:2] == b"\x1f\x8b" else f for f in files]
    return r.returncode, r.stdout, messages, files, timing


def both(exe, args, outputs, chunk_var, ok=True):
    host = run(exe, args, outputs, False, chunk_var)
    dev = run(exe, args, outputs, True, chunk_var)
    assert dev[:4] == host[:4], (dev[:3], host[:3])
    assert (host[0] == 0) == ok, host[:3]
    for t, flag in ((host[4], 0), (dev[4], 1)):
        assert (t or not ok) and all(('"device_inflate": %d, "inflate_kernel_ms": ' % flag) in ln and ln.endswith("}") for ln in t), t
    if ok:
        assert all(f for f in host[3]) and all('"chunks": 1,' not in ln for ln in dev[4]), dev[4]
    return host, dev


# ---- CanvasBin -c
@pytest.fixture(scope="module")
def hits_sample(tmp_path_factory):
    d = tmp_path_factory.mktemp("inflate_hits")
    rng = np.random.RandomState(20261020)
    fa = str(d / "kmer.fa")
    with open(fa, "wb") as f:
        for name, ln in REFS:
            f.write(b">" + name.encode() + b"\n" + rng.choice(np.frombuffer(b"ACGTacgtn", np.uint8), ln).tobytes() + b"\n")
    reads = []
    for ri, (name, ln) in enumerate(REFS):
        for i, p in enumerate(np.sort(rng.randint(0, ln - 40, 3000))):
            flag = 0x1 | 0x40 | (0x2 if rng.rand() < 0.9 else 0) | (0x10 if rng.rand() < 0.3 else 0)
            reads.append(dict(ref=ri, pos=int(p), flag=flag, cigar=[(36, "M")], seq="A" * 36, tlen=int(rng.choice([-300, 0, 180, 333])), name="r%d" % i))
    bam = str(d / "S.bam")
    write_bam(bam, reads, H.write_bam)
    return d, fa, bam


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("mode", ["0", "3", "5"])
def test_canvasbin_observed_alignments(hits_sample, mode, paired):
    d, fa, bam = hits_sample
    out = str(d / "chr1.dat")
    host, dev = both(BIN, ["-b", bam, "-r", fa, "-c", "chr1", "-o", out, "-d", "100", "-m", mode] + (["-p"] if paired else []), [out], "CANVAS_BIN_CHUNK_BYTES")
    assert "Kept" in dev[1] and all('"host_path": 0' in ln for ln in dev[4])


# ---- CanvasBin -m Fragment
@pytest.fixture(scope="module")
def fragment_sample(tmp_path_factory):
    d = tmp_path_factory.mktemp("inflate_frag")
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
    bam = str(d / "pairs.bam")
    write_bam(bam, reads, H.write_bam)
    return d, fa, bed, bam


def test_canvasbin_fragment(fragment_sample):
    d, fa, bed, bam = fragment_sample
    out = str(d / "out.binned")
    host, dev = both(BIN, ["-b", bam, "-r", fa, "-n", bed, "-o", out, "-m", "Fragment", "-p"], [out], "CANVAS_BIN_CHUNK_BYTES")
    assert len(dev[4]) == 2 and all('"host_path": 0' in ln for ln in dev[4])


# ---- CanvasSNV
@pytest.fixture(scope="module")
def snv_sample(tmp_path_factory):
    d = tmp_path_factory.mktemp("inflate_snv")
    rng = np.random.RandomState(20261021)
    reads = []
    for i in range(len(REFS)):
        reads += SC.random_reads(rng, 3000, 25000, long_frac=0.02, exotic=0.05, ref=i)
    bam = str(d / "S.bam")
    write_bam(bam, reads, R.write_bam)
    vcf = str(d / "sites.vcf")
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.1\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\n")
        for c, _ in REFS:
            for p in np.sort(rng.randint(1, 25000, 2000)):
                a, b = rng.choice(list("ACGT"), 2, replace=False)
                f.write("%s\t%d\t.\t%s\t%s\t50\tPASS\t.\tGT\t0/1\n" % (c, p, a, b))
    return d, bam, vcf


def test_canvassnv(snv_sample):
    d, bam, vcf = snv_sample
    out = str(d / "chr1.txt.gz")
    host, dev = both(SNV, ["-c", "chr1", "-v", vcf, "-b", bam, "-o", out], [out, out + ".baf"], "CANVAS_SNV_CHUNK_BYTES")
    assert host[3][0].count(b"\n") > 100


# ---- damaged input
@pytest.mark.parametrize("kind", ["deflate_byte", "isize", "no_deflate_data"])
def test_damaged_bam_canvasbin(hits_sample, fragment_sample, tmp_path, kind):
    d, fa, bam = hits_sample
    out = str(tmp_path / "chr1.dat")
    host, dev = both(BIN, ["-b", damaged(bam, kind, tmp_path), "-r", fa, "-c", "chr1", "-o", out, "-d", "100", "-m", "3"], [out], "CANVAS_BIN_CHUNK_BYTES", ok=False)
    assert host[0] != 0 and (host[2] or kind == "no_deflate_data")      # (both say the same either way: `both`)
    if kind == "no_deflate_data":          # (the blocks behind it have moved: the .bai still finds chr1 and nothing else)
        return
    d, fa, bed, bam = fragment_sample
    out = str(tmp_path / "out.binned")
    host, dev = both(BIN, ["-b", damaged(bam, kind, tmp_path), "-r", fa, "-n", bed, "-o", out, "-m", "Fragment", "-p"], [out], "CANVAS_BIN_CHUNK_BYTES", ok=False)
    assert host[0] != 0 and host[2]


@pytest.mark.parametrize("kind", ["deflate_byte", "isize", "no_deflate_data"])
def test_damaged_bam_canvassnv(snv_sample, tmp_path, kind):
    d, bam, vcf = snv_sample
    out = str(tmp_path / "chr1.txt.gz")
    host, dev = both(SNV, ["-c", "chr1", "-v", vcf, "-b", damaged(bam, kind, tmp_path), "-o", out], [out, out + ".baf"], "CANVAS_SNV_CHUNK_BYTES", ok=False)
    assert host[0] != 0 and any("does not inflate to its recorded size" in m for m in host[2])
