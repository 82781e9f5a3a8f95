"""CanvasBin -c reads the BAM through canvas_hits_from_bam (chunks of raw record bytes, inflated on the tool's threads): the intermediate file and the printed lines
must be what the host loop gives — the same executable with the test hook CANVAS_TOOL_HOST_BAM — byte for byte.  The [bam] line of CANVAS_TOOL_TIMING (stderr) tells
which path a run took."""
import os
import struct
import subprocess

import numpy as np
import pytest

import hits_ref as H
import snv_ref as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "canvas_amd", "bin", "CanvasBin")
REFS = [("chr1", 9001), ("chr2", 7000), ("chrNone", 500), ("chrX", 8003)]
M36 = [(36, "M")]


@pytest.fixture(scope="module", autouse=True)
def built():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from canvas_amd import build
    build.build()


def _reads(rng, refs, per_ref=2500, unmapped=40):
    reads = []
    for ri, (name, ln) in enumerate(refs):
        if name == "chrNone":
            continue
        pos = np.sort(rng.randint(0, ln - 40, per_ref))
        pos[:700] = pos[700]                                  # a pile-up that saturates the byte counter
        for i, p in enumerate(pos):
            u = rng.rand()
            flag, cigar = 0x1 | 0x2 | 0x40, M36
            if u < 0.30: flag |= 0x10
            elif u < 0.33: flag |= 0x400
            elif u < 0.35: flag |= 0x200
            elif u < 0.37: flag |= 0x100
            elif u < 0.39: flag |= 0x800
            elif u < 0.42: cigar = [(5, "S"), (31, "M")]
            elif u < 0.45: cigar = [(34, "M"), (2, "M")]
            elif u < 0.52: flag &= ~0x2
            reads.append(dict(ref=ri, pos=int(p), flag=flag, cigar=cigar, seq="A" * 36, tlen=int(rng.choice([-300, 0, 180, 333, 499, 40000])), name="r%d" % i))
    reads += [dict(ref=-1, pos=-1, flag=0x4 | 0x1, cigar=[], seq="A" * 36, name="u%d" % i) for i in range(unmapped)]
    return reads


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_device")
    rng = np.random.RandomState(20261022)
    fa = str(d / "kmer.fa")
    with open(fa, "wb") as f:
        for name, ln in REFS:
            f.write(b">" + name.encode() + b"\n" + rng.choice(np.frombuffer(b"ACGTacgtn", np.uint8), ln).tobytes() + b"\n")
    reads = _reads(rng, REFS)
    bam = str(d / "S.bam")
    H.write_bam(bam, REFS, reads)
    return d, fa, bam, reads


def run_bin(bam, fa, chrom, out, mode, paired=False, host=False, chunk=None):
    env = dict(os.environ, CANVAS_TEST_HOOKS="1", CANVAS_TOOL_TIMING="1")
    env.pop("CANVAS_TOOL_HOST_BAM", None); env.pop("CANVAS_BIN_CHUNK_BYTES", None)
    if host:
        env["CANVAS_TOOL_HOST_BAM"] = "1"
    if chunk:
        env["CANVAS_BIN_CHUNK_BYTES"] = str(chunk)
    if os.path.exists(out):
        os.remove(out)
    r = subprocess.run([BIN, "-b", bam, "-r", fa, "-c", chrom, "-o", out, "-d", "100", "-m", mode] + (["-p"] if paired else []), capture_output=True, text=True, env=env)
    dat = open(out, "rb").read() if os.path.exists(out) else None
    bam_line = [ln for ln in r.stderr.splitlines() if ln.startswith("[bam]")]
    errors = [ln for ln in r.stderr.splitlines() if not ln.startswith(("[", "{"))]
    return r.returncode, r.stdout, dat, bam_line, errors


def same_both_ways(bam, fa, chrom, out, mode, paired=False, chunk=None, device_expected=True):
    host = run_bin(bam, fa, chrom, out, mode, paired, host=True)
    dev = run_bin(bam, fa, chrom, out, mode, paired, chunk=chunk)
    assert host[0] == 0 and not host[3], host                          # the host loop has no [bam] line
    assert dev[0] == 0 and dev[1] == host[1] and dev[2] == host[2] and dev[2] is not None, (chrom, mode, paired, dev[1], host[1], dev[4])
    assert len(dev[3]) == 1 and ('"host_path": 0' in dev[3][0]) == device_expected, dev[3]
    return dev


@pytest.mark.parametrize("mode", ["0", "TruncatedDynamicRange", "GCContentWeighted"])
@pytest.mark.parametrize("paired", [False, True])
def test_device_path_gives_the_host_loops_file(sample, mode, paired):
    d, fa, bam, reads = sample
    for chrom in ("chr1", "chr2", "chrX"):                             # first, middle, last (followed by the unmapped reads)
        dev = same_both_ways(bam, fa, chrom, str(d / "out.dat"), mode, paired)
        ri = [n for n, _ in REFS].index(chrom)
        first = next(i for i, r in enumerate(reads) if r["ref"] == ri)
        _, _, st = H.observed_alignments(reads[first:], ri, REFS[ri][1], H.MODE_TDR, paired)
        assert "Kept %d of %d total reads" % (st["kept"], st["seen"]) in dev[1] and st["kept"] > 500
        if chrom == "chrX":
            assert st["seen"] == 2500 + 40 and st["stopped"] == 0      # every unmapped read behind the last chromosome is seen
    # a chromosome without reads: no line, no device work for the BAM
    host = run_bin(bam, fa, "chrNone", str(d / "out.dat"), mode, paired, host=True)
    dev = run_bin(bam, fa, "chrNone", str(d / "out.dat"), mode, paired)
    assert dev[:3] == host[:3] and dev[0] == 0 and "Kept" not in dev[1] and not dev[3]


@pytest.mark.parametrize("mode", ["3", "5"])
def test_small_chunks(sample, mode):
    """records of about 100 bytes, 2 500 per chromosome: chunks of 64 KiB cut each chromosome in four, with records spanning the cuts"""
    d, fa, bam, _ = sample
    for chrom in ("chr1", "chrX"):
        dev = same_both_ways(bam, fa, chrom, str(d / "small.dat"), mode, True, chunk=65536)
        assert '"chunks": 1,' not in dev[3][0]
        whole = run_bin(bam, fa, chrom, str(d / "small.dat"), mode, True)
        assert whole[2] == dev[2] and '"chunks": 1,' in whole[3][0]


def test_the_references_own_bam(tmp_path):
    bam = os.path.join(ROOT, "tests", "golden", "ref_data", "single-end.bam")
    refs, _ = H.read_bam(bam)
    L = dict(refs)["chrM"]
    fa = str(tmp_path / "kmer.fa")
    open(fa, "wb").write(b">chrM\n" + np.random.RandomState(4).choice(np.frombuffer(b"ACGTacgt", np.uint8), L).tobytes() + b"\n")
    for mode in ("0", "3", "5"):
        dev = same_both_ways(bam, fa, "chrM", str(tmp_path / "chrM.dat"), mode)
        assert "Kept 0 of 9 total reads" in dev[1]


def test_bgzf_forms(sample):
    d, fa, bam, _ = sample
    other = str(d / "other_form.bam")
    SR.reblock_bam(bam, other)
    for mode in ("3", "5"):
        a = same_both_ways(bam, fa, "chr2", str(d / "form.dat"), mode, True)
        b = same_both_ways(other, fa, "chr2", str(d / "form.dat"), mode, True)
        c = same_both_ways(other, fa, "chr2", str(d / "form.dat"), mode, True, chunk=65536)
        assert a[2] == b[2] == c[2]


def test_unsorted_mode5_takes_the_host_path(sample, tmp_path):
    d, fa, _, reads = sample
    mine = [dict(r) for r in reads]
    k = next(i for i, r in enumerate(mine) if r["ref"] == 1) + 700
    kept = []                                                       # kept records on strictly growing positions
    for i in range(k, k + 300):
        if H.passes_filters(mine[i], True) and (not kept or mine[i]["pos"] > mine[kept[-1]]["pos"]):
            kept.append(i)
    mine[kept[3]]["pos"], mine[kept[0]]["pos"] =mine[kept[0]]["pos"], mine[kept[3]]["pos"]          # one kept position goes backwards
    bam = str(tmp_path / "backwards.bam")
    H.write_bam(bam, REFS, mine)
    same_both_ways(bam, fa, "chr2", str(tmp_path / "b.dat"), "GCContentWeighted", True, device_expected=False)
    same_both_ways(bam, fa, "chr2", str(tmp_path / "b.dat"), "TruncatedDynamicRange", True)          # the counts do not depend on the order: the device path
    same_both_ways(bam, fa, "chr1", str(tmp_path / "b.dat"), "GCContentWeighted", True)               # chr1 stops before it gets there


@pytest.mark.parametrize("damage", ["cut_inside_a_block", "bsize_below_the_header", "cut_inside_a_record", "record_without_its_fixed_fields"])
def test_damaged_bam_is_refused_as_before(sample, tmp_path, damage):
    d, fa, bam, reads = sample
    raw = bytearray(open(bam, "rb").read())
    blocks = SR.bgzf_blocks(raw)
    at, size = blocks[5]                                            # block 0 is the header; chr1's records fill some eighty blocks
    bad = str(tmp_path / "damaged.bam")
    if damage == "cut_inside_a_block":
        raw = raw[:at + size // 2]
    elif damage == "bsize_below_the_header":
        struct.pack_into("<H", raw, at + 16, 10)
    elif damage == "cut_inside_a_record":
        raw = raw[:at]                                              # whole blocks, the last record unfinished (the stream is cut every 3000 bytes)
    if damage == "record_without_its_fixed_fields":
        broken = [dict(r) for r in reads[:1200]] + [dict(reads[1200], block_size=20)] + [dict(r) for r in reads[1201:]]
        H.write_bam(bad, REFS, broken)
    else:
        open(bad, "wb").write(raw)
        open(bad + ".bai", "wb").write(open(bam + ".bai", "rb").read())
    for mode in ("3", "5"):
        host = run_bin(bad, fa, "chr1", str(tmp_path / "chr1.dat"), mode, host=True)
        dev = run_bin(bad, fa, "chr1", str(tmp_path / "chr1.dat"), mode)
        assert dev[0] == host[0] and dev[1] == host[1] and dev[2] == host[2] and dev[4] == host[4], (dev, host)
        if damage == "cut_inside_a_record":                         # the host loop takes the end of the last whole block for the end of the file: so does this path
            assert dev[0] == 0 and dev[2] is not None and "Kept" in dev[1]
        else:
            assert dev[0] == 1 and dev[2] is None and any(bad in ln for ln in dev[4])
