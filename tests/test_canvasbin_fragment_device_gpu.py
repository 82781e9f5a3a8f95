"""CanvasBin -m Fragment counts its fragments through canvas_fragments_from_bam (chunks of raw record bytes, one call per chunk, names carried from chunk to chunk): the
.binned file, the printed lines and the exit code must be what the host loop gives — the same executable with the test hook CANVAS_TOOL_HOST_BAM — byte for byte.
The [frag] lines of CANVAS_TOOL_TIMING (stderr) tell which path a chromosome took."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import fragment_ref as F
import hits_ref as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "canvas_amd", "bin", "CanvasBin")
REFS = [("chr1", 50_000), ("chr2", 30_000), ("chr3", 10_000)]


@pytest.fixture(scope="module", autouse=True)
def built():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from canvas_amd import build
    build.build()


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    d = tmp_path_factory.mktemp("fragdev")
    rng = np.random.RandomState(3)
    fa = str(d / "genome.fa")
    with open(fa, "w") as f:
        for n, L in REFS:
            f.write(">%s\n" % n + rng.choice(np.frombuffer(b"ACGTn", np.uint8), L, p=[0.27, 0.2, 0.2, 0.27, 0.06]).tobytes().decode() + "\n")
    bins = {"chr1": [], "chr2": []}
    for n, L in REFS[:2]:
        p = 500
        while p + 900 < L:
            size = int(rng.randint(120, 800))
            bins[n].append((p, p + size))
            p += size + int(rng.choice([0, 0, 37, 400]))
    bed = str(d / "bins.bed")
    with open(bed, "w") as f:
        for n in ("chr2", "chr1"):                                   # BED order differs from the BAM's; chr2 has no GC column value (-1): PopulateBinGC
            for k, (a, b) in enumerate(bins[n]):
                f.write("%s\t%d\t%d\t%s\n" % (n, a, b, "-1" if n == "chr2" else str(40 + k % 20)))
    return d, fa, bed, bins


def random_pairs(rng, per_ref=6000):
    """the randomised two-chromosome sample of test_canvasbin_fragment_mode: duplicates / QC failures / low mapping quality on either mate, same-position mates,
    improper pairs, secondary records, unmapped mates, fragments between and across bins"""
    reads = []
    for ri, (n, L) in enumerate(REFS[:2]):
        for k in range(per_ref):
            pos = int(rng.randint(0, L - 700))
            tlen = int(rng.choice([0, 150, 300, 450, 600], p=[0.02, 0.2, 0.4, 0.28, 0.1]))
            mpos = pos + max(0, tlen - 36) if rng.rand() > 0.03 else pos
            f1 = f2 = 0x1 | 0x2
            u = rng.rand()
            if u < 0.05: f1 |= 0x400
            elif u < 0.10: f2 |= 0x400
            elif u < 0.13: f1 |= 0x200
            elif u < 0.16: f2 &= ~0x2
            elif u < 0.18: f1 |= 0x100
            elif u < 0.20: f2 |= 0x8
            q1, q2 = (int(rng.choice([0, 2, 3, 30, 60, 255], p=[0.03, 0.03, 0.04, 0.45, 0.42, 0.03])) for _ in range(2))
            name = "q%d_%d" % (ri, k)
            reads.append(F.rd(pos, name, f1 | 0x40, q1, mpos, tlen, ref=ri))
            reads.append(F.rd(mpos, name, f2 | 0x80 | 0x10, q2, pos, -tlen, ref=ri))
    reads.sort(key=lambda r: (r["ref"], r["pos"]))
    return reads


def run(args, host, chunk=65536):
    env = dict(os.environ, CANVAS_TOOL_TIMING="1", CANVAS_BIN_CHUNK_BYTES=str(chunk))
    env.pop("CANVAS_TOOL_HOST_BAM", None)
    if host:
        env.update(CANVAS_TEST_HOOKS="1", CANVAS_TOOL_HOST_BAM="1")
    r = subprocess.run([BIN] + args, capture_output=True, text=True, env=env)
    frag = [json.loads(line[len("[frag] "):]) for line in r.stderr.splitlines() if line.startswith("[frag] ")]
    messages = [line for line in r.stderr.splitlines() if not line.startswith(("[frag]", "[memory]", "{\"tool\""))]
    return r, frag, messages


def both(d, fa, bed, bam, tag):
    outs = []
    for host in (False, True):
        out = str(d / ("%s_%s.binned" % (tag, "host" if host else "dev")))
        r, frag, messages = run(["-b", bam, "-r", fa, "-n", bed, "-o", out, "-m", "Fragment", "-p"], host)
        data = gzip.open(out, "rb").read() if os.path.exists(out) else None
        outs.append((r.returncode, r.stdout.replace(out, "OUT"), messages, data, frag))
    dev, host = outs
    assert dev[:4] == host[:4], (dev[:3], host[:3])
    assert host[4] == []                                   # the host loop prints no [frag] line
    return dev


def test_randomised_sample_matches_the_host_loop(genome):
    d, fa, bed, bins = genome
    reads = random_pairs(np.random.RandomState(3))
    bam = str(d / "pairs.bam")
    H.write_bam(bam, REFS, reads)
    code, stdout, messages, data, frag = both(d, fa, bed, bam, "pairs")
    assert code == 0 and "Output complete" in stdout and data
    assert [f["chrom"] for f in frag] == ["chr1", "chr2"] and all(f["host_path"] == 0 and f["chunks"] >= 4 and f["carried_max"] > 0 for f in frag), frag
    # ... and what both wrote is what the restatement counts
    rows = data.decode().splitlines()
    exp = []
    for ri, n in enumerate(("chr1", "chr2")):
        counts, st = F.sequential([r for r in reads if r["ref"] == ri], ri, bins[n])
        assert st["usable"] > 500
        exp += ["%s\t%d\t%d\t%d.00" % (n, a, b, c) for (a, b), c in zip(bins[n], counts)]
    assert [row.rsplit("\t", 1)[0] for row in rows] == exp


def test_no_usable_fragments(genome):
    d, fa, bed, bins = genome
    reads = [F.rd(1000 + 10 * k, "lq%d" % k, 0x63, 30, 1200 + 10 * k, 240) for k in range(30)] + [F.rd(1200 + 10 * k, "lq%d" % k, 0x93, 1, 1000 + 10 * k, -240) for k in range(30)]
    reads.sort(key=lambda r: r["pos"])
    bam = str(d / "lowq.bam")
    H.write_bam(bam, REFS, reads)
    code, stdout, messages, data, frag = both(d, fa, bed, bam, "lowq")
    assert code == 1 and data is None and any("No passing-filter fragments" in m for m in messages)
    assert frag and frag[0]["host_path"] == 0


def test_unsorted_bam_gets_the_reference_message(genome):
    d, fa, bed, bins = genome
    reads = random_pairs(np.random.RandomState(5), per_ref=800)
    k = next(i for i, r in enumerate(reads) if r["ref"] == 0 and i > 900)
    reads[k]["pos"] = reads[k - 1]["pos"] - 5
    bam = str(d / "unsorted.bam")
    H.write_bam(bam, REFS, reads)
    code, stdout, messages, data, frag = both(d, fa, bed, bam, "unsorted")
    assert code == 1 and data is None and any("are not properly sorted" in m for m in messages)
    assert frag[0]["chrom"] == "chr1" and frag[0]["host_path"] == 1      # the device saw it (state[6]) and handed the chromosome back
