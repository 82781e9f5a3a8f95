"""canvas_amd/bin/FlagUniqueKmers end to end: a folded, CRLF, soft-masked FASTA with descriptions in its headers goes in; the output must be, byte for byte, the layout
INTEGRATION.md fixes ('>' + name, the whole sequence on one line, '\\n' line ends) with the case tests/kmer_ref.py computes, and read back the way CanvasBin reads
kmer.fa (Canvas.mask_from_fasta) it must give the reference mask."""
import os
import subprocess

import numpy as np
import pytest

import kmer_cases as KC
import kmer_ref as R
from gpu_common import get_canvas, to_dev

pytestmark = pytest.mark.gpu
EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "canvas_amd", "bin", "FlagUniqueKmers")


def _genome():
    rng = np.random.RandomState(77)
    G = [bytes(g) for g in KC.planted_genome(seed=5, lengths=[300_000, 120_001, 60_000, 4_097], plants=160)]
    G.insert(2, b"")                                                       # an empty entry
    G.append(KC.rand_seq(rng, 30))                                         # shorter than a 35-mer
    G.append(G[1][1000:3000])                                              # a contig that repeats part of another
    soft = []
    for g in G:                                                            # soft-masked stretches: input case carries nothing
        a = np.frombuffer(g, np.uint8).copy()
        for _ in range(len(a) // 5000 + 1):
            if len(a) > 10:
                s0 = rng.randint(0, len(a) - 5); a[s0:s0 + rng.randint(1, 3000)] |= 0x20
        soft.append(a.tobytes())
    names = ["chr%d" % (i + 1) for i in range(len(soft))]
    return names, soft


def _write_fasta(path, names, seqs, width, eol, last_eol=True):
    with open(path, "wb") as f:
        for i, (n, s) in enumerate(zip(names, seqs)):
            desc = [b" AC:CM000%d.2  gi:568336\tHomo sapiens" % i, b"\tLN:%d" % len(s), b""][i % 3]
            f.write(b">" + n.encode() + desc + eol)
            lines = [s[k:k + width] for k in range(0, len(s), width)]
            body = eol.join(lines)
            f.write(body)
            if i + 1 < len(seqs) or last_eol:
                f.write(eol)


def _run(args):
    return subprocess.run([EXE] + args, capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def cv():
    return get_canvas()


def test_tool_end_to_end(cv, tmp_path):
    names, seqs = _genome()
    flags = R.unique_flags_numpy(seqs)
    want = R.render_fasta(names, seqs, flags)
    src = str(tmp_path / "genome.fa")
    _write_fasta(src, names, seqs, 60, b"\r\n", last_eol=False)
    out = str(tmp_path / "kmer.fa")
    r = _run([src, out])
    assert r.returncode == 0, r.stderr
    got = open(out, "rb").read()
    assert got == want
    total = sum(len(s) for s in seqs)
    assert "%d entries, %d positions" % (len(seqs), total) in r.stdout and "%d unique" % sum(int(f.sum()) for f in flags) in r.stdout
    # a tiny table: many passes, identical bytes
    out2 = str(tmp_path / "kmer_small_table.fa")
    r2 = _run([src, out2, "--table-gb", "0.0008"])
    assert r2.returncode == 0, r2.stderr
    assert open(out2, "rb").read() == want
    passes = int(r2.stdout.split(" passes")[0].split()[-1])
    assert passes >= 8, r2.stdout
    # unfolded input with '\n' line ends: the same output
    src3 = str(tmp_path / "genome_unfolded.fa")
    _write_fasta(src3, names, seqs, 1 << 30, b"\n")
    out3 = str(tmp_path / "kmer3.fa")
    assert _run([src3, out3]).returncode == 0
    assert open(out3, "rb").read() == want
    # the way CanvasBin reads kmer.fa: upper case = possible alignment
    entries = got.split(b">")[1:]
    assert len(entries) == len(seqs)
    for e, n, f in zip(entries, names, flags):
        head, seq, rest = e.split(b"\n")
        assert head == n.encode() and rest == b"" and len(seq) == len(f)
        if len(seq) == 0:
            continue
        d = to_dev(np.frombuffer(seq + b"\0" * ((-len(seq)) % 64), np.uint8), cv.device)
        m = cv.mask_from_fasta(d, len(seq)).cpu().numpy().view(np.uint64)
        assert (m == R.pack_mask(f)).all(), n
    # running the tool on its own output changes nothing
    out4 = str(tmp_path / "kmer4.fa")
    assert _run([out, out4]).returncode == 0
    assert open(out4, "rb").read() == want


def test_tool_fasta_forms_with_an_empty_first_entry(cv, tmp_path):
    """an empty entry FIRST, then contigs of a few thousand bases: one line per sequence with LF, folded at 60 with CRLF, folded with the last line lacking its line end"""
    rng = np.random.RandomState(78)
    names, seqs = ["chrNothing", "chrA", "chrB"], [b"", KC.rand_seq(rng, 3001), KC.rand_seq(rng, 2000)]
    want = R.render_fasta(names, seqs, R.unique_flags_numpy(seqs))
    for tag, width, eol, last_eol in (("single", 1 << 30, b"\n", True), ("crlf60", 60, b"\r\n", True), ("no_last_eol", 60, b"\n", False)):
        src = str(tmp_path / (tag + ".fa")); out = str(tmp_path / (tag + ".kmer.fa"))
        _write_fasta(src, names, seqs, width, eol, last_eol)
        r = _run([src, out])
        assert r.returncode == 0, r.stderr
        assert open(out, "rb").read() == want, tag


def test_tool_errors(tmp_path):
    src = str(tmp_path / "g.fa")
    open(src, "wb").write(b">a\n" + KC.rand_seq(np.random.RandomState(1), 500) + b"\n")
    r = _run([str(tmp_path / "missing.fa"), str(tmp_path / "o.fa")])
    assert r.returncode == 1 and "cannot read" in r.stderr
    r = _run([src, str(tmp_path / "no_such_dir" / "o.fa")])
    assert r.returncode == 1 and "cannot write" in r.stderr
    r = _run([src, str(tmp_path / "o.fa"), "--table-gb", "0.000000001"])          # one byte: no key class fits
    assert r.returncode == 1 and "largest key class" in r.stderr
    r = _run([src])
    assert r.returncode == 0 and r.stderr.splitlines() == ["Usage info:", "  FlagUniqueKmers $InputFASTA $OutputFASTA"]
