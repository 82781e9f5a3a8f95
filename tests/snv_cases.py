"""Inputs of the CanvasSNV tests: raw-record chunks from read dicts, and seeded random reads / sites (tests/test_snv_gpu.py, tests/test_snv_tool_gpu.py, tools/soak_snv.py)."""
import numpy as np

import snv_ref as R

PAD = 1 << 16


def chunk_of(reads, pad=0):
    """records back to back -> (uint8 array with `pad` zero bytes behind the records, int64 offsets, bytes of records)"""
    blobs = [R.encode_record(r) for r in reads]
    offs = np.zeros(len(blobs), np.int64)
    at = 0
    for i, b in enumerate(blobs):
        offs[i] = at
        at += len(b)
    buf = np.zeros(at + pad, np.uint8)
    if at:
        buf[:at] = np.frombuffer(b"".join(blobs), np.uint8)
    return buf, offs, at


def random_cigar(rng, length, exotic=0.0):
    """a CIGAR that consumes exactly `length` read bases (S at the ends, M / I / D inside; with probability `exotic` one operation of N H P = X somewhere)"""
    ops = []
    left = length
    if rng.rand() < 0.3 and left > 10:
        k = int(rng.randint(1, 8)); ops.append((k, "S")); left -= k
    tail = None
    if rng.rand() < 0.3 and left > 10:
        k = int(rng.randint(1, 8)); tail = (k, "S"); left -= k
    while left > 0:
        k = int(min(left, rng.randint(1, max(2, length // 2)))); ops.append((k, "M")); left -= k
        if left > 0:
            t = rng.rand()
            if t < 0.4:
                k = int(min(left, rng.randint(1, 5))); ops.append((k, "I")); left -= k
                if left == 0:
                    ops.append((1, "D"))          # keeps I from being last before the tail (any order is legal for the walk; this one is common)
            elif t < 0.8:
                ops.append((int(rng.randint(1, 12)), "D"))
    if tail:
        ops.append(tail)
    if rng.rand() < exotic:
        op = "NHP=X"[rng.randint(5)]
        at = int(rng.randint(0, len(ops) + 1))
        ln = int(rng.randint(1, 20))
        if op in "=X":          # = and X consume read bases: take them from the sequence's budget so that l_seq still covers the CIGAR
            for j, (k, o) in enumerate(ops):
                if o == "M" and k > ln:
                    ops[j] = (k - ln, "M"); break
            else:
                op = "N"
        ops.insert(at, (ln, op))
    return ops


def random_reads(rng, n, span, lengths=(35, 300), long_frac=0.0, exotic=0.05, ref=0):
    """n reads sorted by position over [0, span)"""
    pos = np.sort(rng.randint(0, max(1, span), n))
    reads = []
    for p in pos:
        L = int(rng.randint(1200, 3000)) if rng.rand() < long_frac else int(rng.randint(lengths[0], lengths[1] + 1))
        seq = "".join("ACGTN="[i] for i in rng.choice(6, L, p=[0.28, 0.22, 0.22, 0.26, 0.01, 0.01]))
        qual = rng.choice([2, 19, 20, 30, 37, 255], L, p=[0.05, 0.05, 0.1, 0.4, 0.38, 0.02]).tolist()
        flag = 0
        for bit, pr in ((0x100, 0.03), (0x4, 0.03), (0x400, 0.05), (0x200, 0.03), (0x800, 0.03), (0x10, 0.5), (0x1, 0.5)):
            if rng.rand() < pr:
                flag |= bit
        reads.append(dict(ref=ref, pos=int(p), flag=flag, mapq=int(rng.choice([0, 1, 5, 6, 30, 60])), cigar=random_cigar(rng, L, exotic), seq=seq, qual=qual,
                          name="q%d" % len(reads)))
    return reads


def random_sites(rng, span, every, chrom="c"):
    """sorted sites, one per `every` bases on average (every = 1: each base), some duplicated, alleles mostly ACGT with the odd '.', lower case, N"""
    if every <= 1:
        pos = np.arange(1, span + 1)
    else:
        pos = np.sort(rng.randint(1, span + 1, max(1, span // every)))
    if len(pos) > 4:
        dup = rng.choice(len(pos), max(1, len(pos) // 50))
        pos = np.sort(np.concatenate([pos, pos[dup]]))
    al = ["A", "C", "G", "T", "A", "C", "G", "T", "A", "C", "G", "T", "N", ".", "a", "=", "R"]
    return [R.Variant(chrom, int(p), al[rng.randint(len(al))], [al[rng.randint(len(al))]]) for p in pos]
