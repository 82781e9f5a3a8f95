"""tests/hits_ref.py (the sequential restatement of CanvasBin's LoadObservedAlignmentsBAM that the GPU tests compare against) checked on the CPU: on the reference's own
BAM fixture, and against a second formulation that shares nothing with its loop — numpy over the filtered prefix (first stopping index, bincount clipped at 255, the
last record of every position for the fragment length)."""
import os

import numpy as np

import hits_ref as H
import snv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _vectorised(reads, ref_id, length, mode, paired_end):
    """the same answer from arrays: filter mask, first stopping index, counts over the prefix"""
    n = len(reads)
    flag = np.array([r.get("flag", 0) for r in reads], np.int64)
    ref = np.array([r["ref"] for r in reads], np.int64)
    pos = np.array([r["pos"] for r in reads], np.int64)
    tlen = np.array([r.get("tlen", 0) for r in reads], np.int64)
    first_m = np.array([bool(r["cigar"]) and r["cigar"][0][1] == "M" and r["cigar"][0][0] >= 35 for r in reads], bool)
    ok = ((flag & (0x4 | 0x200 | 0x400 | 0x10 | 0x100 | 0x800)) == 0) & first_m
    if paired_end:
        ok &= (flag & 0x2) != 0
    stops = np.flatnonzero(ok & (ref != ref_id))
    limit = int(stops[0]) if len(stops) else n
    kept = ok[:limit] & (ref[:limit] == ref_id)
    kp, kt = pos[:limit][kept], tlen[:limit][kept]
    inr = (kp >= 0) & (kp < length)
    cnt = np.bincount(kp[inr], minlength=length)[:length] if length else np.zeros(0, np.int64)
    hits = np.minimum(cnt, 1 if mode == H.MODE_BINARY else 255).astype(np.uint8)
    frag = None
    if mode == H.MODE_GCW:
        frag = np.zeros(length, np.int16)
        p, t = kp[inr][::-1], kt[inr][::-1]                        # the last record of every position: the first one of the reversed list
        u, first = np.unique(p, return_index=True)
        frag[u] = np.clip(t[first], 0, 32767)
    state = [1 if len(stops) else 0, limit + (1 if len(stops) else 0), int(kept.sum()), int((~inr).sum()), 0, int(kp[-1]) if len(kp) else 0]
    return hits, frag, state


def _random_reads(rng, n, length, nrefs=3, sorted_pos=True):
    reads = []
    for ref in range(nrefs):
        k = n // nrefs
        pos = rng.randint(-2, length + 2, k)
        if sorted_pos:
            pos = np.sort(pos)
        pile = int(rng.randint(0, max(1, length)))
        for i, p in enumerate(pos):
            flag = 0
            for bit, pr in ((0x1, 0.5), (0x2, 0.7), (0x4, 0.03), (0x10, 0.4), (0x100, 0.03), (0x200, 0.03), (0x400, 0.05), (0x800, 0.03)):
                if rng.rand() < pr:
                    flag |= bit
            u = rng.rand()
            cigar = [(36, "M")] if u < 0.8 else [(35, "M"), (1, "S")] if u < 0.85 else [(34, "M"), (2, "M")] if u < 0.9 else [(5, "S"), (31, "M")] if u < 0.95 else []
            reads.append(dict(ref=ref, pos=pile if i % 3 == 0 and ref == 1 else int(p), flag=flag, cigar=cigar, seq="A" * sum(k_ for k_, o in cigar if o in "MS"),
                              tlen=int(rng.choice([-7, 0, 150, 300, 32767, 40000]))))
        if sorted_pos:
            reads[-k:] = sorted(reads[-k:], key=lambda r: r["pos"])
    return reads


def test_restatement_agrees_with_the_vectorised_formulation():
    rng = np.random.RandomState(20261020)
    for trial in range(30):
        length = int(rng.choice([1, 7, 50, 400]))
        reads = _random_reads(rng, int(rng.choice([3, 90, 1500])), length)
        for ref_id in (0, 1, 2):
            start = next(i for i, r in enumerate(reads) if r["ref"] == ref_id)
            for mode in (H.MODE_BINARY, H.MODE_TDR, H.MODE_GCW):
                for paired in (False, True):
                    hits, frag, st = H.observed_alignments(reads[start:], ref_id, length, mode, paired)
                    vh, vf, vs = _vectorised(reads[start:], ref_id, length, mode, paired)
                    assert (hits == vh).all() and H.state_words(st) == vs, (trial, ref_id, mode, paired)
                    assert (frag is None and vf is None) or (frag == vf).all()
    assert hits.dtype == np.uint8


def test_saturation_and_chunks_carry_state():
    reads = [dict(ref=0, pos=3, flag=0, cigar=[(40, "M")], seq="A" * 40, tlen=100 + i) for i in range(300)] + [dict(ref=1, pos=0, flag=0, cigar=[(40, "M")], seq="A" * 40)] * 2
    whole = H.observed_alignments(reads, 0, 8, H.MODE_GCW)
    assert whole[0].tolist() == [0, 0, 0, 255, 0, 0, 0, 0] and whole[1][3] == 399 and H.state_words(whole[2]) == [1, 301, 300, 0, 0, 3]
    hits = frag = state = None
    for a, b in ((0, 100), (100, 100), (100, 301), (301, 302)):
        hits, frag, state = H.observed_alignments(reads[a:b], 0, 8, H.MODE_GCW, False, hits, frag, state)
    assert (hits == whole[0]).all() and (frag == whole[1]).all() and state == whole[2]


def test_the_references_own_bam():
    """CanvasTest/Data/single-end.bam: one hit per kept forward read, counted by a reader and a filter written apart from hits_ref (the SAM specification's field
    offsets, the flag bits spelled out)"""
    import struct
    bam = os.path.join(ROOT, "tests", "golden", "ref_data", "single-end.bam")
    refs, reads = H.read_bam(bam)
    buf = R.bgzf_read_all(bam)
    at = 12 + struct.unpack_from("<i", buf, 4)[0]
    for name, _ in refs:
        at += 8 + len(name) + 1
    raw = []
    while at < len(buf):
        bs, ref, pos, lname, _mq, _bin, ncig, flag = struct.unpack_from("<iiiBBHHH", buf, at)
        c0 = struct.unpack_from("<I", buf, at + 36 + lname)[0] if ncig else None
        raw.append((ref, pos, flag, c0, struct.unpack_from("<i", buf, at + 32)[0]))
        at += 4 + bs
    assert len(raw) == len(reads) == 9
    for ref_id, (name, length) in enumerate(refs):
        mine = [i for i, r in enumerate(reads) if r["ref"] == ref_id]
        if not mine:
            continue
        hits, frag, st = H.observed_alignments(reads[mine[0]:], ref_id, length, H.MODE_GCW)
        want = np.zeros(length, np.int64)
        seen = 0
        for ref, pos, flag, c0, tlen in raw[mine[0]:]:
            seen += 1
            forward_main = not flag & 4 and not flag & 16 and not flag & 256 and not flag & 512 and not flag & 1024 and not flag & 2048
            if forward_main and c0 is not None and c0 & 15 == 0 and c0 >> 4 >= 35:
                if ref != ref_id:
                    break
                want[pos] += 1
        assert (hits == np.minimum(want, 255)).all() and st["seen"] == seen and st["kept"] == int(want.sum()) and int(hits.sum()) == st["kept"]
        assert all(r["tlen"] == t[4] for r, t in zip(reads, raw))
