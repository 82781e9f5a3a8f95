"""Two plain Python restatements of CanvasBin -m Fragment (CanvasBin/FragmentBinner.cs) over decoded records, which the fragments_from_bam tests compare against.
Records are the dicts of tests/hits_ref.py (encode_record writes name, mapq, mate_ref, mate_pos and tlen).

(a) sequential(): binFragments + BinOneAlignment + FindBestBin as written (FragmentBinner.cs:211-243,256-369): one loop over the records in file order with a dict
    (read name -> bin index), a set (names seen once with pos == mate pos) and the forward pointer binIndexStart.  It is chunk-aware: the state it returns goes into the
    call for the next chunk.  Where the reference throws on a position that goes backwards, the ordinal of the record is noted and the loop goes on (the counts are void).
(b) decomposed(): the records grouped by name, every group walked in file order as a two-variable state machine, the pointer located by binary search in the running
    maximum of Stop.  It shares nothing with (a) but the filters' definitions.

int arithmetic wraps at 32 bits, as unchecked C# does."""
import bisect

import numpy as np

STATE_WORDS = ("stopped", "seen", "paired", "usable", "malformed", "last_pos", "unsorted", "entries", "carry_bytes")
CARRY_HEADER_BYTES = 24           # frag.hip: one header per carried name, then the name bytes, rounded up to 8


def wrap32(v):
    return ((int(v) + 2 ** 31) % 2 ** 32) - 2 ** 31


def name_of(r):
    """the l_read_name - 1 bytes behind the fixed fields; l_read_name = 0 is the empty name"""
    raw = r.get("name", "r").encode() + b"\x00"
    return raw[:max(r.get("l_read_name", len(raw)) - 1, 0)]


def skipped(flag):
    """FragmentBinner.cs:258-265: !IsMapped, !IsMateMapped, !IsPrimaryAlignment, !(IsPaired && IsProperPair)"""
    return bool(flag & 0x4 or flag & 0x8 or flag & 0x100 or not (flag & 0x1 and flag & 0x2))


def is_bad(r, quality_threshold):
    """IsDuplicateFailedQCLowQuality (:321-332)"""
    flag, mapq = r.get("flag", 0), r.get("mapq", 30)
    return bool(flag & 0x400 or flag & 0x200 or mapq == 255 or mapq < quality_threshold)


def find_best_bin(bins, start_index, frag_start, frag_stop):
    """FindBestBin (:349-369)"""
    best, best_overlap = -1, 0
    for i in range(start_index, len(bins)):
        overlap = wrap32(min(bins[i][1], frag_stop) - max(bins[i][0], frag_start))
        if overlap <= 0:
            break
        if overlap > best_overlap:
            best_overlap, best = overlap, i
    return best


def carry_bytes(names):
    names = list(names)
    return CARRY_HEADER_BYTES * len(names) + (sum(len(n) for n in names) + 7) // 8 * 8 if names else 0


def new_state():
    return dict(stopped=0, seen=0, paired=0, usable=0, malformed=0, last_pos=0, unsorted=0, entries=0, carry_bytes=0, prev=-1, pointer=0, binned={}, same_pos=set())


def sequential(reads, ref_id, bins, quality_threshold=3, counts=None, state=None):
    """(a): one chunk (or a whole chromosome).  bins = [(start, stop)] in BED order.  -> (counts int32[nbins], state); state['binned'] / state['same_pos'] are the
    leftover dictionary and set."""
    if counts is None:
        counts = np.zeros(len(bins), np.int32)
    st = new_state() if state is None else state
    binned, same_pos = st["binned"], st["same_pos"]
    for r in reads:
        if st["stopped"]:
            break
        st["seen"] += 1
        if r.get("malformed"):
            st["malformed"] += 1
            continue
        if r["ref"] != ref_id:
            st["stopped"] = 1
            break
        pos = r["pos"]
        if pos < st["prev"] and not st["unsorted"]:      # the reference throws here
            st["unsorted"] = st["seen"]
        st["prev"] = st["last_pos"] = pos
        flag = r.get("flag", 0)
        if flag & 0x1:
            st["paired"] += 1
        if skipped(flag):
            continue
        name, bad = name_of(r), is_bad(r, quality_threshold)
        if name in binned:
            if bad:
                st["usable"] -= 1
                counts[binned[name]] -= 1
            del binned[name]
            continue
        if bad or r["ref"] != r.get("mate_ref", -1) or pos > r.get("mate_pos", -1):
            continue
        if pos == r.get("mate_pos", -1):
            if name in same_pos:
                same_pos.remove(name)
                continue
            same_pos.add(name)
        tlen = r.get("tlen", 0)
        if tlen == 0:
            continue
        frag_start, frag_stop = pos, wrap32(pos + tlen)
        while st["pointer"] < len(bins) and bins[st["pointer"]][1] <= frag_start:
            st["pointer"] += 1
        if st["pointer"] >= len(bins):
            continue
        best = find_best_bin(bins, st["pointer"], frag_start, frag_stop)
        if best >= 0:
            st["usable"] += 1
            counts[best] += 1
            binned[name] = best
    open_names = set(binned) | same_pos
    st["entries"], st["carry_bytes"] = len(open_names), carry_bytes(open_names)
    return counts, st


def state_words(st):
    return [int(st[k]) for k in STATE_WORDS]


def decomposed(chunks, ref_id, bins, quality_threshold=3):
    """(b): all chunks of a chromosome at once (sorted input).  -> (counts, usable, leftover dict, leftover set)"""
    live = []
    for reads in chunks:
        stop = False
        for r in reads:
            if r.get("malformed"):
                continue
            if r["ref"] != ref_id:
                stop = True
                break
            if not skipped(r.get("flag", 0)):
                live.append(r)
        if stop:
            break
    groups = {}
    for r in live:                                   # file order inside every group
        groups.setdefault(name_of(r), []).append(r)
    pref, run = [], -2 ** 31
    for _, stop in bins:
        run = max(run, stop)
        pref.append(run)
    counts, usable, left_binned, left_same = np.zeros(len(bins), np.int32), 0, {}, set()
    for name, recs in groups.items():
        b, same = -1, False
        for r in recs:
            bad = is_bad(r, quality_threshold)
            if b >= 0:
                if bad:
                    usable -= 1
                    counts[b] -= 1
                b = -1
                continue
            if bad or r["ref"] != r.get("mate_ref", -1) or r["pos"] > r.get("mate_pos", -1):
                continue
            if r["pos"] == r.get("mate_pos", -1):
                was, same = same, not same
                if was:
                    continue
            if r.get("tlen", 0) == 0:
                continue
            start = bisect.bisect_right(pref, r["pos"])          # the first bin whose running maximum of Stop exceeds the fragment's start
            if start >= len(bins):
                continue
            best = find_best_bin(bins, start, r["pos"], wrap32(r["pos"] + r["tlen"]))
            if best >= 0:
                usable += 1
                counts[best] += 1
                b = best
        if b >= 0:
            left_binned[name] = b
        if same:
            left_same.add(name)
    return counts, usable, left_binned, left_same


# ---- scenarios shared by the tests
def rd(pos, name="r", flag=0x3, mapq=30, mate_pos=None, tlen=0, ref=0, mate_ref=None, **kw):
    """one record: a proper pair on `ref` unless told otherwise (mate_pos defaults to pos + 50)"""
    d = dict(ref=ref, pos=pos, name=name, flag=flag, mapq=mapq, mate_ref=ref if mate_ref is None else mate_ref, mate_pos=pos + 50 if mate_pos is None else mate_pos,
             tlen=tlen, cigar=[(8, "M")], seq="ACGTACGT")
    d.update(kw)
    return d


def pair(name, pos, mate_pos, tlen=None, flags=(0x63, 0x93), mapqs=(30, 30)):
    """the two records of a pair (left, right), to be merged into a sorted stream"""
    tlen = mate_pos - pos + 8 if tlen is None else tlen
    return [rd(pos, name, flags[0], mapqs[0], mate_pos, tlen), rd(mate_pos, name, flags[1], mapqs[1], pos, -tlen)]


def random_bins(rng, n, span=4000):
    """n bins in BED-file order: shuffled, overlapping and nested ones among them"""
    bins = []
    for _ in range(n):
        s = int(rng.randint(0, span))
        bins.append((s, s + int(rng.randint(1, 400))))
    kind = rng.randint(3)
    if kind == 0:
        bins.sort()
    elif kind == 1:
        bins.sort()
        for k in range(0, len(bins) - 1, 5):              # a nested bin in front of its host
            s, e = bins[k + 1]
            bins[k] = (s + (e - s) // 4, max(s + (e - s) // 4 + 1, e - (e - s) // 4))
    return bins


def random_reads(rng, nnames, max_group=40, span=4000, other_ref_tail=0):
    """records of `nnames` names with 1 .. max_group records each, every flag / mapq / tlen class among them, sorted by position (stable), then `other_ref_tail`
    records of reference 1"""
    reads = []
    for k in range(nnames):
        name = "n%d" % k if rng.randint(8) else "n%d" % (k // 2)          # some names are shared by two generated groups
        size = 1 if rng.randint(5) == 0 else (2 if rng.randint(4) else int(rng.randint(1, max_group + 1)))
        base = int(rng.randint(0, span))
        for _ in range(size):
            pos = base + (0 if rng.randint(3) == 0 else int(rng.randint(0, 300)))
            mate = pos if rng.randint(6) == 0 else pos + int(rng.randint(-200, 300))
            flag = 0x3 | (int(rng.randint(0, 0x1000)) if rng.randint(4) == 0 else 0)
            if rng.randint(12) == 0:
                flag &= ~int(rng.choice([0x1, 0x2]))
            mapq = int(rng.choice([0, 2, 3, 30, 60, 254, 255]))
            tlen = 0 if rng.randint(10) == 0 else int(rng.randint(-300, 600))
            reads.append(rd(pos, name, flag, mapq, mate, tlen, mate_ref=0 if rng.randint(15) else 1))
    reads.sort(key=lambda r: r["pos"])
    for k in range(other_ref_tail):
        reads.append(rd(k, "tail%d" % k, ref=1))
    return reads
