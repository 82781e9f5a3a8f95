"""Record streams for the framing tests, built from parts with struct.pack (no BAM library): records of chosen total length, records with hostile block_size
words, decoys (byte-exact record chains inside the aux bytes of real records), and random streams per rule.  Every case is (name, bytes, first)."""
import struct

import numpy as np

import frame_ref as FR

REF = 3                                   # the reference id of interest in every rule here
RULES = {"all": (FR.ALL, 0, 0, 0), "snv": (FR.SNV, REF, 0, 0), "hits": (FR.HITS, REF, 0, 0), "hits_paired_sorted": (FR.HITS, REF, 1, 1), "fragments": (FR.FRAGMENTS, REF, 0, 0)}
OPS = "MIDNSHP=X"
HEAD = 36 + 2 + 4                         # block_size, fixed fields, name "r" with its NUL, one CIGAR word: the shortest record rec() makes by default


def rec(ref=REF, pos=0, flag=0, mapq=30, name=b"r", cigar=((36, "M"),), l_seq=0, aux=b"", next_ref=-1, next_pos=-1, tlen=0, block_size=None, l_read_name=None, n_cigar=None,
        total=None):
    """one record with its block_size word.  total: zero aux bytes are added until the record has that many bytes.  block_size / l_read_name / n_cigar overwrite the
    field and leave the bytes alone."""
    var = (name + b"\0" if l_read_name != 0 or name else b"") + b"".join(struct.pack("<I", n << 4 | OPS.index(o)) for n, o in cigar) + bytes((max(l_seq, 0) + 1) // 2 + max(l_seq, 0)) + aux
    if total is not None:
        assert total >= 36 + len(var), (total, len(var))
        var += bytes(total - 36 - len(var))
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(name) + 1 if l_read_name is None else l_read_name, mapq, 0, len(cigar) if n_cigar is None else n_cigar, flag, l_seq,
                       next_ref, next_pos, tlen) + var
    return struct.pack("<i", len(body) if block_size is None else block_size) + body


def least(ref=REF, pos=0):
    """the minimum: block_size 32, no name, no CIGAR, no bases"""
    return rec(ref=ref, pos=pos, name=b"", l_read_name=0, cigar=())


def put(buf, at, blob, inside):
    """blob over buf[at:], which must lie inside the aux bytes of the record spanning `inside` = (start, end)"""
    assert inside[0] + HEAD <= at and at + len(blob) <= inside[1], (at, len(blob), inside)
    buf[at:at + len(blob)] = blob


def sorted_run(n, start=0, step=3, total=None, **kw):
    return [rec(pos=start + step * i, total=total, **kw) for i in range(n)]


def chunk_end_cases():
    r = rec(pos=5, total=100)
    three = b"".join(sorted_run(3, total=77))
    out = [("empty", b"", 0), ("first == nbytes", three, len(three))]
    out += [("%d bytes left" % k, three + r[:k], 0) for k in (1, 2, 3)]
    out += [("%d bytes left behind first" % k, three, len(three) - k) for k in (1, 2, 3)]
    out += [("one record ending at nbytes", r, 0), ("one record a byte short", r[:-1], 0), ("block_size word cut", three + r[:2], 0), ("fixed fields cut", three + r[:20], 0)]
    return out


def tile_cases(T):
    out = []
    out.append(("minimum records", b"".join(least(pos=i) for i in range(400)), 0))
    for res in range(4):
        out.append(("residue %d" % res, rec(total=HEAD + 2 + res) + b"".join(sorted_run(300, total=60)), 0))
    for k in (1, 2):
        for d in (-1, 0, 1):
            lead = rec(total=100) + rec(total=k * T + d - 100)
            out.append(("record starting at %dT%+d" % (k, d), lead + b"".join(sorted_run(120, start=10, total=81)), 0))
    out.append(("record ending at a tile end", rec(total=T - 50) + rec(total=50) + b"".join(sorted_run(20, total=64)), 0))
    out.append(("chunk ending at a tile end", rec(total=T - 50) + rec(total=50), 0))
    for tiles, extra in ((1, 10), (2, 77), (5, 1234)):
        out.append(("record longer than %d tiles" % tiles, b"".join(sorted_run(30, total=90)) + rec(pos=100, total=tiles * T + extra) + b"".join(sorted_run(40, start=200, total=90)), 0))
    out.append(("a chunk that is one record", rec(total=3 * T + 5), 0))
    big = b"".join(sorted_run(150, total=77))
    out.append(("first inside the last tile", big, len(b"".join(sorted_run(140, total=77)))))
    out.append(("20000 minimum records", b"".join(least(pos=i) for i in range(20000)), 0))
    return out


def decoy_cases(T):
    """-> [(name, bytes, first)]: in each, real record R starts in tile 0 and ends in the middle of tile 1; its aux bytes hold a decoy chain that starts 8 bytes behind
    the start of tile 1, in front of every true record start of that tile"""
    out = []
    lead = b"".join(sorted_run(10, total=100))
    Rlen, tail = T + 700 - len(lead), sorted_run(120, start=50, total=90)
    inside = (len(lead), len(lead) + Rlen)
    at = T + 8
    room = inside[1] - at                                       # bytes of R from the decoy's start to R's end

    def base():
        return bytearray(lead + rec(pos=40, total=Rlen) + b"".join(tail))
    # the chain runs past the tile's end: the last decoy claims bytes far behind R
    buf = base()
    put(buf, at, rec(total=120) + rec(total=120) + rec(total=120, block_size=T + 300), inside)
    out.append(("decoy chain past the tile's end", bytes(buf), 0))
    # the chain rejoins the true one at R's end
    buf = base()
    put(buf, at, rec(total=200) + rec(total=room - 200), inside)
    out.append(("decoy chain that rejoins", bytes(buf), 0))
    # never rejoins: from R's aux into a second decoy chain in the aux of a later real record, and so on to the tile's end
    big_tail = [rec(pos=50 + i, total=600) for i in range(12)]
    buf = bytearray(lead + rec(pos=40, total=Rlen) + b"".join(big_tail))
    starts = [inside[1] + 600 * i for i in range(12)]
    hop = at
    for i, s in enumerate(starts):
        land = s + HEAD + 10                                    # where the decoy in front of it has to arrive: inside real record i's aux
        span = (inside if i == 0 else (starts[i - 1], starts[i - 1] + 600))
        put(buf, hop, rec(total=60, block_size=land - hop - 4), span)
        hop = land
    put(buf, hop, rec(total=60), (starts[-1], starts[-1] + 600))
    out.append(("decoy chain that never rejoins", bytes(buf), 0))
    # in the first tile, in front of `first`: a chain from byte 0 that steps over `first`
    front = rec(total=150) + rec(total=150, block_size=150 - 4 + 8)
    buf = bytearray(front + b"".join(sorted_run(100, total=90)))
    out.append(("decoy in front of first", bytes(buf), len(front)))
    return out


def hostile_cases(T):
    out = []
    lead = b"".join(sorted_run(60, total=90))
    for what, bs in (("0", 0), ("31", 31), ("-1", -1), ("INT32_MIN", -(2 ** 31)), ("0x7FFFFFFF", 0x7FFFFFFF)):
        for behind in (b"", b"".join(sorted_run(5, start=500, total=90))):
            out.append(("block_size %s on the chain%s" % (what, ", records behind it" if behind else ""), lead + rec(pos=400, total=90, block_size=bs) + behind, 0))
    for d in (-1, 0, 1):
        last = rec(pos=400, total=90)
        out.append(("block_size nbytes - at - 4 %+d" % d, lead + struct.pack("<i", len(last) - 4 + d) + last[4:], 0))
    # the same words as decoys: at the start of tile 2, inside a real record's aux
    for what, bs in (("0", 0), ("31", 31), ("-1", -1), ("INT32_MIN", -(2 ** 31)), ("0x7FFFFFFF", 0x7FFFFFFF), ("to nbytes - 1", None), ("to nbytes", None), ("to nbytes + 1", None)):
        R = rec(pos=400, total=T)
        tail = b"".join(sorted_run(30, start=500, total=90))
        buf = bytearray(lead + R + tail)
        at = 2 * T + 4
        if bs is None:
            bs = len(buf) - at - 4 + {"to nbytes - 1": -1, "to nbytes": 0, "to nbytes + 1": 1}[what]
        put(buf, at, rec(total=80, block_size=bs), (len(lead), len(lead) + T))
        out.append(("decoy with block_size %s" % what, bytes(buf), 0))
    return out


def random_stream(seed, kind, n=2000, event=None, where=None):
    """n records that give the rule of `kind` no event, with everything mixed in that the rule lets pass; then `event` (a record) put at index `where`"""
    rng = np.random.RandomState(seed)
    flags = [0x1, 0x2, 0x4, 0x10, 0x100, 0x200, 0x400, 0x800]
    out, pos = [], 0
    for i in range(n):
        pos += int(rng.randint(0, 4))
        flag = sum(f for f in flags if rng.rand() < 0.15)
        cigar = [((34, "M"),), ((35, "M"),), ((35, "S"),), ((36, "M"), (3, "D"))][rng.randint(4)]
        ref, p = REF, pos
        if kind == FR.SNV and rng.rand() < 0.3:
            ref = REF - 1
        if kind == FR.HITS:
            filtered = not FR.passes_read_filters(struct.pack("<I", cigar[0][0] << 4 | OPS.index(cigar[0][1])), -36, dict(flag=flag, ncig=1, lname=0), False)      # (dropped unpaired: dropped paired as well)
            if filtered and rng.rand() < 0.5:                   # a record the filters drop may have any reference and position
                ref, p = int(rng.choice([-1, REF - 1, REF, REF + 1])), int(rng.choice([-1, 0, pos]))
        if kind == FR.ALL:
            ref, p = int(rng.choice([-1, REF - 1, REF, REF + 1])), int(rng.choice([-1, pos]))
        out.append(rec(ref=ref, pos=p, flag=flag, cigar=cigar, name=b"q%d" % i, l_seq=int(rng.randint(0, 40)), total=None, aux=bytes(rng.randint(0, 256, rng.randint(0, 30)).astype(np.uint8))))
    if event is not None:
        out.insert(where, event)
    return out


def events_of(kind):
    """[(what, record, event code)] that stop the rule of `kind` wherever they stand in a random_stream (pos 10**6 is behind every position of a stream)"""
    bad = [("block_size 20", rec(pos=10 ** 6, block_size=20), FR.EV_MALFORMED)]
    if kind == FR.ALL:
        return bad
    if kind == FR.SNV:
        return bad + [("unmapped", rec(ref=-1, pos=-1), FR.STOPPED), ("next reference", rec(ref=REF + 1, pos=0), FR.STOPPED), ("negative pos", rec(pos=-1), FR.STOPPED),
                      ("bases past block_size", rec(pos=10 ** 6, l_seq=50, block_size=60), FR.EV_MALFORMED)]
    fit = ("CIGAR past block_size", rec(pos=10 ** 6, n_cigar=5000), FR.EV_MALFORMED)
    if kind == FR.HITS:
        return bad + [fit, ("passing read of another reference", rec(ref=REF + 1, pos=0, flag=0x2), FR.STOPPED), ("passing unmapped reference", rec(ref=-1, pos=0, flag=0x2), FR.STOPPED)]
    return bad + [fit, ("another reference", rec(ref=REF + 1, pos=0), FR.STOPPED), ("filtered read of another reference", rec(ref=REF - 1, flag=0x4), FR.STOPPED)]
