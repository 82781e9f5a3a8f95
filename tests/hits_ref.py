"""Plain Python restatement of CanvasBin's LoadObservedAlignmentsBAM (CanvasBin/CanvasBin.cs:235-272) over decoded records, which the hits_from_bam tests compare
against: the read loop record by record, in file order, with the reference's filters in the reference's order, the `break` at the first passing record of another
reference, the saturating byte count and the fragment length of the last kept read of a position.  BAM building and framing come from tests/snv_ref.py (which shares
no code with canvas_amd/); its record encoder leaves tlen at 0, so the records are encoded and decoded here with that one field added."""
import struct

import numpy as np

import snv_ref as R

MODE_BINARY, MODE_TDR, MODE_GCW = 0, 3, 5
STATE_WORDS = ("stopped", "seen", "kept", "out_of_range", "malformed", "last_pos")


_snv_encode_record = R.encode_record


def encode_record(r):
    """snv_ref.encode_record with r['tlen'] written into the template-length field (byte 28 of the fixed fields)"""
    blob = bytearray(_snv_encode_record(r))
    struct.pack_into("<i", blob, 32, int(r.get("tlen", 0)))
    return bytes(blob)


def decode_record(buf, at):
    r, nxt = R.decode_record(buf, at)
    r["tlen"] = struct.unpack_from("<i", buf, at + 32)[0]
    return r, nxt


def write_bam(path, refs, reads, cut=3000):
    """snv_ref.write_bam with the records encoded by encode_record above (template lengths in place); snv_ref's own encoder is put back afterwards"""
    saved = R.encode_record
    R.encode_record = encode_record
    try:
        R.write_bam(path, refs, reads, cut)
    finally:
        R.encode_record = saved


def read_bam(path):
    """-> ([(name, length)], [record dict with tlen] in file order)"""
    buf = R.bgzf_read_all(path)
    assert buf[:4] == b"BAM\x01"
    ltext = struct.unpack_from("<i", buf, 4)[0]
    at = 8 + ltext
    nref = struct.unpack_from("<i", buf, at)[0]
    at += 4
    refs = []
    for _ in range(nref):
        ln = struct.unpack_from("<i", buf, at)[0]
        refs.append((buf[at + 4:at + 4 + ln - 1].decode(), struct.unpack_from("<i", buf, at + 4 + ln)[0]))
        at += 8 + ln
    reads = []
    while at < len(buf):
        r, at = decode_record(buf, at)
        reads.append(r)
    return refs, reads


def chunk_of(reads, pad=0, extra_offsets=()):
    """records back to back -> (uint8 array with `pad` zero bytes behind the records, int64 offsets, bytes of records).  extra_offsets: (index, offset) pairs of
    offsets that point at no record's start, inserted at that index of the offset list (negative offsets count from the end of the record bytes)."""
    blobs = [encode_record(r) for r in reads]
    offs, at = [], 0
    for b in blobs:
        offs.append(at)
        at += len(b)
    for idx, o in sorted(extra_offsets):
        offs.insert(idx, o if o >= 0 else at + o)
    buf = np.zeros(at + pad, np.uint8)
    if at:
        buf[:at] = np.frombuffer(b"".join(blobs), np.uint8)
    return buf, np.array(offs, np.int64), at


def damaged_records(rd):
    """[(what, record, last_only)]: records whose fixed fields do not describe bytes of the chunk, built with the caller's record builder `rd(pos, **fields)`.
    last_only: damaged only as the LAST record of a chunk without padding (in front of other records its block_size stays inside the chunk)."""
    past = rd(9)
    past["block_size"] = len(encode_record(past)) - 4 + 1
    return [
        ("block_size 31", rd(9, block_size=31), False),
        ("block_size past the chunk", past, True),
        ("name and CIGAR past block_size", rd(9, n_cigar=60000), False),
        ("name past block_size", rd(9, l_read_name=255, cigar=[], seq=""), False),
        ("negative block_size", rd(9, block_size=-8), False),
    ]


def stray_offsets(nbytes):
    """[(what, offset)]: offsets that leave no 36 bytes inside a chunk of `nbytes` (negative ones count from its end, as in chunk_of)"""
    return [("nbytes - 20", -20), ("nbytes - 35", -35), ("nbytes", nbytes), ("nbytes + 1", nbytes + 1), ("2^63 - 1", 2 ** 63 - 1)]


def new_state():
    return dict(stopped=0, seen=0, kept=0, out_of_range=0, malformed=0, last_pos=0)


def passes_filters(r, paired_end):
    """CanvasBin.cs:239-262, the checks in front of the reference-id comparison"""
    flag = r.get("flag", 0)
    if flag & 0x4:                  # !IsMapped
        return False
    if flag & 0x200:                # IsFailedQC
        return False
    if flag & 0x400:                # IsDuplicate
        return False
    if flag & 0x10:                 # IsReverseStrand
        return False
    if flag & 0x900:                # !IsMainAlignment
        return False
    cigar = r["cigar"]
    if r.get("n_cigar", len(cigar)) == 0 or not cigar:
        return False
    length, op = cigar[0]
    if op != "M" or length < 35:
        return False
    if paired_end and not flag & 0x2:
        return False
    return True


def observed_alignments(reads, ref_id, length, mode=MODE_TDR, paired_end=False, hits=None, frag=None, state=None):
    """The read loop over `reads` (one chunk, or a whole chromosome) in file order.  A record with r['malformed'] set stands for bytes that are no record: seen,
    counted, skipped.  hits / frag / state carry over from the chunk before (created when None).  -> (hits uint8[length], frag int16[length] or None, state dict)"""
    if hits is None:
        hits = np.zeros(length, np.uint8)
    if frag is None and mode == MODE_GCW:
        frag = np.zeros(length, np.int16)
    if state is None:
        state = new_state()
    for r in reads:
        if state["stopped"]:
            break
        state["seen"] += 1
        if r.get("malformed"):
            state["malformed"] += 1
            continue
        if not passes_filters(r, paired_end):
            continue
        if r["ref"] != ref_id:
            state["stopped"] = 1
            break
        if r["ref"] == -1:
            continue
        state["kept"] += 1
        pos = r["pos"]
        state["last_pos"] = pos
        if pos < 0 or pos >= length:            # the reference throws IndexOutOfRangeException
            state["out_of_range"] += 1
            continue
        if mode == MODE_BINARY:
            hits[pos] = 1
        elif hits[pos] < 255:
            hits[pos] += 1
        if mode == MODE_GCW:
            frag[pos] = max(min(32767, r.get("tlen", 0)), 0)
    return hits, frag, state


def state_words(state):
    return [int(state[k]) for k in STATE_WORDS]
