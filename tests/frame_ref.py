"""Plain Python restatement of the record framing of the executables: the loop of BamChunkLoop::run over the block_size chain (canvas_amd/tools/tool_common.hpp)
and the three `frame` callables it is given (CanvasSNV's pileup, CanvasBin -c, CanvasBin -m Fragment), one record after the other, every decision in the order the
C++ makes it.  canvas_bam_frame and canvas_amd/csrc/bam_frame.hpp are compared with this; it shares no code with either."""
import struct

ALL, SNV, HITS, FRAGMENTS = 0, 1, 2, 3
TAKE, SKIP, TAKE_AND_STOP, STOP, MALFORMED, UNSORTED = 0, 1, 2, 3, 4, 5
NONE, STOPPED, EV_MALFORMED, EV_UNSORTED, CAPACITY = 0, 1, 2, 3, 4
INT32_MIN = -(2 ** 31)


def fixed(buf, at):
    """BamFixed::decode of the record whose block_size word stands at `at`"""
    ref, pos, lname, mapq, _bin, ncig, flag, lseq, nref, npos, tlen = struct.unpack_from("<iiBBHHHiiii", buf, at + 4)
    return dict(ref=ref, pos=pos, lname=lname, mapq=mapq, ncig=ncig, flag=flag, lseq=lseq, nref=nref, npos=npos, tlen=tlen)


def passes_read_filters(buf, at, f, paired_end):
    """canvas_bin_main.cpp: passes_read_filters"""
    if f["flag"] & 0x4:
        return False
    if f["flag"] & 0x200:
        return False
    if f["flag"] & 0x400:
        return False
    if f["flag"] & 0x10:
        return False
    if f["flag"] & 0x900:
        return False
    if f["ncig"] == 0:
        return False
    c0, = struct.unpack_from("<I", buf, at + 36 + f["lname"])
    if (c0 & 0xF) != 0 or (c0 >> 4) < 35:
        return False
    if paired_end and not f["flag"] & 0x2:
        return False
    return True


class Tool:
    """one tool's `frame` callable with the variable it keeps between records: -> TAKE / SKIP / TAKE_AND_STOP / STOP / MALFORMED / UNSORTED"""

    def __init__(self, rule, state):
        self.kind, self.ref, self.paired, self.sorted = rule
        self.passed, self.last = state[0], state[1]
        self.against = 0

    def compare(self, pos, floor):
        last = self.last if self.passed else floor
        if pos < last:
            self.against = last
            return UNSORTED
        self.last = pos
        self.passed += 1
        return TAKE

    def frame(self, buf, at, bs):
        f = fixed(buf, at)
        fit = 32 + f["lname"] + 4 * f["ncig"] <= bs
        if self.kind == ALL:
            return TAKE
        if self.kind == SNV:
            if f["lseq"] < 0 or 32 + f["lname"] + 4 * f["ncig"] + (f["lseq"] + 1) // 2 + f["lseq"] > bs:
                return MALFORMED
            if f["ref"] < 0 or f["pos"] < 0 or f["ref"] > self.ref:
                return STOP
            if f["ref"] != self.ref:
                return SKIP
            return self.compare(f["pos"], -1)
        if self.kind == HITS:
            if not fit:
                return MALFORMED
            if f["ref"] == self.ref and not self.sorted:
                return TAKE
            if not passes_read_filters(buf, at, f, self.paired):
                return TAKE
            if f["ref"] != self.ref:
                return TAKE_AND_STOP
            return self.compare(f["pos"], INT32_MIN)
        assert self.kind == FRAGMENTS
        if not fit:
            return MALFORMED
        return TAKE_AND_STOP if f["ref"] != self.ref else TAKE


def frame(buf, first, rule, state=None, capacity=None, nbytes=None):
    """-> (offsets, info[0..5], state[4] after the call, [(offset, class)] of the classified records).  The loop of BamChunkLoop::run from `at = first`."""
    n = len(buf) if nbytes is None else nbytes
    state = list(state) if state is not None else [0, 0, 0, 0]
    if n - first < 4:
        return [], [0, 0, first, NONE, -1, 0], state, []
    tool = Tool(rule, state)
    at, offs, seen, event, ev_off = first, [], [], NONE, -1
    while at + 4 <= n:
        bs, = struct.unpack_from("<i", buf, at)
        if bs >= 32 and bs > n - at - 4:
            break                                            # completed by the next chunk
        cls = MALFORMED if bs < 32 else tool.frame(buf, at, bs)
        seen.append((at, cls))
        if cls in (MALFORMED, UNSORTED):
            event, ev_off = (EV_MALFORMED if cls == MALFORMED else EV_UNSORTED), at
            break
        if cls == STOP:
            event, ev_off = STOPPED, at
            break
        if cls != SKIP:
            offs.append(at)
        at += 4 + bs
        if cls == TAKE_AND_STOP:
            event, ev_off = STOPPED, at - 4 - bs
            break
    info = [len(seen), len(offs), at, event, ev_off, tool.against]
    if capacity is not None and len(offs) > capacity:
        info[3] = CAPACITY
        return [], info, state, seen
    return offs, info, [tool.passed, tool.last if tool.passed else state[1], state[2] + len(offs), event], seen
