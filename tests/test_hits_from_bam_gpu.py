"""Canvas.hits_from_bam (canvas_amd/csrc/obs.hip) against the sequential restatement of CanvasBin's LoadObservedAlignmentsBAM (tests/hits_ref.py): every array
and every state word is compared exactly.  A workgroup of obs.hip takes 256 records (four waves of 64)."""
import numpy as np
import pytest

import hits_ref as H
from gpu_common import get_canvas, to_dev

pytestmark = pytest.mark.gpu
WG = 256
M36 = [(36, "M")]


@pytest.fixture(scope="module")
def cv():
    return get_canvas()


def rd(pos, ref=0, flag=0, cigar=M36, tlen=0, **kw):
    d = dict(ref=ref, pos=pos, flag=flag, cigar=cigar, seq="A" * sum(k for k, o in cigar if o in "MIS=X"), tlen=tlen)
    d.update(kw)
    return d


def gpu_run(cv, chunks, ref_id, length, mode, paired=False, hits0=None, frag0=None, pad=0, extra_offsets=None, want_info=True, tail=8):
    """the chunks one after the other through Canvas.hits_from_bam; hits / frag are allocated `tail` elements longer than `length` and those must stay as they were.
    -> (hits[length], frag[length] or None, last info or the state read back)"""
    import torch
    hits = torch.full((length + tail,), 7, dtype=torch.uint8, device=cv.device)
    hits[:length] = 0 if hits0 is None else to_dev(hits0, cv.device)
    frag = None
    if mode == H.MODE_GCW or frag0 is not None:
        frag = torch.full((length + tail,), -3, dtype=torch.int16, device=cv.device)
        frag[:length] = 0 if frag0 is None else to_dev(frag0, cv.device)
    state = torch.zeros(8, dtype=torch.int64, device=cv.device)
    info = None
    torch.cuda.synchronize()                       # torch filled the arrays on its own stream
    for k, reads in enumerate(chunks):
        buf, offs, nbytes = H.chunk_of(reads, pad, (extra_offsets or {}).get(k, ()))
        d_buf = to_dev(buf, cv.device) if len(buf) else torch.zeros(1, dtype=torch.uint8, device=cv.device)
        d_off = to_dev(offs, cv.device) if len(offs) else torch.zeros(0, dtype=torch.int64, device=cv.device)
        hits, frag, state, info = cv.hits_from_bam(d_buf, d_off, ref_id, length, mode, paired, hits, frag, state, nbytes=nbytes, want_info=want_info)
    if not want_info:
        cv.synchronize()
        info = state.cpu().numpy()
    h = hits.cpu().numpy()
    assert (h[length:] == 7).all(), "bytes behind hits[len - 1] changed"
    f = None
    if frag is not None:
        f = frag.cpu().numpy()
        assert (f[length:] == -3).all(), "values behind frag[len - 1] changed"
        f = f[:length]
    return h[:length], f, info


def check(cv, chunks, ref_id=0, length=64, mode=H.MODE_TDR, paired=False, hits0=None, ref_chunks=None, what="", **kw):
    """ref_chunks: what the restatement sees instead of `chunks` (stand-ins for bytes that are no record)"""
    eh = None if hits0 is None else hits0.copy()
    ef = est = None
    for reads in (ref_chunks or chunks):
        eh, ef, est = H.observed_alignments(reads, ref_id, length, mode, paired, eh, ef, est)
    if est is None:
        eh, ef, est = H.observed_alignments([], ref_id, length, mode, paired, eh)
    h, f, info = gpu_run(cv, chunks, ref_id, length, mode, paired, hits0=hits0, **kw)
    assert (h == eh).all(), (what, np.flatnonzero(h != eh)[:8], h[h != eh][:8], eh[h != eh][:8])
    if mode == H.MODE_GCW:
        assert (f == ef).all(), (what, np.flatnonzero(f != ef)[:8], f[f != ef][:8], ef[f != ef][:8])
    assert [int(x) for x in info[:6]] == H.state_words(est), (what, info, est)
    return h, f, info


MODES = (H.MODE_BINARY, H.MODE_TDR, H.MODE_GCW)


def test_filters(cv):
    bits = [0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x400, 0x800]
    flags = [0] + bits + [a | b for i, a in enumerate(bits) for b in bits[i + 1:]] + [0x900, 0xFFFF, 0xF6FB & ~0x14]
    for paired in (False, True):
        for mode in MODES:
            reads = [rd(5 + i % 50, flag=f, tlen=100 + i) for i, f in enumerate(flags)]
            _, _, info = check(cv, [reads], paired=paired, mode=mode, what="all flags")
            assert info[2] == sum(1 for f in flags if not f & 0xF14 and (f & 2 or not paired))
        for f in flags:
            check(cv, [[rd(9, flag=f, tlen=200)]], paired=paired, mode=H.MODE_GCW, what="flag %x paired %d" % (f, paired))
    cigars = [[(36, "S")], [(36, "I")], [(1, "S"), (35, "M")], [(34, "M")], [(35, "M")], [(34, "M"), (35, "M")], [(35, "M"), (1, "S")], [(100000, "M")], [(35, "="), (1, "M")], [(35, "D")]]
    for c in cigars:
        _, _, info = check(cv, [[rd(3, cigar=c, tlen=50)]], mode=H.MODE_GCW, what=str(c))
        assert info[2] == (1 if c[0][1] == "M" and c[0][0] >= 35 else 0)
    check(cv, [[rd(3, cigar=c, tlen=50 + i) for i, c in enumerate(cigars)]], mode=H.MODE_GCW)
    _, _, info = check(cv, [[rd(3, cigar=[]), rd(4), rd(5, cigar=[])]], what="n_cigar 0")
    assert info[1] == 3 and info[2] == 1
    for f, paired, kept in ((0x2, True, 1), (0x0, True, 0), (0x2, False, 1), (0x0, False, 1), (0x1, True, 0), (0x3, True, 1)):
        _, _, info = check(cv, [[rd(7, flag=f)]], paired=paired)
        assert info[2] == kept


def _mixed(rng, n, length, ref=0):
    pos = np.sort(rng.randint(0, length, n))
    out = []
    for i, p in enumerate(pos):
        u = rng.rand()
        flag = 0x1 | 0x2
        cigar = M36
        if u < 0.35: flag |= 0x10
        elif u < 0.40: flag |= 0x400
        elif u < 0.43: flag |= 0x200
        elif u < 0.46: flag |= 0x100
        elif u < 0.49: flag |= 0x800
        elif u < 0.52: flag |= 0x4
        elif u < 0.56: cigar = [(5, "S"), (31, "M")]
        elif u < 0.60: cigar = [(20, "M"), (2, "I"), (14, "M")]
        elif u < 0.63: cigar = []
        elif u < 0.68: flag &= ~0x2
        out.append(rd(int(p), ref=ref, flag=flag, cigar=cigar, tlen=int(rng.choice([-5, 0, 151, 300, 499, 32767, 32768])), name="q%d" % (i % 977)))
    return out


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, WG - 1, WG, WG + 1, 3 * WG + 1])
def test_record_counts(cv, n):
    rng = np.random.RandomState(1000 + n)
    reads = _mixed(rng, n, 97)
    for mode in MODES:
        for paired in (False, True):
            _, _, info = check(cv, [reads], length=97, mode=mode, paired=paired, what="n %d" % n)
            assert info[1] == n and info[0] == 0


def test_saturation_keeps_the_neighbours(cv):
    for lane in range(4):
        p = 8 + lane
        others = [q for q in range(8, 12) if q != p]
        for count in (254, 255, 256, 300):
            for held in (255, 0, 254):
                hits0 = np.zeros(21, np.uint8)
                hits0[others] = held
                hits0[[7, 12]] = 255                      # the words on either side
                reads = [rd(p) for _ in range(count)]
                if held == 254:                           # ... and one read each: they arrive at 255 while their neighbour counts
                    reads = reads[:100] + [rd(q) for q in others] + reads[100:]
                h, _, _ = check(cv, [reads], length=21, mode=H.MODE_TDR, hits0=hits0, what="lane %d count %d held %d" % (lane, count, held))
                assert h[p] == min(255, count) and all(h[q] == (0 if held == 0 else 255) for q in others) and h[7] == 255 and h[12] == 255
        # mode 5 counts the same way; mode 0 stores a 1
        check(cv, [[rd(p, tlen=9) for _ in range(300)]], length=21, mode=H.MODE_GCW, what="gcw lane %d" % lane)
        h, _, _ = check(cv, [[rd(p) for _ in range(300)]], length=21, mode=H.MODE_BINARY, hits0=np.full(21, 0, np.uint8))
        assert h.sum() == 1
    # a count that saturates over several chunks and stays there
    check(cv, [[rd(2) for _ in range(200)], [rd(2) for _ in range(200)], [rd(2), rd(3)]], length=5)


@pytest.mark.parametrize("length", [1, 2, 3, 5, 4095, 4096])
def test_range(cv, length):
    reads = [rd(p, tlen=77) for p in (-1, -1, 0, 0, length - 1, length, length, length + 1, 2 ** 31 - 1)]
    reads.insert(0, rd(-(2 ** 31), tlen=1))
    for mode in MODES:
        _, _, info = check(cv, [reads], length=length, mode=mode, what="len %d" % length)
        assert info[2] == len(reads) and info[3] == 7                   # in range: 0, 0 and len - 1
    _, _, info = check(cv, [[rd(0), rd(5)]], length=0, mode=H.MODE_TDR, tail=4)
    assert info[2] == 2 and info[3] == 2


def _stop_case(n, stops, skipped_foreign=()):
    reads = [rd(i // 3, tlen=100 + i % 50) for i in range(n)]
    for i in skipped_foreign:
        reads[i] = rd(0, ref=1, flag=0x10)
    for i in stops:
        reads[i] = rd(0, ref=1)
    return reads


def test_stop(cv):
    n = 3 * WG + 1
    for mode in (H.MODE_TDR, H.MODE_GCW):
        for stops in ([0], [n - 1], [n // 2], [63], [64], [65], [WG - 1], [WG], [WG + 1], [2 * WG], [100, 101], [64, WG], [WG - 1, 3 * WG], [5, n - 1]):
            _, _, info = check(cv, [_stop_case(n, stops)], length=300, mode=mode, what="stop at %s" % stops)
            assert info[0] == 1 and info[1] == stops[0] + 1
        # a skipped record of another reference does not stop; unmapped reads of another reference neither
        reads = _stop_case(n, [500], skipped_foreign=[3, 64, 256, 499])
        reads[10] = rd(-1, ref=-1, flag=0x4, cigar=[])
        _, _, info = check(cv, [reads], length=300, mode=mode)
        assert info[0] == 1 and info[1] == 501
        _, _, info = check(cv, [_stop_case(n, [], skipped_foreign=range(0, n, 2))], length=300, mode=mode)
        assert info[0] == 0 and info[1] == n
        # a stop in chunk 1 of 3: the later chunks change nothing and are not seen
        c1, c2, c3 = _stop_case(300, [200]), _stop_case(300, []), _stop_case(300, [7])
        _, _, info = check(cv, [c1, c2, c3], length=300, mode=mode)
        assert info[0] == 1 and info[1] == 201
        _, _, info = check(cv, [c2, c1, c3], length=300, mode=mode)
        assert info[1] == 501
    # the chromosome behind it is all unmapped reads: every one is seen, none stops
    tail = [rd(-1, ref=-1, flag=0x4, cigar=[]) for _ in range(300)]
    _, _, info = check(cv, [_stop_case(100, []), tail], length=300)
    assert info[0] == 0 and info[1] == 400


def test_fragment_length(cv):
    L = 600
    for edge in (64, WG, 2 * WG):
        # a run of one position across the edge, with its neighbours' runs ending exactly at it on other positions
        reads = [rd(i // 7, tlen=1000 + i) for i in range(edge - 5)] + [rd(400, tlen=2000 + i) for i in range(10)] + [rd(401 + i // 3, tlen=3000 + i) for i in range(40)]
        _, f, _ = check(cv, [reads], length=L, mode=H.MODE_GCW, what="run across %d" % edge)
        assert f[400] == 2009
        reads2 = [rd(i // 7, tlen=1000 + i) for i in range(edge)] + [rd(edge // 7 + 50, tlen=5000 + i) for i in range(3)]
        check(cv, [reads2], length=L, mode=H.MODE_GCW, what="run ending at %d" % edge)
        # the same run split between two chunks, and its last records skipped
        check(cv, [reads[:edge], reads[edge:]], length=L, mode=H.MODE_GCW)
        for k in (1, 3, 6):
            sk = [dict(r) for r in reads]
            for r in sk[edge + 5 - k:edge + 5]:
                r["flag"] = 0x10
            _, f, _ = check(cv, [sk], length=L, mode=H.MODE_GCW, what="last %d skipped" % k)
            assert f[400] == 2009 - k
            check(cv, [sk[:edge + 5 - k], sk[edge + 5 - k:]], length=L, mode=H.MODE_GCW)
    # 1000 skipped records between two kept ones of one position, then 20 000
    for gap in (1000, 20000):
        reads = [rd(5, tlen=11)] + [rd(5, flag=0x10, tlen=99) for _ in range(gap)] + [rd(5, tlen=22)] + [rd(6, flag=0x400, tlen=98) for _ in range(300)]
        _, f, info = check(cv, [reads], length=L, mode=H.MODE_GCW, what="gap %d" % gap)
        assert f[5] == 22 and info[2] == 2
        _, f, _ = check(cv, [reads[:-301]], length=L, mode=H.MODE_GCW)
        assert f[5] == 11
    # a kept record of the same position BEHIND the stop does not take the length away
    reads = [rd(5, tlen=11), rd(0, ref=1), rd(5, tlen=22)]
    _, f, _ = check(cv, [reads], length=L, mode=H.MODE_GCW)
    assert f[5] == 11
    tl = [-5, 0, 32767, 32768, 10 ** 6, -(2 ** 31), 2 ** 31 - 1, 1]
    _, f, _ = check(cv, [[rd(10 + i, tlen=t) for i, t in enumerate(tl)]], length=L, mode=H.MODE_GCW)
    assert f[10:18].tolist() == [0, 0, 32767, 32767, 32767, 0, 32767, 1]
    # modes 0 and 3 leave a fragment array alone
    for mode in (H.MODE_BINARY, H.MODE_TDR):
        frag0 = np.arange(L).astype(np.int16)
        _, f, _ = check(cv, [[rd(i, tlen=500) for i in range(0, L, 3)]], length=L, mode=mode, frag0=frag0)
        assert (f == frag0).all()


@pytest.fixture(scope="module")
def chromosome():
    rng = np.random.RandomState(20261021)
    L = 4096
    reads = _mixed(rng, 30000, L)
    for r in reads[4000:5500]:
        r["pos"] = reads[4000]["pos"]                         # a pile-up that saturates
    reads += _mixed(rng, 500, L, ref=1)
    out = {}
    for mode in MODES:
        out[mode] = H.observed_alignments(reads, 0, L, mode, True)
    return L, reads, out


@pytest.mark.parametrize("cuts", [(), (15000,), (1, 300, 4100, 4101, 9000, 29999), (12000, 12000, 31000)])
def test_chunking(cv, chromosome, cuts):
    L, reads, exp = chromosome
    bounds = [0] + list(cuts) + [len(reads)]
    chunks = [reads[a:b] for a, b in zip(bounds[:-1], bounds[1:])]
    for mode in MODES:
        eh, ef, est = exp[mode]
        h, f, info = gpu_run(cv, chunks, 0, L, mode, True, pad=3)
        assert (h == eh).all() and [int(x) for x in info[:6]] == H.state_words(est), (mode, info, est)
        assert est["stopped"] == 1 and est["kept"] > 5000 and h.max() == (1 if mode == H.MODE_BINARY else 255)
        if mode == H.MODE_GCW:
            assert (f == ef).all()


def test_order_does_not_matter_for_hits(cv, chromosome):
    L, reads, exp = chromosome
    mine = [r for r in reads if r["ref"] == 0]
    rng = np.random.RandomState(3)
    shuffled = [mine[i] for i in rng.permutation(len(mine))]
    for mode in (H.MODE_BINARY, H.MODE_TDR):
        h, _, info = gpu_run(cv, [shuffled[:11111], shuffled[11111:]], 0, L, mode, True)
        assert (h == exp[mode][0]).all() and info[2] == exp[mode][2]["kept"]


def test_queued_form(cv, chromosome):
    L, reads, exp = chromosome
    for mode in (H.MODE_TDR, H.MODE_GCW):
        h, f, st = gpu_run(cv, [reads[:9000], reads[9000:20000], reads[20000:]], 0, L, mode, True, want_info=False)
        assert (h == exp[mode][0]).all() and [int(x) for x in st[:6]] == H.state_words(exp[mode][2])
        if mode == H.MODE_GCW:
            assert (f == exp[mode][1]).all()


def test_malformed(cv):
    """every damaged record is the LAST bytes of a buffer of exactly the records' size (pad 0): reading past a bound would leave it"""
    good = [rd(3, tlen=10), rd(4, tlen=20), rd(4, tlen=30)]
    stand_in = dict(malformed=True)
    for mode in (H.MODE_TDR, H.MODE_GCW):
        for what, bad, past_chunk in H.damaged_records(rd):
            _, _, info = check(cv, [good + [bad]], ref_chunks=[good + [stand_in]], mode=mode, what=what)
            assert info[4] == 1 and info[2] == 3 and info[1] == 4
            if past_chunk:                         # (in front of other records its block_size stays inside the chunk)
                continue
            # ... and in front of good records (the offsets say where they start)
            _, _, info = check(cv, [[bad] + good], ref_chunks=[[stand_in] + good], mode=mode, what=what + " first")
            assert info[4] == 1 and info[2] == 3
        # an offset 20 bytes in front of the end, one exactly at the end, one behind it: no 36 bytes are left
        buf_len = sum(len(H.encode_record(r)) for r in good)
        for where, off in H.stray_offsets(buf_len):
            for idx in (0, 2, 3):
                ref = list(good)
                ref.insert(idx, stand_in)
                _, _, info = check(cv, [good], ref_chunks=[ref], mode=mode, extra_offsets={0: [(idx, off)]}, what="offset %s at %d" % (where, idx))
                assert info[4] == 1 and info[1] == 4 and info[2] == 3
    # many of them among many records, over a workgroup edge
    reads, ref = [], []
    for i in range(2 * WG + 9):
        if i % 5 == 2:
            reads.append(rd(i // 4, n_cigar=50000)); ref.append(stand_in)
        else:
            reads.append(rd(i // 4, tlen=i)); ref.append(reads[-1])
    _, _, info = check(cv, [reads], ref_chunks=[ref], length=200, mode=H.MODE_GCW)
    assert info[4] == sum(1 for r in ref if r is stand_in)


def test_arguments(cv):
    import torch
    from canvas_amd import CanvasError
    buf, offs, nb = H.chunk_of([rd(1)])
    d_buf, d_off = to_dev(buf, cv.device), to_dev(offs, cv.device)
    for mode in (1, 2, 4, 6, -1):
        with pytest.raises(CanvasError):
            cv.hits_from_bam(d_buf, d_off, 0, 10, mode=mode)
    hits = torch.zeros(16, dtype=torch.uint8, device=cv.device)
    st = torch.zeros(8, dtype=torch.int64, device=cv.device)
    L = cv.lib.canvas_hits_from_bam
    import ctypes as C
    args = lambda mode, length, frag: (cv.ctx, C.c_void_p(d_buf.data_ptr()), C.c_uint64(nb), C.c_void_p(d_off.data_ptr()), C.c_int64(1), C.c_int32(0), C.c_int32(0), C.c_int32(mode),
                                      C.c_int64(length), C.c_void_p(hits.data_ptr()), frag, C.c_void_p(st.data_ptr()), None)
    assert L(*args(5, 10, None)) == -1 and L(*args(3, -1, None)) == -1 and L(*args(3, 2 ** 31, None)) == -1 and L(*args(3, 10, None)) == 0
    cv.synchronize()
    assert hits.cpu().numpy().tolist() == [0, 1] + [0] * 14
