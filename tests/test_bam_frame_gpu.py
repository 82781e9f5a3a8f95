"""Canvas.bam_frame (canvas_amd/csrc/frame.hip) against the sequential restatement of the executables' framing loop (tests/frame_ref.py): the offsets, h_info[0..5]
and d_state are compared exactly, for every case twice — as built, and with CANVAS_FRAME_NO_GUESS=1, which sends every tile through the exact second walk.  The two
runs may differ in h_info[6] (tiles walked twice) and in nothing else.  The device chunk holds exactly the case's bytes; the offsets buffer carries a sentinel behind
the capacity, which has to survive."""
import os
import struct

import numpy as np
import pytest

import frame_cases as FC
import frame_ref as FR
import hits_ref as H
import snv_cases as SC
import snv_ref as R
from gpu_common import get_canvas, to_dev

pytestmark = pytest.mark.gpu
SENTINEL = -0x0123456789


@pytest.fixture(scope="module")
def cv():
    return get_canvas()


@pytest.fixture(scope="module")
def T(cv):
    import torch
    offs, info = cv.bam_frame(torch.zeros(1, dtype=torch.uint8, device=cv.device), 0, FC.RULES["all"], nbytes=0)
    assert len(offs) == 0 and info.tolist()[:6] == [0, 0, 0, 0, -1, 0] and info[7] >= 1024
    return int(info[7])


def device_frame(cv, buf, first, rule, state=None, capacity=None, no_guess=False):
    """-> (offsets, info[8], state[4]) of one call"""
    import torch
    d_buf = to_dev(np.frombuffer(bytes(buf), np.uint8), cv.device) if len(buf) else torch.zeros(1, dtype=torch.uint8, device=cv.device)
    cap = max((len(buf) - min(first, len(buf))) // 36 + 2, 1) if capacity is None else capacity
    d_off = torch.full((cap + 4,), SENTINEL, dtype=torch.int64, device=cv.device)
    d_state = to_dev(np.array(state if state is not None else [0, 0, 0, 0], np.int64), cv.device)
    os.environ.pop("CANVAS_FRAME_NO_GUESS", None)
    if no_guess:
        os.environ["CANVAS_FRAME_NO_GUESS"] = "1"
    try:
        offs, info = cv.bam_frame(d_buf, first, rule, d_off[:cap], d_state, nbytes=len(buf))
    finally:
        os.environ.pop("CANVAS_FRAME_NO_GUESS", None)
    cv.synchronize()
    whole = d_off.cpu().numpy()
    n = len(offs)
    assert (whole[n:] == SENTINEL).all(), "offsets written behind the taken records"
    return whole[:n].tolist(), info, d_state.cpu().numpy().tolist()


def check(cv, name, buf, first, rule, state=None, capacity=None):
    """both forms against frame_ref; -> (info of the default form, state after the call)"""
    e_offs, e_info, e_state, seen = FR.frame(buf, first, rule, state, capacity)
    out = None
    for no_guess in (False, True):
        offs, info, st = device_frame(cv, buf, first, rule, state, capacity, no_guess)
        what = (name, rule, "no guess" if no_guess else "default")
        assert info.tolist()[:6] == e_info, (what, info.tolist(), e_info)
        assert offs == e_offs, (what, len(offs), len(e_offs), [(a, b) for a, b in zip(offs, e_offs) if a != b][:4])
        assert st == e_state, (what, st, e_state)
        if no_guess and len(buf) - first >= 4:
            # the hook took effect: every tile the chain arrives in was walked again — the tile of `first`, and the tile of the byte behind every whole record of
            # the chain but a malformed one, where it ends.  The chain is walked to its end whatever the rule stops at: the records of kind ALL.
            tile = int(info[7])
            chain = FR.frame(buf, first, FC.RULES["all"])[3]
            reached = {first // tile} | {(at + 4 + struct.unpack_from("<i", buf, at)[0]) // tile for at, cls in chain if cls != FR.MALFORMED}
            assert info[6] == len(reached) and info[6] >= out[0][6], (what, info.tolist(), sorted(reached)[:8])
        out = out or (info, st)
    return out


def test_chunk_ends(cv, T):
    for name, buf, first in FC.chunk_end_cases():
        for rule in FC.RULES.values():
            check(cv, name, buf, first, rule)


def test_record_sizes_against_the_tile(cv, T):
    for name, buf, first in FC.tile_cases(T):
        for rule in (FC.RULES["all"], FC.RULES["snv"]):
            info, st = check(cv, name, buf, first, rule)
        if name.startswith("record longer than 5"):
            assert info[6] <= 2, info            # the tiles inside the long record hold no record start and are stepped over, not walked


def test_decoys(cv, T):
    wrong = {}
    for name, buf, first in FC.decoy_cases(T):
        for rule in FC.RULES.values():
            info, st = check(cv, name, buf, first, rule)
        wrong[name] = int(info[6])
    assert max(wrong.values()) > 0, wrong                     # otherwise no decoy was the first plausible candidate of its tile: the cases miss what they aim at
    assert wrong["decoy in front of first"] == 0, wrong       # tile 0 is entered at `first`, whatever stands in front of it


def test_hostile_sizes(cv, T):
    for name, buf, first in FC.hostile_cases(T):
        for rule in (FC.RULES["all"], FC.RULES["snv"], FC.RULES["hits_paired_sorted"]):
            check(cv, name, buf, first, rule)


@pytest.mark.parametrize("kind", [FR.ALL, FR.SNV, FR.HITS, FR.FRAGMENTS])
def test_rules_on_random_streams(cv, T, kind):
    rules = [r for r in FC.RULES.values() if r[0] == kind]
    n = 2000
    plain = b"".join(FC.random_stream(20261021 + kind, kind, n=n))
    for rule in rules:
        info, st = check(cv, "no event", plain, 0, rule)
        assert info[0] == n and info[3] == FR.NONE
    for what, ev, code in FC.events_of(kind):
        for where in (0, n):
            buf = b"".join(FC.random_stream(20261021 + kind, kind, n=n, event=ev, where=where))
            for rule in rules:
                info, st = check(cv, what, buf, 0, rule)
                assert info[3] == code and info[0] == where + 1, (what, where, info)
    # everything mixed without regard to the rule: the event falls where it falls
    rng = np.random.RandomState(7 + kind)
    wild = b"".join(FC.rec(ref=int(rng.choice([-1, FC.REF - 1, FC.REF, FC.REF + 1], p=[0.01, 0.04, 0.9, 0.05])), pos=int(rng.choice([-1, i // 2], p=[0.01, 0.99])),
                           flag=sum(f for f in [0x1, 0x2, 0x4, 0x10, 0x100, 0x200, 0x400, 0x800] if rng.rand() < 0.3),
                           cigar=[((34, "M"),), ((35, "M"),), ((35, "S"),)][rng.randint(3)], total=int(rng.randint(FC.HEAD, 200))) for i in range(n))
    for rule in rules:
        check(cv, "wild", wild, 0, rule)


def test_unsorted(cv, T):
    for rule in (FC.RULES["snv"], FC.RULES["hits_paired_sorted"]):
        flag = 0x2 if rule[0] == FR.HITS else 0
        run = FC.sorted_run(600, start=10, total=83, flag=flag)
        for where in (1, 300, 599):
            recs = list(run)
            recs[where] = FC.rec(pos=9, flag=flag, total=83)
            info, st = check(cv, "unsorted at %d" % where, b"".join(recs), 0, rule)
            assert info[3] == FR.EV_UNSORTED and info[0] == where + 1 and info[4] == 83 * where and info[5] == 10 + 3 * (where - 1)
        # a pair that straddles two calls
        info, st = check(cv, "first call", b"".join(run), 0, rule)
        assert st[:2] == [600, 10 + 3 * 599] and info[3] == FR.NONE
        info, st2 = check(cv, "second call", b"".join(FC.sorted_run(5, start=10 + 3 * 599 - 1, total=83, flag=flag)), 0, rule, state=st)
        assert info[3] == FR.EV_UNSORTED and info[0] == 1 and info[5] == 10 + 3 * 599
        info, st2 = check(cv, "second call in order", b"".join(FC.sorted_run(5, start=10 + 3 * 599, total=83, flag=flag)), 0, rule, state=st)
        assert info[3] == FR.NONE and st2[:3] == [605, 10 + 3 * 599 + 12, 605]


def test_three_calls_share_state_and_carry(cv, T):
    """a stream cut at arbitrary bytes: each call starts at the previous `used`, as the executables' loop moves the tail to the front of the next buffer"""
    for name in ("snv", "hits_paired_sorted", "fragments"):
        rule = FC.RULES[name]
        stream = b"".join(FC.random_stream(99, rule[0], n=1500)) + FC.rec(ref=FC.REF + 1, pos=0, flag=0x2) + b"".join(FC.sorted_run(10, total=70))
        cuts = [0, len(stream) // 3 + 1, 2 * len(stream) // 3 + 2, len(stream)]
        carry, state, taken, events = b"", None, 0, []
        for a, b in zip(cuts[:-1], cuts[1:]):
            buf = carry + stream[a:b]
            info, state = check(cv, "call at %d" % a, buf, 0, rule, state=state)
            carry = buf[int(info[2]):]
            taken += int(info[1])
            events.append(int(info[3]))
        whole = FR.frame(stream, 0, rule)
        assert taken == whole[1][1] and state[2] == taken and events == [FR.NONE, FR.NONE, FR.STOPPED] and state[:2] == whole[2][:2]
        # `first` instead of a moved tail
        used = int(FR.frame(stream[:cuts[1]], 0, rule)[1][2])
        offs, info, st = device_frame(cv, stream, used, rule)
        assert offs == [o for o in whole[0] if o >= used]


def test_capacity(cv, T):
    buf = b"".join(FC.random_stream(3, FR.SNV, n=900))
    rule = FC.RULES["snv"]
    taken = FR.frame(buf, 0, rule)[1][1]
    assert 100 < taken < 900
    info, st = check(cv, "one short", buf, 0, rule, state=[4, 0, 17, 0], capacity=taken - 1)
    assert info[3] == FR.CAPACITY and info[1] == taken and st == [4, 0, 17, 0]
    info, st = check(cv, "repeated", buf, 0, rule, state=st, capacity=taken)
    assert info[3] == FR.NONE and info[1] == taken and st[2] == 17 + taken
    check(cv, "nothing taken, no buffer", FC.rec(ref=-1), 0, rule, capacity=0)


def test_refusals_with_a_live_context(cv, T):
    import ctypes as C
    import torch
    buf = to_dev(np.frombuffer(b"".join(FC.sorted_run(50, total=80)), np.uint8), cv.device)
    offs = torch.full((64,), SENTINEL, dtype=torch.int64, device=cv.device)
    state = torch.full((4,), 5, dtype=torch.int64, device=cv.device)
    rule = np.zeros(1, [("kind", "<i4"), ("ref_id", "<i4"), ("paired_end", "<i4"), ("sorted", "<i4")])
    info = np.full(8, -7, np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    d = lambda t: C.c_void_p(t.data_ptr())
    f = cv.lib.canvas_bam_frame
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    n = buf.numel()
    bad_kind = rule.copy()
    bad_kind["kind"] = 4
    negative = rule.copy()
    negative["kind"] = -1
    for args in ((d(buf), n, 0, None, d(offs), 64, d(state), p(info)), (d(buf), n, 0, p(rule), d(offs), 64, None, p(info)), (d(buf), n, 0, p(rule), d(offs), 64, d(state), None),
                 (d(buf), n, n + 1, p(rule), d(offs), 64, d(state), p(info)), (d(buf), n, 0, p(bad_kind), d(offs), 64, d(state), p(info)),
                 (d(buf), n, 0, p(negative), d(offs), 64, d(state), p(info)), (d(buf), n, 0, p(rule), None, 64, d(state), p(info)),
                 (d(buf), n, 0, p(rule), d(offs), -1, d(state), p(info)), (None, n, 0, p(rule), d(offs), 64, d(state), p(info))):
        assert f(cv.ctx, *args) == -1, args
    cv.synchronize()
    assert (info == -7).all() and (offs.cpu().numpy() == SENTINEL).all() and state.cpu().numpy().tolist() == [5, 5, 5, 5]


def test_hand_off_to_hits_from_bam(cv, T):
    rng = np.random.RandomState(12)
    reads = [dict(ref=0, pos=int(p), flag=int(rng.choice([0x2, 0x12, 0x402, 0x63])), cigar=[(36, "M")], seq="A" * 36, tlen=int(rng.choice([0, 150, 400])), name="h%d" % i)
             for i, p in enumerate(np.sort(rng.randint(0, 5000, 1500)))]
    reads += [dict(ref=1, pos=5, flag=0x4, cigar=[(36, "M")], seq="A" * 36, name="x"), dict(ref=1, pos=6, flag=0x2, cigar=[(36, "M")], seq="A" * 36, name="y"),
              dict(ref=1, pos=7, flag=0x2, cigar=[(36, "M")], seq="A" * 36, name="z")]
    buf, host_offs, nbytes = H.chunk_of(reads)
    e_offs = FR.frame(bytes(buf), 0, (FR.HITS, 0, 1, 1))[0]
    assert e_offs == host_offs.tolist()[:-1]                      # the passing read of reference 1 is taken and stops; the one behind it is not
    d_buf = to_dev(buf, cv.device)
    offs, info = cv.bam_frame(d_buf, 0, (FR.HITS, 0, 1, 1))
    assert offs.cpu().numpy().tolist() == e_offs and info[3] == FR.STOPPED and info[2] == host_offs[-1]
    got = cv.hits_from_bam(d_buf, offs.contiguous(), 0, 5100, H.MODE_GCW, True, nbytes=int(info[2]))
    want = cv.hits_from_bam(d_buf, to_dev(np.array(e_offs, np.int64), cv.device), 0, 5100, H.MODE_GCW, True, nbytes=int(info[2]))
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and got[3].tolist()[:6] == want[3].tolist()[:6] and got[3][2] > 100 and got[3][0] == 1


def test_hand_off_to_snv_count(cv, T):
    from canvas_amd.lib import snv_allele_codes
    rng = np.random.RandomState(13)
    reads = SC.random_reads(rng, 800, 6000, ref=2) + SC.random_reads(rng, 20, 500, ref=3)
    for r in SC.random_reads(rng, 30, 500, ref=1)[::-1]:
        reads.insert(0, r)
    buf, host_offs, nbytes = SC.chunk_of(reads, 0)
    e_offs = FR.frame(bytes(buf[:nbytes]), 0, (FR.SNV, 2, 0, 0))[0]
    assert e_offs == host_offs.tolist()[30:830]
    sites = SC.random_sites(rng, 6000, 7)
    pos = to_dev(np.array([v.pos for v in sites], np.int32), cv.device)
    ref, alt = to_dev(snv_allele_codes([v.ref for v in sites]), cv.device), to_dev(snv_allele_codes([v.alt for v in sites]), cv.device)
    d_buf = to_dev(buf[:nbytes], cv.device)
    offs, info = cv.bam_frame(d_buf, 0, (FR.SNV, 2, 0, 0))
    assert offs.cpu().numpy().tolist() == e_offs and info[3] == FR.STOPPED and info[2] == host_offs[830] and info[0] == 831
    got = cv.snv_count(d_buf, offs.contiguous(), 2, pos, ref, alt, nbytes=int(info[2]))
    want = cv.snv_count(d_buf, to_dev(np.array(e_offs, np.int64), cv.device), 2, pos, ref, alt, nbytes=int(info[2]))
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and got[2].tolist() == want[2].tolist() and int(got[0].sum() + got[1].sum()) > 100
    assert struct.calcsize("<iiii") == 16 and R.Variant is not None
