"""tests/frame_ref.py against expectations written by hand: the decision order of each rule, the chain's ends, `used`, and the carried state."""
import struct

import frame_cases as FC
import frame_ref as FR
from frame_cases import REF, rec


def classes(records, rule, **kw):
    return [c for _, c in FR.frame(b"".join(records), 0, FC.RULES[rule] if isinstance(rule, str) else rule, **kw)[3]]


def test_the_chain_and_used():
    a, b, c = rec(total=50), rec(total=61), rec(total=72)
    buf = a + b + c
    offs, info, state, seen = FR.frame(buf, 0, FC.RULES["all"])
    assert offs == [0, 50, 111] and info == [3, 3, 183, FR.NONE, -1, 0] and state == [0, 0, 3, FR.NONE]
    # an incomplete record and trailing bytes are the carry, and no event
    assert FR.frame(buf[:-1], 0, FC.RULES["all"])[1] == [2, 2, 111, FR.NONE, -1, 0]
    assert FR.frame(buf + b"\x01\x02\x03", 0, FC.RULES["all"])[1] == [3, 3, 183, FR.NONE, -1, 0]
    assert FR.frame(buf, 50, FC.RULES["all"])[0] == [50, 111]
    assert FR.frame(buf, 181, FC.RULES["all"]) == ([], [0, 0, 181, FR.NONE, -1, 0], [0, 0, 0, 0], [])
    # block_size below 32 is malformed whatever stands behind it; 0x7FFFFFFF is a record the next chunk completes
    for bs in (0, 31, -1, -(2 ** 31)):
        assert FR.frame(a + struct.pack("<i", bs) + b[4:] + c, 0, FC.RULES["all"])[1] == [2, 1, 50, FR.EV_MALFORMED, 50, 0]
    assert FR.frame(a + struct.pack("<i", 0x7FFFFFFF) + b[4:] + c, 0, FC.RULES["all"])[1] == [1, 1, 50, FR.NONE, -1, 0]


def test_snv_order_of_decisions():
    # bases that do not fit come before everything else; then the stop, then the skip, then sortedness
    assert classes([rec(ref=-1, pos=-1, l_seq=50, block_size=60)], "snv") == [FR.MALFORMED]
    assert classes([rec(pos=5), rec(ref=-1, pos=7), rec(pos=9)], "snv") == [FR.TAKE, FR.STOP]
    offs, info, state, seen = FR.frame(rec(pos=5) + rec(ref=-1, pos=7) + rec(pos=9), 0, FC.RULES["snv"])
    assert offs == [0] and info[1:5] == [1, FC.HEAD, FR.STOPPED, FC.HEAD]              # SNV stops before an unmapped record and does not take it: `used` stays at it
    assert classes([rec(ref=REF - 1, pos=50), rec(pos=5), rec(ref=REF - 1, pos=1), rec(pos=4)], "snv") == [FR.SKIP, FR.TAKE, FR.SKIP, FR.UNSORTED]
    assert classes([rec(ref=REF + 1, pos=0)], "snv") == [FR.STOP] and classes([rec(pos=-1)], "snv") == [FR.STOP]
    assert FR.frame(rec(pos=5) + rec(pos=4), 0, FC.RULES["snv"])[1] == [2, 1, FC.HEAD, FR.EV_UNSORTED, FC.HEAD, 5]
    assert classes([rec(pos=5), rec(pos=5)], "snv") == [FR.TAKE, FR.TAKE]


def test_hits_order_of_decisions():
    passing, dropped = dict(flag=0x2), dict(flag=0x4)
    # a filtered-out record of another reference does not stop HITS; a passing one is taken and stops
    assert classes([rec(ref=REF + 1, **dropped), rec(**passing), rec(ref=REF + 1, **passing), rec(**passing)], "hits") == [FR.TAKE, FR.TAKE, FR.TAKE_AND_STOP]
    offs, info, state, seen = FR.frame(rec(**passing) + rec(ref=REF + 1, **passing) + rec(**passing), 0, FC.RULES["hits"])
    assert offs == [0, FC.HEAD] and info == [2, 2, 2 * FC.HEAD, FR.STOPPED, FC.HEAD, 0]
    # unsorted input matters to the sorted rule only, and only among the records that pass the filters
    back = [rec(pos=9, **passing), rec(pos=3, **dropped), rec(pos=8, **passing)]
    assert classes(back, "hits") == [FR.TAKE] * 3 and classes(back, "hits_paired_sorted") == [FR.TAKE, FR.TAKE, FR.UNSORTED]
    # the pair filter is part of the rule: without 0x2 a read of another reference passes the unpaired filters and stops, and is dropped by the paired ones
    assert classes([rec(ref=REF + 1, flag=0)], "hits") == [FR.TAKE_AND_STOP] and classes([rec(ref=REF + 1, flag=0)], "hits_paired_sorted") == [FR.TAKE]
    assert classes([rec(ref=REF + 1, cigar=((34, "M"),))], "hits") == [FR.TAKE] and classes([rec(ref=REF + 1, cigar=((35, "S"),))], "hits") == [FR.TAKE]
    assert classes([rec(ref=REF + 1, cigar=((35, "M"),))], "hits") == [FR.TAKE_AND_STOP]
    assert classes([rec(ref=REF + 1, n_cigar=5000, **dropped)], "hits") == [FR.MALFORMED]
    assert classes([rec(pos=-(2 ** 31), **passing)], "hits_paired_sorted") == [FR.TAKE]


def test_fragments_order_of_decisions():
    assert classes([rec(), rec(flag=0x4), rec(ref=REF - 1, flag=0x4), rec()], "fragments") == [FR.TAKE, FR.TAKE, FR.TAKE_AND_STOP]
    assert classes([rec(ref=REF + 1, n_cigar=5000)], "fragments") == [FR.MALFORMED]
    assert classes([rec(pos=9), rec(pos=3)], "fragments") == [FR.TAKE, FR.TAKE]


def test_state_and_capacity():
    run = b"".join(FC.sorted_run(5, start=10, total=70))
    offs, info, state, seen = FR.frame(run, 0, FC.RULES["snv"])
    assert state == [5, 22, 5, FR.NONE]
    offs, info, state2, seen = FR.frame(run, 0, FC.RULES["snv"], state)
    assert info[:2] == [1, 0] and info[3:] == [FR.EV_UNSORTED, 0, 22] and state2 == [5, 22, 5, FR.EV_UNSORTED]
    offs, info, state3, seen = FR.frame(run, 0, FC.RULES["snv"], capacity=4)
    assert offs == [] and info[1] == 5 and info[3] == FR.CAPACITY and state3 == [0, 0, 0, 0]
    # the events of frame_cases stop their rule wherever they stand
    for kind in (FR.ALL, FR.SNV, FR.HITS, FR.FRAGMENTS):
        for what, ev, code in FC.events_of(kind):
            for rule in (r for r in FC.RULES.values() if r[0] == kind):
                assert FR.frame(ev + run, 0, rule)[1][3] == code and FR.frame(run + ev, 0, rule)[1][3] == code, (what, rule)
        for rule in (r for r in FC.RULES.values() if r[0] == kind):
            assert FR.frame(b"".join(FC.random_stream(5, kind, n=400)), 0, rule)[1][:2][0] == 400 and FR.frame(b"".join(FC.random_stream(5, kind, n=400)), 0, rule)[1][3] == FR.NONE
