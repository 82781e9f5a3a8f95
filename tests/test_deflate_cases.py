"""tests/deflate_cases.py held to zlib: the verdict stated with every hand-built stream is zlib's, what zlib wrote is valid, and the mutation list has enough of both
kinds to mean something.  (The decoder itself: test_inflate_host.py on the CPU, test_bgzf_inflate_gpu.py on the device.)"""
import deflate_cases as D


def test_stated_verdicts_are_zlibs():
    cases = D.hand_cases()
    assert len(cases) >= 190
    for name, stream, out_bytes, accepted in cases:
        ok, out = D.zlib_verdict(stream, out_bytes)
        assert ok == accepted, name
        assert len(out) == (out_bytes if ok else 0), name


def test_hand_built_bytes():
    """a few streams whose bytes are plain to see"""
    by = {n: (s, o) for n, s, o, ok in D.hand_cases()}
    for name, want in (("two stored blocks", b"hello world"), ("distance 1 length 258", b"a" * 259), ("match across a deflate-block boundary", b"abcabc"),
                       ("overlap: distance 3 length 258", (b"!\"#" * 87)[:261]), ("dynamic 15-bit literal and distance codes", b"abc" + b"n" * 10),
                       ("the last symbol ends on the last bit of the last byte", b"\xc8" * 6)):
        assert D.zlib_verdict(*by[name]) == (True, want), name


def test_zlib_output_is_valid():
    cases = D.zlib_cases()
    assert len(cases) >= 5 * 3 * 4 * 4 + 1
    too_long = 0
    for name, stream, out_bytes in cases:
        assert D.zlib_verdict(stream, out_bytes)[0], name
        too_long += len(stream) > D.LIMIT
    assert 0 < too_long < 40            # level 0 and random data at 65536 bytes: no BGZF block; expected_status refuses their descriptors


def test_mutations_go_both_ways():
    muts = D.mutations()
    assert len(muts) == 2000
    accepted = sum(D.zlib_verdict(s, o)[0] for n, s, o in muts)
    assert accepted >= 100 and len(muts) - accepted >= 100, accepted
