"""The restatement of the partition states (tests/partition_states_ref.py) against the reference's own loops: the segment start coordinates CBSRunner's cs1 / cs2 loop and
SegmentationInput.DeriveSegments produce are, as a set, the starts of the bins at which the restated states open a segment — and PostProcessSegments (the oracle's, with
and without the -b / gap / -p rules) gives identical ids for either set.  No GPU."""
import numpy as np
import pytest

import oracle_lib as O
import partition_states_ref as P


def _configs():
    out = []
    for name, seg_len, nseg in P.directed_cbs():
        out.append((name, P.LENGTHS, "cbs", seg_len, nseg))
    for name, bps in P.directed_breakpoints():
        out.append((name, P.LENGTHS, "breakpoints", bps))
    for seed in range(200):
        out.append((("random %d" % seed,) + P.random_config(seed)))
    return out


CONFIGS = _configs()


def _both_routes(cfg, start):
    lengths, method = cfg[1], cfg[2]
    off = P.offsets(lengths)
    if method == "cbs":
        state = P.states_cbs(off, cfg[3], cfg[4])
        literal = P.literal_starts_cbs(off, cfg[3], cfg[4], start)
    else:
        state = P.states_breakpoints(off, cfg[3])
        literal = P.literal_starts_breakpoints(off, cfg[3], start)
    return off, state, literal, P.starts_from_states(off, state, start)


def test_the_two_routes_give_the_same_start_sets():
    methods = set()
    for k, cfg in enumerate(CONFIGS):
        start, stop = P.bins(cfg[1], 100 + k)
        off, state, literal, derived = _both_routes(cfg, start)
        assert P.same_start_sets(literal, derived), cfg[0]
        assert len(state) == off[-1] and state.dtype == np.int32
        for c in range(len(cfg[1])):                              # ordinals: 0 at the first bin of a chromosome that derives segments, steps of 0 or 1, -1 throughout otherwise
            s = state[off[c]:off[c + 1]]
            if len(s) and len(literal[c]):
                assert s[0] == 0 and set(np.diff(s).tolist()) <= {0, 1} and s[-1] == len(set(literal[c].tolist())) - 1, (cfg[0], c)
            else:
                assert (s == -1).all(), (cfg[0], c)
        methods.add(cfg[2])
    assert methods == {"cbs", "breakpoints"}


@pytest.mark.parametrize("rules", ("plain", "all rules"))
def test_postprocess_gives_identical_ids_for_either_start_set(rules):
    fired = 0
    for k, cfg in enumerate(CONFIGS):
        lengths = cfg[1]
        start, stop = P.bins(lengths, 100 + k)
        off, state, literal, derived = _both_routes(cfg, start)
        bs = [start[off[c]:off[c + 1]].astype(np.uint32) for c in range(len(lengths))]; be = [stop[off[c]:off[c + 1]].astype(np.uint32) for c in range(len(lengths))]
        if rules == "plain":
            a, la = O.postprocess(bs, be, literal)
            b, lb = O.postprocess(bs, be, derived)
        else:
            excluded, ploidy = P.intervals(lengths, start, stop, 7 + k)
            a, la = O.postprocess_ploidy(bs, be, literal, excluded, ploidy, 2000)
            b, lb = O.postprocess_ploidy(bs, be, derived, excluded, ploidy, 2000)
            fired += la > O.postprocess(bs, be, literal)[1]
        assert la == lb and all((x == y).all() for x, y in zip(a, b)), cfg[0]
    assert rules == "plain" or fired > 100


def test_the_restatement_refuses_what_the_entry_refuses():
    lengths = [5, 0, 12, 7]
    off = P.offsets(lengths)
    seg_len, nseg = P.cbs_layout(lengths, [[0, 2], [], [0, 5, 11], [0]])
    assert P.states_cbs(off, seg_len, nseg).tolist() == [0, 0, 1, 1, 1] + [0] * 5 + [1] * 6 + [2] + [0] * 7
    for change, want in ((lambda s, n: s.__setitem__(6, 0), (2, "length")), (lambda s, n: s.__setitem__(7, 7), (2, "sum")), (lambda s, n: s.__setitem__(7, 5), (2, "sum")),
                         (lambda s, n: n.__setitem__(3, 8), (3, "nseg")), (lambda s, n: n.__setitem__(1, 1), (1, "nseg")), (lambda s, n: n.__setitem__(0, -1), (0, "nseg")),
                         (lambda s, n: (s.__setitem__(0, 9), n.__setitem__(3, 8)), (0, "sum"))):
        s, n = seg_len.copy(), nseg.copy()
        change(s, n)
        with pytest.raises(P.Invalid) as e:
            P.states_cbs(off, s, n)
        assert (e.value.chromosome, e.value.kind) == want
