"""canvas_partition_states_cbs / canvas_partition_states_breakpoints on the device, byte for byte against the numpy restatement (tests/partition_states_ref.py) on the
directed shapes, the refusals, and the chain states -> segment_ids (excluded intervals, ploidy records and a small max_inter_bin_dist, so that all three rules fire)
against the oracle's PostProcessSegments on the LITERAL start sets of CBSRunner / DeriveSegments."""
import numpy as np
import pytest

import oracle_lib as O
import partition_states_ref as P
from gpu_common import get_canvas, to_dev

pytestmark = pytest.mark.gpu
MAX_DIST = 2000
Z3 = (np.zeros(0, np.int32),) * 3


@pytest.fixture(scope="module")
def cv():
    return get_canvas()


def _device_states(cv, cfg):
    """cfg = (lengths, "cbs", seg_len, nseg) | (lengths, "breakpoints", breakpoints) -> (offsets, states from the device, restated states)"""
    import torch
    off = P.offsets(cfg[0])
    out = torch.full((int(off[-1]) + 3,), -77, dtype=torch.int32, device=cv.device)      # three entries behind the last bin: the call must leave them alone
    if cfg[1] == "cbs":
        got = cv.partition_states(off, seg_len=to_dev(cfg[2], cv.device), nseg=cfg[3], out=out)
        want = P.states_cbs(off, cfg[2], cfg[3])
    else:
        got = cv.partition_states(off, breakpoints=cfg[2], out=out)
        want = P.states_breakpoints(off, cfg[2])
    assert got.dtype == torch.int32 and got.numel() == off[-1] and got.data_ptr() == out.data_ptr()
    assert out[int(off[-1]):].tolist() == [-77] * 3
    return off, got, want


def _same(got, want, name):
    g = got.cpu().numpy()
    assert g.dtype == want.dtype and g.tobytes() == want.tobytes(), (name, np.nonzero(g != want)[0][:8].tolist())


def _chain(cv, cfg, off, state, seed, name):
    """the states through segment_ids with every rule against PostProcessSegments on the literal starts; returns (last id, last id without the three rules)"""
    lengths = cfg[0]
    start, stop = P.bins(lengths, seed)
    literal = P.literal_starts_cbs(off, cfg[2], cfg[3], start) if cfg[1] == "cbs" else P.literal_starts_breakpoints(off, cfg[2], start)
    excluded, ploidy = P.intervals(lengths, start, stop, seed + 1)
    bs = [start[off[c]:off[c + 1]].astype(np.uint32) for c in range(len(lengths))]; be = [stop[off[c]:off[c + 1]].astype(np.uint32) for c in range(len(lengths))]
    ids, last = O.postprocess_ploidy(bs, be, literal, excluded, ploidy, MAX_DIST)
    seg, nseg = cv.segment_ids(off, state, to_dev(start, cv.device), to_dev(stop, cv.device), MAX_DIST, excluded=excluded, ploidy=[p if p is not None else Z3 for p in ploidy])
    g = seg.cpu().numpy(); w = np.concatenate(ids + [np.zeros(0, np.int32)])
    assert (g == w).all(), (name, np.nonzero(g != w)[0][:8].tolist())
    assert nseg == last + 1, name
    return last, O.postprocess(bs, be, literal)[1], O.postprocess(bs, be, literal, excluded)[1], O.postprocess(bs, be, literal, None, MAX_DIST)[1], O.postprocess_ploidy(bs, be, literal, None, ploidy)[1]


@pytest.mark.parametrize("k", range(len(P.directed_cbs())))
def test_cbs_directed_shapes(cv, k):
    name, seg_len, nseg = P.directed_cbs()[k]
    cfg = (P.LENGTHS, "cbs", seg_len, nseg)
    off, got, want = _device_states(cv, cfg)
    _same(got, want, name)
    if k == 0:
        assert (want == -1).all()
    if name == "every length 1":
        assert int(nseg.max()) == 4097 > 256                   # the tiled length scan carries its sum over 17 tiles
    last, plain, with_excluded, with_gap, with_ploidy = _chain(cv, cfg, off, got, 500 + k, name)
    if plain + 1 == off[-1]:                                    # every bin opens a segment already: no rule can add one
        assert name == "every length 1" and last == plain
    else:                                                       # all three rules fire (also where every state is -1)
        assert with_excluded > plain and with_gap > plain and with_ploidy > plain and last > max(with_excluded, with_gap, with_ploidy)


@pytest.mark.parametrize("k", range(len(P.BP_PATTERNS)))
def test_breakpoints_directed_shapes(cv, k):
    name, bps = P.directed_breakpoints()[k]
    cfg = (P.LENGTHS, "breakpoints", bps)
    off, got, want = _device_states(cv, cfg)
    _same(got, want, name)
    h = got.cpu().numpy()
    for c, T in enumerate(P.LENGTHS):                           # at most 10 bins, or fewer than two breakpoints: one segment whatever the breakpoints say
        if 0 < T <= 10 or (T and len(bps[c]) < 2):
            assert (h[off[c]:off[c + 1]] == 0).all(), (name, c)
    if k == 0:                                                  # chromosome 3 (11 bins) has "two not from 0", chromosome 2 (10 bins) "two from 0"
        assert len(bps[2]) >= 2 and len(bps[3]) >= 2 and h[off[3]:off[4]].max() == 2 and h[off[2]:off[3]].max() == 0
    last, plain, with_excluded, with_gap, with_ploidy = _chain(cv, cfg, off, got, 600 + k, name)
    assert with_excluded > plain and with_gap > plain and with_ploidy > plain and last > max(with_excluded, with_gap, with_ploidy)


def test_fifty_random_configurations_through_the_chain(cv):
    seen = set()
    for seed in range(50):
        cfg = P.random_config(seed)
        off, got, want = _device_states(cv, cfg)
        _same(got, want, seed)
        _chain(cv, cfg, off, got, 700 + seed, seed)
        seen.add(cfg[1])
    assert seen == {"cbs", "breakpoints"}


def test_cbs_refusals_name_the_chromosome_and_leave_the_states_alone(cv):
    import torch
    from canvas_amd import CanvasError
    lengths = [300, 0, 700, 2050]
    off = P.offsets(lengths)
    seg_len, nseg = P.cbs_layout(lengths, [[0, 100], [], [0, 256, 699], [0, 2048]])
    good = cv.partition_states(off, seg_len=to_dev(seg_len, cv.device), nseg=nseg)
    _same(good, P.states_cbs(off, seg_len, nseg), "good")

    def refused(chromosome, kind, s=None, n=None):
        s = seg_len.copy() if s is None else s; n = nseg.copy() if n is None else n
        with pytest.raises(P.Invalid) as e:
            P.states_cbs(off, s, n)
        assert (e.value.chromosome, e.value.kind) == (chromosome, kind)
        out = torch.full((int(off[-1]),), -77, dtype=torch.int32, device=cv.device)
        with pytest.raises(CanvasError) as e:
            cv.partition_states(off, seg_len=to_dev(s, cv.device), nseg=n, out=out)
        msg = str(e.value)
        assert "error -1" in msg and "canvas_partition_states_cbs: chromosome %d:" % chromosome in msg, msg
        assert (out == -77).all()                               # a refused call writes no state
        return msg

    s = seg_len.copy(); s[300 + 1] = 0; s[300 + 2] = 700 - 256      # a length of 0 on chromosome 2 (the third length makes up for it: the length is what is refused)
    assert "length below 1" in refused(2, "length", s=s)
    for d in (1, -1):                                           # sums of T_c + 1 and T_c - 1
        s = seg_len.copy(); s[300 + 700 + 1] += d
        assert "must sum to its 2050 bins" in refused(3, "sum", s=s)
    n = nseg.copy(); n[0] = 301                                 # nseg > T_c: nothing of that chromosome is read
    assert "0 .. 300" in refused(0, "nseg", n=n)
    n = nseg.copy(); n[1] = 1                                   # a segment on a chromosome without bins
    refused(1, "nseg", n=n)
    n = nseg.copy(); n[3] = -1
    refused(3, "nseg", n=n)
    s = seg_len.copy(); s[0] += 5; n = nseg.copy(); n[2] = 701  # two chromosomes at fault: the first is named
    refused(0, "sum", s=s, n=n)
    # ... and the context is as good as before
    _same(cv.partition_states(off, seg_len=to_dev(seg_len, cv.device), nseg=nseg), P.states_cbs(off, seg_len, nseg), "after the refusals")


def test_breakpoint_refusals_and_argument_checks(cv):
    import torch
    from canvas_amd import CanvasError
    off = P.offsets([12, 0, 18])
    out = torch.full((30,), -77, dtype=torch.int32, device=cv.device)
    for bps, what in (([[3, 12], [], []], "breakpoint 12"), ([[3], [], [-1]], "breakpoint -1"), ([[], [0], []], "breakpoint 0"), ([[], [], [4, 18]], "breakpoint 18")):
        with pytest.raises(CanvasError) as e:
            cv.partition_states(off, breakpoints=[np.array(b, np.int32) for b in bps], out=out)
        assert "error -1" in str(e.value) and what in str(e.value), str(e.value)
        assert (out == -77).all()
    for kw in (dict(), dict(seg_len=out), dict(nseg=[0, 0, 0]), dict(seg_len=out, nseg=[0, 0, 0], breakpoints=[[], [], []]), dict(breakpoints=[[], []]), dict(seg_len=out, nseg=[0, 0])):
        with pytest.raises(CanvasError):
            cv.partition_states(off, **kw)
    # no bin at all: nothing to write, nothing launched
    assert cv.partition_states(np.zeros(3, np.int64), breakpoints=[[], []]).numel() == 0
    assert cv.partition_states(np.zeros(3, np.int64), seg_len=out, nseg=[0, 0]).numel() == 0
