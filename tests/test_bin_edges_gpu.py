"""The CanvasBin kernels at their tile, pos0, wrap and grid edges (tests/bin_edge_cases.py; test_bin_edge_cases.py shows that every case reaches its edge) against the
CPU oracle, chromosome by chromosome and bit for bit: integer work, no tolerance anywhere.  Both device paths of the byte arrays, and the packed planes where named."""
import time

import numpy as np
import pytest

import bin_edge_cases as B
import oracle_lib as O
from gpu_common import get_canvas, to_dev
from test_bin_gpu import _upload
from test_bin_packed_gpu import _host_planes

pytestmark = pytest.mark.gpu

PATHS = ("two_pass", "single_read")
FIELDS = ("start", "stop", "gc", "count")


def _set_path(monkeypatch, path):
    monkeypatch.delenv("CANVAS_BIN_SINGLE_READ", raising=False); monkeypatch.delenv("CANVAS_BIN_TWO_PASS", raising=False)
    monkeypatch.setenv("CANVAS_BIN_SINGLE_READ" if path == "single_read" else "CANVAS_BIN_TWO_PASS", "1")


@pytest.fixture(params=PATHS)
def bin_path(request, monkeypatch):
    """both CanvasBin device paths of the byte arrays (as in test_bin_gpu.py): k_tile_stats + k_bin_pass, and k_tile_summary + k_bin_close2 + k_bin_resolve_fin"""
    _set_path(monkeypatch, request.param)
    return request.param


_expected, _device = {}, {}


def expected(case, bs, mode):
    """the oracle's bins of every chromosome of a case, computed once: (bins per chromosome, {field: all chromosomes' values end to end})"""
    key = (case.name, bs, mode)
    if key not in _expected:
        per = [O.bin_chromosome(b, m, h, bs, mode) for b, h, m in case.data]
        cat = {k: np.concatenate([p[j] for p in per]) for j, k in enumerate(FIELDS)}
        _expected[key] = (np.array([len(p[0]) for p in per], np.int64), cat)
    return _expected[key]


def uploaded(cv, case):
    """the device arrays of the case run last (one genome at a time stays on the device)"""
    if case.name not in _device:
        _device.clear()
        _device[case.name] = _upload(cv, case.data)
    return _device[case.name]


def make_out(cv, cap):
    import torch
    mk = lambda dt: torch.empty(cap, dtype=dt, device=cv.device)
    return dict(chr=mk(torch.int32), start=mk(torch.int32), stop=mk(torch.int32), gc=mk(torch.int32), count=mk(torch.float32))


def check(out, per, total, case, bs, mode, what=""):
    eper, cat = expected(case, bs, mode)
    per = np.asarray(per, np.int64)
    assert per.tolist() == eper.tolist(), (what, case.name, bs, mode, np.nonzero(per != eper)[0][:8])
    assert total == int(eper.sum()), (what, case.name, bs, mode, total)
    chrom = np.repeat(np.arange(len(eper)), eper)
    got = out["chr"][:total].cpu().numpy()
    assert (got == chrom).all(), (what, case.name, bs, mode, "chr", np.nonzero(got != chrom)[0][:8])
    for k in FIELDS:
        got = out[k][:total].cpu().numpy()
        exp = cat[k].astype(np.float32) if k == "count" else cat[k]
        bad = np.nonzero(got != exp)[0]
        assert len(bad) == 0, (what, case.name, bs, mode, k, "chromosomes", np.unique(chrom[bad])[:8], "bins", bad[:8], got[bad[:8]], exp[bad[:8]])


def run_given_sizes(cv, case):
    bases, hits, masks = uploaded(cv, case)
    lens = B.case_lens(case)
    for bs in case.bin_sizes:
        for mode in case.modes:
            out, per, total = cv.bin_genome(bases, masks, hits, lens, bs, mode)
            check(out, per, total, case, bs, mode)


def run_derived_size(cv, case, mode=3):
    """bin_sample with the bin size derived from the autosomes' rates -> (out, per, total, bin size)"""
    bases, hits, masks = uploaded(cv, case)
    lens = B.case_lens(case)
    return cv.bin_sample(bases, masks, hits, lens, case.is_auto, case.counts_per_bin, -1, mode, out=make_out(cv, int(lens.sum()) + 8))


def packed_planes(cv, case):
    href, hpl, pos0, _ = _host_planes(case.data)
    assert pos0.tolist() == [B.pos0_of(b) for b, h, m in case.data]
    return [to_dev(r.view(np.int64), cv.device) for r in href], [to_dev(p.view(np.int64), cv.device) for p in hpl], pos0


def run_packed(cv, case, mode=3):
    dref, dpl, pos0 = packed_planes(cv, case)
    lens = B.case_lens(case)
    for bs in case.bin_sizes:
        out = make_out(cv, int(lens.sum()) // bs + 8)
        _, per, total, got_bs = cv.bin_sample_packed(dref, dpl, lens, pos0, case.is_auto, case.counts_per_bin, bs, mode, out=out)
        assert got_bs == bs
        check(out, per, total, case, bs, mode, "packed")


def test_pos0_everywhere_in_a_tile_and_behind_the_first_stride_trip(bin_path):
    cv = get_canvas()
    case = B.group1_pos0()
    run_given_sizes(cv, case)
    bases, hits, masks = uploaded(cv, case)
    obs, poss, rate = cv.bin_rates(hits, masks, B.case_lens(case))
    for c, (b, h, m) in enumerate(case.data):                       # the positions in front of pos0 count for the rates
        assert (obs[c], poss[c]) == (len(b), len(b)) and rate[c] == O.bin_rate(h, m)
    for mode in case.modes:
        out, per, total, bs = run_derived_size(cv, case, mode)
        assert bs == O.bin_size(rate, case.counts_per_bin) == 100
        check(out, per, total, case, bs, mode, "derived size")


def test_saturated_words_do_not_carry_between_the_packed_fields(bin_path):
    run_given_sizes(get_canvas(), B.group2_saturation())


def test_bins_closing_on_word_tile_and_chromosome_ends(bin_path):
    run_given_sizes(get_canvas(), B.group3_stops())


def test_bin_sizes_around_powers_of_two_and_above_a_tile(bin_path):
    cv = get_canvas()
    case = B.group4_sizes()
    run_given_sizes(cv, case)
    bases, hits, masks = uploaded(cv, case)
    out, per, total = cv.bin_genome(bases, masks, hits, B.case_lens(case), case.meta["too_large"], 3)       # more than the chromosome holds: no bin, no error
    assert total == 0 and per.tolist() == [0]


def test_resolve_kernel_second_stride_trip(bin_path):
    import torch
    cv = get_canvas()
    case = B.group5a_stride()
    assert torch.cuda.get_device_properties(cv.device).multi_processor_count * 8 * 255 < case.meta["bins"]       # more bins than one trip of the resident workgroups takes
    run_given_sizes(cv, case)


def test_resolve_kernel_second_stride_trip_packed():
    import torch
    cv = get_canvas()
    case = B.group5a_stride()
    assert torch.cuda.get_device_properties(cv.device).multi_processor_count * 8 * 255 < case.meta["bins"]
    run_packed(cv, case)


def test_chromosome_firsts_on_the_resolve_kernels_group_slots(bin_path):
    run_given_sizes(get_canvas(), B.group5b_slots())


def test_chromosome_firsts_on_the_resolve_kernels_group_slots_packed():
    run_packed(get_canvas(), B.group5b_slots())


def test_prefixes_past_two_to_the_32_and_two_scan_chunks(bin_path):
    cv = get_canvas()
    t0 = time.perf_counter()
    run_given_sizes(cv, B.group6_wrap())
    print("group 6 (%s): %.1f s" % (bin_path, time.perf_counter() - t0))


def _run_both_paths(cv, case, monkeypatch):
    res = {}
    for path in PATHS:
        _set_path(monkeypatch, path)
        res[path] = run_derived_size(cv, case)
    return res


@pytest.mark.parametrize("case", [c for c in B.group7_decisions() if c.meta["kind"] == "size"], ids=lambda c: c.name.replace(" ", "_").replace(",", ""))
def test_device_decisions_match_the_oracle(case, monkeypatch):
    """the bin size from the autosomes' rates as k_tscan_apply's last workgroup derives it (single_read; needRates takes that path by default) and as the host does (two_pass)"""
    import torch
    cv = get_canvas()
    rates = [O.bin_rate(h, m) for (b, h, m), a in zip(case.data, case.is_auto) if a]
    bs_exp = O.bin_size(rates, case.counts_per_bin)
    res = _run_both_paths(cv, case, monkeypatch)
    for path in PATHS:
        out, per, total, bs = res[path]
        assert bs == bs_exp, (path, bs, bs_exp)
        check(out, per, total, case, bs, 3, path)
    (o1, p1, t1, _), (o2, p2, t2, _) = res["two_pass"], res["single_read"]
    assert t1 == t2 and p1.tolist() == p2.tolist()
    for k in o1:
        assert torch.equal(o1[k][:t1], o2[k][:t1]), k


@pytest.mark.parametrize("case", [c for c in B.group7_decisions() if c.meta["kind"] == "bad_rate"], ids=lambda c: c.name.replace(" ", "_").replace(",", ""))
def test_non_finite_rate_is_decided_alike_on_both_paths(case, monkeypatch):
    """an autosome without a possible position: both paths hand the rate list to the host's sort; they agree with each other and with bin_size_from_rates"""
    import torch
    cv = get_canvas()
    bases, hits, masks = uploaded(cv, case)
    obs, poss, rate = cv.bin_rates(hits, masks, B.case_lens(case))
    auto_rates = [r for r, a in zip(rate, case.is_auto) if a]
    assert not np.isfinite(auto_rates).all()
    bs_exp = cv.bin_size_from_rates(auto_rates, case.counts_per_bin)
    assert bs_exp > 0
    res = _run_both_paths(cv, case, monkeypatch)
    (o1, p1, t1, b1), (o2, p2, t2, b2) = res["two_pass"], res["single_read"]
    assert b1 == b2 == bs_exp and t1 == t2 and p1.tolist() == p2.tolist()
    for k in o1:
        assert torch.equal(o1[k][:t1], o2[k][:t1]), k
    check(o1, p1, t1, case, bs_exp, 3)                               # and the bins of that size are the oracle's


@pytest.mark.parametrize("kind", ["no autosome", "not positive"])
def test_nothing_to_derive_a_bin_size_from_raises(kind, bin_path):
    from canvas_amd.lib import CanvasError
    cv = get_canvas()
    case, = [c for c in B.group7_decisions() if c.meta["kind"] == kind]
    with pytest.raises(CanvasError, match=kind):
        run_derived_size(cv, case)


def test_lone_bytes_above_the_clamp_and_every_base_byte(bin_path):
    cv = get_canvas()
    case = B.group8_bytes()
    run_given_sizes(cv, case)
    bases, hits, masks = uploaded(cv, case)
    obs, poss, rate = cv.bin_rates(hits, masks, B.case_lens(case))
    for c, (b, h, m) in enumerate(case.data):                       # nonzero_bytes4
        assert obs[c] == int((h > 0).sum()) and poss[c] == int(B.mask_bits(m, len(b)).sum()) and rate[c] == O.bin_rate(h, m)
