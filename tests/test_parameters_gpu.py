"""The product away from the defaults of CanvasPartitionParameters.json and of the command lines: CBS across (nperm, alpha) and undo settings, Wavelets across thresholds and
MinSize, segment ids at the MaxInterBinDistInSegment bound, CanvasBin across -d, the evenness window through the tool.  Inputs and settings: tests/parameter_cases.py; that
they reach the regimes they are meant for is asserted on the oracle alone by tests/test_parameters_oracle.py.  Every comparison is exact: segment lengths, RNG consumption,
breakpoints, segment ids, bin sizes and bin rows are integers or bit patterns."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import many_contigs as M
import oracle_flows as F
import oracle_lib as O
import parameter_cases as P
from canvas_amd import synth
from gpu_common import get_canvas, to_dev, pad16

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "canvas_amd", "bin")
NAMES = synth.CHROM_NAMES


def _read(path):
    with gzip.open(path, "rt") as f:
        return f.read().splitlines()


# ---------------------------------------------------------------------------------------------------------------------------------------------------- CBS
def _cbs(cv, per, nperm, alpha, undo=0, undo_sd=3.0, dcov=None):
    """what test_cbs_gpu.py::_run asserts, at any (nperm, alpha, undo, undo_sd): segment lengths per chromosome and the counts of TMaxO calls, permutations and TPermP draws"""
    off = P.offsets(per)
    exp, est = O.cbs_genome(per, alpha, nperm, threads=8, undo=undo, undo_sd=undo_sd)
    dcov = to_dev(np.concatenate(per), cv.device) if dcov is None else dcov
    seg_len, nseg, stats = cv.cbs(dcov, off, alpha, nperm, undo=undo, undo_sd=undo_sd)
    got = seg_len.cpu().numpy()
    what = (nperm, alpha, undo, undo_sd)
    for c in range(len(per)):
        g = got[off[c]:off[c] + nseg[c]]
        assert nseg[c] == len(exp[c]) and (g == exp[c]).all(), (what, c, g[:10], exp[c][:10])
    print("cbs", what, "segments", [len(e) for e in exp], "stats", [int(v) for v in stats[:5]], "oracle", [int(v) for v in est[:5]])
    assert stats[0] == est[0] and stats[2] == est[2] and stats[4] == est[4], (what, [int(v) for v in stats[:5]], [int(v) for v in est[:5]])
    return [e.tolist() for e in exp], [int(v) for v in stats[:5]]


def test_cbs_pairs_in_sequence_on_one_context():
    """Every (nperm, alpha) pair on ONE context, then the first pair again: the per-process boundary table (one pair cached at a time) and the context's draw-stream cache are
    switched back and forth, and the answer must not depend on what ran before.  At every pair the device tail series decided some TailP calls (no silent fall-back to the
    host series), and at every pair but the degenerate one the permutation loop ran."""
    cv = get_canvas()
    per = P.cbs_genome()
    dcov = to_dev(np.concatenate(per), cv.device)
    seen = {}
    for nperm, alpha in P.CBS_PAIRS + [P.CBS_PAIRS[0]]:
        segs, stats = _cbs(cv, per, nperm, alpha, dcov=dcov)
        tp = cv.cbs_tailp_stats(); dv = cv.cbs_device_stats()
        assert tp[0] > 0, ((nperm, alpha), tp)                          # the device series decided calls
        if (nperm, alpha) != P.CBS_DEGENERATE:
            assert stats[2] > 0 and sum(len(s) for s in segs) > len(per), ((nperm, alpha), stats)
            assert dv[0] > 0, ((nperm, alpha), dv)                       # ... and permutations ran on the device
        if (nperm, alpha) in seen:
            assert seen[(nperm, alpha)] == (segs, stats)
        seen[(nperm, alpha)] = (segs, stats)
    assert seen[(10000, 0.05)][0] != seen[(10000, 0.01)][0] != seen[(10000, 0.001)][0]


@pytest.mark.parametrize("nperm,alpha", P.CBS_UNDO_PAIRS)
def test_cbs_undo_settings_away_from_the_default_alpha(nperm, alpha):
    """-s None / Prune / SDUndo, the latter also at undo_sd 1.0 and 6.0 (the reference fixes 3.0, the C ABI does not)"""
    cv = get_canvas()
    per = P.cbs_undo_genome()
    dcov = to_dev(np.concatenate(per), cv.device)
    n = {}
    for undo, sd in [(0, 3.0), (1, 3.0)] + [(2, s) for s in P.CBS_UNDO_SDS]:
        segs, _ = _cbs(cv, per, nperm, alpha, undo=undo, undo_sd=sd, dcov=dcov)
        n[(undo, sd)] = sum(len(s) for s in segs)
    assert n[(0, 3.0)] >= n[(2, 1.0)] > n[(2, 3.0)] > n[(2, 6.0)] > len(per) and n[(1, 3.0)] > len(per), n


@pytest.mark.parametrize("nperm,alpha", [(10000, 0.05), (10000, 0.001), (500, 0.002)])
def test_cbs_device_and_host_tail_series_agree(nperm, alpha, monkeypatch):
    """tail_p_decide compares the device series with alpha inside an error band and derives the number of rejections the permutation loop may still see from it:
    CANVAS_CBS_HOST_TAILP=1 takes the reference's series for every call — same segments, same statistics — and the default run did use the device series"""
    cv = get_canvas()
    per = P.cbs_genome()
    monkeypatch.delenv("CANVAS_CBS_HOST_TAILP", raising=False)
    segs, stats = _cbs(cv, per, nperm, alpha)
    tp = cv.cbs_tailp_stats()
    assert tp[0] > 0 and tp[0] >= tp[1], tp
    monkeypatch.setenv("CANVAS_CBS_HOST_TAILP", "1")
    segs2, stats2 = _cbs(cv, per, nperm, alpha)
    tp2 = cv.cbs_tailp_stats()
    assert tp2[0] == 0 and tp2[1] > 0, tp2
    assert segs2 == segs and stats2 == stats


SHARD_PAIR = (2000, 0.1)


def _free_port():
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _shard_worker(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
        import torch
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from canvas_amd import Canvas, parallel
        cv = Canvas(0)
        parallel.init_host_comm(cv, rank, world)
        res = {}
        per = P.cbs_genome()
        off = P.offsets(per)
        owner = parallel.owner_table([len(p) for p in per], world)
        d = torch.from_numpy(np.concatenate(per)).to(cv.device)
        for undo in (0, 2):
            seg_len, nseg, _ = cv.cbs_sharded(owner, d, off, SHARD_PAIR[1], SHARD_PAIR[0], undo=undo, undo_sd=1.0)
            res["cbs%d" % undo] = [seg_len.cpu().numpy()[int(off[c]):int(off[c]) + int(nseg[c])].tolist() for c in range(len(per))]
        wv = P.wv_genome()
        woff = P.offsets(wv)
        wowner = parallel.owner_table(P.WV_LENGTHS, world)
        dw = torch.from_numpy(np.concatenate(wv)).to(cv.device)
        for k, s in enumerate(P.WV_SHARDED):
            res["wv%d" % k] = [b.tolist() for b in cv.wavelets_sharded(wowner, dw, woff, is_germline=bool(k % 2), window=P.WV_WINDOW, **P.wv_device_kw(s))]
        q.put((rank, sorted(set(owner.tolist())), res))
        dist.destroy_process_group()
    except Exception:                                           # noqa: BLE001
        import traceback
        q.put((rank, "error", traceback.format_exc()))


def test_sharded_cbs_and_wavelets_away_from_the_defaults():
    """cbs_sharded at (2000, 0.1) with undo_sd 1.0 and wavelets_sharded at three settings, on two ranks of one GPU: every rank returns the oracle's answer"""
    get_canvas()
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_shard_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs: p.start()
    got = sorted([q.get(timeout=600) for _ in range(world)], key=lambda t: t[0])
    for p in procs: p.join(60)
    for g in got:
        assert g[1] != "error", g[2]
    per = P.cbs_genome(); wv = P.wv_genome()
    for rank, owners, res in got:
        assert owners == [0, 1]
        for undo in (0, 2):
            exp, _ = O.cbs_genome(per, SHARD_PAIR[1], SHARD_PAIR[0], threads=8, undo=undo, undo_sd=1.0)
            assert res["cbs%d" % undo] == [e.tolist() for e in exp], (rank, undo)
        for k, s in enumerate(P.WV_SHARDED):
            exp = O.wavelets_genome(wv, is_germline=bool(k % 2), window=P.WV_WINDOW, **s)
            assert res["wv%d" % k] == [e.tolist() for e in exp], (rank, s)


def _flow_inputs():
    """three chromosomes with weak deletions of 2 000 to 16 000 bases (every third to every eighth hit removed): change points whose acceptance depends on alpha"""
    lengths = [2_000_000, 1_200_001, 600_000]
    thr = synth.poisson_thresholds(0.21)
    rng = np.random.RandomState(1)
    bases, hits, masks = [], [], []
    for c, L in enumerate(lengths):
        b, h, m = synth.generate_chromosome(20261016 + 3, c, L, 0.21, thr)
        h = h.copy()
        for k in range(L // 100_000):
            a = int(rng.randint(0, L - 20_000)); w = int(rng.choice([2_000, 4_000, 8_000, 16_000])); drop = int(rng.choice([3, 4, 5, 6, 8]))
            h[a:a + w] = np.where(np.arange(a, a + w) % drop == 0, 0, h[a:a + w])
        bases.append(b); hits.append(h); masks.append(m)
    return bases, masks, hits


def test_partition_executable_with_cbs_alpha_from_the_config(tmp_path):
    """CanvasPartition -m CBS --config {"CBSalpha": 0.05} on the cleaned file of the oracle's germline flow: the rows of oracle_flows.germline_single(alpha = 0.05), byte for byte"""
    get_canvas()
    bases, masks, hits = _flow_inputs()
    E = F.germline_single(bases, masks, hits, [1, 1, 1], NAMES, alpha=0.05)
    E0 = F.germline_single(bases, masks, hits, [1, 1, 1], NAMES, alpha=0.01)
    assert E["partitioned_cbs_rows"] != E0["partitioned_cbs_rows"] and E["cbs_stats"][2] > 0          # alpha decides the file
    cleaned = str(tmp_path / "S.cleaned"); part = str(tmp_path / "S.partitioned"); cfg = str(tmp_path / "CanvasPartitionParameters.json")
    with gzip.open(cleaned, "wt") as f:
        f.write("\n".join(E["cleaned_rows"]) + "\n")
    open(cfg, "w").write('{\n  "CBSalpha": 0.05\n}\n')
    r = subprocess.run([os.path.join(BIN, "CanvasPartition"), "-i", cleaned, "-o", part, "-r", str(tmp_path), "-m", "CBS", "--config", cfg], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert _read(part) == E["partitioned_cbs_rows"]
    r = subprocess.run([os.path.join(BIN, "CanvasPartition"), "-i", cleaned, "-o", part, "-r", str(tmp_path), "-m", "CBS"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert _read(part) == E0["partitioned_cbs_rows"]


# ------------------------------------------------------------------------------------------------------------------------------------------------ Wavelets
def _wavelets(cv, per, germline, s, window):
    exp = O.wavelets_genome(per, is_germline=germline, window=window, **s)
    got = cv.wavelets(to_dev(np.concatenate(per), cv.device), P.offsets(per), is_germline=germline, window=window, **P.wv_device_kw(s))
    n = [len(e) for e in exp]
    print("wavelets", s, "germline", germline, "oracle breakpoints per chromosome", n)
    assert len(got) == len(exp)
    for c in range(len(per)):
        assert got[c].tolist() == exp[c].tolist(), (s, germline, c, len(got[c]), n)
    assert cv.wavelets_stats()[1] == 0, (s, germline)
    return n


@pytest.mark.parametrize("germline", [False, True])
@pytest.mark.parametrize("setting", P.WV_SETTINGS, ids=lambda s: ",".join("%s=%g" % kv for kv in s.items()) or "default")
def test_wavelets_thresholds_and_min_size(setting, germline):
    """Oracle breakpoints over chromosomes of 40 000 / 9 001 / 300 / 11 / 10 bins (not germline): MadFactor 50: 23, 5 (default): 32, 0.5: 2 739, 0.05: 41 090, 0: 47 551;
    threshold_upper 1: 28 738; thresholds 0: 47 594; threshold_lower 500: 7 — from a handful of candidates per chromosome to one per bin"""
    cv = get_canvas()
    _wavelets(cv, P.wv_genome(), germline, setting, P.WV_WINDOW)


def test_wavelets_low_threshold_on_a_long_chromosome():
    """1.2 M bins at MadFactor 0.5: 18 116 breakpoints in the oracle against 59 at the default — the candidate, root and long-node lists hold thousands of times what a default
    run puts into them"""
    cv = get_canvas()
    n = _wavelets(cv, P.wv_big(), False, dict(mad_factor=0.5), 100000)
    assert n[0] > 10_000


def test_partition_executable_with_wavelets_thresholds_from_the_config(tmp_path):
    """CanvasPartition (Wavelets, the default method) with "MadFactor": 0.5 and with "ThresholdLowerMaf": 2.0 in --config"""
    get_canvas()
    per0 = P.wv_genome()
    nchr = len(per0)
    per = [F.f2_double(np.asarray(p, np.float32)) for p in per0]                   # the doubles the tool parses from the F2 text
    bs = [(10_000 + 1000 * np.arange(len(p))).astype(np.uint32) for p in per]; be = [b + 1000 for b in bs]
    cleaned = str(tmp_path / "S.cleaned"); part = str(tmp_path / "S.partitioned"); vaf = str(tmp_path / "S.vaf"); open(vaf, "w").write("")
    with gzip.open(cleaned, "wt") as f:
        for c in range(nchr):
            for s, e, v in zip(bs[c], be[c], per0[c]):
                f.write(f"{NAMES[c]}\t{s}\t{e}\t{O.format_f2(float(np.float32(v)))}\t41\n")
    seen = {}
    for js, kw in (('{"EvennessScoreWindow": 1000}', {}), ('{"MadFactor": 0.5, "EvennessScoreWindow": 1000}', dict(mad_factor=0.5)),
                   ('{"ThresholdLowerMaf": 2.0, "EvennessScoreWindow": 1000}', dict(thr_lower=2.0)), ('{"ThresholdLowerMaf": 2.0, "MadFactor": 0.5, "EvennessScoreWindow": 1000}', dict(mad_factor=0.5, thr_lower=2.0))):
        cfg = str(tmp_path / "params.json"); open(cfg, "w").write(js)
        for germline in (False, True):
            r = subprocess.run([os.path.join(BIN, "CanvasPartition"), "-i", cleaned, "-o", part, "-r", str(tmp_path), "-v", vaf, "--config", cfg] + (["-g"] if germline else []),
                               capture_output=True, text=True)
            assert r.returncode == 0, r.stdout + r.stderr
            bps = O.wavelets_genome(per, is_germline=germline, window=1000, **kw)
            wstarts = [bs[c][bps[c]].astype(np.uint32) if (len(bps[c]) >= 2 and len(bs[c]) > 10) else bs[c][:1].astype(np.uint32) for c in range(nchr)]
            ids, _ = O.postprocess(bs, be, wstarts)
            rows = [f"{NAMES[c]}\t{s_}\t{e_}\t{O.format_g15(float(v))}\t{i}" for c in range(nchr) for s_, e_, v, i in zip(bs[c], be[c], per[c], ids[c])]
            assert _read(part) == rows, (js, germline)
            seen[(germline, tuple(sorted(kw)))] = rows
    for g in (False, True):
        # MadFactor 0.5 changes the file; the lower clamp at 2.0 lies below the default threshold (same file) and above the one MadFactor 0.5 gives (another file)
        assert seen[(g, ())] != seen[(g, ("mad_factor",))] != seen[(g, ("mad_factor", "thr_lower"))] and seen[(g, ("thr_lower",))] == seen[(g, ())]


# ------------------------------------------------------------------------------------------------------------------------------------ segment ids at the gap bound
@pytest.mark.parametrize("D", P.GAP_DISTS)
def test_segment_ids_at_the_gap_bound(D):
    """gaps of MaxInterBinDistInSegment - 1, equal and + 1 inside state runs, at a state change, at the first and last bin of a chromosome, next to an excluded interval and next to a
    ploidy record: canvas_segment_ids, _filtered and _ploidy against PostProcessSegments; a bound one off in either direction gives other ids (test_parameters_oracle.py)"""
    cv = get_canvas()
    case = P.gap_case(D)
    state = to_dev(case["state"], cv.device); ds = to_dev(case["start"], cv.device); de = to_dev(case["stop"], cv.device)
    for dist in (D, D + 1, max(0, D - 1)):
        for with_excl, with_ploidy in ((False, False), (True, False), (False, True), (True, True)):
            ids, last = P.gap_expected(case, dist, with_excl, with_ploidy)
            seg, nseg = cv.segment_ids(case["off"], state, ds, de, dist, excluded=case["excl"] if with_excl else None, ploidy=case["ploidy"] if with_ploidy else None)
            got = seg.cpu().numpy()
            assert (got == np.concatenate(ids)).all(), (dist, with_excl, with_ploidy, np.nonzero(got != np.concatenate(ids))[0][:8])
            assert nseg == last + 1


def test_partition_executable_with_max_inter_bin_dist_from_the_config(tmp_path):
    """CanvasPartition -m PerSampleHMM -b filter.bed --config {"MaxInterBinDistInSegment": 1000} on bins with gaps of 999, 1000 and 1001"""
    get_canvas()
    case = P.gap_case(1000)
    off = case["off"]; nchr = len(off) - 1
    rng = np.random.RandomState(7)
    cov = np.round(rng.normal(100, 8, int(off[-1])), 2)
    cov[int(off[0]) + 12:int(off[0]) + 26] *= 0.5                  # a deletion on chr0 for the HMM to find
    per = [F.f2_double(np.asarray(cov[off[c]:off[c + 1]], np.float32)) for c in range(nchr)]
    bs = [case["start"][off[c]:off[c + 1]].astype(np.uint32) for c in range(nchr)]; be = [case["stop"][off[c]:off[c + 1]].astype(np.uint32) for c in range(nchr)]
    cleaned = str(tmp_path / "S.cleaned"); part = str(tmp_path / "S.partitioned"); bed = str(tmp_path / "filter.bed"); cfg = str(tmp_path / "params.json")
    with gzip.open(cleaned, "wt") as f:
        for c in range(nchr):
            for s, e, v in zip(bs[c], be[c], cov[off[c]:off[c + 1]]):
                f.write(f"{NAMES[c]}\t{s}\t{e}\t{O.format_f2(float(np.float32(v)))}\t41\n")
    with open(bed, "w") as f:
        for c in range(nchr):
            for a, b in zip(*case["excl"][c]): f.write(f"{NAMES[c]}\t{a}\t{b}\n")
    paths, ran = O.hmm_genome_per_sample(per, threads=4)
    starts = [O.segments_from_path(paths[c], ran[c], bs[c], be[c])[0] for c in range(nchr)]
    rows = {}
    for D in (1000, 1000000):
        ids, _ = O.postprocess(bs, be, starts, case["excl"], D)
        rows[D] = [f"{NAMES[c]}\t{s_}\t{e_}\t{O.format_g15(float(v))}\t{i}" for c in range(nchr) for s_, e_, v, i in zip(bs[c], be[c], per[c], ids[c])]
    assert rows[1000] != rows[1000000]
    for D, extra in ((1000, ["--config", cfg]), (1000000, [])):
        open(cfg, "w").write('{"MaxInterBinDistInSegment": 1000}')
        r = subprocess.run([os.path.join(BIN, "CanvasPartition"), "-i", cleaned, "-o", part, "-r", str(tmp_path), "-m", "PerSampleHMM", "-b", bed] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert _read(part) == rows[D], D


# ---------------------------------------------------------------------------------------------------------------------------------------------- CanvasBin -d
ALL = O.CLEAN_GCNORM | O.CLEAN_FILTSIZE | O.CLEAN_OUTLIERS | O.CLEAN_LOCALSD


def _bin_buffers(cv, cap):
    import torch
    mk = lambda dt: torch.empty(cap, dtype=dt, device=cv.device)
    return dict(chr=mk(torch.int32), start=mk(torch.int32), stop=mk(torch.int32), gc=mk(torch.int32), count=mk(torch.float32))


def _check_bins(out, per, total, exp, what):
    eper = np.array([len(e[0]) for e in exp], np.int64)
    cat = lambda j: np.concatenate([e[j] for e in exp])
    e = dict(chr=np.repeat(np.arange(len(exp), dtype=np.int32), eper), start=cat(0), stop=cat(1), gc=cat(2), count=cat(3).astype(np.float32))
    assert total == len(e["chr"]), (what, total, len(e["chr"]))
    assert np.asarray(per).tolist() == eper.tolist(), (what, np.nonzero(np.asarray(per) != eper)[0][:8])
    for k in ("chr", "start", "stop", "gc"):
        got = out[k][:total].cpu().numpy()
        assert (got == e[k]).all(), (what, k, np.nonzero(got != e[k])[0][:8])
    got = out["count"][:total].cpu().numpy()
    assert (got.view(np.uint32) == e["count"].view(np.uint32)).all(), (what, np.nonzero(got != e["count"])[0][:8])


@pytest.fixture(scope="module")
def bin_genome_inputs():
    data, is_auto = M.genome(P.BIN_NCHR)
    rates = O.bin_rates_genome([d[2] for d in data], [d[1] for d in data], threads=8)
    rng = np.random.RandomState(P.BIN_NCHR)
    fl = [np.where(d[1] > 0, np.clip(rng.normal(330, 60, len(d[1])), 1, 5000), 0).astype(np.int16) for d in data]
    return data, is_auto, rates, fl


@pytest.mark.parametrize("depth", P.BIN_DEPTHS)
def test_bin_sample_across_counts_per_bin(depth, bin_genome_inputs):
    """canvas_bin_sample, _packed and _gcweighted derive the bin size from -d on the device: bin size, bins per chromosome and rows at 1, 7, 100, 1000 counts per bin and at a depth
    whose bin is longer than the shortest primary chromosome's unique positions"""
    cv = get_canvas()
    data, is_auto, rates, fl = bin_genome_inputs
    bases_h = [d[0] for d in data]; hits_h = [d[1] for d in data]; masks_h = [d[2] for d in data]
    lens = np.array([len(b) for b in bases_h], np.int64)
    bs = O.bin_size(rates[is_auto == 1], depth)
    exp = [O.bin_chromosome(b, m, h, bs, 3) for b, h, m in data]
    print("depth", depth, "bin size", bs, "bins", sum(len(e[0]) for e in exp))
    db = [to_dev(pad16(b), cv.device) for b in bases_h]; dh = [to_dev(pad16(h), cv.device) for h in hits_h]; dm = [to_dev(m.view(np.int64), cv.device) for m in masks_h]
    out = _bin_buffers(cv, int(lens.sum() // bs) + len(data) + 64)
    obs, poss, grate = cv.bin_rates(dh, dm, lens)
    assert cv.bin_size_from_rates(grate[is_auto == 1], depth) == bs
    o, per, total, gbs = cv.bin_sample(db, dm, dh, lens, is_auto, depth, -1, 3, out=out)
    assert gbs == bs, (depth, gbs, bs)
    _check_bins(out, per, total, exp, ("bin_sample", depth))
    dref, dpl, pos0, _ = cv.pack_genome_device(db, dm, dh, lens)
    o, per, total, gbs = cv.bin_sample_packed(dref, dpl, lens, pos0, is_auto, depth, -1, 3, out=out)
    assert gbs == bs, (depth, gbs, bs)
    _check_bins(out, per, total, exp, ("bin_sample_packed", depth))
    gexp, _, _, _ = O.bin_gc_weighted(bases_h, masks_h, hits_h, fl, bs)
    dfl = [to_dev(pad16(f), cv.device) for f in fl]
    o, per, total, gbs = cv.bin_sample_gcweighted(db, dm, dh, dfl, lens, is_auto, depth, -1, out=out)
    assert gbs == bs, (depth, gbs, bs)
    _check_bins(out, per, total, gexp, ("bin_sample_gcweighted", depth))


def _oracle_pipeline(data, is_auto, depth):
    """the oracle's chain behind canvas_sample_pipeline at `depth` counts per bin: rates -> bin size -> bins -> CanvasClean (-g -s -r, local SD) -> F2 -> PerSampleHMM -> segment ids"""
    nchr = len(data)
    bases_h = [d[0] for d in data]; hits_h = [d[1] for d in data]; masks_h = [d[2] for d in data]
    rates = O.bin_rates_genome(masks_h, hits_h, threads=8)
    bs = O.bin_size(rates[is_auto == 1], depth)
    st, en, gc, cnt = O.bin_genome(bases_h, masks_h, hits_h, bs, 3, threads=8)
    B = dict(chr=np.concatenate([np.full(len(st[c]), c, np.int32) for c in range(nchr)]), start=np.concatenate(st), stop=np.concatenate(en), gc=np.concatenate(gc),
             count=np.concatenate(cnt).astype(np.float32))
    ex = O.clean(B["chr"], B["start"], B["stop"], B["count"], B["gc"], is_auto, np.zeros(nchr, np.uint8), ALL)
    cov = F.f2_double(ex["count"])
    off = M.offsets(ex["chr"], nchr)
    per = [np.ascontiguousarray(cov[off[c]:off[c + 1]]) for c in range(nchr)]
    paths, ran = O.hmm_genome_per_sample(per, threads=8)
    bsr = [ex["start"][off[c]:off[c + 1]].astype(np.uint32) for c in range(nchr)]; ber = [ex["stop"][off[c]:off[c + 1]].astype(np.uint32) for c in range(nchr)]
    ids, last = O.postprocess(bsr, ber, [O.segments_from_path(paths[c], ran[c], bsr[c], ber[c])[0] for c in range(nchr)])
    state = np.concatenate([paths[c] if ran[c] else np.full(len(per[c]), -1, np.int32) for c in range(nchr)])
    return dict(bin_size=bs, total=len(B["chr"]), n_out=len(ex["chr"]), nseg=last + 1, off=off, cleaned=ex, cov=cov, state=state, seg=np.concatenate(ids))


@pytest.mark.parametrize("depth", P.BIN_DEPTHS)
def test_sample_pipeline_across_counts_per_bin(depth, bin_genome_inputs):
    """canvas_sample_pipeline (bin -> clean -> F2 -> PerSampleHMM -> segment ids in one call) at each depth against the oracle's chain"""
    import torch
    cv = get_canvas()
    data, is_auto, _, _ = bin_genome_inputs
    E = _oracle_pipeline(data, is_auto, depth)
    print("depth", depth, "bin size", E["bin_size"], "bins", E["total"], "after clean", E["n_out"], "segments", E["nseg"])
    lens = np.array([len(d[0]) for d in data], np.int64)
    db = [to_dev(pad16(d[0]), cv.device) for d in data]; dh = [to_dev(pad16(d[1]), cv.device) for d in data]; dm = [to_dev(d[2].view(np.int64), cv.device) for d in data]
    cap = int(lens.sum() // E["bin_size"]) + len(data) + 64
    out = _bin_buffers(cv, cap)
    dcov = torch.empty(cap, dtype=torch.float64, device=cv.device); dst = torch.empty(cap, dtype=torch.int32, device=cv.device); dseg = torch.empty(cap, dtype=torch.int32, device=cv.device)
    if E["n_out"] < 5:
        # PerSampleHMM takes quartiles of the whole sample's coverage: the reference throws on fewer than 5 bins, and the product refuses the sample
        from canvas_amd.lib import CanvasError
        with pytest.raises(CanvasError, match="fewer than 5 bins"):
            cv.sample_pipeline(db, dm, dh, lens, is_auto, out, dcov, dst, dseg, counts_per_bin=depth, bin_size=-1, mode=3, flags=ALL)
        assert depth == P.BIN_DEPTHS[-1]
        return
    r = cv.sample_pipeline(db, dm, dh, lens, is_auto, out, dcov, dst, dseg, counts_per_bin=depth, bin_size=-1, mode=3, flags=ALL)
    cv.synchronize()
    n = E["n_out"]; ex = E["cleaned"]
    assert (r["bin_size"], r["total"], r["n_out"], r["nseg"]) == (E["bin_size"], E["total"], n, E["nseg"])
    assert list(r["off"]) == E["off"].tolist()
    assert np.float64(r["lsd"]).view(np.uint64) == np.float64(ex["local_sd"]).view(np.uint64)
    for k in ("chr", "start", "stop", "gc"):
        assert (out[k][:n].cpu().numpy() == ex[k]).all(), k
    assert (out["count"][:n].cpu().numpy().view(np.uint32) == ex["count"].view(np.uint32)).all()
    assert (dcov[:n].cpu().numpy().view(np.uint64) == E["cov"].view(np.uint64)).all()
    assert (dst[:n].cpu().numpy() == E["state"]).all()
    assert (dseg[:n].cpu().numpy() == E["seg"]).all()


def test_canvasbin_executable_at_depth_7(tmp_path):
    """CanvasBin -d 7 on three chromosomes' intermediate files: the bin size from the autosomes' rates, the rows of the oracle"""
    get_canvas()
    import test_canvasbin_tool_gpu as T
    rng = np.random.RandomState(77)
    refs = [("chr1", 60_003), ("chr2", 41_000), ("chrX", 24_000)]
    fa = str(tmp_path / "genome.fa"); seqs = {}
    with open(fa, "w") as f:
        for n, L in refs:
            seqs[n] = rng.choice(np.frombuffer(b"ACGTacgt", np.uint8), L, p=[0.2, 0.2, 0.2, 0.2, 0.05, 0.05, 0.05, 0.05])
            f.write(f">{n}\n" + seqs[n].tobytes().decode() + "\n")
    bam = str(tmp_path / "S.bam")
    T._write_bam(bam, refs, [dict(ref=0, pos=100, flag=0x1 | 0x2 | 0x40, cigar=[(36, "M")], tlen=300), dict(ref=-1, pos=-1, flag=0x4 | 0x1, cigar=[], tlen=0)])
    args = []; mk, hk = [], []
    for n, L in refs:
        stored = rng.randint(0, 256, (L + 7) // 8).astype(np.uint8)
        m_read = T._lsb_unpack(stored.tobytes(), L % 8)
        h = (rng.poisson(0.3 if n != "chrX" else 0.9, L) * m_read).astype(np.uint8)
        dat = str(tmp_path / f"{n}.dat")
        open(dat, "wb").write(T._encode_dat(n, stored.tobytes(), h.tobytes(), L % 8))
        args += ["-i", dat]; mk.append(np.packbits(m_read, bitorder="little")); hk.append(h)
    names = [n for n, _ in refs]
    rates = [O.bin_rate(hk[c], mk[c]) for c in (0, 1)]                       # the autosomes; chrX has three times the rate
    got_sizes = []
    for depth in (7, 100):
        bs = O.bin_size(rates, depth); got_sizes.append(bs)
        binned = str(tmp_path / f"S.{depth}.binned")
        r = subprocess.run([os.path.join(BIN, "CanvasBin"), "-b", bam, "-r", fa, "-o", binned, "-d", str(depth), "-m", "TruncatedDynamicRange"] + args, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        res = O.bin_genome([seqs[n] for n in names], mk, hk, bs, mode=3, threads=2)
        exp = [f"{n}\t{s}\t{e}\t{O.format_f2(float(k))}\t{g}" for c, n in enumerate(names) for s, e, g, k in zip(res[0][c], res[1][c], res[2][c], res[3][c])]
        assert _read(binned) == exp, depth
        r = subprocess.run([os.path.join(BIN, "CanvasBin"), "-b", bam, "-r", fa, "-o", binned, "-d", str(depth), "-y", "-m", "TruncatedDynamicRange"] + args, capture_output=True, text=True)
        assert r.returncode == 0 and open(binned + ".binsize").read() == str(bs)
    assert got_sizes[0] < got_sizes[1] and got_sizes[0] < 60
    assert O.bin_size([O.bin_rate(hk[c], mk[c]) for c in range(3)], 100) != got_sizes[1]          # chrX is no autosome: its rate would move the bin size


# ------------------------------------------------------------------------------------------------------------------------------------ evenness window, tool
@pytest.mark.parametrize("window", [1500, 10_001])
def test_evenness_window_from_the_config_on_the_somatic_command_line(tmp_path, window):
    """Somatic-WGS command line (CanvasRunner.cs:954-961) with "EvennessScoreWindow" in --config: the metric file holds GetEvennessScore at that window"""
    get_canvas()
    import test_partition_runner_cli_gpu as R
    nchr = 24
    bins, cov = R._sample(20260927 + 54, 160_000, nchr)
    cleaned = tmp_path / "S.cleaned"; part = tmp_path / "S.partitioned"; snv = tmp_path / "VFResultsS.txt.gz"; bed = tmp_path / "filter.bed"; vcf = tmp_path / "ploidy.vcf"
    ref = tmp_path / "WholeGenomeFasta"; ref.mkdir()
    R._write_cleaned(str(cleaned), bins, cov); open(snv, "w").write("")
    excl = R._filter_bed(str(bed), bins, nchr, 4)
    R._ploidy_vcf(str(vcf), bins, nchr)
    per, bs, be, ex_list, off = R._after_filter(bins, cov, excl, nchr)
    ev = tmp_path / "EvennessMetric.txt"; cfg = tmp_path / "CanvasPartitionParameters.json"
    open(cfg, "w").write('{"EvennessScoreWindow": %d}' % window)
    cmd = f" -v {snv} " + f"-i \"{cleaned}\" " + f"-b \"{bed}\" " + f"-o \"{part}\" " + f" -r \"{ref}\" " + f" -p \"{vcf}\" " + f"--evenness-metric-file \"{ev}\" " + f"--config {cfg}"
    r = R._run(cmd)
    assert r.returncode == 0, r.stdout + r.stderr
    score = O.evenness_score(per, window)
    assert score is not None and max(len(p) for p in per) > window
    assert score != O.evenness_score(per, 3000)
    assert open(ev).read() == "#evenness\t" + O.format_g15(score) + "\n"
