"""The flows over the partition states: (a) cbs / wavelets -> partition_states -> segment_ids -> segment_tables on the device equals Segments.ReadSegments of the
*.partitioned file the CanvasPartition executable writes with -m CBS and -m Wavelets, plain and with -b and -p; (b) Canvas.call_somatic_ids gives every output of
Canvas.call_somatic on the cases of tests/somatic_call_cases.py expanded to per-bin arrays; (c) Canvas.germline_flow with method "cbs" / "wavelets" equals the separately
issued calls, and "hmm" the call without a method; (d) Canvas.somatic_flow equals tumor_normal_flow followed by the separate steps."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import segment_tables_ref as S
import somatic_call_cases as C
from canvas_amd import synth, CanvasError, CLEAN_GCNORM, CLEAN_FILTSIZE, CLEAN_OUTLIERS, CLEAN_LOCALSD
from gpu_common import get_canvas, to_dev, pad16
from test_germline_flow_gpu import per_bin, same_outputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "canvas_amd", "bin", "CanvasPartition")
Z2 = (np.zeros(0, np.int32),) * 2
Z3 = (np.zeros(0, np.int32),) * 3


@pytest.fixture(scope="module")
def cv():
    return get_canvas()


# ---------------------------------------------------------------------------------------------------------------- (a) the executable
@pytest.fixture(scope="module")
def hand_off(tmp_path_factory):
    """the input of test_germline_flow_gpu.py::test_segment_tables_reproduce_the_text_hand_off, a -b BED file and a -p ploidy VCF for it"""
    d = tmp_path_factory.mktemp("partition_flows")
    nchr = 3
    bins = synth.generate_bins(20260927 + 81, 4000, nchr=nchr)
    count = bins["count"].astype(np.float32)
    for a, b, f in ((300, 520, 0.5), (1500, 1900, 1.5), (2600, 2610, 0.5), (3300, 3900, 2.0)):      # copy-number steps: without them every chromosome is one segment
        count[a:b] *= np.float32(f)
    text = [O.format_f2(float(v)) for v in count]
    cleaned = d / "S.cleaned"; ref = d / "WholeGenomeFasta"; ref.mkdir(); vaf = d / "VFResultsS.txt.gz"; vaf.write_text("")
    with gzip.open(cleaned, "wt") as f:
        for c, s, e, v, g in zip(bins["chr"], bins["start"], bins["stop"], text, bins["gc"]):
            f.write(f"{synth.CHROM_NAMES[c]}\t{s}\t{e}\t{v}\t{g}\n")
    rng = np.random.RandomState(3)
    excluded = []
    with open(d / "filter.bed", "w") as f:
        for c in range(nchr):
            idx = np.nonzero(bins["chr"] == c)[0]
            pick = np.sort(rng.choice(len(idx) - 2, 5, replace=False)) if c != 1 else np.zeros(0, np.int64)
            a = bins["stop"][idx[pick]].astype(np.int64) + 1; b = a + 50
            excluded.append((a.astype(np.int32), b.astype(np.int32)))
            for x, y in zip(a, b):
                f.write(f"{synth.CHROM_NAMES[c]}\t{x}\t{y}\n")
    idx = np.nonzero(bins["chr"] == 2)[0]
    s, e = bins["start"][idx].astype(np.int64), bins["stop"][idx].astype(np.int64)
    k1, k2 = len(idx) // 4, len(idx) // 2
    recs = [(int((s[k1] + e[k1]) // 2) + 1, int(e[k2]), 1), (int(e[k2]) + 1, int(e[-1]) + 1000, 3)]      # a boundary inside a bin, one exactly on a bin's end
    with open(d / "ploidy.vcf", "w") as f:
        f.write("##fileformat=VCFv4.1\n##INFO=<ID=END,Number=1,Type=Integer,Description=\"End\">\n##FORMAT=<ID=CN,Number=1,Type=Integer,Description=\"CN\">\n")
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE1\n")
        for a, b, cn in recs:
            f.write(f"{synth.CHROM_NAMES[2]}\t{a}\t.\tN\t<CNV>\t.\tPASS\tEND={b}\tCN\t{cn}\n")
    ploidy = [Z3, Z3, tuple(np.array(col, np.int32) for col in zip(*recs))]
    return dict(dir=d, nchr=nchr, chr=bins["chr"], start=bins["start"].astype(np.int32), stop=bins["stop"].astype(np.int32), cov=np.array([float(t) for t in text]),
                excluded=excluded, ploidy=ploidy)


@pytest.mark.parametrize("method,filtered", [("CBS", False), ("CBS", True), ("Wavelets", False), ("Wavelets", True)])
def test_states_reproduce_the_text_the_executable_writes(cv, hand_off, method, filtered):
    h = hand_off
    d, nchr = h["dir"], h["nchr"]
    part = d / ("S.%s.%d.partitioned" % (method, filtered))
    cmd = [EXE, "-i", str(d / "S.cleaned"), "-o", str(part), "-r", str(d / "WholeGenomeFasta"), "-m", method]
    cmd += ["-v", str(d / "VFResultsS.txt.gz")] if method == "Wavelets" else []
    cmd += ["-b", str(d / "filter.bed"), "-p", str(d / "ploidy.vcf")] if filtered else []
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with gzip.open(part, "rt") as f:
        names, want = S.from_text(f.read())
    assert names == synth.CHROM_NAMES[:nchr] and want["nseg"] > nchr              # a one-segment answer cannot pass
    keep = np.ones(len(h["chr"]), bool)
    if filtered:                                                                 # -b also drops the bins that overlap an interval (CanvasPartition reads the file through the filter)
        for c, (a, b) in enumerate(h["excluded"]):
            for x, y in zip(a, b):
                keep &= ~((h["chr"] == c) & (h["start"] < y) & (h["stop"] > x))
    off = np.concatenate([[0], np.cumsum(np.bincount(h["chr"][keep], minlength=nchr))]).astype(np.int64)
    cov = to_dev(h["cov"][keep], cv.device)                                      # the doubles CanvasPartition parses
    start, stop = to_dev(h["start"][keep], cv.device), to_dev(h["stop"][keep], cv.device)
    if method == "CBS":
        seg_len, nseg, _ = cv.cbs(cov, off)
        state = cv.partition_states(off, seg_len=seg_len, nseg=nseg)
    else:
        state = cv.partition_states(off, breakpoints=cv.wavelets(cov, off))
    assert int(state.max()) >= 1
    seg, _ = cv.segment_ids(off, state, start, stop, excluded=h["excluded"] if filtered else None, ploidy=h["ploidy"] if filtered else None)
    got = cv.segment_tables(off, start, stop, seg, cov)
    S.same_tables(dict(got, counts=got["counts"].cpu().numpy()), want)
    if filtered:                                                                 # the two files really change the answer
        plain, _ = cv.segment_ids(off, state, start, stop)
        assert int(seg.max()) > int(plain.max())


# ---------------------------------------------------------------------------------------------------------------- (b) call_somatic_ids
TIMES = ("stage1_ms", "stage23_ms", "stage4_ms", "stage5_ms", "stage6_ms", "host_table_ms", "upload_ms", "device_ms", "selection_ms")      # wall clock: differ from call to call


def _untimed(out):
    res = {k: v for k, v in out.items() if k not in TIMES and k not in ("fit", "tables", "seg_ref_cn")}
    res.update({"fit." + k: v for k, v in out["fit"].items() if k not in TIMES})
    return res


def _ploidy_of(case):
    """the case's reference copy numbers as ploidy records: one record over [Begin + 1, End] of every segment that is not at 2"""
    cso, ref = case["chr_seg_offset"], case["seg_ref_cn"]
    out = []
    for c in range(len(cso) - 1):
        s = [k for k in range(cso[c], cso[c + 1]) if ref[k] != 2]
        out.append((case["seg_begin"][s] + 1, case["seg_end"][s], ref[s]))
    return out


def _both(cv, case):
    """(call_somatic on the case's tables, call_somatic_ids on its bins), each (result, None) or (partial, code)"""
    b = per_bin(case)
    sites = [to_dev(case[k], cv.device) for k in ("site_pos", "site_ref", "site_alt")]
    outcome = []
    for ids in (False, True):
        try:
            if ids:
                r = cv.call_somatic_ids(b["off"], to_dev(b["start"], cv.device), to_dev(b["stop"], cv.device), to_dev(b["seg"], cv.device), to_dev(b["cov"], cv.device),
                                        case["chr_site_offset"], *sites, case["genome_length"], ploidy=_ploidy_of(case), excluded=case.get("excluded"), **case["params"])
            else:
                r = cv.call_somatic(to_dev(case["counts"], cv.device), case["chr_seg_offset"], case["seg_begin"], case["seg_end"], case["seg_bin_offset"], case["chr_site_offset"], *sites,
                                    case["genome_length"], seg_ref_cn=case["seg_ref_cn"], excluded=case.get("excluded"), **case["params"])
            outcome.append((r, None))
        except CanvasError as e:
            outcome.append((e.partial, e.code))
    return b, outcome[0], outcome[1]


@pytest.mark.parametrize("name", list(C.CASES))
def test_call_somatic_ids_equals_call_somatic(cv, name):
    case = C.built(name)
    b, (want, wcode), (got, gcode) = _both(cv, case)
    assert wcode is None and gcode is None and want["stages"] == 6
    same_outputs(_untimed(got), _untimed(want))
    assert sorted(_untimed(got)) == sorted(_untimed(want))
    assert got["seg_ref_cn"].dtype == np.int32 and (got["seg_ref_cn"] == case["seg_ref_cn"]).all()
    S.same_tables(dict(got["tables"], counts=got["tables"]["counts"].cpu().numpy()), S.from_arrays(b["off"], b["start"], b["stop"], b["seg"], b["cov"]))
    if name == "reference copy number":
        assert sorted(set(case["seg_ref_cn"].tolist())) == [0, 1, 2]


def test_call_somatic_ids_passes_the_somatic_codes_through_with_the_tables(cv):
    from canvas_amd import lib as L
    case = C.built("2 usable")
    b, (want, wcode), (got, gcode) = _both(cv, case)
    assert wcode == gcode == L.ERR_SOMATIC_FEW_SEGMENTS and want["stages"] == got["stages"] == 2
    same_outputs(_untimed(got), _untimed(want))
    S.same_tables(dict(got["tables"], counts=got["tables"]["counts"].cpu().numpy()), S.from_arrays(b["off"], b["start"], b["stop"], b["seg"], b["cov"]))
    assert (got["seg_ref_cn"] == case["seg_ref_cn"]).all()
    # refused by the tables, by the ploidy records, by the call's own checks: CANVAS_ERR_INVALID and nothing to hand back
    case = C.built("base")
    b = per_bin(case)
    dev = [to_dev(b[k], cv.device) for k in ("start", "stop", "seg", "cov")]
    sites = [to_dev(case[k], cv.device) for k in ("site_pos", "site_ref", "site_alt")]
    bad_ploidy = [Z3] * (len(b["off"]) - 1); bad_ploidy[0] = (np.array([1], np.int32), np.array([10], np.int32), np.array([5], np.int32))
    for kw, what in ((dict(cap_seg=3), "room for 3"), (dict(ploidy=bad_ploidy), "copy number outside 0..4"), (dict(genome_length=0), "genome_length")):
        with pytest.raises(CanvasError) as e:
            cv.call_somatic_ids(b["off"], *dev, case["chr_site_offset"], *sites, **dict(dict(genome_length=case["genome_length"]), **kw), **case["params"])
        assert e.value.code == -1 and e.value.partial is None and what in str(e.value), str(e.value)
    # the room for the tables is found in one repeat, as by call_diploid_ids
    old = type(cv).SEGMENT_TABLES_CAP
    try:
        type(cv).SEGMENT_TABLES_CAP = 5
        small = cv.call_somatic_ids(b["off"], *dev, case["chr_site_offset"], *sites, case["genome_length"], **case["params"])
    finally:
        type(cv).SEGMENT_TABLES_CAP = old
    want = cv.call_somatic_ids(b["off"], *dev, case["chr_site_offset"], *sites, case["genome_length"], **case["params"])
    assert small["tables"]["nseg"] == len(case["seg_begin"]) > 5
    same_outputs(_untimed(small), _untimed(want))


# ---------------------------------------------------------------------------------------------------------------- (c) germline_flow
@pytest.fixture(scope="module")
def genome(cv):
    lengths = [3_000_000, 2_200_000, 1_500_000]                 # the genome of tests/test_pipeline_gpu.py
    thr = synth.poisson_thresholds(0.21)
    data = [synth.generate_chromosome(20260927 + 70, c, L, 0.21, thr) for c, L in enumerate(lengths)]
    rng = np.random.RandomState(9)
    pos = [np.arange(700, L, 1500, dtype=np.int32) for L in lengths]
    csi = np.concatenate([[0], np.cumsum([len(p) for p in pos])]).astype(np.int64)
    depth = rng.choice([8, 12, 30, 40], int(csi[-1])); alt = (depth * rng.choice([0.0, 0.3, 0.5, 0.5, 1.0], len(depth))).astype(np.int32)
    return dict(bases=[to_dev(pad16(b), cv.device) for b, h, m in data], hits=[to_dev(pad16(h), cv.device) for b, h, m in data],
                masks=[to_dev(m.view(np.int64), cv.device) for b, h, m in data], lens=np.array(lengths, np.int64), is_auto=np.array([1, 1, 0], np.uint8), csi=csi,
                sites=[to_dev(np.concatenate(pos), cv.device), to_dev((depth - alt).astype(np.int32), cv.device), to_dev(alt, cv.device)],
                flags=CLEAN_GCNORM | CLEAN_FILTSIZE | CLEAN_OUTLIERS | CLEAN_LOCALSD)


def _same_flow(a, b):
    import torch
    assert sorted(a) == sorted(b)
    assert all(a[k] == b[k] for k in ("bin_size", "total", "n_out", "nseg")) and a["off"].tolist() == b["off"].tolist()
    assert np.float64(a["lsd"]).tobytes() == np.float64(b["lsd"]).tobytes()
    for k in a["bins"]:
        assert torch.equal(a["bins"][k], b["bins"][k]), k
    for k in ("cov", "state", "seg"):
        assert torch.equal(a[k], b[k]), k
    same_outputs({k: v for k, v in a["calls"].items() if k != "tables"}, {k: v for k, v in b["calls"].items() if k != "tables"})
    S.same_tables(dict(a["calls"]["tables"], counts=a["calls"]["tables"]["counts"].cpu().numpy()), dict(b["calls"]["tables"], counts=b["calls"]["tables"]["counts"].cpu().numpy()))


def test_germline_flow_hmm_is_the_flow_without_a_method(cv, genome):
    g = genome
    args = (g["bases"], g["masks"], g["hits"], g["lens"], g["is_auto"], g["csi"], *g["sites"])
    _same_flow(cv.germline_flow(*args, flags=g["flags"], method="hmm"), cv.germline_flow(*args, flags=g["flags"]))
    for kw in (dict(method="viterbi"), dict(partition=dict(alpha=0.05)), dict(ploidy=[Z3] * 3), dict(excluded=[Z2] * 3)):
        with pytest.raises(CanvasError):
            cv.germline_flow(*args, flags=g["flags"], **kw)


@pytest.mark.parametrize("method", ("cbs", "wavelets"))
def test_germline_flow_equals_the_separately_issued_calls(cv, genome, method):
    import torch
    g = genome
    nchr = len(g["lens"])
    partition = dict(alpha=0.02, nperm=5000) if method == "cbs" else dict(mad_factor=4.0)
    # the staged route first: its bins decide where the excluded intervals and ploidy records go
    cap = int(g["lens"].sum() // 50) + 64
    mk = lambda dt: torch.empty(cap, dtype=dt, device=cv.device)
    out = dict(chr=mk(torch.int32), start=mk(torch.int32), stop=mk(torch.int32), gc=mk(torch.int32), count=mk(torch.float32))
    _, _, total, bs = cv.bin_sample(g["bases"], g["masks"], g["hits"], g["lens"], g["is_auto"], 100, -1, out=out)
    n, lsd, _ = cv.clean(out, total, g["is_auto"], g["flags"])
    cov = cv.quantize_f2(out["count"], n)
    off = cv.chromosome_offsets(out["chr"], n, nchr)
    hs, he = out["start"][:n].cpu().numpy().astype(np.int64), out["stop"][:n].cpu().numpy().astype(np.int64)
    excluded, ploidy = [], []
    for c in range(nchr):
        e = he[off[c]:off[c + 1]]
        k = np.array([len(e) // 5, len(e) // 2, 4 * len(e) // 5])
        excluded.append(((e[k] - 20).astype(np.int32), (e[k] + 30).astype(np.int32)))
        ploidy.append(Z3 if c != 2 else (np.array([1, int(e[len(e) // 3]) + 1], np.int32), np.array([int(e[len(e) // 3]), int(e[-1]) + 10], np.int32), np.array([1, 2], np.int32)))
    if method == "cbs":
        seg_len, nseg_chr, _ = cv.cbs(cov, off, **partition)
        state = cv.partition_states(off, seg_len=seg_len, nseg=nseg_chr)
    else:
        state = cv.partition_states(off, breakpoints=cv.wavelets(cov, off, is_germline=True, **partition))
    seg, nseg = cv.segment_ids(off, state, out["start"], out["stop"], 1000000, excluded, ploidy=ploidy)
    calls = cv.call_diploid_ids(off, out["start"], out["stop"], seg, cov, g["csi"], *g["sites"])
    want = dict(bin_size=bs, total=total, n_out=n, lsd=lsd, off=off, nseg=nseg, bins={k: v[:n] for k, v in out.items()}, cov=cov[:n], state=state[:n], seg=seg[:n], calls=calls)
    assert n > 5_000 and nseg > nchr + 3 and int(state.min()) >= 0

    flow = cv.germline_flow(g["bases"], g["masks"], g["hits"], g["lens"], g["is_auto"], g["csi"], *g["sites"], flags=g["flags"], method=method, partition=partition,
                            excluded=excluded, ploidy=ploidy)
    _same_flow(flow, want)
    plain = cv.germline_flow(g["bases"], g["masks"], g["hits"], g["lens"], g["is_auto"], g["csi"], *g["sites"], flags=g["flags"], method=method, partition=partition)
    assert plain["nseg"] < nseg and torch.equal(plain["state"], flow["state"])     # the intervals and records reached segment_ids


# ---------------------------------------------------------------------------------------------------------------- (d) somatic_flow
def test_somatic_flow_equals_tumor_normal_flow_and_the_separate_steps(cv):
    import torch
    from test_somatic_flow_gpu import _pair
    lengths = [2_500_000, 1_300_001]                            # the smallest pair of tests/test_somatic_flow_gpu.py
    flags = CLEAN_GCNORM | CLEAN_FILTSIZE | CLEAN_OUTLIERS
    nchr = len(lengths)
    T, N = _pair(lengths)
    is_auto = np.ones(nchr, np.uint8); is_auto[-1] = 0
    bases = [to_dev(pad16(t[0]), cv.device) for t in T]; masks = [to_dev(t[2].view(np.int64), cv.device) for t in T]
    hits_t = [to_dev(pad16(t[1]), cv.device) for t in T]; fl = [to_dev(pad16(t[3]), cv.device) for t in T]; hits_n = [to_dev(pad16(n[1]), cv.device) for n in N]
    lens = np.array(lengths, np.int64)
    rng = np.random.RandomState(4)
    pos = [np.arange(400, L, 700, dtype=np.int32) for L in lengths]
    csi = np.concatenate([[0], np.cumsum([len(p) for p in pos])]).astype(np.int64)
    depth = rng.choice([30, 40, 50], int(csi[-1])); alt = (depth * rng.choice([0.3, 0.45, 0.5, 0.55, 0.7], len(depth))).astype(np.int32)
    sites = [to_dev(np.concatenate(pos), cv.device), to_dev((depth - alt).astype(np.int32), cv.device), to_dev(alt, cv.device)]
    inputs = (bases, masks, hits_t, fl, hits_n, lens, is_auto, flags)
    tn = cv.tumor_normal_flow(*inputs, alpha=0.01, nperm=10000, keep=True)
    assert sorted(tn) == sorted(["bin_size", "n_bins", "n_ratio", "library_size_factor", "tumour", "normal_count", "keep_idx", "ratio", "ratio_count", "to_clean", "n_clean", "local_sd",
                                 "chr_offset", "nseg", "cbs_stats", "segments", "stage_seconds", "cleaned", "cov", "seg_len"])
    assert sorted(cv.tumor_normal_flow(*inputs)) == sorted(["bin_size", "n_bins", "n_ratio", "library_size_factor", "n_clean", "local_sd", "chr_offset", "nseg", "cbs_stats", "segments",
                                                             "stage_seconds"])
    off, R = tn["chr_offset"], tn["cleaned"]
    # excluded intervals cut every chromosome into stretches of more than 5 000 bases (the CBS segments of two small chromosomes alone are too few to model), one ploidy record
    he = R["stop"].cpu().numpy().astype(np.int64)
    excluded, ploidy = [], []
    for c in range(nchr):
        e = he[off[c]:off[c + 1]]
        k = np.arange(1, 8) * len(e) // 8
        excluded.append(((e[k] - 5).astype(np.int32), (e[k] + 5).astype(np.int32)))
        ploidy.append(Z3 if c == 0 else (np.array([int(e[len(e) // 2]) + 1], np.int32), np.array([int(e[-1]) + 10], np.int32), np.array([1], np.int32)))
    params = dict(minimum_purity_hard_limit=95)

    def outcome(fn):
        try:
            return fn(), None
        except CanvasError as e:
            return e.partial, e.code

    flow, fcode = outcome(lambda: cv.somatic_flow(*inputs, csi, *sites, sum(lengths), excluded=excluded, ploidy=ploidy, alpha=0.01, nperm=10000, keep=True, **params))
    if fcode is None:
        for k in tn:                                            # tumor_normal_flow's keys and values, untouched
            if k == "stage_seconds":
                assert sorted(flow[k]) == sorted(tn[k])
            elif k == "cbs_stats":                              # TMaxO calls, permutations, TPermP draws (the other entries are not counters of the arithmetic)
                assert [flow[k][i] for i in (0, 2, 4)] == [tn[k][i] for i in (0, 2, 4)]
            elif isinstance(tn[k], dict):
                assert all(torch.equal(flow[k][a], tn[k][a]) for a in tn[k]), k
            elif isinstance(tn[k], torch.Tensor):
                assert torch.equal(flow[k], tn[k]), k
            else:
                assert np.array_equal(flow[k], tn[k]), k
        assert sorted(set(flow) - set(tn)) == ["calls", "seg", "state"]
    state = cv.partition_states(off, seg_len=tn["seg_len"], nseg=tn["nseg"])
    seg, nseg = cv.segment_ids(off, state, R["start"], R["stop"], 1000000, excluded, ploidy=ploidy)
    want, wcode = outcome(lambda: cv.call_somatic_ids(off, R["start"], R["stop"], seg, tn["cov"], csi, *sites, sum(lengths), ploidy=ploidy, excluded=excluded, **params))
    assert nseg >= 16 and wcode == fcode, (wcode, fcode)
    calls = flow["calls"] if fcode is None else flow
    same_outputs(_untimed(calls), _untimed(want))
    S.same_tables(dict(calls["tables"], counts=calls["tables"]["counts"].cpu().numpy()), dict(want["tables"], counts=want["tables"]["counts"].cpu().numpy()))
    assert (calls["seg_ref_cn"] == want["seg_ref_cn"]).all() and sorted(set(want["seg_ref_cn"].tolist())) == [1, 2]
    assert fcode is None and want["stages"] == 6, (fcode, want["stages"])      # the pair is called, not refused
    assert torch.equal(flow["state"], state) and torch.equal(flow["seg"], seg)
