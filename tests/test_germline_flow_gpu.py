"""The germline sample from segment ids to calls without the text hand-off: (a) Canvas.call_diploid_ids gives every output of Canvas.call_diploid bit for bit on the cases of
tests/diploid_cases.py expanded to per-bin arrays; (b) Canvas.segment_tables on the device arrays of hmm_per_sample + segment_ids equals Segments.ReadSegments of the
*.partitioned file the CanvasPartition executable writes for the same input; (c) Canvas.germline_flow equals sample_pipeline, host-built tables, call_diploid."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import diploid_cases as DC
import oracle_lib as O
import segment_tables_ref as S
from canvas_amd import synth, CLEAN_GCNORM, CLEAN_FILTSIZE, CLEAN_OUTLIERS, CLEAN_LOCALSD
from gpu_common import get_canvas, to_dev, pad16

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "canvas_amd", "bin", "CanvasPartition")


@pytest.fixture(scope="module")
def cv():
    return get_canvas()


def same_outputs(got, want):
    """every entry of `want`, arrays by dtype, shape and bytes (NaN-safe, -0.0 apart from 0.0)"""
    for k, w in want.items():
        g = got[k]
        if isinstance(w, np.ndarray):
            g = np.asarray(g)
            assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
            assert g.tobytes() == w.tobytes(), (k, np.nonzero(g != w)[0][:8].tolist())
        elif isinstance(w, float):
            assert np.float64(g).tobytes() == np.float64(w).tobytes(), (k, g, w)
        else:
            assert g == w, (k, g, w)


def per_bin(case):
    """a case of diploid_cases as the bins a partition would have left: a segment of nb bins from Begin to End is cut into nb abutting bins, the ids return (s % 3 - 1) and
    run across chromosome boundaries, a chromosome without segments is an empty chromosome"""
    sbo, beg, end = case["seg_bin_offset"], case["seg_begin"].astype(np.int64), case["seg_end"].astype(np.int64)
    nseg = len(beg); nb = np.diff(sbo)
    seg_of = np.repeat(np.arange(nseg), nb); j = np.arange(sbo[-1]) - sbo[seg_of]
    cut = lambda jj: beg[seg_of] + (end - beg)[seg_of] * jj // nb[seg_of]
    return dict(off=sbo[case["chr_seg_offset"]], start=cut(j).astype(np.int32), stop=cut(j + 1).astype(np.int32), seg=(seg_of % 3 - 1).astype(np.int32),
                cov=case["counts"].astype(np.float64))


@pytest.mark.parametrize("which", ("edge", 1, 2))
def test_call_diploid_ids_equals_call_diploid(cv, which):
    case = DC.edge_case()[0] if which == "edge" else DC.random_case(which)
    b = per_bin(case)
    tab = S.from_arrays(b["off"], b["start"], b["stop"], b["seg"], b["cov"])
    for k in ("chr_seg_offset", "seg_begin", "seg_end", "seg_bin_offset"):       # the expansion gives back the case's own tables
        assert (tab[k] == case[k]).all(), k
    sites = [to_dev(case[k], cv.device) for k in ("site_pos", "site_ref", "site_alt")]
    want = cv.call_diploid(to_dev(case["counts"], cv.device), case["chr_seg_offset"], case["seg_begin"], case["seg_end"], case["seg_bin_offset"], case["chr_site_offset"], *sites,
                           seg_start_ci=tab["seg_ci4"][:, :2], seg_end_ci=tab["seg_ci4"][:, 2:])
    got = cv.call_diploid_ids(b["off"], to_dev(b["start"], cv.device), to_dev(b["stop"], cv.device), to_dev(b["seg"], cv.device), to_dev(b["cov"], cv.device),
                              case["chr_site_offset"], *sites)
    assert len(want["cn"]) == len(case["seg_begin"]) and len(want["run_first"]) >= 3
    same_outputs(got, want)
    S.same_tables(dict(got["tables"], counts=got["tables"]["counts"].cpu().numpy()), tab)


def test_segment_tables_reproduce_the_text_hand_off(cv, tmp_path):
    nchr = 3
    bins = synth.generate_bins(20260927 + 81, 4000, nchr=nchr)
    count = bins["count"].astype(np.float32)
    for a, b, f in ((300, 520, 0.5), (1500, 1900, 1.5), (2600, 2610, 0.5), (3300, 3900, 2.0)):      # copy-number steps: without them every chromosome is one segment
        count[a:b] *= np.float32(f)
    text = [O.format_f2(float(v)) for v in count]
    cleaned = tmp_path / "S.cleaned"; part = tmp_path / "S.partitioned"; ref = tmp_path / "WholeGenomeFasta"; ref.mkdir()
    with gzip.open(cleaned, "wt") as f:
        for c, s, e, v, g in zip(bins["chr"], bins["start"], bins["stop"], text, bins["gc"]):
            f.write(f"{synth.CHROM_NAMES[c]}\t{s}\t{e}\t{v}\t{g}\n")
    r = subprocess.run([EXE, "-i", str(cleaned), "-o", str(part), "-r", str(ref), "-m", "PerSampleHMM"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with gzip.open(part, "rt") as f:
        names, want = S.from_text(f.read())
    assert names == synth.CHROM_NAMES[:nchr] and want["nseg"] > nchr
    off = np.concatenate([[0], np.cumsum(np.bincount(bins["chr"], minlength=nchr))]).astype(np.int64)
    cov = to_dev(np.array([float(t) for t in text]), cv.device)                 # the double CanvasPartition parses
    start, stop = to_dev(bins["start"].astype(np.int32), cv.device), to_dev(bins["stop"].astype(np.int32), cv.device)
    state = cv.hmm_per_sample(cov, off)
    seg, _ = cv.segment_ids(off, state, start, stop)
    got = cv.segment_tables(off, start, stop, seg, cov)
    S.same_tables(dict(got, counts=got["counts"].cpu().numpy()), want)


def test_germline_flow_equals_the_staged_route(cv):
    import torch
    lengths = [3_000_000, 2_200_000, 1_500_000]                 # the genome of tests/test_pipeline_gpu.py
    is_auto = np.array([1, 1, 0], np.uint8)
    thr = synth.poisson_thresholds(0.21)
    data = [synth.generate_chromosome(20260927 + 70, c, L, 0.21, thr) for c, L in enumerate(lengths)]
    bases = [to_dev(pad16(b), cv.device) for b, h, m in data]; hits = [to_dev(pad16(h), cv.device) for b, h, m in data]
    masks = [to_dev(m.view(np.int64), cv.device) for b, h, m in data]
    lens = np.array(lengths, np.int64)
    flags = CLEAN_GCNORM | CLEAN_FILTSIZE | CLEAN_OUTLIERS | CLEAN_LOCALSD
    rng = np.random.RandomState(9)
    pos = [np.arange(700, L, 1500, dtype=np.int32) for L in lengths]
    csi = np.concatenate([[0], np.cumsum([len(p) for p in pos])]).astype(np.int64)
    depth = rng.choice([8, 12, 30, 40], int(csi[-1])); alt = (depth * rng.choice([0.0, 0.3, 0.5, 0.5, 1.0], len(depth))).astype(np.int32)
    sites = [to_dev(np.concatenate(pos), cv.device), to_dev((depth - alt).astype(np.int32), cv.device), to_dev(alt, cv.device)]
    flow = cv.germline_flow(bases, masks, hits, lens, is_auto, csi, *sites, flags=flags)

    cap = int(lens.sum() // 100) + 16
    mk = lambda dt: torch.empty(cap, dtype=dt, device=cv.device)
    out = dict(chr=mk(torch.int32), start=mk(torch.int32), stop=mk(torch.int32), gc=mk(torch.int32), count=mk(torch.float32))
    cov, state, seg = mk(torch.float64), mk(torch.int32), mk(torch.int32)
    r = cv.sample_pipeline(bases, masks, hits, lens, is_auto, out, cov, state, seg, flags=flags)
    cv.synchronize()
    n = r["n_out"]
    assert n > 5_000 and r["nseg"] >= 3
    assert all(flow[k] == r[k] for k in ("bin_size", "total", "n_out", "nseg")) and flow["off"].tolist() == r["off"].tolist()
    assert np.float64(flow["lsd"]).tobytes() == np.float64(r["lsd"]).tobytes()
    for k in out:
        assert torch.equal(flow["bins"][k], out[k][:n]), k
    assert torch.equal(flow["cov"], cov[:n]) and torch.equal(flow["state"], state[:n]) and torch.equal(flow["seg"], seg[:n])
    # what a caller did before: fetch the four per-bin arrays, group them on the host, hand the tables to call_diploid
    h = lambda t: t[:n].cpu().numpy()
    tab = S.from_arrays(r["off"], h(out["start"]), h(out["stop"]), h(seg), h(cov))
    want = cv.call_diploid(to_dev(tab["counts"], cv.device), tab["chr_seg_offset"], tab["seg_begin"], tab["seg_end"], tab["seg_bin_offset"], csi, *sites,
                           seg_start_ci=tab["seg_ci4"][:, :2], seg_end_ci=tab["seg_ci4"][:, 2:])
    same_outputs(flow["calls"], want)
    S.same_tables(dict(flow["calls"]["tables"], counts=flow["calls"]["tables"]["counts"].cpu().numpy()), tab)
    assert tab["nseg"] >= 3 and len(want["run_first"]) >= 1
