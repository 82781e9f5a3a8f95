"""canvas_call_somatic with the default parameters on synthetic whole-genome-like input:
    python tools/somatic_call_probe.py [--bins 3000000] [--segments 3000] [--sites 3000000] [--median 100] [--reps 10]
A tumour of purity 70 % with copy numbers 1 .. 4 (and 12 for one segment in a hundred) over `segments` segments on 23 chromosomes, `bins` counts around `median`, `sites` variant sites of depth 60.  One warm-up
call, then `reps` calls: as one JSON line the wall time of the call and of its parts as the library reports them (stage 1: sites and the per-segment selects; stages 2-3:
usable segments, compaction and the median level; stage 4: the fit, with its own four parts; stage 5: the ploidy scan and MeanCount; stage 6: the host tail), minimum and
median, and the device time of the call's own kernels from canvas_profile_get in a separate run of calls (the event pairs cost time of their own)."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("CANVAS_TEST_HOOKS", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def genome(rng, nbins, nseg, nsites, median):
    nchr = 23
    per = np.full(nchr, nseg // nchr); per[:nseg - per.sum()] += 1
    cso = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    bins = rng.multinomial(nbins - nseg, np.ones(nseg) / nseg) + 1
    sbo = np.concatenate([[0], np.cumsum(bins)]).astype(np.int64)
    length = bins.astype(np.int64) * 1000
    beg = np.zeros(nseg, np.int64)
    for c in range(nchr):
        sl = slice(cso[c], cso[c + 1])
        beg[sl] = 10000 + np.concatenate([[0], np.cumsum(length[sl])[:-1]])
    end = beg + length
    purity = 0.7
    cn = rng.choice([1, 2, 2, 2, 3, 4], nseg)
    cn[rng.random(nseg) < 0.01] = 12                             # above 2 x the overall median: out of the model, called through MeanCount
    major = np.array([rng.integers((c + 1) // 2, c + 1) for c in cn])
    level = median * (purity * cn / 2 + (1 - purity))
    counts = (np.repeat(level, bins) + rng.normal(0, 0.05 * median, int(bins.sum()))).clip(0).round().astype(np.float32)
    baf = (purity * (cn - major) + (1 - purity)) / (purity * cn + 2 * (1 - purity))
    n = rng.multinomial(nsites, bins / bins.sum())
    seg_of = np.repeat(np.arange(nseg), n)
    pos = np.concatenate([np.sort(rng.integers(beg[s] + 1, end[s], n[s])) for s in range(nseg)]).astype(np.int32)
    alt = rng.binomial(60, np.where(rng.random(nsites) < 0.5, baf[seg_of], 1 - baf[seg_of])).astype(np.int32)
    csi = np.concatenate([[0], np.cumsum(n)])[cso].astype(np.int64)
    return dict(counts=counts, chr_seg_offset=cso, seg_begin=beg.astype(np.int32), seg_end=end.astype(np.int32), seg_bin_offset=sbo, chr_site_offset=csi, site_pos=pos,
                site_ref=(60 - alt).astype(np.int32), site_alt=alt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=3_000_000)
    ap.add_argument("--segments", type=int, default=3000)
    ap.add_argument("--sites", type=int, default=3_000_000)
    ap.add_argument("--median", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    from canvas_amd import Canvas
    cv = Canvas(0)
    g = genome(np.random.default_rng(7), args.bins, args.segments, args.sites, args.median)
    dev = {k: torch.from_numpy(g[k]).to(cv.device) for k in ("counts", "site_pos", "site_ref", "site_alt")}
    call = lambda: cv.call_somatic(dev["counts"], g["chr_seg_offset"], g["seg_begin"], g["seg_end"], g["seg_bin_offset"], g["chr_site_offset"], dev["site_pos"], dev["site_ref"],
                                   dev["site_alt"], 3_000_000_000, min_minor_allele_coverage=0.45 * args.median)
    call()
    rows, wall = [], []
    for _ in range(args.reps):
        t = time.perf_counter(); r = call(); wall.append((time.perf_counter() - t) * 1e3)
        rows.append(dict({k: r[k] for k in ("stage1_ms", "stage23_ms", "stage4_ms", "stage5_ms", "stage6_ms")}, **{"fit_" + k: r["fit"][k] for k in ("host_table_ms", "upload_ms", "device_ms", "selection_ms")}))
    part = lambda k: dict(min=round(min(x[k] for x in rows), 3), median=round(float(np.median([x[k] for x in rows])), 3))
    scopes = ("scall_sites", "call_select_wave", "call_select_lds", "call_select_tiled", "scall_compact", "somatic_fit", "scall_assign")
    cv.profile_enable(1)
    for s in scopes:
        cv.profile_get(s)
    for _ in range(3):
        call()
    kernels = {}
    for s in scopes:
        ms, launches = cv.profile_get(s)
        kernels[s] = dict(ms_per_call=round(ms / 3, 3), scopes_per_call=launches / 3)
    cv.profile_enable(0)
    print(json.dumps(dict(bins=args.bins, segments=args.segments, sites=args.sites, median=args.median, usable=r["nusable"], level=r["median_coverage_level"], models=r["fit"]["nmodels"],
                          best=[r["fit"]["best_coverage"], r["fit"]["best_percent_purity"]], info=r["fit"]["info"], runs=r["nruns"], threshold=r["threshold_used"],
                          mean_routes={str(k): int((r["seg_mean_route"] == k).sum()) for k in (-1, 0, 1)},
                          wall_ms=dict(min=round(min(wall), 3), median=round(float(np.median(wall)), 3)), **{k: part(k) for k in rows[0]}, device_scopes=kernels)), flush=True)


if __name__ == "__main__":
    main()
