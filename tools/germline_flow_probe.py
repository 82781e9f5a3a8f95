"""canvas_segment_tables and the chain behind canvas_sample_pipeline on synthetic whole-genome-like input, by the method of tools/somatic_call_probe.py:
    python tools/germline_flow_probe.py [--bins 3000000] [--segments 3000] [--sites 3000000] [--reps 10] [--no-flow]
`bins` cleaned bins of 1 000 bases on 23 chromosomes in `segments` segments (running ids, copy numbers 1 .. 4 around a median of 100), `sites` variant sites of depth 30, all
device-resident as canvas_sample_pipeline leaves them.  One warm-up call, then `reps` calls of each route; as one JSON line, minimum and median wall time in ms of
    segment_tables     Canvas.segment_tables (three launches, one wait) and the device time of its scope from canvas_profile_get in a separate run of calls
    call_diploid_ids   Canvas.call_diploid_ids: tables and calls in one library call
    host_route         what a caller did before this entry: fetch start / stop / segment_id / cov, group them in numpy (tables, confidence intervals, float counts), upload the
                       counts, Canvas.call_diploid — with the time of its parts (fetch, group, upload + call)
and, unless --no-flow, Canvas.germline_flow on the small synthetic genome of tests/test_pipeline_gpu.py against sample_pipeline followed by the host route."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("CANVAS_TEST_HOOKS", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def genome(rng, nbins, nseg, nsites):
    nchr = 23
    per = np.full(nchr, nseg // nchr); per[:nseg - per.sum()] += 1
    cso = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    bins = rng.multinomial(nbins - nseg, np.ones(nseg) / nseg) + 1
    sbo = np.concatenate([[0], np.cumsum(bins)]).astype(np.int64)
    off = sbo[cso]
    idx = np.arange(nbins, dtype=np.int64)
    chr_of = np.searchsorted(off, idx, side="right") - 1
    start = (10000 + (idx - off[chr_of]) * 1000).astype(np.int32)
    cn = rng.choice([1, 2, 2, 2, 3, 4], nseg)
    cov = np.round(np.repeat(50.0 * cn, bins) + rng.normal(0, 5, nbins)).clip(0)
    n = rng.multinomial(nsites, np.diff(off) / nbins)
    pos = np.concatenate([np.sort(rng.integers(10001, 10000 + 1000 * (off[c + 1] - off[c]), n[c])) for c in range(nchr)]).astype(np.int32)
    alt = rng.binomial(30, 0.5, nsites).astype(np.int32)
    return dict(off=off, start=start, stop=start + 1000, seg=np.repeat(np.arange(nseg), bins).astype(np.int32), cov=cov, chr_site_offset=np.concatenate([[0], np.cumsum(n)]).astype(np.int64),
                site_pos=pos, site_ref=(30 - alt).astype(np.int32), site_alt=alt)


def group_on_host(off, start, stop, seg, cov):
    """Segments.ReadSegments over fetched arrays, vectorised: the tables, the confidence intervals and the float counts"""
    n = len(start)
    first = np.zeros(n, bool); first[off[:-1][off[:-1] < n]] = True
    opens = first.copy(); opens[1:] |= seg[1:] != seg[:-1]
    idx = np.nonzero(opens)[0]; last = np.concatenate([idx[1:] - 1, [n - 1]])
    half = (stop.astype(np.int64) - start + 1) // 2
    abut = np.zeros(n, bool); abut[1:] = (stop[:-1] == start[1:]) & ~first[1:]          # bin i abuts bin i - 1 of its chromosome
    nxt = np.minimum(last + 1, n - 1); abut_next = abut[nxt] & (last + 1 < n)
    ci = np.stack([-np.where(abut[idx], half[np.maximum(idx - 1, 0)], half[idx]), half[idx], -half[last], np.where(abut_next, half[nxt], half[last])], 1).astype(np.int32)
    return dict(chr_seg_offset=np.searchsorted(idx, off).astype(np.int64), seg_begin=start[idx], seg_end=stop[last], seg_bin_offset=np.concatenate([idx, [n]]).astype(np.int64), seg_ci4=ci,
                counts=cov.astype(np.float32))


def stats(ms):
    return dict(min=round(min(ms), 3), median=round(float(np.median(ms)), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=3_000_000)
    ap.add_argument("--segments", type=int, default=3000)
    ap.add_argument("--sites", type=int, default=3_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-flow", action="store_true")
    args = ap.parse_args()
    import torch
    from canvas_amd import Canvas, synth, CLEAN_GCNORM, CLEAN_FILTSIZE, CLEAN_OUTLIERS, CLEAN_LOCALSD
    cv = Canvas(0)
    g = genome(np.random.default_rng(7), args.bins, args.segments, args.sites)
    dev = {k: torch.from_numpy(g[k]).to(cv.device) for k in ("start", "stop", "seg", "cov", "site_pos", "site_ref", "site_alt")}
    sites = (g["chr_site_offset"], dev["site_pos"], dev["site_ref"], dev["site_alt"])
    counts = torch.empty(args.bins, dtype=torch.float32, device=cv.device)
    parts = dict(fetch=[], group=[], call=[])

    def host_route(off, start, stop, seg, cov, n, keep=parts):
        t0 = time.perf_counter()
        h = [t[:n].cpu().numpy() for t in (start, stop, seg, cov)]
        t1 = time.perf_counter()
        t = group_on_host(off, *h)
        t2 = time.perf_counter()
        r = cv.call_diploid(torch.from_numpy(t["counts"]).to(cv.device), t["chr_seg_offset"], t["seg_begin"], t["seg_end"], t["seg_bin_offset"], *sites,
                            seg_start_ci=t["seg_ci4"][:, :2], seg_end_ci=t["seg_ci4"][:, 2:])
        t3 = time.perf_counter()
        if keep is not None:
            keep["fetch"].append((t1 - t0) * 1e3); keep["group"].append((t2 - t1) * 1e3); keep["call"].append((t3 - t2) * 1e3)
        return r, t

    routes = dict(segment_tables=lambda: cv.segment_tables(g["off"], dev["start"], dev["stop"], dev["seg"], dev["cov"], counts=counts),
                  call_diploid_ids=lambda: cv.call_diploid_ids(g["off"], dev["start"], dev["stop"], dev["seg"], dev["cov"], *sites, counts=counts),
                  host_route=lambda: host_route(g["off"], dev["start"], dev["stop"], dev["seg"], dev["cov"], args.bins))
    wall = {}
    for name, f in routes.items():
        f()
        for k in parts:
            parts[k].clear()
        ms = []
        for _ in range(args.reps):
            t = time.perf_counter(); r = f(); ms.append((time.perf_counter() - t) * 1e3)
        wall[name] = stats(ms)
        if name == "call_diploid_ids":
            ids = r
        if name == "host_route":
            wall["host_route_parts"] = {k: stats(v) for k, v in parts.items()}
            same = all(np.asarray(ids[k]).tobytes() == np.asarray(v).tobytes() for k, v in r[0].items() if isinstance(v, np.ndarray)) and \
                all((np.asarray(ids["tables"][k]) == r[1][k]).all() for k in ("chr_seg_offset", "seg_begin", "seg_end", "seg_bin_offset", "seg_ci4"))
    cv.profile_enable(1)
    cv.profile_get("segment_tables")
    for _ in range(3):
        routes["segment_tables"]()
    ms, launches = cv.profile_get("segment_tables")
    cv.profile_enable(0)
    res = dict(bins=args.bins, segments=int(ids["tables"]["nseg"]), sites=args.sites, runs=len(ids["run_first"]), routes_agree=bool(same), wall_ms=wall,
               segment_tables_device_ms=round(ms / 3, 3), segment_tables_scopes_per_call=launches / 3)
    if not args.no_flow:
        lengths = [3_000_000, 2_200_000, 1_500_000]
        thr = synth.poisson_thresholds(0.21)
        data = [synth.generate_chromosome(20260927 + 70, c, L, 0.21, thr) for c, L in enumerate(lengths)]
        pad = lambda a: np.concatenate([a, np.zeros((-len(a)) % 64, a.dtype)])
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cv.device)
        bases = [up(pad(b)) for b, h, m in data]; hits = [up(pad(h)) for b, h, m in data]; masks = [up(m.view(np.int64)) for b, h, m in data]
        lens = np.array(lengths, np.int64); is_auto = np.array([1, 1, 0], np.uint8)
        flags = CLEAN_GCNORM | CLEAN_FILTSIZE | CLEAN_OUTLIERS | CLEAN_LOCALSD
        pos = [np.arange(700, L, 1500, dtype=np.int32) for L in lengths]
        csi = np.concatenate([[0], np.cumsum([len(p) for p in pos])]).astype(np.int64)
        sites = (csi, up(np.concatenate(pos)), up(np.full(int(csi[-1]), 15, np.int32)), up(np.full(int(csi[-1]), 15, np.int32)))
        cap = int(lens.sum() // 50) + 64
        mk = lambda dt: torch.empty(cap, dtype=dt, device=cv.device)
        out = dict(chr=mk(torch.int32), start=mk(torch.int32), stop=mk(torch.int32), gc=mk(torch.int32), count=mk(torch.float32))
        cov, state, seg = mk(torch.float64), mk(torch.int32), mk(torch.int32)

        def staged():
            r = cv.sample_pipeline(bases, masks, hits, lens, is_auto, out, cov, state, seg, flags=flags)
            return host_route(r["off"], out["start"], out["stop"], seg, cov, r["n_out"], keep=None)
        flow = {}
        for name, f in (("germline_flow", lambda: cv.germline_flow(bases, masks, hits, lens, is_auto, *sites, flags=flags)), ("pipeline_then_host_route", staged)):
            f()
            ms = []
            for _ in range(args.reps):
                t = time.perf_counter(); r = f(); ms.append((time.perf_counter() - t) * 1e3)
            flow[name] = stats(ms)
        res["small_genome_wall_ms"] = dict(bases=int(lens.sum()), **flow)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
