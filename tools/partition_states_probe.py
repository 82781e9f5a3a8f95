"""canvas_partition_states_* and the chain behind CBS / Wavelets on synthetic whole-genome-like input, by the method of tools/germline_flow_probe.py:
    python tools/partition_states_probe.py [--bins 3000000] [--segments 3000] [--sites 3000000] [--reps 10] [--purity-limit 20]
`bins` cleaned bins of 1 000 bases on 23 chromosomes in `segments` segments, given the way the two methods leave them: segment lengths on the device in canvas_cbs's layout
with the counts per chromosome on the host, and the segments' first bins as breakpoints on the host.  One warm-up call, then `reps` calls of each route; as one JSON line,
minimum and median wall time in ms of
    partition_states_cbs / _breakpoints   Canvas.partition_states for either input (one wait each), and the device time of their kernels from the event pair of the
                                          "partition_states" scope (canvas_profile_get) in a separate run of calls
    device_route     Canvas.partition_states + Canvas.segment_ids + Canvas.call_somatic_ids: no per-bin array on the host
    host_route       what a caller of call_somatic had before these entries: fetch seg_len / start / stop / cov, build the ids (the starts from the lengths, the gap rule)
                     and the tables in numpy, upload the float counts, Canvas.call_somatic — with the time of its parts (fetch, group, upload + call)
and whether the two routes give identical tables and calls (asserted).  A sample the caller refuses is reported with its code; the routes must then agree on that too."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("CANVAS_TEST_HOOKS", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

from germline_flow_probe import genome, group_on_host, stats

TIMES = ("stage1_ms", "stage23_ms", "stage4_ms", "stage5_ms", "stage6_ms", "host_table_ms", "upload_ms", "device_ms", "selection_ms")


def ids_on_host(off, seg_len, nseg, start, stop, max_inter_bin_dist=1000000):
    """DeriveSegments' starts from the lengths (CBSRunner.cs:127-137) and PostProcessSegments without -b / -p, vectorised: the running segment id of every bin"""
    n = int(off[-1])
    opens = np.zeros(n, bool)
    for c in range(len(off) - 1):
        k = int(nseg[c])
        if k:
            lens = seg_len[off[c]:off[c] + k].astype(np.int64)
            opens[off[c] + np.cumsum(lens) - lens] = True
    first = np.zeros(n, bool); first[off[:-1][off[:-1] < n]] = True
    gap = np.zeros(n, bool); gap[1:] = (stop[:-1] > 0) & (stop[:-1].astype(np.int64) + max_inter_bin_dist < start[1:]) & ~first[1:]
    return (np.cumsum(opens | gap) - 1).astype(np.int32)


def comparable(out):
    """a call's outputs without its wall-clock fields"""
    res = {k: v for k, v in out.items() if k not in TIMES and k not in ("fit", "tables", "seg_ref_cn")}
    res.update({"fit." + k: v for k, v in out["fit"].items() if k not in TIMES})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=3_000_000)
    ap.add_argument("--segments", type=int, default=3000)
    ap.add_argument("--sites", type=int, default=3_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--purity-limit", type=int, default=20)
    args = ap.parse_args()
    import torch
    from canvas_amd import Canvas, CanvasError
    cv = Canvas(0)
    g = genome(np.random.default_rng(7), args.bins, args.segments, args.sites)
    off = g["off"]; nchr = len(off) - 1
    opens = np.zeros(args.bins, bool); opens[0] = True; opens[1:] = g["seg"][1:] != g["seg"][:-1]
    first_bins = np.nonzero(opens)[0]
    chr_of = np.searchsorted(off, first_bins, side="right") - 1
    nseg = np.bincount(chr_of, minlength=nchr).astype(np.int32)
    lens = np.diff(np.concatenate([first_bins, [args.bins]])).astype(np.int32)
    seg_len = np.zeros(args.bins + 1, np.int32); cso = np.concatenate([[0], np.cumsum(nseg)])
    for c in range(nchr):
        seg_len[off[c]:off[c] + nseg[c]] = lens[cso[c]:cso[c + 1]]
    breakpoints = [(first_bins[cso[c]:cso[c + 1]] - off[c]).astype(np.int32) for c in range(nchr)]
    dev = {k: torch.from_numpy(g[k]).to(cv.device) for k in ("start", "stop", "cov", "site_pos", "site_ref", "site_alt")}
    dev["seg_len"] = torch.from_numpy(seg_len).to(cv.device)
    sites = (g["chr_site_offset"], dev["site_pos"], dev["site_ref"], dev["site_alt"])
    genome_length = 3_000_000_000
    params = dict(minimum_purity_hard_limit=args.purity_limit)
    state = torch.empty(args.bins, dtype=torch.int32, device=cv.device); seg = torch.empty_like(state)
    counts = torch.empty(args.bins, dtype=torch.float32, device=cv.device)
    parts = dict(fetch=[], group=[], call=[])

    def outcome(fn):
        try:
            return fn(), 0
        except CanvasError as e:
            if e.partial is None:
                raise
            return e.partial, e.code

    def device_route():
        cv.partition_states(off, seg_len=dev["seg_len"], nseg=nseg, out=state)
        cv.segment_ids(off, state, dev["start"], dev["stop"], out=seg)
        return outcome(lambda: cv.call_somatic_ids(off, dev["start"], dev["stop"], seg, dev["cov"], *sites, genome_length, counts=counts, **params))

    def host_route():
        t0 = time.perf_counter()
        h_len, h_start, h_stop, h_cov = [t.cpu().numpy() for t in (dev["seg_len"], dev["start"], dev["stop"], dev["cov"])]
        t1 = time.perf_counter()
        t = group_on_host(off, h_start, h_stop, ids_on_host(off, h_len, nseg, h_start, h_stop), h_cov)
        t2 = time.perf_counter()
        r = outcome(lambda: cv.call_somatic(torch.from_numpy(t["counts"]).to(cv.device), t["chr_seg_offset"], t["seg_begin"], t["seg_end"], t["seg_bin_offset"], *sites, genome_length, **params))
        t3 = time.perf_counter()
        parts["fetch"].append((t1 - t0) * 1e3); parts["group"].append((t2 - t1) * 1e3); parts["call"].append((t3 - t2) * 1e3)
        return r, t

    routes = dict(partition_states_cbs=lambda: cv.partition_states(off, seg_len=dev["seg_len"], nseg=nseg, out=state),
                  partition_states_breakpoints=lambda: cv.partition_states(off, breakpoints=breakpoints, out=state),
                  device_route=device_route, host_route=host_route)
    wall, kept = {}, {}
    for name, f in routes.items():
        f()
        for k in parts:
            parts[k].clear()
        ms = []
        for _ in range(args.reps):
            t = time.perf_counter(); r = f(); ms.append((time.perf_counter() - t) * 1e3)
        wall[name] = stats(ms)
        kept[name] = r.clone() if name.startswith("partition_states") else r
    wall["host_route_parts"] = {k: stats(v) for k, v in parts.items()}
    assert torch.equal(kept["partition_states_cbs"], kept["partition_states_breakpoints"])          # the same segments either way
    (ids, code), ((host, hcode), tables) = kept["device_route"], kept["host_route"]
    a, b = comparable(ids), comparable(host)
    same = code == hcode and sorted(a) == sorted(b) and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a) and \
        all((np.asarray(ids["tables"][k]) == tables[k]).all() for k in ("chr_seg_offset", "seg_begin", "seg_end", "seg_bin_offset", "seg_ci4")) and \
        ids["tables"]["counts"].cpu().numpy().tobytes() == tables["counts"].tobytes()
    assert same, "the device route and the host route disagree"
    device = {}
    cv.profile_enable(1)
    for name in ("partition_states_cbs", "partition_states_breakpoints"):
        cv.profile_get("partition_states")
        for _ in range(3):
            routes[name]()
        ms, launches = cv.profile_get("partition_states")
        device[name] = dict(device_ms=round(ms / 3, 3), scopes_per_call=launches / 3)
    cv.profile_enable(0)
    print(json.dumps(dict(bins=args.bins, segments=int(ids["tables"]["nseg"]), sites=args.sites, call_code=code, stages=ids["stages"], runs=int(ids["nruns"]), routes_agree=bool(same),
                          wall_ms=wall, partition_states_scope=device)), flush=True)


if __name__ == "__main__":
    main()
