"""canvas_smooth on a genome-sized input that stays in HBM (3 000 000 bins in 24 chromosomes, two-decimal counts with ties):
    python tools/smooth_probe.py [--bins 3000000] [--reps 20]
prints, as JSON lines, for W in {1, 3, 10} the kernel time per call of the fused path ("smooth_fused") and of the per-pass path forced through
CANVAS_SMOOTH_PER_PASS ("smooth_pass", all its launches of one call together), taken from canvas_profile_get (hipEvent pairs around the kernels), the two paths
alternating in one process after a warm-up of each; next to them the floor of 8 B per bin (one float read, one written) at the streaming-read rate measured here
the way tools/bw_probe.py measures it, and whether the two paths gave the same bits."""
import argparse
import json
import os
import sys

os.environ.setdefault("CANVAS_TEST_HOOKS", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=3_000_000)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import time
    import torch
    from canvas_amd import Canvas
    from canvas_amd.lib import smooth_plan
    cv = Canvas(0); dev = cv.device
    # streaming-read rate (tools/bw_probe.py's first figure, on 2 GiB)
    x = torch.ones(2 * 1024**3 // 8, dtype=torch.int64, device=dev)
    for _ in range(3):
        x.sum()
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(10):
        x.sum()
    torch.cuda.synchronize(); read_tbs = x.numel() * 8 / ((time.perf_counter() - t) / 10) / 1e12
    del x
    rng = np.random.RandomState(1)
    w = rng.uniform(0.5, 2.0, 24); lens = np.floor(w / w.sum() * args.bins).astype(np.int64); lens[0] += args.bins - lens.sum()
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    counts = torch.from_numpy((np.round(rng.gamma(40.0, 2.5, args.bins) * 100) / 100).astype(np.float32)).to(dev)
    out = torch.empty_like(counts)
    floor_us = 8.0 * args.bins / (read_tbs * 1e12) * 1e6
    print(json.dumps(dict(bins=args.bins, chromosomes=24, streaming_read_TBps=round(read_tbs, 3), floor_us_8B_per_bin=round(floor_us, 2))), flush=True)

    def timed(W, per_pass, reps):
        if per_pass:
            os.environ["CANVAS_SMOOTH_PER_PASS"] = "1"
        else:
            os.environ.pop("CANVAS_SMOOTH_PER_PASS", None)
        name = "smooth_pass" if per_pass else "smooth_fused"
        assert smooth_plan(W)["fused"] == (not per_pass)
        cv.profile_enable(1); cv.profile_get(name)
        for _ in range(reps):
            cv.smooth(counts, off, W, out=out)
        ms, launches = cv.profile_get(name)
        cv.profile_enable(0)
        return ms / reps * 1e3, launches // reps, out.clone()

    for W in (1, 3, 10):
        timed(W, False, 3); timed(W, True, 1)             # warm-up of both paths at this W
        rows = []
        for rnd in range(2):                              # alternating, twice: the spread between the rounds is the noise
            fu, fl, fo = timed(W, False, args.reps)
            pu, plaunch, po = timed(W, True, max(2, args.reps // 4))
            rows.append((fu, pu))
        same = bool(torch.equal(fo.view(torch.int32), po.view(torch.int32)))
        os.environ.pop("CANVAS_SMOOTH_PER_PASS", None)
        print(json.dumps(dict(W=W, plan=smooth_plan(W), fused_us=[round(r[0], 1) for r in rows], fused_launches=fl,
                              per_pass_us=[round(r[1], 1) for r in rows], per_pass_launches=plaunch, fused_over_floor=round(min(r[0] for r in rows) / floor_us, 2),
                              per_pass_over_floor=round(min(r[1] for r in rows) / floor_us, 2), same_bits=same)), flush=True)
        if not same:
            sys.exit(1)


if __name__ == "__main__":
    main()
