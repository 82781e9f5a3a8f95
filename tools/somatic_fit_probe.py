"""canvas_somatic_model_fit with the default parameters on synthetic whole-genome-like input:
    python tools/somatic_fit_probe.py [--segments 100 3000] [--median 100] [--reps 3]
For each S: S segments around a median coverage of `median` (a tumour of purity 70 %, copy numbers 1 .. 4, a quarter of the segments without MAF), the grid of the
reference (diploid coverage median / 4 .. median * 2.355, purity from the hard limit 20), and as one JSON line the number of models and the wall time of the call with
its four parts as the library reports them (host table, upload, device, selection; the minimum and the median over the repetitions after one warm-up call), and the
device time of the grid kernel alone from canvas_profile_get."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("CANVAS_TEST_HOOKS", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def segments(rng, n, median):
    purity, diploid = 0.7, median
    cn = rng.choice([1, 2, 2, 2, 3, 4], n)
    major = np.array([rng.integers((c + 1) // 2, c + 1) for c in cn])
    cov = diploid * (purity * cn / 2 + (1 - purity)) + rng.normal(0, 0.02 * median, n)
    maf = np.clip((purity * (cn - major) + (1 - purity)) / (purity * cn + 2 * (1 - purity)) * 0.97 + rng.normal(0, 0.01, n), 0, 0.5)
    maf[rng.random(n) < 0.25] = -1.0
    length = rng.integers(10_000, 2_000_000, n).astype(np.int32)
    return np.abs(cov), maf, length.astype(np.float64), length


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, nargs="+", default=[100, 3000])
    ap.add_argument("--median", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from canvas_amd import Canvas
    cv = Canvas(0)
    lo, hi = int(max(10, args.median / 4)), int(max(10, args.median * 2.355))
    for S in args.segments:
        cov, maf, w, length = segments(np.random.default_rng(S), S, args.median)
        mmac = float(np.median(cov)) * 0.45          # a diploid cluster: the lower purity is the hard limit for most coverages
        call = lambda: cv.somatic_model_fit(cov, maf, w, length, 0.6 / float(np.median(cov)), 3_000_000_000, lo, hi, minimum_purity_hard_limit=20,
                                            min_minor_allele_coverage=mmac, all_models=False)
        call()
        rows, wall = [], []
        cv.profile_enable(1); cv.profile_get("somatic_fit")
        for _ in range(args.reps):
            t = time.perf_counter(); r = call(); wall.append((time.perf_counter() - t) * 1e3)
            rows.append(r["times_ms"])
        kernel_ms, launches = cv.profile_get("somatic_fit")
        cv.profile_enable(0)
        part = lambda k: dict(min=round(min(x[k] for x in rows), 3), median=round(float(np.median([x[k] for x in rows])), 3))
        print(json.dumps(dict(segments=S, median=args.median, coverages=[lo, hi], models=r["nmodels"], best=[r["coverage"], r["percent_purity"]], info=r["info"],
                              wall_ms=dict(min=round(min(wall), 3), median=round(float(np.median(wall)), 3)), host_table_ms=part("host_table"), upload_ms=part("upload"),
                              device_ms=part("device"), selection_ms=part("selection"), grid_kernel_ms=round(kernel_ms / max(launches, 1), 3))), flush=True)


if __name__ == "__main__":
    main()
