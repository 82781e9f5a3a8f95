"""Inputs shared by the CanvasSmooth tests, and the runner that puts them through Canvas.smooth.

Run as a program (`python tests/smooth_cases.py OUT.npz [--per-pass]`) it runs every case in a process of its own and stores the results; with --per-pass it sets
CANVAS_SMOOTH_PER_PASS once the cases are made (their sizes come from the fused path's plan), so that every call takes the per-pass path: tests/test_smooth_gpu.py
gets that path's answers next to the fused path's this way."""
import os
import sys

import numpy as np

import smooth_ref as R

KINDS = ("ties", "equal", "monotone", "spikes", "big")
SENTINEL = np.uint32(0x7FC12345)                         # a NaN no kernel produces: what canvas_smooth must leave alone


def data(kind, n, seed):
    """non-negative finite counts"""
    rng = np.random.RandomState(seed)
    if kind == "ties":                                   # two-decimal values out of a few dozen: most windows hold equal values
        return (rng.randint(9000, 9040, n) / 100.0).astype(np.float32)
    if kind == "equal":
        return np.full(n, 100.25, np.float32)
    if kind == "monotone":
        return (1.0 + 0.25 * np.arange(n)).astype(np.float32)
    if kind == "spikes":
        return np.where(np.arange(n) % 2 == 0, 10.0, 1000.0).astype(np.float32)
    if kind == "big":                                    # floats are 2 apart here: the mean of two neighbours is not a float and has to round
        return (3.0e7 + 2.0 * rng.randint(0, 40, n)).astype(np.float32)
    raise ValueError(kind)


def plan(W):
    from canvas_amd.lib import smooth_plan
    return smooth_plan(W)


def largest_fused_w():
    W = 1
    while plan(W + 1)["fused"]:
        W += 1
    return W


def _one(group, name, W, pieces):
    off = np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).astype(np.int64)
    counts = np.concatenate(pieces).astype(np.float32) if pieces else np.zeros(0, np.float32)
    return dict(group=group, name=name, W=W, off=off, counts=counts)


def cases():
    out = []
    for W in (1, 2, 3, 4):                               # every length around the truncation, one chromosome each and all of them in one call
        pieces = []
        for n in range(0, 2 * W + 4):
            for kind in KINDS:
                p = data(kind, n, 100 * W + n)
                out.append(_one("small", "W%d-n%d-%s" % (W, n, kind), W, [p]))
                pieces.append(p)
        out.append(_one("small-concat", "W%d" % W, W, pieces))
    for W in sorted({1, 3, largest_fused_w()}):          # the edges of a tile and of its halo
        pl = plan(W); T, H = pl["tile"], pl["halo"]
        assert pl["fused"] and H == W * (W + 1) // 2 and T > 2 * W + 1
        for n in (T - 1, T, T + 1, T + H, T + H + 1, 3 * T + 17):
            out.append(_one("tile", "W%d-n%d-ties" % (W, n), W, [data("ties", n, n)]))
        for kind in KINDS[1:]:
            out.append(_one("tile", "W%d-n%d-%s" % (W, T + H + 1, kind), W, [data(kind, T + H + 1, W)]))
    rng = np.random.RandomState(4242)
    for W in (2, 5):                                     # chromosome ends at every offset of a tile and of a halo
        lens = rng.randint(0, 41, 3000)
        out.append(_one("many", "W%d" % W, W, [data("ties", int(n), 7000 + i) for i, n in enumerate(lens)]))
    c = _one("many", "W3-offset", 3, [data("ties", int(n), 9000 + i) for i, n in enumerate(rng.randint(0, 41, 500))])
    c["off"] = c["off"] + 7; c["counts"] = np.concatenate([np.full(7, 5.0, np.float32), c["counts"], np.full(3, 6.0, np.float32)])      # bins in front of and behind the call's range
    out.append(c)
    return out


def expected(case, one=R.smooth_windows):
    """(out_n, the bits of d_out when it was filled with SENTINEL before the call)"""
    off, x = case["off"], case["counts"]
    bits = np.full(len(x), SENTINEL, np.uint32)
    out_n = np.zeros(len(off) - 1, np.int64)
    for c, s in enumerate(R.smooth_genome(x, off, case["W"], one)):
        out_n[c] = len(s)
        bits[int(off[c]):int(off[c]) + len(s)] = np.asarray(s, np.float32).view(np.uint32)
    return out_n, bits


def run_case(cv, case):
    import torch
    x = case["counts"]
    d = torch.from_numpy(x if len(x) else np.zeros(1, np.float32)).to(cv.device)
    o = torch.from_numpy(np.full(max(len(x), 1), SENTINEL, np.uint32).view(np.float32)).to(cv.device)
    _, out_n = cv.smooth(d, case["off"], case["W"], out=o)
    return np.array(out_n, np.int64), o.cpu().numpy().view(np.uint32)[:len(x)].copy()


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from canvas_amd import Canvas
    todo = cases()
    if "--per-pass" in sys.argv[2:]:
        os.environ["CANVAS_SMOOTH_PER_PASS"] = "1"      # (read by the library at every call, and only with CANVAS_TEST_HOOKS set)
    cv = Canvas(0)
    res = {"fused_w1": np.array([int(plan(1)["fused"])])}
    for i, case in enumerate(todo):
        res["n%d" % i], res["o%d" % i] = run_case(cv, case)
    np.savez(sys.argv[1], **res)


if __name__ == "__main__":
    main()
