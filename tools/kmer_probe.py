"""canvas_flag_unique_kmers on a human-sized synthetic genome (3.1 Gb, generated in HBM by the bench's synth kernel, repeats planted on top):
    python tools/kmer_probe.py [--scale 1.0] [--plants 6000] [--small-table-divisor 4]
prints, as JSON lines: per-sweep milliseconds (hipEvent pairs around kmer_hist / kmer_insert / kmer_lookup), keyed positions per second of sweep A (>= one 64-bit atomic
each unless the slot already shows "more than once"), table bytes, longest probe, and a digest of the masks under the default table and under a table
--small-table-divisor times smaller (several passes): the two digests must match.
    python tools/kmer_probe.py --host-rate [--host-bases 10000000]
needs no GPU: the same first bases of chr1 (numpy mirror of the generator, the same plants) through the line-by-line restatement of KmerChecker (tests/kmer_ref.py) on one
host core — the only reference figure there is (the C# tool needs Isas.SequencingFiles to build)."""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from canvas_amd import synth

SEED = 20261017
RATE = 0.21


def plant_list(lengths, plants, seed=SEED):
    """[(kind, src chr, src pos, dst chr, dst pos, length, period)]: kind 0 forward copy, 1 reverse-complement copy, 2 tandem repeat of src[:period].  Sources are read
    from the genome as generated (before any plant), so a host mirror can rebuild any destination range without the rest of the genome."""
    rng = np.random.RandomState(seed)
    n = len(lengths)
    out = []
    for i in range(plants):
        kind = i % 3
        ln = int(rng.randint(100, 20000))
        s = int(rng.randint(n)); d = int(rng.randint(n)) if i % 2 else s
        ln = min(ln, lengths[s] // 8, lengths[d] // 8)
        out.append((kind, s, int(rng.randint(0, lengths[s] - ln)), d, int(rng.randint(0, lengths[d] - ln)), ln, 1 + int(rng.randint(40))))
    return out


_RC = np.arange(256, dtype=np.uint8)
for a_, b_ in zip(b"ACGTacgt", b"TGCAtgca"):
    _RC[a_] = b_


def planted_piece_host(kind, src, ln, period):
    if kind == 0:
        return src.copy()
    if kind == 1:
        return _RC[src][::-1].copy()
    return np.tile(src[:period], ln // period + 1)[:ln]


def host_rate(args):
    import kmer_ref as R
    lengths = [int(L * args.scale) for L in synth.GRCH38]
    N = min(args.host_bases, lengths[0])
    thr = synth.poisson_thresholds(RATE)
    gen = lambda c, lo, hi: synth._generate_range(SEED, c, lengths[c], thr, SEED, False, lo, hi)[0]
    b = np.concatenate([gen(0, a, min(N, a + (1 << 22))) for a in range(0, N, 1 << 22)])
    for kind, s, s0, d, d0, ln, period in plant_list(lengths, args.plants):
        if d == 0 and d0 < N:
            piece = planted_piece_host(kind, gen(s, s0, s0 + ln), ln, period)
            k = min(ln, N - d0)
            b[d0:d0 + k] = piece[:k]
    t0 = time.perf_counter()
    flags, passes = R.unique_flags_checker([b.tobytes()])
    dt = time.perf_counter() - t0
    print(json.dumps(dict(what="KmerChecker restatement (tests/kmer_ref.py), one host core", bases=N, seconds=round(dt, 1), positions_per_second=round(N / dt), unique=int(flags[0].sum()), passes=passes)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--plants", type=int, default=6000)
    ap.add_argument("--small-table-divisor", type=int, default=4)
    ap.add_argument("--host-rate", action="store_true")
    ap.add_argument("--host-bases", type=int, default=10_000_000)
    args = ap.parse_args()
    if args.host_rate:
        return host_rate(args)
    import torch
    from canvas_amd import Canvas
    from canvas_amd.lib import synth_generate_device
    cv = Canvas(0); dev = cv.device
    lengths = [int(L * args.scale) for L in synth.GRCH38]
    thr = None; bases = []
    for c, L in enumerate(lengths):
        b, h, m, thr = synth_generate_device(SEED, c, L, RATE, dev, thr)
        del h, m
        bases.append(b)
    torch.cuda.synchronize()
    plants = plant_list(lengths, args.plants)
    rc = torch.from_numpy(_RC).to(dev)
    pieces = []
    for kind, s, s0, d, d0, ln, period in plants:             # every source as generated, then the writes in order
        src = bases[s][s0:s0 + ln]
        pieces.append(src.clone() if kind == 0 else rc[src.long()].flip(0) if kind == 1 else src[:period].repeat(ln // period + 1)[:ln])
    for (kind, s, s0, d, d0, ln, period), piece in zip(plants, pieces):
        bases[d][d0:d0 + ln] = piece
    del pieces
    torch.cuda.synchronize()
    lens = np.array(lengths, np.int64)
    masks = [torch.empty((L + 63) // 64, dtype=torch.int64, device=dev) for L in lengths]

    def run(budget, label):
        cv.profile_enable(1)
        for name in ("kmer_hist", "kmer_insert", "kmer_lookup"):
            cv.profile_get(name)
        t0 = time.perf_counter()
        _, st = cv.flag_unique_kmers(bases, lens, masks=masks, max_table_bytes=budget)
        wall = time.perf_counter() - t0
        ms = {name: cv.profile_get(name) for name in ("kmer_hist", "kmer_insert", "kmer_lookup")}
        cv.profile_enable(0)
        h = hashlib.sha256()
        for m in masks:
            h.update(m.cpu().numpy().tobytes())
        ins = ms["kmer_insert"][0]
        rec = dict(run=label, positions=st["positions"], keyed=st["keyed"], unique=st["unique"], passes=st["passes"], table_bytes=st["table_bytes"], longest_probe=st["longest_probe"],
                   wall_s=round(wall, 3), hist_ms=round(ms["kmer_hist"][0], 2), insert_ms=round(ins, 2), lookup_ms=round(ms["kmer_lookup"][0], 2), launches=[ms[k][1] for k in ms],
                   keyed_per_second_sweep_a=round(st["keyed"] / (ins * 1e-3)) if ins > 0 else None, mask_sha256=h.hexdigest()[:32])
        print(json.dumps(rec), flush=True)
        return rec

    a = run(0, "default table")
    run(0, "default table, again")
    b = run(a["table_bytes"] // args.small_table_divisor, "table / %d" % args.small_table_divisor)
    print(json.dumps(dict(digests_match=a["mask_sha256"] == b["mask_sha256"])), flush=True)
    if a["mask_sha256"] != b["mask_sha256"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
