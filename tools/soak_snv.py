#!/usr/bin/env python3
"""Randomised parity soak of canvas_snv_count on the GPU against the sequential restatement (tests/snv_ref.py); not part of pytest: larger inputs than
tests/test_snv_gpu.py.  usage: tools/soak_snv.py [minutes [seed]]; the summary line belongs in profiles/."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import snv_ref as R
import snv_cases as SC
from canvas_amd import Canvas
from canvas_amd.lib import snv_allele_codes

cv = Canvas(0)
budget = float(sys.argv[1]) * 60 if len(sys.argv) > 1 else 120
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 7
rng = np.random.RandomState(seed)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cv.device)
t0 = time.time(); it = 0; nreads = 0; nsites = 0; ncalls = 0; walked = 0; stopped = 0
while time.time() - t0 < budget:
    span = int(rng.choice([500, 5000, 60000, 400000])); n = int(rng.choice([200, 2000, 12000]))
    every = int(rng.choice([1, 10, 100, 1000, 10000]))
    if every == 1:
        span = min(span, 60000)
    reads = SC.random_reads(rng, n, span, long_frac=float(rng.choice([0, 0.02, 0.2])), exotic=float(rng.choice([0, 0.05, 0.3])))
    sites = SC.random_sites(rng, span + 500, every)
    mq = int(rng.choice([0, 5, 29]))
    exp = R.pileup(reads, 0, sites, mq)
    pos = dev(np.array([v.pos for v in sites], np.int32)); ref = dev(snv_allele_codes([v.ref for v in sites])); alt = dev(snv_allele_codes([v.alt for v in sites]))
    for nchunks in (1, 2, int(rng.randint(3, 40))):
        cuts = [0] + sorted(rng.randint(0, n + 1, nchunks - 1).tolist()) + [n]
        rc = ac = None; info = np.zeros(5, np.int64)
        for a, b in zip(cuts[:-1], cuts[1:]):
            buf, offs, nbytes = SC.chunk_of(reads[a:b], 0)
            d_buf = dev(buf) if len(buf) else torch.zeros(1, dtype=torch.uint8, device=cv.device)
            d_off = dev(offs) if len(offs) else torch.zeros(0, dtype=torch.int64, device=cv.device)
            rc, ac, i5 = cv.snv_count(d_buf, d_off, 0, pos, ref, alt, rc, ac, min_mapq=mq, nbytes=nbytes); info += i5; ncalls += 1
        got = (rc.cpu().numpy()[:len(sites)].tolist(), ac.cpu().numpy()[:len(sites)].tolist())
        if got != (list(exp[0]), list(exp[1])) or info[0] != n or info[4] != 0:
            print(f"MISMATCH seed {seed} iteration {it}: span {span} reads {n} one site per {every} min_mapq {mq} chunks {nchunks} info {info.tolist()}"); sys.exit(1)
        walked += int(info[2]); stopped += int(info[3])
    it += 1; nreads += n; nsites += len(sites)
print(f"soak_snv ok: seed {seed}, {it} configurations x 3 chunkings, {nreads} reads, {nsites} sites, {ncalls} calls, {walked} walks ({stopped} ended at an unsupported CIGAR operation), {time.time() - t0:.0f} s")
