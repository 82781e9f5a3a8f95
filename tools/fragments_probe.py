#!/usr/bin/env python3
"""What CanvasBin -m Fragment costs on this box (not part of pytest or bench.py): writes a synthetic paired-end chromosome (--pairs pairs of 100-base reads over --mb,
insert sizes 150-600, a few duplicates and low mapping qualities on either mate) and a BED file of --bins equal bins, runs the executable --runs times after one
warm-up process with CANVAS_TOOL_TIMING=1 — through canvas_fragments_from_bam and, with the test hook CANVAS_TOOL_HOST_BAM, through the host loop (the parent
commit's Fragment mode, unchanged); --exe names another build to time the same way — then times canvas_fragments_from_bam chunk by chunk on the same records
resident in HBM.  Median and minimum of every figure; one JSON line per section.
usage: tools/fragments_probe.py [--mb 60] [--pairs 1000000] [--bins 30000] [--runs 3] [--dir D] [--exe PATH] [--no-tool] [--chunk-mb 32]"""
import argparse, hashlib, json, os, struct, subprocess, sys, time, zlib
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("CANVAS_TEST_HOOKS", "1")
ap = argparse.ArgumentParser()
ap.add_argument("--mb", type=float, default=60); ap.add_argument("--pairs", type=int, default=1000000); ap.add_argument("--bins", type=int, default=30000)
ap.add_argument("--runs", type=int, default=3); ap.add_argument("--dir", default="/tmp/fragments_probe"); ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--exe", action="append", default=[]); ap.add_argument("--no-tool", action="store_true"); ap.add_argument("--chunk-mb", type=float, default=32)
a = ap.parse_args()
os.makedirs(a.dir, exist_ok=True)
L = 100; span = int(a.mb * 1e6); npairs = a.pairs; n = 2 * npairs
rng = np.random.RandomState(a.seed)
bam = os.path.join(a.dir, "probe.bam"); fa = os.path.join(a.dir, "genome.fa"); bed = os.path.join(a.dir, "bins.bed")


def block(data):
    co = zlib.compressobj(1, zlib.DEFLATED, -15); c = co.compress(data) + co.flush()
    return struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(c) + 25) + c + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data))


t0 = time.time()
NAME = 15                                             # "read/" + 9 digits + NUL
reclen = 32 + NAME + 4 + (L + 1) // 2 + L
left = rng.randint(0, span - 800, npairs).astype(np.int64); insert = rng.randint(150, 600, npairs).astype(np.int64); right = left + np.maximum(insert - L, 0)
pair_id = np.arange(npairs, dtype=np.int64)
pos = np.concatenate([left, right]); mate = np.concatenate([right, left]); tlen = np.concatenate([insert, -insert]); ids = np.concatenate([pair_id, pair_id])
flag = np.concatenate([np.full(npairs, 0x63), np.full(npairs, 0x93)]) | np.where(rng.rand(n) < 0.04, 0x400, 0)
mapq = np.where(rng.rand(n) < 0.05, 0, 60)
order = np.argsort(pos, kind="stable")
pos, mate, tlen, ids, flag, mapq = (x[order] for x in (pos, mate, tlen, ids, flag, mapq))
recs = np.zeros((n, 4 + reclen), np.uint8)
recs[:, 0:4] = np.frombuffer(struct.pack("<i", reclen), np.uint8)
recs[:, 8:12] = pos.astype("<i4").view(np.uint8).reshape(n, 4)
recs[:, 12] = NAME; recs[:, 13] = mapq
recs[:, 16] = 1; recs[:, 18] = flag & 0xFF; recs[:, 19] = flag >> 8
recs[:, 20:24] = np.frombuffer(struct.pack("<i", L), np.uint8)
recs[:, 28:32] = mate.astype("<i4").view(np.uint8).reshape(n, 4)          # (refID and next_refID stay 0)
recs[:, 32:36] = tlen.astype("<i4").view(np.uint8).reshape(n, 4)
recs[:, 36:41] = np.frombuffer(b"read/", np.uint8)
for d in range(9):
    recs[:, 41 + d] = 48 + (ids // 10 ** (8 - d)) % 10
c0 = 36 + NAME
recs[:, c0:c0 + 4] = np.frombuffer(struct.pack("<I", L << 4), np.uint8)
recs[:, c0 + 4:c0 + 4 + (L + 1) // 2] = rng.randint(0, 256, (n, (L + 1) // 2)).astype(np.uint8) & 0x77 | 0x11
recs[:, c0 + 4 + (L + 1) // 2:] = np.array([12, 25, 25, 25, 25, 37, 37, 37, 37, 37, 37, 37, 37, 37, 37, 37], np.uint8)[rng.randint(0, 16, (n, L), dtype=np.uint8)]
stream = recs.tobytes()
text = b"@HD\tVN:1.0\tSO:coordinate\n"
hdr = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", 1) + struct.pack("<i", 5) + b"chrP\x00" + struct.pack("<i", span)
with open(bam, "wb") as f:
    f.write(block(hdr)); first = f.tell()
    for i in range(0, len(stream), 65280):
        f.write(block(stream[i:i + 65280]))
    end = f.tell(); f.write(block(b""))
open(bam + ".bai", "wb").write(b"BAI\x01" + struct.pack("<i", 1) + struct.pack("<i", 1) + struct.pack("<Ii", 0, 1) + struct.pack("<QQ", first << 16, end << 16) + struct.pack("<i", 0))
open(fa, "wb").write(b">chrP\nACGT\n")                # every bin carries its GC content: the FASTA is not read
width = span // a.bins
bin_start = np.arange(a.bins, dtype=np.int64) * width; bin_stop = bin_start + width
with open(bed, "w") as f:
    f.write("".join("chrP\t%d\t%d\t50\n" % (s, e) for s, e in zip(bin_start, bin_stop)))
print(json.dumps({"section": "input", "records": n, "pairs": npairs, "positions": span, "bins": a.bins, "record_bytes": len(stream), "bytes_per_record": 4 + reclen,
                  "bam_bytes": os.path.getsize(bam), "seconds_to_write": round(time.time() - t0, 1)}), flush=True)


def tool(exe, host, label):
    env = dict(os.environ, CANVAS_TOOL_TIMING="1", CANVAS_TOOL_THREADS=os.environ.get("CANVAS_TOOL_THREADS", "16"))
    env.pop("CANVAS_TOOL_HOST_BAM", None)
    if host:
        env["CANVAS_TOOL_HOST_BAM"] = "1"
    runs, sha, frag = [], None, None
    for i in range(a.runs + 1):                       # the first process is the warm-up
        out = os.path.join(a.dir, "probe.binned")
        t = time.time()
        r = subprocess.run([exe, "-b", bam, "-r", fa, "-n", bed, "-o", out, "-m", "Fragment", "-p"], capture_output=True, text=True, env=env)
        wall = time.time() - t
        assert r.returncode == 0, r.stderr
        ph = [json.loads(l) for l in r.stderr.splitlines() if l.startswith("{\"tool\"")]
        fl = [json.loads(l[7:]) for l in r.stderr.splitlines() if l.startswith("[frag] ")]
        row = dict(wall=wall, **(ph[0]["phases"] if ph else {}))
        if fl:
            frag = fl[0]
            row.update(kernel_ms=frag["kernel_ms"], inflate_s=frag["inflate_s"], device_wait_s=frag["device_wait_s"])
        if i:
            runs.append(row)
        sha = hashlib.sha256(open(out, "rb").read()).hexdigest()[:16]
    keys = list(runs[0])
    print(json.dumps({"section": "tool", "which": label, "runs": a.runs, "binned_sha": sha, "frag_line_of_the_last_run": frag,
                      "median": {k: round(float(np.median([r[k] for r in runs])), 4) for k in keys}, "min": {k: round(float(min(r[k] for r in runs)), 4) for k in keys}}), flush=True)


this = os.path.join(ROOT, "canvas_amd", "bin", "CanvasBin")
if not a.no_tool:
    tool(this, False, "this build, canvas_fragments_from_bam")
    tool(this, True, "this build, host loop (CANVAS_TOOL_HOST_BAM): the parent commit's Fragment mode")
    for e in a.exe:
        tool(e, False, "other build: " + e)

import torch
from canvas_amd import Canvas
cv = Canvas(0)
per_chunk = max(1, int(a.chunk_mb * (1 << 20)) // (4 + reclen))
d_start = torch.from_numpy(bin_start.astype(np.int32)).to(cv.device); d_stop = torch.from_numpy(bin_stop.astype(np.int32)).to(cv.device)
chunks = []
for lo in range(0, n, per_chunk):
    hi = min(n, lo + per_chunk)
    chunks.append((torch.from_numpy(recs[lo:hi].reshape(-1)).to(cv.device), torch.arange(hi - lo, dtype=torch.int64, device=cv.device) * (4 + reclen)))
cv.profile_enable(True)                                # (the kernels run on the context's own stream: its event pairs time them, canvas_profile_get)
rows = []
for i in range(max(3, a.runs) + 1):
    counts = carry = state = None
    ms, carried, wall = [], [], []
    for d_rec, d_off in chunks:
        t = time.time()
        counts, carry, state, info = cv.fragments_from_bam(d_rec, d_off, 0, d_start, d_stop, 3, counts, carry, state)
        wall.append((time.time() - t) * 1e3)
        ms.append(cv.profile_get("fragments_from_bam")[0]); carried.append(int(info[7]))
    if i:
        rows.append((ms, wall))
kernel = np.median(np.array([r[0] for r in rows]), axis=0); wall = np.median(np.array([r[1] for r in rows]), axis=0)
# what has to move per record: 36 fixed bytes and the name twice (hash; comparison with the mate) out of the chunk, 32 bytes of summary written and read three times,
# 4 of link + 4 of leader written and read, 4 of event cleared, written for one record in two and read, 8 of slot head cleared and exchanged
must = n * (36 + 2 * (NAME - 1) + 32 * 4 + 16 + 12 + 16)
print(json.dumps({"section": "kernel_resident", "chunks": len(chunks), "records_per_chunk": per_chunk, "state": [int(x) for x in info[:11]], "usable": int(info[3]),
                  "kernel_ms_per_chunk_median": [round(float(x), 3) for x in kernel], "call_wall_ms_per_chunk_median": [round(float(x), 3) for x in wall],
                  "kernel_ms_total": round(float(kernel.sum()), 3), "records_per_s": round(n / float(kernel.sum()) * 1e3), "carried_entries_per_chunk": carried,
                  "longest_group": int(info[10]), "bytes_read_per_record_from_the_chunk": 36 + 2 * (NAME - 1), "must_move_bytes": must,
                  "must_move_GBps": round(must / float(kernel.sum()) / 1e6, 1), "counts_sum": int(counts.sum().item())}), flush=True)
