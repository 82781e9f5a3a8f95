#!/usr/bin/env python3
"""What CanvasBin -c costs on this box (not part of pytest or bench.py): writes a synthetic chromosome (100-base reads, --depth x --mb, half of them on the reverse
strand) and its kmer.fa, runs the executable --runs times after one warm-up process with CANVAS_TOOL_TIMING=1 — through canvas_hits_from_bam and, with the test hook
CANVAS_TOOL_HOST_BAM, through the host loop; --exe names another build (the parent commit's) to time the same way — then times canvas_hits_from_bam on the same
records resident in HBM.  Median and minimum of every figure; one JSON line per section.
usage: tools/hits_probe.py [--mb 40] [--depth 10] [--mode 5] [--runs 3] [--dir D] [--exe PATH] [--no-tool]"""
import argparse, json, os, struct, subprocess, sys, time, zlib
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("CANVAS_TEST_HOOKS", "1")
ap = argparse.ArgumentParser()
ap.add_argument("--mb", type=float, default=40); ap.add_argument("--depth", type=float, default=10); ap.add_argument("--mode", default="5")
ap.add_argument("--runs", type=int, default=3); ap.add_argument("--dir", default="/tmp/hits_probe"); ap.add_argument("--seed", type=int, default=1); ap.add_argument("--exe", action="append", default=[]); ap.add_argument("--no-tool", action="store_true")
a = ap.parse_args()
os.makedirs(a.dir, exist_ok=True)
L = 100; span = int(a.mb * 1e6); n = int(span * a.depth / L)
rng = np.random.RandomState(a.seed)
bam = os.path.join(a.dir, "probe.bam"); fa = os.path.join(a.dir, "kmer.fa")


def block(data):
    co = zlib.compressobj(1, zlib.DEFLATED, -15); c = co.compress(data) + co.flush()
    return struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(c) + 25) + c + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data))


t0 = time.time()
name = b"read/0000000\x00"
reclen = 32 + len(name) + 4 + (L + 1) // 2 + L
recs = np.zeros((n, 4 + reclen), np.uint8)
pos = np.sort(rng.randint(0, span - L, n)).astype("<i4")
recs[:, 0:4] = np.frombuffer(struct.pack("<i", reclen), np.uint8)
recs[:, 8:12] = pos.view(np.uint8).reshape(n, 4)
recs[:, 12] = len(name); recs[:, 13] = 60
recs[:, 16] = 1; flag = 0x3 | np.where(rng.rand(n) < 0.08, 0x400, 0) | np.where(rng.rand(n) < 0.5, 0x10, 0)
recs[:, 18] = flag & 0xFF; recs[:, 19] = flag >> 8
recs[:, 20:24] = np.frombuffer(struct.pack("<i", L), np.uint8)
recs[:, 32:36] = rng.randint(150, 600, n).astype("<i4").view(np.uint8).reshape(n, 4)
recs[:, 36:36 + len(name)] = np.frombuffer(name, np.uint8)
c0 = 36 + len(name)
recs[:, c0:c0 + 4] = np.frombuffer(struct.pack("<I", L << 4), np.uint8)
codes = np.array([1, 2, 4, 8], np.uint8)[rng.randint(0, 4, (n, L + (L & 1)), dtype=np.uint8)]
recs[:, c0 + 4:c0 + 4 + (L + 1) // 2] = (codes[:, 0::2] << 4) | codes[:, 1::2]
del codes
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
with open(fa, "wb") as f:
    f.write(b">chrP\n" + np.frombuffer(b"ACGTACGTACGTacgt", np.uint8)[rng.randint(0, 16, span, dtype=np.uint8)].tobytes() + b"\n")
kept = int(((flag & 0x410) == 0).sum())
print(json.dumps({"section": "input", "reads": n, "kept": kept, "positions": span, "record_bytes": len(stream), "bam_bytes": os.path.getsize(bam), "seconds_to_write": round(time.time() - t0, 1)}), flush=True)


def tool(exe, host, label):
    env = dict(os.environ, CANVAS_TOOL_TIMING="1", CANVAS_TOOL_THREADS=os.environ.get("CANVAS_TOOL_THREADS", "16"))
    env.pop("CANVAS_TOOL_HOST_BAM", None)
    if host:
        env["CANVAS_TOOL_HOST_BAM"] = "1"
    runs, dat = [], None
    for i in range(a.runs + 1):                       # the first process is the warm-up
        out = os.path.join(a.dir, "chrP.dat")
        t = time.time()
        r = subprocess.run([exe, "-b", bam, "-r", fa, "-c", "chrP", "-o", out, "-d", "100", "-m", a.mode, "-p"], capture_output=True, text=True, env=env)
        wall = time.time() - t
        assert r.returncode == 0, r.stderr
        ph = [json.loads(l) for l in r.stderr.splitlines() if l.startswith("{\"tool\"")]
        bl = [json.loads(l[6:]) for l in r.stderr.splitlines() if l.startswith("[bam] ")]
        row = dict(wall=wall, **(ph[0]["phases"] if ph else {}))
        if bl:
            row.update(kernel_ms=bl[0]["kernel_ms"], inflate_s=bl[0]["inflate_s"], device_wait_s=bl[0]["device_wait_s"]); row["_chunks"] = bl[0]["chunks"]; row["_host_path"] = bl[0]["host_path"]
        if i:
            runs.append(row)
        import hashlib
        dat = hashlib.sha256(open(out, "rb").read()).hexdigest()[:16]
        line = [l for l in r.stdout.splitlines() if l.startswith("Kept")]
    keys = [k for k in runs[0] if not k.startswith("_")]
    print(json.dumps({"section": "tool", "which": label, "runs": a.runs, "dat_sha": dat, "line": line, "chunks": runs[0].get("_chunks"), "host_path": runs[0].get("_host_path"),
                      "median": {k: round(float(np.median([r[k] for r in runs])), 4) for k in keys}, "min": {k: round(float(min(r[k] for r in runs)), 4) for k in keys}}), flush=True)


this = os.path.join(ROOT, "canvas_amd", "bin", "CanvasBin")
if not a.no_tool:
    tool(this, False, "this build, canvas_hits_from_bam")
    tool(this, True, "this build, host loop (CANVAS_TOOL_HOST_BAM)")
    for e in a.exe:
        tool(e, False, "other build: " + e)

import torch
from canvas_amd import Canvas
cv = Canvas(0)
d_rec = torch.from_numpy(recs.reshape(-1)).to(cv.device); d_off = torch.arange(n, dtype=torch.int64, device=cv.device) * (4 + reclen)
cv.profile_enable(True)                                # (the kernels run on the context's own stream: its event pairs time them, canvas_profile_get)
for mode in (0, 3, 5):
    ms = []
    for i in range(max(5, a.runs) + 1):
        hits = torch.zeros(span, dtype=torch.uint8, device=cv.device); frag = torch.zeros(span, dtype=torch.int16, device=cv.device); st = torch.zeros(8, dtype=torch.int64, device=cv.device)
        torch.cuda.synchronize()
        cv.hits_from_bam(d_rec, d_off, 0, span, mode, True, hits, frag, st, want_info=False)
        t, _ = cv.profile_get("hits_from_bam")
        if i:
            ms.append(t)
    med, mn = float(np.median(ms)), float(min(ms))
    state = st.cpu().numpy().tolist()
    # what has to move: 40 bytes of every record (block_size, fixed fields, first CIGAR word), 16 bytes of summary per record (written and read), and per kept read the
    # 32-byte sector of hits (read + written) and, in mode 5, of frag (written)
    must = n * (40 + 8 + 16) + state[2] * (64 + (32 if mode == 5 else 0))
    print(json.dumps({"section": "kernel_resident", "mode": mode, "state": state, "ms_median": round(med, 4), "ms_min": round(mn, 4), "records_per_s_median": round(n / med * 1e3),
                      "record_GBps_over_all_record_bytes": round(len(stream) / med / 1e6, 1), "must_move_bytes": must, "must_move_GBps_median": round(must / med / 1e6, 1),
                      "note": "compare with tools/bw_probe.py on the same box"}), flush=True)
