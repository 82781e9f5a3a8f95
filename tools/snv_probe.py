#!/usr/bin/env python3
"""What CanvasSNV costs on this box (not part of pytest or bench.py): writes a synthetic chromosome (150-base reads, --depth x --mb), runs the executable
--runs times with CANVAS_TOOL_TIMING=1 (phases, the kernel's own ms, overlap = inflate + device-wait against the loop's wall time), then times canvas_snv_count on the
same records resident in HBM.  Median and minimum of every figure; one JSON line per section.  usage: tools/snv_probe.py [--mb 50] [--depth 30] [--every 1000] [--runs 3] [--dir D]"""
import argparse, json, os, struct, subprocess, sys, time, zlib
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--mb", type=float, default=50); ap.add_argument("--depth", type=float, default=30); ap.add_argument("--every", type=int, default=1000)
ap.add_argument("--runs", type=int, default=3); ap.add_argument("--dir", default="/tmp/snv_probe"); ap.add_argument("--seed", type=int, default=1)
a = ap.parse_args()
os.makedirs(a.dir, exist_ok=True)
L = 150; span = int(a.mb * 1e6); n = int(span * a.depth / L)
rng = np.random.RandomState(a.seed)
bam = os.path.join(a.dir, "probe.bam"); vcf = os.path.join(a.dir, "probe.vcf")


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
recs[:, 12] = len(name); recs[:, 13] = np.array([0, 30, 30, 30] + [60] * 12, np.uint8)[rng.randint(0, 16, n)]
recs[:, 16] = 1; flag = np.where(rng.rand(n) < 0.08, 0x400, 0) | np.where(rng.rand(n) < 0.5, 0x10, 0)
recs[:, 18] = flag & 0xFF; recs[:, 19] = flag >> 8
recs[:, 20:24] = np.frombuffer(struct.pack("<i", L), np.uint8)
recs[:, 24:28] = 255; recs[:, 28:32] = 255
recs[:, 36:36 + len(name)] = np.frombuffer(name, np.uint8)
c0 = 36 + len(name)
recs[:, c0:c0 + 4] = np.frombuffer(struct.pack("<I", L << 4), np.uint8)
codes = np.array([1, 2, 4, 8], np.uint8)[rng.randint(0, 4, (n, L + (L & 1)), dtype=np.uint8)]
recs[:, c0 + 4:c0 + 4 + (L + 1) // 2] = (codes[:, 0::2] << 4) | codes[:, 1::2]
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
sp = np.sort(rng.randint(1, span, max(1, span // a.every)))
with open(vcf, "w") as f:
    f.write("##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n")
    for p in sp:
        r, v = rng.choice(4, 2, replace=False)
        f.write("chrP\t%d\t.\t%s\t%s\t.\tPASS\t.\tGT\t0/1\n" % (p, "ACGT"[r], "ACGT"[v]))
print(json.dumps({"section": "input", "reads": n, "record_bytes": len(stream), "bam_bytes": os.path.getsize(bam), "sites": len(sp), "seconds_to_write": round(time.time() - t0, 1)}))

exe = os.path.join(ROOT, "canvas_amd", "bin", "CanvasSNV")
runs = []
for i in range(a.runs):
    t = time.time()
    r = subprocess.run([exe, "-c", "chrP", "-v", vcf, "-b", bam, "-o", os.path.join(a.dir, "out.txt.gz")], capture_output=True, text=True, env=dict(os.environ, CANVAS_TOOL_TIMING="1", CANVAS_TOOL_THREADS=os.environ.get("CANVAS_TOOL_THREADS", "16")))
    wall = time.time() - t
    assert r.returncode == 0, r.stderr
    ph = [json.loads(l) for l in r.stderr.splitlines() if l.startswith("{\"tool\"")][0]
    snv = [json.loads(l[6:]) for l in r.stderr.splitlines() if l.startswith("[snv] ")][0]
    runs.append(dict(wall=wall, **ph["phases"], total=ph["total"], kernel_ms=snv["kernel_ms"], chunks=snv["chunks"], threads=snv["threads"]))
keys = [k for k in runs[0] if k not in ("chunks", "threads")]
print(json.dumps({"section": "tool", "runs": a.runs, "threads": runs[0]["threads"], "chunks": runs[0]["chunks"], "median": {k: round(float(np.median([r[k] for r in runs])), 4) for k in keys},
                  "min": {k: round(float(min(r[k] for r in runs)), 4) for k in keys},
                  "note": "inflate + device = the loop's wall time; device = what of the device work did not hide behind inflation; kernel_ms = hipEvents around the kernels"}))

import torch
from canvas_amd import Canvas
from canvas_amd.lib import snv_allele_codes
cv = Canvas(0)
d_rec = torch.from_numpy(recs.reshape(-1)).to(cv.device); d_off = torch.arange(n, dtype=torch.int64, device=cv.device) * (4 + reclen)
d_pos = torch.from_numpy(sp.astype(np.int32)).to(cv.device); codes1 = snv_allele_codes(["A"] * len(sp)); d_ref = torch.from_numpy(codes1).to(cv.device); d_alt = torch.from_numpy(snv_allele_codes(["C"] * len(sp))).to(cv.device)
cv.use_torch_stream()
rc, ac, info = cv.snv_count(d_rec, d_off, 0, d_pos, d_ref, d_alt)
ms = []
for i in range(max(5, a.runs)):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record(); cv.snv_count(d_rec, d_off, 0, d_pos, d_ref, d_alt, rc, ac, want_info=False); e1.record(); torch.cuda.synchronize(); ms.append(e0.elapsed_time(e1))
med, mn = float(np.median(ms)), float(min(ms))
print(json.dumps({"section": "kernel_resident", "info": info.tolist(), "ms_median": round(med, 4), "ms_min": round(mn, 4), "record_GBps_median": round(len(stream) / med / 1e6, 1),
                  "records_per_s_median": round(n / med * 1e3), "fixed_field_fraction_of_record": round(24 / (4 + reclen), 3),
                  "note": "rate over ALL record bytes resident in HBM (the kernel requests 24 bytes of most records); compare with tools/bw_probe.py on the same box"}))
