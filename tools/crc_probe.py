#!/usr/bin/env python3
"""What checking the CRC32 of a BAM's BGZF blocks costs on this box, on the device and on the host (not part of pytest or bench.py).  The input is the BAM
tools/inflate_probe.py writes (it is run here with --no-device for its files: paired 100-base reads at zlib level 6, --file-mb megabytes of records, four of the tools'
chunks by default), and on one chunk of --mb megabytes of records:
  kernel     canvas_bgzf_crc32 on the chunk that canvas_bgzf_inflate has just left in HBM, and canvas_bgzf_inflate itself: milliseconds from the library's event
             pairs (canvas_profile_get), median of ten after a warm-up.  "warm": the same 32 MB every time, which the last call left in the caches, as the inflater
             leaves them for the check in the tools.  "cold": twelve copies of the chunk in turn (384 MB, more than the 256 MiB of Infinity Cache), every call on
             the copy touched longest ago.
  host       zlib's crc32() over the same inflated bytes on 16 threads, each with a sixteenth of the blocks (Python's zlib releases the interpreter lock for
             buffers of this size; the interpreter's loop around the calls is part of the figure); wall clock, median of ten after a warm-up
  hbm        the streaming-read figure of tools/bw_probe.py in the same job
  tools      CanvasSNV, CanvasBin -c and CanvasBin -m Fragment on the whole BAM with CANVAS_TOOL_TIMING=1, with and without CANVAS_TOOL_CHECK_CRC=1, on the host path,
             with CANVAS_TOOL_DEVICE_INFLATE=1 and with CANVAS_TOOL_DEVICE_FRAME=1: the read phase (inflate + device wait of the loop) and the kernels'
             milliseconds, median of --runs processes after one warm-up process
One JSON line per section, on stdout and in --out (default profiles/crc_probe.txt).
usage: tools/crc_probe.py [--mb 32] [--file-mb 128] [--runs 3] [--dir D] [--out FILE] [--no-tool]"""
import argparse, json, os, struct, subprocess, sys, time, zlib
from concurrent.futures import ThreadPoolExecutor
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--mb", type=float, default=32); ap.add_argument("--file-mb", type=float, default=128); ap.add_argument("--runs", type=int, default=3); ap.add_argument("--dir", default="/tmp/crc_probe")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crc_probe.txt")); ap.add_argument("--no-tool", action="store_true")
a = ap.parse_args()
os.makedirs(a.dir, exist_ok=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
lines = []


def say(**kw):
    lines.append(json.dumps(kw)); print(lines[-1], flush=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


# ---- the input: inflate_probe's files (probe.bam + .bai, kmer.fa, bins.bed, sites.vcf)
r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "inflate_probe.py"), "--no-device", "--mb", str(a.mb), "--mb", str(a.file_mb), "--dir", a.dir, "--out", os.path.join(a.dir, "inflate_probe_inputs.txt")],
                   capture_output=True, text=True, timeout=600)
assert r.returncode == 0, r.stderr[-2000:]
bam = os.path.join(a.dir, "probe.bam"); fa = os.path.join(a.dir, "kmer.fa"); bed = os.path.join(a.dir, "bins.bed"); vcf = os.path.join(a.dir, "sites.vcf")
raw = open(bam, "rb").read()
first = struct.unpack_from("<H", raw, 16)[0] + 1                            # behind the header's block

import canvas_amd
import torch
from canvas_amd import Canvas
from canvas_amd.lib import CRC_OK
blocks, info = canvas_amd.bgzf_scan(raw, at=first, max_out_bytes=int(a.mb * 1e6))
lo, hi = int(blocks[0]["src_offset"]), int(blocks[-1]["src_offset"] + blocks[-1]["src_bytes"]) + 8      # with the last trailer
out_bytes, nb = int(info[2]), len(blocks)
cv = Canvas(0)
cv.profile_enable(True)
rel = blocks.copy(); rel["src_offset"] -= lo
d_src = torch.from_numpy(np.frombuffer(raw, np.uint8)[lo:hi].copy()).to(cv.device)
d_blk = torch.from_numpy(rel.view(np.uint8).reshape(-1).copy()).to(cv.device)
d_out = torch.zeros(out_bytes, dtype=torch.uint8, device=cv.device); d_st = torch.zeros(nb, dtype=torch.int32, device=cv.device)
d_crc = torch.zeros(nb, dtype=torch.int32, device=cv.device); d_cst = torch.zeros(nb, dtype=torch.int32, device=cv.device)


def timed(scope, call, n=10):
    ms = []
    for i in range(n + 1):                                    # the first call is the warm-up
        call(i)
        cv.synchronize()
        t, _ = cv.profile_get(scope)
        if i:
            ms.append(t)
    return round(float(np.median(ms)), 4), round(min(ms), 4)


inflate_ms = timed("bgzf_inflate", lambda i: cv.bgzf_inflate(d_src, d_blk, out=d_out, status=d_st, want_info=False))
out, st, inf = cv.bgzf_inflate(d_src, d_blk, out=d_out, status=d_st)
assert inf.tolist() == [nb, 0, out_bytes, -1], inf
crc_warm = timed("bgzf_crc32", lambda i: cv.bgzf_crc32(d_src, d_blk, d_out, inflate_status=d_st, crc=d_crc, status=d_cst, want_info=False))
pair = timed("bgzf_crc32", lambda i: (cv.bgzf_inflate(d_src, d_blk, out=d_out, status=d_st, want_info=False),
                                      cv.bgzf_crc32(d_src, d_blk, d_out, inflate_status=d_st, crc=d_crc, status=d_cst, want_info=False)))
copies = [d_out.clone() for _ in range(12)]
crc_cold = timed("bgzf_crc32", lambda i: cv.bgzf_crc32(d_src, d_blk, copies[i % 12], inflate_status=d_st, crc=d_crc, status=d_cst, want_info=False), n=24)
crc, cst, cinf = cv.bgzf_crc32(d_src, d_blk, d_out, inflate_status=d_st, crc=d_crc, status=d_cst)
assert cinf.tolist() == [nb, 0, out_bytes, -1] and (cst.cpu().numpy() == CRC_OK).all(), cinf
host_bytes = out.cpu().numpy()
got = crc.cpu().numpy().view(np.uint32)
view = memoryview(host_bytes)
spans = [(int(b["dst_offset"]), int(b["dst_offset"]) + int(b["out_bytes"])) for b in blocks]
assert all(zlib.crc32(view[s:e]) == int(g) for (s, e), g in zip(spans, got))
del copies


def host_crc(part):
    return [zlib.crc32(view[s:e]) for s, e in part]


parts = [spans[k::16] for k in range(16)]
ts = []
with ThreadPoolExecutor(16) as ex:
    for i in range(11):
        t = time.perf_counter(); list(ex.map(host_crc, parts)); ts.append((time.perf_counter() - t) * 1e3)
t = time.perf_counter(); host_crc(spans); one_thread_ms = (time.perf_counter() - t) * 1e3
bw = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bw_probe.py")], capture_output=True, text=True, timeout=300)
hbm = bw.stdout.splitlines()[0] if bw.returncode == 0 and bw.stdout else "bw_probe failed: " + bw.stderr[-200:]
per_block = out_bytes / nb
say(section="chunk", chunk_mb=a.mb, blocks=nb, inflated_bytes=out_bytes, bytes_in_per_block=round(per_block + 24 + 4 + 4, 1), bytes_out_per_block=8,
    inflate_kernel_ms_median=inflate_ms[0], inflate_kernel_ms_min=inflate_ms[1],
    crc_kernel_warm_ms_median=crc_warm[0], crc_kernel_warm_ms_min=crc_warm[1], crc_kernel_behind_inflate_ms_median=pair[0], crc_kernel_behind_inflate_ms_min=pair[1],
    crc_kernel_cold_ms_median=crc_cold[0], crc_kernel_cold_ms_min=crc_cold[1],
    crc_warm_GBps=round(out_bytes / crc_warm[0] / 1e6, 1), crc_cold_GBps=round(out_bytes / crc_cold[0] / 1e6, 1), crc_over_inflate=round(pair[0] / inflate_ms[0], 4),
    host_zlib_crc32_16_threads_ms_median=round(float(np.median(ts[1:])), 3), host_zlib_crc32_16_threads_ms_min=round(min(ts[1:]), 3), host_zlib_crc32_1_thread_ms=round(one_thread_ms, 3),
    hbm_bw_probe=hbm)
del d_src, d_blk, d_out, d_st, d_crc, d_cst, out, crc

if not a.no_tool:
    bindir = os.path.join(ROOT, "canvas_amd", "bin")
    tools = (("CanvasSNV", "[snv] ", [os.path.join(bindir, "CanvasSNV"), "-c", "chrP", "-v", vcf, "-b", bam, "-o", os.path.join(a.dir, "snv.txt.gz")]),
             ("CanvasBin -c", "[bam] ", [os.path.join(bindir, "CanvasBin"), "-b", bam, "-r", fa, "-c", "chrP", "-o", os.path.join(a.dir, "chrP.dat"), "-d", "100", "-m", "5", "-p"]),
             ("CanvasBin -m Fragment", "[frag] ", [os.path.join(bindir, "CanvasBin"), "-b", bam, "-r", fa, "-n", bed, "-o", os.path.join(a.dir, "out.binned"), "-m", "Fragment", "-p"]))
    for name, tag, cmd in tools:
        for path in ("host", "CANVAS_TOOL_DEVICE_INFLATE", "CANVAS_TOOL_DEVICE_FRAME"):
            for check in (0, 1):
                env = dict(os.environ, CANVAS_TOOL_TIMING="1", CANVAS_TOOL_THREADS=os.environ.get("CANVAS_TOOL_THREADS", "16"))
                for v in ("CANVAS_TOOL_DEVICE_INFLATE", "CANVAS_TOOL_DEVICE_FRAME", "CANVAS_TOOL_CHECK_CRC"):
                    env.pop(v, None)
                if path != "host":
                    env[path] = "1"
                if check:
                    env["CANVAS_TOOL_CHECK_CRC"] = "1"
                rows = []
                for i in range(a.runs + 1):                       # the first process is the warm-up
                    t = time.time()
                    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
                    wall = time.time() - t
                    assert r.returncode == 0, r.stderr[-2000:]
                    tl = [json.loads(l[len(tag):]) for l in r.stderr.splitlines() if l.startswith(tag)]
                    assert tl and tl[0]["check_crc"] == check and tl[0]["device_inflate"] == (path != "host"), r.stderr[-2000:]
                    if i:
                        rows.append(dict(wall_s=wall, read_phase_s=tl[0]["inflate_s"] + tl[0]["device_wait_s"], inflate_kernel_ms=tl[0]["inflate_kernel_ms"],
                                         crc_kernel_ms=tl[0]["crc_kernel_ms"], _chunks=tl[0]["chunks"], _host_path=tl[0].get("host_path", 0)))
                keys = [k for k in rows[0] if not k.startswith("_")]
                say(section="tool", tool=name, path=path, check_crc=check, runs=a.runs, chunks=rows[0]["_chunks"], host_path=rows[0]["_host_path"],
                    median={k: round(float(np.median([r[k] for r in rows])), 4) for k in keys}, min={k: round(float(min(r[k] for r in rows)), 4) for k in keys})
