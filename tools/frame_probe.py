#!/usr/bin/env python3
"""What framing a BAM's records costs on this box, on the device and on the host (not part of pytest or bench.py).  Writes a synthetic chromosome of paired
100-base reads (--records, default 2 000 000) as a BAM at zlib level 6 and reports, for one chunk of --mb MiB of inflated records (default 32, the executables'
default chunk of 32 << 20 bytes):
  kernel     canvas_bam_frame on the chunk resident in HBM, for each kind: milliseconds from the library's event pairs (canvas_profile_get, scope "bam_frame"),
             median of ten after a warm-up, as built and with CANVAS_FRAME_NO_GUESS=1; the tiles walked twice (h_info[6]) on this real-looking data
  host       the loop of BamChunkLoop::run with the tool's `frame` callable restated (tools/probe_src/frame_walk_host.cpp, g++ -O2, one thread as in the tools) on
             the same bytes: wall clock, median of ten after a warm-up pass
  copy       the chunk copied from the device into pinned host memory: what the host framing of a device-inflated chunk pays first, and the device form removes
  tools      CanvasSNV, CanvasBin -c and CanvasBin -m Fragment on the whole BAM with CANVAS_TOOL_TIMING=1, with CANVAS_TOOL_DEVICE_INFLATE=1 alone and with
             CANVAS_TOOL_DEVICE_FRAME=1: the read phase (inflate + device wait) and the kernels' milliseconds, median of --runs processes after one warm-up process
One JSON line per section, on stdout and in --out (default profiles/frame_probe.txt).  The comparison is the device form against host walk plus copy on the same
bytes, and read phase against read phase; no figure is a share of any peak.
usage: tools/frame_probe.py [--records N] [--mb 32] [--runs 3] [--dir D] [--out FILE] [--no-tool]"""
import argparse, json, os, struct, subprocess, sys, time, zlib
from concurrent.futures import ThreadPoolExecutor
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--records", type=int, default=2_000_000); ap.add_argument("--mb", type=float, default=32); ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--dir", default="/tmp/frame_probe"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_probe.txt")); ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--no-tool", action="store_true")
a = ap.parse_args()
os.environ["CANVAS_TEST_HOOKS"] = "1"                         # (CANVAS_FRAME_NO_GUESS is a hook)
os.makedirs(a.dir, exist_ok=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
lines = []


def say(**kw):
    lines.append(json.dumps(kw)); print(lines[-1], flush=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


# ---- the input of tools/inflate_probe.py: pairs of 100-base reads, 300 bases from end to end, names of their own, sorted by position
L = 100; nlen = 11
reclen = 32 + nlen + 4 + (L + 1) // 2 + L
n = a.records // 2 * 2
span = max(1_000_000, n * 25)
rng = np.random.RandomState(a.seed)
t0 = time.time()
p1 = np.sort(rng.randint(0, span - 400, n // 2))
pos = np.concatenate([p1, p1 + 200]); mate = np.concatenate([p1 + 200, p1]); tlen = np.concatenate([np.full(n // 2, 300), np.full(n // 2, -300)])
flag = np.concatenate([np.full(n // 2, 0x63), np.full(n // 2, 0x93)]) | np.tile(np.where(rng.rand(n // 2) < 0.05, 0x400, 0), 2)
ident = np.tile(np.arange(n // 2), 2)
order = np.argsort(pos, kind="stable")
pos, mate, tlen, flag, ident = (x[order] for x in (pos, mate, tlen, flag, ident))
recs = np.zeros((n, 4 + reclen), np.uint8)
put32 = lambda col, v: recs.__setitem__((slice(None), slice(col, col + 4)), np.ascontiguousarray(v.astype("<i4")).view(np.uint8).reshape(n, 4))
recs[:, 0:4] = np.frombuffer(struct.pack("<i", reclen), np.uint8)
put32(8, pos); recs[:, 12] = nlen; recs[:, 13] = 60; recs[:, 16] = 1
recs[:, 18] = flag & 0xFF; recs[:, 19] = flag >> 8
recs[:, 20:24] = np.frombuffer(struct.pack("<i", L), np.uint8)
put32(28, mate); put32(32, tlen)
recs[:, 36:36 + nlen - 1] = (ident[:, None] // 10 ** np.arange(nlen - 2, -1, -1)) % 10 + 48
c0 = 36 + nlen
recs[:, c0:c0 + 4] = np.frombuffer(struct.pack("<I", L << 4), np.uint8)
ref = np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, span + L, dtype=np.uint8)]
code_of = np.zeros(256, np.uint8); code_of[list(b"ACGT")] = [1, 2, 4, 8]
for lo in range(0, n, 200_000):                                 # reads of the reference, in slices (the index array of all of them is gigabytes)
    bases = code_of[ref[pos[lo:lo + 200_000, None] + np.arange(L)]]
    recs[lo:lo + 200_000, c0 + 4:c0 + 4 + L // 2] = (bases[:, 0::2] << 4) | bases[:, 1::2]
recs[:, c0 + 4 + L // 2:] = np.array([12, 25, 25, 25, 25, 37, 37, 37, 37, 37, 37, 37, 37, 37, 37, 37], np.uint8)[rng.randint(0, 16, (n, L), dtype=np.uint8)]
stream = recs.tobytes(); del recs


def block(data):
    co = zlib.compressobj(6, zlib.DEFLATED, -15); c = co.compress(data) + co.flush()
    return struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(c) + 25) + c + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data))


text = b"@HD\tVN:1.0\tSO:coordinate\n"
hdr = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", 1) + struct.pack("<i", 5) + b"chrP\x00" + struct.pack("<i", span)
with ThreadPoolExecutor(16) as ex:
    body = list(ex.map(block, [stream[i:i + 65280] for i in range(0, len(stream), 65280)]))
bam = os.path.join(a.dir, "probe.bam"); fa = os.path.join(a.dir, "kmer.fa"); bed = os.path.join(a.dir, "bins.bed"); vcf = os.path.join(a.dir, "sites.vcf")
with open(bam, "wb") as f:
    f.write(block(hdr)); first = f.tell()
    f.write(b"".join(body)); end = f.tell(); f.write(block(b""))
open(bam + ".bai", "wb").write(b"BAI\x01" + struct.pack("<i", 1) + struct.pack("<i", 1) + struct.pack("<Ii", 0, 1) + struct.pack("<QQ", first << 16, end << 16) + struct.pack("<i", 0))
say(section="input", reads=n, positions=span, record_bytes=len(stream), bam_bytes=os.path.getsize(bam), zlib_level=6, seconds_to_write=round(time.time() - t0, 1))
del body

# ---- one chunk: the first --mb megabytes of the record stream, cut where the tools' loop cuts (anywhere: the last record is incomplete)
chunk = stream[:int(a.mb * (1 << 20))]
del stream
chunk_file = os.path.join(a.dir, "chunk.bin")
open(chunk_file, "wb").write(chunk)
helper = os.path.join(a.dir, "frame_walk_host")
subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "probe_src", "frame_walk_host.cpp"), "-lz", "-o", helper], check=True, timeout=120)

import torch
from canvas_amd import Canvas
from canvas_amd import lib as CL
cv = Canvas(0)
cv.profile_enable(True)
d_chunk = torch.from_numpy(np.frombuffer(chunk, np.uint8).copy()).to(cv.device)
pinned = torch.empty(len(chunk), dtype=torch.uint8).pin_memory()
ts = []
for i in range(11):
    torch.cuda.synchronize(); t = time.perf_counter(); pinned.copy_(d_chunk); torch.cuda.synchronize(); ts.append((time.perf_counter() - t) * 1e3)
copy_ms = float(np.median(ts[1:]))
say(section="copy", chunk_bytes=len(chunk), d2h_pinned_ms_median=round(copy_ms, 3), d2h_pinned_ms_min=round(min(ts[1:]), 3), GBps_median=round(len(chunk) / copy_ms / 1e6, 2))
d_off = torch.empty(len(chunk) // 36 + 2, dtype=torch.int64, device=cv.device)
for name, kind, sorted_ in (("snv", CL.BAM_FRAME_SNV, 0), ("hits", CL.BAM_FRAME_HITS, 1), ("fragments", CL.BAM_FRAME_FRAGMENTS, 0)):
    host = json.loads(subprocess.run([helper, chunk_file, str(kind), "0", str(sorted_), "10"], capture_output=True, text=True, check=True, timeout=300).stdout)
    row = dict(section="chunk", kind=name, chunk_bytes=len(chunk), records=host["records"], taken=host["taken"], host_walk_ms_median=host["ms_median"], host_walk_ms_min=host["ms_min"],
               host_walk_plus_copy_ms=round(host["ms_median"] + copy_ms, 3))
    for hook in (0, 1):
        os.environ.pop("CANVAS_FRAME_NO_GUESS", None)
        if hook:
            os.environ["CANVAS_FRAME_NO_GUESS"] = "1"
        ms = []
        for i in range(11):
            offs, info = cv.bam_frame(d_chunk, 0, (kind, 0, 1, sorted_), offsets=d_off)
            t, _ = cv.profile_get("bam_frame")
            if i:
                ms.append(t)
        assert [int(info[0]), int(info[1]), int(info[2]), int(info[3])] == [host["records"], host["taken"], host["used"], host["event"]], (info, host)
        assert host["taken"] == 0 or int(offs[-1]) == host["checksum"]
        key = "no_guess_" if hook else ""
        row.update({key + "kernel_ms_median": round(float(np.median(ms)), 3), key + "kernel_ms_min": round(min(ms), 3), key + "tiles_walked_twice": int(info[6])})
    os.environ.pop("CANVAS_FRAME_NO_GUESS", None)
    row.update(tiles=len(chunk) // int(info[7]) + 1, host_walk_plus_copy_over_kernel=round((host["ms_median"] + copy_ms) / row["kernel_ms_median"], 2))
    say(**row)
del d_chunk, d_off, pinned

if not a.no_tool:
    with open(fa, "wb") as f:
        f.write(b">chrP\n" + ref[:span].tobytes() + b"\n")
    with open(bed, "w") as f:
        f.write("".join("chrP\t%d\t%d\t45\n" % (s, s + 1000) for s in range(0, span - 1000, 1000)))
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.1\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\n")
        f.write("".join("chrP\t%d\t.\t%s\t%s\t50\tPASS\t.\tGT\t0/1\n" % (p + 1, chr(ref[p]), "ACGT"[("ACGT".index(chr(ref[p])) + 1) % 4]) for p in range(500, span, 1000)))
    bindir = os.path.join(ROOT, "canvas_amd", "bin")
    tools = (("CanvasSNV", "[snv] ", [os.path.join(bindir, "CanvasSNV"), "-c", "chrP", "-v", vcf, "-b", bam, "-o", os.path.join(a.dir, "snv.txt.gz")]),
             ("CanvasBin -c", "[bam] ", [os.path.join(bindir, "CanvasBin"), "-b", bam, "-r", fa, "-c", "chrP", "-o", os.path.join(a.dir, "chrP.dat"), "-d", "100", "-m", "5", "-p"]),
             ("CanvasBin -m Fragment", "[frag] ", [os.path.join(bindir, "CanvasBin"), "-b", bam, "-r", fa, "-n", bed, "-o", os.path.join(a.dir, "out.binned"), "-m", "Fragment", "-p"]))
    for name, tag, cmd in tools:
        for var in ("CANVAS_TOOL_DEVICE_INFLATE", "CANVAS_TOOL_DEVICE_FRAME"):
            env = dict(os.environ, CANVAS_TOOL_TIMING="1", CANVAS_TOOL_THREADS=os.environ.get("CANVAS_TOOL_THREADS", "16"))
            for v in ("CANVAS_TOOL_DEVICE_INFLATE", "CANVAS_TOOL_DEVICE_FRAME", "CANVAS_TEST_HOOKS"):
                env.pop(v, None)
            env[var] = "1"
            rows = []
            for i in range(a.runs + 1):                       # the first process is the warm-up
                t = time.time()
                r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
                wall = time.time() - t
                assert r.returncode == 0, r.stderr[-2000:]
                tl = [json.loads(l[len(tag):]) for l in r.stderr.splitlines() if l.startswith(tag)]
                assert tl and tl[0]["device_inflate"] == 1 and tl[0]["device_frame"] == (var == "CANVAS_TOOL_DEVICE_FRAME"), r.stderr[-2000:]
                if i:
                    rows.append(dict(wall_s=wall, inflate_s=tl[0]["inflate_s"], device_wait_s=tl[0]["device_wait_s"], read_phase_s=tl[0]["inflate_s"] + tl[0]["device_wait_s"],
                                     kernel_ms=tl[0]["kernel_ms"], inflate_kernel_ms=tl[0]["inflate_kernel_ms"], frame_kernel_ms=tl[0]["frame_kernel_ms"], _chunks=tl[0]["chunks"],
                                     _host_path=tl[0].get("host_path", 0)))
            keys = [k for k in rows[0] if not k.startswith("_")]
            say(section="tool", tool=name, variable=var, runs=a.runs, chunks=rows[0]["_chunks"], host_path=rows[0]["_host_path"],
                median={k: round(float(np.median([r[k] for r in rows])), 4) for k in keys}, min={k: round(float(min(r[k] for r in rows)), 4) for k in keys})
