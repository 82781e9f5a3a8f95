#!/usr/bin/env python3
"""What inflating a BAM's BGZF blocks costs on this box, on the device and on the host (not part of pytest or bench.py).  Writes a synthetic chromosome of paired
100-base reads as a BAM at zlib level 6 and, for chunks of --mb megabytes of records (default 32 and 128):
  kernel     canvas_bgzf_inflate on the chunk's blocks resident in HBM: milliseconds from the library's event pairs (canvas_profile_get), median of ten after a warm-up
  host       the same blocks through inflate_raw (canvas_amd/tools/bam_io.hpp) on the tools' own pool of 16 threads, straight into one buffer, as BamChunkLoop does:
             tools/probe_src/inflate_raw_host.cpp, compiled here with g++; wall clock, median of ten after a warm-up pass.  (The same blocks through Python's zlib in
             a thread pool are reported beside it and are NOT the comparator: the interpreter's share is a multiple of the inflation.)
  tools      CanvasSNV, CanvasBin -c and CanvasBin -m Fragment on the whole BAM with CANVAS_TOOL_TIMING=1, with and without CANVAS_TOOL_DEVICE_INFLATE=1: the inflate /
             device phases of the loop and the kernels' milliseconds, median of --runs processes after one warm-up process
One JSON line per section, on stdout and in --out (default profiles/inflate_probe.txt).  The comparison is device against host on the same blocks; no figure is a
share of any peak.
usage: tools/inflate_probe.py [--mb 32 --mb 128] [--runs 3] [--dir D] [--out FILE] [--no-tool]"""
import argparse, json, os, struct, subprocess, sys, time, zlib
from concurrent.futures import ThreadPoolExecutor
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--mb", type=float, action="append", default=[]); ap.add_argument("--runs", type=int, default=3); ap.add_argument("--dir", default="/tmp/inflate_probe")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate_probe.txt")); ap.add_argument("--seed", type=int, default=1); ap.add_argument("--no-tool", action="store_true")
ap.add_argument("--no-device", action="store_true", help="rehearsal without a GPU: the input and the host figures only")
a = ap.parse_args()
sizes = a.mb or [32, 128]
os.makedirs(a.dir, exist_ok=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
lines = []


def say(**kw):
    lines.append(json.dumps(kw)); print(lines[-1], flush=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


# ---- the input: pairs of 100-base reads, 300 bases from end to end, names of their own, sorted by position
L = 100; nlen = 11
reclen = 32 + nlen + 4 + (L + 1) // 2 + L
n = int(max(sizes) * 1e6 / (4 + reclen)) // 2 * 2
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
bases = code_of[ref[pos[:, None] + np.arange(L)]]                       # reads of the reference: the redundancy a real BAM's bases have
bases[rng.rand(n, L) < 0.002] = 8
recs[:, c0 + 4:c0 + 4 + L // 2] = (bases[:, 0::2] << 4) | bases[:, 1::2]
del bases
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
raw = open(bam, "rb").read()
say(section="input", reads=n, positions=span, record_bytes=len(stream), bam_bytes=len(raw), ratio=round(len(stream) / len(raw), 2), zlib_level=6, seconds_to_write=round(time.time() - t0, 1))
del body, stream

import canvas_amd
all_blocks, info = canvas_amd.bgzf_scan(raw, at=first)
assert info[3] == 1, info


helper = os.path.join(a.dir, "inflate_raw_host")
subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", os.path.join(ROOT, "tools", "probe_src", "inflate_raw_host.cpp"), "-lz", "-o", helper], check=True, timeout=120)


def host_inflate_raw(max_out):
    env = dict(os.environ, CANVAS_TOOL_THREADS=os.environ.get("CANVAS_TOOL_THREADS", "16"))
    r = subprocess.run([helper, bam, str(first), str(max_out), "10"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def host_inflate(blocks):
    def one(b):
        out = zlib.decompress(raw[int(b["src_offset"]):int(b["src_offset"]) + int(b["src_bytes"])], -15)
        assert len(out) == b["out_bytes"]
    ts = []
    with ThreadPoolExecutor(16) as ex:
        for i in range(11):
            t = time.perf_counter(); list(ex.map(one, blocks, chunksize=8)); ts.append(time.perf_counter() - t)
    return ts[1:]


if not a.no_device:
    import torch
    from canvas_amd import Canvas
    cv = Canvas(0)
    cv.profile_enable(True)
for mb in sizes:
    blocks, info = canvas_amd.bgzf_scan(raw, at=first, max_out_bytes=int(mb * 1e6))
    lo, hi = int(blocks[0]["src_offset"]), int(blocks[-1]["src_offset"] + blocks[-1]["src_bytes"])
    comp, out_bytes = hi - lo, int(info[2])
    ts = host_inflate(blocks)
    hr = host_inflate_raw(int(mb * 1e6))
    assert hr["blocks"] == len(blocks) and hr["inflated_bytes"] == out_bytes, hr
    row = dict(section="chunk", chunk_mb=mb, blocks=len(blocks), compressed_bytes=comp, inflated_bytes=out_bytes,
               inflate_raw_threads=hr["threads"], inflate_raw_ms_median=hr["ms_median"], inflate_raw_ms_min=hr["ms_min"], inflate_raw_GBps_inflated_median=round(out_bytes / hr["ms_median"] / 1e6, 2),
               python_zlib_pool_ms_median=round(float(np.median(ts)) * 1e3, 3))
    if not a.no_device:
        rel = blocks.copy(); rel["src_offset"] -= lo
        d_src = torch.from_numpy(np.frombuffer(raw, np.uint8)[lo:hi].copy()).to(cv.device)
        d_blk = torch.from_numpy(rel.view(np.uint8).reshape(-1).copy()).to(cv.device)
        d_out = torch.zeros(out_bytes, dtype=torch.uint8, device=cv.device); d_st = torch.zeros(len(blocks), dtype=torch.int32, device=cv.device)
        ms = []
        for i in range(11):
            cv.bgzf_inflate(d_src, d_blk, out=d_out, status=d_st, want_info=False)
            t, _ = cv.profile_get("bgzf_inflate")
            if i:
                ms.append(t)
        out, st, inf = cv.bgzf_inflate(d_src, d_blk, out=d_out, status=d_st)
        assert inf.tolist() == [len(blocks), 0, out_bytes, -1], inf
        k = len(blocks) // 2
        assert out[int(blocks[k]["dst_offset"]):int(blocks[k]["dst_offset"]) + int(blocks[k]["out_bytes"])].cpu().numpy().tobytes() == \
            zlib.decompress(raw[int(blocks[k]["src_offset"]):int(blocks[k]["src_offset"]) + int(blocks[k]["src_bytes"])], -15)
        med = float(np.median(ms))
        row.update(kernel_ms_median=round(med, 3), kernel_ms_min=round(min(ms), 3), kernel_GBps_inflated_median=round(out_bytes / med / 1e6, 2),
                   kernel_MBps_per_block_wave=round(out_bytes / med / 1e3 / min(len(blocks), 512), 1), inflate_raw_over_kernel=round(hr["ms_median"] / med, 2))
        del d_src, d_blk, d_out, d_st
    say(**row)

if not a.no_tool:                                             # (also without a device: tools/crc_probe.py takes its inputs from here)
    with open(fa, "wb") as f:
        f.write(b">chrP\n" + ref[:span].tobytes() + b"\n")
    with open(bed, "w") as f:
        f.write("".join("chrP\t%d\t%d\t45\n" % (s, s + 1000) for s in range(0, span - 1000, 1000)))
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.1\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\n")
        f.write("".join("chrP\t%d\t.\t%s\t%s\t50\tPASS\t.\tGT\t0/1\n" % (p + 1, chr(ref[p]), "ACGT"[("ACGT".index(chr(ref[p])) + 1) % 4]) for p in range(500, span, 1000)))
if not a.no_tool and not a.no_device:
    bindir = os.path.join(ROOT, "canvas_amd", "bin")
    tools = (("CanvasSNV", "[snv] ", [os.path.join(bindir, "CanvasSNV"), "-c", "chrP", "-v", vcf, "-b", bam, "-o", os.path.join(a.dir, "snv.txt.gz")]),
             ("CanvasBin -c", "[bam] ", [os.path.join(bindir, "CanvasBin"), "-b", bam, "-r", fa, "-c", "chrP", "-o", os.path.join(a.dir, "chrP.dat"), "-d", "100", "-m", "5", "-p"]),
             ("CanvasBin -m Fragment", "[frag] ", [os.path.join(bindir, "CanvasBin"), "-b", bam, "-r", fa, "-n", bed, "-o", os.path.join(a.dir, "out.binned"), "-m", "Fragment", "-p"]))
    for name, tag, cmd in tools:
        for device in (0, 1):
            env = dict(os.environ, CANVAS_TOOL_TIMING="1", CANVAS_TOOL_THREADS=os.environ.get("CANVAS_TOOL_THREADS", "16"))
            env.pop("CANVAS_TOOL_DEVICE_INFLATE", None)
            if device:
                env["CANVAS_TOOL_DEVICE_INFLATE"] = "1"
            rows = []
            for i in range(a.runs + 1):                       # the first process is the warm-up
                t = time.time()
                r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
                wall = time.time() - t
                assert r.returncode == 0, r.stderr[-2000:]
                tl = [json.loads(l[len(tag):]) for l in r.stderr.splitlines() if l.startswith(tag)]
                assert tl and tl[0]["device_inflate"] == device, r.stderr[-2000:]
                if i:
                    rows.append(dict(wall_s=wall, inflate_s=tl[0]["inflate_s"], device_wait_s=tl[0]["device_wait_s"], read_phase_s=tl[0]["inflate_s"] + tl[0]["device_wait_s"],
                                     kernel_ms=tl[0]["kernel_ms"], inflate_kernel_ms=tl[0]["inflate_kernel_ms"], _chunks=tl[0]["chunks"], _host_path=tl[0].get("host_path", 0)))
            keys = [k for k in rows[0] if not k.startswith("_")]
            say(section="tool", tool=name, device_inflate=device, runs=a.runs, chunks=rows[0]["_chunks"], host_path=rows[0]["_host_path"],
                median={k: round(float(np.median([r[k] for r in rows])), 4) for k in keys}, min={k: round(float(min(r[k] for r in rows)), 4) for k in keys})
