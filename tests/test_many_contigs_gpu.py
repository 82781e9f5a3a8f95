"""Every stage on references shaped like a production one — a few primary chromosomes and hundreds to thousands of small contigs (tests/many_contigs.py) — against
the oracle, at both sides of each chromosome-count threshold where the product changes code path:

  64    BIN_BYVAL (bin.hip), HMM_BYVAL (hmm.hip), WV_F3_MAXCHR (wavelets.hip): per-chromosome tables by value / uploaded, factor-of-three statistics on the host
  256   CfArgsPack::isAuto, sAuto[256] (clean_fast.hpp, clean_gc_only.hpp): autosome flags past index 255 come from the table; the -g-only launches decline
  1024  CF_MAXRUN (clean_fast.hpp): device-driven Clean hands back to the host-driven path; WV_MED_MAXR (wavelets.hip): one workgroup per chromosome median

Bin and Clean check once that their oracle result depends on the flags of the non-autosomes past index 255, so that a wrong flag there cannot pass unnoticed.
Also: CBS on 2 000 tiny contigs under a cache bound, the sharded pipeline on two ranks, and the executables on GRCh38-style names."""
import os
import subprocess
import sys

import numpy as np
import pytest

import many_contigs as M
import oracle_flows as F
import oracle_lib as O
from canvas_amd import CLEAN_GCNORM, CLEAN_FILTSIZE, CLEAN_OUTLIERS, CLEAN_LOCALSD
from gpu_common import get_canvas, to_dev, pad16

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = CLEAN_GCNORM | CLEAN_FILTSIZE | CLEAN_OUTLIERS | CLEAN_LOCALSD


def _out(cv, cap):
    import torch
    mk = lambda dt: torch.empty(cap, dtype=dt, device=cv.device)
    return dict(chr=mk(torch.int32), start=mk(torch.int32), stop=mk(torch.int32), gc=mk(torch.int32), count=mk(torch.float32))


def _expected_bins(exp):
    """per-chromosome oracle bins [start, stop, gc, count] -> the concatenated arrays with chromosome ids, and bins per chromosome"""
    per = np.array([len(e[0]) for e in exp], np.int64)
    cat = lambda j: np.concatenate([e[j] for e in exp]) if len(exp) else np.zeros(0, np.int32)
    return dict(chr=np.repeat(np.arange(len(exp), dtype=np.int32), per), start=cat(0), stop=cat(1), gc=cat(2), count=cat(3).astype(np.float32)), per


def _check_bins(out, per, total, exp, what):
    e, eper = _expected_bins(exp)
    assert total == len(e["chr"]), (what, total, len(e["chr"]))
    assert per is None or np.asarray(per).tolist() == eper.tolist(), (what, np.nonzero(np.asarray(per) != eper)[0][:8])
    for k in ("chr", "start", "stop", "gc"):
        got = out[k][:total].cpu().numpy()
        assert (got == e[k]).all(), (what, k, np.nonzero(got != e[k])[0][:8])
    got = out["count"][:total].cpu().numpy()
    assert (got.view(np.uint32) == e["count"].view(np.uint32)).all(), (what, np.nonzero(got != e["count"])[0][:8])


# ------------------------------------------------------------------------------------------------------------------------------------------------ Bin
@pytest.mark.parametrize("nchr", [63, 64, 65, 3000])
def test_bin_many_contigs_matches_oracle(nchr):
    import torch
    cv = get_canvas()
    data0, is_auto = M.genome(nchr)
    rates0 = O.bin_rates_genome([d[2] for d in data0], [d[1] for d in data0], threads=8)
    bs0 = O.bin_size(rates0[is_auto == 1], 100)
    data, is_auto = M.genome(nchr, bin_size=bs0)               # + contigs of bs - 1, bs, bs + 1 possible positions (non-autosomes: the bin size stays)
    bases_h = [d[0] for d in data]; hits_h = [d[1] for d in data]; masks_h = [d[2] for d in data]
    lens = np.array([len(b) for b in bases_h], np.int64)
    rates = O.bin_rates_genome(masks_h, hits_h, threads=8)
    bs = O.bin_size(rates[is_auto == 1], 100)
    assert bs == bs0
    if nchr > 1024:
        assert O.bin_size(rates[M.flipped(is_auto) == 1], 100) != bs          # the flags past index 255 decide the bin size
    exp = [O.bin_chromosome(b, m, h, bs, 3) for b, h, m in data]
    assert [len(exp[c][0]) for c in range(len(M.PRIMARY) + len(M.EDGE_LENGTHS), len(M.PRIMARY) + len(M.EDGE_LENGTHS) + 3)] == [0, 1, 1]
    db = [to_dev(pad16(b), cv.device) for b in bases_h]; dh = [to_dev(pad16(h), cv.device) for h in hits_h]; dm = [to_dev(m.view(np.int64), cv.device) for m in masks_h]
    obs, poss, grate = cv.bin_rates(dh, dm, lens)
    assert (grate.view(np.uint64) == rates.view(np.uint64)).all(), np.nonzero(grate != rates)[0][:8]
    assert cv.bin_size_from_rates(grate[is_auto == 1], 100) == bs
    cap = int(lens.sum() // 50) + 64
    out = _out(cv, cap)
    o, per, total = cv.bin_genome(db, dm, dh, lens, bs, 3, out=out)
    _check_bins(out, per, total, exp, "bin_genome")
    o, per, total, gbs = cv.bin_sample(db, dm, dh, lens, is_auto, 100, -1, 3, out=out)
    assert gbs == bs
    _check_bins(out, per, total, exp, "bin_sample")
    dref, dpl, pos0, _ = cv.pack_genome_device(db, dm, dh, lens)
    assert (pos0 == np.array([int(np.argmax(b != ord('n'))) if (b != ord('n')).any() else len(b) for b in bases_h])).all()
    o, per, total, gbs = cv.bin_sample_packed(dref, dpl, lens, pos0, is_auto, 100, -1, 3, out=out)
    assert gbs == bs
    _check_bins(out, per, total, exp, "bin_sample_packed")
    # streamed uploads: the per-chromosome sweeps start as the chromosomes arrive (reference uploaded too / already resident)
    pin = lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory()
    hb = [pin(pad16(b)) for b in bases_h]; hh = [pin(pad16(h)) for h in hits_h]; hm = [pin(m.view(np.int64)) for m in masks_h]
    for resident in (False, True):
        db2 = [t.clone() for t in db] if resident else [torch.zeros_like(t) for t in db]
        dm2 = [t.clone() for t in dm] if resident else [torch.zeros_like(t) for t in dm]
        dh2 = [torch.zeros_like(t) for t in dh]
        torch.cuda.synchronize()
        cv.upload_genome_begin(lens, None if resident else hb, db2, None if resident else hm, dm2, hh, dh2)
        o, per, total, gbs = cv.bin_sample(db2, dm2, dh2, lens, is_auto, 100, -1, 3, out=out)
        assert gbs == bs
        _check_bins(out, per, total, exp, ("upload_genome_begin", resident))
    cv.upload_genome_wait()
    href = [t.cpu().pin_memory() for t in dref]; hpl = [t.cpu().pin_memory() for t in dpl]
    dref3 = [torch.zeros_like(t) for t in dref]; dpl3 = [torch.zeros_like(t) for t in dpl]
    torch.cuda.synchronize()
    cv.upload_packed_begin(lens, href, dref3, hpl, dpl3)
    o, per, total, gbs = cv.bin_sample_packed(dref3, dpl3, lens, pos0, is_auto, 100, -1, 3, out=out)
    assert gbs == bs
    _check_bins(out, per, total, exp, "upload_packed_begin")
    cv.upload_genome_wait()
    # the hit planes in their two-bit wire form (pack_hits2_host), expanded on the device behind each chromosome's transfer; reference already resident
    from canvas_amd.lib import pack_hits2_host
    pin64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).pin_memory()
    parts = [pack_hits2_host(np.ascontiguousarray(h), len(h)) for h in hits_h]
    dpl4 = [torch.zeros_like(t) for t in dpl]
    torch.cuda.synchronize()
    cv.upload_packed2_begin(lens, None, dref3, [pin64(q[0]) for q in parts], [pin64(q[1]) for q in parts], [pin64(q[2]) for q in parts], [q[3] for q in parts], dpl4)
    o, per, total, gbs = cv.bin_sample_packed(dref3, dpl4, lens, pos0, is_auto, 100, -1, 3, out=out)
    assert gbs == bs
    _check_bins(out, per, total, exp, "upload_packed2_begin")
    cv.upload_genome_wait()
    # GCContentWeighted: the profile and the weights from every chromosome
    rng = np.random.RandomState(nchr)
    fl = [np.where(h > 0, np.clip(rng.normal(330, 60, len(h)), 1, 5000), 0).astype(np.int16) for h in hits_h]
    gexp, _, _, _ = O.bin_gc_weighted(bases_h, masks_h, hits_h, fl, bs)
    dfl = [to_dev(pad16(f), cv.device) for f in fl]
    o, per, total, gbs = cv.bin_sample_gcweighted(db, dm, dh, dfl, lens, is_auto, 100, -1, out=out)
    assert gbs == bs
    _check_bins(out, per, total, gexp, "bin_sample_gcweighted")
    # predefined bins (-n): two per chromosome whose first half holds a base other than 'n', none otherwise (a first bin entirely in leading 'n' bases is refused)
    has = [L >= 2 and p < L // 2 for L, p in zip(lens, pos0)]
    starts = [np.array([0, L // 2], np.int32) if k else np.zeros(0, np.int32) for L, k in zip(lens, has)]
    stops = [np.array([L // 2, L], np.int32) if k else np.zeros(0, np.int32) for L, k in zip(lens, has)]
    gc, cnt = cv.bin_predefined(db, dm, dh, lens, starts, stops, mode=3)
    eg = []; ec = []
    for c, (b, h, m) in enumerate(data):
        k, g_, n_ = O.bin_predefined(b, m, h, starts[c], stops[c], 3)
        eg.append(g_); ec.append(n_)
    eg = np.concatenate(eg); ec = np.concatenate(ec).astype(np.float32)
    assert (gc.cpu().numpy() == eg).all() and (cnt.cpu().numpy() == ec).all()


# ------------------------------------------------------------------------------------------------------------------------------------------------ Clean
def _clean_case(cv, b, is_auto, flags, w, want_device=None):
    is_y = np.zeros(len(is_auto), np.uint8)
    ex = O.clean(b["chr"], b["start"], b["stop"], b["count"], b["gc"], is_auto, is_y, flags, min_bins_weighted=w)
    dev = {k: to_dev(v, cv.device) for k, v in b.items()}
    n_out, lsd, info = cv.clean(dev, len(b["chr"]), is_auto, flags, min_bins_per_gc=w)
    _same_clean(dev, n_out, lsd, ex, (flags, w))
    if want_device is not None:
        assert info[6] == 0 and info[7] == int(want_device), (info, want_device)
    return ex, info


def _same_clean(dev, n_out, lsd, ex, what):
    assert n_out == len(ex["chr"]), (what, n_out, len(ex["chr"]))
    for k in ("chr", "start", "stop", "gc"):
        assert (dev[k][:n_out].cpu().numpy() == ex[k]).all(), (what, k)
    got = dev["count"][:n_out].cpu().numpy()
    assert (got.view(np.uint32) == ex["count"].view(np.uint32)).all(), (what, np.nonzero(got != ex["count"])[0][:8])
    assert np.float64(lsd).view(np.uint64) == np.float64(ex["local_sd"]).view(np.uint64), what


@pytest.mark.parametrize("nchr", [256, 257, 3000])
def test_clean_many_contigs_matches_oracle(nchr):
    cv = get_canvas()
    b, is_auto = M.bins(nchr)
    b["count"] = np.round(b["count"]).astype(np.float32)
    if nchr > 1024:
        e1 = O.clean(b["chr"], b["start"], b["stop"], b["count"], b["gc"], is_auto, np.zeros(nchr, np.uint8), ALL)
        e2 = O.clean(b["chr"], b["start"], b["stop"], b["count"], b["gc"], M.flipped(is_auto), np.zeros(nchr, np.uint8), ALL)
        assert len(e1["chr"]) != len(e2["chr"]) or not (e1["count"].view(np.uint32) == e2["count"].view(np.uint32)).all()
    runs = int((np.bincount(b["chr"], minlength=nchr) > 0).sum())
    for flags in (ALL, CLEAN_GCNORM):
        _, info = _clean_case(cv, b, is_auto, flags, 100)
        if flags == ALL:
            assert info[6] == 0 and info[7] == int(runs <= 1024), (info, runs)
        else:
            assert info[6] == int(nchr <= 256), info                    # the -g-only launches keep 256 flags: past that they decline
    _clean_case(cv, b, is_auto, ALL, 20, want_device=False)             # -w < 100: the weighted-median branch (host-driven)


@pytest.mark.parametrize("nchr", [1024, 1025])
def test_clean_contiguous_chromosome_runs_at_the_device_limit(nchr):
    """with the local-SD filter on 50 000 bins or more, 1 024 contiguous chromosome runs are sorted on the device and 1 025 are handed back to the host-driven path
    (without it the runs are not needed: the device-driven chain takes both) — every case gives the oracle's bits"""
    cv = get_canvas()
    per = np.maximum(M.bin_counts_per_contig(nchr), 12)         # every chromosome keeps bins through the filters: nchr runs reach the local-SD filter
    per[:len(M.PRIMARY)] = [40_000, 20_000, 10_000]
    b, is_auto = M.bins(nchr, per=per)
    b["count"] = np.round(b["count"]).astype(np.float32)
    _, info = _clean_case(cv, b, is_auto, ALL, 100, want_device=nchr <= 1024)
    assert info[1] >= 50_000
    _clean_case(cv, b, is_auto, CLEAN_FILTSIZE | CLEAN_OUTLIERS, 100, want_device=True)


def test_clean_batch_many_contigs_matches_oracle():
    """a cohort of six (more than CF_BYVAL = 4 argument blocks: uploaded) at 257 and 3 000 chromosomes; at 3 000 every sample has more than 1 024 runs and is
    handed back to the host-driven path"""
    cv = get_canvas()
    for nchr in (257, 3000):
        samples, exps, ns = [], [], []
        for s in range(6):
            b, is_auto = M.bins(nchr, seed=M.SEED + 100 * s)
            b["count"] = np.round(b["count"]).astype(np.float32)
            exps.append(O.clean(b["chr"], b["start"], b["stop"], b["count"], b["gc"], is_auto, np.zeros(nchr, np.uint8), ALL))
            samples.append({k: to_dev(v, cv.device) for k, v in b.items()}); ns.append(len(b["chr"]))
        nout, lsd, info = cv.clean_batch(samples, ns, is_auto, ALL)
        for s, ex in enumerate(exps):
            _same_clean(samples[s], int(nout[s]), lsd[s], ex, (nchr, s))
            assert info[s][6] == 0 and info[s][7] == int(nchr <= 1024), (nchr, s, info[s])


# ------------------------------------------------------------------------------------------------------------------------------------------------ PerSampleHMM
@pytest.mark.parametrize("nchr", [63, 64, 65, 1000])
def test_hmm_and_segments_many_contigs_match_oracle(nchr):
    cv = get_canvas()
    b, _ = M.bins(nchr)
    cov = np.round(b["count"].astype(np.float64), 2)
    off = M.offsets(b["chr"], nchr)
    per = [np.ascontiguousarray(cov[off[c]:off[c + 1]]) for c in range(nchr)]
    paths, ran = O.hmm_genome_per_sample(per, threads=8)
    state = cv.hmm_per_sample(to_dev(cov, cv.device), off)
    got = state.cpu().numpy()
    exp = np.concatenate([paths[c] if ran[c] else np.full(len(per[c]), -1, np.int32) for c in range(nchr)])
    assert (got == exp).all(), np.nonzero(got != exp)[0][:8]
    bs = [b["start"][off[c]:off[c + 1]].astype(np.uint32) for c in range(nchr)]
    be = [b["stop"][off[c]:off[c + 1]].astype(np.uint32) for c in range(nchr)]
    starts = [O.segments_from_path(paths[c], ran[c], bs[c], be[c])[0] for c in range(nchr)]
    excl = []
    for c in range(nchr):                        # a forbidden interval over the middle bin of every third chromosome that has bins
        k = len(bs[c])
        excl.append((np.array([bs[c][k // 2]], np.int32), np.array([be[c][k // 2]], np.int32)) if k and c % 3 == 0 else (np.zeros(0, np.int32), np.zeros(0, np.int32)))
    for ex in (None, excl):
        ids, last = O.postprocess(bs, be, starts, ex)
        seg, nseg = cv.segment_ids(off, state, to_dev(b["start"], cv.device), to_dev(b["stop"], cv.device), excluded=ex)
        assert (seg.cpu().numpy() == np.concatenate(ids)).all() and nseg == last + 1


def _oracle_pipeline(data, is_auto):
    """the oracle's chain behind canvas_sample_pipeline: rates -> bin size -> bins -> CanvasClean (-g -s -r, local SD) -> F2 -> PerSampleHMM -> segment ids"""
    nchr = len(data)
    bases_h = [d[0] for d in data]; hits_h = [d[1] for d in data]; masks_h = [d[2] for d in data]
    rates = O.bin_rates_genome(masks_h, hits_h, threads=8)
    bs = O.bin_size(rates[is_auto == 1], 100)
    st, en, gc, cnt = O.bin_genome(bases_h, masks_h, hits_h, bs, 3, threads=8)
    B = dict(chr=np.concatenate([np.full(len(st[c]), c, np.int32) for c in range(nchr)]), start=np.concatenate(st), stop=np.concatenate(en), gc=np.concatenate(gc),
             count=np.concatenate(cnt).astype(np.float32))
    ex = O.clean(B["chr"], B["start"], B["stop"], B["count"], B["gc"], is_auto, np.zeros(nchr, np.uint8), ALL)
    cov = F.f2_double(ex["count"])
    off = M.offsets(ex["chr"], nchr)
    per = [np.ascontiguousarray(cov[off[c]:off[c + 1]]) for c in range(nchr)]
    paths, ran = O.hmm_genome_per_sample(per, threads=8)
    bsr = [ex["start"][off[c]:off[c + 1]].astype(np.uint32) for c in range(nchr)]; ber = [ex["stop"][off[c]:off[c + 1]].astype(np.uint32) for c in range(nchr)]
    ids, last = O.postprocess(bsr, ber, [O.segments_from_path(paths[c], ran[c], bsr[c], ber[c])[0] for c in range(nchr)])
    state = np.concatenate([paths[c] if ran[c] else np.full(len(per[c]), -1, np.int32) for c in range(nchr)])
    return dict(bin_size=bs, total=len(B["chr"]), n_out=len(ex["chr"]), nseg=last + 1, off=off, cleaned=ex, cov=cov, state=state, seg=np.concatenate(ids))


def _check_pipeline(E, r, bins, cov, state, seg):
    """a pipeline's result (r: its returned dict; host arrays of its outputs) against _oracle_pipeline's"""
    n = E["n_out"]
    ex = E["cleaned"]
    assert (r["bin_size"], r["total"], r["n_out"], r["nseg"]) == (E["bin_size"], E["total"], n, E["nseg"])
    assert list(r["off"]) == E["off"].tolist()
    assert np.float64(r["lsd"]).view(np.uint64) == np.float64(ex["local_sd"]).view(np.uint64)
    for k in ("chr", "start", "stop", "gc"):
        assert (bins[k][:n] == ex[k]).all(), k
    assert (bins["count"][:n].view(np.uint32) == ex["count"].view(np.uint32)).all()
    assert (cov[:n].view(np.uint64) == E["cov"].view(np.uint64)).all()
    assert (state[:n] == E["state"]).all()
    assert (seg[:n] == E["seg"]).all()


def _pipeline_buffers(device, cap):
    import torch
    mk = lambda dt: torch.empty(cap, dtype=dt, device=device)
    return dict(chr=mk(torch.int32), start=mk(torch.int32), stop=mk(torch.int32), gc=mk(torch.int32), count=mk(torch.float32)), mk(torch.float64), mk(torch.int32), mk(torch.int32)


def _host(out, dcov, dst, dseg, n):
    return {k: v[:n].cpu().numpy() for k, v in out.items()}, dcov[:n].cpu().numpy(), dst[:n].cpu().numpy(), dseg[:n].cpu().numpy()


@pytest.mark.parametrize("nchr", [63, 64, 65, 1000])
def test_sample_pipeline_many_contigs_matches_oracle(nchr):
    """canvas_sample_pipeline (bin -> clean -> F2 -> PerSampleHMM -> segment ids in one call) against the oracle's chain"""
    cv = get_canvas()
    data, is_auto = M.genome(nchr)
    E = _oracle_pipeline(data, is_auto)
    lens = np.array([len(d[0]) for d in data], np.int64)
    db = [to_dev(pad16(d[0]), cv.device) for d in data]; dh = [to_dev(pad16(d[1]), cv.device) for d in data]; dm = [to_dev(d[2].view(np.int64), cv.device) for d in data]
    out, dcov, dst, dseg = _pipeline_buffers(cv.device, int(lens.sum() // 50) + 64)
    r = cv.sample_pipeline(db, dm, dh, lens, is_auto, out, dcov, dst, dseg, counts_per_bin=100, bin_size=-1, mode=3, flags=ALL)
    cv.synchronize()
    _check_pipeline(E, r, *_host(out, dcov, dst, dseg, r["n_out"]))


# ------------------------------------------------------------------------------------------------------------------------------------------------ Sharded
SHARD_NCHR = 300


def _shard_worker(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from canvas_amd import Canvas, parallel
        cv = Canvas(0)
        parallel.init_host_comm(cv, rank, world)
        data, is_auto = M.genome(SHARD_NCHR)
        lens = np.array([len(d[0]) for d in data], np.int64)
        owner = parallel.owner_table(lens, world)
        mine = lambda k: [to_dev(pad16(d[k]) if k < 2 else d[k].view(np.int64), cv.device) if owner[c] == rank else None for c, d in enumerate(data)]
        db, dh, dm = mine(0), mine(1), mine(2)
        out, dcov, dst, dseg = _pipeline_buffers(cv.device, int(lens.sum() // 50) + 64)
        r = cv.sample_pipeline_sharded(owner, db, dm, dh, lens, is_auto, out, dcov, dst, dseg, counts_per_bin=100, bin_size=-1, mode=3, flags=ALL)
        cv.synchronize()
        q.put((rank, owner.tolist(), dict(r, off=r["off"].tolist()), _host(out, dcov, dst, dseg, r["n_out"])))
        dist.destroy_process_group()
    except Exception:                                           # noqa: BLE001
        import traceback
        q.put((rank, "error", traceback.format_exc(), None))


def test_sharded_pipeline_many_contigs_equals_single_gpu_and_oracle():
    """two ranks on one GPU over the host transport, 300 contigs sharded between them: every rank gets the single-GPU call's result, which is the oracle's"""
    import socket
    import torch.multiprocessing as mp
    cv = get_canvas()
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_shard_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs: p.start()
    got = sorted([q.get(timeout=600) for _ in range(2)], key=lambda t: t[0])
    for p in procs: p.join(60)
    for g in got:
        assert g[1] != "error", g[2]
    assert sorted(set(got[0][1])) == [0, 1]
    data, is_auto = M.genome(SHARD_NCHR)
    E = _oracle_pipeline(data, is_auto)
    lens = np.array([len(d[0]) for d in data], np.int64)
    db = [to_dev(pad16(d[0]), cv.device) for d in data]; dh = [to_dev(pad16(d[1]), cv.device) for d in data]; dm = [to_dev(d[2].view(np.int64), cv.device) for d in data]
    out, dcov, dst, dseg = _pipeline_buffers(cv.device, int(lens.sum() // 50) + 64)
    r = cv.sample_pipeline(db, dm, dh, lens, is_auto, out, dcov, dst, dseg, counts_per_bin=100, bin_size=-1, mode=3, flags=ALL)
    cv.synchronize()
    single = _host(out, dcov, dst, dseg, r["n_out"])
    _check_pipeline(E, r, *single)
    for rank, _, rr, arrs in got:
        _check_pipeline(E, rr, *arrs)
        for a, b in zip(arrs[1:], single[1:]):
            assert a.tobytes() == b.tobytes(), rank


# ------------------------------------------------------------------------------------------------------------------------------------------------ Wavelets
@pytest.mark.parametrize("nchr", [63, 64, 65, 1024, 1025])
@pytest.mark.parametrize("germline", [True, False])
def test_wavelets_many_contigs_match_oracle(nchr, germline):
    """empty and one-bin contigs between long ones; past 64 chromosomes the factor-of-three statistics are computed on a host thread, past 1 024 the medians
    take one workgroup per chromosome"""
    cv = get_canvas()
    per_n = M.bin_counts_per_contig(nchr)
    for c in range(len(M.PRIMARY), nchr, 50):
        per_n[c] = 2_000 + 37 * (c % 11)                       # long ones among the contigs
    per_n[-1] = 6_000                                          # a long, noisy last chromosome: the factor-of-three statistics depend on it
    b, _ = M.bins(nchr, per=per_n)
    cov = np.round(b["count"].astype(np.float64), 2)
    off = M.offsets(b["chr"], nchr)
    cov[off[-2]:] = np.round(cov[off[-2]:] * np.random.RandomState(1).lognormal(0, 0.6, off[-1] - off[-2]), 2)
    per = [np.ascontiguousarray(cov[off[c]:off[c + 1]]) for c in range(nchr)]
    assert (O.factor_of_three(per) != O.factor_of_three(per[:-1])).any()
    exp = O.wavelets_genome(per, is_germline=germline, threads=8)
    got = cv.wavelets(to_dev(cov, cv.device), off, is_germline=germline)
    for c in range(nchr):
        assert got[c].tolist() == exp[c].tolist(), (c, len(per[c]), got[c][:8], exp[c][:8])


# ------------------------------------------------------------------------------------------------------------------------------------------------ CBS
CBS_CHILD = r'''
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import torch
import oracle_lib as O
from canvas_amd import Canvas
bound = float(os.environ["CANVAS_CBS_CACHE_GB"]) * 1e9
cv = Canvas(0)
rng = np.random.RandomState(17)
per = []
for c in range(3):
    n = 30000 + 9000 * c
    x = rng.normal(50.0, 7.0, n)
    for k in range(6): a = rng.randint(0, n - 3000); x[a:a + rng.randint(300, 3000)] += rng.choice([-1.5, 1.2, 2.0])
    per.append(np.round(x, 2))
for c in range(2000):
    n = int(rng.randint(4, 61))
    x = rng.normal(50.0, 7.0, n)
    if c % 5 == 0: x[n // 2:] += 25.0
    per.append(np.round(x, 2))
off = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int64)
cov = torch.from_numpy(np.concatenate(per)).to(cv.device)
exp, est = O.cbs_genome(per, 0.01, 10000, threads=16)
seg_len, nseg, st = cv.cbs(cov, off, 0.01, 10000)
got = seg_len.cpu().numpy()
bad = [c for c in range(len(per)) if not (int(nseg[c]) == len(exp[c]) and (got[off[c]:off[c] + nseg[c]] == exp[c]).all())]
cs = cv.cbs_cache_stats()
print("segments-differ", len(bad), bad[:10], "stats", [int(v) for v in st[:7]], "oracle", [int(v) for v in est[:7]], "cache", [int(v) for v in cs], "bound", int(bound), flush=True)
if bad or int(st[0]) != int(est[0]) or int(st[2]) != int(est[2]) or int(st[4]) != int(est[4]): sys.exit(1)
if int(cs[1]) != 0: sys.exit(2)
if int(cs[4]) > bound: sys.exit(3)
print("DONE")
'''


def test_cbs_many_tiny_contigs_keep_the_long_chromosomes_cached():
    """2 000 contigs of 4-60 bins after three long chromosomes, with a cache bound that holds the long chromosomes' streams but not one 64 MB piece per contig:
    segments and RNG consumption of the oracle, no draws generated inside a batch (the long chromosomes' loops read from the cache; the contigs, too short for
    the device engine, have no stream), never more memory than the bound"""
    env = dict(os.environ, CANVAS_CBS_CACHE_GB="8")
    p = subprocess.run([sys.executable, "-c", CBS_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "DONE" in p.stdout, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])


# ------------------------------------------------------------------------------------------------------------------------------------------------ Executables
ALT_NAMES = ["chr1_KI270706v1_random", "chrUn_GL000220v1", "chrM", "chrEBV", "HLA-A*01:01:01:01"]


def _is_autosome_name(name):
    """tool_common.hpp: is_autosome — a name that is all digits once a leading "chr" is taken off"""
    n = name[3:] if name.startswith("chr") else name
    return len(n) > 0 and n.isdigit()


def _grch38_names(is_auto):
    """names for the chromosomes of many_contigs.bins: digits (with or without "chr") for the autosomes; for the others first ALT_NAMES, then GRCh38's unplaced /
    random / alt / decoy / HLA forms"""
    forms = ["chr%d_KI27%04dv1_random", "chrUn_GL00%04dv1", "chr%d_KI27%04dv1_alt", "chrUn_JTFH0100%04dv1_decoy", "HLA-B*%02d:%02d:01"]
    names, k = [], 0
    for c, a in enumerate(is_auto):
        if a:
            names.append("chr%d" % (c + 1) if c % 2 else "%d" % (c + 1))
            continue
        if k < len(ALT_NAMES):
            names.append(ALT_NAMES[k])
        else:
            f = forms[k % len(forms)]
            names.append(f % ((c % 22 + 1, c) if f.startswith("chr%d") else (c,) if f.count("%") == 1 else (c // 100, c % 100)))
        k += 1
    return names


def test_clean_and_partition_executables_on_grch38_names(tmp_path):
    """CanvasClean -> CanvasPartition (PerSampleHMM, Wavelets) on a .binned file of 300 chromosomes named as GRCh38 names its contigs: rows byte for byte the
    oracle's, with the autosomes those of tool_common.hpp:is_autosome"""
    import gzip
    get_canvas()
    from canvas_amd import build
    build.build_tools()
    BIN = os.path.join(ROOT, "canvas_amd", "bin")
    nchr = 300
    per_n = M.bin_counts_per_contig(nchr)
    per_n[:len(M.PRIMARY)] = [40_000, 20_000, 10_000]           # 50 000 bins and more: the local-SD metric is computed and written
    b, is_auto = M.bins(nchr, per=per_n)
    b["count"] = np.round(b["count"]).astype(np.float32)
    names = _grch38_names(is_auto)
    assert len(set(names)) == nchr and all(n in names for n in ALT_NAMES)
    assert [int(_is_autosome_name(n)) for n in names] == is_auto.tolist()
    rd = lambda path: gzip.open(path, "rt").read().splitlines()
    binned = str(tmp_path / "S.binned"); cleaned = str(tmp_path / "S.cleaned"); lsd = str(tmp_path / "S.localsd"); part = str(tmp_path / "S.partitioned")
    with gzip.open(binned, "wt") as f:
        for c, s_, e_, n_, g_ in zip(b["chr"], b["start"], b["stop"], b["count"], b["gc"]):
            f.write(f"{names[c]}\t{s_}\t{e_}\t{O.format_f2(float(n_))}\t{g_}\n")
    r = subprocess.run([os.path.join(BIN, "CanvasClean"), "-i", binned, "-o", cleaned, "-g", "-s", "-r", "--local-sd-metric-file", lsd], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    ex = O.clean(b["chr"], b["start"], b["stop"], F.f2_float(b["count"]), b["gc"], is_auto, np.zeros(nchr, np.uint8), ALL)
    rows = [f"{names[c]}\t{s_}\t{e_}\t{O.format_f2(float(n_))}\t{g_}" for c, s_, e_, n_, g_ in zip(ex["chr"], ex["start"], ex["stop"], ex["count"], ex["gc"])]
    assert rd(cleaned) == rows and ex["local_sd"] >= 0
    assert open(lsd).read() == "#localSD\t" + O.format_g15(ex["local_sd"]) + "\n"
    # CanvasPartition numbers the chromosomes in the order the file brings them: those Clean left bins of
    present = [c for c in range(nchr) if (ex["chr"] == c).any()]
    cov = F.f2_double(ex["count"])
    per = [cov[ex["chr"] == c] for c in present]
    bs = [ex["start"][ex["chr"] == c].astype(np.uint32) for c in present]; be = [ex["stop"][ex["chr"] == c].astype(np.uint32) for c in present]

    def rows_from(segstarts):
        ids, _ = O.postprocess(bs, be, segstarts)
        return [f"{names[c]}\t{s_}\t{e_}\t{O.format_g15(float(v))}\t{i}" for k, c in enumerate(present) for s_, e_, v, i in zip(bs[k], be[k], per[k], ids[k])]

    r = subprocess.run([os.path.join(BIN, "CanvasPartition"), "-i", cleaned, "-o", part, "-r", str(tmp_path), "-m", "PerSampleHMM"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    paths, ran = O.hmm_genome_per_sample(per, threads=8)
    assert rd(part) == rows_from([O.segments_from_path(paths[k], ran[k], bs[k], be[k])[0] for k in range(len(present))])
    vaf = str(tmp_path / "S.vaf"); open(vaf, "w").write("")
    r = subprocess.run([os.path.join(BIN, "CanvasPartition"), "-i", cleaned, "-o", part, "-r", str(tmp_path), "-v", vaf], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    bps = O.wavelets_genome(per, is_germline=False)
    assert rd(part) == rows_from([bs[k][bps[k]].astype(np.uint32) if (len(bps[k]) >= 2 and len(bs[k]) > 10) else bs[k][:1].astype(np.uint32) for k in range(len(present))])
