"""The grow-only arenas of a context (ctx->ws, pin, call_ws, call_pin, gc_arena) grown and then reused below their size: ONE Canvas context makes a small call, a
large call and the small call again through each of five entry points, and every result is compared bit for bit with the same call on a fresh context (and with the
CPU oracle where CanvasClean's and PerSampleHMM's own tests have one).  The large shapes need far more than 1.25 x the small call's workspace + 1 MB, which is what a
reservation leaves behind: the arena has to be reallocated, and the second small call carves a block that is much larger than its layout."""
import numpy as np
import pytest

import diploid_cases as DC
import oracle_lib as O
from canvas_amd import Canvas, synth, CLEAN_GCNORM, CLEAN_FILTSIZE, CLEAN_OUTLIERS, CLEAN_LOCALSD
from canvas_amd.lib import SELECT_MEDIAN_F64
from gpu_common import get_canvas, pad16, to_dev

pytestmark = pytest.mark.gpu
ALL = CLEAN_GCNORM | CLEAN_FILTSIZE | CLEAN_OUTLIERS | CLEAN_LOCALSD
SMALL = (700, 300, 11, 7)            # bins per chromosome: eleven is the shortest chromosome the speculative Viterbi pass does not skip
LARGE = (30_000,) * 4                # 120 000 bins: above the 50 000 where LocalSD starts
SMALL_BASES = (20_000, 5_000, 1_200)
LARGE_BASES = (2_000_000,) * 3


@pytest.fixture(scope="module")
def cv():
    return get_canvas()


@pytest.fixture(scope="module")
def bins():
    """size -> (SoA of exactly that many bins per chromosome, chromosome offsets): the first bins of every chromosome of a larger synthetic sample"""
    out = {}
    for sizes in (SMALL, LARGE):
        b = synth.generate_bins(20260927 + 40, 2 * sum(sizes) + 64, nchr=len(sizes), lengths=sizes)
        have = np.bincount(b["chr"], minlength=len(sizes)); first = np.concatenate([[0], np.cumsum(have)])
        assert (have >= sizes).all()
        keep = np.concatenate([np.arange(first[c], first[c] + sizes[c]) for c in range(len(sizes))])
        out[sizes] = ({k: np.ascontiguousarray(v[keep]) for k, v in b.items()}, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
    return out


def same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        g = np.asarray(g); w = np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (i, g.shape, w.shape, g.dtype, w.dtype)
        assert g.tobytes() == w.tobytes(), (i, np.nonzero(g.ravel() != w.ravel())[0][:8])


def small_large_small(cv, call, small, large):
    """-> the results of the small and of the large call (checked: on the one context in the order small, large, small, they equal a fresh context's)"""
    got = [call(cv, x) for x in (small, large, small)]
    fresh = [call(Canvas(0), x) for x in (small, large)]
    same(got[0], fresh[0]); same(got[1], fresh[1]); same(got[2], fresh[0])
    return fresh


def test_clean(cv, bins):
    """ctx->ws and ctx->pin (clean_batch_enqueue's layout, with the chromosome table behind it)"""
    def call(c, sizes):
        b, _ = bins[sizes]
        dev = {k: to_dev(v, c.device) for k, v in b.items()}
        n_out, lsd, info = c.clean(dev, len(b["chr"]), [1] * len(sizes), ALL)
        return [np.int64(n_out), np.float64(lsd)] + [dev[k][:n_out].cpu().numpy() for k in ("chr", "start", "stop", "gc", "count")]
    for sizes, got in zip((SMALL, LARGE), small_large_small(cv, call, SMALL, LARGE)):
        b, _ = bins[sizes]
        exp = O.clean(b["chr"], b["start"], b["stop"], b["count"], b["gc"], np.ones(len(sizes), np.uint8), np.zeros(len(sizes), np.uint8), ALL)
        assert exp["count"].dtype == np.float32
        same(got, [np.int64(len(exp["chr"])), np.float64(exp["local_sd"])] + [np.asarray(exp[k]).astype(np.int32) for k in ("chr", "start", "stop", "gc")] + [exp["count"]])


def test_hmm_per_sample(cv, bins):
    """ctx->ws through the layouts of hmm_pipeline (the common buffers, the descriptor blob, the mode's own buffers behind them)"""
    def call(c, sizes):
        b, off = bins[sizes]
        return [c.hmm_per_sample(to_dev(np.round(b["count"].astype(np.float64), 2), c.device), off).cpu().numpy()]
    for sizes, got in zip((SMALL, LARGE), small_large_small(cv, call, SMALL, LARGE)):
        b, off = bins[sizes]
        cov = np.round(b["count"].astype(np.float64), 2)
        per = [np.ascontiguousarray(cov[off[c]:off[c + 1]]) for c in range(len(sizes))]
        paths, ran = O.hmm_genome_per_sample(per, threads=8)
        assert list(ran) == [n > 10 for n in sizes]
        same(got, [np.concatenate([paths[c] if ran[c] else np.full(len(per[c]), -1, np.int32) for c in range(len(sizes))]).astype(np.int32)])


def test_segment_select(cv, bins):
    """ctx->ws and ctx->call_pin (one layout on the device base and on the pinned base): the chromosomes as segments — wave and LDS classes in the small call, tiled in the large"""
    def call(c, sizes):
        b, off = bins[sizes]
        out, nempty = c.segment_select(to_dev(b["count"], c.device), off, SELECT_MEDIAN_F64)
        return [out[:len(sizes)].cpu().numpy(), np.int64(nempty)]
    for sizes, got in zip((SMALL, LARGE), small_large_small(cv, call, SMALL, LARGE)):
        b, off = bins[sizes]
        same(got, [np.array([np.median(b["count"][off[c]:off[c + 1]].astype(np.float64)) for c in range(len(sizes))]), np.int64(0)])


def diploid_case(b, off, seed):
    """the bins of every chromosome as segments of 1 .. 64 bins (the last one takes what is left) with a few sites each"""
    rng = np.random.RandomState(seed)
    B = DC._Builder()
    for c in range(len(off) - 1):
        B.chrom()
        i, pos = int(off[c]), 1000
        while i < off[c + 1]:
            nb = int(min(off[c + 1] - i, rng.choice([1, 2, 7, 30, 64])))
            length = int(rng.choice([3000, 10000, 10186, 40000]))
            k = int(rng.choice([0, 3, 11, 25]))
            ps = np.sort(rng.randint(pos + 1, pos + length, k)); depth = rng.choice([9, 10, 30, 60], k); alt = (depth * rng.choice([0.0, 0.33, 0.5, 1.0], k)).astype(np.int64)
            B.seg(pos, pos + length, np.round(b["count"][i:i + nb], 2), [(int(p), int(d - a), int(a)) for p, d, a in zip(ps, depth, alt)])
            i += nb; pos += length + int(rng.choice([0, 1, 5000]))
    return B.done()


def test_call_diploid(cv, bins):
    """ctx->call_ws (what the call keeps across the selects it enqueues, which carve ctx->ws and ctx->call_pin)"""
    cases = {sizes: diploid_case(*bins[sizes], seed=7) for sizes in (SMALL, LARGE)}

    def call(c, sizes):
        a = cases[sizes]
        dev = {k: to_dev(a[k], c.device) for k in ("counts", "site_pos", "site_ref", "site_alt")}
        got = c.call_diploid(dev["counts"], a["chr_seg_offset"], a["seg_begin"], a["seg_end"], a["seg_bin_offset"], a["chr_site_offset"], dev["site_pos"], dev["site_ref"], dev["site_alt"])
        return [got[k] for k in sorted(got)]
    small_large_small(cv, call, SMALL, LARGE)
    assert len(cases[LARGE]["seg_begin"]) > 50 * len(cases[SMALL]["seg_begin"])


def test_bin_sample_gcweighted(cv):
    """ctx->gc_arena (the read-GC profile of every position), next to ctx->ws and ctx->pin"""
    import torch
    data = {}
    for lengths in (SMALL_BASES, LARGE_BASES):
        rng = np.random.RandomState(len(lengths) + lengths[0] % 97)
        chroms = [synth.generate_chromosome(20260927 + 41, c, L, 0.21) for c, L in enumerate(lengths)]
        fl = [np.where(h > 0, np.clip(rng.normal(350, 60, len(h)), 1, 5000), 0).astype(np.int16) for b, h, m in chroms]
        data[lengths] = (chroms, fl)

    def call(c, lengths):
        chroms, fl = data[lengths]
        bases = [to_dev(pad16(b), c.device) for b, h, m in chroms]; hits = [to_dev(pad16(h), c.device) for b, h, m in chroms]
        masks = [to_dev(m.view(np.int64), c.device) for b, h, m in chroms]; dfl = [to_dev(pad16(f), c.device) for f in fl]
        cap = sum(lengths) // 100 + 64
        out = {k: torch.empty(cap, dtype=torch.float32 if k == "count" else torch.int32, device=c.device) for k in ("chr", "start", "stop", "gc", "count")}
        _, per, total, bs = c.bin_sample_gcweighted(bases, masks, hits, dfl, np.array(lengths, np.int64), [1] * len(lengths), 100, 300, out=out)
        return [per, np.int64(total), np.int64(bs)] + [out[k][:total].cpu().numpy() for k in ("chr", "start", "stop", "gc", "count")]
    small, large = small_large_small(cv, call, SMALL_BASES, LARGE_BASES)
    assert small[1] > 0 and large[1] > 50 * small[1]
