"""The verification of the speculative Viterbi pass (k_vit_verify) and the retry ladder behind it, driven through CANVAS_HMM_TEST_CORRUPT.
  c:t:j      flips the guessed back-pointer of state j at step t of chromosome c: k_vit_verify must notice it wherever it sits (first step after the lead-in, the guarded last
             prefetch group, a last block of one step, the last step of the chromosome), the chromosome goes to the sequential kernel and the states are the oracle's;
  c:t:j:k    does so in the first k attempts and lets the retries run: attempt k (the to-do mask, the plain-chain backbone from attempt 2, the five-constant recurrence from
             attempt 3, lead-ins that reach the chromosome's start) must verify."""
import numpy as np
import pytest

import oracle_lib as O
import hmm_synth
from gpu_common import get_canvas, to_dev

pytestmark = pytest.mark.gpu

LENGTHS = [700, 1000, 300, 1024, 129, 500]          # targets: 1000, 1024 (8 blocks exactly), 129 (a last block of one step); none of them first
TARGETS = {1000: 1, 1024: 3, 129: 4}


def _steps(T):
    return sorted({t for t in (1, 2, 8, 9, 10, 63, 64, 65, 127, 128, 129, 136, 137, T - 10, T - 9, T - 2, T - 1) if 1 <= t < T})


class _Genome:
    def __init__(self, cv, seed, lengths, nsamples=1, **kw):
        self.cv = cv
        self.bins, cov, self.off = hmm_synth.coverage(seed, lengths, **kw)
        assert hmm_synth.dispersion(cov) < 0.2
        self.covs = [cov]
        rng = np.random.RandomState(seed + 1)
        for s in range(1, nsamples):
            self.covs.append(np.ascontiguousarray(np.round((cov * 0.8 + rng.normal(0, 3, len(cov))).clip(0), 2)))
        nchr = len(lengths)
        off = self.off
        if nsamples == 1:
            paths, ran = O.hmm_genome_per_sample([np.ascontiguousarray(cov[off[c]:off[c + 1]]) for c in range(nchr)], threads=4)
        else:
            res = [O.hmm_chromosome([np.ascontiguousarray(x[off[c]:off[c + 1]]) for x in self.covs], per_sample=False) for c in range(nchr)]
            ran, paths = [r[0] for r in res], [r[1] for r in res]
        self.expected = np.concatenate([p if r else np.full(len(p), -1, np.int32) for p, r in zip(paths, ran)])
        self.dev = [to_dev(c, cv.device) for c in self.covs]

    def run(self):
        if len(self.dev) == 1:
            return self.cv.hmm_per_sample(self.dev[0], self.off)
        return self.cv.hmm_joint(self.dev, self.off)

    def counters(self):
        return {k: self.cv.profile_get("viterbi_" + k)[1] for k in ("attempt", "retry", "sequential")}


@pytest.fixture(scope="module")
def genome():
    cv = get_canvas()
    cv.profile_enable(True)
    g = _Genome(cv, 20260927 + 200, LENGTHS)
    g.counters()
    g.base = g.run().cpu().numpy()
    assert (g.base == g.expected).all()
    assert g.counters() == {"attempt": 1, "retry": 0, "sequential": 0}
    return g


@pytest.mark.parametrize("T", sorted(TARGETS))
def test_every_flipped_pointer_is_caught(genome, T, monkeypatch):
    g, c = genome, TARGETS[T]
    assert LENGTHS[c] == T and c > 0
    missed = []
    for t in _steps(T):
        for j in range(5):
            monkeypatch.setenv("CANVAS_HMM_TEST_CORRUPT", f"{c}:{t}:{j}")
            got = g.run().cpu().numpy()
            k = g.counters()
            if k != {"attempt": 1, "retry": 0, "sequential": 1} or not (got == g.expected).all():
                missed.append((t, j, k, int((got != g.expected).sum())))
    assert not missed, missed


@pytest.mark.parametrize("bad", ["6:5:1", "1:0:1", "1:1000:1", "1:5:5", "1:5:1:0", "1:5:1:6", "1:5", "2", "1:5:1:1:1", "x", "1:-5:1", "", "1:5:1:"])
def test_hook_refuses_what_names_no_pointer(genome, bad, monkeypatch):
    from canvas_amd import CanvasError
    monkeypatch.setenv("CANVAS_HMM_TEST_CORRUPT", bad)
    with pytest.raises(CanvasError):
        genome.run()


def _ladder(g, c, t, j, monkeypatch):
    off = g.off
    others = np.ones(len(g.base), bool); others[off[c]:off[c + 1]] = False
    for k in (1, 2, 3, 4):
        monkeypatch.setenv("CANVAS_HMM_TEST_CORRUPT", f"{c}:{t}:{j}:{k}")
        got = g.run().cpu().numpy()
        assert g.counters() == {"attempt": k + 1, "retry": 1, "sequential": 0}, k
        assert (got == g.expected).all(), k
        assert (got[others] == g.base[others]).all(), k          # the chromosomes outside the to-do mask keep the first attempt's states
    monkeypatch.setenv("CANVAS_HMM_TEST_CORRUPT", f"{c}:{t}:{j}:5")
    got = g.run().cpu().numpy()
    assert g.counters() == {"attempt": 5, "retry": 1, "sequential": 1}
    assert (got == g.expected).all()


def test_retry_ladder_per_sample(genome, monkeypatch):
    _ladder(genome, 3, 700, 2, monkeypatch)


def test_segment_ids_enqueued_behind_a_corrupted_first_attempt_are_discarded(monkeypatch):
    """The one-call pipeline enqueues the segment ids behind the first attempt's verification (hmm_pipeline with seg != NULL).  When a chromosome takes another attempt those
    ids come from states that are not final: they must be thrown away and derived again.  The corrupted pointer lies ON the guessed path (the state the path has at that
    step), so the first attempt's path — and with it its ids — really differ from the final ones."""
    import torch
    from canvas_amd import synth, CLEAN_GCNORM, CLEAN_FILTSIZE, CLEAN_OUTLIERS, CLEAN_LOCALSD
    from gpu_common import pad16
    cv = get_canvas()
    cv.profile_enable(True)
    lengths = [1_500_000, 2_000_000, 1_200_000]
    is_auto = np.array([1, 1, 1], np.uint8)
    thr = synth.poisson_thresholds(0.21)
    data = [synth.generate_chromosome(20260927 + 210, c, L, 0.21, thr) for c, L in enumerate(lengths)]
    bases = [to_dev(pad16(b), cv.device) for b, h, m in data]; hits = [to_dev(pad16(h), cv.device) for b, h, m in data]
    masks = [to_dev(m.view(np.int64), cv.device) for b, h, m in data]
    lens = np.array(lengths, np.int64)
    flags = CLEAN_GCNORM | CLEAN_FILTSIZE | CLEAN_OUTLIERS | CLEAN_LOCALSD
    cap = int(lens.sum() // 100) + 16
    mk = lambda dt: torch.empty(cap, dtype=dt, device=cv.device)

    def run():
        out = dict(chr=mk(torch.int32), start=mk(torch.int32), stop=mk(torch.int32), gc=mk(torch.int32), count=mk(torch.float32))
        cov, st, seg = mk(torch.float64), mk(torch.int32), mk(torch.int32)
        for name in ("attempt", "retry", "sequential"):
            cv.profile_get("viterbi_" + name)
        r = cv.sample_pipeline(bases, masks, hits, lens, is_auto, out, cov, st, seg, counts_per_bin=100, bin_size=-1, mode=3, flags=flags)
        cv.synchronize()
        n = r["n_out"]
        k = {name: cv.profile_get("viterbi_" + name)[1] for name in ("attempt", "retry", "sequential")}
        return r, k, out, cov[:n].cpu().numpy(), st[:n], seg[:n].cpu().numpy()

    r0, k0, out0, cov0, st0, seg0 = run()
    off = r0["off"]
    nchr = 3
    assert k0 == {"attempt": 1, "retry": 0, "sequential": 0} and off[2] - off[1] > 400
    # the oracle: states, then the ids of PostProcessSegments
    per = [np.ascontiguousarray(cov0[off[c]:off[c + 1]]) for c in range(nchr)]
    paths, ran = O.hmm_genome_per_sample(per, threads=4)
    start, stop = out0["start"][:r0["n_out"]].cpu().numpy(), out0["stop"][:r0["n_out"]].cpu().numpy()
    bs = [start[off[c]:off[c + 1]].astype(np.uint32) for c in range(nchr)]; be = [stop[off[c]:off[c + 1]].astype(np.uint32) for c in range(nchr)]
    ids, last = O.postprocess(bs, be, [O.segments_from_path(paths[c], ran[c], bs[c], be[c])[0] for c in range(nchr)], None, 1000000)
    exp_state, exp_ids = np.concatenate(paths), np.concatenate(ids)
    assert (st0.cpu().numpy() == exp_state).all() and (seg0 == exp_ids).all() and r0["nseg"] == last + 1
    t = 300
    j = int(exp_state[off[1] + t])
    assert exp_state[off[1] + t - 1] == j          # inside a segment: the flipped pointer sends the guessed path through another state
    for k in (1, 3):
        monkeypatch.setenv("CANVAS_HMM_TEST_CORRUPT", f"1:{t}:{j}:{k}")
        r, kk, out, cov, st, seg = run()
        assert kk == {"attempt": k + 1, "retry": 1, "sequential": 0}, k
        assert (cov.view(np.uint64) == cov0.view(np.uint64)).all() and r["off"].tolist() == off.tolist()
        assert (st.cpu().numpy() == exp_state).all(), k
        assert (seg == exp_ids).all() and r["nseg"] == last + 1, k
        monkeypatch.delenv("CANVAS_HMM_TEST_CORRUPT")
        seg2, nseg2 = cv.segment_ids(off, st, out["start"], out["stop"])          # called afterwards on the final states
        assert nseg2 == r["nseg"] and (seg2[:r["n_out"]].cpu().numpy() == seg).all(), k


def test_retry_ladder_joint(monkeypatch):
    cv = get_canvas()
    cv.profile_enable(True)
    g = _Genome(cv, 20260927 + 201, [600, 1500, 400], nsamples=2, alts=(1, 3))
    g.counters()
    g.base = g.run().cpu().numpy()
    assert (g.base == g.expected).all()
    assert g.counters() == {"attempt": 1, "retry": 0, "sequential": 0}
    _ladder(g, 1, 777, 1, monkeypatch)


def test_one_step_lead_in_still_gives_the_oracle_states(genome, monkeypatch):
    """CANVAS_HMM_LEAD is read at every call: a cold start one step in front of every block guesses badly, and whatever the attempts it takes the states are exact"""
    g = genome
    monkeypatch.setenv("CANVAS_HMM_LEAD", "1")
    got = g.run().cpu().numpy()
    k = g.counters()
    assert (got == g.expected).all()
    assert 1 <= k["attempt"] <= 5 and k["sequential"] in (0, 1)
    monkeypatch.delenv("CANVAS_HMM_LEAD")
    got = g.run().cpu().numpy()
    assert (got == g.expected).all() and g.counters() == {"attempt": 1, "retry": 0, "sequential": 0}
