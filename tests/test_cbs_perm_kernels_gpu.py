"""The three device kernels of CBS' hybrid permutation test, one batch at a time through canvas_cbs_perm_probe, at the sizes where their paths change (cbs_perm_ref.py):
k_perm_stat (probe id 0), k_perm_fy (1) and k_perm_rp (2).  Production reaches each of them only in its own range of segment lengths; the probe runs any of them at any
length, so all three are compared at every size.

Every permutation's interval [lo, hi] must contain the oracle's XPerm + HTMaxP of the same permutation, be as tight as the engine's own hook demands
(CANVAS_CBS_TEST_VERIFY: hi - lo <= 1e-6 |exact| + 1e-300), and for three permutations contain the plain extended-precision restatement as well.  [-inf, inf] is how a
kernel gives a permutation up (the host then evaluates it); it contains everything, so give-ups are counted apart and none is expected: whether a permutation is given
up depends on (n, seed, b) alone and rp_plan's capacities sit 8 sigma above what plain MT19937 draws need."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from canvas_amd.lib import CanvasError
from cbs_perm_ref import BATCHES_AT_1024, KINDS, KIND_SIZES, SEEDS, SIZES_ALL_KERNELS, SIZES_PAST_RP, htmaxp_ld, make_data, xperm_py
from gpu_common import get_canvas

pytestmark = pytest.mark.gpu

KERNEL_NAMES = {0: "k_perm_stat", 1: "k_perm_fy", 2: "k_perm_rp"}
# (kernel, n, seed) -> permutations of the batch a kernel may give up by design.  At most one entry per kernel, at most 1 in 64 of its batch, never all (see the issue).
EXPECTED_GIVE_UPS = {}


@functools.lru_cache(maxsize=None)
def _data(kind, n):
    x, tss = make_data(kind, n)
    x.setflags(write=False)
    return x, tss


@functools.lru_cache(maxsize=None)
def _reference(kind, n, seed, nb):
    """the oracle's statistic of every permutation of the batch, and the restatement's of three of them; computed once, shared by the three kernels"""
    x, tss = _data(kind, n)
    exact = O.htmaxp_batch(x, seed, nb, tss)
    exact.setflags(write=False)
    plain = {b: htmaxp_ld(xperm_py(x, seed, b), tss) for b in sorted({0, min(1, nb - 1)} | ({nb - 1} if n <= 100_000 else set()))}
    return exact, plain


@functools.lru_cache(maxsize=None)
def _canvas():
    return get_canvas()


def _check(kernel, kind, n, nb, seed):
    cv = _canvas()
    x, tss = _data(kind, n)
    exact, plain = _reference(kind, n, seed, nb)
    lohi, _ = cv.cbs_perm_probe(x, seed, nb, kernel, tss)
    lo, hi = lohi[:, 0], lohi[:, 1]
    assert not np.isnan(lohi).any(), (KERNEL_NAMES[kernel], kind, n, seed)
    given_up = np.isinf(lo) | np.isinf(hi)
    ok = ~given_up
    width = float(np.max((hi[ok] - lo[ok]) / np.maximum(np.abs(exact[ok]), 1e-300), initial=0.0))
    print(f"{KERNEL_NAMES[kernel]} {kind} n {n} nb {nb} seed {seed}: given up {int(given_up.sum())}, widest interval {width:.2e} of the exact value")
    assert int(given_up.sum()) == EXPECTED_GIVE_UPS.get((kernel, n, seed), 0), (KERNEL_NAMES[kernel], kind, n, seed, np.nonzero(given_up)[0].tolist())
    outside = np.nonzero(ok & ~((lo <= exact) & (exact <= hi)))[0]
    assert len(outside) == 0, (KERNEL_NAMES[kernel], kind, n, seed, [(int(b), lo[b], exact[b], hi[b]) for b in outside[:4]])
    loose = np.nonzero(ok & ~(hi - lo <= 1e-6 * np.abs(exact) + 1e-300))[0]
    assert len(loose) == 0, (KERNEL_NAMES[kernel], kind, n, seed, [(int(b), lo[b], exact[b], hi[b]) for b in loose[:4]], width)
    for b, v in plain.items():
        if ok[b]:
            tol = 1e-11 * max(1.0, v)
            assert lo[b] - tol <= v <= hi[b] + tol, (KERNEL_NAMES[kernel], kind, n, seed, b, lo[b], v, hi[b])


_SIZE_CASES = [(k, n, nb, s) for n, nb in SIZES_ALL_KERNELS for k in (0, 1, 2) for s in SEEDS] + [(k, n, nb, s) for n, nb in SIZES_PAST_RP for k in (0, 1) for s in SEEDS]


@pytest.mark.parametrize("kernel,n,nb,seed", _SIZE_CASES, ids=[f"{KERNEL_NAMES[k]}-{n}-{s}" for k, n, nb, s in _SIZE_CASES])
def test_kernel_at_its_size_edges(kernel, n, nb, seed):
    _check(kernel, "F2", n, nb, seed)


_KIND_CASES = [(k, kind, n, s) for kind in KINDS if kind != "F2" for n in KIND_SIZES for k in (0, 1, 2) for s in SEEDS]


@pytest.mark.parametrize("kernel,kind,n,seed", _KIND_CASES, ids=[f"{KERNEL_NAMES[k]}-{kind}-{n}-{s}" for k, kind, n, s in _KIND_CASES])
def test_kernel_on_awkward_data(kernel, kind, n, seed):
    _check(kernel, kind, n, 64, seed)


@pytest.mark.parametrize("kernel", (0, 1, 2), ids=list(KERNEL_NAMES.values()))
@pytest.mark.parametrize("nb", BATCHES_AT_1024)
def test_batch_shapes(kernel, nb):
    _check(kernel, "F2", 1024, nb, SEEDS[0])


def test_second_round_of_a_persistent_workgroup():
    """513 permutations on at most 512 workgroups of k_perm_rp: one of them takes a second permutation"""
    _check(2, "F2", 16385, 513, SEEDS[0])


@pytest.mark.parametrize("n,nb", SIZES_PAST_RP)
def test_k_perm_rp_is_refused_past_its_largest_segment(n, nb):
    cv = _canvas()
    x, tss = _data("F2", n)
    with pytest.raises(CanvasError, match="libcanvas_hip error -1:"):          # CANVAS_ERR_INVALID
        cv.cbs_perm_probe(x, SEEDS[0], nb, 2, tss)
