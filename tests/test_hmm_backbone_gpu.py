"""The exact backbone of the speculative Viterbi pass (k_vit_backbone, k_vit_backbone_scan, k_bb_*) on its own, through canvas_hmm_backbone_probe, against the plain sequential
FP64 sum.  k_vit_verify starts every block from carry[] and does not compare one block's last D with the next block's carry, so these carries must be the sequential sum bit
for bit: a carry one ulp off would pass the verification with shifted deltas.  Cases: tests/hmm_backbone_cases.py (lengths on the block / chunk / scan-iteration edges,
round-half-to-even ties at even and odd k, vanishing / subnormal / zero increments, increments above the running sum, binade crossings at chosen steps and in chosen
numbers).  A fail word is accepted only where the case list marks the (case, mode); everywhere else fail == 0 AND equal bits are asserted."""
import numpy as np
import pytest

import hmm_backbone_cases as K
import hmm_backbone_ref as R
from gpu_common import get_canvas

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    cs = K.build_cases()
    for c in cs:
        c.expected = R.carries_numpy(c.v)        # computed once, shared by the modes
    return cs


@pytest.mark.parametrize("mode", K.MODES, ids=[K.MODE_NAMES[m] for m in K.MODES])
def test_carries_are_the_sequential_sum(cases, mode):
    from canvas_amd.lib import BACKBONE_PROBE_UNTOUCHED
    cv = get_canvas()
    mine, v, off = K.genome(cases, mode)
    carry, fail = cv.backbone_probe(mode, v, off)
    bits = carry.view(np.uint64)
    wrong = []
    for i, c in enumerate(mine):
        got = bits[off[i]:off[i + 1]]
        T = len(c.v)
        if T < R.MIN_T:            # skipped: nothing written, no fail word
            assert (got == BACKBONE_PROBE_UNTOUCHED).all() and fail[i] == 0, c.name
            continue
        at = np.arange(0, T, R.CARRY_EVERY)
        rest = np.ones(T, bool); rest[at] = False
        assert (got[rest] == BACKBONE_PROBE_UNTOUCHED).all(), (c.name, "an element that is no carry was written")
        equal = bool((got[at] == c.expected.view(np.uint64)).all())
        if mode == K.CHAIN:
            assert fail[i] == 0
        if fail[i] != 0:
            if c.strict(mode):
                wrong.append((c.name, "gave up"))
            continue
        if not equal:
            bad = np.nonzero(got[at] != c.expected.view(np.uint64))[0]
            wrong.append((c.name, "first wrong carry at step %d of %d: %r, expected %r" % (at[bad[0]], T, carry[off[i] + at[bad[0]]], c.expected[bad[0]])))
    assert not wrong, wrong


def test_probe_refuses_bad_arguments():
    from canvas_amd import CanvasError
    cv = get_canvas()
    v = np.full(100, -1.0)
    with pytest.raises(CanvasError):
        cv.backbone_probe(3, v, [0, 100])
    with pytest.raises(CanvasError):
        cv.backbone_probe(-1, v, [0, 100])
    with pytest.raises(CanvasError):
        cv.backbone_probe(2, v, [0, 101])
    with pytest.raises(CanvasError):
        cv.backbone_probe(2, v, [0, 60, 40, 100])
    with pytest.raises(CanvasError):
        cv.backbone_probe(2, v, [1, 100])
    with pytest.raises(CanvasError):
        cv.backbone_probe(2, v.astype(np.float32), [0, 100])
    carry, fail = cv.backbone_probe(2, np.zeros(0), [0, 0])          # nothing to do is no error
    assert len(carry) == 0 and (fail == 0).all()
    carry, fail = cv.backbone_probe(1, v, [0, 100])
    assert fail[0] == 0 and carry[0] == 0.0 and carry[64] == -64.0
