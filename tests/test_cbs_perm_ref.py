"""The plain restatement of one permutation of the hybrid test (cbs_perm_ref.py) against the oracle, at every size and data set the kernel tests use: xperm_py must be
the oracle's XPerm element for element, htmaxp_ld the oracle's HTMaxP within the tolerance the project uses between the oracle and the every-arc search
(test_oracle_independent.py), and the oracle's batch entry the same numbers as XPerm + HTMaxP one permutation at a time."""
import numpy as np
import pytest

import oracle_lib as O
from cbs_perm_ref import KINDS, KIND_SIZES, SEEDS, SIZES_ALL_KERNELS, SIZES_PAST_RP, htmaxp_ld, make_data, xperm_py

CASES = [("F2", n) for n, _ in SIZES_ALL_KERNELS + SIZES_PAST_RP] + [(k, n) for k in KINDS if k != "F2" for n in KIND_SIZES]


@pytest.mark.parametrize("kind,n", CASES, ids=[f"{k}-{n}" for k, n in CASES])
def test_restatement_equals_the_oracle(kind, n):
    x, tss = make_data(kind, n)
    assert abs(float(np.sum(x))) <= 1e-6 * max(1.0, float(np.sum(np.abs(x))))
    seed = SEEDS[n % 2]
    for b in ((0, 1) if n > 100_000 else (0, 1, 4)):
        px = xperm_py(x, seed, b)
        want = O.xperm(x, seed, b)
        assert px.tobytes() == want.tobytes(), (kind, n, b)
        v, ref = htmaxp_ld(px, tss), O.htmaxp(want, tss)
        assert abs(ref - v) <= 1e-11 * max(1.0, v), (kind, n, b, ref, v)
        if kind == "zeros":
            assert v == 0.0 and ref == 0.0
        if kind == "tiny" and n < 9000:                  # (tss = n * 1e-8: at 16385 bins the data sits just ABOVE the switch of "tss = best + 1", below it at the smaller sizes)
            assert tss < 1e-4


@pytest.mark.parametrize("n", [1024, 2081, 16385])
def test_oracle_batch_entry(n):
    for kind in ("F2", "ties"):
        x, tss = make_data(kind, n)
        got = O.htmaxp_batch(x, SEEDS[0], 5, tss)
        want = [O.htmaxp(O.xperm(x, SEEDS[0], b), tss) for b in range(5)]
        assert got.tolist() == want
