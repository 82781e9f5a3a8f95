"""A plain restatement of what one permutation of CBS' hybrid test computes (XPerm + HTMaxP, ChangePoint.cs:337-364,407-421; CBSTStatistic.cs:354-586), the data sets and
the sizes that test_cbs_perm_ref.py (CPU) and test_cbs_perm_kernels_gpu.py (the three device kernels, through canvas_cbs_perm_probe) share."""
import numpy as np

import oracle_lib as O

# ---- the sizes at which the device kernels change their path (cbs.hip): PT_TILE = RP_BK = 2048 steps, PT_HALO = 32 positions, RP_R = 16384 positions per range,
# RP_TAIL = 512 last steps, PERM_RP_MAX_N = 32 ranges = 524288.  (n, permutations in a batch)
SIZES_ALL_KERNELS = [(n, 64) for n in (1024, 1025, 2047, 2048, 2049, 2079, 2080, 2081,          # a tile +- the halo
                                       16383, 16384, 16385,                                      # the range boundary (and PERM_FY_MIN_N)
                                       16895, 16896, 16897)]                                     # the second range holds 511 / 512 / 513 positions (RP_TAIL)
SIZES_ALL_KERNELS += [(32769, 32), (49153, 32), (131073, 32), (524287, 8), (524288, 8)]         # 3, 4, 9 and 32 ranges; 8 permutations: the batch production uses there
SIZES_PAST_RP = [(524289, 8), (600001, 8)]                                                       # past PERM_RP_MAX_N: production routes to k_perm_fy
BATCHES_AT_1024 = (1, 63, 65, 513, 1025)
KIND_SIZES = (1024, 2049, 16385)
KINDS = ("F2", "ties", "offset", "tiny", "spike", "zeros")
SEEDS = (12345, 20260927)


def make_data(kind, n):
    """the centred data set and its tss"""
    rng = np.random.RandomState(1000 + n % 9973 + 7 * KINDS.index(kind))
    if kind == "F2":                      # what CanvasClean writes: two decimals; a weak step
        x = rng.normal(100, 10, n); x[n // 3:] += 0.4; x = np.round(x, 2)
    elif kind == "ties":                  # many partial sums exactly equal
        x = rng.randint(98, 103, n).astype(np.float64)
    elif kind == "offset":                # cancellation in the prefix sums
        x = 1e6 + rng.normal(0, 1, n)
    elif kind == "tiny":                  # tss < 1e-4: every permutation takes "tss = best + 1"
        x = rng.normal(0, 1, n) * 1e-4
    elif kind == "spike":
        x = np.zeros(n); x[int(rng.randint(0, n))] = 1e4
    elif kind == "zeros":
        x = np.zeros(n)
    else:
        raise ValueError(kind)
    x -= x.mean()
    return x, float(np.sum(x * x))


def xperm_py(x, seed, b):
    """XPerm (ChangePoint.cs:407-421) number b of a generator seeded with `seed`: permutation b takes the words [b n, (b + 1) n) of the stream, step i = n - 1 .. 0 takes
    word n - 1 - i of them, t = int(word * 2^-32 * (i + 1)) clamped to i, swap a[i], a[t]"""
    n = len(x)
    words = O.mt_u32(seed, (b + 1) * n)[b * n:].tolist()
    a = [float(v) for v in x]
    for i in range(n - 1, -1, -1):
        t = int(words[n - 1 - i] * 2.0 ** -32 * (i + 1))
        if t > i:
            t = i
        a[i], a[t] = a[t], a[i]
    return np.array(a, np.float64)


def htmaxp_ld(px, tss, k=25, al0=2):
    """HTMaxP as the maximum over EVERY circular arc of al0 .. k bins (no blocks, no pruning), prefix sums and arcs in extended precision"""
    n = len(px)
    p = np.asarray(px, np.float64).astype(np.longdouble)
    sums = np.concatenate([np.zeros(1, np.longdouble), np.cumsum(np.concatenate([p, p]))])
    best = np.longdouble(0.0)
    rn = np.longdouble(n)
    for length in range(al0, k + 1):
        arc = np.abs(sums[length:length + n] - sums[:n]).max()
        best = max(best, rn / (length * (rn - length)) * arc * arc)
    tss = np.longdouble(tss)
    if tss <= best + np.longdouble(0.0001):
        tss = best + np.longdouble(1.0)
    return float(best / ((tss - best) / (rn - 2)))
