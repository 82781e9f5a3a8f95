"""Plain restatements of what the Wavelets kernels compute (csrc/wavelets.hip), for tests/test_wavelets_ref.py (CPU) and tests/test_wavelets_kernels_gpu.py: Python floats
are IEEE doubles and the library is built with -ffp-contract=off, so the chain and subtree kernels must reproduce inner_products() bit for bit.  No GPU, no oracle."""
import math

import numpy as np

U = 2.0 ** -53


def inner_products(x):
    """GetInnerProdIter (WaveletSegmentation.cs:19-48): the two sequential recurrences -> (I+ - I-, mean of x)"""
    n = len(x)
    plus = [0.0] * (n - 1); minus = [0.0] * (n - 1)
    plus[0] = math.sqrt(1 - 1.0 / n) * x[0]
    rest = 0.0
    for v in x[1:]:
        rest += v
    mean = (x[0] + rest) / n
    minus[0] = (1.0 / math.sqrt(n * (n - 1))) * rest
    for m in range(1, n - 1):
        factor = math.sqrt(float(n - m - 1) * m / float(m + 1) / float(n - m))
        plus[m] = plus[m - 1] * factor + x[m] * math.sqrt(1.0 / (m + 1) - 1.0 / n)
        minus[m] = minus[m - 1] / factor - x[m] / math.sqrt((float(n) * n / float(m + 1)) - float(n))
    return [p - q for p, q in zip(plus, minus)], mean


def first_argmax(ipi):
    """GetInnerProdMax (WaveletSegmentation.cs:54-68): 1-based index of the first largest |value|"""
    top = max(abs(v) for v in ipi)
    for k, v in enumerate(ipi):
        if abs(v) == top:
            return k + 1


def coefficient(x, lim=None):
    """(coefficient, ind) of a node: ipi[ind - 1] / max(0.5, mean / 200) (WaveletSegmentation.cs:282, 314, 340); lim: the arg-max is taken over m <= lim only"""
    ipi, mean = inner_products([float(v) for v in x])
    if lim is not None:
        ipi = ipi[:max(0, int(lim)) + 1]
    ind = first_argmax(ipi)
    return ipi[ind - 1] / max(0.5, mean / 200.0), ind


def subtree(x, level, keep, s1=1):
    """a node with its whole subtree, depth first, with the child rules of WaveletSegmentation.cs:297, 323 (left [a, b] if b - a >= 1, right [b + 1, e] if e - b >= 2).
    -> ({level: nodes}, [(level, s, b, e, coefficient) with |coefficient| > keep]); s, b, e count from s1 at the node's first element"""
    x = [float(v) for v in x]
    counts, cands = {}, []
    todo = [(0, len(x) - 1, level)]
    while todo:
        a, e, lv = todo.pop()
        coef, ind = coefficient(x[a:e + 1])
        b = a + ind - 1
        counts[lv] = counts.get(lv, 0) + 1
        if abs(coef) > keep:
            cands.append((lv, s1 + a, s1 + b, s1 + e, coef))
        if e - b >= 2:
            todo.append((b + 1, e, lv + 1))
        if b - a >= 1:
            todo.append((a, b, lv + 1))
    return counts, cands


def closed_form(k):
    """T[m], B[m] (m = 0 .. n-2, in units of 100 x) of a node with the integers k = 100 x, from the formula of DESIGN.md (Wavelets, *The bound*) on exact Python integers:
         T[m] = A_m S_{m+1} - C_m R_{m+1},   A_m = sqrt((n-m-1) / (n (m+1))),   C_m = sqrt((m+1) / (n (n-m-1))),   S_j = k_0 + ... + k_{j-1},   R_j = S_n - S_j
         B[m] = u { A_m [4.02 SS_m + (3 + n/(n-m-1)) S_{m+1}] + C_m [(n + 1.01) R_1 + 4.03 RR_m + (3.5 + n/(2(n-m-1))) S_{m+1}] + 9 (A_m S_{m+1} + C_m R_{m+1}) } 1.01
    with SS_m = S_0 + ... + S_m, RR_m = R_1 + ... + R_m and n/(n-m-1) from the single-precision reciprocal, rounded up.  A model of the derivation, not of the kernel: the square
    roots are taken of the exact ratios."""
    k = [int(v) for v in k]
    n = len(k)
    S = [0] * (n + 1)
    for j in range(n):
        S[j + 1] = S[j] + k[j]
    T, B = [0.0] * (n - 1), [0.0] * (n - 1)
    SS = 0
    for m in range(n - 1):
        SS += S[m]                                        # S_0 + ... + S_m
        RR = m * S[n] - SS                                # R_1 + ... + R_m
        Sp, R = S[m + 1], S[n] - S[m + 1]
        A = math.sqrt((n - m - 1) / (n * (m + 1))); Cm = math.sqrt((m + 1) / (n * (n - m - 1)))
        ndr = n * float(np.float32(1.0) / np.float32(n - m - 1) * np.float32(1.000001)) * 1.000001
        T[m] = A * Sp - Cm * R
        B[m] = U * (A * (4.02 * SS + (3.0 + ndr) * Sp) + Cm * ((n + 1.01) * (S[n] - S[1]) + 4.03 * RR + (3.5 + 0.5 * ndr) * Sp) + 9.0 * (A * Sp + Cm * R)) * 1.01
    return T, B


def bound_ratio(ipi, T, B):
    """max over m of ||ipi[m]| 100 - |T[m]|| / B[m]; where B is 0 the two must be equal (-> inf otherwise)"""
    worst = 0.0
    for v, t, b in zip(ipi, T, B):
        d = abs(abs(v) * 100.0 - abs(t))
        if b == 0.0:
            if d != 0.0:
                return math.inf
        else:
            worst = max(worst, d / b)
    return worst


def decided(T, B):
    """the decision of the closed form: the index whose lower bound |T| - B lies above every OTHER index's upper bound |T| + B (1-based), or None"""
    lw = [abs(t) - b for t, b in zip(T, B)]
    up = [abs(t) + b for t, b in zip(T, B)]
    best = max(range(len(T)), key=lambda m: (lw[m], -m))
    others = max((up[m] for m in range(len(T)) if m != best), default=-math.inf)
    return best + 1 if lw[best] > others else None


def prefix_sums(k, off):
    """P1[i] = k_0 + ... + k_i, P2[i] = P1[0] + ... + P1[i], restarting at every chromosome (exact: int64)"""
    k = np.asarray(k, np.int64)
    p1 = np.zeros(len(k), np.int64); p2 = np.zeros(len(k), np.int64)
    for a, b in zip(off[:-1], off[1:]):
        p1[a:b] = np.cumsum(k[a:b]); p2[a:b] = np.cumsum(p1[a:b])
    return p1, p2


def stretch_median(k):
    """Utilities.Median (Utilities.cs:428-443) of x = k / 100: the middle element, or (lo + hi) / 2 on the doubles; 0 for an empty stretch"""
    n = len(k)
    if n == 0:
        return 0.0
    ks = np.sort(np.asarray(k, np.int64))
    if n & 1:
        return float(ks[n // 2]) / 100.0
    return (float(ks[n // 2 - 1]) / 100.0 + float(ks[n // 2]) / 100.0) / 2
