"""Inputs for the CanvasClean -m LOESS tests (test_loess_ref.py on the CPU, test_clean_loess_gpu.py on the GPU): every case is a function of a seed and is
built by hand, because the shapes wanted here (2 bins, one GC value, chrY alone at the GC extremes) are out of synth.generate_bins' reach.

A case is a dict: name, chr / start / stop / gc (int32), count (float32, two-decimal values as a .binned file holds), nchr, is_auto, is_y (or None), error
(True where the reference indexes out of range and the product must refuse).  Counts follow a smooth GC trend with multiplicative noise, so the bandwidth
search has a minimum to find."""
import functools

import numpy as np

import loess_ref as R

NCHR = 24                      # chromosome NCHR - 1 is chrY
TILE = 2048                    # LO_TILE of canvas_amd/csrc/loess.hpp
LARGE_N = 1024 * TILE + 1      # k_loess_col_scan takes its second chunk (with the carry) above 1024 tiles; the last tile holds one element

# Share of bins at which the oracle's float32 count is not bit-equal to the extended-precision reference rounded to float32, measured by
# test_loess_ref.py::test_oracle_matches_reference (every such bin is 1 ulp off: a double result and a longdouble result on two sides of a float32 rounding
# boundary).  Both evaluate the same real number with a relative error of n * 2^-53 at worst, so the share is about that error over the float32 spacing
# (2^-24): ORACLE_WORST_SHARE is the largest share over the cases.  The product is a third association of the same double sums with the device's log / exp, so
# the same order of magnitude is expected but not the same bins: the GPU tests allow CAP_FACTOR times the worst share, and never fewer than CAP_MIN_BINS bins.
ORACLE_SHARES = {"large": 1744 / LARGE_N, "gaps": 1 / 5000, "plain30k_s0": 1 / 30000}     # 8.32e-4, 2.0e-4, 3.3e-5; every other case: 0 bins
ORACLE_WORST_SHARE = max(ORACLE_SHARES.values())            # 8.32e-4 (the oracle's double result is within 7.4e-10 relative of the longdouble one there)
CAP_FACTOR = 10
CAP_MIN_BINS = 2


def cap_bins(n):
    return max(CAP_MIN_BINS, int(np.ceil(CAP_FACTOR * ORACLE_WORST_SHARE * n)))


def _trend(gc):
    g = gc.astype(np.float64)
    return np.exp(-0.9 * ((g - 47.0) / 28.0) ** 2) * (1.0 + 0.08 * np.sin(g / 6.0))


def _normal_gc(rng, n, lo=20, hi=75):
    return np.clip(np.round(rng.normal(45, 9, n)), lo, hi).astype(np.int32)


def _make(name, seed, n, gc=None, median=100.0, n_y=None, y_gc=None, zeros=0, is_y_given=True, error=False, gc_fn=None, extra_y=()):
    rng = np.random.RandomState(seed)
    if gc is None:
        gc = (gc_fn or _normal_gc)(rng, n)
    gc = np.asarray(gc, np.int32).copy()
    n_y = (n // 50 if n >= 200 else 0) if n_y is None else n_y
    # chromosome runs in file order: 0 .. NCHR-2 share the first n - n_y bins, chrY takes the rest
    chr_id = np.minimum(np.arange(n, dtype=np.int64) * (NCHR - 1) // max(1, n - n_y), NCHR - 2).astype(np.int32)
    if n_y:
        chr_id[n - n_y:] = NCHR - 1
        if y_gc is not None:
            gc[n - n_y:] = np.resize(np.asarray(y_gc, np.int32), n_y)
    first = np.concatenate([[0], np.flatnonzero(np.diff(chr_id)) + 1])
    pos = np.arange(n) - np.repeat(first, np.diff(np.concatenate([first, [n]])))
    start = (pos * 1000).astype(np.int32); stop = start + 1000
    count = median * _trend(gc) / _trend(np.array([45])) * np.exp(rng.normal(0, 0.12, n))
    count = np.maximum(np.round(count * 100.0) / 100.0, 0.01)              # two decimals, never zero by accident
    if zeros:
        count[rng.choice(n, zeros, replace=False)] = 0.0
    is_auto = np.ones(NCHR, np.uint8); is_auto[NCHR - 2:] = 0
    is_y = np.zeros(NCHR, np.uint8); is_y[NCHR - 1] = 1
    is_y[list(extra_y)] = 1
    return dict(name=name, chr=chr_id, start=start, stop=stop, gc=gc, count=count.astype(np.float32), nchr=NCHR, is_auto=is_auto,
                is_y=is_y if is_y_given else None, error=error)


def _gaps_gc(rng, n):
    allowed = np.array([g for g in range(20, 76) if not (40 <= g <= 47) and g % 5 != 0])
    return allowed[np.clip(np.round(rng.normal(len(allowed) / 2, len(allowed) / 5, n)), 0, len(allowed) - 1).astype(int)].astype(np.int32)


def _lone_gc(rng, n):
    g = _normal_gc(rng, n, 30, 60); g[n // 3] = 95
    return g


def _two_gc(rng, n):
    return np.where(rng.rand(n) < 0.5, 38, 57).astype(np.int32)


def _heavy_gc(rng, n):
    g = _normal_gc(rng, n); g[rng.rand(n) < 0.8] = 44
    return g


SEED = 20261017
_BUILDERS = {}


def _case(name, **kw):
    _BUILDERS[name] = lambda: _make(name, **kw)


# model sizes around the wave and the tile
for _k, _m in enumerate((2, 7, 63, 64, 65, 2047, 2048, 2049, 4097)):
    _case("m%d" % _m, seed=SEED + _k, n=_m)
_case("zeros4097", seed=SEED + 20, n=4097, zeros=60)                       # the model has one tile fewer than the bins; zero counts stay 0
_case("neg_even", seed=SEED + 21, n=3000, median=0.5, n_y=0)                 # nearly every log(count) negative, even and odd model size
_case("neg_odd", seed=SEED + 22, n=3001, median=0.5, n_y=0)
_case("gaps", seed=SEED + 23, n=5000, gc_fn=_gaps_gc)                        # GC 40..47 and every fifth value empty
_case("lone95", seed=SEED + 24, n=4000, gc_fn=_lone_gc)                      # one bin at GC 95, the rest in 30..60
_case("two_gc", seed=SEED + 25, n=3000, gc_fn=_two_gc)
_case("one_gc", seed=SEED + 26, n=2986, gc_fn=lambda rng, n: np.full(n, 45, np.int32))      # every window inside one GC run: all NaN
_case("heavy80", seed=SEED + 27, n=2986, gc_fn=_heavy_gc)                    # 80 % of the bins at GC 44: NaN for part of the bins
_case("y_10_90", seed=SEED + 28, n=5000, gc_fn=lambda rng, n: _normal_gc(rng, n, 25, 70), y_gc=[10, 90])     # chrY alone holds the GC extremes
_case("y_0_90", seed=SEED + 29, n=5000, gc_fn=lambda rng, n: _normal_gc(rng, n, 25, 70), y_gc=[0, 90])       # GC 0 on chrY alone: the reference runs (clamped index)
_case("gc0_autosome", seed=SEED + 30, n=3000, gc_fn=lambda rng, n: np.concatenate([[0], _normal_gc(rng, n - 1)]), error=True)
_case("no_is_y", seed=SEED + 31, n=3000, is_y_given=False)
for _s in range(3):
    _case("plain30k_s%d" % _s, seed=SEED + 40 + _s, n=30_000)
_case("large", seed=SEED + 50, n=LARGE_N)

# the file that the CanvasClean executable reads: three chromosome runs are chrY by the name rule of LoessGCNormalizer ("chry" or "y" after ToLower)
EXE_NAMES = ["chr%d" % (i + 1) for i in range(NCHR)]
EXE_NAMES[10] = "chrY"; EXE_NAMES[21] = "Y"; EXE_NAMES[NCHR - 1] = "chry"
_case("exe_names", seed=SEED + 32, n=5000, extra_y=(10, 21))


def _contigs1025():
    """tests/many_contigs.py's bin list over 1 025 contig runs, with chrY in the middle of the list instead of last"""
    import many_contigs as MC
    b, is_auto = MC.bins(1025)
    is_y = np.zeros(1025, np.uint8); is_y[512] = 1
    assert (b["chr"] == 512).sum() > 0
    return dict(name="contigs1025", nchr=1025, is_auto=np.asarray(is_auto, np.uint8), is_y=is_y, error=False, **{k: np.ascontiguousarray(v) for k, v in b.items()})


_BUILDERS["contigs1025"] = _contigs1025
NAMES = list(_BUILDERS)
SMALL = [k for k in NAMES if k not in ("large", "contigs1025") and not k.startswith("plain30k")]     # up to 5 000 points: the literal layer runs
OK_NAMES = [k for k in NAMES if k != "gc0_autosome"]


@functools.lru_cache(maxsize=None)
def get(name):
    c = _BUILDERS[name]()
    for k in ("chr", "start", "stop", "gc", "count"):
        c[k].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name, layer="grouped"):
    """the extended-precision reference of a case, computed once per process and shared"""
    c = get(name)
    r = R.normalize(c["count"], c["gc"], c["chr"], c["is_y"], layer=layer)
    for k in ("ld", "f32", "nan"):
        r[k].setflags(write=False)
    return r
