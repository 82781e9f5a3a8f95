"""Reference-shaped inputs for the many-contig tests (test_many_contigs_gpu.py, test_many_contigs_oracle.py): a few scaled-down primary chromosomes followed by K
contigs the way GRCh38 with its unplaced / random / alt / decoy / HLA sequences has them — most a few kilobases long, a handful of bins or none each.

Chromosome counts decide code paths all over the product (per-chromosome tables by value up to 64 chromosomes, autosome flags in LDS up to 256, device-driven Clean up to
1 024 chromosome runs), so the generator puts autosomes and non-autosomes at indices on both sides of each of them, and gives the non-autosomes values far from the
autosomes' (a higher hit rate, larger counts): a wrong autosome flag anywhere moves a genome-wide statistic (bin size, Clean's GC medians and quartiles)."""
import numpy as np

from canvas_amd import synth

SEED = 20261016
RATE = 0.21                                   # hits per possible position of the autosomes (about 30x at 100 counts per bin: bins of ~476 positions)
RATE_OTHER = 0.55                             # ... and of the non-autosome contigs
RATE_EXTREME = 2.5                            # non-autosomes at indices above 255 and 1 023
PRIMARY = [420_000, 300_001, 180_000]         # scaled-down chr1..chr3 (autosomes)
EDGE_LENGTHS = [1, 63, 64, 65, 4095, 4096, 4097]


def autosome_flags(nchr, seed=SEED):
    """mixed flags: the primaries are autosomes, about two thirds of the contigs too; past index 255 every multiple of 7 (and 256, 1 024) is a non-autosome"""
    rng = np.random.RandomState(seed + nchr)
    a = (rng.rand(nchr) < 0.65).astype(np.uint8)
    a[:len(PRIMARY)] = 1
    for c in range(256, nchr):
        if c % 7 == 0 or c in (256, 1024):
            a[c] = 0
    for c in (255, 257, 1023, 1025):
        if c < nchr:
            a[c] = 1
    return a


def extreme(c, is_auto):
    """a non-autosome past the LDS table with extreme values (the all-'n' contigs are non-autosomes too, but have no rate to flip)"""
    return c >= 256 and not is_auto[c] and c % 97 != 0


def flipped(is_auto):
    """the autosome flags with the extreme non-autosomes (above index 255) turned into autosomes (what a wrong flag past the LDS table would do)"""
    f = np.array(is_auto, np.uint8).copy()
    f[[c for c in range(256, len(f)) if extreme(c, is_auto)]] = 1
    return f


def contig_lengths(nchr, seed=SEED):
    """lengths of the chromosomes: the primaries, then the edge lengths (1, 63, 64, 65, 4 095, 4 096, 4 097 bases), then 2-40 kb (shorter, 2-12 kb, for very
    many contigs), a contig shorter than 8 kb has its leading 'n' gap (length / 8) inside its only tile or two"""
    rng = np.random.RandomState(seed + 7 * nchr)
    L = list(PRIMARY) + EDGE_LENGTHS
    hi = 40_000 if nchr <= 300 else 12_000
    while len(L) < nchr:
        L.append(int(np.exp(rng.uniform(np.log(2_000), np.log(hi)))))
    return np.array(L[:nchr], np.int64)


def genome(nchr, seed=SEED, bin_size=None):
    """per-base genome: list of (bases, hits, mask) and the autosome flags.  Every 97th contig is all 'n'; a chromosome without a possible position is no autosome.  bin_size given: three
    non-autosome contigs of bin_size - 1, bin_size and bin_size + 1 possible positions follow the edge lengths (0 bins, exactly one, one + a partial tail)."""
    is_auto = autosome_flags(nchr, seed)
    lens = contig_lengths(nchr, seed)
    thr = {r: synth.poisson_thresholds(r) for r in (RATE, RATE_OTHER, RATE_EXTREME)}
    data = []
    rng = np.random.RandomState(seed + 3)
    P = len(PRIMARY)
    special = {} if bin_size is None else {P + len(EDGE_LENGTHS) + k: bin_size - 1 + k for k in range(3)}
    for c in range(nchr):
        if c in special:
            L = special[c]
            is_auto[c] = 0
            b = rng.choice(np.frombuffer(b"ACGT", np.uint8), L)
            h = (rng.rand(L) < RATE_OTHER).astype(np.uint8) * rng.randint(1, 4, L).astype(np.uint8)
            bits = np.zeros((L + 63) // 64 * 64, np.uint8); bits[:L] = 1
            data.append((b, h, np.packbits(bits, bitorder="little")))
            continue
        L = int(lens[c])
        if c >= P and c % 97 == 0:
            data.append((np.full(L, ord('n'), np.uint8), np.zeros(L, np.uint8), np.zeros((L + 63) // 64 * 8, np.uint8)))
            continue
        r = RATE if is_auto[c] else (RATE_EXTREME if extreme(c, is_auto) else RATE_OTHER)
        data.append(synth.generate_chromosome(seed, c, L, r, thr[r]))
    for c, (b, h, m) in enumerate(data):
        if not m.any():
            is_auto[c] = 0                     # no possible position (all 'n', or a few bases all masked): its rate would be 0 / 0
    return data, is_auto


def bin_counts_per_contig(nchr, seed=SEED):
    """bins per chromosome for bin-level inputs: 0, 1, 10, 11 and 12 among the contigs, otherwise 2-60"""
    rng = np.random.RandomState(seed + 11 * nchr)
    n = rng.randint(2, 61, nchr)
    cyc = [0, 1, 10, 11, 12]
    for c in range(len(PRIMARY), nchr, 3):
        n[c] = cyc[(c // 3) % len(cyc)]
    n[:len(PRIMARY)] = [9_000, 6_001, 4_000]
    return n.astype(np.int64)


def bins(nchr, seed=SEED, per=None):
    """a CanvasBin-like bin list over the chromosomes (file order), SoA of numpy arrays, plus the autosome flags.  Non-autosomes above index 255 have three times the
    counts and GC 55-70 (their GC buckets' medians move if they are taken for autosomes).  The flags belong to the reference, not the sample: every seed shares them."""
    is_auto = autosome_flags(nchr)
    per = bin_counts_per_contig(nchr, seed) if per is None else np.asarray(per, np.int64)
    rng = np.random.RandomState(seed + 5)
    chr_id = np.repeat(np.arange(nchr, dtype=np.int32), per)
    N = len(chr_id)
    size = np.maximum(100, np.exp(rng.normal(np.log(1050), 0.25, N))).astype(np.int64)
    start = np.zeros(N, np.int64)
    o = 0
    for c in range(nchr):
        k = int(per[c])
        start[o:o + k] = 10_000 + np.concatenate([[0], np.cumsum(size[o:o + k])[:-1]]) if k else 0
        o += k
    gc = np.clip(np.round(rng.normal(41, 6, N)), 0, 100).astype(np.int32)
    cn = np.ones(N)
    seg = rng.rand(N) < 0.002
    cn[seg] = rng.choice([0.5, 1.5, 0.02], seg.sum())
    ext = np.array([extreme(c, is_auto) for c in range(nchr)])[chr_id] if N else np.zeros(0, bool)
    cn[ext] *= 3.0
    gc[ext] = rng.randint(55, 71, ext.sum())
    mean = 100 * cn * (1 + 0.004 * (gc - 41) - 0.0003 * (gc - 41.0) ** 2)
    r = 60.0
    count = rng.negative_binomial(r, r / (r + np.maximum(mean, 0.5))).astype(np.float32)
    return dict(chr=chr_id, start=start.astype(np.int32), stop=(start + size).astype(np.int32), gc=gc, count=count), is_auto


def offsets(chr_id, nchr):
    return np.concatenate([[0], np.cumsum(np.bincount(chr_id, minlength=nchr))]).astype(np.int64)
