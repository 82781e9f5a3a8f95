"""Inputs of Canvas.call_diploid for the tests: a hand-built case that holds every boundary the caller has, randomised cases, and the one large case of the serial sum.
A case is a dict of the call's arguments as numpy arrays (counts, chr_seg_offset, seg_begin, seg_end, seg_bin_offset, chr_site_offset, site_pos, site_ref, site_alt)."""
import numpy as np

ARGS = ("counts", "chr_seg_offset", "seg_begin", "seg_end", "seg_bin_offset", "chr_site_offset", "site_pos", "site_ref", "site_alt")


class _Builder:
    def __init__(self):
        self.chrs = []                                       # per chromosome: ([(begin, end, counts)], [(pos, ref, alt)])

    def chrom(self):
        self.chrs.append(([], []))

    def seg(self, begin, end, counts, sites=()):
        self.chrs[-1][0].append((begin, end, np.asarray(counts, np.float32)))
        self.chrs[-1][1].extend(sites)
        return sum(len(c[0]) for c in self.chrs) - 1

    def sites(self, sites):
        self.chrs[-1][1].extend(sites)

    def done(self):
        segs = [s for c in self.chrs for s in c[0]]
        for c in self.chrs:
            c[1].sort(key=lambda t: t[0])
        sites = [s for c in self.chrs for s in c[1]]
        return dict(counts=np.concatenate([s[2] for s in segs]).astype(np.float32),
                    chr_seg_offset=np.concatenate([[0], np.cumsum([len(c[0]) for c in self.chrs])]).astype(np.int64),
                    seg_begin=np.array([s[0] for s in segs], np.int32), seg_end=np.array([s[1] for s in segs], np.int32),
                    seg_bin_offset=np.concatenate([[0], np.cumsum([len(s[2]) for s in segs])]).astype(np.int64),
                    chr_site_offset=np.concatenate([[0], np.cumsum([len(c[1]) for c in self.chrs])]).astype(np.int64),
                    site_pos=np.array([s[0] for s in sites], np.int32), site_ref=np.array([s[1] for s in sites], np.int32), site_alt=np.array([s[2] for s in sites], np.int32))


def _spread(begin, end, n, ref, alt):
    """n sites strictly inside [begin + 1, end - 1)"""
    return [(int(p), ref, alt) for p in np.linspace(begin + 2, end - 2, n).astype(np.int64)]


def edge_case():
    """Every count is chosen so that the mean of all bins is exactly 100: the model coverages are 0, 50, 100, ... and a median of 125 or 75 lies exactly midway between two
    of them.  Returns (case, names): names[label] = segment index."""
    b = _Builder(); n = {}
    flat = lambda k, v=100.0: np.full(k, v, np.float32)
    wobble = lambda k: np.where(np.arange(k) % 2 == 0, 99.5, 100.5).astype(np.float32)          # even k: the middle pair is (99.5, 100.5), the median their average
    b.chrom()
    n["begin_end"] = b.seg(1000, 201000, wobble(400), _spread(1000, 201000, 250, 15, 15) + [(1000, 12, 14), (200999, 13, 13), (201000, 20, 10)])   # at Begin, at End - 1, at End
    n["takes_site_at_end"] = b.seg(201000, 301000, flat(200), [(305000, 20, 20)])                   # holds the site at 201000 (Begin <= position); 305000 lies in the gap behind it
    n["gap_9999"] = b.seg(310999, 400000, flat(150))                                               # joins the run
    n["gap_10000"] = b.seg(410000, 500000, flat(100))                                              # does not
    n["density_10"] = b.seg(500000, 510185, flat(20), _spread(500000, 510185, 10, 10, 10))         # (End - Begin) / 463 / 2 = 10: ten sites are informative
    n["density_11"] = b.seg(510185, 520371, flat(20), _spread(510185, 520371, 10, 11, 10))         # ... = 11: ten sites are not, but MCC is kept
    n["nine_sites"] = b.seg(520371, 540371, flat(40), _spread(520371, 540371, 9, 12, 12) + [(530000, 5, 4), (530001, 9, 0)])        # MCC null; two sites of depth 9 dropped
    n["ten_sites"] = b.seg(540371, 560371, flat(40), _spread(540371, 560371, 9, 12, 12) + [(550000, 5, 5)])                          # depth 10 kept: ten sites
    n["cn3"] = b.seg(560371, 700000, flat(300, 150.0), _spread(560371, 700000, 200, 20, 10))
    n["cn1"] = b.seg(700000, 860000, flat(300, 50.0), _spread(700000, 860000, 200, 0, 30))
    n["tie_125"] = b.seg(860000, 900000, flat(50, 125.0))                                          # midway between CN 2 and CN 3, no MAF
    n["tie_75"] = b.seg(900000, 940000, flat(50, 75.0))
    n["tie_125_maf"] = b.seg(940000, 958000, flat(60, 125.0), _spread(940000, 958000, 20, 18, 12))
    n["tie_75_maf"] = b.seg(1000000, 1018000, flat(60, 75.0), _spread(1000000, 1018000, 20, 15, 15))
    b.chrom()
    n["cn6"] = b.seg(1000, 100000, flat(100, 300.0), _spread(1000, 100000, 120, 20, 10))            # max(1, CN - 4) = 2
    n["cn0"] = b.seg(100000, 300000, flat(200, 0.0))
    n["three_bins"] = b.seg(300000, 301500, flat(3))                                               # q-score 2 on its own ...
    n["thousand_bins"] = b.seg(301500, 900000, wobble(1000))                                       # ... 40 as the head of this run: the q10 filter flips
    n["moved_end_a"] = b.seg(920000, 1000000, flat(30))
    n["moved_end_b"] = b.seg(1000000, 1100000, flat(30))
    n["moved_end_c"] = b.seg(1105000, 1200000, flat(30))                                           # 105 000 behind the first segment's end, 5 000 behind the run's
    b.chrom()                                                                                      # a chromosome without segments: its sites are ignored
    b.sites([(100, 30, 30), (50, 30, 30)])
    b.chrom()
    n["next_chromosome"] = b.seg(1100000, 1190000, flat(60), _spread(1100000, 1190000, 12, 14, 16))    # CN 2 like the run in front of it, another chromosome
    n["short"] = b.seg(1195000, 1199000, flat(12, 150.0))                                          # L10kb
    n["short_pair"] = b.seg(1200000, 1203000, flat(12, 50.0))
    case = b.done()
    case["chr_site_offset"] = case["chr_site_offset"].copy()
    # the sites of the chromosome without segments stay unsorted on purpose (they are ignored before anything looks at them)
    c2 = slice(int(case["chr_site_offset"][2]), int(case["chr_site_offset"][3]))
    case["site_pos"][c2] = [100, 50]
    assert float(np.cumsum(case["counts"].astype(np.float64))[-1]) / len(case["counts"]) == 100.0
    return case, n


def random_case(seed, nchr=3, nseg=130):
    rng = np.random.RandomState(seed)
    b = _Builder()
    for _ in range(nchr):
        b.chrom()
        pos = int(rng.randint(0, 5000))
        level = 2
        for _ in range(nseg):
            pos += int(rng.choice([0, 0, 0, 1, 5000, 9999, 10000, 20000]))
            length = int(rng.choice([500, 3000, 9999, 10000, 10185, 10186, 40000, 250000]))
            if rng.rand() < 0.4:
                level = int(rng.choice([0, 1, 2, 2, 2, 3, 4, 6, 9]))
            nb = int(rng.choice([1, 2, 3, 4, 7, 30, 64, 65, 200]))
            counts = np.round(np.maximum(0, level * 50 + rng.randn(nb) * 6), 2)
            k = int(rng.choice([0, 3, 9, 10, 11, 25, 60]))
            ps = np.sort(rng.randint(pos - 50, pos + length + 50, k))
            depth = rng.choice([4, 9, 10, 30, 60], k)
            alt = (depth * rng.choice([0.0, 0.33, 0.5, 0.5, 0.67, 1.0], k)).astype(np.int64)
            b.seg(pos, pos + length, counts, [(max(1, int(p)), int(d - a), int(a)) for p, d, a in zip(ps, depth, alt)])
            pos += length
    return b.done()


def big_case():
    """three million counts near 100 with counts below 0.5 among them that are no multiples of 2^-24: the serial sum of Utilities.Mean and a tree sum differ"""
    rng = np.random.RandomState(5)
    n = 3_000_000
    x = np.round(rng.normal(100, 8, n), 2).astype(np.float32)
    small = rng.randint(0, n, n // 50)
    x[small] = (rng.rand(len(small)) * 0.49).astype(np.float32)
    b = _Builder(); b.chrom()
    edges = [0, 1_000_000, 2_200_000, n]
    for i in range(3):
        b.seg(edges[i] * 100, edges[i + 1] * 100, x[edges[i]:edges[i + 1]], _spread(edges[i] * 100, edges[i + 1] * 100, 50, 15, 15) if i != 1 else ())
    return b.done()


def args(case):
    return [case[k] for k in ARGS]


def file_case(seed, with_ploidy=False):
    """text inputs of the CanvasDiploidCaller executable: (*.partitioned lines, *.vaf lines, [(contig, length)] of GenomeSize.xml in ITS order, ploidy intervals or None).
    Bins of 500 .. 4 000 bases, segments of 1 .. 400 bins with copy-number levels, gaps between some segments, a contig without segments; the file order of the chromosomes differs from the order of GenomeSize.xml"""
    rng = np.random.RandomState(seed)
    contigs = [("chrB", 2_350_000), ("chrEmpty", 500_000), ("chrA", 3_120_500), ("chrX", 1_000_000)]
    part, vaf = [], []
    for name in ("chrA", "chrB", "chrX"):                      # the file's order differs from GenomeSize.xml's
        length = dict(contigs)[name]
        pos, seg_id, level = int(rng.randint(0, 3000)), 0, 2
        while pos < length - 50_000:
            if rng.rand() < 0.5:
                level = int(rng.choice([0, 1, 2, 2, 2, 3, 4, 6]))
            nb = int(rng.choice([1, 3, 12, 40, 150, 400]))
            for _ in range(nb):
                size = int(rng.choice([500, 1000, 1001, 4000]))
                if pos + size >= length:
                    break
                part.append("%s\t%d\t%d\t%.2f\t%d" % (name, pos, pos + size, max(0.0, level * 50 + rng.randn() * 5), seg_id))
                pos += size
            seg_id += 1
            pos += int(rng.choice([0, 0, 0, 700, 9999, 10000, 30000]))
        sites = np.sort(rng.randint(1, length, length // 1500))
        for p in sites:
            depth = int(rng.choice([6, 9, 10, 28, 40])); alt = int(depth * rng.choice([0.0, 0.3, 0.5, 0.5, 0.7, 1.0]))
            vaf.append("%s\t%d\tA\tG\t%d\t%d" % (name, p, depth - alt, alt))
    vaf = ["#chr\tpos\tref\talt\tnref\tnalt", ""] + vaf + ["chrUnplaced\t5\tA\tC\t50\t50"]
    ploidy = {"chrX": [(1, 600_000, 1), (600_001, 1_000_000, 2)], "chrB": [(1_000_001, 1_200_000, 0)]} if with_ploidy else None
    return part, vaf, contigs, ploidy
