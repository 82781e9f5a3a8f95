"""Plain numpy reference of the order-statistics engine (canvas_amd/csrc/select.hpp) and the inputs its tests run on.

The engine returns the k-th smallest KEY of a union of segments, where the key of a float is its order-preserving unsigned image.  Here the image is written from its
definition, the k-th smallest comes from np.sort, and nothing of the kernel is restated.  The one thing this file knows about the kernel is the SHAPE of its histogram step
(tiles of TILE keys, 64 consecutive keys per wave and round, four leader rounds, a switch at more than 24 lanes left over): wave_profile / switch_rounds compute from the keys
which of those paths an input reaches, so that test_select_ref.py can assert that each input named after a path really takes it.

Every generator is seeded and returns a Case: data (float32 / float64 values, or raw uint32 / uint64 keys), segment offsets and queries (seg_lo, seg_hi, k)."""
import collections

import numpy as np

TILE = 4096         # keys per workgroup of the histogram step
MAXQ = 16           # queries one segment can carry
REP = 16            # histogram replicas: tile t flushes into replica t % REP
WAVE = 64
WAVES = 4           # waves per workgroup: wave w takes the 64-key groups w, w + 4, w + 8, ... of its tile
LEADERS = 4         # ballot rounds
LEFTOVER_MAX = 24   # more lanes than this left over after the rounds: the wave stops aggregating for the rest of the tile

Case = collections.namedtuple("Case", "name data seg_off queries")

_UINT = {4: np.uint32, 8: np.uint64}
_FLOAT = {4: np.float32, 8: np.float64}


# ---------------------------------------------------------------- the key image and its inverse
def key_of(values):
    """float32 -> uint32, float64 -> uint64: sign set => all bits flipped, otherwise the top bit is set"""
    values = np.ascontiguousarray(values)
    assert values.dtype in (np.float32, np.float64)
    U = _UINT[values.itemsize]
    u = values.view(U)
    top = U(1) << U(8 * values.itemsize - 1)
    return np.where((u & top) != 0, ~u, u | top).astype(U)


def value_of(keys):
    """the inverse of key_of: uint32 -> float32, uint64 -> float64"""
    keys = np.ascontiguousarray(keys)
    assert keys.dtype in (np.uint32, np.uint64)
    U = _UINT[keys.itemsize]
    top = U(1) << U(8 * keys.itemsize - 1)
    return np.where((keys & top) != 0, keys & ~top, ~keys).astype(U).view(_FLOAT[keys.itemsize])


def keys_of(data):
    """the unsigned keys of a case's data: the image of values, raw keys as they are"""
    data = np.ascontiguousarray(data)
    return key_of(data) if data.dtype.kind == "f" else data


def dtype_code(data):
    """the probe's dtype argument for a case's data"""
    return {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.uint32): 2, np.dtype(np.uint64): 3}[np.asarray(data).dtype]


def kth(keys, seg_off, seg_lo, seg_hi, k):
    """k-th smallest (0-based) unsigned key of the union of segments seg_lo..seg_hi (they are adjacent in the array), as a Python int"""
    part = np.sort(np.asarray(keys)[int(seg_off[seg_lo]):int(seg_off[seg_hi + 1])], kind="stable")
    assert 0 <= k < len(part)
    return int(part[k])


def expected(case):
    """uint64[nq]: the answer of every query of the case"""
    keys = keys_of(case.data)
    cache = {}
    out = np.zeros(len(case.queries), np.uint64)
    for i, (lo, hi, k) in enumerate(case.queries):
        if (lo, hi) not in cache:
            cache[(lo, hi)] = np.sort(keys[int(case.seg_off[lo]):int(case.seg_off[hi + 1])], kind="stable")
        out[i] = cache[(lo, hi)][k]
    return out


def calls_of(case, per_call=MAXQ):
    """a one-segment case with more queries than one call can carry, split into calls of per_call queries"""
    return [case._replace(queries=case.queries[i:i + per_call]) for i in range(0, len(case.queries), per_call)]


# ---------------------------------------------------------------- which path of the histogram step an input reaches
def wave_profile(keys, begin, end, prefixes, p):
    """Pass p (0 = top byte) over the tile keys[begin:end) with the queries' prefixes so far (ints of p bytes; any for p = 0): for each group of 64 consecutive keys
    (matching lanes, distinct (row, digit) among them, lanes left over after the first LEADERS distinct ones in lane order were taken out, rows present)"""
    keys = np.asarray(keys)
    bits = 8 * keys.itemsize
    tile = [int(x) for x in keys[begin:end]]
    rows = sorted(set(prefixes)) if p else [0]
    out = []
    for g in range(0, len(tile), WAVE):
        seen = collections.OrderedDict()
        for x in tile[g:g + WAVE]:
            hi = (x >> (bits - 8 * p)) if p else 0
            if hi in rows:
                cd = (rows.index(hi), (x >> (bits - 8 * (p + 1))) & 255)
                seen[cd] = seen.get(cd, 0) + 1
        counts = list(seen.values())
        out.append((sum(counts), len(counts), sum(counts[LEADERS:]), len({cd[0] for cd in seen})))
    return out


def switch_rounds(profile):
    """per wave of the tile: the round (0-based, 16 per full tile) in which it stops aggregating, None if it never does"""
    res = []
    for w in range(WAVES):
        rounds = profile[w::WAVES]
        res.append(next((r for r, (_, _, left, _) in enumerate(rounds) if left > LEFTOVER_MAX), None))
    return res


def prefix_of(key, bits, p):
    """the top p bytes of a key"""
    return int(key) >> (bits - 8 * p) if p else 0


# ---------------------------------------------------------------- inputs
def _rng(*seed):
    return np.random.default_rng([20261018, *[int(s) for s in seed]])


def _one_segment(name, data, ranks):
    n = len(data)
    return Case(name, data, np.array([0, n], np.int64), [(0, 0, int(k)) for k in ranks])


def standard_ranks(n, seed):
    """every rank up to 257 keys; beyond, the two ends, the middle pair and 10 seeded ranks (16 queries: one call)"""
    if n <= 257:
        return list(range(n))
    fixed = [0, 1, n // 2 - 1, n // 2, n - 2, n - 1]
    return fixed + [int(k) for k in _rng(n, seed, 7).integers(0, n, 10)]


SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 17 * 4096 + 1)


def size_case(n, width):
    """one segment of n values around zero (both signs), float32 (width 4) or float64 (8)"""
    v = _rng(n, width, 1).normal(0.0, 50.0, n).astype(_FLOAT[width])
    return _one_segment(f"size-{n}-f{8 * width}", v, standard_ranks(n, 1))


def special_values(width, n, seed=3):
    """(values, boundaries): negatives, +-0, denormals, +-inf and NaNs of both signs with several payloads, shuffled; boundaries = the ranks at which the classes
    -NaN < -inf < negative normals < negative denormals < -0 < +0 < positive denormals < positive normals < +inf < +NaN meet in key order"""
    U = _UINT[width]
    r = _rng(n, width, seed)
    mant_bits, exp_max = (23, 0xFF) if width == 4 else (52, 0x7FF)
    mant_mask = (1 << mant_bits) - 1
    sign = 1 << (8 * width - 1)
    payloads = [1 << (mant_bits - 1), (1 << (mant_bits - 1)) | 1, 1, mant_mask, 0x1234]
    few = max(1, n // 16)

    def pick(lst, m):
        return [lst[i] for i in r.integers(0, len(lst), m)]
    nan = [(exp_max << mant_bits) | p for p in payloads]
    inf = exp_max << mant_bits
    den = [int(x) for x in r.integers(1, mant_mask + 1, few)]
    normal = lambda m: [(int(e) << mant_bits) | int(f) for e, f in zip(r.integers(1, exp_max, m), r.integers(0, mant_mask + 1, m))]
    rest = n - 8 * few
    assert rest >= 2
    classes = [[sign | b for b in pick(nan, few)], [sign | inf] * few, [sign | b for b in normal(rest // 2)], [sign | b for b in den], [sign] * few,
               [0] * few, pick(den, few), normal(rest - rest // 2), [inf] * few, pick(nan, few)]
    bounds = np.cumsum([len(c) for c in classes])[:-1]
    bits = np.array([b for c in classes for b in c], U)
    r.shuffle(bits)
    return bits.view(_FLOAT[width]), [int(b) for b in bounds]


CONTENT_KINDS = ("random_bits", "whole_near_100", "two_decimal_near_37", "all_equal", "two_values", "top_byte_only", "bottom_byte_only", "ascending", "descending", "special")
CONTENT_SIZES = (4097, 8193)


def content_case(kind, n, width):
    """one segment of n elements of a named content: values (float of `width` bytes) where the content is about values, raw keys where it is about bits"""
    r = _rng(n, width, CONTENT_KINDS.index(kind))
    F, U = _FLOAT[width], _UINT[width]
    bits = 8 * width
    ranks = standard_ranks(n, 2)
    if kind == "random_bits":
        data = r.integers(0, 1 << bits, n, dtype=U)
    elif kind == "whole_near_100":
        data = r.poisson(100.0, n).astype(F)
    elif kind == "two_decimal_near_37":
        data = (np.round(r.normal(37.0, 6.0, n) * 100.0) / 100.0).astype(F)
    elif kind == "all_equal":
        data = np.full(n, 37.25, F)
    elif kind == "two_values":
        na = n // 3 + 1
        data = np.where(r.permutation(n) < na, F(-1.5), F(2.5)).astype(F)
        ranks = [0, na - 2, na - 1, na, na + 1, n - 1]
    elif kind == "top_byte_only":
        data = (r.integers(0, 256, n).astype(U) << U(bits - 8)) | U(0x00ABCDEF12345678 & ((1 << (bits - 8)) - 1))
    elif kind == "bottom_byte_only":
        data = (U(0xC0FFEE1234567800 >> (64 - bits)) & ~U(255)) | r.integers(0, 256, n).astype(U)
    elif kind == "ascending":
        data = np.sort(r.normal(0.0, 1000.0, n).astype(F))
    elif kind == "descending":
        data = np.sort(r.normal(0.0, 1000.0, n).astype(F))[::-1].copy()
    elif kind == "special":
        data, bounds = special_values(width, n)
        ranks = sorted({k for b in bounds for k in (b - 1, b)} | {0, n - 1})
    else:
        raise KeyError(kind)
    return _one_segment(f"{kind}-{n}-{data.dtype.name}", data, ranks)


def _group_with_digits(r, d):
    """64 digits with exactly d distinct values: the four that appear first (lanes 0..3) fill every lane the other d - 4, one lane each, leave free, so d - 4 lanes are left
    over after four leader rounds"""
    vals = [int(v) for v in r.permutation(256)[:d]]
    lanes = vals[:LEADERS] + vals[LEADERS:]
    lanes += [vals[i % min(LEADERS, d)] for i in range(WAVE - len(lanes))]
    return lanes


AGG_DISTINCT = (5, 24, 25, 28, 29)
AGG_NAMES = ("const_then_random", "random_then_const", "partial_random", "partial_5", "two_rows_on", "two_rows_off") + tuple(f"distinct_{d}_{where}" for d in AGG_DISTINCT for where in ("top", "bottom"))


def aggregation_case(name, width):
    """raw keys (uint of `width` bytes) built to reach one path of the ballot aggregation; what the name promises is asserted in test_select_ref.py"""
    U = _UINT[width]
    bits = 8 * width
    r = _rng(width, AGG_NAMES.index(name), 11)
    const = U(0x5A5A5A5A5A5A5A5A >> (64 - bits))
    rand = lambda m: r.integers(0, 1 << bits, m, dtype=U)
    if name == "const_then_random":            # one tile: 32 groups of one digit, then 32 groups of ~57: every wave switches off in its round 8
        data = np.concatenate([np.full(TILE // 2, const, U), rand(TILE // 2)])
    elif name == "random_then_const":          # every wave switches off in round 0 and counts the constant half with plain atomics
        data = np.concatenate([rand(TILE // 2), np.full(TILE // 2, const, U)])
    elif name == "partial_random":             # the second tile holds 37 keys: one group, 37 lanes in range
        data = rand(TILE + 37)
    elif name == "partial_5":                  # two full groups and one of 37 lanes, five digits each
        lanes = [x for _ in range(3) for x in _group_with_digits(r, 5)][:2 * WAVE + 37]
        data = (np.array(lanes, np.uint64).astype(U) << U(bits - 8)) | (const >> U(8))
    elif name.startswith("two_rows"):          # the top byte splits the keys in two (alternate lanes), the bottom byte holds the digits: in the last pass a wave meets two rows
        d = 4 if name.endswith("on") else 16   # distinct digits per row and group: 2 d (row, digit) pairs, of which the first two of each row fill the free lanes
        top, low = [], []
        for _ in range(TILE // WAVE):
            halves = []
            for _row in range(2):
                vals = [int(v) for v in r.permutation(256)[:d]]
                halves.append(vals + [vals[i % 2] for i in range(WAVE // 2 - d)])
            for a, b in zip(*halves):
                top += [0x10, 0x90]; low += [a, b]
        data = (np.array(top, np.uint64).astype(U) << U(bits - 8)) | ((const >> U(8)) & ~U(255)) | np.array(low, np.uint64).astype(U)
    else:
        _, d, where = name.split("_")
        lanes = np.array([x for _ in range(TILE // WAVE) for x in _group_with_digits(r, int(d))], np.uint64).astype(U)
        data = (lanes << U(bits - 8)) | (const >> U(8)) if where == "top" else (const & ~U(255)) | lanes
    n = len(data)
    ranks = sorted({0, n // 2 - 1, n // 2, n - 1} | {int(k) for k in r.integers(0, n, 6)})
    if name.startswith("two_rows"):
        ranks = [n // 4, n // 4 + 1, n // 2 + n // 4, n // 2 + n // 4 + 1]
    return _one_segment(f"agg-{name}-{data.dtype.name}", data, ranks)


QUERY_NAMES = ("sixteen_distinct", "sixteen_identical", "pair_last_pass", "pair_first_pass")


def query_case(name, width):
    """5000 raw keys on one segment and a set of queries of a named shape"""
    U = _UINT[width]
    bits = 8 * width
    n = 5000
    r = _rng(width, QUERY_NAMES.index(name), 13)
    if name == "sixteen_distinct":
        return _one_segment(f"q-{name}-u{bits}", r.integers(0, 1 << bits, n, dtype=U), [int(k) for k in r.permutation(n)[:16]])
    if name == "sixteen_identical":
        return _one_segment(f"q-{name}-u{bits}", r.integers(0, 1 << bits, n, dtype=U), [n // 3] * 16)
    if name == "pair_last_pass":               # neighbouring keys: base + 0 .. n - 1, the pair inside one block of 256
        base = (0x7F3C91D2A4B5C600 >> (64 - bits)) & ~255
        data = (np.uint64(base) + r.permutation(n).astype(np.uint64)).astype(U)
        return _one_segment(f"q-{name}-u{bits}", data, [2 * 256 + 100, 2 * 256 + 101])
    if name == "pair_first_pass":              # half the keys under top byte 0x10, half under 0x90: the middle pair parts in the first pass
        low = r.integers(0, 1 << (bits - 8), n, dtype=U)
        top = np.where(r.permutation(n) < n // 2, U(0x10), U(0x90)).astype(U) << U(bits - 8)
        return _one_segment(f"q-{name}-u{bits}", top | low, [n // 2 - 1, n // 2])
    raise KeyError(name)


def too_many_queries_case(width):
    """17 queries on one segment: refused"""
    c = query_case("sixteen_distinct", width)
    return c._replace(name=f"q-seventeen-u{8 * width}", queries=c.queries + [(0, 0, 0)])


NSEG = 101
SEG_LENGTHS = (0, 1, 99, 100, 4096, 4097, 20011)


def _quartile_ranks(m):
    """median pair and quartile ranks of a segment of m keys (at most four distinct ranks)"""
    return sorted({m // 2, (m - 1) // 2, m // 4, (3 * m) // 4})


def segments_case(width, crowded=False, one_more=False):
    """101 segments like CanvasClean's GC buckets: empty ones at the front, in the middle and at the end, per-segment medians and quartile ranks, the union 0..100 and the
    partial union 40..60, all in one call.  crowded: segment 45 (4097 keys) carries 13 queries of its own, so that with the three union queries it carries 16;
    one_more: a fourth union query on top (17 on segment 45: refused)"""
    r = _rng(width, 17)
    lens = r.choice(SEG_LENGTHS, NSEG, p=[0.1, 0.1, 0.2, 0.2, 0.15, 0.15, 0.1])
    lens[[0, 1, 50, 51, 99, 100]] = 0
    lens[[2, 40, 49, 52, 60, 98]] = [1, 4096, 99, 100, 4097, 20011]
    lens[45] = 4097
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert off[-1] <= 1 << 20
    level = np.repeat(30.0 + 0.5 * np.arange(NSEG), lens)
    data = (np.round(r.normal(level, 5.0) * 100.0) / 100.0).astype(_FLOAT[width])
    queries = []
    for s in range(NSEG):
        if lens[s] and not (crowded and s == 45):
            queries += [(s, s, k) for k in _quartile_ranks(int(lens[s]))]
    if crowded:
        queries += [(45, 45, int(k)) for k in r.permutation(4097)[:13]]
    total, part = int(off[-1]), int(off[61] - off[40])
    queries += [(0, NSEG - 1, (total - 1) // 2), (0, NSEG - 1, total // 2), (40, 60, part // 2)]
    if one_more:
        queries.append((40, 60, 0))
    return Case(f"segments-{'crowded-' if crowded else ''}{'refused-' if one_more else ''}f{8 * width}", data, off, queries)


SEQUENCE_NQ = (1, 16, 3, 40, 2)


def sequence_cases(width):
    """five unrelated problems with 1, 16, 3, 40 and 2 queries for one context in turn (the 40 are spread over four segments)"""
    out = []
    for i, nq in enumerate(SEQUENCE_NQ):
        r = _rng(width, i, 19)
        nseg = 4 if nq > MAXQ else 1
        lens = r.integers(3000, 9000, nseg)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        data = r.normal(10.0 * i, 1.0 + i, int(off[-1])).astype(_FLOAT[width])
        queries = [(s, s, int(r.integers(0, lens[s]))) for s in list(range(nseg)) * (nq // nseg)]
        out.append(Case(f"sequence-{i}-nq{nq}-f{8 * width}", data, off, queries))
    return out


WG_COUNTS = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 5000)
WG_KINDS = ("special", "all_equal", "neighbours")


def wg_case(kind):
    """wg_select2: one segment per count (all but the first start at non-zero offsets), one workgroup per rank pair: (t, t), (t, t + 1) and (0, n - 1).  float64 values for
    'special' and 'all_equal', raw uint64 keys for 'neighbours'.  The queries are (segment, segment, (rank0, rank1))"""
    r = _rng(WG_KINDS.index(kind), 23)
    parts, queries = [], []
    for s, n in enumerate(WG_COUNTS):
        if kind == "special":
            parts.append(special_values(8, n, seed=s)[0] if n >= 63 else special_values(8, 64, seed=s)[0][:n])
        elif kind == "all_equal":
            parts.append(np.full(n, -0.0 if s % 2 else 3.75, np.float64))
        else:
            parts.append(np.uint64(0x7F3C91D2A4B5C600) + r.permutation(n).astype(np.uint64))
        pairs = {(t, t) for t in (0, n // 2, n - 1)} | {(t, t + 1) for t in (0, n // 2 - 1, n - 2) if 0 <= t < n - 1} | {(0, n - 1)}
        queries += [(s, s, p) for p in sorted(pairs)]
    off = np.concatenate([[0], np.cumsum(WG_COUNTS)]).astype(np.int64)
    return Case(f"wg-{kind}", np.concatenate(parts), off, queries)


def expected_pairs(case):
    """uint64[nq, 2] for a wg_case"""
    flat = case._replace(queries=[(lo, hi, k) for lo, hi, pair in case.queries for k in pair])
    return expected(flat).reshape(-1, 2)
