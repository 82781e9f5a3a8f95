"""Genomes for the tests of the CanvasBin kernels (canvas_amd/csrc/bin.hip, bin_tail.hpp, bin_packed.hpp) at their tile, pos0, wrap and grid edges, shared by the CPU test
(test_bin_edge_cases.py asserts, with the oracle and numpy alone, that every case reaches the state it is built for) and the GPU test (test_bin_edges_gpu.py).  numpy only.

A case is a Case(name, data, is_auto, bin_sizes, modes, counts_per_bin, meta): data = [(bases, hits, mask)] per chromosome as the oracle and test_bin_gpu._upload take them
(uint8 per base, uint8 per base, the mask as bytes of whole 64-bit words, bit i of the little-endian stream = position i), meta = what the case was built to reach.
pos0 is the first base that is not 'n'; a tile is 4096 positions, a word 64.

  group1_pos0()        where pos0 lies: every place of a tile, a word and a 16-byte group, the partial tail tile, L - 1, L, and behind k_find_pos0's first stride trip
  group2_saturation()  every word at the maxima of summarize_tile's packed fields (64 possible, 64 G/C, 64 hits of 255), its complement, a word-wise checkerboard
  group3_stops()       masks built so that bins close on bit 63 / bit 0 of a word, on the last / first position of a tile and on the chromosome's last base
  group4_sizes()       one chromosome, the bin sizes around the powers of two, above one tile, above 65535 and above the possible positions
  group5a_stride()     600 000 bins: the second stride trip of the persistent resolve kernel on byte arrays (63 bins a group) and packed planes (255 a group)
  group5b_slots()      chromosomes whose first bins fall on the group slots of that kernel
  group6_wrap()        masked-hit prefixes past 2^32 (twice inside one chromosome), two scan chunks, a chromosome that starts on a chunk's first tile
  group7_decisions()   the decisions k_tscan_apply's last workgroup takes: autosome sets, tie ranks, 2048 / 2049 autosomes, non-finite rates, nothing to derive a size from
  group8_bytes()       hit bytes around the clamp at 10 and the sign bit, all 256 base byte values"""
import collections
import functools

import numpy as np

TILE = 4096
N = ord("n")
PATTERN = np.frombuffer(b"ACGTacgtNGC", np.uint8)          # 11 bytes: no period of a word, of a tile or of a 16-byte group

Case = collections.namedtuple("Case", "name data is_auto bin_sizes modes counts_per_bin meta")


def case_lens(case):
    return np.array([len(b) for b, h, m in case.data], np.int64)


def pack_mask(bits):
    """0 / 1 per position -> the mask bytes (whole 64-bit words, the positions past the end clear)"""
    L = len(bits)
    full = np.zeros((L + 63) // 64 * 64, np.uint8)
    full[:L] = bits
    return np.packbits(full, bitorder="little")


def mask_bits(mask, L):
    return np.unpackbits(mask, bitorder="little")[:L]


def full_mask(L):
    return pack_mask(np.ones(L, np.uint8))


def pattern_bases(L, pattern=PATTERN):
    return np.tile(pattern, L // len(pattern) + 1)[:L].copy()


def pos0_of(bases):
    """the oracle's leading-'n' skip: len(bases) where every base is 'n'"""
    live = bases != N
    return int(np.argmax(live)) if live.any() else len(bases)


# ------------------------------------------------------------------------------------------------ group 1
G1_L = 3 * TILE + 5
G1_POS0 = [0, 1, 15, 16, 17, 63, 64, 4095, 4096, 4097, 8191, 8192, 12288, G1_L - 1, G1_L]
G1_LONG_L = 540_000
G1_LONG_POS0 = 2 * 64 * TILE + 3 * TILE + 37            # behind the first trip of k_find_pos0's 64 workgroups x 4096 positions, and behind the second trip's first 3 tiles


def pos0_chromosome(L, pos0):
    bases = pattern_bases(L)
    bases[:pos0] = N
    hits = (np.arange(L) % 13 + 1).astype(np.uint8)      # never zero, above the clamp at 10 now and then
    return bases, hits, full_mask(L)


@functools.lru_cache(maxsize=None)
def group1_pos0():
    data = [pos0_chromosome(G1_L, p) for p in G1_POS0] + [pos0_chromosome(G1_LONG_L, G1_LONG_POS0)]
    return Case("pos0", data, np.ones(len(data), np.uint8), (1, 64, 100, 4096, 5000), (3, 0), 100, dict(pos0=G1_POS0 + [G1_LONG_POS0]))


# ------------------------------------------------------------------------------------------------ group 2
G2_L = 2 * TILE + 3 * 64 + 7


@functools.lru_cache(maxsize=None)
def group2_saturation():
    L = G2_L
    gc = pattern_bases(L, np.frombuffer(b"GCgcCGg", np.uint8)); at = pattern_bases(L, np.frombuffer(b"ATatNTa", np.uint8))
    sat = (gc, np.full(L, 255, np.uint8), full_mask(L))
    empty = (at, np.zeros(L, np.uint8), full_mask(L))
    word = np.arange(L) // 64
    on = word % 2 == 0                                     # even words saturated; odd words: no possible position, no hit, no G/C
    checker = (np.where(on, gc, at), np.where(on, 255, 0).astype(np.uint8), pack_mask(on.astype(np.uint8)))
    return Case("saturation", [sat, empty, checker], np.ones(3, np.uint8), (1, 64, 4096, 4097), (0, 3), 100, dict(saturated=0, empty=1, checker=2))


# ------------------------------------------------------------------------------------------------ group 3
G3_B = 200                                                 # the bin size of the constructed stops: above 64 + 63, so that a closing word may be full whatever the carry


def stops_mask_bits(L, b, closings, fill):
    """mask bits under which bin k of size b closes exactly on closings[k] and no further bin closes.  fill: the word of every closing position is all set (the bits
    behind the closing position carry into the next bin); otherwise the closing position is the only bit of its word.  The other possible positions of a bin are spread
    over the words between the previous closing word and this one."""
    bits = np.zeros(L, np.uint8)
    carry, free = 0, 0                                     # possible positions behind the last closing position; first position of the words not yet used
    for p in closings:
        w0 = p - p % 64
        w1 = min(w0 + 64, L)
        assert w0 >= free, "closing positions must lie in different words, in rising order"
        if fill:
            bits[w0:w1] = 1
            need = b - carry - (p - w0 + 1)
            after = w1 - 1 - p
        else:
            bits[p] = 1
            need = b - carry - 1
            after = 0
        assert 0 <= need <= w0 - free, "no room for the bin's other possible positions"
        if need:
            stride = (w0 - free) // need
            bits[free + np.arange(need) * stride] = 1
        carry, free = after, w1
    assert carry < b
    return bits


def stops_chromosome(L, closings, fill, b=G3_B):
    hits = (np.arange(L) * 7 % 23).astype(np.uint8)
    return pattern_bases(L), hits, pack_mask(stops_mask_bits(L, b, closings, fill))


def sparse_chromosome(L, positions):
    bits = np.zeros(L, np.uint8)
    bits[np.asarray(positions)] = 1
    hits = (np.arange(L) * 5 % 17 + 1).astype(np.uint8)
    return pattern_bases(L), hits, pack_mask(bits)


G3_MAIN_L = 3 * TILE + 17
# bit 63 of a word, bit 0 of a word, the last position of a tile, the first position of a tile, the last base of the chromosome (L mod 4096 = 17)
G3_MAIN_CLOSINGS = [64 * 10 + 63, 64 * 20, TILE - 1, 2 * TILE, G3_MAIN_L - 1]
G3_TAIL_LENGTHS = [2 * TILE, 2 * TILE + 1, 2 * TILE + 4095]     # L mod 4096 = 0, 1, 4095 (17: the main chromosome)
G3_PER_TILE_L = 12 * TILE + 5
G3_PER_WORD_L = 3 * TILE + 100
G3_RUNS_L = 12 * TILE + 5
G3_RUNS = [10, 4000, 5 * TILE + 4095, 6 * TILE, 6 * TILE + 1, 11 * TILE + 3, 12 * TILE + 4]      # tiles 1-4 and 7-10 hold nothing: runs of zero-pop tiles inside a bin


@functools.lru_cache(maxsize=None)
def group3_stops():
    data, want, size_of = [], [], []
    for fill in (True, False):
        data.append(stops_chromosome(G3_MAIN_L, G3_MAIN_CLOSINGS, fill)); want.append([p + 1 for p in G3_MAIN_CLOSINGS]); size_of.append(G3_B)
        for L in G3_TAIL_LENGTHS:
            closings = [64 * 7 + 5, L - 1]
            data.append(stops_chromosome(L, closings, fill)); want.append([p + 1 for p in closings]); size_of.append(G3_B)
    per_tile = [t * TILE + t * 613 % TILE for t in range(12)] + [12 * TILE + 4]        # one possible position per tile, the last one on the last base
    data.append(sparse_chromosome(G3_PER_TILE_L, per_tile)); want.append([per_tile[k] + 1 for k in range(2, len(per_tile), 3)]); size_of.append(3)
    nw = (G3_PER_WORD_L + 63) // 64
    per_word = [min(w * 64 + w * 37 % 64, G3_PER_WORD_L - 1) for w in range(nw)]          # one possible position per 64-position word
    data.append(sparse_chromosome(G3_PER_WORD_L, per_word)); want.append([per_word[k] + 1 for k in range(2, len(per_word), 3)]); size_of.append(3)
    data.append(sparse_chromosome(G3_RUNS_L, G3_RUNS)); want.append([G3_RUNS[2] + 1, G3_RUNS[5] + 1]); size_of.append(3)
    # at bin size 1 every full word of the filled chromosomes closes 64 bins (16 in every 16-byte lane of bin_tile)
    return Case("stops", data, np.ones(len(data), np.uint8), (G3_B, 3, 1), (3, 0), 100, dict(stops=want, size_of=size_of))


# ------------------------------------------------------------------------------------------------ group 4
G4_L = 1_200_000
G4_SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 4095, 4096, 4097, 65535, 65536, 65537, 1_000_003)
G4_TOO_LARGE = 1_150_000                                   # above the possible positions (about 1.08 M), below the length


@functools.lru_cache(maxsize=None)
def group4_sizes():
    rng = np.random.RandomState(20261021)
    L = G4_L
    bases = rng.choice(np.frombuffer(b"ACGTacgtn", np.uint8), L); bases[:1234] = N
    hits = rng.randint(0, 30, L).astype(np.uint8)
    mask = pack_mask((rng.rand(L) < 0.9).astype(np.uint8))
    return Case("sizes", [(bases, hits, mask)], np.ones(1, np.uint8), G4_SIZES + (G4_TOO_LARGE,), (3,), 100, dict(too_large=G4_TOO_LARGE))


# ------------------------------------------------------------------------------------------------ group 5
G5A_L = 1_200_000
RESIDENT_WORKGROUPS = 256 * 2048 // 256                    # the most 256-thread workgroups an MI355X holds: 256 CUs x 2048 threads
G5_SLOTS_BYTES, G5_SLOTS_PACKED = 63, 255                  # RF_NEW of k_bin_resolve_fin: bins a workgroup owns per stride trip


def full_chromosome(L):
    return pattern_bases(L), (np.arange(L) % 16).astype(np.uint8), full_mask(L)     # hits below 16: the packed planes hold them unsaturated


@functools.lru_cache(maxsize=None)
def group5a_stride():
    return Case("stride", [full_chromosome(G5A_L)], np.ones(1, np.uint8), (2,), (3, 0), 100, dict(bins=G5A_L // 2))


G5B_B = 5
# the bin counts the issue names, in the order that puts the chromosomes' first bins on 0, 1 and 62 modulo 63 and on 0, 1 and 254 modulo 255
G5B_BINS = [62, 1, 64, 126, 1, 255, 2, 0, 254, 63]


@functools.lru_cache(maxsize=None)
def group5b_slots():
    data = [full_chromosome(n * G5B_B + k % G5B_B) for k, n in enumerate(G5B_BINS)]
    firsts = np.concatenate([[0], np.cumsum(G5B_BINS)[:-1]]).tolist()
    return Case("slots", data, np.ones(len(data), np.uint8), (G5B_B,), (3, 0), 100, dict(bins=G5B_BINS, firsts=firsts))


# ------------------------------------------------------------------------------------------------ group 6
TS_CHUNK = 8192                                            # tiles per workgroup of k_tscan_reduce / k_tscan_apply
G6_LENGTHS = [5 * TILE + 1,                                # A: 6 tiles
              8186 * TILE,                                 # B: ends exactly on the chunk boundary
              8225 * TILE + 5,                             # C: starts on tile 8192, spans the next chunk boundary, more than 8192 tiles, 255 x its length is above 2^33
              2 * TILE + 17]                               # D: its tileBase is no multiple of 8


def saturated_chromosome(L):
    return pattern_bases(L), np.full(L, 255, np.uint8), full_mask(L)


@functools.lru_cache(maxsize=None)
def group6_wrap():
    data = [saturated_chromosome(L) for L in G6_LENGTHS]
    ntiles = [(L + TILE - 1) // TILE for L in G6_LENGTHS]
    tile_base = np.concatenate([[0], np.cumsum(ntiles)[:-1]]).tolist()
    return Case("wrap", data, np.ones(4, np.uint8), (1000, 65536), (0,), 100, dict(tile_base=tile_base, ntiles=ntiles))


# ------------------------------------------------------------------------------------------------ group 7
BD_MAX_AUTO = 2048
PRIMES = [101, 103, 107, 109, 113, 127, 131, 137, 139, 149, 151, 157, 163, 167, 173, 179, 181, 191, 193, 197, 199]


def tiny_chromosome(L, possible, observed, shift=0):
    """`possible` mask bits and `observed` positions with a hit, both spread over the chromosome; the hits inside and outside the mask alike (the rate counts both)"""
    bits = np.zeros(L, np.uint8); hits = np.zeros(L, np.uint8)
    if possible: bits[(np.arange(possible) * L // possible + shift) % L] = 1
    if observed: hits[(np.arange(observed) * L // observed + 2 * shift) % L] = (np.arange(observed) % 14 + 1).astype(np.uint8)
    return pattern_bases(L), hits, pack_mask(bits)


def many_autosomes(n):
    """n autosomes of about 200 positions with rates observed / possible, all different: the possible counts are primes and the observed counts lie below them"""
    data = [tiny_chromosome(200 + c % 5, PRIMES[c % 21], 1 + c // 21, c % 3) for c in range(n)]
    return data + [tiny_chromosome(333, 300, 33)]


@functools.lru_cache(maxsize=None)
def group7_decisions():
    """cases with a bin size to expect (meta kind 'size'), with a non-finite rate ('bad_rate'), and the two that must raise ('no autosome', 'not positive')"""
    a, b, c, d = tiny_chromosome(300, 250, 60), tiny_chromosome(411, 300, 33, 1), tiny_chromosome(257, 200, 90, 2), tiny_chromosome(640, 512, 100)
    x = tiny_chromosome(500, 400, 77)                      # never an autosome
    silent = (c[0], np.zeros_like(c[1]), c[2])             # possible positions, no hit
    no_mask = tiny_chromosome(300, 0, 40); no_mask_no_hit = tiny_chromosome(300, 0, 0)
    mk = lambda name, data, auto, kind, cpb=5: Case(name, data, np.array(auto, np.uint8), (), (3,), cpb, dict(kind=kind))
    return [mk("one autosome", [x, a], [0, 1], "size"),
            mk("two autosomes", [a, x, b], [1, 0, 1], "size"),
            mk("three autosomes", [a, b, c, x], [1, 1, 1, 0], "size"),
            mk("four autosomes, two alike", [a, b, x, a, d], [1, 1, 0, 1, 1], "size"),
            mk("an autosome without a hit among three", [a, silent, b, x], [1, 1, 1, 0], "size"),
            mk("2048 autosomes", many_autosomes(BD_MAX_AUTO), [1] * BD_MAX_AUTO + [0], "size"),
            mk("2049 autosomes", many_autosomes(BD_MAX_AUTO + 1), [1] * (BD_MAX_AUTO + 1) + [0], "size"),
            mk("an autosome without a possible position, with hits", [a, no_mask, b, x], [1, 1, 1, 0], "bad_rate"),
            mk("an autosome without a possible position or a hit", [a, no_mask_no_hit, b, x], [1, 1, 1, 0], "bad_rate"),
            mk("no autosome", [a, b, x], [0, 0, 0], "no autosome"),
            mk("every autosome rate 0", [silent, x, (a[0], np.zeros_like(a[1]), a[2])], [1, 0, 1], "not positive")]


# ------------------------------------------------------------------------------------------------ group 8
G8_OUTLIERS = (11, 127, 128, 255)                          # one per 1024-position wave iteration of a tile: the clamp's first value, either side of the sign bit, the maximum
G8_L = 4 * TILE


def outlier_positions():
    """(position, value): in tile t the iteration i holds its single byte above 10 at another lane and another byte of the lane's 16"""
    return [(t * TILE + i * 1024 + (t * 17 + i * 5) % 64 * 16 + (t * 4 + i * 7) % 16, G8_OUTLIERS[i]) for t in range(4) for i in range(4)]


@functools.lru_cache(maxsize=None)
def group8_bytes():
    L = G8_L
    at = np.array([p for p, v in outlier_positions()])
    bits = (np.arange(L) % 5 != 0).astype(np.uint8); bits[at] = 1
    hits = (np.arange(L) % 11).astype(np.uint8)                                    # 0 .. 10
    for p, v in outlier_positions(): hits[p] = v
    clamp = (pattern_bases(L), hits, pack_mask(bits))
    L10 = 2 * TILE + 33
    tens = (pattern_bases(L10), np.full(L10, 10, np.uint8), pack_mask((np.arange(L10) % 7 != 3).astype(np.uint8)))
    sparse = np.zeros(L, np.uint8)                                                   # nonzero_bytes4: a lone 1, 127, 128 or 255 among zeros
    for k, v in enumerate((1, 127, 128, 255) * 8): sparse[k * 509 + k % 4] = v
    lone = (pattern_bases(L), sparse, pack_mask(bits))
    Lb = TILE + 777
    every = (np.arange(Lb) % 256).astype(np.uint8); every[:300] = N                  # all 256 byte values as bases; pos0 = 300 (byte 300 mod 256 = 44 is no 'n')
    every_byte = (every, (np.arange(Lb) % 9 + 1).astype(np.uint8), full_mask(Lb))
    return Case("bytes", [clamp, tens, lone, every_byte], np.ones(4, np.uint8), (1, 64, 100), (3, 0), 100, dict(clamp=0, tens=1, lone=2, every_byte=3))
