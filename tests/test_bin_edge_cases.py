"""tests/bin_edge_cases.py held to its purpose: for every case, the condition that makes it reach the state of the CanvasBin kernels it is built for, asserted with
the oracle and numpy alone; where a case has a closed form, the oracle is held to that form too.  (The kernels themselves: test_bin_edges_gpu.py.)"""
import numpy as np

import bin_edge_cases as B
import oracle_lib as O

TILE = B.TILE


def _stops(chrom, bs, mode=3):
    b, h, m = chrom
    return O.bin_chromosome(b, m, h, bs, mode)[1]


def test_group1_pos0_lies_where_intended():
    case = B.group1_pos0()
    assert len(case.data) == 16 and [len(d[0]) for d in case.data] == [B.G1_L] * 15 + [B.G1_LONG_L]
    assert case.meta["pos0"][:15] == [0, 1, 15, 16, 17, 63, 64, 4095, 4096, 4097, 8191, 8192, 12288, B.G1_L - 1, B.G1_L]
    assert case.meta["pos0"][15] >= 64 * TILE + 3 * TILE and case.meta["pos0"][15] % TILE not in (0, TILE - 1)      # k_find_pos0's second stride trip, inside a tile
    for (b, h, m), p0 in zip(case.data, case.meta["pos0"]):
        L = len(b)
        assert int(np.argmax(b != B.N)) == (p0 if p0 < L else 0) and (b != B.N).any() == (p0 < L)
        assert B.pos0_of(b) == p0
        bits = B.mask_bits(m, L)
        assert bits.all() and (h > 0).all()
        if p0 > 0:
            assert bits[:p0].sum() >= 1 and (h[:p0] > 0).sum() >= 1                 # possible positions and hits in front of pos0: in the rates, not in the bins
        assert O.bin_rate(h, m) == 1.0
        for bs in case.bin_sizes:
            es, ee, eg, ec = O.bin_chromosome(b, m, h, bs, 3)
            assert len(es) == (L - p0) // bs
            if len(es):
                assert es[0] == p0 and (ee - es == bs).all()
    assert (B.G1_L - 1) >> 12 == B.G1_L >> 12 == 3 and B.G1_L % TILE == 5          # pos0 inside the partial tail tile: head tile = tail tile
    assert O.bin_size([1.0] * 16, 100) == 100


def test_group2_words_are_saturated():
    case = B.group2_saturation()
    L = B.G2_L
    assert L == 2 * TILE + 3 * 64 + 7
    b, h, m = case.data[case.meta["saturated"]]
    assert B.mask_bits(m, L).all() and (h == 255).all() and np.isin(b, np.frombuffer(b"GCgc", np.uint8)).all()
    assert 64 | 64 << 7 | 16320 << 14 < 2 ** 32 and 64 * 255 == 16320                # the packed summary of such a word: every field at its maximum
    es, ee, eg, ec = O.bin_chromosome(b, m, h, 64, 0)
    assert len(es) == L // 64 and (ec == 16320).all() and (eg == 100).all() and (ee - es == 64).all()
    es, ee, eg, ec = O.bin_chromosome(b, m, h, 64, 3)
    assert (ec == 640).all()
    es, ee, eg, ec = O.bin_chromosome(b, m, h, 4097, 0)
    assert ec.tolist() == [4097 * 255] * 2
    b, h, m = case.data[case.meta["empty"]]
    assert B.mask_bits(m, L).all() and (h == 0).all() and not np.isin(b, np.frombuffer(b"GCgcn", np.uint8)).any()
    es, ee, eg, ec = O.bin_chromosome(b, m, h, 64, 0)
    assert len(es) == L // 64 and (ec == 0).all() and (eg == 0).all()
    b, h, m = case.data[case.meta["checker"]]
    words = B.mask_bits(m, L)[:L // 64 * 64].reshape(-1, 64).sum(1)
    assert words[0::2].tolist() == [64] * len(words[0::2]) and not words[1::2].any()
    es, ee, eg, ec = O.bin_chromosome(b, m, h, 64, 0)
    assert (ec == 16320).all() and eg[0] == 100 and (eg[1:] == 50).all() and len(es) == (len(words) + 1) // 2      # a bin behind the first spans an empty word and a full one


def test_group3_bins_close_where_intended():
    case = B.group3_stops()
    for c, (chrom, want, bs) in enumerate(zip(case.data, case.meta["stops"], case.meta["size_of"])):
        assert _stops(chrom, bs).tolist() == want, c
    n_main = 1 + len(B.G3_TAIL_LENGTHS)
    for fill, first in ((True, 0), (False, n_main)):
        b, h, m = case.data[first]
        L = len(b)
        bits = B.mask_bits(m, L)
        stops = _stops(case.data[first], B.G3_B).tolist()
        closing = [s - 1 for s in stops]
        assert any(p % 64 == 63 and p % TILE != TILE - 1 for p in closing)            # bit 63 of a word inside a tile
        assert any(p % 64 == 0 and p % TILE != 0 for p in closing)                    # bit 0
        assert any(s % TILE == 0 for s in stops) and any((s - 1) >> 12 != s >> 12 for s in stops)      # the last position of a tile: k_bin_finalize's (stop - 1) >> 12
        assert any(s % TILE == 1 for s in stops)                                      # the first position of a tile
        assert any(s % 64 == 0 for s in stops) and any(s % 64 == 1 for s in stops)
        assert stops[-1] == L and L % TILE == 17                                      # the last base closes the last bin
        for p in closing:                                                             # the rest of the closing word set, or clear
            w = bits[p - p % 64: min(p - p % 64 + 64, L)]
            assert w.all() if fill else w.sum() == 1
        lengths = [len(case.data[first + k][0]) for k in range(n_main)]
        assert sorted(x % TILE for x in lengths) == [0, 1, 17, 4095]
        for k in range(n_main):
            assert _stops(case.data[first + k], B.G3_B)[-1] == lengths[k]
        # 64 bins closing inside one word at bin size 1
        if fill:
            s1 = _stops(case.data[first], 1)
            assert np.bincount((s1 - 1) // 64).max() == 64
    per_tile, per_word, runs = case.data[2 * n_main], case.data[2 * n_main + 1], case.data[2 * n_main + 2]
    L = len(per_tile[0])
    pops = np.add.reduceat(B.mask_bits(per_tile[2], L), np.arange(0, L, TILE))
    assert pops.tolist() == [1] * 13
    assert all(e >> 12 >= (s >> 12) + 2 for s, e in zip(*O.bin_chromosome(per_tile[0], per_tile[2], per_tile[1], 3)[:2]))     # every bin spans three tiles
    L = len(per_word[0])
    assert (np.add.reduceat(B.mask_bits(per_word[2], L), np.arange(0, L, 64)) == 1).all()
    L = len(runs[0])
    pops = np.add.reduceat(B.mask_bits(runs[2], L), np.arange(0, L, TILE))
    assert pops.tolist() == [2, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 1, 1]                     # runs of zero-pop tiles inside the two bins
    assert _stops(runs, 3).tolist() == [5 * TILE + 4096, 11 * TILE + 4]


def test_group4_sizes_cover_the_divisions_edges():
    case = B.group4_sizes()
    (b, h, m), = case.data
    L = len(b)
    possible = int(B.mask_bits(m, L)[B.pos0_of(b):].sum())
    assert L == 1_200_000 and 0.89 < possible / L < 0.91
    assert set((1, 2, 3, 63, 64, 65, 255, 256, 4095, 4096, 4097, 65535, 65536, 65537, 1_000_003)) <= set(case.bin_sizes)
    for bs in case.bin_sizes:
        assert len(_stops(case.data[0], bs)) == possible // bs
    assert possible < case.meta["too_large"] < L and possible // case.meta["too_large"] == 0


def test_group5_bins_reach_the_second_stride_trip_and_the_group_slots():
    case = B.group5a_stride()
    (b, h, m), = case.data
    total = len(_stops(case.data[0], 2))
    assert total == case.meta["bins"] == 600_000 and B.mask_bits(m, len(b)).all() and (h < 16).all()
    assert total > B.RESIDENT_WORKGROUPS * B.G5_SLOTS_PACKED == 522_240 and total > B.RESIDENT_WORKGROUPS * B.G5_SLOTS_BYTES == 129_024
    case = B.group5b_slots()
    assert sorted(case.meta["bins"]) == sorted([62, 1, 63, 64, 126, 0, 255, 254, 1, 2])
    bins = [len(_stops(chrom, B.G5B_B)) for chrom in case.data]
    assert bins == case.meta["bins"]
    firsts = np.concatenate([[0], np.cumsum(bins)[:-1]])
    assert firsts.tolist() == case.meta["firsts"]
    assert {0, 1, 62} <= set((firsts % 63).tolist()) and {0, 1, 254} <= set((firsts % 255).tolist())
    for (b, h, m), n in zip(case.data, bins):
        assert B.mask_bits(m, len(b)).all() and len(b) // B.G5B_B == n


def test_group6_prefixes_wrap_and_tiles_cross_the_chunks():
    case = B.group6_wrap()
    masked = [int(h.astype(np.int64)[B.mask_bits(m, len(b)).astype(bool)].sum()) for b, h, m in case.data]
    assert max(masked) > 2 ** 33
    lens = B.case_lens(case)
    ntiles = ((lens + TILE - 1) // TILE).tolist()
    tile_base = np.concatenate([[0], np.cumsum(ntiles)[:-1]]).tolist()
    assert tile_base == case.meta["tile_base"]
    assert sum(ntiles) > B.TS_CHUNK and max(ntiles) > B.TS_CHUNK
    assert B.TS_CHUNK in tile_base                                                    # a chromosome whose first tile is a chunk's first tile
    assert lens[1] % TILE == 0 and tile_base[1] + ntiles[1] == B.TS_CHUNK             # its neighbour ends exactly there
    assert tile_base[2] < 2 * B.TS_CHUNK < tile_base[2] + ntiles[2]                   # and it spans the next boundary
    assert any(t % 8 for t in tile_base)
    assert ntiles[0] == 6 and lens[3] == 2 * TILE + 17
    for (b, h, m), L in zip(case.data, lens.tolist()):
        es, ee, eg, ec = O.bin_chromosome(b, m, h, 1000, 0)
        assert len(es) == L // 1000 and (ec == 255_000).all() and (ee - es == 1000).all()


def _rates(case):
    return [O.bin_rate(h, m) for (b, h, m), a in zip(case.data, case.is_auto) if a]


def test_group7_decisions_have_what_they_need():
    cases = {c.name: c for c in B.group7_decisions()}
    autos = {name: int(c.is_auto.sum()) for name, c in cases.items()}
    assert [autos[n] for n in ("one autosome", "two autosomes", "three autosomes", "four autosomes, two alike", "2048 autosomes", "2049 autosomes")] == [1, 2, 3, 4, B.BD_MAX_AUTO, B.BD_MAX_AUTO + 1]
    for name, c in cases.items():
        assert all(0 < len(b) <= 640 for b, h, m in c.data), name
        if c.meta["kind"] != "size": continue
        r = _rates(c)
        bs = O.bin_size(r, c.counts_per_bin)
        assert bs > 0, name
        assert sum(len(_stops(chrom, bs)) for chrom in c.data) > 0, name               # and bins come of it
        s = sorted(r); n = len(s)
        med = s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2
        assert bs == int(c.counts_per_bin / med), name
    r = _rates(cases["four autosomes, two alike"])
    assert len(set(r)) == 3 and r[0] == r[2]
    assert _rates(cases["two autosomes"]) == [60 / 250, 33 / 300]
    assert 0.0 in _rates(cases["an autosome without a hit among three"]) and O.bin_size(_rates(cases["an autosome without a hit among three"]), 5) == int(5 / (33 / 300))
    for name in ("2048 autosomes", "2049 autosomes"):
        r = _rates(cases[name])
        assert len(set(r)) == len(r) and all(190 <= len(b) <= 333 for b, h, m in cases[name].data)
    for name, finite in (("an autosome without a possible position, with hits", np.isinf), ("an autosome without a possible position or a hit", np.isnan)):
        c = cases[name]
        with np.errstate(all="ignore"):
            r = [np.float64((h > 0).sum()) / np.float64(B.mask_bits(m, len(b)).sum()) for (b, h, m), a in zip(c.data, c.is_auto) if a]
        assert finite(r[1]) and np.isfinite([r[0], r[2]]).all() and r[0] > r[2] > 0
    assert not cases["no autosome"].is_auto.any()
    c = cases["every autosome rate 0"]
    assert _rates(c) == [0.0, 0.0] and any((h > 0).any() for b, h, m in c.data)


def test_group8_bytes_sit_alone_in_their_iteration():
    case = B.group8_bytes()
    b, h, m = case.data[case.meta["clamp"]]
    assert len(h) == 4 * TILE
    it = h.reshape(-1, 1024)
    assert ((it > 10).sum(1) == 1).all()
    assert it.max(1).reshape(4, 4).tolist() == [[11, 127, 128, 255]] * 4
    bits = B.mask_bits(m, len(b))
    assert bits[h > 10].all() and 0 < bits.sum() < len(b)
    lanes = {(int(p) % 1024) // 16 for p in np.nonzero(h > 10)[0]}; byte = {int(p) % 16 for p in np.nonzero(h > 10)[0]}
    assert len(lanes) >= 12 and len(byte) >= 8
    es, ee, eg, e3 = O.bin_chromosome(b, m, h, 64, 3); e0 = O.bin_chromosome(b, m, h, 64, 0)[3]
    assert int((e0 - e3).sum()) == 4 * (1 + 117 + 118 + 245)                          # what the clamp takes off: every outlier lies inside a bin
    b, h, m = case.data[case.meta["tens"]]
    assert (h == 10).all()
    assert (O.bin_chromosome(b, m, h, 64, 3)[3] == 640).all() and (O.bin_chromosome(b, m, h, 64, 0)[3] == 640).all()
    b, h, m = case.data[case.meta["lone"]]
    assert sorted(set(h.tolist())) == [0, 1, 127, 128, 255] and (h > 0).sum() == 32
    words = h.reshape(-1, 4)
    assert ((words > 0).sum(1) <= 1).all()
    b, h, m = case.data[case.meta["every_byte"]]
    assert B.pos0_of(b) == 300 and set(b[300:].tolist()) == set(range(256))
    es, ee, eg, ec = O.bin_chromosome(b, m, h, 256, 3)
    assert es[0] == 300 and (eg[1:] == 1).all()                                       # 4 of the 256 byte values are G / C: (int)(100f * 4 / 256)
