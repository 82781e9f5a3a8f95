"""Inputs of the FlagUniqueKmers tests (test_kmer_ref.py on the CPU, test_kmer_gpu.py / test_kmer_tool_gpu.py on the GPU): hand-checked cases with their expected
flags written out, and seeded generators of the larger genomes.  Everything is a function of its seed."""
import numpy as np

from kmer_ref import revcomp

ACGT = np.frombuffer(b"ACGT", np.uint8)


def rand_seq(rng, n, alphabet=ACGT):
    return alphabet[rng.randint(0, len(alphabet), n)].tobytes()


def _flags(L, true_ranges):
    f = np.zeros(L, bool)
    for a, b in true_ranges:
        f[a:b] = True
    return f


def hand_cases():
    """[(name, contigs, expected flags)]: the fillers are seeded random sequence (100 random bases share no 35-mer, on either strand, by any realistic chance: the CPU
    test asserts the expected flags, so an accident would show there)"""
    rng = np.random.RandomState(35)
    R = rand_seq(rng, 100)
    cases = []
    # rule 2: p + 35 >= L is non-unique: of 100 positions 0..64 are keyed, 65 = L - 35 (whose 35-mer fits) is not
    cases.append(("tail", [R], [_flags(100, [(0, 65)])]))
    # L = 34, 35: nothing keyed (L <= 35 is entirely lower case); L = 36: position 0 alone; L = 37: positions 0 and 1
    shorts = [rand_seq(rng, n) for n in (34, 35, 36, 37)]
    cases.append(("short", shorts, [_flags(34, []), _flags(35, []), _flags(36, [(0, 1)]), _flags(37, [(0, 2)])]))
    # a 35-mer and its reverse complement on another contig: both non-unique, their neighbours untouched
    X, Y = rand_seq(rng, 20), rand_seq(rng, 50)
    B = X + revcomp(R[10:45]) + Y
    fa = _flags(100, [(0, 65)]); fa[10] = False
    fb = _flags(len(B), [(0, len(B) - 35)]); fb[20] = False
    cases.append(("revcomp_other_contig", [R, B], [fa, fb]))
    # three copies of one 35-mer
    S = rand_seq(rng, 35)
    f1, f2, f3, f4 = rand_seq(rng, 11), rand_seq(rng, 40), rand_seq(rng, 5), rand_seq(rng, 60)
    f1, f2, f3 = f1[:-1] + b"A", b"A" + f2[1:-1] + b"C", b"C" + f3[1:-1] + b"G"      # the bases next to the copies differ, so only the 35-mer itself repeats
    f4 = b"G" + f4[1:]
    T = f1 + S + f2 + S + f3 + S + f4
    ft = _flags(len(T), [(0, len(T) - 35)])
    for p in (11, 11 + 35 + 40, 11 + 35 + 40 + 35 + 5):
        ft[p] = False
    cases.append(("three_copies", [T], [ft]))
    # an N / an IUPAC code inside the window: the 35 windows that contain position 50 (16..50) are not keyed
    for ch in (b"N", b"R", b"-", b"*"):
        Rn = R[:50] + ch + R[51:]
        fn = _flags(100, [(0, 16), (51, 65)])
        cases.append(("non_acgt_" + ch.decode(), [Rn], [fn]))
    # soft-masked input: case carries no information
    Rl = R[:30].lower() + R[30:70] + R[70:].lower()
    cases.append(("soft_masked", [Rl], [_flags(100, [(0, 65)])]))
    cases.append(("soft_masked_copy", [R, Rl], [_flags(100, []), _flags(100, [])]))
    # a copy inside a contig's last 35 positions is never keyed: its partner stays unique
    F = rand_seq(rng, 30)
    C = F + R[20:55]                                   # length 65: the copy starts at 30 = L - 35
    cases.append(("copy_in_tail", [R, C], [_flags(100, [(0, 65)]), _flags(65, [(0, 30)])]))
    # ... one position earlier it is keyed, and both are non-unique
    C2 = F + R[20:55] + b"A"                           # length 66: the copy starts at 30 = L - 36
    fa2 = _flags(100, [(0, 65)]); fa2[20] = False
    cases.append(("copy_before_tail", [R, C2], [fa2, _flags(66, [(0, 30)])]))
    # an empty contig between two others
    cases.append(("empty_contig", [R, b"", C2], [fa2, _flags(0, []), _flags(66, [(0, 30)])]))
    return cases


def low_complexity_genome(seed, ncontigs=5, max_len=1500):
    """small genomes for restatement (a) against (b): few letters, repeats, Ns, short contigs"""
    rng = np.random.RandomState(seed)
    alphabets = [np.frombuffer(b"AC", np.uint8), np.frombuffer(b"AT", np.uint8), ACGT, np.frombuffer(b"ACGTN", np.uint8), np.frombuffer(b"ACGTacgtnR", np.uint8)]
    out = []
    for c in range(ncontigs):
        L = int(rng.choice([0, 1, 34, 35, 36, 37, 70, rng.randint(100, max_len)]))
        a = bytearray(rand_seq(rng, L, alphabets[rng.randint(len(alphabets))]))
        if L > 200:
            unit = rand_seq(rng, rng.randint(1, 41))
            at = rng.randint(0, L - 150)
            a[at:at + 120] = (unit * 120)[:120]
            if out and len(out[rng.randint(len(out))]) > 80:      # a copy from an earlier contig, either strand
                src = out[rng.randint(len(out))]
                if len(src) > 80:
                    s0 = rng.randint(0, len(src) - 60)
                    piece = src[s0:s0 + 60]
                    if rng.rand() < 0.5:
                        piece = revcomp(piece)
                    d0 = rng.randint(0, L - 60 + 1)
                    a[d0:d0 + 60] = piece
        out.append(bytes(a))
    return out


PLANTED_LENGTHS = [6_500_000, 5_000_003, 3_400_000, 2_300_017, 1_500_000, 900_001, 400_000]      # ~20 Mb


def planted_genome(seed=20261017, lengths=PLANTED_LENGTHS, plants=2600):
    """random ACGT contigs with planted material: forward and reverse-complement copies (a third of them from another contig, some landing in a contig's last positions),
    tandem repeats of period 1-40, homopolymer runs and N runs.  Returns a list of uint8 arrays."""
    rng = np.random.RandomState(seed)
    G = [ACGT[rng.randint(0, 4, L)] for L in lengths]
    n = len(G)
    for i in range(plants):
        kind = i % 8
        d = rng.randint(n); Ld = len(G[d])
        if kind in (0, 1, 2, 3, 4):                       # copies
            ln = int(rng.randint(36, 6000))
            s = rng.randint(n) if rng.rand() < 0.34 else d
            Ls = len(G[s])
            ln = min(ln, Ls // 4, Ld // 4)
            s0 = rng.randint(0, Ls - ln + 1)
            if i % 40 == 0:
                d0 = Ld - ln + rng.randint(0, 2) - 1 if ln < Ld else 0      # ends at, or one short of, the contig's end: its last starts are tail positions
                d0 = max(0, min(d0, Ld - ln))
            else:
                d0 = rng.randint(0, Ld - ln + 1)
            piece = G[s][s0:s0 + ln].copy()
            if kind in (3, 4):
                piece = (3 - np.searchsorted(ACGT, piece))[::-1]
                piece = ACGT[piece]
            G[d][d0:d0 + ln] = piece
        elif kind == 5:                                    # tandem repeat
            period = 1 + (i // 8) % 40
            ln = int(rng.randint(50, 3000))
            d0 = rng.randint(0, Ld - ln + 1)
            unit = ACGT[rng.randint(0, 4, period)]
            G[d][d0:d0 + ln] = np.tile(unit, ln // period + 1)[:ln]
        elif kind == 6:                                    # homopolymer
            ln = int(rng.randint(36, 500))
            d0 = rng.randint(0, Ld - ln + 1)
            G[d][d0:d0 + ln] = ACGT[rng.randint(4)]
        else:                                              # N run
            ln = int(rng.randint(1, 2000))
            d0 = rng.randint(0, Ld - ln + 1)
            G[d][d0:d0 + ln] = ord("N")
    return G


def two_letter_genome(seed=7, lengths=(1_000_000, 700_001)):
    """over {A, T} (closed under the reverse complement), with an exact copy of a stretch on the other strand"""
    rng = np.random.RandomState(seed)
    G = [np.frombuffer(b"AT", np.uint8)[rng.randint(0, 2, L)] for L in lengths]
    piece = G[0][1000:51000]
    G[1][200_000:250_000] = np.where(piece == ord("A"), ord("T"), ord("A")).astype(np.uint8)[::-1]
    return G


def period36_genome(seed=11, lengths=(1_000_000, 36 * 5000 + 17)):
    """one random 36-mer tiled over every contig: 36 distinct 35-mers, each tens of thousands of times"""
    rng = np.random.RandomState(seed)
    unit = ACGT[rng.randint(0, 4, 36)]
    return [np.tile(unit, L // 36 + 1)[:L].copy() for L in lengths]


def many_contig_genome(nchr=3000, seed=20261018):
    """lengths in the style of many_contigs.contig_lengths (a few primaries, the edge lengths, then kilobase contigs), plus empty contigs, contigs shorter than 36, all-'n'
    contigs and contigs that repeat an earlier one on either strand"""
    import many_contigs as MC
    rng = np.random.RandomState(seed)
    lens = [int(x) for x in MC.contig_lengths(nchr, seed)]
    for c in range(len(MC.PRIMARY) + len(MC.EDGE_LENGTHS), nchr):
        if c % 53 == 0:
            lens[c] = 0
        elif c % 29 == 0:
            lens[c] = int(rng.randint(1, 37))
    G = []
    for c, L in enumerate(lens):
        if c >= len(MC.PRIMARY) and c % 97 == 0:
            G.append(np.full(L, ord("n"), np.uint8))
        elif c > 20 and c % 11 == 0 and len(G[c - 7]) >= L > 0:
            src = G[c - 7][:L]
            G.append(ACGT[(3 - np.searchsorted(ACGT, src & 0xDF))[::-1] % 4] if c % 22 == 0 and (np.isin(src, ACGT)).all() else src.copy())
        else:
            a = ACGT[rng.randint(0, 4, L)]
            if L > 100 and c % 5 == 0:
                a[L // 3:L // 3 + 20] |= 0x20                       # soft-masked stretch
            G.append(a)
    return G
