"""Two independent CPU restatements of Tools/FlagUniqueKmers (KmerChecker.cs), the reference of canvas_flag_unique_kmers and of canvas_amd/bin/FlagUniqueKmers.

(a) KmerChecker: the C# class line by line — the Dictionary of packed string keys with the first occurrence's genome position, the nonUnique / finished flag arrays, the
    pass loop over a dictionary of at most MaxDictEntries entries (settable here; 400 000 000 in the reference) and the exception of :175-178.  Slow: hand cases and
    small randomised genomes.
(b) unique_flags_numpy: 70-bit canonical keys as (hi, lo) uint64 pairs, sorted, neighbours compared; the contig tail (:136) and the non-ACGT rule (:56-58) as masks.
    Fast enough for the GPU tests' larger genomes.

Contigs are `bytes`; a result is one bool array per contig, True = unique (upper case in the output)."""
import numpy as np

K = 35


# ---------------------------------------------------------------------------------------------------------------- (a)
class KmerChecker:
    KmerLength = K

    def __init__(self, max_dict_entries=400000000):
        self.MaxDictEntries = max_dict_entries
        self.Kmers = {}
        self.ChromosomeNonUniqueFlags = []
        self.ChromosomeFinishedFlags = []
        self.PassIndex = 0
        self.GenomePosition = 0
        self.IncompletePositions = 0

    @staticmethod
    def GetKeyForKmer(kmer):
        """:30-105: both strands packed four bases to a character, the ordinally smaller string; None with a character other than A C G T"""
        out = []
        currentChar = 0
        badChar = False
        for tempChar in range(len(kmer)):
            currentChar = (currentChar * 4) & 0xFF
            ch = kmer[tempChar]
            if ch == "A":
                currentChar += 0
            elif ch == "C":
                currentChar += 1
            elif ch == "G":
                currentChar += 2
            elif ch == "T":
                currentChar += 3
            else:
                badChar = True
            if tempChar % 4 == 3:
                out.append(chr(currentChar))
                currentChar = 0
        out.append(chr(currentChar))
        if badChar:
            return None
        key = "".join(out)
        out = []
        currentChar = 0
        charCount = 0
        for tempChar in range(len(kmer) - 1, -1, -1):
            currentChar = (currentChar * 4) & 0xFF
            ch = kmer[tempChar]
            if ch == "T":
                currentChar += 0
            elif ch == "G":
                currentChar += 1
            elif ch == "C":
                currentChar += 2
            elif ch == "A":
                currentChar += 3
            else:
                badChar = True
            if charCount % 4 == 3:
                out.append(chr(currentChar))
                currentChar = 0
            charCount += 1
        out.append(chr(currentChar))
        key2 = "".join(out)
        return key if key < key2 else key2          # string.Compare(..., Ordinal) < 0: code points below 256, Python compares them the same way

    def _flag_old(self, oldPos, finished_too_check):
        tempPos = 0
        for tempIndex in range(len(self.ChromosomeNonUniqueFlags)):
            if tempPos + len(self.ChromosomeNonUniqueFlags[tempIndex]) > oldPos:
                chrPos = oldPos - tempPos
                if finished_too_check:
                    if self.ChromosomeFinishedFlags[tempIndex][chrPos]:
                        raise Exception("Error: Flagging an already-done position!")
                    self.ChromosomeNonUniqueFlags[tempIndex][chrPos] = 1
                self.ChromosomeFinishedFlags[tempIndex][chrPos] = 1
                break
            tempPos += len(self.ChromosomeNonUniqueFlags[tempIndex])

    def ProcessOneChromosome(self, entry_bases, chromosomeIndex):
        if chromosomeIndex >= len(self.ChromosomeNonUniqueFlags):
            self.ChromosomeNonUniqueFlags.append(bytearray(len(entry_bases)))
            self.ChromosomeFinishedFlags.append(bytearray(len(entry_bases)))
        nonUniqueFlags = self.ChromosomeNonUniqueFlags[chromosomeIndex]
        finishedFlags = self.ChromosomeFinishedFlags[chromosomeIndex]
        bases = entry_bases.upper().decode("latin-1")      # ToUpperInvariant (:124): input case carries nothing (bytes.upper changes ASCII letters only)
        for startPos in range(len(bases)):
            try:
                if finishedFlags[startPos]:
                    continue
                if startPos + self.KmerLength >= len(bases):
                    nonUniqueFlags[startPos] = 1
                    finishedFlags[startPos] = 1
                    continue
                key = self.GetKeyForKmer(bases[startPos:startPos + self.KmerLength])
                if key is None:
                    nonUniqueFlags[startPos] = 1
                    finishedFlags[startPos] = 1
                    continue
                if key in self.Kmers:
                    nonUniqueFlags[startPos] = 1
                    finishedFlags[startPos] = 1
                    oldPos = self.Kmers[key]
                    if oldPos >= 0:
                        self._flag_old(oldPos, True)
                        self.Kmers[key] = -1
                else:
                    if len(self.Kmers) >= self.MaxDictEntries:
                        self.IncompletePositions += 1
                    else:
                        self.Kmers[key] = self.GenomePosition
            finally:
                self.GenomePosition += 1

    def Main(self, contigs):
        """:231-293 without the files: contigs = [bytes]; returns one bool array per contig, True = unique"""
        self.PassIndex = 0
        self.IncompletePositions = 1
        finishedChromosomes = set()
        while self.IncompletePositions > 0:
            self.IncompletePositions = 0
            self.PassIndex += 1
            self.Kmers.clear()
            self.GenomePosition = 0
            for chromosomeIndex, entry in enumerate(contigs):
                if chromosomeIndex in finishedChromosomes:         # (the reference keys this set by name; the index stands for a name that is unique in the file)
                    self.GenomePosition += len(entry)
                    continue
                self.ProcessOneChromosome(entry, chromosomeIndex)
                if self.IncompletePositions == 0:
                    finishedChromosomes.add(chromosomeIndex)
            for key, oldPos in self.Kmers.items():
                if oldPos < 0:
                    continue
                self._flag_old(oldPos, False)
        return [~np.frombuffer(bytes(f), np.uint8).astype(bool) for f in self.ChromosomeNonUniqueFlags]


def unique_flags_checker(contigs, max_dict_entries=400000000):
    ck = KmerChecker(max_dict_entries)
    flags = ck.Main([bytes(c) for c in contigs])
    return flags, ck.PassIndex


# ---------------------------------------------------------------------------------------------------------------- (b)
_CODE = np.full(256, 4, np.uint8)
for _i, _ch in enumerate(b"ACGT"):
    _CODE[_ch] = _i
    _CODE[_ch | 0x20] = _i


def unique_flags_numpy(contigs):
    """one bool array per contig (True = unique); contigs = bytes or uint8 arrays"""
    arrs = [np.frombuffer(bytes(c), np.uint8) if not isinstance(c, np.ndarray) else c.astype(np.uint8, copy=False) for c in contigs]
    his, los, owner, where = [], [], [], []
    for ci, a in enumerate(arrs):
        L = len(a)
        n = L - K                                  # keyed candidates: p + 35 < L  <=>  p < L - 35
        if n <= 0:
            continue
        code = _CODE[a]
        bad = (code > 3).astype(np.int32)
        cs = np.concatenate([[0], np.cumsum(bad)])
        ok = (cs[K:K + n] - cs[:n]) == 0            # no non-ACGT among the 35
        c64 = (code & 3).astype(np.uint64)
        fhi = np.zeros(n, np.uint64); flo = np.zeros(n, np.uint64); rhi = np.zeros(n, np.uint64); rlo = np.zeros(n, np.uint64)
        three = np.uint64(3)
        for j in range(K):
            x = c64[j:j + n]
            sh = 2 * (K - 1 - j)                    # forward: base j is digit 34 - j of the 70-bit number
            if sh >= 64:
                fhi |= x << np.uint64(sh - 64)
            else:
                flo |= x << np.uint64(sh)
            y = three - x                           # reverse complement: base j is its digit j, complemented
            if 2 * j >= 64:
                rhi |= y << np.uint64(2 * j - 64)
            else:
                rlo |= y << np.uint64(2 * j)
        fsmall = (fhi < rhi) | ((fhi == rhi) & (flo < rlo))
        hi = np.where(fsmall, fhi, rhi)[ok]; lo = np.where(fsmall, flo, rlo)[ok]
        his.append(hi); los.append(lo); owner.append(np.full(len(hi), ci, np.int32)); where.append(np.nonzero(ok)[0].astype(np.int64))
    out = [np.zeros(len(a), bool) for a in arrs]
    if not his:
        return out
    hi = np.concatenate(his); lo = np.concatenate(los); owner = np.concatenate(owner); where = np.concatenate(where)
    order = np.lexsort((lo, hi))
    shi = hi[order]; slo = lo[order]
    same_next = np.zeros(len(order), bool); same_next[:-1] = (shi[1:] == shi[:-1]) & (slo[1:] == slo[:-1])
    same_prev = np.zeros(len(order), bool); same_prev[1:] = same_next[:-1]
    uniq_sorted = ~(same_next | same_prev)
    sel = order[uniq_sorted]
    start = np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.int64)
    flat = np.zeros(int(start[-1]), bool)
    flat[start[owner[sel]] + where[sel]] = True             # one scatter over the concatenated genome (a loop over contigs is quadratic with thousands of them)
    return [flat[start[c]:start[c + 1]].copy() for c in range(len(arrs))]


# ---------------------------------------------------------------------------------------------------------------- helpers of the tests
def pack_mask(flags):
    """bool array -> uint64 words in System.Collections.BitArray layout (bit i = bit (i & 63) of word i >> 6), bits past the end 0"""
    L = len(flags)
    bits = np.zeros((L + 63) // 64 * 64, np.uint8)
    bits[:L] = flags
    return np.packbits(bits, bitorder="little").view(np.uint64) if L else np.zeros(0, np.uint64)


def apply_case(seq, flags):
    """KmerChecker.WriteOutputs (:215-224): ASCII letters upper where unique, lower where not; every other byte as it came"""
    a = np.frombuffer(bytes(seq), np.uint8).copy()
    letter = ((a | 0x20) >= ord("a")) & ((a | 0x20) <= ord("z")) & (a < 0x80)
    up = letter & np.asarray(flags, bool)
    lo = letter & ~np.asarray(flags, bool)
    a[up] &= 0xDF
    a[lo] |= 0x20
    return a.tobytes()


def render_fasta(names, seqs, flags):
    """the tool's output layout: '>' + name, '\\n', the whole sequence on one line, '\\n'"""
    return b"".join(b">" + n.encode() + b"\n" + apply_case(s, f) + b"\n" for n, s, f in zip(names, seqs, flags))


def revcomp(s):
    return bytes(s).translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1]
