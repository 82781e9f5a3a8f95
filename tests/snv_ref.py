"""Plain Python restatement of CanvasSNV (CanvasSNV/SNVReviewer.cs) that the SNV tests compare against: LoadVariants, the read loop of ProcessBamFile WITH the
reference's scan pointer carried from read to read, ProcessReadBases base by base, IsVariantSite, GetBAlleleFrequency and the two writers — over a BGZF / BAM
reader and writer of its own (SAM specification 4.1-4.2: BGZF is a series of gzip members with a 'BC' extra subfield; a BAM record is a block_size word and
32 fixed bytes followed by name, CIGAR, 4-bit bases and qualities).  It shares no code with canvas_amd/.

The reference's VcfReader (Isas.SequencingFiles) is not part of the reference tree: records are read by the VCF specification (FORMAT keys zipped with the sample's
':'-separated values)."""
import gzip
import struct
import zlib
from decimal import Decimal

BASE_CODES = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"
MIN_BASE_Q = 20


# ---------------------------------------------------------------- BGZF
def bgzf_block(data):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    c = co.compress(bytes(data)) + co.flush()
    assert len(c) + 26 <= 65536
    return struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(c) + 25) + c + struct.pack("<II", zlib.crc32(bytes(data)) & 0xFFFFFFFF, len(data))


def bgzf_read_all(path):
    """the inflated stream of a BGZF file (member after member)"""
    raw = open(path, "rb").read()
    out = bytearray()
    at = 0
    while at < len(raw):
        assert raw[at:at + 4] == b"\x1f\x8b\x08\x04", "not a BGZF member at %d" % at
        xlen = struct.unpack_from("<H", raw, at + 10)[0]
        bsize = None
        x = at + 12
        while x < at + 12 + xlen:
            si1, si2, slen = struct.unpack_from("<BBH", raw, x)
            if (si1, si2, slen) == (66, 67, 2):
                bsize = struct.unpack_from("<H", raw, x + 4)[0]
            x += 4 + slen
        assert bsize is not None
        cdata = raw[at + 12 + xlen: at + bsize + 1 - 8]
        data = zlib.decompress(cdata, -15)
        crc, isize = struct.unpack_from("<II", raw, at + bsize + 1 - 8)
        assert isize == len(data) and crc == (zlib.crc32(data) & 0xFFFFFFFF)
        out += data
        at += bsize + 1
    return bytes(out)


# ---------------------------------------------------------------- BAM records
def encode_seq(bases):
    codes = [BASE_CODES.index(b) for b in bases]
    if len(codes) & 1:
        codes.append(0)
    return bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2))


def encode_record(r):
    """r: dict(ref, pos, flag, mapq, cigar=[(len, op)], seq='ACGT..', qual=[..]) (+ name, l_seq / n_cigar / l_read_name overrides for malformed records).
    Returns the record's bytes WITH its block_size word."""
    name = r.get("name", "r").encode() + b"\x00"
    cig = b"".join(struct.pack("<I", (ln << 4) | CIGAR_OPS.index(op)) for ln, op in r["cigar"])
    seq = r["seq"]
    qual = bytes(r["qual"]) if "qual" in r else bytes([30] * len(seq))
    assert len(qual) == len(seq)
    body = struct.pack("<iiBBHHHiiii", r["ref"], r["pos"], r.get("l_read_name", len(name)), r.get("mapq", 30), 4680, r.get("n_cigar", len(r["cigar"])), r.get("flag", 0),
                       r.get("l_seq", len(seq)), r.get("mate_ref", -1), r.get("mate_pos", -1), 0)
    body += name + cig + encode_seq(seq) + qual + bytes(r.get("tail", b""))
    return struct.pack("<i", r.get("block_size", len(body))) + body


def decode_record(buf, at):
    """the record at byte `at` of an inflated stream -> (dict, next offset)"""
    bs = struct.unpack_from("<i", buf, at)[0]
    ref, pos, lname, mapq, _bin, ncig, flag, lseq, mref, mpos, _tlen = struct.unpack_from("<iiBBHHHiiii", buf, at + 4)
    p = at + 36
    name = buf[p:p + lname - 1].decode("ascii", "replace")
    p += lname
    cigar = []
    for i in range(ncig):
        v = struct.unpack_from("<I", buf, p + 4 * i)[0]
        cigar.append((v >> 4, CIGAR_OPS[v & 15] if (v & 15) < len(CIGAR_OPS) else "?"))
    p += 4 * ncig
    packed = buf[p:p + (lseq + 1) // 2]
    seq = "".join(BASE_CODES[(packed[i >> 1] >> (0 if i & 1 else 4)) & 15] for i in range(lseq))
    p += (lseq + 1) // 2
    qual = list(buf[p:p + lseq])
    return dict(ref=ref, pos=pos, flag=flag, mapq=mapq, cigar=cigar, seq=seq, qual=qual, name=name), at + 4 + bs


def write_bam(path, refs, reads, cut=3000):
    """refs: [(name, length)]; reads sorted by (ref, pos), ref -1 last.  Every reference starts a BGZF block of its own (its virtual offset goes to the .bai);
    inside a reference the stream is cut every `cut` bytes, so records span blocks."""
    text = b"@HD\tVN:1.0\tSO:coordinate\n"
    hdr = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, ln in refs:
        nm = name.encode() + b"\x00"
        hdr += struct.pack("<i", len(nm)) + nm + struct.pack("<i", ln)
    out = bytearray(bgzf_block(hdr))
    first = {}
    by_ref = {}
    for r in reads:
        by_ref.setdefault(r["ref"], []).append(r)
    for ref in sorted(by_ref, key=lambda x: (x < 0, x)):
        data = b"".join(encode_record(r) for r in by_ref[ref])
        first[ref] = len(out) << 16
        for i in range(0, len(data), cut):
            out += bgzf_block(data[i:i + cut])
    end = len(out) << 16
    out += bgzf_block(b"")
    open(path, "wb").write(out)
    bai = b"BAI\x01" + struct.pack("<i", len(refs))
    for i in range(len(refs)):
        if i in first:
            bai += struct.pack("<i", 1) + struct.pack("<Ii", 0, 1) + struct.pack("<QQ", first[i], end) + struct.pack("<i", 0)
        else:
            bai += struct.pack("<i", 0) + struct.pack("<i", 0)
    open(path + ".bai", "wb").write(bai)


def bgzf_blocks(raw):
    """[(offset, size)] of the blocks of a BGZF file as bgzf_block writes them (BC is the first subfield)"""
    blocks, at = [], 0
    while at < len(raw):
        assert raw[at:at + 4] == b"\x1f\x8b\x08\x04" and raw[at + 12:at + 16] == b"BC\x02\x00"
        size = struct.unpack_from("<H", raw, at + 16)[0] + 1
        blocks.append((at, size)); at += size
    return blocks


def reblock_bam(src, dst):
    """The BAM `src` (and its .bai) written again as `dst` with the same inflated stream in another BGZF form: every block carries a subfield of its own in front of BC
    (XLEN 13 instead of 6), and an empty block (ISIZE 0) stands in the middle of the file.  The virtual offsets of the .bai move with their blocks."""
    raw = open(src, "rb").read()
    blocks = bgzf_blocks(raw)
    extra = b"XY" + struct.pack("<H", 3) + b"abc"

    def with_extra(block):
        return block[:10] + struct.pack("<H", len(extra) + 6) + extra + b"BC" + struct.pack("<HH", 2, len(block) + len(extra) - 1) + block[18:]
    out, moved = bytearray(), {}
    for i, (at, size) in enumerate(blocks):
        if i == len(blocks) // 2:
            out += with_extra(bgzf_block(b""))
        moved[at] = len(out)
        out += with_extra(raw[at:at + size])
    moved[len(raw)] = len(out)
    assert bgzf_read_all(src) == zlib_stream(bytes(out))
    open(dst, "wb").write(out)
    bai = open(src + ".bai", "rb").read()
    new, at = bytearray(bai[:8]), 8

    def copy(n):
        nonlocal at
        new.extend(bai[at:at + n]); at += n
        return struct.unpack_from("<i", bai, at - 4)[0]

    def offsets(n):
        nonlocal at
        for v in struct.unpack_from("<%dQ" % n, bai, at):
            new.extend(struct.pack("<Q", (moved[v >> 16] << 16) | (v & 0xFFFF)))
        at += 8 * n
    for _ in range(struct.unpack_from("<i", bai, 4)[0]):
        for _ in range(copy(4)):                   # n_bin
            offsets(2 * copy(8))                   # bin, n_chunk; chunk_beg, chunk_end
        offsets(copy(4))                           # n_intv; ioffset
    assert at == len(bai)
    open(dst + ".bai", "wb").write(new)


def zlib_stream(raw):
    """the inflated stream of BGZF bytes whose blocks may carry any subfields (zlib's own gzip reader, member after member)"""
    out = bytearray()
    while raw:
        d = zlib.decompressobj(31)
        out += d.decompress(raw)
        raw = d.unused_data
    return bytes(out)


def read_bam(path):
    """-> ([(name, length)], [record dict] in file order)"""
    buf = bgzf_read_all(path)
    assert buf[:4] == b"BAM\x01"
    ltext = struct.unpack_from("<i", buf, 4)[0]
    at = 8 + ltext
    nref = struct.unpack_from("<i", buf, at)[0]
    at += 4
    refs = []
    for _ in range(nref):
        ln = struct.unpack_from("<i", buf, at)[0]
        name = buf[at + 4:at + 4 + ln - 1].decode()
        refs.append((name, struct.unpack_from("<i", buf, at + 4 + ln)[0]))
        at += 8 + ln
    reads = []
    while at < len(buf):
        r, at = decode_record(buf, at)
        reads.append(r)
    return refs, reads


# ---------------------------------------------------------------- LoadVariants (SNVReviewer.cs:86-167, 367-398)
class Variant:
    def __init__(self, chrom, pos, ref, alts):
        self.chrom, self.pos, self.ref, self.alts = chrom, pos, ref, alts

    @property
    def alt(self):
        return self.alts[0]


def _open_text(path):
    with open(path, "rb") as f:
        magic = f.read(2)
    return gzip.open(path, "rt") if magic == b"\x1f\x8b" else open(path, "rt")


def load_variants(vcf_path, chromosome, sample_name="", is_dbsnp=False, is_somatic=False):
    variants = []
    count_this = 0
    samples = []
    checked = False
    sample_index = 0
    with _open_text(vcf_path) as f:
        for line in f:
            line = line.rstrip("\r\n")
            if not line:
                continue
            if line.startswith("#"):
                if line.startswith("#CHROM"):
                    samples = line.split("\t")[9:]
                continue
            if not checked:
                checked = True
                if sample_name and not is_dbsnp:
                    if sample_name not in samples:
                        raise ValueError("File '%s' should contain one genotypes column corresponding to sample %s" % (vcf_path, sample_name))
                    sample_index = samples.index(sample_name)
                elif len(samples) > 1:
                    raise ValueError("File '%s' contains >1 samples, name for a sample of interest must be provided" % vcf_path)
            c = line.split("\t")
            if c[0] != chromosome:
                if count_this > 0:
                    break
                continue
            count_this += 1
            ref, alts = c[3], c[4].split(",")
            if len(alts) != 1 or len(alts[0]) != 1 or len(ref) != 1:
                continue
            if len(c) > 9:
                keys = c[8].split(":")
                g = dict(zip(keys, c[9 + sample_index].split(":")))
                if not (c[6] == "PASS" and ("FT" not in g or g["FT"] == "PASS")):
                    continue
                if "GT" not in g:
                    continue
                het = g["GT"] in ("0/1", "1/0", "0|1", "1|0")
                if is_somatic:
                    if not het:
                        continue
                    if "GQX" in g and (g["GQX"] == "." or Decimal(g["GQX"]) < 30):
                        continue
                elif not (het or g["GT"] in ("1/1", "1|1")):
                    continue
            variants.append(Variant(c[0], int(c[1]), ref, alts))
    if not checked:      # no record at all: the sample checks still apply (the reference makes them when the reader is opened)
        if sample_name and not is_dbsnp:
            if sample_name not in samples:
                raise ValueError("File '%s' should contain one genotypes column corresponding to sample %s" % (vcf_path, sample_name))
        elif len(samples) > 1:
            raise ValueError("File '%s' contains >1 samples, name for a sample of interest must be provided" % vcf_path)
    return variants


# ---------------------------------------------------------------- ProcessBamFile / ProcessReadBases (SNVReviewer.cs:172-271)
def process_read_bases(read, variants, next_variant_index, ref_counts, alt_counts, min_base_q=MIN_BASE_Q):
    position = read["pos"]
    base_index = 0
    for length, op in read["cigar"]:
        if op == "M":
            for _ in range(length):
                var_index = next_variant_index
                while var_index < len(variants):
                    v = variants[var_index]
                    if v.pos - 1 > position:
                        break
                    if v.pos - 1 < position:
                        next_variant_index += 1
                        var_index += 1
                        continue
                    if read["qual"][base_index] >= min_base_q:
                        base = read["seq"][base_index]
                        if base == v.ref[0]:
                            ref_counts[var_index] += 1
                        if base == v.alts[0][0]:
                            alt_counts[var_index] += 1
                    var_index += 1
                position += 1
                base_index += 1
        elif op in ("S", "I"):
            base_index += length
        elif op == "D":
            position += length
        else:
            return


def pileup(reads, ref_id, variants, min_mapq=0, min_base_q=MIN_BASE_Q):
    """the read loop with the scan pointer carried from read to read; `reads` in file order, starting anywhere at or before the chromosome"""
    ref_counts = [0] * len(variants)
    alt_counts = [0] * len(variants)
    next_variant_index = 0
    for read in reads:
        if read["pos"] < 0 or read["ref"] < 0 or read["ref"] > ref_id:
            break
        if read["ref"] < ref_id:
            continue
        flag = read.get("flag", 0)
        if flag & 0x100 or flag & 0x4 or flag & 0x400:
            continue
        if read.get("mapq", 30) <= min_mapq:
            continue
        while next_variant_index < len(variants) and variants[next_variant_index].pos < read["pos"]:
            next_variant_index += 1
        if next_variant_index >= len(variants):
            break
        if read["pos"] + 1000 < variants[next_variant_index].pos:
            continue
        process_read_bases(read, variants, next_variant_index, ref_counts, alt_counts, min_base_q)
    return ref_counts, alt_counts


# ---------------------------------------------------------------- results (SNVReviewer.cs:74-81, 276-365)
def is_variant_site(ref_count, alt_count, is_dbsnp):
    if ref_count + alt_count == 0:
        return False
    if is_dbsnp and alt_count == 0:
        return False
    return True


def _b_allele_preference(allele):
    try:
        return {"a": 0, "t": 1, "g": 2, "c": 3}[allele.lower()]
    except KeyError:
        raise ValueError("Invalid single nucleotide allele: " + allele)


def b_allele_frequency(ref, alt, ref_count, alt_count):
    total = float(ref_count + alt_count)
    if total < 1:
        return None
    if ref == "." or alt == ".":
        return None
    if _b_allele_preference(ref) < _b_allele_preference(alt):
        return ref_count / total
    return alt_count / total


def format_g15(v):
    """double.ToString() of .NET Core 2.x: 15 significant digits, trailing zeros dropped, scientific when the exponent is >= 15 or < -4 (0.0001 but 1E-05)"""
    if v == 0:
        return "0"
    mant, exp = ("%.14e" % abs(v)).split("e")
    digits = mant.replace(".", "").rstrip("0") or "0"
    e10 = int(exp)
    sign = "-" if v < 0 else ""
    if e10 >= 15 or e10 < -4:
        return sign + digits[0] + ("." + digits[1:] if len(digits) > 1 else "") + "E%s%02d" % ("-" if e10 < 0 else "+", abs(e10))
    if e10 < 0:
        return sign + "0." + "0" * (-e10 - 1) + digits
    if len(digits) <= e10 + 1:
        return sign + digits + "0" * (e10 + 1 - len(digits))
    return sign + digits[:e10 + 1] + "." + digits[e10 + 1:]


def result_texts(variants, ref_counts, alt_counts, is_dbsnp=False):
    """-> (text of <out> before gzip, text of <out>.baf)"""
    rows = ["#Chromosome\tPosition\tRef\tAlt\tCountRef\tCountAlt"]
    baf = ["Chromosome,Position,BAF"]
    for v, rc, ac in zip(variants, ref_counts, alt_counts):
        if not is_variant_site(rc, ac, is_dbsnp):
            continue
        rows.append("%s\t%d\t%s\t%s\t%d\t%d" % (v.chrom, v.pos, v.ref, v.alt, rc, ac))
        f = b_allele_frequency(v.ref, v.alt, rc, ac)
        if f is not None:
            baf.append("%s,%d,%s" % (v.chrom, v.pos, format_g15(f)))
    return "\n".join(rows) + "\n", "\n".join(baf) + "\n"


def run(vcf_path, bam_path, chromosome, sample_name="", is_dbsnp=False, min_mapq=0, is_somatic=False):
    """CanvasSNV end to end -> (counts text, baf text)"""
    variants = load_variants(vcf_path, chromosome, sample_name, is_dbsnp, is_somatic)
    refs, reads = read_bam(bam_path)
    names = [n for n, _ in refs]
    if chromosome not in names:
        raise ValueError("Error: Chromosome name '%s' does not match bam file at '%s'" % (chromosome, bam_path))
    rc, ac = pileup(reads, names.index(chromosome), variants, min_mapq)
    return result_texts(variants, rc, ac, is_dbsnp)
