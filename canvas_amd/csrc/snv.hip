// CanvasSNV's pileup: SNVReviewer.ProcessBamFile + ProcessReadBases (CanvasSNV/SNVReviewer.cs:172-271) over RAW BAM record bytes.
//
// The host (tools/canvas_snv_main.cpp) inflates BGZF blocks and finds where each record starts; nothing of a record is decoded there.  One lane takes one record:
//   1. the fixed fields and the shape checks against the record's and the chunk's length (bam_record.hpp: bam_rec_load, and bam_rec_holds_seq for the bases and
//      qualities); the read filters (:200-203);
//   2. k = first site with pos1 >= pos (the reference's scan pointer, :206, found by bisection: per read, needs no state from the read before as long as reads and
//      sites are sorted); no such site or pos + 1000 < pos1[k] (:213) -> the lane is done.  That is where most lanes leave: 24 bytes + ~log2(nsites) site words;
//   3. the survivors are compacted within the workgroup (LDS list), so that the waves that walk CIGARs are full and the others retire;
//   4. the walk: M consumes reference and read, S / I the read, D the reference, anything else ends it (:266-268).  Sites inside an M run are visited through the
//      sorted site list, never base by base; a site's base index comes from the run's start.  Quality >= min_base_q, then the 4-bit base code against the site's two
//      allele codes (the codes of the characters the reference compares, 0xFF for a character no base decodes to): one device atomic per match.
// Expected to be bound by the latency of the dependent loads (offset -> fixed fields -> bisection steps), with HBM traffic limited to the sectors those 24 bytes touch:
// an expectation from the access pattern, to be held against tools/snv_probe.py's figures, not a measurement.  A walking lane reads its CIGAR words
// twice (the pre-pass that rejects a CIGAR outrunning l_seq, then the walk): nothing for short reads, a second pass over up to 65 535 words for a long read's CIGAR.
// Byte loads, offsets and their checks are bam_record.hpp's.  Loops are bounded by n_cigar_op (16 bits) and by the sites inside one M run.  Statistics are reduced per
// workgroup (LDS) before they reach the five global words.
#include "bam_record.hpp"

#define SNV_BLOCK 256
enum { SNV_SEEN = 0, SNV_PASSED = 1, SNV_WALKED = 2, SNV_STOPPED = 3, SNV_MALFORMED = 4, SNV_NINFO = 5 };

struct SnvWork { uint64_t off; int32_t pos; int32_t k; uint32_t lname_ncig; int32_t lseq; };      // a record that has a site in reach

__global__ void __launch_bounds__(SNV_BLOCK) k_snv_count(const uint8_t* __restrict__ rec, uint64_t nbytes, const uint64_t* __restrict__ offs, int64_t nrec, int32_t refId,
                                                         int32_t minMapq, int32_t minBaseQ, const int32_t* __restrict__ sitePos, const uint8_t* __restrict__ siteRef,
                                                         const uint8_t* __restrict__ siteAlt, int32_t nsites, int32_t* __restrict__ refCnt, int32_t* __restrict__ altCnt,
                                                         unsigned long long* __restrict__ info) {
    __shared__ SnvWork work[SNV_BLOCK];
    __shared__ uint32_t sStat[SNV_NINFO];
    __shared__ uint32_t sWork;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < SNV_NINFO) sStat[tid] = 0;
    if (tid == 0) sWork = 0;
    __syncthreads();

    const int64_t r = (int64_t)blockIdx.x * SNV_BLOCK + tid;
    bool seen = r < nrec, malformed = false, passed = false, survive = false;
    SnvWork w; w.off = 0; w.pos = 0; w.k = 0; w.lname_ncig = 0; w.lseq = 0;
    if (seen) {
        const uint64_t off = offs[r]; BamRec b;
        if (!bam_rec_load(rec, nbytes, off, b) || !bam_rec_holds_seq(b)) malformed = true;
        else if (b.refID == refId && b.pos >= 0 && !(b.flag & (0x100u | 0x4u | 0x400u)) && (int32_t)b.mapq > minMapq) {
            passed = true;
            const int32_t p = b.pos;
            int lo = 0, hi = nsites;                                      // first site with pos1 >= p
            while (lo < hi) { const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1); if (sitePos[mid] < p) lo = mid + 1; else hi = mid; }
            if (lo < nsites && !((int64_t)p + 1000 < (int64_t)sitePos[lo])) {
                survive = true;
                w.off = off; w.pos = p; w.k = lo; w.lname_ncig = b.l_read_name | (b.n_cigar_op << 8); w.lseq = b.l_seq;
            }
        }
    }
    // ---- statistics of this phase and the compaction of the survivors: one LDS atomic per wave and counter
    {
        const unsigned long long mSeen = __ballot(seen), mPass = __ballot(passed), mSurv = __ballot(survive), mBad = __ballot(malformed);
        uint32_t base = 0;
        if (lane == 0) {
            if (mSeen) atomicAdd(&sStat[SNV_SEEN], (uint32_t)__popcll(mSeen));
            if (mPass) atomicAdd(&sStat[SNV_PASSED], (uint32_t)__popcll(mPass));
            if (mBad) atomicAdd(&sStat[SNV_MALFORMED], (uint32_t)__popcll(mBad));
            if (mSurv) base = atomicAdd(&sWork, (uint32_t)__popcll(mSurv));
        }
        base = __shfl(base, 0, 64);
        if (survive) work[base + (uint32_t)__popcll(mSurv & ((1ull << lane) - 1ull))] = w;
    }
    __syncthreads();
    const uint32_t nwork = sWork;                                        // <= SNV_BLOCK
    if (tid < (int)nwork) {
        const SnvWork W = work[tid];
        const uint32_t lname = W.lname_ncig & 0xFFu, ncig = W.lname_ncig >> 8;
        const uint64_t cigAt = bam_cigar_at(W.off, lname), seqAt = bam_seq_at(W.off, lname, ncig), qualAt = bam_qual_at(W.off, lname, ncig, W.lseq);       // all inside the record (checked above)
        // the read bases the walk would consume up to its end must exist: a record whose CIGAR outruns l_seq is rejected whole
        int64_t consumed = 0; bool stopped = false;
        for (uint32_t i = 0; i < ncig; i++) {
            const uint32_t c = bam_ld32(rec, cigAt + 4ull * i), op = c & 15u;
            if (op == 0u || op == 1u || op == 4u) consumed += (int64_t)(c >> 4);
            else if (op != 2u) { stopped = true; break; }
        }
        if (consumed > (int64_t)W.lseq) atomicAdd(&sStat[SNV_MALFORMED], 1u);
        else {
            atomicAdd(&sStat[SNV_WALKED], 1u);
            if (stopped) atomicAdd(&sStat[SNV_STOPPED], 1u);
            int64_t refPos = W.pos, baseIndex = 0; int s = W.k;
            for (uint32_t i = 0; i < ncig && s < nsites; i++) {
                const uint32_t c = bam_ld32(rec, cigAt + 4ull * i), op = c & 15u; const int64_t len = (int64_t)(c >> 4);
                if (op == 0u) {
                    while (s < nsites && (int64_t)sitePos[s] - 1 < refPos) s++;
                    while (s < nsites) {
                        const int64_t x = (int64_t)sitePos[s] - 1;
                        if (x >= refPos + len) break;
                        const int64_t b = baseIndex + (x - refPos);             // < consumed <= l_seq
                        if ((int32_t)bam_ld8(rec, qualAt + (uint64_t)b) >= minBaseQ) {
                            const uint32_t two = bam_ld8(rec, seqAt + (uint64_t)(b >> 1)), nib = (b & 1) ? (two & 15u) : (two >> 4);
                            if (nib == (uint32_t)siteRef[s]) atomicAdd(&refCnt[s], 1);
                            if (nib == (uint32_t)siteAlt[s]) atomicAdd(&altCnt[s], 1);
                        }
                        s++;
                    }
                    refPos += len; baseIndex += len;
                } else if (op == 1u || op == 4u) baseIndex += len;
                else if (op == 2u) refPos += len;
                else break;
            }
        }
    }
    __syncthreads();
    if (tid < SNV_NINFO && sStat[tid]) atomicAdd(&info[tid], (unsigned long long)sStat[tid]);
}

extern "C" int32_t canvas_snv_count(canvas_ctx* ctx, const uint8_t* d_records, uint64_t nbytes, const uint64_t* d_record_offsets, int64_t nrecords, int32_t ref_id, int32_t min_mapq,
                                    int32_t min_base_q, const int32_t* d_site_pos, const uint8_t* d_site_ref, const uint8_t* d_site_alt, int32_t nsites, int32_t* d_ref_counts,
                                    int32_t* d_alt_counts, int64_t* h_info) {
    if (!ctx) return CANVAS_ERR_INVALID;
    if (nrecords < 0 || nsites < 0 || (nrecords > 0 && (!d_records || !d_record_offsets)) || (nsites > 0 && (!d_site_pos || !d_site_ref || !d_site_alt || !d_ref_counts || !d_alt_counts)))
        CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_snv_count: bad arguments");
    if (nrecords > (int64_t)0x7FFFFFFF * SNV_BLOCK) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_snv_count: too many records in one chunk");
    CANVAS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (h_info) for (int i = 0; i < SNV_NINFO; i++) h_info[i] = 0;
    if (nrecords == 0) return CANVAS_OK;
    int32_t rc = canvas_ws_reserve(ctx, 4096); if (rc) return rc;
    unsigned long long* dInfo = (unsigned long long*)ctx->ws;
    CANVAS_HIP_TRY(ctx, hipMemsetAsync(dInfo, 0, SNV_NINFO * sizeof(unsigned long long), ctx->stream));
    {
        ProfScope ps(ctx, "snv_count", true);
        hipLaunchKernelGGL(k_snv_count, dim3((unsigned)((nrecords + SNV_BLOCK - 1) / SNV_BLOCK)), dim3(SNV_BLOCK), 0, ctx->stream, d_records, nbytes, d_record_offsets, nrecords, ref_id,
                           min_mapq, min_base_q, d_site_pos, d_site_ref, d_site_alt, nsites, d_ref_counts, d_alt_counts, dInfo);
    }
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    if (!h_info) return CANVAS_OK;                        // asynchronous: the counters are complete once the stream has been waited for
    return bam_mail_fetch(ctx, dInfo, SNV_NINFO, h_info, "canvas_snv_count");      // the call's statistics, through the pinned mailbox
}
