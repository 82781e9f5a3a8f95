// One decoder for the BAM alignment records that snv.hip, obs.hip and frag.hip read, and what their entry points share around it.
//
// The chunk format of the three: `nbytes` of RAW record bytes (what the host inflated out of BGZF blocks, nothing of a record decoded) and a list of 64-bit offsets, one
// per record, each pointing at the record's block_size word.  A record starts at any address, so every field is put together from byte loads.
// Every offset formed is checked first: a hostile chunk cannot make a kernel read outside [rec, rec + nbytes).  bam_rec_load checks the offset, then the record's shape
// against its own and the chunk's length; behind a `true` the name and the CIGAR lie inside the chunk, and behind bam_rec_holds_seq the bases and qualities as well.
// tests/test_bam_record_host.py runs this part on the host under AddressSanitizer, on chunks with no byte of padding behind them.
//
// The decode part is plain C++ and needs <cstdint> only; the part under __HIPCC__ (the stop key, the block reduction, the mailbox tail) needs common.hpp.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include "common.hpp"
#define BAM_FN __host__ __device__ __forceinline__
#else
#define BAM_FN inline
#endif

BAM_FN uint32_t bam_ld8(const uint8_t* __restrict__ p, uint64_t at) { return p[at]; }
BAM_FN uint32_t bam_ld16(const uint8_t* __restrict__ p, uint64_t at) { return (uint32_t)p[at] | ((uint32_t)p[at + 1] << 8); }
BAM_FN uint32_t bam_ld32(const uint8_t* __restrict__ p, uint64_t at) {
    return (uint32_t)p[at] | ((uint32_t)p[at + 1] << 8) | ((uint32_t)p[at + 2] << 16) | ((uint32_t)p[at + 3] << 24);
}

// block_size and the 32 fixed bytes behind it (bytes 0-35 from the record's offset; the 16 bits of `bin` at byte 14 are not kept)
struct BamRec { int32_t block_size, refID, pos; uint32_t l_read_name, mapq, n_cigar_op, flag; int32_t l_seq, next_refID, next_pos, tlen; };

// false: `off` leaves no 36 bytes inside the chunk (b is not written), or block_size does not hold the fixed fields, the name and the CIGAR, or it ends behind the chunk
BAM_FN bool bam_rec_load(const uint8_t* __restrict__ rec, uint64_t nbytes, uint64_t off, BamRec& b) {
    if (off > nbytes || nbytes - off < 36) return false;                 // block_size + the 32 fixed bytes
    // every fixed field is requested before the first decision (a load under a condition is waited for where the condition ends)
    b.block_size = (int32_t)bam_ld32(rec, off); b.refID = (int32_t)bam_ld32(rec, off + 4); b.pos = (int32_t)bam_ld32(rec, off + 8);
    b.l_read_name = bam_ld8(rec, off + 12); b.mapq = bam_ld8(rec, off + 13); b.n_cigar_op = bam_ld16(rec, off + 16); b.flag = bam_ld16(rec, off + 18);
    b.l_seq = (int32_t)bam_ld32(rec, off + 20); b.next_refID = (int32_t)bam_ld32(rec, off + 24); b.next_pos = (int32_t)bam_ld32(rec, off + 28); b.tlen = (int32_t)bam_ld32(rec, off + 32);
    const uint64_t bs = (uint32_t)b.block_size;
    return !(b.block_size < 32 || bs > nbytes - off - 4 || 32ull + b.l_read_name + 4ull * b.n_cigar_op > bs);
}
// ... and the bases and qualities lie inside block_size as well (CanvasSNV's stricter rule; b passed bam_rec_load)
BAM_FN bool bam_rec_holds_seq(const BamRec& b) {
    return b.l_seq >= 0 && 32ull + b.l_read_name + 4ull * b.n_cigar_op + ((uint64_t)b.l_seq + 1) / 2 + (uint64_t)b.l_seq <= (uint64_t)b.block_size;
}
// where the variable parts of a well-formed record at `off` start: l_read_name bytes of name (with its NUL), n_cigar_op words, (l_seq + 1) / 2 bytes of bases, l_seq qualities
BAM_FN uint64_t bam_name_at(uint64_t off) { return off + 36; }
BAM_FN uint64_t bam_cigar_at(uint64_t off, uint32_t l_read_name) { return off + 36 + l_read_name; }
BAM_FN uint64_t bam_seq_at(uint64_t off, uint32_t l_read_name, uint32_t n_cigar_op) { return bam_cigar_at(off, l_read_name) + 4ull * n_cigar_op; }
BAM_FN uint64_t bam_qual_at(uint64_t off, uint32_t l_read_name, uint32_t n_cigar_op, int32_t l_seq) { return bam_seq_at(off, l_read_name, n_cigar_op) + ((uint64_t)l_seq + 1) / 2; }

#if defined(__HIPCC__)
// ---- the first record of a chunk that carries some flag, as one 64-bit word: (epoch << 32) | (0xFFFFFFFF - index), raised with atomicMax.  The smallest index of the newest
// epoch wins, a zeroed word means "none", and a word of an older epoch "in an earlier chunk" — no launch or fill resets it between chunks.  Epochs are never 0.
__device__ __forceinline__ unsigned long long bam_stop_key(uint32_t epoch, int64_t index) { return ((unsigned long long)epoch << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)index); }
__device__ __forceinline__ int64_t bam_stop_index(unsigned long long key) { return (int64_t)(0xFFFFFFFFu - (uint32_t)key); }
__device__ __forceinline__ bool bam_stopped_before(unsigned long long key, uint32_t epoch) { return key != 0ull && (uint32_t)(key >> 32) != epoch; }

// the smallest threadIdx.x of the workgroup whose flag is set, -1 when there is none; every thread calls it and gets the answer: a ballot inside the wave, one word of LDS
// per wave, one barrier.  sWave is not to be touched again before the workgroup's next barrier.
template <int WAVES> __device__ __forceinline__ int bam_block_first(bool flag, int32_t (&sWave)[WAVES]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) sWave[wave] = m ? wave * WAVE + __ffsll((long long)m) - 1 : -1;
    __syncthreads();
    int first = -1;
    for (int w = WAVES - 1; w >= 0; w--) if (sWave[w] >= 0) first = sWave[w];
    return first;
}

// ---- the mailbox tail: n 64-bit state words travel through the context's pinned mailbox (common.hpp: payload, system fence, sequence word last)
static __global__ void k_bam_mail(const unsigned long long* __restrict__ words, int n, long long* pin, unsigned* seqWord, unsigned seq) {
    if ((int)threadIdx.x < n) pin[threadIdx.x] = (long long)words[threadIdx.x];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) cvx_mail_publish(seqWord, seq);
}
// d_words[0 .. n) (n <= 64), as they stand once everything enqueued on the stream has run, into h_info; the call waits.  `who` names the entry point in the await message.
static inline int32_t bam_mail_fetch(canvas_ctx* ctx, const unsigned long long* d_words, int n, int64_t* h_info, const char* who) {
    int32_t rc = canvas_pin_reserve(ctx, ((size_t)n + 1) * 8); if (rc) return rc;
    long long* pin = (long long*)ctx->pin; unsigned* seqWord = (unsigned*)(pin + n);
    const unsigned seq = cvx_mail_arm(ctx, seqWord);
    hipLaunchKernelGGL(k_bam_mail, dim3(1), dim3(64), 0, ctx->stream, d_words, n, pin, seqWord, seq);
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    rc = cvx_mail_await(ctx, seqWord, seq, who); if (rc) return rc;
    for (int i = 0; i < n; i++) h_info[i] = pin[i];
    return CANVAS_OK;
}
#endif
