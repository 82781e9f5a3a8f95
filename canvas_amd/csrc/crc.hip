// canvas_bgzf_crc32: the CRC32 of every inflated BGZF block summed on the device and held against the word of the block's trailer, one workgroup of four waves per block.
//
// The arithmetic is crc32_block.hpp's, the one the host tests run under AddressSanitizer; this file adds how a workgroup shares a block out:
//   loading  the block (at most 64 KiB, at any byte offset of d_dst) comes into LDS once, in 16-byte loads that every lane of a wave issues side by side (LDS index and
//            source address agree mod 16; the bytes in front of and behind the 16-byte words singly): each byte crosses the memory system once, in full lines.  The
//            other choice, every lane reading its own slice from global memory, has the 64 lanes of a load touch 64 different lines for 16 bytes each.
//   slices   lane t sums bytes [260 t, 260 t + 260) from LDS, four bytes a step through four 256-entry tables (the four look-ups of a step do not wait for each other;
//            one table would put an LDS round trip into every byte).  260 bytes are 65 words, an odd count: byte and word reads are served in groups of 32 lanes over
//            32 banks, and at every step the 32 lanes of a group read 32 different banks, whatever the block's skew.  The tables (4 KiB) are one copy per workgroup:
//            their look-ups are indexed by data and do collide, a few ways per step, which is cheaper than the 32 KiB a copy per bank would take: with them a CU
//            would hold one workgroup instead of two.
//   joining  every lane moves its sum to the block's end (times x^(8 * bytes behind the slice), up to 17 multiply-reduce steps of 32 shifts), the sums are xor-ed in the
//            wave by lane exchange and across the four waves through four LDS words, and lane 0 adds the preset's term, inverts, compares and writes.
// 64 KiB + 16 of data, 4 KiB of tables: two workgroups per CU.  A block moves out_bytes + 24 (descriptor) + 4 (trailer) + 4 (the inflater's status) bytes in and 8 out.
#include "crc32_block.hpp"

#define CRC_THREADS 256
struct CrcLds { uint32_t T[CRC32_TABLE_WORDS]; uint32_t part[CRC_THREADS / 64]; uint8_t data[65536 + 16] __attribute__((aligned(16))); };
static_assert(CRC_THREADS * CRC32_SLICE_BYTES >= 65536u, "every byte of a block has a lane");

static __global__ void __launch_bounds__(CRC_THREADS) k_bgzf_crc32(const uint8_t* __restrict__ src, uint64_t srcNbytes, const canvas_bgzf_block* __restrict__ blocks, int64_t nblocks,
                                                                  const uint8_t* __restrict__ dst, uint64_t dstNbytes, const int32_t* __restrict__ inflateStatus,
                                                                  uint32_t* __restrict__ crc, int32_t* __restrict__ status) {
    __shared__ CrcLds S;
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = tid; k < CRC32_TABLE_WORDS; k += CRC_THREADS) S.T[k] = crc32_table_entry(k >> 8, k & 255u);
    __syncthreads();
    for (int64_t i = blockIdx.x; i < nblocks; i += gridDim.x) {      // (everything that decides a branch below is the same for the whole workgroup)
        const canvas_bgzf_block b = blocks[i];
        int32_t st = CANVAS_CRC_SKIPPED; uint32_t value = 0;
        if (!inflateStatus || inflateStatus[i] == 0) {
            st = CANVAS_CRC_DESCRIPTOR;
            if (crc32_descriptor_ok(b, dstNbytes, src != nullptr, srcNbytes)) {
                const uint8_t* from = dst + b.dst_offset;
                const uint32_t skew = (uint32_t)((uintptr_t)from & 15u);
                uint8_t* in = S.data + skew;
                const uint32_t n = b.out_bytes, align = (16u - skew) & 15u, head = align < n ? align : n, body = (n - head) & ~15u;      // bytes, 16-byte words, bytes
                for (uint32_t k = tid; k < head; k += CRC_THREADS) in[k] = from[k];
                for (uint32_t k = 16 * tid; k < body; k += 16 * CRC_THREADS) *(uint4*)(in + head + k) = *(const uint4*)(from + head + k);
                for (uint32_t k = head + body + tid; k < n; k += CRC_THREADS) in[k] = from[k];
                __syncthreads();
                uint32_t term = crc32_slice_term(in, n, tid, CRC32_SLICE_BYTES, S.T);
                for (int o = 32; o > 0; o >>= 1) term ^= (uint32_t)__shfl_xor((int)term, o, 64);
                if ((tid & 63u) == 0) S.part[tid >> 6] = term;
                __syncthreads();
                if (tid == 0) {
                    uint32_t terms = 0;
                    for (uint32_t w = 0; w < CRC_THREADS / 64; w++) terms ^= S.part[w];
                    value = crc32_finish(terms, n);
                    st = !src || bam_ld32(src, b.src_offset + b.src_bytes) == value ? CANVAS_CRC_OK : CANVAS_CRC_MISMATCH;
                }
                __syncthreads();                                      // the next block of this workgroup reuses the LDS
            }
        }
        if (tid == 0) { crc[i] = value; status[i] = st; }
    }
}

// [0] blocks, [1] those neither OK nor SKIPPED, [2] bytes summed (the OK and the MISMATCH ones), [3] the first of [1] or -1
static __global__ void __launch_bounds__(256) k_crc_info(const canvas_bgzf_block* __restrict__ blocks, const int32_t* __restrict__ status, int64_t nblocks, unsigned long long* info) {
    __shared__ unsigned long long sFailed, sBytes, sFirst;
    if (threadIdx.x == 0) { sFailed = 0; sBytes = 0; sFirst = ~0ull; }
    __syncthreads();
    unsigned long long failed = 0, bytes = 0, first = ~0ull;
    for (int64_t i = threadIdx.x; i < nblocks; i += blockDim.x) {
        const int32_t st = status[i];
        if (st == CANVAS_CRC_OK || st == CANVAS_CRC_MISMATCH) bytes += blocks[i].out_bytes;
        if (st != CANVAS_CRC_OK && st != CANVAS_CRC_SKIPPED) { failed++; if (first == ~0ull) first = (unsigned long long)i; }
    }
    if (failed) { atomicAdd(&sFailed, failed); atomicMin(&sFirst, first); }
    if (bytes) atomicAdd(&sBytes, bytes);
    __syncthreads();
    if (threadIdx.x == 0) { info[0] = (unsigned long long)nblocks; info[1] = sFailed; info[2] = sBytes; info[3] = sFirst; }      // (~0 is -1)
}

extern "C" int32_t canvas_bgzf_crc32(canvas_ctx* ctx, const uint8_t* d_src, uint64_t src_nbytes, const canvas_bgzf_block* d_blocks, int64_t nblocks,
                                     const uint8_t* d_dst, uint64_t dst_nbytes, const int32_t* d_inflate_status, uint32_t* d_crc, int32_t* d_status, int64_t* h_info) {
    if (!ctx) return CANVAS_ERR_INVALID;
    if (nblocks < 0 || (nblocks > 0 && (!d_blocks || !d_dst || !d_crc || !d_status))) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_bgzf_crc32: bad arguments");
    if (nblocks == 0) { if (h_info) { h_info[0] = h_info[1] = h_info[2] = 0; h_info[3] = -1; } return CANVAS_OK; }
    CANVAS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    unsigned long long* dInfo = nullptr;
    if (h_info) { int32_t rc = cvx_ws_carve(ctx, 0, [&](WsCarver& cv) { cv.take(dInfo, 4); }); if (rc) return rc; }
    {
        ProfScope ps(ctx, "bgzf_crc32", true);
        const unsigned grid = (unsigned)(nblocks < (int64_t)(1 << 20) ? nblocks : (int64_t)(1 << 20));
        hipLaunchKernelGGL(k_bgzf_crc32, dim3(grid), dim3(CRC_THREADS), 0, ctx->stream, d_src, src_nbytes, d_blocks, nblocks, d_dst, dst_nbytes, d_inflate_status, d_crc, d_status);
    }
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    if (!h_info) return CANVAS_OK;
    hipLaunchKernelGGL(k_crc_info, dim3(1), dim3(256), 0, ctx->stream, d_blocks, (const int32_t*)d_status, nblocks, dInfo);
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    return bam_mail_fetch(ctx, dInfo, 4, h_info, "canvas_bgzf_crc32");
}
