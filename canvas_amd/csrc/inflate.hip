// canvas_bgzf_inflate: the BGZF blocks of a BAM inflated on the device, one wave64 per block, and canvas_bgzf_scan, the host walk that makes their descriptors.
//
// The decoder is inflate_block.hpp's, the one the host tests run under AddressSanitizer; this file adds the Io of a wave:
//   every lane runs the whole decoder on the same bits (symbols of one stream depend on each other: there is nothing to share out), so the tables a lane reads in LDS are
//   the ones it wrote itself, and the lanes only meet in the match copies, which are spread over them: out[pos + i] = out[pos - dist + i % dist], i = lane, lane + 64, ...
//   reads nothing the same copy writes, whether dist < n or not.
//   window  the block's output, at most 64 KiB, lives in LDS until the stream has ended well, and goes out in 16-byte stores (LDS index and destination address agree
//           mod 16).  The other choice, writing to d_dst as it decodes and reading matches back from global memory, would put a global round trip (well over a thousand
//           cycles at one wave's occupancy) into every match of a serial decode, against about a hundred for LDS; the 64 KiB + 5 KiB of tables and input window allow two
//           blocks per CU, 512 on the chip, which is what a 32 MB chunk has.  It also gives the containment rule for free: a failed block writes nothing.
//   input   a 1 KiB window of the stream in LDS, refilled by the 64 lanes with guarded byte loads (no byte outside [src_offset, src_offset + src_bytes) is read, whatever
//           the alignment), read by the bit reader as aligned 32-bit words.
// The only cross-lane traffic is through LDS, one wave per workgroup: __syncthreads() is the wave's own fence there.
#include "inflate_block.hpp"

#define INF_WINDOW_WORDS 256
struct InflateLds { InflateTables T; uint32_t in[INF_WINDOW_WORDS]; uint8_t out[65536 + 16] __attribute__((aligned(16))); };

struct InflateWaveIo {
    const uint8_t* __restrict__ src; uint32_t srcBytes; uint32_t* in; uint8_t* out; uint32_t winAt; uint32_t lane;      // in[] holds words winAt .. winAt + 255; out = the window's byte 0
    __device__ __forceinline__ uint32_t word(uint32_t k) {
        if (k - winAt >= INF_WINDOW_WORDS) {                          // the same for every lane
            __syncthreads();
            winAt = k;
            for (uint32_t j = lane; j < INF_WINDOW_WORDS; j += 64) {
                const uint64_t at = 4ull * (k + j); uint32_t w = 0;
                if (at + 4 <= srcBytes) w = bam_ld32(src, at);
                else for (uint32_t b = 0; b < 4; b++) if (at + b < srcBytes) w |= (uint32_t)src[at + b] << (8 * b);
                in[j] = w;
            }
            __syncthreads();
        }
        return in[k - winAt];
    }
    __device__ __forceinline__ void put(uint32_t pos, uint32_t byte) { if (lane == 0) out[pos] = (uint8_t)byte; }
    __device__ __forceinline__ void copy(uint32_t pos, uint32_t dist, uint32_t n) {
        __syncthreads();                                              // what other lanes have put or copied before
        const uint8_t* from = out + pos - dist;
        if (dist >= n) for (uint32_t i = lane; i < n; i += 64) out[pos + i] = from[i];
        else for (uint32_t i = lane; i < n; i += 64) out[pos + i] = from[i % dist];
    }
    __device__ __forceinline__ void stored(uint32_t pos, uint32_t at, uint32_t n) { for (uint32_t i = lane; i < n; i += 64) out[pos + i] = src[at + i]; }
};

static __global__ void __launch_bounds__(64) k_bgzf_inflate(const uint8_t* __restrict__ src, uint64_t srcNbytes, const canvas_bgzf_block* __restrict__ blocks, int64_t nblocks,
                                                            uint8_t* __restrict__ dst, uint64_t dstNbytes, int32_t* __restrict__ status) {
    __shared__ InflateLds S;
    const uint32_t lane = threadIdx.x;
    for (int64_t i = blockIdx.x; i < nblocks; i += gridDim.x) {
        const canvas_bgzf_block b = blocks[i];
        int32_t st = CANVAS_INFLATE_DESCRIPTOR;
        if (inflate_descriptor_ok(b, srcNbytes, dstNbytes)) {
            uint8_t* to = dst + b.dst_offset;
            const uint32_t skew = (uint32_t)((uintptr_t)to & 15u);
            InflateWaveIo io{src + b.src_offset, b.src_bytes, S.in, S.out + skew, 0xFFFFFF00u, lane};      // (no word of a stream is within 256 of winAt: the first read fills the window)
            st = inflate_stream(io, b.src_bytes, b.out_bytes, S.T);
            __syncthreads();
            if (st == CANVAS_INFLATE_OK) {
                const uint32_t n = b.out_bytes, align = (16u - skew) & 15u, head = align < n ? align : n, body = (n - head) & ~15u;      // bytes, 16-byte words, bytes
                for (uint32_t k = lane; k < head; k += 64) to[k] = io.out[k];
                for (uint32_t k = 16 * lane; k < body; k += 16 * 64) *(uint4*)(to + head + k) = *(const uint4*)(io.out + head + k);
                for (uint32_t k = head + body + lane; k < n; k += 64) to[k] = io.out[k];
            }
            __syncthreads();                                          // the next block of this wave reuses the LDS
        }
        if (lane == 0) status[i] = st;
    }
}

// [0] blocks, [1] failed, [2] bytes of the good ones, [3] the first failed one or -1
static __global__ void __launch_bounds__(256) k_bgzf_info(const canvas_bgzf_block* __restrict__ blocks, const int32_t* __restrict__ status, int64_t nblocks, unsigned long long* info) {
    __shared__ unsigned long long sFailed, sBytes, sFirst;
    if (threadIdx.x == 0) { sFailed = 0; sBytes = 0; sFirst = ~0ull; }
    __syncthreads();
    unsigned long long failed = 0, bytes = 0, first = ~0ull;
    for (int64_t i = threadIdx.x; i < nblocks; i += blockDim.x) {
        if (status[i] == CANVAS_INFLATE_OK) bytes += blocks[i].out_bytes;
        else { failed++; if (first == ~0ull) first = (unsigned long long)i; }
    }
    if (failed) { atomicAdd(&sFailed, failed); atomicMin(&sFirst, first); }
    if (bytes) atomicAdd(&sBytes, bytes);
    __syncthreads();
    if (threadIdx.x == 0) { info[0] = (unsigned long long)nblocks; info[1] = sFailed; info[2] = sBytes; info[3] = sFirst; }      // (~0 is -1)
}

extern "C" int32_t canvas_bgzf_inflate(canvas_ctx* ctx, const uint8_t* d_src, uint64_t src_nbytes, const canvas_bgzf_block* d_blocks, int64_t nblocks,
                                       uint8_t* d_dst, uint64_t dst_nbytes, int32_t* d_status, int64_t* h_info) {
    if (!ctx) return CANVAS_ERR_INVALID;
    if (nblocks < 0 || (nblocks > 0 && (!d_src || !d_blocks || !d_dst || !d_status))) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_bgzf_inflate: bad arguments");
    if (nblocks == 0) { if (h_info) { h_info[0] = h_info[1] = h_info[2] = 0; h_info[3] = -1; } return CANVAS_OK; }
    CANVAS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    unsigned long long* dInfo = nullptr;
    if (h_info) { int32_t rc = canvas_ws_reserve(ctx, 256); if (rc) return rc; dInfo = (unsigned long long*)ctx->ws; }
    {
        ProfScope ps(ctx, "bgzf_inflate", true);
        const unsigned grid = (unsigned)(nblocks < (int64_t)(1 << 20) ? nblocks : (int64_t)(1 << 20));
        hipLaunchKernelGGL(k_bgzf_inflate, dim3(grid), dim3(64), 0, ctx->stream, d_src, src_nbytes, d_blocks, nblocks, d_dst, dst_nbytes, d_status);
    }
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    if (!h_info) return CANVAS_OK;
    hipLaunchKernelGGL(k_bgzf_info, dim3(1), dim3(256), 0, ctx->stream, d_blocks, (const int32_t*)d_status, nblocks, dInfo);
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    return bam_mail_fetch(ctx, dInfo, 4, h_info, "canvas_bgzf_inflate");
}

extern "C" int32_t canvas_bgzf_scan(const uint8_t* h_bytes, uint64_t nbytes, uint64_t at, uint64_t max_out_bytes, canvas_bgzf_block* h_blocks, int64_t capacity, int64_t* h_info) {
    if (!h_info || (!h_bytes && nbytes > 0) || capacity < 0 || (!h_blocks && capacity > 0) || at > nbytes) return CANVAS_ERR_INVALID;
    bgzf_scan_blocks(h_bytes, nbytes, at, max_out_bytes, h_blocks, capacity, h_info);
    return CANVAS_OK;
}
