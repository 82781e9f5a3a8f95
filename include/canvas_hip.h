/* canvas_hip.h — C ABI of libcanvas_hip.so: the MI355X (gfx950) implementation of Canvas's read-depth hot path
 * (CanvasBin merge step -> CanvasClean -> CanvasPartition).
 *
 * The reference (Illumina/canvas, C#) has no in-process FFI for this path: its boundary is three executables that
 * exchange gzip text files.  This header is the boundary a thin C# `Main` P/Invokes instead of running
 * the C# loops; each entry point names the reference code it replaces (paths relative to Src/Canvas/).
 * INTEGRATION.md shows the DllImport stubs.
 *
 * Conventions
 *   - plain C, no exceptions cross the boundary; every function returns int32 status: 0 = ok, <0 = CANVAS_ERR_*;
 *     the message is available from canvas_last_error(ctx).
 *   - "d_" pointers are DEVICE pointers (from canvas_device_malloc or any HIP allocation of the same process);
 *     "h_" pointers are host pointers.  The library never frees or retains caller memory past the call.
 *   - one context = one GPU + one HIP stream; calls on a context are serialized by the caller.
 *   - alignment: d_bases / d_hits 16 bytes, d_mask 8 bytes and padded to a multiple of 8 bytes.
 *   - possible-alignment mask layout = System.Collections.BitArray: bit i of the chromosome is bit (i & 7) of byte i >> 3.
 */
#ifndef CANVAS_HIP_H
#define CANVAS_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct canvas_ctx canvas_ctx;

enum {
    CANVAS_OK = 0,
    CANVAS_ERR_INVALID = -1,     /* bad argument */
    CANVAS_ERR_HIP = -2,         /* HIP runtime error (no device, launch failure, OOM) */
    CANVAS_ERR_UNSUPPORTED = -3, /* reference feature outside the built scope */
    CANVAS_ERR_CAPACITY = -4,    /* caller buffer too small */
    CANVAS_ERR_COMM = -5         /* RCCL error */
};

/* coverage modes: CanvasCommon/Utilities.cs:56-74 (ParseCanvasCoverageMode) */
enum { CANVAS_MODE_BINARY = 0, CANVAS_MODE_TRUNCATED_DYNAMIC_RANGE = 3, CANVAS_MODE_GC_CONTENT_WEIGHTED = 5 };

/* CanvasClean switches: CanvasClean/CanvasClean.cs:431-446 (-g, -s, -r, --local-sd-metric-file, -m LOESS) */
enum { CANVAS_CLEAN_GCNORM = 1, CANVAS_CLEAN_FILTSIZE = 2, CANVAS_CLEAN_OUTLIERS = 4, CANVAS_CLEAN_LOCALSD = 8, CANVAS_CLEAN_LOESS = 16 };

/* ---- context ------------------------------------------------------------------------------------------------- */
canvas_ctx* canvas_create(int device);                 /* NULL when no usable GPU (the product has no CPU fallback) */
void canvas_destroy(canvas_ctx* ctx);
const char* canvas_last_error(canvas_ctx* ctx);
const char* canvas_version(void);
/* Process-wide counters of the results that kernels write straight into pinned host memory (bin size and totals of CanvasBin, quartiles and segment count of
 * CanvasPartition, Wavelets reports ...).  Each carries a sequence word that the kernel stores last (system-scope release) and the host checks after its synchronisation:
 * h_out2[0] = results looked at, h_out2[1] = looks that came before the result had arrived, after which the library polled the word until it did (0 on a quiet system;
 * a synchronisation that returns early was observed about once in eight process starts in round 4).  No reference counterpart. */
int32_t canvas_stale_reads(int64_t* h_out2);
int32_t canvas_set_stream(canvas_ctx* ctx, void* hip_stream); /* run on a caller-owned hipStream_t (NULL = own stream) */
/* A hint, never a change of results: the host makes ONE call per method with this context and then exits (the reference launches CanvasBin / CanvasClean / CanvasPartition as
 * one OS process per sample, Canvas/CanvasRunner.cs:123-128).  The library then uploads from the caller's pageable arrays where it would otherwise stage through pinned host
 * memory of its own: pinning costs ~1.4 ms per MB and the same again when the process leaves, which a second call would amortise and a one-shot process cannot. */
int32_t canvas_set_one_shot(canvas_ctx* ctx, int32_t on);
int32_t canvas_synchronize(canvas_ctx* ctx);
void* canvas_device_malloc(canvas_ctx* ctx, int64_t bytes);
int32_t canvas_device_free(canvas_ctx* ctx, void* d_ptr);
int32_t canvas_memcpy_h2d(canvas_ctx* ctx, void* d_dst, const void* h_src, int64_t bytes);
int32_t canvas_memcpy_d2h(canvas_ctx* ctx, void* h_dst, const void* d_src, int64_t bytes);
/* canvas_memcpy_h2d without the wait: queued on the context's stream; h_src (pinned or registered with canvas_host_register) must not change before the next
 * canvas_synchronize.  What CanvasSNV's chunk loop uses to upload chunk k while it inflates chunk k + 1. */
int32_t canvas_memcpy_h2d_async(canvas_ctx* ctx, void* d_dst, const void* h_src, int64_t bytes);
/* Device to device on the context's stream, queued behind what was queued before and not waited for; the ranges must not overlap.  What the executables' chunk loop
 * moves the carried tail of a chunk with when the records are framed on the device (canvas_bam_frame).  CANVAS_ERR_INVALID: NULL context, negative bytes, a NULL
 * pointer with bytes > 0. */
int32_t canvas_memcpy_d2d_async(canvas_ctx* ctx, void* d_dst, const void* d_src, int64_t bytes);

/* Pins a host array (hipHostRegister) so that uploads from it run at the full PCIe rate and asynchronously: what a C# host does once with the arrays
 * LoadIntermediateData left in memory (GCHandle.Alloc(..., Pinned) + this call). */
int32_t canvas_host_register(canvas_ctx* ctx, void* h_ptr, int64_t bytes);
int32_t canvas_host_unregister(canvas_ctx* ctx, void* h_ptr);
/* The per-base arrays of CanvasBin always start in host memory (CanvasBin.LoadIntermediateData, CanvasBin/CanvasBin.cs:965-969).  This call queues their upload
 * chromosome by chromosome on a copy stream of the context (h_* = host sources, d_* = caller-owned device destinations of at least h_len[c] bytes, the mask
 * ceil(len/64) words; a NULL source table or entry = that array is already resident, e.g. the reference bases and the mask of a cohort) and returns at once.
 * The next canvas_bin_sample / canvas_bin_genome / canvas_sample_pipeline call on this context that is given exactly these destination tables sweeps every
 * chromosome as soon as it has arrived, so the upload of chromosome c + 1 overlaps the sweep of chromosome c: pass time ~ max(PCIe, compute), not the sum.
 * Any other call must be preceded by canvas_upload_genome_wait.  Sources must stay valid (and should be pinned) until the binning call has returned. */
int32_t canvas_upload_genome_begin(canvas_ctx* ctx, int32_t nchr, const int64_t* h_len, const uint8_t* const* h_bases, uint8_t* const* d_bases,
                                   const uint64_t* const* h_mask, uint64_t* const* d_mask, const uint8_t* const* h_hits, uint8_t* const* d_hits);
int32_t canvas_upload_genome_wait(canvas_ctx* ctx);

/* ---- packed per-base inputs -------------------------------------------------------------------------------------
 * The loops this library replaces read, per position, one BitArray bit (CanvasBin.cs:593), whether the base is G/C (CanvasBin.cs:599-606), whether it is 'n'
 * (only to find the first one that is not, CanvasBin.cs:582-584) and min(10, hits) (TruncatedDynamicRange, CanvasBin.cs:618-619) or a 0/1 hit (Binary).
 * The packed planes carry exactly that, 0.75 B/base instead of 2.125 B/base (PCIe, which bounds a whole pass, and the one full HBM sweep both shrink 2.8x):
 *   reference planes  per 64 positions {u64 possible, u64 gc}                        16 B   (depends on the reference genome only)
 *   hit planes        per 64 positions {u64 b0, b1, b2, b3}, bit i of b_k = bit k of min(15, hits[i])   32 B
 *   pos0              first position whose base is not 'n' (len if there is none)
 * Both planes cover whole tiles of 4096 positions (canvas_packed_plane_bytes) and are zero beyond len.  Results are bit-identical to the byte-array entry
 * points in Binary and TruncatedDynamicRange modes (hits above 15 cannot occur in Binary mode and read as 10 in TruncatedDynamicRange either way; the packers
 * report the number of saturated positions).  GCContentWeighted mode reads fragment lengths per base and stays on the byte arrays. */
int32_t canvas_packed_plane_bytes(int64_t len, int64_t* ref_bytes, int64_t* hit_bytes);
/* Host-side packers (plain CPU code, no device, thread-parallel; `threads` <= 0 = one per hardware thread, at most 32): what a host that holds the reference's byte
 * arrays (CanvasBin.cs:965-969) runs once per reference / once per sample before the upload.  A host that fills the planes while parsing needs neither. */
int32_t canvas_pack_reference_host(const uint8_t* bases, const uint64_t* mask, int64_t len, uint64_t* ref_out, int64_t* pos0_out, int32_t threads);
int32_t canvas_pack_hits_host(const uint8_t* hits, int64_t len, uint64_t* planes_out, int64_t* saturated_out, int32_t threads);
/* The same packing for arrays that already are in HBM.  d_bases + d_mask + d_ref_out + h_pos0_out may all be NULL (hits only: a second sample over a packed
 * reference), or d_hits + d_hit_planes_out (reference only). */
int32_t canvas_pack_genome_device(canvas_ctx* ctx, int32_t nchr, const uint8_t* const* d_bases, const uint64_t* const* d_mask, const uint8_t* const* d_hits, const int64_t* h_len,
                                  uint64_t* const* d_ref_out, uint64_t* const* d_hit_planes_out, int64_t* h_pos0_out, int64_t* h_saturated_out);
/* canvas_upload_genome_begin for the planes (h_ref NULL or h_ref[c] NULL: already resident); the next canvas_bin_sample_packed / canvas_sample_pipeline_packed call
 * over these destination tables sweeps chromosome c while chromosome c + 1 is in flight.  canvas_upload_genome_wait applies. */
int32_t canvas_upload_packed_begin(canvas_ctx* ctx, int32_t nchr, const int64_t* h_len, const uint64_t* const* h_ref, uint64_t* const* d_ref,
                                   const uint64_t* const* h_hit_planes, uint64_t* const* d_hit_planes);
/* Two-bit wire form of the hit planes.  At WGS depth four hits or more at one position are rare (6.6e-5 of the positions at 60x), so the planes b2 and b3 are almost
 * entirely zero: over PCIe the hit planes can travel as  lo: per 64 positions {u64 b0, b1} (16 B);  hdr: per tile of 64 words {u64 xmask, u64 xoff} (bit w of xmask: word w
 * of the tile has a non-zero b2 or b3, xoff: index of the tile's first entry in extras);  extras: {u64 b2, b3} of those words, in word order  — 0.25 B/base plus a few MB
 * instead of 0.5 B/base.  canvas_pack_hits2_host builds the three pieces from the byte array (lo_out: 2 u64 per word, hdr_out: 2 u64 per tile, extras_out: room for
 * extras_cap_words entries; CANVAS_ERR_CAPACITY with *n_extras_out = the number needed if that is too small).  canvas_upload_packed2_begin is canvas_upload_packed_begin
 * for this form: the pieces are expanded into d_hit_planes[c] (the four planes) on the device right behind their transfer, so canvas_bin_sample_packed /
 * canvas_sample_pipeline_packed are called exactly as after canvas_upload_packed_begin. */
int32_t canvas_pack_hits2_host(const uint8_t* hits, int64_t len, uint64_t* lo_out, uint64_t* hdr_out, uint64_t* extras_out, int64_t extras_cap_words, int64_t* n_extras_out,
                               int64_t* saturated_out, int32_t threads);
int32_t canvas_upload_packed2_begin(canvas_ctx* ctx, int32_t nchr, const int64_t* h_len, const uint64_t* const* h_ref, uint64_t* const* d_ref,
                                    const uint64_t* const* h_lo, const uint64_t* const* h_hdr, const uint64_t* const* h_extras, const int64_t* h_n_extras, uint64_t* const* d_hit_planes);
/* canvas_bin_sample (below) over the planes: same arguments otherwise, same outputs bit for bit (modes 0 and 3). */
int32_t canvas_bin_sample_packed(canvas_ctx* ctx, int32_t nchr, const uint64_t* const* d_ref, const uint64_t* const* d_hit_planes, const int64_t* h_len, const int64_t* h_pos0,
                                 const uint8_t* h_chr_is_autosome, int32_t counts_per_bin, int32_t bin_size_in, int32_t mode,
                                 int32_t* d_chr, int32_t* d_start, int32_t* d_stop, int32_t* d_gc, float* d_count, int64_t cap,
                                 int32_t* h_bin_size_out, int64_t* h_nbins_per_chr, int64_t* h_nbins_total);

/* ---- CanvasBin ----------------------------------------------------------------------------------------------- */
/* InitializeAlignmentArrays (CanvasBin/CanvasBin.cs:183-200): possible[i] = char.IsUpper(referenceBases[i]).
 * d_mask must hold ceil(len/64) words; bits at and beyond len are written as 0. */
int32_t canvas_mask_from_fasta(canvas_ctx* ctx, const uint8_t* d_bases, int64_t len, uint64_t* d_mask);
/* ExcludeTagsOverlappingFilterFile (CanvasBin.cs:668-692): clear the possible bits of [start, stop) for the n BED intervals
 * of this chromosome (intervals are clipped to [0, len); the reference would throw past the end). */
int32_t canvas_mask_exclude_intervals(canvas_ctx* ctx, uint64_t* d_mask, int64_t len, int32_t n, const int32_t* h_start, const int32_t* h_stop);
/* ScreenObservedTags (CanvasBin.cs:699-716): hits[i] = 0 wherever the position is not a possible alignment. */
int32_t canvas_screen_hits(canvas_ctx* ctx, uint8_t* d_hits, const uint64_t* d_mask, int64_t len);
/* SampleHitArrays.GetRates (CanvasBin/CanvasBin.cs:30-71) + HitArray.CountSetBits (HitArray.cs:24-32) +
 * CanvasBin.CountSetBits (CanvasBin.cs:146-156): per chromosome #positions with hit>0 and popcount(mask).
 * h_observed/h_possible/h_rate have nchr entries (rate = observed/(double)possible). */
int32_t canvas_bin_rates(canvas_ctx* ctx, int32_t nchr, const uint8_t* const* d_hits, const uint64_t* const* d_mask,
                         const int64_t* h_len, int64_t* h_observed, int64_t* h_possible, double* h_rate);
/* SampleHitArrays.GetBinSize (CanvasBin.cs:73-83): (int)(countsPerBin / median(rates)); pass autosome rates only
 * (MultiSampleHitArrays, :86-110: concatenate the samples' rates). Host scalar code. */
int32_t canvas_bin_size_from_rates(const double* h_rates, int32_t n, int32_t counts_per_bin);
/* upper bound for the bin arrays of canvas_bin_genome */
int64_t canvas_bin_count_upper_bound(int32_t nchr, const int64_t* h_len, int32_t bin_size);
/* BinCounts / BinCountsForChromosome (CanvasBin.cs:416-661), no predefined bins: emits the genome's bins in chromosome
 * order as SoA (chromosome index, start, stop, gc, count as float like SampleGenomicBin.Count).  cap = capacity of the
 * output arrays; *h_nbins_total and h_nbins_per_chr (nchr entries, may be NULL) are written on return (one sync). */
int32_t canvas_bin_genome(canvas_ctx* ctx, int32_t nchr, const uint8_t* const* d_bases, const uint64_t* const* d_mask,
                          const uint8_t* const* d_hits, const int64_t* h_len, int32_t bin_size, int32_t mode,
                          int32_t* d_chr, int32_t* d_start, int32_t* d_stop, int32_t* d_gc, float* d_count, int64_t cap,
                          int64_t* h_nbins_per_chr, int64_t* h_nbins_total);

/* CanvasBin.RunSingleSample (CanvasBin.cs:914-931) in one call: when bin_size_in <= 0 the bin size is derived from the
 * autosomes' rates with counts_per_bin (-d) exactly as canvas_bin_rates + canvas_bin_size_from_rates would, and the mask
 * popcounts of the rate pass are reused for the binning pass (saves one 0.125 B/base sweep).  *h_bin_size_out = size used. */
int32_t canvas_bin_sample(canvas_ctx* ctx, int32_t nchr, const uint8_t* const* d_bases, const uint64_t* const* d_mask,
                          const uint8_t* const* d_hits, const int64_t* h_len, const uint8_t* h_chr_is_autosome,
                          int32_t counts_per_bin, int32_t bin_size_in, int32_t mode,
                          int32_t* d_chr, int32_t* d_start, int32_t* d_stop, int32_t* d_gc, float* d_count, int64_t cap,
                          int32_t* h_bin_size_out, int64_t* h_nbins_per_chr, int64_t* h_nbins_total);

/* GCContentWeighted mode (-m 5, Somatic-WGS): CanvasBin.cs:416-506 (read-GC profile from the per-position fragment lengths, mean
 * fragment size), :330-405 (observed-vs-expected weights), :626-636 (count = Round(sum min(10, hit / weight[readGC])) in float32,
 * position order).  d_fraglen = Int16 fragment length per position (0 = no read), one array per chromosome. */
int32_t canvas_bin_sample_gcweighted(canvas_ctx* ctx, int32_t nchr, const uint8_t* const* d_bases, const uint64_t* const* d_mask,
                                     const uint8_t* const* d_hits, const int16_t* const* d_fraglen, const int64_t* h_len,
                                     const uint8_t* h_chr_is_autosome, int32_t counts_per_bin, int32_t bin_size_in,
                                     int32_t* d_chr, int32_t* d_start, int32_t* d_stop, int32_t* d_gc, float* d_count, int64_t cap,
                                     int32_t* h_bin_size_out, int64_t* h_nbins_per_chr, int64_t* h_nbins_total);
/* last canvas_bin_sample_gcweighted of the context: h_out2[0] = bins whose weighted count (CanvasBin.cs:626-636) was decided from the exact sum of its terms and the rounding-error
   interval of the reference's float32 accumulation, h_out2[1] = bins that replayed the reference's additions in position order (an interval that straddles a rounding boundary) */
int32_t canvas_bin_gcw_stats(canvas_ctx* ctx, int64_t* h_out2);

/* Predefined bins (CanvasBin -n; BinCountsForChromosome with usePredefinedBins, CanvasBin.cs:575-655): count and GC of the given intervals instead of bins of a fixed
 * number of possible positions.  Bins of all chromosomes are concatenated in chromosome order, h_bin_offset[nchr+1] indexes them; start / stop (0-based, half open) are
 * given twice, on the host (validated as Utilities.LoadBedFile does) and on the device.  d_count = sum over the possible positions of hit (mode 0) or min(10, hit) (mode 3),
 * d_gc = (int)(100f * #[CcGg] / #positions) — the first bin of a chromosome starts counting at its first base that is not 'n' (:582-584). */
int32_t canvas_bin_predefined(canvas_ctx* ctx, int32_t nchr, const uint8_t* const* d_bases, const uint64_t* const* d_mask, const uint8_t* const* d_hits, const int64_t* h_len,
                              int32_t mode, const int64_t* h_bin_offset, const int32_t* h_bin_start, const int32_t* h_bin_stop, const int32_t* d_bin_start, const int32_t* d_bin_stop,
                              int32_t* d_gc, float* d_count);
/* The same with -m GCContentWeighted (the predefined-bin close shares the weighted branch, CanvasBin.cs:617-636): d_count = (int)Math.Round of the float32 sum over the bin's
 * possible positions of Math.Min(10, hit / observedVsExpectedGC[readGC]).  The mean fragment size, the read-GC profile and the weights are the whole call's — every one of the
 * nchr chromosomes enters them (BinCounts, CanvasBin.cs:427-505), whether it has bins (h_bin_offset[c] < h_bin_offset[c + 1]) or not.  Arrays 16-byte aligned as for
 * canvas_bin_sample_gcweighted; canvas_bin_gcw_stats reports decided / replayed bins. */
int32_t canvas_bin_predefined_gcweighted(canvas_ctx* ctx, int32_t nchr, const uint8_t* const* d_bases, const uint64_t* const* d_mask, const uint8_t* const* d_hits,
                                         const int16_t* const* d_fraglen, const int64_t* h_len, const int64_t* h_bin_offset, const int32_t* h_bin_start, const int32_t* h_bin_stop,
                                         const int32_t* d_bin_start, const int32_t* d_bin_stop, int32_t* d_gc, float* d_count);

/* ---- CanvasClean --------------------------------------------------------------------------------------------- */
/* CanvasClean.Main (CanvasClean/CanvasClean.cs:415-533) on the whole-genome SoA in file order, in place; bins that
 * survive are compacted to the front, *h_n_out = surviving count.  h_chr_is_autosome[nchr] answers
 * GenomeMetadata.SequenceMetadata.IsAutosome for each chromosome index.  min_bins_per_gc = the -w option (default 100).
 * h_local_sd_out receives the #localSD metric (IO.cs:83-98) or -1.  h_info (may be NULL) gets 8 int32 diagnostics:
 * [0] after size filter, [1] after outlier filter, [2] after GC strip, [3] after local-SD filter, [4] variance-normalised,
 * [5] 1 = the medians / quartiles were read off exact per-value counters (counts that are two-decimal values, as the F2 text
 * of a .binned file always is), 0 = radix selects (any other input; same results), [6] 1 = flags were -g alone (CANVAS_CLEAN_GCNORM) on whole-number counts and
 * the stage ran as RemoveBinsWithExtremeGC + NormalizeByGC (CanvasClean.cs:163-237,497-505) in three launches, in place (same results as the general chain), [7] with [6] = 1: chunks
 * k_cg_fixup moved; with [6] = 0: 1 = the device-driven chain (clean_fast.hpp) produced the result, 0 = the host-driven path did (LOESS, -w < 100, more than 1024 chromosome runs). */
int32_t canvas_clean(canvas_ctx* ctx, int64_t n, int32_t* d_chr, int32_t* d_start, int32_t* d_stop, float* d_count,
                     int32_t* d_gc, int32_t nchr, const uint8_t* h_chr_is_autosome, uint32_t flags, int32_t min_bins_per_gc,
                     double* h_local_sd_out, int64_t* h_n_out, int32_t* h_info);

/* same with -m LOESS support (flag CANVAS_CLEAN_LOESS): h_chr_is_y[nchr] marks chrY/Y, which LoessGCNormalizer leaves out of the
 * bandwidth search (LoessGCNormalizer.cs:49-50,63-68).  LOESS-mode counts match the reference within 1e-5 relative (the floating
 * sums are re-associated); MedianByGC mode is bit-exact.  NULL h_chr_is_y = no chromosome is chrY. */
int32_t canvas_clean2(canvas_ctx* ctx, int64_t n, int32_t* d_chr, int32_t* d_start, int32_t* d_stop, float* d_count,
                      int32_t* d_gc, int32_t nchr, const uint8_t* h_chr_is_autosome, const uint8_t* h_chr_is_y, uint32_t flags,
                      int32_t min_bins_per_gc, double* h_local_sd_out, int64_t* h_n_out, int32_t* h_info);
/* canvas_clean2 for a cohort (CanvasRunner launches one CanvasClean per sample of a pedigree, CanvasRunner.cs:1010-1070): sample s uses h_n[s] and the device arrays
 * h_d_*[s] (1 .. 64 samples).  The MedianByGC stage is batch-native: the samples share every kernel launch (one launch chain and one wait for the whole cohort); LOESS
 * mode and -w < 100 run sample after sample.  Outputs per sample: h_n_out[s], h_local_sd_out[s] (may be NULL), h_info[8 * s ..] (may be NULL).  Results are exactly
 * those of nsamples canvas_clean2 calls. */
int32_t canvas_clean_batch(canvas_ctx* ctx, int32_t nsamples, const int64_t* h_n, int32_t* const* h_d_chr, int32_t* const* h_d_start, int32_t* const* h_d_stop, float* const* h_d_count,
                           int32_t* const* h_d_gc, int32_t nchr, const uint8_t* h_chr_is_autosome, const uint8_t* h_chr_is_y, uint32_t flags, int32_t min_bins_per_gc,
                           double* h_local_sd_out, int64_t* h_n_out, int32_t* h_info);
/* Pedigree workflows: Utilities.MergeMultiSampleCleanedBedFile + CanvasRunner.NormalizeCanvasClean (CanvasCommon/Utilities.cs:834-920,
 * CanvasRunner.cs:883-903): keep the bins (keyed by chromosome and start) that every sample's cleaned list still has.  Inputs: per
 * sample the SoA of CanvasClean (sorted by chromosome index, then start).  Outputs: one bin list in the first sample's order (stop taken
 * from the last sample) and, per sample, the counts of the surviving bins (h_d_out_count[s], capacity h_n[0]). */
int32_t canvas_merge_cleaned(canvas_ctx* ctx, int32_t nsamples, const int64_t* h_n, const int32_t* const* h_d_chr, const int32_t* const* h_d_start,
                             const int32_t* const* h_d_stop, const float* const* h_d_count, int32_t* d_out_chr, int32_t* d_out_start, int32_t* d_out_stop,
                             float* const* h_d_out_count, int64_t* h_n_out);
/* bins are grouped by chromosome in file order: h_chr_offset[c] = index of the first bin of chromosome c (nchr+1 entries,
 * h_chr_offset[nchr] = n); chromosomes without bins get an empty range.  Chromosome indices must be non-decreasing. */
int32_t canvas_chromosome_offsets(canvas_ctx* ctx, const int32_t* d_chr, int64_t n, int32_t nchr, int64_t* h_chr_offset);

/* The text hand-off between CanvasClean and CanvasPartition, done in memory: CanvasIO.WriteToTextFile prints the float
 * count with "{3:F2}" (CanvasCommon/IO.cs:21; .NET Core 2.x: 7 significant digits, then half-up at 2 decimals) and
 * CanvasSegment.ReadBedInput parses that text as double (CanvasCommon/CanvasSegment.cs:1146).  d_cov[i] = that double. */
int32_t canvas_quantize_f2(canvas_ctx* ctx, const float* d_count, int64_t n, double* d_cov);

/* ---- CanvasPartition ------------------------------------------------------------------------------------------ */
/* HiddenMarkovModelsRunner.Run with isPerSample (HiddenMarkovModelsRunner.cs:23-109) + BestPathViterbi (HMM.cs:62-130):
 * one sample, all chromosomes.  d_cov = concatenated coverage (double, file order), h_chr_offset[nchr+1] = chromosome
 * boundaries in bins.  d_state receives the Viterbi state (CN 0..4) per bin; chromosomes with <= 10 bins are skipped
 * (state -1), as in :69.  */
int32_t canvas_hmm_per_sample(canvas_ctx* ctx, int32_t nchr, const double* d_cov, const int64_t* h_chr_offset, int32_t* d_state);
/* -m HMM: HiddenMarkovModelsRunner.Run with isPerSample == false (HiddenMarkovModelsRunner.cs:23-152; CanvasPartition.cs:146-158) and
 * NegativeBinomialMixture.EstimateViterbiLikelihood over the genotype combinations (Distributions.cs:257-323,
 * DistributionUtilities.cs:11-40): one state path for nsamples (1..16) samples that share the bins.  h_d_cov[s] = device pointer to
 * sample s's concatenated coverage (same layout and h_chr_offset for all samples).  Emission parameters are per chromosome (median and
 * variance of that chromosome, :117-131); chromosomes with <= 10 bins are skipped (state -1). */
int32_t canvas_hmm_joint(canvas_ctx* ctx, int32_t nsamples, int32_t nchr, const double* const* h_d_cov, const int64_t* h_chr_offset, int32_t* d_state);
/* breakpoints -> segments -> segment id per bin: SegmentationInput.DeriveSegments (Segmentation.cs:83-125) +
 * SegmentationResultsProcessor.PostProcessSegments (SegmentationResultsProcessor.cs:17-129, no forbidden intervals /
 * ploidy file: those stay in the host tool).  d_is_start: 1 where a segment starts at this bin. */
int32_t canvas_segment_ids(canvas_ctx* ctx, int32_t nchr, const int64_t* h_chr_offset, const int32_t* d_state,
                           const int32_t* d_start, const int32_t* d_stop, int32_t max_inter_bin_dist, int32_t* d_segment_id,
                           int64_t* h_nsegments);
/* same, with the forbidden intervals of the -b BED file (SegmentationResultsProcessor.cs:88-111): a segment is split where the
 * midpoint of an interval lies between two bins.  h_excl_offset[nchr+1] indexes h_excl_start/stop per chromosome; intervals must be
 * sorted by end inside a chromosome (the reference walks them with a forward-only cursor). */
int32_t canvas_segment_ids_filtered(canvas_ctx* ctx, int32_t nchr, const int64_t* h_chr_offset, const int32_t* d_state,
                                    const int32_t* d_start, const int32_t* d_stop, int32_t max_inter_bin_dist,
                                    const int64_t* h_excl_offset, const int32_t* h_excl_start, const int32_t* h_excl_stop,
                                    int32_t* d_segment_id, int64_t* h_nsegments);
/* same, with the reference ploidy of CanvasPartition -p (CanvasPartition.cs:114; CanvasRunner.InvokeCanvasPartition always passes it, CanvasRunner.cs:950):
 * a new segment also starts where PloidyInfo.IsUniformReferencePloidy is false for the one-based interval [previous bin end (or 1), this bin's end]
 * (SegmentationResultsProcessor.cs:117-128, PloidyInfo.cs:78-110).  h_ploidy_offset[nchr+1] indexes the records of the ploidy VCF per chromosome
 * (PloidyInfo.LoadPloidyFromVcfFile, PloidyInfo.cs:128-165): h_ploidy_start = POS (one-based), h_ploidy_end = INFO/END, h_ploidy_cn = the CN genotype
 * field ("." = 2), 0..4.  A chromosome without records behaves like one that is not in the VCF.  h_ploidy_offset == NULL: no -p.  The forbidden
 * intervals are optional as above (h_excl_offset == NULL: no -b). */
int32_t canvas_segment_ids_ploidy(canvas_ctx* ctx, int32_t nchr, const int64_t* h_chr_offset, const int32_t* d_state, const int32_t* d_start,
                                  const int32_t* d_stop, int32_t max_inter_bin_dist,
                                  const int64_t* h_excl_offset, const int32_t* h_excl_start, const int32_t* h_excl_stop,
                                  const int64_t* h_ploidy_offset, const int32_t* h_ploidy_start, const int32_t* h_ploidy_end, const int32_t* h_ploidy_cn,
                                  int32_t* d_segment_id, int64_t* h_nsegments);
/* CanvasPartition --evenness-metric-file (Somatic-WGS, CanvasRunner.cs:958-960): SegmentationInput.GetEvennessScore (Segmentation.cs:260-296) as
 * WaveletsRunner.Run computes it before segmenting (WaveletsRunner.cs:58-67).  d_cov / h_chr_offset as for canvas_cbs; window_size =
 * CanvasPartitionParameters.EvennessScoreWindow (100000).  *h_valid = 0 when the reference's Quartiles / Median throw (fewer than two 10000-bin windows,
 * or no window of window_size: the reference then writes no metric file), otherwise *h_score is the value written as "#evenness\t<score>"
 * (IO.cs:88-98).  Bit-exact: the window sums are evaluated in list order. */
int32_t canvas_evenness_score(canvas_ctx* ctx, int32_t nchr, const double* d_cov, const int64_t* h_chr_offset, int32_t window_size, double* h_score, int32_t* h_valid);
/* GenomeSegmentationResults.SplitOverlappingSegments (GenomeSegmentationResults.cs:18-55) for one chromosome: host scalar code. */
int32_t canvas_split_overlapping(int32_t nsamples, const uint32_t* const* h_start, const uint32_t* const* h_end, const int32_t* h_nseg,
                                 uint32_t* h_out_start, uint32_t* h_out_end, int32_t cap, int32_t* h_nout);
/* Partition states: what canvas_cbs / canvas_cbs_undo (segment lengths on the device) and canvas_wavelets (breakpoints on the host) leave, as the per-bin d_state that
 * canvas_segment_ids* takes.  d_state[i] (int32, h_chr_offset[nchr] entries) is the zero-based ordinal, within its chromosome, of the segment that holds bin i; every bin of a
 * chromosome for which the method derives no segment gets -1.  canvas_segment_ids* starts a segment where state >= 0 && (first bin of the chromosome || state != previous
 * state); on these states that is membership of the bin's start in the `starts` set SegmentationResultsProcessor.PostProcessSegments looks up, as long as the bins' starts
 * increase strictly within a chromosome — so canvas_segment_ids*, unchanged, gives the ids CanvasPartition writes for that method.
 * _cbs (CBSRunner.cs:127-137): the layout canvas_cbs documents, chromosome c has its h_nseg[c] lengths at d_seg_len + h_chr_offset[c]; segment k starts at the sum of the
 *   lengths before it; h_nseg[c] == 0 gives -1 throughout.  CANVAS_ERR_INVALID, decided on the device through one error word and naming the first such chromosome:
 *   h_nseg[c] outside 0 .. T_c, a length < 1, lengths that do not sum to T_c (h_nseg[c] > 0).  A refused call leaves d_state alone.
 * _breakpoints (SegmentationInput.DeriveSegments, Segmentation.cs:83-125): chromosome c has the breakpoints h_bp_offset[c] .. h_bp_offset[c+1] of h_breakpoints (bin indices
 *   within the chromosome, as canvas_wavelets returns them).  With at least two breakpoints and T_c > 10 the starts are bin 0 and every breakpoint (in any order, repeats
 *   allowed); otherwise the chromosome is one segment (state 0).  T_c == 0 writes nothing.  CANVAS_ERR_INVALID before the context is looked at and before any launch:
 *   offsets that do not start at 0 or decrease, a breakpoint outside [0, T_c).
 * No per-bin array crosses to the host; each call waits once. */
int32_t canvas_partition_states_cbs(canvas_ctx* ctx, int32_t nchr, const int64_t* h_chr_offset /* nchr+1 */, const int32_t* d_seg_len, const int32_t* h_nseg /* nchr */,
                                    int32_t* d_state);
int32_t canvas_partition_states_breakpoints(canvas_ctx* ctx, int32_t nchr, const int64_t* h_chr_offset /* nchr+1 */, const int32_t* h_breakpoints,
                                            const int64_t* h_bp_offset /* nchr+1 */, int32_t* d_state);
/* CBSRunner.Run / ChangePoint.ChangePoints (CBSRunner.cs:40-151, ChangePoint.cs:44-153), undo = None.
 * d_seg_len receives per chromosome the segment lengths, written at d_seg_len + h_chr_offset[c]; h_nseg[c] = count. */
int32_t canvas_cbs(canvas_ctx* ctx, int32_t nchr, const double* d_cov, const int64_t* h_chr_offset, double alpha, uint32_t nperm,
                   int32_t* d_seg_len, int32_t* h_nseg, int64_t* h_stats);

/* same with -s Prune (undo = 1, ChangePoint.cs:205-271 + Prune.cs, cut-off 0.05), -s SDUndo (undo = 2, ChangePoint.cs:155-196; undo_sd = 3 in
   the reference) or None (0). */
int32_t canvas_cbs_undo(canvas_ctx* ctx, int32_t nchr, const double* d_cov, const int64_t* h_chr_offset, double alpha, uint32_t nperm,
                        int32_t undo, double undo_sd, int32_t* d_seg_len, int32_t* h_nseg, int64_t* h_stats);

/* counters of the device permutation engine for the last canvas_cbs / canvas_cbs_undo call: [0] permutations evaluated on the device
 * (XPerm + HTMaxP, CBSTStatistic.cs:354-586), [1] on the host (segments shorter than 1024 bins, TMaxP), [2] device permutations that
 * were re-evaluated in the reference's exact order because the observed statistic fell inside the rounding interval, [3] batches,
 * [4]/[5] test hook CANVAS_CBS_TEST_VERIFY=1: device intervals checked against the exact statistic / violations. */
int32_t canvas_cbs_device_stats(canvas_ctx* ctx, int64_t* h_out6);
/* the edge tests (CBSTStatistic.TPermP, CBSTStatistic.cs:947-1024) of the last canvas_cbs / canvas_cbs_undo call: [0] tests run by the device kernel (one lane walks the
 * chain of nPerm x min(n1, n2) dependent swaps; CANVAS_CBS_DEVICE_TPERMP=1 — the default is the host chain, which is 30x faster per swap), [1] swaps of all edge tests. */
int32_t canvas_cbs_tpermp_stats(canvas_ctx* ctx, int64_t* h_out2);
/* last canvas_cbs / canvas_cbs_undo call: the analytic tail probability of the hybrid test (TailProbability.TailP, TailProbability.cs:21-85) only feeds two decisions of
 * FindChangePoints (ChangePoint.cs:318-323).  [0] calls decided from the device evaluation of its series (accepted only when every value within 1e-8 relative gives the same
 * decisions), [1] calls recomputed with the host libm in the reference's order. */
int32_t canvas_cbs_tailp_stats(canvas_ctx* ctx, int64_t* h_out2);
/* Diagnostic / test entry: TailProbability.Nu (TailProbability.cs:52-85) of n <= 100 arguments through the device series exactly as canvas_cbs evaluates it (k_tail_nu: the
 * first 512 terms one by one, every later block of the series from the Euler-Maclaurin formula); h_flag[i] != 0: a stopping comparison of the series was too close to call and
 * canvas_cbs would redo the call with the host series. */
int32_t canvas_cbs_tail_probe(canvas_ctx* ctx, const double* h_x, int32_t n, double tol, double* h_nu, int32_t* h_flag);
/* Diagnostic / test entry: ONE batch of nb permutations of the centred segment h_x[n] (n >= 1024, n * nb <= 2^30) through the device permutation engine exactly as the hybrid test of
 * FindChangePoints runs it — XPerm (ChangePoint.cs:407-421) + HTMaxP with k = 25, minimum width 2 (CBSTStatistic.cs:354-586) — from MersenneTwister(seed).  kernel selects the
 * permutation kernel: 0 k_perm_stat (counting sort + pointer doubling), 1 k_perm_fy (block-wise simulation of the swaps in global memory), 2 k_perm_rp (range-partitioned simulation
 * in LDS; n <= 524288, CANVAS_ERR_INVALID beyond).  h_lohi[2 nb]: the interval the engine returns for every permutation's statistic (the exact value lies inside; the stopping rule
 * re-evaluates a permutation on the host only when the observed statistic does too; [-inf, inf]: the kernel gave the permutation up).  tests/test_cbs_perm_kernels_gpu.py compares
 * the intervals of all three kernels with the oracle's XPerm + HTMaxP.
 * h_ms3 (optional): milliseconds of the generator's sequential part, its strided part, and the permutation + statistic kernel.  No reference counterpart: the engine's test bench. */
int32_t canvas_cbs_perm_probe(canvas_ctx* ctx, const double* h_x, int32_t n, uint32_t seed, int32_t nb, int32_t kernel, double tss, double* h_lohi, double* h_ms3);
/* Diagnostic / test entry: the observed statistic TMaxO (CBSTStatistic.cs:19-341) of nseg centred segments, h_x[h_off[s] .. h_off[s + 1]), exactly as canvas_cbs searches it on the
 * device for a segment of 4096 bins or more (here: n >= 4).  mode 0: the pruned search (k_arcp_blocks, k_arcp_bounds, k_arcp_eval, k_arcp_mail), the exhaustive kernel
 * (k_arc_search) when the pair list overflows; mode 1: the exhaustive kernel only (as under CANVAS_CBS_EXHAUSTIVE_ARCS).  al0 >= 1: the minimum arc length.  pair_cap: the pair
 * list's capacity, 0 = the library's 8192, else 1 .. 8192 (a small one reaches the overflow branch on a short segment).  All segments of a call are queued at one launcher
 * before it wakes: they share its launches, 64 requests at a time, in order.  Finite values only.  Per segment s:
 *   h_sx[h_off[s] ..]   the prefix sums;
 *   h_tau[s]            the incumbent the search starts from (the arc between the prefix sums' extremes, both taken as 0 at position n until something beats that; 0 when they coincide);
 *   h_stat[s], h_iseg[2 s ..]  the statistic (before FindChangePoint's 0.99999) and the 1-based arc, as the reference's TMaxO returns them;
 *   h_path[s]           0 no launch (the extremes coincide), 1 the incumbent was kept, 2 the device's unique maximiser was accepted, 3 several arcs attain the maximum (host replay
 *                       of the reference's block order), 4 a unique maximiser that the reference's scan leaves out (host replay); + 8: the pair list overflowed and the exhaustive
 *                       kernel supplied the answer;
 *   h_words[6 s ..]     the pruned search's result words after it finished: the maximum's bits, the number of arcs attaining it, the smallest (L << 32) | i among them (i: 0-based
 *                       start), the number of surviving block pairs, the overflow flag, the best block-extreme arc's bits (zeros when no pruned search ran);
 *   h_dmax, h_first [h_off[s] + L], L = 1 .. n - 1: where the exhaustive kernel ran, max_i |sx[i + L] - sx[i]| and the smallest such i (untouched otherwise).
 * h_sx, h_dmax, h_first are as long as h_x.  tests/test_cbs_arc_kernels_gpu.py compares all of it with an every-arc search in numpy and with the oracle's TMaxO. */
int32_t canvas_cbs_arc_probe(canvas_ctx* ctx, int32_t mode, int32_t nseg, const int64_t* h_off, const double* h_x, int32_t al0, int32_t pair_cap,
                             double* h_sx, double* h_tau, double* h_stat, int32_t* h_iseg, int32_t* h_path, uint64_t* h_words, double* h_dmax, int32_t* h_first);
/* Diagnostic / test entry: the exact order-statistics engine behind every median and quartile of the library (csrc/select.hpp) on caller-supplied data.  d_values (device) holds
 * h_seg_off[nseg] elements partitioned in nseg segments by h_seg_off[nseg + 1] (host, non-decreasing).  dtype: 0 float32 values keyed on the device (the CanvasClean / PerSampleHMM
 * path, 32-bit keys), 1 float64 values keyed on the device (CanvasNormalize / LOESS, 64-bit keys), 2 / 3 raw uint32 / uint64 keys.  The key of a value is its order-preserving
 * unsigned image: all bits flipped when the sign bit is set, the sign bit set otherwise.  variant: 0 radix_select, results through the host; 1 radix_select with its results left
 * on the device (the probe synchronises and copies them, as that contract asks of the caller); 2 wg_select2, one workgroup of 1024 threads per query (dtype 1 or 3 only).
 * Query q asks for the h_k[q]-th smallest key (0-based) of the union of segments h_seg_lo[q]..h_seg_hi[q] -> h_keys_out[q]; with variant 2 h_seg_lo[q] == h_seg_hi[q], h_k holds a
 * PAIR of ranks per query and h_keys_out two keys per query.  CANVAS_ERR_INVALID for decreasing offsets, a segment range that is reversed or outside 0..nseg-1, a rank outside
 * [0, keys in the query's segments), and (variants 0, 1) more than 16 queries on one segment: radix_select's own refusal.  tests/test_select_gpu.py compares every key with a sort. */
int32_t canvas_select_probe(canvas_ctx* ctx, int32_t variant, int32_t dtype, const void* d_values, int32_t nseg, const int64_t* h_seg_off, int32_t nq,
                            const int32_t* h_seg_lo, const int32_t* h_seg_hi, const int64_t* h_k, uint64_t* h_keys_out);
/* Diagnostic / test entry: the exact backbone of the speculative Viterbi pass (csrc/hmm.hip, stage B1) on caller-supplied increments.  d_V (device) holds h_chr_offset[nchr]
 * doubles partitioned in nchr chromosomes by h_chr_offset[nchr + 1] (host, starting at 0, non-decreasing, at most 2^30).  For every chromosome of more than ten steps the entry
 * enqueues exactly the kernels the HMM stage runs for mode 0 (the plain chain), 1 (the parity scan) or 2 (the predicted pieces, the default of the stage) and leaves in
 * d_carry[begin + t] (device, as long as d_V) the sequential FP64 sum of the chromosome's increments 0 .. t-1 for every t = 0, 64, 128, ... below its length; no other element of
 * d_carry is written.  h_fail[nchr]: non-zero where modes 1 / 2 gave the chromosome up (an increment that is positive, infinite or NaN; mode 2: more than 16 binade
 * crossings inside 1024 steps, a predicted binade that turned out wrong) - its carries are then undefined, and the stage recomputes such a chromosome sequentially; mode 0 has
 * no such word and leaves zeros.  CANVAS_ERR_INVALID for a mode outside 0..2, offsets that do not start at 0, decrease or pass 2^30, and missing arrays.
 * tests/test_hmm_backbone_gpu.py compares every carry with the plain sequential sum, bit for bit.  No reference counterpart. */
int32_t canvas_hmm_backbone_probe(canvas_ctx* ctx, int32_t mode, int32_t nchr, const int64_t* h_chr_offset, const double* d_V, double* d_carry, int32_t* h_fail);
/* Host-only (no context, no GPU): the sequential stopping boundary canvas_cbs uses for (nperm, alpha) — GetBoundary.ComputeBoundary (GetBoundary.cs:19-157) with eta = 0.05 as
 * CBSRunner passes it: maxOnes (maxOnes + 1) / 2 entries with maxOnes = floor(nperm alpha) + 1.  Returns the number of entries (or a negative error code).  The library
 * evaluates the table's scans on its host thread pool with the scans' own evaluations and comparisons; exposed so that the table can be checked without a device. */
int64_t canvas_cbs_boundary(uint32_t nperm, double alpha, uint32_t* h_out, int64_t cap);
/* The draw streams of canvas_cbs ahead of its first call.  The k-th chromosome's generator is MersenneTwister(seed_k) with seed_k from MersenneTwister(0) in file order
 * (CBSRunner.cs:107-112) and is consumed strictly in sequence by XPerm / TPermP (ChangePoint.cs:407-421, CBSTStatistic.cs:1009): the words are constants of the method.  The
 * library keeps them per context in device memory (generated once, extended on demand, bounded by CANVAS_CBS_CACHE_GB — default 30 % of the device's memory, 0 = off) and
 * canvas_cbs reads its permutations' draws out of them.  canvas_cbs_prefetch starts the generator for the first `words_per_chromosome` draws of the first nchr streams on a
 * thread and stream of its own — and creates, on another, the streams and request tables of canvas_cbs's launchers (a stream costs ~5 ms on this runtime: 60 ms of a first
 * call) — and returns at once: a host calls it while it is still reading its input (CanvasPartition does).  Optional — canvas_cbs asks for what it needs itself.  canvas_cbs_cache_stats: h_out6 = {draws the last canvas_cbs call read out of the cache, draws it generated inside its batches (cache off / bound reached; chromosomes shorter than the device engine's 201 bins have no stream and draw on the host, uncounted),
 * draws the cache's generator produced during the call, generator states fetched for host code, bytes of device memory the cache holds, draws it holds}. */
int32_t canvas_cbs_prefetch(canvas_ctx* ctx, int32_t nchr, int64_t words_per_chromosome);
/* Diagnostic / test entry: nwords tempered outputs of the chromosome-th generator (0-based, file order) from output number `position` on, read out of the context's cache
 * (generated now if they are not there yet; CANVAS_ERR_CAPACITY when the bound of the cache does not reach that far).  What canvas_cbs's permutation kernels read. */
int32_t canvas_cbs_stream_read(canvas_ctx* ctx, int32_t chromosome, int64_t position, int64_t nwords, uint32_t* h_out);
int32_t canvas_cbs_cache_stats(canvas_ctx* ctx, int64_t* h_out6);
/* Host-only (no context, no GPU): the seeds of the per-chromosome generators canvas_cbs uses, in file order — new MersenneTwister(0) followed by one NextFullRangeInt32() per
 * chromosome (CBSRunner.cs:107-112).  h_out[nchr]; h_variant (optional): which reading of MathNet's NextBytes is in force (0 / 1 / 2, include/canvas_mathnet.h: the one
 * assumption of this path that could not be checked without a .NET SDK; CANVAS_MATHNET_SEED_BYTES selects it at run time).  Returns 0 or a negative error code. */
int32_t canvas_cbs_seeds(int32_t nchr, int32_t* h_out, int32_t* h_variant);

/* CanvasPartition -m Wavelets, the reference's default method: WaveletsRunner.Run up to the breakpoints (WaveletsRunner.cs:52-150 =
 * SegmentationInput.GetCoverageVariability / FactorOfThreeCoverageVariabilities, Segmentation.cs:297-429, then
 * WaveletSegmentation.HaarWavelets per chromosome, WaveletSegmentation.cs:373-425: unbalanced Haar decomposition, HardThresh,
 * reconstruction, GetBreakpointsAfterHealingBadSplits and, with is_germline (-g), RefineSegments).  d_cov / h_chr_offset as for canvas_cbs.
 * The parameters are WaveletsRunnerParams' (WaveletsRunner.cs:28-41): threshold_lower = ThresholdLowerMaf (0.05), threshold_upper = 80,
 * mad_factor = MadFactor (5), variability_window = EvennessScoreWindow (100000), min_size = 10.  h_breakpoints[h_bp_offset[c] .. h_bp_offset[c+1])
 * are the bin indices where a segment starts on chromosome c (empty for a chromosome of at most min_size bins): what the reference
 * hands to SegmentationInput.DeriveSegments (Segmentation.cs:83-125).  Coverage must be finite. */
int32_t canvas_wavelets(canvas_ctx* ctx, int32_t nchr, const double* d_cov, const int64_t* h_chr_offset, int32_t is_germline,
                        double threshold_lower, double threshold_upper, double mad_factor, int32_t variability_window, int32_t min_size,
                        int32_t* h_breakpoints, int64_t cap, int64_t* h_bp_offset);
/* last canvas_wavelets call: [0] tree levels processed, [1] nodes whose shortcut division disagreed with the IEEE one and were recomputed */
int32_t canvas_wavelets_stats(canvas_ctx* ctx, int64_t* h_out2);
/* last canvas_wavelets call: [0] long nodes whose arg-max was decided from the closed form (exact prefix sums + rounding-error bound of WaveletSegmentation.cs:19-48),
   [1] long nodes the bound could not decide (exact chain), [2] long nodes chained for their coefficient (candidates to survive HardThresh, WaveletSegmentation.cs:73-117),
   [3] 1 if the closed form was in use (coverage of non-negative two-decimal values) */
int32_t canvas_wavelets_decisions(canvas_ctx* ctx, int64_t* h_out4);
/* last completed canvas_wavelets call (nchr must be that call's): what its thresholds and its healing step were computed from, as the call itself held them — nothing is
 * computed or waited for here.  *h_has_cv: 1 when the coverage variability was used (at least ten windows of bins), *h_cv: SegmentationInput.GetCoverageVariability
 * (Segmentation.cs:308-328; NaN when most windows have median 0), h_f3_9: FactorOfThreeCoverageVariabilities (Segmentation.cs:366-429), and per chromosome h_is_root (longer than
 * min_size, and selected by the mask of the sharded call), h_median (0 for the others), h_sigma = mad_factor x median x cv clamped to [threshold_lower, threshold_upper]
 * (WaveletSegmentation.cs:394-405) and h_keep_above, the bracket below which the device drops a coefficient (-1 for a NaN threshold).  CANVAS_ERR_INVALID before the first
 * completed call and for another nchr.  *h_paths: which code computed them, bit 0 the factor-of-three values on the device (clear: the host thread, CANVAS_WV_F3_HOST), bit 1 the
 * window statistics of cv on the device (clear: host threads, CANVAS_WV_VAR_HOST, or no cv), bit 2 the chromosome medians on the device (clear: host threads), bit 3 those from the
 * integers by the multi-stretch kernels (clear with bit 2 set: one workgroup per chromosome, CANVAS_WV_MEDIAN_PER_WG or a coverage without two-decimal values).
 * tests/test_wavelets_kernels_gpu.py compares them with the oracle's. */
int32_t canvas_wavelets_inputs(canvas_ctx* ctx, int32_t nchr, int32_t* h_has_cv, double* h_cv, double* h_f3_9, uint8_t* h_is_root, double* h_median, double* h_sigma, double* h_keep_above,
                               int32_t* h_paths);
/* Diagnostic / test entries: the kernels of canvas_wavelets (csrc/wavelets.hip) on caller-supplied nodes, through the launch sets the call itself uses (same kernels, same grids).
 * d_cov (device) holds the coverage; h_chr_offset[nchr + 1] (host) starts at 0 and does not decrease, 1 .. 2^31 - 16 bins.  Nodes are (start, len) into the whole coverage with
 * len >= 2, inside their chromosome.  wv_long (8..256) and the table switch are arguments here (the call reads CANVAS_WV_LONG / CANVAS_WV_NO_TABLE once per process).
 * CANVAS_ERR_INVALID for anything outside these rules.  No reference counterpart; tests/test_wavelets_kernels_gpu.py compares every result with tests/wavelets_ref.py.
 *
 * prefix: k_wv_prefix_tiles + k_wv_prefix_apply.  h_p1[i] = sum of the integers 100 x of the chromosome's bins up to i, h_p2[i] = sum of its h_p1 up to i; h_bad2[0] != 0: some bin
 * is not a non-negative two-decimal value below 2e7, or a chromosome's sums could pass 2^61 (canvas_wavelets then takes the chains); h_bad2[1] != 0: NaN or infinite. */
int32_t canvas_wavelets_prefix_probe(canvas_ctx* ctx, int32_t nchr, const double* d_cov, const int64_t* h_chr_offset, int64_t* h_p1, int64_t* h_p2, int32_t* h_bad2);
/* bound: for node i = (start, len, chromosome) of h_nodes3 and every m = 0 .. len-2, the closed form T[m] and its rounding-error bound B[m] (in units of 100 x) exactly as
 * k_wv_level's inner loop evaluates them (the same device function), concatenated node by node: sum of (len - 1) doubles in h_t and in h_b.  Refuses a coverage with a bad word. */
int32_t canvas_wavelets_bound_probe(canvas_ctx* ctx, int32_t nchr, const double* d_cov, const int64_t* h_chr_offset, int32_t nnodes, const int32_t* h_nodes3, double* h_t, double* h_b);
/* level: k_wv_list_init and ONE k_wv_level (iteration 0, the call's grid) over the nodes (start, len, chromosome, level) of h_nodes4, which share no bin.  h_status[i]: 0 the bound
 * could not decide the node, 1 decided and its coefficient's bracket lies at or below h_keep_above[chromosome] (HardThresh zeroes it), 2 decided and listed for the exact chain;
 * h_ind[i]: the decided arg-max (1-based; 0 for status 0) — the kernel's own record for status 2; for status 1 the kernel keeps none, and the entry RECONSTRUCTS it from the
 * children it appended (the length of the child at the node's first bin, 1 without one): compare it with an independent arg-max before deriving children from it.  h_next4 / *h_nnext: the next level's long nodes (len > wv_long) gathered over the replicas, h_roots6 / *h_nroots: the
 * short children as the subtree walker takes them (start, len, chromosome, level, s1 = 1-based start inside the chromosome, cbase = the chromosome's first bin); both need room for
 * 2 nnodes entries.  h_counts[bins]: the node counters, entry (chromosome's first bin + level).  *h_overflow: the device's overflow word.  Refuses a coverage with a bad word and a
 * list that does not fit the capacities canvas_wavelets allocates for this coverage and wv_long (per replica for the list itself; an eighth of the level's worst case per replica for
 * what it appends, as the call assumes — an assumption, not a guarantee: the kernel checks every append against its capacity and reports a full replica in *h_overflow). */
int32_t canvas_wavelets_level_probe(canvas_ctx* ctx, int32_t nchr, const double* d_cov, const int64_t* h_chr_offset, int32_t nnodes, const int32_t* h_nodes4, const double* h_keep_above,
                                    int32_t wv_long, int32_t* h_status, int32_t* h_ind, int32_t* h_next4, int64_t* h_nnext, int32_t* h_roots6, int64_t* h_nroots, int32_t* h_counts,
                                    int32_t* h_overflow);
/* chain: k_wv_coeff, k_wv_chain_long (fast != 0: the shortcut division, else IEEE), k_wv_chunks and k_wv_reduce over the nodes (start, len) of h_nodes2 in a coverage of n_cov bins.
 * h_lim (optional, >= 0): the chain of node i stops after step h_lim[i].  own_slices != 0: every node gets an operand slice of its own (needed when nodes share bins).  Per node:
 * h_coef = ipi[ind - 1] / max(0.5, mean / 200), h_ind = GetInnerProdMax (1-based), h_flag != 0: a checkpoint of the shortcut chain was not reproduced (canvas_wavelets redoes such
 * a node with IEEE divisions). */
int32_t canvas_wavelets_chain_probe(canvas_ctx* ctx, int64_t n_cov, const double* d_cov, int32_t nnodes, const int32_t* h_nodes2, const int32_t* h_lim, int32_t fast, int32_t own_slices,
                                    double* h_coef, int32_t* h_ind, int32_t* h_flag);
/* subtree: k_wv_fgh_table (use_table != 0) and k_wv_subtree over the roots (start, len <= wv_long, chromosome, level, s1, cbase) of h_roots6, which share no bin.  h_counts[bins] as
 * above; *h_ncand: coefficients above h_keep_above[chromosome] the walkers found, of which the first min(*h_ncand, cap_cand) are in h_cand5 (chromosome, level, s, b, e: 1-based
 * inside the chromosome) and h_cand_coef, in no particular order; *h_overflow != 0: there were more than cap_cand (0 <= cap_cand <= bins + 16). */
int32_t canvas_wavelets_subtree_probe(canvas_ctx* ctx, int32_t nchr, const double* d_cov, const int64_t* h_chr_offset, int32_t nroots, const int32_t* h_roots6, const double* h_keep_above,
                                      int64_t cap_cand, int32_t wv_long, int32_t use_table, int32_t* h_counts, int32_t* h_cand5, double* h_cand_coef, int64_t* h_ncand, int32_t* h_overflow);
/* medians: Utilities.Median (Utilities.cs:428-443) of up to 1024 stretches (start, len >= 0; 0 for an empty one) from the integers of k_wv_prefix_tiles through the three
 * k_wv_rmed_pass launches -> h_median; h_median_wg (optional): the same stretches through k_wv_segment_median, one workgroup per stretch over the doubles.  h_bad2 as for prefix
 * (with a bad word the integers, and h_median, mean nothing). */
int32_t canvas_wavelets_median_probe(canvas_ctx* ctx, int64_t n_cov, const double* d_cov, int32_t nstretch, const int64_t* h_start, const int64_t* h_len, double* h_median, double* h_median_wg,
                                     int32_t* h_bad2);

/* ---- one sample through the whole path in one call -------------------------------------------------------------
 * canvas_bin_sample -> canvas_clean2 -> canvas_quantize_f2 -> canvas_chromosome_offsets -> canvas_hmm_per_sample -> canvas_segment_ids with
 * the arguments of those calls (h_chr_is_y may be NULL).  Outputs: the cleaned bins in d_chr..d_count (first *h_nbins_clean entries), d_cov,
 * d_state and d_segment_id per cleaned bin, h_chr_offset[nchr+1], the bin size, bin counts, #localSD and the number of segments.  Nothing
 * is computed that the individual entry points do not compute: it only saves the caller's per-call overhead between the stages. */
int32_t canvas_sample_pipeline(canvas_ctx* ctx, int32_t nchr, const uint8_t* const* d_bases, const uint64_t* const* d_mask, const uint8_t* const* d_hits,
                               const int64_t* h_len, const uint8_t* h_chr_is_autosome, const uint8_t* h_chr_is_y, int32_t counts_per_bin, int32_t bin_size_in,
                               int32_t mode, uint32_t clean_flags, int32_t min_bins_per_gc, int32_t max_inter_bin_dist,
                               int32_t* d_chr, int32_t* d_start, int32_t* d_stop, int32_t* d_gc, float* d_count, int64_t cap,
                               double* d_cov, int32_t* d_state, int32_t* d_segment_id,
                               int32_t* h_bin_size, int64_t* h_nbins, int64_t* h_nbins_clean, double* h_local_sd, int64_t* h_chr_offset, int64_t* h_nsegments);

/* canvas_sample_pipeline over the packed planes (canvas_bin_sample_packed). */
int32_t canvas_sample_pipeline_packed(canvas_ctx* ctx, int32_t nchr, const uint64_t* const* d_ref, const uint64_t* const* d_hit_planes, const int64_t* h_len, const int64_t* h_pos0,
                                      const uint8_t* h_chr_is_autosome, const uint8_t* h_chr_is_y, int32_t counts_per_bin, int32_t bin_size_in,
                                      int32_t mode, uint32_t clean_flags, int32_t min_bins_per_gc, int32_t max_inter_bin_dist,
                                      int32_t* d_chr, int32_t* d_start, int32_t* d_stop, int32_t* d_gc, float* d_count, int64_t cap,
                                      double* d_cov, int32_t* d_state, int32_t* d_segment_id,
                                      int32_t* h_bin_size, int64_t* h_nbins, int64_t* h_nbins_clean, double* h_local_sd, int64_t* h_chr_offset, int64_t* h_nsegments);

/* ---- CanvasNormalize, ratio path (enrichment / tumour-normal workflows) -------------------------------------------------
 * canvas_normalize_reference = WeightedAverageReferenceGenerator.Run for more than one control sample (WeightedAverageReferenceGenerator.cs:
 * 38-68): weight_i = 1 / median_i (0 if the median is not positive), normalised to sum 1, median_i = BinCounts.OnTargetMedianBinCount
 * (BinCounts.cs:36-60) over the bins listed in d_on_target_idx (NULL: all bins; the list is what BinCounts.LoadBinCounts derives from the
 * Nextera manifest, BinCounts.cs:118-166); d_weighted[j] = sum_i weight_i * counts_i[j].  h_d_counts: nsamples device pointers to n doubles
 * each (the 4th column of the control .binned files, double.Parse).  With one control sample the reference copies the file instead. */
int32_t canvas_normalize_reference(canvas_ctx* ctx, int32_t nsamples, const double* const* h_d_counts, int64_t n, const int32_t* d_on_target_idx, int64_t n_on_target,
                                   double* d_weighted, double* h_weights);
/* LSNormRatioCalculator.Run (mode 0, LSNormRatioCalculator.cs:20-48: library-size factor = reference median / sample median over the on-target
 * bins, bins whose reference count is below 1 are dropped) or RawRatioCalculator.Run (mode 1, RawRatioCalculator.cs:21-46: bins whose reference
 * count lies outside [min_ref, max_ref] are dropped), followed by CanvasNormalizeUtilities.RatiosToCounts (CanvasNormalizeUtilities.cs:23-33:
 * count = ratio * 40 * ploidy / 2; d_ploidy = reference copy number per bin from the ploidy VCF, NULL = 2).  d_sample / d_reference are the float
 * counts of the two .binned files.  Outputs (capacity n): d_keep_idx = indices of the bins that are kept, d_ratio / d_count per kept bin. */
int32_t canvas_normalize_ratio(canvas_ctx* ctx, int64_t n, const float* d_sample, const float* d_reference, const int32_t* d_on_target_idx, int64_t n_on_target,
                               int32_t mode, double min_ref, double max_ref, const int32_t* d_ploidy, int32_t* d_keep_idx, float* d_ratio, float* d_count,
                               int64_t* h_n_out, double* h_library_size_factor);
/* BestLR2ReferenceGenerator.Run for more than one control sample (BestLR2ReferenceGenerator.cs:31-80): weight = 1 / OnTargetMedianBinCount (0 if the
 * median is not positive) for the tumour and every normal, over the bins of d_on_target_idx (NULL: all bins); per normal the mean of
 * log(t*wt / (n*wn))^2 over the bins where n*wn > 0 and the term is finite (GetMeanSquaredLogRatios, :83-124; nBins > 0 ? sum / nBins : sum); the
 * smallest mean wins, the first normal a tie.  d_tumor / h_d_normals: device doubles (double.Parse of the 4th column, BinCounts.cs:51-52).  The sums
 * are taken in parallel with an error bound that covers the summation order and the device's log; the normals the bounds cannot separate from the
 * best one are replayed on the host in the reference's order with libm log, so *h_best is the reference's choice.  Outputs: *h_best, per normal
 * the mean (exact for the replayed ones) and the ignored-bin count (both optional), *h_replayed = how many normals were replayed (optional).
 * With one control sample the reference copies the file and never gets here. */
int32_t canvas_normalize_best_normal(canvas_ctx* ctx, const double* d_tumor, int32_t nnormals, const double* const* h_d_normals, int64_t n, const int32_t* d_on_target_idx,
                                     int64_t n_on_target, int32_t* h_best, double* h_mean_sq_log_ratio, int64_t* h_ignored, int32_t* h_replayed);
/* PCAReferenceGenerator.Run (PCAReferenceGenerator.cs:32-69) with the model of PCAModel.LoadModel (:92-127): d_sample = the sample's float counts
 * (float.Parse), d_mu = the model's float means, h_d_axes = naxes (1..64) device pointers to the raw axes (double.Parse), n = bins of the model.
 * The axes are normalised by their 2-norm (Utilities.NormalizeBy2Norm, an all-zero axis stays as it is); *h_orthogonal = 0 when a pair's
 * |DotProduct| exceeds 1e-4 (AreOrthogonal, :129-140: the reference throws) and nothing else is computed.  Otherwise: centred sample
 * max(1f, count) - mu, projection sizes DotProduct(x, unit axis) (h_sizes, optional), ref = max(1, mu + sum_k size_k * unit_k), its
 * "{F2}" text read back, RawRatioCalculator of the UNCLAMPED sample against it over [min_ref, max_ref] (RawRatioCalculator.cs:21-46),
 * *h_median_ratio = median of those ratios, d_reference[i] = (float)(ref[i] * medianRatio).  The 2-norms and the projection sizes are
 * sequential FP64 sums in the reference's order; the result is bit-identical to the reference's. */
int32_t canvas_normalize_pca_reference(canvas_ctx* ctx, int64_t n, const float* d_sample, const float* d_mu, int32_t naxes, const double* const* h_d_axes,
                                       double min_ref, double max_ref, float* d_reference, double* h_median_ratio, double* h_sizes, int32_t* h_orthogonal);

/* ---- multi-GPU (one process per GPU; chromosomes sharded across ranks) ------------------------------------------ */
int32_t canvas_comm_unique_id(void* h_id128);  /* ncclGetUniqueId, 128 bytes, rank 0 */
int32_t canvas_comm_init(canvas_ctx* ctx, int32_t rank, int32_t nranks, const void* h_id128);
/* transport for ranks that cannot form an RCCL communicator (several ranks on one GPU, a host with its own MPI): fn must all-gather bytes_per_rank bytes from
 * `send` of every rank into `recv` (rank order), host memory, and return 0.  The library stages the device buffers through pinned host memory around it. */
typedef int32_t (*canvas_host_allgather_fn)(void* user, const void* send, int64_t bytes_per_rank, void* recv);
int32_t canvas_comm_init_host(canvas_ctx* ctx, int32_t rank, int32_t nranks, canvas_host_allgather_fn fn, void* user);
/* Sub-communicators for samples x chromosome groups (BASELINE configs[3]; the reference runs the samples of a pedigree as independent CanvasBin / CanvasClean tasks,
 * CanvasRunner.cs:123-128): the ranks that pass the same color form an RCCL communicator of their own (ncclCommSplit), ordered by key, and every sharded call that
 * follows runs inside it; canvas_comm_restore goes back to the communicator of canvas_comm_init (the bin size of a pedigree and its bin intersection span all samples).
 * Collective over the parent communicator.  The host-callback transport has no split: its caller hands canvas_comm_init_host the callback of the group.
 * canvas_comm_rank: rank and size in the communicator the next collective will use. */
int32_t canvas_comm_split(canvas_ctx* ctx, int32_t color, int32_t key);
int32_t canvas_comm_restore(canvas_ctx* ctx);
int32_t canvas_comm_rank(canvas_ctx* ctx, int32_t* h_rank, int32_t* h_nranks);
/* the single RCCL all-gather of the path: every rank contributes nlocal int32 boundary records (padded to max_per_rank) */
int32_t canvas_allgather_boundaries(canvas_ctx* ctx, const int32_t* d_local, int32_t nlocal, int32_t max_per_rank,
                                    int32_t* d_all, int32_t* h_counts);

/* ONE sample, chromosomes sharded over the ranks (BASELINE configs[3], [4]): canvas_sample_pipeline for a rank that holds the per-base arrays of the
 * chromosomes with h_chr_owner[c] == its rank only (entries of the other chromosomes in d_bases / d_mask / d_hits are ignored; h_len, the autosome flags and the owner
 * table describe the whole genome and are the same on every rank).  The reference's per-chromosome tasks (CanvasBin.cs:513-539, HiddenMarkovModelsRunner.cs:51-104) run on
 * the owner; the genome-wide couplings are exchanged with three all-gathers on the communicator of canvas_comm_init / canvas_comm_init_host: the per-chromosome
 * (observed, possible) table (one bin size for everybody, CanvasBin.cs:73-83), the owned bins (16 B/bin), and — the collective north_star names — the segment boundary
 * records [n, (chr, startBin, endBin, state) ...] through canvas_allgather_boundaries.  CanvasClean runs on the gathered whole-genome SoA on every rank (deterministic,
 * redundant).  Every rank returns the same outputs as canvas_sample_pipeline on one GPU, bit for bit: all cleaned bins, coverage, states and the running segment ids
 * in file order (SegmentationResultsProcessor.cs:57-62).  Must be called by all ranks.  Modes 0 and 3. */
/* CanvasBin alone with the chromosomes sharded over the ranks (BASELINE configs[4]: the tumour's GCContentWeighted bins): canvas_bin_sample / canvas_bin_sample_gcweighted for
 * a rank that holds the arrays of its own chromosomes only; every rank ends with the bins of the whole genome in file order, bit-identical to the single-GPU call.
 * d_fraglen: mode 5 only (NULL otherwise).  Mode 5 adds two reductions over the ranks in front of the rate table: the per-chromosome NonZeroMeans of the fragment
 * lengths (MeanFragmentSize, CanvasBin.cs:164-174) and the 2 x 101 counters of the read-GC profile (CanvasBin.cs:372-391).  Must be called by all ranks; a failure on one
 * rank is announced in every exchange and fails all of them. */
int32_t canvas_bin_sample_sharded(canvas_ctx* ctx, int32_t nchr, const int32_t* h_chr_owner, const uint8_t* const* d_bases, const uint64_t* const* d_mask,
                                  const uint8_t* const* d_hits, const int16_t* const* d_fraglen, const int64_t* h_len, const uint8_t* h_chr_is_autosome,
                                  int32_t counts_per_bin, int32_t bin_size_in, int32_t mode, int32_t* d_chr, int32_t* d_start, int32_t* d_stop, int32_t* d_gc, float* d_count,
                                  int64_t cap, int32_t* h_bin_size, int64_t* h_nbins);
int32_t canvas_sample_pipeline_sharded(canvas_ctx* ctx, int32_t nchr, const int32_t* h_chr_owner, const uint8_t* const* d_bases, const uint64_t* const* d_mask,
                                       const uint8_t* const* d_hits, const int64_t* h_len, const uint8_t* h_chr_is_autosome, const uint8_t* h_chr_is_y,
                                       int32_t counts_per_bin, int32_t bin_size_in, int32_t mode, uint32_t clean_flags, int32_t min_bins_per_gc, int32_t max_inter_bin_dist,
                                       int32_t* d_chr, int32_t* d_start, int32_t* d_stop, int32_t* d_gc, float* d_count, int64_t cap,
                                       double* d_cov, int32_t* d_state, int32_t* d_segment_id,
                                       int32_t* h_bin_size, int64_t* h_nbins, int64_t* h_nbins_clean, double* h_local_sd, int64_t* h_chr_offset, int64_t* h_nsegments);
/* canvas_sample_pipeline_sharded over the packed planes of canvas_bin_sample_packed (0.75 B/base; d_ref / d_hit_planes / h_pos0 as for canvas_sample_pipeline_packed,
 * entries of the chromosomes this rank does not own are ignored): same exchanges, same outputs, bit for bit. */
int32_t canvas_sample_pipeline_sharded_packed(canvas_ctx* ctx, int32_t nchr, const int32_t* h_chr_owner, const uint64_t* const* d_ref, const uint64_t* const* d_hit_planes,
                                              const int64_t* h_len, const int64_t* h_pos0, const uint8_t* h_chr_is_autosome, const uint8_t* h_chr_is_y,
                                              int32_t counts_per_bin, int32_t bin_size_in, int32_t mode, uint32_t clean_flags, int32_t min_bins_per_gc, int32_t max_inter_bin_dist,
                                              int32_t* d_chr, int32_t* d_start, int32_t* d_stop, int32_t* d_gc, float* d_count, int64_t cap,
                                              double* d_cov, int32_t* d_state, int32_t* d_segment_id,
                                              int32_t* h_bin_size, int64_t* h_nbins, int64_t* h_nbins_clean, double* h_local_sd, int64_t* h_chr_offset, int64_t* h_nsegments);
/* last canvas_sample_pipeline_sharded call: [0] ranks, [1] chromosomes owned, [2] bins binned locally, [3] bytes this rank contributed to the bins all-gather,
 * [4] boundary records of this rank, [5] bytes per rank of the boundary all-gather */
int32_t canvas_sharded_stats(canvas_ctx* ctx, int64_t* h_out6);
/* CanvasPartition -m CBS / -m Wavelets with the chromosomes sharded over the ranks (the tumour / normal flow of BASELINE configs[4] ends in CBS, the
 * reference's default method is Wavelets).  d_cov / h_chr_offset describe the WHOLE cleaned coverage and are the same on every rank (what canvas_sample_pipeline_sharded
 * leaves everywhere); a rank segments the chromosomes with h_chr_owner[c] == its rank — the reference's own per-chromosome tasks (CBSRunner.cs:62-89, WaveletsRunner.cs:115-135)
 * — while everything that couples chromosomes is computed from the whole coverage on every rank: the per-chromosome seeds drawn in file order and the genome-wide trimmed SD of
 * SDUndo (CBSRunner.cs:102-112), the coverage variability (Segmentation.cs:297-330).  ONE exchange of variable-length lists (the mechanism of
 * canvas_allgather_boundaries) then gives every rank the complete result, identical to canvas_cbs_undo / canvas_wavelets on one GPU.  Must be called by all ranks; a rank
 * that fails locally still takes part in the exchange and every rank returns an error.  h_stats of canvas_cbs_sharded counts this rank's chromosomes only. */
int32_t canvas_cbs_sharded(canvas_ctx* ctx, int32_t nchr, const int32_t* h_chr_owner, const double* d_cov, const int64_t* h_chr_offset, double alpha, uint32_t nperm,
                           int32_t undo, double undo_sd, int32_t* d_seg_len, int32_t* h_nseg, int64_t* h_stats);
/* PerSampleHMM with the chromosomes sharded over the ranks, on a coverage EVERY rank holds (d_cov / h_chr_offset: the whole sample, h_chr_offset[0] = 0) — e.g. behind the bin
 * intersection of a pedigree, which lies between CanvasClean and CanvasPartition (Utilities.cs:834-920).  Emission parameters from the quartiles of the whole coverage
 * (HiddenMarkovModelsRunner.cs:36-50); a rank decodes its own chromosomes, one exchange of state runs gives every rank d_state[0 .. N): identical to canvas_hmm_per_sample. */
int32_t canvas_hmm_per_sample_sharded(canvas_ctx* ctx, int32_t nchr, const int32_t* h_chr_owner, const double* d_cov, const int64_t* h_chr_offset, int32_t* d_state);
int32_t canvas_wavelets_sharded(canvas_ctx* ctx, int32_t nchr, const int32_t* h_chr_owner, const double* d_cov, const int64_t* h_chr_offset, int32_t is_germline,
                                double threshold_lower, double threshold_upper, double mad_factor, int32_t variability_window, int32_t min_size,
                                int32_t* h_breakpoints, int64_t cap, int64_t* h_bp_offset);

/* The sample axis ("samples of a trio add a second axis"; BASELINE configs[3]): one sample of a pedigree per rank.  CanvasBin / CanvasClean / CanvasPartition of
 * a sample run on its rank with the single-GPU entry points; the two places where the reference couples the samples are exchanges:
 *   canvas_allgather_host         bytes_per_rank host bytes from every rank, rank order — the per-chromosome rates of canvas_bin_rates, from which every rank derives the
 *                                 multi-sample bin size (MultiSampleHitArrays / GetBinSize over all samples' autosomes, CanvasBin.cs:86-110) with canvas_bin_size_from_rates;
 *   canvas_merge_cleaned_sharded  MergeMultiSampleCleanedBedFile (Utilities.cs:834-920) with the samples in rank order: this rank's cleaned SoA in, the merged bin list
 *                                 (identical on every rank; capacity cap >= the first sample's bin count) and THIS sample's counts of the surviving bins out — what
 *                                 canvas_merge_cleaned returns for that sample on one GPU.  The (chr, start, stop) columns travel (12 B per bin), padded to the largest sample.
 * Both must be called by all ranks; a rank that fails locally announces it in the exchange and every rank returns an error. */
int32_t canvas_allgather_host(canvas_ctx* ctx, const void* h_send, int64_t bytes_per_rank, void* h_recv);
int32_t canvas_merge_cleaned_sharded(canvas_ctx* ctx, int64_t n_mine, const int32_t* d_chr, const int32_t* d_start, const int32_t* d_stop, const float* d_count,
                                     int32_t* d_out_chr, int32_t* d_out_start, int32_t* d_out_stop, float* d_out_count, int64_t cap, int64_t* h_n_out);

/* ---- CanvasSNV: allele counts at the sites of a VCF (SNVReviewer.ProcessBamFile + ProcessReadBases, CanvasSNV/SNVReviewer.cs:172-271) ---------------- */
/* One chunk of one chromosome's alignments as RAW BAM record bytes (SAM specification 4.2, each record with its block_size word, exactly as BGZF inflation
 * leaves them) plus the byte offset of every record in the chunk; no field is decoded on the host.  Records and sites must be sorted by position (the
 * caller's to check: any indexed BAM and sorted VCF are); then the result equals the reference's sequential scan.
 *   sites       d_site_pos: one-based positions, non-decreasing, duplicates allowed (each is a site of its own); d_site_ref / d_site_alt: the BAM 4-bit code of
 *               the allele's character ("=ACMGRSVTWYHKDBN" -> 0..15), 0xFF for any other character (lower case included: the reference compares chars)
 *   filters     flag & 0x100 / 0x4 / 0x400 and mapq <= min_mapq are skipped; records of another refID or without a position as well
 *   counters    d_ref_counts / d_alt_counts (int32 per site) are ADDED to, never cleared: a chromosome is any number of chunks
 *   h_info      NULL: the call only queues work on the context's stream (counters complete after canvas_synchronize).  Otherwise int64[5], valid on return
 *               (the call waits): records seen, passed the filters, walked (a site within reach: SNVReviewer.cs:206-213), whose walk ended at a CIGAR operation
 *               other than M/I/D/S (:266-268), rejected as malformed (an offset, block_size, name / CIGAR / sequence length that does not fit the record or the
 *               chunk, or a CIGAR that consumes more bases than l_seq: such a record is skipped whole and never read past its bounds).  The CIGAR
 *               is only read for records that are walked, so a record whose CIGAR outruns l_seq but has no site within reach counts as passed, not as malformed:
 *               that one figure depends on the site list; the counters do not (such a record touches no site either way). */
int32_t canvas_snv_count(canvas_ctx* ctx, const uint8_t* d_records, uint64_t nbytes, const uint64_t* d_record_offsets, int64_t nrecords, int32_t ref_id,
                         int32_t min_mapq, int32_t min_base_q, const int32_t* d_site_pos, const uint8_t* d_site_ref, const uint8_t* d_site_alt, int32_t nsites,
                         int32_t* d_ref_counts, int32_t* d_alt_counts, int64_t* h_info);

/* ---- CanvasBin: observed-alignment arrays from BAM records (LoadObservedAlignmentsBAM, CanvasBin/CanvasBin.cs:207-275) ------------------------------ */
/* One chunk of alignments as RAW BAM record bytes plus the byte offset of every record: the chunk format of canvas_snv_count, no field decoded on the host.
 * A chromosome is any number of chunks, in file order, starting anywhere at or before its first record.  d_hits (uint8 per base) and d_frag (int16 per base,
 * mode 5 only, NULL otherwise) are UPDATED and never cleared: the caller zeroes them, and zeroes d_state (8 words) before the first chunk of a chromosome.
 *   per record  in file order (CanvasBin.cs:235-272): counted as seen; skipped on flag 0x4 / 0x200 / 0x400 / 0x10 / 0x900, on n_cigar == 0, on a first CIGAR
 *               operation that is not M or is shorter than 35, and with paired_end on a missing 0x2; a record that passed all of these and has refID != ref_id
 *               STOPS the chromosome: it is seen, and nothing behind it counts or writes, in this chunk or a later one (a skipped record of another reference
 *               does not stop); otherwise the record is kept.  A kept record with pos outside [0, len) is counted and writes nothing (the reference throws).
 *   writes      mode 0 (Binary): hits[pos] = 1.  Modes 3 and 5: hits[pos] = min(255, hits[pos] + 1) (an atomic update of the aligned 32-bit word that holds
 *               the byte: nothing else may write the up to three bytes in front of d_hits[0] or behind d_hits[len - 1] in that word while a call runs).
 *               Mode 5 (GCContentWeighted) also frag[pos] = clamp(tlen, 0, 32767) of the LAST kept record of the position in file order.
 *   order       hits is right for records in ANY order (a saturating count does not depend on it).  frag requires the positions of the kept records to be
 *               non-decreasing within and across the chunks of a chromosome (the caller's to check: any indexed BAM is).
 *   malformed   an offset that does not leave 4 + 32 bytes inside nbytes, a block_size below 32 or past the chunk, a record whose 32 + l_read_name + 4 n_cigar
 *               exceeds block_size: skipped whole, counted, never read past its bounds (as in canvas_snv_count).
 *   d_state     device memory, accumulated over the chunks, written by the kernels only: [0] stopped (0 / 1), [1] records seen (up to and including the stopping
 *               one), [2] kept, [3] kept but out of range, [4] malformed, [5] position of the last kept record, [6] [7] reserved (the library's own).
 *   h_info      NULL: the call only queues work on the context's stream (arrays and state complete after canvas_synchronize).  Otherwise int64[8]: the call
 *               waits and copies d_state out.
 * CANVAS_ERR_INVALID: NULL context or buffers, mode not 0 / 3 / 5, mode 5 without d_frag, len outside [0, 2^31). */
int32_t canvas_hits_from_bam(canvas_ctx* ctx, const uint8_t* d_records, uint64_t nbytes, const uint64_t* d_record_offsets, int64_t nrecords, int32_t ref_id,
                             int32_t paired_end, int32_t mode, int64_t len, uint8_t* d_hits, int16_t* d_frag, int64_t* d_state, int64_t* h_info);

/* ---- CanvasBin -m Fragment: fragment counts of predefined bins from BAM records (FragmentBinner.BinTask, CanvasBin/FragmentBinner.cs:186-369) -------- */
/* One chunk of one chromosome in the chunk format above.  d_bin_start / d_bin_stop: the chromosome's BED bins in FILE order (not assumed sorted or disjoint).
 * d_count (int32 per bin), d_carry and d_state (16 words) carry over from chunk to chunk; the caller zeroes d_count and d_state before the first chunk.
 *   stop        the first record with refID != ref_id stops the chromosome (every record counts here, filtered or not): it is seen, nothing behind it has any
 *               effect, in this chunk or a later one.
 *   per record  before the stop: counted in `paired` on flag 0x1; checked for sortedness; skipped on 0x4 / 0x8 / 0x100 or unless 0x1 and 0x2 are both set
 *               (0x800 passes, as in the reference).  The surviving records drive, per READ NAME (the l_read_name - 1 bytes at offset 36, compared as bytes) and in
 *               file order, BinOneAlignment: bad = flag & 0x600 || mapq == 255 || mapq < quality_threshold.  Name binned: undo the count when bad, forget the name.
 *               Otherwise done when bad, refID != next_refID or pos > next_pos; pos == next_pos toggles the same-position state and is done when it was set; done when
 *               tlen == 0; otherwise the fragment [pos, pos + tlen) (32-bit wrap-around) goes to FindBestBin from the first bin whose running maximum of Stop exceeds
 *               pos: largest overlap, the first bin on ties, the walk ends at the first bin with overlap <= 0.  A hit: count[best]++, usable++, the name is binned.
 *   carry       after a chunk every name that is binned or in the same-position set is an entry of d_carry (8-byte aligned; layout: the library's own, with the name bytes);
 *               resolved names leave it.  If the entries do not fit in carry_capacity the call returns CANVAS_ERR_CAPACITY with d_count, d_carry and d_state
 *               UNCHANGED and h_info[8] = the bytes needed: enlarge the buffer, keep its contents, repeat the call.
 *   sortedness  a record (before the stop) whose pos is below the previous record's sets d_state[6] to 1 + its ordinal among the records seen; the counts are void
 *               from then on (the reference throws).
 *   malformed   as in canvas_hits_from_bam: skipped whole, counted, never read past their bounds.
 *   d_state     [0] stopped, [1] seen, [2] paired, [3] usable fragments (net), [4] malformed, [5] last position, [6] unsorted, [7] carried entries, [8] carry bytes
 *               used, [9] groups in which a byte comparison separated names of equal hash, [10] longest group, [11..15] the library's own.
 *   h_info      int64[16], required: the call always waits (it has to know the carry's size before it commits) and copies d_state out.
 * CANVAS_ERR_INVALID: NULL context or buffers, ref_id < 0, nbins outside [0, 2^31), quality_threshold < 0. */
int32_t canvas_fragments_from_bam(canvas_ctx* ctx, const uint8_t* d_records, uint64_t nbytes, const uint64_t* d_record_offsets, int64_t nrecords, int32_t ref_id,
                                  const int32_t* d_bin_start, const int32_t* d_bin_stop, int64_t nbins, int32_t quality_threshold, int32_t* d_count,
                                  uint8_t* d_carry, uint64_t carry_capacity, int64_t* d_state, int64_t* h_info);

/* ---- reference preparation: Tools/FlagUniqueKmers ---------------------------------------------------------------------- */
/* Tools/FlagUniqueKmers (KmerChecker.cs): d_mask[c] (ceil(len/64) words, BitArray layout, bits >= len written 0) gets bit p = 1 iff position p of
 * chromosome c starts a 35-mer whose canonical key occurs once in the whole input.  d_bases: ASCII, any case, not modified.
 * max_table_bytes: bound of the working table (0 = chosen from free device memory); any value that holds one key class must give the same mask.
 * h_stats[8]: positions, keyed positions, unique positions, passes, table slots, longest probe, table bytes, reserved.
 * Rules (KmerChecker.cs:124,136,147-154 and GetKeyForKmer, :30-105): bases are upper-cased first; position p of a contig of length L is keyed when p + 35 < L and
 * its 35 bases are all of A C G T; a keyed position is flagged when no other keyed position of any contig carries the same 35-mer or its reverse complement.
 * A contig of length 0 has no words (its pointers are not looked at); a single contig is shorter than 2^31.  A budget that does not hold the largest of the 1 024
 * key classes returns CANVAS_ERR_CAPACITY (the message names the bytes needed) and writes no mask.  The call waits for its result. */
int32_t canvas_flag_unique_kmers(canvas_ctx* ctx, int32_t nchr, const uint8_t* const* d_bases, const int64_t* h_len,
                                 uint64_t* const* d_mask, int64_t max_table_bytes, int64_t* h_stats);
/* inverse of canvas_mask_from_fasta: ASCII letters of d_bases become upper case where the mask bit is 1 and lower case where it is 0, in place */
int32_t canvas_fasta_case_from_mask(canvas_ctx* ctx, uint8_t* d_bases, int64_t len, const uint64_t* d_mask);

/* ---- CanvasSmooth: repeated median filter of the bin counts (CanvasSmooth/CanvasSmooth.cs:46-77, CanvasCommon/Utilities.cs:767-791) -------------------- */
/* CanvasSmooth (CanvasSmooth.cs:46-77, Utilities.MedianFilter): h = 1..max_half_window over each chromosome's counts.
 * d_out[h_chr_offset[c] + k], k < h_out_n[c], = the smoothed counts; the rest of d_out is left untouched. d_out must not overlap d_count.
 * A chromosome shorter than 2h + 1 at some pass comes out shorter (the reference's Enumerable.Zip drops the bins beyond the filter's output): h_out_n[c] is the
 * length that is left, possibly 0.  max_half_window = 0 copies the counts.  Counts must be finite (CANVAS_ERR_INVALID names the first index that is not); -0.0
 * compares equal to 0.0 and either may come out.  CANVAS_ERR_INVALID as well for a negative max_half_window, offsets that decrease, a chromosome of 2^31 bins or
 * more, and a d_out that overlaps d_count.  The call waits for its result. */
int32_t canvas_smooth(canvas_ctx* ctx, int32_t nchr, const int64_t* h_chr_offset /* nchr+1 */, const float* d_count,
                      int32_t max_half_window, float* d_out, int64_t* h_out_n /* nchr */);
/* host only, no context: the output length of every chromosome: per pass h, n stays when n >= 2h + 1 and becomes max(0, n-h) + max(0, n-h-1) otherwise */
int32_t canvas_smooth_lengths(int32_t nchr, const int64_t* h_n, int32_t max_half_window, int64_t* h_out_n);
/* host only: how canvas_smooth will run for this W. h_out4 = { fused (0/1), tile payload in bins, halo in bins per side, launches }
 * (per-pass path: launches = max_half_window, an upper bound: the passes end once every chromosome is empty; 0 = a copy) */
int32_t canvas_smooth_plan(int32_t max_half_window, int64_t* h_out4);

/* ---- CanvasDiploidCaller: per-segment order statistics (CanvasDiploidCaller.cs AssignPloidyCallsDistance, CanvasSegment.cs MedianCount / WriteCoveragePlotData) ---- */
#define CANVAS_SELECT_MEDIAN_F32 0 /* a[n/2] for odd n, (a[n/2-1] + a[n/2]) / 2 averaged in float for even n: Utilities.Median(IEnumerable<float>) */
#define CANVAS_SELECT_MEDIAN_F64 1 /* the same with the average taken in double: the median of floats widened into a List<double> */
#define CANVAS_SELECT_UPPER 2      /* a[n/2] of the sorted values (CanvasSegment.cs:696-697) */
/* Exact order statistics of nseg segments of a float32 device array in a fixed sequence of launches (at most 11, whatever nseg is): segment s is
 * d_values[h_seg_offset[s] .. h_seg_offset[s+1]); d_out[s] (double, device) = its statistic — an order statistic is a value of the array bit for bit, widened; the
 * averages are ((double)(float)((a + b) / 2f)) and ((double)a + (double)b) / 2.  An empty segment gives 0 and is counted in *h_nempty (may be NULL).  -0.0 sorts in front of 0.0.
 * Values must be finite (CANVAS_ERR_INVALID names the first index that is not); CANVAS_ERR_INVALID as well for a mode outside 0..2, a negative first offset, offsets that
 * decrease, or 2^31 segments and more — all of that is decided first, before the context is looked at (a NULL ctx returns CANVAS_ERR_INVALID too, but only after
 * *h_nempty has been written for offsets that passed).  The call waits for its result. */
int32_t canvas_segment_select(canvas_ctx* ctx, const float* d_values, int64_t nseg, const int64_t* h_seg_offset /* nseg+1 */, int32_t mode, double* d_out /* nseg */,
                              int64_t* h_nempty);
/* host only, no context: h_out6 = { largest segment of the wave class (rank counting inside a wave), largest segment of the LDS class (staged once, radix-selected in LDS),
 * keys per tile of the tiled multi-pass class above that, launches at most, class forced by the CANVAS_CALL_CLASS test hook (0 none, 1 wave, 2 lds, 3 tiled), 0 } */
int32_t canvas_segment_select_plan(int64_t* h_out6);

/* CanvasDiploidCaller.CallVariants between "files parsed" and "files written" (CanvasDiploidCaller.cs:295-343) on device-resident bins and sites.
 * Bins: d_count[nbins] (float).  Segments (host tables, grouped by chromosome: those of chromosome c are h_chr_seg_offset[c] .. h_chr_seg_offset[c+1]): zero-based
 * h_seg_begin / h_seg_end and the bins h_seg_bin_offset[s] .. h_seg_bin_offset[s+1] (offsets from 0 to nbins, at least one bin each).  Sites of chromosome c:
 * h_chr_site_offset[c] .. [c+1] of d_site_pos (one-based) / d_site_ref / d_site_alt.  h_logistic4 = LogisticGermline{Intercept, LogBinCount, ModelDistance, DistanceRatio}.
 * A site with ref + alt >= 10 belongs to the first segment of its chromosome with End > position if that segment's Begin <= position (IO.cs:156-176, the one-based /
 * zero-based comparison kept); Frequency = alt / (float)(ref + alt), folded as f > 0.5 ? 1 - f : f in float.
 * Per segment (arrays of nseg): median count (Utilities.Median(float)), h_seg_site_offset[nseg+1] (kept sites in front of each segment), informative (nMaf >=
 * max(10, (End-Begin)/463/2)), median folded frequency (double average; -1 when not informative), copy number and major chromosome count of the nearest of the 36 model
 * points (MCC -1 when fewer than 10 sites), its distance and the runner-up's, the LogisticGermline q-score.
 * Per merged run (MergeSegments with its defaults: same chromosome, same CN, Begin - run.End < 10000; arrays of nseg, *h_nruns filled): first and last segment (the run
 * spans Begin of the first to End of the last and takes their confidence intervals), q-score recomputed with the run's bin count, filter bits (1 = q10, 2 = L10kb), median
 * count (double average).  h_scalars2 = { diploidCoverage (bit-equal to the serial Utilities.Mean(float[])), MeanCoverage }; h_info4 (may be NULL) = { kept sites, 1 when
 * diploidCoverage came from the exact integer sum on the device and 0 when the counts were summed on the host in bin order, coverage sum of the kept sites, 0 }.
 * CANVAS_ERR_INVALID (checked on the host tables before the context is looked at unless marked *; *h_nruns is set to 0 once they have passed, also with a NULL ctx): offsets that do not start at 0 / decrease / do not end at nbins, no segment, a segment without
 * bins or with End < Begin, begins that decrease or ends that do not increase within a chromosome (MergeIn would drop the bins of a segment that ends where its
 * predecessor ends), * positions that decrease within a chromosome or negative counts (the message names the site), * no kept site, * a non-finite count.
 * The call waits three times (site table and scalars; per-segment results; run medians). */
int32_t canvas_call_diploid(canvas_ctx* ctx, int64_t nbins, const float* d_count, int32_t nchr, const int64_t* h_chr_seg_offset /* nchr+1 */, const int32_t* h_seg_begin,
                            const int32_t* h_seg_end, const int64_t* h_seg_bin_offset /* nseg+1 */, const int64_t* h_chr_site_offset /* nchr+1 */, const int32_t* d_site_pos,
                            const int32_t* d_site_ref, const int32_t* d_site_alt, const double* h_logistic4,
                            double* h_seg_median_count, int64_t* h_seg_site_offset /* nseg+1 */, int32_t* h_seg_informative, double* h_seg_median_maf, int32_t* h_seg_cn,
                            int32_t* h_seg_mcc, double* h_seg_dist, double* h_seg_dist2, int32_t* h_seg_qscore,
                            int64_t* h_nruns, int64_t* h_run_first, int64_t* h_run_last, int32_t* h_run_qscore, int32_t* h_run_filter, double* h_run_median_count,
                            double* h_scalars2, int64_t* h_info4);

/* Segments.ReadSegments (CanvasCommon/Segments.cs:52-115) on device-resident bins: the host segment tables canvas_call_diploid / canvas_call_somatic take, from the per-bin
 * d_segment_id every partition entry leaves (canvas_sample_pipeline, canvas_segment_ids*, ...).  Bins: d_start / d_stop / d_segment_id (int32[nbins]) grouped by chromosome,
 * h_chr_offset[nchr+1] as canvas_chromosome_offsets returns it (empty chromosomes anywhere).  Bin i starts a segment when it is the first bin of its chromosome or
 * d_segment_id[i] != d_segment_id[i-1] (GroupByAdjacent: only adjacency counts; an id that returns is a new segment, negative ids are ordinary values).
 * *h_nseg = segments; h_chr_seg_offset[nchr+1] = segments in front of each chromosome; per segment Begin (start of its first bin), End (stop of its last bin),
 * h_seg_bin_offset[nseg+1] (index of its first bin; [nseg] = nbins) and h_seg_ci4 = { start.lo, start.hi, end.lo, end.hi } (GetStartConfidenceInterval / GetEndConfidenceInterval:
 * half length = (int)Math.Round((stop - start) / 2.0, AwayFromZero); the neighbouring bin is used only when it lies in the same chromosome and abuts).  The per-segment arrays
 * hold cap_seg entries (h_seg_bin_offset cap_seg + 1, h_seg_ci4 4 * cap_seg); the copies from the device are sized by min(cap_seg, nbins) because the count is known only after
 * the wait, so cap_seg is best near the expected count (a refused call reports the count).  d_cov (double[nbins], may be NULL) given: d_count_f32[i] = (float)d_cov[i] (device,
 * nbins floats, caller-owned) — for a canvas_quantize_f2 coverage that is float.Parse of the text CanvasPartition writes (DESIGN 4 "Segment tables").
 * CANVAS_ERR_INVALID, decided on the host arguments before the context is looked at (*h_nseg untouched): nbins < 1, a negative cap_seg, h_chr_offset that does not start
 * at 0 / decreases / does not end at nbins.  Decided on the device (*h_nseg is written, the tables are not): a start that decreases within a chromosome (the message names
 * the first such bin), stop < start, a non-finite d_cov, nseg >= 2^31, nseg > cap_seg.  The call waits once. */
int32_t canvas_segment_tables(canvas_ctx* ctx, int64_t nbins, int32_t nchr, const int64_t* h_chr_offset /* nchr+1 */, const int32_t* d_start, const int32_t* d_stop,
                              const int32_t* d_segment_id, const double* d_cov, int64_t cap_seg, int64_t* h_nseg, int64_t* h_chr_seg_offset /* nchr+1 */, int32_t* h_seg_begin,
                              int32_t* h_seg_end, int64_t* h_seg_bin_offset /* cap_seg+1 */, int32_t* h_seg_ci4 /* 4*cap_seg */, float* d_count_f32);
/* canvas_segment_tables, then canvas_call_diploid on the tables and the float counts it left: the bins' arrays, cap_seg and the table outputs of the former (d_cov and d_count_f32
 * are required), the sites, coefficients and outputs of the latter (arrays of cap_seg entries, h_seg_site_offset cap_seg + 1).  The refusals of both, in that order.  The call
 * waits four times. */
int32_t canvas_call_diploid_ids(canvas_ctx* ctx, int64_t nbins, int32_t nchr, const int64_t* h_chr_offset /* nchr+1 */, const int32_t* d_start, const int32_t* d_stop,
                                const int32_t* d_segment_id, const double* d_cov, int64_t cap_seg, const int64_t* h_chr_site_offset /* nchr+1 */, const int32_t* d_site_pos,
                                const int32_t* d_site_ref, const int32_t* d_site_alt, const double* h_logistic4,
                                int64_t* h_nseg, int64_t* h_chr_seg_offset /* nchr+1 */, int32_t* h_seg_begin, int32_t* h_seg_end, int64_t* h_seg_bin_offset /* cap_seg+1 */,
                                int32_t* h_seg_ci4 /* 4*cap_seg */, float* d_count_f32,
                                double* h_seg_median_count, int64_t* h_seg_site_offset /* cap_seg+1 */, int32_t* h_seg_informative, double* h_seg_median_maf, int32_t* h_seg_cn,
                                int32_t* h_seg_mcc, double* h_seg_dist, double* h_seg_dist2, int32_t* h_seg_qscore,
                                int64_t* h_nruns, int64_t* h_run_first, int64_t* h_run_last, int32_t* h_run_qscore, int32_t* h_run_filter, double* h_run_median_count,
                                double* h_scalars2, int64_t* h_info4);

/* ---- CanvasSomaticCaller: the purity / ploidy model fit (CanvasSomaticCaller/SomaticCaller.cs:1870-2117, ModelOverallCoverageAndPurity's grid search) ---- */
#define CANVAS_SOMATIC_TILE 256                /* segments per tile of the device kernel: more segments than this take its tile loop */
#define CANVAS_SOMATIC_MAX_CN 10               /* largest MaximumCopyNumber: PercentCN rows always hold CANVAS_SOMATIC_MAX_CN + 1 entries (0 beyond MaximumCopyNumber) */
#define CANVAS_ERR_SOMATIC_NO_MODEL (-6)       /* no model passes the ploidy filter (the reference throws UncallableDataException, :1934-1937) */
#define CANVAS_ERR_SOMATIC_NO_SCORE (-7)       /* no model scores above 0 (the reference dereferences a null bestModel, :2061) */
#define CANVAS_SOMATIC_INFO_CLUSTER_TERM 1u    /* result.info: not enrichment, more than 100 segments and more than 100 with a MAF: the reference would have added ClusterDeviation */
#define CANVAS_SOMATIC_INFO_INDEX_CUTOFF 2u    /* result.info: fewer than DeviationIndexCutoff models within DeviationFactor, worstAllowedDeviation came from the sorted deviations */
#define CANVAS_SOMATIC_MODEL_VALID 1           /* models.flags: passed the ploidy filter (allModels) */
#define CANVAS_SOMATIC_MODEL_SCORED 2          /* models.flags: Deviation <= worstAllowedDeviation, has a score (bestModels; a row of PurityModel.txt) */
/* SomaticCallerParameters as this entry reads them; the comments give SomaticCallerParameters.json */
typedef struct canvas_somatic_params {
    int32_t maximum_copy_number;               /* 8; 2 .. 10 */
    int32_t deviation_index_cutoff;            /* 11 */
    int32_t maximum_related_models;            /* 5; 1 .. 64 */
    float min_allowed_ploidy;                  /* 0.5 */
    float max_allowed_ploidy;                  /* 8 */
    float deviation_factor;                    /* 1.75 */
    double cn2_weighting_factor;               /* 0.175 */
    double deviation_score_weighting_factor;   /* 0.375 */
    double diploid_distance_score_weighting_factor; /* 0.125 */
    double heterogeneity_score_weighting_factor;    /* 0.202 (multiplies a heterogeneity index that is 0 here) */
} canvas_somatic_params;
/* the scalars of the search and its grid: diploid coverage min_coverage .. max_coverage, and per coverage the purities
 * (int)max(minimum_purity_hard_limit, 100 * (1 - 2 * min_minor_allele_coverage / coverage) - 10) .. 100 percent (:1907) */
typedef struct canvas_somatic_grid {
    int32_t min_coverage, max_coverage;        /* 1 .. 100000 */
    int32_t minimum_purity_hard_limit;         /* 5 or 20 in the reference; 0 .. 99 */
    int32_t fixed_percent_purity;              /* < 0: none; else the one purity of every coverage, (int)(userPurity * 100) */
    int32_t fixed_coverage;                    /* < 0: none; else the one coverage, (int)GetDiploidCoverage(median, userPloidy) */
    int32_t is_enrichment;
    double min_minor_allele_coverage;
    double coverage_weighting_factor;          /* CoverageWeightingFactor: already divided by the median coverage level */
    int64_t genome_length;
} canvas_somatic_grid;
typedef struct canvas_somatic_result {
    int32_t best_model;                        /* index in grid order (coverage outer, purity inner); -1 when there is none */
    int32_t best_coverage, best_percent_purity;
    uint32_t info;                             /* CANVAS_SOMATIC_INFO_* */
    int32_t nmodels, nvalid, nscored, reserved;
    /* the best model's CoveragePurityModel */
    double diploid_coverage, purity /* percent / 100f, widened */, deviation, precision_deviation, accuracy_deviation, ploidy, percent_normal, diploid_distance;
    double percent_cn[CANVAS_SOMATIC_MAX_CN + 1];
    double score, inter_model_distance;
    double best_deviation, worst_allowed_deviation;
    double host_table_ms, upload_ms, device_ms, selection_ms;   /* wall time of the call's four parts */
} canvas_somatic_result;
/* every model's columns of PurityModel.txt, in grid order; any pointer may be NULL */
typedef struct canvas_somatic_models {
    int64_t capacity;                          /* models each array holds; CANVAS_ERR_CAPACITY when the grid has more */
    int32_t* coverage; int32_t* percent_purity;
    double* deviation; double* precision_deviation; double* accuracy_deviation; double* ploidy; double* percent_normal;
    double* percent_cn;                        /* capacity * (CANVAS_SOMATIC_MAX_CN + 1) */
    double* diploid_distance;
    int32_t* flags;                            /* CANVAS_SOMATIC_MODEL_* */
    double* score;                             /* 0 where the model has none */
} canvas_somatic_models;
/* Fits every (diploid coverage, purity) model of the grid to nseg usable segments and selects the best one.  coverage / maf (< 0: none) / weight (double) and length
 * (int32, End - Begin) are device arrays when inputs_on_device is not 0 and host arrays otherwise.
 * Per model, bit for bit as the reference: the model points in InitializePloidies' order with InitializeModelPoints(model) and AdjustedMAF (host libm, host threads, one
 * upload); on the device RefineDiploidMAF, the clustering loop of ModelDeviation, the accuracy deviation, PercentCN, Ploidy, PercentNormal, Deviation = 0.5f * precision +
 * 0.5f * accuracy and DiploidModelDistance, every sum over segments in segment order, without fused multiply-adds.  On the host the selection of :1921-2116: ploidy filter,
 * worstAllowedDeviation with the DeviationIndexCutoff fallback, the four sub-scores, the first model with the strictly highest score, and InterModelDistance over the
 * first MaximumRelatedModels models of the stable order by -score.  h_seg_point / h_seg_distance (nseg each, may be NULL): the best model's info.Ploidy.Index and
 * info.Distance after the final ModelDeviation call.
 * NOT built: the cluster term of ModelDeviation (ClusterDeviation, :1309-1313, needs the centroids of the mean-shift / density clustering).  The result equals the
 * reference's where the reference skips that term: enrichment data, at most 100 segments, or at most 100 segments with a MAF.  Otherwise the two-term deviation is still
 * computed and CANVAS_SOMATIC_INFO_CLUSTER_TERM is set.  The ploidies' pure-tumour MinorAlleleFrequency (EstimateDiploidMAF of MeanCoverage) is not an input: the
 * search never reads it (InitializeModelPoints(model) takes every point's MAF from AdjustedMAF).  The de-duplicated-model probe (:2058-2080) only logs and is left out.
 * CANVAS_ERR_INVALID: nseg < 3, a total weight of 0, a negative length or one whose product with MaximumCopyNumber leaves int32, a coverage or weight that is not finite
 * or a MAF that is NaN, an empty grid, a parameter outside the ranges above.  All of that except the segment checks of device inputs is decided before the context
 * is looked at; *h_result is then cleared and nmodels set, also with a NULL ctx (which returns CANVAS_ERR_INVALID).  CANVAS_ERR_SOMATIC_NO_MODEL / _NO_SCORE: the
 * per-model arrays and nmodels / nvalid / nscored are filled, best_model is -1.  The call waits for its result. */
int32_t canvas_somatic_model_fit(canvas_ctx* ctx, int64_t nseg, const double* coverage, const double* maf, const double* weight, const int32_t* length,
                                 int32_t inputs_on_device, const canvas_somatic_grid* grid, const canvas_somatic_params* params, canvas_somatic_result* h_result,
                                 int32_t* h_seg_point, double* h_seg_distance, const canvas_somatic_models* h_models);

/* ---- CanvasSomaticCaller: the calls around the fit (SomaticCaller.cs CallVariants :366-476 between "files parsed" and "files written") ---- */
#define CANVAS_ERR_SOMATIC_FEW_SEGMENTS (-8)   /* fewer than 3 usable segments (NotEnoughUsableSegementsException, :1636): stages 1 and 2 are filled */
#define CANVAS_SOMATIC_MEAN_NONE (-1)          /* seg_mean_route: the best ploidy is not MaximumCopyNumber, MeanCount was not needed (seg_mean_count is 0) */
#define CANVAS_SOMATIC_MEAN_WALK 0             /* ... summed by one lane in bin order */
#define CANVAS_SOMATIC_MEAN_EXACT 1            /* ... summed as integers of 2^e by the whole workgroup, after the proof that every partial sum of the serial loop is exact */
typedef struct canvas_somatic_call_params {
    canvas_somatic_params fit;                 /* deviation_factor is replaced by 2 when there are fewer than 500 segments (:375) */
    int32_t minimum_variant_frequencies;       /* MinimumVariantFrequenciesForInformativeSegment, 50 */
    int32_t minimum_call_size;                 /* 50000 */
    int32_t quality_filter_threshold;          /* 10 */
    int32_t merge_span;                        /* maximumMergeSpan of the enrichment merge: 1 in the reference */
    int32_t is_enrichment;
    int32_t minimum_purity_hard_limit;         /* from the clustering, caller-supplied: 5 or 20 in the reference */
    float lower_coverage_level_weighting_factor; /* 4 */
    float upper_coverage_level_weighting_factor; /* 2.355 */
    float user_purity;                         /* negative: none */
    float user_ploidy;                         /* negative: none */
    double coverage_weighting;                 /* 0.333 */
    double coverage_weighting_with_maf_segmentation; /* 0.20 */
    double evenness_score_threshold;           /* 94.5 */
    double min_evenness_score;                 /* 88 */
    double logistic_intercept;                 /* -0.5143 */
    double logistic_log_bin_count;             /* 0.8596 */
    double logistic_model_distance;            /* -50.4366 */
    double logistic_distance_ratio;            /* -0.6511 */
    double evenness_score;                     /* NaN: none */
    double snv_purity_estimate;                /* NaN: none */
    double min_minor_allele_coverage;          /* from the clustering, caller-supplied */
    int64_t genome_length;
} canvas_somatic_call_params;
/* host arrays the call fills; every pointer is required.  Per-segment arrays hold nseg entries (seg_site_offset nseg + 1), per-run arrays nseg entries of which nruns are filled */
typedef struct canvas_somatic_call_out {
    double* seg_median_count;                  /* stage 1: Utilities.Median(float) of the counts */
    int64_t* seg_site_offset;                  /* stage 1: kept sites in front of each segment */
    double* seg_maf_upper;                     /* stage 1: a[n/2] of the folded frequencies (0 without a site) */
    int32_t* seg_usable;                       /* stage 2 */
    double* seg_coverage;                      /* stage 2: info.Coverage (every segment) */
    double* seg_maf;                           /* stage 2: info.Maf under the threshold finally used (every segment) */
    double* seg_weight;                        /* stage 2: info.Weight (every segment) */
    int32_t* seg_cn;                           /* stage 5: CopyNumber (after the MaximumCopyNumber rule) */
    int32_t* seg_cn2;                          /* stage 5: SecondBestCopyNumber (-1: none) */
    int32_t* seg_mcc;                          /* stage 5: MajorChromosomeCount (-1: null) */
    double* seg_dist;                          /* stage 5: ModelDistance */
    double* seg_dist2;                         /* stage 5: RunnerUpModelDistance */
    double* seg_mean_count;                    /* stage 5: MeanCount where it was needed */
    int32_t* seg_mean_route;                   /* stage 5: CANVAS_SOMATIC_MEAN_* */
    int32_t* seg_qscore;                       /* stage 6: Logistic q-score of the segment */
    int64_t* seg_run;                          /* stage 6: the run the segment went to */
    int64_t* run_owner;                        /* stage 6: the segment whose call (CN, MCC, distances) the run carries */
    int32_t* run_begin;
    int32_t* run_end;
    int64_t* run_bin_count;                    /* what MergeIn left in GenomicBins: a segment merged in without moving Begin or End adds no bins */
    int32_t* run_qscore;
    int32_t* run_filter;                       /* 1 = q<threshold>, 2 = L10kb */
} canvas_somatic_call_out;
typedef struct canvas_somatic_call_scalars {
    int64_t nruns, nusable, kept_sites;
    int32_t stages;                            /* stages filled: 0, 2, 3 or 6 */
    int32_t threshold_used;                    /* stage 2: MinimumVariantFrequenciesForInformativeSegment after the loop of :1626-1634 */
    int32_t median_coverage_level;             /* stage 3 */
    int32_t min_coverage, max_coverage;        /* stage 3: the grid's coverages (equal with a user ploidy) */
    int32_t fixed_percent_purity;              /* stage 3: (int)(userPurity * 100), or -1 */
    float overall_median_coverage;             /* stage 2: Quartiles(...).Item2 */
    float deviation_factor;                    /* stage 3 */
    double mean_coverage;                      /* stage 1: MeanCoverage */
    double coverage_weighting_factor;          /* stage 3 */
    double reported_purity;                    /* stage 6: ##EstimatedTumorPurity (after SelectPurityEstimate) */
    double purity_model_fit;                   /* stage 6: ##PurityModelFit */
    double inter_model_distance;               /* stage 6: ##InterModelDistance */
    double estimated_chromosome_count;         /* stage 6: ##EstimatedChromosomeCount */
    double heterogeneity_proportion;           /* stage 6: 0 (see below) */
    double stage1_ms, stage23_ms, stage4_ms, stage5_ms, stage6_ms;   /* wall time of the call's parts (host clock; each but the last ends in a stream synchronisation) */
} canvas_somatic_call_scalars;
/* CanvasSomaticCaller.CallVariants on device-resident bins and sites, with canvas_somatic_model_fit in the middle.  Bins, segments, sites, their ordering rules and the
 * CANVAS_ERR_INVALID cases are those of canvas_call_diploid.  h_seg_ref_cn (nseg, or NULL = 2 everywhere) is ReferencePloidy.GetReferenceCopyNumber per segment.  Excluded
 * intervals (_excludedIntervals) of chromosome c are h_chr_excl_offset[c] .. [c+1] of h_excl_start / h_excl_stop, sorted by start (h_chr_excl_offset NULL: none).
 *   1  sites to segments, MeanCoverage, per-segment median count, number of folded frequencies and their upper median (device, the select classes of canvas_segment_select)
 *   2  GetUsableSegmentsAndSourcesForModeling (:1432-1493) inside the threshold loop of :1626-1634; overallMedianCoverage is one more select (over every bin, or over the
 *      per-segment medians as floats for enrichment); the usable segments' coverage / maf / weight / length are gathered on the device for the fit
 *   3  medianCoverageLevel = Convert.ToInt32(Quartiles(bins of the usable segments at reference copy number 2).Item2): a device compaction in front of the select;
 *      CoverageWeightingFactor with its evenness branch, the grid's coverages, DeviationFactor
 *   4  canvas_somatic_model_fit on the device arrays of stage 2; *h_fit is its result
 *   5  AssignPloidyCalls (:2379-2457) over all segments against the unrefined ploidy table of the best model (host table, device scan), MeanCount for the segments at
 *      MaximumCopyNumber (bit-equal to the serial double sum in bin order rounded to float: seg_mean_route says how), the rule of :2438-2454
 *   6  host: Logistic q-scores, MergeSegmentsUsingExcludedIntervals or (enrichment) MergeSegments(minimum_call_size, merge_span) with MergeIn as it is, q-scores of the runs
 *      with the bins MergeIn kept, SetFilterForSegments, EstimateChromosomeCount over the original list (int32 arithmetic), SelectPurityEstimate
 * NOT built: the clustering (Program.cs fixes MeanShift, whose KD tree is not in the reference tree), the segment windows, IsSampleClearlyNotAllReferencePloidy and the cluster
 * term: minimum_purity_hard_limit and min_minor_allele_coverage stay caller-supplied as for the fit.  MeanShift never writes ClusterId, so _heterogeneousSegmentsSignature is
 * empty in the reference as shipped: IsHeterogeneous is false everywhere, AdjustPloidyCalls changes nothing and HeterogeneityProportion is 0; none of it is computed.  Nor
 * AssignPloidyCallsGaussianMixture, PruneFrequencies, the truth-set reports, the executable with its VCF and coverage plot file, medians of the merged runs.
 * Errors: CANVAS_ERR_SOMATIC_FEW_SEGMENTS (stages 1-2 filled); CANVAS_ERR_SOMATIC_NO_MODEL / _NO_SCORE from the fit (stages 1-3 and *h_fit filled); CANVAS_ERR_INVALID for a
 * median level below 1 or outside int32, no usable segment at reference copy number 2, CoverageWeighting <= CoverageWeightingWithMafSegmentation on the evenness branch, no
 * kept site, and what the fit refuses.  The host tables and parameters are checked before the context is looked at; *h_scalars is cleared once they have passed. */
int32_t canvas_call_somatic(canvas_ctx* ctx, int64_t nbins, const float* d_count, int32_t nchr, const int64_t* h_chr_seg_offset /* nchr+1 */, const int32_t* h_seg_begin,
                            const int32_t* h_seg_end, const int64_t* h_seg_bin_offset /* nseg+1 */, const int64_t* h_chr_site_offset /* nchr+1 */, const int32_t* d_site_pos,
                            const int32_t* d_site_ref, const int32_t* d_site_alt, const int32_t* h_seg_ref_cn, const int64_t* h_chr_excl_offset /* nchr+1 */,
                            const int32_t* h_excl_start, const int32_t* h_excl_stop, const canvas_somatic_call_params* params, const canvas_somatic_call_out* out,
                            canvas_somatic_call_scalars* h_scalars, canvas_somatic_result* h_fit);

/* PloidyInfo.GetReferenceCopyNumber (PloidyInfo.cs:56-72,92-110) per segment: plain host code, no context, no GPU.  Segments grouped by chromosome (h_chr_seg_offset[nchr+1],
 * zero-based h_seg_begin / h_seg_end), the ploidy records in the layout of canvas_segment_ids_ploidy (h_ploidy_offset NULL: no records).  The counts run over the one-based
 * interval [Begin + 1, End]; the first copy number with the strictly largest count wins; 2 when every count is 0 or the chromosome has no records.  CANVAS_ERR_INVALID for
 * offsets that do not start at 0 or decrease, a missing array and a copy number outside 0..4. */
int32_t canvas_reference_copy_numbers(int32_t nchr, const int64_t* h_chr_seg_offset /* nchr+1 */, const int32_t* h_seg_begin, const int32_t* h_seg_end,
                                      const int64_t* h_ploidy_offset /* nchr+1 */, const int32_t* h_ploidy_start, const int32_t* h_ploidy_end, const int32_t* h_ploidy_cn,
                                      int32_t* h_seg_ref_cn);
/* canvas_segment_tables, canvas_reference_copy_numbers on its tables, then canvas_call_somatic on the tables and the float counts: the counterpart of canvas_call_diploid_ids.
 * The bins' arrays, cap_seg and the table outputs of the first (d_cov and d_count_f32 are required), the ploidy records of the second (h_ploidy_offset NULL: 2 everywhere)
 * with h_seg_ref_cn (cap_seg entries) as an output, the sites, excluded intervals, parameters and outputs of the third (arrays of cap_seg entries, seg_site_offset
 * cap_seg + 1).  The refusals of the three, in that order; more than cap_seg segments are refused with *h_nseg set, as by canvas_call_diploid_ids. */
int32_t canvas_call_somatic_ids(canvas_ctx* ctx, int64_t nbins, int32_t nchr, const int64_t* h_chr_offset /* nchr+1 */, const int32_t* d_start, const int32_t* d_stop,
                                const int32_t* d_segment_id, const double* d_cov, int64_t cap_seg, const int64_t* h_chr_site_offset /* nchr+1 */, const int32_t* d_site_pos,
                                const int32_t* d_site_ref, const int32_t* d_site_alt, const int64_t* h_ploidy_offset /* nchr+1 */, const int32_t* h_ploidy_start,
                                const int32_t* h_ploidy_end, const int32_t* h_ploidy_cn, const int64_t* h_chr_excl_offset /* nchr+1 */, const int32_t* h_excl_start,
                                const int32_t* h_excl_stop, const canvas_somatic_call_params* params,
                                int64_t* h_nseg, int64_t* h_chr_seg_offset /* nchr+1 */, int32_t* h_seg_begin, int32_t* h_seg_end, int64_t* h_seg_bin_offset /* cap_seg+1 */,
                                int32_t* h_seg_ci4 /* 4*cap_seg */, float* d_count_f32, int32_t* h_seg_ref_cn /* cap_seg */, const canvas_somatic_call_out* out,
                                canvas_somatic_call_scalars* h_scalars, canvas_somatic_result* h_fit);

/* ---- BGZF: the blocks of a BAM inflated on the device (what the three readers above take as d_records) ------------------------------------------------- */
/* A BGZF block is an independent raw-deflate stream of at most 64 KiB in and out.  Block i of d_blocks is the stream d_src[src_offset, src_offset + src_bytes) and has to
 * give exactly out_bytes bytes at d_dst[dst_offset, ...): one wave per block, profile scope "bgzf_inflate".
 *   d_status[i] 0, or why the block failed (CANVAS_INFLATE_*).  0 if and only if zlib's raw inflate (inflateInit2(-15), Z_FINISH) reaches Z_STREAM_END with exactly
 *               out_bytes written, and the bytes are then zlib's.  Unused input behind the final deflate block is accepted; the CRC32 of the BGZF trailer is NOT checked (canvas_bgzf_crc32 below does that).
 *   ranges      src_bytes and out_bytes are at most 65536; a larger one, or a range outside src_nbytes / dst_nbytes, is CANVAS_INFLATE_DESCRIPTOR for that block and
 *               nothing of it is read or written.  A block reads no byte outside its source range and writes none outside [dst_offset, dst_offset + out_bytes); the
 *               destination bytes of a FAILED block are unspecified (this build leaves them alone).  Destination ranges of different blocks must not overlap.
 *   h_info      NULL: the call only queues work on the context's stream.  Otherwise int64[4], and the call waits: [0] blocks, [1] failed blocks, [2] bytes written by
 *               good blocks, [3] index of the first failed block (-1: none).
 * CANVAS_ERR_INVALID: NULL context, negative nblocks, a NULL buffer with nblocks > 0.  nblocks == 0 launches nothing. */
typedef struct { uint64_t src_offset; uint64_t dst_offset; uint32_t src_bytes; uint32_t out_bytes; } canvas_bgzf_block;   /* 24 bytes */
#define CANVAS_INFLATE_OK 0
#define CANVAS_INFLATE_DESCRIPTOR 1   /* a size above 65536 or a range outside its buffer */
#define CANVAS_INFLATE_HEADER 2       /* BTYPE 3, stored LEN != ~NLEN, more than 286 literal/length or 30 distance codes */
#define CANVAS_INFLATE_INPUT 3        /* the stream needs bits behind src_bytes */
#define CANVAS_INFLATE_OVERRUN 4      /* the stream gives more than out_bytes */
#define CANVAS_INFLATE_SHORT 5        /* the stream ends before out_bytes */
#define CANVAS_INFLATE_DISTANCE 6     /* a match reaches before the block's first output byte */
#define CANVAS_INFLATE_CODE 7         /* an invalid symbol or code set */
int32_t canvas_bgzf_inflate(canvas_ctx* ctx, const uint8_t* d_src, uint64_t src_nbytes, const canvas_bgzf_block* d_blocks, int64_t nblocks,
                            uint8_t* d_dst, uint64_t dst_nbytes, int32_t* d_status, int64_t* h_info);
/* The descriptors of consecutive BGZF blocks of h_bytes[0, nbytes) from byte `at` on (host memory; no context, no device call): the gzip magic bytes, FEXTRA, a `BC`
 * subfield with SLEN 2, BSIZE, ISIZE <= 65536.  src_offset is the deflate data's offset in h_bytes, dst_offset the running sum of out_bytes from 0.  The walk stops, in
 * this order of precedence, at `capacity` blocks or once the inflated sizes have reached max_out_bytes (CANVAS_BGZF_SCAN_LIMIT), at nbytes (_END), or at bytes that
 * are no whole block (_DAMAGED).  h_info int64[4]: [0] blocks, [1] the file offset the walk stopped at, [2] their inflated bytes, [3] the reason.
 * CANVAS_ERR_INVALID: NULL h_info, NULL h_bytes with nbytes > 0, negative capacity, NULL h_blocks with capacity > 0, at > nbytes. */
#define CANVAS_BGZF_SCAN_LIMIT 0
#define CANVAS_BGZF_SCAN_END 1
#define CANVAS_BGZF_SCAN_DAMAGED 2
int32_t canvas_bgzf_scan(const uint8_t* h_bytes, uint64_t nbytes, uint64_t at, uint64_t max_out_bytes, canvas_bgzf_block* h_blocks, int64_t capacity, int64_t* h_info);
/* The CRC32 (RFC 1952, zlib's crc32) of every inflated block, summed on the device and held against the block's trailer: the descriptors of canvas_bgzf_inflate,
 * unchanged, and the d_dst that call filled.  One workgroup per block, profile scope "bgzf_crc32".
 *   d_crc[i]          the CRC32 of d_dst[dst_offset, dst_offset + out_bytes); 0 for out_bytes == 0 and for a block that is not summed (DESCRIPTOR, SKIPPED).
 *   d_status[i]       CANVAS_CRC_*.  The expected value is the little-endian word at d_src[src_offset + src_bytes, + 4): the BGZF trailer follows the deflate data.
 *   d_src             NULL: compute only, nothing is compared and every block with a valid data range is CANVAS_CRC_OK.
 *   d_inflate_status  NULL: every block is checked.  Otherwise the statuses canvas_bgzf_inflate left: a block whose status is not 0 is CANVAS_CRC_SKIPPED.
 *   h_info            NULL: the call only queues work on the context's stream.  Otherwise int64[4], and the call waits: [0] blocks, [1] blocks whose status is neither
 *                     OK nor SKIPPED, [2] bytes summed (OK and MISMATCH blocks), [3] index of the first block counted in [1] (-1: none).
 * No byte outside a block's data range and its trailer word is read.
 * CANVAS_ERR_INVALID: NULL context, negative nblocks, NULL d_blocks / d_dst / d_crc / d_status with nblocks > 0.  nblocks == 0 launches nothing. */
#define CANVAS_CRC_OK 0
#define CANVAS_CRC_MISMATCH 1      /* computed != the trailer's */
#define CANVAS_CRC_DESCRIPTOR 2    /* out_bytes > 65536, a data range outside dst_nbytes, or (d_src given) a trailer outside src_nbytes */
#define CANVAS_CRC_SKIPPED 3       /* d_inflate_status given and nonzero for this block: nothing read */
int32_t canvas_bgzf_crc32(canvas_ctx* ctx, const uint8_t* d_src, uint64_t src_nbytes, const canvas_bgzf_block* d_blocks, int64_t nblocks,
                          const uint8_t* d_dst, uint64_t dst_nbytes, const int32_t* d_inflate_status,
                          uint32_t* d_crc, int32_t* d_status, int64_t* h_info);

/* ---- BAM record framing on the device: d_record_offsets of the three readers above from the bytes canvas_bgzf_inflate leaves ------------------------------ */
/* d_records[0, nbytes) holds raw record bytes; the block_size chain starts at `first`: next(o) = o + 4 + block_size(o).  The call writes the offsets of the records
 * the rule TAKES, in chain order (each points at the block_size word), and answers in h_info where the chain ended and why.  It always waits (the caller needs the
 * count before it can call a reader); profile scope "bam_frame".
 *   chain       fewer than 4 bytes left, or a block_size >= 32 that reaches beyond nbytes: the chunk ends here; no event, the bytes from here on are the carry of
 *               the next chunk.  A block_size < 32 (negative values included) is MALFORMED.
 *   rule.kind   per whole record, the checks in this order (they restate the executables' own, canvas_amd/csrc/bam_frame.hpp):
 *               CANVAS_BAM_FRAME_ALL        every whole record is taken.
 *               CANVAS_BAM_FRAME_SNV        name, CIGAR, bases and qualities do not fit block_size: MALFORMED; refID < 0, pos < 0 or refID > ref_id: STOP (not taken);
 *                                           refID != ref_id: skipped; pos below the last taken pos: UNSORTED; otherwise taken.
 *               CANVAS_BAM_FRAME_HITS       name and CIGAR do not fit: MALFORMED; refID == ref_id and sorted == 0: taken; failing the read filters of
 *                                           canvas_hits_from_bam (paired_end as there): taken; refID != ref_id: taken, and STOP behind it; pos below the last pos that
 *                                           got this far: UNSORTED; otherwise taken.  sorted = 1 exactly for mode 5 (GCContentWeighted).
 *               CANVAS_BAM_FRAME_FRAGMENTS  name and CIGAR do not fit: MALFORMED; refID != ref_id: taken, and STOP behind it; otherwise taken.
 *   event       the first record in chain order that stops, is malformed or unsorted; nothing behind it is classified, taken or counted.
 *   h_info      int64[8], required: [0] records classified, the event's included; [1] records taken = offsets written; [2] `used`: the offset of a STOP / MALFORMED /
 *               UNSORTED record, the offset behind a taken stopping record, otherwise the offset of the first incomplete record or of the trailing 0-3 bytes;
 *               [3] the event (CANVAS_BAM_FRAME_NONE ...); [4] the offset of the event's record, -1 without one; [5] the pos an UNSORTED record was compared with;
 *               [6] tiles whose guessed entry was wrong and that were walked again (diagnostic: costs time, changes nothing); [7] the tile size in bytes.
 *   d_state     int64[4] in device memory, zeroed before the first chunk, carried from call to call: [0] records that reached the sortedness comparison and passed it,
 *               [1] the pos of the last of them, [2] records taken in all, [3] the last call's event.
 *   capacity    more taken records than `capacity`: event CANVAS_BAM_FRAME_CAPACITY, h_info[1] = the number needed, the other words as the repeated call will
 *               give them, no offset written, d_state unchanged.  The call returns CANVAS_OK and can be repeated.
 *   exactness   the result is the sequential chain's and nothing else.  Record starts are guessed per tile so that the tiles can be walked side by side; a guess is
 *               used only where the chain from the tiles before arrives at exactly that offset.  A record the chain reaches is classified even if it looks like
 *               garbage; bytes that look like a record and are not on the chain are ignored.  No byte outside [d_records, d_records + nbytes) is read.
 * nbytes - first < 4 launches nothing, leaves d_state alone and answers NONE with used = first.
 * CANVAS_ERR_INVALID: NULL context, rule, state or info; first > nbytes; an unknown kind; NULL d_record_offsets with capacity > 0; a negative capacity; NULL d_records
 * with nbytes > 0; nbytes - first of 2^32 and more (a chunk is cut by the caller). */
typedef struct { int32_t kind; int32_t ref_id; int32_t paired_end; int32_t sorted; } canvas_bam_frame_rule;   /* 16 bytes */
#define CANVAS_BAM_FRAME_ALL 0
#define CANVAS_BAM_FRAME_SNV 1
#define CANVAS_BAM_FRAME_HITS 2
#define CANVAS_BAM_FRAME_FRAGMENTS 3
#define CANVAS_BAM_FRAME_NONE 0
#define CANVAS_BAM_FRAME_STOPPED 1
#define CANVAS_BAM_FRAME_MALFORMED 2
#define CANVAS_BAM_FRAME_UNSORTED 3
#define CANVAS_BAM_FRAME_CAPACITY 4
int32_t canvas_bam_frame(canvas_ctx* ctx, const uint8_t* d_records, uint64_t nbytes, uint64_t first, const canvas_bam_frame_rule* rule, uint64_t* d_record_offsets,
                         int64_t capacity, int64_t* d_state, int64_t* h_info);

/* ---- profiling hooks (hipEvent pairs recorded on the context's stream around the named kernels) --------------------- */
/* on: 0 off; 1 every named scope; 2 only the scopes around the dominant (HBM-bound) kernel of CanvasBin — "bin_summary", "bin_summary_packed", "bin_pass",
   "bin_tile_stats" — so that a timed pass carries two event records instead of a dozen (each scope costs two barrier packets on the stream) */
int32_t canvas_profile_enable(canvas_ctx* ctx, int32_t on);
/* name: "bin_pass", "bin_tile_stats", "viterbi"; returns accumulated ms and launch count since the last reset */
int32_t canvas_profile_get(canvas_ctx* ctx, const char* name, double* h_ms_total, int32_t* h_launches, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif
