// P/Invoke binding of libcanvas_hip.so (include/canvas_hip.h) for the three Canvas modules.  Host code stays C# (netcore): the modules keep their
// Main, option parsing and file readers / writers and call the entry points below instead of their compute loops.
// NOT COMPILED IN THIS REPOSITORY'S IMAGE (no dotnet SDK; Illumina.Common / Isas.* are private NuGet packages).  The same ABI is exercised by
// canvas_amd/lib.py (ctypes) and by the C++ drop-in tools under canvas_amd/tools/, which are what the test-suite runs.
using System;
using System.Runtime.InteropServices;

namespace CanvasHipInterop
{
    internal static class CanvasHip
    {
        const string Lib = "canvas_hip";   // libcanvas_hip.so next to the module's dll, or on LD_LIBRARY_PATH

        public const int ModeBinary = 0, ModeTruncatedDynamicRange = 3, ModeGCContentWeighted = 5;                 // Utilities.cs:56-74
        public const uint CleanGcNorm = 1, CleanFiltSize = 2, CleanOutliers = 4, CleanLocalSd = 8, CleanLoess = 16;  // CanvasClean.cs:431-446

        // ---- context, memory
        [DllImport(Lib)] public static extern IntPtr canvas_create(int device);
        [DllImport(Lib)] public static extern void canvas_destroy(IntPtr ctx);
        [DllImport(Lib)] public static extern IntPtr canvas_last_error(IntPtr ctx);
        [DllImport(Lib)] public static extern IntPtr canvas_version();
        [DllImport(Lib)] public static extern int canvas_synchronize(IntPtr ctx);
        [DllImport(Lib)] public static extern IntPtr canvas_device_malloc(IntPtr ctx, long bytes);
        [DllImport(Lib)] public static extern int canvas_device_free(IntPtr ctx, IntPtr dptr);
        [DllImport(Lib)] public static extern int canvas_memcpy_h2d(IntPtr ctx, IntPtr dDst, byte[] hSrc, long bytes);
        [DllImport(Lib)] public static extern int canvas_memcpy_h2d(IntPtr ctx, IntPtr dDst, short[] hSrc, long bytes);
        [DllImport(Lib)] public static extern int canvas_memcpy_h2d(IntPtr ctx, IntPtr dDst, ulong[] hSrc, long bytes);
        [DllImport(Lib)] public static extern int canvas_memcpy_h2d(IntPtr ctx, IntPtr dDst, int[] hSrc, long bytes);
        [DllImport(Lib)] public static extern int canvas_memcpy_h2d(IntPtr ctx, IntPtr dDst, float[] hSrc, long bytes);
        [DllImport(Lib)] public static extern int canvas_memcpy_h2d(IntPtr ctx, IntPtr dDst, double[] hSrc, long bytes);
        [DllImport(Lib)] public static extern int canvas_memcpy_d2h(IntPtr ctx, int[] hDst, IntPtr dSrc, long bytes);
        [DllImport(Lib)] public static extern int canvas_memcpy_d2h(IntPtr ctx, float[] hDst, IntPtr dSrc, long bytes);

        // ---- CanvasBin
        [DllImport(Lib)] public static extern int canvas_mask_from_fasta(IntPtr ctx, IntPtr dBases, long len, IntPtr dMask);
        [DllImport(Lib)] public static extern int canvas_mask_exclude_intervals(IntPtr ctx, IntPtr dMask, long len, int n, int[] start, int[] stop);
        [DllImport(Lib)] public static extern int canvas_screen_hits(IntPtr ctx, IntPtr dHits, IntPtr dMask, long len);
        [DllImport(Lib)] public static extern int canvas_bin_rates(IntPtr ctx, int nchr, IntPtr[] dHits, IntPtr[] dMask, long[] len, long[] observed, long[] possible, double[] rate);
        [DllImport(Lib)] public static extern int canvas_bin_size_from_rates(double[] rates, int n, int countsPerBin);
        [DllImport(Lib)] public static extern long canvas_bin_count_upper_bound(int nchr, long[] len, int binSize);
        [DllImport(Lib)] public static extern int canvas_bin_sample(IntPtr ctx, int nchr, IntPtr[] dBases, IntPtr[] dMask, IntPtr[] dHits, long[] len, byte[] chrIsAutosome,
            int countsPerBin, int binSizeIn, int mode, IntPtr dChr, IntPtr dStart, IntPtr dStop, IntPtr dGc, IntPtr dCount, long cap, out int binSize, long[] nbinsPerChr, out long nbinsTotal);
        [DllImport(Lib)] public static extern int canvas_bin_sample_gcweighted(IntPtr ctx, int nchr, IntPtr[] dBases, IntPtr[] dMask, IntPtr[] dHits, IntPtr[] dFragLen, long[] len,
            byte[] chrIsAutosome, int countsPerBin, int binSizeIn, IntPtr dChr, IntPtr dStart, IntPtr dStop, IntPtr dGc, IntPtr dCount, long cap, out int binSize, long[] nbinsPerChr, out long nbinsTotal);
        // CanvasBin -n (BinCountsForChromosome with usePredefinedBins, CanvasBin.cs:575-655); the _gcweighted form is -n with -m GCContentWeighted (:617-636)
        [DllImport(Lib)] public static extern int canvas_bin_predefined(IntPtr ctx, int nchr, IntPtr[] dBases, IntPtr[] dMask, IntPtr[] dHits, long[] len, int mode, long[] binOffset,
            int[] binStart, int[] binStop, IntPtr dBinStart, IntPtr dBinStop, IntPtr dGc, IntPtr dCount);
        [DllImport(Lib)] public static extern int canvas_bin_predefined_gcweighted(IntPtr ctx, int nchr, IntPtr[] dBases, IntPtr[] dMask, IntPtr[] dHits, IntPtr[] dFragLen, long[] len, long[] binOffset,
            int[] binStart, int[] binStop, IntPtr dBinStart, IntPtr dBinStop, IntPtr dGc, IntPtr dCount);

        // ---- packed per-base inputs (INTEGRATION.md 5b): 0.75 B/base over PCIe instead of 2.125 B/base, same bins
        [DllImport(Lib)] public static extern int canvas_packed_plane_bytes(long len, out long refBytes, out long hitBytes);
        [DllImport(Lib)] public static extern int canvas_pack_reference_host(byte[] bases, ulong[] mask, long len, IntPtr refOut, out long pos0, int threads);
        [DllImport(Lib)] public static extern int canvas_pack_hits_host(byte[] hits, long len, IntPtr planesOut, out long saturated, int threads);
        [DllImport(Lib)] public static extern int canvas_upload_packed_begin(IntPtr ctx, int nchr, long[] len, IntPtr[] hRef, IntPtr[] dRef, IntPtr[] hPlanes, IntPtr[] dPlanes);
        [DllImport(Lib)] public static extern int canvas_pack_hits2_host(byte[] hits, long len, IntPtr loOut, IntPtr hdrOut, IntPtr extrasOut, long extrasCapWords, out long nExtras, out long saturated, int threads);
        [DllImport(Lib)] public static extern int canvas_upload_packed2_begin(IntPtr ctx, int nchr, long[] len, IntPtr[] hRef, IntPtr[] dRef, IntPtr[] hLo, IntPtr[] hHdr, IntPtr[] hExtras, long[] nExtras, IntPtr[] dPlanes);
        [DllImport(Lib)] public static extern int canvas_bin_sample_packed(IntPtr ctx, int nchr, IntPtr[] dRef, IntPtr[] dPlanes, long[] len, long[] pos0, byte[] chrIsAutosome,
            int countsPerBin, int binSizeIn, int mode, IntPtr dChr, IntPtr dStart, IntPtr dStop, IntPtr dGc, IntPtr dCount, long cap, out int binSize, long[] nbinsPerChr, out long nbinsTotal);

        // ---- CanvasClean
        [DllImport(Lib)] public static extern int canvas_clean2(IntPtr ctx, long n, IntPtr dChr, IntPtr dStart, IntPtr dStop, IntPtr dCount, IntPtr dGc, int nchr,
            byte[] chrIsAutosome, byte[] chrIsY, uint flags, int minBinsPerGc, out double localSd, out long nOut, int[] info8);

        // a cohort through CanvasClean in one call (one launch chain for all samples; pedigree runs clean every member, CanvasRunner.cs:1010-1070)
        [DllImport(Lib)] public static extern int canvas_clean_batch(IntPtr ctx, int nsamples, long[] n, IntPtr[] dChr, IntPtr[] dStart, IntPtr[] dStop, IntPtr[] dCount, IntPtr[] dGc, int nchr,
            byte[] chrIsAutosome, byte[] chrIsY, uint flags, int minBinsPerGc, double[] localSd, long[] nOut, int[] info8PerSample);

        // ---- CanvasPartition
        [DllImport(Lib)] public static extern int canvas_evenness_score(IntPtr ctx, int nchr, IntPtr dCov, long[] chrOffset, int windowSize, out double score, out int valid);
        [DllImport(Lib)] public static extern int canvas_wavelets(IntPtr ctx, int nchr, IntPtr dCov, long[] chrOffset, int isGermline, double thresholdLower, double thresholdUpper,
            double madFactor, int variabilityWindow, int minSize, int[] breakpoints, long cap, long[] bpOffset);
        [DllImport(Lib)] public static extern int canvas_cbs_undo(IntPtr ctx, int nchr, IntPtr dCov, long[] chrOffset, double alpha, uint nperm, int undo, double undoSd,
            IntPtr dSegLen, int[] nseg, long[] stats8);
        // the draw streams of CBS are constants of the method (CBSRunner.cs:107-112): started while CanvasSegment.ReadBedInput is still parsing (CanvasPartitionHipMain.Main)
        [DllImport(Lib)] public static extern int canvas_cbs_prefetch(IntPtr ctx, int nchr, long wordsPerChromosome);
        [DllImport(Lib)] public static extern int canvas_cbs_cache_stats(IntPtr ctx, long[] out6);
        [DllImport(Lib)] public static extern int canvas_cbs_seeds(int nchr, int[] seeds, out int mathNetByteVariant);    // to settle include/canvas_mathnet.h: compare seeds[0] with new MersenneTwister(0).NextFullRangeInt32()
        [DllImport(Lib)] public static extern int canvas_hmm_per_sample(IntPtr ctx, int nchr, IntPtr dCov, long[] chrOffset, IntPtr dState);
        [DllImport(Lib)] public static extern int canvas_hmm_joint(IntPtr ctx, int nsamples, int nchr, IntPtr[] dCovPerSample, long[] chrOffset, IntPtr dState);
        [DllImport(Lib)] public static extern int canvas_segment_ids_ploidy(IntPtr ctx, int nchr, long[] chrOffset, IntPtr dState, IntPtr dStart, IntPtr dStop, int maxInterBinDist,
            long[] exclOffset, int[] exclStart, int[] exclStop, long[] ploidyOffset, int[] ploidyStart, int[] ploidyEnd, int[] ploidyCn, IntPtr dSegmentId, out long nSegments);
        [DllImport(Lib)] public static extern int canvas_split_overlapping(int nsamples, IntPtr[] hStart, IntPtr[] hEnd, int[] nseg, uint[] outStart, uint[] outEnd, int cap, out int nOut);

        // ---- multi-GPU (one process per GPU, chromosome groups per rank; see hosts/README.md)
        [DllImport(Lib)] public static extern int canvas_comm_unique_id(byte[] id128);
        [DllImport(Lib)] public static extern int canvas_comm_init(IntPtr ctx, int rank, int nranks, byte[] id128);
        [DllImport(Lib)] public static extern int canvas_allgather_boundaries(IntPtr ctx, IntPtr dLocal, int nLocal, int maxPerRank, IntPtr dAll, int[] counts);
        // samples x chromosome groups: ranks with the same color form a sub-communicator (ncclCommSplit); restore goes back to the communicator of canvas_comm_init
        [DllImport(Lib)] public static extern int canvas_comm_split(IntPtr ctx, int color, int key);
        [DllImport(Lib)] public static extern int canvas_comm_restore(IntPtr ctx);
        [DllImport(Lib)] public static extern int canvas_comm_rank(IntPtr ctx, out int rank, out int nranks);
        // CanvasBin alone, chromosomes sharded over the ranks (modes 0, 3, 5; dFraglen: mode 5 only): every rank receives the whole genome's bins
        [DllImport(Lib)] public static extern int canvas_bin_sample_sharded(IntPtr ctx, int nchr, int[] chrOwner, IntPtr[] dBases, IntPtr[] dMask, IntPtr[] dHits, IntPtr[] dFraglen, long[] len, byte[] chrIsAutosome,
                                                                            int countsPerBin, int binSizeIn, int mode, IntPtr dChr, IntPtr dStart, IntPtr dStop, IntPtr dGc, IntPtr dCount, long cap, out int binSize, out long nBins);
        // PerSampleHMM with the chromosomes sharded over the ranks, on a coverage every rank holds (behind the bin intersection of a pedigree)
        [DllImport(Lib)] public static extern int canvas_hmm_per_sample_sharded(IntPtr ctx, int nchr, int[] chrOwner, IntPtr dCov, long[] chrOffset, IntPtr dState);
        // diagnostics of the last call: mode 5 bins decided by the interval / replayed; edge tests on the device kernel / swaps of all edge tests
        [DllImport(Lib)] public static extern int canvas_bin_gcw_stats(IntPtr ctx, long[] out2);
        [DllImport(Lib)] public static extern int canvas_cbs_tpermp_stats(IntPtr ctx, long[] out2);
        // ONE sample, chromosomes sharded over the ranks (chrOwner[c] = rank that holds chromosome c); every rank receives the whole result
        [DllImport(Lib)] public static extern int canvas_sample_pipeline_sharded(IntPtr ctx, int nchr, int[] chrOwner, IntPtr[] dBases, IntPtr[] dMask, IntPtr[] dHits, long[] len, byte[] chrIsAutosome, byte[] chrIsY,
            int countsPerBin, int binSizeIn, int mode, uint cleanFlags, int minBinsPerGc, int maxInterBinDist, IntPtr dChr, IntPtr dStart, IntPtr dStop, IntPtr dGc, IntPtr dCount, long cap,
            IntPtr dCov, IntPtr dState, IntPtr dSegmentId, out int binSize, out long nBins, out long nBinsClean, out double localSd, long[] chrOffset, out long nSegments);
        [DllImport(Lib)] public static extern int canvas_sample_pipeline_sharded_packed(IntPtr ctx, int nchr, int[] chrOwner, IntPtr[] dRef, IntPtr[] dHitPlanes, long[] len, long[] pos0, byte[] chrIsAutosome, byte[] chrIsY,
            int countsPerBin, int binSizeIn, int mode, uint cleanFlags, int minBinsPerGc, int maxInterBinDist, IntPtr dChr, IntPtr dStart, IntPtr dStop, IntPtr dGc, IntPtr dCount, long cap,
            IntPtr dCov, IntPtr dState, IntPtr dSegmentId, out int binSize, out long nBins, out long nBinsClean, out double localSd, long[] chrOffset, out long nSegments);
        // CanvasPartition -m CBS / -m Wavelets on the coverage that call leaves on every rank (CBSRunner.cs:62-112, WaveletsRunner.cs:89-135: per-chromosome tasks on the owner)
        [DllImport(Lib)] public static extern int canvas_cbs_sharded(IntPtr ctx, int nchr, int[] chrOwner, IntPtr dCov, long[] chrOffset, double alpha, uint nperm, int undo, double undoSd,
            IntPtr dSegLen, int[] nseg, long[] stats8);
        [DllImport(Lib)] public static extern int canvas_wavelets_sharded(IntPtr ctx, int nchr, int[] chrOwner, IntPtr dCov, long[] chrOffset, int isGermline, double thresholdLower, double thresholdUpper,
            double madFactor, int variabilityWindow, int minSize, int[] breakpoints, long cap, long[] bpOffset);
        // a pedigree, one sample per rank: the rates of every sample (multi-sample bin size, CanvasBin.cs:86-110) and the bin intersection (Utilities.cs:834-920)
        [DllImport(Lib)] public static extern int canvas_allgather_host(IntPtr ctx, double[] send, long bytesPerRank, double[] recv);
        [DllImport(Lib)] public static extern int canvas_merge_cleaned_sharded(IntPtr ctx, long nMine, IntPtr dChr, IntPtr dStart, IntPtr dStop, IntPtr dCount,
            IntPtr dOutChr, IntPtr dOutStart, IntPtr dOutStop, IntPtr dOutCount, long cap, out long nOut);
        // CanvasNormalize: the three reference generators (WeightedAverage, BestLR2, PCA) and the LSNorm (mode 0) / Raw (mode 1) ratio + RatiosToCounts
        [DllImport(Lib)] public static extern int canvas_normalize_reference(IntPtr ctx, int nsamples, IntPtr[] dCountsPerSample, long n, IntPtr dOnTargetIdx, long nOnTarget,
            IntPtr dWeighted, double[] weights);
        [DllImport(Lib)] public static extern int canvas_normalize_best_normal(IntPtr ctx, IntPtr dTumor, int nnormals, IntPtr[] dNormals, long n, IntPtr dOnTargetIdx, long nOnTarget,
            out int best, double[] meanSquaredLogRatios, long[] ignoredBins, out int replayed);
        [DllImport(Lib)] public static extern int canvas_normalize_pca_reference(IntPtr ctx, long n, IntPtr dSample, IntPtr dMu, int naxes, IntPtr[] dAxes, double minRef, double maxRef,
            IntPtr dReference, out double medianRatio, double[] sizes, out int orthogonal);
        [DllImport(Lib)] public static extern int canvas_normalize_ratio(IntPtr ctx, long n, IntPtr dSample, IntPtr dReference, IntPtr dOnTargetIdx, long nOnTarget, int mode,
            double minRef, double maxRef, IntPtr dPloidy, IntPtr dKeepIdx, IntPtr dRatio, IntPtr dCount, out long nOut, out double librarySizeFactor);
        // CanvasSNV: allele counts at the variant sites from chunks of raw BAM record bytes (SNVReviewer.ProcessBamFile + ProcessReadBases); info = long[5] or null (queue only)
        [DllImport(Lib)] public static extern int canvas_snv_count(IntPtr ctx, IntPtr dRecords, ulong nbytes, IntPtr dRecordOffsets, long nrecords, int refId, int minMapQ, int minBaseQ,
            IntPtr dSitePos, IntPtr dSiteRef, IntPtr dSiteAlt, int nsites, IntPtr dRefCounts, IntPtr dAltCounts, long[] info);
        // CanvasBin: observed-alignment arrays (byte hits, short fragment lengths for mode 5 or IntPtr.Zero) from the same chunks; dState = 8 zeroed longs on the device, info = long[8] or null (queue only)
        [DllImport(Lib)] public static extern int canvas_hits_from_bam(IntPtr ctx, IntPtr dRecords, ulong nbytes, IntPtr dRecordOffsets, long nrecords, int refId, int pairedEnd, int mode,
            long len, IntPtr dHits, IntPtr dFrag, IntPtr dState, long[] info);
        // CanvasBin -m Fragment: fragment counts of one chromosome's BED bins from the same chunks; dCount (int per bin) and dState (16 longs) zeroed before the first chunk, dCarry = the
        // library's own list of open read names (CANVAS_ERR_CAPACITY: info[8] bytes are needed; enlarge it, keep its contents, call again); info = long[16], the call waits
        [DllImport(Lib)] public static extern int canvas_fragments_from_bam(IntPtr ctx, IntPtr dRecords, ulong nbytes, IntPtr dRecordOffsets, long nrecords, int refId, IntPtr dBinStart,
            IntPtr dBinStop, long nbins, int qualityThreshold, IntPtr dCount, IntPtr dCarry, ulong carryCapacity, IntPtr dState, long[] info);
        // BGZF: the blocks of a BAM inflated on the device, one BgzfBlock (24 bytes) per block; dStatus = int per block (0, or a CANVAS_INFLATE_* code: 1 descriptor, 2 header, 3 input, 4 overrun,
        // 5 short, 6 distance, 7 code); info = long[4] (blocks, failed, bytes of the good blocks, first failed or -1) or null (queue only).  The CRC32 is not checked here: canvas_bgzf_crc32
        [StructLayout(LayoutKind.Sequential)] public struct BgzfBlock { public ulong SrcOffset; public ulong DstOffset; public uint SrcBytes; public uint OutBytes; }
        [DllImport(Lib)] public static extern int canvas_bgzf_inflate(IntPtr ctx, IntPtr dSrc, ulong srcNbytes, IntPtr dBlocks, long nblocks, IntPtr dDst, ulong dstNbytes, IntPtr dStatus, long[] info);
        // the block table of a BGZF buffer in host memory from file offset `at` (no context): info = long[4] (blocks, next offset, inflated bytes, reason: 0 limit, 1 end, 2 damaged)
        [DllImport(Lib)] public static extern int canvas_bgzf_scan(byte[] hBytes, ulong nbytes, ulong at, ulong maxOutBytes, [Out] BgzfBlock[] hBlocks, long capacity, long[] info);
        // the CRC32 of every inflated block against the block's trailer word (the descriptors and dDst of canvas_bgzf_inflate; dSrc = IntPtr.Zero: compute only; dInflateStatus =
        // IntPtr.Zero: every block): dCrc = uint per block, dStatus = int per block (0 ok, 1 mismatch, 2 descriptor, 3 skipped); info = long[4] (blocks, neither ok nor skipped,
        // bytes summed, first such block or -1) or null (queue only)
        [DllImport(Lib)] public static extern int canvas_bgzf_crc32(IntPtr ctx, IntPtr dSrc, ulong srcNbytes, IntPtr dBlocks, long nblocks, IntPtr dDst, ulong dstNbytes, IntPtr dInflateStatus,
            IntPtr dCrc, IntPtr dStatus, long[] info);
        // BAM record framing on the device: the offsets of the records `rule` takes from the block_size chain of a chunk, from byte `first` on (Kind: 0 all, 1 SNV, 2 hits,
        // 3 fragments); dState = long[4] on the device, zeroed before the first chunk; info = long[8] (classified, taken, used, event: 0 none, 1 stopped, 2 malformed, 3 unsorted,
        // 4 capacity; the event's offset or -1; the pos an unsorted record was compared with; tiles walked twice; tile size).  The call waits
        [StructLayout(LayoutKind.Sequential)] public struct BamFrameRule { public int Kind; public int RefId; public int PairedEnd; public int Sorted; }
        [DllImport(Lib)] public static extern int canvas_bam_frame(IntPtr ctx, IntPtr dRecords, ulong nbytes, ulong first, ref BamFrameRule rule, IntPtr dRecordOffsets, long capacity,
            IntPtr dState, long[] info);
        [DllImport(Lib)] public static extern int canvas_memcpy_d2d_async(IntPtr ctx, IntPtr dDst, IntPtr dSrc, long bytes);
        [DllImport(Lib)] public static extern int canvas_memcpy_h2d_async(IntPtr ctx, IntPtr dDst, IntPtr hSrc, long bytes);
        // Tools/FlagUniqueKmers (KmerChecker): unique-35-mer masks of all contigs at once (stats = long[8] or null), and the letter case of kmer.fa from a mask
        [DllImport(Lib)] public static extern int canvas_flag_unique_kmers(IntPtr ctx, int nchr, IntPtr[] dBases, long[] len, IntPtr[] dMask, long maxTableBytes, long[] stats);
        [DllImport(Lib)] public static extern int canvas_fasta_case_from_mask(IntPtr ctx, IntPtr dBases, long len, IntPtr dMask);
        // CanvasSmooth: Utilities.MedianFilter with half window 1 .. maxHalfWindow over every chromosome (chrOffset = nchr + 1 bin offsets); outN[c] bins are left of chromosome c
        // and nothing beyond them is written to dOut.  canvas_smooth_lengths / canvas_smooth_plan are plain host code (no context): the lengths alone, and {fused, tile, halo, launches}
        [DllImport(Lib)] public static extern int canvas_smooth(IntPtr ctx, int nchr, long[] chrOffset, IntPtr dCount, int maxHalfWindow, IntPtr dOut, long[] outN);
        [DllImport(Lib)] public static extern int canvas_smooth_lengths(int nchr, long[] n, int maxHalfWindow, long[] outN);
        [DllImport(Lib)] public static extern int canvas_smooth_plan(int maxHalfWindow, long[] out4);
        // CanvasDiploidCaller's per-segment order statistics: dOut[s] (double) = median (mode 0: even-length average in float, 1: in double) or upper median a[n/2] (mode 2) of
        // dValues[segOffset[s] .. segOffset[s + 1]) (float), 0 for an empty segment (counted in nEmpty).  canvas_segment_select_plan is plain host code: {wave max, LDS max, tile, launches, forced class, 0}
        [DllImport(Lib)] public static extern int canvas_segment_select(IntPtr ctx, IntPtr dValues, long nseg, long[] segOffset, int mode, IntPtr dOut, out long nEmpty);
        [DllImport(Lib)] public static extern int canvas_segment_select_plan(long[] out6);
        // CanvasDiploidCaller.CallVariants between the parsed files and the written ones: sites to segments, MeanCoverage / diploidCoverage, the 36 model points, per-segment
        // medians and nearest model point, q-scores, MergeSegments, filters, run medians.  Per-segment arrays hold nseg entries (segSiteOffset nseg + 1), per-run arrays nseg
        // entries of which nRuns are filled; scalars2 = {diploidCoverage, MeanCoverage}; info4 = {kept sites, integer sum used, coverage sum, 0} or null
        [DllImport(Lib)] public static extern int canvas_call_diploid(IntPtr ctx, long nbins, IntPtr dCount, int nchr, long[] chrSegOffset, int[] segBegin, int[] segEnd, long[] segBinOffset,
            long[] chrSiteOffset, IntPtr dSitePos, IntPtr dSiteRef, IntPtr dSiteAlt, double[] logistic4,
            double[] segMedianCount, long[] segSiteOffset, int[] segInformative, double[] segMedianMaf, int[] segCn, int[] segMcc, double[] segDist, double[] segDist2, int[] segQScore,
            out long nRuns, long[] runFirst, long[] runLast, int[] runQScore, int[] runFilter, double[] runMedianCount, double[] scalars2, long[] info4);
        // Segments.ReadSegments on device-resident bins: the host tables canvas_call_diploid / canvas_call_somatic take, from the per-bin segment ids a partition entry left
        // (a segment starts at the first bin of a chromosome and wherever the id differs from the bin before).  Per-segment arrays hold capSeg entries (segBinOffset capSeg + 1,
        // segCi4 4 * capSeg: {start.lo, start.hi, end.lo, end.hi}); more than capSeg segments are refused with nSeg set.  dCov (double, or IntPtr.Zero) given: dCountF32[i] = (float)dCov[i]
        [DllImport(Lib)] public static extern int canvas_segment_tables(IntPtr ctx, long nbins, int nchr, long[] chrOffset, IntPtr dStart, IntPtr dStop, IntPtr dSegmentId, IntPtr dCov, long capSeg,
            out long nSeg, long[] chrSegOffset, int[] segBegin, int[] segEnd, long[] segBinOffset, int[] segCi4, IntPtr dCountF32);
        // canvas_segment_tables, then canvas_call_diploid on its tables and float counts (dCov and dCountF32 required; the call's arrays hold capSeg entries): four waits
        [DllImport(Lib)] public static extern int canvas_call_diploid_ids(IntPtr ctx, long nbins, int nchr, long[] chrOffset, IntPtr dStart, IntPtr dStop, IntPtr dSegmentId, IntPtr dCov, long capSeg,
            long[] chrSiteOffset, IntPtr dSitePos, IntPtr dSiteRef, IntPtr dSiteAlt, double[] logistic4,
            out long nSeg, long[] chrSegOffset, int[] segBegin, int[] segEnd, long[] segBinOffset, int[] segCi4, IntPtr dCountF32,
            double[] segMedianCount, long[] segSiteOffset, int[] segInformative, double[] segMedianMaf, int[] segCn, int[] segMcc, double[] segDist, double[] segDist2, int[] segQScore,
            out long nRuns, long[] runFirst, long[] runLast, int[] runQScore, int[] runFilter, double[] runMedianCount, double[] scalars2, long[] info4);

        // CanvasSomaticCaller.ModelOverallCoverageAndPurity's grid search (SomaticCaller.cs:1870-2117) over the usable segments (coverage / maf / weight double, length int:
        // device arrays when inputsOnDevice != 0, host arrays otherwise); the structs mirror include/canvas_hip.h field by field.  The cluster term of ModelDeviation is not
        // built: SomaticInfoClusterTerm in result.info says when the reference would have added it.  segPoint / segDistance (nseg, or IntPtr.Zero) and models (or IntPtr.Zero)
        public const int ErrSomaticNoModel = -6, ErrSomaticNoScore = -7, SomaticTile = 256, SomaticMaxCn = 10;
        public const uint SomaticInfoClusterTerm = 1, SomaticInfoIndexCutoff = 2;
        [StructLayout(LayoutKind.Sequential)] public struct canvas_somatic_params
        {
            public int maximum_copy_number, deviation_index_cutoff, maximum_related_models;
            public float min_allowed_ploidy, max_allowed_ploidy, deviation_factor;
            public double cn2_weighting_factor, deviation_score_weighting_factor, diploid_distance_score_weighting_factor, heterogeneity_score_weighting_factor;
        }
        [StructLayout(LayoutKind.Sequential)] public struct canvas_somatic_grid
        {
            public int min_coverage, max_coverage, minimum_purity_hard_limit, fixed_percent_purity, fixed_coverage, is_enrichment;
            public double min_minor_allele_coverage, coverage_weighting_factor;
            public long genome_length;
        }
        [StructLayout(LayoutKind.Sequential)] public unsafe struct canvas_somatic_result
        {
            public int best_model, best_coverage, best_percent_purity;
            public uint info;
            public int nmodels, nvalid, nscored, reserved;
            public double diploid_coverage, purity, deviation, precision_deviation, accuracy_deviation, ploidy, percent_normal, diploid_distance;
            public fixed double percent_cn[11];
            public double score, inter_model_distance, best_deviation, worst_allowed_deviation, host_table_ms, upload_ms, device_ms, selection_ms;
        }
        [StructLayout(LayoutKind.Sequential)] public struct canvas_somatic_models
        {
            public long capacity;
            public IntPtr coverage, percent_purity, deviation, precision_deviation, accuracy_deviation, ploidy, percent_normal, percent_cn, diploid_distance, flags, score;
        }
        [DllImport(Lib)] public static extern int canvas_somatic_model_fit(IntPtr ctx, long nseg, IntPtr coverage, IntPtr maf, IntPtr weight, IntPtr length, int inputsOnDevice,
            ref canvas_somatic_grid grid, ref canvas_somatic_params parameters, out canvas_somatic_result result, IntPtr segPoint, IntPtr segDistance, IntPtr models);

        // CanvasSomaticCaller.CallVariants between the parsed files and the written ones, with canvas_somatic_model_fit in the middle: usable segments, the median level and
        // the grid bounds, the fit, AssignPloidyCalls, Logistic q-scores, the merges, filters and header numbers.  Inputs as canvas_call_diploid plus segRefCn (or null: 2),
        // the excluded intervals per chromosome (chrExclOffset null: none) and the parameter struct; `output` holds host pointers to arrays of nseg entries (seg_site_offset
        // nseg + 1), of which scalars.nruns are filled in the per-run arrays.  The clustering is not built: minimum_purity_hard_limit and min_minor_allele_coverage are inputs
        public const int ErrSomaticFewSegments = -8, SomaticMeanNone = -1, SomaticMeanWalk = 0, SomaticMeanExact = 1;
        [StructLayout(LayoutKind.Sequential)] public struct canvas_somatic_call_params
        {
            public canvas_somatic_params fit;
            public int minimum_variant_frequencies, minimum_call_size, quality_filter_threshold, merge_span, is_enrichment, minimum_purity_hard_limit;
            public float lower_coverage_level_weighting_factor, upper_coverage_level_weighting_factor, user_purity, user_ploidy;
            public double coverage_weighting, coverage_weighting_with_maf_segmentation, evenness_score_threshold, min_evenness_score;
            public double logistic_intercept, logistic_log_bin_count, logistic_model_distance, logistic_distance_ratio;
            public double evenness_score, snv_purity_estimate, min_minor_allele_coverage;
            public long genome_length;
        }
        [StructLayout(LayoutKind.Sequential)] public struct canvas_somatic_call_out
        {
            public IntPtr seg_median_count, seg_site_offset, seg_maf_upper, seg_usable, seg_coverage, seg_maf, seg_weight, seg_cn, seg_cn2, seg_mcc, seg_dist, seg_dist2;
            public IntPtr seg_mean_count, seg_mean_route, seg_qscore, seg_run, run_owner, run_begin, run_end, run_bin_count, run_qscore, run_filter;
        }
        [StructLayout(LayoutKind.Sequential)] public struct canvas_somatic_call_scalars
        {
            public long nruns, nusable, kept_sites;
            public int stages, threshold_used, median_coverage_level, min_coverage, max_coverage, fixed_percent_purity;
            public float overall_median_coverage, deviation_factor;
            public double mean_coverage, coverage_weighting_factor, reported_purity, purity_model_fit, inter_model_distance, estimated_chromosome_count, heterogeneity_proportion;
            public double stage1_ms, stage23_ms, stage4_ms, stage5_ms, stage6_ms;
        }
        [DllImport(Lib)] public static extern int canvas_call_somatic(IntPtr ctx, long nbins, IntPtr dCount, int nchr, long[] chrSegOffset, int[] segBegin, int[] segEnd, long[] segBinOffset,
            long[] chrSiteOffset, IntPtr dSitePos, IntPtr dSiteRef, IntPtr dSiteAlt, int[] segRefCn, long[] chrExclOffset, int[] exclStart, int[] exclStop,
            ref canvas_somatic_call_params parameters, ref canvas_somatic_call_out output, out canvas_somatic_call_scalars scalars, out canvas_somatic_result result);

        // Partition states: the segment lengths canvas_cbs leaves on the device, or the breakpoints canvas_wavelets returns, as the per-bin state canvas_segment_ids* takes
        // (the zero-based ordinal of the bin's segment within its chromosome; -1 throughout a chromosome for which the method derives no segment).  One wait each
        [DllImport(Lib)] public static extern int canvas_partition_states_cbs(IntPtr ctx, int nchr, long[] chrOffset, IntPtr dSegLen, int[] nSeg, IntPtr dState);
        [DllImport(Lib)] public static extern int canvas_partition_states_breakpoints(IntPtr ctx, int nchr, long[] chrOffset, int[] breakpoints, long[] bpOffset, IntPtr dState);
        // PloidyInfo.GetReferenceCopyNumber per segment (host code, no context): the ploidy records in the layout of canvas_segment_ids_ploidy (ploidyOffset null: 2 everywhere)
        [DllImport(Lib)] public static extern int canvas_reference_copy_numbers(int nchr, long[] chrSegOffset, int[] segBegin, int[] segEnd, long[] ploidyOffset, int[] ploidyStart,
            int[] ploidyEnd, int[] ploidyCn, int[] segRefCn);
        // canvas_segment_tables, canvas_reference_copy_numbers, then canvas_call_somatic on the tables and float counts (dCov and dCountF32 required; the call's arrays hold capSeg entries)
        [DllImport(Lib)] public static extern int canvas_call_somatic_ids(IntPtr ctx, long nbins, int nchr, long[] chrOffset, IntPtr dStart, IntPtr dStop, IntPtr dSegmentId, IntPtr dCov, long capSeg,
            long[] chrSiteOffset, IntPtr dSitePos, IntPtr dSiteRef, IntPtr dSiteAlt, long[] ploidyOffset, int[] ploidyStart, int[] ploidyEnd, int[] ploidyCn,
            long[] chrExclOffset, int[] exclStart, int[] exclStop, ref canvas_somatic_call_params parameters,
            out long nSeg, long[] chrSegOffset, int[] segBegin, int[] segEnd, long[] segBinOffset, int[] segCi4, IntPtr dCountF32, int[] segRefCn,
            ref canvas_somatic_call_out output, out canvas_somatic_call_scalars scalars, out canvas_somatic_result result);

        /// <summary>Turns a non-zero status into the module's own failure convention (message on stderr, exit code 1).</summary>
        public static void Check(IntPtr ctx, int status, string what)
        {
            if (status == 0) return;
            throw new InvalidOperationException($"{what} failed ({status}): {Marshal.PtrToStringAnsi(canvas_last_error(ctx))}");
        }

        /// <summary>Device array with the lifetime of a using block.</summary>
        public sealed class DeviceBuffer : IDisposable
        {
            readonly IntPtr _ctx; public IntPtr Ptr { get; }
            public DeviceBuffer(IntPtr ctx, long bytes) { _ctx = ctx; Ptr = canvas_device_malloc(ctx, Math.Max(1, bytes)); if (Ptr == IntPtr.Zero) throw new OutOfMemoryException("canvas_device_malloc"); }
            public void Dispose() { canvas_device_free(_ctx, Ptr); }
        }
    }
}
