// CanvasNormalize with the GPU library: the patch to the three reference generators and the ratio step (Src/Canvas/CanvasNormalize).
// Option parsing (Program.cs), the factory, the file reading (BinCounts, CanvasIO, PCAModel.LoadModel's text parsing) and every file written stay as they are
// in the module; what each generator computes becomes one call:
//   WeightedAverageReferenceGenerator.Run, several controls (:34-68)   -> canvas_normalize_reference (weights + weighted counts; the module formats "{0}")
//   BestLR2ReferenceGenerator.Run, several controls (:31-80)           -> canvas_normalize_best_normal (index of the control the module copies)
//   PCAReferenceGenerator.Run (:32-69) + the axes check of LoadModel   -> canvas_normalize_pca_reference (the reference counts the module writes)
//   LSNormRatioCalculator / RawRatioCalculator + RatiosToCounts        -> canvas_normalize_ratio (as before, CanvasHip.cs)
// NOT COMPILED HERE (no dotnet SDK in the image); canvas_amd/tools/canvas_normalize_main.cpp is the same program in C++ and is what the tests run.
using System;
using System.Collections.Generic;
using System.Linq;
using static CanvasHipInterop.CanvasHip;

namespace CanvasNormalize
{
    static class HipNormalize
    {
        static T WithContext<T>(Func<IntPtr, T> body)
        {
            IntPtr ctx = canvas_create(0);
            if (ctx == IntPtr.Zero) throw new InvalidOperationException("no usable GPU (libcanvas_hip has no CPU fallback)");
            try { return body(ctx); } finally { canvas_destroy(ctx); }
        }

        static DeviceBuffer Upload(IntPtr ctx, double[] v) { var d = new DeviceBuffer(ctx, 8L * v.Length); Check(ctx, canvas_memcpy_h2d(ctx, d.Ptr, v, 8L * v.Length), "upload"); return d; }
        static DeviceBuffer Upload(IntPtr ctx, float[] v) { var d = new DeviceBuffer(ctx, 4L * v.Length); Check(ctx, canvas_memcpy_h2d(ctx, d.Ptr, v, 4L * v.Length), "upload"); return d; }
        static DeviceBuffer Upload(IntPtr ctx, int[] v) { var d = new DeviceBuffer(ctx, 4L * v.Length); Check(ctx, canvas_memcpy_h2d(ctx, d.Ptr, v, 4L * v.Length), "upload"); return d; }

        /// <summary>BestLR2: replaces the loops of Run between reading the BinCounts and copying the file (BestLR2ReferenceGenerator.cs:36-75).
        /// counts = BinCounts.AllCounts of the tumour and of every control (double.Parse), onTarget = BinCounts' OnTargetIndices or null.</summary>
        public static int BestNormal(List<double> tumor, List<List<double>> normals, List<int> onTarget)
        {
            return WithContext(ctx =>
            {
                var d = normals.Select(c => Upload(ctx, c.ToArray())).ToList();
                try
                {
                    using (var dt = Upload(ctx, tumor.ToArray()))
                    using (var di = onTarget == null ? null : Upload(ctx, onTarget.ToArray()))
                    {
                        Check(ctx, canvas_normalize_best_normal(ctx, dt.Ptr, d.Count, d.Select(b => b.Ptr).ToArray(), tumor.Count, di?.Ptr ?? IntPtr.Zero, onTarget?.Count ?? 0,
                                                                out int best, null, null, out int replayed), "canvas_normalize_best_normal");
                        return best;
                    }
                }
                finally { foreach (var b in d) b.Dispose(); }
            });
        }
        // In BestLR2ReferenceGenerator.Run: `if (normalSampleCount > 1) bestNormalSampleIndex = HipNormalize.BestNormal(...);` then the copy as before.

        /// <summary>PCA: the reference counts PCAReferenceGenerator.Run writes (:36-64), the sample cut to the model's length (Enumerable.Zip).
        /// Returns null when the axes are not orthogonal: PCAModel's constructor throws there ("Axes are not orthogonal to each other in {0}.").</summary>
        public static float[] PcaReference(float[] sampleCounts, float[] mu, double[][] rawAxes, double minBinCount, double maxBinCount, out double medianRatio)
        {
            double med = 0;
            var result = WithContext(ctx =>
            {
                int n = mu.Length;
                var d = rawAxes.Select(a => Upload(ctx, a)).ToList();
                try
                {
                    using (var ds = Upload(ctx, sampleCounts.Take(n).ToArray())) using (var dm = Upload(ctx, mu)) using (var dr = new DeviceBuffer(ctx, 4L * n))
                    {
                        Check(ctx, canvas_normalize_pca_reference(ctx, n, ds.Ptr, dm.Ptr, d.Count, d.Select(b => b.Ptr).ToArray(), minBinCount, maxBinCount, dr.Ptr,
                                                                  out med, null, out int orthogonal), "canvas_normalize_pca_reference");
                        if (orthogonal == 0) return null;
                        var reference = new float[n];
                        Check(ctx, canvas_memcpy_d2h(ctx, reference, dr.Ptr, 4L * n), "download");
                        return reference;
                    }
                }
                finally { foreach (var b in d) b.Dispose(); }
            });
            medianRatio = med;
            return result;
        }
        // PCAModel keeps the RAW axes (tempAxes) for this call; LoadModel's NormalizeBy2Norm + AreOrthogonal move into the library.  Run keeps VerifyBinOrder and writes
        // `new SampleGenomicBin(bin.Chromosome, bin.Start, bin.Stop, bin.GC, reference[i])` for the zipped bins with CanvasIO.WriteToTextFile; no temporary file.
    }
}
