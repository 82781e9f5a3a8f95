// CanvasSomaticCaller: what the model fit (somatic.hip) and the calls around it (call.hip) both need of one model's points, on the host.
#pragma once
#include <cmath>

static inline int som_points(int maxCN, unsigned char* cn, unsigned char* major) {       // InitializePloidies (:87-116): copyNumber up, majorCount down while 2 * majorCount >= copyNumber
    int p = 0;
    for (int c = 0; c <= maxCN; c++)
        for (int m = c; m * 2 >= c; m--, p++) { if (cn) { cn[p] = (unsigned char)c; major[p] = (unsigned char)m; } }
    return p;
}

// AdjustedMAF (:686-702) with binomP and logCombinations (:704-716); logFactorial[i] = log(i) + logFactorial[i - 1] is what the reference's growing table holds
static inline double som_adjusted_maf(double theoreticalMAcvg, double coverage, const double* logFactorial) {
    if (coverage < 1.0) return 0;
    if (theoreticalMAcvg == 0) return 0;
    const double mean = theoreticalMAcvg / coverage;
    const int n = (int)coverage;
    const double logP = log(mean), logQ = log(1 - mean);
    double meanObs = 0.0;
    for (int i = 0; i <= n; i++) {
        const double logCombinations = logFactorial[n] - logFactorial[i] - logFactorial[n - i];
        const double binomP = exp(logCombinations + i * logP + (n - i) * logQ);
        const double k = i, other = coverage - i;
        meanObs += (k <= other ? k : other) * binomP;
    }
    return meanObs / coverage;
}

